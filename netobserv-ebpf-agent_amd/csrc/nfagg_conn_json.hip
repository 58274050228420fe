// nfagg_conn_json.hip — extract conntrack's conversation records (newConnection, endConnection, heartbeat) as JSON lines, on
// the shared skeleton of the export encoders (nfagg_encode.h): a size kernel with the block scan, a write kernel with the wave
// image, one encode_conn_line for the counting and the LDS sink. A line's columns come from a layout's column program
// (nfagg_conn_json.h), walked by every lane alike: the program is the same for the whole wave and arrives through the scalar
// cache. Keys come from the carrier record, the Kubernetes blocks and subnet labels from the carrier's rows as FlpK8s / FlpNet
// write them for a flow with the same addresses, everything else from the conversation's nfagg_conn_values. There is never a
// FlowDirection (a conversation has no AgentIP) and no Flags. A conversation with an aggregate column of magnitude >= 2^53
// gets no line and is flagged: above that jsoniter's WriteFloat64 needs a shortest-float printer.
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "nfagg_internal.h"
#include "nfagg_conn_json.h"
#include "nfagg_flp_line.h"
#include "nfagg_tls.h"
#include "nfagg_conn_meta.h"

namespace nfagg {

using ConnBlocks = FlpNet<FlpK8s<FlpTls<FlpPlain>>>;       // only its Kubernetes and subnet hooks are called
constexpr uint32_t kConnWindow = 16384, kConnLds = kConnWindow + kConnLineCap;
static_assert(kConnLds + 16 <= 32768, "four waves per compute unit");
static_assert(sizeof(nfagg_conn_values) == 256 && sizeof(nfagg_conn_snapshot) == 80 && offsetof(nfagg_conn_values, first) == 80 &&
              offsetof(nfagg_conn_values, last) == 160 && offsetof(nfagg_conn_snapshot, n_dirs) == 52 && sizeof(nfagg_conn_field) == 16, "conversation ABI");
constexpr uint64_t kConnExact = 1ull << 53;                // below it a float64 integer prints as its decimal digits

// n bytes of a constant text chosen at run time: one store loop behind the choice, where a lit() per arm was miscompiled (see lit)
template <typename S> NF_DEV void put_text(S& s, const char* t, uint32_t n) {
    if constexpr (is_count<S>::value) s.n += n;
    else for (uint32_t k = 0; k < n; k++) s.put((uint8_t)t[k]);
}

// One line; returns whether the conversation is deferred (its bytes are then not used). v: the conversation's nfagg_conn_values.
// Every column writes ,"name":value; the caller turns the line's first comma into the opening brace.
template <typename S>
NF_DEV bool encode_conn_line(S& s, const Rec& r, const uint8_t* __restrict__ v, const ConnLayoutDev& L, const ConnBlocks& f) {
    enum { kAddr, kUint, kMac, kI64, kDirs, kHashId, kIsFirst, kRecordType };
    bool deferred = false;
    for (uint32_t c = 0; c < L.n_cols; c++) {
        const ConnCol col = L.cols[c];
        const uint32_t a = col.arg & 0xffu, b = col.arg >> 8;
        if (col.kind == kConnColBlock) {
            if (a == 0) f.k8s_dst(s); else if (a == 1) f.dst_subnet(s); else if (a == 2) f.k8s_layer(s); else if (a == 3) f.k8s_src(s); else f.src_subnet(s);
            continue;
        }
        uint32_t what = kUint, u = 0, w[4] = {};
        uint64_t q = 0;
        if (col.kind == kConnColAgg) {                      // float64 in the reference: omitted when zero
            if (a <= 2) {
                const uint64_t* p = reinterpret_cast<const uint64_t*>(v + 16 + 16 * a);
                const uint64_t ab = p[0], ba = p[1];
                q = b == 0 ? ab + ba : b == 1 ? ab : ba;
                if ((b == 0 && (ab >= kConnExact || ba >= kConnExact)) || q >= kConnExact) { deferred = true; continue; }
            } else {
                q = *reinterpret_cast<const uint64_t*>(v + 64 + 8 * (a - 3));
                const uint64_t mag = (int64_t)q < 0 ? 0ull - q : q;
                if (mag >= kConnExact) { deferred = true; continue; }
            }
            if (!q) continue;
            what = kI64;
        } else if (col.kind == kConnColKey) {
            if (a <= 1) { what = kAddr; for (int k = 0; k < 4; k++) w[k] = r.d[4 * a + k]; }
            else u = a == 2 ? r.d[8] & 0xffffu : a == 3 ? r.d[8] >> 16 : r.d[9] & 0xffu;
        } else if (col.kind == kConnColMeta) {
            what = a == 0 ? kHashId : a == 1 ? kIsFirst : kRecordType;
            if (a == 0) q = *reinterpret_cast<const uint64_t*>(v); else u = a == 1 ? v[9] : v[8];
        } else {                                            // a snapshot's value, written even when 0
            const uint32_t* sw = reinterpret_cast<const uint32_t*>(v + 80 + 80 * (b ? 1 : 0));
            switch (a) {
            case NFAGG_CONN_IN_SRC_ADDR: what = kAddr; for (int k = 0; k < 4; k++) w[k] = sw[k]; break;
            case NFAGG_CONN_IN_DST_ADDR: what = kAddr; for (int k = 0; k < 4; k++) w[k] = sw[4 + k]; break;
            case NFAGG_CONN_IN_SRC_PORT: u = sw[8] & 0xffffu; break;
            case NFAGG_CONN_IN_DST_PORT: u = sw[8] >> 16; break;
            case NFAGG_CONN_IN_ETYPE: u = sw[9] & 0xffffu; break;
            case NFAGG_CONN_IN_PROTO: u = (sw[9] >> 16) & 0xffu; break;
            case NFAGG_CONN_IN_DSCP: u = sw[9] >> 24; break;
            case NFAGG_CONN_IN_SRC_MAC: what = kMac; q = (uint64_t)sw[10] | ((uint64_t)(sw[11] & 0xffffu) << 32); break;
            case NFAGG_CONN_IN_DST_MAC: what = kMac; q = (uint64_t)(sw[11] >> 16) | ((uint64_t)sw[12] << 16); break;
            case NFAGG_CONN_IN_TIME_START: what = kI64; q = (uint64_t)sw[16] | ((uint64_t)sw[17] << 32); break;
            case NFAGG_CONN_IN_TIME_END: what = kI64; q = (uint64_t)sw[18] | ((uint64_t)sw[19] << 32); break;
            default: what = kDirs; u = sw[13]; q = sw[14]; break;      // n_dirs @52, dirs @53..59
            }
        }
        put_blob(s, L.blob + col.frag_off, col.frag_len);
        switch (what) {
        case kAddr: s.put('"'); ip_text(s, Ip4w{{w[0], w[1], w[2], w[3]}}); s.put('"'); break;
        case kUint: dec<5>(s, u); break;
        case kMac: s.put('"'); mac_text(s, q); s.put('"'); break;
        case kI64: dec_i64(s, (int64_t)q); break;
        case kDirs: {
            const uint64_t dirs = (uint64_t)(u >> 8) | (q << 24);         // seven bytes
            const uint32_t nd = (u & 0xffu) > 7 ? 7 : u & 0xffu;
            s.put('[');
            for (uint32_t k = 0; k < nd; k++) { if (k) s.put(','); dec<3>(s, (uint32_t)(dirs >> (8 * k)) & 0xffu); }
            s.put(']');
            break; }
        case kHashId: s.put('"'); hex_u64(s, q); s.put('"'); break;
        case kIsFirst: put_text(s, u ? "true" : "false", u ? 4u : 5u); break;
        default:
            put_text(s, u == NFAGG_CONN_RECORD_NEW ? "\"newConnection\"" : u == NFAGG_CONN_RECORD_END ? "\"endConnection\"" : "\"heartbeat\"", u <= NFAGG_CONN_RECORD_END ? 15u : 11u);
            break;
        }
    }
    lit(s, "}\n");
    return deferred;
}

__global__ __launch_bounds__(kScanBlock) void k_conn_json_size(const void* __restrict__ carriers, const uint8_t* __restrict__ values, uint64_t n, ConnLayoutDev L,
                                                               K8sDev K, NetDev N, const uint32_t* __restrict__ k8s_rows, const uint2* __restrict__ net_rows,
                                                               uint32_t* __restrict__ lens, uint32_t* __restrict__ local_off,
                                                               uint32_t* __restrict__ block_sum, uint32_t* __restrict__ n_deferred) {
    __shared__ uint32_t wave_tot[kScanBlock / 64];
    const uint64_t i = (uint64_t)blockIdx.x * kScanBlock + threadIdx.x;
    uint32_t len = 0;
    bool deferred = false;
    if (i < n) {
        Rec r;
        load_record(carriers, i, r);
        ConnBlocks f;
        f.load_k8s(K, k8s_rows, i);
        f.load_net(N, net_rows, i);
        CountSink c;
        deferred = encode_conn_line(c, r, values + i * sizeof(nfagg_conn_values), L, f);
        len = deferred ? 0u : c.n;
        lens[i] = len;
    }
    const uint64_t dm = __ballot(deferred);
    if ((threadIdx.x & 63) == 0 && dm) atomicAdd(n_deferred, (uint32_t)__popcll(dm));
    block_scan(len, i, n, wave_tot, local_off, block_sum);
}

__global__ __launch_bounds__(64) void k_conn_json_write(const void* __restrict__ carriers, const uint8_t* __restrict__ values, uint64_t n, ConnLayoutDev L, K8sDev K,
                                                        NetDev N, const uint32_t* __restrict__ k8s_rows, const uint2* __restrict__ net_rows,
                                                        const uint32_t* __restrict__ lens, const uint32_t* __restrict__ local_off,
                                                        const uint64_t* __restrict__ block_base, uint8_t* __restrict__ out,
                                                        uint64_t* __restrict__ line_offsets, uint8_t* __restrict__ deferred) {
    __shared__ __align__(16) uint8_t lds[kConnLds];
    const uint64_t i0 = (uint64_t)blockIdx.x * 64, i = i0 + threadIdx.x;
    WaveImage w(block_base, local_off, i0);
    uint64_t my_off = 0; uint32_t my_len = 0;
    Rec r;
    ConnBlocks f;
    if (i < n) {
        load_record(carriers, i, r);
        my_len = lens[i];                                         // 0: deferred, whose rows are not read
        if (my_len) { f.load_k8s(K, k8s_rows, i); f.load_net(N, net_rows, i); }
        my_off = record_off(block_base, local_off, i);
        line_offsets[i] = my_off;
        if (i == n - 1) line_offsets[n] = my_off + my_len;
        if (deferred) deferred[i] = my_len == 0 ? 1 : 0;
    }
    w.close(my_off + my_len, out);
    const uint32_t p0 = w.pos(my_off);                            // my line = image bytes [p0, p0 + my_len)
    uint32_t lo = w.shift;
    while (lo < w.span) {                                         // the window loop of k_flp_write
        const uint32_t base = lo & ~15u;
        const bool mine = my_len && p0 >= lo && p0 - base < kConnWindow;
        if (mine) {
            FlpLds s{lds + (p0 - base)};
            encode_conn_line(s, r, values + i * sizeof(nfagg_conn_values), L, f);
            lds[p0 - base] = '{';                                 // the first column's comma
        }
        uint32_t hi = mine ? p0 + my_len : lo;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) { const uint32_t o = __shfl_xor(hi, d, 64); hi = o > hi ? o : hi; }
        __syncthreads();
        copy_image_out(w.dst, lds, base, lo, hi);
        __syncthreads();
        lo = hi;
    }
}

hipError_t launch_conn_json_size(const void* d_carriers, const void* d_values, uint64_t n, const ConnLayoutDev& L, const K8sDev& K, const NetDev& N,
                                 const uint32_t* d_k8s_rows, const uint2* d_net_rows, uint32_t* d_lens, uint32_t* d_local_off, uint32_t* d_block_sum,
                                 uint64_t* d_block_base, uint32_t* d_n_deferred, hipStream_t s) {
    const uint32_t blocks = (uint32_t)((n + kScanBlock - 1) / kScanBlock);
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_conn_json_size, dim3(blocks), dim3(kScanBlock), 0, s, d_carriers, (const uint8_t*)d_values, n, L, K, N, d_k8s_rows, d_net_rows, d_lens,
                       d_local_off, d_block_sum, d_n_deferred);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_scan_block_sums(d_block_sum, blocks, d_block_base, s);
}

hipError_t launch_conn_json_write(const void* d_carriers, const void* d_values, uint64_t n, const ConnLayoutDev& L, const K8sDev& K, const NetDev& N,
                                  const uint32_t* d_k8s_rows, const uint2* d_net_rows, const uint32_t* d_lens, const uint32_t* d_local_off,
                                  const uint64_t* d_block_base, void* d_out, uint64_t* d_line_offsets, uint8_t* d_deferred, hipStream_t s) {
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_conn_json_write, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, s, d_carriers, (const uint8_t*)d_values, n, L, K, N, d_k8s_rows,
                       d_net_rows, d_lens, d_local_off, d_block_base, (uint8_t*)d_out, d_line_offsets, d_deferred);
    return hipGetLastError();
}

}  // namespace nfagg
