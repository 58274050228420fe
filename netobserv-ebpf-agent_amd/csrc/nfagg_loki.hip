// nfagg_loki.hip — write loki on the device (nfagg_loki.h): FlpLoki, the line policy that leaves out the keys
// the stage takes out of the line, and the kernels of a plan and of a write.
//   plan   k_loki_key      per flow: the line's length under FlpLoki (CountSink, less the newline), the timestamp of
//                          extractTimestamp (write_loki.go:253-277: a float64 product, converted, divided and normalised as
//                          time.Unix does), the stream tuple claimed in a table by the two-word claim protocol of
//                          nfagg_metrics.hip, an atomic min of the flow index per stream
//          k_loki_first / scan / k_loki_streams     dense stream ids in order of the first flow
//          scan of the lengths / k_loki_cuts        the cut rule of client.go:154-172, one wave, a wave-wide search per batch
//          k_loki_sortkey / radix sort              the stable permutation by (batch, stream)
//          k_loki_gflag / scans / k_loki_gstart / k_loki_gout     the (batch, stream) groups and their sums
//   write  k_loki_hsz / scan / k_loki_pos / k_loki_batches / k_loki_bent     header sizes, offsets of positions and batches
//          k_loki_write    output position j encodes flow perm[j] (indirect loads) into the wave image; the skeleton's window
//                          loop and copy-out (nfagg_encode.h) unchanged
//          k_loki_headers  a wave per group writes 0x0a len Stream 0x0a len labels behind the write kernel, on the same
//                          stream: a label text of up to 4 096 bytes is a wave's copy, not one lane's byte loop
// logproto (types.go:88-144, timestamp.go:59-106): Entry = 0x0a len Timestamp (always), 0x12 len line; Timestamp = 0x08
// seconds when not 0 (a negative one as ten bytes), 0x10 nanos when not 0.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include "nfagg_loki_line.h"

namespace nfagg {

using LokiPlain = LokiOver<FlpPlain>;

// ---- plan: stream ids by first flow
__global__ __launch_bounds__(256) void k_loki_first(uint64_t n, LokiPlanDev D, uint32_t* __restrict__ flag) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t s = D.slot_of[i];
    flag[i] = s != kNoSlot && D.first[s] == (uint32_t)i ? 1u : 0u;
}
__global__ __launch_bounds__(256) void k_loki_streams(uint64_t n, LokiPlanDev D, const uint32_t* __restrict__ flag, const uint32_t* __restrict__ rank,
                                                      nfagg_loki_stream* __restrict__ streams) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    if (i == n - 1) D.ctl->n_streams = rank[i] + flag[i];
    if (!flag[i]) return;
    const uint32_t s = D.slot_of[i], id = rank[i];
    D.sid[s] = id;
    if (id >= kLokiMaxStreams) return;                      // an overflowed call: the host refuses it
    const uint64_t ka = D.keys[2 * (size_t)s], kb = D.keys[2 * (size_t)s + 1];
    nfagg_loki_stream o;
    o.src_class = (uint32_t)(ka >> 23) & 0x7fffffu; o.dst_class = (uint32_t)ka & 0x7fffffu;
    o.src_label = (uint16_t)kb; o.dst_label = (uint16_t)(kb >> 16);
    o.direction = (uint8_t)(kb >> 32); o.layer = (uint8_t)((kb >> 40) & 3u); o.record_type = (uint8_t)((kb >> 42) & 1u); o.pad_ = 0;
    o.first_flow = (uint32_t)i;
    streams[id] = o;
}

// ---- plan: the cuts. pinc[j]: the line bytes of the flows 0..j that take part. The smallest j in [a, b) with pinc[j] > thr,
// or b: every lane probes one point of the range, the ballot narrows it 64-fold per step.
NF_DEV uint64_t wave_first_above(const uint64_t* __restrict__ pinc, uint64_t a, uint64_t b, uint64_t thr) {
    const uint32_t lane = threadIdx.x & 63;
    while (b - a > 64) {
        const uint64_t step = (b - a + 63) / 64;
        uint64_t q = a + (lane + 1) * step - 1;
        if (q > b - 1) q = b - 1;
        const uint64_t m = __ballot(pinc[q] > thr);
        if (!m) return b;                                   // lane 63 probed b - 1
        const uint32_t f = (uint32_t)__ffsll((long long)m) - 1;
        const uint64_t na = a + (uint64_t)f * step, nb = na + step;
        a = na; b = nb < b ? nb : b;
    }
    const uint64_t q = a + lane;
    const uint64_t m = __ballot(q < b && pinc[q] > thr);
    return m ? a + (uint32_t)__ffsll((long long)m) - 1 : b;
}
// client.go:154-172 over the flows in order: a batch starts with an entry whatever its size; the entry that would take the
// batch's line bytes over batch_size starts the next one. Sequential in where batches end; one wave.
__global__ __launch_bounds__(64) void k_loki_cuts(uint64_t n, const uint64_t* __restrict__ pinc, const uint32_t* __restrict__ lens, uint32_t batch_size,
                                                  uint32_t* __restrict__ cuts, LokiCtl* __restrict__ ctl) {
    constexpr uint64_t kNear = 4096;
    uint64_t lo = 0, thr = 0;
    uint32_t nb = 0;
    while (lo < n) {
        const uint64_t near = lo + kNear < n ? lo + kNear : n;
        uint64_t j = wave_first_above(pinc, lo, near, thr);
        if (j == near && near < n) j = wave_first_above(pinc, near, n, thr);
        if (j >= n) break;
        if (threadIdx.x == 0) cuts[nb] = (uint32_t)j;
        nb++;
        const uint64_t pj = pinc[j], full = pj - lens[j] + batch_size;
        thr = full > pj ? full : pj;                        // the next start adds bytes: a flow without a line behind an oversized first entry is none
        lo = j + 1;
    }
    if (threadIdx.x == 0) ctl->n_batches = nb;
}

__global__ __launch_bounds__(256) void k_loki_sortkey(uint64_t n, LokiPlanDev D, const uint32_t* __restrict__ cuts, uint64_t* __restrict__ key,
                                                      uint32_t* __restrict__ val) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    val[i] = (uint32_t)i;
    const uint32_t s = D.slot_of[i];
    const uint32_t nb = D.ctl->n_batches;
    if (s == kNoSlot || nb == 0) { key[i] = kLokiNoGroup; return; }
    uint32_t lo = 0, hi = nb;                               // the last cut at or before i
    while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (cuts[mid] <= (uint32_t)i) lo = mid; else hi = mid; }
    key[i] = ((uint64_t)lo << kLokiStreamBits) | (D.sid[s] & (kLokiMaxStreams - 1));
}

// ---- plan: the groups of the sorted order
__global__ __launch_bounds__(256) void k_loki_gflag(uint64_t n, LokiPlanDev D, const uint64_t* __restrict__ ks, const uint32_t* __restrict__ perm,
                                                    uint32_t* __restrict__ flag, uint32_t* __restrict__ esz) {
    const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (j > n) return;
    if (j == n) { esz[n] = 0; return; }
    const uint64_t k = ks[j];
    const bool part = k < kLokiNoGroup;
    flag[j] = part && (j == 0 || ks[j - 1] != k) ? 1u : 0u;
    uint32_t e = 0;
    if (part) { const uint64_t i = perm[j]; e = entry_size(D.rows8[i * 8 + 7], D.ts[2 * i], D.ts[2 * i + 1]); }
    esz[j] = e;
}
__global__ __launch_bounds__(256) void k_loki_gstart(uint64_t n, LokiPlanDev D, const uint64_t* __restrict__ ks, const uint32_t* __restrict__ flag,
                                                     const uint32_t* __restrict__ gidx, uint32_t* __restrict__ gs) {
    const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    if (flag[j]) gs[gidx[j] - 1] = (uint32_t)j;
    if (ks[j] < kLokiNoGroup && (j == n - 1 || ks[j + 1] >= kLokiNoGroup)) D.ctl->n_groups = gidx[j];
}
__global__ __launch_bounds__(256) void k_loki_gout(uint64_t n, LokiPlanDev D, const uint64_t* __restrict__ ks, const uint64_t* __restrict__ E,
                                                   const uint32_t* __restrict__ gs, nfagg_loki_group* __restrict__ groups) {
    const uint64_t g = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint32_t ng = D.ctl->n_groups;
    if (g >= n || g >= ng) return;
    const uint32_t a = gs[g], b = g + 1 < ng ? gs[g + 1] : D.ctl->n_part;
    const uint64_t k = ks[a];
    nfagg_loki_group o;
    o.batch = (uint32_t)(k >> kLokiStreamBits); o.stream = (uint32_t)k & (kLokiMaxStreams - 1); o.n_entries = b - a; o.pad_ = 0;
    o.entry_bytes = E[b] - E[a];
    groups[g] = o;
}

// ---- a 64-bit prefix sum of 32-bit values, by the skeleton's own two levels (nfagg_encode.h): block_scan inside 1 024 values, the
// one-workgroup scan of the block sums, then block base + local offset written out wide. (A library scan over 64-bit values keeps
// its look-back state in 16-byte write-through stores, which tests/test_isa_pins.py reserves for ast16.)
__global__ __launch_bounds__(kScanBlock) void k_loki_scan(const uint32_t* __restrict__ in, uint64_t count, uint32_t* __restrict__ local_off,
                                                          uint32_t* __restrict__ block_sum) {
    __shared__ uint32_t wave_tot[kScanBlock / 64];
    const uint64_t i = (uint64_t)blockIdx.x * kScanBlock + threadIdx.x;
    block_scan(i < count ? in[i] : 0u, i, count, wave_tot, local_off, block_sum);
}
__global__ __launch_bounds__(256) void k_loki_widen(const uint32_t* __restrict__ in, uint64_t count, const uint32_t* __restrict__ local_off,
                                                    const uint64_t* __restrict__ block_base, uint32_t inclusive, uint64_t* __restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < count) out[i] = record_off(block_base, local_off, i) + (inclusive ? in[i] : 0u);
}
static hipError_t loki_scan64(const uint32_t* d_in, uint64_t count, bool inclusive, uint64_t* d_out, const LokiScan& X, hipStream_t s) {
    const uint32_t blocks = (uint32_t)((count + kScanBlock - 1) / kScanBlock);
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_loki_scan, dim3(blocks), dim3(kScanBlock), 0, s, d_in, count, X.local_off, X.block_sum);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if ((e = launch_scan_block_sums(X.block_sum, blocks, X.block_base, s)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_loki_widen, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s, d_in, count, (const uint32_t*)X.local_off,
                       (const uint64_t*)X.block_base, inclusive ? 1u : 0u, d_out);
    return hipGetLastError();
}

template <typename Kernel, typename... Args> static hipError_t launch256(Kernel k, uint64_t threads, hipStream_t s, Args... args) {
    (void)hipGetLastError();
    hipLaunchKernelGGL(k, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, args...);
    return hipGetLastError();
}

size_t loki_tmp_bytes(uint64_t n) {
    size_t need = 0, b = 0;
    const int m = (int)(n + 1);
    hipcub::DeviceScan::ExclusiveSum((void*)nullptr, b, (const uint32_t*)nullptr, (uint32_t*)nullptr, m); need = b > need ? b : need;
    hipcub::DeviceScan::InclusiveSum((void*)nullptr, b, (const uint32_t*)nullptr, (uint32_t*)nullptr, m); need = b > need ? b : need;
    hipcub::DeviceRadixSort::SortPairs((void*)nullptr, b, (const uint64_t*)nullptr, (uint64_t*)nullptr, (const uint32_t*)nullptr, (uint32_t*)nullptr, m, 0, 53);
    need = b > need ? b : need;
    return need + 256;
}

// The policy a call selects, as the direct-FLP launchers do: no parts the plain line (here), else nfagg_flp_content.hip's.
hipError_t launch_loki_key(const FlpLineArgs& A, bool content, const LokiDev& L, const LokiPlanDev& D, hipStream_t s) {
    return content ? launch_loki_key_content(A, L, D, s) : loki_key_as<LokiPlain>(A, L, D, s);
}

hipError_t launch_loki_rank(uint64_t n, const LokiPlanDev& D, uint32_t* d_flag, uint32_t* d_rank, nfagg_loki_stream* d_streams, void* d_tmp,
                            size_t tmp_bytes, hipStream_t s) {
    hipError_t e = launch256(k_loki_first, n, s, n, D, d_flag);
    if (e != hipSuccess) return e;
    if ((e = hipcub::DeviceScan::ExclusiveSum(d_tmp, tmp_bytes, (const uint32_t*)d_flag, d_rank, (int)n, s)) != hipSuccess) return e;
    return launch256(k_loki_streams, n, s, n, D, (const uint32_t*)d_flag, (const uint32_t*)d_rank, d_streams);
}

hipError_t launch_loki_cuts(uint64_t n, const LokiPlanDev& D, uint64_t* d_pinc, uint32_t batch_size, uint32_t* d_cuts, const LokiScan& X, hipStream_t s) {
    hipError_t e = loki_scan64(D.lens, n, true, d_pinc, X, s);
    if (e != hipSuccess) return e;
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_loki_cuts, dim3(1), dim3(64), 0, s, n, (const uint64_t*)d_pinc, (const uint32_t*)D.lens, batch_size, d_cuts, D.ctl);
    return hipGetLastError();
}

hipError_t launch_loki_sort(uint64_t n, const LokiPlanDev& D, const uint32_t* d_cuts, uint64_t* d_key, uint64_t* d_key_sorted, uint32_t* d_val,
                            uint32_t* d_perm, void* d_tmp, size_t tmp_bytes, hipStream_t s) {
    hipError_t e = launch256(k_loki_sortkey, n, s, n, D, d_cuts, d_key, d_val);
    if (e != hipSuccess) return e;
    return hipcub::DeviceRadixSort::SortPairs(d_tmp, tmp_bytes, (const uint64_t*)d_key, d_key_sorted, (const uint32_t*)d_val, d_perm, (int)n, 0, 53, s);
}

hipError_t launch_loki_groups(uint64_t n, const LokiPlanDev& D, const uint64_t* d_key_sorted, const uint32_t* d_perm, uint32_t* d_flag,
                              uint32_t* d_gidx, uint32_t* d_esz, uint64_t* d_E, uint32_t* d_gs, nfagg_loki_group* d_groups, void* d_tmp,
                              size_t tmp_bytes, const LokiScan& X, hipStream_t s) {
    hipError_t e = launch256(k_loki_gflag, n + 1, s, n, D, d_key_sorted, d_perm, d_flag, d_esz);
    if (e != hipSuccess) return e;
    if ((e = hipcub::DeviceScan::InclusiveSum(d_tmp, tmp_bytes, (const uint32_t*)d_flag, d_gidx, (int)n, s)) != hipSuccess) return e;
    if ((e = loki_scan64(d_esz, n + 1, false, d_E, X, s)) != hipSuccess) return e;
    if ((e = launch256(k_loki_gstart, n, s, n, D, d_key_sorted, (const uint32_t*)d_flag, (const uint32_t*)d_gidx, d_gs)) != hipSuccess) return e;
    return launch256(k_loki_gout, n, s, n, D, d_key_sorted, (const uint64_t*)d_E, (const uint32_t*)d_gs, d_groups);
}

// ---- write: sizes and offsets. A group's header: 0x0a len Stream, 0x0a len labels, the labels.
__global__ __launch_bounds__(256) void k_loki_hsz(uint32_t ng, LokiWriteDev W) {
    const uint32_t g = blockIdx.x * 256 + threadIdx.x;
    if (g > ng) return;
    if (g == ng) { W.hsz[g] = 0; return; }
    const nfagg_loki_group q = W.groups[g];
    const uint32_t lab = W.lab_off[q.stream + 1] - W.lab_off[q.stream];
    const uint64_t slen = 1 + vlen(lab) + lab + q.entry_bytes;
    W.hsz[g] = 1 + vlen(slen) + 1 + vlen(lab) + lab;
}
// where position j starts (its group's header included when it is the group's first)
NF_DEV uint64_t loki_pos_start(const LokiWriteDev& W, uint32_t j) {
    const uint32_t g = W.gidx[j] - 1;
    return W.E[j] + W.H[g] + (W.flag[j] ? 0u : W.hsz[g]);
}
__global__ __launch_bounds__(256) void k_loki_pos(uint32_t m, uint32_t ng, LokiWriteDev W) {
    const uint32_t j = blockIdx.x * 256 + threadIdx.x;
    if (j >= m) return;
    const uint32_t jb = j / kScanBlock * kScanBlock;
    const uint64_t start = loki_pos_start(W, j), sb = loki_pos_start(W, jb);
    W.local_off[j] = (uint32_t)(start - sb);
    if (j == jb) W.block_base[j / kScanBlock] = start;
    if (j == m - 1) W.block_base[(m + kScanBlock - 1) / kScanBlock] = W.E[m] + W.H[ng];
}
__global__ __launch_bounds__(256) void k_loki_batches(uint32_t m, uint32_t ng, uint32_t nb, LokiWriteDev W, uint64_t* __restrict__ batch_offsets) {
    const uint32_t g = blockIdx.x * 256 + threadIdx.x;
    if (g >= ng) return;
    if (g == 0) { W.bpos[nb] = m; batch_offsets[nb] = W.E[m] + W.H[ng]; }
    const uint32_t b = W.groups[g].batch;
    if (b < nb && (g == 0 || W.groups[g - 1].batch != b)) { W.bpos[b] = W.gs[g]; batch_offsets[b] = W.E[W.gs[g]] + W.H[g]; }
}
__global__ __launch_bounds__(256) void k_loki_bent(uint32_t nb, LokiWriteDev W, uint32_t* __restrict__ batch_entries) {
    const uint32_t b = blockIdx.x * 256 + threadIdx.x;
    if (b < nb) batch_entries[b] = W.bpos[b + 1] - W.bpos[b];
}

hipError_t launch_loki_offsets(uint32_t m, uint32_t n_groups, uint32_t n_batches, const LokiWriteDev& W, uint64_t* d_batch_offsets,
                               uint32_t* d_batch_entries, const LokiScan& X, hipStream_t s) {
    hipError_t e = launch256(k_loki_hsz, (uint64_t)n_groups + 1, s, n_groups, W);
    if (e != hipSuccess) return e;
    if ((e = loki_scan64(W.hsz, (uint64_t)n_groups + 1, false, W.H, X, s)) != hipSuccess) return e;
    if ((e = launch256(k_loki_pos, m, s, m, n_groups, W)) != hipSuccess) return e;
    if ((e = launch256(k_loki_batches, n_groups, s, m, n_groups, n_batches, W, d_batch_offsets)) != hipSuccess) return e;
    return launch256(k_loki_bent, n_batches, s, n_batches, W, d_batch_entries);
}

__global__ __launch_bounds__(64) void k_loki_headers(uint32_t ng, LokiWriteDev W, uint8_t* __restrict__ out) {
    const uint32_t g = blockIdx.x;
    if (g >= ng) return;
    const nfagg_loki_group q = W.groups[g];
    const uint32_t l0 = W.lab_off[q.stream], lab = W.lab_off[q.stream + 1] - l0;
    const uint64_t slen = 1 + vlen(lab) + lab + q.entry_bytes;
    uint8_t* p = out + W.E[W.gs[g]] + W.H[g];
    const uint32_t head = 1 + vlen(slen) + 1 + vlen(lab);
    if (threadIdx.x == 0) {
        uint8_t* o = p;
        *o++ = 0x0a; o = put_varint(o, slen); *o++ = 0x0a; put_varint(o, lab);
    }
    for (uint32_t k = threadIdx.x; k < lab; k += 64) p[head + k] = W.labels[l0 + k];
}

hipError_t launch_loki_write(const FlpLineArgs& A, bool content, const LokiDev& L, const LokiPlanDev& D, const LokiWriteDev& W, uint32_t m, uint32_t n_groups,
                             uint8_t* d_out, hipStream_t s) {
    hipError_t e = content ? launch_loki_write_content(A, L, D, W, m, d_out, s) : loki_write_as<LokiPlain>(A, L, D, W, m, d_out, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_loki_headers, dim3(n_groups), dim3(64), 0, s, n_groups, W, d_out);
    return hipGetLastError();
}

uint32_t loki_max_entry(int policy) { return policy == 0 ? LokiPlain::kMaxEntry : loki_max_entry_content(policy); }

}  // namespace nfagg
