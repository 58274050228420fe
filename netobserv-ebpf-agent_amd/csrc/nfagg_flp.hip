// nfagg_flp.hip — evicted flow_record_t -> direct-FLP JSON lines, in bulk on the GPU. Replaces, for the records
// Accounter.evict produces,
//   pkg/model/record.go:82-114             NewRecord (flow start/end wall-clock times, the interface list)
//   pkg/decode/decode_protobuf.go:57-127   RecordToMap, the keys a BpfFlowMetrics-only record produces
//   flowlogs-pipeline write_stdout.go:37-51 with `format: json`, `reorder: true`:
//   jsoniter.Config{SortMapKeys: true}.Marshal(map) + "\n"
// Output: line i = out[line_offsets[i], line_offsets[i + 1]), '\n' included. A record whose TLS version, cipher suite or
// key share is set needs Go's crypto/tls name tables: its line is empty and it is flagged as deferred.
//
// Keys in byte order (what jsoniter's sorted map encoder gives), [] = only when the rule of RecordToMap says so:
//   AgentIP [Bytes] [Dscp] [DstAddr] DstMac [DstPort] Etype [Flags] [IcmpCode] [IcmpType] IfDirections Interfaces
//   [Packets] [Proto] [Sampling] [SrcAddr] SrcMac [SrcPort] [TLSTypes] TimeFlowEndMs TimeFlowStartMs TimeReceived Udns
//
// The two-pass skeleton of nfagg_encode.h. One encoder
// (encode_line) serves both passes: over a counting sink it adds digit counts (compares against powers of ten) and the
// escaped names' lengths, it never forms a digit or touches a name's bytes. Names and UDNs come escaped and quoted
// from the table the host escaped once per call. A wave writes its 64 lines into an LDS window of kFlpWindow bytes at
// their final relative positions and copies the window out with aligned 16-byte stores; 64 typical lines (~26 KB) fit
// one window. The window is bounded (32 KiB of LDS whatever the lines' lengths): a longer range takes several windows,
// each starting at a line start, so a line (at most kFlpMaxLine bytes) is written whole, once, through a plain pointer.
#include "nfagg_flp_line.h"

namespace nfagg {

constexpr uint32_t kFlpWindow = 28672;                       // line starts a window takes, from its aligned base
constexpr uint32_t kFlpLds = kFlpWindow + (kFlpMaxLine + 15) / 16 * 16;
static_assert(kFlpLds <= 32768, "four waves per compute unit");

// ---- kernel 1: line length per record (the seven interface rows resolved once), block-local exclusive scan
__global__ __launch_bounds__(kScanBlock) void k_flp_size(const void* __restrict__ recs, uint64_t n, FlpParams P,
                                                         uint32_t* __restrict__ rows, uint32_t* __restrict__ local_off,
                                                         uint32_t* __restrict__ block_sum, uint32_t* __restrict__ n_deferred) {
    __shared__ uint32_t wave_tot[kScanBlock / 64];
    __shared__ uint32_t tab_lds[kNamesLdsRows * (kNameRowBytes / 4)];
    const uint8_t* tab = stage_names<kScanBlock>(P.names, P.n_names, tab_lds);
    const uint64_t i = (uint64_t)blockIdx.x * kScanBlock + threadIdx.x;
    uint32_t len = 0;
    bool deferred = false;
    if (i < n) {
        Rec r;
        load_record(recs, i, r);
        uint32_t row[7];
        flp_rows(tab, P.n_names, r, row);
        deferred = flp_deferred(r);
        if (!deferred) { CountSink c; encode_line(c, r, P, row); len = c.n; }
        uint4* o = reinterpret_cast<uint4*>(rows + i * 8);
        o[0] = make_uint4(row[0], row[1], row[2], row[3]);
        o[1] = make_uint4(row[4], row[5], row[6], len);
    }
    const int lane = threadIdx.x & 63;
    const uint64_t dm = __ballot(deferred);
    if (lane == 0 && dm) atomicAdd(n_deferred, (uint32_t)__popcll(dm));
    block_scan(len, i, n, wave_tot, local_off, block_sum);
}

// ---- kernel 3: write. One wave per 64 consecutive records; their lines are contiguous in the output. The wave moves a
// window along its byte range [shift, span) of the image: a window starts at a line start `lo`, takes every line that
// starts less than kFlpWindow bytes behind its 16-byte aligned base, and ends where the last of them ends, so a line is
// always written whole (the buffer has kFlpMaxLine bytes of slack) and exactly once.
__global__ __launch_bounds__(64) void k_flp_write(const void* __restrict__ recs, uint64_t n, FlpParams P,
                                                  const uint32_t* __restrict__ rows, const uint32_t* __restrict__ local_off,
                                                  const uint64_t* __restrict__ block_base, uint8_t* __restrict__ out,
                                                  uint64_t* __restrict__ line_offsets, uint8_t* __restrict__ deferred) {
    __shared__ __align__(16) uint8_t lds[kFlpLds];
    const uint64_t i0 = (uint64_t)blockIdx.x * 64, i = i0 + threadIdx.x;
    WaveImage w(block_base, local_off, i0);
    uint64_t my_off = 0; uint32_t my_len = 0;
    uint32_t row[7] = {};
    Rec r;
    if (i < n) {
        load_record(recs, i, r);
        const uint4* q = reinterpret_cast<const uint4*>(rows + i * 8);
        const uint4 a = q[0], b = q[1];
        row[0] = a.x; row[1] = a.y; row[2] = a.z; row[3] = a.w; row[4] = b.x; row[5] = b.y; row[6] = b.z;
        my_len = b.w;
        my_off = record_off(block_base, local_off, i);
        line_offsets[i] = my_off;
        if (i == n - 1) line_offsets[n] = my_off + my_len;
        if (deferred) deferred[i] = my_len == 0 ? 1 : 0;     // every line that is written has at least its braces
    }
    w.close(my_off + my_len, out);
    const uint32_t p0 = w.pos(my_off);                            // my line = image bytes [p0, p0 + my_len)
    uint32_t lo = w.shift;
    while (lo < w.span) {
        const uint32_t base = lo & ~15u;
        const bool mine = my_len && p0 >= lo && p0 - base < kFlpWindow;
        if (mine) { FlpLds s{lds + (p0 - base)}; encode_line(s, r, P, row); }
        uint32_t hi = mine ? p0 + my_len : lo;                  // the window's end: at most base + kFlpWindow + kFlpMaxLine
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) { const uint32_t o = __shfl_xor(hi, d, 64); hi = o > hi ? o : hi; }
        __syncthreads();
        copy_image_out(w.dst, lds, base, lo, hi);
        __syncthreads();
        lo = hi;
    }
}

hipError_t launch_flp_size(const void* d_recs, uint64_t n, const FlpParams& P, uint32_t* d_rows, uint32_t* d_local_off,
                           uint32_t* d_block_sum, uint64_t* d_block_base, uint32_t* d_n_deferred, hipStream_t s) {
    const uint32_t blocks = (uint32_t)((n + kScanBlock - 1) / kScanBlock);
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_flp_size, dim3(blocks), dim3(kScanBlock), 0, s, d_recs, n, P, d_rows, d_local_off, d_block_sum, d_n_deferred);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_scan_block_sums(d_block_sum, blocks, d_block_base, s);
}

hipError_t launch_flp_write(const void* d_recs, uint64_t n, const FlpParams& P, const uint32_t* d_rows, const uint32_t* d_local_off,
                            const uint64_t* d_block_base, void* d_out, uint64_t* d_line_offsets, uint8_t* d_deferred, hipStream_t s) {
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_flp_write, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, s, d_recs, n, P, d_rows, d_local_off, d_block_base,
                       (uint8_t*)d_out, d_line_offsets, d_deferred);
    return hipGetLastError();
}

}  // namespace nfagg
