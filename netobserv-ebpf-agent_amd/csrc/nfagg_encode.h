// nfagg_encode.h — device pieces the export encoders share (nfagg_pb.hip: protobuf, nfagg_ipfix.hip: IPFIX,
// nfagg_flp.hip: direct-FLP JSON): byte sinks, the flow's wall-clock time, the interface-namer lookup and its LDS
// staging, address words, and the two-pass skeleton around the per-format code: the size kernels'
// block scan, the write kernels' wave image and its copy-out.
#pragma once
#include "nfagg_device.h"

namespace nfagg {

// ---- byte sinks: one counts, one writes (LDS or global bytes)
struct CountSink {
    uint32_t n = 0;
    NF_DEV void put(uint8_t) { n++; }
};
// Writes only the bytes whose position (relative to the wave's LDS image) falls into [lo, lo + len):
// a frame that straddles two windows is encoded once per window.
struct WindowSink {
    uint8_t* lds;      // window base
    uint32_t pos;      // position of the next byte in the wave image
    uint32_t lo, len;
    NF_DEV void put(uint8_t b) { const uint32_t k = pos - lo; if (k < len) lds[k] = b; pos++; }
};

// A 16-byte address as four little-endian dwords in registers, never as a byte pointer: a byte loop over global
// memory is one exposed load latency per byte.
struct Ip4w { uint32_t w[4]; };
NF_DEV uint8_t ip_byte(const Ip4w& a, int k) { return (uint8_t)(a.w[k >> 2] >> (8 * (k & 3))); }
// net.IP.To4() != nil: ten zero bytes, ff ff (::ffff:a.b.c.d)
NF_DEV bool ip_v4_mapped(const Ip4w& a) { return (a.w[0] | a.w[1]) == 0 && a.w[2] == 0xffff0000u; }
// model.AllZeroIP (record.go:233-238): all zero, or ::ffff:0.0.0.0
NF_DEV bool ip_all_zero(const Ip4w& a) { return (a.w[0] | a.w[1] | a.w[3]) == 0 && (a.w[2] == 0 || a.w[2] == 0xffff0000u); }

// currentTime.Add(-Duration(mono_now - ts)) (record.go:90-97) as time.Time's (sec, nsec), 0 <= nsec < 1e9.
// now_sec / now_nsec: currentTime, normalised.
struct TimeParts { int64_t sec, nsec; };
NF_DEV TimeParts flow_time(int64_t now_sec, int64_t now_nsec, uint64_t mono_now, uint64_t ts) {
    const int64_t delta = (int64_t)(mono_now - ts);
    const int64_t d = (int64_t)(0ull - (uint64_t)delta);
    int64_t dsec = d / 1000000000ll, nsec = now_nsec + d % 1000000000ll;   // time.Time.Add
    if (nsec >= 1000000000ll) { dsec++; nsec -= 1000000000ll; } else if (nsec < 0) { dsec--; nsec += 1000000000ll; }
    return TimeParts{now_sec + dsec, nsec};
}

// interfaceNamer(ifIndex, mac) + udnsCache lookup, as a table: exact (index, MAC) row first,
// then the first row of that index that matches any MAC; no row -> the "unknown" name, no UDN. The host hands the
// table over STABLY SORTED by if_index (rows of one index keep their order, so the answer is that of a scan in table
// order): binary search for the first row of the index, then only that index's rows. `tab` is a flat pointer: the
// kernels stage the table in LDS when it fits (kNamesLdsRows rows), so a lookup costs LDS latencies, not HBM ones.
// Row layout (nfagg_intf_name, 92 bytes): if_index@0 mac@4 has_mac@10 name_len@11 name@12 udn_len@28 udn@29.
constexpr uint32_t kNameRowBytes = sizeof(nfagg_intf_name);
constexpr uint32_t kNamesLdsRows = 96;
static_assert(kNameRowBytes == 92 && kNameRowBytes % 4 == 0, "nfagg_intf_name layout");
NF_DEV const uint8_t* lookup_name(const uint8_t* tab, uint32_t n_names, uint32_t if_index, uint64_t mac48) {
    uint32_t lo = 0, hi = n_names;
    while (lo < hi) {                                   // first row with if_index >= the one looked for
        const uint32_t mid = (lo + hi) >> 1;
        if (*reinterpret_cast<const uint32_t*>(tab + (size_t)mid * kNameRowBytes) < if_index) lo = mid + 1; else hi = mid;
    }
    const uint8_t* any = nullptr;
    for (uint32_t k = lo; k < n_names; k++) {
        const uint8_t* e = tab + (size_t)k * kNameRowBytes;
        const uint32_t* p = reinterpret_cast<const uint32_t*>(e);
        const uint32_t w0 = p[0], w1 = p[1], w2 = p[2];
        if (w0 != if_index) break;
        if ((w2 >> 16) & 0xffu) {                       // has_mac: mac bytes 4..9, byte 4 most significant
            const uint64_t m = ((uint64_t)__builtin_bswap32(w1) << 16) | (uint64_t)((w2 & 0xffu) << 8) | (uint64_t)((w2 >> 8) & 0xffu);
            if (m == mac48) return e;
        } else if (!any) any = e;
    }
    return any;
}

// Copy the namer table (device memory, n_names rows) into LDS if it fits; returns the pointer the lookups use.
template <int THREADS>
NF_DEV const uint8_t* stage_names(const nfagg_intf_name* names, uint32_t n_names, uint32_t* lds_words) {
    if (n_names > kNamesLdsRows) return reinterpret_cast<const uint8_t*>(names);
    const uint32_t* src = reinterpret_cast<const uint32_t*>(names);
    const uint32_t words = n_names * (kNameRowBytes / 4);
    for (uint32_t k = threadIdx.x; k < words; k += THREADS) lds_words[k] = src[k];
    __syncthreads();
    return reinterpret_cast<const uint8_t*>(lds_words);
}

NF_DEV uint64_t mac_be(uint64_t mac_le48) {   // Rec::smac() holds byte 0 in the low bits; macToUint64 (proto.go:246-253) wants it on top
    uint64_t v = 0;
    for (int b = 0; b < 6; b++) v = (v << 8) | ((mac_le48 >> (8 * b)) & 0xff);
    return v;
}

// ---- feature parts of a MapTracer flow (protobuf and FLP-JSON content encoders)
// utils.DNSRawNameToDotted (pkg/utils/utils.go:18-58) over the 32-byte kernel copy at `raw` (the lane's LDS slot):
// bytes up to the first NUL, label by label; stops at a zero length, a compression pointer, or a label that
// runs past the end. EMIT = false only measures.
template <bool EMIT, typename S> NF_DEV uint32_t dns_dotted(S& s, const uint8_t* __restrict__ raw) {
    uint32_t nb = 0;
    while (nb < 32 && raw[nb] != 0) nb++;
    uint32_t i = 0, out = 0;
    while (i < nb) {
        const uint32_t l = raw[i];
        if (l == 0 || (l & 0xC0u) == 0xC0u) break;
        i++;
        if (i + l > nb) break;
        if (out) { if (EMIT) s.put('.'); out++; }
        if (EMIT) for (uint32_t k = 0; k < l; k++) s.put(raw[i + k]);
        out += l; i += l;
    }
    return out;
}

template <int N> NF_DEV void load_dwords16(const uint8_t* p, uint32_t (&w)[N]) {   // N/4 16-byte loads
    const uint4* q = reinterpret_cast<const uint4*>(p);
#pragma unroll
    for (int k = 0; k < N / 4; k++) { const uint4 v = q[k]; w[4 * k] = v.x; w[4 * k + 1] = v.y; w[4 * k + 2] = v.z; w[4 * k + 3] = v.w; }
}
template <int N> NF_DEV void load_dwords8(const uint8_t* p, uint32_t (&w)[N]) {    // N/2 8-byte loads
    const uint2* q = reinterpret_cast<const uint2*>(p);
#pragma unroll
    for (int k = 0; k < N / 2; k++) { const uint2 v = q[k]; w[2 * k] = v.x; w[2 * k + 1] = v.y; }
}

// ---- network events (nfagg_netev.h): the rendered object / message of table row r, copied through a sink. The blob's
// pieces start at 16-byte aligned offsets; a counting sink reads nothing.
NF_DEV void put_blob(CountSink& s, const uint8_t*, uint32_t len) { s.n += len; }
template <typename S> NF_DEV void put_blob(S& s, const uint8_t* p, uint32_t len) {
    for (uint32_t c = 0; c < len; c += 16) {
        const uint4 v = *reinterpret_cast<const uint4*>(p + c);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 16; k++)
            if (c + k < len) s.put((uint8_t)(w[k >> 2] >> (8 * (k & 3))));
    }
}
// The four rows of flow i (0xFFFF: none; a row beyond the table counts as none) and the second half of a table row:
// x = json_off, y = pb_off, z = json_len | pb_len << 16.
NF_DEV void netev_rows(const uint16_t* ne_rows, uint64_t i, uint32_t (&ev)[4]) {
    const uint2 v = reinterpret_cast<const uint2*>(ne_rows)[i];
    ev[0] = v.x & 0xffffu; ev[1] = v.x >> 16; ev[2] = v.y & 0xffffu; ev[3] = v.y >> 16;
}
NF_DEV uint4 netev_row_blobs(const uint8_t* ne_tab, uint32_t r) { return reinterpret_cast<const uint4*>(ne_tab)[2 * r + 1]; }

// ---- the two-pass skeleton. Every size kernel runs kScanBlock records per workgroup and scans their lengths inside it
// (block_scan); the block sums go through launch_scan_block_sums (nfagg_internal.h, nfagg_encode.hip). Every write kernel
// runs one wave per 64 records: it builds the wave's bytes in LDS (WaveImage) and copies them out (copy_image_out).
constexpr int kScanBlock = 1024;

// Block-local exclusive scan of one length per thread: inclusive scan inside the wave, then across the 16 waves
// (wave_tot: kScanBlock / 64 words of LDS). Record i < n gets local_off[i]; the block's total goes to block_sum.
NF_DEV void block_scan(uint32_t len, uint64_t i, uint64_t n, uint32_t* wave_tot, uint32_t* local_off, uint32_t* block_sum) {
    uint32_t v = len;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const uint32_t o = __shfl_up(v, d, 64); if (lane >= d) v += o; }
    if (lane == 63) wave_tot[wave] = v;
    __syncthreads();
    uint32_t base = 0;
    for (int w = 0; w < wave; w++) base += wave_tot[w];
    if (i < n) local_off[i] = base + v - len;
    if (threadIdx.x == kScanBlock - 1) block_sum[blockIdx.x] = base + v;
}

// Where record i starts in the output, from the two scans.
NF_DEV uint64_t record_off(const uint64_t* block_base, const uint32_t* local_off, uint64_t i) {
    return block_base[i / kScanBlock] + local_off[i];
}

// The LDS image of the 64 consecutive records from i0 on: their bytes are contiguous in the output, from wave_base.
// The image has the destination's 16-byte alignment: output byte wave_base is image byte `shift`, and image byte c goes
// to dst[c]. close() takes where each lane's record ends (0 beyond n) and finds where the wave's bytes end.
struct WaveImage {
    uint64_t wave_base, end;
    uint32_t shift, span;          // the wave's bytes: image bytes [shift, span)
    uint8_t* dst;                  // 16-byte aligned
    NF_DEV WaveImage(const uint64_t* block_base, const uint32_t* local_off, uint64_t i0)
        : wave_base(record_off(block_base, local_off, i0)), shift((uint32_t)(wave_base & 15)) {}
    NF_DEV uint32_t pos(uint64_t off) const { return shift + (uint32_t)(off - wave_base); }   // image byte of output byte off
    NF_DEV void close(uint64_t my_end, uint8_t* out) {
        end = my_end;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) { const uint64_t o = __shfl_xor(end, d, 64); end = o > end ? o : end; }
        span = pos(end);
        dst = out + (wave_base - shift);
    }
};

// Image bytes [lo, hi) -> dst, by a wave; lds[0] is image byte `base` (a multiple of 16). Aligned 16-byte stores for
// the chunks wholly inside [lo, hi); the partial chunk at either end goes out bytewise, the neighbouring window or wave
// writes the rest of it.
NF_DEV void copy_image_out(uint8_t* dst, const uint8_t* lds, uint32_t base, uint32_t lo, uint32_t hi) {
    for (uint32_t c = base + threadIdx.x * 16; c < hi; c += 64 * 16) {
        if (c >= lo && c + 16 <= hi) {
            *reinterpret_cast<uint4*>(dst + c) = *reinterpret_cast<const uint4*>(lds + (c - base));
        } else {
            for (uint32_t b = c < lo ? lo : c; b < c + 16 && b < hi; b++) dst[b] = lds[b - base];
        }
    }
}

}  // namespace nfagg
