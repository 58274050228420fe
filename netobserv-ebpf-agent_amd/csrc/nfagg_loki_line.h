// nfagg_loki_line.h — the line side of write loki on the device (nfagg_loki.h): FlpLoki, the policy that leaves
// out the keys the stage takes out of a line, and the two kernels that run encode_line under it, k_loki_key<Feat> (plan) and
// k_loki_write<Feat> (write), with their launches. Each instantiation lives in one translation unit: the plain policy's in
// nfagg_loki.hip, those over FlpContent and FlpContentNetev in nfagg_flp_content.hip, which owns those policies. Device code only.
#pragma once
#include "nfagg_internal.h"
#include "nfagg_loki.h"
#include "nfagg_flp_line.h"
#include "nfagg_tls.h"
#include "nfagg_conn_meta.h"

namespace nfagg {

// ---- the policy: FlpConnMeta<..> whose hooks write nothing for a key that is a label or ignored. The Kubernetes blocks come
// from the Loki table's blob (loki_load hands load_joins a K8sDev with its rows and blob), so those two hooks are the base's.
// The line has no newline: encode_line's last byte is counted off and, in the write kernel, lands on the first framing byte of
// the next entry, which is written after it.
template <typename Base> struct FlpLoki : Base {
    static constexpr uint32_t kMaxEntry = Base::kMaxLine - 1 + kLokiFrameMax;
    static constexpr uint32_t kSlack = (kMaxEntry + 1 + 15) / 16 * 16;               // the longest entry and the newline behind it
    static constexpr uint32_t kWindow = (32768 - Base::kSideLds - kSlack) / 16 * 16;
    static constexpr uint32_t kLds = kWindow + kSlack;
    static_assert(kLds + Base::kSideLds <= 32768 && kWindow >= 16384, "four waves per compute unit, and a window worth its copy-out");
    static_assert(kLokiLabelsMax + 16 < kWindow, "a stream header between two entries never hides the next entry from a window");
    uint32_t omit = 0;
    bool has_conn = false;

    template <typename S> NF_DEV void k8s_layer(S& s) const { if (!(omit & NFAGG_DIM_FLOW_LAYER)) Base::k8s_layer(s); }
    template <typename S> NF_DEV void flow_direction(S& s) const { if (!(omit & NFAGG_DIM_FLOW_DIRECTION)) Base::flow_direction(s); }
    template <typename S> NF_DEV void src_subnet(S& s) const { if (!(omit & NFAGG_DIM_SRC_SUBNET_LABEL)) Base::src_subnet(s); }
    template <typename S> NF_DEV void dst_subnet(S& s) const { if (!(omit & NFAGG_DIM_DST_SUBNET_LABEL)) Base::dst_subnet(s); }
    template <typename S> NF_DEV void conn_meta(S& s) const {
        if (!has_conn) return;
        if (!(omit & NFAGG_LOKI_KEY_HASH_ID)) { lit(s, ",\"_HashId\":\""); hex_u64(s, this->hash_id); s.put('"'); }
        if (!(omit & NFAGG_LOKI_KEY_RECORD_TYPE)) lit(s, ",\"_RecordType\":\"flowLog\"");
    }
};

NF_DEV uint32_t vlen(uint64_t v) { return v ? (uint32_t)(70 - __clzll((long long)v)) / 7u : 1u; }     // bytes of a varint
NF_DEV uint8_t* put_varint(uint8_t* p, uint64_t v) {
    while (v >= 0x80u) { *p++ = (uint8_t)(v | 0x80u); v >>= 7; }
    *p++ = (uint8_t)v;
    return p;
}
NF_DEV uint32_t ts_len(int64_t sec, int64_t nsec) { return (sec ? 1u + vlen((uint64_t)sec) : 0u) + (nsec ? 1u + vlen((uint64_t)nsec) : 0u); }
// 0x12 len Entry around a line of `line` bytes
NF_DEV uint32_t entry_size(uint32_t line, int64_t sec, int64_t nsec) {
    const uint32_t body = 2 + ts_len(sec, nsec) + 1 + vlen(line) + line;
    return 1 + vlen(body) + body;
}

// What k_flp_size / k_flp_write load for a line, then FlpLoki's two fields; the id only in a call that has ids.
template <typename Feat>
NF_DEV void loki_load(Feat& f, const FlpLineArgs& A, const LokiDev& L, uint64_t i, uint8_t* name_slot) {
    FlpJoins J{A.K, A.N, A.k8s_rows, A.net_rows, A.hash_ids};
    f.load(A.F, i, name_slot);
    J.K.rows = L.rows; J.K.blob = L.blob;                   // the policy only swaps the blob
    f.tls = A.T;
    typename Feat::Net& joined = f;                         // the layers below FlpConnMeta, as the line kernels fill them
    joined.load_joins(J, i);
    f.omit = L.omit_keys;
    f.has_conn = A.hash_ids != nullptr;
    if (A.hash_ids) f.hash_id = A.hash_ids[i];
}

// ---- plan: the key kernel
template <typename Feat>
__global__ __launch_bounds__(kScanBlock) void k_loki_key(FlpLineArgs A, LokiDev L, LokiPlanDev D) {
    constexpr uint32_t kSlot = Feat::kSideLds >= 64 * 32 ? 32 : 0;       // a DNS name slot per lane where the policy reads one
    __shared__ __align__(16) uint8_t name_lds[kSlot ? kScanBlock * kSlot : 16];
    __shared__ uint32_t tab_lds[kNamesLdsRows * (kNameRowBytes / 4)];
    const uint8_t* tab = stage_names<kScanBlock>(A.P.names, A.P.n_names, tab_lds);
    const uint64_t i = (uint64_t)blockIdx.x * kScanBlock + threadIdx.x;
    bool deferred = false, part = false;
    if (i < A.n) {
        Rec r;
        load_record(A.recs, i, r);
        uint32_t row[7] = {};
        uint32_t len = 0, slot = kNoSlot;
        int64_t sec = L.now_sec, nsec = L.now_nsec;
        if (!A.hash_ids || conn_tracked(r)) {
            flp_rows(tab, A.P.n_names, r, row);
            Feat f;
            loki_load(f, A, L, i, name_lds + threadIdx.x * kSlot);
            CountSink c;
            encode_line(c, r, A.P, row, f);
            len = c.n - 1;                                  // no newline
            if (L.ts_source != NFAGG_LOKI_TS_NOW) {
                const TimeParts t = flow_time(A.P.now_sec, A.P.now_nsec, A.P.mono_now, L.ts_source == NFAGG_LOKI_TS_TIME_FLOW_END_MS ? r.end() : r.start());
                const int64_t ms = t.sec * 1000 + t.nsec / 1000000;
                if (ms != 0) {
                    const double prod = (double)ms * L.ts_scale;         // a float64 multiply, rounded to nearest even as Go's
                    if (!(prod >= -9223372036854775808.0 && prod < 9223372036854775808.0)) deferred = true;     // leaves int64 (or NaN)
                    else {
                        const int64_t tn = (int64_t)prod;                // truncates toward zero, like Go's conversion
                        sec = tn / 1000000000ll; nsec = tn % 1000000000ll;
                        if (nsec < 0) { nsec += 1000000000ll; sec -= 1; }        // time.Unix
                    }
                }
            }
            if (sec < kLokiMinSeconds || sec >= kLokiMaxSeconds) deferred = true;      // validateTimestamp
            part = !deferred;
            if (part) {
                const uint2 kr = reinterpret_cast<const uint2*>(A.k8s_rows)[i];
                const uint32_t c0 = L.cls[0] && kr.x < A.K.n_rows ? L.cls[0][kr.x] : 0u, c1 = L.cls[1] && kr.y < A.K.n_rows ? L.cls[1][kr.y] : 0u;
                const uint2 nr = A.net_rows[i];
                const uint32_t l0 = nr.x & 0xffffu, l1 = nr.x >> 16;
                const uint32_t s0 = (L.label_keys & NFAGG_DIM_SRC_SUBNET_LABEL) && l0 < A.N.n_labels ? L.canon[l0] : 0xffffu;
                const uint32_t s1 = (L.label_keys & NFAGG_DIM_DST_SUBNET_LABEL) && l1 < A.N.n_labels ? L.canon[l1] : 0xffffu;
                const uint32_t dir = (L.label_keys & NFAGG_DIM_FLOW_DIRECTION) && f.dir <= 2 ? f.dir : 255u;
                const uint32_t layer = (L.label_keys & NFAGG_DIM_FLOW_LAYER) ? f.layer : 0u;
                const uint32_t rt = (L.label_keys & NFAGG_LOKI_KEY_RECORD_TYPE) && A.hash_ids ? 1u : 0u;
                const uint64_t ka = (1ull << 63) | ((uint64_t)c0 << 23) | c1;
                const uint64_t kb = (1ull << 63) | s0 | ((uint64_t)s1 << 16) | ((uint64_t)dir << 32) | ((uint64_t)layer << 40) | ((uint64_t)rt << 42);
                uint32_t s = (uint32_t)fmix64(ka * 0x9E3779B97F4A7C15ull ^ kb) & D.mask;
                if (!ald(&D.ctl->over)) {
                    for (uint32_t t = 0; t <= D.mask; t++) {
                        uint64_t* p = D.keys + (size_t)s * 2;
                        uint64_t a = ald(p);
                        if (a == 0) {
                            a = acas(p, (uint64_t)0, ka);
                            if (a == 0 && aadd(&D.ctl->claimed, 1u) >= kLokiMaxStreams) ast(&D.ctl->over, 1u);
                        }
                        if (a == 0 || a == ka) {
                            uint64_t b = ald(p + 1);
                            if (b == 0) b = acas(p + 1, (uint64_t)0, kb);
                            if (b == 0 || b == kb) { slot = s; break; }
                        }
                        s = (s + 1) & D.mask;
                    }
                    if (slot == kNoSlot) ast(&D.ctl->over, 1u);            // the table walked through
                    // the minimum only falls: a flow that already sees a smaller index sends no atomic (most flows of a large stream)
                    else if (ald(&D.first[slot]) > (uint32_t)i) __hip_atomic_fetch_min(&D.first[slot], (uint32_t)i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            } else len = 0;
        }
        uint4* o = reinterpret_cast<uint4*>(D.rows8 + i * 8);
        o[0] = make_uint4(row[0], row[1], row[2], row[3]);
        o[1] = make_uint4(row[4], row[5], row[6], len);
        D.lens[i] = len;
        D.slot_of[i] = slot;
        D.ts[2 * i] = sec; D.ts[2 * i + 1] = nsec;
        D.deferred[i] = deferred ? 1 : 0;
    }
    const uint64_t dm = __ballot(deferred), pm = __ballot(part);
    if ((threadIdx.x & 63) == 0) {
        if (dm) aadd(&D.ctl->n_deferred, (uint32_t)__popcll(dm));
        if (pm) aadd(&D.ctl->n_part, (uint32_t)__popcll(pm));
    }
}


// ---- write: the entries. One wave per 64 consecutive output positions; position j holds flow perm[j]. The wave's bytes are
// contiguous: every position's entry, and in front of a group's first position room for the group's header, which
// k_loki_headers fills afterwards (the copy-out writes that room too, with whatever the LDS held).
template <typename Feat>
__global__ __launch_bounds__(64) void k_loki_write(FlpLineArgs A, LokiDev L, LokiPlanDev D, LokiWriteDev W, uint32_t m, uint8_t* __restrict__ out) {
    static_assert(Feat::kLds + Feat::kSideLds <= 32768, "four waves per compute unit");
    constexpr uint32_t kSlot = Feat::kSideLds >= 64 * 32 ? 32 : 0;
    __shared__ __align__(16) uint8_t lds[Feat::kLds];
    __shared__ __align__(16) uint8_t name_lds[kSlot ? 64 * kSlot : 16];
    const uint64_t j0 = (uint64_t)blockIdx.x * 64, j = j0 + threadIdx.x;
    WaveImage w(W.block_base, W.local_off, j0);
    uint64_t ent_off = 0; uint32_t my_len = 0, line = 0;
    int64_t sec = 0, nsec = 0;
    uint32_t row[7] = {};
    uint64_t i = 0;
    Rec r;
    Feat f;
    if (j < m) {
        i = W.perm[j];
        load_record(A.recs, i, r);
        const uint4* q = reinterpret_cast<const uint4*>(D.rows8 + i * 8);
        const uint4 a = q[0], b = q[1];
        row[0] = a.x; row[1] = a.y; row[2] = a.z; row[3] = a.w; row[4] = b.x; row[5] = b.y; row[6] = b.z;
        line = b.w;
        sec = D.ts[2 * i]; nsec = D.ts[2 * i + 1];
        my_len = entry_size(line, sec, nsec);
        loki_load(f, A, L, i, name_lds + threadIdx.x * kSlot);
        ent_off = record_off(W.block_base, W.local_off, j) + (W.flag[j] ? W.hsz[W.gidx[j] - 1] : 0u);
    }
    w.close(ent_off + my_len, out);
    const uint32_t p0 = w.pos(ent_off);                           // my entry = image bytes [p0, p0 + my_len)
    const uint32_t frame = my_len - line;
    uint32_t lo = w.shift;
    while (lo < w.span) {                                         // the window loop of k_flp_write
        const uint32_t base = lo & ~15u;
        const bool mine = my_len && p0 >= lo && p0 - base < Feat::kWindow;
        if (mine) { FlpLds s{lds + (p0 - base) + frame}; encode_line(s, r, A.P, row, f); }     // its newline: the next entry's first byte
        __syncthreads();
        if (mine) {
            uint8_t* p = lds + (p0 - base);
            const uint32_t tl = ts_len(sec, nsec);
            *p++ = 0x12; p = put_varint(p, 2 + tl + 1 + vlen(line) + line);
            *p++ = 0x0a; *p++ = (uint8_t)tl;
            if (sec) { *p++ = 0x08; p = put_varint(p, (uint64_t)sec); }
            if (nsec) { *p++ = 0x10; p = put_varint(p, (uint64_t)nsec); }
            *p++ = 0x12; put_varint(p, line);
        }
        uint32_t hi = mine ? p0 + my_len : lo;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) { const uint32_t o = __shfl_xor(hi, d, 64); hi = o > hi ? o : hi; }
        __syncthreads();
        copy_image_out(w.dst, lds, base, lo, hi);
        __syncthreads();
        if (hi <= lo) break;                                      // never: a header is shorter than a window
        lo = hi;
    }
}


template <typename Feat>
__attribute__((noinline)) hipError_t loki_key_as(const FlpLineArgs& A, const LokiDev& L, const LokiPlanDev& D, hipStream_t s) {
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_loki_key<Feat>, dim3((unsigned)((A.n + kScanBlock - 1) / kScanBlock)), dim3(kScanBlock), 0, s, A, L, D);
    return hipGetLastError();
}
template <typename Feat>
__attribute__((noinline)) hipError_t loki_write_as(const FlpLineArgs& A, const LokiDev& L, const LokiPlanDev& D, const LokiWriteDev& W, uint32_t m, uint8_t* d_out,
                                                   hipStream_t s) {
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_loki_write<Feat>, dim3((m + 63) / 64), dim3(64), 0, s, A, L, D, W, m, d_out);
    return hipGetLastError();
}
template <typename Base> using LokiOver = FlpLoki<FlpConnMeta<FlpNet<FlpK8s<FlpTls<Base>>>>>;

}  // namespace nfagg
