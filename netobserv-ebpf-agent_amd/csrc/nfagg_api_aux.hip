// nfagg_api_aux.hip — the small side operations of the C ABI (include/nfagg.h): the per-CPU rollups, the merge of the drained
// maps, the sketches' read side. Each stages its arguments in scratch of the handle (nfagg_api_call.h), launches and synchronises.
#include <hip/hip_runtime.h>
#include <string.h>
#include <algorithm>
#include <set>
#include <utility>
#include <vector>

#include "../../include/nfagg.h"
#include "nfagg_internal.h"
#include "nfagg_handle.h"
#include "nfagg_api_call.h"

using namespace nfagg;

extern "C" {

// ---------------------------------------------------------------- rollups
static int rollup_core(nfagg_handle* h, int kind, const void* partials, size_t n_flows, size_t n_cpu,
                       nfagg_flow_metrics* base, void* folded) {
    if (!h || !partials || !base || !folded) return fail(h, NFAGG_EINVAL, "null argument");
    if (n_flows == 0) return NFAGG_OK;
    if (n_cpu == 0) return fail(h, NFAGG_EINVAL, "n_cpu must be >= 1");
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t ssz = rollup_struct_size(kind);
    const size_t pb = n_flows * n_cpu * ssz, bb = n_flows * sizeof(nfagg_flow_metrics), fb = n_flows * ssz;
    API_TRY(h->roll.folded.ensure(h, fb));
    API_TRY(stage_in(h, h->roll.partials, partials, pb));
    API_TRY(stage_in(h, h->roll.base, base, bb));
    hipError_t e = launch_rollup(kind, h->roll.partials.p, n_flows, n_cpu, h->roll.base.p, h->roll.folded.p, h->stream);
    if (e != hipSuccess) return fail(h, NFAGG_EDEVICE, "rollup launch failed: %s", hipGetErrorString(e));
    API_TRY(fetch(h, base, h->roll.base, bb));
    API_TRY(fetch(h, folded, h->roll.folded, fb));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return NFAGG_OK;
}

int nfagg_rollup_additional(nfagg_handle* h, const nfagg_additional_metrics* p, size_t nf, size_t nc,
                            nfagg_flow_metrics* base, nfagg_additional_metrics* folded) { return rollup_core(h, 0, p, nf, nc, base, folded); }
int nfagg_rollup_dns(nfagg_handle* h, const nfagg_dns_metrics* p, size_t nf, size_t nc,
                     nfagg_flow_metrics* base, nfagg_dns_metrics* folded) { return rollup_core(h, 1, p, nf, nc, base, folded); }
int nfagg_rollup_drops(nfagg_handle* h, const nfagg_pkt_drop_metrics* p, size_t nf, size_t nc,
                       nfagg_flow_metrics* base, nfagg_pkt_drop_metrics* folded) { return rollup_core(h, 2, p, nf, nc, base, folded); }
int nfagg_rollup_network_events(nfagg_handle* h, const nfagg_network_events_metrics* p, size_t nf, size_t nc,
                                nfagg_flow_metrics* base, nfagg_network_events_metrics* folded) { return rollup_core(h, 3, p, nf, nc, base, folded); }
int nfagg_rollup_xlat(nfagg_handle* h, const nfagg_xlat_metrics* p, size_t nf, size_t nc,
                      nfagg_flow_metrics* base, nfagg_xlat_metrics* folded) { return rollup_core(h, 4, p, nf, nc, base, folded); }
int nfagg_rollup_quic(nfagg_handle* h, const nfagg_quic_metrics* p, size_t nf, size_t nc,
                      nfagg_flow_metrics* base, nfagg_quic_metrics* folded) { return rollup_core(h, 5, p, nf, nc, base, folded); }

// ---------------------------------------------------------------- map merge (LookupAndDeleteMap's join)
static const int kWalk[7] = {-1, NFAGG_ROLLUP_DNS, NFAGG_ROLLUP_DROPS, NFAGG_ROLLUP_NETWORK_EVENTS, NFAGG_ROLLUP_XLAT,
                             NFAGG_ROLLUP_ADDITIONAL, NFAGG_ROLLUP_QUIC};   // tracer.go:1057-1110; position 0 = main map

static int map_merge_device_core(nfagg_handle* h, const nfagg_map_view* mm, const nfagg_map_view fm[6], size_t n_cpu,
                                 const nfagg_merged_flows* out, size_t cap, size_t* n_out, size_t* n_dup) {
    if (!h || !mm || !fm || !out || !n_out) return fail(h, NFAGG_EINVAL, "null argument");
    if (n_cpu == 0 || n_cpu > 0xFFFFu) return fail(h, NFAGG_EINVAL, "n_cpu must be in [1, 65535]");
    MergeIn in{};
    in.n_cpu = (uint32_t)n_cpu;
    uint64_t total = 0;
    uintptr_t align = 0;
    for (int q = 0; q < 7; q++) {
        const nfagg_map_view& v = q == 0 ? *mm : fm[kWalk[q]];
        if (v.n && (!v.ids || !v.values)) return fail(h, NFAGG_EINVAL, "map %d: null ids/values", q);
        in.ids[q] = (const uint8_t*)v.ids; in.vals[q] = (const uint8_t*)v.values;
        in.off[q] = (uint32_t)total;
        total += v.n;
        if (v.n) align |= (uintptr_t)v.ids | (uintptr_t)v.values;
    }
    if (total > (1ull << 30)) return fail(h, NFAGG_ERANGE, "map merge: more than 2^30 rows");
    in.off[7] = (uint32_t)total;
    *n_out = 0;
    if (n_dup) *n_dup = 0;
    if (total == 0) return NFAGG_OK;
    if (cap && (!out->records || !out->present)) return fail(h, NFAGG_EINVAL, "null records/present output");
    align |= (uintptr_t)out->records | (uintptr_t)out->additional | (uintptr_t)out->dns | (uintptr_t)out->drops |
             (uintptr_t)out->network_events | (uintptr_t)out->xlat | (uintptr_t)out->quic;
    if (align & 7u) return fail(h, NFAGG_EINVAL, "map merge: device arrays must be 8-byte aligned");
    HIP_TRY(h, hipSetDevice(h->device));
    uint32_t n_slots = 1024;
    while ((uint64_t)n_slots < 2 * total) n_slots <<= 1;
    const size_t blocks = (total + 1023) / 1024;
    API_TRY(ensure_all(h, {{h->mm.slots, (size_t)n_slots * merge_slot_bytes()}, {h->mm.slot_of, total * sizeof(uint32_t)}, {h->mm.local_off, total * sizeof(uint32_t)},
                           {h->mm.block_sum, blocks * sizeof(uint32_t)}, {h->mm.block_base, (blocks + 1) * sizeof(uint64_t)}, {h->mm.n_dup, 16}}));
    HIP_TRY(h, hipMemsetAsync(h->mm.slots.p, 0xFF, (size_t)n_slots * merge_slot_bytes(), h->stream));
    HIP_TRY(h, hipMemsetAsync(h->mm.n_dup.p, 0, 16, h->stream));
    hipError_t e = launch_merge_build(in, h->mm.slots.p, n_slots, h->mm.slot_of.as<uint32_t>(), h->mm.n_dup.as<unsigned int>(),
                                      h->mm.local_off.as<uint32_t>(), h->mm.block_sum.as<uint32_t>(), h->stream);
    if (e != hipSuccess) return fail(h, NFAGG_EDEVICE, "map merge build launch failed: %s", hipGetErrorString(e));
    e = launch_scan_block_sums(h->mm.block_sum.as<const uint32_t>(), (uint32_t)blocks, h->mm.block_base.as<uint64_t>(), h->stream);
    if (e != hipSuccess) return fail(h, NFAGG_EDEVICE, "map merge scan launch failed: %s", hipGetErrorString(e));
    uint64_t flows = 0; unsigned int dups = 0;
    HIP_TRY(h, hipMemcpyAsync(&flows, h->mm.block_base.as<uint64_t>() + blocks, sizeof flows, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipMemcpyAsync(&dups, h->mm.n_dup.p, sizeof dups, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    *n_out = (size_t)flows;
    if (n_dup) *n_dup = dups;
    if (flows > cap) return NFAGG_TRUNCATED;
    MergeOut o{out->records, out->present, out->additional, out->dns, out->drops, out->network_events, out->xlat, out->quic};
    e = launch_merge_fold(in, o, h->mm.slots.p, h->mm.slot_of.as<const uint32_t>(), h->mm.local_off.as<const uint32_t>(), h->mm.block_base.as<const uint64_t>(), h->stream);
    if (e != hipSuccess) return fail(h, NFAGG_EDEVICE, "map merge fold launch failed: %s", hipGetErrorString(e));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return NFAGG_OK;
}

int nfagg_map_merge_device(nfagg_handle* h, const nfagg_map_view* d_main_map, const nfagg_map_view d_feature_maps[6],
                           size_t n_cpu, const nfagg_merged_flows* d_out, size_t cap, size_t* n_out, size_t* n_duplicate_keys) {
    return map_merge_device_core(h, d_main_map, d_feature_maps, n_cpu, d_out, cap, n_out, n_duplicate_keys);
}

int nfagg_map_merge(nfagg_handle* h, const nfagg_map_view* main_map, const nfagg_map_view feature_maps[6],
                    size_t n_cpu, const nfagg_merged_flows* out, size_t cap, size_t* n_out, size_t* n_duplicate_keys) {
    if (!h || !main_map || !feature_maps || !out || !n_out) return fail(h, NFAGG_EINVAL, "null argument");
    if (n_cpu == 0) return fail(h, NFAGG_EINVAL, "n_cpu must be >= 1");
    HIP_TRY(h, hipSetDevice(h->device));
    nfagg_map_view dm{}, df[6] = {};
    for (int q = 0; q < 7; q++) {
        const nfagg_map_view& v = q == 0 ? *main_map : feature_maps[q - 1];
        nfagg_map_view& d = q == 0 ? dm : df[q - 1];
        d.n = v.n;
        if (!v.n) continue;
        if (!v.ids || !v.values) return fail(h, NFAGG_EINVAL, "map %d: null ids/values", q);
        const size_t vb = q == 0 ? v.n * sizeof(nfagg_flow_metrics) : v.n * n_cpu * rollup_struct_size(q - 1);
        API_TRY(stage_in(h, h->mm.ids[q], v.ids, v.n * sizeof(nfagg_flow_id)));
        API_TRY(stage_in(h, h->mm.vals[q], v.values, vb));
        d.ids = h->mm.ids[q].as<const nfagg_flow_id>(); d.values = h->mm.vals[q].p;
    }
    void* host_out[8] = {out->records, out->present, out->additional, out->dns, out->drops, out->network_events, out->xlat, out->quic};
    const size_t elem[8] = {sizeof(nfagg_flow_record), 1, sizeof(nfagg_additional_metrics), sizeof(nfagg_dns_metrics), sizeof(nfagg_pkt_drop_metrics),
                            sizeof(nfagg_network_events_metrics), sizeof(nfagg_xlat_metrics), sizeof(nfagg_quic_metrics)};
    void* dev_out[8] = {};
    for (int k = 0; k < 8; k++) {
        if (!host_out[k] || !cap) continue;
        API_TRY(h->mm.out[k].ensure(h, cap * elem[k] + kStageSlack));
        dev_out[k] = h->mm.out[k].p;
    }
    nfagg_merged_flows dout{(nfagg_flow_record*)dev_out[0], (uint8_t*)dev_out[1], (nfagg_additional_metrics*)dev_out[2], (nfagg_dns_metrics*)dev_out[3],
                            (nfagg_pkt_drop_metrics*)dev_out[4], (nfagg_network_events_metrics*)dev_out[5], (nfagg_xlat_metrics*)dev_out[6],
                            (nfagg_quic_metrics*)dev_out[7]};
    API_TRY(map_merge_device_core(h, &dm, df, n_cpu, &dout, cap, n_out, n_duplicate_keys));
    for (int k = 0; k < 8; k++)
        if (dev_out[k]) API_TRY(fetch(h, host_out[k], h->mm.out[k], *n_out * elem[k]));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return NFAGG_OK;
}

// ---------------------------------------------------------------- sketches
static int sketch_info(nfagg_handle* h, int which, void** p, size_t* bytes) {
    if (which == NFAGG_CM_SRC || which == NFAGG_CM_DST) {
        if (!(h->sk.flags & NFAGG_SKETCH_CM)) return fail(h, NFAGG_ESTATE, "Count-Min sketch not enabled");
        *p = h->sk.cm[which - NFAGG_CM_SRC];
        *bytes = ((size_t)h->sk.cm_depth << h->sk.cm_log2w) * sizeof(uint64_t);
        return NFAGG_OK;
    }
    if (which == NFAGG_HLL_SRC || which == NFAGG_HLL_DST) {
        if (!(h->sk.flags & NFAGG_SKETCH_HLL)) return fail(h, NFAGG_ESTATE, "HyperLogLog sketch not enabled");
        *p = h->sk.hll[which - NFAGG_HLL_SRC];
        *bytes = ((size_t)1 << h->sk.hll_p);                     // uint8_t registers
        return NFAGG_OK;
    }
    return fail(h, NFAGG_EINVAL, "unknown sketch id %d", which);
}

int nfagg_sketch_device_ptr(nfagg_handle* h, int which, void** d_ptr, size_t* bytes) {
    if (!h || !d_ptr || !bytes) return fail(h, NFAGG_EINVAL, "null argument");
    return sketch_info(h, which, d_ptr, bytes);
}

int nfagg_sketch_snapshot(nfagg_handle* h, int which, void* out, size_t out_bytes) {
    if (!h || !out) return fail(h, NFAGG_EINVAL, "null argument");
    HIP_TRY(h, hipSetDevice(h->device));
    void* p; size_t bytes;
    int rc = sketch_info(h, which, &p, &bytes);
    if (rc != NFAGG_OK) return rc;
    if (out_bytes < bytes) return NFAGG_TRUNCATED;                   // the device arrays ARE the snapshot layout (HLL: one byte per register)
    HIP_TRY(h, hipMemcpyAsync(out, p, bytes, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return NFAGG_OK;
}

int nfagg_sketch_reset(nfagg_handle* h) {
    if (!h) return NFAGG_EINVAL;
    HIP_TRY(h, hipSetDevice(h->device));
    for (int which = 0; which < 4; which++) {
        const bool on = which < 2 ? (h->sk.flags & NFAGG_SKETCH_CM) : (h->sk.flags & NFAGG_SKETCH_HLL);
        if (!on) continue;
        void* p; size_t bytes;
        int rc = sketch_info(h, which, &p, &bytes);
        if (rc != NFAGG_OK) return rc;
        HIP_TRY(h, hipMemsetAsync(p, 0, bytes, h->stream));
    }
    return NFAGG_OK;
}

// HyperLogLog estimate (Flajolet et al. 2007, 64-bit hash so no large-range
// correction) from the histogram of register values: sum_k hist[k] * 2^-k. The sum is accumulated exactly, as the
// integer sum_k hist[k] << (64 - k) (below 2^103 for any 65 uint32 counts: it fits 128 bits), converted to double once and
// scaled by 2^-64: one rounding whatever the registers hold. (A sum of doubles term by term rounds at every term whose
// exponent lies 53 bits below the running sum's: half of the registers at 1 and half at 47 with p = 18 already does it.)
// alpha * m * m is exact (m is a power of two), the division rounds once. Our own spec; the scalar oracle loops over
// the registers instead and does the same arithmetic.
double nfagg_hll_estimate_from_histogram(const uint32_t* hist, uint32_t p) {
    const double m = (double)(1ull << p);
    const double alpha = (p == 4) ? 0.673 : (p == 5) ? 0.697 : (p == 6) ? 0.709 : 0.7213 / (1.0 + 1.079 / m);
    unsigned __int128 acc = 0;
    for (int k = 0; k <= 64; k++) acc += (unsigned __int128)hist[k] << (64 - k);
    const double sum = __builtin_ldexp((double)acc, -64);
    double e = alpha * m * m / sum;
    if (e <= 2.5 * m && hist[0] != 0) e = m * __builtin_log(m / (double)hist[0]);
    return e;
}

int nfagg_hll_estimate(nfagg_handle* h, int which, double* estimate) {
    if (!h || !estimate) return fail(h, NFAGG_EINVAL, "null argument");
    if (which != NFAGG_HLL_SRC && which != NFAGG_HLL_DST) return fail(h, NFAGG_EINVAL, "which must be an HLL sketch");
    HIP_TRY(h, hipSetDevice(h->device));
    void* p; size_t bytes;
    int rc = sketch_info(h, which, &p, &bytes);
    if (rc != NFAGG_OK) return rc;
    hipError_t e = launch_hll_histogram((const uint8_t*)p, h->sk.hll_p, h->d_hist.as<uint32_t>(), h->stream);
    if (e != hipSuccess) return fail(h, NFAGG_EDEVICE, "hll histogram launch failed: %s", hipGetErrorString(e));
    uint32_t hist[65];
    HIP_TRY(h, hipMemcpyAsync(hist, h->d_hist.p, sizeof hist, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    *estimate = nfagg_hll_estimate_from_histogram(hist, h->sk.hll_p);
    return NFAGG_OK;
}

int nfagg_cm_query(nfagg_handle* h, int which, const uint8_t ip[16], uint64_t* estimate) {
    if (!h || !ip || !estimate) return fail(h, NFAGG_EINVAL, "null argument");
    if (which != NFAGG_CM_SRC && which != NFAGG_CM_DST) return fail(h, NFAGG_EINVAL, "which must be a CM sketch");
    HIP_TRY(h, hipSetDevice(h->device));
    void* p; size_t bytes;
    int rc = sketch_info(h, which, &p, &bytes);
    if (rc != NFAGG_OK) return rc;
    uint64_t lo, hi;
    memcpy(&lo, ip, 8); memcpy(&hi, ip + 8, 8);
    const uint64_t ha = ip_hash(lo, hi, 0), hb = ip_hash(lo, hi, 1) | 1ull;
    uint64_t best = ~0ull;
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    for (uint32_t r = 0; r < h->sk.cm_depth; r++) {
        uint64_t v;
        const uint64_t at = ((uint64_t)r << h->sk.cm_log2w) + cm_index(ha, hb, r, h->sk.cm_log2w);
        HIP_TRY(h, hipMemcpy(&v, (const uint64_t*)p + at, sizeof v, hipMemcpyDeviceToHost));
        if (v < best) best = v;
    }
    *estimate = best;
    return NFAGG_OK;
}

// Heavy hitters. Device: estimate per record, radix sort by estimate (descending). Host: walk the sorted order, keep the
// first occurrence of every address, stop once k distinct addresses are known AND the estimate has dropped below the
// k-th one (ties at the boundary are resolved by address bytes, so every candidate with the boundary estimate must be seen).
static int cm_topk_core(nfagg_handle* h, int which, const void* d_records, size_t n, size_t k, nfagg_heavy_hitter* out, size_t* n_out) {
    if (!h || !n_out || (k && !out) || (n && !d_records)) return fail(h, NFAGG_EINVAL, "null argument");
    if (which != NFAGG_CM_SRC && which != NFAGG_CM_DST) return fail(h, NFAGG_EINVAL, "which must be a CM sketch");
    if (n >= (1ull << 31)) return fail(h, NFAGG_ERANGE, "heavy hitters: more than 2^31 candidate records");
    *n_out = 0;
    void* cm; size_t cm_bytes;
    int rc = sketch_info(h, which, &cm, &cm_bytes);
    if (rc != NFAGG_OK) return rc;
    if (n == 0 || k == 0) return NFAGG_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    const int side = which - NFAGG_CM_SRC;
    size_t temp_bytes = 0;
    hipError_t e = launch_cm_sort_desc(nullptr, nullptr, nullptr, nullptr, n, nullptr, &temp_bytes, h->stream);
    if (e != hipSuccess) return fail(h, NFAGG_EDEVICE, "sort size query failed: %s", hipGetErrorString(e));
    if ((rc = h->hh.est.ensure(h, n * sizeof(uint64_t))) != NFAGG_OK) return rc;
    if ((rc = h->hh.est_sorted.ensure(h, n * sizeof(uint64_t))) != NFAGG_OK) return rc;
    if ((rc = h->hh.idx.ensure(h, n * sizeof(uint32_t))) != NFAGG_OK) return rc;
    if ((rc = h->hh.idx_sorted.ensure(h, n * sizeof(uint32_t))) != NFAGG_OK) return rc;
    if ((rc = h->hh.sort_tmp.ensure(h, temp_bytes + 16)) != NFAGG_OK) return rc;
    e = launch_cm_estimate((const uint64_t*)cm, h->sk.cm_depth, h->sk.cm_log2w, side, d_records, n, h->hh.est.as<uint64_t>(), h->hh.idx.as<uint32_t>(), h->stream);
    if (e == hipSuccess) e = launch_cm_sort_desc(h->hh.est.as<const uint64_t>(), h->hh.est_sorted.as<uint64_t>(), h->hh.idx.as<const uint32_t>(), h->hh.idx_sorted.as<uint32_t>(), n,
                                                 h->hh.sort_tmp.p, &temp_bytes, h->stream);
    if (e != hipSuccess) return fail(h, NFAGG_EDEVICE, "heavy-hitter launch failed: %s", hipGetErrorString(e));
    struct Row { uint64_t lo, hi, est; };
    std::vector<Row> rows, best;                         // best: distinct addresses in order of appearance (estimate descending)
    std::set<std::pair<uint64_t, uint64_t>> group;       // addresses already taken at the current estimate
    uint64_t group_est = ~0ull;
    size_t seen = 0, m = k * 16 < 4096 ? 4096 : k * 16;
    for (;;) {
        if (m > n) m = n;
        if ((rc = h->hh.rows.ensure(h, m * sizeof(Row))) != NFAGG_OK) return rc;
        e = launch_cm_gather(d_records, side, h->hh.est_sorted.as<const uint64_t>(), h->hh.idx_sorted.as<const uint32_t>(), m, h->hh.rows.as<uint64_t>(), h->stream);
        if (e != hipSuccess) return fail(h, NFAGG_EDEVICE, "heavy-hitter gather failed: %s", hipGetErrorString(e));
        rows.resize(m);
        HIP_TRY(h, hipMemcpyAsync(rows.data(), h->hh.rows.p, m * sizeof(Row), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        bool done = false;
        for (; seen < m; seen++) {
            const Row& r = rows[seen];
            if (best.size() >= k && r.est < best[k - 1].est) { done = true; break; }   // below the boundary: nothing further can enter
            // an address always carries the same estimate, so a duplicate can only sit among the entries with THIS estimate
            if (r.est != group_est) { group.clear(); group_est = r.est; }
            if (group.insert(std::make_pair(r.lo, r.hi)).second) best.push_back(r);
        }
        if (done || m == n) break;
        m *= 4;
    }
    std::sort(best.begin(), best.end(), [](const Row& a, const Row& b) {
        if (a.est != b.est) return a.est > b.est;
        return memcmp(&a.lo, &b.lo, 16) < 0;             // lo,hi are adjacent: the 16 address bytes in order
    });
    const size_t cnt = best.size() < k ? best.size() : k;
    for (size_t q = 0; q < cnt; q++) { memcpy(out[q].ip, &best[q].lo, 16); out[q].estimate = best[q].est; }
    *n_out = cnt;
    return NFAGG_OK;
}

int nfagg_cm_topk_device(nfagg_handle* h, int which, const void* d_records, size_t n, size_t k, nfagg_heavy_hitter* out, size_t* n_out) {
    return cm_topk_core(h, which, d_records, n, k, out, n_out);
}

int nfagg_cm_topk(nfagg_handle* h, int which, const void* records, size_t n, size_t k, nfagg_heavy_hitter* out, size_t* n_out) {
    if (!h || (n && !records)) return fail(h, NFAGG_EINVAL, "null argument");
    HIP_TRY(h, hipSetDevice(h->device));
    API_TRY(stage_in(h, h->hh.records, records, n * kRecordBytes));
    return cm_topk_core(h, which, h->hh.records.p, n, k, out, n_out);
}

}  // extern "C"
