// nfagg_metrics.hip — the hash aggregation of nfagg_metrics_fold and nfagg_metrics_fold_content (nfagg_metrics.h): k_metrics_fold
// and k_metrics_fold_content group the flows and sum, k_metrics_count / k_metrics_emit compact each grouping's occupied slots into
// the caller's arrays. Integer sums only, so the result does not depend on the order of the flows; no floating point anywhere.
//
// k_metrics_fold: grid-stride, one lane per flow, one workgroup per 4 096 flows up to 512 workgroups. A lane reads the three 16-byte units of its record that hold the protocol
// (@36), bytes (@56), packets (@64) and the ethertype (@68), its 8 bytes of Kubernetes rows and its 8 bytes of net row; per
// grouping the two class words, and K8sRow.flags of both rows once when a grouping selects the layer. Flows are pre-aggregated
// per workgroup in an LDS open-addressed table shared by the groupings (the key carries the grouping): kMetLdsSlots slots of
// key halves and five sums as seven arrays, 56 KiB, so that two workgroups fit a compute unit's 160 KiB. A lane whose probe of
// the LDS table passes kMetLdsProbe slots goes straight to the global table; at the end of the loop the workgroup flushes its
// LDS entries to the global tables.
//
// k_metrics_fold_content: the same walk with a key of three words (the third: drop cause, drop state, response code, IPsec
// status, bucket) and nine sums. Beside the record a lane loads only what some grouping of the call needs, which is uniform per
// call: present[i]; of additional_metrics the unit @16 (flow_rtt, ipsec_encrypted_ret, ipsec_encrypted); of dns_metrics the
// unit @16 (latency, id, flags) and nothing of the name; of pkt_drop_metrics the unit @16 (bytes, packets, cause, state). The
// bucket of a value is the number of bounds below it, counted over the spec's n_bounds thresholds with scalar loads from the
// kernel arguments: bounds do not decrease, so that is the first k with value <= bounds[k], and n_bounds for +Inf. The LDS
// table has kMetcLdsSlots slots of twelve live words as twelve arrays.
//
// Claim protocol (LDS and global alike; nobody waits, no key is ever partly published as another key's): a key is K words, two
// or three. For k = 0 .. K - 1: load word k of the slot; if it is empty, compare-and-swap it from empty to the lane's word k;
// go on to word k + 1 if the old value was empty or equal to the lane's word, else move to the next slot. The invariant:
//   - a set word never changes, and slots are never freed within a call;
//   - whoever sets word k goes on to word k + 1 of the same slot at once, and there either sets it or finds it set by another
//     lane (which it then compares with its own). Either way word k + 1 is set once that lane has passed, so by induction
//     over k no slot is partly set when the kernel ends: a set first word means K set words;
//   - so a slot whose first j words are set and whose word j is still empty may be taken by ANY key with those first j
//     words: with three words a slot holding (A, B) and an empty third word belongs to whichever key with that (A, B)
//     arrives first, and a later key with the same (A, B) and another C walks on. Nothing is added to a slot before all K
//     words matched, so the sums of a slot are those of exactly one key.
// A key's probe sequence is fixed by its hash and the words it passes never change back, so within one table a key always ends
// in the same slot: one slot per key, one key per slot. Every word carries bit 63 and the grouping, so no word is ever the
// empty value and words of different groupings never match.
//
// Overflow: a first word claimed from empty is one more occupied slot of that grouping, counted in MetCtl::claimed. A count
// over the cap, or a probe that has walked the whole table, sets MetCtl::overflow, and every later lane of that grouping gives
// up at once: the table has twice the cap's slots, so it does not fill up behind the flag except by the lanes already in
// flight, and a probe is bounded by the table's size whatever happens. Flag, cap, count and emit are one code for both slot
// widths (kMetSlotWords, kMetcSlotWords).
#include "nfagg_metrics.h"
#include "nfagg_encode.h"

namespace nfagg {

constexpr int kMetBlock = 512;
constexpr uint32_t kMetLdsSlots = 1024, kMetLdsProbe = 8, kMetMaxBlocks = 512;     // two workgroups per compute unit of 256
// A workgroup's flush costs up to kMetLdsSlots global claims and five adds each whatever it folded, so a workgroup is given
// at least this many flows: a call of a few hundred thousand flows then pays for tens of flushes, not for 512.
constexpr uint64_t kMetFlowsPerBlock = 4096;
static_assert(kMetLdsSlots * 7 * 8 * 2 <= 160 * 1024, "two workgroups' LDS tables in a compute unit");
// The content fold's LDS table: twelve live words per slot. 1 024 slots are 96 KiB, one workgroup per compute unit; 512 are 48 KiB,
// three. Measured on the content leg of tools/flp_json_bench.py, both builds alternating in one run (profiles/flp_metrics_content_bench.txt):
// 1 024 slots take 0.97 ms where 512 take 3.9 ms (342 k flows) and 3.6 ms against 6.4 ms (2.86 M flows): groups multiply by the
// buckets, and what the table does not hold goes to HBM flow by flow. -DNFAGG_METC_LDS_SLOTS builds the other setting.
#ifndef NFAGG_METC_LDS_SLOTS
#define NFAGG_METC_LDS_SLOTS 1024
#endif
constexpr uint32_t kMetcLdsSlots = NFAGG_METC_LDS_SLOTS, kMetcKeys = 3, kMetcSums = 9;
static_assert((kMetcLdsSlots & (kMetcLdsSlots - 1)) == 0 && kMetcLdsSlots * (kMetcKeys + kMetcSums) * 8 <= 160 * 1024, "a power of two that fits a compute unit");
static_assert(kMetMinSlots == kScanBlock, "a table is whole blocks of k_metrics_count");

struct MetLds {
    unsigned long long a[kMetLdsSlots], b[kMetLdsSlots], sum[5][kMetLdsSlots];
};

// NK key words at the head of a slot of W words, NS sums from word S0 on.
template <int NK, int NS, uint32_t W, int S0> NF_DEV void met_global_add_as(const MetDev& M, uint32_t g, uint64_t hash, const uint64_t (&key)[NK], const uint64_t (&v)[NS]) {
    uint32_t* over = &M.ctl->overflow[g];
    if (ald(over)) return;
    const uint32_t mask = M.mask[g];
    uint64_t* tab = M.slots[g];
    uint32_t s = (uint32_t)hash & mask;
    for (uint32_t t = 0; t <= mask; t++) {
        uint64_t* p = tab + (size_t)s * W;
        uint64_t a = ald(p);
        if (a == 0) {
            a = acas(p, (uint64_t)0, key[0]);
            if (a == 0 && aadd(&M.ctl->claimed[g], 1u) >= M.cap[g]) ast(over, 1u);      // this slot is number cap + 1 or later
        }
        bool mine = a == 0 || a == key[0];
#pragma unroll
        for (int k = 1; k < NK; k++)
            if (mine) {
                uint64_t b = ald(p + k);
                if (b == 0) b = acas(p + k, (uint64_t)0, key[k]);
                mine = b == 0 || b == key[k];
            }
        if (mine) {
#pragma unroll
            for (int k = 0; k < NS; k++) if (v[k]) aadd(p + S0 + k, v[k]);
            return;
        }
        if ((t & 7u) == 7u && ald(over)) return;
        s = (s + 1) & mask;
    }
    ast(over, 1u);                                                                       // the table is full
}

NF_DEV void met_global_add(const MetDev& M, uint32_t g, uint64_t ka, uint64_t kb, const uint64_t (&v)[5]) {
    const uint64_t key[2] = {ka, kb};
    met_global_add_as<2, 5, kMetSlotWords, 2>(M, g, met_hash(ka, kb), key, v);
}

__global__ __launch_bounds__(kMetBlock) void k_metrics_fold(const void* __restrict__ recs, uint64_t n, MetDev M, const uint32_t* __restrict__ k8s_rows,
                                                            const uint2* __restrict__ net_rows) {
    __shared__ MetLds L;
    for (uint32_t k = threadIdx.x; k < kMetLdsSlots; k += kMetBlock) {
        L.a[k] = 0; L.b[k] = 0;
#pragma unroll
        for (int j = 0; j < 5; j++) L.sum[j][k] = 0;
    }
    __syncthreads();
    const uint64_t stride = (uint64_t)gridDim.x * kMetBlock;
    for (uint64_t i = (uint64_t)blockIdx.x * kMetBlock + threadIdx.x; i < n; i += stride) {
        const uint4* p = reinterpret_cast<const uint4*>(reinterpret_cast<const uint8_t*>(recs) + i * kRecordBytes);
        const uint4 u2 = p[2], u3 = p[3], u4 = p[4];
        const uint64_t bytes = (uint64_t)u3.z | ((uint64_t)u3.w << 32), packets = u4.x;
        const uint32_t eth = u4.y & 0xffffu;
        const uint32_t is_ip = (eth == 0x0800u || eth == 0x86DDu) ? 1u : 0u;
        const uint32_t proto = is_ip ? (u2.y & 0xffu) : 0u;                              // a record that is not IP has no Proto key
        const uint2 kr = reinterpret_cast<const uint2*>(k8s_rows)[i];
        const uint2 nr = net_rows ? net_rows[i] : make_uint2(0xffffffffu, kNetNoDirection);
        uint32_t layer = 0;
        if (M.any_layer && M.has_layer) {                                                // FlpK8s::load_k8s
            bool app = false;
            if (kr.x < M.n_rows) app = (M.rows[kr.x].flags & kK8sRowApp) != 0;
            if (kr.y < M.n_rows) app = app || (M.rows[kr.y].flags & kK8sRowApp) != 0;
            layer = app ? 2u : 1u;
        }
        const uint64_t v[5] = {1ull, bytes, packets, bytes ? 1ull : 0ull, packets ? 1ull : 0ull};
        for (uint32_t g = 0; g < M.n_groupings; g++) {
            const uint32_t d = M.dims[g];
            const uint32_t* cs = M.cls[g][0];
            const uint32_t* cd = M.cls[g][1];
            const uint32_t sc = cs && kr.x < M.n_rows ? cs[kr.x] : 0u, dc = cd && kr.y < M.n_rows ? cd[kr.y] : 0u;
            const uint64_t ka = met_key_a(g, sc, dc);
            const uint64_t kb = met_key_b(g, (d & NFAGG_DIM_SRC_SUBNET_LABEL) ? nr.x & 0xffffu : kNetNoLabel,
                                          (d & NFAGG_DIM_DST_SUBNET_LABEL) ? nr.x >> 16 : kNetNoLabel,
                                          (d & NFAGG_DIM_FLOW_DIRECTION) ? nr.y & 0xffu : kNetNoDirection, (d & NFAGG_DIM_FLOW_LAYER) ? layer : 0u,
                                          (d & NFAGG_DIM_PROTO) ? proto : 0u, (d & NFAGG_DIM_PROTO) ? is_ip : 0u);
            uint32_t s = (uint32_t)met_hash(ka, kb) & (kMetLdsSlots - 1);
            bool done = false;
            for (uint32_t t = 0; t < kMetLdsProbe && !done; t++) {
                unsigned long long a = __hip_atomic_load(&L.a[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                if (a == 0) a = atomicCAS(&L.a[s], 0ull, (unsigned long long)ka);
                if (a == 0 || a == ka) {
                    unsigned long long b = __hip_atomic_load(&L.b[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    if (b == 0) b = atomicCAS(&L.b[s], 0ull, (unsigned long long)kb);
                    if (b == 0 || b == kb) {
#pragma unroll
                        for (int k = 0; k < 5; k++) if (v[k]) atomicAdd(&L.sum[k][s], (unsigned long long)v[k]);
                        done = true;
                    }
                }
                s = (s + 1) & (kMetLdsSlots - 1);
            }
            if (!done) met_global_add(M, g, ka, kb, v);
        }
    }
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < kMetLdsSlots; k += kMetBlock) {
        const uint64_t ka = L.a[k];
        if (!ka) continue;
        const uint64_t v[5] = {L.sum[0][k], L.sum[1][k], L.sum[2][k], L.sum[3][k], L.sum[4][k]};
        met_global_add(M, met_key_grouping(ka), ka, L.b[k], v);
    }
}

struct MetcLds {
    unsigned long long key[kMetcKeys][kMetcLdsSlots], sum[kMetcSums][kMetcLdsSlots];
};

NF_DEV void metc_global_add(const MetDev& M, uint32_t g, const uint64_t (&key)[kMetcKeys], const uint64_t (&v)[kMetcSums]) {
    met_global_add_as<kMetcKeys, kMetcSums, kMetcSlotWords, 4>(M, g, met_hash(key[0], key[1], key[2]), key, v);
}

// What RecordToMap makes of a flow's feature parts, as far as the metrics read them (the rules of FlpContent's dns, ipsec, drops
// and rtt in nfagg_flp_content.hip): a value and whether its key exists, per source; the four extra dimensions' raw values.
struct MetFlow {
    uint64_t value[NFAGG_MET_VALUE_LAST + 1];
    uint32_t has;                      // bit s: source s exists for this flow
    uint32_t cause, state, rcode, ipsec;
};

__global__ __launch_bounds__(kMetBlock) void k_metrics_fold_content(const void* __restrict__ recs, uint64_t n, MetDev M, MetSpecDev X,
                                                                    const uint32_t* __restrict__ k8s_rows, const uint2* __restrict__ net_rows) {
    __shared__ MetcLds L;
    for (uint32_t k = threadIdx.x; k < kMetcLdsSlots; k += kMetBlock) {
#pragma unroll
        for (int j = 0; j < (int)kMetcKeys; j++) L.key[j][k] = 0;
#pragma unroll
        for (int j = 0; j < (int)kMetcSums; j++) L.sum[j][k] = 0;
    }
    __syncthreads();
    const uint64_t stride = (uint64_t)gridDim.x * kMetBlock;
    for (uint64_t i = (uint64_t)blockIdx.x * kMetBlock + threadIdx.x; i < n; i += stride) {
        const uint4* p = reinterpret_cast<const uint4*>(reinterpret_cast<const uint8_t*>(recs) + i * kRecordBytes);
        const uint4 u2 = p[2], u3 = p[3], u4 = p[4];
        const uint64_t bytes = (uint64_t)u3.z | ((uint64_t)u3.w << 32), packets = u4.x;
        const uint32_t eth = u4.y & 0xffffu;
        const uint32_t is_ip = (eth == 0x0800u || eth == 0x86DDu) ? 1u : 0u;
        const uint32_t proto = is_ip ? (u2.y & 0xffu) : 0u;                              // a record that is not IP has no Proto key
        const uint2 kr = reinterpret_cast<const uint2*>(k8s_rows)[i];
        const uint2 nr = net_rows ? net_rows[i] : make_uint2(0xffffffffu, kNetNoDirection);
        uint32_t layer = 0;
        if (M.any_layer && M.has_layer) {                                                // FlpK8s::load_k8s
            bool app = false;
            if (kr.x < M.n_rows) app = (M.rows[kr.x].flags & kK8sRowApp) != 0;
            if (kr.y < M.n_rows) app = app || (M.rows[kr.y].flags & kK8sRowApp) != 0;
            layer = app ? 2u : 1u;
        }
        MetFlow f;
        f.value[NFAGG_MET_VALUE_NONE] = 0;
        f.value[NFAGG_MET_VALUE_BYTES] = bytes; f.value[NFAGG_MET_VALUE_PACKETS] = packets;
        f.has = (bytes ? 1u << NFAGG_MET_VALUE_BYTES : 0u) | (packets ? 1u << NFAGG_MET_VALUE_PACKETS : 0u);
        f.value[NFAGG_MET_VALUE_RTT_NS] = f.value[NFAGG_MET_VALUE_DNS_LATENCY_MS] = f.value[NFAGG_MET_VALUE_DROP_BYTES] = f.value[NFAGG_MET_VALUE_DROP_PACKETS] = 0;
        f.cause = 0; f.state = 0xffffu; f.rcode = 0xffu; f.ipsec = 0;
        const uint32_t have = X.need ? X.present[i] : 0u;                                // X.need != 0 only with the present bytes
        if ((X.need & kMetNeedAdditional) && (have & NFAGG_FEAT_ADDITIONAL)) {
            const uint4 a = *reinterpret_cast<const uint4*>(X.additional + i * 32 + 16);   // flow_rtt (2), ipsec_encrypted_ret, eth | ipsec_encrypted << 16
            const uint64_t rtt = (uint64_t)a.x | ((uint64_t)a.y << 32);
            f.value[NFAGG_MET_VALUE_RTT_NS] = rtt;
            if (rtt) f.has |= 1u << NFAGG_MET_VALUE_RTT_NS;
            f.ipsec = a.z != 0 ? 2u : ((a.w >> 16) & 0xffu) ? 1u : 0u;
        }
        if ((X.need & kMetNeedDns) && (have & NFAGG_FEAT_DNS)) {
            const uint4 d = *reinterpret_cast<const uint4*>(X.dns + i * 64 + 16);          // latency (2), id | flags << 16, eth | errno << 16 | name[0] << 24
            if (d.z & 0xffffu) {                                                         // DnsId != 0: the four DNS keys exist
                // record.go:116-120 + Duration.Milliseconds(): int64(latency) / 1e6, truncating towards zero
                f.value[NFAGG_MET_VALUE_DNS_LATENCY_MS] = (uint64_t)((int64_t)((uint64_t)d.x | ((uint64_t)d.y << 32)) / 1000000ll);
                f.has |= 1u << NFAGG_MET_VALUE_DNS_LATENCY_MS;
                f.rcode = (d.z >> 16) & 15u;
            }
        }
        if ((X.need & kMetNeedDrops) && (have & NFAGG_FEAT_DROPS)) {
            const uint4 d = *reinterpret_cast<const uint4*>(X.drops + i * 32 + 16);        // bytes | packets << 16, cause, flags | eth << 16, state
            if (d.y) {                                                                   // a cause: the five drop keys exist
                f.value[NFAGG_MET_VALUE_DROP_BYTES] = d.x & 0xffffu; f.value[NFAGG_MET_VALUE_DROP_PACKETS] = d.x >> 16;
                f.has |= (1u << NFAGG_MET_VALUE_DROP_BYTES) | (1u << NFAGG_MET_VALUE_DROP_PACKETS);
                f.cause = d.y; f.state = d.w & 0xffu;
            }
        }
        for (uint32_t g = 0; g < M.n_groupings; g++) {
            const uint32_t d = M.dims[g], xd = X.xdims[g];
            const uint32_t* cs = M.cls[g][0];
            const uint32_t* cd = M.cls[g][1];
            const uint32_t sc = cs && kr.x < M.n_rows ? cs[kr.x] : 0u, dc = cd && kr.y < M.n_rows ? cd[kr.y] : 0u;
            const uint32_t src0 = X.value[g][0], src1 = X.value[g][1], hist = X.hist[g];     // uniform: the selects below are scalar branches
            uint64_t v0 = 0, v1 = 0;
            uint32_t h0 = 0, h1 = 0;
#pragma unroll
            for (uint32_t sidx = 1; sidx <= NFAGG_MET_VALUE_LAST; sidx++) {
                if (src0 == sidx) { v0 = f.value[sidx]; h0 = (f.has >> sidx) & 1u; }
                if (src1 == sidx) { v1 = f.value[sidx]; h1 = (f.has >> sidx) & 1u; }
            }
            uint32_t bucket = NFAGG_MET_NO_BUCKET;
            if (hist) {
                const uint64_t hv = hist == 1 ? v0 : v1;
                const uint32_t hsrc = hist == 1 ? src0 : src1;
                if (hist == 1 ? h0 : h1) {
                    const uint32_t nb = X.n_bounds[g];
                    if (hsrc == NFAGG_MET_VALUE_BYTES && (hv >> 63)) bucket = nb;           // above INT64_MAX: +Inf
                    else {
                        bucket = 0;
                        for (uint32_t k = 0; k < nb; k++) bucket += (int64_t)hv > X.bounds[g][k] ? 1u : 0u;
                    }
                }
            }
            const uint64_t key[kMetcKeys] = {
                met_key_a(g, sc, dc),
                met_key_b(g, (d & NFAGG_DIM_SRC_SUBNET_LABEL) ? nr.x & 0xffffu : kNetNoLabel, (d & NFAGG_DIM_DST_SUBNET_LABEL) ? nr.x >> 16 : kNetNoLabel,
                          (d & NFAGG_DIM_FLOW_DIRECTION) ? nr.y & 0xffu : kNetNoDirection, (d & NFAGG_DIM_FLOW_LAYER) ? layer : 0u,
                          (d & NFAGG_DIM_PROTO) ? proto : 0u, (d & NFAGG_DIM_PROTO) ? is_ip : 0u),
                met_key_c(g, (xd & NFAGG_XDIM_DROP_CAUSE) ? f.cause : 0u, (xd & NFAGG_XDIM_DROP_STATE) ? f.state : 0xffffu,
                          (xd & NFAGG_XDIM_DNS_RCODE) ? f.rcode : 0xffu, (xd & NFAGG_XDIM_IPSEC_STATUS) ? f.ipsec : 0u, bucket)};
            const uint64_t v[kMetcSums] = {1ull, bytes, packets, bytes ? 1ull : 0ull, packets ? 1ull : 0ull, h0 ? v0 : 0ull, h1 ? v1 : 0ull, h0, h1};
            uint32_t s = (uint32_t)met_hash(key[0], key[1], key[2]) & (kMetcLdsSlots - 1);
            bool done = false;
            for (uint32_t t = 0; t < kMetLdsProbe && !done; t++) {
                bool mine = true;
#pragma unroll
                for (int k = 0; k < (int)kMetcKeys; k++)
                    if (mine) {
                        unsigned long long w = __hip_atomic_load(&L.key[k][s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        if (w == 0) w = atomicCAS(&L.key[k][s], 0ull, (unsigned long long)key[k]);
                        mine = w == 0 || w == key[k];
                    }
                if (mine) {
#pragma unroll
                    for (int k = 0; k < (int)kMetcSums; k++) if (v[k]) atomicAdd(&L.sum[k][s], (unsigned long long)v[k]);
                    done = true;
                }
                s = (s + 1) & (kMetcLdsSlots - 1);
            }
            if (!done) metc_global_add(M, g, key, v);
        }
    }
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < kMetcLdsSlots; k += kMetBlock) {
        const uint64_t key[kMetcKeys] = {L.key[0][k], L.key[1][k], L.key[2][k]};
        if (!key[0]) continue;
        uint64_t v[kMetcSums];
#pragma unroll
        for (int j = 0; j < (int)kMetcSums; j++) v[j] = L.sum[j][k];
        metc_global_add(M, met_key_grouping(key[0]), key, v);
    }
}

// Which grouping block b of the concatenated tables belongs to.
NF_DEV uint32_t met_block_grouping(const MetDev& M, uint32_t b) {
    uint32_t g = 0;
    while (g + 1 < M.n_groupings && b >= M.first_block[g + 1]) g++;
    return g;
}

// One lane per slot (of W words) of the concatenated tables: 1 for an occupied slot, scanned inside the block.
template <uint32_t W> __global__ __launch_bounds__(kScanBlock) void k_metrics_count(MetDev M, uint32_t* __restrict__ local_off, uint32_t* __restrict__ block_sum) {
    __shared__ uint32_t wave_tot[kScanBlock / 64];
    const uint32_t g = met_block_grouping(M, blockIdx.x);
    const uint32_t s = (blockIdx.x - M.first_block[g]) * kScanBlock + threadIdx.x;       // tables are multiples of kScanBlock slots
    const uint64_t i = (uint64_t)blockIdx.x * kScanBlock + threadIdx.x;
    const uint32_t occupied = M.slots[g][(size_t)s * W] != 0 ? 1u : 0u;
    block_scan(occupied, i, (uint64_t)gridDim.x * kScanBlock, wave_tot, local_off, block_sum);
}

// block_base: the scan of the block sums over all groupings, the total last. Every lane works out the verdict from the
// groupings' counts; block 0 reports it; the groups are written only when no grouping is over. A slot of kMetSlotWords becomes a
// nfagg_metric_group, one of kMetcSlotWords a nfagg_metric_group_content.
template <uint32_t W> __global__ __launch_bounds__(kScanBlock) void k_metrics_emit(MetDev M, const uint32_t* __restrict__ local_off, const uint64_t* __restrict__ block_base) {
    bool any_over = false;
    for (uint32_t g = 0; g < M.n_groupings; g++) {
        const uint32_t count = (uint32_t)(block_base[M.first_block[g + 1]] - block_base[M.first_block[g]]);
        const bool over = M.ctl->overflow[g] != 0 || count > M.cap[g];
        any_over = any_over || over;
        if (blockIdx.x == 0 && threadIdx.x == g) { M.ctl->count[g] = count; M.ctl->over[g] = over ? 1u : 0u; }
    }
    if (any_over) return;
    const uint32_t g = met_block_grouping(M, blockIdx.x);
    const uint32_t s = (blockIdx.x - M.first_block[g]) * kScanBlock + threadIdx.x;
    const uint4* q = reinterpret_cast<const uint4*>(M.slots[g] + (size_t)s * W);
    const uint4 k = q[0];
    if ((k.x | k.y) == 0) return;
    const uint64_t i = (uint64_t)blockIdx.x * kScanBlock + threadIdx.x;
    const uint64_t at = block_base[blockIdx.x] - block_base[M.first_block[g]] + local_off[i];      // < count <= cap
    const uint64_t ka = (uint64_t)k.x | ((uint64_t)k.y << 32), kb = (uint64_t)k.z | ((uint64_t)k.w << 32);
    uint4* o = reinterpret_cast<uint4*>(reinterpret_cast<uint8_t*>(M.out[g]) + at * (W * 8));
    // nfagg_metric_group: src_class, dst_class, src_label | dst_label << 16, direction | layer << 8 | proto << 16 | is_ip << 24
    o[0] = make_uint4((uint32_t)ka & 0x1fffffffu, (uint32_t)(ka >> 29) & 0x1fffffffu, (uint32_t)kb,
                      ((uint32_t)(kb >> 32) & 0xffu) | (((uint32_t)(kb >> 40) & 3u) << 8) | (((uint32_t)(kb >> 42) & 0xffu) << 16) | (((uint32_t)(kb >> 50) & 1u) << 24));
    if constexpr (W == kMetSlotWords) {
        o[1] = q[1];
        o[2] = q[2];
        const uint4 last = q[3];
        o[3] = make_uint4(last.x, last.y, 0u, 0u);
    } else {
        // the third word back into drop_cause, drop_state | dns_rcode << 16 | ipsec_status << 24, bucket: a masked "none" gets its public value
        const uint4 c = q[1];
        const uint32_t hi = c.y, state = hi & 0x1ffu, rcode = (hi >> 9) & 0x1fu, ipsec = (hi >> 14) & 3u, bucket = (hi >> 16) & 0x3fu;
        o[1] = make_uint4(c.x, (state > 0xffu ? 0xffffu : state) | ((rcode > 15u ? 0xffu : rcode) << 16) | (ipsec << 24),
                          bucket > NFAGG_MET_MAX_BOUNDS ? (uint32_t)NFAGG_MET_NO_BUCKET : bucket, 0u);
#pragma unroll
        for (int k = 2; k < 6; k++) o[k] = q[k];                                         // the five sums, value_sum, flows_with_value[0]
        const uint4 last = q[6];
        o[6] = make_uint4(last.x, last.y, 0u, 0u);                                       // flows_with_value[1]
        o[7] = make_uint4(0u, 0u, 0u, 0u);
    }
}

hipError_t launch_metrics_fold(const void* d_recs, uint64_t n, const MetDev& M, const uint32_t* d_k8s_rows, const uint2* d_net_rows, hipStream_t s) {
    const uint64_t want = (n + kMetFlowsPerBlock - 1) / kMetFlowsPerBlock;
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_metrics_fold, dim3((unsigned)(want < kMetMaxBlocks ? want : kMetMaxBlocks)), dim3(kMetBlock), 0, s, d_recs, n, M, d_k8s_rows, d_net_rows);
    return hipGetLastError();
}

hipError_t launch_metrics_fold_content(const void* d_recs, uint64_t n, const MetDev& M, const MetSpecDev& X, const uint32_t* d_k8s_rows, const uint2* d_net_rows,
                                       hipStream_t s) {
    const uint64_t want = (n + kMetFlowsPerBlock - 1) / kMetFlowsPerBlock;
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_metrics_fold_content, dim3((unsigned)(want < kMetMaxBlocks ? want : kMetMaxBlocks)), dim3(kMetBlock), 0, s, d_recs, n, M, X, d_k8s_rows,
                       d_net_rows);
    return hipGetLastError();
}

template <uint32_t W> static hipError_t metrics_emit_as(const MetDev& M, uint32_t* d_local_off, uint32_t* d_block_sum, uint64_t* d_block_base, hipStream_t s) {
    const uint32_t blocks = M.first_block[M.n_groupings];
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_metrics_count<W>, dim3(blocks), dim3(kScanBlock), 0, s, M, d_local_off, d_block_sum);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if ((e = launch_scan_block_sums(d_block_sum, blocks, d_block_base, s)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_metrics_emit<W>, dim3(blocks), dim3(kScanBlock), 0, s, M, d_local_off, d_block_base);
    return hipGetLastError();
}

hipError_t launch_metrics_emit(const MetDev& M, bool content, uint32_t* d_local_off, uint32_t* d_block_sum, uint64_t* d_block_base, hipStream_t s) {
    return content ? metrics_emit_as<kMetcSlotWords>(M, d_local_off, d_block_sum, d_block_base, s)
                   : metrics_emit_as<kMetSlotWords>(M, d_local_off, d_block_sum, d_block_base, s);
}

}  // namespace nfagg
