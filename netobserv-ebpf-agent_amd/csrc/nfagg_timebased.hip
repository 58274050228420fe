// nfagg_timebased.hip — the kernels of nfagg_timebased_extract (nfagg_timebased.h): the windowed GROUP BY and the top-K of
// flowlogs-pipeline's `extract timebased`. One lane per flow (or per key, or per slice entry), grid-stride where flows are
// walked. Partials are integers; float64 appears only in k_tb_value, where a rule is evaluated. This file is built WITHOUT
// fast-math (csrc/Makefile sets none, and nothing here asks for it): `avg` is one IEEE float64 division and `diff` one IEEE
// subtraction, and uint64 / int64 -> float64 are the compiler's correctly rounded conversions.
//
// The kernels of a call, in stream order:
//   k_tb_presence   per flow the five 16-byte units of its record that hold the id (@0..39), bytes (@56), packets (@64) and the
//                   ethertype (@68), its rows, and of its feature parts what some table's value sources need. Per table: does the
//                   flow enter (every index key present), and has it every value source. One byte of enter bits per flow, one
//                   count of flows that enter a table without one of its values. Nothing else is written: the host reads the
//                   count and refuses the call before any key is claimed.
//   k_tb_claim      (per table) the flow's key, its slot by the claim protocol below, into slot_of[i].
//   k_tb_fold       (per table) after the kernel boundary every slot has its id. The flow adds to its key's call area: n, the
//                   two halves of each value, and atomic max of ~value, value, ~index, index + 1. The lane that finds n == 0
//                   appends the id to the table's touched list (one add per wave for its lanes together).
//   k_tb_finish     (per table) after the boundary the least and the greatest index are final: the flows that own them store
//                   their values as first and last, as k_conn_finish does.
//   k_tb_emit       (per table) one lane per touched id: the partial into the call's slice, the newest value into lastval, the
//                   call area back to zero. A call costs O(flows + touched keys), never O(table).
//   k_tb_merge      (per rule and slice in its window, oldest first) one lane per slice entry into the rule's accumulator of that
//                   id. A key is at most once in a slice and slices follow each other on the stream: no atomics, and the order
//                   gives "first in the window".
//   k_tb_value      (per rule) one lane per id: the float64 value, its flags and its order-preserving integer.
//   k_tb_hist / k_tb_pick, eight times, then k_tb_compact and k_tb_sort (per rule with top_k below the keys): radix select of
//                   the K-th best integer, most significant byte first; everything strictly better, then as many ties as fit;
//                   one workgroup sorts the at most 4 096 survivors in LDS (bitonic) and writes the results.
//
// Claim protocol (that of nfagg_metrics.hip and nfagg_conn.hip, widened; nobody waits, no key is ever partly published as
// another key's): a key is K = n_words key words, one to six. For k = 0 .. K - 1: load word k of the slot; if it is empty,
// compare-and-swap it from empty to the lane's word k; go on to word k + 1 if the old value was empty or equal to the lane's
// word, else move to the next slot. The invariant, for any K:
//   - a set word never changes, and slots are never freed (the table outlives the call: only reset empties it);
//   - whoever sets word k goes on to word k + 1 of the same slot at once, and there either sets it or finds it set by another
//     lane (which it then compares with its own). Either way word k + 1 is set once that lane has passed, so by induction over
//     k no slot is partly set when a kernel ends: a set first word means K set words, in this call and in every later one;
//   - so a slot whose first j words are set and whose word j is still empty may be taken by ANY key with those first j words:
//     it belongs to whichever such key arrives first, and a later key with the same first j words and another word j walks
//     on. Nothing is folded into a slot's id before all K words matched (k_tb_fold runs after the boundary), so an id's
//     partial is that of exactly one key.
// A key's probe sequence is fixed by its hash and the words it passes never change back, so a key always ends in the same
// slot: one slot per key, one key per slot. Every key word carries bit 63, so no word is ever the empty value.
// The dense id belongs to the SLOT: the lane whose compare-and-swap set word 0 draws it from TbCtl::n_keys and stores id + 1
// in word 6 and the slot in slot_of_id[id], whichever key ends up owning the slot. That is a returning add per new key, which
// nfagg_conn.hip avoids by counting behind probe rounds; here the result IS the id, and only a key's first flow ever pays it.
//
// Overflow: an id at or above max_keys sets TbCtl::overflow and is not stored. Probes go in rounds of eight; a lane looks at
// the flag before its first probe and behind every round and gives up, so a table that is too small does not fill up to its
// last slot first: it has at least twice max_keys slots. A probe that has walked the whole table sets the flag too. After an
// overflow k_tb_fold and k_tb_finish do nothing, and the host fails the object.
#include "nfagg_timebased.h"
#include "nfagg_device.h"

namespace nfagg {

constexpr int kTbBlock = 256;
constexpr uint32_t kTbMaxBlocks = 2048, kTbRound = 8, kTbSortMax = NFAGG_TB_MAX_TOPK;
constexpr uint64_t kTbFlowsPerBlock = 1024;

struct TbAllTables { TbTableDev t[kTbMaxTables]; uint32_t n; uint32_t need; };     // need: kMetNeed* bits

constexpr uint32_t kTbNeedAdditional = 1, kTbNeedDns = 2, kTbNeedDrops = 4;

// What RecordToMap makes of a flow, as far as the tables read it: the rules of k_metrics_fold_content for the values.
struct TbFlow {
    uint4 u0, u1;                      // the addresses
    uint32_t ports, proto, is_ip;
    uint2 kr, nr;
    uint64_t value[NFAGG_MET_VALUE_LAST + 1];
    uint32_t has;                      // bit s: source s exists for this flow
};

NF_DEV void tb_load(const TbFlows& F, uint32_t need, uint64_t i, TbFlow& f) {
    const uint4* p = reinterpret_cast<const uint4*>(reinterpret_cast<const uint8_t*>(F.recs) + i * kRecordBytes);
    const uint4 u2 = p[2], u3 = p[3], u4 = p[4];
    f.u0 = p[0]; f.u1 = p[1];
    const uint64_t bytes = (uint64_t)u3.z | ((uint64_t)u3.w << 32), packets = u4.x;
    const uint32_t eth = u4.y & 0xffffu;
    f.is_ip = (eth == 0x0800u || eth == 0x86DDu) ? 1u : 0u;
    f.ports = u2.x; f.proto = u2.y & 0xffu;
    f.kr = F.k8s_rows ? reinterpret_cast<const uint2*>(F.k8s_rows)[i] : make_uint2(0xffffffffu, 0xffffffffu);
    f.nr = F.net_rows ? F.net_rows[i] : make_uint2(0xffffffffu, kNetNoDirection);
#pragma unroll
    for (int s = 0; s <= NFAGG_MET_VALUE_LAST; s++) f.value[s] = 0;
    f.value[NFAGG_MET_VALUE_BYTES] = bytes; f.value[NFAGG_MET_VALUE_PACKETS] = packets;
    f.has = (bytes ? 1u << NFAGG_MET_VALUE_BYTES : 0u) | (packets ? 1u << NFAGG_MET_VALUE_PACKETS : 0u);
    const uint32_t have = need ? F.present[i] : 0u;                                      // need != 0 only with the present bytes
    if ((need & kTbNeedAdditional) && (have & NFAGG_FEAT_ADDITIONAL)) {
        const uint4 a = *reinterpret_cast<const uint4*>(F.additional + i * 32 + 16);     // flow_rtt (2), ...
        const uint64_t rtt = (uint64_t)a.x | ((uint64_t)a.y << 32);
        f.value[NFAGG_MET_VALUE_RTT_NS] = rtt;
        if (rtt) f.has |= 1u << NFAGG_MET_VALUE_RTT_NS;
    }
    if ((need & kTbNeedDns) && (have & NFAGG_FEAT_DNS)) {
        const uint4 d = *reinterpret_cast<const uint4*>(F.dns + i * 64 + 16);            // latency (2), id | flags << 16, ...
        if (d.z & 0xffffu) {
            f.value[NFAGG_MET_VALUE_DNS_LATENCY_MS] = (uint64_t)((int64_t)((uint64_t)d.x | ((uint64_t)d.y << 32)) / 1000000ll);
            f.has |= 1u << NFAGG_MET_VALUE_DNS_LATENCY_MS;
        }
    }
    if ((need & kTbNeedDrops) && (have & NFAGG_FEAT_DROPS)) {
        const uint4 d = *reinterpret_cast<const uint4*>(F.drops + i * 32 + 16);          // bytes | packets << 16, cause, ...
        if (d.y) {
            f.value[NFAGG_MET_VALUE_DROP_BYTES] = d.x & 0xffffu; f.value[NFAGG_MET_VALUE_DROP_PACKETS] = d.x >> 16;
            f.has |= (1u << NFAGG_MET_VALUE_DROP_BYTES) | (1u << NFAGG_MET_VALUE_DROP_PACKETS);
        }
    }
}

// Column c of table T for flow f: is the key present, and its value (an address: 4 units in a[], else v).
NF_DEV bool tb_column(const TbTableDev& T, uint32_t c, const TbFlow& f, uint32_t (&a)[4], uint32_t& v) {
    const uint32_t kind = T.col[c];
    v = 0;
    if (kind == kTbColSrcAddr) { a[0] = f.u0.x; a[1] = f.u0.y; a[2] = f.u0.z; a[3] = f.u0.w; return f.is_ip != 0; }
    if (kind == kTbColDstAddr) { a[0] = f.u1.x; a[1] = f.u1.y; a[2] = f.u1.z; a[3] = f.u1.w; return f.is_ip != 0; }
    const bool ported = f.is_ip && (f.proto == 6u || f.proto == 17u || f.proto == 132u);
    if (kind == kTbColSrcPort) { v = f.ports & 0xffffu; return ported; }
    if (kind == kTbColDstPort) { v = f.ports >> 16; return ported; }
    if (kind == kTbColProto) { v = f.proto; return f.is_ip != 0; }
    if (kind == kTbColDirection) { v = f.nr.y & 0xffu; return v != kNetNoDirection; }
    if (kind == kTbColSrcLabel || kind == kTbColDstLabel) {
        v = kind == kTbColSrcLabel ? f.nr.x & 0xffffu : f.nr.x >> 16;
        return v < kNetMaxCidrs && ((T.label_ok[v >> 6] >> (v & 63u)) & 1ull) != 0;
    }
    const uint32_t row = ((kind - kTbColK8s) >> 4) ? f.kr.y : f.kr.x;                    // a Kubernetes column
    if (row >= T.n_rows) return false;
    v = T.cls[c][row];
    return T.cls_ok[c][v] != 0;
}

NF_DEV bool tb_enters(const TbTableDev& T, const TbFlow& f) {
    bool in = true;
    uint32_t a[4], v;
    for (uint32_t c = 0; c < T.n_cols; c++) in = tb_column(T, c, f, a, v) && in;
    return in;
}

NF_DEV uint64_t tb_value(const TbTableDev& T, uint32_t j, const TbFlow& f) {
    const uint32_t src = T.src[j];
    uint64_t v = 0;
#pragma unroll
    for (uint32_t s = 1; s <= NFAGG_MET_VALUE_LAST; s++) if (src == s) v = f.value[s];
    return tb_src_signed(src) ? v ^ kTbBias : v;
}

__global__ __launch_bounds__(kTbBlock) void k_tb_presence(TbFlows F, TbAllTables A, TbCtl* ctl, uint8_t* __restrict__ enter) {
    const uint64_t stride = (uint64_t)gridDim.x * kTbBlock;
    for (uint64_t i = (uint64_t)blockIdx.x * kTbBlock + threadIdx.x; i < F.n; i += stride) {
        TbFlow f;
        tb_load(F, A.need, i, f);
        uint32_t bits = 0;
        bool missing = false;
        for (uint32_t t = 0; t < A.n; t++) {
            const TbTableDev& T = A.t[t];
            if (!tb_enters(T, f)) continue;
            bits |= 1u << t;
            for (uint32_t j = 0; j < T.n_src; j++) missing = missing || !((f.has >> T.src[j]) & 1u);
        }
        enter[i] = (uint8_t)bits;
        const unsigned long long m = __ballot(missing);                                  // one add per wave
        if (missing && (threadIdx.x & 63) == __ffsll(m) - 1) aadd(&ctl->n_missing, (uint64_t)__popcll(m));
    }
}

NF_DEV bool tb_over(const TbCtl* ctl, uint32_t t) { return ald(&ctl->overflow[t]) != 0; }

NF_DEV uint32_t tb_claim(const TbTableDev& T, TbCtl* ctl, const uint64_t (&raw)[kTbRawWords]) {
    if (tb_over(ctl, T.index)) return kTbNoSlot;
    uint64_t kw[kTbKeyWords];
#pragma unroll
    for (uint32_t j = 0; j < kTbKeyWords; j++) kw[j] = tb_key_word(raw, j);
    const uint32_t mask = T.mask;
    uint32_t s = (uint32_t)tb_hash(raw) & mask;
    for (uint64_t t0 = 0; t0 <= mask; t0 += kTbRound) {
        for (uint32_t t = 0; t < kTbRound && t0 + t <= mask; t++) {
            uint64_t* p = T.slots + (size_t)s * kTbSlotWords;
            uint64_t a = ald(p);
            if (a == 0) {
                a = acas(p, (uint64_t)0, kw[0]);
                if (a == 0) {                                                            // this lane set word 0: the slot's id is its to give
                    const uint32_t id = aadd(&ctl->n_keys[T.index], 1u);
                    if (id >= T.max_keys) ast(&ctl->overflow[T.index], 1u);
                    else { ast(p + kTbIdWord, (uint64_t)id + 1); T.slot_of_id[id] = s; }
                }
            }
            bool mine = a == 0 || a == kw[0];
#pragma unroll
            for (uint32_t k = 1; k < kTbKeyWords; k++)
                if (mine && k < T.n_words) {
                    uint64_t b = ald(p + k);
                    if (b == 0) b = acas(p + k, (uint64_t)0, kw[k]);
                    mine = b == 0 || b == kw[k];
                }
            if (mine) return s;
            s = (s + 1) & mask;
        }
        if (tb_over(ctl, T.index)) return kTbNoSlot;
    }
    ast(&ctl->overflow[T.index], 1u);                                                    // the table is full
    return kTbNoSlot;
}

// Unit `at` of the key's ten: a select per unit, because `at` is uniform but not a constant and a register array cannot be indexed.
NF_DEV void tb_set_unit(uint32_t (&u)[kTbMaxUnits], uint32_t at, uint32_t v) {
#pragma unroll
    for (uint32_t k = 0; k < kTbMaxUnits; k++) u[k] = k == at ? v : u[k];
}

__global__ __launch_bounds__(kTbBlock) void k_tb_claim(TbFlows F, TbTableDev T, TbCtl* ctl, const uint8_t* __restrict__ enter, uint32_t* __restrict__ slot_of) {
    const uint64_t stride = (uint64_t)gridDim.x * kTbBlock;
    for (uint64_t i = (uint64_t)blockIdx.x * kTbBlock + threadIdx.x; i < F.n; i += stride) {
        if (!((enter[i] >> T.index) & 1u)) { slot_of[i] = kTbNoSlot; continue; }
        TbFlow f;
        tb_load(F, 0u, i, f);
        uint32_t u[kTbMaxUnits];
#pragma unroll
        for (uint32_t k = 0; k < kTbMaxUnits; k++) u[k] = 0;
        uint32_t at = 0;
        for (uint32_t c = 0; c < T.n_cols; c++) {
            uint32_t a[4], v;
            tb_column(T, c, f, a, v);
            if (tb_col_is_addr(T.col[c])) {
#pragma unroll
                for (uint32_t k = 0; k < 4; k++) tb_set_unit(u, at + k, a[k]);
                at += 4;
            } else {
                tb_set_unit(u, at, v);
                at += 1;
            }
        }
        uint64_t raw[kTbRawWords];
#pragma unroll
        for (uint32_t j = 0; j < kTbRawWords; j++) raw[j] = (uint64_t)u[2 * j] | ((uint64_t)u[2 * j + 1] << 32);
        slot_of[i] = tb_claim(T, ctl, raw);
    }
}

__global__ __launch_bounds__(kTbBlock) void k_tb_fold(TbFlows F, TbTableDev T, uint32_t need, TbCtl* ctl, const uint32_t* __restrict__ slot_of) {
    if (tb_over(ctl, T.index)) return;
    const uint64_t stride = (uint64_t)gridDim.x * kTbBlock;
    for (uint64_t i = (uint64_t)blockIdx.x * kTbBlock + threadIdx.x; i < F.n; i += stride) {
        const uint32_t s = slot_of[i];
        bool fresh = false;
        uint32_t id = 0;
        if (s != kTbNoSlot) {
            TbFlow f;
            tb_load(F, need, i, f);
            id = (uint32_t)ald(T.slots + (size_t)s * kTbSlotWords + kTbIdWord) - 1u;     // < max_keys: no overflow in this table
            uint64_t* c = T.call + (size_t)id * T.call_words;
            fresh = aadd(c, (uint64_t)1) == 0;
            amax(c + 1, (uint64_t)(uint32_t)~(uint32_t)i);                               // n <= 2^32 - 2: never zero
            amax(c + 2, (uint64_t)(uint32_t)i + 1);
            for (uint32_t j = 0; j < T.n_src; j++) {
                const uint64_t v = tb_value(T, j, f);
                uint64_t* q = c + kTbCallHead + kTbSrcWords * j;
                if (v & 0xffffffffull) aadd(q, (uint64_t)(v & 0xffffffffull));
                if (v >> 32) aadd(q + 1, (uint64_t)(v >> 32));
                amax(q + 2, ~v);
                amax(q + 3, v);
            }
        }
        const unsigned long long born = __ballot(fresh);                                 // the wave's new ids take their places together
        if (fresh) {
            const int lane = (int)(threadIdx.x & 63), leader = __ffsll(born) - 1;
            uint32_t base = 0;
            if (lane == leader) base = aadd(&ctl->touched[T.index], (uint32_t)__popcll(born));
            base = __shfl(base, leader);
            T.touched[base + (uint32_t)__popcll(born & ((1ull << lane) - 1ull))] = id;   // at most one place per id of the table: < max_keys
        }
    }
}

__global__ __launch_bounds__(kTbBlock) void k_tb_finish(TbFlows F, TbTableDev T, uint32_t need, TbCtl* ctl, const uint32_t* __restrict__ slot_of) {
    if (tb_over(ctl, T.index)) return;
    const uint64_t stride = (uint64_t)gridDim.x * kTbBlock;
    for (uint64_t i = (uint64_t)blockIdx.x * kTbBlock + threadIdx.x; i < F.n; i += stride) {
        const uint32_t s = slot_of[i];
        if (s == kTbNoSlot) continue;
        const uint32_t id = (uint32_t)T.slots[(size_t)s * kTbSlotWords + kTbIdWord] - 1u;
        uint64_t* c = T.call + (size_t)id * T.call_words;
        const bool first = c[1] == (uint64_t)(uint32_t)~(uint32_t)i, last = c[2] == (uint64_t)(uint32_t)i + 1;
        if (!first && !last) continue;
        TbFlow f;
        tb_load(F, need, i, f);
        for (uint32_t j = 0; j < T.n_src; j++) {
            const uint64_t v = tb_value(T, j, f);
            uint64_t* q = c + kTbCallHead + kTbSrcWords * j;
            if (first) q[4] = v;
            if (last) q[5] = v;
        }
    }
}

__global__ __launch_bounds__(kTbBlock) void k_tb_emit(TbTableDev T, uint32_t m, uint64_t* __restrict__ slice) {
    const uint32_t e = blockIdx.x * kTbBlock + threadIdx.x;
    if (e >= m) return;
    const uint32_t id = T.touched[e], ew = kTbEntryHead + kTbSrcWords * T.n_src;
    uint64_t* c = T.call + (size_t)id * T.call_words;
    uint64_t* o = slice + (size_t)e * ew;
    o[0] = (uint64_t)id | (c[0] << 32);                                                  // n < 2^32
    for (uint32_t j = 0; j < T.n_src; j++) {
        const uint64_t* q = c + kTbCallHead + kTbSrcWords * j;
        uint64_t* w = o + kTbEntryHead + kTbSrcWords * j;
        w[0] = q[0]; w[1] = q[1]; w[2] = ~q[2]; w[3] = q[3]; w[4] = q[4]; w[5] = q[5];
        T.lastval[(size_t)j * T.max_keys + id] = q[5];
    }
    for (uint32_t k = 0; k < T.call_words; k++) c[k] = 0;
}

__global__ __launch_bounds__(kTbBlock) void k_tb_merge(TbRuleDev R, const uint64_t* __restrict__ slice, uint32_t m) {
    const uint32_t e = blockIdx.x * kTbBlock + threadIdx.x;
    if (e >= m) return;
    const uint64_t* o = slice + (size_t)e * (kTbEntryHead + kTbSrcWords * R.n_src);
    const uint32_t id = (uint32_t)o[0];
    if (id >= R.n_keys) return;                                                          // cannot happen: every id of a slice was given before it
    const uint64_t n = o[0] >> 32;
    const uint64_t* p = o + kTbEntryHead + kTbSrcWords * R.src_slot;
    uint64_t* a = R.acc + (size_t)id * kTbAccWords;
    const uint64_t had = a[0] & ~kTbNegSeen;
    const uint64_t neg = (R.src_signed && p[2] < kTbBias) ? kTbNegSeen : 0ull;
    if (R.op == NFAGG_TB_OP_SUM || R.op == NFAGG_TB_OP_AVG) {
        const uint64_t lo = p[0] + (p[1] << 32), hi = (p[1] >> 32) + (lo < p[0] ? 1ull : 0ull);     // the slice's 128-bit sum
        const uint64_t s = a[1] + lo;
        a[2] += hi + (s < lo ? 1ull : 0ull);
        a[1] = s;
    } else if (R.op == NFAGG_TB_OP_MIN) {
        if (had == 0 || p[2] < a[1]) a[1] = p[2];
    } else if (R.op == NFAGG_TB_OP_MAX) {
        if (had == 0 || p[3] > a[1]) a[1] = p[3];
    } else if (R.op == NFAGG_TB_OP_DIFF) {
        if (had == 0) a[1] = p[4];
    }
    a[0] = ((a[0] & ~kTbNegSeen) + n) | (a[0] & kTbNegSeen) | neg;
}

// The correctly rounded float64 of the 128-bit unsigned integer (hi, lo): the top 64 bits with everything below them folded
// into the lowest one (sticky), converted once (round to nearest even; eleven bits lie below the result's last place, so the
// sticky bit cannot change a tie that is none), then scaled by a power of two, which is exact.
NF_DEV double tb_u128_to_double(uint64_t hi, uint64_t lo) {
    if (hi == 0) return (double)lo;
    const int sh = 64 - __clzll((long long)hi);                                          // 1..64: bits of hi in use
    uint64_t top = sh == 64 ? hi : (hi << (64 - sh)) | (lo >> sh);
    const uint64_t below = sh == 64 ? lo : lo << (64 - sh);
    if (below) top |= 1ull;
    return ldexp((double)top, sh);
}

NF_DEV double tb_plain_to_double(uint64_t v, bool is_signed) { return is_signed ? (double)(int64_t)(v ^ kTbBias) : (double)v; }

__global__ __launch_bounds__(kTbBlock) void k_tb_value(TbRuleDev R) {
    const uint32_t id = blockIdx.x * kTbBlock + threadIdx.x;
    if (id >= R.n_keys) return;
    const uint64_t* a = R.acc + (size_t)id * kTbAccWords;
    const uint64_t n = a[0] & ~kTbNegSeen;
    const bool sg = R.src_signed != 0;
    double v = 0.0;
    uint32_t flags = 0;
    if (R.op == NFAGG_TB_OP_SUM || R.op == NFAGG_TB_OP_AVG) {
        if (n) {
            uint64_t lo = a[1], hi = a[2];
            if (sg) {                                                                    // the values were stored with bit 63 flipped: take n * 2^63 away
                const uint64_t blo = n << 63, bhi = n >> 1;
                hi = hi - bhi - (lo < blo ? 1ull : 0ull);
                lo -= blo;
            }
            const bool negative = (hi >> 63) != 0;
            if (negative) { lo = ~lo + 1; hi = ~hi + (lo == 0 ? 1ull : 0ull); }
            v = tb_u128_to_double(hi, lo);
            if (negative) v = -v;
            if (negative || (a[0] & kTbNegSeen) || hi != 0 || lo >= (1ull << 53)) flags = NFAGG_TB_INEXACT;
            if (R.op == NFAGG_TB_OP_AVG) v = v / (double)n;
        }
    } else if (R.op == NFAGG_TB_OP_COUNT) {
        v = (double)n;
    } else if (R.op == NFAGG_TB_OP_MIN) {
        v = n ? tb_plain_to_double(a[1], sg) : 1.7976931348623157e308;
    } else if (R.op == NFAGG_TB_OP_MAX) {
        v = n ? tb_plain_to_double(a[1], sg) : -1.7976931348623157e308;
    } else if (R.op == NFAGG_TB_OP_LAST) {
        v = tb_plain_to_double(R.lastval[id], sg);
    } else if (R.op == NFAGG_TB_OP_DIFF) {
        v = n ? tb_plain_to_double(R.lastval[id], sg) - tb_plain_to_double(a[1], sg) : 0.0;
    }
    R.value[id] = v;
    R.flags[id] = (uint8_t)flags;
    const uint64_t bits = (uint64_t)__double_as_longlong(v);
    const uint64_t ord = bits ^ ((bits >> 63) ? ~0ull : (1ull << 63));                   // unsigned order = Go's < on float64
    R.ord[id] = R.reversed ? ~ord : ord;
}

__global__ __launch_bounds__(kTbBlock) void k_tb_copy_all(TbRuleDev R, nfagg_tb_result* __restrict__ out) {
    const uint32_t id = blockIdx.x * kTbBlock + threadIdx.x;
    if (id >= R.n_keys) return;
    nfagg_tb_result r;
    r.key = id; r.flags = R.flags[id]; r.value = R.value[id];
    out[id] = r;
}

// One pass of the radix select: the byte at `shift` of every ord that carries the prefix found so far.
__global__ __launch_bounds__(kTbBlock) void k_tb_hist(TbRuleDev R, TbSelect* sel, uint32_t shift) {
    __shared__ uint32_t h[256];
    h[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t prefix = sel->prefix, mask = sel->mask;
    const uint32_t stride = gridDim.x * kTbBlock;
    for (uint32_t id = blockIdx.x * kTbBlock + threadIdx.x; id < R.n_keys; id += stride) {
        const uint64_t o = R.ord[id];
        if ((o & mask) == prefix) atomicAdd(&h[(uint32_t)(o >> shift) & 0xffu], 1u);
    }
    __syncthreads();
    if (h[threadIdx.x]) atomicAdd(&sel->hist[threadIdx.x], h[threadIdx.x]);
}
static_assert(kTbBlock == 256, "k_tb_hist: one lane per bin");

__global__ void k_tb_want(TbSelect* sel, uint32_t k) {
    if (threadIdx.x == 0 && blockIdx.x == 0) sel->want = k;
}

// The byte in which the want-th best lies, from the top; what is above it is taken whole.
__global__ void k_tb_pick(TbSelect* sel, uint32_t shift) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    uint32_t want = sel->want;
    uint32_t d = 255;
    for (;; d--) {
        const uint32_t c = sel->hist[d];
        if (want <= c || d == 0) break;
        want -= c;
    }
    sel->want = want;
    sel->prefix |= (uint64_t)d << shift;
    sel->mask |= 0xffull << shift;
    for (uint32_t k = 0; k < 256; k++) sel->hist[k] = 0;
}

// sel->prefix is the k-th best ord and sel->want the ties that still fit: everything above it, then that many of its equals.
__global__ __launch_bounds__(kTbBlock) void k_tb_compact(TbRuleDev R, TbSelect* sel, uint32_t k, uint64_t* __restrict__ pairs) {
    const uint32_t id = blockIdx.x * kTbBlock + threadIdx.x;
    if (id >= R.n_keys) return;
    const uint64_t o = R.ord[id], kth = sel->prefix;
    const uint32_t want = sel->want;
    uint32_t at = kTbNoSlot;
    if (o > kth) at = atomicAdd(&sel->above, 1u);                                        // k - want of them
    else if (o == kth) {
        const uint32_t t = atomicAdd(&sel->ties, 1u);
        if (t < want) at = k - want + t;
    }
    if (at < k) { pairs[at] = o; pairs[kTbSortMax + at] = id; }
}

__global__ __launch_bounds__(kTbBlock) void k_tb_take_all(TbRuleDev R, uint64_t* __restrict__ pairs) {
    const uint32_t id = blockIdx.x * kTbBlock + threadIdx.x;
    if (id < R.n_keys && id < kTbSortMax) { pairs[id] = R.ord[id]; pairs[kTbSortMax + id] = id; }
}

// One workgroup: the k pairs into LDS, padded to a power of two with pairs that sort last, a bitonic sort by (ord descending,
// id ascending), then the results.
__global__ __launch_bounds__(1024) void k_tb_sort(TbRuleDev R, uint32_t k, const uint64_t* __restrict__ pairs, nfagg_tb_result* __restrict__ out) {
    __shared__ uint64_t so[kTbSortMax];
    __shared__ uint32_t si[kTbSortMax];
    uint32_t p2 = 1;
    while (p2 < k) p2 <<= 1;
    for (uint32_t x = threadIdx.x; x < p2; x += 1024) {
        so[x] = x < k ? pairs[x] : 0ull;
        si[x] = x < k ? (uint32_t)pairs[kTbSortMax + x] : 0xffffffffu;
    }
    __syncthreads();
    for (uint32_t size = 2; size <= p2; size <<= 1)
        for (uint32_t step = size >> 1; step > 0; step >>= 1) {
            for (uint32_t x = threadIdx.x; x < p2; x += 1024) {
                const uint32_t y = x ^ step;
                if (y > x) {
                    const uint64_t ox = so[x], oy = so[y];
                    const uint32_t ix = si[x], iy = si[y];
                    const bool x_first = ox > oy || (ox == oy && ix < iy);               // x belongs before y in the final order
                    const bool up = (x & size) == 0;
                    if (up ? !x_first : x_first) { so[x] = oy; so[y] = ox; si[x] = iy; si[y] = ix; }
                }
            }
            __syncthreads();
        }
    for (uint32_t x = threadIdx.x; x < k; x += 1024) {
        const uint32_t id = si[x];
        nfagg_tb_result r;
        r.key = id; r.flags = id < R.n_keys ? R.flags[id] : 0u; r.value = id < R.n_keys ? R.value[id] : 0.0;
        out[x] = r;
    }
}

__global__ __launch_bounds__(kTbBlock) void k_tb_gather_keys(TbTableDev T, uint32_t n_keys, const uint32_t* __restrict__ ids, uint32_t n, uint64_t* __restrict__ out,
                                                             uint32_t* bad) {
    const uint32_t e = blockIdx.x * kTbBlock + threadIdx.x;
    if (e >= n) return;
    const uint32_t id = ids[e];
    if (id >= n_keys || id >= T.max_keys) { *bad = 1u; return; }
    const uint32_t s = T.slot_of_id[id] & T.mask;
    for (uint32_t k = 0; k < kTbSlotWords; k++) out[(size_t)e * kTbSlotWords + k] = T.slots[(size_t)s * kTbSlotWords + k];
}

static unsigned tb_flow_blocks(uint64_t n) {
    const uint64_t want = (n + kTbFlowsPerBlock - 1) / kTbFlowsPerBlock;
    return (unsigned)(want < 1 ? 1 : want < kTbMaxBlocks ? want : kTbMaxBlocks);
}
static unsigned tb_item_blocks(uint32_t n) { return (n + kTbBlock - 1) / kTbBlock; }

static uint32_t tb_need(const TbFlows& F, const TbTableDev* T, uint32_t n_tables) {
    uint32_t need = 0;
    for (uint32_t t = 0; t < n_tables; t++)
        for (uint32_t j = 0; j < T[t].n_src; j++) {
            const uint32_t s = T[t].src[j];
            need |= s == NFAGG_MET_VALUE_RTT_NS ? kTbNeedAdditional : s == NFAGG_MET_VALUE_DNS_LATENCY_MS ? kTbNeedDns :
                    (s == NFAGG_MET_VALUE_DROP_BYTES || s == NFAGG_MET_VALUE_DROP_PACKETS) ? kTbNeedDrops : 0u;
        }
    // a part whose array is missing, or all of them without the present bytes, is absent for every flow
    return need & (!F.present ? 0u : (F.additional ? kTbNeedAdditional : 0u) | (F.dns ? kTbNeedDns : 0u) | (F.drops ? kTbNeedDrops : 0u));
}

hipError_t launch_tb_presence(const TbFlows& F, const TbTableDev* T, uint32_t n_tables, TbCtl* ctl, uint8_t* enter, hipStream_t s) {
    TbAllTables A{};
    for (uint32_t t = 0; t < n_tables; t++) A.t[t] = T[t];
    A.n = n_tables;
    A.need = tb_need(F, T, n_tables);
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_tb_presence, dim3(tb_flow_blocks(F.n)), dim3(kTbBlock), 0, s, F, A, ctl, enter);
    return hipGetLastError();
}

hipError_t launch_tb_fold(const TbFlows& F, const TbTableDev& T, TbCtl* ctl, const uint8_t* enter, uint32_t* slot_of, hipStream_t s) {
    const uint32_t need = tb_need(F, &T, 1);
    const dim3 grid(tb_flow_blocks(F.n)), block(kTbBlock);
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_tb_claim, grid, block, 0, s, F, T, ctl, enter, slot_of);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_tb_fold, grid, block, 0, s, F, T, need, ctl, (const uint32_t*)slot_of);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_tb_finish, grid, block, 0, s, F, T, need, ctl, (const uint32_t*)slot_of);
    return hipGetLastError();
}

hipError_t launch_tb_emit(const TbTableDev& T, uint32_t m, uint64_t* slice, hipStream_t s) {
    if (!m) return hipSuccess;
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_tb_emit, dim3(tb_item_blocks(m)), dim3(kTbBlock), 0, s, T, m, slice);
    return hipGetLastError();
}

hipError_t launch_tb_merge(const TbRuleDev& R, const uint64_t* slice, uint32_t m, hipStream_t s) {
    if (!m) return hipSuccess;
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_tb_merge, dim3(tb_item_blocks(m)), dim3(kTbBlock), 0, s, R, slice, m);
    return hipGetLastError();
}

hipError_t launch_tb_value(const TbRuleDev& R, hipStream_t s) {
    if (!R.n_keys) return hipSuccess;
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_tb_value, dim3(tb_item_blocks(R.n_keys)), dim3(kTbBlock), 0, s, R);
    return hipGetLastError();
}

hipError_t launch_tb_select(const TbRuleDev& R, uint32_t k, TbSelect* sel, uint64_t* pairs, nfagg_tb_result* out, hipStream_t s) {
    if (!R.n_keys) return hipSuccess;
    const dim3 grid(tb_item_blocks(R.n_keys)), block(kTbBlock);
    (void)hipGetLastError();
    if (k == 0) {
        hipLaunchKernelGGL(k_tb_copy_all, grid, block, 0, s, R, out);
        return hipGetLastError();
    }
    if (k > R.n_keys || k > kTbSortMax) return hipErrorInvalidValue;
    hipError_t e;
    if (k == R.n_keys) {
        hipLaunchKernelGGL(k_tb_take_all, grid, block, 0, s, R, pairs);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    } else {
        if ((e = hipMemsetAsync(sel, 0, sizeof(TbSelect), s)) != hipSuccess) return e;
        hipLaunchKernelGGL(k_tb_want, dim3(1), dim3(64), 0, s, sel, k);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        const dim3 hgrid(grid.x < 1024u ? grid.x : 1024u);
        for (int b = 7; b >= 0; b--) {
            hipLaunchKernelGGL(k_tb_hist, hgrid, block, 0, s, R, sel, (uint32_t)(8 * b));
            if ((e = hipGetLastError()) != hipSuccess) return e;
            hipLaunchKernelGGL(k_tb_pick, dim3(1), dim3(64), 0, s, sel, (uint32_t)(8 * b));
            if ((e = hipGetLastError()) != hipSuccess) return e;
        }
        hipLaunchKernelGGL(k_tb_compact, grid, block, 0, s, R, sel, k, pairs);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_tb_sort, dim3(1), dim3(1024), 0, s, R, k, (const uint64_t*)pairs, out);
    return hipGetLastError();
}

hipError_t launch_tb_gather_keys(const TbTableDev& T, uint32_t n_keys, const uint32_t* ids, uint32_t n, uint64_t* out, uint32_t* bad, hipStream_t s) {
    if (!n) return hipSuccess;
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_tb_gather_keys, dim3(tb_item_blocks(n)), dim3(kTbBlock), 0, s, T, n_keys, ids, n, out, bad);
    return hipGetLastError();
}

}  // namespace nfagg
