// nfagg_timebased.h — flowlogs-pipeline's `extract timebased` on the device (include/nfagg.h, "extract timebased"; DESIGN.md
// §4.7r): what the host hands the kernels of nfagg_timebased.hip, and the layouts they share. Host + device.
//
// A TABLE is one distinct index-key list. Its key is up to ten 32-bit UNITS in the order of the list: an address is four units,
// every other column one. The units are packed into kTbRawWords 64-bit raw words (unit 2j low, unit 2j + 1 high), and the raw
// words are cut into KEY WORDS of 63 bits each with bit 63 set: key word j = kTbMark | bits [63 j, 63 j + 63) of the raw string.
// So no key word is ever the empty value 0 although an address may be all zero, and the widest key (40 bytes, 320 bits) takes six
// key words. tb_hash() of the raw words places the key; probing is linear.
//
// Slot of a table (kTbSlotWords = 8 words, one 64-byte line): key words 0..5 (those past the table's n_words stay 0), word 6 =
// the slot's dense id + 1, written by the lane that set word 0, word 7 unused. The table is persistent: slots are never freed
// except by reset, and an id, once given, stays.
//
// Call area of a table, indexed by the dense id (kTbCallHead + kTbSrcWords * n_src words per id), zero between calls:
//   [0] n            flows of this call with the key
//   [1] ~first       max over ~(flow index): the least index
//   [2] last + 1     max over (flow index + 1): the greatest index
//   [3] unused
//   per value source j at [4 + 6 j]: sum of the low halves, sum of the high halves (neither can wrap: n < 2^32), ~min, max,
//   the value at the least index, the value at the greatest index.
// Values are 64-bit patterns ordered as unsigned integers: an unsigned source (Bytes, Packets, PktDrop*) as it is, a signed one
// (TimeFlowRttNs, DnsLatencyMs: int64 in the reference) with bit 63 flipped, so that one order serves both.
//
// Slice (one call's partials of one table, compact, stamped by the host): kTbEntryHead + kTbSrcWords * n_src words per touched
// key: [0] id | n << 32 (each in a 32-bit half of its own: never pack an index and a count into one dword), then per source sum_lo, sum_hi, min, max, first, last.
//
// Accumulator of a rule during its evaluation, kTbAccWords words per id: [0] n (bit 63: a negative value was seen), [1], [2]: the
// 128-bit sum (sum, avg), or the extremum (min, max), or the first value inside the window (diff).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "nfagg_flp.h"

namespace nfagg {

constexpr uint32_t kTbMaxTables = NFAGG_TB_MAX_TABLES, kTbMaxRules = NFAGG_TB_MAX_RULES, kTbMaxCols = NFAGG_TB_MAX_COLUMNS, kTbMaxSrc = NFAGG_TB_MAX_VALUES;
constexpr uint32_t kTbMaxUnits = 10, kTbRawWords = 5, kTbKeyWords = 6, kTbSlotWords = 8, kTbIdWord = 6, kTbMinSlots = 1024;
constexpr uint32_t kTbCallHead = 4, kTbEntryHead = 1, kTbSrcWords = 6, kTbAccWords = 3;
constexpr uint32_t kTbNoSlot = 0xFFFFFFFFu;
constexpr uint64_t kTbMark = 1ull << 63, kTbBias = 1ull << 63, kTbNegSeen = 1ull << 63;
constexpr uint64_t kTbHashSeed = 0x6E66616767207462ull;      // "nfagg tb"
static_assert(kTbMaxUnits * 32 <= kTbKeyWords * 63 && kTbMaxUnits <= 2 * kTbRawWords, "the key and id fields");
static_assert(sizeof(nfagg_tb_result) == 16 && sizeof(nfagg_tb_key) == 64, "result and key layout");

// Column kinds. A Kubernetes column is kTbColK8s + 16 * side + field.
enum : uint32_t { kTbColSrcAddr = 1, kTbColDstAddr, kTbColSrcPort, kTbColDstPort, kTbColProto, kTbColSrcLabel, kTbColDstLabel, kTbColDirection, kTbColK8s = 32 };
NF_HD bool tb_col_is_addr(uint32_t kind) { return kind == kTbColSrcAddr || kind == kTbColDstAddr; }
NF_HD bool tb_col_is_k8s(uint32_t kind) { return kind >= kTbColK8s; }
NF_HD bool tb_src_signed(uint32_t src) { return src == NFAGG_MET_VALUE_RTT_NS || src == NFAGG_MET_VALUE_DNS_LATENCY_MS; }

NF_HD uint64_t tb_hash(const uint64_t (&raw)[kTbRawWords]) {
    uint64_t h = kTbHashSeed;
    for (uint32_t i = 0; i < kTbRawWords; i++) h = (rotl64(h, 27) ^ raw[i]) * kMul;
    return fmix64(h);
}
// Key word j of the raw string: 63 bits from bit 63 j on, under the mark.
NF_HD uint64_t tb_key_word(const uint64_t (&raw)[kTbRawWords], uint32_t j) {
    const uint32_t at = 63u * j, idx = at >> 6, sh = at & 63u;
    uint64_t v = idx < kTbRawWords ? raw[idx] >> sh : 0ull;
    if (sh && idx + 1 < kTbRawWords) v |= raw[idx + 1] << (64u - sh);
    return kTbMark | (v & ~kTbMark);
}

// Control words, persistent (n_keys, failed state is the host's) and per call; the host zeroes the per-call part before a call.
struct TbCtl {
    uint32_t n_keys[kTbMaxTables];       // persistent: ids given so far (beyond max_keys once a table has overflowed)
    uint32_t overflow[kTbMaxTables];     // per call: a claim got an id >= max_keys, or a probe walked the whole table
    uint32_t touched[kTbMaxTables];      // per call: keys this call has touched = entries of its slice
    uint32_t pad_[kTbMaxTables];
    uint64_t n_missing;                  // per call: entering flows that lack a value source of their table
    uint64_t pad2_;
};
static_assert(sizeof(TbCtl) == 80, "TbCtl layout");

// One table as the kernels take it.
struct TbTableDev {
    uint64_t* slots;                     // (mask + 1) * kTbSlotWords
    uint64_t* call;                      // max_keys * call_words
    uint64_t* lastval;                   // n_src arrays of max_keys: the value of the newest entry a key ever had
    uint32_t* touched;                   // max_keys ids
    uint32_t* slot_of_id;                // persistent: the slot that carries id, written with the id
    const uint32_t* cls[kTbMaxCols];     // a Kubernetes column: the rows' classes (of the side the column names)
    const uint8_t* cls_ok[kTbMaxCols];   //   and per class 1 when its text is present and not empty
    uint64_t label_ok[kNetMaxCidrs / 64];   // bit k: label k has a text that is not empty
    uint32_t col[kTbMaxCols];            // kinds
    uint32_t src[kTbMaxSrc];             // NFAGG_MET_VALUE_*
    uint32_t n_cols, n_src, n_words, mask, max_keys, call_words, n_rows, index;
};

// The flows of a call.
struct TbFlows {
    const void* recs;
    const uint32_t* k8s_rows;            // 2 per flow, or nullptr
    const uint2* net_rows;               // or nullptr
    const uint8_t* present;              // the feature parts, as MetSpecDev has them; nullptr: none
    const uint8_t* additional;
    const uint8_t* dns;
    const uint8_t* drops;
    uint64_t n;
};

// One rule's evaluation.
struct TbRuleDev {
    uint64_t* acc;                       // n_keys * kTbAccWords, zeroed by the host
    double* value;                       // n_keys
    uint64_t* ord;                       // n_keys: the order-preserving integer of value (inverted for `reversed`): greater is better
    uint8_t* flags;                      // n_keys
    const uint64_t* lastval;             // the rule's source
    uint32_t op, src_slot, src_signed, reversed, n_keys, n_src;
};

// The selection's state on the device: the prefix found so far, how many are still wanted among the keys that share it.
struct TbSelect {
    uint64_t prefix, mask;
    uint32_t want, above, ties, pad_;    // above / ties: the compaction's cursors
    uint32_t hist[256];
};

hipError_t launch_tb_presence(const TbFlows& F, const TbTableDev* T, uint32_t n_tables, TbCtl* ctl, uint8_t* enter, hipStream_t s);
// claim, fold and finish of one table: slot_of is u32[n] scratch.
hipError_t launch_tb_fold(const TbFlows& F, const TbTableDev& T, TbCtl* ctl, const uint8_t* enter, uint32_t* slot_of, hipStream_t s);
// The touched keys' partials into `slice` (m entries), the call area cleared, lastval brought up to date.
hipError_t launch_tb_emit(const TbTableDev& T, uint32_t m, uint64_t* slice, hipStream_t s);
// One slice (m entries of a table with n_src sources) into a rule's accumulators.
hipError_t launch_tb_merge(const TbRuleDev& R, const uint64_t* slice, uint32_t m, hipStream_t s);
// Accumulators -> value, flags and ord of every key.
hipError_t launch_tb_value(const TbRuleDev& R, hipStream_t s);
// top_k == 0: every key into out. Else the k best (k <= n_keys, k <= NFAGG_TB_MAX_TOPK), sorted, into out; sel: a TbSelect; pairs: 2 * 4096 words.
hipError_t launch_tb_select(const TbRuleDev& R, uint32_t k, TbSelect* sel, uint64_t* pairs, nfagg_tb_result* out, hipStream_t s);
// keys read-back: the slot (kTbSlotWords words) of each of n ids into out; *bad = 1 when an id is not below n_keys.
hipError_t launch_tb_gather_keys(const TbTableDev& T, uint32_t n_keys, const uint32_t* ids, uint32_t n, uint64_t* out, uint32_t* bad, hipStream_t s);

}  // namespace nfagg
