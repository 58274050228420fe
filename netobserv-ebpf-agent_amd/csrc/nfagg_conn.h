// nfagg_conn.h — the per-call fold under flowlogs-pipeline's `extract conntrack` (include/nfagg.h, "Conversation tracking"):
// the gob + FNV-64a bytes of the three hashes, the layout of a connection's slot, and what the host hands the kernels of
// nfagg_conn.hip. Host + device.
//
// Hashes: a field is hashed as the message of a fresh gob encoder, [count][type id, zigzag][0x00][value]. Every byte goes
// through a sink's put(); FnvSink IS the FNV-64a state, so no byte is ever stored. The address text is written twice by its
// caller: once into a counting sink for the two length bytes, once into the FNV sink.
//
// Slot of the connection table, sixteen 64-bit words (a table is a power of two of slots, at least kConnMinSlots and at least
// twice min(the caller's cap, the call's flows), probed linearly from the low bits of fmix64(hashTotal)):
//   0  key 0 = 1<<63 | hashTotal >> 32          bit 63 set: the all-zero "empty" value is never a key, and hashTotal == 0
//   1  key 1 = 1<<63 | hashTotal & 0xFFFFFFFF   needs no special case
//   2  ~first_idx (low 32 bits) | last_idx << 32            every one of these only ever grows from zero under an atomic
//   3  ~first_fin_idx (low) | flags_or << 32                max / or: "none" is zero, and ~0 is NFAGG_CONN_NO_IDX
//   4..9   flows[2], bytes[2], packets[2]                   bytes 32..79 of nfagg_conn_partial as they stand
//   10 ~(start_ms ^ 1<<63) under max = the least start      the bias turns int64 order into uint64 order
//   11   end_ms ^ 1<<63   under max = the greatest end
//   12 first_hash_a, stored by the one flow at first_idx
//   13..15 zero
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "../../include/nfagg.h"
#include "nfagg_hash.h"

namespace nfagg {

constexpr uint64_t kFnvOffset = 0xcbf29ce484222325ull, kFnvPrime = 0x100000001b3ull;
constexpr uint64_t kConnMark = 1ull << 63, kConnBias = 1ull << 63;
constexpr uint32_t kConnSlotWords = 16, kConnMinSlots = 1024, kConnMaxConns = NFAGG_CONN_MAX_CONNS;
constexpr uint32_t kConnNoSlot = 0xFFFFFFFFu;
static_assert(sizeof(nfagg_conn_partial) == 128 && kConnSlotWords * 8 == 128 && offsetof(nfagg_conn_partial, first_idx) == 16 &&
              offsetof(nfagg_conn_partial, flows) == 32 && offsetof(nfagg_conn_partial, start_ms_min) == 80 && offsetof(nfagg_conn_partial, pad_) == 96,
              "nfagg_conn_partial layout");
static_assert(sizeof(nfagg_conn_options) == 24, "nfagg_conn_options layout");

struct FnvSink {
    uint64_t h = kFnvOffset;
    NF_HD void put(uint8_t b) { h = (h ^ b) * kFnvPrime; }
};

// gob's message for a uint8 / uint16 value v: 03 06 00 v below 128, else the negated byte count and the minimal big-endian bytes.
template <typename S> NF_HD void gob_uint(S& s, uint32_t v) {
    if (v < 128u) { s.put(3); s.put(6); s.put(0); s.put((uint8_t)v); }
    else if (v < 256u) { s.put(4); s.put(6); s.put(0); s.put(0xff); s.put((uint8_t)v); }
    else { s.put(5); s.put(6); s.put(0); s.put(0xfe); s.put((uint8_t)(v >> 8)); s.put((uint8_t)v); }
}
// ... and the head of a string's message; its len bytes follow. An address text has at most 39 bytes: one length byte each.
template <typename S> NF_HD void gob_string_head(S& s, uint32_t len) { s.put((uint8_t)(3 + len)); s.put(0x0c); s.put(0); s.put((uint8_t)len); }
template <typename S> NF_HD void put_be64(S& s, uint64_t v) {
    for (int k = 7; k >= 0; k--) s.put((uint8_t)(v >> (8 * k)));
}
// hash.go:53-71: the common group's hash, then the smaller of the endpoint hashes, then the other.
NF_HD uint64_t conn_total(uint64_t common, uint64_t a, uint64_t b) {
    FnvSink t;
    put_be64(t, common); put_be64(t, a < b ? a : b); put_be64(t, a < b ? b : a);
    return t.h;
}
NF_HD bool conn_tracked(uint32_t eth, uint32_t proto) { return (eth == 0x0800u || eth == 0x86DDu) && (proto == 6u || proto == 17u || proto == 132u); }

// Control words at the head of the slot scratch, zeroed with it by the call's one memset, and the call's one read-back.
struct ConnCtl {
    uint32_t claimed;        // slots whose first word has been set so far
    uint32_t overflow;       // a probe walked the whole table (claimed and overflow are read as one 64-bit word)
    uint32_t count;          // k_conn_emit: occupied slots
    uint32_t over;           // k_conn_emit: overflow || count > cap
    uint32_t discarded;      // flows the filter turned away
    uint32_t pad_[27];
};
static_assert(offsetof(ConnCtl, claimed) == 0 && offsetof(ConnCtl, overflow) == 4 && sizeof(ConnCtl) == 128, "ConnCtl layout");

struct ConnDev {
    uint64_t* slots;             // (mask + 1) slots of kConnSlotWords words
    ConnCtl* ctl;
    uint32_t* slot_of;           // per flow: its connection's slot, kConnNoSlot for a discarded flow
    uint64_t* hash_a;            // per flow: hashA (kept, not recomputed: DESIGN.md §4.7k)
    uint64_t* hash_ids;          // the caller's, or nullptr
    nfagg_conn_partial* out;     // the caller's
    int64_t now_sec, now_nsec;   // currentTime, normalised (0 <= nsec < 1e9)
    uint64_t mono_now;
    uint32_t mask, cap;
};

// The caller has zeroed ctl and the slots on s. claim: k_conn_claim; finish: k_conn_finish, then count, scan and emit
// (local_off: one word per slot; block_sum: one per kConnMinSlots slots; block_base: one more than that).
hipError_t launch_conn_claim(const void* d_recs, uint64_t n, const ConnDev& D, hipStream_t s);
hipError_t launch_conn_finish(const void* d_recs, uint64_t n, const ConnDev& D, uint32_t* d_local_off, uint32_t* d_block_sum, uint64_t* d_block_base, hipStream_t s);

}  // namespace nfagg
