// nfagg_variants.h — THE list of nfagg_config.ingest_variant values: what each number forces, and the dispatch rules over it.
// Host-only, plain C++17, no HIP: a host compiler builds it alone (tests/test_ingest_variants.py does, and holds every answer of
// the functions below against tests/golden/ingest_variant_paths.txt). The numbers are ABI: bench.py and the tests pass integers.
#pragma once
#include <cstdint>

namespace nfagg {

enum IngestVariant : int {
    kVariantDefault = 0, kVariantDirect = 1, kVariantCached512x2 = 3, kVariantCached256x4 = 4, kVariantCached1024h = 5,
    kVariantCachedTiming = 6, kVariantCached = 7, kVariantPass1Timing = 8, kVariantPass2Timing = 9, kVariantTwoPass = 10,
    kVariantTwoPassNoDoor = 11, kVariantDedupOneRound = 12, kVariantDedupNoFlush = 13, kVariantDedupNoFold = 14,
    kVariantDedupNoClaim = 15, kVariantDedupSortFirst = 16, kVariantPass1Free = 17, kVariantAblBase = 20, kVariantAblNoQueue = 21,
    kVariantAblNoFold = 22, kVariantAblNoQueueNoFold = 23, kVariantAblNoClaimNoQueue = 25, kVariantAblLoadsOnly = 27,
    kVariantAccountChain = 30,
};

enum class IngestPath { Direct, Cached, TwoPass, DedupDirect, DedupCached };
enum class Force : uint8_t { BySize, Direct, Cached, TwoPass };   // what a variant makes of the choice by batch size (TwoPass: accounter mode only)
enum class Avail : uint8_t { Shipping, DiagOnly, Never };         // libnfagg.so and libnfagg_diag.so / the latter (-DNFAGG_DIAG) only / no build
// the modes (nfagg_config.mode) in which a variant's kernels are built WITHOUT the sketch updates: the caller launches those itself
constexpr uint8_t kFused = 0, kUnfusedAccounter = 1, kUnfusedDedup = 2;

struct VariantRow {
    int number;
    Force accounter, dedup;        // NFAGG_MODE_ACCOUNTER / NFAGG_MODE_KERNEL_DEDUP
    Avail avail;
    bool exact;                    // results are right (false: a timing ablation)
    uint8_t unfused;
    const char* what;
};

// `Never` rows pin what the dispatch makes of a number no build accepts (nfagg_create refuses it first); a number without a row
// is treated as kUnlisted. 24, 26 and 28 stay retired: their result files name them.
constexpr VariantRow kVariants[] = {
    {kVariantDefault,           Force::BySize,  Force::BySize, Avail::Shipping, true,  kFused,            "the default: kernels chosen by batch size"},
    {kVariantDirect,            Force::Direct,  Force::Direct, Avail::Shipping, true,  kFused,            "direct per-record kernels always"},
    {2,                         Force::Cached,  Force::BySize, Avail::Never,    true,  kFused,            "retired: round 1's per-tile LDS variant"},
    {kVariantCached512x2,       Force::Cached,  Force::BySize, Avail::Shipping, true,  kFused,            "single-pass cached kernel, 2 workgroups per CU x 64 KB"},
    {kVariantCached256x4,       Force::Cached,  Force::BySize, Avail::Shipping, true,  kFused,            "single-pass cached kernel, 4 workgroups per CU x 32 KB"},
    {kVariantCached1024h,       Force::Cached,  Force::BySize, Avail::Shipping, true,  kFused,            "single-pass cached kernel, 1024 lanes over 512 entries, 2 per CU"},
    {kVariantCachedTiming,      Force::Cached,  Force::BySize, Avail::DiagOnly, true,  kUnfusedAccounter, "single-pass cached kernel, phase-timing build"},
    {kVariantCached,            Force::Cached,  Force::BySize, Avail::Shipping, true,  kFused,            "single-pass cached kernel always (1 workgroup per CU x 120 KB)"},
    {kVariantPass1Timing,       Force::TwoPass, Force::BySize, Avail::DiagOnly, true,  kUnfusedAccounter, "two-pass fold, pass-1 phase-timing build"},
    {kVariantPass2Timing,       Force::TwoPass, Force::BySize, Avail::DiagOnly, true,  kUnfusedAccounter, "two-pass fold, pass-2 phase-timing build"},
    {kVariantTwoPass,           Force::TwoPass, Force::Cached, Avail::Shipping, true,  kFused,            "two-pass fold / cached dedup passes whatever the batch size"},
    {kVariantTwoPassNoDoor,     Force::TwoPass, Force::BySize, Avail::Shipping, true,  kFused,            "two-pass fold, pass 1 without the admission filter"},
    {kVariantDedupOneRound,     Force::Cached,  Force::Cached, Avail::Shipping, true,  kFused,            "cached dedup passes always, no retry rounds in the partition pass"},
    {kVariantDedupNoFlush,      Force::Cached,  Force::Cached, Avail::DiagOnly, false, kUnfusedDedup,     "dedup partition pass ablation: no flush"},
    {kVariantDedupNoFold,       Force::Cached,  Force::Cached, Avail::DiagOnly, false, kUnfusedDedup,     "dedup partition pass ablation: no flush, no fold"},
    {kVariantDedupNoClaim,      Force::Cached,  Force::Cached, Avail::DiagOnly, false, kUnfusedDedup,     "dedup partition pass ablation: no flush, no fold, no claim"},
    {kVariantDedupSortFirst,    Force::Cached,  Force::Cached, Avail::Shipping, true,  kFused,            "cached dedup passes always, the partition pass always sorts its items first"},
    {kVariantPass1Free,         Force::TwoPass, Force::BySize, Avail::Shipping, true,  kFused,            "two-pass fold, pass 1 without its barriers (k_pass1_free)"},
    {18,                        Force::Cached,  Force::BySize, Avail::Never,    true,  kFused,            "retired: round 6's old-flush A/B (profiles/r06x_midsize_cache_entries.txt)"},
    {19,                        Force::Cached,  Force::BySize, Avail::Never,    true,  kFused,            "unassigned"},
    {kVariantAblBase,           Force::TwoPass, Force::BySize, Avail::DiagOnly, true,  kUnfusedAccounter, "pass-1 ablation series, nothing ablated (as 10, sketches unfused)"},
    {kVariantAblNoQueue,        Force::TwoPass, Force::BySize, Avail::DiagOnly, false, kUnfusedAccounter, "pass-1 ablation: spills counted, not queued"},
    {kVariantAblNoFold,         Force::TwoPass, Force::BySize, Avail::DiagOnly, false, kUnfusedAccounter, "pass-1 ablation: no fold into the cache entry"},
    {kVariantAblNoQueueNoFold,  Force::TwoPass, Force::BySize, Avail::DiagOnly, false, kUnfusedAccounter, "pass-1 ablation: no spill queueing, no fold"},
    {24,                        Force::TwoPass, Force::BySize, Avail::Never,    true,  kUnfusedAccounter, "retired: wave-level duplicate combining (profiles/r05x_wave_combining.txt)"},
    {kVariantAblNoClaimNoQueue, Force::TwoPass, Force::BySize, Avail::DiagOnly, false, kUnfusedAccounter, "pass-1 ablation: no cache claim, no spill queueing"},
    {26,                        Force::TwoPass, Force::BySize, Avail::Never,    false, kUnfusedAccounter, "retired: 64-byte queue stores (profiles/r05x_queue_stores.txt)"},
    {kVariantAblLoadsOnly,      Force::TwoPass, Force::BySize, Avail::DiagOnly, false, kUnfusedAccounter, "pass-1 ablation: loads, hash and barriers only"},
    {28,                        Force::TwoPass, Force::BySize, Avail::Never,    true,  kUnfusedAccounter, "retired: records requested two tiles ahead (profiles/r05x_pass1_two_tiles_ahead.txt)"},
    {kVariantAccountChain,      Force::BySize,  Force::BySize, Avail::Shipping, true,  kFused,            "as 0, but nfagg_account always takes its kernel chain"},
};
constexpr VariantRow kUnlisted = {-1, Force::Cached, Force::BySize, Avail::Never, true, kUnfusedAccounter, "not a variant"};

constexpr const VariantRow& variant_row(int variant) {
    for (const VariantRow& r : kVariants) if (r.number == variant) return r;
    return kUnlisted;
}

// Default kernel by batch size, measured on configs[1]'s stream, per call (round 3: profiles/r03_batch_size_sweep.txt; round 2:
// profiles/r02_batch_size_sweep.txt; round 1: profiles/r01e_batch_size_crossover.txt):
//   below 6 144 records the direct kernel (one record per lane, HBM atomics; no LDS cache to set up and flush);
//   below 384 Ki records (768 Ki in round 2) the single-pass LDS-cached kernel: 0.049 ms per 65 536 records against 0.063 ms for the launches
//     of the two-pass fold, 0.130 against 0.120 ms at 256 Ki;
//   from there the two-pass partitioned fold: 0.17 against 0.24 ms at 512 Ki, 0.26 against 0.41 ms at 1 Mi, 0.70 against 1.29 ms at
//     4 Mi (partitions scaled to the batch and a cheaper flush moved the crossover from 768 Ki to ~300 Ki this round).
constexpr uint64_t kDirectMaxBatch = 6144;
constexpr uint64_t kPartMinBatch = 3u << 17;   // 384 Ki (round 3: 0.114 against 0.128 ms at 256 Ki, 0.18 against 0.23 at 512 Ki)
constexpr uint64_t kDedupCachedMinBatch = 1u << 16;

constexpr bool ingest_variant_supported(int variant, bool diag_build) {
    const Avail a = variant_row(variant).avail;
    return a == Avail::Shipping || (diag_build && a == Avail::DiagOnly);
}
// mode: nfagg_config.mode (1 = NFAGG_MODE_KERNEL_DEDUP, else the accounter). With sketches on, the cached kernel fuses them (one
// launch): the default goes direct below kDirectMaxBatch only without them.
constexpr IngestPath ingest_path(int mode, int variant, uint64_t n, uint32_t sketch_flags) {
    const VariantRow& r = variant_row(variant);
    if (mode == 1) return r.dedup == Force::Direct || (r.dedup == Force::BySize && n < kDedupCachedMinBatch) ? IngestPath::DedupDirect : IngestPath::DedupCached;
    if (r.accounter == Force::TwoPass || (r.accounter == Force::BySize && n >= kPartMinBatch)) return IngestPath::TwoPass;
    if (r.accounter == Force::Direct || (r.accounter == Force::BySize && n < kDirectMaxBatch && sketch_flags == 0)) return IngestPath::Direct;
    return IngestPath::Cached;
}
// the call needs the spill queues (two-pass fold, cached dedup passes)
constexpr bool ingest_needs_spill(int mode, int variant, uint64_t n) {
    const IngestPath p = ingest_path(mode == 0 ? 0 : 1, variant, n, 0);
    return p == IngestPath::TwoPass || p == IngestPath::DedupCached;
}
// the fold kernels apply the sketch updates themselves (dedup mode: the partition pass's flushes feed them)
constexpr bool ingest_fuses_sketches(int mode, int variant, uint64_t n, uint32_t sketch_flags) {
    const IngestPath p = ingest_path(mode, variant, n, sketch_flags);
    const uint8_t unfused = variant_row(variant).unfused;
    if (mode == 1) return p == IngestPath::DedupCached && !(unfused & kUnfusedDedup);
    return mode == 0 && p != IngestPath::Direct && !(unfused & kUnfusedAccounter);
}

}  // namespace nfagg
