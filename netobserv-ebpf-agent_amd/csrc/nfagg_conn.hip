// nfagg_conn.hip — the kernels of nfagg_conn_fold (nfagg_conn.h): k_conn_claim hashes every flow, finds its connection's slot and
// folds what does not depend on the direction; k_conn_finish adds the flow to its side; k_conn_count / k_conn_emit compact the
// occupied slots into the caller's partials. One lane per flow, grid-stride; integer work only; no LDS beside the scan's
// sixteen words, no scratch.
//
// k_conn_claim: a lane reads the five 16-byte units of its record that hold the id (@0..39), the two times (@40, @48), bytes
// (@56), packets (@64), the ethertype (@68) and the flags (@70): 80 of the record's 144 bytes. A flow the filter turns away
// gets hash id 0 and no slot. The others format each address with ip_text twice, into a counting sink for gob's two length
// bytes and into the FNV state, hash the three field groups and the total, and claim a slot by the total. There the lane
// folds, with atomic max / or on words that start at zero, its position into first, last and (TCP with FIN) first-FIN, its
// TCP flags, and the two times. It leaves the slot's index and its hashA in the per-flow scratch, 12 bytes.
//
// k_conn_finish, after the kernel boundary: first_idx is final, so "same or other" is hashA of the flow against hashA of the
// flow at first_idx, read from the scratch (one scattered 8-byte load; recomputing would format that record's address again).
// The lane adds 1, bytes and packets to its side, skipping adds of zero; the flow at first_idx stores first_hash_a.
//
// Claim protocol (that of nfagg_metrics.hip, copied so that those kernels stay as they are; nobody waits, no key is ever
// partly published as another key's): a key is two words. For k = 0, 1: load word k of the slot; if it is empty,
// compare-and-swap it from empty to the lane's word k; go on to word k + 1 if the old value was empty or equal to the lane's
// word, else move to the next slot. The invariant:
//   - a set word never changes, and slots are never freed within a call;
//   - whoever sets word 0 goes on to word 1 of the same slot at once, and there either sets it or finds it set by another
//     lane (which it then compares with its own). Either way word 1 is set once that lane has passed, so no slot is partly
//     set when the kernel ends: a set first word means two set words;
//   - so a slot whose first word is set and whose second is still empty may be taken by ANY key with that first word: it
//     belongs to whichever such key arrives first, and a later key with the same first word and another second walks on.
//     Nothing is folded into a slot before both words matched, so a slot's values are those of exactly one key.
// A key's probe sequence is fixed by its hash and the words it passes never change back, so a key always ends in the same
// slot: one slot per key, one key per slot. Both words carry bit 63, so no word is ever the empty value.
//
// Overflow: a first word claimed from empty is one more occupied slot, counted in ConnCtl::claimed. Probes go in rounds of
// eight. Behind every round the lanes of the wave that end it together (those that have just found their slot, and those that
// walk on) add their wins with one atomic whose result nobody waits for, and the walkers look at the count and the flag, one
// 8-byte load, as every lane does before its first probe: a count over the cap, or ConnCtl::overflow (set by a probe that has
// walked the whole table), and the lane gives up (its hash id is written first). Why there and nowhere else, measured on 2.86 M
// flows that are 2.86 M connections: a returning add per claim, or any add between the two compare-and-swaps of a claim, costs
// the kernel 1.9 ms of 4.8; one add after the whole wave has left the probe loop costs nothing, but a wave leaves only with its
// last walker, so a table that is too small fills up to the last slot before any count is seen and every probe walks all of it
// (one launch of 506 ms). Behind a round the add is off the claim's dependent chain and at most eight probes late. The table has
// at least twice the cap's slots, so it does not fill up behind the count. k_conn_finish does nothing after an overflow, and
// k_conn_emit writes no partial. The look only ends the work early: the verdict is k_conn_emit's, from the scan's exact count
// of occupied slots against the cap.
#include "nfagg_conn.h"
#include "nfagg_flp_line.h"

namespace nfagg {

constexpr int kConnBlock = 256;
constexpr uint32_t kConnMaxBlocks = 2048;
constexpr uint64_t kConnFlowsPerBlock = 1024;
static_assert(kConnMinSlots == kScanBlock, "a table is whole blocks of k_conn_count");

// toBytes(SrcAddr) / toBytes(DstAddr): the text's length from a counting pass, then the text into the FNV state.
NF_DEV void gob_addr(FnvSink& f, const Ip4w& a) {
    CountSink c;
    ip_text(c, a);
    gob_string_head(f, c.n);
    ip_text(f, a);
}

NF_DEV bool conn_over(const ConnDev& D) {                       // claimed and overflow lie side by side: one load
    const uint64_t w = ald(reinterpret_cast<const uint64_t*>(D.ctl));
    return (uint32_t)w > D.cap || (w >> 32) != 0;
}

// The slot of the key (k0, k1), or kConnNoSlot when the call has overflowed. Probes go in rounds of eight; behind every round the
// lanes of the wave that are still here or have just found their slot count their wins together and look at the count.
constexpr uint32_t kConnRound = 8;
NF_DEV uint32_t conn_claim(const ConnDev& D, uint64_t total, uint64_t k0, uint64_t k1) {
    if (conn_over(D)) return kConnNoSlot;
    const uint32_t mask = D.mask;
    uint32_t s = (uint32_t)fmix64(total) & mask, found = kConnNoSlot;
    for (uint64_t t0 = 0; t0 <= mask; t0 += kConnRound) {
        bool won = false;
        for (uint32_t t = 0; t < kConnRound && t0 + t <= mask; t++) {
            uint64_t* p = D.slots + (size_t)s * kConnSlotWords;
            uint64_t a = ald(p);
            if (a == 0) {
                a = acas(p, (uint64_t)0, k0);
                won = won || a == 0;
            }
            if (a == 0 || a == k0) {
                uint64_t b = ald(p + 1);
                if (b == 0) b = acas(p + 1, (uint64_t)0, k1);
                if (b == 0 || b == k1) { found = s; break; }
            }
            s = (s + 1) & mask;
        }
        // every set first word is counted exactly once, by the lowest winner among the lanes that end this round together
        const unsigned long long born = __ballot(won);
        if (won && (threadIdx.x & 63) == __ffsll(born) - 1) aadd(&D.ctl->claimed, (uint32_t)__popcll(born));
        if (found != kConnNoSlot) return found;
        if (conn_over(D)) return kConnNoSlot;
    }
    ast(&D.ctl->overflow, 1u);                                                           // the table is full
    return kConnNoSlot;
}

__global__ __launch_bounds__(kConnBlock) void k_conn_claim(const void* __restrict__ recs, uint64_t n, ConnDev D) {
    const uint64_t stride = (uint64_t)gridDim.x * kConnBlock;
    for (uint64_t i = (uint64_t)blockIdx.x * kConnBlock + threadIdx.x; i < n; i += stride) {
        const uint4* p = reinterpret_cast<const uint4*>(reinterpret_cast<const uint8_t*>(recs) + i * kRecordBytes);
        const uint4 u0 = p[0], u1 = p[1], u2 = p[2], u3 = p[3], u4 = p[4];
        const uint32_t eth = u4.y & 0xffffu, flags = u4.y >> 16, proto = u2.y & 0xffu;
        const bool tracked = conn_tracked(eth, proto);
        const unsigned long long gone = __ballot(!tracked);                              // one add per wave, not per discarded flow
        if (!tracked) {
            if ((threadIdx.x & 63) == __ffsll(gone) - 1) aadd(&D.ctl->discarded, (uint32_t)__popcll(gone));
            if (D.hash_ids) D.hash_ids[i] = 0;
            D.slot_of[i] = kConnNoSlot;
            continue;
        }
        FnvSink fa, fb, fc;
        gob_addr(fa, Ip4w{{u0.x, u0.y, u0.z, u0.w}}); gob_uint(fa, u2.x & 0xffffu);      // src = [SrcAddr, SrcPort]
        gob_addr(fb, Ip4w{{u1.x, u1.y, u1.z, u1.w}}); gob_uint(fb, u2.x >> 16);          // dst = [DstAddr, DstPort]
        gob_uint(fc, proto);                                                             // common = [Proto]
        const uint64_t total = conn_total(fc.h, fa.h, fb.h);
        if (D.hash_ids) D.hash_ids[i] = total;
        D.hash_a[i] = fa.h;
        const uint32_t s = conn_claim(D, total, kConnMark | (total >> 32), kConnMark | (total & 0xffffffffull));
        D.slot_of[i] = s;
        if (s == kConnNoSlot) continue;
        uint64_t* q = D.slots + (size_t)s * kConnSlotWords;
        uint32_t* w = reinterpret_cast<uint32_t*>(q + 2);
        const uint32_t at = (uint32_t)i;                                                 // n <= 2^32 - 2: ~at is never zero
        amax(w, ~at);
        amax(w + 1, at);
        if (proto == 6u) {                                                               // only TCP has the Flags key
            if (flags & 1u) amax(w + 2, ~at);
            if (flags) aor(w + 3, flags);
        }
        const TimeParts ts = flow_time(D.now_sec, D.now_nsec, D.mono_now, (uint64_t)u2.z | ((uint64_t)u2.w << 32));
        const TimeParts te = flow_time(D.now_sec, D.now_nsec, D.mono_now, (uint64_t)u3.x | ((uint64_t)u3.y << 32));
        const uint64_t start_ms = (uint64_t)ts.sec * 1000ull + (uint64_t)(ts.nsec / 1000000), end_ms = (uint64_t)te.sec * 1000ull + (uint64_t)(te.nsec / 1000000);
        amax(q + 10, ~(start_ms ^ kConnBias));
        amax(q + 11, end_ms ^ kConnBias);
    }
}

__global__ __launch_bounds__(kConnBlock) void k_conn_finish(const void* __restrict__ recs, uint64_t n, ConnDev D) {
    if (D.ctl->overflow || D.ctl->claimed > D.cap) return;                               // nothing will be emitted
    const uint64_t stride = (uint64_t)gridDim.x * kConnBlock;
    for (uint64_t i = (uint64_t)blockIdx.x * kConnBlock + threadIdx.x; i < n; i += stride) {
        const uint32_t s = D.slot_of[i];
        if (s == kConnNoSlot) continue;
        uint64_t* q = D.slots + (size_t)s * kConnSlotWords;
        const uint32_t first = ~reinterpret_cast<const uint32_t*>(q + 2)[0];
        const uint64_t ha = D.hash_a[i];
        const uint64_t hf = first == (uint32_t)i ? ha : D.hash_a[first];
        const uint4* p = reinterpret_cast<const uint4*>(reinterpret_cast<const uint8_t*>(recs) + i * kRecordBytes);
        const uint4 u3 = p[3];
        const uint64_t bytes = (uint64_t)u3.z | ((uint64_t)u3.w << 32), packets = p[4].x;
        const uint32_t side = ha == hf ? 0u : 1u;
        aadd(q + 4 + side, (uint64_t)1);
        if (bytes) aadd(q + 6 + side, bytes);
        if (packets) aadd(q + 8 + side, packets);
        if (first == (uint32_t)i) q[12] = ha;
    }
}

// One lane per slot: 1 for an occupied slot, scanned inside the block.
__global__ __launch_bounds__(kScanBlock) void k_conn_count(ConnDev D, uint32_t* __restrict__ local_off, uint32_t* __restrict__ block_sum) {
    __shared__ uint32_t wave_tot[kScanBlock / 64];
    const uint64_t i = (uint64_t)blockIdx.x * kScanBlock + threadIdx.x;
    const uint32_t occupied = D.slots[(size_t)i * kConnSlotWords] != 0 ? 1u : 0u;
    block_scan(occupied, i, (uint64_t)gridDim.x * kScanBlock, wave_tot, local_off, block_sum);
}

// block_base: the scan of the block sums, the total last. Every lane works out the verdict; block 0 reports it; the partials
// are written only when the call has not overflowed.
__global__ __launch_bounds__(kScanBlock) void k_conn_emit(ConnDev D, const uint32_t* __restrict__ local_off, const uint64_t* __restrict__ block_base) {
    const uint32_t count = (uint32_t)block_base[gridDim.x];
    const bool over = D.ctl->overflow != 0 || count > D.cap;
    if (blockIdx.x == 0 && threadIdx.x == 0) { D.ctl->count = count; D.ctl->over = over ? 1u : 0u; }
    if (over) return;
    const uint64_t i = (uint64_t)blockIdx.x * kScanBlock + threadIdx.x;
    const uint4* q = reinterpret_cast<const uint4*>(D.slots + (size_t)i * kConnSlotWords);
    const uint4 k = q[0];
    if ((k.x | k.y) == 0) return;
    const uint64_t at = block_base[blockIdx.x] + local_off[i];                            // < count <= cap
    uint4* o = reinterpret_cast<uint4*>(D.out + at);
    const uint4 idx = q[1], t = q[5], fa = q[6];
    o[0] = make_uint4(k.z, k.x, fa.x, fa.y);                                             // hash_total (low, high), first_hash_a
    o[1] = make_uint4(~idx.x, idx.y, ~idx.z, idx.w);                                     // first_idx, last_idx, first_fin_idx, flags_or
    o[2] = q[2]; o[3] = q[3]; o[4] = q[4];                                               // flows, bytes, packets
    o[5] = make_uint4(~t.x, ~t.y ^ 0x80000000u, t.z, t.w ^ 0x80000000u);                 // start_ms_min, end_ms_max
    o[6] = make_uint4(0u, 0u, 0u, 0u);
    o[7] = make_uint4(0u, 0u, 0u, 0u);
}

static unsigned conn_blocks(uint64_t n) {
    const uint64_t want = (n + kConnFlowsPerBlock - 1) / kConnFlowsPerBlock;
    return (unsigned)(want < kConnMaxBlocks ? want : kConnMaxBlocks);
}

hipError_t launch_conn_claim(const void* d_recs, uint64_t n, const ConnDev& D, hipStream_t s) {
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_conn_claim, dim3(conn_blocks(n)), dim3(kConnBlock), 0, s, d_recs, n, D);
    return hipGetLastError();
}

hipError_t launch_conn_finish(const void* d_recs, uint64_t n, const ConnDev& D, uint32_t* d_local_off, uint32_t* d_block_sum, uint64_t* d_block_base, hipStream_t s) {
    const uint32_t blocks = (D.mask + 1) / kConnMinSlots;
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_conn_finish, dim3(conn_blocks(n)), dim3(kConnBlock), 0, s, d_recs, n, D);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_conn_count, dim3(blocks), dim3(kScanBlock), 0, s, D, d_local_off, d_block_sum);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = launch_scan_block_sums(d_block_sum, blocks, d_block_base, s)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_conn_emit, dim3(blocks), dim3(kScanBlock), 0, s, D, d_local_off, d_block_base);
    return hipGetLastError();
}

}  // namespace nfagg
