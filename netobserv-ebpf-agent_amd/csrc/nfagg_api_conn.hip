// nfagg_api_conn.hip — the host side of the conversation fold (include/nfagg.h, "Conversation tracking"; nfagg_conn.h):
// nfagg_conn_fold, nfagg_conn_fold_device and the host's own nfagg_conn_hash. The scratch is the handle's grow-only buffers;
// a call costs one memset (control words and table), five launches and one 128-byte read-back.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>

#include "../../include/nfagg.h"
#include "nfagg_internal.h"
#include "nfagg_handle.h"
#include "nfagg_api_call.h"
#include "nfagg_conn.h"

using namespace nfagg;

namespace {

// net.IP.String() of a 16-byte address into out (at most 39 bytes), as ip_text (nfagg_flp_line.h) prints it on the device:
// the dotted quad for ten zero bytes and ff ff, else netip's appendTo6 (the first longest run of two or more zero groups
// becomes "::", lower-case hex without leading zeros). Returns the length.
uint32_t host_ip_text(const uint8_t ip[16], char out[40]) {
    static const uint8_t v4pre[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0xff, 0xff};
    if (memcmp(ip, v4pre, 12) == 0) return (uint32_t)snprintf(out, 40, "%u.%u.%u.%u", ip[12], ip[13], ip[14], ip[15]);
    uint32_t g[8];
    for (int k = 0; k < 8; k++) g[k] = ((uint32_t)ip[2 * k] << 8) | ip[2 * k + 1];
    int z0 = -1, zlen = 1;
    for (int k = 0; k < 8; k++) {
        int j = k;
        while (j < 8 && g[j] == 0) j++;
        if (j - k > zlen) { z0 = k; zlen = j - k; }
    }
    uint32_t n = 0;
    for (int k = 0; k < 8; k++) {
        if (k == z0) { out[n++] = ':'; out[n++] = ':'; k += zlen - 1; continue; }
        if (k > 0 && k != z0 + zlen) out[n++] = ':';
        n += (uint32_t)snprintf(out + n, 40 - n, "%x", g[k]);
    }
    return n;
}

void host_gob_addr(FnvSink& f, const uint8_t ip[16]) {
    char text[40];
    const uint32_t len = host_ip_text(ip, text);
    gob_string_head(f, len);
    for (uint32_t k = 0; k < len; k++) f.put((uint8_t)text[k]);
}

}  // namespace

extern "C" {

uint64_t nfagg_conn_hash(const void* record, uint64_t* hash_a, uint64_t* hash_b) {
    if (hash_a) *hash_a = 0;
    if (hash_b) *hash_b = 0;
    if (!record) return 0;
    const uint8_t* r = (const uint8_t*)record;
    const uint32_t sport = r[32] | ((uint32_t)r[33] << 8), dport = r[34] | ((uint32_t)r[35] << 8), proto = r[36];
    const uint32_t eth = r[68] | ((uint32_t)r[69] << 8);
    if (!conn_tracked(eth, proto)) return 0;
    FnvSink fa, fb, fc;
    host_gob_addr(fa, r); gob_uint(fa, sport);
    host_gob_addr(fb, r + 16); gob_uint(fb, dport);
    gob_uint(fc, proto);
    if (hash_a) *hash_a = fa.h;
    if (hash_b) *hash_b = fb.h;
    return conn_total(fc.h, fa.h, fb.h);
}

int nfagg_conn_fold_device(nfagg_handle* h, const void* d_records, size_t n, const nfagg_conn_options* opt, uint64_t* d_hash_ids, uint32_t cap,
                           nfagg_conn_partial* d_out, uint32_t* n_conns, uint32_t* n_discarded) {
    if (!h || !opt || !n_conns || !n_discarded || (n && !d_records)) return fail(h, NFAGG_EINVAL, "null argument");
    if (opt->struct_size != sizeof(nfagg_conn_options)) return fail(h, NFAGG_EINVAL, "nfagg_conn_options.struct_size mismatch");
    if (cap > kConnMaxConns) return fail(h, NFAGG_ERANGE, "a cap of %u connections, more than %u", cap, kConnMaxConns);
    if (n > 0xFFFFFFFEull) return fail(h, NFAGG_ERANGE, "%zu records in one call, more than 2^32 - 2", n);
    if (cap && !d_out) return fail(h, NFAGG_EINVAL, "a cap without an output array");
    if (((uintptr_t)d_records & 15u) != 0 || ((uintptr_t)d_out & 15u) != 0 || ((uintptr_t)d_hash_ids & 7u) != 0)
        return fail(h, NFAGG_EINVAL, "device records and partials must be 16-byte, hash ids 8-byte aligned");
    *n_conns = 0; *n_discarded = 0;
    if (!n) return NFAGG_OK;
    ConnDev D{};
    D.cap = cap;
    // there are no more connections than flows: a large cap over a small call does not zero and scan a large table
    D.mask = (uint32_t)std::max<uint64_t>(next_pow2(2ull * std::min<uint64_t>(cap, n)), kConnMinSlots) - 1;
    D.hash_ids = d_hash_ids; D.out = d_out;
    split_now(opt->now_unix_ns, D.now_sec, D.now_nsec);
    D.mono_now = opt->mono_now_ns;
    const size_t slots = (size_t)D.mask + 1, blocks = slots / kConnMinSlots;
    const size_t slot_bytes = slots * kConnSlotWords * sizeof(uint64_t);
    auto& S = h->enc;
    HIP_TRY(h, hipSetDevice(h->device));
    API_TRY(ensure_all(h, {{S.conn_slots, 256 + slot_bytes}, {S.conn_flow, n * (sizeof(uint64_t) + sizeof(uint32_t)) + 16}, {S.local_off, slots * sizeof(uint32_t)},
                           {S.block_sum, blocks * sizeof(uint32_t)}, {S.block_base, (blocks + 1) * sizeof(uint64_t)}}));
    D.ctl = S.conn_slots.as<ConnCtl>();
    D.slots = (uint64_t*)(S.conn_slots.as<uint8_t>() + 256);
    D.hash_a = S.conn_flow.as<uint64_t>();                        // n hashes, then n slot indexes
    D.slot_of = (uint32_t*)(D.hash_a + n);
    HIP_TRY(h, hipMemsetAsync(S.conn_slots.p, 0, 256 + slot_bytes, h->stream));
    hipError_t e = launch_conn_claim(d_records, n, D, h->stream);
    if (e != hipSuccess) return fail(h, NFAGG_EDEVICE, "conn claim launch failed: %s", hipGetErrorString(e));
    e = launch_conn_finish(d_records, n, D, S.local_off.as<uint32_t>(), S.block_sum.as<uint32_t>(), S.block_base.as<uint64_t>(), h->stream);
    if (e != hipSuccess) return fail(h, NFAGG_EDEVICE, "conn finish launch failed: %s", hipGetErrorString(e));
    ConnCtl ctl;
    HIP_TRY(h, hipMemcpyAsync(&ctl, D.ctl, sizeof ctl, hipMemcpyDeviceToHost, h->stream));      // the one read-back: counts and flags
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    *n_discarded = ctl.discarded;
    // an overflowed call stopped claiming behind its cap: its count is a lower bound, and above the cap
    *n_conns = ctl.over ? std::max(ctl.count, cap + 1) : ctl.count;
    return ctl.over ? NFAGG_TRUNCATED : NFAGG_OK;
}

int nfagg_conn_fold(nfagg_handle* h, const void* records, size_t n, const nfagg_conn_options* opt, uint64_t* hash_ids, uint32_t cap,
                    nfagg_conn_partial* out, uint32_t* n_conns, uint32_t* n_discarded) {
    if (!h || !opt || !n_conns || !n_discarded || (n && !records)) return fail(h, NFAGG_EINVAL, "null argument");
    if (cap > kConnMaxConns) return fail(h, NFAGG_ERANGE, "a cap of %u connections, more than %u", cap, kConnMaxConns);
    if (n > 0xFFFFFFFEull) return fail(h, NFAGG_ERANGE, "%zu records in one call, more than 2^32 - 2", n);
    if (cap && !out) return fail(h, NFAGG_EINVAL, "a cap without an output array");
    auto& S = h->enc;
    HIP_TRY(h, hipSetDevice(h->device));
    API_TRY(ensure_all(h, {{S.conn_ids, n * sizeof(uint64_t) + kStageSlack}, {S.conn_out, std::min<size_t>(cap, n) * sizeof(nfagg_conn_partial) + kStageSlack}}));
    API_TRY(stage_in(h, S.in_records, records, n * kRecordBytes));
    const int rc = nfagg_conn_fold_device(h, S.in_records.p, n, opt, hash_ids ? S.conn_ids.as<uint64_t>() : nullptr, cap, S.conn_out.as<nfagg_conn_partial>(), n_conns,
                                n_discarded);
    if (rc != NFAGG_OK && rc != NFAGG_TRUNCATED) return rc;
    API_TRY(fetch(h, hash_ids, S.conn_ids, hash_ids ? n * sizeof(uint64_t) : 0));
    if (rc == NFAGG_OK) API_TRY(fetch(h, out, S.conn_out, (size_t)*n_conns * sizeof(nfagg_conn_partial)));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return rc;
}

}  // extern "C"
