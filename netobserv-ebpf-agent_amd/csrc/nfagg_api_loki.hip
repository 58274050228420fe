// nfagg_api_loki.hip — the host side of write loki on the device (include/nfagg.h, "write loki on the device"; nfagg_loki.h):
// the table (the Kubernetes blocks without the keys the stage takes out of a line, the label classes, the canonical subnet
// labels), nfagg_loki_plan[_device], nfagg_loki_write[_device]. A plan costs one memset, the launches of nfagg_loki.hip and one
// 32-byte read-back; a write one upload of the label text, one 8-byte read-back for the size, and the launches.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>
#include <algorithm>
#include <map>
#include <string>
#include <vector>

#include "../../include/nfagg.h"
#include "nfagg_internal.h"
#include "nfagg_handle.h"
#include "nfagg_api_call.h"
#include "nfagg_api_tables.h"
#include "nfagg_loki.h"

using namespace nfagg;

struct nfagg_loki_table {
    nfagg_handle* h = nullptr;
    const nfagg_k8s_table* k8s = nullptr;              // not owned: the caller keeps both alive
    const nfagg_net_table* net = nullptr;
    nfagg_loki_spec spec{};
    uint32_t omit = 0;                                  // label or ignored
    std::vector<K8sRow> rows;
    std::vector<uint8_t> blob;
    std::vector<uint32_t> cls[2];                       // per row; empty: no label field of that side
    std::vector<uint32_t> first_row[2];                 // [class - 1]
    std::vector<uint16_t> canon;
    DevBuf d_rows, d_blob, d_cls[2], d_canon;
};

namespace nfagg {

// The plan a handle keeps: the arrays the write reads again, and what the call was made with. Its staging is its own, the
// namer table and the host entry points' arrays included: the plan outlives the call that made it and nfagg_loki_write reads it
// again, so the handle's EncodeScratch, which the next encoder call reuses, cannot hold it.
struct LokiPlan {
    DevBuf ctl, keys, first, sid, slot_of, rows8, ts, lens, deferred;               // the key kernel's
    DevBuf flag, rank, streams, pinc, cuts, key, key_sorted, val, perm, gidx, esz, E, gs, groups, tmp;
    DevBuf scan_local, scan_sum, scan_base;                                           // the 64-bit prefix sums' two levels
    DevBuf hsz, H, labels, lab_off, bpos, local_off, block_base, names, esc, k8s_rows, net_rows;      // the write's, and a call's own staging
    DevBuf in_records, in_ids, out, boffs, bents, out_streams, out_groups, out_deferred;               // the host entry points'
    size_t tmp_bytes = 0;
    bool valid = false, content = false;
    DevBuf in_ne_rows;
    FlpLineArgs A{};
    LokiDev L{};
    LokiPlanDev D{};
    LokiCtl counts{};
    std::vector<nfagg_intf_name> h_names;
    std::vector<uint8_t> h_esc;
};

}  // namespace nfagg

namespace {

void loki_plan_delete(LokiPlan* p) { delete p; }

LokiPlan* plan_of(nfagg_handle* h) {
    if (!h->loki) h->loki = std::unique_ptr<LokiPlan, void (*)(LokiPlan*)>(new LokiPlan, loki_plan_delete);
    return h->loki.get();
}

// utf8.Valid: no overlong form, no surrogate, nothing above U+10FFFF
bool utf8_valid(const std::string& s) {
    const size_t n = s.size();
    for (size_t k = 0; k < n;) {
        const uint8_t b = (uint8_t)s[k];
        if (b < 0x80) { k++; continue; }
        uint32_t need, lo = 0x80, hi = 0xBF;
        if (b >= 0xC2 && b <= 0xDF) need = 1;
        else if (b >= 0xE0 && b <= 0xEF) { need = 2; if (b == 0xE0) lo = 0xA0; if (b == 0xED) hi = 0x9F; }
        else if (b >= 0xF0 && b <= 0xF4) { need = 3; if (b == 0xF0) lo = 0x90; if (b == 0xF4) hi = 0x8F; }
        else return false;
        if (k + need >= n) return false;
        for (uint32_t c = 1; c <= need; c++) {
            const uint8_t x = (uint8_t)s[k + c];
            if (x < (c == 1 ? lo : 0x80u) || x > (c == 1 ? hi : 0xBFu)) return false;
        }
        k += need + 1;
    }
    return true;
}

// A JSON string as flp_escape wrote it, from the opening quote at p[0]: its bytes back (*text) and where it ends (the index
// behind the closing quote). flp_escape passes every byte from 0x80 up as it is, so the text is the caller's.
size_t unescape(const uint8_t* p, size_t n, std::string* text) {
    text->clear();
    size_t k = 1;
    while (k < n && p[k] != '"') {
        if (p[k] != '\\') { text->push_back((char)p[k++]); continue; }
        const uint8_t e = k + 1 < n ? p[k + 1] : 0;
        if (e == 'u' && k + 5 < n) {
            auto hexv = [](uint8_t c) { return c <= '9' ? c - '0' : (c | 0x20) - 'a' + 10; };
            text->push_back((char)(hexv(p[k + 4]) * 16 + hexv(p[k + 5])));
            k += 6;
        } else { text->push_back(e == 'n' ? '\n' : e == 'r' ? '\r' : e == 't' ? '\t' : (char)e); k += 2; }
    }
    return k + 1;
}

// nfagg_k8s_entry's field order (the bits of NFAGG_DIM_SRC_K8S) by the key's name behind SrcK8S_ / DstK8S_
int k8s_field_of(const std::string& name) {
    static const char* const kNames[9] = {"Namespace", "Name", "Type", "OwnerName", "OwnerType", "NetworkName", "HostIP", "HostName", "Zone"};
    for (int f = 0; f < 9; f++) if (name == kNames[f]) return f;
    return -1;
}

int check_spec(nfagg_handle* h, const nfagg_loki_spec* s) {
    if (s->struct_size != sizeof(nfagg_loki_spec)) return fail(h, NFAGG_EINVAL, "nfagg_loki_spec.struct_size mismatch");
    if (s->label_keys & ~NFAGG_LOKI_KEY_ALL) return fail(h, NFAGG_EINVAL, "label_keys: unknown key bits 0x%x", s->label_keys & ~NFAGG_LOKI_KEY_ALL);
    if (s->ignore_keys & ~NFAGG_LOKI_KEY_ALL) return fail(h, NFAGG_EINVAL, "ignore_keys: unknown key bits 0x%x", s->ignore_keys & ~NFAGG_LOKI_KEY_ALL);
    if (s->label_keys & ~s->ignore_keys & NFAGG_LOKI_KEY_HASH_ID) return fail(h, NFAGG_EINVAL, "_HashId as a label is not served: a stream per conversation");
    if (s->timestamp_source > NFAGG_LOKI_TS_TIME_FLOW_START_MS) return fail(h, NFAGG_EINVAL, "unknown timestamp source %u", s->timestamp_source);
    if (!(s->timestamp_scale > 0) || !isfinite(s->timestamp_scale)) return fail(h, NFAGG_EINVAL, "timestamp_scale must be finite and positive");
    if (s->batch_size < 1 || s->batch_size > 0x7fffffffu) return fail(h, NFAGG_EINVAL, "batch_size %u, not 1 .. 2^31 - 1", s->batch_size);
    return NFAGG_OK;
}

int up(nfagg_handle* h, DevBuf& d, const void* src, size_t bytes) {
    HIP_TRY(h, d.alloc(std::max<size_t>(bytes, 16)));
    if (bytes) HIP_TRY(h, hipMemcpy(d.p, src, bytes, hipMemcpyHostToDevice));
    return NFAGG_OK;
}

}  // namespace

extern "C" {

int nfagg_loki_table_create(nfagg_handle* h, const nfagg_k8s_table* k8s, const nfagg_net_table* net, const nfagg_loki_spec* spec,
                            nfagg_loki_table** table) {
    if (!table || !k8s || !net || !spec) return fail(h, NFAGG_EINVAL, "null argument");
    *table = nullptr;
    int rc = check_spec(h, spec);
    if (rc != NFAGG_OK) return rc;
    if (k8s->h != h || net->h != h) return fail(h, NFAGG_EINVAL, "the Kubernetes and the net table were not created for this handle");
    nfagg_loki_table* t = new (std::nothrow) nfagg_loki_table;
    if (!t) return fail(h, NFAGG_ENOMEM, "out of memory");
    t->h = h; t->k8s = k8s; t->net = net; t->spec = *spec;
    const uint32_t labels = spec->label_keys & ~spec->ignore_keys;           // the ignore list is looked at first
    t->spec.label_keys = labels;
    t->omit = labels | spec->ignore_keys;
    const size_t n = k8s->rows.size();
    t->rows.resize(n);
    std::vector<uint8_t> bad(n * 9, 0);                                      // a label field whose text is not valid UTF-8
    std::string name, text;
    for (size_t r = 0; r < n; r++) {
        K8sRow row = k8s->rows[r];
        for (int side = 0; side < 2; side++) {
            const uint8_t* p = k8s->blob.data() + (size_t)(side ? row.dst_off : row.src_off) * 16;
            const size_t len = side ? row.dst_len : row.src_len;
            const uint32_t omit = (t->omit >> (9 * side)) & 0x1ffu, lab = (labels >> (9 * side)) & 0x1ffu;
            const uint32_t off = (uint32_t)(t->blob.size() / 16);
            size_t k = 0, kept = 0;
            while (k < len) {                                                // ,"SrcK8S_<Name>":"<escaped>"
                const size_t start = k;
                size_t q = k + 9;
                name.clear();
                while (q < len && p[q] != '"') name.push_back((char)p[q++]);
                q += 2;                                                      // the quote and the colon
                k = q < len ? q + unescape(p + q, len - q, &text) : len;
                const int f = k8s_field_of(name);
                const bool is_label = f >= 0 && (lab >> f) & 1u;
                if (is_label && !utf8_valid(text)) { bad[r * 9 + f] = 1; continue; }     // gone from labels and from the line
                if (f >= 0 && (omit >> f) & 1u) continue;
                t->blob.insert(t->blob.end(), p + start, p + k);
                kept += k - start;
            }
            t->blob.resize((t->blob.size() + 15) / 16 * 16, 0);
            if (kept == 0) t->blob.resize(t->blob.size() + 16, 0);           // a block's offset is always inside the blob
            if (side == 0) { row.src_off = off; row.src_len = (uint16_t)kept; } else { row.dst_off = off; row.dst_len = (uint16_t)kept; }
        }
        t->rows[r] = row;
    }
    for (int side = 0; side < 2; side++) {
        const uint32_t lab = (labels >> (9 * side)) & 0x1ffu;
        if (!lab) continue;
        std::map<std::vector<uint32_t>, uint32_t> seen;
        std::vector<uint32_t> key;
        t->cls[side].resize(n);
        for (size_t r = 0; r < n; r++) {
            key.clear();
            bool any = false;
            for (int f = 0; f < 9; f++)
                if (lab & (1u << f)) { const uint32_t id = bad[r * 9 + f] ? 0u : k8s->field_ids[r * 9 + f]; key.push_back(id); any = any || id; }
            if (!any) { t->cls[side][r] = 0; continue; }                     // no label of this side: the class of a flow without a row
            const auto it = seen.emplace(key, (uint32_t)seen.size() + 1);
            if (it.second) t->first_row[side].push_back((uint32_t)r);
            t->cls[side][r] = it.first->second;
        }
    }
    std::map<std::string, uint16_t> texts;
    for (size_t l = 0; l < net->frags.size(); l++) {
        const NetFrag& f = net->frags[l];
        uint16_t c = 0xffffu;
        if (f.src_len) {                                                     // ,"SrcSubnetLabel":"<escaped>"
            unescape(net->blob.data() + (size_t)f.src_off * 16 + 18, f.src_len - 18, &text);
            if (utf8_valid(text)) c = texts.emplace(text, (uint16_t)l).first->second;
        }
        t->canon.push_back(c);
    }
    if (h) {
        auto upload = [&]() -> int {
            HIP_TRY(h, hipSetDevice(h->device));
            int rc2;
            if ((rc2 = up(h, t->d_rows, t->rows.data(), n * sizeof(K8sRow))) != NFAGG_OK) return rc2;
            if ((rc2 = up(h, t->d_blob, t->blob.data(), t->blob.size())) != NFAGG_OK) return rc2;
            for (int side = 0; side < 2; side++)
                if (!t->cls[side].empty() && (rc2 = up(h, t->d_cls[side], t->cls[side].data(), n * sizeof(uint32_t))) != NFAGG_OK) return rc2;
            return up(h, t->d_canon, t->canon.data(), t->canon.size() * sizeof(uint16_t));
        };
        rc = upload();
        if (rc != NFAGG_OK) { nfagg_loki_table_destroy(t); return rc; }
    }
    *table = t;
    return NFAGG_OK;
}

void nfagg_loki_table_destroy(nfagg_loki_table* t) { destroy_on_handle(t); }

uint32_t nfagg_loki_n_classes(const nfagg_loki_table* t, int side) {
    return t && (side == 0 || side == 1) ? (uint32_t)t->first_row[side].size() : 0u;
}

int nfagg_loki_class_row(const nfagg_loki_table* t, int side, uint32_t cls, uint32_t* row) {
    if (!t || !row) return fail(nullptr, NFAGG_EINVAL, "null argument");
    if (side != 0 && side != 1) return fail(nullptr, NFAGG_EINVAL, "unknown side %d", side);
    if (cls < 1 || cls > t->first_row[side].size()) return fail(nullptr, NFAGG_EINVAL, "class %u of %zu", cls, t->first_row[side].size());
    *row = t->first_row[side][cls - 1];
    return NFAGG_OK;
}

int nfagg_loki_render(const nfagg_loki_table* t, int side, uint32_t row, void* out, size_t cap, size_t* n_out) {
    if (!t || !n_out) return fail(nullptr, NFAGG_EINVAL, "null argument");
    if (side != 0 && side != 1) return fail(nullptr, NFAGG_EINVAL, "unknown side %d", side);
    if (row >= t->rows.size()) return fail(nullptr, NFAGG_EINVAL, "row %u of %zu", row, t->rows.size());
    const K8sRow& r = t->rows[row];
    const size_t off = (size_t)(side ? r.dst_off : r.src_off) * 16, len = side ? r.dst_len : r.src_len;
    *n_out = len;
    if (len && (!out || cap < len)) return NFAGG_TRUNCATED;
    if (len) memcpy(out, t->blob.data() + off, len);
    return NFAGG_OK;
}

uint32_t nfagg_loki_max_entry(int policy) { return loki_max_entry(policy); }

int nfagg_loki_plan_device(nfagg_handle* h, const void* d_records, size_t n, const nfagg_pb_features* d_features, const uint16_t* d_rows,
                           const nfagg_netev_table* netev_table, const nfagg_tls_names* tls_names, const nfagg_k8s_table* k8s,
                           const nfagg_net_table* net, const uint64_t* d_hash_ids, const nfagg_flp_options* opt, const nfagg_loki_table* table,
                           int64_t now_unix_ns, nfagg_loki_stream* d_streams, uint32_t stream_cap, nfagg_loki_group* d_groups, uint32_t group_cap,
                           uint8_t* d_deferred, nfagg_loki_counts* counts) {
    int rc = check_flp_options(h, opt);
    if (rc != NFAGG_OK) return rc;
    if (!h || !tls_names || !k8s || !net || !table || !counts || (n && !d_records) || (stream_cap && !d_streams) || (group_cap && !d_groups))
        return fail(h, NFAGG_EINVAL, "null argument");
    const NetevArgs ne{d_rows, netev_table};
    if ((rc = netev_together(h, ne, n)) != NFAGG_OK) return rc;
    if (d_rows && !d_features) return fail(h, NFAGG_EINVAL, "network-events rows without the flows' feature parts");
    PbFeat F{};
    if (netev_table && (rc = device_netev(h, &ne, n, &F)) != NFAGG_OK) return rc;
    if (d_features && (rc = device_features(h, d_features, &F)) != NFAGG_OK) return rc;
    const bool content = d_features != nullptr;
    const FlpLineTables t{FlpLevel::Conn, tls_names, k8s, net, d_hash_ids};       // d_hash_ids nullptr: no conntrack stage
    if ((rc = check_flp_tables(h, t)) != NFAGG_OK) return rc;
    if (table->h != h || !table->d_rows) return fail(h, NFAGG_EINVAL, "the Loki table was not created for this handle");
    if (table->k8s != k8s || table->net != net) return fail(h, NFAGG_EINVAL, "the Loki table was built over other tables than the call's");
    if (stream_cap > kLokiMaxStreams) return fail(h, NFAGG_ERANGE, "a cap of %u streams, more than %u", stream_cap, kLokiMaxStreams);
    if (n > (1ull << 30)) return fail(h, NFAGG_ERANGE, "%zu flows in one call, more than 2^30", n);
    if (((uintptr_t)d_records & 15u) != 0 || (((uintptr_t)d_hash_ids | (uintptr_t)d_streams | (uintptr_t)d_groups) & 7u) != 0)
        return fail(h, NFAGG_EINVAL, "device records must be 16-byte, hash ids, streams and groups 8-byte aligned");
    *counts = nfagg_loki_counts{};
    LokiPlan& S = *plan_of(h);
    S.valid = false;
    S.counts = LokiCtl{};
    if (!n) { S.valid = true; S.A = FlpLineArgs{}; S.content = false; return NFAGG_OK; }
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t slots = (size_t)std::max<uint64_t>(next_pow2(2ull * std::min<uint64_t>(n, kLokiMaxStreams)), kLokiMinSlots);
    const size_t n_streams_max = std::min<size_t>(n, kLokiMaxStreams);
    S.tmp_bytes = loki_tmp_bytes(n);
    API_TRY(ensure_all(h, {
        {S.ctl, 256}, {S.keys, slots * 16}, {S.first, slots * 4}, {S.sid, slots * 4}, {S.slot_of, n * 4}, {S.rows8, n * 32}, {S.ts, n * 16},
        {S.lens, n * 4}, {S.deferred, n + 16}, {S.flag, (n + 1) * 4}, {S.rank, (n + 1) * 4}, {S.streams, n_streams_max * sizeof(nfagg_loki_stream)},
        {S.pinc, (n + 1) * 8}, {S.cuts, n * 4}, {S.key, n * 8}, {S.key_sorted, (n + 1) * 8}, {S.val, n * 4}, {S.perm, n * 4}, {S.gidx, (n + 1) * 4},
        {S.esz, (n + 1) * 4}, {S.E, (n + 1) * 8}, {S.gs, n * 4}, {S.groups, n * sizeof(nfagg_loki_group)}, {S.tmp, S.tmp_bytes},
        {S.scan_local, (n + 1) * 4}, {S.scan_sum, ((n + 1) / 1024 + 2) * 4}, {S.scan_base, ((n + 1) / 1024 + 3) * 8}}));
    const LokiScan X{S.scan_local.as<uint32_t>(), S.scan_sum.as<uint32_t>(), S.scan_base.as<uint64_t>()};      // behind ensure: a growth moves the blocks
    FlpLineArgs& A = S.A;                                   // into the plan's own staging: the write reads both again
    if ((rc = stage_flp_line(h, d_records, n, opt, F, t, FlpLineStage{S.names, S.esc, S.k8s_rows, S.net_rows, S.h_names, S.h_esc}, &A)) != NFAGG_OK) return rc;
    S.content = content;
    LokiDev& L = S.L;
    L = LokiDev{};
    L.rows = table->d_rows.as<const K8sRow>(); L.blob = table->d_blob.as<const uint8_t>();
    for (int side = 0; side < 2; side++) L.cls[side] = table->cls[side].empty() ? nullptr : table->d_cls[side].as<const uint32_t>();
    L.canon = table->d_canon.as<const uint16_t>();
    L.label_keys = table->spec.label_keys; L.omit_keys = table->omit;
    L.ts_source = table->spec.timestamp_source; L.ts_scale = table->spec.timestamp_scale;
    split_now(now_unix_ns, L.now_sec, L.now_nsec);
    LokiPlanDev& D = S.D;
    D = LokiPlanDev{S.ctl.as<LokiCtl>(), S.keys.as<uint64_t>(), S.first.as<uint32_t>(), S.sid.as<uint32_t>(), (uint32_t)slots - 1, S.slot_of.as<uint32_t>(),
                    S.rows8.as<uint32_t>(), S.ts.as<int64_t>(), S.lens.as<uint32_t>(), S.deferred.as<uint8_t>()};
    HIP_TRY(h, hipMemsetAsync(S.ctl.p, 0, 256, h->stream));
    HIP_TRY(h, hipMemsetAsync(S.keys.p, 0, slots * 16, h->stream));
    HIP_TRY(h, hipMemsetAsync(S.first.p, 0xff, slots * 4, h->stream));
    hipError_t e;
    if ((e = launch_loki_key(A, content, L, D, h->stream)) != hipSuccess) return fail(h, NFAGG_EDEVICE, "Loki key launch failed: %s", hipGetErrorString(e));
    if ((e = launch_loki_rank(n, D, S.flag.as<uint32_t>(), S.rank.as<uint32_t>(), S.streams.as<nfagg_loki_stream>(), S.tmp.p, S.tmp_bytes, h->stream)) != hipSuccess)
        return fail(h, NFAGG_EDEVICE, "Loki stream rank failed: %s", hipGetErrorString(e));
    if ((e = launch_loki_cuts(n, D, S.pinc.as<uint64_t>(), table->spec.batch_size, S.cuts.as<uint32_t>(), X, h->stream)) != hipSuccess)
        return fail(h, NFAGG_EDEVICE, "Loki cut walk failed: %s", hipGetErrorString(e));
    if ((e = launch_loki_sort(n, D, S.cuts.as<const uint32_t>(), S.key.as<uint64_t>(), S.key_sorted.as<uint64_t>(), S.val.as<uint32_t>(), S.perm.as<uint32_t>(), S.tmp.p,
                              S.tmp_bytes, h->stream)) != hipSuccess)
        return fail(h, NFAGG_EDEVICE, "Loki sort failed: %s", hipGetErrorString(e));
    if ((e = launch_loki_groups(n, D, S.key_sorted.as<const uint64_t>(), S.perm.as<const uint32_t>(), S.flag.as<uint32_t>(), S.gidx.as<uint32_t>(),
                                S.esz.as<uint32_t>(), S.E.as<uint64_t>(), S.gs.as<uint32_t>(), S.groups.as<nfagg_loki_group>(), S.tmp.p, S.tmp_bytes, X, h->stream)) != hipSuccess)
        return fail(h, NFAGG_EDEVICE, "Loki grouping failed: %s", hipGetErrorString(e));
    HIP_TRY(h, hipMemcpyAsync(&S.counts, S.ctl.p, sizeof S.counts, hipMemcpyDeviceToHost, h->stream));      // the one read-back
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    const LokiCtl& c = S.counts;
    if (c.over) return fail(h, NFAGG_ERANGE, "more than %u streams in one call", kLokiMaxStreams);
    *counts = nfagg_loki_counts{c.n_streams, c.n_groups, c.n_batches, c.n_deferred};
    if (d_deferred) HIP_TRY(h, hipMemcpyAsync(d_deferred, S.deferred.p, n, hipMemcpyDeviceToDevice, h->stream));
    if (c.n_streams > stream_cap || c.n_groups > group_cap) { HIP_TRY(h, hipStreamSynchronize(h->stream)); return NFAGG_TRUNCATED; }
    if (c.n_streams) HIP_TRY(h, hipMemcpyAsync(d_streams, S.streams.p, c.n_streams * sizeof(nfagg_loki_stream), hipMemcpyDeviceToDevice, h->stream));
    if (c.n_groups) HIP_TRY(h, hipMemcpyAsync(d_groups, S.groups.p, c.n_groups * sizeof(nfagg_loki_group), hipMemcpyDeviceToDevice, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    S.valid = true;
    return NFAGG_OK;
}

int nfagg_loki_plan(nfagg_handle* h, const void* records, size_t n, const nfagg_pb_features* features, const uint16_t* rows,
                    const nfagg_netev_table* netev_table, const nfagg_tls_names* tls_names, const nfagg_k8s_table* k8s, const nfagg_net_table* net,
                    const uint64_t* hash_ids, const nfagg_flp_options* opt, const nfagg_loki_table* table, int64_t now_unix_ns,
                    nfagg_loki_stream* streams, uint32_t stream_cap, nfagg_loki_group* groups, uint32_t group_cap, uint8_t* deferred,
                    nfagg_loki_counts* counts) {
    if (!h || !counts || (n && !records) || (stream_cap && !streams) || (group_cap && !groups)) return fail(h, NFAGG_EINVAL, "null argument");
    if (stream_cap > kLokiMaxStreams) return fail(h, NFAGG_ERANGE, "a cap of %u streams, more than %u", stream_cap, kLokiMaxStreams);
    if (n > (1ull << 30)) return fail(h, NFAGG_ERANGE, "%zu flows in one call, more than 2^30", n);
    LokiPlan& S = *plan_of(h);
    HIP_TRY(h, hipSetDevice(h->device));
    API_TRY(ensure_all(h, {{S.out_streams, (size_t)stream_cap * sizeof(nfagg_loki_stream) + kStageSlack},
                           {S.out_groups, (size_t)group_cap * sizeof(nfagg_loki_group) + kStageSlack}, {S.out_deferred, n + kStageSlack}}));
    API_TRY(stage_in(h, S.in_records, records, n * kRecordBytes));
    API_TRY(stage_in(h, S.in_ids, hash_ids, hash_ids ? n * 8 : 0));
    if (features && features->struct_size != sizeof(nfagg_pb_features)) return fail(h, NFAGG_EINVAL, "nfagg_pb_features.struct_size mismatch");
    nfagg_pb_features dfeat{};
    if (features && n) API_TRY(stage_pb_features(h, features, n, &dfeat));      // the handle's encoder staging: no other encoder call before the write
    const uint16_t* d_rows = nullptr;
    if (rows && n) {
        API_TRY(stage_in(h, S.in_ne_rows, rows, n * 8));
        d_rows = S.in_ne_rows.as<const uint16_t>();
    }
    int rc = nfagg_loki_plan_device(h, S.in_records.p, n, (features && n) ? &dfeat : nullptr, rows && !n ? rows : d_rows, netev_table, tls_names, k8s, net,
                                hash_ids ? S.in_ids.as<const uint64_t>() : nullptr, opt,
                                table, now_unix_ns, stream_cap ? S.out_streams.as<nfagg_loki_stream>() : nullptr, stream_cap,
                                group_cap ? S.out_groups.as<nfagg_loki_group>() : nullptr, group_cap, deferred ? S.out_deferred.as<uint8_t>() : nullptr, counts);
    if (rc != NFAGG_OK && rc != NFAGG_TRUNCATED) return rc;
    API_TRY(fetch(h, deferred, S.out_deferred, deferred ? n : 0));
    if (rc == NFAGG_OK) {
        API_TRY(fetch(h, streams, S.out_streams, counts->n_streams * sizeof(nfagg_loki_stream)));
        API_TRY(fetch(h, groups, S.out_groups, counts->n_groups * sizeof(nfagg_loki_group)));
    }
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return rc;
}

int nfagg_loki_write_device(nfagg_handle* h, const void* labels, const uint64_t* label_offsets, void* d_out, size_t out_cap, uint64_t* d_batch_offsets,
                            uint32_t* d_batch_entries, size_t* out_bytes) {
    if (!h || !out_bytes || !d_batch_offsets) return fail(h, NFAGG_EINVAL, "null argument");
    *out_bytes = 0;
    if (!h->loki || !h->loki->valid) return fail(h, NFAGG_EINVAL, "no plan: nfagg_loki_plan has not run on this handle, or its outputs were truncated");
    LokiPlan& S = *h->loki;
    const LokiCtl& c = S.counts;
    if (((uintptr_t)d_out & 15u) != 0 || ((uintptr_t)d_batch_offsets & 7u) != 0 || ((uintptr_t)d_batch_entries & 3u) != 0)
        return fail(h, NFAGG_EINVAL, "the output must be 16-byte, the batch offsets 8-byte aligned");
    if (c.n_streams && (!labels || !label_offsets)) return fail(h, NFAGG_EINVAL, "null label text");
    if (c.n_batches && !d_batch_entries) return fail(h, NFAGG_EINVAL, "null argument");
    HIP_TRY(h, hipSetDevice(h->device));
    if (!c.n_part) { HIP_TRY(h, hipMemsetAsync(d_batch_offsets, 0, sizeof(uint64_t), h->stream)); HIP_TRY(h, hipStreamSynchronize(h->stream)); return NFAGG_OK; }
    std::vector<uint32_t> off(c.n_streams + 1);
    for (uint32_t s = 0; s <= c.n_streams; s++) {
        const uint64_t o = label_offsets[s] - label_offsets[0];
        if (s && (label_offsets[s] < label_offsets[s - 1] + 2 || label_offsets[s] - label_offsets[s - 1] > kLokiLabelsMax))
            return fail(h, NFAGG_EINVAL, "stream %u: a label text of %lld bytes, not 2 .. %u", s - 1, (long long)(label_offsets[s] - label_offsets[s - 1]), kLokiLabelsMax);
        off[s] = (uint32_t)o;
    }
    if (label_offsets[c.n_streams] - label_offsets[0] >= (1ull << 32)) return fail(h, NFAGG_ERANGE, "the streams' label texts come to 2^32 bytes or more");
    const uint32_t m = c.n_part, ng = c.n_groups, nb = c.n_batches;
    const size_t blocks = (m + 1023) / 1024;
    API_TRY(ensure_all(h, {{S.hsz, (ng + 1) * 4ull}, {S.H, (ng + 1) * 8ull}, {S.labels, off[c.n_streams] + 16ull}, {S.lab_off, (c.n_streams + 1) * 4ull},
                           {S.bpos, (nb + 1) * 4ull}, {S.local_off, m * 4ull}, {S.block_base, (blocks + 1) * 8}}));
    HIP_TRY(h, hipMemcpyAsync(S.labels.p, (const uint8_t*)labels + label_offsets[0], off[c.n_streams], hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemcpyAsync(S.lab_off.p, off.data(), off.size() * 4, hipMemcpyHostToDevice, h->stream));
    LokiWriteDev W{S.ctl.as<const LokiCtl>(), S.perm.as<const uint32_t>(), S.flag.as<const uint32_t>(), S.gidx.as<const uint32_t>(), S.E.as<const uint64_t>(),
                   S.gs.as<const uint32_t>(), S.groups.as<const nfagg_loki_group>(), S.labels.as<const uint8_t>(), S.lab_off.as<const uint32_t>(),
                   S.hsz.as<uint32_t>(), S.H.as<uint64_t>(), S.local_off.as<uint32_t>(), S.block_base.as<uint64_t>(), S.bpos.as<uint32_t>()};
    const LokiScan X{S.scan_local.as<uint32_t>(), S.scan_sum.as<uint32_t>(), S.scan_base.as<uint64_t>()};     // sized by the plan: n_groups + 1 <= n + 1
    // the two passes are written out: the scans are the plan's own (encode_two_pass hands out the handle's), the size pass has
    // no block sums of its own, and its messages are not "<what> <verb> launch failed"
    hipError_t e = launch_loki_offsets(m, ng, nb, W, d_batch_offsets, d_batch_entries, X, h->stream);
    if (e != hipSuccess) return fail(h, NFAGG_EDEVICE, "Loki offsets failed: %s", hipGetErrorString(e));
    uint64_t total = 0;
    HIP_TRY(h, hipMemcpyAsync(&total, S.block_base.as<uint64_t>() + blocks, sizeof total, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));                  // off and the caller's label text have been consumed
    *out_bytes = (size_t)total;
    if (total > out_cap || !d_out) return NFAGG_TRUNCATED;
    e = launch_loki_write(S.A, S.content, S.L, S.D, W, m, ng, (uint8_t*)d_out, h->stream);
    if (e != hipSuccess) return fail(h, NFAGG_EDEVICE, "Loki write launch failed: %s", hipGetErrorString(e));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return NFAGG_OK;
}

int nfagg_loki_write(nfagg_handle* h, const void* labels, const uint64_t* label_offsets, void* out, size_t out_cap, uint64_t* batch_offsets,
                     uint32_t* batch_entries, size_t* out_bytes) {
    if (!h || !out_bytes || !batch_offsets) return fail(h, NFAGG_EINVAL, "null argument");
    *out_bytes = 0;
    if (!h->loki || !h->loki->valid) return fail(h, NFAGG_EINVAL, "no plan: nfagg_loki_plan has not run on this handle, or its outputs were truncated");
    LokiPlan& S = *h->loki;
    const uint32_t nb = S.counts.n_batches;
    if (nb && !batch_entries) return fail(h, NFAGG_EINVAL, "null argument");
    HIP_TRY(h, hipSetDevice(h->device));
    API_TRY(ensure_all(h, {{S.out, out_cap + kStageSlack}, {S.boffs, (nb + 1) * 8ull}, {S.bents, (nb + 1) * 4ull}}));
    const int rc = nfagg_loki_write_device(h, labels, label_offsets, out ? S.out.p : nullptr, out_cap, S.boffs.as<uint64_t>(), S.bents.as<uint32_t>(), out_bytes);
    if (rc != NFAGG_OK && rc != NFAGG_TRUNCATED) return rc;
    API_TRY(fetch(h, batch_offsets, S.boffs, (nb + 1) * 8ull));
    API_TRY(fetch(h, batch_entries, S.bents, nb * 4ull));
    if (rc == NFAGG_OK) API_TRY(fetch(h, out, S.out, *out_bytes));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return rc;
}

}  // extern "C"
