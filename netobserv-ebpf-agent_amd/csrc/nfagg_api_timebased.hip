// nfagg_api_timebased.hip — the host side of `extract timebased` (include/nfagg.h, "extract timebased"; nfagg_timebased.h): the
// rule set and its tables, nfagg_timebased_extract[_device], nfagg_timebased_results[_device], the key read-back. The tables, the
// slices and the evaluation scratch belong to the object; the staged inputs of the host-memory twins are the handle's
// (nfagg_api_call.h). A call with flows costs two read-backs before the evaluation (the missing count, which may refuse the call
// before anything has changed; then the key counts and the touched counts, which size the slices) and one synchronisation behind it.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <deque>
#include <string>
#include <vector>

#include "../../include/nfagg.h"
#include "nfagg_internal.h"
#include "nfagg_handle.h"
#include "nfagg_api_call.h"
#include "nfagg_api_tables.h"
#include "nfagg_timebased.h"

using namespace nfagg;

namespace {

struct TbSlice {
    int64_t stamp = 0;
    uint32_t m = 0;                      // entries
    DevBuf buf;
};

struct TbTable {
    std::string name;                    // the index keys joined by ','
    uint32_t n_cols = 0, col[kTbMaxCols] = {};
    uint32_t n_src = 0, src[kTbMaxSrc] = {};
    uint32_t n_units = 0, n_words = 0, slots = 0, n_keys = 0;
    int64_t max_interval = 0;
    // the Kubernetes columns' classes: grouping met_g[c] of `met` (a one-bit mask each), and per class whether the text is there
    nfagg_metrics_table* met = nullptr;
    int met_g[kTbMaxCols] = {-1, -1, -1, -1};
    std::vector<uint8_t> cls_ok[kTbMaxCols];
    size_t cls_ok_off[kTbMaxCols] = {};
    uint64_t label_ok[kNetMaxCidrs / 64] = {};
    DevBuf d_slots, d_call, d_lastval, d_touched, d_slot_of_id, d_cls_ok;
    std::deque<TbSlice> slices;          // oldest first
};

struct TbRule { uint32_t table, op, src, src_slot, top_k, reversed; int64_t interval; };

const char* const kK8sSuffix[9] = {"Namespace", "Name", "Type", "OwnerName", "OwnerType", "NetworkName", "HostIP", "HostName", "Zone"};

// The column a key name selects, 0 for a name that is not served.
uint32_t column_of(const char* name) {
    static const struct { const char* name; uint32_t kind; } plain[] = {
        {"SrcAddr", kTbColSrcAddr}, {"DstAddr", kTbColDstAddr}, {"SrcPort", kTbColSrcPort}, {"DstPort", kTbColDstPort}, {"Proto", kTbColProto},
        {"SrcSubnetLabel", kTbColSrcLabel}, {"DstSubnetLabel", kTbColDstLabel}, {"FlowDirection", kTbColDirection}};
    for (const auto& p : plain) if (strcmp(name, p.name) == 0) return p.kind;
    for (uint32_t side = 0; side < 2; side++) {
        const char* prefix = side ? "DstK8S_" : "SrcK8S_";
        if (strncmp(name, prefix, 7) != 0) continue;
        for (uint32_t f = 0; f < 9; f++) if (strcmp(name + 7, kK8sSuffix[f]) == 0) return kTbColK8s + 16 * side + f;
    }
    return 0;
}

}  // namespace

struct nfagg_timebased {
    nfagg_handle* h = nullptr;
    const nfagg_k8s_table* k8s = nullptr;          // not owned
    const nfagg_net_table* net = nullptr;
    uint32_t max_keys = 0, n_tables = 0, n_rules = 0;
    TbTable tables[kTbMaxTables];
    TbRule rules[kTbMaxRules] = {};
    bool failed = false, has_clock = false;
    int64_t last_now = 0;
    DevBuf d_ctl;
    DevBuf enter, slot_of;                         // per call: u8[n], u32[n]
    DevBuf acc, value, ord, flags, sel, pairs;     // per rule evaluation
    DevBuf out_stage, key_ids, key_out;            // the host-memory twins' results; the key read-back
    ~nfagg_timebased() { for (auto& t : tables) nfagg_metrics_table_destroy(t.met); }
};

namespace {

TbTableDev table_dev(const nfagg_timebased* tb, uint32_t t) {
    const TbTable& T = tb->tables[t];
    TbTableDev D{};
    D.slots = T.d_slots.as<uint64_t>(); D.call = T.d_call.as<uint64_t>(); D.lastval = T.d_lastval.as<uint64_t>();
    D.touched = T.d_touched.as<uint32_t>(); D.slot_of_id = T.d_slot_of_id.as<uint32_t>();
    for (uint32_t c = 0; c < T.n_cols; c++) {
        D.col[c] = T.col[c];
        if (T.met_g[c] >= 0) {
            const uint32_t side = (T.col[c] - kTbColK8s) >> 4;
            D.cls[c] = T.met->d_cls.as<const uint32_t>() + T.met->d_off[T.met_g[c]][side];
            D.cls_ok[c] = T.d_cls_ok.as<const uint8_t>() + T.cls_ok_off[c];
        }
    }
    for (uint32_t j = 0; j < T.n_src; j++) D.src[j] = T.src[j];
    memcpy(D.label_ok, T.label_ok, sizeof D.label_ok);
    D.n_cols = T.n_cols; D.n_src = T.n_src; D.n_words = T.n_words; D.mask = T.slots - 1; D.max_keys = tb->max_keys;
    D.call_words = kTbCallHead + kTbSrcWords * T.n_src;
    D.n_rows = tb->k8s ? (uint32_t)tb->k8s->rows.size() : 0u;
    D.index = t;
    return D;
}

size_t held_bytes(const nfagg_timebased* tb) {
    size_t b = tb->d_ctl.cap + tb->enter.cap + tb->slot_of.cap + tb->acc.cap + tb->value.cap + tb->ord.cap + tb->flags.cap + tb->sel.cap + tb->pairs.cap +
               tb->out_stage.cap + tb->key_ids.cap + tb->key_out.cap;
    for (uint32_t t = 0; t < tb->n_tables; t++) {
        const TbTable& T = tb->tables[t];
        b += T.d_slots.cap + T.d_call.cap + T.d_lastval.cap + T.d_touched.cap + T.d_slot_of_id.cap + T.d_cls_ok.cap;
        for (const TbSlice& s : T.slices) b += s.buf.cap;
    }
    return b;
}

// Everything a table holds on the device back to "no key yet".
int clear_device(nfagg_timebased* tb) {
    nfagg_handle* h = tb->h;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    HIP_TRY(h, hipMemsetAsync(tb->d_ctl.p, 0, sizeof(TbCtl), h->stream));
    for (uint32_t t = 0; t < tb->n_tables; t++) {
        TbTable& T = tb->tables[t];
        T.slices.clear();
        T.n_keys = 0;
        HIP_TRY(h, hipMemsetAsync(T.d_slots.p, 0, (size_t)T.slots * kTbSlotWords * 8, h->stream));
        HIP_TRY(h, hipMemsetAsync(T.d_call.p, 0, (size_t)tb->max_keys * (kTbCallHead + kTbSrcWords * T.n_src) * 8, h->stream));
        HIP_TRY(h, hipMemsetAsync(T.d_lastval.p, 0, (size_t)tb->max_keys * T.n_src * 8, h->stream));
        HIP_TRY(h, hipMemsetAsync(T.d_slot_of_id.p, 0, (size_t)tb->max_keys * 4, h->stream));
    }
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    tb->failed = false; tb->has_clock = false; tb->last_now = 0;
    return NFAGG_OK;
}

// The classes of a table's Kubernetes columns and which of them carry a text; a text with ',' is refused.
int build_classes(nfagg_handle* h, nfagg_timebased* tb, TbTable& T, uint32_t rule) {
    uint32_t dims[kTbMaxCols], g = 0;
    for (uint32_t c = 0; c < T.n_cols; c++)
        if (tb_col_is_k8s(T.col[c])) {
            const uint32_t side = (T.col[c] - kTbColK8s) >> 4, f = (T.col[c] - kTbColK8s) & 15u;
            dims[g] = 1u << (9 * side + f);
            T.met_g[c] = (int)g++;
        }
    if (!g) return NFAGG_OK;
    API_TRY(nfagg_metrics_table_create(h, tb->k8s, dims, g, &T.met));
    std::vector<const std::string*> text(tb->k8s->field_text.size(), nullptr);
    for (const auto& kv : tb->k8s->field_text) text[kv.second] = &kv.first;
    size_t off = 0;
    for (uint32_t c = 0; c < T.n_cols; c++) {
        if (T.met_g[c] < 0) continue;
        const uint32_t side = (T.col[c] - kTbColK8s) >> 4, f = (T.col[c] - kTbColK8s) & 15u;
        const std::vector<uint32_t>& first = T.met->first_row[T.met_g[c]][side];
        T.cls_ok[c].assign(first.size() + 1, 0);
        for (size_t k = 0; k < first.size(); k++) {
            const uint32_t fid = tb->k8s->field_ids[(size_t)first[k] * 9 + f];
            if (!fid) continue;                                          // the row has no such field
            const std::string& s = *text[fid - 1];
            if (s.empty()) continue;                                     // ConvertToString gives "": the flow stays out
            if (s.find(',') != std::string::npos)
                return fail(h, NFAGG_EINVAL, "rule %u: index key \"%s%s\": the text \"%s\" contains ','", rule, side ? "DstK8S_" : "SrcK8S_", kK8sSuffix[f], s.c_str());
            T.cls_ok[c][k + 1] = 1;
        }
        T.cls_ok_off[c] = off;
        off += (T.cls_ok[c].size() + 15) / 16 * 16;
    }
    if (h) {
        HIP_TRY(h, hipSetDevice(h->device));
        HIP_TRY(h, T.d_cls_ok.alloc(std::max<size_t>(off, 16)));
        for (uint32_t c = 0; c < T.n_cols; c++)
            if (T.met_g[c] >= 0)
                HIP_TRY(h, hipMemcpy(T.d_cls_ok.as<uint8_t>() + T.cls_ok_off[c], T.cls_ok[c].data(), T.cls_ok[c].size(), hipMemcpyHostToDevice));
    }
    return NFAGG_OK;
}

// Which labels carry a text; a text with ',' is refused. A label's fragment is ,"SrcSubnetLabel":"<escaped text>".
int build_labels(nfagg_handle* h, nfagg_timebased* tb, TbTable& T, uint32_t rule) {
    bool any = false;
    for (uint32_t c = 0; c < T.n_cols; c++) any = any || T.col[c] == kTbColSrcLabel || T.col[c] == kTbColDstLabel;
    if (!any) return NFAGG_OK;
    const size_t head = sizeof(",\"SrcSubnetLabel\":\"") - 1;
    for (size_t k = 0; k < tb->net->frags.size() && k < kNetMaxCidrs; k++) {
        const NetFrag& fr = tb->net->frags[k];
        if (!fr.src_len) continue;
        const uint8_t* p = tb->net->blob.data() + (size_t)fr.src_off * 16;
        if (fr.src_len > head + 1 && memchr(p + head, ',', fr.src_len - head - 1))
            return fail(h, NFAGG_EINVAL, "rule %u: index key \"SrcSubnetLabel\" / \"DstSubnetLabel\": the text of label %zu contains ','", rule, k);
        T.label_ok[k >> 6] |= 1ull << (k & 63);
    }
    return NFAGG_OK;
}

int create_core(nfagg_handle* h, nfagg_timebased* tb, const nfagg_tb_rule* rules, uint32_t n_rules) {
    for (uint32_t r = 0; r < n_rules; r++) {
        const nfagg_tb_rule& ru = rules[r];
        if (ru.struct_size != sizeof(nfagg_tb_rule)) return fail(h, NFAGG_EINVAL, "rule %u: struct_size %u, not %zu", r, ru.struct_size, sizeof(nfagg_tb_rule));
        if (ru.n_index_keys < 1 || ru.n_index_keys > kTbMaxCols) return fail(h, NFAGG_EINVAL, "rule %u: %u index keys, not 1..%u", r, ru.n_index_keys, kTbMaxCols);
        uint32_t col[kTbMaxCols] = {}, units = 0;
        std::string name;
        for (uint32_t c = 0; c < ru.n_index_keys; c++) {
            if (!ru.index_keys[c]) return fail(h, NFAGG_EINVAL, "rule %u: index key %u is null", r, c);
            col[c] = column_of(ru.index_keys[c]);
            if (!col[c]) return fail(h, NFAGG_EINVAL, "rule %u: index key \"%s\" is not served", r, ru.index_keys[c]);
            if (tb_col_is_k8s(col[c]) && !tb->k8s) return fail(h, NFAGG_EINVAL, "rule %u: index key \"%s\" needs the Kubernetes table", r, ru.index_keys[c]);
            if ((col[c] == kTbColSrcLabel || col[c] == kTbColDstLabel) && !tb->net) return fail(h, NFAGG_EINVAL, "rule %u: index key \"%s\" needs the net table", r, ru.index_keys[c]);
            units += tb_col_is_addr(col[c]) ? 4u : 1u;
            name += (c ? "," : "") + std::string(ru.index_keys[c]);
        }
        if (units > kTbMaxUnits) return fail(h, NFAGG_EINVAL, "rule %u: the index keys take %u bytes, more than %u", r, 4 * units, 4 * kTbMaxUnits);
        if (ru.operation < NFAGG_TB_OP_SUM || ru.operation > NFAGG_TB_OP_DIFF) return fail(h, NFAGG_EINVAL, "rule %u: unknown operation %u", r, ru.operation);
        if (ru.value < 1 || ru.value > NFAGG_MET_VALUE_LAST) return fail(h, NFAGG_EINVAL, "rule %u: unknown value source %u", r, ru.value);
        if (ru.top_k > NFAGG_TB_MAX_TOPK) return fail(h, NFAGG_EINVAL, "rule %u: top_k %u, more than %u", r, ru.top_k, NFAGG_TB_MAX_TOPK);
        if (ru.interval_ns < 0) return fail(h, NFAGG_EINVAL, "rule %u: a negative interval", r);
        uint32_t t = 0;
        while (t < tb->n_tables && tb->tables[t].name != name) t++;
        if (t == tb->n_tables) {
            if (t == kTbMaxTables) return fail(h, NFAGG_EINVAL, "rule %u: more than %u distinct index-key lists", r, kTbMaxTables);
            TbTable& T = tb->tables[tb->n_tables++];
            T.name = name;
            T.n_cols = ru.n_index_keys;
            for (uint32_t c = 0; c < T.n_cols; c++) T.col[c] = col[c];
            T.n_units = units;
            T.n_words = (32 * units + 62) / 63;
            API_TRY(build_classes(h, tb, T, r));
            API_TRY(build_labels(h, tb, T, r));
        }
        TbTable& T = tb->tables[t];
        T.max_interval = std::max(T.max_interval, ru.interval_ns);
        uint32_t j = 0;
        while (j < T.n_src && T.src[j] != ru.value) j++;
        if (j == T.n_src) {
            if (j == kTbMaxSrc) return fail(h, NFAGG_EINVAL, "rule %u: table \"%s\" has more than %u value sources", r, name.c_str(), kTbMaxSrc);
            T.src[T.n_src++] = ru.value;
        }
        tb->rules[r] = TbRule{t, ru.operation, ru.value, j, ru.top_k, ru.reversed ? 1u : 0u, ru.interval_ns};
    }
    tb->n_rules = n_rules;
    if (!h) return NFAGG_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, tb->d_ctl.alloc(256));
    HIP_TRY(h, tb->sel.alloc(sizeof(TbSelect)));
    HIP_TRY(h, tb->pairs.alloc(2 * (size_t)NFAGG_TB_MAX_TOPK * 8));
    for (uint32_t t = 0; t < tb->n_tables; t++) {
        TbTable& T = tb->tables[t];
        T.slots = (uint32_t)std::max<uint64_t>(next_pow2(2ull * tb->max_keys), kTbMinSlots);
        HIP_TRY(h, T.d_slots.alloc((size_t)T.slots * kTbSlotWords * 8));
        HIP_TRY(h, T.d_call.alloc((size_t)tb->max_keys * (kTbCallHead + kTbSrcWords * T.n_src) * 8));
        HIP_TRY(h, T.d_lastval.alloc((size_t)tb->max_keys * T.n_src * 8));
        HIP_TRY(h, T.d_touched.alloc((size_t)tb->max_keys * 4));
        HIP_TRY(h, T.d_slot_of_id.alloc((size_t)tb->max_keys * 4));
    }
    return clear_device(tb);
}

bool reads_k8s(const nfagg_timebased* tb) {
    for (uint32_t t = 0; t < tb->n_tables; t++)
        for (uint32_t c = 0; c < tb->tables[t].n_cols; c++) if (tb_col_is_k8s(tb->tables[t].col[c])) return true;
    return false;
}
bool reads_net(const nfagg_timebased* tb) {
    for (uint32_t t = 0; t < tb->n_tables; t++)
        for (uint32_t c = 0; c < tb->tables[t].n_cols; c++) {
            const uint32_t k = tb->tables[t].col[c];
            if (k == kTbColSrcLabel || k == kTbColDstLabel || k == kTbColDirection) return true;
        }
    return false;
}

int check_object(nfagg_handle* h, const nfagg_timebased* tb) {
    if (tb->h != h || !tb->d_ctl) return fail(h, NFAGG_EINVAL, "the timebased rules were not created for this handle");
    if (tb->failed) return fail(h, NFAGG_EINVAL, "a table has met more keys than max_keys (%u): nfagg_timebased_reset it", tb->max_keys);
    return NFAGG_OK;
}

// n_out of every rule; NFAGG_TRUNCATED when a cap is below it.
int result_counts(nfagg_handle* h, const nfagg_timebased* tb, const uint32_t* cap, void* const* out, uint32_t* n_out) {
    bool small = false;
    for (uint32_t r = 0; r < tb->n_rules; r++) {
        const uint32_t nk = tb->tables[tb->rules[r].table].n_keys;
        n_out[r] = tb->rules[r].top_k ? std::min(tb->rules[r].top_k, nk) : nk;
        if (cap[r] && !out[r]) return fail(h, NFAGG_EINVAL, "rule %u: a cap without an output array", r);
        if (((uintptr_t)out[r] & 15u) != 0) return fail(h, NFAGG_EINVAL, "rule %u: the results must be 16-byte aligned", r);
        small = small || cap[r] < n_out[r];
    }
    return small ? NFAGG_TRUNCATED : NFAGG_OK;
}

// Every rule at tb->last_now into d_out (DEVICE memory). The caller has checked the caps.
int evaluate(nfagg_handle* h, nfagg_timebased* tb, nfagg_tb_result* const* d_out, const uint32_t* n_out) {
    // the four arrays of a rule's evaluation, sized once for the largest table: the rules share them in stream order, and a growth
    // between two rules would free what the kernels of the first still use
    size_t most = 0;
    for (uint32_t t = 0; t < tb->n_tables; t++) most = std::max<size_t>(most, tb->tables[t].n_keys);
    if (most) API_TRY(ensure_all(h, {{tb->acc, most * kTbAccWords * 8}, {tb->value, most * 8}, {tb->ord, most * 8}, {tb->flags, most}}));
    for (uint32_t r = 0; r < tb->n_rules; r++) {
        const TbRule& ru = tb->rules[r];
        TbTable& T = tb->tables[ru.table];
        const uint32_t nk = T.n_keys;
        if (!nk) continue;
        TbRuleDev R{};
        R.acc = tb->acc.as<uint64_t>(); R.value = tb->value.as<double>(); R.ord = tb->ord.as<uint64_t>(); R.flags = tb->flags.as<uint8_t>();
        R.lastval = T.d_lastval.as<const uint64_t>() + (size_t)ru.src_slot * tb->max_keys;
        R.op = ru.op; R.src_slot = ru.src_slot; R.src_signed = tb_src_signed(ru.src) ? 1u : 0u; R.reversed = ru.reversed; R.n_keys = nk; R.n_src = T.n_src;
        HIP_TRY(h, hipMemsetAsync(R.acc, 0, (size_t)nk * kTbAccWords * 8, h->stream));
        if (ru.op != NFAGG_TB_OP_LAST)
            for (const TbSlice& s : T.slices) {
                // inside the window iff not Before(now - interval): now - stamp <= interval (stamps never exceed now)
                if ((uint64_t)tb->last_now - (uint64_t)s.stamp > (uint64_t)ru.interval) continue;
                const hipError_t e = launch_tb_merge(R, s.buf.as<const uint64_t>(), s.m, h->stream);
                if (e != hipSuccess) return fail(h, NFAGG_EDEVICE, "timebased merge launch failed: %s", hipGetErrorString(e));
            }
        hipError_t e = launch_tb_value(R, h->stream);
        if (e != hipSuccess) return fail(h, NFAGG_EDEVICE, "timebased value launch failed: %s", hipGetErrorString(e));
        e = launch_tb_select(R, ru.top_k ? n_out[r] : 0u, tb->sel.as<TbSelect>(), tb->pairs.as<uint64_t>(), d_out[r], h->stream);
        if (e != hipSuccess) return fail(h, NFAGG_EDEVICE, "timebased select launch failed: %s", hipGetErrorString(e));
    }
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return NFAGG_OK;
}

void trim(nfagg_timebased* tb) {
    for (uint32_t t = 0; t < tb->n_tables; t++) {
        TbTable& T = tb->tables[t];
        while (!T.slices.empty() && (uint64_t)tb->last_now - (uint64_t)T.slices.front().stamp > (uint64_t)T.max_interval) T.slices.pop_front();
    }
}

}  // namespace

extern "C" {

int nfagg_timebased_rules_create(nfagg_handle* h, const nfagg_k8s_table* k8s_table, const nfagg_net_table* net_table, const nfagg_tb_rule* rules,
                                 uint32_t n_rules, const nfagg_tb_options* options, nfagg_timebased** tb) {
    if (!tb || !rules || !options) return fail(h, NFAGG_EINVAL, "null argument");
    *tb = nullptr;
    if (options->struct_size != sizeof(nfagg_tb_options)) return fail(h, NFAGG_EINVAL, "nfagg_tb_options.struct_size %u, not %zu", options->struct_size, sizeof(nfagg_tb_options));
    if (options->max_keys < 1 || options->max_keys > NFAGG_TB_MAX_KEYS) return fail(h, NFAGG_EINVAL, "max_keys %u, not 1..%u", options->max_keys, NFAGG_TB_MAX_KEYS);
    if (n_rules < 1 || n_rules > kTbMaxRules) return fail(h, NFAGG_EINVAL, "%u rules, not 1..%u", n_rules, kTbMaxRules);
    if (k8s_table && k8s_table->h != h) return fail(h, NFAGG_EINVAL, "the Kubernetes table was not created for this handle");
    if (net_table && net_table->h != h) return fail(h, NFAGG_EINVAL, "the net table was not created for this handle");
    nfagg_timebased* t = new (std::nothrow) nfagg_timebased;
    if (!t) return fail(h, NFAGG_ENOMEM, "out of memory");
    t->h = h; t->k8s = k8s_table; t->net = net_table; t->max_keys = options->max_keys;
    const int rc = create_core(h, t, rules, n_rules);
    if (rc != NFAGG_OK) { nfagg_timebased_destroy(t); return rc; }
    *tb = t;
    return NFAGG_OK;
}

void nfagg_timebased_destroy(nfagg_timebased* tb) { destroy_on_handle(tb); }

int nfagg_timebased_results_device(nfagg_handle* h, nfagg_timebased* tb, const uint32_t* result_cap, nfagg_tb_result* const* d_out, uint32_t* n_out) {
    if (!h || !tb || !result_cap || !d_out || !n_out) return fail(h, NFAGG_EINVAL, "null argument");
    API_TRY(check_object(h, tb));
    if (!tb->has_clock) return fail(h, NFAGG_ESTATE, "nfagg_timebased_results before the first nfagg_timebased_extract");
    API_TRY(result_counts(h, tb, result_cap, (void* const*)d_out, n_out));
    HIP_TRY(h, hipSetDevice(h->device));
    return evaluate(h, tb, d_out, n_out);
}

int nfagg_timebased_extract_device(nfagg_handle* h, nfagg_timebased* tb, const void* d_records, size_t n, const nfagg_pb_features* d_features,
                                   const uint32_t* d_k8s_rows, const nfagg_net_row* d_net_rows, int64_t now_ns, const uint32_t* result_cap,
                                   nfagg_tb_result* const* d_out, uint32_t* n_out, uint64_t* n_missing) {
    if (!h || !tb || !result_cap || !d_out || !n_out || !n_missing || (n && !d_records)) return fail(h, NFAGG_EINVAL, "null argument");
    *n_missing = 0;
    API_TRY(check_object(h, tb));
    for (uint32_t r = 0; r < tb->n_rules; r++) n_out[r] = 0;
    if (tb->has_clock && now_ns < tb->last_now) return fail(h, NFAGG_EINVAL, "now_ns %lld is below the previous call's %lld", (long long)now_ns, (long long)tb->last_now);
    if (n > 0xFFFFFFFEull) return fail(h, NFAGG_ERANGE, "%zu flows, more than 2^32 - 2", n);
    if (n && reads_k8s(tb) && !d_k8s_rows) return fail(h, NFAGG_EINVAL, "a rule names a Kubernetes key: it needs the flows' k8s rows");
    if (n && reads_net(tb) && !d_net_rows) return fail(h, NFAGG_EINVAL, "a rule names a subnet label or the direction: it needs the flows' net rows");
    if (((uintptr_t)d_records & 15u) != 0 || ((uintptr_t)d_k8s_rows & 7u) != 0 || ((uintptr_t)d_net_rows & 7u) != 0)
        return fail(h, NFAGG_EINVAL, "device records must be 16-byte, rows 8-byte aligned");
    for (uint32_t r = 0; r < tb->n_rules; r++) {
        if (result_cap[r] && !d_out[r]) return fail(h, NFAGG_EINVAL, "rule %u: a cap without an output array", r);
        if (((uintptr_t)d_out[r] & 15u) != 0) return fail(h, NFAGG_EINVAL, "rule %u: the results must be 16-byte aligned", r);
    }
    if (n)                                                   // the slices this call's trim will leave are what counts; nothing is trimmed yet
        for (uint32_t t = 0; t < tb->n_tables; t++) {
            const TbTable& T = tb->tables[t];
            size_t live = 0;
            for (const TbSlice& s : T.slices) live += (uint64_t)now_ns - (uint64_t)s.stamp <= (uint64_t)T.max_interval ? 1 : 0;
            if (live >= NFAGG_TB_MAX_SLICES)
                return fail(h, NFAGG_ERANGE, "table \"%s\" holds %u live slices inside its largest window already", T.name.c_str(), (uint32_t)NFAGG_TB_MAX_SLICES);
        }
    HIP_TRY(h, hipSetDevice(h->device));
    if (n) {
        TbFlows F{};
        F.recs = d_records; F.k8s_rows = d_k8s_rows; F.net_rows = (const uint2*)d_net_rows; F.n = n;
        if (d_features) {
            PbFeat P{};
            API_TRY(device_features(h, d_features, &P));
            F.present = P.present; F.additional = P.additional; F.dns = P.dns; F.drops = P.drops;
        }
        API_TRY(tb->enter.ensure(h, n + kStageSlack));
        API_TRY(tb->slot_of.ensure(h, n * sizeof(uint32_t)));
        TbCtl* ctl = tb->d_ctl.as<TbCtl>();
        TbCtl got;
        TbTableDev D[kTbMaxTables];
        for (uint32_t t = 0; t < tb->n_tables; t++) D[t] = table_dev(tb, t);
        // the per-call words: everything behind n_keys
        HIP_TRY(h, hipMemsetAsync(reinterpret_cast<uint8_t*>(ctl) + offsetof(TbCtl, overflow), 0, sizeof(TbCtl) - offsetof(TbCtl, overflow), h->stream));
        hipError_t e = launch_tb_presence(F, D, tb->n_tables, ctl, tb->enter.as<uint8_t>(), h->stream);
        if (e != hipSuccess) return fail(h, NFAGG_EDEVICE, "timebased presence launch failed: %s", hipGetErrorString(e));
        HIP_TRY(h, hipMemcpyAsync(&got, ctl, sizeof got, hipMemcpyDeviceToHost, h->stream));       // read-back 1: may refuse the call
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        if (got.n_missing) {
            *n_missing = got.n_missing;
            return NFAGG_EDEFER;
        }
        for (uint32_t t = 0; t < tb->n_tables; t++) {
            e = launch_tb_fold(F, D[t], ctl, tb->enter.as<const uint8_t>(), tb->slot_of.as<uint32_t>(), h->stream);
            if (e != hipSuccess) { tb->failed = true; return fail(h, NFAGG_EDEVICE, "timebased fold launch failed: %s", hipGetErrorString(e)); }
        }
        tb->failed = true;                                                                          // until the call's state is whole again
        HIP_TRY(h, hipMemcpyAsync(&got, ctl, sizeof got, hipMemcpyDeviceToHost, h->stream));       // read-back 2: keys, overflow, touched
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        for (uint32_t t = 0; t < tb->n_tables; t++)
            if (got.overflow[t] || got.n_keys[t] > tb->max_keys) {
                return fail(h, NFAGG_TRUNCATED, "table \"%s\" has met more than max_keys = %u keys", tb->tables[t].name.c_str(), tb->max_keys);   // failed stays set
            }
        for (uint32_t t = 0; t < tb->n_tables; t++) {
            TbTable& T = tb->tables[t];
            T.n_keys = got.n_keys[t];
            const uint32_t m = got.touched[t];
            if (!m) continue;
            T.slices.emplace_back();
            TbSlice& s = T.slices.back();
            s.stamp = now_ns; s.m = m;
            const size_t bytes = (size_t)m * (kTbEntryHead + kTbSrcWords * T.n_src) * 8;
            if (s.buf.alloc(bytes) != hipSuccess) { T.slices.pop_back(); return fail(h, NFAGG_ENOMEM, "hipMalloc(%zu) failed for a slice", bytes); }
            e = launch_tb_emit(D[t], m, s.buf.as<uint64_t>(), h->stream);
            if (e != hipSuccess) return fail(h, NFAGG_EDEVICE, "timebased emit launch failed: %s", hipGetErrorString(e));
        }
        tb->failed = false;
    }
    tb->has_clock = true;
    tb->last_now = now_ns;
    int rc = result_counts(h, tb, result_cap, (void* const*)d_out, n_out);
    if (rc == NFAGG_OK) rc = evaluate(h, tb, d_out, n_out);
    else HIP_TRY(h, hipStreamSynchronize(h->stream));
    trim(tb);
    return rc;
}

// The results of the host-memory twins: one staging block, rule r's part at most max_keys results long.
static int stage_results(nfagg_handle* h, nfagg_timebased* tb, const uint32_t* result_cap, nfagg_tb_result* const* out, uint32_t* caps, nfagg_tb_result** d_out) {
    size_t total = 0;
    for (uint32_t r = 0; r < tb->n_rules; r++) {
        if (result_cap[r] && !out[r]) return fail(h, NFAGG_EINVAL, "rule %u: a cap without an output array", r);
        caps[r] = std::min(result_cap[r], tb->max_keys);
        total += caps[r];
    }
    API_TRY(tb->out_stage.ensure(h, total * sizeof(nfagg_tb_result) + kStageSlack));
    size_t at = 0;
    for (uint32_t r = 0; r < tb->n_rules; r++) { d_out[r] = tb->out_stage.as<nfagg_tb_result>() + at; at += caps[r]; }
    return NFAGG_OK;
}

static int fetch_results(nfagg_handle* h, nfagg_timebased* tb, nfagg_tb_result* const* out, nfagg_tb_result* const* d_out, const uint32_t* n_out) {
    for (uint32_t r = 0; r < tb->n_rules; r++)
        if (n_out[r]) HIP_TRY(h, hipMemcpyAsync(out[r], d_out[r], (size_t)n_out[r] * sizeof(nfagg_tb_result), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return NFAGG_OK;
}

int nfagg_timebased_results(nfagg_handle* h, nfagg_timebased* tb, const uint32_t* result_cap, nfagg_tb_result* const* out, uint32_t* n_out) {
    if (!h || !tb || !result_cap || !out || !n_out) return fail(h, NFAGG_EINVAL, "null argument");
    API_TRY(check_object(h, tb));
    HIP_TRY(h, hipSetDevice(h->device));
    uint32_t caps[kTbMaxRules];
    nfagg_tb_result* d_out[kTbMaxRules];
    API_TRY(stage_results(h, tb, result_cap, out, caps, d_out));
    API_TRY(nfagg_timebased_results_device(h, tb, caps, d_out, n_out));
    return fetch_results(h, tb, out, d_out, n_out);
}

int nfagg_timebased_extract(nfagg_handle* h, nfagg_timebased* tb, const void* records, size_t n, const nfagg_pb_features* features,
                            const uint32_t* k8s_rows, const nfagg_net_row* net_rows, int64_t now_ns, const uint32_t* result_cap,
                            nfagg_tb_result* const* out, uint32_t* n_out, uint64_t* n_missing) {
    if (!h || !tb || !result_cap || !out || !n_out || !n_missing || (n && !records)) return fail(h, NFAGG_EINVAL, "null argument");
    *n_missing = 0;
    API_TRY(check_object(h, tb));
    if (features && features->struct_size != sizeof(nfagg_pb_features)) return fail(h, NFAGG_EINVAL, "nfagg_pb_features.struct_size mismatch");
    if (n > 0xFFFFFFFEull) return fail(h, NFAGG_ERANGE, "%zu flows, more than 2^32 - 2", n);
    auto& S = h->enc;
    HIP_TRY(h, hipSetDevice(h->device));
    uint32_t caps[kTbMaxRules];
    nfagg_tb_result* d_out[kTbMaxRules];
    API_TRY(stage_results(h, tb, result_cap, out, caps, d_out));
    API_TRY(stage_in(h, S.in_records, records, n * kRecordBytes));
    API_TRY(stage_in(h, S.k8s_rows, k8s_rows, k8s_rows ? n * 2 * sizeof(uint32_t) : 0));
    API_TRY(stage_in(h, S.net_rows, net_rows, net_rows ? n * sizeof(nfagg_net_row) : 0));
    nfagg_pb_features dfeat{};
    if (features && n) API_TRY(stage_pb_features(h, features, n, &dfeat));
    API_TRY(nfagg_timebased_extract_device(h, tb, n ? S.in_records.p : nullptr, n, (features && n) ? &dfeat : nullptr,
                                           (k8s_rows && n) ? S.k8s_rows.as<const uint32_t>() : nullptr, (net_rows && n) ? S.net_rows.as<const nfagg_net_row>() : nullptr,
                                           now_ns, caps, d_out, n_out, n_missing));
    return fetch_results(h, tb, out, d_out, n_out);
}

int nfagg_timebased_keys(nfagg_timebased* tb, uint32_t table, const uint32_t* keys, size_t n, nfagg_tb_key* out) {
    nfagg_handle* h = tb ? tb->h : nullptr;
    if (!tb || (n && (!keys || !out))) return fail(h, NFAGG_EINVAL, "null argument");
    if (!h || !tb->d_ctl) return fail(h, NFAGG_EINVAL, "the timebased rules were built on the host alone: they hold no key");
    if (table >= tb->n_tables) return fail(h, NFAGG_EINVAL, "table %u of %u", table, tb->n_tables);
    if (n > NFAGG_TB_MAX_KEYS) return fail(h, NFAGG_ERANGE, "%zu keys at once, more than %u", n, NFAGG_TB_MAX_KEYS);
    if (!n) return NFAGG_OK;
    const TbTable& T = tb->tables[table];
    HIP_TRY(h, hipSetDevice(h->device));
    API_TRY(stage_in(h, tb->key_ids, keys, n * sizeof(uint32_t)));
    API_TRY(tb->key_out.ensure(h, 16 + n * kTbSlotWords * 8));
    HIP_TRY(h, hipMemsetAsync(tb->key_out.p, 0, 16 + n * kTbSlotWords * 8, h->stream));
    const hipError_t e = launch_tb_gather_keys(table_dev(tb, table), T.n_keys, tb->key_ids.as<const uint32_t>(), (uint32_t)n,
                                               tb->key_out.as<uint64_t>() + 2, tb->key_out.as<uint32_t>(), h->stream);
    if (e != hipSuccess) return fail(h, NFAGG_EDEVICE, "timebased key gather launch failed: %s", hipGetErrorString(e));
    std::vector<uint64_t> w(2 + n * kTbSlotWords);
    HIP_TRY(h, hipMemcpyAsync(w.data(), tb->key_out.p, w.size() * 8, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if ((uint32_t)w[0]) return fail(h, NFAGG_EINVAL, "a key id is not below the table's %u keys", T.n_keys);
    for (size_t k = 0; k < n; k++) {
        const uint64_t* kw = w.data() + 2 + k * kTbSlotWords;
        uint32_t u[kTbMaxUnits + 2] = {};
        for (uint32_t b = 0; b < 32 * T.n_units; b++)                    // bit b of the raw string is bit b % 63 of key word b / 63
            if ((kw[b / 63] >> (b % 63)) & 1ull) u[b >> 5] |= 1u << (b & 31);
        memset(&out[k], 0, sizeof out[k]);
        uint32_t at = 0;
        for (uint32_t c = 0; c < T.n_cols; c++) {
            const uint32_t units = tb_col_is_addr(T.col[c]) ? 4u : 1u;
            memcpy(out[k].col[c], u + at, 4 * units);
            at += units;
        }
    }
    return NFAGG_OK;
}

int nfagg_timebased_class_row(const nfagg_timebased* tb, uint32_t table, uint32_t column, uint32_t cls, uint32_t* row) {
    nfagg_handle* h = tb ? tb->h : nullptr;
    if (!tb || !row) return fail(h, NFAGG_EINVAL, "null argument");
    if (table >= tb->n_tables || column >= tb->tables[table].n_cols || tb->tables[table].met_g[column] < 0)
        return fail(h, NFAGG_EINVAL, "table %u, column %u: not a Kubernetes column", table, column);
    const TbTable& T = tb->tables[table];
    return nfagg_metrics_class_row(T.met, (uint32_t)T.met_g[column], (int)((T.col[column] - kTbColK8s) >> 4), cls, row);
}

uint64_t nfagg_timebased_key_hash(const nfagg_timebased* tb, uint32_t table, const nfagg_tb_key* key) {
    if (!tb || !key || table >= tb->n_tables) return 0;
    const TbTable& T = tb->tables[table];
    uint32_t u[kTbMaxUnits + 4] = {}, at = 0;
    for (uint32_t c = 0; c < T.n_cols; c++) {
        const uint32_t units = tb_col_is_addr(T.col[c]) ? 4u : 1u;
        memcpy(u + at, key->col[c], 4 * units);
        at += units;
    }
    uint64_t raw[kTbRawWords];
    for (uint32_t j = 0; j < kTbRawWords; j++) raw[j] = (uint64_t)u[2 * j] | ((uint64_t)u[2 * j + 1] << 32);
    return tb_hash(raw);
}

int nfagg_timebased_reset(nfagg_timebased* tb) {
    if (!tb) return fail(nullptr, NFAGG_EINVAL, "null argument");
    if (!tb->h || !tb->d_ctl) { tb->failed = false; tb->has_clock = false; return NFAGG_OK; }
    return clear_device(tb);
}

int nfagg_timebased_stats(const nfagg_timebased* tb, nfagg_tb_stats* out) {
    if (!tb || !out) return fail(tb ? tb->h : nullptr, NFAGG_EINVAL, "null argument");
    memset(out, 0, sizeof *out);
    out->n_tables = tb->n_tables; out->n_rules = tb->n_rules;
    for (uint32_t t = 0; t < tb->n_tables; t++) {
        out->keys[t] = tb->tables[t].n_keys; out->slots[t] = tb->tables[t].slots; out->slices[t] = (uint32_t)tb->tables[t].slices.size();
    }
    for (uint32_t r = 0; r < tb->n_rules; r++) out->table_of_rule[r] = tb->rules[r].table;
    out->bytes_held = held_bytes(tb);
    out->last_now_ns = tb->last_now;
    out->failed = tb->failed ? 1u : 0u; out->has_clock = tb->has_clock ? 1u : 0u;
    return NFAGG_OK;
}

}  // extern "C"
