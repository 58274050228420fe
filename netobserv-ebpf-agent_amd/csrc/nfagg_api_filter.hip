// nfagg_api_filter.hip — the host side of the transform filter stage (include/nfagg.h, "transform filter"): the spec's checks and
// its compiled form, the roll as a pure host function, nfagg_filter_apply and nfagg_gather with their host-memory variants.
#include <string.h>

#include <new>
#include <vector>

#include "nfagg_api_tables.h"
#include "nfagg_api_call.h"
#include "nfagg_filter.h"

using namespace nfagg;

// The filter of nfagg_filter_create: the compiled program and the truth bytes, on the host and (with a handle) on its device;
// the per-call scratch that no other entry point has (the sampling to store, the deferred counter).
struct nfagg_filter {
    nfagg_handle* h = nullptr;
    const nfagg_k8s_table* k8s = nullptr;      // not owned: the caller keeps them alive
    const nfagg_net_table* net = nullptr;
    FilterProg prog{};
    std::vector<uint8_t> truth;
    DevBuf d_prog;                             // the program, then the truth bytes from kTruthOff on
    DevBuf d_samp;                             // u32[n], and one counter in front
};

namespace {

constexpr size_t kTruthOff = (sizeof(FilterProg) + 255) / 256 * 256;
constexpr size_t kMaxFlows = 0xFFFFFFFEull;

const char* const kFieldNames[NFAGG_FILTER_F_LAST + 1] = {
    "Etype", "Bytes", "Packets", "Sampling", "Proto", "Dscp", "SrcPort", "DstPort", "IcmpType", "IcmpCode", "Flags", "TimeFlowStartMs", "TimeFlowEndMs",
    "FlowDirection", "TimeFlowRttNs", "DnsLatencyMs", "DnsId", "DnsFlags", "DnsErrno", "PktDropBytes", "PktDropPackets", "PktDropLatestFlags",
    "IPSecRetCode", "SrcAddr", "DstAddr", "SrcMac", "DstMac"};

uint32_t field_need(uint32_t f) {
    switch (f) {
    case NFAGG_FILTER_F_TIME_FLOW_START_MS: case NFAGG_FILTER_F_TIME_FLOW_END_MS: return kFilterNeedClock;
    case NFAGG_FILTER_F_FLOW_DIRECTION: return kFilterNeedNet;
    case NFAGG_FILTER_F_TIME_FLOW_RTT_NS: case NFAGG_FILTER_F_IPSEC_RET_CODE: return kFilterNeedAdditional;
    case NFAGG_FILTER_F_DNS_LATENCY_MS: case NFAGG_FILTER_F_DNS_ID: case NFAGG_FILTER_F_DNS_FLAGS: case NFAGG_FILTER_F_DNS_ERRNO: return kFilterNeedDns;
    case NFAGG_FILTER_F_PKT_DROP_BYTES: case NFAGG_FILTER_F_PKT_DROP_PACKETS: case NFAGG_FILTER_F_PKT_DROP_LATEST_FLAGS: return kFilterNeedDrops;
    default: return 0;
    }
}

// One atom checked and compiled into *o; its truth bytes appended to `truth`.
int compile_atom(nfagg_handle* h, uint32_t k, const nfagg_filter_atom& a, const nfagg_k8s_table* k8s, const nfagg_net_table* net, FilterAtom* o,
                 std::vector<uint8_t>& truth, uint32_t* need) {
    if (a.pad_[0] | a.pad_[1]) return fail(h, NFAGG_EINVAL, "filter atom %u: non-zero padding", k);
    *o = FilterAtom{};
    o->kind = a.kind;
    switch (a.kind) {
    case NFAGG_FILTER_ATOM_CONST:
        o->a = a.value_const != 0;
        return NFAGG_OK;
    case NFAGG_FILTER_ATOM_NUM:
    case NFAGG_FILTER_ATOM_PRESENT:
        if (a.field > NFAGG_FILTER_F_LAST) return fail(h, NFAGG_EINVAL, "filter atom %u: unknown field %u", k, a.field);
        if (a.kind == NFAGG_FILTER_ATOM_NUM) {
            if (a.field > NFAGG_FILTER_F_NUM_LAST) return fail(h, NFAGG_EINVAL, "filter atom %u: %s is a presence-only field", k, kFieldNames[a.field]);
            if (a.cmp > NFAGG_FILTER_CMP_GE) return fail(h, NFAGG_EINVAL, "filter atom %u: unknown comparison %u", k, a.cmp);
            o->cmp = a.cmp; o->value = a.value;
        }
        o->a = a.field;
        *need |= field_need(a.field);
        return NFAGG_OK;
    case NFAGG_FILTER_ATOM_TABLE: {
        size_t want = 0;
        switch (a.dim) {
        case NFAGG_FILTER_DIM_SRC_K8S_ROW: case NFAGG_FILTER_DIM_DST_K8S_ROW:
            if (!k8s) return fail(h, NFAGG_EINVAL, "filter atom %u: a Kubernetes-row table atom without a Kubernetes table", k);
            want = k8s->rows.size() + 1; *need |= kFilterNeedK8s;
            break;
        case NFAGG_FILTER_DIM_SRC_SUBNET_LABEL: case NFAGG_FILTER_DIM_DST_SUBNET_LABEL:
            if (!net) return fail(h, NFAGG_EINVAL, "filter atom %u: a subnet-label table atom without a net table", k);
            want = net->frags.size() + 1; *need |= kFilterNeedNet;
            break;
        case NFAGG_FILTER_DIM_FLOW_LAYER:
            if (!k8s) return fail(h, NFAGG_EINVAL, "filter atom %u: a flow-layer table atom without a Kubernetes table", k);
            want = 3; *need |= kFilterNeedK8s | kFilterNeedK8sRow;
            break;
        case NFAGG_FILTER_DIM_DNS_RCODE: want = 17; *need |= kFilterNeedDns; break;
        case NFAGG_FILTER_DIM_IPSEC_STATUS: want = 3; *need |= kFilterNeedAdditional; break;
        default: return fail(h, NFAGG_EINVAL, "filter atom %u: unknown dimension %u", k, a.dim);
        }
        if (!a.truth) return fail(h, NFAGG_EINVAL, "filter atom %u: null truth bytes", k);
        if (a.n_truth != want) return fail(h, NFAGG_EINVAL, "filter atom %u: %u truth entries, its dimension has %zu", k, a.n_truth, want);
        o->a = a.dim; o->n_truth = a.n_truth; o->truth_off = truth.size();
        truth.insert(truth.end(), a.truth, a.truth + a.n_truth);
        return NFAGG_OK;
    }
    case NFAGG_FILTER_ATOM_ADDR:
    case NFAGG_FILTER_ATOM_MAC:
        if (a.side > 1) return fail(h, NFAGG_EINVAL, "filter atom %u: unknown side %u", k, a.side);
        o->a = a.side;
        memcpy(o->w, a.bytes, a.kind == NFAGG_FILTER_ATOM_ADDR ? 16 : 6);
        return NFAGG_OK;
    default:
        return fail(h, NFAGG_EINVAL, "filter atom %u: unknown kind %u", k, a.kind);
    }
}

int grow_samp(nfagg_handle* h, nfagg_filter* f, size_t n) { return f->d_samp.ensure(h, 16 + (n + 4) * sizeof(uint32_t)); }

}  // namespace

extern "C" {

int nfagg_filter_roll(uint64_t seed, uint64_t flow_index, uint32_t step, uint32_t value) { return filter_roll(seed, flow_index, step, value) ? 1 : 0; }

int nfagg_filter_create(nfagg_handle* h, const nfagg_k8s_table* k8s_table, const nfagg_net_table* net_table, const nfagg_filter_spec* spec,
                        nfagg_filter** filter) {
    if (!filter || !spec) return fail(h, NFAGG_EINVAL, "null argument");
    *filter = nullptr;
    if (spec->struct_size != sizeof(nfagg_filter_spec)) return fail(h, NFAGG_EINVAL, "nfagg_filter_spec.struct_size mismatch");
    if (spec->flags & ~NFAGG_FILTER_STORE_SAMPLING) return fail(h, NFAGG_EINVAL, "unknown filter flags 0x%x", spec->flags & ~NFAGG_FILTER_STORE_SAMPLING);
    if (spec->pad_) return fail(h, NFAGG_EINVAL, "nfagg_filter_spec: non-zero padding");
    if (spec->n_atoms > kFilterMaxAtoms) return fail(h, NFAGG_EINVAL, "%u filter atoms, more than %u", spec->n_atoms, kFilterMaxAtoms);
    if (spec->n_ops > kFilterMaxOps) return fail(h, NFAGG_EINVAL, "%u filter ops, more than %u", spec->n_ops, kFilterMaxOps);
    if (spec->n_steps > kFilterMaxSteps) return fail(h, NFAGG_EINVAL, "%u filter steps, more than %u", spec->n_steps, kFilterMaxSteps);
    if ((spec->n_atoms && !spec->atoms) || (spec->n_ops && !spec->ops) || (spec->n_steps && !spec->steps)) return fail(h, NFAGG_EINVAL, "null list with a count");
    if (k8s_table && k8s_table->h != h) return fail(h, NFAGG_EINVAL, "the Kubernetes table was not created for this handle");
    if (net_table && net_table->h != h) return fail(h, NFAGG_EINVAL, "the net table was not created for this handle");
    nfagg_filter* f = new (std::nothrow) nfagg_filter;
    if (!f) return fail(h, NFAGG_ENOMEM, "out of memory");
    f->h = h; f->k8s = k8s_table; f->net = net_table;
    FilterProg& P = f->prog;
    P.n_atoms = spec->n_atoms; P.n_ops = spec->n_ops; P.n_steps = spec->n_steps;
    P.flags = ((spec->flags & NFAGG_FILTER_STORE_SAMPLING) ? kFilterStore : 0u) |
              ((net_table && (net_table->flags & NFAGG_NET_DECODE_TCP_FLAGS)) ? kFilterFlagNames : 0u);
    int rc = NFAGG_OK;
    for (uint32_t k = 0; k < spec->n_atoms && rc == NFAGG_OK; k++) rc = compile_atom(h, k, spec->atoms[k], k8s_table, net_table, &P.atoms[k], f->truth, &P.need);
    for (uint32_t k = 0; k < spec->n_ops && rc == NFAGG_OK; k++) {
        const uint8_t op = spec->ops[k];
        if (op < kFilterMaxAtoms ? op >= spec->n_atoms : (op != NFAGG_FILTER_OP_AND && op != NFAGG_FILTER_OP_OR && op != NFAGG_FILTER_OP_NOT))
            rc = op < kFilterMaxAtoms ? fail(h, NFAGG_EINVAL, "filter op %u: atom %u of %u", k, op, spec->n_atoms) : fail(h, NFAGG_EINVAL, "filter op %u: unknown op 0x%02x", k, op);
        P.ops[k] = op;
    }
    for (uint32_t s = 0; s < spec->n_steps && rc == NFAGG_OK; s++) {
        const nfagg_filter_step& st = spec->steps[s];
        if (st.kind > NFAGG_FILTER_STEP_SAMPLE_IF) { rc = fail(h, NFAGG_EINVAL, "filter step %u: unknown kind %u", s, st.kind); break; }
        if (st.kind == NFAGG_FILTER_STEP_KEEP) {
            if (P.n_keep != s) { rc = fail(h, NFAGG_EINVAL, "filter step %u: a KEEP step behind a step of another kind", s); break; }
            P.n_keep = s + 1;
        }
        if (st.group > 31 || (st.kind != NFAGG_FILTER_STEP_SAMPLE_IF && st.group)) { rc = fail(h, NFAGG_EINVAL, "filter step %u: group %u", s, st.group); break; }
        if (st.kind == NFAGG_FILTER_STEP_REMOVE && st.value) { rc = fail(h, NFAGG_EINVAL, "filter step %u: a REMOVE step with a sampling value", s); break; }
        if ((uint32_t)st.op_begin + st.op_count > spec->n_ops) { rc = fail(h, NFAGG_EINVAL, "filter step %u: ops [%u, %u) of %u", s, st.op_begin, st.op_begin + st.op_count, spec->n_ops); break; }
        uint32_t depth = 0;
        for (uint32_t pc = st.op_begin; pc < (uint32_t)st.op_begin + st.op_count && rc == NFAGG_OK; pc++) {
            const uint8_t op = spec->ops[pc];
            if (op < kFilterMaxAtoms) {
                if (++depth > kFilterMaxStack) rc = fail(h, NFAGG_EINVAL, "filter step %u: op %u grows the stack beyond %u", s, pc, kFilterMaxStack);
            } else if (op == NFAGG_FILTER_OP_NOT) {
                if (depth < 1) rc = fail(h, NFAGG_EINVAL, "filter step %u: op %u underflows the stack", s, pc);
            } else {
                if (depth < 2) rc = fail(h, NFAGG_EINVAL, "filter step %u: op %u underflows the stack", s, pc);
                else depth--;
            }
        }
        if (rc == NFAGG_OK && depth != 1) rc = fail(h, NFAGG_EINVAL, "filter step %u: its ops leave %u values, not one", s, depth);
        P.steps[s].kind = st.kind; P.steps[s].group = st.group; P.steps[s].value = st.value; P.steps[s].op_begin = st.op_begin; P.steps[s].op_count = st.op_count;
    }
    if (rc != NFAGG_OK) { delete f; return rc; }
    if (h) {
        if ((k8s_table && !k8s_table->d_slots) || (net_table && !net_table->d_mem)) { delete f; return fail(h, NFAGG_EINVAL, "a table without a device copy"); }
        auto up = [&]() -> int {
            std::vector<uint8_t> img(kTruthOff + f->truth.size() + 16, 0);
            memcpy(img.data(), &f->prog, sizeof(FilterProg));
            if (!f->truth.empty()) memcpy(img.data() + kTruthOff, f->truth.data(), f->truth.size());
            HIP_TRY(h, hipSetDevice(h->device));
            HIP_TRY(h, f->d_prog.alloc(img.size()));
            HIP_TRY(h, hipMemcpy(f->d_prog.p, img.data(), img.size(), hipMemcpyHostToDevice));
            return NFAGG_OK;
        };
        rc = up();
        if (rc != NFAGG_OK) { nfagg_filter_destroy(f); return rc; }
    }
    *filter = f;
    return NFAGG_OK;
}

void nfagg_filter_destroy(nfagg_filter* f) { destroy_on_handle(f); }

int nfagg_filter_apply_device(nfagg_handle* h, const nfagg_filter* filter, const void* d_records, size_t n, const nfagg_pb_features* d_features,
                              const uint32_t* d_k8s_rows, const nfagg_net_row* d_net_rows, const nfagg_flp_options* opt, uint64_t seed,
                              uint64_t first_index, uint8_t* d_keep, uint8_t* d_rule, uint32_t* d_kept_idx, void* d_out_records, size_t cap,
                              size_t* n_kept, size_t* n_deferred) {
    if (!h || !filter || !n_kept || (n && !d_records)) return fail(h, NFAGG_EINVAL, "null argument");
    *n_kept = 0;
    if (n_deferred) *n_deferred = 0;
    if (filter->h != h || !filter->d_prog) return fail(h, NFAGG_EINVAL, "the filter was not created for this handle");
    if (n > kMaxFlows) return fail(h, NFAGG_ERANGE, "%zu records: more than 2^32 - 2 in one call", n);
    const FilterProg& P = filter->prog;
    if (n && (P.need & kFilterNeedK8s) && !d_k8s_rows) return fail(h, NFAGG_EINVAL, "the filter reads the flows' Kubernetes rows");
    if (n && (P.need & kFilterNeedNet) && !d_net_rows) return fail(h, NFAGG_EINVAL, "the filter reads the flows' net rows");
    FilterClock clk{};
    if (P.need & kFilterNeedClock) {
        if (!opt) return fail(h, NFAGG_EINVAL, "the filter reads the flow times: the options are required");
        if (opt->struct_size != sizeof(nfagg_flp_options)) return fail(h, NFAGG_EINVAL, "nfagg_flp_options.struct_size mismatch");
        split_now(opt->now_unix_ns, clk.now_sec, clk.now_nsec);
        clk.mono_now = opt->mono_now_ns;
    }
    PbFeat F{};
    if (d_features) { int rc = device_features(h, d_features, &F); if (rc != NFAGG_OK) return rc; }
    if (((uintptr_t)d_records & 15u) != 0 || ((uintptr_t)d_out_records & 15u) != 0 || ((uintptr_t)d_k8s_rows & 7u) != 0 || ((uintptr_t)d_net_rows & 7u) != 0 ||
        ((uintptr_t)d_kept_idx & 3u) != 0)
        return fail(h, NFAGG_EINVAL, "device records must be 16-byte, rows 8-byte, kept_idx 4-byte aligned");
    HIP_TRY(h, hipSetDevice(h->device));
    if (!n) return NFAGG_OK;
    auto& S = h->enc;
    nfagg_filter* f = const_cast<nfagg_filter*>(filter);          // the scratch alone
    const size_t blocks = (n + kFilterScanBlock - 1) / kFilterScanBlock;
    API_TRY(ensure_all(h, {{S.local_off, (n + 1) * sizeof(uint32_t)}, {S.block_sum, blocks * sizeof(uint32_t)}, {S.block_base, (blocks + 1) * sizeof(uint64_t)}}));
    API_TRY(grow_samp(h, f, n));
    uint32_t* d_counter = f->d_samp.as<uint32_t>();
    uint32_t* d_samp = d_counter + 4;
    HIP_TRY(h, hipMemsetAsync(d_counter, 0, 16, h->stream));
    const K8sDev K = (P.need & kFilterNeedK8sRow) ? k8s_dev(filter->k8s) : K8sDev{};
    hipError_t e = launch_filter_eval(d_records, n, f->d_prog.as<const FilterProg>(), f->d_prog.as<const uint8_t>() + kTruthOff, F, d_k8s_rows, K,
                                      (const uint2*)d_net_rows, clk, seed, first_index, d_keep, d_rule, d_samp, S.local_off.as<uint32_t>(),
                                      S.block_sum.as<uint32_t>(), S.block_base.as<uint64_t>(), d_counter, h->stream);
    if (e != hipSuccess) return fail(h, NFAGG_EDEVICE, "filter eval launch failed: %s", hipGetErrorString(e));
    uint64_t total = 0;
    uint32_t deferred = 0;
    HIP_TRY(h, hipMemcpyAsync(&total, S.block_base.as<const uint64_t>() + blocks, sizeof total, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipMemcpyAsync(&deferred, d_counter, sizeof deferred, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    *n_kept = (size_t)total;
    if (n_deferred) *n_deferred = deferred;
    if (!d_kept_idx && !d_out_records) return NFAGG_OK;
    if (total > cap) return NFAGG_TRUNCATED;
    if (total) {
        e = launch_filter_compact(d_records, n, d_samp, S.local_off.as<const uint32_t>(), S.block_base.as<const uint64_t>(), d_kept_idx, d_out_records, h->stream);
        if (e != hipSuccess) return fail(h, NFAGG_EDEVICE, "filter compact launch failed: %s", hipGetErrorString(e));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
    }
    return NFAGG_OK;
}

int nfagg_filter_apply(nfagg_handle* h, const nfagg_filter* filter, const void* records, size_t n, const nfagg_pb_features* features,
                       const uint32_t* k8s_rows, const nfagg_net_row* net_rows, const nfagg_flp_options* opt, uint64_t seed, uint64_t first_index,
                       uint8_t* keep, uint8_t* rule, uint32_t* kept_idx, void* out_records, size_t cap, size_t* n_kept, size_t* n_deferred) {
    if (!h || !filter || !n_kept || (n && !records)) return fail(h, NFAGG_EINVAL, "null argument");
    *n_kept = 0;
    if (n_deferred) *n_deferred = 0;
    if (n > kMaxFlows) return fail(h, NFAGG_ERANGE, "%zu records: more than 2^32 - 2 in one call", n);
    if (features && features->struct_size != sizeof(nfagg_pb_features)) return fail(h, NFAGG_EINVAL, "nfagg_pb_features.struct_size mismatch");
    auto& S = h->enc;
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t room = cap < n ? cap : n;              // never more kept than flows
    API_TRY(ensure_all(h, {{S.out_extra[0], n + kStageSlack}, {S.out_extra[1], n + kStageSlack}, {S.out_offsets, room * sizeof(uint32_t) + kStageSlack},
                           {S.out, out_records ? room * kRecordBytes + kStageSlack : 0}}));
    API_TRY(stage_in(h, S.in_records, records, n * kRecordBytes));
    API_TRY(stage_in(h, S.k8s_rows, k8s_rows, k8s_rows ? n * 2 * sizeof(uint32_t) : 0));
    API_TRY(stage_in(h, S.net_rows, net_rows, net_rows ? n * sizeof(nfagg_net_row) : 0));
    nfagg_pb_features dfeat{};
    if (features && n) API_TRY(stage_pb_features(h, features, n, &dfeat));
    const bool compact = kept_idx || out_records;
    const int rc = nfagg_filter_apply_device(h, filter, S.in_records.p, n, (features && n) ? &dfeat : nullptr, k8s_rows ? S.k8s_rows.as<const uint32_t>() : nullptr,
                                   net_rows ? S.net_rows.as<const nfagg_net_row>() : nullptr, opt, seed, first_index, S.out_extra[0].as<uint8_t>(),
                                   S.out_extra[1].as<uint8_t>(), compact ? S.out_offsets.as<uint32_t>() : nullptr, out_records ? S.out.p : nullptr, room,
                                   n_kept, n_deferred);
    if (rc != NFAGG_OK && rc != NFAGG_TRUNCATED) return rc;
    API_TRY(fetch(h, keep, S.out_extra[0], keep ? n : 0));
    API_TRY(fetch(h, rule, S.out_extra[1], rule ? n : 0));
    if (rc == NFAGG_OK) {
        API_TRY(fetch(h, kept_idx, S.out_offsets, kept_idx ? *n_kept * sizeof(uint32_t) : 0));
        API_TRY(fetch(h, out_records, S.out, out_records ? *n_kept * kRecordBytes : 0));
    }
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return rc;
}

static int gather_unit(size_t elem_bytes) {
    if (elem_bytes == 1 || elem_bytes == 2 || elem_bytes == 4) return (int)elem_bytes;
    if (elem_bytes >= 8 && elem_bytes <= 64 && elem_bytes % 8 == 0) return 8;
    return 0;
}

int nfagg_gather_device(nfagg_handle* h, const void* d_src, size_t n_src, size_t elem_bytes, const uint32_t* d_kept_idx, size_t n_kept, void* d_dst) {
    if (!h) return fail(h, NFAGG_EINVAL, "null argument");
    uint32_t unit = (uint32_t)gather_unit(elem_bytes);
    if (!unit) return fail(h, NFAGG_EINVAL, "gather of %zu-byte elements: not 1, 2, 4, 8 or a multiple of 8 up to 64", elem_bytes);
    if (n_kept && (!d_src || !d_kept_idx || !d_dst)) return fail(h, NFAGG_EINVAL, "null argument");
    if (n_kept > kMaxFlows || n_src > kMaxFlows) return fail(h, NFAGG_ERANGE, "more than 2^32 - 2 elements in one call");
    if ((((uintptr_t)d_src | (uintptr_t)d_dst) & (unit - 1)) != 0 || ((uintptr_t)d_kept_idx & 3u) != 0)
        return fail(h, NFAGG_EINVAL, "gather of %zu-byte elements: src and dst must be %u-byte, kept_idx 4-byte aligned", elem_bytes, unit);
    if (unit == 8 && elem_bytes % 16 == 0 && (((uintptr_t)d_src | (uintptr_t)d_dst) & 15u) == 0) unit = 16;
    HIP_TRY(h, hipSetDevice(h->device));
    if (!n_kept) return NFAGG_OK;
    hipError_t e = launch_gather(d_src, n_src, (uint32_t)elem_bytes, unit, d_kept_idx, n_kept, d_dst, h->stream);
    if (e != hipSuccess) return fail(h, NFAGG_EDEVICE, "gather launch failed: %s", hipGetErrorString(e));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return NFAGG_OK;
}

int nfagg_gather(nfagg_handle* h, const void* src, size_t n_src, size_t elem_bytes, const uint32_t* kept_idx, size_t n_kept, void* dst) {
    if (!h) return fail(h, NFAGG_EINVAL, "null argument");
    if (!gather_unit(elem_bytes)) return fail(h, NFAGG_EINVAL, "gather of %zu-byte elements: not 1, 2, 4, 8 or a multiple of 8 up to 64", elem_bytes);
    if (n_kept && (!kept_idx || !dst)) return fail(h, NFAGG_EINVAL, "null argument");
    if (n_src && !src) return fail(h, NFAGG_EINVAL, "null argument");
    if (n_kept > kMaxFlows || n_src > kMaxFlows) return fail(h, NFAGG_ERANGE, "more than 2^32 - 2 elements in one call");
    auto& S = h->enc;
    HIP_TRY(h, hipSetDevice(h->device));
    if (!n_kept) return NFAGG_OK;
    API_TRY(S.out.ensure(h, n_kept * elem_bytes + kStageSlack));
    API_TRY(stage_in(h, S.in_records, src, n_src * elem_bytes));
    API_TRY(stage_in(h, S.out_offsets, kept_idx, n_kept * sizeof(uint32_t)));
    API_TRY(nfagg_gather_device(h, S.in_records.p, n_src, elem_bytes, S.out_offsets.as<const uint32_t>(), n_kept, S.out.p));
    API_TRY(fetch(h, dst, S.out, n_kept * elem_bytes));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return NFAGG_OK;
}

}  // extern "C"
