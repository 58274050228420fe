// nfagg_api_flp_ipfix.hip — the host side of write ipfix on the device (include/nfagg.h, "write ipfix on the device";
// nfagg_flp_ipfix.h): the template message, the strings table, the writer (the element state of both families and the call's
// own scratch; the scans, the namer table and the host entry point's staging are the handle's, nfagg_api_call.h),
// nfagg_flp_ipfix_write[_device]. A write costs the upload of the namer table, the launches of nfagg_flp_ipfix.hip and one
// 16-byte read-back (bytes and sent flows) between the size pass and the write pass.
#include <hip/hip_runtime.h>
#include <string.h>
#include <algorithm>
#include <new>
#include <vector>

#include "../../include/nfagg.h"
#include "nfagg_internal.h"
#include "nfagg_handle.h"
#include "nfagg_api_call.h"
#include "nfagg_api_tables.h"
#include "nfagg_flp_ipfix.h"

using namespace nfagg;

struct nfagg_flp_ipfix_strings {
    nfagg_handle* h = nullptr;
    std::vector<IxStrRow> rows;
    std::vector<uint8_t> blob;
    DevBuf d_rows, d_blob;
};

struct nfagg_flp_ipfix_writer {
    nfagg_handle* h = nullptr;
    DevBuf state;                                                      // nfagg_flp_ipfix_elements[2]: v4, v6
    DevBuf meta, src, agg, pre, rows, seq_local, seq_sum, seq_base;     // the plan pass's arrays and the scan of the sent flows
};

namespace {

// prepareTemplate's element lists: (element id, length), registry/registry_IANA.go; write_ipfix.go:60-108
const uint16_t kLeadV4[6][2] = {{8, 4}, {12, 4}, {176, 1}, {177, 1}, {225, 4}, {226, 4}};
const uint16_t kLeadV6[7][2] = {{27, 16}, {28, 16}, {193, 1}, {178, 1}, {179, 1}, {281, 16}, {282, 16}};
const uint16_t kCommon[17][2] = {{256, 2}, {61, 1}, {56, 6}, {80, 6}, {4, 1}, {7, 2}, {11, 2}, {1, 8}, {152, 8}, {153, 8}, {2, 8},
                                 {82, 65535}, {6, 2}, {227, 2}, {228, 2}, {304, 2}, {311, 8}};
const uint16_t kEnterprise[9][2] = {{7733, 65535}, {7734, 65535}, {7735, 65535}, {7736, 65535}, {7737, 65535}, {7738, 65535},
                                    {7740, 8}, {7741, 65535}, {7742, 65535}};

int check_options(nfagg_handle* h, const nfagg_flp_ipfix_options* opt) {
    if (!opt) return fail(h, NFAGG_EINVAL, "null options");
    if (opt->struct_size != sizeof(nfagg_flp_ipfix_options)) return fail(h, NFAGG_EINVAL, "nfagg_flp_ipfix_options.struct_size mismatch");
    if (opt->max_msg_size > 65535u) return fail(h, NFAGG_EINVAL, "max_msg_size %u, more than 65535", opt->max_msg_size);
    return check_namer(h, opt->names, opt->n_names, opt->unknown_len, false);
}

// NewWriteIpfix's element lists (DecodeAndCreateInfoElementWithValue with a nil value): numbers 0, strings empty, addresses
// and MACs nil
void initial_state(nfagg_flp_ipfix_elements* e) {
    memset(e, 0, 2 * sizeof *e);
    e[0].struct_size = e[1].struct_size = sizeof *e;
}

}  // namespace

extern "C" {

int nfagg_flp_ipfix_template(const nfagg_flp_ipfix_options* opt, int v6, void* out, size_t cap, size_t* n_out) {
    if (!opt || !n_out) return fail(nullptr, NFAGG_EINVAL, "null argument");
    if (opt->struct_size != sizeof(nfagg_flp_ipfix_options)) return fail(nullptr, NFAGG_EINVAL, "nfagg_flp_ipfix_options.struct_size mismatch");
    return ipfix_template_message({opt->export_time_s, opt->seq0, opt->obs_domain_id, v6 ? opt->template_id_v6 : opt->template_id_v4},
                                  {v6 ? IpfixFields{kLeadV6, 7} : IpfixFields{kLeadV4, 6}, {kCommon, 17}}, {kEnterprise, 9}, opt->enterprise_id, out, cap, n_out);
}

int nfagg_flp_ipfix_strings_create(nfagg_handle* h, const nfagg_k8s_entry* entries, size_t n, nfagg_flp_ipfix_strings** strings) {
    if (!strings || (n && !entries)) return fail(h, NFAGG_EINVAL, "null argument");
    *strings = nullptr;
    if (n > NFAGG_K8S_MAX_ROWS) return fail(h, NFAGG_EINVAL, "%zu entries, more than %u", n, NFAGG_K8S_MAX_ROWS);
    nfagg_flp_ipfix_strings* t = new (std::nothrow) nfagg_flp_ipfix_strings;
    if (!t) return fail(h, NFAGG_ENOMEM, "out of memory");
    t->h = h;
    t->rows.resize(n);
    for (size_t r = 0; r < n; r++) {
        const nfagg_k8s_entry& e = entries[r];
        const char* text[3] = {e.namespace_, e.name, e.host_name};
        const uint32_t len[3] = {e.namespace_len, e.name_len, e.host_name_len};
        static const char* const what[3] = {"namespace", "name", "host_name"};
        if (e.host_ip_len && !e.host_ip) { delete t; return fail(h, NFAGG_EINVAL, "entry %zu: host_ip is null with a length", r); }
        IxStrRow& row = t->rows[r];
        row = IxStrRow{};
        for (int f = 0; f < 3; f++) {
            if (len[f] && !text[f]) { delete t; return fail(h, NFAGG_EINVAL, "entry %zu: %s is null with a length", r, what[f]); }
            if (len[f] > NFAGG_FLP_IPFIX_MAX_STRING) {
                delete t;
                return fail(h, NFAGG_EINVAL, "entry %zu: %s has %u bytes, more than %u", r, what[f], len[f], NFAGG_FLP_IPFIX_MAX_STRING);
            }
            if ((t->blob.size() + len[f] + 32) >> 32) { delete t; return fail(h, NFAGG_ERANGE, "the strings come to 2^32 bytes or more"); }
            row.off[f] = (uint32_t)t->blob.size(); row.len[f] = len[f];
            if (len[f]) t->blob.insert(t->blob.end(), text[f], text[f] + len[f]);
            t->blob.resize((t->blob.size() + 15) / 16 * 16, 0);
        }
        // nfagg_k8s_render's presence: Name always, Namespace when not empty, HostName when HostIP and HostName are not empty
        row.present = (e.namespace_len ? 1u : 0u) | 2u | ((e.host_ip_len && e.host_name_len) ? 4u : 0u);
    }
    t->blob.resize(t->blob.size() + 16, 0);                          // an offset is always inside the blob
    if (h) {
        auto upload = [&]() -> int {
            HIP_TRY(h, hipSetDevice(h->device));
            HIP_TRY(h, t->d_rows.alloc(std::max<size_t>(n * sizeof(IxStrRow), 32)));
            HIP_TRY(h, t->d_blob.alloc(t->blob.size()));
            if (n) HIP_TRY(h, hipMemcpy(t->d_rows.p, t->rows.data(), n * sizeof(IxStrRow), hipMemcpyHostToDevice));
            HIP_TRY(h, hipMemcpy(t->d_blob.p, t->blob.data(), t->blob.size(), hipMemcpyHostToDevice));
            return NFAGG_OK;
        };
        const int rc = upload();
        if (rc != NFAGG_OK) { nfagg_flp_ipfix_strings_destroy(t); return rc; }
    }
    *strings = t;
    return NFAGG_OK;
}

void nfagg_flp_ipfix_strings_destroy(nfagg_flp_ipfix_strings* t) { destroy_on_handle(t); }

int nfagg_flp_ipfix_writer_create(nfagg_handle* h, nfagg_flp_ipfix_writer** writer) {
    if (!h || !writer) return fail(h, NFAGG_EINVAL, "null argument");
    *writer = nullptr;
    nfagg_flp_ipfix_writer* w = new (std::nothrow) nfagg_flp_ipfix_writer;
    if (!w) return fail(h, NFAGG_ENOMEM, "out of memory");
    w->h = h;
    auto init = [&]() -> int {
        HIP_TRY(h, hipSetDevice(h->device));
        HIP_TRY(h, w->state.alloc(2 * sizeof(nfagg_flp_ipfix_elements)));
        return nfagg_flp_ipfix_writer_reset(w);
    };
    const int rc = init();
    if (rc != NFAGG_OK) { nfagg_flp_ipfix_writer_destroy(w); return rc; }
    *writer = w;
    return NFAGG_OK;
}

void nfagg_flp_ipfix_writer_destroy(nfagg_flp_ipfix_writer* w) { destroy_on_handle(w); }

int nfagg_flp_ipfix_writer_reset(nfagg_flp_ipfix_writer* w) {
    if (!w) return fail(nullptr, NFAGG_EINVAL, "null argument");
    nfagg_handle* h = w->h;
    std::vector<nfagg_flp_ipfix_elements> init(2);
    initial_state(init.data());
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    HIP_TRY(h, hipMemcpy(w->state.p, init.data(), 2 * sizeof(nfagg_flp_ipfix_elements), hipMemcpyHostToDevice));
    return NFAGG_OK;
}

int nfagg_flp_ipfix_writer_get(nfagg_flp_ipfix_writer* w, int v6, nfagg_flp_ipfix_elements* out) {
    if (!w || !out) return fail(w ? w->h : nullptr, NFAGG_EINVAL, "null argument");
    nfagg_handle* h = w->h;
    if (v6 != 0 && v6 != 1) return fail(h, NFAGG_EINVAL, "unknown family %d", v6);
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    HIP_TRY(h, hipMemcpy(out, w->state.as<nfagg_flp_ipfix_elements>() + v6, sizeof *out, hipMemcpyDeviceToHost));
    return NFAGG_OK;
}

int nfagg_flp_ipfix_write_device(nfagg_handle* h, nfagg_flp_ipfix_writer* w, const void* d_records, size_t n,
                                 const nfagg_pb_features* d_features, const uint32_t* d_k8s_rows,
                                 const nfagg_flp_ipfix_strings* strings, const nfagg_flp_ipfix_options* opt, void* d_out,
                                 size_t out_cap, uint64_t* d_msg_offsets, uint8_t* d_status, size_t* n_sent, size_t* out_bytes) {
    int rc = check_options(h, opt);
    if (rc != NFAGG_OK) return rc;
    if (!h || !w || !out_bytes || !n_sent || !d_msg_offsets || (n && (!d_records || !d_status))) return fail(h, NFAGG_EINVAL, "null argument");
    if (w->h != h) return fail(h, NFAGG_EINVAL, "the writer was not created for this handle");
    if (d_k8s_rows && !strings) return fail(h, NFAGG_EINVAL, "Kubernetes rows without the strings table they index");
    if (strings && (strings->h != h || !strings->d_rows)) return fail(h, NFAGG_EINVAL, "the strings table was not created for this handle");
    if ((((uintptr_t)d_records | (uintptr_t)d_out) & 15u) != 0 || (((uintptr_t)d_k8s_rows | (uintptr_t)d_msg_offsets) & 7u) != 0)
        return fail(h, NFAGG_EINVAL, "device records and output must be 16-byte, rows and offsets 8-byte aligned");
    if (n > (1ull << 30)) return fail(h, NFAGG_ERANGE, "%zu flows in one call, more than 2^30", n);
    PbFeat F{};
    if (d_features && (rc = device_features(h, d_features, &F)) != NFAGG_OK) return rc;
    *n_sent = 0;
    bool done;
    if ((rc = encode_begin(h, n, d_msg_offsets, out_bytes, opt->names, opt->n_names, &done)) != NFAGG_OK || done) return rc;
    const size_t blocks = (n + 1023) / 1024, stride = blocks + 1;
    API_TRY(ensure_all(h, {{w->meta, n * 4}, {w->src, n * kIxGroups * 4}, {w->agg, 2 * kIxAggs * stride * 4}, {w->pre, 2 * kIxAggs * stride * 4},
                           {w->rows, n * 32}, {w->seq_local, n * 4}, {w->seq_sum, blocks * 4}, {w->seq_base, (blocks + 1) * 8}}));
    IxArgs A{};
    A.recs = d_records; A.n = n; A.F = F;
    A.k8s_rows = d_k8s_rows;
    if (strings) { A.srows = strings->d_rows.as<const IxStrRow>(); A.sblob = strings->d_blob.as<const uint8_t>(); A.n_srows = (uint32_t)strings->rows.size(); }
    A.state = w->state.as<nfagg_flp_ipfix_elements>();
    A.names = h->enc.names.as<const nfagg_intf_name>(); A.n_names = opt->n_names;
    memcpy(A.unknown_w, opt->unknown_name, 16); A.unknown_len = opt->unknown_len;
    split_now(opt->now_unix_ns, A.now_sec, A.now_nsec);
    A.mono_now = opt->mono_now_ns;
    A.export_time = opt->export_time_s; A.seq0 = opt->seq0; A.obs_domain = opt->obs_domain_id;
    A.tid_v4 = opt->template_id_v4; A.tid_v6 = opt->template_id_v6; A.enterprise = opt->enterprise_id; A.max_msg = opt->max_msg_size;
    A.flags_mask = opt->flags_decoded ? 0x7ffu : 0xffffu;          // EncodeTCPFlags(DecodeTCPFlags(x)): the eleven known bits
    A.meta = w->meta.as<uint32_t>(); A.src = w->src.as<int32_t>(); A.agg = w->agg.as<int32_t>(); A.pre = w->pre.as<int32_t>();
    A.rows = w->rows.as<uint32_t>();
    A.seq_local = w->seq_local.as<uint32_t>(); A.seq_sum = w->seq_sum.as<uint32_t>(); A.seq_base = w->seq_base.as<uint64_t>();
    // the one read-back: the bytes, and the sent flows in the same synchronisation. Too small a buffer ends the call before the
    // write pass, which alone touches the state.
    uint64_t sent = 0;
    rc = encode_two_pass(h, n, {"write ipfix", "plan", "write"}, d_out, out_cap, out_bytes, {A.seq_base + blocks, &sent, sizeof sent},
        [&](uint32_t* local_off, uint32_t* block_sum, uint64_t* block_base) {
            A.local_off = local_off; A.block_sum = block_sum; A.block_base = block_base;
            return launch_ipfix_flp_plan(A, h->stream); },
        [&](const uint32_t*, const uint64_t*, uint64_t) { return launch_ipfix_flp_write(A, (uint8_t*)d_out, d_msg_offsets, d_status, h->stream); });
    *n_sent = (size_t)sent;
    return rc;
}

int nfagg_flp_ipfix_write(nfagg_handle* h, nfagg_flp_ipfix_writer* w, const void* records, size_t n, const nfagg_pb_features* features,
                          const uint32_t* k8s_rows, const nfagg_flp_ipfix_strings* strings, const nfagg_flp_ipfix_options* opt, void* out,
                          size_t out_cap, uint64_t* msg_offsets, uint8_t* status, size_t* n_sent, size_t* out_bytes) {
    int rc = check_options(h, opt);
    if (rc != NFAGG_OK) return rc;
    if (!h || !w || !out_bytes || !n_sent || !msg_offsets || (n && (!records || !status))) return fail(h, NFAGG_EINVAL, "null argument");
    if (w->h != h) return fail(h, NFAGG_EINVAL, "the writer was not created for this handle");
    if (features && features->struct_size != sizeof(nfagg_pb_features)) return fail(h, NFAGG_EINVAL, "nfagg_pb_features.struct_size mismatch");
    return encode_staged(h, records, n, out, out_cap, msg_offsets, out_bytes, {{status, 1}},
        [&](const void* d_records, void* d_out, uint64_t* d_offsets) {
            if (k8s_rows) API_TRY(stage_in(h, h->enc.k8s_rows, k8s_rows, n * 8));
            nfagg_pb_features dfeat{};
            if (features && n) API_TRY(stage_pb_features(h, features, n, &dfeat));
            return nfagg_flp_ipfix_write_device(h, w, d_records, n, (features && n) ? &dfeat : nullptr, k8s_rows ? h->enc.k8s_rows.as<const uint32_t>() : nullptr,
                                                strings, opt, d_out, out_cap, d_offsets, h->enc.out_extra[0].as<uint8_t>(), n_sent, out_bytes); });
}

}  // extern "C"
