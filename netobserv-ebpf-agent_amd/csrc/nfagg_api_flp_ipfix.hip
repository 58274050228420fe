// nfagg_api_flp_ipfix.hip — the host side of write ipfix on the device (include/nfagg.h, "write ipfix on the device";
// nfagg_flp_ipfix.h): the template message, the strings table, the writer (the element state of both families and the call's
// scratch), nfagg_flp_ipfix_write[_device]. A write costs the upload of the namer table, the launches of nfagg_flp_ipfix.hip and one
// 16-byte read-back (bytes and sent flows) between the size pass and the write pass.
#include <hip/hip_runtime.h>
#include <string.h>
#include <algorithm>
#include <new>
#include <vector>

#include "../../include/nfagg.h"
#include "nfagg_internal.h"
#include "nfagg_handle.h"
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
    DevBuf names, meta, src, agg, pre, rows, local_off, block_sum, block_base, seq_local, seq_sum, seq_base;
    DevBuf in_records, in_rows, out, out_offsets, out_status;          // the host entry point's staging
    std::vector<nfagg_intf_name> h_names;                              // kept until the stream has consumed it
};

namespace {

// prepareTemplate's element lists: (element id, length), registry/registry_IANA.go; write_ipfix.go:60-108
const uint16_t kLeadV4[6][2] = {{8, 4}, {12, 4}, {176, 1}, {177, 1}, {225, 4}, {226, 4}};
const uint16_t kLeadV6[7][2] = {{27, 16}, {28, 16}, {193, 1}, {178, 1}, {179, 1}, {281, 16}, {282, 16}};
const uint16_t kCommon[17][2] = {{256, 2}, {61, 1}, {56, 6}, {80, 6}, {4, 1}, {7, 2}, {11, 2}, {1, 8}, {152, 8}, {153, 8}, {2, 8},
                                 {82, 65535}, {6, 2}, {227, 2}, {228, 2}, {304, 2}, {311, 8}};
const uint16_t kEnterprise[9][2] = {{7733, 65535}, {7734, 65535}, {7735, 65535}, {7736, 65535}, {7737, 65535}, {7738, 65535},
                                    {7740, 8}, {7741, 65535}, {7742, 65535}};

void be16(uint8_t* p, uint32_t v) { p[0] = (uint8_t)(v >> 8); p[1] = (uint8_t)v; }
void be32(uint8_t* p, uint32_t v) { be16(p, v >> 16); be16(p + 2, v); }

int check_options(nfagg_handle* h, const nfagg_flp_ipfix_options* opt) {
    if (!opt) return fail(h, NFAGG_EINVAL, "null options");
    if (opt->struct_size != sizeof(nfagg_flp_ipfix_options)) return fail(h, NFAGG_EINVAL, "nfagg_flp_ipfix_options.struct_size mismatch");
    if (opt->max_msg_size > 65535u) return fail(h, NFAGG_EINVAL, "max_msg_size %u, more than 65535", opt->max_msg_size);
    if (opt->unknown_len > 16 || (opt->n_names && !opt->names)) return fail(h, NFAGG_EINVAL, "bad namer table");
    for (uint32_t k = 0; k < opt->n_names; k++)
        if (opt->names[k].name_len > 16) return fail(h, NFAGG_EINVAL, "namer row %u: name too long", k);
    return NFAGG_OK;
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
    const uint32_t n_lead = v6 ? 7 : 6, n_ent = opt->enterprise_id ? 9 : 0;
    const size_t total = 16 + 4 + 4 + 4 * (n_lead + 17) + 8 * n_ent;
    *n_out = total;
    if (!out || cap < total) return NFAGG_TRUNCATED;
    uint8_t* p = (uint8_t*)out;
    be16(p, 10); be16(p + 2, (uint32_t)total); be32(p + 4, opt->export_time_s); be32(p + 8, opt->seq0); be32(p + 12, opt->obs_domain_id);
    be16(p + 16, 2); be16(p + 18, (uint32_t)total - 16);                                       // template set
    be16(p + 20, v6 ? opt->template_id_v6 : opt->template_id_v4); be16(p + 22, n_lead + 17 + n_ent);
    uint8_t* q = p + 24;
    const uint16_t (*lead)[2] = v6 ? kLeadV6 : kLeadV4;
    for (uint32_t k = 0; k < n_lead; k++, q += 4) { be16(q, lead[k][0]); be16(q + 2, lead[k][1]); }
    for (uint32_t k = 0; k < 17; k++, q += 4) { be16(q, kCommon[k][0]); be16(q + 2, kCommon[k][1]); }
    for (uint32_t k = 0; k < n_ent; k++, q += 8) {                                             // entities/record.go:252-265
        be16(q, kEnterprise[k][0] | 0x8000u); be16(q + 2, kEnterprise[k][1]); be32(q + 4, opt->enterprise_id);
    }
    return NFAGG_OK;
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
    *out_bytes = 0; *n_sent = 0;
    HIP_TRY(h, hipSetDevice(h->device));
    if (!n) { HIP_TRY(h, hipMemsetAsync(d_msg_offsets, 0, sizeof(uint64_t), h->stream)); HIP_TRY(h, hipStreamSynchronize(h->stream)); return NFAGG_OK; }
    const size_t blocks = (n + 1023) / 1024, stride = blocks + 1;
    struct { DevBuf* b; size_t bytes; } need[] = {
        {&w->names, (size_t)(opt->n_names + 1) * sizeof(nfagg_intf_name)}, {&w->meta, n * 4}, {&w->src, n * kIxGroups * 4},
        {&w->agg, 2 * kIxAggs * stride * 4}, {&w->pre, 2 * kIxAggs * stride * 4}, {&w->rows, n * 32}, {&w->local_off, n * 4},
        {&w->block_sum, blocks * 4}, {&w->block_base, (blocks + 1) * 8}, {&w->seq_local, n * 4}, {&w->seq_sum, blocks * 4},
        {&w->seq_base, (blocks + 1) * 8}};
    for (auto& q : need) if ((rc = q.b->ensure(h, q.bytes)) != NFAGG_OK) return rc;
    // the kernels binary-search the namer table: a stable sort by if_index keeps the scan-in-table-order answer
    w->h_names.assign(opt->names, opt->names + opt->n_names);
    std::stable_sort(w->h_names.begin(), w->h_names.end(), [](const nfagg_intf_name& a, const nfagg_intf_name& b) { return a.if_index < b.if_index; });
    if (opt->n_names) HIP_TRY(h, hipMemcpyAsync(w->names.p, w->h_names.data(), opt->n_names * sizeof(nfagg_intf_name), hipMemcpyHostToDevice, h->stream));
    IxArgs A{};
    A.recs = d_records; A.n = n; A.F = F;
    A.k8s_rows = d_k8s_rows;
    if (strings) { A.srows = strings->d_rows.as<const IxStrRow>(); A.sblob = strings->d_blob.as<const uint8_t>(); A.n_srows = (uint32_t)strings->rows.size(); }
    A.state = w->state.as<nfagg_flp_ipfix_elements>();
    A.names = w->names.as<const nfagg_intf_name>(); A.n_names = opt->n_names;
    memcpy(A.unknown_w, opt->unknown_name, 16); A.unknown_len = opt->unknown_len;
    A.now_sec = opt->now_unix_ns / 1000000000ll; A.now_nsec = opt->now_unix_ns % 1000000000ll;       // time.Time's (sec, nsec), 0 <= nsec < 1e9
    if (A.now_nsec < 0) { A.now_nsec += 1000000000ll; A.now_sec -= 1; }
    A.mono_now = opt->mono_now_ns;
    A.export_time = opt->export_time_s; A.seq0 = opt->seq0; A.obs_domain = opt->obs_domain_id;
    A.tid_v4 = opt->template_id_v4; A.tid_v6 = opt->template_id_v6; A.enterprise = opt->enterprise_id; A.max_msg = opt->max_msg_size;
    A.flags_mask = opt->flags_decoded ? 0x7ffu : 0xffffu;          // EncodeTCPFlags(DecodeTCPFlags(x)): the eleven known bits
    A.meta = w->meta.as<uint32_t>(); A.src = w->src.as<int32_t>(); A.agg = w->agg.as<int32_t>(); A.pre = w->pre.as<int32_t>();
    A.rows = w->rows.as<uint32_t>();
    A.local_off = w->local_off.as<uint32_t>(); A.block_sum = w->block_sum.as<uint32_t>(); A.block_base = w->block_base.as<uint64_t>();
    A.seq_local = w->seq_local.as<uint32_t>(); A.seq_sum = w->seq_sum.as<uint32_t>(); A.seq_base = w->seq_base.as<uint64_t>();
    hipError_t e = launch_ipfix_flp_plan(A, h->stream);
    if (e != hipSuccess) return fail(h, NFAGG_EDEVICE, "write ipfix plan launch failed: %s", hipGetErrorString(e));
    uint64_t total = 0, sent = 0;
    HIP_TRY(h, hipMemcpyAsync(&total, A.block_base + blocks, sizeof total, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipMemcpyAsync(&sent, A.seq_base + blocks, sizeof sent, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    *out_bytes = (size_t)total; *n_sent = (size_t)sent;
    if (total > out_cap || !d_out) return NFAGG_TRUNCATED;         // the state has not been touched
    e = launch_ipfix_flp_write(A, (uint8_t*)d_out, d_msg_offsets, d_status, h->stream);
    if (e != hipSuccess) return fail(h, NFAGG_EDEVICE, "write ipfix write launch failed: %s", hipGetErrorString(e));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return NFAGG_OK;
}

int nfagg_flp_ipfix_write(nfagg_handle* h, nfagg_flp_ipfix_writer* w, const void* records, size_t n, const nfagg_pb_features* features,
                          const uint32_t* k8s_rows, const nfagg_flp_ipfix_strings* strings, const nfagg_flp_ipfix_options* opt, void* out,
                          size_t out_cap, uint64_t* msg_offsets, uint8_t* status, size_t* n_sent, size_t* out_bytes) {
    int rc = check_options(h, opt);
    if (rc != NFAGG_OK) return rc;
    if (!h || !w || !out_bytes || !n_sent || !msg_offsets || (n && (!records || !status))) return fail(h, NFAGG_EINVAL, "null argument");
    if (w->h != h) return fail(h, NFAGG_EINVAL, "the writer was not created for this handle");
    if (features && features->struct_size != sizeof(nfagg_pb_features)) return fail(h, NFAGG_EINVAL, "nfagg_pb_features.struct_size mismatch");
    HIP_TRY(h, hipSetDevice(h->device));
    struct { DevBuf* b; size_t bytes; } need[] = {{&w->in_records, n * kRecordBytes + 16}, {&w->in_rows, n * 8 + 16}, {&w->out, out_cap + 32},
                                                  {&w->out_offsets, (n + 1) * 8}, {&w->out_status, n + 16}};
    for (auto& q : need) if ((rc = q.b->ensure(h, q.bytes)) != NFAGG_OK) return rc;
    if (n) HIP_TRY(h, hipMemcpyAsync(w->in_records.p, records, n * kRecordBytes, hipMemcpyHostToDevice, h->stream));
    if (n && k8s_rows) HIP_TRY(h, hipMemcpyAsync(w->in_rows.p, k8s_rows, n * 8, hipMemcpyHostToDevice, h->stream));
    nfagg_pb_features dfeat{};
    if (features && n && (rc = stage_pb_features(h, features, n, &dfeat)) != NFAGG_OK) return rc;
    rc = nfagg_flp_ipfix_write_device(h, w, w->in_records.p, n, (features && n) ? &dfeat : nullptr, k8s_rows ? w->in_rows.as<const uint32_t>() : nullptr,
                                      strings, opt, out ? w->out.p : nullptr, out_cap, w->out_offsets.as<uint64_t>(), w->out_status.as<uint8_t>(),
                                      n_sent, out_bytes);
    if (rc != NFAGG_OK) return rc;                                  // truncated: out, msg_offsets and status are not written
    if (*out_bytes) HIP_TRY(h, hipMemcpyAsync(out, w->out.p, *out_bytes, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipMemcpyAsync(msg_offsets, w->out_offsets.p, (n + 1) * 8, hipMemcpyDeviceToHost, h->stream));
    if (n) HIP_TRY(h, hipMemcpyAsync(status, w->out_status.p, n, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return NFAGG_OK;
}

}  // extern "C"
