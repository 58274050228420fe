// nfagg_api_export.hip — the export encoders' host side of the C ABI (include/nfagg.h): evicted records to protobuf, IPFIX and
// direct-FLP JSON, from device memory or staged from the host. The tables the *_netev, *_tls, *_k8s and *_net entry points take
// are nfagg_api_tables.hip's.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>

#include "../../include/nfagg.h"
#include "nfagg_internal.h"
#include "nfagg_handle.h"
#include "nfagg_api_call.h"
#include "nfagg_api_tables.h"
#include "nfagg_pb.h"
#include "nfagg_ipfix.h"
#include "nfagg_flp.h"

using namespace nfagg;

extern "C" {

// nfagg_pb_features with DEVICE pointers, checked, as the kernels take it (protobuf and direct-FLP content encoders)
int device_features(nfagg_handle* h, const nfagg_pb_features* feat, PbFeat* F) {
    if (feat->struct_size != sizeof(nfagg_pb_features)) return fail(h, NFAGG_EINVAL, "nfagg_pb_features.struct_size mismatch");
    if ((((uintptr_t)feat->additional | (uintptr_t)feat->dns | (uintptr_t)feat->drops | (uintptr_t)feat->xlat | (uintptr_t)feat->quic) & 7u) != 0)
        return fail(h, NFAGG_EINVAL, "feature arrays must be 8-byte aligned");
    F->present = feat->present;
    F->additional = (const uint8_t*)feat->additional; F->dns = (const uint8_t*)feat->dns; F->drops = (const uint8_t*)feat->drops;
    F->xlat = (const uint8_t*)feat->xlat; F->quic = (const uint8_t*)feat->quic;
    return NFAGG_OK;
}

// The *_netev entry points' extra inputs: the flows' rows (DEVICE memory) and the table they index, checked, into F.
int device_netev(nfagg_handle* h, const NetevArgs* ne, size_t n, PbFeat* F) {
    if (!ne->table || (n && !ne->rows)) return fail(h, NFAGG_EINVAL, "null network-events rows or table");
    if (ne->table->h != h || !ne->table->d_rows) return fail(h, NFAGG_EINVAL, "the network-events table was not created for this handle");
    if (((uintptr_t)ne->rows & 7u) != 0) return fail(h, NFAGG_EINVAL, "network-events rows must be 8-byte aligned");
    F->ne_rows = ne->rows; F->ne_tab = ne->table->d_rows.as<const uint8_t>(); F->ne_blob = ne->table->d_blob.as<const uint8_t>();
    F->ne_n = (uint32_t)ne->table->rows.size();
    return NFAGG_OK;
}
// The rows of a host-memory call, uploaded.
static int stage_netev_rows(nfagg_handle* h, const NetevArgs* ne, size_t n, NetevArgs* dne) {
    *dne = *ne;
    if (!n || !ne->rows) return NFAGG_OK;
    API_TRY(stage_in(h, h->enc.ne_rows, ne->rows, n * 8));
    dne->rows = h->enc.ne_rows.as<const uint16_t>();
    return NFAGG_OK;
}

// ---- record -> protobuf (nfagg_pb.hip)
// feat (optional): DEVICE pointers. ne (optional): the network events of the *_netev entry points.
static int encode_pb_device_core(nfagg_handle* h, const void* d_records, size_t n, const nfagg_pb_features* feat, const NetevArgs* ne,
                                 const nfagg_pb_options* opt,
                                 void* d_out, size_t out_cap, uint64_t* d_frame_offsets, uint32_t* d_body_len,
                                 void* d_kafka_keys, size_t* out_bytes) {
    if (!h || !opt || !out_bytes || !d_frame_offsets || (n && (!d_records || !d_body_len))) return fail(h, NFAGG_EINVAL, "null argument");
    if (opt->struct_size != sizeof(nfagg_pb_options)) return fail(h, NFAGG_EINVAL, "nfagg_pb_options.struct_size mismatch");
    if (opt->unknown_len > 16 || (opt->n_names && !opt->names)) return fail(h, NFAGG_EINVAL, "bad namer table");   // ahead of the alignment, the rows behind it
    if ((((uintptr_t)d_records | (uintptr_t)d_out | (uintptr_t)d_kafka_keys) & 15u) != 0) return fail(h, NFAGG_EINVAL, "device buffers must be 16-byte aligned");
    int rc = check_namer(h, opt->names, opt->n_names, opt->unknown_len, true);
    if (rc != NFAGG_OK) return rc;
    PbFeat F{};
    if (feat && (rc = device_features(h, feat, &F)) != NFAGG_OK) return rc;
    if (ne && (rc = device_netev(h, ne, n, &F)) != NFAGG_OK) return rc;
    bool done;
    if ((rc = encode_begin(h, n, d_frame_offsets, out_bytes, opt->names, opt->n_names, &done)) != NFAGG_OK || done) return rc;
    PbParams P{};
    split_now(opt->now_unix_ns, P.now_sec, P.now_nsec);
    P.mono_now = opt->mono_now_ns;
    memcpy(P.agent_ip_w, opt->agent_ip, 16);
    static const uint8_t v4pre[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0xff, 0xff};
    P.agent_is_v4 = memcmp(opt->agent_ip, v4pre, 12) == 0;     // net.IP.To4() != nil (proto.go:255-261)
    P.names = h->enc.names.as<const nfagg_intf_name>(); P.n_names = opt->n_names;
    P.unknown_len = opt->unknown_len; memcpy(P.unknown, opt->unknown_name, 16);
    return encode_two_pass(h, n, {"protobuf", "size", "encode"}, d_out, out_cap, out_bytes, {},
        [&](uint32_t* local_off, uint32_t* block_sum, uint64_t* block_base) {
            return launch_pb_size(d_records, n, P, F, d_body_len, local_off, block_sum, block_base, h->stream); },
        [&](const uint32_t* local_off, const uint64_t* block_base, uint64_t total) {
            return launch_pb_write(d_records, n, P, F, d_body_len, local_off, block_base, d_out, d_frame_offsets, d_kafka_keys, total, h->stream); });
}

// The feature parts of a host-memory call, uploaded: *dfeat gets the device pointers.
int stage_pb_features(nfagg_handle* h, const nfagg_pb_features* feat, size_t n, nfagg_pb_features* dfeat) {
    dfeat->struct_size = sizeof *dfeat;
    const void* src[6] = {feat->present, feat->additional, feat->dns, feat->drops, feat->xlat, feat->quic};
    const size_t elem[6] = {1, sizeof(nfagg_additional_metrics), sizeof(nfagg_dns_metrics), sizeof(nfagg_pkt_drop_metrics),
                            sizeof(nfagg_xlat_metrics), sizeof(nfagg_quic_metrics)};
    void* dst[6] = {};
    for (int k = 0; k < 6; k++) {
        if (!src[k]) continue;
        API_TRY(stage_in(h, h->enc.pb_feat[k], src[k], n * elem[k]));
        dst[k] = h->enc.pb_feat[k].p;
    }
    dfeat->present = (const uint8_t*)dst[0]; dfeat->additional = (const nfagg_additional_metrics*)dst[1];
    dfeat->dns = (const nfagg_dns_metrics*)dst[2]; dfeat->drops = (const nfagg_pkt_drop_metrics*)dst[3];
    dfeat->xlat = (const nfagg_xlat_metrics*)dst[4]; dfeat->quic = (const nfagg_quic_metrics*)dst[5];
    return NFAGG_OK;
}

// feat (optional): HOST pointers
static int encode_pb_host_core(nfagg_handle* h, const void* records, size_t n, const nfagg_pb_features* feat, const NetevArgs* ne,
                               const nfagg_pb_options* opt,
                               void* out, size_t out_cap, uint64_t* frame_offsets, uint32_t* body_len,
                               void* kafka_keys, size_t* out_bytes) {
    if (!h || !opt || !out_bytes || !frame_offsets || (n && (!records || !body_len))) return fail(h, NFAGG_EINVAL, "null argument");
    if (feat && feat->struct_size != sizeof(nfagg_pb_features)) return fail(h, NFAGG_EINVAL, "nfagg_pb_features.struct_size mismatch");
    return encode_staged(h, records, n, out, out_cap, frame_offsets, out_bytes, {{body_len, sizeof(uint32_t)}, {kafka_keys, 32}},
        [&](const void* d_records, void* d_out, uint64_t* d_offsets) {
            nfagg_pb_features dfeat{};
            if (feat && n) API_TRY(stage_pb_features(h, feat, n, &dfeat));
            NetevArgs dne{};
            if (ne) API_TRY(stage_netev_rows(h, ne, n, &dne));
            return encode_pb_device_core(h, d_records, n, (feat && n) ? &dfeat : nullptr, ne ? &dne : nullptr, opt, d_out, out_cap, d_offsets,
                                         h->enc.out_extra[0].as<uint32_t>(), kafka_keys ? h->enc.out_extra[1].p : nullptr, out_bytes); });
}

int nfagg_encode_pb_device(nfagg_handle* h, const void* d_records, size_t n, const nfagg_pb_options* opt,
                           void* d_out, size_t out_cap, uint64_t* d_frame_offsets, uint32_t* d_body_len,
                           void* d_kafka_keys, size_t* out_bytes) {
    return encode_pb_device_core(h, d_records, n, nullptr, nullptr, opt, d_out, out_cap, d_frame_offsets, d_body_len, d_kafka_keys, out_bytes);
}

int nfagg_encode_pb(nfagg_handle* h, const void* records, size_t n, const nfagg_pb_options* opt,
                    void* out, size_t out_cap, uint64_t* frame_offsets, uint32_t* body_len,
                    void* kafka_keys, size_t* out_bytes) {
    return encode_pb_host_core(h, records, n, nullptr, nullptr, opt, out, out_cap, frame_offsets, body_len, kafka_keys, out_bytes);
}

int nfagg_encode_pb_content_device(nfagg_handle* h, const void* d_records, size_t n, const nfagg_pb_features* d_features,
                                   const nfagg_pb_options* opt, void* d_out, size_t out_cap, uint64_t* d_frame_offsets,
                                   uint32_t* d_body_len, void* d_kafka_keys, size_t* out_bytes) {
    if (!d_features) return fail(h, NFAGG_EINVAL, "null features (use nfagg_encode_pb_device)");
    return encode_pb_device_core(h, d_records, n, d_features, nullptr, opt, d_out, out_cap, d_frame_offsets, d_body_len, d_kafka_keys, out_bytes);
}

int nfagg_encode_pb_content(nfagg_handle* h, const void* records, size_t n, const nfagg_pb_features* features,
                            const nfagg_pb_options* opt, void* out, size_t out_cap, uint64_t* frame_offsets,
                            uint32_t* body_len, void* kafka_keys, size_t* out_bytes) {
    if (!features) return fail(h, NFAGG_EINVAL, "null features (use nfagg_encode_pb)");
    return encode_pb_host_core(h, records, n, features, nullptr, opt, out, out_cap, frame_offsets, body_len, kafka_keys, out_bytes);
}

int nfagg_encode_pb_content_netev_device(nfagg_handle* h, const void* d_records, size_t n, const nfagg_pb_features* d_features,
                                         const uint16_t* d_rows, const nfagg_netev_table* table,
                                         const nfagg_pb_options* opt, void* d_out, size_t out_cap, uint64_t* d_frame_offsets,
                                         uint32_t* d_body_len, void* d_kafka_keys, size_t* out_bytes) {
    const NetevArgs ne{d_rows, table};
    return encode_pb_device_core(h, d_records, n, d_features, &ne, opt, d_out, out_cap, d_frame_offsets, d_body_len, d_kafka_keys, out_bytes);
}

int nfagg_encode_pb_content_netev(nfagg_handle* h, const void* records, size_t n, const nfagg_pb_features* features,
                                  const uint16_t* rows, const nfagg_netev_table* table,
                                  const nfagg_pb_options* opt, void* out, size_t out_cap, uint64_t* frame_offsets,
                                  uint32_t* body_len, void* kafka_keys, size_t* out_bytes) {
    const NetevArgs ne{rows, table};
    return encode_pb_host_core(h, records, n, features, &ne, opt, out, out_cap, frame_offsets, body_len, kafka_keys, out_bytes);
}

// ---- record -> IPFIX (nfagg_ipfix.hip)
static const uint16_t kIpfixTemplateV4[19][2] = {   // ipfix.go:89-135 + AddRecordValuesToTemplate; IDs and lengths: registry_IANA.go
    {256, 2}, {61, 1}, {56, 6}, {80, 6}, {8, 4}, {12, 4}, {4, 1}, {7, 2}, {11, 2}, {176, 1}, {177, 1},
    {1, 8}, {6, 2}, {150, 4}, {152, 8}, {151, 4}, {153, 8}, {2, 8}, {82, 65535}};
static const uint16_t kIpfixTemplateV6[19][2] = {   // ipfix.go:158-204 + AddRecordValuesToTemplate
    {256, 2}, {61, 1}, {56, 6}, {80, 6}, {27, 16}, {28, 16}, {193, 1}, {7, 2}, {11, 2}, {178, 1}, {179, 1},
    {1, 8}, {6, 2}, {150, 4}, {152, 8}, {151, 4}, {153, 8}, {2, 8}, {82, 65535}};

int nfagg_ipfix_template(const nfagg_ipfix_options* opt, int v6, void* out, size_t cap, size_t* n_out) {
    if (!opt || !n_out) return fail(nullptr, NFAGG_EINVAL, "null argument");
    if (opt->struct_size != sizeof(nfagg_ipfix_options)) return fail(nullptr, NFAGG_EINVAL, "nfagg_ipfix_options.struct_size mismatch");
    return ipfix_template_message({opt->export_time_s, opt->seq0, opt->obs_domain_id, v6 ? opt->template_id_v6 : opt->template_id_v4},
                                  {{v6 ? kIpfixTemplateV6 : kIpfixTemplateV4, 19}}, {}, 0, out, cap, n_out);      // enterprise bit never set
}

// The options are checked first, before the handle: a caller learns of a bad table without any device work.
static int encode_ipfix_check(nfagg_handle* h, const nfagg_ipfix_options* opt) {
    if (!opt) return fail(h, NFAGG_EINVAL, "null options");
    if (opt->struct_size != sizeof(nfagg_ipfix_options)) return fail(h, NFAGG_EINVAL, "nfagg_ipfix_options.struct_size mismatch");
    return check_namer(h, opt->names, opt->n_names, opt->unknown_len, false);
}

int nfagg_encode_ipfix_device(nfagg_handle* h, const void* d_records, size_t n, const nfagg_ipfix_options* opt,
                              void* d_out, size_t out_cap, uint64_t* d_msg_offsets, size_t* out_bytes) {
    int rc = encode_ipfix_check(h, opt);
    if (rc != NFAGG_OK) return rc;
    if (!h || !out_bytes || !d_msg_offsets || (n && !d_records)) return fail(h, NFAGG_EINVAL, "null argument");
    if ((((uintptr_t)d_records | (uintptr_t)d_out) & 15u) != 0) return fail(h, NFAGG_EINVAL, "device buffers must be 16-byte aligned");
    bool done;
    if ((rc = encode_begin(h, n, d_msg_offsets, out_bytes, opt->names, opt->n_names, &done)) != NFAGG_OK || done) return rc;
    if ((rc = h->enc.ipfix_name_rows.ensure(h, n * sizeof(uint32_t))) != NFAGG_OK) return rc;
    uint32_t* name_rows = h->enc.ipfix_name_rows.as<uint32_t>();
    IpfixParams P{};
    split_now(opt->now_unix_ns, P.now_sec, P.now_nsec);
    P.mono_now = opt->mono_now_ns;
    P.names = h->enc.names.as<const nfagg_intf_name>(); P.n_names = opt->n_names;
    P.unknown_len = opt->unknown_len; memcpy(P.unknown_w, opt->unknown_name, 16);
    P.export_time = opt->export_time_s; P.seq0 = opt->seq0; P.obs_domain = opt->obs_domain_id;
    P.tid_v4 = opt->template_id_v4; P.tid_v6 = opt->template_id_v6;
    return encode_two_pass(h, n, {"IPFIX", "size", "write"}, d_out, out_cap, out_bytes, {},
        [&](uint32_t* local_off, uint32_t* block_sum, uint64_t* block_base) {
            return launch_ipfix_size(d_records, n, P, name_rows, local_off, block_sum, block_base, h->stream); },
        [&](const uint32_t* local_off, const uint64_t* block_base, uint64_t) {
            return launch_ipfix_write(d_records, n, P, name_rows, local_off, block_base, d_out, d_msg_offsets, h->stream); });
}

int nfagg_encode_ipfix(nfagg_handle* h, const void* records, size_t n, const nfagg_ipfix_options* opt,
                       void* out, size_t out_cap, uint64_t* msg_offsets, size_t* out_bytes) {
    int rc = encode_ipfix_check(h, opt);
    if (rc != NFAGG_OK) return rc;
    if (!h || !out_bytes || !msg_offsets || (n && !records)) return fail(h, NFAGG_EINVAL, "null argument");
    return encode_staged(h, records, n, out, out_cap, msg_offsets, out_bytes, {},
        [&](const void* d_records, void* d_out, uint64_t* d_offsets) {
            return nfagg_encode_ipfix_device(h, d_records, n, opt, d_out, out_cap, d_offsets, out_bytes); });
}

// ---- record -> direct-FLP JSON lines (nfagg_flp.hip), and what write loki's plan (nfagg_api_loki.hip) sets up in the same way
// The options are checked first, before the handle: a caller learns of a bad table without any device work.
int check_flp_options(nfagg_handle* h, const nfagg_flp_options* opt) {
    if (!opt) return fail(h, NFAGG_EINVAL, "null options");
    if (opt->struct_size != sizeof(nfagg_flp_options)) return fail(h, NFAGG_EINVAL, "nfagg_flp_options.struct_size mismatch");
    return check_namer(h, opt->names, opt->n_names, opt->unknown_len, true);
}

int check_flp_tables(nfagg_handle* h, const FlpLineTables& t) {
    if (t.level >= FlpLevel::Tls && (t.tls->h != h || !t.tls->d_mem)) return fail(h, NFAGG_EINVAL, "the TLS name table was not created for this handle");
    if (t.level >= FlpLevel::K8s && (t.k8s->h != h || !t.k8s->d_slots)) return fail(h, NFAGG_EINVAL, "the Kubernetes table was not created for this handle");
    if (t.level >= FlpLevel::Net && (t.net->h != h || !t.net->d_mem)) return fail(h, NFAGG_EINVAL, "the net table was not created for this handle");
    return NFAGG_OK;
}

int netev_together(nfagg_handle* h, const NetevArgs& ne, size_t n) {
    if ((ne.rows != nullptr) != (ne.table != nullptr) && (n || ne.rows)) return fail(h, NFAGG_EINVAL, "network-events rows and table go together");
    return NFAGG_OK;
}

static void flp_escape_row(uint8_t* row, const char* name, uint32_t name_len, const char* udn, uint32_t udn_len) {
    const uint16_t nl = (uint16_t)flp_escape(name, name_len, row + kFlpEscNameOff), ul = (uint16_t)flp_escape(udn, udn_len, row + kFlpEscUdnOff);
    memcpy(row, &nl, 2); memcpy(row + 2, &ul, 2);
}

int stage_flp_line(nfagg_handle* h, const void* d_records, size_t n, const nfagg_flp_options* opt, const PbFeat& F, const FlpLineTables& t,
                          const FlpLineStage& st, FlpLineArgs* args) {
    const size_t esc_bytes = (size_t)(opt->n_names + 1) * kFlpEscRowBytes;
    API_TRY(stage_namer(h, opt->names, opt->n_names, st.names, st.h_names));
    API_TRY(st.esc.ensure(h, esc_bytes));
    // names and UDNs are escaped here, once per row of the sorted table: no kernel escapes per flow
    st.h_esc.assign(esc_bytes, 0);
    flp_escape_row(st.h_esc.data(), opt->unknown_name, opt->unknown_len, "", 0);
    for (uint32_t k = 0; k < opt->n_names; k++) {
        const nfagg_intf_name& e = st.h_names[k];
        flp_escape_row(st.h_esc.data() + (size_t)(k + 1) * kFlpEscRowBytes, e.name, e.name_len, e.udn, e.udn_len);
    }
    HIP_TRY(h, hipMemcpyAsync(st.esc.p, st.h_esc.data(), esc_bytes, hipMemcpyHostToDevice, h->stream));
    FlpLineArgs& A = *args;
    A = FlpLineArgs{};
    A.recs = d_records; A.n = n; A.F = F; A.hash_ids = t.hash_ids;
    split_now(opt->now_unix_ns, A.P.now_sec, A.P.now_nsec);
    A.P.mono_now = opt->mono_now_ns;
    A.P.time_received = opt->time_received_s;
    A.P.names = st.names.as<const nfagg_intf_name>(); A.P.esc = st.esc.as<const uint8_t>(); A.P.n_names = opt->n_names;
    A.P.agent_nil = opt->agent_ip_nil ? 1u : 0u; memcpy(A.P.agent_ip_w, opt->agent_ip, 16);
    if (t.level >= FlpLevel::Tls) {
        A.T.ids = t.tls->d_mem.as<const uint16_t>();
        A.T.rows = t.tls->d_mem.as<const uint8_t>() + t.tls->ids.size() * sizeof(uint16_t);
        for (uint32_t k = 0; k < kTlsKinds; k++) A.T.n[k] = t.tls->n[k];
    }
    if (t.level >= FlpLevel::K8s) {
        API_TRY(st.k8s_rows.ensure(h, n * 2 * sizeof(uint32_t)));
        A.K = k8s_dev(t.k8s); A.k8s_rows = st.k8s_rows.as<const uint32_t>();
        const hipError_t e = launch_k8s_resolve(d_records, n, A.K, st.k8s_rows.as<uint32_t>(), h->stream);
        if (e != hipSuccess) return fail(h, NFAGG_EDEVICE, "Kubernetes resolve launch failed: %s", hipGetErrorString(e));
    }
    if (t.level >= FlpLevel::Net) {
        API_TRY(st.net_rows.ensure(h, n * sizeof(uint2)));
        A.N = net_dev(t.net); A.net_rows = st.net_rows.as<const uint2>();
        const hipError_t e = launch_net_resolve(d_records, n, A.N, A.k8s_rows, t.k8s->d_host_ids.as<const uint32_t>(), A.K.n_rows, net_reporter(t.k8s, opt),
                                                st.net_rows.as<uint2>(), h->stream);
        if (e != hipSuccess) return fail(h, NFAGG_EDEVICE, "net resolve launch failed: %s", hipGetErrorString(e));
    }
    return NFAGG_OK;
}

// From *_tls up the network events are an option: rows and table both, or neither (*ne = nullptr).
static int netev_optional(nfagg_handle* h, const NetevArgs** ne, size_t n) {
    if (!*ne) return NFAGG_OK;
    const int rc = netev_together(h, **ne, n);
    if (rc == NFAGG_OK && !(*ne)->table) *ne = nullptr;
    return rc;
}

// t.level says which tables the entry point takes; one it takes is required. A pointer t has above its level is not looked at.
static bool flp_null_argument(const nfagg_handle* h, const FlpLineTables& t, const void* records, size_t n, const void* offsets, const size_t* out_bytes) {
    return !h || (t.level >= FlpLevel::Tls && !t.tls) || (t.level >= FlpLevel::K8s && !t.k8s) || (t.level >= FlpLevel::Net && !t.net) || !out_bytes ||
           !offsets || (n && !records) || (t.level == FlpLevel::Conn && n && !t.hash_ids);
}

// feat (optional): DEVICE pointers. The launchers pick the kernels' feature policy from the parts: neither feat nor ne the plain
// line, ne (the *_netev entry points, and from *_tls up) the one with the NetworkEvents hook; t.level puts the TLS names, the
// Kubernetes keys, the transform network keys and extract conntrack's keys on top (hash ids in DEVICE memory). From FlpLevel::Tls
// on no record is deferred: flags and counter are not used.
static int encode_flp_device_core(nfagg_handle* h, const void* d_records, size_t n, const nfagg_pb_features* feat, const NetevArgs* ne,
                                  const FlpLineTables& t, const nfagg_flp_options* opt,
                                  void* d_out, size_t out_cap, uint64_t* d_line_offsets, uint8_t* d_deferred,
                                  size_t* n_deferred, size_t* out_bytes) {
    const bool tls = t.level >= FlpLevel::Tls;
    int rc;
    if (tls && (rc = netev_optional(h, &ne, n)) != NFAGG_OK) return rc;
    if ((rc = check_flp_options(h, opt)) != NFAGG_OK) return rc;
    if (flp_null_argument(h, t, d_records, n, d_line_offsets, out_bytes)) return fail(h, NFAGG_EINVAL, "null argument");
    if (t.level == FlpLevel::Conn && ((uintptr_t)t.hash_ids & 7u) != 0) return fail(h, NFAGG_EINVAL, "hash ids must be 8-byte aligned");
    if ((rc = check_flp_tables(h, t)) != NFAGG_OK) return rc;
    if ((((uintptr_t)d_records | (uintptr_t)d_out) & 15u) != 0) return fail(h, NFAGG_EINVAL, "device buffers must be 16-byte aligned");
    PbFeat F{};
    if (feat && (rc = device_features(h, feat, &F)) != NFAGG_OK) return rc;
    if (ne && (rc = device_netev(h, ne, n, &F)) != NFAGG_OK) return rc;
    if (n_deferred) *n_deferred = 0;
    bool done;
    if ((rc = encode_begin(h, n, d_line_offsets, out_bytes, nullptr, 0, &done)) != NFAGG_OK || done) return rc;
    auto& S = h->enc;
    API_TRY(ensure_all(h, {{S.flp_rows, n * 8 * sizeof(uint32_t)}, {S.flp_n_deferred, 16}}));
    HIP_TRY(h, hipMemsetAsync(S.flp_n_deferred.p, 0, 16, h->stream));
    FlpLineArgs A;
    if ((rc = stage_flp_line(h, d_records, n, opt, F, t, FlpLineStage{S.names, S.flp_esc, S.k8s_rows, S.net_rows, S.h_names, S.h_flp_esc}, &A)) != NFAGG_OK) return rc;
    uint32_t* rows = S.flp_rows.as<uint32_t>();
    uint32_t* counter = S.flp_n_deferred.as<uint32_t>();
    static const char* const kWhat[5] = {"FLP JSON", "FLP JSON with TLS names", "FLP JSON with Kubernetes keys", "FLP JSON with transform network keys",
                                         "FLP JSON flow logs of extract conntrack"};
    const char* what = !tls && (feat || ne) ? "FLP JSON content" : kWhat[(int)t.level];
    uint32_t deferred = 0;
    rc = encode_two_pass(h, n, {what, "size", "write"}, d_out, out_cap, out_bytes, tls ? ReadBack{} : ReadBack{counter, &deferred, sizeof deferred},
        [&](uint32_t* local_off, uint32_t* block_sum, uint64_t* block_base) {
            return launch_flp_size(A, t.level, rows, local_off, block_sum, block_base, counter, h->stream); },
        [&](const uint32_t* local_off, const uint64_t* block_base, uint64_t) {
            return launch_flp_write(A, t.level, rows, local_off, block_base, d_out, d_line_offsets, d_deferred, h->stream); });
    if (!tls && n_deferred) *n_deferred = deferred;
    return rc;
}

// feat (optional): HOST pointers, uploaded beside the records, as are the rows of ne and the hash ids of FlpLevel::Conn
static int encode_flp_host_core(nfagg_handle* h, const void* records, size_t n, const nfagg_pb_features* feat, const NetevArgs* ne,
                                const FlpLineTables& t, const nfagg_flp_options* opt,
                                void* out, size_t out_cap, uint64_t* line_offsets, uint8_t* deferred,
                                size_t* n_deferred, size_t* out_bytes) {
    int rc = check_flp_options(h, opt);
    if (rc != NFAGG_OK) return rc;
    if (flp_null_argument(h, t, records, n, line_offsets, out_bytes)) return fail(h, NFAGG_EINVAL, "null argument");
    if (t.level >= FlpLevel::Tls && (rc = netev_optional(h, &ne, n)) != NFAGG_OK) return rc;
    if (feat && feat->struct_size != sizeof(nfagg_pb_features)) return fail(h, NFAGG_EINVAL, "nfagg_pb_features.struct_size mismatch");
    return encode_staged(h, records, n, out, out_cap, line_offsets, out_bytes, {{deferred, 1}},
        [&](const void* d_records, void* d_out, uint64_t* d_offsets) {
            nfagg_pb_features dfeat{};
            if (feat && n) API_TRY(stage_pb_features(h, feat, n, &dfeat));
            NetevArgs dne{};
            if (ne) API_TRY(stage_netev_rows(h, ne, n, &dne));
            FlpLineTables dt = t;
            if (t.level == FlpLevel::Conn) {                              // the hash ids, uploaded
                dt.hash_ids = nullptr;
                if (n) {
                    API_TRY(stage_in(h, h->enc.conn_ids, t.hash_ids, n * sizeof(uint64_t)));
                    dt.hash_ids = h->enc.conn_ids.as<const uint64_t>();
                }
            }
            return encode_flp_device_core(h, d_records, n, (feat && n) ? &dfeat : nullptr, ne ? &dne : nullptr, dt, opt, d_out, out_cap, d_offsets,
                                          deferred ? h->enc.out_extra[0].as<uint8_t>() : nullptr, n_deferred, out_bytes); });
}

int nfagg_encode_flp_json_device(nfagg_handle* h, const void* d_records, size_t n, const nfagg_flp_options* opt,
                                 void* d_out, size_t out_cap, uint64_t* d_line_offsets, uint8_t* d_deferred,
                                 size_t* n_deferred, size_t* out_bytes) {
    return encode_flp_device_core(h, d_records, n, nullptr, nullptr, FlpLineTables{}, opt, d_out, out_cap, d_line_offsets, d_deferred, n_deferred, out_bytes);
}

int nfagg_encode_flp_json(nfagg_handle* h, const void* records, size_t n, const nfagg_flp_options* opt,
                          void* out, size_t out_cap, uint64_t* line_offsets, uint8_t* deferred,
                          size_t* n_deferred, size_t* out_bytes) {
    return encode_flp_host_core(h, records, n, nullptr, nullptr, FlpLineTables{}, opt, out, out_cap, line_offsets, deferred, n_deferred, out_bytes);
}

// features == NULL: the flows carry no parts, the call is nfagg_encode_flp_json[_device]
int nfagg_encode_flp_json_content_device(nfagg_handle* h, const void* d_records, size_t n, const nfagg_pb_features* d_features,
                                         const nfagg_flp_options* opt, void* d_out, size_t out_cap, uint64_t* d_line_offsets,
                                         uint8_t* d_deferred, size_t* n_deferred, size_t* out_bytes) {
    return encode_flp_device_core(h, d_records, n, d_features, nullptr, FlpLineTables{}, opt, d_out, out_cap, d_line_offsets, d_deferred, n_deferred, out_bytes);
}

int nfagg_encode_flp_json_content(nfagg_handle* h, const void* records, size_t n, const nfagg_pb_features* features,
                                  const nfagg_flp_options* opt, void* out, size_t out_cap, uint64_t* line_offsets,
                                  uint8_t* deferred, size_t* n_deferred, size_t* out_bytes) {
    return encode_flp_host_core(h, records, n, features, nullptr, FlpLineTables{}, opt, out, out_cap, line_offsets, deferred, n_deferred, out_bytes);
}

int nfagg_encode_flp_json_content_netev_device(nfagg_handle* h, const void* d_records, size_t n, const nfagg_pb_features* d_features,
                                               const uint16_t* d_rows, const nfagg_netev_table* table,
                                               const nfagg_flp_options* opt, void* d_out, size_t out_cap, uint64_t* d_line_offsets,
                                               uint8_t* d_deferred, size_t* n_deferred, size_t* out_bytes) {
    const NetevArgs ne{d_rows, table};
    return encode_flp_device_core(h, d_records, n, d_features, &ne, FlpLineTables{}, opt, d_out, out_cap, d_line_offsets, d_deferred, n_deferred, out_bytes);
}

int nfagg_encode_flp_json_content_netev(nfagg_handle* h, const void* records, size_t n, const nfagg_pb_features* features,
                                        const uint16_t* rows, const nfagg_netev_table* table,
                                        const nfagg_flp_options* opt, void* out, size_t out_cap, uint64_t* line_offsets,
                                        uint8_t* deferred, size_t* n_deferred, size_t* out_bytes) {
    const NetevArgs ne{rows, table};
    return encode_flp_host_core(h, records, n, features, &ne, FlpLineTables{}, opt, out, out_cap, line_offsets, deferred, n_deferred, out_bytes);
}

// ---- direct-FLP JSON with the TLS names, the Kubernetes keys, the transform network keys: the tables are nfagg_api_tables.hip's
uint32_t nfagg_flp_json_tls_max_line(int policy) { return flp_max_line(FlpLevel::Tls, policy); }

int nfagg_encode_flp_json_tls_device(nfagg_handle* h, const void* d_records, size_t n, const nfagg_pb_features* d_features,
                                     const uint16_t* d_rows, const nfagg_netev_table* netev_table, const nfagg_tls_names* tls_names,
                                     const nfagg_flp_options* opt, void* d_out, size_t out_cap, uint64_t* d_line_offsets, size_t* out_bytes) {
    const NetevArgs ne{d_rows, netev_table};
    const FlpLineTables t{FlpLevel::Tls, tls_names};
    return encode_flp_device_core(h, d_records, n, d_features, &ne, t, opt, d_out, out_cap, d_line_offsets, nullptr, nullptr, out_bytes);
}

int nfagg_encode_flp_json_tls(nfagg_handle* h, const void* records, size_t n, const nfagg_pb_features* features,
                              const uint16_t* rows, const nfagg_netev_table* netev_table, const nfagg_tls_names* tls_names,
                              const nfagg_flp_options* opt, void* out, size_t out_cap, uint64_t* line_offsets, size_t* out_bytes) {
    const NetevArgs ne{rows, netev_table};
    const FlpLineTables t{FlpLevel::Tls, tls_names};
    return encode_flp_host_core(h, records, n, features, &ne, t, opt, out, out_cap, line_offsets, nullptr, nullptr, out_bytes);
}

uint32_t nfagg_flp_json_k8s_max_line(int policy) { return flp_max_line(FlpLevel::K8s, policy); }

int nfagg_encode_flp_json_k8s_device(nfagg_handle* h, const void* d_records, size_t n, const nfagg_pb_features* d_features,
                                     const uint16_t* d_rows, const nfagg_netev_table* netev_table, const nfagg_tls_names* tls_names,
                                     const nfagg_k8s_table* k8s_table, const nfagg_flp_options* opt, void* d_out, size_t out_cap,
                                     uint64_t* d_line_offsets, size_t* out_bytes) {
    const NetevArgs ne{d_rows, netev_table};
    const FlpLineTables t{FlpLevel::K8s, tls_names, k8s_table};
    return encode_flp_device_core(h, d_records, n, d_features, &ne, t, opt, d_out, out_cap, d_line_offsets, nullptr, nullptr, out_bytes);
}

int nfagg_encode_flp_json_k8s(nfagg_handle* h, const void* records, size_t n, const nfagg_pb_features* features,
                              const uint16_t* rows, const nfagg_netev_table* netev_table, const nfagg_tls_names* tls_names,
                              const nfagg_k8s_table* k8s_table, const nfagg_flp_options* opt, void* out, size_t out_cap,
                              uint64_t* line_offsets, size_t* out_bytes) {
    const NetevArgs ne{rows, netev_table};
    const FlpLineTables t{FlpLevel::K8s, tls_names, k8s_table};
    return encode_flp_host_core(h, records, n, features, &ne, t, opt, out, out_cap, line_offsets, nullptr, nullptr, out_bytes);
}

uint32_t nfagg_flp_json_net_max_line(int policy) { return flp_max_line(FlpLevel::Net, policy); }

int nfagg_encode_flp_json_net_device(nfagg_handle* h, const void* d_records, size_t n, const nfagg_pb_features* d_features,
                                     const uint16_t* d_rows, const nfagg_netev_table* netev_table, const nfagg_tls_names* tls_names,
                                     const nfagg_k8s_table* k8s_table, const nfagg_net_table* net_table, const nfagg_flp_options* opt,
                                     void* d_out, size_t out_cap, uint64_t* d_line_offsets, size_t* out_bytes) {
    const NetevArgs ne{d_rows, netev_table};
    const FlpLineTables t{FlpLevel::Net, tls_names, k8s_table, net_table};
    return encode_flp_device_core(h, d_records, n, d_features, &ne, t, opt, d_out, out_cap, d_line_offsets, nullptr, nullptr, out_bytes);
}

int nfagg_encode_flp_json_net(nfagg_handle* h, const void* records, size_t n, const nfagg_pb_features* features,
                              const uint16_t* rows, const nfagg_netev_table* netev_table, const nfagg_tls_names* tls_names,
                              const nfagg_k8s_table* k8s_table, const nfagg_net_table* net_table, const nfagg_flp_options* opt,
                              void* out, size_t out_cap, uint64_t* line_offsets, size_t* out_bytes) {
    const NetevArgs ne{rows, netev_table};
    const FlpLineTables t{FlpLevel::Net, tls_names, k8s_table, net_table};
    return encode_flp_host_core(h, records, n, features, &ne, t, opt, out, out_cap, line_offsets, nullptr, nullptr, out_bytes);
}

// ---- extract conntrack's flow logs: the *_net line with _HashId and _RecordType, no line for a flow the stage does not track
uint32_t nfagg_flp_json_conn_max_line(int policy) { return flp_max_line(FlpLevel::Conn, policy); }

int nfagg_encode_flp_json_conn_device(nfagg_handle* h, const void* d_records, size_t n, const nfagg_pb_features* d_features,
                                      const uint16_t* d_rows, const nfagg_netev_table* netev_table, const nfagg_tls_names* tls_names,
                                      const nfagg_k8s_table* k8s_table, const nfagg_net_table* net_table, const uint64_t* d_hash_ids,
                                      const nfagg_flp_options* opt, void* d_out, size_t out_cap, uint64_t* d_line_offsets, size_t* out_bytes) {
    const NetevArgs ne{d_rows, netev_table};
    const FlpLineTables t{FlpLevel::Conn, tls_names, k8s_table, net_table, d_hash_ids};
    return encode_flp_device_core(h, d_records, n, d_features, &ne, t, opt, d_out, out_cap, d_line_offsets, nullptr, nullptr, out_bytes);
}

int nfagg_encode_flp_json_conn(nfagg_handle* h, const void* records, size_t n, const nfagg_pb_features* features,
                               const uint16_t* rows, const nfagg_netev_table* netev_table, const nfagg_tls_names* tls_names,
                               const nfagg_k8s_table* k8s_table, const nfagg_net_table* net_table, const uint64_t* hash_ids,
                               const nfagg_flp_options* opt, void* out, size_t out_cap, uint64_t* line_offsets, size_t* out_bytes) {
    const NetevArgs ne{rows, netev_table};
    const FlpLineTables t{FlpLevel::Conn, tls_names, k8s_table, net_table, hash_ids};
    return encode_flp_host_core(h, records, n, features, &ne, t, opt, out, out_cap, line_offsets, nullptr, nullptr, out_bytes);
}

// ---- extract conntrack's conversation records as JSON lines (nfagg_conn_json.hip): the layout, then the two entry points
int nfagg_conn_layout_create(nfagg_handle* h, const nfagg_conn_field* fields, size_t n_fields, nfagg_conn_layout** layout) {
    if (!layout || (n_fields && !fields)) return fail(h, NFAGG_EINVAL, "null argument");
    *layout = nullptr;
    if (n_fields > NFAGG_CONN_MAX_FIELDS) return fail(h, NFAGG_EINVAL, "%zu output fields, more than %d", n_fields, NFAGG_CONN_MAX_FIELDS);
    struct Named { std::string name; ConnCol col; uint32_t value_max; };
    std::vector<Named> cols;
    static const char* const kKeys[5] = {"SrcAddr", "DstAddr", "SrcPort", "DstPort", "Proto"};
    static const uint32_t kKeyMax[5] = {kConnAddrMax, kConnAddrMax, 5, 5, 3};
    for (uint32_t k = 0; k < 5; k++) cols.push_back({kKeys[k], {kConnColKey, k, 0, 0}, kKeyMax[k]});
    static const char* const kBlocks[5] = {"DstK8S_", "DstSubnetLabel", "K8S_FlowLayer", "SrcK8S_", "SrcSubnetLabel"};
    const uint32_t layer_max = sizeof(",\"K8S_FlowLayer\":\"infra\"") - 1;
    const uint32_t block_max[5] = {kK8sMaxRendered, kNetFragMax, layer_max, kK8sMaxRendered, kNetFragMax};
    for (uint32_t k = 0; k < 5; k++) cols.push_back({kBlocks[k], {kConnColBlock, k, 0, 0}, block_max[k]});
    static const char* const kMeta[3] = {"_HashId", "_IsFirst", "_RecordType"};
    static const uint32_t kMetaMax[3] = {kConnHashIdMax, kConnIsFirstMax, kConnRecordTypeMax};
    for (uint32_t k = 0; k < 3; k++) cols.push_back({kMeta[k], {kConnColMeta, k, 0, 0}, kMetaMax[k]});
    for (size_t k = 0; k < n_fields; k++) {
        const nfagg_conn_field& f = fields[k];
        if (!f.name_len || !f.name) return fail(h, NFAGG_EINVAL, "output field %zu: empty name", k);
        if (f.name_len > NFAGG_CONN_NAME_MAX) return fail(h, NFAGG_EINVAL, "output field %zu: name of %u bytes, more than %d", k, f.name_len, NFAGG_CONN_NAME_MAX);
        const std::string name(f.name, f.name_len);
        if (name.compare(0, 7, "SrcK8S_") == 0 || name.compare(0, 7, "DstK8S_") == 0)
            return fail(h, NFAGG_EINVAL, "output field %zu (%s): the name begins with a Kubernetes block's prefix", k, name.c_str());
        for (const char* r : {"K8S_FlowLayer", "SrcSubnetLabel", "DstSubnetLabel", "_HashId", "_IsFirst", "_RecordType"})
            if (name == r) return fail(h, NFAGG_EINVAL, "output field %zu (%s): the name is a column of the line's own", k, name.c_str());
        const bool split = f.split_ab != 0;
        uint32_t src = 0, vmax = kConnAggMax, kind = kConnColAgg;
        switch (f.op) {
        case NFAGG_CONN_OP_COUNT: src = 0; break;
        case NFAGG_CONN_OP_SUM:
            if (f.input != NFAGG_CONN_IN_BYTES && f.input != NFAGG_CONN_IN_PACKETS)
                return fail(h, NFAGG_EINVAL, "output field %zu (%s): sum is served over Bytes and Packets", k, name.c_str());
            src = f.input == NFAGG_CONN_IN_BYTES ? 1 : 2;
            break;
        case NFAGG_CONN_OP_MIN:
            if (f.input != NFAGG_CONN_IN_TIME_START || split) return fail(h, NFAGG_EINVAL, "output field %zu (%s): min is served over TimeFlowStartMs, not split", k, name.c_str());
            src = 3;
            break;
        case NFAGG_CONN_OP_MAX:
            if (f.input != NFAGG_CONN_IN_TIME_END || split) return fail(h, NFAGG_EINVAL, "output field %zu (%s): max is served over TimeFlowEndMs, not split", k, name.c_str());
            src = 4;
            break;
        case NFAGG_CONN_OP_FIRST: case NFAGG_CONN_OP_LAST:
            if (f.input < NFAGG_CONN_IN_TIME_START || f.input > NFAGG_CONN_IN_IF_DIRECTIONS || split)
                return fail(h, NFAGG_EINVAL, "output field %zu (%s): first / last take one of the snapshot's inputs, not split", k, name.c_str());
            kind = kConnColSnap;
            src = f.input | (f.op == NFAGG_CONN_OP_LAST ? 1u << 8 : 0u);
            vmax = (f.input == NFAGG_CONN_IN_SRC_ADDR || f.input == NFAGG_CONN_IN_DST_ADDR) ? kConnAddrMax
                   : (f.input == NFAGG_CONN_IN_SRC_MAC || f.input == NFAGG_CONN_IN_DST_MAC) ? kConnMacMax
                   : f.input == NFAGG_CONN_IN_IF_DIRECTIONS ? kConnDirsMax : kConnI64Max;
            break;
        default: return fail(h, NFAGG_EINVAL, "output field %zu (%s): unknown operation %u", k, name.c_str(), f.op);
        }
        for (uint32_t side = split ? 1 : 0; side <= (split ? 2u : 0u); side++) {
            const std::string full = name + (side == 1 ? "_AB" : side == 2 ? "_BA" : "");
            bool is_key = false;
            for (const Named& c : cols) {
                if (c.name != full) continue;
                if (c.col.kind != kConnColKey) return fail(h, NFAGG_EINVAL, "output field %zu: duplicate name %s", k, full.c_str());
                is_key = true;                                      // conn.go:109-112: the keys prevail
            }
            if (!is_key) cols.push_back({full, {kind, kind == kConnColAgg ? src | side << 8 : src, 0, 0}, vmax});
        }
    }
    std::stable_sort(cols.begin(), cols.end(), [](const Named& a, const Named& b) { return a.name < b.name; });
    nfagg_conn_layout* t = new nfagg_conn_layout;
    t->h = h;
    size_t longest = 2;                                             // the closing brace and the newline; the opening brace takes a comma's place
    for (Named& c : cols) {
        if (c.col.kind != kConnColBlock) {
            uint8_t esc[2 + 6 * (NFAGG_CONN_NAME_MAX + 3)];
            const uint32_t el = flp_escape(c.name.data(), (uint32_t)c.name.size(), esc);
            c.col.frag_off = (uint32_t)t->blob.size();
            c.col.frag_len = el + 2;
            t->blob.push_back(',');
            t->blob.insert(t->blob.end(), esc, esc + el);
            t->blob.push_back(':');
            t->blob.resize((t->blob.size() + 15) / 16 * 16, 0);
        }
        longest += c.col.frag_len + c.value_max;
        t->cols.push_back(c.col);
    }
    t->max_line = (uint32_t)longest;
    if (longest > kConnLineCap) {
        delete t;
        return fail(h, NFAGG_ERANGE, "the layout's longest line has %zu bytes, more than %u", longest, kConnLineCap);
    }
    if (h) {
        auto up = [&]() -> int {
            const size_t cols_bytes = t->cols.size() * sizeof(ConnCol);            // a multiple of 16
            std::vector<uint8_t> img(cols_bytes + t->blob.size() + 16, 0);
            memcpy(img.data(), t->cols.data(), cols_bytes);
            memcpy(img.data() + cols_bytes, t->blob.data(), t->blob.size());
            HIP_TRY(h, hipSetDevice(h->device));
            HIP_TRY(h, t->d_mem.alloc(img.size()));
            HIP_TRY(h, hipMemcpy(t->d_mem.p, img.data(), img.size(), hipMemcpyHostToDevice));
            return NFAGG_OK;
        };
        const int rc = up();
        if (rc != NFAGG_OK) { nfagg_conn_layout_destroy(t); return rc; }
    }
    *layout = t;
    return NFAGG_OK;
}

void nfagg_conn_layout_destroy(nfagg_conn_layout* t) { destroy_on_handle(t); }

uint32_t nfagg_conn_layout_columns(const nfagg_conn_layout* t) { return t ? (uint32_t)t->cols.size() : 0u; }
uint32_t nfagg_conn_layout_max_line(const nfagg_conn_layout* t) { return t ? t->max_line : 0u; }

int nfagg_conn_layout_render(const nfagg_conn_layout* t, uint32_t column, void* out, size_t cap, size_t* n_out) {
    if (!t || !n_out) return fail(nullptr, NFAGG_EINVAL, "null argument");
    if (column >= t->cols.size()) return fail(nullptr, NFAGG_EINVAL, "column %u of %zu", column, t->cols.size());
    const ConnCol& c = t->cols[column];
    *n_out = c.frag_len;
    if (c.frag_len > cap || (c.frag_len && !out)) return NFAGG_TRUNCATED;
    if (c.frag_len) memcpy(out, t->blob.data() + c.frag_off, c.frag_len);
    return NFAGG_OK;
}

int nfagg_encode_conn_json_device(nfagg_handle* h, const void* d_carriers, const nfagg_conn_values* d_values, size_t n,
                                  const nfagg_conn_layout* layout, const nfagg_k8s_table* k8s, const nfagg_net_table* net,
                                  void* d_out, size_t out_cap, uint64_t* d_line_offsets, uint8_t* d_deferred, size_t* n_deferred,
                                  size_t* out_bytes) {
    if (!h || !layout || !k8s || !net || !out_bytes || !d_line_offsets || (n && (!d_carriers || !d_values))) return fail(h, NFAGG_EINVAL, "null argument");
    if (layout->h != h || !layout->d_mem) return fail(h, NFAGG_EINVAL, "the layout was not created for this handle");
    if (k8s->h != h || !k8s->d_slots) return fail(h, NFAGG_EINVAL, "the Kubernetes table was not created for this handle");
    if (net->h != h || !net->d_mem) return fail(h, NFAGG_EINVAL, "the net table was not created for this handle");
    if ((((uintptr_t)d_carriers | (uintptr_t)d_values | (uintptr_t)d_out) & 15u) != 0) return fail(h, NFAGG_EINVAL, "device buffers must be 16-byte aligned");
    if (n_deferred) *n_deferred = 0;
    int rc;
    bool done;
    if ((rc = encode_begin(h, n, d_line_offsets, out_bytes, nullptr, 0, &done)) != NFAGG_OK || done) return rc;
    auto& S = h->enc;
    API_TRY(ensure_all(h, {{S.flp_rows, n * sizeof(uint32_t)}, {S.flp_n_deferred, 16}, {S.k8s_rows, n * 2 * sizeof(uint32_t)}, {S.net_rows, n * sizeof(uint2)}}));
    HIP_TRY(h, hipMemsetAsync(S.flp_n_deferred.p, 0, 16, h->stream));
    uint32_t* lens = S.flp_rows.as<uint32_t>();
    uint32_t* k8s_rows = S.k8s_rows.as<uint32_t>();
    const K8sDev K = k8s_dev(k8s);
    const NetDev N = net_dev(net);
    const ConnLayoutDev L{layout->d_mem.as<const ConnCol>(), layout->d_mem.as<const uint8_t>() + layout->cols.size() * sizeof(ConnCol), (uint32_t)layout->cols.size()};
    // the carriers are flow records: both joins run on them unchanged. A conversation has no AgentIP, so no reporter and no direction.
    hipError_t e = launch_k8s_resolve(d_carriers, n, K, k8s_rows, h->stream);
    if (e != hipSuccess) return fail(h, NFAGG_EDEVICE, "Kubernetes resolve launch failed: %s", hipGetErrorString(e));
    e = launch_net_resolve(d_carriers, n, N, k8s_rows, k8s->d_host_ids.as<const uint32_t>(), K.n_rows, kNetNoHost, S.net_rows.as<uint2>(), h->stream);
    if (e != hipSuccess) return fail(h, NFAGG_EDEVICE, "net resolve launch failed: %s", hipGetErrorString(e));
    uint32_t deferred = 0;
    rc = encode_two_pass(h, n, {"conversation JSON", "size", "write"}, d_out, out_cap, out_bytes, {S.flp_n_deferred.p, &deferred, sizeof deferred},
        [&](uint32_t* local_off, uint32_t* block_sum, uint64_t* block_base) {
            return launch_conn_json_size(d_carriers, d_values, n, L, K, N, k8s_rows, S.net_rows.as<const uint2>(), lens, local_off, block_sum, block_base,
                                         S.flp_n_deferred.as<uint32_t>(), h->stream); },
        [&](const uint32_t* local_off, const uint64_t* block_base, uint64_t) {
            return launch_conn_json_write(d_carriers, d_values, n, L, K, N, k8s_rows, S.net_rows.as<const uint2>(), lens, local_off, block_base, d_out,
                                          d_line_offsets, d_deferred, h->stream); });
    if (n_deferred) *n_deferred = deferred;
    return rc;
}

int nfagg_encode_conn_json(nfagg_handle* h, const void* carriers, const nfagg_conn_values* values, size_t n, const nfagg_conn_layout* layout,
                           const nfagg_k8s_table* k8s, const nfagg_net_table* net, void* out, size_t out_cap,
                           uint64_t* line_offsets, uint8_t* deferred, size_t* n_deferred, size_t* out_bytes) {
    if (!h || !layout || !k8s || !net || !out_bytes || !line_offsets || (n && (!carriers || !values))) return fail(h, NFAGG_EINVAL, "null argument");
    return encode_staged(h, carriers, n, out, out_cap, line_offsets, out_bytes, {{deferred, 1}},
        [&](const void* d_carriers, void* d_out, uint64_t* d_offsets) {
            API_TRY(stage_in(h, h->enc.conn_out, values, n * sizeof(nfagg_conn_values)));
            return nfagg_encode_conn_json_device(h, d_carriers, h->enc.conn_out.as<const nfagg_conn_values>(), n, layout, k8s, net, d_out, out_cap, d_offsets,
                                                 deferred ? h->enc.out_extra[0].as<uint8_t>() : nullptr, n_deferred, out_bytes); });
}

}  // extern "C"
