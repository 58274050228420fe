// nfagg_api_tables.h — the five caller tables behind the opaque types of include/nfagg.h (network events, TLS names,
// Kubernetes, subnets and direction, metrics) as nfagg_api_tables.hip builds them, and what the encoders' host side
// (nfagg_api_export.hip) reads of them. Private to csrc/.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string>
#include <unordered_map>
#include <vector>

#include "nfagg_handle.h"
#include "nfagg_flp.h"
#include "nfagg_netev.h"
#include "nfagg_metrics.h"
#include "nfagg_pb.h"
#include "nfagg_conn_json.h"

// The cookie table of nfagg_netev_table_create: the sorted rows and the rendered blob, on the host and (with a handle) on its device.
struct nfagg_netev_table {
    nfagg_handle* h = nullptr;
    std::vector<nfagg::NetevRow> rows;
    std::vector<uint8_t> blob;
    nfagg::DevBuf d_rows;
    nfagg::DevBuf d_blob;
};

// The TLS name table of nfagg_tls_names_create (nfagg_tls.h):
// per kind the ids ascending and a 64-byte row per id (length byte, name), on the host and (with a handle) on its device.
struct nfagg_tls_names {
    nfagg_handle* h = nullptr;
    uint32_t n[nfagg::kTlsKinds] = {};
    std::vector<uint16_t> ids = std::vector<uint16_t>(nfagg::kTlsKinds * nfagg::kTlsMaxRows, 0);
    std::vector<uint8_t> rows = std::vector<uint8_t>((size_t)nfagg::kTlsKinds * nfagg::kTlsMaxRows * nfagg::kTlsRowBytes, 0);
    nfagg::DevBuf d_mem;        // the ids, then the rows
};

// The Kubernetes table of nfagg_k8s_table_create (nfagg_flp.h, nfagg_k8s.h): the slots, the rows and the rendered blocks, on the
// host and (with a handle) on its device.
struct nfagg_k8s_table {
    nfagg_handle* h = nullptr;
    std::vector<nfagg::K8sSlot> slots;
    std::vector<nfagg::K8sRow> rows;
    std::vector<uint8_t> blob;
    bool has_layer = false;
    // reinterpret_direction compares host-IP TEXT: every row's host_ip interned, 0 for the empty string, in an array of its
    // own beside the rows (the kernels that read K8sRow do not see it); host_text finds a call's reporter
    std::vector<uint32_t> host_ids;
    std::unordered_map<std::string, uint32_t> host_text;
    // nfagg_metrics_table_create groups rows by the TEXT of their fields: nine ids per row in nfagg_k8s_entry's order, 0: the
    // field is absent as nfagg_k8s_render has it, else 1 + the interned text (the empty string has an id like any other).
    // Host side only.
    std::vector<uint32_t> field_ids;
    std::unordered_map<std::string, uint32_t> field_text;
    nfagg::DevBuf d_slots;
    nfagg::DevBuf d_rows;
    nfagg::DevBuf d_blob;
    nfagg::DevBuf d_host_ids;
};

// The table of nfagg_net_table_create (nfagg_flp.h, nfagg_net.h): the normalised CIDR list, the labels' fragments, on the host
// and (with a handle) in one allocation on its device: cidrs, meta, frags, blob, each 32-byte aligned.
struct nfagg_net_table {
    nfagg_handle* h = nullptr;
    uint32_t flags = 0;
    std::vector<nfagg::NetCidr> cidrs;
    std::vector<uint32_t> meta;
    std::vector<nfagg::NetFrag> frags;
    std::vector<uint8_t> blob;
    size_t off_meta = 0, off_frags = 0, off_blob = 0;
    nfagg::DevBuf d_mem;
};

// The table of nfagg_metrics_table_create (nfagg_metrics.h): per grouping and side the class of every row of a Kubernetes table.
struct nfagg_metrics_table {
    nfagg_handle* h = nullptr;
    const nfagg_k8s_table* k8s = nullptr;              // not owned: the caller keeps it alive
    uint32_t n_groupings = 0;
    uint32_t dims[nfagg::kMetMaxGroupings] = {};
    std::vector<uint32_t> cls[nfagg::kMetMaxGroupings][2];    // per row; empty: the grouping selects no field of that side
    std::vector<uint32_t> first_row[nfagg::kMetMaxGroupings][2];   // [class - 1] = the first row of that class
    nfagg::DevBuf d_cls;                             // the non-empty cls arrays one behind the other
    size_t d_off[nfagg::kMetMaxGroupings][2] = {};            // in words
    // nfagg_metrics_table_create_specs: the checked specs (a plain table's are its masks without values, for the content fold)
    bool has_specs = false;
    nfagg_metric_spec specs[nfagg::kMetMaxGroupings] = {};
};

// The layout of nfagg_conn_layout_create (nfagg_conn_json.h): the sorted column program and the rendered key fragments, on the
// host and (with a handle) in one allocation on its device: the columns, then the blob.
struct nfagg_conn_layout {
    nfagg_handle* h = nullptr;
    std::vector<nfagg::ConnCol> cols;
    std::vector<uint8_t> blob;
    uint32_t max_line = 0;
    nfagg::DevBuf d_mem;
};

namespace nfagg {

// jsoniter's Stream.WriteString of src[0..len) into dst (room for 2 + 6 * len bytes); returns the length. The tables' rendered
// text and the encoders' namer table are escaped by the same code.
uint32_t flp_escape(const char* src, uint32_t len, uint8_t* dst);
// The tables as the kernels take them (DEVICE pointers: the table was created with a handle).
NetDev net_dev(const nfagg_net_table* t);
K8sDev k8s_dev(const nfagg_k8s_table* t);
// The reporter of a call for reinterpret_direction: the id of AgentIP's text among the table's host IPs, or kNetNoHost.
uint32_t net_reporter(const nfagg_k8s_table* k8s, const nfagg_flp_options* opt);

// The network events of a call: the flows' rows (DEVICE memory where a PbFeat is filled from them) and the table they index.
struct NetevArgs { const uint16_t* rows; const nfagg_netev_table* table; };
// The tables and ids a call's level takes (nfagg_flp.h: FlpLevel); what lies above the level is not looked at.
struct FlpLineTables {
    FlpLevel level = FlpLevel::Plain;
    const nfagg_tls_names* tls = nullptr; const nfagg_k8s_table* k8s = nullptr; const nfagg_net_table* net = nullptr;
    const uint64_t* hash_ids = nullptr;
};
// The staging stage_flp_line fills and FlpLineArgs then points into: it outlives the kernels that read the arguments.
struct FlpLineStage {
    DevBuf& names; DevBuf& esc; DevBuf& k8s_rows; DevBuf& net_rows;
    std::vector<nfagg_intf_name>& h_names; std::vector<uint8_t>& h_esc;      // host copies, kept until the stream has consumed them
};

}  // namespace nfagg

// The feature parts of a content call (nfagg_api_export.hip), shared by the encoders and the content metrics fold:
// device_features checks a nfagg_pb_features with DEVICE pointers into the kernels' PbFeat; stage_pb_features uploads the parts
// of a host-memory call into the handle's scratch and fills *dfeat with the device pointers.
extern "C" {
int device_features(nfagg_handle* h, const nfagg_pb_features* feat, nfagg::PbFeat* F);
int stage_pb_features(nfagg_handle* h, const nfagg_pb_features* feat, size_t n, nfagg_pb_features* dfeat);

// What the direct-FLP JSON encoders and write loki's plan set up alike for the line kernels (nfagg_api_export.hip). The checks
// come one by one, because the entry points make them in different orders and the first message is part of the C ABI:
//   check_flp_options   null options, struct_size, the namer table's rows
//   netev_together      rows and table both, or neither
//   device_netev        rows and table present, the table this handle's, the rows aligned; then both into F
//   check_flp_tables    the TLS, Kubernetes and net table of t's level are this handle's
// stage_flp_line follows them: the namer table stably sorted by if_index and its escaped rows, uploaded; FlpParams; and by t's
// level TlsDev, k8s_dev and the Kubernetes resolve launch, net_dev and the net resolve launch, the hash ids. *A comes back filled
// for launch_flp_size / launch_flp_write or the Loki kernels.
int check_flp_options(nfagg_handle* h, const nfagg_flp_options* opt);
int netev_together(nfagg_handle* h, const nfagg::NetevArgs& ne, size_t n);
int device_netev(nfagg_handle* h, const nfagg::NetevArgs* ne, size_t n, nfagg::PbFeat* F);
int check_flp_tables(nfagg_handle* h, const nfagg::FlpLineTables& t);
int stage_flp_line(nfagg_handle* h, const void* d_records, size_t n, const nfagg_flp_options* opt, const nfagg::PbFeat& F,
                   const nfagg::FlpLineTables& t, const nfagg::FlpLineStage& st, nfagg::FlpLineArgs* A);
}
