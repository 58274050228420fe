// nfagg_flp.h — launch interface of the record -> direct-FLP JSON line kernels (nfagg_flp_line.h; nfagg_flp.hip, nfagg_flp_content.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/nfagg.h"
#include "nfagg_hash.h"
#include "nfagg_pb.h"

namespace nfagg {

// One row of the escaped namer table the host builds when it stages the table (nfagg_api_export.hip): the row's name and UDN
// as JSON strings, quotes included, escaped once per call and not per flow. Row 0 is the unknown name (UDN ""), row
// k + 1 is row k of the sorted table. name: at most 2 + 6 x 16 bytes, udn: at most 2 + 6 x 63.
constexpr uint32_t kFlpEscRowBytes = 512;
constexpr uint32_t kFlpEscNameOff = 16, kFlpEscNameMax = 98;      // name_len (u16) @0, udn_len (u16) @2
constexpr uint32_t kFlpEscUdnOff = 128, kFlpEscUdnMax = 380;
static_assert(kFlpEscNameOff + kFlpEscNameMax <= kFlpEscUdnOff && kFlpEscUdnOff + kFlpEscUdnMax <= kFlpEscRowBytes, "escaped row layout");

struct FlpParams {
    int64_t now_sec, now_nsec;    // currentTime, normalised (0 <= nsec < 1e9)
    uint64_t mono_now;
    int64_t time_received;
    const nfagg_intf_name* names; // device copy of the namer table, stably sorted by if_index
    const uint8_t* esc;           // device copy of the escaped table, n_names + 1 rows of kFlpEscRowBytes
    uint32_t n_names;
    uint32_t agent_nil;           // Record.AgentIP == nil: "<nil>"
    uint32_t agent_ip_w[4];       // Record.AgentIP as a 16-byte net.IP, four little-endian dwords
};

// The TLS name table of nfagg_tls_names_create on the device (nfagg_tls.h): per kind kTlsMaxRows ids, ascending, the first
// n[kind] of them in use, and as many 64-byte rows (a length byte, then up to 63 name bytes).
constexpr uint32_t kTlsKinds = 3, kTlsMaxRows = NFAGG_TLS_MAX_ROWS, kTlsRowBytes = 64;
static_assert(NFAGG_TLS_NAME_MAX + 1 == kTlsRowBytes && (kTlsMaxRows & (kTlsMaxRows - 1)) == 0, "TLS name row layout, search steps");
struct TlsDev {
    const uint16_t* ids;          // [kTlsKinds][kTlsMaxRows]
    const uint8_t* rows;          // [kTlsKinds][kTlsMaxRows][kTlsRowBytes], 16-byte aligned
    uint32_t n[kTlsKinds];
};

// The Kubernetes table of nfagg_k8s_table_create on the device (nfagg_k8s.h). Slots: open addressing over the 16 address
// bytes, a power of two of them, at most half in use, home slot = the low bits of k8s_hash, linear probe; a slot is 32
// bytes so that one aligned read holds the key and the row (row == kK8sNoRow: free). Rows: where the row's two rendered
// blocks (",\"SrcK8S_..\":..", ",\"DstK8S_..\":..", each at most kK8sMaxRendered bytes) start in the blob, in 16-byte units,
// and their lengths; kK8sRowApp: the namespace is not empty and objectIsApp holds (enrich.go:143-165).
constexpr uint32_t kK8sNoRow = NFAGG_K8S_NO_ROW, kK8sMaxRendered = NFAGG_K8S_MAX_RENDERED, kK8sSeedIndex = 3, kK8sRowApp = 1;
NF_HD uint64_t k8s_hash(uint64_t lo, uint64_t hi) { return ip_hash(lo, hi, kK8sSeedIndex); }
struct K8sSlot { uint32_t ip[4]; uint32_t row; uint32_t pad_[3]; };
struct K8sRow { uint32_t src_off, dst_off; uint16_t src_len, dst_len; uint32_t flags; };
static_assert(sizeof(K8sSlot) == 32 && sizeof(K8sRow) == 16, "Kubernetes table layout");
struct K8sDev {
    const K8sSlot* slots;         // mask + 1 of them, 32-byte aligned
    const K8sRow* rows;
    const uint8_t* blob;          // 16-byte aligned
    uint32_t mask, n_rows;
    uint32_t has_layer;           // the table was created with a layer: every line carries K8S_FlowLayer
};

// Line lengths (0 = deferred) and the seven resolved interface rows per record (d_rows: 8 dwords per record, rows 0..6
// and the length), block-local scan, scan of the block sums: d_block_base[ceil(n / 1024)] = total bytes afterwards. Then the
// write pass. F (optional) names the feature parts of full BpfFlowContents as it does for the protobuf encoder; with
// F->ne_rows the line carries the flows' network events. T (optional): TLSVersion, TLSCipherSuite and TLSGroup are looked up in
// it and written. Without T a record that has them is deferred: no line, d_deferred[i] = 1 (where given), counted in
// *d_n_deferred (zeroed by the caller); with T neither is touched.
hipError_t launch_flp_size(const void* d_recs, uint64_t n, const FlpParams& P, const PbFeat* F, const TlsDev* T, uint32_t* d_rows,
                           uint32_t* d_local_off, uint32_t* d_block_sum, uint64_t* d_block_base, uint32_t* d_n_deferred, hipStream_t s);
hipError_t launch_flp_write(const void* d_recs, uint64_t n, const FlpParams& P, const PbFeat* F, const TlsDev* T, const uint32_t* d_rows,
                            const uint32_t* d_local_off, const uint64_t* d_block_base, void* d_out, uint64_t* d_line_offsets,
                            uint8_t* d_deferred, hipStream_t s);
// The longest line each policy can write with T (0: plain, 1: content, 2: content with network events).
uint32_t flp_tls_max_line(int policy);

// The same two passes with the Kubernetes enrichment on top of T (required): d_k8s_rows holds two rows per record, as
// launch_k8s_resolve (nfagg_k8s.hip: one lane per flow, two probes of K) wrote them. Nothing is deferred.
hipError_t launch_k8s_resolve(const void* d_recs, uint64_t n, const K8sDev& K, uint32_t* d_rows_out, hipStream_t s);
hipError_t launch_flp_k8s_size(const void* d_recs, uint64_t n, const FlpParams& P, const PbFeat* F, const TlsDev& T, const K8sDev& K,
                               const uint32_t* d_k8s_rows, uint32_t* d_rows, uint32_t* d_local_off, uint32_t* d_block_sum, uint64_t* d_block_base,
                               hipStream_t s);
hipError_t launch_flp_k8s_write(const void* d_recs, uint64_t n, const FlpParams& P, const PbFeat* F, const TlsDev& T, const K8sDev& K,
                                const uint32_t* d_k8s_rows, const uint32_t* d_rows, const uint32_t* d_local_off, const uint64_t* d_block_base,
                                void* d_out, uint64_t* d_line_offsets, hipStream_t s);
uint32_t flp_k8s_max_line(int policy);

// The table of nfagg_net_table_create on the device (nfagg_net.h): the CIDR list in walk order, every entry normalised so
// that one masked compare of the 16 address bytes decides Contains within the family (an IPv4 network carries the
// v4-mapped prefix in `net` and twelve 0xff bytes in front of its mask; an IPv6 one is flagged, and a v4-mapped address
// never matches it); per label the two rendered fragments in a blob, 16-byte aligned.
constexpr uint32_t kNetMaxCidrs = NFAGG_NET_MAX_CIDRS, kNetLabelMax = NFAGG_NET_LABEL_MAX, kNetNoLabel = NFAGG_NET_NO_LABEL,
                   kNetNoDirection = NFAGG_NET_NO_DIRECTION, kNetCidrV6 = 1u << 16, kNetNoHost = 0xFFFFFFFFu;
constexpr uint32_t kNetFragMax = (sizeof(",\"SrcSubnetLabel\":\"\"") - 1) + kNetLabelMax;      // one fragment: key text, quotes, the escaped label
struct NetCidr { uint32_t net[4]; uint32_t mask[4]; };
struct NetFrag { uint32_t src_off, src_len, dst_off, dst_len; };      // offsets in 16-byte units; len 0: an empty label, no key
static_assert(sizeof(NetCidr) == 32 && sizeof(NetFrag) == 16, "net table layout");
struct NetDev {
    const NetCidr* cidrs;         // n_cidrs of them, 32-byte aligned
    const uint32_t* meta;         // per CIDR: its label | kNetCidrV6
    const NetFrag* frags;         // n_labels of them
    const uint8_t* blob;          // 16-byte aligned
    uint32_t n_cidrs, n_labels, flags;
};

// The join of nfagg_net_resolve (nfagg_net.hip: one lane per flow): 8 bytes per record, nfagg_net_row. d_k8s_rows / d_host_ids
// / reporter: the flows' Kubernetes rows, the rows' interned host-IP ids and the reporter's id (kNetNoHost: no row has its
// text); read only with NFAGG_NET_REINTERPRET_DIRECTION.
hipError_t launch_net_resolve(const void* d_recs, uint64_t n, const NetDev& N, const uint32_t* d_k8s_rows, const uint32_t* d_host_ids,
                              uint32_t n_k8s_rows, uint32_t reporter, uint2* d_out, hipStream_t s);
hipError_t launch_flp_net_size(const void* d_recs, uint64_t n, const FlpParams& P, const PbFeat* F, const TlsDev& T, const K8sDev& K,
                               const NetDev& N, const uint32_t* d_k8s_rows, const uint2* d_net_rows, uint32_t* d_rows, uint32_t* d_local_off,
                               uint32_t* d_block_sum, uint64_t* d_block_base, hipStream_t s);
hipError_t launch_flp_net_write(const void* d_recs, uint64_t n, const FlpParams& P, const PbFeat* F, const TlsDev& T, const K8sDev& K,
                                const NetDev& N, const uint32_t* d_k8s_rows, const uint2* d_net_rows, const uint32_t* d_rows,
                                const uint32_t* d_local_off, const uint64_t* d_block_base, void* d_out, uint64_t* d_line_offsets, hipStream_t s);
uint32_t flp_net_max_line(int policy);

// The same two passes as extract conntrack's flow logs (nfagg_conn_meta.h): d_hash_ids holds one id per record, as
// launch_conn_fold wrote them. A flow the stage does not track gets a zero-length line; the others end in _HashId and _RecordType.
hipError_t launch_flp_conn_size(const void* d_recs, uint64_t n, const FlpParams& P, const PbFeat* F, const TlsDev& T, const K8sDev& K,
                                const NetDev& N, const uint32_t* d_k8s_rows, const uint2* d_net_rows, const uint64_t* d_hash_ids, uint32_t* d_rows,
                                uint32_t* d_local_off, uint32_t* d_block_sum, uint64_t* d_block_base, hipStream_t s);
hipError_t launch_flp_conn_write(const void* d_recs, uint64_t n, const FlpParams& P, const PbFeat* F, const TlsDev& T, const K8sDev& K,
                                 const NetDev& N, const uint32_t* d_k8s_rows, const uint2* d_net_rows, const uint64_t* d_hash_ids,
                                 const uint32_t* d_rows, const uint32_t* d_local_off, const uint64_t* d_block_base, void* d_out,
                                 uint64_t* d_line_offsets, hipStream_t s);
uint32_t flp_conn_max_line(int policy);

}  // namespace nfagg
