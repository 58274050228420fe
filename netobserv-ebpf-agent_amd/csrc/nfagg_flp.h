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

// The two joins a line may carry, resolved ahead of the line kernels, one lane per flow. launch_k8s_resolve (nfagg_k8s.hip): two
// probes of K, two rows per record. launch_net_resolve (nfagg_net.hip): 8 bytes per record, nfagg_net_row; d_k8s_rows / d_host_ids
// / reporter: the flows' Kubernetes rows, the rows' interned host-IP ids and the reporter's id (kNetNoHost: no row has its
// text); read only with NFAGG_NET_REINTERPRET_DIRECTION.
hipError_t launch_k8s_resolve(const void* d_recs, uint64_t n, const K8sDev& K, uint32_t* d_rows_out, hipStream_t s);
hipError_t launch_net_resolve(const void* d_recs, uint64_t n, const NetDev& N, const uint32_t* d_k8s_rows, const uint32_t* d_host_ids,
                              uint32_t n_k8s_rows, uint32_t reporter, uint2* d_out, hipStream_t s);

// What a line can carry, each level on top of the one before it: the TLS names of T; the Kubernetes keys of K and k8s_rows; the
// transform network keys of N and net_rows; extract conntrack's two keys from hash_ids (one id per record, as launch_conn_fold
// wrote them), and no line for a flow that stage does not track. Below Tls a record with TLS names is deferred.
enum class FlpLevel : int { Plain, Tls, K8s, Net, Conn };

// The arguments of the line kernels at every level, and of write loki's (nfagg_loki.h). A level reads what it names above and
// nothing of the rest. F: every pointer null for the plain line; with F.ne_rows the line carries the flows' network events.
struct FlpLineArgs {
    const void* recs; uint64_t n; FlpParams P; PbFeat F; TlsDev T; K8sDev K; NetDev N;
    const uint32_t* k8s_rows; const uint2* net_rows; const uint64_t* hash_ids;      // write loki: hash_ids nullptr, no conntrack stage
};
// The base policy a call's parts select (0: plain, 1: content, 2: content with network events). Parts without a present array
// load nothing, so which of 0 and 1 runs them changes no byte.
inline int flp_policy(const PbFeat& F) {
    return F.ne_rows ? 2 : (F.present || F.additional || F.dns || F.drops || F.xlat || F.quic) ? 1 : 0;
}

// Line lengths (0: deferred, or not tracked) and the seven resolved interface rows per record (d_rows: 8 dwords per record, rows
// 0..6 and the length), block-local scan, scan of the block sums: d_block_base[ceil(n / 1024)] = total bytes afterwards. Then the
// write pass. Below Tls a deferred record gets no line, d_deferred[i] = 1 (where given), and is counted in *d_n_deferred (zeroed
// by the caller); from Tls on neither is touched.
hipError_t launch_flp_size(const FlpLineArgs& A, FlpLevel level, uint32_t* d_rows, uint32_t* d_local_off, uint32_t* d_block_sum,
                           uint64_t* d_block_base, uint32_t* d_n_deferred, hipStream_t s);
hipError_t launch_flp_write(const FlpLineArgs& A, FlpLevel level, const uint32_t* d_rows, const uint32_t* d_local_off,
                            const uint64_t* d_block_base, void* d_out, uint64_t* d_line_offsets, uint8_t* d_deferred, hipStream_t s);
// The longest line a level can write over each base policy; 0 for a policy there is none of.
uint32_t flp_max_line(FlpLevel level, int policy);

}  // namespace nfagg
