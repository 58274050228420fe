// nfagg_k8s.h — the Kubernetes enrichment of the direct-FLP JSON line (flowlogs-pipeline transform network: add_kubernetes
// for SrcAddr and DstAddr, then add_kubernetes_infra; enrich.go:37-104,140-165), as a feature policy on top of FlpTls<Base>
// that k_flp_size / k_flp_write (nfagg_flp_line.h) run. The informers' answers come as the caller's table (nfagg_k8s_table_create): both
// sides' blocks of a row are rendered once on the host, a flow costs two probes of an open-addressed table (k_k8s_resolve,
// nfagg_k8s.hip) and a byte copy per block. Device code only; the table's layout is in nfagg_flp.h.
//   after DstAddr:     [,"DstK8S_HostIP":..,"DstK8S_Zone":..]   the dst row's block
//   after Interfaces:  [,"K8S_FlowLayer":"app"|"infra"]        with a layer
//   after SrcAddr:     [,"SrcK8S_HostIP":..,"SrcK8S_Zone":..]   the src row's block
#pragma once
#include "nfagg_tls.h"

namespace nfagg {

constexpr uint32_t kK8sLayerMax = sizeof(",\"K8S_FlowLayer\":\"infra\"") - 1;
constexpr uint32_t kK8sLineMax = 2 * kK8sMaxRendered + kK8sLayerMax;

// Row of the address w[0..3] (four little-endian dwords), kK8sNoRow when the table has none: linear probe from the
// hash's home slot; a step is the slot's two 16-byte halves, one aligned 32-byte read. The table is at most half full, so
// a probe ends at a free slot.
NF_DEV uint32_t k8s_probe(const K8sDev& K, uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3) {
    const uint64_t lo = (uint64_t)w0 | ((uint64_t)w1 << 32), hi = (uint64_t)w2 | ((uint64_t)w3 << 32);
    uint32_t s = (uint32_t)k8s_hash(lo, hi) & K.mask;
    for (uint32_t t = 0; t <= K.mask; t++) {
        const uint4* p = reinterpret_cast<const uint4*>(K.slots + s);
        const uint4 key = p[0], val = p[1];
        if (val.x == kK8sNoRow) return kK8sNoRow;
        if (key.x == w0 && key.y == w1 && key.z == w2 && key.w == w3) return val.x;
        s = (s + 1) & K.mask;
    }
    return kK8sNoRow;
}

// FlpTls<Base> with the enrichment. The window takes what the longest line leaves of 32 KiB beside the wave's side LDS,
// as FlpTls sizes its own.
template <typename Base> struct FlpK8s : Base {
    static constexpr uint32_t kMaxLine = Base::kMaxLine + kK8sLineMax;
    static constexpr uint32_t kWindow = (32768 - Base::kSideLds - (kMaxLine + 15) / 16 * 16) / 16 * 16;
    static constexpr uint32_t kLds = kWindow + (kMaxLine + 15) / 16 * 16;
    static_assert(!Base::kDefers && kLds + Base::kSideLds <= 32768 && kWindow >= 16384, "four waves per compute unit, and a window worth its copy-out");
    const uint8_t* blob = nullptr;
    uint32_t off[2] = {}, len[2] = {};      // the src and the dst block: offset in 16-byte units, bytes (0: no row)
    uint32_t layer = 0;                     // 0: no key, 1: infra, 2: app

    // rows: the flow's two rows as k_k8s_resolve wrote them (kK8sNoRow for a record that is not IP: it has no address key)
    NF_DEV void load_k8s(const K8sDev& K, const uint32_t* __restrict__ rows, uint64_t i) {
        const uint2 r = reinterpret_cast<const uint2*>(rows)[i];
        const uint32_t row[2] = {r.x, r.y};
        blob = K.blob;
        bool app = false;
#pragma unroll
        for (int k = 0; k < 2; k++)
            if (row[k] < K.n_rows) {
                const uint4 m = reinterpret_cast<const uint4*>(K.rows)[row[k]];       // K8sRow
                off[k] = k ? m.y : m.x;
                len[k] = k ? m.z >> 16 : m.z & 0xffffu;
                app = app || (m.w & kK8sRowApp);
            }
        layer = K.has_layer ? (app ? 2u : 1u) : 0u;
    }
    static constexpr bool kJoins = true;
    NF_DEV void load_joins(const FlpJoins& J, uint64_t i) { load_k8s(J.K, J.k8s_rows, i); }
    template <typename S> NF_DEV void k8s_src(S& s) const { if (len[0]) put_blob(s, blob + (size_t)off[0] * 16, len[0]); }
    template <typename S> NF_DEV void k8s_dst(S& s) const { if (len[1]) put_blob(s, blob + (size_t)off[1] * 16, len[1]); }
    template <typename S> NF_DEV void k8s_layer(S& s) const {              // enrich.go:140-151
        if (layer == 2) lit(s, ",\"K8S_FlowLayer\":\"app\"");
        else if (layer == 1) lit(s, ",\"K8S_FlowLayer\":\"infra\"");
    }
};

}  // namespace nfagg
