// nfagg_conn_meta.h — the flow logs of flowlogs-pipeline's extract conntrack stage on the direct-FLP JSON line, as a feature
// policy on top of FlpNet<FlpK8s<FlpTls<Base>>> that k_flp_size / k_flp_write (nfagg_flp_line.h) run. The stage drops every flow its filter
// turns away (conntrack.go:70-74) and adds two keys to the others (conntrack.go:120-126, 281-287):
//   an untracked flow:   no line (a zero-length one: line_offsets[i + 1] == line_offsets[i])
//   a tracked flow:      ,"_HashId":"<hex>","_RecordType":"flowLog"      in front of the closing brace
// Tracked is conn_tracked (nfagg_flp_line.h): kTrackedOnly has the size kernel measure an untracked flow as 0, and the write
// kernel's window loop already passes over a lane without a line. <hex> is strconv.FormatUint(id, 16). The ids are what nfagg_conn_fold wrote for these records. Device code only.
#pragma once
#include "nfagg_net.h"

namespace nfagg {

constexpr uint32_t kConnMetaLineMax = (sizeof(",\"_HashId\":\"\",\"_RecordType\":\"flowLog\"") - 1) + 16;
static_assert(kConnMetaLineMax == 53, "extract conntrack's two keys");

// strconv.FormatUint(v, 16): lower case, no padding, "0" for 0
template <typename S> NF_DEV void hex_u64(S& s, uint64_t v) {
    const uint32_t nd = v ? (uint32_t)(67 - __clzll((long long)v)) / 4u : 1u;
    if constexpr (is_count<S>::value) s.n += nd;
    else {
#pragma unroll
        for (int k = 15; k >= 0; k--)
            if ((uint32_t)k < nd) s.put(hexc((uint32_t)(v >> (4 * k)) & 15u));
    }
}

// FlpNet<..> with the two keys. The window takes what the longest line leaves of 32 KiB beside the wave's side LDS, as FlpNet
// sizes its own. All three bases leave at least 16 384.
template <typename Base> struct FlpConnMeta : Base {
    static constexpr uint32_t kMaxLine = Base::kMaxLine + kConnMetaLineMax;
    static constexpr uint32_t kWindow = (32768 - Base::kSideLds - (kMaxLine + 15) / 16 * 16) / 16 * 16;
    static constexpr uint32_t kLds = kWindow + (kMaxLine + 15) / 16 * 16;
    static_assert(!Base::kDefers && kLds + Base::kSideLds <= 32768 && kWindow >= 16384, "four waves per compute unit, and a window worth its copy-out");
    static constexpr bool kTrackedOnly = true;
    using Net = Base;             // write loki (nfagg_loki_line.h) fills the layers below, and the id only in a call that has ids
    uint64_t hash_id = 0;

    NF_DEV void load_joins(const FlpJoins& J, uint64_t i) { Base::load_joins(J, i); hash_id = J.hash_ids[i]; }
    template <typename S> NF_DEV void conn_meta(S& s) const {
        lit(s, ",\"_HashId\":\""); hex_u64(s, hash_id); lit(s, "\",\"_RecordType\":\"flowLog\"");
    }
};

}  // namespace nfagg
