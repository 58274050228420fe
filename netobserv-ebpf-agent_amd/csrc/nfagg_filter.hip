// nfagg_filter.hip — the kernels of nfagg_filter_apply and nfagg_gather (nfagg_filter.h).
//   k_filter_eval     one lane per flow, kScanBlock flows per workgroup: the record, the rows and (only if the program names
//                     them) the part fields, then the program. Every lane runs the same op at the same time: the program
//                     counter, the op and the atom are wave-uniform, only the atom's answer differs per lane. The stack is a
//                     64-bit mask, one bit per level, bit 0 the top. It writes keep / rule / the sampling to store and feeds
//                     the keep bit to block_scan.
//   k_filter_compact  one wave per 64 flows: its kept records land in one contiguous range of the output, so the lanes walk
//                     (kept record, 16-byte unit) pairs and every store instruction writes consecutive uint4s.
//   k_gather          dst[j] = src[idx[j]] in 1-, 2-, 4-, 8- or 16-byte units, consecutive lanes on consecutive units.
#include "nfagg_filter.h"

#include "nfagg_encode.h"

namespace nfagg {

static_assert(kFilterScanBlock == kScanBlock, "one scan block");

namespace {

// What a lane holds of its flow beside the record: everything an atom can ask for, loaded once.
struct FilterFlow {
    uint32_t k8s_row[2] = {kK8sNoRow, kK8sNoRow};
    uint32_t label[2] = {kNetNoLabel, kNetNoLabel};
    uint32_t dir = kNetNoDirection;
    uint32_t layer = 2;              // NFAGG_FILTER_DIM_FLOW_LAYER's index: 0 infra, 1 app, 2 no key
    bool has_add = false, has_dns = false, has_drops = false;
    uint64_t rtt = 0, dns_latency = 0;
    int32_t ipsec_ret = 0;
    uint32_t ipsec_enc = 0;
    uint32_t dns_id = 0, dns_flags = 0, dns_errno = 0;
    uint32_t drop_bytes = 0, drop_packets = 0, drop_cause = 0, drop_flags = 0;
    int64_t start_ms = 0, end_ms = 0;
    uint64_t samp = 0;               // Sampling as the rules see it: the record's, then what a keep rule stored; 0: no key
};

// The key `field` of the flow: does it exist, and the int ConvertToInt gives (NUM fields only).
NF_DEV bool field_value(uint32_t field, const Rec& r, const FilterFlow& x, uint32_t flags, bool& numeric, int64_t& v) {
    const uint32_t eth = r.eth(), proto = r.d[9] & 0xffu;
    const bool ip = eth == 0x0800u || eth == 0x86DDu;
    const bool icmp = ip && (proto == 1 || proto == 58), ports = ip && (proto == 6 || proto == 17 || proto == 132);
    numeric = true;
    switch (field) {
    case NFAGG_FILTER_F_ETYPE: v = eth; return true;
    case NFAGG_FILTER_F_BYTES: v = (int64_t)r.bytes(); return r.bytes() != 0;
    case NFAGG_FILTER_F_PACKETS: v = r.packets(); return r.packets() != 0;
    case NFAGG_FILTER_F_SAMPLING: v = (int64_t)x.samp; return x.samp != 0;
    case NFAGG_FILTER_F_PROTO: v = proto; return ip;
    case NFAGG_FILTER_F_DSCP: v = r.dscp(); return ip;
    case NFAGG_FILTER_F_SRC_PORT: v = r.d[8] & 0xffffu; return ports;
    case NFAGG_FILTER_F_DST_PORT: v = r.d[8] >> 16; return ports;
    case NFAGG_FILTER_F_ICMP_TYPE: v = (r.d[9] >> 8) & 0xffu; return icmp;
    case NFAGG_FILTER_F_ICMP_CODE: v = (r.d[9] >> 16) & 0xffu; return icmp;
    case NFAGG_FILTER_F_FLAGS: v = r.flags(); numeric = !(flags & kFilterFlagNames); return ip && proto == 6;
    case NFAGG_FILTER_F_TIME_FLOW_START_MS: v = x.start_ms; return true;
    case NFAGG_FILTER_F_TIME_FLOW_END_MS: v = x.end_ms; return true;
    case NFAGG_FILTER_F_FLOW_DIRECTION: v = x.dir; return x.dir <= 2;
    case NFAGG_FILTER_F_TIME_FLOW_RTT_NS: v = (int64_t)x.rtt; return x.has_add && x.rtt != 0;
    case NFAGG_FILTER_F_DNS_LATENCY_MS: v = (int64_t)x.dns_latency / 1000000ll; return x.has_dns && x.dns_id != 0;
    case NFAGG_FILTER_F_DNS_ID: v = x.dns_id; return x.has_dns && x.dns_id != 0;
    case NFAGG_FILTER_F_DNS_FLAGS: v = x.dns_flags; return x.has_dns && x.dns_id != 0;
    case NFAGG_FILTER_F_DNS_ERRNO: v = x.dns_errno; return x.has_dns && x.dns_errno != 0;
    case NFAGG_FILTER_F_PKT_DROP_BYTES: v = x.drop_bytes; return x.has_drops && x.drop_cause != 0;
    case NFAGG_FILTER_F_PKT_DROP_PACKETS: v = x.drop_packets; return x.has_drops && x.drop_cause != 0;
    case NFAGG_FILTER_F_PKT_DROP_LATEST_FLAGS: v = x.drop_flags; return x.has_drops && x.drop_cause != 0;
    case NFAGG_FILTER_F_IPSEC_RET_CODE: v = x.ipsec_ret; return x.has_add && (x.ipsec_ret != 0 || x.ipsec_enc != 0);
    case NFAGG_FILTER_F_SRC_ADDR: case NFAGG_FILTER_F_DST_ADDR: numeric = false; v = 0; return ip;
    default: numeric = false; v = 0; return true;        // SrcMac, DstMac (create refuses anything else)
    }
}

NF_DEV bool eval_atom(const FilterAtom& a, const uint8_t* __restrict__ truth, const Rec& r, const FilterFlow& x, uint32_t flags) {
    switch (a.kind) {
    case NFAGG_FILTER_ATOM_CONST: return a.a != 0;
    case NFAGG_FILTER_ATOM_PRESENT: { bool num; int64_t v; return field_value(a.a, r, x, flags, num, v); }
    case NFAGG_FILTER_ATOM_NUM: {
        bool num; int64_t v;
        if (!field_value(a.a, r, x, flags, num, v) || !num) return false;
        switch (a.cmp) {
        case NFAGG_FILTER_CMP_EQ: return v == a.value;
        case NFAGG_FILTER_CMP_NE: return v != a.value;
        case NFAGG_FILTER_CMP_LT: return v < a.value;
        case NFAGG_FILTER_CMP_GT: return v > a.value;
        case NFAGG_FILTER_CMP_LE: return v <= a.value;
        default: return v >= a.value;
        }
    }
    case NFAGG_FILTER_ATOM_TABLE: {
        const uint32_t none = a.n_truth - 1;         // create: n_truth >= 1
        uint32_t k;
        switch (a.a) {
        case NFAGG_FILTER_DIM_SRC_K8S_ROW: k = x.k8s_row[0]; break;
        case NFAGG_FILTER_DIM_DST_K8S_ROW: k = x.k8s_row[1]; break;
        case NFAGG_FILTER_DIM_SRC_SUBNET_LABEL: k = x.label[0]; break;
        case NFAGG_FILTER_DIM_DST_SUBNET_LABEL: k = x.label[1]; break;
        case NFAGG_FILTER_DIM_FLOW_LAYER: k = x.layer; break;
        case NFAGG_FILTER_DIM_DNS_RCODE: k = (x.has_dns && x.dns_id != 0) ? (x.dns_flags & 0xFu) : none; break;
        default: k = !x.has_add ? none : x.ipsec_ret != 0 ? 1u : x.ipsec_enc ? 0u : none; break;      // IPSecStatus
        }
        return truth[a.truth_off + (k < none ? k : none)] != 0;     // never beyond the atom's own entries
    }
    case NFAGG_FILTER_ATOM_ADDR: {
        const uint32_t eth = r.eth();
        const bool dst = a.a != 0;                   // selects, not a runtime index into the record's registers
        const uint32_t w0 = dst ? r.d[4] : r.d[0], w1 = dst ? r.d[5] : r.d[1], w2 = dst ? r.d[6] : r.d[2], w3 = dst ? r.d[7] : r.d[3];
        return (eth == 0x0800u || eth == 0x86DDu) && w0 == a.w[0] && w1 == a.w[1] && w2 == a.w[2] && w3 == a.w[3];
    }
    default: {                                       // MAC
        const uint64_t m = a.a ? r.dmac() : r.smac();
        return m == ((uint64_t)a.w[0] | ((uint64_t)(a.w[1] & 0xffffu) << 32));
    }
    }
}

}  // namespace

__global__ __launch_bounds__(kScanBlock) void k_filter_eval(const void* __restrict__ recs, uint64_t n, const FilterProg* __restrict__ prog,
                                                            const uint8_t* __restrict__ truth, PbFeat F, const uint32_t* __restrict__ k8s_rows,
                                                            K8sDev K, const uint2* __restrict__ net_rows, FilterClock clk, uint64_t seed,
                                                            uint64_t first_index, uint8_t* __restrict__ keep, uint8_t* __restrict__ rule,
                                                            uint32_t* __restrict__ samp_out, uint32_t* __restrict__ local_off,
                                                            uint32_t* __restrict__ block_sum, uint32_t* __restrict__ n_deferred) {
    __shared__ uint32_t wave_tot[kScanBlock / 64];
    const uint64_t i = (uint64_t)blockIdx.x * kScanBlock + threadIdx.x;
    uint32_t kept = 0;
    bool deferred = false;
    if (i < n) {
        const uint32_t need = prog->need, flags = prog->flags, n_steps = prog->n_steps, n_keep = prog->n_keep;
        Rec r;
        load_record(recs, i, r);
        FilterFlow x;
        x.samp = r.sampling();
        if (need & kFilterNeedK8s) {
            const uint2 q = reinterpret_cast<const uint2*>(k8s_rows)[i];
            x.k8s_row[0] = q.x; x.k8s_row[1] = q.y;
            if (need & kFilterNeedK8sRow) {          // FlpK8s::load_k8s: app when either side's row has the app flag
                bool app = false;
                if (q.x < K.n_rows) app = app || (reinterpret_cast<const uint4*>(K.rows)[q.x].w & kK8sRowApp);
                if (q.y < K.n_rows) app = app || (reinterpret_cast<const uint4*>(K.rows)[q.y].w & kK8sRowApp);
                x.layer = K.has_layer ? (app ? 1u : 0u) : 2u;
            }
        }
        if (need & kFilterNeedNet) {
            const uint2 q = net_rows[i];
            x.label[0] = q.x & 0xffffu; x.label[1] = q.x >> 16; x.dir = q.y & 0xffu;
        }
        const uint32_t present = F.present ? F.present[i] : 0u;
        if ((need & kFilterNeedAdditional) && F.additional && (present & NFAGG_FEAT_ADDITIONAL)) {
            const uint4 q = reinterpret_cast<const uint4*>(F.additional + i * 32)[1];     // flow_rtt @16, ret @24, encrypted @30
            x.has_add = true;
            x.rtt = (uint64_t)q.x | ((uint64_t)q.y << 32); x.ipsec_ret = (int32_t)q.z; x.ipsec_enc = (q.w >> 16) & 0xffu;
        }
        if ((need & kFilterNeedDns) && F.dns && (present & NFAGG_FEAT_DNS)) {
            const uint4 q = reinterpret_cast<const uint4*>(F.dns + i * 64)[1];            // latency @16, id @24, flags @26, errno @30
            x.has_dns = true;
            x.dns_latency = (uint64_t)q.x | ((uint64_t)q.y << 32); x.dns_id = q.z & 0xffffu; x.dns_flags = q.z >> 16; x.dns_errno = (q.w >> 16) & 0xffu;
        }
        if ((need & kFilterNeedDrops) && F.drops && (present & NFAGG_FEAT_DROPS)) {
            const uint4 q = reinterpret_cast<const uint4*>(F.drops + i * 32)[1];          // bytes @16, packets @18, cause @20, latest_flags @24
            x.has_drops = true;
            x.drop_bytes = q.x & 0xffffu; x.drop_packets = q.x >> 16; x.drop_cause = q.y; x.drop_flags = q.z & 0xffffu;
        }
        if (need & kFilterNeedClock) {
            const TimeParts ts = flow_time(clk.now_sec, clk.now_nsec, clk.mono_now, r.start());
            const TimeParts te = flow_time(clk.now_sec, clk.now_nsec, clk.mono_now, r.end());
            x.start_ms = ts.sec * 1000 + ts.nsec / 1000000; x.end_ms = te.sec * 1000 + te.nsec / 1000000;      // t.UnixMilli()
        }
        bool alive = true, admitted = false, stored = false;
        uint32_t admit = NFAGG_FILTER_NO_RULE, decided = 0;
        for (uint32_t s = 0; s < n_steps; s++) {
            if (s == n_keep && n_keep && !admitted) alive = false;       // transform_filter.go:62-73
            const FilterStep st = prog->steps[s];
            uint64_t stack = 0;
            for (uint32_t pc = st.op_begin; pc < st.op_begin + st.op_count; pc++) {
                const uint32_t op = prog->ops[pc];
                if (op < kFilterMaxAtoms) stack = (stack << 1) | (eval_atom(prog->atoms[op], truth, r, x, flags) ? 1ull : 0ull);
                else if (op == NFAGG_FILTER_OP_NOT) stack ^= 1ull;
                else {
                    const uint64_t a = (stack >> 1) & 1ull, b = stack & 1ull;
                    stack = ((stack >> 2) << 1) | (op == NFAGG_FILTER_OP_AND ? (a & b) : (a | b));
                }
            }
            const bool p = (stack & 1ull) != 0;
            if (st.kind == NFAGG_FILTER_STEP_KEEP) {
                if (!admitted && p && filter_roll(seed, first_index + i, s, st.value)) {       // applyKeepPredicate, 192-206
                    admitted = true; admit = s;
                    if (st.value && (flags & kFilterStore)) { x.samp = (x.samp ? x.samp : 1ull) * st.value; stored = true; }   // storeSampling
                }
            } else if (st.kind == NFAGG_FILTER_STEP_REMOVE) {
                if (p) alive = false;
            } else if (p && !((decided >> st.group) & 1u)) {                                   // sample, 208-215
                decided |= 1u << st.group;
                if (!filter_roll(seed, first_index + i, s, st.value)) alive = false;
            }
        }
        if (n_keep && !admitted) alive = false;                          // a spec of keep rules alone
        kept = alive ? 1u : 0u;
        deferred = alive && stored && x.samp > 0xFFFFFFFFull;
        if (keep) keep[i] = (uint8_t)(alive ? (deferred ? 2 : 1) : 0);
        if (rule) rule[i] = (uint8_t)admit;
        samp_out[i] = (stored && !deferred) ? (uint32_t)x.samp : r.sampling();
    }
    const uint64_t def = __ballot(deferred);
    if ((threadIdx.x & 63) == 0 && def) atomicAdd(n_deferred, (uint32_t)__popcll(def));
    block_scan(kept, i, n, wave_tot, local_off, block_sum);
}

__global__ __launch_bounds__(64) void k_filter_compact(const void* __restrict__ recs, uint64_t n, const uint32_t* __restrict__ samp,
                                                       const uint32_t* __restrict__ local_off, const uint64_t* __restrict__ block_base,
                                                       uint32_t* __restrict__ kept_idx, void* __restrict__ out) {
    __shared__ uint32_t src_lane[64];
    const uint64_t i0 = (uint64_t)blockIdx.x * 64, i = i0 + threadIdx.x;
    // a flow is kept iff the scan moves behind it: its successor's offset, or the block's total for the block's last flow
    const uint64_t base = record_off(block_base, local_off, i0);
    uint64_t mine = 0, next = 0;
    if (i < n) {
        mine = record_off(block_base, local_off, i);
        next = (i + 1 < n && (i + 1) / kScanBlock == i / kScanBlock) ? block_base[i / kScanBlock] + local_off[i + 1] : block_base[i / kScanBlock + 1];
    }
    const bool k = i < n && next != mine;
    const uint32_t rank = (uint32_t)(mine - base);
    if (k) { src_lane[rank] = threadIdx.x; if (kept_idx) kept_idx[mine] = (uint32_t)i; }
    uint32_t cnt = k ? rank + 1 : 0;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { const uint32_t o = __shfl_xor(cnt, d, 64); cnt = o > cnt ? o : cnt; }
    if (!out) return;
    __syncthreads();
    const uint4* in4 = reinterpret_cast<const uint4*>(recs);
    uint4* out4 = reinterpret_cast<uint4*>(out);
    for (uint32_t u = threadIdx.x; u < cnt * 9; u += 64) {
        const uint32_t j = u / 9, c = u - j * 9;
        const uint64_t src = i0 + src_lane[j];
        uint4 v = in4[src * 9 + c];
        if (c == 5) v.w = samp[src];                 // sampling @92: dword 23
        out4[(base + j) * 9 + c] = v;
    }
}

template <typename U>
__global__ __launch_bounds__(256) void k_gather(const U* __restrict__ src, uint64_t n_src, uint32_t per, const uint32_t* __restrict__ idx,
                                                uint64_t units, U* __restrict__ dst) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= units) return;
    const uint64_t j = t / per;
    const uint32_t c = (uint32_t)(t - j * per);
    const uint64_t s = idx[j];
    U v{};
    if (s < n_src) v = src[s * per + c];
    dst[t] = v;
}

hipError_t launch_filter_eval(const void* d_recs, uint64_t n, const FilterProg* d_prog, const uint8_t* d_truth, const PbFeat& F,
                              const uint32_t* d_k8s_rows, const K8sDev& K, const uint2* d_net_rows, const FilterClock& clk, uint64_t seed,
                              uint64_t first_index, uint8_t* d_keep, uint8_t* d_rule, uint32_t* d_samp, uint32_t* d_local_off,
                              uint32_t* d_block_sum, uint64_t* d_block_base, uint32_t* d_n_deferred, hipStream_t s) {
    const uint32_t blocks = (uint32_t)((n + kScanBlock - 1) / kScanBlock);
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_filter_eval, dim3(blocks), dim3(kScanBlock), 0, s, d_recs, n, d_prog, d_truth, F, d_k8s_rows, K, d_net_rows, clk, seed,
                       first_index, d_keep, d_rule, d_samp, d_local_off, d_block_sum, d_n_deferred);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_scan_block_sums(d_block_sum, blocks, d_block_base, s);
}

hipError_t launch_filter_compact(const void* d_recs, uint64_t n, const uint32_t* d_samp, const uint32_t* d_local_off,
                                 const uint64_t* d_block_base, uint32_t* d_kept_idx, void* d_out, hipStream_t s) {
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_filter_compact, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, s, d_recs, n, d_samp, d_local_off, d_block_base, d_kept_idx,
                       d_out);
    return hipGetLastError();
}

hipError_t launch_gather(const void* d_src, uint64_t n_src, uint32_t elem_bytes, uint32_t unit, const uint32_t* d_idx, uint64_t n_kept, void* d_dst,
                         hipStream_t s) {
    const uint32_t per = elem_bytes / unit;
    const uint64_t units = n_kept * per;
    const dim3 grid((unsigned)((units + 255) / 256)), block(256);
    (void)hipGetLastError();
    switch (unit) {
    case 1: hipLaunchKernelGGL(k_gather<uint8_t>, grid, block, 0, s, (const uint8_t*)d_src, n_src, per, d_idx, units, (uint8_t*)d_dst); break;
    case 2: hipLaunchKernelGGL(k_gather<uint16_t>, grid, block, 0, s, (const uint16_t*)d_src, n_src, per, d_idx, units, (uint16_t*)d_dst); break;
    case 4: hipLaunchKernelGGL(k_gather<uint32_t>, grid, block, 0, s, (const uint32_t*)d_src, n_src, per, d_idx, units, (uint32_t*)d_dst); break;
    case 8: hipLaunchKernelGGL(k_gather<uint2>, grid, block, 0, s, (const uint2*)d_src, n_src, per, d_idx, units, (uint2*)d_dst); break;
    default: hipLaunchKernelGGL(k_gather<uint4>, grid, block, 0, s, (const uint4*)d_src, n_src, per, d_idx, units, (uint4*)d_dst); break;
    }
    return hipGetLastError();
}

}  // namespace nfagg
