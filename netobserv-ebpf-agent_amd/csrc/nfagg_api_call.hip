// nfagg_api_call.hip — the host-call vocabulary of nfagg_api_call.h: what is not a template.
#include <hip/hip_runtime.h>
#include <algorithm>

#include "nfagg_api_call.h"

namespace nfagg {

void split_now(int64_t now_unix_ns, int64_t& sec, int64_t& nsec) {
    sec = now_unix_ns / 1000000000ll; nsec = now_unix_ns % 1000000000ll;
    if (nsec < 0) { nsec += 1000000000ll; sec -= 1; }
}

int ipfix_template_message(const IpfixTemplateHeader& hd, std::initializer_list<IpfixFields> fields, IpfixFields enterprise, uint32_t enterprise_id,
                           void* out, size_t cap, size_t* n_out) {
    if (!enterprise_id) enterprise.n = 0;
    uint32_t count = enterprise.n;
    for (const IpfixFields& l : fields) count += l.n;
    const size_t total = 16 + 4 + 4 + 4 * (size_t)count + 4 * (size_t)enterprise.n;
    *n_out = total;
    if (!out || cap < total) return NFAGG_TRUNCATED;
    uint8_t* p = (uint8_t*)out;
    put_be16(p, 10); put_be16(p + 2, (uint32_t)total); put_be32(p + 4, hd.export_time); put_be32(p + 8, hd.seq); put_be32(p + 12, hd.obs_domain);
    put_be16(p + 16, 2); put_be16(p + 18, (uint32_t)total - 16);                              // template set
    put_be16(p + 20, hd.template_id); put_be16(p + 22, count);                                // template record header
    uint8_t* q = p + 24;
    for (const IpfixFields& l : fields)
        for (uint32_t k = 0; k < l.n; k++, q += 4) { put_be16(q, l.f[k][0]); put_be16(q + 2, l.f[k][1]); }
    for (uint32_t k = 0; k < enterprise.n; k++, q += 8) {                                     // entities/record.go:252-265
        put_be16(q, enterprise.f[k][0] | 0x8000u); put_be16(q + 2, enterprise.f[k][1]); put_be32(q + 4, enterprise_id);
    }
    return NFAGG_OK;
}

int check_namer(nfagg_handle* h, const nfagg_intf_name* names, uint32_t n_names, uint32_t unknown_len, bool check_udn) {
    if (unknown_len > 16 || (n_names && !names)) return fail(h, NFAGG_EINVAL, "bad namer table");
    for (uint32_t k = 0; k < n_names; k++) {
        if (names[k].name_len > 16) return fail(h, NFAGG_EINVAL, "namer row %u: name too long", k);
        if (check_udn && names[k].udn_len > 63) return fail(h, NFAGG_EINVAL, "namer row %u: udn too long", k);
    }
    return NFAGG_OK;
}

int stage_namer(nfagg_handle* h, const nfagg_intf_name* names, uint32_t n_names, DevBuf& dst, std::vector<nfagg_intf_name>& host_copy) {
    API_TRY(dst.ensure(h, (size_t)(n_names + 1) * sizeof(nfagg_intf_name)));
    host_copy.assign(names, names + n_names);
    std::stable_sort(host_copy.begin(), host_copy.end(), [](const nfagg_intf_name& a, const nfagg_intf_name& b) { return a.if_index < b.if_index; });
    if (n_names) HIP_TRY(h, hipMemcpyAsync(dst.p, host_copy.data(), n_names * sizeof(nfagg_intf_name), hipMemcpyHostToDevice, h->stream));
    return NFAGG_OK;
}

int ensure_all(nfagg_handle* h, std::initializer_list<BufNeed> need) {
    for (const BufNeed& q : need) API_TRY(q.buf.ensure(h, q.bytes));
    return NFAGG_OK;
}

int stage_in(nfagg_handle* h, DevBuf& buf, const void* src, size_t bytes, size_t slack) {
    API_TRY(buf.ensure(h, bytes + slack));
    if (bytes) HIP_TRY(h, hipMemcpyAsync(buf.p, src, bytes, hipMemcpyHostToDevice, h->stream));
    return NFAGG_OK;
}

int fetch(nfagg_handle* h, void* dst, const DevBuf& buf, size_t bytes) {
    if (bytes) HIP_TRY(h, hipMemcpyAsync(dst, buf.p, bytes, hipMemcpyDeviceToHost, h->stream));
    return NFAGG_OK;
}

int encode_begin(nfagg_handle* h, size_t n, uint64_t* d_offsets, size_t* out_bytes, const nfagg_intf_name* names, uint32_t n_names, bool* done) {
    HIP_TRY(h, hipSetDevice(h->device));
    *out_bytes = 0;
    *done = n == 0;
    if (n == 0) { HIP_TRY(h, hipMemsetAsync(d_offsets, 0, sizeof(uint64_t), h->stream)); HIP_TRY(h, hipStreamSynchronize(h->stream)); return NFAGG_OK; }
    const size_t blocks = (n + 1023) / 1024;
    API_TRY(ensure_all(h, {{h->enc.local_off, n * sizeof(uint32_t)}, {h->enc.block_sum, blocks * sizeof(uint32_t)},
                           {h->enc.block_base, (blocks + 1) * sizeof(uint64_t)}}));
    return stage_namer(h, names, n_names, h->enc.names, h->enc.h_names);
}

}  // namespace nfagg
