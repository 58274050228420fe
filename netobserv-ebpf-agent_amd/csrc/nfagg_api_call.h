// nfagg_api_call.h — what the host entry points of the C ABI do alike, once: the clock and the namer table of a
// call, the scratch a call needs, the two passes of an encoder with the read-back between them, and the host-memory twin of a
// device entry point (stage the inputs, call the device entry point on the staged copies, fetch the outputs, synchronise).
// Every call serialises on h->stream and synchronises before it returns, so the handle's EncodeScratch serves them all.
// The definitions that are not templates are nfagg_api_call.hip's. Private to csrc/.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <initializer_list>
#include <vector>

#include "../../include/nfagg.h"
#include "nfagg_internal.h"
#include "nfagg_handle.h"

#define API_TRY(expr)                                  \
    do {                                               \
        const int rc_ = (expr);                        \
        if (rc_ != NFAGG_OK) return rc_;               \
    } while (0)

namespace nfagg {

// time.Time's (sec, nsec) of now_unix_ns, 0 <= nsec < 1e9
void split_now(int64_t now_unix_ns, int64_t& sec, int64_t& nsec);

inline void put_be16(uint8_t* p, uint32_t v) { p[0] = (uint8_t)(v >> 8); p[1] = (uint8_t)v; }
inline void put_be32(uint8_t* p, uint32_t v) { put_be16(p, v >> 16); put_be16(p + 2, v); }

// An IPFIX template message (RFC 7011 §3.1, §3.4.1): the message header, one template set with one template record, its field
// specifiers (element id, length) list by list, then `enterprise`'s with the enterprise bit and the number; enterprise_id == 0:
// no enterprise part. *n_out is the message's length; NFAGG_TRUNCATED without room for it.
struct IpfixFields { const uint16_t (*f)[2]; uint32_t n; };
struct IpfixTemplateHeader { uint32_t export_time, seq, obs_domain; uint16_t template_id; };
int ipfix_template_message(const IpfixTemplateHeader& hd, std::initializer_list<IpfixFields> fields, IpfixFields enterprise, uint32_t enterprise_id,
                           void* out, size_t cap, size_t* n_out);

// The namer table of a call: its rows checked (check_udn: the formats that print the UDN), then stably sorted by if_index — the
// kernels binary-search it, and the stable sort keeps the scan-in-table-order answer — and uploaded into dst. host_copy is the
// sorted table, kept until the stream has consumed it.
int check_namer(nfagg_handle* h, const nfagg_intf_name* names, uint32_t n_names, uint32_t unknown_len, bool check_udn);
int stage_namer(nfagg_handle* h, const nfagg_intf_name* names, uint32_t n_names, DevBuf& dst, std::vector<nfagg_intf_name>& host_copy);

// Scratch of a call: every buffer at least `bytes` large, or the first one's error. A growth moves the block: take pointers
// from a DevBuf behind the last ensure of it in the call.
struct BufNeed { DevBuf& buf; size_t bytes; };
int ensure_all(nfagg_handle* h, std::initializer_list<BufNeed> need);

// A host array into the handle's staging and back. The kernels read whole 16-byte units past the last element: `slack` bytes
// lie behind the staged ones. bytes == 0: the buffer is there, nothing is copied.
constexpr size_t kStageSlack = 32;
int stage_in(nfagg_handle* h, DevBuf& buf, const void* src, size_t bytes, size_t slack = kStageSlack);
int fetch(nfagg_handle* h, void* dst, const DevBuf& buf, size_t bytes);

// What follows the argument checks of a device entry point: the device, the zeroed results, the answer for n == 0 (*done), the
// scratch of the two scans, the namer table (into h->enc.names).
int encode_begin(nfagg_handle* h, size_t n, uint64_t* d_offsets, size_t* out_bytes, const nfagg_intf_name* names, uint32_t n_names, bool* done);

// The two passes: size(local_off, block_sum, block_base) launches the size kernel and the scan of the block sums; the total is
// read back, and with it `extra` (a counter the size pass left: `bytes` from dev to host, none for bytes == 0) in the same
// synchronisation; a buffer that is too small or absent ends it there, with the total in *out_bytes; write(local_off,
// block_base, total) launches the write kernel. The scan scratch is h->enc's, as encode_begin sized it.
struct PassNames { const char* what; const char* size_verb; const char* write_verb; };      // "<what> <verb> launch failed: .."
struct ReadBack { const void* dev = nullptr; void* host = nullptr; size_t bytes = 0; };
template <typename SizeLaunch, typename WriteLaunch>
int encode_two_pass(nfagg_handle* h, size_t n, const PassNames& names, void* d_out, size_t out_cap, size_t* out_bytes, const ReadBack& extra,
                    SizeLaunch size, WriteLaunch write) {
    auto& S = h->enc;
    const size_t blocks = (n + 1023) / 1024;
    hipError_t e = size(S.local_off.as<uint32_t>(), S.block_sum.as<uint32_t>(), S.block_base.as<uint64_t>());
    if (e != hipSuccess) return fail(h, NFAGG_EDEVICE, "%s %s launch failed: %s", names.what, names.size_verb, hipGetErrorString(e));
    uint64_t total = 0;
    HIP_TRY(h, hipMemcpyAsync(&total, S.block_base.as<uint64_t>() + blocks, sizeof total, hipMemcpyDeviceToHost, h->stream));
    if (extra.bytes) HIP_TRY(h, hipMemcpyAsync(extra.host, extra.dev, extra.bytes, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    *out_bytes = (size_t)total;
    if (total > out_cap || !d_out) return NFAGG_TRUNCATED;
    e = write(S.local_off.as<const uint32_t>(), S.block_base.as<const uint64_t>(), total);
    if (e != hipSuccess) return fail(h, NFAGG_EDEVICE, "%s %s launch failed: %s", names.what, names.write_verb, hipGetErrorString(e));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return NFAGG_OK;
}

// The host-memory twin of an encoder: records in, device(d_records, d_out or null, d_offsets) = the device entry point (it
// stages what else the format takes first), bytes and offsets out, and the format's per-record extras (out_extra[k] -> host,
// `bytes` per record; skipped when the caller passed no host array). Anything but NFAGG_OK from the device entry point ends the
// call there: none of the caller's arrays is written.
struct EncodeExtra { void* host; size_t bytes; };
template <typename DeviceEntry>
int encode_staged(nfagg_handle* h, const void* records, size_t n, void* out, size_t out_cap, uint64_t* offsets, size_t* out_bytes,
                  std::initializer_list<EncodeExtra> extras, DeviceEntry device) {
    auto& S = h->enc;
    HIP_TRY(h, hipSetDevice(h->device));
    API_TRY(ensure_all(h, {{S.in_records, n * kRecordBytes + kStageSlack}, {S.out, out_cap + kStageSlack}, {S.out_offsets, (n + 1) * sizeof(uint64_t)}}));
    size_t k = 0;
    for (const EncodeExtra& x : extras) { if (x.host) API_TRY(S.out_extra[k].ensure(h, n * x.bytes + kStageSlack)); k++; }
    API_TRY(stage_in(h, S.in_records, records, n * kRecordBytes));
    API_TRY(device(S.in_records.p, out ? S.out.p : nullptr, S.out_offsets.as<uint64_t>()));
    API_TRY(fetch(h, out, S.out, *out_bytes));
    API_TRY(fetch(h, offsets, S.out_offsets, (n + 1) * sizeof(uint64_t)));
    k = 0;
    for (const EncodeExtra& x : extras) { if (x.host) API_TRY(fetch(h, x.host, S.out_extra[k], n * x.bytes)); k++; }
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return NFAGG_OK;
}

}  // namespace nfagg
