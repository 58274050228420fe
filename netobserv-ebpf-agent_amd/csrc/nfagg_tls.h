// nfagg_tls.h — TLSVersion, TLSCipherSuite and TLSGroup of the direct-FLP JSON line (decode_protobuf.go:99-110,
// record.go:240-257), as a feature policy on top of another one. The names come from the caller's table
// (nfagg_tls_names_create): nothing of Go's crypto/tls is restated here. Device code only.
//   TLSVersion      ssl_version != 0:      the name, else 0x%04X; "~ " in front when misc_flags & 1 (MiscFlagsSSLMismatch)
//   TLSCipherSuite  tls_cipher_suite != 0: the name, else 0x%04X
//   TLSGroup        tls_key_share != 0:    the name, else CurveID(%d)
#pragma once
#include "nfagg_flp_line.h"

namespace nfagg {

// What the three keys add to a line at most: the key literals with their value's quotes, the "~ ", three names at the cap
// (both fall-back formats are shorter than a name may be).
constexpr uint32_t kTlsLineMax = (sizeof(",\"TLSCipherSuite\":\"\"") - 1) + (sizeof(",\"TLSGroup\":\"\"") - 1) + (sizeof(",\"TLSVersion\":\"\"") - 1) + 2 +
                                 3 * NFAGG_TLS_NAME_MAX;
static_assert(kTlsLineMax == (20 + 14 + 16 + 2) + 3 * 63 && NFAGG_TLS_NAME_MAX >= sizeof("CurveID(65535)") - 1, "TLS keys");

// Row of (kind, id) in the table, -1 when the kind has no row for the id: the last id <= the one looked for, in
// log2(kTlsMaxRows) = 8 steps.
NF_DEV int tls_find(const TlsDev& t, uint32_t kind, uint32_t id) {
    const uint16_t* a = t.ids + kind * kTlsMaxRows;
    const uint32_t n = t.n[kind];
    uint32_t pos = 0;
#pragma unroll
    for (uint32_t step = kTlsMaxRows / 2; step; step >>= 1)
        if (pos + step < n && a[pos + step] <= id) pos += step;
    return n && a[pos] == id ? (int)(kind * kTlsMaxRows + pos) : -1;
}

NF_DEV uint8_t hexc_upper(uint32_t x) { return (uint8_t)(x < 10 ? '0' + x : 'A' + (x - 10)); }

// The unquoted value of one key. The counting pass reads a row's length byte and nothing else, and forms no digit.
template <uint32_t KIND, typename S> NF_DEV void tls_value(S& s, const TlsDev& t, uint32_t id) {
    const int row = tls_find(t, KIND, id);
    if (row >= 0) {
        const uint8_t* p = t.rows + (size_t)row * kTlsRowBytes;
        const uint32_t len = p[0];                                     // 1..63: the name is row bytes [1, 1 + len)
        if constexpr (is_count<S>::value) s.n += len;
        else {
            for (uint32_t c = 0; c <= len; c += 16) {
                const uint4 v = *reinterpret_cast<const uint4*>(p + c);
                const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int k = 0; k < 16; k++)
                    if (c + k >= 1 && c + k <= len) s.put((uint8_t)(w[k >> 2] >> (8 * (k & 3))));
            }
        }
    } else if constexpr (KIND == NFAGG_TLS_GROUP) {
        lit(s, "CurveID("); dec<5>(s, id); s.put(')');
    } else {
        lit(s, "0x");
        if constexpr (is_count<S>::value) s.n += 4;
        else {
#pragma unroll
            for (int k = 3; k >= 0; k--) s.put(hexc_upper((id >> (4 * k)) & 15u));
        }
    }
}

// Base with the TLS keys: no record is deferred. The window takes what the longest line leaves of 32 KiB beside the wave's
// side LDS; a base without name slots leaves one 16-byte chunk unused.
template <typename Base> struct FlpTls : Base {
    static constexpr bool kDefers = false;
    static constexpr uint32_t kMaxLine = Base::kMaxLine + kTlsLineMax;
    static constexpr uint32_t kSideLds = Base::kSideLds ? Base::kSideLds : 16;
    static constexpr uint32_t kWindow = (32768 - kSideLds - (kMaxLine + 15) / 16 * 16) / 16 * 16;
    static constexpr uint32_t kLds = kWindow + (kMaxLine + 15) / 16 * 16;
    static_assert(kLds + kSideLds <= 32768 && kWindow >= 16384, "four waves per compute unit, and a window worth its copy-out");
    TlsDev tls;                   // the kernels assign it (kDefers == false)

    template <typename S> NF_DEV void tls_names(S& s, const Rec& r) const {
        const uint32_t cipher = r.d[33] >> 16, group = r.d[34] & 0xffffu;   // tls_cipher_suite @134, tls_key_share @136
        if (cipher) { lit(s, ",\"TLSCipherSuite\":\""); tls_value<NFAGG_TLS_CIPHER_SUITE>(s, tls, cipher); s.put('"'); }
        if (group) { lit(s, ",\"TLSGroup\":\""); tls_value<NFAGG_TLS_GROUP>(s, tls, group); s.put('"'); }
    }
    template <typename S> NF_DEV void tls_version(S& s, const Rec& r) const {
        const uint32_t version = r.d[33] & 0xffffu;                         // ssl_version @132, misc_flags @139
        if (!version) return;
        lit(s, ",\"TLSVersion\":\"");
        if ((r.d[34] >> 24) & 1u) lit(s, "~ ");
        tls_value<NFAGG_TLS_VERSION>(s, tls, version);
        s.put('"');
    }
};

}  // namespace nfagg
