// nfagg_api_tables.hip — the caller tables of the C ABI (include/nfagg.h): network events, TLS names, Kubernetes, subnets and
// direction, metrics. Each is checked, rendered and laid out on the host and (with a handle) uploaded; the resolve kernels and the
// metrics fold run over them alone, the direct-FLP encoders (nfagg_api_export.hip) read them through nfagg_api_tables.h.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <map>
#include <new>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/nfagg.h"
#include "nfagg_internal.h"
#include "nfagg_handle.h"
#include "nfagg_api_call.h"
#include "nfagg_api_tables.h"
#include "nfagg_flp.h"
#include "nfagg_netev.h"
#include "nfagg_metrics.h"
#include "nfagg_flp_names.h"

using namespace nfagg;

namespace {

// net.IP.String() of a 16-byte address, as ip_text (nfagg_flp_line.h) prints AgentIP on the device: the dotted quad for a
// v4-mapped one, else netip's appendTo6.
std::string go_ip_text(const uint8_t ip[16]) {
    static const uint8_t v4[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0xff, 0xff};
    char buf[48];
    if (memcmp(ip, v4, 12) == 0) { snprintf(buf, sizeof buf, "%u.%u.%u.%u", ip[12], ip[13], ip[14], ip[15]); return buf; }
    uint32_t g[8];
    for (int k = 0; k < 8; k++) g[k] = ((uint32_t)ip[2 * k] << 8) | ip[2 * k + 1];
    int z0 = -1, zlen = 1, cur = 0, curlen = 0;                          // only runs of two or more zero groups count; the first longest wins
    for (int k = 0; k < 8; k++) {
        if (g[k] == 0) { if (curlen == 0) cur = k; curlen++; if (curlen > zlen) { z0 = cur; zlen = curlen; } }
        else curlen = 0;
    }
    const int z1 = z0 < 0 ? -1 : z0 + zlen;
    std::string o;
    for (int k = 0; k < 8; k++) {
        if (k == z0) o += "::";
        else if (k < z0 || k >= z1) {
            if (k > 0 && k != z1) o += ':';
            snprintf(buf, sizeof buf, "%x", g[k]);
            o += buf;
        }
    }
    return o;
}

}  // namespace

// ---- what the encoders' host side (nfagg_api_export.hip) shares with the tables: declared in nfagg_api_tables.h
namespace nfagg {

// jsoniter's Stream.WriteString without HTML escaping (stream_str.go:311-372): the quotes, \" \\ \n \r \t, any other byte
// below 0x20 as \u00xx in lower-case hex, every other byte (0x7f and everything from 0x80 up) as it is. Returns the length.
uint32_t flp_escape(const char* src, uint32_t len, uint8_t* dst) {
    static const char hex[] = "0123456789abcdef";
    uint32_t o = 0;
    dst[o++] = '"';
    for (uint32_t k = 0; k < len; k++) {
        const uint8_t b = (uint8_t)src[k];
        if (b == '"' || b == '\\') { dst[o++] = '\\'; dst[o++] = b; }
        else if (b == '\n') { dst[o++] = '\\'; dst[o++] = 'n'; }
        else if (b == '\r') { dst[o++] = '\\'; dst[o++] = 'r'; }
        else if (b == '\t') { dst[o++] = '\\'; dst[o++] = 't'; }
        else if (b < 0x20) { memcpy(dst + o, "\\u00", 4); o += 4; dst[o++] = (uint8_t)hex[b >> 4]; dst[o++] = (uint8_t)hex[b & 15]; }
        else dst[o++] = b;
    }
    dst[o++] = '"';
    return o;
}

NetDev net_dev(const nfagg_net_table* t) {
    const uint8_t* m = t->d_mem.as<const uint8_t>();
    return NetDev{(const NetCidr*)m, (const uint32_t*)(m + t->off_meta), (const NetFrag*)(m + t->off_frags), m + t->off_blob,
                  (uint32_t)t->cidrs.size(), (uint32_t)t->frags.size(), t->flags};
}

K8sDev k8s_dev(const nfagg_k8s_table* t) {
    return K8sDev{t->d_slots.as<const K8sSlot>(), t->d_rows.as<const K8sRow>(), t->d_blob.as<const uint8_t>(), (uint32_t)t->slots.size() - 1,
                  (uint32_t)t->rows.size(), t->has_layer ? 1u : 0u};
}

// The reporter of a call: the id of AgentIP's text among the table's host IPs, kNetNoHost when no row carries that text
// (transform_network_direction.go:37-44; "<nil>" is not empty, so the rule goes on).
uint32_t net_reporter(const nfagg_k8s_table* k8s, const nfagg_flp_options* opt) {
    const auto it = k8s->host_text.find(opt->agent_ip_nil ? std::string("<nil>") : go_ip_text(opt->agent_ip));
    return it == k8s->host_text.end() ? kNetNoHost : it->second;
}

}  // namespace nfagg

// ---- network events: the cookie table and the resolve kernel (nfagg_netev.hip)
namespace {

struct NetevStr { const char* p; uint32_t len; };
// networkevents.ToMap (network_events.go:38-52), keys in byte order. Returns the number of pairs, 0 for an undecodable entry.
int netev_pairs(const nfagg_netev_entry& e, const char* (&keys)[6], NetevStr (&vals)[6]) {
    if (e.kind == NFAGG_NETEV_ACL) {
        static const char* const k[6] = {"Action", "Direction", "Feature", "Name", "Namespace", "Type"};
        const NetevStr v[6] = {{e.action, e.action_len}, {e.direction, e.direction_len}, {"acl", 3}, {e.name, e.name_len},
                               {e.namespace_, e.namespace_len}, {e.actor, e.actor_len}};
        for (int q = 0; q < 6; q++) { keys[q] = k[q]; vals[q] = v[q]; }
        return 6;
    }
    if (e.kind == NFAGG_NETEV_OTHER) { keys[0] = "Message"; vals[0] = {e.string, e.string_len}; return 1; }
    return 0;
}

bool netev_strings_ok(const nfagg_netev_entry& e) {
    const NetevStr v[6] = {{e.action, e.action_len}, {e.actor, e.actor_len}, {e.name, e.name_len}, {e.namespace_, e.namespace_len},
                           {e.direction, e.direction_len}, {e.string, e.string_len}};
    for (int q = e.kind == NFAGG_NETEV_ACL ? 0 : 5; q < 6; q++)
        if (v[q].len && !v[q].p) return false;
    return true;
}

void put_varint_host(std::vector<uint8_t>& o, uint64_t v) {
    while (v >= 0x80) { o.push_back((uint8_t)(v | 0x80)); v >>= 7; }
    o.push_back((uint8_t)v);
}

// The rendered bytes of one entry. false: an undecodable entry, or a string so long that the rendering cannot fit the cap
// (checked before anything of that size is built).
bool netev_render(const nfagg_netev_entry& e, int format, std::vector<uint8_t>& o) {
    const char* keys[6]; NetevStr vals[6];
    const int np = netev_pairs(e, keys, vals);
    o.clear();
    if (!np) return false;
    for (int q = 0; q < np; q++) if (vals[q].len > kNetevMaxRendered) return false;
    if (format == NFAGG_NETEV_JSON) {
        uint8_t buf[2 + 6 * kNetevMaxRendered];
        o.push_back('{');
        for (int q = 0; q < np; q++) {
            if (q) o.push_back(',');
            o.push_back('"'); o.insert(o.end(), keys[q], keys[q] + strlen(keys[q])); o.push_back('"'); o.push_back(':');
            const uint32_t n = flp_escape(vals[q].p, vals[q].len, buf);
            o.insert(o.end(), buf, buf + n);
        }
        o.push_back('}');
    } else {
        for (int q = 0; q < np; q++) {                       // map entry: key = 1, value = 2, both written even when empty
            const size_t kl = strlen(keys[q]);
            std::vector<uint8_t> ent;
            ent.push_back(0x0A); put_varint_host(ent, kl); ent.insert(ent.end(), keys[q], keys[q] + kl);
            ent.push_back(0x12); put_varint_host(ent, vals[q].len); ent.insert(ent.end(), vals[q].p, vals[q].p + vals[q].len);
            o.push_back(0x0A); put_varint_host(o, ent.size()); o.insert(o.end(), ent.begin(), ent.end());
        }
    }
    return true;
}

uint32_t netev_cause(const nfagg_netev_entry& e) {          // networkevents.ToDropReasonCode (network_events.go:121-131)
    static const char* const causes[10] = {"Unknown", "EgressFirewall", "AdminNetworkPolicy", "BaselineAdminNetworkPolicy", "NetworkPolicy",
                                           "MulticastNS", "MulticastCluster", "NetpolNode", "NetpolNamespace", "UDNIsolation"};
    if (e.kind != NFAGG_NETEV_ACL || e.action_len != 4 || memcmp(e.action, "drop", 4) != 0) return 0;
    for (uint32_t q = 0; q < 10; q++)
        if (strlen(causes[q]) == e.actor_len && memcmp(causes[q], e.actor, e.actor_len) == 0) return (1u << 24) + q;
    return 1u << 24;
}

uint64_t netev_cookie(const uint8_t* c) { uint64_t v; memcpy(&v, c, 8); return v; }

}  // namespace

extern "C" {

int nfagg_netev_render(const nfagg_netev_entry* entry, int format, void* out, size_t cap, size_t* n_out) {
    if (!entry || !n_out) return fail(nullptr, NFAGG_EINVAL, "null argument");
    if (format != NFAGG_NETEV_JSON && format != NFAGG_NETEV_PB) return fail(nullptr, NFAGG_EINVAL, "unknown format %d", format);
    if (entry->kind > NFAGG_NETEV_UNDECODABLE || !netev_strings_ok(*entry)) return fail(nullptr, NFAGG_EINVAL, "bad network-events entry");
    std::vector<uint8_t> o;
    if (!netev_render(*entry, format, o)) {
        if (entry->kind == NFAGG_NETEV_UNDECODABLE) return fail(nullptr, NFAGG_EINVAL, "an undecodable entry renders to nothing");
        return fail(nullptr, NFAGG_EINVAL, "rendered event exceeds %u bytes", kNetevMaxRendered);
    }
    if (o.size() > kNetevMaxRendered) return fail(nullptr, NFAGG_EINVAL, "rendered event has %zu bytes, more than %u", o.size(), kNetevMaxRendered);
    *n_out = o.size();
    if (!out || cap < o.size()) return NFAGG_TRUNCATED;
    memcpy(out, o.data(), o.size());
    return NFAGG_OK;
}

int nfagg_netev_table_create(nfagg_handle* h, const nfagg_netev_entry* entries, size_t n, nfagg_netev_table** table) {
    if (!table || (n && !entries)) return fail(h, NFAGG_EINVAL, "null argument");
    *table = nullptr;
    if (n > NFAGG_NETEV_MAX_ROWS) return fail(h, NFAGG_EINVAL, "%zu network-events entries, more than %d", n, NFAGG_NETEV_MAX_ROWS);
    std::vector<uint32_t> order(n);
    for (size_t k = 0; k < n; k++) {
        order[k] = (uint32_t)k;
        if (entries[k].kind > NFAGG_NETEV_UNDECODABLE) return fail(h, NFAGG_EINVAL, "network-events entry %zu: unknown kind %u", k, entries[k].kind);
        if (!netev_strings_ok(entries[k])) return fail(h, NFAGG_EINVAL, "network-events entry %zu: null string with a length", k);
    }
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return netev_cookie(entries[a].cookie) < netev_cookie(entries[b].cookie); });
    for (size_t r = 1; r < n; r++)
        if (netev_cookie(entries[order[r]].cookie) == netev_cookie(entries[order[r - 1]].cookie))
            return fail(h, NFAGG_EINVAL, "network-events entries %u and %u carry the same cookie", std::min(order[r - 1], order[r]), std::max(order[r - 1], order[r]));
    nfagg_netev_table* t = new (std::nothrow) nfagg_netev_table;
    if (!t) return fail(h, NFAGG_ENOMEM, "out of memory");
    t->h = h;
    t->rows.resize(n);
    std::vector<uint8_t> piece;
    for (size_t r = 0; r < n; r++) {
        const nfagg_netev_entry& e = entries[order[r]];
        NetevRow& row = t->rows[r];
        row = NetevRow{};
        row.cookie = netev_cookie(e.cookie);
        row.kind = (uint16_t)e.kind;
        row.cls = (uint16_t)kNetevNoRow;
        if (e.kind == NFAGG_NETEV_UNDECODABLE) continue;
        row.cause = netev_cause(e);
        row.cls = (uint16_t)r;                                      // the first row with the same String() bytes
        for (size_t q = 0; q < r; q++) {
            const nfagg_netev_entry& f = entries[order[q]];
            if (f.kind != NFAGG_NETEV_UNDECODABLE && f.string_len == e.string_len && (e.string_len == 0 || memcmp(f.string, e.string, e.string_len) == 0)) {
                row.cls = (uint16_t)q;
                break;
            }
        }
        for (int format : {NFAGG_NETEV_JSON, NFAGG_NETEV_PB}) {
            if (!netev_render(e, format, piece) || piece.size() > kNetevMaxRendered) {
                const size_t got = piece.size();
                delete t;
                return fail(h, NFAGG_EINVAL, "network-events entry %u: its %s rendering has %s%zu bytes, the cap is %u", order[r],
                            format == NFAGG_NETEV_JSON ? "JSON" : "protobuf", got ? "" : "more than ", got ? got : (size_t)kNetevMaxRendered, kNetevMaxRendered);
            }
            const uint32_t off = (uint32_t)t->blob.size();
            t->blob.insert(t->blob.end(), piece.begin(), piece.end());
            t->blob.resize((t->blob.size() + 15) / 16 * 16, 0);      // the kernels read a piece 16 bytes at a time
            if (format == NFAGG_NETEV_JSON) { row.json_off = off; row.json_len = (uint16_t)piece.size(); }
            else { row.pb_off = off; row.pb_len = (uint16_t)piece.size(); }
        }
    }
    if (h) {
        auto up = [&]() -> int {
            HIP_TRY(h, hipSetDevice(h->device));
            HIP_TRY(h, t->d_rows.alloc(std::max<size_t>(n, 1) * sizeof(NetevRow)));
            HIP_TRY(h, t->d_blob.alloc(std::max<size_t>(t->blob.size(), 16)));
            if (n) HIP_TRY(h, hipMemcpy(t->d_rows.p, t->rows.data(), n * sizeof(NetevRow), hipMemcpyHostToDevice));
            if (!t->blob.empty()) HIP_TRY(h, hipMemcpy(t->d_blob.p, t->blob.data(), t->blob.size(), hipMemcpyHostToDevice));
            return NFAGG_OK;
        };
        const int rc = up();
        if (rc != NFAGG_OK) { nfagg_netev_table_destroy(t); return rc; }
    }
    *table = t;
    return NFAGG_OK;
}

void nfagg_netev_table_destroy(nfagg_netev_table* t) { destroy_on_handle(t); }

int nfagg_netev_resolve_device(nfagg_handle* h, const nfagg_netev_table* table, const uint8_t* d_present,
                               const nfagg_network_events_metrics* d_network_events, const nfagg_pkt_drop_metrics* d_drops, size_t n,
                               uint8_t* d_present_out, nfagg_pkt_drop_metrics* d_drops_out, uint16_t* d_rows_out,
                               uint64_t* d_missing_set, size_t missing_cap, size_t* n_missing, int* zero_missing, int* overflow) {
    if (!h || !table || !n_missing || !zero_missing || !overflow || (missing_cap && !d_missing_set) ||
        (n && (!d_present || !d_present_out || !d_drops_out || !d_rows_out)))
        return fail(h, NFAGG_EINVAL, "null argument");
    if (table->h != h || !table->d_rows) return fail(h, NFAGG_EINVAL, "the network-events table was not created for this handle");
    if ((((uintptr_t)d_network_events | (uintptr_t)d_drops | (uintptr_t)d_drops_out | (uintptr_t)d_rows_out | (uintptr_t)d_missing_set) & 7u) != 0)
        return fail(h, NFAGG_EINVAL, "device arrays must be 8-byte aligned");
    if (missing_cap > 0xffffffffull) return fail(h, NFAGG_EINVAL, "missing_cap too large");
    *n_missing = 0; *zero_missing = 0; *overflow = 0;
    HIP_TRY(h, hipSetDevice(h->device));
    API_TRY(h->enc.ne_info.ensure(h, 16));
    HIP_TRY(h, hipMemsetAsync(h->enc.ne_info.p, 0, 16, h->stream));
    if (missing_cap) HIP_TRY(h, hipMemsetAsync(d_missing_set, 0, missing_cap * sizeof(uint64_t), h->stream));
    if (n) {
        hipError_t e = launch_netev_resolve(d_present, (const uint8_t*)d_network_events, (const uint8_t*)d_drops, n, table->d_rows.as<const NetevRow>(),
                                            (uint32_t)table->rows.size(), d_present_out, (uint8_t*)d_drops_out, d_rows_out, d_missing_set,
                                            (uint32_t)missing_cap, h->enc.ne_info.as<uint32_t>(), h->stream);
        if (e != hipSuccess) return fail(h, NFAGG_EDEVICE, "network-events resolve launch failed: %s", hipGetErrorString(e));
    }
    uint32_t info[4] = {};
    HIP_TRY(h, hipMemcpyAsync(info, h->enc.ne_info.p, sizeof info, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    *n_missing = info[0]; *overflow = info[1] ? 1 : 0; *zero_missing = info[2] ? 1 : 0;
    return NFAGG_OK;
}

int nfagg_netev_resolve(nfagg_handle* h, const nfagg_netev_table* table, const uint8_t* present,
                        const nfagg_network_events_metrics* network_events, const nfagg_pkt_drop_metrics* drops, size_t n,
                        uint8_t* present_out, nfagg_pkt_drop_metrics* drops_out, uint16_t* rows_out,
                        uint8_t (*missing)[8], size_t missing_cap, size_t* n_missing, int* overflow) {
    if (!h || !table || !n_missing || !overflow || (missing_cap && !missing) || (n && (!present || !present_out || !drops_out || !rows_out)))
        return fail(h, NFAGG_EINVAL, "null argument");
    auto& S = h->enc;
    HIP_TRY(h, hipSetDevice(h->device));
    const void* src[3] = {present, network_events, drops};
    const size_t elem[3] = {1, sizeof(nfagg_network_events_metrics), sizeof(nfagg_pkt_drop_metrics)}, out_elem[3] = {1, sizeof(nfagg_pkt_drop_metrics), 8};
    for (int k = 0; k < 3; k++) {
        API_TRY(S.ne_out[k].ensure(h, n * out_elem[k] + kStageSlack));
        if (src[k] && n) API_TRY(stage_in(h, S.ne_in[k], src[k], n * elem[k]));
    }
    API_TRY(S.ne_missing.ensure(h, missing_cap * sizeof(uint64_t) + kStageSlack));
    size_t stored = 0; int zero = 0;
    API_TRY(nfagg_netev_resolve_device(h, table, S.ne_in[0].as<const uint8_t>(), network_events ? S.ne_in[1].as<const nfagg_network_events_metrics>() : nullptr,
                                    drops ? S.ne_in[2].as<const nfagg_pkt_drop_metrics>() : nullptr, n, S.ne_out[0].as<uint8_t>(),
                                    S.ne_out[1].as<nfagg_pkt_drop_metrics>(), S.ne_out[2].as<uint16_t>(), missing_cap ? S.ne_missing.as<uint64_t>() : nullptr,
                                    missing_cap, &stored, &zero, overflow));
    void* dst[3] = {present_out, drops_out, rows_out};
    for (int k = 0; k < 3; k++) API_TRY(fetch(h, dst[k], S.ne_out[k], n * out_elem[k]));
    std::vector<uint64_t> set(missing_cap);
    API_TRY(fetch(h, set.data(), S.ne_missing, missing_cap * sizeof(uint64_t)));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    size_t m = 0;
    for (uint64_t v : set) if (v) memcpy(missing[m++], &v, 8);
    if (zero) { if (m < missing_cap) memset(missing[m++], 0, 8); else *overflow = 1; }    // the all-zero cookie takes a place of the list like any other
    *n_missing = m;
    return NFAGG_OK;
}

}  // extern "C"

// ---- TLS names: the caller's table (nfagg_tls.h)
extern "C" {

int nfagg_tls_names_create(nfagg_handle* h, const nfagg_tls_name_entry* entries, size_t n, nfagg_tls_names** table) {
    if (!table || (n && !entries)) return fail(h, NFAGG_EINVAL, "null argument");
    *table = nullptr;
    size_t count[kTlsKinds] = {};
    std::vector<uint32_t> order(n);
    for (size_t k = 0; k < n; k++) {
        const nfagg_tls_name_entry& e = entries[k];
        order[k] = (uint32_t)k;
        if (e.kind >= kTlsKinds) return fail(h, NFAGG_EINVAL, "TLS name entry %zu: unknown kind %u", k, (unsigned)e.kind);
        if (e.name_len == 0 || !e.name) return fail(h, NFAGG_EINVAL, "TLS name entry %zu: empty name", k);
        if (e.name_len > NFAGG_TLS_NAME_MAX) return fail(h, NFAGG_EINVAL, "TLS name entry %zu: a name of %u bytes, the cap is %d", k, e.name_len, NFAGG_TLS_NAME_MAX);
        for (uint32_t b = 0; b < e.name_len; b++) {
            const uint8_t c = (uint8_t)e.name[b];
            if (c < 0x20 || c == '"' || c == '\\') return fail(h, NFAGG_EINVAL, "TLS name entry %zu: byte 0x%02x at %u would need escaping", k, c, b);
        }
        if (++count[e.kind] > kTlsMaxRows) return fail(h, NFAGG_EINVAL, "TLS name entry %zu: more than %u rows of kind %u", k, kTlsMaxRows, (unsigned)e.kind);
    }
    auto key = [&](uint32_t k) { return ((uint32_t)entries[k].kind << 16) | entries[k].id; };
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return key(a) != key(b) ? key(a) < key(b) : a < b; });
    for (size_t r = 1; r < n; r++)
        if (key(order[r]) == key(order[r - 1]))
            return fail(h, NFAGG_EINVAL, "TLS name entries %u and %u carry the same kind %u and id 0x%04x", order[r - 1], order[r],
                        (unsigned)entries[order[r]].kind, (unsigned)entries[order[r]].id);
    nfagg_tls_names* t = new (std::nothrow) nfagg_tls_names;
    if (!t) return fail(h, NFAGG_ENOMEM, "out of memory");
    t->h = h;
    for (size_t r = 0; r < n; r++) {
        const nfagg_tls_name_entry& e = entries[order[r]];
        const size_t slot = (size_t)e.kind * kTlsMaxRows + t->n[e.kind]++;
        t->ids[slot] = e.id;
        uint8_t* row = t->rows.data() + slot * kTlsRowBytes;
        row[0] = (uint8_t)e.name_len;
        memcpy(row + 1, e.name, e.name_len);
    }
    if (h) {
        const size_t id_bytes = t->ids.size() * sizeof(uint16_t);
        static_assert(kTlsKinds * kTlsMaxRows * sizeof(uint16_t) % 16 == 0, "the rows start 16-byte aligned");
        auto up = [&]() -> int {
            HIP_TRY(h, hipSetDevice(h->device));
            HIP_TRY(h, t->d_mem.alloc(id_bytes + t->rows.size()));
            HIP_TRY(h, hipMemcpy(t->d_mem.p, t->ids.data(), id_bytes, hipMemcpyHostToDevice));
            HIP_TRY(h, hipMemcpy(t->d_mem.as<uint8_t>() + id_bytes, t->rows.data(), t->rows.size(), hipMemcpyHostToDevice));
            return NFAGG_OK;
        };
        const int rc = up();
        if (rc != NFAGG_OK) { nfagg_tls_names_destroy(t); return rc; }
    }
    *table = t;
    return NFAGG_OK;
}

void nfagg_tls_names_destroy(nfagg_tls_names* t) { destroy_on_handle(t); }

int nfagg_tls_names_render(const nfagg_tls_names* t, int kind, uint16_t id, int mismatch, void* out, size_t cap, size_t* n_out) {
    if (!t || !n_out) return fail(nullptr, NFAGG_EINVAL, "null argument");
    if (kind < 0 || kind >= (int)kTlsKinds) return fail(nullptr, NFAGG_EINVAL, "unknown kind %d", kind);
    char buf[2 + NFAGG_TLS_NAME_MAX + 1];
    size_t len = 0;
    if (kind == NFAGG_TLS_VERSION && mismatch) { buf[0] = '~'; buf[1] = ' '; len = 2; }
    const uint16_t* ids = t->ids.data() + (size_t)kind * kTlsMaxRows;
    const uint16_t* hit = std::lower_bound(ids, ids + t->n[kind], id);
    if (hit != ids + t->n[kind] && *hit == id) {
        const uint8_t* row = t->rows.data() + ((size_t)kind * kTlsMaxRows + (size_t)(hit - ids)) * kTlsRowBytes;
        memcpy(buf + len, row + 1, row[0]);
        len += row[0];
    } else {
        len += (size_t)snprintf(buf + len, sizeof buf - len, kind == NFAGG_TLS_GROUP ? "CurveID(%u)" : "0x%04X", (unsigned)id);
    }
    *n_out = len;
    if (!out || cap < len) return NFAGG_TRUNCATED;
    memcpy(out, buf, len);
    return NFAGG_OK;
}

}  // extern "C"

// ---- Kubernetes enrichment: the caller's table (nfagg_k8s.h) and the hash join alone
namespace {

struct K8sStr { const char* p; uint32_t len; };

// One side's block. false: a null string with a length (*bad_string), or a value so long that the block cannot fit the cap
// (checked before anything of that size is built).
bool k8s_render(const nfagg_k8s_entry& e, int side, std::vector<uint8_t>& o, bool* bad_string) {
    // enrich.go:51-87 in the byte order of the keys (transform_network.go:153-162)
    const bool host_ip = e.host_ip_len != 0;
    const struct { const char* key; K8sStr v; bool on; } kv[9] = {
        {"HostIP", {e.host_ip, e.host_ip_len}, host_ip}, {"HostName", {e.host_name, e.host_name_len}, host_ip && e.host_name_len != 0},
        {"Name", {e.name, e.name_len}, true}, {"Namespace", {e.namespace_, e.namespace_len}, e.namespace_len != 0},
        {"NetworkName", {e.network_name, e.network_name_len}, true}, {"OwnerName", {e.owner_name, e.owner_name_len}, true},
        {"OwnerType", {e.owner_kind, e.owner_kind_len}, true}, {"Type", {e.kind, e.kind_len}, true},
        {"Zone", {e.zone, e.has_zone ? e.zone_len : 0u}, e.has_zone != 0}};
    o.clear();
    *bad_string = false;
    for (const auto& q : kv) if (q.v.len && !q.v.p) { *bad_string = true; return false; }
    for (const auto& q : kv) if (q.on && q.v.len > kK8sMaxRendered) return false;
    uint8_t buf[2 + 6 * kK8sMaxRendered];
    for (const auto& q : kv) {
        if (!q.on) continue;
        const char* head = side ? ",\"DstK8S_" : ",\"SrcK8S_";
        o.insert(o.end(), head, head + 9);
        o.insert(o.end(), q.key, q.key + strlen(q.key));
        o.push_back('"'); o.push_back(':');
        const uint32_t n = flp_escape(q.v.p, q.v.len, buf);
        o.insert(o.end(), buf, buf + n);
    }
    return true;
}

// enrich.go:143-165 for one row: EnrichLayer asks only about a side whose namespace is not empty
bool k8s_is_app(const nfagg_k8s_entry& e, const nfagg_k8s_layer& l) {
    if (!e.namespace_len) return false;
    for (uint32_t k = 0; k < l.n_prefixes; k++) {
        const size_t pl = strlen(l.infra_prefixes[k]);
        if (pl <= e.namespace_len && memcmp(e.namespace_, l.infra_prefixes[k], pl) == 0) return false;
    }
    for (uint32_t k = 0; k < l.n_refs; k++) {
        const char *ns = l.infra_refs[2 * k], *nm = l.infra_refs[2 * k + 1];
        if (strlen(ns) == e.namespace_len && memcmp(ns, e.namespace_, e.namespace_len) == 0 && strlen(nm) == e.name_len &&
            (e.name_len == 0 || memcmp(nm, e.name, e.name_len) == 0))
            return false;
    }
    return true;
}

}  // namespace

extern "C" {

int nfagg_k8s_render(const nfagg_k8s_entry* entry, int side, void* out, size_t cap, size_t* n_out) {
    if (!entry || !n_out) return fail(nullptr, NFAGG_EINVAL, "null argument");
    if (side != 0 && side != 1) return fail(nullptr, NFAGG_EINVAL, "unknown side %d", side);
    std::vector<uint8_t> o;
    bool bad_string;
    if (!k8s_render(*entry, side, o, &bad_string))
        return bad_string ? fail(nullptr, NFAGG_EINVAL, "null string with a length") : fail(nullptr, NFAGG_EINVAL, "rendered block exceeds %u bytes", kK8sMaxRendered);
    if (o.size() > kK8sMaxRendered) return fail(nullptr, NFAGG_EINVAL, "rendered block has %zu bytes, more than %u", o.size(), kK8sMaxRendered);
    *n_out = o.size();
    if (!out || cap < o.size()) return NFAGG_TRUNCATED;
    memcpy(out, o.data(), o.size());
    return NFAGG_OK;
}

int nfagg_k8s_table_create(nfagg_handle* h, const nfagg_k8s_entry* entries, size_t n, const nfagg_k8s_layer* layer, nfagg_k8s_table** table) {
    if (!table || (n && !entries)) return fail(h, NFAGG_EINVAL, "null argument");
    *table = nullptr;
    if (layer) {
        if (layer->struct_size != sizeof(nfagg_k8s_layer)) return fail(h, NFAGG_EINVAL, "nfagg_k8s_layer.struct_size mismatch");
        if ((layer->n_prefixes && !layer->infra_prefixes) || (layer->n_refs && !layer->infra_refs)) return fail(h, NFAGG_EINVAL, "null layer list with a count");
        for (uint32_t k = 0; k < layer->n_prefixes; k++) if (!layer->infra_prefixes[k]) return fail(h, NFAGG_EINVAL, "layer prefix %u is null", k);
        for (uint32_t k = 0; k < 2 * layer->n_refs; k++) if (!layer->infra_refs[k]) return fail(h, NFAGG_EINVAL, "layer ref %u is null", k / 2);
    }
    if (n > NFAGG_K8S_MAX_ROWS) return fail(h, NFAGG_EINVAL, "%zu Kubernetes entries, more than %u", n, NFAGG_K8S_MAX_ROWS);
    nfagg_k8s_table* t = new (std::nothrow) nfagg_k8s_table;
    if (!t) return fail(h, NFAGG_ENOMEM, "out of memory");
    t->h = h;
    t->has_layer = layer != nullptr;
    size_t cap = 1;
    while (cap < 2 * n) cap <<= 1;                                       // at most half full: a probe always meets a free slot
    K8sSlot free_slot{};
    free_slot.row = kK8sNoRow;
    t->slots.assign(cap, free_slot);
    t->rows.resize(n);
    t->host_ids.assign(n, 0u);
    std::vector<uint8_t> piece;
    for (size_t r = 0; r < n; r++) {
        const nfagg_k8s_entry& e = entries[r];
        K8sSlot key{};
        memcpy(key.ip, e.ip, 16);
        uint64_t lo, hi;
        memcpy(&lo, e.ip, 8); memcpy(&hi, e.ip + 8, 8);
        size_t s = (size_t)((uint32_t)k8s_hash(lo, hi) & (uint32_t)(cap - 1));
        while (t->slots[s].row != kK8sNoRow) {
            if (memcmp(t->slots[s].ip, key.ip, 16) == 0) {
                const uint32_t first = t->slots[s].row;
                delete t;
                return fail(h, NFAGG_EINVAL, "Kubernetes entries %u and %zu carry the same address", first, r);
            }
            s = (s + 1) & (cap - 1);
        }
        key.row = (uint32_t)r;
        t->slots[s] = key;
        K8sRow& row = t->rows[r];
        row = K8sRow{};
        for (int side = 0; side < 2; side++) {
            bool bad_string;
            if (!k8s_render(e, side, piece, &bad_string) || piece.size() > kK8sMaxRendered) {
                const size_t got = piece.size();
                delete t;
                if (bad_string) return fail(h, NFAGG_EINVAL, "Kubernetes entry %zu: null string with a length", r);
                return fail(h, NFAGG_EINVAL, "Kubernetes entry %zu: its %s block has %s%zu bytes, the cap is %u", r, side ? "DstK8S" : "SrcK8S",
                            got ? "" : "more than ", got ? got : (size_t)kK8sMaxRendered, kK8sMaxRendered);
            }
            const uint32_t off = (uint32_t)(t->blob.size() / 16);
            t->blob.insert(t->blob.end(), piece.begin(), piece.end());
            t->blob.resize((t->blob.size() + 15) / 16 * 16, 0);          // the kernels read a block 16 bytes at a time
            if (side == 0) { row.src_off = off; row.src_len = (uint16_t)piece.size(); }
            else { row.dst_off = off; row.dst_len = (uint16_t)piece.size(); }
        }
        row.flags = layer && k8s_is_app(e, *layer) ? kK8sRowApp : 0u;
        // the text of the row's SrcK8S_HostIP / DstK8S_HostIP key, as reinterpret_direction compares it; the key is absent for ""
        t->host_ids[r] = e.host_ip_len ? t->host_text.emplace(std::string(e.host_ip, e.host_ip_len), (uint32_t)t->host_text.size() + 1).first->second : 0u;
        const K8sStr field[9] = {{e.namespace_, e.namespace_len}, {e.name, e.name_len}, {e.kind, e.kind_len}, {e.owner_name, e.owner_name_len},
                                 {e.owner_kind, e.owner_kind_len}, {e.network_name, e.network_name_len}, {e.host_ip, e.host_ip_len},
                                 {e.host_name, e.host_name_len}, {e.zone, e.zone_len}};
        const bool present[9] = {e.namespace_len != 0, true, true, true, true, true, e.host_ip_len != 0, e.host_ip_len != 0 && e.host_name_len != 0,
                                 e.has_zone != 0};
        for (int f = 0; f < 9; f++)                                      // k8s_render has refused a null string with a length
            t->field_ids.push_back(present[f] ? 1u + t->field_text.emplace(std::string(field[f].p ? field[f].p : "", field[f].len),
                                                                           (uint32_t)t->field_text.size()).first->second : 0u);
    }
    if (h) {
        auto up = [&]() -> int {
            HIP_TRY(h, hipSetDevice(h->device));
            HIP_TRY(h, t->d_slots.alloc(cap * sizeof(K8sSlot)));
            HIP_TRY(h, t->d_rows.alloc(std::max<size_t>(n, 1) * sizeof(K8sRow)));
            HIP_TRY(h, t->d_blob.alloc(std::max<size_t>(t->blob.size(), 16)));
            HIP_TRY(h, t->d_host_ids.alloc(std::max<size_t>(n, 1) * sizeof(uint32_t)));
            if (n) HIP_TRY(h, hipMemcpy(t->d_host_ids.p, t->host_ids.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice));
            HIP_TRY(h, hipMemcpy(t->d_slots.p, t->slots.data(), cap * sizeof(K8sSlot), hipMemcpyHostToDevice));
            if (n) HIP_TRY(h, hipMemcpy(t->d_rows.p, t->rows.data(), n * sizeof(K8sRow), hipMemcpyHostToDevice));
            if (!t->blob.empty()) HIP_TRY(h, hipMemcpy(t->d_blob.p, t->blob.data(), t->blob.size(), hipMemcpyHostToDevice));
            return NFAGG_OK;
        };
        const int rc = up();
        if (rc != NFAGG_OK) { nfagg_k8s_table_destroy(t); return rc; }
    }
    *table = t;
    return NFAGG_OK;
}

void nfagg_k8s_table_destroy(nfagg_k8s_table* t) { destroy_on_handle(t); }

int nfagg_k8s_resolve_device(nfagg_handle* h, const nfagg_k8s_table* table, const void* d_records, size_t n, uint32_t* d_rows) {
    if (!h || !table || (n && (!d_records || !d_rows))) return fail(h, NFAGG_EINVAL, "null argument");
    if (table->h != h || !table->d_slots) return fail(h, NFAGG_EINVAL, "the Kubernetes table was not created for this handle");
    if (((uintptr_t)d_records & 15u) != 0 || ((uintptr_t)d_rows & 7u) != 0) return fail(h, NFAGG_EINVAL, "device records must be 16-byte, rows 8-byte aligned");
    HIP_TRY(h, hipSetDevice(h->device));
    if (n) {
        hipError_t e = launch_k8s_resolve(d_records, n, k8s_dev(table), d_rows, h->stream);
        if (e != hipSuccess) return fail(h, NFAGG_EDEVICE, "Kubernetes resolve launch failed: %s", hipGetErrorString(e));
    }
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return NFAGG_OK;
}

int nfagg_k8s_resolve(nfagg_handle* h, const nfagg_k8s_table* table, const void* records, size_t n, uint32_t* rows) {
    if (!h || !table || (n && (!records || !rows))) return fail(h, NFAGG_EINVAL, "null argument");
    auto& S = h->enc;
    HIP_TRY(h, hipSetDevice(h->device));
    API_TRY(S.k8s_rows.ensure(h, n * 2 * sizeof(uint32_t) + kStageSlack));
    API_TRY(stage_in(h, S.in_records, records, n * kRecordBytes));
    API_TRY(nfagg_k8s_resolve_device(h, table, S.in_records.p, n, S.k8s_rows.as<uint32_t>()));
    API_TRY(fetch(h, rows, S.k8s_rows, n * 2 * sizeof(uint32_t)));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return NFAGG_OK;
}

}  // extern "C"

// ---- direction, subnet labels, TCP flag names (nfagg_net.h): the caller's rules as a table and the join alone
namespace {

// One label's fragment, ,"SrcSubnetLabel":"<escaped>" or ,"DstSubnetLabel":"<escaped>"; empty for an empty label.
void net_render(const char* text, uint32_t len, int side, std::vector<uint8_t>& o) {
    o.clear();
    if (!len) return;
    const char* head = side ? ",\"DstSubnetLabel\":" : ",\"SrcSubnetLabel\":";
    o.insert(o.end(), head, head + 18);
    std::vector<uint8_t> buf(2 + 6 * (size_t)len);
    const uint32_t n = flp_escape(text, len, buf.data());
    o.insert(o.end(), buf.begin(), buf.begin() + n);
}

// net.CIDRMask(ones, 128) as four little-endian dwords of the 16 bytes
void net_mask128(uint32_t ones, uint8_t m[16]) {
    for (uint32_t k = 0; k < 16; k++) m[k] = ones >= 8 * (k + 1) ? 0xffu : ones > 8 * k ? (uint8_t)(0xff00u >> (ones - 8 * k)) : 0u;
}

}  // namespace

extern "C" {

int nfagg_net_table_create(nfagg_handle* h, const nfagg_net_rules* rules, nfagg_net_table** table) {
    if (!table || !rules) return fail(h, NFAGG_EINVAL, "null argument");
    *table = nullptr;
    if (rules->struct_size != sizeof(nfagg_net_rules)) return fail(h, NFAGG_EINVAL, "nfagg_net_rules.struct_size mismatch");
    const uint32_t known = NFAGG_NET_REINTERPRET_DIRECTION | NFAGG_NET_SUBNET_LABELS | NFAGG_NET_DECODE_TCP_FLAGS;
    if (rules->flags & ~known) return fail(h, NFAGG_EINVAL, "unknown net rule flags 0x%x", rules->flags & ~known);
    if ((rules->n_cidrs && !rules->cidrs) || (rules->n_labels && !rules->labels)) return fail(h, NFAGG_EINVAL, "null list with a count");
    if (rules->n_cidrs > NFAGG_NET_MAX_CIDRS) return fail(h, NFAGG_EINVAL, "%u CIDRs, more than %u", rules->n_cidrs, (unsigned)NFAGG_NET_MAX_CIDRS);
    if (rules->n_labels > NFAGG_NET_MAX_CIDRS) return fail(h, NFAGG_EINVAL, "%u labels, more than %u", rules->n_labels, (unsigned)NFAGG_NET_MAX_CIDRS);
    nfagg_net_table* t = new (std::nothrow) nfagg_net_table;
    if (!t) return fail(h, NFAGG_ENOMEM, "out of memory");
    t->h = h;
    t->flags = rules->flags;
    std::vector<uint8_t> piece;
    for (uint32_t k = 0; k < rules->n_labels; k++) {
        const nfagg_net_label& l = rules->labels[k];
        if (l.len && !l.text) { delete t; return fail(h, NFAGG_EINVAL, "net label %u: null string with a length", k); }
        if (l.len > kNetLabelMax) { delete t; return fail(h, NFAGG_EINVAL, "net label %u: its escaped value has more than %u bytes", k, kNetLabelMax); }
        NetFrag f{};
        for (int side = 0; side < 2; side++) {
            net_render(l.text, l.len, side, piece);
            if (piece.size() > kNetFragMax) {
                const size_t got = piece.size() - (kNetFragMax - kNetLabelMax);
                delete t;
                return fail(h, NFAGG_EINVAL, "net label %u: its escaped value has %zu bytes, the cap is %u", k, got, kNetLabelMax);
            }
            const uint32_t off = (uint32_t)(t->blob.size() / 16);
            t->blob.insert(t->blob.end(), piece.begin(), piece.end());
            t->blob.resize((t->blob.size() + 15) / 16 * 16, 0);          // the kernels read a fragment 16 bytes at a time
            if (side == 0) { f.src_off = off; f.src_len = (uint32_t)piece.size(); }
            else { f.dst_off = off; f.dst_len = (uint32_t)piece.size(); }
        }
        t->frags.push_back(f);
    }
    static const uint8_t v4_prefix[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0xff, 0xff};
    for (uint32_t k = 0; k < rules->n_cidrs; k++) {
        const nfagg_net_cidr& c = rules->cidrs[k];
        if (c.bits != 32 && c.bits != 128) { delete t; return fail(h, NFAGG_EINVAL, "CIDR %u: %u bits, neither 32 nor 128", k, c.bits); }
        if (c.ones > c.bits) { delete t; return fail(h, NFAGG_EINVAL, "CIDR %u: a prefix of %u in %u bits", k, c.ones, c.bits); }
        if (c.label >= rules->n_labels) { delete t; return fail(h, NFAGG_EINVAL, "CIDR %u: label %u of %u", k, c.label, rules->n_labels); }
        if (c.bits == 32 && memcmp(c.ip, v4_prefix, 12) != 0) { delete t; return fail(h, NFAGG_EINVAL, "CIDR %u: 32 bits and an address that is not v4-mapped", k); }
        // net.IPNet.Contains -> networkNumberAndMask: the network is IPv4 iff its masked address is v4-mapped, and then only
        // the mask's last 32 bits count; the twelve 0xff in front make the compare refuse every address that is not v4-mapped
        uint8_t mask[16], netw[16];
        net_mask128(c.bits == 32 ? 96 + c.ones : c.ones, mask);
        for (int b = 0; b < 16; b++) netw[b] = c.ip[b] & mask[b];
        const bool v4 = memcmp(netw, v4_prefix, 12) == 0;
        if (v4) memset(mask, 0xff, 12);
        NetCidr d;
        memcpy(d.net, netw, 16); memcpy(d.mask, mask, 16);
        t->cidrs.push_back(d);
        t->meta.push_back(c.label | (v4 ? 0u : kNetCidrV6));
    }
    auto up32 = [](size_t x) { return (x + 31) / 32 * 32; };
    t->off_meta = up32(std::max<size_t>(t->cidrs.size(), 1) * sizeof(NetCidr));
    t->off_frags = t->off_meta + up32(std::max<size_t>(t->meta.size(), 1) * sizeof(uint32_t));
    t->off_blob = t->off_frags + up32(std::max<size_t>(t->frags.size(), 1) * sizeof(NetFrag));
    if (h) {
        auto up = [&]() -> int {
            std::vector<uint8_t> img(t->off_blob + std::max<size_t>(t->blob.size(), 16), 0);
            if (!t->cidrs.empty()) memcpy(img.data(), t->cidrs.data(), t->cidrs.size() * sizeof(NetCidr));
            if (!t->meta.empty()) memcpy(img.data() + t->off_meta, t->meta.data(), t->meta.size() * sizeof(uint32_t));
            if (!t->frags.empty()) memcpy(img.data() + t->off_frags, t->frags.data(), t->frags.size() * sizeof(NetFrag));
            if (!t->blob.empty()) memcpy(img.data() + t->off_blob, t->blob.data(), t->blob.size());
            HIP_TRY(h, hipSetDevice(h->device));
            HIP_TRY(h, t->d_mem.alloc(img.size()));
            HIP_TRY(h, hipMemcpy(t->d_mem.p, img.data(), img.size(), hipMemcpyHostToDevice));
            return NFAGG_OK;
        };
        const int rc = up();
        if (rc != NFAGG_OK) { nfagg_net_table_destroy(t); return rc; }
    }
    *table = t;
    return NFAGG_OK;
}

void nfagg_net_table_destroy(nfagg_net_table* t) { destroy_on_handle(t); }

int nfagg_net_render(const nfagg_net_table* table, int side, uint32_t label, void* out, size_t cap, size_t* n_out) {
    if (!table || !n_out) return fail(nullptr, NFAGG_EINVAL, "null argument");
    if (side != 0 && side != 1) return fail(nullptr, NFAGG_EINVAL, "unknown side %d", side);
    if (label >= table->frags.size()) return fail(nullptr, NFAGG_EINVAL, "label %u of %zu", label, table->frags.size());
    const NetFrag& f = table->frags[label];
    const size_t off = (size_t)(side ? f.dst_off : f.src_off) * 16, len = side ? f.dst_len : f.src_len;
    *n_out = len;
    if (len && (!out || cap < len)) return NFAGG_TRUNCATED;
    if (len) memcpy(out, table->blob.data() + off, len);
    return NFAGG_OK;
}

int nfagg_net_resolve_device(nfagg_handle* h, const nfagg_net_table* net_table, const nfagg_k8s_table* k8s_table, const void* d_records,
                             size_t n, const uint32_t* d_k8s_rows, const nfagg_flp_options* opt, nfagg_net_row* d_out) {
    if (!h || !net_table || (n && (!d_records || !d_out))) return fail(h, NFAGG_EINVAL, "null argument");
    if (net_table->h != h || !net_table->d_mem) return fail(h, NFAGG_EINVAL, "the net table was not created for this handle");
    const bool dir = (net_table->flags & NFAGG_NET_REINTERPRET_DIRECTION) != 0;
    if (dir) {
        if (!k8s_table || !opt || (n && !d_k8s_rows)) return fail(h, NFAGG_EINVAL, "reinterpret_direction needs the Kubernetes table, the flows' rows and the options");
        if (opt->struct_size != sizeof(nfagg_flp_options)) return fail(h, NFAGG_EINVAL, "nfagg_flp_options.struct_size mismatch");
        if (k8s_table->h != h || !k8s_table->d_slots) return fail(h, NFAGG_EINVAL, "the Kubernetes table was not created for this handle");
    }
    if (((uintptr_t)d_records & 15u) != 0 || ((uintptr_t)d_out & 7u) != 0 || (dir && ((uintptr_t)d_k8s_rows & 7u) != 0))
        return fail(h, NFAGG_EINVAL, "device records must be 16-byte, rows 8-byte aligned");
    HIP_TRY(h, hipSetDevice(h->device));
    if (n) {
        hipError_t e = launch_net_resolve(d_records, n, net_dev(net_table), dir ? d_k8s_rows : nullptr, dir ? k8s_table->d_host_ids.as<const uint32_t>() : nullptr,
                                          dir ? (uint32_t)k8s_table->rows.size() : 0u, dir ? net_reporter(k8s_table, opt) : kNetNoHost, (uint2*)d_out,
                                          h->stream);
        if (e != hipSuccess) return fail(h, NFAGG_EDEVICE, "net resolve launch failed: %s", hipGetErrorString(e));
    }
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return NFAGG_OK;
}

int nfagg_net_resolve(nfagg_handle* h, const nfagg_net_table* net_table, const nfagg_k8s_table* k8s_table, const void* records, size_t n,
                      const uint32_t* k8s_rows, const nfagg_flp_options* opt, nfagg_net_row* out) {
    if (!h || !net_table || (n && (!records || !out))) return fail(h, NFAGG_EINVAL, "null argument");
    const bool dir = (net_table->flags & NFAGG_NET_REINTERPRET_DIRECTION) != 0;
    if (dir && n && !k8s_rows) return fail(h, NFAGG_EINVAL, "reinterpret_direction needs the Kubernetes table, the flows' rows and the options");
    auto& S = h->enc;
    HIP_TRY(h, hipSetDevice(h->device));
    API_TRY(S.net_rows.ensure(h, n * sizeof(nfagg_net_row) + kStageSlack));
    API_TRY(stage_in(h, S.in_records, records, n * kRecordBytes));
    API_TRY(stage_in(h, S.k8s_rows, k8s_rows, dir ? n * 2 * sizeof(uint32_t) : 0));
    API_TRY(nfagg_net_resolve_device(h, net_table, k8s_table, S.in_records.p, n, S.k8s_rows.as<const uint32_t>(), opt, S.net_rows.as<nfagg_net_row>()));
    API_TRY(fetch(h, out, S.net_rows, n * sizeof(nfagg_net_row)));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return NFAGG_OK;
}

}  // extern "C"

// ---- flow metrics (nfagg_metrics.h): the groupings' classes over a Kubernetes table, and the fold's host side
extern "C" {

// specs == nullptr: the plain table of dims.
static int metrics_table_create(nfagg_handle* h, const nfagg_k8s_table* k8s_table, const uint32_t* dims, const nfagg_metric_spec* specs, uint32_t n_groupings,
                                nfagg_metrics_table** table) {
    if (n_groupings < 1 || n_groupings > kMetMaxGroupings) return fail(h, NFAGG_EINVAL, "%u groupings, not 1..%u", n_groupings, kMetMaxGroupings);
    for (uint32_t g = 0; g < n_groupings; g++)
        if (dims[g] & ~NFAGG_DIM_ALL) return fail(h, NFAGG_EINVAL, "grouping %u: unknown dimension bits 0x%x", g, dims[g] & ~NFAGG_DIM_ALL);
    if (k8s_table->h != h) return fail(h, NFAGG_EINVAL, "the Kubernetes table was not created for this handle");
    nfagg_metrics_table* t = new (std::nothrow) nfagg_metrics_table;
    if (!t) return fail(h, NFAGG_ENOMEM, "out of memory");
    t->h = h;
    t->k8s = k8s_table;
    t->n_groupings = n_groupings;
    t->has_specs = specs != nullptr;
    for (uint32_t g = 0; g < n_groupings; g++) {
        if (specs) t->specs[g] = specs[g];
        else { t->specs[g].struct_size = sizeof(nfagg_metric_spec); t->specs[g].dims = dims[g]; }
    }
    const size_t n = k8s_table->rows.size();
    size_t words = 0;
    for (uint32_t g = 0; g < n_groupings; g++) {
        t->dims[g] = dims[g];
        for (int side = 0; side < 2; side++) {
            const uint32_t sel = (dims[g] >> (9 * side)) & kMetSrcFields;
            if (!sel) continue;
            std::map<std::vector<uint32_t>, uint32_t> seen;
            std::vector<uint32_t> key;
            t->cls[g][side].resize(n);
            for (size_t r = 0; r < n; r++) {
                key.clear();
                for (int f = 0; f < 9; f++) if (sel & (1u << f)) key.push_back(k8s_table->field_ids[r * 9 + f]);
                const auto it = seen.emplace(key, (uint32_t)seen.size() + 1);
                if (it.second) t->first_row[g][side].push_back((uint32_t)r);
                t->cls[g][side][r] = it.first->second;
            }
            t->d_off[g][side] = words;
            words += (n + 3) / 4 * 4;
        }
    }
    if (h) {
        auto up = [&]() -> int {
            HIP_TRY(h, hipSetDevice(h->device));
            HIP_TRY(h, t->d_cls.alloc(std::max<size_t>(words, 4) * sizeof(uint32_t)));
            for (uint32_t g = 0; g < n_groupings; g++)
                for (int side = 0; side < 2; side++)
                    if (n && !t->cls[g][side].empty())
                        HIP_TRY(h, hipMemcpy(t->d_cls.as<uint32_t>() + t->d_off[g][side], t->cls[g][side].data(), n * sizeof(uint32_t), hipMemcpyHostToDevice));
            return NFAGG_OK;
        };
        const int rc = up();
        if (rc != NFAGG_OK) { nfagg_metrics_table_destroy(t); return rc; }
    }
    *table = t;
    return NFAGG_OK;
}

int nfagg_metrics_table_create(nfagg_handle* h, const nfagg_k8s_table* k8s_table, const uint32_t* dims, uint32_t n_groupings,
                               nfagg_metrics_table** table) {
    if (!table || !k8s_table || !dims) return fail(h, NFAGG_EINVAL, "null argument");
    *table = nullptr;
    return metrics_table_create(h, k8s_table, dims, nullptr, n_groupings, table);
}

int nfagg_metrics_table_create_specs(nfagg_handle* h, const nfagg_k8s_table* k8s_table, const nfagg_metric_spec* specs, uint32_t n_groupings,
                                     nfagg_metrics_table** table) {
    if (!table || !k8s_table || !specs) return fail(h, NFAGG_EINVAL, "null argument");
    *table = nullptr;
    if (n_groupings < 1 || n_groupings > kMetMaxGroupings) return fail(h, NFAGG_EINVAL, "%u groupings, not 1..%u", n_groupings, kMetMaxGroupings);
    uint32_t dims[kMetMaxGroupings] = {};
    for (uint32_t g = 0; g < n_groupings; g++) {
        const nfagg_metric_spec& sp = specs[g];
        if (sp.struct_size != sizeof(nfagg_metric_spec)) return fail(h, NFAGG_EINVAL, "grouping %u: struct_size %u, not %zu", g, sp.struct_size, sizeof(nfagg_metric_spec));
        if (sp.xdims & ~NFAGG_XDIM_ALL) return fail(h, NFAGG_EINVAL, "grouping %u: unknown xdims bits 0x%x", g, sp.xdims & ~NFAGG_XDIM_ALL);
        for (int k = 0; k < 2; k++)
            if (sp.value[k] > NFAGG_MET_VALUE_LAST) return fail(h, NFAGG_EINVAL, "grouping %u: value[%d]: unknown source %u", g, k, sp.value[k]);
        if (sp.hist > 2) return fail(h, NFAGG_EINVAL, "grouping %u: hist %u, not 0, 1 or 2", g, sp.hist);
        if (sp.hist) {
            if (sp.value[sp.hist - 1] == NFAGG_MET_VALUE_NONE) return fail(h, NFAGG_EINVAL, "grouping %u: hist %u names the empty value[%u]", g, sp.hist, sp.hist - 1u);
            if (sp.n_bounds < 1 || sp.n_bounds > NFAGG_MET_MAX_BOUNDS) return fail(h, NFAGG_EINVAL, "grouping %u: n_bounds %u, not 1..%u", g, sp.n_bounds, NFAGG_MET_MAX_BOUNDS);
            for (uint32_t k = 1; k < sp.n_bounds; k++)
                if (sp.bounds[k] < sp.bounds[k - 1]) return fail(h, NFAGG_EINVAL, "grouping %u: bounds[%u] is below bounds[%u]: bounds must not decrease", g, k, k - 1);
        }
        dims[g] = sp.dims;
    }
    return metrics_table_create(h, k8s_table, dims, specs, n_groupings, table);
}

void nfagg_metrics_table_destroy(nfagg_metrics_table* t) { destroy_on_handle(t); }

uint64_t nfagg_metrics_group_hash(uint32_t grouping, const nfagg_metric_group* key) {
    if (!key || grouping >= kMetMaxGroupings) return 0;
    return met_hash(met_key_a(grouping, key->src_class, key->dst_class),
                    met_key_b(grouping, key->src_label, key->dst_label, key->direction, key->layer, key->proto, key->is_ip));
}

uint64_t nfagg_metrics_group_hash_content(uint32_t grouping, const nfagg_metric_group_content* key) {
    if (!key || grouping >= kMetMaxGroupings || key->ipsec_status > 2 || (key->bucket > NFAGG_MET_MAX_BOUNDS && key->bucket != NFAGG_MET_NO_BUCKET)) return 0;
    return met_hash(met_key_a(grouping, key->src_class, key->dst_class),
                    met_key_b(grouping, key->src_label, key->dst_label, key->direction, key->layer, key->proto, key->is_ip),
                    met_key_c(grouping, key->drop_cause, key->drop_state, key->dns_rcode, key->ipsec_status, key->bucket));
}

int nfagg_flp_enum_name(int kind, uint32_t raw, void* out, size_t cap, size_t* len) {
    if (!len) return fail(nullptr, NFAGG_EINVAL, "null argument");
    uint32_t idx;
    if (kind == NFAGG_FLP_ENUM_DNS_RCODE) idx = rcode_name(raw);
    else if (kind == NFAGG_FLP_ENUM_TCP_STATE) idx = tcp_state_name(raw);
    else if (kind == NFAGG_FLP_ENUM_DROP_CAUSE) idx = drop_cause_name(raw);
    else return fail(nullptr, NFAGG_EINVAL, "unknown enum kind %d", kind);
    const size_t n = strlen(kFlpNames[idx]);
    *len = n;
    if (!out || cap < n) return NFAGG_TRUNCATED;
    memcpy(out, kFlpNames[idx], n);
    return NFAGG_OK;
}

uint32_t nfagg_metrics_n_classes(const nfagg_metrics_table* table, uint32_t g, int side) {
    if (!table || g >= table->n_groupings || (side != 0 && side != 1)) return 0;
    return (uint32_t)table->first_row[g][side].size();
}

int nfagg_metrics_class_row(const nfagg_metrics_table* table, uint32_t g, int side, uint32_t cls, uint32_t* row) {
    nfagg_handle* h = table ? table->h : nullptr;
    if (!table || !row) return fail(h, NFAGG_EINVAL, "null argument");
    if (g >= table->n_groupings || (side != 0 && side != 1)) return fail(h, NFAGG_EINVAL, "grouping %u, side %d: out of range", g, side);
    if (cls > table->first_row[g][side].size()) return fail(h, NFAGG_EINVAL, "class %u of %zu", cls, table->first_row[g][side].size());
    *row = cls ? table->first_row[g][side][cls - 1] : NFAGG_K8S_NO_ROW;
    return NFAGG_OK;
}

// The device side of both folds. X == nullptr: nfagg_metrics_fold_device (d_out: nfagg_metric_group arrays); else the content
// fold over X's specs and feature arrays (d_out: nfagg_metric_group_content arrays).
static int metrics_fold_device_core(nfagg_handle* h, const nfagg_metrics_table* table, const void* d_records, size_t n, MetSpecDev* X,
                                    const uint32_t* d_k8s_rows, const nfagg_net_row* d_net_rows, const uint32_t* group_cap, void* const* d_out,
                                    uint32_t* n_groups) {
    if (!h || !table || !group_cap || !d_out || !n_groups || (n && (!d_records || !d_k8s_rows))) return fail(h, NFAGG_EINVAL, "null argument");
    if (table->h != h || !table->d_cls) return fail(h, NFAGG_EINVAL, "the metrics table was not created for this handle");
    if (!X && table->has_specs) return fail(h, NFAGG_EINVAL, "the metrics table was created from specs: use nfagg_metrics_fold_content");
    const uint32_t G = table->n_groupings;
    const uint32_t net_dims = NFAGG_DIM_SRC_SUBNET_LABEL | NFAGG_DIM_DST_SUBNET_LABEL | NFAGG_DIM_FLOW_DIRECTION;
    const uint32_t words = X ? kMetcSlotWords : kMetSlotWords;
    MetDev M{};
    M.n_groupings = G;
    uint64_t blocks = 0;
    for (uint32_t g = 0; g < G; g++) {
        if (group_cap[g] > kMetMaxGroups) return fail(h, NFAGG_ERANGE, "grouping %u: a cap of %u groups, more than %u", g, group_cap[g], kMetMaxGroups);
        if (group_cap[g] && !d_out[g]) return fail(h, NFAGG_EINVAL, "grouping %u: a cap without an output array", g);
        if (((uintptr_t)d_out[g] & 15u) != 0) return fail(h, NFAGG_EINVAL, "device records and group arrays must be 16-byte, rows 8-byte aligned");
        if (n && (table->dims[g] & net_dims) && !d_net_rows) return fail(h, NFAGG_EINVAL, "grouping %u selects a label or the direction: it needs the flows' net rows", g);
        M.dims[g] = table->dims[g];
        M.cap[g] = group_cap[g];
        M.mask[g] = (uint32_t)std::max<uint64_t>(next_pow2(2ull * group_cap[g]), kMetMinSlots) - 1;
        M.first_block[g] = (uint32_t)blocks;
        blocks += ((uint64_t)M.mask[g] + 1) / kMetMinSlots;
        M.out[g] = d_out[g];
        if (M.dims[g] & NFAGG_DIM_FLOW_LAYER) M.any_layer = 1;
        for (int side = 0; side < 2; side++)
            M.cls[g][side] = table->cls[g][side].empty() ? nullptr : table->d_cls.as<const uint32_t>() + table->d_off[g][side];
        if (X) {
            const nfagg_metric_spec& sp = table->specs[g];
            X->xdims[g] = sp.xdims; X->value[g][0] = sp.value[0]; X->value[g][1] = sp.value[1];
            X->hist[g] = sp.hist; X->n_bounds[g] = sp.hist ? (uint8_t)sp.n_bounds : 0;
            for (uint32_t k = 0; k < X->n_bounds[g]; k++) X->bounds[g][k] = sp.bounds[k];
            uint32_t need = 0;
            for (int k = 0; k < 2; k++)
                need |= sp.value[k] == NFAGG_MET_VALUE_RTT_NS ? kMetNeedAdditional : sp.value[k] == NFAGG_MET_VALUE_DNS_LATENCY_MS ? kMetNeedDns :
                        (sp.value[k] == NFAGG_MET_VALUE_DROP_BYTES || sp.value[k] == NFAGG_MET_VALUE_DROP_PACKETS) ? kMetNeedDrops : 0u;
            need |= (sp.xdims & NFAGG_XDIM_IPSEC_STATUS ? kMetNeedAdditional : 0u) | (sp.xdims & NFAGG_XDIM_DNS_RCODE ? kMetNeedDns : 0u) |
                    (sp.xdims & (NFAGG_XDIM_DROP_CAUSE | NFAGG_XDIM_DROP_STATE) ? kMetNeedDrops : 0u);
            X->need |= need;
        }
    }
    if (X)      // a part whose array is missing, or all of them without the present bytes, is absent for every flow
        X->need &= !X->present ? 0u : (X->additional ? kMetNeedAdditional : 0u) | (X->dns ? kMetNeedDns : 0u) | (X->drops ? kMetNeedDrops : 0u);
    M.first_block[G] = (uint32_t)blocks;
    if (((uintptr_t)d_records & 15u) != 0 || ((uintptr_t)d_k8s_rows & 7u) != 0 || ((uintptr_t)d_net_rows & 7u) != 0)
        return fail(h, NFAGG_EINVAL, "device records and group arrays must be 16-byte, rows 8-byte aligned");
    for (uint32_t g = 0; g < G; g++) n_groups[g] = 0;
    if (!n) return NFAGG_OK;
    const K8sDev K = k8s_dev(table->k8s);
    M.rows = K.rows; M.n_rows = K.n_rows; M.has_layer = K.has_layer;
    auto& S = h->enc;
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t slot_bytes = (size_t)blocks * kMetMinSlots * words * sizeof(uint64_t);
    API_TRY(ensure_all(h, {{S.met_slots, 256 + slot_bytes}, {S.local_off, (size_t)blocks * kMetMinSlots * sizeof(uint32_t)},
                           {S.block_sum, (size_t)blocks * sizeof(uint32_t)}, {S.block_base, ((size_t)blocks + 1) * sizeof(uint64_t)}}));
    M.ctl = S.met_slots.as<MetCtl>();
    uint64_t* slots = (uint64_t*)(S.met_slots.as<uint8_t>() + 256);
    for (uint32_t g = 0; g < G; g++) M.slots[g] = slots + (size_t)M.first_block[g] * kMetMinSlots * words;
    HIP_TRY(h, hipMemsetAsync(S.met_slots.p, 0, 256 + slot_bytes, h->stream));
    hipError_t e = X ? launch_metrics_fold_content(d_records, n, M, *X, d_k8s_rows, (const uint2*)d_net_rows, h->stream)
                     : launch_metrics_fold(d_records, n, M, d_k8s_rows, (const uint2*)d_net_rows, h->stream);
    if (e != hipSuccess) return fail(h, NFAGG_EDEVICE, "metrics fold launch failed: %s", hipGetErrorString(e));
    e = launch_metrics_emit(M, X != nullptr, S.local_off.as<uint32_t>(), S.block_sum.as<uint32_t>(), S.block_base.as<uint64_t>(), h->stream);
    if (e != hipSuccess) return fail(h, NFAGG_EDEVICE, "metrics emit launch failed: %s", hipGetErrorString(e));
    MetCtl ctl;
    HIP_TRY(h, hipMemcpyAsync(&ctl, M.ctl, sizeof ctl, hipMemcpyDeviceToHost, h->stream));      // the one read-back: counts and flags
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    bool over = false;
    for (uint32_t g = 0; g < G; g++) {
        // an overflowed grouping stopped claiming behind its cap: its count is a lower bound, and above the cap
        n_groups[g] = ctl.over[g] ? std::max(ctl.count[g], group_cap[g] + 1) : ctl.count[g];
        over = over || ctl.over[g];
    }
    return over ? NFAGG_TRUNCATED : NFAGG_OK;
}

// The host-memory side of both folds: stage the inputs, run the device core on the staged copies, fetch the groups. feat: HOST
// pointers; content selects the entry point (feat may be nullptr there: no flow has a part).
static int metrics_fold_host_core(nfagg_handle* h, const nfagg_metrics_table* table, const void* records, size_t n, bool content, const nfagg_pb_features* feat,
                                  const uint32_t* k8s_rows, const nfagg_net_row* net_rows, const uint32_t* group_cap, void* const* out, uint32_t* n_groups) {
    if (!h || !table || !group_cap || !out || !n_groups || (n && (!records || !k8s_rows))) return fail(h, NFAGG_EINVAL, "null argument");
    if (feat && feat->struct_size != sizeof(nfagg_pb_features)) return fail(h, NFAGG_EINVAL, "nfagg_pb_features.struct_size mismatch");
    const uint32_t G = table->n_groupings;
    const size_t group_bytes = content ? sizeof(nfagg_metric_group_content) : sizeof(nfagg_metric_group);
    size_t total = 0;
    for (uint32_t g = 0; g < G; g++) {
        if (group_cap[g] > kMetMaxGroups) return fail(h, NFAGG_ERANGE, "grouping %u: a cap of %u groups, more than %u", g, group_cap[g], kMetMaxGroups);
        if (group_cap[g] && !out[g]) return fail(h, NFAGG_EINVAL, "grouping %u: a cap without an output array", g);
        total += group_cap[g];
    }
    auto& S = h->enc;
    HIP_TRY(h, hipSetDevice(h->device));
    API_TRY(S.met_out.ensure(h, total * group_bytes + kStageSlack));
    API_TRY(stage_in(h, S.in_records, records, n * kRecordBytes));
    API_TRY(stage_in(h, S.k8s_rows, k8s_rows, n * 2 * sizeof(uint32_t)));
    API_TRY(stage_in(h, S.net_rows, net_rows, net_rows ? n * sizeof(nfagg_net_row) : 0));
    int rc;
    void* d_out[kMetMaxGroupings] = {};
    size_t at = 0;
    for (uint32_t g = 0; g < G; g++) { d_out[g] = S.met_out.as<uint8_t>() + at * group_bytes; at += group_cap[g]; }
    const nfagg_net_row* d_net = net_rows ? S.net_rows.as<const nfagg_net_row>() : nullptr;
    if (content) {
        nfagg_pb_features dfeat{};
        if (feat && n) API_TRY(stage_pb_features(h, feat, n, &dfeat));
        rc = nfagg_metrics_fold_content_device(h, table, S.in_records.p, n, (feat && n) ? &dfeat : nullptr, S.k8s_rows.as<const uint32_t>(), d_net, group_cap,
                                               (nfagg_metric_group_content* const*)d_out, n_groups);
    } else
        rc = nfagg_metrics_fold_device(h, table, S.in_records.p, n, S.k8s_rows.as<const uint32_t>(), d_net, group_cap, (nfagg_metric_group* const*)d_out, n_groups);
    if (rc != NFAGG_OK) return rc;
    for (uint32_t g = 0; g < G; g++)          // each grouping's part of met_out
        if (n_groups[g]) HIP_TRY(h, hipMemcpyAsync(out[g], d_out[g], (size_t)n_groups[g] * group_bytes, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return NFAGG_OK;
}

int nfagg_metrics_fold_device(nfagg_handle* h, const nfagg_metrics_table* table, const void* d_records, size_t n, const uint32_t* d_k8s_rows,
                              const nfagg_net_row* d_net_rows, const uint32_t* group_cap, nfagg_metric_group* const* d_out, uint32_t* n_groups) {
    return metrics_fold_device_core(h, table, d_records, n, nullptr, d_k8s_rows, d_net_rows, group_cap, (void* const*)d_out, n_groups);
}

int nfagg_metrics_fold(nfagg_handle* h, const nfagg_metrics_table* table, const void* records, size_t n, const uint32_t* k8s_rows,
                       const nfagg_net_row* net_rows, const uint32_t* group_cap, nfagg_metric_group* const* out, uint32_t* n_groups) {
    return metrics_fold_host_core(h, table, records, n, false, nullptr, k8s_rows, net_rows, group_cap, (void* const*)out, n_groups);
}

int nfagg_metrics_fold_content_device(nfagg_handle* h, const nfagg_metrics_table* table, const void* d_records, size_t n,
                                      const nfagg_pb_features* d_features, const uint32_t* d_k8s_rows, const nfagg_net_row* d_net_rows,
                                      const uint32_t* group_cap, nfagg_metric_group_content* const* d_out, uint32_t* n_groups) {
    MetSpecDev X{};
    if (d_features) {
        PbFeat F{};
        const int rc = device_features(h, d_features, &F);
        if (rc != NFAGG_OK) return rc;
        X.present = F.present; X.additional = F.additional; X.dns = F.dns; X.drops = F.drops;
    }
    return metrics_fold_device_core(h, table, d_records, n, &X, d_k8s_rows, d_net_rows, group_cap, (void* const*)d_out, n_groups);
}

int nfagg_metrics_fold_content(nfagg_handle* h, const nfagg_metrics_table* table, const void* records, size_t n,
                               const nfagg_pb_features* features, const uint32_t* k8s_rows, const nfagg_net_row* net_rows,
                               const uint32_t* group_cap, nfagg_metric_group_content* const* out, uint32_t* n_groups) {
    return metrics_fold_host_core(h, table, records, n, true, features, k8s_rows, net_rows, group_cap, (void* const*)out, n_groups);
}

}  // extern "C"
