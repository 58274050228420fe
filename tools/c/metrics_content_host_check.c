/* metrics_content_host_check.c — the host side of the content metrics (histograms, feature values and labels) driven from
 * plain C, without a handle and without a device: every refusal of nfagg_metrics_table_create_specs with its message, specs at
 * the limits (32 bounds, equal neighbours, INT64_MIN / INT64_MAX), nfagg_metrics_group_hash_content (the packing of the third
 * word: "none" values against real ones, every key field moves the hash, agreement with nfagg_metrics_group_hash's fields), and
 * nfagg_flp_enum_name over the whole of the three tables with caps of every size. A stand-alone program with its own main,
 * meant to be built with -fsanitize=address,undefined, so that the sanitizers see the checks' reads of the specs, the name
 * tables and the caller's buffers. Prints "metrics content host check ok" and returns 0.
 *   cc -std=c11 -O1 -g -fsanitize=address,undefined -I include tools/c/metrics_content_host_check.c -o check -L <libdir> -lnfagg -Wl,-rpath,<libdir> */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "nfagg.h"

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: %s\n  last error: %s\n", __FILE__, __LINE__, #cond, nfagg_last_error(NULL)); exit(1); } } while (0)

static nfagg_metric_spec spec(uint32_t dims, uint32_t xdims, uint8_t v0, uint8_t v1, uint8_t hist, uint32_t n_bounds) {
    nfagg_metric_spec s;
    memset(&s, 0, sizeof s);
    s.struct_size = sizeof s; s.dims = dims; s.xdims = xdims; s.value[0] = v0; s.value[1] = v1; s.hist = hist; s.n_bounds = n_bounds;
    for (uint32_t k = 0; k < n_bounds && k < NFAGG_MET_MAX_BOUNDS; k++) s.bounds[k] = (int64_t)k * 10;
    return s;
}

static nfagg_k8s_table* k8s;

static void refused(nfagg_metric_spec bad, const char* message) {
    nfagg_metric_spec specs[2] = {spec(0, 0, 0, 0, 0, 0), bad};
    nfagg_metrics_table* t = (nfagg_metrics_table*)&specs;
    CHECK(nfagg_metrics_table_create_specs(NULL, k8s, specs, 2, &t) == NFAGG_EINVAL && !t);
    if (!strstr(nfagg_last_error(NULL), message)) { fprintf(stderr, "wanted \"%s\", got \"%s\"\n", message, nfagg_last_error(NULL)); exit(1); }
}

static uint64_t hash_of(nfagg_metric_group_content g) { return nfagg_metrics_group_hash_content(3, &g); }

static size_t name_of(int kind, uint32_t raw, char* text) {
    size_t len = 999;
    char* exact;
    CHECK(nfagg_flp_enum_name(kind, raw, NULL, 0, &len) == NFAGG_TRUNCATED && len > 0 && len < 64);
    exact = malloc(len);                                        /* a buffer of exactly the length: one byte more is an overflow the sanitizer sees */
    CHECK(exact && nfagg_flp_enum_name(kind, raw, exact, len, &len) == NFAGG_OK);
    memcpy(text, exact, len);
    text[len] = 0;
    if (len > 1) { size_t l2 = 0; CHECK(nfagg_flp_enum_name(kind, raw, exact, len - 1, &l2) == NFAGG_TRUNCATED && l2 == len); }
    free(exact);
    return len;
}

int main(void) {
    CHECK(nfagg_k8s_table_create(NULL, NULL, 0, NULL, &k8s) == NFAGG_OK && k8s);

    /* ---- specs: the refusals, each naming the grouping and the field */
    nfagg_metric_spec s;
    refused(spec(1u << 23, 0, 0, 0, 0, 0), "grouping 1: unknown dimension bits 0x800000");
    refused(spec(0, 16, 0, 0, 0, 0), "grouping 1: unknown xdims bits 0x10");
    refused(spec(0, 0, NFAGG_MET_VALUE_LAST + 1, 0, 0, 0), "grouping 1: value[0]: unknown source 7");
    refused(spec(0, 0, 0, 255, 0, 0), "grouping 1: value[1]: unknown source 255");
    refused(spec(0, 0, NFAGG_MET_VALUE_RTT_NS, 0, 2, 4), "grouping 1: hist 2 names the empty value[1]");
    refused(spec(0, 0, 0, 0, 1, 4), "grouping 1: hist 1 names the empty value[0]");
    refused(spec(0, 0, NFAGG_MET_VALUE_RTT_NS, 0, 3, 4), "grouping 1: hist 3");
    refused(spec(0, 0, NFAGG_MET_VALUE_RTT_NS, 0, 1, 0), "grouping 1: n_bounds 0, not 1..32");
    refused(spec(0, 0, NFAGG_MET_VALUE_RTT_NS, 0, 1, 33), "grouping 1: n_bounds 33, not 1..32");
    s = spec(0, 0, NFAGG_MET_VALUE_RTT_NS, 0, 1, 5); s.bounds[3] = 19;
    refused(s, "grouping 1: bounds[3] is below bounds[2]");
    s = spec(0, 0, 0, 0, 0, 0); s.struct_size = sizeof s - 8;
    refused(s, "grouping 1: struct_size 272, not 280");
    nfagg_metrics_table* t = NULL;
    nfagg_metric_spec nine[9];
    for (int k = 0; k < 9; k++) nine[k] = spec(0, (uint32_t)k, 0, 0, 0, 0);
    CHECK(nfagg_metrics_table_create_specs(NULL, k8s, nine, 9, &t) == NFAGG_EINVAL && strstr(nfagg_last_error(NULL), "9 groupings"));
    CHECK(nfagg_metrics_table_create_specs(NULL, k8s, nine, 0, &t) == NFAGG_EINVAL);
    CHECK(nfagg_metrics_table_create_specs(NULL, NULL, nine, 1, &t) == NFAGG_EINVAL && nfagg_metrics_table_create_specs(NULL, k8s, NULL, 1, &t) == NFAGG_EINVAL);
    CHECK(nfagg_metrics_table_create_specs(NULL, k8s, nine, 1, NULL) == NFAGG_EINVAL);

    /* ---- specs at the limits: eight groupings, 32 bounds, equal neighbours, the ends of int64; n_bounds is ignored without a histogram */
    nfagg_metric_spec good[8];
    for (int k = 0; k < 8; k++) good[k] = spec(NFAGG_DIM_ALL, NFAGG_XDIM_ALL, NFAGG_MET_VALUE_DROP_BYTES, NFAGG_MET_VALUE_DROP_PACKETS, 0, 0);
    good[1] = spec(0, 0, NFAGG_MET_VALUE_DNS_LATENCY_MS, NFAGG_MET_VALUE_BYTES, 2, 32);
    good[2] = spec(0, 0, NFAGG_MET_VALUE_RTT_NS, 0, 1, 32);
    for (int k = 0; k < 32; k++) good[2].bounds[k] = k < 7 ? 0 : k < 31 ? k : INT64_MAX;       /* scale 1 folds seven bounds onto 0 */
    good[2].bounds[0] = INT64_MIN;
    good[3] = spec(0, 0, NFAGG_MET_VALUE_PACKETS, 0, 1, 1);
    good[4] = spec(0, 0, 0, 0, 0, 77);
    CHECK(nfagg_metrics_table_create_specs(NULL, k8s, good, 8, &t) == NFAGG_OK && t);
    CHECK(nfagg_metrics_n_classes(t, 0, 0) == 0);
    /* both folds refuse a table without a handle; the plain fold has no room for these groups at all */
    uint32_t cap = 4, n_groups = 0;
    nfagg_metric_group* out = NULL;
    nfagg_metric_group_content* outc = NULL;
    CHECK(nfagg_metrics_fold(NULL, t, NULL, 0, NULL, NULL, &cap, &out, &n_groups) == NFAGG_EINVAL);
    CHECK(nfagg_metrics_fold_content(NULL, t, NULL, 0, NULL, NULL, NULL, &cap, &outc, &n_groups) == NFAGG_EINVAL);
    CHECK(nfagg_metrics_fold_content_device(NULL, t, NULL, 0, NULL, NULL, NULL, &cap, &outc, &n_groups) == NFAGG_EINVAL);
    nfagg_metrics_table_destroy(t);
    nfagg_k8s_table_destroy(k8s);

    /* ---- the hash of a content group */
    nfagg_metric_group_content g;
    memset(&g, 0, sizeof g);
    g.src_class = 5; g.dst_class = 9; g.src_label = g.dst_label = NFAGG_NET_NO_LABEL; g.direction = NFAGG_NET_NO_DIRECTION;
    g.drop_state = 0xFFFF; g.dns_rcode = 0xFF; g.bucket = NFAGG_MET_NO_BUCKET;
    const uint64_t h0 = hash_of(g);
    CHECK(h0 != 0 && hash_of(g) == h0);
    nfagg_metric_group_content v;
    v = g; v.flows = 7; v.value_sum[1] = 9; v.pad_[3] = 1; CHECK(hash_of(v) == h0);            /* only the key fields are read */
    v = g; v.drop_cause = 1; CHECK(hash_of(v) != h0);
    v = g; v.drop_cause = 0xFFFFFFFFu; CHECK(hash_of(v) != h0);
    v = g; v.drop_state = 0; CHECK(hash_of(v) != h0);                                          /* a real state 0 is not "none" */
    v = g; v.drop_state = 255; CHECK(hash_of(v) != h0);
    v = g; v.dns_rcode = 0; CHECK(hash_of(v) != h0);
    v = g; v.dns_rcode = 15; CHECK(hash_of(v) != h0);
    v = g; v.ipsec_status = 1; CHECK(hash_of(v) != h0);
    v = g; v.ipsec_status = 2; CHECK(hash_of(v) != h0);
    v = g; v.bucket = 0; CHECK(hash_of(v) != h0);
    v = g; v.bucket = 32; CHECK(hash_of(v) != h0);
    v = g; v.src_class = 6; CHECK(hash_of(v) != h0);
    v = g; v.proto = 6; v.is_ip = 1; CHECK(hash_of(v) != h0);
    uint64_t seen[34];
    for (int b = 0; b <= 32; b++) { v = g; v.bucket = (uint8_t)b; seen[b] = hash_of(v); for (int k = 0; k < b; k++) CHECK(seen[k] != seen[b]); }
    CHECK(nfagg_metrics_group_hash_content(3, &g) != nfagg_metrics_group_hash_content(4, &g));
    CHECK(nfagg_metrics_group_hash_content(8, &g) == 0 && nfagg_metrics_group_hash_content(0, NULL) == 0);
    v = g; v.bucket = 33; CHECK(hash_of(v) == 0);
    v = g; v.ipsec_status = 3; CHECK(hash_of(v) == 0);

    /* ---- the names */
    char text[64];
    static const char* const rcodes[11] = {"NoError", "FormErr", "ServFail", "NXDomain", "NotImp", "Refused", "YXDomain", "YXRRSet", "NXRRSet", "NotAuth", "NotZone"};
    for (uint32_t r = 0; r < 16; r++) { name_of(NFAGG_FLP_ENUM_DNS_RCODE, r, text); CHECK(strcmp(text, r < 11 ? rcodes[r] : "UnDefined") == 0); }
    name_of(NFAGG_FLP_ENUM_TCP_STATE, 1, text); CHECK(strcmp(text, "TCP_ESTABLISHED") == 0);
    name_of(NFAGG_FLP_ENUM_TCP_STATE, 11, text); CHECK(strcmp(text, "TCP_NEW_SYN_RECV") == 0);
    for (uint32_t st = 0; st < 256; st += (st < 12 ? 1 : 61)) { name_of(NFAGG_FLP_ENUM_TCP_STATE, st, text); CHECK((strcmp(text, "TCP_INVALID_STATE") == 0) == (st == 0 || st > 11)); }
    name_of(NFAGG_FLP_ENUM_DROP_CAUSE, 2, text); CHECK(strcmp(text, "SKB_DROP_REASON_NOT_SPECIFIED") == 0);
    name_of(NFAGG_FLP_ENUM_DROP_CAUSE, 80, text); CHECK(strcmp(text, "SKB_DROP_REASON_TC_RECLASSIFY_LOOP") == 0);
    name_of(NFAGG_FLP_ENUM_DROP_CAUSE, (3u << 16) + 1, text); CHECK(strcmp(text, "OVS_DROP_LAST_ACTION") == 0);
    name_of(NFAGG_FLP_ENUM_DROP_CAUSE, (3u << 16) + 11, text); CHECK(strcmp(text, "OVS_DROP_IP_TTL") == 0);
    name_of(NFAGG_FLP_ENUM_DROP_CAUSE, (1u << 24) + 9, text); CHECK(strcmp(text, "NetworkEvent_UDNIsolation") == 0);
    static const uint32_t unknown[8] = {0, 1, 81, (3u << 16), (3u << 16) + 12, (1u << 24) + 10, 0xFFFFFFFFu, 1u << 31};
    for (int k = 0; k < 8; k++) { name_of(NFAGG_FLP_ENUM_DROP_CAUSE, unknown[k], text); CHECK(strcmp(text, "SKB_DROP_UNKNOWN_CAUSE") == 0); }
    for (uint32_t c = 2; c <= 80; c++) { name_of(NFAGG_FLP_ENUM_DROP_CAUSE, c, text); CHECK(strncmp(text, "SKB_DROP_REASON_", 16) == 0); }
    size_t len = 0;
    CHECK(nfagg_flp_enum_name(3, 0, text, sizeof text, &len) == NFAGG_EINVAL && nfagg_flp_enum_name(-1, 0, text, sizeof text, &len) == NFAGG_EINVAL);
    CHECK(nfagg_flp_enum_name(NFAGG_FLP_ENUM_DNS_RCODE, 0, text, sizeof text, NULL) == NFAGG_EINVAL);
    puts("metrics content host check ok");
    return 0;
}
