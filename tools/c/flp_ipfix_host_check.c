/* flp_ipfix_host_check.c — the host-only entry points of write ipfix driven from plain C, without a handle and without a
 * device: nfagg_flp_ipfix_template for both families with and without an enterprise number (sizes, the set and record headers,
 * the enterprise bit and number, truncation, the refusals) and nfagg_flp_ipfix_strings_create(NULL, ...): strings of 0, 1, 254,
 * 255, 256 and 1024 bytes in each position, every byte value, a string of 1025 bytes, a null pointer with a length. Meant to be
 * linked against a build of the library whose host code carries -fsanitize=address,undefined: the sanitizers then see the
 * template writer and the table builder. Prints "flp ipfix host check ok" and returns 0.
 *   cc -std=c11 -O1 -g -fsanitize=address,undefined -I include tools/c/flp_ipfix_host_check.c -o flp_ipfix_host_check -L <libdir> -lnfagg -Wl,-rpath,<libdir> */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "nfagg.h"

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: %s\n  last error: %s\n", __FILE__, __LINE__, #cond, nfagg_last_error(NULL)); exit(1); } } while (0)

static unsigned be16(const unsigned char* p) { return (unsigned)p[0] << 8 | p[1]; }
static unsigned long be32(const unsigned char* p) { return (unsigned long)be16(p) << 16 | be16(p + 2); }

static nfagg_flp_ipfix_options options(uint32_t enterprise) {
    nfagg_flp_ipfix_options o;
    memset(&o, 0, sizeof o);
    o.struct_size = sizeof o;
    o.export_time_s = 1700000000u; o.seq0 = 42; o.obs_domain_id = 1; o.template_id_v4 = 256; o.template_id_v6 = 257;
    o.enterprise_id = enterprise; o.max_msg_size = 512;
    return o;
}

static nfagg_k8s_entry entry(uint8_t last, const char* ns, uint32_t ns_len, const char* name, uint32_t name_len, const char* host, uint32_t host_len) {
    nfagg_k8s_entry e;
    memset(&e, 0, sizeof e);
    e.ip[10] = e.ip[11] = 0xff; e.ip[12] = 10; e.ip[15] = last;
    e.namespace_ = ns; e.namespace_len = ns_len;
    e.name = name; e.name_len = name_len;
    e.host_ip = "10.0.0.1"; e.host_ip_len = 8;
    e.host_name = host; e.host_name_len = host_len;
    return e;
}

int main(void) {
    static unsigned char out[256];
    size_t n = 0;
    /* the templates: 16 + 4 + 4 + 4 * fields, + 8 for each of the nine enterprise elements */
    for (int v6 = 0; v6 < 2; v6++)
        for (int ent = 0; ent < 2; ent++) {
            nfagg_flp_ipfix_options o = options(ent ? 2 : 0);
            const unsigned fields = (v6 ? 24 : 23) + (ent ? 9 : 0);
            const size_t want = 24 + 4 * (size_t)(v6 ? 24 : 23) + (ent ? 72 : 0);
            memset(out, 0xAB, sizeof out);
            CHECK(nfagg_flp_ipfix_template(&o, v6, out, sizeof out, &n) == NFAGG_OK && n == want);
            CHECK(be16(out) == 10 && be16(out + 2) == want && be32(out + 4) == 1700000000ul && be32(out + 8) == 42 && be32(out + 12) == 1);
            CHECK(be16(out + 16) == 2 && be16(out + 18) == want - 16 && be16(out + 20) == (v6 ? 257u : 256u) && be16(out + 22) == fields);
            CHECK(be16(out + 24) == (v6 ? 27u : 8u) && be16(out + 26) == (v6 ? 16u : 4u));          /* source address first */
            CHECK(out[want] == 0xAB);
            if (ent) {                                                                              /* directions last: 7742, variable, enterprise 2 */
                CHECK(be16(out + want - 8) == (7742u | 0x8000u) && be16(out + want - 6) == 65535u && be32(out + want - 4) == 2);
                CHECK(be16(out + want - 24) == (7740u | 0x8000u) && be16(out + want - 22) == 8u);   /* timeFlowRttNs: fixed 8 */
            } else {
                CHECK(be16(out + want - 4) == 311u && be16(out + want - 2) == 8u);                  /* samplingProbability last */
            }
            memset(out, 0xAB, sizeof out);
            CHECK(nfagg_flp_ipfix_template(&o, v6, out, want - 1, &n) == NFAGG_TRUNCATED && n == want && out[0] == 0xAB);
            CHECK(nfagg_flp_ipfix_template(&o, v6, NULL, 0, &n) == NFAGG_TRUNCATED && n == want);
        }
    nfagg_flp_ipfix_options bad = options(0);
    bad.struct_size = 8;
    CHECK(nfagg_flp_ipfix_template(&bad, 0, out, sizeof out, &n) == NFAGG_EINVAL && strstr(nfagg_last_error(NULL), "struct_size"));
    bad = options(0);
    CHECK(nfagg_flp_ipfix_template(NULL, 0, out, sizeof out, &n) == NFAGG_EINVAL && nfagg_flp_ipfix_template(&bad, 0, out, sizeof out, NULL) == NFAGG_EINVAL);

    /* the strings table on the host */
    static char big[1025];
    for (int k = 0; k < 1025; k++) big[k] = (char)(k * 7 + 1);          /* every byte value, NUL included */
    static const uint32_t lens[6] = {0, 1, 254, 255, 256, 1024};
    nfagg_k8s_entry rows[18];
    int r = 0;
    for (int pos = 0; pos < 3; pos++)
        for (int l = 0; l < 6; l++, r++)
            rows[r] = entry((uint8_t)(r + 1), pos == 0 ? big : "ns", pos == 0 ? lens[l] : 2, pos == 1 ? big : "pod", pos == 1 ? lens[l] : 3,
                            pos == 2 ? big : "node", pos == 2 ? lens[l] : 4);
    nfagg_flp_ipfix_strings* t = NULL;
    CHECK(nfagg_flp_ipfix_strings_create(NULL, rows, 18, &t) == NFAGG_OK && t);
    nfagg_flp_ipfix_strings_destroy(t); t = NULL;
    CHECK(nfagg_flp_ipfix_strings_create(NULL, NULL, 0, &t) == NFAGG_OK && t);                      /* no row at all */
    nfagg_flp_ipfix_strings_destroy(t); t = NULL;
    nfagg_flp_ipfix_strings_destroy(NULL);
    for (int pos = 0; pos < 3; pos++) {                                                             /* 1025 bytes in each position */
        nfagg_k8s_entry e = entry(1, pos == 0 ? big : "ns", pos == 0 ? 1025 : 2, pos == 1 ? big : "pod", pos == 1 ? 1025 : 3, pos == 2 ? big : "node",
                                  pos == 2 ? 1025 : 4);
        CHECK(nfagg_flp_ipfix_strings_create(NULL, &e, 1, &t) == NFAGG_EINVAL && !t && strstr(nfagg_last_error(NULL), "1025 bytes"));
    }
    for (int pos = 0; pos < 3; pos++) {                                                             /* a null pointer with a length */
        nfagg_k8s_entry e = entry(1, pos == 0 ? NULL : "ns", 2, pos == 1 ? NULL : "pod", 3, pos == 2 ? NULL : "node", 4);
        CHECK(nfagg_flp_ipfix_strings_create(NULL, &e, 1, &t) == NFAGG_EINVAL && !t && strstr(nfagg_last_error(NULL), "null with a length"));
    }
    nfagg_k8s_entry e = entry(1, "ns", 2, "pod", 3, "node", 4);
    e.host_ip = NULL;
    CHECK(nfagg_flp_ipfix_strings_create(NULL, &e, 1, &t) == NFAGG_EINVAL && !t);
    CHECK(nfagg_flp_ipfix_strings_create(NULL, NULL, 1, &t) == NFAGG_EINVAL && nfagg_flp_ipfix_strings_create(NULL, rows, 1, NULL) == NFAGG_EINVAL);
    /* the writer lives on a device: without a handle it is refused */
    nfagg_flp_ipfix_writer* w = NULL;
    CHECK(nfagg_flp_ipfix_writer_create(NULL, &w) == NFAGG_EINVAL && !w);
    nfagg_flp_ipfix_writer_destroy(NULL);
    printf("flp ipfix host check ok\n");
    return 0;
}
