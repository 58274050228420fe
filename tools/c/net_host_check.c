/* net_host_check.c — the host side of the transform network rules driven from plain C, without a handle and without a device:
 * nfagg_net_table_create(NULL, ...) and nfagg_net_render over labels that stress the escaper and the cap (every byte value, a
 * label that escapes to 256 and to 257 bytes, a null label with a length), every refusal of a CIDR, the list and the labels
 * at their caps, the family normalisation of prefixes 0..32 and 0..128, and nfagg_k8s_table_create(NULL, ...) with host IPs to
 * intern (the empty one, repeats, 1000 distinct ones, a text of every byte value). Meant to be linked against a build of the
 * library whose host code carries -fsanitize=address,undefined: the sanitizers then see the render buffer, the escaper, the
 * masks and the interning. Prints "net host check ok" and returns 0.
 *   cc -std=c11 -O1 -g -fsanitize=address,undefined -I include tools/c/net_host_check.c -o net_host_check -L <libdir> -lnfagg -Wl,-rpath,<libdir> */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "nfagg.h"

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: %s\n  last error: %s\n", __FILE__, __LINE__, #cond, nfagg_last_error(NULL)); exit(1); } } while (0)

static nfagg_net_cidr cidr(const uint8_t ip[16], uint32_t ones, uint32_t bits, uint32_t label) {
    nfagg_net_cidr c;
    memset(&c, 0, sizeof c);
    memcpy(c.ip, ip, 16);
    c.ones = ones; c.bits = bits; c.label = label;
    return c;
}

static int create(uint32_t flags, const nfagg_net_cidr* cidrs, uint32_t n_cidrs, const nfagg_net_label* labels, uint32_t n_labels, nfagg_net_table** t) {
    nfagg_net_rules r = {sizeof r, flags, cidrs, labels, n_cidrs, n_labels};
    return nfagg_net_table_create(NULL, &r, t);
}

int main(void) {
    static const uint8_t v4[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0xff, 0xff, 10, 1, 2, 3};
    static const uint8_t v6[16] = {0x20, 0x01, 0x0d, 0xb8, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff};
    static char out[NFAGG_NET_LABEL_MAX + 32];
    nfagg_net_table* t = NULL;
    size_t n = 0;

    /* labels: every byte value in pieces that fit the cap, one at the cap by escapes, the empty one */
    char all[256];
    for (int k = 0; k < 256; k++) all[k] = (char)k;
    char cap[46];
    memset(cap, 1, 42); memcpy(cap + 42, "nnnn", 4);                  /* 42 x 6 + 4 = 256 */
    nfagg_net_label labels[8] = {{all, 32, 0}, {all + 32, 100, 0}, {all + 132, 124, 0}, {cap, 46, 0}, {"", 0, 0}, {NULL, 0, 0}, {"plain", 5, 0}, {all + 9, 2, 0}};
    CHECK(create(7, NULL, 0, labels, 8, &t) == NFAGG_OK && t);
    for (int side = 0; side < 2; side++) {
        CHECK(nfagg_net_render(t, side, 3, out, sizeof out, &n) == NFAGG_OK && n == 20 + NFAGG_NET_LABEL_MAX && out[n - 1] == '"');
        CHECK(memcmp(out, side ? ",\"DstSubnetLabel\":\"\\u0001" : ",\"SrcSubnetLabel\":\"\\u0001", 25) == 0);
        CHECK(nfagg_net_render(t, side, 3, out, n - 1, &n) == NFAGG_TRUNCATED && nfagg_net_render(t, side, 3, NULL, 0, &n) == NFAGG_TRUNCATED);
        CHECK(nfagg_net_render(t, side, 0, out, sizeof out, &n) == NFAGG_OK && n == 20 + 29 * 6 + 3 * 2);       /* 0x00..0x1f: \t \n \r short */
        CHECK(nfagg_net_render(t, side, 1, out, sizeof out, &n) == NFAGG_OK && n == 20 + 100 + 2);               /* the quote and the backslash */
        CHECK(nfagg_net_render(t, side, 2, out, sizeof out, &n) == NFAGG_OK && n == 20 + 124);                   /* 0x84..0xff copied */
        CHECK(nfagg_net_render(t, side, 4, out, sizeof out, &n) == NFAGG_OK && n == 0);
        CHECK(nfagg_net_render(t, side, 5, out, 0, &n) == NFAGG_OK && n == 0);
        CHECK(nfagg_net_render(t, side, 7, out, sizeof out, &n) == NFAGG_OK && n == 24 && memcmp(out + 19, "\\t\\n\"", 5) == 0);
    }
    CHECK(nfagg_net_render(t, 2, 0, out, sizeof out, &n) == NFAGG_EINVAL && nfagg_net_render(t, 0, 8, out, sizeof out, &n) == NFAGG_EINVAL);
    CHECK(nfagg_net_render(NULL, 0, 0, out, sizeof out, &n) == NFAGG_EINVAL && nfagg_net_render(t, 0, 0, out, sizeof out, NULL) == NFAGG_EINVAL);
    nfagg_net_table_destroy(t);

    /* one byte over the cap, by an escape and by length; a length without its string */
    char over[258];
    memset(over, 1, 42); memcpy(over + 42, "nnnnn", 5);
    nfagg_net_label bad[2] = {{"ok", 2, 0}, {over, 47, 0}};
    CHECK(create(0, NULL, 0, bad, 2, &t) == NFAGG_EINVAL && !t && strstr(nfagg_last_error(NULL), "net label 1: its escaped value has 257 bytes, the cap is 256"));
    memset(over, 'n', sizeof over);
    bad[1].len = 257;
    CHECK(create(0, NULL, 0, bad, 2, &t) == NFAGG_EINVAL && !t && strstr(nfagg_last_error(NULL), "net label 1: its escaped value has more than 256 bytes"));
    bad[1].len = 256;
    CHECK(create(0, NULL, 0, bad, 2, &t) == NFAGG_OK && t);
    nfagg_net_table_destroy(t);
    bad[1].text = NULL; bad[1].len = 3;
    CHECK(create(0, NULL, 0, bad, 2, &t) == NFAGG_EINVAL && !t && strstr(nfagg_last_error(NULL), "net label 1: null string with a length"));

    /* every prefix length of both families, the v4-mapped address in IPv6 text too: the masks and the family test */
    enum { ALL = 33 + 129 + 129 };
    nfagg_net_cidr* cs = calloc(NFAGG_NET_MAX_CIDRS + 1, sizeof *cs);
    CHECK(cs != NULL);
    uint32_t k = 0;
    for (uint32_t ones = 0; ones <= 32; ones++) cs[k++] = cidr(v4, ones, 32, ones % 2);
    for (uint32_t ones = 0; ones <= 128; ones++) cs[k++] = cidr(v6, ones, 128, ones % 2);
    for (uint32_t ones = 0; ones <= 128; ones++) cs[k++] = cidr(v4, ones, 128, ones % 2);
    CHECK(k == ALL && create(NFAGG_NET_SUBNET_LABELS, cs, k, labels, 2, &t) == NFAGG_OK && t);
    nfagg_net_table_destroy(t);

    /* the list at its cap and one over; the labels at their cap and one over */
    for (k = 0; k < NFAGG_NET_MAX_CIDRS + 1; k++) cs[k] = cidr(v4, k % 33, 32, 0);
    CHECK(create(2, cs, NFAGG_NET_MAX_CIDRS, labels, 1, &t) == NFAGG_OK && t);
    nfagg_net_table_destroy(t);
    CHECK(create(2, cs, NFAGG_NET_MAX_CIDRS + 1, labels, 1, &t) == NFAGG_EINVAL && !t && strstr(nfagg_last_error(NULL), "1025 CIDRs, more than 1024"));
    nfagg_net_label* many = calloc(NFAGG_NET_MAX_CIDRS + 1, sizeof *many);
    CHECK(many != NULL);
    for (k = 0; k < NFAGG_NET_MAX_CIDRS + 1; k++) { many[k].text = cap; many[k].len = 46; }
    CHECK(create(2, cs, 4, many, NFAGG_NET_MAX_CIDRS, &t) == NFAGG_OK && t);
    CHECK(nfagg_net_render(t, 1, NFAGG_NET_MAX_CIDRS - 1, out, sizeof out, &n) == NFAGG_OK && n == 20 + NFAGG_NET_LABEL_MAX);
    nfagg_net_table_destroy(t);
    CHECK(create(2, cs, 4, many, NFAGG_NET_MAX_CIDRS + 1, &t) == NFAGG_EINVAL && !t && strstr(nfagg_last_error(NULL), "1025 labels, more than 1024"));
    free(many);

    /* every refusal of a CIDR names it */
    cs[0] = cidr(v4, 8, 32, 0); cs[1] = cidr(v4, 33, 32, 0);
    CHECK(create(2, cs, 2, labels, 1, &t) == NFAGG_EINVAL && !t && strstr(nfagg_last_error(NULL), "CIDR 1: a prefix of 33 in 32 bits"));
    cs[1] = cidr(v6, 129, 128, 0);
    CHECK(create(2, cs, 2, labels, 1, &t) == NFAGG_EINVAL && !t && strstr(nfagg_last_error(NULL), "CIDR 1: a prefix of 129 in 128 bits"));
    cs[1] = cidr(v6, 8, 64, 0);
    CHECK(create(2, cs, 2, labels, 1, &t) == NFAGG_EINVAL && !t && strstr(nfagg_last_error(NULL), "CIDR 1: 64 bits, neither 32 nor 128"));
    cs[1] = cidr(v4, 8, 32, 1);
    CHECK(create(2, cs, 2, labels, 1, &t) == NFAGG_EINVAL && !t && strstr(nfagg_last_error(NULL), "CIDR 1: label 1 of 1"));
    cs[1] = cidr(v6, 8, 32, 0);
    CHECK(create(2, cs, 2, labels, 1, &t) == NFAGG_EINVAL && !t && strstr(nfagg_last_error(NULL), "CIDR 1: 32 bits and an address that is not v4-mapped"));
    CHECK(create(8, cs, 1, labels, 1, &t) == NFAGG_EINVAL && !t && create(2, NULL, 1, labels, 1, &t) == NFAGG_EINVAL && create(2, cs, 1, NULL, 1, &t) == NFAGG_EINVAL);
    nfagg_net_rules r = {8, 0, NULL, NULL, 0, 0};
    CHECK(nfagg_net_table_create(NULL, &r, &t) == NFAGG_EINVAL && nfagg_net_table_create(NULL, NULL, &t) == NFAGG_EINVAL);
    r.struct_size = sizeof r;
    CHECK(nfagg_net_table_create(NULL, &r, NULL) == NFAGG_EINVAL);
    CHECK(nfagg_net_table_create(NULL, &r, &t) == NFAGG_OK && t);        /* no rule, no CIDR, no label */
    nfagg_net_table_destroy(t);
    nfagg_net_table_destroy(NULL);
    free(cs);

    /* the Kubernetes table interns its rows' host IPs: the empty one, repeats, 1000 distinct ones, a text of every byte value */
    enum { ROWS = 1200 };
    nfagg_k8s_entry* rows = calloc(ROWS, sizeof *rows);
    static char hosts[ROWS][24];
    CHECK(rows != NULL);
    for (int i = 0; i < ROWS; i++) {
        rows[i].ip[15] = (uint8_t)i; rows[i].ip[14] = (uint8_t)(i >> 8);
        rows[i].name = "pod"; rows[i].name_len = 3;
        if (i % 6 == 0) continue;                                   /* no host IP */
        snprintf(hosts[i], sizeof hosts[i], "10.0.%d.%d", (i % 1000) >> 8, (i % 1000) & 255);
        rows[i].host_ip = hosts[i]; rows[i].host_ip_len = (uint32_t)strlen(hosts[i]);
    }
    rows[1].host_ip = all; rows[1].host_ip_len = 256;
    rows[2].host_ip = "<nil>"; rows[2].host_ip_len = 5;
    nfagg_k8s_table* kt = NULL;
    CHECK(nfagg_k8s_table_create(NULL, rows, ROWS, NULL, &kt) == NFAGG_OK && kt);
    nfagg_k8s_table_destroy(kt);
    free(rows);
    puts("net host check ok");
    return 0;
}
