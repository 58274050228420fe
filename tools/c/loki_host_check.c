/* loki_host_check.c — the host side of write loki driven from plain C, without a handle and without a device: every refusal of
 * nfagg_loki_table_create's spec with its message, and the table over a nfagg_k8s_table_create(NULL, ...) and a
 * nfagg_net_table_create(NULL, ...): the blocks without the masked keys (nfagg_loki_render), the label classes with their
 * presence rule, a text of every byte value and texts that are not valid UTF-8 (truncated, overlong, a surrogate, above
 * U+10FFFF), which count as absent and leave the line. Meant to be linked against a build of the library whose host code
 * carries -fsanitize=address,undefined: the sanitizers then see the block parser, the unescaper and the UTF-8 check. Prints
 * "loki host check ok" and returns 0.
 *   cc -std=c11 -O1 -g -fsanitize=address,undefined -I include tools/c/loki_host_check.c -o loki_host_check -L <libdir> -lnfagg -Wl,-rpath,<libdir> */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "nfagg.h"

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: %s\n  last error: %s\n", __FILE__, __LINE__, #cond, nfagg_last_error(NULL)); exit(1); } } while (0)

enum { NS = 0, NAME = 1, KIND = 2, OWNER = 3, ZONE = 8 };

static nfagg_k8s_entry row(uint8_t last, const char* ns, const char* name, uint32_t name_len, const char* owner, uint32_t owner_len) {
    nfagg_k8s_entry e;
    memset(&e, 0, sizeof e);
    e.ip[10] = e.ip[11] = 0xff; e.ip[12] = 10; e.ip[15] = last;
    e.namespace_ = ns; e.namespace_len = (uint32_t)strlen(ns);
    e.name = name; e.name_len = name_len;
    e.kind = "Pod"; e.kind_len = 3;
    e.owner_name = owner; e.owner_name_len = owner_len;
    return e;
}

static nfagg_loki_spec spec(uint32_t labels, uint32_t ignore) {
    nfagg_loki_spec s;
    memset(&s, 0, sizeof s);
    s.struct_size = sizeof s; s.label_keys = labels; s.ignore_keys = ignore;
    s.timestamp_source = NFAGG_LOKI_TS_TIME_FLOW_END_MS; s.timestamp_scale = 1e6; s.batch_size = 100 * 1024;
    return s;
}

static int has(const char* buf, size_t n, const char* what) {
    const size_t w = strlen(what);
    for (size_t k = 0; k + w <= n; k++) if (memcmp(buf + k, what, w) == 0) return 1;
    return 0;
}

int main(void) {
    static char all[256];
    for (int k = 0; k < 256; k++) all[k] = (char)k;
    nfagg_k8s_entry rows[10] = {
        row(1, "shop", "a", 1, "cart", 4),
        row(2, "shop", "b", 1, "cart", 4),                     /* the class of row 0 over (namespace, owner name) */
        row(3, "", "c", 1, "", 0),                             /* namespace absent, owner name "" present */
        row(4, "shop", "d", 1, "\xc3", 1),                     /* truncated sequence */
        row(5, "shop", "e", 1, "\xc0\xaf", 2),                 /* overlong */
        row(6, "shop", "f", 1, "\xed\xa0\x80", 3),             /* a surrogate */
        row(7, "shop", "g", 1, "\xf4\x90\x80\x80", 4),         /* above U+10FFFF */
        row(8, "shop", "h", 1, "caf\xc3\xa9 \xe2\x82\xac \xf0\x9f\x98\x80", 14),     /* valid two-, three- and four-byte sequences */
        row(9, "shop", all + 1, 120, "q\"b\\\t\n\r\x01", 8),   /* every escape in a label value, bytes 1..120 in a line value */
        row(10, "shop", all + 121, 135, "cart", 4),            /* bytes 121..255 in a field that is no label: stays in the line as it is */
    };
    nfagg_k8s_table* k8s = NULL;
    CHECK(nfagg_k8s_table_create(NULL, rows, 10, NULL, &k8s) == NFAGG_OK && k8s);
    nfagg_net_label labels[5] = {{"lan", 3, 0}, {"", 0, 0}, {"lan", 3, 0}, {"x\xff", 2, 0}, {all + 1, 40, 0}};
    nfagg_net_rules rules = {sizeof rules, NFAGG_NET_SUBNET_LABELS, NULL, labels, 0, 5};
    nfagg_net_table* net = NULL;
    CHECK(nfagg_net_table_create(NULL, &rules, &net) == NFAGG_OK && net);

    /* the spec's refusals */
    nfagg_loki_table* t = NULL;
    nfagg_loki_spec s = spec(0, 0);
    s.struct_size = 8;
    CHECK(nfagg_loki_table_create(NULL, k8s, net, &s, &t) == NFAGG_EINVAL && !t && strstr(nfagg_last_error(NULL), "struct_size"));
    s = spec(NFAGG_DIM_PROTO, 0);
    CHECK(nfagg_loki_table_create(NULL, k8s, net, &s, &t) == NFAGG_EINVAL && !t && strstr(nfagg_last_error(NULL), "label_keys: unknown key bits 0x400000"));
    s = spec(0, 1u << 31);
    CHECK(nfagg_loki_table_create(NULL, k8s, net, &s, &t) == NFAGG_EINVAL && !t && strstr(nfagg_last_error(NULL), "ignore_keys: unknown key bits 0x80000000"));
    s = spec(NFAGG_LOKI_KEY_HASH_ID, 0);
    CHECK(nfagg_loki_table_create(NULL, k8s, net, &s, &t) == NFAGG_EINVAL && !t && strstr(nfagg_last_error(NULL), "_HashId as a label"));
    s = spec(NFAGG_LOKI_KEY_HASH_ID, NFAGG_LOKI_KEY_HASH_ID);                      /* ignored as well: the ignore list wins */
    CHECK(nfagg_loki_table_create(NULL, k8s, net, &s, &t) == NFAGG_OK && t);
    nfagg_loki_table_destroy(t); t = NULL;
    s = spec(0, 0); s.timestamp_source = 3;
    CHECK(nfagg_loki_table_create(NULL, k8s, net, &s, &t) == NFAGG_EINVAL && !t && strstr(nfagg_last_error(NULL), "unknown timestamp source 3"));
    const double bad_scale[4] = {0.0, -1.0, INFINITY, NAN};
    for (int k = 0; k < 4; k++) {
        s = spec(0, 0); s.timestamp_scale = bad_scale[k];
        CHECK(nfagg_loki_table_create(NULL, k8s, net, &s, &t) == NFAGG_EINVAL && !t && strstr(nfagg_last_error(NULL), "timestamp_scale"));
    }
    s = spec(0, 0); s.batch_size = 0;
    CHECK(nfagg_loki_table_create(NULL, k8s, net, &s, &t) == NFAGG_EINVAL && !t && strstr(nfagg_last_error(NULL), "batch_size 0"));
    s = spec(0, 0); s.batch_size = 1u << 31;
    CHECK(nfagg_loki_table_create(NULL, k8s, net, &s, &t) == NFAGG_EINVAL && !t);
    s = spec(0, 0); s.batch_size = (1u << 31) - 1;
    CHECK(nfagg_loki_table_create(NULL, k8s, net, &s, &t) == NFAGG_OK && t);
    CHECK(nfagg_loki_n_classes(t, 0) == 0 && nfagg_loki_n_classes(t, 1) == 0 && nfagg_loki_n_classes(t, 2) == 0 && nfagg_loki_n_classes(NULL, 0) == 0);
    nfagg_loki_table_destroy(t); t = NULL;
    s = spec(0, 0);
    CHECK(nfagg_loki_table_create(NULL, NULL, net, &s, &t) == NFAGG_EINVAL && nfagg_loki_table_create(NULL, k8s, NULL, &s, &t) == NFAGG_EINVAL);
    CHECK(nfagg_loki_table_create(NULL, k8s, net, NULL, &t) == NFAGG_EINVAL && nfagg_loki_table_create(NULL, k8s, net, &s, NULL) == NFAGG_EINVAL);

    /* labels: src namespace and owner name, dst owner name; ignored: both zones' key and the src kind */
    s = spec(NFAGG_DIM_SRC_K8S(NS) | NFAGG_DIM_SRC_K8S(OWNER) | NFAGG_DIM_DST_K8S(OWNER) | NFAGG_DIM_SRC_SUBNET_LABEL,
             NFAGG_DIM_SRC_K8S(KIND) | NFAGG_DIM_SRC_K8S(ZONE) | NFAGG_DIM_DST_K8S(ZONE));
    CHECK(nfagg_loki_table_create(NULL, k8s, net, &s, &t) == NFAGG_OK && t);
    /* src classes over (namespace, owner name): {0, 1, 9}, {2}, {3, 4, 5, 6} (the owner name is no text: only the namespace), {7}, {8} */
    CHECK(nfagg_loki_n_classes(t, 0) == 5);
    uint32_t r = 99;
    const uint32_t first[5] = {0, 2, 3, 7, 8};
    for (uint32_t c = 1; c <= 5; c++) CHECK(nfagg_loki_class_row(t, 0, c, &r) == NFAGG_OK && r == first[c - 1]);
    /* dst classes over the owner name alone: {0, 1, 9}, {2} (""), {7}, {8}; rows 3..6 have no label left: class 0 */
    CHECK(nfagg_loki_n_classes(t, 1) == 4);
    CHECK(nfagg_loki_class_row(t, 1, 4, &r) == NFAGG_OK && r == 8);
    CHECK(nfagg_loki_class_row(t, 1, 5, &r) == NFAGG_EINVAL && nfagg_loki_class_row(t, 1, 0, &r) == NFAGG_EINVAL && nfagg_loki_class_row(t, 2, 1, &r) == NFAGG_EINVAL);
    CHECK(nfagg_loki_class_row(NULL, 0, 1, &r) == NFAGG_EINVAL && nfagg_loki_class_row(t, 0, 1, NULL) == NFAGG_EINVAL);

    static char out[NFAGG_K8S_MAX_RENDERED], whole[NFAGG_K8S_MAX_RENDERED];
    size_t n = 0, nw = 0;
    CHECK(nfagg_loki_render(t, 0, 0, out, sizeof out, &n) == NFAGG_OK);
    CHECK(n == strlen(",\"SrcK8S_Name\":\"a\",\"SrcK8S_NetworkName\":\"\",\"SrcK8S_OwnerType\":\"\"") &&
          memcmp(out, ",\"SrcK8S_Name\":\"a\",\"SrcK8S_NetworkName\":\"\",\"SrcK8S_OwnerType\":\"\"", n) == 0);
    CHECK(nfagg_loki_render(t, 1, 0, out, sizeof out, &n) == NFAGG_OK && !has(out, n, "OwnerName") && has(out, n, ",\"DstK8S_Namespace\":\"shop\"") && has(out, n, "DstK8S_Type"));
    CHECK(nfagg_loki_render(t, 0, 0, out, n ? 1 : 0, &n) == NFAGG_TRUNCATED && nfagg_loki_render(t, 0, 0, NULL, 0, &n) == NFAGG_TRUNCATED);
    for (uint32_t bad = 3; bad <= 6; bad++)                    /* not valid UTF-8: gone from the line on the sides where it is a label */
        for (int side = 0; side < 2; side++)
            CHECK(nfagg_loki_render(t, side, bad, out, sizeof out, &n) == NFAGG_OK && !has(out, n, "OwnerName") && has(out, n, "K8S_Name\":"));
    /* a field that is no label keeps every byte: the block is the table's own less the masked keys */
    nfagg_k8s_entry e9 = rows[9];
    CHECK(nfagg_k8s_render(&e9, 1, whole, sizeof whole, &nw) == NFAGG_OK);
    CHECK(nfagg_loki_render(t, 1, 9, out, sizeof out, &n) == NFAGG_OK && n == nw - strlen(",\"DstK8S_OwnerName\":\"cart\"") && has(out, n, "\xfe\xff\""));
    CHECK(nfagg_loki_render(t, 0, 8, out, sizeof out, &n) == NFAGG_OK && has(out, n, "\\u0001") && !has(out, n, "OwnerName") && !has(out, n, "Namespace"));
    CHECK(nfagg_loki_render(t, 2, 0, out, sizeof out, &n) == NFAGG_EINVAL && nfagg_loki_render(t, 0, 10, out, sizeof out, &n) == NFAGG_EINVAL);
    CHECK(nfagg_loki_render(NULL, 0, 0, out, sizeof out, &n) == NFAGG_EINVAL && nfagg_loki_render(t, 0, 0, out, sizeof out, NULL) == NFAGG_EINVAL);
    nfagg_loki_table_destroy(t);

    /* every maskable key alone, as a label and as ignored: the table builds, and a masked Kubernetes key is in no block */
    static const char* const kNames[9] = {"Namespace", "Name", "Type", "OwnerName", "OwnerType", "NetworkName", "HostIP", "HostName", "Zone"};
    for (int bit = 0; bit < 25; bit++) {
        if (bit == 22) continue;                               /* Proto: not maskable */
        for (int ign = 0; ign < 2; ign++) {
            if (!ign && (1u << bit) == NFAGG_LOKI_KEY_HASH_ID) continue;
            s = ign ? spec(0, 1u << bit) : spec(1u << bit, 0);
            t = NULL;
            CHECK(nfagg_loki_table_create(NULL, k8s, net, &s, &t) == NFAGG_OK && t);
            if (bit < 18) {
                char key[40];
                snprintf(key, sizeof key, "%sK8S_%s\":", bit < 9 ? "Src" : "Dst", kNames[bit % 9]);
                for (uint32_t k = 0; k < 10; k++) CHECK(nfagg_loki_render(t, bit / 9, k, out, sizeof out, &n) == NFAGG_OK && !has(out, n, key));
                CHECK((!ign || nfagg_loki_n_classes(t, bit / 9) == 0) && nfagg_loki_n_classes(t, 1 - bit / 9) == 0);
            }
            nfagg_loki_table_destroy(t);
        }
    }
    nfagg_loki_table_destroy(NULL);
    nfagg_net_table_destroy(net);
    nfagg_k8s_table_destroy(k8s);
    CHECK(nfagg_loki_max_entry(0) == nfagg_flp_json_conn_max_line(0) - 1 + 27 && nfagg_loki_max_entry(7) == 0);
    printf("loki host check ok\n");
    return 0;
}
