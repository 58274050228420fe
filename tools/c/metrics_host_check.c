/* metrics_host_check.c — the host side of the flow metrics driven from plain C, without a handle and without a device:
 * nfagg_k8s_table_create(NULL, ...) over a handful of rows, nfagg_metrics_table_create(NULL, ...) over groupings that select
 * fields of one side, of both and of none, the classes of every row through nfagg_metrics_class_row (rows that differ only in
 * an unselected field, an empty zone against an absent one, a host name without a host IP, a text of every byte value), and
 * every NFAGG_EINVAL path of the three calls. Meant to be linked against a build of the library whose host code carries
 * -fsanitize=address,undefined: the sanitizers then see the interning, the tuples and the class arrays. Prints "metrics host
 * check ok" and returns 0.
 *   cc -std=c11 -O1 -g -fsanitize=address,undefined -I include tools/c/metrics_host_check.c -o metrics_host_check -L <libdir> -lnfagg -Wl,-rpath,<libdir> */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "nfagg.h"

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: %s\n  last error: %s\n", __FILE__, __LINE__, #cond, nfagg_last_error(NULL)); exit(1); } } while (0)

enum { NS = 0, NAME = 1, KIND = 2, HOST_IP = 6, HOST_NAME = 7, ZONE = 8 };

static nfagg_k8s_entry row(uint8_t last, const char* ns, const char* name, const char* host_ip, const char* host_name, const char* zone) {
    nfagg_k8s_entry e;
    memset(&e, 0, sizeof e);
    e.ip[10] = e.ip[11] = 0xff; e.ip[12] = 10; e.ip[15] = last;
    e.namespace_ = ns; e.namespace_len = (uint32_t)strlen(ns);
    e.name = name; e.name_len = (uint32_t)strlen(name);
    e.kind = "Pod"; e.kind_len = 3;
    e.host_ip = host_ip; e.host_ip_len = (uint32_t)strlen(host_ip);
    e.host_name = host_name; e.host_name_len = (uint32_t)strlen(host_name);
    if (zone) { e.zone = zone; e.zone_len = (uint32_t)strlen(zone); e.has_zone = 1; }
    return e;
}

/* the class of entry r in grouping g, side: the class whose first row's class equals r's — found through class_row alone */
static uint32_t first_row_of(const nfagg_metrics_table* t, uint32_t g, int side, uint32_t cls) {
    uint32_t r = 12345;
    CHECK(nfagg_metrics_class_row(t, g, side, cls, &r) == NFAGG_OK);
    return r;
}

int main(void) {
    static char all[256];
    for (int k = 0; k < 256; k++) all[k] = (char)k;
    nfagg_k8s_entry rows[8] = {
        row(1, "shop", "a", "10.9.0.1", "node-1", "z1"),
        row(2, "shop", "b", "10.9.0.1", "node-1", "z1"),      /* differs from row 0 in the name only */
        row(3, "shop", "a", "", "node-1", ""),                 /* no host IP: the host name is absent too; an empty zone */
        row(4, "shop", "a", "", "other", NULL),                /* no zone at all */
        row(5, "", "a", "10.9.0.2", "", "z1"),                 /* no namespace, a host IP without a host name */
        row(6, "shop", "a", "10.9.0.1", "node-1", "z1"),       /* row 0 again under another address */
        row(7, "shop", "a", "", "", ""),
        row(8, "shop", "a", "", "", ""),
    };
    rows[7].name = all; rows[7].name_len = 256;                /* a text of every byte value */
    nfagg_k8s_table* k8s = NULL;
    CHECK(nfagg_k8s_table_create(NULL, rows, 8, NULL, &k8s) == NFAGG_OK && k8s);

    const uint32_t dims[5] = {
        NFAGG_DIM_SRC_K8S(NS) | NFAGG_DIM_SRC_K8S(HOST_IP) | NFAGG_DIM_DST_K8S(NAME),   /* name unselected on the src side */
        NFAGG_DIM_SRC_K8S(ZONE),
        NFAGG_DIM_DST_K8S(HOST_NAME),
        NFAGG_DIM_PROTO | NFAGG_DIM_FLOW_LAYER,                                          /* no field of either side */
        NFAGG_DIM_ALL,
    };
    nfagg_metrics_table* t = NULL;
    CHECK(nfagg_metrics_table_create(NULL, k8s, dims, 5, &t) == NFAGG_OK && t);
    /* grouping 0, src: (namespace, host IP): {0, 1, 5}, {2, 3, 6, 7}, {4}; dst: name: {0, 2, 3, 4, 5, 6}, {1}, {7} */
    CHECK(nfagg_metrics_n_classes(t, 0, 0) == 3 && nfagg_metrics_n_classes(t, 0, 1) == 3);
    CHECK(first_row_of(t, 0, 0, 1) == 0 && first_row_of(t, 0, 0, 2) == 2 && first_row_of(t, 0, 0, 3) == 4);
    CHECK(first_row_of(t, 0, 1, 1) == 0 && first_row_of(t, 0, 1, 2) == 1 && first_row_of(t, 0, 1, 3) == 7);
    CHECK(first_row_of(t, 0, 0, 0) == NFAGG_K8S_NO_ROW && first_row_of(t, 0, 1, 0) == NFAGG_K8S_NO_ROW);
    /* grouping 1, src zone: "z1" {0, 1, 4, 5}, "" {2, 6, 7}, absent {3}: the empty and the absent zone are two classes */
    CHECK(nfagg_metrics_n_classes(t, 1, 0) == 3 && nfagg_metrics_n_classes(t, 1, 1) == 0);
    CHECK(first_row_of(t, 1, 0, 1) == 0 && first_row_of(t, 1, 0, 2) == 2 && first_row_of(t, 1, 0, 3) == 3);
    /* grouping 2, dst host name: present only with a host IP: "node-1" {0, 1, 5}, absent {2, 3, 4, 6, 7} */
    CHECK(nfagg_metrics_n_classes(t, 2, 1) == 2 && first_row_of(t, 2, 1, 1) == 0 && first_row_of(t, 2, 1, 2) == 2);
    CHECK(nfagg_metrics_n_classes(t, 3, 0) == 0 && nfagg_metrics_n_classes(t, 3, 1) == 0 && first_row_of(t, 3, 0, 0) == NFAGG_K8S_NO_ROW);
    /* every field: rows 0 and 5 are one class, and so are rows 2 and 6 (a host name without a host IP is absent); row 7 differs in the name */
    CHECK(nfagg_metrics_n_classes(t, 4, 0) == 6 && nfagg_metrics_n_classes(t, 4, 1) == 6 && first_row_of(t, 4, 0, 6) == 7 && first_row_of(t, 4, 1, 3) == 2);

    /* arguments out of range */
    uint32_t r = 0;
    CHECK(nfagg_metrics_n_classes(t, 5, 0) == 0 && nfagg_metrics_n_classes(t, 0, 2) == 0 && nfagg_metrics_n_classes(NULL, 0, 0) == 0);
    CHECK(nfagg_metrics_class_row(t, 5, 0, 0, &r) == NFAGG_EINVAL && nfagg_metrics_class_row(t, 0, 2, 0, &r) == NFAGG_EINVAL);
    CHECK(nfagg_metrics_class_row(t, 0, 0, 4, &r) == NFAGG_EINVAL && strstr(nfagg_last_error(NULL), "class 4 of 3"));
    CHECK(nfagg_metrics_class_row(t, 0, 0, 1, NULL) == NFAGG_EINVAL && nfagg_metrics_class_row(NULL, 0, 0, 1, &r) == NFAGG_EINVAL);
    nfagg_metrics_table_destroy(t);

    /* the refusals of the table */
    const uint32_t bad[2] = {NFAGG_DIM_PROTO, 1u << 23};
    const uint32_t nine[9] = {1, 2, 3, 4, 5, 6, 7, 8, 9};
    t = (nfagg_metrics_table*)&r;
    CHECK(nfagg_metrics_table_create(NULL, k8s, bad, 2, &t) == NFAGG_EINVAL && !t && strstr(nfagg_last_error(NULL), "grouping 1: unknown dimension bits 0x800000"));
    CHECK(nfagg_metrics_table_create(NULL, k8s, nine, 9, &t) == NFAGG_EINVAL && !t && strstr(nfagg_last_error(NULL), "9 groupings"));
    CHECK(nfagg_metrics_table_create(NULL, k8s, nine, 0, &t) == NFAGG_EINVAL && !t);
    CHECK(nfagg_metrics_table_create(NULL, NULL, nine, 1, &t) == NFAGG_EINVAL && nfagg_metrics_table_create(NULL, k8s, NULL, 1, &t) == NFAGG_EINVAL);
    CHECK(nfagg_metrics_table_create(NULL, k8s, nine, 1, NULL) == NFAGG_EINVAL);
    CHECK(nfagg_metrics_table_create(NULL, k8s, nine, 8, &t) == NFAGG_OK && t);          /* eight groupings: the cap */
    nfagg_metrics_table_destroy(t);
    nfagg_metrics_table_destroy(NULL);
    nfagg_k8s_table_destroy(k8s);

    /* an empty Kubernetes table: every grouping has no class */
    CHECK(nfagg_k8s_table_create(NULL, NULL, 0, NULL, &k8s) == NFAGG_OK && k8s);
    CHECK(nfagg_metrics_table_create(NULL, k8s, dims, 5, &t) == NFAGG_OK && t && nfagg_metrics_n_classes(t, 4, 0) == 0);
    nfagg_metrics_table_destroy(t);
    /* the fold refuses a table built without a handle, and a null handle */
    uint32_t cap = 4, n_groups = 0;
    nfagg_metric_group* out = NULL;
    CHECK(nfagg_metrics_fold(NULL, NULL, NULL, 0, NULL, NULL, &cap, &out, &n_groups) == NFAGG_EINVAL);
    CHECK(nfagg_metrics_fold_device(NULL, NULL, NULL, 0, NULL, NULL, &cap, &out, &n_groups) == NFAGG_EINVAL);
    nfagg_k8s_table_destroy(k8s);
    puts("metrics host check ok");
    return 0;
}
