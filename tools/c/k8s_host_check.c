/* k8s_host_check.c — the host side of the Kubernetes enrichment driven from plain C, without a handle and without a device:
 * nfagg_k8s_render and nfagg_k8s_table_create(NULL, ...) over values that stress the escaper and the cap (every byte value,
 * 2048 bytes that each escape six-fold, blocks of 2048 and 2049 bytes, a null string with a length, duplicate addresses, a
 * layer). Meant to be linked against a build of the library whose host code carries -fsanitize=address,undefined: the
 * sanitizers then see the render buffer, the escaper and the table build. Prints "k8s host check ok" and returns 0.
 *   cc -std=c11 -O1 -g -fsanitize=address,undefined -I include tools/c/k8s_host_check.c -o k8s_host_check -L <libdir> -lnfagg -Wl,-rpath,<libdir> */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "nfagg.h"

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: %s\n  last error: %s\n", __FILE__, __LINE__, #cond, nfagg_last_error(NULL)); exit(1); } } while (0)

static nfagg_k8s_entry entry(const char* name, uint32_t name_len, uint8_t last) {
    nfagg_k8s_entry e;
    memset(&e, 0, sizeof e);
    e.ip[15] = last;
    e.name = name; e.name_len = name_len;
    return e;
}

int main(void) {
    static char out[NFAGG_K8S_MAX_RENDERED];
    size_t n = 0;

    /* every byte value in one value */
    char all[256];
    for (int k = 0; k < 256; k++) all[k] = (char)k;
    nfagg_k8s_entry e = entry(all, 256, 1);
    e.namespace_ = "ns"; e.namespace_len = 2;
    e.host_ip = "10.0.0.1"; e.host_ip_len = 8;
    e.host_name = "node"; e.host_name_len = 4;
    e.zone = ""; e.has_zone = 1;
    for (int side = 0; side < 2; side++) {
        CHECK(nfagg_k8s_render(&e, side, out, sizeof out, &n) == NFAGG_OK);
        CHECK(n > 256 + 181 && memcmp(out, side ? ",\"DstK8S_HostIP\":\"10.0.0.1\"" : ",\"SrcK8S_HostIP\":\"10.0.0.1\"", 27) == 0);
        CHECK(nfagg_k8s_render(&e, side, out, n - 1, &n) == NFAGG_TRUNCATED);
        CHECK(nfagg_k8s_render(&e, side, NULL, 0, &n) == NFAGG_TRUNCATED);
    }
    CHECK(nfagg_k8s_render(&e, 2, out, sizeof out, &n) == NFAGG_EINVAL);

    /* 2048 bytes that escape six-fold each: the escaper's largest output; the block is refused */
    static char ctl[NFAGG_K8S_MAX_RENDERED + 1];
    memset(ctl, 1, sizeof ctl);
    e = entry(ctl, NFAGG_K8S_MAX_RENDERED, 2);
    CHECK(nfagg_k8s_render(&e, 0, out, sizeof out, &n) == NFAGG_EINVAL);
    e.name_len = NFAGG_K8S_MAX_RENDERED + 1;                       /* refused before it is escaped */
    CHECK(nfagg_k8s_render(&e, 0, out, sizeof out, &n) == NFAGG_EINVAL);

    /* five keys of 102 bytes of key text: a name of 1946 plain bytes fills the cap, one more exceeds it */
    static char plain[2000];
    memset(plain, 'n', sizeof plain);
    e = entry(plain, NFAGG_K8S_MAX_RENDERED - 102, 3);
    CHECK(nfagg_k8s_render(&e, 1, out, sizeof out, &n) == NFAGG_OK && n == NFAGG_K8S_MAX_RENDERED && out[n - 1] == '"');
    e.name_len++;
    CHECK(nfagg_k8s_render(&e, 1, out, sizeof out, &n) == NFAGG_EINVAL);
    /* the same size reached by escapes: 324 control bytes at six bytes each and two plain ones */
    e = entry(ctl, 324, 3);
    e.kind = "kk"; e.kind_len = 2;
    CHECK(nfagg_k8s_render(&e, 0, out, sizeof out, &n) == NFAGG_OK && n == NFAGG_K8S_MAX_RENDERED);

    /* a length without its string */
    e = entry(NULL, 3, 4);
    CHECK(nfagg_k8s_render(&e, 0, out, sizeof out, &n) == NFAGG_EINVAL);

    /* tables without a handle: empty, 1000 rows with a layer, a duplicate, a block over the cap */
    nfagg_k8s_table* t = NULL;
    CHECK(nfagg_k8s_table_create(NULL, NULL, 0, NULL, &t) == NFAGG_OK && t);
    nfagg_k8s_table_destroy(t);
    enum { ROWS = 1000 };
    nfagg_k8s_entry* rows = calloc(ROWS + 1, sizeof *rows);
    static char names[ROWS][16];
    CHECK(rows != NULL);
    for (int k = 0; k < ROWS; k++) {
        snprintf(names[k], sizeof names[k], "pod-%d", k);
        rows[k] = entry(names[k], (uint32_t)strlen(names[k]), (uint8_t)k);
        rows[k].ip[14] = (uint8_t)(k >> 8);
        rows[k].namespace_ = k % 3 ? "openshift-dns" : "shop"; rows[k].namespace_len = k % 3 ? 13 : 4;
    }
    const char* prefixes[2] = {"openshift", "kube-"};
    const char* refs[4] = {"shop", "pod-3", "default", "kubernetes"};
    nfagg_k8s_layer layer = {sizeof layer, 2, prefixes, refs, 2, 0};
    CHECK(nfagg_k8s_table_create(NULL, rows, ROWS, &layer, &t) == NFAGG_OK && t);
    nfagg_k8s_table_destroy(t);
    rows[ROWS] = rows[17];
    CHECK(nfagg_k8s_table_create(NULL, rows, ROWS + 1, &layer, &t) == NFAGG_EINVAL && !t);
    CHECK(strstr(nfagg_last_error(NULL), "entries 17 and 1000 carry the same address") != NULL);
    rows[ROWS] = entry(plain, NFAGG_K8S_MAX_RENDERED - 101, 255);
    rows[ROWS].ip[0] = 0xfe;
    CHECK(nfagg_k8s_table_create(NULL, rows, ROWS + 1, NULL, &t) == NFAGG_EINVAL && !t);
    CHECK(strstr(nfagg_last_error(NULL), "entry 1000: its SrcK8S block has 2049 bytes") != NULL);
    free(rows);
    puts("k8s host check ok");
    return 0;
}
