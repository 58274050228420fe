/* nfagg_ipfix_cdriver.c — the IPFIX export of libnfagg driven from plain C, as a cgo shim would drive it: no Python, no torch,
 * only include/nfagg.h and lib/libnfagg.so. Reads 144-byte flow_record_t (evicted flows) from a file and writes
 *   <out>.ipfix : the v4 template message, the v6 template message, then one IPFIX message per flow (nfagg_encode_ipfix)
 *   <out>.off   : the n + 1 message offsets of the data messages (uint64, relative to the first data message)
 *   stdout      : "templates <bytes> messages <n> bytes <data bytes>"
 * The namer table is the small fixed one below (index 2 -> "eth0", index 3 -> "veth3", index 3 with MAC 02:00:00:00:00:01 ->
 * "veth3a"); other interfaces are "unknown".
 * usage: nfagg_ipfix_cdriver <records.bin> <out-prefix> <now_unix_ns> <mono_now_ns> <export_time_s> <seq0>
 *   cc -std=c11 -O2 -I include tools/c/nfagg_ipfix_cdriver.c -o nfagg_ipfix_cdriver -L <libdir> -lnfagg -Wl,-rpath,<libdir> */
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "nfagg.h"

static void die(nfagg_handle* h, const char* what, int rc) {
    fprintf(stderr, "%s failed: %d: %s\n", what, rc, nfagg_last_error(h) ? nfagg_last_error(h) : "");
    exit(2);
}

static nfagg_intf_name row(uint32_t if_index, const uint8_t* mac, const char* name) {
    nfagg_intf_name r;
    memset(&r, 0, sizeof r);
    r.if_index = if_index;
    if (mac) { memcpy(r.mac, mac, 6); r.has_mac = 1; }
    r.name_len = (uint8_t)strlen(name);
    memcpy(r.name, name, r.name_len);
    return r;
}

int main(int argc, char** argv) {
    if (argc != 7) { fprintf(stderr, "usage: %s records.bin out-prefix now_unix_ns mono_now_ns export_time_s seq0\n", argv[0]); return 1; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 1; }
    fseek(f, 0, SEEK_END);
    const size_t n = (size_t)ftell(f) / sizeof(nfagg_flow_record);
    fseek(f, 0, SEEK_SET);
    nfagg_flow_record* recs = malloc(n ? n * sizeof *recs : 1);
    if (fread(recs, sizeof *recs, n, f) != n) { fprintf(stderr, "short read\n"); return 1; }
    fclose(f);

    static const uint8_t mac[6] = {0x02, 0, 0, 0, 0, 0x01};
    nfagg_intf_name names[3];
    names[0] = row(2, 0, "eth0");
    names[1] = row(3, mac, "veth3a");
    names[2] = row(3, 0, "veth3");

    nfagg_ipfix_options opt;
    memset(&opt, 0, sizeof opt);
    opt.struct_size = sizeof opt;
    opt.n_names = 3;
    opt.names = names;
    opt.now_unix_ns = strtoll(argv[3], 0, 10);
    opt.mono_now_ns = strtoull(argv[4], 0, 10);
    opt.export_time_s = (uint32_t)strtoul(argv[5], 0, 10);
    opt.seq0 = (uint32_t)strtoul(argv[6], 0, 10);
    memcpy(opt.unknown_name, "unknown", 7);
    opt.unknown_len = 7;
    opt.obs_domain_id = 1;           /* ipfix.go:229 */
    opt.template_id_v4 = 256;        /* NewTemplateID() from 255: v4 first */
    opt.template_id_v6 = 257;

    uint8_t templates[200];
    size_t t4 = 0, t6 = 0;
    int rc = nfagg_ipfix_template(&opt, 0, templates, sizeof templates, &t4);
    if (rc != NFAGG_OK) die(0, "nfagg_ipfix_template(v4)", rc);
    rc = nfagg_ipfix_template(&opt, 1, templates + t4, sizeof templates - t4, &t6);
    if (rc != NFAGG_OK) die(0, "nfagg_ipfix_template(v6)", rc);

    nfagg_config cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.struct_size = sizeof cfg;
    cfg.max_entries = 64;
    nfagg_handle* h = 0;
    rc = nfagg_create(&cfg, &h);
    if (rc != NFAGG_OK) die(0, "nfagg_create", rc);

    uint64_t* off = malloc((n + 1) * sizeof *off);
    size_t need = 0;
    rc = nfagg_encode_ipfix(h, recs, n, &opt, 0, 0, off, &need);      /* size query: nothing written */
    if (rc != NFAGG_OK && rc != NFAGG_TRUNCATED) die(h, "nfagg_encode_ipfix (size)", rc);
    uint8_t* out = malloc(need ? need : 1);
    size_t wrote = 0;
    rc = nfagg_encode_ipfix(h, recs, n, &opt, out, need, off, &wrote);
    if (rc != NFAGG_OK || wrote != need) die(h, "nfagg_encode_ipfix", rc);

    char path[4096];
    snprintf(path, sizeof path, "%s.ipfix", argv[2]);
    FILE* o = fopen(path, "wb");
    if (!o) { perror(path); return 1; }
    fwrite(templates, 1, t4 + t6, o);
    fwrite(out, 1, wrote, o);
    fclose(o);
    snprintf(path, sizeof path, "%s.off", argv[2]);
    o = fopen(path, "wb");
    if (!o) { perror(path); return 1; }
    fwrite(off, sizeof *off, n + 1, o);
    fclose(o);
    printf("templates %zu messages %zu bytes %zu\n", t4 + t6, n, wrote);
    nfagg_destroy(h);
    free(out);
    free(off);
    free(recs);
    return 0;
}
