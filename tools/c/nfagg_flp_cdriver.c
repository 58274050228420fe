/* nfagg_flp_cdriver.c — the direct-FLP JSON export of libnfagg driven from plain C, as a cgo shim would drive it: no Python, no
 * torch, only include/nfagg.h and lib/libnfagg.so. Reads 144-byte flow_record_t (evicted flows) from a file and writes
 *   <out>.json  : one JSON line per flow that the encoder formats (nfagg_encode_flp_json), in record order
 *   <out>.off   : the n + 1 line offsets (uint64); a deferred record's line is empty
 *   <out>.def   : n bytes, 1 = deferred (TLS version / cipher suite / key share set: the Go side formats that record)
 *   stdout      : "lines <n> deferred <d> bytes <bytes>"
 * The namer table is the small fixed one below (index 2 -> "eth0", index 3 -> "veth3", index 3 with MAC 02:00:00:00:00:01 ->
 * "veth3a" in UDN "blue"); other interfaces are "unknown". AgentIP is 10.9.8.7.
 * usage: nfagg_flp_cdriver <records.bin> <out-prefix> <now_unix_ns> <mono_now_ns> <time_received_s>
 *   cc -std=c11 -O2 -I include tools/c/nfagg_flp_cdriver.c -o nfagg_flp_cdriver -L <libdir> -lnfagg -Wl,-rpath,<libdir> */
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "nfagg.h"

_Static_assert(sizeof(nfagg_flp_options) == 80, "nfagg_flp_options layout");

static void die(nfagg_handle* h, const char* what, int rc) {
    fprintf(stderr, "%s failed: %d: %s\n", what, rc, nfagg_last_error(h) ? nfagg_last_error(h) : "");
    exit(2);
}

static nfagg_intf_name row(uint32_t if_index, const uint8_t* mac, const char* name, const char* udn) {
    nfagg_intf_name r;
    memset(&r, 0, sizeof r);
    r.if_index = if_index;
    if (mac) { memcpy(r.mac, mac, 6); r.has_mac = 1; }
    r.name_len = (uint8_t)strlen(name);
    memcpy(r.name, name, r.name_len);
    r.udn_len = (uint8_t)strlen(udn);
    memcpy(r.udn, udn, r.udn_len);
    return r;
}

static void dump(const char* prefix, const char* ext, const void* p, size_t bytes) {
    char path[4096];
    snprintf(path, sizeof path, "%s.%s", prefix, ext);
    FILE* o = fopen(path, "wb");
    if (!o) { perror(path); exit(1); }
    fwrite(p, 1, bytes, o);
    fclose(o);
}

int main(int argc, char** argv) {
    if (argc != 6) { fprintf(stderr, "usage: %s records.bin out-prefix now_unix_ns mono_now_ns time_received_s\n", argv[0]); return 1; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 1; }
    fseek(f, 0, SEEK_END);
    const size_t n = (size_t)ftell(f) / sizeof(nfagg_flow_record);
    fseek(f, 0, SEEK_SET);
    nfagg_flow_record* recs = malloc(n ? n * sizeof *recs : 1);
    if (fread(recs, sizeof *recs, n, f) != n) { fprintf(stderr, "short read\n"); return 1; }
    fclose(f);

    static const uint8_t mac[6] = {0x02, 0, 0, 0, 0, 0x01};
    static const uint8_t agent[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0xff, 0xff, 10, 9, 8, 7};
    nfagg_intf_name names[3];
    names[0] = row(2, 0, "eth0", "");
    names[1] = row(3, mac, "veth3a", "blue");
    names[2] = row(3, 0, "veth3", "");

    nfagg_flp_options opt;
    memset(&opt, 0, sizeof opt);
    opt.struct_size = sizeof opt;
    opt.n_names = 3;
    opt.names = names;
    opt.now_unix_ns = strtoll(argv[3], 0, 10);
    opt.mono_now_ns = strtoull(argv[4], 0, 10);
    opt.time_received_s = strtoll(argv[5], 0, 10);
    memcpy(opt.unknown_name, "unknown", 7);
    opt.unknown_len = 7;
    memcpy(opt.agent_ip, agent, 16);

    nfagg_config cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.struct_size = sizeof cfg;
    cfg.max_entries = 64;
    nfagg_handle* h = 0;
    int rc = nfagg_create(&cfg, &h);
    if (rc != NFAGG_OK) die(0, "nfagg_create", rc);

    uint64_t* off = malloc((n + 1) * sizeof *off);
    uint8_t* deferred = malloc(n ? n : 1);
    size_t need = 0, n_deferred = 0;
    rc = nfagg_encode_flp_json(h, recs, n, &opt, 0, 0, off, deferred, &n_deferred, &need);      /* size query: nothing written */
    if (rc != NFAGG_OK && rc != NFAGG_TRUNCATED) die(h, "nfagg_encode_flp_json (size)", rc);
    uint8_t* out = malloc(need ? need : 1);
    size_t wrote = 0;
    rc = nfagg_encode_flp_json(h, recs, n, &opt, out, need, off, deferred, &n_deferred, &wrote);
    if (rc != NFAGG_OK || wrote != need) die(h, "nfagg_encode_flp_json", rc);

    dump(argv[2], "json", out, wrote);
    dump(argv[2], "off", off, (n + 1) * sizeof *off);
    dump(argv[2], "def", deferred, n);
    printf("lines %zu deferred %zu bytes %zu\n", n, n_deferred, wrote);
    nfagg_destroy(h);
    free(out);
    free(deferred);
    free(off);
    free(recs);
    return 0;
}
