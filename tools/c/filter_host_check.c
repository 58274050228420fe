/* filter_host_check.c — the host side of the transform filter stage driven from plain C, without a handle and without a device:
 * nfagg_filter_create(NULL, ...) over specs at the limits (64 atoms, 256 ops, 32 steps, a stack of 32), every refusal with the
 * atom, op or step it names, truth lengths against host-only Kubernetes and net tables, and nfagg_filter_roll against the
 * formula of the header restated here. Prints "filter host check ok" and returns 0.
 *   cc -std=c11 -O1 -g -I include tools/c/filter_host_check.c -o filter_host_check -L <libdir> -lnfagg -Wl,-rpath,<libdir> */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "nfagg.h"

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: %s\n  last error: %s\n", __FILE__, __LINE__, #cond, nfagg_last_error(NULL)); exit(1); } } while (0)
#define REFUSED(text) (rc == NFAGG_EINVAL && !f && strstr(nfagg_last_error(NULL), text))

static uint64_t fmix64(uint64_t x) {
    x ^= x >> 33; x *= 0xff51afd7ed558ccdull;
    x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull;
    x ^= x >> 33;
    return x;
}
static int roll(uint64_t seed, uint64_t i, uint32_t step, uint32_t value) {
    const uint64_t k = 0x9E3779B97F4A7C15ull;
    return value == 0 || fmix64(fmix64(seed + k * i) ^ (k * ((uint64_t)step + 1))) % value == 0;
}

static nfagg_filter_atom num(uint8_t field, uint8_t cmp, int64_t value) {
    nfagg_filter_atom a;
    memset(&a, 0, sizeof a);
    a.kind = NFAGG_FILTER_ATOM_NUM; a.field = field; a.cmp = cmp; a.value = value;
    return a;
}

static nfagg_filter_atom atoms[NFAGG_FILTER_MAX_ATOMS + 1];
static uint8_t ops[NFAGG_FILTER_MAX_OPS + 1];
static nfagg_filter_step steps[NFAGG_FILTER_MAX_STEPS + 1];

static int create(const nfagg_k8s_table* k8s, const nfagg_net_table* net, uint32_t flags, uint32_t n_atoms, uint32_t n_ops, uint32_t n_steps, nfagg_filter** f) {
    nfagg_filter_spec s = {sizeof s, flags, n_atoms, n_ops, n_steps, 0, atoms, ops, steps};
    return nfagg_filter_create(NULL, k8s, net, &s, f);
}

int main(void) {
    nfagg_filter* f = NULL;
    int rc;
    CHECK(sizeof(nfagg_filter_atom) == 48 && sizeof(nfagg_filter_step) == 8);

    /* the roll: the header's formula, value 0 and 1 always in */
    for (uint64_t i = 0; i < 20000; i++) {
        const uint64_t seed = i * 0x100000001b3ull, idx = (i << 33) ^ i;
        const uint32_t step = (uint32_t)(i % 32), value = (uint32_t)(i % 7 == 0 ? 65535 : i % 1001);
        CHECK(nfagg_filter_roll(seed, idx, step, value) == roll(seed, idx, step, value));
    }
    CHECK(nfagg_filter_roll(1, 2, 3, 0) == 1 && nfagg_filter_roll(1, 2, 3, 1) == 1);

    /* no steps: valid; at the limits: 64 atoms, 32 steps of 8 ops, one of them a stack of 32 */
    CHECK(create(NULL, NULL, 0, 0, 0, 0, &f) == NFAGG_OK && f);
    nfagg_filter_destroy(f);
    for (int k = 0; k < NFAGG_FILTER_MAX_ATOMS; k++) atoms[k] = num((uint8_t)(k % (NFAGG_FILTER_F_NUM_LAST + 1)), (uint8_t)(k % 6), k - 5);
    for (int s = 0; s < NFAGG_FILTER_MAX_STEPS; s++) {
        uint8_t* o = ops + 8 * s;
        o[0] = (uint8_t)(2 * s); o[1] = (uint8_t)(2 * s + 1); o[2] = NFAGG_FILTER_OP_AND; o[3] = NFAGG_FILTER_OP_NOT;
        o[4] = (uint8_t)s; o[5] = NFAGG_FILTER_OP_OR; o[6] = 63; o[7] = NFAGG_FILTER_OP_AND;
        steps[s].kind = s < 4 ? NFAGG_FILTER_STEP_KEEP : s < 20 ? NFAGG_FILTER_STEP_REMOVE : NFAGG_FILTER_STEP_SAMPLE_IF;
        steps[s].group = s < 20 ? 0 : (uint8_t)(s - 20); steps[s].value = s < 20 ? (s < 4 ? (uint16_t)(10 * s) : 0) : 65535;
        steps[s].op_begin = (uint16_t)(8 * s); steps[s].op_count = 8;
    }
    CHECK(create(NULL, NULL, NFAGG_FILTER_STORE_SAMPLING, 64, 256, 32, &f) == NFAGG_OK && f);
    nfagg_filter_destroy(f);
    nfagg_filter_destroy(NULL);
    f = NULL;
    rc = create(NULL, NULL, 0, 65, 256, 32, &f); CHECK(REFUSED("65 filter atoms, more than 64"));
    rc = create(NULL, NULL, 0, 64, 257, 32, &f); CHECK(REFUSED("257 filter ops, more than 256"));
    rc = create(NULL, NULL, 0, 64, 256, 33, &f); CHECK(REFUSED("33 filter steps, more than 32"));
    rc = create(NULL, NULL, 2, 64, 256, 32, &f); CHECK(REFUSED("unknown filter flags"));

    /* the stack: 32 pushes and 31 ORs fit, 33 pushes do not; underflow; a step that leaves two values, or none */
    for (int k = 0; k < 33; k++) ops[k] = (uint8_t)k;
    for (int k = 33; k < 65; k++) ops[k] = NFAGG_FILTER_OP_OR;
    steps[0].kind = NFAGG_FILTER_STEP_REMOVE; steps[0].group = 0; steps[0].value = 0; steps[0].op_begin = 1; steps[0].op_count = 32 + 31;
    CHECK(create(NULL, NULL, 0, 64, 65, 1, &f) == NFAGG_OK && f);
    nfagg_filter_destroy(f); f = NULL;
    steps[0].op_begin = 0; steps[0].op_count = 65;
    rc = create(NULL, NULL, 0, 64, 65, 1, &f); CHECK(REFUSED("filter step 0: op 32 grows the stack beyond 32"));
    ops[0] = 0; ops[1] = NFAGG_FILTER_OP_AND; steps[0].op_count = 2;
    rc = create(NULL, NULL, 0, 64, 2, 1, &f); CHECK(REFUSED("filter step 0: op 1 underflows the stack"));
    ops[0] = NFAGG_FILTER_OP_NOT; steps[0].op_count = 1;
    rc = create(NULL, NULL, 0, 64, 1, 1, &f); CHECK(REFUSED("filter step 0: op 0 underflows the stack"));
    ops[0] = 0; ops[1] = 1; steps[0].op_count = 2;
    rc = create(NULL, NULL, 0, 64, 2, 1, &f); CHECK(REFUSED("filter step 0: its ops leave 2 values, not one"));
    steps[0].op_count = 0;
    rc = create(NULL, NULL, 0, 64, 2, 1, &f); CHECK(REFUSED("filter step 0: its ops leave 0 values, not one"));
    steps[0].op_begin = 2; steps[0].op_count = 1;
    rc = create(NULL, NULL, 0, 64, 2, 1, &f); CHECK(REFUSED("filter step 0: ops [2, 3) of 2"));

    /* unknown ids */
    steps[0].op_begin = 0; steps[0].op_count = 1; ops[0] = 5;
    rc = create(NULL, NULL, 0, 5, 1, 1, &f); CHECK(REFUSED("filter op 0: atom 5 of 5"));
    ops[0] = 0x83;
    rc = create(NULL, NULL, 0, 5, 1, 1, &f); CHECK(REFUSED("filter op 0: unknown op 0x83"));
    ops[0] = 0;
    steps[0].kind = 3;
    rc = create(NULL, NULL, 0, 5, 1, 1, &f); CHECK(REFUSED("filter step 0: unknown kind 3"));
    steps[0].kind = NFAGG_FILTER_STEP_SAMPLE_IF; steps[0].group = 32;
    rc = create(NULL, NULL, 0, 5, 1, 1, &f); CHECK(REFUSED("filter step 0: group 32"));
    steps[0].kind = NFAGG_FILTER_STEP_REMOVE; steps[0].group = 0; steps[1] = steps[0]; steps[1].kind = NFAGG_FILTER_STEP_KEEP;
    rc = create(NULL, NULL, 0, 5, 1, 2, &f); CHECK(REFUSED("filter step 1: a KEEP step behind a step of another kind"));
    atoms[1].kind = 6;
    rc = create(NULL, NULL, 0, 5, 1, 1, &f); CHECK(REFUSED("filter atom 1: unknown kind 6"));
    atoms[1] = num(NFAGG_FILTER_F_LAST + 1, 0, 0);
    rc = create(NULL, NULL, 0, 5, 1, 1, &f); CHECK(REFUSED("filter atom 1: unknown field 27"));
    atoms[1] = num(NFAGG_FILTER_F_SRC_ADDR, 0, 0);
    rc = create(NULL, NULL, 0, 5, 1, 1, &f); CHECK(REFUSED("filter atom 1: SrcAddr is a presence-only field"));
    atoms[1] = num(NFAGG_FILTER_F_BYTES, 6, 0);
    rc = create(NULL, NULL, 0, 5, 1, 1, &f); CHECK(REFUSED("filter atom 1: unknown comparison 6"));
    atoms[1] = num(0, 0, 0); atoms[1].kind = NFAGG_FILTER_ATOM_PRESENT; atoms[1].field = NFAGG_FILTER_F_DST_MAC;
    atoms[2] = num(0, 0, 0); atoms[2].kind = NFAGG_FILTER_ATOM_MAC; atoms[2].side = 2;
    rc = create(NULL, NULL, 0, 5, 1, 1, &f); CHECK(REFUSED("filter atom 2: unknown side 2"));
    atoms[2].side = 1; atoms[2].pad_[1] = 1;
    rc = create(NULL, NULL, 0, 5, 1, 1, &f); CHECK(REFUSED("filter atom 2: non-zero padding"));
    atoms[2].pad_[1] = 0;

    /* TABLE atoms: the table must be there, and the truth as long as its dimension */
    static uint8_t truth[64];
    nfagg_filter_atom t;
    memset(&t, 0, sizeof t);
    t.kind = NFAGG_FILTER_ATOM_TABLE; t.truth = truth;
    atoms[3] = t; atoms[3].dim = NFAGG_FILTER_DIM_LAST + 1; atoms[3].n_truth = 3;
    rc = create(NULL, NULL, 0, 5, 1, 1, &f); CHECK(REFUSED("filter atom 3: unknown dimension 7"));
    atoms[3].dim = NFAGG_FILTER_DIM_DST_K8S_ROW;
    rc = create(NULL, NULL, 0, 5, 1, 1, &f); CHECK(REFUSED("filter atom 3: a Kubernetes-row table atom without a Kubernetes table"));
    atoms[3].dim = NFAGG_FILTER_DIM_SRC_SUBNET_LABEL;
    rc = create(NULL, NULL, 0, 5, 1, 1, &f); CHECK(REFUSED("filter atom 3: a subnet-label table atom without a net table"));
    atoms[3].dim = NFAGG_FILTER_DIM_FLOW_LAYER;
    rc = create(NULL, NULL, 0, 5, 1, 1, &f); CHECK(REFUSED("filter atom 3: a flow-layer table atom without a Kubernetes table"));
    atoms[3].dim = NFAGG_FILTER_DIM_DNS_RCODE; atoms[3].n_truth = 16;
    rc = create(NULL, NULL, 0, 5, 1, 1, &f); CHECK(REFUSED("filter atom 3: 16 truth entries, its dimension has 17"));
    atoms[3].n_truth = 17; atoms[3].truth = NULL;
    rc = create(NULL, NULL, 0, 5, 1, 1, &f); CHECK(REFUSED("filter atom 3: null truth bytes"));
    atoms[3].truth = truth;
    atoms[4] = t; atoms[4].dim = NFAGG_FILTER_DIM_IPSEC_STATUS; atoms[4].n_truth = 3;
    CHECK(create(NULL, NULL, 0, 5, 1, 1, &f) == NFAGG_OK && f);
    nfagg_filter_destroy(f); f = NULL;

    nfagg_k8s_entry rows[5];
    memset(rows, 0, sizeof rows);
    for (int i = 0; i < 5; i++) { rows[i].ip[15] = (uint8_t)(i + 1); rows[i].name = "pod"; rows[i].name_len = 3; }
    nfagg_k8s_table* kt = NULL;
    CHECK(nfagg_k8s_table_create(NULL, rows, 5, NULL, &kt) == NFAGG_OK && kt);
    nfagg_net_label labels[3] = {{"a", 1, 0}, {"", 0, 0}, {"c", 1, 0}};
    nfagg_net_rules nr = {sizeof nr, NFAGG_NET_SUBNET_LABELS | NFAGG_NET_DECODE_TCP_FLAGS, NULL, labels, 0, 3};
    nfagg_net_table* nt = NULL;
    CHECK(nfagg_net_table_create(NULL, &nr, &nt) == NFAGG_OK && nt);
    atoms[3].dim = NFAGG_FILTER_DIM_SRC_K8S_ROW; atoms[3].n_truth = 5;
    rc = create(kt, nt, 0, 5, 1, 1, &f); CHECK(REFUSED("filter atom 3: 5 truth entries, its dimension has 6"));
    atoms[3].n_truth = 6;
    atoms[4].dim = NFAGG_FILTER_DIM_DST_SUBNET_LABEL; atoms[4].n_truth = 3;
    rc = create(kt, nt, 0, 5, 1, 1, &f); CHECK(REFUSED("filter atom 4: 3 truth entries, its dimension has 4"));
    atoms[4].n_truth = 4;
    CHECK(create(kt, nt, 0, 5, 1, 1, &f) == NFAGG_OK && f);
    nfagg_filter_destroy(f); f = NULL;
    atoms[4].dim = NFAGG_FILTER_DIM_FLOW_LAYER; atoms[4].n_truth = 3;
    CHECK(create(kt, NULL, 0, 5, 1, 1, &f) == NFAGG_OK && f);
    nfagg_filter_destroy(f); f = NULL;

    /* the struct itself */
    nfagg_filter_spec s = {8, 0, 0, 0, 0, 0, NULL, NULL, NULL};
    rc = nfagg_filter_create(NULL, NULL, NULL, &s, &f); CHECK(REFUSED("struct_size"));
    s.struct_size = sizeof s; s.n_ops = 1;
    rc = nfagg_filter_create(NULL, NULL, NULL, &s, &f); CHECK(REFUSED("null list with a count"));
    s.n_ops = 0; s.pad_ = 1;
    rc = nfagg_filter_create(NULL, NULL, NULL, &s, &f); CHECK(REFUSED("non-zero padding"));
    s.pad_ = 0;
    CHECK(nfagg_filter_create(NULL, NULL, NULL, NULL, &f) == NFAGG_EINVAL && nfagg_filter_create(NULL, NULL, NULL, &s, NULL) == NFAGG_EINVAL);
    nfagg_net_table_destroy(nt);
    nfagg_k8s_table_destroy(kt);
    puts("filter host check ok");
    return 0;
}
