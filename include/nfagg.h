/*
 * nfagg.h — C ABI of libnfagg, the MI355X (gfx950) flow-aggregation backend.
 *
 * This header is the drop-in boundary behind netobserv-ebpf-agent's userspace
 * flow stage. Every entry point names the reference interface it replaces
 * (paths relative to the reference repository root). The reference-side cgo
 * binding a maintainer would add is shown in INTEGRATION.md.
 *
 * Rules of the boundary:
 *   - plain C, plain pointers and sizes; no callbacks into the caller, no
 *     pointer retained after a call returns (cgo pointer rules);
 *   - the caller owns input buffers until the call returns, the library owns
 *     the flow table, eviction output goes into caller-provided buffers;
 *   - one producer per handle; calls on a handle are synchronous and must not
 *     overlap (exactly one goroutine runs Accounter.Account, account.go:58);
 *   - return value 0 = NFAGG_OK, >0 = a condition the caller must act on,
 *     <0 = error (nfagg_last_error gives the text). No Go-visible panics.
 *
 * There is NO CPU fallback behind this ABI: if the HIP runtime or a gfx950
 * device is missing, nfagg_create fails with NFAGG_ENODEV.
 */
#ifndef NFAGG_H
#define NFAGG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NFAGG_ABI_VERSION 2u   /* 2 (round 6): nfagg_stats grew by account_epochs_first / account_chain / account_declined in round 5 without a bump — a
                                   caller built against version 1's header must not be handed the longer struct; cfg.copy_threads = 0 means "the
                                   calibrated number of parts" (was: 4) */

/* ------------------------------------------------------------------ */
/* Record ABI — byte-for-byte the structs of bpf/types.h               */
/* ------------------------------------------------------------------ */

/* bpf/types.h:191-204 flow_id; pkg/ebpf/bpf_x86_bpfel.go:108-120 BpfFlowId.
 * 40 bytes, alignment 2. Byte 39 is padding: the library zeroes it on ingest
 * (the kernel memsets it, bpf/flows.c:177-178; Go ignores it). */
typedef struct nfagg_flow_id {
    uint8_t  src_ip[16];          /* IPv4 as ::ffff:a.b.c.d */
    uint8_t  dst_ip[16];
    uint16_t src_port;            /* host endian */
    uint16_t dst_port;
    uint8_t  transport_protocol;
    uint8_t  icmp_type;
    uint8_t  icmp_code;
    uint8_t  pad_;
} nfagg_flow_id;

/* bpf/types.h:94-126 flow_metrics; bpf_x86_bpfel.go:122-153 BpfFlowMetrics.
 * 104 bytes, alignment 8. */
typedef struct nfagg_flow_metrics {
    uint64_t start_mono_time_ts;  /* @0  */
    uint64_t end_mono_time_ts;    /* @8  */
    uint64_t bytes;               /* @16 */
    uint32_t packets;             /* @24 */
    uint16_t eth_protocol;        /* @28 */
    uint16_t flags;               /* @30 */
    uint8_t  src_mac[6];          /* @32 */
    uint8_t  dst_mac[6];          /* @38 */
    uint32_t if_index_first_seen; /* @44 */
    uint32_t lock;                /* @48 struct bpf_spin_lock */
    uint32_t sampling;            /* @52 */
    uint8_t  direction_first_seen;/* @56 */
    uint8_t  errno_;              /* @57 */
    uint8_t  dscp;                /* @58 */
    uint8_t  nb_observed_intf;    /* @59 */
    uint8_t  observed_direction[6];/* @60 */
    uint8_t  pad2_[2];            /* @66 */
    uint32_t observed_intf[6];    /* @68 */
    uint16_t ssl_version;         /* @92 */
    uint16_t tls_cipher_suite;    /* @94 */
    uint16_t tls_key_share;       /* @96 */
    uint8_t  tls_types;           /* @98 */
    uint8_t  misc_flags;          /* @99 */
    uint8_t  pad4_[4];            /* @100 */
} nfagg_flow_metrics;

/* bpf/types.h:212-215 flow_record; pkg/model/record.go:63 RawRecord.
 * 144 bytes — the unit on the ring buffer (byte-exact vector:
 * pkg/model/record_test.go:19-102). */
typedef struct nfagg_flow_record {
    nfagg_flow_id      id;        /* @0  */
    nfagg_flow_metrics metrics;   /* @40 */
} nfagg_flow_record;

/* bpf/types.h:174-181 additional_metrics (RTT / IPsec). 32 bytes. */
typedef struct nfagg_additional_metrics {
    uint64_t start_mono_time_ts;
    uint64_t end_mono_time_ts;
    uint64_t flow_rtt;
    int32_t  ipsec_encrypted_ret;
    uint16_t eth_protocol;
    uint8_t  ipsec_encrypted;     /* bool */
    uint8_t  pad_;
} nfagg_additional_metrics;

/* bpf/types.h:131-140 dns_metrics. 64 bytes (name is NOT 2-aligned). */
typedef struct nfagg_dns_metrics {
    uint64_t start_mono_time_ts;
    uint64_t end_mono_time_ts;
    uint64_t latency;
    uint16_t id;
    uint16_t flags;
    uint16_t eth_protocol;
    uint8_t  errno_;
    char     name[32];
    uint8_t  pad_;
} nfagg_dns_metrics;

/* bpf/types.h:142-151 pkt_drop_metrics. 32 bytes. */
typedef struct nfagg_pkt_drop_metrics {
    uint64_t start_mono_time_ts;
    uint64_t end_mono_time_ts;
    uint16_t bytes;
    uint16_t packets;
    uint32_t latest_drop_cause;
    uint16_t latest_flags;
    uint16_t eth_protocol;
    uint8_t  latest_state;
    uint8_t  pad_[3];
} nfagg_pkt_drop_metrics;

/* bpf/types.h:153-161 network_events_metrics. 72 bytes. */
typedef struct nfagg_network_events_metrics {
    uint64_t start_mono_time_ts;
    uint64_t end_mono_time_ts;
    uint8_t  network_events[4][8];
    uint16_t bytes[4];
    uint16_t packets[4];
    uint16_t eth_protocol;
    uint8_t  network_events_idx;
    uint8_t  pad_[5];
} nfagg_network_events_metrics;

/* bpf/types.h:163-172 xlat_metrics. 56 bytes. */
typedef struct nfagg_xlat_metrics {
    uint64_t start_mono_time_ts;
    uint64_t end_mono_time_ts;
    uint8_t  saddr[16];
    uint8_t  daddr[16];
    uint16_t sport;
    uint16_t dport;
    uint16_t zone_id;
    uint16_t eth_protocol;
} nfagg_xlat_metrics;

/* bpf/types.h quic_metrics_t. 24 bytes. */
typedef struct nfagg_quic_metrics {
    uint64_t start_mono_time_ts;
    uint64_t end_mono_time_ts;
    uint32_t version;
    uint16_t eth_protocol;
    uint8_t  seen_long_hdr;
    uint8_t  seen_short_hdr;
} nfagg_quic_metrics;

/* ------------------------------------------------------------------ */
/* Status codes                                                         */
/* ------------------------------------------------------------------ */
enum {
    NFAGG_OK       = 0,
    /* >0: the caller must act, nothing went wrong */
    NFAGG_FULL     = 1,  /* ingest stopped before a record whose NEW key would
                            exceed max_entries (account.go:85): evict with
                            NFAGG_REASON_FULL, then resubmit the remainder.
                            (An epoch is never ended for lack of sequence
                            numbers: the slots' 32-bit sequence tags are
                            window-relative and the window moves,
                            stats.sequence_rebases.) */
    NFAGG_TRUNCATED = 2, /* output buffer smaller than the result */
    NFAGG_EDEFER   = 3,  /* nfagg_timebased_extract: some flow has no value for a rule of a table it enters; nothing was changed,
                            drop those flows and call again */
    /* <0: errors */
    NFAGG_EINVAL   = -1,
    NFAGG_ENODEV   = -2, /* no HIP runtime / no gfx950 device: there is no CPU path */
    NFAGG_ENOMEM   = -3,
    NFAGG_EDEVICE  = -4, /* a HIP call failed; see nfagg_last_error */
    NFAGG_ESTATE   = -5, /* call not valid in the handle's current state */
    NFAGG_ERANGE   = -6, /* an argument is out of the supported range (e.g. map merge over more than 2^30 rows) */
};

/* Eviction reasons — the label values of the reference's Prometheus counters
 * (pkg/flow/account.go:71,78,90; pkg/metrics/metrics.go). */
enum {
    NFAGG_REASON_TIMEOUT = 0,   /* "timeout" */
    NFAGG_REASON_FULL    = 1,   /* "full"    */
    NFAGG_REASON_CLOSING = 2,   /* "closing" */
};

/* Accumulation semantics of the flow table. */
enum {
    /* pkg/model/flow_content.go:28-61 AccumulateBase, first record of a key
     * stored whole (account.go:95). This is what Accounter does. */
    NFAGG_MODE_ACCOUNTER = 0,
    /* bpf/flows.c:98-143 update_existing_flow + :76-96 add_observed_intf:
     * bytes/packets counted only on if_index_first_seen, other interfaces are
     * appended to observed_intf[] ("direction dedup"). */
    NFAGG_MODE_KERNEL_DEDUP = 1,
};

enum {
    NFAGG_SKETCH_CM  = 1u,  /* Count-Min over src IP and dst IP, adding bytes */
    NFAGG_SKETCH_HLL = 2u,  /* HyperLogLog over src IP and dst IP */
};

/* Sketch identifiers for snapshot / device-pointer / estimate calls. */
enum {
    NFAGG_CM_SRC  = 0,   /* uint64_t[cm_depth << cm_log2_width] */
    NFAGG_CM_DST  = 1,
    NFAGG_HLL_SRC = 2,   /* uint8_t [1 << hll_p], on the device and in snapshots */
    NFAGG_HLL_DST = 3,
};

/* ------------------------------------------------------------------ */
/* Handle and configuration                                             */
/* ------------------------------------------------------------------ */
typedef struct nfagg_handle nfagg_handle;

/* Replaces the arguments of flow.NewAccounter (pkg/flow/account.go:34-53;
 * call site pkg/agent/agent.go:208-212). Clocks, Prometheus metrics and the
 * OVN sample decoder stay on the Go side. Zero = default for every field
 * except struct_size. */
typedef struct nfagg_config {
    uint32_t struct_size;        /* sizeof(nfagg_config); ABI guard */
    int32_t  device;             /* HIP device ordinal */
    uint64_t max_entries;        /* CACHE_MAX_FLOWS (config.go:146); 0 -> 5000 */
    uint32_t table_log2_slots;   /* 0 -> smallest 2^k >= 2*max_entries (min 2^16) */
    uint32_t mode;               /* NFAGG_MODE_* */
    uint32_t sketch_flags;       /* NFAGG_SKETCH_* */
    uint32_t cm_depth;           /* 0 -> 4  (1..8) */
    uint32_t cm_log2_width;      /* 0 -> 20 */
    uint32_t hll_p;              /* 0 -> 14 (4..18) */
    uint64_t staging_records;    /* pinned staging ring, records per buffer; 0 -> 1<<20 */
    uint32_t n_shards;           /* 0/1 -> unsharded. Records whose
                                    nfagg_shard_of(id,n_shards) != shard_id are
                                    skipped on ingest and counted in stats */
    uint32_t shard_id;
    uint32_t profile;            /* 1 -> bracket kernels with HIP events (stats) */
    uint32_t ingest_variant;     /* 0 -> default kernels by batch size (direct kernel below 6144 records,
                                    single-pass LDS-cached kernel below 384 Ki, two-pass partitioned fold from
                                    there); others are A/B and diagnostic builds: csrc/nfagg_variants.h lists
                                    them all */
    /* Optional caller-owned DEVICE buffers for the sketches (so that another
     * library, e.g. RCCL via torch.distributed, can all-reduce them in place).
     * NULL -> the library allocates. Sizes as listed under NFAGG_CM_* above
     * (HLL: one byte per register, buffer 4-byte aligned). */
    void*    ext_sketch[4];
    uint32_t copy_threads;       /* parts a caller buffer is cut into for the copy workers (nfagg_host_threads) on its way into
                                    the pinned staging ring (one core moves ~28 GB/s, PCIe Gen5 x16 takes ~57); 0 -> what the
                                    workers' calibration found best on this host, 1 -> inline */
    uint32_t group_flags;        /* nfagg_group_create only: NFAGG_GROUP_* */
    uint32_t local_fold;         /* nfagg_create only (a NFAGG_GROUP_LOCAL_FOLD group sets it for its members): 1 = this handle is
                                    one rank of a local-fold job (nfagg_set_sequence / nfagg_partials_* below): it folds whatever
                                    part of ONE record stream arrives at it and other tables hold other records of the same flows.
                                    NFAGG_MODE_ACCOUNTER: no effect (a slot is a mergeable partial as it is).
                                    NFAGG_MODE_KERNEL_DEDUP: what a table counts for a flow depends on the flow's FIRST interface
                                    (bpf/flows.c:100-126), and that is the interface of the earliest record anywhere in the job —
                                    so the table is keyed by the SUB-FLOW (flow key, if_index_first_seen) and keeps, per
                                    interface, both what a counted and what a side interface needs; the flow itself is put
                                    together when the epoch ends (the sub-flows of all ranks having met at the flow's owner):
                                    nfagg_evict* / nfagg_evict_owned_device deliver exactly what ONE table over all the records
                                    would. Differences on such a handle: max_entries and nfagg_len count (flow, interface) pairs
                                    — NFAGG_FULL comes when a NEW pair finds max_entries of them; partials are
                                    NFAGG_PARTIAL_BYTES_DEDUP bytes; the 32-bit sequence window does not move: an epoch ends
                                    (NFAGG_FULL) once 2^32 - 16 sequence numbers have gone by in the job, and
                                    nfagg_window_restart_device is refused. */
} nfagg_config;

enum {
    /* Local-fold ("combiner") mode of a group: no per-record routing. Every member folds the chunks that arrive on ITS
     * device, whatever their keys, with sequence numbers global to the group; a flow may live on several members at once. At
     * the eviction the members' raw slots — mergeable partials, sequence tags included — travel to the member that owns the
     * flow (nfagg_shard_of), are merged there exactly (sums, ORs, maxima, earliest-tag-wins words) and the owner evicts the
     * flow. xGMI carries 192 bytes per (flow, member) instead of 144 bytes per record, and one hot flow (BASELINE configs[4])
     * is folded by all GPUs instead of by the one that owns it. Every eviction is bit-identical to one Accounter that saw
     * the same records between the same two evictions. Differences to the routed mode: max_entries bounds every member's
     * table, undivided — NFAGG_FULL is returned when ONE member holds max_entries flows and meets a new one, which is never
     * earlier and can be later than one Accounter over the whole stream would (an eviction may deliver up to
     * N x max_entries flows); use it where evictions are timeout-driven (CACHE_ACTIVE_TIMEOUT) and max_entries is the
     * safety net. nfagg_group_len is an upper bound (a flow counts once per member that saw it). After an eviction call
     * that returned NFAGG_TRUNCATED the group only accepts the repeated eviction (ingest returns NFAGG_FULL): the members'
     * slots have been merged already. Both modes: in NFAGG_MODE_KERNEL_DEDUP the members are created with
     * nfagg_config.local_fold (tables keyed by (flow, interface), see there), every eviction is bit-identical to ONE
     * kernel-dedup table (bpf/flows.c:76-143) over the same records — BASELINE configs[4]'s hot flow alternating over two
     * interfaces is counted on the interface of its earliest record whichever member saw that record — and an epoch ends
     * (NFAGG_FULL) after 2^32 - 16 records. */
    NFAGG_GROUP_LOCAL_FOLD = 1u,
};

typedef struct nfagg_stats {
    uint64_t records_ingested;   /* accepted into the table (this shard) */
    uint64_t records_skipped;    /* not this shard */
    uint64_t entries;            /* live keys now  (accounter-entries gauge, account.go:98) */
    uint64_t evictions[3];       /* per NFAGG_REASON_* (evictions_total) */
    uint64_t evicted_flows[3];   /* per reason (evicted_flows_total) */
    uint64_t epoch_seq;          /* records ingested since the last eviction */
    uint64_t table_slots;
    uint64_t table_bytes;
    /* filled when cfg.profile != 0 (HIP events on the handle's stream) */
    uint64_t ingest_launches;
    double   ingest_kernel_ms;   /* sum of ingest-kernel durations */
    uint64_t evict_launches;
    double   evict_kernel_ms;
    uint64_t sketch_launches;
    double   sketch_kernel_ms;
    uint64_t max_probe;          /* longest probe sequence seen */
    uint64_t records_bypassed;   /* records that found no entry in a pass-1 LDS flow cache (spilled to the
                                    second pass, or merged into HBM one by one by the single-pass kernel) */
    uint64_t optimistic_folds;   /* batches with live + batch > max_entries folded whole and checked afterwards */
    uint64_t optimistic_rollbacks; /* ... of which crossed max_entries (account.go:85) and were rolled back and split */
    uint64_t sequence_rebases;     /* times the 32-bit window of the slots' sequence tags was moved (once per ~2^32 records of an
                                      epoch; the epoch itself goes on: account.go:58-100 has no maximum length) */
    uint64_t account_epochs_first; /* nfagg_account[_device]: launches that found their epochs first and folded them from the sorted call */
    uint64_t account_chain;        /* ... launches of the kernel chain (short calls; calls the first path declined) */
    uint64_t account_declined;     /* ... of which were calls the first path declined (too many other flows' records between a
                                      record and its previous occurrence among equal hash bits) */
} nfagg_stats;

uint32_t nfagg_abi_version(void);

/* Replaces flow.NewAccounter (pkg/flow/account.go:34-53). */
int nfagg_create(const nfagg_config* cfg, nfagg_handle** out);

/* Replaces nothing in the reference (Go GC frees the Accounter); required by
 * C ownership. Pending flows are discarded: evict with NFAGG_REASON_CLOSING
 * first (account.go:73-80). */
void nfagg_destroy(nfagg_handle* h);

/* Text of the last error on this handle (NULL handle: last create error). */
const char* nfagg_last_error(const nfagg_handle* h);

/* ------------------------------------------------------------------ */
/* Ingest — replaces the `case record, ok := <-in` arm of               */
/* Accounter.Account (pkg/flow/account.go:72-96), batched.              */
/* ------------------------------------------------------------------ */

/* records: n x 144-byte flow_record_t in HOST memory (what
 * model.ReadFrom decodes, pkg/model/record.go:227-231), in arrival order.
 * The records are folded in exactly that order. *consumed = number of
 * leading records folded; returns NFAGG_FULL when it stopped early.
 * One limit: start_mono_time_ts = 2^64 - 1 is folded as 0 ("not set"): the
 * slots keep ~start with 0 for "no start yet" (tagged words). */
int nfagg_ingest(nfagg_handle* h, const void* records, size_t n, size_t* consumed);

/* Same, records already in DEVICE memory of cfg.device (16-byte aligned). ASYNCHRONOUS when the batch cannot fill the table
 * (live + n <= max_entries): the kernels run on the handle's stream after the call returned and read d_records (the fold,
 * and k_finalize's copy of the new flows' first records), so the buffer must stay valid and unmodified until the handle
 * synchronises — nfagg_sync, nfagg_len, nfagg_evict*, nfagg_stats_get, or work ordered after nfagg_stream(h). (The host
 * variants copy into the library's own staging ring and have no such requirement.) */
int nfagg_ingest_device(nfagg_handle* h, const void* d_records, size_t n, size_t* consumed);

/* Page-locked host memory (hipHostMalloc). Record buffers handed to nfagg_ingest / nfagg_account and output buffers handed to
 * nfagg_evict / nfagg_account that lie in page-locked memory — from here, or registered by the caller (hipHostRegister) — cross
 * PCIe by DMA straight from / into them; pageable buffers go through the library's pinned staging ring (one more host copy:
 * ~30 GB/s instead of the link's ~50). A Go caller keeps its batch in such a buffer instead of a Go slice. */
int nfagg_host_alloc(size_t bytes, void** p);
void nfagg_host_free(void* p);

/* The host side's copy workers (one pool per process; csrc/nfagg_hostpool.h): what moves records with host cores — a pageable
 * caller buffer into the pinned staging ring (nfagg_ingest / nfagg_account), evictions out of the pinned bounce buffers, the BPF
 * ring buffer into the staging buffer (nfagg_ringbuf_drain, the batch form of RingBufTracer's loop,
 * pkg/flow/tracer_ringbuf.go:112-134). Created by the first nfagg_create: 16 workers bound to the CPUs of that handle's GPU's
 * NUMA node, non-temporal copies, and the number of parts a large copy is cut into MEASURED on this host (a calibration of a few
 * milliseconds) rather than assumed. nfagg_host_threads re-shapes the pool: `threads` workers (0 = keep the number), bound to
 * `numa_node` (-1 = unbound); returns the workers running (>= 0) or NFAGG_EINVAL. An agent that wants its cores left alone
 * calls nfagg_host_threads(2, -1) — or sets nfagg_config.copy_threads = 1 and drains the ring itself. */
typedef struct nfagg_host_pool_info {
    uint32_t struct_size;        /* sizeof(nfagg_host_pool_info) */
    uint32_t workers;            /* threads in the pool (the calling thread always works too) */
    uint32_t parts;              /* parts a large copy is cut into: the calibration's choice */
    uint32_t bound;              /* 1: the workers are bound to numa_node's CPUs */
    int32_t  numa_node;          /* -1: unbound */
    uint32_t pad_;
    double   calibrated_gbs;     /* what the best setting copied in the calibration, GB/s (host memory to host memory) */
} nfagg_host_pool_info;
int nfagg_host_threads(unsigned threads, int numa_node);
int nfagg_host_info(nfagg_host_pool_info* out);
/* The NUMA node `device` hangs off (/sys/bus/pci/devices/<bdf>/numa_node); -1 when unknown. */
int nfagg_device_numa_node(int device);

/* Zero-copy producer path: borrow the next pinned staging buffer
 * (capacity = cfg.staging_records), fill it (e.g. straight from the eBPF ring,
 * pkg/flow/tracer_ringbuf.go:112-134), then commit the first n records.
 * commit has nfagg_ingest semantics. */
int nfagg_staging_acquire(nfagg_handle* h, void** buf, size_t* capacity_records);
int nfagg_staging_commit(nfagg_handle* h, size_t n, size_t* consumed);

/* len(c.entries) (account.go:85,98). Synchronises with the device. */
int nfagg_len(nfagg_handle* h, uint64_t* entries);

/* ------------------------------------------------------------------ */
/* Evict — replaces Accounter.evict (pkg/flow/account.go:102-124) up to */
/* the point where model.NewRecord is called per entry.                 */
/* ------------------------------------------------------------------ */

/* Writes every live flow as one 144-byte flow_record_t {id, folded metrics}
 * into `out` (HOST memory, room for `cap` records), clears the table, starts
 * a new epoch. Order of records is unspecified (Go map order is random;
 * the reference's tests compare by key, account_test.go:94-98).
 * If cap < live entries nothing is evicted: *n_out = live entries and
 * NFAGG_TRUNCATED is returned. The caller turns each record into a
 * model.Record with model.NewRecord(key, &content, now, mono, ...)
 * exactly as account.go:116-119 (helper: nfagg_record_times). */
int nfagg_evict(nfagg_handle* h, int reason, void* out, size_t cap, size_t* n_out);

/* Same with `d_out` in DEVICE memory. */
int nfagg_evict_device(nfagg_handle* h, int reason, void* d_out, size_t cap, size_t* n_out);

/* ------------------------------------------------------------------ */
/* Account — the record arm of Accounter.Account WITH its evictions on   */
/* "full" (pkg/flow/account.go:81-96) in one call.                      */
/* ------------------------------------------------------------------ */

/* Folds records in arrival order exactly as nfagg_ingest does, but does not stop at a record whose NEW key finds
 * len(entries) >= max_entries (account.go:85): as the reference does inline (:86-94) it evicts every live flow — appended to
 * `out`, reason "full" — restarts the epoch and inserts that record. On return *n_epochs evictions have taken place; the
 * e-th delivered out[epoch_end[e-1] .. epoch_end[e]) (epoch_end[-1] = 0), the caller turns each into one `[]*model.Record`
 * for the exporter (account.go:111-123, one channel send per eviction); the table holds the epoch in progress, as after
 * nfagg_ingest. *consumed = leading records folded. Returns NFAGG_OK when all n are, NFAGG_TRUNCATED when `out` has no room
 * for another eviction (out_cap - records written < live flows; keep out_cap >= max_entries) or max_epochs are used up:
 * drain `out`, then call again with the rest (a pending eviction is delivered first).
 * With a small CACHE_MAX_FLOWS (the reference ships 5000, pkg/config/config.go:146, deploys 10 000, scripts/agent.yml:35-36, and
 * benchmarks 1 k / 10 k / 100 k, pkg/flow/tracer_map_bench_test.go:64-111) the stream stops on "full" every few thousand records;
 * here that whole loop runs on the device (NFAGG_MODE_ACCOUNTER, max_entries <= 2^22). A call of more than five chain windows'
 * worth of records (n >= 5 / (1 / 16384 + 1 / (2 max_entries)): 31 k at 5000 entries, never more than 80 k) has its epochs FOUND
 * FIRST (csrc/nfagg_epoch_par.hip): previous-occurrence links from one sort of (key hash, index) keys, one prefix
 * count per epoch — WHERE the loop of account.go:81-96 evicts does not need the map — and every complete epoch is then folded on
 * its own, all of them at once, each flow's records gathered in arrival order and folded as flow_content.go:28-61 folds them,
 * straight into `out`; only the call's first epoch (it continues what the table holds) and its last (it stays live) touch the
 * table. Sketches are fed along. Shorter calls take a chain of small kernels driven by a control block in device memory, replayed
 * from hipGraphs of 2 / 6 / 24 windows (csrc/nfagg_epoch_chain.hip; max_entries <= 32768; beyond: the optimistic fold of
 * nfagg_ingest); ingest_variant 30 forces that chain for every call (tests). Same evictions, in the same order, either way.
 * A call costs ~80 us whatever it holds: gather records (64 Ki, or what 1 ms brings) before calling — INTEGRATION.md section 3.
 * All pointers HOST memory: */
int nfagg_account(nfagg_handle* h, const void* records, size_t n, void* out, size_t out_cap, uint64_t* epoch_end,
                  size_t max_epochs, size_t* n_epochs, size_t* consumed);
/* Same with d_records / d_out in DEVICE memory (16-byte aligned); epoch_end stays in HOST memory. Synchronous: d_records
 * may be reused when the call returns. */
int nfagg_account_device(nfagg_handle* h, const void* d_records, size_t n, void* d_out, size_t out_cap, uint64_t* epoch_end,
                         size_t max_epochs, size_t* n_epochs, size_t* consumed);

/* ------------------------------------------------------------------ */
/* Capacity limiter — replaces, for the evictions of ONE nfagg_account   */
/* call, the decision of CapacityLimiter.Limit                            */
/* (pkg/flow/limiter.go:28-38): `if len(out) < cap(out) || cap(out) == 0  */
/* { out <- i } else { dropped += len(i) }`.                              */
/* ------------------------------------------------------------------ */

/* nfagg_account delivers n_epochs evictions at once (out[epoch_end[e-1] .. epoch_end[e])); the reference's limiter sees them
 * one by one on a channel and drops a whole batch when the exporter's channel is full. The shim takes this decision BEFORE it
 * builds a single model.Record (model.NewRecord per flow is the hottest allocation site, pkg/model/record_bench_test.go:10-13):
 * queue_len / queue_cap = len(out) / cap(out) of the exporter's channel now. keep[e] = 1: batch e is forwarded (it then occupies
 * one more slot of the channel; nothing is assumed to drain meanwhile: the exporter can only make the outcome better), 0: dropped.
 * *dropped_flows = the flows of the dropped batches — what the shim adds to DroppedFlowsCounter("limiter", "full") and to the
 * droppedFlows the limiter's periodic warning reports (limiter.go:33-34,41-57). queue_cap == 0 (unbuffered channel) never
 * drops (limiter.go:30). Pure host arithmetic, no device. Returns the number of batches kept. */
size_t nfagg_limit_batches(const uint64_t* epoch_end, size_t n_epochs, size_t queue_len, size_t queue_cap, uint8_t* keep,
                           uint64_t* dropped_flows);

/* pkg/model/record.go:90-97: TimeFlowStart = now - (mono_now - start_mono),
 * TimeFlowEnd likewise; uint64 wrap then signed nanoseconds, as Go does.
 * now_unix_ns is the wall clock in ns since the Unix epoch. */
void nfagg_record_times(int64_t now_unix_ns, uint64_t mono_now_ns,
                        const nfagg_flow_metrics* m,
                        int64_t* time_flow_start_unix_ns,
                        int64_t* time_flow_end_unix_ns);

enum {   /* the per-CPU feature maps, in the order of the nfagg_rollup_* entries */
    NFAGG_ROLLUP_ADDITIONAL = 0, NFAGG_ROLLUP_DNS = 1, NFAGG_ROLLUP_DROPS = 2,
    NFAGG_ROLLUP_NETWORK_EVENTS = 3, NFAGG_ROLLUP_XLAT = 4, NFAGG_ROLLUP_QUIC = 5
};
/* bits of a "present" byte: which parts of model.BpfFlowContent are non-nil */
enum {
    NFAGG_FEAT_ADDITIONAL     = 1 << NFAGG_ROLLUP_ADDITIONAL,
    NFAGG_FEAT_DNS            = 1 << NFAGG_ROLLUP_DNS,
    NFAGG_FEAT_DROPS          = 1 << NFAGG_ROLLUP_DROPS,
    NFAGG_FEAT_NETWORK_EVENTS = 1 << NFAGG_ROLLUP_NETWORK_EVENTS,
    NFAGG_FEAT_XLAT           = 1 << NFAGG_ROLLUP_XLAT,
    NFAGG_FEAT_QUIC           = 1 << NFAGG_ROLLUP_QUIC
};

/* ------------------------------------------------------------------ */
/* Per-CPU map rollup — replaces lookupAndDeletePerCPUMap's accumulator */
/* closures (pkg/tracer/tracer.go:1057-1110,1118-1146).                 */
/* ------------------------------------------------------------------ */

/* For each of n_flows flows: fold n_cpu per-CPU partials (CPU index
 * ascending; element 0 adopted whole, elements 1.. folded into it) with the
 * matching model.Accumulate* (pkg/model/flow_content.go), and apply
 * buildBaseFromAdditional (flow_content.go:63-74) to base[i] for every
 * partial. `base` is in/out: the caller passes the flow's base metrics from
 * the main map, or zeroes when the main map had no entry
 * (tracer.go:1136-1139). All pointers are HOST memory.
 *   partials: n_flows * n_cpu structs, flow-major
 *   folded:   n_flows structs */
int nfagg_rollup_additional(nfagg_handle* h, const nfagg_additional_metrics* partials,
                            size_t n_flows, size_t n_cpu,
                            nfagg_flow_metrics* base, nfagg_additional_metrics* folded);
int nfagg_rollup_dns(nfagg_handle* h, const nfagg_dns_metrics* partials,
                     size_t n_flows, size_t n_cpu,
                     nfagg_flow_metrics* base, nfagg_dns_metrics* folded);
int nfagg_rollup_drops(nfagg_handle* h, const nfagg_pkt_drop_metrics* partials,
                       size_t n_flows, size_t n_cpu,
                       nfagg_flow_metrics* base, nfagg_pkt_drop_metrics* folded);
int nfagg_rollup_network_events(nfagg_handle* h, const nfagg_network_events_metrics* partials,
                                size_t n_flows, size_t n_cpu,
                                nfagg_flow_metrics* base, nfagg_network_events_metrics* folded);
int nfagg_rollup_xlat(nfagg_handle* h, const nfagg_xlat_metrics* partials,
                      size_t n_flows, size_t n_cpu,
                      nfagg_flow_metrics* base, nfagg_xlat_metrics* folded);
int nfagg_rollup_quic(nfagg_handle* h, const nfagg_quic_metrics* partials,
                      size_t n_flows, size_t n_cpu,
                      nfagg_flow_metrics* base, nfagg_quic_metrics* folded);

/* ------------------------------------------------------------------ */
/* Map merge — replaces FlowFetcher.LookupAndDeleteMap's join            */
/* (pkg/tracer/tracer.go:1022-1116) including lookupAndDeletePerCPUMap    */
/* (:1118-1146): the caller drains the eBPF maps (syscalls stay in Go)    */
/* and hands the raw arrays over; the join by flow id, the per-CPU folds  */
/* and buildBaseFromAdditional happen on the device in one call.          */
/* ------------------------------------------------------------------ */

/* One drained map: n keys and their values. Main map (aggregated_flows):
 * values = nfagg_flow_metrics[n]. Feature map k (NFAGG_ROLLUP_*): values =
 * that map's struct[n * n_cpu], flow-major (what cilium's per-CPU Lookup
 * returns per key). A key listed twice in one map keeps its first row (the
 * reference's second LookupAndDelete fails and is skipped, :1048-1052,
 * :1130-1134); such rows are counted in *n_duplicate_keys. */
typedef struct nfagg_map_view {
    const nfagg_flow_id* ids;
    const void*          values;
    size_t               n;
} nfagg_map_view;

/* Caller-allocated outputs, `cap` entries each. records[i] = {id, base metrics
 * after every buildBaseFromAdditional}; present[i] = NFAGG_FEAT_* bits (the
 * non-nil parts of model.BpfFlowContent); part arrays hold the folded part
 * (zeroes when absent) and may be NULL when not wanted. The layout is what
 * nfagg_encode_pb_content consumes. Flows come out in order of first
 * appearance: main map first, then the feature maps in the order the reference
 * walks them (dns, drops, network events, xlat, additional, quic) — Go's map
 * order is random, so any order is valid. id byte 39 (a blank field in Go) is
 * not part of the key and is written as zero. */
typedef struct nfagg_merged_flows {
    nfagg_flow_record*            records;
    uint8_t*                      present;
    nfagg_additional_metrics*     additional;
    nfagg_dns_metrics*            dns;
    nfagg_pkt_drop_metrics*       drops;
    nfagg_network_events_metrics* network_events;
    nfagg_xlat_metrics*           xlat;
    nfagg_quic_metrics*           quic;
} nfagg_merged_flows;

/* feature_maps[k], k = NFAGG_ROLLUP_*; n = 0 for a map that is not enabled.
 * NFAGG_TRUNCATED (nothing written, *n_out = flows) when cap is too small.
 * All pointers HOST memory: */
int nfagg_map_merge(nfagg_handle* h, const nfagg_map_view* main_map, const nfagg_map_view feature_maps[6],
                    size_t n_cpu, const nfagg_merged_flows* out, size_t cap, size_t* n_out, size_t* n_duplicate_keys);
/* Same with every data pointer in DEVICE memory (8-byte aligned). */
int nfagg_map_merge_device(nfagg_handle* h, const nfagg_map_view* d_main_map, const nfagg_map_view d_feature_maps[6],
                           size_t n_cpu, const nfagg_merged_flows* d_out, size_t cap, size_t* n_out, size_t* n_duplicate_keys);

/* ------------------------------------------------------------------ */
/* Sketches — new functionality (no reference counterpart; spec in      */
/* DESIGN.md §sketches, scalar oracle in oracle/).                      */
/* ------------------------------------------------------------------ */

/* Copy a sketch to HOST memory. CM: uint64_t[depth<<log2w]; HLL: uint8_t[1<<p]. */
int nfagg_sketch_snapshot(nfagg_handle* h, int which, void* out, size_t out_bytes);
/* Device pointer and byte size of a sketch array (for in-place RCCL all-reduce:
 * CM sum uint64, HLL max uint8 — 16 KiB per array at p = 14). */
int nfagg_sketch_device_ptr(nfagg_handle* h, int which, void** d_ptr, size_t* bytes);
/* Zero all sketches (start of a sketch window). */
int nfagg_sketch_reset(nfagg_handle* h);
/* Cardinality from the device registers: integer histogram of register values
 * computed on the GPU, FP64 estimate from the histogram in a fixed order.
 * which = NFAGG_HLL_SRC / NFAGG_HLL_DST. */
int nfagg_hll_estimate(nfagg_handle* h, int which, double* estimate);
/* Count-Min point query for one 16-byte IP: min over rows. Host-side read of
 * d counters. which = NFAGG_CM_SRC / NFAGG_CM_DST. */
int nfagg_cm_query(nfagg_handle* h, int which, const uint8_t ip[16], uint64_t* estimate);
/* Heavy hitters: the k endpoints with the largest Count-Min byte estimate among the addresses that occur in `records`
 * — Count-Min stores no keys, so the candidates come from a record batch, typically the one nfagg_evict just returned
 * (the sketch is keyed by src address for NFAGG_CM_SRC, by dst address for NFAGG_CM_DST, and the same side of each
 * record is looked up). Order: estimate descending, then the 16 address bytes ascending; *n_out = min(k, distinct
 * addresses). Estimates are computed and sorted on the device; `out` is HOST memory. */
typedef struct nfagg_heavy_hitter {
    uint8_t  ip[16];
    uint64_t estimate;
} nfagg_heavy_hitter;            /* 24 bytes */
int nfagg_cm_topk(nfagg_handle* h, int which, const void* records, size_t n, size_t k,
                  nfagg_heavy_hitter* out, size_t* n_out);
/* Same with d_records in DEVICE memory (16-byte aligned), e.g. straight from nfagg_evict_device. */
int nfagg_cm_topk_device(nfagg_handle* h, int which, const void* d_records, size_t n, size_t k,
                         nfagg_heavy_hitter* out, size_t* n_out);
/* The HLL estimator itself, on a host histogram hist[0..64] of register
 * values for m = 1<<p registers (exposed so callers can estimate after a
 * cross-GPU max-merge). */
double nfagg_hll_estimate_from_histogram(const uint32_t* hist, uint32_t p);

/* ------------------------------------------------------------------ */
/* Ring-buffer drain — replaces the per-sample loop of                   */
/* RingBufTracer.listenAndForwardRingBuffer (pkg/flow/tracer_ringbuf.go:  */
/* 112-134) over ringbuf.Reader / ringReader.readRecord                   */
/* (vendor/github.com/cilium/ebpf/ringbuf/ring.go:44-101): one bulk copy  */
/* of every committed sample into a staging buffer instead of one         */
/* reflection decode + channel send per record. Host-only, no device.     */
/* ------------------------------------------------------------------ */

/* A BPF_MAP_TYPE_RINGBUF as user space maps it (kernel/bpf/ringbuf.c):
 * data = the data pages (size mask+1; the second mapping cilium relies on is
 * not required), producer_pos / consumer_pos = the two position pages. */
typedef struct nfagg_ringbuf {
    const uint8_t* data;
    uint64_t mask;                        /* data size - 1, size a power of two */
    const volatile uint64_t* producer_pos;/* written by the kernel */
    volatile uint64_t* consumer_pos;      /* written by this call   */
} nfagg_ringbuf;

/* Copies committed 144-byte samples, in ring order, into dst (room for
 * cap_records; e.g. the buffer of nfagg_staging_acquire) until the ring is
 * empty, the next sample is still busy (ring.go:67-72), or dst is full; then
 * publishes the consumer position once. Discarded samples (ring.go:84-90) and
 * samples whose length is not 144 (model.ReadFrom would fail,
 * tracer_ringbuf.go:119-122) are skipped and counted in *n_skipped.
 * errno_counts (optional, 256 entries, ADDED to): records per metrics.errno,
 * for EvictedPacketsCounter("ringbuffer", errno) (tracer_ringbuf.go:128-130).
 * Returns NFAGG_OK, or NFAGG_EINVAL when the ring content is truncated
 * (io.ErrUnexpectedEOF in the reference); nothing is consumed past that point. */
int nfagg_ringbuf_drain(const nfagg_ringbuf* rb, void* dst, size_t cap_records,
                        size_t* n_records, size_t* n_skipped, uint64_t* errno_counts);

/* ------------------------------------------------------------------ */
/* Export encode — replaces, for evicted records, model.NewRecord's time */
/* and interface derivation (pkg/model/record.go:82-125), pbflow.FlowToPB */
/* / FlowsToPB (pkg/pbflow/proto.go:18-149), proto.Marshal of each        */
/* pbflow.Record (pkg/exporter/kafka_proto.go:53; gRPC marshalling of     */
/* pbflow.Records) and getFlowKey (pkg/exporter/kafka_proto.go:37-47).    */
/* ------------------------------------------------------------------ */

/* One row of the interface namer as a table: what
 * registerer.IfaceNameForIndexAndMAC (pkg/agent/interfaces_listener.go:74-80)
 * returns for (if_index, mac), and the UDN NewIntfDirUdn (record.go:167-183)
 * resolves for that name ("" = none). Lookup: the row with this index and MAC,
 * else the first row with this index and has_mac == 0, else unknown_name. */
typedef struct nfagg_intf_name {
    uint32_t if_index;
    uint8_t  mac[6];
    uint8_t  has_mac;
    uint8_t  name_len;           /* <= 16 */
    char     name[16];
    uint8_t  udn_len;            /* <= 63 */
    char     udn[63];
} nfagg_intf_name;               /* 92 bytes */

typedef struct nfagg_pb_options {
    uint32_t struct_size;        /* sizeof(nfagg_pb_options) */
    uint32_t n_names;
    int64_t  now_unix_ns;        /* currentTime   (account.go:103 c.clock())     */
    uint64_t mono_now_ns;        /* monotonicCurrentTime (account.go:104)        */
    uint8_t  agent_ip[16];       /* Record.AgentIP as a 16-byte net.IP           */
    const nfagg_intf_name* names;/* HOST memory, n_names rows (copied per call)  */
    char     unknown_name[16];   /* the namer's answer for an unknown interface  */
    uint8_t  unknown_len;
    uint8_t  pad_[7];
} nfagg_pb_options;

/* Serialise n evicted flow_record_t. Frame i = 0x0A varint(body_len[i]) body
 * starts at frame_offsets[i]; frame_offsets[n] = *out_bytes. Any run of frames
 * [a,b) is a serialized pbflow.Records{entries a..b-1}; the last body_len[i]
 * bytes of frame i are the serialized pbflow.Record (the Kafka message value).
 * kafka_keys (optional): n x 32 bytes, getFlowKey. Records carry only
 * BpfFlowMetrics (what Accounter evicts); the per-feature messages of the
 * MapTracer branch are not produced here. Returns NFAGG_TRUNCATED with
 * *out_bytes = bytes needed when out_cap is too small (nothing written).
 * All pointers HOST memory: */
int nfagg_encode_pb(nfagg_handle* h, const void* records, size_t n, const nfagg_pb_options* opt,
                    void* out, size_t out_cap, uint64_t* frame_offsets, uint32_t* body_len,
                    void* kafka_keys, size_t* out_bytes);
/* Same with d_records / d_out / d_frame_offsets / d_body_len / d_kafka_keys in
 * DEVICE memory (16-byte aligned), e.g. straight from nfagg_evict_device. */
int nfagg_encode_pb_device(nfagg_handle* h, const void* d_records, size_t n, const nfagg_pb_options* opt,
                           void* d_out, size_t out_cap, uint64_t* d_frame_offsets, uint32_t* d_body_len,
                           void* d_kafka_keys, size_t* out_bytes);

/* The MapTracer branch (pkg/flow/tracer_map.go:103-146): every flow is a full
 * model.BpfFlowContent (pkg/model/flow_content.go:9-17) — base metrics plus the
 * optional per-feature parts that LookupAndDeleteMap merged
 * (pkg/tracer/tracer.go:1057-1110; here: the `folded` outputs of nfagg_rollup_*).
 * Struct of arrays indexed like the records; part k is present for flow i (the Go
 * pointer is non-nil) when its array is non-NULL and present[i] has
 * NFAGG_FEAT_* set. Encoded per NewRecord (record.go:116-125: DNSLatency,
 * TimeFlowRtt) and FlowToPB (proto.go:79-118,129-138: dns_id/flags/errno/name
 * via utils.DNSRawNameToDotted, dns_latency only when non-zero, pkt_drop_*, xlat
 * with the address family of the FLOW's eth_protocol, ipsec_encrypted[_ret],
 * quic). Network events (NFAGG_FEAT_NETWORK_EVENTS) need the OVN sample decoder's
 * answers: here they are encoded as NewRecord does with a nil decoder
 * (record.go:126) — field 27 empty, no drop injected; a caller with a decoder
 * uses nfagg_netev_resolve and nfagg_encode_pb_content_netev (below).
 * dns.name bytes are copied as they are (Go's Marshal rejects a non-UTF-8 string). */
typedef struct nfagg_pb_features {
    uint32_t struct_size;        /* sizeof(nfagg_pb_features) */
    uint32_t reserved_;
    const uint8_t* present;                      /* n bytes of NFAGG_FEAT_* bits (NULL: none) */
    const nfagg_additional_metrics* additional;  /* n entries or NULL */
    const nfagg_dns_metrics*        dns;
    const nfagg_pkt_drop_metrics*   drops;
    const nfagg_xlat_metrics*       xlat;
    const nfagg_quic_metrics*       quic;
} nfagg_pb_features;

/* nfagg_encode_pb over (records[i].id, BpfFlowContent{records[i].metrics, features[i]}).
 * Same outputs and return codes. All pointers HOST memory: */
int nfagg_encode_pb_content(nfagg_handle* h, const void* records, size_t n, const nfagg_pb_features* features,
                            const nfagg_pb_options* opt, void* out, size_t out_cap, uint64_t* frame_offsets,
                            uint32_t* body_len, void* kafka_keys, size_t* out_bytes);
/* Same with every data pointer (also those inside d_features) in DEVICE memory;
 * the nfagg_pb_features struct itself is in host memory. */
int nfagg_encode_pb_content_device(nfagg_handle* h, const void* d_records, size_t n, const nfagg_pb_features* d_features,
                                   const nfagg_pb_options* opt, void* d_out, size_t out_cap, uint64_t* d_frame_offsets,
                                   uint32_t* d_body_len, void* d_kafka_keys, size_t* out_bytes);

/* ------------------------------------------------------------------ */
/* IPFIX export — replaces, for evicted records, the IPFIX exporter     */
/* (EXPORT=ipfix+udp / ipfix+tcp, pkg/exporter/ipfix.go) and go-ipfix's */
/* message encoding: one IPFIX message (RFC 7011) per flow, holding one */
/* data record of the v4 or v6 template of StartIPFIXExporter.          */
/* ------------------------------------------------------------------ */

typedef struct nfagg_ipfix_options {
    uint32_t struct_size;        /* sizeof(nfagg_ipfix_options)                                   */
    uint32_t n_names;
    int64_t  now_unix_ns;        /* as nfagg_pb_options                                           */
    uint64_t mono_now_ns;
    const nfagg_intf_name* names;/* HOST memory: same table and lookup rule as nfagg_pb_options (the UDN is not used) */
    char     unknown_name[16];   /* the namer's answer for an unknown interface                   */
    uint8_t  unknown_len;
    uint8_t  pad_[3];
    uint32_t export_time_s;      /* message header Export Time: one value for every message of a call */
    uint32_t seq0;               /* sequence number of message 0; message i carries seq0 + i (mod 2^32) */
    uint32_t obs_domain_id;      /* Observation Domain ID: 1 in the reference (ipfix.go:229)      */
    uint16_t template_id_v4;     /* 256 in the reference (NewTemplateID starts at 255)            */
    uint16_t template_id_v6;     /* 257                                                           */
} nfagg_ipfix_options;

/* The template message StartIPFIXExporter sends (ipfix.go:220-262): 100 bytes,
 * header (Export Time = export_time_s, Sequence Number = seq0: the number of
 * data records sent so far, a template does not advance it), one template set
 * (ID 2) with the 19 field specifiers of the v4 (v6 == 0) or v6 template, in
 * ipfix.go's order. Host only: no handle, no device. Returns NFAGG_TRUNCATED
 * with *n_out = 100 when cap is smaller (nothing written). */
int nfagg_ipfix_template(const nfagg_ipfix_options* opt, int v6, void* out, size_t cap, size_t* n_out);

/* Encode n evicted flow_record_t as n IPFIX messages, as IPFIX.ExportFlows
 * sends them (ipfix.go:364-383): message i = out[msg_offsets[i],
 * msg_offsets[i+1]), msg_offsets[n] = *out_bytes; each is one UDP datagram or
 * one TCP write. Template v6 iff eth_protocol == 0x86DD; on v4 an address that
 * is not v4-mapped is sent as 0.0.0.0 (model.IP.To4() == nil); times and the
 * interface name as model.NewRecord derives them (record.go:82-106).
 * One difference from the reference, by design: the reference reads the clock
 * for every message's Export Time, here one export_time_s covers the whole
 * call; the bytes are identical whenever the reference's messages of a batch
 * fall within one second. Returns NFAGG_TRUNCATED with *out_bytes = bytes
 * needed when out_cap is too small (nothing written). All pointers HOST memory: */
int nfagg_encode_ipfix(nfagg_handle* h, const void* records, size_t n, const nfagg_ipfix_options* opt,
                       void* out, size_t out_cap, uint64_t* msg_offsets, size_t* out_bytes);
/* Same with d_records / d_out / d_msg_offsets in DEVICE memory (d_records and
 * d_out 16-byte aligned), e.g. straight from nfagg_evict_device. d_out may be
 * NULL to ask for the size. */
int nfagg_encode_ipfix_device(nfagg_handle* h, const void* d_records, size_t n, const nfagg_ipfix_options* opt,
                              void* d_out, size_t out_cap, uint64_t* d_msg_offsets, size_t* out_bytes);

/* ------------------------------------------------------------------ */
/* direct-FLP export — replaces, for evicted records, the direct-FLP    */
/* exporter (EXPORT=direct-flp, pkg/exporter/direct_flp.go) in front of */
/* a `write: stdout, format: json` stage: decode.RecordToMap per flow   */
/* and its JSON line, keys sorted (write_stdout.go:37-51, reorder).     */
/* ------------------------------------------------------------------ */

typedef struct nfagg_flp_options {
    uint32_t struct_size;        /* sizeof(nfagg_flp_options)                                     */
    uint32_t n_names;
    int64_t  now_unix_ns;        /* as nfagg_pb_options                                           */
    uint64_t mono_now_ns;
    const nfagg_intf_name* names;/* HOST memory: same table and lookup rule as nfagg_pb_options; names and UDNs are arbitrary bytes */
    char     unknown_name[16];   /* the namer's answer for an unknown interface                   */
    uint8_t  unknown_len;
    uint8_t  agent_ip_nil;       /* non-zero: Record.AgentIP is nil, printed as "<nil>"; agent_ip is not read */
    uint8_t  pad_[6];
    uint8_t  agent_ip[16];       /* Record.AgentIP as a 16-byte net.IP                            */
    int64_t  time_received_s;    /* "TimeReceived": one value for every line of a call            */
} nfagg_flp_options;

/* Encode n evicted flow_record_t as n JSON lines: line i = out[line_offsets[i],
 * line_offsets[i+1]), its '\n' included, line_offsets[n] = *out_bytes. Line i
 * is jsoniter.Config{SortMapKeys: true}.Marshal(decode.RecordToMap(
 * model.NewRecord(...))) + "\n" for a record that carries only BpfFlowMetrics
 * (decode_protobuf.go:57-127): compact, keys in byte order, strings escaped as
 * jsoniter's WriteString (no HTML escaping, bytes from 0x80 up copied as they
 * are), addresses as net.IP.String() of the 16-byte slice, MACs as
 * net.HardwareAddr.String(), times and interfaces as model.NewRecord derives
 * them (record.go:82-114; nb_observed_intf above 6 counts as 6).
 * Deferred records: TLSVersion, TLSCipherSuite and TLSGroup take their text
 * from Go's crypto/tls, which is not restated here. A record whose
 * ssl_version, tls_cipher_suite or tls_key_share is non-zero gets an EMPTY
 * line (line_offsets[i+1] == line_offsets[i]); deferred[i] (optional, n bytes)
 * is 1 for it and 0 otherwise, *n_deferred (optional) is their count. The
 * caller formats those records itself, or hands the names over as a table and
 * calls nfagg_encode_flp_json_tls (below), which defers nothing.
 * One difference from the reference, by design: the reference reads the clock
 * for every flow's TimeReceived, here one time_received_s covers the call.
 * Returns NFAGG_TRUNCATED with *out_bytes = bytes needed (and *n_deferred)
 * when out_cap is too small: out, line_offsets and deferred are not written.
 * All pointers HOST memory: */
int nfagg_encode_flp_json(nfagg_handle* h, const void* records, size_t n, const nfagg_flp_options* opt,
                          void* out, size_t out_cap, uint64_t* line_offsets, uint8_t* deferred,
                          size_t* n_deferred, size_t* out_bytes);
/* Same with d_records / d_out / d_line_offsets / d_deferred in DEVICE memory
 * (d_records and d_out 16-byte aligned), e.g. straight from
 * nfagg_evict_device. d_out may be NULL to ask for the size. */
int nfagg_encode_flp_json_device(nfagg_handle* h, const void* d_records, size_t n, const nfagg_flp_options* opt,
                                 void* d_out, size_t out_cap, uint64_t* d_line_offsets, uint8_t* d_deferred,
                                 size_t* n_deferred, size_t* out_bytes);

/* The MapTracer branch (pkg/flow/tracer_map.go:103-146) through direct-FLP:
 * nfagg_encode_flp_json over (records[i].id, BpfFlowContent{records[i].metrics,
 * features[i]}), `features` as for nfagg_encode_pb_content (what
 * nfagg_map_merge writes: part k is present for flow i when its array is
 * non-NULL and present[i] has its NFAGG_FEAT_* bit). The line gains, at their
 * places in byte order, the keys of decode_protobuf.go:130-192 with
 * NewRecord's DNSLatency / TimeFlowRtt (record.go:116-125):
 *   dns:        DnsErrno when non-zero; when id != 0 DnsFlags,
 *               DnsFlagsResponseCode (DNSRcodeToStr(flags & 0xF),
 *               decode_protobuf.go:426-464), DnsId, DnsLatencyMs
 *               (int64(latency) / 1e6, truncating), and DnsName when
 *               utils.DNSRawNameToDotted (pkg/utils/utils.go:18-60) is not
 *               empty, escaped as every other string of the line;
 *   drops:      when latest_drop_cause != 0 PktDropBytes, PktDropPackets,
 *               PktDropLatestFlags, PktDropLatestState (TCPStateToStr,
 *               decode_protobuf.go:199-225), PktDropLatestDropCause
 *               (PktDropCauseToStr, decode_protobuf.go:230-422, with the
 *               "NetworkEvent_" causes of network_events.go:17-28,133-138);
 *   xlat:       unless model.AllZeroIP (record.go:233-238: all zero, or
 *               ::ffff:0.0.0.0) holds for saddr or daddr: ZoneId, XlatSrcAddr,
 *               XlatDstAddr (net.IP.String() of the 16 bytes, whatever the
 *               flow's eth_protocol), XlatSrcPort / XlatDstPort when non-zero;
 *   additional: IPSecRetCode and IPSecStatus ("error" when
 *               ipsec_encrypted_ret != 0, else "success" with code 0 when
 *               ipsec_encrypted), TimeFlowRttNs when flow_rtt != 0;
 *   quic:       QuicVersion (record.go:259-270), QuicSeenLongHdr,
 *               QuicSeenShortHdr.
 * Network events (NFAGG_FEAT_NETWORK_EVENTS) need the OVN sample decoder's
 * answers: here the line is the one NewRecord gives with a nil decoder
 * (record.go:126) — no NetworkEvents key, no drop injected; a caller with a
 * decoder uses nfagg_netev_resolve and nfagg_encode_flp_json_content_netev.
 * Outputs, deferred records and return codes as nfagg_encode_flp_json;
 * features == NULL is nfagg_encode_flp_json. All pointers HOST memory: */
int nfagg_encode_flp_json_content(nfagg_handle* h, const void* records, size_t n, const nfagg_pb_features* features,
                                  const nfagg_flp_options* opt, void* out, size_t out_cap, uint64_t* line_offsets,
                                  uint8_t* deferred, size_t* n_deferred, size_t* out_bytes);
/* Same with every data pointer (also those inside d_features) in DEVICE memory,
 * e.g. the d_out of nfagg_map_merge_device; the nfagg_pb_features struct
 * itself is in host memory. */
int nfagg_encode_flp_json_content_device(nfagg_handle* h, const void* d_records, size_t n, const nfagg_pb_features* d_features,
                                         const nfagg_flp_options* opt, void* d_out, size_t out_cap, uint64_t* d_line_offsets,
                                         uint8_t* d_deferred, size_t* n_deferred, size_t* out_bytes);

/* ------------------------------------------------------------------ */
/* Network events — the part of model.NewRecord that takes the OVN      */
/* sample decoder (record.go:126-157), with the decoder's ANSWERS handed */
/* over as a table: the host asks its decoder once per distinct cookie,  */
/* the GPU does the per-flow work (look-up, `seen` de-duplication, drop   */
/* injection, the bytes of both wire formats) and names the cookies the   */
/* table does not know yet.                                              */
/* ------------------------------------------------------------------ */

enum { NFAGG_NETEV_ACL = 0,          /* *ovnmodel.ACLEvent                                       */
       NFAGG_NETEV_OTHER = 1,        /* any other ovnmodel.NetworkEvent                          */
       NFAGG_NETEV_UNDECODABLE = 2   /* DecodeCookie8Bytes returned an error (record.go:131)     */ };
enum { NFAGG_NETEV_JSON = 0, NFAGG_NETEV_PB = 1 };      /* nfagg_netev_render formats */
/* A rendered event (either format) has at most this many bytes; a longer one fails the table. The bound is what lets a
 * JSON line with four events still fit the write kernel's LDS window. The reference's own test event renders to 115 bytes,
 * two 63-byte Kubernetes names give about 330. */
#define NFAGG_NETEV_MAX_RENDERED 512
#define NFAGG_NETEV_MAX_ROWS     65535
#define NFAGG_NETEV_NO_ROW       0xFFFFu

/* What the decoder said about one cookie. Strings are arbitrary bytes, pointer and length each (NULL with length 0 is
 * the empty string); they are read during the call only. `string` is the event's String() — the library does not restate
 * ACLEvent.String(): rows whose String() bytes are equal share one de-duplication class (record.go:132-137). */
typedef struct nfagg_netev_entry {
    uint8_t  cookie[8];          /* NetworkEvents[i] as the kernel wrote it */
    uint32_t kind;               /* NFAGG_NETEV_* */
    uint32_t reserved_;
    const char* action;          /* ACL only: ACLEvent.Action, .Actor, .Name, .Namespace, .Direction */
    const char* actor;
    const char* name;
    const char* namespace_;
    const char* direction;
    const char* string;          /* ACL and OTHER: String() */
    uint32_t action_len, actor_len, name_len, namespace_len, direction_len, string_len;
} nfagg_netev_entry;

typedef struct nfagg_netev_table nfagg_netev_table;

/* Render one entry as the encoders will emit it (host only: no handle, no device; the CPU suite pins the bytes with it).
 *   NFAGG_NETEV_JSON: the JSON object of networkevents.ToMap (network_events.go:38-52), keys in byte order, values
 *     escaped as jsoniter's WriteString: ACL {"Action","Direction","Feature":"acl","Name","Namespace","Type"} with
 *     Type = Actor and empty strings still present; OTHER {"Message": String()}.
 *   NFAGG_NETEV_PB: the serialized pbflow.NetworkEvent (proto/flow.proto:27-29, proto.go:140-147): one
 *     0x0A len {0x0A klen key 0x12 vlen value} per map entry, keys in byte order, key and value written even when
 *     empty — Go's deterministic marshal.
 * NFAGG_EINVAL for an UNDECODABLE entry (it renders to nothing) and for a rendering of more than
 * NFAGG_NETEV_MAX_RENDERED bytes; NFAGG_TRUNCATED with *n_out = bytes needed when cap is smaller. */
int nfagg_netev_render(const nfagg_netev_entry* entry, int format, void* out, size_t cap, size_t* n_out);

/* Build the table from n entries, one per cookie the caller has asked its decoder about (n <= NFAGG_NETEV_MAX_ROWS).
 * Every row is rendered once, in both formats. Rows are kept sorted by the cookie's little-endian 64-bit value: ROW r of
 * the table, as nfagg_netev_resolve reports it, is the r-th cookie in that order. Per row the table also holds the
 * de-duplication class and the drop cause networkevents.ToDropReasonCode gives (network_events.go:121-131: an ACL with
 * Action "drop" -> (1 << 24) + the index of Actor in network_events.go:17-28, + 0 for an unknown actor).
 * Errors (NFAGG_EINVAL, nfagg_last_error names the entry): a duplicate cookie, an unknown kind, a rendering over the cap.
 * With a handle the table is uploaded to that handle's device and serves its calls until destroyed. h == NULL builds
 * and checks the table on the host alone (errors through nfagg_last_error(NULL)); such a table is refused by the device calls. */
int nfagg_netev_table_create(nfagg_handle* h, const nfagg_netev_entry* entries, size_t n, nfagg_netev_table** table);
void nfagg_netev_table_destroy(nfagg_netev_table* table);

/* record.go:126-157 for n flows, one GPU lane per flow. Inputs as nfagg_map_merge writes them: present (NFAGG_FEAT_*
 * bits), network_events (NULL: no flow has the part) and drops (NULL: no flow has the part, whatever present says).
 * For a flow with the network-events part, slots i = 0..3 in order, packets[i] == 0 skipped:
 *   - the cookie is looked up; a row of kind UNDECODABLE is skipped whole;
 *   - the row joins the flow's list unless an earlier row of this flow had the same class (the FIRST cookie's map stays);
 *   - a row with a drop cause injects a packet drop, also when its class was seen: drops part absent -> created with
 *     start/end of the network-events part, the cause, bytes[i], packets[i], everything else zero, and NFAGG_FEAT_DROPS
 *     set; present -> cause overwritten, bytes and packets added saturating at 65535 (flow_content.go:209-215), flags
 *     and state kept.
 * Outputs (present_out / drops_out may be the input arrays): present_out[n]; drops_out[n] (all zero for a flow without
 * the part; without a drops input NFAGG_FEAT_DROPS is set only where a drop was injected); rows_out[4n]: the table
 * rows of the flow's events in order, NFAGG_NETEV_NO_ROW for none. Every other flow is copied through.
 * A cookie the table has no row for adds nothing to its flow in this call; the distinct ones are returned in `missing`
 * (missing_cap cookies of 8 bytes, order unspecified; *n_missing = how many were stored; *overflow = 1 when there were
 * more than fit, what is stored is then a subset without duplicates). The protocol: resolve, ask the decoder about
 * the missing cookies, rebuild the table, resolve again until *n_missing == 0.
 * All pointers HOST memory: */
int nfagg_netev_resolve(nfagg_handle* h, const nfagg_netev_table* table, const uint8_t* present,
                        const nfagg_network_events_metrics* network_events, const nfagg_pkt_drop_metrics* drops, size_t n,
                        uint8_t* present_out, nfagg_pkt_drop_metrics* drops_out, uint16_t* rows_out,
                        uint8_t (*missing)[8], size_t missing_cap, size_t* n_missing, int* overflow);
/* Same with the arrays in DEVICE memory (8-byte aligned), e.g. the outputs of nfagg_map_merge_device. The missing cookies
 * come as an open-addressed set of missing_cap 64-bit slots (d_missing_set, zeroed by the call; a slot holds the
 * cookie's little-endian value, 0 = empty). The all-zero cookie, which a slot cannot hold, is reported by
 * *zero_missing = 1. *n_missing counts the distinct cookies recorded (the all-zero one included); *overflow as above. */
int nfagg_netev_resolve_device(nfagg_handle* h, const nfagg_netev_table* table, const uint8_t* d_present,
                               const nfagg_network_events_metrics* d_network_events, const nfagg_pkt_drop_metrics* d_drops, size_t n,
                               uint8_t* d_present_out, nfagg_pkt_drop_metrics* d_drops_out, uint16_t* d_rows_out,
                               uint64_t* d_missing_set, size_t missing_cap, size_t* n_missing, int* zero_missing, int* overflow);

/* nfagg_encode_pb_content with the flows' network events: `features` carries the present_out / drops_out of
 * nfagg_netev_resolve (so an injected drop is encoded as any other), `rows` its rows_out, `table` the table those rows
 * index. Field 27 (network_events_metadata, proto.go:140-147) gets one length-delimited NetworkEvent per row, between
 * dup_list and xlat; no row, no field. A row index beyond the table counts as none. Everything else as
 * nfagg_encode_pb_content. All pointers HOST memory: */
int nfagg_encode_pb_content_netev(nfagg_handle* h, const void* records, size_t n, const nfagg_pb_features* features,
                                  const uint16_t* rows, const nfagg_netev_table* table,
                                  const nfagg_pb_options* opt, void* out, size_t out_cap, uint64_t* frame_offsets,
                                  uint32_t* body_len, void* kafka_keys, size_t* out_bytes);
/* Same with every data pointer (d_rows and those inside d_features too) in DEVICE memory. */
int nfagg_encode_pb_content_netev_device(nfagg_handle* h, const void* d_records, size_t n, const nfagg_pb_features* d_features,
                                         const uint16_t* d_rows, const nfagg_netev_table* table,
                                         const nfagg_pb_options* opt, void* d_out, size_t out_cap, uint64_t* d_frame_offsets,
                                         uint32_t* d_body_len, void* d_kafka_keys, size_t* out_bytes);

/* nfagg_encode_flp_json_content with the flows' network events, inputs as for nfagg_encode_pb_content_netev. A flow
 * with at least one row gains "NetworkEvents":[obj,obj,...] (decode_protobuf.go:184-186) between Interfaces and
 * Packets; an injected drop prints its "NetworkEvent_" cause. Deferred records stay deferred, their rows are not read.
 * features may be NULL (no flow carries another part). All pointers HOST memory: */
int nfagg_encode_flp_json_content_netev(nfagg_handle* h, const void* records, size_t n, const nfagg_pb_features* features,
                                        const uint16_t* rows, const nfagg_netev_table* table,
                                        const nfagg_flp_options* opt, void* out, size_t out_cap, uint64_t* line_offsets,
                                        uint8_t* deferred, size_t* n_deferred, size_t* out_bytes);
/* Same with every data pointer in DEVICE memory. */
int nfagg_encode_flp_json_content_netev_device(nfagg_handle* h, const void* d_records, size_t n, const nfagg_pb_features* d_features,
                                               const uint16_t* d_rows, const nfagg_netev_table* table,
                                               const nfagg_flp_options* opt, void* d_out, size_t out_cap, uint64_t* d_line_offsets,
                                               uint8_t* d_deferred, size_t* n_deferred, size_t* out_bytes);

/* ------------------------------------------------------------------ */
/* TLS names — TLSVersion, TLSCipherSuite and TLSGroup of the direct-FLP */
/* line (decode_protobuf.go:99-110, record.go:240-257) take their text    */
/* from Go's crypto/tls. The library does not restate it: the caller      */
/* hands the names over as a table, built once at start from its own      */
/* crypto/tls, and the GPU does the look-up, the      */
/* fall-back formats and the bytes.                                       */
/* ------------------------------------------------------------------ */

enum { NFAGG_TLS_VERSION = 0,        /* ssl_version:      tls.VersionName(id),       unknown: 0x%04X        */
       NFAGG_TLS_CIPHER_SUITE = 1,   /* tls_cipher_suite: tls.CipherSuiteName(id),   unknown: 0x%04X        */
       NFAGG_TLS_GROUP = 2           /* tls_key_share:    tls.CurveID(id).String(),  unknown: CurveID(%d)   */ };
#define NFAGG_TLS_NAME_MAX 63        /* bytes of a name */
#define NFAGG_TLS_MAX_ROWS 256       /* rows of one kind */

typedef struct nfagg_tls_name_entry {
    uint16_t kind;               /* NFAGG_TLS_* */
    uint16_t id;
    uint32_t name_len;
    const char* name;            /* read during the call only */
} nfagg_tls_name_entry;

typedef struct nfagg_tls_names nfagg_tls_names;

/* Build the table from n entries (n == 0 is valid: every value then takes its kind's fall-back format, as does an id
 * its kind has no row for). Errors (NFAGG_EINVAL, nfagg_last_error names the entry): an unknown kind, a duplicate
 * (kind, id), an empty name, a name of more than NFAGG_TLS_NAME_MAX bytes, more than NFAGG_TLS_MAX_ROWS rows of a kind,
 * a name with a byte jsoniter's WriteString would escape (below 0x20, '"' or '\\'): every name of Go's tables is plain
 * ASCII, and refusing the others keeps the device side a plain copy and bounds how much a line can grow.
 * With a handle the table is uploaded to that handle's device and serves its calls until destroyed. h == NULL builds
 * and checks the table on the host alone (errors through nfagg_last_error(NULL)); such a table is refused by the device calls. */
int nfagg_tls_names_create(nfagg_handle* h, const nfagg_tls_name_entry* entries, size_t n, nfagg_tls_names** table);
void nfagg_tls_names_destroy(nfagg_tls_names* table);

/* The unquoted string the encoder emits for one value (host only: no handle, no device; the CPU suite pins the bytes
 * with it): the name or the kind's fall-back format, with "~ " in front for NFAGG_TLS_VERSION when mismatch != 0
 * (MiscFlagsSSLMismatch, record.go:240-257). NFAGG_TRUNCATED with *n_out = bytes needed when cap is smaller. */
int nfagg_tls_names_render(const nfagg_tls_names* table, int kind, uint16_t id, int mismatch, void* out, size_t cap, size_t* n_out);

/* The three pairs of direct-FLP entry points in one, with the TLS keys written instead of their records deferred:
 *   features == NULL                      the line of nfagg_encode_flp_json,
 *   features, rows == table == NULL       that of nfagg_encode_flp_json_content,
 *   features, rows and netev_table        that of nfagg_encode_flp_json_content_netev
 * (rows and netev_table both NULL or both set, else NFAGG_EINVAL), plus, between SrcPort and TimeFlowEndMs and in byte
 * order with TLSTypes: "TLSCipherSuite" when tls_cipher_suite != 0, "TLSGroup" when tls_key_share != 0, "TLSVersion"
 * when ssl_version != 0, each a JSON string as nfagg_tls_names_render gives it. tls_names is required and must have been
 * created for this handle. No record is deferred: every line has at least its braces, and there is neither a deferred
 * array nor a count. A record without a TLS field gets the bytes the other entry points give it. Size query (out == NULL),
 * NFAGG_TRUNCATED, alignment and n == 0 as there. All pointers HOST memory: */
int nfagg_encode_flp_json_tls(nfagg_handle* h, const void* records, size_t n, const nfagg_pb_features* features,
                              const uint16_t* rows, const nfagg_netev_table* netev_table, const nfagg_tls_names* tls_names,
                              const nfagg_flp_options* opt, void* out, size_t out_cap, uint64_t* line_offsets, size_t* out_bytes);
/* Same with every data pointer (d_rows and those inside d_features too) in DEVICE memory. */
int nfagg_encode_flp_json_tls_device(nfagg_handle* h, const void* d_records, size_t n, const nfagg_pb_features* d_features,
                                     const uint16_t* d_rows, const nfagg_netev_table* netev_table, const nfagg_tls_names* tls_names,
                                     const nfagg_flp_options* opt, void* d_out, size_t out_cap, uint64_t* d_line_offsets, size_t* out_bytes);
/* The longest line nfagg_encode_flp_json_tls can write, in bytes with its newline (policy 0: features == NULL, 1: features,
 * 2: features with network events; 0 for any other value). The write kernels size their LDS windows by it. */
uint32_t nfagg_flp_json_tls_max_line(int policy);

/* ------------------------------------------------------------------ */
/* Kubernetes enrichment — what flowlogs-pipeline's `transform network` */
/* stage adds in front of the writer NetObserv ships: add_kubernetes    */
/* for SrcAddr and for DstAddr, then add_kubernetes_infra               */
/* (pkg/pipeline/transform/kubernetes/enrich.go:37-104: Enrich with the */
/* default assignee, no label or annotation prefixes, zone on;          */
/* enrich.go:140-165: EnrichLayer and objectIsApp;                      */
/* pkg/api/transform_network.go:153-162: the key names). The informers  */
/* are not restated: the caller asks its own and hands over, per IP     */
/* address, what IndexLookup(nil, ip) returns (pod, then node, then     */
/* service; checkParent and NetworkName = "primary" applied) and the    */
/* zone fillInK8sZone would pick (a node's own label, a pod's node's).  */
/* The GPU does the per-flow work: a hash join of both addresses        */
/* against the table and a copy of the row's pre-rendered keys.         */
/*                                                                      */
/* The rule shape is fixed as NetObserv configures it: outputs SrcK8S   */
/* for SrcAddr, DstK8S for DstAddr and K8S_FlowLayer, the layer rule's  */
/* NamespaceNameFields = [(SrcK8S_Name, SrcK8S_Namespace),              */
/* (DstK8S_Name, DstK8S_Namespace)], rule order src, dst, infra.        */
/*                                                                      */
/* Differences from the reference, by design:                           */
/*  - addresses match by value, not by text: an informer string that is */
/*    not in Go's canonical form misses in Go and hits here;            */
/*  - one table serves a whole call, where the reference can see an     */
/*    informer update between two flows of a batch;                     */
/*  - a side's block of more than NFAGG_K8S_MAX_RENDERED bytes fails    */
/*    the table (Kubernetes' own bounds on names, namespaces, kinds and */
/*    label values keep a block near 1.5 KB before escapes);            */
/*  - out of scope: secondary-network keys (MAC, interface, UDN         */
/*    indexes), label and annotation copies, the otel assignee, other   */
/*    output names. Three more transform network rules are further     */
/*    down (nfagg_encode_flp_json_net); the others are out of scope.    */
/* ------------------------------------------------------------------ */

typedef struct nfagg_k8s_entry {      /* strings: pointer + length, arbitrary bytes, read during the call only */
    uint8_t ip[16];                   /* net.IP.To16(): an IPv4 address as ::ffff:a.b.c.d, as the flow id holds it */
    const char *namespace_, *name, *kind, *owner_name, *owner_kind, *network_name, *host_ip, *host_name, *zone;
    uint32_t namespace_len, name_len, kind_len, owner_name_len, owner_kind_len, network_name_len, host_ip_len, host_name_len, zone_len;
    uint8_t has_zone;                 /* the zone label exists (it may be empty: the key is then written with "") */
} nfagg_k8s_entry;

/* K8sInfraRule: a namespace that starts with one of infra_prefixes, or a (namespace, name) pair among infra_refs, is
 * infrastructure. NUL-terminated strings; infra_refs holds 2 * n_refs of them, namespace then name. */
typedef struct nfagg_k8s_layer {
    uint32_t struct_size;
    uint32_t n_prefixes;
    const char* const* infra_prefixes;
    const char* const* infra_refs;
    uint32_t n_refs;
    uint32_t pad_;
} nfagg_k8s_layer;

#define NFAGG_K8S_MAX_RENDERED 2048   /* one side's block: 181 bytes of key text, the escaped values */
#define NFAGG_K8S_MAX_ROWS (1u << 22)
#define NFAGG_K8S_NO_ROW 0xFFFFFFFFu

typedef struct nfagg_k8s_table nfagg_k8s_table;

/* One side's block as the encoder emits it behind SrcAddr (side 0: "SrcK8S_" keys) or DstAddr (side 1: "DstK8S_"), with
 * its leading comma (host only: no handle, no device). Keys in byte order: HostIP, HostName, Name, Namespace,
 * NetworkName, OwnerName, OwnerType, Type (= kind), Zone. Name, Type, OwnerName, OwnerType and NetworkName are always
 * there, even when empty; Namespace only when non-empty; HostIP only when non-empty, HostName only when HostIP and
 * HostName are both non-empty (enrich.go:81-86); Zone only when has_zone. Values are escaped as jsoniter's WriteString
 * does without HTML escaping; bytes from 0x80 up are copied. NFAGG_EINVAL for a block of more than
 * NFAGG_K8S_MAX_RENDERED bytes, NFAGG_TRUNCATED with *n_out = bytes needed when cap is smaller. */
int nfagg_k8s_render(const nfagg_k8s_entry* entry, int side, void* out, size_t cap, size_t* n_out);

/* Build the table from n entries (n == 0 is valid: no address has a row): both blocks of every row rendered once, the
 * row's app flag (its namespace is not empty and objectIsApp(namespace, name) holds for `layer`), an open-addressed table
 * keyed by the 16 address bytes (a power of two of slots, at most half in use, home slot = the low bits of
 * nfagg_ip_hash(ip, 3), linear probe). Row r, as nfagg_k8s_resolve reports it, is entries[r]. layer == NULL: the lines get
 * no K8S_FlowLayer key. Errors (NFAGG_EINVAL, nfagg_last_error names the entry): a duplicate address, a null string with
 * a length, a block over the cap, more than NFAGG_K8S_MAX_ROWS entries. Every row's host_ip TEXT is interned as well (one id per
 * row, 0 for the empty string, in an array of its own): nfagg_encode_flp_json_net's reinterpret_direction compares ids. With a handle the table is uploaded to that
 * handle's device and serves its calls until destroyed; rebuild it when the informer caches changed. h == NULL builds and
 * checks the table on the host alone (errors through nfagg_last_error(NULL)); such a table is refused by the device calls. */
int nfagg_k8s_table_create(nfagg_handle* h, const nfagg_k8s_entry* entries, size_t n, const nfagg_k8s_layer* layer, nfagg_k8s_table** table);
void nfagg_k8s_table_destroy(nfagg_k8s_table* table);

/* The hash join alone, one GPU lane per flow: rows[2i] = the row of record i's src_ip, rows[2i + 1] that of its dst_ip,
 * NFAGG_K8S_NO_ROW for an address without a row. A record whose eth_protocol is neither 0x0800 nor 0x86DD has no SrcAddr /
 * DstAddr key for Enrich to look up and gets NFAGG_K8S_NO_ROW twice, whatever its id bytes hold. All pointers HOST memory: */
int nfagg_k8s_resolve(nfagg_handle* h, const nfagg_k8s_table* table, const void* records, size_t n, uint32_t* rows);
/* Same with records and rows in DEVICE memory (records 16-byte, rows 8-byte aligned). */
int nfagg_k8s_resolve_device(nfagg_handle* h, const nfagg_k8s_table* table, const void* d_records, size_t n, uint32_t* d_rows);

/* nfagg_encode_flp_json_tls (same three policies chosen by features / rows, tls_names required, nothing deferred) plus
 * the enrichment: the dst row's block behind DstAddr, the src row's behind SrcAddr, and, for a table with a layer,
 * "K8S_FlowLayer":"app"|"infra" on every line between Interfaces and NetworkEvents / Packets: "app" when at least one side
 * resolved to a row whose app flag is set, else "infra". A record that is not IP has no address keys and so no block; it
 * still gets K8S_FlowLayer ("infra"), which EnrichLayer sets unconditionally. k8s_table is required and must have been
 * created for this handle; with an empty table and no layer the output is byte for byte that of nfagg_encode_flp_json_tls.
 * All pointers HOST memory: */
int nfagg_encode_flp_json_k8s(nfagg_handle* h, const void* records, size_t n, const nfagg_pb_features* features,
                              const uint16_t* rows, const nfagg_netev_table* netev_table, const nfagg_tls_names* tls_names,
                              const nfagg_k8s_table* k8s_table, const nfagg_flp_options* opt, void* out, size_t out_cap,
                              uint64_t* line_offsets, size_t* out_bytes);
/* Same with every data pointer (d_rows and those inside d_features too) in DEVICE memory. */
int nfagg_encode_flp_json_k8s_device(nfagg_handle* h, const void* d_records, size_t n, const nfagg_pb_features* d_features,
                                     const uint16_t* d_rows, const nfagg_netev_table* netev_table, const nfagg_tls_names* tls_names,
                                     const nfagg_k8s_table* k8s_table, const nfagg_flp_options* opt, void* d_out, size_t out_cap,
                                     uint64_t* d_line_offsets, size_t* out_bytes);
/* The longest line nfagg_encode_flp_json_k8s can write: nfagg_flp_json_tls_max_line(policy) plus two blocks at the cap
 * and ,"K8S_FlowLayer":"infra"; 0 for an unknown policy. The write kernels size their LDS windows by it. */
uint32_t nfagg_flp_json_k8s_max_line(int policy);

/* ------------------------------------------------------------------ */
/* Direction, subnet labels, TCP flag names — three more rules of the   */
/* `transform network` stage that are pure per-flow work, on top of the */
/* Kubernetes enrichment (paths under flowlogs-pipeline's pkg/):         */
/*  - reinterpret_direction                                             */
/*    (pipeline/transform/transform_network_direction.go:32-64) with    */
/*    FlowDirectionField = FlowDirection, ReporterIPField = AgentIP,    */
/*    SrcHostField = SrcK8S_HostIP, DstHostField = DstK8S_HostIP.       */
/*    decode.RecordToMap writes no FlowDirection key                    */
/*    (decode/decode_protobuf.go:57-128 has only IfDirections), so the  */
/*    IfDirectionField copy of lines 33-35 never fires: no such key.    */
/*    With s, d the two host-IP keys ("" when absent: no row, a row     */
/*    with an empty host IP, a record that is not IP) and reporter the  */
/*    text of AgentIP ("<nil>" for a nil address):                      */
/*      s != d, s == reporter                  "FlowDirection":1        */
/*      s != d, s != reporter, d == reporter   "FlowDirection":0        */
/*      s == d, s != ""                        "FlowDirection":2        */
/*      otherwise                              no key                   */
/*  - add_subnet_label for SrcAddr -> SrcSubnetLabel and DstAddr ->     */
/*    DstSubnetLabel (pipeline/transform/transform_network.go:129-146,  */
/*    166-196): the categories in configuration order, each one's CIDRs */
/*    in order, the FIRST net.IPNet.Contains hit names the label (not   */
/*    the longest prefix). An empty name still ends the search and      */
/*    writes no key. Contains compares within one family: an address is */
/*    IPv4 iff its 16 bytes are v4-mapped, a network iff its masked     */
/*    address is (for a CIDR given in IPv6 text the mask is then its    */
/*    last 32 bits): ::/0 holds no IPv4 address, 0.0.0.0/0 no IPv6 one. */
/*    A record that is not IP has no address key and gets no label. The */
/*    two-minute ipLabelCache cannot be seen between two configuration  */
/*    updates and is not restated.                                      */
/*  - decode_tcp_flags in place on Flags (transform_network.go:147-156, */
/*    utils/tcp_flags.go:8-48): the value becomes the array of the      */
/*    names whose bit is set, in table order FIN 1, SYN 2, RST 4,       */
/*    PSH 8, ACK 16, URG 32, ECE 64, CWR 128, SYN_ACK 256, FIN_ACK 512, */
/*    RST_ACK 1024; higher bits are ignored; with no known bit the      */
/*    value is a nil slice, which jsoniter writes as null               */
/*    (json-iterator/go/reflect_slice.go:28-29). Input equals output,   */
/*    so the key is always written where Flags is (IP, protocol 6).     */
/* Rule order: add_kubernetes src, dst, reinterpret_direction,          */
/* add_kubernetes_infra, the two add_subnet_label, decode_tcp_flags;    */
/* only "direction after Kubernetes" matters.                           */
/*                                                                      */
/* Differences from the reference, by design:                           */
/*  - one table serves a whole call (an Update between two flows of a   */
/*    batch cannot be seen);                                            */
/*  - the rule shape and the key names are fixed as above;              */
/*  - a label whose escaped value has more than NFAGG_NET_LABEL_MAX     */
/*    bytes, or more than NFAGG_NET_MAX_CIDRS CIDRs, fail the table;    */
/*  - none for the host-IP comparison: it is textual, as the            */
/*    reference's is. nfagg_k8s_table_create interns every row's        */
/*    host_ip text (id 0: the empty string), the call renders AgentIP   */
/*    as the line prints it and looks that text up once, and the device */
/*    compares ids. "<nil>", an agent address no row has and a host IP  */
/*    in non-canonical text behave as in the reference.                 */
/*  - out of scope: add_location, add_service (they need files the      */
/*    agent does not ship), add_subnet (unused by NetObserv).           */
/* ------------------------------------------------------------------ */

#define NFAGG_NET_REINTERPRET_DIRECTION 1u
#define NFAGG_NET_SUBNET_LABELS 2u
#define NFAGG_NET_DECODE_TCP_FLAGS 4u

#define NFAGG_NET_MAX_CIDRS 1024      /* CIDRs, and labels, of one table */
#define NFAGG_NET_LABEL_MAX 256       /* one label's escaped value, without its quotes */
#define NFAGG_NET_NO_LABEL 0xFFFFu
#define NFAGG_NET_NO_DIRECTION 0xFFu

/* One CIDR as net.ParseCIDR returns it (transform_network.go:166-183), flattened in walk order: the categories in
 * configuration order (one without CIDRs left out), each one's CIDRs in order. */
typedef struct nfagg_net_cidr {
    uint8_t ip[16];                   /* the parsed address, net.IP.To16() */
    uint32_t ones;                    /* prefix length, 0..bits */
    uint32_t bits;                    /* 32: IPv4 text, 128: IPv6 text */
    uint32_t label;                   /* index of the category's name in labels */
} nfagg_net_cidr;

typedef struct nfagg_net_label {      /* arbitrary bytes, read during the call only; len 0: the search ends, no key */
    const char* text;
    uint32_t len;
    uint32_t pad_;
} nfagg_net_label;

typedef struct nfagg_net_rules {
    uint32_t struct_size;
    uint32_t flags;                   /* NFAGG_NET_*: each rule on its own */
    const nfagg_net_cidr* cidrs;
    const nfagg_net_label* labels;
    uint32_t n_cidrs;
    uint32_t n_labels;
} nfagg_net_rules;

/* What nfagg_net_resolve writes per flow. */
typedef struct nfagg_net_row {
    uint16_t src_label, dst_label;    /* index of the first matching CIDR's label (an empty one included); NFAGG_NET_NO_LABEL: none */
    uint8_t direction;                /* 0 ingress, 1 egress, 2 inner; NFAGG_NET_NO_DIRECTION: no key */
    uint8_t pad_[3];                  /* 0 */
} nfagg_net_row;

typedef struct nfagg_net_table nfagg_net_table;

/* Build the table: every CIDR normalised to its family as Contains does (transform_network.go:170-176 and net.IPNet), every
 * label's two fragments rendered once (nfagg_net_render). rules->n_cidrs == 0 is valid: no address has a label; flags == 0 is
 * valid: the lines are those of nfagg_encode_flp_json_k8s. Errors (NFAGG_EINVAL, nfagg_last_error names the entry): ones >
 * bits, bits neither 32 nor 128, bits 32 with an address that is not v4-mapped, a label index out of range, a null label
 * with a length, a label over NFAGG_NET_LABEL_MAX, more than NFAGG_NET_MAX_CIDRS CIDRs or labels, unknown flag bits.
 * With a handle the table is uploaded to that handle's device and serves its calls until destroyed; rebuild it when the
 * stage's configuration is updated. h == NULL builds and checks the table on the host alone (errors through
 * nfagg_last_error(NULL)); such a table is refused by the device calls. */
int nfagg_net_table_create(nfagg_handle* h, const nfagg_net_rules* rules, nfagg_net_table** table);
void nfagg_net_table_destroy(nfagg_net_table* table);

/* One label's fragment as the encoder emits it behind SrcPort (side 0: ,"SrcSubnetLabel":"..") or DstPort (side 1:
 * ,"DstSubnetLabel":".."), with its leading comma; nothing (*n_out = 0) for an empty label. The value is escaped as interface
 * names are. Host only. NFAGG_TRUNCATED with *n_out = bytes needed when cap is smaller. */
int nfagg_net_render(const nfagg_net_table* table, int side, uint32_t label, void* out, size_t cap, size_t* n_out);

/* The join alone, one GPU lane per flow: a first-match walk of the CIDR list for both addresses and the direction from the
 * host-IP ids of the flow's two Kubernetes rows. k8s_rows: what nfagg_k8s_resolve wrote for these records with k8s_table
 * (both required when the table has NFAGG_NET_REINTERPRET_DIRECTION, else ignored). opt: its agent_ip / agent_ip_nil name the
 * reporter; nothing else of it is read. A rule that is off leaves its fields at "none". All pointers HOST memory: */
int nfagg_net_resolve(nfagg_handle* h, const nfagg_net_table* net_table, const nfagg_k8s_table* k8s_table, const void* records, size_t n,
                      const uint32_t* k8s_rows, const nfagg_flp_options* opt, nfagg_net_row* out);
/* Same with records, k8s_rows and out in DEVICE memory (records 16-byte, the others 8-byte aligned). */
int nfagg_net_resolve_device(nfagg_handle* h, const nfagg_net_table* net_table, const nfagg_k8s_table* k8s_table, const void* d_records,
                             size_t n, const uint32_t* d_k8s_rows, const nfagg_flp_options* opt, nfagg_net_row* d_out);

/* nfagg_encode_flp_json_k8s (same three policies, same outputs and return codes, nothing deferred) plus the rules that are
 * switched on in net_table: "FlowDirection":0|1|2 behind Flags, ,"SrcSubnetLabel":".." behind SrcPort, ,"DstSubnetLabel":".."
 * behind DstPort, and the array of names (or null) as the value of Flags. net_table is required and must have been created
 * for this handle; with no rule on the output is byte for byte that of nfagg_encode_flp_json_k8s. All pointers HOST memory: */
int nfagg_encode_flp_json_net(nfagg_handle* h, const void* records, size_t n, const nfagg_pb_features* features,
                              const uint16_t* rows, const nfagg_netev_table* netev_table, const nfagg_tls_names* tls_names,
                              const nfagg_k8s_table* k8s_table, const nfagg_net_table* net_table, const nfagg_flp_options* opt,
                              void* out, size_t out_cap, uint64_t* line_offsets, size_t* out_bytes);
/* Same with every data pointer (d_rows and those inside d_features too) in DEVICE memory. */
int nfagg_encode_flp_json_net_device(nfagg_handle* h, const void* d_records, size_t n, const nfagg_pb_features* d_features,
                                     const uint16_t* d_rows, const nfagg_netev_table* netev_table, const nfagg_tls_names* tls_names,
                                     const nfagg_k8s_table* k8s_table, const nfagg_net_table* net_table, const nfagg_flp_options* opt,
                                     void* d_out, size_t out_cap, uint64_t* d_line_offsets, size_t* out_bytes);
/* The longest line nfagg_encode_flp_json_net can write: nfagg_flp_json_k8s_max_line(policy) plus two label fragments at the
 * cap (18 bytes of key text, the quotes, NFAGG_NET_LABEL_MAX), ,"FlowDirection":2 and the eleven flag names in place of five
 * digits; 0 for an unknown policy. The write kernels size their LDS windows by it. */
uint32_t nfagg_flp_json_net_max_line(int policy);

/* The flow logs of flowlogs-pipeline's extract conntrack stage (pkg/pipeline/extract/conntrack/conntrack.go:70-74, 120-126,
 * 281-287): nfagg_encode_flp_json_net (same three policies, same tables, same outputs and return codes, nothing deferred) for
 * the flows the stage tracks, and no line for the others.
 *   - A flow is tracked when its ethertype is 0x0800 or 0x86DD and its protocol is 6, 17 or 132: the condition under which
 *     a line has SrcPort / DstPort, and the one nfagg_conn_fold applies. The encoder reads it from the record, never from
 *     the id (a tracked flow's id may be 0), and knows nothing of the store: a flow turned away by maxConnectionsTracked
 *     still has its line.
 *   - An untracked flow's line has length zero: line_offsets[i + 1] == line_offsets[i].
 *   - A tracked flow's line is byte for byte its nfagg_encode_flp_json_net line with
 *     ,"_HashId":"<hex>","_RecordType":"flowLog" in front of the closing brace; <hex> is strconv.FormatUint(hash_ids[i], 16):
 *     lower case, no padding, "0" for 0. Both keys sort behind every other key of the line.
 * hash_ids: n values, what nfagg_conn_fold wrote for these records; NULL with n > 0 is NFAGG_EINVAL.
 * All pointers HOST memory (hash_ids needs no alignment here: it is copied to the device): */
int nfagg_encode_flp_json_conn(nfagg_handle* h, const void* records, size_t n, const nfagg_pb_features* features,
                               const uint16_t* rows, const nfagg_netev_table* netev_table, const nfagg_tls_names* tls_names,
                               const nfagg_k8s_table* k8s_table, const nfagg_net_table* net_table, const uint64_t* hash_ids,
                               const nfagg_flp_options* opt, void* out, size_t out_cap, uint64_t* line_offsets, size_t* out_bytes);
/* Same with every data pointer (d_rows, d_hash_ids and those inside d_features too) in DEVICE memory; d_hash_ids 8-byte
 * aligned: the d_hash_ids of nfagg_conn_fold_device as they are. */
int nfagg_encode_flp_json_conn_device(nfagg_handle* h, const void* d_records, size_t n, const nfagg_pb_features* d_features,
                                      const uint16_t* d_rows, const nfagg_netev_table* netev_table, const nfagg_tls_names* tls_names,
                                      const nfagg_k8s_table* k8s_table, const nfagg_net_table* net_table, const uint64_t* d_hash_ids,
                                      const nfagg_flp_options* opt, void* d_out, size_t out_cap, uint64_t* d_line_offsets, size_t* out_bytes);
/* The longest line nfagg_encode_flp_json_conn can write: nfagg_flp_json_net_max_line(policy) plus 53 (the two keys with
 * sixteen hex digits); 0 for an unknown policy. The write kernels size their LDS windows by it. */
uint32_t nfagg_flp_json_conn_max_line(int policy);

/* The conversation records of extract conntrack (newConnection, endConnection, heartbeat) as JSON lines: conn.go:101-114
 * (toGenericMap: aggregates, first / last values, the keys prevail), then addHashField / addTypeField / addIsFirstField, then
 * the Kubernetes enrichment and the subnet labels of the stages behind conntrack, keys sorted. n conversations arrive as two
 * parallel arrays. CARRIERS: n ordinary 144-byte flow records that carry the connection's keys: src_ip / dst_ip / src_port /
 * dst_port as the connection stores them (after swapAB), transport_protocol, an IP ethertype; nothing else of a carrier is
 * read, and because they are flow records the Kubernetes and the net join run on them as on flows. VALUES: one
 * nfagg_conn_values each. A LAYOUT compiled from the stage's outputFields says which columns a line has. */
#define NFAGG_CONN_MAX_FIELDS 32
#define NFAGG_CONN_NAME_MAX 64
enum { NFAGG_CONN_OP_COUNT = 0, NFAGG_CONN_OP_SUM = 1, NFAGG_CONN_OP_MIN = 2, NFAGG_CONN_OP_MAX = 3, NFAGG_CONN_OP_FIRST = 4, NFAGG_CONN_OP_LAST = 5 };
enum { NFAGG_CONN_IN_NONE = 0, NFAGG_CONN_IN_BYTES = 1, NFAGG_CONN_IN_PACKETS = 2, NFAGG_CONN_IN_TIME_START = 3, NFAGG_CONN_IN_TIME_END = 4,
       NFAGG_CONN_IN_SRC_ADDR = 5, NFAGG_CONN_IN_DST_ADDR = 6, NFAGG_CONN_IN_SRC_PORT = 7, NFAGG_CONN_IN_DST_PORT = 8, NFAGG_CONN_IN_PROTO = 9,
       NFAGG_CONN_IN_SRC_MAC = 10, NFAGG_CONN_IN_DST_MAC = 11, NFAGG_CONN_IN_ETYPE = 12, NFAGG_CONN_IN_DSCP = 13, NFAGG_CONN_IN_IF_DIRECTIONS = 14 };
enum { NFAGG_CONN_RECORD_NEW = 0, NFAGG_CONN_RECORD_END = 1, NFAGG_CONN_RECORD_HEARTBEAT = 2 };

/* One outputField. Served: count (input ignored); sum over BYTES or PACKETS; min over TIME_START and max over TIME_END, not
 * split; first / last over any input from TIME_START on, not split. */
typedef struct nfagg_conn_field {
    const char* name;                 /* name_len bytes, 1..NFAGG_CONN_NAME_MAX */
    uint32_t name_len;
    uint8_t op, input, split_ab, pad_;
} nfagg_conn_field;

/* What `first` / `last` can copy from one flow, 80 bytes. */
typedef struct nfagg_conn_snapshot {
    uint8_t src_ip[16], dst_ip[16];
    uint16_t src_port, dst_port, eth_protocol;
    uint8_t proto, dscp;
    uint8_t src_mac[6], dst_mac[6];
    uint8_t n_dirs, dirs[7];          /* IfDirections: n_dirs (1..7) values */
    uint32_t pad_;
    int64_t start_ms, end_ms;
} nfagg_conn_snapshot;

typedef struct nfagg_conn_values {    /* 256 bytes */
    uint64_t hash_total;
    uint8_t record_type, is_first, pad_[6];
    uint64_t flows[2], bytes[2], packets[2];   /* AB, BA */
    int64_t start_ms_min, end_ms_max;
    nfagg_conn_snapshot first, last;
    uint64_t pad2_[2];
} nfagg_conn_values;

typedef struct nfagg_conn_layout nfagg_conn_layout;
/* Compile n_fields outputFields into a sorted column program: every key fragment (,"name": escaped as interface names are)
 * rendered once, the columns in byte order together with the five keys, the blocks (DstK8S_*, DstSubnetLabel, K8S_FlowLayer,
 * SrcK8S_*, SrcSubnetLabel; a block sorts as its prefix) and _HashId, _IsFirst, _RecordType. A split field gives name_AB and
 * name_BA. A field named as a key is dropped: the keys prevail. NFAGG_EINVAL (nfagg_last_error names the field): more than
 * NFAGG_CONN_MAX_FIELDS fields, an empty or too long name, a name beginning SrcK8S_ or DstK8S_ or equal to a block or meta
 * column, duplicates after the _AB / _BA expansion, an operation / input pair that is not served. NFAGG_ERANGE: the layout's
 * longest possible line exceeds what the write kernel's window leaves. h == NULL builds and checks on the host alone. */
int nfagg_conn_layout_create(nfagg_handle* h, const nfagg_conn_field* fields, size_t n_fields, nfagg_conn_layout** layout);
void nfagg_conn_layout_destroy(nfagg_conn_layout* layout);
uint32_t nfagg_conn_layout_columns(const nfagg_conn_layout* layout);
uint32_t nfagg_conn_layout_max_line(const nfagg_conn_layout* layout);
/* Column `column`'s fragment in sorted order (nothing for a block). Host only; NFAGG_TRUNCATED with *n_out when cap is smaller. */
int nfagg_conn_layout_render(const nfagg_conn_layout* layout, uint32_t column, void* out, size_t cap, size_t* n_out);

/* One line per conversation, columns in the layout's order. Aggregates (count, sum, min, max) are float64 in the reference and
 * omitted when zero; below 2^53 in magnitude jsoniter prints their decimal digits. A conversation with an aggregate column of
 * magnitude >= 2^53 is DEFERRED: a zero-length line, deferred[i] = 1, the caller formats it. first / last columns are written
 * even when 0. Outputs and return codes as nfagg_encode_flp_json_net; deferred (n bytes) and n_deferred may be NULL.
 * All pointers HOST memory: */
int nfagg_encode_conn_json(nfagg_handle* h, const void* carriers, const nfagg_conn_values* values, size_t n, const nfagg_conn_layout* layout,
                           const nfagg_k8s_table* k8s_table, const nfagg_net_table* net_table, void* out, size_t out_cap,
                           uint64_t* line_offsets, uint8_t* deferred, size_t* n_deferred, size_t* out_bytes);
/* Same with carriers, values, out, line_offsets and deferred in DEVICE memory (16-byte aligned). */
int nfagg_encode_conn_json_device(nfagg_handle* h, const void* d_carriers, const nfagg_conn_values* d_values, size_t n,
                                  const nfagg_conn_layout* layout, const nfagg_k8s_table* k8s_table, const nfagg_net_table* net_table,
                                  void* d_out, size_t out_cap, uint64_t* d_line_offsets, uint8_t* d_deferred, size_t* n_deferred,
                                  size_t* out_bytes);

/* ------------------------------------------------------------------ */
/* Flow metrics — the GROUP BY under flowlogs-pipeline's `encode prom`  */
/* counters (pkg/pipeline/encode/metrics_common.go:107-125 ProcessCounter, */
/* 179-211 prepareMetric, 265-295 extractLabels; pkg/api/encode_prom.go). */
/* The reference walks every flow for every metric: filters, value,     */
/* label map, a timed-cache lookup, Add. Here the device groups the     */
/* flows by a tuple of small dimension ids and sums; the host then      */
/* visits the GROUPS (thousands, not millions) and does there what      */
/* prepareMetric does per flow: filters with a real regex engine, the   */
/* value key, the label texts, Add. A metric's grouping is the set of   */
/* keys its labels AND its filters name; that is exact, because every   */
/* predicate of utils/filters/filters.go and every label value is a     */
/* function of those keys alone. Everything a counter needs per flow is */
/* on the device as small integers already: the two Kubernetes rows     */
/* (nfagg_k8s_resolve), the two label indexes and the direction         */
/* (nfagg_net_resolve), the row's app flag, and bytes, packets, the     */
/* ethertype and the protocol of the record. The sums are integers, so  */
/* the result does not depend on the order of the flows.                */
/*                                                                      */
/* Differences from the reference, by design:                           */
/*  - one table serves a whole call;                                    */
/*  - MaxMetrics and the expiry cache are the host's business: they     */
/*    depend on the order of the flows and are not restated;            */
/*  - sums are exact integers: a valueScale is applied by the host to   */
/*    the sum, not per flow;                                            */
/*  - counters and histograms: the RTT, DNS, drop and IPsec keys of a   */
/*    MapTracer flow are value sources and extra dimensions of          */
/*    nfagg_metrics_fold_content (below); gauges (last write wins),     */
/*    agg_histogram, `flatten` and the other keys outside the dimension */
/*    list (Interfaces, Dscp, ...) stay on the host path.               */
/* ------------------------------------------------------------------ */

/* One grouping is a mask of dimensions. Bit f (0..8): field f of the src row in nfagg_k8s_entry's order (namespace, name,
 * kind, owner_name, owner_kind, network_name, host_ip, host_name, zone); bit 9 + f: the same field of the dst row. */
#define NFAGG_DIM_SRC_K8S(f) (1u << (f))
#define NFAGG_DIM_DST_K8S(f) (1u << (9 + (f)))
#define NFAGG_DIM_SRC_SUBNET_LABEL (1u << 18)
#define NFAGG_DIM_DST_SUBNET_LABEL (1u << 19)
#define NFAGG_DIM_FLOW_DIRECTION (1u << 20)
#define NFAGG_DIM_FLOW_LAYER (1u << 21)
#define NFAGG_DIM_PROTO (1u << 22)
#define NFAGG_DIM_ALL ((1u << 23) - 1u)

#define NFAGG_MET_MAX_GROUPINGS 8
#define NFAGG_MET_MAX_GROUPS (1u << 20)

/* One group of one grouping. A dimension that the grouping does not select carries its "none" value in every group. */
typedef struct nfagg_metric_group {
    uint32_t src_class, dst_class;    /* nfagg_metrics_class_row turns a class back into a table row; 0: no row, or no field selected */
    uint16_t src_label, dst_label;    /* the net row's values; NFAGG_NET_NO_LABEL: none */
    uint8_t direction;                /* NFAGG_NET_NO_DIRECTION: none */
    uint8_t layer;                    /* 0: no key, 1: infra, 2: app */
    uint8_t proto;                    /* 0 unless is_ip */
    uint8_t is_ip;                    /* eth_protocol 0x0800 or 0x86DD: only then does RecordToMap write Proto (decode_protobuf.go:112-116) */
    uint64_t flows, bytes, packets;   /* sums over the group's flows (modulo 2^64) */
    /* RecordToMap omits Bytes / Packets when zero (decode_protobuf.go:87-93) and extractGenericValue then skips the flow
     * before its labels are registered (metrics_common.go:249-253): a series exists for a value key only if its count is not 0 */
    uint64_t flows_with_bytes, flows_with_packets;
    uint64_t pad_;                    /* 0 */
} nfagg_metric_group;

typedef struct nfagg_metrics_table nfagg_metrics_table;

/* Build the table of n_groupings (1..NFAGG_MET_MAX_GROUPINGS) masks over the rows of k8s_table, which must outlive it. For
 * every grouping and side each Kubernetes row gets a CLASS: the dense id, from 1 in order of first appearance, of the tuple of
 * its selected fields, each taken as (text, presence) with nfagg_k8s_render's presence: namespace and host_ip only when not
 * empty, host_name only when host_ip and host_name are both not empty, zone only with has_zone, the other five always. Two
 * rows with equal selected tuples share a class; class 0: the side has no row, or the grouping selects no field of it.
 * Unknown bits, n_groupings out of range, a null argument: NFAGG_EINVAL. With a handle (k8s_table must be of the same
 * handle) the classes are uploaded, one uint32 per row, grouping and selected side; h == NULL builds and checks the table on
 * the host alone (k8s_table built with h == NULL as well; errors through nfagg_last_error(NULL)), and the fold refuses it. */
int nfagg_metrics_table_create(nfagg_handle* h, const nfagg_k8s_table* k8s_table, const uint32_t* dims, uint32_t n_groupings,
                               nfagg_metrics_table** table);
void nfagg_metrics_table_destroy(nfagg_metrics_table* table);
/* Classes of grouping g, side 0 (src) or 1 (dst), class 0 not counted; 0 for arguments out of range. */
uint32_t nfagg_metrics_n_classes(const nfagg_metrics_table* table, uint32_t g, int side);
/* *row = the first entry index of class cls (NFAGG_K8S_NO_ROW for class 0): the caller turns a class back into strings from
 * its own entries. NFAGG_EINVAL for arguments out of range. */
int nfagg_metrics_class_row(const nfagg_metrics_table* table, uint32_t g, int side, uint32_t cls, uint32_t* row);

/* The fold. k8s_rows (2 x uint32 per record) and net_rows are what nfagg_k8s_resolve and nfagg_net_resolve wrote for these
 * records; net_rows may be NULL only if no grouping selects a label or direction dimension (else NFAGG_EINVAL). group_cap,
 * out and n_groups are arrays of n_groupings: out[g] has room for group_cap[g] (<= NFAGG_MET_MAX_GROUPS, else NFAGG_ERANGE)
 * groups and receives grouping g's groups in unspecified order, n_groups[g] their number. If any grouping has more distinct
 * groups than its cap: NFAGG_TRUNCATED, nothing is written to any out[g], n_groups[g] is exact for the groupings that fit
 * and some value greater than group_cap[g] (a lower bound) for those that did not. n == 0 is valid: no groups. All pointers
 * HOST memory: */
int nfagg_metrics_fold(nfagg_handle* h, const nfagg_metrics_table* table, const void* records, size_t n, const uint32_t* k8s_rows,
                       const nfagg_net_row* net_rows, const uint32_t* group_cap, nfagg_metric_group* const* out, uint32_t* n_groups);
/* Same with records, k8s_rows, net_rows and every out[g] in DEVICE memory (records and every out[g] 16-byte, the rows 8-byte
 * aligned); the three arrays of n_groupings themselves stay in host memory. */
int nfagg_metrics_fold_device(nfagg_handle* h, const nfagg_metrics_table* table, const void* d_records, size_t n,
                              const uint32_t* d_k8s_rows, const nfagg_net_row* d_net_rows, const uint32_t* group_cap,
                              nfagg_metric_group* const* d_out, uint32_t* n_groups);

/* ---- Histograms, and the values and labels of the feature parts (MapTracer flows).
 * A histogram (metrics_common.go:144-159, encode_prom.go:78-86, client_golang's histogram.Observe) is a GROUP BY over
 * (key, bucket) with two sums, the observation count and the sum of the values: the bucket index is one more key dimension, and
 * the hash aggregation above carries it without a bucket array per slot. The values are the integers RecordToMap writes
 * (decode_protobuf.go:130-182, record.go:116-125); a valueScale and the float bounds of a metric are the host's business: it
 * turns each float bound into the largest integer of the source's domain that the reference's float comparison still accepts,
 * which is exact because float(x) / scale does not decrease with x. Sums are exact integers as above, so the host applies the
 * scale once to a series' sum, not per flow.
 *
 * "Part present" below is nfagg_encode_pb_content's rule: the array is non-NULL and present[i] has the NFAGG_FEAT_* bit. */
#define NFAGG_MET_VALUE_NONE 0
#define NFAGG_MET_VALUE_RTT_NS 1          /* TimeFlowRttNs: additional part present and flow_rtt != 0; (int64)flow_rtt */
#define NFAGG_MET_VALUE_DNS_LATENCY_MS 2  /* DnsLatencyMs: dns part present and id != 0; (int64)latency / 1000000, truncating toward zero (a latency of 0 is a value) */
#define NFAGG_MET_VALUE_DROP_BYTES 3      /* PktDropBytes: drops part present and latest_drop_cause != 0; the 16-bit count (0 is a value) */
#define NFAGG_MET_VALUE_DROP_PACKETS 4    /* PktDropPackets: likewise */
#define NFAGG_MET_VALUE_BYTES 5           /* the record's bytes when not 0, for a histogram over them */
#define NFAGG_MET_VALUE_PACKETS 6         /* the record's packets when not 0 */
#define NFAGG_MET_VALUE_LAST 6

/* Extra dimensions, a mask of their own beside NFAGG_DIM_*. */
#define NFAGG_XDIM_DNS_RCODE 1u      /* DnsFlagsResponseCode: flags & 0xF; 0xFF unless DnsId exists (dns part present and id != 0) */
#define NFAGG_XDIM_DROP_CAUSE 2u     /* PktDropLatestDropCause: the raw 32-bit latest_drop_cause; 0: none (the drop keys exist only with a cause) */
#define NFAGG_XDIM_DROP_STATE 4u     /* PktDropLatestState: the raw latest_state; 0xFFFF unless the drop keys exist */
#define NFAGG_XDIM_IPSEC_STATUS 8u   /* IPSecStatus: 2 "error" when ipsec_encrypted_ret != 0, else 1 "success" when ipsec_encrypted, else 0: none */
#define NFAGG_XDIM_ALL 15u

#define NFAGG_MET_MAX_BOUNDS 32
#define NFAGG_MET_NO_BUCKET 0xFF     /* the flow has no value to bucket, or the grouping has no histogram */

/* One grouping: the dimensions, up to two value sources summed per group, and optionally the buckets of one of them. A flow's
 * bucket is the first k with value <= bounds[k], or n_bounds (+Inf); bounds are integer thresholds in the value's own unit and
 * must not decrease (equal neighbours occur when a scale folds several float bounds onto one integer: the first of them takes
 * the flows). A flow without value[hist - 1] gets NFAGG_MET_NO_BUCKET and is still counted in `flows`. A BYTES value above
 * INT64_MAX goes to +Inf. */
typedef struct nfagg_metric_spec {
    uint32_t struct_size;            /* sizeof(nfagg_metric_spec) */
    uint32_t dims;                   /* NFAGG_DIM_* */
    uint32_t xdims;                  /* NFAGG_XDIM_* */
    uint8_t value[2];                /* NFAGG_MET_VALUE_*; 0: the slot is empty */
    uint8_t hist;                    /* 0: no histogram; 1 / 2: bucket value[hist - 1] */
    uint8_t pad_;                    /* 0 */
    uint32_t n_bounds;               /* 1..NFAGG_MET_MAX_BOUNDS with a histogram; ignored without */
    uint32_t pad2_;
    int64_t bounds[NFAGG_MET_MAX_BOUNDS];
} nfagg_metric_spec;

/* nfagg_metrics_table_create over specs: the same opaque table, h == NULL as there. NFAGG_EINVAL, with a message that names the
 * grouping and the field, for unknown bits in dims or xdims, an unknown value source, hist > 2 or naming an empty value slot,
 * n_bounds outside 1..NFAGG_MET_MAX_BOUNDS with a histogram, bounds that decrease, a wrong struct_size. nfagg_metrics_fold[_device]
 * refuses a table made this way (NFAGG_EINVAL): its groups do not fit nfagg_metric_group. */
int nfagg_metrics_table_create_specs(nfagg_handle* h, const nfagg_k8s_table* k8s_table, const nfagg_metric_spec* specs, uint32_t n_groupings,
                                     nfagg_metrics_table** table);

/* One group of one spec, 128 bytes. The first 16 bytes are nfagg_metric_group's key fields; a dimension the grouping does not
 * select carries its "none" value. */
typedef struct nfagg_metric_group_content {
    uint32_t src_class, dst_class;
    uint16_t src_label, dst_label;
    uint8_t direction, layer, proto, is_ip;
    uint32_t drop_cause;              /* 0: none */
    uint16_t drop_state;              /* 0xFFFF: none */
    uint8_t dns_rcode;                /* 0xFF: none */
    uint8_t ipsec_status;             /* 0: none, 1: success, 2: error */
    uint8_t bucket;                   /* 0..n_bounds, or NFAGG_MET_NO_BUCKET */
    uint8_t pad_[7];                  /* 0 */
    uint64_t flows, bytes, packets, flows_with_bytes, flows_with_packets;      /* as nfagg_metric_group */
    uint64_t value_sum[2];            /* the sum of value[k] over the flows that have it: two's complement, modulo 2^64 */
    uint64_t flows_with_value[2];     /* the flows that have value[k]: extractGenericValue skips the others before their labels are registered */
    uint64_t pad2_[3];                /* 0 */
} nfagg_metric_group_content;

/* nfagg_metrics_fold over specs and the flows' feature parts. records, k8s_rows, net_rows, group_cap, n_groups, truncation,
 * NFAGG_ERANGE and n == 0 exactly as nfagg_metrics_fold; features as nfagg_encode_pb_content takes them (the struct in host
 * memory), NULL: no flow has a part. A table of nfagg_metrics_table_create is served too: each mask is a spec without values,
 * and the first 16 bytes and the five sums of a group are those nfagg_metrics_fold writes. A caller with an OVN decoder passes
 * the present / drops that nfagg_netev_resolve wrote: an injected drop counts like any other. All pointers HOST memory: */
int nfagg_metrics_fold_content(nfagg_handle* h, const nfagg_metrics_table* table, const void* records, size_t n,
                               const nfagg_pb_features* features, const uint32_t* k8s_rows, const nfagg_net_row* net_rows,
                               const uint32_t* group_cap, nfagg_metric_group_content* const* out, uint32_t* n_groups);
/* Same with records, the arrays inside d_features, the rows and every out[g] in DEVICE memory (records and out[g] 16-byte, the
 * rows and the feature arrays 8-byte aligned); the features struct and the three arrays of n_groupings stay in host memory. */
int nfagg_metrics_fold_content_device(nfagg_handle* h, const nfagg_metrics_table* table, const void* d_records, size_t n,
                                      const nfagg_pb_features* d_features, const uint32_t* d_k8s_rows, const nfagg_net_row* d_net_rows,
                                      const uint32_t* group_cap, nfagg_metric_group_content* const* d_out, uint32_t* n_groups);

/* The text the direct-FLP JSON encoders print for a raw value (DNSRcodeToStr, TCPStateToStr, PktDropCauseToStr and the
 * "NetworkEvent_" causes): the label values of the groups above. *len = the text's length; NFAGG_TRUNCATED when cap is smaller
 * (nothing written), NFAGG_EINVAL for an unknown kind or a null len. Not NUL-terminated. Pure CPU. */
#define NFAGG_FLP_ENUM_DNS_RCODE 0
#define NFAGG_FLP_ENUM_TCP_STATE 1
#define NFAGG_FLP_ENUM_DROP_CAUSE 2
int nfagg_flp_enum_name(int kind, uint32_t raw, void* out, size_t cap, size_t* len);

/* ------------------------------------------------------------------ */
/* Conversation tracking — the per-call fold under flowlogs-pipeline's  */
/* `extract conntrack` (pkg/pipeline/extract/conntrack: conntrack.go    */
/* 59-142 Extract, hash.go 41-110 computeHash, aggregator.go 144-199).  */
/* The reference walks every flow: six gob encoders and three FNV-64a   */
/* hashes, a map lookup by the 64-bit total, the aggregators, one or    */
/* two list moves. Here the device does what is per flow and order-free */
/* (the filter, the three hashes, the GROUP BY connection, the sums,    */
/* the minimum and the maximum) and the host visits CONNECTIONS: it     */
/* keeps what depends on order and on the clock (the store, the         */
/* timeouts, maxConnectionsTracked, the newConnection / heartbeat /     */
/* endConnection records). Three positions per connection make the host */
/* part exact without seeing the flows: the call's first tracked flow   */
/* of the connection (who creates it, and in which order connections    */
/* are admitted), its last one (where it ends up in the expiry list)    */
/* and its first one with FIN (where it goes terminating).              */
/*                                                                      */
/* The key definition is the one NetObserv's operator generates, fixed  */
/* here: field groups src = [SrcAddr, SrcPort], dst = [DstAddr,         */
/* DstPort], common = [Proto]; the hash over [common], A = src, B =     */
/* dst. A flow is tracked only if RecordToMap writes Proto (ethertype   */
/* 0x0800 or 0x86DD) and the protocol is 6, 17 or 132 (conntrack.go     */
/* 59-64). A field's bytes are those of a fresh gob encoder:            */
/*   [count][type id, zigzag][0x00][value]                              */
/* with 0x0c for a string (uint length, bytes: the text net.IP.String() */
/* prints) and 0x06 for the uint16 ports and the uint8 protocol (a gob  */
/* uint below 128 is one byte, else the negated byte count and the      */
/* minimal big-endian bytes). FNV-64a (offset 0xcbf29ce484222325, prime */
/* 0x100000001b3) over a group's fields gives its hash; the total is    */
/* FNV-64a over the 8 big-endian bytes of the common hash, of           */
/* min(hashA, hashB) and of the other one. These bytes are written from */
/* encoding/gob's documentation and pinned to the restatement of        */
/* tests/conntrack_ref.py, not to a Go run (tools/go/conntrack_hash_dump */
/* prints Go's values on a host that has Go).                           */
/*                                                                      */
/* Differences from the reference, by design:                           */
/*  - one `now` per call: the reference reads its clock several times   */
/*    per Extract;                                                      */
/*  - sums are exact integers, so above 2^53 a result is the correctly  */
/*    rounded sum and the reference's running float64 is not;           */
/*  - two endpoint pairs whose 64-bit totals collide are one connection */
/*    on both sides (the reference's store is keyed by the total        */
/*    alone); only the AB / BA split of such a merged connection may    */
/*    differ.                                                           */
/* The flow logs' _HashId / _RecordType in the device's JSON lines:      */
/* nfagg_encode_flp_json_conn, which takes this fold's hash_ids.        */
/* The conversation records as JSON lines: nfagg_encode_conn_json.      */
/* Not here: a store                                                    */
/* that lives in device memory across calls; a least and a greatest     */
/* Bytes / Packets, and extremes per direction (the partial carries one */
/* least start, one greatest end).                                      */
/* ------------------------------------------------------------------ */

#define NFAGG_CONN_MAX_CONNS (1u << 22)
#define NFAGG_CONN_NO_IDX 0xFFFFFFFFu

typedef struct nfagg_conn_options {
    uint32_t struct_size;             /* sizeof(nfagg_conn_options) */
    uint32_t reserved_;               /* 0 */
    int64_t now_unix_ns;              /* currentTime and the monotonic clock at that instant, as in nfagg_flp_options: */
    uint64_t mono_now_ns;             /*   TimeFlowStartMs / TimeFlowEndMs are record.go:90-97's times in milliseconds */
} nfagg_conn_options;

/* What one call's tracked flows of one connection fold to, 128 bytes. "Same" (index 0) are the flows whose hashA equals
 * first_hash_a, "other" (index 1) the rest: the host maps them to AB / BA by comparing first_hash_a with the connection's
 * stored hashA. */
typedef struct nfagg_conn_partial {
    uint64_t hash_total;              /* the connection's 64-bit total (_HashId is its lower-case hex) */
    uint64_t first_hash_a;            /* hashA of the flow at first_idx */
    uint32_t first_idx, last_idx;     /* least and greatest position of the connection's tracked flows in this call */
    uint32_t first_fin_idx;           /* least position of a TCP flow with FIN (0x01) in Flags, else NFAGG_CONN_NO_IDX */
    uint32_t flags_or;                /* OR of the TCP flows' Flags (only protocol 6 has the key) */
    uint64_t flows[2], bytes[2], packets[2];   /* exact integer sums (modulo 2^64) */
    int64_t start_ms_min, end_ms_max; /* least TimeFlowStartMs, greatest TimeFlowEndMs */
    uint64_t pad_[4];                 /* 0 */
} nfagg_conn_partial;

/* Fold n records (HOST memory). hash_ids (n values, may be NULL) receives every flow's total, 0 for a flow the filter
 * discards; *n_discarded their number. out has room for cap (<= NFAGG_CONN_MAX_CONNS, else NFAGG_ERANGE) partials and
 * receives the call's connections in unspecified order (first_idx is unique per connection: sort by it), *n_conns their
 * number. More connections than cap: NFAGG_TRUNCATED, nothing is written to out, *n_conns is some value greater than cap (a
 * lower bound), hash_ids and *n_discarded are complete. n == 0 is valid: NFAGG_OK, nothing written. n above 2^32 - 2:
 * NFAGG_ERANGE. The connections live in an open-addressed table of max(1024, the power of two >= 2 * min(cap, n)) slots,
 * probed linearly from the low bits of fmix64(hash_total) (MurmurHash3's 64-bit finalizer). */
int nfagg_conn_fold(nfagg_handle* h, const void* records, size_t n, const nfagg_conn_options* opt, uint64_t* hash_ids, uint32_t cap,
                    nfagg_conn_partial* out, uint32_t* n_conns, uint32_t* n_discarded);
/* Same with records, hash_ids and out in DEVICE memory (records and out 16-byte, hash_ids 8-byte aligned). */
int nfagg_conn_fold_device(nfagg_handle* h, const void* d_records, size_t n, const nfagg_conn_options* opt, uint64_t* d_hash_ids,
                           uint32_t cap, nfagg_conn_partial* d_out, uint32_t* n_conns, uint32_t* n_discarded);
/* The three hashes of one 144-byte record as the fold computes them: returns the total, *hash_a and *hash_b (either may be
 * NULL) the endpoint hashes. A record the filter discards, or record == NULL: 0, and 0 in both. Pure CPU, no handle. */
uint64_t nfagg_conn_hash(const void* record, uint64_t* hash_a, uint64_t* hash_b);

/* ------------------------------------------------------------------ */
/* transform filter — flowlogs-pipeline's `transform filter` stage      */
/* (paths under flowlogs-pipeline's pkg/: pipeline/transform/           */
/* transform_filter.go, dsl/lexer.go, dsl/expr.y, dsl/eval.go,          */
/* utils/filters/filters.go, utils/convert.go) for the flows of         */
/* decode.RecordToMap (the agent's pkg/decode/decode_protobuf.go:57-195) */
/* behind the Kubernetes and the transform network enrichment above.    */
/* The reference walks every flow through a predicate tree: a map       */
/* lookup per atom, reflection in ConvertToInt. Every predicate of      */
/* filters.go is a function of a handful of keys, and those keys are on */
/* the device as small integers already (the metrics section above): a  */
/* filter is a short boolean program, the same for every flow, and a    */
/* stable compaction behind it. Every encoder and fold then runs        */
/* unchanged on the kept flows.                                         */
/*                                                                      */
/* Stage order (transform_filter.go:55-95 Transform, 234-261 configure): */
/*  - configure splits the rules: every keep_entry_query goes to        */
/*    KeepRules in configuration order, wherever it stands; the others  */
/*    keep their order (243-254).                                       */
/*  - With at least one keep rule a flow survives only if some rule's   */
/*    predicate is true and that rule's roll succeeds (62-73, 192-206   */
/*    applyKeepPredicate). A flow sampled out of rule r is still        */
/*    offered to rule r + 1: applyKeepPredicate returns false and the   */
/*    loop goes on. The first admitting rule ends the loop.             */
/*  - Then the remaining rules, in order; the first that removes the    */
/*    flow ends it (74-78).                                             */
/* Sampling (217-232): rollSampling passes for value 0, else one chance */
/* in `value`. storeSampling runs only for an admitting keep rule with  */
/* keepEntrySampling > 0 and a samplingField: Sampling becomes          */
/* max(Sampling, 1) * value, an absent key counting as 1.               */
/* conditional_sampling never stores (208-215). The rules behind the    */
/* keep rules see the multiplied value.                                 */
/* The other rule types (99-122, 168-171, 181-189):                     */
/*  - remove_entry_if_exists / _if_doesnt_exist: the key's presence;    */
/*  - remove_entry_if_equal / _if_not_equal compare interface{} values  */
/*    with == / != (113, 119): a YAML number (int or float64) never     */
/*    equals a uint8 / uint16 / uint32 / uint64 / int64 map value, so   */
/*    if_equal with a number is constant false and if_not_equal with a  */
/*    number removes whenever the key exists; only strings compare;     */
/*  - remove_entry_all_satisfied: the AND of its entries;               */
/*  - conditional_sampling: the first condition whose rules are all     */
/*    satisfied decides: its value is rolled, a failed roll drops.      */
/* The query language (dsl): text/scanner tokens in its default mode    */
/* (identifiers, decimal integers, "..." through strconv.Unquote, raw   */
/* strings, comments skipped; a float is an error, lexer.go:187-189;    */
/* 0x10 scans as an Int and fails ParseInt(s, 10, 64), 178-184); the    */
/* two-character operators by peeking one rune (203-209); and / or /    */
/* with / without in any letter case (211). There is no unary minus: a  */
/* leading '-' is an NF_FIELD token and a syntax error. expr.y:16-17    */
/* declares %left AND before %left OR, and yacc gives a LATER line the  */
/* higher precedence: OR binds tighter than AND, `a and b or c` is      */
/* `a and (b or c)`; both are left-associative. The generated tables   */
/* of expr.y.go agree: the state behind `expr AND expr` shifts on OR.   */
/* Predicates (filters.go, convertString == false as lexer.go:61,67     */
/* pass it): `=` with a string is true only for a key whose value is a  */
/* Go string equal to it (57-62), so constant false on a numeric key;   */
/* `!=` is its negation (65-68), true for an absent key. The six        */
/* numeric comparisons go through ConvertToInt (94-103; convert.go      */
/* 178-213): every integer type converts, uint64 wraps into int, a      */
/* string goes through ParseInt, a slice fails and the predicate is     */
/* false. =~ / !~ match unanchored over ConvertToString (105-121). A    */
/* $(Key) variable in an `=` value (29-44) is not served.               */
/* Division of labour, as for nfagg_metrics_table_create's classes: a   */
/* predicate over a STRING key (a Kubernetes field, a subnet label, the */
/* flow layer, the DNS response code, the IPsec status) is evaluated by */
/* the caller once per table row, whatever its operator, because only   */
/* the caller has a regex engine; the device looks the answer up.       */
/*                                                                      */
/* Differences from the reference, by design:                           */
/*  - the roll: Go's generator is seeded from the clock                 */
/*    (transform_filter.go:39), so there is no sequence to reproduce.   */
/*    Here a roll is a pure function of (seed, flow index, step), see   */
/*    nfagg_filter_roll;                                                */
/*  - Sampling is stored in the record's 32 bits: a product that does   */
/*    not fit defers the flow to the host (keep = 2);                   */
/*  - field-mutating rules (add_*, remove_field, the label rules) are   */
/*    not served: such a stage stays on the host path.                  */
/* ------------------------------------------------------------------ */

#define NFAGG_FILTER_MAX_ATOMS 64
#define NFAGG_FILTER_MAX_OPS   256
#define NFAGG_FILTER_MAX_STEPS 32
#define NFAGG_FILTER_MAX_STACK 32
#define NFAGG_FILTER_NO_RULE   0xFFu

enum { NFAGG_FILTER_ATOM_CONST = 0,     /* value_const != 0 */
       NFAGG_FILTER_ATOM_NUM = 1,       /* the key `field` exists, is a number, and (int)value_of_key `cmp` value */
       NFAGG_FILTER_ATOM_PRESENT = 2,   /* the key `field` exists */
       NFAGG_FILTER_ATOM_TABLE = 3,     /* truth[the flow's index in dimension `dim`] != 0 */
       NFAGG_FILTER_ATOM_ADDR = 4,      /* SrcAddr (side 0) / DstAddr (side 1) exists and its 16 bytes equal bytes[0..16) */
       NFAGG_FILTER_ATOM_MAC = 5 };     /* SrcMac / DstMac: its 6 bytes equal bytes[0..6) */
enum { NFAGG_FILTER_CMP_EQ = 0, NFAGG_FILTER_CMP_NE = 1, NFAGG_FILTER_CMP_LT = 2, NFAGG_FILTER_CMP_GT = 3, NFAGG_FILTER_CMP_LE = 4,
       NFAGG_FILTER_CMP_GE = 5 };
/* Fields of NUM and PRESENT atoms: when the key exists (decode_protobuf.go:63-182 and the enrichment rules above) and the
 * int ConvertToInt gives. "IP": eth_protocol 0x0800 or 0x86DD. A part is present as nfagg_encode_pb_content has it. */
enum { NFAGG_FILTER_F_ETYPE = 0,             /* always; eth_protocol */
       NFAGG_FILTER_F_BYTES = 1,             /* bytes != 0; (int64)bytes: 2^63 and above is negative */
       NFAGG_FILTER_F_PACKETS = 2,           /* packets != 0 */
       NFAGG_FILTER_F_SAMPLING = 3,          /* sampling != 0, or an admitting keep rule stored it; the stored value */
       NFAGG_FILTER_F_PROTO = 4,             /* IP */
       NFAGG_FILTER_F_DSCP = 5,              /* IP */
       NFAGG_FILTER_F_SRC_PORT = 6,          /* IP and protocol 6, 17 or 132 */
       NFAGG_FILTER_F_DST_PORT = 7,
       NFAGG_FILTER_F_ICMP_TYPE = 8,         /* IP and protocol 1 or 58 */
       NFAGG_FILTER_F_ICMP_CODE = 9,
       NFAGG_FILTER_F_FLAGS = 10,            /* IP and protocol 6. With NFAGG_NET_DECODE_TCP_FLAGS in the net table the value is a
                                                []string: the key exists, every NUM atom on it is false */
       NFAGG_FILTER_F_TIME_FLOW_START_MS = 11,   /* always; opt's clocks as nfagg_record_times, in milliseconds (time.Time.UnixMilli) */
       NFAGG_FILTER_F_TIME_FLOW_END_MS = 12,
       NFAGG_FILTER_F_FLOW_DIRECTION = 13,   /* the net row's direction is 0, 1 or 2 */
       NFAGG_FILTER_F_TIME_FLOW_RTT_NS = 14, /* additional part, flow_rtt != 0; (int64)flow_rtt */
       NFAGG_FILTER_F_DNS_LATENCY_MS = 15,   /* dns part, id != 0; (int64)latency / 1000000 */
       NFAGG_FILTER_F_DNS_ID = 16,           /* dns part, id != 0 */
       NFAGG_FILTER_F_DNS_FLAGS = 17,        /* dns part, id != 0 */
       NFAGG_FILTER_F_DNS_ERRNO = 18,        /* dns part, errno != 0 */
       NFAGG_FILTER_F_PKT_DROP_BYTES = 19,   /* drops part, latest_drop_cause != 0 */
       NFAGG_FILTER_F_PKT_DROP_PACKETS = 20,
       NFAGG_FILTER_F_PKT_DROP_LATEST_FLAGS = 21,
       NFAGG_FILTER_F_IPSEC_RET_CODE = 22,   /* additional part, ipsec_encrypted_ret != 0 or ipsec_encrypted; the int32 */
       NFAGG_FILTER_F_NUM_LAST = 22,
       /* presence only: a NUM atom on them is refused */
       NFAGG_FILTER_F_SRC_ADDR = 23,         /* IP */
       NFAGG_FILTER_F_DST_ADDR = 24,
       NFAGG_FILTER_F_SRC_MAC = 25,          /* always */
       NFAGG_FILTER_F_DST_MAC = 26,
       NFAGG_FILTER_F_LAST = 26 };
/* Dimensions of TABLE atoms and their truth entries; the last entry is the answer for "none". */
enum { NFAGG_FILTER_DIM_SRC_K8S_ROW = 0,     /* k8s table rows + 1: the flow's src row as nfagg_k8s_resolve wrote it; last: no row */
       NFAGG_FILTER_DIM_DST_K8S_ROW = 1,
       NFAGG_FILTER_DIM_SRC_SUBNET_LABEL = 2,/* net table labels + 1: the net row's src_label; last: NFAGG_NET_NO_LABEL */
       NFAGG_FILTER_DIM_DST_SUBNET_LABEL = 3,
       NFAGG_FILTER_DIM_FLOW_LAYER = 4,      /* 3: [0] infra, [1] app, [2] no key (a table without a layer) */
       NFAGG_FILTER_DIM_DNS_RCODE = 5,       /* 17: flags & 0xF where DnsId exists; [16] no key */
       NFAGG_FILTER_DIM_IPSEC_STATUS = 6,    /* 3: [0] success, [1] error, [2] no key */
       NFAGG_FILTER_DIM_LAST = 6 };
/* The postfix stream: a byte below NFAGG_FILTER_MAX_ATOMS pushes that atom's value. */
enum { NFAGG_FILTER_OP_AND = 0x80, NFAGG_FILTER_OP_OR = 0x81, NFAGG_FILTER_OP_NOT = 0x82 };
enum { NFAGG_FILTER_STEP_KEEP = 0,           /* a keep_entry_query; value: keepEntrySampling. KEEP steps come first */
       NFAGG_FILTER_STEP_REMOVE = 1,         /* the flow is dropped when the predicate is true */
       NFAGG_FILTER_STEP_SAMPLE_IF = 2 };    /* one condition of a conditional_sampling rule `group` (0..31): within a group the
                                                first true predicate decides, its value is rolled, a failed roll drops */
#define NFAGG_FILTER_STORE_SAMPLING 1u       /* samplingField == "Sampling" */

typedef struct nfagg_filter_atom {           /* 48 bytes */
    uint8_t kind;                            /* NFAGG_FILTER_ATOM_* */
    uint8_t field;                           /* NUM, PRESENT */
    uint8_t cmp;                             /* NUM */
    uint8_t dim;                             /* TABLE */
    uint8_t side;                            /* ADDR, MAC: 0 src, 1 dst */
    uint8_t value_const;                     /* CONST */
    uint8_t pad_[2];                         /* 0 */
    int64_t value;                           /* NUM */
    uint8_t bytes[16];                       /* ADDR: net.IP.To16(); MAC: the first 6 */
    const uint8_t* truth;                    /* TABLE: HOST memory, n_truth bytes, read during nfagg_filter_create only */
    uint32_t n_truth;
    uint32_t pad2_;
} nfagg_filter_atom;

typedef struct nfagg_filter_step {           /* 8 bytes */
    uint8_t kind;                            /* NFAGG_FILTER_STEP_* */
    uint8_t group;                           /* SAMPLE_IF */
    uint16_t value;                          /* KEEP, SAMPLE_IF: the sampling value, 0: always passes */
    uint16_t op_begin, op_count;             /* the step's slice of ops: it leaves exactly one value on the stack */
} nfagg_filter_step;

typedef struct nfagg_filter_spec {
    uint32_t struct_size;                    /* sizeof(nfagg_filter_spec) */
    uint32_t flags;                          /* NFAGG_FILTER_STORE_SAMPLING */
    uint32_t n_atoms, n_ops, n_steps, pad_;
    const nfagg_filter_atom* atoms;
    const uint8_t* ops;
    const nfagg_filter_step* steps;
} nfagg_filter_spec;

typedef struct nfagg_filter nfagg_filter;

/* Check and compile a spec. k8s_table / net_table: the tables whose rows the TABLE atoms index (either may be NULL when no atom
 * needs it; the flow layer needs k8s_table, FlowDirection neither); NFAGG_NET_DECODE_TCP_FLAGS of net_table decides what Flags
 * is. Errors (NFAGG_EINVAL, nfagg_last_error names the atom, op or step): more atoms, ops or steps than the limits, an unknown
 * kind, field, comparison, dimension, side, op or step kind, a NUM atom on a presence-only field, a TABLE atom whose table is
 * NULL, whose truth is NULL or whose n_truth is not what its dimension has, an op that names an atom beyond n_atoms, a slice
 * beyond n_ops, a stack that underflows, grows beyond NFAGG_FILTER_MAX_STACK or does not end with exactly one value, a KEEP
 * step behind another kind, a group above 31, non-zero padding, a wrong struct_size. A spec with no steps is valid: it keeps
 * everything. With a handle (the tables must be of the same handle) the program and the truth bytes are uploaded; h == NULL
 * checks on the host alone (tables built with h == NULL; errors through nfagg_last_error(NULL)), and nfagg_filter_apply
 * refuses such a filter. The tables must outlive the filter. */
int nfagg_filter_create(nfagg_handle* h, const nfagg_k8s_table* k8s_table, const nfagg_net_table* net_table, const nfagg_filter_spec* spec,
                        nfagg_filter** filter);
void nfagg_filter_destroy(nfagg_filter* filter);

/* The roll: sampled in (1) or out (0). value 0: 1. Else with fmix64 MurmurHash3's 64-bit finalizer and K = 0x9E3779B97F4A7C15
 * (all arithmetic modulo 2^64)
 *   u = fmix64(fmix64(seed + K * flow_index) ^ (K * (step + 1)))
 * and the flow is in iff u % value == 0. flow_index = first_index + the flow's position in the call, step = the index of the
 * KEEP or SAMPLE_IF step in the spec. Pure CPU; the device computes the same. */
int nfagg_filter_roll(uint64_t seed, uint64_t flow_index, uint32_t step, uint32_t value);

/* Run the filter over n records and compact. features (optional) as nfagg_encode_pb_content takes them: NULL, or a part's
 * array NULL, means no flow has it. k8s_rows / net_rows: what nfagg_k8s_resolve / nfagg_net_resolve wrote for these records;
 * required (NFAGG_EINVAL) when the program reads them, else ignored. opt: its now_unix_ns / mono_now_ns are read, and only by
 * a program that names TimeFlowStartMs / TimeFlowEndMs (then required). seed, first_index: the roll's; pass first_index = the
 * flows handed to earlier calls so that consecutive calls do not reuse rolls.
 *   keep[i]      0 dropped, 1 kept, 2 kept and DEFERRED: an admitting keep rule stores max(sampling, 1) * value and the product
 *                does not fit the record's 32 bits; the record is copied with sampling unchanged and the caller formats it.
 *   rule[i]      the admitting KEEP step, NFAGG_FILTER_NO_RULE if none (no keep rule, or the flow was not admitted)
 *   kept_idx[j]  the index of the j-th kept flow, ascending: the compaction is stable
 *   out_records  (optional) the kept records, dense, sampling rewritten where a keep rule stored it
 * keep and rule have n entries, kept_idx and out_records room for cap; any of the four may be NULL. *n_kept (required) is
 * exact always; *n_deferred (optional). NFAGG_TRUNCATED when *n_kept > cap and kept_idx or out_records is asked for: neither is
 * written, keep and rule are. n == 0 is valid; n above 2^32 - 2: NFAGG_ERANGE. All pointers HOST memory: */
int nfagg_filter_apply(nfagg_handle* h, const nfagg_filter* filter, const void* records, size_t n, const nfagg_pb_features* features,
                       const uint32_t* k8s_rows, const nfagg_net_row* net_rows, const nfagg_flp_options* opt, uint64_t seed, uint64_t first_index,
                       uint8_t* keep, uint8_t* rule, uint32_t* kept_idx, void* out_records, size_t cap, size_t* n_kept, size_t* n_deferred);
/* Same with records, the arrays inside d_features, the rows and the four outputs in DEVICE memory (records and out_records
 * 16-byte, the rows and the feature arrays 8-byte, kept_idx 4-byte aligned); the features struct is in host memory.
 * d_out_records must not overlap d_records, nor d_kept_idx any input: the compaction reads the records of other waves while it
 * writes, so a call in place would race. */
int nfagg_filter_apply_device(nfagg_handle* h, const nfagg_filter* filter, const void* d_records, size_t n, const nfagg_pb_features* d_features,
                              const uint32_t* d_k8s_rows, const nfagg_net_row* d_net_rows, const nfagg_flp_options* opt, uint64_t seed,
                              uint64_t first_index, uint8_t* d_keep, uint8_t* d_rule, uint32_t* d_kept_idx, void* d_out_records, size_t cap,
                              size_t* n_kept, size_t* n_deferred);

/* dst[j] = src[kept_idx[j]] for the side arrays that travel with the records (k8s_rows, net_rows, hash_ids, present, the
 * part arrays, the network-event rows): n_src elements of elem_bytes each, elem_bytes 1, 2, 4, 8 or a multiple of 8 up to 64
 * (else NFAGG_EINVAL). An index from n_src up yields a zeroed element. n_kept == 0 is valid. All pointers HOST memory: */
int nfagg_gather(nfagg_handle* h, const void* src, size_t n_src, size_t elem_bytes, const uint32_t* kept_idx, size_t n_kept, void* dst);
/* Same in DEVICE memory: src and dst aligned to elem_bytes for 1, 2, 4, to 8 otherwise (16 lets a multiple of 16 move in
 * 16-byte units), kept_idx to 4. */
int nfagg_gather_device(nfagg_handle* h, const void* d_src, size_t n_src, size_t elem_bytes, const uint32_t* d_kept_idx, size_t n_kept, void* d_dst);

/* ------------------------------------------------------------------ */
/* Sharding, stats, sync                                                */
/* ------------------------------------------------------------------ */

/* Shard of a flow key: the function that routes records to GPUs
 * (hash of the 40 key bytes with byte 39 forced to 0). */
uint32_t nfagg_shard_of(const nfagg_flow_id* id, uint32_t n_shards);
/* Host-side router: shard id of each of n 144-byte records (HOST memory), for a
 * caller that feeds one handle per GPU. Pure CPU; no device needed. */
void nfagg_shard_ids(const void* records, size_t n, uint32_t n_shards, uint32_t* out_shard);
/* The 64-bit key hash itself (table index / fingerprint / shard all derive from it). */
uint64_t nfagg_key_hash(const nfagg_flow_id* id);
/* The 64-bit hash of a 16-byte IP with the given seed index (0..3): 0..2 as used
 * by the sketches, 3 by the Kubernetes table. */
uint64_t nfagg_ip_hash(const uint8_t ip[16], uint32_t seed_index);
/* The 64-bit hash that places a group of grouping index `grouping` (0..NFAGG_MET_MAX_GROUPINGS - 1) in the tables of
 * nfagg_metrics_fold; only the eight key fields of *key are read. Pure CPU. The key is packed into two 64-bit halves
 *   A = 1<<63 | grouping<<58 | dst_class<<29 | src_class
 *   B = 1<<63 | grouping<<56 | is_ip<<50 | proto<<42 | layer<<40 | direction<<32 | dst_label<<16 | src_label
 * and the hash is fmix64((rotl64(A * K, 27) ^ B) * K) with K = 0x9E3779B97F4A7C15 and MurmurHash3's 64-bit finalizer
 * fmix64. A table of 2^k slots is probed linearly from the hash's low k bits. key == NULL or a grouping out of range: 0. */
uint64_t nfagg_metrics_group_hash(uint32_t grouping, const nfagg_metric_group* key);
/* The same for a group of nfagg_metrics_fold_content; the thirteen key fields of *key are read. Three 64-bit words, A and B as
 * above and
 *   C = 1<<63 | grouping<<56 | (bucket & 0x3F)<<48 | ipsec_status<<46 | (dns_rcode & 0x1F)<<41 | (drop_state & 0x1FF)<<32 | drop_cause
 * (the masks keep the "none" values apart from every real one: a bucket is at most 32, a response code at most 15, a state at
 * most 255), and the hash is fmix64((rotl64(H, 27) ^ C) * K) with H the two-word hash above. key == NULL, a grouping out of
 * range, a bucket above NFAGG_MET_MAX_BOUNDS other than NFAGG_MET_NO_BUCKET or an ipsec_status above 2: 0. */
uint64_t nfagg_metrics_group_hash_content(uint32_t grouping, const nfagg_metric_group_content* key);

int nfagg_stats_get(nfagg_handle* h, nfagg_stats* out);
int nfagg_stats_reset_profile(nfagg_handle* h);
/* Wait until all submitted work of this handle has finished. */
int nfagg_sync(nfagg_handle* h);
/* The hipStream_t the handle launches on (as void*), for event timing by the caller. */
void* nfagg_stream(nfagg_handle* h);
/* ------------------------------------------------------------------ */
/* Multi-GPU group — N devices behind ONE process.                      */
/* The agent is one process with one pipeline (pkg/agent/agent.go:387-442;  */
/* the Accounter is built at agent.go:208-212), so its N GPUs are driven   */
/* from that process: flows shard by key hash (nfagg_shard_of), member i    */
/* is an ordinary handle owning shard i. A batch enters on one member's     */
/* device, is partitioned there in arrival order (stable device partition)  */
/* and the buckets go to their owners over xGMI; every owner folds its      */
/* bucket. Flow state needs no collective; the Count-Min / HyperLogLog      */
/* arrays are all-reduced with RCCL at the eviction tick (librccl is        */
/* loaded on demand; a single-GPU process never loads it).                  */
/* ------------------------------------------------------------------ */
typedef struct nfagg_group nfagg_group;

/* cfg as for nfagg_create, except: device / n_shards / shard_id / ext_sketch are set per member, and max_entries is
 * CACHE_MAX_FLOWS for the whole group — every shard holds at most ceil(max_entries / n_devices) flows.
 * devices: HIP ordinals, one per member; all distinct (production), or all equal (several members on ONE GPU: lets a
 * single-GPU box exercise partition, routing and the stop-on-full logic; the sketch merge then runs as local kernels). */
int nfagg_group_create(const nfagg_config* cfg, const int32_t* devices, uint32_t n_devices, nfagg_group** out);
void nfagg_group_destroy(nfagg_group* g);
const char* nfagg_group_last_error(const nfagg_group* g);   /* NULL: last create error */
uint32_t nfagg_group_size(const nfagg_group* g);
/* Member i (shard i): sketch queries, stats, device-side export (nfagg_encode_pb_device ...) go through its handle.
 * Do not ingest into or evict a member directly. */
nfagg_handle* nfagg_group_member(nfagg_group* g, uint32_t i);

/* The record arm of Accounter.Account (account.go:81-96) for the group: records in HOST memory, in arrival order.
 * Chunks go up the members' PCIe links in turn (pinned staging ring of the member), are partitioned on that device
 * and routed. Returns NFAGG_FULL with *consumed = the leading records folded when the next record's NEW key finds
 * its shard full (account.go:85): evict the group with NFAGG_REASON_FULL, then resubmit the rest. */
int nfagg_group_ingest(nfagg_group* g, const void* records, size_t n, size_t* consumed);
/* Same, records already in DEVICE memory of member `src_member`'s device (16-byte aligned, < 2^31 records). In local-fold
 * mode the chunk is folded by that member, asynchronously: the buffer must stay valid until the group synchronises
 * (nfagg_group_len, nfagg_group_evict*), as for nfagg_ingest_device.
 * THREADS: distinct source members may be fed concurrently, one host thread per source member (how N PCIe links are kept
 * busy from one process). Routed mode partitions every chunk on its source's own stream — the partitions of concurrent calls
 * overlap — and folds the buckets one call at a time (arrival order between concurrent calls = the order in which they get
 * there); local-fold mode reserves the chunk's sequence numbers and folds concurrently. Every other group call needs the
 * ingest threads to have returned. */
int nfagg_group_ingest_device(nfagg_group* g, uint32_t src_member, const void* d_records, size_t n, size_t* consumed);
/* len(c.entries) over all shards. */
int nfagg_group_len(nfagg_group* g, uint64_t* entries);
/* The per-tick collective: ncclAllReduce(sum, uint64) over each Count-Min array and ncclAllReduce(max, uint8) over each
 * HLL register array, in place on every member, on the members' streams. Afterwards every member answers
 * nfagg_hll_estimate / nfagg_cm_query / nfagg_cm_topk for the whole node. IN PLACE means: call it ONCE per window, then
 * nfagg_sketch_reset every member (nfagg_group_member) before the next window's records arrive — a second call, or the next
 * tick's call without the reset, would sum N copies of the already merged counters (Count-Min inflated N x per call). */
int nfagg_group_merge_sketches(nfagg_group* g);
/* Accounter.evict (account.go:102-124) for every shard: the members' flows back to back in `out` (HOST memory). */
int nfagg_group_evict(nfagg_group* g, int reason, void* out, size_t cap, size_t* n_out);
/* Same, shard i's flows into d_out[i] (DEVICE memory of member i's device, cap[i] records, 16-byte aligned), n_out[i] of
 * them: the input of nfagg_encode_pb_device on member i. NFAGG_TRUNCATED (nothing evicted, n_out = sizes needed) when a
 * buffer is too small. */
int nfagg_group_evict_device(nfagg_group* g, int reason, void* const* d_out, const size_t* cap, size_t* n_out);

/* ------------------------------------------------------------------ */
/* Local fold across GPUs with ONE PROCESS PER GPU (ranks of a           */
/* torch.distributed / MPI job; the in-process form is                   */
/* NFAGG_GROUP_LOCAL_FOLD above). Every rank owns an unsharded handle     */
/* (n_shards = 1) and folds the part of the ONE record stream that        */
/* arrives at it, whatever its keys — no per-record routing. Sequence     */
/* numbers must be global to the job: before folding a chunk the rank     */
/* tells the handle the arrival position of its first record              */
/* (nfagg_set_sequence). At the eviction tick a table's slots are         */
/* mergeable partials of their flows (sums, ORs, maxima, sequence-tagged  */
/* words where the earlier / later record wins):                          */
/*   1. nfagg_partials_export_device  the live flows as 192-byte          */
/*      partials grouped by owner, owner = nfagg_shard_of(key, n_shards)  */
/*   2. the caller moves segment o to rank o (RCCL all-to-all over xGMI,  */
/*      hipMemcpyPeerAsync, ...)                                          */
/*   3. nfagg_partials_merge_device   rank o merges what it received      */
/*   4. nfagg_evict_owned_device      rank o evicts the flows it owns;    */
/*      everything else in its table expires with the epoch.              */
/* The union of the ranks' evictions is bit-identical to ONE sequential   */
/* Accounter (pkg/flow/account.go:58-124) over the records folded since   */
/* the last eviction, in the order of their sequence numbers.             */
/* NFAGG_MODE_KERNEL_DEDUP (bpf/flows.c:76-143): the handle must have been  */
/* created with nfagg_config.local_fold = 1; its partials are SUB-FLOWS      */
/* (flow, interface) of NFAGG_PARTIAL_BYTES_DEDUP bytes, owned by the owner  */
/* of their FLOW; step 4 joins the sub-flows of each flow (first interface = */
/* interface of the earliest record in the job) and the union of the ranks'  */
/* evictions is bit-identical to ONE kernel-dedup table over those records.  */
/* ------------------------------------------------------------------ */
#define NFAGG_PARTIAL_BYTES 192u
#define NFAGG_PARTIAL_BYTES_DEDUP 256u
/* Bytes per partial on this handle: NFAGG_PARTIAL_BYTES, or NFAGG_PARTIAL_BYTES_DEDUP in kernel-dedup mode. */
size_t nfagg_partial_bytes(const nfagg_handle* h);
#define NFAGG_SHARD_NONE 0xFFFFFFFFu

/* The next record folded by this handle carries sequence number next_seq (epoch-relative: every eviction restarts the
 * epoch at 0; 64 bits). Must not be smaller than the number the handle has reached. Gaps are harmless: only the order
 * matters. Marks the handle as sharing its numbering with other tables (see nfagg_window_restart_device). */
int nfagg_set_sequence(nfagg_handle* h, uint64_t next_seq);

/* Step 1. d_out: DEVICE memory, 64-byte aligned, room for `cap` partials of nfagg_partial_bytes(h). Segment o (the flows shard
 * o owns) starts at partial sum(counts[0..o)) and holds counts[o] partials; counts: HOST array of n_shards (<= 64) words.
 * The flows of self_shard stay in the table and are not exported (counts[self_shard] = 0); NFAGG_SHARD_NONE exports all.
 * *n_out = partials written. NFAGG_TRUNCATED (nothing written, nothing changed, *n_out = partials needed; an upper bound
 * known in advance is nfagg_len) when cap is too small. Synchronous: the partials are complete when the call returns.
 * Afterwards the handle accepts no records (nfagg_ingest* return NFAGG_FULL) until nfagg_evict_owned_device ran: the
 * exported flows still sit in the table and would be exported twice. */
int nfagg_partials_export_device(nfagg_handle* h, uint32_t n_shards, uint32_t self_shard, void* d_out, size_t cap,
                                 uint64_t* counts, size_t* n_out);
/* Step 3. d_partials: n partials in DEVICE memory of this handle's device (16-byte aligned), all owned by shard_id of
 * n_shards (a partial of another shard fails the next synchronising call). Asynchronous on the handle's stream: the buffer
 * must stay valid until the handle synchronises. May be called several times (one call per source). The table needs room
 * for the flows it receives: size it with table_log2_slots (about 4 slots per max_entries, as the group does). */
int nfagg_partials_merge_device(nfagg_handle* h, uint32_t n_shards, uint32_t shard_id, const void* d_partials, size_t n);
/* Step 4. nfagg_evict_device restricted to the flows shard_id of n_shards owns; ends the epoch of the whole table.
 * NFAGG_TRUNCATED (nothing evicted, *n_out = records needed) when cap is too small. (Kernel-dedup mode: *n_out counts FLOWS,
 * which only the join of the sub-flows tells: call with cap = 0 first, or keep cap >= nfagg_len.) */
int nfagg_evict_owned_device(nfagg_handle* h, int reason, uint32_t n_shards, uint32_t shard_id, void* d_out, size_t cap,
                             size_t* n_out);

/* The sequence window of ranks that share one numbering. The slots carry sequence numbers relative to a 32-bit window; a
 * handle that alone holds its flows moves the window by itself when ~2^32 records of an epoch have gone by. Ranks of a
 * local-fold job cannot (the order between the ranks' partials of one flow would be lost): nfagg_ingest* fails with
 * NFAGG_ERANGE on such a handle (one that had nfagg_set_sequence) when its window is used up. Before that happens — every
 * rank knows the job's position — all ranks bring the flows together at their owners WITHOUT evicting:
 *   nfagg_partials_export_device(h, n_shards, NFAGG_SHARD_NONE, ...)   every flow, the rank's own included
 *   exchange: segment o to rank o (the own segment stays)
 *   nfagg_window_restart_device(h, n_shards, shard_id, d_partials, n, next_seq)     (NFAGG_MODE_ACCOUNTER only)
 * which empties the table (the epoch tag; nothing is written), merges the n partials this rank owns and rebases their tags;
 * the next record folded carries next_seq (>= every number used in the job so far). The epoch goes on: sketches untouched,
 * nfagg_len = the flows this rank owns. The in-process group (NFAGG_GROUP_LOCAL_FOLD) does all of this by itself. */
int nfagg_window_restart_device(nfagg_handle* h, uint32_t n_shards, uint32_t shard_id, const void* d_partials, size_t n,
                                uint64_t next_seq);

/* Testing aid: account for `records` more records in the current eviction epoch without folding any (their sequence
 * numbers are skipped), so that the moves of the 32-bit sequence window (every ~2^32 records) can be exercised without
 * feeding 600 GB. */
int nfagg_debug_skip_sequence(nfagg_handle* h, uint64_t records);
int nfagg_group_debug_skip_sequence(nfagg_group* g, uint64_t records);   /* the group's common position (local fold) / every member's */

/* Testing aid: the device and page-locked allocations of the library that are alive in this process (handles, caller tables,
 * filters, layouts, groups; not nfagg_host_alloc's buffers, which are the caller's). Every object returns to the count it
 * found when it is destroyed; a grow-only scratch buffer that grows replaces its block and leaves the count as it was. */
uint64_t nfagg_debug_live_buffers(void);

/* ---------------------------------------------------------------------- */
/* write loki on the device: streams, batches and push-request bodies      */
/* ---------------------------------------------------------------------- */
/* flowlogs-pipeline's `write loki` (pkg/pipeline/write/write_loki.go) and the batching of loki-client-go, for the flows
 * of one call: every flow's JSON line WITHOUT the keys the stage takes out of it (splitLabelsLines, :223-251) and without a
 * trailing newline (formatter "json", write_stdout.go:42-51), its timestamp (extractTimestamp, :253-277), its stream (the
 * label VALUES it carries), the batches of the client (client.go:154-172: a batch starts with an entry whatever its size and
 * is sent when bytes + len(line) > BatchSize, bytes counting line bytes only, batch.go:39-40, 63-65), and every batch as the
 * body of one logproto.PushRequest (pkg/logproto/types.go:88-144, timestamp.go:59-106):
 *   PushRequest   0x0a len Stream                                    per stream, ascending stream id
 *   Stream        0x0a len labels, then 0x12 len Entry               per entry, in arrival order (batch.go:39-54, 96-107)
 *   Entry         0x0a len Timestamp (always, even with len 0), then 0x12 len line
 *   Timestamp     0x08 seconds when not 0 (negative: a ten-byte varint), 0x10 nanos when not 0
 * Stream order in a request is Go map order in the reference; ascending stream id is one admissible order. Snappy and the
 * HTTP / gRPC send stay with the caller.
 *
 * Keys that can be named as a label or as ignored are those the line policies write through a hook: the nine SrcK8S_* and
 * nine DstK8S_* fields (the bits of NFAGG_DIM_SRC_K8S / NFAGG_DIM_DST_K8S), SrcSubnetLabel, DstSubnetLabel, FlowDirection,
 * K8S_FlowLayer (NFAGG_DIM_*), _RecordType and _HashId (below). No other key is expressible: such a stage stays on the host.
 * A key named in both masks is ignored (the ignore list is looked at first). _HashId as a LABEL is refused: it would make
 * a stream per conversation. */
#define NFAGG_LOKI_KEY_RECORD_TYPE (1u << 23)
#define NFAGG_LOKI_KEY_HASH_ID (1u << 24)
#define NFAGG_LOKI_KEY_ALL ((NFAGG_DIM_ALL & ~NFAGG_DIM_PROTO) | NFAGG_LOKI_KEY_RECORD_TYPE | NFAGG_LOKI_KEY_HASH_ID)
#define NFAGG_LOKI_TS_NOW 0u                 /* TimestampLabel "": timeNow() */
#define NFAGG_LOKI_TS_TIME_FLOW_END_MS 1u
#define NFAGG_LOKI_TS_TIME_FLOW_START_MS 2u
#define NFAGG_LOKI_MAX_STREAMS (1u << 20)
#define NFAGG_LOKI_LABELS_MAX 4096u          /* one stream's LabelSet.String() */

typedef struct {
    uint32_t struct_size;
    uint32_t label_keys;                     /* NFAGG_DIM_* / NFAGG_LOKI_KEY_*: keys that become labels */
    uint32_t ignore_keys;                    /* keys of the ignore list */
    uint32_t timestamp_source;               /* NFAGG_LOKI_TS_* */
    double timestamp_scale;                  /* float64(time.ParseDuration(TimestampScale)): 1e6 for "1ms" */
    uint32_t batch_size;                     /* 1 .. 2^31 - 1 */
    uint32_t pad_;
} nfagg_loki_spec;

/* A stream of a plan: what tells its label values. A class is that of nfagg_loki_class_row (0: the side has no row, or no
 * label field of the row is present); a label is the net table's label index (0xFFFF: none, or the key is no label);
 * direction 0..2 (255: none); layer 0 none, 1 infra, 2 app; record_type 1: "flowLog". first_flow: the first flow of the
 * call that belongs to it; stream ids ascend with it. */
typedef struct {
    uint32_t src_class, dst_class;
    uint16_t src_label, dst_label;
    uint8_t direction, layer, record_type, pad_;
    uint32_t first_flow;
} nfagg_loki_stream;

/* One (batch, stream) of a plan, ascending by batch, then stream. entry_bytes: the stream's framed entries (every 0x12 len
 * Entry), what a Stream holds behind its labels. */
typedef struct {
    uint32_t batch, stream, n_entries, pad_;
    uint64_t entry_bytes;
} nfagg_loki_group;

typedef struct { uint32_t n_streams, n_groups, n_batches, n_deferred; } nfagg_loki_counts;

typedef struct nfagg_loki_table nfagg_loki_table;

/* Over the rows of k8s_table (kept alive by the caller): (a) both sides' rendered blocks once more with the label and the
 * ignored keys left out, in the shape of the table's own; (b) one class per row and side over the LABEL fields, by
 * nfagg_metrics_table_create's (text, presence) rule with one addition: a field whose text is not valid UTF-8 counts as
 * absent, and is left out of the line as well (write_loki.go:240-243). Subnet labels of net_table with equal text share a
 * stream; one whose text is not valid UTF-8 is dropped likewise. NFAGG_EINVAL: a spec with unknown bits, _HashId as a label,
 * an unknown timestamp source, a scale that is not finite and positive, batch_size outside 1 .. 2^31 - 1. h == NULL builds and
 * checks on the host alone (tables built with h == NULL; errors through nfagg_last_error(NULL)); the plan refuses such a table. */
int nfagg_loki_table_create(nfagg_handle* h, const nfagg_k8s_table* k8s_table, const nfagg_net_table* net_table,
                            const nfagg_loki_spec* spec, nfagg_loki_table** table);
void nfagg_loki_table_destroy(nfagg_loki_table* table);
/* Classes of a side (0 src, 1 dst), numbered from 1, and the first row of a class: its label fields are the class's values. */
uint32_t nfagg_loki_n_classes(const nfagg_loki_table* table, int side);
int nfagg_loki_class_row(const nfagg_loki_table* table, int side, uint32_t cls, uint32_t* row);
/* One side's block of row `row` as the lines of this table carry it. */
int nfagg_loki_render(const nfagg_loki_table* table, int side, uint32_t row, void* out, size_t cap, size_t* n_out);

/* The plan of one call. Arguments as nfagg_encode_flp_json_conn takes them, then the table and timeNow(). hash_ids NULL: no
 * conntrack stage in front, every flow has a line and neither _RecordType nor _HashId; otherwise a flow the stage does not
 * track has no line and takes part in nothing. All three line policies are served: features NULL the plain line, features
 * the parts of full flow contents, rows and netev_table (both or neither; they need features) their network events.
 * A flow whose timestamp product leaves int64, or whose time lies outside [year 1, year 10000) (validateTimestamp), is
 * DEFERRED: deferred[i] = 1, and it is kept out of every batch and every cut; the caller formats it. (The reference would
 * lose the whole batch.)
 * Stream ids are dense, in order of each stream's first flow. Batches are cut over the flows in order, from an empty batch.
 * streams / groups: room for stream_cap / group_cap; with more, NFAGG_TRUNCATED, counts hold what is needed and nothing is
 * written to streams and groups (stream_cap at most NFAGG_LOKI_MAX_STREAMS). deferred: n bytes, or NULL; it is written whatever
 * the return code. The handle keeps the plan, and the
 * records and tables must stay as they are, until nfagg_loki_write ran or the next plan. All pointers HOST memory: */
int nfagg_loki_plan(nfagg_handle* h, const void* records, size_t n, const nfagg_pb_features* features,
                    const uint16_t* rows, const nfagg_netev_table* netev_table, const nfagg_tls_names* tls_names,
                    const nfagg_k8s_table* k8s_table, const nfagg_net_table* net_table, const uint64_t* hash_ids,
                    const nfagg_flp_options* opt, const nfagg_loki_table* table, int64_t now_unix_ns,
                    nfagg_loki_stream* streams, uint32_t stream_cap, nfagg_loki_group* groups, uint32_t group_cap,
                    uint8_t* deferred, nfagg_loki_counts* counts);
/* Same with d_records, d_hash_ids, d_streams, d_groups and d_deferred in DEVICE memory (records 16-byte, the others 8-byte
 * aligned, d_rows and the arrays inside d_features as the *_conn_device encoder takes them); counts stays on the host. */
int nfagg_loki_plan_device(nfagg_handle* h, const void* d_records, size_t n, const nfagg_pb_features* d_features,
                           const uint16_t* d_rows, const nfagg_netev_table* netev_table, const nfagg_tls_names* tls_names,
                           const nfagg_k8s_table* k8s_table, const nfagg_net_table* net_table, const uint64_t* d_hash_ids,
                           const nfagg_flp_options* opt, const nfagg_loki_table* table, int64_t now_unix_ns,
                           nfagg_loki_stream* d_streams, uint32_t stream_cap, nfagg_loki_group* d_groups, uint32_t group_cap,
                           uint8_t* d_deferred, nfagg_loki_counts* counts);
/* The bodies of the handle's plan, back to back. labels: every stream's LabelSet.String() (labelset_string.go:23-43), stream
 * s at labels[label_offsets[s] .. label_offsets[s + 1]), each 2 .. NFAGG_LOKI_LABELS_MAX bytes; the caller renders it once per
 * stream. batch_offsets: n_batches + 1 values, batch_entries: n_batches. NFAGG_TRUNCATED with *out_bytes = bytes needed when
 * out_cap is smaller or out is NULL (offsets and entries are written all the same); NFAGG_EINVAL without a plan, or with a
 * plan that was truncated; NFAGG_ERANGE when the label texts come to 2^32 bytes or more. All pointers HOST memory: */
int nfagg_loki_write(nfagg_handle* h, const void* labels, const uint64_t* label_offsets, void* out, size_t out_cap,
                     uint64_t* batch_offsets, uint32_t* batch_entries, size_t* out_bytes);
/* Same with d_out (16-byte aligned), d_batch_offsets and d_batch_entries in DEVICE memory; the label text stays on the host. */
int nfagg_loki_write_device(nfagg_handle* h, const void* labels, const uint64_t* label_offsets, void* d_out, size_t out_cap,
                            uint64_t* d_batch_offsets, uint32_t* d_batch_entries, size_t* out_bytes);
/* The longest framed entry (0x12 len Entry) a flow can take: nfagg_flp_json_conn_max_line(policy) - 1 (no newline) plus 27
 * bytes of framing; 0 for an unknown policy. */
uint32_t nfagg_loki_max_entry(int policy);

/* ------------------------------------------------------------------ */
/* write ipfix on the device — flowlogs-pipeline's `write ipfix` stage  */
/* (pkg/pipeline/write/write_ipfix.go) behind a direct-FLP pipeline:    */
/* the ENRICHED flow as one IPFIX message per flow, as go-ipfix's       */
/* exporter sends it (exporter/msg.go, entities/set.go, entities/ie.go  */
/* 624-713). This is not nfagg_encode_ipfix, which restates the agent's */
/* own exporter (two fixed 19-field templates, no state).               */
/*                                                                      */
/* Input: decode.RecordToMap (decode_protobuf.go:57-192) of the flow    */
/* plus SrcK8S_* / DstK8S_* as nfagg_k8s_render defines their presence; */
/* only Namespace, Name and HostName are read on each side.             */
/* Template v6 iff Etype == 0x86DD, anything else (non-IP too) v4.      */
/* Templates (prepareTemplate): v4 = sourceIPv4Address,                 */
/* destinationIPv4Address, icmpTypeIPv4, icmpCodeIPv4,                  */
/* postNATSourceIPv4Address, postNATDestinationIPv4Address + the 17     */
/* common fields; v6 = sourceIPv6Address, destinationIPv6Address,       */
/* nextHeaderIPv6, icmpTypeIPv6, icmpCodeIPv6, the two postNAT*IPv6 +   */
/* the 17. Common: ethernetType flowDirection sourceMacAddress          */
/* destinationMacAddress protocolIdentifier sourceTransportPort         */
/* destinationTransportPort octetDeltaCount flowStartMilliseconds       */
/* flowEndMilliseconds packetDeltaCount interfaceName tcpControlBits    */
/* postNAPTSourceTransportPort postNAPTDestinationTransportPort         */
/* selectorAlgorithm samplingProbability. With enterprise_id != 0 nine  */
/* enterprise elements follow: sourcePodNamespace 7733 sourcePodName    */
/* 7734 destinationPodNamespace 7735 destinationPodName 7736            */
/* sourceNodeName 7737 destinationNodeName 7738 (strings),              */
/* timeFlowRttNs 7740 (unsigned64), interfaces 7741, directions 7742    */
/* (strings). Ids, types and lengths of the IANA names:                 */
/* registry/registry_IANA.go.                                           */
/*                                                                      */
/* The writer is STATEFUL: createDataRecord mutates one element list    */
/* per family, and a key that is absent from a flow's map and has no    */
/* Default leaves the value the last flow of that family set. Carried   */
/* that way: Bytes, Packets, Sampling (selectorAlgorithm and            */
/* samplingProbability), SrcAddr / DstAddr / Proto, IcmpType /          */
/* IcmpCode, SrcPort / DstPort, Flags, XlatSrcPort, XlatDstPort,        */
/* TimeFlowRttNs and the six Kubernetes strings, each on its own. The   */
/* postNAT*Address elements are not carried (Default: the zero          */
/* address); Interfaces and IfDirections are never empty for a          */
/* model.Record (record.go:104), so they are set by every flow.         */
/* A record FAILS and is not sent (status 1) when an Ipv4Address        */
/* element's value has no To4(): the initial nil before the first IP    */
/* flow of the v4 family, an address under a v4 Etype that is not       */
/* v4-mapped, a non-mapped XlatSrcAddr / XlatDstAddr in the v4          */
/* template; (status 2) when 16 + set length > max_msg_size. The        */
/* setters ran before the failure: the state has moved. The sequence    */
/* number counts sent data records only.                                */
/* Flags: the raw uint16, or with flags_decoded (decode_tcp_flags in    */
/* front) EncodeTCPFlags(DecodeTCPFlags(x)) = x & 0x7FF                 */
/* (utils/tcp_flags.go). samplingProbability: 1.0 / float64(interval),  */
/* correctly rounded, big-endian.                                       */
/*                                                                      */
/* The bytes are pinned to a restatement of the Go source               */
/* (tests/flp_ipfix_ref.py), not to a Go run.                           */
/* Differences from the reference, by design: one Export Time per call; */
/* one strings table per call; the template refresh timer is the        */
/* caller's and runs between calls; the conversation records of extract */
/* conntrack are out of scope (flow logs only); a string value has at   */
/* most NFAGG_FLP_IPFIX_MAX_STRING bytes, the table is refused beyond   */
/* (go-ipfix's own limit is 65535).                                     */
/* ------------------------------------------------------------------ */

#define NFAGG_FLP_IPFIX_MAX_STRING 1024
#define NFAGG_FLP_IPFIX_SENT 0          /* status values */
#define NFAGG_FLP_IPFIX_FAIL_FAMILY 1
#define NFAGG_FLP_IPFIX_FAIL_SIZE 2

typedef struct nfagg_flp_ipfix_options {
    uint32_t struct_size;        /* sizeof(nfagg_flp_ipfix_options)                               */
    uint32_t n_names;
    int64_t  now_unix_ns;        /* as nfagg_flp_options                                          */
    uint64_t mono_now_ns;
    const nfagg_intf_name* names;/* HOST memory: same table and lookup rule (the UDN is not used) */
    char     unknown_name[16];
    uint8_t  unknown_len;
    uint8_t  flags_decoded;      /* non-zero: decode_tcp_flags ran in front of the writer          */
    uint8_t  pad_[2];
    uint32_t export_time_s;      /* Export Time of every message of the call                      */
    uint32_t seq0;               /* the exporter's seqNumber at the start of the call             */
    uint32_t obs_domain_id;      /* 1 (write_ipfix.go:598)                                        */
    uint16_t template_id_v4;     /* 256 (NewTemplateID starts at 255)                             */
    uint16_t template_id_v6;     /* 257                                                           */
    uint32_t enterprise_id;      /* 0: no enterprise elements in either template                  */
    uint32_t max_msg_size;       /* 512 for UDP without PMTU, 65535 for TCP (exporter/process.go:121-158); at most 65535 */
} nfagg_flp_ipfix_options;

/* The element values of one family as plain values. *_set == 0: the element is still the nil NewWriteIpfix created it with.
 * str: interfaceName, sourcePodNamespace, sourcePodName, destinationPodNamespace, destinationPodName, sourceNodeName,
 * destinationNodeName, interfaces, directions. */
#define NFAGG_FLP_IPFIX_N_STRINGS 9
typedef struct nfagg_flp_ipfix_elements {
    uint32_t struct_size;
    uint8_t  addr_set, xlat_set, mac_set, pad0_;
    uint8_t  src_addr[16], dst_addr[16], xlat_src_addr[16], xlat_dst_addr[16];   /* net.IP.To16() */
    uint8_t  src_mac[6], dst_mac[6];
    uint8_t  proto, icmp_type, icmp_code, flow_direction;
    uint16_t etype, src_port, dst_port, flags, xlat_src_port, xlat_dst_port, selector_algorithm, pad1_;
    uint64_t bytes, packets, start_ms, end_ms, rtt_ns;
    double   sampling_probability;
    uint32_t str_len[NFAGG_FLP_IPFIX_N_STRINGS];
    uint32_t pad3_[5];           /* str at 208: 16-byte aligned */
    char     str[NFAGG_FLP_IPFIX_N_STRINGS][NFAGG_FLP_IPFIX_MAX_STRING];
} nfagg_flp_ipfix_elements;     /* 9424 bytes */

typedef struct nfagg_flp_ipfix_strings nfagg_flp_ipfix_strings;
typedef struct nfagg_flp_ipfix_writer nfagg_flp_ipfix_writer;

/* The template message NewWriteIpfix sends for a family (v6 == 0: v4): header (Export Time export_time_s, Sequence Number
 * seq0, a template does not advance it), one template set (ID 2), the 23 / 24 IANA field specifiers and, with enterprise_id
 * != 0, the nine enterprise ones (enterprise bit, then the 4-byte enterprise number); variable-length elements carry 65535.
 * Host only. NFAGG_TRUNCATED with *n_out = bytes needed when cap is smaller (nothing written). */
int nfagg_flp_ipfix_template(const nfagg_flp_ipfix_options* opt, int v6, void* out, size_t cap, size_t* n_out);

/* The three strings the writer reads of every row of a Kubernetes table, from the same entries (row r = entries[r], so the
 * rows of nfagg_k8s_resolve index it), with their presence as nfagg_k8s_render has it (Name always, Namespace when not empty,
 * HostName when HostIP and HostName are both not empty). The bytes are kept as they go on the wire, each string 16-byte
 * aligned; its length prefix (one byte below 255 bytes, else 0xFF and two bytes) follows from the length. NFAGG_EINVAL: a string of more than NFAGG_FLP_IPFIX_MAX_STRING bytes, a null string with a length, more than
 * NFAGG_K8S_MAX_ROWS entries. h == NULL builds and checks on the host alone (errors through nfagg_last_error(NULL)); the write
 * refuses such a table. */
int nfagg_flp_ipfix_strings_create(nfagg_handle* h, const nfagg_k8s_entry* entries, size_t n, nfagg_flp_ipfix_strings** strings);
void nfagg_flp_ipfix_strings_destroy(nfagg_flp_ipfix_strings* strings);

/* The element state of both families on the handle's device, as NewWriteIpfix leaves it. String values are owned bytes: the
 * strings table may be destroyed or rebuilt between calls. */
int nfagg_flp_ipfix_writer_create(nfagg_handle* h, nfagg_flp_ipfix_writer** writer);
void nfagg_flp_ipfix_writer_destroy(nfagg_flp_ipfix_writer* writer);
int nfagg_flp_ipfix_writer_get(nfagg_flp_ipfix_writer* writer, int v6, nfagg_flp_ipfix_elements* out);
int nfagg_flp_ipfix_writer_reset(nfagg_flp_ipfix_writer* writer);

/* Write n flows in order. features NULL: records that carry only BpfFlowMetrics (no xlat, no RTT); k8s_rows NULL: no address
 * resolved, else 2 x n rows as nfagg_k8s_resolve writes them, indexing `strings` (required then). Message i =
 * out[msg_offsets[i], msg_offsets[i + 1]), empty for a failed flow; msg_offsets[n] = *out_bytes; status[i] one of
 * NFAGG_FLP_IPFIX_*; message i carries seq0 + the number of sent flows before i; *n_sent their count. NFAGG_TRUNCATED with
 * *out_bytes = bytes needed (and *n_sent) when out_cap is smaller or out is NULL: nothing is written and the writer's state
 * stays as it was. The state advances only with a call that wrote. All pointers HOST memory: */
int nfagg_flp_ipfix_write(nfagg_handle* h, nfagg_flp_ipfix_writer* writer, const void* records, size_t n,
                          const nfagg_pb_features* features, const uint32_t* k8s_rows, const nfagg_flp_ipfix_strings* strings,
                          const nfagg_flp_ipfix_options* opt, void* out, size_t out_cap, uint64_t* msg_offsets, uint8_t* status,
                          size_t* n_sent, size_t* out_bytes);
/* Same with d_records, the arrays inside d_features, d_k8s_rows, d_out, d_msg_offsets and d_status in DEVICE memory (records
 * and output 16-byte, rows and offsets 8-byte aligned). */
int nfagg_flp_ipfix_write_device(nfagg_handle* h, nfagg_flp_ipfix_writer* writer, const void* d_records, size_t n,
                                 const nfagg_pb_features* d_features, const uint32_t* d_k8s_rows,
                                 const nfagg_flp_ipfix_strings* strings, const nfagg_flp_ipfix_options* opt, void* d_out,
                                 size_t out_cap, uint64_t* d_msg_offsets, uint8_t* d_status, size_t* n_sent, size_t* out_bytes);

/* ------------------------------------------------------------------ */
/* extract timebased — flowlogs-pipeline's windowed GROUP BY and top-K  */
/* (pkg/pipeline/extract/extract_timebased.go:35-59,                    */
/* extract/timebased/{timebased,tables,filters,heap}.go,                */
/* api/extract_timebased.go). The reference keeps, per index-key table  */
/* and key, a list of (stamp, flow map) and walks every entry of every  */
/* list for every rule of every call. Every entry of one call carries   */
/* the call's one `now`, so a window is a union of whole calls: here a  */
/* table is a persistent hash table of keys in device memory, a call    */
/* leaves one compact SLICE of per-key partials stamped `now`, a rule   */
/* merges the slices inside its window into one accumulator per key,    */
/* and a float64 selection takes the K best.                            */
/*                                                                      */
/* Differences from the reference, by design:                           */
/*  - a flow that enters a table but lacks the operation key of one of  */
/*    that table's rules makes the reference panic (ConvertToFloat64 of */
/*    a missing key, utils/convert.go:56-59): such a call is refused    */
/*    with NFAGG_EDEFER and changes nothing;                            */
/*  - the keys of a table are capped (options.max_keys); the reference  */
/*    never forgets a key and has no cap. One key more than the cap     */
/*    fails the object until nfagg_timebased_reset;                     */
/*  - partials are integers. A sum below 2^53 of values that are not    */
/*    negative equals the reference's float sum in any order; otherwise */
/*    the value is the correctly rounded float64 of the exact integer   */
/*    total and the result carries NFAGG_TB_INEXACT, because the        */
/*    reference's own value then depends on its order of summation;     */
/*  - ties at the K-th place are broken arbitrarily, as Go's map order  */
/*    breaks them.                                                      */
/* ------------------------------------------------------------------ */
#define NFAGG_TB_MAX_TABLES 4           /* distinct index-key lists */
#define NFAGG_TB_MAX_RULES 16
#define NFAGG_TB_MAX_COLUMNS 4          /* index keys of one rule; together at most 40 bytes (an address: 16, anything else: 4) */
#define NFAGG_TB_MAX_VALUES 4           /* distinct value sources of the rules of one table */
#define NFAGG_TB_MAX_KEYS (1u << 24)    /* options.max_keys per table; a table has the power of two >= 2 * max_keys slots, at least 1024 */
#define NFAGG_TB_MAX_TOPK 4096
#define NFAGG_TB_MAX_SLICES 1024        /* calls with flows inside a table's largest window */

#define NFAGG_TB_OP_SUM 1
#define NFAGG_TB_OP_AVG 2
#define NFAGG_TB_OP_MIN 3
#define NFAGG_TB_OP_MAX 4
#define NFAGG_TB_OP_COUNT 5
#define NFAGG_TB_OP_LAST 6
#define NFAGG_TB_OP_DIFF 7

#define NFAGG_TB_INEXACT 1u             /* nfagg_tb_result.flags: the value is the rounded exact total; the reference's depends on its order */

/* One rule of api.TimebasedFilterRule. index_keys: the names of the rule's indexKeys (or its one indexKey), the keys RecordToMap
 * and the transforms write, with their presence rules:
 *   SrcAddr, DstAddr                     the 16 address bytes; present with eth_protocol 0x0800 / 0x86DD
 *   SrcPort, DstPort                     present with IP and transport_protocol 6 / 17 / 132
 *   Proto                                present with IP
 *   SrcK8S_<f>, DstK8S_<f>               one field of the flow's Kubernetes row, f one of Namespace, Name, Type, OwnerName,
 *                                        OwnerType, NetworkName, HostIP, HostName, Zone, as a CLASS: the dense id of the field's
 *                                        (text, presence) by nfagg_k8s_render's rules, what nfagg_metrics_table_create computes
 *                                        for that one bit; present when the row has the field and its text is not empty
 *   SrcSubnetLabel, DstSubnetLabel       the net row's label index; present when there is one and its text is not empty
 *   FlowDirection                        the net row's direction; present unless NFAGG_NET_NO_DIRECTION
 * A flow enters a rule's table only if every index key is present. Rules with equal key lists share a table. value: the
 * operation key as one of NFAGG_MET_VALUE_* 1..6, with the presence rules stated there; every operation reads it, `count` too
 * (filters.go:86-91). interval_ns: the rule's timeInterval; an entry stamped exactly `now - interval_ns` is inside the window. */
typedef struct nfagg_tb_rule {
    uint32_t struct_size;               /* sizeof(nfagg_tb_rule) */
    uint32_t n_index_keys;              /* 1..NFAGG_TB_MAX_COLUMNS */
    const char* index_keys[NFAGG_TB_MAX_COLUMNS];   /* NUL-terminated */
    uint32_t operation;                 /* NFAGG_TB_OP_* */
    uint32_t value;                     /* NFAGG_MET_VALUE_* 1..6 */
    uint32_t top_k;                     /* 0: every key, in unspecified order; else at most NFAGG_TB_MAX_TOPK */
    uint32_t reversed;                  /* 0: the K largest, descending; 1: the K smallest, ascending */
    int64_t interval_ns;                /* >= 0 */
} nfagg_tb_rule;

typedef struct nfagg_tb_options {
    uint32_t struct_size;               /* sizeof(nfagg_tb_options) */
    uint32_t max_keys;                  /* per table, 1..NFAGG_TB_MAX_KEYS */
} nfagg_tb_options;

typedef struct nfagg_tb_result {
    uint32_t key;                       /* the key's dense id in its table, in order of first claim: nfagg_timebased_keys reads it back */
    uint32_t flags;                     /* NFAGG_TB_INEXACT */
    double value;
} nfagg_tb_result;

/* One key's columns, in the order of its table's index keys: the 16 address bytes, or a 32-bit value in the first four bytes
 * (little endian: a port, the protocol, a class, a label index, the direction) and zeroes. */
typedef struct nfagg_tb_key {
    uint8_t col[NFAGG_TB_MAX_COLUMNS][16];
} nfagg_tb_key;

typedef struct nfagg_tb_stats {
    uint32_t n_tables, n_rules;
    uint32_t keys[NFAGG_TB_MAX_TABLES];         /* distinct keys so far */
    uint32_t slots[NFAGG_TB_MAX_TABLES];        /* of the table's hash table */
    uint32_t slices[NFAGG_TB_MAX_TABLES];       /* live slices */
    uint32_t table_of_rule[NFAGG_TB_MAX_RULES];
    uint64_t bytes_held;                        /* device memory of the tables, the slices and the evaluation scratch */
    int64_t last_now_ns;
    uint32_t failed, has_clock;
} nfagg_tb_stats;

typedef struct nfagg_timebased nfagg_timebased;

/* Build the rule set: n_rules 1..NFAGG_TB_MAX_RULES. k8s_table / net_table: required when a rule names a Kubernetes key / a
 * subnet label (else may be NULL), must be of the same handle and outlive the object. NFAGG_EINVAL, with a message that names
 * the rule and the offender: a key name outside the list above, a selected Kubernetes or label text that contains ',' (the
 * reference joins a key's values by ',' and splits the result again), a key list wider than 40 bytes, an unknown operation or
 * value source, top_k over NFAGG_TB_MAX_TOPK, a negative interval, more than NFAGG_TB_MAX_TABLES distinct key lists or
 * NFAGG_TB_MAX_VALUES value sources in one table, max_keys out of range, a wrong struct_size. h == NULL builds and checks on the
 * host alone (errors through nfagg_last_error(NULL)); extract refuses such an object. */
int nfagg_timebased_rules_create(nfagg_handle* h, const nfagg_k8s_table* k8s_table, const nfagg_net_table* net_table, const nfagg_tb_rule* rules,
                                 uint32_t n_rules, const nfagg_tb_options* options, nfagg_timebased** tb);
void nfagg_timebased_destroy(nfagg_timebased* tb);

/* Extract(entries) at `now_ns`: the flows enter their tables as one slice stamped now_ns, every rule is evaluated, and slices
 * older than their table's largest interval are freed. records, features (as nfagg_metrics_fold_content takes them; NULL: no flow
 * has a part), k8s_rows and net_rows (as the resolves wrote them; NULL when no rule reads them, else NFAGG_EINVAL) describe the n
 * flows. result_cap, out, n_out: arrays of n_rules. out[r] receives rule r's results in the reference's order (sorted for top_k
 * > 0, any order for 0); n_out[r] is exact always.
 *   NFAGG_EDEFER     some entering flow lacks a value source of its table; *n_missing = their number; NOTHING has changed (no
 *                    key, no slice, no clock). Drop them (nfagg_filter_apply with a presence query, nfagg_gather) and repeat.
 *   NFAGG_TRUNCATED  (a) some result_cap[r] < n_out[r]: nothing is written to any out[r], but the window state HAS advanced:
 *                    repeat with nfagg_timebased_results, not with this call. (b) a table met more distinct keys than max_keys:
 *                    n_out is all zero, the object has failed and every later call returns NFAGG_EINVAL until
 *                    nfagg_timebased_reset (nfagg_timebased_stats tells the two apart).
 *   NFAGG_EINVAL     now_ns below the previous call's; a failed object; arguments.
 *   NFAGG_ERANGE     n above 2^32 - 2; a table holds NFAGG_TB_MAX_SLICES slices that are still inside its largest window at now_ns (nothing has changed).
 * n == 0 is a valid call: time passes, windows shrink and the trim runs. All pointers HOST memory: */
int nfagg_timebased_extract(nfagg_handle* h, nfagg_timebased* tb, const void* records, size_t n, const nfagg_pb_features* features,
                            const uint32_t* k8s_rows, const nfagg_net_row* net_rows, int64_t now_ns, const uint32_t* result_cap,
                            nfagg_tb_result* const* out, uint32_t* n_out, uint64_t* n_missing);
/* Same with d_records, the arrays inside d_features, d_k8s_rows, d_net_rows and every d_out[r] in DEVICE memory (records and
 * results 16-byte, rows 8-byte aligned); result_cap, the array d_out itself, n_out and n_missing are host memory. */
int nfagg_timebased_extract_device(nfagg_handle* h, nfagg_timebased* tb, const void* d_records, size_t n, const nfagg_pb_features* d_features,
                                   const uint32_t* d_k8s_rows, const nfagg_net_row* d_net_rows, int64_t now_ns, const uint32_t* result_cap,
                                   nfagg_tb_result* const* d_out, uint32_t* n_out, uint64_t* n_missing);
/* Evaluate the rules again at the last call's now_ns, without adding a slice: what a caller does after NFAGG_TRUNCATED (a).
 * NFAGG_ESTATE before the first extract. */
int nfagg_timebased_results(nfagg_handle* h, nfagg_timebased* tb, const uint32_t* result_cap, nfagg_tb_result* const* out, uint32_t* n_out);
int nfagg_timebased_results_device(nfagg_handle* h, nfagg_timebased* tb, const uint32_t* result_cap, nfagg_tb_result* const* d_out, uint32_t* n_out);

/* The columns of n keys of table `table` (nfagg_tb_stats.table_of_rule) by their ids. The host renders them with what it has:
 * net.IP.String() for an address, decimal for a port, the protocol and the direction, nfagg_timebased_class_row and the
 * Kubernetes entries for a class, the label list for a label index. NFAGG_EINVAL for an id that no key has. */
int nfagg_timebased_keys(nfagg_timebased* tb, uint32_t table, const uint32_t* keys, size_t n, nfagg_tb_key* out);
/* The first row of the Kubernetes table whose field has class `cls` in column `column` of table `table` (a Kubernetes column). */
int nfagg_timebased_class_row(const nfagg_timebased* tb, uint32_t table, uint32_t column, uint32_t cls, uint32_t* row);
/* The hash that places a key in its table: the slot of first probe is hash & (slots - 1), probing is linear. Pure CPU; 0 for
 * arguments out of range. For tests that craft collisions. */
uint64_t nfagg_timebased_key_hash(const nfagg_timebased* tb, uint32_t table, const nfagg_tb_key* key);
/* Forget every key, slice and the clock; a failed object works again. */
int nfagg_timebased_reset(nfagg_timebased* tb);
int nfagg_timebased_stats(const nfagg_timebased* tb, nfagg_tb_stats* out);

#ifdef __cplusplus
}
#endif
#endif /* NFAGG_H */
