"""ctypes binding of libnfagg.so (include/nfagg.h). There is no fallback: if the
HIP library has not been built, importing this module raises."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# NFAGG_LIB: tools/phase_timing.py points this at lib/libnfagg_diag.so (the -DNFAGG_DIAG build with the phase-timing kernels)
LIB_PATH = os.environ.get("NFAGG_LIB") or os.path.join(_HERE, "lib", "libnfagg.so")
SYNTH_PATH = os.path.join(_HERE, "lib", "libnfagg_synth.so")

if not os.path.exists(LIB_PATH):
    raise ImportError(
        f"{LIB_PATH} is missing: build it with `make -C {os.path.join(_HERE, 'csrc')}` "
        "(or __graft_entry__.build()). libnfagg has no CPU/Python fallback.")

# PyTorch-ROCm bundles its own libamdhip64.so (same soname as /opt/rocm's). A
# process must use ONE HIP runtime: when torch is installed, let it load first so
# libnfagg.so binds to the runtime torch's tensors, streams and RCCL live in.
# (A Go/C host without torch simply gets /opt/rocm's runtime.)
try:
    import torch  # noqa: F401
except Exception:   # torch is optional plumbing, not a dependency of the library
    torch = None

lib = C.CDLL(LIB_PATH)

OK, FULL, TRUNCATED, EDEFER = 0, 1, 2, 3
EINVAL, ENODEV, ENOMEM, EDEVICE, ESTATE, ERANGE = -1, -2, -3, -4, -5, -6
REASON_TIMEOUT, REASON_FULL, REASON_CLOSING = 0, 1, 2
REASON_NAMES = {0: "timeout", 1: "full", 2: "closing"}
MODE_ACCOUNTER, MODE_KERNEL_DEDUP = 0, 1
GROUP_LOCAL_FOLD = 1
PARTIAL_BYTES = 192
PARTIAL_BYTES_DEDUP = 256
SHARD_NONE = 0xFFFFFFFF
SKETCH_CM, SKETCH_HLL = 1, 2
CM_SRC, CM_DST, HLL_SRC, HLL_DST = 0, 1, 2, 3


class Config(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("device", C.c_int32), ("max_entries", C.c_uint64),
        ("table_log2_slots", C.c_uint32), ("mode", C.c_uint32), ("sketch_flags", C.c_uint32),
        ("cm_depth", C.c_uint32), ("cm_log2_width", C.c_uint32), ("hll_p", C.c_uint32),
        ("staging_records", C.c_uint64), ("n_shards", C.c_uint32), ("shard_id", C.c_uint32),
        ("profile", C.c_uint32), ("ingest_variant", C.c_uint32), ("ext_sketch", C.c_void_p * 4),
        ("copy_threads", C.c_uint32), ("group_flags", C.c_uint32), ("local_fold", C.c_uint32),
    ]


class RingBuf(C.Structure):
    """nfagg_ringbuf (include/nfagg.h)."""
    _fields_ = [("data", C.c_void_p), ("mask", C.c_uint64), ("producer_pos", C.c_void_p), ("consumer_pos", C.c_void_p)]


class PbOptions(C.Structure):
    """nfagg_pb_options (include/nfagg.h)."""
    _fields_ = [
        ("struct_size", C.c_uint32), ("n_names", C.c_uint32), ("now_unix_ns", C.c_int64), ("mono_now_ns", C.c_uint64),
        ("agent_ip", C.c_uint8 * 16), ("names", C.c_void_p), ("unknown_name", C.c_char * 16), ("unknown_len", C.c_uint8),
        ("pad_", C.c_uint8 * 7),
    ]


class IpfixOptions(C.Structure):
    """nfagg_ipfix_options (include/nfagg.h)."""
    _fields_ = [
        ("struct_size", C.c_uint32), ("n_names", C.c_uint32), ("now_unix_ns", C.c_int64), ("mono_now_ns", C.c_uint64),
        ("names", C.c_void_p), ("unknown_name", C.c_char * 16), ("unknown_len", C.c_uint8), ("pad_", C.c_uint8 * 3),
        ("export_time_s", C.c_uint32), ("seq0", C.c_uint32), ("obs_domain_id", C.c_uint32),
        ("template_id_v4", C.c_uint16), ("template_id_v6", C.c_uint16),
    ]


class FlpOptions(C.Structure):
    """nfagg_flp_options (include/nfagg.h)."""
    _fields_ = [
        ("struct_size", C.c_uint32), ("n_names", C.c_uint32), ("now_unix_ns", C.c_int64), ("mono_now_ns", C.c_uint64),
        ("names", C.c_void_p), ("unknown_name", C.c_char * 16), ("unknown_len", C.c_uint8), ("agent_ip_nil", C.c_uint8),
        ("pad_", C.c_uint8 * 6), ("agent_ip", C.c_uint8 * 16), ("time_received_s", C.c_int64),
    ]


class MapView(C.Structure):
    """nfagg_map_view (include/nfagg.h)."""
    _fields_ = [("ids", C.c_void_p), ("values", C.c_void_p), ("n", C.c_size_t)]


class MergedFlows(C.Structure):
    """nfagg_merged_flows (include/nfagg.h)."""
    _fields_ = [("records", C.c_void_p), ("present", C.c_void_p), ("additional", C.c_void_p), ("dns", C.c_void_p),
                ("drops", C.c_void_p), ("network_events", C.c_void_p), ("xlat", C.c_void_p), ("quic", C.c_void_p)]


class PbFeatures(C.Structure):
    """nfagg_pb_features (include/nfagg.h)."""
    _fields_ = [("struct_size", C.c_uint32), ("reserved_", C.c_uint32), ("present", C.c_void_p), ("additional", C.c_void_p),
                ("dns", C.c_void_p), ("drops", C.c_void_p), ("xlat", C.c_void_p), ("quic", C.c_void_p)]


class NetevEntry(C.Structure):
    """nfagg_netev_entry (include/nfagg.h)."""
    _fields_ = [("cookie", C.c_uint8 * 8), ("kind", C.c_uint32), ("reserved_", C.c_uint32),
                ("action", C.c_char_p), ("actor", C.c_char_p), ("name", C.c_char_p), ("namespace_", C.c_char_p),
                ("direction", C.c_char_p), ("string", C.c_char_p),
                ("action_len", C.c_uint32), ("actor_len", C.c_uint32), ("name_len", C.c_uint32), ("namespace_len", C.c_uint32),
                ("direction_len", C.c_uint32), ("string_len", C.c_uint32)]


class TlsNameEntry(C.Structure):
    """nfagg_tls_name_entry (include/nfagg.h)."""
    _fields_ = [("kind", C.c_uint16), ("id", C.c_uint16), ("name_len", C.c_uint32), ("name", C.c_char_p)]


class K8sEntry(C.Structure):
    """nfagg_k8s_entry (include/nfagg.h)."""
    _STRINGS = ("namespace_", "name", "kind", "owner_name", "owner_kind", "network_name", "host_ip", "host_name", "zone")
    _fields_ = ([("ip", C.c_uint8 * 16)] + [(f, C.c_char_p) for f in _STRINGS] +
                [(f.rstrip("_") + "_len", C.c_uint32) for f in _STRINGS] + [("has_zone", C.c_uint8)])


class K8sLayer(C.Structure):
    """nfagg_k8s_layer (include/nfagg.h)."""
    _fields_ = [("struct_size", C.c_uint32), ("n_prefixes", C.c_uint32), ("infra_prefixes", C.POINTER(C.c_char_p)),
                ("infra_refs", C.POINTER(C.c_char_p)), ("n_refs", C.c_uint32), ("pad_", C.c_uint32)]


K8S_MAX_RENDERED, K8S_MAX_ROWS, K8S_NO_ROW = 2048, 1 << 22, 0xFFFFFFFF


class NetCidr(C.Structure):
    """nfagg_net_cidr (include/nfagg.h)."""
    _fields_ = [("ip", C.c_uint8 * 16), ("ones", C.c_uint32), ("bits", C.c_uint32), ("label", C.c_uint32)]


class NetLabel(C.Structure):
    """nfagg_net_label (include/nfagg.h)."""
    _fields_ = [("text", C.c_char_p), ("len", C.c_uint32), ("pad_", C.c_uint32)]


class NetRules(C.Structure):
    """nfagg_net_rules (include/nfagg.h)."""
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("cidrs", C.POINTER(NetCidr)), ("labels", C.POINTER(NetLabel)),
                ("n_cidrs", C.c_uint32), ("n_labels", C.c_uint32)]


class NetRow(C.Structure):
    """nfagg_net_row (include/nfagg.h)."""
    _fields_ = [("src_label", C.c_uint16), ("dst_label", C.c_uint16), ("direction", C.c_uint8), ("pad_", C.c_uint8 * 3)]


NET_REINTERPRET_DIRECTION, NET_SUBNET_LABELS, NET_DECODE_TCP_FLAGS = 1, 2, 4
NET_MAX_CIDRS, NET_LABEL_MAX, NET_NO_LABEL, NET_NO_DIRECTION = 1024, 256, 0xFFFF, 0xFF

# flow metrics (nfagg_metrics_*): one grouping is a mask of dimensions
DIM_SRC_K8S, DIM_DST_K8S = (lambda f: 1 << f), (lambda f: 1 << (9 + f))      # f: index into table.K8S_FIELDS
DIM_SRC_SUBNET_LABEL, DIM_DST_SUBNET_LABEL, DIM_FLOW_DIRECTION, DIM_FLOW_LAYER, DIM_PROTO = 1 << 18, 1 << 19, 1 << 20, 1 << 21, 1 << 22
DIM_ALL = (1 << 23) - 1
MET_MAX_GROUPINGS, MET_MAX_GROUPS = 8, 1 << 20
# the content fold (nfagg_metrics_fold_content): value sources, extra dimensions, buckets
MET_VALUE_NONE, MET_VALUE_RTT_NS, MET_VALUE_DNS_LATENCY_MS, MET_VALUE_DROP_BYTES, MET_VALUE_DROP_PACKETS, MET_VALUE_BYTES, MET_VALUE_PACKETS = range(7)
XDIM_DNS_RCODE, XDIM_DROP_CAUSE, XDIM_DROP_STATE, XDIM_IPSEC_STATUS, XDIM_ALL = 1, 2, 4, 8, 15
MET_MAX_BOUNDS, MET_NO_BUCKET = 32, 0xFF
FLP_ENUM_DNS_RCODE, FLP_ENUM_TCP_STATE, FLP_ENUM_DROP_CAUSE = 0, 1, 2


class MetricSpec(C.Structure):
    """nfagg_metric_spec (include/nfagg.h)."""
    _fields_ = [("struct_size", C.c_uint32), ("dims", C.c_uint32), ("xdims", C.c_uint32), ("value", C.c_uint8 * 2), ("hist", C.c_uint8),
                ("pad_", C.c_uint8), ("n_bounds", C.c_uint32), ("pad2_", C.c_uint32), ("bounds", C.c_int64 * 32)]


# write loki (nfagg_loki_*): maskable keys are the NFAGG_DIM_* bits without Proto, and two of their own
LOKI_KEY_RECORD_TYPE, LOKI_KEY_HASH_ID = 1 << 23, 1 << 24
LOKI_KEY_ALL = (DIM_ALL & ~DIM_PROTO) | LOKI_KEY_RECORD_TYPE | LOKI_KEY_HASH_ID
LOKI_TS_NOW, LOKI_TS_TIME_FLOW_END_MS, LOKI_TS_TIME_FLOW_START_MS = 0, 1, 2
LOKI_MAX_STREAMS, LOKI_LABELS_MAX = 1 << 20, 4096


class LokiSpec(C.Structure):
    """nfagg_loki_spec (include/nfagg.h)."""
    _fields_ = [("struct_size", C.c_uint32), ("label_keys", C.c_uint32), ("ignore_keys", C.c_uint32), ("timestamp_source", C.c_uint32),
                ("timestamp_scale", C.c_double), ("batch_size", C.c_uint32), ("pad_", C.c_uint32)]


class LokiCounts(C.Structure):
    """nfagg_loki_counts (include/nfagg.h)."""
    _fields_ = [("n_streams", C.c_uint32), ("n_groups", C.c_uint32), ("n_batches", C.c_uint32), ("n_deferred", C.c_uint32)]


# write ipfix (nfagg_flp_ipfix_*)
FLP_IPFIX_MAX_STRING, FLP_IPFIX_N_STRINGS = 1024, 9
FLP_IPFIX_SENT, FLP_IPFIX_FAIL_FAMILY, FLP_IPFIX_FAIL_SIZE = 0, 1, 2


class FlpIpfixOptions(C.Structure):
    """nfagg_flp_ipfix_options (include/nfagg.h)."""
    _fields_ = [
        ("struct_size", C.c_uint32), ("n_names", C.c_uint32), ("now_unix_ns", C.c_int64), ("mono_now_ns", C.c_uint64),
        ("names", C.c_void_p), ("unknown_name", C.c_char * 16), ("unknown_len", C.c_uint8), ("flags_decoded", C.c_uint8),
        ("pad_", C.c_uint8 * 2), ("export_time_s", C.c_uint32), ("seq0", C.c_uint32), ("obs_domain_id", C.c_uint32),
        ("template_id_v4", C.c_uint16), ("template_id_v6", C.c_uint16), ("enterprise_id", C.c_uint32), ("max_msg_size", C.c_uint32),
    ]


class FlpIpfixElements(C.Structure):
    """nfagg_flp_ipfix_elements (include/nfagg.h), 9424 bytes."""
    _fields_ = [
        ("struct_size", C.c_uint32), ("addr_set", C.c_uint8), ("xlat_set", C.c_uint8), ("mac_set", C.c_uint8), ("pad0_", C.c_uint8),
        ("src_addr", C.c_uint8 * 16), ("dst_addr", C.c_uint8 * 16), ("xlat_src_addr", C.c_uint8 * 16), ("xlat_dst_addr", C.c_uint8 * 16),
        ("src_mac", C.c_uint8 * 6), ("dst_mac", C.c_uint8 * 6),
        ("proto", C.c_uint8), ("icmp_type", C.c_uint8), ("icmp_code", C.c_uint8), ("flow_direction", C.c_uint8),
        ("etype", C.c_uint16), ("src_port", C.c_uint16), ("dst_port", C.c_uint16), ("flags", C.c_uint16), ("xlat_src_port", C.c_uint16),
        ("xlat_dst_port", C.c_uint16), ("selector_algorithm", C.c_uint16), ("pad1_", C.c_uint16),
        ("bytes", C.c_uint64), ("packets", C.c_uint64), ("start_ms", C.c_uint64), ("end_ms", C.c_uint64), ("rtt_ns", C.c_uint64),
        ("sampling_probability", C.c_double), ("str_len", C.c_uint32 * 9), ("pad3_", C.c_uint32 * 5), ("str", (C.c_uint8 * 1024) * 9),
    ]


# conversation tracking (nfagg_conn_*)
CONN_MAX_CONNS, CONN_NO_IDX = 1 << 22, 0xFFFFFFFF


CONN_MAX_FIELDS, CONN_NAME_MAX = 32, 64
CONN_OPS = {"count": 0, "sum": 1, "min": 2, "max": 3, "first": 4, "last": 5}                                      # NFAGG_CONN_OP_*
CONN_INPUTS = {"": 0, "Bytes": 1, "Packets": 2, "TimeFlowStartMs": 3, "TimeFlowEndMs": 4, "SrcAddr": 5, "DstAddr": 6, "SrcPort": 7, "DstPort": 8,
               "Proto": 9, "SrcMac": 10, "DstMac": 11, "Etype": 12, "Dscp": 13, "IfDirections": 14}                 # NFAGG_CONN_IN_*
CONN_RECORD_TYPES = {"newConnection": 0, "endConnection": 1, "heartbeat": 2}                                      # NFAGG_CONN_RECORD_*


# extract timebased (nfagg_timebased_*)
TB_MAX_TABLES, TB_MAX_RULES, TB_MAX_COLUMNS, TB_MAX_VALUES, TB_MAX_KEYS, TB_MAX_TOPK, TB_MAX_SLICES = 4, 16, 4, 4, 1 << 24, 4096, 1024
TB_OP_SUM, TB_OP_AVG, TB_OP_MIN, TB_OP_MAX, TB_OP_COUNT, TB_OP_LAST, TB_OP_DIFF = range(1, 8)
TB_INEXACT = 1


class TbRule(C.Structure):
    """nfagg_tb_rule (include/nfagg.h)."""
    _fields_ = [("struct_size", C.c_uint32), ("n_index_keys", C.c_uint32), ("index_keys", C.c_char_p * 4), ("operation", C.c_uint32),
                ("value", C.c_uint32), ("top_k", C.c_uint32), ("reversed", C.c_uint32), ("interval_ns", C.c_int64)]


class TbOptions(C.Structure):
    """nfagg_tb_options (include/nfagg.h)."""
    _fields_ = [("struct_size", C.c_uint32), ("max_keys", C.c_uint32)]


class TbStats(C.Structure):
    """nfagg_tb_stats (include/nfagg.h)."""
    _fields_ = [("n_tables", C.c_uint32), ("n_rules", C.c_uint32), ("keys", C.c_uint32 * 4), ("slots", C.c_uint32 * 4), ("slices", C.c_uint32 * 4),
                ("table_of_rule", C.c_uint32 * 16), ("bytes_held", C.c_uint64), ("last_now_ns", C.c_int64), ("failed", C.c_uint32),
                ("has_clock", C.c_uint32)]


class ConnField(C.Structure):
    """nfagg_conn_field (include/nfagg.h)."""
    _fields_ = [("name", C.c_char_p), ("name_len", C.c_uint32), ("op", C.c_uint8), ("input", C.c_uint8), ("split_ab", C.c_uint8), ("pad_", C.c_uint8)]


class ConnOptions(C.Structure):
    """nfagg_conn_options (include/nfagg.h)."""
    _fields_ = [("struct_size", C.c_uint32), ("reserved_", C.c_uint32), ("now_unix_ns", C.c_int64), ("mono_now_ns", C.c_uint64)]


class ConnPartial(C.Structure):
    """nfagg_conn_partial (include/nfagg.h), 128 bytes; table.CONN_PARTIAL is the numpy view."""
    _fields_ = [("hash_total", C.c_uint64), ("first_hash_a", C.c_uint64), ("first_idx", C.c_uint32), ("last_idx", C.c_uint32),
                ("first_fin_idx", C.c_uint32), ("flags_or", C.c_uint32), ("flows", C.c_uint64 * 2), ("bytes", C.c_uint64 * 2),
                ("packets", C.c_uint64 * 2), ("start_ms_min", C.c_int64), ("end_ms_max", C.c_int64), ("pad_", C.c_uint64 * 4)]


# transform filter (nfagg_filter_*)
FILTER_MAX_ATOMS, FILTER_MAX_OPS, FILTER_MAX_STEPS, FILTER_MAX_STACK, FILTER_NO_RULE = 64, 256, 32, 32, 0xFF
FILTER_STORE_SAMPLING = 1


class FilterAtom(C.Structure):
    """nfagg_filter_atom (include/nfagg.h), 48 bytes."""
    _fields_ = [("kind", C.c_uint8), ("field", C.c_uint8), ("cmp", C.c_uint8), ("dim", C.c_uint8), ("side", C.c_uint8), ("value_const", C.c_uint8),
                ("pad_", C.c_uint8 * 2), ("value", C.c_int64), ("bytes", C.c_uint8 * 16), ("truth", C.c_void_p), ("n_truth", C.c_uint32),
                ("pad2_", C.c_uint32)]


class FilterStep(C.Structure):
    """nfagg_filter_step (include/nfagg.h), 8 bytes."""
    _fields_ = [("kind", C.c_uint8), ("group", C.c_uint8), ("value", C.c_uint16), ("op_begin", C.c_uint16), ("op_count", C.c_uint16)]


class FilterSpec(C.Structure):
    """nfagg_filter_spec (include/nfagg.h)."""
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("n_atoms", C.c_uint32), ("n_ops", C.c_uint32), ("n_steps", C.c_uint32),
                ("pad_", C.c_uint32), ("atoms", C.c_void_p), ("ops", C.c_void_p), ("steps", C.c_void_p)]


TLS_VERSION, TLS_CIPHER_SUITE, TLS_GROUP = 0, 1, 2
TLS_NAME_MAX, TLS_MAX_ROWS = 63, 256

NETEV_ACL, NETEV_OTHER, NETEV_UNDECODABLE = 0, 1, 2
NETEV_JSON, NETEV_PB = 0, 1
NETEV_MAX_RENDERED, NETEV_MAX_ROWS, NETEV_NO_ROW = 512, 65535, 0xFFFF

FEAT_ADDITIONAL, FEAT_DNS, FEAT_DROPS, FEAT_NETWORK_EVENTS, FEAT_XLAT, FEAT_QUIC = 1, 2, 4, 8, 16, 32


class Stats(C.Structure):
    _fields_ = [
        ("records_ingested", C.c_uint64), ("records_skipped", C.c_uint64), ("entries", C.c_uint64),
        ("evictions", C.c_uint64 * 3), ("evicted_flows", C.c_uint64 * 3), ("epoch_seq", C.c_uint64),
        ("table_slots", C.c_uint64), ("table_bytes", C.c_uint64),
        ("ingest_launches", C.c_uint64), ("ingest_kernel_ms", C.c_double),
        ("evict_launches", C.c_uint64), ("evict_kernel_ms", C.c_double),
        ("sketch_launches", C.c_uint64), ("sketch_kernel_ms", C.c_double), ("max_probe", C.c_uint64),
        ("records_bypassed", C.c_uint64),
        ("optimistic_folds", C.c_uint64), ("optimistic_rollbacks", C.c_uint64), ("sequence_rebases", C.c_uint64),
        ("account_epochs_first", C.c_uint64), ("account_chain", C.c_uint64), ("account_declined", C.c_uint64),
    ]


_vp, _sz, _psz = C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)

# every symbol include/nfagg.h declares, with its signature
SIGNATURES = {
    "nfagg_abi_version": (C.c_uint32, []),
    "nfagg_create": (C.c_int, [C.POINTER(Config), C.POINTER(_vp)]),
    "nfagg_destroy": (None, [_vp]),
    "nfagg_last_error": (C.c_char_p, [_vp]),
    "nfagg_ingest": (C.c_int, [_vp, _vp, _sz, _psz]),
    "nfagg_ingest_device": (C.c_int, [_vp, _vp, _sz, _psz]),
    "nfagg_host_alloc": (C.c_int, [C.c_size_t, C.POINTER(_vp)]),
    "nfagg_host_free": (None, [_vp]),
    "nfagg_host_threads": (C.c_int, [C.c_uint, C.c_int]),
    "nfagg_host_info": (C.c_int, [_vp]),
    "nfagg_device_numa_node": (C.c_int, [C.c_int]),
    "nfagg_staging_acquire": (C.c_int, [_vp, C.POINTER(_vp), _psz]),
    "nfagg_staging_commit": (C.c_int, [_vp, _sz, _psz]),
    "nfagg_len": (C.c_int, [_vp, C.POINTER(C.c_uint64)]),
    "nfagg_evict": (C.c_int, [_vp, C.c_int, _vp, _sz, _psz]),
    "nfagg_evict_device": (C.c_int, [_vp, C.c_int, _vp, _sz, _psz]),
    "nfagg_account": (C.c_int, [_vp, _vp, _sz, _vp, _sz, C.POINTER(C.c_uint64), _sz, _psz, _psz]),
    "nfagg_account_device": (C.c_int, [_vp, _vp, _sz, _vp, _sz, C.POINTER(C.c_uint64), _sz, _psz, _psz]),
    "nfagg_record_times": (None, [C.c_int64, C.c_uint64, _vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "nfagg_rollup_additional": (C.c_int, [_vp, _vp, _sz, _sz, _vp, _vp]),
    "nfagg_rollup_dns": (C.c_int, [_vp, _vp, _sz, _sz, _vp, _vp]),
    "nfagg_rollup_drops": (C.c_int, [_vp, _vp, _sz, _sz, _vp, _vp]),
    "nfagg_rollup_network_events": (C.c_int, [_vp, _vp, _sz, _sz, _vp, _vp]),
    "nfagg_rollup_xlat": (C.c_int, [_vp, _vp, _sz, _sz, _vp, _vp]),
    "nfagg_rollup_quic": (C.c_int, [_vp, _vp, _sz, _sz, _vp, _vp]),
    "nfagg_sketch_snapshot": (C.c_int, [_vp, C.c_int, _vp, _sz]),
    "nfagg_sketch_device_ptr": (C.c_int, [_vp, C.c_int, C.POINTER(_vp), _psz]),
    "nfagg_sketch_reset": (C.c_int, [_vp]),
    "nfagg_hll_estimate": (C.c_int, [_vp, C.c_int, C.POINTER(C.c_double)]),
    "nfagg_cm_query": (C.c_int, [_vp, C.c_int, _vp, C.POINTER(C.c_uint64)]),
    "nfagg_hll_estimate_from_histogram": (C.c_double, [_vp, C.c_uint32]),
    "nfagg_ringbuf_drain": (C.c_int, [C.POINTER(RingBuf), _vp, _sz, _psz, _psz, _vp]),
    "nfagg_limit_batches": (C.c_size_t, [C.POINTER(C.c_uint64), _sz, _sz, _sz, _vp, C.POINTER(C.c_uint64)]),
    "nfagg_encode_pb": (C.c_int, [_vp, _vp, _sz, C.POINTER(PbOptions), _vp, _sz, _vp, _vp, _vp, _psz]),
    "nfagg_encode_pb_device": (C.c_int, [_vp, _vp, _sz, C.POINTER(PbOptions), _vp, _sz, _vp, _vp, _vp, _psz]),
    "nfagg_cm_topk": (C.c_int, [_vp, C.c_int, _vp, _sz, _sz, _vp, _psz]),
    "nfagg_cm_topk_device": (C.c_int, [_vp, C.c_int, _vp, _sz, _sz, _vp, _psz]),
    "nfagg_map_merge": (C.c_int, [_vp, C.POINTER(MapView), C.POINTER(MapView), _sz, C.POINTER(MergedFlows), _sz, _psz, _psz]),
    "nfagg_map_merge_device": (C.c_int, [_vp, C.POINTER(MapView), C.POINTER(MapView), _sz, C.POINTER(MergedFlows), _sz, _psz, _psz]),
    "nfagg_encode_pb_content": (C.c_int, [_vp, _vp, _sz, C.POINTER(PbFeatures), C.POINTER(PbOptions), _vp, _sz, _vp, _vp, _vp, _psz]),
    "nfagg_encode_pb_content_device": (C.c_int, [_vp, _vp, _sz, C.POINTER(PbFeatures), C.POINTER(PbOptions), _vp, _sz, _vp, _vp, _vp, _psz]),
    "nfagg_ipfix_template": (C.c_int, [C.POINTER(IpfixOptions), C.c_int, _vp, _sz, _psz]),
    "nfagg_encode_ipfix": (C.c_int, [_vp, _vp, _sz, C.POINTER(IpfixOptions), _vp, _sz, _vp, _psz]),
    "nfagg_encode_ipfix_device": (C.c_int, [_vp, _vp, _sz, C.POINTER(IpfixOptions), _vp, _sz, _vp, _psz]),
    "nfagg_encode_flp_json": (C.c_int, [_vp, _vp, _sz, C.POINTER(FlpOptions), _vp, _sz, _vp, _vp, _psz, _psz]),
    "nfagg_encode_flp_json_device": (C.c_int, [_vp, _vp, _sz, C.POINTER(FlpOptions), _vp, _sz, _vp, _vp, _psz, _psz]),
    "nfagg_encode_flp_json_content": (C.c_int, [_vp, _vp, _sz, C.POINTER(PbFeatures), C.POINTER(FlpOptions), _vp, _sz, _vp, _vp, _psz, _psz]),
    "nfagg_encode_flp_json_content_device": (C.c_int, [_vp, _vp, _sz, C.POINTER(PbFeatures), C.POINTER(FlpOptions), _vp, _sz, _vp, _vp, _psz, _psz]),
    "nfagg_netev_render": (C.c_int, [C.POINTER(NetevEntry), C.c_int, _vp, _sz, _psz]),
    "nfagg_netev_table_create": (C.c_int, [_vp, C.POINTER(NetevEntry), _sz, C.POINTER(_vp)]),
    "nfagg_netev_table_destroy": (None, [_vp]),
    "nfagg_netev_resolve": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _sz, _vp, _vp, _vp, _vp, _sz, _psz, C.POINTER(C.c_int)]),
    "nfagg_netev_resolve_device": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _sz, _vp, _vp, _vp, _vp, _sz, _psz, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "nfagg_encode_pb_content_netev": (C.c_int, [_vp, _vp, _sz, C.POINTER(PbFeatures), _vp, _vp, C.POINTER(PbOptions), _vp, _sz, _vp, _vp, _vp, _psz]),
    "nfagg_encode_pb_content_netev_device": (C.c_int, [_vp, _vp, _sz, C.POINTER(PbFeatures), _vp, _vp, C.POINTER(PbOptions), _vp, _sz, _vp, _vp, _vp, _psz]),
    "nfagg_encode_flp_json_content_netev": (C.c_int, [_vp, _vp, _sz, C.POINTER(PbFeatures), _vp, _vp, C.POINTER(FlpOptions), _vp, _sz, _vp, _vp, _psz, _psz]),
    "nfagg_encode_flp_json_content_netev_device": (C.c_int, [_vp, _vp, _sz, C.POINTER(PbFeatures), _vp, _vp, C.POINTER(FlpOptions), _vp, _sz, _vp, _vp, _psz, _psz]),
    "nfagg_tls_names_create": (C.c_int, [_vp, C.POINTER(TlsNameEntry), _sz, C.POINTER(_vp)]),
    "nfagg_tls_names_destroy": (None, [_vp]),
    "nfagg_tls_names_render": (C.c_int, [_vp, C.c_int, C.c_uint16, C.c_int, _vp, _sz, _psz]),
    "nfagg_encode_flp_json_tls": (C.c_int, [_vp, _vp, _sz, C.POINTER(PbFeatures), _vp, _vp, _vp, C.POINTER(FlpOptions), _vp, _sz, _vp, _psz]),
    "nfagg_encode_flp_json_tls_device": (C.c_int, [_vp, _vp, _sz, C.POINTER(PbFeatures), _vp, _vp, _vp, C.POINTER(FlpOptions), _vp, _sz, _vp, _psz]),
    "nfagg_flp_json_tls_max_line": (C.c_uint32, [C.c_int]),
    "nfagg_k8s_render": (C.c_int, [C.POINTER(K8sEntry), C.c_int, _vp, _sz, _psz]),
    "nfagg_k8s_table_create": (C.c_int, [_vp, C.POINTER(K8sEntry), _sz, C.POINTER(K8sLayer), C.POINTER(_vp)]),
    "nfagg_k8s_table_destroy": (None, [_vp]),
    "nfagg_k8s_resolve": (C.c_int, [_vp, _vp, _vp, _sz, _vp]),
    "nfagg_k8s_resolve_device": (C.c_int, [_vp, _vp, _vp, _sz, _vp]),
    "nfagg_encode_flp_json_k8s": (C.c_int, [_vp, _vp, _sz, C.POINTER(PbFeatures), _vp, _vp, _vp, _vp, C.POINTER(FlpOptions), _vp, _sz, _vp, _psz]),
    "nfagg_encode_flp_json_k8s_device": (C.c_int, [_vp, _vp, _sz, C.POINTER(PbFeatures), _vp, _vp, _vp, _vp, C.POINTER(FlpOptions), _vp, _sz, _vp, _psz]),
    "nfagg_flp_json_k8s_max_line": (C.c_uint32, [C.c_int]),
    "nfagg_net_table_create": (C.c_int, [_vp, C.POINTER(NetRules), C.POINTER(_vp)]),
    "nfagg_net_table_destroy": (None, [_vp]),
    "nfagg_net_render": (C.c_int, [_vp, C.c_int, C.c_uint32, _vp, _sz, _psz]),
    "nfagg_net_resolve": (C.c_int, [_vp, _vp, _vp, _vp, _sz, _vp, C.POINTER(FlpOptions), _vp]),
    "nfagg_net_resolve_device": (C.c_int, [_vp, _vp, _vp, _vp, _sz, _vp, C.POINTER(FlpOptions), _vp]),
    "nfagg_encode_flp_json_net": (C.c_int, [_vp, _vp, _sz, C.POINTER(PbFeatures), _vp, _vp, _vp, _vp, _vp, C.POINTER(FlpOptions), _vp, _sz, _vp, _psz]),
    "nfagg_encode_flp_json_net_device": (C.c_int, [_vp, _vp, _sz, C.POINTER(PbFeatures), _vp, _vp, _vp, _vp, _vp, C.POINTER(FlpOptions), _vp, _sz, _vp, _psz]),
    "nfagg_flp_json_net_max_line": (C.c_uint32, [C.c_int]),
    "nfagg_encode_flp_json_conn": (C.c_int, [_vp, _vp, _sz, C.POINTER(PbFeatures), _vp, _vp, _vp, _vp, _vp, _vp, C.POINTER(FlpOptions), _vp, _sz, _vp, _psz]),
    "nfagg_encode_flp_json_conn_device": (C.c_int, [_vp, _vp, _sz, C.POINTER(PbFeatures), _vp, _vp, _vp, _vp, _vp, _vp, C.POINTER(FlpOptions), _vp, _sz, _vp, _psz]),
    "nfagg_flp_json_conn_max_line": (C.c_uint32, [C.c_int]),
    "nfagg_metrics_table_create": (C.c_int, [_vp, _vp, C.POINTER(C.c_uint32), C.c_uint32, C.POINTER(_vp)]),
    "nfagg_metrics_table_destroy": (None, [_vp]),
    "nfagg_metrics_n_classes": (C.c_uint32, [_vp, C.c_uint32, C.c_int]),
    "nfagg_metrics_class_row": (C.c_int, [_vp, C.c_uint32, C.c_int, C.c_uint32, C.POINTER(C.c_uint32)]),
    "nfagg_metrics_fold": (C.c_int, [_vp, _vp, _vp, _sz, _vp, _vp, C.POINTER(C.c_uint32), C.POINTER(_vp), C.POINTER(C.c_uint32)]),
    "nfagg_metrics_fold_device": (C.c_int, [_vp, _vp, _vp, _sz, _vp, _vp, C.POINTER(C.c_uint32), C.POINTER(_vp), C.POINTER(C.c_uint32)]),
    "nfagg_metrics_table_create_specs": (C.c_int, [_vp, _vp, C.POINTER(MetricSpec), C.c_uint32, C.POINTER(_vp)]),
    "nfagg_metrics_fold_content": (C.c_int, [_vp, _vp, _vp, _sz, C.POINTER(PbFeatures), _vp, _vp, C.POINTER(C.c_uint32), C.POINTER(_vp), C.POINTER(C.c_uint32)]),
    "nfagg_metrics_fold_content_device": (C.c_int, [_vp, _vp, _vp, _sz, C.POINTER(PbFeatures), _vp, _vp, C.POINTER(C.c_uint32), C.POINTER(_vp),
                                                    C.POINTER(C.c_uint32)]),
    "nfagg_flp_enum_name": (C.c_int, [C.c_int, C.c_uint32, _vp, _sz, _psz]),
    "nfagg_conn_fold": (C.c_int, [_vp, _vp, _sz, C.POINTER(ConnOptions), _vp, C.c_uint32, _vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "nfagg_conn_fold_device": (C.c_int, [_vp, _vp, _sz, C.POINTER(ConnOptions), _vp, C.c_uint32, _vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "nfagg_conn_layout_create": (C.c_int, [_vp, C.POINTER(ConnField), _sz, C.POINTER(_vp)]),
    "nfagg_conn_layout_destroy": (None, [_vp]),
    "nfagg_conn_layout_columns": (C.c_uint32, [_vp]),
    "nfagg_conn_layout_max_line": (C.c_uint32, [_vp]),
    "nfagg_conn_layout_render": (C.c_int, [_vp, C.c_uint32, _vp, _sz, _psz]),
    "nfagg_encode_conn_json": (C.c_int, [_vp, _vp, _vp, _sz, _vp, _vp, _vp, _vp, _sz, _vp, _vp, _psz, _psz]),
    "nfagg_encode_conn_json_device": (C.c_int, [_vp, _vp, _vp, _sz, _vp, _vp, _vp, _vp, _sz, _vp, _vp, _psz, _psz]),
    "nfagg_conn_hash": (C.c_uint64, [_vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "nfagg_filter_create": (C.c_int, [_vp, _vp, _vp, C.POINTER(FilterSpec), C.POINTER(_vp)]),
    "nfagg_filter_destroy": (None, [_vp]),
    "nfagg_filter_roll": (C.c_int, [C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32]),
    "nfagg_filter_apply": (C.c_int, [_vp, _vp, _vp, _sz, C.POINTER(PbFeatures), _vp, _vp, C.POINTER(FlpOptions), C.c_uint64, C.c_uint64, _vp, _vp, _vp,
                                     _vp, _sz, _psz, _psz]),
    "nfagg_filter_apply_device": (C.c_int, [_vp, _vp, _vp, _sz, C.POINTER(PbFeatures), _vp, _vp, C.POINTER(FlpOptions), C.c_uint64, C.c_uint64, _vp, _vp,
                                            _vp, _vp, _sz, _psz, _psz]),
    "nfagg_loki_table_create": (C.c_int, [_vp, _vp, _vp, C.POINTER(LokiSpec), C.POINTER(_vp)]),
    "nfagg_loki_table_destroy": (None, [_vp]),
    "nfagg_loki_n_classes": (C.c_uint32, [_vp, C.c_int]),
    "nfagg_loki_class_row": (C.c_int, [_vp, C.c_int, C.c_uint32, C.POINTER(C.c_uint32)]),
    "nfagg_loki_render": (C.c_int, [_vp, C.c_int, C.c_uint32, _vp, _sz, _psz]),
    "nfagg_loki_plan": (C.c_int, [_vp, _vp, _sz, C.POINTER(PbFeatures), _vp, _vp, _vp, _vp, _vp, _vp, C.POINTER(FlpOptions), _vp, C.c_int64, _vp,
                                  C.c_uint32, _vp, C.c_uint32, _vp, C.POINTER(LokiCounts)]),
    "nfagg_loki_plan_device": (C.c_int, [_vp, _vp, _sz, C.POINTER(PbFeatures), _vp, _vp, _vp, _vp, _vp, _vp, C.POINTER(FlpOptions), _vp, C.c_int64, _vp,
                                         C.c_uint32, _vp, C.c_uint32, _vp, C.POINTER(LokiCounts)]),
    "nfagg_loki_write": (C.c_int, [_vp, _vp, _vp, _vp, _sz, _vp, _vp, _psz]),
    "nfagg_loki_write_device": (C.c_int, [_vp, _vp, _vp, _vp, _sz, _vp, _vp, _psz]),
    "nfagg_loki_max_entry": (C.c_uint32, [C.c_int]),
    "nfagg_flp_ipfix_template": (C.c_int, [C.POINTER(FlpIpfixOptions), C.c_int, _vp, _sz, _psz]),
    "nfagg_flp_ipfix_strings_create": (C.c_int, [_vp, C.POINTER(K8sEntry), _sz, C.POINTER(_vp)]),
    "nfagg_flp_ipfix_strings_destroy": (None, [_vp]),
    "nfagg_flp_ipfix_writer_create": (C.c_int, [_vp, C.POINTER(_vp)]),
    "nfagg_flp_ipfix_writer_destroy": (None, [_vp]),
    "nfagg_flp_ipfix_writer_get": (C.c_int, [_vp, C.c_int, C.POINTER(FlpIpfixElements)]),
    "nfagg_flp_ipfix_writer_reset": (C.c_int, [_vp]),
    "nfagg_flp_ipfix_write": (C.c_int, [_vp, _vp, _vp, _sz, C.POINTER(PbFeatures), _vp, _vp, C.POINTER(FlpIpfixOptions), _vp, _sz, _vp, _vp, _psz, _psz]),
    "nfagg_flp_ipfix_write_device": (C.c_int, [_vp, _vp, _vp, _sz, C.POINTER(PbFeatures), _vp, _vp, C.POINTER(FlpIpfixOptions), _vp, _sz, _vp, _vp, _psz,
                                               _psz]),
    "nfagg_gather": (C.c_int, [_vp, _vp, _sz, _sz, _vp, _sz, _vp]),
    "nfagg_gather_device": (C.c_int, [_vp, _vp, _sz, _sz, _vp, _sz, _vp]),
    "nfagg_shard_of": (C.c_uint32, [_vp, C.c_uint32]),
    "nfagg_shard_ids": (None, [_vp, _sz, C.c_uint32, _vp]),
    "nfagg_key_hash": (C.c_uint64, [_vp]),
    "nfagg_ip_hash": (C.c_uint64, [_vp, C.c_uint32]),
    "nfagg_timebased_rules_create": (C.c_int, [_vp, _vp, _vp, C.POINTER(TbRule), C.c_uint32, C.POINTER(TbOptions), C.POINTER(_vp)]),
    "nfagg_timebased_destroy": (None, [_vp]),
    "nfagg_timebased_extract": (C.c_int, [_vp, _vp, _vp, _sz, C.POINTER(PbFeatures), _vp, _vp, C.c_int64, C.POINTER(C.c_uint32), C.POINTER(_vp),
                                          C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]),
    "nfagg_timebased_extract_device": (C.c_int, [_vp, _vp, _vp, _sz, C.POINTER(PbFeatures), _vp, _vp, C.c_int64, C.POINTER(C.c_uint32), C.POINTER(_vp),
                                                 C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]),
    "nfagg_timebased_results": (C.c_int, [_vp, _vp, C.POINTER(C.c_uint32), C.POINTER(_vp), C.POINTER(C.c_uint32)]),
    "nfagg_timebased_results_device": (C.c_int, [_vp, _vp, C.POINTER(C.c_uint32), C.POINTER(_vp), C.POINTER(C.c_uint32)]),
    "nfagg_timebased_keys": (C.c_int, [_vp, C.c_uint32, _vp, _sz, _vp]),
    "nfagg_timebased_class_row": (C.c_int, [_vp, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32)]),
    "nfagg_timebased_key_hash": (C.c_uint64, [_vp, C.c_uint32, _vp]),
    "nfagg_timebased_reset": (C.c_int, [_vp]),
    "nfagg_timebased_stats": (C.c_int, [_vp, C.POINTER(TbStats)]),
    "nfagg_metrics_group_hash": (C.c_uint64, [C.c_uint32, _vp]),
    "nfagg_metrics_group_hash_content": (C.c_uint64, [C.c_uint32, _vp]),
    "nfagg_stats_get": (C.c_int, [_vp, C.POINTER(Stats)]),
    "nfagg_stats_reset_profile": (C.c_int, [_vp]),
    "nfagg_sync": (C.c_int, [_vp]),
    "nfagg_stream": (_vp, [_vp]),
    "nfagg_debug_skip_sequence": (C.c_int, [_vp, C.c_uint64]),
    "nfagg_debug_live_buffers": (C.c_uint64, []),
    "nfagg_set_sequence": (C.c_int, [_vp, C.c_uint64]),
    "nfagg_partial_bytes": (C.c_size_t, [_vp]),
    "nfagg_partials_export_device": (C.c_int, [_vp, C.c_uint32, C.c_uint32, _vp, _sz, C.POINTER(C.c_uint64), _psz]),
    "nfagg_partials_merge_device": (C.c_int, [_vp, C.c_uint32, C.c_uint32, _vp, _sz]),
    "nfagg_window_restart_device": (C.c_int, [_vp, C.c_uint32, C.c_uint32, _vp, _sz, C.c_uint64]),
    "nfagg_evict_owned_device": (C.c_int, [_vp, C.c_int, C.c_uint32, C.c_uint32, _vp, _sz, _psz]),
    "nfagg_group_debug_skip_sequence": (C.c_int, [_vp, C.c_uint64]),
    "nfagg_group_create": (C.c_int, [C.POINTER(Config), C.POINTER(C.c_int32), C.c_uint32, C.POINTER(_vp)]),
    "nfagg_group_destroy": (None, [_vp]),
    "nfagg_group_last_error": (C.c_char_p, [_vp]),
    "nfagg_group_size": (C.c_uint32, [_vp]),
    "nfagg_group_member": (_vp, [_vp, C.c_uint32]),
    "nfagg_group_ingest": (C.c_int, [_vp, _vp, _sz, _psz]),
    "nfagg_group_ingest_device": (C.c_int, [_vp, C.c_uint32, _vp, _sz, _psz]),
    "nfagg_group_len": (C.c_int, [_vp, C.POINTER(C.c_uint64)]),
    "nfagg_group_merge_sketches": (C.c_int, [_vp]),
    "nfagg_group_evict": (C.c_int, [_vp, C.c_int, _vp, _sz, _psz]),
    "nfagg_group_evict_device": (C.c_int, [_vp, C.c_int, C.POINTER(_vp), _psz, _psz]),
}

for _name, (_res, _args) in SIGNATURES.items():
    _fn = getattr(lib, _name)   # AttributeError here = the .so does not export the ABI
    _fn.restype = _res
    _fn.argtypes = _args


def load_synth():
    """libnfagg_synth.so: device-side synthetic stream generator (bench/test support)."""
    if not os.path.exists(SYNTH_PATH):
        raise ImportError(f"{SYNTH_PATH} is missing: build with make -C {os.path.join(_HERE, 'csrc')}")
    s = C.CDLL(SYNTH_PATH)
    u64 = C.c_uint64
    s.nfagg_synth_stream.restype = C.c_int
    s.nfagg_synth_stream.argtypes = [_vp, u64, u64, u64, u64, _vp, C.c_uint32, C.c_uint32, _vp, _vp]
    s.nfagg_synth_zipf_thresholds.restype = None
    s.nfagg_synth_zipf_thresholds.argtypes = [u64, C.c_double, _vp]
    s.nfagg_synth_shard_population.restype = None
    s.nfagg_synth_shard_population.argtypes = [u64, C.c_uint32, C.c_uint32, _vp]
    s.nfagg_synth_stream_host.restype = None
    s.nfagg_synth_stream_host.argtypes = [_vp, u64, u64, u64, u64, _vp, C.c_uint32, C.c_uint32, _vp]
    s.nfagg_synth_yardstick.restype = C.c_double
    s.nfagg_synth_yardstick.argtypes = [C.c_int, _vp, _vp, u64, _vp, C.c_int]
    return s
