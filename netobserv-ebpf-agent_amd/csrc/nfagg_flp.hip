// nfagg_flp.hip — evicted flow_record_t -> direct-FLP JSON lines, in bulk on the GPU. Replaces, for the records
// Accounter.evict produces,
//   pkg/model/record.go:82-114             NewRecord (flow start/end wall-clock times, the interface list)
//   pkg/decode/decode_protobuf.go:57-127   RecordToMap, the keys a BpfFlowMetrics-only record produces
//   flowlogs-pipeline write_stdout.go:37-51 with `format: json`, `reorder: true`:
//   jsoniter.Config{SortMapKeys: true}.Marshal(map) + "\n"
// Output: line i = out[line_offsets[i], line_offsets[i + 1]), '\n' included. A record whose TLS version, cipher suite or
// key share is set needs Go's crypto/tls name tables: its line is empty and it is flagged as deferred.
//
// Keys in byte order (what jsoniter's sorted map encoder gives), [] = only when the rule of RecordToMap says so:
//   AgentIP [Bytes] [Dscp] [DstAddr] DstMac [DstPort] Etype [Flags] [IcmpCode] [IcmpType] IfDirections Interfaces
//   [Packets] [Proto] [Sampling] [SrcAddr] SrcMac [SrcPort] [TLSTypes] TimeFlowEndMs TimeFlowStartMs TimeReceived Udns
//
// The two-pass skeleton of nfagg_encode.h. One encoder
// (encode_line) serves both passes: over a counting sink it adds digit counts (compares against powers of ten) and the
// escaped names' lengths, it never forms a digit or touches a name's bytes. Names and UDNs come escaped and quoted
// from the table the host escaped once per call. A wave writes its 64 lines into an LDS window of kFlpWindow bytes at
// their final relative positions and copies the window out with aligned 16-byte stores; 64 typical lines (~26 KB) fit
// one window. The window is bounded (32 KiB of LDS whatever the lines' lengths): a longer range takes several windows,
// each starting at a line start, so a line (at most kFlpMaxLine bytes) is written whole, once, through a plain pointer.
//
// The kernels are k_flp_size<Feat> and k_flp_write<Feat> of nfagg_flp_line.h. This file compiles them for FlpPlain, the policy
// of the records Accounter.evict produces: every hook empty, nothing loaded. An instantiation is a kernel of its own, so this
// path has its own code and registers (tests/test_isa_pins.py holds it to no scratch); nfagg_flp_content.hip compiles the other
// policies and has launch_flp_size / launch_flp_write, which select among all fifteen.
#include "nfagg_flp_line.h"

namespace nfagg {

template hipError_t flp_size_as<FlpPlain>(const FlpLineArgs&, uint32_t*, uint32_t*, uint32_t*, uint64_t*, uint32_t*, hipStream_t);
template hipError_t flp_write_as<FlpPlain>(const FlpLineArgs&, const uint32_t*, const uint32_t*, const uint64_t*, void*, uint64_t*, uint8_t*,
                                           hipStream_t);

}  // namespace nfagg
