// conntrack_hash_dump_test.go — HASH DUMP of flowlogs-pipeline's own computeHash, for a host with a Go toolchain; libnfagg's
// own build and tests neither compile nor run it. libnfagg's conversation fold (include/nfagg.h,
// "Conversation tracking") restates the gob message of every key field from encoding/gob's documentation; _HashId is pinned to
// that restatement (tests/conntrack_ref.py, tests/golden/conntrack_vectors.json), not to a Go run. This prints Go's values for the
// vectors' tuples beside the vectors', so that a difference shows at once.
//
// 1. Drop this file into pkg/pipeline/extract/conntrack/ of flowlogs-pipeline (it needs the package's unexported computeHash).
// 2. NFAGG_CONNTRACK_VECTORS=<libnfagg checkout>/tests/golden/conntrack_vectors.json go test ./pkg/pipeline/extract/conntrack/ -run TestConntrackHashDump -v
//    One line per tuple: hashA, hashB and hashTotal as Go computes them (lower-case hex, as strconv.FormatUint(h, 16) writes
//    _HashId), then the vector's three, then "ok" or "DIFFERS". The value types are RecordToMap's: string addresses, uint16
//    ports, uint8 protocol (decode_protobuf.go:57-127).
package conntrack

import (
	"encoding/json"
	"fmt"
	"hash/fnv"
	"os"
	"testing"

	"github.com/netobserv/flowlogs-pipeline/pkg/api"
	"github.com/netobserv/flowlogs-pipeline/pkg/config"
)

func TestConntrackHashDump(t *testing.T) {
	path := os.Getenv("NFAGG_CONNTRACK_VECTORS")
	if path == "" {
		t.Skip("NFAGG_CONNTRACK_VECTORS not set")
	}
	raw, err := os.ReadFile(path)
	if err != nil {
		t.Fatal(err)
	}
	var vectors struct {
		Tuples []struct {
			SrcText   string `json:"src_text"`
			DstText   string `json:"dst_text"`
			Sport     uint16 `json:"sport"`
			Dport     uint16 `json:"dport"`
			Proto     uint8  `json:"proto"`
			HashA     string `json:"hash_a"`
			HashB     string `json:"hash_b"`
			HashTotal string `json:"hash_total"`
		} `json:"tuples"`
	}
	if err := json.Unmarshal(raw, &vectors); err != nil {
		t.Fatal(err)
	}
	kd := api.KeyDefinition{
		FieldGroups: []api.FieldGroup{
			{Name: "src", Fields: []string{"SrcAddr", "SrcPort"}},
			{Name: "dst", Fields: []string{"DstAddr", "DstPort"}},
			{Name: "common", Fields: []string{"Proto"}},
		},
		Hash: api.ConnTrackHash{FieldGroupRefs: []string{"common"}, FieldGroupARef: "src", FieldGroupBRef: "dst"},
	}
	differs := 0
	for _, v := range vectors.Tuples {
		fl := config.GenericMap{"SrcAddr": v.SrcText, "SrcPort": v.Sport, "DstAddr": v.DstText, "DstPort": v.Dport, "Proto": v.Proto}
		h, err := computeHash(fl, &kd, fnv.New64a(), nil)
		if err != nil {
			t.Fatal(err)
		}
		a, b, total := fmt.Sprintf("%x", h.hashA), fmt.Sprintf("%x", h.hashB), fmt.Sprintf("%x", h.hashTotal)
		verdict := "ok"
		if a != v.HashA || b != v.HashB || total != v.HashTotal {
			verdict = "DIFFERS"
			differs++
		}
		fmt.Printf("%s:%d > %s:%d proto %d  go %s %s %s  vector %s %s %s  %s\n", v.SrcText, v.Sport, v.DstText, v.Dport, v.Proto, a, b, total,
			v.HashA, v.HashB, v.HashTotal, verdict)
	}
	if differs != 0 {
		t.Errorf("%d of %d tuples differ from the vectors", differs, len(vectors.Tuples))
	}
}
