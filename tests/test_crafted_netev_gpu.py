"""The batteries of tests/netevcraft.py through csrc/nfagg_netev.hip (k_netev_resolve, netev_find, netev_missing) and the *_netev
encoders, bit for bit against tests/netev_ref.py, host and device entry points (the helpers of tests/test_netev_gpu.py):

  scripts   all 10^4 sequences of four slot symbols x four states of the drops part, against the ten answers alone (LDS search) and
            among 300-odd fillers (HBM search, stride 32); host entry, device entry out of place and in place
  search    cookies one dword, one bit or a byte swap apart and the ends of the range, every table cookie found and every +- 1
            neighbour missing; evenly spaced tables of 1 .. 65 535 rows with every row probed (row 0xFFFE returned), one probe
            below and one above; the encoders over the first and last 128 flows of the largest call
  missing   the missing-cookie set on cookies with chosen home slots: one home, chains through slot 0, exactly full, one over, the
            all-zero cookie beside a full set; every stored cookie on its probe path from mix(cookie) % cap
  pieces    Message events of every length 0..140 and 484..498 through both encoders, every length at every slot of a line; rows
            with holes handed straight to the encoders

tests/test_netevcraft_cpu.py holds the batteries to that list. A failing script is named by its four symbols and its drops state.

Sensitivity, observed once on an MI355X with the library rebuilt from a scratch copy of csrc/nfagg_netev.hip carrying one changed
token (compares and arithmetic only; no mutant touches a bound, an index or a pointer). "old" is tests/test_netev_gpu.py, 24 tests:

  mutant                                                              this file (26 tests)                      old
  netev_find compares (uint32_t) of both sides                        14 fail: scripts 6, search 8              10 fail of 22, 2 never end
  netev_find compares >> 32 of both sides                             18 fail: scripts 6, search 11, pieces 1   not run: the same two
  seen: `(uint32_t)j < cnt && cls[j] == c` -> `cls[j] == c`           18 fail: scripts 6, search 11, pieces 1   14 fail
  `dw[5] = cause` only where the part is created (first cause wins)   6 fail: scripts 6                         14 fail
  sat16 on bytes only (packets: the sum masked to 16 bits)            6 fail: scripts 6                         7 fail
  netev_mix: `x >> 27` -> `x >> 28`                                   6 fail: missing, every cap but 1          all pass

The old file tells the loop mutants too (its PATTERNS meet a second cause and a saturating packet count); what it cannot tell is the
hash of the set, and under a search that loses a cookie of the table its two tests with the shim's protocol loop (resolve, decode
the missing cookies, rebuild, resolve again: test_missing_set_capacities_and_the_loop, test_map_tracer_with_a_python_decoder) never
converge — the loop is the host's, every call returns — which is why no test of this file loops until nothing is missing. Without
`j < cnt` an unset `seen` entry is class 0, the table's first row: an event of that row is taken for seen and never kept.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import netev_ref as N  # noqa: E402
import netevcraft as nc  # noqa: E402
import test_flp_json_gpu as G  # noqa: E402
import test_netev_gpu as E  # noqa: E402

pytestmark = pytest.mark.gpu

NOW, MONO, RECEIVED, AGENT, NAMES = G.NOW, G.MONO, G.RECEIVED, G.AGENT, G.NAMES
ZERO = bytes(8)


@pytest.fixture(scope="module")
def tab(nf):
    with nf.FlowTable(max_entries=64) as t:
        yield t


@pytest.fixture(scope="module")
def dt(nf):
    return nf.NETWORK_EVENTS, nf.PKT_DROP


# ---------------------------------------------------------------- scripts
@pytest.fixture(scope="module")
def battery(dt):
    """The two calls (with a drops array: states 0..2; without: state 3) and, per table, the answers and the restatement's result."""
    calls = {"drops": nc.script_call(*dt, states=(0, 1, 2)), "null": nc.script_call(*dt, states=(3,))}
    tables = {"lds": nc.small_answers(), "global": nc.big_answers()}
    want = {(t, c): N.resolve(call.present, call.netev, call.drops, a) for t, a in tables.items() for c, call in calls.items()}
    return calls, tables, want


def check_scripts(got, want, call, what):
    """check_resolve, with the first flow that differs named by its script and its drops state."""
    p, d, rows, missing, over = got
    wp, wd, wrows, _, wmissing = want
    bad = np.flatnonzero((p != wp) | (rows != wrows).any(axis=1) | (d != wd).any(axis=1))
    if len(bad):
        i = int(bad[0])
        raise AssertionError("%s: %d of %d flows differ, first flow %d%s, %s:\n got present %#x rows %s drops %s\nwant present %#x rows %s drops %s" % (
            what, len(bad), call.n, i, "" if call.live[i] else " (network-events bit clear)", nc.describe(int(call.script[i]), int(call.state[i])),
            p[i], rows[i].tolist(), d[i].tobytes().hex(), wp[i], wrows[i].tolist(), wd[i].tobytes().hex()))
    E.check_resolve(got, want)


@pytest.mark.parametrize("entry", ["host", "device", "in place"])
@pytest.mark.parametrize("which", ["lds", "global"])
def test_scripts(nf, tab, battery, which, entry):
    calls, tables, want = battery
    with tab.netev_table(tables[which].items()) as t:
        assert (len(t) <= E.LDS_ROWS) == (which == "lds")
        for name, call in calls.items():
            for state in np.unique(call.state):                                        # no script is left out
                assert np.array_equal(call.script[(call.state == state) & call.live], np.arange(nc.N_SCRIPTS))
            parts = {"network_events": call.netev, "drops": call.drops}
            has = call.drops is not None
            if entry == "host":
                got = E.host_resolve(tab, t, call.present, parts, drops=has)
            else:
                got, _ = E.device_resolve(tab, t, call.present, parts, drops=has, in_place=entry == "in place")
            check_scripts(got, want[which, name], call, "%s table, %s entry, %s" % (which, entry, "drops array" if has else "no drops array"))
            assert got[3] == {nc.ck(nc.COOKIE["M"])}


# ---------------------------------------------------------------- search
def test_search_crafted_cookies(nf, O, tab, dt):
    cookies = nc.search_cookies()
    near = nc.neighbours(cookies)
    answers = nc.search_answers(cookies)
    present, ne, drops = nc.probe_flows(cookies + near, *dt)
    n = len(present)
    parts = {"network_events": ne, "drops": drops}
    with tab.netev_table(answers.items()) as t:
        want = E.check_all(nf, O, tab, t, answers, G.stream(nf, O, n, seed=21), present, parts)
    order = N.table_rows(answers)
    assert want[2][:len(cookies), 0].tolist() == [order[nc.ck(c)] for c in cookies]          # the returned row names the cookie
    assert (want[2][len(cookies):] == N.NO_ROW).all() and want[4] == {nc.ck(c) for c in near}
    # the table without 0, probed with 0 too: the all-zero cookie is missing, and its flag says so
    del answers[ZERO]
    with tab.netev_table(answers.items()) as t:
        want = E.check_all(nf, O, tab, t, answers, G.stream(nf, O, n, seed=22), present, parts, pb_too=False)
        _, zero, over = device_set(tab, t, present, ne, 64)[1:4]
    assert want[4] == {nc.ck(c) for c in near} | {ZERO} and zero and not over


@pytest.mark.parametrize("rows", nc.SIZES)
def test_search_every_row_of_spaced_tables(nf, O, tab, dt, rows):
    answers = nc.spaced_answers(rows)
    cookies = nc.spaced_cookies(rows).tolist()
    below, above = cookies[0] - 1, cookies[-1] + 1
    present, ne, drops = nc.probe_flows(cookies + [below, above], *dt)
    parts = {"network_events": ne, "drops": drops}
    want = N.resolve(present, ne, drops, answers)
    assert np.array_equal(want[2][:rows, 0], np.arange(rows)) and (want[2][rows:] == N.NO_ROW).all() and (want[2][:, 1:] == N.NO_ROW).all()
    with tab.netev_table(answers.items()) as t:
        assert len(t) == rows
        for got in (E.host_resolve(tab, t, present, parts), E.device_resolve(tab, t, present, parts)[0]):
            bad = np.flatnonzero(got[2][:rows, 0] != np.arange(rows))
            assert len(bad) == 0, "%d rows: %d probes returned another row, first: row %d gave %#x" % (rows, len(bad), bad[0], got[2][bad[0], 0])
            E.check_resolve(got, want)
            assert got[3] == {nc.ck(below), nc.ck(above)}
        if rows == nc.MAX_ROWS:
            assert want[2][rows - 1, 0] == 0xFFFE
            with pytest.raises(nf.NfaggError) as e:
                tab.netev_table(list(answers.items()) + [(nc.ck(1), b"one too many")])
            assert e.value.code == nf._lib.EINVAL
            wp, wd, wrows, events, _ = want
            for cut in (slice(0, 128), slice(rows - 128, rows)):                       # the pieces of the first and the last rows
                recs = G.stream(nf, O, 128, seed=23)
                dparts = {"drops": wd[cut].copy().view(nf.PKT_DROP).reshape(-1)}
                p, r, ev = wp[cut].copy(), wrows[cut].copy(), events[cut]
                wj = N.encode_json(recs, p, dparts, ev, NOW, MONO, G.rows(NAMES), AGENT, RECEIVED)
                G.check(tab.encode_flp_json_netev(recs, p, dparts, r, t, NOW, MONO, G.table(nf, NAMES), AGENT, RECEIVED), wj)
                G.check(E.device_encode_json(nf, tab, t, recs, p, dparts, r), wj)
                wpb = N.encode_pb(O, recs, p, dparts, ev, NOW, MONO, AGENT, E.PB_NAMES)
                E.check_pb(tab.encode_pb_netev(recs, p, dparts, r, t, NOW, MONO, AGENT, nf.intf_table(E.PB_NAMES)), wpb)
                E.check_pb(E.device_encode_pb(nf, tab, t, recs, p, dparts, r), wpb)


# ---------------------------------------------------------------- missing
def device_set(tab, table, present, ne, cap):
    """The device entry with the set's slots kept: (slots uint64[cap], n_missing, zero flag, overflow, rows)."""
    import torch
    n = len(present)
    d_p, d_ne = E.dev(present), E.dev(ne)
    d_po = torch.empty((n,), dtype=torch.uint8, device="cuda")
    d_do = torch.empty((n * 32,), dtype=torch.uint8, device="cuda")
    d_rows = torch.full((n * 4,), 0x7777, dtype=torch.int16, device="cuda")
    d_set = torch.full((cap,), -1, dtype=torch.int64, device="cuda")
    n_miss, zero, over = tab.netev_resolve_device(table, d_p.data_ptr(), d_ne.data_ptr(), 0, n, d_po.data_ptr(), d_do.data_ptr(), d_rows.data_ptr(),
                                                  d_set.data_ptr(), cap)
    torch.cuda.synchronize()
    return d_set.cpu().numpy().view(np.uint64), n_miss, zero, over, d_rows.cpu().numpy().view(np.uint16)


@pytest.mark.parametrize("cap", nc.CAPS)
def test_missing_set_on_crafted_homes(nf, tab, dt, cap):
    with tab.netev_table([]) as empty:
        for name, cookies, homes in nc.missing_cases(cap):
            what = "cap %d, %s" % (cap, name)
            present, ne, drops = nc.missing_flows(cookies, *dt)
            planted = {c for c in cookies if c}
            has_zero, over_want = 0 in cookies, len(planted) > cap
            # the device path: the zero cookie is counted and takes no slot
            slots, n_miss, zero, over, rows = device_set(tab, empty, present, ne, cap)
            stored = [int(v) for v in slots if v]
            assert (rows == N.NO_ROW).all(), what
            assert len(stored) == len(set(stored)), "%s: a cookie stored twice" % what
            assert bool(zero) == has_zero and bool(over) == over_want, what
            assert n_miss == len(stored) + has_zero, what
            if over_want:                                                            # raised only after cap occupied slots were seen
                assert len(stored) == cap and set(stored) < planted, what
            else:
                assert set(stored) == planted and n_miss == len(cookies), what
            assert nc.off_path(slots, cap) == [], "%s: stored where no probe from mix(cookie) %% cap finds it" % what
            # the host path: the zero cookie takes a place of the list, and raises overflow when there is none
            got = E.host_resolve(tab, empty, present, {"network_events": ne, "drops": drops}, cap)
            listed = {N.cookie_value(c) for c in got[3]}
            if len(cookies) > cap:
                assert got[4] and len(listed) == cap and listed <= set(cookies) and (over_want or listed == planted), what
            else:
                assert not got[4] and listed == set(cookies), what
            assert (got[2] == N.NO_ROW).all() and np.array_equal(got[0], present) and not got[1].any(), what


# ---------------------------------------------------------------- pieces
@pytest.fixture(scope="module")
def pieces(nf, O, dt):
    present, ne, drops, pick = nc.piece_flows(*dt)
    return nc.piece_answers(), G.stream(nf, O, len(present), seed=31), present, {"network_events": ne, "drops": drops}, pick


def test_pieces_of_every_length_through_both_encoders(nf, O, tab, pieces):
    answers, recs, present, parts, pick = pieces
    with tab.netev_table(answers.items()) as t:
        wp, wd, wrows, events, missing = E.check_all(nf, O, tab, t, answers, recs, present, parts)
    assert not missing and all(len(e) == 4 for e in events)
    assert [e for e in events[3]] == [nc.piece_event(nc.PIECE_T[k]) for k in pick[3]]


def test_rows_with_holes_go_straight_to_the_encoders(nf, O, tab, pieces):
    """(NO_ROW, r, NO_ROW, r'): the resolve packs its rows to the front, the encoders skip a slot on its own."""
    answers, recs, present, parts, pick = pieces
    order = N.table_rows(answers)
    row_of = np.array([order[nc.piece_cookie(t)] for t in nc.PIECE_T], dtype=np.uint16)
    rows = np.full((len(recs), 4), N.NO_ROW, dtype=np.uint16)
    rows[:, 1], rows[:, 3] = row_of[pick[:, 1]], row_of[pick[:, 3]]
    rows[5] = N.NO_ROW                                                                 # and a flow with nothing but holes
    rows[6, 3] = N.NO_ROW
    events = [[nc.piece_event(nc.PIECE_T[pick[i, k]]) for k in (1, 3) if rows[i, k] != N.NO_ROW] for i in range(len(recs))]
    dparts = {"drops": parts["drops"]}
    with tab.netev_table(answers.items()) as t:
        wj = N.encode_json(recs, present, dparts, events, NOW, MONO, G.rows(NAMES), AGENT, RECEIVED)
        G.check(tab.encode_flp_json_netev(recs, present, dparts, rows, t, NOW, MONO, G.table(nf, NAMES), AGENT, RECEIVED), wj)
        G.check(E.device_encode_json(nf, tab, t, recs, present, dparts, rows), wj)
        wpb = N.encode_pb(O, recs, present, dparts, events, NOW, MONO, AGENT, E.PB_NAMES)
        E.check_pb(tab.encode_pb_netev(recs, present, dparts, rows, t, NOW, MONO, AGENT, nf.intf_table(E.PB_NAMES)), wpb)
        E.check_pb(E.device_encode_pb(nf, tab, t, recs, present, dparts, rows), wpb)
    assert len(events[5]) == 0 and len(events[6]) == 1 and len(events[7]) == 2
