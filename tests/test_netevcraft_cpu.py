"""tests/netevcraft.py on the CPU: the batteries are what they claim. Every symbol in every slot and all 10^4 scripts once per drops
state; the saturation sums reached by the arithmetic of the restatement itself (tests/netev_ref.py, which tests/golden/netev_vectors.json
pins: there is no second model of the loop here); both tables with the ten answers where they were designed to be; the hash
restatement on splitmix64's first two outputs and its inverse; the crafted homes for every capacity; the piece lengths through
nfagg_netev_render; every family's table through the host-only nfagg_netev_table_create, the 65 536-row one refused."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import netev_ref as N  # noqa: E402
import netevcraft as nc  # noqa: E402


@pytest.fixture(scope="module")
def dt(nf):
    return nf.NETWORK_EVENTS, nf.PKT_DROP


@pytest.fixture(scope="module")
def calls(dt):
    return nc.script_call(*dt, states=(0, 1, 2)), nc.script_call(*dt, states=(3,))


# ---------------------------------------------------------------- scripts
def test_every_script_once_per_state_and_every_symbol_in_every_slot(calls):
    both, null = calls
    assert both.drops is not None and null.drops is None
    seen = set()
    for c in calls:
        for state in np.unique(c.state):
            m = (c.state == state) & c.live
            assert np.array_equal(c.script[m], np.arange(nc.N_SCRIPTS)), state
            seen.add(int(state))
        assert abs(8 * int((~c.live).sum()) - c.n) <= 4 * len(np.unique(c.state))      # one flow in eight carries a script for nothing
        assert not (c.present[~c.live] & nc.FEAT_NETEV).any() and (c.present[c.live] & nc.FEAT_NETEV).all()
        cookies = c.netev["network_events"].copy().view("<u8").reshape(c.n, 4)
        sym = nc.script_symbols(c.script)
        for k in range(4):
            assert set(sym[:, k].tolist()) == set(range(10))
            for s, name in enumerate(nc.SYMBOLS):
                m = sym[:, k] == s
                assert (cookies[m, k] == nc.COOKIE[name]).all()
                assert (c.netev["packets"][m, k] == 0).all() == (name == "Z")
        at = (c.script[:, None] + np.arange(4)) % 4
        assert np.array_equal(c.netev["bytes"], nc.COUNTS[at])
        assert np.array_equal(c.netev["packets"][sym != 0], nc.COUNTS[3 - at][sym != 0])
    assert seen == {0, 1, 2, 3}
    has = (both.present & nc.FEAT_DROPS) != 0
    assert not has[both.state == 0].any() and has[both.state != 0].all()
    has3 = (null.present & nc.FEAT_DROPS) != 0                                          # no array: the bit says nothing, so it takes both values
    assert has3.any() and not has3.all()
    d = both.drops
    assert (d["bytes"][both.state == 2] == 0xFFFE).all() and (d["packets"][both.state == 2] == 0xFFFF).all()
    small = d[both.state == 1]
    assert (small["bytes"] == 1).all() and (small["packets"] == 1).all() and (small["latest_drop_cause"] == 7).all()
    assert (small["latest_flags"] == 0x12).all() and (small["latest_state"] == 3).all() and len(np.unique(small["pad_"], axis=0)) > 1000


def test_symbols_are_what_the_table_of_the_issue_says():
    a = nc.small_answers()
    ev = lambda s: a[nc.ck(nc.COOKIE[s])]                                               # noqa: E731
    assert len(a) == 10 and nc.ck(nc.COOKIE["M"]) not in a and ev("U") is None
    assert N.event_string(ev("A1")) == N.event_string(ev("A2")) == N.event_string(ev("D3")) == nc.S1.encode()
    assert N.event_string(ev("D1")) == N.event_string(ev("D2")) == N.event_string(ev("T2")) == nc.S2.encode()
    assert N.event_string(ev("T")) == nc.S3.encode() and not N.is_acl(ev("T")) and not N.is_acl(ev("T2"))
    assert [N.drop_cause(ev(s)) for s in ("A1", "A2", "T", "T2")] == [0] * 4
    assert N.drop_cause(ev("D1")) == (1 << 24) + N.CAUSES.index("NetworkPolicy") > 1 << 24
    assert N.drop_cause(ev("D2")) == 1 << 24 and N.drop_cause(ev("D3")) == (1 << 24) + N.CAUSES.index("EgressFirewall") > 1 << 24
    assert N.drop_cause(ev("Z")) > 1 << 24 and N.to_map(ev("A1")) != N.to_map(ev("A2"))
    assert nc.COOKIE["A2"] < nc.COOKIE["D3"] < nc.COOKIE["A1"] and nc.COOKIE["T2"] < nc.COOKIE["D2"] < nc.COOKIE["D1"]
    assert nc.COOKIE["A1"] & 0xFFFFFFFF == nc.COOKIE["A2"] & 0xFFFFFFFF and nc.COOKIE["A2"] >> 32 == nc.COOKIE["D3"] >> 32
    assert nc.COOKIE["M"] & 0xFFFFFFFF == nc.COOKIE["T2"] & 0xFFFFFFFF and nc.COOKIE["M"] + 1 == nc.COOKIE["X"]


@pytest.mark.parametrize("which", ["lds", "global"])
def test_tables_place_the_ten_answers_as_designed(nf, which):
    answers = nc.small_answers() if which == "lds" else nc.big_answers()
    rows = N.table_rows(answers)
    ten = sorted(rows[nc.ck(nc.COOKIE[s])] for s in nc.EVENT)
    with nf.NetevTable(answers.items()) as t:
        assert t.cookies == sorted(answers, key=N.cookie_value)
    r = lambda s: rows[nc.ck(nc.COOKIE[s])]                                            # noqa: E731
    assert r("T") == 0                                                                  # class number 0 is a row the scripts meet
    assert r("A2") < r("D3") < r("A1") and r("T2") < r("D2") < r("D1")                   # the class's first row is not the plain one
    if which == "lds":
        assert len(answers) == 10 <= nc.LDS_ROWS and ten == list(range(10))
    else:
        assert len(answers) >= 310 > nc.LDS_ROWS
        # a filler between any two of them, but for A1 and D1, whose cookies are consecutive numbers
        assert [a for a, b in zip(ten, ten[1:]) if b - a == 1] == [r("A1")] and r("D1") == r("A1") + 1
        fill = [v for c, v in answers.items() if c not in nc.small_answers()]
        assert sum(v is None for v in fill) > 90 and sum(isinstance(v, bytes) for v in fill) > 90 and sum(isinstance(v, tuple) for v in fill) > 90
        assert nc.ck(nc.COOKIE["M"] - 1) in answers and nc.ck(nc.COOKIE["M"]) not in answers


def test_saturation_sums_are_reached_by_the_restatement(calls, monkeypatch):
    """0x8000 + 0x8000, 0xFFFF + 1, 0x7FFF + 0x8000 and the full part's 0xFFFE / 0xFFFF + anything, as netev_ref.add_u16 sees them;
    an injected first drop, a last cause that differs from the first, a suppressed event that still injects."""
    pairs = set()
    real = N.add_u16

    def spy(a, b):
        pairs.add((a, b))
        return real(a, b)

    monkeypatch.setattr(N, "add_u16", spy)
    both, null = calls
    answers = nc.small_answers()
    p, d, rows, events, missing = N.resolve(both.present, both.netev, both.drops, answers)
    p3, d3, _, events3, missing3 = N.resolve(null.present, null.netev, None, answers)
    either = lambda a, b: (a, b) in pairs or (b, a) in pairs                            # noqa: E731
    assert either(0x8000, 0x8000) and either(0xFFFF, 1) and either(0x7FFF, 0x8000) and either(0xFFFE, 1) and either(0xFFFE, 0xFFFF)
    assert missing == missing3 == {nc.ck(nc.COOKIE["M"])}
    for c, pp, ee in ((both, p, events), (null, p3, events3)):
        assert not any(ee[i] for i in np.flatnonzero(~c.live)[:200]) and np.array_equal(pp[~c.live] & ~np.uint8(4), c.present[~c.live] & ~np.uint8(4))
    assert max(len(e) for e in events) == 3 and (rows[:, 3] == N.NO_ROW).all()          # three String()s besides the skipped ones
    cause = d.view("<u4")[:, 5]
    made = (both.state == 0) & ((p & nc.FEAT_DROPS) != 0)
    assert made.any() and set(cause[made].tolist()) == {1 << 24, (1 << 24) + 1, (1 << 24) + 4}
    assert (d3[(p3 & nc.FEAT_DROPS) == 0] == 0).all() and ((p3 & nc.FEAT_DROPS) != 0).any()
    # D1 after T2: no event of its own, the drop still injected
    s = int("".join(str(nc.SYMBOLS.index(k)) for k in ("T2", "D1", "U", "M")))
    i = int(np.flatnonzero((both.script == s) & both.live & (both.state == 0))[0])
    assert events[i] == [nc.EVENT["T2"]] and cause[i] == (1 << 24) + 4


# ---------------------------------------------------------------- search
def test_search_tables(nf):
    cookies = nc.search_cookies()
    assert set(nc.EDGES) <= set(cookies) and len(cookies) == 9 + 9 + 6
    lo, hi = {}, {}
    for c in cookies:
        lo.setdefault(c & 0xFFFFFFFF, []).append(c)
        hi.setdefault(c >> 32, []).append(c)
    assert sum(len(v) > 1 for v in lo.values()) >= 4 and sum(len(v) > 1 for v in hi.values()) >= 4
    near = nc.neighbours(cookies)
    assert not set(near) & set(cookies) and 2 in near and (1 << 63) + 1 in near and nc.M64 - 2 in near and len(near) <= 60
    answers = nc.search_answers(cookies)
    assert len({N.event_string(e) for e in answers.values()}) == len(cookies)
    with nf.NetevTable(answers.items()) as t:
        assert len(t) == len(cookies) and t.cookies[0] == bytes(8) and t.cookies[-1] == b"\xff" * 8
    present, ne, drops = nc.probe_flows(cookies + near, nf.NETWORK_EVENTS, nf.PKT_DROP)
    live = ne["packets"] != 0
    assert (live.sum(axis=1) == 1).all() and set(np.argmax(live, axis=1).tolist()) == {0, 1, 2, 3}
    assert [int(v) for v in ne["network_events"].copy().view("<u8").reshape(-1, 4)[live]] == cookies + near


@pytest.mark.parametrize("rows", nc.SIZES)
def test_spaced_tables(nf, rows):
    c = nc.spaced_cookies(rows)
    assert len(c) == rows and c[0] > 0 and c[-1] < nc.M64 and (rows == 1 or (np.diff(c) == c[0]).all())
    answers = nc.spaced_answers(rows)
    assert len({N.event_string(e) for e in answers.values()}) == (rows if rows <= 1025 else 1)
    with nf.NetevTable(answers.items()) as t:
        assert len(t) == rows
    if rows == nc.MAX_ROWS:
        assert rows - 1 == 0xFFFE == N.NO_ROW - 1
        with pytest.raises(nf.NfaggError) as e:
            nf.NetevTable(list(answers.items()) + [(nc.ck(1), b"one too many")])
        assert e.value.code == nf._lib.EINVAL and "65536" in str(e.value)


# ---------------------------------------------------------------- missing
def test_hash_restatement_on_splitmix64s_first_outputs():
    g = 0x9E3779B97F4A7C15
    assert nc.mix(g) == 0xE220A8397B1DCDAF and nc.mix((2 * g) & nc.M64) == 0x6E789E6AA1B965F4
    assert nc.mix(0) == 0 == nc.unmix(0)
    for v in np.random.default_rng(9).integers(0, nc.M64, 1000, dtype=np.uint64).tolist() + [1, nc.M64]:
        assert nc.mix(nc.unmix(v)) == v and nc.unmix(nc.mix(v)) == v


@pytest.mark.parametrize("cap", nc.CAPS)
def test_crafted_homes(nf, cap):
    names = []
    for name, cookies, homes in nc.missing_cases(cap):
        names.append(name.split(" ")[0])
        assert len(set(cookies)) == len(cookies) == len(homes)
        for c, h in zip(cookies, homes):
            assert (c == 0 and h is None) or (c != 0 and nc.mix(c) % cap == h)
        if name.startswith("one_home"):
            assert len(set(homes)) == 1 and cap - len(homes) in (0, 1, len(homes), len(homes) + 1)    # cap = m, m + 1, 2m (2m + 1: an odd cap)
        if name == "wrap":
            assert set(homes) == {(cap - 2) % cap, cap - 1} and (cap < 6 or len(homes) == 6)      # slots cap - 2 .. 3: through slot 0
        if name == "exact":
            assert len(cookies) == cap
        if name == "exact + 1":
            assert len(cookies) == cap + 1
        if name.startswith("zero"):
            assert cookies.count(0) == 1 and len(cookies) == cap + (name == "zero beside full")
        present, ne, drops = nc.missing_flows(cookies, nf.NETWORK_EVENTS, nf.PKT_DROP)
        flat = ne["network_events"].copy().view("<u8").reshape(-1, 4)
        live = ne["packets"] != 0
        for c in cookies[:5] + cookies[-2:]:
            at = np.flatnonzero(((flat == c) & live).any(axis=1))
            assert len(at) >= 65 and len(set((at // 256).tolist())) >= (3 if len(cookies) <= 256 else 2) and ((flat[at] == c) & live[at]).all(axis=1).sum() == 1
        assert set(flat[live].tolist()) == set(cookies)
    assert set(names) == {"one_home", "wrap", "exact", "zero"}


def test_off_path_tells_a_misplaced_cookie():
    cap = 7
    (a, b) = nc.cookies_at([5, 5], cap, np.random.default_rng(1))
    slots = [0] * cap
    slots[5], slots[6] = a, b
    assert nc.off_path(slots, cap) == []
    slots[6], slots[0] = 0, b                                                           # a hole before it
    assert nc.off_path(slots, cap) == [(0, b)]
    slots[6] = nc.cookies_at([6], cap, np.random.default_rng(2))[0]
    assert nc.off_path(slots, cap) == []                                                # the chain runs through slot 0
    slots[4], slots[5] = a, 0                                                           # below its home
    assert (4, a) in nc.off_path(slots, cap)


# ---------------------------------------------------------------- pieces
def test_piece_lengths_through_the_library(nf):
    js, pb = {}, {}
    for t in nc.PIECE_T:
        ev = nc.piece_event(t)
        js[t], pb[t] = nf.netev_render(ev, nf._lib.NETEV_JSON), nf.netev_render(ev, nf._lib.NETEV_PB)
        assert js[t] == N.render_json(ev) and pb[t] == N.render_pb(ev)
        assert len(js[t]) == 14 + t and len(pb[t]) == nc.piece_pb_len(t)
        assert len(ev) == (t if t != nc.T_CAP else t - 1)
    assert set(nc.PIECE_T) == set(range(141)) | set(range(484, 499)) and len(set(map(nc.piece_event, nc.PIECE_T))) == len(nc.PIECE_T)
    jl, pl = [len(v) for v in js.values()], [len(v) for v in pb.values()]
    for lens in (jl, pl):
        assert {127, 128, 512} <= set(lens) and max(lens) == 512
        assert all(sum(v % 16 == r for v in lens) >= 3 for r in range(16))              # every residue, several times
    # the protobuf piece across 127 / 128 in its value length, its entry length and its whole length
    assert pb[127][12:14] == b"\x12\x7f" and pb[128][12:15] == b"\x12\x80\x01"
    assert pb[116][:2] == b"\x0a\x7f" and pb[117][:3] == b"\x0a\x80\x01" and (len(pb[114]), len(pb[115])) == (127, 128)
    assert [t for t in nc.PIECE_T if len(js[t]) == 512] == [498] and [t for t in nc.PIECE_T if len(pb[t]) == 512] == [497, 498]
    with pytest.raises(nf.NfaggError):                                                  # why 498 is not 498 plain bytes
        nf.netev_render(b"m" * 498, nf._lib.NETEV_PB)
    with nf.NetevTable(nc.piece_answers().items()) as t:
        assert len(t) == len(nc.PIECE_T)
    present, ne, drops, pick = nc.piece_flows(nf.NETWORK_EVENTS, nf.PKT_DROP)
    assert len(present) == 64 * 3 + 5 and (ne["packets"] == 1).all()
    for slot in range(4):                                                               # every length starts at every place of a line
        assert {nc.PIECE_T[k] for k in pick[:, slot]} == set(nc.PIECE_T)
