"""tests/dedupcraft.py on the CPU: the builder builds what it says (every sequence, once; distinct keys; layouts that keep each
script's order), the oracle's kernel-dedup Accounter on the families agrees with the second, independent restatement in Python,
and every family REACHES what it was built for — asserted on the oracle's output, so that a later edit of the builder cannot
silently empty a case. (That the oracle equals the reference's own flows.c on these families is tests/test_oracle_ref.py.)"""
import numpy as np
import pytest

import dedupcraft as dc
import keycraft as kc
from test_oracle_second_opinion import account, to_dict

SSL_MISMATCH = 0x01


@pytest.fixture(scope="module")
def want(O):
    """name -> (family, the oracle's flows, the script of each flow): one kernel-dedup Accounter per family, nothing evicted early."""
    cache = {}

    def get(name):
        if name not in cache:
            fam = dc.family(name)
            ev = O.run_accounter(fam.recs, 1 << 20, mode=1)
            assert len(ev) == 1 and len(ev[0][1]) == fam.n_scripts
            cache[name] = (fam, ev[0][1], fam.scripts_of(ev[0][1]))
        return cache[name]
    return get


def last_record(fam, scripts):
    """The metrics of the last record of each of these scripts."""
    return fam.recs["metrics"][fam.start[scripts] + fam.length[scripts] - 1]


# ---------------------------------------------------------------- the builder
@pytest.mark.parametrize("name", dc.EXHAUSTIVE)
def test_exhaustive_families_hold_every_sequence_once(name):
    fam = dc.family(name)
    n_sym, max_len = len(dc.SYMBOLS[name]), dc.MAX_LEN[name]
    assert fam.n_scripts == sum(n_sym ** k for k in range(1, max_len + 1))
    assert len(fam.recs) == sum(k * n_sym ** k for k in range(1, max_len + 1))
    sym = dc.symbol_numbers(fam.symbols, fam.recs)                       # from the records' fields
    strings = {"".join(dc.DIGITS[k] for k in sym[a:a + n]) for a, n in zip(fam.start, fam.length)}
    assert len(strings) == fam.n_scripts                                 # all different: with the count, every sequence exactly once
    assert {len(s) for s in strings} == set(range(1, max_len + 1))
    if name == "hello":                                                  # one length more would pass the limit
        assert sum(k * n_sym ** k for k in range(1, max_len + 2)) >= dc.MAX_RECORDS
    assert fam.describe(0).endswith("'0'")


def test_intf_family_is_the_size_the_issue_names():
    fam = dc.family("intf")
    assert (fam.n_scripts, len(fam.recs)) == (9330, 44790)


@pytest.mark.parametrize("name", dc.FAMILIES)
def test_keys_are_distinct_and_everything_else_is_plain(name):
    fam = dc.family(name)
    assert len(fam.recs) < dc.MAX_RECORDS
    assert kc.distinct_flows(fam.recs) == fam.n_scripts == len(np.unique(fam.keys, axis=0))
    raw = fam.recs.view(np.uint8).reshape(-1, 144)
    assert not raw[:, 39].any() and np.array_equal(raw[:, :39], fam.keys[fam.script, :39])
    m = fam.recs["metrics"]
    assert (m["packets"] == 1).all() and (m["bytes"] == 100).all() and (m["start"] == 1000).all()
    if name != "last":
        assert (m["end"] == 2001 + fam.pos).all()                        # increasing along every script
    if name != "capacity":
        assert not m["nb_observed_intf"].any() and not m["observed_intf"].any() and not m["observed_direction"].any()
    if name not in ("ssl", "hello"):
        assert not (m["ssl_version"].any() or m["tls_types"].any() or m["tls_cipher_suite"].any() or m["tls_key_share"].any())


def test_seeded_families_have_the_asked_shapes():
    cap, wave = dc.family("capacity"), dc.family("wave")
    assert cap.n_scripts == 2000 and cap.length.min() == 8 and cap.length.max() == 24
    first = cap.recs["metrics"][cap.start]
    assert set(first["nb_observed_intf"].tolist()) == {0, 1, 2, 3, 4, 5, 6, 7, 255}
    assert set(np.unique(first["observed_intf"]).tolist()) == set(range(1, 10)) and set(np.unique(first["observed_direction"]).tolist()) == {0, 1, 2, 3}
    assert any(len(set(row.tolist())) < 6 for row in first["observed_intf"])                   # duplicates in a list
    assert set(np.unique(cap.recs["metrics"]["direction_first_seen"]).tolist()) == {0, 1, 2, 3, 7}
    assert wave.n_scripts == 64 and (wave.length == 64).all() and (wave.start % 64 == 0).all()
    assert set(np.unique(wave.recs["metrics"]["if_index_first_seen"]).tolist()) == set(range(9))
    assert dc.family("capacity") is cap                                                        # built once


@pytest.mark.parametrize("name", dc.FAMILIES)
def test_layouts_are_permutations_that_keep_every_scripts_order(name):
    fam = dc.family(name)
    n = len(fam.recs)
    rm, bounds = dc.round_major(fam)
    for what, order in (("flow_major", dc.flow_major(fam)), ("round_major", rm), ("shuffled", dc.shuffled(fam)), ("shuffled 2", dc.shuffled(fam, 2))):
        assert np.array_equal(np.sort(order), np.arange(n)), what
        assert np.array_equal(order[np.argsort(fam.script[order], kind="stable")], np.arange(n)), what     # script by script: its own order
    assert bounds[0] == 0 and bounds[-1] == n and len(bounds) == fam.length.max() + 1
    for j in range(len(bounds) - 1):
        part = rm[bounds[j]:bounds[j + 1]]
        assert (fam.pos[part] == j).all() and np.array_equal(fam.script[part], np.nonzero(fam.length > j)[0])
    sh = dc.shuffled(fam)
    assert not np.array_equal(sh, np.arange(n)) and not np.array_equal(sh, dc.shuffled(fam, 2))
    if fam.length.max() > 1:
        assert (np.diff(fam.script[sh]) != 0).mean() > 0.9                                   # a merge: neighbours are other flows


# ---------------------------------------------------------------- a second opinion on the oracle
@pytest.mark.parametrize("name", ["intf", "capacity"])
def test_python_restatement_agrees_on_the_families(O, want, name):
    fam, flows, _ = want(name)
    entries = account(fam.recs, 1 << 20, True)
    assert [r for r, _ in entries] == ["closing"] and len(entries[0][1]) == len(flows)
    for rec in flows:
        d = entries[0][1][rec["id"].tobytes()[:39]]
        g = to_dict(rec["metrics"])
        assert g == d, (fam.describe(fam.script_of_key(rec["id"].tobytes())), {k: (g[k], d[k]) for k in g if g[k] != d[k]})


# ---------------------------------------------------------------- the families reach what they were built for
def test_intf_reaches_zero_first_interface_both_and_ignored_records(want):
    fam, flows, scripts = want("intf")
    m = flows["metrics"]
    assert (m["if_index_first_seen"] == 0).any()                                               # F = 0: interface 0 is the counted one
    assert (m["observed_direction"] == 3).any()                                                # the merge to BOTH
    last = last_record(fam, scripts)
    ignored = m["end"] != last["end"]                                                          # end is the last record's unless it was ignored
    assert ignored.any() and (last["if_index_first_seen"][ignored] == 0).all() and (m["if_index_first_seen"][ignored] != 0).all()
    assert (m["nb_observed_intf"] <= 2).all() and (m["nb_observed_intf"] == 2).any()           # F = 0 with side records on 1 and 2


def test_capacity_fills_the_list_in_both_halves(want):
    fam, flows, scripts = want("capacity")
    m = flows["metrics"]
    half = scripts % 2
    assert [p["half"] for p in fam.info["plans"][:2]] == [0, 1]
    full = m["nb_observed_intf"] == 6
    last_side_absent = np.zeros(len(flows), dtype=bool)
    for i, s in enumerate(scripts):
        r = fam.records_of(s)["metrics"]
        side = r["if_index_first_seen"][1:][(r["if_index_first_seen"][1:] != r["if_index_first_seen"][0]) & (r["if_index_first_seen"][1:] != 0)]
        last_side_absent[i] = len(side) > 0 and side[-1] not in m["observed_intf"][i][:min(int(m["nb_observed_intf"][i]), 6)]
    for h in (0, 1):
        assert (full & (half == h)).sum() > 100, "half %d" % h
        assert (full & (half == h) & last_side_absent).sum() > 20, "half %d" % h
    # "listed": the sixth distinct side interface still found room (it is the flow's seventh distinct interface, counting F)
    listed_sixth = 0
    for i in np.nonzero(full & (half == 0))[0]:
        r = fam.records_of(scripts[i])["metrics"]
        F, nb0 = int(r["if_index_first_seen"][0]), int(r["nb_observed_intf"][0])
        seen = []
        for x in r["if_index_first_seen"][1:]:
            if x != F and x != 0 and x not in seen:
                seen.append(int(x))
        listed_sixth += nb0 < 6 and len(seen) >= 6 and m["observed_intf"][i][5] == seen[5]
    assert listed_sixth > 20
    # "between": X is in the list with its first direction only, although its other direction arrived later
    between = 0
    for i in np.nonzero(full & (half == 1))[0]:
        p = fam.info["plans"][scripts[i]]
        at = np.nonzero(m["observed_intf"][i] == p["X"])[0]
        between += len(at) > 0 and m["observed_direction"][i][at[0]] == p["d1"]
    assert between > 100


def test_ssl_reaches_mismatch_and_its_absence_with_two_versions(want):
    fam, flows, scripts = want("ssl")
    mismatch = (flows["metrics"]["misc_flags"] & SSL_MISMATCH) != 0
    two, counted_two = np.zeros(len(flows), dtype=bool), np.zeros(len(flows), dtype=bool)
    for i, s in enumerate(scripts):
        r = fam.records_of(s)["metrics"]
        v, on_f = r["ssl_version"], r["if_index_first_seen"] == r["if_index_first_seen"][0]
        two[i] = len(set(v[v != 0].tolist())) == 2
        counted_two[i] = len(set(v[on_f & (v != 0)].tolist())) == 2
    assert (mismatch & two).any() and (~mismatch & two).any()
    assert np.array_equal(mismatch, counted_two)                 # set exactly when COUNTED records carried both; a side record's version is ignored
    assert (~mismatch & two & ~counted_two).sum() == (~mismatch & two).sum() > 100


def test_hello_and_last_keep_values_that_are_not_the_last_records(want):
    fam, flows, scripts = want("hello")
    m, last = flows["metrics"], last_record(fam, scripts)
    assert (m["tls_cipher_suite"] != last["tls_cipher_suite"]).sum() > 100 and (m["tls_key_share"] != last["tls_key_share"]).sum() > 100
    first = fam.recs["metrics"][fam.start[scripts]]
    kept = (first["tls_types"] == 1) & (first["tls_cipher_suite"] != 0) & (m["tls_cipher_suite"] == first["tls_cipher_suite"]) & (fam.length[scripts] > 1)
    assert kept.any()                                            # a first record that is no server hello keeps its own cipher suite
    assert (m["tls_types"] != 3).any() and (m["tls_types"] == 3).any()
    fam, flows, scripts = want("last")
    m, last = flows["metrics"], last_record(fam, scripts)
    assert (m["end"] == last["end"]).all()                       # end: the last record of either role (no interface 0 here)
    assert (m["dscp"] != last["dscp"]).sum() > 100 and (m["sampling"] != last["sampling"]).sum() > 100
    back = np.array([fam.records_of(s)["metrics"]["end"].max() for s in scripts])
    assert (m["end"] < back).any() and (m["end"] == 0).any()     # end went backwards, and to zero
    assert ((m["dscp"] == 0) & np.array([fam.records_of(s)["metrics"]["dscp"].any() for s in scripts])).any()   # "last value, zero included"
