"""Writes conntrack_crafted.json beside itself (data only; run once, by hand: `python gen_conntrack_crafted.py`, about a minute).
The searches are those of tests/conncraft.py; every tuple written is hashed again HERE with the plain byte-by-byte FNV-64a.

  same_home    200 connections of the space of conntrack_collisions.json (10.1.2.3 -> 10.9.8.7, 2 048 x 2 048 ports from 1024 on,
               TCP) whose home slot in the smallest table (1 024 slots) is `home_slot`, the most crowded one
  wrap_1024    40 connections of that space whose home is one of the last three slots of the 1 024-slot table
  wrap_8192    30 whose home is one of the last three slots of the 8 192-slot table
  same_word0   pairs of connections whose totals share the upper 32 bits (the table's first key word) and the 1 024-slot home,
               from 2^25 tuples of 8 x 4 addresses 10.101.102.x -> 10.201.202.y and 1 024 x 1 024 ports, TCP
  candidates   how many the searches found of each kind"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import conncraft as cc  # noqa: E402
import conntrack_streams as ST  # noqa: E402


def recheck(t, slots=1024):
    total = cc.plain_hashes(t["src"], t["sport"], t["dst"], t["dport"], t["proto"])[2]
    assert "%x" % total == t["total"] and ST.home_slot(total, slots) == t["home"], t
    return total


if __name__ == "__main__":
    homes, word0 = cc.search_homes(), cc.search_word0()
    assert len(homes["same_home"]) == 200 and len(homes["wrap_1024"]) == 40 and len(homes["wrap_8192"]) == 30 and len(word0["pairs"]) >= 16
    assert all(recheck(t) % 1024 >= 0 and t["home"] == homes["home_slot"] for t in homes["same_home"])
    assert all(recheck(t) >= 0 and t["home"] >= 1021 for t in homes["wrap_1024"])
    assert all(recheck(t, 8192) >= 0 and t["home"] >= 8189 for t in homes["wrap_8192"])
    for a, b in word0["pairs"]:
        ta, tb = recheck(a), recheck(b)
        assert ta != tb and ta >> 32 == tb >> 32 and a["home"] == b["home"]
    out = dict(searched=homes["searched"], home_slot=homes["home_slot"], same_home=homes["same_home"], wrap_1024=homes["wrap_1024"],
               wrap_8192=homes["wrap_8192"], searched_word0=word0["searched"], same_word0=word0["pairs"],
               candidates=dict(homes["candidates"], same_word0=word0["candidates"]))
    json.dump(out, open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "conntrack_crafted.json"), "w"), indent=1)
    print(out["candidates"])
