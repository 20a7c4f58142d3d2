"""Grouped aggregates (``POST .../aggregate``): one answer on every execution path.

``brute`` below is the oracle: a loop over the documents written from the route's description
(group, count, histogram of the key's values, then the aggregate formulas), sharing only the
primitives ``get_path`` / ``vkey`` / ``compare`` with the code under test.  Against it: the
semantics function ``reduce_hist``, ``ColumnarIndex.aggregate`` on the CPU, the route on both
backing fronts with the accelerator off (native engine + document walk) and on the CPU mirror,
the two-shard merge against one store, and -- marked ``gpu`` -- the fused HIP kernel path.
"""
import asyncio
import functools
import json
import math
import random

import pytest

from aca_dotnet_workshop_amd.backing.client import BackingClient, BackingError
from aca_dotnet_workshop_amd.backing.shards import ShardedBackingClient
from aca_dotnet_workshop_amd.ops import columnar
from aca_dotnet_workshop_amd.ops.columnar import ColumnarIndex, compare, get_path, vkey

from helpers import run
from test_backing_front import FRONTS, Backing
from test_shards import backings  # noqa: F401  (fixture: three CPU-mirror shards and one plain store)

MISSING = columnar._MISSING


# ------------------------------------------------------------------ the oracle
def _num(v):
    return isinstance(v, (int, float)) and not isinstance(v, bool)


def _canon(v):
    if not _num(v):
        return v
    f = float(v) + 0.0
    return int(f) if f.is_integer() and abs(f) < 2.0 ** 53 else f


def _order(a, b):
    for x, y in zip(a, b):
        c = (y is MISSING) - (x is MISSING) if x is MISSING or y is MISSING else compare(x, y)
        if c:
            return c
    return 0


def brute(docs, q, prefix="", hist=False):
    """``docs``: {key: document}.  The response of the aggregate route."""
    gb, aggs, flt = q.get("groupBy") or [], q.get("aggregate") or [], q.get("filter")
    groups = {}
    if not gb:
        groups[()] = {"vals": (), "count": 0, "h": {}}
    for key, d in docs.items():
        if not key.startswith(prefix) or not _match(d, flt):
            continue
        vals = tuple(get_path(d, p) for p in gb)
        g = groups.setdefault(tuple(None if v is MISSING else vkey(v) for v in vals),
                              {"vals": tuple(v if v is MISSING else _canon(v) for v in vals), "count": 0, "h": {}})
        g["count"] += 1
        for k in dict.fromkeys(a["key"] for a in aggs if "key" in a):
            v = get_path(d, k)
            if v is not MISSING:
                e = g["h"].setdefault(k, {}).setdefault(vkey(v), [_canon(v), 0])
                e[1] += 1
    out = []
    for g in sorted(groups.values(), key=functools.cmp_to_key(lambda a, b: _order(a["vals"], b["vals"]))):
        o = {"group": {p: v for p, v in zip(gb, g["vals"]) if v is not MISSING}, "count": g["count"]}
        if hist:
            o["hist"] = {k: sorted(map(list, g["h"].get(k, {}).values()),
                                   key=functools.cmp_to_key(lambda a, b: compare(a[0], b[0])))
                         for k in dict.fromkeys(a["key"] for a in aggs if "key" in a)}
            out.append(o)
            continue
        o["aggregates"] = res = []
        for a in aggs:
            op = a["op"].upper()
            if "key" not in a:
                res.append({"op": op, "value": g["count"]})
                continue
            pairs = list(g["h"].get(a["key"], {}).values())
            nums = [(v, c) for v, c in pairs if _num(v)]
            if op == "COUNT":
                val = sum(c for _, c in pairs)
            elif op in ("SUM", "AVG"):
                if not nums:
                    continue
                val = math.fsum(float(v) * c for v, c in nums)
                if op == "AVG":
                    val /= sum(c for _, c in nums)
            else:
                if not pairs:
                    continue
                pick = min if op == "MIN" else max
                val = pick((v for v, _ in pairs), key=functools.cmp_to_key(compare))
            res.append({"op": op, "key": a["key"], "value": val})
        out.append(o)
    return {"groups": out}


def _match(d, f):
    if not f:
        return True
    (op, arg), = f.items()
    op = op.upper()
    if op == "AND":
        return all(_match(d, x) for x in arg)
    if op == "OR":
        return any(_match(d, x) for x in arg)
    (path, val), = arg.items()
    v = get_path(d, path)
    if op == "EQ":
        return v is not MISSING and vkey(v) == vkey(val)
    if op == "NEQ":
        return v is MISSING or vkey(v) != vkey(val)
    if op == "IN":
        return v is not MISSING and vkey(v) in {vkey(x) for x in val}
    if v is MISSING or columnar.type_rank(v) != columnar.type_rank(val):
        return False
    c = compare(v, val)
    return {"GT": c > 0, "GTE": c >= 0, "LT": c < 0, "LTE": c <= 0}[op]


def _docs(n, seed=5):
    """Documents with missing paths, nulls, numbers equal as int and as float, bools, strings,
    a nested path and sums that cancel catastrophically unless added exactly."""
    rng = random.Random(seed)
    out = {}
    for i in range(n):
        d = {"who": f"user{rng.randrange(7)}", "done": rng.random() < 0.4, "i": i,
             "pts": rng.choice([1, 1.0, 2, 2.5, -3, 0, -0.0, 1e16, -1e16, 0.1, None, "n/a", True])}
        if rng.random() < 0.8:
            d["team"] = rng.choice(["red", "blue", None, 3, 3.0, False])
        if rng.random() < 0.7:
            d["meta"] = {"prio": rng.choice([1, 2, 3, "high", None])}
        if rng.random() < 0.1:
            del d["pts"]
        out[f"{'a' if i % 3 else 'b'}||k{i:05d}"] = d
    return out


QUERIES = [
    {"groupBy": ["who"], "aggregate": [{"op": "COUNT"}]},
    {"filter": {"EQ": {"done": False}}, "groupBy": ["who"],
     "aggregate": [{"op": "COUNT"}, {"op": "MIN", "key": "i"}, {"op": "MAX", "key": "pts"}, {"op": "SUM", "key": "pts"}]},
    {"filter": {"LT": {"i": 1500}}, "groupBy": ["team", "meta.prio"],
     "aggregate": [{"op": "AVG", "key": "pts"}, {"op": "COUNT", "key": "pts"}, {"op": "sum", "key": "i"},
                   {"op": "MIN", "key": "team"}]},
    {"filter": {"OR": [{"NEQ": {"team": "red"}}, {"GTE": {"pts": 2}}]}, "groupBy": [],
     "aggregate": [{"op": "SUM", "key": "pts"}, {"op": "AVG", "key": "pts"}, {"op": "MAX", "key": "meta.prio"},
                   {"op": "MIN", "key": "nowhere"}, {"op": "COUNT", "key": "nowhere"}]},
    {"filter": {"EQ": {"who": "nobody"}}, "groupBy": ["team"], "aggregate": [{"op": "COUNT"}]},
    {"filter": {"EQ": {"who": "nobody"}}, "aggregate": [{"op": "SUM", "key": "pts"}]},
    {"groupBy": ["pts", "done"]},
]
BAD = [{"groupBy": ["a", "b", "c"]}, {"aggregate": [{"op": "MEDIAN", "key": "a"}]}, {"aggregate": [{"op": "SUM"}]},
       {"groupBy": ["\x00keyprefix"]}, {"aggregate": [{"op": "MIN", "key": "\x00x"}]}, [1, 2],
       {"filter": {"EQ": {"a": 1, "b": 2}}, "groupBy": ["a"]}, {"filter": {"BETWEEN": {"a": 1}}}]


# ------------------------------------------------------------------ semantics
def test_reduce_hist_cases():
    ops = ["COUNT", "SUM", "AVG", "MIN", "MAX"]
    mixed = [("b", 2), (None, 1), (3, 4), (True, 5), (2.5, 2), ([1], 1), ({"a": 1}, 1)]
    assert columnar.reduce_hist(mixed, ops) == {"COUNT": 16, "SUM": 17.0, "AVG": (17.0, 6), "MIN": None,
                                                "MAX": {"a": 1}}
    # no numeric value: SUM and AVG are left out; bool is not a number
    assert columnar.reduce_hist([("x", 3), (True, 2), (None, 1)], ops) == {"COUNT": 6, "MIN": None, "MAX": "x"}
    assert columnar.reduce_hist([(True, 2), (False, 1)], ["SUM", "AVG", "MAX"]) == {"MAX": True}
    assert columnar.reduce_hist([], ops) == {"COUNT": 0}
    assert columnar.reduce_hist([(7, 0)], ops) == {"COUNT": 0}  # a value no row holds is not there
    # correctly rounded whatever the order: a left-to-right float sum gives 0.0 or 2.0 here
    pairs = [(1e16, 1), (1.0, 1), (-1e16, 1), (1.0, 1)]
    for perm in ([0, 1, 2, 3], [1, 3, 0, 2], [0, 2, 1, 3], [3, 2, 1, 0]):
        assert columnar.reduce_hist([pairs[i] for i in perm], ["SUM", "AVG"]) == {"SUM": 2.0, "AVG": (2.0, 4)}
    assert columnar.reduce_hist([(0.1, 3)], ["SUM"]) == {"SUM": math.fsum([0.1 * 3])}


def test_parse_aggregate_rejects():
    for q in BAD[:6]:
        with pytest.raises(ValueError):
            columnar.parse_aggregate(q)
    spec = columnar.parse_aggregate({"aggregate": [{"op": "min", "key": "a"}, {"op": "COUNT"}, {"op": "MAX", "key": "a"}]})
    assert spec.aggs == [("MIN", "a"), ("COUNT", None), ("MAX", "a")] and spec.keys == ["a"] and spec.group_by == []


@pytest.fixture(scope="module")
def docs():
    return _docs(3000)


@pytest.fixture(scope="module")
def index(docs):
    ix = ColumnarIndex()
    ix.bulk_load(docs.items())
    return ix


@pytest.mark.parametrize("qi", range(len(QUERIES)))
def test_columnar_aggregate_cpu_matches_brute_force(index, docs, qi):
    q = QUERIES[qi]
    want = brute(docs, q)
    assert index.aggregate(q) == want
    assert index.aggregate(q, hist=True) == brute(docs, q, hist=True)
    if qi == 1:
        assert len(want["groups"]) == 7 and all(len(g["aggregates"]) == 4 for g in want["groups"])
    if qi == 2:  # the {} group, the null group and the int == float group are all there
        gs = [g["group"] for g in want["groups"]]
        assert {} in gs and {"team": None, "meta.prio": None} in gs and {"team": 3, "meta.prio": "high"} in gs
    if qi == 4:
        assert want == {"groups": []}
    if qi == 5:
        assert want == {"groups": [{"group": {}, "count": 0, "aggregates": []}]}


def test_columnar_aggregate_sparse_key_space(index, docs, monkeypatch):
    """More cells than the host counts densely: the same answer through the sparse count."""
    monkeypatch.setattr(ColumnarIndex, "HOST_MAX_CELLS", 16)
    q = {"groupBy": ["who", "team"], "aggregate": [{"op": "MAX", "key": "i"}, {"op": "AVG", "key": "pts"}]}
    assert index.aggregate(q) == brute(docs, q)


# ------------------------------------------------------------------ the route
ACCT, DB = "acct", "db"


async def _agg(c, coll, q, prefix="", hist=False):
    body = q if isinstance(q, bytes) else json.dumps(q).encode()
    return json.loads(await c.doc_aggregate(ACCT, DB, coll, body, prefix, hist))


async def _load(c, coll, docs):
    items = [{"key": k, "value": json.dumps(v)} for k, v in docs.items()]
    for lo in range(0, len(items), 200):
        await c.doc_bulk_set(ACCT, DB, coll, items[lo:lo + 200])


@pytest.mark.parametrize("mode", ["off", "cpu"])
@pytest.mark.parametrize("front", FRONTS)
def test_aggregate_route_matches_brute_force(front, mode, monkeypatch):
    monkeypatch.setenv("TT_QUERY_ACCEL", mode)
    monkeypatch.setenv("TT_QUERY_ACCEL_MIN_DOCS", "1")
    docs = _docs(500, seed=9)

    async def main():
        async with Backing(front, monkeypatch) as b:
            c = BackingClient(b.base, identity="x")
            try:
                await _load(c, "c", docs)
                for q in QUERIES:
                    assert await _agg(c, "c", q) == brute(docs, q), q
                    assert await _agg(c, "c", q, "b||") == brute(docs, q, "b||"), q
                # written and deleted after the mirror was built: the next answer has them
                late = {f"b||late{i}": {"who": "user1", "done": False, "i": 10_000 + i, "pts": 0.25} for i in range(40)}
                await _load(c, "c", late)
                docs.update(late)
                for k in list(docs)[5:60]:
                    assert await c.doc_delete(ACCT, DB, "c", k)
                    del docs[k]
                for q in QUERIES[:4]:
                    assert await _agg(c, "c", q) == brute(docs, q), q
                    assert await _agg(c, "c", q, "b||", hist=True) == brute(docs, q, "b||", hist=True), q
                for q in BAD:
                    with pytest.raises(BackingError) as e:
                        await _agg(c, "c", q)
                    assert e.value.status == 400, q
                with pytest.raises(BackingError) as e:
                    await _agg(c, "c", b"{not json")
                assert e.value.status == 400
                # a collection with TTL writes has no mirror: the document walk answers
                await _load(c, "t", dict(list(docs.items())[:50]))
                await c.doc_put(ACCT, DB, "t", "a||ttl", json.dumps({"who": "user1", "pts": 1}), ttl_ms=3_600_000)
                small = {**dict(list(docs.items())[:50]), "a||ttl": {"who": "user1", "pts": 1}}
                assert await _agg(c, "t", QUERIES[1]) == brute(small, QUERIES[1])
                st = (await c.doc_stats(ACCT, DB, "c"))["accelerator"]
                if mode == "off":
                    assert st["cpu"] == st["gpu"] == 0 and st["native"] > 0
                else:
                    assert st["cpu"] > 0 and st["gpu"] == 0 and st["native"] == 0 and st["rows"] > 0
            finally:
                await c.http.close()
    run(main())


def test_two_shards_equal_one_store(backings):  # noqa: F811
    docs = _docs(600, seed=13)

    async def main():
        sh = ShardedBackingClient(backings[:2], identity="platform-admin")
        one = BackingClient(backings[3], identity="platform-admin")
        try:
            for c in (sh, one):
                await _load(c, "agg", docs)
            per = [(await c.doc_stats(ACCT, DB, "agg"))["docs"] for c in sh.shards]
            assert sum(per) == 600 and min(per) > 200, per
            for q in QUERIES:
                for prefix in ("", "a||"):
                    got = await sh.doc_aggregate(ACCT, DB, "agg", json.dumps(q).encode(), prefix)
                    assert got == await one.doc_aggregate(ACCT, DB, "agg", json.dumps(q).encode(), prefix), q
                    assert json.loads(got) == brute(docs, q, prefix), q
            q = QUERIES[2]
            assert json.loads(await sh.doc_aggregate(ACCT, DB, "agg", json.dumps(q).encode(), hist=True)) == \
                brute(docs, q, hist=True)
            with pytest.raises(BackingError) as e:
                await sh.doc_aggregate(ACCT, DB, "agg", json.dumps(BAD[0]).encode())
            assert e.value.status == 400
        finally:
            await sh.http.close()
            await one.http.close()
    run(main())


# ------------------------------------------------------------------ GPU
@pytest.mark.gpu
def test_gpu_columnar_aggregate_equals_cpu():
    from aca_dotnet_workshop_amd.ops.gpu import GpuKernels
    k = GpuKernels()
    docs = _docs(20_000, seed=21)
    ix = ColumnarIndex()
    ix.bulk_load(docs.items())
    for q in QUERIES + [{"groupBy": ["i"], "aggregate": [{"op": "MAX", "key": "pts"}]},           # 20,000 groups
                        {"groupBy": ["i", "who"], "aggregate": [{"op": "SUM", "key": "i"}]}]:    # past the device cap
        got = ix.aggregate(q, k)
        assert got == ix.aggregate(q), q
        if q in QUERIES[1:3]:  # the CPU path has its own comparison with the oracle above
            assert got == brute(docs, q), q


@pytest.mark.gpu
@pytest.mark.parametrize("front", FRONTS)
def test_gpu_aggregate_route(front, monkeypatch):
    monkeypatch.setenv("TT_QUERY_ACCEL", "gpu")
    monkeypatch.setenv("TT_QUERY_ACCEL_MIN_DOCS", "1")
    docs = _docs(2000, seed=33)

    async def main():
        async with Backing(front, monkeypatch) as b:
            c = BackingClient(b.base, identity="x")
            try:
                await _load(c, "c", docs)
                before = (await c.doc_stats(ACCT, DB, "c"))["accelerator"]["gpu"]
                for q in QUERIES[:4]:
                    assert await _agg(c, "c", q, "a||") == brute(docs, q, "a||"), q
                st = (await c.doc_stats(ACCT, DB, "c"))["accelerator"]
                assert st["gpu"] == before + 4 and st["fallback"] == 0 and st["cpu"] == 0
            finally:
                await c.http.close()
    run(main())
