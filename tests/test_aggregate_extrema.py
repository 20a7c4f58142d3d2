"""MIN / MAX / COUNT(key) per group without a histogram (``ColumnarIndex.extrema_numpy``, on the GPU
``hip/group_extrema.hip``) and the ``project=partial`` form shards merge: the same answers as the
histogram path, checked against ``brute`` of ``test_aggregate_query`` -- the document loop that
shares only ``get_path`` / ``vkey`` / ``compare`` with the code under test.

``EXTREMA_FROM_CELLS`` is lowered to 0 so every eligible key takes the new path at these sizes,
and a spy on ``extrema_numpy`` / ``GpuKernels.extrema_scans`` confirms that it did.
"""
import copy
import functools
import json
import random

import numpy as np
import pytest

from aca_dotnet_workshop_amd.backing.client import BackingClient
from aca_dotnet_workshop_amd.backing.shards import ShardedBackingClient
from aca_dotnet_workshop_amd.ops import columnar
from aca_dotnet_workshop_amd.ops.columnar import AggGroups, ColumnarIndex, Unsupported, compare, parse_aggregate

from helpers import run
from test_aggregate_query import ACCT, DB, QUERIES, _docs, _load, brute
from test_backing_front import FRONTS, Backing
from test_shards import backings  # noqa: F401  (fixture: three CPU-mirror shards and one plain store)


def _ext_docs(n, seed):
    """``_docs`` plus ``stamp``, a string no two documents share (a timestamp), and ``solo``, a
    key only two of the seven ``who`` groups hold."""
    rng = random.Random(seed + 1000)
    out = copy.deepcopy(_docs(n, seed))
    for i, d in enumerate(out.values()):
        d["stamp"] = f"2024-{1 + rng.randrange(12):02d}-{1 + rng.randrange(28):02d}T{rng.randrange(24):02d}:00:00.{i:07d}"
        if d["who"] in ("user1", "user2") and rng.random() < 0.5:
            d["solo"] = rng.choice([4, "four", None, 4.5])
    return out


NOBODY = {"EQ": {"who": "nobody"}}
ELIGIBLE = [
    {"aggregate": [{"op": "MIN", "key": "stamp"}, {"op": "MAX", "key": "stamp"}, {"op": "COUNT", "key": "stamp"}]},
    {"filter": {"EQ": {"done": False}}, "groupBy": ["who"],
     "aggregate": [{"op": "COUNT"}, {"op": "MIN", "key": "i"}, {"op": "MAX", "key": "pts"}, {"op": "COUNT", "key": "pts"}]},
    {"filter": {"LT": {"i": 1500}}, "groupBy": ["team", "meta.prio"],
     "aggregate": [{"op": "MIN", "key": "pts"}, {"op": "max", "key": "team"}, {"op": "COUNT", "key": "meta.prio"},
                   {"op": "MAX", "key": "stamp"}]},
    {"groupBy": ["who"], "aggregate": [{"op": "MIN", "key": "solo"}, {"op": "MAX", "key": "solo"},     # absent from
                                       {"op": "COUNT", "key": "solo"}]},                               # whole groups
    {"groupBy": ["team"], "aggregate": [{"op": "MIN", "key": "nowhere"}, {"op": "COUNT", "key": "nowhere"}]},
    {"filter": NOBODY, "groupBy": ["team"], "aggregate": [{"op": "MIN", "key": "i"}]},
    {"filter": NOBODY, "aggregate": [{"op": "MAX", "key": "i"}, {"op": "COUNT", "key": "i"}]},
]
MIXED = [
    {"groupBy": ["who"], "aggregate": [{"op": "MIN", "key": "stamp"}, {"op": "MAX", "key": "stamp"},
                                       {"op": "SUM", "key": "pts"}, {"op": "AVG", "key": "i"}]},
    # pts is asked a SUM too: it stays on the histogram, stamp next to it does not
    {"filter": {"GTE": {"i": 100}}, "groupBy": ["done"],
     "aggregate": [{"op": "MIN", "key": "pts"}, {"op": "SUM", "key": "pts"}, {"op": "MAX", "key": "stamp"}]},
]
# eligible keys per query: how many extrema reductions one aggregate() makes
N_EXT = [1, 2, 4, 1, 1, 1, 1, 1, 1]


@pytest.fixture(scope="module")
def docs():
    return _ext_docs(3000, 5)


def _index(docs):
    ix = ColumnarIndex()
    ix.bulk_load(docs.items())
    return ix


@pytest.fixture(scope="module")
def index(docs):
    return _index(docs)


@pytest.fixture
def extrema_calls(monkeypatch):
    """Every eligible key on the extrema path; the list collects the key column of each call."""
    monkeypatch.setattr(ColumnarIndex, "EXTREMA_FROM_CELLS", 0)
    calls = []
    real = ColumnarIndex.extrema_numpy

    def spy(self, rows, gcols, gdims, kc):
        calls.append(kc)
        return real(self, rows, gcols, gdims, kc)
    monkeypatch.setattr(ColumnarIndex, "extrema_numpy", spy)
    return calls


@pytest.mark.parametrize("qi", range(len(ELIGIBLE + MIXED)))
def test_extrema_path_matches_brute_force(index, docs, extrema_calls, qi):
    q = (ELIGIBLE + MIXED)[qi]
    want = brute(docs, q)
    assert index.aggregate(q) == want
    assert len(extrema_calls) == N_EXT[qi]
    if qi == 3:  # five groups without the key: COUNT 0 and neither MIN nor MAX
        bare = [g for g in want["groups"] if g["aggregates"] == [{"op": "COUNT", "key": "solo", "value": 0}]]
        assert len(bare) == 5 and len(want["groups"]) == 7
    if qi == 5:
        assert want == {"groups": []}
    if qi == 6:
        assert want == {"groups": [{"group": {}, "count": 0, "aggregates": [{"op": "COUNT", "key": "i", "value": 0}]}]}
    # full histograms are still histograms, and take the histogram path
    del extrema_calls[:]
    assert index.aggregate(q, hist=True) == brute(docs, q, hist=True)
    assert not extrema_calls


def test_default_threshold_keeps_small_keys_on_the_histogram(index, docs, monkeypatch):
    monkeypatch.setattr(ColumnarIndex, "extrema_numpy", lambda *a: pytest.fail("extrema path below the threshold"))
    assert ColumnarIndex.EXTREMA_FROM_CELLS == 1 << 22
    for q in ELIGIBLE[:3]:
        assert index.aggregate(q) == brute(docs, q)


def test_extrema_numpy_is_the_kernel_contract(index):
    """(cells, counts, lo, hi) with lo / hi = rank << 32 | row, ties on the rank to the lowest /
    highest row, against a loop over the rows."""
    who, pts = index.col_of["who"], index.col_of["pts"]
    rows = np.nonzero(index.live[:index.n])[0][::3].astype(np.int32)
    d = len(index.columns[who].values)
    cells, counts, lo, hi = index.extrema_numpy(rows, [who], [d], pts)
    ranks = index.columns[pts].ranks()
    want = {}
    for r in rows.tolist():
        v = int(index.ids[pts, r])
        if v < 0:
            continue
        g = int(index.ids[who, r])
        key = (int(ranks[v]) << 32) | r
        e = want.setdefault(d if g < 0 else g, [0, key, key])
        e[0], e[1], e[2] = e[0] + 1, min(e[1], key), max(e[2], key)
    assert cells.tolist() == sorted(want)
    assert [[int(c), int(a), int(b)] for c, a, b in zip(counts, lo, hi)] == [want[c] for c in sorted(want)]
    empty = index.extrema_numpy(rows[:0], [who], [d], pts)
    assert all(a.size == 0 for a in empty)


def test_after_writes_deletes_and_a_compaction(extrema_calls):
    docs = _ext_docs(2500, 7)
    ix = _index(docs)
    queries = [ELIGIBLE[0], ELIGIBLE[1], ELIGIBLE[3], MIXED[0]]
    for q in queries:
        assert ix.aggregate(q) == brute(docs, q)
    keys = list(docs)
    late = {f"a||late{i:04d}": {"who": f"user{i % 9}", "done": False, "i": 10_000 + i, "pts": 0.25,
                                "stamp": f"2031-01-01T00:00:00.{i:07d}", "solo": "late"} for i in range(300)}
    for k, d in late.items():  # new dictionary values of every key column, two new groups
        ix.upsert(k, d)
    docs.update(late)
    for k in keys[:400]:      # overwritten: the old rows die
        docs[k] = {**docs[k], "stamp": "1999-" + docs[k]["stamp"][5:], "pts": -7}
        ix.upsert(k, docs[k])
    for k in keys[400:900]:
        ix.delete(k)
        del docs[k]
    assert ix._dead == 900 and ix.n > len(docs)
    for q in queries:
        assert ix.aggregate(q) == brute(docs, q), q
    ix.compact()
    assert ix.n == len(docs)
    for q in queries:
        assert ix.aggregate(q) == brute(docs, q), q
    assert len(extrema_calls) == 3 * (1 + 2 + 1 + 1)


# ------------------------------------------------------------------ the partial form
def _partial_of(docs, q, prefix=""):
    """The ``project=partial`` answer from the oracle's histograms: [count, min, max] ([0]
    without a value) for the keys of which only COUNT / MIN / MAX are asked."""
    res = brute(docs, q, prefix, hist=True)
    asked = {}
    for a in q.get("aggregate") or []:
        if "key" in a:
            asked.setdefault(a["key"], set()).add(a["op"].upper())
    ext = [k for k, ops in asked.items() if ops <= {"COUNT", "MIN", "MAX"}]
    by = functools.cmp_to_key(compare)
    for g in res["groups"]:
        g["ext"] = {}
        for k in ext:
            pairs = g["hist"].pop(k)
            vals = [v for v, _ in pairs]
            g["ext"][k] = [sum(c for _, c in pairs), min(vals, key=by), max(vals, key=by)] if pairs else [0]
    return res


@pytest.mark.parametrize("from_cells", [0, 1 << 22])
def test_partial_form_has_one_shape_on_either_path(index, docs, monkeypatch, from_cells):
    monkeypatch.setattr(ColumnarIndex, "EXTREMA_FROM_CELLS", from_cells)
    for q in ELIGIBLE + MIXED + QUERIES[:4]:
        assert index.aggregate(q, partial=True) == _partial_of(docs, q), q
    q = MIXED[1]
    g = index.aggregate(q, partial=True)["groups"][0]
    assert set(g["hist"]) == {"pts"} and set(g["ext"]) == {"stamp"} and "aggregates" not in g
    # hist wins over partial: full histograms
    assert index.aggregate(q, hist=True, partial=True) == brute(docs, q, hist=True)


@pytest.mark.parametrize("from_cells", [0, 1 << 22])
def test_partials_of_two_halves_merge_to_the_one_store_answer(docs, monkeypatch, from_cells):
    monkeypatch.setattr(ColumnarIndex, "EXTREMA_FROM_CELLS", from_cells)
    items = list(docs.items())
    halves = [_index(dict(items[:1100])), _index(dict(items[1100:]))]
    one = _index(docs)
    for q in ELIGIBLE + MIXED:
        merged = AggGroups(parse_aggregate(q))
        for ix in halves:  # as the shard client gets them: through JSON
            merged.add_response(json.loads(json.dumps(ix.aggregate(q, partial=True))))
        assert merged.response() == one.aggregate(q) == brute(docs, q), q
        assert merged.response(partial=True) == one.aggregate(q, partial=True), q


def test_extrema_merge_by_compare_across_types():
    spec = parse_aggregate({"aggregate": [{"op": "MIN", "key": "k"}, {"op": "MAX", "key": "k"},
                                          {"op": "COUNT", "key": "k"}]})
    g = AggGroups(spec)
    g.add_extrema((), "k", 2, 2.5, 7.0)
    g.add_extrema((), "k", 0)                    # no defined value: nothing
    g.add_extrema((), "k", 1, "a", "a")          # string > number
    g.add_extrema((), "k", 3, None, True)        # null < bool < number
    g.add_extrema((), "k", 4, 1.0, "B")          # "B" < "a"; 1.0 is held as 1
    g.add_rows((), 12)
    assert g.response() == {"groups": [{"group": {}, "count": 12, "aggregates": [
        {"op": "MIN", "key": "k", "value": None}, {"op": "MAX", "key": "k", "value": "a"},
        {"op": "COUNT", "key": "k", "value": 10}]}]}
    h = AggGroups(spec)
    h.add_extrema((), "k", 4, 1.0, "B")
    h.add_extrema((), "k", 2, 2.5, 7.0)
    assert h.response(partial=True) == {"groups": [{"group": {}, "count": 0, "hist": {}, "ext": {"k": [6, 1, "B"]}}]}
    assert AggGroups(spec).response(partial=True)["groups"][0]["ext"] == {"k": [0]}


def test_key_space_past_2_62_answers(index, docs, monkeypatch):
    """A timestamp dictionary so large that (groups + 1) x (values + 1) passes 2^62: MIN / MAX /
    COUNT answer, at the default threshold; a SUM over it is still refused."""
    stamp = index.col_of["stamp"]
    real = ColumnarIndex._dict_size
    monkeypatch.setattr(ColumnarIndex, "_dict_size", lambda self, col: 1 << 62 if col == stamp else real(self, col))
    assert ColumnarIndex.EXTREMA_FROM_CELLS == 1 << 22
    for q in (ELIGIBLE[0], MIXED[0]):
        assert index.aggregate(q) == brute(docs, q)
    with pytest.raises(Unsupported):
        index.aggregate({"groupBy": ["who"], "aggregate": [{"op": "SUM", "key": "stamp"}]})
    with pytest.raises(Unsupported):
        index.aggregate(ELIGIBLE[0], hist=True)


# ------------------------------------------------------------------ the route
async def _agg(c, coll, q, prefix="", **kw):
    return json.loads(await c.doc_aggregate(ACCT, DB, coll, json.dumps(q).encode(), prefix, **kw))


@pytest.mark.parametrize("mode", ["off", "cpu"])
@pytest.mark.parametrize("front", FRONTS)
def test_partial_route(front, mode, monkeypatch, extrema_calls):
    monkeypatch.setenv("TT_QUERY_ACCEL", mode)
    monkeypatch.setenv("TT_QUERY_ACCEL_MIN_DOCS", "1")
    docs = _ext_docs(400, 9)

    async def main():
        async with Backing(front, monkeypatch) as b:
            c = BackingClient(b.base, identity="x")
            try:
                await _load(c, "c", docs)
                for q in (ELIGIBLE[1], ELIGIBLE[3], ELIGIBLE[6], MIXED[1]):
                    assert await _agg(c, "c", q, partial=True) == _partial_of(docs, q), q
                    assert await _agg(c, "c", q, "b||", partial=True) == _partial_of(docs, q, "b||"), q
                    assert await _agg(c, "c", q) == brute(docs, q), q
                    assert await _agg(c, "c", q, hist=True) == brute(docs, q, hist=True), q
            finally:
                await c.http.close()
    run(main())
    # accelerator off: the document walk, reduced by AggGroups; on: every eligible key by extrema
    assert len(extrema_calls) == (0 if mode == "off" else 3 * (2 + 1 + 1 + 1))


def test_two_shards_ask_for_partials_and_equal_one_store(backings):  # noqa: F811
    docs = _ext_docs(600, 13)

    async def main():
        sh = ShardedBackingClient(backings[:2], identity="platform-admin")
        one = BackingClient(backings[3], identity="platform-admin")
        asked = []
        for c in sh.shards:
            def spy(*a, _real=c.doc_aggregate, **kw):
                asked.append(kw)
                return _real(*a, **kw)
            c.doc_aggregate = spy
        try:
            for c in (sh, one):
                await _load(c, "ext", docs)
            for q in (ELIGIBLE[2], ELIGIBLE[3], MIXED[0], MIXED[1]):
                for prefix in ("", "a||"):
                    del asked[:]
                    got = await sh.doc_aggregate(ACCT, DB, "ext", json.dumps(q).encode(), prefix)
                    assert asked == [{"hist": False, "partial": True}] * 2
                    assert got == await one.doc_aggregate(ACCT, DB, "ext", json.dumps(q).encode(), prefix), q
                    assert json.loads(got) == brute(docs, q, prefix), q
            q = MIXED[0]
            del asked[:]
            got = await sh.doc_aggregate(ACCT, DB, "ext", json.dumps(q).encode(), hist=True)
            assert asked == [{"hist": True, "partial": False}] * 2 and json.loads(got) == brute(docs, q, hist=True)
            got = await sh.doc_aggregate(ACCT, DB, "ext", json.dumps(q).encode(), partial=True)
            assert json.loads(got) == _partial_of(docs, q)
        finally:
            await sh.http.close()
            await one.http.close()
    run(main())


# ------------------------------------------------------------------ GPU
GPU_QUERIES = [ELIGIBLE[0], ELIGIBLE[1], ELIGIBLE[2], ELIGIBLE[3], ELIGIBLE[6], MIXED[1],
               # 6,000 groups among 20,001 cells: more than the kernel keeps in LDS
               {"filter": {"LT": {"i": 6000}}, "groupBy": ["i"],
                "aggregate": [{"op": "MAX", "key": "stamp"}, {"op": "MIN", "key": "pts"}]}]
GPU_N_EXT = [1, 2, 4, 1, 1, 1, 2]


@pytest.mark.gpu
@pytest.mark.parametrize("stage", ["fresh", "writes", "deletes"])
def test_gpu_extrema_equal_cpu_and_brute_force(monkeypatch, stage):
    """20,000 documents, every eligible key reduced by ``tt_scan_extrema`` (the host selection is
    barred), a unique-per-document string key and the mixed-type ``pts`` among them: on a fresh
    index; after writes that add dictionary values to a mirror that holds the rank copies (new
    rank version: they are re-encoded); and after deletes on top of those."""
    from aca_dotnet_workshop_amd.ops.gpu import GpuKernels
    k = GpuKernels()
    docs = _ext_docs(20_000, 21)
    ix = _index(docs)
    monkeypatch.setattr(ColumnarIndex, "EXTREMA_FROM_CELLS", 0)
    if stage != "fresh":
        for q in GPU_QUERIES:  # the mirror and its rank copies, as of before the writes
            ix.aggregate(q, k)
        grown = [ix.col_of[p] for p in ("stamp", "pts", "i", "solo")]  # the writes add values to these
        assert set(grown) <= set(ix.mirror.ranks)
        versions = {c: ix.mirror.ranks[c].ver for c in grown}
        late = {f"a||late{i:04d}": {"who": f"user{i % 9}", "done": i % 2 == 0, "i": 100_000 + i, "pts": -0.5 - i,
                                    "stamp": f"1990-01-01T00:00:00.{i:07d}", "solo": f"late{i}"} for i in range(500)}
        for key, d in late.items():
            ix.upsert(key, d)
        docs.update(late)
        assert all(ix.columns[c].rank_version > v for c, v in versions.items())
    if stage == "deletes":
        for key in list(docs)[1000:4000]:
            ix.delete(key)
            del docs[key]

    def barred(*a, **kw):
        raise AssertionError("host selection on the device path")

    for q, n_ext in zip(GPU_QUERIES, GPU_N_EXT):
        with monkeypatch.context() as m:
            m.setattr(ColumnarIndex, "select_native", barred)
            m.setattr(ColumnarIndex, "select_numpy", barred)
            before = k.extrema_scans
            got = ix.aggregate(q, k)
            assert k.extrema_scans == before + n_ext, q
        assert got == ix.aggregate(q) == brute(docs, q), q
    if stage != "fresh":
        assert all(ix.mirror.ranks[c].ver > v for c, v in versions.items())  # re-encoded from the new ranks


