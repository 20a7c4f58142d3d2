"""``ColumnarIndex.aggregate`` over a device mirror that changes under it.

The kernels behind grouped aggregates are pinned by ``test_gpu_group_agg`` / ``test_gpu_group_extrema``;
here it is the state they read -- the rank-encoded copies ``DeviceMirror.program`` keeps of the
MIN / MAX / COUNT value columns, their rows of the descriptor table, the row under ``lo`` / ``hi``
-- and the planner that picks between the device and the host around ``tt_group_max_cells()``.

``AggRun`` is ``test_device_mirror_state.Run`` plus the documents themselves.  ``AggRun.aggregate``
asks the device path, checks the mirror invariant with the rank columns the planner must have
asked for (computed here from the dictionary sizes, never read back from the mirror), compares
the answer with the document loop ``brute`` of ``test_aggregate_query`` and with the host path,
and asserts the path taken: the number of ``scan_extrema`` launches, and whether the host
selection ran.  The histories run on ``HostKernels`` in the CPU suite and, marked ``gpu``, on the
device.  ``EXTREMA_FROM_CELLS`` is 0 throughout (every eligible key takes the extrema path at
these sizes) except in ``history_default_threshold``.

Every extrema key's values arrive in no sorted order -- dictionary ids do not order like ranks,
which each history asserts on its own data -- so a kernel handed ids for ranks answers wrongly.
"""
import json
import math
import random

import numpy as np
import pytest

from aca_dotnet_workshop_amd.ops.codes import width_for
from aca_dotnet_workshop_amd.ops.columnar import AggGroups, ColumnarIndex, extrema_keys, parse_aggregate

from test_aggregate_extrema import _partial_of
from test_aggregate_query import brute
from test_device_mirror_state import (F_EQ, F_PAGE, F_RANGE1, F_RANGE2, F_RANGE_M, SEEDS, SORTS, TILE, HostKernels,
                                      Run, _host, _make, gpu)  # noqa: F401  (gpu: fixture)


@pytest.fixture(autouse=True)
def _every_eligible_key_on_the_extrema_path(monkeypatch):
    monkeypatch.setattr(ColumnarIndex, "EXTREMA_FROM_CELLS", 0)


def _qid(q):
    return json.dumps(q, sort_keys=True)


# ------------------------------------------------------------------ the aggregate step
class AggRun(Run):
    """``Run`` that also keeps the documents as ``put`` / ``delete`` change them, and counts the
    bursts of writes (``changes``) and how many of them an invariant check followed (``covered``)."""

    def __init__(self, ix, kernels, read, store=None):
        super().__init__(ix, kernels, read, store)
        self.docs = {}
        self.dirty, self.changes, self.covered = False, 0, 0
        self.defined, self.empty, self.asked_queries = set(), set(), set()
        self.ext, self.ext_dev, self.fits = [], False, True  # of the last aggregate
        self._last_aggregate = False

    def _wrote(self):
        if not self.dirty:
            self.dirty = True
            self.changes += 1

    def put(self, key, doc):
        super().put(key, doc)
        self.docs[key] = doc
        self._wrote()

    def delete(self, key):
        super().delete(key)
        self.docs.pop(key, None)
        self._wrote()

    def compact(self):
        """The index's own compaction: rows renumber."""
        self.flush()
        self.ix.compact()
        self.plans = []
        self._wrote()

    def check(self):
        super().check()
        if self.dirty:
            self.dirty = False
            self.covered += 1

    def select(self, flt):
        self._last_aggregate = False
        return super().select(flt)

    def page(self, flt, sort, offset, limit):
        self._last_aggregate = False
        return super().page(flt, sort, offset, limit)

    def order(self, flt, sort):
        self._last_aggregate = False
        return super().order(flt, sort)

    def warm(self):
        """After an aggregate, ``warm`` keeps the rank copies the aggregate asked for."""
        want = self.asked if self._last_aggregate else None
        super().warm()
        assert want is None or self.asked == want, (self.asked, want)

    def size(self, path):
        return len(self.ix.columns[self.ix.col_of[path]].values)

    def cells(self, q):
        """Group cells of ``q`` from the index's dictionary sizes."""
        return math.prod(self.size(p) + 1 for p in (q.get("groupBy") or []))

    def aggregate(self, q, hist=False, partial=False, host=None):
        """The device answer == the document loop == the host path, after the invariant; the
        path taken is the one the dictionary sizes and the cap call for.  ``host``: whether this
        step is designed to need the host selection (None: whatever the sizes say)."""
        ix, k = self.ix, self.k
        self.flush()
        spec = parse_aggregate(q)
        cap = int(k.lib.tt_group_max_cells())
        ncols, gen, scans = len(ix.columns), ix._dict_gen, k.extrema_scans
        selections = []
        with pytest.MonkeyPatch.context() as mp:
            for name in ("select_native", "select_numpy"):
                def spy(ix_, *a, _real=getattr(ColumnarIndex, name), _name=name, **kw):
                    selections.append(_name)
                    return _real(ix_, *a, **kw)
                mp.setattr(ColumnarIndex, name, spy)
            got = ix.aggregate(q, k, hist, partial)
        if (len(ix.columns), ix._dict_gen) != (ncols, gen):
            self.plans = []  # a column the aggregate added: the sort plans belong to the old layout
        # the plan, from the request, the dictionary sizes and the cap
        gcells = self.cells(q)
        from_cells = min(ColumnarIndex.EXTREMA_FROM_CELLS, cap)
        ext = [] if hist else [key for key in extrema_keys(spec) if gcells * (self.size(key) + 1) > from_cells]
        ext_dev = gcells <= cap
        hists = [gcells] + [gcells * (self.size(key) + 1) for key in spec.keys if key not in ext]
        fits = (ext_dev or not ext) and all(h <= cap for h in hists)
        self.ext, self.ext_dev, self.fits = ext, ext_dev, fits
        prog = ix.compile_cached(spec.filter or {})
        self.asked = sorted(set(self._range_cols(prog)) | ({ix.col_of[key] for key in ext} if ext_dev else set()))
        self.check()
        self._last_aggregate = True
        assert k.extrema_scans - scans == (len(ext) if ext_dev else 0), (q, ext, ext_dev)
        # everything fits the device: no host selection; otherwise it must have run
        assert bool(selections) == (not fits), (q, selections, gcells, hists, cap)
        assert host is None or host == (not fits), (q, gcells, hists, cap)
        want = _partial_of(self.docs, q) if partial and not hist else brute(self.docs, q, hist=hist)
        assert got == want, q
        assert ix.aggregate(q, None, hist, partial) == want, q
        if not hist and not partial:
            qid = _qid(q)
            self.asked_queries.add(qid)
            if any(a["op"] in ("MIN", "MAX") and "value" in a for g in got["groups"] for a in g["aggregates"]):
                self.defined.add(qid)
            if not got["groups"] or (not spec.group_by and got["groups"][0]["count"] == 0):
                self.empty.add(qid)
        return got

    def ids_do_not_order_like_ranks(self, *paths):
        for p in paths:
            ranks = self.ix.columns[self.ix.col_of[p]].ranks()
            assert ranks.size > 2 and (np.diff(ranks) < 0).any(), f"{p}: ids order like ranks"

    def finish(self, empties=()):
        """Every burst of writes was followed by an invariant check, every query asked had a
        defined MIN / MAX at some step, and the designed ones an empty answer at some step."""
        assert not self.dirty and self.covered == self.changes > 0 and self.checks >= self.changes
        assert self.asked_queries and self.defined == self.asked_queries, \
            [q for q in self.asked_queries - self.defined]
        for q in empties:
            assert _qid(q) in self.empty, q
        return self


def _agg_make(kernels, read, backend="docs", capacity=2 * TILE, paths=("b", "m", "d", "c")):
    run = _make(kernels, read, backend, capacity=capacity, paths=list(paths))
    return AggRun(run.ix, run.k, run.read, run.store)


# ------------------------------------------------------------------ documents and queries
def _stamp(t, tail=""):
    return f"2025-01-{1 + t // 1440:02d}T{t // 60 % 24:02d}:{t % 60:02d}:00{tail}"


def _adoc(rnd, stamps=40_000):
    """b: 2-bit codes; m, d, e: one byte; c: timestamps in no order; p: values of every JSON type;
    s: only the groups m000..m019 hold it."""
    t = rnd.randrange(stamps)
    d = {"b": rnd.choice([True, False, None]), "m": f"m{rnd.randrange(100):03d}", "d": rnd.randrange(50),
         "c": _stamp(t), "e": rnd.randrange(5), "p": rnd.choice([1, 1.0, 2.5, -3, 0, None, "n/a", True, 1e16])}
    if d["m"] < "m020":
        d["s"] = rnd.choice([4, "four", None, 4.5, t])
    if rnd.random() < 0.06:
        del d[rnd.choice(["b", "m", "d", "c", "e", "p"])]
    return d


def _ops(key, *ops):
    return [{"op": op, "key": key} for op in ops]


NOBODY = {"EQ": {"m": "m999"}}  # nobody, until a history writes such a document
# no group column (the register reduction); the range leaf and the extrema key share one rank copy
Q_NOGROUP = {"filter": {"GTE": {"c": "2025-01-09"}}, "aggregate": _ops("c", "MIN", "MAX", "COUNT")}
# a 2-bit group column (interleaved copies); a histogram key (SUM, AVG) next to an extrema key
Q_2BIT = {"groupBy": ["b"], "aggregate": [{"op": "COUNT"}, *_ops("c", "MIN", "MAX"), *_ops("d", "SUM", "AVG")]}
# a one-byte group column (LDS cells); s is absent from whole groups; d is range leaf and extrema key
Q_BYTE = {"filter": {"LT": {"d": 30}}, "groupBy": ["m"], "aggregate": [*_ops("s", "MIN", "MAX", "COUNT"), *_ops("d", "MAX")]}
# two group columns, e first seen by the aggregate itself; a key no document holds; p is asked
# before c, whose column comes first: the rank copies' rows of the table follow the columns' order
Q_TWO = {"groupBy": ["e", "b"], "aggregate": [*_ops("p", "MAX"), *_ops("c", "MIN"), *_ops("nowhere", "MIN", "COUNT")]}
# empty selections, grouped (no group at all) and not (one group of no rows)
Q_NONE_G = {"filter": NOBODY, "groupBy": ["b"], "aggregate": _ops("c", "MIN")}
Q_NONE = {"filter": NOBODY, "aggregate": _ops("c", "MAX", "COUNT")}
QUERIES = [Q_NOGROUP, Q_2BIT, Q_BYTE, Q_TWO, Q_NONE_G, Q_NONE]
EMPTIES = [Q_NONE_G, Q_NONE]


def _first_round(run):
    """Every query once: s, e, p and nowhere become columns (layout changes), the empty
    selections are empty; then a document of m999, so that they are not."""
    ix = run.ix
    for q in QUERIES:
        ncols = len(ix.columns)
        run.aggregate(q, host=False)
        if q is Q_BYTE:
            assert len(ix.columns) == ncols + 1 and ix.col_of["s"] == ncols
        if q is Q_TWO:
            assert len(ix.columns) == ncols + 3 and run.size("nowhere") == 0
    assert _qid(Q_NONE) in run.empty and _qid(Q_NONE_G) in run.empty
    assert run.cells(Q_2BIT) == 4 and 64 < run.cells(Q_BYTE) <= 256 and run.cells(Q_TWO) == 24
    c, d = ix.col_of["c"], ix.col_of["d"]
    assert c in run._range_cols(ix.compile_cached(Q_NOGROUP["filter"]))
    assert d in run._range_cols(ix.compile_cached(Q_BYTE["filter"]))
    run.put("nobody", {"m": "m999", "b": True, "c": _stamp(777, ".5"), "d": 7})
    run.aggregate(Q_NONE_G, host=False)
    run.aggregate(Q_NONE, host=False)


# ------------------------------------------------------------------ a. appends
def history_appends(kernels, read, seed):
    """Batches that end on every row offset mod 16 across the first tile boundary, an aggregate
    after each: batches of values the dictionaries hold already (the rank copy of c is encoded
    over the new rows only) and batches with new timestamps and a new group (a new rank version:
    the copy is re-encoded from row 0)."""
    rnd = random.Random(seed)
    run = _agg_make(kernels, read)
    ix = run.ix
    made = 0

    def append(doc):
        nonlocal made
        run.put(f"k{made}", doc)
        made += 1

    for _ in range(TILE - 150):
        append(_adoc(rnd))
    for key in rnd.sample(sorted(run.docs), 6000):  # the rows stay (no compaction yet): a short document loop
        run.delete(key)
    _first_round(run)
    assert ix.n == TILE - 149 and ix._dead == 6000
    c = ix.col_of["c"]
    calls = getattr(kernels, "calls", None)  # the stand-in counts the rows it rank-encodes
    sizes = [1, 3, 7, 16, 15] + [17] * 16 + [5, 64, 1]
    ends, crossed, old = set(), set(), list(run.docs.values())
    for i, size in enumerate(sizes):
        fresh = i % 2 == 1
        version, n = ix.columns[c].rank_version, ix.n
        for j in range(size):
            if fresh:
                doc = dict(_adoc(rnd), c=_stamp(rnd.randrange(40_000), f".{made:05d}"))
                if j == 0:
                    doc["m"] = f"m1{i:02d}"  # a new group
                append(doc)
            else:
                append(dict(rnd.choice(old)))
        assert (ix.columns[c].rank_version != version) == fresh and ix.n == n + size
        ends.add(ix.n % 16)
        crossed.add(ix.n > TILE)
        rows = calls and calls["rank_rows"]
        run.aggregate(Q_2BIT, host=False)  # the last aggregate before the batch left c's copy synced to its n
        assert calls is None or calls["rank_rows"] - rows == (ix.n if fresh else size)  # from row 0 / [synced, n)
        assert ix.mirror.ranks[c].ver == ix.columns[c].rank_version
        if i % 4 == 0:
            rows = calls and calls["rank_rows"]
            run.aggregate(Q_2BIT, host=False)  # nothing new: nothing encoded
            assert calls is None or calls["rank_rows"] == rows
        run.aggregate(QUERIES[i % len(QUERIES)], host=False)
        for _ in range(16):  # known values again, next to another query's copies
            append(dict(rnd.choice(old)))
        rows = calls and calls["rank_rows"]
        run.aggregate(Q_2BIT, host=False)
        assert calls is None or calls["rank_rows"] == rows + 16
    assert ends >= set(range(16)) and crossed == {False, True} and ix.cap == 2 * TILE
    for q in QUERIES:
        run.aggregate(q, host=False)
    run.ids_do_not_order_like_ranks("c", "d", "s", "p")
    return run.finish(EMPTIES)


@pytest.mark.parametrize("seed", SEEDS)
def test_appends(seed):
    history_appends(*_host(), seed)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", SEEDS)
def test_gpu_appends(gpu, seed):
    history_appends(*gpu, seed)


# ------------------------------------------------------------------ b. tombstones, updates, compaction
def _holders(docs, group, lo, hi):
    return [k for k, d in docs.items() if d.get("b", "-") == group and d.get("c") in (lo, hi)]


def history_tombstones(kernels, read, seed):
    """The documents that hold a group's MIN and MAX are deleted (found through the document
    loop): the next extremum comes up.  Overwrites kill old rows, the capacity grows past its
    first tile, and ``compact`` renumbers the rows under ``lo`` / ``hi``."""
    rnd = random.Random(seed)
    run = _agg_make(kernels, read, capacity=TILE)
    ix = run.ix
    for i in range(TILE - 300):
        run.put(f"k{i}", _adoc(rnd))
    _first_round(run)
    made = TILE - 300
    for r, group in enumerate([True, False, None]):
        was = {g["group"].get("b", "-"): g["aggregates"] for g in brute(run.docs, Q_2BIT)["groups"]}[group]
        lo, hi = was[1]["value"], was[2]["value"]
        victims = _holders(run.docs, group, lo, hi)
        assert len(victims) >= 2 and lo < hi
        for key in victims:
            run.delete(key)
        now = {g["group"].get("b", "-"): g["aggregates"] for g in run.aggregate(Q_2BIT, host=False)["groups"]}[group]
        assert lo < now[1]["value"] <= now[2]["value"] < hi
        run.aggregate(Q_NOGROUP, host=False)
        for key in rnd.sample(sorted(run.docs), 40):  # overwritten: the old rows die
            run.put(key, _adoc(rnd))
        run.aggregate(Q_BYTE, host=False)
        run.aggregate(Q_TWO, host=False)
        if r == 0:  # past the first tile: the capacity doubles
            for _ in range(400):
                run.put(f"k{made}", _adoc(rnd))
                made += 1
            run.aggregate(Q_2BIT, host=False)
            assert ix.cap == 2 * TILE and ix.n > TILE
            run.aggregate(Q_NONE, host=False)
        if r >= 1:
            run.delete("nobody") if r == 1 else run.put("nobody", {"m": "m999", "c": _stamp(5), "b": None})
            n, dead = ix.n, ix._dead
            assert dead > 40
            run.compact()
            assert ix.n == n - dead
            for q in (Q_2BIT, Q_NONE_G, Q_BYTE, Q_NOGROUP):
                run.aggregate(q, host=False)
            run.select(F_RANGE2)
            run.aggregate(Q_TWO, host=False)
    run.ids_do_not_order_like_ranks("c", "d", "s", "p")
    return run.finish(EMPTIES)


@pytest.mark.parametrize("seed", SEEDS)
def test_tombstones_updates_and_compaction(seed):
    history_tombstones(*_host(), seed)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", SEEDS)
def test_gpu_tombstones_updates_and_compaction(gpu, seed):
    history_tombstones(*gpu, seed)


# ------------------------------------------------------------------ c. width growth
W_GROUP = {"groupBy": ["g"], "aggregate": _ops("v", "MIN", "MAX", "COUNT")}
W_LEAF = {"filter": {"GTE": {"v": "v30000"}}, "aggregate": _ops("v", "MIN", "MAX")}
W_TWO = {"groupBy": ["g", "o"], "aggregate": [*_ops("v", "MAX"), *_ops("n", "SUM")]}
W_2BIT = {"groupBy": ["o"], "aggregate": [{"op": "COUNT"}, *_ops("v", "MIN"), *_ops("n", "AVG")]}
W_STOPS = [2, 3, 4, 63, 64, 254, 255, 4095, 4096, 65_534, 65_535]


def history_width_growth(kernels, read, seed):
    """The value key v goes through 3 -> 4, 254 -> 255 and 65,534 -> 65,535 values (its rank copy
    1 -> 2 -> 4 bytes), the group column g through 3 -> 4 (2-bit to one byte), 63 -> 64 (65
    cells: past the interleaved copies) and 4,095 -> 4,096 values (4,097 cells: past the LDS):
    aggregates right before and right after each switch.  Both arrive in no order."""
    rnd = random.Random(seed)
    run = _agg_make(kernels, read, capacity=9 * TILE, paths=["v", "g", "o", "n"])
    ix, m = run.ix, run.ix.mirror
    v, g = ix.col_of["v"], ix.col_of["g"]
    for j in range(10):  # o (2-bit) and n are complete before v and g begin
        run.put(f"o{j}", {"o": "xyz"[j % 3], "n": j})
    names = [f"v{j:05d}" for j in range(65_535)]
    groups = [f"g{j:04d}" for j in range(4096)]
    rnd.shuffle(names)
    rnd.shuffle(groups)
    rank_width = {254: 1, 255: 2, 4095: 2, 4096: 2, 65_534: 2, 65_535: 4}
    made = 0
    for size in W_STOPS:
        while made < size:
            run.put(f"k{made}", {"v": names[made], "g": groups[made if made < 4096 else rnd.randrange(4096)],
                                 "o": rnd.choice("xyz"), "n": rnd.randrange(10)})
            made += 1
            if rnd.random() < 0.02:  # v missing, and g too at times
                run.put(f"x{made}", {"o": rnd.choice("xyz"), "n": 3, **({"g": groups[rnd.randrange(min(made, 4096))]}
                                                                          if rnd.random() < 0.5 else {})})
        gsize = min(size, 4096)
        assert run.size("v") == size and run.size("g") == gsize and run.size("o") == 3
        for q in {65_534: [W_GROUP], 65_535: [W_GROUP, W_LEAF]}.get(size, [W_GROUP, W_LEAF, W_TWO, W_2BIT]):
            run.aggregate(q, host=False)
            assert m.ranks[v].w == rank_width.get(size, 1) and m.widths[v] == width_for(size)
            assert m.widths[g] == width_for(gsize) and m.widths[ix.col_of["o"]] == 0
        assert run.cells(W_GROUP) == gsize + 1 and run.cells(W_TWO) == 4 * (gsize + 1)
    assert ix.n <= ix.cap == 9 * TILE and m.ranks[v].w == 4
    run.ids_do_not_order_like_ranks("v")
    granks = ix.columns[g].ranks()
    assert (np.diff(granks) < 0).any()
    return run.finish()


@pytest.mark.parametrize("seed", SEEDS)
def test_width_growth(seed):
    history_width_growth(*_host(), seed)


@pytest.mark.gpu
def test_gpu_width_growth(gpu):
    history_width_growth(*gpu, SEEDS[0])


# ------------------------------------------------------------------ d. rank slots
Q_LEAF_D = {"filter": {"LT": {"d": 30}}, "groupBy": ["b"], "aggregate": _ops("c", "MIN", "MAX")}  # c's copy behind d's


def history_rank_slots(kernels, read, seed):
    """Aggregates with different extrema keys between selects with zero, one and two range
    leaves, pages, an ordering and ``warm``: the extra rank copies are dropped, re-added and
    re-numbered, and a program's cached device copy follows the slots of its leaves."""
    rnd = random.Random(seed)
    run = _agg_make(kernels, read, capacity=3 * TILE)
    ix, m = run.ix, run.ix.mirror
    made = 0

    def append(count):
        nonlocal made
        for _ in range(count):
            run.put(f"k{made}", _adoc(rnd))
            made += 1

    append(TILE + 500)
    _first_round(run)
    c, d = ix.col_of["c"], ix.col_of["d"]
    steps = [lambda: run.aggregate(Q_2BIT, host=False), lambda: run.select(F_EQ),
             lambda: run.aggregate(Q_BYTE, host=False), lambda: run.select(F_RANGE1),
             lambda: run.page(F_PAGE, SORTS[1], 0, 50), lambda: run.aggregate(Q_NOGROUP, host=False),
             lambda: run.select(F_RANGE2), lambda: run.aggregate(Q_TWO, host=False),
             lambda: run.order(F_PAGE, SORTS[2]), lambda: run.aggregate(Q_NONE_G, host=False),
             lambda: run.select(F_RANGE_M), lambda: run.aggregate(Q_NONE, host=False),
             lambda: run.aggregate(Q_LEAF_D, host=False)]
    aggregates = {0, 2, 5, 7, 9, 11, 12}
    slots = {c: set(), d: set()}
    for order in (range(13), reversed(range(13)), rnd.sample(range(13), 13), rnd.sample(range(13), 13)):
        for i in order:
            steps[i]()
            for col in slots:
                if col in run.asked:
                    slots[col].add(m.rank_slot[col])
            if i in aggregates and rnd.random() < 0.5:
                append(rnd.choice([1, 3, 16]))
                run.warm()  # the copies of the aggregate before it, brought up to the new rows
                steps[i]()
            append(rnd.choice([0, 3, 16, 33]))
    for i in sorted(aggregates):
        steps[i]()
    # the copies of c and d sat in different rows of the table with the company they kept
    assert len(slots[c]) >= 2 and len(slots[d]) >= 2, slots
    run.ids_do_not_order_like_ranks("c", "d", "s", "p")
    return run.finish(EMPTIES)


@pytest.mark.parametrize("seed", SEEDS)
def test_rank_slots(seed):
    history_rank_slots(*_host(), seed)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", SEEDS)
def test_gpu_rank_slots(gpu, seed):
    history_rank_slots(*gpu, seed)


# ------------------------------------------------------------------ e. the native mirror
def history_native(kernels, read, seed):
    """An index fed by a ``DocStore``'s column mirror, written through the store alone: appends,
    overwrites and deletes between aggregates, columns added late (new generations) and a
    compaction on the store's side (rows renumber under the index)."""
    rnd = random.Random(seed)
    run = _agg_make(kernels, read, "native")
    ix, store = run.ix, run.store
    assert ix.native is store and ix.docs is None
    live = 2500
    for i in range(live):
        run.put(f"k{i}", _adoc(rnd))
    gen = ix.generation
    _first_round(run)  # s, then e, p and nowhere: two new generations
    assert ix.generation >= gen + 2
    for r in range(3):
        for _ in range(rnd.choice([5, 17, 60])):
            run.put(f"k{rnd.randrange(live)}", dict(_adoc(rnd), c=_stamp(rnd.randrange(40_000), f".{r}")))
        run.aggregate(Q_2BIT, host=False)
        for key in rnd.sample(sorted(run.docs), 30):
            run.delete(key)
        run.aggregate(Q_BYTE, host=False)
        run.select(F_RANGE2)
        run.aggregate(Q_TWO, host=False)
        run.aggregate(Q_NOGROUP, host=False)
    # rewritten until the store compacts its mirror: the documents stay, their rows renumber
    texts = {key: json.dumps(doc) for key, doc in run.docs.items()}
    before, gen = store.mirror_stats()["compactions"], ix.generation
    for _ in range(40):
        for key, text in texts.items():
            store.set(key, text)
        if store.mirror_stats()["compactions"] > before:
            break
    assert store.mirror_stats()["compactions"] == before + 1
    run.plans = []
    run._wrote()
    run.put("late", dict(_adoc(rnd), late="z"))
    for q in (Q_2BIT, Q_BYTE, Q_NONE_G):
        run.aggregate(q, host=False)
    assert ix.generation > gen and ix.n <= 2 * TILE
    gen = ix.generation
    run.aggregate({"groupBy": ["late"], "aggregate": _ops("c", "MIN", "MAX")}, host=False)  # a column added late
    assert ix.generation > gen
    for q in (Q_TWO, Q_NOGROUP, Q_NONE):
        run.aggregate(q, host=False)
    run.ids_do_not_order_like_ranks("c", "d", "s", "p")
    return run.finish(EMPTIES)


@pytest.mark.parametrize("seed", SEEDS)
def test_native_mirror(seed):
    history_native(*_host(), seed)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", SEEDS)
def test_gpu_native_mirror(gpu, seed):
    history_native(*gpu, seed)


# ------------------------------------------------------------------ f. cell caps
C_HIST = {"groupBy": ["b"], "aggregate": [*_ops("c", "MIN", "MAX"), *_ops("d", "SUM")]}   # 4 groups, 4 x 51 cells
C_GROUPS = {"filter": {"LT": {"d": 30}}, "groupBy": ["m", "b"], "aggregate": _ops("c", "MIN", "COUNT")}  # 101 x 4 groups
C_EDGE = {"groupBy": ["w"], "aggregate": _ops("c", "MIN", "MAX")}                        # 64, then 65 groups
C_EDGE2 = {"groupBy": ["h", "b"], "aggregate": _ops("c", "MAX")}                         # 16 x 4, then 17 x 4


def history_cell_caps(kernels, read, seed):
    """A device that takes 64 cells.  Groups that fit with a histogram that does not (the
    extrema on the device, the histogram by ``bincount`` or ``np.unique`` on the host); groups
    alone past the cap (``extrema_numpy`` over the host selection, the device keeps the program
    and the range leaf's copy); exactly 64 group cells, then 65."""
    rnd = random.Random(seed)
    cap = int(kernels.lib.tt_group_max_cells())
    assert cap == 64
    run = _agg_make(kernels, read, paths=["b", "m", "d", "c", "w", "h"])
    ix = run.ix
    made = 0

    def append(count, **fields):
        nonlocal made
        for _ in range(count):
            run.put(f"k{made}", {**_adoc(rnd), "w": f"w{made % 63:02d}", "h": f"h{rnd.randrange(15):02d}", **fields})
            made += 1

    append(TILE + 100)
    for r in range(2):
        append(40)
        assert run.cells(C_HIST) == 4 <= cap < 4 * (run.size("d") + 1)
        run.aggregate(C_HIST, host=True)
        assert run.ext == ["c"] and run.ext_dev
        with pytest.MonkeyPatch.context() as mp:  # the sparse host count
            mp.setattr(ColumnarIndex, "HOST_MAX_CELLS", 16)
            run.aggregate(C_HIST, host=True)
        assert run.cells(C_GROUPS) == 101 * 4 > cap
        run.aggregate(C_GROUPS, host=True)
        assert run.ext == ["c"] and not run.ext_dev and run.asked == [ix.col_of["d"]]
        run.select(F_RANGE1)
        if r == 0:
            assert run.cells(C_EDGE) == cap == run.cells(C_EDGE2)
            run.aggregate(C_EDGE, host=False)
            run.aggregate(C_EDGE2, host=False)
            assert run.ext_dev and run.fits
            append(1, w="w63")
            assert run.cells(C_EDGE) == cap + 1
            run.aggregate(C_EDGE, host=True)
            assert not run.ext_dev
            run.aggregate(C_EDGE2, host=False)
            append(1, h="h15")
            assert run.cells(C_EDGE2) == cap + 4
            run.aggregate(C_EDGE2, host=True)
    run.ids_do_not_order_like_ranks("c", "d")
    return run.finish()


@pytest.mark.parametrize("seed", SEEDS)
def test_cell_caps(seed):
    history_cell_caps(HostKernels(max_cells=64), lambda t: t.numpy(), seed)


C_DEVICE = {"groupBy": ["x", "y"], "aggregate": [{"op": "COUNT"}, *_ops("c", "MIN", "MAX")]}


def history_device_cell_cap(kernels, read, seed):
    """The device's own cap, 2^22 cells, in one tile of rows: two group columns of 2,047 values
    each are 2,048^2 cells, exactly the cap (everything on the device); one more value each,
    2,049^2 cells, is one product past it (everything on the host).  A single group column at
    the cap needs 2^22 - 1 distinct values, more rows than a tile: ``test_gpu_group_agg`` has it."""
    rnd = random.Random(seed)
    cap = int(kernels.lib.tt_group_max_cells())
    assert cap == 1 << 22
    run = _agg_make(kernels, read, capacity=TILE, paths=["x", "y", "c"])
    xs, ys = rnd.sample(range(10_000), 2048), rnd.sample(range(10_000), 2048)
    for i in range(TILE - 20):
        doc = {"x": xs[i % 2047 if i < 4094 else rnd.randrange(2047)], "c": _stamp(rnd.randrange(40_000)),
               "y": ys[(i * 7) % 2047 if i < 4094 else rnd.randrange(2047)]}
        if i % 50 == 0:
            del doc["xy"[i // 50 % 2]]
        run.put(f"k{i}", doc)
    assert run.size("y") == 2047 and run.size("x") == 2047
    assert run.cells(C_DEVICE) == cap
    run.aggregate(C_DEVICE, host=False)
    assert run.ext == ["c"] and run.ext_dev
    run.put("x+", {"x": xs[2047], "y": ys[0], "c": _stamp(1)})
    run.aggregate(C_DEVICE, host=True)   # 2,049 x 2,048 cells
    assert not run.ext_dev
    run.put("y+", {"x": xs[1], "y": ys[2047], "c": _stamp(2)})
    assert run.cells(C_DEVICE) == 2049 * 2049
    run.aggregate(C_DEVICE, host=True)
    assert not run.ext_dev and run.ix.n <= TILE
    run.ids_do_not_order_like_ranks("c", "x")
    return run.finish()


def test_device_cell_cap():
    history_device_cell_cap(*_host(), SEEDS[0])


@pytest.mark.gpu
def test_gpu_device_cell_cap(gpu):
    history_device_cell_cap(*gpu, SEEDS[0])


# ------------------------------------------------------------------ g. the forms of the answer
def history_forms(kernels, read, seed):
    """``hist`` and ``partial`` answers on the device path at two points of one history, and the
    partials of two mirrors that each hold half the documents, merged through JSON as the shard
    client merges them, against the answer of one mirror over all of them."""
    rnd = random.Random(seed)
    one, halves = _agg_make(kernels, read), [_agg_make(kernels, read, capacity=TILE) for _ in range(2)]
    made = 0

    def append(count):
        nonlocal made
        for _ in range(count):
            doc = _adoc(rnd)
            one.put(f"k{made}", doc)
            halves[made % 2].put(f"k{made}", doc)
            made += 1

    for count in (3000, 300):
        append(count)
        if count == 300:  # the empty selections of the first round are not empty in the second
            for run in (one, halves[1]):
                run.put("nobody", {"m": "m999", "b": False, "c": _stamp(4242)})
        for key in rnd.sample(sorted(one.docs), 50):
            for run in (one, *halves):
                run.delete(key)
        for q in QUERIES[:4]:
            one.aggregate(q, hist=True, host=False)
            assert one.ext == []
            one.aggregate(q, partial=True, host=False)
            assert one.ext and one.ext_dev
            one.aggregate(q, hist=True, partial=True, host=False)
        for q in QUERIES:
            merged = AggGroups(parse_aggregate(q))
            for run in halves:
                merged.add_response(json.loads(json.dumps(run.aggregate(q, partial=True, host=False))))
            assert merged.response() == one.aggregate(q, host=False), q
            assert merged.response(partial=True) == _partial_of(one.docs, q), q
    assert set(one.docs) == set(halves[0].docs) | set(halves[1].docs)
    one.ids_do_not_order_like_ranks("c", "d", "s", "p")
    return one.finish(EMPTIES)


@pytest.mark.parametrize("seed", SEEDS)
def test_forms(seed):
    history_forms(*_host(), seed)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", SEEDS)
def test_gpu_forms(gpu, seed):
    history_forms(*gpu, seed)


# ------------------------------------------------------------------ h. the default threshold
D_EXT = {"groupBy": ["m", "e"], "aggregate": _ops("c", "MIN", "MAX")}   # 101 x 6 x 20,000 cells: past 2^22
D_HIST = {"groupBy": ["m"], "aggregate": _ops("c", "MIN", "MAX")}       # 101 x 20,000 cells: a histogram


def history_default_threshold(kernels, read, seed):
    """``EXTREMA_FROM_CELLS`` as shipped: a timestamp per document under 606 groups passes it
    (one ``scan_extrema``), under 101 groups it stays a histogram on the device (none)."""
    rnd = random.Random(seed)
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(ColumnarIndex, "EXTREMA_FROM_CELLS", 1 << 22)
        run = _agg_make(kernels, read, capacity=3 * TILE, paths=["m", "e", "c"])
        stamps = rnd.sample(range(10_000_000), 20_600)
        made = 0
        for count in (20_400, 7, 150):
            for _ in range(count):
                s = stamps[made]
                run.put(f"k{made}", dict(_adoc(rnd), c=f"2025-{1 + s // 1_000_000:02d}-01T00:00:00.{s % 1_000_000:06d}"))
                made += 1
            run.aggregate(D_EXT, host=False)
            assert run.ext == ["c"] and run.ext_dev and run.cells(D_EXT) * (run.size("c") + 1) > 1 << 22
            run.aggregate(D_HIST, host=False)
            assert run.ext == [] and run.cells(D_HIST) * (run.size("c") + 1) <= 1 << 22
            run.select(F_RANGE_M)
        run.ids_do_not_order_like_ranks("c")
        return run.finish()


def test_default_threshold():
    history_default_threshold(*_host(), SEEDS[0])


@pytest.mark.gpu
def test_gpu_default_threshold(gpu):
    history_default_threshold(*gpu, SEEDS[0])
