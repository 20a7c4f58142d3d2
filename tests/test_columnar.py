"""Columnar query compiler vs the native engine (CPU), and the HIP kernels vs both (GPU).

The native ``DocStore.query`` is the semantic reference; the NumPy executor runs the exact
program the HIP kernel runs, so CPU tests pin the compiler and GPU tests pin the kernels.
"""
import json
import random

import numpy as np
import pytest
from hypothesis import HealthCheck, example, given, settings
from hypothesis import strategies as st

from aca_dotnet_workshop_amd import native
from aca_dotnet_workshop_amd.ops.columnar import ColumnarIndex, Unsupported

N = native.load()
scalars = st.one_of(st.none(), st.booleans(), st.integers(-3, 3), st.floats(-3, 3, allow_nan=False).map(lambda x: round(x, 1)),
                    st.sampled_from(["a", "b", "c", "2024-05-01T00:00:00"]))
docs_st = st.lists(st.fixed_dictionaries({}, optional={"f": scalars, "g": scalars, "h": st.fixed_dictionaries({"k": scalars})}),
                   max_size=30)
paths = st.sampled_from(["f", "g", "h.k"])


def leaf():
    return st.one_of(
        st.builds(lambda p, v: {"EQ": {p: v}}, paths, scalars),
        st.builds(lambda p, v: {"NEQ": {p: v}}, paths, scalars),
        st.builds(lambda p, vs: {"IN": {p: vs}}, paths, st.lists(scalars, min_size=1, max_size=3)),
        st.builds(lambda o, p, v: {o: {p: v}}, st.sampled_from(["GT", "GTE", "LT", "LTE"]), paths,
                  st.one_of(st.integers(-3, 3), st.sampled_from(["a", "b", "2024-01-01"]), st.booleans())),
    )


filters_st = st.one_of(st.just({}), st.recursive(leaf(), lambda inner: st.one_of(
    st.builds(lambda xs: {"AND": xs}, st.lists(inner, min_size=1, max_size=3)),
    st.builds(lambda xs: {"OR": xs}, st.lists(inner, min_size=1, max_size=3))), max_leaves=6))
sort_st = st.one_of(st.none(), st.lists(st.fixed_dictionaries({"key": paths, "order": st.sampled_from(["ASC", "DESC"])}),
                                       min_size=1, max_size=2))


def _native_keys(docs, ops, q):
    s = N.DocStore()
    for k, d in ops:
        if d is None:
            s.delete(k)
        else:
            s.set(k, json.dumps(d))
    return [r["key"] for r in json.loads(s.query(json.dumps(q)))["results"]]


def _ops(docs, rnd):
    """Insert every doc, then update / delete a few (exercises tombstones + seq carry-over)."""
    ops = [(str(i), d) for i, d in enumerate(docs)]
    for _ in range(len(docs) // 3):
        i = rnd.randrange(len(docs))
        ops.append((str(i), None if rnd.random() < 0.4 else docs[rnd.randrange(len(docs))]))
    return ops


def _columnar(ops):
    ix = ColumnarIndex(["f"])
    for k, d in ops:
        if d is None:
            ix.delete(k)
        else:
            ix.upsert(k, d)
    return ix


@settings(max_examples=250, deadline=None)
@given(docs_st, filters_st, sort_st, st.integers(0, 1000))
@example(docs=[{"f": None, "h": {"k": -0.0}}], flt={"EQ": {"h.k": 0}}, sort=None, seed=0)  # -0.0 == 0
def test_numpy_executor_matches_native(docs, flt, sort, seed):
    if not docs:
        return
    ops = _ops(docs, random.Random(seed))
    q = {"filter": flt}
    if sort:
        q["sort"] = sort
    want = _native_keys(docs, ops, q)
    ix = _columnar(ops)
    got, token = ix.query(q)
    if sort:
        # ties inside equal sort keys are ordered by insertion in both engines
        assert got == want
    else:
        assert got == want


@settings(max_examples=150, deadline=None)
@given(docs_st, sort_st, st.integers(0, 1000))
def test_packed_sort_keys_match_lexsort(docs, sort, seed):
    """The packed 63-bit keys (what hip/sort_keys.hip computes) order rows exactly like the
    reference lexsort path."""
    if not docs:
        return
    ix = _columnar(_ops(docs, random.Random(seed)))
    rows = ix.select_numpy(ix.compile({}))
    if sort:
        for s in sort:
            ix.add_column(s["key"])
    plan = ix.sort_specs(sort)
    assert plan is not None
    got = rows[np.argsort(ix.sort_keys_numpy(rows, plan), kind="stable")]
    assert got.tolist() == ix.order_lexsort(rows, sort).tolist()


@settings(max_examples=120, deadline=None)
@given(docs_st, filters_st, sort_st, st.integers(0, 1000))
def test_bulk_encoded_index_matches_native(docs, flt, sort, seed):
    """ColumnarIndex.from_source (native DocStore.encode_columns, no Python docs kept) answers
    like the native engine, before and after incremental writes and a late column (re-encode)."""
    if not docs:
        return
    rnd = random.Random(seed)
    ops = _ops(docs, rnd)
    store = N.DocStore()
    for k, d in ops[: len(ops) // 2]:
        store.delete(k) if d is None else store.set(k, json.dumps(d))
    ix = ColumnarIndex.from_source(lambda paths: store.encode_columns("", paths), ["f"])
    assert ix.docs is None
    for k, d in ops[len(ops) // 2:]:  # mirrored writes, as the accelerator hooks apply them
        if d is None:
            store.delete(k)
            ix.delete(k)
        else:
            store.set(k, json.dumps(d))
            ix.upsert(k, d)
    q = {"filter": flt}
    if sort:
        q["sort"] = sort
    want = [r["key"] for r in json.loads(store.query(json.dumps(q)))["results"]]
    got, _ = ix.query(q)  # may add columns -> re-encode from the store
    assert got == want


@settings(max_examples=120, deadline=None)
@given(docs_st, filters_st, sort_st, st.integers(1, 7), st.integers(0, 1000))
def test_pages_concatenate_to_the_full_order(docs, flt, sort, limit, seed):
    """Paged queries (top-k partition per page on the host) walk the same order as one full query."""
    if not docs:
        return
    ix = _columnar(_ops(docs, random.Random(seed)))
    q = {"filter": flt, **({"sort": sort} if sort else {})}
    full, _ = ix.query(q)
    got, token = [], None
    while True:
        page = {"limit": limit, **({"token": token} if token else {})}
        keys, token = ix.query({**q, "page": page})
        got += keys
        if token is None:
            break
    assert got == full


def test_paging_and_compaction():
    ix = ColumnarIndex()
    for i in range(10000):
        ix.upsert(f"k{i}", {"n": i % 7, "s": f"v{i % 3}"})
    for i in range(0, 10000, 2):
        ix.delete(f"k{i}")
    keys, tok = ix.query({"filter": {"EQ": {"n": 3}}, "sort": [{"key": "s", "order": "DESC"}], "page": {"limit": 100}})
    assert len(keys) == 100 and tok == "100"
    before = ix.query({"filter": {"EQ": {"n": 3}}})[0]
    ix.compact()
    assert ix.n == 5000
    assert ix.query({"filter": {"EQ": {"n": 3}}})[0] == before


def test_unsupported_filters_raise():
    ix = ColumnarIndex(["a"])
    with pytest.raises(Unsupported):
        ix.compile({"LIKE": {"a": 1}})
    with pytest.raises(Unsupported):
        ix.compile({"EQ": {"a": [1, 2]}})
    deep = {"EQ": {"a": 1}}
    for _ in range(40):
        deep = {"AND": [{"EQ": {"a": 1}}, deep]}
    with pytest.raises(Unsupported):
        ix.compile(deep)


def test_group_count_numpy():
    ix = ColumnarIndex()
    for i in range(1000):
        ix.upsert(str(i), {"assignee": f"a{i % 5}", "done": i % 2 == 0})
    res = ix.group_count_numpy(ix.compile({"EQ": {"done": False}}), "assignee")
    assert res == {json.dumps(f"a{j}"): 100 for j in range(5)}


@settings(max_examples=150, deadline=None)
@given(docs_st, filters_st, st.integers(0, 1000), st.integers(1, 4))
def test_native_cpu_executor_matches_numpy(docs, flt, seed, threads):
    """native/src/cpuscan.hpp runs the same program over the device-layout narrow codes."""
    if not docs:
        return
    ix = _columnar(_ops(docs, random.Random(seed)))
    prog = ix.compile(flt)
    want = ix.select_numpy(prog).tolist()
    assert ix.select_native(prog, threads).tolist() == want
    assert ix.select_native(prog, threads, simd=False).tolist() == want


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097, 70_001])
def test_native_cpu_executor_all_widths(n):
    """1-, 2- and 4-byte code columns (dictionary sizes 3 / 300 / 70,000), range leaves on
    their rank copies, missing paths, tombstones, several threads -- against the NumPy reference."""
    rnd = random.Random(n)
    ix = ColumnarIndex(capacity=n)
    for i in range(n):
        d = {"small": rnd.choice([True, False, None]), "mid": f"m{rnd.randrange(300)}", "big": i % 70_000}
        if rnd.random() < 0.05:
            del d["mid"]
        ix.upsert(str(i), d)
    for i in rnd.sample(range(n), n // 20):
        ix.delete(str(i))
    filters = [{}, {"EQ": {"small": False}}, {"NEQ": {"mid": "m7"}}, {"LT": {"mid": "m150"}},
               {"AND": [{"GTE": {"big": 100}}, {"LT": {"big": 60_000}}, {"EQ": {"small": True}}]},
               {"OR": [{"IN": {"mid": ["m1", "m2", "m299"]}}, {"GT": {"big": 69_990}}]},
               {"EQ": {"nowhere": 1}}, {"EQ": {"mid": "not-a-value"}}]
    for f in filters:
        prog = ix.compile(f)
        want = ix.select_numpy(prog)
        for threads in (1, 3, 16):
            assert np.array_equal(ix.select_native(prog, threads), want), (n, f, threads)
        assert np.array_equal(ix.select_native(prog, 2, simd=False), want), (n, f, "scalar")


# ----------------------------------------------------------------------------- GPU
def _kernels():
    from aca_dotnet_workshop_amd.ops.gpu import GpuKernels
    return GpuKernels()


def _random_collection(n, rnd):
    creators = [f"user{i}@x" for i in range(97)]
    days = [f"2024-05-{d:02d}T00:00:00" for d in range(1, 29)]
    ix = ColumnarIndex(["taskCreatedBy", "taskDueDate", "isCompleted", "isOverDue"], capacity=n)
    for i in range(n):
        ix.upsert(str(i), {"taskCreatedBy": rnd.choice(creators), "taskDueDate": rnd.choice(days),
                           "isCompleted": rnd.random() < 0.3, "isOverDue": rnd.random() < 0.1, "prio": rnd.randrange(5)})
    for i in rnd.sample(range(n), n // 50):
        ix.delete(str(i))
    return ix


GPU_FILTERS = [
    {},
    {"EQ": {"taskCreatedBy": "user3@x"}},
    {"AND": [{"LT": {"taskDueDate": "2024-05-10T00:00:00"}}, {"EQ": {"isCompleted": False}}, {"EQ": {"isOverDue": False}}]},
    {"OR": [{"IN": {"prio": [0, 4]}}, {"NEQ": {"taskCreatedBy": "user7@x"}}]},
    {"AND": [{"GTE": {"prio": 2}}, {"OR": [{"EQ": {"isCompleted": True}}, {"GT": {"taskDueDate": "2024-05-20"}}]}]},
    {"EQ": {"missing.path": 1}},
]


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 4095, 4097, 200_003])
def test_gpu_scan_matches_numpy(n):
    k = _kernels()
    ix = _random_collection(n, random.Random(n))
    for f in GPU_FILTERS:
        prog = ix.compile(f)
        want = ix.select_numpy(prog)
        got = ix.select_gpu(prog, k)
        assert np.array_equal(got, want), (n, f)


@pytest.mark.gpu
@pytest.mark.parametrize("tiles", [1, 63, 64, 65, 1025, 12_207, 16_385])
def test_gpu_compaction_offsets_over_many_chunks(tiles):
    """The compaction on a synthetic selection mask far larger than the other tests'
    collections (12,207 tiles = 1e8 rows; 16,385 = one past the offset kernel's first pass, with
    a partial 16-tile group): tt_tile_offsets (exclusive offsets of all tiles in one block, total
    to device and pinned host memory) + tt_scan_compact_w (every wave finds its own base)."""
    import torch
    k = _kernels()
    g = torch.Generator().manual_seed(tiles)
    dens = torch.rand(tiles, 1, generator=g)  # per-tile density: chunk counts vary widely
    bits = torch.rand(tiles, 8192, generator=g) < dens
    counts = bits.sum(1).to(torch.int32)
    words = (bits.view(-1, 16).to(torch.int32) << torch.arange(16)).sum(1).to(torch.int16)  # row r -> bit r % 16
    mask, counts_d = words.to(k.device), counts.to(k.device)
    scratch = torch.full((tiles,), -1, dtype=torch.int32, device=k.device)
    nrows = tiles * 8192
    out = torch.empty(nrows, dtype=torch.int32, device=k.device)
    total = torch.empty(1, dtype=torch.int64, device=k.device)
    pinned = torch.zeros(1, dtype=torch.int64, pin_memory=True)
    want = torch.nonzero(bits.view(-1)).view(-1).to(torch.int32)
    # an output sized from a too-small estimate: the waves past it write nothing, the total is
    # exact, and the compaction alone re-runs into a buffer of that size
    small = max(1, want.numel() // 2)
    sentinel = torch.full((small + 64,), -7, dtype=torch.int32, device=k.device)
    assert k.lib.tt_launch_scan_compact(mask.data_ptr(), counts_d.data_ptr(), scratch.data_ptr(), nrows,
                                        sentinel.data_ptr(), small, total.data_ptr(), pinned.data_ptr(),
                                        k._stream()) == 0
    torch.cuda.synchronize()
    assert int(total.item()) == want.numel() and bool((sentinel[small:] == -7).all())
    assert k.lib.tt_launch_compact(mask.data_ptr(), scratch.data_ptr(), nrows, out.data_ptr(), want.numel(),
                                   k._stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(out[:want.numel()].cpu(), want)
    assert k.lib.tt_launch_scan_compact(mask.data_ptr(), counts_d.data_ptr(), scratch.data_ptr(), nrows,
                                        out.data_ptr(), nrows, total.data_ptr(), pinned.data_ptr(), k._stream()) == 0
    torch.cuda.synchronize()
    n = int(total.item())
    assert n == want.numel() == int(pinned[0])
    assert torch.equal(out[:n].cpu(), want)
    ref = torch.cumsum(counts.to(torch.int64), 0) - counts
    assert torch.equal(scratch.cpu(), ref.to(torch.int32))


@pytest.mark.gpu
def test_gpu_concurrent_selects_from_threads():
    """Queries of different collections run on different threads of the backing (one lock per
    collection): the shared pinned total / event of the kernels object must not mix results."""
    import threading
    k = _kernels()
    cols = [_random_collection(n, random.Random(n)) for n in (50_001, 120_007)]
    wants = [[ix.select_numpy(ix.compile(f)) for f in GPU_FILTERS] for ix in cols]
    errors = []

    def worker(i):
        ix = cols[i]
        try:
            for _ in range(15):
                for f, want in zip(GPU_FILTERS, wants[i]):
                    got = ix.select_gpu(ix.compile(f), k)
                    if not np.array_equal(got, want):
                        errors.append((i, f))
        except Exception as e:  # surfaced below
            errors.append((i, repr(e)))
    ts = [threading.Thread(target=worker, args=(i,)) for i in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors[:3]


@pytest.mark.gpu
def test_gpu_query_matches_native_engine():
    k = _kernels()
    rnd = random.Random(7)
    docs = [{"taskCreatedBy": f"u{rnd.randrange(20)}", "taskDueDate": f"2024-05-{rnd.randrange(1, 29):02d}T00:00:00",
             "isCompleted": rnd.random() < 0.3, "n": rnd.randrange(100)} for _ in range(20000)]
    s = N.DocStore()
    ix = ColumnarIndex()
    for i, d in enumerate(docs):
        s.set(str(i), json.dumps(d))
        ix.upsert(str(i), d)
    for q in ({"filter": {"AND": [{"LT": {"taskDueDate": "2024-05-15"}}, {"EQ": {"isCompleted": False}}]},
               "sort": [{"key": "n", "order": "DESC"}], "page": {"limit": 50}},
              {"filter": {"OR": [{"EQ": {"taskCreatedBy": "u1"}}, {"GT": {"n": 95}}]}}):
        want = [r["key"] for r in json.loads(s.query(json.dumps(q)))["results"]]
        got, _ = ix.query(q, k)
        assert got == want


@pytest.mark.gpu
@pytest.mark.parametrize("n", [3, 5000, 120_001])
def test_gpu_ordering_matches_host(n):
    """Device ordering (tt_sort_keys + radix sort / top-k) == host ordering, with paging."""
    k = _kernels()
    ix = _random_collection(n, random.Random(n + 1))
    for sort in (None, [{"key": "taskDueDate", "order": "DESC"}],
                 [{"key": "taskCreatedBy", "order": "ASC"}, {"key": "prio", "order": "DESC"}],
                 [{"key": "isCompleted"}, {"key": "missing.path", "order": "DESC"}]):
        for page in ({}, {"limit": 7}, {"limit": 50, "token": "10"}):
            q = {"filter": {"NEQ": {"taskCreatedBy": "user5@x"}}, "sort": sort, "page": page}
            if sort is None:
                del q["sort"]
            assert ix.query(q, k) == ix.query(q), (n, sort, page)


@pytest.mark.gpu
def test_gpu_range_leaves_track_rank_shifts():
    """Range leaves read a rank-encoded device column: new dictionary values that shift the
    ranks of existing ones (same width) force a re-encode; plain appends are incremental."""
    k = _kernels()
    ix = ColumnarIndex(["v"])
    for i in range(20000):
        ix.upsert(str(i), {"v": (i % 3 + 1) * 10})  # 10, 20, 30
    for f in ({"LT": {"v": 25}}, {"GTE": {"v": 20}}):
        prog = ix.compile(f)
        assert (prog.code[:, 0] == 7).any()  # compiled to OP_RANGE
        assert np.array_equal(ix.select_gpu(prog, k), ix.select_numpy(prog))
    for i in range(20000, 30000):
        ix.upsert(str(i), {"v": 15 if i % 2 else 20})  # 15 lands between existing ranks
    for f in ({"LT": {"v": 25}}, {"GT": {"v": 12}}, {"LTE": {"v": 15}}):
        prog = ix.compile(f)
        assert np.array_equal(ix.select_gpu(prog, k), ix.select_numpy(prog)), f
    for i in range(30000, 31000):
        ix.upsert(str(i), {"v": 30})  # existing value: incremental rank sync
    prog = ix.compile({"GTE": {"v": 30}})
    assert np.array_equal(ix.select_gpu(prog, k), ix.select_numpy(prog))


@pytest.mark.gpu
def test_gpu_group_count():
    k = _kernels()
    ix = _random_collection(50_000, random.Random(3))
    prog = ix.compile({"EQ": {"isCompleted": False}})
    assert ix.group_count_gpu(prog, "taskCreatedBy", k) == ix.group_count_numpy(prog, "taskCreatedBy")


@pytest.mark.gpu
def test_gpu_incremental_sync_and_width_growth():
    k = _kernels()
    rnd = random.Random(11)
    ix = ColumnarIndex(["v", "flag"])
    for i in range(30000):
        ix.upsert(str(i), {"v": rnd.randrange(200), "flag": i % 3 == 0})
    prog = ix.compile({"AND": [{"LT": {"v": 100}}, {"EQ": {"flag": True}}]})
    assert np.array_equal(ix.select_gpu(prog, k), ix.select_numpy(prog))
    assert ix.mirror.widths[ix.col_of["v"]] == 1
    # appends + tombstones + a dictionary that outgrows 8 and then 16 bits
    for i in range(30000, 100000):
        ix.upsert(str(i), {"v": i, "flag": i % 5 == 0})
    for i in rnd.sample(range(100000), 5000):
        ix.delete(str(i))
    for i in rnd.sample(range(100000), 3000):
        ix.upsert(str(i), {"v": rnd.randrange(50), "flag": True})
    for f in ({"AND": [{"LT": {"v": 100}}, {"EQ": {"flag": True}}]}, {"GTE": {"v": 70000}}, {"NEQ": {"flag": True}}):
        prog = ix.compile(f)
        assert np.array_equal(ix.select_gpu(prog, k), ix.select_numpy(prog)), f
    assert ix.mirror.widths[ix.col_of["v"]] == 4
    ix.compact()
    prog = ix.compile({"LT": {"v": 1000}})
    assert np.array_equal(ix.select_gpu(prog, k), ix.select_numpy(prog))


@pytest.mark.gpu
def test_gpu_two_bit_columns():
    """Dictionaries of <= 3 values (booleans, with null) are 2-bit codes on the device: appends
    that end mid-byte, EQ / NEQ / IN / range leaves, ordering and grouping by such a column, and
    the re-encode when the dictionary outgrows 2 bits -- all against the host executors."""
    k = _kernels()
    rnd = random.Random(5)
    ix = ColumnarIndex(["done", "state"])
    flags = [True, False]

    def check(label):
        for f in ({"EQ": {"done": False}}, {"NEQ": {"done": True}}, {"IN": {"state": [None, "b"]}},
                  {"AND": [{"EQ": {"done": True}}, {"GTE": {"state": "b"}}]}, {"OR": [{"EQ": {"state": "a"}}, {"EQ": {"done": True}}]},
                  {"LT": {"done": True}}):
            prog = ix.compile(f)
            want = ix.select_numpy(prog)
            assert np.array_equal(ix.select_gpu(prog, k), want), (label, f)
            assert np.array_equal(ix.select_native(prog, 2), want), (label, f)
        q = {"filter": {"EQ": {"done": False}}, "sort": [{"key": "state", "order": "DESC"}, {"key": "done"}],
             "page": {"limit": 50}}
        assert ix.query(q, k) == ix.query(q), label
        assert ix.group_count_gpu(ix.compile({}), "state", k) == ix.group_count_numpy(ix.compile({}), "state"), label

    n = 0
    for batch in (4097, 3, 1, 20000, 7):  # every append ends at a different row mod 4
        for _ in range(batch):
            d = {"done": rnd.choice(flags)}
            if rnd.random() < 0.9:
                d["state"] = rnd.choice(["a", "b", None])
            ix.upsert(str(n), d)
            n += 1
        check(f"n={n}")
    assert ix.mirror.widths[ix.col_of["done"]] == 0 and ix.mirror.widths[ix.col_of["state"]] == 0
    for i in rnd.sample(range(n), 300):
        ix.delete(str(i))
    check("tombstones")
    ix.upsert("grow", {"done": True, "state": "c"})  # 4 distinct values: the column becomes 1 byte
    check("grown")
    assert ix.mirror.widths[ix.col_of["state"]] == 1


def _interleaved(ix, store, rnd, kernels=None, rounds=12):
    """Repeat the same queries between writes that add dictionary values (new creators, new due
    dates that land between existing ones) and delete rows: memoised programs / ordering plans
    must never answer from a stale dictionary."""
    qs = [{"filter": {"EQ": {"c": "u-new-3"}}},
          {"filter": {"LT": {"d": "2024-05-10"}}, "sort": [{"key": "d", "order": "DESC"}], "page": {"limit": 25}},
          {"filter": {"IN": {"c": ["u1", "u-new-1"]}}, "sort": [{"key": "c"}, {"key": "n", "order": "DESC"}]},
          {"filter": {"OR": [{"GT": {"n": 40}}, {"EQ": {"d": "2024-05-09T12:00:00"}}]}}]
    nxt = [1000]
    for r in range(rounds):
        for q in qs:
            want = [x["key"] for x in json.loads(store.query(json.dumps(q)))["results"]]
            assert ix.query(q, kernels)[0] == want, (r, q)
        for _ in range(300):
            k = str(nxt[0])
            nxt[0] += 1
            d = {"c": rnd.choice(["u0", "u1", "u2", f"u-new-{r}"]),
                 "d": rnd.choice(["2024-05-01T00:00:00", "2024-05-20T00:00:00", f"2024-05-{r % 28 + 1:02d}T12:00:00"]),
                 "n": rnd.randrange(r * 5 + 5)}
            store.set(k, json.dumps(d))
            ix.upsert(k, d)
        for k in rnd.sample(range(1000, nxt[0]), 50):
            store.delete(str(k))
            ix.delete(str(k))


def test_query_caches_follow_dictionary_growth():
    rnd = random.Random(5)
    store = N.DocStore()
    ix = ColumnarIndex(["c", "d", "n"])
    _interleaved(ix, store, rnd)
    assert ix._prog_cache  # the repeated filters were memoised


def test_query_caches_survive_reencode():
    """A source-backed index rebuilds its dictionaries when a column is added: cached programs
    keyed on the old dictionaries must not be reused."""
    store = N.DocStore()
    for i in range(500):
        store.set(str(i), json.dumps({"c": f"u{i % 4}", "d": f"2024-05-{i % 28 + 1:02d}T00:00:00", "n": i % 50}))
    ix = ColumnarIndex.from_source(lambda paths: store.encode_columns("", paths), ["c"])
    q = {"filter": {"EQ": {"c": "u2"}}}
    assert ix.query(q)[0] == [x["key"] for x in json.loads(store.query(json.dumps(q)))["results"]]
    for i in range(0, 500, 4):  # u0 rows go away in the store; the index mirrors the deletes
        store.delete(str(i))
        ix.delete(str(i))
    ix.add_column("d")  # re-encode: u0 leaves the dictionary, ids shift
    assert ix.query(q)[0] == [x["key"] for x in json.loads(store.query(json.dumps(q)))["results"]]
    _interleaved(ix, store, random.Random(6), rounds=4)


@pytest.mark.gpu
def test_gpu_query_caches_follow_dictionary_growth():
    k = _kernels()
    store = N.DocStore()
    ix = ColumnarIndex(["c", "d", "n"])
    _interleaved(ix, store, random.Random(9), kernels=k)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 1000, 70_001])
def test_gpu_interpreter_over_column_widths(n):
    """tt_scan_eval == NumPy on 1-, 2- and 4-byte columns, register and LDS bitmaps, range
    leaves, NOT / OR, and the mask it returns for grouped counts."""
    k = _kernels()
    rnd = random.Random(n)
    ix = ColumnarIndex(["s", "m", "w", "d"], capacity=n)
    for i in range(n):
        ix.upsert(str(i), {"s": rnd.randrange(20), "m": f"m{rnd.randrange(300)}", "w": rnd.randrange(100_000),
                           "d": f"2024-05-{rnd.randrange(1, 29):02d}"} if rnd.random() < 0.95 else {"s": 1})
    for i in rnd.sample(range(n), n // 10):
        ix.delete(str(i))
    filters = [{}, {"EQ": {"s": 3}}, {"NEQ": {"m": "m7"}}, {"IN": {"s": [1, 2, 19]}},
               {"IN": {"m": [f"m{j}" for j in range(0, 300, 7)]}}, {"LT": {"d": "2024-05-10"}},
               {"GTE": {"w": 50_000}}, {"EQ": {"w": 12345}}, {"EQ": {"missing": 1}},
               {"AND": [{"LT": {"d": "2024-05-20"}}, {"NEQ": {"s": 4}}, {"IN": {"m": ["m1", "m2", "m299"]}}]},
               {"OR": [{"EQ": {"s": 5}}, {"GT": {"w": 90_000}}, {"NEQ": {"d": "2024-05-03"}}]},
               {"OR": [{"EQ": {"m": "m3"}}, {"EQ": {"s": 7}}]}]
    for f in filters:
        prog = ix.compile(f)
        want = ix.select_numpy(prog)
        interp, imask = ix.select_gpu(prog, k, return_mask=True)
        assert np.array_equal(interp.cpu().numpy(), want), (n, f)
        bits = imask.cpu().numpy().view(np.uint16)
        rows = np.nonzero(np.unpackbits(bits.view(np.uint8), bitorder="little")[:ix.n])[0]
        assert np.array_equal(rows, want), (n, f)


def torch_equal(a, b):
    import torch
    return bool(torch.equal(a, b))


@pytest.mark.gpu
@pytest.mark.parametrize("ndistinct", [50, 3000, 70_000])
def test_gpu_rank_encode_unaligned_ranges(ndistinct):
    """tt_rank_encode: full encodes and incremental syncs whose [lo, hi) are not multiples of
    16 rows (row-by-row head / tail + vectorised body), 1-, 2- and 4-byte rank columns."""
    k = _kernels()
    rnd = random.Random(ndistinct)
    ix = ColumnarIndex(["v"])
    n0 = 1000 + ndistinct
    for i in range(n0):
        v = i if i < ndistinct else rnd.randrange(ndistinct)  # every value present: width by ndistinct
        ix.upsert(str(i), {"v": v} if i % 13 or i < ndistinct else {"w": 1})
    lo_v = ndistinct // 3
    for f in ({"LT": {"v": lo_v}}, {"GTE": {"v": lo_v}}):
        prog = ix.compile(f)
        assert np.array_equal(ix.select_gpu(prog, k), ix.select_numpy(prog)), f
    assert ix.mirror.ranks[ix.col_of["v"]].w == {50: 1, 3000: 2, 70_000: 4}[ndistinct]
    for extra in (37, 5, 16, 1):  # incremental syncs of existing values (no rank shift)
        base = ix.n
        for i in range(base, base + extra):
            ix.upsert(str(i), {"v": rnd.randrange(ndistinct)})
        prog = ix.compile({"LT": {"v": lo_v}})
        assert np.array_equal(ix.select_gpu(prog, k), ix.select_numpy(prog)), extra


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 5, 2047, 2049, 4097, 8192, 8193, 70_000, 300_001, 3_000_017])
def test_gpu_radix_pair_sort_matches_stable_argsort(n):
    """tt_sort_pairs (hip/radix_pairs.hip, the repo's own LSD radix sort) against NumPy's
    stable argsort of the same keys: every used-bit width from one digit pass to eight, keys
    crowded into few digits (heavy ties: stability decides the order), partial last tiles and
    digit-count tables spanning many scan chunks."""
    import torch
    k = _kernels()
    rng = np.random.default_rng(n)
    for end_bit in (1, 8, 9, 20, 37, 63):
        hi = 1 << end_bit
        keys = rng.integers(0, hi, size=n, dtype=np.uint64)
        if end_bit >= 20:  # a block of equal high digits
            keys[: n // 2] &= np.uint64(0xFF)
        rows = rng.permutation(n).astype(np.int32)
        want = rows[np.argsort(keys, kind="stable")]
        got = k._sorted_rows(torch.from_numpy(keys.view(np.int64)).to(k.device), torch.from_numpy(rows).to(k.device),
                             end_bit)
        assert np.array_equal(got.cpu().numpy(), want), (n, end_bit)
    assert k.check_sort()


def test_sort_fault_is_cleared_and_reported_once():
    """A look-back timeout in the device sort costs the query it hit its device ordering (the
    caller then orders on the host), not every later query."""
    import torch

    from aca_dotnet_workshop_amd.ops.gpu import GpuKernels
    k = GpuKernels.__new__(GpuKernels)
    k.torch = torch
    assert k.check_sort()  # no sort yet
    k._sort_fault = torch.tensor([2], dtype=torch.int32)
    assert not k.check_sort() and k.sort_faults == 1
    assert k.check_sort() and int(k._sort_fault.item()) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("n", [5, 70_000, 300_001])
def test_gpu_ordered_queries_match_the_host(n):
    """Full orderings and top-k pages through the device sort equal the host executor's."""
    k = _kernels()
    ix = _random_collection(n, random.Random(n + 3))
    for sort in ([{"key": "taskDueDate", "order": "DESC"}], [{"key": "taskCreatedBy"}, {"key": "prio", "order": "DESC"}]):
        for page in ({}, {"limit": 25}, {"limit": 40, "token": "7"}):
            q = {"filter": {"EQ": {"isCompleted": False}}, "sort": sort, "page": page}
            assert ix.query(q, k) == ix.query(q), (n, sort, page)


@settings(max_examples=150, deadline=None)
@given(docs_st, filters_st, sort_st, st.integers(0, 1000))
def test_native_mirror_index_matches_native(docs, flt, sort, seed):
    """ColumnarIndex.from_native (the DocStore's own column mirror, deltas pulled by ``sync``)
    answers like the native engine, with writes made only to the store before and after the
    mirror exists and a late column (new mirror generation)."""
    if not docs:
        return
    rnd = random.Random(seed)
    ops = _ops(docs, rnd)
    store = N.DocStore()
    for k, d in ops[: len(ops) // 2]:
        store.delete(k) if d is None else store.set(k, json.dumps(d))
    ix = ColumnarIndex.from_native(store, ["f"])
    for k, d in ops[len(ops) // 2:]:  # the store mirrors these itself
        store.delete(k) if d is None else store.set(k, json.dumps(d))
    ix.sync()
    q = {"filter": flt}
    if sort:
        q["sort"] = sort
    want = json.loads(store.query(json.dumps(q)))["results"]
    rows, _ = ix.query_rows(q)  # may add columns -> new generation, full reload
    got = json.loads(store.mirror_results(rows, "", "", gen=ix.generation)[0])["results"]
    assert got == want


def test_native_mirror_compacts_and_tracks_updates():
    """Updates append rows and kill the old ones; the store compacts its mirror once dead rows
    dominate (new generation) and the index reloads -- it stays proportional to live docs."""
    store = N.DocStore()
    ix = ColumnarIndex.from_native(store, ["n", "done"])
    for i in range(20000):
        store.set(f"k{i}", json.dumps({"n": i % 100, "done": False}))
    q = {"filter": {"AND": [{"LT": {"n": 10}}, {"EQ": {"done": False}}]}, "page": {"limit": 50}}
    ix.sync()
    rows, tok = ix.query_rows(q)
    assert len(rows) == 50 and tok == "50"
    for rnd in range(4):  # rewrite everything 4x: 100k row appends
        for i in range(20000):
            store.set(f"k{i}", json.dumps({"n": i % 100, "done": i % 3 == rnd % 3}))
        ix.sync()
        st_ = store.mirror_stats()
        assert st_["live_rows"] == 20000
        assert st_["rows"] <= 2 * 20000 + 65536
        full = dict(q, page={})
        want = [r["key"] for r in json.loads(store.query(json.dumps(full)))["results"]]
        rows, _ = ix.query_rows(full)
        got = [r["key"] for r in json.loads(store.mirror_results(rows, "", "", gen=ix.generation)[0])["results"]]
        assert got == want
    assert store.mirror_stats()["compactions"] >= 1
    assert ix.n <= 2 * 20000 + 65536


def _compact_mirror(store, n: int) -> None:
    """Rewrite every document until the store compacts its mirror (a new generation)."""
    before = store.mirror_stats()["compactions"]
    for rnd in range(8):
        for i in range(n):
            store.set(f"k{i}", json.dumps({"n": i % 100, "done": True}))
        if store.mirror_stats()["compactions"] > before:
            return
    raise AssertionError("the mirror never compacted")


def test_mirror_results_refuses_rows_of_another_generation():
    """Row numbers selected before a compaction must not be mapped onto the renumbered mirror:
    the store answers None (stale) instead of returning whatever document now sits there."""
    store = N.DocStore()
    n = 40000
    for i in range(n):
        store.set(f"k{i}", json.dumps({"n": i % 100, "done": False}))
    ix = ColumnarIndex.from_native(store, ["n", "done"])
    q = {"filter": {"AND": [{"LT": {"n": 10}}, {"EQ": {"done": False}}]}}
    rows, _ = ix.query_rows(q)
    gen = ix.generation
    assert store.mirror_results(rows, "", "", gen=gen) is not None
    _compact_mirror(store, n)
    assert store.mirror_results(rows, "", "", gen=gen) is None
    ix.sync()
    rows, _ = ix.query_rows(q)
    assert json.loads(store.mirror_results(rows, "", "", gen=ix.generation)[0])["results"] == []


def test_accelerator_reselects_after_a_concurrent_compaction():
    """A compaction that lands between the accelerator's selection and the result lookup (a
    GIL-free native write) makes it re-sync and select again: every returned document matches
    the filter (a stale row could name a completed task for the overdue sweep)."""
    from aca_dotnet_workshop_amd.backing.accel import CollectionAccelerator
    store = N.DocStore()
    n = 40000
    for i in range(n):
        store.set(f"k{i}", json.dumps({"n": i % 100, "done": i % 2 == 0}))
    acc = CollectionAccelerator("cpu", 0)
    q = {"filter": {"AND": [{"LT": {"n": 10}}, {"EQ": {"done": False}}]}}
    assert acc.query(q, "", store) is not None  # builds the mirror-fed index
    real = acc.index.query_rows
    fired = []

    def racing_query_rows(qq, k=None):
        out = real(qq, k)
        if not fired:  # the race: the store compacts right after the selection
            fired.append(1)
            for rnd in range(8):
                for i in range(n):
                    store.set(f"k{i}", json.dumps({"n": (i + 7) % 100, "done": (i + rnd) % 3 == 0}))
                if store.mirror_stats()["compactions"]:
                    break
        return out
    acc.index.query_rows = racing_query_rows
    res = json.loads(acc.query(q, "", store))["results"]
    assert fired and acc.stats.get("stale_retries", 0) >= 1
    want = json.loads(store.query(json.dumps(q)))["results"]
    assert sorted(r["key"] for r in res) == sorted(r["key"] for r in want)
    assert all(r["data"]["n"] < 10 and not r["data"]["done"] for r in res)


@pytest.mark.gpu
def test_gpu_native_mirror_matches_native():
    """The GPU path over a native-mirror index (incremental device sync of appended rows and
    killed rows) equals the native engine after interleaved writes."""
    k = _kernels()
    rnd = random.Random(11)
    store = N.DocStore()
    for i in range(30000):
        store.set(f"k{i}", json.dumps({"d": f"2024-05-{rnd.randrange(1, 29):02d}T00:00:00",
                                       "c": rnd.random() < 0.3, "o": False}))
    ix = ColumnarIndex.from_native(store, ["d", "c", "o"])
    q = {"filter": {"AND": [{"LT": {"d": "2024-05-15T00:00:00"}}, {"EQ": {"c": False}}, {"EQ": {"o": False}}]},
         "sort": [{"key": "d"}]}
    for round_ in range(5):
        ix.sync()
        rows, _ = ix.query_rows(q, k)
        got = [r["key"] for r in json.loads(store.mirror_results(rows, "", "", gen=ix.generation)[0])["results"]]
        want = [r["key"] for r in json.loads(store.query(json.dumps(q)))["results"]]
        assert got == want, round_
        for _ in range(3000):  # mark some overdue, complete some, add new due dates, delete some
            i = rnd.randrange(40000)
            r = rnd.random()
            if r < 0.1:
                store.delete(f"k{i}")
            else:
                store.set(f"k{i}", json.dumps({"d": f"2024-0{rnd.randrange(4, 7)}-{rnd.randrange(1, 29):02d}T00:00:00",
                                               "c": r < 0.4, "o": r > 0.8}))


@pytest.fixture(params=["native", "numpy"])
def rank_path(request, monkeypatch):
    """The string ranks both ways: native/src/strrank.hpp, and the numpy merge it replaced."""
    from aca_dotnet_workshop_amd.ops import columnar
    if request.param == "numpy":
        monkeypatch.setattr(columnar, "_NATIVE", [None])
    else:
        assert columnar._native_module() is not None
    return request.param


@settings(max_examples=200, deadline=None, suppress_health_check=[HealthCheck.function_scoped_fixture])
@given(st.lists(st.lists(st.text(max_size=6), max_size=30), min_size=1, max_size=6))
def test_string_ranks_incremental_match_the_comparison_sort(rank_path, batches):
    """The incremental string-dictionary ranks (merge of each batch of new values) equal the
    general comparison sort after every batch; a non-string value switches to the general path."""
    from aca_dotnet_workshop_amd.ops.columnar import Column
    c = Column("p")
    for b in batches:
        for v in b:
            c.encode(v)
        c._rank_cache = None
        assert c.ranks().tolist() == c._general_ranks().tolist()
    c.encode(5)
    c._rank_cache = None
    assert c.ranks().tolist() == c._general_ranks().tolist()


def test_bulk_string_encode_and_append_ranks(rank_path):
    """``encode_json_many`` (the mirror sync's bulk path) gives the ids per-value ``encode``
    would, the in-place append path (every new value sorts last: new timestamps) keeps the ranks
    equal to the comparison sort, a value already present falls back per value, and non-string
    or NUL-terminated values leave the string-only path."""
    import json as _json
    from aca_dotnet_workshop_amd.ops.columnar import Column
    a, b = Column("p"), Column("p")
    ts = [f"2026-10-17T10:{m:02d}:{s:02d}" for m in range(60) for s in range(0, 60, 7)]
    for lo in range(0, len(ts), 97):  # ascending batches: the append path
        batch = ts[lo:lo + 97]
        got = a.encode_json_many([_json.dumps(x) for x in batch])
        assert got.tolist() == [b.encode(x) for x in batch]
        a._rank_cache = None
        assert a.ranks().tolist() == a._general_ranks().tolist()
    older = ["2026-10-16T00:00:0" + str(i) for i in range(5)] + ["z\"q\u00e9"]
    a.encode_json_many([_json.dumps(x) for x in older])  # sorts before the old values: the merge path
    a._rank_cache = None
    assert a.ranks().tolist() == a._general_ranks().tolist() and a.str_only
    n = len(a.values)
    assert a.lookup(ts[5]) == 5 and a.lookup("z\"q\u00e9") == n - 1 and len(a.ids) == n  # keyed on first use
    assert a.encode(ts[3]) == 3 and a.encode("new") == n and a.lookup("new") == n
    a.encode_json_many([_json.dumps("nul\x00")])
    assert not a.str_only
    a._rank_cache = None
    assert a.ranks().tolist() == a._general_ranks().tolist()
    assert a.encode_json_many(["1", "true", "null"]).tolist() == [a.lookup(1), a.lookup(True), a.lookup(None)]


class _FakePageKernels:
    """The page path's kernels (hip/page_topk.hip) emulated on the host over the index's own
    arrays: what ``ref_page`` of test_gpu_kernel_edges is checked against.  The page-path tests
    below run over ``HostKernels`` (test_device_mirror_state), which answers from the buffers the
    mirror uploaded, so ``ColumnarIndex.page_gpu``'s zone maps, tile choice, retries and
    continuation tokens -- and the uploads under them -- run in the CPU suite; the real kernels
    are pinned by the GPU tests."""

    def __init__(self, ix, cap=8192):
        import torch
        self.torch, self.device, self.page_cap, self.max_sort_keys = torch, torch.device("cpu"), cap, 4
        self.ix, self.prog, self.sort = ix, None, None
        self.calls = {"zone_tiles": 0, "page_tiles": 0, "pages": 0}

    def rank_encode(self, *a):  # device rank columns are not read by the emulation
        pass

    def upload(self, segments):  # GpuKernels.upload, on host tensors: the same bytes written in place
        import ctypes
        for dst, a in segments:
            b = np.ascontiguousarray(a)
            ctypes.memmove(int(dst), b.ctypes.data, b.nbytes)

    def _keys(self, rows):
        return self.ix.sort_keys_numpy(rows, self.ix.sort_specs(self.sort)).astype(np.uint64)

    def zone_argmin(self, table, live16, nrows, specs, ranks, seq, seq_bits, tiles):
        ix, out = self.ix, []
        self.calls["zone_tiles"] += len(tiles)
        for t in tiles.tolist():
            rows = np.arange(t * 8192, min((t + 1) * 8192, ix.n))
            rows = rows[ix.live[rows] != 0]
            out.append(int(rows[np.argmin(self._keys(rows))]) if rows.size else -1)
        return np.asarray(out, dtype=np.int32)

    def page(self, table, live16, nrows, prog, bitmaps, specs, ranks, seq, seq_bits, tiles, k, offset, bound):
        self.calls["pages"] += 1
        self.calls["page_tiles"] += len(tiles)
        sel = self.ix.select_numpy(self.prog)
        sel = sel[np.isin(sel // 8192, tiles)]
        keys = self._keys(sel)
        sel = sel[keys < np.uint64(bound)] if bound != np.iinfo(np.uint64).max else sel
        keys = self._keys(sel)
        total = sel.size
        order = sel[np.argsort(keys, kind="stable")][: self.page_cap]
        n = min(total, self.page_cap)
        if total > self.page_cap:
            complete = False
        elif n >= k:
            complete = True
        else:
            complete = bound == np.iinfo(np.uint64).max
        return order[offset:min(n, k)].astype(np.int32), total, complete

    def select(self, table, live16, capacity, nrows, prog, bitmaps, return_mask=False):
        return self.torch.from_numpy(self.ix.select_numpy(self.prog))


@settings(max_examples=20, deadline=None)
@given(st.integers(0, 10_000), st.sampled_from([None, [{"key": "c"}], [{"key": "d", "order": "DESC"}, {"key": "c"}]]),
       st.sampled_from([1, 7, 100, 900]))
def test_page_path_host_logic_matches_full_order(seed, sort, limit):
    """page_gpu (zone maps + tile choice + bound check + token) walks the same pages as the full
    host query, through interleaved writes that dirty tiles, for sorted and unsorted queries."""
    rnd = random.Random(seed)
    ix = ColumnarIndex(["c", "d", "x"])
    for i in range(30_000):
        ix.upsert(f"k{i}", {"c": f"2025-01-{rnd.randrange(1, 29):02d}T{rnd.randrange(24):02d}:00:00",
                            "d": rnd.randrange(50), "x": rnd.random() < 0.2})
    from test_device_mirror_state import HostKernels
    fk = HostKernels()  # answers from what the mirror uploaded, not from the index
    flt = {"AND": [{"EQ": {"x": False}}, {"LT": {"d": 40}}]}
    for rnd_ in range(3):
        q = {"filter": flt, **({"sort": sort} if sort else {})}
        full, _ = ix.query(q)
        prog = ix.compile(flt)
        got, token, ended = [], None, False
        for _ in range(25):
            off = int(token or 0)
            res = ix.page_gpu(prog, sort, fk, off, limit)
            if res is None:  # keys not clustered by tile / past what one workgroup sorts: the full path's job
                assert sort is not None or off + limit > 1000
                break
            rows, token = res
            got += [ix.keys[r] for r in rows.tolist()]
            if token is None:
                ended = True
                break
        assert got == full[:len(got)] and (not ended or got == full), (rnd_, len(got), len(full))
        for _ in range(500):  # dirty some tiles: updates re-append rows, deletes kill them
            i = rnd.randrange(30_000)
            if rnd.random() < 0.2:
                ix.delete(f"k{i}")
            else:
                ix.upsert(f"k{i}", {"c": f"2025-01-{rnd.randrange(1, 29):02d}T00:00:00", "d": rnd.randrange(50),
                                    "x": rnd.random() < 0.2})
    # the zone maps did their job: pages read a few tiles, not the collection
    assert fk.calls["page_tiles"] / max(1, fk.calls["pages"]) < (ix.n + 8191) // 8192


def test_device_sort_plan_grows_in_place_and_matches_the_host_keys():
    """The paged path's sort plan keeps its rank tables across queries: new timestamps that sort
    last only append their ranks (same device buffer, rebuilt only when its capacity doubles);
    values landing inside the order re-copy the ids whose rank moved.  The packed keys it yields
    always equal the host reference's."""
    import torch
    from test_device_mirror_state import HostKernels, assert_mirror_matches_index
    ix = ColumnarIndex(["c", "d"])
    fk = HostKernels()  # uploads copy: the device table below is a buffer of its own
    sort = [{"key": "c"}, {"key": "d", "order": "DESC"}]

    def check():
        hit = ix.mirror.sort_plan(sort, fk)
        rows = np.nonzero(ix.live[:ix.n])[0]
        want = ix.sort_keys_numpy(rows, ix.sort_specs(sort))
        assert np.array_equal(ix.sort_keys_numpy(rows, hit[4]), want)
        assert not np.shares_memory(hit[1].numpy(), hit[4][1])
        assert torch.equal(hit[1], torch.from_numpy(hit[4][1]))  # device table == host table
        ix.mirror.sync(fk)
        assert_mirror_matches_index(ix, fk, lambda t: t.numpy(), plans=[sort])  # ... == the keys' rank tables
        return hit
    for i in range(3000):
        ix.upsert(f"k{i}", {"c": f"2026-01-01T00:{i // 60:02d}:{i % 60:02d}", "d": i % 7})
    buf, rebuilds = check()[1], 0
    for lo in range(3000, 9000, 500):  # newer timestamps only: appended in place
        for i in range(lo, lo + 500):
            ix.upsert(f"k{i}", {"c": f"2026-01-02T{i // 3600:02d}:{i // 60 % 60:02d}:{i % 60:02d}", "d": i % 7})
        hit = check()
        rebuilds += hit[1] is not buf
        buf = hit[1]
    assert rebuilds <= 2  # capacity doublings only (3,000 -> 9,000 ranks)
    # a batch slightly out of order (concurrent writers): the newest old ids move up by one
    col = ix.columns[ix.col_of["c"]]
    ix.upsert("late-1", {"c": "2026-01-02T02:29:58.5", "d": 1})
    ix.upsert("late-2", {"c": "2026-01-02T02:30:01", "d": 1})
    col.ranks()
    assert col._rank_lo >= len(col.values) - 10  # only the newest ids' ranks changed
    check()
    ix.upsert("old", {"c": "2025-12-31T00:00:00", "d": 3})  # sorts first: every rank moves
    check()
    ix.upsert("k5", {"c": "2026-01-03T00:00:00", "d": 99})   # update: a new row, a new d value
    check()


def test_page_path_overflow_and_tiny_cap_fall_back():
    """More candidates than the device top-k holds: fewer tiles are taken, and a page that
    cannot fit at all is left to the full path (None)."""
    ix = ColumnarIndex(["c"])
    for i in range(40_000):
        ix.upsert(f"k{i}", {"c": i // 40})  # clustered by tile, like a creation timestamp
    from test_device_mirror_state import HostKernels
    fk = HostKernels()  # the device cap is one tile: a single tile always fits
    sort = [{"key": "c"}]
    prog = ix.compile({})
    rows, token = ix.page_gpu(prog, sort, fk, 0, 100)
    assert [ix.keys[r] for r in rows] == ix.query({"sort": sort, "page": {"limit": 100}})[0] and token == "100"
    assert ix.page_gpu(prog, sort, fk, 8100, 200) is None  # beyond the capacity
    fk.page_cap = 16  # a tile's matches alone overflow: the full path answers
    assert ix.page_gpu(prog, sort, fk, 0, 10) is None


@pytest.mark.gpu
@pytest.mark.parametrize("sort", [None, [{"key": "c"}], [{"key": "d", "order": "DESC"}, {"key": "c"}]])
def test_gpu_page_path_matches_host(sort):
    """hip/page_topk.hip (zone argmins, gather of the chosen tiles, LDS bitonic top-k) pages
    exactly like the host path -- rows and continuation tokens -- over a collection whose sort
    key is clustered by insertion (a creation timestamp), through updates that re-append rows
    and deletes that kill them."""
    k = _kernels()
    rnd = random.Random(3)
    ix = ColumnarIndex(["c", "d", "x"])
    n = 120_000
    for i in range(n):
        ix.upsert(f"k{i}", {"c": f"2025-03-01T{i // 3600:02d}:{i // 60 % 60:02d}:{i % 60:02d}",
                            "d": rnd.randrange(40), "x": rnd.random() < 0.3})
    flt = {"AND": [{"EQ": {"x": False}}, {"LT": {"d": 30}}]}
    used = 0
    for round_ in range(3):
        q = {"filter": flt, **({"sort": sort} if sort else {})}
        for limit in (1, 64, 1000):
            token = None
            for _ in range(3):
                page = {"limit": limit, **({"token": token} if token else {})}
                before = ix.mirror.zones.copy()
                got = ix.query({**q, "page": page}, k)
                want = ix.query({**q, "page": page})
                assert got == want, (round_, limit, token)
                used += bool(ix.mirror.zones) or bool(before)
                token = got[1]
                if token is None:
                    break
        for _ in range(4000):  # updates land at the end (new tiles), deletes punch holes
            i = rnd.randrange(n)
            if rnd.random() < 0.2:
                ix.delete(f"k{i}")
            else:
                ix.upsert(f"k{i}", {"c": f"2025-03-01T{i // 3600:02d}:{i // 60 % 60:02d}:{i % 60:02d}",
                                    "d": rnd.randrange(40), "x": rnd.random() < 0.3})
    assert used and ix.mirror.zones


@pytest.mark.gpu
@pytest.mark.parametrize("n,wide", [(0, False), (1, False), (63, False), (64, False), (65, False), (700, False),
                                    (1023, False), (1024, False), (1025, False), (2583, False), (2583, True),
                                    (4096, False), (4097, True), (8191, False), (8192, True)])
def test_gpu_page_topk_sorts_every_candidate_count(n, wide):
    """tt_page_topk (bitonic sort of all candidates, or -- more candidates than the page --
    a radix select of the k-th key, compaction of the k smallest and a sort of those) returns the
    [offset, k) slice of the key order for every candidate count up to the LDS capacity, for
    clustered and full-width 63-bit keys, with the completeness flag the host relies on."""
    import torch
    k = _kernels()
    rng = np.random.default_rng(n)
    if wide:  # keys over the whole 63-bit range
        keys = np.unique(rng.integers(0, np.iinfo(np.int64).max, n + 64, dtype=np.int64))[:n]
        rng.shuffle(keys)
    else:  # clustered: a narrow band, like one tile's packed keys
        keys = (rng.integers(0, 1 << 40, n, dtype=np.int64) << 20) | np.arange(n, dtype=np.int64)
    rows = rng.permutation(n).astype(np.int32)
    dk, dr = torch.from_numpy(keys).to(k.device), torch.from_numpy(rows).to(k.device)
    order = rows[np.argsort(keys.astype(np.uint64), kind="stable")]
    for kk, off in ((1, 0), (1000, 0), (1000, 400), (8192, 0), (64, 64)):
        got, info = k.page_topk(dk, dr, kk, off, np.iinfo(np.uint64).max)
        assert got.tolist() == order[off:min(n, kk)].tolist(), (n, kk, off)
        assert info[0] == n and info[2] == max(0, min(n, kk) - off)
        assert info[1] == 1  # bound = all tiles read: complete
    got, info = k.page_topk(dk, dr, 1000, 0, 12345)  # a bound: complete only with k candidates
    assert info[1] == (1 if n >= 1000 else 0)
    # the phase clocks (scripts/topk_phases.py): the stamps a branch writes never go backwards,
    # and setting them does not change the answer
    stamps = torch.zeros(6, dtype=torch.int64, device=k.device)
    got, info = k.page_topk(dk, dr, 1000, 0, np.iinfo(np.uint64).max, stamps=stamps)
    assert got.tolist() == order[:min(n, 1000)].tolist()
    s = [int(x) for x in stamps.cpu().tolist() if x != 0]
    assert len(s) >= 4 and s == sorted(s)


@pytest.mark.gpu
def test_gpu_select_grows_past_its_estimated_output():
    """tt_scan_compact sizes its output from the previous count of the same program; a
    selection that outgrew that estimate is compacted again into an exact buffer."""
    k = _kernels()
    ix = ColumnarIndex(["v"])
    for i in range(60_000):
        ix.upsert(str(i), {"v": 1 if i < 100 else 0})
    prog = ix.compile({"EQ": {"v": 1}})
    assert np.array_equal(ix.select_gpu(prog, k), ix.select_numpy(prog))  # 100 rows: the estimate
    assert np.array_equal(ix.select_gpu(prog, k), ix.select_numpy(prog))  # sized from it
    for i in range(100, 40_000):
        ix.upsert(str(i), {"v": 1})
    got, want = ix.select_gpu(prog, k), ix.select_numpy(prog)
    assert got.size == want.size == 40_000 and np.array_equal(got, want)


@pytest.mark.gpu
def test_gpu_zone_argmin_matches_numpy():
    k = _kernels()
    rnd = random.Random(8)
    ix = ColumnarIndex(["c"])
    for i in range(50_000):
        ix.upsert(str(i), {"c": rnd.randrange(1000)})
    for i in rnd.sample(range(50_000), 9000):
        ix.delete(str(i))
    sort = [{"key": "c", "order": "DESC"}]
    specs_t, ranks_t, seq_bits, _, plan = ix.mirror.sort_plan(sort, k)
    m = ix.mirror.sync(k)
    tiles = np.arange((ix.n + TILE_ROWS - 1) // TILE_ROWS, dtype=np.int32)
    got = k.zone_argmin(m.table, m.live, ix.n, specs_t, ranks_t, m.seq, seq_bits, tiles)
    for t, r in zip(tiles.tolist(), got.tolist()):
        rows = np.arange(t * TILE_ROWS, min((t + 1) * TILE_ROWS, ix.n))
        rows = rows[ix.live[rows] != 0]
        want = int(rows[np.argmin(ix.sort_keys_numpy(rows, plan))]) if rows.size else -1
        assert r == want, t


TILE_ROWS = 8192


@pytest.mark.gpu
def test_gpu_scatter_upload_writes_every_segment():
    """GpuKernels.upload (hip/mirror_upload.hip): segments of every size and destination
    alignment -- 1..70 KB, odd byte offsets, 2- and 4-byte aligned, 16-byte aligned -- land
    exactly where they go in one launch, and nothing around them changes."""
    import torch
    k = _kernels()
    rng = np.random.default_rng(7)
    dst = torch.zeros(1 << 20, dtype=torch.uint8, device=k.device)
    want = np.zeros(1 << 20, dtype=np.uint8)
    segs, at = [], 0
    for size in (1, 3, 15, 16, 17, 31, 33, 255, 4096, 4097, 70000, 5, 64):
        at += int(rng.integers(1, 40))  # any alignment
        payload = rng.integers(0, 256, size=size, dtype=np.uint8)
        segs.append((dst.data_ptr() + at, payload))
        want[at:at + size] = payload
        at += size
    for align in (2, 4, 16):
        at = (at + align - 1) // align * align
        payload = rng.integers(0, 256, size=1000 + align, dtype=np.uint8)
        segs.append((dst.data_ptr() + at, payload))
        want[at:at + payload.size] = payload
        at += payload.size
    words = rng.integers(-5, 5, size=333).astype(np.int32)  # typed payloads go up as their bytes
    at = (at + 3) // 4 * 4
    segs.append((dst.data_ptr() + at, words))
    want[at:at + 4 * words.size] = words.view(np.uint8)
    before = k.uploads
    k.upload(segs)
    torch.cuda.synchronize()
    assert np.array_equal(dst.cpu().numpy(), want)
    assert k.uploads == before + 1
    k.upload([])  # nothing to write: no launch
    assert k.uploads == before + 1


@pytest.mark.gpu
def test_gpu_upload_ring_reuses_its_slots_in_order():
    """Back-to-back uploads with no synchronise between them cycle through the staging ring
    (GpuKernels.UPLOAD_SLOTS pinned slots, each reused once the scatter that read it has
    finished -- its event, not a stream synchronise): later writes to the same bytes win in
    order, growing payloads re-allocate a slot safely, and every segment lands."""
    import torch
    k = _kernels()
    rng = np.random.default_rng(11)
    dst = torch.zeros(1 << 18, dtype=torch.int32, device=k.device)
    want = np.zeros(1 << 18, dtype=np.int32)
    for step in range(5 * k.UPLOAD_SLOTS):
        size = int(rng.integers(1, 4096)) * (1 + step)  # growing: slots re-allocate on the way
        at = int(rng.integers(1, want.size - size))  # the two segments of one launch never overlap
        payload = rng.integers(-1000, 1000, size=size).astype(np.int32)
        k.upload([(dst.data_ptr() + 4 * at, payload), (dst.data_ptr(), np.array([step], dtype=np.int32))])
        want[at:at + size] = payload
        want[0] = step
    torch.cuda.synchronize()
    assert np.array_equal(dst.cpu().numpy(), want)


@pytest.mark.gpu
def test_gpu_sweep_query_tracks_a_growing_native_mirror():
    """The sweep's query on the GPU (range on taskDueDate, two booleans, ORDER BY taskCreatedOn,
    a page) against the host's answer, round after round of writes to a native mirror: new due
    dates re-rank their column (rank tables re-sent into kept buffers), created stamps arrive a
    little out of order (native string ranks merge them into the tail), completions and
    overdue marks kill rows, the filter program stays cached across the sort column's growth,
    and every upload goes through the staging ring."""
    import json as _json
    from aca_dotnet_workshop_amd.native import load
    N = load()
    rnd = random.Random(5)
    store = N.DocStore("", 0, 256)
    prefix = "api||"

    def put(i, due_day, done=False, over=False, jitter=0):
        us = 1000 * i + jitter
        doc = {"taskId": f"{i:08d}-0000-0000-0000-000000000000", "taskName": f"t{i}",
               "taskCreatedOn": f"2025-01-01T{us // 3_600_000_000 % 24:02d}:{us // 60_000_000 % 60:02d}:"
                                f"{us // 1_000_000 % 60:02d}.{us % 1_000_000:06d}0",
               "taskDueDate": f"2024-{1 + due_day // 28:02d}-{1 + due_day % 28:02d}T00:00:00",
               "isCompleted": done, "isOverDue": over}
        store.set(f"{prefix}{i:08d}", _json.dumps(doc))

    n = 0
    for _ in range(30_000):
        put(n, rnd.randrange(60))
        n += 1
    paths = ["\u0000keyprefix", "taskDueDate", "isCompleted", "isOverDue", "taskCreatedOn"]
    ix = ColumnarIndex.from_native(store, paths)
    k = _kernels()
    q = {"filter": {"AND": [{"EQ": {"\u0000keyprefix": prefix}},
                            {"AND": [{"LT": {"taskDueDate": "2024-02-15T00:00:00"}}, {"EQ": {"isCompleted": False}},
                                     {"EQ": {"isOverDue": False}}]}]},
         "sort": [{"key": "taskCreatedOn", "order": "ASC"}], "page": {"limit": 500}}
    for rnd_i in range(12):
        for _ in range(1500):  # new tasks, a few with due dates never seen before, stamps a little shuffled
            put(n, rnd.randrange(60 + rnd_i * 3), jitter=rnd.randrange(-3000, 3000))
            n += 1
        for _ in range(200):  # completions and overdue marks of older tasks
            i = rnd.randrange(n)
            put(i, rnd.randrange(60), done=rnd.random() < 0.5, over=rnd.random() < 0.5)
        ix.sync()
        gpu_rows, gpu_tok = ix.query_rows(q, k)
        host_rows, host_tok = ix.query_rows(q, None)
        assert gpu_rows.tolist() == host_rows.tolist() and gpu_tok == host_tok, rnd_i
    assert k.uploads > 12
