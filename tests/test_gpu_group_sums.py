"""``tt_scan_sums`` (ops/hip/group_sums.hip), the fused filter + per-group exact sums of one numeric
key, over synthetic device tables: every ``nums`` / ``sum`` / ``abs`` word compared for equality with
``ref_sums`` below -- ``ref_select``, then per cell a count and two integer sums of ``table[id]`` --
at every row count around a 16-row group and a tile, on one, two and all blocks, on every value id
width, with missing ids, ids past the number table and the not-a-number entry among the rows, with
magnitudes that carry past 32 bits, either side of the interleaved copies and of the LDS / global
switch, at the cell cap, with the leaf bitmaps staged in LDS and left in global memory; two
launches into one triple; the same launch twice; and ``ColumnarIndex.aggregate`` on the device.
A guard region behind each output must stay zero.  ``ref_sums`` itself is compared with
``ColumnarIndex.sums_numpy`` in the CPU suite (``test_aggregate_sums``).
"""
import math

import numpy as np
import pytest

from aca_dotnet_workshop_amd.ops.columnar import NOT_A_NUMBER, OP_AND, OP_LEAF, OP_RANGE, OP_TRUE, ColumnarIndex

from test_aggregate_query import brute
from test_gpu_kernel_edges import MAX_ID, TILE, _Synth, _dev, _ids, _limits, k, ref_select  # noqa: F401

pytestmark = pytest.mark.gpu
GUARD = 256  # words past each output that no launch may touch
NO_BITMAPS = np.zeros(1, dtype=np.uint32)
TRUE = [[OP_TRUE, 0, 0, 0]]


def ref_sums(T, code, bitmaps, keys, dims, vcol, table):
    """(nums uint32, sum int64, abs uint64 [prod(dims + 1)]) and the selected rows left out for a
    missing id, an id past ``table`` and a not-a-number entry: cells as ``tt_scan_group``'s."""
    rows = ref_select(T.cols, T.live, T.n, code, bitmaps)
    cell = np.zeros(rows.size, dtype=np.int64)
    keep = np.ones(rows.size, dtype=bool)
    for c, d in zip(keys, dims):
        ids = np.asarray(T.cols[c][0], dtype=np.int64)[rows]
        keep &= (ids >= -1) & (ids < d)
        cell = cell * (d + 1) + np.where(ids == -1, d, ids)
    val = np.asarray(T.cols[vcol][0], dtype=np.int64)[rows]
    table = np.asarray(table, dtype=np.int64)
    inside = (val >= 0) & (val < table.size)
    m = np.concatenate([table, [NOT_A_NUMBER]])[np.where(inside, val, table.size)]
    ok = keep & (m != NOT_A_NUMBER)
    ncells = math.prod(d + 1 for d in dims)
    cnt = np.bincount(cell[ok], minlength=ncells).astype(np.uint32)
    s, a = np.zeros(ncells, dtype=np.int64), np.zeros(ncells, dtype=np.uint64)
    np.add.at(s, cell[ok], m[ok])
    np.add.at(a, cell[ok], np.abs(m[ok]).astype(np.uint64))
    left = (int((keep & (val == -1)).sum()), int((keep & (val >= table.size)).sum()),
            int((keep & inside & (m == NOT_A_NUMBER)).sum()))
    return (cnt, s, a), left


def _buffers(k, ncells):
    import torch
    return (torch.zeros(ncells + GUARD, dtype=torch.int32, device=k.device),
            torch.zeros(ncells + GUARD, dtype=torch.int64, device=k.device),
            torch.zeros(ncells + GUARD, dtype=torch.int64, device=k.device))


def _host(bufs):
    return (bufs[0].cpu().numpy().view(np.uint32), bufs[1].cpu().numpy(), bufs[2].cpu().numpy().view(np.uint64))


def _sums(k, T, code, bitmaps, keys, dims, vcol, table, max_blocks=0, n=None, bufs=None):
    """The kernel's three outputs, after checking that the guard region behind each is untouched."""
    code = np.asarray(code, dtype=np.int32).reshape(-1, 4)
    ncells = math.prod(d + 1 for d in dims)
    bufs = _buffers(k, ncells) if bufs is None else bufs
    out = k.scan_sums(T.table, T.live16, T.cap, T.n if n is None else n, _dev(k, code),
                      _dev(k, np.asarray(bitmaps, dtype=np.uint32)), keys, dims, vcol,
                      _dev(k, np.asarray(table, dtype=np.int64)), max_blocks, out=bufs)
    assert out is bufs
    got = _host(bufs)
    assert not any(g[ncells:].any() for g in got), "wrote past the outputs"
    return tuple(g[:ncells] for g in got)


def _same(got, want):
    return all(np.array_equal(g, w) for g, w in zip(got, want))


# columns of the shared table: (index, dictionary size)
G0, G1, GBIG, BIG4, FLT, W2, V0, V1, V2, V4 = range(10)
SIZE = {G0: 1, G1: 64, GBIG: 4096, BIG4: 2047, FLT: 10, W2: 300}
VALUES = {V0: 0, V1: 1, V2: 2, V4: 4}   # value column -> width
NROWS = [0, 1, 15, 16, 17, TILE - 1, TILE, TILE + 1, 3 * TILE + 5]


def _number_table(rng, size):
    """``size`` scaled integers up to +-2^45 (a handful of rows carry a sum past 32 bits), the
    extremes of that range in entries 0 and 1, every seventh entry no number."""
    t = rng.integers(-(1 << 45), 1 << 45, size, dtype=np.int64)
    t[:2] = [(1 << 45) - 1, -(1 << 45)][:size]
    t[6::7] = NOT_A_NUMBER
    return t


@pytest.fixture(scope="module")
def table(k):
    """n = 3 tiles + 5 rows in a capacity of 4 tiles, ~10 % dead rows below n, every row past the
    16-row group of row n live and full: only the kernel's own row bound keeps those out.  The
    value columns hold every id of their width, ~10 % missing; their number tables are shorter
    than the ids they hold (the two-bit one apart) and hold not-a-number entries."""
    rng = np.random.default_rng(61)
    n, cap = 3 * TILE + 5, 4 * TILE
    cols = [(_ids(rng, cap, SIZE[G0] + 1), 0), (_ids(rng, cap, SIZE[G1] + 1), 1), (_ids(rng, cap, SIZE[GBIG] + 1), 2),
            (_ids(rng, cap, SIZE[BIG4]), 4), (_ids(rng, cap, SIZE[FLT], missing=0.0), 1), (_ids(rng, cap, SIZE[W2]), 2)]
    live = rng.random(cap) < 0.9
    live[[0, 15, 16, n - 1]] = True
    live[n:(n + 15) // 16 * 16] = False
    live[(n + 15) // 16 * 16:] = True
    for w in VALUES.values():
        v = _ids(rng, cap, min(MAX_ID[w] + 1, 100_000))
        v[[0, 15, 16, n - 1]] = [0, 1, 2, 0]
        v[n:] = np.where(v[n:] < 0, 1, v[n:])  # rows past n all hold a value
        cols.append((v, w))
    T = _Synth(k, cols, live, n, cap)
    T.nums = {V0: np.array([(1 << 40) + 1, -(1 << 40), NOT_A_NUMBER], dtype=np.int64), V1: _number_table(rng, 200),
              V2: _number_table(rng, 60_000), V4: _number_table(rng, 90_000)}
    return T


HALF = [[OP_RANGE, FLT, 0, 5]]


@pytest.mark.parametrize("keys,dims", [([], []), ([G0], [1]), ([G1], [63]), ([G1], [64]), ([GBIG], [4095]),
                                       ([GBIG], [4096]), ([G0, G1], [1, 64])])
def test_row_counts_blocks_and_value_widths(k, table, keys, dims):
    """1, 2, 64, 65, 4096, 4097 and 130 cells -- registers, interleaved copies, LDS cells, global
    cells -- over every row count and value id width, on the default grid and on one and two
    blocks (a block walks several tiles)."""
    import types
    assert math.prod(d + 1 for d in dims) in (1, 2, 64, 65, 4096, 4097, 130)
    for n in NROWS:
        T = types.SimpleNamespace(cols=table.cols, live=table.live, n=(n + 15) // 16 * 16)  # the bound is the group's
        for vcol in VALUES:
            want, left = ref_sums(T, TRUE, NO_BITMAPS, keys, dims, vcol, table.nums[vcol])
            for max_blocks in (0, 1, 2):
                got = _sums(k, table, TRUE, NO_BITMAPS, keys, dims, vcol, table.nums[vcol], max_blocks, n=n)
                assert _same(got, want), (n, vcol, max_blocks)
            if n >= TILE - 1:  # missing ids, ids past the table (not the 2-bit one) and not-a-number entries
                assert left[0] > 0 and left[2] > 0 and (left[1] > 0 or vcol == V0), left
    # the whole table: magnitudes past 32 bits, and the signed sum differs from them
    assert int(want[2].max()) > 1 << 40 and not np.array_equal(want[1].view(np.uint64), want[2])
    assert n == table.n


def test_sums_carry_past_32_bits_in_every_mode(k, table):
    for keys, dims in (([], []), ([G0], [1]), ([G1], [64]), ([GBIG], [4096])):
        want, _ = ref_sums(table, HALF, NO_BITMAPS, keys, dims, V0, table.nums[V0])
        got = _sums(k, table, HALF, NO_BITMAPS, keys, dims, V0, table.nums[V0])
        assert _same(got, want)
        # +-2^40 cancel in the signed sum and add up in the magnitudes
        assert int(got[2].sum()) > 1000 << 40 and abs(int(got[1].sum())) < int(got[2].sum()) // 4


def test_cell_cap_and_bad_arguments(k, table):
    """Exactly ``tt_group_max_cells()`` cells are summed; one product above is refused by the
    launcher, which launches nothing; so is every malformed argument."""
    import torch
    cap = int(k.lib.tt_group_max_cells())
    assert cap == 2048 * 2048
    want, _ = ref_sums(table, HALF, NO_BITMAPS, [BIG4, BIG4], [2047, 2047], V4, table.nums[V4])
    got = _sums(k, table, HALF, NO_BITMAPS, [BIG4, BIG4], [2047, 2047], V4, table.nums[V4])
    assert _same(got, want) and int(got[0].sum(dtype=np.int64)) > 5000
    half, nob, nums = _dev(k, np.asarray(HALF, dtype=np.int32)), _dev(k, NO_BITMAPS), _dev(k, table.nums[V1])
    bufs = _buffers(k, cap)
    args = (table.table, table.live16, table.cap, table.n, half, nob)
    with pytest.raises(ValueError):
        k.scan_sums(*args, [BIG4, BIG4], [2047, 2048], V4, nums, out=bufs)
    assert not any(g.any() for g in _host(bufs))
    ncols = int(table.table.shape[0])
    bufs = _buffers(k, 65)
    for keys, dims, vcol in (([ncols], [3], V1), ([G0, G1, W2], [1, 64, 300], V1), ([G0], [1, 4], V1), ([G0], [-1], V1),
                             ([G1], [64], -1), ([G1], [64], ncols), ([-1], [3], V1)):
        with pytest.raises(ValueError):  # a key outside the table, three keys, sizes that do not pair, no value column
            k.scan_sums(*args, keys, dims, vcol, nums, out=bufs)
    for bad in ((bufs[0], bufs[1]), (bufs[1], bufs[1], bufs[2]), (bufs[0], bufs[1][:10], bufs[2]),
                (bufs[0], bufs[1], bufs[2].to(torch.int32))):
        with pytest.raises(ValueError):  # not a triple, wrong types, too short
            k.scan_sums(*args, [G1], [64], V1, nums, out=bad)
    for bad in (nums.to(torch.int32), nums.reshape(2, -1), nums[::2]):
        with pytest.raises(ValueError):  # the number table: int64, flat, contiguous
            k.scan_sums(*args, [G1], [64], V1, bad, out=bufs)
    with pytest.raises(ValueError):
        k.scan_sums(table.table, table.live16, table.cap, table.cap + 1, half, nob, [G1], [64], V1, nums, out=bufs)
    assert not any(g.any() for g in _host(bufs))
    before = k.sum_scans
    k.scan_sums(*args, [G1], [64], V1, nums)
    assert k.sum_scans == before + 1
    # an empty number table: every id is past it
    got = _sums(k, table, TRUE, NO_BITMAPS, [G1], [64], V1, np.zeros(0, dtype=np.int64))
    assert not any(g.any() for g in got)


@pytest.mark.parametrize("extra", [0, 1])
def test_bitmaps_and_cells_share_the_lds(k, table, extra):
    """A 300-bit leaf bitmap at the end of a tensor of exactly ``tt_max_lds_bitmap_words()`` words
    -- staged in LDS, 32 KiB next to up to 80 KiB of cells -- and of one word more, read from
    global memory."""
    rng = np.random.default_rng(64 + extra)
    words = _limits(k)["bitmaps"] + extra
    bm = rng.integers(0, 1 << 32, words, dtype=np.uint64).astype(np.uint32)
    code = [[OP_LEAF, W2, words - 10, 300], [OP_RANGE, FLT, 0, 8], [OP_AND, 2, 0, 0]]
    for keys, dims in (([], []), ([G0], [1]), ([G1], [64]), ([GBIG], [4095]), ([GBIG], [4096])):
        want, _ = ref_sums(table, code, bm, keys, dims, V2, table.nums[V2])
        got = _sums(k, table, code, bm, keys, dims, V2, table.nums[V2])
        assert _same(got, want), (keys, dims)
        assert 1000 < int(want[0].sum(dtype=np.int64)) < table.n // 2


def test_two_launches_into_one_triple_and_the_same_launch_twice(k, table):
    """The rows with FLT below 5 and the rest, added into one zeroed triple, equal one launch
    over all rows; and a launch repeated gives the same words (integer atomics)."""
    lo, hi = [[OP_RANGE, FLT, 0, 5]], [[OP_RANGE, FLT, 5, 11]]
    for keys, dims in (([], []), ([G0], [1]), ([G1], [64]), ([GBIG], [4096])):
        ncells = math.prod(d + 1 for d in dims)
        want, _ = ref_sums(table, TRUE, NO_BITMAPS, keys, dims, V4, table.nums[V4])
        bufs = _buffers(k, ncells)
        half = _sums(k, table, lo, NO_BITMAPS, keys, dims, V4, table.nums[V4], bufs=bufs)
        assert not _same(half, want)
        assert _same(_sums(k, table, hi, NO_BITMAPS, keys, dims, V4, table.nums[V4], bufs=bufs), want)
        again = [_sums(k, table, TRUE, NO_BITMAPS, keys, dims, V4, table.nums[V4]) for _ in range(2)]
        assert _same(again[0], want) and _same(again[1], again[0])


# ------------------------------------------------------------------ the planner on the device
def _sum_docs(n):
    """``amount``: a near-unique integer; ``hours``: quarters, negative too; ``mixed``: numbers next
    to strings, nulls and bools; ``big``: +-(2^40 + i), cancelling."""
    rng = np.random.default_rng(71)
    docs = {}
    for i in range(n):
        d = {"who": f"user{i % 9}", "team": ["red", "blue", None][i % 3], "amount": int(rng.integers(0, 10 * n)),
             "hours": int(rng.integers(-400, 400)) / 4, "mixed": [i, "n/a", None, True, i + 0.5][i % 5],
             "big": (1 if i % 2 else -1) * ((1 << 40) + i), "i": i}
        if i % 11 == 0:
            del d["amount"]
        docs[f"a||k{i:06d}"] = d
    return docs


SUM_QUERIES = [
    ({"groupBy": ["who"], "aggregate": [{"op": "SUM", "key": "amount"}, {"op": "AVG", "key": "amount"}]}, 1, 0),
    # big over all rows: its magnitudes pass 2^53, the sums prove nothing and its histogram answers
    ({"aggregate": [{"op": "AVG", "key": "hours"}, {"op": "SUM", "key": "big"}]}, 2, 0),
    ({"filter": {"LT": {"i": 9000}}, "groupBy": ["who", "team"],
      "aggregate": [{"op": "SUM", "key": "mixed"}, {"op": "MIN", "key": "mixed"}, {"op": "COUNT", "key": "mixed"},
                    {"op": "MAX", "key": "hours"}]}, 1, 2),
    # 12,000 groups among 12,001 cells: more than the kernel keeps in LDS
    ({"groupBy": ["i"], "aggregate": [{"op": "SUM", "key": "big"}, {"op": "COUNT"}]}, 1, 0),
    ({"filter": {"EQ": {"who": "nobody"}}, "aggregate": [{"op": "SUM", "key": "amount"}]}, 1, 0),
]


def test_gpu_aggregate_sums_equal_cpu_and_brute_force(k, monkeypatch):
    """Every SUM / AVG key summed by ``tt_scan_sums`` (the host selection is barred), COUNT / MIN /
    MAX of the same key by ``tt_scan_extrema``, the group counts by ``tt_scan_group``."""
    docs = _sum_docs(12_000)
    ix = ColumnarIndex()
    ix.bulk_load(docs.items())
    monkeypatch.setattr(ColumnarIndex, "SUMS_FROM_CELLS", 0)
    monkeypatch.setattr(ColumnarIndex, "EXTREMA_FROM_CELLS", 0)

    def barred(*a, **kw):
        raise AssertionError("host selection on the device path")

    for q, n_sums, n_ext in SUM_QUERIES:
        with monkeypatch.context() as m:
            m.setattr(ColumnarIndex, "select_native", barred)
            m.setattr(ColumnarIndex, "select_numpy", barred)
            sums, ext = k.sum_scans, k.extrema_scans
            got = ix.aggregate(q, k)
            assert (k.sum_scans - sums, k.extrema_scans - ext) == (n_sums, n_ext), q
        assert got == ix.aggregate(q) == brute(docs, q), q
    # appended rows with new numbers, one of them on a finer quantum: the device table follows
    late = {f"a||late{i}": {"who": "user1", "amount": 10 ** 7 + i, "hours": 0.125 + i, "big": -i, "i": 50_000 + i}
            for i in range(40)}
    for key, d in late.items():
        ix.upsert(key, d)
    docs.update(late)
    for q, *_ in SUM_QUERIES[:2]:
        assert ix.aggregate(q, k) == ix.aggregate(q) == brute(docs, q), q

