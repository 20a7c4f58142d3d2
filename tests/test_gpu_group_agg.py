"""``tt_scan_group`` (ops/hip/group_agg.hip), the fused filter + N-dimensional histogram, over
synthetic device tables: every counter compared for equality with ``ref_group`` below --
``ref_select``, then ``np.bincount`` of the cell index -- at a partial tile with dead rows, on
every key width and axis count, at the missing slot of each axis, with ids past the dictionary
size (dropped, and a guard region past the counters stays zero), at the LDS / global counter
switch, at the cell cap, through the persistent tile loop, and with the leaf bitmaps staged in
LDS next to the histogram and left in global memory.
"""
import math

import numpy as np
import pytest

from aca_dotnet_workshop_amd.ops.columnar import OP_AND, OP_EQ, OP_LEAF, OP_OR, OP_RANGE, OP_TRUE

from test_gpu_kernel_edges import TILE, _Synth, _dev, _ids, _limits, _live16, _table, k, ref_select  # noqa: F401

pytestmark = pytest.mark.gpu
GUARD = 256  # counters past the histogram that no launch may touch
NO_BITMAPS = np.zeros(1, dtype=np.uint32)


def ref_group(T, code, bitmaps, keys, dims):
    """(counters uint32 [prod(dims + 1)], selected rows, rows dropped for an id past its
    dictionary): axis i has dims[i] + 1 slots, the last one for a missing path."""
    rows = ref_select(T.cols, T.live, T.n, code, bitmaps)
    cell = np.zeros(rows.size, dtype=np.int64)
    keep = np.ones(rows.size, dtype=bool)
    for c, d in zip(keys, dims):
        ids = np.asarray(T.cols[c][0], dtype=np.int64)[rows]
        keep &= (ids >= -1) & (ids < d)
        cell = cell * (d + 1) + np.where(ids == -1, d, ids)
    ncells = math.prod(d + 1 for d in dims)
    return np.bincount(cell[keep], minlength=ncells).astype(np.uint32), rows.size, int((~keep).sum())


def _group(k, T, code, bitmaps, keys, dims, max_blocks=0, n=None):
    """The kernel's counters, after checking that the guard region behind them is untouched."""
    import torch
    code = np.asarray(code, dtype=np.int32).reshape(-1, 4)
    ncells = math.prod(d + 1 for d in dims)
    buf = torch.zeros(ncells + GUARD, dtype=torch.int32, device=k.device)
    out = k.scan_group(T.table, T.live16, T.cap, T.n if n is None else n, _dev(k, code),
                       _dev(k, np.asarray(bitmaps, dtype=np.uint32)), keys, dims, max_blocks, counts=buf)
    assert out is buf
    got = buf.cpu().numpy().view(np.uint32)
    assert not got[ncells:].any(), "wrote past the counters"
    return got[:ncells]


# columns of the shared table: (index, dictionary size)
W0, W1, W2, W4, FLT, BIG2, BIG4, WIDE = range(8)
SIZE = {W0: 3, W1: 130, W2: 300, W4: 1000, FLT: 10, BIG2: 8191, BIG4: 2047}


@pytest.fixture(scope="module")
def table(k):
    """n = 3 tiles + 37 rows in a capacity of 4 tiles, ~10 % dead rows below n; past the 16-row
    group that holds row n every row is live and holds ids, so only the kernel's own row bound
    keeps them out.  WIDE is a 4-byte column whose ids run past every dictionary size used."""
    rng = np.random.default_rng(41)
    n, cap = 3 * TILE + 37, 4 * TILE
    cols = [(_ids(rng, cap, SIZE[W0]), 0), (_ids(rng, cap, SIZE[W1]), 1), (_ids(rng, cap, SIZE[W2]), 2),
            (_ids(rng, cap, SIZE[W4]), 4), (_ids(rng, cap, SIZE[FLT], missing=0.0), 1),
            (_ids(rng, cap, SIZE[BIG2]), 2), (_ids(rng, cap, SIZE[BIG4]), 4), (_ids(rng, cap, 5000), 4)]
    live = rng.random(cap) < 0.9
    live[n:(n + 15) // 16 * 16] = False
    live[(n + 15) // 16 * 16:] = True
    for c in (BIG2, BIG4):  # the first and the last id of the large dictionaries in live rows
        cols[c][0][np.nonzero(live[:n])[0][:2]] = [0, SIZE[c] - 1]
    return _Synth(k, cols, live, n, cap)


HALF = [[OP_RANGE, FLT, 0, 5]]                                   # ids 0..4 of FLT: about half
THIRD = [[OP_EQ, FLT, 3, 0], [OP_RANGE, FLT, 6, 8], [OP_OR, 2, 0, 0]]


@pytest.mark.parametrize("keys", [[], [W0], [W1], [W2], [W4], [W0, W1], [W4, W0], [W2, W4], [W0, W1, W2], [W1, W0, W0],
                                  [W4, W2, W0], [W0, W0]])
def test_partial_tile_every_width_and_axis_count(k, table, keys):
    """0 to 3 key columns of 2-bit, 1-, 2- and 4-byte codes: LDS counters up to 8192 cells, global
    ones above ([W2, W4]: 301,301 cells).  Rows >= n and dead rows count nowhere; with every id
    in range the counters add up to the selection; each axis's missing slot is populated."""
    dims = [SIZE[c] for c in keys]
    for code in (HALF, THIRD, [[OP_TRUE, 0, 0, 0]]):
        want, selected, dropped = ref_group(table, code, NO_BITMAPS, keys, dims)
        got = _group(k, table, code, NO_BITMAPS, keys, dims)
        assert np.array_equal(got, want), (keys, code)
        assert dropped == 0 and int(got.sum(dtype=np.int64)) == selected and 0 < selected < table.n
    shaped = want.reshape([d + 1 for d in dims])
    for axis in range(len(keys)):
        assert np.take(shaped, dims[axis], axis=axis).sum() > 0, ("missing slot", axis)


@pytest.mark.parametrize("keys,dims", [([WIDE], [1000]), ([W1, WIDE], [100, 4999]), ([WIDE, W0, W2], [7, 3, 299]),
                                       ([W2], [1]), ([W0], [0]), ([W1], [63]), ([W1], [64]), ([W0, W0], [2, 2])])
def test_ids_past_the_dictionary_are_dropped(k, table, keys, dims):
    """A dictionary size below the ids a column holds (it grew after the host read it): those rows
    count nowhere, the missing slot keeps only the missing rows, nothing lands past the counters
    -- on LDS counters and on global ones, and on either side of the 64 cells up to which the
    kernel keeps interleaved copies of the LDS histogram."""
    want, selected, dropped = ref_group(table, HALF, NO_BITMAPS, keys, dims)
    got = _group(k, table, HALF, NO_BITMAPS, keys, dims)
    assert np.array_equal(got, want)
    assert dropped > 0 and int(got.sum(dtype=np.int64)) == selected - dropped


@pytest.mark.parametrize("keys,dims", [([BIG2], [8191]), ([BIG2], [8192]), ([W1, W1], [63, 127]), ([W1, W1], [63, 128]),
                                       ([W0, W4], [2, 2730])])
def test_lds_and_global_counters_at_the_switch(k, table, keys, dims):
    """8192 cells (the most the LDS holds) and 8193 in one axis over the same column; in two axes
    64 x 128 = 8192 and 64 x 129 over the same columns, and 3 x 2731 = 8193 exactly."""
    lim = _limits(k)["groups"]
    ncells = math.prod(d + 1 for d in dims)
    assert ncells in (lim, lim + 1, 64 * 129)
    want, selected, _ = ref_group(table, [[OP_TRUE, 0, 0, 0]], NO_BITMAPS, keys, dims)
    got = _group(k, table, [[OP_TRUE, 0, 0, 0]], NO_BITMAPS, keys, dims)
    assert np.array_equal(got, want) and want[-1] > 0  # the last cell: every axis missing
    assert want[0] > 0 or keys[0] != keys[-1]
    if keys == [BIG2]:
        assert want[8190] > 0 and int(got.sum(dtype=np.int64)) == selected


def test_cell_cap(k, table):
    """Exactly ``tt_group_max_cells()`` cells are counted; one product above is refused by the
    launcher, which launches nothing."""
    import torch
    cap = int(k.lib.tt_group_max_cells())
    assert cap == 2048 * 2048
    want, selected, _ = ref_group(table, HALF, NO_BITMAPS, [BIG4, BIG4], [2047, 2047])
    got = _group(k, table, HALF, NO_BITMAPS, [BIG4, BIG4], [2047, 2047])
    assert np.array_equal(got, want) and int(got.sum(dtype=np.int64)) == selected
    buf = torch.zeros(cap + GUARD, dtype=torch.int32, device=k.device)
    with pytest.raises(ValueError):
        k.scan_group(table.table, table.live16, table.cap, table.n, _dev(k, np.asarray(HALF, dtype=np.int32)),
                     _dev(k, NO_BITMAPS), [BIG4, BIG4], [2047, 2048], counts=buf)
    assert not buf.any().item()
    for bad in ([[8], [3]], [[W0, W1, W2, W4], [3, 130, 300, 1000]], [[W0], [3, 4]], [[W0], [-1]]):
        with pytest.raises(ValueError):  # a key outside the table, four keys, sizes that do not pair
            k.scan_group(table.table, table.live16, table.cap, table.n, _dev(k, np.asarray(HALF, dtype=np.int32)),
                         _dev(k, NO_BITMAPS), bad[0], bad[1])


def test_persistent_tile_loop(k):
    """5 tiles on 2 blocks (tiles 0, 2, 4 and 1, 3) equal 5 tiles on the default grid, LDS and
    global counters."""
    rng = np.random.default_rng(43)
    n, cap = 4 * TILE + 1234, 5 * TILE
    cols = [(_ids(rng, n, 200), 1), (_ids(rng, n, 9000), 2), (_ids(rng, n, 10, missing=0.0), 1)]
    T = _Synth(k, cols, rng.random(n) < 0.95, n, cap)
    code = [[OP_RANGE, 2, 0, 7]]
    for keys, dims in (([0], [200]), ([1], [9000]), ([0, 1], [200, 9000])):
        want, selected, _ = ref_group(T, code, NO_BITMAPS, keys, dims)
        for max_blocks in (2, 0, 1, 5, 64):
            got = _group(k, T, code, NO_BITMAPS, keys, dims, max_blocks)
            assert np.array_equal(got, want), (keys, max_blocks)
        assert int(want.sum(dtype=np.int64)) == selected and want[-1] > 0
        last = np.asarray(T.cols[keys[0]][0])[4 * TILE:]  # the fifth tile's rows are in the counts
        assert (last >= 0).any()


@pytest.mark.parametrize("extra", [0, 1])
def test_bitmaps_and_histogram_share_the_lds(k, table, extra):
    """A 300-bit leaf bitmap (memory words, not registers) at the end of a tensor of exactly
    ``tt_max_lds_bitmap_words()`` words -- staged in LDS, where it and the 8192-cell histogram
    take 32 KiB each -- and of one word more, read from global memory."""
    rng = np.random.default_rng(44 + extra)
    words = _limits(k)["bitmaps"] + extra
    bm = rng.integers(0, 1 << 32, words, dtype=np.uint64).astype(np.uint32)
    code = [[OP_LEAF, W2, words - 10, 300], [OP_RANGE, FLT, 0, 8], [OP_AND, 2, 0, 0]]
    for keys, dims in (([BIG2], [8191]), ([W1], [130]), ([BIG2], [8192])):
        want, selected, _ = ref_group(table, code, bm, keys, dims)
        got = _group(k, table, code, bm, keys, dims)
        assert np.array_equal(got, want), (keys, dims)
        assert 1000 < selected < table.n // 2 and int(got.sum(dtype=np.int64)) == selected


def test_empty_selection_and_no_rows(k, table):
    for keys, dims in (([], []), ([W1], [130]), ([W2, W4], [300, 1000])):
        got = _group(k, table, [[OP_EQ, FLT, 200, 0]], NO_BITMAPS, keys, dims)  # no row holds id 200
        assert got.size == math.prod(d + 1 for d in dims) and not got.any()
        assert not _group(k, table, [[OP_TRUE, 0, 0, 0]], NO_BITMAPS, keys, dims, n=0).any()
