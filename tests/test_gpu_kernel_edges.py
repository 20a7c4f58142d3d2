"""The gfx950 query kernels (ops/hip/*.hip) at the branches no document of the other suites
reaches: size thresholds (LDS staging against global memory, register bitmaps against memory
words, grid-stride loops), every code width, the full interpreter stack, bounds and overflow of
the page gather, and the width switches of ``ColumnarIndex.width_for``.

The GPU half drives ``GpuKernels`` over synthetic device tables: NumPy arrays of ids packed into
the device layout by ``_table`` below (written from the layout comment at the top of
``query_scan.hip``, sharing no code with ``ColumnarIndex``), compared for exact equality with
the few-line references ``ref_select`` / ``ref_keys`` / ``ref_page``.  The unmarked tests check
those references, and the packer, against the host executors on a machine without a GPU.
"""
import ctypes
import random

import numpy as np
import pytest

from aca_dotnet_workshop_amd import native
from aca_dotnet_workshop_amd.ops.columnar import (MAX_DEPTH, OP_AND, OP_EQ, OP_LEAF, OP_NOT, OP_OR, OP_RANGE, OP_TRUE,
                                                  ColumnarIndex, Unsupported)

TILE = 8192
TOP = (1 << 64) - 1                       # bound = "every tile was read"
MISSING = {0: 3, 1: 0xFF, 2: 0xFFFF}      # the all-ones code of a width
MAX_ID = {0: 2, 1: 254, 2: 65534, 4: (1 << 31) - 1}


# ------------------------------------------------------------------ the device layout
def _pack(ids, width, cap):
    """One column of ``cap`` rows in the device layout, as bytes.  ``ids``: int32 [n], -1 =
    missing; rows past n are missing.  Width 0: 2 bits per row, row r in bits 2(r mod 4) of byte
    r / 4, missing = 3, and 16 bytes of padding; widths 1 and 2: all-ones = missing; width 4:
    the int32 as is."""
    ids = np.asarray(ids, dtype=np.int32)
    assert cap % TILE == 0 and ids.size <= cap
    assert ids.size == 0 or (ids.min() >= -1 and ids.max() <= MAX_ID[width]), "ids do not fit the width"
    v = np.full(cap, -1, dtype=np.int32)
    v[:ids.size] = ids
    if width == 4:
        out = v
    elif width == 0:
        c = np.where(v < 0, MISSING[0], v).astype(np.uint8)
        out = np.concatenate([c[0::4] | (c[1::4] << 2) | (c[2::4] << 4) | (c[3::4] << 6), np.zeros(16, dtype=np.uint8)])
    else:
        out = np.where(v < 0, MISSING[width], v).astype(np.uint8 if width == 1 else np.uint16)
    return np.ascontiguousarray(out).view(np.uint8)


def _table(k, cols, cap):
    """``cols`` = [(ids int32 [n], width)] on the device: the column tensors (keep them alive)
    and the int64 [ncols, 2] descriptor table of (address, width)."""
    import torch
    tensors = [torch.from_numpy(_pack(ids, w, cap)).to(k.device) for ids, w in cols]
    desc = np.array([[t.data_ptr(), w] for t, (_, w) in zip(tensors, cols)], dtype=np.int64).reshape(-1, 2)
    return tensors, torch.from_numpy(desc).to(k.device)


def _live16(live_bool, cap):
    """The int16 liveness words of ``cap`` rows (bit r mod 16 of word r / 16), rows past the
    array dead."""
    bits = np.zeros(cap, dtype=np.uint8)
    bits[:len(live_bool)] = np.asarray(live_bool, dtype=bool)
    return np.packbits(bits, bitorder="little").view("<u2").view(np.int16)


# ------------------------------------------------------------------ references
def ref_select(cols, live, n, code, bitmaps):
    """Rows (ascending int32) of the live rows that satisfy the postfix program, over raw ids;
    OP_RANGE reads the column's values directly (a synthetic range column holds ranks)."""
    bm = np.ascontiguousarray(bitmaps).view(np.uint32)
    stack = []
    for op, a, b, c in np.asarray(code).reshape(-1, 4).tolist():
        if op in (OP_EQ, OP_RANGE, OP_LEAF):
            v = np.asarray(cols[a][0][:n], dtype=np.int64)
        if op == OP_EQ:
            stack.append(v == b)
        elif op == OP_RANGE:
            stack.append((v >= 0) & (v >= b) & (v < c))
        elif op == OP_LEAF:
            bits = np.unpackbits(bm[b:b + (c + 31) // 32].view(np.uint8), bitorder="little")[:c]
            ok = (v >= 0) & (v < c)
            hit = np.zeros(n, dtype=bool)
            hit[ok] = bits[v[ok]] == 1
            stack.append(hit)
        elif op in (OP_AND, OP_OR):
            xs = [stack.pop() for _ in range(a)]
            stack.append(np.logical_and.reduce(xs) if op == OP_AND else np.logical_or.reduce(xs))
        elif op == OP_NOT:
            stack.append(~stack.pop())
        else:
            assert op == OP_TRUE
            stack.append(np.ones(n, dtype=bool))
    return np.nonzero(stack[-1] & np.asarray(live[:n], dtype=bool))[0].astype(np.int32)


def ref_keys(cols, rows, specs, ranks, seq, seq_bits):
    """The packed ordering keys (uint64) of ``rows``: [rank(key 0) | ... | seq], most significant
    first; an id outside the key's rank table, or a missing one, ranks as ``missing``; DESC
    stores max_rank - rank."""
    rows = np.asarray(rows, dtype=np.int64)
    ranks = np.asarray(ranks, dtype=np.int64)
    k = np.zeros(rows.size, dtype=np.uint64)
    for col, off, nranks, bits, desc, miss, max_rank, _ in np.asarray(specs).reshape(-1, 8).tolist():
        ids = np.asarray(cols[col][0], dtype=np.int64)[rows]
        ok = (ids >= 0) & (ids < nranks)
        r = np.full(rows.size, miss, dtype=np.int64)
        r[ok] = ranks[off + ids[ok]]
        if desc:
            r = max_rank - r
        k = (k << np.uint64(bits)) | r.astype(np.uint64)
    return (k << np.uint64(seq_bits)) | np.asarray(seq)[rows].astype(np.uint64)


def ref_page(cols, live, n, code, bitmaps, specs, ranks, seq, seq_bits, tiles, k, offset, bound, cap=TILE):
    """(rows [offset, k) of the key order, candidates, complete) among the matches in ``tiles``
    whose key orders strictly before ``bound`` (TOP: no bound)."""
    sel = ref_select(cols, live, n, code, bitmaps)
    sel = sel[np.isin(sel // TILE, np.asarray(tiles, dtype=np.int64))]
    keys = ref_keys(cols, sel, specs, ranks, seq, seq_bits)
    if bound != TOP:
        keep = keys < np.uint64(bound)
        sel, keys = sel[keep], keys[keep]
    total = int(sel.size)
    held = min(total, cap)
    order = sel[np.argsort(keys, kind="stable")][:cap]
    complete = False if total > cap else True if held >= k else bound == TOP
    return order[offset:min(held, k)].astype(np.int32), total, complete


def _depth(code):
    """Largest number of stack entries the program holds."""
    d = top = 0
    for op, a, _, _ in np.asarray(code).reshape(-1, 4).tolist():
        d += 1 - a if op in (OP_AND, OP_OR) else 0 if op == OP_NOT else 1
        top = max(top, d)
    assert d == 1
    return top


def _chain(depth):
    """A right-nested filter alternating AND and OR, ``depth`` leaves deep, ending in a NEQ: its
    postfix form pushes ``depth`` leaves and applies the NOT while all of them are stacked."""
    f = {"NEQ": {"a": True}}
    for i in range(depth - 1, 0, -1):
        if i % 2:
            f = {"AND": [{"IN": {"b": [j for j in range(20) if j != i]}}, f]}
        else:
            f = {"OR": [{"EQ": {"b": i}}, f]}
    return f


def _chain_index(n=TILE + 53, seed=2):
    rnd = random.Random(seed)
    ix = ColumnarIndex(["a", "b"], capacity=n)
    for i in range(n):
        d = {"a": rnd.choice([True, False, None]), "b": rnd.randrange(20)}
        if rnd.random() < 0.06:
            del d[rnd.choice(["a", "b"])]
        ix.upsert(str(i), d)
    for i in rnd.sample(range(n), n // 10):
        ix.delete(str(i))
    return ix


# ------------------------------------------------------------------ CPU: the references and the packer
@pytest.fixture(scope="module")
def host_index():
    """Columns of all four widths (3 / 200 / 3,000 / 66,000 values), missing paths, tombstones."""
    rnd = random.Random(11)
    n = 66_500
    ix = ColumnarIndex(["s", "m", "w", "x"], capacity=n)
    for i in range(n):
        d = {"s": rnd.choice([True, False, None]), "m": f"m{rnd.randrange(200):03d}",
             "w": f"w{rnd.randrange(3000):04d}", "x": f"x{i % 66_000:05d}"}
        if rnd.random() < 0.07:
            del d[rnd.choice(["s", "m", "w", "x"] if i >= 66_000 else ["s", "m", "w"])]
        ix.upsert(str(i), d)
    for i in rnd.sample(range(n), n // 15):
        ix.delete(str(i))
    return ix


_HOST_WIDTHS = [0, 1, 2, 4]
_HOST_FILTERS = [
    {}, {"EQ": {"s": False}}, {"NEQ": {"m": "m007"}}, {"EQ": {"x": "nowhere"}}, {"NEQ": {"x": "nowhere"}},
    {"IN": {"m": [f"m{j:03d}" for j in range(0, 200, 3)]}}, {"IN": {"s": [True, None]}},
    {"IN": {"x": ["x00000", "x65999", "x31000"]}}, {"LT": {"w": "w1500"}}, {"GTE": {"x": "x65990"}},
    {"AND": [{"GTE": {"m": "m050"}}, {"LT": {"x": "x60000"}}, {"EQ": {"s": True}}]},
    {"OR": [{"IN": {"w": ["w0001", "w2999"]}}, {"GT": {"x": "x65900"}}, {"NEQ": {"s": None}}]},
]


def _host_cols(ix, prog):
    """The index's id arrays as synthetic columns, plus one rank-valued column per range leaf
    (ranks looked up here, missing stays -1), and the program with its range leaves pointed at them."""
    n = ix.n
    assert [len(c.values) for c in ix.columns[:4]] == [3, 200, 3000, 66_000]
    cols = [(ix.ids[c, :n], w) for c, w in enumerate(_HOST_WIDTHS)]
    code = prog.code.copy()
    for row in code:
        if row[0] == OP_RANGE:
            ids = ix.ids[row[1], :n]
            table = ix.columns[row[1]].ranks()
            rank = np.where(ids >= 0, table[np.maximum(ids, 0)], -1).astype(np.int32)
            cols.append((rank, max(1, _HOST_WIDTHS[row[1]])))
            row[1] = len(cols) - 1
    return cols, code


def test_ref_select_and_the_packed_layout_match_the_host_executors(host_index):
    """ref_select == ColumnarIndex.select_numpy, and the C++ host executor (which reads the same
    narrow layout as the kernels) selects the same rows from the arrays ``_pack`` builds."""
    ix = host_index
    n, cap = ix.n, (ix.n + TILE - 1) // TILE * TILE
    live = ix.live[:n] != 0
    for f in _HOST_FILTERS:
        prog = ix.compile(f)
        want = ix.select_numpy(prog)
        cols, code = _host_cols(ix, prog)
        assert np.array_equal(ref_select(cols, live, n, code, prog.bitmaps), want), f
        packed = [(_pack(ids, w, cap), w) for ids, w in cols]
        got = native.load().scan_select(packed, _live16(live, cap).view(np.uint16), n, np.ascontiguousarray(code),
                                        prog.bitmaps.view(np.uint32), 3, True)
        assert np.array_equal(got, want), f


def test_pack_layout_by_hand():
    """The packer against the layout comment, bit by bit, on one small example per width."""
    ids = np.array([0, 1, 2, -1, 2, -1, 0, 1], dtype=np.int32)
    p0 = _pack(ids, 0, TILE)
    assert p0.size == TILE // 4 + 16 and p0[0] == 0b11_10_01_00 and p0[1] == 0b01_00_11_10 and p0[2] == 0xFF
    assert _pack(ids, 1, TILE)[:9].tolist() == [0, 1, 2, 255, 2, 255, 0, 1, 255]
    assert _pack(ids, 2, TILE).view("<u2")[:9].tolist() == [0, 1, 2, 65535, 2, 65535, 0, 1, 65535]
    assert _pack(ids, 4, TILE).view("<i4")[:9].tolist() == [0, 1, 2, -1, 2, -1, 0, 1, -1]
    assert _live16([1, 0, 0, 1] + [0] * 12 + [1], TILE).view(np.uint16)[:3].tolist() == [0b1001, 1, 0]


def test_index_codes_follow_the_hand_packed_layout():
    """``ops/codes.py`` (what the index uploads) on the example above, and the id -> value gather."""
    from aca_dotnet_workshop_amd.ops.codes import encode_codes, gather
    ids = np.array([0, 1, 2, -1, 2, -1, 0, 1], dtype=np.int32)
    assert encode_codes(ids, 0).tolist() == [0b11_10_01_00, 0b01_00_11_10]
    for w, nbytes in ((0, 2), (1, 8), (2, 16), (4, 32)):
        got = encode_codes(ids, w)
        assert got.nbytes == nbytes and got.tobytes() == _pack(ids, w, TILE).tobytes()[:nbytes]
    assert encode_codes(ids, 4) is ids
    table = np.array([10, 20, 30], dtype=np.int64)
    assert gather(table, ids, -7).tolist() == [10, 20, 30, -7, 30, -7, 10, 20]
    assert gather(table[:0], np.array([-1, -1]), 5).tolist() == [5, 5]


@pytest.mark.parametrize("sort", [[], [{"key": "m", "order": "DESC"}], [{"key": "x"}, {"key": "s", "order": "DESC"}],
                                  [{"key": "s"}, {"key": "m"}, {"key": "w", "order": "DESC"}, {"key": "x"}]])
def test_ref_keys_match_the_host_sort_keys(host_index, sort):
    ix = host_index
    plan = ix.sort_specs(sort)
    specs, ranks, seq_bits = plan
    cols = [(ix.ids[c, :ix.n], w) for c, w in enumerate(_HOST_WIDTHS)]
    rows = np.nonzero(ix.live[:ix.n])[0][::3]
    got = ref_keys(cols, rows, specs, ranks, ix.seq, seq_bits)
    assert np.array_equal(got, ix.sort_keys_numpy(rows, plan).astype(np.uint64))


def test_ref_page_matches_the_emulated_page_kernels(host_index):
    from test_columnar import _FakePageKernels  # the host emulation page_gpu is tested with
    ix = host_index
    n, live = ix.n, ix.live[:ix.n] != 0
    sort = [{"key": "m", "order": "DESC"}, {"key": "w"}]
    specs, ranks, seq_bits = ix.sort_specs(sort)
    prog = ix.compile({"AND": [{"EQ": {"s": True}}, {"LT": {"w": "w0600"}}]})
    cols, code = _host_cols(ix, prog)
    fk = _FakePageKernels(ix)
    fk.prog, fk.sort = prog, sort
    every = np.arange((n + TILE - 1) // TILE)
    allkeys = np.sort(ref_keys(cols, ix.select_numpy(prog), specs, ranks, ix.seq, seq_bits))
    assert allkeys.size > 2000
    for tiles in (every, every[::-2], every[3:4], every[:0]):
        for bound in (TOP, int(allkeys[allkeys.size // 2]), int(allkeys[7]), 0):
            for k, offset in ((1, 0), (64, 64), (1000, 400), (8192, 0)):
                want = fk.page(None, None, n, None, None, None, None, None, seq_bits, tiles, k, offset, bound)
                got = ref_page(cols, live, n, code, prog.bitmaps, specs, ranks, ix.seq, seq_bits, tiles, k, offset,
                               bound)
                assert np.array_equal(got[0], want[0]) and got[1:] == want[1:], (tiles, bound, k, offset)
    fk.page_cap = 100  # overflow: counted, incomplete
    want = fk.page(None, None, n, None, None, None, None, None, seq_bits, every, 50, 0, TOP)
    got = ref_page(cols, live, n, code, prog.bitmaps, specs, ranks, ix.seq, seq_bits, every, 50, 0, TOP, cap=100)
    assert got[1:] == want[1:] == (allkeys.size, False)


def test_filter_depth_at_the_device_stack_limit():
    """A filter whose postfix form holds exactly MAX_DEPTH entries compiles; one level deeper is
    Unsupported (the device stack is a 128-bit register of 16-bit masks)."""
    ix = _chain_index(200)
    prog = ix.compile(_chain(MAX_DEPTH))
    assert _depth(prog.code) == MAX_DEPTH
    nots = np.nonzero(prog.code[:, 0] == OP_NOT)[0]
    assert nots.size == 1 and _depth(np.vstack([prog.code[:nots[0]], [[OP_AND, MAX_DEPTH, 0, 0]]])) == MAX_DEPTH
    cols = [(ix.ids[0, :ix.n], 0), (ix.ids[1, :ix.n], 1)]
    assert np.array_equal(ref_select(cols, ix.live[:ix.n] != 0, ix.n, prog.code, prog.bitmaps), ix.select_numpy(prog))
    with pytest.raises(Unsupported):
        ix.compile(_chain(MAX_DEPTH + 1))
    wide = {"AND": [{"EQ": {"b": j}} for j in range(MAX_DEPTH + 1)]}  # nine operands: also too deep
    with pytest.raises(Unsupported):
        ix.compile(wide)


# ------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def k():
    from aca_dotnet_workshop_amd.ops.gpu import GpuKernels
    return GpuKernels()


def _limits(k):
    """The kernels' size thresholds, from the library itself."""
    return {"bitmaps": int(k.lib.tt_max_lds_bitmap_words()), "ranks": int(k.lib.tt_max_lds_ranks()),
            "groups": int(k.lib.tt_max_lds_groups()), "sort_ranks": int(k.lib.tt_lds_rank_words()),
            "bins": int(k.lib.tt_hist_bins())}


def _dev(k, a):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    elif a.dtype == np.uint64:
        a = a.view(np.int64)
    return torch.from_numpy(a).to(k.device)


def _ids(rng, n, hi, missing=0.1):
    """Random ids in [0, hi) with a share of missing rows; 0 and hi - 1 are present."""
    v = rng.integers(0, hi, n).astype(np.int32)
    v[rng.random(n) < missing] = -1
    v[rng.choice(n, 2, replace=False)] = [0, hi - 1]
    return v


class _Synth:
    """One synthetic table on the device and its host arrays."""

    def __init__(self, k, cols, live, n, cap, seq=None):
        self.cols, self.live, self.n, self.cap = cols, np.asarray(live, dtype=bool), n, cap
        self.tensors, self.table = _table(k, cols, cap)
        self.live16 = _dev(k, _live16(self.live, cap))
        self.seq = None if seq is None else np.asarray(seq, dtype=np.uint32)
        if seq is not None:
            padded = np.zeros(cap, dtype=np.uint32)
            padded[:len(seq)] = seq
            self.seq_t = _dev(k, padded)


def _run_select(k, T, code, bitmaps, return_mask=False):
    code = np.asarray(code, dtype=np.int32).reshape(-1, 4)
    bitmaps = np.asarray(bitmaps, dtype=np.uint32)
    res = k.select(T.table, T.live16, T.cap, T.n, _dev(k, code), _dev(k, bitmaps), return_mask=return_mask)
    want = ref_select(T.cols, T.live, T.n, code, bitmaps)
    rows = (res[0] if return_mask else res).cpu().numpy()
    if return_mask:  # one bit per row of the launched tiles, zero for every row not selected
        words = res[1].cpu().numpy().view(np.uint8)
        bits = np.zeros(words.size * 8, dtype=np.uint8)
        bits[want] = 1
        assert np.array_equal(np.unpackbits(words, bitorder="little"), bits)
    return rows, want


# -- 1. leaf edges
@pytest.fixture(scope="module")
def leaf_table(k):
    """Per width a column of small ids for bitmap leaves (ids run past every bitmap tested) and,
    for widths 1, 2 and 4, one that uses the whole code range (EQ, and ranks for RANGE)."""
    rng = np.random.default_rng(1)
    n, cap = TILE + 53, 2 * TILE
    small = {0: 3, 1: 130, 2: 130, 4: 130}
    full = {1: 255, 2: 65535, 4: 65536}  # largest value 254 / 65,534 / 65,535
    cols = [(_ids(rng, n, small[w]), w) for w in (0, 1, 2, 4)] + [(_ids(rng, n, full[w]), w) for w in (1, 2, 4)]
    live = rng.random(n) < 0.8
    for ids, w in cols[4:]:  # live rows at both ends of the code range
        ids[np.nonzero(live)[0][10:15]] = [full[w] - 1, full[w] - 2, 50, 1, 0]
    T = _Synth(k, cols, live, n, cap)
    T.small, T.full, T.full_max = {0: 0, 1: 1, 2: 2, 4: 3}, {1: 4, 2: 5, 4: 6}, {w: full[w] - 1 for w in full}
    return T


@pytest.mark.gpu
@pytest.mark.parametrize("width", [0, 1, 2, 4])
def test_gpu_bitmap_leaf_at_the_register_and_word_switches(k, leaf_table, width):
    """OP_LEAF with 1 .. 97 bitmap bits: one register word, two (33 .. 64), memory words (65 on),
    on every code width.  The bitmap is random, its last bit set, the words after it random
    too; ids at or past ``nbits`` and missing codes must not match.  Then the same with the last
    bit alone (a bit read from the wrong word or position cannot pass by chance)."""
    T, rng = leaf_table, np.random.default_rng(10 + width)
    col = T.small[width]
    ids = T.cols[col][0]
    for nbits in ((1, 2, 3) if width == 0 else (1, 31, 32, 33, 63, 64, 65, 96, 97)):
        base = int(rng.integers(0, 5))
        bm = rng.integers(0, 1 << 32, base + 5, dtype=np.uint64).astype(np.uint32)
        word, bit = base + (nbits - 1) // 32, np.uint32(1 << ((nbits - 1) % 32))
        bm[word] |= bit
        got, want = _run_select(k, T, [[OP_LEAF, col, base, nbits]], bm, return_mask=nbits in (3, 33))
        assert np.array_equal(got, want), (width, nbits)
        assert 0 < want.size < T.live.sum()
        assert (ids[want] < nbits).all() and (ids[want] == nbits - 1).any()
        assert (ids >= nbits).any() or nbits > MAX_ID[width]
        bm[base:word + 1] = 0
        bm[word] = bit
        got, want = _run_select(k, T, [[OP_LEAF, col, base, nbits]], bm)
        assert np.array_equal(got, want) and want.size and (ids[want] == nbits - 1).all(), (width, nbits, "one bit")


@pytest.mark.gpu
@pytest.mark.parametrize("width", [0, 1, 2, 4])
def test_gpu_eq_next_to_the_missing_code(k, leaf_table, width):
    """OP_EQ with the id of an absent value (-2) and with the largest id the width holds, plain
    and negated: the missing code is neither; NEQ of an absent value selects every live row."""
    T = leaf_table
    col, top = (T.small[0], 2) if width == 0 else (T.full[width], T.full_max[width])
    live = np.nonzero(T.live)[0]
    for b in (-2, top):
        got, want = _run_select(k, T, [[OP_EQ, col, b, 0]], [0], return_mask=b == top)
        assert np.array_equal(got, want) and want.size == (0 if b == -2 else (T.cols[col][0][live] == top).sum())
        got, want = _run_select(k, T, [[OP_EQ, col, b, 0], [OP_NOT, 0, 0, 0]], [0])
        assert np.array_equal(got, want), (width, b)
        if b == -2:
            assert np.array_equal(got, live) and (T.cols[col][0][live] < 0).any()


@pytest.mark.gpu
@pytest.mark.parametrize("width", [1, 2, 4])
def test_gpu_range_next_to_the_missing_code(k, leaf_table, width):
    """OP_RANGE on rank columns whose largest rank sits next to the all-ones code (254, 65,534;
    65,535 on 4 bytes): intervals ending at max + 1, the empty interval, missing rows."""
    T = leaf_table
    col, top = T.full[width], T.full_max[width]
    for lo, hi in ((1, top + 1), (top, top + 1), (top // 2, top + 1), (0, top + 1), (1, 1), (3, 100), (top - 1, top)):
        got, want = _run_select(k, T, [[OP_RANGE, col, lo, hi]], [0], return_mask=(lo, hi) == (1, top + 1))
        assert np.array_equal(got, want), (width, lo, hi)
        assert (want.size == 0) == (lo == hi)


# -- 2. stack depth
@pytest.mark.gpu
def test_gpu_full_interpreter_stack(k, leaf_table):
    """Eight stacked masks: AND and OR of 8 operands (the first leaf pushed ends in bits
    112..127), and a compiled right-nested chain that negates the top while 8 are stacked."""
    T, rng = leaf_table, np.random.default_rng(20)
    assert k.max_depth == MAX_DEPTH == 8
    for op, dense in ((OP_AND, 0.85), (OP_OR, 0.08)):
        bm = np.packbits(rng.random(8 * 160) < dense, bitorder="little").view(np.uint32)  # 8 bitmaps of 5 words
        code = [[OP_LEAF, T.small[(1, 2, 4)[j % 3]], 5 * j, 130] for j in range(8)] + [[op, 8, 0, 0]]
        assert _depth(code) == 8
        got, want = _run_select(k, T, code, bm)
        assert np.array_equal(got, want) and 100 < want.size < T.live.sum() - 100
        # the bottom entry counts: without the first leaf the selection differs
        assert not np.array_equal(ref_select(T.cols, T.live, T.n, code[1:8] + [[op, 7, 0, 0]], bm), want)
    ix = _chain_index()
    prog = ix.compile(_chain(8))
    assert _depth(prog.code) == 8 and prog.code[8].tolist() == [OP_NOT, 0, 0, 0]
    C = _Synth(k, [(ix.ids[0, :ix.n], 0), (ix.ids[1, :ix.n], 2)], ix.live[:ix.n] != 0, ix.n, ix.cap)
    got, want = _run_select(k, C, prog.code, prog.bitmaps, return_mask=True)
    assert np.array_equal(got, want) and np.array_equal(want, ix.select_numpy(prog))
    assert 100 < want.size < C.live.sum() - 100
    # NOT below the top of a deep stack, hand-written: a b NOT c d NOT OR3 NOT AND2
    code = [[OP_EQ, T.small[0], 1, 0], [OP_EQ, T.small[1], 7, 0], [OP_NOT, 0, 0, 0], [OP_RANGE, T.full[2], 1, 30000],
            [OP_EQ, T.small[4], 3, 0], [OP_NOT, 0, 0, 0], [OP_OR, 3, 0, 0], [OP_NOT, 0, 0, 0], [OP_TRUE, 0, 0, 0],
            [OP_AND, 2, 0, 0], [OP_OR, 2, 0, 0]]
    got, want = _run_select(k, T, code, [0])
    assert np.array_equal(got, want) and want.size


# -- 4. gather + top-k (the table of tests 3 and 5 too)
@pytest.fixture(scope="module")
def page_table(k):
    """Five tiles, the last partial: tiles 0 and 1 fully live, tile 2 dead, 3 and 4 random.
    Sort columns of widths 1 (DESC), 2 (ids past its rank table, missing ranks 5), 0 and 4; a
    filter column; a 17-bit insertion sequence."""
    rng = np.random.default_rng(4)
    n, cap = 5 * TILE - 7, 5 * TILE
    live = rng.random(n) < 0.8
    live[:2 * TILE] = True
    live[2 * TILE:3 * TILE] = False
    cols = [(_ids(rng, n, 200), 1), (_ids(rng, n, 1200), 2), (_ids(rng, n, 3), 0), (_ids(rng, n, 70_000), 4),
            (_ids(rng, n, 10), 1), (_ids(rng, n, 400), 2)]
    seq = rng.permutation(1 << 17)[:n]
    tables = [rng.permutation(200) + 1, rng.permutation(1000) + 1, np.array([2, 3, 1]), rng.permutation(70_000) + 1]
    # one live row of the last tile orders before every other row, whatever the number of keys: a
    # row count cut just below it must leave it out (tt_zone_argmin masks the rows past the count)
    first = 4 * TILE + 32 * 101 + 4
    live[first] = True
    for c, want_rank in ((0, 200), (1, 1), (2, 1), (3, 70_000)):  # DESC keys store max_rank - rank
        cols[c][0][first] = int(np.nonzero(tables[c] == want_rank)[0][0])
    low = int(np.argmin(seq))
    seq[low], seq[first] = seq[first], seq[low]
    T = _Synth(k, cols, live, n, cap, seq=seq)
    T.seq_bits, T.first = 17, first
    T.ranks = np.concatenate(tables).astype(np.int32)
    offs = np.cumsum([0] + [t.size for t in tables])
    #          col off            nranks  bits desc missing max_rank
    T.specs = np.array([[0, offs[0], 200, 8, 1, 0, 200, 0],
                        [1, offs[1], 1000, 10, 0, 5, 1000, 0],
                        [2, offs[2], 3, 2, 0, 0, 3, 0],
                        [3, offs[3], 70_000, 17, 1, 0, 70_000, 0]], dtype=np.int32)
    T.ranks_t = _dev(k, T.ranks)
    T.specs_t = {nk: _dev(k, T.specs[:nk]) for nk in (0, 1, 2, 4)}
    # the filter: column 4 == 3 OR column 0 in a sparse bitmap (about one row in seven)
    bm = np.packbits(rng.random(224) < 0.05, bitorder="little").view(np.uint32)
    T.code = np.array([[OP_EQ, 4, 3, 0], [OP_LEAF, 0, 0, 200], [OP_OR, 2, 0, 0]], dtype=np.int32)
    T.bitmaps = bm
    T.code_t, T.bitmaps_t = _dev(k, T.code), _dev(k, bm)
    return T


def _page(k, T, nk, tiles, kk, off, bound, code=None, bitmaps=None, n=None):
    code = T.code if code is None else np.asarray(code, dtype=np.int32).reshape(-1, 4)
    bitmaps = T.bitmaps if bitmaps is None else np.asarray(bitmaps, dtype=np.uint32)
    tiles = np.asarray(tiles, dtype=np.int32)
    n = T.n if n is None else n
    got = k.page(T.table, T.live16, n, _dev(k, code), _dev(k, bitmaps), T.specs_t[nk], T.ranks_t, T.seq_t, T.seq_bits,
                 tiles, kk, off, bound)
    want = ref_page(T.cols, T.live, n, code, bitmaps, T.specs[:nk], T.ranks, T.seq, T.seq_bits, tiles, kk, off, bound,
                    cap=k.page_cap)
    return got, want


_TILE_LISTS = ([4, 0, 3], [2], [3, 2, 1, 4, 0], [], [1])
_PAGES = ((1, 0), (64, 64), (1000, 400), (8192, 0))


@pytest.mark.gpu
@pytest.mark.parametrize("nkeys", [0, 1, 2, 4])
def test_gpu_page_gather_and_topk_against_the_reference(k, page_table, nkeys):
    """GpuKernels.page (tt_page_gather + tt_page_topk in one launch) over unordered tile lists
    -- the partial last tile, a dead tile, none -- with no bound, bounds inside the candidates'
    keys (strict: a candidate whose key equals the bound is left out) and 0."""
    T = page_table
    assert k.page_cap == TILE
    sel = ref_select(T.cols, T.live, T.n, T.code, T.bitmaps)
    for tiles in _TILE_LISTS:
        cand = sel[np.isin(sel // TILE, tiles)]
        keys = np.sort(ref_keys(T.cols, cand, T.specs[:nkeys], T.ranks, T.seq, T.seq_bits))
        assert np.unique(keys).size == keys.size <= k.page_cap and (keys.size > 2000) == (len(tiles) > 2)
        bounds = [TOP, 0] + ([int(keys[keys.size // 2]), int(keys[keys.size // 5])] if keys.size else [12345])
        for bound in bounds:
            for kk, off in _PAGES:
                (rows, total, complete), want = _page(k, T, nkeys, tiles, kk, off, bound)
                assert np.array_equal(rows, want[0]) and (total, complete) == want[1:], (tiles, bound, kk, off)
            if bound not in (TOP, 0, 12345):  # the candidate at the bound: on the full page, not on the bounded one
                at = cand[ref_keys(T.cols, cand, T.specs[:nkeys], T.ranks, T.seq, T.seq_bits) == np.uint64(bound)]
                assert at.size == 1 and at[0] not in rows and total == int((keys < np.uint64(bound)).sum())
                (rows, _, _), _ = _page(k, T, nkeys, tiles, 8192, 0, TOP)
                assert at[0] in rows
    # a row count inside a 16-row group of the last tile: the live matches past it are not candidates
    n_cut = 4 * TILE + 16 * 203 + 5
    assert (sel >= n_cut).any() and ((sel >= n_cut) & (sel < n_cut + 11)).any()
    (rows, total, complete), want = _page(k, T, nkeys, [4, 0, 3], 8192, 0, TOP, n=n_cut)
    assert np.array_equal(rows, want[0]) and (total, complete) == want[1:] and rows.max() < n_cut


@pytest.mark.gpu
def test_gpu_page_overflow_is_counted_not_written(k, page_table):
    """More matches than the candidate buffer holds: every one is counted, none is written past
    the capacity, the page is reported incomplete, and the counter is reset for the next query."""
    import torch
    T, cap = page_table, k.page_cap
    true = [[OP_TRUE, 0, 0, 0]]
    (rows, total, complete), want = _page(k, T, 1, [1, 0], 100, 0, TOP, code=true, bitmaps=[0])
    assert (total, complete) == (2 * TILE, False) == want[1:]
    (rows, total, complete), want = _page(k, T, 2, [4, 0, 3], 1000, 400, TOP)  # the counter was reset
    assert np.array_equal(rows, want[0]) and (total, complete) == want[1:] and rows.size == 600
    # the same overflow into buffers of our own, with a sentinel tail
    ck = torch.full((cap + 64,), -0x5A5A5A5A5A5A5A5B, dtype=torch.int64, device=k.device)
    cr = torch.full((cap + 64,), -77, dtype=torch.int32, device=k.device)
    counter = torch.zeros(1, dtype=torch.int32, device=k.device)
    info = torch.full((4,), -1, dtype=torch.int32, device=k.device)
    out = torch.full((cap,), -1, dtype=torch.int32, device=k.device)
    tiles_t, prog_t = _dev(k, np.array([1, 0], dtype=np.int32)), _dev(k, np.array(true, dtype=np.int32))
    bm_t = _dev(k, np.zeros(1, dtype=np.int32))
    rc = k.lib.tt_launch_page(T.table.data_ptr(), T.n, T.live16.data_ptr(), prog_t.data_ptr(), 1, bm_t.data_ptr(), 1,
                              T.specs_t[1].data_ptr(), 1, T.ranks_t.data_ptr(), T.seq_t.data_ptr(), T.seq_bits,
                              tiles_t.data_ptr(), 2, ck.data_ptr(), cr.data_ptr(), counter.data_ptr(), 100, 0,
                              ctypes.c_uint64(TOP), info.data_ptr(), out.data_ptr(), k._stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert info.cpu().tolist() == [2 * TILE, 0, 100, 0] and int(counter.item()) == 0
    ck, cr = ck.cpu().numpy(), cr.cpu().numpy()
    assert (ck[cap:] == -0x5A5A5A5A5A5A5A5B).all() and (cr[cap:] == -77).all()
    # what did land is cap distinct rows of the two tiles, each with its own key
    assert np.unique(cr[:cap]).size == cap and cr[:cap].min() >= 0 and cr[:cap].max() < 2 * TILE
    assert np.array_equal(ck[:cap].view(np.uint64), ref_keys(T.cols, cr[:cap], T.specs[:1], T.ranks, T.seq, T.seq_bits))


# -- 3. bitmaps past the LDS stage
@pytest.mark.gpu
@pytest.mark.parametrize("extra", [0, 1])
def test_gpu_bitmaps_at_and_past_the_lds_limit(k, page_table, extra):
    """A 300-bit bitmap at the end of a tensor of exactly kMaxLdsBitmapWords words (staged in
    LDS) and of one more (read from global memory, no dynamic LDS), behind random filler:
    tt_scan_eval and tt_page_gather stage their bitmaps separately."""
    T, rng = page_table, np.random.default_rng(30 + extra)
    words = _limits(k)["bitmaps"] + extra
    bm = rng.integers(0, 1 << 32, words, dtype=np.uint64).astype(np.uint32)
    bm[-10:] &= rng.integers(0, 1 << 32, 10, dtype=np.uint64).astype(np.uint32)  # one bit in four
    bm[-1] |= np.uint32(1 << (299 - 9 * 32))  # the bits past 300 in the last word stay random
    code = [[OP_LEAF, 5, words - 10, 300]]
    got, want = _run_select(k, T, code, bm, return_mask=True)
    assert np.array_equal(got, want) and 3000 < want.size < k.page_cap
    assert (T.cols[5][0][want] == 299).any() and (T.cols[5][0] >= 300).any()
    for tiles in ([0, 1, 2, 3, 4], [4, 1]):
        (rows, total, complete), ref = _page(k, T, 0, tiles, 8192, 0, TOP, code=code, bitmaps=bm)
        assert np.array_equal(rows, ref[0]) and (total, complete) == ref[1:] and total > 1000, tiles
    assert total < want.size


# -- 5. zone argmin
@pytest.mark.gpu
@pytest.mark.parametrize("nkeys", [0, 2, 4])
def test_gpu_zone_argmin_over_key_counts_and_partial_tiles(k, page_table, nkeys):
    """tt_zone_argmin with 0, 2 and 4 keys, every tile in a permuted order, a row count that is
    not a multiple of the 32 rows a lane reads (as is, and cut to a multiple plus one), and a
    tile without a live row."""
    T = page_table
    assert T.n % 32 not in (0, 1)
    tiles = np.array([3, 0, 4, 2, 1], dtype=np.int32)
    for n in (T.n, 4 * TILE + 32 * 101 + 1):
        got = k.zone_argmin(T.table, T.live16, n, T.specs_t[nkeys], T.ranks_t, T.seq_t, T.seq_bits, tiles)
        for t, r in zip(tiles.tolist(), got.tolist()):
            rows = np.arange(t * TILE, min((t + 1) * TILE, n))
            rows = rows[T.live[rows]]
            keys = ref_keys(T.cols, rows, T.specs[:nkeys], T.ranks, T.seq, T.seq_bits)
            assert r == (int(rows[np.argmin(keys)]) if rows.size else -1), (n, t)
        assert got[3] == -1 and (got[[0, 1, 2, 4]] >= 0).all()
        # the last tile's first row in key order sits three rows past the cut count, in the same lane
        assert (got[2] == T.first) == (n == T.n) and n % 32 and T.first // 32 == (4 * TILE + 32 * 101 + 1) // 32


# -- 6. sort keys
@pytest.fixture(scope="module")
def sort_table(k):
    """About 600,000 rows, one column per width, a 20-bit sequence."""
    rng = np.random.default_rng(6)
    n, cap = 600_000, 74 * TILE
    cols = [(_ids(rng, n, 3), 0), (_ids(rng, n, 221), 1), (_ids(rng, n, 1100), 2), (_ids(rng, n, 7200), 4)]
    T = _Synth(k, cols, np.ones(n, dtype=bool), n, cap, seq=rng.permutation(1 << 20)[:n])
    T.seq_bits = 20
    T.row_sets = [np.sort(rng.choice(n, m, replace=False)).astype(np.int32) for m in (1, 255, 257, 2048 * 256 + 300)]
    return T


def _sort_plan(rng, words):
    """Four keys whose rank tables fill a rank tensor of exactly ``words`` words (the last table
    ends at the last word); ids past a table take the missing rank."""
    sizes = [3, 200, 1000, words - 1203]
    tables = [rng.permutation(s) + 1 for s in sizes]
    offs = np.cumsum([0] + sizes)
    bits4 = int(sizes[3]).bit_length()
    specs = np.array([[1, offs[1], 200, 8, 1, 0, 200, 0],
                      [2, offs[2], 1000, 10, 0, 5, 1000, 0],
                      [0, offs[0], 3, 2, 0, 0, 3, 0],
                      [3, offs[3], sizes[3], bits4, 1, 0, sizes[3], 0]], dtype=np.int32)
    return specs, np.concatenate(tables).astype(np.int32), 8 + 10 + 2 + bits4


@pytest.mark.gpu
@pytest.mark.parametrize("extra", [0, 1])
@pytest.mark.parametrize("nkeys", [0, 4])
def test_gpu_sort_keys_and_fused_histogram(k, sort_table, nkeys, extra):
    """tt_sort_keys against ref_keys, and its fused histogram against a bincount of the keys'
    12-bit digit: rank tables of exactly kLdsRankWords words (LDS) and one more (global memory),
    with and without the histogram in front of them in LDS, 1 .. 2048 * 256 + 300 rows (the second
    trip of the grid-stride loop), no key and four."""
    import torch
    T, lim = sort_table, _limits(k)
    specs, ranks, bits = _sort_plan(np.random.default_rng(60 + extra), lim["sort_ranks"] + extra)
    specs = specs[:nkeys]
    assert ranks.size == lim["sort_ranks"] + extra
    specs_t, ranks_t = _dev(k, specs), _dev(k, ranks)
    key_bits = (bits if nkeys else 0) + T.seq_bits
    assert T.row_sets[-1].size > 2048 * 256 and lim["bins"] == 4096
    for rows in T.row_sets:
        want = ref_keys(T.cols, rows, specs, ranks, T.seq, T.seq_bits)
        rows_t = _dev(k, rows)
        got = k.sort_keys(T.table, rows_t, specs_t, ranks_t, T.seq_t, T.seq_bits)
        assert np.array_equal(got.cpu().numpy().view(np.uint64), want), (rows.size, "no histogram")
        for shift in (0, key_bits - 12):
            hist = torch.zeros(lim["bins"], dtype=torch.int32, device=k.device)
            got = k.sort_keys(T.table, rows_t, specs_t, ranks_t, T.seq_t, T.seq_bits, hist, shift)
            assert np.array_equal(got.cpu().numpy().view(np.uint64), want), (rows.size, shift)
            digits = ((want >> np.uint64(shift)) & np.uint64(4095)).astype(np.int64)
            assert np.array_equal(hist.cpu().numpy(), np.bincount(digits, minlength=4096)), (rows.size, shift)
    if nkeys:  # the last word of the rank tensor was read, and ids past the last table took `missing`
        ids = T.cols[3][0][T.row_sets[-1]]
        assert (ids == specs[3, 2] - 1).any() and (ids >= specs[3, 2]).any()


# -- 7. top-k select
@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2, 4095, 4097, 8193])
def test_gpu_select_le_bin_odd_sizes_and_short_capacity(k, n):
    """tt_select_le_bin directly: odd sizes (the last pair of keys straddles n), an exact
    capacity (the pairs at or below the bin, as a set), and a capacity 10 short of the matches
    (counted in full, nothing written past the capacity)."""
    import torch
    rng = np.random.default_rng(70 + n)
    shift = 20
    keys = rng.integers(0, 1 << 32, n, dtype=np.uint64)
    keys[0] = 0  # bin 0 is never empty
    rows = rng.permutation(n).astype(np.int32)
    keys_t, rows_t = _dev(k, keys), _dev(k, rows)
    bins = ((keys >> np.uint64(shift)) & np.uint64(4095)).astype(np.int64)
    for last_bin in (0, 2047, 4095):
        match = bins <= last_bin
        count = int(match.sum())
        want = set(zip(keys[match].tolist(), rows[match].tolist()))
        assert count >= 1 and (n < 4000 or last_bin == 0 or count > 1000)
        for capacity in (count, max(0, count - 10)):
            ok = torch.full((count + 64,), -3, dtype=torch.int64, device=k.device)
            orr = torch.full((count + 64,), -5, dtype=torch.int32, device=k.device)
            counter = torch.zeros(1, dtype=torch.int32, device=k.device)
            rc = k.lib.tt_launch_select_le_bin(keys_t.data_ptr(), rows_t.data_ptr(), n, shift, last_bin, ok.data_ptr(),
                                               orr.data_ptr(), counter.data_ptr(), capacity, k._stream())
            assert rc == 0
            torch.cuda.synchronize()
            assert int(counter.item()) == count, (n, last_bin, capacity)
            ok, orr = ok.cpu().numpy(), orr.cpu().numpy()
            assert (ok[capacity:] == -3).all() and (orr[capacity:] == -5).all(), (n, last_bin, capacity)
            got = set(zip(ok[:capacity].view(np.uint64).tolist(), orr[:capacity].tolist()))
            assert len(got) == capacity and got <= want and (capacity < count or got == want), (n, last_bin, capacity)


@pytest.mark.gpu
@pytest.mark.parametrize("crowded", [True, False])
def test_gpu_order_top_k_declines_crowded_keys(k, crowded):
    """GpuKernels.order(k=10) without sort keys over 2**21 + 4099 rows.  Keys crowded into one
    histogram bin (40 key bits, sequences below 2**28): _top_k declines and the full sort
    answers.  Keys spread over the bins: _top_k answers.  Either way the first 10 of the
    stable order, and no sort fault."""
    import torch
    n = (1 << 21) + 4099
    rng = np.random.default_rng(77)
    seq_bits, key_bits = (28, 40) if crowded else (32, 32)
    seq = np.unique(rng.integers(0, 1 << seq_bits, n + n // 32, dtype=np.uint64))  # distinct sequences
    assert seq.size >= n
    seq = rng.permutation(seq)[:n].astype(np.uint32)
    cap = (n + TILE - 1) // TILE * TILE
    T = _Synth(k, [(np.zeros(1, dtype=np.int32), 1)], np.ones(n, dtype=bool), n, cap, seq=seq)
    rows = torch.arange(n, dtype=torch.int32, device=k.device)
    specs = torch.zeros((0, 8), dtype=torch.int32, device=k.device)
    ranks = torch.zeros(1, dtype=torch.int32, device=k.device)
    answers = []
    top_k = k._top_k
    k._top_k = lambda *a, **kw: answers.append(top_k(*a, **kw)) or answers[-1]
    try:
        got = k.order(T.table, rows, specs, ranks, T.seq_t, seq_bits, k=10, key_bits=key_bits)
    finally:
        del k._top_k
    assert len(answers) == 1 and (answers[0] is None) == crowded
    assert got.cpu().numpy().tolist() == np.argsort(seq, kind="stable")[:10].tolist()
    assert k.check_sort()


# -- 8. group count
@pytest.fixture(scope="module")
def group_table(k):
    rng = np.random.default_rng(8)
    n, cap = TILE + 21, 2 * TILE
    hi = _limits(k)["groups"] + 200
    cols = [(_ids(rng, n, 3), 0), (_ids(rng, n, 255), 1), (_ids(rng, n, hi), 2), (_ids(rng, n, hi), 4)]
    T = _Synth(k, cols, np.ones(n, dtype=bool), n, cap)
    T.selected = (rng.random(n) < 0.7) & np.repeat(rng.random(cap // 16) < 0.4, 16)[:n]  # most mask words are zero
    T.selected[rng.choice(n, 40, replace=False)] = True
    T.mask_t = _dev(k, _live16(T.selected, cap))
    return T


@pytest.mark.gpu
@pytest.mark.parametrize("width", [0, 1, 2, 4])
def test_gpu_group_count_over_widths_and_the_lds_limit(k, group_table, width):
    """tt_group_count == bincount on every code width; on 2- and 4-byte columns with as many
    groups as the LDS counters hold and one more (global atomics); ids at or past ``ngroups``
    and missing ids are ignored."""
    T, lim = group_table, _limits(k)["groups"]
    g = {0: 0, 1: 1, 2: 2, 4: 3}[width]
    ids = T.cols[g][0]
    if width >= 2:  # the last group of either size is hit by a selected row
        ids[np.nonzero(T.selected)[0][:2]] = [lim - 1, lim]
        T.tensors[g].copy_(_dev(k, _pack(ids, width, T.cap)))
    for ngroups in {0: (3, 2), 1: (200, 255), 2: (lim, lim + 1), 4: (lim, lim + 1)}[width]:
        picked = ids[T.selected]
        want = np.bincount(picked[(picked >= 0) & (picked < ngroups)], minlength=ngroups)
        got = k.group_count(T.table, g, T.mask_t, T.n, ngroups).cpu().numpy()
        assert np.array_equal(got, want), (width, ngroups)
        assert want[-1] > 0 and (picked < 0).any() and ((picked >= ngroups).any() or ngroups > MAX_ID[width])


@pytest.mark.gpu
def test_gpu_group_count_grid_stride_loop(k):
    """More 16-row slices than the launch has threads (2048 blocks x 256): the second trip of
    the grid-stride loop."""
    rng = np.random.default_rng(81)
    n = 2048 * 256 * 16 + 4099
    cap = (n + TILE - 1) // TILE * TILE
    ids = rng.integers(0, 255, n).astype(np.int32)
    ids[rng.random(n) < 0.05] = -1
    T = _Synth(k, [(ids, 1)], np.ones(n, dtype=bool), n, cap)
    selected = rng.random(n) < 0.3
    selected[-4099:] = True  # the rows only the second trip reaches
    got = k.group_count(T.table, 0, _dev(k, _live16(selected, cap)), n, 200).cpu().numpy()
    picked = ids[selected]
    assert np.array_equal(got, np.bincount(picked[(picked >= 0) & (picked < 200)], minlength=200))


# -- 9. rank encode
def _rank_encode_case(k, src_ids, src_w, table, dst_w, lo, hi, cap):
    import torch
    src_t, desc = _table(k, [(src_ids, src_w)], cap)
    np_dt, t_dt, miss = {1: (np.uint8, torch.uint8, 0xFF), 2: (np.uint16, torch.int16, 0xFFFF),
                         4: (np.int32, torch.int32, -1)}[dst_w]
    before = np.full(cap, 0xA5A5A5A5 & (0xFFFFFFFF >> (32 - 8 * dst_w)), dtype=np.uint32).astype(np_dt)
    dst = torch.from_numpy(before.view({1: np.uint8, 2: np.int16, 4: np.int32}[dst_w]).copy()).to(k.device)
    assert dst.dtype == t_dt
    k.rank_encode(desc, _dev(k, table.astype(np.int32)), lo, hi, dst, dst_w)
    got = dst.cpu().numpy().view(np_dt)
    ids = np.full(cap, -1, dtype=np.int64)
    ids[:src_ids.size] = src_ids
    ok = (ids >= 0) & (ids < table.size)
    want = before.copy()
    inside = np.where(ok, table[np.where(ok, ids, 0)], miss).astype(np.int64).astype(np_dt)
    want[lo:hi] = inside[lo:hi]
    assert np.array_equal(got, want), (src_w, dst_w, table.size, lo, hi)
    return ids, ok


@pytest.mark.gpu
@pytest.mark.parametrize("src_w", [0, 1, 2, 4])
def test_gpu_rank_encode_widths_ranges_and_the_lds_limit(k, src_w):
    """tt_rank_encode from every source width into every destination width that holds the
    largest rank, rank tables at the LDS limit and one past it (and small ones where the source
    width cannot reach the limit, so ids past the table exist), the short range (no aligned
    body), an aligned one and a long unaligned one; nothing outside [lo, hi) is written."""
    lim = _limits(k)["ranks"]
    rng = np.random.default_rng(90 + src_w)
    cap = 2 * TILE
    n = cap - 5  # the rows past n hold the missing code
    id_hi = {0: 3, 1: 255, 2: lim + 150, 4: lim + 150}[src_w]
    src = _ids(rng, n, id_hi)
    for nranks in {0: (2,), 1: (100,), 2: (), 4: ()}[src_w] + (lim, lim + 1):
        src[5:9] = [min(nranks, id_hi) - 1, min(nranks, id_hi - 1), -1, 0]  # inside every range below
        for dst_w, top in ((1, 254), (2, 65534), (4, (1 << 31) - 2)):
            table = rng.integers(1, top + 1, nranks)
            table[min(nranks, id_hi) - 1] = top
            for lo, hi in ((5, 11), (0, 16), (3, TILE + 37)):
                ids, ok = _rank_encode_case(k, src, src_w, table, dst_w, lo, hi, cap)
                assert ok[lo:hi].any() and (ids[lo:hi] < 0).any() and (nranks >= id_hi or (ids[lo:hi] >= nranks).any())


@pytest.mark.gpu
def test_gpu_rank_encode_grid_stride_loop(k):
    """More 16-row groups than the launch has threads (4096 blocks x 256): the body's second trip."""
    rng = np.random.default_rng(95)
    lo, hi = 3, 4096 * 256 * 16 + 37
    cap = (hi + 40 + TILE - 1) // TILE * TILE
    src = rng.integers(-1, 255, hi + 40).astype(np.int32)
    table = rng.integers(1, 255, 200)
    _rank_encode_case(k, src, 1, table, 1, lo, hi, cap)


# -- 10. width switches through ColumnarIndex
@pytest.mark.gpu
def test_gpu_queries_at_the_width_switches(k):
    """One column grown to 3, 4, 254, 255, 65,534 and 65,535 values: on either side of a switch of
    ``width_for`` the largest id and rank sit next to the all-ones code.  Filters, ordered page,
    full ordering and grouped count on the device equal the host at every size."""
    rnd = random.Random(10)
    ix = ColumnarIndex(["v"])
    col, made = ix.col_of["v"], 0

    def add(doc):
        ix.upsert(f"k{ix.n}", doc)

    expect = {3: (0, 1), 4: (1, 1), 254: (1, 1), 255: (2, 2), 65534: (2, 2), 65535: (4, 4)}
    for size, (width, rank_width) in expect.items():
        while made < size:
            add({"v": f"v{made:05d}"})
            made += 1
            if rnd.random() < 0.075:
                add({"other": 1})
        for _ in range(40):
            add({"v": f"v{rnd.randrange(made):05d}"} if rnd.random() > 0.07 else {"other": 2})
        add({"v": "v00001"})
        ix.delete(f"k{ix.n - 1}")  # a tombstone
        assert len(ix.columns[col].values) == size and ix.width_for(size) == width
        newest, oldest = f"v{size - 1:05d}", "v00000"
        for f in ({"EQ": {"v": newest}}, {"IN": {"v": [newest, oldest]}}, {"GTE": {"v": newest}},
                  {"NEQ": {"v": "absent"}}, {"AND": [{"LTE": {"v": newest}}, {"GT": {"v": oldest}}]}):
            prog = ix.compile(f)
            want = ix.select_numpy(prog)
            assert np.array_equal(ix.select_gpu(prog, k), want) and want.size, (size, f)
        assert ix.mirror.widths[col] == width and ix.mirror.ranks[col].w == rank_width
        sort = [{"key": "v", "order": "DESC"}]
        for q in ({"sort": sort, "page": {"limit": 50}}, {"sort": sort},
                  {"filter": {"LTE": {"v": newest}}, "sort": sort}):
            assert ix.query(q, k) == ix.query(q), (size, q)
        assert k.check_sort()
        prog = ix.compile({})
        assert ix.group_count_gpu(prog, "v", k) == ix.group_count_numpy(prog, "v"), size
