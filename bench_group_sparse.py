#!/usr/bin/env python3
"""The histogram of a sparse group space in the scan pass (``ops/hip/group_sparse.hip``
tt_scan_sparse) against the host path it replaces, by the method of ``bench_group_sums.py``: the
sides alternate, ``--reps`` rounds each after a warm-up of all, the median round counts, the spread
is the rounds' (max - min) / median; host clock around calls that end in a device synchronise.

One ``ColumnarIndex`` per (rows, values per group column): a filter column of 100 values and two
group columns of ``card`` values each, so (card + 1)^2 dense cells -- past ``tt_group_max_cells()``
from 2,048 values on.  ``GROUP BY g1, g2`` under a filter that selects 1 / 30 / 100 %:

  device   ``GpuKernels.scan_sparse`` over the mirror's buffers, with its table allocated and
           initialised, compacted and sorted on the device, and the occupied cells copied to the
           host (what ``ColumnarIndex.aggregate`` does from ``SPARSE_FROM_ROWS`` rows on)
  host     ``select_native`` + ``cells_of`` + ``np.unique`` (what it does below that, and did for
           every such request before the hashed scans)

The answers (cells and counts) are checked equal at every point; "overflow" there means the table,
capped at ``SPARSE_MAX_SLOTS``, was too small for the cells that occur and the scan said so (its time
is then the time of a refused attempt).  ``--orders``: ``sequential`` (g1
rises with the row, g2 cycles: neighbours share g1), ``shuffled`` (both random: about
min(rows, card^2) pairs), ``hot`` (shuffled, and half the rows hold one pair).  For orientation the
dense ``scan_group`` over two columns of 2,047 values (2,048^2 cells, the cap) on the same rows.

``--out`` appends the table (markdown).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))


def _stats(xs) -> tuple[float, float]:
    import numpy as np
    xs = np.asarray(xs, dtype=np.float64)
    return round(float(np.median(xs)), 4), round(float((xs.max() - xs.min()) / np.median(xs)), 3)


def _index(n: int, card: int, order: str, seed: int):
    """The index in columnar form: f (100 values), g1, g2 (``card`` values each)."""
    import numpy as np

    from aca_dotnet_workshop_amd.ops.columnar import Column, ColumnarIndex

    rng = np.random.default_rng(seed)
    ix = ColumnarIndex(capacity=n)
    cols = []
    for path, size in (("f", 100), ("g1", card), ("g2", card)):
        c = Column(path)
        c.encode_json_many([str(i) for i in range(size)], False)
        cols.append(c)
    ix.columns, ix.col_of = cols, {"f": 0, "g1": 1, "g2": 2}
    ix.ids = np.full((3, ix.cap), -1, dtype=np.int32)
    ix.ids[0, :n] = rng.integers(0, 100, n)
    if order == "sequential":
        ix.ids[1, :n] = np.arange(n, dtype=np.int64) * card // n
        ix.ids[2, :n] = np.arange(n) % card
    else:
        ix.ids[1, :n] = rng.integers(0, card, n)
        ix.ids[2, :n] = rng.integers(0, card, n)
        if order == "hot":
            hot = rng.random(n) < 0.5
            ix.ids[1, :n][hot] = card // 2
            ix.ids[2, :n][hot] = card // 3
    ix.live[:n] = 1
    ix.seq[:n] = np.arange(1, n + 1)
    ix._next_seq = n
    ix.n = n
    ix.keys = []
    ix.version += 1
    ix.mirror.invalidate()
    return ix


def bench(a) -> dict:
    import numpy as np
    import torch

    from aca_dotnet_workshop_amd.ops.gpu import GpuKernels

    k = GpuKernels("cuda:0")
    cap_cells = int(k.lib.tt_group_max_cells())
    points = []
    for n in a.rows:
        for card in a.cards:
            for order in a.orders:
                ix = _index(n, card, order, seed=n % 1000 + card)
                dims = [card, card]
                ncells = (card + 1) ** 2
                slots = min(ix.SPARSE_MAX_SLOTS, max(2, 1 << (2 * min(ncells, n) - 1).bit_length()))
                for pct in a.pcts:
                    prog = ix.compile_cached({"LT": {"f": pct}})
                    m, code, bitmaps = ix.mirror.program(prog, k)

                    def device():
                        got = k.scan_sparse(m.table, m.live, ix.cap, ix.n, code, bitmaps, [1, 2], dims, slots)
                        return None if got is None else tuple(t.cpu().numpy() for t in got)

                    def host():
                        rows = ix.select_native(prog)
                        return np.unique(ix.cells_of(rows, [1, 2], dims), return_counts=True)

                    def dense():
                        return k.scan_group(m.table, m.live, ix.cap, ix.n, code, bitmaps, [1, 2], dims).cpu()

                    fns = [device, host] + ([dense] if ncells <= cap_cells else [])
                    d, h = device(), host()
                    # None: more cells occur than the capped table takes (the planner then asks the host)
                    same = "overflow" if d is None else bool(
                        np.array_equal(d[0], h[0]) and np.array_equal(d[1].view(np.uint32).astype(np.int64), h[1]))
                    # the host side is seconds per call at 1e8 rows: fewer calls there
                    iters = [a.iters, max(1, min(a.iters, int(2e7 // max(n, 1)))), a.iters]

                    def once(fn, it: int) -> float:
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        for _ in range(it):
                            fn()
                        torch.cuda.synchronize()
                        return (time.perf_counter() - t0) / it

                    for fn in fns[:1] + fns[2:]:
                        for _ in range(a.warmup):
                            fn()
                    rounds = [[once(fn, it) * 1e3 for fn, it in zip(fns, iters)] for _ in range(a.reps)]
                    st = [_stats([r[i] for r in rounds]) for i in range(len(fns))]
                    points.append({"rows": n, "card": card, "order": order, "selectivity_pct": pct,
                                   "selected": int(h[1].sum()), "groups": int(h[0].size), "slots": slots,
                                   "device_ms": st[0][0], "host_ms": st[1][0], "device_spread": st[0][1],
                                   "host_spread": st[1][1], "dense_ms": st[2][0] if len(st) > 2 else None,
                                   "answers_equal": same})
                    print(json.dumps(points[-1]), file=sys.stderr, flush=True)
                del ix
    res = {"metric": "group_sparse_vs_host_selection", "iters": a.iters, "reps": a.reps,
           "device": torch.cuda.get_device_name(0), "points": points}
    if a.out:
        with open(a.out, "a") as f:
            f.write(f"## `scan_sparse` against `select_native` + `np.unique`\n\n{res['device']}, median of {a.reps} "
                    f"rounds of {a.iters} calls (host: fewer from 1e7 rows on), the sides alternating "
                    f"(`bench_group_sparse.py`).  dense: `scan_group` where the cells fit its cap.\n\n"
                    "| rows | values / column | order | selected | groups | slots | device ms | host ms | host / device "
                    "| dense ms | spread d / h | answers equal |\n|---|---|---|---|---|---|---|---|---|---|---|---|\n")
            for p in points:
                dense = "" if p["dense_ms"] is None else f"{p['dense_ms']:.4f}"
                f.write(f"| {p['rows']:,} | {p['card']:,} | {p['order']} | {p['selectivity_pct']} % ({p['selected']:,}) | "
                        f"{p['groups']:,} | {p['slots']:,} | {p['device_ms']:.4f} | {p['host_ms']:.3f} | "
                        f"{p['host_ms'] / p['device_ms']:.1f} | {dense} | {p['device_spread']:.2f} / "
                        f"{p['host_spread']:.2f} | {p['answers_equal']} |\n")
            f.write("\n")
    return res


def main() -> None:
    ints = lambda s: [int(float(x)) for x in s.split(",")]  # noqa: E731
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=ints, default=ints("1e6,1e7,1e8"))
    ap.add_argument("--cards", type=ints, default=ints("2100,10000,100000"), help="values per group column")
    ap.add_argument("--pcts", type=ints, default=ints("1,30,100"))
    ap.add_argument("--orders", type=lambda s: s.split(","), default=["sequential", "shuffled", "hot"])
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=3, help="alternating rounds per point")
    ap.add_argument("--out", default="", help="append the table (markdown) here")
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    print(json.dumps(bench(a)), flush=True)


if __name__ == "__main__":
    main()
