#!/usr/bin/env python3
"""Exact SUM / AVG per group in the scan pass (``ops/hip/group_sums.hip`` tt_scan_sums), measured
two ways, by the method of ``bench_group_extrema.py``: the sides alternate, ``--reps`` rounds each
after a warm-up of all, the median round counts, the spread is the rounds' (max - min) / median;
host clock around calls that end in a device synchronise.

(a) default -- kernel against kernel: ``tt_scan_sums`` (group columns + a 4-byte id column no two
    rows share an id of, gathering from an int64 table of one entry per row) against
    ``tt_scan_extrema`` over the same columns and against ``tt_scan_group`` over the group columns
    alone (the same scan less the value: the floor).  ``--rows`` rows (1e8), a range filter
    selecting 1 / 30 / 100 %, 1 (no group column) / 200 / 100,000 groups.  ``--order``: the ids in
    row order (a key written in order: the gather is sequential) or shuffled.

(b) ``--query`` -- ``ColumnarIndex.aggregate(q, kernels)`` for SUM + AVG of an integer key hardly
    two rows share, grouped by a 200-value column, over ``--query-rows`` rows: this tree against
    the tree at ``--against`` (a checkout of the parent commit with its library built, where the
    histogram is past the device cap and the host counts it and loops).  Each round starts one
    fresh child process per tree (``--query-child``).

``--out`` appends the table (markdown).
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))


def _stats(xs) -> tuple[float, float]:
    import numpy as np
    xs = np.asarray(xs, dtype=np.float64)
    return round(float(np.median(xs)), 4), round(float((xs.max() - xs.min()) / np.median(xs)), 3)


def kernel_bench(a) -> dict:
    import numpy as np
    import torch

    from aca_dotnet_workshop_amd.ops.columnar import OP_RANGE, TILE
    from aca_dotnet_workshop_amd.ops.gpu import GpuKernels

    k = GpuKernels("cuda:0")
    dev = k.device
    n = a.rows
    cap = (n + TILE - 1) // TILE * TILE
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)

    def column(card: int, width: int):
        ids = torch.randint(0, card, (cap,), device=dev, generator=gen, dtype=torch.int32)
        return ids if width == 4 else ids.to(torch.uint8)

    groups = [(1, None), (200, 1), (100_000, 4)]
    widths = [1] + [w for _, w in groups[1:]] + [4]
    # column 0: the filter's; 1..2: the group columns; 3: the value's ids, one per row
    ids = torch.arange(cap, device=dev, dtype=torch.int32) if a.order == "sequential" else \
        torch.randperm(cap, device=dev, generator=gen).to(torch.int32)
    tensors = [column(100, 1)] + [column(card, w) for card, w in groups[1:]] + [ids]
    value = len(tensors) - 1
    nums = torch.randint(-(1 << 20), 1 << 20, (cap,), device=dev, generator=gen, dtype=torch.int64)
    table = torch.tensor([[t.data_ptr(), w] for t, w in zip(tensors, widths)], dtype=torch.int64).to(dev)
    live = torch.full((cap // 16,), -1, dtype=torch.int16, device=dev)  # rows < n live, 16 bits per word
    live[(n + 15) // 16:] = 0
    if n % 16:
        live[n // 16] = (1 << (n % 16)) - 1
    bitmaps = torch.zeros(1, dtype=torch.int32, device=dev)

    def once(fn, iters: int) -> float:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
            torch.cuda.synchronize()  # as the caller, which reads the cells back after each
        return (time.perf_counter() - t0) / iters

    points = []
    for pct in (1, 30, 100):
        code = torch.tensor([[OP_RANGE, 0, 0, pct]], dtype=torch.int32).to(dev)  # ids 0 .. pct-1 of 100
        for g, (card, w) in enumerate(groups):
            keys, dims = ([], []) if w is None else ([g], [card])
            fns = (lambda: k.scan_sums(table, live, cap, n, code, bitmaps, keys, dims, value, nums),
                   lambda: k.scan_extrema(table, live, cap, n, code, bitmaps, keys, dims, value),
                   lambda: k.scan_group(table, live, cap, n, code, bitmaps, keys, dims))
            s, h = fns[0](), fns[2]().cpu().numpy()
            same = bool(np.array_equal(s[0].cpu().numpy(), h)) and \
                bool((s[1].cpu().numpy().astype(np.float64) <= s[2].cpu().numpy().astype(np.float64)).all())
            for _ in range(a.warmup):
                for fn in fns:
                    fn()
            rounds = [[once(fn, a.iters) * 1e3 for fn in fns] for _ in range(a.reps)]
            (sm, sms), (ex, exs), (hs, hss) = (_stats([r[i] for r in rounds]) for i in range(3))
            points.append({"selectivity_pct": pct, "groups": card, "selected": int(h.astype(np.int64).sum()),
                           "sums_ms": sm, "extrema_ms": ex, "histogram_ms": hs, "sums_spread": sms,
                           "extrema_spread": exs, "histogram_spread": hss, "counts_equal": same})
    res = {"metric": "group_sums_vs_extrema_vs_histogram", "rows": n, "order": a.order, "iters": a.iters,
           "reps": a.reps, "device": torch.cuda.get_device_name(0), "points": points}
    if a.out:
        with open(a.out, "a") as f:
            f.write(f"## (a) `tt_scan_sums` against `tt_scan_extrema` and `tt_scan_group`, ids {a.order}\n\n"
                    f"{res['device']}, {n:,} rows, median of {a.reps} rounds of {a.iters} calls, the three kernels "
                    f"alternating (`bench_group_sums.py --order {a.order}`).  The histogram reads no value column: "
                    f"the floor.\n\n"
                    "| selected | groups | sums ms | extrema ms | histogram ms | sums / extrema | sums / histogram "
                    "| spread s / e / h | counts equal |\n|---|---|---|---|---|---|---|---|---|\n")
            for p in points:
                f.write(f"| {p['selectivity_pct']} % ({p['selected']:,}) | {p['groups']:,} | {p['sums_ms']:.4f} | "
                        f"{p['extrema_ms']:.4f} | {p['histogram_ms']:.4f} | {p['sums_ms'] / p['extrema_ms']:.2f} | "
                        f"{p['sums_ms'] / p['histogram_ms']:.2f} | {p['sums_spread']:.2f} / {p['extrema_spread']:.2f} / "
                        f"{p['histogram_spread']:.2f} | {p['counts_equal']} |\n")
            f.write("\n")
    return res


QUERY = {"groupBy": ["taskAssignedTo"], "aggregate": [{"op": "SUM", "key": "taskPoints"},
                                                      {"op": "AVG", "key": "taskPoints"}]}


def query_child(a) -> dict:
    """One tree's side of one round: the index in columnar form (200 assignees, an integer per row
    in no order), ``--warmup`` calls, then ``--iters`` timed ones."""
    import hashlib

    import numpy as np
    import torch

    from aca_dotnet_workshop_amd.ops.columnar import Column, ColumnarIndex
    from aca_dotnet_workshop_amd.ops.gpu import GpuKernels

    n = a.query_rows
    rng = np.random.default_rng(0)
    ix = ColumnarIndex(capacity=n)
    who = Column("taskAssignedTo")
    for i in range(200):
        who.encode(f"user{i}@bench")
    points = Column("taskPoints")
    points.encode_json_many([str(7 * i) for i in rng.permutation(n).tolist()], False)
    ix.columns, ix.col_of = [who, points], {"taskAssignedTo": 0, "taskPoints": 1}
    ix.ids = np.full((2, ix.cap), -1, dtype=np.int32)
    ix.ids[0, :n] = rng.integers(0, 200, n)
    ix.ids[1, :n] = np.arange(n)
    ix.live[:n] = 1
    ix.seq[:n] = np.arange(1, n + 1)
    ix._next_seq = n
    ix.n = n
    ix.keys = []
    ix.version += 1
    ix.mirror.invalidate()
    k = GpuKernels("cuda:0")
    for _ in range(a.warmup):
        res = ix.aggregate(QUERY, k)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.iters):
        res = ix.aggregate(QUERY, k)
    dt = (time.perf_counter() - t0) / a.iters
    return {"ms": dt * 1e3, "groups": len(res["groups"]), "sum_scans": getattr(k, "sum_scans", None),
            "answer_sha": hashlib.sha256(json.dumps(res, sort_keys=True).encode()).hexdigest()[:16],
            "device": torch.cuda.get_device_name(0)}


def query_bench(a) -> dict:
    def child(root: str) -> dict:
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--query-child", "--root", root,
                              "--query-rows", str(a.query_rows), "--iters", str(a.iters), "--warmup", str(a.warmup)],
                             check=True, capture_output=True, text=True, timeout=a.child_timeout).stdout
        return json.loads(out.strip().splitlines()[-1])
    rounds = [(child(ROOT), child(os.path.abspath(a.against))) for _ in range(a.reps)]
    (new, news), (old, olds) = (_stats([r[i]["ms"] for r in rounds]) for i in (0, 1))
    first = rounds[0]
    res = {"metric": "aggregate_sum_avg_unique_key_vs_parent", "rows": a.query_rows, "iters": a.iters, "reps": a.reps,
           "device": first[0]["device"], "this_ms": new, "parent_ms": old, "this_spread": news, "parent_spread": olds,
           "groups": first[0]["groups"], "answers_equal": all(x["answer_sha"] == y["answer_sha"] for x, y in rounds),
           "this_sum_scans": first[0]["sum_scans"], "parent_sum_scans": first[1]["sum_scans"]}
    if a.out:
        with open(a.out, "a") as f:
            f.write(f"## (b) `ColumnarIndex.aggregate`: SUM + AVG of an integer key hardly two rows share, 200 groups\n\n"
                    f"{res['device']}, {a.query_rows:,} rows, median of {a.reps} rounds of {a.iters} calls, a fresh "
                    f"process per tree and round, the two trees alternating (`bench_group_sums.py --query`).  "
                    f"The parent's histogram of 201 x {a.query_rows + 1:,} cells is past the device cap: the host "
                    f"selects, counts and loops.\n\n"
                    "| this tree ms | parent ms | parent / this | spread this / parent | answers equal |\n"
                    "|---|---|---|---|---|\n"
                    f"| {new:.2f} | {old:.2f} | {old / new:.1f} | {news:.2f} / {olds:.2f} | {res['answers_equal']} |\n\n")
    return res


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--order", choices=["sequential", "shuffled"], default="sequential")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5, help="alternating rounds per point")
    ap.add_argument("--out", default="", help="append the table (markdown) here")
    ap.add_argument("--query", action="store_true", help="instead: (b), the whole aggregate call against --against")
    ap.add_argument("--against", default="", help="--query: the other tree (the parent commit, library built)")
    ap.add_argument("--query-rows", type=int, default=1_000_000)
    ap.add_argument("--child-timeout", type=float, default=300.0)
    ap.add_argument("--query-child", action="store_true", help="(internal) one tree's side of one --query round")
    ap.add_argument("--root", default=ROOT, help="(internal) the tree --query-child imports the package from")
    a = ap.parse_args()
    sys.path.insert(0, a.root if a.query_child else ROOT)
    if a.query_child:
        res = query_child(a)
    elif a.query:
        if not a.against:
            ap.error("--query needs --against")
        res = query_bench(a)
    else:
        res = kernel_bench(a)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
