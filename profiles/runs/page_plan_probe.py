"""Where a sweep query's host time goes on the GPU path (page plan + program).

A native DocStore with the column mirror on, 400 k tasks (the headline's mirror size), then
rounds of: ~1,300 new tasks (what 20 ms of the headline's create rate adds), the mirror sync,
and the sweep's own query (range + two booleans, ORDER BY taskCreatedOn, page of 4,096) through
ColumnarIndex.page_gpu on the gfx950 kernels.  Prints the index's phase timings per query and a
cProfile of the plan + program phases.  Run on the GPU box:

    python profiles/runs/page_plan_probe.py > gpurun_out/probe/plan.txt
"""
import cProfile
import json
import pstats
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))

import numpy as np  # noqa: E402

from aca_dotnet_workshop_amd.native import load  # noqa: E402
from aca_dotnet_workshop_amd.ops.columnar import ColumnarIndex  # noqa: E402
from aca_dotnet_workshop_amd.ops.gpu import GpuKernels  # noqa: E402

N = load()
PREFIX = "tasksmanager-backend-api||"


def doc(i: int) -> str:
    us = 37 * i
    ts = f"2025-01-01T{us // 3_600_000_000 % 24:02d}:{us // 60_000_000 % 60:02d}:{us // 1_000_000 % 60:02d}.{us % 1_000_000:06d}0"
    due = "2024-12-01T00:00:00" if i % 64 == 0 else f"2025-0{2 + i % 7}-{1 + i % 28:02d}T00:00:00"
    return json.dumps({"taskId": f"{i:08d}-aaaa-bbbb-cccc-dddddddddddd", "taskName": f"Task {i}",
                       "taskCreatedBy": f"u{i % 4096}@bench.local", "taskCreatedOn": ts, "taskDueDate": due,
                       "taskAssignedTo": "someone@mail.com", "isCompleted": False, "isOverDue": False})


def main() -> None:
    store = N.DocStore("", 0, 256)
    n = 400_000
    t0 = time.perf_counter()
    for i in range(n):
        store.set(f"{PREFIX}{i:08d}", doc(i))
    print(f"filled {n} in {time.perf_counter() - t0:.1f} s", flush=True)
    q = {"filter": {"AND": [{"EQ": {"\u0000keyprefix": PREFIX}},
                            {"AND": [{"LT": {"taskDueDate": "2025-01-01T00:00:00"}}, {"EQ": {"isCompleted": False}},
                                     {"EQ": {"isOverDue": False}}]}]},
         "sort": [{"key": "taskCreatedOn", "order": "ASC"}], "page": {"limit": 4096}}
    paths = ["\u0000keyprefix", "taskDueDate", "isCompleted", "isOverDue", "taskCreatedOn"]
    ix = ColumnarIndex.from_native(store, paths)
    k = GpuKernels()
    ix.sync()
    rows, _ = ix.query_rows(q, k)  # warm: plan, zones, device columns
    print(f"first page: {rows.size} rows", flush=True)
    prof = cProfile.Profile()
    per = []
    i = n
    for rnd in range(40):
        for _ in range(1300):
            store.set(f"{PREFIX}{i:08d}", doc(i))
            i += 1
        before = dict(ix.mirror.timing)
        t = time.perf_counter()
        ix.sync()
        t_sync = time.perf_counter() - t
        if rnd >= 10:
            prof.enable()
        t = time.perf_counter()
        rows, _ = ix.query_rows(q, k)
        t_q = time.perf_counter() - t
        if rnd >= 10:
            prof.disable()
            d = {key: ix.mirror.timing.get(key, 0.0) - before.get(key, 0.0) for key in ix.mirror.timing}
            per.append((t_sync * 1e3, t_q * 1e3, d))
    print("per query (ms, median of 30): sync %.3f, query %.3f" % (np.median([p[0] for p in per]), np.median([p[1] for p in per])))
    for key in ("page_plan_ms", "page_program_ms", "page_zones_ms", "page_kernels_ms"):
        print(f"  {key}: {np.median([p[2].get(key, 0.0) for p in per]):.3f}")
    print(f"kernels: uploads {k.uploads}, segments {k.upload_segments}")
    st = pstats.Stats(prof)
    st.sort_stats("cumulative").print_stats(35)
    st.sort_stats("tottime").print_stats(25)


if __name__ == "__main__":
    main()
