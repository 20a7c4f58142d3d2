"""Columnar, dictionary-encoded mirror of a state-store collection + the query compiler.

Why: the reference's queries (``EQ taskCreatedBy``, ``EQ taskDueDate`` then in-app
filtering, Services/TasksStoreManager.cs:54-69, 104-139) are whole-collection scans in
Cosmos; equality is served by the native store's hash indexes, but range/NEQ/OR filters,
the corrected overdue sweep (``taskDueDate < today AND NOT isCompleted AND NOT isOverDue``)
and dashboard aggregates (open tasks per assignee) are O(collection).  Those run here,
on the GPU when one is present (``ops/hip/query_scan.hip``), with a NumPy executor of the
*same* compiled program as the CPU path and as the correctness oracle.

Encoding: each indexed JSON path is an int32 column of dictionary ids (-1 = path missing).
Equality and ordering semantics are evaluated on the host against the (small) dictionary,
exactly mirroring the native engine's ``compare`` (type order null < bool < number < string;
numbers by value; ranges only between like types), producing one bitmap per leaf.
"""
from __future__ import annotations

import functools
import itertools
import json
import math
import operator
import os
from dataclasses import dataclass, field
from typing import Any, Iterable, NamedTuple

import numpy as np

from .codes import (MAX_DEPTH, OP_AND, OP_EQ, OP_LEAF, OP_NOT, OP_OR, OP_RANGE, OP_TRUE, TILE, col_bytes,
                    encode_codes, gather, width_for)
from .device_mirror import DeviceMirror

_TYPE_ORDER = {type(None): 0, bool: 1, int: 2, float: 2, str: 3, list: 4, dict: 5}


@functools.lru_cache(maxsize=1)
def cpu_share() -> int:
    """CPUs this process may use: the cgroup quota (``cpu.max``) when set, else its affinity
    (read once per process)."""
    try:
        with open("/sys/fs/cgroup/cpu.max") as f:
            quota, period = f.read().split()[:2]
        if quota != "max":
            return max(1, int(quota) // int(period))
    except (OSError, ValueError):
        pass
    return max(1, len(os.sched_getaffinity(0)))


class Unsupported(Exception):
    """Filter cannot run on the columnar engine (caller falls back to the native store)."""


def vkey(v: Any) -> str:
    """Canonical dictionary key with the native engine's equality semantics."""
    if v is None:
        return "n"
    if isinstance(v, bool):
        return "b1" if v else "b0"
    if isinstance(v, (int, float)):
        return "d" + repr(float(v) + 0.0)  # + 0.0 folds -0.0 into 0.0 (IEEE equality)
    if isinstance(v, str):
        return "s" + v
    return "j" + json.dumps(_norm(v), separators=(",", ":"))


def _norm(v: Any) -> Any:
    if isinstance(v, bool) or v is None or isinstance(v, str):
        return v
    if isinstance(v, (int, float)):
        return float(v) + 0.0
    if isinstance(v, list):
        return [_norm(x) for x in v]
    if isinstance(v, dict):
        return {k: _norm(x) for k, x in v.items()}
    return v


def type_rank(v: Any) -> int:
    return _TYPE_ORDER.get(type(v), 6)


def compare(a: Any, b: Any) -> int:
    ta, tb = type_rank(a), type_rank(b)
    if ta != tb:
        return -1 if ta < tb else 1
    if ta == 0:
        return 0
    if ta in (1, 2, 3):
        return (a > b) - (a < b)
    if ta == 4:
        for x, y in zip(a, b):
            c = compare(x, y)
            if c:
                return c
        return (len(a) > len(b)) - (len(a) < len(b))
    sa, sb = json.dumps(a, separators=(",", ":")), json.dumps(b, separators=(",", ":"))
    return (sa > sb) - (sa < sb)


_MISSING = object()


def get_path(doc: Any, path: str) -> Any:
    cur = doc
    for seg in path.split("."):
        if isinstance(cur, dict):
            if seg in cur:
                cur = cur[seg]
            else:
                low = seg.lower()
                for k, v in cur.items():
                    if k.lower() == low:
                        cur = v
                        break
                else:
                    return _MISSING
        elif isinstance(cur, list) and seg.isdigit():
            i = int(seg)
            if i >= len(cur):
                return _MISSING
            cur = cur[i]
        else:
            return _MISSING
    return cur


def filter_paths(f: Any) -> list[str]:
    """Every document path a filter references (so all columns are encoded in one pass)."""
    out: list[str] = []
    if isinstance(f, dict) and len(f) == 1:
        (op, arg), = f.items()
        if op.upper() in ("AND", "OR") and isinstance(arg, list):
            for x in arg:
                out += filter_paths(x)
        elif isinstance(arg, dict) and len(arg) == 1:
            out.append(next(iter(arg)))
    return out


# -- grouped aggregates: the semantics, shared by every execution path -----------------------
# GPU (hip/group_agg.hip), CPU columnar, the native engine's documents (backing/server.py) and
# the shard merge (backing/shards.py) all reduce to per-group histograms of (value, row count)
# held in ``AggGroups`` and finish in ``reduce_hist``: one definition, one answer.  A key of which
# only COUNT / MIN / MAX are asked may instead arrive as per-group extrema (hip/group_extrema.hip,
# ``ColumnarIndex.extrema_numpy``, a shard's ``project=partial``), merged by ``compare``.
AGG_OPS = ("COUNT", "SUM", "AVG", "MIN", "MAX")
MAX_GROUP_BY = 2


def _canon(v: Any) -> Any:
    """One representative per ``vkey`` class of numbers (1 and 1.0 are one dictionary value,
    and which was written first differs between the paths): integral below 2^53 as int, else float."""
    if isinstance(v, bool) or not isinstance(v, (int, float)):
        return v
    f = float(v) + 0.0
    return int(f) if f.is_integer() and abs(f) < 2.0 ** 53 else f


def reduce_hist(hist: Iterable[tuple[Any, int]], ops: Iterable[str]) -> dict[str, Any]:
    """The aggregates ``ops`` of one path within one group from its histogram -- (JSON value,
    rows holding it) pairs, rows where the path is missing not among them -- undivided:
    COUNT = rows where the path is defined; SUM over int and float values (not bool), correctly
    rounded (``fsum``: the order of the pairs does not matter); AVG = (numeric sum, numeric
    rows), divided last by the caller; MIN / MAX by ``compare``.  An aggregate without an
    eligible value is left out (COUNT is 0 then)."""
    hist = [(v, int(c)) for v, c in hist if c]
    nums = [(v, c) for v, c in hist if type_rank(v) == 2]
    out: dict[str, Any] = {}
    for op in ops:
        if op == "COUNT":
            out[op] = sum(c for _, c in hist)
        elif op in ("SUM", "AVG") and nums:
            s = math.fsum(float(v) * c for v, c in nums)
            out[op] = s if op == "SUM" else (s, sum(c for _, c in nums))
        elif op in ("MIN", "MAX") and hist:
            best = hist[0][0]
            for v, _ in hist[1:]:
                c = compare(v, best)
                if (c < 0) if op == "MIN" else (c > 0):
                    best = v
            out[op] = best
    return out


@dataclass
class AggSpec:
    filter: Any
    group_by: list[str]
    aggs: list[tuple[str, str | None]]   # (op, key); key None = COUNT of the group's rows
    keys: list[str]                      # the distinct aggregate keys, in request order


def parse_aggregate(q: Any) -> AggSpec:
    """The aggregate request body, validated (ValueError = the route's 400)."""
    if not isinstance(q, dict):
        raise ValueError("aggregate request must be a JSON object")
    group_by = q.get("groupBy") or []
    if not isinstance(group_by, list) or len(group_by) > MAX_GROUP_BY:
        raise ValueError(f"groupBy takes at most {MAX_GROUP_BY} paths")
    aggs: list[tuple[str, str | None]] = []
    raw = q.get("aggregate") or []
    if not isinstance(raw, list):
        raise ValueError("aggregate must be an array")
    for a in raw:
        op = a.get("op") if isinstance(a, dict) else None
        op = op.upper() if isinstance(op, str) else op
        if op not in AGG_OPS:
            raise ValueError(f"unknown aggregate op {op!r}")
        key = a.get("key")
        if key is None and op != "COUNT":
            raise ValueError(f"{op} needs a key")
        aggs.append((op, key))
    for p in [*group_by, *(k for _, k in aggs if k is not None)]:
        if not isinstance(p, str) or not p or p.startswith("\x00"):
            raise ValueError("a path must be a non-empty string that does not begin with NUL")
    flt = q.get("filter")
    if flt is not None and not isinstance(flt, dict):
        raise ValueError("filter must be an object")
    return AggSpec(flt or None, list(group_by), aggs, list(dict.fromkeys(k for _, k in aggs if k is not None)))


EXTREMA_OPS = frozenset(("COUNT", "MIN", "MAX"))


def extrema_keys(spec: AggSpec) -> list[str]:
    """The aggregate keys of which only COUNT, MIN and MAX are asked: three numbers per group
    answer them (``AggGroups.add_extrema``), no histogram is needed."""
    return [k for k in spec.keys if all(op in EXTREMA_OPS for op, kk in spec.aggs if kk == k)]


def sum_keys(spec: AggSpec) -> list[str]:
    """The aggregate keys that are asked a SUM or an AVG: exact scaled-integer sums per group can
    answer those (``AggGroups.add_sums``), their COUNT / MIN / MAX then come from extrema."""
    return [k for k in spec.keys if any(op in ("SUM", "AVG") for op, kk in spec.aggs if kk == k)]


class Inexact(Exception):
    """A group's scaled-integer sums cannot prove its SUM (``AggGroups``): the sum of magnitudes
    reached 2^53.  The histograms answer (``hist=True``); not a malformed request."""


def _scaled(v: Any) -> tuple[int, int] | None:
    """(m, e), ``float(v) == m * 2^e`` exactly with e <= 0; None for a number that is not finite."""
    try:
        num, den = float(v).as_integer_ratio()
    except (OverflowError, ValueError):
        return None
    return num, 1 - den.bit_length()


class AggGroups:
    """Per group (the group-by values, a missing path apart from JSON null): its row count and,
    per aggregate key, the histogram of the key's values -- or, for a key of ``extrema_keys``,
    its extrema: [rows where it is defined, smallest value, largest value].  Counts of equal
    groups and values (``vkey``) add and extrema merge by ``compare``, so partial answers --
    launches, shards -- merge by adding themselves.  Which form a key is held in follows from
    the request and the path taken, the same for every part of one answer.

    A key of ``sum_keys`` may also be held as sums of scaled integers, ``[nums, S, A, e]``: over
    the ``nums`` rows whose value is a number ``m * 2^e``, S = the sum of the m and A = the sum
    of the |m| (Python ints), with extrema next to them when COUNT / MIN / MAX are asked too.
    While A < 2^53 every product value x rows is exact in a double and so is their sum:
    ``reduce_hist``'s correctly rounded SUM is ``ldexp(S, e)``.  Such sums merge with one another
    (rescaled to the smaller e) and with histograms of the same key from parts below the
    threshold, whose numeric pairs are folded in exactly; at A >= 2^53 the reduction raises
    ``Inexact`` and the caller asks for histograms."""

    def __init__(self, spec: AggSpec) -> None:
        self.spec = spec
        self.groups: dict[tuple, dict[str, Any]] = {}
        if not spec.group_by:
            self._group(())  # no GROUP BY: one group, also over an empty selection

    def _group(self, gvals: tuple) -> dict[str, Any]:
        gk = tuple(None if v is _MISSING else vkey(v) for v in gvals)
        g = self.groups.get(gk)
        if g is None:
            g = self.groups[gk] = {"values": tuple(v if v is _MISSING else _canon(v) for v in gvals), "count": 0,
                                   "hist": {k: {} for k in self.spec.keys}, "ext": {}, "sum": {}}
        return g

    def add_sums(self, gvals: tuple, key: str, nums: int, s: int = 0, a: int = 0, e: int = 0) -> None:
        """``nums`` rows of the group hold a number under ``key``, ``s`` and ``a`` the sums of
        their m and |m| at the quantum 2^``e``; nothing when ``nums`` is 0."""
        if not nums:
            return
        sums = self._group(gvals)["sum"]
        cur = sums.get(key)
        sums[key] = [int(nums), int(s), int(a), int(e)] if cur is None else \
            self._merged(cur, [int(nums), int(s), int(a), int(e)])

    @staticmethod
    def _merged(x: list, y: list) -> list:
        e = min(x[3], y[3])
        return [x[0] + y[0], (x[1] << (x[3] - e)) + (y[1] << (y[3] - e)),
                (x[2] << (x[3] - e)) + (y[2] << (y[3] - e)), e]

    def _sums(self, g: dict[str, Any], key: str) -> list | None:
        """[nums, S, A, e] of ``key`` in group ``g``: its sums with the numeric pairs of its
        histogram folded in ([0, 0, 0, 0] without a number); None when a pair is not finite.
        e only ever falls: 2^e divides every single m that went in, which is what A < 2^53
        speaks about -- a coarser spelling of the same S and A (their common trailing zeros
        shifted out) would hide a product that rounds, so the same content may arrive at
        different e from different paths (a column's scale, a group's own)."""
        out = g["sum"].get(key) or [0, 0, 0, 0]
        for v, c in g["hist"][key].values():
            if c and type_rank(v) == 2:
                me = _scaled(v)
                if me is None:
                    return None
                out = self._merged(out, [c, me[0] * c, abs(me[0]) * c, me[1]])
        return list(out)

    def add_extrema(self, gvals: tuple, key: str, count: int, lo_value: Any = None, hi_value: Any = None) -> None:
        """``count`` rows of the group hold ``key``, their values between ``lo_value`` and
        ``hi_value`` (both among them); nothing when ``count`` is 0."""
        if not count:
            return
        lo, hi = _canon(lo_value), _canon(hi_value)
        ext = self._group(gvals)["ext"]
        e = ext.get(key)
        if e is None:
            ext[key] = [int(count), lo, hi]
            return
        e[0] += int(count)
        if compare(lo, e[1]) < 0:
            e[1] = lo
        if compare(hi, e[2]) > 0:
            e[2] = hi

    def add_rows(self, gvals: tuple, n: int) -> None:
        self._group(gvals)["count"] += int(n)

    def add_value(self, gvals: tuple, key: str, value: Any, n: int) -> None:
        h = self._group(gvals)["hist"][key]
        e = h.get(vkey(value))
        if e is None:
            h[vkey(value)] = [_canon(value), int(n)]
        else:
            e[1] += int(n)

    def add_doc(self, doc: Any) -> None:
        """One document (the path without a column mirror)."""
        gvals = tuple(get_path(doc, p) for p in self.spec.group_by)
        self.add_rows(gvals, 1)
        for k in self.spec.keys:
            v = get_path(doc, k)
            if v is not _MISSING:
                self.add_value(gvals, k, v, 1)

    def add_response(self, res: dict[str, Any]) -> None:
        """A ``project=hist`` or ``project=partial`` answer of another store (a shard)."""
        for g in res["groups"]:
            gvals = tuple(g["group"].get(p, _MISSING) for p in self.spec.group_by)
            self.add_rows(gvals, g["count"])
            for k, pairs in g.get("hist", {}).items():
                for v, c in pairs:
                    self.add_value(gvals, k, v, c)
            for k, e in g.get("ext", {}).items():
                self.add_extrema(gvals, k, *e)
            for k, e in g.get("sum", {}).items():
                self.add_sums(gvals, k, *e)

    def _extrema(self, g: dict[str, Any], key: str) -> list | None:
        """[count, min, max] of ``key`` in group ``g`` from its extrema and its histogram (a key
        held as sums may have both, from different parts); None without a defined value."""
        e = g["ext"].get(key)
        r = reduce_hist(g["hist"][key].values(), ("COUNT", "MIN", "MAX"))
        if not r["COUNT"]:
            return e
        if e is None:
            return [r["COUNT"], r["MIN"], r["MAX"]]
        return [e[0] + r["COUNT"], r["MIN"] if compare(r["MIN"], e[1]) < 0 else e[1],
                r["MAX"] if compare(r["MAX"], e[2]) > 0 else e[2]]

    def _reduce_forms(self, g: dict[str, Any], key: str, ops: list[str]) -> dict[str, Any]:
        """``reduce_hist`` for a key that group ``g`` holds as extrema or sums (and maybe a
        histogram next to them).  ``Inexact`` when the sums do not prove the SUM."""
        out: dict[str, Any] = {}
        x = self._extrema(g, key)
        if "COUNT" in ops:
            out["COUNT"] = x[0] if x else 0
        if x:
            out.update((op, v) for op, v in (("MIN", x[1]), ("MAX", x[2])) if op in ops)
        if key not in g["sum"]:
            out.update(reduce_hist(g["hist"][key].values(), [op for op in ops if op in ("SUM", "AVG")]))
            return out
        t = self._sums(g, key)
        if t is None or t[2] >= 1 << 53:
            raise Inexact(f"sum of magnitudes of {key!r} past 2^53")
        s = math.ldexp(float(t[1]), t[3])
        out.update((op, v) for op, v in (("SUM", s), ("AVG", (s, t[0]))) if op in ops)
        return out

    def _sum_form(self) -> dict[str, dict]:
        """The keys a partial answer carries as sums, each with its folded sums per group (by
        ``id``): a key of ``sum_keys`` that some group holds as sums already, or whose histograms
        have more pairs than ``ColumnarIndex.SUMS_FROM_CELLS`` (a document walk over a
        high-cardinality key) and prove every group's SUM here (magnitudes below 2^53: not 0.1
        next to 1e16, which stays a histogram)."""
        out = {}
        for k in sum_keys(self.spec):
            gs = list(self.groups.values())
            held = any(k in g["sum"] for g in gs)
            if not held and sum(len(g["hist"][k]) for g in gs) <= ColumnarIndex.SUMS_FROM_CELLS:
                continue
            folded = {id(g): self._sums(g, k) for g in gs}
            if held and any(t is None for t in folded.values()):
                raise Inexact(f"a number of {k!r} next to its sums is not finite")
            if all(t is not None and (held or t[2] < 1 << 53) for t in folded.values()):
                out[k] = folded
        return out

    def response(self, hist: bool = False, partial: bool = False) -> dict[str, Any]:
        """The route's answer: groups sorted by their values (``compare``, a missing path
        first); ``hist``: the raw histograms per aggregate key instead of the reduced values;
        ``partial`` (without ``hist``): what another ``AggGroups`` merges (``add_response``)
        at the least size -- ``"ext": {key: [count, min, max]}`` for the keys of
        ``extrema_keys`` (``[0]``: no defined value), ``"sum": {key: [nums, S, A, e]}`` (``[0]``:
        no number; present only when some key is in that form, see ``_sum_form``) with ``"ext"``
        for the COUNT / MIN / MAX asked of the same key, and ``"hist"`` for the others."""
        ext_keys = set() if hist else set(extrema_keys(self.spec))
        sum_form = self._sum_form() if partial and not hist else {}
        sum_ext = {k for k in sum_form if any(op in EXTREMA_OPS for op, kk in self.spec.aggs if kk == k)}
        def cmp(a: dict, b: dict) -> int:
            for x, y in zip(a["values"], b["values"]):
                if x is _MISSING or y is _MISSING:
                    c = (y is _MISSING) - (x is _MISSING)
                else:
                    c = compare(x, y)
                if c:
                    return c
            return 0
        out = []
        for g in sorted(self.groups.values(), key=functools.cmp_to_key(cmp)):
            if not g["count"] and self.spec.group_by:
                continue
            o: dict[str, Any] = {"group": {p: v for p, v in zip(self.spec.group_by, g["values"]) if v is not _MISSING},
                                 "count": g["count"]}
            if hist or partial:
                o["hist"] = {k: sorted(([v, c] for v, c in h.values()),
                                       key=functools.cmp_to_key(lambda a, b: compare(a[0], b[0])))
                             for k, h in g["hist"].items() if k not in ext_keys and k not in sum_form}
                if not hist:
                    o["ext"] = {k: self._extrema(g, k) or [0] for k in self.spec.keys if k in ext_keys or k in sum_ext}
                    if sum_form:
                        o["sum"] = {k: t[id(g)] if t[id(g)][0] else [0] for k, t in sum_form.items()}
            else:
                red = {}
                for k, h in g["hist"].items():
                    ops = [op for op, kk in self.spec.aggs if kk == k]
                    if k in g["ext"] or k in g["sum"]:
                        red[k] = self._reduce_forms(g, k, ops)
                    else:
                        red[k] = reduce_hist(h.values(), ops)
                aggs = []
                for op, k in self.spec.aggs:
                    if k is None:
                        aggs.append({"op": op, "value": g["count"]})
                    elif op in red[k]:
                        v = red[k][op]
                        aggs.append({"op": op, "key": k, "value": v[0] / v[1] if op == "AVG" else v})
                o["aggregates"] = aggs
            out.append(o)
        return {"groups": out}


def rank_interval(c: "Column", sat: np.ndarray) -> tuple[int, int] | None:
    """A range predicate's satisfying dictionary ids as a half-open interval of sort ranks, when
    they are exactly the ids whose rank falls in it (values of one JSON type are contiguous in
    the sort order, so GT/GTE/LT/LTE always are)."""
    if sat.size == 0:
        return None
    ranks = c.ranks()
    if not sat.any():
        return (1, 1)  # empty interval: no row satisfies
    r = ranks[sat]
    lo, hi = int(r.min()), int(r.max()) + 1
    inside = (ranks >= lo) & (ranks < hi)
    if not np.array_equal(inside, sat):
        return None
    return lo, hi


class KeyTable:
    """Row -> document key.  Bulk-loaded keys stay in one UTF-8 blob with offsets (decoded on
    access, so a 10 M-row index holds no 10 M Python strings); appended keys go to a list."""

    def __init__(self, blob: bytes = b"", offsets: np.ndarray | None = None) -> None:
        self.blob = blob
        self.off = offsets if offsets is not None else np.zeros(1, dtype=np.int64)
        self.base = len(self.off) - 1
        self.extra: list[str] = []

    def __len__(self) -> int:
        return self.base + len(self.extra)

    def __getitem__(self, i: int) -> str:
        if i < self.base:
            return self.blob[self.off[i]:self.off[i + 1]].decode()
        return self.extra[i - self.base]

    def append(self, key: str) -> None:
        self.extra.append(key)

    def __iter__(self):
        for i in range(len(self)):
            yield self[i]


_RANK_EPOCHS = itertools.count(1)


_starts_with_quote = operator.methodcaller("startswith", '"')

_NATIVE = []  # [module or None], resolved on first use


def _native_module():
    """The native extension for ``StrRanker`` (None where it cannot load, or with
    ``TT_NATIVE_RANKS=0``: the numpy ranks then answer)."""
    if not _NATIVE:
        mod = None
        if os.environ.get("TT_NATIVE_RANKS", "1") != "0":
            try:
                from ..native import load
                mod = load()
                if not hasattr(mod, "StrRanker"):
                    mod = None
            except Exception:  # no compiler / stale build: the numpy path is complete on its own
                mod = None
        _NATIVE.append(mod)
    return _NATIVE[0]


NOT_A_NUMBER = -1 << 63  # in a table of scaled integers (``Column.nums``): the value is no number


def _quanta(f: np.ndarray) -> np.ndarray:
    """Per finite double the exponent q of its lowest set bit, ``f == odd * 2^q`` (0 for 0.0)."""
    mant, exp = np.frexp(f)
    m53 = np.ldexp(mant, 53).astype(np.int64)  # the 53-bit significand as an integer: exact
    low = (m53 & -m53).astype(np.float64)      # its lowest set bit, a power of two
    return np.where(m53 == 0, 0, exp.astype(np.int64) - 53 + np.frexp(low)[1] - 1)


class Column:
    def __init__(self, path: str) -> None:
        self.path = path
        self._ids: dict[str, int] = {}
        self._ids_n = 0  # values[:_ids_n] are in _ids (bulk-appended strings are keyed lazily)
        self.values: list[Any] = []
        self._num_cache: np.ndarray | None = None
        self._rank_cache: np.ndarray | None = None
        self.rank_version = 0  # bumps whenever a new value may shift the sort ranks
        # which ids' ranks each recomputation changed: (recomputation number, first id whose rank
        # moved); consumers that keep a copy of the ranks (the device sort plan) re-copy only
        # ids >= that bound (the newest ids, for timestamps written roughly in order)
        self.rank_seq = next(_RANK_EPOCHS)
        self._rank_log: list[tuple[int, int]] = []
        self._rank_lo = 0
        # every value a str without a trailing NUL (numpy's fixed-width strings drop those):
        # the ranks are then positions in the sorted dictionary (_string_ranks)
        self.str_only = True
        self._str_sorted = None
        self._nr = None       # native/src/strrank.hpp StrRanker (the string-only ranks)
        self._nr_buf = None   # its rank buffer (int64, capacity-doubled, owned here)
        # the number scale (``num_scale``): values[:_scale_n] are in it; float(v) = m * 2^e with
        # ``_scale_m[id]`` = m as a Python-exact int64 (NOT_A_NUMBER for a value that is no number)
        self._scale_n = 0
        self._scale_e = 0
        self._scale_max = 0          # max |m|
        self._scale_any = False      # the dictionary holds a number
        self._scale_bad = False      # ... one that is not finite, or whose m leaves int64
        self._scale_m = np.zeros(0, dtype=np.int64)  # capacity-doubled
        self.scale_epoch = 0         # bumps when every m changed (e dropped, dictionary replaced)

    @property
    def ids(self) -> dict[str, int]:
        """vkey -> dictionary id.  Strings appended in bulk by ``encode_json_many`` are keyed on
        first use: a column only ordered or range-filtered (timestamps) never pays for it."""
        n = len(self.values)
        if self._ids_n < n:
            self._ids.update(zip([vkey(v) for v in self.values[self._ids_n:]], range(self._ids_n, n)))
            self._ids_n = n
        return self._ids

    @ids.setter
    def ids(self, d: dict[str, int]) -> None:
        self._ids, self._ids_n = d, len(self.values)

    def encode(self, v: Any) -> int:
        if v is _MISSING:
            return -1
        k = vkey(v)
        ids = self.ids
        i = ids.get(k)
        if i is None:
            i = ids[k] = len(self.values)
            self.values.append(v)
            self._ids_n += 1
            if type(v) is not str or v.endswith("\x00"):
                self.str_only = False
            self._num_cache = None
            self._rank_cache = None
            self.rank_version += 1
        return i

    def encode_json_many(self, texts: list[str], all_strings: bool | None = None) -> np.ndarray:
        """Dictionary ids of JSON value texts (the native mirror's new dictionary entries).
        Strings -- timestamps, names, e-mails, the values a growing collection adds on every
        write -- are decoded in one ``json.loads`` and appended in bulk: the native dictionary
        holds each string once (strings compare by value there, as here), so none is already
        here and no per-value ``vkey`` or dictionary probe is needed."""
        if all_strings is None:  # the mirror says; other callers have it checked (a C-level loop)
            all_strings = all(map(_starts_with_quote, texts))
        if texts and all_strings:
            joined = ",".join(texts)
            strs = json.loads("[" + joined + "]")
            base = len(self.values)
            self.values.extend(strs)  # keyed lazily (``ids``)
            if self.str_only and "\\u0000" in joined and any(x.endswith("\x00") for x in strs):
                self.str_only = False
            self._num_cache = None
            self._rank_cache = None
            self.rank_version += 1
            return np.arange(base, base + len(strs), dtype=np.int32)
        return np.fromiter((self.encode(json.loads(t)) for t in texts), dtype=np.int32, count=len(texts))

    def lookup(self, v: Any) -> int:
        return self.ids.get(vkey(v), -2)

    def satisfying(self, op: str, val: Any) -> np.ndarray:
        """Boolean array over the dictionary: which ids satisfy ``<value> op val``."""
        n = len(self.values)
        out = np.zeros(n, dtype=bool)
        if op == "IN":
            for x in val:
                i = self.lookup(x)
                if i >= 0:
                    out[i] = True
            return out
        tv = type_rank(val)
        if tv == 2:  # numeric fast path (vectorised)
            if self._num_cache is None:
                self._num_cache = np.array([float(x) if type_rank(x) == 2 else np.nan for x in self.values],
                                           dtype=np.float64)
            arr = self._num_cache
            with np.errstate(invalid="ignore"):
                res = {"GT": arr > val, "GTE": arr >= val, "LT": arr < val, "LTE": arr <= val}[op]
            return res & ~np.isnan(arr)
        for i, x in enumerate(self.values):
            if type_rank(x) != tv:
                continue
            c = compare(x, val)
            out[i] = {"GT": c > 0, "GTE": c >= 0, "LT": c < 0, "LTE": c <= 0}[op]
        return out

    def num_scale(self, rows: int = 1) -> tuple[int, int] | None:
        """(e, max |m|): the largest power-of-two quantum 2^e, -1074 <= e <= 0, of which every
        number of the dictionary (``type_rank`` 2: int and float, not bool) is an integer
        multiple, ``float(v) == m * 2^e`` -- integers have e = 0, 2.5 makes it -1, 0.1 makes it
        -55 -- and the largest magnitude among the m.  ``m`` is that of ``float(v)``: an int past
        2^53 counts as its double, as ``reduce_hist`` adds it.  None when the dictionary holds no
        number, one that is not finite, or when ``max|m| * max(rows, 1)`` reaches 2^63: ``rows``
        scaled integers could then wrap a 64-bit sum.  Kept incrementally: new dictionary values
        extend the table of m (``nums``), one that lowers e rescales it (``scale_epoch`` bumps)."""
        self._scale_extend()
        if self._scale_bad or not self._scale_any or self._scale_max * max(int(rows), 1) >= 1 << 63:
            return None
        return self._scale_e, self._scale_max

    def nums(self, lo: int, hi: int) -> np.ndarray:
        """The m of ids [lo, hi) at the scale of ``num_scale`` (int64; ``NOT_A_NUMBER`` for a value
        that is no number).  Only while ``num_scale()`` is not None."""
        self._scale_extend()
        return self._scale_m[lo:hi]

    def _scale_extend(self) -> None:
        n = len(self.values)
        if self._scale_n > n:  # the dictionary was replaced
            self._scale_n, self._scale_e, self._scale_max = 0, 0, 0
            self._scale_any = self._scale_bad = False
            self.scale_epoch += 1
        if self._scale_n == n:
            return
        lo, self._scale_n = self._scale_n, n
        if self._scale_bad:
            return
        new = self.values[lo:n]
        isnum = np.fromiter((type_rank(v) == 2 for v in new), dtype=bool, count=len(new))
        if self._scale_m.size < n:
            grown = np.empty(max(1024, 2 * n), dtype=np.int64)
            grown[:lo] = self._scale_m[:lo]
            self._scale_m = grown
        self._scale_m[lo:n] = NOT_A_NUMBER
        if not isnum.any():
            return
        try:
            f = np.array([float(v) for v, k in zip(new, isnum) if k], dtype=np.float64)
        except OverflowError:  # an int past the doubles
            f = np.array([np.inf])
        if not np.isfinite(f).all():
            self._scale_bad, self._scale_m = True, np.zeros(0, dtype=np.int64)
            return
        e = min(self._scale_e, int(_quanta(f).min()))
        if e < self._scale_e:  # every m so far is rescaled to the finer quantum
            shift = self._scale_e - e
            self._scale_max <<= shift
            if 0 < self._scale_max < 1 << 63:  # (all zeros: nothing to shift)
                old = self._scale_m[:lo]
                np.left_shift(old, shift, out=old, where=old != NOT_A_NUMBER)
            self._scale_e = e
            self.scale_epoch += 1
        with np.errstate(over="ignore"):
            m = np.ldexp(f, -e)  # integers: exact unless past the doubles (inf)
        self._scale_max = max(self._scale_max, int(np.abs(m).max()) if np.isfinite(m).all() else 1 << 63)
        if self._scale_max >= 1 << 63:
            self._scale_bad, self._scale_m = True, np.zeros(0, dtype=np.int64)
            return
        self._scale_any = True
        self._scale_m[lo:n][isnum] = m.astype(np.int64)

    def missing_rank(self) -> int:
        """A missing path sorts like JSON null (the native engine compares it as null)."""
        if self.str_only:
            return 0  # no null in a string-only dictionary (and no need to key it)
        i = self.ids.get("n")
        return int(self.ranks()[i]) if i is not None else 0

    def ranks(self) -> np.ndarray:
        """Sort rank of every dictionary id (ties share a rank, ranks start at 1)."""
        if self._rank_cache is None:
            self._rank_lo = 0
            self._rank_cache = self._string_ranks() if self._all_strings() else self._general_ranks()
            self.rank_seq = next(_RANK_EPOCHS)
            self._rank_log.append((self.rank_seq, self._rank_lo))
            if len(self._rank_log) > 64:
                del self._rank_log[0]
        return self._rank_cache

    def rank_changes_since(self, seq: int) -> int | None:
        """The first id whose rank may differ from the ranks of recomputation ``seq`` (the
        dictionary size when none moved); None when ``seq`` is too old to tell."""
        self.ranks()
        if seq == self.rank_seq:
            return len(self.values)
        if not any(s == seq for s, _ in self._rank_log):
            return None
        return min([lo for s, lo in self._rank_log if s > seq] or [len(self.values)])

    def _all_strings(self) -> bool:
        if not self.str_only:
            self._str_sorted = None
            self._nr = self._nr_buf = None
        return self.str_only

    def _string_ranks(self) -> np.ndarray:
        r = self._string_ranks_native()
        return r if r is not None else self._string_ranks_numpy()

    def _string_ranks_native(self) -> np.ndarray | None:
        """``_string_ranks`` in C++ (``native/src/strrank.hpp``): the new values are read from
        the dictionary list as UTF-8 (no numpy string array), sorted alone and merged into the
        tail of the order; the ranks land in a buffer owned here, so earlier views stay valid.
        None without the native module (the numpy path then answers)."""
        mod = _native_module()
        if mod is None:
            return None
        n = len(self.values)
        nr = self._nr
        if nr is None or nr.size > n:  # first use, or the dictionary was replaced
            nr, self._nr_buf = mod.StrRanker(), None
        buf = self._nr_buf
        if buf is None or buf.size < n:
            grown = np.empty(max(1024, 2 * n), dtype=np.int64)
            if buf is not None:
                grown[:nr.size] = buf[:nr.size]
            buf = grown
        try:
            lo = nr.extend(self.values, buf)
        except (TypeError, ValueError):  # not a list of values as expected: the numpy path
            lo = -1
        if lo < 0:  # a value UTF-8 cannot carry (a lone surrogate): the numpy path orders it
            self._nr = self._nr_buf = None
            return None
        self._nr, self._nr_buf = nr, buf
        self._rank_lo = int(lo)
        return buf[:n]

    def _string_ranks_numpy(self) -> np.ndarray:
        """A dictionary of strings only (timestamps, e-mails, names): distinct values never tie
        and Python's string order is ``compare``'s, so the ranks are positions in the sorted
        dictionary.  Kept incrementally: values appended since the last call are sorted alone
        and merged in (``searchsorted`` + ``insert``), an O(dictionary) vector pass instead of a
        comparison sort of the whole dictionary per new value -- the overdue sweep orders by
        ``taskCreatedOn``, whose dictionary grows with every created task.  When every new value
        sorts after the old ones (timestamps of new writes) the sorted copy and the ranks grow
        in place, in capacity-doubling buffers: O(new values), not O(dictionary)."""
        n = len(self.values)
        prev = self._str_sorted
        if prev is None or prev[1] > n:
            arr = np.array(self.values, dtype=str) if n else np.zeros(0, dtype="<U1")
            order = np.argsort(arr, kind="stable")
            r = np.empty(n, dtype=np.int64)
            r[order] = np.arange(1, n + 1)
            self._str_sorted = (arr[order], n, r, order.astype(np.int64))
            self._rank_lo = 0
            return r[:n]
        srt, m, old_r, ids = prev  # sorted values, count, rank per id, id per sorted position
        if m == n:
            self._rank_lo = n
            return old_r[:n]
        new = np.array(self.values[m:], dtype=str)
        k = new.size
        if k < 2 or bool(np.all(new[1:] >= new[:-1])):  # written in order (timestamps): no sort
            norder = np.arange(k, dtype=np.int64)
            new_sorted = new
        else:
            norder = np.argsort(new, kind="stable")
            new_sorted = new[norder]
        # insertion point of the smallest new value: only the old values from there on move
        pos0 = m if m == 0 or new_sorted[0] > srt[m - 1] else int(np.searchsorted(srt[:m], new_sorted[0]))
        if new_sorted.dtype.itemsize <= srt.dtype.itemsize and m - pos0 <= 4 * k + 65536:
            # new values land in (or just before) the tail of the order -- new timestamps,
            # written a little out of order by concurrent writers: re-sort only that tail with
            # them, in capacity-doubling buffers; O(tail + new), not O(dictionary)
            if srt.size < n:  # grow the buffers (doubling): amortised O(1) per appended value
                cap = max(n, 2 * srt.size, 1024)
                srt2 = np.empty(cap, dtype=srt.dtype)
                srt2[:m] = srt[:m]
                r2 = np.empty(cap, dtype=np.int64)
                r2[:m] = old_r[:m]
                i2 = np.empty(cap, dtype=np.int64)
                i2[:m] = ids[:m]
                srt, old_r, ids = srt2, r2, i2
            tail_ids = ids[pos0:m].copy()
            if pos0 == m:
                srt[m:n] = new_sorted
                ids[m:n] = m + norder
            else:
                # merge two sorted runs (the old tail, the new values) without a comparison
                # sort: each new value lands after the old ones equal to it (a stable sort of
                # old-then-new would do the same)
                tail = srt[pos0:m].copy()
                ins = np.searchsorted(tail, new_sorted, side="right")
                at_new = ins + np.arange(k)                                  # merged positions of new values
                at_old = np.arange(tail.size) + np.searchsorted(ins, np.arange(tail.size), side="right")
                seg_v = np.empty(tail.size + k, dtype=srt.dtype)
                seg_i = np.empty(tail.size + k, dtype=np.int64)
                seg_v[at_old], seg_v[at_new] = tail, new_sorted
                seg_i[at_old], seg_i[at_new] = tail_ids, m + norder
                srt[pos0:n] = seg_v
                ids[pos0:n] = seg_i
            old_r[ids[pos0:n]] = np.arange(pos0 + 1, n + 1)
            self._str_sorted = (srt, n, old_r, ids)
            self._rank_lo = int(min(int(tail_ids.min()), m)) if tail_ids.size else m
            return old_r[:n]
        srt = srt[:m]
        old_r = old_r[:m]
        ids = ids[:m]
        width = max(srt.dtype.itemsize, new.dtype.itemsize) // 4
        srt = srt.astype(f"<U{max(width, 1)}", copy=False)
        new_sorted = new_sorted.astype(srt.dtype, copy=False)
        pos = np.searchsorted(srt, new_sorted)            # insertion points in the old order
        before = np.searchsorted(pos, old_r - 1, side="right")  # new values ahead of each old one
        r = np.empty(n, dtype=np.int64)
        r[:m] = old_r + before
        r[m + norder] = pos + np.arange(new.size) + 1
        # the old values at or after the first insertion point moved up: the first id among
        # them bounds what changed (new timestamps arriving a little out of order: recent ids)
        moved = ids[int(pos[0]):]
        self._rank_lo = int(min(int(moved.min()), m)) if moved.size else m
        self._str_sorted = (np.insert(srt, pos, new_sorted), n, r, np.insert(ids, pos, m + norder))
        return r

    def _general_ranks(self) -> np.ndarray:
        order = sorted(range(len(self.values)), key=functools.cmp_to_key(lambda a, b: compare(self.values[a], self.values[b])))
        r = np.empty(len(order), dtype=np.int64)
        rank = 0
        for pos, i in enumerate(order):
            if pos and compare(self.values[order[pos - 1]], self.values[i]) != 0:
                rank += 1
            r[i] = rank + 1  # 0 reserved for missing (sorts like null, first)
        return r


@dataclass
class Program:
    code: np.ndarray      # [L, 4] int32
    bitmaps: np.ndarray   # int32 words (uint32 bit patterns)
    columns: list[int]
    # its device copy, kept by DeviceMirror.program: ((rank slots, device), code, bitmaps)
    device: Any = field(default=None, compare=False, repr=False)


class SortField(NamedTuple):
    """One sort key's field of the packed ordering key [rank(key0) | ... | seq]."""
    col: int
    ranks: np.ndarray   # dictionary id -> sort rank (int64)
    missing: int        # rank of a missing path (it sorts like null)
    max_rank: int       # a DESC key stores max_rank - rank
    bits: int
    desc: int


class ColumnarIndex:
    width_for = staticmethod(width_for)
    col_bytes = staticmethod(col_bytes)


    def __init__(self, paths: Iterable[str] = (), capacity: int = TILE) -> None:
        self.columns: list[Column] = []
        self.col_of: dict[str, int] = {}
        self.cap = max(TILE, (capacity + TILE - 1) // TILE * TILE)
        self.ids = np.full((0, self.cap), -1, dtype=np.int32)
        self.live = np.zeros(self.cap, dtype=np.int32)
        self.seq = np.zeros(self.cap, dtype=np.int64)
        self._next_seq = 0
        self.keys: KeyTable | list[str] = []
        self._row_of: dict[str, int] | None = {}
        self.docs: list[Any] | None = []  # None when columns come from `source` (bulk-encoded)
        self.source = None  # callable(paths) -> (keys, seqs, [(values_json, ids)]) for re-encoding
        self.native = None  # DocStore whose column mirror feeds this index (from_native)
        self._dead = 0      # tombstoned rows since the last compaction (upsert/delete path)
        self.n = 0
        self.version = 0
        # compiled programs, keyed by the filter and the dictionaries' state (append-only
        # dictionaries: sizes + rank versions identify their contents)
        self._prog_cache: dict[Any, Program] = {}
        self._dict_gen = 0  # bumps when the dictionaries are rebuilt (re-encode from `source`)
        self._host: dict | None = None  # the CPU scan's copies in the device layout (_host_mirror)
        self._ncur = (0, 0, 0)  # native mirror cursor: (generation, rows seen, kill-log position)
        # per column: native dictionary id -> this index's id, in a capacity-doubled buffer
        # (``_remap_n`` entries used): a sync appends the new values' ids in place instead of
        # copying the whole map (taskCreatedOn's grows by one per write)
        self._remap: list[np.ndarray] = []
        self._remap_n: list[int] = []
        self.mirror = DeviceMirror(self)  # the GPU side: told what changes, synced by the queries
        for p in paths:
            self.add_column(p)

    # -- bulk load ------------------------------------------------------------
    @classmethod
    def from_source(cls, source, paths: Iterable[str]) -> "ColumnarIndex":
        """Index built from a native bulk encoder (``DocStore.encode_columns``): no per-document
        Python objects are kept; a column added later re-encodes from ``source``."""
        ix = cls()
        ix.source = source
        ix.docs = None
        ix._load(list(dict.fromkeys(paths)))
        return ix

    def _load(self, paths: list[str]) -> None:
        keys, seqs, cols = self.source(paths)
        n = len(seqs)
        cap = max(TILE, (n + TILE - 1) // TILE * TILE)
        self.cap = cap
        self.columns, self.col_of = [], {}
        self._dict_gen += 1
        self.ids = np.full((len(paths), cap), -1, dtype=np.int32)
        for i, (path, (values, ids)) in enumerate(zip(paths, cols)):
            c = Column(path)
            remap = np.empty(len(values), dtype=np.int32)
            for j, text in enumerate(values):  # dictionary built by Python's own equality (vkey)
                remap[j] = c.encode(json.loads(text))
            ids = np.asarray(ids, dtype=np.int32)
            self.ids[i, :n] = gather(remap, ids, -1)
            self.columns.append(c)
            self.col_of[path] = i
        self.live = np.zeros(cap, dtype=np.int32)
        self.live[:n] = 1
        self.seq = np.zeros(cap, dtype=np.int64)
        self.seq[:n] = seqs
        self._next_seq = int(seqs.max()) if n else 0
        if isinstance(keys, tuple):  # (blob, offsets) from DocStore.encode_columns
            self.keys = KeyTable(keys[0], np.asarray(keys[1], dtype=np.int64))
        else:
            self.keys = list(keys)
        self._row_of = None  # built on the first write (read-only use never needs it)
        self.n = n
        self.version += 1
        self.mirror.invalidate()
        self.mirror.reset_zones()

    # -- native mirror (DocStore column mirror, native/src/docstore.hpp) ---------------
    @classmethod
    def from_native(cls, store, paths: Iterable[str]) -> "ColumnarIndex":
        """Index fed by the document store's own column mirror: the store appends a row per
        write in C++ (the native HTTP front never hands writes to Python), and ``sync`` pulls
        only what changed since the last sync (new rows, new dictionary values, killed rows).
        Rows map back to documents through ``store.mirror_results``."""
        ix = cls()
        ix.native = store
        ix.docs = None
        if not store.mirror_enable(list(dict.fromkeys(paths))):
            raise Unsupported("collection cannot be mirrored (TTL writes)")
        ix.sync()
        return ix

    def sync(self) -> bool:
        """Apply the native mirror's changes; returns True when anything changed."""
        gen, rows, kc = self._ncur
        d = self.native.mirror_delta(gen, rows, kc, list(self._remap_n))
        if d["disabled"] or not d["on"]:
            raise Unsupported("collection mirror disabled (TTL writes)")
        lo, hi = int(d["from"]), int(d["n"])
        changed = d["full"] or hi > lo or d["kills"].size > 0
        if d["full"]:
            self.columns, self.col_of, self._remap, self._remap_n = [], {}, [], []
            for path, *_ in d["columns"]:
                self.col_of[path] = len(self.columns)
                self.columns.append(Column(path))
                self._remap.append(np.zeros(0, dtype=np.int32))
                self._remap_n.append(0)
            self.cap = max(TILE, (hi + TILE - 1) // TILE * TILE)
            self.ids = np.full((len(self.columns), self.cap), -1, dtype=np.int32)
            self.live = np.zeros(self.cap, dtype=np.int32)
            self.seq = np.zeros(self.cap, dtype=np.int64)
            self.n, self._next_seq = 0, 0
            self._dict_gen += 1
            self.mirror.invalidate()
            self.keys = []
        assert lo == self.n, (lo, self.n)
        self._grow(hi)
        for c, (path, dict_from, values, ids, all_str) in enumerate(d["columns"]):
            col = self.columns[c]
            if values:  # new dictionary values, mapped onto Python's equality (vkey)
                add = col.encode_json_many(values, all_str)
                need = dict_from + add.size
                buf = self._remap[c]
                if buf.size < need:
                    grown = np.empty(max(need, 2 * buf.size, 1024), dtype=np.int32)
                    grown[:dict_from] = buf[:dict_from]
                    buf = self._remap[c] = grown
                buf[dict_from:need] = add
                self._remap_n[c] = need
            rm = self._remap[c][:self._remap_n[c]]
            if hi > lo:
                self.ids[c, lo:hi] = gather(rm, ids, -1)
        if hi > lo:
            self.seq[lo:hi] = d["seqs"]
            self.live[lo:hi] = d["live"]
            self._next_seq = max(self._next_seq, int(d["seqs"].max()))
            self.mirror.touch(np.arange(lo // TILE, (hi - 1) // TILE + 1))
        if d["kills"].size:
            self.live[d["kills"].astype(np.int64)] = 0
            self.mirror.tombstoned()
            self.mirror.touch(np.unique(d["kills"].astype(np.int64) // TILE))
        if d["full"]:
            self.mirror.reset_zones()
        self.n = hi
        self._ncur = (int(d["gen"]), hi, int(d["kill_cursor"]))
        if changed:
            self.version += 1
        return bool(changed)

    @property
    def generation(self) -> int:
        """Mirror generation the row numbers belong to (``DocStore.mirror_results`` checks it)."""
        return int(self._ncur[0]) if self.native is not None else 0

    @property
    def row_of(self) -> dict[str, int]:
        if self._row_of is None:
            self._row_of = {self.keys[r]: r for r in np.nonzero(self.live[:self.n])[0].tolist()}
        return self._row_of

    def ensure_columns(self, paths: Iterable[str]) -> None:
        """Add every missing column at once (one re-encode for a source-backed index)."""
        missing = [p for p in dict.fromkeys(paths) if p not in self.col_of]
        if not missing:
            return
        if self.native is not None:
            if not self.native.mirror_enable([c.path for c in self.columns] + missing):
                raise Unsupported("collection mirror disabled (TTL writes)")
            self.sync()  # a new column is a new mirror generation: full reload
        elif self.docs is None:
            self._load([c.path for c in self.columns] + missing)
        else:
            for p in missing:
                self.add_column(p)

    # -- maintenance ----------------------------------------------------------
    def add_column(self, path: str) -> int:
        if path in self.col_of:
            return self.col_of[path]
        if self.docs is None:
            self.ensure_columns([path])
            return self.col_of[path]
        c = Column(path)
        idx = len(self.columns)
        self.columns.append(c)
        self.col_of[path] = idx
        col = np.full((1, self.cap), -1, dtype=np.int32)
        for r in range(self.n):
            if self.live[r]:
                col[0, r] = c.encode(get_path(self.docs[r], path))
        self.ids = np.concatenate([self.ids, col], axis=0)
        self.version += 1
        self.mirror.invalidate()
        return idx

    def _grow(self, need: int) -> None:
        if need <= self.cap:
            return
        cap = self.cap
        while cap < need:
            cap *= 2
        ids = np.full((len(self.columns), cap), -1, dtype=np.int32)
        ids[:, :self.n] = self.ids[:, :self.n]
        live = np.zeros(cap, dtype=np.int32)
        live[:self.n] = self.live[:self.n]
        seq = np.zeros(cap, dtype=np.int64)
        seq[:self.n] = self.seq[:self.n]
        self.ids, self.live, self.seq, self.cap = ids, live, seq, cap
        self.mirror.invalidate()

    def upsert(self, key: str, doc: Any) -> None:
        old = self.row_of.get(key)
        if old is not None:
            self.live[old] = 0
            if self.docs is not None:
                self.docs[old] = None
            self.mirror.tombstoned()
            self._dead += 1
            seq = int(self.seq[old])  # an update keeps the key's original position (native engine semantics)
        else:
            self._next_seq += 1
            seq = self._next_seq
        self._grow(self.n + 1)
        r = self.n
        self.seq[r] = seq
        for i, c in enumerate(self.columns):
            self.ids[i, r] = c.encode(get_path(doc, c.path))
        self.live[r] = 1
        self.keys.append(key)
        if self.docs is not None:
            self.docs.append(doc)
        self.row_of[key] = r
        self.n += 1
        self.version += 1
        self.mirror.touch([r // TILE] if old is None else [r // TILE, old // TILE])
        self._maybe_compact()

    def delete(self, key: str) -> None:
        r = self.row_of.pop(key, None)
        if r is not None:
            self.live[r] = 0
            if self.docs is not None:
                self.docs[r] = None
            self.mirror.tombstoned()
            self._dead += 1
            self.version += 1
            self.mirror.touch([r // TILE])
        self._maybe_compact()

    def _maybe_compact(self) -> None:
        """Keep the index proportional to the live documents, not to the number of writes."""
        if self._dead > TILE and self._dead * 2 > self.n:
            self.compact()

    def bulk_load(self, items: Iterable[tuple[str, Any]]) -> None:
        for k, d in items:
            self.upsert(k, d)

    def live_rows(self) -> int:
        return int(np.count_nonzero(self.live[:self.n]))

    def compact(self) -> None:
        """Drop tombstones (rows are renumbered in order)."""
        keep = np.nonzero(self.live[:self.n])[0]
        self.ids[:, :len(keep)] = self.ids[:, keep]
        self.ids[:, len(keep):] = -1
        self.seq[:len(keep)] = self.seq[keep]
        self.live[:] = 0
        self.live[:len(keep)] = 1
        self.keys = [self.keys[i] for i in keep.tolist()]
        if self.docs is not None:
            self.docs = [self.docs[i] for i in keep]
        self._row_of = {k: i for i, k in enumerate(self.keys)}
        self.n = len(keep)
        self._dead = 0
        self.version += 1
        self.mirror.invalidate()
        self.mirror.reset_zones()

    # -- compilation ---------------------------------------------------------
    def _dict_state(self) -> tuple:
        return (self._dict_gen,) + tuple((len(c.values), c.rank_version) for c in self.columns)

    def compile_cached(self, flt: Any) -> Program:
        """``compile`` memoised per filter and the dictionary state of the columns it reads
        (queries repeat: the cron sweep, the same creator's list page) -- not of every column:
        the sort key's dictionary (``taskCreatedOn``, one value per write) grows between any two
        sweeps and would otherwise recompile, and re-upload, the same program every time.
        Bounded, oldest entries dropped."""
        fj = json.dumps(flt, sort_keys=True, default=str)
        cols = [self.col_of.get(p) for p in filter_paths(flt)]
        if any(c is None for c in cols):  # compile adds the column: key on everything this once
            state = self._dict_state()
        else:
            state = (self._dict_gen,) + tuple((c, len(self.columns[c].values), self.columns[c].rank_version)
                                              for c in sorted(set(cols)))
        key = (fj, state)
        prog = self._prog_cache.get(key)
        if prog is None:
            prog = self.compile(flt)
            if len(self._prog_cache) >= 128:
                self._prog_cache.pop(next(iter(self._prog_cache)))
            self._prog_cache[key] = prog
        return prog

    def compile(self, flt: Any) -> Program:
        code: list[list[int]] = []
        words: list[np.ndarray] = []
        nwords = [0]
        used: list[int] = []
        depth = [0, 0]

        def push() -> None:
            depth[0] += 1
            depth[1] = max(depth[1], depth[0])

        def leaf_bitmap(col: int, sat: np.ndarray) -> None:
            nbits = len(sat)
            padded = np.zeros(((nbits + 31) // 32) * 32, dtype=bool)
            padded[:nbits] = sat
            w = np.packbits(padded, bitorder="little").view("<u4").astype(np.uint32)
            if w.size == 0:
                w = np.zeros(1, dtype=np.uint32)
            code.append([OP_LEAF, col, nwords[0], nbits])
            words.append(w)
            nwords[0] += w.size
            push()

        def emit(f: Any) -> None:
            if not isinstance(f, dict) or len(f) != 1:
                raise Unsupported("filter node must be a single-operator object")
            (op, arg), = f.items()
            op = op.upper()
            if op in ("AND", "OR"):
                if not isinstance(arg, list) or not arg:
                    raise Unsupported(f"{op} expects a non-empty array")
                for x in arg:
                    emit(x)
                n = len(arg)
                if n > 1:
                    code.append([OP_AND if op == "AND" else OP_OR, n, 0, 0])
                    depth[0] -= n - 1
                return
            if not isinstance(arg, dict) or len(arg) != 1:
                raise Unsupported(f"{op} expects {{path: value}}")
            (path, val), = arg.items()
            col = self.col_of.get(path)
            if col is None:
                col = self.add_column(path)
            used.append(col)
            c = self.columns[col]
            if op in ("EQ", "NEQ"):
                if isinstance(val, (list, dict)):
                    raise Unsupported("structured equality")
                code.append([OP_EQ, col, c.lookup(val), 0])
                push()
                if op == "NEQ":
                    code.append([OP_NOT, 0, 0, 0])
            elif op == "IN":
                if not isinstance(val, list):
                    raise Unsupported("IN expects a list")
                leaf_bitmap(col, c.satisfying("IN", val))
            elif op in ("GT", "GTE", "LT", "LTE"):
                sat = c.satisfying(op, val)
                rng = rank_interval(c, sat)
                if rng is None:
                    leaf_bitmap(col, sat)
                else:  # one integer compare per row on the rank-encoded column
                    code.append([OP_RANGE, col, rng[0], rng[1]])
                    push()
            else:
                raise Unsupported(f"operator {op}")

        if not flt:
            code.append([OP_TRUE, 0, 0, 0])
            push()
        else:
            emit(flt)
        if depth[1] > MAX_DEPTH:
            raise Unsupported("filter nesting too deep for the device stack")
        bitmaps = np.concatenate(words) if words else np.zeros(1, dtype=np.uint32)
        return Program(np.asarray(code, dtype=np.int32), bitmaps.view(np.int32), sorted(set(used)))

    # -- execution -------------------------------------------------------------
    def select_numpy(self, prog: Program) -> np.ndarray:
        """Reference executor: identical semantics to the HIP kernel."""
        n = self.n
        stack: list[np.ndarray] = []
        bm = prog.bitmaps.view(np.uint32)
        for op, a, b, c in prog.code.tolist():
            if op == OP_EQ:
                stack.append(self.ids[a, :n] == b)
            elif op == OP_RANGE:
                r = gather(self.columns[a].ranks(), self.ids[a, :n], -1)
                stack.append((r >= b) & (r < c))
            elif op == OP_LEAF:
                v = self.ids[a, :n]
                ok = (v >= 0) & (v < c)
                vv = np.where(ok, v, 0)
                bits = (bm[b + (vv >> 5)] >> (vv & 31).astype(np.uint32)) & 1
                stack.append(ok & (bits == 1))
            elif op in (OP_AND, OP_OR):
                xs = stack[-a:]
                del stack[-a:]
                r = xs[0].copy()
                for x in xs[1:]:
                    r = (r & x) if op == OP_AND else (r | x)
                stack.append(r)
            elif op == OP_NOT:
                stack[-1] = ~stack[-1]
            else:
                stack.append(np.ones(n, dtype=bool))
        sel = stack[-1] & (self.live[:n] != 0)
        return np.nonzero(sel)[0].astype(np.int32)

    def select_native(self, prog: Program, threads: int | None = None, simd: bool = True) -> np.ndarray:
        """The program on the host's CPU share (``native/src/cpuscan.hpp``): every core, SIMD
        compares, over the same narrow codes / rank copies / liveness bits the GPU kernels read
        -- the fair CPU baseline for ``select_gpu`` and the executor without a GPU.  Same result
        as ``select_numpy`` (the reference)."""
        from ..native import load
        hm = self._host_mirror(prog)
        code = prog.code
        rng = code[:, 0] == OP_RANGE
        if rng.any():  # range leaves read the rank-encoded copy of their column
            code = code.copy()
            code[rng, 1] = [hm["rank_slot"][c] for c in prog.code[rng, 1].tolist()]
        return load().scan_select(hm["cols"], hm["live"], self.n, np.ascontiguousarray(code, dtype=np.int32),
                                  prog.bitmaps.view(np.uint32), threads or cpu_share(), simd)

    def _host_mirror(self, prog: Program) -> dict:
        """Host copies of the columns in the device layout (narrow codes, rank-encoded copies for
        the program's range leaves, 1-bit liveness), rebuilt when the index changed."""
        key = (self.version, self.n, self.cap, self._dict_state())
        hm = self._host
        if hm is None or hm["key"] != key:
            widths = [width_for(len(c.values)) for c in self.columns]
            hm = self._host = {"key": key, "widths": widths, "ranks": {},
                               "cols": [(np.ascontiguousarray(self.codes(i, 0, self.cap, w)).view(np.uint8), w)
                                        for i, w in enumerate(widths)],
                               "live": np.ascontiguousarray(self.live_words(0, self.cap // 16)).view(np.uint16)}
        rank_cols = sorted(set(prog.code[prog.code[:, 0] == OP_RANGE, 1].tolist()))
        slots = {}
        cols = list(hm["cols"][:len(self.columns)])
        for col in rank_cols:
            r = hm["ranks"].get(col)
            if r is None:
                w = max(1, hm["widths"][col])
                rk = encode_codes(gather(self.columns[col].ranks(), self.ids[col, :self.cap], -1), w)
                r = hm["ranks"][col] = (np.ascontiguousarray(rk).view(np.uint8), w)
            slots[col] = len(cols)
            cols.append(r)
        return {"cols": cols, "live": hm["live"], "rank_slot": slots}

    def codes(self, col: int, lo: int, hi: int, width: int) -> np.ndarray:
        """Codes of rows [lo, hi) of a column in the device layout (width 0: ``lo``/``hi``
        multiples of 4)."""
        return encode_codes(self.ids[col, lo:hi], width)

    def live_words(self, lo_word: int, hi_word: int) -> np.ndarray:
        """Liveness of rows [16 lo_word, 16 hi_word), one bit per row."""
        bits = self.live[lo_word * 16:hi_word * 16].astype(np.uint8)
        return np.packbits(bits, bitorder="little").view("<u2").view(np.int16)

    # -- on the GPU (device_mirror.py keeps the device side) ---------------------------------
    def select_gpu(self, prog: Program, kernels, return_mask: bool = False, on_device: bool = False):
        res = self.mirror.select(prog, kernels, return_mask)
        if return_mask or on_device:
            return res
        return res.cpu().numpy()

    def group_count_gpu(self, prog: Program, group_path: str, kernels) -> dict[str, int]:
        g = self.add_column(group_path)
        _, mask = self.select_gpu(prog, kernels, return_mask=True)
        col = self.columns[g]
        if mask is None or not col.values:
            return {}
        counts = kernels.group_count(self.mirror.table, g, mask, self.n, len(col.values)).cpu().numpy()
        return {json.dumps(col.values[i]): int(x) for i, x in enumerate(counts) if x}

    def group_count_numpy(self, prog: Program, group_path: str) -> dict[str, int]:
        g = self.add_column(group_path)
        rows = self.select_numpy(prog)
        col = self.columns[g]
        ids = self.ids[g, rows]
        ids = ids[ids >= 0]
        cnt = np.bincount(ids, minlength=len(col.values))
        return {json.dumps(col.values[i]): int(x) for i, x in enumerate(cnt) if x}

    # Histogram cells the host path counts with ``np.bincount``; sparser key spaces go through
    # ``np.unique`` (no array of all cells).  The device's own cap is ``tt_group_max_cells()``.
    HOST_MAX_CELLS = 1 << 22

    # An aggregate key of which only COUNT / MIN / MAX are asked leaves the histogram for the
    # per-group extrema (``hip/group_extrema.hip``, ``extrema_numpy``) when its histogram would
    # have more cells than this; with kernels, than the smaller of this and the device's cap.
    EXTREMA_FROM_CELLS = 1 << 22

    # An aggregate key that is asked a SUM or an AVG leaves the histogram for exact scaled-integer
    # sums per group (``hip/group_sums.hip``, ``sums_numpy``) when its histogram would have more
    # cells than this and its numbers share a scale (``Column.num_scale``).  Compared alone, not
    # with the device's cap (in production the two are equal).
    SUMS_FROM_CELLS = 1 << 22

    # A histogram, extrema or sums request whose dense cells are past the device's cap
    # (``tt_group_max_cells()``: a product of dictionary sizes, passed long before the groups that
    # occur are many) keeps its cells in a hash table on the device instead
    # (``hip/sparse_cells.h``; ``GpuKernels.scan_sparse`` / ``scan_extrema_sparse`` /
    # ``scan_sums_sparse``), from this many rows on: below it the host selection answers as before.
    # The measured crossover (profiles/group_sparse.md): the hashed scan's fixed cost -- filling the
    # table, reading its status, compacting it -- loses to ``select_native`` + ``np.unique`` at
    # 20,000 to 40,000 rows, is level with it at 50,000 and wins from 70,000 on at every
    # selectivity and grouping measured.  Never below 20,000, ``TT_QUERY_ACCEL_MIN_DOCS``'s default:
    # below that production does not use the accelerator at all.
    SPARSE_FROM_ROWS = 50_000
    # The table takes the next power of two of slots >= 2 x min(cells, rows) -- load <= 0.5, it
    # cannot overflow -- up to this many: a memory choice (12 bytes per slot with counts, 768 MiB;
    # 28 bytes with value words, 1.75 GiB).  Capped, it can overflow: the kernels then say so and
    # the host answers that request.
    SPARSE_MAX_SLOTS = 1 << 26

    def cells_of(self, rows: np.ndarray, cols: list[int], dims: list[int]) -> np.ndarray:
        """The cell of each of ``rows`` over the key columns ``cols``: axis i has ``dims[i] + 1``
        slots, slot ``dims[i]`` = path missing (the rule of group_cells, ``hip/scan_cells.h``)."""
        cell = np.zeros(rows.size, dtype=np.int64)
        for c, d in zip(cols, dims):
            ids = self.ids[c, rows]
            cell = cell * (d + 1) + np.where(ids < 0, d, ids)
        return cell

    def sums_numpy(self, rows: np.ndarray, gcols: list[int], gdims: list[int],
                   kc: int) -> tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
        """Host twin of ``hip/group_sums.hip`` over the selected ``rows``: (cells with a number
        in column ``kc``, how many rows hold one, the sum of their scaled integers m as int64, the
        sum of |m| as uint64), cells by ``cells_of``.  Integer adds only (``reduceat``): exact in any order."""
        col = self.columns[kc]
        ids = self.ids[kc, rows]
        rows, ids = rows[ids >= 0], ids[ids >= 0]
        m = col.nums(0, len(col.values))[ids] if ids.size else np.zeros(0, dtype=np.int64)
        rows, m = rows[m != NOT_A_NUMBER], m[m != NOT_A_NUMBER]
        cell = self.cells_of(rows, gcols, gdims)
        if not cell.size:
            return cell, cell, m, m.astype(np.uint64)
        order = np.argsort(cell, kind="stable")
        cell, m = cell[order], m[order]
        starts = np.flatnonzero(np.concatenate([[True], cell[1:] != cell[:-1]]))
        ends = np.concatenate([starts[1:], [cell.size]])
        return (cell[starts], ends - starts, np.add.reduceat(m, starts),
                np.add.reduceat(np.abs(m).astype(np.uint64), starts))

    def _dict_size(self, col: int) -> int:
        """The dictionary size of a column as the aggregate planner sees it."""
        return len(self.columns[col].values)

    def extrema_numpy(self, rows: np.ndarray, gcols: list[int], gdims: list[int],
                      kc: int) -> tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
        """Host twin of ``hip/group_extrema.hip`` over the selected ``rows``: (cells with a
        defined value of column ``kc``, their row counts, smallest and largest ``rank << 32 |
        row``), cells by ``cells_of`` over the group columns."""
        ids = self.ids[kc, rows]
        rows, ids = rows[ids >= 0], ids[ids >= 0]
        cell = self.cells_of(rows, gcols, gdims)
        ranks = self.columns[kc].ranks()[ids] if ids.size else np.zeros(0, dtype=np.int64)
        key = (ranks.astype(np.uint64) << np.uint64(32)) | rows.astype(np.uint64)
        order = np.lexsort((key, cell))  # by cell, then by key: a cell's extrema at its ends
        cell, key = cell[order], key[order]
        if not cell.size:
            return cell, cell, key, key
        starts = np.flatnonzero(np.concatenate([[True], cell[1:] != cell[:-1]]))
        ends = np.concatenate([starts[1:], [cell.size]])
        return cell[starts], ends - starts, key[starts], key[ends - 1]

    def aggregate(self, q: dict[str, Any], kernels=None, hist: bool = False, partial: bool = False) -> dict[str, Any]:
        """Grouped aggregates over the filtered collection (``parse_aggregate`` has the request,
        ``AggGroups.response`` the answer).  One histogram of dictionary ids over the key columns
        (group-by..., aggregate key) per distinct aggregate key and one over (group-by...) for
        the row counts, slot ``len(values)`` of an axis = path missing: with ``kernels`` each is
        one fused filter + histogram launch (``hip/group_agg.hip``), without them a
        ``np.bincount`` over the rows the CPU scan selected -- also for a histogram with more
        cells than the device takes.  The non-zero cells decode through the dictionaries into
        ``AggGroups``; ``reduce_hist`` finishes, the same on every path.
        A key of ``extrema_keys`` whose histogram would pass ``EXTREMA_FROM_CELLS`` cells (a
        timestamp: one dictionary value per write) gets no histogram unless ``hist`` asks for
        it: one ``scan_extrema`` launch over the group columns and the key's rank-encoded copy
        gives its count, smallest and largest rank per group, the row under each rank decodes
        them -- O(groups).  Without kernels, or with more groups than the device takes,
        ``extrema_numpy`` does the same over the CPU selection.
        A key that is asked a SUM or an AVG, whose histogram would pass ``SUMS_FROM_CELLS`` cells
        and whose numbers share a scale (``Column.num_scale``: amounts, durations, points) gets,
        unless ``hist``, one ``scan_sums`` launch over the group columns and its own id column
        (``hip/group_sums.hip``; ``sums_numpy`` without kernels or past the device's groups):
        exact integer sums per group, which ``AggGroups`` turns into ``reduce_hist``'s answer;
        its COUNT / MIN / MAX come from the extrema path.  If a group's magnitudes reach 2^53
        the sums prove nothing and the key's histogram answers as before.
        A histogram, extrema or sums request past the device's cap of dense cells goes, from
        ``SPARSE_FROM_ROWS`` rows on and with kernels that have them, through the hashed scans
        (``scan_sparse`` / ``scan_extrema_sparse`` / ``scan_sums_sparse``): the same (cell, count,
        words) as the host's ``np.unique``, of the cells that occur, with no host selection.  A
        table capped at ``SPARSE_MAX_SLOTS`` that overflows answers None and that request alone
        falls through to the host code.
        ``partial``: the answer in the form shards merge (``AggGroups.response``)."""
        spec = parse_aggregate(q)
        # every referenced column first: one re-encode (source-backed) and one device upload
        self.ensure_columns(filter_paths(spec.filter) + spec.group_by + spec.keys)
        prog = self.compile_cached(spec.filter or {})
        gcols = [self.col_of[p] for p in spec.group_by]
        gdims = [self._dict_size(c) for c in gcols]
        gcells = math.prod(d + 1 for d in gdims)
        cap = int(kernels.lib.tt_group_max_cells()) if kernels is not None else None
        from_cells = self.EXTREMA_FROM_CELLS if cap is None else min(self.EXTREMA_FROM_CELLS, cap)
        ext_keys = [] if hist else [k for k in extrema_keys(spec)
                                    if gcells * (self._dict_size(self.col_of[k]) + 1) > from_cells]
        ext_dev = kernels is not None and gcells <= cap  # else the groups alone are past the dense cells
        # ... and then go through the hashed cells, when the kernels have them (a stand-in device
        # without them keeps the host plan) and the collection is worth a launch
        sparse = kernels is not None and self.n >= self.SPARSE_FROM_ROWS and all(
            getattr(kernels, name, None) is not None
            for name in ("scan_sparse", "scan_extrema_sparse", "scan_sums_sparse"))
        val_dev = ext_dev or (sparse and gcells < 1 << 62)  # the value kernels run on the device
        # SUM / AVG keys past their own threshold (compared alone: the device's cap does not lower
        # it) whose numbers share a scale that cannot wrap 64 bits over this many rows
        sum_path = [] if hist else [k for k in sum_keys(spec)
                                    if gcells * (self._dict_size(self.col_of[k]) + 1) > self.SUMS_FROM_CELLS
                                    and self.columns[self.col_of[k]].num_scale(self.n) is not None]
        # ... their COUNT / MIN / MAX then come from extrema, whatever EXTREMA_FROM_CELLS says
        sum_ext = [k for k in sum_path if any(op in EXTREMA_OPS for op, kk in spec.aggs if kk == k)]
        dev = None
        if kernels is not None:
            dev = (*self.mirror.program(prog, kernels, [self.col_of[k] for k in ext_keys + sum_ext] if val_dev else (),
                                        [self.col_of[k] for k in sum_path] if val_dev else ()), cap)
        host_rows: list[np.ndarray] = []  # the CPU selection, made once when a histogram needs it

        def selection() -> np.ndarray:
            if not host_rows:
                try:
                    host_rows.append(self.select_native(prog))
                except ImportError:
                    host_rows.append(self.select_numpy(prog))
            return host_rows[0]

        def counted(cnt, *words) -> tuple[np.ndarray, ...]:
            """(non-zero cells, their counts, each of ``words`` at those cells) of a device vector
            of uint32 counts held as int32; ``words``: (device vector, the dtype to read it as)."""
            cnt = cnt.cpu().numpy().view(np.uint32)
            cells = np.nonzero(cnt)[0]
            return (cells, cnt[cells], *(w.cpu().numpy().view(t)[cells] for w, t in words))

        def slots_for(ncells: int) -> int:
            """The hash table's slots for a space of ``ncells`` cells over this collection."""
            need = 2 * max(1, min(ncells, self.n))
            return min(self.SPARSE_MAX_SLOTS, max(2, 1 << (need - 1).bit_length()))

        def hashed(got, *types) -> tuple[np.ndarray, ...] | None:
            """A hashed scan's (cells, counts, words...) on the host; None (the table overflowed:
            the host answers) stays None."""
            if got is None:
                return None
            cells, cnt, *words = (t.cpu().numpy() for t in got)
            return (cells, cnt.view(np.uint32), *(w.view(t) for w, t in zip(words, types)))

        def extrema(kc: int) -> tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
            """(cells, rows with a value, smallest, largest rank << 32 | row) of column ``kc``."""
            if not ext_dev:
                if val_dev:
                    m = dev[0]
                    got = hashed(kernels.scan_extrema_sparse(m.table, m.live, self.cap, self.n, dev[1], dev[2], gcols,
                                                             gdims, m.rank_slot[kc], slots_for(gcells)),
                                 np.uint64, np.uint64)
                    if got is not None:
                        return got
                return self.extrema_numpy(selection(), gcols, gdims, kc)
            m = dev[0]
            cnt, lo, hi = kernels.scan_extrema(m.table, m.live, self.cap, self.n, dev[1], dev[2], gcols, gdims,
                                               m.rank_slot[kc])
            return counted(cnt, (lo, np.uint64), (hi, np.uint64))

        def sums(kc: int) -> tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
            """(cells, rows holding a number, sum of their m, sum of their |m|) of column ``kc``."""
            if not ext_dev:
                if val_dev:
                    m = dev[0]
                    got = hashed(kernels.scan_sums_sparse(m.table, m.live, self.cap, self.n, dev[1], dev[2], gcols,
                                                          gdims, kc, m.nums[kc], slots_for(gcells)),
                                 np.int64, np.uint64)
                    if got is not None:
                        return got
                return self.sums_numpy(selection(), gcols, gdims, kc)
            m = dev[0]
            cnt, s, a = kernels.scan_sums(m.table, m.live, self.cap, self.n, dev[1], dev[2], gcols, gdims, kc,
                                          m.nums[kc])
            return counted(cnt, (s, np.int64), (a, np.uint64))

        def histogram(cols: list[int]) -> tuple[np.ndarray, np.ndarray, list[int]]:
            """(non-zero cells, their counts, the axes' sizes) of the key columns ``cols``."""
            dims = [self._dict_size(c) for c in cols]  # after the upload: widths match
            ncells = math.prod(d + 1 for d in dims)
            if ncells >= 1 << 62:
                raise Unsupported("aggregate key space too large")
            if dev is not None and ncells <= dev[3]:
                return *counted(kernels.scan_group(dev[0].table, dev[0].live, self.cap, self.n, dev[1], dev[2],
                                                   cols, dims)), dims
            if sparse:
                got = hashed(kernels.scan_sparse(dev[0].table, dev[0].live, self.cap, self.n, dev[1], dev[2],
                                                 cols, dims, slots_for(ncells)))
                if got is not None:
                    return *got, dims
            cell = self.cells_of(selection(), cols, dims)
            if ncells <= self.HOST_MAX_CELLS:
                counts = np.bincount(cell, minlength=ncells)
                cells = np.nonzero(counts)[0]
                return cells, counts[cells], dims
            cells, counts = np.unique(cell, return_counts=True)
            return cells, counts, dims

        def decode(cells: np.ndarray, dims: list[int]) -> list[list[int]]:
            slots = []
            for d in reversed(dims):
                cells, s = np.divmod(cells, d + 1)
                slots.append(s.tolist())
            return slots[::-1]

        def value(col: int, slot: int) -> Any:
            vals = self.columns[col].values
            return vals[slot] if slot < len(vals) else _MISSING

        groups = AggGroups(spec)
        cells, counts, dims = histogram(gcols)
        slots = decode(cells, dims)
        for i, n in enumerate(counts.tolist()):
            groups.add_rows(tuple(value(c, s[i]) for c, s in zip(gcols, slots)), n)
        for key in spec.keys:
            kc = self.col_of[key]
            summed = False
            if key in sum_path:
                cells, counts, s, a = sums(kc)
                # a group whose magnitudes reach 2^53 proves nothing: the key's histogram answers.
                # That fallback costs one pass more than before -- this launch, and for a key of
                # ``sum_ext`` the rank-encoded copy uploaded above -- known only after the sums.
                summed = not bool((a >= np.uint64(1 << 53)).any())
                if summed:
                    e = self.columns[kc].num_scale(self.n)[0]
                    slots = decode(cells, gdims)
                    for i, (n, si, ai) in enumerate(zip(counts.tolist(), s.tolist(), a.tolist())):
                        groups.add_sums(tuple(value(c, sl[i]) for c, sl in zip(gcols, slots)), key, n, si, ai, e)
                    if key not in sum_ext:
                        continue
            if key in ext_keys or summed:
                cells, counts, lo, hi = extrema(kc)
                slots = decode(cells, gdims)
                vals = self.columns[kc].values
                lo_ids = self.ids[kc, (lo & np.uint64(0xFFFFFFFF)).astype(np.int64)].tolist()
                hi_ids = self.ids[kc, (hi & np.uint64(0xFFFFFFFF)).astype(np.int64)].tolist()
                for i, n in enumerate(counts.tolist()):
                    groups.add_extrema(tuple(value(c, s[i]) for c, s in zip(gcols, slots)), key, n,
                                       vals[lo_ids[i]], vals[hi_ids[i]])
                continue
            cells, counts, dims = histogram(gcols + [kc])
            slots = decode(cells, dims)
            for i, n in enumerate(counts.tolist()):
                v = value(kc, slots[-1][i])
                if v is not _MISSING:
                    groups.add_value(tuple(value(c, s[i]) for c, s in zip(gcols, slots)), key, v, n)
        return groups.response(hist, partial)

    # -- full query --------------------------------------------------------------
    def order(self, rows: np.ndarray, sort: list[dict[str, Any]] | None, k: int | None = None) -> np.ndarray:
        """``rows`` in result order; with ``k``, only the first ``k`` of that order (a page: one
        partition of the packed keys, then a sort of those ``k``, instead of a full sort)."""
        if rows.size == 0:
            return rows
        plan = self.sort_specs(sort)
        if plan is not None:  # packed keys (the ones the GPU path sorts; unique: seq is the tail)
            keys = self.sort_keys_numpy(rows, plan)
            if k is not None and 0 < k < rows.size:
                part = np.argpartition(keys, k - 1)[:k]
                return rows[part[np.argsort(keys[part])]]
            return rows[np.argsort(keys, kind="stable")]
        out = self.order_lexsort(rows, sort)
        return out[:k] if k else out

    def order_lexsort(self, rows: np.ndarray, sort: list[dict[str, Any]] | None) -> np.ndarray:
        """Reference ordering: insertion order, then a stable lexsort on the sort keys' ranks."""
        if rows.size == 0:
            return rows
        rows = rows[np.argsort(self.seq[rows], kind="stable")]  # insertion order, then stable sort keys
        if not sort:
            return rows
        keys = []
        for f in reversed(self.sort_fields(sort)[0]):  # np.lexsort: last key is primary
            r = gather(f.ranks, self.ids[f.col, rows], f.missing)
            keys.append(-r if f.desc else r)
        return rows[np.lexsort(keys)]

    def sort_fields(self, sort: list[dict[str, Any]] | None) -> tuple[list[SortField], int]:
        """The packed ordering key [rank(key0) | ... | seq] of ``sort``: its fields, primary first,
        and the bits of the sequence tail -- for ``sort_specs``, ``DeviceMirror.sort_plan`` and
        ``order_lexsort`` alike."""
        fields = []
        for s in sort or []:
            col = self.add_column(s["key"])
            c = self.columns[col]
            ranks = c.ranks() if c.values else np.zeros(0, dtype=np.int64)
            miss = c.missing_rank()
            # a string-only dictionary's ranks are exactly 1..n: no O(dictionary) max per query
            max_rank = max(len(c.values) if c.str_only else int(ranks.max(initial=0)), miss)
            desc = int(str(s.get("order", "ASC")).upper() == "DESC")
            fields.append(SortField(col, ranks, miss, max_rank, max(1, max_rank.bit_length()), desc))
        # every seq is <= the last one handed out
        return fields, max(1, int(self._next_seq).bit_length())

    def sort_specs(self, sort: list[dict[str, Any]] | None) -> tuple[np.ndarray, np.ndarray, int] | None:
        """Device ordering plan: (specs int32 [nkeys, 8], concatenated rank tables, seq bits), or
        None when the packed key would not fit 63 bits (the host path orders instead)."""
        fields, seq_bits = self.sort_fields(sort)
        if seq_bits + sum(f.bits for f in fields) > 63:
            return None
        offs = np.cumsum([0] + [f.ranks.size for f in fields])
        specs = [[f.col, int(off), f.ranks.size, f.bits, f.desc, f.missing, f.max_rank, 0]
                 for f, off in zip(fields, offs)]
        tables = [f.ranks.astype(np.int32) for f in fields if f.ranks.size] or [np.zeros(1, dtype=np.int32)]
        return np.array(specs, dtype=np.int32).reshape(-1, 8), np.concatenate(tables), seq_bits

    def sort_keys_numpy(self, rows: np.ndarray, plan) -> np.ndarray:
        """Host reference of ``hip/sort_keys.hip``: the packed ordering key of every row."""
        specs, ranks, seq_bits = plan
        k = np.zeros(rows.size, dtype=np.int64)
        for col, off, nranks, bits, desc, miss, max_rank, _ in specs.tolist():
            ids = self.ids[col, rows]
            ok = (ids >= 0) & (ids < nranks)
            r = np.full(rows.size, miss, dtype=np.int64)
            r[ok] = ranks[off + ids[ok]]
            if desc:
                r = max_rank - r
            k = (k << bits) | r
        return (k << seq_bits) | self.seq[rows]

    def order_gpu(self, rows, sort, kernels, k: int | None = None):
        """Order a device selection on the GPU; device rows, or None when the host must order."""
        return self.mirror.order(rows, sort, kernels, k)

    def warm(self, kernels) -> None:
        """Called by the accelerator's background sync (backing/accel.py) under its lock."""
        self.mirror.warm(kernels)

    def page_gpu(self, prog: Program, sort, kernels, offset: int, limit: int):
        """(rows, token) of the page, or None: the caller takes the full path (``DeviceMirror.page``)."""
        return self.mirror.page(prog, sort, kernels, offset, limit)

    def query(self, q: dict[str, Any], kernels=None) -> tuple[list[str], str | None]:
        """Returns (keys in result order for the requested page, continuation token)."""
        rows, token = self.query_rows(q, kernels)
        return [self.keys[i] for i in rows.tolist()], token

    def query_rows(self, q: dict[str, Any], kernels=None) -> tuple[np.ndarray, str | None]:
        """(rows in result order for the requested page, continuation token)."""
        sort = q.get("sort")
        # every referenced column first: one re-encode (source-backed) and one device upload
        self.ensure_columns(filter_paths(q.get("filter")) + [s["key"] for s in sort or []
                                                             if isinstance(s, dict) and "key" in s])
        prog = self.compile_cached(q.get("filter") or {})
        page = q.get("page") or {}
        limit = int(page.get("limit") or 0)
        offset = int(page.get("token") or 0)
        rows = None
        if kernels is not None and limit:
            paged = self.page_gpu(prog, sort, kernels, offset, limit)
            if paged is not None:
                return paged
        if kernels is not None:
            dev_rows = self.select_gpu(prog, kernels, on_device=True)
            total = int(dev_rows.numel())
            ordered = self.order_gpu(dev_rows, sort, kernels, offset + limit if limit else None)
            if ordered is not None:
                end = min(total, offset + limit) if limit else total
                sel = ordered[offset:end].cpu().numpy()
                if kernels.check_sort():
                    token = str(end) if limit and end < total else None
                    return sel.astype(np.int32, copy=False), token
                # a look-back timed out in the device sort: this query orders on the host
            rows = dev_rows.cpu().numpy()
        if rows is None:  # no GPU: every core of the CPU share over the same narrow codes
            try:
                rows = self.select_native(prog)
            except ImportError:
                rows = self.select_numpy(prog)
        total = rows.size
        rows = self.order(rows, sort, offset + limit if limit else None)
        end = min(total, offset + limit) if limit else total
        sel = rows[offset:end]
        token = str(end) if limit and end < total else None
        return sel.astype(np.int32, copy=False), token
