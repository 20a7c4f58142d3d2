"""The GPU side of a ``ColumnarIndex``: its columns in the narrow code layout (``ops/codes.py``),
rank-encoded copies for range leaves, the descriptor table, the ordering plans' rank tables, the
zone maps and tile search of the paged path.  The index tells it what changed (``invalidate``,
``tombstoned``, ``touch``, ``reset_zones``); it reads the index's ``ids / live / seq / n / cap /
columns`` and reaches the device only through the ``kernels`` handed in (``ops/gpu.py``)."""
from __future__ import annotations

import json
import time
from collections import Counter
from dataclasses import dataclass, field
from typing import Any, NamedTuple

import numpy as np

from .codes import OP_EQ, OP_LEAF, OP_RANGE, TILE, torch_dtype, width_for


@dataclass
class RankColumn:
    """A column's rows as sort ranks (what range leaves compare), kept on the device."""
    t: Any                  # the rank codes, one per row of the index's capacity
    w: int                  # their width (bytes)
    ver: int                # Column.rank_version they were encoded from
    synced: int = 0         # rows encoded so far
    table: Any = None       # id -> rank on the device: table_buf[:dictionary size]
    table_buf: Any = None   # its buffer, kept across versions and grown by doubling
    src: Any = None         # the source column's 16-byte descriptor on the device ...
    src_key: tuple | None = None  # ... and what it holds: (address, width)


@dataclass
class NumTable:
    """A column's scaled integers per dictionary id (``Column.nums``), kept on the device."""
    buf: Any                # int64, grown by doubling
    n: int = 0              # ids uploaded so far
    epoch: int = -1         # Column.scale_epoch they were computed at


@dataclass
class Zone:
    """Zone map of one sort spec: per tile the live row with the smallest ordering key."""
    sort: Any
    zarg: np.ndarray = field(default_factory=lambda: np.zeros(0, dtype=np.int32))
    dirty: set = field(default_factory=set)       # tiles whose rows changed since the last refresh
    all: bool = True                              # every tile is to be recomputed
    density: dict = field(default_factory=dict)   # per filter: candidates per row of a chosen tile
    short: dict = field(default_factory=dict)     # per filter: the last page held every match


class SortPlan(NamedTuple):
    specs: Any      # int32 [nkeys, 8] on the device (hip/sort_key.h SortSpec)
    ranks: Any      # the keys' rank tables on the device
    seq_bits: int
    key_bits: int
    host: tuple     # (specs, rank tables, seq bits) for ColumnarIndex.sort_keys_numpy


@dataclass
class _PlanBuffers:  # rank tables of one sort spec: one capacity-doubled region per key, host and device
    caps: list[int]
    offs: np.ndarray
    seqs: list[int]         # Column.rank_seq each region was last copied at
    host: np.ndarray
    dev: Any
    specs_dev: Any
    specs: np.ndarray | None = None


class DeviceMirror:
    def __init__(self, index) -> None:
        self.index = index
        # device buffers and how far they follow the index
        self.cols: list[Any] = []
        self.widths: list[int] = []
        self.live: Any = None
        self.seq: Any = None
        self.synced = 0
        self.cap = 0
        self.ranks: dict[int, RankColumn] = {}
        self.rank_slot: dict[int, int] = {}   # column -> row of its rank copy in ``table``
        self.rank_cols: list[int] = []        # columns the last program read as ranks (``warm``)
        self._nums: dict[int, NumTable] = {}
        self.nums: dict[int, Any] = {}        # column -> id -> m on the device, of the last ``program``
        self.table: Any = None                # the column descriptor table of the last sync
        self.table_widths: np.ndarray | None = None
        self._tables: dict[tuple, Any] = {}   # descriptor tables by content: no upload per query
        self._tomb_dirty = False   # liveness changed for rows that are already on the device
        self._full_dirty = True    # layout changed (compaction / new column / growth)
        self._plan_cache: dict[Any, _PlanBuffers] = {}
        self.zones: dict[str, Zone] = {}
        self.timing: Counter = Counter()  # where the paged device path spends its time (summed)
        self._plan_tm: Counter | None = None  # ``timing`` while ``page`` plans (sub-step times)

    # -- what the index reports -----------------------------------------------------------
    def invalidate(self) -> None:
        """The layout changed (reload, compaction, new column, growth): upload everything."""
        self._full_dirty = True

    def tombstoned(self) -> None:
        """Rows that are already uploaded died."""
        self._tomb_dirty = True

    def touch(self, tiles) -> None:
        """Rows of ``tiles`` were added or killed."""
        for z in self.zones.values():
            if not z.all:
                z.dirty.update(int(t) for t in tiles)

    def reset_zones(self) -> None:
        for z in self.zones.values():
            z.all, z.dirty = True, set()

    # -- upload -----------------------------------------------------------------------------
    def _column(self, kernels, col: int, width: int):
        """The whole column in the device layout; 2-bit columns get 16 bytes of padding (the
        reads past the end of a partial group stay inside the buffer)."""
        v = self.index.codes(col, 0, self.index.cap, width)
        if width == 0:
            v = np.concatenate([v, np.zeros(16, dtype=np.uint8)])
        return kernels.torch.from_numpy(np.ascontiguousarray(v)).to(kernels.device)

    def sync(self, kernels, rank_cols=()) -> "DeviceMirror":
        """Bring the device copies up to the index.  Columns are append-only between compactions,
        so only rows added since the last sync are uploaded; tombstones re-upload the 1-bit
        liveness mask (N/8 bytes); a column whose dictionary outgrows its width is re-encoded."""
        ix = self.index
        torch = kernels.torch
        dev = kernels.device
        widths = [width_for(len(c.values)) for c in ix.columns]
        nwords = ix.cap // 16
        if self._full_dirty or self.cap != ix.cap or len(self.cols) != len(ix.columns):
            if self._full_dirty:
                self.reset_zones()
            self.cols = [self._column(kernels, i, w) for i, w in enumerate(widths)]
            self.widths = widths
            self.live = torch.from_numpy(ix.live_words(0, nwords)).to(dev)
            self.seq = torch.from_numpy(ix.seq[:ix.cap].astype(np.int32)).to(dev)  # uint32 on device
            self.synced, self.cap = ix.n, ix.cap
            self.ranks, self.rank_slot, self._tables = {}, {}, {}
            self._nums, self.nums = {}, {}
        else:
            lo, hi = self.synced, ix.n
            # the appended rows of every column, the sequence and the liveness words go up in
            # one scatter launch (GpuKernels.upload), not one copy each
            segs = []
            for i, w in enumerate(widths):
                if w != self.widths[i]:
                    self.cols[i] = self._column(kernels, i, w)
                    self.widths[i] = w
                elif hi > lo and w == 0:  # whole bytes of 4 rows: re-pack the edge bytes
                    a, b = lo // 4, (hi + 3) // 4
                    segs.append((self.cols[i].data_ptr() + a, ix.codes(i, 4 * a, 4 * b, 0)))
                elif hi > lo:
                    segs.append((self.cols[i].data_ptr() + lo * w, ix.codes(i, lo, hi, w)))
            if hi > lo:
                segs.append((self.seq.data_ptr() + 4 * lo, ix.seq[lo:hi].astype(np.int32)))
            if self._tomb_dirty:
                segs.append((self.live.data_ptr(), ix.live_words(0, nwords)))
            elif hi > lo:
                w0, w1 = lo // 16, (hi + 15) // 16
                segs.append((self.live.data_ptr() + 2 * w0, ix.live_words(w0, w1)))
            kernels.upload(segs)
            self.synced = hi
        self._full_dirty = False
        self._tomb_dirty = False
        rows = [[c.data_ptr(), w] for c, w in zip(self.cols, self.widths)]
        if rank_cols:
            # rank-encoded copies of the columns that range leaves read (appended to the table)
            slot = {}
            for col in sorted(set(rank_cols)):
                rc = self._sync_rank_column(kernels, col)
                slot[col] = len(rows)
                rows.append([rc.t.data_ptr(), rc.w])
            self.rank_slot = slot
        # the descriptor table only changes with the device buffers: no upload per query
        self.table_widths = np.array([w for _, w in rows], dtype=np.int64)
        tkey = tuple(tuple(r) for r in rows)
        t = self._tables.get(tkey)
        if t is None:
            if len(self._tables) >= 16:
                self._tables.clear()
            t = self._tables[tkey] = torch.from_numpy(np.array(rows, dtype=np.int64).reshape(-1, 2)).to(dev)
        self.table = t
        return self

    def _sync_rank_column(self, kernels, col: int) -> RankColumn:
        ix = self.index
        torch = kernels.torch
        c = ix.columns[col]
        w = max(1, self.widths[col])  # ranks run 1..n and need a distinct missing code: >= 1 byte
        cur = self.ranks.get(col)
        full = cur is None or cur.w != w or cur.ver != c.rank_version
        lo = 0 if full else cur.synced
        if not full and lo >= ix.n:
            return cur
        segs = []  # the rank table and the source descriptor: one scatter launch, no copies
        if full:
            prev = cur
            # re-encoded from row 0 into the same buffer when it still fits: its address is in
            # the column descriptor table, which then needs no new upload
            keep = prev is not None and prev.w == w and prev.t.numel() == ix.cap
            cur = self.ranks[col] = RankColumn(
                prev.t if keep else torch.empty(ix.cap, dtype=torch_dtype(torch, w), device=kernels.device),
                w, c.rank_version)
            table = c.ranks().astype(np.int32) if c.values else np.zeros(1, dtype=np.int32)
            # a new dictionary value re-ranks the column (every new due date does): the table's
            # device buffer is kept across versions and grown by doubling
            buf = prev.table_buf if prev is not None else None
            if buf is None or buf.numel() < table.size:
                buf = torch.empty(max(1024, 1 << (table.size - 1).bit_length()), dtype=torch.int32,
                                  device=kernels.device)
            cur.table_buf, cur.table = buf, buf[:table.size]
            segs.append((buf.data_ptr(), table))
            if prev is not None:
                cur.src, cur.src_key = prev.src, prev.src_key
        key = (self.cols[col].data_ptr(), self.widths[col])
        if cur.src_key != key:  # the source column's descriptor: uploaded when it changes
            if cur.src is None:
                cur.src = torch.empty((1, 2), dtype=torch.int64, device=kernels.device)
            segs.append((cur.src.data_ptr(), np.array([list(key)], dtype=np.int64)))
            cur.src_key = key
        kernels.upload(segs)
        kernels.rank_encode(cur.src, cur.table, lo, ix.n, cur.t, w)
        cur.synced = ix.n
        return cur

    def _sync_num_table(self, kernels, col: int) -> Any:
        """The device copy of ``Column.nums`` up to the dictionary's size: the new tail alone
        while the scale holds, the whole table when it changed (``scale_epoch``) and after a
        full re-upload."""
        torch = kernels.torch
        c = self.index.columns[col]
        if c.num_scale() is None:
            raise ValueError("the column's numbers share no scale")
        n = len(c.values)
        cur = self._nums.get(col)
        if cur is None:
            cur = self._nums[col] = NumTable(torch.empty(max(1024, 1 << max(0, n - 1).bit_length()),
                                                         dtype=torch.int64, device=kernels.device))
        if cur.epoch != c.scale_epoch or cur.n > n:
            cur.n, cur.epoch = 0, c.scale_epoch
        if cur.buf.numel() < n:
            grown = torch.empty(1 << (n - 1).bit_length(), dtype=torch.int64, device=kernels.device)
            grown[:cur.n] = cur.buf[:cur.n]
            cur.buf = grown
        if n > cur.n:
            kernels.upload([(cur.buf.data_ptr() + 8 * cur.n, c.nums(cur.n, n))])
            cur.n = n
        return cur.buf[:n]

    def program(self, prog, kernels, rank_cols=(), num_cols=()):
        """Sync for ``prog`` and return (mirror, program, bitmaps) ready for ``GpuKernels.select``
        (range leaves remapped to their rank-encoded columns).  ``rank_cols``: further columns to
        keep rank-encoded copies of (``rank_slot`` has their rows of the table): the value
        columns of ``GpuKernels.scan_extrema``.  ``num_cols``: columns whose scaled-integer
        tables (``Column.nums``) to keep on the device (``nums`` has them): the value columns
        of ``GpuKernels.scan_sums``."""
        leaf = (prog.code[:, 0] == OP_LEAF) | (prog.code[:, 0] == OP_EQ) | (prog.code[:, 0] == OP_RANGE)
        if leaf.any() and int(prog.code[leaf, 1].max()) >= len(self.index.columns):
            raise ValueError("program references a column outside the index")
        if any(not 0 <= c < len(self.index.columns) for c in rank_cols):
            raise ValueError("rank column outside the index")
        rng = prog.code[:, 0] == OP_RANGE
        leaves = prog.code[rng, 1].tolist()
        self.rank_cols = leaves + [int(c) for c in rank_cols]
        if any(not 0 <= c < len(self.index.columns) for c in num_cols):
            raise ValueError("number column outside the index")
        self.sync(kernels, self.rank_cols)
        self.nums = {int(c): self._sync_num_table(kernels, int(c)) for c in sorted(set(num_cols))}
        slots = tuple(sorted((c, self.rank_slot[c]) for c in set(leaves)))  # the program's own
        cached = prog.device
        if cached is not None and cached[0] == (slots, str(kernels.device)):
            return self, cached[1], cached[2]
        code_np = prog.code
        if rng.any():  # range leaves read the rank-encoded copy of their column
            code_np = prog.code.copy()
            code_np[rng, 1] = [self.rank_slot[c] for c in leaves]
        code = kernels.torch.from_numpy(code_np).to(kernels.device)
        bitmaps = kernels.torch.from_numpy(prog.bitmaps).to(kernels.device)
        prog.device = ((slots, str(kernels.device)), code, bitmaps)  # reused while the slots hold
        return self, code, bitmaps

    def select(self, prog, kernels, return_mask: bool = False):
        _, code, bitmaps = self.program(prog, kernels)
        return kernels.select(self.table, self.live, self.index.cap, self.index.n, code, bitmaps,
                              return_mask=return_mask)

    # -- ordering ---------------------------------------------------------------------------
    def sort_plan(self, sort, kernels) -> SortPlan | None:
        """The packed key's specs and rank tables on the device, with the host plan of the same
        key, kept per sort spec; None when the device cannot order by it (too many keys, a key
        over 63 bits, a sequence over 32 bits).  Only the ids whose rank is new or moved since the
        last query are copied (``Column.rank_changes_since``): for the timestamps of new writes
        those are the newest ids -- O(new values) per query, not the whole table."""
        if len(sort or []) > kernels.max_sort_keys:
            return None
        ix = self.index
        tm = self._plan_tm  # ``page``'s timing dict while it plans (None for the background warm)
        c0 = time.thread_time()
        fields, seq_bits = ix.sort_fields(sort)
        key_bits = seq_bits + sum(f.bits for f in fields)
        if seq_bits > 32 or key_bits > 63:  # the device keeps a 32-bit insertion sequence
            return None
        torch = kernels.torch
        pkey = (json.dumps(sort, sort_keys=True, default=str), str(kernels.device), ix._dict_gen)
        ent = self._plan_cache.get(pkey)
        cols = [ix.columns[f.col] for f in fields]
        specs_rows = [[f.col, 0, f.ranks.size, f.bits, f.desc, f.missing, f.max_rank, 0] for f in fields]
        los = [None] * len(fields) if ent is None else \
            [c.rank_changes_since(sq) for c, sq in zip(cols, ent.seqs)]
        rebuild = ent is None or any(lo is None for lo in los) or \
            any(f.ranks.size > cap for f, cap in zip(fields, ent.caps))
        c1 = time.thread_time()
        if tm is not None:
            tm.update(plan_ranks_ms=(c1 - c0) * 1e3, plan_rebuilds=int(rebuild))
        if rebuild:
            caps = [max(1024, 1 << max(0, int(f.ranks.size * 1.25) + 1).bit_length()) for f in fields]
            offs = np.concatenate([[0], np.cumsum(caps)[:-1]]).astype(np.int64) if caps else np.zeros(0, np.int64)
            host = np.zeros(max(1, int(sum(caps))), dtype=np.int32)
            for f, off in zip(fields, offs):
                host[off:off + f.ranks.size] = f.ranks
            ent = _PlanBuffers(caps, offs, [c.rank_seq for c in cols], host,
                               torch.from_numpy(host).to(kernels.device),
                               torch.empty((len(specs_rows), 8), dtype=torch.int32, device=kernels.device))
            if len(self._plan_cache) >= 64:
                self._plan_cache.pop(next(iter(self._plan_cache)))
            self._plan_cache[pkey] = ent
        segs = []  # rank tails and the spec rows: one scatter launch (ops/gpu.py upload)
        if not rebuild:
            for i, (f, c, lo) in enumerate(zip(fields, cols, los)):
                off = int(ent.offs[i])
                if f.ranks.size > lo:  # the ids whose rank is new or moved (the newest ones)
                    tail = f.ranks[lo:].astype(np.int32)
                    ent.host[off + lo:off + f.ranks.size] = tail
                    segs.append((ent.dev.data_ptr() + 4 * (off + lo), tail))
                ent.seqs[i] = c.rank_seq
        for row, off in zip(specs_rows, ent.offs):
            row[1] = int(off)
        specs = np.array(specs_rows, dtype=np.int32).reshape(-1, 8)
        if ent.specs is None or not np.array_equal(specs, ent.specs):
            # the spec rows change with every new dictionary value (row[2] is the table's size):
            # they ride the same launch into a buffer allocated once per plan
            ent.specs = specs
            segs.append((ent.specs_dev.data_ptr(), specs))
        c2 = time.thread_time()
        kernels.upload(segs)
        if tm is not None:
            tm.update(plan_tails_ms=(c2 - c1) * 1e3, plan_upload_ms=(time.thread_time() - c2) * 1e3,
                      plan_tail_rows=sum(int(t.size) for _, t in segs))
        return SortPlan(ent.specs_dev, ent.dev, seq_bits, key_bits, (specs, ent.host, seq_bits))

    def order(self, rows, sort, kernels, k: int | None = None):
        """Order a device selection (``hip/sort_keys.hip`` + radix sort / top-k); device rows, or
        None when the host must order."""
        plan = self.sort_plan(sort, kernels)
        if plan is None:
            return None
        self.sync(kernels)  # sort keys may have added columns
        return kernels.order(self.table, rows, plan.specs, plan.ranks, self.seq, plan.seq_bits, k, plan.key_bits)

    # -- paged ordered queries ------------------------------------------------------------------
    def _ntiles(self) -> int:
        return (self.index.n + TILE - 1) // TILE

    def _zone_refresh(self, z: Zone, kernels, plan: SortPlan) -> None:
        """Recompute the zone argmin of the tiles that changed since the last refresh."""
        ntiles = self._ntiles()
        if z.zarg.size < ntiles:  # new tiles: not computed yet
            z.dirty.update(range(z.zarg.size, ntiles))
            z.zarg = np.concatenate([z.zarg, np.full(ntiles - z.zarg.size, -1, dtype=np.int32)])
        z.zarg = z.zarg[:ntiles]
        todo = np.arange(ntiles, dtype=np.int32) if z.all else \
            np.fromiter((t for t in z.dirty if t < ntiles), dtype=np.int32)
        if todo.size:
            z.zarg[todo] = kernels.zone_argmin(self.table, self.live, self.index.n, plan.specs, plan.ranks,
                                               self.seq, plan.seq_bits, todo)
        z.all, z.dirty = False, set()

    def warm(self, kernels) -> None:
        """Upload the rows synced since the last query (with the rank-encoded columns the last
        queries read) and refresh the zone maps of the sorts already served, so a query finds
        little to do."""
        self.sync(kernels, self.rank_cols)
        for z in list(self.zones.values()):
            if z.all or z.dirty or z.zarg.size < self._ntiles():
                plan = self.sort_plan(z.sort, kernels)
                if plan is not None:
                    self._zone_refresh(z, kernels, plan)

    def page(self, prog, sort, kernels, offset: int, limit: int):
        """A page [offset, offset + limit) of an ordered query without scanning the collection
        (``hip/page_topk.hip``): zone maps pick the tiles that can hold the page, only those are
        evaluated, one workgroup orders the candidates.  Returns (rows, token) or None when the
        page does not fit the device top-k (the caller takes the full path)."""
        k_total = offset + limit
        if limit <= 0 or k_total > kernels.page_cap:
            return None
        ix = self.index
        tm = self.timing
        t0, c0 = time.perf_counter(), time.thread_time()
        self._plan_tm = tm
        try:
            plan = self.sort_plan(sort, kernels)
        finally:
            self._plan_tm = None
        if plan is None:
            return None
        t1 = time.perf_counter()
        _, code, bitmaps = self.program(prog, kernels)
        t2, c2 = time.perf_counter(), time.thread_time()
        # host_cpu: this thread's CPU time in plan + program, the wall time less the waits (GIL,
        # other threads on the core)
        tm.update(page_plan_ms=(t1 - t0) * 1e3, page_program_ms=(t2 - t1) * 1e3, page_host_cpu_ms=(c2 - c0) * 1e3)
        ntiles = self._ntiles()
        if ntiles == 0:
            return np.zeros(0, dtype=np.int32), None
        zkey = json.dumps(sort, sort_keys=True, default=str)
        z = self.zones.get(zkey)
        if z is None:
            z = self.zones[zkey] = Zone(sort)
        self._zone_refresh(z, kernels, plan)
        t3 = time.perf_counter()
        tm["page_zones_ms"] += (t3 - t2) * 1e3
        valid = z.zarg >= 0
        nvalid = int(valid.sum())
        if nvalid == 0:
            return np.zeros(0, dtype=np.int32), None
        top = np.iinfo(np.uint64).max
        keys = np.full(ntiles, top, dtype=np.uint64)
        keys[valid] = ix.sort_keys_numpy(z.zarg[valid], plan.host).astype(np.uint64)
        pkey = (prog.code.tobytes(), prog.bitmaps.tobytes())
        dens = z.density.get(pkey, 0.25)  # candidates per row of a chosen tile, from the last page
        b = min(nvalid, max(1, int(np.ceil(1.5 * k_total / max(dens * TILE, 1.0)))))
        if z.short.get(pkey):
            # the last page of this filter held every match in the collection (fewer than the
            # page): start from every tile instead of growing towards it one launch at a time
            b = nvalid
        lo_b, hi_b = 0, None  # largest tile count seen short of k candidates / smallest that overflowed
        launches = 0
        for _ in range(24):
            if b >= nvalid:
                chosen, bound = np.nonzero(valid)[0].astype(np.int32), top
            else:
                part = np.argpartition(keys, b)
                chosen, bound = part[:b].astype(np.int32), int(keys[part[b]])
            rows, total, complete = kernels.page(self.table, self.live, ix.n, code, bitmaps, plan.specs, plan.ranks,
                                                 self.seq, plan.seq_bits, chosen, k_total, offset, bound)
            launches += 1
            if complete:
                break
            if total > kernels.page_cap:  # more candidates than one workgroup sorts: fewer tiles
                hi_b = b
            else:
                lo_b = b
            if hi_b is None:
                b = min(nvalid, b * 4)
            elif hi_b - lo_b <= 1:
                return None  # no tile count gives k candidates the LDS sort holds
            else:
                b = (lo_b + hi_b) // 2
        else:
            return None
        if len(chosen):
            z.density[pkey] = max(total / (len(chosen) * TILE), 1e-4)
            if len(z.density) > 64:
                z.density.pop(next(iter(z.density)))
        z.short[pkey] = bound == top and total < k_total
        if len(z.short) > 64:
            z.short.pop(next(iter(z.short)))
        t4 = time.perf_counter()
        tm.update(page_kernels_ms=(t4 - t3) * 1e3, page_launches=launches)
        if total > k_total:
            more = True
        elif bound == top:
            more = False
        else:  # the page used every candidate: are there matches in the tiles left out?
            more = int(self.select(prog, kernels).numel()) > k_total
            tm["page_more_ms"] += (time.perf_counter() - t4) * 1e3
        return rows, (str(k_total) if more else None)
