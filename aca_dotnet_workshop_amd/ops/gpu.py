"""ctypes bindings to the gfx950 query kernels (``_ttgpu.so``) operating on torch tensors.

No silent fallback: ``GpuKernels()`` raises if the library or a HIP device is missing; the
caller (``backing.accel``) decides explicitly whether to use the CPU executor instead.
"""
from __future__ import annotations

import ctypes
import threading
from typing import Any

import numpy as np

from .build import LIB, build_gpu

_lib = None


def load_library(build: bool = True) -> ctypes.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    if build:
        build_gpu()
    if not LIB.exists():
        raise RuntimeError(f"GPU kernel library {LIB} is missing; run `python -m aca_dotnet_workshop_amd.ops.build`")
    # PyDLL: calls keep the GIL.  Every entry point but one is a kernel launch (microseconds);
    # releasing the GIL around those costs more -- a query thread next to a busy event loop
    # waits up to the switch interval to get it back, once per call.  The exception is the
    # stream synchronise (``_sync``): it waits for whatever the shared stream holds (another
    # thread's mirror sync included), so it goes through a CDLL handle that drops the GIL while
    # it waits -- the backing's event loop keeps serving meanwhile.
    lib = ctypes.PyDLL(str(LIB))
    wait = ctypes.CDLL(str(LIB))
    wait.tt_stream_sync.argtypes = [ctypes.c_void_p]
    wait.tt_stream_sync.restype = ctypes.c_int
    lib.blocking_sync = wait.tt_stream_sync
    P, I64, I32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32
    lib.tt_launch_scan_eval.argtypes = [P, I64, P, P, I32, P, I32, P, P, P]
    lib.tt_launch_scan_eval.restype = ctypes.c_int
    lib.tt_sort_pairs_temp_bytes.argtypes = [I64, I32]
    lib.tt_sort_pairs_temp_bytes.restype = ctypes.c_int64
    lib.tt_sort_pairs.argtypes = [P, P, P, P, I64, I32, P, I64, P, P]
    lib.tt_sort_pairs.restype = ctypes.c_int
    lib.tt_launch_scan_compact.argtypes = [P, P, P, I64, P, I64, P, P, P]
    lib.tt_launch_compact.argtypes = [P, P, I64, P, I64, P]
    lib.tt_launch_compact.restype = ctypes.c_int
    lib.tt_launch_scan_compact.restype = ctypes.c_int
    lib.tt_launch_group_count.argtypes = [P, I32, P, I64, I32, P, P]
    lib.tt_launch_group_count.restype = ctypes.c_int
    lib.tt_launch_scan_group.argtypes = [P, I64, P, P, I32, P, I32, P, P, I32, P, I32, P]
    lib.tt_launch_scan_group.restype = ctypes.c_int
    lib.tt_group_max_cells.restype = ctypes.c_int
    lib.tt_launch_scan_extrema.argtypes = [P, I64, P, P, I32, P, I32, P, P, I32, I32, P, P, P, I32, P]
    lib.tt_launch_scan_extrema.restype = ctypes.c_int
    lib.tt_extrema_max_lds_cells.restype = ctypes.c_int
    lib.tt_launch_scan_sums.argtypes = [P, I64, P, P, I32, P, I32, P, P, I32, I32, P, I64, P, P, P, I32, P]
    lib.tt_launch_scan_sums.restype = ctypes.c_int
    lib.tt_launch_scan_sparse.argtypes = [P, I64, P, P, I32, P, I32, P, P, I32, P, P, I64, P, I32, P]
    lib.tt_launch_scan_sparse.restype = ctypes.c_int
    lib.tt_sparse_max_probes.restype = ctypes.c_int
    lib.tt_launch_scan_extrema_sparse.argtypes = [P, I64, P, P, I32, P, I32, P, P, I32, I32, P, P, P, P, I64, P, I32, P]
    lib.tt_launch_scan_extrema_sparse.restype = ctypes.c_int
    lib.tt_launch_scan_sums_sparse.argtypes = [P, I64, P, P, I32, P, I32, P, P, I32, I32, P, I64, P, P, P, P, I64, P,
                                               I32, P]
    lib.tt_launch_scan_sums_sparse.restype = ctypes.c_int
    lib.tt_launch_sort_keys.argtypes = [P, P, I64, P, I32, P, I32, P, I32, P, P, I32, P]
    lib.tt_launch_sort_keys.restype = ctypes.c_int
    lib.tt_sort_max_keys.restype = ctypes.c_int
    lib.tt_launch_select_le_bin.argtypes = [P, P, I64, I32, ctypes.c_uint32, P, P, P, ctypes.c_uint32, P]
    lib.tt_launch_select_le_bin.restype = ctypes.c_int
    lib.tt_hist_bins.restype = ctypes.c_int
    lib.tt_launch_rank_encode.argtypes = [P, P, I32, I64, I64, P, I32, P]
    lib.tt_launch_rank_encode.restype = ctypes.c_int
    lib.tt_page_cap.restype = ctypes.c_int
    lib.tt_launch_page_reset.argtypes = [P, P]
    lib.tt_launch_page_topk.argtypes = [P, P, P, I32, I32, ctypes.c_uint64, P, P, P, P]
    lib.tt_launch_page_topk.restype = ctypes.c_int
    lib.tt_launch_page_reset.restype = ctypes.c_int
    lib.tt_launch_zone_argmin.argtypes = [P, I64, P, P, I32, P, P, I32, P, I32, P, P]
    lib.tt_launch_zone_argmin.restype = ctypes.c_int
    lib.tt_launch_page.argtypes = [P, I64, P, P, I32, P, I32, P, I32, P, P, I32, P, I32, P, P, P, I32, I32,
                                   ctypes.c_uint64, P, P, P]
    lib.tt_launch_page.restype = ctypes.c_int
    lib.tt_launch_scatter_segments.argtypes = [P, I64, I32, I64, P]
    lib.tt_launch_scatter_segments.restype = ctypes.c_int
    lib.tt_host_alloc.argtypes = [I64]
    lib.tt_host_alloc.restype = ctypes.c_void_p
    lib.tt_host_device_ptr.argtypes = [P]
    lib.tt_host_device_ptr.restype = ctypes.c_void_p
    lib.tt_host_free.argtypes = [P]
    lib.tt_host_free.restype = ctypes.c_int
    lib.tt_stream_sync.argtypes = [P]
    lib.tt_stream_sync.restype = ctypes.c_int
    lib.tt_tile_rows.restype = ctypes.c_int
    lib.tt_max_depth.restype = ctypes.c_int
    lib.tt_max_lds_bitmap_words.restype = ctypes.c_int
    lib.tt_max_lds_ranks.restype = ctypes.c_int
    lib.tt_max_lds_groups.restype = ctypes.c_int
    lib.tt_lds_rank_words.restype = ctypes.c_int
    _lib = lib
    return lib


class GpuKernels:
    def __init__(self, device: Any = None) -> None:
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("no HIP device available")
        self.torch = torch
        self.lib = load_library()
        self.device = torch.device(device or "cuda")
        self.tile_rows = int(self.lib.tt_tile_rows())
        self.max_depth = int(self.lib.tt_max_depth())
        self.max_sort_keys = int(self.lib.tt_sort_max_keys())
        # the pinned total, its event and the cached scratch buffers are shared by every caller
        # of this object (queries of different collections run on different threads): one
        # select at a time
        self._total_lock = threading.Lock()
        self._bufs: dict[str, Any] = {}
        self._est: dict[int, int] = {}  # last selection count per device program: output sizing
        self.page_cap = int(self.lib.tt_page_cap())
        # every launch goes to the device's current stream at construction (the default stream:
        # nothing here switches streams); resolved once -- torch.cuda.current_stream costs
        # microseconds of device-index lookups per call, several calls per query
        self._tstream = torch.cuda.current_stream(self.device)
        self._stream_handle = ctypes.c_void_p(self._tstream.cuda_stream)
        # staging slots of ``upload`` and the event recorded after the scatter that last read each
        self._upload_ev: list[Any] = [None] * self.UPLOAD_SLOTS
        self._upload_slot = 0

    UPLOAD_SLOTS = 4
    # made on first use (declared on the class: the sort-fault test builds a bare object)
    _pinned_total = _total_event = None  # ``select``'s pinned row count and its event
    _sort_temp = _sort_fault = None      # ``_sorted_rows``' scratch and look-back fault word

    def _stream(self) -> ctypes.c_void_p:
        return self._stream_handle

    def select(self, table, live16, capacity: int, nrows: int, prog, bitmaps, return_mask: bool = False):
        """Row indices (int32, ascending) of live rows satisfying ``prog``.

        ``table``: int64 [ncols, 2] of (device pointer, width) column descriptors, every column
        allocated for ``capacity`` rows (a multiple of the kernel tile); ``live16``: uint16 liveness
        bits for ``capacity`` rows."""
        torch = self.torch
        tiles = (nrows + self.tile_rows - 1) // self.tile_rows
        if tiles == 0:
            empty = torch.empty(0, dtype=torch.int32, device=self.device)
            return (empty, None) if return_mask else empty
        self._check_scan_args(table, live16, capacity, nrows, prog)
        with self._total_lock:  # also guards the cached scratch buffers
            nmask = tiles * self.tile_rows // 16
            mask = (torch.empty(nmask, dtype=torch.int16, device=self.device) if return_mask
                    else self._buf("mask", nmask, torch.int16))
            counts = self._buf("counts", tiles, torch.int32)
            stream = self._stream()
            rc = self.lib.tt_launch_scan_eval(table.data_ptr(), nrows, live16.data_ptr(), prog.data_ptr(),
                                              prog.shape[0], bitmaps.data_ptr(), bitmaps.numel(),
                                              mask.data_ptr(), counts.data_ptr(), stream)
            if rc != 0:
                raise RuntimeError(f"tt_scan_eval launch failed ({rc})")
            # the tiles' output offsets in one block (tt_tile_offsets, which also writes the total
            # straight into pinned host memory), then the wave-independent compaction: no torch
            # launches, no host sync between the kernels -- one event wait at the end.  The ids go
            # into a fresh buffer the caller owns, sized from the previous count of this program
            # (+12.5 %); when the selection grew past it, the compaction alone runs again into an
            # exact one (no full-collection buffer held by a result, no copy of the ids).
            key = prog.data_ptr()
            est = self._est.get(key)
            cap = nrows if est is None else min(nrows, est + est // 8 + 4096)
            out = torch.empty(max(cap, 1), dtype=torch.int32, device=self.device)
            # [0] = total (int64), byte 16 on: int32 tile offsets
            scratch = self._buf("scratch", tiles // 2 + 3, torch.int64)
            pinned = self._pinned()
            rc = self.lib.tt_launch_scan_compact(mask.data_ptr(), counts.data_ptr(), scratch.data_ptr() + 16, nrows,
                                                 out.data_ptr(), cap, scratch.data_ptr(), pinned.data_ptr(), stream)
            if rc != 0:
                raise RuntimeError(f"tt_scan_compact launch failed ({rc})")
            self._total_event.record(self._tstream)
            self._total_event.synchronize()
            total = int(pinned[0])
            if total > cap:
                out = torch.empty(max(total, 1), dtype=torch.int32, device=self.device)
                rc = self.lib.tt_launch_compact(mask.data_ptr(), scratch.data_ptr() + 16, nrows, out.data_ptr(),
                                                total, stream)
                if rc != 0:
                    raise RuntimeError(f"tt_scan_compact launch failed ({rc})")
            if len(self._est) > 256:
                self._est.clear()
            self._est[key] = total
            out = out[:total]
        return (out, mask) if return_mask else out

    def _check_scan_args(self, table, live16, capacity: int, nrows: int, prog) -> None:
        torch = self.torch
        if capacity % self.tile_rows or nrows > capacity:
            raise ValueError("column capacity must be a multiple of the tile and >= nrows")
        if live16.dtype != torch.int16 or live16.numel() * 16 < capacity:
            raise ValueError("liveness mask must be int16 bits covering the capacity")
        if table.dtype != torch.int64 or table.ndim != 2 or table.shape[1] != 2:
            raise ValueError("column table must be int64 [ncols, 2]")
        if prog.dtype != torch.int32 or prog.ndim != 2 or prog.shape[1] != 4:
            raise ValueError("program must be int32 [L, 4]")

    def _buf(self, name: str, n: int, dtype):
        """Cached device scratch of at least ``n`` elements (caller holds ``_total_lock``)."""
        t = self._bufs.get(name)
        if t is None or t.numel() < n or t.dtype != dtype:
            t = self._bufs[name] = self.torch.empty(max(n, 1), dtype=dtype, device=self.device)
        return t

    def _pinned(self):
        p = self._pinned_total
        if p is None:
            p = self._pinned_total = self.torch.zeros(1, dtype=self.torch.int64, pin_memory=True)
            self._total_event = self.torch.cuda.Event()
        return p

    def rank_encode(self, src_desc, rank_table, lo: int, hi: int, dst, width: int) -> None:
        """dst[lo:hi] = sort rank of each row's dictionary id (``hip/query_scan.hip`` tt_rank_encode);
        ``src_desc`` is the source column's 16-byte row of the column table."""
        rc = self.lib.tt_launch_rank_encode(src_desc.data_ptr(), rank_table.data_ptr(), rank_table.numel(), lo, hi,
                                            dst.data_ptr(), width, self._stream())
        if rc != 0:
            raise RuntimeError(f"tt_rank_encode launch failed ({rc})")

    # -- paged ordered queries (hip/page_topk.hip) -------------------------------------------
    def _mailbox(self, name: str, n: int):
        """Pinned, coherent, device-mapped host int32 array of at least ``n`` elements (caller
        holds ``_total_lock``): the page kernels read their tile list from it and write their
        answer into it, so a page query moves no data through copy kernels."""
        mb = self._bufs.get(name)
        if mb is None or mb[2].size < n:
            if mb is not None:
                self.lib.tt_host_free(ctypes.c_void_p(mb[0]))
            size = max(1024, 1 << max(0, int(n) - 1).bit_length())
            host = self.lib.tt_host_alloc(4 * size)
            dev = self.lib.tt_host_device_ptr(ctypes.c_void_p(host)) if host else None
            if not host or not dev:
                raise RuntimeError("pinned host mailbox allocation failed")
            arr = np.ctypeslib.as_array((ctypes.c_int32 * size).from_address(host))
            mb = self._bufs[name] = (host, dev, arr)
        return mb

    uploads = 0  # scatter launches (one per mirror sync)
    upload_segments = 0

    def upload(self, segments) -> None:
        """Write ``segments`` -- [(device address, host numpy array)] -- to the device in ONE
        kernel launch (``hip/mirror_upload.hip`` tt_scatter_segments): the payloads and their
        segment table are staged in a pinned, device-mapped mailbox the kernel reads directly,
        instead of one copy (copyBuffer + DMA set-up) per segment.  Stream-ordered with every
        other launch of this process (the current stream)."""
        segs = [(int(d), np.ascontiguousarray(a).view(np.uint8).reshape(-1)) for d, a in segments if a.size]
        if not segs:
            return
        table = (24 * len(segs) + 15) & ~15
        offs, at = [], table
        for _, b in segs:
            offs.append(at)
            at += (b.size + 15) & ~15
        with self._total_lock:
            stream = self._stream()
            # a ring of staging slots: the scatter that last read this slot has finished before
            # its bytes change or it is replaced -- its event, not a whole-stream synchronise
            # (which would wait for every kernel queued since, once per upload)
            slot = self._upload_slot
            self._upload_slot = (slot + 1) % self.UPLOAD_SLOTS
            ev = self._upload_ev[slot]
            if ev is not None and not ev.query():
                ev.synchronize()
            host, dev, arr = self._mailbox(f"upload{slot}", (at + 3) // 4)
            buf = arr.view(np.uint8)
            desc = np.empty((len(segs), 3), dtype=np.int64)
            for i, ((d, b), o) in enumerate(zip(segs, offs)):
                buf[o:o + b.size] = b
                desc[i] = (o, d, b.size)
            buf[:24 * len(segs)] = desc.view(np.uint8).reshape(-1)
            rc = self.lib.tt_launch_scatter_segments(ctypes.c_void_p(dev), 0, len(segs),
                                                     max(b.size for _, b in segs), stream)
            if rc != 0:
                raise RuntimeError(f"tt_scatter_segments launch failed ({rc})")
            if ev is None:
                ev = self._upload_ev[slot] = self.torch.cuda.Event()
            ev.record(self._tstream)
            self.uploads += 1
            self.upload_segments += len(segs)

    def _sync(self, stream) -> None:
        rc = self.lib.blocking_sync(stream)  # GIL released while waiting (see load_library)
        if rc != 0:
            raise RuntimeError(f"stream synchronise failed ({rc})")

    def zone_argmin(self, table, live16, nrows: int, specs, ranks, seq, seq_bits: int, tiles):
        """Per listed tile (numpy int32), the live row with the smallest packed key (-1: none)."""
        n = len(tiles)
        with self._total_lock:
            _, tdev, tarr = self._mailbox("zone_tiles", n)
            _, odev, oarr = self._mailbox("zone_out", n)
            tarr[:n] = tiles
            stream = self._stream()
            rc = self.lib.tt_launch_zone_argmin(table.data_ptr(), nrows, live16.data_ptr(), specs.data_ptr(),
                                                specs.shape[0], ranks.data_ptr(), seq.data_ptr(), seq_bits,
                                                tdev, n, odev, stream)
            if rc != 0:
                raise RuntimeError(f"tt_zone_argmin launch failed ({rc})")
            self._sync(stream)
            return oarr[:n].copy()

    def page(self, table, live16, nrows: int, prog, bitmaps, specs, ranks, seq, seq_bits: int, tiles, k: int,
             offset: int, bound: int):
        """The rows [offset, k) of the key order among the matches in ``tiles`` (numpy int32), and
        (candidates, complete): see hip/page_topk.hip."""
        torch = self.torch
        if not 0 < k <= self.page_cap or not 0 <= offset <= k:
            raise ValueError("page outside the device top-k capacity")
        n = len(tiles)
        with self._total_lock:
            _, tdev, tarr = self._mailbox("page_tiles", n)
            _, odev, oarr = self._mailbox("page_out", 4 + self.page_cap)
            tarr[:n] = tiles
            ck = self._buf("page_keys", self.page_cap, torch.int64)
            cr = self._buf("page_rows", self.page_cap, torch.int32)
            stream = self._stream()
            if "page_counter" not in self._bufs:  # zeroed once; tt_page_topk resets it after each query
                self._bufs["page_counter"] = torch.empty(1, dtype=torch.int32, device=self.device)
                if self.lib.tt_launch_page_reset(self._bufs["page_counter"].data_ptr(), stream) != 0:
                    raise RuntimeError("tt_page_reset launch failed")
            rc = self.lib.tt_launch_page(table.data_ptr(), nrows, live16.data_ptr(), prog.data_ptr(), prog.shape[0],
                                         bitmaps.data_ptr(), bitmaps.numel(), specs.data_ptr(), specs.shape[0],
                                         ranks.data_ptr(), seq.data_ptr(), seq_bits, tdev, n,
                                         ck.data_ptr(), cr.data_ptr(), self._bufs["page_counter"].data_ptr(), k,
                                         offset, ctypes.c_uint64(bound), odev, odev + 16, stream)
            if rc != 0:
                raise RuntimeError(f"tt_page launch failed ({rc})")
            self._sync(stream)
            total, complete, written = int(oarr[0]), bool(oarr[1]), int(oarr[2])
            return oarr[4:4 + written].copy(), total, complete

    def page_topk(self, cand_keys, cand_rows, k: int, offset: int, bound: int, stamps=None):
        """``tt_page_topk`` alone over caller-filled device candidates (uint64 keys as int64,
        int32 rows; their number = ``cand_keys.numel()``): (rows [offset, k) of the key order,
        info [total, complete, written]).  ``stamps``: an int64 device tensor of 6 that gets
        the kernel's shader clock at its phase boundaries.  For the kernel tests."""
        torch = self.torch
        n = int(cand_keys.numel())
        if n > self.page_cap or cand_rows.numel() != n:
            raise ValueError("candidates exceed the top-k capacity")
        with self._total_lock:
            counter = torch.tensor([n], dtype=torch.int32, device=self.device)
            _, odev, oarr = self._mailbox("topk_out", 4 + self.page_cap)
            stream = self._stream()
            rc = self.lib.tt_launch_page_topk(cand_keys.data_ptr(), cand_rows.data_ptr(), counter.data_ptr(), k,
                                              offset, ctypes.c_uint64(bound), odev, odev + 16,
                                              None if stamps is None else stamps.data_ptr(), stream)
            if rc != 0:
                raise RuntimeError(f"tt_page_topk launch failed ({rc})")
            self._sync(stream)
            info = oarr[:3].copy()
            return oarr[4:4 + int(info[2])].astype(np.int32), info

    def group_count(self, table, g: int, mask, nrows: int, ngroups: int):
        torch = self.torch
        counts = torch.zeros(max(ngroups, 1), dtype=torch.int32, device=self.device)
        rc = self.lib.tt_launch_group_count(table.data_ptr(), g, mask.data_ptr(), nrows, max(ngroups, 1),
                                            counts.data_ptr(), self._stream())
        if rc != 0:
            raise RuntimeError(f"tt_group_count launch failed ({rc})")
        return counts[:ngroups]

    def _group_args(self, table, live16, capacity: int, nrows: int, prog, keys, dims, max_keys: int, what: str,
                    value_col=None, out=None, fills=None, dense: bool = True):
        """What the grouped scans check alike: the scan's own arguments, ``keys`` / ``dims`` (at
        most ``max_keys``, called ``what`` in a refusal) and ``value_col`` against ``table``.
        Returns (keys, dims, cells, the device's cell limit, outputs): with ``fills`` the (int32,
        int64, int64) triple of one element per cell, ``out`` checked or a new one so filled.
        ``dense=False`` (the hashed scans, whose outputs follow their slots): the limit is the
        2^62 cells a 64-bit cell takes, not ``tt_group_max_cells()``."""
        torch = self.torch
        keys, dims = [int(x) for x in keys], [int(x) for x in dims]
        if len(keys) != len(dims) or len(keys) > max_keys:
            raise ValueError(f"at most {max_keys} {what} columns, one dictionary size each")
        self._check_scan_args(table, live16, capacity, nrows, prog)
        if any(not 0 <= c < table.shape[0] for c in keys) or any(d < 0 for d in dims):
            raise ValueError(f"{what} columns must be rows of the column table, dictionary sizes >= 0")
        if value_col is not None and not 0 <= value_col < table.shape[0]:
            raise ValueError("the value column must be a row of the column table")
        ncells = 1
        for d in dims:
            ncells *= d + 1
        limit = int(self.lib.tt_group_max_cells()) if dense else (1 << 62) - 1
        n = min(ncells, limit)
        dtypes = (torch.int32, torch.int64, torch.int64)
        if fills is not None and out is None:
            out = tuple(torch.full((n,), f, dtype=t, device=self.device) if f else
                        torch.zeros(n, dtype=t, device=self.device) for f, t in zip(fills, dtypes))
        elif fills is not None and (len(out) != 3 or any(o.dtype != t or o.numel() < n for o, t in zip(out, dtypes))):
            raise ValueError("outputs must be (int32, int64, int64), one element per cell")
        return keys, dims, ncells, limit, out

    def scan_group(self, table, live16, capacity: int, nrows: int, prog, bitmaps, keys, dims, max_blocks: int = 0,
                   counts=None):
        """Histogram (device int32 holding uint32 counts, ``prod(dims[i] + 1)`` cells) of the key
        columns' dictionary ids over the live rows satisfying ``prog``: filter and histogram in
        one pass (``hip/group_agg.hip`` tt_scan_group).  ``keys``: up to 3 rows of ``table``;
        ``dims``: their dictionary sizes, slot ``dims[i]`` of axis i counting the rows where the
        path is missing; ids at or past ``dims[i]`` are dropped.  ``table`` / ``live16`` /
        ``capacity`` as for ``select``.  ``counts``: a zeroed tensor to add into instead of a
        new one.  ValueError when the cells exceed ``tt_group_max_cells()``."""
        torch = self.torch
        keys, dims, ncells, limit, _ = self._group_args(table, live16, capacity, nrows, prog, keys, dims, 3, "key")
        if counts is None:
            counts = torch.zeros(min(ncells, limit), dtype=torch.int32, device=self.device)
        elif counts.dtype != torch.int32 or counts.numel() < min(ncells, limit):
            raise ValueError("counters must be int32, one per cell")
        n = len(keys)
        rc = self.lib.tt_launch_scan_group(table.data_ptr(), nrows, live16.data_ptr(), prog.data_ptr(), prog.shape[0],
                                           bitmaps.data_ptr(), bitmaps.numel(), (ctypes.c_int32 * 3)(*keys),
                                           (ctypes.c_int32 * 3)(*dims), n, counts.data_ptr(), max_blocks,
                                           self._stream())
        if rc == -2:
            raise ValueError(f"{ncells} histogram cells exceed the device limit of {limit}")
        if rc != 0:
            raise RuntimeError(f"tt_scan_group launch failed ({rc})")
        return counts

    extrema_scans = 0  # tt_scan_extrema launches

    def scan_extrema(self, table, live16, capacity: int, nrows: int, prog, bitmaps, keys, dims, value_col: int,
                     max_blocks: int = 0, out=None):
        """Per group cell, over the live rows satisfying ``prog`` whose value is defined: (counts
        int32 holding uint32, lo int64, hi int64 holding uint64), ``lo`` / ``hi`` the smallest and
        the largest ``code << 32 | row`` of the value column -- filter and reduction in one pass
        (``hip/group_extrema.hip`` tt_scan_extrema).  ``keys`` / ``dims``: up to 2 group columns
        and their dictionary sizes, cells as for ``scan_group``; ``value_col``: the row of
        ``table`` whose codes are compared as unsigned integers (a rank-encoded copy), its
        all-ones code = undefined.  ``lo`` / ``hi`` of a cell mean something only where its count
        is not 0.  ``out``: a (counts, lo, hi) triple initialised to 0 / -1 / 0 to reduce into
        instead of a new one.  ValueError when the cells exceed ``tt_group_max_cells()``."""
        value_col = int(value_col)
        keys, dims, ncells, limit, out = self._group_args(table, live16, capacity, nrows, prog, keys, dims, 2, "group",
                                                          value_col, out, (0, -1, 0))
        if nrows > 1 << 32:
            raise ValueError("rows past 2^32 do not fit next to the code")
        rc = self.lib.tt_launch_scan_extrema(table.data_ptr(), nrows, live16.data_ptr(), prog.data_ptr(),
                                             prog.shape[0], bitmaps.data_ptr(), bitmaps.numel(),
                                             (ctypes.c_int32 * 2)(*keys), (ctypes.c_int32 * 2)(*dims), len(keys),
                                             value_col, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(),
                                             max_blocks, self._stream())
        if rc == -2:
            raise ValueError(f"{ncells} group cells exceed the device limit of {limit}")
        if rc != 0:
            raise RuntimeError(f"tt_scan_extrema launch failed ({rc})")
        self.extrema_scans += 1
        return out

    sum_scans = 0  # tt_scan_sums launches

    def scan_sums(self, table, live16, capacity: int, nrows: int, prog, bitmaps, keys, dims, value_col: int, nums,
                  max_blocks: int = 0, out=None):
        """Per group cell, over the live rows satisfying ``prog`` whose value is a number: (nums
        int32 holding uint32, sum int64, abs int64 holding uint64) -- how many, the sum of their
        scaled integers ``m`` and the sum of ``|m|``, filter and sums in one pass
        (``hip/group_sums.hip`` tt_scan_sums).  ``keys`` / ``dims``: up to 2 group columns and
        their dictionary sizes, cells as for ``scan_group``; ``value_col``: the row of ``table``
        with the key's dictionary ids; ``nums``: device int64, the ``m`` of every id
        (``Column.num_scale``), INT64_MIN where the value is no number; ids at or past its size
        add nothing.  Integer atomics: the same buffers on every run.  ``out``: a zeroed (nums,
        sum, abs) triple to add into instead of a new one.  ValueError when the cells exceed
        ``tt_group_max_cells()``."""
        torch = self.torch
        value_col = int(value_col)
        keys, dims, ncells, limit, out = self._group_args(table, live16, capacity, nrows, prog, keys, dims, 2, "group",
                                                          value_col, out, (0, 0, 0))
        if nrows > 1 << 32:
            raise ValueError("rows past 2^32 do not fit a cell's count")
        if nums.dtype != torch.int64 or nums.ndim != 1 or not nums.is_contiguous() or nums.numel() > 1 << 31:
            raise ValueError("the number table must be contiguous int64, one entry per dictionary id")
        rc = self.lib.tt_launch_scan_sums(table.data_ptr(), nrows, live16.data_ptr(), prog.data_ptr(),
                                          prog.shape[0], bitmaps.data_ptr(), bitmaps.numel(),
                                          (ctypes.c_int32 * 2)(*keys), (ctypes.c_int32 * 2)(*dims), len(keys),
                                          value_col, nums.data_ptr() if nums.numel() else None, nums.numel(),
                                          out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(),
                                          max_blocks, self._stream())
        if rc == -2:
            raise ValueError(f"{ncells} group cells exceed the device limit of {limit}")
        if rc != 0:
            raise RuntimeError(f"tt_scan_sums launch failed ({rc})")
        self.sum_scans += 1
        return out

    sparse_scans = 0  # tt_scan_sparse / tt_scan_extrema_sparse / tt_scan_sums_sparse launches

    def _sparse_args(self, table, live16, capacity: int, nrows: int, prog, keys, dims, max_keys: int, what: str,
                     slots: int, value_col=None):
        """The hashed scans' checks (``_group_args`` without the dense limit, ``slots`` a power of
        two) and their table: (keys, dims, cells, table keys set to all-ones, a zeroed status word)."""
        torch = self.torch
        keys, dims, ncells, limit, _ = self._group_args(table, live16, capacity, nrows, prog, keys, dims, max_keys,
                                                        what, value_col, dense=False)
        slots = int(slots)
        if slots < 2 or slots > 1 << 31 or slots & (slots - 1):
            raise ValueError("the hash table takes a power of two of slots, 2 to 2^31")
        if nrows > 1 << 32:
            raise ValueError("rows past 2^32 do not fit a cell's count")
        if ncells > limit:
            raise ValueError(f"{ncells} group cells do not fit a 64-bit cell")
        return (keys, dims, ncells, torch.full((slots,), -1, dtype=torch.int64, device=self.device),
                torch.zeros(1, dtype=torch.int32, device=self.device))

    def _sparse_result(self, table_keys, status, counts, *words):
        """The occupied slots of a hashed scan, compacted on the device and sorted by cell: (cells
        int64, counts, each of ``words``); None when the scan set ``status`` (a probe reached its
        bound: the table was too full and rows were dropped)."""
        torch = self.torch
        self.sparse_scans += 1
        if int(status.item()):
            return None
        slots = torch.nonzero(counts).flatten()
        cells, order = torch.sort(table_keys[slots])
        slots = slots[order]
        return (cells, counts[slots], *(w[slots] for w in words))

    def scan_sparse(self, table, live16, capacity: int, nrows: int, prog, bitmaps, keys, dims, slots: int,
                    max_blocks: int = 0):
        """The histogram of ``scan_group`` for a cell space of any size below 2^62, through a hash
        table of ``slots`` slots (a power of two) in device memory (``hip/group_sparse.hip``
        tt_scan_sparse): (cells int64 ascending, counts int32 holding uint32) of the cells that
        occur, both on the device; cells as ``scan_group``'s, in 64 bits.  None when the table
        was too full for the cells that occur (``slots`` of at least twice their number never
        is)."""
        keys, dims, _, tkeys, status = self._sparse_args(table, live16, capacity, nrows, prog, keys, dims, 3, "key",
                                                         slots)
        counts = self.torch.zeros(int(slots), dtype=self.torch.int32, device=self.device)
        rc = self.lib.tt_launch_scan_sparse(table.data_ptr(), nrows, live16.data_ptr(), prog.data_ptr(),
                                            prog.shape[0], bitmaps.data_ptr(), bitmaps.numel(),
                                            (ctypes.c_int32 * 3)(*keys), (ctypes.c_int32 * 3)(*dims), len(keys),
                                            tkeys.data_ptr(), counts.data_ptr(), int(slots), status.data_ptr(),
                                            max_blocks, self._stream())
        if rc != 0:
            raise RuntimeError(f"tt_scan_sparse launch failed ({rc})")
        return self._sparse_result(tkeys, status, counts)

    def scan_extrema_sparse(self, table, live16, capacity: int, nrows: int, prog, bitmaps, keys, dims,
                            value_col: int, slots: int, max_blocks: int = 0):
        """``scan_extrema`` for a group space of any size below 2^62, through a hash table of
        ``slots`` slots (``hip/group_extrema.hip`` tt_scan_extrema_sparse): (cells int64
        ascending, counts, lo, hi) of the cells with a defined value, on the device; None when
        the table was too full."""
        value_col = int(value_col)
        keys, dims, _, tkeys, status = self._sparse_args(table, live16, capacity, nrows, prog, keys, dims, 2, "group",
                                                         slots, value_col)
        torch, n = self.torch, int(slots)
        out = (torch.zeros(n, dtype=torch.int32, device=self.device),
               torch.full((n,), -1, dtype=torch.int64, device=self.device),
               torch.zeros(n, dtype=torch.int64, device=self.device))
        rc = self.lib.tt_launch_scan_extrema_sparse(table.data_ptr(), nrows, live16.data_ptr(), prog.data_ptr(),
                                                    prog.shape[0], bitmaps.data_ptr(), bitmaps.numel(),
                                                    (ctypes.c_int32 * 2)(*keys), (ctypes.c_int32 * 2)(*dims),
                                                    len(keys), value_col, out[0].data_ptr(), out[1].data_ptr(),
                                                    out[2].data_ptr(), tkeys.data_ptr(), n, status.data_ptr(),
                                                    max_blocks, self._stream())
        if rc != 0:
            raise RuntimeError(f"tt_scan_extrema_sparse launch failed ({rc})")
        return self._sparse_result(tkeys, status, *out)

    def scan_sums_sparse(self, table, live16, capacity: int, nrows: int, prog, bitmaps, keys, dims, value_col: int,
                         nums, slots: int, max_blocks: int = 0):
        """``scan_sums`` for a group space of any size below 2^62, through a hash table of
        ``slots`` slots (``hip/group_sums.hip`` tt_scan_sums_sparse): (cells int64 ascending,
        nums, sum, abs) of the cells that hold a number, on the device; None when the table was
        too full."""
        value_col = int(value_col)
        keys, dims, _, tkeys, status = self._sparse_args(table, live16, capacity, nrows, prog, keys, dims, 2, "group",
                                                         slots, value_col)
        torch, n = self.torch, int(slots)
        if nums.dtype != torch.int64 or nums.ndim != 1 or not nums.is_contiguous() or nums.numel() > 1 << 31:
            raise ValueError("the number table must be contiguous int64, one entry per dictionary id")
        out = (torch.zeros(n, dtype=torch.int32, device=self.device),
               torch.zeros(n, dtype=torch.int64, device=self.device),
               torch.zeros(n, dtype=torch.int64, device=self.device))
        rc = self.lib.tt_launch_scan_sums_sparse(table.data_ptr(), nrows, live16.data_ptr(), prog.data_ptr(),
                                                 prog.shape[0], bitmaps.data_ptr(), bitmaps.numel(),
                                                 (ctypes.c_int32 * 2)(*keys), (ctypes.c_int32 * 2)(*dims), len(keys),
                                                 value_col, nums.data_ptr() if nums.numel() else None, nums.numel(),
                                                 out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(),
                                                 tkeys.data_ptr(), n, status.data_ptr(), max_blocks, self._stream())
        if rc != 0:
            raise RuntimeError(f"tt_scan_sums_sparse launch failed ({rc})")
        return self._sparse_result(tkeys, status, *out)

    def sort_keys(self, table, rows, specs, ranks, seq, seq_bits: int, hist=None, shift: int = 0):
        """Packed 63-bit ordering keys (int64) for ``rows`` (int32, device): see
        ``hip/sort_keys.hip``.  ``specs``: int32 [nkeys, 8] device tensor; ``ranks``: int32
        rank tables (concatenated); ``seq``: int32 (uint32) insertion sequence per row.  With
        ``hist`` the 12-bit radix-select histogram of key bits [shift, shift+12) is fused in."""
        torch = self.torch
        n = rows.numel()
        keys = torch.empty(max(n, 1), dtype=torch.int64, device=self.device)
        if specs.shape[0] > self.max_sort_keys:
            raise ValueError("too many sort keys for the device path")
        if seq.dtype != torch.int32 or seq_bits > 32:
            raise ValueError("device sequence must be 32-bit")
        rc = self.lib.tt_launch_sort_keys(table.data_ptr(), rows.data_ptr(), n, specs.data_ptr(), specs.shape[0],
                                          ranks.data_ptr(), ranks.numel(), seq.data_ptr(), seq_bits, keys.data_ptr(),
                                          hist.data_ptr() if hist is not None else None, shift, self._stream())
        if rc != 0:
            raise RuntimeError(f"tt_sort_keys launch failed ({rc})")
        return keys[:n]

    def order(self, table, rows, specs, ranks, seq, seq_bits: int, k: int | None = None, key_bits: int = 63):
        """Rows in result order (device int32); only the first ``k`` when given (top-k by
        radix select: histogram of the top 12 used key bits, compaction of the candidates at or
        below the k-th key's bin, sort of the candidates only)."""
        torch = self.torch
        n = rows.numel()
        if n == 0:
            return rows
        if k is not None and k < n and n > 65536:
            bins = int(self.lib.tt_hist_bins())
            shift = max(0, key_bits - (bins.bit_length() - 1))
            hist = torch.zeros(bins, dtype=torch.int32, device=self.device)
            keys = self.sort_keys(table, rows, specs, ranks, seq, seq_bits, hist, shift)
            top = self._top_k(keys, rows, k, shift, hist, key_bits)
            if top is not None:
                return top
        else:
            keys = self.sort_keys(table, rows, specs, ranks, seq, seq_bits)
        out = self._sorted_rows(keys, rows, key_bits)
        return out[:k] if k is not None else out

    def _sorted_rows(self, keys, rows, key_bits: int):
        """``rows`` ordered by ``keys`` (ascending, stable): ``tt_sort_pairs``, the LSD radix
        sort of (key, row) pairs over the key's used bits (hip/radix_pairs.hip)."""
        if rows.dtype != self.torch.int32 or keys.dtype != self.torch.int64:
            raise ValueError("the pair sort takes int64 keys and int32 rows")
        keys, rows = keys.contiguous(), rows.contiguous()
        n = keys.numel()
        end_bit = max(1, min(64, int(key_bits)))
        need = int(self.lib.tt_sort_pairs_temp_bytes(n, end_bit))
        if need < 0:
            raise RuntimeError("tt_sort_pairs: bad size or bit range")
        temp = self._sort_temp
        if temp is None or temp.numel() < need:
            temp = self._sort_temp = self.torch.empty(max(need, 1), dtype=self.torch.uint8, device=self.device)
        fault = self._sort_fault
        if fault is None:
            fault = self._sort_fault = self.torch.zeros(1, dtype=self.torch.int32, device=self.device)
        keys_out = self.torch.empty_like(keys)
        rows_out = self.torch.empty_like(rows)
        rc = self.lib.tt_sort_pairs(keys.data_ptr(), keys_out.data_ptr(), rows.data_ptr(), rows_out.data_ptr(), n,
                                    end_bit, temp.data_ptr(), need, fault.data_ptr(), self._stream())
        if rc != 0:
            raise RuntimeError(f"tt_sort_pairs failed ({rc})")
        return rows_out

    sort_faults = 0  # sorts whose output was discarded (a look-back spin timed out)

    def check_sort(self) -> bool:
        """False if a sort since the last check saw a look-back spin time out (its output is not
        trustworthy: the caller orders on the host instead).  The fault word is cleared, so one
        timeout costs one query its device ordering, not every later one.  Reads one device
        word: call it where the caller synchronises anyway."""
        fault = self._sort_fault
        if fault is None or int(fault.item()) == 0:
            return True
        fault.zero_()
        self.sort_faults += 1
        return False

    def _top_k(self, keys, rows, k: int, shift: int, hist, key_bits: int = 63):
        torch = self.torch
        n = keys.numel()
        cum = np.cumsum(hist.cpu().numpy().astype(np.int64))
        last = int(np.searchsorted(cum, k))  # first bin where the running count reaches k
        cand = int(cum[last])
        if cand > max(8 * k, 1 << 21):
            return None  # keys too concentrated in one bin: a full sort is cheaper than refining
        out_keys = torch.empty(cand, dtype=torch.int64, device=self.device)
        out_rows = torch.empty(cand, dtype=torch.int32, device=self.device)
        counter = torch.zeros(1, dtype=torch.int32, device=self.device)
        rc = self.lib.tt_launch_select_le_bin(keys.data_ptr(), rows.data_ptr(), n, shift, last, out_keys.data_ptr(),
                                              out_rows.data_ptr(), counter.data_ptr(), cand, self._stream())
        if rc != 0:
            raise RuntimeError("tt_select_le_bin launch failed")
        return self._sorted_rows(out_keys, out_rows, key_bits)[:k]

