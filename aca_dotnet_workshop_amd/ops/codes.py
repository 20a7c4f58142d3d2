"""The formats the host index, its device mirror and the kernels share (``hip/scan_common.h``):
the compiled program's opcodes, the kernel tile, and the column code layout.

Code layout: a column holds one code per row in 2 bits (four rows per byte, row r in bits
2(r mod 4)), 1, 2 or 4 bytes -- ``width`` 0, 1, 2, 4.  The all-ones code of the width means
"path missing" (-1 at width 4).
"""
from __future__ import annotations

import numpy as np

OP_LEAF, OP_AND, OP_OR, OP_NOT, OP_TRUE, OP_EQ, OP_RANGE = 1, 2, 3, 4, 5, 6, 7
TILE = 8192           # rows per kernel tile (ops/hip/scan_common.h kTileRows)
MAX_DEPTH = 8         # device stack depth (16-bit masks in a 128-bit register)

_DTYPE = {1: np.uint8, 2: np.uint16, 4: np.int32}


def width_for(dict_size: int) -> int:
    """Code width of a column whose dictionary has ``dict_size`` ids (all-ones = missing):
    0 = 2 bits per row (<= 3 ids: booleans, with or without null), else bytes per row."""
    return 0 if dict_size <= 3 else 1 if dict_size <= 254 else 2 if dict_size <= 65534 else 4


def col_bytes(rows: int, width: int) -> int:
    return rows // 4 if width == 0 else rows * width


def torch_dtype(torch, width: int):
    """The tensor type of a 1-, 2- or 4-byte code column (torch's 16-bit integers are signed:
    the same bits)."""
    return getattr(torch, np.dtype(_DTYPE[width]).name.replace("uint16", "int16"))


def encode_codes(values: np.ndarray, width: int) -> np.ndarray:
    """``values`` (ids or ranks, < 0 = missing) as codes of ``width``; width 0 packs four rows
    per byte (``values.size`` a multiple of 4)."""
    if width == 4:
        return values.astype(np.int32, copy=False)
    if width == 0:
        c = np.where(values < 0, 3, values).astype(np.uint8).reshape(-1, 4)
        return c[:, 0] | (c[:, 1] << 2) | (c[:, 2] << 4) | (c[:, 3] << 6)
    dt = _DTYPE[width]
    return np.where(values < 0, np.iinfo(dt).max, values).astype(dt)


def gather(table: np.ndarray, ids: np.ndarray, missing: int) -> np.ndarray:
    """``table[ids]``, ``missing`` where the id is (< 0)."""
    return np.where(ids >= 0, table[np.maximum(ids, 0)] if table.size else missing, missing)
