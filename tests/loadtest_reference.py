"""numpy references for the load self-test (``cpp/loadtest_kernels.hpp`` and
``cpp/loadtest_core.hpp``).

numpy only and no GPU import: ``test_load_selftest`` checks this module on
the CPU, ``test_load_selftest_gpu`` compares the kernels with it.

A is ``[M][K]``, B is kept transposed as ``[N][K]``; C is ``[M][N]`` float32.
Operand values are ``v * 2^e``, integer ``v`` in [-8, 8] and ``e`` in
{-1, 0, 1}. Everything here is computed in integers: operands in units of
2^-1, products and sums in units of 2^-2.
"""

import numpy as np

import cutest_reference as C
import hip_reference as R
import selftest_reference as S

TILE = 128
BK = 64
MAX_K = 8192
BATCH = 8
POISON = 0xFFFFFFFF
RECORD_BYTES = 16  # (hw_id, xcc_id, tile, 0) uint32
MAX_RECORDS = S.MAX_RECORDS

_M64 = (1 << 64) - 1


def half_units(seed, which, rows, k):
    """Operand ``which`` (0 = A, 1 = B^T) as a ``(rows, k)`` int64 array in
    units of 2^-1, from the key ``which << 56 | row << 28 | k``."""
    r = np.arange(rows, dtype=np.uint64)[:, None]
    c = np.arange(k, dtype=np.uint64)[None, :]
    key = (np.uint64(which) << np.uint64(56)) | (r << np.uint64(28)) | c
    with np.errstate(over="ignore"):
        h = S.mix(key + np.uint64(seed & _M64))
    v = (h % np.uint64(17)).astype(np.int64) - 8
    e = ((h >> np.uint64(32)) % np.uint64(3)).astype(np.int64)  # e + 1
    return v * (1 << e)


def values(units):
    """float64 values of half units."""
    return np.asarray(units, dtype=np.float64) * 0.5


def bits_of(units):
    """bf16 bit patterns (uint16) of half units; raises if one is not exact."""
    return R.bf16_bits(values(units))


def units_of(bits):
    """Half units of bf16 bit patterns; raises if one is not a multiple of
    2^-1."""
    v = R.bf16_value(np.asarray(bits, dtype=np.uint16)).astype(np.float64) * 2
    if (v != np.rint(v)).any():
        raise ValueError("an operand is not a multiple of 2^-1")
    return v.astype(np.int64)


def gemm_units(a_units, bt_units):
    """``A @ B`` in int64 units of 2^-2. The product is formed in float64,
    where it is exact (every sum is far below 2^53), because numpy multiplies
    float matrices much faster than integer ones."""
    a = np.asarray(a_units, dtype=np.int64)
    bt = np.asarray(bt_units, dtype=np.int64)
    assert np.abs(a).max() <= 256 and np.abs(bt).max() <= 256
    return np.rint(a.astype(np.float64) @ bt.astype(np.float64).T).astype(np.int64)


def to_f32(c_units):
    """Units of 2^-2 as float32; raises when one does not fit 24 bits."""
    c_units = np.asarray(c_units, dtype=np.int64)
    if (np.abs(c_units) > (1 << 24)).any():
        raise ValueError("a sum is not exact in float32")
    return (c_units.astype(np.float64) * 0.25).astype(np.float32)


def gemm_f32(a_units, bt_units):
    return to_f32(gemm_units(a_units, bt_units))


def checksum(a_units, bt_units):
    """Row sums ``A (B 1)`` and column sums ``(1^T A) B`` of C in units of
    2^-2, without forming C."""
    a = np.asarray(a_units, dtype=np.int64)
    bt = np.asarray(bt_units, dtype=np.int64)
    return a @ bt.sum(axis=0), bt @ a.sum(axis=0)


def tile_of(row, col, n):
    return (row // TILE) * (n // TILE) + col // TILE


def expected_mismatches(got, want):
    """``{(row, col, got_bits, want_bits)}`` where two float32 C differ in
    their bits."""
    g = np.ascontiguousarray(got, dtype=np.float32).view(np.uint32)
    w = np.ascontiguousarray(want, dtype=np.float32).view(np.uint32)
    return {
        (int(r), int(c), int(g[r, c]), int(w[r, c]))
        for r, c in zip(*np.nonzero(g != w))
    }


def bad_tiles(mismatches, n, iterations=1):
    """The sorted ``[(tile_row, tile_col, mismatches)]`` of a mismatch set
    that every one of ``iterations`` iterations reports."""
    count = {}
    for row, col, _, _ in mismatches:
        key = (row // TILE, col // TILE)
        count[key] = count.get(key, 0) + iterations
    return [(tr, tc, c) for (tr, tc), c in sorted(count.items())]


def parse_tile_records(records_bytes, tiles):
    """``(iterations, tiles, 4)`` uint32 from the records' bytes (no
    guards)."""
    assert len(records_bytes) % (RECORD_BYTES * tiles) == 0
    return np.frombuffer(bytes(records_bytes), dtype="<u4").reshape(-1, tiles, 4)


def bad_cus(records, per_tile):
    """The sorted ``bad_cus`` list from tile records ``(iterations, tiles,
    4)`` and ``{tile: mismatches per iteration}``."""
    count = {}
    for it in range(records.shape[0]):
        for tile, bad in per_tile.items():
            hw, xcc = int(records[it, tile, 0]), int(records[it, tile, 1])
            key = C.decode(hw, xcc)
            count[key] = count.get(key, 0) + bad
    return [
        dict(xcc=k[0], se=k[1], sh=k[2], cu=k[3], mismatches=v)
        for k, v in sorted(count.items())
    ]


def cus_seen(records):
    return len(
        {
            C.decode(int(hw), int(xcc))
            for hw, xcc in records.reshape(-1, 4)[:, :2]
        }
    )
