"""numpy references for the MX load self-test (``cpp/mxtest_kernels.hpp`` and
``cpp/mxtest_core.hpp``).

numpy only and no GPU import: ``test_mx_selftest`` checks this module on the
CPU, ``test_mx_selftest_gpu`` compares the kernels with it.

A is ``[M][K]``, B is kept transposed as ``[N][K]``; both are MX operands:
element codes (OCP e4m3 bytes for ``mxfp8``, e2m1 nibbles for ``mxfp4``) and
one E8M0 scale byte per 32 consecutive k of a row. C is ``[M][N]`` float32.
Generated scaled elements are multiples of 2^-2 ("quarter units"); products
and sums are kept in integer units of 2^-4.
"""

import numpy as np

import loadtest_reference as L
import selftest_reference as S

FORMATS = ("mxfp8", "mxfp4")
MAX_K = {"mxfp8": 8192, "mxfp4": 7168}
#: largest magnitude of a generated scaled element, in quarter units
MAX_QUARTER = {"mxfp8": 64, "mxfp4": 48}
TILE = 128
BK = 128
BLOCK = 32
SCALE_BIAS = 127
BATCH = L.BATCH
POISON = L.POISON
RECORD_BYTES = L.RECORD_BYTES
MAX_RECORDS = L.MAX_RECORDS

_M64 = (1 << 64) - 1


# ---------------------------------------------------------------------------
# formats, written from the OCP tables and not from the C++ decode
# ---------------------------------------------------------------------------
def _e4m3_table():
    out = np.zeros(256, dtype=np.float64)
    for code in range(256):
        e, m = (code >> 3) & 15, code & 7
        if e == 15 and m == 7:
            mag = np.nan
        elif e == 0:
            mag = (m / 8.0) * 2.0**-6
        else:
            mag = (1.0 + m / 8.0) * 2.0 ** (e - 7)
        out[code] = -mag if code & 0x80 else mag
    return out


E4M3 = _e4m3_table()
_E2M1_MAG = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)
E2M1 = np.array(_E2M1_MAG + tuple(-v for v in _E2M1_MAG), dtype=np.float64)
E4M3.setflags(write=False)
E2M1.setflags(write=False)


def table(fmt):
    return {"mxfp8": E4M3, "mxfp4": E2M1}[fmt]


def decode(fmt, codes):
    """float64 values of element codes."""
    return table(fmt)[np.asarray(codes, dtype=np.int64)]


def encode(fmt, values):
    """Element codes (uint8) of values that the format holds exactly; raises
    otherwise. +0 encodes as code 0."""
    tab = table(fmt)
    values = np.asarray(values, dtype=np.float64)
    codes = np.zeros(values.shape, dtype=np.uint8)
    found = values == 0
    for code in range(1, len(tab)):
        if np.isnan(tab[code]) or tab[code] == 0:
            continue
        hit = values == tab[code]
        codes[hit] = code
        found |= hit
    if not found.all():
        raise ValueError(f"a value is not exact in {fmt}")
    return codes


def e8m0(scale_bytes):
    """float64 value 2^(b - 127) of E8M0 bytes; 0xFF is NaN."""
    b = np.asarray(scale_bytes, dtype=np.int64)
    out = np.ldexp(1.0, b - SCALE_BIAS)
    return np.where(b == 0xFF, np.nan, out)


def row_bytes(fmt, k):
    return k // 2 if fmt == "mxfp4" else k


def pack(fmt, codes):
    """``(rows, k)`` element codes as the kernels take them: one byte each
    for mxfp8, two to a byte with the even k in the low nibble for mxfp4."""
    codes = np.ascontiguousarray(codes, dtype=np.uint8)
    if fmt == "mxfp8":
        return codes
    assert (codes < 16).all() and codes.shape[1] % 2 == 0
    return (codes[:, 0::2] | (codes[:, 1::2] << 4)).astype(np.uint8)


def unpack(fmt, packed, k):
    packed = np.asarray(packed, dtype=np.uint8)
    if fmt == "mxfp8":
        return packed.reshape(-1, k)
    packed = packed.reshape(-1, k // 2)
    out = np.empty((packed.shape[0], k), dtype=np.uint8)
    out[:, 0::2] = packed & 15
    out[:, 1::2] = packed >> 4
    return out


# ---------------------------------------------------------------------------
# generator
# ---------------------------------------------------------------------------
def _hash(seed, fmt, scale, which, rows, cols):
    f = FORMATS.index(fmt) + 1
    r = np.arange(rows, dtype=np.uint64)[:, None]
    c = np.arange(cols, dtype=np.uint64)[None, :]
    key = (
        (np.uint64(f) << np.uint64(60))
        | (np.uint64(scale) << np.uint64(57))
        | (np.uint64(which) << np.uint64(56))
        | (r << np.uint64(28))
        | c
    )
    with np.errstate(over="ignore"):
        return S.mix(key + np.uint64(seed & _M64))


def element_codes(seed, fmt, which, rows, k):
    """Generated element codes of operand ``which`` (0 = A, 1 = B^T),
    ``(rows, k)`` uint8."""
    h = _hash(seed, fmt, 0, which, rows, k)
    if fmt == "mxfp4":
        return (h % np.uint64(16)).astype(np.uint8)
    v = (h % np.uint64(17)).astype(np.int64) - 8
    return encode(fmt, v)


def scale_bytes(seed, fmt, which, rows, k):
    """Generated scale bytes, ``(rows, k / 32)`` uint8: 126, 127 or 128."""
    h = _hash(seed, fmt, 1, which, rows, k // BLOCK)
    return (SCALE_BIAS - 1 + ((h >> np.uint64(32)) % np.uint64(3))).astype(np.uint8)


def quarter_units(fmt, codes, scales):
    """Scaled elements ``decode(code) * 2^(scale - 127)`` as int64 multiples
    of 2^-2; raises when one is not such a multiple or not finite."""
    v = decode(fmt, codes) * np.repeat(e8m0(scales), BLOCK, axis=1) * 4.0
    if not np.isfinite(v).all() or (v != np.rint(v)).any():
        raise ValueError("a scaled element is not a multiple of 2^-2")
    return np.rint(v).astype(np.int64)


def generate(seed, fmt, which, rows, k):
    """``(codes, scales, quarter units)`` of a generated operand."""
    codes = element_codes(seed, fmt, which, rows, k)
    scales = scale_bytes(seed, fmt, which, rows, k)
    return codes, scales, quarter_units(fmt, codes, scales)


# ---------------------------------------------------------------------------
# product
# ---------------------------------------------------------------------------
def gemm_units(a_quarter, bt_quarter):
    """``A @ B`` in int64 units of 2^-4, formed in float64 where it is exact
    (every sum is far below 2^53)."""
    a = np.asarray(a_quarter, dtype=np.int64)
    bt = np.asarray(bt_quarter, dtype=np.int64)
    assert np.abs(a).max() <= 4096 and np.abs(bt).max() <= 4096
    return np.rint(a.astype(np.float64) @ bt.astype(np.float64).T).astype(np.int64)


def to_f32(c_units):
    """Units of 2^-4 as float32; raises when one needs more than 24
    significant bits."""
    c = np.asarray(c_units, dtype=np.int64)
    mag = np.abs(c)
    low = mag & -mag  # lowest set bit
    low[mag == 0] = 1
    if (mag // low >= (1 << 24)).any():
        raise ValueError("a sum is not exact in float32")
    return (c.astype(np.float64) / 16.0).astype(np.float32)


#: What a sum may reach, in units of 2^-4, for the caps on K. mxfp4: 2^24
#: units, all of fp32's significand. mxfp8: generated scaled elements are
#: multiples of 2^-1, so sums are multiples of 4 units; the cap keeps them
#: inside 2^23 of those, one bit to spare, exactly as the bf16 load test does.
BOUND_UNITS = {"mxfp8": 1 << 25, "mxfp4": 1 << 24}


def bound_holds(fmt, k):
    """Whether a sum of ``k`` largest products stays inside the format's
    bound: the argument behind ``MAX_K``."""
    return MAX_QUARTER[fmt] ** 2 * k <= BOUND_UNITS[fmt]


def gemm_f32(a_quarter, bt_quarter):
    return to_f32(gemm_units(a_quarter, bt_quarter))


def checksum(a_quarter, bt_quarter):
    """Row sums ``A (B 1)`` and column sums ``(1^T A) B`` of C in units of
    2^-4, without forming C."""
    a = np.asarray(a_quarter, dtype=np.int64)
    bt = np.asarray(bt_quarter, dtype=np.int64)
    return a @ bt.sum(axis=0), bt @ a.sum(axis=0)


# ---------------------------------------------------------------------------
# lane map of v_mfma_scale_f32_16x16x128_f8f6f4
# ---------------------------------------------------------------------------
def operand_lane(fmt, row, k):
    """``(lane, element j of the lane's 32)`` that holds A[row][k] (or
    B^T[col][k] with the column for the row). mxfp4: 32 consecutive k per
    lane. mxfp8: 16 consecutive k in elements 0..15 and the 16 that lie 64
    further in elements 16..31."""
    if fmt == "mxfp4":
        return (k // 32) * 16 + row, k % 32
    return ((k % 64) // 16) * 16 + row, 16 * (k // 64) + k % 16


def scale_lane(row, block):
    """The lane whose scale register holds the scale of ``row`` and k-block
    ``block`` (k = 32 block .. 32 block + 31), for both formats."""
    return block * 16 + row


def result_lane(row, col):
    """``(lane, register)`` that holds C[row][col]."""
    return (row // 4) * 16 + col, row % 4


tile_of = L.tile_of
expected_mismatches = L.expected_mismatches
bad_tiles = L.bad_tiles
bad_cus = L.bad_cus
cus_seen = L.cus_seen
