"""The MX load self-test on an MI355X: the lane map and the arithmetic of
``v_mfma_scale_f32_16x16x128_f8f6f4`` pinned with one instruction,
``mx_gemm_ref`` and ``mx_gemm`` against an exact integer product,
``c_verify``'s reports against the numpy reference, and the path from the
child process up to the driver.

No test provokes a fault: what is injected is wrong data at valid indices of
A (checked on the host before any launch) or a wrong expectation, never a
wrong address. Every device buffer that comes back lies between canary
guards, and every call checks them.
"""

import functools

import numpy as np
import pytest

# torch must load before the system-ROCm-linked _hiphealth extension (see
# test_gpu.py): import order is load-bearing.
import torch  # noqa: F401

import hip_reference as R
import mxtest_reference as X

pytestmark = pytest.mark.gpu

SEED = 0x0123456789ABCDEF
FORMATS = list(X.FORMATS)


def shapes(fmt):
    # one K-step; the LDS image used again; M != N both ways, so a transposed
    # tile map shows; the cap on K
    return [(128, 128, 128), (128, 128, 256), (256, 128, 384), (128, 384, 128),
            (128, 128, X.MAX_K[fmt])]


CASES = [(f, s) for f in FORMATS for s in shapes(f)]


def case_id(c):
    return c[0] + "-" + "x".join(map(str, c[1]))


@pytest.fixture(scope="module")
def hh():
    from k8s_dra_driver_amd import _hiphealth

    assert _hiphealth.device_count() >= 1
    assert _hiphealth.PROBE_CANARY == R.CANARY
    assert _hiphealth.SELFTEST_MAX_RECORDS == X.MAX_RECORDS
    assert tuple(_hiphealth.MXTEST_FORMATS) == X.FORMATS
    assert dict(_hiphealth.MXTEST_MAX_K) == X.MAX_K
    assert _hiphealth.LOADTEST_BATCH == X.BATCH
    assert _hiphealth.LOADTEST_POISON == X.POISON
    return _hiphealth


class Operand:
    """Codes ``(rows, k)``, scale bytes ``(rows, k / 32)`` and the scaled
    elements in quarter units."""

    def __init__(self, fmt, codes, scales):
        self.fmt = fmt
        self.codes = np.ascontiguousarray(codes, dtype=np.uint8)
        self.scales = np.ascontiguousarray(scales, dtype=np.uint8)
        self.quarter = X.quarter_units(fmt, self.codes, self.scales)
        for arr in (self.codes, self.scales, self.quarter):
            arr.setflags(write=False)

    @property
    def packed(self):
        return X.pack(self.fmt, self.codes)


# built once per case, shared and never modified
@functools.lru_cache(maxsize=None)
def case(fmt, m, n, k):
    a = Operand(fmt, *X.generate(SEED, fmt, 0, m, k)[:2])
    bt = Operand(fmt, *X.generate(SEED, fmt, 1, n, k)[:2])
    want = X.gemm_f32(a.quarter, bt.quarter)
    want.setflags(write=False)
    return a, bt, want


def payload(hh, raw, nbytes, dtype, shape):
    """The payload of guard + payload + guard, both guards checked."""
    before, body, after = R.split_guarded(raw, nbytes, hh.PROBE_GUARD_BYTES)
    assert (before == hh.PROBE_CANARY).all() and (after == hh.PROBE_CANARY).all()
    return body.view(dtype).reshape(shape)


def probe(hh, a, bt, stage, want=None, iterations=1, flips=()):
    """One ``mx_gemm_probe`` call. Checks what holds for every call: intact
    guards, every tile's own record, and a report that agrees with the raw
    records. Returns ``(C as uint32, report, tile records (iterations run,
    tiles, 4))``."""
    fmt = a.fmt
    m, k = a.codes.shape
    n = bt.codes.shape[0]
    tiles = (m // X.TILE) * (n // X.TILE)
    raw_c, d, raw_rec = hh.mx_gemm_probe(
        0, fmt, a.packed.tobytes(), a.scales.tobytes(), bt.packed.tobytes(),
        bt.scales.tobytes(), m, n, k,
        b"" if want is None else np.ascontiguousarray(want, np.float32).tobytes(),
        iterations, list(flips), stage,
    )
    c = payload(hh, raw_c, 4 * m * n, np.uint32, (m, n))
    if stage == "ref":
        assert d is None and raw_rec is None
        return c, None, None
    rec = payload(
        hh, raw_rec, X.RECORD_BYTES * tiles * iterations, "<u4", (iterations, tiles, 4)
    )
    ran = 1 if stage == "gemm" else d["iterations"]
    assert (rec[ran:] == 0xA5A5A5A5).all()  # iterations that never ran
    rec = rec[:ran]
    assert (rec[:, :, 2] == np.arange(tiles)).all()  # its own tile index
    assert (rec[:, :, 3] == 0).all()
    assert (rec[:, :, 1] < 8).all()  # XCC_ID, nothing else of that register
    if stage == "gemm":
        assert d is None
        return c, None, rec
    assert (d["m"], d["n"], d["k"], d["device"]) == (m, n, k, 0)
    assert d["format"] == fmt
    assert d["ok"] is (d["mismatches"] == 0) and d["checksum_ok"] is True
    assert d["cus_seen"] == X.cus_seen(rec)
    assert sum(t[2] for t in d["bad_tiles"]) == d["mismatches"]
    assert sum(cu["mismatches"] for cu in d["bad_cus"]) == d["mismatches"]
    assert len(d["records"]) == min(d["mismatches"], X.MAX_RECORDS)
    assert (c == X.POISON).all()  # verified, then poisoned
    return c, d, rec


def one_mfma(hh, fmt, a_codes, a_scales, bt_codes, bt_scales, c, opsel=0, other=136):
    """D [16][16] float32 of one scaled MFMA on operands in matrix form."""
    raw = hh.mx_mfma_probe(
        0, fmt, X.pack(fmt, a_codes).tobytes(),
        np.ascontiguousarray(a_scales, np.uint8).tobytes(),
        X.pack(fmt, bt_codes).tobytes(),
        np.ascontiguousarray(bt_scales, np.uint8).tobytes(),
        np.ascontiguousarray(c, np.float32).tobytes(), opsel, other,
    )
    return payload(hh, raw, 4 * 256, np.float32, (16, 16))


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


# ---------------------------------------------------------------------------
# one instruction: decode, scales, lane map, exactness
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS)
def test_every_code_decodes_and_lands_where_the_lane_map_says(hh, fmt):
    """Sixteen codes per instruction, each in a row, a column and a k of its
    own that vary with the code, against 1.0 in B at the same k. Every (row,
    block) has its own scale byte, A's differ from B's, and the scales travel
    in each of the four bytes of the scale registers in turn."""
    tab = X.table(fmt)
    codes = [c for c in range(len(tab)) if not np.isnan(tab[c])]
    assert len(codes) == (254 if fmt == "mxfp8" else 16)
    one = int(X.encode(fmt, [1.0])[0])
    blocks_used, scales_used = set(), set()
    for g in range(0, len(codes), 16):
        group = codes[g:g + 16]
        gi = g // 16
        a = np.zeros((16, 128), dtype=np.uint8)
        bt = np.zeros((16, 128), dtype=np.uint8)
        r, b = np.meshgrid(np.arange(16), np.arange(4), indexing="ij")
        sa = (120 + (r + 3 * b + gi) % 15).astype(np.uint8)
        sb = (121 + (2 * r + b + gi) % 13).astype(np.uint8)
        want = np.zeros((16, 16), dtype=np.float64)
        for i, code in enumerate(group):
            row = (5 * i + gi) % 16
            col = (3 * i + 2 * gi + 1) % 16
            k = 8 * i + (gi + code) % 8
            a[row, k] = code
            bt[col, k] = one
            sa[row, k // 32] = 117 + code % 21  # 2^-10 .. 2^10
            sb[col, k // 32] = 137 - (5 * code + 3) % 21
            blocks_used.add(k // 32)
            scales_used |= {int(sa[row, k // 32]), int(sb[col, k // 32])}
            want[row, col] = tab[code] * 2.0 ** (
                int(sa[row, k // 32]) + int(sb[col, k // 32]) - 254
            )
        assert (sa != sb).any() and (want != want.T).any()
        want32 = want.astype(np.float32)
        assert (want32.astype(np.float64) == want).all()
        want32[want32 == 0] = 0.0  # -0 * 1 + (+0) is +0
        got = one_mfma(hh, fmt, a, sa, bt, sb, np.zeros((16, 16)), opsel=gi % 4)
        bad = np.nonzero(bits(got) != bits(want32))
        assert bad[0].size == 0, (group, bad, got[bad], want32[bad])
    assert blocks_used == {0, 1, 2, 3}
    if fmt == "mxfp8":
        assert {117, 137} <= scales_used


@pytest.mark.parametrize("fmt", FORMATS)
def test_one_instruction_adds_exactly_across_the_whole_significand(hh, fmt):
    half = int(X.encode(fmt, [0.5])[0])
    top = 6.0 if fmt == "mxfp4" else 8.0
    big = int(X.encode(fmt, [top])[0])
    down = np.full((16, 4), 126, dtype=np.uint8)  # 2^-1
    up = np.full((16, 4), 128, dtype=np.uint8)

    # C at the top of the range, one product at the bottom
    a = np.zeros((16, 128), dtype=np.uint8)
    bt = np.zeros((16, 128), dtype=np.uint8)
    a[5, 77] = half
    bt[9, 77] = half
    c = np.zeros((16, 16), dtype=np.float32)
    c[5, 9] = np.float32(2.0**20 - 2.0**-4)
    c[6, 9] = np.float32(2.0**20 - 2.0**-4)
    assert float(c[5, 9]) == 2.0**20 - 2.0**-4
    want = c.copy()
    want[5, 9] = 2.0**20
    got = one_mfma(hh, fmt, a, down, bt, down, c)
    assert (bits(got) == bits(want)).all(), (got[5, 9], got[6, 9])

    # 128 products of 2^-4 under a C that they carry to a power of two
    a[:] = 0
    bt[:] = 0
    a[5, :] = half
    bt[9, :] = half
    c[:] = 0
    c[5, 9] = np.float32(2.0**20 - 8.0)
    want = c.copy()
    want[5, 9] = 2.0**20
    got = one_mfma(hh, fmt, a, down, bt, down, c)
    assert (bits(got) == bits(want)).all(), got[5, 9]

    # 127 largest products and one smallest in the same sum, every position
    # of the smallest in turn for one k-block and one k of each other block
    for k_small in list(range(32)) + [45, 64, 127]:
        a[:] = 0
        bt[:] = 0
        a[5, :] = big
        bt[9, :] = big
        sa, sb = up.copy(), up.copy()
        blk = k_small // 32
        sa[5, blk] = 126
        sb[9, blk] = 126
        a[5, k_small] = half
        bt[9, k_small] = half
        qa = X.quarter_units(fmt, a, sa)
        qb = X.quarter_units(fmt, bt, sb)
        assert qa[5, k_small] == 1 and qb[9, k_small] == 1
        want = X.gemm_f32(qa, qb)
        assert int(round(float(want[5, 9]) * 16)) % 2 == 1  # lowest unit set
        got = one_mfma(hh, fmt, a, sa, bt, sb, np.zeros((16, 16)))
        assert (bits(got) == bits(want)).all(), (k_small, got[5, 9], want[5, 9])


# ---------------------------------------------------------------------------
# exact results
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("c", CASES, ids=case_id)
@pytest.mark.parametrize("stage", ["ref", "gemm"])
def test_both_kernels_equal_the_integer_product_bit_for_bit(hh, c, stage):
    fmt, shape = c
    a, bt, want = case(fmt, *shape)
    got, _, _ = probe(hh, a, bt, stage)
    bad = np.nonzero(got != want.view(np.uint32))
    assert bad[0].size == 0, (bad[0][:8], bad[1][:8])


@pytest.mark.parametrize("fmt", FORMATS)
def test_generated_operands_equal_the_numpy_generator(hh, fmt):
    def check(m, n, k, seed):
        raws = hh.mx_operands_probe(0, fmt, m, n, k, seed)
        rb, kb = X.row_bytes(fmt, k), k // X.BLOCK
        for which, rows, raw_e, raw_s in ((0, m, raws[0], raws[1]),
                                          (1, n, raws[2], raws[3])):
            codes, scales, _ = X.generate(seed, fmt, which, rows, k)
            got_e = payload(hh, raw_e, rows * rb, np.uint8, (rows, rb))
            got_s = payload(hh, raw_s, rows * kb, np.uint8, (rows, kb))
            assert (got_e == X.pack(fmt, codes)).all()
            assert (got_s == scales).all()

    check(128, 384, 128, SEED)
    check(256, 128, 384, SEED)
    check(128, 128, 128, 2**64 - 1)  # the seed wraps mod 2^64 like the host's


# ---------------------------------------------------------------------------
# layout
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS)
def test_identity_times_an_asymmetric_b_is_b(hh, fmt):
    """A = I: C must be B itself. With B[k][j] != B[j][k] a C written with
    rows and columns swapped does not pass."""
    n = 128
    one = int(X.encode(fmt, [1.0])[0])
    a = Operand(fmt, one * np.eye(n, dtype=np.uint8), np.full((n, 4), 127))
    j, k = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    if fmt == "mxfp4":
        codes = (3 * j + 5 * k) % 16
    else:
        codes = X.encode(fmt, (3 * j + 5 * k) % 17 - 8)
    jb, kb = np.meshgrid(np.arange(n), np.arange(4), indexing="ij")
    bt = Operand(fmt, codes, 126 + (jb + 2 * kb) % 3)
    assert (bt.quarter != bt.quarter.T).any()
    want = X.gemm_f32(a.quarter, bt.quarter)
    assert (want == (bt.quarter.T * 0.25).astype(np.float32)).all()
    for stage in ("ref", "gemm"):
        c, _, _ = probe(hh, a, bt, stage)
        assert (c == want.view(np.uint32)).all(), stage


@pytest.mark.parametrize("fmt", FORMATS)
def test_the_largest_sums_at_the_cap_on_k_are_exact(hh, fmt):
    """Every scaled element the largest the generator makes, but one pair of
    the smallest magnitude the bound's derivation allows. mxfp4: 6 * 2^1
    everywhere; the block of the pair has scale 2^-1 and the pair is 0.5
    each, a product of 2^-4. mxfp8: 8 * 2^1 everywhere; the pair is 0.25 *
    2^1 each, a product of 2^-2 (mxfp8's sums are multiples of 2^-2). The
    element they meet in has the lowest unit set."""
    k = X.MAX_K[fmt]
    top = 6.0 if fmt == "mxfp4" else 8.0
    codes_a = np.full((128, k), int(X.encode(fmt, [top])[0]), dtype=np.uint8)
    codes_b = codes_a.copy()
    sa = np.full((128, k // 32), 128, dtype=np.uint8)
    sb = sa.copy()
    where = 4321
    if fmt == "mxfp4":
        small, unit = 0.5, 1
        sa[77, where // 32] = 126
        sb[19, where // 32] = 126
    else:
        small, unit = 0.25, 4
    codes_a[77, where] = codes_b[19, where] = int(X.encode(fmt, [small])[0])
    a, bt = Operand(fmt, codes_a, sa), Operand(fmt, codes_b, sb)
    assert np.abs(a.quarter).max() == X.MAX_QUARTER[fmt]
    want = X.gemm_f32(a.quarter, bt.quarter)
    units = X.gemm_units(a.quarter, bt.quarter)
    assert units[0, 0] == X.MAX_QUARTER[fmt] ** 2 * k
    assert units[77, 19] % (2 * unit) == unit
    assert units.max() <= X.BOUND_UNITS[fmt]
    for stage in ("ref", "gemm"):
        c, _, _ = probe(hh, a, bt, stage)
        bad = np.nonzero(c != want.view(np.uint32))
        assert bad[0].size == 0, (stage, bad[0][:8], bad[1][:8])


# ---------------------------------------------------------------------------
# c_verify
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS)
def test_nothing_injected_nothing_found(hh, fmt):
    for shape in [(128, 128, 128), (256, 128, 384), (128, 384, 128)]:
        a, bt, want = case(fmt, *shape)
        for w in (None, want):  # mx_gemm_ref's expectation, then the integer one
            _, d, rec = probe(hh, a, bt, "verify", want=w, iterations=3)
            assert d["ok"] is True and d["mismatches"] == 0
            assert d["iterations"] == 3 and rec.shape[0] == 3
            assert d["records"] == [] and d["bad_tiles"] == [] and d["bad_cus"] == []


@pytest.mark.parametrize("fmt", FORMATS)
def test_sign_flips_in_a_are_found_where_they_are(hh, fmt):
    m, n, k = 256, 128, 384
    a, bt, want = case(fmt, m, n, k)
    flips, flipped = [], a.quarter.copy()
    # one row in each of the two tiles; an even k, then an odd one
    for row, parity in ((3, 0), (200, 1)):
        nonzero = np.nonzero(a.quarter[row])[0]
        col = int(nonzero[nonzero % 2 == parity][5])
        if fmt == "mxfp4":  # the even k is the low nibble
            flips.append((row * (k // 2) + col // 2, 0x80 if col % 2 else 0x08))
        else:
            flips.append((row * k + col, 0x80))
        flipped[row, col] = -flipped[row, col]
    mism = X.expected_mismatches(X.gemm_f32(flipped, bt.quarter), want)
    assert {r for r, _, _, _ in mism} == {3, 200} and len(mism) > X.MAX_RECORDS

    asked = 20  # more than one batch: the first one is the last
    _, d, rec = probe(hh, a, bt, "verify", iterations=asked, flips=flips)
    assert d["ok"] is False
    assert d["iterations"] == X.BATCH
    assert d["mismatches"] == X.BATCH * len(mism)
    assert {r[1:] for r in d["records"]} <= mism
    assert {r[0] for r in d["records"]} <= set(range(X.BATCH))
    assert len(set(d["records"])) == X.MAX_RECORDS
    assert d["bad_tiles"] == X.bad_tiles(mism, n, iterations=X.BATCH)
    assert [t[:2] for t in d["bad_tiles"]] == [(0, 0), (1, 0)]
    per_tile = {0: 0, 1: 0}
    for row, col, _, _ in mism:
        per_tile[X.tile_of(row, col, n)] += 1
    assert d["bad_cus"] == X.bad_cus(rec, per_tile)

    # the same flip twice cancels
    _, d, _ = probe(hh, a, bt, "verify", iterations=2, flips=flips + flips)
    assert d["ok"] is True and d["iterations"] == 2


@pytest.mark.parametrize("fmt", FORMATS)
def test_a_wrong_expectation_is_reported_once_per_iteration(hh, fmt):
    m, n, k = 128, 384, 128
    a, bt, want = case(fmt, m, n, k)
    wrong = want.copy()
    wrong[70, 300] += np.float32(0.0625)  # one unit
    assert wrong[70, 300] != want[70, 300]
    _, d, rec = probe(hh, a, bt, "verify", want=wrong, iterations=3)
    got_bits = int(want.view(np.uint32)[70, 300])
    want_bits = int(wrong.view(np.uint32)[70, 300])
    assert d["mismatches"] == 3 and d["iterations"] == 3
    assert sorted(d["records"]) == [(i, 70, 300, got_bits, want_bits) for i in range(3)]
    assert d["bad_tiles"] == [(0, 2, 3)]
    assert d["bad_cus"] == X.bad_cus(rec, {2: 1})


def test_record_cap(hh):
    a, bt, want = case("mxfp4", 128, 128, 128)
    rng = np.random.default_rng(64)
    where = rng.choice(want.size, size=100, replace=False)
    wrong = want.copy()
    wrong.reshape(-1)[where] += np.float32(1)
    mism = X.expected_mismatches(want, wrong)
    assert len(mism) == 100
    _, d, _ = probe(hh, a, bt, "verify", want=wrong, iterations=1)
    assert d["mismatches"] == 100
    assert len(set(d["records"])) == X.MAX_RECORDS
    assert {r[1:] for r in d["records"]} <= mism
    assert d["bad_tiles"] == [(0, 0, 100)]


# ---------------------------------------------------------------------------
# arguments
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS)
def test_arguments_are_validated_before_any_launch(hh, fmt):
    m, n, k = 128, 128, 128
    rb = X.row_bytes(fmt, k)
    cap = X.MAX_K[fmt]
    names = ("device", "format", "a", "a_scales", "b_t", "b_t_scales", "m", "n",
             "k", "want", "iterations", "flips", "stage")
    ok = dict(zip(names, (0, fmt, bytes(m * rb), bytes([127]) * (m * 4),
                          bytes(n * rb), bytes([127]) * (n * 4), m, n, k, b"",
                          1, [], "verify")))

    def operands(rows_m, rows_n, depth):
        return dict(
            a=bytes(rows_m * X.row_bytes(fmt, depth)),
            a_scales=bytes(rows_m * (depth // 32)),
            b_t=bytes(rows_n * X.row_bytes(fmt, depth)),
            b_t_scales=bytes(rows_n * (depth // 32)),
        )

    def call(**kw):
        args = dict(ok)
        args.update(kw)
        return hh.mx_gemm_probe(*[args[name] for name in names])

    assert call()[1]["ok"] is True
    big = 8192
    for bad in (
        dict(a=ok["a"][:-1]),
        dict(b_t=ok["b_t"] + b"\0"),
        dict(a_scales=ok["a_scales"][:-1]),
        dict(b_t_scales=ok["b_t_scales"] + b"\0"),
        dict(want=bytes(4 * m * n - 4)),
        dict(m=0), dict(m=-128), dict(m=64), dict(m=192),
        dict(n=0), dict(n=130),
        dict(k=0), dict(k=64), dict(k=192, **operands(m, n, 192)),
        dict(k=cap + 128, **operands(m, n, cap + 128)),
        # shapes whose buffers exceed the probe's cap
        dict(m=big, n=big, **operands(big, big, k)),
        dict(iterations=0),
        dict(iterations=hh.LOADTEST_PROBE_MAX_ITERATIONS + 1),
        dict(flips=[(m * rb, 1)]),
        dict(flips=[(-1, 1)]),
        dict(flips=[(0, 0x100)]),
        dict(flips=[(0, -1)]),
        dict(flips=[(0, 1)] * 4097),
        dict(stage="check"),
        dict(format="mxfp6"), dict(format=""),
        dict(device=-1),
        dict(device=hh.device_count()),
    ):
        with pytest.raises(ValueError):
            call(**bad)
    for kw in (
        dict(seconds=0.0), dict(seconds=-1.0), dict(seconds=600.5),
        dict(seconds=float("nan")), dict(m=100), dict(n=0), dict(k=cap + 128),
        dict(k=64), dict(format="bf16"),
        dict(device=-1), dict(device=hh.device_count()),
    ):
        args = dict(device=0, format=fmt, seconds=1.0)
        args.update(kw)
        with pytest.raises(ValueError):
            hh.mx_selftest(**args)
    for args in ((0, fmt, 100, 128, 128, 1), (0, fmt, 128, 128, cap + 128, 1),
                 (0, "fp8", 128, 128, 128, 1), (-1, fmt, 128, 128, 128, 1)):
        with pytest.raises(ValueError):
            hh.mx_operands_probe(*args)
    rows = bytes(16 * X.row_bytes(fmt, 128))
    sc, c = bytes([127]) * 64, bytes(1024)
    for args in (
        (0, fmt, rows[:-1], sc, rows, sc, c), (0, fmt, rows, sc[:-1], rows, sc, c),
        (0, fmt, rows, sc, rows + b"\0", sc, c), (0, fmt, rows, sc, rows, sc + sc, c),
        (0, fmt, rows, sc, rows, sc, c[:-4]), (0, "mxfp6", rows, sc, rows, sc, c),
        (0, fmt, rows, sc, rows, sc, c, 4), (0, fmt, rows, sc, rows, sc, c, -1),
        (0, fmt, rows, sc, rows, sc, c, 0, 255),
        (hh.device_count(), fmt, rows, sc, rows, sc, c),
    ):
        with pytest.raises(ValueError):
            hh.mx_mfma_probe(*args)


# ---------------------------------------------------------------------------
# production path
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS)
def test_one_second_of_the_default_shape(hh, fmt):
    """Coverage is measured against ``cu_footprint`` in the same process:
    both see the same CU mask, whatever the machine sets. The TF/s figure
    is printed, never judged."""
    foot = hh.cu_footprint(0)
    r = hh.mx_selftest(0, fmt, 1.0)
    print(
        f"mx_selftest {fmt}: {r['iterations']} iterations of "
        f"{r['m']}x{r['n']}x{r['k']} in {r['seconds']:.2f}s, "
        f"{r['tflops']:.0f} TF/s, {r['cus_seen']} CUs seen "
        f"(cu_footprint {foot['count']}), golden stage "
        f"{r['golden_seconds']:.2f}s"
    )
    assert r["format"] == fmt
    assert r["ok"] is True and r["checksum_ok"] is True
    assert r["checksum_first_bad"] == ""
    assert r["mismatches"] == 0 and r["records"] == []
    assert r["bad_tiles"] == [] and r["bad_cus"] == []
    assert (r["m"], r["n"], r["k"]) == (4096, 4096, 4096)
    assert r["iterations"] >= 1 and r["iterations"] % X.BATCH == 0
    assert r["seconds"] >= 1.0
    assert r["cus_seen"] == foot["count"]


# ---------------------------------------------------------------------------
# child and driver
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def real_lib():
    from k8s_dra_driver_amd.hal.amdsmi import AmdSmiDeviceLib

    lib = AmdSmiDeviceLib()
    lib.open()
    yield lib
    lib.close()


def test_the_child_passes_with_the_mx_stages(hh, real_lib):
    from k8s_dra_driver_amd import selftest

    gpu = real_lib.enumerate()[0]
    res = selftest.run(gpu, mib=64, load_seconds=1, load_formats=("mxfp8", "mxfp4"))
    print("child --load-formats mxfp8,mxfp4:", res.outcome, f"{res.seconds:.2f}s",
          res.error)
    assert res.outcome == "pass", res.error
    assert res.findings() == []
    assert list(res.report["load_mx"]) == ["mxfp8", "mxfp4"]
    for fmt, part in res.report["load_mx"].items():
        assert part["format"] == fmt
        assert part["ok"] is True and part["checksum_ok"] is True
        assert part["iterations"] >= 1 and part["mismatches"] == 0


def test_driver_startup_selftest_with_mx_on_the_real_hal(real_lib, tmp_path):
    from k8s_dra_driver_amd.kube.client import InMemoryKube
    from k8s_dra_driver_amd.plugin.driver import Driver

    kube = InMemoryKube()
    kube.api_versions = ["v1beta2", "v1beta1"]
    driver = Driver(
        real_lib,
        kube,
        node_name="gpu-node",
        cdi_root=str(tmp_path / "cdi"),
        checkpoint_root=str(tmp_path / "state"),
        use_tmpfs=False,
        gpu_indices=[0],
    )
    try:
        results = driver.run_startup_selftest(
            mib=64, load_seconds=1, load_formats=("mxfp8", "mxfp4")
        )
        assert results == {0: "pass"}
        assert driver.health.findings(0) == []
        value = driver.metrics.registry.get_sample_value
        for fmt in ("mxfp8", "mxfp4"):
            labels = {"gpu": "0", "format": fmt}
            assert value("dra_gpu_selftest_mx_iterations", labels) >= 1
            assert value("dra_gpu_selftest_mx_mismatches", labels) == 0
        assert value("dra_gpu_selftest_load_iterations", {"gpu": "0"}) >= 1
    finally:
        driver.shutdown(unpublish=False)
