"""The load self-test on an MI355X: ``gemm_ref`` and ``load_gemm`` against an
exact integer product, ``c_verify``'s reports against the numpy reference,
and the path from the child process up to the driver.

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
import loadtest_reference as L

pytestmark = pytest.mark.gpu

SEED = 0x0123456789ABCDEF
# one tile and one K-step; two K-steps (the LDS image is used again); M != N
# both ways, so a transposed tile map shows; the cap on K
SHAPES = [(128, 128, 64), (128, 128, 128), (256, 128, 192), (128, 384, 64),
          (128, 128, 8192)]


@pytest.fixture(scope="module")
def hh():
    from k8s_dra_driver_amd import _hiphealth

    assert _hiphealth.device_count() >= 1
    assert _hiphealth.PROBE_CANARY == R.CANARY
    assert _hiphealth.SELFTEST_MAX_RECORDS == L.MAX_RECORDS
    assert _hiphealth.LOADTEST_MAX_K == L.MAX_K
    assert _hiphealth.LOADTEST_BATCH == L.BATCH
    assert _hiphealth.LOADTEST_POISON == L.POISON
    return _hiphealth


# built once per shape, shared and never modified
@functools.lru_cache(maxsize=None)
def case(m, n, k):
    a = L.half_units(SEED, 0, m, k)
    bt = L.half_units(SEED, 1, n, k)
    want = L.gemm_f32(a, bt)
    for arr in (a, bt, want):
        arr.setflags(write=False)
    return a, bt, want


def payload(hh, raw, nbytes, dtype, shape):
    """The payload of guard + payload + guard, both guards checked."""
    before, body, after = R.split_guarded(raw, nbytes, hh.PROBE_GUARD_BYTES)
    assert (before == hh.PROBE_CANARY).all() and (after == hh.PROBE_CANARY).all()
    return body.view(dtype).reshape(shape)


def probe(hh, a, bt, stage, want=None, iterations=1, flips=()):
    """One ``load_gemm_probe`` call on operands in half units. Checks what
    holds for every call: intact guards, every tile's own record, and a
    report that agrees with the raw records. Returns ``(C as uint32,
    report, tile records (iterations run, tiles, 4))``."""
    m, k = a.shape
    n = bt.shape[0]
    tiles = (m // L.TILE) * (n // L.TILE)
    raw_c, d, raw_rec = hh.load_gemm_probe(
        0, L.bits_of(a).tobytes(), L.bits_of(bt).tobytes(), m, n, k,
        b"" if want is None else np.ascontiguousarray(want, np.float32).tobytes(),
        iterations, list(flips), stage,
    )
    c = payload(hh, raw_c, 4 * m * n, np.uint32, (m, n))
    if stage == "ref":
        assert d is None and raw_rec is None
        return c, None, None
    rec = payload(
        hh, raw_rec, L.RECORD_BYTES * tiles * iterations, "<u4", (iterations, tiles, 4)
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
    assert d["ok"] is (d["mismatches"] == 0) and d["checksum_ok"] is True
    assert d["cus_seen"] == L.cus_seen(rec)
    assert sum(t[2] for t in d["bad_tiles"]) == d["mismatches"]
    assert sum(cu["mismatches"] for cu in d["bad_cus"]) == d["mismatches"]
    assert len(d["records"]) == min(d["mismatches"], L.MAX_RECORDS)
    assert (c == L.POISON).all()  # verified, then poisoned
    return c, d, rec


# ---------------------------------------------------------------------------
# exact results
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("stage", ["ref", "gemm"])
def test_both_kernels_equal_the_integer_product_bit_for_bit(hh, shape, stage):
    a, bt, want = case(*shape)
    c, _, _ = probe(hh, a, bt, stage)
    bad = np.nonzero(c != want.view(np.uint32))
    assert bad[0].size == 0, (bad[0][:8], bad[1][:8])


def test_generated_operands_equal_the_numpy_generator(hh):
    for m, n, k in [(128, 384, 64), (256, 128, 192)]:
        a, bt, _ = case(m, n, k)
        raw_a, raw_bt = hh.load_operands_probe(0, m, n, k, SEED)
        got_a = payload(hh, raw_a, 2 * m * k, np.uint16, (m, k))
        got_bt = payload(hh, raw_bt, 2 * n * k, np.uint16, (n, k))
        assert (got_a == L.bits_of(a)).all()
        assert (got_bt == L.bits_of(bt)).all()
    # the seed wraps mod 2^64 like the host's
    raw_a, _ = hh.load_operands_probe(0, 128, 128, 64, 2**64 - 1)
    got = payload(hh, raw_a, 2 * 128 * 64, np.uint16, (128, 64))
    assert (got == L.bits_of(L.half_units(2**64 - 1, 0, 128, 64))).all()


# ---------------------------------------------------------------------------
# layout
# ---------------------------------------------------------------------------
def test_identity_times_an_asymmetric_b_is_b(hh):
    """A = I: C must be B itself. With B[k][j] != B[j][k] a C written with
    rows and columns swapped does not pass."""
    n = 128
    a = 2 * np.eye(n, dtype=np.int64)  # 1.0 in half units
    j, k = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    bt = (3 * j + 5 * k) % 33 - 16  # B^T[j][k] = B[k][j]
    assert (bt != bt.T).any()
    want = L.gemm_f32(a, bt)
    assert (want == (bt.T * 0.5).astype(np.float32)).all()
    for stage in ("ref", "gemm"):
        c, _, _ = probe(hh, a, bt, stage)
        assert (c == want.view(np.uint32)).all(), stage


def test_the_largest_sums_at_the_cap_on_k_are_exact(hh):
    """Every entry 16 but one pair of 0.5: the element they meet in is
    256 * 8191 + 0.25, 23 bits of units of 2^-2 with the lowest one set."""
    k = L.MAX_K
    a = np.full((128, k), 32, dtype=np.int64)
    bt = np.full((128, k), 32, dtype=np.int64)
    a[77, 4321] = 1
    bt[19, 4321] = 1
    want = L.gemm_f32(a, bt)
    assert float(want[77, 19]) == 256.0 * (k - 1) + 0.25
    assert float(want[0, 0]) == 256.0 * k
    for stage in ("ref", "gemm"):
        c, _, _ = probe(hh, a, bt, stage)
        bad = np.nonzero(c != want.view(np.uint32))
        assert bad[0].size == 0, (stage, bad[0][:8], bad[1][:8])


# ---------------------------------------------------------------------------
# c_verify
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(128, 128, 64), (256, 128, 192), (128, 384, 64)])
def test_nothing_injected_nothing_found(hh, shape):
    a, bt, want = case(*shape)
    for w in (None, want):  # gemm_ref's expectation, then the integer one
        _, d, rec = probe(hh, a, bt, "verify", want=w, iterations=3)
        assert d["ok"] is True and d["mismatches"] == 0
        assert d["iterations"] == 3 and rec.shape[0] == 3
        assert d["records"] == [] and d["bad_tiles"] == [] and d["bad_cus"] == []


def test_sign_flips_in_a_are_found_where_they_are(hh):
    m, n, k = 256, 128, 192
    a, bt, want = case(m, n, k)
    flips, flipped = [], a.copy()
    for row in (3, 200):  # one row in each of the two tiles
        col = int(np.nonzero(a[row])[0][5])
        flips.append((row * k + col, 0x8000))
        flipped[row, col] = -flipped[row, col]
    mism = L.expected_mismatches(L.gemm_f32(flipped, bt), want)
    assert {r for r, _, _, _ in mism} == {3, 200} and len(mism) > L.MAX_RECORDS

    asked = 20  # more than one batch: the first one is the last
    _, d, rec = probe(hh, a, bt, "verify", iterations=asked, flips=flips)
    assert d["ok"] is False
    assert d["iterations"] == L.BATCH
    assert d["mismatches"] == L.BATCH * len(mism)
    assert {r[1:] for r in d["records"]} <= mism
    assert {r[0] for r in d["records"]} <= set(range(L.BATCH))
    assert len(set(d["records"])) == L.MAX_RECORDS
    assert d["bad_tiles"] == L.bad_tiles(mism, n, iterations=L.BATCH)
    assert [t[:2] for t in d["bad_tiles"]] == [(0, 0), (1, 0)]
    per_tile = {0: 0, 1: 0}
    for row, col, _, _ in mism:
        per_tile[L.tile_of(row, col, n)] += 1
    assert d["bad_cus"] == L.bad_cus(rec, per_tile)

    # the same flip twice cancels
    _, d, _ = probe(hh, a, bt, "verify", iterations=2, flips=flips + flips)
    assert d["ok"] is True and d["iterations"] == 2


def test_a_wrong_expectation_is_reported_once_per_iteration(hh):
    m, n, k = 128, 384, 64
    a, bt, want = case(m, n, k)
    wrong = want.copy()
    wrong[70, 300] += np.float32(0.25)  # one unit
    assert wrong[70, 300] != want[70, 300]
    _, d, rec = probe(hh, a, bt, "verify", want=wrong, iterations=3)
    got_bits = int(want.view(np.uint32)[70, 300])
    want_bits = int(wrong.view(np.uint32)[70, 300])
    assert d["mismatches"] == 3 and d["iterations"] == 3
    assert sorted(d["records"]) == [(i, 70, 300, got_bits, want_bits) for i in range(3)]
    assert d["bad_tiles"] == [(0, 2, 3)]
    assert d["bad_cus"] == L.bad_cus(rec, {2: 1})


def test_record_cap(hh):
    a, bt, want = case(128, 128, 64)
    rng = np.random.default_rng(64)
    where = rng.choice(want.size, size=100, replace=False)
    wrong = want.copy()
    wrong.reshape(-1)[where] += np.float32(1)
    mism = L.expected_mismatches(want, wrong)
    assert len(mism) == 100
    _, d, _ = probe(hh, a, bt, "verify", want=wrong, iterations=1)
    assert d["mismatches"] == 100
    assert len(set(d["records"])) == L.MAX_RECORDS
    assert {r[1:] for r in d["records"]} <= mism
    assert d["bad_tiles"] == [(0, 0, 100)]


def test_arguments_are_validated_before_any_launch(hh):
    m, n, k = 128, 128, 64
    a = bytes(2 * m * k)
    bt = bytes(2 * n * k)
    names = ("device", "a", "b_t", "m", "n", "k", "want", "iterations", "flips", "stage")
    ok = dict(zip(names, (0, a, bt, m, n, k, b"", 1, [], "verify")))

    def call(**kw):
        args = dict(ok)
        args.update(kw)
        return hh.load_gemm_probe(*[args[name] for name in names])

    assert call()[1]["ok"] is True
    big = 8192
    for bad in (
        dict(a=a[:-2]),
        dict(b_t=bt + b"\0\0"),
        dict(want=bytes(4 * m * n - 4)),
        dict(m=0), dict(m=-128), dict(m=64), dict(m=192),
        dict(n=0), dict(n=130),
        dict(k=0), dict(k=32), dict(k=96),
        dict(k=L.MAX_K + 64, a=bytes(2 * m * (L.MAX_K + 64)),
             b_t=bytes(2 * n * (L.MAX_K + 64))),
        # shapes whose buffers exceed the probe's cap
        dict(m=big, n=big, a=bytes(2 * big * k), b_t=bytes(2 * big * k)),
        dict(iterations=0),
        dict(iterations=hh.LOADTEST_PROBE_MAX_ITERATIONS + 1),
        dict(flips=[(m * k, 1)]),
        dict(flips=[(-1, 1)]),
        dict(flips=[(0, 0x10000)]),
        dict(flips=[(0, -1)]),
        dict(flips=[(0, 1)] * 4097),
        dict(stage="check"),
        dict(device=-1),
        dict(device=hh.device_count()),
    ):
        with pytest.raises(ValueError):
            call(**bad)
    for kw in (
        dict(seconds=0.0), dict(seconds=-1.0), dict(seconds=600.5),
        dict(seconds=float("nan")), dict(m=100), dict(n=0), dict(k=L.MAX_K + 64),
        dict(device=-1), dict(device=hh.device_count()),
    ):
        with pytest.raises(ValueError):
            hh.load_selftest(**kw)
    for args in ((0, 100, 128, 64, 1), (0, 128, 128, 8256, 1), (-1, 128, 128, 64, 1)):
        with pytest.raises(ValueError):
            hh.load_operands_probe(*args)


# ---------------------------------------------------------------------------
# production path
# ---------------------------------------------------------------------------
def test_one_second_of_the_default_shape(hh):
    """Coverage is measured against ``cu_footprint`` in the same process:
    both see the same CU mask, whatever the machine sets. The TF/s figure
    is printed, never judged."""
    foot = hh.cu_footprint(0)
    r = hh.load_selftest(0, seconds=1.0)
    print(
        f"load_selftest: {r['iterations']} iterations of "
        f"{r['m']}x{r['n']}x{r['k']} in {r['seconds']:.2f}s, "
        f"{r['tflops']:.0f} TF/s, {r['cus_seen']} CUs seen "
        f"(cu_footprint {foot['count']})"
    )
    assert r["ok"] is True and r["checksum_ok"] is True
    assert r["checksum_first_bad"] == ""
    assert r["mismatches"] == 0 and r["records"] == []
    assert r["bad_tiles"] == [] and r["bad_cus"] == []
    assert (r["m"], r["n"], r["k"]) == (4096, 4096, 4096)
    assert r["iterations"] >= 1 and r["iterations"] % L.BATCH == 0
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


def test_the_child_passes_with_the_load_stage(hh, real_lib):
    from k8s_dra_driver_amd import selftest

    gpu = real_lib.enumerate()[0]
    res = selftest.run(gpu, mib=64, load_seconds=1)
    print("child --load-seconds 1:", res.outcome, f"{res.seconds:.2f}s", res.error)
    assert res.outcome == "pass", res.error
    assert res.findings() == []
    load = res.report["load"]
    assert load["ok"] is True and load["checksum_ok"] is True
    assert load["iterations"] >= 1 and load["mismatches"] == 0


def test_driver_startup_selftest_with_load_on_the_real_hal(real_lib, tmp_path):
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
        results = driver.run_startup_selftest(mib=64, load_seconds=1)
        assert results == {0: "pass"}
        assert driver.health.findings(0) == []
        value = driver.metrics.registry.get_sample_value
        assert value("dra_gpu_selftest_load_iterations", {"gpu": "0"}) >= 1
        assert value("dra_gpu_selftest_load_mismatches", {"gpu": "0"}) == 0
    finally:
        driver.shutdown(unpublish=False)
