"""The HIP kernels of ``_hiphealth`` against exact references.

Each test runs one kernel once through a probe binding on data of the
test's choosing and compares what comes back with ``hip_reference``: the
copies byte for byte, the MFMA exactly, the n-body step to a bound derived
from float32 rounding alone. Every device buffer of a probe lies between
canary-filled guards that are returned with the result, so an access past
either end shows here as a changed guard byte.
"""

import numpy as np
import pytest

# torch must load before the system-ROCm-linked _hiphealth extension (see
# test_gpu.py): import order is load-bearing.
import torch  # noqa: F401

import hip_reference as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hh():
    from k8s_dra_driver_amd import _hiphealth

    assert _hiphealth.device_count() >= 1
    assert _hiphealth.PROBE_GUARD_BYTES >= 4096
    assert _hiphealth.PROBE_CANARY == R.CANARY
    return _hiphealth


def _payload(hh, buf, nbytes, what):
    """Payload of a guarded result; fails on a changed guard byte."""
    guard = hh.PROBE_GUARD_BYTES
    before, payload, after = R.split_guarded(buf, nbytes, guard)
    for name, g in (("before", before), ("after", after)):
        hit = np.flatnonzero(g != R.CANARY)
        assert hit.size == 0, (
            f"{what}: guard {name} the buffer changed at {hit[:8].tolist()} "
            f"({hit.size} bytes)"
        )
    return payload


# ---------------------------------------------------------------------------
# copy_f4, copy_f4_nt, copy_f4_nt_u4
# ---------------------------------------------------------------------------
def _copy_sizes(blocks):
    stride = 256 * blocks
    return {
        "0": 0,
        "1": 1,
        "255": 255,
        "256": 256,
        "257": 257,
        "stride-1": stride - 1,
        "stride": stride,
        "stride+1": stride + 1,
        "3*stride+5": 3 * stride + 5,
        "4*stride-1": 4 * stride - 1,
        "4*stride": 4 * stride,
        "4*stride+1": 4 * stride + 1,
        "9*stride+77": 9 * stride + 77,
    }


class TestCopyKernels:
    @pytest.mark.parametrize("size", list(_copy_sizes(1)))
    @pytest.mark.parametrize("blocks", [1, 3])
    @pytest.mark.parametrize("variant", ["plain", "nt", "nt_u4"])
    def test_copy_is_byte_exact(self, hh, variant, blocks, size):
        n = _copy_sizes(blocks)[size]
        src = R.make_pattern(n).tobytes()
        out = hh.copy_probe(0, src, variant, blocks)
        problems = R.check_copy(out, src, hh.PROBE_GUARD_BYTES)
        assert not problems, (variant, blocks, n, problems)

    def test_arguments_are_validated(self, hh):
        ok = R.make_pattern(4).tobytes()
        with pytest.raises(ValueError):
            hh.copy_probe(0, ok, "fast", 1)
        with pytest.raises(ValueError):
            hh.copy_probe(0, ok[:-1], "plain", 1)
        with pytest.raises(ValueError):
            hh.copy_probe(0, ok, "plain", 0)
        with pytest.raises(ValueError):
            hh.copy_probe(0, ok, "plain", 1 << 20)
        with pytest.raises(ValueError):
            hh.copy_probe(-1, ok, "plain", 1)
        with pytest.raises(ValueError):
            hh.copy_probe(hh.device_count(), ok, "plain", 1)


# ---------------------------------------------------------------------------
# v_mfma_f32_16x16x32_bf16
# ---------------------------------------------------------------------------
# Exactness. Inputs are m * 2^e with integer |m| <= 15 and e in [-2, 2]:
# 4 significant bits, exact in bf16, |value| <= 60, a multiple of 2^-2.
# A product is a multiple of 2^-4 of magnitude <= 3600. Any partial sum of
# the 32 products of up to 4 chained instructions plus an integer
# |C| <= 1000 is a multiple of 2^-4 below 4*32*3600 + 1000 = 461800 < 2^19,
# i.e. an integer below 2^23 in units of 2^-4: exact in fp32's 24 bits
# whatever the order in which the hardware adds. So equality is exact.
def _exact_values(rng, shape):
    m = rng.integers(-15, 16, shape).astype(np.float64)
    e = rng.integers(-2, 3, shape)
    return m * 2.0**e


def _run_mfma(hh, a, b, c, iters):
    out = hh.mfma_frag_probe(
        0,
        R.pack_a(a).tobytes(),
        R.pack_b(b).tobytes(),
        R.pack_c(c).tobytes(),
        iters,
    )
    raw = _payload(hh, out, 64 * 4 * 4, "mfma_frag_probe")
    return R.unpack_d(raw.view(np.float32).reshape(64, 4)).astype(np.float64)


def _diff(d, want):
    bad = np.argwhere(d != want)
    return (
        f"{len(bad)} of 256 elements differ; first (row, col) "
        f"{bad[:4].tolist()}: got {[d[tuple(i)] for i in bad[:4]]}, "
        f"want {[want[tuple(i)] for i in bad[:4]]}"
    )


class TestMfmaFragments:
    @pytest.fixture(scope="class")
    def abc(self):
        rng = np.random.default_rng(950)
        a = _exact_values(rng, (16, 32))
        b = _exact_values(rng, (32, 16))
        c = rng.integers(-1000, 1001, (16, 16)).astype(np.float64)
        return a, b, c

    @pytest.mark.parametrize("iters", [1, 4])
    def test_random_exact(self, hh, abc, iters):
        a, b, c = abc
        d = _run_mfma(hh, a, b, c, iters)
        want = R.mfma_ref(a, b, c, iters)
        assert np.array_equal(d, want), _diff(d, want)

    def test_zero_iterations_return_c(self, hh, abc):
        a, b, c = abc
        d = _run_mfma(hh, a, b, c, 0)
        assert np.array_equal(d, c), _diff(d, c)

    @pytest.mark.parametrize("half", [0, 1])
    def test_identity_a_selects_half_of_b(self, hh, abc, half):
        _, b, _ = abc  # random, so asymmetric
        a = np.zeros((16, 32))
        a[:, 16 * half : 16 * half + 16] = np.eye(16)
        d = _run_mfma(hh, a, b, np.zeros((16, 16)), 1)
        want = b[16 * half : 16 * half + 16, :]
        assert np.array_equal(d, want), _diff(d, want)

    def test_identity_b_selects_half_of_a(self, hh, abc):
        a, _, _ = abc
        b = np.zeros((32, 16))
        b[:16, :] = np.eye(16)
        d = _run_mfma(hh, a, b, np.zeros((16, 16)), 1)
        want = a[:, :16]
        assert np.array_equal(d, want), _diff(d, want)

    @pytest.mark.parametrize(
        "i, k, j",
        [(0, 0, 0), (5, 19, 11), (15, 31, 0), (0, 8, 15), (12, 7, 4), (9, 24, 9)],
    )
    def test_one_hot(self, hh, i, k, j):
        a = np.zeros((16, 32))
        b = np.zeros((32, 16))
        a[i, k] = 3.0
        b[k, j] = 5.0
        d = _run_mfma(hh, a, b, np.zeros((16, 16)), 1)
        want = np.zeros((16, 16))
        want[i, j] = 15.0
        landed = [(int(r), int(c), d[r, c]) for r, c in np.argwhere(d != 0)]
        assert np.array_equal(d, want), (
            f"A[{i}][{k}] * B[{k}][{j}] should land in D[{i}][{j}] alone, "
            f"landed in {landed}: a wrong row points at the A or C/D map, a "
            f"wrong column at the B or C/D map, nothing at all at the k maps"
        )
        # the same k must also miss every other k of B
        b2 = np.zeros((32, 16))
        b2[(k + 8) % 32, j] = 5.0
        d2 = _run_mfma(hh, a, b2, np.zeros((16, 16)), 1)
        assert not d2.any(), f"A k={k} met B k={(k + 8) % 32}"

    def test_arguments_are_validated(self, hh):
        z = bytes(1024)
        with pytest.raises(ValueError):
            hh.mfma_frag_probe(0, z[:-2], z, z, 1)
        with pytest.raises(ValueError):
            hh.mfma_frag_probe(0, z, z + z, z, 1)
        with pytest.raises(ValueError):
            hh.mfma_frag_probe(0, z, z, z[:16], 1)
        with pytest.raises(ValueError):
            hh.mfma_frag_probe(0, z, z, z, -1)


class TestMfmaBurn:
    # a is all ones. b is 0x3F80 = 1.0 in even lanes and 0x3F81 = 1 + 2^-7
    # in odd lanes; lane l supplies column l & 15 of B, so B's odd columns
    # hold 1.0078125. One instruction adds sum_k 1 * B[k][col] = 32 or
    # 32 * 1.0078125 = 32.25 to each of the lane's 4 accumulator registers
    # (the lane's own column, so its own parity). After `iters` iterations
    # of 8 accumulators the thread's sum is 8 * 4 * iters * 32(.25). At
    # iters = 64 that is 65536 or 66048, a multiple of 0.25 below 2^17:
    # 19 bits, exact in fp32, like every partial sum on the way.
    @pytest.mark.parametrize("iters", [1, 64])
    def test_every_thread_sum_is_exact(self, hh, iters):
        blocks = 2
        out = hh.mfma_burn_probe(0, iters, blocks)
        s = _payload(hh, out, blocks * 256 * 4, "mfma_burn_probe").view(np.float32)
        want = np.where(
            np.arange(blocks * 256) % 2 == 0,
            8 * 4 * iters * 32.0,
            8 * 4 * iters * 32.25,
        ).astype(np.float32)
        bad = np.flatnonzero(s != want)
        assert bad.size == 0, (
            f"{bad.size} of {s.size} threads wrong, first {bad[:4].tolist()}: "
            f"got {s[bad[:4]].tolist()}, want {want[bad[:4]].tolist()}"
        )

    def test_arguments_are_validated(self, hh):
        with pytest.raises(ValueError):
            hh.mfma_burn_probe(0, -1, 2)
        with pytest.raises(ValueError):
            hh.mfma_burn_probe(0, 1, 0)


# ---------------------------------------------------------------------------
# nbody_step
# ---------------------------------------------------------------------------
def _nbody_step(hh, pos, vel, dt, soft2):
    """One probe call. Returns (pos_out, vel_out) as (n, 4) float32 after
    checking the guards of both buffers."""
    n = pos.shape[0]
    p_raw, v_raw = hh.nbody_step_probe(
        0, pos.tobytes(), vel.tobytes(), float(dt), float(soft2)
    )
    p = _payload(hh, p_raw, 16 * n, f"nbody pos_out n={n}")
    v = _payload(hh, v_raw, 16 * n, f"nbody vel n={n}")
    return (
        p.view(np.float32).reshape(n, 4).copy(),
        v.view(np.float32).reshape(n, 4).copy(),
    )


def _check_step(p_out, v_out, pos, vel, dt, soft2):
    problems = R.nbody_problems(v_out[:, :3], p_out[:, :3], pos, vel, dt, soft2)
    use = R.nbody_bound_use(v_out[:, :3], p_out[:, :3], pos, vel, dt, soft2)
    print(f"n={pos.shape[0]}: uses {use[0]:.3f} of the v bound, {use[1]:.3f} of p")
    assert not problems, problems
    # mass and the fourth velocity component pass through bit for bit
    assert np.array_equal(p_out[:, 3].view(np.uint32), pos[:, 3].view(np.uint32))
    assert np.array_equal(v_out[:, 3].view(np.uint32), vel[:, 3].view(np.uint32))


class TestNbodyStep:
    @pytest.mark.parametrize("n", R.NBODY_SHAPES)
    def test_one_step_all_bodies(self, hh, n):
        pos, vel = R.nbody_case(n)
        p_out, v_out = _nbody_step(hh, pos, vel, R.NBODY_DT, R.NBODY_SOFT2)
        _check_step(p_out, v_out, pos, vel, R.NBODY_DT, R.NBODY_SOFT2)

    def test_no_bodies_nothing_written(self, hh):
        p_raw, v_raw = hh.nbody_step_probe(0, b"", b"", 1e-3, 1e-4)
        assert _payload(hh, p_raw, 0, "nbody pos_out n=0").size == 0
        assert _payload(hh, v_raw, 0, "nbody vel n=0").size == 0

    def test_three_chained_steps(self, hh):
        # each step starts from the GPU's own previous output and is held
        # against one reference step from that same input, so no error
        # compounds into the tolerance
        pos, vel = R.nbody_case(257)
        for _ in range(3):
            p_out, v_out = _nbody_step(hh, pos, vel, R.NBODY_DT, R.NBODY_SOFT2)
            _check_step(p_out, v_out, pos, vel, R.NBODY_DT, R.NBODY_SOFT2)
            pos, vel = p_out, v_out

    def test_two_unit_masses_one_unit_apart(self, hh):
        # no softening: f = 1 / 1^3, so each body gains |v| = dt toward
        # the other. The only rounded steps are the reciprocal square
        # root of 1 (1 ulp), its cube and the two fused updates.
        pos = np.array([[0, 0, 0, 1], [1, 0, 0, 1]], dtype=np.float32)
        vel = np.zeros((2, 4), dtype=np.float32)
        dt = R.NBODY_DT
        p_out, v_out = _nbody_step(hh, pos, vel, dt, 0.0)
        tol = 4 * 2.0**-24 * float(dt)
        assert abs(float(v_out[0, 0]) - float(dt)) <= tol, v_out
        assert abs(float(v_out[1, 0]) + float(dt)) <= tol, v_out
        assert not v_out[:, 1:].any(), v_out
        assert not p_out[:, 1:3].any(), p_out
        _check_step(p_out, v_out, pos, vel, dt, 0.0)

    def test_arguments_are_validated(self, hh):
        pos, vel = R.nbody_case(4)
        p, v = pos.tobytes(), vel.tobytes()
        with pytest.raises(ValueError):
            hh.nbody_step_probe(0, p[:-4], v[:-4], 1e-3, 1e-4)
        with pytest.raises(ValueError):
            hh.nbody_step_probe(0, p, v[:-16], 1e-3, 1e-4)
        with pytest.raises(ValueError):
            hh.nbody_step_probe(0, p, v, float("nan"), 1e-4)
        with pytest.raises(ValueError):
            hh.nbody_step_probe(0, p, v, 1e-3, -1.0)
        with pytest.raises(ValueError):
            hh.nbody_step_probe(hh.device_count(), p, v, 1e-3, 1e-4)
