"""CPU checks of ``hip_reference``: the references that the GPU tests
compare the HIP kernels with are right, and each comparator fails when it
should. No GPU and no native extension is touched here."""

import numpy as np
import pytest

import hip_reference as R

GUARD = 4096


# ---------------------------------------------------------------------------
# MFMA lane maps
# ---------------------------------------------------------------------------
class TestMfmaMaps:
    @pytest.mark.parametrize(
        "index, slots, shape",
        [
            (R.a_index, 8, (16, 32)),
            (R.b_index, 8, (32, 16)),
            (R.cd_index, 4, (16, 16)),
        ],
    )
    def test_lane_map_is_bijection(self, index, slots, shape):
        seen = {index(lane, j) for lane in range(64) for j in range(slots)}
        assert len(seen) == 64 * slots == shape[0] * shape[1]
        assert seen == {(r, c) for r in range(shape[0]) for c in range(shape[1])}

    def test_maps_are_the_documented_ones(self):
        # lane 37 = 16*2 + 5
        assert R.a_index(37, 3) == (5, 19)
        assert R.b_index(37, 3) == (19, 5)
        assert R.cd_index(37, 3) == (11, 5)

    @pytest.mark.parametrize("seed", [0, 1, 2])
    def test_lanewise_emulation_equals_matmul(self, seed):
        rng = np.random.default_rng(seed)
        a = rng.integers(-15, 16, (16, 32)).astype(np.float64)
        b = rng.integers(-15, 16, (32, 16)).astype(np.float64)
        c = rng.integers(-1000, 1001, (16, 16)).astype(np.float64)
        d = R.emulate_mfma(R.pack_a(a), R.pack_b(b), R.pack_c(c))
        assert np.array_equal(R.unpack_d(d), a @ b + c)
        assert np.array_equal(R.unpack_d(d), R.mfma_ref(a, b, c, 1))

    def test_emulation_rejects_a_transposed_pack(self):
        rng = np.random.default_rng(3)
        a = rng.integers(-15, 16, (16, 32)).astype(np.float64)
        b = rng.integers(-15, 16, (32, 16)).astype(np.float64)
        c = np.zeros((16, 16))
        # B packed with A's map (its transpose laid out as A) is a
        # different matrix unless B is symmetric in the map's sense
        wrong = R.emulate_mfma(R.pack_a(a), R.pack_a(b.T[:, ::-1]), R.pack_c(c))
        assert not np.array_equal(R.unpack_d(wrong), a @ b)

    def test_pack_unpack_roundtrip(self):
        c = np.arange(256, dtype=np.float32).reshape(16, 16)
        assert np.array_equal(R.unpack_d(R.pack_c(c)), c)

    def test_bf16_bits(self):
        vals = np.array([1.0, -0.25, 60.0, 0.0, 1.0078125])
        bits = R.bf16_bits(vals)
        assert list(bits) == [0x3F80, 0xBE80, 0x4270, 0x0000, 0x3F81]
        assert np.array_equal(R.bf16_value(bits), vals.astype(np.float32))
        with pytest.raises(ValueError):
            R.bf16_bits(np.array([1.0 + 2.0**-9]))
        with pytest.raises(ValueError):
            R.bf16_bits(np.array([1.0 + 2.0**-30]))  # lost already in float32


# ---------------------------------------------------------------------------
# copy comparator
# ---------------------------------------------------------------------------
def _guarded(payload: bytes) -> bytearray:
    g = bytes([R.CANARY]) * GUARD
    return bytearray(g + payload + g)


class TestCopyComparator:
    N = 300

    @pytest.fixture(scope="class")
    def src(self):
        return R.make_pattern(self.N).tobytes()

    def test_pattern_elements_are_distinct_and_awkward(self):
        p = R.make_pattern(self.N)
        assert p.shape == (self.N, 4) and p.dtype == np.uint32
        assert len({row.tobytes() for row in p}) == self.N
        words = set(p.ravel().tolist())
        for w in R.AWKWARD_WORDS:
            assert w in words
        # the tail of the buffer carries them too
        assert set(p[-10:].ravel().tolist()) & set(R.AWKWARD_WORDS)
        assert R.make_pattern(0).shape == (0, 4)
        assert R.make_pattern(1).shape == (1, 4)

    def test_exact_copy_passes(self, src):
        assert R.check_copy(bytes(_guarded(src)), src, GUARD) == []
        assert R.check_copy(bytes(_guarded(b"")), b"", GUARD) == []

    def test_rejects_element_left_at_canary(self, src):
        out = _guarded(src)
        i = 123
        out[GUARD + 16 * i : GUARD + 16 * (i + 1)] = bytes([R.CANARY]) * 16
        problems = R.check_copy(bytes(out), src, GUARD)
        assert len(problems) == 1
        assert "dst[123]" in problems[0] and "never written" in problems[0]

    def test_rejects_two_elements_swapped(self, src):
        out = _guarded(src)
        a, b = 7, 260
        ea = bytes(out[GUARD + 16 * a : GUARD + 16 * (a + 1)])
        eb = bytes(out[GUARD + 16 * b : GUARD + 16 * (b + 1)])
        out[GUARD + 16 * a : GUARD + 16 * (a + 1)] = eb
        out[GUARD + 16 * b : GUARD + 16 * (b + 1)] = ea
        problems = R.check_copy(bytes(out), src, GUARD)
        assert len(problems) == 1
        assert "dst[7] holds src[260]" in problems[0]
        assert "2 of 300" in problems[0]

    def test_rejects_flipped_nan_payload_bit(self, src):
        words = R.make_pattern(self.N).ravel()
        (where,) = np.nonzero(words == 0x7FC12345)
        out = _guarded(src)
        # lowest payload bit of the quiet NaN: still a NaN, equal as floats
        # to nothing, and only a byte compare sees the change
        out[GUARD + 4 * int(where[0])] ^= 0x01
        problems = R.check_copy(bytes(out), src, GUARD)
        assert len(problems) == 1 and f"dst[{int(where[0]) // 4}]" in problems[0]

    def test_rejects_changed_guard_byte_before(self, src):
        out = _guarded(src)
        out[GUARD - 1] ^= 0xFF
        problems = R.check_copy(bytes(out), src, GUARD)
        assert len(problems) == 1 and "before" in problems[0] and "-1" in problems[0]

    def test_rejects_changed_guard_byte_after(self, src):
        out = _guarded(src)
        out[GUARD + len(src)] = 0x00
        problems = R.check_copy(bytes(out), src, GUARD)
        assert len(problems) == 1 and "after" in problems[0] and "[0]" in problems[0]

    def test_rejects_wrong_length(self, src):
        assert R.check_copy(bytes(_guarded(src))[:-1], src, GUARD)


# ---------------------------------------------------------------------------
# n-body reference, tolerance and mutations
# ---------------------------------------------------------------------------
def _step64(pos, vel, **kw):
    """One float64 step as ``(v, p)`` with a reference term changed."""
    pos = pos.astype(np.float64)
    vel3 = vel.astype(np.float64)[:, :3]
    dt = float(R.NBODY_DT)
    soft2 = 0.0 if kw.get("no_softening") else float(R.NBODY_SOFT2)
    sources = pos[: kw.get("sources", pos.shape[0])].copy()
    if kw.get("unit_mass"):
        sources[:, 3] = 1.0 / pos.shape[0]
    x = pos[:, :3]
    d = sources[None, :, :3] - x[:, None, :]
    r2 = (d * d).sum(-1) + soft2
    with np.errstate(divide="ignore", invalid="ignore"):
        f = np.where(r2 > 0, sources[None, :, 3] / (r2 * np.sqrt(r2)), 0.0)
    acc = (f[:, :, None] * d).sum(1)
    v = vel3 + acc * dt
    p = x + (vel3 if kw.get("old_velocity") else v) * dt
    return v, p


#: name -> (keyword for _step64 as a function of n, smallest n at which the
#: change alters the result at all)
MUTATIONS = {
    "last body dropped": (lambda n: {"sources": n - 1}, 2),
    "last tile dropped": (lambda n: {"sources": (n - 1) // 256 * 256}, 2),
    "masses ignored": (lambda n: {"unit_mass": True}, 2),
    "softening omitted": (lambda n: {"no_softening": True}, 2),
    "position advanced with the old velocity": (lambda n: {"old_velocity": True}, 2),
}


class TestNbodyReference:
    def test_unmutated_helper_is_the_reference(self):
        pos, vel = R.nbody_case(257)
        v, p = _step64(pos, vel)
        v_ref, p_ref, _ = R.nbody_ref64(pos, vel, R.NBODY_DT, R.NBODY_SOFT2)
        assert np.allclose(v, v_ref, rtol=1e-13, atol=0)
        assert np.allclose(p, p_ref, rtol=1e-13, atol=0)
        assert R.nbody_problems(v, p, pos, vel, R.NBODY_DT, R.NBODY_SOFT2) == []

    def test_case_has_the_awkward_bodies(self):
        for n in R.NBODY_SHAPES:
            pos, vel = R.nbody_case(n)
            assert pos.shape == vel.shape == (n, 4)
            assert np.abs(pos[:, :3]).max() <= 0.5
            assert (vel[:, :3] != 0).all()
            if n >= 3:
                assert np.array_equal(pos[n - 1, :3], pos[0, :3])
                assert pos[n // 2, 3] == 0 and (pos[:, 3] == 0).sum() == 1
            if n >= 2:
                assert len(set(pos[:, 3].tolist())) > 1

    def test_two_body_analytic(self):
        pos = np.array([[0, 0, 0, 1], [1, 0, 0, 1]], dtype=np.float32)
        vel = np.zeros((2, 4), dtype=np.float32)
        v, p, s = R.nbody_ref64(pos, vel, R.NBODY_DT, 0.0)
        dt = float(R.NBODY_DT)
        assert np.array_equal(v, [[dt, 0, 0], [-dt, 0, 0]])
        assert np.array_equal(s, [[1, 0, 0], [1, 0, 0]])
        assert np.allclose(p, [[dt * dt, 0, 0], [1 - dt * dt, 0, 0]], rtol=1e-15)

    @pytest.mark.parametrize("n", R.NBODY_SHAPES)
    def test_float32_emulation_inside_tolerance(self, n):
        pos, vel = R.nbody_case(n)
        v, p = R.nbody_emul32(pos, vel, R.NBODY_DT, R.NBODY_SOFT2)
        use_v, use_p = R.nbody_bound_use(v, p, pos, vel, R.NBODY_DT, R.NBODY_SOFT2)
        print(f"n={n}: emulation uses {use_v:.3f} of the v bound, {use_p:.3f} of p")
        assert R.nbody_problems(v, p, pos, vel, R.NBODY_DT, R.NBODY_SOFT2) == []
        assert use_v <= 1.0 and use_p <= 1.0

    @pytest.mark.parametrize("name", sorted(MUTATIONS))
    @pytest.mark.parametrize("n", R.NBODY_SHAPES)
    def test_mutated_reference_outside_tolerance(self, n, name):
        make_kw, n_min = MUTATIONS[name]
        pos, vel = R.nbody_case(n)
        v, p = _step64(pos, vel, **make_kw(n))
        problems = R.nbody_problems(v, p, pos, vel, R.NBODY_DT, R.NBODY_SOFT2)
        if n < n_min:
            # a lone body feels no force: the change alters nothing
            assert problems == []
        else:
            assert problems, f"{name} at n={n} passes the tolerance"

    @pytest.mark.parametrize("n", [2, 257, 513])
    def test_dropping_one_body_misses_by_a_wide_margin(self, n):
        pos, vel = R.nbody_case(n)
        v, p = _step64(pos, vel, sources=n - 1)
        use_v, _ = R.nbody_bound_use(v, p, pos, vel, R.NBODY_DT, R.NBODY_SOFT2)
        assert use_v > 1000

    @pytest.mark.parametrize("n", R.NBODY_SHAPES)
    def test_output_equal_to_input_outside_tolerance(self, n):
        pos, vel = R.nbody_case(n)
        problems = R.nbody_problems(
            vel[:, :3], pos[:, :3], pos, vel, R.NBODY_DT, R.NBODY_SOFT2
        )
        assert any(p.startswith("p[") for p in problems)
        if n >= 2:
            assert any(p.startswith("v[") for p in problems)

    def test_nan_is_outside_tolerance(self):
        pos, vel = R.nbody_case(2)
        v, p = R.nbody_emul32(pos, vel, R.NBODY_DT, R.NBODY_SOFT2)
        v = v.copy()
        v[1, 2] = np.nan
        assert R.nbody_problems(v, p, pos, vel, R.NBODY_DT, R.NBODY_SOFT2)


class TestExistingNbodyTestGap:
    """``test_gpu.TestNbodyCorrectness`` compared positions after 3 steps
    to 1e-3 of the scale; the bodies move less than that, so a kernel that
    copies its input passed. Its displacement assertion closes the gap."""

    N, ITERS = 512, 3

    @pytest.fixture(scope="class")
    def trajectory(self):
        p0 = R.lcg_bodies(self.N)
        pos = p0.astype(np.float64)
        vel = np.zeros((self.N, 3))
        for _ in range(self.ITERS):
            vel, x, _ = R.nbody_ref64(pos, vel, np.float32(1e-3), np.float32(1e-4))
            pos = np.concatenate([x, pos[:, 3:]], axis=1)
        return p0, pos

    def test_lcg_init(self):
        p0 = R.lcg_bodies(4)
        assert p0.dtype == np.float32 and p0.shape == (4, 4)
        s = (0x5A1AD * 1664525 + 1013904223) & 0xFFFFFFFF
        assert p0[0, 0] == np.float32(s >> 8) / np.float32(1 << 24) - np.float32(0.5)
        assert (p0[:, 3] == np.float32(0.25)).all()

    def test_displacement_is_below_the_old_tolerance(self, trajectory):
        p0, pos = trajectory
        moved = np.abs(pos[:64, :3] - p0[:64, :3].astype(np.float64)).max()
        scale = np.abs(pos[:64, :3]).max()
        assert moved / scale < 1e-3  # so pos_out = pos_in met the old check
        assert moved / scale < 1e-4

    def test_displacement_assertion_rejects_a_noop_kernel(self, trajectory):
        p0, pos = trajectory
        p0_64 = p0[:64, :3].astype(np.float64)
        noop = p0_64  # pos_out = pos_in
        miss = np.abs((noop - p0_64) - (pos[:64, :3] - p0_64)).max()
        bound = 4 * self.ITERS * 2.0**-25
        assert miss > 50 * bound, (miss, bound)
