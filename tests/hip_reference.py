"""High-precision references for the kernels in ``cpp/hiphealth.hip``.

numpy only and no GPU import: ``test_hip_reference`` checks this module on
the CPU (that the references are right and that the comparators can fail),
``test_hip_kernels`` and ``test_gpu`` compare the kernels with it.

Everything the kernels leave to the caller lives here: the test pattern of
the copies, the lane maps of ``v_mfma_f32_16x16x32_bf16``, and one n-body
step in float64 with the error bound that a float32 kernel must meet.
"""

import numpy as np

CANARY = 0xA5

# ---------------------------------------------------------------------------
# copy
# ---------------------------------------------------------------------------

#: bit patterns a copy must not touch: -0.0, smallest and largest denormal
#: (the latter negative), +inf, -inf, a quiet NaN with payload, and the
#: signalling NaN 0x7F800001 that any float move may quieten.
AWKWARD_WORDS = (
    0x80000000,
    0x00000001,
    0x807FFFFF,
    0x7F800000,
    0xFF800000,
    0x7FC12345,
    0x7F800001,
)

_GOLDEN = 0x9E3779B1  # odd, so k -> k * _GOLDEN mod 2^32 is a bijection


def make_pattern(n):
    """``n`` float4 as a ``(n, 4)`` uint32 array. Word ``k`` of the buffer
    holds ``k * 0x9E3779B1 mod 2^32``: every word names its own index, so
    no two elements are equal and a misplaced one is recognisable. The
    awkward patterns overwrite every fifth word from word 1, and again
    counted back from the end, so they fall in the main loop and in the
    tail of an unrolled kernel."""
    words = (np.arange(4 * n, dtype=np.uint64) * _GOLDEN) & 0xFFFFFFFF
    words = words.astype(np.uint32)
    for k, w in enumerate(AWKWARD_WORDS):
        for idx in (5 * k + 1, 4 * n - 2 - 5 * k):
            if 0 <= idx < 4 * n:
                words[idx] = w
    return words.reshape(n, 4)


def check_copy(out, src, guard, canary=CANARY):
    """Compare a guarded destination with its source, bytes for bytes.

    ``out`` is ``guard + dst + guard`` as the probe returns it, ``src`` the
    bytes handed in. Returns a list of findings, empty when the copy is
    exact: a wrong length, the first wrong 16-byte element (and which
    source element it holds, if any), and every changed guard byte."""
    out = np.frombuffer(bytes(out), dtype=np.uint8)
    src = np.frombuffer(bytes(src), dtype=np.uint8)
    problems = []
    if out.size != src.size + 2 * guard:
        return [f"length {out.size}, expected {src.size} + 2*{guard}"]
    before, dst, after = (
        out[:guard],
        out[guard : guard + src.size],
        out[guard + src.size :],
    )
    if src.size % 16 == 0:
        d16 = dst.reshape(-1, 16)
        s16 = src.reshape(-1, 16)
        wrong = np.flatnonzero((d16 != s16).any(axis=1))
        if wrong.size:
            i = int(wrong[0])
            got = d16[i].tobytes()
            if got == bytes([canary]) * 16:
                what = "was never written (canary)"
            else:
                same = np.flatnonzero((s16 == d16[i]).all(axis=1))
                what = (
                    f"holds src[{int(same[0])}]"
                    if same.size
                    else f"holds {got.hex()}, expected {s16[i].tobytes().hex()}"
                )
            problems.append(
                f"dst[{i}] {what}; {wrong.size} of {d16.shape[0]} elements wrong"
            )
    elif (dst != src).any():
        problems.append(f"byte {int(np.flatnonzero(dst != src)[0])} differs")
    for name, g, base in (("before", before, -guard), ("after", after, 0)):
        hit = np.flatnonzero(g != canary)
        if hit.size:
            problems.append(
                f"guard {name} dst changed at offsets "
                f"{[int(h) + base for h in hit[:8]]} ({hit.size} bytes)"
            )
    return problems


# ---------------------------------------------------------------------------
# MFMA: v_mfma_f32_16x16x32_bf16, D(16x16) = A(16x32) @ B(32x16) + C(16x16)
# ---------------------------------------------------------------------------
M, N, K = 16, 16, 32
LANES = 64


def a_index(lane, j):
    """(row, k) of A held in slot ``j`` of ``lane``'s 8-element fragment."""
    return lane & 15, 8 * (lane >> 4) + j


def b_index(lane, j):
    """(k, col) of B held in slot ``j`` of ``lane``'s 8-element fragment."""
    return 8 * (lane >> 4) + j, lane & 15


def cd_index(lane, reg):
    """(row, col) of C/D held in accumulator register ``reg`` of ``lane``."""
    return 4 * (lane >> 4) + reg, lane & 15


def bf16_bits(x):
    """bf16 bit patterns of float values that bf16 holds exactly."""
    x32 = np.asarray(x, dtype=np.float32)
    bits = x32.view(np.uint32)
    if (bits & 0xFFFF).any() or (x32 != np.asarray(x)).any():
        raise ValueError("value is not exactly representable in bf16")
    return (bits >> 16).astype(np.uint16)


def bf16_value(bits):
    """float32 values of bf16 bit patterns."""
    return (np.asarray(bits, dtype=np.uint32) << 16).view(np.float32)


def pack_a(a):
    """A (16x32) -> the (64, 8) uint16 fragments of the wave."""
    a = bf16_bits(a).reshape(M, K)
    out = np.empty((LANES, 8), dtype=np.uint16)
    for lane in range(LANES):
        for j in range(8):
            out[lane, j] = a[a_index(lane, j)]
    return out


def pack_b(b):
    """B (32x16) -> the (64, 8) uint16 fragments of the wave."""
    b = bf16_bits(b).reshape(K, N)
    out = np.empty((LANES, 8), dtype=np.uint16)
    for lane in range(LANES):
        for j in range(8):
            out[lane, j] = b[b_index(lane, j)]
    return out


def pack_c(c):
    """C (16x16) -> the (64, 4) float32 accumulator registers of the wave."""
    c = np.asarray(c, dtype=np.float32).reshape(M, N)
    out = np.empty((LANES, 4), dtype=np.float32)
    for lane in range(LANES):
        for reg in range(4):
            out[lane, reg] = c[cd_index(lane, reg)]
    return out


def unpack_d(d):
    """The (64, 4) accumulator registers of the wave -> D (16x16)."""
    d = np.asarray(d).reshape(LANES, 4)
    out = np.empty((M, N), dtype=d.dtype)
    for lane in range(LANES):
        for reg in range(4):
            out[cd_index(lane, reg)] = d[lane, reg]
    return out


def mfma_ref(a, b, c, iters=1):
    """``iters * (A @ B) + C`` in float64: what ``iters`` chained
    instructions leave in the accumulator when every step is exact."""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return iters * (a @ b) + np.asarray(c, dtype=np.float64)


def emulate_mfma(a_frag, b_frag, c_frag):
    """The instruction as the hardware documents it, on packed fragments
    and written from the consumer's side: output register ``reg`` of lane
    ``l`` is row ``4*(l>>4)+reg``, column ``l&15``; its k-th term takes A
    from slot ``k&7`` of lane ``row + 16*(k>>3)`` and B from slot ``k&7``
    of lane ``col + 16*(k>>3)``. Deliberately does not call the pack
    functions' index maps, so that a wrong map cannot cancel itself."""
    av = bf16_value(a_frag).astype(np.float64).reshape(LANES, 8)
    bv = bf16_value(b_frag).astype(np.float64).reshape(LANES, 8)
    out = np.array(c_frag, dtype=np.float64).reshape(LANES, 4)
    for lane in range(LANES):
        col = lane % 16
        for reg in range(4):
            row = 4 * (lane // 16) + reg
            acc = 0.0
            for k in range(K):
                acc += av[row + 16 * (k // 8), k % 8] * bv[col + 16 * (k // 8), k % 8]
            out[lane, reg] += acc
    return out


# ---------------------------------------------------------------------------
# n-body: one step of nbody_step (all pairs, symplectic Euler)
# ---------------------------------------------------------------------------
EPS32 = 2.0**-24  # unit roundoff of float32


def lcg_bodies(n):
    """The deterministic init of ``nbody_positions``/``nbody_benchmark``:
    ``(n, 4)`` float32, positions from the 32-bit LCG in [-0.5, 0.5), mass
    ``1/n``. ``n`` is the rounded-up body count the entry points use."""
    s = 0x5A1AD
    out = np.empty((n, 4), dtype=np.float32)
    for i in range(n):
        for c in range(3):
            s = (s * 1664525 + 1013904223) & 0xFFFFFFFF
            out[i, c] = np.float32(s >> 8) / np.float32(1 << 24) - np.float32(0.5)
    out[:, 3] = np.float32(1.0) / np.float32(n)
    return out


def nbody_ref64(pos, vel, dt, soft2):
    """One step in float64 over all bodies. ``pos`` is ``(n, 4)`` with the
    mass in column 3, ``vel`` is ``(n, 3)`` or ``(n, 4)``.

    Returns ``(v, p, S)``, each ``(n, 3)``: the new velocity, the new
    position and ``S[i, c] = sum_j |f_ij * d_ij,c|``, the sum of the
    magnitudes of the terms of the acceleration, which scales the rounding
    error of any summation order. A pair at distance zero with no
    softening (a body and itself) exerts no force."""
    pos = np.asarray(pos, dtype=np.float64)
    vel = np.asarray(vel, dtype=np.float64)[:, :3]
    dt = float(dt)
    x = pos[:, :3]
    d = x[None, :, :] - x[:, None, :]  # d[i, j] = x_j - x_i
    r2 = (d * d).sum(-1) + float(soft2)
    with np.errstate(divide="ignore"):
        f = np.where(r2 > 0, pos[None, :, 3] / (r2 * np.sqrt(r2)), 0.0)
    terms = f[:, :, None] * d
    acc = terms.sum(1)
    s = np.abs(terms).sum(1)
    v = vel + acc * dt
    p = x + v * dt
    return v, p, s


def _fma32(a, b, c):
    # a*b is exact in float64 for float32 inputs; one rounding to float64
    # and one to float32 stand in for fmaf's single rounding.
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(
        np.float32
    )


def nbody_emul32(pos, vel, dt, soft2):
    """The same step in float32 in the kernel's order: acceleration summed
    sequentially over ``j`` with fused multiply-adds, ``inv_r`` cubed.
    Returns ``(v, p)``, each ``(n, 3)`` float32."""
    pos = np.asarray(pos, dtype=np.float32)
    vel = np.asarray(vel, dtype=np.float32)[:, :3]
    dt = np.float32(dt)
    soft2 = np.float32(soft2)
    x = pos[:, :3]
    acc = np.zeros_like(x)
    dtv = np.full(x.shape[0], dt, dtype=np.float32)
    with np.errstate(divide="ignore"):
        for j in range(x.shape[0]):
            d = x[j][None, :] - x
            r2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2] + soft2
            inv_r = np.where(
                r2 > 0, np.float32(1.0) / np.sqrt(r2, dtype=np.float32), np.float32(0)
            ).astype(np.float32)
            f = pos[j, 3] * inv_r * inv_r * inv_r
            for c in range(3):
                acc[:, c] = _fma32(f, d[:, c], acc[:, c])
    v = np.stack([_fma32(acc[:, c], dtv, vel[:, c]) for c in range(3)], axis=1)
    p = np.stack([_fma32(v[:, c], dtv, x[:, c]) for c in range(3)], axis=1)
    return v, p


def nbody_bounds(n, s, v_ref, p_ref, dt):
    """Largest admissible ``|v - v_ref|`` and ``|p - p_ref|`` per body and
    component for a float32 kernel, from the float64 step:

        v_tol = gamma * S * dt + 2^-24 |v_ref|,   gamma = (n + 16) 2^-24
        p_tol = v_tol * dt + 2^-24 |p_ref|

    ``n`` units cover the worst case of a sequential sum of n terms, 16
    the rounding of one term (differences, r^2, the 1-ulp reciprocal
    square root cubed, two products); the last summands are the single
    rounding of the fused update of v and of p."""
    gamma = (n + 16) * EPS32
    v_tol = gamma * s * float(dt) + EPS32 * np.abs(v_ref)
    p_tol = v_tol * float(dt) + EPS32 * np.abs(p_ref)
    return v_tol, p_tol


def nbody_problems(v, p, pos, vel, dt, soft2):
    """Compare one step's velocities and positions (``(n, 3)`` each) with
    the float64 step from ``pos``/``vel``. Returns a list of findings,
    empty when every body and component is inside ``nbody_bounds``."""
    n = np.asarray(pos).shape[0]
    v_ref, p_ref, s = nbody_ref64(pos, vel, dt, soft2)
    v_tol, p_tol = nbody_bounds(n, s, v_ref, p_ref, dt)
    problems = []
    for name, got, ref, tol in (("v", v, v_ref, v_tol), ("p", p, p_ref, p_tol)):
        err = np.abs(np.asarray(got, dtype=np.float64) - ref)
        bad = ~(err <= tol)  # also true for NaN
        if bad.any():
            i, c = np.argwhere(bad)[0]
            problems.append(
                f"{name}[{i}][{c}] = {np.asarray(got)[i, c]!r}, reference "
                f"{ref[i, c]!r}: error {err[i, c]:.3e} > bound {tol[i, c]:.3e}; "
                f"{int(bad.sum())} of {bad.size} components outside"
            )
    return problems


def nbody_bound_use(v, p, pos, vel, dt, soft2):
    """Largest ``error / bound`` over all bodies and components, for v and
    for p: how much of the tolerance a result uses."""
    n = np.asarray(pos).shape[0]
    v_ref, p_ref, s = nbody_ref64(pos, vel, dt, soft2)
    v_tol, p_tol = nbody_bounds(n, s, v_ref, p_ref, dt)
    use = []
    for got, ref, tol in ((v, v_ref, v_tol), (p, p_ref, p_tol)):
        err = np.abs(np.asarray(got, dtype=np.float64) - ref)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(err == 0, 0.0, err / tol)
        use.append(float(ratio.max()) if ratio.size else 0.0)
    return tuple(use)


NBODY_SHAPES = (1, 2, 255, 256, 257, 513)
NBODY_DT = np.float32(1e-3)
NBODY_SOFT2 = np.float32(1e-4)


def nbody_case(n, seed=20240607):
    """Seeded test bodies: ``(pos, vel)``, both ``(n, 4)`` float32.
    Positions in [-0.5, 0.5)^3, masses unequal in [0.5, 1.5)/n, velocities
    in [-0.1, 0.1)^3. From three bodies on, the last body sits exactly on
    body 0 and body n//2 has mass zero. ``vel.w`` carries a marker the
    kernel must leave alone."""
    rng = np.random.default_rng(seed + n)
    pos = np.empty((n, 4), dtype=np.float32)
    vel = np.empty((n, 4), dtype=np.float32)
    pos[:, :3] = rng.random((n, 3), dtype=np.float32) - np.float32(0.5)
    pos[:, 3] = (rng.random(n, dtype=np.float32) + np.float32(0.5)) / np.float32(n)
    vel[:, :3] = (rng.random((n, 3), dtype=np.float32) - np.float32(0.5)) * np.float32(
        0.2
    )
    vel[:, 3] = np.arange(n, dtype=np.float32) + np.float32(0.25)
    if n >= 3:
        pos[n - 1, :3] = pos[0, :3]
        pos[n // 2, 3] = 0.0
    return pos, vel


def split_guarded(buf, payload_bytes, guard):
    """``guard + payload + guard`` -> (before, payload, after) as uint8."""
    raw = np.frombuffer(bytes(buf), dtype=np.uint8)
    assert raw.size == payload_bytes + 2 * guard, (raw.size, payload_bytes, guard)
    return raw[:guard], raw[guard : guard + payload_bytes], raw[guard + payload_bytes :]
