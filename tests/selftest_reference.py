"""numpy references for the startup self-test (``cpp/selftest_kernels.hpp``).

numpy only and no GPU import: ``test_selftest`` checks this module on the
CPU, ``test_selftest_gpu`` compares the kernels with it.

The memory patterns are defined over word indices: the region is ``n``
16-byte elements = ``2n`` little-endian 64-bit words, and word ``w`` is an
index inside the region, never an address.
"""

import numpy as np

import hip_reference as R

PATTERNS = ("addr", "addr_inv", "hash", "hash_inv")
MAX_RECORDS = 64
KAT_VECTORS = 16
KAT_CHAIN = 4

_M64 = (1 << 64) - 1


def mix_int(x):
    """The splitmix64 finaliser on one Python int, all mod 2^64."""
    z = (x + 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def mix(x):
    """The same on a uint64 array (numpy wraps unsigned arithmetic)."""
    x = np.asarray(x, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = x + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def pattern_words(pattern, nwords, seed):
    """Words 0 .. nwords-1 of a pattern as a uint64 array."""
    w = np.arange(nwords, dtype=np.uint64)
    seed = np.uint64(seed & _M64)
    if pattern in ("addr", "addr_inv"):
        out = w ^ seed
    elif pattern in ("hash", "hash_inv"):
        with np.errstate(over="ignore"):
            out = mix(w + seed)
    else:
        raise ValueError(f"unknown pattern {pattern!r}")
    return ~out if pattern.endswith("_inv") else out


def pattern_bytes(pattern, nbytes, seed):
    """The region's bytes: ``nbytes`` must be a multiple of 16."""
    assert nbytes % 16 == 0
    return pattern_words(pattern, nbytes // 8, seed).astype("<u8").tobytes()


def expected_records(pattern, seed, flips, nwords):
    """What a verify must report after ``flips`` (``(word, mask)`` pairs,
    XORed in order) went into a filled region: the set of
    ``(word, got, want)``. Masks on one word combine; a word whose masks
    cancel is no mismatch."""
    words = pattern_words(pattern, nwords, seed)
    masks = {}
    for word, mask in flips:
        assert 0 <= word < nwords
        masks[word] = masks.get(word, 0) ^ (mask & _M64)
    return {
        (word, int(words[word]) ^ mask, int(words[word]))
        for word, mask in masks.items()
        if mask
    }


def apply_flips(region, flips):
    """The filled region's bytes with the flips applied, as the device
    holds it when verify runs."""
    words = np.frombuffer(bytes(region), dtype="<u8").copy()
    for word, mask in flips:
        words[word] ^= np.uint64(mask & _M64)
    return words.tobytes()


# ---------------------------------------------------------------------------
# MFMA known-answer table
# ---------------------------------------------------------------------------
def kat_tables(seed=950):
    """A 16-vector table for ``mfma_kat`` inside the exactness bounds of
    ``test_hip_kernels`` (A, B = m * 2^e with |m| <= 15, e in [-2, 2];
    integer |C| <= 1000; chain of 4), packed with ``hip_reference``'s lane
    maps. Returns ``(a, b, c, want)``: uint16 ``(16, 64, 8)`` twice and
    float32 ``(16, 64, 4)`` twice."""
    rng = np.random.default_rng(seed)
    a_tab = np.empty((KAT_VECTORS, R.LANES, 8), dtype=np.uint16)
    b_tab = np.empty_like(a_tab)
    c_tab = np.empty((KAT_VECTORS, R.LANES, 4), dtype=np.float32)
    want_tab = np.empty_like(c_tab)
    for v in range(KAT_VECTORS):
        a = rng.integers(-15, 16, (R.M, R.K)) * 2.0 ** rng.integers(-2, 3, (R.M, R.K))
        b = rng.integers(-15, 16, (R.K, R.N)) * 2.0 ** rng.integers(-2, 3, (R.K, R.N))
        c = rng.integers(-1000, 1001, (R.M, R.N)).astype(np.float64)
        d = R.mfma_ref(a, b, c, KAT_CHAIN)
        assert np.array_equal(d.astype(np.float32).astype(np.float64), d)
        a_tab[v] = R.pack_a(a)
        b_tab[v] = R.pack_b(b)
        c_tab[v] = R.pack_c(c)
        want_tab[v] = R.pack_c(d)
    return a_tab, b_tab, c_tab, want_tab
