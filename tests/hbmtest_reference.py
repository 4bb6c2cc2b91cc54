"""numpy reference for the HBM march self-test (``cpp/hbmtest_core.hpp`` and
``cpp/hbmtest_kernels.hpp``).

numpy only and no GPU import: ``test_hbm_selftest`` checks this module on the
CPU against cases written out by hand, ``test_hbm_selftest_gpu`` compares the
kernels and the host loop with it.

The coverage is one array of little-endian 64-bit words with a global index
``w``, cut into chunks. Round ``r`` leaves pattern ``r % 4`` of
``selftest_reference.PATTERNS`` with seed ``mix(seed + r // 4)`` in every
word. Pass 0 writes round 0, pass ``p`` (``1 <= p < rounds``) reads round
``p - 1`` and writes round ``p``, pass ``rounds`` reads round ``rounds - 1``.
"""

import numpy as np

import selftest_reference as S

CHUNK_BYTES = 1 << 30
PAGE_BYTES = 2 << 20
MIN_BYTES = 1 << 30
RESERVE_MIN_BYTES = 2 << 30
RESERVE_PERCENT = 2
MAX_RECORDS = 64
PAGES_FIRST = 8

_M64 = (1 << 64) - 1


# ---------------------------------------------------------------------------
# chunk plan
# ---------------------------------------------------------------------------
def reserve(total_bytes):
    return max(RESERVE_MIN_BYTES, total_bytes // 100 * RESERVE_PERCENT)


def target(free_bytes, total_bytes, mib=0):
    """Bytes to cover, rounded down to whole pages."""
    t = mib << 20 if mib else max(0, free_bytes - reserve(total_bytes))
    return t // PAGE_BYTES * PAGE_BYTES


def plan(total, chunk_bytes=CHUNK_BYTES):
    """``[(bytes, word0)]``: chunks of ``chunk_bytes``, the last one shorter
    when ``total`` is no multiple; ``word0`` is the bytes before it / 8."""
    assert total % 16 == 0 and chunk_bytes % 16 == 0 and chunk_bytes > 0
    return [
        (min(chunk_bytes, total - at), at // 8) for at in range(0, total, chunk_bytes)
    ]


def chunk_of(chunks, word):
    for c, (nbytes, word0) in enumerate(chunks):
        if word0 <= word < word0 + nbytes // 8:
            return c
    raise ValueError(f"word {word} outside the coverage")


# ---------------------------------------------------------------------------
# round schedule
# ---------------------------------------------------------------------------
def round_of(seed, r):
    """``(pattern name, seed)`` of round ``r``."""
    return S.PATTERNS[r % 4], S.mix_int((seed + r // 4) & _M64)


def descending(pas, rounds):
    """Whether pass ``pas`` of a run of ``rounds`` rounds goes downwards: in
    the odd cycles of the round it writes; the closing verify writes none
    and goes the way of the round it reads."""
    return bool((min(pas, rounds - 1) // 4) & 1)


def words(seed, r, word0, nwords):
    """Global words ``word0 .. word0 + nwords - 1`` after round ``r``."""
    pattern, s = round_of(seed, r)
    w = np.arange(nwords, dtype=np.uint64) + np.uint64(word0)
    s = np.uint64(s)
    if pattern.startswith("addr"):
        out = w ^ s
    else:
        with np.errstate(over="ignore"):
            out = S.mix(w + s)
    return ~out if pattern.endswith("_inv") else out


def word(seed, r, w):
    return int(words(seed, r, w, 1)[0])


def contents(seed, r, chunks):
    """The bytes of every chunk after round ``r``."""
    return [
        words(seed, r, word0, nbytes // 8).astype("<u8").tobytes()
        for nbytes, word0 in chunks
    ]


# ---------------------------------------------------------------------------
# what a run with flips must report
# ---------------------------------------------------------------------------
def expected(seed, rounds, chunks, flips):
    """What a run of ``rounds`` rounds over ``chunks`` must report when every
    ``(pass, word, mask)`` of ``flips`` is XORed in before that pass reads.
    The first pass with a mismatch is the last one; later flips never
    happen. Masks on one word in one pass combine. Returns a dict with the
    fields of the binding's result that depend on the flips, ``records`` as a
    set (all of them, not the first 64), and ``contents``: the bytes every
    chunk holds when the run ends."""
    by_pass = {}
    for pas, w, mask in flips:
        assert 1 <= pas <= rounds
        chunk_of(chunks, w)
        by_word = by_pass.setdefault(pas, {})
        by_word[w] = by_word.get(w, 0) ^ (mask & _M64)
    last = rounds  # the closing verify
    hit = {}
    for pas in sorted(by_pass):
        hit = {w: m for w, m in by_pass[pas].items() if m}
        if hit:
            last = pas
            break
    records = {
        (last, w, word(seed, last - 1, w) ^ m, word(seed, last - 1, w))
        for w, m in hit.items()
    }
    flipped_or = 0
    per_chunk, pages = {}, set()
    for w, m in hit.items():
        flipped_or |= m
        c = chunk_of(chunks, w)
        per_chunk[c] = per_chunk.get(c, 0) + 1
        pages.add((c, (w - chunks[c][1]) * 8 // PAGE_BYTES))
    # a march pass rewrites every word it read; the verify leaves the flip
    written = last if last < rounds else rounds - 1
    held = [np.frombuffer(b, dtype="<u8").copy() for b in contents(seed, written, chunks)]
    if last == rounds:
        for w, m in hit.items():
            c = chunk_of(chunks, w)
            held[c][w - chunks[c][1]] ^= np.uint64(m)
    return {
        "ok": not hit,
        "rounds": written + 1,
        "passes": last + 1,
        "mismatches": len(hit),
        "flipped_or": flipped_or,
        "bad_chunks": sorted(per_chunk.items()),
        "bad_pages": len(pages),
        "bad_pages_first": sorted(pages)[:PAGES_FIRST],
        "records": records,
        "contents": [h.tobytes() for h in held],
    }
