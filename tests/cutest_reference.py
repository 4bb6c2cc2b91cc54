"""numpy references for the per-CU self-test (``cpp/cutest_kernels.hpp``).

numpy only and no GPU import: ``test_cu_selftest`` checks this module on the
CPU, ``test_cu_selftest_gpu`` compares the kernel and the host aggregation
with it.

Block ``b`` of ``cu_test`` fills the first ``nwords`` 64-bit words of its
CU's LDS with the patterns of ``selftest_reference`` under the seed
``seed + b`` (mod 2^64), and leaves one 32-byte record of eight little-endian
uint32: ``hw_id, xcc_id, block, simd_mask, lds_mismatches, mfma_mismatches,
0, 0``.
"""

import numpy as np

import selftest_reference as S

LDS_BYTES = 163840  # all of a CU's LDS on gfx950
RECORD_BYTES = 32
WAVES = 4  # per block
_M64 = (1 << 64) - 1


def lds_words(pattern, nwords, seed, block):
    """The LDS words of one block while it holds ``pattern``."""
    return S.pattern_words(pattern, nwords, (seed + block) & _M64)


def expected_lds_records(seed, flips, nwords):
    """What the LDS test must report after ``flips`` (``(block, pattern,
    word, mask)``): the set of ``(block, pattern, word, got, want)``. A flip
    shows in its own block and pattern only; masks on one word combine."""
    groups = {}
    for block, pattern, word, mask in flips:
        groups.setdefault((block, pattern), []).append((word, mask))
    out = set()
    for (block, pattern), pairs in groups.items():
        recs = S.expected_records(pattern, (seed + block) & _M64, pairs, nwords)
        out |= {(block, pattern, w, got, want) for w, got, want in recs}
    return out


def lds_mismatches_per_block(records, blocks):
    """Mismatching words per block from a complete set of LDS records."""
    out = [0] * blocks
    for block, *_ in records:
        out[block] += 1
    return out


def expected_mfma_records(truth, want, blocks):
    """What the known-answer test must report when the table expects
    ``want`` and the matrix pipes give ``truth`` (both float32
    ``(16, 64, 4)``): ``(block, wave, vector, lane, slot, got_bits,
    want_bits)`` for every wave of every block, since each wave runs the
    whole table."""
    got_bits = np.ascontiguousarray(truth, dtype=np.float32).view(np.uint32)
    want_bits = np.ascontiguousarray(want, dtype=np.float32).view(np.uint32)
    out = set()
    for v, lane, slot in zip(*np.nonzero(got_bits != want_bits)):
        g, w = int(got_bits[v, lane, slot]), int(want_bits[v, lane, slot])
        for b in range(blocks):
            for wave in range(WAVES):
                out.add((b, wave, int(v), int(lane), int(slot), g, w))
    return out


# ---------------------------------------------------------------------------
# per-block records
# ---------------------------------------------------------------------------
def decode(hw_id, xcc_id):
    """``(xcc, se, sh, cu)`` from the HW_REG_HW_ID and HW_REG_XCC_ID words:
    CU_ID 11:8, SH_ID 12, SE_ID 14:13, XCC_ID 3:0 of its own register."""
    return (
        xcc_id & 0xF,
        (hw_id >> 13) & 0x3,
        (hw_id >> 12) & 0x1,
        (hw_id >> 8) & 0xF,
    )


def simd_id(hw_id):
    """SIMD_ID, bits 5:4 of HW_REG_HW_ID."""
    return (hw_id >> 4) & 0x3


def make_hw_id(se, sh, cu, simd=0, wave=0):
    """A HW_REG_HW_ID word with those fields, everything else 0."""
    assert se < 4 and sh < 2 and cu < 16 and simd < 4 and wave < 16
    return (se << 13) | (sh << 12) | (cu << 8) | (simd << 4) | wave


def pack_record(hw_id, xcc_id, block, simd_mask, lds=0, mfma=0):
    return np.array(
        [hw_id, xcc_id, block, simd_mask, lds, mfma, 0, 0], dtype="<u4"
    ).tobytes()


def parse_records(records_bytes):
    """``(blocks, 8)`` uint32 from the records' bytes (no guards)."""
    assert len(records_bytes) % RECORD_BYTES == 0
    return np.frombuffer(bytes(records_bytes), dtype="<u4").reshape(-1, 8)


def aggregate(records_bytes):
    """What the host's ``aggregate`` derives from the per-block records:
    ``covered``, ``per_xcc``, ``blocks_per_cu_min/max``,
    ``simds_per_cu_min`` and the sorted ``bad_cus``."""
    rec = parse_records(records_bytes)
    per_cu = {}
    for b, (hw, xcc, block, simd_mask, lds, mfma, pad0, pad1) in enumerate(
        rec.tolist()
    ):
        if block != b or pad0 or pad1:
            raise ValueError(f"block {b} left no record")
        c = per_cu.setdefault(decode(hw, xcc), [0, 0, 0, 0])
        c[0] += 1
        c[1] |= simd_mask
        c[2] += lds
        c[3] += mfma
    per_xcc = {}
    for xcc, _, _, _ in per_cu:
        per_xcc[xcc] = per_xcc.get(xcc, 0) + 1
    return {
        "covered": len(per_cu),
        "per_xcc": per_xcc,
        "blocks_per_cu_min": min(c[0] for c in per_cu.values()),
        "blocks_per_cu_max": max(c[0] for c in per_cu.values()),
        "simds_per_cu_min": min(bin(c[1]).count("1") for c in per_cu.values()),
        "bad_cus": [
            {
                "xcc": k[0],
                "se": k[1],
                "sh": k[2],
                "cu": k[3],
                "blocks": c[0],
                "lds_mismatches": c[2],
                "mfma_mismatches": c[3],
            }
            for k, c in sorted(per_cu.items())
            if c[2] or c[3]
        ],
    }


AGGREGATE_KEYS = (
    "covered",
    "per_xcc",
    "blocks_per_cu_min",
    "blocks_per_cu_max",
    "simds_per_cu_min",
    "bad_cus",
)
