"""The per-CU self-test on an MI355X: ``cu_test`` against the numpy patterns
and a known-answer table built with ``hip_reference``'s lane maps, the host
aggregation against its Python mirror, coverage against the independent
``cu_footprint``, and the path from the child process up to the driver.

No test provokes a fault: what is injected is wrong data at valid LDS word
indices (checked on the host before any launch) or a wrong expectation,
never a wrong address. The per-block records lie between canary guards that
come back with the result.
"""

import numpy as np
import pytest

# torch must load before the system-ROCm-linked _hiphealth extension (see
# test_gpu.py): import order is load-bearing.
import torch  # noqa: F401

import cutest_reference as C
import hip_reference as R
import selftest_reference as S

pytestmark = pytest.mark.gpu

SEED = 0x0123456789ABCDEF
WRAPPING_SEED = 2**64 - 2  # block 2 of a grid runs under seed 0
MAX_FLIPS = 4096


@pytest.fixture(scope="module")
def hh():
    from k8s_dra_driver_amd import _hiphealth

    assert _hiphealth.device_count() >= 1
    assert _hiphealth.PROBE_CANARY == R.CANARY
    assert _hiphealth.SELFTEST_MAX_RECORDS == S.MAX_RECORDS
    assert _hiphealth.SELFTEST_KAT_VECTORS == S.KAT_VECTORS
    assert _hiphealth.CUTEST_LDS_BYTES == C.LDS_BYTES
    return _hiphealth


# built once, shared and never modified
@pytest.fixture(scope="module")
def tables():
    return S.kat_tables()


def probe(hh, tables, blocks, lds_bytes, flips=(), seed=SEED, want=None):
    """One ``cu_selftest_probe`` call. Checks what holds for every call:
    intact guards, every block's own record, and a dict that equals the
    Python aggregation of the raw records. Returns ``(dict, records)``,
    records as ``(blocks, 8)`` uint32."""
    a, b, c, w = tables
    if want is not None:
        w = want
    raw, d = hh.cu_selftest_probe(
        0, a.tobytes(), b.tobytes(), c.tobytes(), w.tobytes(), seed, blocks,
        lds_bytes, list(flips),
    )
    guard = hh.PROBE_GUARD_BYTES
    assert len(raw) == guard + C.RECORD_BYTES * blocks + guard
    buf = np.frombuffer(raw, dtype=np.uint8)
    assert (buf[:guard] == hh.PROBE_CANARY).all()
    assert (buf[-guard:] == hh.PROBE_CANARY).all()
    rec = C.parse_records(raw[guard:-guard])
    assert (rec[:, 2] == np.arange(blocks)).all()  # its own block index
    assert ((rec[:, 3] != 0) & (rec[:, 3] <= 0xF)).all()  # simd_mask
    assert (rec[:, 1] < 8).all()  # XCC_ID, nothing else of that register
    assert (rec[:, 6:] == 0).all()
    want_agg = C.aggregate(raw[guard:-guard])
    assert {k: d[k] for k in C.AGGREGATE_KEYS} == want_agg
    assert d["blocks"] == blocks and d["lds_bytes"] == lds_bytes
    assert d["seed"] == seed and d["device"] == 0
    assert d["lds"]["checked_words"] == blocks * 4 * lds_bytes // 8
    assert d["mfma"]["checked"] == blocks * 4 * 16 * 64 * 4
    assert d["ok"] is (d["lds"]["mismatches"] == 0 and d["mfma"]["mismatches"] == 0)
    assert int(rec[:, 4].sum()) == d["lds"]["mismatches"]
    assert int(rec[:, 5].sum()) == d["mfma"]["mismatches"]
    return d, rec


# ---------------------------------------------------------------------------
# cu_test, one launch between guards
# ---------------------------------------------------------------------------
# one element, one short of a trip of 256 lanes, one trip, one over, one
# short of all of LDS, all of it
@pytest.mark.parametrize("lds_bytes", [16, 4080, 4096, 4112, 163824, 163840])
@pytest.mark.parametrize("blocks", [1, 3])
def test_known_answers_and_clean_lds(hh, tables, blocks, lds_bytes):
    d, rec = probe(hh, tables, blocks, lds_bytes)
    assert d["ok"] is True
    assert d["lds"]["mismatches"] == 0 and d["lds"]["records"] == []
    assert d["mfma"]["mismatches"] == 0 and d["mfma"]["records"] == []
    assert d["bad_cus"] == []
    assert (rec[:, 4:6] == 0).all()


@pytest.mark.parametrize("lds_bytes", [16, 4112, 163840])
@pytest.mark.parametrize("pattern", ["addr", "hash_inv"])
def test_lds_flips_are_found_where_they_are(hh, tables, pattern, lds_bytes):
    """Three single-bit flips per block: bit 0 of the first word, bit 63 of
    the last, bit 31 of word 512 (the first word of the element a lane
    reaches on its second trip) or, in a shorter region, of the middle
    word. In the region of one element the middle word is the last one:
    its two masks combine and the block has 2 mismatching words, not 3."""
    blocks = 3
    nwords = lds_bytes // 8
    boundary = 512 if nwords > 512 else nwords // 2
    flips = [
        (b, pattern, word, mask)
        for b in range(blocks)
        for word, mask in [(0, 1), (nwords - 1, 1 << 63), (boundary, 1 << 31)]
    ]
    want_recs = C.expected_lds_records(WRAPPING_SEED, flips, nwords)
    per_block = C.lds_mismatches_per_block(want_recs, blocks)
    assert per_block == [len({0, nwords - 1, boundary})] * blocks

    d, rec = probe(hh, tables, blocks, lds_bytes, flips, seed=WRAPPING_SEED)
    assert d["ok"] is False
    assert d["lds"]["mismatches"] == len(want_recs), d["lds"]
    records = d["lds"]["records"]
    assert len(records) == len(want_recs)
    assert set(records) == want_recs
    # nothing shows in the other three patterns
    assert {p for _, p, _, _, _ in records} == {pattern}
    masks = {}
    for b, _, word, mask in flips:
        masks[b, word] = masks.get((b, word), 0) ^ mask
    for b, _, word, got, want in records:
        assert got ^ want == masks[b, word]
    assert rec[:, 4].tolist() == per_block
    assert d["mfma"]["mismatches"] == 0 and (rec[:, 5] == 0).all()
    # probe() has compared bad_cus with the reference aggregation
    assert d["bad_cus"]
    assert sum(c["lds_mismatches"] for c in d["bad_cus"]) == len(want_recs)
    assert sum(c["blocks"] for c in d["bad_cus"]) == blocks
    assert all(c["mfma_mismatches"] == 0 for c in d["bad_cus"])


def test_a_wrong_expectation_is_reported_by_every_wave(hh, tables):
    want = tables[3]
    vector, lane, slot = 3, 37, 2
    truth = want[vector, lane, slot]
    wrong = want.copy()
    wrong[vector, lane, slot] = truth + np.float32(0.0625)  # one unit of 2^-4
    assert wrong[vector, lane, slot] != truth
    blocks = 5
    d, rec = probe(hh, tables, blocks, 4096, want=wrong)
    truth_bits = int(truth.view(np.uint32))
    wrong_bits = int(wrong[vector, lane, slot].view(np.uint32))
    assert d["mfma"]["mismatches"] == blocks * 4
    expected = {
        (b, w, vector, lane, slot, truth_bits, wrong_bits)
        for b in range(blocks)
        for w in range(4)
    }
    assert expected == C.expected_mfma_records(want, wrong, blocks)
    assert len(d["mfma"]["records"]) == blocks * 4
    assert set(d["mfma"]["records"]) == expected
    assert rec[:, 5].tolist() == [4] * blocks
    assert d["lds"]["mismatches"] == 0 and (rec[:, 4] == 0).all()
    assert sum(c["mfma_mismatches"] for c in d["bad_cus"]) == blocks * 4


def test_record_cap(hh, tables):
    lds_bytes = 16 * (3 * 256 + 5)
    nwords = lds_bytes // 8
    rng = np.random.default_rng(64)
    words = rng.choice(nwords, size=100, replace=False)
    flips = [(1, "hash", int(w), 1 << int(rng.integers(64))) for w in words]
    want_recs = C.expected_lds_records(SEED, flips, nwords)
    assert len(want_recs) == 100
    d, rec = probe(hh, tables, 2, lds_bytes, flips)
    assert d["lds"]["mismatches"] == 100
    records = d["lds"]["records"]
    assert len(records) == S.MAX_RECORDS
    assert len(set(records)) == S.MAX_RECORDS
    assert set(records) <= want_recs
    assert rec[:, 4].tolist() == [0, 100]


def test_arguments_are_validated_before_any_launch(hh, tables):
    a, b, c, want = (t.tobytes() for t in tables)
    names = (
        "device", "a_tab", "b_tab", "c_tab", "want_tab", "seed", "blocks",
        "lds_bytes", "flips",
    )
    ok = dict(zip(names, (0, a, b, c, want, SEED, 1, 64, [])))

    def call(**kw):
        args = dict(ok)
        args.update(kw)
        return hh.cu_selftest_probe(*[args[k] for k in names])

    assert call()[1]["ok"] is True
    for bad in (
        dict(a_tab=a[:-2]),
        dict(b_tab=b + b"\0\0"),
        dict(c_tab=c[:-4]),
        dict(want_tab=b""),
        dict(lds_bytes=0),
        dict(lds_bytes=24),
        dict(lds_bytes=C.LDS_BYTES + 16),
        dict(lds_bytes=-16),
        dict(blocks=0),
        dict(blocks=hh.FOOTPRINT_MAX_BLOCKS + 1),
        dict(flips=[(0, "addr", 8, 1)]),  # 64 bytes = words 0..7
        dict(flips=[(0, "addr", -1, 1)]),
        dict(flips=[(1, "addr", 0, 1)]),  # the grid has block 0 only
        dict(flips=[(-1, "addr", 0, 1)]),
        dict(flips=[(0, "addr", 0, 1)] * (MAX_FLIPS + 1)),
        dict(flips=[(0, "walking_ones", 0, 1)]),
        dict(device=-1),
        dict(device=hh.device_count()),
    ):
        with pytest.raises(ValueError):
            call(**bad)
    assert call(flips=[(0, "addr", 7, 1)] * MAX_FLIPS)[1]["ok"] is True  # cancel
    for kw in (
        dict(device=-1),
        dict(device=hh.device_count()),
        dict(blocks=-1),
        dict(blocks=hh.FOOTPRINT_MAX_BLOCKS + 1),
    ):
        with pytest.raises(ValueError):
            hh.cu_selftest(**kw)


# ---------------------------------------------------------------------------
# production path, default grid
# ---------------------------------------------------------------------------
def test_default_grid_covers_what_cu_footprint_sees(hh, tables):
    """Coverage is measured against ``cu_footprint`` in the same process:
    both see the same CU mask, whatever the machine sets."""
    foot = hh.cu_footprint(0)
    r = hh.cu_selftest(0)
    print(
        f"cu_selftest: kernel {r['kernel_ms']:.3f} ms, {r['blocks']} blocks, "
        f"covered {r['covered']} of {r['multi_processor_count']} "
        f"(cu_footprint {foot['count']}), simds per CU min "
        f"{r['simds_per_cu_min']}, blocks per CU "
        f"{r['blocks_per_cu_min']}..{r['blocks_per_cu_max']}"
    )
    assert r["ok"] is True and r["bad_cus"] == []
    assert r["lds"]["mismatches"] == 0 and r["mfma"]["mismatches"] == 0
    assert r["lds_bytes"] == C.LDS_BYTES == hh.CUTEST_LDS_BYTES
    info = hh.device_info(0)
    assert r["multi_processor_count"] == info["multi_processor_count"]
    assert r["blocks"] == min(
        hh.CUTEST_BLOCKS_PER_CU * info["multi_processor_count"],
        hh.FOOTPRINT_MAX_BLOCKS,
    )
    assert r["covered"] == foot["count"]
    assert r["per_xcc"] == foot["per_xcc"]
    # the same grid through the hook, for the records themselves
    d, rec = probe(hh, tables, r["blocks"], C.LDS_BYTES)
    cus = {C.decode(int(h), int(x)) for h, x in rec[:, :2]}
    assert cus == set(foot["cus"])
    assert d["covered"] == foot["count"] and d["ok"] is True


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


def test_the_child_passes_with_the_per_cu_stage(hh, real_lib):
    from k8s_dra_driver_amd import selftest

    gpu = real_lib.enumerate()[0]
    res = selftest.run(gpu, mib=64, timeout_s=120, per_cu=True)
    print("child --per-cu:", res.outcome, f"{res.seconds:.2f}s", res.error)
    assert res.outcome == "pass", res.error
    assert res.findings() == []
    assert res.report["ok"] is True
    cu = res.report["cu"]
    assert cu["covered"] > 0 and cu["bad_cus"] == []
    assert cu["lds_bytes"] == C.LDS_BYTES


def test_driver_startup_selftest_per_cu_on_the_real_hal(real_lib, tmp_path):
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
        results = driver.run_startup_selftest(mib=64, per_cu=True)
        assert results == {0: "pass"}
        assert driver.health.findings(0) == []
        value = driver.metrics.registry.get_sample_value
        assert value("dra_gpu_selftest_cus_covered", {"gpu": "0"}) > 0
        assert value("dra_gpu_selftest_cus_bad", {"gpu": "0"}) == 0
    finally:
        driver.shutdown(unpublish=False)
