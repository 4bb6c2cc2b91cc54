"""The startup self-test on an MI355X: the fill and verify kernels against
the numpy patterns byte for byte, the MFMA known-answer kernel against a
table built with ``hip_reference``'s lane maps, and the path from the
child process up to the driver.

No test provokes a fault: what is injected is wrong data at valid word
indices (checked on the host before any launch), never a wrong address.
Every region lies between canary guards that come back with the result.
"""

import numpy as np
import pytest

# torch must load before the system-ROCm-linked _hiphealth extension (see
# test_gpu.py): import order is load-bearing.
import torch  # noqa: F401

import hip_reference as R
import selftest_reference as S

pytestmark = pytest.mark.gpu

SEED = 0x0123456789ABCDEF


@pytest.fixture(scope="module")
def hh():
    from k8s_dra_driver_amd import _hiphealth

    assert _hiphealth.device_count() >= 1
    assert _hiphealth.PROBE_CANARY == R.CANARY
    assert _hiphealth.SELFTEST_MAX_RECORDS == S.MAX_RECORDS
    assert _hiphealth.SELFTEST_KAT_VECTORS == S.KAT_VECTORS
    return _hiphealth


def _copy_sizes(blocks):
    """The 13 element counts of test_hip_kernels' copy tests."""
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


# ---------------------------------------------------------------------------
# mem_fill / mem_verify
# ---------------------------------------------------------------------------
class TestMemoryKernels:
    @pytest.mark.parametrize("size", list(_copy_sizes(1)))
    @pytest.mark.parametrize("blocks", [1, 3])
    @pytest.mark.parametrize("pattern", S.PATTERNS)
    def test_fill_is_exact(self, hh, pattern, blocks, size):
        n = _copy_sizes(blocks)[size]
        out, count, records = hh.memtest_probe(
            0, 16 * n, pattern, SEED, blocks, [], "fill"
        )
        want = S.pattern_bytes(pattern, 16 * n, SEED)
        problems = R.check_copy(out, want, hh.PROBE_GUARD_BYTES)
        assert not problems, (pattern, blocks, n, problems)
        assert count == 0 and records == []

    @pytest.mark.parametrize("size", ["1", "257", "3*stride+5"])
    @pytest.mark.parametrize("blocks", [1, 3])
    @pytest.mark.parametrize("pattern", ["addr", "hash_inv"])
    def test_verify_finds_exactly_what_was_flipped(self, hh, pattern, blocks, size):
        """Three single-bit flips: bit 0 of the first word, bit 63 of the
        last, one bit of a word in between. The count is the number of
        distinct words flipped: 3, except for the region of one element,
        whose two words cannot hold three (the last word takes two of the
        flips there and the count is 2)."""
        n = _copy_sizes(blocks)[size]
        nwords = 2 * n
        stride = 256 * blocks
        # first word, last word, and the first word of the element at
        # which a lane starts its second trip (inside the region when the
        # region is that long, else the middle word)
        boundary = 2 * stride if n > stride else nwords // 2
        flips = [(0, 1), (nwords - 1, 1 << 63), (boundary, 1 << 31)]
        want_recs = S.expected_records(pattern, SEED, flips, nwords)
        assert len(want_recs) == len({w for w, _ in flips})

        out, count, records = hh.memtest_probe(
            0, 16 * n, pattern, SEED, blocks, flips, "verify"
        )
        assert count == len(want_recs), (count, records)
        assert len(records) == count
        assert set(records) == want_recs
        masks = {}
        for w, m in flips:
            masks[w] = masks.get(w, 0) ^ m
        for word, got, want in records:
            assert got ^ want == masks[word]
        # verify wrote nothing: the region is the pattern with the flips,
        # every other byte untouched, and the guards are intact
        clean = S.pattern_bytes(pattern, 16 * n, SEED)
        problems = R.check_copy(out, S.apply_flips(clean, flips), hh.PROBE_GUARD_BYTES)
        assert not problems, problems

    @pytest.mark.parametrize("blocks", [1, 3])
    @pytest.mark.parametrize("pattern", ["addr", "hash_inv"])
    def test_no_flips_no_mismatch(self, hh, pattern, blocks):
        n = 3 * 256 * blocks + 5
        out, count, records = hh.memtest_probe(
            0, 16 * n, pattern, SEED, blocks, [], "verify"
        )
        assert count == 0 and records == []
        want = S.pattern_bytes(pattern, 16 * n, SEED)
        assert not R.check_copy(out, want, hh.PROBE_GUARD_BYTES)

    def test_a_wrong_seed_is_seen_everywhere(self, hh):
        """The comparator looks at every word: a region filled as the
        pattern of one seed and flipped into that of another differs in
        every word."""
        n = 300
        flips = [(w, 1) for w in range(2 * n)]  # addr, seed ^ 1
        _, count, records = hh.memtest_probe(0, 16 * n, "addr", SEED, 2, flips, "verify")
        assert count == 2 * n
        assert len(records) == S.MAX_RECORDS

    def test_record_cap(self, hh):
        n = 3 * 256 + 5
        rng = np.random.default_rng(64)
        words = rng.choice(2 * n, size=100, replace=False)
        flips = [(int(w), 1 << int(rng.integers(64))) for w in words]
        want_recs = S.expected_records("hash", SEED, flips, 2 * n)
        assert len(want_recs) == 100
        _, count, records = hh.memtest_probe(0, 16 * n, "hash", SEED, 3, flips, "verify")
        assert count == 100
        assert len(records) == S.MAX_RECORDS
        assert len(set(records)) == S.MAX_RECORDS
        assert set(records) <= want_recs

    def test_arguments_are_validated(self, hh):
        ok = (0, 64, "addr", SEED, 1, [], "verify")

        def call(**kw):
            names = ("device", "nbytes", "pattern", "seed", "blocks", "flips", "stage")
            args = dict(zip(names, ok))
            args.update(kw)
            return hh.memtest_probe(*[args[k] for k in names])

        assert call()[1] == 0
        with pytest.raises(ValueError):
            call(pattern="walking_ones")
        with pytest.raises(ValueError):
            call(nbytes=24)
        with pytest.raises(ValueError):
            call(nbytes=(64 << 20) + 16)
        with pytest.raises(ValueError):
            call(blocks=0)
        with pytest.raises(ValueError):
            call(blocks=1 << 20)
        with pytest.raises(ValueError):
            call(flips=[(8, 1)])  # 64 bytes = words 0..7
        with pytest.raises(ValueError):
            call(flips=[(-1, 1)])
        with pytest.raises(ValueError):
            call(nbytes=0, flips=[(0, 1)])
        with pytest.raises(ValueError):
            call(flips=[(0, 1)] * 4097)
        with pytest.raises(ValueError):
            call(stage="scrub")
        with pytest.raises(ValueError):
            call(device=-1)
        with pytest.raises(ValueError):
            call(device=hh.device_count())


# ---------------------------------------------------------------------------
# mfma_kat
# ---------------------------------------------------------------------------
class TestMfmaKat:
    @pytest.fixture(scope="class")
    def tables(self):
        return S.kat_tables()

    @staticmethod
    def _run(hh, a, b, c, want, blocks):
        return hh.mfma_kat_probe(
            0, a.tobytes(), b.tobytes(), c.tobytes(), want.tobytes(), blocks
        )

    @pytest.mark.parametrize("blocks", [1, 5])
    def test_known_answers_hold(self, hh, tables, blocks):
        count, records, checked = self._run(hh, *tables, blocks)
        assert count == 0, records[:4]
        assert records == []
        assert checked == blocks * 4 * 256

    def test_a_wrong_expectation_is_reported_where_it_is(self, hh, tables):
        a, b, c, want = tables
        vector, lane, slot = 3, 37, 2
        truth = want[vector, lane, slot]
        wrong = want.copy()
        wrong[vector, lane, slot] = truth + np.float32(0.0625)  # one unit of 2^-4
        assert wrong[vector, lane, slot] != truth
        blocks = 10  # 40 waves: vector 3 is taken by waves 3, 19, 35
        count, records, checked = self._run(hh, a, b, c, wrong, blocks)
        truth_bits = int(truth.view(np.uint32))
        wrong_bits = int(wrong[vector, lane, slot].view(np.uint32))
        assert count == 3
        assert sorted(records) == [
            (w, lane, slot, truth_bits, wrong_bits) for w in (3, 19, 35)
        ]
        assert checked == blocks * 4 * 256

    def test_bad_table_lengths_are_rejected(self, hh, tables):
        a, b, c, want = (t.tobytes() for t in tables)
        for bad in (
            (a[:-2], b, c, want),
            (a, b + b"\0\0", c, want),
            (a, b, c[:-4], want),
            (a, b, c, b""),
        ):
            with pytest.raises(ValueError):
                hh.mfma_kat_probe(0, *bad, 1)
        with pytest.raises(ValueError):
            hh.mfma_kat_probe(0, a, b, c, want, 0)
        with pytest.raises(ValueError):
            hh.mfma_kat_probe(hh.device_count(), a, b, c, want, 1)


# ---------------------------------------------------------------------------
# production path
# ---------------------------------------------------------------------------
def test_selftest_passes_on_a_healthy_gpu(hh):
    r = hh.selftest(0, mib=64)
    print("selftest(mib=64):", r)
    assert r["ok"] is True
    assert r["bytes"] == 64 << 20
    assert [p["pattern"] for p in r["memory"]] == list(S.PATTERNS)
    for p in r["memory"]:
        assert p["mismatches"] == 0 and p["records"] == []
        assert p["fill_gbs"] > 0 and p["verify_gbs"] > 0  # reported, not judged
    assert r["mfma"]["mismatches"] == 0
    assert r["mfma"]["checked"] == r["mfma"]["blocks"] * 256 * 4 > 0
    info = hh.device_info(0)
    assert r["mfma"]["blocks"] == 4 * info["multi_processor_count"]


def test_selftest_validates_before_it_allocates(hh):
    with pytest.raises(ValueError):
        hh.selftest(0, mib=0)
    with pytest.raises(ValueError):
        hh.selftest(0, mib=64, blocks=-1)
    with pytest.raises(ValueError):
        hh.selftest(hh.device_count(), mib=64)
    with pytest.raises(ValueError):
        hh.pci_bus_id(hh.device_count())


@pytest.fixture(scope="module")
def real_lib():
    from k8s_dra_driver_amd.hal.amdsmi import AmdSmiDeviceLib

    lib = AmdSmiDeviceLib()
    lib.open()
    yield lib
    lib.close()


class TestChildEndToEnd:
    def test_the_real_gpu_passes(self, hh, real_lib):
        from k8s_dra_driver_amd import selftest

        gpu = real_lib.enumerate()[0]
        assert gpu.pcie_bdf
        visible = [hh.pci_bus_id(d).lower() for d in range(hh.device_count())]
        assert gpu.pcie_bdf.lower() in visible
        res = selftest.run(gpu, mib=64, timeout_s=120)
        print("child:", res.outcome, f"{res.seconds:.2f}s", res.error)
        assert res.outcome == "pass", res.error
        assert res.findings() == []
        assert res.report["bdf"] == gpu.pcie_bdf.lower()
        assert res.report["bytes"] == 64 << 20

    def test_an_address_nobody_has_is_a_selftest_error(self):
        from k8s_dra_driver_amd import selftest

        class Gpu:
            index = 0
            pcie_bdf = "ffff:ff:1f.7"

        res = selftest.run(Gpu(), mib=64, timeout_s=120)
        assert res.outcome == "error"
        assert "exit 2" in res.error and "ffff:ff:1f.7" in res.error
        assert [f.reason for f in res.findings()] == ["SelftestError"]


def test_driver_startup_selftest_on_the_real_hal(real_lib, tmp_path):
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
        results = driver.run_startup_selftest(mib=64)
        driver.startup()
        assert results == {0: "pass"}
        assert driver.health.unhealthy_gpus == set()
        assert not any(
            f.reason.startswith("Selftest") for f in driver.health.findings(0)
        )
        devices = [
            d
            for s in kube.list_resource_slices("gpu.amd.com")
            for d in s["spec"]["devices"]
        ]
        assert devices and not any("taints" in d for d in devices)
        value = driver.metrics.registry.get_sample_value
        runs = "dra_gpu_selftest_runs_total"
        assert value(runs, {"gpu": "0", "result": "pass"}) == 1
        assert value("dra_gpu_selftest_seconds", {"gpu": "0"}) > 0
    finally:
        driver.shutdown(unpublish=False)
