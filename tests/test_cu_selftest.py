"""The per-CU self-test without a GPU: the numpy reference on hand-written
records, the parent half of ``k8s_dra_driver_amd.selftest`` on a stub child
with a ``cu`` part, the driver's startup pass, and the CLIs."""

import json

import numpy as np
import pytest

import cutest_reference as C
import selftest_reference as S
from k8s_dra_driver_amd import ctl, selftest
from k8s_dra_driver_amd.plugin import main as plugin_main
from test_selftest import Gpu, make_driver, report, sample, spawn_returning, stub_runner


# ---------------------------------------------------------------------------
# reference
# ---------------------------------------------------------------------------
class TestReference:
    def test_decode_reads_the_documented_fields(self):
        # SE_ID 14:13 = 2, SH_ID 12 = 1, CU_ID 11:8 = 9, SIMD_ID 5:4 = 3
        hw = (2 << 13) | (1 << 12) | (9 << 8) | (3 << 4) | 0x7
        assert C.make_hw_id(2, 1, 9, simd=3, wave=7) == hw
        assert C.decode(hw, 5) == (5, 2, 1, 9)
        assert C.simd_id(hw) == 3
        # queue, pipe and wave-slot bits do not name a CU
        assert C.decode(hw | 0xFFFF80C0, 0xFFFFFFF5) == (5, 2, 1, 9)

    def test_block_words_are_the_pattern_of_seed_plus_block(self):
        seed = 2**64 - 1  # block 1 wraps to seed 0
        assert np.array_equal(
            C.lds_words("addr", 6, seed, 1), np.arange(6, dtype=np.uint64)
        )
        assert np.array_equal(
            C.lds_words("hash_inv", 6, 10, 3), S.pattern_words("hash_inv", 6, 13)
        )

    def test_lds_records_stay_in_their_block_and_pattern(self):
        flips = [(0, "addr", 3, 1), (2, "addr", 3, 1 << 63), (2, "hash", 0, 2)]
        recs = C.expected_lds_records(100, flips, 8)
        h = int(S.pattern_words("hash", 8, 102)[0])
        assert recs == {
            (0, "addr", 3, (3 ^ 100) ^ 1, 3 ^ 100),
            (2, "addr", 3, (3 ^ 102) ^ (1 << 63), 3 ^ 102),
            (2, "hash", 0, h ^ 2, h),
        }
        assert C.lds_mismatches_per_block(recs, 3) == [1, 0, 2]
        # masks on one word combine, and cancel
        twice = [(1, "addr", 0, 1), (1, "addr", 0, 1)]
        assert C.expected_lds_records(0, twice, 8) == set()

    def test_a_wrong_expectation_shows_in_every_wave_of_every_block(self):
        truth = np.zeros((16, 64, 4), dtype=np.float32)
        truth[3, 37, 2] = 1.5
        want = truth.copy()
        want[3, 37, 2] = 1.5625
        recs = C.expected_mfma_records(truth, want, 2)
        t, w = 0x3FC00000, 0x3FC80000
        assert recs == {(b, v, 3, 37, 2, t, w) for b in range(2) for v in range(4)}
        assert C.expected_mfma_records(truth, truth, 5) == set()

    def test_aggregate_on_hand_written_records(self):
        cu_a = C.make_hw_id(1, 0, 4, simd=0)
        cu_a_other_wave = C.make_hw_id(1, 0, 4, simd=2, wave=5)
        cu_b = C.make_hw_id(3, 1, 15, simd=1)
        raw = b"".join(
            [
                # two blocks on xcc 0 se 1 sh 0 cu 4, different SIMDs
                C.pack_record(cu_a, 0, 0, 0b0011),
                C.pack_record(cu_b, 7, 1, 0b1111, lds=2, mfma=4),
                C.pack_record(cu_a_other_wave, 0, 2, 0b0100),
                # the same HW_ID on another XCC is another CU
                C.pack_record(cu_a, 1, 3, 0b0001),
            ]
        )
        assert C.aggregate(raw) == {
            "covered": 3,
            "per_xcc": {0: 1, 1: 1, 7: 1},
            "blocks_per_cu_min": 1,
            "blocks_per_cu_max": 2,
            "simds_per_cu_min": 1,  # the lone block on xcc 1
            "bad_cus": [
                {
                    "xcc": 7,
                    "se": 3,
                    "sh": 1,
                    "cu": 15,
                    "blocks": 1,
                    "lds_mismatches": 2,
                    "mfma_mismatches": 4,
                }
            ],
        }
        # the two blocks of one CU OR their masks: 0b0011 | 0b0100
        assert C.aggregate(raw[: 3 * C.RECORD_BYTES])["simds_per_cu_min"] == 3

    def test_aggregate_sums_a_cu_and_sorts_the_bad_ones(self):
        raw = b"".join(
            [
                C.pack_record(C.make_hw_id(2, 0, 1), 3, 0, 1, mfma=4),
                C.pack_record(C.make_hw_id(0, 0, 9), 1, 1, 2, lds=1),
                C.pack_record(C.make_hw_id(2, 0, 1), 3, 2, 4, lds=5),
            ]
        )
        bad = C.aggregate(raw)["bad_cus"]
        assert [(c["xcc"], c["se"], c["sh"], c["cu"]) for c in bad] == [
            (1, 0, 0, 9),
            (3, 2, 0, 1),
        ]
        assert (bad[1]["blocks"], bad[1]["lds_mismatches"], bad[1]["mfma_mismatches"]) == (
            2,
            5,
            4,
        )

    def test_a_record_without_its_block_index_raises(self):
        raw = C.pack_record(0, 0, 0, 1) + C.pack_record(0, 0, 5, 1)
        with pytest.raises(ValueError, match="block 1"):
            C.aggregate(raw)
        canary = bytes([0xA5]) * C.RECORD_BYTES
        with pytest.raises(ValueError, match="block 0"):
            C.aggregate(canary)


# ---------------------------------------------------------------------------
# selftest.run on a stub child
# ---------------------------------------------------------------------------
BAD_CU = {
    "xcc": 5,
    "se": 2,
    "sh": 1,
    "cu": 9,
    "blocks": 8,
    "lds_mismatches": 2,
    "mfma_mismatches": 4,
}


def cu_part(bad_cus=(), lds_records=(), mfma_records=()):
    """The ``cu`` part of a child's report."""
    return {
        "ok": not bad_cus,
        "device": 0,
        "seed": 1,
        "blocks": 2048,
        "lds_bytes": 163840,
        "multi_processor_count": 256,
        "covered": 256,
        "per_xcc": {str(x): 32 for x in range(8)},
        "blocks_per_cu_min": 8,
        "blocks_per_cu_max": 8,
        "simds_per_cu_min": 4,
        "lds": {
            "checked_words": 2048 * 4 * 20480,
            "mismatches": sum(c["lds_mismatches"] for c in bad_cus),
            "records": [list(r) for r in lds_records],
        },
        "mfma": {
            "checked": 2048 * 4 * 16 * 64 * 4,
            "mismatches": sum(c["mfma_mismatches"] for c in bad_cus),
            "records": [list(r) for r in mfma_records],
        },
        "bad_cus": [dict(c) for c in bad_cus],
        "kernel_ms": 0.4,
    }


def bad_cu_part():
    return cu_part(
        [BAD_CU],
        lds_records=[(77, "hash", 300, 0xFF, 0xFE), (12, "addr", 5, 7, 6)],
        mfma_records=[(12, w, 3, 37, 2, 0x42280000, 0x42290000) for w in (3, 0, 1, 2)],
    )


def with_cu(cu, **kw):
    rep = report(**kw)
    rep["cu"] = cu
    rep["ok"] = bool(rep["ok"] and isinstance(cu, dict) and cu.get("ok"))
    return rep


class TestRun:
    def test_the_argument_is_present_only_when_asked(self):
        spawn = spawn_returning(0, json.dumps(with_cu(cu_part())))
        res = selftest.run(Gpu(0), mib=64, spawn=spawn, per_cu=True)
        assert res.outcome == "pass"
        assert res.findings() == []
        assert res.report["cu"]["covered"] == 256
        spawn2 = spawn_returning(0, json.dumps(report()))
        assert selftest.run(Gpu(0), mib=64, spawn=spawn2).outcome == "pass"
        spawn3 = spawn_returning(0, json.dumps(report()))
        assert selftest.run(Gpu(0), mib=64, spawn=spawn3, per_cu=False).outcome == "pass"
        (argv, _), = spawn.calls
        assert argv[-2:] == ["--json", "--per-cu"]
        for s in (spawn2, spawn3):
            (argv, _), = s.calls
            assert "--per-cu" not in argv and argv[-1] == "--json"

    def test_a_bad_cu_is_a_compute_mismatch_that_names_it(self):
        spawn = spawn_returning(1, json.dumps(with_cu(bad_cu_part())))
        res = selftest.run(Gpu(0), spawn=spawn, per_cu=True)
        assert res.outcome == "compute", res.error
        (f,) = res.findings()
        assert (f.reason, f.severity) == ("SelftestComputeMismatch", "fatal")
        assert "1 of 256 covered CU(s) bad" in f.detail
        assert "xcc 5 se 2 sh 1 cu 9 (lds 2, mfma 4)" in f.detail
        # the lowest record of each kind
        assert "block 12 pattern addr word 5" in f.detail
        assert "0x0000000000000007" in f.detail and "0x0000000000000006" in f.detail
        assert "block 12 wave 0 vector 3 lane 37 slot 2" in f.detail
        assert "0x42280000" in f.detail and "0x42290000" in f.detail

    def test_only_the_first_few_bad_cus_are_spelt_out(self):
        bad = [dict(BAD_CU, cu=c, lds_mismatches=1, mfma_mismatches=0) for c in range(7)]
        spawn = spawn_returning(1, json.dumps(with_cu(cu_part(bad))))
        (f,) = selftest.run(Gpu(0), spawn=spawn, per_cu=True).findings()
        assert "7 of 256 covered CU(s) bad" in f.detail
        assert "cu 3 (lds 1, mfma 0)" in f.detail and "cu 4 (" not in f.detail
        assert "and 3 more" in f.detail

    def test_memory_outranks_and_every_part_has_its_finding(self):
        rep = with_cu(
            bad_cu_part(),
            memory_bad=("addr", 1, [(0, 1, 0)]),
            mfma_records=[(0, 0, 0, 1, 2)],
        )
        res = selftest.run(Gpu(0), spawn=spawn_returning(1, json.dumps(rep)), per_cu=True)
        assert res.outcome == "memory"
        assert [f.reason for f in res.findings()] == [
            "SelftestMemoryMismatch",
            "SelftestComputeMismatch",
            "SelftestComputeMismatch",
        ]
        assert "per-CU test" in res.findings()[2].detail

    @pytest.mark.parametrize(
        "cu",
        [
            None,
            [],
            "fine",
            {"ok": True},
            {k: v for k, v in cu_part().items() if k != "bad_cus"},
            {k: v for k, v in cu_part().items() if k != "covered"},
            dict(cu_part(), lds={"mismatches": 0}),
            dict(cu_part(), mfma={"mismatches": "many", "records": []}),
            dict(cu_part(), ok=False),  # not ok but lists no mismatch
            dict(bad_cu_part(), bad_cus=[]),  # mismatches on no CU
            dict(bad_cu_part(), bad_cus=[{"xcc": 1}]),
            dict(bad_cu_part(), ok=True),
            dict(cu_part(), lds={"mismatches": 0, "records": [[1, 2, 3]]}),
        ],
    )
    def test_a_malformed_cu_part_is_an_error(self, cu):
        rep = with_cu(cu)
        for rc in (0, 1):
            res = selftest.run(
                Gpu(0), spawn=spawn_returning(rc, json.dumps(rep)), per_cu=True
            )
            assert res.outcome == "error", (rc, cu)
            (f,) = res.findings()
            assert (f.reason, f.severity) == ("SelftestError", "soft")

    def test_asked_for_but_missing_is_an_error(self):
        spawn = spawn_returning(0, json.dumps(report()))
        res = selftest.run(Gpu(0), spawn=spawn, per_cu=True)
        assert res.outcome == "error" and "cu" in res.error

    def test_a_report_without_cu_behaves_as_before(self):
        rec = (19, 5, 2, 0x42280000, 0x42290000)
        cases = [
            (0, report(), "pass", []),
            (1, report(("hash", 1, [(12, 5, 4)])), "memory", ["SelftestMemoryMismatch"]),
            (1, report(mfma_records=[rec]), "compute", ["SelftestComputeMismatch"]),
        ]
        for rc, rep, outcome, reasons in cases:
            res = selftest.run(Gpu(0), spawn=spawn_returning(rc, json.dumps(rep)))
            assert res.outcome == outcome
            assert [f.reason for f in res.findings()] == reasons
            assert "cu" not in res.report
        (f,) = res.findings()
        assert "wave 19 lane 5 slot 2" in f.detail and "per-CU" not in f.detail

    def test_child_flag_parses(self, monkeypatch, capsys):
        seen = []

        def child(bdf, mib, per_cu=False):
            seen.append((bdf, mib, per_cu))
            return 2, {"ok": False, "error": "stub"}

        monkeypatch.setattr(selftest, "_child", child)
        assert selftest.main(["--bdf", "0000:c1:00.0", "--mib", "8", "--per-cu"]) == 2
        assert selftest.main(["--bdf", "0000:c1:00.0", "--mib", "8"]) == 2
        assert seen == [("0000:c1:00.0", 8, True), ("0000:c1:00.0", 8, False)]


# ---------------------------------------------------------------------------
# driver
# ---------------------------------------------------------------------------
def per_cu_runner(outcomes):
    """runner(gpu, mib=, timeout_s=, per_cu=) with a ``cu`` part."""
    calls = []

    def runner(gpu, *, mib, timeout_s, per_cu=False):
        calls.append((gpu.index, per_cu))
        outcome = outcomes.get(gpu.index, "pass")
        cu = bad_cu_part() if outcome == "compute" else cu_part()
        selftest._classify_cu(cu)  # as run() leaves it
        rep = with_cu(cu) if per_cu else report()
        return selftest.SelftestResult(
            gpu.index, gpu.pcie_bdf, outcome, rep, "", seconds=0.25
        )

    runner.calls = calls
    return runner


class TestDriver:
    def test_old_signature_runner_still_works_with_per_cu_off(self, tmp_path):
        d, _, _ = make_driver(tmp_path, gpu_indices=[0, 1])
        try:
            runner = stub_runner({})  # accepts mib and timeout_s only
            assert d.run_startup_selftest(runner, mib=64) == {0: "pass", 1: "pass"}
            assert d.run_startup_selftest(runner, mib=64, per_cu=False) == {
                0: "pass",
                1: "pass",
            }
            assert len(runner.calls) == 4
            for name in ("dra_gpu_selftest_cus_covered", "dra_gpu_selftest_cus_bad"):
                assert sample(d.metrics, name, gpu="0") is None
        finally:
            d.shutdown(unpublish=False)

    def test_per_cu_reaches_the_runner_and_sets_the_gauges(self, tmp_path, caplog):
        d, kube, _ = make_driver(tmp_path, gpu_indices=[0, 1])
        try:
            runner = per_cu_runner({1: "compute"})
            with caplog.at_level("INFO", logger="k8s_dra_driver_amd.plugin.driver"):
                results = d.run_startup_selftest(runner, mib=64, per_cu=True)
            assert results == {0: "pass", 1: "compute"}
            assert runner.calls == [(0, True), (1, True)]
            m = d.metrics
            assert sample(m, "dra_gpu_selftest_cus_covered", gpu="0") == 256
            assert sample(m, "dra_gpu_selftest_cus_bad", gpu="0") == 0
            assert sample(m, "dra_gpu_selftest_cus_covered", gpu="1") == 256
            assert sample(m, "dra_gpu_selftest_cus_bad", gpu="1") == 1
            assert d.health.findings(0) == []
            (f,) = d.health.findings(1)
            assert f.reason == "SelftestComputeMismatch"
            assert "xcc 5 se 2 sh 1 cu 9" in f.detail
            assert any(
                "gpu-0" in r.getMessage() and "256 of 256 CUs covered" in r.getMessage()
                for r in caplog.records
            )
        finally:
            d.shutdown(unpublish=False)


# ---------------------------------------------------------------------------
# CLIs
# ---------------------------------------------------------------------------
class TestPluginFlags:
    class FakeDriver:
        def __init__(self):
            self.calls = []

        def run_startup_selftest(self, **kw):
            self.calls.append(kw)

    def test_default_is_off(self, monkeypatch):
        monkeypatch.delenv("SELFTEST_PER_CU", raising=False)
        args = plugin_main.build_parser().parse_args(["--startup-selftest", "on"])
        assert args.selftest_per_cu == "off"
        drv = self.FakeDriver()
        assert plugin_main.startup_selftest(args, drv) is True
        assert drv.calls == [{"mib": 1024, "timeout_s": 120.0}]

    def test_on_is_passed_through(self, monkeypatch):
        monkeypatch.setenv("SELFTEST_PER_CU", "on")
        args = plugin_main.build_parser().parse_args(
            ["--startup-selftest", "on", "--selftest-mib", "64"]
        )
        assert args.selftest_per_cu == "on"
        drv = self.FakeDriver()
        assert plugin_main.startup_selftest(args, drv) is True
        assert drv.calls == [{"mib": 64, "timeout_s": 120.0, "per_cu": True}]
        args = plugin_main.build_parser().parse_args(
            ["--startup-selftest", "on", "--selftest-per-cu", "off"]
        )
        assert args.selftest_per_cu == "off"

    def test_it_means_nothing_without_the_selftest(self, monkeypatch):
        monkeypatch.delenv("STARTUP_SELFTEST", raising=False)
        args = plugin_main.build_parser().parse_args(["--selftest-per-cu", "on"])
        drv = self.FakeDriver()
        assert plugin_main.startup_selftest(args, drv) is False
        assert drv.calls == []

    def test_bad_value_is_rejected(self):
        with pytest.raises(SystemExit):
            plugin_main.build_parser().parse_args(["--selftest-per-cu", "maybe"])


class TestCtl:
    def test_per_cu_json_lists_coverage_and_bad_cus(self, monkeypatch, capsys):
        runner = per_cu_runner({4: "compute"})
        monkeypatch.setattr(
            selftest, "run", lambda gpu, **kw: runner(gpu, timeout_s=0, **kw)
        )
        rc = ctl.main(["--hal", "fake", "health", "--selftest", "--per-cu", "--json"])
        assert rc == 1
        assert runner.calls == [(i, True) for i in range(8)]
        records = json.loads(capsys.readouterr().out)
        assert records[0]["selftest"]["cu"] == {
            "covered": 256,
            "expected": 256,
            "bad_cus": [],
        }
        assert records[4]["selftest"]["result"] == "compute"
        assert records[4]["selftest"]["cu"]["bad_cus"] == [BAD_CU]
        (f,) = records[4]["findings"]
        assert f["reason"] == "SelftestComputeMismatch" and "cu 9" in f["detail"]

    def test_per_cu_text_names_the_bad_cu(self, monkeypatch, capsys):
        runner = per_cu_runner({4: "compute"})
        monkeypatch.setattr(
            selftest, "run", lambda gpu, **kw: runner(gpu, timeout_s=0, **kw)
        )
        assert ctl.main(["--hal", "fake", "health", "--selftest", "--per-cu"]) == 1
        out = capsys.readouterr().out
        assert "per CU: 256 of 256 CUs covered, 0 bad" in out
        assert "per CU: 256 of 256 CUs covered, 1 bad" in out
        assert "xcc 5 se 2 sh 1 cu 9: lds 2, mfma 4" in out

    def test_without_the_flag_the_runner_sees_the_old_call(self, monkeypatch, capsys):
        runner = stub_runner({})  # would reject per_cu
        monkeypatch.setattr(
            selftest, "run", lambda gpu, **kw: runner(gpu, timeout_s=0, **kw)
        )
        assert ctl.main(["--hal", "fake", "health", "--selftest", "--json"]) == 0
        records = json.loads(capsys.readouterr().out)
        assert all("cu" not in r["selftest"] for r in records)
