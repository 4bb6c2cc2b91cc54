"""The startup self-test without a GPU: the numpy references, the parent
half of ``k8s_dra_driver_amd.selftest`` on a stub child, the monitor's
sticky findings, the driver's startup pass, and the CLIs."""

import json
import subprocess
import threading
import time

import numpy as np
import pytest

import selftest_reference as S
from k8s_dra_driver_amd import DRIVER_NAME, ctl, selftest
from k8s_dra_driver_amd.hal import FakeDeviceLib
from k8s_dra_driver_amd.kube.client import InMemoryKube
from k8s_dra_driver_amd.plugin import main as plugin_main
from k8s_dra_driver_amd.plugin.driver import ClaimRef, Driver
from k8s_dra_driver_amd.plugin.health import (
    REASONS,
    HealthFinding,
    HealthMonitor,
)


# ---------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------
class TestReference:
    def test_mix_known_answers(self):
        assert S.mix_int(0) == 0xE220A8397B1DCDAF
        assert S.mix_int(1) == 0x910A2DEC89025CC1
        got = S.mix(np.array([0, 1], dtype=np.uint64))
        assert got.tolist() == [0xE220A8397B1DCDAF, 0x910A2DEC89025CC1]

    def test_mix_wraps_like_the_integer_form(self):
        xs = [0, 1, 2**63, 2**64 - 1, 0x0123456789ABCDEF]
        got = S.mix(np.array(xs, dtype=np.uint64)).tolist()
        assert got == [S.mix_int(x) for x in xs]

    @pytest.mark.parametrize("base", ["addr", "hash"])
    def test_inverse_is_the_complement(self, base):
        seed = 0xDEADBEEF12345678
        a = S.pattern_words(base, 1000, seed)
        b = S.pattern_words(base + "_inv", 1000, seed)
        assert np.array_equal(a ^ b, np.full(1000, 2**64 - 1, dtype=np.uint64))

    def test_addr_with_seed_zero_is_arange(self):
        assert np.array_equal(
            S.pattern_words("addr", 777, 0), np.arange(777, dtype=np.uint64)
        )

    def test_hash_adds_the_seed_mod_2_64(self):
        w = S.pattern_words("hash", 4, 2**64 - 2)
        assert w.tolist() == [S.mix_int((i + 2**64 - 2) % 2**64) for i in range(4)]

    def test_bytes_are_little_endian_words(self):
        raw = S.pattern_bytes("addr", 32, 0x0102030405060708)
        assert raw[:8] == bytes([8, 7, 6, 5, 4, 3, 2, 1])
        assert len(raw) == 32

    def test_expected_records_are_exactly_the_injected_set(self):
        seed = 99
        flips = [(0, 1), (41, 1 << 63), (7, 0b1010)]
        recs = S.expected_records("hash_inv", seed, flips, 42)
        words = S.pattern_words("hash_inv", 42, seed)
        assert recs == {
            (0, int(words[0]) ^ 1, int(words[0])),
            (41, int(words[41]) ^ (1 << 63), int(words[41])),
            (7, int(words[7]) ^ 0b1010, int(words[7])),
        }
        assert all(got ^ want in (1, 1 << 63, 0b1010) for _, got, want in recs)
        # masks on one word combine, and cancel
        assert S.expected_records("addr", 0, [(3, 1), (3, 2)], 8) == {(3, 0, 3)}
        assert S.expected_records("addr", 0, [(3, 1), (3, 1)], 8) == set()

    def test_apply_flips_changes_only_those_words(self):
        clean = S.pattern_bytes("addr", 64, 5)
        dirty = S.apply_flips(clean, [(2, 0xFF)])
        assert dirty[:16] == clean[:16] and dirty[24:] == clean[24:]
        assert dirty[16] == clean[16] ^ 0xFF

    def test_kat_tables_hold_what_the_emulated_instruction_gives(self):
        import hip_reference as R

        a, b, c, want = S.kat_tables()
        assert a.shape == (16, 64, 8) and want.shape == (16, 64, 4)
        for v in (0, 15):
            acc = c[v].astype(np.float64)
            for _ in range(S.KAT_CHAIN):
                acc = R.emulate_mfma(a[v], b[v], acc)
            assert np.array_equal(acc, want[v].astype(np.float64))
        assert not np.array_equal(want[0], want[1])


# ---------------------------------------------------------------------------
# selftest.run on a stub child
# ---------------------------------------------------------------------------
class Gpu:
    def __init__(self, index, bdf="0000:c1:00.0"):
        self.index = index
        self.pcie_bdf = bdf


def report(memory_bad=None, mfma_records=()):
    """A child's report; ``memory_bad`` = (pattern, count, records)."""
    passes = []
    for p in S.PATTERNS:
        count, records = 0, []
        if memory_bad and memory_bad[0] == p:
            count, records = memory_bad[1], memory_bad[2]
        passes.append(
            {
                "pattern": p,
                "mismatches": count,
                "records": [list(r) for r in records],
                "fill_gbs": 3000.0,
                "verify_gbs": 4000.0,
            }
        )
    return {
        "ok": not memory_bad and not mfma_records,
        "device": 0,
        "seed": 1,
        "bytes": 64 << 20,
        "memory": passes,
        "mfma": {
            "blocks": 1024,
            "checked": 1024 * 1024,
            "mismatches": len(mfma_records),
            "records": [list(r) for r in mfma_records],
        },
    }


def spawn_returning(rc, out, err=""):
    calls = []

    def spawn(argv, timeout_s):
        calls.append((argv, timeout_s))
        return rc, out, err

    spawn.calls = calls
    return spawn


class TestRun:
    def test_pass_gives_no_findings(self):
        spawn = spawn_returning(0, json.dumps(report()) + "\n")
        res = selftest.run(Gpu(3, "0000:C1:00.0"), mib=64, timeout_s=7, spawn=spawn)
        assert res.outcome == "pass" and res.gpu_index == 3
        assert res.findings() == []
        (argv, timeout_s), = spawn.calls
        assert argv[1:] == [
            "-m",
            "k8s_dra_driver_amd.selftest",
            "--bdf",
            "0000:C1:00.0",
            "--mib",
            "64",
            "--json",
        ]
        assert timeout_s == 7

    def test_memory_mismatch_is_fatal_with_word_and_hex(self):
        recs = [(77, 0xDEADBEEF00000001, 0xDEADBEEF00000000), (12, 5, 4)]
        spawn = spawn_returning(1, json.dumps(report(("hash", 2, recs))))
        res = selftest.run(Gpu(0), spawn=spawn)
        assert res.outcome == "memory"
        (f,) = res.findings()
        assert (f.reason, f.severity) == ("SelftestMemoryMismatch", "fatal")
        assert "pattern hash" in f.detail and "2 mismatching" in f.detail
        # the lowest recorded word, got and want in hex
        assert "word 12" in f.detail
        assert "0x0000000000000005" in f.detail
        assert "0x0000000000000004" in f.detail

    def test_compute_mismatch_is_fatal(self):
        rec = (19, 5, 2, 0x42280000, 0x42290000)
        spawn = spawn_returning(1, json.dumps(report(mfma_records=[rec])))
        res = selftest.run(Gpu(0), spawn=spawn)
        assert res.outcome == "compute"
        (f,) = res.findings()
        assert (f.reason, f.severity) == ("SelftestComputeMismatch", "fatal")
        assert "wave 19 lane 5 slot 2" in f.detail
        assert "0x42280000" in f.detail and "0x42290000" in f.detail

    def test_both_mismatches_give_both_findings(self):
        rep = report(("addr", 1, [(0, 1, 0)]), [(0, 0, 0, 1, 2)])
        res = selftest.run(Gpu(0), spawn=spawn_returning(1, json.dumps(rep)))
        assert res.outcome == "memory"
        assert [f.reason for f in res.findings()] == [
            "SelftestMemoryMismatch",
            "SelftestComputeMismatch",
        ]

    def _assert_error(self, res, *needles):
        assert res.outcome == "error"
        (f,) = res.findings()
        assert (f.reason, f.severity) == ("SelftestError", "soft")
        for n in needles:
            assert n in f.detail, f.detail

    def test_exit_2_is_an_error(self):
        out = json.dumps({"ok": False, "error": "no HIP device at ffff:ff:1f.7"})
        res = selftest.run(Gpu(0), spawn=spawn_returning(2, out))
        self._assert_error(res, "exit 2", "no HIP device")

    def test_timeout_is_an_error_and_is_not_retried(self):
        calls = []

        def spawn(argv, timeout_s):
            calls.append(argv)
            raise subprocess.TimeoutExpired(argv, timeout_s)

        res = selftest.run(Gpu(0), timeout_s=3, spawn=spawn)
        self._assert_error(res, "timed out after 3s")
        assert len(calls) == 1

    @pytest.mark.parametrize(
        "rc,out",
        [
            (0, "Segmentation fault"),
            (0, ""),
            (0, "[1, 2]"),
            (0, json.dumps({"ok": True})),
            (-11, ""),
            (1, json.dumps(report())),  # exit code contradicts the report
            (0, json.dumps(report(("addr", 1, [(0, 1, 0)])))),
        ],
    )
    def test_garbage_is_an_error(self, rc, out):
        res = selftest.run(Gpu(0), spawn=spawn_returning(rc, out, "boom"))
        self._assert_error(res)

    def test_a_spawn_that_cannot_start_is_an_error(self):
        def spawn(argv, timeout_s):
            raise OSError("no such interpreter")

        self._assert_error(selftest.run(Gpu(0), spawn=spawn), "no such interpreter")

    def test_one_child_at_a_time(self):
        alive, overlaps = [], []
        guard = threading.Lock()
        entered = threading.Barrier(2, timeout=5)

        def spawn(argv, timeout_s):
            with guard:
                alive.append(argv)
                if len(alive) > 1:
                    overlaps.append(list(alive))
            # give a second child every chance to start beside this one
            for _ in range(50):
                time.sleep(0)
            with guard:
                alive.remove(argv)
            return 0, json.dumps(report()), ""

        def one(i):
            entered.wait()
            results.append(selftest.run(Gpu(i), spawn=spawn))

        results = []
        threads = [threading.Thread(target=one, args=(i,)) for i in range(2)]
        for t in threads:
            t.start()
        for t in threads:
            t.join(10)
        assert [r.outcome for r in results] == ["pass", "pass"]
        assert overlaps == []

    def test_real_child_for_an_address_nobody_has(self):
        # A real child process (this process must not load HIP): with or
        # without a GPU there is no device at this address, so it exits 2
        # with one JSON object and the parent maps that to SelftestError.
        res = selftest.run(Gpu(0, "ffff:ff:1f.7"), mib=1, timeout_s=120)
        self._assert_error(res, "exit 2", "ffff:ff:1f.7")
        assert res.report["ok"] is False


def test_new_reasons_sit_at_the_end_of_their_severity_group():
    names = [r for r, _ in REASONS]
    sev = dict(REASONS)
    assert sev["SelftestMemoryMismatch"] == sev["SelftestComputeMismatch"] == "fatal"
    assert sev["SelftestError"] == "soft"
    fatal = [r for r in names if sev[r] == "fatal"]
    soft = [r for r in names if sev[r] == "soft"]
    assert fatal[-2:] == ["SelftestMemoryMismatch", "SelftestComputeMismatch"]
    assert soft[-1] == "SelftestError"
    # the reasons that were there before keep their relative order
    assert [r for r in names if not r.startswith("Selftest")] == [
        "UncorrectableEcc",
        "BadPagesPending",
        "BadPageUnreservable",
        "BadPageThreshold",
        "ThermalCritical",
        "HealthCheckFailed",
        "HealthSignalsError",
        "UncorrectableEccHistoric",
        "CorrectableEccGrowth",
        "DeferredEcc",
        "RetiredPages",
        "Throttled",
    ]


# ---------------------------------------------------------------------------
# monitor
# ---------------------------------------------------------------------------
MEM = HealthFinding("SelftestMemoryMismatch", "fatal", "pattern addr: 1 word")
ERR = HealthFinding("SelftestError", "soft", "timed out")


class TestMonitor:
    def test_sticky_fatal_finding_taints_on_the_next_poll(self, fake_lib):
        mon = HealthMonitor(fake_lib)
        mon.set_selftest_findings(2, [MEM])
        assert mon.unhealthy_gpus == set()  # nothing before a poll
        assert mon.check_once() == {2}
        assert mon.primary_reason(2) == "SelftestMemoryMismatch"
        for _ in range(3):  # the signals are clean: it stays
            assert mon.check_once() == {2}
            assert mon.findings(2) == [MEM]
        mon.set_selftest_findings(2, [])
        assert mon.check_once() == set()
        assert mon.findings(2) == []

    def test_selftest_error_needs_two_polls(self, fake_lib):
        mon = HealthMonitor(fake_lib, failures_to_unhealthy=2)
        mon.set_selftest_findings(5, [ERR])
        assert mon.check_once() == set()
        assert mon.findings(5) == [ERR]
        assert mon.check_once() == {5}
        assert mon.primary_reason(5) == "SelftestError"

    def test_a_fatal_signal_outranks_nothing_it_should_not(self, fake_lib):
        mon = HealthMonitor(fake_lib)
        mon.set_selftest_findings(1, [MEM])
        fake_lib.set_health_signals(1, bad_pages_pending=1)
        assert mon.check_once() == {1}
        assert mon.primary_reason(1) == "BadPagesPending"  # table order
        assert [f.reason for f in mon.findings(1)] == [
            "BadPagesPending",
            "SelftestMemoryMismatch",
        ]

    def test_nothing_set_reports_as_before(self):
        def scripted(mon, lib):
            reports = []
            mon.on_poll = lambda r: reports.append(
                (r.gpu_index, [f.reason for f in r.findings], r.unhealthy, r.primary_reason)
            )
            mon.check_once()
            lib.set_health_signals(3, ecc_uncorrectable=1)
            mon.check_once()
            lib.set_health_signals(5, temp_hotspot_c=111.0)
            mon.check_once()
            mon.check_once()
            lib.set_health_signals(3, ecc_uncorrectable=0)
            mon.check_once()
            return reports

        runs = []
        for touch in (False, True):
            lib = FakeDeviceLib()
            lib.open()
            mon = HealthMonitor(lib)
            if touch:  # set and cleared again = nothing set
                mon.set_selftest_findings(3, [MEM])
                mon.set_selftest_findings(3, [])
            runs.append(scripted(mon, lib))
        assert runs[0] == runs[1]
        flat = [reason for _, reasons, _, _ in runs[0] for reason in reasons]
        assert "UncorrectableEcc" in flat and "ThermalCritical" in flat
        assert not any(r.startswith("Selftest") for r in flat)


# ---------------------------------------------------------------------------
# driver
# ---------------------------------------------------------------------------
def make_driver(tmp_path, lib=None, **kw):
    if lib is None:
        lib = FakeDeviceLib()
        lib.open()
    kube = InMemoryKube()
    kube.api_versions = ["v1beta2", "v1beta1"]
    d = Driver(
        lib,
        kube,
        node_name="n",
        cdi_root=str(tmp_path / "cdi"),
        checkpoint_root=str(tmp_path / "state"),
        use_tmpfs=False,
        **kw,
    )
    return d, kube, lib


def published(kube):
    return {
        dev["name"]: dev
        for s in kube.list_resource_slices(DRIVER_NAME)
        for dev in s["spec"]["devices"]
    }


def sample(metrics, name, **labels):
    return metrics.registry.get_sample_value(name, labels)


def stub_runner(outcomes):
    """runner(gpu, mib=, timeout_s=) with a scripted outcome per index."""
    calls = []

    def runner(gpu, *, mib, timeout_s):
        calls.append((gpu.index, mib, timeout_s))
        outcome = outcomes.get(gpu.index, "pass")
        rep, error = None, ""
        if outcome == "memory":
            rep = report(("addr_inv", 3, [(9, 0xFE, 0xFF)]))
        elif outcome == "compute":
            rep = report(mfma_records=[(1, 2, 3, 4, 5)])
        elif outcome == "error":
            error = "timed out after 120s; child killed"
        return selftest.SelftestResult(
            gpu.index, gpu.pcie_bdf, outcome, rep, error, seconds=0.25
        )

    runner.calls = calls
    return runner


class TestDriver:
    def test_failing_gpu_is_tainted_in_the_first_published_slice(self, tmp_path):
        d, kube, lib = make_driver(tmp_path)
        try:
            runner = stub_runner({2: "memory", 6: "error"})
            assert kube.list_resource_slices(DRIVER_NAME) == []
            results = d.run_startup_selftest(runner, mib=64, timeout_s=9)
            d.startup()
            assert results == {
                i: {2: "memory", 6: "error"}.get(i, "pass") for i in range(8)
            }
            assert [c[0] for c in runner.calls] == list(range(8))  # in order
            assert {c[1:] for c in runner.calls} == {(64, 9)}
            devs = published(kube)
            assert len(devs) == 8
            assert devs["gpu-2"]["taints"] == [
                {
                    "key": "gpu.amd.com/unhealthy",
                    "effect": "NoSchedule",
                    "value": "SelftestMemoryMismatch",
                }
            ]
            assert [n for n, dev in devs.items() if "taints" in dev] == ["gpu-2"]
            # the soft error needs a second poll
            d.health.check_once()
            assert published(kube)["gpu-6"]["taints"][0]["value"] == "SelftestError"

            m = d.metrics
            runs = "dra_gpu_selftest_runs_total"
            assert sample(m, runs, gpu="2", result="memory") == 1
            assert sample(m, runs, gpu="6", result="error") == 1
            assert sample(m, runs, gpu="0", result="pass") == 1
            assert sample(m, runs, gpu="2", result="pass") is None
            assert sample(m, "dra_gpu_selftest_seconds", gpu="2") >= 0
            assert (
                sample(m, "dra_gpu_unhealthy", gpu="2", reason="SelftestMemoryMismatch")
                == 1
            )
        finally:
            d.shutdown(unpublish=False)

    def test_compute_mismatch_taints_too(self, tmp_path):
        d, kube, _ = make_driver(tmp_path)
        try:
            d.run_startup_selftest(stub_runner({0: "compute"}))
            d.startup()
            assert (
                published(kube)["gpu-0"]["taints"][0]["value"]
                == "SelftestComputeMismatch"
            )
            assert (
                sample(
                    d.metrics, "dra_gpu_selftest_runs_total", gpu="0", result="compute"
                )
                == 1
            )
        finally:
            d.shutdown(unpublish=False)

    def test_held_and_partitioned_gpus_are_skipped(self, tmp_path, caplog):
        # first life: a claim is prepared on gpu-3
        d, kube, lib = make_driver(tmp_path)
        d.startup()
        kube.put_resource_claim(
            {
                "metadata": {"namespace": "team-a", "name": "c", "uid": "uid-1"},
                "status": {
                    "allocation": {
                        "devices": {
                            "results": [
                                {
                                    "request": "gpu",
                                    "driver": DRIVER_NAME,
                                    "pool": "n",
                                    "device": "gpu-3",
                                }
                            ]
                        }
                    }
                },
            }
        )
        res = d.node_prepare_resources([ClaimRef("team-a", "c", "uid-1")])["uid-1"]
        assert not res.error, res.error
        d.shutdown(unpublish=False)
        # the node is repartitioned while the plugin is down
        lib.set_compute_partition(5, "CPX")

        # second life: the checkpoint gives gpu-3 its holder back
        d2, kube2, _ = make_driver(tmp_path, lib=lib)
        try:
            assert d2.state.ledger.holders(3) == ["uid-1"]
            runner = stub_runner({3: "memory", 5: "memory"})
            with caplog.at_level("INFO", logger="k8s_dra_driver_amd.plugin.driver"):
                results = d2.run_startup_selftest(runner)
            assert results[3] == results[5] == "skipped"
            assert sorted(c[0] for c in runner.calls) == [0, 1, 2, 4, 6, 7]
            skipped = [
                r.getMessage() for r in caplog.records if "skipped" in r.getMessage()
            ]
            assert any("gpu-3" in s and "recovered claim" in s for s in skipped)
            assert any("gpu-5" in s and "partitioned" in s for s in skipped)
            d2.startup()
            assert d2.health.unhealthy_gpus == set()
            assert d2.health.findings(3) == [] and d2.health.findings(5) == []
            assert not any("taints" in dev for dev in published(kube2).values())
            runs = "dra_gpu_selftest_runs_total"
            assert sample(d2.metrics, runs, gpu="3", result="skipped") == 1
            assert sample(d2.metrics, runs, gpu="5", result="skipped") == 1
            assert sample(d2.metrics, "dra_gpu_selftest_seconds", gpu="3") is None
        finally:
            d2.shutdown(unpublish=False)

    def test_gpus_out_of_scope_are_not_tested(self, tmp_path):
        d, _, _ = make_driver(tmp_path, gpu_indices=[1, 4])
        try:
            runner = stub_runner({})
            assert d.run_startup_selftest(runner) == {1: "pass", 4: "pass"}
            assert [c[0] for c in runner.calls] == [1, 4]
        finally:
            d.shutdown(unpublish=False)

    def test_a_runner_that_raises_is_a_selftest_error(self, tmp_path):
        d, _, _ = make_driver(tmp_path, gpu_indices=[0])
        try:

            def runner(gpu, *, mib, timeout_s):
                raise RuntimeError("fork failed")

            assert d.run_startup_selftest(runner) == {0: "error"}
            assert [f.reason for f in d.health.findings(0)] == ["SelftestError"]
        finally:
            d.shutdown(unpublish=False)


# ---------------------------------------------------------------------------
# CLIs
# ---------------------------------------------------------------------------
class TestCtl:
    def test_selftest_findings_land_in_the_record(self, monkeypatch, capsys):
        runner = stub_runner({4: "memory"})
        monkeypatch.setattr(
            selftest, "run", lambda gpu, **kw: runner(gpu, timeout_s=0, **kw)
        )
        rc = ctl.main(
            ["--hal", "fake", "health", "--selftest", "--selftest-mib", "32", "--json"]
        )
        assert rc == 1
        records = json.loads(capsys.readouterr().out)
        assert [c[:2] for c in runner.calls] == [(i, 32) for i in range(8)]
        assert [(f["reason"], f["severity"]) for f in records[4]["findings"]] == [
            ("SelftestMemoryMismatch", "fatal")
        ]
        assert "0x00000000000000fe" in records[4]["findings"][0]["detail"]
        assert records[4]["selftest"]["result"] == "memory"
        assert records[0]["findings"] == []
        assert records[0]["selftest"]["result"] == "pass"

    def test_text_output_names_the_finding(self, monkeypatch, capsys):
        runner = stub_runner({1: "error"})
        monkeypatch.setattr(
            selftest, "run", lambda gpu, **kw: runner(gpu, timeout_s=0, **kw)
        )
        assert ctl.main(["--hal", "fake", "health", "--selftest"]) == 1
        out = capsys.readouterr().out
        assert "selftest: pass" in out and "selftest: error" in out
        assert "finding [soft] SelftestError: timed out" in out

    def test_all_pass_exits_0(self, monkeypatch, capsys):
        runner = stub_runner({})
        monkeypatch.setattr(
            selftest, "run", lambda gpu, **kw: runner(gpu, timeout_s=0, **kw)
        )
        assert ctl.main(["--hal", "fake", "health", "--selftest", "--json"]) == 0

    def test_without_the_flag_no_child_is_started(self, monkeypatch, capsys):
        def boom(*a, **kw):
            raise AssertionError("self-test started without --selftest")

        monkeypatch.setattr(selftest, "run", boom)
        assert ctl.main(["--hal", "fake", "health", "--json"]) == 0
        records = json.loads(capsys.readouterr().out)
        assert all("selftest" not in r for r in records)


class TestPluginFlags:
    class FakeDriver:
        def __init__(self):
            self.calls = []

        def run_startup_selftest(self, **kw):
            self.calls.append(kw)

    def test_default_is_off_and_off_runs_nothing(self, monkeypatch):
        for name in ("STARTUP_SELFTEST", "SELFTEST_MIB", "SELFTEST_TIMEOUT_S"):
            monkeypatch.delenv(name, raising=False)
        args = plugin_main.build_parser().parse_args([])
        assert args.startup_selftest == "off"
        assert args.selftest_mib == 1024
        assert args.selftest_timeout_s == 120
        drv = self.FakeDriver()
        monkeypatch.setattr(selftest, "extension_path", lambda: "")
        plugin_main.require_selftest_extension(args)  # off: nothing to require
        assert plugin_main.startup_selftest(args, drv) is False
        assert drv.calls == []

    def test_on_passes_the_sizes_through(self, monkeypatch):
        monkeypatch.setenv("STARTUP_SELFTEST", "on")
        monkeypatch.setenv("SELFTEST_MIB", "512")
        args = plugin_main.build_parser().parse_args(["--selftest-timeout-s", "30"])
        assert args.startup_selftest == "on"
        drv = self.FakeDriver()
        assert plugin_main.startup_selftest(args, drv) is True
        assert drv.calls == [{"mib": 512, "timeout_s": 30.0}]

    def test_on_without_the_extension_refuses_to_start(self, monkeypatch):
        args = plugin_main.build_parser().parse_args(["--startup-selftest", "on"])
        monkeypatch.setattr(selftest, "extension_path", lambda: "")
        with pytest.raises(RuntimeError, match="_hiphealth extension is not built"):
            plugin_main.require_selftest_extension(args)
        monkeypatch.setattr(selftest, "extension_path", lambda: "/x/_hiphealth.so")
        plugin_main.require_selftest_extension(args)

    def test_bad_value_is_rejected(self):
        with pytest.raises(SystemExit):
            plugin_main.build_parser().parse_args(["--startup-selftest", "maybe"])
