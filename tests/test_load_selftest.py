"""The load self-test without a GPU: the numpy mirror's exactness argument,
the parent half of ``k8s_dra_driver_amd.selftest`` on a stub child with a
``"load"`` part, the driver, the command lines, and the stand-alone
sanitizer build of ``loadtest_core.hpp``.
"""

import json
import os
import subprocess
import types

import numpy as np
import pytest

import hip_reference as R
import loadtest_reference as L
import k8s_dra_driver_amd
from k8s_dra_driver_amd import build_native, ctl, selftest, workload
from k8s_dra_driver_amd.plugin import main as plugin_main
from k8s_dra_driver_amd.plugin.health import REASONS

from test_selftest import Gpu, make_driver, report, sample, spawn_returning, stub_runner

SEED = 0x0123456789ABCDEF


# ---------------------------------------------------------------------------
# the mirror and the exactness argument
# ---------------------------------------------------------------------------
class TestExactness:
    def test_generated_values_are_exact_in_bf16(self):
        for which in (0, 1):
            h = L.half_units(SEED, which, 256, 192)
            assert h.min() >= -32 and h.max() <= 32
            # every v * 2^e occurs
            want = {v * (1 << e) for v in range(-8, 9) for e in range(3)}
            assert set(np.unique(h).tolist()) == want
            bits = L.bits_of(h)  # raises if a value is not exact
            assert (R.bf16_value(bits).astype(np.float64) == L.values(h)).all()
            assert (L.units_of(bits) == h).all()
        a, b = L.half_units(SEED, 0, 8, 64), L.half_units(SEED, 1, 8, 64)
        assert (a != b).any()
        assert (L.half_units(SEED + 1, 0, 8, 64) != a).any()

    def test_one_value_by_hand(self):
        key = (1 << 56) | (5 << 28) | 7
        r = L.S.mix_int((SEED + key) & (2**64 - 1))
        want = (r % 17 - 8) * (1 << ((r >> 32) % 3))
        assert int(L.half_units(SEED, 1, 6, 8)[5, 7]) == want

    def test_the_adversarial_operands_stay_inside_24_bits_at_the_cap(self):
        k = L.MAX_K
        a = np.full((1, k), 32, dtype=np.int64)  # 16.0 in half units
        bt = np.full((2, k), 32, dtype=np.int64)
        a[0, 100] = 1  # 0.5
        bt[0, 100] = 1
        c = L.gemm_units(a, bt)
        assert c[0, 0] == 4 * 256 * (k - 1) + 1  # 256 * 8191 + 0.25
        assert np.abs(c).max() == 4 * 256 * (k - 1) + 32 < 1 << 24
        # the largest sum the generator's range allows at all
        assert 4 * 16 * 16 * k == 1 << 23
        f = L.to_f32(c)
        assert float(f[0, 0]) == 256.0 * (k - 1) + 0.25
        with pytest.raises(ValueError):
            L.to_f32(np.array([(1 << 24) + 1]))

    def test_float32_accumulation_in_any_order_equals_the_integers(self):
        k = L.MAX_K
        rng = np.random.default_rng(7)
        a = np.full(k, 32, dtype=np.int64)
        b = np.full(k, 32, dtype=np.int64)
        a[17] = b[17] = 1
        prod = (L.values(a) * L.values(b)).astype(np.float32)
        assert (prod.astype(np.float64) == L.values(a) * L.values(b)).all()
        want = L.to_f32(L.gemm_units(a[None, :], b[None, :]))[0, 0]
        for _ in range(3):
            acc = np.float32(0)
            for p in prod[rng.permutation(k)]:
                acc = np.float32(acc + p)  # one rounding per step, if any
            assert acc == want
        # grouped as the kernel groups: partial sums of 32, then their sum
        parts = prod[rng.permutation(k)].reshape(-1, 32)
        partial = np.zeros(parts.shape[0], dtype=np.float32)
        for j in range(32):
            partial = (partial + parts[:, j]).astype(np.float32)
        acc = np.float32(0)
        for p in partial:
            acc = np.float32(acc + p)
        assert acc == want

    def test_checksum_is_the_sum_of_the_product(self):
        a, bt = L.half_units(SEED, 0, 128, 192), L.half_units(SEED, 1, 256, 192)
        c = L.gemm_units(a, bt)
        rows, cols = L.checksum(a, bt)
        assert (rows == c.sum(axis=1)).all() and (cols == c.sum(axis=0)).all()

    def test_expected_mismatches_and_tiles(self):
        want = L.gemm_f32(L.half_units(1, 0, 256, 64), L.half_units(1, 1, 128, 64))
        got = want.copy()
        got[3, 5] += np.float32(0.25)
        got[200, 127] = -got[200, 127] - np.float32(1)
        mism = L.expected_mismatches(got, want)
        assert {(r, c) for r, c, _, _ in mism} == {(3, 5), (200, 127)}
        assert L.bad_tiles(mism, 128, iterations=3) == [(0, 0, 3), (1, 0, 3)]
        assert L.tile_of(200, 127, 128) == 1 and L.tile_of(130, 300, 384) == 5


# ---------------------------------------------------------------------------
# selftest.run on a stub child
# ---------------------------------------------------------------------------
BAD_CUS = [
    {"xcc": x, "se": 1, "sh": 0, "cu": 3, "mismatches": 2 + x} for x in range(6)
]


def load_part(bad=False, checksum_ok=True):
    part = {
        "ok": not bad and checksum_ok,
        "device": 0,
        "seed": 1,
        "m": 4096,
        "n": 4096,
        "k": 4096,
        "iterations": 8 if bad else 1200,
        "seconds": 1.0,
        "checksum_ok": checksum_ok,
        "checksum_first_bad": "" if checksum_ok else "row 12",
        "mismatches": 0,
        "records": [],
        "bad_tiles": [],
        "bad_cus": [],
        "cus_seen": 256,
        "tflops": 1.0,
    }
    if bad:
        part["mismatches"] = sum(c["mismatches"] for c in BAD_CUS)
        part["records"] = [[5, 130, 7, 0x40800000, 0x40000000], [2, 9, 300, 1, 2]]
        part["bad_tiles"] = [[0, 2, 20], [1, 0, 7]]
        part["bad_cus"] = [dict(c) for c in BAD_CUS]
    return part


def with_load(part):
    rep = report()
    rep["load"] = part
    rep["ok"] = rep["ok"] and part["ok"]
    return rep


class TestRun:
    def test_argv_carries_the_flag_only_when_asked_and_the_limit_grows(self):
        spawn = spawn_returning(0, json.dumps(with_load(load_part())))
        res = selftest.run(Gpu(0), mib=64, timeout_s=30, spawn=spawn, load_seconds=2.5)
        assert res.outcome == "pass", res.error
        assert res.findings() == []
        argv, limit = spawn.calls[0]
        assert argv[-3:] == ["--json", "--load-seconds", "2.5"]
        assert limit == 30 + 2.5 + selftest.LOAD_GOLDEN_ALLOWANCE_S
        for kw in ({}, {"load_seconds": 0}, {"load_seconds": 0.0}):
            spawn = spawn_returning(0, json.dumps(report()))
            assert selftest.run(Gpu(0), timeout_s=30, spawn=spawn, **kw).outcome == "pass"
            argv, limit = spawn.calls[0]
            assert "--load-seconds" not in argv and limit == 30

    def test_with_per_cu_both_flags_are_there(self):
        spawn = spawn_returning(2, json.dumps({"ok": False, "error": "x"}))
        selftest.run(Gpu(0), spawn=spawn, per_cu=True, load_seconds=1)
        argv, _ = spawn.calls[0]
        assert argv[-3:] == ["--per-cu", "--load-seconds", "1"]

    def test_a_bad_load_part_is_a_compute_failure(self):
        spawn = spawn_returning(1, json.dumps(with_load(load_part(bad=True))))
        res = selftest.run(Gpu(0), spawn=spawn, load_seconds=1)
        assert res.outcome == "compute", res.error
        (f,) = res.findings()
        assert f.reason == "SelftestComputeMismatch"
        assert dict(REASONS)[f.reason] == f.severity
        assert f.detail == (
            "load test: 27 mismatching value(s) in 8 iteration(s) of "
            "4096x4096x4096; 6 of 256 CU(s) seen bad: "
            "xcc 0 se 1 sh 0 cu 3 (2), xcc 1 se 1 sh 0 cu 3 (3), "
            "xcc 2 se 1 sh 0 cu 3 (4), xcc 3 se 1 sh 0 cu 3 (5), and 2 more; "
            "first recorded value: iteration 2 row 9 col 300: "
            "got 0x00000001, want 0x00000002"
        )

    def test_a_failed_checksum_is_a_compute_failure(self):
        part = load_part(checksum_ok=False)
        spawn = spawn_returning(1, json.dumps(with_load(part)))
        res = selftest.run(Gpu(0), spawn=spawn, load_seconds=1)
        assert res.outcome == "compute", res.error
        (f,) = res.findings()
        assert f.detail == (
            "load test: 0 mismatching value(s) in 1200 iteration(s) of "
            "4096x4096x4096; golden product failed its checksum at row 12"
        )

    def test_a_missing_load_part_is_an_error(self):
        spawn = spawn_returning(0, json.dumps(report()))
        res = selftest.run(Gpu(0), spawn=spawn, load_seconds=1)
        assert res.outcome == "error" and "load" in res.error

    @pytest.mark.parametrize(
        "change",
        [
            dict(ok=False),  # not ok, yet nothing is wrong
            dict(mismatches=3),  # mismatches without CUs, tiles or records
            dict(bad_cus=[dict(BAD_CUS[0])]),
            dict(records=[[0, 1, 2, 3, 4]]),
            dict(bad_tiles=[[0, 0, 1]]),
            dict(checksum_ok=False),  # ok with a failed checksum
            dict(iterations=0),
            dict(ok="yes"),
            dict(checksum_ok=1),
            dict(records=[[0, 1, 2, 3]], mismatches=1),
            dict(mismatches="many"),
            dict(tflops=None),
        ],
    )
    def test_a_contradictory_or_malformed_load_part_is_an_error(self, change):
        part = load_part()
        part.update(change)
        for rc in (0, 1):
            spawn = spawn_returning(rc, json.dumps(with_load(part)))
            res = selftest.run(Gpu(0), spawn=spawn, load_seconds=1)
            assert res.outcome == "error", (change, rc)
            assert res.report is None

    @pytest.mark.parametrize("missing", ["bad_cus", "mismatches", "checksum_ok", "m"])
    def test_a_load_part_without_a_key_is_an_error(self, missing):
        part = load_part(bad=True)
        del part[missing]
        spawn = spawn_returning(1, json.dumps(with_load(part)))
        assert selftest.run(Gpu(0), spawn=spawn, load_seconds=1).outcome == "error"

    def test_load_is_not_a_dict(self):
        rep = report()
        rep["load"] = [1, 2]
        spawn = spawn_returning(0, json.dumps(rep))
        assert selftest.run(Gpu(0), spawn=spawn, load_seconds=1).outcome == "error"

    def test_exit_code_must_agree_with_the_load_part(self):
        spawn = spawn_returning(0, json.dumps(with_load(load_part(bad=True))))
        assert selftest.run(Gpu(0), spawn=spawn, load_seconds=1).outcome == "error"

    def test_reasons_are_unchanged(self):
        assert [r for r, _ in REASONS if r.startswith("Selftest")] == [
            "SelftestMemoryMismatch",
            "SelftestComputeMismatch",
            "SelftestError",
        ]

    def test_child_main_hands_the_seconds_on(self, monkeypatch, capsys):
        seen = []

        def child(bdf, mib, per_cu=False, load_seconds=0.0):
            seen.append((bdf, mib, per_cu, load_seconds))
            return 0, with_load(load_part())

        monkeypatch.setattr(selftest, "_child", child)
        assert selftest.main(["--bdf", "0000:c1:00.0", "--load-seconds", "3"]) == 0
        assert seen == [("0000:c1:00.0", selftest.DEFAULT_MIB, False, 3.0)]
        out = capsys.readouterr().out
        assert "load: 1200 iteration(s) of 4096x4096x4096" in out
        assert "0 mismatch(es), checksum ok" in out
        for bad in ("-1", "601"):
            with pytest.raises(SystemExit):
                selftest.main(["--bdf", "0000:c1:00.0", "--load-seconds", bad])


# ---------------------------------------------------------------------------
# driver
# ---------------------------------------------------------------------------
def load_runner(outcomes):
    """runner(gpu, mib=, timeout_s=, load_seconds=) with a ``load`` part."""
    calls = []

    def runner(gpu, *, mib, timeout_s, load_seconds=0):
        calls.append((gpu.index, load_seconds))
        outcome = outcomes.get(gpu.index, "pass")
        part = load_part(bad=outcome == "compute")
        selftest._classify_load(part)  # as run() leaves it
        rep = with_load(part) if load_seconds else report()
        return selftest.SelftestResult(
            gpu.index, gpu.pcie_bdf, outcome, rep, "", seconds=0.25
        )

    runner.calls = calls
    return runner


GAUGES = ("dra_gpu_selftest_load_iterations", "dra_gpu_selftest_load_mismatches")


class TestDriver:
    def test_old_signature_runner_still_works_with_the_load_stage_off(self, tmp_path):
        d, _, _ = make_driver(tmp_path, gpu_indices=[0, 1])
        try:
            runner = stub_runner({})  # would reject load_seconds
            assert d.run_startup_selftest(runner, mib=64) == {0: "pass", 1: "pass"}
            assert d.run_startup_selftest(runner, mib=64, load_seconds=0) == {
                0: "pass",
                1: "pass",
            }
            for name in GAUGES:
                assert sample(d.metrics, name, gpu="0") is None
        finally:
            d.shutdown(unpublish=False)

    def test_load_seconds_reach_the_runner_and_set_the_gauges(self, tmp_path):
        d, _, _ = make_driver(tmp_path, gpu_indices=[0, 1])
        try:
            runner = load_runner({1: "compute"})
            results = d.run_startup_selftest(runner, mib=64, load_seconds=2)
            assert results == {0: "pass", 1: "compute"}
            assert runner.calls == [(0, 2), (1, 2)]
            m = d.metrics
            assert sample(m, GAUGES[0], gpu="0") == 1200
            assert sample(m, GAUGES[1], gpu="0") == 0
            assert sample(m, GAUGES[0], gpu="1") == 8
            assert sample(m, GAUGES[1], gpu="1") == 27
            assert d.health.findings(0) == []
            (f,) = d.health.findings(1)
            assert f.reason == "SelftestComputeMismatch"
            assert f.detail.startswith("load test: 27 mismatching value(s)")
        finally:
            d.shutdown(unpublish=False)


# ---------------------------------------------------------------------------
# command lines
# ---------------------------------------------------------------------------
class FakeDriver:
    def __init__(self):
        self.calls = []

    def run_startup_selftest(self, **kw):
        self.calls.append(kw)
        return {}


class TestFlags:
    def test_plugin_flag_defaults_to_off(self, monkeypatch):
        monkeypatch.delenv("SELFTEST_LOAD_SECONDS", raising=False)
        args = plugin_main.build_parser().parse_args(["--startup-selftest", "on"])
        assert args.selftest_load_seconds == 0
        drv = FakeDriver()
        assert plugin_main.startup_selftest(args, drv) is True
        assert drv.calls == [{"mib": 1024, "timeout_s": 120.0}]

    def test_plugin_flag_and_its_environment_mirror(self, monkeypatch):
        args = plugin_main.build_parser().parse_args(
            ["--startup-selftest", "on", "--selftest-load-seconds", "7.5"]
        )
        drv = FakeDriver()
        plugin_main.startup_selftest(args, drv)
        assert drv.calls == [{"mib": 1024, "timeout_s": 120.0, "load_seconds": 7.5}]
        monkeypatch.setenv("SELFTEST_LOAD_SECONDS", "3")
        args = plugin_main.build_parser().parse_args([])
        assert args.selftest_load_seconds == 3.0
        drv = FakeDriver()
        assert plugin_main.startup_selftest(args, drv) is False  # selftest off
        assert drv.calls == []

    def test_ctl_passes_the_seconds_and_prints_the_figures(self, monkeypatch, capsys):
        runner = load_runner({4: "compute"})
        monkeypatch.setattr(
            selftest, "run", lambda gpu, **kw: runner(gpu, timeout_s=0, **kw)
        )
        rc = ctl.main(
            ["--hal", "fake", "health", "--selftest", "--load-seconds", "2", "--json"]
        )
        assert rc == 1
        records = json.loads(capsys.readouterr().out)
        assert all(c == (i, 2.0) for i, c in enumerate(runner.calls))
        assert records[0]["selftest"]["load"] == {
            "iterations": 1200,
            "mismatches": 0,
            "checksum_ok": True,
            "cus_seen": 256,
            "tflops": 1.0,
            "bad_cus": [],
        }
        assert records[4]["selftest"]["result"] == "compute"
        assert records[4]["selftest"]["load"]["mismatches"] == 27
        assert ctl.main(["--hal", "fake", "health", "--selftest", "--load-seconds", "2"]) == 1
        out = capsys.readouterr().out
        assert (
            "load: 1200 iteration(s), 0 mismatch(es), checksum ok, 256 CUs "
            "seen, 1 TF/s (informative)" in out
        )
        assert "load: 8 iteration(s), 27 mismatch(es)" in out
        assert "SelftestComputeMismatch: load test: 27" in out

    def test_ctl_without_the_flag_does_not_pass_it(self, monkeypatch, capsys):
        runner = stub_runner({})  # would reject load_seconds
        monkeypatch.setattr(
            selftest, "run", lambda gpu, **kw: runner(gpu, timeout_s=0, **kw)
        )
        assert ctl.main(["--hal", "fake", "health", "--selftest", "--json"]) == 0
        records = json.loads(capsys.readouterr().out)
        assert all("load" not in r["selftest"] for r in records)

    @pytest.mark.parametrize("bad", [False, True])
    def test_workload_flag_runs_it_and_exits_1_on_a_mismatch(
        self, monkeypatch, capsys, bad
    ):
        calls = []

        def load_selftest(device, seconds):
            calls.append((device, seconds))
            return load_part(bad=bad)

        fake = types.SimpleNamespace(device_count=lambda: 2, load_selftest=load_selftest)
        monkeypatch.setattr(k8s_dra_driver_amd, "_hiphealth", fake, raising=False)
        monkeypatch.setattr(
            workload,
            "visible_devices",
            lambda: {"kfd": True, "render_nodes": ["renderD128"]},
        )
        assert workload.main(["--load-selftest", "1.5"]) == (1 if bad else 0)
        assert calls == [(0, 1.5), (1, 1.5)]
        out = capsys.readouterr().out
        if bad:
            assert "device 1: load-selftest FAILED: 8 iteration(s)" in out
            assert "6 bad CU(s): xcc 0 se 1 sh 0 cu 3" in out
        else:
            assert "device 0: load-selftest ok: 1200 iteration(s) of 4096x4096x4096" in out


# ---------------------------------------------------------------------------
# loadtest_core.hpp under AddressSanitizer and UBSan, as its own program
# ---------------------------------------------------------------------------
def test_core_selftest_program_builds_and_passes(tmp_path):
    if build_native.sanitizer_link_flags() is None:
        pytest.skip("gcc has no ASan/UBSan runtime installed")
    exe = build_native.build_loadtest_core_selftest(str(tmp_path / "lt_core_selftest"))
    done = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert done.returncode == 0, done.stdout + done.stderr[-3000:]
    assert "loadtest_core_selftest: ok" in done.stdout
    assert "Sanitizer" not in done.stderr and "runtime error" not in done.stderr


def test_the_header_is_part_of_the_extension_build():
    src = open(os.path.join(build_native.CPP_DIR, "hiphealth.hip")).read()
    assert src.index('"cutest_kernels.hpp"') < src.index('"loadtest_kernels.hpp"')
