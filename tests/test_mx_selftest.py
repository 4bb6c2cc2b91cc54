"""The MX load self-test without a GPU: the numpy mirror's formats and
exactness argument, the parent half of ``k8s_dra_driver_amd.selftest`` on a
stub child with a ``"load_mx"`` part, the driver, the command lines, and the
stand-alone sanitizer build of ``mxtest_core.hpp``.
"""

import json
import os
import subprocess
import types

import numpy as np
import pytest

import mxtest_reference as X
import k8s_dra_driver_amd
from k8s_dra_driver_amd import build_native, ctl, selftest, workload
from k8s_dra_driver_amd.plugin import main as plugin_main
from k8s_dra_driver_amd.plugin.health import REASONS

from test_selftest import Gpu, make_driver, report, sample, spawn_returning, stub_runner
from test_load_selftest import BAD_CUS, load_part, with_load

SEED = 0x0123456789ABCDEF


# ---------------------------------------------------------------------------
# the mirror: formats
# ---------------------------------------------------------------------------
class TestFormats:
    def test_all_256_e4m3_codes_are_the_ocp_values(self):
        t = X.E4M3
        assert np.isnan(t[0x7F]) and np.isnan(t[0xFF])
        assert np.isfinite(np.delete(t, [0x7F, 0xFF])).all()  # no infinities
        assert np.nanmax(t) == 448.0 == t[0x7E] and np.nanmin(t) == -448.0 == t[0xFE]
        assert t[0x00] == 0 and t[0x80] == 0 and np.signbit(t[0x80])
        # subnormals: m * 2^-9; the smallest normal is 2^-6
        assert [t[c] for c in range(1, 8)] == [m * 2.0**-9 for m in range(1, 8)]
        assert t[0x08] == 2.0**-6
        assert (t[0x38], t[0x3C], t[0x40], t[0x50]) == (1.0, 1.5, 2.0, 8.0)
        # by hand, independent of the table's formula: sign, then a
        # significand of 3 (subnormal) or 4 bits times a power of two
        for code in range(256):
            if code & 0x7F == 0x7F:
                continue
            e, m = (code >> 3) & 15, code & 7
            mag = m * 2.0**-9 if e == 0 else (8 + m) * 2.0 ** (e - 10)
            assert t[code] == (-mag if code & 0x80 else mag)
        pos = t[:0x7F]
        assert (np.diff(pos) > 0).all()  # strictly increasing in the code
        assert (t[0x80:0xFF] == -pos).all()

    def test_all_16_e2m1_codes(self):
        assert X.E2M1.tolist() == [
            0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0,
            -0.0, -0.5, -1.0, -1.5, -2.0, -3.0, -4.0, -6.0,
        ]
        assert np.signbit(X.E2M1[8]) and not np.signbit(X.E2M1[0])

    def test_e8m0(self):
        assert X.e8m0([127, 126, 128, 117, 137]).tolist() == [
            1.0, 0.5, 2.0, 2.0**-10, 2.0**10,
        ]
        assert X.e8m0([0])[0] == 2.0**-127 and np.isnan(X.e8m0([255])[0])

    def test_encode_inverts_decode_and_rejects_what_does_not_fit(self):
        for fmt in X.FORMATS:
            tab = X.table(fmt)
            codes = np.array(
                [c for c in range(len(tab)) if not np.isnan(tab[c]) and tab[c] != 0]
            )
            assert (X.encode(fmt, tab[codes]) == codes).all()
            assert X.encode(fmt, [0.0])[0] == 0
        for fmt, bad in (("mxfp4", 5.0), ("mxfp4", 0.25), ("mxfp8", 17.0), ("mxfp8", 449.0)):
            with pytest.raises(ValueError):
                X.encode(fmt, [bad])

    def test_pack_and_unpack(self):
        codes = np.arange(32, dtype=np.uint8).reshape(2, 16) % 16
        packed = X.pack("mxfp4", codes)
        assert packed.shape == (2, 8)
        assert packed[0, 0] == 0x10 and packed[0, 1] == 0x32  # even k low
        assert (X.unpack("mxfp4", packed, 16) == codes).all()
        assert (X.pack("mxfp8", codes) == codes).all()
        assert X.row_bytes("mxfp4", 128) == 64 and X.row_bytes("mxfp8", 128) == 128

    def test_the_lane_map(self):
        for fmt in X.FORMATS:
            seen = set()
            for row in range(16):
                for k in range(128):
                    lane, j = X.operand_lane(fmt, row, k)
                    assert lane % 16 == row and 0 <= lane < 64 and 0 <= j < 32
                    seen.add((lane, j))
            assert len(seen) == 64 * 32  # a bijection
        assert X.operand_lane("mxfp4", 3, 40) == (16 + 3, 8)
        # mxfp8: a lane's two halves lie in two k-blocks, 64 apart
        assert X.operand_lane("mxfp8", 3, 40) == (2 * 16 + 3, 8)
        assert X.operand_lane("mxfp8", 3, 104) == (2 * 16 + 3, 24)
        assert X.operand_lane("mxfp8", 3, 15) == (3, 15)
        assert X.operand_lane("mxfp8", 3, 16) == (16 + 3, 0)
        assert X.scale_lane(3, 2) == 35
        assert {X.result_lane(r, c) for r in range(16) for c in range(16)} == {
            (lane, reg) for lane in range(64) for reg in range(4)
        }
        assert X.result_lane(9, 3) == (2 * 16 + 3, 1)


# ---------------------------------------------------------------------------
# the mirror: generator and the exactness argument
# ---------------------------------------------------------------------------
# what mxtest_core_selftest.cpp asserts of the C++ generator: row 3, codes of
# k = 0..7, both scale bytes of k < 64, quarter units of k = 30..33
FIXED = {
    ("mxfp8", 0): ([202, 202, 204, 196, 192, 74, 56, 78], [128, 128], [32, -56, -8, -64]),
    ("mxfp8", 1): ([206, 200, 192, 184, 202, 64, 72, 206], [126, 127], [-6, 10, -12, -32]),
    ("mxfp4", 0): ([9, 8, 15, 10, 11, 4, 4, 9], [126, 127], [-8, 4, -12, -16]),
    ("mxfp4", 1): ([11, 5, 1, 14, 15, 5, 4, 3], [126, 128], [4, -12, 32, 0]),
}


class TestGenerator:
    @pytest.mark.parametrize("fmt", X.FORMATS)
    def test_generated_values_stay_inside_the_stated_sets(self, fmt):
        for which in (0, 1):
            codes, scales, q = X.generate(SEED, fmt, which, 256, 256)
            assert set(np.unique(scales).tolist()) == {126, 127, 128}
            v = X.decode(fmt, codes)
            if fmt == "mxfp4":
                assert set(np.unique(codes).tolist()) == set(range(16))
                assert (v * 2 == np.rint(v * 2)).all() and np.abs(v).max() == 6
                assert np.abs(q).max() == 48  # 12.0
            else:
                assert set(np.unique(v).tolist()) == set(range(-8, 9))
                assert np.abs(q).max() == 64 and (q % 2 == 0).all()
            assert np.abs(q).max() == X.MAX_QUARTER[fmt]
            assert (q == np.rint(v * np.repeat(X.e8m0(scales), 32, axis=1) * 4)).all()
        a = X.generate(SEED, fmt, 0, 8, 128)
        b = X.generate(SEED, fmt, 1, 8, 128)
        assert (a[0] != b[0]).any() and (a[1] != b[1]).any()
        assert (X.generate(SEED + 1, fmt, 0, 8, 128)[0] != a[0]).any()

    def test_fixed_vectors_shared_with_the_host_core(self):
        for (fmt, which), (codes, scales, quarter) in FIXED.items():
            c, s, q = X.generate(SEED, fmt, which, 4, 64)
            assert c[3, :8].tolist() == codes
            assert s[3].tolist() == scales
            assert q[3, 30:34].tolist() == quarter

    def test_one_value_by_hand(self):
        mix = X.S.mix_int
        m64 = 2**64 - 1
        for f, fmt in enumerate(X.FORMATS):
            base = ((f + 1) << 60) | (1 << 56) | (5 << 28)
            r = mix((SEED + (base | 70)) & m64)
            rs = mix((SEED + (base | (1 << 57) | 2)) & m64)
            scale = 126 + (rs >> 32) % 3
            codes, scales, _ = X.generate(SEED, fmt, 1, 6, 128)
            assert int(scales[5, 2]) == scale
            if fmt == "mxfp4":
                assert int(codes[5, 70]) == r % 16
            else:
                assert X.E4M3[codes[5, 70]] == r % 17 - 8

    @pytest.mark.parametrize("fmt", X.FORMATS)
    def test_the_bound_holds_at_the_cap_and_fails_one_step_above(self, fmt):
        cap = X.MAX_K[fmt]
        assert cap % X.BK == 0 and cap >= 4096
        assert X.bound_holds(fmt, cap) and not X.bound_holds(fmt, cap + X.BK)
        top = {"mxfp8": 8.0, "mxfp4": 6.0}[fmt]
        codes = np.full((1, cap + X.BK), X.encode(fmt, [top])[0], dtype=np.uint8)
        scales = np.full((1, (cap + X.BK) // 32), 128, dtype=np.uint8)
        q = X.quarter_units(fmt, codes, scales)
        assert (q == X.MAX_QUARTER[fmt]).all()
        at_cap = X.gemm_units(q[:, :cap], q[:, :cap])[0, 0]
        above = X.gemm_units(q, q)[0, 0]
        assert at_cap == X.MAX_QUARTER[fmt] ** 2 * cap <= X.BOUND_UNITS[fmt] < above
        assert float(X.to_f32([at_cap])[0]) == at_cap / 16
        # with the lowest unit the derivation allows set, the cap's largest
        # sum is still exact and the one above it is not
        unit = 4 if fmt == "mxfp8" else 1
        X.to_f32([at_cap - X.MAX_QUARTER[fmt] ** 2 + unit])
        if fmt == "mxfp4":
            with pytest.raises(ValueError):
                X.to_f32([above + unit])
        with pytest.raises(ValueError):
            X.to_f32([(1 << 24) + 1])

    @pytest.mark.parametrize("fmt", X.FORMATS)
    def test_float32_accumulation_in_any_order_equals_the_integers(self, fmt):
        k = X.MAX_K[fmt]
        rng = np.random.default_rng(7)
        q = X.MAX_QUARTER[fmt]
        a = np.full(k, q, dtype=np.int64)
        b = np.full(k, q, dtype=np.int64)
        a[17] = b[17] = 2 if fmt == "mxfp8" else 1
        prod = (a * b / 16.0).astype(np.float32)
        want = X.to_f32(X.gemm_units(a[None, :], b[None, :]))[0, 0]
        # grouped as the instruction may group: partial sums of 128, then
        # their sum, in a random order
        parts = prod[rng.permutation(k)].reshape(-1, 128)
        partial = np.zeros(parts.shape[0], dtype=np.float32)
        for j in range(128):
            partial = (partial + parts[:, j]).astype(np.float32)
        acc = np.float32(0)
        for p in partial:
            acc = np.float32(acc + p)
        assert acc == want

    def test_checksum_is_the_sum_of_the_product(self):
        for fmt in X.FORMATS:
            a = X.generate(SEED, fmt, 0, 128, 256)[2]
            bt = X.generate(SEED, fmt, 1, 256, 256)[2]
            c = X.gemm_units(a, bt)
            rows, cols = X.checksum(a, bt)
            assert (rows == c.sum(axis=1)).all() and (cols == c.sum(axis=0)).all()


# ---------------------------------------------------------------------------
# selftest.run on a stub child
# ---------------------------------------------------------------------------
def mx_part(fmt, bad=False, checksum_ok=True):
    part = load_part(bad=bad, checksum_ok=checksum_ok)
    part["format"] = fmt
    part["golden_seconds"] = 2.0
    return part


def with_mx(parts):
    rep = with_load(load_part())
    rep["load_mx"] = parts
    rep["ok"] = rep["ok"] and all(p["ok"] for p in parts.values())
    return rep


BOTH = ("mxfp8", "mxfp4")


class TestRun:
    def test_argv_carries_the_formats_and_the_limit_grows_per_format(self):
        rep = with_mx({f: mx_part(f) for f in BOTH})
        spawn = spawn_returning(0, json.dumps(rep))
        res = selftest.run(
            Gpu(0), mib=64, timeout_s=30, spawn=spawn, load_seconds=2.5,
            load_formats=BOTH,
        )
        assert res.outcome == "pass", res.error
        assert res.findings() == []
        argv, limit = spawn.calls[0]
        assert argv[-5:] == ["--json", "--load-seconds", "2.5", "--load-formats",
                             "mxfp8,mxfp4"]
        assert limit == (30 + 2.5 + selftest.LOAD_GOLDEN_ALLOWANCE_S
                         + 2 * (2.5 + selftest.MX_GOLDEN_ALLOWANCE_S))
        # the order given is the order asked of the child; the child prints
        # its report with sorted keys, and the result is in the order asked
        for asked in ("mxfp4,mxfp8", "mxfp8,mxfp4"):
            rep = with_mx({f: mx_part(f) for f in BOTH})
            spawn = spawn_returning(0, json.dumps(rep, sort_keys=True))
            res = selftest.run(Gpu(0), spawn=spawn, load_seconds=1, load_formats=asked)
            assert res.outcome == "pass", res.error
            assert spawn.calls[0][0][-1] == asked
            assert list(res.report["load_mx"]) == asked.split(",")

    def test_without_formats_nothing_changes(self):
        spawn = spawn_returning(0, json.dumps(with_load(load_part())))
        res = selftest.run(Gpu(0), timeout_s=30, spawn=spawn, load_seconds=2)
        assert res.outcome == "pass"
        argv, limit = spawn.calls[0]
        assert "--load-formats" not in argv
        assert limit == 30 + 2 + selftest.LOAD_GOLDEN_ALLOWANCE_S
        assert "load_mx" not in res.report

    def test_formats_need_load_seconds_and_known_names(self):
        for kw in (
            dict(load_formats=BOTH),
            dict(load_formats=BOTH, load_seconds=0),
            dict(load_formats=("mxfp6",), load_seconds=1),
            dict(load_formats="mxfp8,bf16", load_seconds=1),
            dict(load_formats=("mxfp8", "mxfp8"), load_seconds=1),
        ):
            spawn = spawn_returning(0, json.dumps(report()))
            res = selftest.run(Gpu(0), spawn=spawn, **kw)
            assert res.outcome == "error", kw
            assert spawn.calls == []  # no child was started
            (f,) = res.findings()
            assert f.reason == "SelftestError"

    def test_a_mismatching_part_is_one_compute_finding_named_by_format(self):
        rep = with_mx({"mxfp8": mx_part("mxfp8"), "mxfp4": mx_part("mxfp4", bad=True)})
        spawn = spawn_returning(1, json.dumps(rep))
        res = selftest.run(Gpu(0), spawn=spawn, load_seconds=1, load_formats=BOTH)
        assert res.outcome == "compute", res.error
        (f,) = res.findings()
        assert f.reason == "SelftestComputeMismatch"
        assert dict(REASONS)[f.reason] == f.severity
        assert f.detail == (
            "mxfp4 load test: 27 mismatching value(s) in 8 iteration(s) of "
            "4096x4096x4096; 6 of 256 CU(s) seen bad: "
            "xcc 0 se 1 sh 0 cu 3 (2), xcc 1 se 1 sh 0 cu 3 (3), "
            "xcc 2 se 1 sh 0 cu 3 (4), xcc 3 se 1 sh 0 cu 3 (5), and 2 more; "
            "first recorded value: iteration 2 row 9 col 300: "
            "got 0x00000001, want 0x00000002"
        )

    def test_a_failed_checksum_is_a_compute_failure(self):
        rep = with_mx({"mxfp8": mx_part("mxfp8", checksum_ok=False)})
        spawn = spawn_returning(1, json.dumps(rep))
        res = selftest.run(Gpu(0), spawn=spawn, load_seconds=1, load_formats=("mxfp8",))
        assert res.outcome == "compute", res.error
        (f,) = res.findings()
        assert f.detail.startswith("mxfp8 load test: 0 mismatching value(s)")
        assert f.detail.endswith("golden product failed its checksum at row 12")

    def test_both_parts_bad_are_two_findings(self):
        rep = with_mx({f: mx_part(f, bad=True) for f in BOTH})
        spawn = spawn_returning(1, json.dumps(rep))
        res = selftest.run(Gpu(0), spawn=spawn, load_seconds=1, load_formats=BOTH)
        assert [f.detail.split()[0] for f in res.findings()] == list(BOTH)

    def test_a_missing_or_unasked_part_is_an_error(self):
        spawn = spawn_returning(0, json.dumps(with_load(load_part())))
        res = selftest.run(Gpu(0), spawn=spawn, load_seconds=1, load_formats=BOTH)
        assert res.outcome == "error" and "load_mx" in res.error
        rep = with_mx({"mxfp8": mx_part("mxfp8")})
        spawn = spawn_returning(0, json.dumps(rep))
        res = selftest.run(Gpu(0), spawn=spawn, load_seconds=1)
        assert res.outcome == "error" and "load_mx" in res.error

    @pytest.mark.parametrize(
        "parts",
        [
            {"mxfp8": mx_part("mxfp8")},  # one of the two asked for
            {"mxfp8": mx_part("mxfp8"), "mxfp4": mx_part("mxfp8")},  # wrong name inside
            {"mxfp8": mx_part("mxfp8"), "mxfp4": mx_part("mxfp4"), "mxfp6": mx_part("mxfp6")},
            {"mxfp8": mx_part("mxfp8"), "mxfp4": [1, 2]},
            {"mxfp8": mx_part("mxfp8"), "mxfp4": {**mx_part("mxfp4"), "format": None}},
            [mx_part("mxfp8"), mx_part("mxfp4")],
        ],
    )
    def test_parts_that_do_not_match_what_was_asked_are_an_error(self, parts):
        rep = with_load(load_part())
        rep["load_mx"] = parts
        for rc in (0, 1):
            spawn = spawn_returning(rc, json.dumps(rep))
            res = selftest.run(Gpu(0), spawn=spawn, load_seconds=1, load_formats=BOTH)
            assert res.outcome == "error", rc
            assert res.report is None

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
    def test_an_inconsistent_part_is_an_error(self, change):
        part = mx_part("mxfp4")
        part.update(change)
        rep = with_load(load_part())
        rep["load_mx"] = {"mxfp8": mx_part("mxfp8"), "mxfp4": part}
        for rc in (0, 1):
            spawn = spawn_returning(rc, json.dumps(rep))
            res = selftest.run(Gpu(0), spawn=spawn, load_seconds=1, load_formats=BOTH)
            assert res.outcome == "error", (change, rc)
            assert "load_mx['mxfp4']" in res.error or "malformed" in res.error
            assert res.report is None

    @pytest.mark.parametrize("missing", ["bad_cus", "mismatches", "checksum_ok", "m", "format"])
    def test_a_part_without_a_key_is_an_error(self, missing):
        part = mx_part("mxfp8", bad=True)
        del part[missing]
        spawn = spawn_returning(1, json.dumps(with_mx({"mxfp8": part}) if missing != "format"
                                              else {**with_load(load_part()),
                                                    "load_mx": {"mxfp8": part}, "ok": False}))
        res = selftest.run(Gpu(0), spawn=spawn, load_seconds=1, load_formats=("mxfp8",))
        assert res.outcome == "error"

    def test_exit_code_must_agree_with_the_parts(self):
        rep = with_mx({"mxfp8": mx_part("mxfp8", bad=True)})
        spawn = spawn_returning(0, json.dumps(rep))
        res = selftest.run(Gpu(0), spawn=spawn, load_seconds=1, load_formats=("mxfp8",))
        assert res.outcome == "error"

    def test_a_report_without_load_mx_has_the_findings_it_had(self):
        rep = with_load(load_part(bad=True))
        res = selftest.SelftestResult(0, "b", "compute", rep)
        (f,) = res.findings()
        assert f.detail.startswith("load test: 27 mismatching value(s)")

    def test_child_main_hands_the_formats_on(self, monkeypatch, capsys):
        seen = []

        def child(bdf, mib, per_cu=False, load_seconds=0.0, load_formats=()):
            seen.append((bdf, mib, per_cu, load_seconds, load_formats))
            return 0, with_mx({f: mx_part(f) for f in load_formats})

        monkeypatch.setattr(selftest, "_child", child)
        argv = ["--bdf", "0000:c1:00.0", "--load-seconds", "3"]
        assert selftest.main(argv + ["--load-formats", "mxfp4,mxfp8"]) == 0
        assert seen == [("0000:c1:00.0", selftest.DEFAULT_MIB, False, 3.0, ("mxfp4", "mxfp8"))]
        out = capsys.readouterr().out
        assert "load mxfp4: 1200 iteration(s) of 4096x4096x4096" in out
        assert "load mxfp8: 1200 iteration(s)" in out
        assert out.index("load mxfp4") < out.index("load mxfp8")
        for bad in (
            ["--bdf", "b", "--load-formats", "mxfp8"],  # no --load-seconds
            ["--bdf", "b", "--load-seconds", "0", "--load-formats", "mxfp8"],
            argv + ["--load-formats", "mxfp6"],
            argv + ["--load-formats", "mxfp8,mxfp8"],
        ):
            with pytest.raises(SystemExit):
                selftest.main(bad)
        assert len(seen) == 1

    def test_the_child_runs_each_format_after_the_bf16_stage(self, monkeypatch):
        order = []

        def selftest_stub(ordinal, mib):
            order.append("base")
            return report()

        def load_stub(ordinal, seconds):
            order.append(("load", seconds))
            return load_part()

        def mx_stub(ordinal, fmt, seconds):
            order.append((fmt, seconds))
            return mx_part(fmt, bad=fmt == "mxfp4")

        fake = types.SimpleNamespace(
            device_count=lambda: 1,
            pci_bus_id=lambda o: "0000:C1:00.0",
            selftest=selftest_stub,
            load_selftest=load_stub,
            mx_selftest=mx_stub,
        )
        monkeypatch.setattr(k8s_dra_driver_amd, "_hiphealth", fake, raising=False)
        rc, rep = selftest._child("0000:c1:00.0", 64, False, 2.0, ("mxfp4", "mxfp8"))
        assert order == ["base", ("load", 2.0), ("mxfp4", 2.0), ("mxfp8", 2.0)]
        assert rc == selftest.EXIT_MISMATCH and rep["ok"] is False
        assert list(rep["load_mx"]) == ["mxfp4", "mxfp8"]
        rc, rep = selftest._child("0000:c1:00.0", 64, False, 2.0)
        assert rc == selftest.EXIT_PASS and "load_mx" not in rep

    def test_parse_load_formats(self):
        assert selftest.LOAD_FORMATS == X.FORMATS
        assert selftest.parse_load_formats("") == ()
        assert selftest.parse_load_formats(()) == ()
        assert selftest.parse_load_formats(" mxfp4 , mxfp8 ") == ("mxfp4", "mxfp8")
        assert selftest.parse_load_formats(["mxfp8"]) == ("mxfp8",)


# ---------------------------------------------------------------------------
# driver
# ---------------------------------------------------------------------------
def mx_runner(outcomes):
    """runner(gpu, mib=, timeout_s=, load_seconds=, load_formats=) with a
    ``load_mx`` part; the mxfp4 part is the bad one of a compute outcome."""
    calls = []

    def runner(gpu, *, mib, timeout_s, load_seconds=0, load_formats=()):
        calls.append((gpu.index, load_seconds, load_formats))
        outcome = outcomes.get(gpu.index, "pass")
        rep = with_load(load_part()) if load_seconds else report()
        if load_formats:
            rep = with_mx(
                {f: mx_part(f, bad=outcome == "compute" and f == "mxfp4")
                 for f in load_formats}
            )
        selftest._classify(rep, load_formats)  # as run() leaves it
        return selftest.SelftestResult(
            gpu.index, gpu.pcie_bdf, outcome, rep, "", seconds=0.25
        )

    runner.calls = calls
    return runner


MX_GAUGES = ("dra_gpu_selftest_mx_iterations", "dra_gpu_selftest_mx_mismatches")
LOAD_GAUGES = ("dra_gpu_selftest_load_iterations", "dra_gpu_selftest_load_mismatches")


class TestDriver:
    def test_formats_reach_the_runner_and_set_the_gauges(self, tmp_path):
        d, _, _ = make_driver(tmp_path, gpu_indices=[0, 1])
        try:
            runner = mx_runner({1: "compute"})
            results = d.run_startup_selftest(
                runner, mib=64, load_seconds=2, load_formats=["mxfp8", "mxfp4"]
            )
            assert results == {0: "pass", 1: "compute"}
            assert runner.calls == [(0, 2, BOTH), (1, 2, BOTH)]
            m = d.metrics
            for fmt in BOTH:
                assert sample(m, MX_GAUGES[0], gpu="0", format=fmt) == 1200
                assert sample(m, MX_GAUGES[1], gpu="0", format=fmt) == 0
            assert sample(m, MX_GAUGES[0], gpu="1", format="mxfp8") == 1200
            assert sample(m, MX_GAUGES[0], gpu="1", format="mxfp4") == 8
            assert sample(m, MX_GAUGES[1], gpu="1", format="mxfp4") == 27
            # the load gauges keep their labels
            assert sample(m, LOAD_GAUGES[0], gpu="1") == 1200
            assert sample(m, LOAD_GAUGES[1], gpu="1") == 0
            assert d.health.findings(0) == []
            (f,) = d.health.findings(1)
            assert f.reason == "SelftestComputeMismatch"
            assert f.detail.startswith("mxfp4 load test: 27 mismatching value(s)")
        finally:
            d.shutdown(unpublish=False)

    def test_without_formats_the_runner_is_called_as_before(self, tmp_path):
        d, _, _ = make_driver(tmp_path, gpu_indices=[0])
        try:
            runner = stub_runner({})  # would reject load_formats
            assert d.run_startup_selftest(runner, mib=64) == {0: "pass"}
            assert d.run_startup_selftest(runner, mib=64, load_formats=()) == {0: "pass"}
            for name in MX_GAUGES:
                for fmt in BOTH:
                    assert sample(d.metrics, name, gpu="0", format=fmt) is None
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
    def test_plugin_flag_defaults_to_empty(self, monkeypatch):
        monkeypatch.delenv("SELFTEST_LOAD_FORMATS", raising=False)
        args = plugin_main.build_parser().parse_args(
            ["--startup-selftest", "on", "--selftest-load-seconds", "2"]
        )
        assert args.selftest_load_formats == ""
        drv = FakeDriver()
        assert plugin_main.startup_selftest(args, drv) is True
        assert drv.calls == [{"mib": 1024, "timeout_s": 120.0, "load_seconds": 2.0}]

    def test_plugin_flag_and_its_environment_mirror(self, monkeypatch):
        args = plugin_main.build_parser().parse_args(
            ["--startup-selftest", "on", "--selftest-load-seconds", "2",
             "--selftest-load-formats", "mxfp8,mxfp4"]
        )
        drv = FakeDriver()
        plugin_main.startup_selftest(args, drv)
        assert drv.calls == [
            {"mib": 1024, "timeout_s": 120.0, "load_seconds": 2.0, "load_formats": BOTH}
        ]
        monkeypatch.setenv("SELFTEST_LOAD_FORMATS", "mxfp4")
        args = plugin_main.build_parser().parse_args(["--selftest-load-seconds", "1"])
        assert args.selftest_load_formats == "mxfp4"
        assert plugin_main.selftest_load_formats(args) == ("mxfp4",)

    def test_plugin_rejects_formats_it_cannot_run(self):
        parse = plugin_main.build_parser().parse_args
        for argv in (
            ["--selftest-load-formats", "mxfp8"],  # no load seconds
            ["--selftest-load-seconds", "2", "--selftest-load-formats", "fp8"],
        ):
            with pytest.raises(ValueError):
                plugin_main.selftest_load_formats(parse(argv))

    def test_ctl_passes_the_formats_and_prints_the_figures(self, monkeypatch, capsys):
        runner = mx_runner({4: "compute"})
        monkeypatch.setattr(
            selftest, "run", lambda gpu, **kw: runner(gpu, timeout_s=0, **kw)
        )
        argv = ["--hal", "fake", "health", "--selftest", "--load-seconds", "2",
                "--load-formats", "mxfp8,mxfp4"]
        assert ctl.main(argv + ["--json"]) == 1
        records = json.loads(capsys.readouterr().out)
        assert all(c == (i, 2.0, BOTH) for i, c in enumerate(runner.calls))
        assert records[0]["selftest"]["load_mx"]["mxfp4"] == {
            "iterations": 1200,
            "mismatches": 0,
            "checksum_ok": True,
            "cus_seen": 256,
            "tflops": 1.0,
            "bad_cus": [],
        }
        assert list(records[0]["selftest"]["load_mx"]) == ["mxfp4", "mxfp8"]  # sorted JSON
        assert records[4]["selftest"]["result"] == "compute"
        assert records[4]["selftest"]["load_mx"]["mxfp4"]["mismatches"] == 27
        assert records[4]["selftest"]["load"]["mismatches"] == 0
        assert ctl.main(argv) == 1
        out = capsys.readouterr().out
        assert (
            "load mxfp8: 1200 iteration(s), 0 mismatch(es), checksum ok, 256 CUs "
            "seen, 1 TF/s (informative)" in out
        )
        assert "load mxfp4: 8 iteration(s), 27 mismatch(es)" in out
        assert "SelftestComputeMismatch: mxfp4 load test: 27" in out

    def test_ctl_rejects_formats_it_cannot_run(self, capsys):
        for argv in (
            ["health", "--selftest", "--load-formats", "mxfp8"],
            ["health", "--load-seconds", "2", "--load-formats", "mxfp8"],
            ["health", "--selftest", "--load-seconds", "2", "--load-formats", "mxfp6"],
        ):
            with pytest.raises(SystemExit):
                ctl.main(["--hal", "fake"] + argv)
        capsys.readouterr()

    @pytest.mark.parametrize("bad", [False, True])
    def test_workload_flag_runs_it_and_exits_1_on_a_mismatch(
        self, monkeypatch, capsys, bad
    ):
        calls = []

        def mx_selftest(device, fmt, seconds):
            calls.append((device, fmt, seconds))
            return mx_part(fmt, bad=bad)

        fake = types.SimpleNamespace(device_count=lambda: 2, mx_selftest=mx_selftest)
        monkeypatch.setattr(k8s_dra_driver_amd, "_hiphealth", fake, raising=False)
        monkeypatch.setattr(
            workload,
            "visible_devices",
            lambda: {"kfd": True, "render_nodes": ["renderD128"]},
        )
        assert workload.main(["--mx-selftest", "mxfp4", "1.5"]) == (1 if bad else 0)
        assert calls == [(0, "mxfp4", 1.5), (1, "mxfp4", 1.5)]
        out = capsys.readouterr().out
        if bad:
            assert "device 1: mx-selftest mxfp4 FAILED: 8 iteration(s)" in out
            assert "6 bad CU(s): xcc 0 se 1 sh 0 cu 3" in out
        else:
            assert "device 0: mx-selftest mxfp4 ok: 1200 iteration(s) of 4096x4096x4096" in out

    def test_workload_rejects_a_bad_format_or_time(self, capsys):
        for argv in (["mxfp6", "1"], ["mxfp8", "0"], ["mxfp8", "soon"], ["mxfp8", "601"]):
            with pytest.raises(SystemExit):
                workload.main(["--mx-selftest"] + argv)
        capsys.readouterr()


# ---------------------------------------------------------------------------
# mxtest_core.hpp under AddressSanitizer and UBSan, as its own program
# ---------------------------------------------------------------------------
def test_core_selftest_program_builds_and_passes(tmp_path):
    if build_native.sanitizer_link_flags() is None:
        pytest.skip("gcc has no ASan/UBSan runtime installed")
    exe = build_native.build_mxtest_core_selftest(str(tmp_path / "mx_core_selftest"))
    done = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert done.returncode == 0, done.stdout + done.stderr[-3000:]
    assert "mxtest_core_selftest: ok" in done.stdout
    assert done.stderr == ""


def test_the_headers_are_part_of_the_extension_build(monkeypatch):
    src = open(os.path.join(build_native.CPP_DIR, "hiphealth.hip")).read()
    assert src.index('"loadtest_kernels.hpp"') < src.index('"mxtest_kernels.hpp"')
    kern = open(os.path.join(build_native.CPP_DIR, "mxtest_kernels.hpp")).read()
    core = open(os.path.join(build_native.CPP_DIR, "mxtest_core.hpp")).read()
    assert '#include "mxtest_core.hpp"' in kern
    for banned in ("hip/hip_runtime.h", "pybind11"):
        assert banned not in core
    # a change to either header rebuilds the extension
    asked = []
    monkeypatch.setattr(
        build_native, "_needs_build", lambda src, out: asked.append(src) or False
    )
    build_native.build_hiphealth()
    names = [os.path.basename(p) for p in asked]
    assert "mxtest_kernels.hpp" in names and "mxtest_core.hpp" in names
    assert "loadtest_kernels.hpp" in names and "hiphealth.hip" in names
