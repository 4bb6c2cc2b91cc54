"""The HBM march self-test without a GPU: the numpy reference against cases
written out by hand, the parent half of ``k8s_dra_driver_amd.selftest`` on a
stub child with an ``"hbm"`` part, the driver, the command lines, and the
stand-alone sanitizer build of ``hbmtest_core.hpp``.
"""

import json
import os
import subprocess
import types

import numpy as np
import pytest

import hbmtest_reference as H
import selftest_reference as S
import k8s_dra_driver_amd
from k8s_dra_driver_amd import build_native, ctl, selftest, workload
from k8s_dra_driver_amd.plugin import main as plugin_main
from k8s_dra_driver_amd.plugin.health import REASONS

from test_selftest import Gpu, make_driver, report, sample, spawn_returning, stub_runner

GIB = 1 << 30
MIB = 1 << 20
M64 = 2**64 - 1
SEED = 0x0123456789ABCDEF


# ---------------------------------------------------------------------------
# the reference, against cases written out by hand
# ---------------------------------------------------------------------------
class TestReference:
    def test_round_0_with_a_seed_known_from_the_splitmix_answers(self):
        # seed_0 = mix(seed + 0): mix(0) and mix(1) are the known answers
        assert H.round_of(0, 0) == ("addr", 0xE220A8397B1DCDAF)
        assert H.round_of(1, 0) == ("addr", 0x910A2DEC89025CC1)
        got = H.words(0, 0, 0, 4).tolist()
        assert got == [w ^ 0xE220A8397B1DCDAF for w in range(4)]
        # the next cycle of seed 0 has the seed of the first cycle of seed 1
        assert H.round_of(0, 4) == ("addr", 0x910A2DEC89025CC1)
        assert H.round_of(M64, 4) == ("addr", 0xE220A8397B1DCDAF)  # wraps

    def test_the_patterns_come_in_the_order_of_the_startup_test(self):
        assert [H.round_of(SEED, r)[0] for r in range(8)] == list(S.PATTERNS) * 2
        for r in range(8):
            assert H.round_of(SEED, r)[1] == S.mix_int(SEED + r // 4)
        # and are the startup test's patterns at the cycle's seed
        s1 = S.mix_int(SEED + 1)
        for r, name in enumerate(S.PATTERNS):
            assert np.array_equal(
                H.words(SEED, 4 + r, 0, 100), S.pattern_words(name, 100, s1)
            )

    @pytest.mark.parametrize("q", [0, 1, 5])
    def test_round_4q_plus_1_is_the_complement_of_4q(self, q):
        a = H.words(SEED, 4 * q, 12345, 1000)
        b = H.words(SEED, 4 * q + 1, 12345, 1000)
        assert np.array_equal(a ^ b, np.full(1000, M64, dtype=np.uint64))
        c = H.words(SEED, 4 * q + 2, 12345, 1000)
        d = H.words(SEED, 4 * q + 3, 12345, 1000)
        assert np.array_equal(c ^ d, np.full(1000, M64, dtype=np.uint64))
        # so every bit holds both values in consecutive rounds
        assert H.word(SEED, 4 * q + 2, 7) == S.mix_int((7 + S.mix_int(SEED + q)) & M64)

    def test_word0_of_chunk_2_continues_chunk_1(self):
        chunks = H.plan(3 * 4096 + 1024, 4096)
        assert chunks == [(4096, 0), (4096, 512), (4096, 1024), (1024, 1536)]
        whole = H.words(SEED, 6, 0, 1664).astype("<u8").tobytes()
        assert b"".join(H.contents(SEED, 6, chunks)) == whole
        last_of_1 = np.frombuffer(H.contents(SEED, 0, chunks)[1], dtype="<u8")[-1]
        first_of_2 = np.frombuffer(H.contents(SEED, 0, chunks)[2], dtype="<u8")[0]
        s0 = S.mix_int(SEED)
        assert (int(last_of_1), int(first_of_2)) == (1023 ^ s0, 1024 ^ s0)
        assert [H.chunk_of(chunks, w) for w in (0, 511, 512, 1535, 1536, 1663)] == [
            0, 0, 1, 2, 3, 3,
        ]
        with pytest.raises(ValueError):
            H.chunk_of(chunks, 1664)

    def test_the_production_plan(self):
        assert H.plan(2 * GIB + 6 * MIB) == [
            (GIB, 0), (GIB, GIB // 8), (6 * MIB, 2 * GIB // 8),
        ]
        assert H.plan(GIB) == [(GIB, 0)] and H.plan(0) == []
        assert H.reserve(64 * GIB) == 2 * GIB
        assert H.reserve(288 * 10**9) == 5_760_000_000
        assert H.target(10 * GIB + 3 * MIB + 5, 16 * GIB) == 8 * GIB + 2 * MIB
        assert H.target(GIB, 16 * GIB) == 0
        assert H.target(5, 16 * GIB, mib=1025) == GIB

    def test_the_direction_by_cycle(self):
        assert [H.descending(p, 9) for p in range(10)] == (
            [False] * 4 + [True] * 4 + [False] * 2
        )
        # the closing verify goes the way of the last round
        assert H.descending(4, 4) is False and H.descending(5, 5) is True
        assert H.descending(8, 8) is True and H.descending(1, 1) is False

    def test_a_flip_in_pass_r_is_expected_in_pass_r_only(self):
        chunks = H.plan(3 * 4096 + 1024, 4096)
        clean = H.expected(SEED, 9, chunks, [])
        assert clean["ok"] and clean["passes"] == 10 and clean["rounds"] == 9
        assert clean["records"] == set() and clean["flipped_or"] == 0
        assert clean["contents"] == H.contents(SEED, 8, chunks)
        # a flip before pass 3 shows as round 2's word in pass 3, and pass 3
        # writes round 3 over it; the flip of pass 6 never happens
        want = H.word(SEED, 2, 600)
        got = H.expected(SEED, 9, chunks, [(3, 600, 1 << 40), (6, 0, 1)])
        assert got["records"] == {(3, 600, want ^ (1 << 40), want)}
        assert want == S.mix_int((600 + S.mix_int(SEED)) & M64)
        assert (got["passes"], got["rounds"], got["mismatches"]) == (4, 4, 1)
        assert got["flipped_or"] == 1 << 40 and not got["ok"]
        assert got["bad_chunks"] == [(1, 1)]
        assert got["bad_pages"] == 1 and got["bad_pages_first"] == [(1, 0)]
        assert got["contents"] == H.contents(SEED, 3, chunks)
        # in the closing verify the flipped word stays as it is
        got = H.expected(SEED, 4, chunks, [(4, 1663, 3)])
        want = H.word(SEED, 3, 1663)
        assert got["records"] == {(4, 1663, want ^ 3, want)}
        assert (got["passes"], got["rounds"]) == (5, 4)
        held = np.frombuffer(got["contents"][3], dtype="<u8")
        assert int(held[-1]) == want ^ 3
        assert got["contents"][:3] == H.contents(SEED, 3, chunks)[:3]
        # masks on one word combine, and a pass whose masks cancel is clean
        got = H.expected(SEED, 4, chunks, [(2, 5, 1), (2, 5, 1), (3, 5, 6), (3, 5, 1)])
        assert got["passes"] == 4 and got["flipped_or"] == 7

    def test_pages_are_counted_inside_their_chunk(self):
        chunks = H.plan(2 * (2 * MIB + 4096), 2 * MIB + 4096)
        w0 = chunks[1][1]
        got = H.expected(
            SEED, 1, chunks, [(1, 0, 1), (1, w0 + 5, 2), (1, w0 + (2 * MIB) // 8, 4)]
        )
        assert got["bad_pages"] == 3
        assert got["bad_pages_first"] == [(0, 0), (1, 0), (1, 1)]
        assert got["bad_chunks"] == [(0, 1), (1, 2)] and got["flipped_or"] == 7


# ---------------------------------------------------------------------------
# selftest.run on a stub child
# ---------------------------------------------------------------------------
RECORDS = [[7, 134217728 + 9, 0xF1, 0xF0], [7, 300, 0x8000000000000002, 2]]
BAD_PAGES = [[0, 0], [1, 0], [1, 17], [2, 3], [2, 4], [3, 511]]


def hbm_part(bad=False, gib=4):
    part = {
        "ok": not bad,
        "device": 0,
        "seed": 1,
        "seconds": 2.0,
        "alloc_seconds": 0.5,
        "bytes": gib * GIB,
        "chunks": gib,
        "chunk_bytes": [GIB] * gib,
        "free_bytes": 280 * GIB,
        "total_bytes": 288 * GIB,
        "alloc_short": False,
        "rounds": 8 if bad else 40,
        "passes": 8 if bad else 41,
        "mismatches": 0,
        "flipped_or": 0,
        "bad_chunks": [],
        "bad_pages": 0,
        "bad_pages_first": [],
        "records": [],
        "gbs": {"fill": 4000.0, "march_addr": 5000.0, "march_hash": 4900.0, "verify": 4500.0},
    }
    if bad:
        part["mismatches"] = 9
        part["flipped_or"] = 0x8000000000000003
        part["bad_chunks"] = [[0, 1], [1, 2], [2, 5], [3, 1]]
        part["bad_pages"] = 6
        part["bad_pages_first"] = [list(p) for p in BAD_PAGES]
        part["records"] = [list(r) for r in RECORDS]
    return part


def with_hbm(part, base=None):
    rep = base if base is not None else report()
    rep["hbm"] = part
    rep["ok"] = rep["ok"] and part["ok"]
    return rep


BAD_DETAIL = (
    "hbm march: 9 mismatching word(s) in 8 pass(es) over 4.0 GiB; "
    "flipped bits 0x8000000000000003; 6 bad 2 MiB block(s): "
    "chunk 0 block 0, chunk 1 block 0, chunk 1 block 17, chunk 2 block 3, "
    "and 2 more; first recorded word: pass 7 word 300: "
    "got 0x8000000000000002, want 0x0000000000000002"
)


class TestRun:
    def test_flags_appear_only_when_asked_and_the_limit_grows(self):
        spawn = spawn_returning(0, json.dumps(with_hbm(hbm_part())))
        res = selftest.run(Gpu(0), mib=64, timeout_s=30, spawn=spawn, hbm_seconds=2.5)
        assert res.outcome == "pass", res.error
        assert res.findings() == []
        argv, limit = spawn.calls[0]
        assert argv[-3:] == ["--json", "--hbm-seconds", "2.5"]
        assert "--hbm-mib" not in argv
        assert limit == 30 + 2.5 + selftest.HBM_ALLOWANCE_S
        spawn = spawn_returning(0, json.dumps(with_hbm(hbm_part())))
        res = selftest.run(
            Gpu(0), timeout_s=30, spawn=spawn, hbm_seconds=1, hbm_mib=4096
        )
        assert res.outcome == "pass", res.error
        assert spawn.calls[0][0][-5:] == [
            "--json", "--hbm-seconds", "1", "--hbm-mib", "4096",
        ]
        for kw in ({}, {"hbm_seconds": 0}, {"hbm_seconds": 0.0, "hbm_mib": 0}):
            spawn = spawn_returning(0, json.dumps(report()))
            assert selftest.run(Gpu(0), timeout_s=30, spawn=spawn, **kw).outcome == "pass"
            argv, limit = spawn.calls[0]
            assert not any(a.startswith("--hbm") for a in argv) and limit == 30

    def test_the_march_comes_last_and_every_stage_extends_the_limit(self):
        from test_load_selftest import load_part, with_load

        rep = with_hbm(hbm_part(), with_load(load_part()))
        spawn = spawn_returning(0, json.dumps(rep))
        res = selftest.run(
            Gpu(0), timeout_s=30, spawn=spawn, per_cu=False, load_seconds=2, hbm_seconds=3
        )
        assert res.outcome == "pass", res.error
        argv, limit = spawn.calls[0]
        assert argv[-4:] == ["--load-seconds", "2", "--hbm-seconds", "3"]
        assert limit == (
            30 + 2 + selftest.LOAD_GOLDEN_ALLOWANCE_S + 3 + selftest.HBM_ALLOWANCE_S
        )

    def test_the_allowance_is_what_the_profile_derives(self):
        text = open(
            os.path.join(os.path.dirname(build_native.PKG_DIR), "profiles", "hbm_selftest.md")
        ).read()
        assert f"HBM_ALLOWANCE_S = {selftest.HBM_ALLOWANCE_S:g}" in text

    def test_arguments_that_cannot_run_start_no_child(self):
        for kw in (
            dict(hbm_mib=2048),  # no seconds
            dict(hbm_mib=2048, hbm_seconds=0),
            dict(hbm_mib=512, hbm_seconds=1),  # the Infinity Cache
            dict(hbm_mib=-1, hbm_seconds=1),
        ):
            spawn = spawn_returning(0, json.dumps(report()))
            res = selftest.run(Gpu(0), spawn=spawn, **kw)
            assert res.outcome == "error", kw
            assert spawn.calls == []
            (f,) = res.findings()
            assert f.reason == "SelftestError"

    def test_a_bad_part_is_one_memory_finding_with_the_specified_text(self):
        spawn = spawn_returning(1, json.dumps(with_hbm(hbm_part(bad=True))))
        res = selftest.run(Gpu(0), spawn=spawn, hbm_seconds=1)
        assert res.outcome == "memory", res.error
        (f,) = res.findings()
        assert (f.reason, f.severity) == ("SelftestMemoryMismatch", "fatal")
        assert dict(REASONS)[f.reason] == f.severity
        assert f.detail.startswith("hbm march:")
        assert f.detail == BAD_DETAIL
        # types are coerced as the other parts' are
        assert res.report["hbm"]["records"][0] == (7, 134217728 + 9, 0xF1, 0xF0)
        assert res.report["hbm"]["bad_chunks"][2] == (2, 5)

    def test_few_bad_pages_are_all_spelt_out(self):
        part = hbm_part(bad=True)
        part.update(
            mismatches=1, bad_chunks=[[3, 1]], bad_pages=1, bad_pages_first=[[3, 9]],
            records=[[2, 5, 4, 0]], flipped_or=4, passes=3, rounds=3,
        )
        spawn = spawn_returning(1, json.dumps(with_hbm(part)))
        res = selftest.run(Gpu(0), spawn=spawn, hbm_seconds=1)
        assert res.outcome == "memory", res.error
        (f,) = res.findings()
        assert f.detail == (
            "hbm march: 1 mismatching word(s) in 3 pass(es) over 4.0 GiB; "
            "flipped bits 0x0000000000000004; 1 bad 2 MiB block(s): chunk 3 "
            "block 9; first recorded word: pass 2 word 5: "
            "got 0x0000000000000004, want 0x0000000000000000"
        )

    def test_memory_and_march_mismatches_give_both_findings(self):
        rep = with_hbm(hbm_part(bad=True), report(("addr", 1, [(0, 1, 0)])))
        res = selftest.run(Gpu(0), spawn=spawn_returning(1, json.dumps(rep)), hbm_seconds=1)
        assert res.outcome == "memory"
        assert [f.reason for f in res.findings()] == ["SelftestMemoryMismatch"] * 2
        assert res.findings()[1].detail.startswith("hbm march: 9 mismatching")

    def test_a_missing_or_unasked_part_is_an_error(self):
        spawn = spawn_returning(0, json.dumps(report()))
        res = selftest.run(Gpu(0), spawn=spawn, hbm_seconds=1)
        assert res.outcome == "error" and "hbm" in res.error
        spawn = spawn_returning(0, json.dumps(with_hbm(hbm_part())))
        res = selftest.run(Gpu(0), spawn=spawn)
        assert res.outcome == "error" and "hbm" in res.error

    @pytest.mark.parametrize(
        "change",
        [
            dict(ok=False),  # not ok, yet nothing is wrong
            dict(mismatches=3),  # mismatches without records, chunks or pages
            dict(records=[[1, 2, 3, 4]]),
            dict(bad_chunks=[[0, 1]]),
            dict(bad_pages=1),
            dict(bad_pages_first=[[0, 0]]),
            dict(flipped_or=1),
            dict(passes=4),  # a clean run has a whole cycle
            dict(passes=0),
            dict(bytes=GIB - 2 * MIB, chunks=1, chunk_bytes=[GIB - 2 * MIB]),
            dict(bytes=2 * GIB),  # not what the chunks add up to
            dict(chunks=3),
            dict(ok="yes"),
            dict(alloc_short=0),
            dict(mismatches="many"),
            dict(mismatches=-1),
            dict(passes=5.5),
            dict(gbs=None),
            dict(gbs={"fill": "fast"}),
            dict(seconds=None),
        ],
    )
    def test_a_contradictory_or_malformed_clean_part_is_an_error(self, change):
        part = hbm_part()
        part.update(change)
        for rc in (0, 1):
            spawn = spawn_returning(rc, json.dumps(with_hbm(part)))
            res = selftest.run(Gpu(0), spawn=spawn, hbm_seconds=1)
            assert res.outcome == "error", (change, rc)
            assert res.report is None

    @pytest.mark.parametrize(
        "change",
        [
            dict(ok=True),
            dict(mismatches=0),
            dict(records=[]),
            dict(bad_chunks=[]),
            dict(bad_pages=0),
            dict(bad_pages_first=[]),
            dict(flipped_or=0),
            dict(mismatches=10),  # the chunks count 9
            dict(records=[[7, 300, 2]]),
            dict(bad_chunks=[[0, 1, 2], [1, 8]]),
            dict(bad_pages_first=[[0]]),
            dict(passes=1),  # the fill reads nothing
            dict(records="none"),
        ],
    )
    def test_a_contradictory_or_malformed_bad_part_is_an_error(self, change):
        part = hbm_part(bad=True)
        part.update(change)
        for rc in (0, 1):
            spawn = spawn_returning(rc, json.dumps(with_hbm(part)))
            res = selftest.run(Gpu(0), spawn=spawn, hbm_seconds=1)
            assert res.outcome == "error", (change, rc)

    @pytest.mark.parametrize(
        "missing", ["ok", "bytes", "passes", "mismatches", "records", "bad_chunks",
                    "bad_pages", "flipped_or", "gbs", "alloc_short", "chunk_bytes"]
    )
    def test_a_part_without_a_key_is_an_error(self, missing):
        part = hbm_part(bad=True)
        del part[missing]
        rep = with_hbm(hbm_part(bad=True))
        rep["hbm"] = part
        res = selftest.run(Gpu(0), spawn=spawn_returning(1, json.dumps(rep)), hbm_seconds=1)
        assert res.outcome == "error"

    def test_a_part_that_is_no_object_is_an_error(self):
        rep = report()
        rep["hbm"] = [1, 2]
        res = selftest.run(Gpu(0), spawn=spawn_returning(0, json.dumps(rep)), hbm_seconds=1)
        assert res.outcome == "error"

    def test_exit_code_must_agree_with_the_part(self):
        spawn = spawn_returning(0, json.dumps(with_hbm(hbm_part(bad=True))))
        assert selftest.run(Gpu(0), spawn=spawn, hbm_seconds=1).outcome == "error"
        spawn = spawn_returning(1, json.dumps(with_hbm(hbm_part())))
        assert selftest.run(Gpu(0), spawn=spawn, hbm_seconds=1).outcome == "error"

    def test_a_report_without_hbm_has_the_findings_it_had(self):
        rep = report(("hash", 2, [(12, 5, 4)]))
        res = selftest.SelftestResult(0, "b", "memory", rep)
        (f,) = res.findings()
        assert f.detail.startswith("pattern hash: 2 mismatching word(s)")

    def test_child_main_hands_the_flags_on_only_when_given(self, monkeypatch, capsys):
        seen = []

        def child(bdf, mib, per_cu=False, **kw):
            seen.append((bdf, mib, per_cu, kw))
            rep = report()
            if "hbm_seconds" in kw:
                rep = with_hbm(hbm_part())
            return 0, rep

        monkeypatch.setattr(selftest, "_child", child)
        argv = ["--bdf", "0000:c1:00.0"]
        assert selftest.main(argv) == 0
        assert selftest.main(argv + ["--hbm-seconds", "3"]) == 0
        assert selftest.main(argv + ["--hbm-seconds", "3", "--hbm-mib", "2048"]) == 0
        assert [s[3] for s in seen] == [
            {},
            {"hbm_seconds": 3.0},
            {"hbm_seconds": 3.0, "hbm_mib": 2048},
        ]
        out = capsys.readouterr().out
        assert (
            "hbm march: 41 pass(es) over 4.0 GiB in 4 chunk(s) in 2.0s, "
            "0 mismatch(es) in 0 2 MiB block(s); fill 4000, march 5000 / 4900, "
            "verify 4500 GB/s (informative)" in out
        )
        for bad in (
            argv + ["--hbm-mib", "2048"],  # no --hbm-seconds
            argv + ["--hbm-seconds", "0", "--hbm-mib", "2048"],
            argv + ["--hbm-seconds", "-1"],
            argv + ["--hbm-seconds", "601"],
            argv + ["--hbm-seconds", "1", "--hbm-mib", "512"],
        ):
            with pytest.raises(SystemExit):
                selftest.main(bad)
        assert len(seen) == 3
        capsys.readouterr()

    def test_the_child_runs_the_march_after_every_other_stage(self, monkeypatch):
        from test_load_selftest import load_part

        order = []

        def selftest_stub(ordinal, mib):
            order.append("base")
            return report()

        def load_stub(ordinal, seconds):
            order.append(("load", seconds))
            return load_part()

        def hbm_stub(ordinal, seconds, mib):
            order.append(("hbm", seconds, mib))
            return hbm_part(bad=mib == 2048)

        fake = types.SimpleNamespace(
            device_count=lambda: 1,
            pci_bus_id=lambda o: "0000:C1:00.0",
            selftest=selftest_stub,
            load_selftest=load_stub,
            hbm_selftest=hbm_stub,
        )
        monkeypatch.setattr(k8s_dra_driver_amd, "_hiphealth", fake, raising=False)
        rc, rep = selftest._child("0000:c1:00.0", 64, False, 2.0, hbm_seconds=1.5)
        assert order == ["base", ("load", 2.0), ("hbm", 1.5, 0)]
        assert rc == selftest.EXIT_PASS and rep["hbm"]["ok"] and rep["ok"]
        rc, rep = selftest._child("0000:c1:00.0", 64, hbm_seconds=1.5, hbm_mib=2048)
        assert order[-2:] == ["base", ("hbm", 1.5, 2048)]
        assert rc == selftest.EXIT_MISMATCH and rep["ok"] is False
        rc, rep = selftest._child("0000:c1:00.0", 64)
        assert rc == selftest.EXIT_PASS and "hbm" not in rep


# ---------------------------------------------------------------------------
# driver
# ---------------------------------------------------------------------------
def hbm_runner(outcomes):
    """runner(gpu, mib=, timeout_s=, hbm_seconds=, hbm_mib=) with an ``hbm``
    part that is the bad one of a memory outcome."""
    calls = []

    def runner(gpu, *, mib, timeout_s, hbm_seconds=0, **kw):
        calls.append((gpu.index, hbm_seconds, kw))
        outcome = outcomes.get(gpu.index, "pass")
        rep = with_hbm(hbm_part(bad=outcome == "memory"))
        selftest._classify(rep)  # as run() leaves it
        return selftest.SelftestResult(
            gpu.index, gpu.pcie_bdf, outcome, rep, "", seconds=0.25
        )

    runner.calls = calls
    return runner


HBM_GAUGES = (
    "dra_gpu_selftest_hbm_bytes",
    "dra_gpu_selftest_hbm_passes",
    "dra_gpu_selftest_hbm_mismatches",
)


class TestDriver:
    def test_the_arguments_reach_the_runner_and_set_the_gauges(self, tmp_path):
        d, _, _ = make_driver(tmp_path, gpu_indices=[0, 1])
        try:
            runner = hbm_runner({1: "memory"})
            results = d.run_startup_selftest(runner, mib=64, hbm_seconds=2)
            assert results == {0: "pass", 1: "memory"}
            assert runner.calls == [(0, 2, {}), (1, 2, {})]  # no hbm_mib
            m = d.metrics
            assert sample(m, HBM_GAUGES[0], gpu="0") == 4 * GIB
            assert sample(m, HBM_GAUGES[1], gpu="0") == 41
            assert sample(m, HBM_GAUGES[2], gpu="0") == 0
            assert sample(m, HBM_GAUGES[1], gpu="1") == 8
            assert sample(m, HBM_GAUGES[2], gpu="1") == 9
            assert d.health.findings(0) == []
            (f,) = d.health.findings(1)
            assert f.reason == "SelftestMemoryMismatch"
            assert f.detail.startswith("hbm march: 9 mismatching word(s)")
            runner = hbm_runner({})
            d.run_startup_selftest(runner, mib=64, hbm_seconds=2, hbm_mib=4096)
            assert runner.calls == [(0, 2, {"hbm_mib": 4096}), (1, 2, {"hbm_mib": 4096})]
        finally:
            d.shutdown(unpublish=False)

    def test_without_the_march_an_old_signature_runner_is_called_as_before(self, tmp_path):
        d, _, _ = make_driver(tmp_path, gpu_indices=[0])
        try:
            runner = stub_runner({})  # would reject hbm_seconds
            assert d.run_startup_selftest(runner, mib=64) == {0: "pass"}
            assert d.run_startup_selftest(runner, mib=64, hbm_seconds=0) == {0: "pass"}
            # a coverage without seconds asks for nothing
            assert d.run_startup_selftest(runner, mib=64, hbm_mib=4096) == {0: "pass"}
            for name in HBM_GAUGES:
                assert sample(d.metrics, name, gpu="0") is None
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
    def test_plugin_flags_default_to_off(self, monkeypatch):
        monkeypatch.delenv("SELFTEST_HBM_SECONDS", raising=False)
        monkeypatch.delenv("SELFTEST_HBM_MIB", raising=False)
        args = plugin_main.build_parser().parse_args(["--startup-selftest", "on"])
        assert args.selftest_hbm_seconds == 0 and args.selftest_hbm_mib == 0
        drv = FakeDriver()
        assert plugin_main.startup_selftest(args, drv) is True
        assert drv.calls == [{"mib": 1024, "timeout_s": 120.0}]

    def test_plugin_flags_and_their_environment_mirror(self, monkeypatch):
        parse = plugin_main.build_parser().parse_args
        drv = FakeDriver()
        plugin_main.startup_selftest(
            parse(["--startup-selftest", "on", "--selftest-hbm-seconds", "20"]), drv
        )
        plugin_main.startup_selftest(
            parse(["--startup-selftest", "on", "--selftest-hbm-seconds", "20",
                   "--selftest-hbm-mib", "8192"]),
            drv,
        )
        assert drv.calls == [
            {"mib": 1024, "timeout_s": 120.0, "hbm_seconds": 20.0},
            {"mib": 1024, "timeout_s": 120.0, "hbm_seconds": 20.0, "hbm_mib": 8192},
        ]
        monkeypatch.setenv("SELFTEST_HBM_SECONDS", "7.5")
        monkeypatch.setenv("SELFTEST_HBM_MIB", "2048")
        args = plugin_main.build_parser().parse_args([])
        assert plugin_main.selftest_hbm(args) == {"hbm_seconds": 7.5, "hbm_mib": 2048}

    def test_plugin_rejects_what_it_cannot_run(self):
        parse = plugin_main.build_parser().parse_args
        for argv in (
            ["--selftest-hbm-seconds", "-1"],
            ["--selftest-hbm-seconds", str(selftest.MAX_LOAD_SECONDS + 1)],
            ["--selftest-hbm-mib", "2048"],  # no seconds
            ["--selftest-hbm-seconds", "5", "--selftest-hbm-mib", "512"],
            ["--selftest-hbm-seconds", "5", "--selftest-hbm-mib", "-4"],
        ):
            with pytest.raises(ValueError):
                plugin_main.selftest_hbm(parse(argv))
        assert plugin_main.selftest_hbm(
            parse(["--selftest-hbm-seconds", str(selftest.MAX_LOAD_SECONDS)])
        ) == {"hbm_seconds": selftest.MAX_LOAD_SECONDS}

    def test_ctl_passes_the_flags_and_prints_the_figures(self, monkeypatch, capsys):
        runner = hbm_runner({4: "memory"})
        monkeypatch.setattr(
            selftest, "run", lambda gpu, **kw: runner(gpu, timeout_s=0, **kw)
        )
        argv = ["--hal", "fake", "health", "--selftest", "--hbm-seconds", "2"]
        assert ctl.main(argv + ["--hbm-mib", "4096", "--json"]) == 1
        records = json.loads(capsys.readouterr().out)
        assert all(c == (i, 2.0, {"hbm_mib": 4096}) for i, c in enumerate(runner.calls))
        assert records[0]["selftest"]["hbm"] == {
            "bytes": 4 * GIB,
            "chunks": 4,
            "alloc_short": False,
            "passes": 41,
            "mismatches": 0,
            "flipped_or": 0,
            "bad_chunks": [],
            "bad_pages": 0,
            "gbs": hbm_part()["gbs"],
        }
        assert records[4]["selftest"]["result"] == "memory"
        assert records[4]["selftest"]["hbm"]["mismatches"] == 9
        assert records[4]["selftest"]["hbm"]["bad_chunks"] == [[0, 1], [1, 2], [2, 5], [3, 1]]
        del runner.calls[:]
        assert ctl.main(argv) == 1
        assert all(c == (i, 2.0, {}) for i, c in enumerate(runner.calls))
        out = capsys.readouterr().out
        assert (
            "hbm march: 41 pass(es) over 4.0 GiB in 4 chunk(s), 0 mismatch(es) "
            "in 0 2 MiB block(s), march 4900 GB/s (informative)" in out
        )
        assert "hbm march: 8 pass(es) over 4.0 GiB in 4 chunk(s), 9 mismatch(es)" in out
        assert "SelftestMemoryMismatch: hbm march: 9 mismatching word(s)" in out

    def test_ctl_without_the_flag_calls_run_as_before(self, monkeypatch, capsys):
        runner = stub_runner({})  # would reject hbm_seconds
        monkeypatch.setattr(
            selftest, "run", lambda gpu, **kw: runner(gpu, timeout_s=0, **kw)
        )
        assert ctl.main(["--hal", "fake", "health", "--selftest", "--json"]) == 0
        records = json.loads(capsys.readouterr().out)
        assert "hbm" not in records[0]["selftest"]

    def test_ctl_rejects_what_it_cannot_run(self, capsys):
        for argv in (
            ["health", "--hbm-seconds", "2"],  # no --selftest
            ["health", "--selftest", "--hbm-mib", "2048"],
            ["health", "--selftest", "--hbm-seconds", "-2"],
            ["health", "--selftest", "--hbm-seconds", "601"],
            ["health", "--selftest", "--hbm-seconds", "2", "--hbm-mib", "100"],
        ):
            with pytest.raises(SystemExit):
                ctl.main(["--hal", "fake"] + argv)
        capsys.readouterr()

    @pytest.mark.parametrize("bad", [False, True])
    def test_workload_flag_runs_it_and_exits_1_on_a_mismatch(
        self, monkeypatch, capsys, bad
    ):
        calls = []

        def hbm_selftest(device, seconds):
            calls.append((device, seconds))
            return hbm_part(bad=bad)

        fake = types.SimpleNamespace(device_count=lambda: 2, hbm_selftest=hbm_selftest)
        monkeypatch.setattr(k8s_dra_driver_amd, "_hiphealth", fake, raising=False)
        monkeypatch.setattr(
            workload,
            "visible_devices",
            lambda: {"kfd": True, "render_nodes": ["renderD128"]},
        )
        assert workload.main(["--hbm-selftest", "1.5"]) == (1 if bad else 0)
        assert calls == [(0, 1.5), (1, 1.5)]
        out = capsys.readouterr().out
        if bad:
            assert "device 1: hbm-selftest FAILED: 8 pass(es) over 4.0 GiB" in out
            assert "9 mismatch(es), flipped bits 0x8000000000000003" in out
            assert "6 bad 2 MiB block(s): chunk 0 block 0, chunk 1 block 0" in out
        else:
            assert (
                "device 0: hbm-selftest ok: 41 pass(es) over 4.0 GiB in 4 chunk(s) "
                "in 2.0s, 0 mismatch(es)" in out
            )

    def test_workload_rejects_a_bad_time(self, capsys):
        for argv in (["-1"], ["soon"], ["601"]):
            with pytest.raises(SystemExit):
                workload.main(["--hbm-selftest"] + argv)
        capsys.readouterr()


# ---------------------------------------------------------------------------
# hbmtest_core.hpp under AddressSanitizer and UBSan, as its own program
# ---------------------------------------------------------------------------
def test_core_selftest_program_builds_and_passes(tmp_path):
    if build_native.sanitizer_link_flags() is None:
        pytest.skip("gcc has no ASan/UBSan runtime installed")
    exe = build_native.build_hbmtest_core_selftest(str(tmp_path / "hbm_core_selftest"))
    done = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert done.returncode == 0, done.stdout + done.stderr[-3000:]
    assert "hbmtest_core_selftest: ok" in done.stdout
    assert done.stderr == ""


def test_the_headers_are_part_of_the_extension_build(monkeypatch):
    src = open(os.path.join(build_native.CPP_DIR, "hiphealth.hip")).read()
    assert src.index('"selftest_kernels.hpp"') < src.index('"hbmtest_kernels.hpp"')
    kern = open(os.path.join(build_native.CPP_DIR, "hbmtest_kernels.hpp")).read()
    core = open(os.path.join(build_native.CPP_DIR, "hbmtest_core.hpp")).read()
    assert '#include "hbmtest_core.hpp"' in kern
    for banned in ("hip/hip_runtime.h", "pybind11", "__device__"):
        assert banned not in core
    # a change to either header rebuilds the extension
    asked = []
    monkeypatch.setattr(
        build_native, "_needs_build", lambda src, out: asked.append(src) or False
    )
    build_native.build_hiphealth()
    names = [os.path.basename(p) for p in asked]
    assert "hbmtest_kernels.hpp" in names and "hbmtest_core.hpp" in names
    assert "mxtest_kernels.hpp" in names and "hiphealth.hip" in names


def test_the_reference_has_the_constants_of_the_core():
    core = open(os.path.join(build_native.CPP_DIR, "hbmtest_core.hpp")).read()
    for text in (
        "kHbChunkBytes = 1ull << 30",
        "kHbPageBytes = 2ull << 20",
        "kHbMinBytes = 1ull << 30",
        "kHbReserveMinBytes = 2ull << 30",
        "kHbReservePercent = 2",
        "kHbMaxRecords = 64",
        "kHbPagesFirst = 8",
    ):
        assert text in core
    assert (H.CHUNK_BYTES, H.PAGE_BYTES, H.MIN_BYTES) == (GIB, 2 * MIB, GIB)
    assert (H.RESERVE_MIN_BYTES, H.RESERVE_PERCENT) == (2 * GIB, 2)
    assert (H.MAX_RECORDS, H.PAGES_FIRST) == (64, 8)
    assert selftest.HBM_MIN_BYTES == H.MIN_BYTES
