"""CU footprint, the part that needs no GPU: the decode of the hardware id
words, the HSA_CU_MASK parser, the parent half of ``measure`` with an
injected child, the Footprint arithmetic and the workload's verdict."""

import json
import os
import subprocess

import pytest

from k8s_dra_driver_amd import workload
from k8s_dra_driver_amd.api.types import SharedComputeSettings
from k8s_dra_driver_amd.hal.model import AllocatableDevice
from k8s_dra_driver_amd.sharing import footprint as F
from k8s_dra_driver_amd.sharing.shared import SharedComputeManager, cu_mask_hex

ALL = 0xFFFFFFFF
# HW_ID fields (hip/amd_detail/amd_device_functions.h, GCN and CDNA)
CU_BITS = 0xF << 8
SH_BIT = 1 << 12
SE_BITS = 0x3 << 13
KEY_BITS = CU_BITS | SH_BIT | SE_BITS


# ---------------------------------------------------------------------------
# decode
# ---------------------------------------------------------------------------
class TestDecode:
    def test_zero(self):
        assert F.decode(0, 0) == (0, 0, 0, 0)

    @pytest.mark.parametrize(
        "hw_id, xcc_id, want",
        [
            # one field at its maximum, every bit outside the key set
            ((ALL & ~KEY_BITS) | CU_BITS, ALL & ~0xF, (0, 0, 0, 15)),
            ((ALL & ~KEY_BITS) | SH_BIT, ALL & ~0xF, (0, 0, 1, 0)),
            ((ALL & ~KEY_BITS) | SE_BITS, ALL & ~0xF, (0, 3, 0, 0)),
            (ALL & ~KEY_BITS, ALL, (15, 0, 0, 0)),
            # and all of them
            (ALL, ALL, (15, 3, 1, 15)),
        ],
    )
    def test_each_field_at_its_maximum_amid_garbage(self, hw_id, xcc_id, want):
        assert F.decode(hw_id, xcc_id) == want

    def test_fields_are_read_where_they_are(self):
        assert F.decode(0x5 << 8, 0) == (0, 0, 0, 5)
        assert F.decode(0x2 << 13, 0) == (0, 2, 0, 0)
        assert F.decode((0x1 << 13) | SH_BIT | (0x9 << 8), 7) == (7, 1, 1, 9)

    @pytest.mark.parametrize(
        "noise",
        [
            0xF,  # WAVE_ID 3:0
            0x3 << 4,  # SIMD_ID 5:4
            0x3 << 6,  # PIPE_ID 7:6
            1 << 15,  # third SE bit of gfx908/gfx90a: not SE on four-SE parts
            0xF << 16,  # TG_ID
            0xF << 20,  # VM_ID
            0x7 << 24,  # QUEUE_ID
            0x7 << 27,  # STATE_ID
            0x3 << 30,  # ME_ID
        ],
    )
    def test_wave_bits_do_not_leak_into_the_key(self, noise):
        base = (0x2 << 13) | SH_BIT | (0xA << 8)
        assert F.decode(base | noise, 3) == F.decode(base, 3) == (3, 2, 1, 10)

    def test_two_waves_of_one_cu_give_one_key(self):
        base = (0x1 << 13) | (0x4 << 8)
        keys = {F.decode(base | simd << 4 | wave, 5) for simd in range(4) for wave in range(10)}
        assert keys == {(5, 1, 0, 4)}


# ---------------------------------------------------------------------------
# parse_cu_mask
# ---------------------------------------------------------------------------
def _gpu_devices(lib, *indices):
    gpus = lib.enumerate()
    return [AllocatableDevice.from_gpu(gpus[i]) for i in indices]


def _mask_env(session):
    (entry,) = [e for e in session.env if e.startswith("HSA_CU_MASK=")]
    return entry.split("=", 1)[1]


class TestParseCuMask:
    def test_what_the_supervisor_emits_for_one_gpu(self, tmp_path, fake_lib):
        mgr = SharedComputeManager(root=str(tmp_path / "s"), use_tmpfs=False)
        settings = SharedComputeSettings(default_cu_share_percent=25)
        devs = _gpu_devices(fake_lib, 0)
        assert devs[0].parent_gpu.cu_count == 256
        a = _mask_env(mgr.start_session("claim-a", devs, settings))
        b = _mask_env(mgr.start_session("claim-b", devs, settings))
        assert a == "0:" + cu_mask_hex(0, 64)
        assert b == "0:" + cu_mask_hex(64, 64)
        assert F.parse_cu_mask(a) == {0: (1 << 64) - 1}
        assert F.parse_cu_mask(b) == {0: ((1 << 64) - 1) << 64}

    def test_what_the_supervisor_emits_for_two_gpus(self, tmp_path, fake_lib):
        mgr = SharedComputeManager(root=str(tmp_path / "s"), use_tmpfs=False)
        settings = SharedComputeSettings(default_cu_share_percent=25)
        mgr.start_session("first", _gpu_devices(fake_lib, 1), settings)
        value = _mask_env(
            mgr.start_session("second", _gpu_devices(fake_lib, 0, 1), settings)
        )
        assert value == f"0:{cu_mask_hex(0, 64)};1:{cu_mask_hex(64, 64)}"
        masks = F.parse_cu_mask(value)
        assert masks == {0: (1 << 64) - 1, 1: ((1 << 64) - 1) << 64}
        assert [F.popcount(m) for m in masks.values()] == [64, 64]

    def test_the_three_syntaxes_agree(self):
        quarter = {0: (1 << 64) - 1}
        assert F.parse_cu_mask("0:0-63") == F.parse_cu_mask("0:" + cu_mask_hex(0, 64))
        assert F.parse_cu_mask("0:0-63") == quarter
        assert F.parse_cu_mask("0:0-63;1:0-63") == {0: quarter[0], 1: quarter[0]}
        assert F.parse_cu_mask("0:64-127") == F.parse_cu_mask("0:" + cu_mask_hex(64, 64))

    def test_decimal_lists(self):
        want = ((1 << 32) - 1) | (((1 << 32) - 1) << 64)
        assert F.parse_cu_mask("0:0-31,64-95") == {0: want}
        assert F.parse_cu_mask("2:5") == {2: 1 << 5}
        assert F.parse_cu_mask("0:1,3,5-6") == {0: 0b1101010}
        assert F.parse_cu_mask("0:3,3,2-4") == {0: 0b11100}
        assert F.parse_cu_mask(" 0 : 0-3 ; 1 : 0xF0 ") == {0: 0xF, 1: 0xF0}
        assert F.parse_cu_mask("0-1:0-3") == {0: 0xF, 1: 0xF}
        assert F.parse_cu_mask("0,2:0X3") == {0: 3, 2: 3}

    def test_popcounts(self):
        assert F.popcount(0) == 0
        assert F.popcount(F.parse_cu_mask("0:0-63")[0]) == 64
        assert F.popcount(F.parse_cu_mask("0:0-31,64-95")[0]) == 64
        assert F.popcount(F.parse_cu_mask("0:" + cu_mask_hex(0, 256))[0]) == 256
        assert F.popcount(F.parse_cu_mask("0:0x8000000000000001")[0]) == 2

    @pytest.mark.parametrize(
        "bad",
        [
            "",
            "   ",
            "0x" + "f" * 16,  # no GPU index
            ":0xff",
            "0:",
            "0:0x",
            "0:0xfg",
            "0:ff",  # hex digits without 0x
            "0:-1",
            "0:5-",
            "0:-5",
            "0:63-0",
            "0:1,,2",
            "0:1;",
            ";0:1",
            "a:0xff",
            "-1:0xff",
            "0:0x0",
            "0:0xff:1",
            "0:0xff;0:0xff00",  # one GPU twice
            "0=0xff",
            "0:1 2",
            None,
            0xFF,
        ],
    )
    def test_malformed_raises(self, bad):
        with pytest.raises(ValueError):
            F.parse_cu_mask(bad)


# ---------------------------------------------------------------------------
# Footprint
# ---------------------------------------------------------------------------
def _fp(cus, device=0):
    return F.Footprint(device=device, cus=frozenset(cus))


class TestFootprint:
    def test_overlap(self):
        a = _fp({(0, 0, 0, 0), (0, 0, 0, 1), (1, 2, 1, 7)})
        b = _fp({(1, 2, 1, 7), (1, 2, 0, 7), (0, 0, 0, 2)})
        assert a.overlap(b) == b.overlap(a) == {(1, 2, 1, 7)}
        assert a.overlap(_fp(set())) == set()
        assert not a.overlap(_fp({(2, 0, 0, 0)}))
        assert a.count == 3 and a.ok

    def test_exceeds_counts_bits(self):
        three = _fp({(0, 0, 0, 0), (0, 0, 0, 1), (0, 0, 0, 2)})
        assert not three.exceeds(0b111)
        assert not three.exceeds(0b1111)
        assert three.exceeds(0b11)
        assert three.exceeds(1 << 200)  # which bits does not matter, how many does
        assert not three.exceeds(None)

    def test_exceeds_reads_its_own_device_from_a_mask_string(self):
        three = _fp({(0, 0, 0, 0), (0, 0, 0, 1), (0, 0, 0, 2)}, device=1)
        assert three.exceeds("0:0xff;1:0x3")
        assert not three.exceeds("0:0x1;1:0x7")
        assert not three.exceeds("0:0x1")  # no entry for device 1: unmasked
        with pytest.raises(ValueError):
            three.exceeds("nonsense")


# ---------------------------------------------------------------------------
# measure, with the child injected
# ---------------------------------------------------------------------------
def _report(cus, cu_mask, **over):
    per_xcc = {}
    for cu in cus:
        per_xcc[str(cu[0])] = per_xcc.get(str(cu[0]), 0) + 1
    r = {
        "cus": [list(c) for c in sorted(cus)],
        "count": len(cus),
        "per_xcc": per_xcc,
        "blocks_per_cu_min": 7,
        "blocks_per_cu_max": 9,
        "blocks": 2048,
        "spin": 4096,
        "multi_processor_count": 256,
        "kernel_ms": 0.5,
        "device": 0,
        "cu_mask": cu_mask,
    }
    r.update(over)
    return r


class _Spawn:
    def __init__(self, rc=0, out="", err="", raises=None):
        self.rc, self.out, self.err, self.raises = rc, out, err, raises
        self.calls = []

    def __call__(self, argv, env, timeout_s):
        self.calls.append((list(argv), dict(env), timeout_s))
        if self.raises:
            raise self.raises
        return self.rc, self.out, self.err


CUS = {(0, 0, 0, 0), (0, 1, 0, 3), (5, 3, 1, 15)}


class TestMeasure:
    def test_the_mask_reaches_the_child_and_nowhere_else(self, monkeypatch):
        monkeypatch.delenv("HSA_CU_MASK", raising=False)
        before = dict(os.environ)
        spawn = _Spawn(out="noise\n" + json.dumps(_report(CUS, "0:0-63")) + "\n")
        fp = F.measure(0, cu_mask="0:0-63", timeout_s=5, spawn=spawn)
        assert fp.ok, fp.error
        ((argv, env, timeout_s),) = spawn.calls
        assert env["HSA_CU_MASK"] == "0:0-63"
        assert "HSA_CU_MASK" not in os.environ
        assert dict(os.environ) == before
        assert timeout_s == 5
        assert argv[1:] == [
            "-m",
            "k8s_dra_driver_amd.sharing.footprint",
            "--device",
            "0",
            "--json",
        ]
        assert fp.cus == CUS and fp.count == 3
        assert fp.per_xcc == {0: 2, 5: 1}
        assert fp.cu_mask == "0:0-63" and fp.device == 0
        assert fp.multi_processor_count == 256 and fp.blocks == 2048
        assert not fp.exceeds("0:0-63") and fp.exceeds("0:0-1")

    def test_no_mask_removes_an_inherited_one_from_the_child_only(self, monkeypatch):
        monkeypatch.setenv("HSA_CU_MASK", "0:0-127")
        spawn = _Spawn(out=json.dumps(_report(CUS, None)))
        fp = F.measure(1, spawn=spawn)
        assert fp.ok, fp.error
        ((argv, env, _),) = spawn.calls
        assert "HSA_CU_MASK" not in env
        assert os.environ["HSA_CU_MASK"] == "0:0-127"
        assert argv[argv.index("--device") + 1] == "1"
        assert fp.cu_mask is None and fp.device == 1

    def test_the_child_finds_the_package(self):
        spawn = _Spawn(out=json.dumps(_report(CUS, None)))
        F.measure(0, spawn=spawn)
        ((_, env, _),) = spawn.calls
        root = os.path.dirname(os.path.dirname(os.path.abspath(workload.__file__)))
        assert env["PYTHONPATH"].split(os.pathsep)[0] == root

    def test_a_timeout_is_an_error_result(self):
        spawn = _Spawn(raises=subprocess.TimeoutExpired(["python"], 3))
        fp = F.measure(0, cu_mask="0:0-63", timeout_s=3, spawn=spawn)
        assert not fp.ok and "timed out after 3s" in fp.error
        assert fp.cus == frozenset() and fp.count == 0
        assert len(spawn.calls) == 1  # never a retry

    def test_a_child_that_cannot_start_is_an_error_result(self):
        fp = F.measure(0, spawn=_Spawn(raises=OSError("no python")))
        assert not fp.ok and "no python" in fp.error

    def test_a_non_json_line_is_an_error_result(self):
        spawn = _Spawn(out="Segmentation fault\n", err="boom\n", rc=0)
        fp = F.measure(0, spawn=spawn)
        assert not fp.ok and "unparsable output" in fp.error and "boom" in fp.error
        fp = F.measure(0, spawn=_Spawn(out="", rc=0))
        assert not fp.ok and "unparsable output" in fp.error
        fp = F.measure(0, spawn=_Spawn(out="[1, 2]", rc=0))
        assert not fp.ok and "unparsable output" in fp.error

    def test_a_non_zero_exit_is_an_error_result(self):
        spawn = _Spawn(rc=2, out=json.dumps({"error": "RuntimeError: no device"}))
        fp = F.measure(0, spawn=spawn)
        assert not fp.ok and "exit 2" in fp.error and "no device" in fp.error
        # also when the report itself looks fine
        fp = F.measure(0, spawn=_Spawn(rc=1, out=json.dumps(_report(CUS, None))))
        assert not fp.ok and "exit 1" in fp.error
        fp = F.measure(0, spawn=_Spawn(rc=-11, out=""))
        assert not fp.ok and "exit -11" in fp.error

    def test_a_report_under_another_mask_is_an_error_result(self):
        spawn = _Spawn(out=json.dumps(_report(CUS, None)))
        fp = F.measure(0, cu_mask="0:0-63", spawn=spawn)
        assert not fp.ok and "ran under" in fp.error

    @pytest.mark.parametrize(
        "over",
        [
            {"count": 4},
            {"per_xcc": {"0": 3}},
            {"cus": [[0, 0, 0]]},
            {"cus": [[0, 0, 0, 0], [0, 0, 0, 0]], "count": 2},
            {"cus": "nope"},
            {"blocks": None},
        ],
    )
    def test_a_malformed_report_is_an_error_result(self, over):
        report = _report(CUS, None)
        report.update(over)
        fp = F.measure(0, spawn=_Spawn(out=json.dumps(report)))
        assert not fp.ok and "malformed report" in fp.error
        missing = _report(CUS, None)
        del missing["multi_processor_count"]
        fp = F.measure(0, spawn=_Spawn(out=json.dumps(missing)))
        assert not fp.ok and "malformed report" in fp.error

    def test_a_malformed_mask_never_starts_a_child(self):
        spawn = _Spawn(out=json.dumps(_report(CUS, "0:zz")))
        fp = F.measure(0, cu_mask="0:zz", spawn=spawn)
        assert not fp.ok and spawn.calls == []


# ---------------------------------------------------------------------------
# amd-dra-workload --cu-footprint
# ---------------------------------------------------------------------------
class _FakeHip:
    def __init__(self, counts):
        self.counts = counts

    def device_count(self):
        return len(self.counts)

    def cu_footprint(self, device):
        n = self.counts[device]
        return {"count": n, "per_xcc": {0: n}, "multi_processor_count": 256}


class TestWorkloadVerdict:
    def test_within_mask(self):
        rows = workload.cu_footprint_rows({0: 64}, "0:" + cu_mask_hex(0, 64))
        assert rows == [(0, 64, 64)]
        assert workload.cu_footprint_exit_code(rows) == 0
        assert workload.cu_footprint_exit_code([(0, 48, 64)]) == 0

    def test_exceeds_mask(self):
        rows = workload.cu_footprint_rows({0: 70}, "0:0-63")
        assert rows == [(0, 70, 64)]
        assert workload.cu_footprint_exit_code(rows) == 1
        # one device over is enough
        rows = workload.cu_footprint_rows({0: 64, 1: 65}, "0:0-63;1:0-63")
        assert workload.cu_footprint_exit_code(rows) == 1

    def test_no_mask(self):
        rows = workload.cu_footprint_rows({0: 256, 1: 256}, "")
        assert rows == [(0, 256, None), (1, 256, None)]
        assert workload.cu_footprint_exit_code(rows) == 0
        # a mask that names another device leaves this one unmasked
        rows = workload.cu_footprint_rows({0: 256}, "1:0-63")
        assert rows == [(0, 256, None)]
        assert workload.cu_footprint_exit_code(rows) == 0

    @pytest.mark.parametrize(
        "counts, mask, rc, said",
        [
            ([64], "0:0-63", 0, "mask allows 64: ok"),
            ([70], "0:0-63", 1, "mask allows 64: EXCEEDS MASK"),
            ([256, 256], None, 0, "no mask: ok"),
            ([64], "0:zz", 1, ""),
            ([], None, 1, ""),
        ],
    )
    def test_the_printed_report(self, monkeypatch, capsys, counts, mask, rc, said):
        if mask is None:
            monkeypatch.delenv("HSA_CU_MASK", raising=False)
        else:
            monkeypatch.setenv("HSA_CU_MASK", mask)
        assert workload.run_cu_footprint(_FakeHip(counts)) == rc
        out = capsys.readouterr().out
        assert said in out
        if said:
            assert out.count("device ") == len(counts)
            assert f"cu footprint {counts[0]} of 256 CUs, per XCD 0:{counts[0]}" in out
