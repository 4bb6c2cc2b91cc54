"""amd-dra-ctl health --signals / --json on the fake HAL."""

import json

from k8s_dra_driver_amd import ctl
from k8s_dra_driver_amd.hal import FakeDeviceLib
from k8s_dra_driver_amd.hal.model import HEALTH_SIGNAL_NAMES


def test_json_one_record_per_gpu(capsys):
    assert ctl.main(["--hal", "fake", "health", "--json"]) == 0
    records = json.loads(capsys.readouterr().out)
    assert [r["name"] for r in records] == [f"gpu-{i}" for i in range(8)]
    for r in records:
        assert r["health"]["status"] == "healthy"
        assert r["findings"] == []
        # every signal once: a value or an unsupported entry
        assert set(r["signals"]) | set(r["unsupported"]) == set(
            HEALTH_SIGNAL_NAMES
        )
        assert not set(r["signals"]) & set(r["unsupported"])


def test_plain_output_keeps_the_per_gpu_line(capsys):
    assert ctl.main(["--hal", "fake", "health"]) == 0
    lines = capsys.readouterr().out.splitlines()
    assert len(lines) == 8
    assert lines[0].startswith("gpu-0: {'status': 'healthy'")


def test_signals_dump_is_readable(capsys):
    assert ctl.main(["--hal", "fake", "health", "--signals"]) == 0
    out = capsys.readouterr().out
    assert "gpu-0: {'status': 'healthy'" in out
    assert "ecc_uncorrectable: 0" in out
    assert "temp_hotspot_c: 45.0" in out
    assert "findings: none" in out


def _sick_lib(monkeypatch, **fields):
    lib = FakeDeviceLib()
    lib.set_health_signals(3, **fields)
    monkeypatch.setattr(ctl, "new_device_lib", lambda hal: lib)
    return lib


def test_pending_page_exits_1(monkeypatch, capsys):
    _sick_lib(monkeypatch, bad_pages_pending=1)
    assert ctl.main(["--hal", "fake", "health", "--json"]) == 1
    records = json.loads(capsys.readouterr().out)
    assert len(records) == 8
    sick = records[3]
    assert sick["signals"]["bad_pages_pending"] == 1
    assert [(f["reason"], f["severity"]) for f in sick["findings"]] == [
        ("BadPagesPending", "fatal")
    ]
    assert all(r["findings"] == [] for r in records if r["index"] != 3)
    # the same without --json, and the dump names the finding
    assert ctl.main(["--hal", "fake", "health", "--signals"]) == 1
    assert "finding [fatal] BadPagesPending" in capsys.readouterr().out


def test_soft_finding_exits_1_warning_does_not(monkeypatch, capsys):
    lib = _sick_lib(monkeypatch, temp_hotspot_c=115.0)
    assert ctl.main(["--hal", "fake", "health"]) == 1
    lib.set_health_signals(3, reset=True, bad_pages_reserved=1, temp_vram_c=None)
    assert ctl.main(["--hal", "fake", "health", "--signals"]) == 0
    out = capsys.readouterr().out
    assert "finding [warning] RetiredPages" in out
    assert "unsupported temp_vram_c" in out
