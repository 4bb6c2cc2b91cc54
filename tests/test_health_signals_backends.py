"""health_signals() of the amdsmi backend (stub native ext) and of the
KFD/sysfs backend (a sysfs tree the test writes itself)."""

import os

import pytest

from k8s_dra_driver_amd.hal.amdsmi import AmdSmiDeviceLib
from k8s_dra_driver_amd.hal.kfd import KfdDeviceLib
from k8s_dra_driver_amd.hal.model import (
    BAD_PAGE_SIGNALS,
    ECC_SIGNALS,
    HEALTH_SIGNAL_NAMES,
    THROTTLE_SIGNALS,
)
from k8s_dra_driver_amd.plugin.health import evaluate


def reported_once(sig):
    """Every signal is a value or listed as unsupported — never both,
    never neither."""
    for name in HEALTH_SIGNAL_NAMES:
        has_value = getattr(sig, name) is not None
        assert has_value != (name in sig.unsupported), name
    return True


# ---------------------------------------------------------------------------
# amdsmi backend over a stub ext
# ---------------------------------------------------------------------------
class StubExt:
    """Two GPUs; GPU 1 (oam 1) is in DPX mode: processors 1 and 2."""

    def __init__(self):
        self.asked = []

    def init(self):
        pass

    def shutdown(self):
        pass

    def enumerate(self):
        return [
            {"index": 0, "oam_id": 0, "current_partition_id": 0},
            # listed partition-1 first: the head is found by partition id
            {"index": 1, "oam_id": 1, "current_partition_id": 1,
             "compute_partition": "DPX"},
            {"index": 2, "oam_id": 1, "current_partition_id": 0,
             "compute_partition": "DPX"},
        ]

    def health_signals(self, index):
        self.asked.append(index)
        return {
            "ecc_correctable": 12,
            "ecc_uncorrectable": 1,
            "ecc_deferred": 0,
            "ecc_blocks": {
                "UMC": {"correctable": 12, "uncorrectable": 1, "deferred": 0}
            },
            "bad_pages_reserved": 2,
            "bad_pages_pending": 0,
            "bad_pages_unreservable": 0,
            "temp_hotspot_c": 64,
            "temp_hotspot_crit_c": 110,
            "temp_vram_c": 51,
            "throttle_prochot": False,
            "throttle_ppt": True,
            "unsupported": {
                "bad_page_threshold": "AMDSMI_STATUS_NO_PERM",
                "temp_vram_crit_c": "AMDSMI_STATUS_NOT_SUPPORTED",
                "throttle_socket_thermal": "not reported (0xFF)",
                "throttle_vr_thermal": "not reported (0xFF)",
                "throttle_hbm_thermal": "not reported (0xFF)",
                "ecc_blocks.GFX": "AMDSMI_STATUS_NOT_SUPPORTED",
            },
        }


def test_amdsmi_backend_converts_values_and_unsupported():
    ext = StubExt()
    lib = AmdSmiDeviceLib(sysfs_root="/nonexistent", ext=ext)
    lib.open()
    s = lib.health_signals(0)
    assert ext.asked == [0]
    assert reported_once(s)
    assert (s.ecc_correctable, s.ecc_uncorrectable, s.ecc_deferred) == (12, 1, 0)
    assert s.ecc_blocks["UMC"]["uncorrectable"] == 1
    assert (s.bad_pages_reserved, s.bad_pages_pending) == (2, 0)
    assert s.bad_page_threshold is None
    assert s.unsupported["bad_page_threshold"] == "AMDSMI_STATUS_NO_PERM"
    assert s.temp_hotspot_c == 64 and s.temp_vram_crit_c is None
    assert s.throttle_ppt is True and s.throttle_prochot is False
    assert s.throttle_hbm_thermal is None
    assert s.active_throttles() == ["throttle_ppt"]
    # per-block refusals are carried through, not dropped
    assert "ecc_blocks.GFX" in s.unsupported
    # unsupported threshold -> a warning, not a threshold finding
    assert [f.reason for f in evaluate(s, s, s)] == [
        "UncorrectableEccHistoric",
        "RetiredPages",
        "Throttled",
    ]


def test_amdsmi_backend_asks_the_primary_processor():
    ext = StubExt()
    lib = AmdSmiDeviceLib(sysfs_root="/nonexistent", ext=ext)
    lib.open()
    lib.health_signals(1)
    assert ext.asked == [2]  # partition 0 of GPU 1 is processor 2


def test_amdsmi_backend_marks_silently_missing_signals_unsupported():
    class Sparse(StubExt):
        def health_signals(self, index):
            return {"ecc_uncorrectable": 0, "unsupported": {}}

    lib = AmdSmiDeviceLib(sysfs_root="/nonexistent", ext=Sparse())
    lib.open()
    s = lib.health_signals(0)
    assert reported_once(s)
    assert s.ecc_uncorrectable == 0
    assert s.bad_pages_pending is None  # never a zero


# ---------------------------------------------------------------------------
# KFD / sysfs backend
# ---------------------------------------------------------------------------
def write(path, text):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        f.write(text)


def make_tree(root, *, ras=True, hwmon=True):
    """One GPU (KFD node 1, renderD128) with clean RAS files and sensors."""
    root = str(root)
    nodes = os.path.join(root, "class", "kfd", "kfd", "topology", "nodes")
    write(os.path.join(nodes, "0", "properties"), "simd_count 0\n")
    write(
        os.path.join(nodes, "1", "properties"),
        "simd_count 1024\nsimd_per_cu 4\ngfx_target_version 90500\n"
        "drm_render_minor 128\nlocation_id 768\ndomain 0\nunique_id 43981\n",
    )
    dev = os.path.join(root, "devices", "pci-gpu-0")
    os.makedirs(dev)
    drm = os.path.join(root, "class", "drm")
    for name in ("card0", "renderD128"):
        os.makedirs(os.path.join(drm, name))
        os.symlink(dev, os.path.join(drm, name, "device"))
    if ras:
        for block in ("umc", "gfx", "sdma"):
            write(
                os.path.join(dev, "ras", f"{block}_err_count"),
                "ue: 0\nce: 0\nde: 0\n",
            )
        write(os.path.join(dev, "ras", "gpu_vram_bad_pages"), "")
        write(os.path.join(dev, "ras", "features"), "feature mask: 0x3fff\n")
    if hwmon:
        hw = os.path.join(dev, "hwmon", "hwmon4")
        write(os.path.join(hw, "temp1_label"), "junction\n")
        write(os.path.join(hw, "temp1_input"), "48000\n")
        write(os.path.join(hw, "temp1_crit"), "100000\n")
        write(os.path.join(hw, "temp2_label"), "mem\n")
        write(os.path.join(hw, "temp2_input"), "41000\n")
        write(os.path.join(hw, "temp2_crit"), "105000\n")
    return dev


def kfd_lib(root):
    lib = KfdDeviceLib(sysfs_root=str(root))
    lib.open()
    return lib


def test_kfd_clean_tree(tmp_path):
    make_tree(tmp_path)
    s = kfd_lib(tmp_path).health_signals(0)
    assert reported_once(s)
    assert (s.ecc_correctable, s.ecc_uncorrectable, s.ecc_deferred) == (0, 0, 0)
    assert sorted(s.ecc_blocks) == ["GFX", "SDMA", "UMC"]
    assert (
        s.bad_pages_reserved,
        s.bad_pages_pending,
        s.bad_pages_unreservable,
    ) == (0, 0, 0)
    assert (s.temp_hotspot_c, s.temp_hotspot_crit_c) == (48.0, 100.0)
    assert (s.temp_vram_c, s.temp_vram_crit_c) == (41.0, 105.0)
    # no plain-text sysfs source for these
    assert set(s.unsupported) == {"bad_page_threshold", *THROTTLE_SIGNALS}
    assert evaluate(s, s, s) == []


def test_kfd_uncorrectable_in_umc(tmp_path):
    dev = make_tree(tmp_path)
    lib = kfd_lib(tmp_path)
    baseline = lib.health_signals(0)
    write(os.path.join(dev, "ras", "umc_err_count"), "ue: 3\nce: 5\n")
    write(os.path.join(dev, "ras", "gfx_err_count"), "ue: 0\nce: 2\nde: 1\n")
    s = lib.health_signals(0)
    assert s.ecc_uncorrectable == 3
    assert s.ecc_correctable == 7  # totals are the sum over blocks
    assert s.ecc_deferred == 1  # umc has no de: line; the others count
    assert s.ecc_blocks["UMC"] == {"uncorrectable": 3, "correctable": 5}
    assert [f.reason for f in evaluate(baseline, baseline, s)] == [
        "UncorrectableEcc",
        "CorrectableEccGrowth",
        "DeferredEcc",
    ]


def test_kfd_old_kernel_without_deferred_lines(tmp_path):
    dev = make_tree(tmp_path)
    for block in ("umc", "gfx", "sdma"):
        write(os.path.join(dev, "ras", f"{block}_err_count"), "ue: 0\nce: 1\n")
    s = kfd_lib(tmp_path).health_signals(0)
    assert reported_once(s)
    assert s.ecc_correctable == 3
    assert s.ecc_deferred is None and "ecc_deferred" in s.unsupported


def test_kfd_aca_layout_as_on_mi355x(tmp_path):
    """MI355X nodes name the per-block files ras/aca_<block> (same ue/ce/de
    lines) and have no *_err_count files; other ras/ files are not blocks."""
    dev = make_tree(tmp_path)
    for block in ("umc", "gfx", "sdma"):
        os.remove(os.path.join(dev, "ras", f"{block}_err_count"))
    for block, ue in (("umc", 2), ("gfx", 0), ("xgmi_wafl", 1), ("vcn", 0)):
        write(
            os.path.join(dev, "ras", f"aca_{block}"),
            f"ue: {ue}\nce: 4\nde: 0\n",
        )
    write(os.path.join(dev, "ras", "schema"), "schema: 0x8\n")
    write(
        os.path.join(dev, "ras", "event_state"),
        "current seqno: 1\nFatal Error: count:0, last_seqno:0\n",
    )
    s = kfd_lib(tmp_path).health_signals(0)
    assert reported_once(s)
    assert sorted(s.ecc_blocks) == ["GFX", "UMC", "VCN", "XGMI_WAFL"]
    assert (s.ecc_uncorrectable, s.ecc_correctable, s.ecc_deferred) == (3, 16, 0)
    # a block present under both names is counted once
    write(os.path.join(dev, "ras", "umc_err_count"), "ue: 2\nce: 4\nde: 0\n")
    assert kfd_lib(tmp_path).health_signals(0).ecc_uncorrectable == 3


def test_kfd_bad_pages_by_flag(tmp_path):
    dev = make_tree(tmp_path)
    write(
        os.path.join(dev, "ras", "gpu_vram_bad_pages"),
        "0x00000001 : 0x00001000 : R\n"
        "0x00000002 : 0x00001000 : P\n"
        "0x00000003 : 0x00001000 : F\n",
    )
    s = kfd_lib(tmp_path).health_signals(0)
    assert (
        s.bad_pages_reserved,
        s.bad_pages_pending,
        s.bad_pages_unreservable,
    ) == (1, 1, 1)
    assert [f.reason for f in evaluate(s, s, s)] == [
        "BadPagesPending",
        "BadPageUnreservable",
        "RetiredPages",
    ]


def test_kfd_junction_above_critical(tmp_path):
    dev = make_tree(tmp_path)
    write(os.path.join(dev, "hwmon", "hwmon4", "temp1_input"), "101000\n")
    s = kfd_lib(tmp_path).health_signals(0)
    assert s.temp_hotspot_c == 101.0 and s.temp_hotspot_crit_c == 100.0
    found = evaluate(s, s, s)
    assert [(f.reason, f.severity) for f in found] == [("ThermalCritical", "soft")]
    assert "hotspot" in found[0].detail


def test_kfd_without_ras_directory(tmp_path):
    make_tree(tmp_path, ras=False)
    s = kfd_lib(tmp_path).health_signals(0)  # no exception
    assert reported_once(s)
    for name in ECC_SIGNALS + ("ecc_blocks",) + BAD_PAGE_SIGNALS:
        assert getattr(s, name) is None
        assert name in s.unsupported
    assert s.temp_hotspot_c == 48.0  # the rest is still read
    assert evaluate(s, s, s) == []


def test_kfd_without_hwmon(tmp_path):
    make_tree(tmp_path, hwmon=False)
    s = kfd_lib(tmp_path).health_signals(0)
    assert reported_once(s)
    assert s.temp_hotspot_c is None and s.temp_vram_crit_c is None
    assert s.ecc_uncorrectable == 0


def test_kfd_sensor_without_crit_file(tmp_path):
    dev = make_tree(tmp_path)
    os.remove(os.path.join(dev, "hwmon", "hwmon4", "temp2_crit"))
    s = kfd_lib(tmp_path).health_signals(0)
    assert reported_once(s)
    assert s.temp_vram_c == 41.0
    assert s.temp_vram_crit_c is None


def test_kfd_unknown_gpu_index(tmp_path):
    from k8s_dra_driver_amd.hal.base import HalError

    make_tree(tmp_path)
    with pytest.raises(HalError):
        kfd_lib(tmp_path).health_signals(3)
