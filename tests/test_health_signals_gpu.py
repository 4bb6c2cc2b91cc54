"""Passive health signals on a real MI355X: the native binding, the two
real backends against each other, and the monitor on real telemetry.

Nothing here launches a kernel: the signals are counters and sensors the
amdgpu driver keeps, read through AMD SMI and sysfs.
"""

import os
import time

import pytest

from k8s_dra_driver_amd.hal.model import (
    BAD_PAGE_SIGNALS,
    ECC_SIGNALS,
    HEALTH_SIGNAL_NAMES,
    TEMP_SIGNALS,
    THROTTLE_SIGNALS,
)

pytestmark = pytest.mark.gpu

COUNT_SIGNALS = ECC_SIGNALS + BAD_PAGE_SIGNALS + ("bad_page_threshold",)
#: plausible range for a powered MI355X sensor or its critical limit
TEMP_RANGE_C = (10, 120)


@pytest.fixture(scope="module")
def real_lib():
    from k8s_dra_driver_amd.hal.amdsmi import AmdSmiDeviceLib

    lib = AmdSmiDeviceLib()
    lib.open()
    yield lib
    lib.close()


@pytest.fixture(scope="module")
def kfd_lib():
    from k8s_dra_driver_amd.hal.kfd import KfdDeviceLib

    lib = KfdDeviceLib()
    lib.open()
    yield lib
    lib.close()


def dump(title, signals):
    print(f"\n{title}")
    for k, v in signals.items():
        if k != "unsupported":
            print(f"  {k}: {v}")
    for k, v in sorted(signals.get("unsupported", {}).items()):
        print(f"  unsupported {k}: {v}")


class TestNativeBinding:
    def test_every_signal_exactly_once(self, real_lib):
        from k8s_dra_driver_amd import _amdhal

        raw = _amdhal.health_signals(0)
        dump("_amdhal.health_signals(0)", raw)
        unsupported = raw["unsupported"]
        assert isinstance(unsupported, dict)
        for name in HEALTH_SIGNAL_NAMES:
            assert (name in raw) != (name in unsupported), name
        # nothing unnamed: every other key is a per-block refusal
        assert set(raw) - {"unsupported"} <= set(HEALTH_SIGNAL_NAMES)
        for name, why in unsupported.items():
            assert name in HEALTH_SIGNAL_NAMES or name.startswith("ecc_blocks.")
            assert isinstance(why, str) and why

        for name in COUNT_SIGNALS:
            if name in raw:
                assert type(raw[name]) is int and raw[name] >= 0, name
        for block, counts in raw.get("ecc_blocks", {}).items():
            assert block not in (f[len("ecc_blocks."):] for f in unsupported)
            assert set(counts) == {"correctable", "uncorrectable", "deferred"}
            assert all(type(c) is int and c >= 0 for c in counts.values())
        for name in TEMP_SIGNALS:
            if name in raw:
                assert TEMP_RANGE_C[0] <= raw[name] <= TEMP_RANGE_C[1], name
        for name in THROTTLE_SIGNALS:
            if name in raw:
                assert type(raw[name]) is bool, name

        supported = [n for n in HEALTH_SIGNAL_NAMES if n in raw]
        assert supported, (
            "AMD SMI answered 'unsupported' to every health signal: "
            f"{unsupported}"
        )

    def test_out_of_range_index_raises(self, real_lib):
        from k8s_dra_driver_amd import _amdhal

        with pytest.raises(IndexError):
            _amdhal.health_signals(10_000)

    def test_enumerate_is_not_blocked_by_a_concurrent_reader(self, real_lib):
        """health_signals drops the GIL before it takes the native mutex;
        enumerate() takes the mutex while holding the GIL. Both orders
        must make progress."""
        import threading

        from k8s_dra_driver_amd import _amdhal

        errors = []

        def reader():
            try:
                for _ in range(3):
                    _amdhal.health_signals(0)
            except Exception as e:  # pragma: no cover - reported below
                errors.append(e)

        t = threading.Thread(target=reader)
        t.start()
        for _ in range(3):
            assert _amdhal.enumerate()
        t.join(timeout=60)
        assert not t.is_alive(), "health_signals/enumerate deadlocked"
        assert not errors


class TestBackendsAgree:
    def test_amdsmi_and_sysfs_report_the_same_counts(self, real_lib, kfd_lib):
        g = real_lib.enumerate()[0]
        kfd_index = next(
            k.index
            for k in kfd_lib.enumerate()
            if k.render_minor == g.render_minor
        )
        t0 = time.perf_counter()
        smi = real_lib.health_signals(g.index)
        smi_ms = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        sysfs = kfd_lib.health_signals(kfd_index)
        sysfs_ms = (time.perf_counter() - t0) * 1e3
        dump(f"amdsmi gpu-{g.index} ({smi_ms:.1f} ms)", smi.to_dict())
        dump(f"sysfs renderD{g.render_minor} ({sysfs_ms:.1f} ms)", sysfs.to_dict())

        both = []
        for name in ECC_SIGNALS + BAD_PAGE_SIGNALS:
            a, b = getattr(smi, name), getattr(sysfs, name)
            if a is not None and b is not None:
                both.append(name)
                assert a == b, f"{name}: amdsmi {a} != sysfs {b}"
        print(f"compared: {both}")
        for src in (smi, sysfs):
            for name in TEMP_SIGNALS:
                v = getattr(src, name)
                if v is not None:
                    assert TEMP_RANGE_C[0] <= v <= TEMP_RANGE_C[1], name
        for name in ("temp_hotspot_c", "temp_vram_c"):
            a, b = getattr(smi, name), getattr(sysfs, name)
            if a is not None and b is not None:
                # reported, not asserted: two reads a few ms apart
                print(f"{name}: amdsmi {a} C, sysfs {b} C, diff {a - b:+.1f} C")


class TestMonitorOnRealTelemetry:
    def test_healthy_box_stays_untainted(self, real_lib, tmp_path):
        from k8s_dra_driver_amd import DRIVER_NAME
        from k8s_dra_driver_amd.kube.client import InMemoryKube
        from k8s_dra_driver_amd.plugin.driver import Driver
        from k8s_dra_driver_amd.plugin.health import HealthMonitor

        mon = HealthMonitor(real_lib)
        first, second = mon.check_once(), mon.check_once()
        for g in real_lib.enumerate():
            for f in mon.findings(g.index):
                print(f"gpu-{g.index}: [{f.severity}] {f.reason}: {f.detail}")
        assert first == set() and second == set()

        kube = InMemoryKube()
        kube.api_versions = ["v1beta2", "v1beta1"]
        d = Driver(
            real_lib,
            kube,
            node_name="gpu-node",
            cdi_root=os.path.join(tmp_path, "cdi"),
            checkpoint_root=os.path.join(tmp_path, "state"),
            use_tmpfs=False,
        )
        d.startup()
        try:
            assert d.health.check_once() == set()
            assert d.health.check_once() == set()
            devs = {
                dev["name"]: dev
                for s in kube.list_resource_slices(DRIVER_NAME)
                for dev in s["spec"]["devices"]
            }
            assert "gpu-0" in devs
            assert "taints" not in devs["gpu-0"]
        finally:
            d.shutdown(unpublish=False)
