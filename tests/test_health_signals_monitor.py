"""HealthMonitor driven by passive signals on the fake HAL: severity
classes, hysteresis, clearing, and how the Driver surfaces the result
(taint value, claim events, metrics)."""

import pytest

from k8s_dra_driver_amd import DRIVER_NAME
from k8s_dra_driver_amd.hal import FakeDeviceLib
from k8s_dra_driver_amd.hal.base import HalError
from k8s_dra_driver_amd.kube.client import InMemoryKube
from k8s_dra_driver_amd.plugin.driver import ClaimRef, Driver
from k8s_dra_driver_amd.plugin.health import HealthMonitor


def monitor(lib, **kw):
    changes = []
    kw.setdefault("failures_to_unhealthy", 2)
    mon = HealthMonitor(lib, on_change=lambda s: changes.append(set(s)), **kw)
    return mon, changes


def test_uncorrectable_growth_taints_on_the_same_poll(fake_lib):
    mon, changes = monitor(fake_lib)
    assert mon.check_once() == set()  # baseline poll
    fake_lib.set_health_signals(3, ecc_uncorrectable=1)
    assert mon.check_once() == {3}  # one poll, despite failures_to_unhealthy=2
    assert changes == [{3}]
    assert mon.primary_reason(3) == "UncorrectableEcc"
    assert [f.reason for f in mon.findings(3)] == ["UncorrectableEcc"]
    assert mon.findings(0) == []
    assert mon.primary_reason(0) == ""


def test_uncorrectable_stays_raised_until_counter_resets(fake_lib):
    mon, changes = monitor(fake_lib)
    mon.check_once()
    fake_lib.set_health_signals(1, ecc_uncorrectable=3)
    assert mon.check_once() == {1}
    # the count holds: still raised, poll after poll, no flapping
    for _ in range(3):
        assert mon.check_once() == {1}
        assert [f.reason for f in mon.findings(1)] == ["UncorrectableEcc"]
    assert changes == [{1}]
    # driver reload / GPU reset zeroes the counter: that clears it
    fake_lib.set_health_signals(1, ecc_uncorrectable=0)
    assert mon.check_once() == set()
    assert mon.findings(1) == []
    assert changes == [{1}, set()]
    # ... and the new, lower baseline still catches the next error
    fake_lib.set_health_signals(1, ecc_uncorrectable=1)
    assert mon.check_once() == {1}


def test_reset_below_nonzero_baseline_rebaselines(fake_lib):
    fake_lib.set_health_signals(0, ecc_uncorrectable=5)
    mon, _ = monitor(fake_lib)
    assert mon.check_once() == set()
    assert [f.reason for f in mon.findings(0)] == ["UncorrectableEccHistoric"]
    fake_lib.set_health_signals(0, ecc_uncorrectable=0)  # reset
    assert mon.check_once() == set()
    fake_lib.set_health_signals(0, ecc_uncorrectable=2)  # below old baseline
    assert mon.check_once() == {0}
    assert mon.primary_reason(0) == "UncorrectableEcc"


def test_recovery_needs_successes_to_healthy_clean_polls(fake_lib):
    mon, _ = monitor(fake_lib, successes_to_healthy=2)
    mon.check_once()
    fake_lib.set_health_signals(2, bad_pages_pending=1)
    assert mon.check_once() == {2}
    assert mon.primary_reason(2) == "BadPagesPending"
    fake_lib.set_health_signals(2, bad_pages_pending=0)
    assert mon.check_once() == {2}  # first clean poll
    assert mon.primary_reason(2) == "BadPagesPending"
    assert mon.check_once() == set()  # second clean poll
    assert mon.primary_reason(2) == ""


@pytest.mark.parametrize(
    "fields,reason",
    [
        ({"bad_pages_pending": 1}, "BadPagesPending"),
        ({"bad_pages_unreservable": 1}, "BadPageUnreservable"),
        (
            {"bad_pages_reserved": 128, "bad_page_threshold": 128},
            "BadPageThreshold",
        ),
    ],
)
def test_fatal_page_findings_taint_immediately(fake_lib, fields, reason):
    mon, _ = monitor(fake_lib)
    fake_lib.set_health_signals(4, **fields)
    assert mon.check_once() == {4}  # even on the very first poll
    assert mon.primary_reason(4) == reason


def test_thermal_critical_needs_two_polls(fake_lib):
    mon, changes = monitor(fake_lib)
    fake_lib.set_health_signals(5, temp_hotspot_c=110.0)
    assert mon.check_once() == set()
    assert [f.reason for f in mon.findings(5)] == ["ThermalCritical"]
    assert mon.check_once() == {5}
    assert mon.primary_reason(5) == "ThermalCritical"
    assert changes == [{5}]
    fake_lib.set_health_signals(5, temp_hotspot_c=70.0)
    assert mon.check_once() == set()


def test_one_hot_poll_is_forgiven(fake_lib):
    mon, changes = monitor(fake_lib)
    fake_lib.set_health_signals(5, temp_vram_c=105.0)
    assert mon.check_once() == set()
    fake_lib.set_health_signals(5, temp_vram_c=80.0)
    assert mon.check_once() == set()
    fake_lib.set_health_signals(5, temp_vram_c=105.0)
    assert mon.check_once() == set()  # not consecutive
    assert changes == []


def test_fatal_outranks_soft_as_primary_reason(fake_lib):
    mon, _ = monitor(fake_lib)
    fake_lib.set_health_signals(0, temp_hotspot_c=120.0)
    mon.check_once()
    assert mon.check_once() == {0}
    assert mon.primary_reason(0) == "ThermalCritical"
    fake_lib.set_health_signals(0, bad_pages_unreservable=1, bad_pages_pending=1)
    assert mon.check_once() == {0}
    assert mon.primary_reason(0) == "BadPagesPending"  # table order


def test_warnings_never_change_the_unhealthy_set(fake_lib):
    fake_lib.set_health_signals(6, ecc_uncorrectable=2)  # historic
    mon, changes = monitor(fake_lib, failures_to_unhealthy=1)
    reports = []
    mon.on_poll = reports.append
    assert mon.check_once() == set()
    fake_lib.set_health_signals(
        6,
        ecc_correctable=10,
        ecc_deferred=1,
        bad_pages_reserved=3,
        throttle_prochot=True,
    )
    for _ in range(3):
        assert mon.check_once() == set()
    assert changes == []
    assert {f.severity for f in mon.findings(6)} == {"warning"}
    assert {f.reason for f in mon.findings(6)} == {
        "UncorrectableEccHistoric",
        "RetiredPages",
        "Throttled",
    }  # growth warnings belong to the poll that saw the growth
    # each warning is reported as new exactly once
    new = [w for r in reports if r.gpu_index == 6 for w in r.new_warnings]
    assert sorted(new) == [
        "CorrectableEccGrowth",
        "DeferredEcc",
        "RetiredPages",
        "Throttled",
        "UncorrectableEccHistoric",
    ]


def test_health_signals_exception_is_one_soft_failure(fake_lib):
    mon, changes = monitor(fake_lib)
    fake_lib.faults.fail_next("health_signals", HalError("smi wedged"))
    assert mon.check_once() == set()  # one soft failure: below threshold
    assert [f.reason for f in mon.findings(0)] == ["HealthSignalsError"]
    assert mon.check_once() == set()  # and the loop goes on
    assert mon.findings(0) == []
    fake_lib.faults.fail_next("health_signals", HalError("smi wedged"))
    mon.check_once()
    # health_signals is called once per GPU per poll; 8 GPUs -> the next
    # poll's first call is gpu-0 again
    fake_lib.faults.fail_next("health_signals", HalError("smi wedged"))
    assert mon.check_once() == {0}
    assert mon.primary_reason(0) == "HealthSignalsError"
    assert changes == [{0}]


def test_unsupported_signal_is_no_finding_and_logged_once(fake_lib, caplog):
    fake_lib.set_health_signals(
        7, ecc_uncorrectable=None, bad_pages_pending=None, temp_hotspot_c=None
    )
    mon, changes = monitor(fake_lib)
    with caplog.at_level("INFO", logger="k8s_dra_driver_amd.plugin.health"):
        for _ in range(3):
            assert mon.check_once() == set()
    assert mon.findings(7) == []
    lines = [
        r.getMessage() for r in caplog.records if "unsupported" in r.getMessage()
    ]
    assert len(lines) == 3  # one per signal, not one per poll
    assert all(l.startswith("gpu-7:") for l in lines)


def test_default_backend_reports_everything_unsupported():
    """A backend that never heard of health signals keeps working."""
    from k8s_dra_driver_amd.hal.base import DeviceLib
    from k8s_dra_driver_amd.hal.model import HEALTH_SIGNAL_NAMES

    class Legacy(FakeDeviceLib):
        health_signals = DeviceLib.health_signals

    lib = Legacy()
    lib.open()
    assert set(lib.health_signals(0).unsupported) == set(HEALTH_SIGNAL_NAMES)
    mon, _ = monitor(lib)
    assert mon.check_once() == set()
    assert mon.check_once() == set()


# ---------------------------------------------------------------------------
# Driver surfacing
# ---------------------------------------------------------------------------
def make_driver(tmp_path, api_versions):
    lib = FakeDeviceLib()
    lib.open()
    kube = InMemoryKube()
    kube.api_versions = api_versions
    d = Driver(
        lib,
        kube,
        node_name="n",
        cdi_root=str(tmp_path / "cdi"),
        checkpoint_root=str(tmp_path / "state"),
        use_tmpfs=False,
    )
    d.startup()
    return d, kube, lib


def published(kube):
    return {
        dev["name"]: dev
        for s in kube.list_resource_slices(DRIVER_NAME)
        for dev in s["spec"]["devices"]
    }


def hold_gpu(driver, kube, device, uid):
    kube.put_resource_claim(
        {
            "metadata": {"namespace": "team-a", "name": f"claim-{uid}", "uid": uid},
            "status": {
                "allocation": {
                    "devices": {
                        "results": [
                            {
                                "request": "gpu",
                                "driver": DRIVER_NAME,
                                "pool": "n",
                                "device": device,
                            }
                        ]
                    }
                }
            },
        }
    )
    ref = ClaimRef("team-a", f"claim-{uid}", uid)
    res = driver.node_prepare_resources([ref])[uid]
    assert not res.error, res.error
    return ref


def sample(metrics, name, **labels):
    return metrics.registry.get_sample_value(name, labels)


def test_v1beta2_taint_value_event_and_metrics(tmp_path):
    d, kube, lib = make_driver(tmp_path, ["v1beta2", "v1beta1"])
    try:
        hold_gpu(d, kube, "gpu-2", "uid-held")
        hold_gpu(d, kube, "gpu-3", "uid-elsewhere")
        calls_before = lib.faults.call_counts.get("health_signals", 0)
        assert calls_before == 0  # prepare never reads health signals
        d.health.check_once()
        lib.set_health_signals(
            2, ecc_uncorrectable=4, ecc_correctable=17, bad_pages_reserved=2
        )
        lib.set_health_signals(2, temp_hotspot_c=71.0, temp_vram_c=None)
        for _ in range(3):
            d.health.check_once()

        devs = published(kube)
        assert devs["gpu-2"]["taints"] == [
            {
                "key": "gpu.amd.com/unhealthy",
                "effect": "NoSchedule",
                "value": "UncorrectableEcc",
            }
        ]
        assert "taints" not in devs["gpu-3"]

        events = [e for e in kube.events if e["reason"] == "DeviceUnhealthy"]
        assert len(events) == 1  # one per transition, not one per poll
        ev = events[0]
        assert ev["type"] == "Warning"
        assert ev["namespace"] == "team-a"
        assert ev["involvedObject"]["uid"] == "uid-held"
        assert ev["involvedObject"]["name"] == "claim-uid-held"
        assert "gpu-2" in ev["message"] and "UncorrectableEcc" in ev["message"]

        m = d.metrics
        assert sample(m, "dra_gpu_ecc_errors", gpu="2", kind="uncorrectable") == 4
        assert sample(m, "dra_gpu_ecc_errors", gpu="2", kind="correctable") == 17
        assert sample(m, "dra_gpu_ecc_errors", gpu="3", kind="uncorrectable") == 0
        assert sample(m, "dra_gpu_bad_pages", gpu="2", status="reserved") == 2
        assert sample(m, "dra_gpu_bad_pages", gpu="2", status="pending") == 0
        assert (
            sample(m, "dra_gpu_temperature_celsius", gpu="2", sensor="hotspot")
            == 71.0
        )
        # unsupported signal: no sample at all
        assert (
            sample(m, "dra_gpu_temperature_celsius", gpu="2", sensor="vram")
            is None
        )
        assert sample(m, "dra_gpu_unhealthy", gpu="2", reason="UncorrectableEcc") == 1
        assert sample(m, "dra_gpu_unhealthy", gpu="3", reason="UncorrectableEcc") is None
        assert (
            sample(
                m, "dra_gpu_health_warnings_total", gpu="2", reason="RetiredPages"
            )
            == 1
        )
        assert (
            sample(
                m,
                "dra_gpu_health_warnings_total",
                gpu="2",
                reason="CorrectableEccGrowth",
            )
            == 1
        )

        # recovery: counter reset -> taint and gauge go away; a second
        # transition emits a second event
        lib.set_health_signals(2, reset=True)
        d.health.check_once()
        assert "taints" not in published(kube)["gpu-2"]
        assert (
            sample(m, "dra_gpu_unhealthy", gpu="2", reason="UncorrectableEcc")
            is None
        )
        lib.set_health_signals(2, bad_pages_pending=1)
        d.health.check_once()
        assert published(kube)["gpu-2"]["taints"][0]["value"] == "BadPagesPending"
        events = [e for e in kube.events if e["reason"] == "DeviceUnhealthy"]
        assert len(events) == 2
    finally:
        d.shutdown(unpublish=False)


def test_v1beta1_removes_the_device(tmp_path):
    d, kube, lib = make_driver(tmp_path, ["v1beta1"])
    try:
        d.health.check_once()
        lib.set_health_signals(5, bad_pages_unreservable=1)
        d.health.check_once()
        devs = published(kube)
        assert "gpu-5" not in devs
        assert len(devs) == 7
        assert not any("taints" in dev for dev in devs.values())
    finally:
        d.shutdown(unpublish=False)


def test_clean_signals_publish_exactly_as_before(tmp_path):
    d, kube, lib = make_driver(tmp_path, ["v1beta2", "v1beta1"])
    try:
        before = published(kube)
        d.health.check_once()
        d.health.check_once()
        assert published(kube) == before
        assert not any("taints" in dev for dev in before.values())
        assert [e for e in kube.events if e["reason"] == "DeviceUnhealthy"] == []
    finally:
        d.shutdown(unpublish=False)
