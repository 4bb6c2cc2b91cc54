"""Guards the bench.py driver contract: flags, JSON schema, single line."""

import json
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.timeout(300)
def test_bench_json_contract():
    out = subprocess.run(
        [
            sys.executable,
            os.path.join(REPO, "bench.py"),
            "--steps",
            "2",
            "--warmup",
            "1",
            "--pods-per-step",
            "4",
        ],
        capture_output=True,
        text=True,
        cwd=REPO,
        timeout=280,
    )
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.strip().splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    d = json.loads(lines[0])
    for key in (
        "metric",
        "value",
        "unit",
        "n_gpus",
        "steps",
        "warmup",
        "ms_per_step",
        "higher_is_better",
        "scaling",
        "vs_baseline",
        "dtype",
        "data",
        "config",
    ):
        assert key in d, key
    assert d["metric"] == "gpu_pods_scheduled_per_sec"
    assert d["n_gpus"] == 1
    assert d["steps"] == 2 and d["warmup"] == 1
    assert d["higher_is_better"] is True
    assert d["scaling"] == "weak"
    assert d["vs_baseline"] is None  # reference publishes no number
    assert d["value"] > 0 and d["ms_per_step"] > 0
    cfg = d["config"]
    assert cfg["model"] == "dra-claim-lifecycle/whole"
    assert cfg["hal"] in ("fake", "amdsmi")
    assert cfg["alloc_prepare_p50_ms"] > 0
    # a plain run measures the headline only; the rest is behind --full
    assert "configs" not in cfg
    assert cfg["cpus"]  # the L3 domain it pinned itself to, or "unpinned"


def test_bench_cpu_list_parsing_and_pinning():
    sys.path.insert(0, REPO)
    import bench

    assert bench._parse_cpu_list("16-23,144-151\n") == set(range(16, 24)) | set(
        range(144, 152)
    )
    assert bench._parse_cpu_list("3") == {3}
    before = os.sched_getaffinity(0)
    try:
        pinned = bench.pin_to_one_l3()
        after = os.sched_getaffinity(0)
        if pinned:
            assert after < before
            assert after == bench._parse_cpu_list(pinned) & before
        else:
            assert after == before
    finally:
        for tid in os.listdir("/proc/self/task"):
            os.sched_setaffinity(int(tid), before)


@pytest.mark.timeout(300)
def test_bench_dump_outputs_reproducible(tmp_path):
    """--dump-outputs writes the last step's allocation results + prepare
    responses as float arrays, identical from run to run."""
    import numpy as np

    dumps = []
    for name in ("a", "b"):
        out = subprocess.run(
            [
                sys.executable,
                os.path.join(REPO, "bench.py"),
                "--steps", "2", "--warmup", "1", "--pods-per-step", "4",
                "--hal", "fake",
                "--dump-outputs", str(tmp_path / name),
            ],
            capture_output=True,
            text=True,
            cwd=REPO,
            timeout=280,
        )
        assert out.returncode == 0, out.stderr[-2000:]
        files = sorted(os.listdir(tmp_path / name))
        assert files == ["lifecycle_results.npy", "prepared_device_counts.npy"]
        dumps.append({f: np.load(tmp_path / name / f) for f in files})
    a, b = dumps
    for f in a:
        assert a[f].dtype == np.float32
        assert np.array_equal(a[f], b[f]), f
    # one record per lifecycle of the last step, each with its one device
    assert a["prepared_device_counts.npy"].tolist() == [1.0] * 4
    rows = a["lifecycle_results.npy"]
    assert rows.shape[0] == 4
    rec = json.loads(bytes(rows[0].astype("uint8")).rstrip(b"\0"))
    (uid,) = rec["allocation"]
    assert rec["allocation"][uid][0]["device"] == "gpu-0"
    dev = rec["prepared"][uid][0]
    assert dev["device_name"] == "gpu-0"
    assert dev["pool_name"] == "bench-node-0"
    assert len(dev["cdi_device_ids"]) == 2


def test_metrics_histograms():
    from k8s_dra_driver_amd.metrics.prom import PluginMetrics
    from prometheus_client import generate_latest

    m = PluginMetrics()
    with m.time_prepare():
        pass
    m.prepared_claims.inc()
    m.allocatable_devices.set(8)
    text = generate_latest(m.registry).decode()
    assert "dra_prepare_seconds_bucket" in text
    assert "dra_prepared_claims_total 1.0" in text
    assert "dra_allocatable_devices 8.0" in text


def test_repartition_metric_counts(tmp_path):
    from k8s_dra_driver_amd.api.types import API_GROUP_VERSION
    from k8s_dra_driver_amd.hal import FakeDeviceLib
    from k8s_dra_driver_amd.kube.client import InMemoryKube
    from k8s_dra_driver_amd.plugin.driver import ClaimRef, Driver
    from prometheus_client import generate_latest

    lib = FakeDeviceLib()
    lib.open()
    kube = InMemoryKube()
    driver = Driver(
        lib,
        kube,
        node_name="n",
        cdi_root=str(tmp_path / "cdi"),
        checkpoint_root=str(tmp_path / "s"),
        use_tmpfs=False,
    )
    driver.startup()
    kube.put_resource_claim(
        {
            "metadata": {"namespace": "d", "name": "c", "uid": "u"},
            "status": {
                "allocation": {
                    "devices": {
                        "results": [
                            {
                                "request": "g",
                                "driver": "gpu.amd.com",
                                "pool": "n",
                                "device": "gpu-0",
                            }
                        ],
                        "config": [
                            {
                                "source": "FromClaim",
                                "requests": [],
                                "opaque": {
                                    "driver": "gpu.amd.com",
                                    "parameters": {
                                        "apiVersion": API_GROUP_VERSION,
                                        "kind": "PartitionConfig",
                                        "computePartition": "CPX",
                                        "memoryPartition": "NPS1",
                                        "allowDynamicRepartition": True,
                                    },
                                },
                            }
                        ],
                    }
                }
            },
        }
    )
    driver.node_prepare_resources([ClaimRef("d", "c", "u")])
    driver.node_unprepare_resources([ClaimRef("d", "c", "u")])
    text = generate_latest(driver.metrics.registry).decode()
    # one switch at prepare + one restore at unprepare
    assert "dra_repartitions_total 2.0" in text


def test_bench_all_configs_attested():
    """BASELINE configs #1-#5 are first-class bench modes:
    --full emits the whole-GPU headline plus per-config results."""
    out = subprocess.run(
        [
            sys.executable,
            os.path.join(REPO, "bench.py"),
            "--steps", "2", "--warmup", "1", "--pods-per-step", "8",
            "--full",
        ],
        capture_output=True,
        text=True,
        cwd=REPO,
        timeout=280,
    )
    assert out.returncode == 0, out.stderr[-2000:]
    d = json.loads(out.stdout.strip().splitlines()[-1])
    assert d["config"]["model"] == "dra-claim-lifecycle/whole"
    configs = d["config"]["configs"]
    for name in ("mock", "shared", "cpx", "topo4"):
        assert name in configs, name
        sub = configs[name]
        assert "error" not in sub, f"{name}: {sub}"
        assert sub["pods_per_sec"] > 0
        assert sub["alloc_prepare_p50_ms"] > 0
    assert configs["mock"]["hal"] == "fake"


def test_bench_hal_amdsmi_hard_fails_without_gpu():
    """--hal amdsmi must never silently bench the fake backend."""
    out = subprocess.run(
        [
            sys.executable,
            os.path.join(REPO, "bench.py"),
            "--steps", "1", "--warmup", "0", "--pods-per-step", "1",
            "--hal", "amdsmi",
        ],
        capture_output=True,
        text=True,
        cwd=REPO,
        timeout=280,
    )
    if out.returncode == 0:  # only on a real GPU box
        d = json.loads(out.stdout.strip().splitlines()[-1])
        assert d["config"]["hal"] == "amdsmi"
    else:
        assert "amdsmi" in out.stderr
