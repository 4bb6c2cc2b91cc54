"""On the MI355X node: the native claim-persistence path is the one in
use after build(), and whole-GPU lifecycles through the Driver with the
amdsmi HAL leave exactly the bytes the pure-Python path leaves."""

import pytest

pytestmark = pytest.mark.gpu

DRIVER_NAME = "gpu.amd.com"
NODE = "gpu-node"


@pytest.fixture
def native_switch():
    from k8s_dra_driver_amd.utils import atomicfile

    prev = atomicfile.set_native(True)
    yield atomicfile.set_native
    atomicfile.set_native(prev)


def _lifecycles(lib, root, claims):
    """Prepare + unprepare each (uid, device names) claim through a fresh
    Driver; returns [(checkpoint bytes, claim spec bytes)] as found on disk
    between the two calls."""
    from k8s_dra_driver_amd.kube.client import InMemoryKube
    from k8s_dra_driver_amd.plugin.driver import ClaimRef, Driver

    kube = InMemoryKube()
    driver = Driver(
        lib,
        kube,
        node_name=NODE,
        cdi_root=str(root / "cdi"),
        checkpoint_root=str(root / "state"),
        use_tmpfs=False,
    )
    driver.startup()
    out = []
    try:
        for uid, devices in claims:
            kube.put_resource_claim(
                {
                    "metadata": {"namespace": "default", "name": f"claim-{uid}", "uid": uid},
                    "status": {
                        "allocation": {
                            "devices": {
                                "results": [
                                    {
                                        "request": f"gpu-{i}",
                                        "driver": DRIVER_NAME,
                                        "pool": NODE,
                                        "device": d,
                                    }
                                    for i, d in enumerate(devices)
                                ]
                            }
                        }
                    },
                }
            )
            ref = [ClaimRef("default", f"claim-{uid}", uid)]
            res = driver.node_prepare_resources(ref)[uid]
            assert not res.error, res.error
            assert [d["device_name"] for d in res.devices] == list(devices)
            ckpt = open(driver.state.checkpoints._path(uid), "rb").read()
            spec = open(driver.state.cdi._claim_spec_path(uid), "rb").read()
            out.append((ckpt, spec))
            res = driver.node_unprepare_resources(ref)[uid]
            assert not res.error, res.error
    finally:
        driver.shutdown(unpublish=False)
    return out


def _both_paths(lib, tmp_path, native_switch, claims):
    native_switch(True)
    native = _lifecycles(lib, tmp_path / "native", claims)
    native_switch(False)
    python = _lifecycles(lib, tmp_path / "python", claims)
    return native, python


def test_claimio_is_loaded_and_in_use():
    from k8s_dra_driver_amd import _claimio
    from k8s_dra_driver_amd.utils import atomicfile

    assert atomicfile.native() is _claimio


def test_whole_gpu_lifecycles_same_bytes_as_python(tmp_path, native_switch):
    from k8s_dra_driver_amd.hal.amdsmi import AmdSmiDeviceLib

    lib = AmdSmiDeviceLib()
    lib.open()
    try:
        gpus = lib.enumerate()
        assert gpus, "no GPUs enumerated via amdsmi"
        name = gpus[0].canonical_name
        claims = [(f"hw-uid-{i}", [name]) for i in range(32)]
        native, python = _both_paths(lib, tmp_path, native_switch, claims)
    finally:
        lib.close()
    assert len(native) == 32
    assert native == python
    assert name.encode() in native[0][0] and name.encode() in native[0][1]


def test_eight_result_claim_same_bytes_as_python(tmp_path, native_switch, fake_lib):
    # the 1-GPU pool boxes cannot supply eight devices: fake HAL
    names = [g.canonical_name for g in fake_lib.enumerate()][:8]
    assert len(names) == 8
    claims = [("eight-uid", names)]
    native, python = _both_paths(fake_lib, tmp_path, native_switch, claims)
    assert native == python
    assert native[0][1].count(b'"name"') == 8
