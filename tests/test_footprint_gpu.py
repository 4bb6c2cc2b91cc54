"""CU footprint on an MI355X: the raw records of ``cu_where`` between their
guards, and where the blocks of a process really run, unmasked and under
the HSA_CU_MASK values the SharedCompute supervisor hands out.

Every measurement under a mask runs in a fresh child process, one at a
time (``footprint.measure``); the masks are quarter masks, 64 of 256 CUs,
which leave every XCD with CUs. No test provokes a fault.
"""

import numpy as np
import pytest

# torch must load before the system-ROCm-linked _hiphealth extension (see
# test_gpu.py): import order is load-bearing.
import torch  # noqa: F401

from k8s_dra_driver_amd.api.types import SharedComputeSettings
from k8s_dra_driver_amd.hal import FakeDeviceLib
from k8s_dra_driver_amd.hal.model import AllocatableDevice
from k8s_dra_driver_amd.sharing import footprint as F
from k8s_dra_driver_amd.sharing.shared import SharedComputeManager, cu_mask_hex

pytestmark = pytest.mark.gpu

LOW_QUARTER = "0:" + cu_mask_hex(0, 64)
NEXT_QUARTER = "0:" + cu_mask_hex(64, 64)


@pytest.fixture(scope="module")
def hh():
    from k8s_dra_driver_amd import _hiphealth

    assert _hiphealth.device_count() >= 1
    return _hiphealth


def _measure(cu_mask):
    fp = F.measure(0, cu_mask=cu_mask, timeout_s=60)
    print(
        f"mask {cu_mask!r}: {fp.count} CUs, per XCD {sorted(fp.per_xcc.items())}, "
        f"blocks per CU {fp.blocks_per_cu_min}..{fp.blocks_per_cu_max}, "
        f"kernel {fp.kernel_ms:.3f} ms, child {fp.seconds:.2f} s {fp.error}"
    )
    assert fp.ok, fp.error
    return fp


# measured once each, shared by the tests below and never modified
@pytest.fixture(scope="module")
def unmasked():
    return _measure(None)


@pytest.fixture(scope="module")
def low_quarter():
    return _measure(LOW_QUARTER)


@pytest.fixture(scope="module")
def next_quarter():
    return _measure(NEXT_QUARTER)


# ---------------------------------------------------------------------------
# cu_where, one launch between guards
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("spin", [0, 64])
@pytest.mark.parametrize("blocks", [1, 3, 257, 2048])
def test_probe_records(hh, blocks, spin):
    raw = hh.cu_footprint_probe(0, blocks, spin)
    guard = hh.PROBE_GUARD_BYTES
    assert len(raw) == guard + 16 * blocks + guard
    buf = np.frombuffer(raw, dtype=np.uint8)
    assert (buf[:guard] == hh.PROBE_CANARY).all()
    assert (buf[-guard:] == hh.PROBE_CANARY).all()
    rec = np.frombuffer(raw[guard:-guard], dtype="<u4").reshape(blocks, 4)
    assert (rec[:, 2] == np.arange(blocks)).all()  # its own block index
    assert (rec[:, 3] == 0).all()  # the pad
    assert (rec[:, 1] < 8).all()  # XCC_ID, nothing else of that register
    canary_word = int.from_bytes(bytes([hh.PROBE_CANARY]) * 4, "little")
    assert not (rec == canary_word).all(axis=1).any()
    # the host decode and its Python mirror name the same CUs
    keys = {F.decode(int(h), int(x)) for h, x in rec[:, :2]}
    assert 1 <= len(keys) <= blocks
    assert all(xcc < 8 and se < 4 and sh < 2 and cu < 16 for xcc, se, sh, cu in keys)


def test_arguments_are_validated_before_any_launch(hh):
    assert len(hh.cu_footprint_probe(0, 1, 0)) == 2 * hh.PROBE_GUARD_BYTES + 16
    for device, blocks, spin in [
        (-1, 1, 0),
        (hh.device_count(), 1, 0),
        (0, 0, 0),
        (0, -1, 0),
        (0, hh.FOOTPRINT_MAX_BLOCKS + 1, 0),
        (0, 1, -1),
        (0, 1, hh.FOOTPRINT_MAX_SPIN + 1),
    ]:
        with pytest.raises(ValueError):
            hh.cu_footprint_probe(device, blocks, spin)
    for device, blocks, spin in [
        (-1, 0, 0),
        (hh.device_count(), 0, 0),
        (0, -1, 0),
        (0, hh.FOOTPRINT_MAX_BLOCKS + 1, 0),
        (0, 0, -1),
        (0, 0, hh.FOOTPRINT_MAX_SPIN + 1),
    ]:
        with pytest.raises(ValueError):
            hh.cu_footprint(device, blocks, spin)


def test_production_path_in_this_process(hh):
    """The dict of ``cu_footprint`` agrees with itself; which CUs it lists
    is the business of the tests below, which choose the mask."""
    r = hh.cu_footprint(0)
    info = hh.device_info(0)
    assert r["multi_processor_count"] == info["multi_processor_count"]
    assert r["blocks"] == min(8 * info["multi_processor_count"], hh.FOOTPRINT_MAX_BLOCKS)
    assert r["spin"] == hh.FOOTPRINT_DEFAULT_SPIN
    assert r["cus"] == sorted(set(r["cus"])) and r["count"] == len(r["cus"])
    assert sum(r["per_xcc"].values()) == r["count"] and len(r["per_xcc"]) <= 8
    assert 1 <= r["blocks_per_cu_min"] <= r["blocks_per_cu_max"] <= r["blocks"]
    small = hh.cu_footprint(0, blocks=3, spin=16)
    assert small["blocks"] == 3 and small["spin"] == 16 and 1 <= small["count"] <= 3


# ---------------------------------------------------------------------------
# where a process runs
# ---------------------------------------------------------------------------
def test_unmasked_sees_every_cu(hh, unmasked):
    """What validates the register layout on real hardware: a field read
    from the wrong bits merges or splits CUs and the count is off."""
    info = hh.device_info(0)
    assert unmasked.multi_processor_count == info["multi_processor_count"]
    assert unmasked.count == info["multi_processor_count"]
    assert sum(unmasked.per_xcc.values()) == unmasked.count


def test_two_quarter_masks_are_disjoint_quarters(unmasked, low_quarter, next_quarter):
    for fp in (low_quarter, next_quarter):
        assert 0 < fp.count <= 64
        assert fp.cus <= unmasked.cus
        assert not fp.exceeds(fp.cu_mask)
    assert low_quarter.overlap(next_quarter) == frozenset()


def test_decimal_syntax_selects_the_same_cus(low_quarter):
    assert F.parse_cu_mask("0:0-63") == F.parse_cu_mask(LOW_QUARTER)
    assert _measure("0:0-63").cus == low_quarter.cus


def test_supervisor_sessions_run_on_disjoint_cus(tmp_path):
    lib = FakeDeviceLib()
    lib.open()
    try:
        gpu = lib.enumerate()[0]
        assert gpu.cu_count == 256
        devs = [AllocatableDevice.from_gpu(gpu)]
        mgr = SharedComputeManager(str(tmp_path), use_tmpfs=False)
        settings = SharedComputeSettings(default_cu_share_percent=25)
        masks = []
        for claim in ("claim-a", "claim-b"):
            session = mgr.start_session(claim, devs, settings)
            (entry,) = [e for e in session.env if e.startswith("HSA_CU_MASK=")]
            masks.append(entry.split("=", 1)[1])
    finally:
        lib.close()
    assert masks == [LOW_QUARTER, NEXT_QUARTER]
    a, b = (_measure(m) for m in masks)
    assert a.cu_mask == masks[0] and b.cu_mask == masks[1]
    assert a.count > 0 and b.count > 0
    assert a.overlap(b) == frozenset()
    assert not a.exceeds(masks[0]) and not b.exceeds(masks[1])
