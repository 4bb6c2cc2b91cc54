"""RepartitionLedger: the differences between the mode-switch sites of
DeviceState (explicit PartitionConfig, auto-carve, rollback, unprepare,
drain retry) are behaviour. One small test per cell that differs, on the
fake HAL with injected faults, plus the locking of the deferred-restore map.
"""

import threading
import time
from dataclasses import fields

import pytest

from k8s_dra_driver_amd.api.types import API_GROUP_VERSION
from k8s_dra_driver_amd.hal.base import HalError
from k8s_dra_driver_amd.partition.manager import RepartitionFailed
from k8s_dra_driver_amd.state.devicestate import PrepareError
from k8s_dra_driver_amd.state.repartition import RepartitionLedger
from tests.test_devicestate import make_claim, make_state, opaque

CPX_CFG = opaque(
    {
        "apiVersion": API_GROUP_VERSION,
        "kind": "PartitionConfig",
        "computePartition": "CPX",
        "memoryPartition": "NPS4",
        "allowDynamicRepartition": True,
    }
)


def _mode(lib, gpu_index=0):
    g = lib.enumerate()[gpu_index]
    return (g.compute_partition, g.memory_partition)


def _observed(state):
    """Wire both ledger callbacks the way the Driver does. Returns (switch count holder, deferred counts)."""
    switches, deferred = [], []
    state.ledger.on_repartition = lambda: switches.append(1)
    state.ledger.on_deferred_restores_change = deferred.append
    return switches, deferred


def _fail_claim_spec_write(state, claim_uid, before_raise=lambda: None):
    """Make the claim-spec write of one claim fail, so that its prepare
    rolls back after a successful carve."""
    write = state.cdi.create_claim_spec

    def boom(uid, *a, **k):
        if uid != claim_uid:
            return write(uid, *a, **k)
        before_raise()
        raise OSError("disk full")

    state.cdi.create_claim_spec = boom


# -- on_repartition: rollback stays silent, unprepare fires ------------------
def test_rollback_does_not_fire_on_repartition_and_unprepare_does(tmp_path):
    state, lib = make_state(tmp_path)
    switches, _ = _observed(state)
    _fail_claim_spec_write(state, "u-rb")
    with pytest.raises(OSError):
        state.prepare(make_claim("u-rb", ["gpu-0"], configs=[CPX_CFG]))
    # the carve fired once; the revert switched the GPU back without firing
    assert _mode(lib) == ("SPX", "NPS1")
    assert len(switches) == 1

    state.prepare(make_claim("u-ok", ["gpu-0"], configs=[CPX_CFG]))
    assert len(switches) == 2
    state.unprepare("u-ok")
    assert _mode(lib) == ("SPX", "NPS1")
    assert len(switches) == 3


# -- deferred entry: unprepare assigns, rollback uses setdefault -------------
def test_unprepare_overwrites_a_pending_deferred_restore(tmp_path):
    state, lib = make_state(tmp_path)
    _, deferred = _observed(state)
    state.prepare(make_claim("u-own", ["gpu-0"], configs=[CPX_CFG]))
    state.prepare(make_claim("u-other", ["gpu-0-cpx-3"]))
    state.ledger.defer(0, ("DPX", "NPS1"), overwrite=False)
    state.unprepare("u-own")  # refused: u-other still holds gpu-0
    assert _mode(lib) == ("CPX", "NPS4")
    assert deferred[-1] == 1
    state.unprepare("u-other")  # drained: the pending restore is applied
    assert _mode(lib) == ("SPX", "NPS1")  # u-own's target replaced DPX/NPS1
    assert deferred[-1] == 0


def test_rollback_keeps_a_pending_deferred_restore(tmp_path):
    state, lib = make_state(tmp_path)
    _, deferred = _observed(state)
    state.ledger.defer(0, ("DPX", "NPS1"), overwrite=False)
    # the carve succeeds, the claim-spec write fails, and the revert that
    # rollback attempts hits a HAL fault on its first step
    _fail_claim_spec_write(
        state,
        "u-rb",
        lambda: lib.faults.fail_next("set_memory_partition", HalError("flaky")),
    )
    with pytest.raises(OSError):
        state.prepare(make_claim("u-rb", ["gpu-0"], configs=[CPX_CFG]))
    assert _mode(lib) == ("CPX", "NPS4")
    assert deferred[-1] == 1
    state.unprepare("no-such-claim")  # sweep: gpu-0 has no holders
    assert _mode(lib) == ("DPX", "NPS1")  # the earlier entry won
    assert deferred[-1] == 0


def test_rollback_leaves_a_refused_gpu_partitioned_without_deferring(tmp_path):
    state, lib = make_state(tmp_path)
    _, deferred = _observed(state)
    # by the time u-rb rolls back, another claim holds a partition of gpu-0
    _fail_claim_spec_write(
        state, "u-rb", lambda: state.prepare(make_claim("u-other", ["gpu-0-cpx-3"]))
    )
    with pytest.raises(OSError):
        state.prepare(make_claim("u-rb", ["gpu-0"], configs=[CPX_CFG]))
    assert _mode(lib) == ("CPX", "NPS4")
    assert deferred == []
    state.unprepare("u-other")  # nothing pending: the GPU stays carved
    assert _mode(lib) == ("CPX", "NPS4")


# -- failures: unprepare propagates, the drain retry keeps the entry ---------
def test_unprepare_propagates_failed_restore_and_can_be_repeated(tmp_path):
    state, lib = make_state(tmp_path)
    _, deferred = _observed(state)
    state.prepare(make_claim("u-f", ["gpu-0"], configs=[CPX_CFG]))
    lib.faults.fail_next("set_memory_partition", HalError("flaky"))
    with pytest.raises(RepartitionFailed):
        state.unprepare("u-f")
    # nothing was deferred and the claim is still checkpointed, so kubelet's
    # retry finds it; holdership was released before the restore attempt
    assert deferred == []
    assert state.checkpoints.read("u-f") is not None
    assert state.claims_holding_gpu(0) == []
    state.unprepare("u-f")
    assert _mode(lib) == ("SPX", "NPS1")
    assert state.checkpoints.read("u-f") is None
    assert state.claims_holding_gpu(0) == []
    assert state.cdi.list_claim_spec_uids() == []


def test_drain_retry_keeps_entry_while_held_and_clears_it_when_drained(tmp_path):
    state, lib = make_state(tmp_path)
    _, deferred = _observed(state)
    state.prepare(make_claim("u-own", ["gpu-0"], configs=[CPX_CFG]))
    state.prepare(make_claim("u-other", ["gpu-0-cpx-3"]))
    state.unprepare("u-own")
    assert deferred == [1]
    state.unprepare("no-such-claim")  # sweep while u-other holds gpu-0
    assert _mode(lib) == ("CPX", "NPS4")
    assert deferred == [1]
    state.unprepare("u-other")
    assert _mode(lib) == ("SPX", "NPS1")
    assert deferred == [1, 0]


def test_drain_retry_keeps_entry_when_the_switch_fails(tmp_path):
    state, lib = make_state(tmp_path)
    _, deferred = _observed(state)
    state.partition_manager.ensure_mode(0, "CPX", "NPS4", allow_dynamic=True)
    state.ledger.defer(0, ("SPX", "NPS1"), overwrite=False)
    lib.faults.fail_next("set_memory_partition", HalError("flaky"))
    state.unprepare("no-such-claim")  # swallowed: retried on the next one
    assert _mode(lib) == ("CPX", "NPS4")
    assert deferred == [1]
    state.unprepare("no-such-claim")
    assert _mode(lib) == ("SPX", "NPS1")
    assert deferred == [1, 0]


# -- prepare: explicit PartitionConfig vs scheduler-driven carve -------------
@pytest.mark.parametrize(
    "claim, message",
    [
        (
            make_claim("u-x", ["gpu-0"], configs=[CPX_CFG]),
            r"^gpu-0 mode switch to CPX/NPS4 failed",
        ),
        (
            make_claim("u-x", ["gpu-0-cpx-3"]),
            r"^auto-carve of gpu-0 to CPX failed: gpu-0 mode switch",
        ),
    ],
    ids=["explicit", "auto-carve"],
)
def test_failed_switch_in_prepare_defers_the_original_mode(tmp_path, claim, message):
    state, lib = make_state(tmp_path)
    switches, deferred = _observed(state)
    # the carve reports a failure after the mode has moved, and the
    # manager's own revert fails as well
    set_compute = lib.set_compute_partition

    def moves_then_fails(gpu_index, mode):
        if mode != "SPX":
            set_compute(gpu_index, mode)
        raise HalError("flaky")

    lib.set_compute_partition = moves_then_fails
    with pytest.raises(PrepareError, match=message):
        state.prepare(claim)
    assert _mode(lib) == ("CPX", "NPS1")  # stuck in the intermediate mode
    assert switches == [] and deferred == [1]
    # publication was re-synced with what the hardware really is
    assert "gpu-0-cpx-0" in {d.canonical_name for d in state.allocatable_devices()}
    lib.set_compute_partition = set_compute
    state.unprepare("no-such-claim")
    assert _mode(lib) == ("SPX", "NPS1")
    assert deferred == [1, 0]


def test_refused_switch_messages_in_prepare(tmp_path):
    state, _ = make_state(tmp_path)
    state.prepare(make_claim("u-hold", ["gpu-0"]))
    with pytest.raises(PrepareError, match=r"^gpu-0 repartition refused: held by"):
        state.prepare(make_claim("u-x", ["gpu-0"], configs=[CPX_CFG]))
    with pytest.raises(
        PrepareError,
        match=r"^allocated device 'gpu-0-cpx-3' requires carving gpu-0 to CPX: gpu-0 rep",
    ):
        state.prepare(make_claim("u-y", ["gpu-0-cpx-3"]))


# -- the deferred-restore map under its lock ---------------------------------
class _NoopManager:
    """ensure_mode finds every GPU already in the requested mode."""

    def __init__(self, during_switch=lambda: None):
        self.applied = set()
        self.during_switch = during_switch

    def ensure_mode(self, gpu_index, compute, memory, **kwargs):
        self.applied.add((compute, memory))
        self.during_switch()
        return False


def test_restore_recorded_during_a_retry_is_not_dropped():
    counts = []
    manager = _NoopManager()
    ledger = RepartitionLedger(manager, resync=lambda: None)
    ledger.on_deferred_restores_change = counts.append
    ledger.defer(5, ("SPX", "NPS1"), overwrite=True)
    # another claim records a different restore for gpu-5 while the retry
    # is inside ensure_mode (which also shows the lock is not held there)
    manager.during_switch = lambda: ledger.defer(5, ("DPX", "NPS1"), overwrite=True)
    ledger.retry_deferred("sweep")
    manager.during_switch = lambda: None
    assert counts[-1] == 1
    assert ("DPX", "NPS1") not in manager.applied
    ledger.retry_deferred("sweep")
    assert ("DPX", "NPS1") in manager.applied
    assert counts[-1] == 0


def test_concurrent_record_and_retry_never_drop_the_last_record():
    threads_n, rounds, iterations = 4, 40, 8
    manager = _NoopManager(during_switch=lambda: time.sleep(0))  # yield mid-retry
    ledger = RepartitionLedger(manager, resync=lambda: None)
    counts = []
    ledger.on_deferred_restores_change = counts.append
    barrier = threading.Barrier(threads_n + 1)
    order_lock = threading.Lock()
    recorded = []  # every record, in the order the ledger took them

    def record(target):
        with order_lock:
            ledger.defer(5, target, overwrite=True)
            recorded.append(target)

    def run(tid):
        try:
            for rnd in range(rounds):
                barrier.wait()
                for k in range(iterations):
                    target = ("SPX", f"t{tid}-{rnd}-{k}")  # unique: a record is traceable
                    if tid % 2:
                        record(target)
                        ledger.retry_deferred(f"t{tid}")
                    else:
                        ledger.retry_deferred(f"t{tid}")
                        record(target)
                barrier.wait()
        except threading.BrokenBarrierError:
            pass  # the main thread is done, or found a violation and gave up

    threads = [threading.Thread(target=run, args=(t,)) for t in range(threads_n)]
    for t in threads:
        t.start()
    try:
        for rnd in range(rounds):
            barrier.wait(timeout=10)  # the round runs
            barrier.wait(timeout=10)  # every thread idles until the next round
            with ledger._lock:
                final = dict(ledger._deferred_restores)
            last = recorded[-1]
            # the last record is either still pending or was applied by a retry
            # that started after it; it is never deleted unapplied
            assert final == {5: last} or (final == {} and last in manager.applied), rnd
            assert counts[-1] == len(final), rnd
    finally:
        barrier.abort()  # releases the workers if an assertion ended the loop early
        for t in threads:
            t.join(timeout=10)


# -- PreparedClaim carries only what is checkpointed -------------------------
def test_prepared_claim_has_no_attributes_beyond_its_fields(tmp_path):
    state, _ = make_state(tmp_path)
    state.prepare(make_claim("u-plain", ["gpu-0"]))
    pc = state.checkpoints.read("u-plain")
    assert vars(pc).keys() == {f.name for f in fields(pc)}
