"""RepartitionLedger: who holds each GPU, which mode restores are pending,
and the only place under ``state/`` that asks the PartitionManager to
switch a GPU's mode.

``_lock`` guards both maps. It is never held across ``ensure_mode`` (the
manager calls back into ``holders`` through its ``in_use_fn`` and the lock
is not re-entrant) nor across any callback. One exception to "one lock":
``_notify_lock`` is held across ``on_deferred_restores_change`` and nothing
else, because only serialised calls can promise that the last count a
listener is given is the current one. That listener must not call back
into the ledger.
"""

from __future__ import annotations

import logging
import threading
from typing import Callable, Dict, Iterable, List, Optional

from ..partition.manager import PartitionManager, RepartitionFailed, RepartitionRefused

log = logging.getLogger(__name__)


class PrepareError(RuntimeError):
    pass


class RepartitionLedger:
    def __init__(self, manager: PartitionManager, resync: Callable[[], None]):
        self.manager = manager
        self._resync = resync
        #: optional callback per performed mode switch (metrics)
        self.on_repartition = None
        #: optional callback(count) when the deferred-restore set changes
        self.on_deferred_restores_change = None
        self._lock = threading.Lock()
        #: gpu_index -> set of claim uids with prepared devices on it
        self._gpu_holders: Dict[int, set] = {}
        #: gpu_index -> (compute, memory) restore that could not be applied
        #: yet; retried when the GPU drains
        self._deferred_restores: Dict[int, tuple] = {}
        #: serialises on_deferred_restores_change (see the module docstring)
        self._notify_lock = threading.Lock()

    def hold(self, claim_uid: str, devices: Iterable) -> None:
        with self._lock:
            for dev in devices:
                # adminAccess (monitoring) claims neither block
                # repartition drains nor count as exclusive holders
                if dev.parent_gpu_index >= 0 and not dev.admin:
                    self._gpu_holders.setdefault(dev.parent_gpu_index, set()).add(claim_uid)

    def holders(self, gpu_index: int) -> List[str]:
        with self._lock:
            return sorted(self._gpu_holders.get(gpu_index, ()))

    def defer(self, gpu_index: int, target: tuple, *, overwrite: bool) -> None:
        """Remember that the GPU should return to ``target``. Without
        ``overwrite`` a restore already pending for it wins."""
        with self._lock:
            if overwrite or gpu_index not in self._deferred_restores:
                self._deferred_restores[gpu_index] = target
        self._notify_deferred()

    def _notify_deferred(self) -> None:
        with self._notify_lock:
            with self._lock:
                count = len(self._deferred_restores)
            if self.on_deferred_restores_change is not None:
                try:
                    self.on_deferred_restores_change(count)
                except Exception:
                    pass

    def _switch(self, gpu_index, compute, memory, claim_uid, allow_dynamic, fire):
        switched = self.manager.ensure_mode(
            gpu_index, compute, memory, requesting_claim=claim_uid, allow_dynamic=allow_dynamic
        )
        if switched and fire and self.on_repartition is not None:
            self.on_repartition()
        return switched

    def switch_for_claim(
        self, gpu_index: int, compute: str, memory: str, claim_uid: str,
        *, allow_dynamic: bool, carve_for: Optional[str] = None,
    ) -> bool:
        """Mode switch during prepare; True if the GPU was switched. Every
        failure surfaces as PrepareError (the caller rolls back any earlier
        switch of the claim). ``carve_for`` names the prospective partition
        device of a scheduler-driven carve and selects that path's
        messages; None is the explicit PartitionConfig path."""
        carve_failed = f"auto-carve of gpu-{gpu_index} to {compute} failed: "
        try:
            return self._switch(gpu_index, compute, memory, claim_uid, allow_dynamic, True)
        except RepartitionRefused as e:
            if carve_for is None:
                raise PrepareError(str(e)) from e
            raise PrepareError(
                f"allocated device {carve_for!r} requires carving "
                f"gpu-{gpu_index} to {compute}: {e}"
            ) from e
        except RepartitionFailed as e:
            if not e.reverted:
                # The switch died mid-sequence and the manager's revert did
                # not restore the original mode: remember it as a deferred
                # restore (one already pending wins) and re-sync
                # publication with the actual hardware state.
                self.defer(gpu_index, e.original, overwrite=False)
                self._resync()
            raise PrepareError(str(e) if carve_for is None else f"{carve_failed}{e}") from e
        except Exception as e:
            # HAL failure mid-switch: surface typed
            explicit = f"repartition of gpu-{gpu_index} failed: "
            raise PrepareError(f"{explicit if carve_for is None else carve_failed}{e}") from e

    def revert(self, repartitioned: Dict[str, list], claim_uid: str) -> None:
        """Rollback of a failed prepare: return the GPUs the claim switched to
        their previous modes. Never raises, never fires ``on_repartition``."""
        moved = [
            self._restore_one(int(gpu_index), modes[0], modes[1], claim_uid, True)
            for gpu_index, modes in repartitioned.items()
        ]
        if any(moved):
            self._resync()

    def release(self, claim_uid: str, repartitioned: Dict[str, list]) -> None:
        """Unprepare: drop the claim's holdership first, so that it does not
        block its own drain check, then restore the modes it switched and
        retry the deferred restores. A failed restore reaches the caller."""
        with self._lock:
            for holders in self._gpu_holders.values():
                holders.discard(claim_uid)
            # read here so that a whole-GPU unprepare takes this lock once
            pending = list(self._deferred_restores.items())
        moved = False
        for gpu_index, modes in repartitioned.items():
            if self._restore_one(int(gpu_index), modes[0], modes[1], claim_uid, False):
                moved = True
        if repartitioned:
            pending = None  # read again: a refused restore above may have added one
        if self.retry_deferred(claim_uid, pending):
            moved = True
        if moved:
            self._resync()

    def _restore_one(self, gpu_index, compute, memory, claim_uid, rollback) -> bool:
        try:
            return self._switch(gpu_index, compute, memory, claim_uid, True, not rollback)
        except RepartitionRefused as e:
            if rollback:
                log.warning("rollback: leaving gpu-%s partitioned (%s)", gpu_index, e)
                return False
            # other claims still hold partitions of this GPU;
            # remember the restore and retry when it drains
            self.defer(gpu_index, (compute, memory), overwrite=True)
            log.warning(
                "leaving gpu-%s partitioned for now (%s); restore deferred "
                "until the GPU drains", gpu_index, e
            )
            return False
        except Exception as e:
            if not rollback:
                raise
            # revert itself failed (transient HAL error): remember
            # the target mode and retry when the GPU drains
            self.defer(gpu_index, (compute, memory), overwrite=False)
            log.warning("rollback: revert of gpu-%s failed (%s); restore deferred", gpu_index, e)
            return True  # hardware may have moved: re-sync

    def retry_deferred(self, claim_uid: str, pending: Optional[List[tuple]] = None) -> bool:
        """Apply deferred mode restores for GPUs that have drained (the
        last pod of a scheduler-carved GPU left: return it to SPX so the
        whole-GPU device becomes allocatable again). True if a GPU was
        switched; the caller re-syncs. ``pending``: the caller's snapshot."""
        if pending is None:
            with self._lock:
                pending = list(self._deferred_restores.items())
        restored = False
        for gpu_index, target in pending:
            if self.holders(gpu_index):
                continue
            try:
                if self._switch(gpu_index, *target, claim_uid, True, True):
                    restored = True
                    log.info(
                        "gpu-%d drained: deferred restore to %s/%s applied", gpu_index, *target
                    )
            except Exception:
                # raced a new prepare or transient HAL failure:
                # keep the entry, retried on the next unprepare
                continue
            with self._lock:
                if self._deferred_restores.get(gpu_index) != target:
                    continue  # a different restore recorded meanwhile stays
                del self._deferred_restores[gpu_index]
            self._notify_deferred()
        return restored
