"""DeviceState: the claim prepare/unprepare state machine.

Reference analog: ``cmd/nvidia-dra-plugin/device_state.go`` (Prepare :128,
Unprepare :161, prepareDevices :192, applyConfig :367). Differences that
matter for the pods-scheduled/sec metric (SURVEY.md §7 hard-part 5):

- **per-claim locking** instead of the reference's two coarse mutexes
  (driver.go:34 + device_state.go:46) that serialize every claim on the
  node; a per-GPU lock protects only partition changes;
- **per-claim checkpoint files** instead of a full-map rewrite per
  operation (checkpoint.py);
- **no subprocess execs** on the hot path: scheduler-quantum and partition
  calls go through the in-process HAL (vs exec'ing nvidia-smi per GPU,
  nvlib.go:521-558);
- **no daemon spawn + readiness poll** on the shared path: the
  SharedComputeManager is node-local and synchronous (vs seconds of
  Deployment polling, sharing.go:289-344).

Claim flow: checkpoint lookup (idempotency) -> allocation parse -> opaque
config decode + precedence merge -> partition intent -> sharing apply ->
CDI claim spec -> checkpoint write.
"""

from __future__ import annotations

import contextlib
import logging
import os
import re
import threading
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass
from typing import Dict, List, Optional

from ..api.types import (
    ConfigError,
    GpuConfig,
    OpaqueConfig,
    PartitionConfig,
    SHARED_COMPUTE,
    TIME_SLICING,
    decode_config,
    select_config_for_request,
)
from ..cdi.handler import CDIHandler
from ..cdi.spec import ContainerEdits
from ..hal.base import DeviceLib
from ..hal.model import AllocatableDevice
from ..partition.manager import (
    PartitionManager,
    RepartitionFailed,
    RepartitionRefused,
)
from ..sharing.shared import SharedComputeManager
from ..sharing.timeslice import TimeSlicingManager
from .checkpoint import CheckpointStore, PreparedClaim, PreparedDevice

log = logging.getLogger(__name__)

DRIVER_NAME = "gpu.amd.com"

#: canonical partition device name: gpu-<index>-<mode>-<pid>
_PARTITION_NAME_RE = re.compile(r"^gpu-(\d+)-([a-z]+)-(\d+)$")


class PrepareError(RuntimeError):
    pass


class _RefLock:
    """A lock plus a waiter/holder refcount (guarded by the registry lock)."""

    __slots__ = ("lock", "refs")

    def __init__(self) -> None:
        self.lock = threading.Lock()
        self.refs = 0


@dataclass
class _ClaimInfo:
    uid: str
    namespace: str
    name: str


def _parse_claim_meta(claim: dict) -> _ClaimInfo:
    meta = claim.get("metadata") or {}
    uid = meta.get("uid")
    if not uid:
        raise PrepareError("claim has no metadata.uid")
    return _ClaimInfo(uid=uid, namespace=meta.get("namespace", ""), name=meta.get("name", ""))


class DeviceState:
    def __init__(
        self,
        lib: DeviceLib,
        cdi: CDIHandler,
        checkpoints: CheckpointStore,
        *,
        pool_name: str,
        ts_manager: Optional[TimeSlicingManager] = None,
        shared_manager: Optional[SharedComputeManager] = None,
        partition_manager: Optional[PartitionManager] = None,
    ):
        self.lib = lib
        self.cdi = cdi
        self.checkpoints = checkpoints
        self.pool_name = pool_name
        self.ts_manager = ts_manager or TimeSlicingManager(lib)
        self.shared_manager = shared_manager
        self.partition_manager = partition_manager or PartitionManager(
            lib, in_use_fn=self.claims_holding_gpu
        )

        #: optional callback fired after the allocatable set changes
        #: (repartition) — the Driver republishes ResourceSlices from it.
        self.on_allocatable_change = None
        #: optional callback(claim_info, reason, message) for user-facing
        #: Warning events (e.g. advisory time-slicing); wired by Driver
        self.on_warning = None
        #: optional callback per performed mode switch (metrics)
        self.on_repartition = None
        #: optional callback(count) when the deferred-restore set changes
        self.on_deferred_restores_change = None

        self._registry_lock = threading.Lock()
        self._claim_locks: Dict[str, "_RefLock"] = {}
        #: overlaps the claim CDI-spec write with the checkpoint write
        self._write_pool = ThreadPoolExecutor(
            max_workers=4, thread_name_prefix="cdi-write"
        )
        #: gpu_index -> set of claim uids with prepared devices on it
        self._gpu_holders: Dict[int, set] = {}
        #: gpu_index -> (compute, memory) restore that was refused while
        #: other claims held the GPU; retried when the GPU drains
        self._deferred_restores: Dict[int, tuple] = {}
        #: canonical name -> AllocatableDevice
        self._allocatable: Dict[str, AllocatableDevice] = {}
        self.refresh_allocatable()
        self._recover()

    # ------------------------------------------------------------------
    # allocatable snapshot
    # ------------------------------------------------------------------
    def refresh_allocatable(self) -> None:
        """Re-enumerate hardware; called at startup and after repartition
        (the reference requires a plugin restart for this)."""
        devices: Dict[str, AllocatableDevice] = {}
        for gpu in self.lib.enumerate():
            if gpu.partitions:
                for p in gpu.partitions:
                    d = AllocatableDevice.from_partition(gpu, p)
                    devices[d.canonical_name] = d
            else:
                d = AllocatableDevice.from_gpu(gpu)
                devices[d.canonical_name] = d
        with self._registry_lock:
            self._allocatable = devices
        # Publisher fingerprints the device set, so an unchanged snapshot
        # costs no API calls.
        if self.on_allocatable_change is not None:
            self.on_allocatable_change()

    def close(self) -> None:
        """Release the write pool (Driver.shutdown calls this)."""
        self._write_pool.shutdown(wait=True)

    def allocatable_devices(self) -> List[AllocatableDevice]:
        with self._registry_lock:
            return list(self._allocatable.values())

    def write_base_cdi_spec(self) -> str:
        return self.cdi.create_standard_spec(self.allocatable_devices())

    # ------------------------------------------------------------------
    # recovery (crash-safe resume; reference device_state.go:94-125)
    # ------------------------------------------------------------------
    def _recover(self) -> None:
        recovered = self.checkpoints.list_all()
        #: claims whose checkpointed devices no longer exist on the node
        #: (hardware/partition drift while the plugin was down) — the
        #: stale-resume gap the reference leaves unhandled (SURVEY §5.4:
        #: checkpoints are never re-validated against live hardware).
        #: They are kept (their pods may still run) but flagged for
        #: operators and the health/metrics surface.
        self.stale_claims: Dict[str, List[str]] = {}
        with self._registry_lock:
            live_names = set(self._allocatable)
        for uid, pc in recovered.items():
            # Claim CDI specs are written without fsync (regenerable);
            # after a power-loss reboot rebuild any missing ones here so
            # containerd can start the claim's containers again without
            # waiting for a kubelet re-prepare.
            try:
                self._ensure_claim_spec(pc)
            except Exception:
                log.exception("claim %s: CDI spec regeneration failed", uid)
            missing = [
                d.device_name
                for d in pc.devices
                if d.device_name not in live_names
            ]
            if missing:
                self.stale_claims[uid] = missing
                log.warning(
                    "recovered claim %s references device(s) %s that no "
                    "longer exist (partition/hardware drift while the "
                    "plugin was down); claim kept, flagged stale",
                    uid,
                    missing,
                )
            for dev in pc.devices:
                if dev.parent_gpu_index >= 0 and not dev.admin:
                    self._gpu_holders.setdefault(dev.parent_gpu_index, set()).add(uid)
            # Re-register shared sessions so CU-range bookkeeping survives
            # a plugin restart (stale-state gap the reference leaves open,
            # SURVEY.md §5.4).
            if pc.sharing_strategy == SHARED_COMPUTE and self.shared_manager:
                from ..sharing.shared import SharedSession

                spec_uids = set(self.cdi.list_claim_spec_uids())
                if uid in spec_uids:
                    # claim_env carries the checkpointed HSA_CU_MASK entries;
                    # recover_session parses them back into CU-range
                    # bookkeeping so a post-restart SharedCompute claim on the
                    # same GPU cannot be handed an overlapping CU slice.
                    self.shared_manager.recover_session(
                        SharedSession(
                            session_id=pc.shared_session_id or uid[:36],
                            claim_uid=uid,
                            shm_dir="",
                            env=list(pc.claim_env),
                            mounts=[],
                            gpu_indices=[
                                d.parent_gpu_index for d in pc.devices
                            ],
                        )
                    )
        if recovered:
            log.info("recovered %d prepared claim(s) from checkpoints", len(recovered))

    # ------------------------------------------------------------------
    # locking
    # ------------------------------------------------------------------
    @contextlib.contextmanager
    def _claim_lock(self, uid: str):
        """Refcounted per-claim mutex.

        Entries are GC'd only when no thread holds or waits on them, so a
        kubelet retry racing an unprepare can never mint a second lock for
        the same claim and run two operations concurrently (the
        pop-while-waiters-blocked race of the old ``pop`` on unprepare).
        """
        with self._registry_lock:
            rl = self._claim_locks.setdefault(uid, _RefLock())
            rl.refs += 1
        try:
            with rl.lock:
                yield
        finally:
            with self._registry_lock:
                rl.refs -= 1
                if rl.refs == 0 and self._claim_locks.get(uid) is rl:
                    del self._claim_locks[uid]

    def claims_holding_gpu(self, gpu_index: int) -> List[str]:
        with self._registry_lock:
            return sorted(self._gpu_holders.get(gpu_index, set()))

    # ------------------------------------------------------------------
    # prepare
    # ------------------------------------------------------------------
    def prepare(self, claim: dict) -> List[dict]:
        """Prepare one ResourceClaim; returns kubelet Device dicts
        (request_names/pool_name/device_name/cdi_device_ids)."""
        info = _parse_claim_meta(claim)
        with self._claim_lock(info.uid):
            cached = self.checkpoints.read(info.uid)
            if cached is not None:
                self._ensure_claim_spec(cached)
                return [self._to_kubelet_device(d) for d in cached.devices]

            results, configs = self._parse_allocation(claim)
            prepared = self._prepare_devices(info, results, configs)
            try:
                self.checkpoints.write(prepared)
                fut = getattr(prepared, "_cdi_write", None)
                if fut is not None:
                    fut.result()  # join the overlapped claim-spec write
            except BaseException:
                self._rollback(prepared, info.uid)
                raise
            with self._registry_lock:
                for dev in prepared.devices:
                    # adminAccess (monitoring) claims neither block
                    # repartition drains nor count as exclusive holders
                    if dev.parent_gpu_index >= 0 and not dev.admin:
                        self._gpu_holders.setdefault(
                            dev.parent_gpu_index, set()
                        ).add(info.uid)
            return [self._to_kubelet_device(d) for d in prepared.devices]

    def _parse_allocation(self, claim: dict):
        status = claim.get("status") or {}
        allocation = status.get("allocation")
        if not allocation:
            raise PrepareError("claim has no status.allocation")
        devices = allocation.get("devices") or {}
        results = [
            r
            for r in devices.get("results") or []
            if r.get("driver") == DRIVER_NAME
        ]
        if not results:
            raise PrepareError(
                f"no allocation results for driver {DRIVER_NAME}"
            )
        # Opaque config decode, class-config < claim-config precedence
        # (reference device_state.go:457-510). Defaults are prepended with
        # lowest precedence (:210-221).
        configs: List[OpaqueConfig] = [
            OpaqueConfig("default", [], GpuConfig().normalize())
        ]
        for c in devices.get("config") or []:
            opaque = c.get("opaque") or {}
            if opaque.get("driver") != DRIVER_NAME:
                continue
            source = "claim" if c.get("source") == "FromClaim" else "class"
            try:
                cfg = decode_config(opaque.get("parameters") or {})
                cfg.normalize()
                cfg.validate()
            except ConfigError as e:
                raise PrepareError(f"invalid opaque config ({source}): {e}") from e
            configs.append(OpaqueConfig(source, list(c.get("requests") or []), cfg))
        return results, configs

    def _prepare_devices(
        self,
        info: _ClaimInfo,
        results: List[dict],
        configs: List[OpaqueConfig],
    ) -> PreparedClaim:
        prepared = PreparedClaim(
            claim_uid=info.uid, namespace=info.namespace, name=info.name
        )

        # --- resolve devices, honoring partition intent --------------------
        # PartitionConfig on a whole-GPU result repartitions that GPU as part
        # of Prepare (dynamic MIG analog the reference shipped disabled).
        repartition_done = False
        try:
            for r in results:
                req = r.get("request", "")
                pcfg = select_config_for_request(req, configs, PartitionConfig)
                if pcfg is None:
                    continue
                dev = self._find_device(r["device"])
                if dev is None or dev.kind != "gpu":
                    continue
                gpu_index = dev.parent_gpu.index
                try:
                    cur = dev.parent_gpu
                    switched = self.partition_manager.ensure_mode(
                        gpu_index,
                        pcfg.compute_partition,
                        pcfg.memory_partition,
                        requesting_claim=info.uid,
                        allow_dynamic=pcfg.allow_dynamic_repartition,
                    )
                except RepartitionRefused as e:
                    raise PrepareError(str(e)) from e
                except RepartitionFailed as e:
                    self._note_failed_switch(gpu_index, e)
                    raise PrepareError(str(e)) from e
                except Exception as e:
                    # HAL failure mid-switch: surface typed, and let the
                    # outer rollback undo any PRIOR switch of this claim
                    raise PrepareError(
                        f"repartition of gpu-{gpu_index} failed: {e}"
                    ) from e
                if switched:
                    if self.on_repartition is not None:
                        self.on_repartition()
                    prepared.repartitioned[str(gpu_index)] = [
                        cur.compute_partition,
                        cur.memory_partition,
                        pcfg.compute_partition,
                        pcfg.memory_partition,
                    ]
                    repartition_done = True
            # Scheduler-driven carve (DRA partitionable devices): an
            # allocation may name a PROSPECTIVE partition device (published
            # with sharedCounters before any carve). If the device doesn't
            # exist yet but its name parses as a partition of a known GPU,
            # carve that GPU now — the dynamic-MIG flow the reference
            # shipped disabled (nvlib.go:560-669), scheduler-driven.
            if self._auto_carve_for_results(info, results, prepared):
                repartition_done = True
        except BaseException:
            # undo any mode switch this claim already performed (a claim
            # spanning several GPUs can fail on the second switch) and
            # re-sync publication if hardware state moved
            if prepared.repartitioned:
                self._rollback(prepared, info.uid)
            raise
        if repartition_done:
            self.refresh_allocatable()
            self.write_base_cdi_spec()

        try:
            return self._prepare_after_partition(info, results, configs, prepared)
        except BaseException:
            # a failure past a successful mode switch must not leak it
            self._rollback(prepared, info.uid)
            raise

    def _auto_carve_for_results(
        self, info: _ClaimInfo, results: List[dict], prepared: PreparedClaim
    ) -> bool:
        from ..partition.catalog import preferred_memory_mode

        changed = False
        for r in results:
            name = r.get("device", "")
            if self._find_device(name) is not None:
                continue
            m = _PARTITION_NAME_RE.match(name)
            if not m:
                continue
            gpu_index = int(m.group(1))
            mode = m.group(2).upper()
            gpu = next(
                (g for g in self.lib.enumerate() if g.index == gpu_index),
                None,
            )
            if gpu is None or gpu.compute_partition == mode:
                continue  # unknown GPU, or carved but pid out of range
            mem = preferred_memory_mode(mode, gpu.nps_caps)
            try:
                switched = self.partition_manager.ensure_mode(
                    gpu_index,
                    mode,
                    mem,
                    requesting_claim=info.uid,
                    allow_dynamic=True,
                )
            except RepartitionRefused as e:
                raise PrepareError(
                    f"allocated device {name!r} requires carving "
                    f"gpu-{gpu_index} to {mode}: {e}"
                ) from e
            except RepartitionFailed as e:
                self._note_failed_switch(gpu_index, e)
                raise PrepareError(
                    f"auto-carve of gpu-{gpu_index} to {mode} failed: {e}"
                ) from e
            except Exception as e:
                raise PrepareError(
                    f"auto-carve of gpu-{gpu_index} to {mode} failed: {e}"
                ) from e
            if switched:
                if self.on_repartition is not None:
                    self.on_repartition()
                prepared.repartitioned.setdefault(
                    str(gpu_index),
                    [
                        gpu.compute_partition,
                        gpu.memory_partition,
                        mode,
                        mem,
                    ],
                )
                log.info(
                    "claim %s: auto-carved gpu-%d to %s/%s for "
                    "scheduler-allocated partition %s",
                    info.uid,
                    gpu_index,
                    mode,
                    mem,
                    name,
                )
                changed = True
        return changed

    def _prepare_after_partition(
        self,
        info: _ClaimInfo,
        results: List[dict],
        configs: List[OpaqueConfig],
        prepared: PreparedClaim,
    ) -> PreparedClaim:
        # --- group results by sharing config -------------------------------
        per_result_dev: List[tuple] = []
        for r in results:
            name = r.get("device", "")
            dev = self._find_device(name)
            if dev is None:
                # A whole-GPU result whose GPU we just partitioned resolves
                # to ALL its partitions (the claim holds the whole die).
                parts = self._partitions_of_gpu_name(name)
                if not parts:
                    raise PrepareError(
                        f"allocated device {name!r} not found on this node "
                        f"(ResourceSlice drift? plugin will republish)"
                    )
                for p in parts:
                    per_result_dev.append((r, p))
            else:
                per_result_dev.append((r, dev))

        # --- sharing --------------------------------------------------------
        shared_edits: Optional[ContainerEdits] = None
        gcfg_by_dev: List[tuple] = []
        strategies = set()
        for r, dev in per_result_dev:
            gcfg = select_config_for_request(r.get("request", ""), configs, GpuConfig)
            gcfg_by_dev.append((gcfg, dev))
            if gcfg and gcfg.sharing:
                strategies.add(gcfg.sharing.strategy)

        if SHARED_COMPUTE in strategies:
            if self.shared_manager is None:
                raise PrepareError("SharedCompute requested but supervisor disabled")
            sc_devices = [
                dev
                for gcfg, dev in gcfg_by_dev
                if gcfg and gcfg.sharing and gcfg.sharing.strategy == SHARED_COMPUTE
            ]
            settings = next(
                gcfg.sharing.shared_compute
                for gcfg, _ in gcfg_by_dev
                if gcfg and gcfg.sharing and gcfg.sharing.strategy == SHARED_COMPUTE
            )
            try:
                session = self.shared_manager.start_session(
                    info.uid, sc_devices, settings
                )
            except Exception as e:
                raise PrepareError(f"shared-compute session failed: {e}") from e
            prepared.sharing_strategy = SHARED_COMPUTE
            prepared.shared_session_id = session.session_id
            shared_edits = session.container_edits()

        # Group time-sliced devices by their settings: two requests in one
        # claim may carry different intervals, and collapsing them to the
        # first match would silently mis-apply (round-1 "weak" finding).
        # A genuine conflict — two intervals for the SAME parent GPU — is
        # rejected rather than resolved arbitrarily.
        ts_by_quantum: Dict[int, tuple] = {}
        gpu_interval: Dict[int, str] = {}
        for gcfg, dev in gcfg_by_dev:
            if not (
                gcfg
                and gcfg.sharing
                and gcfg.sharing.strategy == TIME_SLICING
                and gcfg.sharing.time_slicing.interval != "Default"
            ):
                continue
            ts = gcfg.sharing.time_slicing
            idx = dev.parent_gpu.index
            if gpu_interval.get(idx, ts.interval) != ts.interval:
                raise PrepareError(
                    f"conflicting TimeSlicing intervals for gpu-{idx} in one "
                    f"claim ({gpu_interval[idx]} vs {ts.interval})"
                )
            gpu_interval[idx] = ts.interval
            entry = ts_by_quantum.setdefault(ts.quantum_us, (ts, []))
            entry[1].append(dev)
        if ts_by_quantum:
            for settings, devs in ts_by_quantum.values():
                try:
                    prepared.timeslice_gpus.extend(
                        self.ts_manager.set_timeslice(devs, settings)
                    )
                except Exception as e:
                    # _rollback (invoked by the caller) undoes the session
                    raise PrepareError(f"time-slicing failed: {e}") from e
            if not prepared.sharing_strategy:
                prepared.sharing_strategy = TIME_SLICING
            if not self.lib.timeslice_effective():
                # Surface the platform gap instead of silently reporting
                # success: this hardware has no runtime
                # scheduler-quantum control, so the interval is advisory.
                msg = (
                    "TimeSlicing interval(s) "
                    f"{sorted(set(gpu_interval.values()))} accepted but "
                    "ADVISORY on this node: amdgpu exposes no runtime "
                    "scheduler-quantum control (timeSlicingEffective=false "
                    "on the published devices); HSA default queue "
                    "multiplexing applies"
                )
                log.warning("claim %s: %s", info.uid, msg)
                if self.on_warning is not None:
                    try:
                        self.on_warning(info, "TimeSlicingAdvisory", msg)
                    except Exception:
                        log.exception("warning callback failed")

        # --- CDI claim spec -------------------------------------------------
        claim_edits = ContainerEdits(
            env=[f"AMD_DRA_CLAIM_UID={info.uid}"]
        )
        if shared_edits is not None:
            claim_edits = claim_edits.merge(shared_edits)
        prepared.claim_env = list(claim_edits.env)
        prepared.claim_mounts = [m.to_json() for m in claim_edits.mounts]
        device_names = [dev.canonical_name for _, dev in per_result_dev]
        # Overlap the claim-spec write with building the response and the
        # checkpoint written by the caller: the spec is regenerable from
        # the checkpoint (see prepare()'s cache-hit path), so ordering is
        # no longer a crash-safety requirement. The future rides on the
        # (per-claim) prepared object; prepare() joins it. The spec is no
        # longer fsynced, but its native write runs with the GIL released
        # and still overlaps: on an MI355X node the handoff measured 3-5%
        # more pods/s than the same call made inline
        # (profiles/claimio_r03.md).
        prepared._cdi_write = self._write_pool.submit(
            self.cdi.create_claim_spec, info.uid, device_names, claim_edits
        )

        # --- response -------------------------------------------------------
        for r, dev in per_result_dev:
            prepared.devices.append(
                PreparedDevice(
                    request_names=[r["request"]] if r.get("request") else [],
                    pool_name=self.pool_name,
                    device_name=dev.canonical_name,
                    cdi_device_ids=[
                        self.cdi.device_id(dev.canonical_name),
                        self.cdi.claim_device_id(info.uid, dev.canonical_name),
                    ],
                    parent_gpu_index=dev.parent_gpu.index,
                    kind=dev.kind,
                    device_uuid=dev.uuid,
                    admin=bool(r.get("adminAccess")),
                )
            )
        return prepared

    def _rollback(self, prepared: PreparedClaim, claim_uid: str) -> None:
        """Best-effort undo of a partially-prepared claim: stop the shared
        session, restore time-slice defaults, revert any mode switch, and
        drop on-disk artifacts — so a failed Prepare leaves the node as it
        found it (kubelet will retry from scratch)."""
        try:
            if prepared.shared_session_id and self.shared_manager:
                self.shared_manager.stop_session(prepared.shared_session_id)
            if prepared.timeslice_gpus:
                self.ts_manager.restore_default(prepared.timeslice_gpus)
            reverted = False
            for gpu_index_s, modes in prepared.repartitioned.items():
                try:
                    if self.partition_manager.ensure_mode(
                        int(gpu_index_s),
                        modes[0],
                        modes[1],
                        requesting_claim=claim_uid,
                        allow_dynamic=True,
                    ):
                        reverted = True
                except RepartitionRefused as e:
                    log.warning(
                        "rollback: leaving gpu-%s partitioned (%s)",
                        gpu_index_s,
                        e,
                    )
                except Exception as e:
                    # revert itself failed (transient HAL error): remember
                    # the target mode and retry when the GPU drains
                    self._deferred_restores.setdefault(
                        int(gpu_index_s), (modes[0], modes[1])
                    )
                    self._notify_deferred()
                    reverted = True  # hardware may have moved: re-sync
                    log.warning(
                        "rollback: revert of gpu-%s failed (%s); restore "
                        "deferred",
                        gpu_index_s,
                        e,
                    )
            if reverted:
                self.refresh_allocatable()
                self.write_base_cdi_spec()
            self.cdi.delete_claim_spec(claim_uid)
            self.checkpoints.delete(claim_uid)
        except Exception:
            log.exception("rollback of claim %s incomplete", claim_uid)

    def _ensure_claim_spec(self, pc: PreparedClaim) -> None:
        """Regenerate the claim CDI spec if a crash between the overlapped
        writes (or manual deletion) left it missing."""
        path = self.cdi._claim_spec_path(pc.claim_uid)
        if os.path.exists(path):
            return
        from ..cdi.spec import Mount

        edits = ContainerEdits(
            env=list(pc.claim_env),
            mounts=[
                Mount(
                    host_path=m["hostPath"],
                    container_path=m["containerPath"],
                    options=list(m.get("options") or []),
                )
                for m in pc.claim_mounts
            ],
        )
        self.cdi.create_claim_spec(
            pc.claim_uid, [d.device_name for d in pc.devices], edits
        )

    def _find_device(self, name: str) -> Optional[AllocatableDevice]:
        with self._registry_lock:
            return self._allocatable.get(name)

    def _partitions_of_gpu_name(self, gpu_name: str) -> List[AllocatableDevice]:
        with self._registry_lock:
            return [
                d
                for d in self._allocatable.values()
                if d.kind == "partition"
                and d.canonical_name.startswith(gpu_name + "-")
            ]

    @staticmethod
    def _to_kubelet_device(d: PreparedDevice) -> dict:
        return {
            "request_names": list(d.request_names),
            "pool_name": d.pool_name,
            "device_name": d.device_name,
            "cdi_device_ids": list(d.cdi_device_ids),
        }

    # ------------------------------------------------------------------
    # unprepare
    # ------------------------------------------------------------------
    def unprepare(self, claim_uid: str) -> None:
        """Idempotent unprepare (reference device_state.go:161-190)."""
        with self._claim_lock(claim_uid):
            pc = self.checkpoints.read(claim_uid)
            if pc is None:
                # unknown claim: no-op (:171-173) — but still sweep any
                # deferred mode restores (a concurrent batch drain can
                # leave one pending with no further real unprepare)
                if self._deferred_restores and self._retry_deferred_restores(
                    claim_uid
                ):
                    self.refresh_allocatable()
                    self.write_base_cdi_spec()
                return

            if pc.sharing_strategy == SHARED_COMPUTE and self.shared_manager:
                self.shared_manager.stop_session(pc.shared_session_id or claim_uid[:36])
            if pc.timeslice_gpus:
                self.ts_manager.restore_default(pc.timeslice_gpus)

            # Release holdership BEFORE attempting mode restore so our own
            # claim does not block the drain check.
            with self._registry_lock:
                for holders in self._gpu_holders.values():
                    holders.discard(claim_uid)

            restored = False
            for gpu_index_s, modes in pc.repartitioned.items():
                prev_c, prev_m = modes[0], modes[1]
                try:
                    if self.partition_manager.ensure_mode(
                        int(gpu_index_s),
                        prev_c,
                        prev_m,
                        requesting_claim=claim_uid,
                        allow_dynamic=True,
                    ):
                        restored = True
                        if self.on_repartition is not None:
                            self.on_repartition()
                except RepartitionRefused as e:
                    # other claims still hold partitions of this GPU;
                    # remember the restore and retry when it drains
                    self._deferred_restores[int(gpu_index_s)] = (
                        prev_c,
                        prev_m,
                    )
                    self._notify_deferred()
                    log.warning(
                        "leaving gpu-%s partitioned for now (%s); restore "
                        "deferred until the GPU drains",
                        gpu_index_s,
                        e,
                    )
            if self._retry_deferred_restores(claim_uid):
                restored = True
            if restored:
                self.refresh_allocatable()
                self.write_base_cdi_spec()

            self.cdi.delete_claim_spec(claim_uid)
            self.checkpoints.delete(claim_uid)

    def _note_failed_switch(self, gpu_index: int, e: RepartitionFailed) -> None:
        """A mode switch died mid-sequence. If the manager's revert did
        not restore the original mode, remember it as a deferred restore
        (retried on every unprepare) and re-sync publication with the
        actual hardware state."""
        if not e.reverted:
            self._deferred_restores.setdefault(gpu_index, e.original)
            self._notify_deferred()
            self.refresh_allocatable()
            self.write_base_cdi_spec()

    def _notify_deferred(self) -> None:
        if self.on_deferred_restores_change is not None:
            try:
                self.on_deferred_restores_change(len(self._deferred_restores))
            except Exception:
                pass

    def _retry_deferred_restores(self, requesting_claim: str) -> bool:
        """Apply deferred mode restores for GPUs that have drained (the
        last pod of a scheduler-carved GPU left: return it to SPX so the
        whole-GPU device becomes allocatable again)."""
        restored = False
        for gpu_index in list(self._deferred_restores):
            if self.claims_holding_gpu(gpu_index):
                continue
            prev_c, prev_m = self._deferred_restores[gpu_index]
            try:
                if self.partition_manager.ensure_mode(
                    gpu_index,
                    prev_c,
                    prev_m,
                    requesting_claim=requesting_claim,
                    allow_dynamic=True,
                ):
                    restored = True
                    if self.on_repartition is not None:
                        self.on_repartition()
                    log.info(
                        "gpu-%d drained: deferred restore to %s/%s applied",
                        gpu_index,
                        prev_c,
                        prev_m,
                    )
                del self._deferred_restores[gpu_index]
                self._notify_deferred()
            except Exception:
                pass  # raced a new prepare or transient HAL failure:
                      # keep the entry, retried on the next unprepare
        return restored
