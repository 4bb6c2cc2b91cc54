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
import re
import threading
from concurrent.futures import Future, ThreadPoolExecutor
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

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
from ..cdi.spec import ContainerEdits, Mount
from ..hal.base import DeviceLib
from ..hal.model import AllocatableDevice
from ..partition.catalog import preferred_memory_mode
from ..partition.manager import PartitionManager
from ..sharing.shared import SharedComputeManager, SharedSession
from ..sharing.timeslice import TimeSlicingManager
from .checkpoint import CheckpointStore, PreparedClaim, PreparedDevice
from .repartition import PrepareError, RepartitionLedger

log = logging.getLogger(__name__)

DRIVER_NAME = "gpu.amd.com"

#: canonical partition device name: gpu-<index>-<mode>-<pid>
_PARTITION_NAME_RE = re.compile(r"^gpu-(\d+)-([a-z]+)-(\d+)$")


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


def _strategy(gcfg: Optional[GpuConfig]) -> str:
    """The sharing strategy a request's GpuConfig asks for ("" = none)."""
    return gcfg.sharing.strategy if gcfg and gcfg.sharing else ""


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
        #: holders, deferred restores, mode switches; the Driver sets on_* on it
        self.ledger = RepartitionLedger(self.partition_manager, self._resync)

        #: optional callback fired after the allocatable set changes
        #: (repartition) — the Driver republishes ResourceSlices from it.
        self.on_allocatable_change = None
        #: optional callback(claim_info, reason, message) for user-facing
        #: Warning events (e.g. advisory time-slicing); wired by Driver
        self.on_warning = None

        self._registry_lock = threading.Lock()
        self._claim_locks: Dict[str, "_RefLock"] = {}
        #: overlaps the claim CDI-spec write with the checkpoint write
        self._write_pool = ThreadPoolExecutor(
            max_workers=4, thread_name_prefix="cdi-write"
        )
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

    def _resync(self) -> None:
        """Bring publication back in line with hardware that (may have) moved."""
        self.refresh_allocatable()
        self.write_base_cdi_spec()

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
            self.ledger.hold(uid, pc.devices)
        self._recover_shared_sessions(recovered.values())
        if recovered:
            log.info("recovered %d prepared claim(s) from checkpoints", len(recovered))

    def _recover_shared_sessions(self, claims) -> None:
        """Re-register shared sessions so CU-range bookkeeping survives a
        plugin restart (stale-state gap the reference leaves open,
        SURVEY.md §5.4)."""
        shared_claims = [pc for pc in claims if pc.sharing_strategy == SHARED_COMPUTE]
        if not (shared_claims and self.shared_manager):
            return
        # listed once, and only after _recover has regenerated every
        # missing claim spec
        spec_uids = set(self.cdi.list_claim_spec_uids())
        for pc in shared_claims:
            if pc.claim_uid in spec_uids:
                # claim_env carries the checkpointed HSA_CU_MASK entries;
                # recover_session parses them back into CU-range
                # bookkeeping so a post-restart SharedCompute claim on the
                # same GPU cannot be handed an overlapping CU slice.
                self.shared_manager.recover_session(
                    SharedSession(
                        session_id=pc.shared_session_id or pc.claim_uid[:36],
                        claim_uid=pc.claim_uid,
                        shm_dir="",
                        env=list(pc.claim_env),
                        mounts=[],
                        gpu_indices=[d.parent_gpu_index for d in pc.devices],
                    )
                )

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
        return self.ledger.holders(gpu_index)

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
            prepared, spec_write = self._prepare_devices(info, results, configs)
            try:
                self.checkpoints.write(prepared)
                spec_write.result()  # join the overlapped claim-spec write
            except BaseException:
                self._rollback(prepared, info.uid)
                raise
            self.ledger.hold(info.uid, prepared.devices)
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
        self, info: _ClaimInfo, results: List[dict], configs: List[OpaqueConfig]
    ) -> Tuple[PreparedClaim, Future]:
        """Returns the prepared claim and its in-flight claim-spec write."""
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
                cur = dev.parent_gpu
                target = [pcfg.compute_partition, pcfg.memory_partition]
                if self.ledger.switch_for_claim(
                    cur.index, *target, info.uid, allow_dynamic=pcfg.allow_dynamic_repartition
                ):
                    prepared.repartitioned[str(cur.index)] = [
                        cur.compute_partition, cur.memory_partition, *target
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
            self._resync()

        try:
            return prepared, self._prepare_after_partition(info, results, configs, prepared)
        except BaseException:
            # a failure past a successful mode switch must not leak it
            self._rollback(prepared, info.uid)
            raise

    def _auto_carve_for_results(
        self, info: _ClaimInfo, results: List[dict], prepared: PreparedClaim
    ) -> bool:
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
            if self.ledger.switch_for_claim(
                gpu_index, mode, mem, info.uid, allow_dynamic=True, carve_for=name
            ):
                prepared.repartitioned.setdefault(
                    str(gpu_index), [gpu.compute_partition, gpu.memory_partition, mode, mem]
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
    ) -> Future:
        """Sharing, claim spec and response for the resolved devices; fills
        ``prepared`` and returns the in-flight claim-spec write."""
        per_result_dev = self._resolve_devices(results)
        gcfg_by_dev = [
            (select_config_for_request(r.get("request", ""), configs, GpuConfig), dev)
            for r, dev in per_result_dev
        ]
        shared_edits = self._start_shared_compute(info, gcfg_by_dev, prepared)
        self._apply_time_slices(info, gcfg_by_dev, prepared)

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
        # no longer a crash-safety requirement. prepare() joins the
        # returned future. The spec is no longer fsynced, but its native
        # write runs with the GIL released and still overlaps: on an
        # MI355X node the handoff measured 3-5% more pods/s than the same
        # call made inline (profiles/claimio_r03.md).
        spec_write = self._write_pool.submit(
            self.cdi.create_claim_spec, info.uid, device_names, claim_edits
        )
        self._build_response(info, per_result_dev, prepared)
        return spec_write

    def _resolve_devices(self, results: List[dict]) -> List[tuple]:
        """(result, AllocatableDevice) pairs for every allocation result."""
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
                per_result_dev.extend((r, p) for p in parts)
            else:
                per_result_dev.append((r, dev))
        return per_result_dev

    def _start_shared_compute(
        self, info: _ClaimInfo, gcfg_by_dev: List[tuple], prepared: PreparedClaim
    ) -> Optional[ContainerEdits]:
        """One session over the claim's SharedCompute devices -> its edits."""
        shared = [(g, dev) for g, dev in gcfg_by_dev if _strategy(g) == SHARED_COMPUTE]
        if not shared:
            return None
        if self.shared_manager is None:
            raise PrepareError("SharedCompute requested but supervisor disabled")
        try:
            session = self.shared_manager.start_session(
                info.uid, [dev for _, dev in shared], shared[0][0].sharing.shared_compute
            )
        except Exception as e:
            raise PrepareError(f"shared-compute session failed: {e}") from e
        prepared.sharing_strategy = SHARED_COMPUTE
        prepared.shared_session_id = session.session_id
        return session.container_edits()

    def _apply_time_slices(
        self, info: _ClaimInfo, gcfg_by_dev: List[tuple], prepared: PreparedClaim
    ) -> None:
        # Group time-sliced devices by their settings: two requests in one
        # claim may carry different intervals, and collapsing them to the
        # first match would silently mis-apply (round-1 "weak" finding).
        # A genuine conflict — two intervals for the SAME parent GPU — is
        # rejected rather than resolved arbitrarily.
        ts_by_quantum: Dict[int, tuple] = {}
        gpu_interval: Dict[int, str] = {}
        for gcfg, dev in gcfg_by_dev:
            if _strategy(gcfg) != TIME_SLICING:
                continue
            ts = gcfg.sharing.time_slicing
            if ts.interval == "Default":
                continue
            idx = dev.parent_gpu.index
            if gpu_interval.get(idx, ts.interval) != ts.interval:
                raise PrepareError(
                    f"conflicting TimeSlicing intervals for gpu-{idx} in one "
                    f"claim ({gpu_interval[idx]} vs {ts.interval})"
                )
            gpu_interval[idx] = ts.interval
            entry = ts_by_quantum.setdefault(ts.quantum_us, (ts, []))
            entry[1].append(dev)
        if not ts_by_quantum:
            return
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

    def _build_response(
        self, info: _ClaimInfo, per_result_dev: List[tuple], prepared: PreparedClaim
    ) -> None:
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
            self.ledger.revert(prepared.repartitioned, claim_uid)
            self.cdi.delete_claim_spec(claim_uid)
            self.checkpoints.delete(claim_uid)
        except Exception:
            log.exception("rollback of claim %s incomplete", claim_uid)

    def _ensure_claim_spec(self, pc: PreparedClaim) -> None:
        """Regenerate the claim CDI spec if a crash between the overlapped
        writes (or manual deletion) left it missing."""
        if self.cdi.has_claim_spec(pc.claim_uid):
            return
        edits = ContainerEdits(
            env=list(pc.claim_env), mounts=[Mount.from_json(m) for m in pc.claim_mounts]
        )
        self.cdi.create_claim_spec(pc.claim_uid, [d.device_name for d in pc.devices], edits)

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
                if self.ledger.retry_deferred(claim_uid):
                    self._resync()
                return

            if pc.sharing_strategy == SHARED_COMPUTE and self.shared_manager:
                self.shared_manager.stop_session(pc.shared_session_id or claim_uid[:36])
            if pc.timeslice_gpus:
                self.ts_manager.restore_default(pc.timeslice_gpus)

            # releases holdership BEFORE it restores modes and retries
            self.ledger.release(claim_uid, pc.repartitioned)

            self.cdi.delete_claim_spec(claim_uid)
            self.checkpoints.delete(claim_uid)
