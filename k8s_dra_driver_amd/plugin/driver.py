"""Driver: the node-side orchestration behind the DRA gRPC surface.

Reference analog: ``cmd/nvidia-dra-plugin/driver.go`` (NewDriver :40,
NodePrepareResources :96, nodePrepareResource :118). Differences:

- claims in one batch are prepared **concurrently** (the reference holds a
  driver-level mutex so every claim on the node serializes,
  ``driver.go:119`` — SURVEY.md §7 hard-part 5);
- ResourceSlices are republished on allocatable-set changes (repartition),
  not only once at startup (``driver.go:70-84``).

Per-claim failures are reported inside the response map, never as gRPC
errors, exactly like the reference (``driver.go:96-116``).
"""

from __future__ import annotations

import logging
import threading
import time
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass
from typing import Dict, List, Optional

from .. import DRIVER_NAME
from ..cdi.handler import CDIHandler
from ..hal.base import DeviceLib
from ..kube.client import KubeClient, NotFound
from ..kube.resourceslice import ResourceSlicePublisher
from ..metrics.prom import PluginMetrics
from ..sharing.shared import SharedComputeManager
from ..sharing.timeslice import TimeSlicingManager
from ..state.checkpoint import CheckpointStore
from ..state.devicestate import DeviceState, PrepareError

log = logging.getLogger(__name__)


@dataclass
class ClaimRef:
    namespace: str
    name: str
    uid: str


@dataclass
class ClaimResult:
    devices: List[dict]
    error: str = ""


class Driver:
    def __init__(
        self,
        lib: DeviceLib,
        kube: KubeClient,
        *,
        node_name: str,
        cdi_root: str,
        checkpoint_root: str,
        shared_root: Optional[str] = None,
        use_tmpfs: Optional[bool] = None,
        max_concurrent_claims: int = 16,
        metrics: Optional[PluginMetrics] = None,
        device_kinds: Optional[List[str]] = None,
        shared_enforcement: str = "warn",  # off | warn | kill
        gpu_indices: Optional[List[int]] = None,
        rocm_mount: str = "",  # "", "auto", or an explicit host path
        dev_root: str = "",
        prospective_partitions: str = "",  # "" off | "cpx"|"dpx"|"qpx"
    ):
        self.lib = lib
        self.kube = kube
        self.node_name = node_name
        self.metrics = metrics or PluginMetrics()
        # which device kinds to publish ("gpu", "partition") — the
        # reference's --device-classes subsystem gating (driver.go:66,
        # nvlib.go:113-133); None = all.
        self.device_kinds = device_kinds
        # Scope this plugin instance to a subset of the node's GPUs — the
        # nvkind multi-node-simulation analog (reference
        # values.yaml:40-48 maskNvidiaDriverParams splits one box's GPUs
        # across kind workers); also the SCALE bench shape (one plugin
        # per GPU). None = manage all.
        self.gpu_indices = set(gpu_indices) if gpu_indices is not None else None
        # Scheduler-driven dynamic partitioning (DRA partitionable
        # devices, K8s 1.33): publish prospective partitions of this mode
        # with sharedCounters so the default scheduler can allocate them
        # directly; prepare auto-carves on demand (the dynamic-MIG
        # capability the reference shipped disabled, nvlib.go:560-669).
        self.prospective_partitions = prospective_partitions.lower()
        rocm_path = ""
        if rocm_mount:
            from ..cdi.rocmroot import discover_rocm_root

            found = discover_rocm_root(rocm_mount, host_root=dev_root)
            if found:
                rocm_path = found[0]
            elif rocm_mount != "auto":
                raise RuntimeError(
                    f"--rocm-mount {rocm_mount!r}: no ROCm userspace found "
                    "there (need lib/libamdhip64.so* or libhsa-runtime64.so*)"
                )
        cdi = CDIHandler(
            cdi_root=cdi_root, dev_root=dev_root, rocm_mount=rocm_path
        )
        checkpoints = CheckpointStore(checkpoint_root)
        shared = SharedComputeManager(
            root=shared_root or f"{checkpoint_root}/shared", use_tmpfs=use_tmpfs
        )
        self.state = DeviceState(
            lib,
            cdi,
            checkpoints,
            pool_name=node_name,
            ts_manager=TimeSlicingManager(lib),
            shared_manager=shared,
        )
        node_uid = ""
        try:
            node_uid = (self.kube.get_node(node_name).get("metadata") or {}).get(
                "uid", ""
            )
        except Exception:
            pass  # no Node object (tests/bench) -> no owner reference
        self.publisher = ResourceSlicePublisher(
            kube,
            driver_name=DRIVER_NAME,
            node_name=node_name,
            node_uid=node_uid,
        )
        self.publisher.on_heal = self.metrics.slice_heals.inc
        self.state.ledger.on_deferred_restores_change = (
            self.metrics.deferred_restores.set
        )
        self._pool = ThreadPoolExecutor(
            max_workers=max_concurrent_claims, thread_name_prefix="claim"
        )
        # Republish whenever the allocatable set changes (repartition).
        self.state.on_allocatable_change = self.publish_resources
        self.state.ledger.on_repartition = self.metrics.repartitions.inc
        self.state.on_warning = self._emit_claim_warning
        # Failure detection: unhealthy GPUs are pulled from publication
        # (start()ed by main.py; tests drive check_once directly).
        from .health import HealthMonitor

        self.health = HealthMonitor(
            lib,
            on_change=self._on_health_change,
            on_poll=self._on_health_poll,
        )
        #: unhealthy set at the last change (to tell transitions apart)
        self._last_unhealthy: set = set()
        self._health_change_lock = threading.Lock()
        # Out-of-band shared-GPU isolation enforcement (sharing.go:211-221
        # analog): detect containers that stripped/altered their CU mask.
        self.enforcer = None
        if shared_enforcement != "off":
            from ..sharing.enforce import SharedEnforcer

            self.enforcer = SharedEnforcer(
                shared,
                action=shared_enforcement,
                on_violation=self._on_isolation_violation,
            )

    def _on_isolation_violation(self, v) -> None:
        """Surface a shared-GPU isolation violation: metric + Warning
        event on the offending claim (namespace/name from its checkpoint)."""
        self.metrics.isolation_violations.inc()
        pc = self.state.checkpoints.read(v.claim_uid) if v.claim_uid else None
        info = ClaimRef(
            namespace=pc.namespace if pc else "default",
            name=pc.name if pc else v.claim_uid,
            uid=v.claim_uid,
        )
        self._emit_claim_warning(
            info,
            "SharedIsolationViolation",
            f"pid {v.pid}: {v.kind} — {v.detail}"
            + (" (process killed)" if self.enforcer.action == "kill" else ""),
        )

    def _on_health_change(self, unhealthy) -> None:
        """Republish, and tell every claim holding a GPU that just turned
        unhealthy — once per transition, not once per poll."""
        with self._health_change_lock:
            newly = set(unhealthy) - self._last_unhealthy
            self._last_unhealthy = set(unhealthy)
        self.publish_resources()
        for gpu_index in sorted(newly):
            reason = self.health.primary_reason(gpu_index)
            detail = next(
                (
                    f.detail
                    for f in self.health.findings(gpu_index)
                    if f.reason == reason
                ),
                "",
            )
            for uid in self.state.ledger.holders(gpu_index):
                try:
                    pc = self.state.checkpoints.read(uid)
                    info = ClaimRef(
                        namespace=pc.namespace if pc else "default",
                        name=pc.name if pc else uid,
                        uid=uid,
                    )
                    self._emit_claim_warning(
                        info,
                        "DeviceUnhealthy",
                        f"gpu-{gpu_index} is unhealthy"
                        + (f": {reason}" if reason else "")
                        + (f" ({detail})" if detail else ""),
                    )
                except Exception:
                    log.exception("DeviceUnhealthy event for %s failed", uid)

    def _on_health_poll(self, report) -> None:
        self.metrics.observe_health(report)

    # ------------------------------------------------------------------
    def run_startup_selftest(
        self,
        runner=None,
        *,
        mib: int = 1024,
        timeout_s: float = 120.0,
        per_cu: bool = False,
        load_seconds: float = 0,
        load_formats=(),
        hbm_seconds: float = 0,
        hbm_mib: int = 0,
    ) -> Dict[int, str]:
        """Self-test every GPU in scope that nothing is using, one after
        another, and hand the findings to the health monitor. Meant for
        one moment only: between construction and :meth:`startup`, when no
        slice is published and no gRPC server exists, so nothing can start
        using a GPU while it is tested. Returns ``{gpu index: result}``
        with result in pass | memory | compute | error | skipped.
        ``per_cu`` adds the per-CU stage (LDS and matrix pipes of every
        compute unit); only then is the runner called with ``per_cu=True``.
        A positive ``load_seconds`` adds the load stage (a tiled bf16 GEMM
        checked bit for bit for that long); only then is the runner called
        with ``load_seconds``. A non-empty ``load_formats`` (MX format
        names, e.g. ``("mxfp8", "mxfp4")``) runs the load stage again on the
        block-scaled MFMA for each of them; only then is the runner called
        with ``load_formats``. A positive ``hbm_seconds`` adds the HBM march
        as the last stage (all free memory less a reserve, or ``hbm_mib``
        MiB, read, verified and rewritten in place for that long); only then
        is the runner called with ``hbm_seconds``, and with ``hbm_mib`` only
        when that is not 0.

        A GPU is skipped (logged, no finding) when a claim recovered from
        the checkpoints holds it, when it is partitioned, or when it has
        no PCI address to find it by."""
        if runner is None:
            from .. import selftest

            runner = selftest.run
        results: Dict[int, str] = {}
        for gpu in self.lib.enumerate():
            idx = gpu.index
            if self.gpu_indices is not None and idx not in self.gpu_indices:
                continue
            holders = self.state.ledger.holders(idx)
            if holders:
                why = f"held by {len(holders)} recovered claim(s)"
            elif gpu.compute_partition.upper() != "SPX" or gpu.partitions:
                why = f"partitioned ({gpu.compute_partition})"
            elif not gpu.pcie_bdf:
                why = "no PCI address reported"
            else:
                why = ""
            if why:
                log.info("gpu-%d: startup self-test skipped: %s", idx, why)
                results[idx] = "skipped"
                self.metrics.gpu_selftest_runs.labels(str(idx), "skipped").inc()
                continue
            t0 = time.perf_counter()
            extra = {"per_cu": True} if per_cu else {}
            if load_seconds and load_seconds > 0:
                extra["load_seconds"] = load_seconds
            if load_formats:
                extra["load_formats"] = tuple(load_formats)
            if hbm_seconds and hbm_seconds > 0:
                extra["hbm_seconds"] = hbm_seconds
                if hbm_mib:
                    extra["hbm_mib"] = hbm_mib
            cu = load = load_mx = hbm = None
            try:
                res = runner(gpu, mib=mib, timeout_s=timeout_s, **extra)
                outcome, findings = res.outcome, res.findings()
                if per_cu:
                    cu = (res.report or {}).get("cu")
                if "load_seconds" in extra:
                    load = (res.report or {}).get("load")
                if "load_formats" in extra:
                    load_mx = (res.report or {}).get("load_mx")
                if "hbm_seconds" in extra:
                    hbm = (res.report or {}).get("hbm")
            except Exception as e:
                log.exception("gpu-%d: startup self-test failed to run", idx)
                from .health import HealthFinding, SOFT

                outcome = "error"
                findings = [HealthFinding("SelftestError", SOFT, str(e))]
            seconds = time.perf_counter() - t0
            results[idx] = outcome
            self.metrics.gpu_selftest_runs.labels(str(idx), outcome).inc()
            self.metrics.gpu_selftest_seconds.labels(str(idx)).set(seconds)
            if cu:
                self.metrics.gpu_selftest_cus_covered.labels(str(idx)).set(
                    cu["covered"]
                )
                self.metrics.gpu_selftest_cus_bad.labels(str(idx)).set(
                    len(cu["bad_cus"])
                )
            if load:
                self.metrics.gpu_selftest_load_iterations.labels(str(idx)).set(
                    load["iterations"]
                )
                self.metrics.gpu_selftest_load_mismatches.labels(str(idx)).set(
                    load["mismatches"]
                )
            for fmt, part in (load_mx or {}).items():
                self.metrics.gpu_selftest_mx_iterations.labels(str(idx), fmt).set(
                    part["iterations"]
                )
                self.metrics.gpu_selftest_mx_mismatches.labels(str(idx), fmt).set(
                    part["mismatches"]
                )
            if hbm:
                self.metrics.gpu_selftest_hbm_bytes.labels(str(idx)).set(hbm["bytes"])
                self.metrics.gpu_selftest_hbm_passes.labels(str(idx)).set(
                    hbm["passes"]
                )
                self.metrics.gpu_selftest_hbm_mismatches.labels(str(idx)).set(
                    hbm["mismatches"]
                )
            self.health.set_selftest_findings(idx, findings)
            if findings:
                for f in findings:
                    log.error(
                        "gpu-%d: startup self-test: %s: %s", idx, f.reason, f.detail
                    )
            else:
                log.info(
                    "gpu-%d: startup self-test passed in %.1fs%s",
                    idx,
                    seconds,
                    f"; {cu['covered']} of {cu['multi_processor_count']} "
                    "CUs covered"
                    if cu
                    else "",
                )
        self.health.check_once()
        return results

    def startup(self) -> None:
        """Write the base CDI spec and publish ResourceSlices
        (reference main.go:167-206 + driver.go:70-84)."""
        self.state.write_base_cdi_spec()
        self.publish_resources()
        # Watch our slices and republish on external deletion/mutation
        # (resourceslicecontroller.go:407-431 parity).
        self.publisher.start_self_heal()

    def shutdown(self, unpublish: bool = True) -> None:
        if self.enforcer is not None:
            self.enforcer.stop()
        self.publisher.stop_self_heal()
        self._pool.shutdown(wait=True)
        self.state.close()
        if unpublish:
            try:
                self.publisher.unpublish_all()
            except Exception:
                log.exception("unpublish failed")

    def _emit_claim_warning(self, info, reason: str, message: str) -> None:
        """Kubernetes Warning event on the claim (operator visibility for
        platform gaps like advisory time-slicing; best-effort)."""
        self.kube.create_event(
            info.namespace or "default",
            {
                "metadata": {
                    "generateName": f"{(info.name or info.uid)[:40]}-",
                },
                "type": "Warning",
                "reason": reason,
                "message": message,
                "involvedObject": {
                    "apiVersion": "resource.k8s.io/v1beta1",
                    "kind": "ResourceClaim",
                    "namespace": info.namespace,
                    "name": info.name,
                    "uid": info.uid,
                },
                "source": {"component": DRIVER_NAME},
            },
        )

    #: taint applied to devices of unhealthy GPUs on v1beta2+ (DRA device
    #: taints, K8s 1.33): the scheduler stops placing new claims, while
    #: monitoring claims with a matching toleration can still reach the
    #: sick device — richer than unpublishing (the v1beta1 behavior).
    UNHEALTHY_TAINT = {
        "key": "gpu.amd.com/unhealthy",
        "effect": "NoSchedule",
    }

    def _in_scope(self, d, *, include_unhealthy: bool = False) -> bool:
        return (
            (
                include_unhealthy
                or d.parent_gpu.index not in self.health.unhealthy_gpus
            )
            and (self.device_kinds is None or d.kind in self.device_kinds)
            and (
                self.gpu_indices is None
                or d.parent_gpu.index in self.gpu_indices
            )
        )

    def _taints_for(self, d) -> list:
        if d.parent_gpu.index in self.health.unhealthy_gpus:
            taint = dict(self.UNHEALTHY_TAINT)
            reason = self.health.primary_reason(d.parent_gpu.index)
            if reason:
                taint["value"] = reason
            return [taint]
        return []

    def publish_resources(self) -> None:
        # On v1beta2+ unhealthy devices stay published but TAINTED; on
        # v1beta1 (no taints) they are removed as before.
        taint_capable = self.publisher.negotiated_version() != "v1beta1"
        allocatable = [
            d
            for d in self.state.allocatable_devices()
            if self._in_scope(d, include_unhealthy=taint_capable)
        ]
        mode = self.prospective_partitions
        if not mode or (
            self.device_kinds is not None
            and "partition" not in self.device_kinds
        ):
            devices = []
            for d in allocatable:
                dev = d.to_device()
                taints = self._taints_for(d)
                if taints:
                    dev["taints"] = taints
                devices.append(dev)
            self.publisher.publish(devices)
            self.metrics.allocatable_devices.set(len(devices))
            return

        from ..hal.model import (
            consumes_counters,
            gpu_device_with_counters,
            prospective_partition_devices,
            shared_counter_set,
        )
        from ..partition.catalog import make_profile, preferred_memory_mode

        devices, counter_devices, shared_counters = [], [], []
        for d in allocatable:
            gpu = d.parent_gpu
            taints = self._taints_for(d)
            if d.kind == "gpu":
                # uncarved GPU: whole-GPU device + prospective partitions
                # overlapping via the counter set
                shared_counters.append(shared_counter_set(gpu))
                gdev = gpu_device_with_counters(gpu)
                if taints:
                    gdev["taints"] = taints
                devices.append(gdev)
                if taints:
                    continue  # no prospective carves of a sick GPU
                if mode.upper() in gpu.compute_caps and gpu.repartition_capable:
                    try:
                        prof = make_profile(
                            mode.upper(),
                            preferred_memory_mode(mode.upper(), gpu.nps_caps),
                            vram_total_mib=gpu.vram_total_mib or 288 * 1024,
                            cu_count=gpu.cu_count or 256,
                            xcd_count=gpu.xcd_count or 8,
                            nps_caps=gpu.nps_caps,
                        )
                    except ValueError as e:
                        log.warning(
                            "gpu-%d: no valid %s profile (%s); not "
                            "publishing prospective partitions",
                            gpu.index,
                            mode,
                            e,
                        )
                        continue
                    counter_devices.extend(
                        prospective_partition_devices(gpu, prof)
                    )
            else:
                # real (carved) partition: same counter accounting
                if not any(
                    c["name"] == f"{gpu.canonical_name}-counters"
                    for c in shared_counters
                ):
                    shared_counters.append(shared_counter_set(gpu))
                dev = d.to_device()
                dev["consumesCounters"] = consumes_counters(
                    gpu,
                    d.partition.profile.memory_slices_of(
                        d.partition.partition_id
                    ),
                )
                if taints:
                    dev["taints"] = taints
                devices.append(dev)
        self.publisher.publish(
            devices,
            counter_devices=counter_devices,
            shared_counters=shared_counters,
        )
        self.metrics.allocatable_devices.set(len(devices))

    # ------------------------------------------------------------------
    def node_prepare_resources(
        self, claims: List[ClaimRef]
    ) -> Dict[str, ClaimResult]:
        """Batch prepare; one result per claim UID."""
        if not claims:
            return {}
        if len(claims) == 1:  # kubelet's common case: skip pool dispatch
            return {claims[0].uid: self._prepare_one(claims[0])}
        futures = {
            c.uid: self._pool.submit(self._prepare_one, c) for c in claims
        }
        return {uid: f.result() for uid, f in futures.items()}

    def _prepare_one(self, ref: ClaimRef) -> ClaimResult:
        with self.metrics.time_prepare():
            try:
                claim = self.kube.get_resource_claim(ref.namespace, ref.name)
            except NotFound:
                self.metrics.prepare_errors.inc()
                return ClaimResult(
                    [], f"resourceclaim {ref.namespace}/{ref.name} not found"
                )
            except Exception as e:
                self.metrics.prepare_errors.inc()
                return ClaimResult([], f"fetching claim: {e}")
            got_uid = (claim.get("metadata") or {}).get("uid", "")
            if ref.uid and got_uid and got_uid != ref.uid:
                self.metrics.prepare_errors.inc()
                return ClaimResult(
                    [],
                    f"claim {ref.namespace}/{ref.name} UID mismatch: "
                    f"have {got_uid}, prepare was for {ref.uid}",
                )
            try:
                t0 = time.perf_counter()
                devices = self.state.prepare(claim)
                log.debug(
                    "prepared %s/%s uid=%s devices=%d in %.2fms",
                    ref.namespace,
                    ref.name,
                    ref.uid,
                    len(devices),
                    (time.perf_counter() - t0) * 1e3,
                )
            except PrepareError as e:
                self.metrics.prepare_errors.inc()
                self._emit_failure_event(ref, str(e))
                return ClaimResult([], str(e))
            except Exception as e:
                log.exception("prepare %s failed", ref.uid)
                self.metrics.prepare_errors.inc()
                return ClaimResult([], f"internal error preparing claim: {e}")
            self.metrics.prepared_claims.inc()
            return ClaimResult(devices)

    def _emit_failure_event(self, ref: ClaimRef, message: str) -> None:
        """Kubernetes Event on prepare failure (operator visibility the
        reference lacks — failures only surface in kubelet logs there)."""
        try:
            self.kube.create_event(
                ref.namespace,
                {
                    "metadata": {
                        "generateName": "amd-dra-prepare-",
                        "namespace": ref.namespace,
                    },
                    "type": "Warning",
                    "reason": "PrepareFailed",
                    "message": message[:1024],
                    "involvedObject": {
                        "apiVersion": "resource.k8s.io/v1beta1",
                        "kind": "ResourceClaim",
                        "namespace": ref.namespace,
                        "name": ref.name,
                        "uid": ref.uid,
                    },
                    "source": {"component": DRIVER_NAME},
                },
            )
        except Exception:
            log.debug("event emission failed", exc_info=True)

    # ------------------------------------------------------------------
    def cleanup_orphans(self) -> List[str]:
        """Unprepare claims whose ResourceClaim object is gone or has been
        re-created with a new UID — the cleanup the reference leaves as a
        TODO (driver.go:156-168: leaked CDI files / sharing artifacts for
        deleted claims). Returns the UIDs cleaned."""
        cleaned: List[str] = []
        for uid, pc in self.state.checkpoints.list_all().items():
            stale = False
            if not pc.namespace or not pc.name:
                continue
            try:
                cur = self.kube.get_resource_claim(pc.namespace, pc.name)
                if (cur.get("metadata") or {}).get("uid") != uid:
                    stale = True
            except NotFound:
                stale = True
            except Exception:
                continue  # apiserver hiccup: never GC on uncertainty
            if stale:
                try:
                    self.state.unprepare(uid)
                    cleaned.append(uid)
                except Exception:
                    log.exception("orphan cleanup of %s failed", uid)
        # claim CDI specs with no checkpoint (crash between the two writes)
        live = set(self.state.checkpoints.list_all())
        for uid in self.state.cdi.list_claim_spec_uids():
            if uid not in live and uid not in cleaned:
                self.state.cdi.delete_claim_spec(uid)
                cleaned.append(uid)
        if cleaned:
            log.info("cleaned %d orphaned claim(s): %s", len(cleaned), cleaned[:5])
        return cleaned

    def node_unprepare_resources(
        self, claims: List[ClaimRef]
    ) -> Dict[str, ClaimResult]:
        if len(claims) == 1:
            return {claims[0].uid: self._unprepare_one(claims[0])}
        futures = {
            c.uid: self._pool.submit(self._unprepare_one, c) for c in claims
        }
        return {uid: f.result() for uid, f in futures.items()}

    def _unprepare_one(self, ref: ClaimRef) -> ClaimResult:
        with self.metrics.time_unprepare():
            try:
                self.state.unprepare(ref.uid)
            except Exception as e:
                log.exception("unprepare %s failed", ref.uid)
                self.metrics.unprepare_errors.inc()
                return ClaimResult([], f"internal error unpreparing claim: {e}")
            return ClaimResult([])
