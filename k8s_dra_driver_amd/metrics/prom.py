"""Prometheus metrics for the plugin's prepare hot path.

The reference exposes metrics only on the controller; the plugin — whose
latency IS the north-star metric — has none (SURVEY.md §5.5 calls this a
gap to fix). Metrics are registry-scoped so tests and multi-instance
benches never collide on the global default registry.
"""

from __future__ import annotations

import contextlib
import time
from typing import Optional

from prometheus_client import (
    CollectorRegistry,
    Counter,
    Gauge,
    Histogram,
    start_http_server,
)

_BUCKETS = (
    0.0005,
    0.001,
    0.0025,
    0.005,
    0.01,
    0.025,
    0.05,
    0.1,
    0.25,
    0.5,
    1.0,
    2.5,
    5.0,
)


class PluginMetrics:
    def __init__(self, registry: Optional[CollectorRegistry] = None):
        self.registry = registry or CollectorRegistry()
        self.prepare_seconds = Histogram(
            "dra_prepare_seconds",
            "NodePrepareResources per-claim latency",
            buckets=_BUCKETS,
            registry=self.registry,
        )
        self.unprepare_seconds = Histogram(
            "dra_unprepare_seconds",
            "NodeUnprepareResources per-claim latency",
            buckets=_BUCKETS,
            registry=self.registry,
        )
        self.prepared_claims = Counter(
            "dra_prepared_claims_total",
            "Successfully prepared claims",
            registry=self.registry,
        )
        self.prepare_errors = Counter(
            "dra_prepare_errors_total",
            "Failed claim preparations",
            registry=self.registry,
        )
        self.unprepare_errors = Counter(
            "dra_unprepare_errors_total",
            "Failed claim unpreparations",
            registry=self.registry,
        )
        self.allocatable_devices = Gauge(
            "dra_allocatable_devices",
            "Devices currently published in ResourceSlices",
            registry=self.registry,
        )
        self.repartitions = Counter(
            "dra_repartitions_total",
            "Dynamic partition mode switches performed",
            registry=self.registry,
        )
        self.isolation_violations = Counter(
            "dra_shared_isolation_violations_total",
            "Shared-GPU processes caught with stripped/altered CU masks",
            registry=self.registry,
        )
        self.slice_heals = Counter(
            "dra_resourceslice_heals_total",
            "ResourceSlice republications triggered by external drift",
            registry=self.registry,
        )
        self.deferred_restores = Gauge(
            "dra_deferred_mode_restores",
            "GPUs whose partition-mode restore is pending a drain",
            registry=self.registry,
        )

        # Passive health signals (set by the health monitor's poll, never
        # on the prepare path). An unsupported signal exports no sample.
        self.gpu_ecc_errors = Gauge(
            "dra_gpu_ecc_errors",
            "Accumulated ECC error count since the amdgpu driver loaded",
            ["gpu", "kind"],
            registry=self.registry,
        )
        self.gpu_bad_pages = Gauge(
            "dra_gpu_bad_pages",
            "Retired (bad) VRAM pages by status",
            ["gpu", "status"],
            registry=self.registry,
        )
        self.gpu_temperature = Gauge(
            "dra_gpu_temperature_celsius",
            "GPU temperature by sensor",
            ["gpu", "sensor"],
            registry=self.registry,
        )
        self.gpu_unhealthy = Gauge(
            "dra_gpu_unhealthy",
            "1 while the GPU is marked unhealthy, labelled with the reason",
            ["gpu", "reason"],
            registry=self.registry,
        )
        self.gpu_health_warnings = Counter(
            "dra_gpu_health_warnings_total",
            "Health warnings raised (warnings never taint a GPU)",
            ["gpu", "reason"],
            registry=self.registry,
        )
        # Startup self-test (Driver.run_startup_selftest)
        self.gpu_selftest_runs = Counter(
            "dra_gpu_selftest_runs_total",
            "Startup self-tests by result "
            "(pass, memory, compute, error, skipped)",
            ["gpu", "result"],
            registry=self.registry,
        )
        self.gpu_selftest_seconds = Gauge(
            "dra_gpu_selftest_seconds",
            "Wall time of the GPU's last startup self-test",
            ["gpu"],
            registry=self.registry,
        )
        # its per-CU stage, set only when that stage ran
        self.gpu_selftest_cus_covered = Gauge(
            "dra_gpu_selftest_cus_covered",
            "Compute units the last per-CU startup self-test ran on",
            ["gpu"],
            registry=self.registry,
        )
        self.gpu_selftest_cus_bad = Gauge(
            "dra_gpu_selftest_cus_bad",
            "Compute units with an LDS or MFMA mismatch in the last per-CU "
            "startup self-test",
            ["gpu"],
            registry=self.registry,
        )
        # its load stage, set only when that stage ran
        self.gpu_selftest_load_iterations = Gauge(
            "dra_gpu_selftest_load_iterations",
            "GEMM iterations the last startup load self-test ran and verified",
            ["gpu"],
            registry=self.registry,
        )
        self.gpu_selftest_load_mismatches = Gauge(
            "dra_gpu_selftest_load_mismatches",
            "Mismatching values in the last startup load self-test",
            ["gpu"],
            registry=self.registry,
        )
        # its MX load stages, one series per format that ran
        self.gpu_selftest_mx_iterations = Gauge(
            "dra_gpu_selftest_mx_iterations",
            "Block-scaled GEMM iterations the last startup MX load self-test "
            "ran and verified",
            ["gpu", "format"],
            registry=self.registry,
        )
        self.gpu_selftest_mx_mismatches = Gauge(
            "dra_gpu_selftest_mx_mismatches",
            "Mismatching values in the last startup MX load self-test",
            ["gpu", "format"],
            registry=self.registry,
        )
        # its HBM march, set only when that stage ran
        self.gpu_selftest_hbm_bytes = Gauge(
            "dra_gpu_selftest_hbm_bytes",
            "Bytes of HBM the last startup HBM march covered",
            ["gpu"],
            registry=self.registry,
        )
        self.gpu_selftest_hbm_passes = Gauge(
            "dra_gpu_selftest_hbm_passes",
            "Passes over its whole coverage the last startup HBM march ran",
            ["gpu"],
            registry=self.registry,
        )
        self.gpu_selftest_hbm_mismatches = Gauge(
            "dra_gpu_selftest_hbm_mismatches",
            "Mismatching 64-bit words in the last startup HBM march",
            ["gpu"],
            registry=self.registry,
        )
        #: gpu label -> reason label currently exported as dra_gpu_unhealthy
        self._unhealthy_reason = {}

    @staticmethod
    def _set_or_drop(gauge: Gauge, labels: tuple, value) -> None:
        if value is None:
            try:
                gauge.remove(*labels)
            except KeyError:
                pass
        else:
            gauge.labels(*labels).set(value)

    def observe_health(self, report) -> None:
        """Export one GPU's poll (a plugin.health.PollReport)."""
        gpu = str(report.gpu_index)
        s = report.signals
        if s is not None:
            for kind in ("correctable", "uncorrectable", "deferred"):
                self._set_or_drop(
                    self.gpu_ecc_errors, (gpu, kind), getattr(s, f"ecc_{kind}")
                )
            for status in ("reserved", "pending", "unreservable"):
                self._set_or_drop(
                    self.gpu_bad_pages,
                    (gpu, status),
                    getattr(s, f"bad_pages_{status}"),
                )
            for sensor in ("hotspot", "vram"):
                self._set_or_drop(
                    self.gpu_temperature,
                    (gpu, sensor),
                    getattr(s, f"temp_{sensor}_c"),
                )
        for reason in report.new_warnings:
            self.gpu_health_warnings.labels(gpu, reason).inc()
        reason = (report.primary_reason or "Unknown") if report.unhealthy else ""
        old = self._unhealthy_reason.get(gpu, "")
        if old and old != reason:
            self._set_or_drop(self.gpu_unhealthy, (gpu, old), None)
        if reason:
            self.gpu_unhealthy.labels(gpu, reason).set(1)
            self._unhealthy_reason[gpu] = reason
        else:
            self._unhealthy_reason.pop(gpu, None)

    @contextlib.contextmanager
    def time_prepare(self):
        t0 = time.perf_counter()
        try:
            yield
        finally:
            self.prepare_seconds.observe(time.perf_counter() - t0)

    @contextlib.contextmanager
    def time_unprepare(self):
        t0 = time.perf_counter()
        try:
            yield
        finally:
            self.unprepare_seconds.observe(time.perf_counter() - t0)

    def serve(self, port: int) -> None:
        """Expose /metrics (controller parity: reference main.go:194-214)."""
        start_http_server(port, registry=self.registry)
