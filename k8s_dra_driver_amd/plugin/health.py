"""GPU health monitoring: failure detection + ResourceSlice self-healing.

The reference has no device health path at all — a dead GPU stays
advertised until the plugin restarts (SURVEY.md §5.3 lists only claim-level
retry loops). This monitor:

- polls ``DeviceLib.health_check`` and ``DeviceLib.health_signals`` per GPU
  on an interval (a background thread; never the prepare path),
- turns the passive RAS / thermal signals into findings (:func:`evaluate`),
- on failure, excludes that GPU's devices from publication and republishes
  (scheduler stops placing new claims there),
- on recovery, re-includes them,
- carries the findings of the startup self-test (sticky: they hold until
  they are replaced, see :meth:`HealthMonitor.set_selftest_findings`),
- exposes state for metrics and node conditions.

The signals are the telemetry the amdgpu driver already keeps (ECC counts,
retired pages, temperatures, throttle flags): reading them launches nothing
on the device, so polling is safe while tenants hold the GPU.

The fake HAL's fault injector doubles as the test harness.
"""

from __future__ import annotations

import logging
import threading
from dataclasses import dataclass
from typing import Callable, Dict, List, Optional, Set, Tuple

from ..hal.base import DeviceLib
from ..hal.model import HealthSignals

log = logging.getLogger(__name__)

FATAL = "fatal"
SOFT = "soft"
WARNING = "warning"

#: reasons in policy-table order; within a severity class the earlier one
#: is the primary reason of an unhealthy GPU
REASONS: Tuple[Tuple[str, str], ...] = (
    ("UncorrectableEcc", FATAL),
    ("BadPagesPending", FATAL),
    ("BadPageUnreservable", FATAL),
    ("BadPageThreshold", FATAL),
    # raised by the startup self-test (k8s_dra_driver_amd.selftest)
    ("SelftestMemoryMismatch", FATAL),
    ("SelftestComputeMismatch", FATAL),
    ("ThermalCritical", SOFT),
    # raised by the monitor itself, not by evaluate()
    ("HealthCheckFailed", SOFT),
    ("HealthSignalsError", SOFT),
    ("SelftestError", SOFT),
    ("UncorrectableEccHistoric", WARNING),
    ("CorrectableEccGrowth", WARNING),
    ("DeferredEcc", WARNING),
    ("RetiredPages", WARNING),
    ("Throttled", WARNING),
)
_SEVERITY = dict(REASONS)
_SEVERITY_RANK = {FATAL: 0, SOFT: 1, WARNING: 2}
_REASON_RANK = {r: i for i, (r, _) in enumerate(REASONS)}


@dataclass(frozen=True)
class HealthFinding:
    reason: str
    severity: str  # fatal | soft | warning
    detail: str = ""


def _finding(reason: str, detail: str) -> HealthFinding:
    return HealthFinding(reason, _SEVERITY[reason], detail)


def _sorted(findings: List[HealthFinding]) -> List[HealthFinding]:
    return sorted(
        findings,
        key=lambda f: (_SEVERITY_RANK[f.severity], _REASON_RANK[f.reason]),
    )


def evaluate(
    baseline: Optional[HealthSignals],
    previous: Optional[HealthSignals],
    current: HealthSignals,
) -> List[HealthFinding]:
    """Pure policy: what ``current`` says about one GPU.

    ``baseline`` is the reading of the monitor's first poll, ``previous``
    the poll before this one; either may be ``None`` (nothing to compare
    with yet). A signal that is ``None`` (unsupported) on either side of a
    comparison never produces a finding. Returned in primary-reason order:
    fatal, soft, warning; policy-table order within a class.
    """
    out: List[HealthFinding] = []
    c = current

    ue = c.ecc_uncorrectable
    base_ue = baseline.ecc_uncorrectable if baseline is not None else None
    if ue is not None and base_ue is not None:
        if ue > base_ue:
            out.append(
                _finding(
                    "UncorrectableEcc",
                    f"uncorrectable ECC count {ue} (baseline {base_ue})",
                )
            )
        elif base_ue > 0 and ue > 0:
            out.append(
                _finding(
                    "UncorrectableEccHistoric",
                    f"uncorrectable ECC count {ue} predates monitoring",
                )
            )

    if c.bad_pages_pending:
        out.append(
            _finding(
                "BadPagesPending",
                f"{c.bad_pages_pending} page(s) pending retirement",
            )
        )
    if c.bad_pages_unreservable:
        out.append(
            _finding(
                "BadPageUnreservable",
                f"{c.bad_pages_unreservable} page(s) could not be reserved",
            )
        )
    reserved, threshold = c.bad_pages_reserved, c.bad_page_threshold
    if reserved:
        if threshold is not None and threshold > 0 and reserved >= threshold:
            out.append(
                _finding(
                    "BadPageThreshold",
                    f"{reserved} retired page(s), threshold {threshold}",
                )
            )
        else:
            out.append(
                _finding(
                    "RetiredPages",
                    f"{reserved} retired page(s)"
                    + (
                        f", threshold {threshold}"
                        if threshold
                        else ", threshold not reported"
                    ),
                )
            )

    hot = []
    for label, cur, crit in (
        ("hotspot", c.temp_hotspot_c, c.temp_hotspot_crit_c),
        ("vram", c.temp_vram_c, c.temp_vram_crit_c),
    ):
        if cur is not None and crit is not None and crit > 0 and cur >= crit:
            hot.append(f"{label} {cur:g}C >= critical {crit:g}C")
    if hot:
        out.append(_finding("ThermalCritical", "; ".join(hot)))

    if previous is not None:
        for reason, name, what in (
            ("CorrectableEccGrowth", "ecc_correctable", "correctable"),
            ("DeferredEcc", "ecc_deferred", "deferred"),
        ):
            now, before = getattr(c, name), getattr(previous, name)
            if now is not None and before is not None and now > before:
                out.append(
                    _finding(reason, f"{what} ECC count {before} -> {now}")
                )

    active = c.active_throttles()
    if active:
        out.append(
            _finding(
                "Throttled",
                ", ".join(n[len("throttle_"):] for n in active),
            )
        )
    return _sorted(out)


@dataclass
class PollReport:
    """What one poll saw on one GPU (handed to ``on_poll``)."""

    gpu_index: int
    signals: Optional[HealthSignals]
    findings: List[HealthFinding]
    #: warning reasons that were not raised on the previous poll
    new_warnings: List[str]
    unhealthy: bool
    primary_reason: str


class HealthMonitor:
    def __init__(
        self,
        lib: DeviceLib,
        *,
        on_change: Optional[Callable[[Set[int]], None]] = None,
        on_poll: Optional[Callable[[PollReport], None]] = None,
        interval_s: float = 30.0,
        failures_to_unhealthy: int = 2,
        successes_to_healthy: int = 1,
    ):
        self.lib = lib
        self.on_change = on_change
        self.on_poll = on_poll
        self.interval_s = interval_s
        self.failures_to_unhealthy = failures_to_unhealthy
        self.successes_to_healthy = successes_to_healthy
        self._fail_counts: Dict[int, int] = {}
        self._ok_counts: Dict[int, int] = {}
        self._unhealthy: Set[int] = set()
        #: first / latest reading per GPU (evaluate()'s baseline, previous)
        self._baseline: Dict[int, HealthSignals] = {}
        self._previous: Dict[int, HealthSignals] = {}
        #: uncorrectable count on the poll that raised UncorrectableEcc
        self._ue_raised_at: Dict[int, int] = {}
        self._findings: Dict[int, List[HealthFinding]] = {}
        #: why each unhealthy GPU is unhealthy (kept until it recovers)
        self._reasons: Dict[int, str] = {}
        self._logged_unsupported: Set[Tuple[int, str]] = set()
        #: sticky self-test findings per GPU, added to every poll
        self._selftest: Dict[int, List[HealthFinding]] = {}
        self._stop = threading.Event()
        self._thread: Optional[threading.Thread] = None
        self._lock = threading.Lock()
        #: one poll at a time: the lib calls are made without _lock held
        self._poll_lock = threading.Lock()

    @property
    def unhealthy_gpus(self) -> Set[int]:
        with self._lock:
            return set(self._unhealthy)

    def findings(self, gpu_index: int) -> List[HealthFinding]:
        """Findings of the latest poll for one GPU (warnings included)."""
        with self._lock:
            return list(self._findings.get(gpu_index, ()))

    def signals(self, gpu_index: int) -> Optional[HealthSignals]:
        """Latest successful reading for one GPU."""
        with self._lock:
            return self._previous.get(gpu_index)

    def primary_reason(self, gpu_index: int) -> str:
        """Why the GPU is unhealthy; "" when it is healthy or the reason
        is not known."""
        with self._lock:
            if gpu_index not in self._unhealthy:
                return ""
            return self._reasons.get(gpu_index, "")

    def set_selftest_findings(
        self, gpu_index: int, findings: List[HealthFinding]
    ) -> None:
        """Findings of an active self-test of one GPU. No poll can observe
        them again, so they are sticky: every poll adds them to what it
        found itself until the next call replaces them; an empty list
        clears them. They take effect on the next poll, by the usual rules
        (fatal at once, soft after ``failures_to_unhealthy`` polls)."""
        with self._lock:
            if findings:
                self._selftest[gpu_index] = list(findings)
            else:
                self._selftest.pop(gpu_index, None)

    # ------------------------------------------------------------------
    def _read(self, gpu_index: int):
        """All HAL calls for one GPU; no monitor lock held."""
        extra: List[HealthFinding] = []
        try:
            status = self.lib.health_check(gpu_index).get("status")
            if status != "healthy":
                extra.append(
                    _finding("HealthCheckFailed", f"status {status!r}")
                )
        except Exception as e:
            log.warning("gpu-%d health check error: %s", gpu_index, e)
            extra.append(_finding("HealthCheckFailed", str(e)))
        signals = None
        try:
            signals = self.lib.health_signals(gpu_index)
        except Exception as e:
            log.warning("gpu-%d health signals error: %s", gpu_index, e)
            extra.append(_finding("HealthSignalsError", str(e)))
        return signals, extra

    def _evaluate_locked(
        self, idx: int, signals: Optional[HealthSignals]
    ) -> List[HealthFinding]:
        if signals is None:
            return []
        for name, why in signals.unsupported.items():
            if (idx, name) not in self._logged_unsupported:
                self._logged_unsupported.add((idx, name))
                log.info("gpu-%d: health signal %s unsupported: %s", idx, name, why)
        baseline = self._baseline.setdefault(idx, signals)
        ue, base_ue = signals.ecc_uncorrectable, baseline.ecc_uncorrectable
        if ue is not None and (
            base_ue is None
            or ue < base_ue
            or ue < self._ue_raised_at.get(idx, 0)
        ):
            # The driver zeroes its RAS counters on reload / GPU reset:
            # a count below the baseline, or below the level that raised
            # UncorrectableEcc, starts a new baseline (and clears it).
            baseline = self._baseline[idx] = signals
            self._ue_raised_at.pop(idx, None)
        found = evaluate(baseline, self._previous.get(idx), signals)
        if any(f.reason == "UncorrectableEcc" for f in found):
            self._ue_raised_at.setdefault(idx, ue)
        self._previous[idx] = signals
        return found

    def check_once(self) -> Set[int]:
        """One poll over all GPUs; returns the unhealthy set after
        hysteresis. Fires on_change when the set (or an unhealthy GPU's
        primary reason) changes."""
        try:
            gpus = self.lib.enumerate()
        except Exception:
            log.exception("health enumeration failed")
            return self.unhealthy_gpus
        changed = False
        reports: List[PollReport] = []
        with self._poll_lock:
            readings = [(g.index, *self._read(g.index)) for g in gpus]
            with self._lock:
                for idx, signals, extra in readings:
                    found = _sorted(
                        self._evaluate_locked(idx, signals)
                        + extra
                        + self._selftest.get(idx, [])
                    )
                    before = {
                        f.reason
                        for f in self._findings.get(idx, ())
                        if f.severity == WARNING
                    }
                    self._findings[idx] = found
                    new_warnings = [
                        f.reason
                        for f in found
                        if f.severity == WARNING and f.reason not in before
                    ]
                    for f in found:
                        if f.severity == WARNING and f.reason in new_warnings:
                            log.warning(
                                "gpu-%d: %s: %s", idx, f.reason, f.detail
                            )
                    failing = [f for f in found if f.severity != WARNING]
                    if not failing:
                        self._ok_counts[idx] = self._ok_counts.get(idx, 0) + 1
                        self._fail_counts[idx] = 0
                        if (
                            idx in self._unhealthy
                            and self._ok_counts[idx]
                            >= self.successes_to_healthy
                        ):
                            self._unhealthy.discard(idx)
                            self._reasons.pop(idx, None)
                            changed = True
                            log.info("gpu-%d recovered; republishing", idx)
                    else:
                        self._fail_counts[idx] = (
                            self._fail_counts.get(idx, 0) + 1
                        )
                        self._ok_counts[idx] = 0
                        primary = failing[0]
                        fatal = primary.severity == FATAL
                        if idx in self._unhealthy:
                            if self._reasons.get(idx) != primary.reason:
                                self._reasons[idx] = primary.reason
                                changed = True
                        elif (
                            fatal
                            or self._fail_counts[idx]
                            >= self.failures_to_unhealthy
                        ):
                            self._unhealthy.add(idx)
                            self._reasons[idx] = primary.reason
                            changed = True
                            log.error(
                                "gpu-%d marked unhealthy (%s: %s) after %d "
                                "failing poll(s)",
                                idx,
                                primary.reason,
                                primary.detail,
                                self._fail_counts[idx],
                            )
                    reports.append(
                        PollReport(
                            gpu_index=idx,
                            signals=signals,
                            findings=found,
                            new_warnings=new_warnings,
                            unhealthy=idx in self._unhealthy,
                            primary_reason=self._reasons.get(idx, "")
                            if idx in self._unhealthy
                            else "",
                        )
                    )
                result = set(self._unhealthy)
        if self.on_poll is not None:
            for r in reports:
                try:
                    self.on_poll(r)
                except Exception:
                    log.exception("health on_poll callback failed")
        if changed and self.on_change is not None:
            self.on_change(result)
        return result

    def run(self) -> None:
        while not self._stop.is_set():
            try:
                self.check_once()
            except Exception:
                # e.g. a failed republication: keep polling
                log.exception("health poll failed")
            self._stop.wait(self.interval_s)

    def start(self) -> None:
        self._thread = threading.Thread(
            target=self.run, name="gpu-health", daemon=True
        )
        self._thread.start()

    def stop(self) -> None:
        self._stop.set()
        if self._thread:
            self._thread.join(timeout=5)
