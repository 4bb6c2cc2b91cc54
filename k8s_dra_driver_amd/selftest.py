"""Startup GPU self-test: write known data to HBM, read it back, and compute
a known answer on the matrix pipes, before the GPU is offered to anybody.

The passive signals of ``plugin/health.py`` only listen to what the amdgpu
driver counts. This is the active counterpart, deliberately narrow: it runs
on a GPU that nothing is using, at a moment when nothing can start using it
(plugin startup, before the first publication), or when an operator asks
for it (``amd-dra-ctl health --selftest``).

Two halves:

- **child** (``python -m k8s_dra_driver_amd.selftest --bdf B --mib N
  --json``): finds the HIP device with that PCI address, runs
  ``_hiphealth.selftest`` on it and prints one JSON object. Exit 0 = passed,
  1 = mismatches found, 2 = could not run. Imports neither torch nor the
  plugin. With ``--per-cu`` it goes on to ``_hiphealth.cu_selftest`` (LDS
  pattern test and the whole known-answer table on every compute unit) and
  puts that result under ``"cu"``: a mismatch then carries the name of the
  CU it happened on. With ``--load-seconds S`` it goes on to
  ``_hiphealth.load_selftest``: a tiled bf16 MFMA GEMM on exact data runs for
  S seconds, every element of every iteration is compared bit for bit, and
  the result goes under ``"load"``. With ``--load-formats mxfp8,mxfp4`` each
  named MX format then runs ``_hiphealth.mx_selftest`` (the same loop on the
  block-scaled MFMA) for as long again, in the order given, and the results
  go under ``"load_mx"``, one per format. With ``--hbm-seconds S`` the last
  stage is ``_hiphealth.hbm_selftest``, the HBM march: all free memory less a
  reserve (or ``--hbm-mib N``) is written, then read, verified and rewritten
  in place pass after pass for S seconds, and the result goes under
  ``"hbm"``.
- **parent** (:func:`run`): starts that child in a fresh process with a
  timeout, one child at a time, and turns what it says into a
  :class:`SelftestResult`. The calling process never initialises HIP, so a
  hung or crashed test cannot take the plugin with it.
"""

from __future__ import annotations

import argparse
import importlib.machinery
import json
import os
import subprocess
import sys
import threading
import time
from dataclasses import dataclass
from typing import Callable, List, Optional, Tuple

PKG_DIR = os.path.dirname(os.path.abspath(__file__))

DEFAULT_MIB = 1024
DEFAULT_TIMEOUT_S = 120.0
#: added to the child's time limit with the load stage, on top of its
#: seconds: generating the operands, the golden product on the vector ALUs
#: and its checksum on the host
LOAD_GOLDEN_ALLOWANCE_S = 60.0
MAX_LOAD_SECONDS = 600.0
#: the MX formats the load stage can go on to, in the extension's order
LOAD_FORMATS = ("mxfp8", "mxfp4")
#: added to the child's time limit per MX format, on top of the load seconds:
#: twice what mx_gemm_ref, the download and the host checksum take at 4096^3,
#: measured as 0.25 s for mxfp8 and 0.19 s for mxfp4 on an MI355X
#: (profiles/mx_selftest.md)
MX_GOLDEN_ALLOWANCE_S = 0.5
#: added to the child's time limit with the HBM march, on top of its seconds:
#: twice what allocating 282 chunks (7.0 s), the first five passes (the
#: shortest run there is, 0.5 s) and freeing the chunks (2.5 s) were measured
#: to take at the default coverage of an empty MI355X, 302 GB
#: (profiles/hbm_selftest.md)
HBM_ALLOWANCE_S = 20.0
#: the least the HBM march covers: below it the region would sit in the
#: 256 MiB Infinity Cache
HBM_MIN_BYTES = 1 << 30
#: how many bad 2 MiB blocks a finding spells out
MAX_PAGES_IN_DETAIL = 4

EXIT_PASS = 0
EXIT_MISMATCH = 1
EXIT_ERROR = 2

#: spawn(argv, timeout_s) -> (returncode, stdout, stderr); raises
#: subprocess.TimeoutExpired when the child had to be killed
Spawn = Callable[[List[str], float], Tuple[int, str, str]]


def extension_path() -> str:
    """The built ``_hiphealth`` extension as a file, "" when it is missing
    (looked for, not imported: importing it initialises nothing, but the
    plugin has no business loading HIP)."""
    for suffix in importlib.machinery.EXTENSION_SUFFIXES:
        path = os.path.join(PKG_DIR, "_hiphealth" + suffix)
        if os.path.exists(path):
            return path
    return ""


# ---------------------------------------------------------------------------
# result
# ---------------------------------------------------------------------------
@dataclass
class SelftestResult:
    gpu_index: int
    bdf: str
    #: pass | memory | compute | error
    outcome: str
    #: the child's JSON object (None when there is none to trust)
    report: Optional[dict] = None
    error: str = ""
    seconds: float = 0.0

    def findings(self) -> list:
        """The result as health findings: none for a pass."""
        from .plugin.health import REASONS, HealthFinding

        severity = dict(REASONS)

        def finding(reason, detail):
            return HealthFinding(reason, severity[reason], detail)

        if self.outcome == "pass":
            return []
        if self.outcome == "error":
            return [finding("SelftestError", self.error)]
        out = []
        report = self.report or {}
        for p in report.get("memory", ()):
            if not p["mismatches"]:
                continue
            detail = f"pattern {p['pattern']}: {p['mismatches']} mismatching word(s)"
            if p["records"]:
                word, got, want = min(p["records"])
                detail += (
                    f"; first recorded word {word}: got 0x{got:016x}, "
                    f"want 0x{want:016x}"
                )
            out.append(finding("SelftestMemoryMismatch", detail))
        mfma = report.get("mfma") or {}
        if mfma.get("mismatches"):
            detail = f"{mfma['mismatches']} mismatching accumulator value(s)"
            if mfma["records"]:
                wave, lane, slot, got, want = min(mfma["records"])
                detail += (
                    f"; first recorded wave {wave} lane {lane} slot {slot}: "
                    f"got 0x{got:08x}, want 0x{want:08x}"
                )
            out.append(finding("SelftestComputeMismatch", detail))
        cu = report.get("cu") or {}
        if cu.get("bad_cus"):
            out.append(finding("SelftestComputeMismatch", _cu_detail(cu)))
        load = report.get("load") or {}
        if load and not load.get("ok", True):
            out.append(finding("SelftestComputeMismatch", _load_detail(load)))
        for fmt, part in (report.get("load_mx") or {}).items():
            if not part.get("ok", True):
                out.append(
                    finding(
                        "SelftestComputeMismatch",
                        f"{fmt} {_load_detail(part)}",
                    )
                )
        hbm = report.get("hbm") or {}
        if hbm and not hbm.get("ok", True):
            out.append(finding("SelftestMemoryMismatch", _hbm_detail(hbm)))
        return out


#: how many bad CUs a finding spells out
MAX_CUS_IN_DETAIL = 4


def _cu_detail(cu: dict) -> str:
    """The per-CU part of a report as one finding's text: how many CUs are
    bad out of those covered, the first few by name, and the lowest record
    of each kind."""
    bad = cu["bad_cus"]
    detail = f"per-CU test: {len(bad)} of {cu['covered']} covered CU(s) bad: "
    detail += ", ".join(
        f"xcc {c['xcc']} se {c['se']} sh {c['sh']} cu {c['cu']} "
        f"(lds {c['lds_mismatches']}, mfma {c['mfma_mismatches']})"
        for c in bad[:MAX_CUS_IN_DETAIL]
    )
    if len(bad) > MAX_CUS_IN_DETAIL:
        detail += f", and {len(bad) - MAX_CUS_IN_DETAIL} more"
    if cu["lds"]["records"]:
        block, pattern, word, got, want = min(cu["lds"]["records"])
        detail += (
            f"; first recorded LDS word: block {block} pattern {pattern} "
            f"word {word}: got 0x{got:016x}, want 0x{want:016x}"
        )
    if cu["mfma"]["records"]:
        block, wave, vector, lane, slot, got, want = min(cu["mfma"]["records"])
        detail += (
            f"; first recorded MFMA value: block {block} wave {wave} vector "
            f"{vector} lane {lane} slot {slot}: got 0x{got:08x}, "
            f"want 0x{want:08x}"
        )
    return detail


def _load_detail(load: dict) -> str:
    """The load part of a report as one finding's text: how long it ran, how
    many values were wrong, the first few bad CUs by name and the lowest
    record."""
    detail = (
        f"load test: {load['mismatches']} mismatching value(s) in "
        f"{load['iterations']} iteration(s) of "
        f"{load['m']}x{load['n']}x{load['k']}"
    )
    if not load["checksum_ok"]:
        detail += (
            "; golden product failed its checksum at "
            f"{load['checksum_first_bad'] or 'an unnamed place'}"
        )
    bad = load["bad_cus"]
    if bad:
        detail += f"; {len(bad)} of {load['cus_seen']} CU(s) seen bad: "
        detail += ", ".join(
            f"xcc {c['xcc']} se {c['se']} sh {c['sh']} cu {c['cu']} "
            f"({c['mismatches']})"
            for c in bad[:MAX_CUS_IN_DETAIL]
        )
        if len(bad) > MAX_CUS_IN_DETAIL:
            detail += f", and {len(bad) - MAX_CUS_IN_DETAIL} more"
    if load["records"]:
        it, row, col, got, want = min(load["records"])
        detail += (
            f"; first recorded value: iteration {it} row {row} col {col}: "
            f"got 0x{got:08x}, want 0x{want:08x}"
        )
    return detail


def _hbm_detail(hbm: dict) -> str:
    """The HBM march's part of a report as one finding's text: how many words
    were wrong in how many passes over how much memory, which bits flipped,
    the first few bad 2 MiB blocks by (chunk, block) and the lowest record."""
    detail = (
        f"hbm march: {hbm['mismatches']} mismatching word(s) in "
        f"{hbm['passes']} pass(es) over {hbm['bytes'] / 2**30:.1f} GiB; "
        f"flipped bits 0x{hbm['flipped_or']:016x}; "
        f"{hbm['bad_pages']} bad 2 MiB block(s): "
    )
    first = hbm["bad_pages_first"]
    detail += ", ".join(
        f"chunk {c} block {p}" for c, p in first[:MAX_PAGES_IN_DETAIL]
    )
    if hbm["bad_pages"] > MAX_PAGES_IN_DETAIL:
        detail += f", and {hbm['bad_pages'] - MAX_PAGES_IN_DETAIL} more"
    if hbm["records"]:
        p, word, got, want = min(hbm["records"])
        detail += (
            f"; first recorded word: pass {p} word {word}: "
            f"got 0x{got:016x}, want 0x{want:016x}"
        )
    return detail


def parse_load_formats(text) -> Tuple[str, ...]:
    """``"mxfp8,mxfp4"`` (or a sequence of names) as a tuple of format names
    in the order given; raises ValueError on an unknown or repeated name."""
    if isinstance(text, str):
        names = [n.strip() for n in text.split(",") if n.strip()]
    else:
        names = [str(n) for n in (text or ())]
    for name in names:
        if name not in LOAD_FORMATS:
            raise ValueError(
                f"unknown load format {name!r} (known: {', '.join(LOAD_FORMATS)})"
            )
    if len(set(names)) != len(names):
        raise ValueError("a load format is named twice")
    return tuple(names)


def _classify_load_mx(load_mx, formats) -> bool:
    """True when an MX part of a report is bad; raises unless ``load_mx`` has
    exactly the formats asked for, each with the documented shape of the
    load part plus its own name. The child prints its report with sorted
    keys, so the order the formats ran in is not in it: ``load_mx`` is put
    back into the order asked for."""
    if not isinstance(load_mx, dict):
        raise TypeError("load_mx is not an object")
    if sorted(load_mx) != sorted(formats):
        raise ValueError(
            f"load_mx has {sorted(load_mx)}, asked for {sorted(formats)}"
        )
    parts = {fmt: load_mx[fmt] for fmt in formats}
    load_mx.clear()
    load_mx.update(parts)
    bad = False
    for fmt, part in load_mx.items():
        if not isinstance(part, dict) or part.get("format") != fmt:
            raise ValueError(f"load_mx[{fmt!r}] does not carry its format")
        if _classify_load(part, f"load_mx[{fmt!r}]"):
            bad = True
    return bad


def _classify_load(load, name: str = "load") -> bool:
    """True when the load part of a report is bad (a mismatch or a failed
    checksum of the golden product); raises on a part that does not have the
    documented shape."""
    if not isinstance(load, dict):
        raise TypeError(f"{name} is not an object")
    for key in ("m", "n", "k", "iterations", "mismatches", "cus_seen"):
        load[key] = int(load[key])
    if not isinstance(load["ok"], bool) or not isinstance(load["checksum_ok"], bool):
        raise TypeError(f"{name}: ok and checksum_ok must be booleans")
    load["checksum_first_bad"] = str(load.get("checksum_first_bad", ""))
    load["tflops"] = float(load["tflops"])
    load["records"] = [tuple(int(v) for v in r) for r in load["records"]]
    if any(len(r) != 5 for r in load["records"]):
        raise ValueError(f"a record of {name} does not have 5 fields")
    load["bad_tiles"] = [tuple(int(v) for v in t) for t in load["bad_tiles"]]
    if any(len(t) != 3 for t in load["bad_tiles"]):
        raise ValueError(f"a bad tile of {name} does not have 3 fields")
    names = ("xcc", "se", "sh", "cu", "mismatches")
    load["bad_cus"] = [{k: int(c[k]) for k in names} for c in load["bad_cus"]]
    mismatched = bool(load["mismatches"])
    if (
        mismatched != bool(load["bad_cus"])
        or mismatched != bool(load["records"])
        or mismatched != bool(load["bad_tiles"])
        or load["ok"] != (not mismatched and load["checksum_ok"])
    ):
        raise ValueError(
            f"{name}: ok, mismatches, checksum_ok and bad_cus disagree"
        )
    if load["iterations"] < 1:
        raise ValueError(f"{name}: no iteration ran")
    return not load["ok"]


def _classify_hbm(hbm) -> bool:
    """True when the HBM march's part of a report lists a mismatch; raises on
    a part that does not have the documented shape, that contradicts itself,
    or that covered too little to have tested HBM."""
    if not isinstance(hbm, dict):
        raise TypeError("hbm is not an object")
    for key in (
        "bytes", "chunks", "free_bytes", "total_bytes", "rounds", "passes",
        "mismatches", "flipped_or", "bad_pages",
    ):
        if isinstance(hbm[key], (bool, float)):
            raise TypeError(f"hbm: {key} must be an integer")
        hbm[key] = int(hbm[key])
        if hbm[key] < 0:
            raise ValueError(f"hbm: {key} is negative")
    if not isinstance(hbm["ok"], bool) or not isinstance(hbm["alloc_short"], bool):
        raise TypeError("hbm: ok and alloc_short must be booleans")
    hbm["seconds"] = float(hbm["seconds"])
    hbm["chunk_bytes"] = [int(b) for b in hbm["chunk_bytes"]]
    hbm["gbs"] = {str(k): float(v) for k, v in dict(hbm["gbs"]).items()}
    hbm["records"] = [tuple(int(v) for v in r) for r in hbm["records"]]
    if any(len(r) != 4 for r in hbm["records"]):
        raise ValueError("a record of hbm does not have 4 fields")
    hbm["bad_chunks"] = [tuple(int(v) for v in c) for c in hbm["bad_chunks"]]
    if any(len(c) != 2 for c in hbm["bad_chunks"]):
        raise ValueError("a bad chunk of hbm does not have 2 fields")
    hbm["bad_pages_first"] = [
        tuple(int(v) for v in p) for p in hbm["bad_pages_first"]
    ]
    if any(len(p) != 2 for p in hbm["bad_pages_first"]):
        raise ValueError("a bad page of hbm does not have 2 fields")
    mismatched = bool(hbm["mismatches"])
    if (
        mismatched != bool(hbm["records"])
        or mismatched != bool(hbm["bad_chunks"])
        or mismatched != bool(hbm["bad_pages"])
        or mismatched != bool(hbm["bad_pages_first"])
        or mismatched != bool(hbm["flipped_or"])
        or hbm["ok"] == mismatched
    ):
        raise ValueError(
            "hbm: ok, mismatches, records, bad_chunks and bad_pages disagree"
        )
    if sum(n for _, n in hbm["bad_chunks"]) != hbm["mismatches"]:
        raise ValueError("hbm: bad_chunks do not add up to mismatches")
    if len(hbm["chunk_bytes"]) != hbm["chunks"] or sum(hbm["chunk_bytes"]) != hbm["bytes"]:
        raise ValueError("hbm: chunk_bytes do not add up to bytes")
    if hbm["bytes"] < HBM_MIN_BYTES:
        raise ValueError(f"hbm: {hbm['bytes']} bytes covered, less than 1 GiB")
    # a clean run is a fill, at least one cycle of four rounds and a verify;
    # a run that found something may have stopped at any pass that reads
    if hbm["passes"] < (2 if mismatched else 5):
        raise ValueError(f"hbm: only {hbm['passes']} pass(es) ran")
    return mismatched


def _classify_cu(cu) -> bool:
    """True when the per-CU part of a report lists a mismatch; raises on a
    part that does not have the documented shape."""
    if not isinstance(cu, dict):
        raise TypeError("cu is not an object")
    lds, mfma = cu["lds"], cu["mfma"]
    bad = bool(int(lds["mismatches"])) or bool(int(mfma["mismatches"]))
    lds["records"] = [
        (int(b), str(p), int(w), int(got), int(want))
        for b, p, w, got, want in lds["records"]
    ]
    mfma["records"] = [tuple(int(v) for v in r) for r in mfma["records"]]
    if any(len(r) != 7 for r in mfma["records"]):
        raise ValueError("an MFMA record of cu does not have 7 fields")
    cu["covered"] = int(cu["covered"])
    cu["multi_processor_count"] = int(cu["multi_processor_count"])
    names = ("xcc", "se", "sh", "cu", "blocks", "lds_mismatches", "mfma_mismatches")
    cu["bad_cus"] = [{k: int(c[k]) for k in names} for c in cu["bad_cus"]]
    if bad != bool(cu["bad_cus"]) or bad == bool(cu["ok"]):
        raise ValueError("cu: ok, the mismatch counts and bad_cus disagree")
    return bad


def _classify(report: dict, load_formats=()) -> str:
    """pass | memory | compute from a child's report; raises on a report
    that does not have the documented shape."""
    memory_bad = any(int(p["mismatches"]) for p in report["memory"])
    compute_bad = bool(int(report["mfma"]["mismatches"]))
    if "cu" in report and _classify_cu(report["cu"]):
        compute_bad = True
    if "load" in report and _classify_load(report["load"]):
        compute_bad = True
    if "load_mx" in report and _classify_load_mx(report["load_mx"], load_formats):
        compute_bad = True
    if "hbm" in report and _classify_hbm(report["hbm"]):
        memory_bad = True
    for part in list(report["memory"]) + [report["mfma"]]:
        part["records"] = [tuple(int(v) for v in r) for r in part["records"]]
    if any("pattern" not in p for p in report["memory"]):
        raise KeyError("pattern")
    if memory_bad:
        return "memory"
    if compute_bad:
        return "compute"
    if not report["ok"]:
        raise ValueError("report says not ok but lists no mismatch")
    return "pass"


# ---------------------------------------------------------------------------
# parent
# ---------------------------------------------------------------------------
def _spawn_child(argv: List[str], timeout_s: float) -> Tuple[int, str, str]:
    env = dict(os.environ)
    # the child must import this very package
    root = os.path.dirname(PKG_DIR)
    env["PYTHONPATH"] = os.pathsep.join(
        p for p in (root, env.get("PYTHONPATH", "")) if p
    )
    # subprocess.run kills the child and reaps it when the timeout expires
    done = subprocess.run(
        argv,
        capture_output=True,
        text=True,
        env=env,
        timeout=timeout_s,
        stdin=subprocess.DEVNULL,
    )
    return done.returncode, done.stdout, done.stderr


#: one child at a time, whoever calls
_one_child = threading.Lock()


def run(
    gpu,
    *,
    mib: int = DEFAULT_MIB,
    timeout_s: float = DEFAULT_TIMEOUT_S,
    spawn: Spawn = _spawn_child,
    per_cu: bool = False,
    load_seconds: float = 0.0,
    load_formats=(),
    hbm_seconds: float = 0.0,
    hbm_mib: int = 0,
) -> SelftestResult:
    """Self-test one GPU (a ``hal.model.GpuInfo``: ``index`` and
    ``pcie_bdf`` are used) in a child process; ``per_cu`` adds the per-CU
    stage, a positive ``load_seconds`` the load stage of that length, which
    extends the child's time limit by as much plus
    ``LOAD_GOLDEN_ALLOWANCE_S``. Each MX format of ``load_formats`` (names of
    ``LOAD_FORMATS``; only with a positive ``load_seconds``) then runs for
    ``load_seconds`` as well and extends the limit by as much plus
    ``MX_GOLDEN_ALLOWANCE_S``. A positive ``hbm_seconds`` adds the HBM march
    of that length as the last stage, over ``hbm_mib`` MiB (0 = all free
    memory less the reserve), and extends the limit by as much plus
    ``HBM_ALLOWANCE_S``. Never raises and never retries: whatever goes
    wrong is an ``error`` result."""
    bdf = gpu.pcie_bdf
    load_seconds = float(load_seconds)
    hbm_seconds = float(hbm_seconds)
    t0 = time.monotonic()
    try:
        load_formats = parse_load_formats(load_formats)
        if load_formats and not load_seconds > 0:
            raise ValueError("load formats need a positive load_seconds")
        hbm_mib = int(hbm_mib)
        if hbm_mib and not hbm_seconds > 0:
            raise ValueError("hbm_mib needs a positive hbm_seconds")
        if hbm_mib < 0 or 0 < hbm_mib < HBM_MIN_BYTES >> 20:
            raise ValueError("hbm_mib must be 0 or at least 1024")
    except ValueError as e:
        return SelftestResult(
            gpu_index=gpu.index, bdf=bdf, outcome="error", error=str(e)
        )
    argv = [
        sys.executable,
        "-m",
        "k8s_dra_driver_amd.selftest",
        "--bdf",
        bdf,
        "--mib",
        str(int(mib)),
        "--json",
    ]
    if per_cu:
        argv.append("--per-cu")
    with_load = load_seconds > 0
    if with_load:
        argv += ["--load-seconds", f"{load_seconds:g}"]
        timeout_s = timeout_s + load_seconds + LOAD_GOLDEN_ALLOWANCE_S
    if load_formats:
        argv += ["--load-formats", ",".join(load_formats)]
        timeout_s += len(load_formats) * (load_seconds + MX_GOLDEN_ALLOWANCE_S)
    with_hbm = hbm_seconds > 0
    if with_hbm:
        argv += ["--hbm-seconds", f"{hbm_seconds:g}"]
        if hbm_mib:
            argv += ["--hbm-mib", str(hbm_mib)]
        timeout_s = timeout_s + hbm_seconds + HBM_ALLOWANCE_S

    def result(outcome, report=None, error=""):
        return SelftestResult(
            gpu_index=gpu.index,
            bdf=bdf,
            outcome=outcome,
            report=report,
            error=error,
            seconds=time.monotonic() - t0,
        )

    with _one_child:
        t0 = time.monotonic()
        try:
            rc, out, err = spawn(argv, timeout_s)
        except subprocess.TimeoutExpired:
            return result("error", error=f"timed out after {timeout_s:g}s; child killed")
        except Exception as e:
            return result("error", error=f"could not start the self-test: {e}")
        last = (out.strip().splitlines() or [""])[-1]
        try:
            report = json.loads(last)
            if not isinstance(report, dict):
                raise ValueError("not a JSON object")
        except ValueError:
            tail = (err.strip().splitlines() or [""])[-1]
            return result(
                "error",
                error=f"exit {rc}, unparsable output {last[:80]!r}"
                + (f" ({tail[:200]})" if tail else ""),
            )
        if rc == EXIT_ERROR or rc not in (EXIT_PASS, EXIT_MISMATCH):
            return result(
                "error",
                report=report,
                error=f"exit {rc}: {report.get('error', 'no reason given')}",
            )
        try:
            if per_cu and "cu" not in report:
                raise KeyError("cu")
            if with_load and "load" not in report:
                raise KeyError("load")
            if load_formats and "load_mx" not in report:
                raise KeyError("load_mx")
            if not load_formats and "load_mx" in report:
                raise ValueError("load_mx was not asked for")
            if with_hbm and "hbm" not in report:
                raise KeyError("hbm")
            if not with_hbm and "hbm" in report:
                raise ValueError("hbm was not asked for")
            outcome = _classify(report, load_formats)
        except (KeyError, TypeError, ValueError) as e:
            return result("error", error=f"exit {rc}, malformed report: {e!r}")
        if (outcome == "pass") != (rc == EXIT_PASS):
            return result(
                "error", error=f"exit {rc} contradicts the report ({outcome})"
            )
        return result(outcome, report=report)


# ---------------------------------------------------------------------------
# child
# ---------------------------------------------------------------------------
def _child(
    bdf: str,
    mib: int,
    per_cu: bool = False,
    load_seconds: float = 0.0,
    load_formats=(),
    hbm_seconds: float = 0.0,
    hbm_mib: int = 0,
) -> Tuple[int, dict]:
    try:
        from k8s_dra_driver_amd import _hiphealth

        want = bdf.strip().lower()
        seen = []
        for ordinal in range(_hiphealth.device_count()):
            have = _hiphealth.pci_bus_id(ordinal).strip().lower()
            seen.append(have)
            if have == want:
                report = _hiphealth.selftest(ordinal, mib=mib)
                report["bdf"] = have
                if per_cu:
                    report["cu"] = _hiphealth.cu_selftest(ordinal)
                    report["ok"] = bool(report["ok"] and report["cu"]["ok"])
                if load_seconds > 0:
                    report["load"] = _hiphealth.load_selftest(
                        ordinal, seconds=load_seconds
                    )
                    report["ok"] = bool(report["ok"] and report["load"]["ok"])
                if load_formats:
                    report["load_mx"] = {}
                    for fmt in load_formats:
                        part = _hiphealth.mx_selftest(ordinal, fmt, load_seconds)
                        report["load_mx"][fmt] = part
                        report["ok"] = bool(report["ok"] and part["ok"])
                if hbm_seconds > 0:
                    report["hbm"] = _hiphealth.hbm_selftest(
                        ordinal, seconds=hbm_seconds, mib=hbm_mib
                    )
                    report["ok"] = bool(report["ok"] and report["hbm"]["ok"])
                return (EXIT_PASS if report["ok"] else EXIT_MISMATCH), report
        return EXIT_ERROR, {
            "ok": False,
            "error": f"no HIP device at {bdf} (visible: {seen or 'none'})",
        }
    except Exception as e:
        return EXIT_ERROR, {"ok": False, "error": f"{type(e).__name__}: {e}"}


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(
        "python -m k8s_dra_driver_amd.selftest",
        description="self-test one GPU; exit 0 passed, 1 mismatches, 2 could not run",
    )
    ap.add_argument("--bdf", required=True, help="PCI address, e.g. 0000:c1:00.0")
    ap.add_argument("--mib", type=int, default=DEFAULT_MIB, help="HBM region to test")
    ap.add_argument(
        "--per-cu",
        action="store_true",
        help="also test every compute unit's LDS and matrix pipes, by name",
    )
    ap.add_argument(
        "--load-seconds",
        type=float,
        default=0.0,
        help="also run the load test (a tiled bf16 GEMM on exact data, "
        "every element of every iteration compared) for this long; 0 = off",
    )
    ap.add_argument(
        "--load-formats",
        default="",
        help="after the load test, run it again on the block-scaled MFMA for "
        "each of these MX formats (comma-separated: "
        + ", ".join(LOAD_FORMATS)
        + "), --load-seconds each; needs --load-seconds",
    )
    ap.add_argument(
        "--hbm-seconds",
        type=float,
        default=0.0,
        help="as the last stage, run the HBM march (every element of the "
        "coverage read, verified and rewritten in place, pass after pass) "
        "for this long; 0 = off",
    )
    ap.add_argument(
        "--hbm-mib",
        type=int,
        default=0,
        help="memory the HBM march covers, at least 1024; 0 = all that is "
        "free less max(2 GiB, 2 %% of the total); needs --hbm-seconds",
    )
    ap.add_argument("--json", action="store_true", help="print the full report")
    args = ap.parse_args(argv)
    t0 = time.monotonic()
    if args.load_seconds < 0 or args.load_seconds > MAX_LOAD_SECONDS:
        ap.error(f"--load-seconds must be in [0, {MAX_LOAD_SECONDS:g}]")
    try:
        formats = parse_load_formats(args.load_formats)
    except ValueError as e:
        ap.error(f"--load-formats: {e}")
    if formats and not args.load_seconds > 0:
        ap.error("--load-formats needs a positive --load-seconds")
    extra = {"load_seconds": args.load_seconds} if args.load_seconds > 0 else {}
    if formats:
        extra["load_formats"] = formats
    if args.hbm_seconds < 0 or args.hbm_seconds > MAX_LOAD_SECONDS:
        ap.error(f"--hbm-seconds must be in [0, {MAX_LOAD_SECONDS:g}]")
    if args.hbm_mib and not args.hbm_seconds > 0:
        ap.error("--hbm-mib needs a positive --hbm-seconds")
    if args.hbm_mib < 0 or 0 < args.hbm_mib < HBM_MIN_BYTES >> 20:
        ap.error("--hbm-mib must be 0 or at least 1024")
    if args.hbm_seconds > 0:
        extra["hbm_seconds"] = args.hbm_seconds
        if args.hbm_mib:
            extra["hbm_mib"] = args.hbm_mib
    rc, report = _child(args.bdf, args.mib, args.per_cu, **extra)
    report["seconds"] = round(time.monotonic() - t0, 3)
    if args.json:
        print(json.dumps(report, sort_keys=True))
    elif "error" in report:
        print(f"{args.bdf}: error: {report['error']}")
    else:
        bad = sum(p["mismatches"] for p in report["memory"])
        print(
            f"{args.bdf}: {'ok' if report['ok'] else 'FAILED'}: "
            f"{report['bytes'] >> 20} MiB x 4 patterns, {bad} memory "
            f"mismatch(es); mfma {report['mfma']['mismatches']} mismatch(es) "
            f"in {report['mfma']['checked']} values"
        )
        if "cu" in report:
            cu = report["cu"]
            print(
                f"{args.bdf}: per CU: {cu['covered']} of "
                f"{cu['multi_processor_count']} CUs covered, "
                f"{len(cu['bad_cus'])} bad; lds {cu['lds']['mismatches']} "
                f"mismatch(es), mfma {cu['mfma']['mismatches']} mismatch(es)"
            )
        if "load" in report:
            load = report["load"]
            print(
                f"{args.bdf}: load: {load['iterations']} iteration(s) of "
                f"{load['m']}x{load['n']}x{load['k']} in "
                f"{load['seconds']:.1f}s on {load['cus_seen']} CUs, "
                f"{load['mismatches']} mismatch(es), checksum "
                f"{'ok' if load['checksum_ok'] else 'FAILED'}; "
                f"{load['tflops']:.0f} TF/s (informative)"
            )
        for fmt, part in report.get("load_mx", {}).items():
            print(
                f"{args.bdf}: load {fmt}: {part['iterations']} iteration(s) of "
                f"{part['m']}x{part['n']}x{part['k']} in "
                f"{part['seconds']:.1f}s on {part['cus_seen']} CUs, "
                f"{part['mismatches']} mismatch(es), checksum "
                f"{'ok' if part['checksum_ok'] else 'FAILED'}; "
                f"{part['tflops']:.0f} TF/s (informative)"
            )
        if "hbm" in report:
            hbm = report["hbm"]
            gbs = hbm["gbs"]
            print(
                f"{args.bdf}: hbm march: {hbm['passes']} pass(es) over "
                f"{hbm['bytes'] / 2**30:.1f} GiB in {hbm['chunks']} chunk(s)"
                f"{' (allocation fell short)' if hbm['alloc_short'] else ''} "
                f"in {hbm['seconds']:.1f}s, {hbm['mismatches']} mismatch(es) "
                f"in {hbm['bad_pages']} 2 MiB block(s); fill "
                f"{gbs['fill']:.0f}, march {gbs['march_addr']:.0f} / "
                f"{gbs['march_hash']:.0f}, verify {gbs['verify']:.0f} GB/s "
                "(informative)"
            )
    return rc


if __name__ == "__main__":
    raise SystemExit(main())
