"""Measured CU footprint of a SharedCompute share.

``shared.py`` hands every claim on a GPU a disjoint bit range of
``HSA_CU_MASK`` and ``enforce.py`` audits that the variable is still in a
process's environment. Neither looks at the GPU. This module does: it runs
one launch of ``_hiphealth.cu_footprint`` under a given mask and reports
which physical compute units the blocks ran on, each named by
``(xcc, se, sh, cu)`` as the hardware id registers give it.

Two halves, the same discipline as ``selftest.py``:

- **child** (``python -m k8s_dra_driver_amd.sharing.footprint --device N
  --json``): runs the launch under whatever ``HSA_CU_MASK`` its environment
  holds and prints one JSON object. Exit 0 = measured, 2 = could not run.
  Imports neither torch nor the plugin.
- **parent** (:func:`measure`): starts that child in a fresh process with
  the mask set (or removed) in the child's environment only, one child at a
  time, under a timeout, never a retry, and turns what it says into a
  :class:`Footprint`. ROCr reads the mask once, when a process opens the
  GPU, so a footprint under another mask needs another process; and the
  calling process never initialises HIP.
"""

from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time
from dataclasses import dataclass, field
from typing import Callable, Dict, FrozenSet, List, Optional, Tuple, Union

from ..selftest import _one_child  # one GPU child at a time, whoever calls

PKG_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DEFAULT_TIMEOUT_S = 60.0
ENV_VAR = "HSA_CU_MASK"

EXIT_OK = 0
EXIT_ERROR = 2

#: (xcc, se, sh, cu)
CuKey = Tuple[int, int, int, int]

#: spawn(argv, env, timeout_s) -> (returncode, stdout, stderr); raises
#: subprocess.TimeoutExpired when the child had to be killed
Spawn = Callable[[List[str], Dict[str, str], float], Tuple[int, str, str]]


# ---------------------------------------------------------------------------
# the hardware words
# ---------------------------------------------------------------------------
def decode(hw_id: int, xcc_id: int) -> CuKey:
    """``(xcc, se, sh, cu)`` from the two register words a block stored: the
    mirror of ``foot_decode`` in ``cpp/footprint_kernels.hpp``.

    HW_ID on gfx950 as HIP's ``__smid()`` reads it: CU_ID in bits 11:8,
    SH_ID in bit 12, SE_ID in bits 14:13; XCC_ID in bits 3:0 of its own
    register. The wave slot, SIMD and pipe (bits 7:0), bit 15 and all above
    say which wave, not which CU, and are dropped."""
    return (
        xcc_id & 0xF,
        (hw_id >> 13) & 0x3,
        (hw_id >> 12) & 0x1,
        (hw_id >> 8) & 0xF,
    )


# ---------------------------------------------------------------------------
# HSA_CU_MASK
# ---------------------------------------------------------------------------
def _parse_index_list(text: str, what: str) -> List[int]:
    """``0``, ``0-63``, ``0-31,64-95`` -> sorted distinct indices."""
    out = set()
    for part in text.split(","):
        part = part.strip()
        lo_s, dash, hi_s = part.partition("-")
        lo_s, hi_s = lo_s.strip(), hi_s.strip()
        if not lo_s.isdigit() or (dash and not hi_s.isdigit()):
            raise ValueError(f"{ENV_VAR}: bad {what} {part!r}")
        lo = int(lo_s)
        hi = int(hi_s) if dash else lo
        if hi < lo:
            raise ValueError(f"{ENV_VAR}: {what} range {part!r} runs backwards")
        if hi >= 1 << 16:
            raise ValueError(f"{ENV_VAR}: {what} {hi} is no index")
        out.update(range(lo, hi + 1))
    return sorted(out)


def parse_cu_mask(value: str) -> Dict[int, int]:
    """``HSA_CU_MASK`` text -> ``{gpu_index: mask}``, bit ``i`` of a mask
    set when CU ``i`` is enabled.

    Entries are ``<gpus>:<cus>`` joined by ``;``. ``<cus>`` is a hex
    literal (``0x...``, what the supervisor emits) or a decimal list of
    indices and ranges (``0-63``, ``0-31,64-95``); ``<gpus>`` is a decimal
    index, list or range. Anything else, an entry that enables no CU and a
    GPU named twice raise ``ValueError``."""
    if not isinstance(value, str):
        raise ValueError(f"{ENV_VAR}: not a string: {value!r}")
    if not value.strip():
        raise ValueError(f"{ENV_VAR}: empty")
    masks: Dict[int, int] = {}
    for entry in value.split(";"):
        gpus_s, colon, cus_s = entry.partition(":")
        cus_s = cus_s.strip()
        if not colon or ":" in cus_s:
            raise ValueError(f"{ENV_VAR}: entry {entry!r} is not <gpus>:<cus>")
        gpus = _parse_index_list(gpus_s, "GPU index")
        if cus_s[:2].lower() == "0x":
            digits = cus_s[2:]
            if not digits or any(c not in "0123456789abcdefABCDEF" for c in digits):
                raise ValueError(f"{ENV_VAR}: bad hex mask {cus_s!r}")
            mask = int(digits, 16)
        else:
            mask = 0
            for cu in _parse_index_list(cus_s, "CU index"):
                mask |= 1 << cu
        if mask == 0:
            raise ValueError(f"{ENV_VAR}: entry {entry!r} enables no CU")
        for gpu in gpus:
            if gpu in masks:
                raise ValueError(f"{ENV_VAR}: GPU {gpu} is named twice")
            masks[gpu] = mask
    return masks


def popcount(mask: int) -> int:
    return bin(mask).count("1")


# ---------------------------------------------------------------------------
# result
# ---------------------------------------------------------------------------
@dataclass
class Footprint:
    device: int
    #: the HSA_CU_MASK value the child ran under, None for no mask
    cu_mask: Optional[str] = None
    cus: FrozenSet[CuKey] = frozenset()
    per_xcc: Dict[int, int] = field(default_factory=dict)
    multi_processor_count: int = 0
    blocks: int = 0
    spin: int = 0
    blocks_per_cu_min: int = 0
    blocks_per_cu_max: int = 0
    kernel_ms: float = 0.0
    #: why there is no measurement ("" when there is one)
    error: str = ""
    seconds: float = 0.0

    @property
    def ok(self) -> bool:
        return not self.error

    @property
    def count(self) -> int:
        return len(self.cus)

    def overlap(self, other: "Footprint") -> FrozenSet[CuKey]:
        """The CUs both footprints ran on."""
        return self.cus & other.cus

    def exceeds(self, mask: Union[int, str, None]) -> bool:
        """True when more CUs were seen than ``mask`` has bits. ``mask`` is
        one GPU's bit mask, or an ``HSA_CU_MASK`` value, of which the entry
        of this footprint's device counts; no mask, or no entry for the
        device, allows everything."""
        if mask is None:
            return False
        if isinstance(mask, str):
            mask = parse_cu_mask(mask).get(self.device)
            if mask is None:
                return False
        return self.count > popcount(mask)


def from_report(device: int, cu_mask: Optional[str], report: dict) -> Footprint:
    """A child's (or ``_hiphealth.cu_footprint``'s) dict as a Footprint;
    raises on one that does not have the documented shape."""
    cus = frozenset(tuple(int(v) for v in cu) for cu in report["cus"])
    if any(len(cu) != 4 for cu in cus):
        raise ValueError("a CU is not (xcc, se, sh, cu)")
    if len(cus) != len(report["cus"]) or len(cus) != int(report["count"]):
        raise ValueError("count does not match the CUs listed")
    per_xcc = {int(k): int(v) for k, v in dict(report["per_xcc"]).items()}
    seen: Dict[int, int] = {}
    for cu in cus:
        seen[cu[0]] = seen.get(cu[0], 0) + 1
    if per_xcc != seen:
        raise ValueError("per_xcc does not match the CUs listed")
    return Footprint(
        device=device,
        cu_mask=cu_mask,
        cus=cus,
        per_xcc=per_xcc,
        multi_processor_count=int(report["multi_processor_count"]),
        blocks=int(report["blocks"]),
        spin=int(report["spin"]),
        blocks_per_cu_min=int(report["blocks_per_cu_min"]),
        blocks_per_cu_max=int(report["blocks_per_cu_max"]),
        kernel_ms=float(report.get("kernel_ms", 0.0)),
    )


# ---------------------------------------------------------------------------
# parent
# ---------------------------------------------------------------------------
def _spawn_child(
    argv: List[str], env: Dict[str, str], timeout_s: float
) -> Tuple[int, str, str]:
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


def child_env(cu_mask: Optional[str]) -> Dict[str, str]:
    """A copy of this process's environment for the child: the mask set or
    removed, and the directory of this very package on its import path."""
    env = dict(os.environ)
    env.pop(ENV_VAR, None)
    if cu_mask is not None:
        env[ENV_VAR] = cu_mask
    root = os.path.dirname(PKG_DIR)
    env["PYTHONPATH"] = os.pathsep.join(
        p for p in (root, env.get("PYTHONPATH", "")) if p
    )
    return env


def measure(
    device: int = 0,
    cu_mask: Optional[str] = None,
    timeout_s: float = DEFAULT_TIMEOUT_S,
    spawn: Spawn = _spawn_child,
) -> Footprint:
    """The CU footprint of HIP device ``device`` in a fresh child process
    that runs under ``cu_mask`` (``None``: under no mask, whatever this
    process runs under). Never raises for what goes wrong with the child
    and never retries: that is a Footprint with ``error`` set."""
    argv = [
        sys.executable,
        "-m",
        "k8s_dra_driver_amd.sharing.footprint",
        "--device",
        str(int(device)),
        "--json",
    ]

    def failed(error):
        return Footprint(
            device=device,
            cu_mask=cu_mask,
            error=error,
            seconds=time.monotonic() - t0,
        )

    t0 = time.monotonic()
    if cu_mask is not None:
        try:
            parse_cu_mask(cu_mask)
        except ValueError as e:
            return failed(str(e))
    with _one_child:
        t0 = time.monotonic()
        try:
            rc, out, err = spawn(argv, child_env(cu_mask), timeout_s)
        except subprocess.TimeoutExpired:
            return failed(f"timed out after {timeout_s:g}s; child killed")
        except Exception as e:
            return failed(f"could not start the footprint child: {e}")
        last = (out.strip().splitlines() or [""])[-1]
        try:
            report = json.loads(last)
            if not isinstance(report, dict):
                raise ValueError("not a JSON object")
        except ValueError:
            tail = (err.strip().splitlines() or [""])[-1]
            return failed(
                f"exit {rc}, unparsable output {last[:80]!r}"
                + (f" ({tail[:200]})" if tail else "")
            )
        if rc != EXIT_OK:
            return failed(f"exit {rc}: {report.get('error', 'no reason given')}")
        if report.get("cu_mask") != cu_mask:
            return failed(
                f"the child ran under {ENV_VAR}={report.get('cu_mask')!r}, "
                f"not {cu_mask!r}"
            )
        try:
            fp = from_report(device, cu_mask, report)
        except (KeyError, TypeError, ValueError) as e:
            return failed(f"malformed report: {e!r}")
        fp.seconds = time.monotonic() - t0
        return fp


# ---------------------------------------------------------------------------
# child
# ---------------------------------------------------------------------------
def _child(device: int, blocks: int, spin: int) -> Tuple[int, dict]:
    try:
        from k8s_dra_driver_amd import _hiphealth

        report = dict(_hiphealth.cu_footprint(device, blocks, spin))
        report["cus"] = [list(cu) for cu in report["cus"]]
        report["per_xcc"] = {str(k): v for k, v in report["per_xcc"].items()}
        report["device"] = device
        report["cu_mask"] = os.environ.get(ENV_VAR)
        return EXIT_OK, report
    except Exception as e:
        return EXIT_ERROR, {"error": f"{type(e).__name__}: {e}"}


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(
        "python -m k8s_dra_driver_amd.sharing.footprint",
        description="which CUs this process's blocks run on under its "
        f"{ENV_VAR}; exit 0 measured, 2 could not run",
    )
    ap.add_argument("--device", type=int, default=0, help="HIP device ordinal")
    ap.add_argument("--blocks", type=int, default=0, help="grid (0 = 8 per CU)")
    ap.add_argument("--spin", type=int, default=0, help="FMAs per thread (0 = default)")
    ap.add_argument("--json", action="store_true", help="print the full report")
    args = ap.parse_args(argv)
    rc, report = _child(args.device, args.blocks, args.spin)
    if args.json:
        print(json.dumps(report, sort_keys=True))
    elif "error" in report:
        print(f"device {args.device}: error: {report['error']}")
    else:
        per_xcc = " ".join(f"{k}:{v}" for k, v in sorted(report["per_xcc"].items()))
        print(
            f"device {args.device}: {report['count']} of "
            f"{report['multi_processor_count']} CUs (per XCD {per_xcc}) under "
            f"{ENV_VAR}={report['cu_mask']!r}"
        )
    return rc


if __name__ == "__main__":
    raise SystemExit(main())
