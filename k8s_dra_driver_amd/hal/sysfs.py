"""KFD / DRM sysfs topology parsing.

The ``/proc/devices``-parsing analog of the reference (``nvlib.go:446-488``)
— but richer: KFD exposes the full node topology under
``/sys/class/kfd/kfd/topology/nodes/<n>/``:

- ``properties``: key/value lines (simd_count, gfx_target_version,
  drm_render_minor, location_id, unique_id, ...). Each *compute partition*
  appears as its own KFD node with its own drm_render_minor — this is how
  partition device nodes are discovered after a mode switch.
- ``io_links/<i>/properties``: inter-node links (type 11 = xGMI) giving the
  fabric adjacency the topology-aware allocator publishes.

Root is injectable so tests run against a fixture tree.
"""

from __future__ import annotations

import os
from dataclasses import dataclass, field
from typing import Dict, List

from .model import (
    BAD_PAGE_SIGNALS,
    ECC_SIGNALS,
    THROTTLE_SIGNALS,
    HealthSignals,
)

KFD_IOLINK_TYPE_PCIE = 2
KFD_IOLINK_TYPE_XGMI = 11


@dataclass
class KfdIoLink:
    node_from: int
    node_to: int
    link_type: int
    weight: int = 0
    min_bandwidth: int = 0
    max_bandwidth: int = 0

    @property
    def is_xgmi(self) -> bool:
        return self.link_type == KFD_IOLINK_TYPE_XGMI


@dataclass
class KfdNode:
    node_id: int
    properties: Dict[str, int] = field(default_factory=dict)
    io_links: List[KfdIoLink] = field(default_factory=list)

    @property
    def is_gpu(self) -> bool:
        return self.properties.get("simd_count", 0) > 0

    @property
    def render_minor(self) -> int:
        return self.properties.get("drm_render_minor", -1)

    @property
    def gfx_target_version(self) -> int:
        return self.properties.get("gfx_target_version", 0)

    @property
    def gfx_arch(self) -> str:
        """Decode gfx_target_version (major*10000+minor*100+step) to the
        gfx name, e.g. 90500 -> gfx950."""
        v = self.gfx_target_version
        if v == 0:
            return ""
        major, minor, step = v // 10000, (v // 100) % 100, v % 100
        return f"gfx{major}{minor:x}{step:x}"

    @property
    def cu_count(self) -> int:
        simd = self.properties.get("simd_count", 0)
        per_cu = self.properties.get("simd_per_cu", 4) or 4
        return simd // per_cu

    @property
    def unique_id(self) -> int:
        return self.properties.get("unique_id", 0)

    @property
    def location_id(self) -> int:
        return self.properties.get("location_id", 0)

    @property
    def domain(self) -> int:
        return self.properties.get("domain", 0)

    @property
    def bdf(self) -> str:
        loc = self.location_id
        return f"{self.domain:04x}:{(loc >> 8) & 0xFF:02x}:{(loc >> 3) & 0x1F:02x}.{loc & 0x7}"

    def xgmi_peers(self) -> List[int]:
        return sorted(
            l.node_to for l in self.io_links if l.is_xgmi and l.node_to != self.node_id
        )


def _parse_properties(path: str) -> Dict[str, int]:
    out: Dict[str, int] = {}
    try:
        with open(path) as f:
            for line in f:
                parts = line.split()
                if len(parts) == 2:
                    try:
                        out[parts[0]] = int(parts[1])
                    except ValueError:
                        pass
    except (FileNotFoundError, PermissionError):
        pass
    return out


# ---------------------------------------------------------------------------
# Passive health signals from the amdgpu device directory
# (<root>/class/drm/renderD<minor>/device/):
#
# - ``ras/<block>_err_count``, or ``ras/aca_<block>`` on kernels whose RAS
#   counters come from the ACA error banks (what MI355X nodes expose):
#   lines ``ue: N``, ``ce: N`` and, on newer kernels, ``de: N``
#   (uncorrectable / correctable / deferred);
# - ``ras/gpu_vram_bad_pages``: one ``address : size : flag`` line per
#   retired page, flag R (reserved), P (pending) or F (unreservable);
# - ``hwmon/hwmon*/temp<N>_{label,input,crit}``: labels ``junction`` and
#   ``mem``, values in millidegrees Celsius.
#
# A missing or unreadable file means the signal is unsupported, never zero.
# The retirement threshold and the throttle flags have no plain-text sysfs
# file, so this source always reports them unsupported.
# ---------------------------------------------------------------------------
_ERR_KEYS = {"ue": "uncorrectable", "ce": "correctable", "de": "deferred"}
_PAGE_FLAGS = {
    "R": "bad_pages_reserved",
    "P": "bad_pages_pending",
    "F": "bad_pages_unreservable",
}
_HWMON_LABELS = {"junction": "temp_hotspot", "mem": "temp_vram"}
_NO_SYSFS_FILE = "no sysfs file for this signal"


def _read_text(path: str):
    """File content, or ``(None, reason)`` when it cannot be read."""
    try:
        with open(path) as f:
            return f.read(), ""
    except FileNotFoundError:
        return None, "missing"
    except OSError as e:
        return None, e.strerror or type(e).__name__


def _parse_err_count(text: str) -> Dict[str, int]:
    out: Dict[str, int] = {}
    for line in text.splitlines():
        key, sep, val = line.partition(":")
        name = _ERR_KEYS.get(key.strip())
        if sep and name:
            try:
                out[name] = int(val.strip())
            except ValueError:
                pass
    return out


def _err_count_block(name: str) -> str:
    """Block name of a per-block error-count file, "" for any other file."""
    if name.endswith("_err_count"):
        return name[: -len("_err_count")].upper()
    if name.startswith("aca_"):
        return name[len("aca_"):].upper()
    return ""


def _read_ecc(dev: str, sig: HealthSignals) -> None:
    ras = os.path.join(dev, "ras")
    try:
        files = sorted(n for n in os.listdir(ras) if _err_count_block(n))
        why = "no ras/*_err_count or ras/aca_* files"
    except OSError as e:
        files, why = [], f"ras/: {e.strerror or type(e).__name__}"
    blocks: Dict[str, Dict[str, int]] = {}
    for name in files:
        block = _err_count_block(name)
        if block in blocks:
            continue  # both file generations present: count the block once
        text, err = _read_text(os.path.join(ras, name))
        counts = _parse_err_count(text) if text is not None else {}
        if counts:
            blocks[block] = counts
        else:
            sig.unsupported[f"ecc_blocks.{block}"] = (
                f"ras/{name}: {err or 'no ue:/ce: lines'}"
            )
    if not blocks:
        for n in ECC_SIGNALS + ("ecc_blocks",):
            sig.unsupported[n] = why
        return
    sig.ecc_blocks = blocks
    for kind in ("correctable", "uncorrectable", "deferred"):
        have = [b[kind] for b in blocks.values() if kind in b]
        if have:
            setattr(sig, f"ecc_{kind}", sum(have))
        else:
            sig.unsupported[f"ecc_{kind}"] = (
                f"no {kind} line in the ras/ error-count files"
            )


def _read_bad_pages(dev: str, sig: HealthSignals) -> None:
    text, err = _read_text(os.path.join(dev, "ras", "gpu_vram_bad_pages"))
    if text is None:
        for n in BAD_PAGE_SIGNALS:
            sig.unsupported[n] = f"ras/gpu_vram_bad_pages: {err}"
        return
    counts = {n: 0 for n in BAD_PAGE_SIGNALS}
    for line in text.splitlines():
        parts = [p.strip() for p in line.split(":")]
        if len(parts) == 3 and parts[2] in _PAGE_FLAGS:
            counts[_PAGE_FLAGS[parts[2]]] += 1
    for n, v in counts.items():
        setattr(sig, n, v)


def _read_temps(dev: str, sig: HealthSignals) -> None:
    hwmon_root = os.path.join(dev, "hwmon")
    try:
        hwmons = sorted(
            n for n in os.listdir(hwmon_root) if n.startswith("hwmon")
        )
    except OSError:
        hwmons = []
    found: Dict[str, str] = {}  # signal prefix -> path prefix of temp<N>
    for hw in hwmons:
        d = os.path.join(hwmon_root, hw)
        try:
            names = os.listdir(d)
        except OSError:
            continue
        for n in sorted(names):
            if n.startswith("temp") and n.endswith("_label"):
                text, _ = _read_text(os.path.join(d, n))
                prefix = _HWMON_LABELS.get((text or "").strip())
                if prefix and prefix not in found:
                    found[prefix] = os.path.join(d, n[: -len("_label")])
    for prefix in _HWMON_LABELS.values():
        for suffix, field_name in (
            ("_input", f"{prefix}_c"),
            ("_crit", f"{prefix}_crit_c"),
        ):
            if prefix not in found:
                sig.unsupported[field_name] = "no hwmon sensor with this label"
                continue
            text, err = _read_text(found[prefix] + suffix)
            try:
                setattr(sig, field_name, int((text or "").strip()) / 1000.0)
            except ValueError:
                sig.unsupported[field_name] = (
                    f"hwmon {os.path.basename(found[prefix])}{suffix}: "
                    f"{err or 'not a number'}"
                )


def read_health_signals(sysfs_root: str, render_minor: int) -> HealthSignals:
    """Health signals of the GPU behind ``renderD<render_minor>``, read
    from plain sysfs files only. Never raises for a missing file."""
    dev = os.path.join(
        sysfs_root, "class", "drm", f"renderD{render_minor}", "device"
    )
    sig = HealthSignals()
    _read_ecc(dev, sig)
    _read_bad_pages(dev, sig)
    _read_temps(dev, sig)
    for n in ("bad_page_threshold",) + THROTTLE_SIGNALS:
        sig.unsupported[n] = _NO_SYSFS_FILE
    return sig


class KfdTopology:
    def __init__(self, sysfs_root: str = "/sys"):
        self.root = sysfs_root
        self.nodes_dir = os.path.join(
            sysfs_root, "class", "kfd", "kfd", "topology", "nodes"
        )

    def available(self) -> bool:
        return os.path.isdir(self.nodes_dir)

    def nodes(self) -> List[KfdNode]:
        out: List[KfdNode] = []
        if not self.available():
            return out
        for name in sorted(os.listdir(self.nodes_dir), key=lambda s: int(s) if s.isdigit() else -1):
            if not name.isdigit():
                continue
            node_dir = os.path.join(self.nodes_dir, name)
            node = KfdNode(
                node_id=int(name),
                properties=_parse_properties(os.path.join(node_dir, "properties")),
            )
            links_dir = os.path.join(node_dir, "io_links")
            if os.path.isdir(links_dir):
                for ln in sorted(os.listdir(links_dir)):
                    props = _parse_properties(
                        os.path.join(links_dir, ln, "properties")
                    )
                    if props:
                        node.io_links.append(
                            KfdIoLink(
                                node_from=props.get("node_from", node.node_id),
                                node_to=props.get("node_to", -1),
                                link_type=props.get("type", -1),
                                weight=props.get("weight", 0),
                                min_bandwidth=props.get("min_bandwidth", 0),
                                max_bandwidth=props.get("max_bandwidth", 0),
                            )
                        )
            out.append(node)
        return out

    def gpu_nodes(self) -> List[KfdNode]:
        return [n for n in self.nodes() if n.is_gpu]

    def card_minor_for_render(self, render_minor: int) -> int:
        """Map renderD minor -> cardN via /sys/class/drm (same PCI device)."""
        drm = os.path.join(self.root, "class", "drm")
        try:
            target = os.path.realpath(
                os.path.join(drm, f"renderD{render_minor}", "device")
            )
            for name in os.listdir(drm):
                if name.startswith("card") and name[4:].isdigit():
                    dev = os.path.realpath(os.path.join(drm, name, "device"))
                    if dev == target:
                        return int(name[4:])
        except (FileNotFoundError, PermissionError):
            pass
        return -1
