"""amd-dra-ctl — operational CLI for the driver's hardware layer.

The nvidia-smi-adjacent workflows an operator needs around this driver:
inspect devices/topology as the driver sees them, dump the ResourceSlice
projection, carve/restore partitions, and run the health probes.

    amd-dra-ctl list                 # devices incl. partitions
    amd-dra-ctl topology             # xGMI adjacency matrix
    amd-dra-ctl slice                # ResourceSlice device JSON
    amd-dra-ctl partition 0 CPX NPS1 # dynamic repartition (needs idle GPU)
    amd-dra-ctl health               # per-GPU health + HIP probes
    amd-dra-ctl health --signals     # + ECC / retired-page / thermal signals
    amd-dra-ctl health --selftest    # + HBM pattern / MFMA known-answer test
    amd-dra-ctl health --selftest --per-cu   # + LDS / MFMA test of every CU
    amd-dra-ctl health --selftest --load-seconds 5   # + checked GEMM under load
    amd-dra-ctl health --selftest --load-seconds 5 --load-formats mxfp8,mxfp4
    amd-dra-ctl health --selftest --hbm-seconds 10   # + march over all free HBM
                                     # + the same on the block-scaled MFMA
Use ``--hal fake`` anywhere to drive the modeled 8xMI355X node.
"""

from __future__ import annotations

import argparse
import json
import sys

from .hal import new_device_lib
from .hal.model import AllocatableDevice


def _lib(args):
    lib = new_device_lib(args.hal)
    lib.open()
    return lib


def cmd_list(args) -> int:
    lib = _lib(args)
    for g in lib.enumerate():
        print(
            f"{g.canonical_name}: {g.product_name} [{g.architecture}] "
            f"uuid={g.uuid} oam={g.oam_id} vram={g.vram_total_mib}MiB "
            f"cu={g.cu_count} renderD{g.render_minor} "
            f"mode={g.compute_partition}/{g.memory_partition}"
        )
        for p in g.partitions:
            print(
                f"  {p.canonical_name}: kfd={p.kfd_node_id} "
                f"renderD{p.render_minor} "
                f"cu={p.profile.cus_per_partition} "
                f"mem={p.profile.memory_mib_per_partition}MiB "
                f"domain={p.profile.memory_domain_of(p.partition_id)}"
            )
    return 0


def cmd_topology(args) -> int:
    lib = _lib(args)
    gpus = lib.enumerate()
    ids = [g.oam_id for g in gpus]
    print("xGMI adjacency (links between OAM ids):")
    print("     " + " ".join(f"{i:>3}" for i in ids))
    for g in gpus:
        peers = set(g.xgmi_peer_oam_ids())
        row = " ".join(
            "  x" if i == g.oam_id else ("  1" if i in peers else "  .")
            for i in ids
        )
        print(f"{g.oam_id:>4} {row}")
    hives = {g.xgmi_hive_id for g in gpus}
    print(f"hives: {sorted(hives)}")
    return 0


def cmd_slice(args) -> int:
    lib = _lib(args)
    devices = []
    shared_counters = []
    for g in lib.enumerate():
        if g.partitions:
            devices.extend(
                AllocatableDevice.from_partition(g, p).to_device()
                for p in g.partitions
            )
        else:
            if getattr(args, "prospective", ""):
                from .hal.model import (
                    gpu_device_with_counters,
                    prospective_partition_devices,
                    shared_counter_set,
                )
                from .partition.catalog import (
                    make_profile,
                    preferred_memory_mode,
                )

                shared_counters.append(shared_counter_set(g))
                devices.append(gpu_device_with_counters(g))
                prof = make_profile(
                    args.prospective.upper(),
                    preferred_memory_mode(
                        args.prospective.upper(), g.nps_caps
                    ),
                    vram_total_mib=g.vram_total_mib or 288 * 1024,
                    cu_count=g.cu_count or 256,
                    nps_caps=g.nps_caps,
                )
                devices.extend(prospective_partition_devices(g, prof))
            else:
                devices.append(AllocatableDevice.from_gpu(g).to_device())
    out: dict = {"devices": devices}
    if shared_counters:
        out["sharedCounters"] = shared_counters
    print(json.dumps(out, indent=2, sort_keys=True))
    return 0


def cmd_partition(args) -> int:
    from .partition.manager import PartitionManager, RepartitionRefused

    lib = _lib(args)
    mgr = PartitionManager(lib)
    try:
        switched = mgr.ensure_mode(
            args.gpu, args.compute.upper(), args.memory.upper(), allow_dynamic=True
        )
    except (RepartitionRefused, ValueError) as e:
        print(f"refused: {e}", file=sys.stderr)
        return 1
    g = lib.enumerate()[args.gpu]
    print(
        f"gpu-{args.gpu}: {'switched to' if switched else 'already'} "
        f"{g.compute_partition}/{g.memory_partition} "
        f"({len(g.partitions) or 1} device(s))"
    )
    return 0


def _health_record(lib, g) -> dict:
    """health_check + passive signals + one-shot policy for one GPU. A
    single reading has no earlier poll to compare with, so growth-based
    findings (UncorrectableEcc, CorrectableEccGrowth, DeferredEcc) can only
    come from the running plugin; a non-zero uncorrectable count shows up
    here as UncorrectableEccHistoric."""
    from .plugin.health import HealthFinding, evaluate

    h = lib.health_check(g.index)
    findings = []
    if h.get("status") != "healthy":
        findings.append(
            HealthFinding(
                "HealthCheckFailed", "soft", f"status {h.get('status')!r}"
            )
        )
    signals = None
    try:
        signals = lib.health_signals(g.index)
        findings += evaluate(signals, None, signals)
    except Exception as e:
        findings.append(HealthFinding("HealthSignalsError", "soft", str(e)))
    return {
        "name": g.canonical_name,
        "index": g.index,
        "uuid": g.uuid,
        "health": h,
        "signals": {
            k: v
            for k, v in (signals.to_dict() if signals else {}).items()
            if k != "unsupported" and v is not None
        },
        "unsupported": dict(signals.unsupported) if signals else {},
        "findings": [
            {"reason": f.reason, "severity": f.severity, "detail": f.detail}
            for f in findings
        ],
    }


def _print_signals(rec: dict) -> None:
    for k, v in rec["signals"].items():
        if k == "ecc_blocks":
            for block, counts in sorted(v.items()):
                print(
                    f"    ecc_blocks.{block}: "
                    + " ".join(f"{n}={c}" for n, c in sorted(counts.items()))
                )
        else:
            print(f"    {k}: {v}")
    for f in rec["findings"]:
        print(f"    finding [{f['severity']}] {f['reason']}: {f['detail']}")
    if not rec["findings"]:
        print("    findings: none")
    for k, why in sorted(rec["unsupported"].items()):
        print(f"    unsupported {k}: {why}")


def _load_formats(text: str):
    """argparse type of --load-formats: a tuple of MX format names."""
    from . import selftest

    try:
        return selftest.parse_load_formats(text)
    except ValueError as e:
        raise argparse.ArgumentTypeError(str(e))


def _selftest_into(
    rec: dict,
    g,
    mib: int,
    per_cu: bool = False,
    load_seconds: float = 0.0,
    load_formats=(),
    hbm_seconds: float = 0.0,
    hbm_mib: int = 0,
) -> None:
    """Self-test one GPU in a child process and add what it found to the
    GPU's record. The operator vouches that nothing is using the GPU; a
    partitioned GPU, or one without a PCI address, is skipped."""
    from . import selftest

    if g.compute_partition.upper() != "SPX" or g.partitions or not g.pcie_bdf:
        rec["selftest"] = {"result": "skipped"}
        return
    extra = {"per_cu": True} if per_cu else {}
    if load_seconds > 0:
        extra["load_seconds"] = load_seconds
    if load_formats:
        extra["load_formats"] = tuple(load_formats)
    if hbm_seconds > 0:
        extra["hbm_seconds"] = hbm_seconds
        if hbm_mib:
            extra["hbm_mib"] = hbm_mib
    res = selftest.run(g, mib=mib, **extra)
    rec["selftest"] = {
        "result": res.outcome,
        "seconds": round(res.seconds, 3),
        "mib": mib,
    }
    cu = (res.report or {}).get("cu") if per_cu else None
    if cu:
        rec["selftest"]["cu"] = {
            "covered": cu["covered"],
            "expected": cu["multi_processor_count"],
            "bad_cus": cu["bad_cus"],
        }
    load = (res.report or {}).get("load") if load_seconds > 0 else None
    if load:
        rec["selftest"]["load"] = {
            "iterations": load["iterations"],
            "mismatches": load["mismatches"],
            "checksum_ok": load["checksum_ok"],
            "cus_seen": load["cus_seen"],
            "tflops": load["tflops"],
            "bad_cus": load["bad_cus"],
        }
    load_mx = (res.report or {}).get("load_mx") if load_formats else None
    if load_mx:
        rec["selftest"]["load_mx"] = {
            fmt: {
                "iterations": part["iterations"],
                "mismatches": part["mismatches"],
                "checksum_ok": part["checksum_ok"],
                "cus_seen": part["cus_seen"],
                "tflops": part["tflops"],
                "bad_cus": part["bad_cus"],
            }
            for fmt, part in load_mx.items()
        }
    hbm = (res.report or {}).get("hbm") if hbm_seconds > 0 else None
    if hbm:
        rec["selftest"]["hbm"] = {
            "bytes": hbm["bytes"],
            "chunks": hbm["chunks"],
            "alloc_short": hbm["alloc_short"],
            "passes": hbm["passes"],
            "mismatches": hbm["mismatches"],
            "flipped_or": hbm["flipped_or"],
            "bad_chunks": hbm["bad_chunks"],
            "bad_pages": hbm["bad_pages"],
            "gbs": hbm["gbs"],
        }
    rec["findings"] += [
        {"reason": f.reason, "severity": f.severity, "detail": f.detail}
        for f in res.findings()
    ]


def cmd_health(args) -> int:
    lib = _lib(args)
    rc = 0
    records = []
    for g in lib.enumerate():
        rec = _health_record(lib, g)
        if args.selftest:
            _selftest_into(
                rec,
                g,
                args.selftest_mib,
                args.per_cu,
                args.load_seconds,
                args.load_formats,
                args.hbm_seconds,
                args.hbm_mib,
            )
        records.append(rec)
        if not args.json:
            print(f"{g.canonical_name}: {rec['health']}")
            if args.signals:
                _print_signals(rec)
            if args.selftest:
                st = rec["selftest"]
                print(
                    f"    selftest: {st['result']}"
                    + (f" ({st['seconds']:.1f}s)" if "seconds" in st else "")
                )
                if "cu" in st:
                    cu = st["cu"]
                    print(
                        f"    per CU: {cu['covered']} of {cu['expected']} CUs "
                        f"covered, {len(cu['bad_cus'])} bad"
                    )
                    for c in cu["bad_cus"]:
                        print(
                            f"      xcc {c['xcc']} se {c['se']} sh {c['sh']} "
                            f"cu {c['cu']}: lds {c['lds_mismatches']}, "
                            f"mfma {c['mfma_mismatches']}"
                        )
                if "load" in st:
                    load = st["load"]
                    print(
                        f"    load: {load['iterations']} iteration(s), "
                        f"{load['mismatches']} mismatch(es), checksum "
                        f"{'ok' if load['checksum_ok'] else 'FAILED'}, "
                        f"{load['cus_seen']} CUs seen, "
                        f"{load['tflops']:.0f} TF/s (informative)"
                    )
                for fmt, part in st.get("load_mx", {}).items():
                    print(
                        f"    load {fmt}: {part['iterations']} iteration(s), "
                        f"{part['mismatches']} mismatch(es), checksum "
                        f"{'ok' if part['checksum_ok'] else 'FAILED'}, "
                        f"{part['cus_seen']} CUs seen, "
                        f"{part['tflops']:.0f} TF/s (informative)"
                    )
                if "hbm" in st:
                    hbm = st["hbm"]
                    print(
                        f"    hbm march: {hbm['passes']} pass(es) over "
                        f"{hbm['bytes'] / 2**30:.1f} GiB in {hbm['chunks']} "
                        f"chunk(s), {hbm['mismatches']} mismatch(es) in "
                        f"{hbm['bad_pages']} 2 MiB block(s), march "
                        f"{hbm['gbs']['march_hash']:.0f} GB/s (informative)"
                    )
                if not args.signals:
                    for f in rec["findings"]:
                        if f["reason"].startswith("Selftest"):
                            print(
                                f"    finding [{f['severity']}] "
                                f"{f['reason']}: {f['detail']}"
                            )
        if any(f["severity"] in ("fatal", "soft") for f in rec["findings"]):
            rc = 1
    if args.json:
        print(json.dumps(records, indent=2, sort_keys=True))
    if args.probe:
        from . import _hiphealth

        for d in range(_hiphealth.device_count()):
            chk = _hiphealth.mfma_check(d)
            bw = _hiphealth.bandwidth_gbs(d, 256, 5)
            print(
                f"hip:{d}: mfma_ok={chk['ok']} bandwidth={bw:.0f}GB/s",
                file=sys.stderr if args.json else sys.stdout,
            )
            if not chk["ok"]:
                rc = 1
    return rc


def cmd_labels(args) -> int:
    """Preview the node labels the controller would derive from this
    node's devices (gpu.count, architecture, hive, partition modes)."""
    from .controller.manager import labels_for_node

    lib = _lib(args)
    devices = []
    for g in lib.enumerate():
        if g.partitions:
            devices.extend(
                AllocatableDevice.from_partition(g, p).to_device()
                for p in g.partitions
            )
        else:
            devices.append(AllocatableDevice.from_gpu(g).to_device())
    for k, v in sorted(labels_for_node(devices).items()):
        print(f"{k}={v}")
    return 0


def cmd_profile(args) -> int:
    """Fetch an on-demand CPU profile from a running plugin/controller's
    diag server (/debug/profile) — the `go tool pprof` moment for the
    prepare path; output is collapsed-stack (flamegraph.pl-ready)."""
    import urllib.request

    url = (
        f"http://{args.host}:{args.port}/debug/profile"
        f"?seconds={args.seconds}"
    )
    body = urllib.request.urlopen(url, timeout=args.seconds + 30).read()
    sys.stdout.write(body.decode())
    return 0


def main(argv=None) -> int:
    ap = argparse.ArgumentParser("amd-dra-ctl")
    ap.add_argument("--hal", default="amdsmi", choices=["amdsmi", "kfd", "fake"])
    sub = ap.add_subparsers(dest="cmd", required=True)
    sub.add_parser("list")
    sub.add_parser("topology")
    sp = sub.add_parser("slice")
    sp.add_argument(
        "--prospective",
        default="",
        choices=["", "cpx", "dpx", "qpx"],
        help="include prospective partitions + counter sets (what "
        "--prospective-partitions would publish)",
    )
    pp = sub.add_parser("partition")
    pp.add_argument("gpu", type=int)
    pp.add_argument("compute")
    pp.add_argument("memory", nargs="?", default="NPS1")
    sub.add_parser("labels")
    hp = sub.add_parser("health")
    hp.add_argument("--probe", action="store_true", help="also run HIP kernels")
    hp.add_argument(
        "--signals",
        action="store_true",
        help="also print ECC / retired-page / thermal signals, findings "
        "and the unsupported list",
    )
    hp.add_argument(
        "--selftest",
        action="store_true",
        help="also fill and verify HBM with known patterns and run the MFMA "
        "known-answer test, one GPU at a time in a child process; only for "
        "GPUs that nothing is using",
    )
    hp.add_argument(
        "--per-cu",
        action="store_true",
        help="with --selftest, also test the LDS and the matrix pipes of "
        "every compute unit and name the CUs that fail",
    )
    hp.add_argument(
        "--load-seconds",
        type=float,
        default=0.0,
        help="with --selftest, also run a tiled bf16 GEMM on exact data for "
        "this many seconds per GPU and compare every element of every "
        "iteration bit for bit (0 = off)",
    )
    hp.add_argument(
        "--load-formats",
        type=_load_formats,
        default=(),
        metavar="FORMAT[,FORMAT]",
        help="with --load-seconds, run the load test again on the "
        "block-scaled MFMA for each of these MX formats (mxfp8, mxfp4), "
        "--load-seconds each",
    )
    hp.add_argument(
        "--hbm-seconds",
        type=float,
        default=0.0,
        help="with --selftest, finish with the HBM march: all free memory "
        "is written, then read, verified and rewritten in place, pass after "
        "pass, for this many seconds per GPU (0 = off)",
    )
    hp.add_argument(
        "--hbm-mib",
        type=int,
        default=0,
        help="with --hbm-seconds, the memory the march covers, at least "
        "1024 (0 = all that is free less max(2 GiB, 2 %% of the total))",
    )
    hp.add_argument(
        "--selftest-mib",
        type=int,
        default=1024,
        help="HBM region to test per GPU (default 1024)",
    )
    hp.add_argument(
        "--json", action="store_true", help="one JSON record per GPU"
    )
    prof = sub.add_parser("profile")
    prof.add_argument("--host", default="127.0.0.1")
    prof.add_argument("--port", type=int, default=8083)
    prof.add_argument("--seconds", type=float, default=5.0)
    args = ap.parse_args(argv)
    if args.cmd == "health" and args.load_formats and not (
        args.selftest and args.load_seconds > 0
    ):
        ap.error("--load-formats needs --selftest and a positive --load-seconds")
    if args.cmd == "health":
        from .selftest import HBM_MIN_BYTES, MAX_LOAD_SECONDS

        if not 0 <= args.hbm_seconds <= MAX_LOAD_SECONDS:
            ap.error(f"--hbm-seconds must be in [0, {MAX_LOAD_SECONDS:g}]")
        if args.hbm_seconds > 0 and not args.selftest:
            ap.error("--hbm-seconds needs --selftest")
        if args.hbm_mib and not args.hbm_seconds > 0:
            ap.error("--hbm-mib needs a positive --hbm-seconds")
        if args.hbm_mib < 0 or 0 < args.hbm_mib < HBM_MIN_BYTES >> 20:
            ap.error("--hbm-mib must be 0 or at least 1024")
    return {
        "list": cmd_list,
        "topology": cmd_topology,
        "slice": cmd_slice,
        "partition": cmd_partition,
        "health": cmd_health,
        "labels": cmd_labels,
        "profile": cmd_profile,
    }[args.cmd](args)


if __name__ == "__main__":
    raise SystemExit(main())
