"""Demo workload CLI — the nbody-sample analog.

Runs inside claim-bearing pods: prints which devices the CDI injection made
visible, then optionally burns compute / measures bandwidth on them, so the
demo specs can validate sharing and partitioning exactly like the
reference's pods validate with ``nvidia-smi -L`` + the nbody benchmark
(reference gpu-test1.yaml:33-37, gpu-test5.yaml:53-87).
"""

from __future__ import annotations

import argparse
import glob
import json
import os
import sys


def visible_devices() -> dict:
    return {
        "kfd": os.path.exists("/dev/kfd"),
        "render_nodes": sorted(glob.glob("/dev/dri/renderD*")),
        "card_nodes": sorted(glob.glob("/dev/dri/card*")),
        "claim_uid": os.environ.get("AMD_DRA_CLAIM_UID", ""),
        "shared_session": os.environ.get("AMD_DRA_SHARED_SESSION", ""),
        "cu_mask": os.environ.get("HSA_CU_MASK", ""),
    }


def _allreduce_worker(rank, world, nelem, results):
    """One process per visible GPU; RCCL ring all-reduce over xGMI."""
    import os as _os
    import time

    import torch
    import torch.distributed as dist

    _os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    _os.environ.setdefault("MASTER_PORT", "29781")
    dist.init_process_group("nccl", rank=rank, world_size=world)
    torch.cuda.set_device(rank)
    x = torch.ones(nelem, dtype=torch.bfloat16, device=f"cuda:{rank}")
    for _ in range(3):  # warmup
        dist.all_reduce(x)
    torch.cuda.synchronize()
    iters = 20
    t0 = time.perf_counter()
    for _ in range(iters):
        dist.all_reduce(x)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    # ring all-reduce moves 2*(n-1)/n of the buffer per GPU per iteration
    bytes_moved = 2 * (world - 1) / world * nelem * 2 * iters
    # each all-reduce multiplies by world; bf16 rounds non-power-of-two
    # worlds, so compare with tolerance
    expected = float(world) ** (iters + 3)
    ok = bool(
        torch.allclose(
            x.float(),
            torch.full_like(x, expected, dtype=torch.float32),
            rtol=0.05,
        )
    )
    results[rank] = (bytes_moved / dt / 1e9, ok)
    dist.destroy_process_group()


def run_allreduce(size_mb: int) -> int:
    """RCCL all-reduce across every visible GPU (the xGMI fabric demo for
    multi-GPU topology claims, gpu-test7)."""
    import torch
    import torch.multiprocessing as mp

    world = torch.cuda.device_count()
    if world == 0:
        print("ERROR: no HIP devices", file=sys.stderr)
        return 1
    nelem = size_mb * 1024 * 1024 // 2  # bf16
    if world == 1:
        print("1 visible GPU: all-reduce is a no-op; device healthy")
        return 0
    with mp.Manager() as mgr:
        results = mgr.dict()
        mp.spawn(
            _allreduce_worker,
            args=(world, nelem, results),
            nprocs=world,
            join=True,
        )
        per_gpu = dict(results)
    for r, (gbps, ok) in sorted(per_gpu.items()):
        print(f"rank {r}: busbw {gbps:.1f} GB/s numerics_ok={ok}")
    return 0 if all(ok for _, ok in per_gpu.values()) else 1


def cu_footprint_rows(counts: dict, cu_mask: str) -> list:
    """One row per device for ``--cu-footprint``: ``(device, CUs seen, bits
    of this process's HSA_CU_MASK entry for that ordinal or None)``.
    ``counts`` is ``{device: CUs seen}``; an unparsable mask raises
    ``ValueError``."""
    from .sharing.footprint import parse_cu_mask, popcount

    masks = parse_cu_mask(cu_mask) if cu_mask else {}
    return [
        (d, counts[d], popcount(masks[d]) if d in masks else None)
        for d in sorted(counts)
    ]


def cu_footprint_exit_code(rows) -> int:
    """The verdict of ``--cu-footprint``: 1 when any device shows more CUs
    than its mask has bits, else 0. A device with no mask entry is allowed
    everything."""
    return int(any(bits is not None and seen > bits for _, seen, bits in rows))


def run_cu_footprint(hh) -> int:
    """Print, for every visible device, where this process's blocks run;
    exit code as :func:`cu_footprint_exit_code`."""
    cu_mask = os.environ.get("HSA_CU_MASK", "")
    reports = {d: hh.cu_footprint(d) for d in range(hh.device_count())}
    if not reports:
        print("ERROR: no HIP devices to measure", file=sys.stderr)
        return 1
    try:
        rows = cu_footprint_rows({d: r["count"] for d, r in reports.items()}, cu_mask)
    except ValueError as e:
        print(f"ERROR: {e}", file=sys.stderr)
        return 1
    for d, seen, bits in rows:
        r = reports[d]
        per_xcd = " ".join(f"{x}:{n}" for x, n in sorted(r["per_xcc"].items()))
        allowed = "no mask" if bits is None else f"mask allows {bits}"
        verdict = "EXCEEDS MASK" if bits is not None and seen > bits else "ok"
        print(
            f"device {d}: cu footprint {seen} of {r['multi_processor_count']} "
            f"CUs, per XCD {per_xcd}; {allowed}: {verdict}"
        )
    return cu_footprint_exit_code(rows)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser("amd-dra-workload")
    ap.add_argument("--list", action="store_true", help="print visible devices (nvidia-smi -L analog)")
    ap.add_argument("--benchmark", action="store_true", help="run bandwidth + MFMA probes")
    ap.add_argument("--burn-ms", type=int, default=0, help="occupancy burn duration")
    ap.add_argument(
        "--nbody",
        type=int,
        default=0,
        help="run the all-pairs n-body benchmark with this many bodies "
        "(the reference demo's nbody --benchmark analog)",
    )
    ap.add_argument(
        "--allreduce-mb",
        type=int,
        default=0,
        help="RCCL all-reduce of this buffer size across visible GPUs",
    )
    ap.add_argument(
        "--selftest",
        type=int,
        nargs="?",
        const=1024,
        default=0,
        metavar="MiB",
        help="fill and verify this much HBM (default 1024 MiB) with known "
        "patterns and run the MFMA known-answer test on every visible "
        "device; exit 1 on a mismatch",
    )
    ap.add_argument(
        "--cu-selftest",
        action="store_true",
        help="test the LDS and the matrix pipes of every compute unit of "
        "every visible device and name the CUs that fail; exit 1 on a "
        "mismatch",
    )
    ap.add_argument(
        "--load-selftest",
        type=float,
        default=0.0,
        metavar="SECONDS",
        help="run a tiled bf16 GEMM on exact data on every visible device "
        "for this long, compare every element of every iteration bit for "
        "bit and name the tiles and CUs that fail; exit 1 on a mismatch",
    )
    ap.add_argument(
        "--mx-selftest",
        nargs=2,
        default=None,
        metavar=("FORMAT", "SECONDS"),
        help="run a tiled GEMM on the block-scaled MFMA (FORMAT mxfp8 or "
        "mxfp4) on exact data on every visible device for SECONDS, compare "
        "every element of every iteration bit for bit and name the tiles and "
        "CUs that fail; exit 1 on a mismatch",
    )
    ap.add_argument(
        "--hbm-selftest",
        type=float,
        default=0.0,
        metavar="SECONDS",
        help="march over all free memory of every visible device (less "
        "max(2 GiB, 2 %% of the total)) for this long: every element is "
        "read, verified and rewritten in place, pass after pass; exit 1 on a "
        "mismatch",
    )
    ap.add_argument(
        "--cu-footprint",
        action="store_true",
        help="print which compute units this process's blocks run on, per "
        "device and per XCD, next to the size of its HSA_CU_MASK entry; "
        "exit 1 if a device shows more CUs than its mask allows",
    )
    args = ap.parse_args(argv)
    mx = None
    if args.mx_selftest:
        from k8s_dra_driver_amd.selftest import LOAD_FORMATS, MAX_LOAD_SECONDS

        fmt, seconds = args.mx_selftest
        if fmt not in LOAD_FORMATS:
            ap.error(f"--mx-selftest: FORMAT must be one of {', '.join(LOAD_FORMATS)}")
        try:
            seconds = float(seconds)
        except ValueError:
            ap.error("--mx-selftest: SECONDS must be a number")
        if not 0 < seconds <= MAX_LOAD_SECONDS:
            ap.error(f"--mx-selftest: SECONDS must be in (0, {MAX_LOAD_SECONDS:g}]")
        mx = (fmt, seconds)
    if args.hbm_selftest:
        from k8s_dra_driver_amd.selftest import MAX_LOAD_SECONDS

        if not 0 < args.hbm_selftest <= MAX_LOAD_SECONDS:
            ap.error(f"--hbm-selftest: SECONDS must be in (0, {MAX_LOAD_SECONDS:g}]")

    info = visible_devices()
    print(json.dumps(info))
    if not info["kfd"] or not info["render_nodes"]:
        print("ERROR: no GPU devices injected", file=sys.stderr)
        return 1
    rc = 0
    if (
        args.benchmark
        or args.burn_ms
        or args.nbody
        or args.selftest
        or args.cu_selftest
        or args.load_selftest
        or mx
        or args.hbm_selftest
        or args.cu_footprint
    ):
        from k8s_dra_driver_amd import _hiphealth

        n = _hiphealth.device_count()
        print(f"hip devices: {n}")
        if args.cu_footprint:
            rc = run_cu_footprint(_hiphealth) or rc
        for d in range(n):
            if args.benchmark:
                bw = _hiphealth.bandwidth_gbs(d, 256, 5)
                chk = _hiphealth.mfma_check(d)
                print(f"device {d}: bandwidth {bw:.0f} GB/s mfma_ok={chk['ok']}")
            if args.burn_ms:
                ms = _hiphealth.burn_ms(d, args.burn_ms)
                print(f"device {d}: burned {ms:.0f} ms")
            if args.nbody:
                r = _hiphealth.nbody_benchmark(d, args.nbody, 10)
                print(
                    f"device {d}: nbody {r['bodies']} bodies x {r['iters']} "
                    f"iters = {r['gflops']:.0f} GFLOP/s finite={r['finite']}"
                )
            if args.selftest:
                r = _hiphealth.selftest(d, mib=args.selftest)
                bad = sum(p["mismatches"] for p in r["memory"])
                print(
                    f"device {d}: selftest {'ok' if r['ok'] else 'FAILED'}: "
                    f"{args.selftest} MiB x 4 patterns, {bad} memory "
                    f"mismatch(es), mfma {r['mfma']['mismatches']} "
                    f"mismatch(es) in {r['mfma']['checked']} values"
                )
                if not r["ok"]:
                    rc = 1
            if args.cu_selftest:
                r = _hiphealth.cu_selftest(d)
                bad = ", ".join(
                    f"xcc {c['xcc']} se {c['se']} sh {c['sh']} cu {c['cu']}"
                    for c in r["bad_cus"]
                )
                print(
                    f"device {d}: cu-selftest {'ok' if r['ok'] else 'FAILED'}: "
                    f"{r['covered']} of {r['multi_processor_count']} CUs "
                    f"covered by {r['blocks']} blocks, lds "
                    f"{r['lds']['mismatches']} mismatch(es), mfma "
                    f"{r['mfma']['mismatches']} mismatch(es), "
                    f"{len(r['bad_cus'])} bad CU(s)" + (f": {bad}" if bad else "")
                )
                if not r["ok"]:
                    rc = 1
            if args.load_selftest:
                r = _hiphealth.load_selftest(d, seconds=args.load_selftest)
                bad = ", ".join(
                    f"xcc {c['xcc']} se {c['se']} sh {c['sh']} cu {c['cu']}"
                    for c in r["bad_cus"]
                )
                print(
                    f"device {d}: load-selftest {'ok' if r['ok'] else 'FAILED'}: "
                    f"{r['iterations']} iteration(s) of "
                    f"{r['m']}x{r['n']}x{r['k']} in {r['seconds']:.1f}s on "
                    f"{r['cus_seen']} CUs, {r['mismatches']} mismatch(es), "
                    f"checksum {'ok' if r['checksum_ok'] else 'FAILED'}, "
                    f"{r['tflops']:.0f} TF/s (informative), "
                    f"{len(r['bad_cus'])} bad CU(s)" + (f": {bad}" if bad else "")
                )
                if not r["ok"]:
                    rc = 1
            if mx:
                r = _hiphealth.mx_selftest(d, mx[0], mx[1])
                bad = ", ".join(
                    f"xcc {c['xcc']} se {c['se']} sh {c['sh']} cu {c['cu']}"
                    for c in r["bad_cus"]
                )
                print(
                    f"device {d}: mx-selftest {mx[0]} "
                    f"{'ok' if r['ok'] else 'FAILED'}: "
                    f"{r['iterations']} iteration(s) of "
                    f"{r['m']}x{r['n']}x{r['k']} in {r['seconds']:.1f}s on "
                    f"{r['cus_seen']} CUs, {r['mismatches']} mismatch(es), "
                    f"checksum {'ok' if r['checksum_ok'] else 'FAILED'}, "
                    f"{r['tflops']:.0f} TF/s (informative), "
                    f"{len(r['bad_cus'])} bad CU(s)" + (f": {bad}" if bad else "")
                )
                if not r["ok"]:
                    rc = 1
            if args.hbm_selftest:
                r = _hiphealth.hbm_selftest(d, seconds=args.hbm_selftest)
                bad = ", ".join(f"chunk {c} block {p}" for c, p in r["bad_pages_first"])
                print(
                    f"device {d}: hbm-selftest {'ok' if r['ok'] else 'FAILED'}: "
                    f"{r['passes']} pass(es) over {r['bytes'] / 2**30:.1f} GiB "
                    f"in {r['chunks']} chunk(s)"
                    f"{' (allocation fell short)' if r['alloc_short'] else ''} "
                    f"in {r['seconds']:.1f}s, {r['mismatches']} mismatch(es), "
                    f"flipped bits 0x{r['flipped_or']:016x}, march "
                    f"{r['gbs']['march_hash']:.0f} GB/s (informative), "
                    f"{r['bad_pages']} bad 2 MiB block(s)" + (f": {bad}" if bad else "")
                )
                if not r["ok"]:
                    rc = 1
    if args.allreduce_mb:
        return run_allreduce(args.allreduce_mb) or rc
    return rc


if __name__ == "__main__":
    raise SystemExit(main())
