#!/usr/bin/env python3
"""Where a pod lifecycle's time goes, phase by phase.

``bench.py --dump-profile`` samples ``sys._current_frames()`` from a Python
thread, which only runs while it holds the GIL: it sees threads parked in
syscalls and gRPC waits, and almost none of the pure-Python CPU time. This
tool instead brackets each phase of the benchmark's own lifecycle with
``perf_counter`` and prints the median per phase:

  make claim / allocate / put / prepare RPC / unprepare RPC
      the five steps of ``BenchRank._one_lifecycle`` (config ``whole``)
  driver.node_prepare_resources, driver.node_unprepare_resources
      the same claims through the Driver, no gRPC
  state.prepare, state.unprepare
      ``DeviceState`` alone: config decode, CDI spec, checkpoint

The three groups are measured in separate passes over fresh claims, so
RPC cost = prepare RPC - driver.node_prepare_resources, and the Driver's
own overhead = driver.* - state.*.

    python scripts/lifecycle_breakdown.py --hal amdsmi --lifecycles 3000
"""

from __future__ import annotations

import argparse
import gc
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import bench  # noqa: E402
from k8s_dra_driver_amd.plugin.driver import ClaimRef  # noqa: E402


def _med_us(xs) -> float:
    return round(statistics.median(xs) * 1e6, 1)


def measure(rank: "bench.BenchRank", n: int) -> dict:
    pc = time.perf_counter
    phases: dict = {}

    def rec(name, dt):
        phases.setdefault(name, []).append(dt)

    # pass 1: the benchmark's lifecycle, step by step
    for _ in range(n):
        uid = rank._next_uid("b")
        t0 = pc()
        claim = bench.make_claim_spec(uid, "whole")
        t1 = pc()
        rank.allocator.allocate_into_claim(
            claim, rank.devices, pool=rank.node, node_name=rank.node
        )
        t2 = pc()
        rank.kube.put_resource_claim(claim)
        t3 = pc()
        rank._grpc_prepare([uid])
        t4 = pc()
        rank._grpc_unprepare([uid])
        t5 = pc()
        rec("make claim", t1 - t0)
        rec("allocate", t2 - t1)
        rec("put", t3 - t2)
        rec("prepare RPC", t4 - t3)
        rec("unprepare RPC", t5 - t4)
        rec("lifecycle", t5 - t0)

    # pass 2: Driver entry points called directly (no gRPC)
    driver = rank.driver
    for _ in range(n):
        uid = rank._next_uid("d")
        claim = bench.make_claim_spec(uid, "whole")
        rank._alloc_and_put(claim)
        ref = [ClaimRef("default", f"claim-{uid}", uid)]
        t0 = pc()
        res = driver.node_prepare_resources(ref)
        t1 = pc()
        driver.node_unprepare_resources(ref)
        t2 = pc()
        if res[uid].error:
            raise RuntimeError(res[uid].error)
        rec("driver.node_prepare_resources", t1 - t0)
        rec("driver.node_unprepare_resources", t2 - t1)

    # pass 3: DeviceState alone
    state = driver.state
    for _ in range(n):
        uid = rank._next_uid("s")
        claim = bench.make_claim_spec(uid, "whole")
        rank.allocator.allocate_into_claim(
            claim, rank.devices, pool=rank.node, node_name=rank.node
        )
        t0 = pc()
        state.prepare(claim)
        t1 = pc()
        state.unprepare(uid)
        t2 = pc()
        rec("state.prepare", t1 - t0)
        rec("state.unprepare", t2 - t1)

    return {k: _med_us(v) for k, v in phases.items()}


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--hal", choices=["auto", "amdsmi", "fake"], default="auto")
    ap.add_argument("--lifecycles", type=int, default=3000)
    ap.add_argument("--no-pin", action="store_true")
    ap.add_argument("--json", action="store_true", help="one JSON line only")
    args = ap.parse_args()
    pinned = "" if args.no_pin else bench.pin_to_one_l3()

    # BenchRank warms its own pipeline for PIPELINE_WARMUP_S on construction
    rank = bench.BenchRank(0, target_gpu=0, config="whole", hal_mode=args.hal)
    try:
        gc.collect()
        gc.freeze()
        med = measure(rank, args.lifecycles)
        hal = rank.hal_kind
    finally:
        rank.close()

    try:
        from k8s_dra_driver_amd.utils import atomicfile

        native = bool(getattr(atomicfile, "native", lambda: None)())
    except Exception:
        native = False
    out = {
        "hal": hal,
        "lifecycles": args.lifecycles,
        "cpus": pinned or "unpinned",
        "native_claimio": native,
        "median_us": med,
    }
    if args.json:
        print(json.dumps(out))
        return 0
    print(
        f"hal={hal} lifecycles/pass={args.lifecycles} cpus={out['cpus']} "
        f"native_claimio={native}"
    )
    print(f"{'phase':<36}{'median us':>10}")
    for k, v in med.items():
        print(f"{k:<36}{v:>10.1f}")
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
