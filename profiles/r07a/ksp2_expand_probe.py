"""Probe: bench.py's KSP2 rebuild loop (fabric, 2-0-0) in this process, one
JSON line: build ms, loop ms and the per-build counters bench.py's
ksp2_route_db section prints, plus the two the device expansion adds
(kth_expand_us, ksp2_device_expanded).  argv[1] = the tree to import
(default: this checkout), argv[2] = a tag for the line.  The caller sets
OPENR_KSP2_DEVICE_EXPAND; run one process per variant, alternating."""
import json
import os
import sys

ROOT = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.dirname(
    os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import torch  # noqa: E402,F401

import bench  # noqa: E402
import openr_amd._openr_spf as E  # noqa: E402
from openr_amd import topologies as TP  # noqa: E402

assert os.path.abspath(bench.__file__).startswith(ROOT), bench.__file__
snap = {}
parity = bench._routedb_parity


def parity_with_snapshot(*a, **k):
    snap.update(E.get_counters())  # the timed builds' counters, before the check's
    return parity(*a, **k)


bench._routedb_parity = parity_with_snapshot
topo = TP.fabric(10000)
r = bench.ksp2_route_db(topo, 0, iters=int(os.environ.get("PROBE_ITERS", "2")))
n = max(1, snap.get("decision.route_build_runs", 1))
pb = r["per_build"]
print(json.dumps({
    "tag": sys.argv[2] if len(sys.argv) > 2 else "",
    "expand_env": os.environ.get("OPENR_KSP2_DEVICE_EXPAND"),
    "build_ms_median": r.get("build_ms_median"), "ms_median": r.get("ms_median"),
    "ksp2_nexthops_us": pb.get("ksp2_nexthops_us"), "ksp2_paths_us": pb.get("ksp2_paths_us"),
    "kth_trace_us": pb.get("kth_trace_us"), "kth2_device_trace_us": pb.get("kth2_device_trace_us"),
    "kth_fill_us": pb.get("kth_fill_us"), "route_prefetch_us": pb.get("route_prefetch_us"),
    "kth_expand_us": round(snap.get("decision.kth_expand_us", 0) / n, 1),
    "ksp2_device_expanded": round(snap.get("decision.ksp2_device_expanded", 0) / n, 1),
    "builds": n, "parity": r.get("parity_check")}), flush=True)
