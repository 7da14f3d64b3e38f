"""Measurement: prefix churn applied to a resident all-nodes route table in
place (AllNodesRouteTable.apply_prefix_changes -> one
spf_route_table_patch_columns) against the only other route to the same
delta: a fresh AllNodesRouteTable, diff, deltas().

Host level ("host" in the output), on the 10k fabric with spare_columns=64.
Three events, each published with PrefixState.updatePrefixDatabase:

  new_prefix      one RSW announces one new /128
  node_withdrawn  one RSW's whole prefix database withdrawn
  announce_64     64 RSWs announce one new /128 each, one merged call

Per event, medians over --reps repetitions after one warm-up (every
repetition is followed by the inverse event, untimed, so the table returns to
the base state and the columns are reused):

  patch_ms        device time of the patch (bitmap clear + spf_route_patch_kernel)
  apply_wall_ms   apply_prefix_changes: rescan, classification, the ABI call,
                  host bookkeeping
  deltas_wall_ms  deltas() in C++ (deltas_timed): pack, fetch, assembly of
                  every node's DecisionRouteUpdate
  rebuild         the same delta the other way, in the same run: a fresh
                  AllNodesRouteTable of the state after the event (graph, SPF,
                  prefix scan, route kernel), diff against the base table,
                  deltas()

ABI level ("abi"): the same three shapes through the C ABI on one resident
query, with spf_route_table_kernel timed on a side table of the event's k
columns alone (what recomputing them costs without the fused compare).

  python profiles/prefix_churn.py [--nodes N] [--reps R] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from openr_amd import abi  # noqa: E402
from openr_amd import topologies as TP  # noqa: E402

SPARE = 64


def ms_since(t0):
    return (time.perf_counter() - t0) * 1e3


def kernel_ms(t):
    ms = C.c_float()
    abi._check(abi.load().spf_route_table_elapsed_ms(t.h, C.byref(ms)), "elapsed_ms")
    return float(ms.value)


def med(xs):
    return round(statistics.median(xs), 4)


def measure(q, t, ann, cols, lists, reps):
    old = [ann[c] for c in cols]
    patch_ms, patch_wall, pack_wall, cells = [], [], [], 0
    for r in range(reps + 1):  # the first pair warms up
        t0 = time.perf_counter()
        counts = t.patch_columns(cols, lists)
        w = ms_since(t0)
        d = t.patch_ms()
        t0 = time.perf_counter()
        pk = t.delta_pack()
        p = ms_since(t0)
        cells = int(counts.sum())
        assert pk["cells"] == cells
        t.patch_columns(cols, old)
        if r:
            patch_ms.append(d)
            patch_wall.append(w)
            pack_wall.append(p)
    side = []
    s = abi.RouteTable(q, lists)
    for r in range(reps + 1):
        s.run()
        side.append(kernel_ms(s))
    s.close()
    ann2 = list(ann)
    for c, l in zip(cols, lists):
        ann2[c] = l
    build, route, diff, pack2 = [], [], [], []
    for r in range(3):
        t0 = time.perf_counter()
        n = abi.RouteTable(q, ann2).run()
        rk = kernel_ms(n)  # waits for the run
        build.append(ms_since(t0))
        route.append(rk)
        t0 = time.perf_counter()
        counts = n.diff(t)
        diff.append(ms_since(t0))
        t0 = time.perf_counter()
        pk = n.delta_pack()
        pack2.append(ms_since(t0))
        assert int(counts.sum()) == cells == pk["cells"]
        n.close()
    return {
        "columns": len(cols), "changed_cells": cells,
        "patch_ms": med(patch_ms), "patch_wall_ms": med(patch_wall), "pack_wall_ms": med(pack_wall),
        "side_kernel_ms": med(side[1:]),
        "rebuild": {"create_run_wall_ms": med(build[1:]), "route_kernel_ms": med(route[1:]),
                    "diff_wall_ms": med(diff[1:]), "pack_wall_ms": med(pack2[1:])},
    }


def host_level(topo, reps):
    import openr_amd._openr_spf as E
    from openr_amd import thrift as T

    E.set_spf_device(0)
    areas = E.AreaLinkStates()
    ls = areas.add("0")
    for db in topo.adj_dbs():
        ls.updateAdjacencyDatabase(db)
    ps = E.PrefixState()
    pdbs = {db.thisNodeName: db for db in topo.prefix_dbs("0")}
    for db in pdbs.values():
        ps.updatePrefixDatabase(db)
    base = E.AllNodesRouteTable(areas, "0", ps, True, False)  # the state every event starts from
    t = E.AllNodesRouteTable(areas, "0", ps, True, False, spare_columns=SPARE)
    rsw = sorted(n for n in pdbs if n.startswith("3-"))
    rng = np.random.RandomState(1)
    many = [rsw[int(i)] for i in rng.choice(len(rsw), size=SPARE, replace=False)]

    def entry(k):
        return T.createPrefixEntry(T.toIpPrefix(f"fc77::{k + 1:x}/128"))

    def announce(nodes):
        saved = {n: list(pdbs[n].prefixEntries) for n in nodes}
        for k, n in enumerate(nodes):
            pdbs[n].prefixEntries = saved[n] + [entry(k)]
        return saved

    def withdraw(nodes):
        saved = {n: list(pdbs[n].prefixEntries) for n in nodes}
        for n in nodes:
            pdbs[n].prefixEntries = []
        return saved

    def publish(nodes):
        changed = set()
        for n in nodes:
            changed |= set(ps.updatePrefixDatabase(pdbs[n]))
        return changed

    events = {
        "new_prefix": (announce, [rsw[7]]),
        "node_withdrawn": (withdraw, [rsw[len(rsw) // 2]]),
        "announce_64": (announce, many),
    }
    out = {"prefixes": t.num_prefixes, "nodes": t.num_nodes}
    for name, (edit, nodes) in events.items():
        patch_ms, apply_wall, deltas_wall, build, diff, deltas2 = [], [], [], [], [], []
        routes = cols = 0
        for r in range(reps + 1):
            saved = edit(nodes)
            changed = publish(nodes)
            t0 = time.perf_counter()
            counts = t.apply_prefix_changes(ps, changed)
            w = ms_since(t0)
            pm = t.patch_ms
            d = t.deltas_timed()
            assert d["routes"] == sum(counts)
            routes, cols = int(d["routes"]), len(changed)
            fresh_ms = diff_ms = 0.0
            if r <= 3:  # (the rebuild side: three samples are enough for tens of ms)
                t0 = time.perf_counter()
                fresh = E.AllNodesRouteTable(areas, "0", ps, True, False)
                fresh_ms = ms_since(t0)
                t0 = time.perf_counter()
                c2 = fresh.diff(base)
                diff_ms = ms_since(t0)
                d2 = fresh.deltas_timed()
                assert sum(c2) == sum(counts) and d2["routes"] == d["routes"]
                del fresh
            for n in nodes:  # the inverse event, untimed
                pdbs[n].prefixEntries = saved[n]
            t.apply_prefix_changes(ps, publish(nodes))
            if r:
                patch_ms.append(pm)
                apply_wall.append(w)
                deltas_wall.append(d["us"] / 1e3)
                if r <= 3:
                    build.append(fresh_ms)
                    diff.append(diff_ms)
                    deltas2.append(d2["us"] / 1e3)
        out[name] = {
            "changed_prefixes": cols, "changed_routes": routes,
            "patch_ms": med(patch_ms), "apply_wall_ms": med(apply_wall),
            "deltas_wall_ms": med(deltas_wall),
            "rebuild": {"table_wall_ms": med(build), "diff_wall_ms": med(diff),
                        "deltas_wall_ms": med(deltas2)},
        }
        print("host", name, out[name], file=sys.stderr, flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    torch.cuda.init()
    topo = TP.fabric(args.nodes)
    _, names = topo.rank()
    V = len(names)
    g = abi.Graph(topo.csr())
    q = g.query(np.arange(V, dtype=np.uint32), abi.SPF_F_NEXTHOPS).run()
    ann = [[v // 2] for v in range(2 * V)] + [[] for _ in range(SPARE)]
    P = len(ann)
    t = abi.RouteTable(q, ann).run()
    rsw = [i for i, n in enumerate(names) if n.startswith("3-")]
    rng = np.random.RandomState(1)
    spare = list(range(2 * V, P))
    x = rsw[len(rsw) // 2]
    events = {
        "new_prefix": ([spare[0]], [[rsw[7]]]),
        "node_withdrawn": ([2 * x, 2 * x + 1], [[], []]),
        "announce_64": (spare, [[int(a)] for a in rng.choice(rsw, size=SPARE)]),
    }
    result = {"topology": f"fabric({args.nodes})", "nodes": V, "columns": P, "spare_columns": SPARE,
              "gpu": torch.cuda.get_device_name(0), "reps": args.reps,
              "full_route_kernel_ms": round(kernel_ms(t), 3)}
    result["abi"] = {}
    for name, (cols, lists) in events.items():
        result["abi"][name] = measure(q, t, ann, cols, lists, args.reps)
        print("abi", name, result["abi"][name], file=sys.stderr, flush=True)
    t.close()
    q.close()
    g.close()
    result["host"] = host_level(topo, args.reps)
    line = json.dumps(result)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
