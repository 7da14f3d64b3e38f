"""Probe: the route delta of EVERY node for a link flap on the full fabric,
as routes (not counts): the packed path against the per-node loop.

The flap is the one of route_delta_flap_probe.py (one RSW-FSW link down).
After the mapped diff:

  (a) AllNodesRouteTable::deltas() (deltas_timed, C++ wall time, no Python
      conversion), split into the pack call (count, scan, fill on the device),
      the fetch of the packed list, the two sparse cell gathers for the MPLS
      candidates, and the host assembly;
  (b) the delta(node) loop in C++ over the nodes with a changed column: all
      of them if the loop fits the probe's time budget, else a fixed seeded
      sample of at least 200 of them, scaled to all (the sample size is in
      the output).

One process, 3 warm-ups, then (a) and (b) alternating per timed round.  Bytes
copied from the device are counted from shapes on the host for both paths.

  python profiles/route_delta_all_probe.py [--nodes 10000] [--rounds 5]
      [--budget-s 240] [--out DIR]
"""
import argparse
import json
import os
import random
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from openr_amd import topologies as TP  # noqa: E402

WARM, SAMPLE = 3, 200


def _stats(xs):
    xs = sorted(xs)
    return {"median": round(statistics.median(xs), 3), "min": round(xs[0], 3),
            "max": round(xs[-1], 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=10000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--budget-s", type=float, default=240.0,
                    help="time the per-node loops may take over all rounds")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    torch.cuda.init()
    import openr_amd._openr_spf as E

    topo = TP.fabric(args.nodes)
    areas = E.AreaLinkStates()
    ls = areas.add("0")
    dbs = topo.adj_dbs()
    for db in dbs:
        ls.updateAdjacencyDatabase(db)
    ps = E.PrefixState()
    for pdb in topo.prefix_dbs("0"):
        ps.updatePrefixDatabase(pdb)
    base = E.AllNodesRouteTable(areas, "0", ps, True)

    by = {db.thisNodeName: db for db in dbs}
    rsw = next(n for n in topo.names if n.startswith("3-"))
    adj = next(a for a in by[rsw].adjacencies if a.otherNodeName.startswith("2-"))
    fsw = adj.otherNodeName
    back = next(a for a in by[fsw].adjacencies
                if a.otherNodeName == rsw and a.ifName == adj.otherIfName)
    by[rsw].adjacencies.remove(adj)
    by[fsw].adjacencies.remove(back)
    ls.updateAdjacencyDatabase(by[rsw])
    ls.updateAdjacencyDatabase(by[fsw])
    flap = E.AllNodesRouteTable(areas, "0", ps, True)
    print("tables built", file=sys.stderr, flush=True)

    changed = flap.diff(base)
    assert flap.diff_was_mapped
    changed_nodes = [flap.node_name(i) for i, c in enumerate(changed) if c]
    sample = sorted(random.Random(9).sample(changed_nodes, min(SAMPLE, len(changed_nodes))))

    # warm-ups; the first one decides whether (b) can run over every changed node
    loop_nodes = sample
    for k in range(WARM):
        flap.deltas_timed()
        _, us, _ = flap.delta_loop_timed(loop_nodes)
        if k == 0:
            full_s = us / 1e6 / len(sample) * len(changed_nodes)
            if full_s * (WARM - 1 + args.rounds) <= args.budget_s:
                loop_nodes = changed_nodes
        print(f"warm-up {k}: loop over {len(loop_nodes)} nodes next", file=sys.stderr, flush=True)
    scale = len(changed_nodes) / len(loop_nodes)

    a_ms, a_parts, b_ms = [], {"pack": [], "fetch": [], "gather": [], "assemble": []}, []
    a_last = b_routes = b_bytes = None
    for _ in range(args.rounds):
        d = flap.deltas_timed()
        a_ms.append(d["us"] / 1e3)
        for k in a_parts:
            a_parts[k].append(d[k + "_us"] / 1e3)
        a_last = d
        b_routes, us, b_bytes = flap.delta_loop_timed(loop_nodes)
        b_ms.append(us / 1e3 * scale)
        print(f"round: (a) {a_ms[-1]:.1f} ms, (b) {b_ms[-1]:.0f} ms", file=sys.stderr, flush=True)

    out = {
        "what": "route delta of every node for one RSW-FSW link down on the fabric: "
                "(a) deltas() from one packed fetch vs (b) the delta(node) loop over the "
                "changed nodes",
        "nodes": flap.num_nodes, "prefixes": flap.num_prefixes,
        "label_columns": flap.num_label_columns, "link": [rsw, fsw],
        "warmups": WARM, "timed_rounds": args.rounds,
        "changed_cells": int(sum(changed)), "nodes_with_changes": len(changed_nodes),
        "a_deltas_ms": _stats(a_ms),
        "a_parts_ms": {k: _stats(v) for k, v in a_parts.items()},
        "a_ms_each": [round(x, 3) for x in a_ms],
        "a_sizes": {k: int(a_last[k]) for k in ("cells", "gone", "link_words", "link_metrics",
                                                  "newer_cells", "older_cells", "routes", "nodes")},
        "a_bytes_from_device": int(a_last["bytes"]),
        "b_loop_nodes": len(loop_nodes), "b_is_sample": loop_nodes is sample,
        "b_scale": round(scale, 4),
        "b_delta_loop_ms_all_changed_nodes": _stats(b_ms),
        "b_ms_each": [round(x, 1) for x in b_ms],
        "b_routes_in_loop": int(b_routes),
        "b_bytes_from_device_all_changed_nodes": int(b_bytes * scale),
        "b_over_a_median": round(statistics.median(b_ms) / statistics.median(a_ms), 1),
    }
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "route_delta_all.json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
