"""Probe: the network-wide route delta of a link flap on the full fabric.

  (a) the mapped diff (spf_route_table_diff_mapped) of the table with one
      RSW-FSW link down against the base table: two rows leave the identity
      link path, every other row takes the straight word compare;
  (b) spf_route_table_diff on a drain pair of the same size (one RSW
      overloaded), in the same process -- the equal-layout kernel, the
      baseline;
  (c) what a caller without the diff has to do: routes(node) on both tables,
      timed in C++ for 100 sampled nodes.

20 timed calls after 3 warm-ups, (a) and (b) alternating, medians.  "call" is
the C ABI call alone (maps already built; upload, kernel, count copy, sync);
"host" is AllNodesRouteTable::diff, which for (a) also builds the maps.

  python profiles/route_delta_flap_probe.py [--nodes 10000] [--out DIR]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from openr_amd import topologies as TP  # noqa: E402

WARM, TIMED, SAMPLE = 3, 20, 100


def _stats(xs):
    xs = sorted(xs)
    return {"median": round(statistics.median(xs), 4), "min": round(xs[0], 4),
            "max": round(xs[-1], 4), "p25": round(xs[len(xs) // 4], 4),
            "p75": round(xs[(3 * len(xs)) // 4], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=10000)
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
    # the RSW drained (same layout as the base): the pair of (b)
    by[rsw].isOverloaded = True
    ls.updateAdjacencyDatabase(by[rsw])
    drain = E.AllNodesRouteTable(areas, "0", ps, True)
    # undrained again, the link down: both ends withdraw the adjacency
    by[rsw].isOverloaded = False
    by[rsw].adjacencies.remove(adj)
    by[fsw].adjacencies.remove(back)
    ls.updateAdjacencyDatabase(by[rsw])
    ls.updateAdjacencyDatabase(by[fsw])
    flap = E.AllNodesRouteTable(areas, "0", ps, True)

    a_call, a_host, b_call, b_host = [], [], [], []
    ca = cb = None
    for k in range(WARM + TIMED):
        for table, call, host in ((flap, a_call, a_host), (drain, b_call, b_host)):
            t0 = time.perf_counter()
            changed = table.diff(base)
            ms = (time.perf_counter() - t0) * 1e3
            if k >= WARM:
                call.append(table.diff_call_ms)
                host.append(ms)
            if table is flap:
                ca = changed
            else:
                cb = changed
    assert flap.diff_was_mapped and not drain.diff_was_mapped

    names = sorted(topo.names)
    sample = names[:: max(1, len(names) // SAMPLE)][:SAMPLE]
    us_new = us_old = 0.0
    routes = 0
    for node in sample:
        n1, u1 = flap.routes_timed(node)
        n0, u0 = base.routes_timed(node)
        us_new += u1
        us_old += u0
        routes += n1 + n0
    c_ms = (us_new + us_old) / 1e3
    # the ends of the link are the only rows off the identity path
    upd_r, del_r = flap.delta(rsw)
    out = {
        "what": "route delta of one RSW-FSW link down on the fabric: mapped diff (a) vs the "
                "equal-layout diff of a drain pair (b) vs materialising routes(node) twice (c)",
        "nodes": flap.num_nodes, "prefixes": flap.num_prefixes,
        "label_columns": flap.num_label_columns, "link": [rsw, fsw],
        "warmups": WARM, "timed_calls": TIMED,
        "a_mapped_diff_call_ms": _stats(a_call), "a_mapped_diff_host_ms": _stats(a_host),
        "b_plain_diff_call_ms": _stats(b_call), "b_plain_diff_host_ms": _stats(b_host),
        "a_call_ms_each": [round(x, 4) for x in a_call],
        "b_call_ms_each": [round(x, 4) for x in b_call],
        "a_changed_cells": int(sum(ca)), "a_nodes_with_changes": int(sum(1 for c in ca if c)),
        "b_changed_cells": int(sum(cb)), "b_nodes_with_changes": int(sum(1 for c in cb if c)),
        "rsw_delta": {"updates": len(upd_r), "deletes": len(del_r)},
        "c_routes_both_tables_ms": {"sampled_nodes": len(sample), "routes": routes,
                                    "total_ms": round(c_ms, 2),
                                    "per_node_ms": round(c_ms / len(sample), 4),
                                    "all_nodes_ms_extrapolated":
                                        round(c_ms / len(sample) * flap.num_nodes, 1)},
    }
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "route_delta_flap.json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
