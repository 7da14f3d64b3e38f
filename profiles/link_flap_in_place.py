"""Measurement: one link going down and coming back, applied to a resident
all-nodes route table in place (AllNodesRouteTable with links_in_place:
apply_topology_changes -> spf_graph_set_edges, a new all-sources query, one
spf_route_table_refresh_rows) against the path it replaces, in the same run: a
fresh AllNodesRouteTable of the state after the event plus diff (through the
maps) against a table of the state before.

Workloads: the 10k fabric (the RSW 3-0-0 - FSW 2-0-0 link of DESIGN.md §6,
"Route delta of a link flap") and one link of the WAN-10k topology, one prefix
per node, LFA off.  Each round takes the link down and brings it back; per
event (a) and (b) run one after the other on the same LinkState.  3 warm-up
rounds, then --reps timed ones; median and min-max of

  (a) apply_wall_ms, spf_ms, refresh_ms, listed_rows, changed_routes
  (b) table_wall_ms (the fresh table), diff_wall_ms, their sum, spf_ms,
      route_ms, changed_routes
  engine_wall_ms  LinkState's own engine graph following the update (forced
                  before either path, common to both)

Both sides must report the same number of changed routes (asserted).

  python profiles/link_flap_in_place.py [--nodes N] [--reps R] [--out FILE]
                                        [--topologies fabric,wan]
"""
import argparse
import copy
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from openr_amd import topologies as TP  # noqa: E402

WARM = 3


def ms_since(t0):
    return (time.perf_counter() - t0) * 1e3


def stats(xs):
    xs = sorted(xs)
    return {"median": round(statistics.median(xs), 4), "min": round(xs[0], 4),
            "max": round(xs[-1], 4)}


def flap(topo, pick, reps):
    import openr_amd._openr_spf as E

    E.set_spf_device(0)
    areas = E.AreaLinkStates()
    ls = areas.add("0")
    dbs = {db.thisNodeName: db for db in topo.adj_dbs()}
    for db in dbs.values():
        ls.updateAdjacencyDatabase(db)
    ps = E.PrefixState()
    for db in topo.prefix_dbs("0"):
        ps.updatePrefixDatabase(db)
    u, adj = pick(dbs)
    v = adj.otherNodeName
    back = next(a for a in dbs[v].adjacencies
                if a.otherNodeName == u and a.ifName == adj.otherIfName)
    t = E.AllNodesRouteTable(areas, "0", ps, True, False, links_in_place=True)

    def down():
        dbs[u].adjacencies.remove(adj)
        dbs[v].adjacencies.remove(back)

    def up():
        dbs[u].adjacencies.append(adj)
        dbs[v].adjacencies.append(back)

    out = {"nodes": t.num_nodes, "prefixes": t.num_prefixes, "link": [u, v],
           "warmups": WARM, "timed_rounds": reps}
    acc = {"down": [], "up": []}
    for r in range(WARM + reps):
        for name, edit in (("down", down), ("up", up)):
            older = E.AllNodesRouteTable(areas, "0", ps, True, False)  # (b)'s state before
            edit()
            for n in (u, v):
                ls.updateAdjacencyDatabase(copy.deepcopy(dbs[n]))
            # LinkState refreshes its own engine graph on first use after an
            # update: whichever path ran first would pay for it, so it is
            # forced (one cached SPF) and timed apart from both
            t0 = time.perf_counter()
            ls.prefetchSpf([u], True)
            w_engine = ms_since(t0)
            t0 = time.perf_counter()
            counts = t.apply_topology_changes(areas, "0")
            m = {"engine_wall_ms": w_engine, "a_apply_wall_ms": ms_since(t0),
                 "a_spf_ms": t.spf_ms, "a_refresh_ms": t.refresh_ms,
                 "a_listed_rows": t.refresh_rows, "a_changed_routes": int(sum(counts)),
                 "down_links": t.down_links}
            t0 = time.perf_counter()
            fresh = E.AllNodesRouteTable(areas, "0", ps, True, False)
            m["b_table_wall_ms"] = ms_since(t0)
            t0 = time.perf_counter()
            c2 = fresh.diff(older)
            m["b_diff_wall_ms"] = ms_since(t0)
            m["b_wall_ms"] = m["b_table_wall_ms"] + m["b_diff_wall_ms"]
            m["b_diff_call_ms"] = fresh.diff_call_ms
            m["b_spf_ms"], m["b_route_ms"] = fresh.spf_ms, fresh.route_ms
            m["b_changed_routes"] = int(sum(c2))
            assert fresh.diff_was_mapped
            assert m["a_changed_routes"] == m["b_changed_routes"], (name, m)
            assert list(c2) == list(counts), name
            del fresh, older
            if r >= WARM:
                acc[name].append(m)
    for name, ms in acc.items():
        out[name] = {k: stats([m[k] for m in ms]) for k in ms[0]}
        print(name, out[name], file=sys.stderr, flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--topologies", default="fabric,wan")
    args = ap.parse_args()

    import torch

    torch.cuda.init()
    result = {"gpu": torch.cuda.get_device_name(0)}

    def fabric_link(dbs):
        rsw = next(n for n in sorted(dbs) if n.startswith("3-"))
        return rsw, next(a for a in dbs[rsw].adjacencies if a.otherNodeName.startswith("2-"))

    def wan_link(dbs):
        names = sorted(dbs)
        n = names[len(names) // 3]
        return n, dbs[n].adjacencies[0]

    for kind in args.topologies.split(","):
        topo = TP.fabric(args.nodes) if kind == "fabric" else TP.wan(args.nodes, 10 * args.nodes)
        res = flap(topo, fabric_link if kind == "fabric" else wan_link, args.reps)
        res["topology"] = f"{kind}({args.nodes})"
        result[kind] = res
    line = json.dumps(result)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
