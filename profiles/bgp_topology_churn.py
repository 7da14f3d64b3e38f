"""Measurement: topology churn applied in place to a resident all-nodes route
table WITH BGP columns under bgpUseIgpMetric (selected columns, bgp_in_place;
AllNodesRouteTable.apply_topology_changes -> graph patch, all-sources SPF
re-run, one spf_route_table_refresh_rows_sel that folds every selected column
of the listed rows again) against the path it replaces: a fresh table of the
state after the event plus its (mapped) diff against a table of the state
before.

Workload: the 10k fabric with one loopback per node and the 512 BGP prefixes of
profiles/bgp_igp_table.py (four random RSW announcers each, one tie-breaker
entity, so the IGP cost decides first), LFA off.  Events, each from the state
the previous one left, on one resident table built with links_in_place:

  metric_raised / metric_lowered   one RSW uplink's metric (one direction)
  node_drained / node_undrained    one RSW that announces a BGP prefix
  link_down / link_up              one RSW - FSW link withdrawn and announced again

Per event, median / min / max over --reps repetitions after WARM warm-ups:

  apply_wall_ms     apply_topology_changes
  spf_ms            device time of the new all-sources query
  refresh_ms        device time of the refresh (bitmap clear + spf_route_refresh_kernel<true>)
  listed_rows, changed_routes
  engine_wall_ms    LinkState's own engine graph following the update (forced
                    before either path, common to both)
  b_table_wall_ms / b_diff_wall_ms / b_wall_ms   the fresh table, its diff, their sum

Both paths must report the same changed counts (asserted).

  python profiles/bgp_topology_churn.py [--nodes N] [--reps R] [--out FILE]
"""
import argparse
import copy
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from openr_amd import topologies as TP  # noqa: E402
from profiles.bgp_igp_table import N_ANNOUNCERS, N_BGP, prefix_dbs  # noqa: E402
from profiles.link_flap_in_place import ms_since, stats  # noqa: E402

WARM = 2


def churn(topo, reps):
    import openr_amd._openr_spf as E

    E.set_spf_device(0)
    areas = E.AreaLinkStates()
    ls = areas.add("0")
    dbs = {db.thisNodeName: db for db in topo.adj_dbs()}
    for db in dbs.values():
        ls.updateAdjacencyDatabase(db)
    ps = E.PrefixState()
    announcers = set()
    for pdb in prefix_dbs(topo):
        ps.updatePrefixDatabase(pdb)
        if len(pdb.prefixEntries) > 1:
            announcers.add(pdb.thisNodeName)

    def table(**kw):
        return E.AllNodesRouteTable(areas, "0", ps, True, False, bgp_columns=True,
                                    bgp_use_igp_metric=True, **kw)

    # an RSW that announces a BGP prefix: its first uplink moves, it is drained,
    # and its link to an FSW goes down and comes back
    u = next(n for n in sorted(dbs) if n.startswith("3-") and n in announcers)
    adj = next(a for a in dbs[u].adjacencies if a.otherNodeName.startswith("2-"))
    v = adj.otherNodeName
    back = next(a for a in dbs[v].adjacencies
                if a.otherNodeName == u and a.ifName == adj.otherIfName)
    t = table(bgp_in_place=True, links_in_place=True)

    def metric(f):
        def edit():
            adj.metric = f(adj.metric)
            return [u]
        return edit

    def drain(on):
        def edit():
            dbs[u].isOverloaded = on
            return [u]
        return edit

    def down():
        dbs[u].adjacencies.remove(adj)
        dbs[v].adjacencies.remove(back)
        return [u, v]

    def up():
        dbs[u].adjacencies.append(adj)
        dbs[v].adjacencies.append(back)
        return [u, v]

    events = [("metric_raised", metric(lambda m: m * 4 + 1)),
              ("metric_lowered", metric(lambda m: (m - 1) // 4)),
              ("node_drained", drain(True)), ("node_undrained", drain(False)),
              ("link_down", down), ("link_up", up)]
    out = {"nodes": t.num_nodes, "prefixes": t.num_prefixes, "bgp_prefixes": t.num_bgp_prefixes,
           "selected_columns": t.num_selected_columns, "node": u, "link": [u, v],
           "warmups": WARM, "timed_rounds": reps}
    acc = {name: [] for name, _ in events}
    for r in range(WARM + reps):
        for name, edit in events:
            older = table()  # the replaced path's state before
            for n in edit():
                ls.updateAdjacencyDatabase(copy.deepcopy(dbs[n]))
            t0 = time.perf_counter()
            ls.prefetchSpf([u], True)
            w_engine = ms_since(t0)
            t0 = time.perf_counter()
            counts = t.apply_topology_changes(areas, "0")
            m = {"engine_wall_ms": w_engine, "apply_wall_ms": ms_since(t0), "spf_ms": t.spf_ms,
                 "refresh_ms": t.refresh_ms, "listed_rows": t.refresh_rows,
                 "changed_routes": int(sum(counts))}
            t0 = time.perf_counter()
            fresh = table()
            m["b_table_wall_ms"] = ms_since(t0)
            t0 = time.perf_counter()
            c2 = fresh.diff(older)
            m["b_diff_wall_ms"] = ms_since(t0)
            m["b_wall_ms"] = m["b_table_wall_ms"] + m["b_diff_wall_ms"]
            m["b_spf_ms"], m["b_route_ms"] = fresh.spf_ms, fresh.route_ms
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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    torch.cuda.init()
    res = churn(TP.fabric(args.nodes), args.reps)
    res.update({"gpu": torch.cuda.get_device_name(0), "topology": f"fabric({args.nodes})",
                "bgp_prefixes_announced": N_BGP, "announcers_per_prefix": N_ANNOUNCERS})
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
