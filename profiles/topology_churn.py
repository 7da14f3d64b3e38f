"""Measurement: topology churn that keeps the CSR layout (link metrics, node
drains) applied to a resident all-nodes route table in place
(AllNodesRouteTable.apply_topology_changes -> graph patch, all-sources SPF
re-run, one spf_route_table_refresh_rows) against the path it replaces: a
fresh AllNodesRouteTable of the state after the event plus diff against a
table of the state before.

Workloads: the 10k fabric and the WAN-10k topology (openr_amd/topologies.py),
one prefix per node, LFA off.  Events, each from the state the previous one
left:

  metric_raised   one link's metric (one direction) raised
  metric_lowered  the same metric lowered back
  node_drained    one node drained
  node_undrained  the same node undrained
  metrics_64      64 half-edges get another metric at once (undone untimed)

Per event, medians over --reps repetitions after one warm-up:

  ABI level ("abi"), on one resident graph, query and table:
    listed_rows, changed_cells
    screen_wall_ms    spf_graph_diff + spf_table_screen on the resident rows
    patch_wall_ms     spf_graph_patch_metrics / spf_graph_set_transit
    spf_ms            device time of the new all-sources query
    query_wall_ms     its creation and run
    refresh_ms        device time of the refresh (bitmap clear + spf_route_refresh_kernel)
    refresh_wall_ms   spf_route_table_refresh_rows
    rebuild           the same delta the other way, in the same run: a new
                      graph, query and table of the state after, diff against
                      a table of the state before (wall times)
  Host level ("host"):
    listed_rows, changed_routes, spf_ms, refresh_ms
    engine_wall_ms    LinkState's own engine graph following the update (forced
                      before either path, common to both)
    apply_wall_ms     apply_topology_changes
    rebuild           fresh AllNodesRouteTable wall + diff wall

Both paths must report the same changed counts (asserted).

  python profiles/topology_churn.py [--nodes N] [--reps R] [--out FILE]
                                    [--sections abi,host] [--topologies fabric,wan]
"""
import argparse
import copy
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


def ms_since(t0):
    return (time.perf_counter() - t0) * 1e3


def med(xs):
    return round(statistics.median(xs), 4) if xs else None


def csr_with(csr, metric, ov):
    return abi.Csr(csr.num_nodes, csr.row_ptr, csr.col, metric, csr.link_id, csr.rev, ov,
                   csr.num_links)


class AbiState:
    """One resident graph / query / table that follows the events in place,
    and the replaced path beside it."""

    def __init__(self, csr):
        self.csr = csr
        self.V = csr.num_nodes
        self.src = np.arange(self.V, dtype=np.uint32)
        self.ann = [[v] for v in range(self.V)]
        self.g = abi.Graph(csr)
        self.q = self.g.query(self.src, abi.SPF_F_NEXTHOPS).run()
        self.t = abi.RouteTable(self.q, self.ann).run()

    def fresh(self, csr):
        """(graph, query, table, walls) of `csr`, built from nothing."""
        t0 = time.perf_counter()
        g = abi.Graph(csr)
        w_graph = ms_since(t0)
        t0 = time.perf_counter()
        q = g.query(self.src, abi.SPF_F_NEXTHOPS).run()
        w_query = ms_since(t0)
        t0 = time.perf_counter()
        t = abi.RouteTable(q, self.ann).run()
        t.fetch(0)  # waits for the run
        w_table = ms_since(t0)
        return g, q, t, {"graph_wall_ms": w_graph, "query_wall_ms": w_query, "spf_ms": q.elapsed_ms(),
                         "table_wall_ms": w_table}

    def apply(self, new):
        """The resident table follows self.csr -> new in place."""
        old = self.csr
        out = {}
        t0 = time.perf_counter()
        rows = None
        if np.array_equal(old.overloaded, new.overloaded):
            deltas = abi.graph_diff(old, new)
            dp, _, _, _ = self.q.device_rows()
            pitch = abi.load().spf_query_row_stride(self.q.h)
            hit = self.g.table_screen(dp, pitch, self.src, deltas)
            rows = np.flatnonzero(hit).astype(np.uint32)
        out["screen_wall_ms"] = ms_since(t0)
        t0 = time.perf_counter()
        e = np.flatnonzero(old.metric != new.metric)
        if len(e):
            self.g.patch_metrics(e, new.metric[e])
        if rows is None:
            self.g.set_transit(new.overloaded)
        out["patch_wall_ms"] = ms_since(t0)
        t0 = time.perf_counter()
        q = self.g.query(self.src, abi.SPF_F_NEXTHOPS).run()
        out["query_wall_ms"] = ms_since(t0)
        out["spf_ms"] = q.elapsed_ms()
        t0 = time.perf_counter()
        counts = self.t.refresh_rows(q, rows)
        out["refresh_wall_ms"] = ms_since(t0)
        out["refresh_ms"] = self.t.refresh_ms()
        self.q.close()
        self.q, self.csr = q, new
        out["listed_rows"] = self.V if rows is None else int(len(rows))
        return counts, out

    def close(self):
        self.t.close()
        self.q.close()
        self.g.close()


def pick_events(csr, node, rng):
    """{name: (metric array, overload array)} in the order they are applied;
    `node`: the tail of the changed link and the drained node."""
    m0, ov0 = csr.metric, csr.overloaded
    e = int(csr.row_ptr[node])
    raised = m0.copy()
    raised[e] = m0[e] * 4 + 1
    drained = ov0.copy()
    drained[node] = 1
    many = m0.copy()
    es = rng.choice(len(m0), size=64, replace=False)
    many[es] = m0[es] + 3
    return [("metric_raised", raised, ov0), ("metric_lowered", m0, ov0),
            ("node_drained", m0, drained), ("node_undrained", m0, ov0),
            ("metrics_64", many, ov0), (None, m0, ov0)]  # (None: the way back, untimed)


def abi_level(csr, node, reps):
    st = AbiState(csr)
    out = {"nodes": st.V, "columns": st.V}
    acc = {}
    for r in range(reps + 1):  # the first round warms up
        rng = np.random.RandomState(1)
        for name, metric, ov in pick_events(csr, node, rng):
            new = csr_with(csr, metric, ov)
            older = older_q = older_g = None
            rebuild = name is not None and r <= 3
            if rebuild:  # a table of the state before, for the replaced path's diff
                older_g, older_q, older, _ = st.fresh(st.csr)
            counts, m = st.apply(new)
            if rebuild:
                g2, q2, t2, walls = st.fresh(new)
                t0 = time.perf_counter()
                c2 = t2.diff(older)
                walls["diff_wall_ms"] = ms_since(t0)
                assert c2.tolist() == counts.tolist(), name
                for o in (t2, older, q2, older_q, g2, older_g):
                    o.close()
                m["rebuild"] = walls
            if name is None or not r:
                continue
            m["changed_cells"] = int(counts.sum())
            acc.setdefault(name, []).append(m)
    for name, ms in acc.items():
        out[name] = {k: med([m[k] for m in ms]) for k in ms[0] if k != "rebuild"}
        rb = [m["rebuild"] for m in ms if "rebuild" in m]
        out[name]["rebuild"] = {k: med([x[k] for x in rb]) for k in rb[0]}
        print("abi", name, out[name], file=sys.stderr, flush=True)
    st.close()
    return out


def host_level(topo, node_name, reps):
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
    t = E.AllNodesRouteTable(areas, "0", ps, True, False)
    names = sorted(dbs)
    rng = np.random.RandomState(1)
    many = [names[int(i)] for i in rng.choice(len(names), size=64, replace=False)]

    def set_metric(nodes, f):
        for n in nodes:
            a = dbs[n].adjacencies[0]
            a.metric = f(a.metric)
        return nodes

    def set_drain(n, on):
        dbs[n].isOverloaded = on
        return [n]

    events = [
        ("metric_raised", lambda: set_metric([node_name], lambda m: m * 4 + 1)),
        ("metric_lowered", lambda: set_metric([node_name], lambda m: (m - 1) // 4)),
        ("node_drained", lambda: set_drain(node_name, True)),
        ("node_undrained", lambda: set_drain(node_name, False)),
        ("metrics_64", lambda: set_metric(many, lambda m: m + 3)),
        (None, lambda: set_metric(many, lambda m: m - 3)),  # the way back, untimed
    ]
    out = {"nodes": t.num_nodes, "prefixes": t.num_prefixes}
    acc = {}
    for r in range(reps + 1):  # the first round warms up
        for name, edit in events:
            rebuild = name is not None and r <= 3
            older = E.AllNodesRouteTable(areas, "0", ps, True, False) if rebuild else None
            for n in edit():
                ls.updateAdjacencyDatabase(copy.deepcopy(dbs[n]))
            # LinkState refreshes its own engine graph on first use after an
            # update: whichever path ran first would pay for it, so it is
            # forced (one cached SPF) and timed apart from both
            t0 = time.perf_counter()
            ls.prefetchSpf([node_name], True)
            w_engine = ms_since(t0)
            t0 = time.perf_counter()
            counts = t.apply_topology_changes(areas, "0")
            m = {"engine_wall_ms": w_engine,
                 "apply_wall_ms": ms_since(t0), "spf_ms": t.spf_ms, "refresh_ms": t.refresh_ms,
                 "listed_rows": t.refresh_rows, "changed_routes": int(sum(counts))}
            if rebuild:
                t0 = time.perf_counter()
                fresh = E.AllNodesRouteTable(areas, "0", ps, True, False)
                w_table = ms_since(t0)
                t0 = time.perf_counter()
                c2 = fresh.diff(older)
                m["rebuild"] = {"table_wall_ms": w_table, "diff_wall_ms": ms_since(t0),
                                "spf_ms": fresh.spf_ms, "route_ms": fresh.route_ms}
                assert list(c2) == list(counts), name
                del fresh, older
            if name is None or not r:
                continue
            acc.setdefault(name, []).append(m)
    for name, ms in acc.items():
        out[name] = {k: med([m[k] for m in ms]) for k in ms[0] if k != "rebuild"}
        rb = [m["rebuild"] for m in ms if "rebuild" in m]
        out[name]["rebuild"] = {k: med([x[k] for x in rb]) for k in rb[0]}
        print("host", name, out[name], file=sys.stderr, flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--sections", default="abi,host")
    ap.add_argument("--topologies", default="fabric,wan")
    args = ap.parse_args()
    sections = set(args.sections.split(","))

    import torch

    torch.cuda.init()
    result = {"gpu": torch.cuda.get_device_name(0), "reps": args.reps}
    for kind in args.topologies.split(","):
        topo = TP.fabric(args.nodes) if kind == "fabric" else TP.wan(args.nodes, 10 * args.nodes)
        _, names = topo.rank()
        # the node whose first link moves and which is drained: a rack switch of
        # the fabric, any node with a few links of the WAN
        if kind == "fabric":
            node = next(i for i, n in enumerate(names) if n.startswith("3-")) + 7
        else:
            node = len(names) // 3
        res = {"topology": f"{kind}({args.nodes})", "node": names[node]}
        if "abi" in sections:
            res["abi"] = abi_level(topo.csr(), node, args.reps)
        if "host" in sections:
            res["host"] = host_level(topo, names[node], args.reps)
        result[kind] = res
    line = json.dumps(result)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
