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

BGP columns, ABI level ("abi_bgp"): the table above plus 512 BGP prefixes of
4 RSW announcers each (the workload of profiles/bgp_igp_table.py: one
tie-breaker entity, so the IGP cost decides first), through
spf_route_table_patch_columns_sel, for both column kinds:

  selected       the 512 are selected columns (bgpUseIgpMetric: candidates and
                 pair codes, folded per node), 8 spare selected columns
  host_selected  the 512 are unselected columns holding the host selection's
                 winner; SPF_MAP_NONE in their dirty lists

  candidate_withdrawn  one column loses a candidate (host_selected: its winner)
  new_bgp_prefix       a spare column gets a BGP prefix
  metric_vectors_64    64 columns get other metric vectors (other pair codes,
                       every candidate dirty; another winner)

against, in the same run, a fresh spf_route_table_create_sel table of the
state after the event, run, and spf_route_table_diff_mapped with the same
dirty lists.

BGP columns, host level ("host_bgp"): the same workload published through
PrefixState (profiles/bgp_igp_table.py's prefix databases) into an
AllNodesRouteTable with bgp_columns, bgp_in_place and 64 spare columns of
either kind, with and without bgp_use_igp_metric; the three events above
through apply_prefix_changes, against a fresh table with the same flags plus
diff, in the same run.

  python profiles/prefix_churn.py [--nodes N] [--reps R] [--out FILE]
                                  [--sections abi,host,abi_bgp,host_bgp]
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


N_BGP, N_ANNOUNCERS, SPARE_SEL = 512, 4, 8
WINNER, LOOSER = 0, 4


def tie_codes(ties):
    """Pair table of candidates whose vectors differ in one tie-breaker: the
    nearer one wins, at equal distance the larger tie-breaker."""
    out = []
    for i in range(1, len(ties)):
        for b in range(i):
            eq = WINNER if ties[i] > ties[b] else LOOSER
            out.append(WINNER | (eq << 3) | (LOOSER << 6))
    return out


def measure_bgp(q, t, ann, sel, cols, lists, psel, dirty, reps):
    P = len(ann)
    old = [ann[c] for c in cols]
    old_sel = {c: sel[c] for c in cols if c in sel}
    patch_ms, patch_wall, pack_wall, cells = [], [], [], 0
    for r in range(reps + 1):  # the first pair warms up
        t0 = time.perf_counter()
        counts = t.patch_columns_sel(cols, lists, psel, dirty)
        w = ms_since(t0)
        d = t.patch_ms()
        t0 = time.perf_counter()
        pk = t.delta_pack()
        p = ms_since(t0)
        cells = int(counts.sum())
        assert pk["cells"] == cells
        t.patch_columns_sel(cols, old, old_sel)
        if r:
            patch_ms.append(d)
            patch_wall.append(w)
            pack_wall.append(p)
    ann2, sel2 = list(ann), dict(sel)
    for c, l in zip(cols, lists):
        ann2[c] = l
    sel2.update(psel)
    maps = {}
    if dirty is not None:
        off = np.zeros(P + 1, dtype=np.uint32)
        off[np.asarray(cols) + 1] = [len(x) for x in dirty]
        order = np.argsort(cols)
        flat = [int(x) for k in order for x in dirty[k]]
        maps = {"dirty_off": np.cumsum(off, dtype=np.uint32),
                "dirty_ann": np.asarray(flat if flat else [0], dtype=np.uint32)}
    build, route, select, diff, pack2 = [], [], [], [], []
    for r in range(3):
        t0 = time.perf_counter()
        n = abi.RouteTable(q, ann2, 0, sel2 or None).run()
        rk = kernel_ms(n)  # waits for the run
        build.append(ms_since(t0))
        route.append(rk)
        select.append(n.select_ms())
        t0 = time.perf_counter()
        counts = n.diff_mapped(t, **maps)
        diff.append(ms_since(t0))
        t0 = time.perf_counter()
        pk = n.delta_pack()
        pack2.append(ms_since(t0))
        assert int(counts.sum()) == cells == pk["cells"], (int(counts.sum()), cells)
        n.close()
    return {
        "columns": len(cols), "changed_cells": cells,
        "patch_ms": med(patch_ms), "patch_wall_ms": med(patch_wall), "pack_wall_ms": med(pack_wall),
        "rebuild": {"create_run_wall_ms": med(build[1:]), "route_kernel_ms": med(route[1:]),
                    "select_kernel_ms": med(select[1:]), "diff_mapped_wall_ms": med(diff[1:]),
                    "pack_wall_ms": med(pack2[1:])},
    }


def bgp_level(q, V, names, reps):
    rng = np.random.RandomState(2)
    rsw = [i for i, n in enumerate(names) if n.startswith("3-")]
    base = [[v // 2] for v in range(2 * V)]
    cands = [[int(a) for a in rng.choice(rsw, size=N_ANNOUNCERS, replace=False)] for _ in range(N_BGP)]
    ties = [rng.permutation(N_ANNOUNCERS).tolist() for _ in range(N_BGP)]
    b0 = 2 * V  # first BGP column
    out = {"bgp_prefixes": N_BGP, "announcers": N_ANNOUNCERS}
    for kind in ("selected", "host_selected"):
        if kind == "selected":
            ann = base + cands + [[] for _ in range(SPARE + SPARE_SEL)]
            sel = {b0 + k: (tie_codes(ties[k]), [1] * N_ANNOUNCERS) for k in range(N_BGP)}
            spare = b0 + N_BGP + SPARE  # first spare selected column
            sel.update({spare + j: ([], []) for j in range(SPARE_SEL)})
            new_ties = [rng.permutation(N_ANNOUNCERS).tolist() for _ in range(64)]
            events = {
                "candidate_withdrawn": ([b0], [cands[0][1:]], {b0: (tie_codes(ties[0][1:]), [1] * 3)}, None),
                "new_bgp_prefix": ([spare], [cands[1]], {spare: (tie_codes(ties[1]), [1] * 4)}, None),
                "metric_vectors_64": (
                    [b0 + k for k in range(64)], [cands[k] for k in range(64)],
                    {b0 + k: (tie_codes(new_ties[k]), [1] * 4) for k in range(64)},
                    [cands[k] for k in range(64)]),
            }
        else:
            def winner(k, skip=None, tv=None):
                tv = tv or ties[k]
                return max((tv[c], cands[k][c]) for c in range(N_ANNOUNCERS) if c != skip)[1]
            ann = base + [[winner(k)] for k in range(N_BGP)] + [[] for _ in range(SPARE + SPARE_SEL)]
            sel = {}
            spare = b0 + N_BGP
            flipped = [[(v + 1) % N_ANNOUNCERS for v in ties[k]] for k in range(64)]
            events = {
                "candidate_withdrawn": ([b0], [[winner(0, ties[0].index(max(ties[0])))]], {},
                                        [[abi.SPF_MAP_NONE]]),
                "new_bgp_prefix": ([spare], [[winner(1)]], {}, [[abi.SPF_MAP_NONE]]),
                "metric_vectors_64": (
                    [b0 + k for k in range(64)], [[winner(k, None, flipped[k])] for k in range(64)], {},
                    [[abi.SPF_MAP_NONE, winner(k, None, flipped[k])] for k in range(64)]),
            }
        t = abi.RouteTable(q, ann, 0, sel or None).run()
        out[kind] = {"columns": len(ann), "full_route_kernel_ms": round(kernel_ms(t), 3),
                     "full_select_kernel_ms": round(t.select_ms(), 3)}
        for name, (cols, lists, psel, dirty) in events.items():
            out[kind][name] = measure_bgp(q, t, ann, sel, cols, lists, psel, dirty, reps)
            print("abi_bgp", kind, name, out[kind][name], file=sys.stderr, flush=True)
        t.close()
    return out


def host_bgp_level(topo, reps):
    import copy

    import openr_amd._openr_spf as E
    from openr_amd import thrift as T

    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import bgp_igp_table as B

    E.set_spf_device(0)
    areas = E.AreaLinkStates()
    ls = areas.add("0")
    for db in topo.adj_dbs():
        ls.updateAdjacencyDatabase(db)
    out = {}
    for igp in (True, False):
        ps = E.PrefixState()
        pdbs = {db.thisNodeName: db for db in B.prefix_dbs(topo)}
        for db in pdbs.values():
            ps.updatePrefixDatabase(db)
        kw = dict(bgp_columns=True, bgp_use_igp_metric=igp)
        base = E.AllNodesRouteTable(areas, "0", ps, True, False, **kw)
        t = E.AllNodesRouteTable(areas, "0", ps, True, False, bgp_in_place=True,
                                 spare_columns=SPARE, spare_selected_columns=SPARE, **kw)
        holders = {}  # BGP prefix -> its announcers
        for n, db in sorted(pdbs.items()):
            for e in db.prefixEntries:
                if e.type == T.PrefixType.BGP:
                    holders.setdefault((bytes(e.prefix.prefixAddress.addr), e.prefix.prefixLength),
                                       []).append(n)
        keys = sorted(holders)
        new = T.toIpPrefix("2001:db8:ffff::/48")

        def is_key(e, k):
            return (bytes(e.prefix.prefixAddress.addr), e.prefix.prefixLength) == k

        def withdraw_candidate():
            n = holders[keys[0]][0]
            pdbs[n].prefixEntries = [e for e in pdbs[n].prefixEntries if not is_key(e, keys[0])]
            return [n]

        def new_prefix():
            nodes = holders[keys[1]]
            for v, n in enumerate(nodes):
                mv = T.MetricVector(0, [T.createMetricEntity(
                    1, 10, T.CompareType.WIN_IF_PRESENT, True, [v])])
                pdbs[n].prefixEntries = list(pdbs[n].prefixEntries) + [
                    T.createPrefixEntry(new, T.PrefixType.BGP, n, mv=mv)]
            return nodes

        def vectors_64():
            nodes = []
            for k in keys[2:66]:
                n = holders[k][0]
                entries = []
                for e in pdbs[n].prefixEntries:
                    if is_key(e, k):
                        e = copy.deepcopy(e)
                        e.mv.metrics[0].metric[0] += 10  # this announcer now wins the tie-break
                    entries.append(e)
                pdbs[n].prefixEntries = entries
                nodes.append(n)
            return sorted(set(nodes))

        def publish(nodes):
            changed = set()
            for n in nodes:
                changed |= set(ps.updatePrefixDatabase(pdbs[n]))
            return changed

        res = {"prefixes": t.num_prefixes, "bgp_prefixes": t.num_bgp_prefixes,
               "selected_columns": t.num_selected_columns}
        events = {"candidate_withdrawn": withdraw_candidate, "new_bgp_prefix": new_prefix,
                  "metric_vectors_64": vectors_64}
        for name, edit in events.items():
            patch_ms, apply_wall, build, diff = [], [], [], []
            routes = cols = 0
            for r in range(reps + 1):
                saved = {n: list(db.prefixEntries) for n, db in pdbs.items()}
                nodes = edit()
                changed = publish(nodes)
                t0 = time.perf_counter()
                counts = t.apply_prefix_changes(ps, changed)
                w = ms_since(t0)
                pm = t.patch_ms
                routes, cols = int(sum(counts)), len(changed)
                if r <= 3:  # (the rebuild side: three samples are enough for tens of ms)
                    t0 = time.perf_counter()
                    fresh = E.AllNodesRouteTable(areas, "0", ps, True, False, **kw)
                    fresh_ms = ms_since(t0)
                    t0 = time.perf_counter()
                    c2 = fresh.diff(base)
                    diff_ms = ms_since(t0)
                    assert sum(c2) == routes, (sum(c2), routes)
                    del fresh
                for n in nodes:  # the inverse event, untimed
                    pdbs[n].prefixEntries = saved[n]
                t.apply_prefix_changes(ps, publish(nodes))
                if r:
                    patch_ms.append(pm)
                    apply_wall.append(w)
                    if r <= 3:
                        build.append(fresh_ms)
                        diff.append(diff_ms)
            res[name] = {"changed_prefixes": cols, "changed_routes": routes,
                         "patch_ms": med(patch_ms), "apply_wall_ms": med(apply_wall),
                         "rebuild": {"table_wall_ms": med(build), "diff_wall_ms": med(diff)}}
            print("host_bgp", "selected" if igp else "host_selected", name, res[name],
                  file=sys.stderr, flush=True)
        out["selected" if igp else "host_selected"] = res
        del t, base
    return out


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
    ap.add_argument("--sections", default="abi,host,abi_bgp,host_bgp")
    args = ap.parse_args()
    sections = set(args.sections.split(","))

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
    if "abi" in sections:
        result["abi"] = {}
        for name, (cols, lists) in events.items():
            result["abi"][name] = measure(q, t, ann, cols, lists, args.reps)
            print("abi", name, result["abi"][name], file=sys.stderr, flush=True)
    t.close()
    if "abi_bgp" in sections:
        result["abi_bgp"] = bgp_level(q, V, names, args.reps)
    q.close()
    g.close()
    if "host" in sections:
        result["host"] = host_level(topo, args.reps)
    if "host_bgp" in sections:
        result["host_bgp"] = host_bgp_level(topo, args.reps)
    line = json.dumps(result)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
