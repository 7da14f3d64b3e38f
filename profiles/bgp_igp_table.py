"""Measurement: BGP prefixes under bgpUseIgpMetric in the all-nodes route
table, selected on the device (bgp_igp_on_device) against the host path.

On the 10k fabric, 512 BGP prefixes are added, each announced by four random
RSWs whose metric vectors hold one tie-breaker entity (so the IGP cost decides
first and equidistant announcers are ordered by the tie-breaker).
AllAreasRouteTable is built with bgp_use_igp_metric=True and the flag on and
off; reported per run: the selection kernel's and the route kernel's device
time, the table build's wall time, and the wall time of routeDb(node) over
every node (C++ loop, no Python conversion) with the routes that came from
the device table and from the host share.

  python profiles/bgp_igp_table.py [--nodes N] [--out FILE]
"""
import argparse
import json
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from openr_amd import thrift as T  # noqa: E402
from openr_amd import topologies as TP  # noqa: E402

N_BGP, N_ANNOUNCERS = 512, 4


def prefix_dbs(topo, seed=1):
    """The fabric's loopbacks plus the BGP prefixes, one db per node."""
    rng = random.Random(seed)
    rsws = [n for n in topo.names if n.startswith("3-")]
    extra = {}
    for k in range(N_BGP):
        prefix = T.toIpPrefix(f"2001:db8:{k:x}::/48")
        tie = list(range(N_ANNOUNCERS))
        rng.shuffle(tie)
        for n, v in zip(rng.sample(rsws, N_ANNOUNCERS), tie):
            mv = T.MetricVector(0, [T.createMetricEntity(
                1, 10, T.CompareType.WIN_IF_PRESENT, True, [v])])
            extra.setdefault(n, []).append(
                T.createPrefixEntry(prefix, T.PrefixType.BGP, n, mv=mv))
    out = []
    for db in topo.prefix_dbs("0"):
        db.prefixEntries = list(db.prefixEntries) + extra.get(db.thisNodeName, [])
        out.append(db)
    return out


def run(E, areas, ps, nodes, on_device):
    t0 = time.perf_counter()
    t = E.AllAreasRouteTable(areas, ps, True, False, False, True, bgp_igp_on_device=on_device)
    build_ms = (time.perf_counter() - t0) * 1e3
    table = host = 0
    us = 0.0
    for i in range(0, len(nodes), 500):  # chunks: a sign of life on stderr
        a, b, c = t.route_db_loop_timed(nodes[i:i + 500])
        table, host, us = table + a, host + b, us + c
        print(f"  on_device={on_device}: {min(i + 500, len(nodes))}/{len(nodes)} nodes",
              file=sys.stderr, flush=True)
    return {
        "bgp_device_prefixes": t.bgp_device_prefixes,
        "select_kernel_ms": round(t.select_ms, 3),
        "route_kernel_ms": round(t.route_ms, 3),
        "build_wall_ms": round(build_ms, 1),
        "route_db_nodes": len(nodes),
        "route_db_wall_ms": round(us / 1e3, 1),
        "route_db_ms_per_node": round(us / 1e3 / max(len(nodes), 1), 3),
        "table_routes": table,
        "host_routes": host,
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=0, help="routeDb over the first N nodes (0: all)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    torch.cuda.init()
    import openr_amd._openr_spf as E

    E.set_spf_device(0)
    topo = TP.fabric(10000)
    areas = E.AreaLinkStates()
    ls = areas.add("0")
    for db in topo.adj_dbs():
        ls.updateAdjacencyDatabase(db)
    ps = E.PrefixState()
    for pdb in prefix_dbs(topo):
        ps.updatePrefixDatabase(pdb)
    nodes = sorted(topo.names)
    if args.nodes:
        nodes = nodes[:: max(1, len(nodes) // args.nodes)][: args.nodes]
    E.AllAreasRouteTable(areas, ps, True, False, False, True, bgp_igp_on_device=True)  # warm
    result = {
        "topology": "fabric(10000)", "nodes": len(topo.names), "bgp_prefixes": N_BGP,
        "announcers_per_prefix": N_ANNOUNCERS, "gpu": torch.cuda.get_device_name(0),
        "on_device": run(E, areas, ps, nodes, True),
        "on_host": run(E, areas, ps, nodes, False),
    }
    line = json.dumps(result)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
