"""AllNodesRouteTable::diff / delta across link, node, prefix and label
changes: the tables differ in nodes, columns and link
layout, so the diff goes through maps (spf_route_table_diff_mapped) -- rows
and best announcers by node name, unicast columns by prefix, node-label
columns by (label, owner), link bits by Link identity, changed PrefixEntries
as dirty announcers.

For every node of the newer table the delta equals getRouteDelta
(openr/decision/Decision.cpp:47-85) of that node's routes in the two tables,
and of the CPU oracle's buildRouteDb before and after (unicast and MPLS); a
node the older table lacks has every route as an update.
"""

import copy
import random

import pytest

from openr_amd import thrift as T
from tests import randomized as RZ

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def E(gpu_ready):
    import openr_amd._openr_spf as E

    return E


@pytest.fixture(scope="module")
def O():
    from oracle import build

    build.build()
    from oracle import _oracle_ref

    return _oracle_ref


def _ecmp_only(unicast):
    # SR_MPLS prefixes (fd00::/64 in the generator) are not in the table
    return {k: v for k, v in unicast.items()
            if not bytes(k[0][0] if isinstance(k[0], tuple) else k[0]).startswith(b"\xfd\x00")}


def _delta_py(new, old):
    """getRouteDelta (Decision.cpp:47-85) over route dicts: updates = new or
    changed entries, deletes = keys only in old."""
    upd = {k: v for k, v in new.items() if old.get(k) != v}
    dele = sorted(k for k in old if k not in new)
    return upd, dele


ANYCAST = "fc99::1/128"


def _link(dbs, u, v, tag, metric=4, k=0):
    """One more link u - v (a new interface pair on both sides)."""
    ifu, ifv = f"if_{u}_{v}_{tag}", f"if_{v}_{u}_{tag}"
    dbs[u].adjacencies.append(
        T.createAdjacency(v, ifu, ifv, f"fe80::fa:{k}:1", f"10.250.{k}.1", metric, 59000 + 2 * k))
    dbs[v].adjacencies.append(
        T.createAdjacency(u, ifv, ifu, f"fe80::fa:{k}:2", f"10.250.{k}.2", metric + 1, 59001 + 2 * k))


def _unlink(dbs, u, adj):
    """Remove the link of u's adjacency `adj` from both adjacency databases."""
    v = adj.otherNodeName
    dbs[u].adjacencies.remove(adj)
    back = [a for a in dbs[v].adjacencies if a.otherNodeName == u and a.ifName == adj.otherIfName]
    assert len(back) == 1
    dbs[v].adjacencies.remove(back[0])


def _base(seed):
    """The network of the older table: RZ.random_network plus what the events
    below need to exist (a parallel pair, an anycast announcer)."""
    names, adj_dbs, prefix_dbs = RZ.random_network(
        2300 + seed, n_nodes=40, n_links=90, overload_prob=0.1, link_overload_prob=0.03)
    dbs = {db.thisNodeName: db for db in adj_dbs["0"]}
    first = adj_dbs["0"][0]
    _link(dbs, first.thisNodeName, first.adjacencies[0].otherNodeName, "twin", metric=3, k=9)
    pdb0 = prefix_dbs[0]
    if not any(e.prefix == T.toIpPrefix(ANYCAST) for e in pdb0.prefixEntries):
        pdb0.prefixEntries.append(T.createPrefixEntry(T.toIpPrefix(ANYCAST)))
    return names, adj_dbs, prefix_dbs


def _churn(seed, names, adj_dbs, prefix_dbs):
    """One event of each kind between the two loads (on copies)."""
    adj_dbs = copy.deepcopy(adj_dbs)
    prefix_dbs = copy.deepcopy(prefix_dbs)
    rng = random.Random(seed)
    dbs = {db.thisNodeName: db for db in adj_dbs["0"]}
    pdbs = {p.thisNodeName: p for p in prefix_dbs}
    first = adj_dbs["0"][0].thisNodeName
    # the roles are distinct nodes, none of them the node with the twin link
    removed, withdrawn, entry, label, anycast2, a1, a2, j1, j2, cut = rng.sample(
        [n for n in names if n in dbs and n != first and n != prefix_dbs[0].thisNodeName], 10)
    # a link removed from both adjacency databases
    _unlink(dbs, cut, next(a for a in dbs[cut].adjacencies if a.otherNodeName != first))
    # a parallel link removed while its twin stays (the older of the two: the
    # twin's bit moves)
    twin = [a for a in dbs[first].adjacencies if a.ifName.endswith("_twin")][0]
    orig = [a for a in dbs[first].adjacencies
            if a.otherNodeName == twin.otherNodeName and a is not twin][0]
    _unlink(dbs, first, orig)
    # a link added
    _link(dbs, a1, a2, "new", k=1)
    # a node added with two links and a prefix (its name sorts mid-range)
    new = "n500000-new"
    dbs[new] = T.createAdjDb(new, [], 9001, False, "0")
    adj_dbs["0"].append(dbs[new])
    _link(dbs, new, j1, "join", k=2)
    _link(dbs, new, j2, "join", k=3)
    prefix_dbs.append(T.createPrefixDb(new, [T.createPrefixEntry(T.toIpPrefix("fc00:ffff::1/128"))], "0"))
    # a node removed: its databases and every adjacency towards it
    adj_dbs["0"].remove(dbs.pop(removed))
    for db in dbs.values():
        db.adjacencies = [a for a in db.adjacencies if a.otherNodeName != removed]
    prefix_dbs.remove(pdbs.pop(removed))
    # a prefix withdrawn
    del pdbs[withdrawn].prefixEntries[0]
    # a second announcer of the anycast prefix
    if not any(e.prefix == T.toIpPrefix(ANYCAST) for e in pdbs[anycast2].prefixEntries):
        pdbs[anycast2].prefixEntries.append(T.createPrefixEntry(T.toIpPrefix(ANYCAST)))
    # a prefix entry changed in a field RibUnicastEntry equality sees
    # (bestPrefixEntry), the announcer unchanged
    pdbs[entry].prefixEntries[0].data = b"churn"
    # a node label changed
    dbs[label].nodeLabel = 9100
    return adj_dbs, prefix_dbs, new, removed


@pytest.mark.parametrize("lfa", [False, True])
@pytest.mark.parametrize("seed", range(4))
def test_route_table_delta_across_churn(E, O, seed, lfa):
    names, adj0, pfx0 = _base(seed)
    adj1, pfx1, new, removed = _churn(seed, names, adj0, pfx0)
    osolver = O.SpfSolver(names[0], True, lfa)
    areas, ps = RZ.load(E, adj0, pfx0, seed)
    oareas, ops = RZ.load(O, adj0, pfx0, seed)
    before = {n: osolver.buildRouteDb(n, oareas, ops) for n in names}
    t0 = E.AllNodesRouteTable(areas, "0", ps, True, lfa)
    areas1, ps1 = RZ.load(E, adj1, pfx1, seed + 50)
    oareas1, ops1 = RZ.load(O, adj1, pfx1, seed + 50)
    t1 = E.AllNodesRouteTable(areas1, "0", ps1, True, lfa)
    changed = t1.diff(t0)
    assert t1.diff_was_mapped
    nodes = [t1.node_name(i) for i in range(len(changed))]
    assert new in nodes and removed not in nodes
    total = 0
    for node, c in zip(nodes, changed):
        upd, dele = t1.delta(node)
        uni, lab = t1.changed_split(node)
        assert uni + lab == c, node
        assert len(upd) + len(dele) == uni, node
        # the device delta == getRouteDelta of the two tables' routes ...
        assert (upd, sorted(dele)) == _delta_py(t1.routes(node), t0.routes(node)), node
        # ... == getRouteDelta of the oracle's RouteDbs before and after
        after = osolver.buildRouteDb(node, oareas1, ops1)
        b, a = before.get(node), after
        bu = _ecmp_only(b["unicast"]) if b else {}
        au = _ecmp_only(a["unicast"]) if a else {}
        assert (upd, sorted(dele)) == _delta_py(au, bu), node
        mu, md = t1.delta_mpls(node)
        assert (mu, sorted(md)) == _delta_py(a["mpls"] if a else {}, b["mpls"] if b else {}), node
        if node == new:
            assert dele == [] and upd == t1.routes(node) and len(upd) > 0
        total += c
    assert total > 0


def test_route_table_delta_fabric_link_down(E, O):
    """TP.fabric(600) with one RSW-FSW link down, sampled nodes plus the two
    ends of the link (the only rows whose link bits move)."""
    from openr_amd import topologies as TP

    topo = TP.fabric(600)

    def load(M, dbs):
        areas = M.AreaLinkStates()
        ls = areas.add("0")
        for db in dbs:
            ls.updateAdjacencyDatabase(db)
        ps = M.PrefixState()
        for pdb in topo.prefix_dbs("0"):
            ps.updatePrefixDatabase(pdb)
        return areas, ps

    dbs0 = topo.adj_dbs(overloaded=[5])
    dbs1 = topo.adj_dbs(overloaded=[5])
    by = {db.thisNodeName: db for db in dbs1}
    rsw = next(n for n in topo.names if n.startswith("3-"))
    adj = next(a for a in by[rsw].adjacencies if a.otherNodeName.startswith("2-"))
    fsw = adj.otherNodeName
    _unlink(by, rsw, adj)
    ea, eps = load(E, dbs0)
    oa, ops = load(O, dbs0)
    ea1, eps1 = load(E, dbs1)
    oa1, ops1 = load(O, dbs1)
    t0 = E.AllNodesRouteTable(ea, "0", eps, True)
    t1 = E.AllNodesRouteTable(ea1, "0", eps1, True)
    changed = t1.diff(t0)
    assert t1.diff_was_mapped
    count = {t1.node_name(i): c for i, c in enumerate(changed)}
    solver = O.SpfSolver("2-0-0", True, False)
    total = 0
    for node in sorted(topo.names)[:: max(1, topo.num_nodes // 25)] + [rsw, fsw]:
        b = solver.buildRouteDb(node, oa, ops)
        a = solver.buildRouteDb(node, oa1, ops1)
        upd, dele = t1.delta(node)
        assert (upd, sorted(dele)) == _delta_py(a["unicast"], b["unicast"]), node
        mu, md = t1.delta_mpls(node)
        assert (mu, sorted(md)) == _delta_py(a["mpls"], b["mpls"]), node
        assert sum(t1.changed_split(node)) == count[node], node
        total += count[node]
    assert count[rsw] > 0 and count[fsw] > 0 and total > 0
