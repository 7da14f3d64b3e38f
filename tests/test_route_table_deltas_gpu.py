"""AllNodesRouteTable::deltas(): the route delta of EVERY node (getRouteDelta,
openr/decision/Decision.cpp:47-85) from one packed fetch of the changed cells
(spf_route_table_delta_pack) plus one sparse read per table for the MPLS
candidates (spf_route_table_fetch_cells), instead of two whole rows per node.

Entry i equals delta(node i) and delta_mpls(node i) as sets, and -- where an
oracle is built -- getRouteDelta of the CPU oracle's buildRouteDb before and
after, independently of delta().
"""

import copy

import pytest

from openr_amd import thrift as T
from tests import randomized as RZ
from tests.test_route_table_delta_churn_gpu import _base, _churn, _delta_py, _ecmp_only, _unlink

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


def _check_against_delta(t1, nodes=None):
    """deltas()[i] == delta(node i) + delta_mpls(node i), lists as sets.
    Returns {node: (upd, sorted dele, mpls upd, sorted mpls dele)}."""
    out = {}
    all_ = t1.deltas()
    assert len(all_) == t1.num_nodes
    for i, (upd, dele, mupd, mdele) in enumerate(all_):
        node = t1.node_name(i)
        assert len(set(dele)) == len(dele) and len(set(mdele)) == len(mdele), node
        out[node] = (upd, sorted(dele), mupd, sorted(mdele))
        if nodes is not None and node not in nodes:
            continue
        u, d = t1.delta(node)
        mu, md = t1.delta_mpls(node)
        assert (upd, sorted(dele)) == (u, sorted(d)), node
        assert (mupd, sorted(mdele)) == (mu, sorted(md)), node
    return out


@pytest.mark.parametrize("lfa", [False, True])
@pytest.mark.parametrize("seed", range(4))
def test_deltas_across_churn(E, O, seed, lfa):
    names, adj0, pfx0 = _base(seed)
    adj1, pfx1, new, removed = _churn(seed, names, adj0, pfx0)
    areas, ps = RZ.load(E, adj0, pfx0, seed)
    t0 = E.AllNodesRouteTable(areas, "0", ps, True, lfa)
    areas1, ps1 = RZ.load(E, adj1, pfx1, seed + 50)
    t1 = E.AllNodesRouteTable(areas1, "0", ps1, True, lfa)
    changed = t1.diff(t0)
    assert t1.diff_was_mapped
    got = _check_against_delta(t1)
    assert new in got and removed not in got
    assert sum(len(u) + len(d) + len(mu) + len(md) for u, d, mu, md in got.values()) > 0
    for node, c in zip((t1.node_name(i) for i in range(len(changed))), changed):
        uni, _ = t1.changed_split(node)
        assert len(got[node][0]) + len(got[node][1]) == uni, node
    if seed == 0:
        # independently of delta(): the oracle's RouteDbs before and after
        osolver = O.SpfSolver(names[0], True, lfa)
        oareas, ops = RZ.load(O, adj0, pfx0, seed)
        oareas1, ops1 = RZ.load(O, adj1, pfx1, seed + 50)
        for node, (upd, dele, mupd, mdele) in got.items():
            b = osolver.buildRouteDb(node, oareas, ops) if node in names else None
            a = osolver.buildRouteDb(node, oareas1, ops1)
            bu = _ecmp_only(b["unicast"]) if b else {}
            au = _ecmp_only(a["unicast"]) if a else {}
            assert (upd, dele) == _delta_py(au, bu), node
            assert (mupd, mdele) == _delta_py(a["mpls"] if a else {}, b["mpls"] if b else {}), node


def _collision_network():
    """Seven nodes.  c and f share node label 200 (two columns under one
    label; c, the smaller name, wins wherever it is reachable); b's adjacency
    towards a carries adjacency label 104, which is d's node label.  Newer:
    links b-c and c-d go, so c (with its stub g) is unreachable from the rest
    and f becomes the winner of label 200 there -- through cells of column
    (200, f) that did not change.  b reaches d over b-d before and after, so
    label 104 at b is a candidate (adjacency label) whose column is unchanged."""
    labels = {"a": 101, "b": 102, "c": 200, "d": 104, "e": 105, "f": 200, "g": 107}
    dbs = {n: T.createAdjDb(n, [], lab, False, "0") for n, lab in labels.items()}

    def link(u, v, metric, k, lab_uv=None):
        ifu, ifv = f"if_{u}_{v}", f"if_{v}_{u}"
        dbs[u].adjacencies.append(T.createAdjacency(
            v, ifu, ifv, f"fe80::{k}:1", f"10.9.{k}.1", metric, lab_uv or 50000 + 2 * k))
        dbs[v].adjacencies.append(T.createAdjacency(
            u, ifv, ifu, f"fe80::{k}:2", f"10.9.{k}.2", metric, 50001 + 2 * k))

    link("b", "a", 2, 1, lab_uv=104)
    link("b", "c", 1, 2)
    link("c", "d", 1, 3)
    link("b", "d", 1, 4)
    link("d", "e", 2, 5)
    link("d", "f", 2, 6)
    link("c", "g", 1, 7)
    link("a", "e", 3, 8)
    names = sorted(labels)
    pfx = [T.createPrefixDb(n, [T.createPrefixEntry(T.toIpPrefix(f"fc00:{k + 1}::1/128"))], "0")
           for k, n in enumerate(names)]
    adj0 = {"0": [dbs[n] for n in names]}
    adj1 = copy.deepcopy(adj0)
    by = {db.thisNodeName: db for db in adj1["0"]}
    _unlink(by, "b", next(a for a in by["b"].adjacencies if a.otherNodeName == "c"))
    _unlink(by, "c", next(a for a in by["c"].adjacencies if a.otherNodeName == "d"))
    return names, adj0, adj1, pfx


@pytest.mark.parametrize("lfa", [False, True])
def test_deltas_label_collisions(E, O, lfa):
    names, adj0, adj1, pfx = _collision_network()
    areas, ps = RZ.load(E, adj0, pfx, 1)
    areas1, ps1 = RZ.load(E, adj1, pfx, 2)
    t0 = E.AllNodesRouteTable(areas, "0", ps, True, lfa)
    t1 = E.AllNodesRouteTable(areas1, "0", ps1, True, lfa)
    assert t1.num_label_columns == 7
    t1.diff(t0)
    got = _check_against_delta(t1)
    osolver = O.SpfSolver("a", True, lfa)
    oareas, ops = RZ.load(O, adj0, pfx, 1)
    oareas1, ops1 = RZ.load(O, adj1, pfx, 2)
    for node, (upd, dele, mupd, mdele) in got.items():
        b = osolver.buildRouteDb(node, oareas, ops)
        a = osolver.buildRouteDb(node, oareas1, ops1)
        assert (upd, dele) == _delta_py(a["unicast"], b["unicast"]), node
        assert (mupd, mdele) == _delta_py(a["mpls"], b["mpls"]), node
    # the winner of label 200 moved from c to f where c is cut off (at f
    # itself c's SWAP route gave way to POP_AND_LOOKUP) ...
    for node in ("a", "b", "d", "e", "f"):
        assert 200 in got[node][2], node
    # ... and stayed at g, which still reaches c
    assert 200 not in got["g"][2] and 200 not in got["g"][3]
    if not lfa:
        # label 104 at b (a candidate through b's adjacency label) is unchanged;
        # with LFA the lost link b-c was an alternate towards d
        assert 104 not in got["b"][2] and 104 not in got["b"][3]


@pytest.mark.parametrize("lfa", [False, True])
def test_deltas_equal_layout_drain(E, lfa):
    names, adj0, pfx0 = _base(1)
    adj1 = copy.deepcopy(adj0)
    drained = next(db for db in adj1["0"] if not db.isOverloaded and len(db.adjacencies) > 2)
    drained.isOverloaded = True
    areas, ps = RZ.load(E, adj0, pfx0, 1)
    areas1, ps1 = RZ.load(E, adj1, pfx0, 1)
    t0 = E.AllNodesRouteTable(areas, "0", ps, True, lfa)
    t1 = E.AllNodesRouteTable(areas1, "0", ps1, True, lfa)
    changed = t1.diff(t0)
    assert not t1.diff_was_mapped and sum(changed) > 0
    got = _check_against_delta(t1)
    assert sum(len(u) + len(d) for u, d, _, _ in got.values()) == sum(
        t1.changed_split(n)[0] for n in got)
    timed = t1.deltas_timed()
    assert timed["cells"] == sum(changed) and timed["gone"] == 0 and timed["bytes"] > 0


def test_deltas_fabric_link_down(E):
    """TP.fabric(600) with one RSW-FSW link down: deltas() against delta(node)
    on sampled nodes plus the two ends of the link."""
    from openr_amd import topologies as TP

    topo = TP.fabric(600)

    def load(dbs):
        areas = E.AreaLinkStates()
        ls = areas.add("0")
        for db in dbs:
            ls.updateAdjacencyDatabase(db)
        ps = E.PrefixState()
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
    ea, eps = load(dbs0)
    ea1, eps1 = load(dbs1)
    t0 = E.AllNodesRouteTable(ea, "0", eps, True)
    t1 = E.AllNodesRouteTable(ea1, "0", eps1, True)
    changed = t1.diff(t0)
    assert t1.diff_was_mapped
    sample = set(sorted(topo.names)[:: max(1, topo.num_nodes // 25)] + [rsw, fsw])
    got = _check_against_delta(t1, sample)
    assert len(got[rsw][0]) + len(got[rsw][1]) > 0 and len(got[fsw][0]) + len(got[fsw][1]) > 0
    # every node: as many unicast updates + deletes as changed unicast columns
    for i, c in enumerate(changed):
        node = t1.node_name(i)
        assert len(got[node][0]) + len(got[node][1]) <= c, node
        if node in sample:
            assert len(got[node][0]) + len(got[node][1]) == t1.changed_split(node)[0], node


def test_deltas_before_a_diff_raises(E):
    names, adj0, pfx0 = _base(2)
    areas, ps = RZ.load(E, adj0, pfx0, 2)
    t0 = E.AllNodesRouteTable(areas, "0", ps, True)
    with pytest.raises(RuntimeError, match="no diff"):
        t0.deltas()
    with pytest.raises(RuntimeError, match="no diff"):
        t0.deltas_timed()
