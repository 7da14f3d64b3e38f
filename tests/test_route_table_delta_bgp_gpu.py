"""AllNodesRouteTable::diff / delta / deltas over BGP columns (bgp_columns):
host-selected columns (one metric-vector selection for all nodes) and
selected columns (bgp_use_igp_metric: the fold per node on the device).

A BGP route can change while its (metric, best, links) cell stays the same:
bestNexthop.metric of a selected column is the cell's igp word (the minimum
distance over every reachable candidate, not the winners' alone), and the
best entry and loopback of a host-selected column are the column's, not the
cell's.  For every node the delta must equal getRouteDelta
(openr/decision/Decision.cpp:47-85) of the node's routes in the two tables,
and of the CPU oracle's buildRouteDb before and after over the prefixes both
tables serve; the hand-built cases also state what the change means for named
nodes.
"""

import copy
import random

import pytest

from openr_amd import thrift as T
from tests import randomized as RZ
from tests.test_route_table_bgp_igp_gpu import (HI1, HI2, PFX, TB3, TB5, WIP, _ent, _line, _mv,
                                                _net)
from tests.test_route_table_delta_churn_gpu import _delta_py, _unlink

pytestmark = pytest.mark.gpu

_P = T.toIpPrefix(PFX)
KEY = (bytes(_P.prefixAddress.addr), _P.prefixLength)
LINE = [f"n{i:02d}" for i in range(7)]


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


def _table(E, adj_dbs, prefix_dbs, igp, lfa=False, dry=False, columns=True, seed=0):
    areas, ps = RZ.load(E, adj_dbs, prefix_dbs, seed)
    return E.AllNodesRouteTable(areas, "0", ps, True, lfa, bgp_columns=columns, bgp_dry_run=dry,
                                bgp_use_igp_metric=igp)


def _oracle_dbs(O, names, adj_dbs, prefix_dbs, igp, lfa=False, dry=False, seed=0):
    oa, op = RZ.load(O, adj_dbs, prefix_dbs, seed)
    return {n: O.SpfSolver(n, True, lfa, False, dry, igp).buildRouteDb(n, oa, op) for n in names}


def _diff_all(t1, t0, before=None, after=None):
    """diff, then for every node: delta == deltas()[i] == getRouteDelta of the
    two tables' routes, the counts of diff() and changed_split, and (given the
    oracle's RouteDbs) getRouteDelta of the oracle over the prefixes both
    tables serve.  Returns {node: (updates, sorted deletes)}."""
    changed = t1.diff(t0)
    both = set(t1.prefixes) & set(t0.prefixes)
    packed = t1.deltas()
    out = {}
    for i, c in enumerate(changed):
        node = t1.node_name(i)
        upd, dele = t1.delta(node)
        mu, md = t1.delta_mpls(node)
        pu, pd, pmu, pmd = packed[i]
        assert (pu, sorted(pd), pmu, sorted(pmd)) == (upd, sorted(dele), mu, sorted(md)), node
        uni, lab = t1.changed_split(node)
        assert uni + lab == c, node
        assert len(upd) + len(dele) == uni, node
        assert (upd, sorted(dele)) == _delta_py(t1.routes(node), t0.routes(node)), node
        if after is not None:
            a = {k: v for k, v in (after.get(node) or {"unicast": {}})["unicast"].items()
                 if k in both}
            b = {k: v for k, v in (before.get(node) or {"unicast": {}})["unicast"].items()
                 if k in both}
            got = ({k: v for k, v in upd.items() if k in both},
                   sorted(k for k in dele if k in both))
            assert got == _delta_py(a, b), node
        out[node] = (upd, sorted(dele))
    return out


def _metric_of(route):
    return route["bestNexthop"][4]


def _via(route):
    return sorted(nh[1].split("_")[2] for nh in route["nexthops"])


# ------------------------------------------------- 1, 2, 8: igp-only changes

HI = {"n00": _mv(HI2), "n06": _mv(HI1)}  # n00 wins everywhere


def _line_far_end(metric, stub=False):
    links = _line(7)
    links[-1] = ("n05", "n06", metric)
    if stub:
        links.append(("n00", "n07", 1))
    return links


def _expect_igp_only(deltas, t1, t0):
    # n00 stays best with the same next hops: only bestNexthop.metric (the
    # distance to the nearer n06) moves, at the two nodes nearer to n06
    for node, old, new in (("n04", 2, 3), ("n05", 1, 2)):
        upd, dele = deltas[node]
        assert KEY in upd and KEY not in dele, node
        r1, r0 = t1.routes(node)[KEY], t0.routes(node)[KEY]
        assert upd[KEY] == r1
        assert (_metric_of(r0), _metric_of(r1)) == (old, new), node
        assert r0["nexthops"] == r1["nexthops"] and _via(r1) == [f"n{int(node[1:]) - 1:02d}"]
        assert r0["bestPrefixEntry"] == r1["bestPrefixEntry"]
        assert r1["bestPrefixEntry"][2] == b"n00"
    for node in ("n01", "n02", "n03"):
        upd, dele = deltas[node]
        assert KEY not in upd and KEY not in dele, node


def test_igp_only_change_equal_layout(E, O):
    names, adj0, pfx0 = _net(_line_far_end(1), HI)
    _, adj1, pfx1 = _net(_line_far_end(2), HI)
    t0, t1 = _table(E, adj0, pfx0, True), _table(E, adj1, pfx1, True)
    assert t1.num_selected_columns == 1 and t1.num_bgp_prefixes == 1 and KEY in t1.prefixes
    deltas = _diff_all(t1, t0, _oracle_dbs(O, names, adj0, pfx0, True),
                       _oracle_dbs(O, names, adj1, pfx1, True))
    assert not t1.diff_was_mapped
    _expect_igp_only(deltas, t1, t0)


def test_igp_only_change_mapped(E, O):
    names0, adj0, pfx0 = _net(_line_far_end(1), HI)
    names1, adj1, pfx1 = _net(_line_far_end(2, stub=True), HI)
    assert names1 == names0 + ["n07"]
    # (n07's loopback takes the next index: the others keep theirs)
    assert pfx0 == pfx1[:7]
    t0, t1 = _table(E, adj0, pfx0, True), _table(E, adj1, pfx1, True)
    deltas = _diff_all(t1, t0, _oracle_dbs(O, names0, adj0, pfx0, True),
                       _oracle_dbs(O, names1, adj1, pfx1, True))
    assert t1.diff_was_mapped
    _expect_igp_only(deltas, t1, t0)
    upd, dele = deltas["n07"]
    assert dele == [] and upd == t1.routes("n07") and KEY in upd and len(upd) == 8


def test_all_areas_area_table(E):
    _, adj0, pfx0 = _net(_line_far_end(1), HI)
    _, adj1, pfx1 = _net(_line_far_end(2), HI)
    alls = []
    for adj, pfx in ((adj0, pfx0), (adj1, pfx1)):
        areas, ps = RZ.load(E, adj, pfx, 0)
        alls.append(E.AllAreasRouteTable(areas, ps, True, False, False, True,
                                         bgp_igp_on_device=True))
    a0, a1 = alls
    assert a1.area_table("nope") is None
    t0, t1 = a0.area_table("0"), a1.area_table("0")
    assert t1.num_selected_columns == 1
    deltas = _diff_all(t1, t0)
    assert not t1.diff_was_mapped
    _expect_igp_only(deltas, t1, t0)
    # the same deltas as the tables built directly
    d0, d1 = _table(E, adj0, pfx0, True), _table(E, adj1, pfx1, True)
    assert deltas == _diff_all(d1, d0)


# ------------------------------------- 3: a host-selected column flips its best


def test_host_selected_best_flips(E, O):
    names, adj0, pfx0 = _net(_line(7), {"n00": _mv(TB5), "n06": _mv(TB3)})
    _, adj1, pfx1 = _net(_line(7), {"n00": _mv(TB5), "n06": _mv(_ent(1, 10, WIP, True, [7]))})
    t0, t1 = _table(E, adj0, pfx0, False), _table(E, adj1, pfx1, False)
    assert t1.num_bgp_prefixes == 1 and t1.num_selected_columns == 0
    deltas = _diff_all(t1, t0, _oracle_dbs(O, names, adj0, pfx0, False),
                       _oracle_dbs(O, names, adj1, pfx1, False))
    for node in LINE:
        upd, dele = deltas[node]
        assert KEY not in dele
        if node in ("n00", "n06"):
            assert KEY not in upd  # both ends win: no route at either
            continue
        # both ends stay winners, the cell is the same: only the best entry moved
        r1, r0 = t1.routes(node)[KEY], t0.routes(node)[KEY]
        assert upd == {KEY: r1}, node
        assert r0["nexthops"] == r1["nexthops"]
        assert (r0["bestPrefixEntry"][2], r1["bestPrefixEntry"][2]) == (b"n00", b"n06")


# ---------------------------------------------------- 4: the column kind changes


@pytest.mark.parametrize("igp", [True, False])
def test_column_kind_changes(E, O, igp):
    names, adj0, pfx0 = _net(_line(7), {"n00": _mv(TB5)})
    _, adj1, pfx1 = _net(_line(7), {})
    n00 = next(p for p in pfx1 if p.thisNodeName == "n00")
    n00.prefixEntries.append(T.createPrefixEntry(T.toIpPrefix(PFX)))
    t0, t1 = _table(E, adj0, pfx0, igp), _table(E, adj1, pfx1, igp)
    assert (t0.num_bgp_prefixes, t1.num_bgp_prefixes) == (1, 0)
    assert KEY in t0.prefixes and KEY in t1.prefixes
    deltas = _diff_all(t1, t0, _oracle_dbs(O, names, adj0, pfx0, igp),
                       _oracle_dbs(O, names, adj1, pfx1, igp))
    assert t1.diff_was_mapped
    assert deltas["n00"] == ({}, [])
    for node in LINE[1:]:
        upd, dele = deltas[node]
        assert dele == [] and upd == {KEY: t1.routes(node)[KEY]}, node
        assert upd[KEY]["bestNexthop"] is None and t0.routes(node)[KEY]["bestNexthop"] is not None


# -------------------------- 5: candidates of a selected column come, go or move

THREE = {"n00": _mv(TB5), "n03": _mv(TB3), "n06": _mv(TB3)}


def test_selected_candidate_withdrawn(E, O):
    names, adj0, pfx0 = _net(_line(7), THREE)
    _, adj1, pfx1 = _net(_line(7), {"n00": _mv(TB5), "n03": _mv(TB3)})
    t0, t1 = _table(E, adj0, pfx0, True), _table(E, adj1, pfx1, True)
    deltas = _diff_all(t1, t0, _oracle_dbs(O, names, adj0, pfx0, True),
                       _oracle_dbs(O, names, adj1, pfx1, True))
    assert t1.diff_was_mapped
    # n05 went to its neighbour n06 and now goes to n03; n06 gains a route
    assert _via(deltas["n05"][0][KEY]) == ["n04"] and _via(t0.routes("n05")[KEY]) == ["n06"]
    assert KEY in deltas["n06"][0] and KEY not in t0.routes("n06")
    assert KEY not in deltas["n01"][0] and KEY not in deltas["n01"][1]


def test_selected_candidate_loopback_changes(E, O):
    names, adj0, pfx0 = _net(_line(7), THREE)
    adj1, pfx1 = copy.deepcopy(adj0), copy.deepcopy(pfx0)
    n06 = next(p for p in pfx1 if p.thisNodeName == "n06")
    old = n06.prefixEntries[0].prefix
    n06.prefixEntries[0] = T.createPrefixEntry(T.toIpPrefix("fc00:77::1/128"))
    t0, t1 = _table(E, adj0, pfx0, True), _table(E, adj1, pfx1, True)
    deltas = _diff_all(t1, t0, _oracle_dbs(O, names, adj0, pfx0, True),
                       _oracle_dbs(O, names, adj1, pfx1, True))
    assert t1.diff_was_mapped
    # the cell is the same; the best candidate's loopback is the bestNexthop
    r1, r0 = t1.routes("n05")[KEY], t0.routes("n05")[KEY]
    assert deltas["n05"][0][KEY] == r1 and r1["nexthops"] == r0["nexthops"]
    assert r0["bestNexthop"][0] == bytes(old.prefixAddress.addr) != r1["bestNexthop"][0]
    assert KEY not in deltas["n01"][0]  # best n00 there


# ------------------------------------------------------------- 6: random churn

BGP_KEYS = {(bytes(T.toIpPrefix(p).prefixAddress.addr), 48) for p in RZ._BGP_PREFIXES}
SEEDS = (12, 9, 0, 14)  # the oracle check runs on the first two (9: bgp_dry_run)


def _all_reach(adj_dbs):
    """every node reaches every other over usable links, drained nodes no transit"""
    dbs = {db.thisNodeName: db for db in adj_dbs["0"]}
    nbrs = {}
    for u, db in dbs.items():
        for a in db.adjacencies:
            v = a.otherNodeName
            back = v in dbs and any(b.otherNodeName == u and b.ifName == a.otherIfName
                                    and not b.isOverloaded for b in dbs[v].adjacencies)
            if back and not a.isOverloaded:
                nbrs.setdefault(u, set()).add(v)
    for s in dbs:
        seen, todo = {s}, [s]
        while todo:
            u = todo.pop()
            if u != s and dbs[u].isOverloaded:
                continue
            for v in nbrs.get(u, ()):
                if v not in seen:
                    seen.add(v)
                    todo.append(v)
        if len(seen) != len(dbs):
            return False
    return True


def _bgp_ip_entries(prefix_dbs):
    return [(pdb, e) for pdb in prefix_dbs for e in pdb.prefixEntries
            if e.type == T.PrefixType.BGP and e.forwardingType == T.PrefixForwardingType.IP]


def _churn(seed, adj_dbs, prefix_dbs):
    """One link removed, one metric changed, one node drained (each keeping
    every node in reach of every other, so that host-selected columns stay on
    the device), one BGP entry's metric vector changed, one BGP announcer
    withdrawn."""
    adj_dbs, prefix_dbs = copy.deepcopy(adj_dbs), copy.deepcopy(prefix_dbs)
    rng = random.Random(seed)
    dbs = {db.thisNodeName: db for db in adj_dbs["0"]}
    order = sorted(dbs)
    rng.shuffle(order)

    def first(attempt):
        for n in order:
            trial = copy.deepcopy(adj_dbs)
            if attempt({db.thisNodeName: db for db in trial["0"]}, n) and _all_reach(trial):
                attempt(dbs, n)
                return n
        raise AssertionError("no such event keeps the network connected")

    def cut(d, n):
        if len(d[n].adjacencies) < 2:
            return False
        _unlink(d, n, d[n].adjacencies[0])
        return True

    def remetric(d, n):
        a = d[n].adjacencies[-1]
        back = [b for b in d[a.otherNodeName].adjacencies
                if b.otherNodeName == n and b.ifName == a.otherIfName]
        a.metric = back[0].metric = a.metric + 7
        return True

    def drain(d, n):
        if d[n].isOverloaded:
            return False
        d[n].isOverloaded = True
        return True

    first(cut)
    order.reverse()
    first(remetric)
    rng.shuffle(order)
    first(drain)
    bgp = _bgp_ip_entries(prefix_dbs)
    (_, changed), (pdb, withdrawn) = rng.sample(bgp, 2)
    changed.mv.metrics[0].metric[0] += 1
    pdb.prefixEntries.remove(withdrawn)
    return adj_dbs, prefix_dbs


def _random(seed):
    names, adj0, pfx0 = RZ.random_network(7000 + seed, n_nodes=40, n_links=120, bgp=True)
    adj1, pfx1 = _churn(seed, adj0, pfx0)
    return names, adj0, pfx0, adj1, pfx1


@pytest.mark.parametrize("lfa", [False, True])
@pytest.mark.parametrize("igp", [False, True])
@pytest.mark.parametrize("seed", SEEDS)
def test_random_churn(E, O, seed, igp, lfa):
    names, adj0, pfx0, adj1, pfx1 = _random(seed)
    dry = seed % 2 == 1
    t0 = _table(E, adj0, pfx0, igp, lfa, dry, seed=seed)
    t1 = _table(E, adj1, pfx1, igp, lfa, dry, seed=seed + 50)
    assert (t1.num_selected_columns > 0) == igp
    both = set(t1.prefixes) & set(t0.prefixes)
    assert both & BGP_KEYS
    before = after = None
    if seed in SEEDS[:2]:
        before = _oracle_dbs(O, names, adj0, pfx0, igp, lfa, dry, seed)
        after = _oracle_dbs(O, names, adj1, pfx1, igp, lfa, dry, seed + 50)
    deltas = _diff_all(t1, t0, before, after)
    assert t1.diff_was_mapped
    assert any(k in both & BGP_KEYS for upd, dele in deltas.values() for k in list(upd) + dele)


# ---------------------------------------------------------------- 7: refusals


def test_refusals(E):
    _, adj, pfx = _net(_line(7), HI)
    base = _table(E, adj, pfx, True)
    with pytest.raises(ValueError):
        _table(E, adj, pfx, True, dry=True).diff(base)
    with pytest.raises(ValueError):
        _table(E, adj, pfx, False).diff(base)
    with pytest.raises(ValueError):
        _table(E, adj, pfx, True, columns=False).diff(base)
    with pytest.raises(ValueError):
        _table(E, adj, pfx, True, lfa=True).diff(base)
    assert list(_table(E, adj, pfx, True).diff(base)) == [0] * 7
