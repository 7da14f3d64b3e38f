"""AllNodesRouteTable::applyPrefixChanges over BGP columns (bgp_in_place):
prefix churn applied to a resident bgp_columns table in place
(spf_route_table_patch_columns_sel), for host-selected columns (no IGP metric)
and selected columns (bgp_use_igp_metric).

Six rounds of PrefixState::updatePrefixDatabase on a random network; each
round's changed set goes to apply_prefix_changes.  After every round, for
every node: routes == a freshly built table's == the CPU oracle's buildRouteDb
over the prefixes the fresh table serves, delta == getRouteDelta
(Decision.cpp:47-85) of the oracle's RouteDbs before and after the round,
deltas()[i] == delta(node), no MPLS delta, the returned counts ==
changed_split.
"""

import pytest

from openr_amd import thrift as T
from tests.test_route_table_delta_bgp_gpu import BGP_KEYS
from tests.test_route_table_prefix_churn_gpu import World, _delta_py

pytestmark = pytest.mark.gpu

NEW = "2001:db8:77::/48"
_NEW = T.toIpPrefix(NEW)
NEW_KEY = (bytes(_NEW.prefixAddress.addr), _NEW.prefixLength)
ALL_BGP = BGP_KEYS | {NEW_KEY}


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


def _bgp(node, tie):
    mv = T.MetricVector(0, [T.createMetricEntity(1, 10, T.CompareType.WIN_IF_PRESENT, True, [tie])])
    return T.createPrefixEntry(_NEW, T.PrefixType.BGP, node, mv=mv)


class BgpWorld(World):
    def __init__(self, E, O, seed, lfa, igp):
        super().__init__(E, O, seed, lfa, bgp=True)
        self.igp = igp
        self.solvers = {n: O.SpfSolver(n, True, lfa, False, False, igp) for n in self.names}

    def oracle(self):
        return {n: self.solvers[n].buildRouteDb(n, self.oareas, self.ops) for n in self.names}

    def table(self, **kw):
        return self.E.AllNodesRouteTable(self.areas, "0", self.ps, True, self.lfa, bgp_columns=True,
                                         bgp_use_igp_metric=self.igp, **kw)

    def resident(self):
        return self.table(bgp_in_place=True, spare_columns=8, spare_selected_columns=8)


def _served(db, served):
    return {k: v for k, v in (db or {"unicast": {}})["unicast"].items() if k in served}


def check_round(w, t, counts, before, served0, mpls0):
    """-> (oracle RouteDbs after, the served prefixes, changed routes, changed BGP routes)"""
    after = w.oracle()
    fresh = w.table()
    served = set(fresh.prefixes)
    all_deltas = t.deltas()
    total = bgp = 0
    for i in range(len(counts)):
        node = t.node_name(i)
        got = t.routes(node)
        assert got == fresh.routes(node), node
        assert got == _served(after.get(node), served), node
        upd, dele = t.delta(node)
        want = _delta_py(_served(after.get(node), served), _served(before.get(node), served0))
        assert (upd, sorted(dele)) == want, node
        du, dd, mu, md = all_deltas[i]
        assert (du, sorted(dd)) == (upd, sorted(dele)), node
        assert (mu, list(md)) == ({}, []) and t.delta_mpls(node) == ({}, []), node
        assert t.mpls_routes(node) == mpls0[node], node
        assert t.changed_split(node) == (counts[i], 0), node
        assert len(upd) + len(dele) == counts[i], node
        total += counts[i]
        bgp += sum(k in ALL_BGP for k in list(upd) + list(dele))
    assert sorted(t.prefixes) == sorted(fresh.prefixes) and t.num_prefixes == fresh.num_prefixes
    assert t.count_routes() == fresh.count_routes()
    assert t.num_bgp_prefixes == fresh.num_bgp_prefixes
    assert t.num_selected_columns == fresh.num_selected_columns
    return after, served, total, bgp


@pytest.mark.parametrize("lfa", [False, True])
@pytest.mark.parametrize("igp", [False, True])
def test_six_rounds_of_bgp_churn(E, O, igp, lfa):
    w = BgpWorld(E, O, 0, lfa, igp)
    start = w.oracle()
    t0 = w.table()
    t = w.resident()
    served = served_start = set(t0.prefixes)
    assert sorted(t.prefixes) == sorted(t0.prefixes) and t.count_routes() == t0.count_routes()
    assert t.num_bgp_prefixes > 0 and (t.num_selected_columns > 0) == igp
    assert t.free_columns == 8 and t.free_selected_columns == (8 if igp else 0)
    mpls0 = {n: t.mpls_routes(n) for n in w.names}
    before = start
    bgp_total = 0

    def apply(nodes):
        nonlocal before, served, bgp_total
        counts = t.apply_prefix_changes(w.ps, w.publish(nodes))
        before, served, total, bgp = check_round(w, t, counts, before, served, mpls0)
        assert total > 0
        bgp_total += bgp
        return bgp

    def free():
        return t.free_columns, t.free_selected_columns

    def take(f, plain=0, selected=0):
        # (selected columns exist under igp only: a BGP prefix takes a plain one otherwise)
        return (f[0] - plain - (0 if igp else selected), f[1] - (selected if igp else 0))

    # a new BGP prefix, announced by three nodes; z's vector wins
    x, y, z = w.in_graph[3:6]
    f = free()
    w.pdbs[x].prefixEntries.append(_bgp(x, 5))
    w.pdbs[y].prefixEntries.append(_bgp(y, 3))
    w.pdbs[z].prefixEntries.append(_bgp(z, 9))
    assert apply([x, y, z]) > 0 and NEW_KEY in served
    assert free() == take(f, selected=1)
    # a BGP candidate, the winner, withdrawn: x's vector wins
    w.pdbs[z].prefixEntries.pop()
    assert apply([z]) > 0
    # y's metric vector changes and now wins: the best path flips
    w.pdbs[y].prefixEntries[-1] = _bgp(y, 7)
    assert apply([y]) > 0
    # the loopback of y, the best announcer, changes (its loopback prefix is
    # replaced: one column freed, one taken): the BGP routes' bestNexthop moves
    # although the BGP prefix itself is not in the changed set
    f = free()
    w.pdbs[y].prefixEntries[0] = T.createPrefixEntry(T.toIpPrefix("fc00:77::1/128"))
    assert apply([y]) > 0
    assert free() == f
    # the prefix moves BGP -> Open/R and back (the column kind changes)
    f = free()
    w.pdbs[x].prefixEntries[-1] = T.createPrefixEntry(_NEW)
    w.pdbs[y].prefixEntries[-1] = T.createPrefixEntry(_NEW)
    assert apply([x, y]) > 0
    assert free() == ((f[0] - 1, f[1] + 1) if igp else f)
    w.pdbs[x].prefixEntries[-1] = _bgp(x, 5)
    w.pdbs[y].prefixEntries[-1] = _bgp(y, 7)
    assert apply([x, y]) > 0
    assert free() == f
    # withdrawn by all of its announcers, then announced again: the freed
    # column is the one reused
    ex, ey = w.pdbs[x].prefixEntries.pop(), w.pdbs[y].prefixEntries.pop()
    assert apply([x, y]) > 0 and NEW_KEY not in served
    assert free() == take(f, selected=-1)
    w.pdbs[x].prefixEntries.append(ex)
    w.pdbs[y].prefixEntries.append(ey)
    assert apply([x, y]) > 0 and NEW_KEY in served
    assert free() == f
    assert bgp_total > 0
    # diff against the starting table == the oracle's overall delta
    final = before
    counts = t.diff(t0)
    for i, c in enumerate(counts):
        node = t.node_name(i)
        upd, dele = t.delta(node)
        want = _delta_py(_served(final.get(node), served), _served(start.get(node), served_start))
        assert (upd, sorted(dele)) == want, node
        assert t.delta_mpls(node) == ({}, []), node
        assert sum(t.changed_split(node)) == c, node
    assert sum(counts) > 0
    t1 = w.table()
    assert sum(t1.diff(t)) == 0
    for i in range(len(counts)):
        assert t1.delta(t1.node_name(i)) == ({}, [])


def test_more_new_selected_prefixes_than_free_selected_columns(E, O):
    w = BgpWorld(E, O, 1, False, True)
    t = w.table(bgp_in_place=True, spare_columns=4, spare_selected_columns=1)
    routes = {n: t.routes(n) for n in w.names}
    a, b = w.in_graph[3], w.in_graph[5]
    w.pdbs[a].prefixEntries.append(_bgp(a, 5))
    other = T.createPrefixEntry(T.toIpPrefix("2001:db8:78::/48"), T.PrefixType.BGP, b,
                                mv=_bgp(b, 3).mv)
    w.pdbs[b].prefixEntries.append(other)
    with pytest.raises(ValueError):  # std::length_error
        t.apply_prefix_changes(w.ps, w.publish([a, b]))
    assert (t.free_columns, t.free_selected_columns) == (4, 1)
    assert {n: t.routes(n) for n in w.names} == routes


def test_bgp_columns_need_the_flag(E, O):
    """Without bgp_in_place a bgp_columns table refuses the call as before."""
    w = BgpWorld(E, O, 2, False, True)
    t = w.table(spare_columns=4, spare_selected_columns=2)
    assert t.free_selected_columns == 2
    n = w.in_graph[0]
    w.pdbs[n].prefixEntries.append(_bgp(n, 1))
    with pytest.raises(ValueError):
        t.apply_prefix_changes(w.ps, w.publish([n]))


def test_border_nodes_table_is_still_refused(E, O):
    """bgp_in_place does not open a borderNodes table to the call."""
    w = BgpWorld(E, O, 3, False, True)
    t = w.table(bgp_in_place=True, spare_columns=4, spare_selected_columns=2,
                border_nodes={w.in_graph[0]})
    routes = {n: t.routes(n) for n in w.names}
    n = w.in_graph[7]
    w.pdbs[n].prefixEntries.append(_bgp(n, 1))
    with pytest.raises(ValueError):  # std::invalid_argument
        t.apply_prefix_changes(w.ps, w.publish([n]))
    assert (t.free_columns, t.free_selected_columns) == (4, 2)
    assert {n: t.routes(n) for n in w.names} == routes


@pytest.mark.parametrize("lfa", [False, True])
def test_selected_candidates_with_equal_entries_and_one_loopback_address(E, O, lfa):
    """Two candidates whose PrefixEntries are equal and whose nodes announce
    the same loopback address: where best moves from one to the other the
    materialised bestPrefixEntry and loopback are equal, so only what else
    moved (next hops, igp) makes a route change -- the oracle decides."""
    w = BgpWorld(E, O, 1, lfa, True)
    a, b = w.in_graph[2], w.in_graph[9]
    same = T.createPrefixEntry(T.toIpPrefix("fc00:99::1/128"))
    w.pdbs[a].prefixEntries[0] = same
    w.pdbs[b].prefixEntries[0] = same
    w.pdbs[a].prefixEntries.append(_bgp("same", 4))
    w.publish([a, b])
    t = w.resident()
    before, served = w.oracle(), set(w.table().prefixes)
    assert NEW_KEY in served
    mpls0 = {n: t.mpls_routes(n) for n in w.names}
    w.pdbs[b].prefixEntries.append(_bgp("same", 4))
    counts = t.apply_prefix_changes(w.ps, w.publish([b]))
    before, served, total, bgp = check_round(w, t, counts, before, served, mpls0)
    assert bgp > 0
    w.pdbs[a].prefixEntries.pop()
    counts = t.apply_prefix_changes(w.ps, w.publish([a]))
    _, _, total, bgp = check_round(w, t, counts, before, served, mpls0)
    assert bgp > 0
