"""AllNodesRouteTable::applyTopologyChanges with links_in_place: links that go
down and come back (an adjacency withdrawn or announced again, a link overload
bit) applied to a resident table in place, at the level a Decision-style caller
uses it.

Six rounds of LinkState::updateAdjacencyDatabase on the random network of
tests/test_route_table_topology_churn_gpu.py: a link withdrawn on both sides; a
second one withdrawn with two metric changes elsewhere, then a prefix announced
in place; the first link back with another metric and adjacency label; every
link of one node withdrawn and restored; a link drained together with a node;
nothing changed.  After every round every claim of that module's check_round
holds (routes, MPLS routes, delta, delta_mpls, deltas against a fresh table and
the CPU oracle; counts; a zero diff against the fresh table both ways), plus
down_links and refresh_rows <= num_nodes.
"""

import pytest

from openr_amd import thrift as T
from tests.test_route_table_topology_churn_gpu import (E, NEW, O, World, _routes,  # noqa: F401
                                                       _unicast, check_round)

pytestmark = pytest.mark.gpu


def up_links(w, avoid=()):
    """(u, adjacency at u, v, adjacency at v) of links that are up, u < v."""
    out = []
    for n, a in w.up_adjacencies():
        v = a.otherNodeName
        if n < v and v in w.adj and n not in avoid and v not in avoid:
            back = [b for b in w.adj[v].adjacencies
                    if b.otherNodeName == n and b.ifName == a.otherIfName]
            if len(back) == 1 and not back[0].isOverloaded:
                out.append((n, a, v, back[0]))
    return out


def withdraw(w, link):
    u, a, v, b = link
    w.adj[u].adjacencies.remove(a)
    w.adj[v].adjacencies.remove(b)
    return {u, v}


def announce(w, link):
    u, a, v, b = link
    w.adj[u].adjacencies.append(a)
    w.adj[v].adjacencies.append(b)
    return {u, v}


def apply(w, t, before, down_links):
    counts = t.apply_topology_changes(w.areas, "0")
    before, total = check_round(w, t, counts, before)
    assert t.down_links == down_links and t.refresh_rows <= t.num_nodes
    return before, total


@pytest.mark.parametrize("lfa", [False, True])
@pytest.mark.parametrize("seed", range(4))
def test_six_rounds_of_link_churn(E, O, seed, lfa):  # noqa: F811
    w = World(E, O, seed, lfa)
    t = w.table(links_in_place=True, spare_columns=4)
    assert t.down_links == 0
    before = w.oracle()
    # the node of round 4 and links that do not touch it
    hub = next(n for n in w.in_graph if len(w.adj[n].adjacencies) >= 3
               and all(not a.isOverloaded for a in w.adj[n].adjacencies)
               and sum(1 for l in up_links(w) if n in (l[0], l[2])) == len(w.adj[n].adjacencies))
    first, second, third = w.rng.sample(up_links(w, avoid={hub}), 3)
    # round 1: one link withdrawn on both sides
    w.publish_adj(withdraw(w, first))
    before, total = apply(w, t, before, 1)
    assert total > 0
    # round 2: a second link withdrawn and two metrics changed elsewhere, then
    # a prefix announced into a spare column
    w.publish_adj(withdraw(w, second) | w.change_metrics(2))
    before, total = apply(w, t, before, 2)
    assert total > 0
    a = w.rng.choice(w.in_graph)
    w.pdbs[a].prefixEntries.append(T.createPrefixEntry(T.toIpPrefix(NEW)))
    t.apply_prefix_changes(w.ps, w.publish_prefixes([a]))
    before = w.oracle()
    fresh = w.table()
    for n in w.names:
        assert t.routes(n) == fresh.routes(n) == _unicast(before.get(n)), n
    # round 3: the first link returns with another metric and adjacency label
    first[1].metric = first[1].metric % 20 + 3
    first[1].adjLabel = 59980
    w.publish_adj(announce(w, first))
    before, total = apply(w, t, before, 1)
    assert total > 0
    # round 4: every link of one node withdrawn (it keeps its empty adjacency
    # database), then restored
    mine = [l for l in up_links(w) if hub in (l[0], l[2])]
    assert len(mine) == len(w.adj[hub].adjacencies) >= 3
    touched = set()
    for l in mine:
        touched |= withdraw(w, l)
    assert w.adj[hub].adjacencies == []
    w.publish_adj(touched)
    before, total = apply(w, t, before, 1 + len(mine))
    assert total > 0 and t.routes(hub) == {}
    for l in mine:
        announce(w, l)
    w.publish_adj(touched)
    before, total = apply(w, t, before, 1)
    assert total > 0
    # round 5: a link drained (down for the engine) together with a node drain
    third[1].isOverloaded = True
    w.publish_adj({third[0]} | w.toggle_drains())
    before, total = apply(w, t, before, 2)
    assert total > 0 and t.refresh_rows == t.num_nodes
    # round 6: nothing changed
    before, total = apply(w, t, before, 2)
    assert total == 0 and t.refresh_rows == 0


@pytest.mark.parametrize("event", ["link_added", "node_joined", "node_label", "metric_zero",
                                   "returns_with_another_address"])
def test_refused_changes_with_the_flag_on(E, O, event):  # noqa: F811
    w = World(E, O, 1, False)
    t = w.table(links_in_place=True)
    link = next(l for l in up_links(w) if len(w.adj[l[0]].adjacencies) > 2
                and len(w.adj[l[2]].adjacencies) > 2)
    u, a, v, b = link
    touched = {u, v}
    if event == "returns_with_another_address":
        w.publish_adj(withdraw(w, link))
        t.apply_topology_changes(w.areas, "0")
        assert t.down_links == 1
        a.nextHopV6 = T.toBinaryAddress("fe80::cc:1")
        announce(w, link)
    elif event == "link_added":
        w.adj[u].adjacencies.append(T.createAdjacency(
            v, "if_new_u", "if_new_v", "fe80::aa:1", "10.251.0.1", 3, 58001))
        w.adj[v].adjacencies.append(T.createAdjacency(
            u, "if_new_v", "if_new_u", "fe80::aa:2", "10.251.0.2", 3, 58002))
    elif event == "node_joined":
        new = "n500000-new"
        w.adj[new] = T.createAdjDb(new, [T.createAdjacency(
            u, "if_join_n", "if_join_u", "fe80::bb:1", "10.252.0.1", 2, 58003)], 9001, False, "0")
        w.adj[u].adjacencies.append(T.createAdjacency(
            new, "if_join_u", "if_join_n", "fe80::bb:2", "10.252.0.2", 2, 58004))
        touched = {u, new}
    elif event == "node_label":
        w.adj[u].nodeLabel = 9002
        touched = {u}
    else:
        a.metric = 0  # needs 64-bit rows
        touched = {u}
    routes = _routes(w, t)
    down = t.down_links
    w.publish_adj(touched)
    with pytest.raises(ValueError):  # std::invalid_argument
        t.apply_topology_changes(w.areas, "0")
    assert _routes(w, t) == routes and t.down_links == down


def test_without_the_flag_a_withdrawn_link_is_still_refused(E, O):  # noqa: F811
    w = World(E, O, 1, False)
    t = w.table(links_in_place=False)
    routes = _routes(w, t)
    link = next(l for l in up_links(w) if len(w.adj[l[0]].adjacencies) > 2)
    w.publish_adj(withdraw(w, link))
    with pytest.raises(ValueError):  # std::invalid_argument
        t.apply_topology_changes(w.areas, "0")
    assert _routes(w, t) == routes and t.down_links == 0
