"""AllNodesRouteTable::applyPrefixChanges: prefix churn applied to a resident
table in place (spf_route_table_patch_columns), at the level a Decision-style
caller uses it.

Three rounds of PrefixState::updatePrefixDatabase on a random network; each
round's returned prefix sets, merged, go to apply_prefix_changes.  After every
round, for every node: routes == a freshly built table's == the CPU oracle's
buildRouteDb (ECMP prefixes), delta == getRouteDelta (Decision.cpp:47-85) of
the oracle's RouteDbs before and after the round, deltas()[i] == delta(node),
no MPLS delta, and the returned counts == changed_split.
"""

import copy

import pytest

from openr_amd import thrift as T
from tests import randomized as RZ

pytestmark = pytest.mark.gpu

ANYCAST = "fc99::1/128"
NEW, SRMPLS = "fc77::1/128", "fd00:ffff::/64"


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
    """getRouteDelta (Decision.cpp:47-85) over route dicts."""
    upd = {k: v for k, v in new.items() if old.get(k) != v}
    dele = sorted(k for k in old if k not in new)
    return upd, dele


def _has(pdb, prefix):
    return any(e.prefix == T.toIpPrefix(prefix) for e in pdb.prefixEntries)


class World:
    """The network, both PrefixStates (engine and oracle) and the oracle's
    RouteDbs of the current state."""

    def __init__(self, E, O, seed, lfa, bgp=False):
        self.E, self.O, self.lfa = E, O, lfa
        self.names, adj, pfx = RZ.random_network(
            4100 + seed, n_nodes=40, n_links=90, overload_prob=0.1, link_overload_prob=0.03,
            bgp=bgp)
        self.pdbs = {p.thisNodeName: copy.deepcopy(p) for p in pfx}
        self.areas, self.ps = RZ.load(E, adj, list(self.pdbs.values()), seed)
        self.oareas, self.ops = RZ.load(O, adj, list(self.pdbs.values()), seed)
        self.solver = O.SpfSolver(self.names[0], True, lfa)
        self.in_graph = [db.thisNodeName for db in adj["0"]]

    def oracle(self):
        return {n: self.solver.buildRouteDb(n, self.oareas, self.ops) for n in self.names}

    def table(self, **kw):
        return self.E.AllNodesRouteTable(self.areas, "0", self.ps, True, self.lfa, **kw)

    def publish(self, nodes):
        """updatePrefixDatabase of the touched nodes on both sides; the merged changed set."""
        changed = set()
        for n in nodes:
            changed |= set(self.ps.updatePrefixDatabase(self.pdbs[n]))
            self.ops.updatePrefixDatabase(self.pdbs[n])
        return changed


def _unicast(db):
    return _ecmp_only(db["unicast"]) if db else {}


def check_round(w, t, counts, before, mpls0):
    after = w.oracle()
    fresh = w.table()
    all_deltas = t.deltas()
    nodes = [t.node_name(i) for i in range(len(counts))]
    total = 0
    for i, node in enumerate(nodes):
        got = t.routes(node)
        assert got == fresh.routes(node), node
        assert got == _unicast(after.get(node)), node
        upd, dele = t.delta(node)
        want = _delta_py(_unicast(after.get(node)), _unicast(before.get(node)))
        assert (sorted(upd), sorted(dele)) == (sorted(want[0]), want[1]), node
        assert (upd, sorted(dele)) == want, node
        du, dd, mu, md = all_deltas[i]
        assert (du, sorted(dd)) == (upd, sorted(dele)), node
        assert (mu, list(md)) == ({}, []) and t.delta_mpls(node) == ({}, []), node
        assert t.mpls_routes(node) == mpls0[node], node
        assert t.changed_split(node) == (counts[i], 0), node
        assert len(upd) + len(dele) == counts[i], node
        total += counts[i]
    assert sorted(t.prefixes) == sorted(fresh.prefixes) and t.num_prefixes == fresh.num_prefixes
    assert t.count_routes() == fresh.count_routes()
    return after, total


def three_rounds(w, t):
    """The events of the issue; returns the oracle's RouteDbs after round 3."""
    a, b, c, d, f, g = [n for n in w.in_graph if not _has(w.pdbs[n], ANYCAST)][2:8]
    mpls0 = {n: t.mpls_routes(n) for n in w.names}
    before = w.oracle()
    assert t.free_columns == 8
    # round 1: a new prefix, a prefix withdrawn by its only announcer, a second
    # (or first more) announcer of the anycast prefix, an SR_MPLS prefix
    w.pdbs[a].prefixEntries.append(T.createPrefixEntry(T.toIpPrefix(NEW)))
    gone = w.pdbs[b].prefixEntries.pop(0)
    w.pdbs[c].prefixEntries.append(T.createPrefixEntry(T.toIpPrefix(ANYCAST)))
    w.pdbs[d].prefixEntries.append(T.createPrefixEntry(
        T.toIpPrefix(SRMPLS), forwardingType=T.PrefixForwardingType.SR_MPLS,
        forwardingAlgorithm=T.PrefixForwardingAlgorithm.KSP2_ED_ECMP))
    counts = t.apply_prefix_changes(w.ps, w.publish([a, b, c, d]))
    before, total = check_round(w, t, counts, before, mpls0)
    assert total > 0 and t.free_columns == 8  # one taken, one freed, none for SR_MPLS
    assert t.patch_ms >= 0.0
    # round 2: an announcer moved to another node, a PrefixEntry field changed
    w.pdbs[a].prefixEntries = [e for e in w.pdbs[a].prefixEntries if e.prefix != T.toIpPrefix(NEW)]
    w.pdbs[f].prefixEntries.append(T.createPrefixEntry(T.toIpPrefix(NEW)))
    w.pdbs[g].prefixEntries[0].data = b"churn"
    counts = t.apply_prefix_changes(w.ps, w.publish([a, f, g]))
    before, total = check_round(w, t, counts, before, mpls0)
    assert total > 0 and t.free_columns == 8
    # round 3: the withdrawn prefix announced again (the freed column is the
    # first one taken)
    w.pdbs[b].prefixEntries.insert(0, gone)
    counts = t.apply_prefix_changes(w.ps, w.publish([b]))
    before, total = check_round(w, t, counts, before, mpls0)
    assert total > 0 and t.free_columns == 7
    return before


@pytest.mark.parametrize("lfa", [False, True])
def test_three_rounds_of_prefix_churn(E, O, lfa):
    w = World(E, O, 0, lfa)
    start = w.oracle()
    t0 = w.table()  # spare_columns = 0, the default: the state before the rounds
    t = w.table(spare_columns=8)
    assert sorted(t.prefixes) == sorted(t0.prefixes) and t.count_routes() == t0.count_routes()
    final = three_rounds(w, t)
    # diff across spare and freed columns, both ways
    counts = t.diff(t0)
    for i, c in enumerate(counts):
        node = t.node_name(i)
        upd, dele = t.delta(node)
        assert (upd, sorted(dele)) == _delta_py(_unicast(final.get(node)), _unicast(start.get(node))), node
        assert t.delta_mpls(node) == ({}, []), node
        assert sum(t.changed_split(node)) == c, node
    assert sum(counts) > 0
    t1 = w.table()
    assert sum(t1.diff(t)) == 0
    for i in range(len(counts)):
        assert t1.delta(t1.node_name(i)) == ({}, [])


def test_more_new_prefixes_than_free_columns(E, O):
    w = World(E, O, 1, False)
    t = w.table(spare_columns=1)
    routes = {n: t.routes(n) for n in w.names}
    a, b = w.in_graph[3], w.in_graph[5]
    w.pdbs[a].prefixEntries.append(T.createPrefixEntry(T.toIpPrefix("fc77::2/128")))
    w.pdbs[b].prefixEntries.append(T.createPrefixEntry(T.toIpPrefix("fc77::3/128")))
    with pytest.raises(ValueError):  # std::length_error
        t.apply_prefix_changes(w.ps, w.publish([a, b]))
    assert t.free_columns == 1
    assert {n: t.routes(n) for n in w.names} == routes


def test_bgp_columns_table_is_refused(E, O):
    w = World(E, O, 2, False, bgp=True)
    t = w.table(bgp_columns=True, spare_columns=4)
    routes = {n: t.routes(n) for n in w.names}
    n = next(n for n in w.in_graph
             if any(e.type == T.PrefixType.BGP for e in w.pdbs[n].prefixEntries))
    w.pdbs[n].prefixEntries = [e for e in w.pdbs[n].prefixEntries if e.type != T.PrefixType.BGP]
    with pytest.raises(ValueError):  # std::invalid_argument
        t.apply_prefix_changes(w.ps, w.publish([n]))
    assert t.free_columns == 4
    assert {n: t.routes(n) for n in w.names} == routes
