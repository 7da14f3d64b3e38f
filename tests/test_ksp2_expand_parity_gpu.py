"""KSP2 RouteDbs with the traced paths' costs and label stacks from the
device (OPENR_KSP2_DEVICE_EXPAND=1, spf_path_expand_kernel) against the CPU
oracle: seeded random networks whose KSP2 / SR-MPLS prefixes carry prepend
labels and minNexthop thresholds, forced trace overflows, the cluster path,
a node-label change that keeps the topology, and the variable unset."""

import copy

import pytest

from openr_amd import thrift as T
from tests import randomized as RZ

pytestmark = pytest.mark.gpu

EXPANDED = "decision.ksp2_device_expanded"


@pytest.fixture(scope="module")
def mods(gpu_ready):
    from oracle import _oracle_ref
    import openr_amd._openr_spf as E

    return E, _oracle_ref


def ksp2_entry(prefix, label, min_nexthop=None):
    e = T.createPrefixEntry(
        T.toIpPrefix(prefix),
        forwardingType=T.PrefixForwardingType.SR_MPLS,
        forwardingAlgorithm=T.PrefixForwardingAlgorithm.KSP2_ED_ECMP,
        minNexthop=min_nexthop,
    )
    e.prependLabel = label
    return e


def network(seed):
    """RZ.random_network plus KSP2_ED_ECMP / SR_MPLS prefixes with prepend
    labels (minNexthop 1 / 2 / 5 on some) and one anycast KSP2 prefix."""
    names, adj_dbs, prefix_dbs = RZ.random_network(seed, n_nodes=30, n_links=80)
    by_node = {p.thisNodeName: p for p in prefix_dbs}
    mins = (None, 1, None, 2, None, 5)
    for idx, n in enumerate(names):
        by_node[n].prefixEntries.append(
            ksp2_entry(f"fd77:{idx:x}::/64", 60000 + idx, mins[idx % len(mins)]))
    for idx in (3, 11, 19):
        by_node[names[idx]].prefixEntries.append(ksp2_entry("fd99::/64", 61000 + idx))
    return names, adj_dbs, prefix_dbs


def build_six(E, O, names, ea, ep, oa, op):
    es = E.SpfSolver(names[0], True, False)
    os_ = O.SpfSolver(names[0], True, False)
    out = []
    for node in names[:6]:
        got = es.buildRouteDb(node, ea, ep)
        assert got == os_.buildRouteDb(node, oa, op), node
        out.append(got)
    return out


def run(E, O, seed):
    names, adj_dbs, prefix_dbs = network(seed)
    ea, ep = RZ.load(E, adj_dbs, prefix_dbs, seed)
    oa, op = RZ.load(O, adj_dbs, prefix_dbs, seed)
    E.reset_counters()
    O.reset_counters()
    dbs = build_six(E, O, names, ea, ep, oa, op)
    c = E.get_counters()
    assert c.get("decision.spf_runs") == O.get_counters().get("decision.spf_runs")
    return names, adj_dbs, (ea, ep, oa, op), dbs, c


@pytest.mark.parametrize("seed", [900, 901, 902])
def test_ksp2_route_db_device_expand(mods, seed, monkeypatch):
    monkeypatch.setenv("OPENR_KSP2_DEVICE_EXPAND", "1")
    E, O = mods
    *_, c = run(E, O, seed)
    assert c.get(EXPANDED, 0) > 0
    assert c.get("decision.kth_expand_us") is not None


@pytest.mark.parametrize("seed", [900, 901, 902])
def test_ksp2_expand_with_trace_overflows(mods, seed, monkeypatch):
    """Traces the device gives up on (a link capacity of 6) are traced and
    walked on the host; the rest still come from the expansion."""
    monkeypatch.setenv("OPENR_KSP2_DEVICE_EXPAND", "1")
    monkeypatch.setenv("OPENR_SPF_TRACE_CAP", "6")
    E, O = mods
    *_, c = run(E, O, seed)
    assert c.get(EXPANDED, 0) > 0


@pytest.mark.parametrize("seed", [900, 901, 902])
def test_ksp2_expand_cluster_path(mods, seed, monkeypatch):
    monkeypatch.setenv("OPENR_KSP2_DEVICE_EXPAND", "1")
    E, O = mods
    E.set_spf_devices([0])
    E.set_cluster_min_sources(1)
    try:
        *_, c = run(E, O, seed)
        assert c.get("decision.spf_cluster_batches", 0) > 0
        assert c.get(EXPANDED, 0) > 0
    finally:
        E.set_cluster_min_sources(64)
        E.set_spf_devices([])


def walk(ls, labels, src, path):
    at, cost, seen = src, 0, []
    for link in path:
        cost += link.getMetricFromNode(at)
        at = link.getOtherNodeName(at)
        seen.append(labels[at])
    return cost, seen[:0:-1]


def test_kth_path_expansion_accessor(mods, monkeypatch):
    monkeypatch.setenv("OPENR_KSP2_DEVICE_EXPAND", "1")
    E, O = mods
    names, adj_dbs, (ea, *_), _, _ = run(E, O, 900)
    ls = ea["0"]
    labels = {db.thisNodeName: db.nodeLabel for db in adj_dbs["0"]}
    src, stored = names[0], 0
    for dst in names[1:]:
        for k in (1, 2):
            got = ls.getKthPathExpansion(src, dst, k)
            paths = ls.getKthPaths(src, dst, k)
            if got is None:
                continue
            stored += 1
            assert [(c, list(s)) for c, s in got] == [walk(ls, labels, src, p) for p in paths], (dst, k)
    assert stored > len(names)


def test_label_change_without_topology_change(mods, monkeypatch):
    """A new nodeLabel with the same adjacencies keeps the k-th path memo;
    the stacks stored under the old label are not served."""
    monkeypatch.setenv("OPENR_KSP2_DEVICE_EXPAND", "1")
    E, O = mods
    names, adj_dbs, (ea, ep, oa, op), before, _ = run(E, O, 901)
    ls = ea["0"]
    src = names[0]
    # a node whose label is inside a stored stack that a route of the first
    # node's RouteDb carries
    def stacks(db_):
        # next hop: (address, ifName, weight, (action, swapLabel, pushLabels), ...)
        return [l for r in db_["unicast"].values() for nh in r["nexthops"]
                for l in ((nh[3] or (0, None, None))[2] or ())]

    by_label = {db.nodeLabel: db for db in adj_dbs["0"]}
    served = set(stacks(before[0]))
    pick = None
    for dst in names[1:]:
        for k in (1, 2):
            for _, stack in ls.getKthPathExpansion(src, dst, k) or []:
                if pick is None and stack and stack[-1] in served and stack[-1] in by_label:
                    pick = (dst, k, by_label[stack[-1]])
    assert pick is not None
    dst, k, db = pick
    db = copy.deepcopy(db)
    old = db.nodeLabel
    db.nodeLabel = 7000
    runs = E.get_counters().get("decision.spf_runs")
    for M, areas in ((E, ea), (O, oa)):
        areas["0"].updateAdjacencyDatabase(db)
    assert ls.getKthPathExpansion(src, dst, k) is None  # stale: not served
    after = build_six(E, O, names, ea, ep, oa, op)
    assert E.get_counters().get("decision.spf_runs") == runs  # the memo survived
    assert after[0] != before[0]

    assert old in stacks(before[0])
    assert old not in stacks(after[0]) and 7000 in stacks(after[0])


def test_variable_unset(mods, monkeypatch):
    monkeypatch.delenv("OPENR_KSP2_DEVICE_EXPAND", raising=False)
    E, O = mods
    *_, c = run(E, O, 900)
    assert c.get(EXPANDED, 0) == 0
    assert "decision.kth_expand_us" not in c
