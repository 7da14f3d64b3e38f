"""spf_route_select_kernel through the C ABI (ctypes): the per-node BGP best
path fold of selected columns (include/openr_spf.h, spf_route_table_create_sel;
reference runBestPathSelectionBgp with bgpUseIgpMetric,
openr/decision/Decision.cpp:714-803, and selectEcmpBgp :805-866).

The expected cells come from a pure-Python fold over the query's own
distance rows (spf_query_dist) with the rule of the header: candidates in
order, unreachable ones skipped, the pair code chosen by the sign of the
distance difference, igp = min over every reachable candidate, drained
filter on the winners, no route on TIE / ERROR, an empty mask, the row's
node among the filtered winners or a best candidate without loopback.  No
oracle is involved: pair tables hold random codes, so folds no metric vector
could produce are covered too.
"""

import random

import numpy as np
import pytest

from openr_amd import abi

pytestmark = pytest.mark.gpu

INF = 0xFFFFFFFF
WINNER, TIE_WINNER, TIE, TIE_LOOSER, LOOSER, ERROR = range(6)
V = 48
MAIN, ISLAND, ISOLATED = range(0, 41), range(41, 47), 47
N_SELECTED, N_PLAIN = 300, 20  # 300 selected columns: lanes wrap past one 256-lane pass


def _network(seed):
    rng = random.Random(seed)
    links = []
    for part in (MAIN, ISLAND):
        part = list(part)
        for k in range(1, len(part)):  # a random tree, then chords
            links.append((part[rng.randrange(k)], part[k]))
        for _ in range(len(part)):
            u, v = rng.sample(part, 2)
            links.append((u, v))
    links = [(u, v, rng.randint(1, 9), rng.randint(1, 9)) for u, v in links]
    drained = np.zeros(V, dtype=np.uint8)
    for v in rng.sample(range(V), 9):
        drained[v] = 1
    return links, drained


def _code(rng):
    # all six results; TIE / ERROR rare enough that long folds still end in routes
    return rng.choices(range(6), weights=[20, 20, 3, 27, 27, 3])[0]


def _columns(seed):
    """announcers per column, {selected column: (pair codes, loopback flags)}"""
    rng = random.Random(seed)
    P = N_SELECTED + N_PLAIN
    selected_cols = set(rng.sample(range(P), N_SELECTED))
    announcers, selected = [], {}
    for p in range(P):
        if p not in selected_cols:
            announcers.append(rng.sample(range(V), rng.randint(1, 4)))
            continue
        n = rng.choice([1, 2, 3, 7, 32])
        cands = rng.sample(range(V), n)
        pair = [_code(rng) | (_code(rng) << 3) | (_code(rng) << 6) for _ in range(n * (n - 1) // 2)]
        flags = [1 if rng.random() < 0.85 else 0 for _ in range(n)]
        announcers.append(cands)
        selected[p] = (pair, flags)
    return announcers, selected


def _fold(d, s, cands, pair, flags, drained):
    """(winners, best, igp, metric) of one cell, the header's rule."""
    none = (0, INF, INF, INF)
    best, mask, igp = None, 0, INF
    for i, c in enumerate(cands):
        if d[c] >= INF:
            continue
        igp = min(igp, int(d[c]))
        code = WINNER
        if best is not None:
            db = d[cands[best]]
            shift = 0 if d[c] < db else 3 if d[c] == db else 6
            code = (pair[i * (i - 1) // 2 + best] >> shift) & 7
        if code in (TIE, ERROR):
            return none
        if code == WINNER:
            mask = 0
        if code <= TIE_WINNER:
            best = i
        if code <= TIE_LOOSER:
            mask |= 1 << i
    undrained = sum(1 << i for i in range(len(cands)) if (mask >> i) & 1 and not drained[cands[i]])
    filt = undrained or mask
    members = [cands[i] for i in range(len(cands)) if (filt >> i) & 1]
    if not filt or s in members or not flags[best]:
        return none
    return filt, cands[best], igp, min(int(d[c]) for c in members)


@pytest.fixture(scope="module")
def net(gpu_ready):
    links, drained = _network(77)
    csr = abi.Csr.from_links(V, links, drained)
    g = abi.Graph(csr)
    q = g.query(np.arange(V, dtype=np.uint32), abi.SPF_F_NEXTHOPS).run()
    dist = [q.dist(i) for i in range(V)]
    # the shape the cases rely on: an island and an isolated node out of reach
    assert dist[0][ISLAND[0]] >= INF and dist[0][ISOLATED] >= INF and dist[ISLAND[0]][ISLAND[1]] < INF
    yield g, q, dist, drained
    q.close()
    g.close()


@pytest.mark.parametrize("lfa", [False, True])
def test_selected_cells_equal_python_fold(net, lfa):
    g, q, dist, drained = net
    announcers, selected = _columns(5)
    flags = abi.SPF_RT_LFA if lfa else 0
    t = abi.RouteTable(q, announcers, flags, selected=selected).run()
    plain = abi.RouteTable(q, announcers, flags).run()
    routes_by_n, codes_hit = {}, set()
    for pair, _ in selected.values():
        for e in pair:
            codes_hit.update(((e >> 0) & 7, (e >> 3) & 7, (e >> 6) & 7))
    assert codes_hit == set(range(6))
    for s in range(V):
        metric, best, links, igp, winners = t.fetch_sel(s)
        pm, pb, pl = plain.fetch(s)
        m2, b2, l2 = t.fetch(s)  # the plain call on a table with selected columns
        assert (m2 == metric).all() and (b2 == best).all() and (l2 == links).all()
        for p, cands in enumerate(announcers):
            if p not in selected:
                # an unselected column beside selected ones: the plain table's cell
                assert (metric[p], best[p]) == (pm[p], pb[p]) and (links[p] == pl[p]).all()
                assert (igp[p], winners[p]) == (INF, 0)
                continue
            want = _fold(dist[s], s, cands, *selected[p], drained)
            got = (int(winners[p]), int(best[p]), int(igp[p]), int(metric[p]))
            assert got == want, (s, p, cands, got, want)
            if want[0]:
                routes_by_n[len(cands)] = routes_by_n.get(len(cands), 0) + 1
                assert links[p].any()  # a route has next hops
            else:
                assert not links[p].any()
    # every candidate count produced routes (the test is not all no-route cells)
    assert set(routes_by_n) == {1, 2, 3, 7, 32}, routes_by_n
    assert t.select_ms() > 0 and plain.select_ms() == 0
    t.close()
    plain.close()


def test_single_winner_cell_equals_plain_column(net):
    """A selected column whose pair codes make candidate 0 beat everyone
    (LOOSER for every later candidate) is, at rows that reach candidate 0, the
    plain column announced by candidate 0 alone: same metric and link mask."""
    g, q, dist, drained = net
    cands = [3, 17, 29, 40]
    pair = [LOOSER | (LOOSER << 3) | (LOOSER << 6)] * 6
    t = abi.RouteTable(q, [cands], 0, selected={0: (pair, [1, 1, 1, 1])}).run()
    plain = abi.RouteTable(q, [[3]]).run()
    for s in MAIN:
        metric, best, links, igp, winners = t.fetch_sel(s)
        pm, pb, pl = plain.fetch(s)
        if s == 3:
            assert metric[0] == INF and winners[0] == 0
            continue
        assert (metric[0], best[0], winners[0]) == (pm[0], 3, 1) and (links[0] == pl[0]).all()
        assert igp[0] == min(int(dist[s][c]) for c in cands)  # losers count too
    t.close()
    plain.close()


@pytest.mark.parametrize("lfa", [False, True])
def test_no_selected_columns_rows_byte_identical(net, lfa):
    g, q, dist, drained = net
    announcers, _ = _columns(9)
    flags = abi.SPF_RT_LFA if lfa else 0
    a = abi.RouteTable(q, announcers, flags).run()
    b = abi.RouteTable(q, announcers, flags, selected={}).run()  # create_sel, nothing selected
    for s in range(V):
        m, bst, l = a.fetch(s)
        for tab in (a, b):
            m2, b2, l2, igp, winners = tab.fetch_sel(s)
            assert m.tobytes() == m2.tobytes() and bst.tobytes() == b2.tobytes()
            assert l.tobytes() == l2.tobytes()
            assert (igp == INF).all() and (winners == 0).all()
    a.close()
    b.close()


def test_create_sel_rejects_bad_descriptors(net):
    g, q, dist, drained = net
    with pytest.raises(Exception):  # 33 candidates in a selected column
        abi.RouteTable(q, [list(range(33))], 0, selected={0: ([0] * (33 * 16), [1] * 33)})
    with pytest.raises(Exception):  # pair table shorter than n(n-1)/2
        abi.RouteTable(q, [[1, 2, 3]], 0, selected={0: ([0, 0], [1, 1, 1])})
    with pytest.raises(Exception):  # column out of range
        abi.RouteTable(q, [[1, 2]], 0, selected={5: ([0], [1, 1])})
