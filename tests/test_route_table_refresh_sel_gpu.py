"""spf_route_table_refresh_rows_sel straight through the C ABI (ctypes): a
topology change that keeps the CSR layout under a resident route table WITH
selected (BGP) columns.  spf_route_refresh_kernel<true> folds the resident
candidates of every selected column again over the new distance rows and the
current transit bits, recomputes every cell of the listed rows and swaps it
with the cell it replaces; spf_route_table_fetch_cells_prev_igp reads the igp
words it replaced.

Ground truth, as in test_route_table_refresh_gpu.py and
test_route_table_patch_sel_gpu.py.  Cells and selection words: a fresh
create_sel table over the new query with the same lists, pair tables and
flags, compared exactly in every row (unlisted rows keep their cells), igp and
winners through fetch_sel.  Bitmap and counts: fresh_after.diff(fresh_before),
and the numpy cell rule with the igp clause on whole-row snapshots.  Pack,
delta_fetch_igp, fetch_cells, fetch_cells_igp: built from the bitmap and the
rows.  fetch_cells_prev and _prev_igp: the snapshot taken before.
"""

import ctypes as C
import random

import numpy as np
import pytest

from openr_amd import abi
from tests.test_route_table_patch_gpu import (DRAINED, MIXED_V, check_after_patch, mixed_links,
                                              same, seeded_lists, snapshot)
from tests.test_route_table_patch_sel_gpu import (ERROR, LOOSER, TIE, TIE_LOOSER, WINNER,
                                                  check_igp_lanes, ring40_links, same_sel,
                                                  seeded_codes, snapshot_sel, uniform)
from tests.test_route_table_refresh_gpu import (TNet, bitmaps, check_prev, hub_links, mixed_ann,
                                                rule_bits, snapshot_row)

pytestmark = pytest.mark.gpu

INF = 0xFFFFFFFF
SPF_E_INVALID, SPF_E_UNSUPPORTED = -1, -4
# two candidates, the closer one wins: c1 against the best so far by d1 <, ==, > d_best
CLOSER = [WINNER | (TIE_LOOSER << 3) | (LOOSER << 6)]

# the selected columns of the mixed net (ring 0..9 with the chord 0 - 5, 3 and 7
# drained, the island 10 - 11, node 12 alone) and what the events below do there
C_CLOSER, C_LOSER, C_BOTH = 63, 64, 65  # [1, 6] closer wins; [1, 6] 6 always loses; [6, 1] both win
C_SELF, C_TIE, C_ERR = 3, 10, 11        # [3, 6] both win; [8, 2] TIE; [8, 2] ERROR
C_NONE, C_ONE, C_NOLB = 7, 8, 9         # no candidate; [5]; [2, 9] whose best 2 has no loopback


def sel_ann(P, seed):
    """mixed_ann with the selected columns above; returns (ann, selected)."""
    ann = mixed_ann(P, seed)
    sel = {}
    for c, cands, codes, flags in (
            (C_CLOSER, [1, 6], CLOSER, [1, 1]),
            (C_LOSER, [1, 6], uniform(2, LOOSER), [1, 1]),
            (C_BOTH, [6, 1], uniform(2, TIE_LOOSER), [1, 1]),
            (C_SELF, [3, 6], uniform(2, TIE_LOOSER), [1, 1]),
            (C_TIE, [8, 2], uniform(2, TIE), [1, 1]),
            (C_ERR, [8, 2], uniform(2, ERROR), [1, 1]),
            (C_NONE, [], [], []),
            (C_ONE, [5], [], [1]),
            (C_NOLB, [2, 9], uniform(2, LOOSER), [0, 1])):
        ann[c] = cands
        sel[c] = (codes, flags)
    return ann, sel


def rule_bits_sel(before, after, routes_only=False, rows=None):
    """rule_bits plus the igp clause: a cell with a route on both sides whose
    igp word differs is changed (snapshot_sel pairs)."""
    bits = rule_bits(before[0], after[0], routes_only, rows)
    for i, ((oi, _), (ni, _)) in enumerate(zip(before[1], after[1])):
        if rows is not None and i not in rows:
            continue
        routed = (before[0][i][0] != INF) & (after[0][i][0] != INF)
        bits[i] |= routed & (oi != ni)
    return bits


def check_prev_igp(net, t, words):
    """fetch_cells_prev_igp of every (row, column) against the words before."""
    rr = np.repeat(np.arange(net.V), t.P)
    cc = np.tile(np.arange(t.P), net.V)
    assert t.fetch_cells_prev_igp(rr, cc).tolist() == np.concatenate([w[0] for w in words]).tolist()


def check_refresh_sel(net, ann, sel, lfa, screened=False, routes_only=False, t=None, apply=None,
                      rerun=True, **event):
    """`t` (or a fresh table of (ann, sel)) follows `event` (TNet.change; or
    apply(net) -> listed rows) by refresh_rows_sel over a new query; every
    ground truth of the module docstring.  With `rerun` the table then diffs
    against the fresh one (which replaces its bitmap) and runs (which ends the
    previous cells).  Returns (table, counts, bits, snapshot_sel before,
    snapshot_sel after, listed rows)."""
    t = t or net.table(ann, lfa, selected=sel)
    older = net.table(ann, lfa, selected=sel)
    if routes_only:
        t.diff_routes(True)
    before = snapshot_sel(net, t)
    assert same_sel(before, snapshot_sel(net, older))
    q_old = net.q
    if apply:
        rows = apply(net)
    else:
        rows = net.change(screen=q_old if screened else None, lfa=lfa, **event)
    net.q = net.query()
    counts = t.refresh_rows_sel(net.q, rows)
    assert t.refresh_ms() >= 0.0
    after = snapshot_sel(net, t)
    fresh = net.table(ann, lfa, selected=sel)
    if routes_only:
        fresh.diff_routes(True)
    assert same_sel(after, snapshot_sel(net, fresh))
    want_counts = fresh.diff(older)
    bits = bitmaps(net, fresh)
    assert np.array_equal(bits, rule_bits_sel(before, after, routes_only))
    assert counts.tolist() == want_counts.tolist() == bits.sum(axis=1).tolist()
    if rows is not None:
        assert not bits[[i for i in range(net.V) if i not in rows]].any()
    pk = check_after_patch(net, t, after[0], bits)
    check_igp_lanes(net, t, pk, bits, after[1])
    check_prev(net, t, before[0])
    check_prev_igp(net, t, before[1])
    # every cell and igp word against the fresh table, both ways
    assert not fresh.diff(t).any()
    if rerun:
        assert not t.diff(fresh).any()
    for x in (older, fresh):
        net.objs.remove(x)
        x.close()
    # the binding moved: the old query goes, the new one stays while t lives
    assert abi.load().spf_query_destroy(q_old.h) == abi.SPF_OK
    q_old.h = None
    assert abi.load().spf_query_destroy(net.q.h) == SPF_E_INVALID
    if rerun:
        assert same_sel(snapshot_sel(net, t.run()), after)
    return t, counts, bits, before, after, rows


def mixed_net():
    return TNet(MIXED_V, mixed_links(), DRAINED)


EVENTS = {
    # 5 -> 6 from 4 to 1: node 3 is then nearer to 6 (6) than to 1 (7)
    "flip": dict(metrics={5: (1, 3)}),
    # 5 -> 6 from 4 to 3: 6 comes closer to 4 and 5 and still loses to 1
    "igp_alone": dict(metrics={5: (3, 3)}),
    "drain_a_winner": dict(drain=[6]),
    "undrain_the_rows_own_node": dict(undrain=[3]),
    "raise_tight": dict(metrics={0: (9, 9)}),
    "metric_and_drain": dict(metrics={8: (1, 6)}, drain=[9]),
}


def popcount(x):
    return bin(int(x)).count("1")


@pytest.mark.parametrize("screened", [False, True])
@pytest.mark.parametrize("lfa,routes_only", [(False, False), (True, False), (True, True)])
@pytest.mark.parametrize("event", sorted(EVENTS))
def test_events(gpu_ready, event, lfa, routes_only, screened):
    net = mixed_net()
    try:
        ann, sel = sel_ann(70, 7)
        _, counts, bits, before, after, rows = check_refresh_sel(
            net, ann, sel, lfa, screened, routes_only, **EVENTS[event])
        assert counts.sum() > 0
        (b_rows, b_words), (a_rows, a_words) = before, after
        if event == "flip":
            # the sign of d(3, 6) - d(3, 1) flipped: winners and best move from 1 to 6
            assert (b_words[3][1][C_CLOSER], b_rows[3][1][C_CLOSER]) == (0b01, 1)
            assert (a_words[3][1][C_CLOSER], a_rows[3][1][C_CLOSER]) == (0b10, 6)
            assert bits[3, C_CLOSER]
        if event == "igp_alone":
            for i in (4, 5):
                # metric, best, links, link metrics of the cell stayed
                assert all(np.array_equal(x[C_LOSER], y[C_LOSER])
                           for x, y in zip(b_rows[i], a_rows[i]) if x is not None)
                assert b_words[i][1][C_LOSER] == a_words[i][1][C_LOSER] == 0b01
                assert a_words[i][0][C_LOSER] == b_words[i][0][C_LOSER] - 1
                assert bits[i, C_LOSER]
        if event == "drain_a_winner":
            assert rows is None  # a transit bit flipped: every row
            # the drained winner leaves the winners word; best is not chosen again
            # (the winners word is no cell word: at 0, nearer to 1 anyway, the shortest-path
            # cell stays; at 5, next to 6, the route turns to 1)
            for i in (0, 5):
                assert (b_words[i][1][C_BOTH], b_rows[i][1][C_BOTH]) == (0b11, 6)
                assert (a_words[i][1][C_BOTH], a_rows[i][1][C_BOTH]) == (0b10, 6)
            assert (lfa or not bits[0, C_BOTH]) and bits[5, C_BOTH]
            assert (b_rows[5][0][C_BOTH], a_rows[5][0][C_BOTH]) == (4, 6)
        if event == "undrain_the_rows_own_node":
            # 3 was filtered out beside the undrained 6; now it is a winner of its own row
            assert b_words[3][1][C_SELF] == 0b10 and b_rows[3][0][C_SELF] != INF
            assert a_words[3][1][C_SELF] == 0 and a_rows[3][0][C_SELF] == INF
            assert a_words[3][0][C_SELF] == INF and bits[3, C_SELF]
        # 0, 1 and 2 candidates: no route without a candidate, and none where the best has no loopback
        d = [net.q.dist(i) for i in range(MIXED_V)]  # (64-bit: unreached is INF or above)
        assert all(r[0][C_NONE] == INF for r in a_rows)
        assert [bool(r[0][C_ONE] != INF) for r in a_rows] == [i != 5 and int(d[i][5]) < INF
                                                               for i in range(MIXED_V)]
        assert all(a_rows[i][0][C_NOLB] == INF for i in range(MIXED_V) if int(d[i][2]) < INF)
    finally:
        net.close()


@pytest.mark.parametrize("screened", [False, True])
@pytest.mark.parametrize("lfa", [False, True])
@pytest.mark.parametrize("P", [70, 130])
def test_selected_columns_at_word_edges_and_lanes_past_P(gpu_ready, P, lfa, screened):
    net = mixed_net()
    try:
        ann, sel = sel_ann(P, P)
        _, _, bits, _, _, _ = check_refresh_sel(net, ann, sel, lfa, screened, **EVENTS["flip"])
        assert all(bits[:, c].any() for c in (C_CLOSER, C_LOSER, C_BOTH))
        assert bits[:, [c for c in range(P) if c not in sel]].any()
    finally:
        net.close()


@pytest.mark.parametrize("lfa", [False, True])
def test_thirty_two_candidates(gpu_ready, lfa):
    net = TNet(40, ring40_links(), (4, 9, 22))
    try:
        rng = random.Random(32)
        ann = [[3, 7], rng.sample(range(40), 32), [1], rng.sample(range(40), 32)]
        sel = {0: (uniform(2, TIE_LOOSER), [1, 1]),
               1: (seeded_codes(32, rng, (30, 30, 1, 30, 30, 1)),
                   [1 if rng.random() < 0.9 else 0 for _ in range(32)]),
               3: (uniform(32, TIE_LOOSER), [1] * 32)}
        t, _, bits, _, after, _ = check_refresh_sel(
            net, ann, sel, lfa, True, metrics={0: (7, 7), 17: (9, 1), 40: (1, 1)})
        assert bits[:, 1].any() and bits[:, 3].any()
        assert any(popcount(w[1][3]) >= 29 for w in after[1])  # all but the drained ones win
        check_refresh_sel(net, ann, sel, lfa, t=t, drain=[30], undrain=[9])
    finally:
        net.close()


def halves(net, link):
    """The two half-edges of link `link` of a TNet."""
    e = np.flatnonzero(net.csr.link_id == link)
    assert len(e) == 2
    return [int(e[0]), int(e[1])]


@pytest.mark.parametrize("lfa", [False, True])
def test_set_edges_takes_the_only_link_to_a_candidate_down_and_back(gpu_ready, lfa):
    """7 is drained, so 8 - 9 is the only way to 8 for every row but 7 and 8.
    With it down the fold skips candidate 8: the columns [8, 2] under TIE and
    under ERROR get a route to 2; with it back they lose it again."""
    net = mixed_net()
    try:
        ann, sel = sel_ann(70, 5)
        u, v, a, b = net.links[8]
        assert (u, v) == (8, 9)

        def set_link(up):
            def apply(net):
                e = halves(net, 8)
                m = [a, b] if net.csr.col[e[0]] == v else [b, a]
                net.g.set_edges(e, [up, up], m)
                return None  # every row
            return apply

        t, _, bits, before, after, _ = check_refresh_sel(net, ann, sel, lfa, apply=set_link(0))
        for c in (C_TIE, C_ERR):
            assert all(r[0][c] == INF for r in before[0])
            routed = [i for i in range(MIXED_V) if after[0][i][0][c] != INF]
            assert routed == [0, 1, 3, 4, 5, 6, 9] and bits[routed, c].all()
            assert all(after[1][i][1][c] == 0b10 and after[0][i][1][c] == 2 for i in routed)
        assert after[0][8][0][C_CLOSER] == INF and bits[8, C_CLOSER]  # 8 is cut off
        _, _, bits, before, after, _ = check_refresh_sel(net, ann, sel, lfa, t=t, apply=set_link(1))
        for c in (C_TIE, C_ERR):
            assert all(r[0][c] == INF for r in after[0]) and bits[:, c].sum() == 7
        assert after[0][8][0][C_CLOSER] != INF
    finally:
        net.close()


def test_hub_row_one_past_the_stage(gpu_ready):
    """1,030 links at the hub: the unstaged path of the cell under a winners word."""
    net = TNet(1031, hub_links(1030))
    try:
        assert net.degs[0] == 1030
        ann = seeded_lists(65, 1031, 4)
        ann[0], ann[63], ann[64] = [17], [17, 900], [900, 17, 5]
        sel = {63: (CLOSER, [1, 1]), 64: (uniform(3, TIE_LOOSER), [1, 1, 1])}
        t = net.table(ann, False, selected=sel)
        older = net.table(ann, False, selected=sel)
        rows_of = lambda tab: [(snapshot_row(net, tab, i), [np.array(x) for x in tab.fetch_sel(i)[3:]])
                               for i in (0, 17, 18, 900, 1030)]
        before = rows_of(t)
        net.change(metrics={16: (40, 3)})  # the link 0 - 17
        q_old, net.q = net.q, net.query()
        counts = t.refresh_rows_sel(net.q)
        fresh = net.table(ann, False, selected=sel)
        assert counts.tolist() == fresh.diff(older).tolist()
        older.close()
        net.objs.remove(older)
        now, want = rows_of(t), rows_of(fresh)
        for (r1, w1), (r2, w2) in zip(now, want):
            assert same([r1], [r2]) and all(np.array_equal(x, y) for x, y in zip(w1, w2))
        # at the hub 17 was the closer one (2 + 16 % 3 = 3 against 2 + 899 % 3 = 4), now 900 is
        assert (before[0][1][1][63], before[0][0][1][63]) == (0b01, 17)
        assert (now[0][1][1][63], now[0][0][1][63]) == (0b10, 900)
        assert counts[0] >= 2 and counts.sum() > counts[0]
        assert not t.diff(fresh).any() and not fresh.diff(t).any()  # every cell, every igp word
        assert abi.load().spf_query_destroy(q_old.h) == abi.SPF_OK
        q_old.h = None
    finally:
        net.close()


def test_lfa_hub_of_300_spokes_is_refused_at_creation_as_before(gpu_ready):
    net = TNet(301, hub_links(300))
    try:
        with pytest.raises(abi.SpfError):
            abi.RouteTable(net.q, [[5, 9]], abi.SPF_RT_LFA, {0: (CLOSER, [1, 1])})
    finally:
        net.close()


@pytest.mark.parametrize("lfa", [False, True])
def test_refresh_patch_refresh_refresh(gpu_ready, lfa):
    """refresh, then patch_columns_sel; then a refresh that must fold with the
    PATCHED pair tables and lists; then another one, whose store and previous
    igp words are its own and which stales an earlier pack."""
    net = mixed_net()
    try:
        ann, sel = sel_ann(70, 1)
        t, _, _, _, _, _ = check_refresh_sel(net, ann, sel, lfa, rerun=False, **EVENTS["raise_tight"])
        # the patch: C_LOSER gets the closer-wins table, C_ONE a second candidate, an unselected column moves
        cols, lists = [C_LOSER, C_ONE, 40], [[1, 6], [5, 9], [2, 8]]
        psel = {C_LOSER: (CLOSER, [1, 1]), C_ONE: (uniform(2, TIE_LOOSER), [1, 1])}
        mid = snapshot_sel(net, t)
        counts = t.patch_columns_sel(cols, lists, psel)
        for c, l in zip(cols, lists):
            ann[c] = l
        sel.update(psel)
        fresh = net.table(ann, lfa, selected=sel)
        after = snapshot_sel(net, t)
        assert same_sel(after, snapshot_sel(net, fresh)) and counts.any()
        net.objs.remove(fresh)
        fresh.close()
        assert not same_sel(mid, after)
        # the patch ended the refresh's previous cells
        with pytest.raises(abi.SpfError):
            t.fetch_cells_prev_igp([0], [C_LOSER])
        with pytest.raises(abi.SpfError):
            t.fetch_cells_prev([0], [C_LOSER], net.degs)
        # the flip now moves C_LOSER as well: only the patched pair table lets 6 win at 3
        _, _, bits, before, now, _ = check_refresh_sel(net, ann, sel, lfa, True, t=t, rerun=False,
                                                       **EVENTS["flip"])
        assert (before[1][3][1][C_LOSER], now[1][3][1][C_LOSER]) == (0b01, 0b10)
        assert bits[3, C_LOSER] and bits[3, C_CLOSER]
        z = abi._RouteDeltaSizes()
        assert abi.load().spf_route_table_delta_pack(t.h, C.byref(z)) == abi.SPF_OK
        assert z.cells == bits.sum() > 0
        # a second refresh in a row (check_refresh_sel compares its store with ITS snapshot before)
        check_refresh_sel(net, ann, sel, lfa, t=t, **EVENTS["drain_a_winner"])
        with pytest.raises(abi.SpfError):
            t.delta_fetch(z)
        # ... whose run() ended its previous cells in turn
        with pytest.raises(abi.SpfError):
            t.fetch_cells_prev_igp([0], [C_LOSER])
    finally:
        net.close()


@pytest.mark.parametrize("lfa", [False, True])
def test_no_change_rerun_and_refresh(gpu_ready, lfa):
    """The table's own query re-run: zero bits, cells and words untouched."""
    net = mixed_net()
    try:
        ann, sel = sel_ann(70, 3)
        t = net.table(ann, lfa, selected=sel)
        before = snapshot_sel(net, t)
        net.q.run()
        for rows in (None, [], [4, 12]):
            counts = t.refresh_rows_sel(net.q, rows)
            assert not counts.any() and same_sel(snapshot_sel(net, t), before)
            check_after_patch(net, t, before[0], np.zeros((net.V, 70), dtype=bool))
            check_prev(net, t, before[0])
            check_prev_igp(net, t, before[1])
    finally:
        net.close()


@pytest.mark.parametrize("lfa", [False, True])
def test_strict_subset_of_the_affected_rows(gpu_ready, lfa):
    """Listed rows equal the fresh table; unlisted rows keep cells AND words."""
    net = mixed_net()
    try:
        ann, sel = sel_ann(130, 11)
        t = net.table(ann, lfa, selected=sel)
        before = snapshot_sel(net, t)
        q_old = net.q
        affected = net.change(screen=q_old, lfa=lfa, **EVENTS["raise_tight"])
        assert len(affected) >= 3
        listed = affected[::2][::-1].copy()  # a strict subset, not ascending
        net.q = net.query()
        counts = t.refresh_rows_sel(net.q, listed)
        after = snapshot_sel(net, t)
        fresh = net.table(ann, lfa, selected=sel)
        want = snapshot_sel(net, fresh)
        for i in range(net.V):
            ref = want if i in listed else before
            assert same([after[0][i]], [ref[0][i]]), i
            assert all(np.array_equal(x, y) for x, y in zip(after[1][i], ref[1][i])), i
        bits = rule_bits_sel(before, after, rows=set(listed.tolist()))
        assert np.array_equal(bitmaps(net, t), bits) and bits.any()
        assert counts.tolist() == bits.sum(axis=1).tolist()
        check_prev(net, t, before[0])
        check_prev_igp(net, t, before[1])
    finally:
        net.close()


@pytest.mark.parametrize("lfa", [False, True])
def test_a_table_without_selected_columns_takes_the_plain_path(gpu_ready, lfa):
    """refresh_rows_sel == refresh_rows there: same cells, same bits; and no
    igp words to read."""
    nets = [mixed_net(), mixed_net()]
    try:
        ann = mixed_ann(70, 9)
        got = []
        for net, call in zip(nets, ("refresh_rows", "refresh_rows_sel")):
            t = net.table(ann, lfa)
            before = snapshot(net, t)
            rows = net.change(screen=net.q, lfa=lfa, **EVENTS["raise_tight"])
            q_old, net.q = net.q, net.query()
            counts = getattr(t, call)(net.q, rows)
            q_old.close()
            after = snapshot(net, t)
            assert counts.tolist() == rule_bits(before, after).sum(axis=1).tolist() and counts.any()
            check_prev(net, t, before)
            got.append((counts.tolist(), bitmaps(net, t), after, t))
        assert got[0][0] == got[1][0] and np.array_equal(got[0][1], got[1][1])
        assert same(got[0][2], got[1][2])
        out = np.zeros(1, dtype=np.uint32)
        p32 = lambda x: abi._p(x, C.c_uint32)
        assert abi.load().spf_route_table_fetch_cells_prev_igp(
            got[1][3].h, 1, p32(out), p32(out), p32(out)) == SPF_E_UNSUPPORTED
    finally:
        for net in nets:
            net.close()


@pytest.mark.parametrize("lfa", [False, True])
def test_rejected_inputs_leave_the_table_as_it_was(gpu_ready, lfa):
    lib = abi.load()
    V = MIXED_V
    net = mixed_net()
    other = mixed_net()
    try:
        ann, sel = sel_ann(70, 6)
        flags = abi.SPF_RT_LFA if lfa else 0
        q0 = net.q
        t = net.table(ann, lfa, selected=sel)
        out1 = np.zeros(1, dtype=np.uint32)
        p32 = lambda x: abi._p(x, C.c_uint32)
        prev_igp = lambda: lib.spf_route_table_fetch_cells_prev_igp(t.h, 1, p32(out1), p32(out1),
                                                                    p32(out1))
        assert prev_igp() == SPF_E_INVALID  # no refresh ran
        before = snapshot_sel(net, t)
        cols, lists = [2, C_ONE], [[1], [4, 8]]
        t.patch_columns_sel(cols, lists, {C_ONE: (uniform(2, TIE_LOOSER), [1, 1])})
        rows = snapshot_sel(net, t)
        bits = bitmaps(net, t)
        assert bits.any() and not same_sel(before, rows)
        pk = check_after_patch(net, t, rows[0], bits)
        z = abi._RouteDeltaSizes()
        assert lib.spf_route_table_delta_pack(t.h, C.byref(z)) == abi.SPF_OK

        def raw(tab, q, n, lst, fn=lib.spf_route_table_refresh_rows_sel):
            a = None if lst is None else np.asarray(lst if len(lst) else [0], dtype=np.uint32)
            out = np.zeros(V, dtype=np.uint32)
            return fn(tab.h if tab else None, q.h if q else None, n,
                      abi._p(a, C.c_uint32) if a is not None else None, abi._p(out, C.c_uint32))

        idle = abi.RouteTable(q0, ann, flags, sel)  # has not run
        net.objs.append(idle)
        unrun = net.g.query(net.src, abi.SPF_F_NEXTHOPS)
        fewer = net.g.query(net.src[:-1], abi.SPF_F_NEXTHOPS).run()
        swapped = net.g.query(net.src[::-1].copy(), abi.SPF_F_NEXTHOPS).run()
        no_nh = net.g.query(net.src, 0).run()
        unit = net.g.query(net.src, abi.SPF_F_NEXTHOPS | abi.SPF_F_UNIT_METRIC).run()
        ign = net.g.query(net.src, abi.SPF_F_NEXTHOPS, [[0]] + [[] for _ in range(V - 1)]).run()
        good = net.query()
        invalid = [
            lambda: raw(None, good, 0, None),
            lambda: raw(t, None, 0, None),
            lambda: raw(idle, good, 0, None),
            lambda: raw(t, unrun, 0, None),
            lambda: raw(t, other.q, 0, None),
            lambda: raw(t, fewer, 0, None),
            lambda: raw(t, swapped, 0, None),
            lambda: raw(t, no_nh, 0, None),
            lambda: raw(t, unit, 0, None),
            lambda: raw(t, ign, 0, None),
            lambda: raw(t, good, 1, [V]),
            lambda: raw(t, good, 3, [1, 4, 1]),
        ]

        def untouched(k):
            assert same_sel(snapshot_sel(net, t), rows), k
            assert np.array_equal(bitmaps(net, t), bits), k
            assert t.delta_fetch(z)["col"].tolist() == pk["col"].tolist(), k  # the pack is still good
            assert lib.spf_query_destroy(q0.h) == SPF_E_INVALID, k  # and so is the binding

        # the plain call still refuses the selected table
        assert raw(t, good, 0, None, lib.spf_route_table_refresh_rows) == SPF_E_UNSUPPORTED
        untouched("plain")
        for k, call in enumerate(invalid):
            assert call() == SPF_E_INVALID, k
            untouched(k)
        assert prev_igp() == SPF_E_INVALID  # still no refresh
        for q in (unrun, fewer, swapped, no_nh, unit, ign, good):
            assert lib.spf_query_destroy(q.h) == abi.SPF_OK
            q.h = None
        # 64-bit rows (a metric past 2^31 on the graph): SPF_E_UNSUPPORTED
        net.change(metrics={4: (3_000_000_000, 3)})
        wide = net.g.query(net.src, abi.SPF_F_NEXTHOPS).run()
        assert wide.device_rows()[1] == 8
        assert raw(t, wide, 0, None) == SPF_E_UNSUPPORTED
        untouched("wide")
        wide.close()
    finally:
        other.close()
        net.close()
