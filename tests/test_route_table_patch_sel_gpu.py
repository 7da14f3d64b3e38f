"""spf_route_table_patch_columns_sel straight through the C ABI (ctypes):
listed columns of a resident route table with selected (BGP) columns get new
candidate lists, pair tables and flags in place.

Two ground truths for every case.  Cells: a fresh create_sel table over the
same query with the patched lists, pair tables and flags -- cells and the
fetch_sel words (igp, winners) bit-equal, and again after run().  Bitmap:
diff_mapped(before_fresh, after_fresh) with identity maps and the same dirty
lists -- bitmap and counts equal.  Pack, delta_fetch_igp, fetch_cells and
fetch_cells_igp are built from the bitmap and the rows.
"""

import ctypes as C
import random

import numpy as np
import pytest

from openr_amd import abi
from tests import test_route_table_patch_gpu as base

pytestmark = pytest.mark.gpu

INF = base.INF
SPF_E_INVALID, SPF_E_UNSUPPORTED = -1, -4
NONE = abi.SPF_MAP_NONE
WINNER, TIE_WINNER, TIE, TIE_LOOSER, LOOSER, ERROR = range(6)
MIXED_V = base.MIXED_V


def uniform(n, code):
    """Pair table of n candidates with `code` in all three distance slots."""
    return [code | (code << 3) | (code << 6)] * (n * (n - 1) // 2)


def seeded_codes(n, rng, weights=(20, 20, 3, 27, 27, 3)):
    def one():
        return rng.choices(range(6), weights=weights)[0]
    return [one() | (one() << 3) | (one() << 6) for _ in range(n * (n - 1) // 2)]


def snapshot_sel(net, t):
    """base.snapshot plus per row (igp [P], winners [P])."""
    words = []
    for i in range(net.V):
        _, _, _, igp, winners = t.fetch_sel(i)
        words.append((np.array(igp), np.array(winners)))
    return base.snapshot(net, t), words


def same_sel(a, b):
    return base.same(a[0], b[0]) and all(
        np.array_equal(i1, i2) and np.array_equal(w1, w2) for (i1, w1), (i2, w2) in zip(a[1], b[1]))


def dirty_csr(P, cols, dirty):
    """The dirty lists of a patch as spf_route_diff_map arrays over all P columns."""
    by_col = {c: list(d) for c, d in zip(cols, dirty)}
    off, flat = [0], []
    for c in range(P):
        flat += by_col.get(c, [])
        off.append(len(flat))
    return np.asarray(off, np.uint32), np.asarray(flat if flat else [0], np.uint32)


def bitmap(net, t):
    return np.array([t.changed(i) for i in range(net.V)])


def check_igp_lanes(net, t, pk, bits, words):
    rr, col, igp = [], [], []
    for i in range(net.V):
        ch = np.flatnonzero(bits[i])
        rr += [i] * len(ch)
        col += ch.tolist()
        igp += words[i][0][ch].tolist()
    assert t.delta_fetch_igp(pk["cells"]).tolist() == igp
    assert t.fetch_cells_igp(rr, col).tolist() == igp


def patched(ann, sel, cols, lists, psel):
    ann2 = [list(a) for a in ann]
    for c, l in zip(cols, lists):
        ann2[c] = list(l)
    sel2 = dict(sel)
    sel2.update(psel)
    return ann2, sel2


def check_patch_sel(net, ann, sel, lfa, cols, lists, psel, dirty=None, routes_only=False, t=None):
    """Patch a table of (ann, sel) -- `t`, or a fresh one -- and compare with
    the two ground truths.  Returns (table, counts, bits, rows after, igp/winner words)."""
    t = t or net.table(ann, lfa, sel)
    older = net.table(ann, lfa, sel)
    ann2, sel2 = patched(ann, sel, cols, lists, psel)
    fresh = net.table(ann2, lfa, sel2)
    if routes_only:
        t.diff_routes(True)
        fresh.diff_routes(True)
    counts = t.patch_columns_sel(cols, lists, psel, dirty)
    after, want = snapshot_sel(net, t), snapshot_sel(net, fresh)
    assert same_sel(after, want)
    maps = {}
    if dirty is not None:
        maps["dirty_off"], maps["dirty_ann"] = dirty_csr(len(ann), cols, dirty)
    want_counts = fresh.diff_mapped(older, **maps)
    bits = bitmap(net, fresh)
    assert counts.tolist() == want_counts.tolist() == bits.sum(axis=1).tolist()
    assert not bits[:, [c for c in range(len(ann)) if c not in cols]].any()
    pk = base.check_after_patch(net, t, after[0], bits)
    if sel:
        check_igp_lanes(net, t, pk, bits, after[1])
    assert t.patch_ms() >= 0.0
    t.run()  # the resident announcer, flag and pair arrays were replaced too
    assert same_sel(snapshot_sel(net, t), want)
    return t, counts, bits, after[0], after[1]


@pytest.fixture(scope="module")
def mixed(gpu_ready):
    net = base.PNet(MIXED_V, base.mixed_links(), base.DRAINED)
    yield net
    net.close()


def ring40_links():
    ring = [(i, (i + 1) % 40, 1 + i % 4, 1 + (i * 3) % 5) for i in range(40)]
    return ring + [(0, 20, 3, 2), (5, 31, 2, 2), (11, 27, 4, 1), (16, 38, 1, 3)]


@pytest.fixture(scope="module")
def ring40(gpu_ready):
    net = base.PNet(40, ring40_links(), (4, 9, 22))
    yield net
    net.close()


def test_create_sel_accepts_an_empty_selected_column(mixed):
    """A spare selected column: selected at creation with no candidates."""
    t = mixed.table([[1], [], [2, 5]], False, {1: ([], []), 2: (uniform(2, TIE_LOOSER), [1, 1])})
    for i in range(MIXED_V):
        metric, best, links, igp, winners = t.fetch_sel(i)
        assert (metric[1], best[1], igp[1], winners[1]) == (INF, INF, INF, 0) and not links[1].any()


@pytest.mark.parametrize("lfa", [False, True])
@pytest.mark.parametrize("P", [63, 64, 65, 130])
def test_selected_columns_at_word_edges_beside_unselected_ones(mixed, P, lfa):
    rng = random.Random(P)
    ann = base.seeded_lists(P, MIXED_V, P)
    mid = {63: 62, 64: 62, 65: 63, 130: 64}[P]
    chosen = sorted({0, mid, P - 1})
    sel = {}
    for c in chosen:
        ann[c] = [1, 5, 8]
        sel[c] = (seeded_codes(3, rng, (1, 1, 0, 1, 1, 0)), [1, 1, 1])
    # unselected columns 1 and P - 3 share bitmap words with selected ones, in the same call
    new = {0: [6, 2, 9, 0], mid: [8, 5], P - 1: [2, 9], 1: [4, 6], P - 3: [0]}
    cols = [P - 1, 1, 0, P - 3, mid] if mid != P - 1 else [P - 1, 1, 0, P - 3]
    psel = {c: (seeded_codes(len(new[c]), rng, (1, 1, 0, 1, 1, 0)), [1] * len(new[c])) for c in chosen}
    _, counts, bits, _, _ = check_patch_sel(mixed, ann, sel, lfa, cols, [new[c] for c in cols], psel)
    assert all(bits[:, c].any() for c in cols)


@pytest.mark.parametrize("lfa,routes_only", [(False, False), (True, False), (True, True)])
def test_candidate_list_shapes(mixed, lfa, routes_only):
    """0 candidates (the column freed), a spare column filled, 1 and 2
    candidates, a list that changes its length before an unlisted selected
    column, which must select the same cells after run()."""
    ann = [[1, 5], [], [4, 8], [2, 6], [0, 9, 5], [1]]
    sel = {0: (uniform(2, TIE_LOOSER), [1, 1]), 1: ([], []), 2: (uniform(2, LOOSER), [1, 1]),
           3: (uniform(2, WINNER), [1, 1]), 4: (uniform(3, TIE_LOOSER), [1, 1, 1])}
    cols = [0, 1, 2, 3]
    lists = [[], [8, 2], [6], [2, 6, 9, 1]]
    psel = {0: ([], []), 1: (uniform(2, TIE_WINNER), [1, 1]), 2: ([], [1]),
            3: (uniform(4, TIE_LOOSER), [1] * 4)}
    _, _, bits, rows, words = check_patch_sel(mixed, ann, sel, lfa, cols, lists, psel, None,
                                              routes_only)
    assert bits[:, 0].sum() == 8 and bits[:, 1].sum() == 8  # ring rows but the candidates'
    assert all(r[0][0] == INF for r in rows) and any(r[0][4] != INF for r in rows)
    assert any(bin(int(w[1][3])).count("1") > 1 for w in words)  # ECMP over several winners


@pytest.mark.parametrize("lfa", [False, True])
def test_thirty_two_candidates(ring40, lfa):
    rng = random.Random(32)
    ann = [[3, 7], rng.sample(range(40), 32), [1], []]
    sel = {0: (uniform(2, TIE_LOOSER), [1, 1]), 1: (seeded_codes(32, rng), [1] * 32), 3: ([], [])}
    cands = [rng.sample(range(40), 32), rng.sample(range(40), 32)]
    flags = [[1 if rng.random() < 0.9 else 0 for _ in range(32)], [1] * 32]
    psel = {1: (seeded_codes(32, rng, (30, 30, 1, 30, 30, 1)), flags[0]),
            3: (uniform(32, TIE_LOOSER), flags[1])}
    _, _, bits, rows, words = check_patch_sel(ring40, ann, sel, lfa, [3, 1, 2], cands + [[6, 30]], psel)
    assert bits[:, 1].any() and bits[:, 3].any()
    assert any(bin(int(w[1][3])).count("1") >= 29 for w in words)  # all but the drained ones win


@pytest.mark.parametrize("lfa", [False, True])
def test_pair_codes_and_refusals(mixed, lfa):
    """Seeded codes with TIE and ERROR; candidates on the island (skipped by
    ring rows), drained (3, 7), the row's own node among the winners, a best
    candidate without loopback."""
    rng = random.Random(11)
    P = 40
    ann, sel = [], {}
    for p in range(P):
        n = rng.choice([1, 2, 3, 5, 8])
        ann.append(rng.sample(range(MIXED_V), n))
        sel[p] = (seeded_codes(n, rng), [1] * n)
    cols = list(range(0, P, 2)) + [1, 3]
    lists, psel = [], {}
    for c in cols:
        n = rng.choice([1, 2, 3, 5, 8])
        lists.append(rng.sample(range(MIXED_V), n))
        psel[c] = (seeded_codes(n, rng, (20, 20, 6, 27, 27, 6)),
                   [1 if rng.random() < 0.8 else 0 for _ in range(n)])
    # fixed shapes: every winner drained; a drained and an undrained winner; island and ring
    # candidates; the best (first reachable under LOOSER) without loopback
    lists[-1], psel[3] = [3, 7], (uniform(2, TIE_LOOSER), [1, 1])
    lists[-2], psel[1] = [3, 2, 10], (uniform(3, TIE_LOOSER), [1, 1, 1])
    lists[0], psel[0] = [5, 8], (uniform(2, LOOSER), [0, 1])
    lists[1], psel[2] = [2, 3], (uniform(2, TIE), [1, 1])
    _, _, bits, rows, words = check_patch_sel(mixed, ann, sel, lfa, cols, lists, psel)
    assert bits.any()
    # drained candidates alone still route; beside an undrained winner they are filtered out
    assert words[0][1][3] == 0b11 and words[0][1][1] == 0b010
    # the island rows take the island candidate, the ring rows skip it
    assert words[11][1][1] == 0b100 and rows[10][0][1] == INF  # (row 10 is the winner itself)
    assert all(r[0][0] == INF for r in rows[:10])  # best 5 has no loopback flag
    assert [r[0][2] != INF for r in rows[:10]] == [False] * 10  # TIE: no route
    assert rows[2][0][1] == INF and rows[4][0][1] != INF  # the row's own node among the winners


@pytest.mark.parametrize("lfa", [False, True])
def test_igp_alone_sets_the_bit(mixed, lfa):
    """Column 1 gains candidate 6, which loses to candidate 1 in all three
    slots: winners, best, metric and links stay, igp drops exactly in the rows
    nearer to 6 than to 1."""
    ann = [[2], [1], [4, 8]]
    sel = {1: ([], [1]), 2: (uniform(2, TIE_LOOSER), [1, 1])}
    d = [mixed.q.dist(i) for i in range(MIXED_V)]
    t = mixed.table(ann, lfa, sel)
    before = snapshot_sel(mixed, t)
    _, _, bits, rows, words = check_patch_sel(
        mixed, ann, sel, lfa, [1], [[1, 6]], {1: (uniform(2, LOOSER), [1, 1])}, t=t)
    assert base.same(before[0], rows)  # metric, best, links, link metrics: unchanged
    want = [bool(rows[i][0][1] != INF and d[i][6] < d[i][1]) for i in range(MIXED_V)]
    assert bits[:, 1].tolist() == want and 0 < sum(want) < sum(r[0][1] != INF for r in rows)
    for i in np.flatnonzero(want):
        assert words[i][0][1] == d[i][6] < before[1][i][0][1] == d[i][1]
        assert words[i][1][1] == before[1][i][1][1] == 1
    for i in np.flatnonzero(~np.array(want)):
        assert words[i][0][1] == before[1][i][0][1]


@pytest.mark.parametrize("lfa", [False, True])
def test_dirty_lists(mixed, lfa):
    ann = [[1, 4], [4, 8], [2, 6], [5, 9]]
    sel = {0: (uniform(2, LOOSER), [1, 1]), 1: (uniform(2, TIE_LOOSER), [1, 1])}
    psel = dict(sel)
    # the same lists and tables again: all clear
    t, counts, bits, _, _ = check_patch_sel(mixed, ann, sel, lfa, [0, 1, 2], ann[:3], psel)
    assert not counts.any() and not bits.any()
    # a dirty candidate with unchanged lists: bits exactly where best is that candidate
    _, _, bits, rows, _ = check_patch_sel(mixed, ann, sel, lfa, [0, 1, 2], ann[:3], psel,
                                          [[1], [8], []], t=t)
    want = [bool(r[0][0] != INF and r[1][0] == 1) for r in rows]
    assert bits[:, 0].tolist() == want and sum(want) == 9  # (LOOSER: best is the first, 1)
    assert bits[:, 1].tolist() == [bool(r[0][1] != INF and r[1][1] == 8) for r in rows]
    assert not bits[:, 2].any()
    # SPF_MAP_NONE in an unselected column: a best-only move sets no bit; without it, it does.
    # Column 3 [5, 9] -> [5, 9, 0]: rows whose nearest announcer stays 5 or 9 move best alone
    moved = check_patch_sel(mixed, ann, sel, lfa, [3], [[5, 9, 0]], {}, [[]])[2]
    quiet = check_patch_sel(mixed, ann, sel, lfa, [3], [[5, 9, 0]], {}, [[NONE]])[2]
    assert moved[:, 3].sum() > quiet[:, 3].sum() > 0
    # ... and on a table without any selected column
    quiet0 = check_patch_sel(mixed, ann, {}, lfa, [3, 0], [[5, 9, 0], [1]], {}, [[NONE], [1]])[2]
    assert quiet0[:, 3].tolist() == quiet[:, 3].tolist() and quiet0[:, 0].any()


@pytest.mark.parametrize("lfa", [False, True])
@pytest.mark.parametrize("spokes", [(44, 3), (75, 4)])
def test_hub_rows(gpu_ready, spokes, lfa):
    """Hub degree 132 (a wave's slice of LDS) and 300 (the one-row-per-workgroup shape)."""
    per, n = spokes
    net = base.PNet(13, base.hub_links(per, list(range(0, 12, 12 // n))[:n]), drained=(6,))
    try:
        ann = base.seeded_lists(66, 13, 2)
        ann[0], ann[65] = [3, 9], [6, 1]
        sel = {0: (uniform(2, TIE_LOOSER), [1, 1]), 65: (uniform(2, LOOSER), [1, 1])}
        psel = {0: (uniform(3, TIE_LOOSER), [1, 1, 1]), 65: (uniform(2, WINNER), [1, 1])}
        t, _, bits, _, _ = check_patch_sel(net, ann, sel, lfa, [0, 64, 65], [[5, 2, 6], [2], [6, 9]], psel)
        assert t.link_words(12) == (per * n + 63) // 64 >= 3 and bits[12, 0] and bits[12, 65]
    finally:
        net.close()


def test_hub_with_more_links_than_the_stage_holds(gpu_ready):
    """1040 links: the general path (non-LFA only)."""
    net = base.PNet(13, base.hub_links(130, [0, 1, 2, 3, 5, 7, 8, 10]))
    try:
        assert net.degs[12] == 1040
        ann = base.seeded_lists(10, 13, 4)
        ann[1] = [4, 6]
        sel = {1: (uniform(2, TIE_LOOSER), [1, 1])}
        _, _, bits, _, _ = check_patch_sel(net, ann, sel, False, [1, 9], [[9, 3, 6], [12]],
                                           {1: (uniform(3, TIE_LOOSER), [1, 1, 1])})
        assert bits[12, 1]
    finally:
        net.close()


@pytest.mark.parametrize("lfa", [False, True])
def test_more_than_256_listed_columns(mixed, lfa):
    rng = random.Random(300)
    P = 600
    ann = base.seeded_lists(P, MIXED_V, 12)
    sel = {}
    for c in range(0, P, 2):
        ann[c] = rng.sample(range(10), 3)
        sel[c] = (seeded_codes(3, rng), [1, 1, 1])
    cols = rng.sample(range(P), 560)  # more than 256 selected and more than 256 unselected ones
    lists, psel = [], {}
    for c in cols:
        n = rng.randint(0, 4)
        lists.append(rng.sample(range(MIXED_V), n))
        if c in sel:
            psel[c] = (seeded_codes(n, rng), [1] * n)
    assert len(psel) > 256 and len(cols) - len(psel) > 256
    _, counts, _, _, _ = check_patch_sel(mixed, ann, sel, lfa, cols, lists, psel)
    assert counts.sum() > len(cols)


@pytest.mark.parametrize("lfa", [False, True])
def test_second_patch_reports_its_own_bits_and_stales_the_pack(mixed, lfa):
    ann = base.seeded_lists(70, MIXED_V, 1)
    ann[1], ann[66] = [2, 5], [8]
    sel = {1: (uniform(2, TIE_LOOSER), [1, 1]), 66: ([], [1])}
    psel = {1: (uniform(1, WINNER), [1]), 66: (uniform(2, WINNER), [1, 1])}
    t, _, bits, _, _ = check_patch_sel(mixed, ann, sel, lfa, [1, 66], [[6], [8, 0]], psel)
    assert bits[:, [1, 66]].any()
    t.patch_columns_sel([1, 66], [[2, 5], [8]], sel)
    z = abi._RouteDeltaSizes()
    assert abi.load().spf_route_table_delta_pack(t.h, C.byref(z)) == abi.SPF_OK
    _, _, bits2, _, _ = check_patch_sel(mixed, ann, sel, lfa, [40], [[5, 9]], {}, t=t)
    with pytest.raises(abi.SpfError):
        t.delta_fetch(z)
    assert bits2[:, 40].any() and not bits2[:, [1, 66]].any()


def raw_sel(t, patch, sel):
    """patch = (k, cols, off, ann[, doff, dann]); sel = (n, cols, poff, codes, flags) or None."""
    keep = [np.asarray(x, dtype=np.uint32) if x is not None else None
            for x in (list(patch[1:]) + [None, None])[:5]]
    m = abi._RoutePatch(patch[0], *[abi._p(x, C.c_uint32) if x is not None else None for x in keep])
    d = None
    if sel is not None:
        types = (np.uint32, np.uint64, np.uint16, np.uint8)
        ctypes_ = (C.c_uint32, C.c_uint64, C.c_uint16, C.c_uint8)
        keep2 = [np.asarray(x, dtype=ty) if x is not None else None for x, ty in zip(sel[1:], types)]
        d = C.byref(abi._RouteSelectDesc(
            sel[0], *[abi._p(x, ct) if x is not None else None for x, ct in zip(keep2, ctypes_)]))
    out = np.zeros(t.n, dtype=np.uint32)
    return abi.load().spf_route_table_patch_columns_sel(t.h, C.byref(m), d, abi._p(out, C.c_uint32))


@pytest.mark.parametrize("lfa", [False, True])
def test_rejected_inputs_leave_the_table_as_it_was(mixed, lfa):
    lib = abi.load()
    V = MIXED_V
    ann = base.seeded_lists(70, V, 6)
    ann[3], ann[5] = [1, 8], [2]
    sel = {3: (uniform(2, TIE_LOOSER), [1, 1]), 5: ([], [1])}
    t0 = abi.RouteTable(mixed.q, ann, abi.SPF_RT_LFA if lfa else 0, sel)
    mixed.tables.append(t0)
    ok_sel = (1, [3], [0, 1], [0], [1, 1])
    assert raw_sel(t0, (1, [3], [0, 2], [1, 2]), ok_sel) == SPF_E_INVALID  # has not run
    t, _, bits, rows, words = check_patch_sel(
        mixed, ann, sel, lfa, [2, 3], [[1], [4, 8]], {3: (uniform(2, WINNER), [1, 1])})
    t.patch_columns_sel([2, 3], [ann[2], ann[3]], {3: sel[3]})  # (check_patch_sel ran the table)
    rows, words = snapshot_sel(mixed, t)
    bits = bitmap(mixed, t)
    assert bits.any()
    pk = base.check_after_patch(mixed, t, rows, bits)
    z = abi._RouteDeltaSizes()
    assert lib.spf_route_table_delta_pack(t.h, C.byref(z)) == abi.SPF_OK
    p2 = (1, [3], [0, 2], [1, 2])
    many = list(range(13)) * 3
    bad = [
        # the selection descriptor
        lambda: raw_sel(t, (2, [3, 2], [0, 2, 3], [1, 2, 4]), (1, [4], [0, 1], [0], [1, 1, 1])),  # not listed
        lambda: raw_sel(t, (2, [3, 2], [0, 2, 3], [1, 2, 4]), (2, [3, 2], [0, 1, 1], [0], [1, 1, 1])),  # not selected
        lambda: raw_sel(t, p2, None),                                     # a listed selected column missing
        lambda: raw_sel(t, p2, (0, None, None, None, None)),
        lambda: raw_sel(t, (2, [3, 5], [0, 2, 3], [1, 2, 4]), ok_sel),    # column 5 missing
        lambda: raw_sel(t, p2, (2, [3, 3], [0, 1, 2], [0, 0], [1, 1])),   # listed twice
        lambda: raw_sel(t, (1, [3], [0, 33], many[:33]), (1, [3], [0, 528], [0] * 528, [1] * 33)),  # 33 candidates
        lambda: raw_sel(t, p2, (1, [3], [0, 0], [0], [1, 1])),            # a short pair table
        lambda: raw_sel(t, p2, (1, [3], [1, 2], [0, 0], [1, 1])),         # pair_offsets[0] != 0
        lambda: raw_sel(t, (2, [3, 5], [0, 2, 3], [1, 2, 4]), (2, [3, 5], [0, 2, 1], [0, 0], [1, 1, 1])),  # decreasing
        lambda: raw_sel(t, p2, (1, None, [0, 1], [0], [1, 1])),           # null arrays
        lambda: raw_sel(t, p2, (1, [3], None, [0], [1, 1])),
        lambda: raw_sel(t, p2, (1, [3], [0, 1], None, [1, 1])),
        lambda: raw_sel(t, p2, (1, [3], [0, 1], [0], None)),
        lambda: raw_sel(t, (1, [3], [0, 2], [1, 2], [0, 1], [NONE]), ok_sel),  # NONE in a selected column
        # everything the old call rejects
        lambda: lib.spf_route_table_patch_columns_sel(t.h, None, None, None),
        lambda: lib.spf_route_table_patch_columns_sel(None, C.byref(abi._RoutePatch()), None, None),
        lambda: raw_sel(t, (1, None, [0, 1], [1]), None),
        lambda: raw_sel(t, (1, [0], None, [1]), None),
        lambda: raw_sel(t, (1, [0], [0, 1], None), None),
        lambda: raw_sel(t, (1, [0], [0, 0], [0], [0, 1], None), None),
        lambda: raw_sel(t, (1, [70], [0, 1], [1]), None),
        lambda: raw_sel(t, (2, [6, 6], [0, 1, 2], [1, 2]), None),
        lambda: raw_sel(t, (1, [0], [0, 1], [V]), None),
        lambda: raw_sel(t, (1, [0], [0, 1], [1], [0, 1], [V]), None),
        lambda: raw_sel(t, (1, [0], [1, 2], [1, 2]), None),
        lambda: raw_sel(t, (2, [0, 1], [0, 2, 1], [1, 2]), None),
        lambda: raw_sel(t, (1, [0], [0, 1], [1], [1, 2], [1, 2]), None),
        lambda: raw_sel(t, (2, [0, 1], [0, 1, 2], [1, 2], [0, 2, 1], [1, 2]), None),
    ]
    for k, call in enumerate(bad):
        assert call() == SPF_E_INVALID, k
        assert same_sel(snapshot_sel(mixed, t), (rows, words)), k
        assert np.array_equal(bitmap(mixed, t), bits), k
        assert t.delta_fetch(z)["col"].tolist() == pk["col"].tolist(), k  # the pack is still good
    # the old call keeps its refusals
    assert base.raw_patch(t, 1, [3], [0, 1], [1]) == SPF_E_UNSUPPORTED
    assert base.raw_patch(t, 1, [0], [0, 1], [1], [0, 1], [NONE]) == SPF_E_INVALID
    # sel NULL with no listed column selected: the old call's behaviour
    assert raw_sel(t, (1, [0], [0, 1], [1]), None) == abi.SPF_OK
