"""spf_route_table_patch_columns straight through the C ABI (ctypes): new
announcer lists for listed columns of a resident route table, recomputed in
place by spf_route_patch_kernel and compared with the cells they replace.

Ground truth.  Cells: a fresh RouteTable over the same query with the patched
lists, run by the existing kernel -- equality is exact, in every column.
Bitmap: a numpy comparison of whole-row fetches taken before and after the
patch with the cell rule of include/openr_spf.h (one side without a route; or
metric, best, link words or an LFA link metric differ; or the new best is a
dirty announcer), listed columns only.  Pack / fetch_cells: built from the
bitmap and the rows.
"""

import ctypes as C

import numpy as np
import pytest

from openr_amd import abi

pytestmark = pytest.mark.gpu

INF = 0xFFFFFFFF
SPF_E_INVALID, SPF_E_UNSUPPORTED = -1, -4


class PNet:
    """A graph given as links [(u, v, metric u->v, metric v->u)] and its
    all-sources query; tables over it on demand."""

    def __init__(self, V, links, drained=()):
        self.V = V
        ov = np.zeros(V, dtype=np.uint8)
        ov[list(drained)] = 1
        self.csr = abi.Csr.from_links(V, links, ov)
        self.degs = [0] * V
        for u, v, _, _ in links:
            self.degs[u] += 1
            self.degs[v] += 1
        self.g = abi.Graph(self.csr)
        self.q = self.g.query(np.arange(V, dtype=np.uint32), abi.SPF_F_NEXTHOPS).run()
        self.tables = []

    def table(self, ann, lfa, selected=None):
        t = abi.RouteTable(self.q, ann, abi.SPF_RT_LFA if lfa else 0, selected).run()
        self.tables.append(t)
        return t

    def close(self):
        for t in self.tables:
            t.close()
        self.q.close()
        self.g.close()


def snapshot(net, t):
    """Per row (metric [P], best [P], link words [P, W], link metrics [P, deg] or None)."""
    out = []
    for i in range(net.V):
        m, b, w = t.fetch(i)
        W = t.link_words(i)
        w = np.array(w[: t.P * W]).reshape(t.P, W)
        lm = np.array(t.fetch_link_metrics(i, net.degs[i])).reshape(t.P, net.degs[i]) if t.lfa else None
        out.append((np.array(m[: t.P]), np.array(b[: t.P]), w, lm))
    return out


def same(a, b):
    for (m1, b1, w1, l1), (m2, b2, w2, l2) in zip(a, b):
        if not (np.array_equal(m1, m2) and np.array_equal(b1, b2) and np.array_equal(w1, w2)):
            return False
        if l1 is not None and not np.array_equal(l1, l2):
            return False
    return True


def expected_bits(before, after, cols, dirty, routes_only):
    """[V, P] bool by the rule of spf_route_table_patch_columns."""
    P = len(before[0][0])
    out = np.zeros((len(before), P), dtype=bool)
    for i, ((om, ob, ow, ol), (nm, nb, nw, nl)) in enumerate(zip(before, after)):
        for k, c in enumerate(cols):
            if (om[c] == INF) != (nm[c] == INF):
                out[i, c] = True
            elif om[c] != INF:
                ch = (om[c] != nm[c] and not routes_only) or ob[c] != nb[c]
                ch = ch or not np.array_equal(ow[c], nw[c])
                ch = ch or (ol is not None and not np.array_equal(ol[c], nl[c]))
                ch = ch or (dirty is not None and int(nb[c]) in dirty[k])
                out[i, c] = ch
    return out


def check_after_patch(net, t, rows, bits):
    """changed / pack / fetch_cells of `t` against the bitmap `bits` and the
    rows `rows` (a snapshot of t)."""
    got_bits = np.array([t.changed(i) for i in range(net.V)])
    assert np.array_equal(got_bits, bits)
    assert not any(len(t.changed_gone(i)) for i in range(net.V))
    pk = t.delta_pack()
    cell_off = np.concatenate([[0], np.cumsum(bits.sum(axis=1))])
    assert pk["cell_off"].tolist() == cell_off.tolist() and pk["num_gone"] == 0
    assert not pk["gone_off"].any()
    col, metric, best, links, lmet, rr = [], [], [], [], [], []
    for i in range(net.V):
        ch = np.flatnonzero(bits[i])
        m, b, w, lm = rows[i]
        col += ch.tolist()
        rr += [i] * len(ch)
        metric += m[ch].tolist()
        best += b[ch].tolist()
        links += w[ch].reshape(-1).tolist()
        if lm is not None:
            lmet += lm[ch].reshape(-1).tolist()
    assert pk["col"].tolist() == col and pk["metric"].tolist() == metric
    assert pk["best"].tolist() == best and pk["links"].tolist() == links
    assert pk["link_metrics"].tolist() == lmet
    gm, gb, gl, glm = t.fetch_cells(rr, col, net.degs)
    assert gm.tolist() == metric and gb.tolist() == best and gl.tolist() == links
    assert glm.tolist() == lmet
    return pk


def check_patch(net, ann, lfa, cols, lists, dirty=None, routes_only=False):
    """Patch a fresh table of `ann`; compare with a fresh table of the patched
    lists and with the bitmap rule.  Returns (table, counts, bits)."""
    t = net.table(ann, lfa)
    if routes_only:
        t.diff_routes(True)
    before = snapshot(net, t)
    counts = t.patch_columns(cols, lists, dirty)
    after = snapshot(net, t)
    ann2 = [list(a) for a in ann]
    for c, l in zip(cols, lists):
        ann2[c] = list(l)
    want = snapshot(net, net.table(ann2, lfa))
    assert same(after, want)
    bits = expected_bits(before, after, cols, dirty, routes_only)
    assert counts.tolist() == bits.sum(axis=1).tolist()
    check_after_patch(net, t, after, bits)
    assert t.patch_ms() >= 0.0
    t.run()  # the resident announcer arrays were replaced too
    assert same(snapshot(net, t), want)
    return t, counts, bits


def mixed_links():
    """Ring 0..9 with a chord, the island 10 - 11, node 12 without links."""
    ring = [(i, (i + 1) % 10, 2 + i % 3, 2 + (i * 5) % 4) for i in range(10)]
    return ring + [(0, 5, 3, 4), (10, 11, 1, 1)]


MIXED_V = 13
DRAINED = (3, 7)


def seeded_lists(P, V, seed):
    rng = np.random.RandomState(seed)
    return [sorted(set(rng.randint(0, V, size=p % 4).tolist())) for p in range(P)]


@pytest.fixture(scope="module")
def mixed(gpu_ready):
    net = PNet(MIXED_V, mixed_links(), DRAINED)
    yield net
    net.close()


@pytest.mark.parametrize("lfa", [False, True])
@pytest.mark.parametrize("P", [63, 64, 65, 130])
def test_column_counts_and_word_edges(mixed, P, lfa):
    ann = seeded_lists(P, MIXED_V, P)
    cols = sorted({0, 63, 64, P - 1} & set(range(P)))
    lists = [sorted({(c + 1) % 10, (c + 4) % 10}) for c in cols]
    _, counts, bits = check_patch(mixed, ann, lfa, cols, lists)
    assert counts.sum() > 0
    assert not bits[:, [c for c in range(P) if c not in cols]].any()


@pytest.mark.parametrize("lfa", [False, True])
@pytest.mark.parametrize("cols", [[3, 40], [5, 70]])
def test_two_columns_in_one_bitmap_word_and_in_two(mixed, cols, lfa):
    ann = seeded_lists(100, MIXED_V, 3)
    _, _, bits = check_patch(mixed, ann, lfa, cols, [[1], [6, 2]])
    assert bits[:, cols[0]].any() and bits[:, cols[1]].any()


@pytest.mark.parametrize("lfa,routes_only", [(False, False), (True, False), (True, True)])
def test_list_shapes_self_island_and_drained(mixed, lfa, routes_only):
    """grow, shrink, becomes empty, was empty, same again, an island
    announcer, all announcers drained, some drained; every announcer's own
    row is the no-route (self) case.  Rows 10 and 11 reach only each other,
    row 12 (no links) nothing.  routes_only: spf_route_table_diff_routes
    (LFA tables only)."""
    ann = seeded_lists(65, MIXED_V, 7)
    base = {0: [1], 1: [1, 5, 8], 2: [4], 3: [], 12: [9], 10: [2], 63: [2], 64: [2], 20: [10]}
    new = {0: [1, 5], 1: [5], 2: [], 3: [6], 12: [9], 10: [11, 2], 63: [3, 7], 64: [3, 4], 20: [12]}
    for c, l in base.items():
        ann[c] = l
    cols = sorted(new)
    _, _, bits = check_patch(mixed, ann, lfa, cols, [new[c] for c in cols], None, routes_only)
    assert not bits[:, 12].any()          # the same list again
    assert bits[:10, 2].sum() == 9        # every ring row but the announcer lost its route
    assert bits[10, 10] and bits[11, 20]  # island rows gain / lose their island routes


@pytest.mark.parametrize("lfa", [False, True])
def test_same_lists_again_change_nothing(mixed, lfa):
    ann = seeded_lists(70, MIXED_V, 9)
    cols = list(range(70))
    t, counts, bits = check_patch(mixed, ann, lfa, cols, ann)
    assert not counts.any() and not bits.any()
    assert t.run().patch_columns(cols, ann).sum() == 0 and t.delta_pack()["cells"] == 0


@pytest.mark.parametrize("lfa", [False, True])
def test_dirty_announcer_with_unchanged_list(mixed, lfa):
    ann = seeded_lists(66, MIXED_V, 5)
    ann[64], ann[65] = [1, 4], [4, 8]
    cols, lists, dirty = [64, 65, 2], [[1, 4], [4, 8], ann[2]], [[1], [8], []]
    t, _, bits = check_patch(mixed, ann, lfa, cols, lists, dirty)
    rows = snapshot(mixed, t)
    # best is the smallest reachable announcer: 1 for every ring row with a
    # route in column 64 (not rows 1 and 4, the announcers), never 8 in column 65
    want64 = [bool(r[0][64] != INF and r[1][64] == 1) for r in rows]
    assert bits[:, 64].tolist() == want64 and sum(want64) == 8
    assert not bits[:, 65].any() and not bits[:, 2].any()


def hub_links(spokes_per_node, nodes):
    """Ring of 12 + hub 12 with `spokes_per_node` parallel links to each of `nodes`."""
    ring = [(i, (i + 1) % 12, 3, 3) for i in range(12)]
    spokes = [(12, v, 2 + (j + v) % 3, 2 + (j * 7) % 4) for v in nodes for j in range(spokes_per_node)]
    return ring + spokes


@pytest.mark.parametrize("lfa", [False, True])
@pytest.mark.parametrize("spokes", [(44, 3), (75, 4)])
def test_hub_rows_with_three_link_words_and_beyond_a_wave_slice(gpu_ready, spokes, lfa):
    """Hub degree 132 (three link words, staged in a wave's slice of LDS) and
    300 (beyond the slice: the one-row-per-workgroup shape, which LFA cells
    need staged)."""
    per, n = spokes
    net = PNet(13, hub_links(per, list(range(0, 12, 12 // n))[:n]), drained=(6,))
    try:
        ann = seeded_lists(66, 13, 2)
        t, _, bits = check_patch(net, ann, lfa, [0, 64, 65], [[12, 5], [2], [6, 9]])
        assert t.link_words(12) == (per * n + 63) // 64 >= 3 and bits[12].any()
    finally:
        net.close()


def test_hub_with_more_links_than_the_stage_holds(gpu_ready):
    """1040 links: the general path (non-LFA only; LFA tables refuse the row)."""
    net = PNet(13, hub_links(130, [0, 1, 2, 3, 5, 7, 8, 10]))
    try:
        assert net.degs[12] == 1040
        ann = seeded_lists(10, 13, 4)
        _, _, bits = check_patch(net, ann, False, [1, 9], [[4, 6], [12]])
        assert bits[12].any()
    finally:
        net.close()


@pytest.mark.parametrize("lfa", [False, True])
@pytest.mark.parametrize("P,k", [(130, 65), (130, 130), (300, 257), (300, 300)])
def test_long_column_lists(mixed, P, k, lfa):
    """65 and 130 columns stride a wave's lanes; above 256 columns every row
    takes the 256-lane shape."""
    ann = seeded_lists(P, MIXED_V, P + k)
    cols = np.random.RandomState(k).permutation(P)[:k].tolist()
    lists = [sorted({(c * 3) % 12, (c + 5) % 11}) for c in cols]
    _, counts, _ = check_patch(mixed, ann, lfa, cols, lists)
    assert counts.sum() > k


@pytest.mark.parametrize("lfa", [False, True])
def test_second_patch_reports_its_own_bits_and_stales_the_pack(mixed, lfa):
    ann = seeded_lists(70, MIXED_V, 1)
    t = mixed.table(ann, lfa)
    assert t.patch_columns([1, 66], [[2], [8]]).sum() > 0
    assert np.array([t.changed(i) for i in range(MIXED_V)])[:, [1, 66]].any()
    z = abi._RouteDeltaSizes()
    assert abi.load().spf_route_table_delta_pack(t.h, C.byref(z)) == abi.SPF_OK
    before = snapshot(mixed, t)
    counts = t.patch_columns([40], [[5, 9]])
    with pytest.raises(abi.SpfError):
        t.delta_fetch(z)
    after = snapshot(mixed, t)
    bits2 = expected_bits(before, after, [40], None, False)
    assert counts.tolist() == bits2.sum(axis=1).tolist() and not bits2[:, [1, 66]].any()
    check_after_patch(mixed, t, after, bits2)
    # no columns: an all-clear bitmap
    assert not t.patch_columns([], []).any()
    check_after_patch(mixed, t, after, np.zeros_like(bits2))


def raw_patch(t, k, cols, off, ann, doff=None, dann=None):
    keep = [np.asarray(x, dtype=np.uint32) if x is not None else None
            for x in (cols, off, ann, doff, dann)]
    ptr = [abi._p(x, C.c_uint32) if x is not None else None for x in keep]
    m = abi._RoutePatch(k, *ptr)
    out = np.zeros(t.n, dtype=np.uint32)
    return abi.load().spf_route_table_patch_columns(t.h, C.byref(m), abi._p(out, C.c_uint32))


@pytest.mark.parametrize("lfa", [False, True])
def test_rejected_inputs_leave_the_table_as_it_was(mixed, lfa):
    lib = abi.load()
    ann = seeded_lists(70, MIXED_V, 6)
    V = MIXED_V
    t0 = abi.RouteTable(mixed.q, ann, abi.SPF_RT_LFA if lfa else 0)
    mixed.tables.append(t0)
    assert raw_patch(t0, 1, [0], [0, 1], [1]) == SPF_E_INVALID  # has not run
    t = mixed.table(ann, lfa)
    before = snapshot(mixed, t)
    t.patch_columns([2, 65], [[1], [4, 8]])
    rows = snapshot(mixed, t)
    bits = expected_bits(before, rows, [2, 65], None, False)
    pk = check_after_patch(mixed, t, rows, bits)
    assert bits.any()
    z = abi._RouteDeltaSizes()
    assert lib.spf_route_table_delta_pack(t.h, C.byref(z)) == abi.SPF_OK
    bad = [
        lambda: lib.spf_route_table_patch_columns(t.h, None, None),
        lambda: lib.spf_route_table_patch_columns(None, C.byref(abi._RoutePatch()), None),
        lambda: raw_patch(t, 1, None, [0, 1], [1]),
        lambda: raw_patch(t, 1, [0], None, [1]),
        lambda: raw_patch(t, 1, [0], [0, 1], None),
        lambda: raw_patch(t, 1, [0], [0, 0], [0], [0, 1], None),
        lambda: raw_patch(t, 1, [70], [0, 1], [1]),
        lambda: raw_patch(t, 2, [5, 5], [0, 1, 2], [1, 2]),
        lambda: raw_patch(t, 1, [0], [0, 1], [V]),
        lambda: raw_patch(t, 1, [0], [0, 1], [1], [0, 1], [V]),
        lambda: raw_patch(t, 1, [0], [0, 1], [1], [0, 1], [abi.SPF_MAP_NONE]),
        lambda: raw_patch(t, 1, [0], [1, 2], [1, 2]),
        lambda: raw_patch(t, 2, [0, 1], [0, 2, 1], [1, 2]),
        lambda: raw_patch(t, 1, [0], [0, 1], [1], [1, 2], [1, 2]),
        lambda: raw_patch(t, 2, [0, 1], [0, 1, 2], [1, 2], [0, 2, 1], [1, 2]),
    ]
    for k, call in enumerate(bad):
        assert call() == SPF_E_INVALID, k
        assert same(snapshot(mixed, t), rows), k
        assert np.array_equal(np.array([t.changed(i) for i in range(V)]), bits), k
        assert t.delta_fetch(z)["col"].tolist() == pk["col"].tolist(), k  # the pack is still good


@pytest.mark.parametrize("lfa", [False, True])
def test_selected_column_is_refused_and_others_patch_beside_it(mixed, lfa):
    """Column 3 is a selected one (one candidate): patching it is
    SPF_E_UNSUPPORTED; a patch that changes the length of column 1's list moves
    column 3's candidate flags along, so a rerun still selects it."""
    ann = [[1], [2, 4], [], [8], [5]]
    sel = {3: ([], [1])}
    t = mixed.table(ann, lfa, sel)
    before = snapshot(mixed, t)
    assert raw_patch(t, 2, [1, 3], [0, 1, 2], [1, 2]) == SPF_E_UNSUPPORTED
    assert same(snapshot(mixed, t), before)
    counts = t.patch_columns([1, 4], [[2, 4, 6, 9], []])
    ann2 = [[1], [2, 4, 6, 9], [], [8], []]
    want = snapshot(mixed, mixed.table(ann2, lfa, sel))
    after = snapshot(mixed, t)
    assert same(after, want)
    assert counts.tolist() == expected_bits(before, after, [1, 4], None, False).sum(axis=1).tolist()
    assert same(snapshot(mixed, t.run()), want)
    assert any(r[0][3] != INF for r in want)
