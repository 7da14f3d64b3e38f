"""spf_route_table_diff_mapped straight through the C ABI (ctypes): the
route delta of every node (getRouteDelta, openr/decision/Decision.cpp:47-85)
between two route tables whose nodes, columns and link layouts differ.

The expected bitmaps are computed here, in numpy, from spf_route_table_fetch
(and _fetch_link_metrics) of both tables with the cell rule of
include/openr_spf.h: cell (i, p) of the newer table against cell
(row_of[i], col_of[p]) of the older one, link masks through link_of as sets
of links, best announcers through node_of, dirty announcers, gone columns.
No oracle is involved.  Where the topology makes it possible the rule's
result is checked a second way too: by decoding both cells into (metric,
best node name, set of link names) and comparing those.
"""

import ctypes as C

import numpy as np
import pytest

from openr_amd import abi

pytestmark = pytest.mark.gpu

NONE = abi.SPF_MAP_NONE
INF = 0xFFFFFFFF


class Net:
    """A graph given as named links, its all-sources query and route table.
    links: [(u, v, metric u->v, metric v->u, name)]; a node's link bits are
    in the input order of `links` (abi.Csr.from_links)."""

    def __init__(self, V, links, announcers, lfa=False, overloaded=None):
        self.V = V
        self.csr = abi.Csr.from_links(V, [l[:4] for l in links], overloaded)
        self.rows = [[] for _ in range(V)]
        for u, v, _, _, name in links:
            self.rows[u].append(name)
            self.rows[v].append(name)
        self.g = abi.Graph(self.csr)
        self.q = self.g.query(np.arange(V, dtype=np.uint32), abi.SPF_F_NEXTHOPS).run()
        self.lfa = lfa
        self.t = abi.RouteTable(self.q, announcers, abi.SPF_RT_LFA if lfa else 0).run()
        self.P = len(announcers)
        self._cells = {}

    def cells(self, i):
        """(metric [P], best [P], link bits bool [P, deg], link metrics [P, deg] or None)"""
        if i not in self._cells:
            deg = len(self.rows[i])
            metric, best, words = self.t.fetch(i)
            bits = np.unpackbits(np.ascontiguousarray(words).view(np.uint8), axis=1,
                                 bitorder="little")[:, :deg].astype(bool)
            lm = self.t.fetch_link_metrics(i, deg) if self.lfa else None
            self._cells[i] = (metric.copy(), best.copy(), bits, lm)
        return self._cells[i]

    def close(self):
        self.t.close()
        self.q.close()
        self.g.close()


def link_maps(A, B, row_of):
    """Per newer row: older bit position of every link, by link name."""
    out = []
    for i in range(B.V):
        ia = row_of[i]
        if ia == NONE:
            out.append([NONE] * len(B.rows[i]))
            continue
        pos = {name: j for j, name in enumerate(A.rows[ia])}
        out.append([pos.get(name, NONE) for name in B.rows[i]])
    return out


def expected(A, B, row_of, col_of, gone, node_of, link_of, dirty):
    """The rule of include/openr_spf.h in numpy: (changed bool [rows, P],
    gone bool [rows, len(gone)])."""
    ch = np.zeros((B.V, B.P), dtype=bool)
    gn = np.zeros((B.V, len(gone)), dtype=bool)
    for i in range(B.V):
        mb, bb, Lb, xb = B.cells(i)
        ia = row_of[i]
        if ia == NONE:
            ch[i] = mb != INF
            continue
        ma, ba, La, xa = A.cells(ia)
        gn[i] = [ma[c] != INF for c in gone]
        lo = link_of[i]
        for p in range(B.P):
            pa = col_of[p]
            has_b = mb[p] != INF
            has_a = pa != NONE and ma[pa] != INF
            if not (has_a and has_b):
                ch[i, p] = has_a != has_b
                continue
            if ma[pa] != mb[p] or node_of[ba[pa]] != bb[p] or int(bb[p]) in dirty.get(p, ()):
                ch[i, p] = True
                continue
            js = np.flatnonzero(Lb[p])
            img = [lo[j] for j in js]
            if NONE in img or set(img) != set(np.flatnonzero(La[pa]).tolist()):
                ch[i, p] = True
                continue
            if B.lfa:
                ch[i, p] = any(xb[p, j] != xa[pa, t] for j, t in zip(js, img))
    return ch, gn


def truth_by_names(A, B, name_a, name_b, col_of):
    """Changed cells by decoding: (metric, best node name, {link name: its
    metric}) of the newer cell against the older cell of the same node name
    and column; no maps involved."""
    row_a = {n: i for i, n in enumerate(name_a)}
    ch = np.zeros((B.V, B.P), dtype=bool)

    def decode(N, names, i, p):
        m, b, L, x = N.cells(i)
        if m[p] == INF:
            return None
        return (int(m[p]), names[b[p]],
                {N.rows[i][j]: (int(x[p, j]) if N.lfa else 0) for j in np.flatnonzero(L[p])})

    for i in range(B.V):
        ia = row_a.get(name_b[i])
        for p in range(B.P):
            new = decode(B, name_b, i, p)
            old = None if ia is None or col_of[p] == NONE else decode(A, name_a, ia, col_of[p])
            ch[i, p] = new != old
    return ch


def run_mapped(A, B, row_of, col_of, gone, node_of, link_of, dirty):
    """The device diff with these maps: (counts, changed bool, gone bool)."""
    link_off = np.zeros(B.V + 1, dtype=np.uint32)
    link_off[1:] = np.cumsum([len(x) for x in link_of])
    flat = [x for row in link_of for x in row]
    dirty_off = np.zeros(B.P + 1, dtype=np.uint32)
    dirty_off[1:] = np.cumsum([len(dirty.get(p, ())) for p in range(B.P)])
    dflat = [x for p in range(B.P) for x in dirty.get(p, ())]
    counts = B.t.diff_mapped(A.t, row_of=row_of, col_of=col_of, gone_cols=gone, node_of=node_of,
                             link_off=link_off, link_of=flat, dirty_off=dirty_off, dirty_ann=dflat)
    ch = np.array([B.t.changed(i) for i in range(B.V)]).reshape(B.V, B.P)
    gn = np.array([B.t.changed_gone(i) for i in range(B.V)]).reshape(B.V, len(gone))
    return counts, ch, gn


def check(A, B, row_of, col_of, gone, node_of, dirty=None, link_of=None):
    dirty = dirty or {}
    link_of = link_of or link_maps(A, B, row_of)
    want_ch, want_gn = expected(A, B, row_of, col_of, gone, node_of, link_of, dirty)
    counts, ch, gn = run_mapped(A, B, row_of, col_of, gone, node_of, link_of, dirty)
    bad = np.argwhere(ch != want_ch)
    assert bad.size == 0, f"changed bitmap differs at (row, col) {bad[:8].tolist()}"
    bad = np.argwhere(gn != want_gn)
    assert bad.size == 0, f"gone bitmap differs at (row, gone col) {bad[:8].tolist()}"
    assert counts.tolist() == (want_ch.sum(axis=1) + want_gn.sum(axis=1)).tolist()
    return want_ch, want_gn


def grid_links(n, metric=lambda u, v: 1):
    links = []
    for r in range(n):
        for c in range(n):
            v = r * n + c
            if c + 1 < n:
                links.append((v, v + 1, metric(v, v + 1), metric(v + 1, v), f"{v}-{v + 1}"))
            if r + 1 < n:
                links.append((v, v + n, metric(v, v + n), metric(v + n, v), f"{v}-{v + n}"))
    return links


# 65 single-announcer prefixes (two ballot words, ragged tail) + one anycast
GRID_ANN = [[k] for k in range(64)] + [[0]] + [[5, 40, 63]]


def test_link_removed_bits_shift_inside_one_word(gpu_ready):
    """8x8 grid, interior link 27-28 removed: the bits of rows 27 and 28
    shift down by one position from the removed link on.  Every row reports
    exactly the cells whose route changed; in rows 27 and 28 the cells the
    removed link did not carry report 0 although their mask words differ."""
    links = grid_links(8)
    A = Net(64, links, GRID_ANN)
    B = Net(64, [l for l in links if l[4] != "27-28"], GRID_ANN)
    try:
        ident = np.arange(64, dtype=np.uint32)
        col_of = np.arange(66, dtype=np.uint32)
        want, _ = check(A, B, ident, col_of, [], ident)
        names = [str(i) for i in range(64)]
        truth = truth_by_names(A, B, names, names, col_of)
        assert (want == truth).all()
        for r in (27, 28):
            _, _, La, _ = A.cells(r)
            _, _, Lb, _ = B.cells(r)
            j = A.rows[r].index("27-28")
            assert j < len(A.rows[r]) - 1  # links after it do shift
            shifted = [p for p in range(66) if not truth[r, p] and La[p, j + 1:].any()]
            assert shifted, "no unchanged route over a shifted bit"
            for p in shifted:
                assert La[p].tolist() != np.append(Lb[p], False).tolist()
            assert truth[r].any() and not truth[r].all()
        # the plain diff still refuses this pair
        out = np.zeros(64, dtype=np.uint32)
        st = abi.load().spf_route_table_diff(A.t.h, B.t.h, out.ctypes.data_as(C.POINTER(C.c_uint32)))
        assert st == abi.SPF_E_UNSUPPORTED
    finally:
        A.close()
        B.close()


def _hub_nets(lfa):
    """Ring of 130 nodes + hub 130 with a spoke to every ring node (130
    links: three mask words).  Newer: the hub's links at row positions 3 and
    64 removed, one parallel spoke added in the middle of its row."""
    n = 130
    ring = [(i, (i + 1) % n, 3, 3, f"r{i}") for i in range(n)]
    spokes = [(n, i, 2 + i % 3, 2 + (i * 7) % 4, f"s{i}") for i in range(n)]
    ann = [[k] for k in range(n + 1)] + [[2, 66, 120]]
    A = Net(n + 1, ring + spokes, ann, lfa)
    assert A.rows[n][3] == "s3" and A.rows[n][64] == "s64"
    spokes2 = [s for s in spokes if s[4] not in ("s3", "s64")]
    spokes2.insert(60, (n, 50, 2, 2, "s50b"))
    B = Net(n + 1, ring + spokes2, ann, lfa)
    return A, B, n


@pytest.mark.parametrize("lfa", [False, True])
def test_hub_row_links_removed_and_added(gpu_ready, lfa):
    A, B, n = _hub_nets(lfa)
    try:
        assert len(A.rows[n]) == 130 and len(B.rows[n]) == 129
        ident = np.arange(n + 1, dtype=np.uint32)
        col_of = np.arange(B.P, dtype=np.uint32)
        want, _ = check(A, B, ident, col_of, [], ident)
        names = [str(i) for i in range(n + 1)]
        assert (want == truth_by_names(A, B, names, names, col_of)).all()
        # the hub row has routes over all three words, changed and unchanged
        _, _, Lb, _ = B.cells(n)
        assert Lb[:, :64].any() and Lb[:, 64:128].any() and Lb[:, 128:].any()
        assert want[n].any() and not want[n].all()
    finally:
        A.close()
        B.close()


def test_columns_permuted_new_gone_and_dirty(gpu_ready):
    """8x8 grid with a few metrics raised, plus a separate 4-node chain; the
    older table has 70 more columns (gone: two bitmap words), the newer one
    has its columns permuted and one new column.  best is the smallest
    reachable announcer, so the column announced by {40, 66} has best 40 in
    the grid and 66 on the chain: with 40 dirty, only grid rows are marked."""
    chain = [(64, 65, 1, 1, "c0"), (65, 66, 1, 1, "c1"), (66, 67, 1, 1, "c2")]
    links = grid_links(8) + chain
    raised = {"9-10", "27-35", "44-45"}
    links2 = [(u, v, a + 4 * (k in raised), b + 4 * (k in raised), k) for u, v, a, b, k in links]
    kept = GRID_ANN + [[40, 66]]  # 67 columns
    gone_ann = [[(7 * k) % 64] if k % 5 else [(7 * k) % 64, (11 * k + 3) % 64] for k in range(70)]
    ann_a = kept[:30] + gone_ann[:35] + kept[30:] + gone_ann[35:]
    cols_a = list(range(30)) + [None] * 35 + list(range(30, 67)) + [None] * 35
    rng = np.random.RandomState(5)
    perm = rng.permutation(67)  # newer column k is kept[perm[k]]
    ann_b = [kept[k] for k in perm] + [[12, 51]]
    where_a = {c: pa for pa, c in enumerate(cols_a) if c is not None}
    col_of = np.array([where_a[k] for k in perm] + [NONE], dtype=np.uint32)
    gone = [pa for pa, c in enumerate(cols_a) if c is None]
    assert len(gone) == 70
    col = int(np.flatnonzero(perm == 66)[0])
    A = Net(68, links, ann_a)
    B = Net(68, links2, ann_b)
    try:
        ident = np.arange(68, dtype=np.uint32)
        want, want_gone = check(A, B, ident, col_of, gone, ident, dirty={col: [40]})
        # the dirty announcer is best for some rows and not for others, and it
        # is what marks them: without it those rows' cells are unchanged
        plain, _ = expected(A, B, ident, col_of, gone, ident, link_maps(A, B, ident), {})
        best = np.array([B.cells(i)[1][col] for i in range(68)])
        assert (best == 40).sum() == 63 and (best == 66).sum() == 3
        only_dirty = want[:, col] & ~plain[:, col]
        assert only_dirty.any() and (best[only_dirty] == 40).all()
        assert not want[best == 66, col].any()
        assert (want[:, 67] == (np.array([B.cells(i)[0][67] for i in range(68)]) != INF)).all()
        assert want_gone[:, :64].any() and want_gone[:, 64:].any() and not want_gone.all()
    finally:
        A.close()
        B.close()


def _with_node():
    """6x6 grid (36 nodes) and the same grid with a node inserted at id 17
    (every id from 17 on shifts), linked to old nodes 3 and 30."""
    base = grid_links(6, metric=lambda u, v: 1 + (u * 5 + v) % 3)
    up = lambda v: v + (v >= 17)  # noqa: E731
    more = [(up(u), up(v), a, b, k) for u, v, a, b, k in base]
    more += [(17, up(3), 2, 2, "x-3"), (17, up(30), 2, 2, "x-30")]
    names36 = [f"g{v}" for v in range(36)]
    names37 = names36[:17] + ["x"] + names36[17:]
    small = Net(36, base, [[k] for k in range(36)] + [[4, 33]])
    big = Net(37, more, [[up(k)] for k in range(36)] + [[up(4), up(33)], [17]])
    return small, big, names36, names37


def test_node_inserted_in_the_middle_of_the_id_range(gpu_ready):
    A, B, names_a, names_b = _with_node()
    try:
        row_of = np.array([v - (v > 17) if v != 17 else NONE for v in range(37)], dtype=np.uint32)
        node_of = np.array([v + (v >= 17) for v in range(36)], dtype=np.uint32)
        col_of = np.array(list(range(37)) + [NONE], dtype=np.uint32)
        want, _ = check(A, B, row_of, col_of, [], node_of)
        assert (want == truth_by_names(A, B, names_a, names_b, col_of)).all()
        # the new row: every route is an update
        assert (want[17] == (B.cells(17)[0] != INF)).all() and want[17].sum() == 37
        # the new node's own prefix is a new route everywhere else
        assert want[:, 37].sum() == 36
        # rows that only had their ids shifted keep unchanged cells unchanged
        assert not want[:17, :37].all() and not want[18:, :37].all()
    finally:
        A.close()
        B.close()


def test_node_removed(gpu_ready):
    B, A, names_b, names_a = _with_node()  # older: 37 nodes, newer: 36
    try:
        row_of = np.array([v + (v >= 17) for v in range(36)], dtype=np.uint32)
        node_of = np.array([v - (v > 17) if v != 17 else NONE for v in range(37)], dtype=np.uint32)
        col_of = np.arange(37, dtype=np.uint32)
        want, want_gone = check(A, B, row_of, col_of, [37], node_of)
        assert (want == truth_by_names(A, B, names_a, names_b, col_of)).all()
        assert want_gone.all()  # every remaining node had a route to the removed node's prefix
    finally:
        A.close()
        B.close()


@pytest.mark.parametrize("lfa", [False, True])
def test_identity_maps_equal_the_plain_diff(gpu_ready, lfa):
    """Equal layouts (metric changes and a drained node): null maps, and
    explicit identity maps, give spf_route_table_diff's counts and bitmaps."""
    links = grid_links(8)
    raised = {"9-10", "27-35", "44-45", "0-1"}
    links2 = [(u, v, a + 2 * (k in raised), b + 5 * (k in raised), k) for u, v, a, b, k in links]
    ov = np.zeros(64, dtype=np.uint8)
    ov[20] = 1
    A = Net(64, links, GRID_ANN, lfa)
    B = Net(64, links2, GRID_ANN, lfa, overloaded=ov)
    try:
        plain = B.t.diff(A.t)
        plain_bits = np.array([B.t.changed(i) for i in range(64)])
        assert plain.sum() > 0 and plain.tolist() == plain_bits.sum(axis=1).tolist()
        null = B.t.diff_mapped(A.t)
        null_bits = np.array([B.t.changed(i) for i in range(64)])
        assert null.tolist() == plain.tolist() and (null_bits == plain_bits).all()
        ident = np.arange(64, dtype=np.uint32)
        want, _ = check(A, B, ident, np.arange(66, dtype=np.uint32), [], ident)
        assert (want == plain_bits).all()
    finally:
        A.close()
        B.close()


def test_errors(gpu_ready):
    links = grid_links(4)
    ann = [[k] for k in range(16)]
    A = Net(16, links, ann)
    B = Net(16, [l for l in links if l[4] != "5-6"], ann)
    L = Net(16, links, ann, lfa=True)
    lib = abi.load()
    try:
        ident = np.arange(16, dtype=np.uint32)
        lo = link_maps(A, B, ident)
        # two links of row 0 mapped to the same older link
        dup = [list(r) for r in lo]
        dup[0] = [0] * len(dup[0])
        with pytest.raises(abi.SpfError, match="invalid"):
            run_mapped(A, B, ident, ident, [], ident, dup, {})
        assert b"link_of" in lib.spf_last_error_detail()
        # two columns mapped to the same older column
        with pytest.raises(abi.SpfError, match="invalid"):
            run_mapped(A, B, ident, np.zeros(16, dtype=np.uint32), [], ident, lo, {})
        # out of range
        bad = ident.copy()
        bad[3] = 16
        with pytest.raises(abi.SpfError, match="invalid"):
            run_mapped(A, B, bad, ident, [], ident, lo, {})
        with pytest.raises(abi.SpfError, match="invalid"):
            run_mapped(A, B, ident, ident, [16], ident, lo, {})
        # identity links over rows with different link counts
        out = np.zeros(16, dtype=np.uint32)
        st = lib.spf_route_table_diff_mapped(A.t.h, B.t.h, None, out.ctypes.data_as(C.POINTER(C.c_uint32)))
        assert st == abi.SPF_E_INVALID
        # LFA against non-LFA
        st = lib.spf_route_table_diff_mapped(L.t.h, A.t.h, None, out.ctypes.data_as(C.POINTER(C.c_uint32)))
        assert st == abi.SPF_E_UNSUPPORTED
        # the plain diff still refuses the differing pair
        st = lib.spf_route_table_diff(A.t.h, B.t.h, out.ctypes.data_as(C.POINTER(C.c_uint32)))
        assert st == abi.SPF_E_UNSUPPORTED
        # and the valid maps still work after the refusals
        check(A, B, ident, ident, [], ident)
    finally:
        A.close()
        B.close()
        L.close()
