"""The igp word of selected columns in the route-table diff and in the packed
delta, through the C ABI (ctypes): spf_route_table_diff and _diff_mapped mark
a cell of a column selected in both tables whose igp differs,
spf_route_table_delta_fetch_igp and spf_route_table_fetch_cells_igp return the
word spf_route_table_fetch_sel reads (include/openr_spf.h).  Beside them:
the SPF_MAP_NONE entry of a dirty list (best left out of a column's compare)
and spf_route_table_diff_routes (the metric word left out on LFA tables).

The graph is a 6-node line 0 - 1 - ... - 5; the newer one has the metric of
4 - 5 raised from 1 to 2.  Column A = candidates [0, 5] where 0 always wins
(candidate 1 is a LOOSER at any distance), column B = [5, 0] where 5 always
wins, two plain columns between them.  At rows 3 and 4 column A keeps metric,
best and links (towards 0) while igp = min(d(0), d(5)) moves with the raised
metric: the cells only the igp compare finds.  The expected bitmaps are
computed here from the two tables' fetch_sel rows.
"""

import ctypes as C

import numpy as np
import pytest

from openr_amd import abi

pytestmark = pytest.mark.gpu

INF = 0xFFFFFFFF
LOOSER = 4
V = 6
ALWAYS_FIRST = ([LOOSER | (LOOSER << 3) | (LOOSER << 6)], [1, 1])
ANN = [[0, 5], [2], [0], [5, 0]]  # A, plain, plain, B
SEL = {0: ALWAYS_FIRST, 3: ALWAYS_FIRST}
# the older table of the mapped case: other column order, rows reversed
COL_OF = [3, 1, 0, 2]             # newer column -> older column
ANN_PERM = [[0], [2], [5, 0], [0, 5]]
SEL_PERM = {2: ALWAYS_FIRST, 3: ALWAYS_FIRST}
ROW_OF = [5 - i for i in range(V)]


def _line(last):
    return [(i, i + 1, 1, 1) for i in range(V - 2)] + [(V - 2, V - 1, last, last)]


class _Net:
    def __init__(self, last, sources=None):
        self.g = abi.Graph(abi.Csr.from_links(V, _line(last)))
        srcs = np.asarray(range(V) if sources is None else sources, dtype=np.uint32)
        self.q = self.g.query(srcs, abi.SPF_F_NEXTHOPS).run()
        self.tables = []

    def table(self, ann, selected=None, run=True):
        t = abi.RouteTable(self.q, ann, 0, selected=selected)
        self.tables.append(t)
        return t.run() if run else t

    def close(self):
        for t in self.tables:
            t.close()
        self.q.close()
        self.g.close()


@pytest.fixture(scope="module")
def nets(gpu_ready):
    old, new, rev = _Net(1), _Net(2), _Net(1, sources=ROW_OF)
    yield old, new, rev
    for n in (old, new, rev):
        n.close()


def _rows(t):
    return [t.fetch_sel(i) for i in range(V)]


def _expected(newer, older, selected, col_of=None, row_of=None):
    """bool [V, P]: the header's rule from the fetched rows (same link layout)"""
    rn, ro = _rows(newer), _rows(older)
    out = np.zeros((V, len(ANN)), dtype=bool)
    for i in range(V):
        ia = i if row_of is None else row_of[i]
        for p in range(len(ANN)):
            pa = p if col_of is None else col_of[p]
            mn, bn, ln, gn, _ = rn[i]
            mo, bo, lo, go, _ = ro[ia]
            out[i, p] = (mn[p] != mo[pa] or bn[p] != bo[pa] or (ln[p] != lo[pa]).any()
                         or (p in selected and gn[p] != go[pa]))
    return out


def _changed(t):
    return np.stack([t.changed(i) for i in range(V)])


def test_equal_layout_diff_marks_igp_only_cells(nets):
    old, new, _ = nets
    a, b = old.table(ANN, SEL), new.table(ANN, SEL)
    counts = b.diff(a)
    want = _expected(b, a, SEL)
    assert (_changed(b) == want).all()
    assert (counts == want.sum(axis=1)).all()
    ra, rb = _rows(a), _rows(b)
    for row, igp_old, igp_new in ((3, 2, 3), (4, 1, 2)):
        # column A: the same cell but for igp, and marked
        for k in range(3):
            assert (np.asarray(ra[row][k][0]) == np.asarray(rb[row][k][0])).all()
        assert rb[row][1][0] == 0 and rb[row][0][0] == row
        assert (ra[row][3][0], rb[row][3][0]) == (igp_old, igp_new)
        assert want[row, 0]
    assert not want[2, 0] and not want[1, 0]  # d(0) is the smaller one there
    # without the igp word those cells are equal
    assert not _expected(b, a, {})[3, 0] and not _expected(b, a, {})[4, 0]


def test_equal_layout_diff_needs_the_same_selected_columns(nets):
    old, new, _ = nets
    lib = abi.load()
    out = np.zeros(V, dtype=np.uint32)
    b = new.table(ANN, SEL)
    for other in (None, {0: ALWAYS_FIRST}, {0: ALWAYS_FIRST, 2: ([], [1])}):
        a = old.table(ANN, other)
        for x, y in ((a, b), (b, a)):
            st = lib.spf_route_table_diff(x.h, y.h, out.ctypes.data_as(C.POINTER(C.c_uint32)))
            assert st == abi.SPF_E_UNSUPPORTED, other


def test_mapped_diff_reads_the_older_igp_through_the_maps(nets):
    old, new, rev = nets
    a, b = rev.table(ANN_PERM, SEL_PERM), new.table(ANN, SEL)
    counts = b.diff_mapped(a, row_of=np.asarray(ROW_OF, dtype=np.uint32),
                           col_of=np.asarray(COL_OF, dtype=np.uint32))
    want = _expected(b, a, SEL, COL_OF, ROW_OF)
    # the same answer as against the older table in the newer one's layout
    assert (want == _expected(b, old.table(ANN, SEL), SEL)).all()
    assert want[3, 0] and want[4, 0] and not want[2, 0]
    assert (_changed(b) == want).all()
    assert (counts == want.sum(axis=1)).all()


def test_mapped_diff_rejects_selected_paired_with_unselected(nets):
    old, new, _ = nets
    a, b = old.table(ANN, SEL), new.table(ANN, SEL)
    with pytest.raises(abi.SpfError, match="selected column with an unselected"):
        b.diff_mapped(a, col_of=np.asarray([1, 0, 2, 3], dtype=np.uint32))
    # left without a counterpart the pair is accepted
    none = abi.SPF_MAP_NONE
    b.diff_mapped(a, col_of=np.asarray([none, none, 2, 3], dtype=np.uint32),
                  gone_cols=np.asarray([0, 1], dtype=np.uint32))


def test_packed_delta_and_cell_list_carry_the_igp_word(nets):
    old, new, _ = nets
    a, b = old.table(ANN, SEL), new.table(ANN, SEL)
    b.diff(a)
    pk = b.delta_pack()
    igp = b.delta_fetch_igp(pk["cells"])
    rows = _rows(b)
    seen_plain = seen_selected = 0
    for i in range(V):
        for k in range(int(pk["cell_off"][i]), int(pk["cell_off"][i + 1])):
            p = int(pk["col"][k])
            assert igp[k] == rows[i][3][p], (i, p)
            assert (igp[k] == INF) == (p not in SEL or rows[i][0][p] == INF)
            seen_plain += p not in SEL
            seen_selected += p in SEL and igp[k] != INF
    assert seen_plain and seen_selected and pk["cells"] == len(igp)
    rs = [4, 4, 0, 5, 3, 4, 2, 0]
    cs = [0, 0, 3, 1, 3, 2, 0, 0]
    got = b.fetch_cells_igp(rs, cs)
    assert [int(x) for x in got] == [int(rows[r][3][c]) for r, c in zip(rs, cs)]
    assert INF in got and any(x != INF for x in got)
    # the sibling calls are unchanged beside them
    m, bst, _, _ = b.fetch_cells(rs, cs)
    assert [int(x) for x in m] == [int(rows[r][0][c]) for r, c in zip(rs, cs)]
    assert len(b.fetch_cells_igp([], [])) == 0


def test_new_calls_refuse_plain_and_stale_tables(nets):
    old, new, _ = nets
    lib = abi.load()
    buf = np.zeros(64, dtype=np.uint32)
    p32 = lambda x: x.ctypes.data_as(C.POINTER(C.c_uint32))  # noqa: E731
    rs, cs = np.zeros(2, dtype=np.uint32), np.zeros(2, dtype=np.uint32)
    # no selected columns: unsupported, packed or not
    pa, pb = old.table(ANN), new.table(ANN)
    assert lib.spf_route_table_delta_fetch_igp(pb.h, p32(buf)) == abi.SPF_E_UNSUPPORTED
    pb.diff(pa)
    assert pb.delta_pack()["cells"] > 0
    assert lib.spf_route_table_delta_fetch_igp(pb.h, p32(buf)) == abi.SPF_E_UNSUPPORTED
    assert (lib.spf_route_table_fetch_cells_igp(pb.h, 2, p32(rs), p32(cs), p32(buf))
            == abi.SPF_E_UNSUPPORTED)
    # selected columns: invalid before a pack and once the pack is stale
    a, b = old.table(ANN, SEL), new.table(ANN, SEL)
    assert lib.spf_route_table_delta_fetch_igp(b.h, p32(buf)) == abi.SPF_E_INVALID
    b.diff(a)
    assert lib.spf_route_table_delta_fetch_igp(b.h, p32(buf)) == abi.SPF_E_INVALID
    cells = b.delta_pack()["cells"]
    assert cells and lib.spf_route_table_delta_fetch_igp(b.h, p32(buf)) == abi.SPF_OK
    b.diff(a)  # the bitmaps moved on
    assert lib.spf_route_table_delta_fetch_igp(b.h, p32(buf)) == abi.SPF_E_INVALID
    b.delta_pack()
    b.run()
    assert lib.spf_route_table_delta_fetch_igp(b.h, p32(buf)) == abi.SPF_E_INVALID
    # the cell list: a table that has not run, and cells out of range
    idle = new.table(ANN, SEL, run=False)
    assert (lib.spf_route_table_fetch_cells_igp(idle.h, 2, p32(rs), p32(cs), p32(buf))
            == abi.SPF_E_INVALID)
    for r, c in ((V, 0), (0, len(ANN))):
        rs[1], cs[1] = r, c
        assert (lib.spf_route_table_fetch_cells_igp(b.h, 2, p32(rs), p32(cs), p32(buf))
                == abi.SPF_E_INVALID)


def _bitmaps(t, n):
    return np.stack([t.changed(i) for i in range(n)])


def test_dirty_list_none_entry_leaves_best_out(nets):
    """A column whose best announcer is no part of its routes (a BGP column
    selected once for all nodes): announced by 3 in the older table and by 3
    and 0 in the newer one, rows 4 and 5 keep metric and links (3 is nearer)
    while best, the smallest announcer, moves from 3 to 0."""
    old, _, _ = nets
    a, b = old.table([[3], [2]]), old.table([[3, 0], [2]])
    ra, rb = [a.fetch(i) for i in range(V)], [b.fetch(i) for i in range(V)]
    for row in (4, 5):
        assert ra[row][0][0] == rb[row][0][0] and (ra[row][2][0] == rb[row][2][0]).all()
        assert (ra[row][1][0], rb[row][1][0]) == (3, 0)
    plain = b.diff_mapped(a)
    assert _bitmaps(b, V)[[4, 5], 0].all() and plain[4] == 1 and plain[5] == 1
    off = np.asarray([0, 1, 1], dtype=np.uint32)
    counts = b.diff_mapped(a, dirty_off=off, dirty_ann=np.asarray([abi.SPF_MAP_NONE], np.uint32))
    bits = _bitmaps(b, V)
    # what is left: the cells whose metric or links moved (0 is nearer there)
    want = np.asarray([ra[i][0][0] != rb[i][0][0] or (ra[i][2][0] != rb[i][2][0]).any()
                       for i in range(V)])
    assert (bits[:, 0] == want).all() and not want[4] and not want[5] and want.any()
    assert not bits[:, 1].any() and (counts == bits.sum(axis=1)).all()
    # a dirty announcer beside the entry still marks the cells whose best it is
    off = np.asarray([0, 2, 2], dtype=np.uint32)
    b.diff_mapped(a, dirty_off=off, dirty_ann=np.asarray([abi.SPF_MAP_NONE, 0], np.uint32))
    routed = np.asarray([rb[i][0][0] != INF for i in range(V)])
    assert (_bitmaps(b, V)[:, 0] == (want | routed)).all() and routed[4]


def test_diff_routes_leaves_the_lfa_metric_word_out(gpu_ready):
    """s = 0 reaches x = 2 over D = 1 (1 + 1) or over y = 3 (2 + 2).  Draining D
    raises d(s, x) from 2 to 4, yet both links of s keep their bits and their
    own metrics: to D 1 + d(D, x) = 2 (the shortest path before, an alternate
    after), to y 2 + 2 = 4 (an alternate before, the shortest path after)."""
    links = [(0, 1, 1, 1), (1, 2, 1, 1), (0, 3, 2, 2), (3, 2, 2, 2)]
    drained = np.zeros(4, dtype=np.uint8)
    drained[1] = 1
    objs, tabs = [], []
    for ov in (None, drained):
        g = abi.Graph(abi.Csr.from_links(4, links, ov))
        q = g.query(np.arange(4, dtype=np.uint32), abi.SPF_F_NEXTHOPS).run()
        tabs.append(abi.RouteTable(q, [[2]], abi.SPF_RT_LFA).run())
        objs += [q, g]
    a, b = tabs
    try:
        cells = []
        for t in (a, b):
            cells.append([(t.fetch(i), t.fetch_link_metrics(i, 2)) for i in range(4)])
        (m0, b0, l0), x0 = cells[0][0]
        (m1, b1, l1), x1 = cells[1][0]
        assert (m0[0], m1[0]) == (2, 4) and b0[0] == b1[0] and (l0 == l1).all()
        assert sorted(x0[0].tolist()) == sorted(x1[0].tolist()) == [2, 4]
        # the header's rule with and without the metric word
        def want(with_metric):
            out = []
            for (ma, ba, la), xa in cells[0]:
                (mb, bb, lb), xb = cells[1][len(out)]
                both = ma[0] != INF and mb[0] != INF
                out.append((ma[0] != INF) != (mb[0] != INF) or (both and (
                    (with_metric and ma[0] != mb[0]) or ba[0] != bb[0] or (la != lb).any()
                    or (xa != xb).any())))
            return np.asarray(out)
        assert want(True)[0] and not want(False)[0]
        for call in (lambda: b.diff(a), lambda: b.diff_mapped(a)):
            b.diff_routes(False)
            counts = call()
            assert (_bitmaps(b, 4)[:, 0] == want(True)).all() and counts[0] == 1
            b.diff_routes(True)
            counts = call()
            assert (_bitmaps(b, 4)[:, 0] == want(False)).all() and counts[0] == 0
        plain = abi.RouteTable(objs[0], [[2]]).run()
        tabs.append(plain)
        assert abi.load().spf_route_table_diff_routes(plain.h, 1) == abi.SPF_E_INVALID
    finally:
        for t in tabs:
            t.close()
        for o in objs:
            o.close()
