"""spf_route_table_delta_pack / _delta_fetch / _fetch_cells straight through
the C ABI (ctypes): the changed cells of the last diff as one device-built
record list (the updates and deletes of getRouteDelta,
openr/decision/Decision.cpp:47-85, for every node at once), and the sparse
read of listed cells.

The expected arrays come from the existing readers alone -- changed(i),
changed_gone(i), fetch(i), fetch_link_metrics(i) -- with np.flatnonzero and
cumsum; equality is exact.
"""

import ctypes as C

import numpy as np
import pytest

from openr_amd import abi
from tests.test_route_table_diff_mapped_gpu import (
    GRID_ANN, NONE, Net, _hub_nets, _with_node, grid_links, link_maps, run_mapped)

pytestmark = pytest.mark.gpu

FILL_BLOCK = 256  # threads of the fill workgroup: bitmap words it scans per pass


def expected_pack(B):
    """The packed list of B's last diff from the per-row readers."""
    cell_off, gone_off = [0], [0]
    col, metric, best, links, lmet, gone = [], [], [], [], [], []
    for i in range(B.V):
        ch = np.flatnonzero(B.t.changed(i)) if B.P else np.zeros(0, dtype=np.int64)
        gn = np.flatnonzero(B.t.changed_gone(i)) if B.t.num_gone else np.zeros(0, dtype=np.int64)
        m, b, words = B.t.fetch(i)
        col.append(ch.astype(np.uint32))
        metric.append(m[ch])
        best.append(b[ch])
        links.append(words[ch].reshape(-1))
        if B.lfa:
            lmet.append(B.t.fetch_link_metrics(i, len(B.rows[i]))[ch].reshape(-1))
        gone.append(gn.astype(np.uint32))
        cell_off.append(cell_off[-1] + len(ch))
        gone_off.append(gone_off[-1] + len(gn))
    cat = lambda xs, dt: np.concatenate(xs).astype(dt) if xs else np.zeros(0, dtype=dt)  # noqa: E731
    return {
        "cell_off": np.array(cell_off, dtype=np.uint64), "col": cat(col, np.uint32),
        "metric": cat(metric, np.uint32), "best": cat(best, np.uint32),
        "links": cat(links, np.uint64), "link_metrics": cat(lmet, np.uint32),
        "gone_off": np.array(gone_off, dtype=np.uint64), "gone": cat(gone, np.uint32),
    }


def check_pack(B, mapped):
    """Pack B's last diff and compare every array; returns the pack."""
    if not mapped:
        B.t.num_gone = 0  # the Python view's gone count is the last MAPPED diff's
    got = B.t.delta_pack()
    want = expected_pack(B)
    for k, w in want.items():
        assert got[k].dtype == w.dtype and got[k].tolist() == w.tolist(), k
    assert got["cells"] == len(want["col"]) and got["num_gone"] == len(want["gone"])
    assert got["link_words"] == len(want["links"])
    assert got["num_link_metrics"] == len(want["link_metrics"])
    return got


def ring_nets(V, P, lfa=False, seed=0, live=None):
    """A V-ring with one chord; the newer net raises two ring metrics, which
    cuts nodes 1 and 2 off the cheap way round: their route to any announcer
    outside {1, 2} changes, and node 0's to one inside.  Announcers seeded at
    random; with `live` (column indices) every other column is announced by
    all nodes, so it has no route in any row and never changes."""
    rng = np.random.RandomState(seed)
    links = [(i, (i + 1) % V, 2, 2, f"r{i}") for i in range(V)] + [(0, V // 2, 3, 3, "chord")]
    links2 = [(u, v, a + 5 * (k in ("r0", "r2")), b + 5 * (k in ("r0", "r2")), k)
              for u, v, a, b, k in links]
    ann = [sorted(set(rng.randint(0, V, size=1 + p % 2).tolist())) for p in range(P)]
    if live is not None:
        keep = set(live)
        ann = [a if p in keep else list(range(V)) for p, a in enumerate(ann)]
    return Net(V, links, ann, lfa), Net(V, links2, ann, lfa)


@pytest.mark.parametrize("lfa", [False, True])
@pytest.mark.parametrize("P", [1, 63, 64, 65, 130])
def test_column_counts_straddling_bitmap_words(gpu_ready, P, lfa):
    A, B = ring_nets(6 + P % 7, P, lfa, seed=P)
    try:
        counts = B.t.diff(A.t)
        got = check_pack(B, mapped=False)
        assert got["cells"] == counts.sum() > 0
        assert got["num_gone"] == 0 and not got["gone_off"].any()
    finally:
        A.close()
        B.close()


def test_more_words_per_row_than_one_fill_pass_scans(gpu_ready):
    """P = 64 * (workgroup threads + 1) + 1: 258 bitmap words per row, so the
    fill workgroup's scan over word popcounts takes two passes and the second
    carries the first's running prefix."""
    P = 64 * (FILL_BLOCK + 1) + 1
    edge = 64 * FILL_BLOCK  # first column of the second pass
    live = np.random.RandomState(2).choice(P, size=120, replace=False).tolist()
    live += [0, 63, 64, edge - 1, edge, edge + 30, P - 1]
    A, B = ring_nets(6, P, seed=11, live=live)
    try:
        counts = B.t.diff(A.t)
        got = check_pack(B, mapped=False)
        # 127 live columns, two to six changed rows each: a few hundred cells
        assert got["cells"] == counts.sum() and 100 <= got["cells"] <= 127 * 6
        # changed cells on both sides of the pass boundary, in one row
        per_row = [got["col"][int(a):int(b)] for a, b in zip(got["cell_off"][:-1], got["cell_off"][1:])]
        assert any((c < 64 * FILL_BLOCK).any() and (c >= 64 * FILL_BLOCK).any() for c in per_row)
    finally:
        A.close()
        B.close()


@pytest.mark.parametrize("lfa", [False, True])
def test_rows_with_zero_one_and_three_link_words(gpu_ready, lfa):
    """The 130-link hub (three mask words) among ring nodes (one word):
    every row's cells carry its own word count (and, with SPF_RT_LFA, its own
    number of link metrics)."""
    A, B, n = _hub_nets(lfa)
    try:
        ident = np.arange(n + 1, dtype=np.uint32)
        run_mapped(A, B, ident, np.arange(B.P, dtype=np.uint32), [], ident,
                   link_maps(A, B, ident), {})
        got = check_pack(B, mapped=True)
        assert B.t.link_words(n) == 3 and B.t.link_words(0) == 1
        assert got["cell_off"][n + 1] > got["cell_off"][n]
    finally:
        A.close()
        B.close()


@pytest.mark.parametrize("lfa", [False, True])
def test_row_without_links_between_changed_rows(gpu_ready, lfa):
    """Node 5 has no link in either table (W = 0): no route, so no changed
    cell and no link word, between rows 4 and 6 that have some.  (A row
    without links has no route, and the diffs map a row to one with the same
    link count or through a full link map, so its cells never change.)
    fetch_cells over rows 4, 5, 5, 6 packs no link word for the two cells of
    row 5."""
    V = 8
    ring = [(0, 1, 1, 1, "a"), (1, 2, 1, 1, "b"), (2, 3, 1, 1, "c"), (3, 4, 1, 1, "d"),
            (4, 6, 1, 1, "e"), (6, 7, 1, 1, "f"), (7, 0, 1, 1, "g")]
    ring2 = [l for l in ring if l[4] != "c"] + [(2, 4, 1, 1, "h")]
    ann = [[k] for k in range(V)] + [[0, 6]]
    A = Net(V, ring, ann, lfa)
    B = Net(V, ring2, ann, lfa)
    try:
        ident = np.arange(V, dtype=np.uint32)
        counts, _, _ = run_mapped(A, B, ident, np.arange(B.P, dtype=np.uint32), [], ident,
                                  link_maps(A, B, ident), {})
        got = check_pack(B, mapped=True)
        off = got["cell_off"]
        assert B.t.link_words(5) == 0 and B.t.link_words(4) == 1
        assert counts[5] == 0 and off[5] == off[6] and counts[4] > 0 and counts[6] > 0
        degs = [len(r) for r in B.rows]
        metric, best, links, lmet = B.t.fetch_cells([4, 5, 5, 6], [2, 0, 8, 2], degs)
        assert metric[1] == metric[2] == 0xFFFFFFFF and metric[0] != 0xFFFFFFFF
        assert links.tolist() == [int(B.t.fetch(4)[2][2, 0]), int(B.t.fetch(6)[2][2, 0])]
        assert len(lmet) == (degs[4] + degs[6] if lfa else 0)
    finally:
        A.close()
        B.close()


def test_row_with_every_cell_changed(gpu_ready):
    """A node the older table lacks (inserted in the middle of the id range):
    every route of its row is a changed cell."""
    A, B, _, _ = _with_node()
    try:
        row_of = np.array([v - (v > 17) if v != 17 else NONE for v in range(37)], dtype=np.uint32)
        node_of = np.array([v + (v >= 17) for v in range(36)], dtype=np.uint32)
        col_of = np.array(list(range(37)) + [NONE], dtype=np.uint32)
        counts, ch, _ = run_mapped(A, B, row_of, col_of, [], node_of, link_maps(A, B, row_of), {})
        got = check_pack(B, mapped=True)
        # row 17: all 37 routes (its own prefix is no route and unchanged)
        assert got["cell_off"][18] - got["cell_off"][17] == 37 == ch[17].sum()
        assert got["cell_off"][-1] + got["gone_off"][-1] == counts.sum()
    finally:
        A.close()
        B.close()


@pytest.mark.parametrize("lfa", [False, True])
def test_equal_layout_drain(gpu_ready, lfa):
    links = grid_links(8)
    ov = np.zeros(64, dtype=np.uint8)
    ov[20] = 1
    A = Net(64, links, GRID_ANN, lfa)
    B = Net(64, links, GRID_ANN, lfa, overloaded=ov)
    try:
        counts = B.t.diff(A.t)
        got = check_pack(B, mapped=False)
        assert got["cells"] == counts.sum() > 0
        assert got["num_gone"] == 0 and not got["gone_off"].any()
    finally:
        A.close()
        B.close()


def _permuted_pair():
    """Columns permuted, one new, 70 gone (two gone bitmap words), a node
    removed and metrics raised: 8x8 grid + chain, as the mapped-diff test."""
    chain = [(64, 65, 1, 1, "c0"), (65, 66, 1, 1, "c1"), (66, 67, 1, 1, "c2")]
    links = grid_links(8) + chain
    raised = {"9-10", "27-35", "44-45"}
    links2 = [(u, v, a + 4 * (k in raised), b + 4 * (k in raised), k) for u, v, a, b, k in links]
    kept = GRID_ANN + [[40, 66]]
    gone_ann = [[(7 * k) % 64] if k % 5 else [(7 * k) % 64, (11 * k + 3) % 64] for k in range(70)]
    ann_a = kept[:30] + gone_ann[:35] + kept[30:] + gone_ann[35:]
    cols_a = list(range(30)) + [None] * 35 + list(range(30, 67)) + [None] * 35
    perm = np.random.RandomState(5).permutation(67)
    ann_b = [kept[k] for k in perm] + [[12, 51]]
    where_a = {c: pa for pa, c in enumerate(cols_a) if c is not None}
    col_of = np.array([where_a[k] for k in perm] + [NONE], dtype=np.uint32)
    gone = [pa for pa, c in enumerate(cols_a) if c is None]
    return Net(68, links, ann_a), Net(68, links2, ann_b), col_of, gone


def test_mapped_diff_permuted_new_and_gone_columns(gpu_ready):
    A, B, col_of, gone = _permuted_pair()
    try:
        ident = np.arange(68, dtype=np.uint32)
        counts, ch, gn = run_mapped(A, B, ident, col_of, gone, ident, link_maps(A, B, ident), {})
        got = check_pack(B, mapped=True)
        assert got["cell_off"][-1] + got["gone_off"][-1] == counts.sum()
        assert got["num_gone"] == gn.sum() > 0 and got["cells"] == ch.sum() > 0
        assert (got["gone"] >= 64).any() and (got["gone"] < 64).any()
    finally:
        A.close()
        B.close()


def test_mapped_diff_nodes_inserted_and_removed(gpu_ready):
    small, big, _, _ = _with_node()
    try:
        # older: 37 nodes, newer: 36 -- the removed node's prefix is a gone column
        row_of = np.array([v + (v >= 17) for v in range(36)], dtype=np.uint32)
        node_of = np.array([v - (v > 17) if v != 17 else NONE for v in range(37)], dtype=np.uint32)
        counts, ch, gn = run_mapped(big, small, row_of, np.arange(37, dtype=np.uint32), [37],
                                    node_of, link_maps(big, small, row_of), {})
        got = check_pack(small, mapped=True)
        assert got["cell_off"][-1] + got["gone_off"][-1] == counts.sum()
        assert got["num_gone"] == 36 and gn.all()
    finally:
        big.close()
        small.close()


def test_identical_tables_pack_nothing(gpu_ready):
    links = grid_links(3)
    ann = [[k % 9] for k in range(65)]
    A = Net(9, links, ann)
    B = Net(9, links, ann)
    try:
        assert B.t.diff(A.t).sum() == 0
        got = B.t.delta_pack()
        assert (got["cells"], got["num_gone"], got["link_words"], got["num_link_metrics"]) == (0,) * 4
        assert not got["cell_off"].any() and not got["gone_off"].any()
        assert len(got["cell_off"]) == A.V + 1 and len(got["col"]) == 0
    finally:
        A.close()
        B.close()


def test_second_diff_then_pack_returns_the_second_result(gpu_ready):
    links = grid_links(8)
    ov = np.zeros(64, dtype=np.uint8)
    ov[20] = 1
    raised = {"9-10", "27-35"}
    links2 = [(u, v, a + 3 * (k in raised), b + 3 * (k in raised), k) for u, v, a, b, k in links]
    A = Net(64, links, GRID_ANN)
    A2 = Net(64, links2, GRID_ANN)
    B = Net(64, links, GRID_ANN, overloaded=ov)
    try:
        B.t.diff(A.t)
        first = check_pack(B, mapped=False)
        B.t.diff(A2.t)
        second = check_pack(B, mapped=False)
        assert first["col"].tolist() != second["col"].tolist() or \
            first["cell_off"].tolist() != second["cell_off"].tolist()
        # and a mapped diff with a gone column after the plain ones
        ident = np.arange(64, dtype=np.uint32)
        counts, _, _ = run_mapped(A, B, ident, np.arange(66, dtype=np.uint32), [3], ident,
                                  link_maps(A, B, ident), {})
        third = check_pack(B, mapped=True)
        assert third["num_gone"] > 0
        assert third["cell_off"][-1] + third["gone_off"][-1] == counts.sum()
        # back to a plain diff: the gone list is empty again
        B.t.diff(A.t)
        again = check_pack(B, mapped=False)
        assert again["num_gone"] == 0 and again["col"].tolist() == first["col"].tolist()
    finally:
        A.close()
        A2.close()
        B.close()


def _check_cells(N, rows, cols):
    """fetch_cells(rows, cols) of N against indexing fetch(i) / fetch_link_metrics(i)."""
    degs = [len(r) for r in N.rows]
    metric, best, links, lmet = N.t.fetch_cells(rows, cols, degs)
    row = {i: N.t.fetch(i) for i in set(rows)}
    xs = {i: N.t.fetch_link_metrics(i, degs[i]) for i in set(rows)} if N.lfa else {}
    lo = mo = 0
    for k, (i, p) in enumerate(zip(rows, cols)):
        m, b, words = row[i]
        assert (metric[k], best[k]) == (m[p], b[p]), k
        W = N.t.link_words(i)
        assert links[lo:lo + W].tolist() == words[p].tolist(), k
        lo += W
        if N.lfa:
            assert lmet[mo:mo + degs[i]].tolist() == xs[i][p].tolist(), k
            mo += degs[i]
    assert lo == len(links) and mo == len(lmet)


@pytest.mark.parametrize("lfa", [False, True])
def test_staging_grows_and_is_reused_at_a_smaller_size(gpu_ready, lfa):
    """One newer table B (the 8x8 grid, node 20 drained so that cells change
    too) diffed against an older table with 1 extra column, then one with 130
    (130 gone columns: three gone-bitmap words per row instead of one, a longer
    map stage, a longer packed list), then the first again: the grow-only
    staging of B is grown and then reused at the smaller size, and the third
    pack equals the first.  The same for the gather staging of fetch_cells:
    1 cell, 300 cells, 1 cell.  Every extra column is announced by one node,
    so it has a route in the 63 other rows."""
    links = grid_links(8)
    ov = np.zeros(64, dtype=np.uint8)
    ov[20] = 1
    extra = [[(7 * k + 3) % 64] for k in range(130)]
    B = Net(64, links, GRID_ANN, lfa, overloaded=ov)
    A1 = Net(64, links, GRID_ANN + extra[:1], lfa)
    A2 = Net(64, links, GRID_ANN + extra, lfa)
    try:
        ident = np.arange(64, dtype=np.uint32)
        cols = np.arange(B.P, dtype=np.uint32)
        packs = []
        for A in (A1, A2, A1):
            gone = list(range(B.P, A.P))
            counts, _, gn = run_mapped(A, B, ident, cols, gone, ident, link_maps(A, B, ident), {})
            got = check_pack(B, mapped=True)
            assert got["cells"] > 0 and got["num_gone"] == gn.sum() == 63 * len(gone)
            assert got["cell_off"][-1] + got["gone_off"][-1] == counts.sum()
            packs.append(got)
        for k, first in packs[0].items():
            assert np.array_equal(packs[2][k], first), k
        assert packs[1]["num_gone"] == 130 * packs[0]["num_gone"]
        # the gather staging: small, large (cells repeated across rows and columns), small
        rng = np.random.RandomState(7)
        rows = rng.randint(0, 64, size=300).tolist()
        pcols = rng.randint(0, B.P, size=300).tolist()
        rows[100:110] = [rows[0]] * 10
        pcols[100:110] = [pcols[0]] * 10
        _check_cells(B, [9], [65])
        _check_cells(B, rows, pcols)
        _check_cells(B, [9], [65])
    finally:
        A1.close()
        A2.close()
        B.close()


def _fetch_status(t, z):
    """spf_route_table_delta_fetch into buffers sized by z: the status."""
    u64 = lambda n: np.zeros(max(int(n), 1), dtype=np.uint64)  # noqa: E731
    u32 = lambda n: np.zeros(max(int(n), 1), dtype=np.uint32)  # noqa: E731
    bufs = [u64(t.n + 1), u32(z.cells), u32(z.cells), u32(z.cells), u64(z.link_words),
            u32(z.link_metrics), u64(t.n + 1), u32(z.gone)]
    ptr = [b.ctypes.data_as(C.POINTER(C.c_uint64 if b.dtype == np.uint64 else C.c_uint32))
           for b in bufs]
    return abi.load().spf_route_table_delta_fetch(t.h, *ptr)


def test_too_early_stale_and_not_run_are_invalid(gpu_ready):
    lib = abi.load()
    links = grid_links(4)
    ann = [[k] for k in range(16)]
    ov = np.zeros(16, dtype=np.uint8)
    ov[5] = 1
    A = Net(16, links, ann)
    B = Net(16, links, ann, overloaded=ov)
    fresh = abi.RouteTable(A.q, ann)  # created, not run
    try:
        z = abi._RouteDeltaSizes()
        # pack before any diff; fetch before a pack
        assert lib.spf_route_table_delta_pack(B.t.h, C.byref(z)) == abi.SPF_E_INVALID
        assert _fetch_status(B.t, z) == abi.SPF_E_INVALID
        B.t.diff(A.t)
        assert _fetch_status(B.t, z) == abi.SPF_E_INVALID  # diffed, still not packed
        assert lib.spf_route_table_delta_pack(B.t.h, C.byref(z)) == abi.SPF_OK and z.cells > 0
        assert _fetch_status(B.t, z) == abi.SPF_OK
        # a later diff makes the pack stale ...
        B.t.diff(A.t)
        assert _fetch_status(B.t, z) == abi.SPF_E_INVALID
        assert lib.spf_route_table_delta_pack(B.t.h, C.byref(z)) == abi.SPF_OK
        assert _fetch_status(B.t, z) == abi.SPF_OK
        # ... and so does a later run
        B.t.run()
        assert _fetch_status(B.t, z) == abi.SPF_E_INVALID
        # fetch_cells on a table that has not run
        one = np.zeros(1, dtype=np.uint32)
        out = np.zeros(4, dtype=np.uint32)
        w = np.zeros(4, dtype=np.uint64)
        p32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32))  # noqa: E731
        st = lib.spf_route_table_fetch_cells(fresh.h, 1, p32(one), p32(one), p32(out), p32(out),
                                             w.ctypes.data_as(C.POINTER(C.c_uint64)), None)
        assert st == abi.SPF_E_INVALID
    finally:
        fresh.close()
        A.close()
        B.close()


@pytest.mark.parametrize("lfa", [False, True])
def test_fetch_cells_equals_indexing_the_rows(gpu_ready, lfa):
    A, B, n = _hub_nets(lfa)
    B.close()
    try:
        rng = np.random.RandomState(3)
        rows = rng.randint(0, n + 1, size=300).astype(np.uint32)
        rows[:40] = n  # the three-word hub row, often
        cols = rng.randint(0, A.P, size=300).astype(np.uint32)
        rows[100:110] = rows[0]  # repeats of one cell
        cols[100:110] = cols[0]
        degs = [len(r) for r in A.rows]
        metric, best, links, lmet = A.t.fetch_cells(rows, cols, degs)
        wl, wm, lo, mo = [], [], 0, 0
        for k, (i, p) in enumerate(zip(rows.tolist(), cols.tolist())):
            m, b, words = A.t.fetch(i)
            assert (metric[k], best[k]) == (m[p], b[p]), k
            W = A.t.link_words(i)
            assert links[lo:lo + W].tolist() == words[p].tolist(), k
            lo += W
            if lfa:
                x = A.t.fetch_link_metrics(i, degs[i])
                assert lmet[mo:mo + degs[i]].tolist() == x[p].tolist(), k
                mo += degs[i]
        assert lo == len(links) and mo == len(lmet)
        # n = 0
        assert abi.load().spf_route_table_fetch_cells(A.t.h, 0, None, None, None, None, None,
                                                      None) == abi.SPF_OK
        # one row, then one column, out of range: refused on the host, before
        # any launch -- the outputs keep their sentinel
        for bad_rows, bad_cols in (([0, n + 1], [0, 0]), ([0, 1], [0, A.P])):
            r = np.array(bad_rows, dtype=np.uint32)
            c = np.array(bad_cols, dtype=np.uint32)
            out_m = np.full(2, 0xABCD, dtype=np.uint32)
            out_b = np.full(2, 0xABCD, dtype=np.uint32)
            out_l = np.zeros(8, dtype=np.uint64)
            out_x = np.zeros(512, dtype=np.uint32)
            p32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32))  # noqa: E731
            st = abi.load().spf_route_table_fetch_cells(
                A.t.h, 2, p32(r), p32(c), p32(out_m), p32(out_b),
                out_l.ctypes.data_as(C.POINTER(C.c_uint64)), p32(out_x))
            assert st == abi.SPF_E_INVALID
            assert (out_m == 0xABCD).all() and (out_b == 0xABCD).all()
    finally:
        A.close()
