"""spf_route_table_refresh_rows straight through the C ABI (ctypes): a topology
change that keeps the CSR layout (metrics patched, transit bits flipped), the
listed rows of a resident route table recomputed in place by
spf_route_refresh_kernel from a re-run or new query and swapped with the cells
they replace.

Ground truth.  Cells: a fresh RouteTable over the new query, compared exactly
in every row (which also pins that screened-out rows keep their cells).
Bitmap and counts: fresh_after.diff(fresh_before) of two fresh tables, and the
numpy cell rule of include/openr_spf.h on whole-row snapshots taken before and
after.  Pack / fetch_cells: built from the bitmap and the rows.
fetch_cells_prev: the snapshot taken before, for every row and column.
"""

import ctypes as C

import numpy as np
import pytest

from openr_amd import abi
from tests.test_route_table_patch_gpu import (DRAINED, MIXED_V, check_after_patch, mixed_links,
                                              same, seeded_lists, snapshot)

pytestmark = pytest.mark.gpu

INF = 0xFFFFFFFF
SPF_E_INVALID, SPF_E_UNSUPPORTED = -1, -4


class TNet:
    """A graph given as links [(u, v, metric u->v, metric v->u)] whose metrics
    and drained set change in place; queries and tables over it on demand."""

    def __init__(self, V, links, drained=()):
        self.V = V
        self.links = [tuple(l) for l in links]
        self.drained = set(drained)
        self.csr = self._csr()
        self.degs = [0] * V
        for u, v, _, _ in links:
            self.degs[u] += 1
            self.degs[v] += 1
        self.g = abi.Graph(self.csr)
        self.src = np.arange(V, dtype=np.uint32)
        self.q = self.query()
        self.objs = []

    def _csr(self):
        ov = np.zeros(self.V, dtype=np.uint8)
        ov[sorted(self.drained)] = 1
        return abi.Csr.from_links(self.V, self.links, ov)

    def query(self):
        return self.g.query(self.src, abi.SPF_F_NEXTHOPS).run()

    def table(self, ann, lfa, q=None, selected=None):
        t = abi.RouteTable(q or self.q, ann, abi.SPF_RT_LFA if lfa else 0, selected).run()
        self.objs.append(t)
        return t

    def change(self, metrics=None, drain=(), undrain=(), screen=None, lfa=False):
        """Apply {link index: (metric u->v, metric v->u)} and the drain changes
        to the graph in place.  With `screen` (the query whose resident rows
        describe the graph before) returns the affected rows -- None (every
        row) when a transit bit flipped -- closed over what LFA cells read."""
        old = self.csr
        for i, (a, b) in (metrics or {}).items():
            u, v, _, _ = self.links[i]
            self.links[i] = (u, v, a, b)
        self.drained = (self.drained | set(drain)) - set(undrain)
        new = self._csr()
        assert np.array_equal(old.row_ptr, new.row_ptr) and np.array_equal(old.col, new.col)
        rows = None
        if screen is not None and np.array_equal(old.overloaded, new.overloaded):
            deltas = abi.graph_diff(old, new)
            hit = np.zeros(self.V, dtype=bool)
            if len(deltas):
                dp, eb, _, _ = screen.device_rows()
                assert eb == 4
                pitch = abi.load().spf_query_row_stride(screen.h)
                hit = self.g.table_screen(dp, pitch, self.src, deltas).astype(bool)
            if lfa:
                base = hit.copy()
                for u, v, _, _ in self.links:
                    hit[u] |= base[v]
                    hit[v] |= base[u]
                hit[[int(d["tail"]) for d in deltas]] = True
            rows = np.flatnonzero(hit).astype(np.uint32)
        e = np.flatnonzero(old.metric != new.metric)
        if len(e):
            self.g.patch_metrics(e, new.metric[e])
        if not np.array_equal(old.overloaded, new.overloaded):
            self.g.set_transit(new.overloaded)
        self.csr = new
        return rows

    def close(self):
        for t in self.objs:
            t.close()
        self.g.close()


def rule_bits(before, after, routes_only=False, rows=None):
    """[V, P] bool by the cell rule of spf_route_table_diff, listed rows only."""
    P = len(before[0][0])
    out = np.zeros((len(before), P), dtype=bool)
    for i, ((om, ob, ow, ol), (nm, nb, nw, nl)) in enumerate(zip(before, after)):
        if rows is not None and i not in rows:
            continue
        for c in range(P):
            if (om[c] == INF) != (nm[c] == INF):
                out[i, c] = True
            elif om[c] != INF:
                ch = (om[c] != nm[c] and not routes_only) or ob[c] != nb[c]
                ch = ch or not np.array_equal(ow[c], nw[c])
                out[i, c] = ch or (ol is not None and not np.array_equal(ol[c], nl[c]))
    return out


def bitmaps(net, t):
    return np.array([t.changed(i) for i in range(net.V)])


def check_prev(net, t, before):
    """fetch_cells_prev of every (row, column) against the snapshot `before`."""
    rr = np.repeat(np.arange(net.V), t.P)
    cc = np.tile(np.arange(t.P), net.V)
    gm, gb, gl, glm = t.fetch_cells_prev(rr, cc, net.degs)
    assert gm.tolist() == np.concatenate([r[0] for r in before]).tolist()
    assert gb.tolist() == np.concatenate([r[1] for r in before]).tolist()
    assert gl.tolist() == np.concatenate([r[2].reshape(-1) for r in before]).tolist()
    if t.lfa:
        assert glm.tolist() == np.concatenate([r[3].reshape(-1) for r in before]).tolist()


def check_refresh(net, ann, lfa, screened, routes_only=False, **event):
    """A fresh table of `ann` follows `event` by refresh_rows over a new query;
    every ground truth of the module docstring.  Returns (table, counts, bits,
    rows before, rows after, listed rows)."""
    t = net.table(ann, lfa)
    older = net.table(ann, lfa)
    if routes_only:
        t.diff_routes(True)
    before = snapshot(net, t)
    q_old = net.q
    rows = net.change(screen=q_old if screened else None, lfa=lfa, **event)
    net.q = net.query()
    counts = t.refresh_rows(net.q, rows)
    assert t.refresh_ms() >= 0.0
    after = snapshot(net, t)
    fresh = net.table(ann, lfa)
    if routes_only:
        fresh.diff_routes(True)
    assert same(after, snapshot(net, fresh))
    want_counts = fresh.diff(older)
    older.close()
    bits = bitmaps(net, fresh)
    assert np.array_equal(bits, rule_bits(before, after, routes_only))
    assert counts.tolist() == want_counts.tolist() == bits.sum(axis=1).tolist()
    if rows is not None:
        assert not bits[[i for i in range(net.V) if i not in rows]].any()
    check_after_patch(net, t, after, bits)
    check_prev(net, t, before)
    # the binding moved: the old query goes, the new one stays while t lives
    assert abi.load().spf_query_destroy(q_old.h) == abi.SPF_OK
    q_old.h = None
    assert abi.load().spf_query_destroy(net.q.h) == SPF_E_INVALID
    assert same(snapshot(net, t.run()), after)
    return t, counts, bits, before, after, rows


def fresh_rows(net, ann, lfa):
    """The rows of a fresh table over the current query (closed again: it
    would keep the query alive)."""
    f = abi.RouteTable(net.q, ann, abi.SPF_RT_LFA if lfa else 0).run()
    try:
        return snapshot(net, f)
    finally:
        f.close()


def mixed_net():
    return TNet(MIXED_V, mixed_links(), DRAINED)


def mixed_ann(P, seed):
    """Seeded lists with the announcers the events below move: 3 (reached from
    0 over 1 - 2 at cost 9 and over the chord at 10), 11 (the island), 5."""
    ann = seeded_lists(P, MIXED_V, seed)
    ann[1], ann[2], ann[5] = [3], [11], [5]
    return ann


EVENTS = {
    # link 0 is 0 - 1 (2 / 2): the only way between them that passes no drained node
    "raise_tight": dict(metrics={0: (9, 9)}),
    # the chord 0 -> 5 from 3 to 2: 0 reaches 3 over the chord at 9 as well
    "lower_to_ecmp": dict(metrics={10: (2, 4)}),
    "one_direction": dict(metrics={1: (7, 2)}),
    "island": dict(metrics={11: (5, 1)}),
    "drain": dict(drain=[1]),
    "undrain": dict(undrain=[3]),
    "metric_and_drain": dict(metrics={8: (1, 6)}, drain=[9]),
}


@pytest.mark.parametrize("screened", [False, True])
@pytest.mark.parametrize("lfa", [False, True])
@pytest.mark.parametrize("P", [63, 64, 65, 130])
def test_word_edges(gpu_ready, P, lfa, screened):
    net = mixed_net()
    try:
        _, counts, _, _, _, _ = check_refresh(net, mixed_ann(P, P), lfa, screened,
                                              **EVENTS["raise_tight"])
        assert counts.sum() > 0
    finally:
        net.close()


@pytest.mark.parametrize("screened", [False, True])
@pytest.mark.parametrize("lfa", [False, True])
@pytest.mark.parametrize("event", sorted(EVENTS))
def test_events(gpu_ready, event, lfa, screened):
    net = mixed_net()
    try:
        _, counts, bits, before, after, rows = check_refresh(net, mixed_ann(65, 7), lfa, screened,
                                                             **EVENTS[event])
        assert counts.sum() > 0
        if event == "lower_to_ecmp" and not lfa:
            pop = lambda w: bin(int(w[0])).count("1")
            assert pop(before[0][2][1]) == 1 and pop(after[0][2][1]) == 2 and bits[0, 1]
        if event == "island":
            assert bits[10, 2] and not bits[:10].any()
            assert rows is None or set(rows.tolist()) <= {10, 11}
        if event in ("drain", "undrain", "metric_and_drain"):
            assert rows is None  # a transit bit flipped: every row
    finally:
        net.close()


@pytest.mark.parametrize("lfa", [False, True])
def test_no_change_rerun_and_refresh(gpu_ready, lfa):
    """The table's own query re-run: zero bits, cells untouched, binding kept."""
    net = mixed_net()
    try:
        t = net.table(mixed_ann(65, 3), lfa)
        before = snapshot(net, t)
        net.q.run()
        for rows in (None, [], [4, 12]):
            counts = t.refresh_rows(net.q, rows)
            assert not counts.any() and same(snapshot(net, t), before)
            check_after_patch(net, t, before, np.zeros((net.V, 65), dtype=bool))
            check_prev(net, t, before)
        assert abi.load().spf_query_destroy(net.q.h) == SPF_E_INVALID
    finally:
        net.close()


def test_diff_routes_leaves_the_metric_word_out(gpu_ready):
    """s = 0 reaches x = 2 over D = 1 (1 + 1) or over y = 3 (2 + 2).  Draining D
    raises d(s, x) from 2 to 4, yet both links of s keep their bits and their
    own metrics: the metric word moves and, with diff_routes, the bit stays clear."""
    links = [(0, 1, 1, 1), (1, 2, 1, 1), (0, 3, 2, 2), (3, 2, 2, 2)]
    for routes_only in (False, True):
        net = TNet(4, links)
        try:
            t, counts, bits, before, after, _ = check_refresh(net, [[2]], True, False, routes_only,
                                                              drain=[1])
            assert before[0][0][0] == 2 and after[0][0][0] == 4
            assert np.array_equal(before[0][2], after[0][2]) and np.array_equal(before[0][3], after[0][3])
            assert bits[0, 0] == (not routes_only) and counts[0] == (0 if routes_only else 1)
        finally:
            net.close()


@pytest.mark.parametrize("lfa", [False, True])
def test_strict_subset_of_the_affected_rows(gpu_ready, lfa):
    """Listed rows equal the fresh table; unlisted rows are bit-identical to
    before and their bitmap words are zero."""
    net = mixed_net()
    try:
        ann = mixed_ann(130, 11)
        t = net.table(ann, lfa)
        before = snapshot(net, t)
        q_old = net.q
        affected = net.change(screen=q_old, lfa=lfa, **EVENTS["raise_tight"])
        assert len(affected) >= 3
        listed = affected[::2][::-1].copy()  # a strict subset, not ascending
        net.q = net.query()
        counts = t.refresh_rows(net.q, listed)
        after = snapshot(net, t)
        want = fresh_rows(net, ann, lfa)
        for i in range(net.V):
            ref = want if i in listed else before
            assert same([after[i]], [ref[i]]), i
        bits = rule_bits(before, after, rows=set(listed.tolist()))
        assert np.array_equal(bitmaps(net, t), bits) and bits.any()
        assert counts.tolist() == bits.sum(axis=1).tolist()
        assert not bits[[i for i in range(net.V) if i not in listed]].any()
        check_after_patch(net, t, after, bits)
        check_prev(net, t, before)
    finally:
        net.close()


def grid_links(n, metric):
    at = lambda r, c: r * n + c
    out = []
    for r in range(n):
        for c in range(n):
            if c + 1 < n:
                out.append((at(r, c), at(r, c + 1), metric, metric))
            if r + 1 < n:
                out.append((at(r, c), at(r + 1, c), metric, metric))
    return out


def test_plan_change_needs_a_new_query(gpu_ready):
    """6 x 6 grid with one uniform metric: a patched metric ends the uniform
    plan, the way back starts it again; a new query each time."""
    net = TNet(36, grid_links(6, 5))
    try:
        ann = seeded_lists(70, 36, 2)
        t = net.table(ann, False)
        for metrics in ({7: (9, 5)}, {7: (5, 5)}):
            before = snapshot(net, t)
            q_old = net.q
            net.change(metrics=metrics)
            net.q = net.query()
            assert q_old.kernel != net.q.kernel
            counts = t.refresh_rows(net.q)
            after = snapshot(net, t)
            assert same(after, fresh_rows(net, ann, False))
            bits = rule_bits(before, after)
            assert counts.tolist() == bits.sum(axis=1).tolist() and bits.any()
            check_prev(net, t, before)
            assert abi.load().spf_query_destroy(q_old.h) == abi.SPF_OK
            q_old.h = None
    finally:
        net.close()


def hub_links(leaves):
    return [(0, 1 + i, 2 + i % 3, 3) for i in range(leaves)]


def test_hub_row_one_past_the_stage(gpu_ready):
    """1,030 links at the hub: the unstaged path of the cell.  LFA tables
    refuse such a row at creation, before and after this change alike."""
    net = TNet(1031, hub_links(1030))
    try:
        assert net.degs[0] == 1030
        ann = seeded_lists(65, 1031, 4)
        ann[0], ann[64] = [17], [0, 900]
        t = net.table(ann, False)
        older = net.table(ann, False)
        before0 = snapshot_row(net, t, 0)
        net.change(metrics={16: (40, 3)})  # the link 0 - 17
        q_old, net.q = net.q, net.query()
        counts = t.refresh_rows(net.q)
        fresh = net.table(ann, False)
        assert counts.tolist() == fresh.diff(older).tolist()
        older.close()
        for i in (0, 17, 18, 900, 1030):
            assert same([snapshot_row(net, t, i)], [snapshot_row(net, fresh, i)])
        after0 = snapshot_row(net, t, 0)
        assert counts[0] == rule_bits([before0], [after0]).sum() > 0 and counts.sum() > counts[0]
        assert not t.diff(fresh).any()  # every cell of every row
        assert abi.load().spf_query_destroy(q_old.h) == abi.SPF_OK
        q_old.h = None
        with pytest.raises(abi.SpfError):
            abi.RouteTable(net.q, ann, abi.SPF_RT_LFA)
    finally:
        net.close()


def snapshot_row(net, t, i):
    m, b, w = t.fetch(i)
    W = t.link_words(i)
    return (np.array(m[: t.P]), np.array(b[: t.P]), np.array(w[: t.P * W]).reshape(t.P, W), None)


@pytest.mark.parametrize("lfa", [False, True])
def test_after_a_refresh(gpu_ready, lfa):
    """patch_columns on the refreshed table equals a fresh table with both
    changes and its bitmap replaces the refresh's; a second refresh replaces
    the first one's previous cells; a pack taken before a refresh is stale."""
    net = mixed_net()
    try:
        ann = mixed_ann(70, 1)
        t = net.table(ann, lfa)
        t.patch_columns([4], [[2, 6]])
        ann[4] = [2, 6]
        z = abi._RouteDeltaSizes()
        assert abi.load().spf_route_table_delta_pack(t.h, C.byref(z)) == abi.SPF_OK
        net.change(**EVENTS["raise_tight"])
        q0, net.q = net.q, net.query()
        assert t.refresh_rows(net.q).sum() > 0
        q0.close()
        with pytest.raises(abi.SpfError):
            t.delta_fetch(z)
        mid = snapshot(net, t)
        counts = t.patch_columns([40, 66], [[5, 9], [1]])
        ann[40], ann[66] = [5, 9], [1]
        after = snapshot(net, t)
        assert same(after, fresh_rows(net, ann, lfa))
        bits = rule_bits(mid, after)
        assert not bits[:, [c for c in range(70) if c not in (40, 66)]].any() and bits.any()
        assert counts.tolist() == bits.sum(axis=1).tolist()
        check_after_patch(net, t, after, bits)
        # the patch ended the refresh's previous cells
        one = np.zeros(1, dtype=np.uint32)
        out = np.zeros(8, dtype=np.uint32)
        lk = np.zeros(8, dtype=np.uint64)
        p32 = lambda a: abi._p(a, C.c_uint32)
        prev = lambda: abi.load().spf_route_table_fetch_cells_prev(
            t.h, 1, p32(one), p32(one), p32(out), p32(out), abi._p(lk, C.c_uint64), p32(out))
        assert prev() == SPF_E_INVALID
        # a second and a third refresh: each one's previous cells are its own
        for event in ("drain", "island"):
            before = snapshot(net, t)
            net.change(**EVENTS[event])
            q0, net.q = net.q, net.query()
            counts = t.refresh_rows(net.q)
            q0.close()
            now = snapshot(net, t)
            assert same(now, fresh_rows(net, ann, lfa))
            assert counts.tolist() == rule_bits(before, now).sum(axis=1).tolist() and counts.any()
            check_prev(net, t, before)
        t.run()
        assert prev() == SPF_E_INVALID and same(snapshot(net, t), now)
    finally:
        net.close()


def test_lifetime_follows_the_binding(gpu_ready):
    lib = abi.load()
    net = mixed_net()
    try:
        t = net.table(mixed_ann(10, 2), False)
        q0, q1 = net.q, net.query()
        assert lib.spf_query_destroy(q0.h) == SPF_E_INVALID
        assert lib.spf_query_destroy(q1.h) == abi.SPF_OK
        q1.h = None
        q1 = net.query()
        t.refresh_rows(q1, [])  # no rows: the binding moves all the same
        assert lib.spf_query_destroy(q0.h) == abi.SPF_OK
        q0.h = None
        assert lib.spf_query_destroy(q1.h) == SPF_E_INVALID
        t.close()
        assert lib.spf_query_destroy(q1.h) == abi.SPF_OK
        q1.h = None
    finally:
        net.close()


@pytest.mark.parametrize("lfa", [False, True])
def test_rejected_inputs_leave_the_table_as_it_was(gpu_ready, lfa):
    lib = abi.load()
    V = MIXED_V
    net = mixed_net()
    other = mixed_net()
    try:
        ann = mixed_ann(70, 6)
        flags = abi.SPF_RT_LFA if lfa else 0
        q0 = net.q
        t = net.table(ann, lfa)
        before = snapshot(net, t)
        t.patch_columns([2, 65], [[1], [4, 8]])
        ann[2], ann[65] = [1], [4, 8]
        rows = snapshot(net, t)
        bits = rule_bits(before, rows)
        pk = check_after_patch(net, t, rows, bits)
        assert bits.any()
        z = abi._RouteDeltaSizes()
        assert lib.spf_route_table_delta_pack(t.h, C.byref(z)) == abi.SPF_OK

        def raw(tab, q, n, lst):
            a = None if lst is None else np.asarray(lst if len(lst) else [0], dtype=np.uint32)
            out = np.zeros(V, dtype=np.uint32)
            return lib.spf_route_table_refresh_rows(
                tab.h if tab else None, q.h if q else None, n,
                abi._p(a, C.c_uint32) if a is not None else None, abi._p(out, C.c_uint32))

        idle = abi.RouteTable(q0, ann, flags)  # has not run
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
        sel = net.table([[1], [2, 4], [], [8]], lfa, selected={3: ([], [1])})
        sel_rows = snapshot(net, sel)
        assert raw(sel, good, 0, None) == SPF_E_UNSUPPORTED
        assert same(snapshot(net, sel), sel_rows)
        for k, call in enumerate(invalid):
            assert call() == SPF_E_INVALID, k
            assert same(snapshot(net, t), rows), k
            assert np.array_equal(bitmaps(net, t), bits), k
            assert t.delta_fetch(z)["col"].tolist() == pk["col"].tolist(), k  # the pack is still good
            assert lib.spf_query_destroy(q0.h) == SPF_E_INVALID, k  # and so is the binding
        for q in (unrun, fewer, swapped, no_nh, unit, ign, good):
            assert lib.spf_query_destroy(q.h) == abi.SPF_OK
            q.h = None
        # 64-bit rows (a metric past 2^31 on the graph): SPF_E_UNSUPPORTED
        net.change(metrics={4: (3_000_000_000, 3)})
        wide = net.g.query(net.src, abi.SPF_F_NEXTHOPS).run()
        assert wide.device_rows()[1] == 8
        assert raw(t, wide, 0, None) == SPF_E_UNSUPPORTED
        assert np.array_equal(bitmaps(net, t), bits)
        assert lib.spf_query_destroy(q0.h) == SPF_E_INVALID
        wide.close()
        # no refresh ran: no previous cells
        with pytest.raises(abi.SpfError):
            t.fetch_cells_prev([0], [0], net.degs)
    finally:
        other.close()
        net.close()
