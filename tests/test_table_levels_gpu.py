"""SPF_T_GATHER_LEVELS: all-sources tables exchanged as 8-bit level rows on a
uniform metric (include/openr_spf.h), expanded back to uint32 rows by
spf_levels_expand_kernel.  Every reader must return the rows of the plain
query and of the CPU oracle bit for bit, in both forms a run can take:
"levels" (no BFS level reached 255) and the "rows32" fallback.

All comparisons are exact and cover every row.  The oracle rows of a graph
are computed once per module and shared.
"""

import ctypes as C
import functools
import types

import numpy as np
import pytest

from openr_amd import abi
from oracle import spf_py

INF32 = 0xFFFFFFFF
NH = abi.SPF_F_NEXTHOPS
LV = abi.SPF_T_GATHER_LEVELS


def _oracle_rows(csr, sources, use_link_metric=True):
    # the oracle indexes the CSR element by element: plain lists, not numpy
    # scalars, keep its pure-Python loops quick
    lists = types.SimpleNamespace(
        row_ptr=csr.row_ptr.tolist(), col=csr.col.tolist(), metric=csr.metric.tolist(),
        link_id=csr.link_id.tolist(), overloaded=csr.overloaded.tolist())
    rows = np.full((len(sources), csr.num_nodes), INF32, dtype=np.uint32)
    for i, s in enumerate(sources):
        for v, r in spf_py.run_spf(lists, int(s), use_link_metric).items():
            rows[i, v] = r[0]
    return rows


def _island_links(V, seed, metric):
    """A random connected graph on the first V - k nodes and a k-node island
    (a ring of its own) that no link of the rest reaches; k = 20, or V // 4
    on a graph too small for 20.  metric: an int, or None for random ones."""
    rng = np.random.default_rng(seed)
    k = min(20, V // 4)
    m = V - k
    w = (lambda: metric) if metric else (lambda: int(rng.integers(1, 20)))
    links = [(int(rng.integers(0, v)), v, w(), w()) for v in range(1, m)]
    for _ in range(m // 8):
        a, b = (int(x) for x in rng.integers(0, m, size=2))
        if a != b:
            links.append((a, b, w(), w()))
    for j in range(k):
        if k > 2 or j == 0:
            links.append((m + j, m + (j + 1) % k, w(), w()))
    ov = (rng.random(V) < 0.05).astype(np.uint8)
    return abi.Csr.from_links(V, links, ov)


@functools.lru_cache(maxsize=None)
def _parity_case(V, unit):
    csr = _island_links(V, 100 + V + unit, None if unit else 7)
    sources = np.arange(0, V, 7, dtype=np.uint32)
    return csr, sources, _oracle_rows(csr, sources, not unit)


def _path_csr(V, metric, drained=()):
    ov = np.zeros(V, dtype=np.uint8)
    ov[list(drained)] = 1
    return abi.Csr.from_links(V, [(v, v + 1, metric, metric) for v in range(V - 1)], ov)


@functools.lru_cache(maxsize=None)
def _path_rows(V, metric, drained=()):
    return _oracle_rows(_path_csr(V, metric, drained), range(V))


def _cluster(mode):
    if mode == "local":
        return abi.Cluster([0])
    return abi.Cluster(world=1, rank=0, uid=abi.cluster_unique_id(), device=0)


def _query_rows(g, sources, flags):
    q = g.query(sources, flags).run()
    rows = np.empty((len(sources), g.V), dtype=np.uint32)
    q.fetch_rows(0, len(sources), rows.ctypes.data, g.V * 4, on_device=False)
    masks = q.fetch_nexthops(0, len(sources)) if flags & NH else None
    q.close()
    return rows, masks


def _check_levels_table(t, csr, sources, ref, qflags, scale):
    """Every reader of a table in levels form against the oracle rows."""
    n, V = len(sources), csr.num_nodes
    form, sc, gathered = t.row_form()
    assert (form, sc) == ("levels", scale)
    pitch, slot_bytes, _ = t.levels_layout()
    assert gathered == t.cluster.world * slot_bytes
    assert t.levels_buffer(0) == (t.levels_buffer(0)[0], pitch, slot_bytes) and t.levels_buffer(0)[0]
    assert t.device_buffers(0)[0] is None
    exp = t.expand_rows(0, n)
    assert (exp == ref).all()
    assert (t.fetch_rows(0, n) == ref).all()
    if n > 4:
        lo, cnt = 3, min(n - 3, 5)  # a sub-range starting at an odd row
        assert (t.expand_rows(lo, cnt) == ref[lo : lo + cnt]).all()
        assert (t.expand_rows(n - 1, 1) == ref[n - 1 :]).all()
    lv = t.fetch_levels(0, n)
    assert lv.shape == (n, V) and lv.dtype == np.uint8
    assert ((lv == 255) == (ref == INF32)).all()
    assert (np.where(lv == 255, INF32, lv.astype(np.uint64) * scale) == ref).all()
    g = abi.Graph(csr)
    rows, masks = _query_rows(g, sources, qflags)
    g.close()
    assert (rows == ref).all()
    assert (t.fetch_nexthops(0, n) == masks).all()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["local", "rank"])
@pytest.mark.parametrize("V", [17, 1003, 3000])
def test_levels_parity_awkward_shapes(gpu_ready, V, mode):
    """Uniform metric 7, an unreachable island, drained nodes, a source count
    that is no multiple of 64; V = 1003 makes the 4V-byte rows of expand_rows
    4-byte aligned only (the kernel's scalar-store path), V = 17 is below one
    16-byte level pitch, V = 3000 takes three chunks per row."""
    csr, sources, ref = _parity_case(V, False)
    assert len(sources) % 64 != 0
    c = _cluster(mode)
    t = abi.Table(c, csr, sources, NH | LV | abi.SPF_T_GATHER_NEXTHOPS).run()
    assert t.kernel(0) == "msbfs+levels"
    _check_levels_table(t, csr, sources, ref, NH, 7)
    assert t.device_buffers(0)[1]  # the masks are gathered as before
    t.close()
    c.close()


@pytest.mark.gpu
def test_levels_parity_unit_metric(gpu_ready):
    """Random metrics with SPF_F_UNIT_METRIC: hop counts, scale 1."""
    csr, sources, ref = _parity_case(1003, True)
    assert len(set(csr.metric.tolist())) > 1
    c = _cluster("local")
    flags = NH | abi.SPF_F_UNIT_METRIC
    t = abi.Table(c, csr, sources, flags | LV | abi.SPF_T_GATHER_NEXTHOPS).run()
    _check_levels_table(t, csr, sources, ref, flags, 1)
    t.close()
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("offset,pad", [(4, 32), (16, 36)])
def test_levels_expand_no_overrun(gpu_ready, offset, pad):
    """spf_table_expand_rows into the middle of a sentinel-filled buffer:
    pitch 4V + 32 from a base 4 bytes off (4-byte stores), and a 16-byte
    aligned base and pitch (uint4 stores, V % 4 != 0 so every row ends in a
    partial group).  The gap words between rows and everything before and
    after the range keep the sentinel."""
    import torch

    csr, sources, ref = _parity_case(1003, False)
    V, n = csr.num_nodes, len(sources)
    pitch = 4 * V + pad
    assert pitch % 4 == 0 and (pitch % 16 == 0) == (offset % 16 == 0)
    c = _cluster("local")
    t = abi.Table(c, csr, sources, NH | LV).run()
    assert t.row_form()[0] == "levels"
    first, count = 5, n - 9
    words = (offset + count * pitch) // 4 + 64
    sent = 0xDEADBEEF
    buf = torch.from_numpy(np.full(words, sent, dtype=np.uint32)).cuda()
    assert buf.data_ptr() % 16 == 0
    st = abi.load().spf_table_expand_rows(t.h, 0, first, count, C.c_void_p(buf.data_ptr() + offset), pitch)
    assert st == abi.SPF_OK
    t.sync()
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    o, p = offset // 4, pitch // 4
    assert (got[:o] == sent).all()
    body = got[o : o + count * p].reshape(count, p)
    assert (body[:, :V] == ref[first : first + count]).all()
    # (the last row's gap belongs to the tail check below)
    assert (body[:-1, V:] == sent).all()
    assert (got[o + (count - 1) * p + V :] == sent).all()
    t.close()
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("V", [255, 256])
def test_levels_boundary_254_255(gpu_ready, V):
    """A path of V nodes, metric 3, every node a source: the largest level is
    V - 1.  254 still fits a level byte; at 255 the byte is the unreached
    mark, so the run falls back to uint32 rows."""
    csr, ref = _path_csr(V, 3), _path_rows(V, 3)
    assert int(ref.max()) == 3 * (V - 1)
    sources = np.arange(V, dtype=np.uint32)
    c = _cluster("local")
    t = abi.Table(c, csr, sources, NH | LV).run()
    lib = abi.load()
    if V == 255:
        _check_levels_table(t, csr, sources, ref, NH, 3)
        assert int(t.fetch_levels(0, 1).max()) == 254
    else:
        form, _, gathered = t.row_form()
        assert form == "rows32"
        _, slot_bytes, _ = t.levels_layout()
        assert gathered == slot_bytes + V * V * 4  # the level exchange, then the fallback's
        out = np.zeros((V, V), dtype=np.uint8)
        assert lib.spf_table_fetch_levels(t.h, 0, V, out.ctypes.data_as(C.POINTER(C.c_uint8))) == \
            abi.SPF_E_UNSUPPORTED
        with pytest.raises(abi.SpfError):
            t.fetch_levels(0, V)
        assert (t.expand_rows(0, V) == ref).all()
        assert (t.expand_rows(3, 7) == ref[3:10]).all()
        assert (t.fetch_rows(0, V) == ref).all()
        assert t.device_buffers(0)[0]
        compute, gather = t.elapsed_ms()
        assert compute > 0 and gather > 0
    t.close()
    c.close()


@pytest.mark.gpu
def test_levels_form_follows_drains(gpu_ready):
    """The form is decided per run: a 300-node path is deep (rows32), with
    node 100 drained no level passes 199 (levels), undrained it is deep
    again."""
    V, w = 300, 5
    sources = np.arange(V, dtype=np.uint32)
    c = _cluster("local")
    cg = abi.ClusterGraph(c, _path_csr(V, w))
    t = cg.table(sources, NH, gather=LV)
    for drained, want in (((), "rows32"), ((100,), "levels"), ((), "rows32")):
        ov = np.zeros(V, dtype=np.uint8)
        ov[list(drained)] = 1
        cg.set_transit(ov)
        t.run()
        ref = _path_rows(V, w, drained)
        assert t.row_form()[0] == want, drained
        assert (t.expand_rows(0, V) == ref).all(), drained
        assert (t.fetch_rows(0, V) == ref).all(), drained
        if want == "levels":
            assert t.row_form()[1] == w
            lv = t.fetch_levels(0, V)
            assert (np.where(lv == 255, INF32, lv.astype(np.uint64) * w) == ref).all()
            assert int(lv[lv != 255].max()) == 199
    t.close()
    cg.close()
    c.close()


def _create(c, csr, sources, flags):
    d, keep = abi._graph_desc(csr, 0)
    src = np.ascontiguousarray(sources, dtype=np.uint32)
    h = C.c_void_p()
    st = abi.load().spf_table_create(c.h, C.byref(d), len(src), src.ctypes.data_as(C.POINTER(C.c_uint32)),
                                     flags, C.byref(h))
    return st, h


@pytest.mark.gpu
def test_levels_refusals(gpu_ready):
    lib = abi.load()
    csr, sources, ref = _parity_case(1003, False)
    wcsr = _parity_case(1003, True)[0]  # random metrics
    V, n = csr.num_nodes, len(sources)
    c = _cluster("local")
    # both row gathers at once
    assert _create(c, csr, sources, NH | LV | abi.SPF_T_GATHER_ROWS)[0] == abi.SPF_E_INVALID
    # a metric that is not uniform, without SPF_F_UNIT_METRIC: no level rows, ever
    assert _create(c, wcsr, sources, NH | LV)[0] == abi.SPF_E_UNSUPPORTED
    st, h = _create(c, wcsr, sources, NH | LV | abi.SPF_F_UNIT_METRIC)  # hop counts are uniform
    assert st == abi.SPF_OK and lib.spf_table_destroy(h) == abi.SPF_OK
    cg = abi.ClusterGraph(c, wcsr)
    with pytest.raises(abi.SpfError):
        cg.table(sources, NH, gather=LV)
    cg.close()
    # the new calls before the first run, and bad arguments after it
    st, h = _create(c, csr, sources, NH | LV)
    assert st == abi.SPF_OK
    f, s, b = C.c_uint32(), C.c_uint32(), C.c_uint64()
    lv = np.zeros((n, V), dtype=np.uint8)
    plv = lv.ctypes.data_as(C.POINTER(C.c_uint8))
    dbuf = C.c_void_p()
    assert lib.spf_device_alloc(0, n * V * 4, C.byref(dbuf)) == abi.SPF_OK
    assert lib.spf_table_row_form(h, C.byref(f), C.byref(s), C.byref(b)) == abi.SPF_E_INVALID
    assert lib.spf_table_fetch_levels(h, 0, n, plv) == abi.SPF_E_INVALID
    assert lib.spf_table_expand_rows(h, 0, 0, n, dbuf, V * 4) == abi.SPF_E_INVALID
    assert lib.spf_table_run(h) == abi.SPF_OK and lib.spf_table_sync(h) == abi.SPF_OK
    assert lib.spf_table_row_form(h, C.byref(f), C.byref(s), C.byref(b)) == abi.SPF_OK and f.value == 2
    assert lib.spf_table_row_form(None, C.byref(f), C.byref(s), C.byref(b)) == abi.SPF_E_INVALID
    assert lib.spf_table_fetch_levels(h, 0, n, None) == abi.SPF_E_INVALID
    assert lib.spf_table_fetch_levels(h, 1, n, plv) == abi.SPF_E_INVALID
    assert lib.spf_table_expand_rows(h, 0, 1, n, dbuf, V * 4) == abi.SPF_E_INVALID  # range
    assert lib.spf_table_expand_rows(h, 1, 0, n, dbuf, V * 4) == abi.SPF_E_INVALID  # local device
    assert lib.spf_table_expand_rows(h, 0, 0, n, None, V * 4) == abi.SPF_E_INVALID
    assert lib.spf_table_expand_rows(h, 0, 0, n, dbuf, V * 4 - 4) == abi.SPF_E_INVALID  # pitch < 4V
    assert lib.spf_table_expand_rows(h, 0, 0, 1, dbuf, V * 4 + 2) == abi.SPF_E_INVALID  # pitch % 4
    assert lib.spf_table_levels_buffer(h, 1, C.byref(dbuf), None, None) == abi.SPF_E_INVALID
    assert lib.spf_table_fetch_levels(h, 0, n, plv) == abi.SPF_OK
    assert lib.spf_table_destroy(h) == abi.SPF_OK
    assert lib.spf_device_free(0, dbuf) == abi.SPF_OK
    # tables without the flag: the form their flags say, the results they had
    t = abi.Table(c, csr, sources, NH).run()
    assert t.row_form() == ("none", 0, 0)
    assert t.levels_buffer(0)[0] is None
    assert (t.fetch_rows(0, n) == ref).all()
    with pytest.raises(abi.SpfError):
        t.expand_rows(0, n)  # nothing gathered
    with pytest.raises(abi.SpfError):
        t.fetch_levels(0, n)
    t.close()
    t = abi.Table(c, csr, sources, NH | abi.SPF_T_GATHER_ROWS).run()
    assert t.row_form() == ("rows32", 0, n * V * 4)
    assert t.device_buffers(0)[0] and t.levels_buffer(0)[0] is None
    assert (t.fetch_rows(0, n) == ref).all()
    assert (t.expand_rows(0, n) == ref).all()  # the strided copy of the uint32 gather
    with pytest.raises(abi.SpfError):
        t.fetch_levels(0, n)
    t.close()
    c.close()
