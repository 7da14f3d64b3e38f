"""The life of a query object across in-place graph changes (DESIGN.md §8,
include/openr_spf.h at spf_query_run).

spf_query_create fixes a query's plan; spf_graph_set_transit, _patch_metrics
and _set_edges then change the graph under it.  A re-run must either compute
exactly what a query created now would, or be refused as stale -- never wrong
rows.  Every cell below is (plan, change, expectation): the query is created
and run, the change is applied to the live graph, and rerun_or_stale proves
whichever side spf_query_stale chose:

  stale   run() raises "stale query", and the rows of the previous run are
          still readable and unchanged;
  fresh   the re-run equals, bit for bit, a new query on a NEW graph built from
          the changed CSR (links that are down removed), the plan names agree
          where the class is kept, and sampled rows equal the literal replay
          (oracle/spf_py.py).

A cell marked "reject" is never run unless stale() said 1, so a wrong predicate
fails an assert on the host instead of launching over freed or missing
buffers.  "accept" cells are run twice: change, re-run, change back, re-run.

Before spf_query_stale existed the cells marked WHY below returned, measured
on the engine as it was: a uniform metric that ends (M4) -- every distance 0
on msbfs, msbfs+levels, bfs and bfs+rows; the zero-metric plan's c -> c' (now
M3 on zero*, exact since the scale is read live) -- 195 of 200 rows wrong; a
metric past the packable width (M9b) -- the LDS-row plan was refused by an
internal guard and the packed pass read its pointer live, both right; a graph
that starts to need 64-bit rows (M6, T2) -- right rows at these shapes, where
no shortest path reaches the raised metric.  A neighbour that comes up without
a row (E6) indexes the row table with -1 and was not run.
"""

import copy
import functools
import random

import numpy as np
import pytest

from openr_amd import abi
from tests.test_abi_gpu import check_query, random_links
from tests.test_route_table_patch_gpu import same, seeded_lists, snapshot
from tests.test_route_table_refresh_gpu import EVENTS, TNet, mixed_ann, mixed_net

pytestmark = pytest.mark.gpu

NH = abi.SPF_F_NEXTHOPS
UNIT = abi.SPF_F_UNIT_METRIC

# (plan, code) -> "stale" | "ran", filled by the cells as they run
OUTCOME = {}


# ---------------------------------------------------------------- CSR helpers


def with_metric(csr, edges, metrics):
    c = copy.copy(csr)
    c.metric = csr.metric.copy()
    c.metric[np.asarray(edges, dtype=np.int64)] = np.asarray(metrics, dtype=np.uint64)
    return c


def with_drains(csr, ov):
    c = copy.copy(csr)
    c.overloaded = np.asarray(ov, dtype=np.uint8)
    return c


def without_halves(csr, down):
    """The CSR of the half-edges that are up (both halves of every down link
    listed), link ids and num_links kept, so ignore lists still name the same
    links."""
    E = len(csr.col)
    keep = np.ones(E, dtype=bool)
    keep[np.asarray(down, dtype=np.int64)] = False
    assert (keep == keep[csr.rev]).all(), "a fresh graph needs both halves of a link"
    new_idx = np.cumsum(keep) - 1
    tail = np.repeat(np.arange(csr.num_nodes), np.diff(csr.row_ptr.astype(np.int64)))
    row = np.zeros(csr.num_nodes + 1, dtype=np.int64)
    np.add.at(row, tail[keep] + 1, 1)
    return abi.Csr(csr.num_nodes, np.cumsum(row).astype(np.uint32), csr.col[keep].copy(),
                   csr.metric[keep].copy(), csr.link_id[keep].copy(),
                   new_idx[csr.rev[keep]].astype(np.uint32), csr.overloaded.copy(), csr.num_links)


def row_of(csr, s):
    return range(int(csr.row_ptr[s]), int(csr.row_ptr[s + 1]))


def links_to(csr, s):
    """{neighbour: [link ids]} of node s."""
    out = {}
    for e in row_of(csr, s):
        out.setdefault(int(csr.col[e]), []).append(int(csr.link_id[e]))
    return out


def halves(csr, link):
    h = np.flatnonzero(csr.link_id == link).astype(np.uint32)
    assert len(h) == 2
    return h


def width_class(nn):
    """Bytes per node of a source's next-hop masks (spf_query_nh_bytes)."""
    return 1 if nn <= 8 else 2 if nn <= 16 else 4 if nn <= 32 else 8 * ((nn + 63) // 64)


# ------------------------------------------------------------------- the plans


class Case:
    def __init__(self, csr, srcs, flags, plan, ign=None, env=None, kernels=(), wrange=None,
                 hub=None, hubdeg=9):
        self.csr, self.srcs, self.flags, self.plan = csr, [int(s) for s in srcs], flags, plan
        self.ign, self.env, self.kernels = ign, env or {}, kernels
        self.wrange = wrange  # metrics a class-keeping patch may draw from (None: uniform)
        self.hub, self.hubdeg = hub, hubdeg  # a source with exactly hubdeg neighbours, one link each


@functools.lru_cache(maxsize=None)
def net(seed, V, L, wmin, wmax, asym=True, parallel=0.03, hub=False, drained=0.02):
    """Seeded random graph (cached: nobody writes into its arrays); hub: node
    V - 1 gets exactly hub neighbours (True: 9; 0, 3, 6, ...), one link each,
    and nothing else."""
    rng = random.Random(seed)
    links = random_links(rng, V, L, wmin, wmax, parallel, asym)
    if hub:
        links = [l for l in links if V - 1 not in l[:2]]
        links += [(V - 1, 3 * k, wmin, wmin) for k in range(9 if hub is True else hub)]
    ov = np.zeros(V, dtype=np.uint8)
    ov[rng.sample(range(30, V - 1), int(V * drained))] = 1
    return abi.Csr.from_links(V, links, ov)


def p_lds(flags=NH, hub=9):
    csr = net(1, 300, 1200, 1, 20, hub=hub)
    return Case(csr, list(range(0, 299, 7)) + [299], flags, "lds", wrange=(1, 20), hub=299,
                hubdeg=hub)


def p_lds_rows():
    return Case(net(2, 250, 900, 1, 20, hub=True), range(250), NH, "lds+rows", wrange=(1, 20),
                hub=249)


def p_uniform300(flags=NH, msbfs=True, hub=9):
    csr = net(3, 300, 1000, 7, 7, asym=False, hub=hub)
    if msbfs:
        plan, k = ("msbfs+levels", ("spf_msbfs_kernel", "spf_nh_levels_v2_kernel")) \
            if flags & NH else ("msbfs", ("spf_msbfs_kernel",))
        return Case(csr, range(300), flags, plan, kernels=k, hub=299, hubdeg=hub)
    plan = "bfs+rows" if flags & NH else "bfs"
    return Case(csr, range(300), flags, plan, env={"OPENR_SPF_MSBFS": "0"},
                kernels=("spf_bfs_kernel",), hub=299)


def p_helpers():
    csr = net(4, 3001, 9000, 7, 7, asym=False, hub=True)
    # the block [0, 700) and the hub: their neighbours outside ride along as helper sources
    return Case(csr, list(range(700)) + [3000], NH, "msbfs+levels", kernels=("spf_msbfs_kernel",),
                hub=3000)


def p_big(kind):
    if kind == "bfs-gmem":
        csr = net(5, 40000, 120000, 7, 7, asym=False, parallel=0.0, drained=0.01)
        return Case(csr, [0, 777, 39998], 0, "bfs-gmem", kernels=("spf_bfs_kernel",))
    csr = net(6, 40000, 120000, 1, 300, parallel=0.02, drained=0.01)
    srcs = [0, 777, 39998]
    if kind == "dstep":
        return Case(csr, srcs, NH, "dstep", wrange=(1, 300), kernels=("spf_dstep_kernel",))
    if kind == "dstep-ldsrow":
        return Case(csr, srcs, 0, "dstep-ldsrow", wrange=(1, 300), kernels=("spf_dlds_kernel",))
    assert kind == "gmem"
    return Case(csr, srcs, NH, "gmem", wrange=(1, 300), env={"OPENR_SPF_DSTEP": "0"})


def p_packed_dstep():
    """Distances only past the LDS-row range (a metric above 4,094): the
    packed push-only delta-stepping pass alone."""
    csr = net(7, 40000, 120000, 1, 5000, parallel=0.02, drained=0.01)
    assert int(csr.metric.max()) > 4094
    return Case(csr, [0, 777, 39998], 0, "dstep", wrange=(1, 5000), kernels=("spf_dstep_kernel",))


def p_few_rows():
    csr = net(8, 5000, 15000, 1, 300, hub=True)
    return Case(csr, [3, 2500, 4999], NH, "dstep-ldsrow", wrange=(1, 300), hub=4999,
                kernels=("spf_dlds_kernel", "spf_nh_rows_kernel"))


def p_wide():
    return Case(net(9, 150, 500, 0, 5), range(0, 150, 5), NH, "wide", wrange=(1, 5))


def p_exact():
    csr = net(10, 50, 160, 1, 10)
    e = int(csr.row_ptr[3])  # one half-edge wraps: an i32 metric of -5
    return Case(with_metric(csr, [e], [(1 << 64) - 5]), range(0, 50, 3), NH, "exact",
                wrange=(1, 10))


def p_zero(nz, flags=NH):
    """Uniform 7 with nz metric-0 links on disjoint node pairs (one of them in
    one direction only)."""
    csr = net(11, 200, 700, 7, 7, asym=False, parallel=0.0)
    used, zero = set(), []
    for l in range(csr.num_links):
        h = halves(csr, l)
        u, v = int(csr.col[h[0]]), int(csr.col[h[1]])
        if u not in used and v not in used and len(zero) < nz:
            used |= {u, v}
            zero.append(h if len(zero) != 1 else h[:1])
    e = np.concatenate(zero)
    plan = "msbfs0+levels" if flags & NH else "msbfs0"
    c = Case(with_metric(csr, e, np.zeros(len(e))), range(200), flags, plan,
             kernels=("spf_msbfs_kernel",))
    c.zero_nodes = used
    return c


def p_lds_uniform():
    """Two next-hop sources of a uniform graph past the small-area MS-BFS
    plan: one SSSP workgroup each, next hops inline."""
    return Case(net(12, 1500, 5000, 3, 3, asym=False, parallel=0.05), [5, 900], NH, "lds")


def p_msbfs_ign():
    rng = random.Random(12)
    csr = net(12, 1500, 5000, 3, 3, asym=False, parallel=0.05)
    srcs = [rng.randrange(1500) for _ in range(60)] + [7] * 70
    ign = [rng.sample(range(csr.num_links), rng.choice([0, 1, 3, 20, 200])) for _ in srcs]
    return Case(csr, srcs, 0, "msbfs", ign=ign, kernels=("spf_msbfs_kernel", "spf_ms_ign_kernel"))


def p_whatif_repair():
    """Single-link failures from repeated sources on a weighted graph: the
    screen and the repair SSSP."""
    rng = random.Random(13)
    csr = net(13, 2000, 6000, 1, 30)
    srcs = [0] * 300 + [int(np.flatnonzero(csr.overloaded)[0])] * 100 + [7] * 100
    ign = [[rng.randrange(csr.num_links)] for _ in srcs]
    ign[5], ign[6] = [csr.num_links + 3], []
    return Case(csr, srcs, NH, "lds", ign=ign, env={"OPENR_SPF_MSBFS_IGN": "0"}, wrange=(1, 30),
                kernels=("spf_whatif_screen_kernel", "spf_sssp_kernel"))


def p_whatif_source_links(unit=False):
    """Uniform metric, failures of the source's own links (the first-hop form)
    and of a source link plus another link (the pull / heavy kernel)."""
    rng = random.Random(14)
    csr = net(14, 1200, 4200, 3, 3, asym=False, parallel=0.0, hub=True)
    s = 1199
    sl = sorted(l for ls in links_to(csr, s).values() for l in ls)
    ign = [[l] for l in sl] + [sorted(rng.sample(sl, 2)) for _ in range(5)]
    ign += [sorted({l, rng.randrange(csr.num_links)}) for l in sl]
    ign.append(sorted(sl))
    return Case(csr, [s] * len(ign), NH | (UNIT if unit else 0), "lds", ign=ign, hub=s,
                env={"OPENR_SPF_MSBFS_IGN": "0"}, wrange=(1, 9) if unit else None,
                kernels=("spf_whatif_firsthop_kernel", "spf_whatif_screen_kernel"))


def p_msd():
    csr = net(15, 70000, 200000, 1, 300, parallel=0.02, drained=0.01)
    rng = random.Random(15)
    return Case(csr, [rng.randrange(70000) for _ in range(150)], 0, "msdstep", wrange=(1, 300),
                env={"OPENR_SPF_MSD": "1"}, kernels=("spf_msdstep_kernel",))


PLANS = {
    "lds": p_lds,
    "lds-dist": lambda: p_lds(0),
    "lds-unit": lambda: _unit(p_lds()),
    "lds+rows": p_lds_rows,
    "msbfs+levels": p_uniform300,
    "msbfs": lambda: p_uniform300(0),
    "msbfs+levels-unit": lambda: _unit(p_uniform300()),
    "helpers": p_helpers,
    "bfs+rows": lambda: p_uniform300(NH, msbfs=False),
    "bfs": lambda: p_uniform300(0, msbfs=False),
    "bfs-gmem": lambda: p_big("bfs-gmem"),
    "gmem": lambda: p_big("gmem"),
    "dstep": lambda: p_big("dstep"),
    "dstep-ldsrow": lambda: p_big("dstep-ldsrow"),
    "dstep-packed": p_packed_dstep,
    "few-rows": p_few_rows,
    "wide": p_wide,
    "exact": p_exact,
    "zero1": lambda: p_zero(1),
    "zero3": lambda: p_zero(3),
    "zero3-dist": lambda: p_zero(3, 0),
    "zero1-dist": lambda: p_zero(1, 0),
    "lds-uniform": p_lds_uniform,
    "lds-h17": lambda: p_lds(hub=17),
    "lds-h33": lambda: p_lds(hub=33),
    "lds-h65": lambda: p_lds(hub=65),
    "msbfs+levels-h65": lambda: p_uniform300(hub=65),
    "msbfs-ign": p_msbfs_ign,
    "whatif-repair": p_whatif_repair,
    "whatif-links": p_whatif_source_links,
    "whatif-links-unit": lambda: p_whatif_source_links(True),
    "msd": p_msd,
}

# the unit-metric twin of a weighted case lands on the BFS family: its plan
# string is asserted from this table
UNIT_PLAN = {"lds": "msbfs+levels", "msbfs+levels": "msbfs+levels"}  # (what-if: still "lds")


def _unit(c):
    if c.plan in UNIT_PLAN:
        c.plan, c.kernels = UNIT_PLAN[c.plan], ("spf_msbfs_kernel",)
    c.flags |= UNIT
    c.wrange = c.wrange or (1, 9)  # a unit-metric query survives any metric
    return c


# ----------------------------------------------------------------- the changes
#
# A change is (pre, steps): `pre` (or None) is applied to the graph before the
# query is created; each step is (apply(g), the CSR a fresh graph is built
# from afterwards).  The first step is the cell's change, the second puts the
# graph back.


def metric_steps(c, edges, metrics):
    edges = np.asarray(edges, dtype=np.uint32)
    new = with_metric(c.csr, edges, metrics)
    old = c.csr.metric[edges].copy()
    return None, [(lambda g: g.patch_metrics(edges, new.metric[edges]), new),
                  (lambda g: g.patch_metrics(edges, old), c.csr)]


def class_kept(c, n, seed):
    """n half-edges and new metrics of the case's own range that differ from
    the old ones (metric 0 and wrapping half-edges stay as they are)."""
    rng = random.Random(seed)
    lo, hi = c.wrange
    ok = np.flatnonzero((c.csr.metric != 0) & (c.csr.metric <= 0x7FFFFFFF))
    e = np.array(sorted(rng.sample(ok.tolist(), n)), dtype=np.uint32)
    m = [(int(c.csr.metric[x]) - lo + 1 + rng.randrange(hi - lo)) % (hi - lo + 1) + lo for x in e]
    assert all(int(c.csr.metric[x]) != y and lo <= y <= hi for x, y in zip(e, m))
    return e, m


def ch_T1(c):
    rng = random.Random(21)
    V = c.csr.num_nodes
    s = c.srcs[0]
    ov = c.csr.overloaded.copy()
    ov[rng.sample(range(V), max(2, V // 50))] = 1
    ov[s] = 1
    ov[int(c.csr.col[int(c.csr.row_ptr[s])])] = 1  # a neighbour of that source
    return None, [(lambda g: g.set_transit(ov), with_drains(c.csr, ov)),
                  (lambda g: g.set_transit(c.csr.overloaded), c.csr)]


def ch_M1(c):
    E = len(c.csr.col)
    n = min(6, E // 64)
    assert n >= 1 and n * 64 <= E  # the sparse path
    return metric_steps(c, *class_kept(c, n, 22))


def ch_M2(c):
    E = len(c.csr.col)
    n = E // 32
    assert n * 64 > E  # the full upload
    return metric_steps(c, *class_kept(c, n, 23))


def ch_M3(c):
    """Uniform c -> c' on every half-edge (metric-0 half-edges stay: M8)."""
    e = np.flatnonzero(c.csr.metric != 0)
    return metric_steps(c, e, np.full(len(e), int(c.csr.metric[e[0]]) + 2))


def ch_M4(c):
    e = int(c.csr.row_ptr[c.srcs[0]])
    return metric_steps(c, [e], [int(c.csr.metric[e]) + 1])


def ch_M5(c):
    e = np.arange(len(c.csr.col))
    return metric_steps(c, e, np.full(len(e), 5))


def ch_M6(c):
    """One metric raised to 2^31 - 1: no hop bound keeps the sums in 32 bits."""
    ok = np.flatnonzero((c.csr.metric != 0) & (c.csr.metric <= 0x7FFFFFFF))
    return metric_steps(c, [int(ok[len(ok) // 2])], [0x7FFFFFFF])


def ch_M7(c):
    """Metric 0 introduced; on a graph that has some, one of them removed."""
    z = np.flatnonzero(c.csr.metric == 0)
    if len(z):
        return metric_steps(c, [int(z[0])], [3])
    return metric_steps(c, [int(c.csr.row_ptr[c.srcs[0]])], [0])


def ch_M8b(c):
    """A fourth metric-0 link, disjoint from the three."""
    for l in range(c.csr.num_links):
        h = halves(c.csr, l)
        if not {int(c.csr.col[h[0]]), int(c.csr.col[h[1]])} & c.zero_nodes:
            return metric_steps(c, h, [0, 0])
    raise AssertionError("no disjoint link")


def ch_M8c(c):
    """A second nonzero value."""
    e = int(np.flatnonzero(c.csr.metric != 0)[5])
    return metric_steps(c, [e], [int(c.csr.metric[e]) + 1])


def ch_M9(c):
    e = int(c.csr.row_ptr[c.srcs[0]])
    return metric_steps(c, [e], [4095])  # past kDlMaxDist (4,094), still packable


def ch_M9b(c):
    V = c.csr.num_nodes
    bits = max(1, (V - 1).bit_length())
    e = int(c.csr.row_ptr[c.srcs[0]])
    return metric_steps(c, [e], [1 << (32 - bits)])  # the packed word cannot hold it


def edge_steps(c, h, pre_down=False):
    """Half-edges h down then up again (pre_down: down before the query is
    created, then up, then down again)."""
    h = np.asarray(h, dtype=np.uint32)
    m = c.csr.metric[h].astype(np.uint64)
    paired = set(h.tolist()) == set(c.csr.rev[h].tolist())
    down = (lambda g: g.set_edges(h, np.zeros(len(h), dtype=np.uint8), m),
            without_halves(c.csr, h) if paired else None)
    up = (lambda g: g.set_edges(h, np.ones(len(h), dtype=np.uint8), m), c.csr)
    return (down, [up, down]) if pre_down else (None, [down, up])


def ch_E1(c):
    src = set(c.srcs)
    for l in range(c.csr.num_links):
        h = halves(c.csr, l)
        if not {int(c.csr.col[h[0]]), int(c.csr.col[h[1]])} & src:
            return edge_steps(c, h)
    raise AssertionError("every link touches a source")


def single_link_at_source(c, keep_class=True):
    """(source, link): the source's only link to that neighbour; keep_class:
    losing one another keeps the mask width class of both ends (the far end may
    be a source too)."""
    def kept(x):
        n = len(links_to(c.csr, x))
        return n >= 2 and (not keep_class or width_class(n) == width_class(n - 1))

    for s in dict.fromkeys(c.srcs):
        if kept(s):
            for f, ls in sorted(links_to(c.csr, s).items()):
                if len(ls) == 1 and kept(f):
                    return s, ls[0]
    raise AssertionError("no such source")


def ch_E2(c):
    return edge_steps(c, halves(c.csr, single_link_at_source(c)[1]))


def ch_E3(c):
    for s in dict.fromkeys(c.srcs):
        for f, ls in sorted(links_to(c.csr, s).items()):
            if len(ls) >= 2:
                return edge_steps(c, halves(c.csr, ls[0]))
    raise AssertionError("no parallel links at a source")


def ch_E4(c):
    s, l = single_link_at_source(c, keep_class=False)
    h = halves(c.csr, l)
    return edge_steps(c, [x for x in h if x in row_of(c.csr, s)])


def hub_link(c):
    nb = links_to(c.csr, c.hub)
    assert len(nb) == c.hubdeg and all(len(ls) == 1 for ls in nb.values())
    return halves(c.csr, nb[max(nb)][0])


def ch_E5(c):
    return edge_steps(c, hub_link(c))


def ch_E5b(c):
    return edge_steps(c, hub_link(c), pre_down=True)


def ch_E6(c):
    """Every link of the hub down while the query is created over every other
    source; one comes up: its far end gains a neighbour without a row."""
    hs = np.concatenate([halves(c.csr, ls[0]) for ls in links_to(c.csr, c.hub).values()])
    m = c.csr.metric[hs].astype(np.uint64)
    c.srcs = [s for s in c.srcs if s != c.hub]
    nb = links_to(c.csr, c.hub)
    # comes up at a source that keeps its mask width class: only the row is missing
    one = halves(c.csr, nb[min(f for f in nb if f in c.srcs and width_class(len(links_to(c.csr, f)))
                               == width_class(len(links_to(c.csr, f)) - 1))][0])
    rest = np.array(sorted(set(hs.tolist()) - set(one.tolist())), dtype=np.uint32)
    pre = (lambda g: g.set_edges(hs, np.zeros(len(hs), dtype=np.uint8), m), without_halves(c.csr, hs))
    up = (lambda g: g.set_edges(one, np.ones(2, dtype=np.uint8), c.csr.metric[one].astype(np.uint64)),
          without_halves(c.csr, rest))
    return pre, [up, pre]


CHANGES = {k[3:]: v for k, v in list(globals().items()) if k.startswith("ch_")}


# ------------------------------------------------------------------ the helper


def sample_rows(c):
    n = len(c.srcs)
    if c.csr.num_nodes >= 20000:
        return {0, n - 1}
    return {0, 1, n // 3, n // 2, n - 2, n - 1} if n >= 6 else set(range(n))


def read_rows(q, rows):
    nh = bool(q.flags & NH)
    return {i: (q.dist(i), q.nexthops(i) if nh else None) for i in rows}


def rerun_or_stale(q, g, new_csr, expect, c, prev, fact=""):
    """See the module docstring.  fact: what the refusal's detail must name.
    Returns "stale" or "ran"."""
    if q.stale():
        assert expect != "accept", "a change the contract says a live query survives was refused"
        with pytest.raises(abi.SpfError, match="stale query: .*" + fact):
            q.run()
        assert q.stale()
        for i, (d, m) in prev.items():  # the last run's rows: readable, unchanged
            assert (q.dist(i) == d).all(), i
            assert m is None or (q.nexthops(i) == m).all(), i
        return "stale"
    assert expect != "reject", "spf_query_stale let a change through that the plan cannot follow"
    assert new_csr is not None, "no fresh graph can stand for a half-edge down alone"
    q.run()
    f = abi.Graph(new_csr)
    try:
        r = f.query(c.srcs, c.flags, ignore=c.ign).run()
        if expect == "accept":
            assert q.kernel == r.kernel, (q.kernel, r.kernel)
        for i, s in enumerate(c.srcs):
            assert (q.dist(i) == r.dist(i)).all(), (i, s)
            if not c.flags & NH:
                continue
            assert list(g.nbrs(s)) == list(f.nbrs(s)), s  # mask bits name the same neighbours
            if q.nh_words(i) == r.nh_words(i):
                assert (q.nexthops(i) == r.nexthops(i)).all(), (i, s)
            else:
                assert q.nexthop_sets(i, s) == r.nexthop_sets(i, s), (i, s)
        r.close()
    finally:
        f.close()
    check_query(new_csr, q, c.srcs, not c.flags & UNIT, ignore=c.ign, rows=sample_rows(c))
    return "ran"


# ------------------------------------------------------------------ the matrix

A, R, X = "accept", "reject", "either"
WEIGHTED32 = ["lds", "lds-dist", "lds+rows", "gmem", "dstep", "dstep-ldsrow", "few-rows",
              "whatif-repair"]
UNIFORM = ["msbfs+levels", "msbfs", "helpers", "bfs+rows", "bfs", "bfs-gmem", "msbfs-ign",
           "whatif-links"]
UNITS = ["lds-unit", "msbfs+levels-unit", "whatif-links-unit"]
# spf_graph_set_edges applies to 32-bit graphs without metric 0: not to wide,
# exact and zero*.  E1 needs a link that touches no source: not the all-sources
# batches.  E2 on the what-if source-link batches, whose one source is the
# 9-neighbour hub (losing one crosses a width class: E5), is
# test_whatif_firsthop_gpu.py's source link set down between runs.  E3 where
# some source has parallel links to one neighbour.
ALL_SOURCES = ["lds+rows", "msbfs+levels", "msbfs", "msbfs+levels-unit", "bfs+rows", "bfs"]
SPARSE = ["lds", "lds-dist", "lds-unit", "lds-uniform", "helpers", "few-rows", "gmem", "dstep",
          "dstep-ldsrow", "dstep-packed", "bfs-gmem", "msbfs-ign", "msd", "whatif-repair"]
WHATIF_LINKS = ["whatif-links", "whatif-links-unit"]
PARALLEL = ["lds", "lds-dist", "lds-unit", "lds+rows", "msbfs+levels", "msbfs",
            "msbfs+levels-unit", "bfs+rows", "bfs"]

# what the refusal of a reject cell must name
FACT = {"M4": "uniform", "M6": "64-bit", "M8b": "metric-0", "M8c": "one nonzero",
        "M9": "LDS-row range", "M9b": "packed edge", "E5": "mask width", "E5b": "mask width",
        "E6": "no row"}


def fact_of(plan, code):
    if code == "M7":  # the first metric 0 moves the graph to 64-bit rows; one more or less, the set
        return "metric-0" if plan in ("wide", "zero3") else "64-bit"
    return FACT[code]


MATRIX = []
MATRIX += [(p, "T1", A) for p in PLANS if p != "msd" and "-h" not in p]
MATRIX += [(p, "M1", A) for p in WEIGHTED32 + ["dstep-packed", "wide", "exact", "msd"] + UNITS]
MATRIX += [(p, "M2", A) for p in WEIGHTED32 + ["dstep-packed", "wide", "exact"] + UNITS]
MATRIX += [(p, "M3", A) for p in UNIFORM]
MATRIX += [(p, "M3", A) for p in ("zero1", "zero3", "zero3-dist", "zero1-dist")]  # M8: the scale is read live
MATRIX += [(p, "M4", R) for p in UNIFORM]                           # WHY: uniformity ends
MATRIX += [("lds-uniform", "M4", X)]  # an SSSP plan would follow; the predicate is conservative
MATRIX += [(p, "M4", A) for p in UNITS]
MATRIX += [(p, "M5", X) for p in ("lds", "lds+rows", "dstep-ldsrow")]
MATRIX += [(p, "M6", R) for p in ("lds", "lds+rows", "msbfs+levels", "dstep", "dstep-ldsrow")]  # WHY
MATRIX += [("wide", "M6", X), ("lds-unit", "M6", A)]
MATRIX += [(p, "M7", R) for p in ("lds", "lds+rows", "msbfs+levels", "wide", "zero3")]
MATRIX += [("lds-unit", "M7", A)]
MATRIX += [("zero3", "M8b", R), ("zero3-dist", "M8b", R), ("zero1", "M8c", R), ("zero3", "M8c", R),
           ("zero1-dist", "M8c", R)]
MATRIX += [("dstep-ldsrow", "M9", R), ("few-rows", "M9", R), ("dstep-packed", "M9", X)]
MATRIX += [("dstep-ldsrow", "M9b", R), ("dstep-packed", "M9b", R), ("few-rows", "M9b", R)]  # WHY
MATRIX += [(p, "E1", A) for p in SPARSE + WHATIF_LINKS]
MATRIX += [(p, "E2", A) for p in SPARSE + ALL_SOURCES]
MATRIX += [(p, "E3", A) for p in PARALLEL]
MATRIX += [(p, "E4", X) for p in ("msbfs+levels", "whatif-links")]
# a width class crossed at 8 / 9, 16 / 17, 32 / 33 and 64 / 65 (the word count too) neighbours
MATRIX += [(p, "E5", R) for p in ("lds", "lds+rows", "msbfs+levels", "helpers", "whatif-links",
                                  "lds-h17", "lds-h65")]
MATRIX += [(p, "E5b", R) for p in ("lds", "msbfs+levels", "helpers", "lds-h33", "msbfs+levels-h65")]
MATRIX += [(p, "E6", R) for p in ("lds+rows", "msbfs+levels", "bfs+rows", "helpers", "few-rows")]  # WHY


@pytest.mark.parametrize("plan,code,expect", MATRIX, ids=[f"{p}-{k}-{e}" for p, k, e in MATRIX])
def test_cell(gpu_ready, plan, code, expect, monkeypatch):
    c = PLANS[plan]()
    for k, v in c.env.items():
        monkeypatch.setenv(k, v)
    pre, steps = CHANGES[code](c)
    g = abi.Graph(c.csr)
    try:
        exact0 = g.needs_exact
        if pre:
            pre[0](g)
        q = g.query(c.srcs, c.flags, ignore=c.ign).run()
        assert q.kernel == c.plan, q.kernel
        assert set(c.kernels) <= set(q.kernels()), q.kernels()
        assert not q.stale()
        prev = read_rows(q, sample_rows(c))
        for k, (apply, new_csr) in enumerate(steps):
            apply(g)
            if code in ("T1", "M1", "M2", "M3"):
                assert g.needs_exact == exact0  # the class is kept
            if code == "M6" and k == 0:
                assert g.needs_exact != exact0 or exact0
            want = expect if k == 0 else (A if expect == A else X)
            out = rerun_or_stale(q, g, new_csr, want, c, prev,
                                 fact_of(plan, code) if want == R else "")
            if k == 0:
                OUTCOME[(plan, code)] = out
            if out == "ran":
                prev = read_rows(q, sample_rows(c))
        q.close()
    finally:
        g.close()


def test_drain_that_flips_needs_exact(gpu_ready):
    """T2, WHY: the star of test_hop_bound_follows_drains.  Draining 8 withdraws
    the hop bound, so the graph needs 64-bit rows: the 32-bit query is refused,
    its unit-metric twin runs on; undraining makes the first one fresh again."""
    w = (1 << 32) // 7
    csr = abi.Csr.from_links(10, [(0, v, w, w) for v in range(1, 9)] + [(8, 9, w, w)])
    g = abi.Graph(csr)
    srcs = list(range(10))
    c = Case(csr, srcs, NH, "bfs+rows")
    cu = Case(csr, srcs, NH | UNIT, "bfs+rows")
    q = g.query(srcs, NH).run()
    qu = g.query(srcs, NH | UNIT).run()
    assert q.kernel == c.plan and qu.kernel == cu.plan and not g.needs_exact
    prev, prevu = read_rows(q, set(srcs)), read_rows(qu, set(srcs))
    ov = np.zeros(10, dtype=np.uint8)
    ov[8] = 1
    g.set_transit(ov)
    assert g.needs_exact
    OUTCOME[("star", "T2")] = rerun_or_stale(q, g, with_drains(csr, ov), R, c, prev, "64-bit")
    OUTCOME[("star-unit", "T2")] = rerun_or_stale(qu, g, with_drains(csr, ov), X, cu, prevu)
    g.set_transit(np.zeros(10, dtype=np.uint8))
    assert not g.needs_exact
    assert rerun_or_stale(q, g, csr, A, c, prev) == "ran"
    g.close()


def test_stale_is_cached_per_graph_generation(gpu_ready):
    """stale() after a change, asked twice, and after the change is undone."""
    c = p_uniform300()
    g = abi.Graph(c.csr)
    q = g.query(c.srcs, c.flags).run()
    _, steps = ch_M4(c)
    steps[0][0](g)
    assert q.stale() and q.stale()
    steps[1][0](g)
    assert not q.stale() and not q.stale()
    q.run()
    g.close()


def leaf_net():
    """40 nodes, node 39 a leaf behind 0 - 39 (the last link): with more than
    64 half-edges per patched one, a one-half-edge patch takes the sparse path."""
    links = [l for l in random_links(random.Random(5), 40, 100, 1, 9, parallel=0.0)
             if 39 not in l[:2]] + [(39, 0, 4, 4)]
    return TNet(40, links, (3, 7)), len(links) - 1


@pytest.mark.parametrize("event", ["raise_tight", "drain", "sparse"])
def test_route_table_refresh_with_its_own_query_rerun(gpu_ready, event):
    """spf_route_table_refresh_rows driven with the table's OWN query re-run
    after a metric patch and after a drain (the path include/openr_spf.h
    promises): the table equals a fresh table over a new query, and the query
    stays bound.  At the refresh module's V = 13 a patch takes the full upload
    (raise_tight); "sparse" patches one half-edge of 200, the path in-place
    route tables take, and moves every row's route to the leaf's prefix."""
    if event == "sparse":
        n, last = leaf_net()
        ann = seeded_lists(65, 40, 7)
        ann[1] = [39]
        change = dict(metrics={last: (4, 9)})  # 0 -> 39 alone
        assert 64 <= len(n.csr.col)
    else:
        n, ann, change = mixed_net(), mixed_ann(65, 7), EVENTS[event]
    try:
        t = n.table(ann, False)
        before = snapshot(n, t)
        n.change(**change)
        assert not n.q.stale()
        n.q.run()
        counts = t.refresh_rows(n.q, None)
        after = snapshot(n, t)
        assert counts.sum() > 0 and not same(before, after)
        q2 = n.query()
        fresh = n.table(ann, False, q=q2)
        assert same(after, snapshot(n, fresh))
        check_query(n.csr, n.q, [int(s) for s in n.src], True)
        assert abi.load().spf_query_destroy(n.q.h) == abi.SPF_E_INVALID  # still the table's
        assert same(snapshot(n, t.run()), after)
    finally:
        n.close()


def test_matrix_counts():
    """No accept cell was reported stale, no reject cell was run (the helper
    asserts both as it goes; this pins the totals), and at most a third of the
    cells leave the choice to the predicate."""
    cells = MATRIX + [("star", "T2", R), ("star-unit", "T2", X)]
    assert len(set((p, k) for p, k, _ in cells)) == len(cells)
    either = [x for x in cells if x[2] == X]
    assert 3 * len(either) <= len(cells), (len(either), len(cells))
    for p, k, e in cells:
        got = OUTCOME.get((p, k))
        if got is not None:
            assert (e, got) not in ((A, "stale"), (R, "ran")), (p, k, e, got)
    ran = [x for x in cells if (x[0], x[1]) in OUTCOME]
    if len(ran) == len(cells):  # the whole module ran: every side was exercised
        assert {OUTCOME[(p, k)] for p, k, _ in cells} == {"stale", "ran"}
