"""GPU parity of every per-source SPF kernel instance, ignore-list storage
form and query-to-query carry-over against the literal DijkstraQ replay
(oracle/spf_py.py), through the raw C ABI.

The per-source kernels are a family of template instances
(spf_sssp_kernel<WMAX, UNIT, IGN, GMEM>, spf_dstep_kernel<WMAX, IGN, BS, LBK>,
spf_wide_kernel, spf_nh_rows_kernel).  Which instance a batch runs follows
from spf_query_create's plan and three read-backs: the plan string
(spf_query_kernel_name), the widest mask of the batch (spf_query_nh_words ->
WMAX 1 / 4 / 16) and the flags and ignore lists the batch was created with.

  A. instance matrix: every case asserts its plan string and mask-word class
     before it compares anything; a case that lands on another plan fails.
  B. ignore-list storage forms: one batch per plan whose lists have 0, 1, 7,
     8, 9, 200, 2047, 2048, 2049 and ~3000 entries (nothing / LDS sorted list /
     LDS hash set / global list, and the boundaries between them), with the
     what-if screen and repair on and off.
  C. carry-over: nq = 2 * B * CUs + 64 queries (B = the planner's bound on
     workgroups per CU), so every workgroup runs at least two queries and the
     LDS state one query leaves is the state the next one starts from.

One planner fact the cases are laid out around: a unit-metric batch with next
hops and no ignore list takes the MS-BFS plan whenever V <= 20,448 (the
batch's neighbours ride along as helper sources), so spf_sssp_kernel<W, UNIT,
no IGN> on the LDS plan is reachable only for 20,448 < V <= ~25,680.  Those
cells of the matrix run on a 21,000-node graph; every other LDS cell runs on
the 420-node graph.
"""

import random

import numpy as np
import pytest

from openr_amd import abi
from oracle import spf_py

from .test_abi_gpu import check_query, random_links

pytestmark = pytest.mark.gpu

NH = abi.SPF_F_NEXTHOPS
UNIT = abi.SPF_F_UNIT_METRIC
H4, H16 = 5, 9  # hubs: 100 neighbours (2 mask words), 300 neighbours (5 words)
LENGTHS = (0, 1, 7, 8, 9, 200, 2047, 2048, 2049, 3000)


# ---------------------------------------------------------------- reference


class RefCache:
    """spf_py.run_spf results keyed by (graph, source, unit, ignore set), so
    the slow replay of a big-graph row runs once per module.  Installed in
    place of spf_py.run_spf for this module (check_query calls it there).
    Cached rows drop the path links (check_query does not read them) and share
    equal next-hop sets."""

    def __init__(self, run_spf):
        self.run_spf = run_spf
        self.rows = {}
        self.dag = {}
        self.sets = {}

    def __call__(self, csr, src, use_link_metric=True, ignore=frozenset()):
        key = (id(csr), int(src), bool(use_link_metric), frozenset(ignore))
        hit = self.rows.get(key)
        if hit is None:
            full = self.run_spf(csr, int(src), bool(use_link_metric), key[3])
            if not key[3]:
                self.dag[key[:3]] = sorted(
                    {int(csr.link_id[e]) for (_, _, p, _) in full.values() for (e, _) in p})
            row = {v: (d, self.sets.setdefault(nh, nh), None, rank)
                   for v, (d, nh, _, rank) in full.items()}
            hit = self.rows[key] = (csr, row)  # (the csr is kept alive: its id is the key)
        return hit[1]

    def dag_links(self, csr, src, use_link_metric):
        """Link ids on the shortest-path DAG of `src` (the replay's path links)."""
        self(csr, src, use_link_metric)
        return self.dag[(id(csr), int(src), bool(use_link_metric))]


@pytest.fixture(scope="module", autouse=True)
def ref():
    mp = pytest.MonkeyPatch()
    cache = RefCache(spf_py.run_spf)
    mp.setattr(spf_py, "run_spf", cache)
    yield cache
    mp.undo()


def same_row(a, b):
    return a.keys() == b.keys() and all(a[v][:2] == b[v][:2] for v in a)


# ----------------------------------------------------------------- fixtures


class Net:
    """A graph fixture: csr, device graph, the hubs (None without) and three
    leaf sources (a plain node, a drained node, a spoke of both hubs' range)."""


def hub_csr(seed, V, L, wmin, wmax, hubs=True):
    """(csr, leaf sources) of a random asymmetric backbone with parallel
    links and about 3 % drained nodes; `hubs`: H4 and H16 with exactly 100 and
    300 distinct neighbours (one reached over three parallel links, one
    drained), every other node with at most 64."""
    rng = random.Random(seed)
    links = random_links(rng, V, L, wmin=wmin, wmax=wmax, parallel=0.03)
    ov = np.zeros(V, dtype=np.uint8)
    if hubs:
        links = [l for l in links if l[0] not in (H4, H16) and l[1] not in (H4, H16)]
        links += [(H4, v, rng.randint(wmin, wmax), rng.randint(wmin, wmax)) for v in range(20, 120)]
        links += [(H16, v, rng.randint(wmin, wmax), rng.randint(wmin, wmax))
                  for v in range(100, 400)]
        # two more links parallel to one spoke, other metrics
        links += [(H16, 100, wmax, max(wmin, 1)), (100, H16, max(wmin, 1), wmax)]
        rng.shuffle(links)
    for v in rng.sample(range(V), max(3, V * 3 // 100)):
        if v not in (H4, H16):
            ov[v] = 1
    if hubs:
        ov[20] = 1  # a drained node next to a hub
    plain, spoke = V - 20, (250 if hubs else V // 2)
    ov[plain] = ov[spoke] = 0
    drained = [int(v) for v in np.flatnonzero(ov) if v != 20]
    csr = abi.Csr.from_links(V, links, overloaded=ov)
    if hubs:
        row, col = csr.row_ptr, csr.col
        nbrs = [len(set(col[row[v]:row[v + 1]].tolist())) for v in range(V)]
        assert nbrs[H4] == 100 and nbrs[H16] == 300
        assert max(n for v, n in enumerate(nbrs) if v not in (H4, H16)) <= 64
    return csr, [plain, drained[0], spoke]


def hub_net(seed, V, L, wmin, wmax, hubs=True):
    net = Net()
    net.csr, net.leaves = hub_csr(seed, V, L, wmin, wmax, hubs)
    net.H4, net.H16 = (H4, H16) if hubs else (None, None)
    net.g = abi.Graph(net.csr)
    net.V = V
    if hubs:
        assert net.g.num_nbrs(H4) == 100 and net.g.num_nbrs(H16) == 300
    net.pairs = {}
    return net


@pytest.fixture(scope="module")
def small(gpu_ready):
    net = hub_net(101, 420, 1300, 1, 20)
    yield net
    net.g.close()


@pytest.fixture(scope="module")
def dense(gpu_ready):
    """The small graph's ingredients with more than 3000 links (part B's lists)."""
    net = hub_net(102, 420, 3300, 1, 20)
    assert net.csr.num_links > 3100
    yield net
    net.g.close()


@pytest.fixture(scope="module")
def mid(gpu_ready):
    """Past the MS-BFS plan's 20,448 nodes, within the LDS plan's image."""
    net = hub_net(103, 21000, 45000, 1, 20)
    yield net
    net.g.close()


@pytest.fixture(scope="module")
def big(gpu_ready):
    net = hub_net(104, 26000, 60000, 1, 300)
    yield net
    net.g.close()


@pytest.fixture(scope="module")
def few(gpu_ready):
    """4096 nodes, metrics past 12 bits: the few-source delta-stepping form
    (the LDS-row / helper-rows plan needs metrics <= 4094)."""
    net = hub_net(105, 4096, 12000, 1, 5000)
    assert int(net.csr.metric.max()) > 4094
    yield net
    net.g.close()


@pytest.fixture(scope="module")
def wide150(gpu_ready):
    """150 nodes, metric-0 links, more than 3000 links (part B, wide plan)."""
    net = hub_net(106, 150, 3300, 0, 6, hubs=False)
    assert net.g.needs_exact and net.csr.num_links > 3100
    yield net
    net.g.close()


@pytest.fixture(scope="module")
def widehub(gpu_ready):
    """The dense graph's ingredients with metric-0 links (part C, wide plan)."""
    net = hub_net(107, 420, 3300, 0, 6)
    assert net.g.needs_exact and net.csr.num_links > 3100
    yield net
    net.g.close()


@pytest.fixture(scope="module")
def cus(gpu_ready):
    import torch

    return int(torch.cuda.get_device_properties(0).multi_processor_count)


# ------------------------------------------------------------------ helpers


def make_list(rng, csr, dag, n, src, fake=False):
    """A strictly sorted ignore list of n link ids, about a third of them on
    the source's shortest-path DAG (its own links first: a short list must
    still change the row); `fake`: one of the n names no link."""
    want = n - (1 if fake else 0)
    own = set(csr.link_id[csr.row_ptr[src]:csr.row_ptr[src + 1]].tolist())
    first = [l for l in dag if l in own]
    rest = [l for l in dag if l not in own]
    rng.shuffle(first)
    rng.shuffle(rest)
    s = set((first + rest)[:max(1, want // 3)]) if want > 0 else set()
    while len(s) < want:
        s.add(rng.randrange(csr.num_links))
    out = sorted(s)
    if fake:
        out.append(csr.num_links + 3)
    assert len(out) == n
    return out


def matrix_ignore(ref, net, srcs):
    """Part A's lists: 12 links per source, some on its (metric) DAG."""
    return [make_list(random.Random(1000 + s), net.csr, ref.dag_links(net.csr, s, True), 12, s)
            for s in srcs]


def matrix_batch(net, wclass):
    a, b, c = net.leaves
    return {1: [a, b, c], 4: [net.H4, a, b], 16: [net.H16, a, b]}[wclass]


def in_class(words, wclass):
    return {0: words == 0, 1: words == 1, 4: 2 <= words <= 4, 16: 5 <= words <= 16}[wclass]


def run_case(net, srcs, flags, ign, kernel, wclass):
    q = net.g.query(srcs, flags, ignore=ign).run()
    try:
        assert q.kernel == kernel, (q.kernel, kernel)
        if flags & NH:
            words = max(q.nh_words(i) for i in range(len(srcs)))
            assert in_class(words, wclass), (words, wclass)
        else:
            assert wclass == 0
        check_query(net.csr, q, srcs, not (flags & UNIT), ign)
    finally:
        q.close()


def storage_pairs(ref, net, unit):
    """Part B's batch as (source, ignore list) pairs: the ten list lengths
    over repeated sources (the what-if screen runs only when sources repeat),
    one list with an id past num_links, one list entirely off the source's DAG.
    Every non-empty list but that one changes its source's reference row."""
    key = bool(unit)
    if key in net.pairs:
        return net.pairs[key]
    a, b, c = net.leaves
    h4 = net.H4 if net.H4 is not None else 3
    h16 = net.H16 if net.H16 is not None else 11
    src_of = {0: a, 1: a, 7: b, 8: a, 9: h4, 200: b, 2047: a, 2048: b, 2049: h16, 3000: a}
    rng = random.Random(7 + key)

    def matters(s, lst):
        return not same_row(ref(net.csr, s, not unit), ref(net.csr, s, not unit, frozenset(lst)))

    def draw(s, n, fake=False):
        # (a parallel link or an equal-cost detour can hide one ignored link:
        # draw again until the reference row changes)
        for _ in range(8):
            lst = make_list(rng, net.csr, ref.dag_links(net.csr, s, not unit), n, s, fake)
            if n == 0 or matters(s, lst):
                return (s, tuple(lst))
        raise AssertionError(f"no list of {n} links changes the row of source {s}")

    pairs = [draw(src_of[n], n, fake=(n == 9)) for n in LENGTHS]
    on_dag = set(ref.dag_links(net.csr, b, not unit))
    off = next(l for l in range(net.csr.num_links) if l not in on_dag)
    assert not matters(b, [off])
    pairs.append((b, (off,)))
    pairs.append(draw(c, 1))
    net.pairs[key] = pairs
    return pairs


# -------------------------------------------------------- A. instance matrix

WUI = [(w, u, i) for w in (1, 4, 16) for u in (False, True) for i in (False, True)]


def _id(case):
    return "-".join(str(int(x)) for x in case) if isinstance(case, tuple) else str(case)


@pytest.mark.parametrize("case", WUI, ids=_id)
def test_matrix_sssp_lds(small, mid, ref, case):
    """spf_sssp_kernel<WMAX, UNIT, IGN, false>: a hub (or a third leaf) plus
    two leaves, too few for the rows plan."""
    wclass, unit, ign = case
    net = mid if unit and not ign else small  # (see the module docstring)
    srcs = matrix_batch(net, wclass)
    run_case(net, srcs, NH | (UNIT if unit else 0),
             matrix_ignore(ref, net, srcs) if ign else None, "lds", wclass)


@pytest.mark.parametrize("case", WUI + [(0, False, True), (0, True, True)], ids=_id)
def test_matrix_sssp_gmem(big, ref, case, monkeypatch):
    """spf_sssp_kernel<WMAX, UNIT, IGN, true>: the distance row does not fit
    LDS; weighted batches with delta-stepping off, unit-metric ones as they
    come (past the MS-BFS plan's size, and next hops or ignore lists keep them
    off the BFS kernel).  WMAX 0: distances only, with ignore lists."""
    wclass, unit, ign = case
    monkeypatch.setenv("OPENR_SPF_DSTEP", "0")
    srcs = matrix_batch(big, wclass or 1)
    run_case(big, srcs, (NH if wclass else 0) | (UNIT if unit else 0),
             matrix_ignore(ref, big, srcs) if ign else None, "gmem", wclass)


DSTEP = [(w, i, lbk) for w in (1, 4, 16) for i in (False, True) for lbk in (True, False)]


@pytest.mark.parametrize("case", DSTEP + [(0, True, True), (0, True, False)], ids=_id)
def test_matrix_dstep(big, ref, case, monkeypatch):
    """spf_dstep_kernel<WMAX, IGN, BS, LBK>: bucket bytes in LDS or read from
    the distance row.  WMAX 0: distances only, with ignore lists (without
    them the LDS-row kernel takes the batch)."""
    wclass, ign, lbk = case
    monkeypatch.delenv("OPENR_SPF_DSTEP", raising=False)
    monkeypatch.setenv("OPENR_SPF_DSTEP_LDSBKT", "1" if lbk else "0")
    srcs = matrix_batch(big, wclass or 1)
    run_case(big, srcs, NH if wclass else 0,
             matrix_ignore(ref, big, srcs) if ign else None, "dstep", wclass)


@pytest.mark.parametrize("wclass", [4, 16])
def test_matrix_dstep_few_sources(few, wclass, monkeypatch):
    """One hub source of a weighted graph that fits LDS: the few-source form
    of delta-stepping (next hops inline: metrics past 12 bits rule out the
    helper-rows plan)."""
    monkeypatch.delenv("OPENR_SPF_DSTEP", raising=False)
    run_case(few, [few.H4 if wclass == 4 else few.H16], NH, None, "dstep", wclass)


def test_matrix_rows_plan_hubs(small):
    """All sources, weighted: distance rows on the LDS plan, next hops from
    the rows (spf_nh_rows_kernel), the hubs' with 2 and 5 mask words."""
    srcs = list(range(small.V))
    q = small.g.query(srcs, NH).run()
    try:
        assert q.kernel == "lds+rows"
        assert q.nh_words(H4) == 2 and q.nh_words(H16) == 5
        assert max(q.nh_words(i) for i in srcs if i not in (H4, H16)) == 1
        check_query(small.csr, q, srcs, True)
    finally:
        q.close()


# ------------------------------------------------ B. ignore-list storage forms

PLANS = {
    # plan: (fixture, flags, OPENR_SPF_DSTEP, workgroups per CU the planner allows)
    "lds": ("dense", NH, None, 4),
    "gmem": ("big", NH, "0", 2),
    "dstep": ("big", NH, None, 2),
    "wide": ("wide150", NH | abi.SPF_F_ORDER, None, 2),
}


def set_knobs(monkeypatch, dstep, screen):
    if dstep is None:
        monkeypatch.delenv("OPENR_SPF_DSTEP", raising=False)
    else:
        monkeypatch.setenv("OPENR_SPF_DSTEP", dstep)
    if screen:
        monkeypatch.delenv("OPENR_SPF_WHATIF_SCREEN", raising=False)
    else:
        monkeypatch.setenv("OPENR_SPF_WHATIF_SCREEN", "0")


@pytest.mark.parametrize("screen", [True, False], ids=["screen", "scratch"])
@pytest.mark.parametrize("plan", list(PLANS))
def test_ignore_list_forms(request, ref, plan, screen, monkeypatch):
    """Lists of 0, 1, 7, 8, 9, 200, 2047, 2048, 2049 and 3000 links in one
    batch: with the default knobs (sources repeat: the what-if screen copies
    the off-DAG queries and the repair path reads the hashed and the global
    lists) and with every query run from scratch."""
    fixture, flags, dstep, _ = PLANS[plan]
    net = request.getfixturevalue(fixture)
    pairs = storage_pairs(ref, net, False)
    assert sorted({len(l) for _, l in pairs}) == sorted(LENGTHS)
    set_knobs(monkeypatch, dstep, screen)
    srcs = [s for s, _ in pairs]
    ign = [list(l) for _, l in pairs]
    assert all(a < b for l in ign for a, b in zip(l, l[1:]))  # strictly sorted
    assert any(x >= net.csr.num_links for l in ign for x in l)
    q = net.g.query(srcs, flags, ignore=ign).run()
    try:
        assert q.kernel == plan
        if plan in ("lds", "gmem"):
            n = q.screened()
            if screen:
                assert n is not None and 0 < n < len(srcs), n
        check_query(net.csr, q, srcs, True, ign)
    finally:
        q.close()


# ------------------------------------- C. carry-over inside one workgroup

CARRY = {
    # case: (fixture, flags, OPENR_SPF_DSTEP, B, plan, ignore lists)
    "lds": ("dense", NH, None, 4, "lds", True),
    "gmem": ("big", NH, "0", 2, "gmem", True),
    "dstep": ("big", NH, None, 2, "dstep", True),
    "dstep-noign": ("big", NH, None, 2, "dstep", False),
    "wide": ("widehub", NH | abi.SPF_F_ORDER, None, 2, "wide", True),
    "lds-unit": ("dense", NH | UNIT, None, 4, "lds", True),
}


@pytest.mark.parametrize("screen", [True, False], ids=["screen", "scratch"])
@pytest.mark.parametrize("case", list(CARRY))
def test_carry_over_between_queries(request, ref, cus, case, screen, monkeypatch):
    """nq = 2 * B * CUs + 64 queries drawn from a small pool of (source,
    ignore list) pairs: wide and narrow masks, all four ignore forms, in
    shuffled order, so each workgroup runs a second (64 of them a third) query
    on the LDS state the one before left.  Each pair's first occurrence equals
    the replay; every later one is byte-equal to the first."""
    fixture, flags, dstep, B, plan, with_ign = CARRY[case]
    net = request.getfixturevalue(fixture)
    unit = bool(flags & UNIT)
    if with_ign:
        pool = list(storage_pairs(ref, net, unit))
        if net.V < 1000:  # small graphs: a few more pairs (the big pool stays at 12)
            pool += [(net.H16, ()), (net.H4, ()), (net.leaves[2], ())]
    else:
        pool = [(s, ()) for s in net.leaves + [net.H4, net.H16, 1000, 2000, 3000]]
    assert len(pool) <= (12 if net.V > 1000 else 48)
    stride = B * cus
    nq = 2 * stride + 64
    assert nq >= 2 * B * cus + 64
    order = [i % len(pool) for i in range(nq)]
    random.Random(2024).shuffle(order)
    words = [max(1, (net.g.num_nbrs(s) + 63) // 64) for s, _ in pool]
    assert any(words[order[i]] >= 5 and words[order[i + stride]] == 1 for i in range(nq - stride))
    if with_ign:
        lens = [len(l) for _, l in pool]
        assert any(8 <= lens[order[i]] <= 1024 and 1 <= lens[order[i + stride]] < 8
                   for i in range(nq - stride))
    set_knobs(monkeypatch, dstep, screen)
    srcs = [pool[k][0] for k in order]
    ign = [list(pool[k][1]) for k in order] if with_ign else None
    q = net.g.query(srcs, flags, ignore=ign).run()
    try:
        assert q.kernel == plan
        first = {}
        for i, k in enumerate(order):
            first.setdefault(k, i)
        assert len(first) == len(pool)
        check_query(net.csr, q, srcs, not unit, ign, rows=set(first.values()))
        want = {k: (q.dist(i), q.nexthops(i)) for k, i in first.items()}
        for i, k in enumerate(order):
            if i == first[k]:
                continue
            d, m = want[k]
            assert np.array_equal(q.dist(i), d), (i, k)
            assert np.array_equal(q.nexthops(i), m), (i, k)
    finally:
        q.close()
