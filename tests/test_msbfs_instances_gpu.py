"""GPU parity of every multi-source BFS kernel instance, node-count boundary
and batch-to-batch carry-over, through the raw C ABI.

The uniform-metric all-sources path runs spf_msbfs_kernel<MT, KMAX, SELL, GEN>
and then the level-row next-hop passes.  launch_msbfs picks the instance by
batch width (MT: 64 or 32 sources), by nodes per thread (K = ceil(V / 1024),
rounded up to a KMAX class), by sliced-ELL or plain CSR (OPENR_MS_SELL) and by
plain or general form (GEN: ignore masks, OPENR_MS_WREC, the zero-metric
closure).  With OPENR_SPF_CREATE_TIMING=1 it reports each launch on stderr:

  [launch_msbfs] bits=32 kmax=12 sell=1 gen=0 grid=256 nbatch=321 blocked=0 tables=1

Every case here reads that line back (capfd) and asserts the instance, and
where it matters the batch count, BEFORE it compares anything: a case that
lands on another instance or another plan fails.  The instance is read back,
not inferred.

References: oracle/csr_spf.h summaries (reached, distance sum, next-hop count
and the mix over every (node, distance) and (node, next hop) pair) for every
query of every case, the literal DijkstraQ replay (oracle/spf_py.py) node by
node on a few rows.  All integers, every comparison bit-exact.

  A. test_matrix_plain / test_matrix_past_the_plan: plain form at every KMAX
     class and every node count where the instance changes.
  B. general form: ignore masks (test_ignore_masks), OPENR_MS_WREC=1
     (test_wave_recorded_rows), the zero-metric closure (test_zero_closure_*)
     and the what-if first-hop batches' blocked node under 32-bit batches
     (test_blocked_batches_32bit).
  C. test_carry_over_small / test_carry_over_production: a workgroup runs a
     second and third batch on the LDS and vis[] state the one before left.
  D. test_deep_levels_kmax12: levels past 127 and 254 in a 32-bit batch.

Which case runs which instance (bits, KMAX, SELL, GEN); V as listed, "k32" =
under OPENR_SPF_MSBFS=32:

  64  4  1 0  A 4096                 64  4  0 0  A 4096 (second run, SELL=0)
  64  8  1 0  A 4097 5000 8192       64  8  0 0  A 5000
  64 10  1 0  A 8193 9000 10224      64 10  0 0  A 9000
  32  4  1 0  A k32 1023 4096        32  4  0 0  A k32 1023
  32  8  1 0  A k32 4097 8192        32  8  0 0  A k32 4097
  32 12  1 0  A k32 8193, 10225 10240 10241 11000 12288
                                     32 12  0 0  A 11000
  32 16  1 0  A 12289 14000 16384    32 16  0 0  A 14000
  32 20  1 0  A 16385 18000 20448; C production (at 256 CUs)
                                     32 20  0 0  A 18000
  64  4  1 1  B wrec 4096; C small (ignore lists)
  64  8  1 1  B wrec 5000; B ignore 4097
  64 10  1 1  B wrec 9000; B ignore 8193
  32  4  1 1  B wrec k32 1023; B ignore k32 1500; B zero closure k32 260;
              C small k32 (ignore lists)
  32  8  1 1  B wrec k32 5000
  32 12  1 1  B wrec 11000; B ignore 10241; B zero closure 11000
  32 16  1 1  B wrec 14000
  32 20  1 1  B wrec 18000; B ignore 16385
  (any) 0 1   B wrec, every size above: its third run sets OPENR_MS_SELL=0

The size limits.  Every instance holds 256 bytes of static LDS (the workgroup
reduction behind __syncthreads_or) beside the dynamic frontier double buffer,
and a workgroup may hold 160 KB in all.  So a 64-bit batch fits for 2 * V * 8
+ 256 <= 163,840, V <= 10,224, and a 32-bit batch for V <= 20,448 (ms_fits in
spf_device.hip, which reads the static figure back from the runtime).  The
seams are therefore 10,224 / 10,225 (the width switch) and 20,448 / 20,449
(the end of the plan): a launch with the double buffer alone at 160 KB is
refused by the runtime.  10,240 / 10,241 and 20,480 / 20,481 stay in the
matrix as ordinary sizes.

Unreachable: spf_msbfs_kernel<uint64_t, 12 | 16, *, *>.  spf_query_create
narrows a batch to 32 sources for V > 10,224, so a 64-bit batch never has more
than 10 nodes per thread.  launch_msbfs no longer instantiates them (an
"internal:" SPF_E_INVALID stands in their place); test_matrix_plain at V =
10224 / 10225 pins the width switch itself.  Past 20,448 nodes no MS-BFS plan
exists: test_matrix_past_the_plan.

The zero-metric plan's own limit is the 32-bit plain plan's (V <= 20,448), so
it is kept at 10,241 <= V <= 12,288 and test_zero_closure_kmax12 runs it there.

Carry-over: the planner's grid is min(nbatch, CUs * per_cu), per_cu = min(2,
160 KB / frontier bytes).  The small graph (per_cu = 2) takes nq = 2 * B * grid
+ B + 1, so nbatch >= 2 * grid + 1 and EVERY workgroup runs at least two
batches.  The production form, batches of 32 on one workgroup per CU, meets
the same bound with all sources of a max(10241, 64 * CUs + 33)-node graph
(16,417 nodes and 514 batches at 256 CUs; 32 * CUs + 33 nodes would give a
second batch to a quarter of the workgroups only).  It needs all of them as
sources: the bound is on rows, 32 * (2 * CUs) + 1 of them.
"""

import random
import re

import numpy as np
import pytest

from openr_amd import abi
from oracle import spf_py
from tests.golden.summary import summaries_full

from .test_abi_gpu import check_query, random_links
from .test_config_sized_gpu import _batch_summaries, _check_summary

pytestmark = pytest.mark.gpu

NH = abi.SPF_F_NEXTHOPS
UNIT = abi.SPF_F_UNIT_METRIC
SLOT = 1024  # kMsThreads: thread t owns nodes t, t + 1024, ...
LDS = 160 * 1024 - 256  # per workgroup, less the kernel's static 256 bytes (ms_fits)
MS_MAX_V = LDS // 8  # 20,448: the 32-bit frontier double buffer, 2 * V * 4 bytes, still fits
DEGREES = (0, 4, 8, 9, 12, 13)  # the 8 / 4 / 1 tails of the CSR pull, odd and even uint4 groups


# ------------------------------------------------------------------ helpers


@pytest.fixture(autouse=True)
def replay_memo(monkeypatch):
    """One literal replay per (graph, source, metric mode, ignore list) and
    test: check_query is called on the same rows of several queries."""
    real, memo = spf_py.run_spf, {}

    def run_spf(csr, src, use_link_metric=True, ignore=frozenset()):
        key = (id(csr), int(src), bool(use_link_metric), frozenset(ignore))
        if key not in memo:
            memo[key] = real(csr, int(src), use_link_metric, key[3])
        return memo[key]

    monkeypatch.setattr(spf_py, "run_spf", run_spf)
    monkeypatch.setenv("OPENR_SPF_CREATE_TIMING", "1")
    for knob in ("OPENR_SPF_MSBFS", "OPENR_MS_SELL", "OPENR_MS_WREC", "OPENR_MS_COOP"):
        monkeypatch.delenv(knob, raising=False)


@pytest.fixture(scope="module")
def cus(gpu_ready):
    import torch

    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def kmax_of(bits, V):
    """launch_msbfs's KMAX class of K = ceil(V / 1024) nodes per thread."""
    K = (V + SLOT - 1) // SLOT
    return next(k for k in ((4, 8, 10) if bits == 64 else (4, 8, 12, 16, 20)) if K <= k)


def width_of(V, knob):
    """spf_query_create's batch width: OPENR_SPF_MSBFS (default 64), lowered
    to 32 once the 64-bit frontier double buffer, 2 * V * 8 bytes, no longer
    fits LDS (V > 10,224)."""
    return 32 if knob == "32" or 2 * V * 8 > LDS else 64


def run_logged(q, capfd):
    """q.run(); the [launch_msbfs] lines of that run as dicts."""
    capfd.readouterr()
    q.run()
    err = capfd.readouterr().err
    return [{k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", line)}
            for line in err.splitlines() if line.startswith("[launch_msbfs]")]


def one_launch(lines, bits, kmax, sell, gen, **more):
    want = dict(bits=bits, kmax=kmax, sell=sell, gen=gen, blocked=0, **more)
    assert len(lines) == 1, lines
    got = {k: lines[0][k] for k in want}
    assert got == want, (lines[0], want)
    return lines[0]


def oracle(csr, srcs, nh, ign=None):
    from oracle import build as OB

    OB.build()
    from oracle import _oracle_ref as O

    ioff = il = None
    if ign is not None:
        lists = [sorted({int(x) for x in l}) for l in ign]
        ioff = np.zeros(len(lists) + 1, dtype=np.uint32)
        ioff[1:] = np.cumsum([len(l) for l in lists])
        il = np.asarray([x for l in lists for x in l] or [0], dtype=np.uint32)
    return O.csr_spf_summary(csr.row_ptr, csr.col, csr.metric.astype(np.uint64), csr.link_id,
                             csr.overloaded, np.asarray(srcs, dtype=np.uint32), ioff, il,
                             True, bool(nh), 8)


def summaries(q, g, srcs, chunk=4096):
    """_batch_summaries' four numbers of every query, fetched `chunk` queries
    at a time (the carry-over batches are tens of thousands of rows), and for
    distance-only queries too (no masks: pair count 0)."""
    srcs = np.asarray(srcs, dtype=np.uint32)
    if q.flags & NH and len(srcs) <= chunk:
        return _batch_summaries(q, g, srcs, None)
    nbr, out = {}, []
    for lo in range(0, len(srcs), chunk):
        n = min(chunk, len(srcs) - lo)
        if q.flags & NH:
            rows, masks = q.fetch_host(lo, n)
            words = [q.nh_words(i) for i in range(lo, lo + n)]
            nbrs = []
            for s in srcs[lo:lo + n]:
                if int(s) not in nbr:
                    nbr[int(s)] = g.nbrs(int(s))
                nbrs.append(nbr[int(s)])
        else:
            rows, _ = q.fetch_host(lo, n, masks=False)
            masks, words, nbrs = np.zeros(1, dtype=np.uint64), [0] * n, [()] * n
        out.append(summaries_full(rows, masks, words, nbrs))
    return np.concatenate(out)


def check_all(q, g, csr, srcs, what, ign=None, want=None):
    """Every query's summary against the oracle's for the same sources."""
    if want is None:
        want = oracle(csr, srcs, q.flags & NH, ign)
    _check_summary(summaries(q, g, srcs), want, None, what)


def same_rows(q, i, j):
    assert np.array_equal(q.dist(i), q.dist(j)), (i, j)
    if q.flags & NH:
        assert np.array_equal(q.nexthops(i), q.nexthops(j)), (i, j)


def image(q):
    """Every row and mask of the query, as fetched."""
    rows, masks = q.fetch_host(0, q.n, masks=bool(q.flags & NH))
    return rows, masks


def same_image(a, b, what):
    assert np.array_equal(a[0], b[0]), f"{what}: distance rows differ"
    if a[1] is not None:
        assert np.array_equal(a[1], b[1]), f"{what}: next-hop masks differ"


class Net:
    pass


def uniform_net(V, metric, seed, parallel=0.01):
    """About 3V links of one metric with a few parallel ones; one node each of
    degree 0, 4, 8, 9, 12 and 13; about 2 % drained nodes, among them V - 1
    and the first node of the last thread slot."""
    rng = random.Random(seed)
    links = random_links(rng, V, 3 * V, wmin=metric, wmax=metric, parallel=parallel, asym=False)
    K = (V + SLOT - 1) // SLOT
    last0 = (K - 1) * SLOT
    slot_nodes = [min(k * SLOT + 5, V - 1) for k in range(K)]  # a source in every thread slot
    fixed = {0, V - 1, V - 2, last0} | set(slot_nodes)
    pool = [v for v in rng.sample(range(V), 40) if v not in fixed]
    special = dict(zip(DEGREES, pool))
    sp = set(special.values())
    links = [l for l in links if l[0] not in sp and l[1] not in sp]
    for d, v in special.items():
        for _ in range(d):
            u = rng.randrange(V)
            while u in sp:
                u = rng.randrange(V)
            links.append((v, u, metric, metric))
    ov = np.zeros(V, dtype=np.uint8)
    ov[rng.sample(range(V), max(2, V // 50))] = 1
    ov[V - 1] = ov[last0] = 1
    if last0:
        ov[0] = 0
    net = Net()
    net.V, net.rng, net.last0, net.special, net.slot_nodes = V, rng, last0, special, slot_nodes
    net.csr = abi.Csr.from_links(V, links, overloaded=ov)
    deg = np.diff(net.csr.row_ptr.astype(np.int64))
    assert all(deg[v] == d for d, v in special.items()), [(d, deg[v]) for d, v in special.items()]
    net.drained = int(next(v for v in np.flatnonzero(ov) if v not in fixed and v not in sp))
    net.g = abi.Graph(net.csr)
    return net


def matrix_sources(net, B):
    """n = 3 B + 1 sources.  Positions 0, 3 and 6 (kept by the every-third
    distance batch): node 0, a drained node, a node of the last thread slot.
    Also V - 1, the linkless node, a node of every thread slot, one source
    repeated inside its batch and one repeated two batches on.  The filler is
    redrawn until the rows the planner adds (the sources' neighbours outside
    the batch, helper sources) leave ONE live bit in the last batch."""
    V, rng = net.V, net.rng
    slot_nodes = net.slot_nodes
    # (V - 1 is itself the last slot's source where that slot holds one node)
    second = V - 1 if slot_nodes[-1] != V - 1 else V - 2
    head = [0, second, net.special[0], net.drained, net.special[9], net.special[13], slot_nodes[-1]]
    need = head + [v for v in slot_nodes[:-1] if v not in head]
    n = 3 * B + 1
    fill = [v for v in rng.sample(range(V), n) if v not in need][:n - 2 - len(need)]
    base = need + fill
    assert len(set(base)) == len(base) == n - 2
    nbrs = {}

    def rows(srcs):
        have = set(srcs)
        for s in have:
            if s not in nbrs:
                nbrs[s] = set(net.g.nbrs(s).tolist())
        return len(srcs) + len(set().union(*(nbrs[s] for s in have)) - have)

    for _ in range(4000):
        srcs = list(base)
        srcs.insert(9, srcs[4])           # repeated inside batch 0
        srcs.insert(2 * B + 3, srcs[1])   # repeated two batches on
        assert len(srcs) == n and srcs[0] == 0 and srcs[3] == net.drained
        assert srcs[6] == slot_nodes[-1] and srcs[6] >= net.last0
        if rows(srcs) % B == 1:
            return srcs, rows
        v = rng.randrange(V)
        if v not in base:
            base[-1 - rng.randrange(len(fill))] = v
    raise AssertionError("no filler leaves one live bit in the last batch")


# ------------------------------------------- A. instance and boundary matrix

DEFAULT_V = (4096, 4097, 5000, 8192, 8193, 9000, 10224, 10225, 10240, 10241, 11000, 12288, 12289,
             14000, 16384, 16385, 18000, 20448)
KNOB32_V = (1023, 4096, 4097, 8192, 8193)
# one size per (width, KMAX) class that also runs over the plain CSR
SELL0 = {(None, 4096), (None, 5000), (None, 9000), (None, 11000), (None, 14000), (None, 18000),
         ("32", 1023), ("32", 4097)}
MATRIX = [(None, V) for V in DEFAULT_V] + [("32", V) for V in KNOB32_V]


def _case_id(c):
    return f"k{c[0]}-{c[1]}" if c[0] else str(c[1])


@pytest.mark.parametrize("metric", [1, 7])
@pytest.mark.parametrize("case", MATRIX, ids=_case_id)
def test_matrix_plain(gpu_ready, case, metric, monkeypatch, capfd):
    """Metric 1 under SPF_F_UNIT_METRIC, metric 7 without (scale 7).  Three
    queries: 3 B + 1 sources with next hops, the first B - 1 of them with
    next hops (one partial batch), every third with distances alone (B + 1
    sources: the BFS stores the distances, the last batch holds one source)."""
    knob, V = case
    if knob:
        monkeypatch.setenv("OPENR_SPF_MSBFS", knob)
    B = width_of(V, knob)
    kmax = kmax_of(B, V)
    flags = UNIT if metric == 1 else 0
    net = uniform_net(V, metric, 1000 + V)
    g, csr = net.g, net.csr
    srcs, nrows = matrix_sources(net, B)
    queries = [(srcs, NH | flags, "msbfs+levels"), (srcs[:B - 1], NH | flags, "msbfs+levels"),
               (srcs[::3], flags, "msbfs")]
    assert len(queries[2][0]) == B + 1
    held = []
    for qs, f, plan in queries:
        q = g.query(qs, f)
        assert q.kernel == plan, (q.kernel, plan)
        rows = nrows(qs) if f & NH else len(qs)
        nbatch = (rows + B - 1) // B
        line = one_launch(run_logged(q, capfd), B, kmax, 1, 0, nbatch=nbatch, tables=1)
        if len(qs) > B:
            assert rows % B == 1 and line["grid"] == nbatch
        what = f"V={V} B={B} metric={metric} n={len(qs)} {plan}"
        check_all(q, g, csr, qs, what)
        replay = {0, 3, 6} if len(qs) == len(srcs) else {0, 1, 2}
        if len(qs) == B - 1:
            replay = {6}
        check_query(csr, q, qs, metric != 1, rows=replay)
        if len(qs) == len(srcs):
            same_rows(q, 4, 9)
            same_rows(q, 1, 2 * B + 3)
        if case in SELL0:
            # a new query, made while the first still holds its rows: every
            # byte of its result is written by the plain-CSR run
            monkeypatch.setenv("OPENR_MS_SELL", "0")
            p = g.query(qs, f)
            one_launch(run_logged(p, capfd), B, kmax, 0, 0, nbatch=nbatch, tables=1)
            monkeypatch.delenv("OPENR_MS_SELL")
            check_all(p, g, csr, qs, what + " plain CSR")
            same_image(image(q), image(p), what + " plain CSR vs sliced-ELL")
            held.append(p)
        held.append(q)
    for q in held:  # (open until here: a freed block comes back with its rows in it)
        q.close()
    g.close()


@pytest.mark.parametrize("metric", [1, 7])
@pytest.mark.parametrize("V", [MS_MAX_V + 1, 20480, 20481])
def test_matrix_past_the_plan(gpu_ready, V, metric, capfd):
    """V = 20,449 and 20,480: the 32-bit frontier double buffer and the
    kernel's static LDS pass 160 KB; V = 20,481: 21 nodes per thread, past
    kMsMaxK.  No MS-BFS plan, no launch line, and the same rows."""
    flags = UNIT if metric == 1 else 0
    net = uniform_net(V, metric, 1000 + V)
    srcs, _ = matrix_sources(net, 32)
    for qs, f in ((srcs, NH | flags), (srcs[::3], flags)):
        q = net.g.query(qs, f)
        assert not q.kernel.startswith("msbfs"), q.kernel
        assert run_logged(q, capfd) == []
        check_all(q, net.g, net.csr, qs, f"V={V} metric={metric} {q.kernel}")
        check_query(net.csr, q, qs, metric != 1, rows={0, 3, 6} if f & NH else {0, 1, 2})
        q.close()
    net.g.close()


# ------------------------------------------------------------ B. general form


def ignore_batch(V, seed):
    """test_msbfs_ignore_lists' batch at any size: 60 random sources and one
    source 70 times, lists of 0, 1, 3, 20 and 200 links, ids past the graph,
    nq = 130 (no multiple of 32 or 64), and at the repeated source two
    parallel links with one, then both of them ignored."""
    rng = random.Random(seed)
    links = random_links(rng, V, 10 * V // 3, wmin=3, wmax=3, parallel=0.05, asym=False)
    par = len(links)
    links += [(7, V // 2, 3, 3), (7, V // 2, 3, 3)]
    ov = np.zeros(V, dtype=np.uint8)
    ov[rng.sample(range(V), V // 50)] = 1
    ov[7] = 0
    csr = abi.Csr.from_links(V, links, overloaded=ov)
    srcs = [rng.randrange(V) for _ in range(60)] + [7] * 70
    ign = []
    for i in range(len(srcs)):
        k = rng.choice([0, 1, 3, 20, 200])
        ign.append(rng.sample(range(len(links)), k) + ([len(links) + 5] if i % 9 == 0 else []))
    own = sorted({int(l) for l in csr.link_id[csr.row_ptr[7]:csr.row_ptr[8]]} - {par, par + 1})
    ign[64] = [par]
    ign[100] = [par, par + 1]
    ign[129] = own  # only the parallel pair is left
    assert {len(l) for l in ign} >= {0, 1, 3, 20, 200}
    return csr, srcs, ign


@pytest.mark.parametrize("case", [("32", 1500), (None, 10241), (None, 16385), (None, 4097),
                                  (None, 8193)], ids=_case_id)
def test_ignore_masks(gpu_ready, case, monkeypatch, capfd):
    """Distance-only batches with ignore lists: the 64-bit mask words narrowed
    to a 32-bit batch (~(MT)m[e]; spf_ms_ign_kernel with 32 queries per
    batch), and 64-bit batches at KMAX 8 and 10.  Every row equals the
    per-query kernels', every summary the oracle's with the same lists."""
    knob, V = case
    if knob:
        monkeypatch.setenv("OPENR_SPF_MSBFS", knob)
    B = width_of(V, knob)
    csr, srcs, ign = ignore_batch(V, 70 + V)
    g = abi.Graph(csr)
    q = g.query(srcs, 0, ignore=ign)
    assert q.kernel == "msbfs"
    one_launch(run_logged(q, capfd), B, kmax_of(B, V), 1, 1, nbatch=(len(srcs) + B - 1) // B,
               tables=1)
    monkeypatch.setenv("OPENR_SPF_MSBFS_IGN", "0")
    r = g.query(srcs, 0, ignore=ign)
    assert not r.kernel.startswith("msbfs"), r.kernel
    r.run()
    same_image(image(r), image(q), f"V={V} B={B} per-query kernels vs ignore masks")
    check_all(q, g, csr, srcs, f"V={V} B={B} ignore masks", ign=ign)
    check_query(csr, q, srcs, True, ignore=ign, rows={64, 100, 129})
    q.close()
    r.close()
    g.close()


WREC = [(None, 4096), (None, 5000), (None, 9000), (None, 11000), (None, 14000), (None, 18000),
        ("32", 1023), ("32", 5000)]


@pytest.mark.parametrize("case", WREC, ids=_case_id)
def test_wave_recorded_rows(gpu_ready, case, monkeypatch, capfd):
    """OPENR_MS_WREC=1 (the general instance's wave-cooperative row stores),
    over the sliced copy and over the plain CSR.  Each form runs as a query
    of its own, and all of the test's queries stay open to its end (a freed
    block would be handed to the next query with its rows in it), so no
    result byte is left over from another run; every one equals the oracle,
    and its rows and masks are byte-equal to the default run's."""
    knob, V = case
    if knob:
        monkeypatch.setenv("OPENR_SPF_MSBFS", knob)
    B = width_of(V, knob)
    kmax = kmax_of(B, V)
    net = uniform_net(V, 7, 2000 + V)
    srcs, _ = matrix_sources(net, B)
    held = []
    for qs, f in ((srcs, NH), (srcs[::3], 0)):
        q = net.g.query(qs, f)
        one_launch(run_logged(q, capfd), B, kmax, 1, 0)
        what = f"V={V} B={B} wave-recorded rows"
        check_all(q, net.g, net.csr, qs, what)
        first = image(q)
        want = oracle(net.csr, qs, f & NH)
        monkeypatch.setenv("OPENR_MS_WREC", "1")
        held.append(q)
        for sell in (1, 0):
            monkeypatch.setenv("OPENR_MS_SELL", str(sell))
            w = net.g.query(qs, f)
            held.append(w)
            one_launch(run_logged(w, capfd), B, kmax, sell, 1)
            check_all(w, net.g, net.csr, qs, f"{what} sell={sell}", want=want)
            same_image(first, image(w), f"{what} sell={sell}")
        monkeypatch.delenv("OPENR_MS_WREC")
        monkeypatch.delenv("OPENR_MS_SELL")
    for w in held:
        w.close()
    net.g.close()


def test_zero_closure_32bit(gpu_ready, monkeypatch, capfd):
    """The zero-metric closure (ms_zero_close) in 32-bit batches: the smallest
    graph of tests/test_zero_metric_plan.py under OPENR_SPF_MSBFS=32."""
    from .test_zero_metric_plan import _same_as_wide, _zero_graph

    monkeypatch.setenv("OPENR_SPF_MSBFS", "32")
    rng = random.Random(1)
    V = 260
    csr, ends = _zero_graph(rng, V, 700, 1, 1)
    g = abi.Graph(csr)
    sources = list(range(V))
    q = g.query(sources, NH)
    assert q.kernel == "msbfs0+levels"
    one_launch(run_logged(q, capfd), 32, 4, 1, 1, nbatch=(V + 31) // 32, tables=2)
    check_query(csr, q, sources, True, rows=set(ends) | set(rng.sample(range(V), 40)))
    _same_as_wide(csr, q, sources, monkeypatch)
    d = g.query(sources[::2], 0)
    assert d.kernel == "msbfs0"
    one_launch(run_logged(d, capfd), 32, 4, 1, 1, nbatch=(V // 2 + 31) // 32, tables=1)
    check_query(csr, d, sources[::2], True, rows=set(range(0, V // 2, 10)))
    _same_as_wide(csr, d, sources[::2], monkeypatch)
    g.close()


def test_zero_closure_kmax12(gpu_ready, monkeypatch, capfd):
    """The zero-metric plan past 10,240 nodes: its limit is the 32-bit
    batch's (V <= 20,448), so the planner keeps it and the batches are 32
    wide, 11 nodes per thread.  Both ends of the metric-0 link are sources."""
    from .test_zero_metric_plan import _same_as_wide, _zero_graph

    rng = random.Random(3)
    V = 11000
    csr, ends = _zero_graph(rng, V, 3 * V, 1, 1, ov_frac=0.02)
    g = abi.Graph(csr)
    sources = list(ends) + [0, V - 1, 10 * SLOT + 5] + rng.sample(range(1, V - 1), 59)
    q = g.query(sources, NH)
    assert q.kernel == "msbfs0+levels"
    line = one_launch(run_logged(q, capfd), 32, 12, 1, 1, tables=2)
    assert line["nbatch"] >= 3  # (the sources' neighbours ride along)
    check_query(csr, q, sources, True, rows={0, 1, 2, 4})
    _same_as_wide(csr, q, sources, monkeypatch, rows=set(range(0, len(sources), 4)) | {1})
    g.close()


def test_blocked_batches_32bit(gpu_ready, monkeypatch, capfd):
    """tests/test_whatif_firsthop_gpu.py's "blocked" form under
    OPENR_SPF_MSBFS=32: the nested batch names one blocked node per 32 rows
    (per = ms_bits / 32 of spf_query_create)."""
    from .test_whatif_firsthop_gpu import FH, _lists, _reference, _same, _uniform_graph

    monkeypatch.setenv("OPENR_SPF_MSBFS", "32")
    monkeypatch.setenv("OPENR_SPF_WHATIF_FIRSTHOP_BLOCKED", "1")
    rng, links, ov, s = _uniform_graph(41)
    csr = abi.Csr.from_links(len(ov), links, overloaded=ov)
    g = abi.Graph(csr)
    L = int(csr.link_id.max()) + 1
    ign = _lists(rng, csr, s, L)
    ign2 = _lists(rng, csr, 7, L)
    qs = [s] * len(ign) + [7] * len(ign2)
    ign = ign + ign2
    q = g.query(qs, NH, ignore=ign)
    lines = run_logged(q, capfd)
    assert FH in q.kernels(), q.kernels()
    nested = [l for l in lines if l["blocked"]]
    # each source's neighbours are padded to whole 64-row batches: 2 x 2 of 32
    assert len(nested) == 1 and nested[0]["bits"] == 32 and nested[0]["gen"] == 0, lines
    assert nested[0]["nbatch"] == 4 and nested[0]["kmax"] == 4, lines
    r = _reference(g, qs, NH, ign, monkeypatch)
    _same(q, r, len(qs))
    n1 = len(qs) - len(ign2)
    check_query(csr, q, qs, True, ignore=ign, rows={0, 1, n1 - 1, n1, len(qs) - 1})
    g.close()


# ------------------------------------------------------------- C. carry-over


@pytest.mark.parametrize("knob", [None, "32"], ids=["b64", "b32"])
def test_carry_over_small(gpu_ready, cus, knob, monkeypatch, capfd):
    """V = 1,100: nq = 2 B grid + B + 1 sources cycling over all nodes, so
    every workgroup runs a second batch, one a third, and the last batch is
    partial.  With next hops, with distances alone, and with per-query ignore
    lists (the general form)."""
    if knob:
        monkeypatch.setenv("OPENR_SPF_MSBFS", knob)
    V, B = 1100, 32 if knob else 64
    rng = random.Random(300 + B)
    links = random_links(rng, V, 3300, wmin=2, wmax=2, parallel=0.02, asym=False)
    ov = np.zeros(V, dtype=np.uint8)
    ov[rng.sample(range(V), 22)] = 1
    ov[V - 1] = ov[SLOT] = 1
    csr = abi.Csr.from_links(V, links, overloaded=ov)
    g = abi.Graph(csr)
    grid = 2 * cus  # per_cu = min(2048 / 1024, 160 KB / (2 * 1100 * B / 8))
    nq = 2 * B * grid + B + 1
    srcs = np.arange(nq, dtype=np.uint32) % V
    want = {True: oracle(csr, np.arange(V), True), False: oracle(csr, np.arange(V), False)}
    for f, plan in ((NH, "msbfs+levels"), (0, "msbfs")):
        q = g.query(srcs, f)
        assert q.kernel == plan
        line = one_launch(run_logged(q, capfd), B, 4, 1, 0, grid=grid, tables=1)
        assert line["nbatch"] == 2 * grid + 2 >= 2 * line["grid"] + 1, line
        check_all(q, g, csr, srcs, f"carry-over B={B} {plan}", want=want[bool(f)][srcs])
        for s in (0, B, V - 1):  # first and last occurrence of one source
            same_rows(q, s, s + (nq - 1 - s) // V * V)
        check_query(csr, q, srcs.tolist(), True, rows={nq - 1})
        q.close()
    pool = [[], [5], sorted(rng.sample(range(len(links)), 3)), [len(links) + 2],
            sorted(rng.sample(range(len(links)), 40)), [int(csr.link_id[0])], []]
    ign = [pool[i % len(pool)] for i in range(nq)]
    q = g.query(srcs, 0, ignore=ign)
    assert q.kernel == "msbfs"
    line = one_launch(run_logged(q, capfd), B, 4, 1, 1, grid=grid, tables=1)
    assert line["nbatch"] >= 2 * line["grid"] + 1, line
    check_all(q, g, csr, srcs, f"carry-over B={B} ignore lists", ign=ign)
    check_query(csr, q, srcs.tolist(), True, ignore=ign, rows={2, nq - 1})
    g.close()


def test_carry_over_production(gpu_ready, cus, capfd):
    """All sources of a max(10241, 64 CUs + 33)-node graph: batches of 32 on
    one workgroup per CU, every workgroup runs at least two.  Then two more
    runs of the same query: the level-flag words alternate per launch."""
    V = max(10241, 64 * cus + 33)
    assert V <= MS_MAX_V, f"{cus} CUs: {V} nodes are past the MS-BFS plan's {MS_MAX_V}"
    net = uniform_net(V, 1, 4000)
    srcs = np.arange(V, dtype=np.uint32)
    q = net.g.query(srcs, NH)
    assert q.kernel == "msbfs+levels"
    line = one_launch(run_logged(q, capfd), 32, kmax_of(32, V), 1, 0, nbatch=(V + 31) // 32,
                      tables=1)
    assert line["grid"] == cus and line["nbatch"] >= 2 * line["grid"] + 1, line
    check_all(q, net.g, net.csr, srcs, f"all {V} sources")
    rows = {0, net.drained, V - 1}
    check_query(net.csr, q, srcs.tolist(), True, rows=rows)
    for _ in range(2):
        one_launch(run_logged(q, capfd), 32, kmax_of(32, V), 1, 0)
        check_query(net.csr, q, srcs.tolist(), True, rows=rows)
    net.g.close()


# ------------------------------------------------------------ D. deep levels


@pytest.mark.parametrize("chain", [130, 300])
def test_deep_levels_kmax12(gpu_ready, chain, capfd):
    """V = 10,241: a chain hangs off node 10,240, the one node of the last
    thread slot.  Levels pass 127 (kMsShallowLevel: the next-hop pass leaves
    its one-add byte compare) and, with 300 nodes, 254 (the 32-bit rows)."""
    V = 10241
    M = V - 1 - chain  # core 0 .. M - 1, chain M .. V - 2, its head V - 1
    rng = random.Random(500 + chain)
    links = random_links(rng, M, 3 * M, wmin=3, wmax=3, parallel=0.01, asym=False)
    attach = rng.randrange(1, M)
    links.append((attach, V - 1, 3, 3))
    links += [(v + 1, v, 3, 3) for v in range(M, V - 1)]  # V-1 - V-2 - ... - M
    ov = np.zeros(V, dtype=np.uint8)
    ov[rng.sample(range(1, M), M // 50)] = 1
    ov[attach] = 0
    csr = abi.Csr.from_links(V, links, overloaded=ov)
    g = abi.Graph(csr)
    srcs = [M, 0, V - 1, M + chain // 2] + rng.sample(range(1, M), 36)
    q = g.query(srcs, NH)
    assert q.kernel == "msbfs+levels"
    one_launch(run_logged(q, capfd), 32, 12, 1, 0, tables=1)
    far = q.dist(0)
    assert int(far[V - 1]) == 3 * chain
    assert int(far[far != np.uint64(abi.SPF_UNREACHABLE)].max()) > 3 * (chain + 2)
    check_all(q, g, csr, srcs, f"chain of {chain}")
    check_query(csr, q, srcs, True, rows={0, 1, 5})
    d = g.query(srcs, 0)
    assert d.kernel == "msbfs"
    one_launch(run_logged(d, capfd), 32, 12, 1, 0, nbatch=2, tables=1)
    check_all(d, g, csr, srcs, f"chain of {chain}, distances")
    g.close()
