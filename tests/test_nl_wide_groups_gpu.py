"""Wide shared groups of the v2 next-hop pass (the default;
OPENR_NL_WIDE_GROUPS=0 forms none; DESIGN.md §6 "Round 15"): wide sources
whose neighbour lists agree on at
least half of their 8-entry blocks share one block of
spf_nh_levels_v2_kernel, which loads the agreeing blocks' level words once.

Every case runs all sources with next hops through the MS-BFS plan and
  * asserts from the item counts (the [build_nl_v2] line of
    OPENR_SPF_CREATE_TIMING=1) that wide groups were formed, and none with
    the knob at 0;
  * compares every source's distance row and next-hop sets with the oracle
    (oracle/csr_spf.h summaries: reached, distance sum, next-hop count and a
    hash over every (node, next hop) pair), and a few sources node by node
    with the literal replay (oracle/spf_py.py);
  * compares rows and masks byte for byte with the same query under
    OPENR_NL_WIDE_GROUPS=0.

A group has kNlWS = 2 members (the kernel's register budget, DESIGN), so a
plane of 3 SSWs is one full group and a one-member remainder.
"""

import re

import numpy as np
import pytest

from openr_amd import abi
from openr_amd import topologies as TP
from tests.test_abi_gpu import check_query
from tests.test_config_sized_gpu import _batch_summaries, _check_summary

pytestmark = pytest.mark.gpu

WS = 2  # kNlWS


def _counts(err):
    lines = [l for l in err.splitlines() if l.startswith("[build_nl_v2]")]
    assert lines, err
    return {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", lines[-1])}


def _pair(g, srcs, monkeypatch, capfd):
    """The query with wide groups and the same query without; item counts."""
    monkeypatch.setenv("OPENR_SPF_CREATE_TIMING", "1")
    capfd.readouterr()
    monkeypatch.setenv("OPENR_NL_WIDE_GROUPS", "1")
    a = g.query(srcs, abi.SPF_F_NEXTHOPS)
    ca = _counts(capfd.readouterr().err)
    monkeypatch.setenv("OPENR_NL_WIDE_GROUPS", "0")
    b = g.query(srcs, abi.SPF_F_NEXTHOPS)
    cb = _counts(capfd.readouterr().err)
    monkeypatch.delenv("OPENR_NL_WIDE_GROUPS")
    monkeypatch.delenv("OPENR_SPF_CREATE_TIMING")
    assert cb["wide"] == 0 and cb["wide_members"] == 0, cb
    # the members left the solo items, nothing else moved
    assert ca["group"] == cb["group"] and ca["solo"] + ca["wide_members"] == cb["solo"], (ca, cb)
    return a, b, ca


def _oracle(csr, srcs):
    from oracle import build as OB

    OB.build()
    from oracle import _oracle_ref as O

    return O.csr_spf_summary(csr.row_ptr, csr.col, csr.metric.astype(np.uint64), csr.link_id,
                             csr.overloaded, srcs, None, None, True, True, 8)


def _check(csr, g, a, b, rows, v2=True):
    V = csr.num_nodes
    srcs = np.arange(V, dtype=np.uint32)
    a.run()
    b.run()
    assert a.kernel == "msbfs+levels" and b.kernel == "msbfs+levels"
    assert "spf_nh_levels_v2_kernel" in a.kernels()
    _check_summary(_batch_summaries(a, g, srcs, None), _oracle(csr, srcs), None, "wide groups")
    ra = np.empty((V, V), dtype=np.uint32)
    rb = np.empty((V, V), dtype=np.uint32)
    a.fetch_rows(0, V, ra.ctypes.data, V * 4, on_device=False)
    b.fetch_rows(0, V, rb.ctypes.data, V * 4, on_device=False)
    assert (ra == rb).all()
    ma, mb = a.fetch_nexthops(0, V), b.fetch_nexthops(0, V)
    if not (ma == mb).all():
        bad = int(np.flatnonzero(ma != mb)[0])
        pytest.fail(f"mask word {bad} differs: {ma[bad]:#x} vs {mb[bad]:#x}")
    check_query(csr, a, [int(s) for s in srcs], True, rows=set(rows))
    return ra


def _ids(topo, *names):
    _, by_rank = topo.rank()
    return [by_rank.index(n) for n in names]


@pytest.mark.parametrize("ssw", [WS + 1, 2 * WS])
def test_small_fabric_three_word_ssw_lists(gpu_ready, ssw, monkeypatch, capfd):
    """131 pods of 2 FSWs and 3 RSWs: the SSW lists are 131 long (3 mask
    words, a last block of 3 entries) and identical within a plane; the FSW
    lists (ssw + 3 entries, one block) stay with today's items.  V = 661 or
    663: one chunk, a partly filled last segment, V % 4 != 0.  WS + 1 SSWs
    per plane: one full group and a solo remainder."""
    topo = TP.fabric(2 * ssw + 131 * 5, 2, ssw, 3)
    csr = topo.csr()
    V = csr.num_nodes
    assert V == 2 * ssw + 655 and V % 4 != 0
    g = abi.Graph(csr)
    assert all(len(g.nbrs(s)) == 131 for s in _ids(topo, "1-0-0", f"1-1-{ssw - 1}"))
    a, b, c = _pair(g, np.arange(V, dtype=np.uint32), monkeypatch, capfd)
    per_plane = ssw // WS
    assert c["wide"] == 2 * per_plane and c["wide_members"] == 2 * per_plane * WS, c
    assert c["wide_shared_blocks"] == 17 * c["wide"] and c["wide_private_blocks"] == 0, c
    assert all(a.nh_words(s) == 3 for s in _ids(topo, "1-0-0", "1-1-0"))
    _check(csr, g, a, b, _ids(topo, "1-0-0", f"1-0-{ssw - 1}", "1-1-1", "2-130-1", "3-77-2"))


def _fabric_20_50(extra_names=(), extra_links=(), cut=None):
    """2 planes of 20 SSWs, 22 pods of 2 FSWs and 50 RSWs (V = 1,184: two
    chunks).  An FSW list is 20 SSWs then 50 RSWs: 2 mask words, 9 blocks,
    the pod's shared run starting mid-block at position 20 -- blocks 0-2
    private, 3-8 shared between the pod's two FSWs."""
    topo = TP.fabric(1184, 2, 20, 50)
    assert topo.num_nodes == 1184
    base = len(topo.names)
    topo.names += list(extra_names)
    ix = {n: i for i, n in enumerate(topo.names)}
    topo.links += [(ix[x], ix[y], 1, 1) for x, y in extra_links]
    if cut is not None:
        topo.links = [l for l in topo.links if ix[cut] not in (l[0], l[1])]
    assert len(topo.names) >= base
    return topo


def test_fabric_shared_run_from_mid_block(gpu_ready, monkeypatch, capfd):
    topo = _fabric_20_50()
    csr = topo.csr()
    V = csr.num_nodes
    g = abi.Graph(csr)
    fsw = _ids(topo, "2-0-0", "2-0-1", "2-21-1")
    assert all(len(g.nbrs(s)) == 70 for s in fsw)
    a, b, c = _pair(g, np.arange(V, dtype=np.uint32), monkeypatch, capfd)
    assert c["wide"] == 22 and c["wide_members"] == 44, c
    assert c["wide_shared_blocks"] == 22 * 6 and c["wide_private_blocks"] == 22 * 3, c
    assert all(a.nh_words(s) == 2 for s in fsw)
    _check(csr, g, a, b, fsw + _ids(topo, "1-1-19", "3-21-49"))


@pytest.mark.parametrize("what,name", [
    ("shared neighbour", "3-0-10"),        # position 30 of pod 0's FSW lists: block 3
    ("private neighbour (SSW)", "1-0-5"),  # block 0 of the plane-0 FSW lists
    ("private neighbour (mixed block)", "3-0-1"),  # position 21: block 2
    ("member", "2-0-1"),
])
def test_fabric_drained(gpu_ready, what, name, monkeypatch, capfd):
    topo = _fabric_20_50()
    csr = topo.csr(overloaded=[topo.names.index(name)])
    V = csr.num_nodes
    g = abi.Graph(csr)
    a, b, c = _pair(g, np.arange(V, dtype=np.uint32), monkeypatch, capfd)
    assert c["wide"] == 22 and c["wide_members"] == 44, c
    _check(csr, g, a, b, _ids(topo, name, "2-0-0", "2-0-1", "2-5-0", "3-0-2"))


def test_fabric_node_cut_off(gpu_ready, monkeypatch, capfd):
    """An RSW with no links: unreached in every row (level 255), and its own
    row reaches nothing.  Its pod's FSW lists are one entry shorter."""
    topo = _fabric_20_50(cut="3-3-30")
    csr = topo.csr()
    V = csr.num_nodes
    g = abi.Graph(csr)
    a, b, c = _pair(g, np.arange(V, dtype=np.uint32), monkeypatch, capfd)
    assert c["wide"] == 22 and c["wide_members"] == 44, c
    cutid, f0 = _ids(topo, "3-3-30", "2-3-0")
    rows = _check(csr, g, a, b, [cutid, f0] + _ids(topo, "2-3-1", "2-0-0"))
    assert rows[f0, cutid] == 0xFFFFFFFF and (rows[cutid] != 0xFFFFFFFF).sum() == 1


@pytest.mark.parametrize("chain,v2", [(130, True), (300, False)])
def test_fabric_deep_levels(gpu_ready, chain, v2, monkeypatch, capfd):
    """A chain hung off one RSW.  130 nodes: levels pass 127, so the wide
    groups take the exact compare.  300 nodes: deeper than 254 levels, the
    v2 pass steps aside for spf_nh_levels_swar_kernel as without groups."""
    names = [f"9-0-{i:03d}" for i in range(chain)]
    links = [("3-2-7", names[0])] + list(zip(names, names[1:]))
    topo = _fabric_20_50(names, links)
    csr = topo.csr()
    V = csr.num_nodes
    assert V == 1184 + chain
    g = abi.Graph(csr)
    a, b, c = _pair(g, np.arange(V, dtype=np.uint32), monkeypatch, capfd)
    assert c["wide"] == 22 and c["wide_members"] == 44, c
    far = _ids(topo, names[-1])[0]
    rows = _check(csr, g, a, b, [far] + _ids(topo, "2-2-0", "2-2-1", "2-9-1"))
    depth = int(rows[far][rows[far] != 0xFFFFFFFF].max())
    assert (127 <= depth <= 254) if v2 else depth > 254, depth
    assert "spf_nh_levels_swar_kernel" in a.kernels()


def test_no_wide_groups_with_trit_rows(gpu_ready, monkeypatch, capfd):
    topo = TP.fabric(661, 2, 3, 3)
    csr = topo.csr()
    g = abi.Graph(csr)
    monkeypatch.setenv("OPENR_SPF_CREATE_TIMING", "1")
    monkeypatch.setenv("OPENR_NL_WIDE_GROUPS", "1")
    monkeypatch.setenv("OPENR_NL_TRIT", "1")
    capfd.readouterr()
    q = g.query(np.arange(csr.num_nodes, dtype=np.uint32), abi.SPF_F_NEXTHOPS)
    c = _counts(capfd.readouterr().err)
    assert c["wide"] == 0 and c["wide_members"] == 0, c
    q.run()
    assert "spf_lvl_trit_kernel" in q.kernels()
