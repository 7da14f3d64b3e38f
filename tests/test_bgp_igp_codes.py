"""The reduction behind the device's per-node BGP best path (RouteTable.h,
bgpUseIgpMetric; CPU only).

runBestPathSelectionBgp appends an OPENR_IGP_COST entity holding -d(node,
announcer) to both vectors before compareMetricVectors (reference
openr/decision/Decision.cpp:746-766).  That entity has one metric element
and compareMetrics only tests < and >, so the result depends on the two IGP
values only through the sign of their difference: three results per ordered
pair (bgp_igp_pair_codes) stand for every pair of distances, and the device
kernel picks one by that sign.  Checked here against the direct compare with
explicit IGP values, on random vectors with priorities on both sides of 3500,
tie-breakers, version mismatches and unequal metric lengths.
"""

import random

import pytest

from openr_amd import thrift as T

# (priority of a type is fixed, as in tests/randomized.py::_bgp_entries;
# 4000 sorts above the IGP entity's 3500, the others below)
_PRIORITY = {0: 4000, 1: 10, 2: 9, 3: 8, 4: 3900}
_OPS = [T.CompareType.WIN_IF_PRESENT, T.CompareType.WIN_IF_NOT_PRESENT,
        T.CompareType.IGNORE_IF_NOT_PRESENT]
# MetricVectorUtils::CompareResult
WINNER, TIE_WINNER, TIE, TIE_LOOSER, LOOSER, ERROR = range(6)


def _vector(rng, tie_breaker_of):
    metrics = []
    for t in rng.sample(range(5), rng.randint(0, 4)):
        metrics.append(T.createMetricEntity(
            t, _PRIORITY[t], rng.choice(_OPS),
            # mostly a per-type flag (a mismatch between the sides is an ERROR)
            tie_breaker_of[t] if rng.random() < 0.9 else not tie_breaker_of[t],
            [rng.randint(0, 2) for _ in range(1 if rng.random() < 0.85 else 2)]))
    if rng.random() < 0.5:
        rng.shuffle(metrics)  # unsorted input: compareMetricVectors sorts its copies
    return T.MetricVector(0 if rng.random() < 0.95 else 1, metrics)


@pytest.fixture(scope="module")
def E():
    import openr_amd._openr_spf as E

    return E


def test_pair_codes_equal_direct_compare(E):
    rng = random.Random(20260)
    seen = set()
    for _ in range(2000):
        tb = {t: rng.random() < 0.4 for t in range(5)}
        l, r = _vector(rng, tb), _vector(rng, tb)
        codes = E.bgp_igp_pair_codes(l, r)
        assert len(codes) == 3 and all(0 <= c <= 5 for c in codes)
        seen.update(codes)
        for li, ri in ((3, 7), (7, 7), (7, 3), (0, 1)):
            want = E.compare_metric_vectors_with_igp(l, li, r, ri)
            got = codes[0 if li < ri else 1 if li == ri else 2]
            assert got == want, (l, r, li, ri, codes)
    assert seen == {WINNER, TIE_WINNER, TIE, TIE_LOOSER, LOOSER, ERROR}


def test_pair_codes_known_answers(E):
    """Hand-checked cases: IGP decides below a tie-breaker, above priority
    3500 it does not; a version mismatch is an ERROR whatever the distance."""
    tb = T.createMetricEntity(1, 10, T.CompareType.WIN_IF_PRESENT, True, [5])
    tb_low = T.createMetricEntity(1, 10, T.CompareType.WIN_IF_PRESENT, True, [3])
    # a tie-breaker below IGP: the closer wins outright, equal distance: the tie-breaker
    assert E.bgp_igp_pair_codes(T.MetricVector(0, [tb]), T.MetricVector(0, [tb_low])) == (
        WINNER, TIE_WINNER, LOOSER)
    # identical vectors: a TIE at equal distance
    assert E.bgp_igp_pair_codes(T.MetricVector(0, [tb]), T.MetricVector(0, [tb])) == (
        WINNER, TIE, LOOSER)
    # a priority-4000 entity decides before the IGP cost is looked at
    hi = T.createMetricEntity(0, 4000, T.CompareType.WIN_IF_PRESENT, False, [2])
    hi_low = T.createMetricEntity(0, 4000, T.CompareType.WIN_IF_PRESENT, False, [1])
    assert E.bgp_igp_pair_codes(T.MetricVector(0, [hi]), T.MetricVector(0, [hi_low])) == (
        WINNER, WINNER, WINNER)
    # a priority-4000 tie-breaker is overridden by IGP and kept on equal IGP
    hit = T.createMetricEntity(0, 4000, T.CompareType.WIN_IF_PRESENT, True, [2])
    hit_low = T.createMetricEntity(0, 4000, T.CompareType.WIN_IF_PRESENT, True, [1])
    assert E.bgp_igp_pair_codes(T.MetricVector(0, [hit]), T.MetricVector(0, [hit_low])) == (
        WINNER, TIE_WINNER, LOOSER)
    assert E.bgp_igp_pair_codes(T.MetricVector(0, [tb]), T.MetricVector(1, [tb])) == (
        ERROR, ERROR, ERROR)
