"""CPU: the sample geometry the knot kernel is instantiated by.  fit_knot_launch picks the instantiation of fit_lm_knot_kernel from
the plan's shortest and longest segment (d2d_fit_knot_segments, a host function, returns what it uses): they must be what the
oracle's knot geometry (oracle/fit_knot.py: oracle/fit.py sample_segments) gives, for every K the knot kernel can be asked for."""
import numpy as np
import pytest

KS = range(12, 65)


def _oracle_lengths(K):
    from oracle import fit as F
    _, seg, _, _ = F.sample_segments(K, 6, 0.1 * (K - 1))
    return np.bincount(seg, minlength=6)


@pytest.mark.parametrize('K', KS)
def test_host_segment_range_is_the_oracles(K):
    import d2dhip
    n = _oracle_lengths(K)
    k0, smin, smax, floor = d2dhip.knot_segments(6, K, 0.1 * (K - 1))
    assert k0.tolist() == np.concatenate([[0], np.cumsum(n)]).tolist()
    assert (smin, smax) == (int(n.min()), int(n.max()))
    # the one instantiated floor: every segment holds eight samples or more from K = 48 on
    assert floor == (8 if n.min() >= 8 else 0) == (8 if K >= 48 else 0)


def test_the_geometries_the_gpu_test_covers():
    """tests/test_gpu_knot_segmin.py picks its K from these facts: no K <= 64 has segments that differ by two samples; K = 48 is
    the first with the floor and has equal segments; the SEG9 boundary (longest segment 9 -> 10) lies between K = 54 and 55."""
    n = {K: _oracle_lengths(K) for K in KS}
    assert max(int(v.max() - v.min()) for v in n.values()) == 1
    assert n[48].tolist() == [8] * 6 and n[47].min() == 7
    assert n[54].max() == 9 and n[55].max() == 10 and n[55].min() == 9
    assert n[50].tolist() == [9, 8, 8, 8, 8, 9]


def test_bad_arguments_are_refused():
    import d2dhip
    for S, K, dur in ((0, 50, 4.9), (7, 50, 4.9), (6, 1, 4.9), (6, 50, 0.0)):
        with pytest.raises(d2dhip.D2DError):
            d2dhip.knot_segments(S, K, dur)
