"""The zero blocks the knot kernel's factorisation leaves out (csrc/fit_knot.hip nd_panel3_chunk0_zero<KnotMetric>, csrc/fit_phases.h
damped_solve), stated on the oracle (oracle/fit_knot.py).

In the kernel's dense order of the 48 free entries -- knot 0 -> rows 0 .. 3, knot j = 1 .. 5 -> rows 8 j - 4 .. 8 j + 3, knot 6 -> rows
44 .. 47: KnotBasis' knot-major order -- the panels of four rows never straddle a knot, and in every block column of 16 the rows of
panel 3 (12 .. 15, 28 .. 31, 44 .. 47) and the columns of chunk 0 (0 .. 3, 16 .. 19, 32 .. 35) belong to knots that are NOT neighbours.
H_u (first and second order) and the metric Mu are block tridiagonal in the knots, so those three 4 x 4 blocks are EXACTLY zero in both
and in the fp32 Cholesky factor of H_u + par Mu: what the panel's dot products skip is a sum of +-0.

Exactly zero is a statement about the matrices as the kernel forms them: sample by sample from the Hermite tables (H_u), from the banded
Gram matrix of the knot data (Mu).  KnotBasis.eval_normal and KnotBasis.Mu are the same matrices formed THROUGH the dense q statement
(B^T H_q B, B^T B with B from a least-squares solve), exact to rounding only -- 1e-15 of the largest entry in those blocks -- so the
test forms both directly from the oracle's own pieces (the Hermite tables KnotBasis.Hb, F.residuals' partials, F.curvature_blocks,
F.junction_map and F.sample_matrix), checks that they ARE KnotBasis' matrices to rounding, and asserts the exact zeros on them."""
import math

import numpy as np
import pytest

from oracle import fit as F, fit_knot as FK

S_ = 6
N = 8 * S_
BLOCKS = [(slice(16 * b + 12, 16 * b + 16), slice(16 * b, 16 * b + 4)) for b in range(3)]
N_SCEN = 8


def _knot_of(i):
    return 0 if i < 4 else (S_ if i >= N - 4 else 1 + (i - 4) // 8)


@pytest.fixture(scope='module', params=[40, 50, 57, 64])
def setup(request):
    from d2dhip import synth
    K = request.param
    dur = synth.planner_timing(0, (K - 1) / 10.0, 10)[2]
    wref = synth.default_wref(0.1, K)
    basis = F.FitBasis(S_, K, dur, wref)
    kb = FK.KnotBasis(basis)
    sc = synth.synth_scenarios(N_SCEN, seed=7, obj_scale=0.1, K=K, dist_range=(30. * dur / 4.9, 55. * dur / 4.9))
    return K, dur, wref, kb, sc


def _rows(kb):
    """Gu (K, 6, 8 (S+1)): d(x, y, xd, yd, xdd, ydd)(t_k) / d(the full knot vector [knot][axis][4]) -- two knots per sample"""
    Gu = np.zeros((kb.K, 6, FK.NK * (kb.S + 1)))
    for k in range(kb.K):
        s = int(kb.seg[k])
        for d in range(3):
            for a in range(2):
                Gu[k, 2 * d + a, FK.NK * s + 4 * a:FK.NK * s + 4 * a + 4] = kb.Hb[d, k, :4]
                Gu[k, 2 * d + a, FK.NK * (s + 1) + 4 * a:FK.NK * (s + 1) + 4 * a + 4] = kb.Hb[d, k, 4:]
    return Gu


def _direct_hessian(kb, Gu, sc, u, second_order):
    """H_u over the free entries, sample by sample in knot coordinates (what the kernel's MFMA pass accumulates)"""
    basis = kb.basis
    wp = F.waypoints(sc, basis.K, basis.duration)
    q = kb.to_q(sc, u)
    _, D = F.residuals(basis, sc, q, wp, want_jac=True)
    J = np.einsum('kry,kye->kre', D, Gu)
    H = np.einsum('kre,krf->ef', J, J)
    if second_order:
        H = H + np.einsum('kia,kij,kjb->ab', Gu, F.curvature_blocks(basis, sc, q, wp), Gu)
    fi = kb.full_index
    return H[np.ix_(fi, fi)]


def _direct_metric(kb, K, dur, wref):
    """Mu = dsc^-1 Nf^T Mref Nf dsc^-1 per axis (KnotBasis.Mu_ax's closed form), in the knot-major order of both axes"""
    Phi = [F.sample_matrix(K, S_, dur, d) for d in range(3)]
    Nj = F.junction_map(S_, kb.T)
    Nf = Nj[:, kb.free]
    M = sum(w * P.T @ P for w, P in zip(wref, Phi))
    ds = kb.dsc[kb.free]
    Max = (Nf.T @ M @ Nf) / ds[:, None] / ds[None, :]
    nq = len(kb.free)
    Mu2 = np.zeros((2 * nq, 2 * nq))
    Mu2[:nq, :nq] = Max; Mu2[nq:, nq:] = Max
    return Mu2[np.ix_(kb.order, kb.order)]


def test_dense_order_is_four_eight_four(setup):
    """the alignment everything rests on: 4 / 8 x 5 / 4 free entries per knot, in the kernel's dense order"""
    _, _, _, kb, _ = setup
    assert len(kb.full_index) == N and (np.diff(kb.full_index) > 0).all()
    assert [int(e) // FK.NK for e in kb.full_index] == [_knot_of(i) for i in range(N)]
    for rows, cols in BLOCKS:
        kr = {_knot_of(i) for i in range(rows.start, rows.stop)}
        kc = {_knot_of(i) for i in range(cols.start, cols.stop)}
        assert len(kr) == 1 and len(kc) == 1 and abs(kr.pop() - kc.pop()) == 2


def test_metric_is_zero_in_the_skipped_blocks(setup):
    K, dur, wref, kb, _ = setup
    Mu = _direct_metric(kb, K, dur, wref)
    assert np.abs(Mu - kb.Mu).max() <= 1e-11 * np.abs(kb.Mu).max()            # KnotBasis' metric, to rounding
    for rows, cols in BLOCKS:
        assert not Mu[rows, cols].any() and not Mu[cols, rows].any()
        assert np.abs(kb.Mu[rows, cols]).max() <= 1e-13 * np.abs(kb.Mu).max()
    far = np.array([[abs(_knot_of(i) - _knot_of(j)) > 1 for j in range(N)] for i in range(N)])
    assert not Mu[far].any()                                                     # block tridiagonal in the knots


@pytest.mark.parametrize('second_order', [False, True])
def test_hessian_and_factor_are_zero_in_the_skipped_blocks(setup, second_order):
    K, dur, wref, kb, scs = setup
    Mu = _direct_metric(kb, K, dur, wref)
    Gu = _rows(kb)
    far = np.array([[abs(_knot_of(i) - _knot_of(j)) > 1 for j in range(N)] for i in range(N)])
    rng = np.random.default_rng(K)
    for n, sc in enumerate(scs):
        wp = F.waypoints(sc, kb.basis.K, kb.basis.duration)
        u = kb.to_u(sc, F.initial_guess(kb.basis, sc, wp))
        if n % 2:                                        # every other scenario away from the start point (hinge rows wake up)
            u = u + 0.05 * rng.standard_normal(N) * np.abs(u).max()
        H = _direct_hessian(kb, Gu, sc, u, second_order)
        _, _, Hq = kb.eval_normal(sc, u, wp, second_order=second_order)
        assert np.abs(H - Hq).max() <= 1e-9 * np.abs(Hq).max()                 # the oracle's H_u, to rounding
        assert not H[far].any()
        for rows, cols in BLOCKS:
            assert not H[rows, cols].any() and not H[cols, rows].any()
        # the fp32 factor of an SPD instance H_u + par Mu (the exact Hessian may be indefinite: par grows until it is not)
        Lc = None
        for e in range(0, 13):
            A = (H + 10.0 ** e * Mu).astype(np.float32)
            try:
                Lc = np.linalg.cholesky(A)
                break
            except np.linalg.LinAlgError:
                continue
        assert Lc is not None and np.isfinite(Lc).all()
        for rows, cols in BLOCKS:
            assert not A[rows, cols].any()
            assert not Lc[rows, cols].any()
        assert not Lc[far & np.tril(np.ones((N, N), bool))].any()               # no fill outside the knot band
