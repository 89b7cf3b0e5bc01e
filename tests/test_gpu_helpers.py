"""GPU: the single-evaluation entry points (d2d_flatness, d2d_cont_jac, d2d_gvf_eval, d2d_dcf_eval, d2d_lqr) and the fit helpers
(d2d_fit_project, d2d_fit_coeffs, d2d_fit_sample) through ctx.lib.d2d_* directly, at batch sizes around the wave and block edges
(tests/helper_cases.py), against the oracle element by element -- with the tolerances tests/test_gpu_mirror.py and
tests/test_gpu_fit.py hold the same quantities to at n = 1 -- and against themselves: element i of a batch is, bit for bit, the
n = 1 call on the same input.  Every output is a view into a larger device buffer filled with a sentinel, GUARD doubles in front
and behind, and every input a view with GUARD finite doubles around it.  GUARD is larger than a block of the widest kernel here
(256 threads), so even a launch without its `i >= n` guard stays inside the test's own allocations: a stray write is a failed
assertion here, not a fault."""
import ctypes as C

import numpy as np
import pytest

import helper_cases as HC
from oracle import fit as F

pytestmark = pytest.mark.gpu

GUARD = 320                             # > 256 threads of a block (and >= the 64 that would catch an off-by-one)
SENT = -6.0221407e300                   # no kernel here computes it
EINVAL = -1                             # include/d2d.h D2D_EINVAL


@pytest.fixture(scope='module')
def ctx():
    import d2dhip
    c = d2dhip.Context(0)
    yield c
    c.close()


class Out:
    """An output of `shape` doubles inside a sentinel-filled device buffer."""

    def __init__(self, ctx, *shape):
        import torch
        self.size = int(np.prod(shape))
        self.buf = torch.full((GUARD + self.size + GUARD,), SENT, dtype=torch.float64, device=ctx.device)
        self.view = self.buf[GUARD:GUARD + self.size]
        self.shape = shape
        self.ptr = C.c_void_p(self.view.data_ptr())

    def host(self):
        """The output, after checking that both guards are intact and every element was written."""
        b = self.buf.cpu().numpy()
        assert (b[:GUARD] == SENT).all() and (b[GUARD + self.size:] == SENT).all(), 'a write outside the output'
        got = b[GUARD:GUARD + self.size]
        assert (got != SENT).all(), 'output elements %s never written' % np.flatnonzero(got == SENT)[:8]
        return got.reshape(self.shape).copy()

    def untouched(self):
        return bool((self.buf == SENT).all().item())


def _dp(ctx, a):
    """(buffer, pointer) of a device copy of `a` with GUARD ones in front of it and behind."""
    a = np.ascontiguousarray(a, dtype=np.float64).reshape(-1)
    t = ctx.dev(np.concatenate([np.ones(GUARD), a, np.ones(GUARD)]))
    return t, C.c_void_p(t.data_ptr() + 8 * GUARD)


def _hp(a):
    return a.ctypes.data_as(C.c_void_p)


def _ok(ctx, rc):
    assert rc == 0, (rc, ctx.lib.d2d_last_error().decode())
    ctx.sync()


def _refused(ctx, rc, who, *outs):
    assert rc == EINVAL, (who, rc)
    assert who in ctx.lib.d2d_last_error().decode(), (who, ctx.lib.d2d_last_error())
    ctx.sync()
    assert all(o.untouched() for o in outs), who


def _used(got, ref, rtol, atol):
    """assert_allclose(got, ref, rtol, atol), returning the largest share of the allowance that was used."""
    np.testing.assert_allclose(got, ref, rtol=rtol, atol=atol)
    return float((np.abs(got - ref) / (atol + rtol * np.abs(ref))).max()) if got.size else 0.0


def _bits(a, b, what):
    assert a.shape == b.shape and a.tobytes() == b.tobytes(), what


# ---- the calls ----------------------------------------------------------------------------------------------------------------
def flatness(ctx, variant, Yref, w, tau_phi, tau_v, xdot=True):
    n = Yref.shape[1]
    keep, py = _dp(ctx, Yref)
    X, U, Xd = Out(ctx, 5, n), Out(ctx, 2, n), Out(ctx, 5, n)
    _ok(ctx, ctx.lib.d2d_flatness(ctx.h, variant, n, py, w[0], w[1], tau_phi, tau_v, X.ptr, U.ptr, Xd.ptr if xdot else None))
    assert xdot or Xd.untouched()
    return X.host(), U.host(), (Xd.host() if xdot else None)


def cont_jac(ctx, Xr, tau_phi, tau_v):
    n = Xr.shape[1]
    keep, px = _dp(ctx, Xr)
    A, B = Out(ctx, 25, n), Out(ctx, 10, n)
    _ok(ctx, ctx.lib.d2d_cont_jac(ctx.h, n, px, tau_phi, tau_v, A.ptr, B.ptr))
    return A.host(), B.host()


def gvf_eval(ctx, X, e, nvec, H, ke, kd):
    n = X.shape[1]
    ins = [_dp(ctx, a) for a in (X, e, nvec, H)]
    U = Out(ctx, 3, n)
    _ok(ctx, ctx.lib.d2d_gvf_eval(ctx.h, n, *[p for _, p in ins], ke, kd, U.ptr))
    return U.host()


def dcf_eval(ctx, n_ac, B, z_des, kr, centres, pos, eth=True):
    N = pos.shape[1]
    n_form = N // n_ac
    B, z_des = np.ascontiguousarray(B, dtype=np.float64), np.ascontiguousarray(z_des, dtype=np.float64)
    ins = [_dp(ctx, centres), _dp(ctx, pos)]
    Ur, E = Out(ctx, N), Out(ctx, n_form * (n_ac - 1))
    _ok(ctx, ctx.lib.d2d_dcf_eval(ctx.h, n_form, n_ac, _hp(B), _hp(z_des), kr, ins[0][1], ins[1][1], Ur.ptr, E.ptr if eth else None))
    assert eth or E.untouched()
    return Ur.host(), (E.host() if eth else None)


def lqr(ctx, A, B, Q, R, want_P=True):
    n = A.shape[1]
    ins = [_dp(ctx, A), _dp(ctx, B)]
    Q, R = np.ascontiguousarray(Q, dtype=np.float64).reshape(25), np.ascontiguousarray(R, dtype=np.float64).reshape(4)
    K, P = Out(ctx, 10, n), Out(ctx, 25, n)
    _ok(ctx, ctx.lib.d2d_lqr(ctx.h, n, ins[0][1], ins[1][1], _hp(Q), _hp(R), K.ptr, P.ptr if want_P else None))
    assert want_P or P.untouched()
    return K.host(), (P.host() if want_P else None)


# ---- against the oracle and against themselves ---------------------------------------------------------------------------------
def test_flatness_both_variants_at_ragged_sizes(ctx):
    """Tolerances: test_gpu_mirror.py test_flatness_maps (variant 0: X, U, Xdot 1e-12 / 1e-12; variant 1: X 1e-12 / 1e-12,
    U 1e-11 / 1e-12)."""
    worst = {}
    for variant in (0, 1):
        for n in HC.NS:
            c = HC.flatness_case(variant, n)
            args = (c['w'], c['tau_phi'], c['tau_v'])
            X, U, Xd = flatness(ctx, variant, c['Yref'], *args)
            u = max(_used(X, c['X'], 1e-12, 1e-12), _used(U, c['U'], 1e-12 if variant == 0 else 1e-11, 1e-12),
                    _used(Xd, c['Xdot'], 1e-12, 1e-12))
            worst[variant] = max(worst.get(variant, 0.0), u)
            X2, U2, _ = flatness(ctx, variant, c['Yref'], *args, xdot=False)      # Xdot = NULL changes nothing else
            _bits(X2, X, ('X without Xdot', variant, n)); _bits(U2, U, ('U without Xdot', variant, n))
            for i in HC.probe_indices(n):
                X1, U1, Xd1 = flatness(ctx, variant, c['Yref'][:, i:i + 1], *args)
                _bits(X1[:, 0], X[:, i], ('X', variant, n, i)); _bits(U1[:, 0], U[:, i], ('U', variant, n, i))
                _bits(Xd1[:, 0], Xd[:, i], ('Xdot', variant, n, i))
    print('flatness vs oracle: largest share of the tolerance used, variant 0: %.2e, variant 1: %.2e' % (worst[0], worst[1]))


def test_cont_jac_at_ragged_sizes(ctx):
    """Tolerances: test_gpu_mirror.py test_aircraft_disc_dyn_and_jac (A 1e-13 / 1e-13, B rtol 1e-15)."""
    worst = 0.0
    for n in HC.NS:
        c = HC.cont_jac_case(n)
        A, B = cont_jac(ctx, c['Xr'], c['tau_phi'], c['tau_v'])
        worst = max(worst, _used(A, c['A'], 1e-13, 1e-13))
        np.testing.assert_allclose(B, c['B'], rtol=1e-15)
        for i in HC.probe_indices(n):
            A1, B1 = cont_jac(ctx, c['Xr'][:, i:i + 1], c['tau_phi'], c['tau_v'])
            _bits(A1[:, 0], A[:, i], ('A', n, i)); _bits(B1[:, 0], B[:, i], ('B', n, i))
    print('cont_jac vs oracle: largest share of the tolerance used by A: %.2e' % worst)


def test_gvf_eval_at_ragged_sizes(ctx):
    """Tolerance: test_gpu_mirror.py test_dcf_circle_gvf_helpers (U, U1, U2 1e-11 / 1e-11)."""
    worst = 0.0
    for n in HC.NS:
        c = HC.gvf_case(n)
        U = gvf_eval(ctx, c['X'], c['e'], c['nvec'], c['H'], c['ke'], c['kd'])
        worst = max(worst, _used(U, c['U'], 1e-11, 1e-11))
        for i in HC.probe_indices(n):
            U1 = gvf_eval(ctx, c['X'][:, i:i + 1], c['e'][i:i + 1], c['nvec'][:, i:i + 1], c['H'][:, i:i + 1], c['ke'], c['kd'])
            _bits(U1[:, 0], U[:, i], ('U', n, i))
    print('gvf_eval vs oracle: largest share of the tolerance used: %.2e' % worst)


def test_dcf_eval_formations_edges_and_dense_B(ctx):
    """Tolerances: test_gpu_mirror.py test_dcf_circle_gvf_helpers (U_r and e_theta [deg] 1e-12 / 1e-11); the formations whose
    unwrapped error is exactly +pi, -pi, 2 pi (e > pi and e <= -pi wrap: pi, pi, 0) are compared exactly.  A formation alone
    (n_form = 1) gives the bits it gives anywhere in a batch; eth_deg = NULL changes nothing in U_r."""
    worst, n_edge, n_out = 0.0, 0, 0
    for c in HC.dcf_cases():
        n_form, n_ac, nm = c['n_form'], c['n_ac'], c['n_ac'] - 1
        args = (n_ac, c['B'], c['z_des'], c['kr'])
        Ur, eth = dcf_eval(ctx, *args, c['centres'], c['pos'])
        worst = max(worst, _used(Ur, c['U_r'], 1e-12, 1e-11), _used(eth, c['eth_deg'], 1e-12, 1e-11))
        n_out += int((np.abs(eth) > 180.0).sum())
        for f, kind in c['edges']:
            np.testing.assert_array_equal(eth[f * nm:(f + 1) * nm], c['eth_deg'][f * nm:(f + 1) * nm])
            np.testing.assert_array_equal(Ur[f * n_ac:(f + 1) * n_ac], c['U_r'][f * n_ac:(f + 1) * n_ac])
            assert eth[f * nm] == (180.0, 180.0, 0.0)[kind]
            n_edge += 1
        Ur2, _ = dcf_eval(ctx, *args, c['centres'], c['pos'], eth=False)
        _bits(Ur2, Ur, ('U_r without eth_deg', n_form, n_ac))
        for f in sorted(set(HC.probe_indices(n_form)) | {f for f, _ in c['edges']}):
            s = slice(f * n_ac, (f + 1) * n_ac)
            Ur1, eth1 = dcf_eval(ctx, *args, c['centres'][:, s], c['pos'][:, s])
            _bits(Ur1, Ur[s], ('U_r', n_form, n_ac, f)); _bits(eth1, eth[f * nm:(f + 1) * nm], ('eth_deg', n_form, n_ac, f))
    assert n_edge >= 3 * 3 and n_out >= 1
    print('dcf_eval vs oracle: largest share of the tolerance used: %.2e; %d exact edge formations; %d answers outside (-180, 180]'
          % (worst, n_edge, n_out))


def test_lqr_around_the_wavefront(ctx):
    """Tolerances: test_gpu_mirror.py test_lqr_vs_scipy_care (P 1e-8 rel / 1e-8 |P|max, K 1e-7 / 1e-8 |P|max).  No n = 1 identity
    here: a lane's doubling count depends on its wave companions (sim_device.h sda_doubling).  P = NULL leaves K bit-identical."""
    worst = 0.0
    for n in HC.NS_LQR:
        c = HC.lqr_case(n)
        K, P = lqr(ctx, c['A'], c['B'], c['Q'], c['R'])
        assert np.isfinite(K).all() and np.isfinite(P).all()
        for i in range(n):
            pm = np.abs(c['P'][:, i]).max()
            worst = max(worst, _used(P[:, i], c['P'][:, i], 1e-8, 1e-8 * pm), _used(K[:, i], c['K'][:, i], 1e-7, 1e-8 * pm))
        K2, _ = lqr(ctx, c['A'], c['B'], c['Q'], c['R'], want_P=False)
        _bits(K2, K, ('K without P', n))
    print('lqr vs scipy CARE: largest share of the tolerance used: %.2e' % worst)


def test_incidence_buffer_is_not_shared_between_callers(ctx):
    """d2d_dcf_eval and the formation loop both upload B and z_des into ctx->Bmat_dev (sim_kernels.hip upload_Bz): a dcf_eval with
    another n_ac and B between two identical gvf_run calls changes nothing in the second; and n_ac = 4, 64, 4 on a fresh context
    (the buffer grows, then holds stale words behind the 15 that n_ac = 4 uploads) answers the same bits first and last."""
    import d2dhip
    r = np.random.default_rng(5)
    n_ac, n_form = 5, 3
    N = n_ac * n_form
    cen = r.uniform(-40, 40, (2, N)); X0 = np.stack([cen[0] + 50, cen[1], np.full(N, np.pi / 2), np.zeros(N), np.full(N, 12.0)])
    dev = [ctx.dev(X0), ctx.dev(cen), ctx.dev(np.full(N, 60.0))]
    run = lambda: {k: v.cpu().numpy() for k, v in ctx.gvf_run(*dev, n_ac, 40, 0.05, 15.0).items() if k in ('X', 'U', 'Rr', 'eth')}   # noqa: E731
    first = run()
    d3 = HC.dcf_case(4, 3, dense=True)
    dcf_eval(ctx, 3, d3['B'], d3['z_des'], d3['kr'], d3['centres'], d3['pos'])
    again = run()
    assert np.abs(first['eth']).max() > 0 and np.isfinite(first['X']).all()
    for k in first:
        _bits(again[k], first[k], k)
    fresh = d2dhip.Context(0)
    try:
        c4, c64 = HC.dcf_case(255, 4), HC.dcf_case(1, 64)
        a = dcf_eval(fresh, 4, c4['B'], c4['z_des'], c4['kr'], c4['centres'], c4['pos'])
        Ur64, _ = dcf_eval(fresh, 64, c64['B'], c64['z_des'], c64['kr'], c64['centres'], c64['pos'])
        b = dcf_eval(fresh, 4, c4['B'], c4['z_des'], c4['kr'], c4['centres'], c4['pos'])
    finally:
        fresh.close()
    np.testing.assert_allclose(Ur64, c64['U_r'], rtol=1e-12, atol=1e-11)
    np.testing.assert_allclose(a[0], c4['U_r'], rtol=1e-12, atol=1e-11)
    _bits(b[0], a[0], 'U_r after the regrow'); _bits(b[1], a[1], 'eth_deg after the regrow')


def test_refusals_name_the_entry_point_and_write_nothing(ctx, fit_plans):
    lib, h = ctx.lib, ctx.h
    f, j, g, l = HC.flatness_case(0, 63), HC.cont_jac_case(63), HC.gvf_case(63), HC.lqr_case(63)
    d = HC.dcf_case(1, 2)
    (kY, pY), (kX, pXr) = _dp(ctx, f['Yref']), _dp(ctx, j['Xr'])
    X, U, Xd, A, B, Ug, K, P, Ur, E = (Out(ctx, 5, 63), Out(ctx, 2, 63), Out(ctx, 5, 63), Out(ctx, 25, 63), Out(ctx, 10, 63), Out(ctx, 3, 63),
                                      Out(ctx, 10, 63), Out(ctx, 25, 63), Out(ctx, 65), Out(ctx, 64))
    _refused(ctx, lib.d2d_flatness(h, 0, 0, pY, 0.0, 0.0, 0.01, 1.0, X.ptr, U.ptr, Xd.ptr), 'd2d_flatness', X, U, Xd)
    _refused(ctx, lib.d2d_flatness(h, 2, 63, pY, 0.0, 0.0, 0.01, 1.0, X.ptr, U.ptr, Xd.ptr), 'd2d_flatness', X, U, Xd)
    _refused(ctx, lib.d2d_cont_jac(h, 0, pXr, 0.01, 1.0, A.ptr, B.ptr), 'd2d_cont_jac', A, B)
    _refused(ctx, lib.d2d_cont_jac(h, 63, pXr, 0.0, 1.0, A.ptr, B.ptr), 'd2d_cont_jac', A, B)
    gi = [_dp(ctx, g[k]) for k in ('X', 'e', 'nvec', 'H')]
    _refused(ctx, lib.d2d_gvf_eval(h, 0, *[p for _, p in gi], g['ke'], g['kd'], Ug.ptr), 'd2d_gvf_eval', Ug)
    li = [_dp(ctx, l['A']), _dp(ctx, l['B'])]
    Q, R = np.ascontiguousarray(l['Q']).reshape(25), np.ascontiguousarray(l['R']).reshape(4)
    _refused(ctx, lib.d2d_lqr(h, 0, li[0][1], li[1][1], _hp(Q), _hp(R), K.ptr, P.ptr), 'd2d_lqr', K, P)
    Rs = np.array([2.0, 1.0, 4.0, 2.0])                                          # singular
    _refused(ctx, lib.d2d_lqr(h, 63, li[0][1], li[1][1], _hp(Q), _hp(Rs), K.ptr, P.ptr), 'd2d_lqr', K, P)
    di = [_dp(ctx, np.zeros((2, 65))), _dp(ctx, np.ones((2, 65)))]
    Bh, zh = np.zeros(65 * 64), np.zeros(64)
    for n_form, n_ac in ((0, 2), (1, 0), (1, 65)):
        _refused(ctx, lib.d2d_dcf_eval(h, n_form, n_ac, _hp(Bh), _hp(zh), d['kr'], di[0][1], di[1][1], Ur.ptr, E.ptr), 'd2d_dcf_eval', Ur, E)
    kind, plan, ob = fit_plans[0]
    c = _fit_case(kind, ob, 3)
    fi = [_dp(ctx, c[k]) for k in ('scen', 'xy', 'q')]
    q, z, Y, Xs = Out(ctx, 3, 2 * plan.nq), Out(ctx, 3, 2, plan.S, 8), Out(ctx, 3, 6, plan.K), Out(ctx, 3, 5, plan.K)
    _refused(ctx, lib.d2d_fit_project(h, plan.h, 0, fi[0][1], fi[1][1], q.ptr), 'd2d_fit_project', q)
    _refused(ctx, lib.d2d_fit_coeffs(h, plan.h, 0, fi[0][1], fi[2][1], z.ptr), 'd2d_fit_coeffs', z)
    _refused(ctx, lib.d2d_fit_sample(h, plan.h, 0, fi[0][1], fi[2][1], Y.ptr, Xs.ptr), 'd2d_fit_sample', Y, Xs)
    del kY, kX, gi, li, di, fi


# ---- the fit helpers -------------------------------------------------------------------------------------------------------------
FIT_S = 6
FIT_SHAPES = (('fused', 50), ('knot', 57), ('long', 121))       # (plan.kernel, K); K = 57: an odd count of tests/test_gpu_knot.py


@pytest.fixture(scope='module')
def fit_plans(ctx):
    """[(kind, plan, oracle basis fed with the plan's own arrays)] -- one plan of each kernel family."""
    import d2dhip
    out = []
    for kind, K in FIT_SHAPES:
        dur = F.planner_timing(0, 4.9, 10)[2] if K == 50 else (K - 1) / 10.0
        s = 0.1 / K
        plan = d2dhip.FitPlan(ctx, FIT_S, K, dur, (0.02 ** 2, s * 5.0, s / F.G_ACC ** 2), kernel='auto' if kind == 'long' else kind)
        out.append((kind, plan, F.FitBasis.from_arrays(FIT_S, K, dur, *plan.basis())))
    yield out
    for _, plan, _ in out:
        plan.close()


_FIT_CASES = {}


def _fit_case(kind, ob, B):
    """HC.fit_case of a plan kind, built once for the tests that share it."""
    if (kind, B) not in _FIT_CASES:
        _FIT_CASES[kind, B] = HC.fit_case(ob, B)
    return _FIT_CASES[kind, B]


def fit_project(ctx, plan, scen, xy):
    B = len(scen)
    ins = [_dp(ctx, scen), _dp(ctx, xy)]
    q = Out(ctx, B, 2 * plan.nq)
    _ok(ctx, ctx.lib.d2d_fit_project(ctx.h, plan.h, B, ins[0][1], ins[1][1], q.ptr))
    return q.host()


def fit_coeffs(ctx, plan, scen, q):
    B = len(scen)
    ins = [_dp(ctx, scen), _dp(ctx, q)]
    z = Out(ctx, B, 2, plan.S, 8)
    _ok(ctx, ctx.lib.d2d_fit_coeffs(ctx.h, plan.h, B, ins[0][1], ins[1][1], z.ptr))
    return z.host()


def fit_sample(ctx, plan, scen, q, want_Y=True, want_Xs=True):
    B = len(scen)
    ins = [_dp(ctx, scen), _dp(ctx, q)]
    Y, Xs = Out(ctx, B, 6, plan.K), Out(ctx, B, 5, plan.K)
    _ok(ctx, ctx.lib.d2d_fit_sample(ctx.h, plan.h, B, ins[0][1], ins[1][1], Y.ptr if want_Y else None, Xs.ptr if want_Xs else None))
    assert (want_Y or Y.untouched()) and (want_Xs or Xs.untouched())
    return (Y.host() if want_Y else None), (Xs.host() if want_Xs else None)


def test_fit_project_vs_oracle_and_vs_init(ctx, fit_plans):
    """d2d_fit_project of random node positions against F.initial_guess(basis, sc, wp=xy) (tolerance: test_gpu_fit.py
    test_init_eval_vs_oracle holds d2d_fit_init to 1e-9 max(1, |q|max)), at batch sizes around the four trajectories of a block;
    row b of a batch is the B = 1 call bit for bit.

    d2d_fit_project of the oracle's own 'tri' waypoints against d2d_fit_init: fit_project_kernel and fit_init_kernel
    (csrc/fit_kernels.hip) run the same accumulation, acc += Pinit[j][k] * (w[k] - Gp[k] . d), in the same order; what differs is
    where w[k] comes from.  fit_init forms it on the device (fit_device.h load_scen, linspace_at: the apex p2 += h * (-uy) and the
    node i * step + a are contracted into fused multiply-adds, D * D - d * d under the root too), numpy's np.linspace and
    oracle/fit.py triangle round every product.  On the random scenarios the two sets of waypoints therefore differ in their last
    bits and so do the projections (measured on an MI355X: at most 2.8e-14 in q; a first version of this test asserted bit equality
    there and failed at B = 1) -- they are held to the tolerance of d2d_fit_init above.  Where the waypoints are exactly
    representable whatever the evaluation order (HC.fit_lattice_case: integer nodes, no dog-leg) the numbers ARE the same, and
    project equals init bit for bit."""
    worst = dwp = 0.0
    for kind, plan, ob in fit_plans:
        assert plan.kernel == kind
        for B in HC.FIT_BS:
            c = _fit_case(kind, ob, B)
            q = fit_project(ctx, plan, c['scen'], c['xy'])
            for i in range(B):
                tol = 1e-9 * max(1.0, np.abs(c['q_xy'][i]).max())
                worst = max(worst, _used(q[i], c['q_xy'][i], 0.0, tol))
            for i in sorted({0, B // 2, B - 1}):
                _bits(fit_project(ctx, plan, c['scen'][i:i + 1], c['xy'][i:i + 1])[0], q[i], ('project', kind, B, i))
            q_init = plan.init(ctx.dev(c['scen'])).cpu().numpy()
            q_wp = fit_project(ctx, plan, c['scen'], c['wp'])
            dwp = max(dwp, np.abs(q_wp - q_init).max())
            for i in range(B):
                tol = 1e-9 * max(1.0, np.abs(c['q_wp'][i]).max())
                worst = max(worst, _used(q_wp[i], c['q_wp'][i], 0.0, tol), _used(q_wp[i], q_init[i], 0.0, tol))
            lat = HC.fit_lattice_case(ob, B)
            q_init = plan.init(ctx.dev(lat['scen'])).cpu().numpy()
            q_lat = fit_project(ctx, plan, lat['scen'], lat['wp'])
            _bits(q_lat, q_init, ('project of the oracle waypoints vs init', kind, B))
            for i in range(B):
                worst = max(worst, _used(q_lat[i], lat['q_wp'][i], 0.0, 1e-9 * max(1.0, np.abs(lat['q_wp'][i]).max())))
    print('fit_project vs oracle: largest share of the tolerance used: %.2e; project(oracle waypoints) vs init on the random rows: '
          '%.1e in q, on the lattice rows: bit-identical' % (worst, dwp))


def test_fit_coeffs_and_sample_vs_oracle(ctx, fit_plans):
    """d2d_fit_coeffs against F.coefficients, d2d_fit_sample against F.flat_outputs and F.flatness, every other row in a wind
    (tolerances: test_gpu_fit.py test_cost_vs_reference_classes_golden -- z 1e-9 |z|max, the states 1e-8 / 1e-8, the flat outputs
    1e-9 / 1e-8).  Y = NULL and Xs = NULL, each alone, leave the other output bit-identical; row b of a batch is the B = 1 call."""
    wz = wx = wy = 0.0
    for kind, plan, ob in fit_plans:
        assert plan.kernel == kind
        for B in HC.FIT_BS:
            c = _fit_case(kind, ob, B)
            z = fit_coeffs(ctx, plan, c['scen'], c['q'])
            Y, Xs = fit_sample(ctx, plan, c['scen'], c['q'])
            for i in range(B):
                wz = max(wz, _used(z[i], c['z'][i], 0.0, 1e-9 * np.abs(c['z'][i]).max()))
            wx = max(wx, _used(Xs, c['Xs'], 1e-8, 1e-8)); wy = max(wy, _used(Y, c['Y'], 1e-9, 1e-8))
            _, Xs2 = fit_sample(ctx, plan, c['scen'], c['q'], want_Y=False)
            Y2, _ = fit_sample(ctx, plan, c['scen'], c['q'], want_Xs=False)
            _bits(Xs2, Xs, ('Xs without Y', kind, B)); _bits(Y2, Y, ('Y without Xs', kind, B))
            for i in sorted({0, B // 2, B - 1}):
                Y1, Xs1 = fit_sample(ctx, plan, c['scen'][i:i + 1], c['q'][i:i + 1])
                _bits(Y1[0], Y[i], ('Y', kind, B, i)); _bits(Xs1[0], Xs[i], ('Xs', kind, B, i))
                _bits(fit_coeffs(ctx, plan, c['scen'][i:i + 1], c['q'][i:i + 1])[0], z[i], ('z', kind, B, i))
    print('fit_coeffs / fit_sample vs oracle: largest share of the tolerance used, z: %.2e, Xs: %.2e, Y: %.2e' % (wz, wx, wy))
