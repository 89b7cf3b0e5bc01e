"""GPU parity of every launch variant of the formation loop and of the tracking loop, against oracle/sim.py in fp64.

d2d_sim_gvf_run picks its kernel by n_ac and launch size (csrc/sim_kernels.hip): gvf_run_quad_wide_kernel<NAC> / gvf_run_quad_kernel<NAC>
for n_ac = 1, 2, 4 (the wide one while the launch has at most 4 blocks per CU), gvf_run_kernel for every other size (the unrolled
small_form branch at n_ac = 3, the loop branch above four).  Each test below names the instantiations it reaches.  The tracking loop
and the gain are run at ragged batch sizes with user weights, limits, wind and lags."""
import numpy as np
import pytest

from oracle import sim as S

pytestmark = pytest.mark.gpu

DT, V_C = 0.05, 13.0
GAINS = dict(ke=4e-4, kd=25.0, kr=20.0)
TOL_X, TOL_U, TOL_RR = 1e-8, 1e-9, 1e-7          # as test_gpu_sim.py test_gvf_closed_loop_vs_oracle_and_log


@pytest.fixture(scope='module')
def ctx():
    import d2dhip
    c = d2dhip.Context(0)
    yield c
    c.close()


@pytest.fixture(scope='module')
def n_cu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _planes(a):          # (n, c) -> plane-major (c, n)
    return np.ascontiguousarray(np.asarray(a, float).T)


def _amax(a):
    a = np.asarray(a)
    return np.abs(a).max() if a.size else 0.0


def _fpb(n_ac):
    """Formations per block of the launch: 64-thread blocks when 64 % n_ac == 0, else 256 (d2d_sim_gvf_run)."""
    return (64 if 64 % n_ac == 0 else 256) // n_ac


def _straddler(n_ac):
    """First formation of a block whose lanes cross a 64-lane wave boundary (None when none does)."""
    for fl in range(1, _fpb(n_ac)):
        if (fl * n_ac) // 64 != (fl * n_ac + n_ac - 1) // 64:
            return fl
    return None


def _formations(seed, n_form, n_ac):
    """Own centres, radius and start state per formation; bank angles far from the first bank command (both plant branches)."""
    rng = np.random.default_rng(seed)
    sh = (n_form, n_ac)
    c = rng.uniform(-40, 40, sh + (2,))
    r = rng.uniform(35.0, 70.0, n_form)
    X0 = np.stack([rng.uniform(-80, 80, sh), rng.uniform(-80, 80, sh), rng.uniform(-np.pi, np.pi, sh),
                   rng.uniform(-0.6, 0.6, sh), rng.uniform(9.0, 16.0, sh)], -1)
    return c, r, X0


def _physics(kind, n_ac):
    """'plain': no wind, the default lags, B and z_des; 'wind': wind, tau_phi 0.9667, tau_v != 1, a non-default B and z_des."""
    if kind == 'plain':
        return {}
    rng = np.random.default_rng(1000 + n_ac)
    kw = dict(W=(1.3, -0.9), tau_phi=0.9667, tau_v=0.6)
    if n_ac > 1:
        kw['B'] = S.construct_b_matrix(n_ac) * rng.uniform(0.5, 1.5, (n_ac, n_ac - 1))
        kw['z_des'] = rng.uniform(-0.4, 0.4, n_ac - 1)
    return kw


def _gvf(ctx, c, r, X0, T, gains=GAINS, X0f=None, **kw):
    n_form, n_ac = X0.shape[:2]
    N = n_form * n_ac
    if X0f is not None:
        kw['X0f'] = ctx.dev(_planes(X0f.reshape(N, -1)[:, :3]))
    out = ctx.gvf_run(ctx.dev(_planes(X0.reshape(N, 5))), ctx.dev(_planes(c.reshape(N, 2))), ctx.dev(np.repeat(r, n_ac)),
                      n_ac, T, DT, V_C, **gains, **kw)
    ctx.sync()
    return out


def _oracle(c, r, X0, f, T, gains=GAINS, **kw):
    return S.formation_gvf_run(c[f], r[f], V_C, X0[f], T, DT, **gains, **kw)


def _fetch(out, fs, n_ac):
    """Columns of formations fs, sliced on the device -> host arrays X [rows][F][n_ac][5], U [rows][F][n_ac][2], Rr [rows][F][n_ac],
    eth [rows][F][n_ac-1], X_final [F][n_ac][5], stop_row / conv_row [F]."""
    import torch
    dev = out['X_final'].device
    F = len(fs)
    cols = torch.tensor([f * n_ac + a for f in fs for a in range(n_ac)], device=dev)
    got = {}
    for k, nc in (('X', 5), ('U', 2)):
        if out.get(k) is not None:
            got[k] = out[k].index_select(2, cols).cpu().numpy().reshape(-1, nc, F, n_ac).transpose(0, 2, 3, 1)
    if out.get('Rr') is not None:
        got['Rr'] = out['Rr'].index_select(1, cols).cpu().numpy().reshape(-1, F, n_ac)
    if out.get('eth') is not None:
        ecols = torch.tensor([f * (n_ac - 1) + m for f in fs for m in range(n_ac - 1)], device=dev)
        got['eth'] = out['eth'].index_select(1, ecols).cpu().numpy().reshape(-1, F, n_ac - 1)
    got['X_final'] = out['X_final'].index_select(1, cols).cpu().numpy().reshape(5, F, n_ac).transpose(1, 2, 0)
    fi = torch.tensor(list(fs), device=dev)
    got['stop_row'] = out['stop_row'].index_select(0, fi).cpu().numpy()
    got['conv_row'] = out['conv_row'].index_select(0, fi).cpu().numpy()
    return got


def _check(got, k, ref, rs=1, nan_tail=False, what=''):
    """Formation k of `got` against one oracle run.  Recorded row j holds step j*rs: X, Rr, eth of the steps before the stop row, U
    (the command of that step) of the steps before the last one integrated.  nan_tail: rows from the stop row on were not written."""
    Xo, Uo, Rro, etho, s = ref[:5]
    assert got['stop_row'][k] == s, (what, k, got['stop_row'][k], s)
    X = got['X'][:, k]
    steps = np.arange(X.shape[0]) * rs
    live, ulive = steps < s, steps < s - 1
    d = X[live] - Xo[steps[live]]; d[..., 2] = S.norm_mpi_pi(d[..., 2])
    assert _amax(d) <= TOL_X, (what, k, _amax(d))
    if 'U' in got:
        assert _amax(got['U'][ulive, k] - Uo[steps[ulive]]) <= TOL_U, (what, k, _amax(got['U'][ulive, k] - Uo[steps[ulive]]))
    rl = live & (steps >= 1)                  # (row 0 of Rr / eth is not a step of the loop)
    if 'Rr' in got:
        assert _amax(got['Rr'][rl, k] - Rro[steps[rl]]) <= TOL_RR, (what, k)
    if 'eth' in got:
        assert _amax(got['eth'][rl, k] - etho[steps[rl]]) <= TOL_RR, (what, k)
    d = got['X_final'][k] - Xo[s - 1]; d[..., 2] = S.norm_mpi_pi(d[..., 2])
    assert _amax(d) <= TOL_X, (what, k, 'X_final')
    if nan_tail:
        assert np.isnan(X[~live]).all() and np.isnan(got['U'][~ulive, k]).all(), (what, k)
        assert np.isnan(got['Rr'][~live, k]).all() and np.isnan(got['eth'][~live, k]).all(), (what, k)


# ------------------------------------------------------------------------------------------------------------------------------
# 1. launch matrix
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('phys', ['plain', 'wind'])
@pytest.mark.parametrize('n_ac', [1, 2, 4])
def test_gvf_quad_wide_single_formation_and_partial_block(ctx, n_ac, phys):
    """gvf_run_quad_wide_kernel<1|2|4>: one formation alone, then the same formation first in a launch of one full and one partial block
    (n_ac = 2: an odd number of formations, the last one alone in its quad)."""
    fpb, T = _fpb(n_ac), 300
    n_form = fpb + fpb // 2 + 1
    c, r, X0 = _formations(10 + n_ac, n_form, n_ac)
    kw = _physics(phys, n_ac)
    one = _gvf(ctx, c[:1], r[:1], X0[:1], T, **kw)
    out = _gvf(ctx, c, r, X0, T, **kw)
    fs = [0, fpb - 1, fpb, n_form - 2, n_form - 1]
    got, got1 = _fetch(out, fs, n_ac), _fetch(one, [0], n_ac)
    for k, f in enumerate(fs):
        ref = _oracle(c, r, X0, f, T, **kw)
        _check(got, k, ref, what=(n_ac, phys, f))
        if f == 0:
            _check(got1, 0, ref, what=(n_ac, phys, 'alone'))
    for key in ('X', 'U', 'Rr', 'eth'):                     # the lone formation is the batch's formation 0, bit for bit
        if key in got1:
            assert np.array_equal(got1[key][:, 0], got[key][:, 0], equal_nan=True), key


@pytest.mark.parametrize('n_ac, phys', [(1, 'plain'), (2, 'wind'), (4, 'plain')])
def test_gvf_quad_kernel_past_the_wide_threshold(ctx, n_cu, n_ac, phys):
    """gvf_run_quad_kernel<1|2|4>: one block more than 4 per CU (the wide instantiation ends there), history every 20th row;
    formation 0, the last one and 30 seeded samples against the oracle."""
    fpb, T, rs = _fpb(n_ac), 200, 20
    n_form = 4 * n_cu * fpb + 1
    c, r, X0 = _formations(20 + n_ac, n_form, n_ac)
    kw = _physics(phys, n_ac)
    out = _gvf(ctx, c, r, X0, T, rec_stride=rs, **kw)
    rng = np.random.default_rng(30 + n_ac)
    fs = [0] + sorted(rng.choice(np.arange(1, n_form - 1), 30, replace=False).tolist()) + [n_form - 1]
    got = _fetch(out, fs, n_ac)
    assert got['X'].shape[0] == (T + rs - 1) // rs
    for k, f in enumerate(fs):
        _check(got, k, _oracle(c, r, X0, f, T, **kw), rs, what=(n_ac, f))


@pytest.mark.parametrize('n_ac, n_form, phys', [(3, 90, 'plain'), (5, 53, 'wind'), (8, 11, 'plain'), (33, 9, 'wind'), (64, 2, 'plain')])
def test_gvf_general_kernel_straddling_and_partial_block(ctx, n_ac, n_form, phys):
    """gvf_run_kernel: small_form branch (n_ac = 3) and loop branch (5, 8, 33, 64); 256-thread blocks where 64 % n_ac != 0, so that
    formations straddle a wave boundary (n_ac = 5: formation 12 on lanes 60-64), and a partial last block."""
    fpb, T = _fpb(n_ac), 200
    c, r, X0 = _formations(40 + n_ac, n_form, n_ac)
    kw = _physics(phys, n_ac)
    out = _gvf(ctx, c, r, X0, T, **kw)
    st = _straddler(n_ac)
    if n_ac == 33:
        fs = [st, fpb - 1, n_form - 1]                       # (33 aircraft a formation: three formations of oracle time)
    elif n_ac == 64:
        fs = [n_form - 1]
    else:
        fs = sorted({0, fpb - 1, min(fpb, n_form - 1), n_form - 1} | ({st, st + fpb} & set(range(n_form)) if st else set()))
    assert n_form > fpb or n_ac == 64
    got = _fetch(out, fs, n_ac)
    for k, f in enumerate(fs):
        _check(got, k, _oracle(c, r, X0, f, T, **kw), what=(n_ac, f))


# ------------------------------------------------------------------------------------------------------------------------------
# 2. stop rules and recording
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n_ac, phys', [(2, 'plain'), (4, 'wind')])
def test_gvf_state_stop_rule_quad_rows_stride_and_out_reuse(ctx, n_ac, phys):
    """use_stop 1 on gvf_run_quad_wide_kernel<2|4>: six formations of one wavefront stop on six different rows (targets = the
    oracle's own states at known steps).  Once into buffers of an earlier call pre-filled with NaN (rows from the stop row on stay
    NaN, X_final is the last live row), once with every 7th row recorded."""
    n_form, T, tol = 6, 200, (0.5, 0.5, 0.05)
    assert n_form <= _fpb(n_ac)
    c, r, X0 = _formations(50 + n_ac, n_form, n_ac)
    kw = _physics(phys, n_ac)
    X0f = np.array([_oracle(c, r, X0, f, 42 + 13 * f, **kw)[0][41 + 13 * f] for f in range(n_form)])
    refs = [_oracle(c, r, X0, f, T, X0f=X0f[f], stop_tol=tol, **kw) for f in range(n_form)]
    stops = [ref[4] for ref in refs]
    assert len(set(stops)) == n_form and max(stops) < T, stops
    out = _gvf(ctx, c, r, X0, T, **kw)                      # same shapes, no stop rule: every row written
    for key in ('X', 'U', 'Rr', 'eth', 'X_final'):
        out[key].fill_(float('nan'))
    out2 = _gvf(ctx, c, r, X0, T, X0f=X0f, stop_tol=tol, out=out, **kw)
    assert out2 is out
    got = _fetch(out, range(n_form), n_ac)
    for f in range(n_form):
        _check(got, f, refs[f], nan_tail=True, what=(n_ac, f))
        assert np.array_equal(got['X_final'][f], got['X'][stops[f] - 1, f])
    got7 = _fetch(_gvf(ctx, c, r, X0, T, X0f=X0f, stop_tol=tol, rec_stride=7, **kw), range(n_form), n_ac)
    assert got7['X'].shape[0] == (T + 6) // 7
    for f in range(n_form):
        _check(got7, f, refs[f], rs=7, what=(n_ac, f, 'rs7'))
    assert (got7['conv_row'] == -1).all()                # (no phase-error rule)


def _phase_formations(seed, n_form, n_ac):
    """Aircraft of a formation around nearby centres, phases 3 to 17 degrees apart: the phase errors converge over 5-15 s."""
    rng = np.random.default_rng(seed)
    sh = (n_form, n_ac)
    c = np.repeat(rng.uniform(-30, 30, (n_form, 1, 2)), n_ac, 1) + rng.uniform(-3, 3, sh + (2,))
    r = rng.uniform(40, 60, n_form)
    th = np.cumsum(np.concatenate([rng.uniform(-3, 3, (n_form, 1)), rng.uniform(0.05, 0.3, (n_form, n_ac - 1))], 1), 1)
    X0 = np.stack([c[..., 0] + r[:, None] * np.cos(th), c[..., 1] + r[:, None] * np.sin(th), th + np.pi / 2 + rng.uniform(-.3, .3, sh),
                   rng.uniform(-.5, .5, sh), rng.uniform(10, 15, sh)], -1)
    return c, r, X0


@pytest.mark.parametrize('n_ac, tol_deg', [(3, 2.0), (5, 8.0)])
def test_gvf_phase_error_rule_with_hold_general_kernel(ctx, n_ac, tol_deg):
    """use_stop 2 with stop_hold > 0 on gvf_run_kernel (small_form at 3, loop branch at 5): the break row, the first convergence
    index, every recorded row -- at stride 1 and 7."""
    import full_sim
    n_form, T, t_opt = 6, 300, 0.3
    gains = dict(GAINS, kr=60.0)
    c, r, X0 = _phase_formations(n_ac, n_form, n_ac)
    refs = [_oracle(c, r, X0, f, T, gains, etheta_tol_deg=tol_deg, t_opt_comp=t_opt) for f in range(n_form)]
    stops = [ref[4] for ref in refs]
    assert len({s for s in stops if s < T}) >= 3, stops
    hold = full_sim.hold_steps(t_opt, DT)
    assert hold > 0
    for rs in (1, 7):
        got = _fetch(_gvf(ctx, c, r, X0, T, gains, etheta_tol_deg=tol_deg, stop_hold=hold, rec_stride=rs), range(n_form), n_ac)
        for f in range(n_form):
            _check(got, f, refs[f], rs, what=(n_ac, f, rs))
            conv = refs[f][5]
            assert got['conv_row'][f] == (conv[0] if conv is not None else -1), (f, got['conv_row'][f], conv)


# ------------------------------------------------------------------------------------------------------------------------------
# 3. bit-level invariants stated in the code
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n_ac', [2, 3, 4, 5, 33])
def test_gvf_identical_formations_bit_identical_wherever_they_sit(ctx, n_ac):
    """one formation copied to the first slot, a wave-straddling slot (general kernel), the last slot of the full block
    and the last slot of the partial block: every history equal bit for bit."""
    import torch
    fpb = _fpb(n_ac)
    n_form = fpb + fpb // 2 + 1
    c, r, X0 = _formations(60 + n_ac, n_form, n_ac)
    st = _straddler(n_ac)
    slots = sorted({fpb - 1, n_form - 1} | ({st} if st else set()))
    for f in slots:
        c[f], r[f], X0[f] = c[0], r[0], X0[0]
    out = _gvf(ctx, c, r, X0, 300, **_physics('wind', n_ac))
    nm = n_ac - 1
    for f in slots:
        for key in ('X', 'U', 'Rr', 'X_final'):
            assert torch.equal(out[key][..., f * n_ac:(f + 1) * n_ac], out[key][..., :n_ac]), (f, key)
        assert torch.equal(out['eth'][:, f * nm:(f + 1) * nm], out['eth'][:, :nm]), f


def test_gvf_quad_path_bit_identical_to_lds_path(ctx):
    """sim_kernels.hip: the DPP quad path does the same sums in the same order as the LDS path.  Two 4-aircraft formations through
    gvf_run_quad_wide_kernel<4> = one 8-aircraft formation through gvf_run_kernel with B = blockdiag(B4, B4) and its column 3 (the
    link between them) zero, z_des = [z4, 0, z4]."""
    import torch
    T = 300
    c, r, X0 = _formations(70, 2, 4)
    kw = _physics('wind', 4)
    B4, z4 = kw.pop('B'), kw.pop('z_des')
    quad = _gvf(ctx, c, r, X0, T, B=B4, z_des=z4, **kw)
    B8 = np.zeros((8, 7)); B8[:4, :3] = B4; B8[4:, 4:] = B4
    lds = ctx.gvf_run(ctx.dev(_planes(X0.reshape(8, 5))), ctx.dev(_planes(c.reshape(8, 2))), ctx.dev(np.repeat(r, 4)), 8, T, DT, V_C,
                      **GAINS, B=B8, z_des=np.r_[z4, 0.0, z4], **kw)
    ctx.sync()
    for key in ('X', 'U', 'Rr', 'X_final'):
        assert torch.equal(quad[key], lds[key]), (key, (quad[key] - lds[key]).abs().max().item())
    ref = _oracle(c, r, X0, 1, T, B=B4, z_des=z4, **kw)
    _check(_fetch(quad, [1], 4), 0, ref, what='quad')


# ------------------------------------------------------------------------------------------------------------------------------
# 4. tracking loop and gain: ragged sizes, user weights, limits, wind, lags
# ------------------------------------------------------------------------------------------------------------------------------
# (lags, then compute_gain's weights and limits; the kernel's track_params takes both by the same names)
WEIGHTS = {
    'default': dict(),
    'q3_ne_q4': dict(tau_v=1.4, Q=(2.0, 0.5, 0.3, 0.05, 0.002), R=(3.0, 0.5), err_sats=(10.0, 15.0, 0.8, 0.5, 2.0), v_min=8.0,
                     v_max=16.0, phi_lim=np.deg2rad(35)),
    'extreme': dict(tau_phi=0.002, Q=(1e-3,) * 5, R=(1e3, 1e-2), phi_lim=np.deg2rad(45)),
}
WIND = (1.2, -0.7)
T_TRACK = 30


def _track_case(seed, n, T=T_TRACK):
    """Per-drone reference curves (circles of either sense, some straight lines) and start errors beyond err_sats and the limits.
    Returns x_ref, y_ref [T][n], X0 (n, 5), Yref0 (n, 8): the flat outputs at row 0 with a random third derivative."""
    rng = np.random.default_rng(seed)
    t = np.arange(T) * DT
    R = rng.uniform(30, 90, n); sp = rng.uniform(9, 15, n)
    om = rng.choice([-1.0, 1.0], n) * sp / R
    a0 = rng.uniform(-np.pi, np.pi, n); cx, cy = rng.uniform(-50, 50, n), rng.uniform(-50, 50, n)
    al = om * t[:, None] + a0
    x, y = cx + R * np.cos(al), cy + R * np.sin(al)
    xd, yd = -R * om * np.sin(al), R * om * np.cos(al)
    xdd, ydd = -R * om ** 2 * np.cos(al), -R * om ** 2 * np.sin(al)
    line = rng.random(n) < 0.3
    vx, vy = sp * np.cos(a0), sp * np.sin(a0)
    x[:, line] = (cx + vx * t[:, None])[:, line]; y[:, line] = (cy + vy * t[:, None])[:, line]
    xd[:, line], yd[:, line] = vx[line], vy[line]
    xdd[:, line] = 0.0; ydd[:, line] = 0.0
    psi = np.arctan2(yd[0], xd[0])
    X0 = np.stack([x[0] + rng.uniform(-35, 35, n), y[0] + rng.uniform(-35, 35, n), psi + rng.uniform(-1.6, 1.6, n),
                   rng.uniform(-1.0, 1.0, n), sp + rng.uniform(-4, 4, n)], 1)
    Yref0 = np.stack([x[0], y[0], xd[0], yd[0], xdd[0], ydd[0], rng.uniform(-2, 2, n), rng.uniform(-2, 2, n)], 1)
    return np.ascontiguousarray(x), np.ascontiguousarray(y), X0, Yref0


def _split(wkey):
    kw = dict(WEIGHTS[wkey])
    lags = dict(tau_phi=kw.pop('tau_phi', 0.01), tau_v=kw.pop('tau_v', 1.0))
    return lags, kw


@pytest.mark.parametrize('n', [1, 63, 65, 200])
@pytest.mark.parametrize('wkey', list(WEIGHTS))
def test_track_run_and_gain_ragged_sizes_user_weights(ctx, wkey, n):
    """track_run_kernel and ctrl_gain_kernel at one drone, one partial wave, one wave + 1 and 200 drones, against the oracle on
    every drone (n = 200: the last one and 32 samples)."""
    lags, gkw = _split(wkey)
    x_ref, y_ref, X0, Yref0 = _track_case(7 * n + list(WEIGHTS).index(wkey), n)
    idx = np.arange(n) if n < 200 else np.r_[np.sort(np.random.default_rng(n).choice(n - 1, 32, replace=False)), n - 1]
    # the tracking loop
    out = ctx.track_run(ctx.dev(x_ref), ctx.dev(y_ref), ctx.dev(_planes(X0)), DT, w=WIND, **lags, **gkw)
    ctx.sync()
    T = T_TRACK
    X, U, Xr, dX = (out[k].cpu().numpy()[:, :, idx].transpose(0, 2, 1) for k in ('X', 'U', 'Xr', 'dX'))
    time = np.arange(T) * DT
    Xo, Uo, Xro, _, _, dXo, _ = S.track_run(time, x_ref[:, idx], y_ref[:, idx], X0[idx], WIND, lags['tau_phi'], lags['tau_v'], **gkw)
    d = X - Xo; d[..., 2] = S.norm_mpi_pi(d[..., 2])
    assert _amax(d) <= 1e-7, (wkey, n, _amax(d))
    assert _amax(U[:T - 1] - Uo[:T - 1]) <= 1e-6, (wkey, n, _amax(U[:T - 1] - Uo[:T - 1]))
    assert _amax(dX[:T - 1] - dXo[:T - 1]) <= 1e-7, (wkey, n)
    np.testing.assert_allclose(Xr[:T - 1], Xro[:T - 1], rtol=1e-10, atol=1e-10)
    if n >= 63:                          # the scenario reaches the error saturations and the command clips
        sats = np.asarray(gkw.get('err_sats', S.ERR_SATS), float)
        assert (np.abs(dXo[0]) == sats).any(0).all(), wkey
        phi_lim, v_min, v_max = gkw.get('phi_lim', S.PHI_LIM), gkw.get('v_min', S.V_MIN), gkw.get('v_max', S.V_MAX)
        assert np.isin(Uo[:T - 1, :, 1], (v_min, v_max)).any(), wkey
        assert (np.abs(Uo[:T - 1, :, 0]) == phi_lim).any() or wkey == 'extreme', wkey      # (r_phi = 1e3: a bank gain of ~1e-3)
    # the gain alone, at the start states and a reference sample with a third derivative
    Xr, dX, U, K = (t.cpu().numpy()[:, idx].T for t in ctx.ctrl_gain(ctx.dev(_planes(X0)), ctx.dev(_planes(Yref0)), w=WIND, **lags, **gkw))
    K = K.reshape(-1, 2, 5)
    for j, i in enumerate(idx):
        y = Yref0[i]
        args = (X0[i], y[0:2], y[2:4], y[4:6], y[6:8], WIND, lags['tau_phi'], lags['tau_v'])
        Xro, dXo, Uo, Ko = S.compute_gain(*args, **gkw)
        if wkey == 'extreme' and not (np.allclose(K[j], Ko, rtol=1e-8, atol=1e-9) and np.allclose(U[j], Uo, rtol=1e-8, atol=1e-9)):
            # in this corner scipy's CARE is off by up to ~1.5e-9 in entries of K whose true size is ~1e-16 (K[1][2]; the kernel's
            # doubling is within 6e-13 of a 40-digit solution): the same tolerances against the gain polished in 40 digits
            _, _, Uo, Ko = S.compute_gain(*args, refined=True, **gkw)
        np.testing.assert_allclose(Xr[j], Xro, rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(dX[j], dXo, rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(K[j], Ko, rtol=1e-8, atol=1e-9, err_msg=str((wkey, n, i)))
        np.testing.assert_allclose(U[j], Uo, rtol=1e-8, atol=1e-9, err_msg=str((wkey, n, i)))


@pytest.mark.parametrize('wkey', ['default', 'extreme'])
def test_track_same_drone_anywhere_in_the_batch(ctx, wkey):
    """The tracking loop is not bit-reproducible across batch layouts (the doubling's early exit and the pivot exchange are
    wave-wide votes, sim_device.h inverse / sda_doubling): one drone at lanes 0, 63, 64, 130 and 199 of 200 stays within 1e-10 in
    X and 1e-12 (relative) in K."""
    lags, gkw = _split(wkey)
    n, slots = 200, (63, 64, 130, 199)
    x_ref, y_ref, X0, Yref0 = _track_case(90, n)
    for i in slots:
        x_ref[:, i], y_ref[:, i], X0[i], Yref0[i] = x_ref[:, 0], y_ref[:, 0], X0[0], Yref0[0]
    out = ctx.track_run(ctx.dev(x_ref), ctx.dev(y_ref), ctx.dev(_planes(X0)), DT, w=WIND, record=('X',), **lags, **gkw)
    K = ctx.ctrl_gain(ctx.dev(_planes(X0)), ctx.dev(_planes(Yref0)), w=WIND, **lags, **gkw)[3]
    ctx.sync()
    X = out['X'].cpu().numpy(); K = K.cpu().numpy()
    for i in slots:
        d = X[:, :, i] - X[:, :, 0]; d[:, 2] = S.norm_mpi_pi(d[:, 2])
        assert _amax(d) <= 1e-10, (i, _amax(d))
        assert _amax(K[:, i] - K[:, 0]) <= 1e-12 * _amax(K[:, 0]), (i, _amax(K[:, i] - K[:, 0]))
