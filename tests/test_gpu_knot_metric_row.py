"""Round 9 of the knot kernel's solver loop, bit for bit against tests/golden/knot_r9_parent_bits.npz
(tools/dump_knot_bits.py --r9: written once with the build of the commit before it).  The round removes two pieces of work from
damped_solve without touching a rounding: KnotMetric::damp() reads a row of zeros instead of selecting per lane, and the back
substitution scales its column with packed multiplies.  cost, q, trial counts and status of 32 fits a case must be np.array_equal.

Knot kernel: K = 23 (the generic instantiation), 48 (every segment at the floor), 50, 55 (not SEG9), 64, and K = 50 with
so_lambda = 0 and in CostBank's max mode.  32 fits start at once, so the hand-out order plays no part; the first trial of every fit
holds both kinds of solve, Gauss-Newton (no lane damped) and damped.  The back substitution is shared: one case each through
d2d_fit_plan_opts.kernel = FUSED (fit_lm_kernel), a long-horizon plan (K = 121, fit_lm_long_kernel) and solve_groups (2 aircraft x 16
replicas, fit_groups_kernel) pins it there."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden', 'knot_r9_parent_bits.npz')
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import dump_knot_bits as DK  # noqa: E402


@pytest.fixture(scope='module')
def ctx():
    import d2dhip
    c = d2dhip.Context(0)
    yield c
    c.close()


@pytest.fixture(scope='module')
def gold():
    return dict(np.load(GOLD, allow_pickle=False))


def test_fixture_is_complete(gold):
    assert DK.R9_KNOT == ('k23', 'k48', 'k50', 'k55', 'k64', 'so0', 'bankmax') and DK.R9_SHARED == ('fused', 'long', 'groups')
    assert (DK.R9_B, DK.R9_MAX_ITER) == (32, 40)
    assert sorted(gold) == sorted(f'{n}_{k}' for n in DK.R9_CASES for k in DK.R9_FIELDS)
    for n in DK.R9_CASES:
        assert gold[n + '_cost'].dtype == np.float64 and gold[n + '_cost'].shape == (32,)
        assert gold[n + '_q'].dtype == np.float64 and gold[n + '_q'].shape == (32, 48)
        assert gold[n + '_iters'].dtype == np.int32 and gold[n + '_status'].dtype == np.int32
        if n != 'groups':
            assert gold[n + '_iters'].shape == (32,) and gold[n + '_status'].shape == (32,)
            # (at least one accepted step everywhere: the first trial -- a Gauss-Newton solve, then damped ones -- was run)
            assert gold[n + '_iters'].min() >= 1 and gold[n + '_iters'].max() <= DK.R9_MAX_ITER


@pytest.mark.parametrize('name', DK.R9_CASES)
def test_bits_are_the_parents(ctx, gold, name):
    r = DK.r9_run(ctx, name)
    for k in DK.R9_FIELDS:
        got, want = r[k], gold[f'{name}_{k}']
        assert got.dtype == want.dtype and got.shape == want.shape, (name, k)
        if not np.array_equal(got, want):
            bad = np.nonzero((got != want).reshape(len(got), -1).any(1))[0]
            pytest.fail(f'{name}.{k}: {len(bad)} of {len(got)} rows differ from the fixture (first: {bad[:8].tolist()})')
