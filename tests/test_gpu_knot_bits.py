"""The knot kernel's results, bit for bit, against tests/golden/knot_parent_bits.npz (tools/dump_knot_bits.py: written once with the
build of the commit before the round-7 pass over the solver loop).  That pass only removes work the banded,
metric-damped solve never needed, and every later change of that kind is held to the same fixture: cost, q, trial counts, status and
the batch statistics of six small families -- bench scenarios at K = 50, K = 40 and K = 64 (the generic instantiation), so_lambda = 0,
CostBank's max mode, and a solve resumed launch after launch (7 trials each) -- must be np.array_equal."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden', 'knot_parent_bits.npz')
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
    assert sorted(gold) == sorted(f'{n}_{k}' for n in DK.FAMILIES for k in DK.FIELDS)
    sizes = {n: len(gold[n + '_cost']) for n in DK.FAMILIES}
    assert sizes == {'bench': 192, 'k40': 64, 'k64': 64, 'so0': 64, 'bankmax': 64, 'resume': 64}
    for n in DK.FAMILIES:
        assert gold[n + '_q'].dtype == np.float64 and gold[n + '_q'].shape == (sizes[n], 48)
        assert gold[n + '_iters'].max() <= DK.MAX_ITER


@pytest.mark.parametrize('name', DK.FAMILIES)
def test_knot_kernel_bits_are_the_parents(ctx, gold, name):
    r = DK.run(ctx, name)
    for k in DK.FIELDS:
        got, want = r[k], gold[f'{name}_{k}']
        assert got.dtype == want.dtype and got.shape == want.shape, (name, k)
        if not np.array_equal(got, want):
            bad = np.nonzero((got != want).reshape(len(got), -1).any(1))[0] if got.ndim else np.array([0])
            pytest.fail(f'{name}.{k}: {len(bad)} of {len(got)} rows differ from the fixture (first: {bad[:8].tolist()})')
