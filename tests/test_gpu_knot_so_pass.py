"""GPU: the knot kernel's second-order pass under the segment floor (csrc/fit_knot.hip knot_mfma_so_floor: straight-line k-steps
round-robin over three accumulators, the A operands read by address from the fp32 Hermite table's pad word, J^T r riding on the
k-steps where no segment holds more than nine samples) computes what the rolled pass and the stand-alone phase 2 computed, bit for bit.

tests/golden/knot_r10_parent_bits.npz (tools/dump_knot_bits.py --r10) was written once with the build of the commit before that
pass: 32 fits a case, max_iter = 150; cost, q, trial counts, status and the evaluation count must be np.array_equal.  Cases: K = 48
(every segment at the floor, no predicated k-step), 50 (the bench's), 54 | 55 (either side of SEG9), 64 (the longest segments, three
predicated k-steps), CostBank's max mode (long finishes with rejected trials), so_lambda = 0, and K = 50 resumed in launches of 7
trials (a fit resumed inside the finish enters through the second-order pass with its kept knot vector).  Every case must have
reached second-order evaluations: its evaluation count differs from that of the same fits solved with mp_finish = 0.

The floor's pass against the rolled one in ONE build (D2D_FIT_ABLATE & 64 forces the generic instantiation) for K = 64 and the resumed
solve, which tests/test_gpu_knot_segmin.py does not cover."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden', 'knot_r10_parent_bits.npz')
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import dump_knot_bits as DK  # noqa: E402

COMPARED = ('cost', 'q', 'iters', 'status', 'evals')


@pytest.fixture(scope='module')
def ctx():
    import d2dhip
    c = d2dhip.Context(0)
    yield c
    c.close()


@pytest.fixture(scope='module')
def gold():
    return dict(np.load(GOLD, allow_pickle=False))


def _same(name, what, got, want):
    for k in COMPARED:
        a, b = got[k], want[k]
        assert a.dtype == b.dtype and a.shape == b.shape, (name, k)
        if not np.array_equal(a, b):
            bad = np.nonzero((a != b).reshape(len(a), -1).any(1))[0]
            pytest.fail(f'{name}.{k}: {len(bad)} of {len(a)} rows differ from {what} (first: {bad[:8].tolist()})')


def test_fixture_is_complete(gold):
    assert DK.R10_CASES == ('k48', 'k50', 'k54', 'k55', 'k64', 'bankmax', 'so0', 'resume')
    assert sorted(gold) == sorted(f'{n}_{k}' for n in DK.R10_CASES for k in DK.R10_FIELDS)
    for n in DK.R10_CASES:
        assert gold[n + '_q'].dtype == np.float64 and gold[n + '_q'].shape == (DK.R10_B, 48) and DK.R10_B == 32
        assert gold[n + '_cost'].shape == (32,) and gold[n + '_iters'].dtype == np.int32 and gold[n + '_status'].dtype == np.int32
        assert 1 <= gold[n + '_iters'].min() and gold[n + '_iters'].max() <= DK.MAX_ITER == 150
        assert gold[n + '_evals'].shape == (1,) and gold[n + '_slice'].shape == (1,) and 0 <= int(gold[n + '_slice'][0]) <= DK.R10_POOL - 32


@pytest.mark.parametrize('name', DK.R10_CASES)
def test_second_order_pass_bits_are_the_parents(ctx, gold, name):
    import d2dhip
    K, dur, _, _ = DK.r10_scenarios(name, 0)
    smin, smax, floor = d2dhip.knot_segments(6, K, dur)[1:4]
    assert floor == 8 and (smin, smax) == {48: (8, 8), 50: (8, 9), 54: (9, 9), 55: (9, 10), 64: (10, 11)}[K]
    first = int(gold[name + '_slice'][0])
    got = DK.r10_run(ctx, name, first)
    lmder = DK.r10_run(ctx, name, first, mp_finish=0)
    print(name, 'evaluations', int(got['evals'][0]), 'with mp_finish = 0', int(lmder['evals'][0]), 'trials', int(got['iters'].min()), int(got['iters'].max()))
    assert got['evals'][0] != lmder['evals'][0], f'{name}: no fit left lmder -- the case reaches no second-order evaluation'
    _same(name, 'the fixture', got, {k: gold[f'{name}_{k}'] for k in COMPARED})


@pytest.mark.parametrize('name', ['k64', 'resume'])
def test_floor_and_generic_second_order_pass_agree_bit_for_bit(ctx, gold, monkeypatch, name):
    first = int(gold[name + '_slice'][0])
    monkeypatch.delenv('D2D_FIT_ABLATE', raising=False)
    spec = DK.r10_run(ctx, name, first)
    monkeypatch.setenv('D2D_FIT_ABLATE', '64')
    gen = DK.r10_run(ctx, name, first)
    _same(name, 'the generic instantiation', spec, gen)
