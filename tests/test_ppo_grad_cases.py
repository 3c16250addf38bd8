"""ppo_grad_cases.parity without a GPU: the acceptance loop of the five PPO gradient test files passes a gradient that is right -- the
mode's own float32 autograd, laid out as the kernel lays its outputs out -- and reports one that is wrong in each way the loop is there to
catch.  Net `tiny`, three batch sizes: every branch of the loop (both index forms, the pooling with its look-ahead, both values of every
cycling flag) at a cost of seconds."""
import numpy as np
import pytest

import ppo_grad_cases as G
import ppo_reference as R

BATCHES = (1, 17, 100)
MODES = sorted(G.MODES)


@pytest.fixture(autouse=True)
def _no_records(monkeypatch):
    monkeypatch.delenv("MOCCA_TEST_OUT", raising=False)      # these figures are not the kernel's


def _scale_one_tensor(p, grad, stats, samples):
    a, b = R.tensor_slices(p)[0]
    grad[a:b] *= np.float32(1 + 1e-3)
    stats[5] = (grad.astype(np.float64) ** 2).sum()      # consistent with the returned gradient: only the gradient rule can object


def _clip_fraction_one_row_off(p, grad, stats, samples):
    stats[4] = (np.float32(round(float(stats[4]) * samples)) + (1 if stats[4] < 0.5 else -1)) / np.float32(samples)


def _forbidden_non_zero(mode):
    def spoil(p, grad, stats, samples):
        stats[6] = 1
        if mode.stat7 == "zero":
            stats[7] = 1
    return spoil


def _sum_of_squares_off(p, grad, stats, samples):
    stats[5] *= np.float32(1 + 1e-4)      # the rule allows 1e-5


def autograd32(mode, spoil=None):
    """parity's `compute` from float32 autograd: stats[4] formed as the kernel forms it (the count over the samples, divided in float32),
    stats[5] the sum of squares of the gradient, zeros wherever the reference has none; then spoiled"""
    def compute(p, tables, st, idx, flag, strided, coef):
        f32 = mode.loss(p, tables, coef, R.gather(st, idx), "float32", flag)
        grad, stats = f32.grad.astype(np.float32), np.zeros(8, np.float32)
        stats[:len(f32.stats)] = f32.stats
        samples = mode.samples * (st["obs"].shape[0] if idx is None else len(idx))
        stats[4] = np.float32(round(f32.stats[4] * samples)) / np.float32(samples)
        stats[5] = (grad.astype(np.float64) ** 2).sum()
        if spoil:
            spoil(p, grad, stats, samples)
        return grad, stats
    return compute


@pytest.mark.parametrize("mode", MODES)
def test_configurations_cover_both_values_of_both_cycling_flags(mode):
    """what parity asserts before it starts, at the batch sizes the GPU files use and at this file's: every weight of the mode's setter
    meets the fourth flag on and off, and the strided obs is on and off"""
    for batches in (None, BATCHES):
        cfgs = list(G.configs(G.MODES[mode], batches))
        assert len(cfgs) == 4 * len(batches or G.MODES[mode].batches) and {c[4] for c in cfgs} == {False, True}
        assert {(c[3], c[5]) for c in cfgs} == {(f, c) for f in (False, True) for c in G.MODES[mode].coefs}


@pytest.mark.parametrize("mode", MODES)
def test_float32_autograd_passes(mode):
    assert not (f := G.parity(G.MODES[mode], "tiny", autograd32(G.MODES[mode]), BATCHES)), f


@pytest.mark.parametrize("mode", MODES)
def test_one_tensor_scaled_is_a_gradient_failure(mode):
    """one parameter tensor times 1 + 1e-3: an error of 1e-3 of that tensor's largest entry against a float32 yardstick near 1e-6 breaks the
    3 x rule at the maximum by orders of magnitude, in every pool, and nothing else objects"""
    failures = G.parity(G.MODES[mode], "tiny", autograd32(G.MODES[mode], _scale_one_tensor), BATCHES)
    assert failures and all(len(f) == 3 and f[0] != "stats" and not R.within(f[1], f[2]) for f in failures), failures


@pytest.mark.parametrize("mode", MODES)
def test_clip_fraction_one_row_off_is_reported(mode):
    failures = G.parity(G.MODES[mode], "tiny", autograd32(G.MODES[mode], _clip_fraction_one_row_off), BATCHES)
    assert sum(f[1] == "clip fraction" for f in failures) == 4 * len(BATCHES), failures


@pytest.mark.parametrize("mode", MODES)
def test_a_forbidden_non_zero_is_reported(mode):
    failures = G.parity(G.MODES[mode], "tiny", autograd32(G.MODES[mode], _forbidden_non_zero(G.MODES[mode])), BATCHES)
    assert sum(f[1] == "stats[6], stats[7]" for f in failures) == 4 * len(BATCHES), failures


@pytest.mark.parametrize("mode", MODES)
def test_sum_of_squares_1e_4_off_is_reported(mode):
    failures = G.parity(G.MODES[mode], "tiny", autograd32(G.MODES[mode], _sum_of_squares_off), BATCHES)
    assert sum(f[1] == "sum of grad^2" for f in failures) == 4 * len(BATCHES), failures
