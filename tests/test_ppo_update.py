"""The checker of mocca_adam_step / mocca_ppo_update (tests/ppo_update_reference.py) against what it stands for, without a GPU: the
permutation is a bijection, spreads evenly and follows its key; launch A / B agree with torch.optim.Adam behind clip_grad_norm_ to the
rounding noise torch's own float32 run shows against float64; a NaN gradient skips the step; and the comparisons reject three deliberate
mistakes.  The GPU tests (test_gpu_ppo_update.py) hold the kernels to this checker bit for bit."""
import json
import os
import re

import numpy as np
import pytest

import ppo_update_reference as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (1, 2, 3, 16, 17, 1000, 4097, 131072)


@pytest.mark.parametrize("n", SIZES)
def test_permutation_is_a_bijection(n):
    for t, seed in ((0, 0), (1, 12345), (7, (1 << 63) + 5)):
        p = U.permutation(n, t, seed)
        assert p.dtype == np.int64 and np.array_equal(np.sort(p), np.arange(n))


def _spread(how=None):
    """R = 64 over seeds 1000 .. 5095 at t = 1: (the position x value table's cells in binomial sigmas of their mean 64, chi^2 / dof)"""
    seeds = np.arange(1000, 5096, dtype=np.uint64)[:, None]
    perms = U.permutation(64, 1, seeds, how=how)
    table = np.stack([np.bincount(perms[:, pos], minlength=64) for pos in range(64)]).astype(np.float64)
    sigma = np.sqrt(4096 * (1 / 64) * (63 / 64))
    return (table - 64.0) / sigma, float(((table - 64.0) ** 2 / 64.0).sum() / 3969)


def test_permutation_spreads_evenly():
    """every cell within 6 sigma; chi^2 / dof within 1 +- 0.11, five standard deviations of chi^2 / dof at 3969 degrees of freedom"""
    z, chi = _spread()
    print(f"cells {z.min():+.2f} .. {z.max():+.2f} sigma, chi^2 / dof {chi:.4f}")
    assert np.abs(z).max() < 6.0
    assert abs(chi - 1.0) < 0.11


def test_permutation_follows_its_key():
    """another t or another seed (either half of it) is another permutation, agreeing in about 1 / R of the positions"""
    base = U.permutation(1000, 1, 5)
    for t, seed in ((2, 5), (1, 6), (1, 5 + (1 << 32)), (1 + (1 << 32), 5)):
        other = U.permutation(1000, t, seed)
        assert (other == base).mean() < 0.02, (t, seed)
    assert np.array_equal(base, U.permutation(1000, 1, 5))


N_ADAM, STEPS = 4096, 10


def _torch_run(dtype, p0, grads, max_norm=0.5):
    import torch
    p = torch.nn.Parameter(torch.tensor(p0, dtype=dtype))
    opt = torch.optim.Adam([p], lr=3e-4, eps=1e-5, foreach=False)
    out = []
    for g in grads:
        p.grad = torch.tensor(g, dtype=dtype)
        torch.nn.utils.clip_grad_norm_([p], max_norm)
        opt.step()
        out.append(p.detach().numpy().astype(np.float64).copy())
    return out


def _checker_run(p0, grads, how=None):
    p, m, v, clock = p0.copy(), np.zeros_like(p0), np.zeros_like(p0), np.array(U.FRESH_CLOCK)
    out = []
    for g in grads:
        p, m, v, clock, _ = U.adam_step(p, g, m, v, clock, how=how)
        out.append(p.astype(np.float64))
    assert clock[0] == len(grads) and clock[3] == 0
    return out


def _distance(run, ref, p0):
    """per step and parameter: |p - p_f64| over the largest |step| of that step in the float64 run -> [steps][n]"""
    prev, out = p0.astype(np.float64), []
    for p, r in zip(run, ref):
        out.append(np.abs(p - r) / np.abs(r - prev).max())
        prev = r
    return np.array(out)


@pytest.fixture(scope="module")
def adam_runs():
    rng = np.random.default_rng(3)
    p0 = rng.normal(0, 0.3, N_ADAM).astype(np.float32)
    # steps alternate between a norm far above max_grad_norm (coef < 1) and one below it (coef = 1)
    grads = [U.gradients(N_ADAM, 100 + k, hi=10.0 if k % 2 == 0 else 1e-3) for k in range(STEPS)]
    ref = _torch_run(__import__("torch").float64, p0, grads)
    return p0, grads, ref, _distance(_torch_run(__import__("torch").float32, p0, grads), ref, p0)


def test_adam_checker_against_torch(adam_runs):
    """the checker's float32 run stays within 2 x the distance torch's own float32 run keeps from float64 -- at the largest and at the
    mean over steps and parameters: two roundings of one formula; a factor above rounding noise would be another formula"""
    p0, grads, ref, yard = adam_runs
    got = _distance(_checker_run(p0, grads), ref, p0)
    doc = {"what": "tests/test_ppo_update.py: 10 Adam steps behind clip_grad_norm_(0.5) on 4096 parameters, |p_f32 - p_f64| per parameter over "
                   "the step's largest |delta p| (float64 run), as [mean, max] over steps and parameters",
           "torch_f32_vs_f64": [float(yard.mean()), float(yard.max())], "checker_vs_f64": [float(got.mean()), float(got.max())],
           "per_step_max": {"torch_f32": [float(x) for x in yard.max(1)], "checker": [float(x) for x in got.max(1)]}}
    print(json.dumps(doc))
    out = os.environ.get("MOCCA_TEST_OUT")     # a directory: measured figures are collected there (profiles/ppo_update_parity.json)
    if out:
        with open(os.path.join(out, "ppo_update_parity.json"), "w") as f:
            json.dump(doc, f, indent=1, sort_keys=True)
            f.write("\n")
    assert got.max() <= 2.0 * yard.max() and got.mean() <= 2.0 * yard.mean()


@pytest.mark.parametrize("how", ["no_bias_correction", "coef_after_moments"])
def test_the_torch_comparison_rejects_a_wrong_formula(adam_runs, how):
    p0, grads, ref, yard = adam_runs
    got = _distance(_checker_run(p0, grads, how=how), ref, p0)
    assert got.max() > 2.0 * yard.max() and got.mean() > 2.0 * yard.mean()


def test_five_feistel_rounds_are_another_permutation_and_a_worse_one():
    """the direct comparison of permutations rejects the five-round network"""
    for n in (17, 1000):
        assert not np.array_equal(U.permutation(n, 1, 5), U.permutation(n, 1, 5, how="five_rounds"))


def test_a_nan_gradient_skips_the_step():
    rng = np.random.default_rng(4)
    p, m, v = (rng.normal(0, 1, 300).astype(np.float32) for _ in range(3))
    v = np.abs(v)
    clock = np.array([5.0, 0.9 ** 5, 0.999 ** 5, 2.0])
    g = U.gradients(300, 1)
    for bad in (np.nan, np.inf, -np.inf):
        g2 = g.copy()
        g2[123] = bad
        q, mq, vq, cq, coef = U.adam_step(p, g2, m, v, clock)
        assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in ((p, q), (m, mq), (v, vq)))
        assert np.array_equal(cq[:3], clock[:3]) and cq[3] == 3.0 and coef == 0.0
    g2 = g.copy()
    g2[299] = np.nan      # beyond n_params: not part of the norm
    q, _, _, cq, coef = U.adam_step(p, g2, m, v, clock, n_params=299)
    assert cq[0] == 6.0 and cq[3] == 2.0 and coef > 0 and q[299] == p[299] and not np.array_equal(q[:299], p[:299])


def test_sum_of_squares_is_the_sum():
    g = U.gradients(1000, 2)
    assert abs(U.sum_of_squares(g) - float((g.astype(np.float64) ** 2).sum())) < 1e-12 * float((g.astype(np.float64) ** 2).sum())
    assert U.sum_of_squares(np.zeros(3, np.float32)) == 0.0


def test_abi_version_is_still_8_and_the_entry_points_are_bound():
    from mocca_envs_amd import lib
    header = open(os.path.join(ROOT, "include", "mocca.h")).read()
    assert lib.ABI_VERSION == 8 and re.search(r"#define\s+MOCCA_ABI_VERSION\s+8\b", header)
    for name in ("mocca_adam_step", "mocca_ppo_update"):
        assert name in lib.SYMBOLS and re.search(r"\bint " + name + r"\(", header)
    assert len(lib.SYMBOLS["mocca_adam_step"][1]) == 13 and len(lib.SYMBOLS["mocca_ppo_update"][1]) == 28


def test_adam_state_and_the_argument_checks():
    """AdamState's fresh state and checkpoint round trip, and the refusals that need no device"""
    import torch
    from types import SimpleNamespace
    from mocca_envs_amd import rollout as ro
    st = ro.AdamState(10, "cpu")
    assert st.moments.shape == (2, 10) and not st.moments.any() and st.clock.tolist() == list(U.FRESH_CLOCK)
    st.moments.fill_(2.0), st.clock.copy_(torch.tensor([3.0, 0.7, 0.99, 1.0], dtype=torch.float64))
    saved = st.state_dict()
    st.reset()
    assert not st.moments.any() and st.clock.tolist() == list(U.FRESH_CLOCK)
    st.load_state_dict(saved)
    assert (st.moments == 2.0).all() and st.clock.tolist() == [3.0, 0.7, 0.99, 1.0]
    with pytest.raises(ValueError):
        st.load_state_dict({"moments": torch.zeros(2, 9), "clock": torch.zeros(4)})
    pol = SimpleNamespace(n_head=lambda: 10, in_dim=3)
    cpu, ok = torch.device("cpu"), dict(n_params=None, lr=3e-4, betas=(0.9, 0.999), eps=1e-5, max_grad_norm=0.5)
    params, grad = torch.zeros(16), torch.zeros(10)
    call = lambda p=params, g=grad, s=st, **kw: ro.adam_args(pol, cpu, p, g, s, **{**ok, **kw})
    assert call() == 10 and call(p=torch.zeros(10), n_params=7, g=torch.zeros(7)) == 7 and call(g=None) == 10
    for kw in (dict(p=torch.zeros(11)), dict(p=torch.zeros(16, dtype=torch.float64)), dict(g=torch.zeros(9)), dict(n_params=0), dict(n_params=11),
               dict(s=ro.AdamState(9, "cpu")), dict(s=None), dict(lr=float("nan")), dict(lr=-1.0), dict(eps=float("inf")), dict(betas=(1.0, 0.9)),
               dict(betas=(0.9, -0.1)), dict(max_grad_norm=float("nan")), dict(max_grad_norm=-1.0)):
        with pytest.raises(ValueError):
            call(**kw)
    assert ro.update_args(200, 48, 3, 0, None, cpu) == 4
    for args in ((200, 0, 1, 0), (200, 201, 1, 0), (200, 48, 0, 0), (200, 48, 1, -1), (200, 48, 1, 1 << 64), ((1 << 22) + 1, 48, 1, 0)):
        with pytest.raises(ValueError):
            ro.update_args(*args, None, cpu)
    with pytest.raises(ValueError):
        ro.update_args(200, 48, 3, 0, torch.zeros(11, 8), cpu)
