"""mocca_distill_grad and the teacher's slot without a GPU: the ABI's declarations, bindings and exports, the reference's hand-written per-row
lines against autograd, and the negative controls -- wrong losses that the GPU test's acceptance rule must refuse.  The checker is
tests/distill_reference.py."""
import os
import re
import subprocess

import numpy as np
import pytest

import distill_reference as D
import ppo_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"mocca_distill_grad": 12, "mocca_distill_update": 23, "mocca_set_teacher": 6, "mocca_update_teacher": 4, "mocca_teacher_act": 7}


def test_header_declares_binding_lists_and_library_exports_the_entry_points():
    from mocca_envs_amd import lib
    from mocca_envs_amd.build import build_lib
    header = open(os.path.join(ROOT, "include", "mocca.h")).read()
    names = subprocess.run(["nm", "-D", "--defined-only", build_lib()], capture_output=True, text=True, check=True).stdout
    for name, n_args in NEW.items():
        assert re.search(r"\bint %s\(mocca_handle h," % name, header), name
        assert len(lib.SYMBOLS[name][1]) == n_args, name
        assert re.search(r"\bT %s\b" % name, names), name
    assert re.search(r"#define MOCCA_ABI_VERSION 8\b", header) and lib.ABI_VERSION == 8


@pytest.mark.parametrize("use_value", [True, False])
@pytest.mark.parametrize("act", ["identity", "relu", "tanh", "softsign"])
def test_hand_formulas_equal_autograd_in_f64(act, use_value):
    """every activation, with and without value targets: 1e-12 relative to the largest gradient entry of each tensor (the bound
    tests/test_ppo.py holds ppo_reference.grad_by_hand to); tensors whose gradient is identically zero are zero by hand too"""
    p = R.make_policy("mixed", norm=True, seed=3, acts=[act, act, act])
    st = D.make_storage("mixed", p, 64, seed=1)
    kw = dict(distill_coef=0.7, value_coef=0.5, use_value=use_value)
    want, got = D.loss_autograd(p, st, **kw).grad, D.grad_by_hand(p, st, **kw)
    assert R.tensor_errors(p, got, want).max() <= 1e-12
    zeros = D.zero_tensors(p, want)
    assert len(zeros) == (1 if use_value else 1 + 2 * len(p.critic)) and all(not np.any(got[a:b]) for a, b in zeros)


def test_stats_layout_of_the_reference():
    p = R.make_policy("tiny", norm=False, seed=2)
    st = D.make_storage("tiny", p, 17, seed=2)
    ref = D.loss_autograd(p, st)
    mu_err = R._forward64(p.actor, np.asarray(st["obs"], np.float64))[-1] - st["target"]
    assert abs(ref.stats[7] - np.mean(mu_err ** 2)) <= 1e-12 and ref.stats[1] > 0 and not ref.stats[[0, 3, 4, 6]].any()
    assert D.loss_autograd(p, st, use_value=False).stats[1] == 0


@pytest.mark.parametrize("name,use_value", [("tiny", True), ("mixed", False), ("ppo", True)])
def test_the_rule_accepts_the_float32_reference(name, use_value):
    """the rule is not vacuous the other way: float32 autograd itself, and the by-hand gradient rounded to float32, pass it"""
    p = R.make_policy(name, norm=True, seed=1)
    st = D.make_storage(name, p, 100, seed=2)
    want = D.loss_autograd(p, st, use_value=use_value).grad
    f32 = D.loss_autograd(p, st, "float32", use_value=use_value).grad
    assert D.accepts(p, f32, f32, want)
    assert D.accepts(p, D.grad_by_hand(p, st, use_value=use_value).astype(np.float32), f32, want)


@pytest.mark.parametrize("mutation", D.MUTATIONS)
@pytest.mark.parametrize("name", ["tiny", "ppo"])
def test_negative_controls_fail_the_gpu_tests_rule(name, mutation):
    """a gradient from a loss with a missing 1 / A, a missing factor 2, a flipped sign, target columns rolled by one, a value term leaking
    into the actor or an entropy term on log_std FAILS the rule tests/test_gpu_distill.py applies, against the unmutated f64 gradient"""
    p = R.make_policy(name, norm=True, seed=1)
    st = D.make_storage(name, p, 100, seed=2)
    want = D.loss_autograd(p, st).grad
    f32 = D.loss_autograd(p, st, "float32").grad
    wrong = D.loss_autograd(p, st, "float32", mutation=mutation).grad
    assert not D.accepts(p, wrong, f32, want), mutation
