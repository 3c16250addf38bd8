"""mocca_ppo_grad_sym without a GPU: the ABI's declaration, binding and export, the header's by-hand formulas against float64 autograd,
the teeth of the parity rule (every backward mutation is rejected by it) and the identity tables.  The checker is
tests/ppo_symmetry_reference.py."""
import os
import re
import subprocess

import numpy as np
import pytest

import ppo_reference as R
import ppo_symmetry_reference as PS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KW = dict(value_coef=0.5, entropy_coef=0.01)


def _header():
    return open(os.path.join(ROOT, "include", "mocca.h")).read()


def _tables(p, seed=3):
    return PS.random_tables(p.actor[0][0].shape[1], seed, p.log_std.size)


def test_header_declares_and_binding_lists_mocca_ppo_grad_sym():
    from mocca_envs_amd import lib
    assert re.search(r"\bint mocca_ppo_grad_sym\(mocca_handle h,", _header())
    assert lib.SYMBOLS["mocca_ppo_grad_sym"] == lib.SYMBOLS["mocca_ppo_grad"]      # the same argument list
    assert re.search(r"#define MOCCA_ABI_VERSION 8\b", _header()) and lib.ABI_VERSION == 8      # additive


def test_library_exports_mocca_ppo_grad_sym():
    from mocca_envs_amd.build import build_lib
    names = subprocess.run(["nm", "-D", "--defined-only", build_lib()], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT mocca_ppo_grad_sym\b", names) and re.search(r"\bT mocca_ppo_grad\b", names)


def test_minibatch_bound_of_the_symmetric_call():
    from mocca_envs_amd import rollout
    assert rollout.MAX_MINIBATCH_SYM == 1 << 21 and rollout.MAX_MINIBATCH == 1 << 22
    assert re.search(r"n_rows is 1 \.\. 2\^21", _header())


@pytest.mark.parametrize("value_clip", [False, True])
@pytest.mark.parametrize("act", ["identity", "relu", "tanh", "softsign"])
def test_hand_formulas_equal_autograd_in_f64(act, value_clip):
    """the header's lines -- the symmetrised mu / ls / v, each head's half, dL/df2 through act_perm and act_sign, 1/2 (T[j] + T[pj]) for
    log_std, both passes' weight gradients added -- against float64 autograd: 1e-10 relative to the largest entry of each tensor; rows on
    both sides of both clip bounds and, for value_clip, of the value clamp"""
    p = R.make_policy("mixed", norm=True, seed=3, acts=[act, act, act])
    tables = _tables(p)
    st = PS.make_storage_sym(p, tables, 64, seed=1)
    ratio = np.exp(PS.loss_autograd_sym(p, tables, st).logp - st["old_logp"])
    assert (ratio < 0.8).any() and ((ratio > 0.8) & (ratio < 1)).any() and ((ratio > 1) & (ratio < 1.2)).any() and (ratio > 1.2).any()
    assert np.abs(ratio / np.array(R.RATIOS)[np.abs(ratio[:, None] / np.array(R.RATIOS) - 1).argmin(1)] - 1).max() < 0.0101
    kw = dict(KW, value_clip=value_clip)
    want, got = PS.loss_autograd_sym(p, tables, st, **kw).grad, PS.grad_by_hand_sym(p, tables, st, **kw)
    assert R.tensor_errors(p, got, want).max() <= 1e-10


def test_relu_rows_keep_their_margin_in_both_passes():
    p = R.make_policy("mixed", norm=True, seed=1)
    tables = _tables(p)
    st = PS.make_storage_sym(p, tables, 40, seed=2)
    pre = PS.loss_autograd_sym(p, tables, st).pre
    n_layers = len(p.actor) + len(p.critic)
    assert len(pre) == 2 * n_layers      # the as-given and the mirrored pass of every layer
    acts = [act for _, _, act in p.actor] * 2 + [act for _, _, act in p.critic] * 2      # the order the reference runs them in
    assert acts.count("relu") == 4 and all(np.abs(z).min() > R.RELU_MARGIN for z, act in zip(pre, acts) if act == "relu")


@pytest.mark.parametrize("n_rows", [17, 100])
@pytest.mark.parametrize("norm", [True, False])
@pytest.mark.parametrize("name", ["tiny", "ppo", "wide", "single"])
def test_parity_rule_rejects_every_backward_mutation(name, norm, n_rows):
    """The rule the GPU test applies (errors against float64 autograd within 3 x float32 autograd's at the median, the 99th percentile and the
    maximum) rejects a float32 gradient whose backward is wrong in any of BACKWARD_MUTATIONS' ways, although its forward -- loss and
    statistics -- is right.  The yardstick's triple is about [5e-8, 8e-7, 3e-6]; a mutation's largest error is of order 1."""
    p = R.make_policy(name, norm=norm, seed=1)
    tables = _tables(p)
    st = PS.make_storage_sym(p, tables, n_rows, seed=2)
    ref = PS.loss_autograd_sym(p, tables, st, "float64", **KW)
    f32 = PS.loss_autograd_sym(p, tables, st, "float32", **KW)
    yard = R.triple(R.tensor_errors(p, f32.grad, ref.grad))
    assert R.within(yard, yard) and yard[2] < 1e-4
    for how in PS.BACKWARD_MUTATIONS:
        bad = PS.loss_autograd_sym(p, tables, st, "float32", how=how, **KW)
        got = R.triple(R.tensor_errors(p, bad.grad, ref.grad))
        print(f"{name} norm={norm} B={n_rows} {how}: {got} against {yard}")
        assert not R.within(got, yard), (how, got, yard)
        assert got[2] >= 0.1, (how, got)      # a wiring error is of the gradient's own size: five orders above the yardstick
        assert np.allclose(bad.stats[:5], f32.stats[:5], rtol=1e-5, atol=1e-6), how      # the forward is the right one


@pytest.mark.parametrize("how", PS.MUTATIONS)
def test_parity_rule_rejects_the_forward_mutations_too(how):
    p = R.make_policy("tiny", norm=True, seed=1)
    tables = _tables(p)
    st = PS.make_storage_sym(p, tables, 100, seed=2)
    ref = PS.loss_autograd_sym(p, tables, st, "float64", **KW)
    yard = R.triple(R.tensor_errors(p, PS.loss_autograd_sym(p, tables, st, "float32", **KW).grad, ref.grad))
    got = R.triple(R.tensor_errors(p, PS.loss_autograd_sym(p, tables, st, "float32", how=how, **KW).grad, ref.grad))
    assert not R.within(got, yard), (got, yard)


@pytest.mark.parametrize("value_clip", [False, True])
def test_identity_tables_give_the_plain_gradient(value_clip):
    """perm = arange, sign = +1: both passes are the plain pass, each head receives half twice -- the plain loss_autograd gradient"""
    p = R.make_policy("mixed", norm=True, seed=2)
    st = R.make_storage(p, 50, seed=3)
    tables = PS.identity_tables(65, 21)
    kw = dict(KW, value_clip=value_clip)
    plain, sym = R.loss_autograd(p, st, **kw), PS.loss_autograd_sym(p, tables, st, **kw)
    assert R.tensor_errors(p, sym.grad, plain.grad).max() <= 1e-12 and np.allclose(sym.stats, plain.stats, rtol=1e-12, atol=0)
    assert R.tensor_errors(p, PS.grad_by_hand_sym(p, tables, st, **kw), plain.grad).max() <= 1e-12


def test_mirrored_minibatch_has_the_same_loss_and_gradient_in_f64():
    """(M_o s, M_a a) with the same old_logp, adv and returns: the symmetric policy's loss is the same function of the parameters"""
    p = R.make_policy("mixed", norm=True, seed=4)
    tables = _tables(p)
    st = PS.make_storage_sym(p, tables, 50, seed=5)
    a = PS.loss_autograd_sym(p, tables, st, value_clip=True, **KW)
    b = PS.loss_autograd_sym(p, tables, PS.mirror_storage(st, tables), value_clip=True, **KW)
    assert R.tensor_errors(p, b.grad, a.grad).max() <= 1e-10 and np.allclose(a.stats, b.stats, rtol=1e-10, atol=0)
