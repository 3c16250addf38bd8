"""mocca_ppo_grad_mirror and mocca_set_policy_mirror_loss without a GPU: the ABI's declarations, bindings and exports, the header's by-hand
formulas against float64 autograd, coef = 0 and the identity tables against the plain checker, the mirrored storage, the teeth of the parity
rule (every mutation of the term is rejected by it) and symmetry.mirror_loss in torch.  The checker is tests/ppo_mirror_reference.py."""
import os
import re
import subprocess

import numpy as np
import pytest

import ppo_mirror_reference as PM
import ppo_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KW = dict(value_coef=0.5, entropy_coef=0.01)


def _header():
    return open(os.path.join(ROOT, "include", "mocca.h")).read()


def _tables(p, seed=3):
    return PM.random_tables(p.actor[0][0].shape[1], seed, p.log_std.size)


def test_header_declares_and_binding_lists_the_two_entry_points():
    import ctypes as C
    from mocca_envs_amd import lib
    assert re.search(r"\bint mocca_ppo_grad_mirror\(mocca_handle h,", _header())
    assert re.search(r"\bint mocca_set_policy_mirror_loss\(mocca_handle h,[^;]*double mirror_coef\);", _header())
    assert lib.SYMBOLS["mocca_ppo_grad_mirror"] == lib.SYMBOLS["mocca_ppo_grad"]      # the same argument list
    res, args = lib.SYMBOLS["mocca_set_policy_mirror_loss"]
    assert (res, args) == (lib.SYMBOLS["mocca_set_policy_symmetry"][0], lib.SYMBOLS["mocca_set_policy_symmetry"][1] + [C.c_double])
    assert re.search(r"#define MOCCA_ABI_VERSION 8\b", _header()) and lib.ABI_VERSION == 8      # additive


def test_library_exports_the_two_entry_points():
    from mocca_envs_amd.build import build_lib
    names = subprocess.run(["nm", "-D", "--defined-only", build_lib()], capture_output=True, text=True, check=True).stdout
    for name in ("mocca_ppo_grad_mirror", "mocca_set_policy_mirror_loss", "mocca_ppo_grad", "mocca_ppo_grad_sym", "mocca_set_policy_symmetry"):
        assert re.search(rf"\bT {name}\b", names), name


@pytest.mark.parametrize("value_clip", [False, True])
@pytest.mark.parametrize("act", ["identity", "relu", "tanh", "softsign"])
def test_hand_formulas_equal_autograd_in_f64(act, value_clip):
    """the header's lines -- u = 2 coef d / (B A) added to dL/df1, -(u act_sign) through act_perm to the mirrored pass, both passes' actor
    gradients added, the critic's as-given pass alone, the row's term (sum_j d^2) / A -- against float64 autograd: 1e-10 relative to the
    largest entry of each tensor, and L_m to 1e-12"""
    p = R.make_policy("mixed", norm=True, seed=3, acts=[act, act, act])
    tables = _tables(p)
    st = R.make_storage(p, 64, seed=1)
    kw = dict(KW, value_clip=value_clip)
    for coef in (0.0, 0.5, 4.0):
        want = PM.loss_autograd_mirror(p, tables, coef, st, **kw)
        got, l_m = PM.grad_by_hand_mirror(p, tables, coef, st, **kw)
        assert R.tensor_errors(p, got, want.grad).max() <= 1e-10, coef
        assert want.stats[7] > 1e-3 and abs(l_m - want.stats[7]) <= 1e-12 * want.stats[7] and want.stats[6] == 0.0


@pytest.mark.parametrize("value_clip", [False, True])
def test_coef_zero_is_the_plain_loss(value_clip):
    """coef = 0: the gradient and stats[0..5] are ppo_reference.loss_autograd's, and L_m is still reported"""
    p = R.make_policy("mixed", norm=True, seed=2)
    st = R.make_storage(p, 50, seed=3)
    kw = dict(KW, value_clip=value_clip)
    plain, got = R.loss_autograd(p, st, **kw), PM.loss_autograd_mirror(p, _tables(p), 0.0, st, **kw)
    assert np.array_equal(got.grad, plain.grad) and np.array_equal(got.stats[:6], plain.stats) and got.stats[7] > 1e-3


def test_identity_tables_have_no_mirror_loss():
    """perm = arange, sign = +1: both passes are the same pass, d = 0 exactly, and the gradient is the plain one at any coef"""
    p = R.make_policy("mixed", norm=True, seed=2)
    st = R.make_storage(p, 50, seed=3)
    tables = PM.identity_tables(65, 21)
    plain = R.loss_autograd(p, st, **KW)
    for dtype in ("float64", "float32"):
        got = PM.loss_autograd_mirror(p, tables, 4.0, st, dtype, **KW)
        assert got.stats[7] == 0.0
    got = PM.loss_autograd_mirror(p, tables, 4.0, st, **KW)
    assert R.tensor_errors(p, got.grad, plain.grad).max() <= 1e-12 and np.allclose(got.stats[:6], plain.stats, rtol=1e-12, atol=0)
    by_hand, l_m = PM.grad_by_hand_mirror(p, tables, 4.0, st, **KW)
    assert l_m == 0.0 and R.tensor_errors(p, by_hand, plain.grad).max() <= 1e-12


def test_mirrored_storage_has_the_same_mirror_loss_in_f64():
    """on (M_o s, M_a a) the two passes swap roles: d -> -M_a d, so L_m -- and its gradient, the coef = 4 gradient minus the coef = 0 one -- is
    the original's"""
    p = R.make_policy("mixed", norm=True, seed=4)
    tables = _tables(p)
    st = R.make_storage(p, 50, seed=5)
    mst = PM.mirror_storage(st, tables)
    a0, a4 = (PM.loss_autograd_mirror(p, tables, c, st, **KW) for c in (0.0, 4.0))
    b0, b4 = (PM.loss_autograd_mirror(p, tables, c, mst, **KW) for c in (0.0, 4.0))
    assert abs(a4.stats[7] - b4.stats[7]) <= 1e-12 * a4.stats[7] and a0.stats[7] == a4.stats[7]
    term_a, term_b = a4.grad - a0.grad, b4.grad - b0.grad
    assert np.abs(term_a).max() > 1e-3 and R.tensor_errors(p, term_b, term_a).max() <= 1e-10


@pytest.mark.parametrize("n_rows", [17, 100])
@pytest.mark.parametrize("norm", [True, False])
@pytest.mark.parametrize("name", ["tiny", "ppo", "wide", "single"])
def test_parity_rule_rejects_every_mutation(name, norm, n_rows):
    """The rule the GPU test applies (errors against float64 autograd within 3 x float32 autograd's at the median, the 99th percentile and the
    maximum) rejects a float32 gradient whose mirror term is wrong in any of MUTATIONS' ways, at both weights the GPU test trains on."""
    p = R.make_policy(name, norm=norm, seed=1)
    tables = _tables(p)
    st = R.make_storage(p, n_rows, seed=2)
    for coef in (0.5, 4.0):
        ref = PM.loss_autograd_mirror(p, tables, coef, st, "float64", **KW)
        f32 = PM.loss_autograd_mirror(p, tables, coef, st, "float32", **KW)
        yard = R.triple(R.tensor_errors(p, f32.grad, ref.grad))
        assert R.within(yard, yard) and yard[2] < 1e-4
        for how in PM.MUTATIONS:
            bad = PM.loss_autograd_mirror(p, tables, coef, st, "float32", how=how, **KW)
            got = R.triple(R.tensor_errors(p, bad.grad, ref.grad))
            print(f"{name} norm={norm} B={n_rows} coef={coef} {how}: {got} against {yard}")
            assert not R.within(got, yard), (how, got, yard)
            assert got[2] >= 100 * yard[2], (how, got, yard)      # a wiring error, not a rounding: orders above the yardstick
            assert np.allclose(bad.stats[:5], f32.stats[:5], rtol=1e-5, atol=1e-6), how      # PPO's own forward is the right one


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_symmetry_mirror_loss_in_torch_equals_the_checker(dtype):
    """symmetry.mirror_loss over a MirrorTransform built from index lists: the checker's L_m and, through autograd, its gradient"""
    import torch
    from mocca_envs_amd.symmetry import MirrorTransform, mirror_loss, mirror_tables
    from policy_symmetry_reference import sequentials
    p = R.make_policy("ppo", norm=True, seed=5)
    rng = np.random.default_rng(7)
    idx = rng.permutation(52)
    mi = (idx[:9], idx[9:25], idx[25:41], [0, 5, 6], list(range(7, 14)), list(range(14, 21)))
    tables = mirror_tables(mi, 52, 21)
    st = R.make_storage(p, 40, seed=6)
    dt = getattr(torch, dtype)
    actor, _, _ = sequentials(p, dt)
    tr = MirrorTransform(mi, 52, 21)
    tr.obs_sign, tr.act_sign = tr.obs_sign.to(dt), tr.act_sign.to(dt)
    mean, inv_std = torch.tensor(p.obs_mean, dtype=dt), torch.tensor(p.inv_std, dtype=dt)
    loss = mirror_loss(lambda x: actor(((x - mean) * inv_std).clamp(-p.clip, p.clip)), torch.tensor(st["obs"], dtype=dt), tr)
    want = PM.loss_autograd_mirror(p, tables, 0.0, st, dtype, **KW)
    tol = 1e-12 if dtype == "float64" else 1e-5
    assert abs(loss.item() - want.stats[7]) <= tol * want.stats[7]
    grads = torch.autograd.grad(loss, list(actor.parameters()))
    got = np.concatenate([g.numpy().reshape(-1) for g in grads])
    term = (PM.loss_autograd_mirror(p, tables, 1.0, st, "float64", **KW).grad - PM.loss_autograd_mirror(p, tables, 0.0, st, "float64", **KW).grad)[:got.size]
    assert np.abs(got - term).max() <= (1e-10 if dtype == "float64" else 1e-4) * np.abs(term).max()
