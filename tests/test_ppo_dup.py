"""mocca_ppo_grad_dup and mocca_set_policy_mirror_dup without a GPU: the ABI's declarations, bindings and exports, the header's by-hand
lines against float64 autograd, the identity tables against the plain checker, the teeth of the parity rule (every way of forming the
twins wrongly is rejected by it) and symmetry.duplicate_minibatch in torch.  The checker is tests/ppo_dup_reference.py."""
import os
import re
import subprocess

import numpy as np
import pytest

import ppo_dup_reference as PD
import ppo_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KW = dict(value_coef=0.5, entropy_coef=0.01)


def _header():
    return open(os.path.join(ROOT, "include", "mocca.h")).read()


def _tables(p, seed=3):
    """random tables with at least one swapped pair and one negative sign on both sides: with less, a mutation could not be seen"""
    in_dim, act_dim = p.actor[0][0].shape[1], p.log_std.size
    for s in range(seed, seed + 64):
        t = PD.random_tables(in_dim, s, act_dim)
        if all((np.asarray(perm) != np.arange(len(perm))).any() and (np.asarray(sign) < 0).any() for perm, sign in (t[:2], t[2:])):
            return t
    raise AssertionError("no tables with a swapped pair and a negative sign on both sides")


def test_header_declares_and_binding_lists_the_two_entry_points():
    from mocca_envs_amd import lib
    assert re.search(r"\bint mocca_ppo_grad_dup\(mocca_handle h,", _header())
    assert re.search(r"\bint mocca_set_policy_mirror_dup\(mocca_handle h,[^;]*const float \*act_sign_host\);", _header())
    assert lib.SYMBOLS["mocca_ppo_grad_dup"] == lib.SYMBOLS["mocca_ppo_grad"]      # the same argument list
    assert lib.SYMBOLS["mocca_set_policy_mirror_dup"] == lib.SYMBOLS["mocca_set_policy_symmetry"]
    assert re.search(r"#define MOCCA_ABI_VERSION 8\b", _header()) and lib.ABI_VERSION == 8      # additive
    assert "off-policy" in _header().lower() and "pi_old(M_a a | M_o s)" in _header()      # the method's assumption and what is out of scope


def test_library_exports_the_two_entry_points():
    from mocca_envs_amd.build import build_lib
    names = subprocess.run(["nm", "-D", "--defined-only", build_lib()], capture_output=True, text=True, check=True).stdout
    for name in ("mocca_ppo_grad_dup", "mocca_set_policy_mirror_dup", "mocca_ppo_grad", "mocca_ppo_grad_sym", "mocca_ppo_grad_mirror"):
        assert re.search(rf"\bT {name}\b", names), name


@pytest.mark.parametrize("value_clip", [False, True])
@pytest.mark.parametrize("act", ["identity", "relu", "tanh", "softsign"])
def test_hand_formulas_equal_autograd_in_f64(act, value_clip):
    """the header's lines, once per kind of sample with ib = 1 / (2 B) and the sums added, against float64 autograd of the plain loss on
    the concatenated rows: 1e-10 relative to the largest entry of each tensor; the twins' share of stats[3] to 1e-12"""
    p = PD.make_policy("mixed", norm=True, seed=3, acts=[act, act, act])
    tables = _tables(p)
    st = PD.make_storage_dup(p, tables, 64, seed=1)
    kw = dict(KW, value_clip=value_clip)
    want = PD.loss_autograd_dup(p, tables, st, **kw)
    got, share = PD.grad_by_hand_dup(p, tables, st, **kw)
    assert R.tensor_errors(p, got, want.grad).max() <= 1e-10
    assert abs(share - want.stats[7]) <= 1e-12 * (1 + abs(want.stats[7])) and want.stats[6] == 0.0
    assert want.logp.shape == (128,) and want.value.shape == (128,)


@pytest.mark.parametrize("name", sorted(R.NETS))
def test_storage_keeps_both_kinds_of_sample_on_policy_and_off_every_tie(name):
    """make_storage_dup: rows and twins have ratios next to ppo_reference.RATIOS -- both reach the actor --, and no ratio or value gap of
    either kind sits on a clip bound"""
    p = PD.make_policy(name, norm=True, seed=1)
    tables = _tables(p)
    st = PD.make_storage_dup(p, tables, 100, seed=2)
    ref = PD.loss_autograd_dup(p, tables, st, value_clip=True, **KW)
    r = np.exp(ref.logp - np.concatenate([st["old_logp"], st["old_logp"]]).astype(np.float64))
    nearest = np.abs(r[:, None] / np.asarray(R.RATIOS)[None, :] - 1).min(1)
    assert nearest.max() < 0.012 and np.abs(r - 0.8).min() > 0.05 and np.abs(r - 1.2).min() > 0.05
    assert 0.2 < ref.stats[4] < 0.8
    dd = np.abs(ref.value - np.concatenate([st["old_value"], st["old_value"]]))
    assert np.abs(dd - R.CLIP).min() > 0.049
    assert not np.array_equal(ref.logp[:100], ref.logp[100:])
    z = (PD.concatenate(st, tables)["action"] - R.loss_autograd(p, PD.concatenate(st, tables)).pre[len(p.actor) - 1]) / np.exp(p.log_std.astype(np.float64))
    assert np.sqrt((z * z).mean()) < 1.5      # both kinds of sample at a rollout's |z|


@pytest.mark.parametrize("n_rows", [17, 100])
@pytest.mark.parametrize("norm", [True, False])
@pytest.mark.parametrize("name", sorted(R.NETS))
def test_parity_rule_rejects_every_mutation(name, norm, n_rows):
    """The rule the GPU test applies (errors against float64 autograd within 3 x float32 autograd's at the median, the 99th percentile and the
    maximum) rejects a float32 gradient whose twins are formed wrongly in any of MUTATIONS' ways, on every net of ppo_reference.NETS.
    Precondition: the tables swap a pair and negate an entry on both sides -- with identity tables a twin IS its row and no mutation of the
    mirror could be seen."""
    p = PD.make_policy(name, norm=norm, seed=1)
    tables = _tables(p)
    for perm, sign in (tables[:2], tables[2:]):
        assert (np.asarray(perm) != np.arange(len(perm))).any() and (np.asarray(sign) < 0).any()
    st = PD.make_storage_dup(p, tables, n_rows, seed=2)
    ref = PD.loss_autograd_dup(p, tables, st, "float64", **KW)
    f32 = PD.loss_autograd_dup(p, tables, st, "float32", **KW)
    yard = R.triple(R.tensor_errors(p, f32.grad, ref.grad))
    assert R.within(yard, yard) and yard[2] < 1e-4
    for how in PD.MUTATIONS:
        bad = PD.loss_autograd_dup(p, tables, st, "float32", how=how, **KW)
        got = R.triple(R.tensor_errors(p, bad.grad, ref.grad))
        print(f"{name} norm={norm} B={n_rows} {how}: {got} against {yard}")
        assert not R.within(got, yard), (how, got, yard)
        assert got[2] >= 100 * yard[2], (how, got, yard)      # a wiring error, not a rounding: orders above the yardstick


@pytest.mark.parametrize("value_clip", [False, True])
def test_identity_tables_give_the_plain_gradient(value_clip):
    """perm = arange, sign = +1: a twin is its row, the 2 B-sample mean is the B-row mean, and the gradient is ppo_reference.loss_autograd's
    at float64; the twins' share of stats[3] is half of it"""
    p = R.make_policy("mixed", norm=True, seed=2)
    st = R.make_storage(p, 50, seed=3)
    tables = PD.identity_tables(65, 21)
    kw = dict(KW, value_clip=value_clip)
    plain, got = R.loss_autograd(p, st, **kw), PD.loss_autograd_dup(p, tables, st, **kw)
    assert R.tensor_errors(p, got.grad, plain.grad).max() <= 1e-12
    assert np.allclose(got.stats[:5], plain.stats[:5], rtol=1e-12, atol=0) and got.stats[4] == plain.stats[4]
    assert abs(got.stats[7] - 0.5 * plain.stats[3]) <= 1e-12 * abs(plain.stats[3])
    by_hand, share = PD.grad_by_hand_dup(p, tables, st, **kw)
    assert R.tensor_errors(p, by_hand, plain.grad).max() <= 1e-12 and abs(share - got.stats[7]) <= 1e-12 * abs(got.stats[7])


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_symmetry_duplicate_minibatch_equals_the_checkers_concatenation(dtype):
    """symmetry.duplicate_minibatch over a MirrorTransform built from index lists: the checker's concatenate() on symmetry.mirror_tables
    of the same lists, bit for bit in all six tensors; old_value None stays None"""
    import torch
    from mocca_envs_amd.symmetry import MirrorTransform, duplicate_minibatch, mirror_tables
    p = R.make_policy("ppo", norm=True, seed=5)
    rng = np.random.default_rng(7)
    idx = rng.permutation(52)
    mi = (idx[:9], idx[9:25], idx[25:41], [0, 5, 6], list(range(7, 14)), list(range(14, 21)))
    tables = mirror_tables(mi, 52, 21)
    st = {k: v.astype(dtype) for k, v in R.make_storage(p, 40, seed=6).items()}
    dt = getattr(torch, dtype)
    tr = MirrorTransform(mi, 52, 21)
    tr.obs_sign, tr.act_sign = tr.obs_sign.to(dt), tr.act_sign.to(dt)
    keys = ("obs", "action", "old_logp", "adv", "returns", "old_value")
    got = duplicate_minibatch(*[torch.tensor(st[k]) for k in keys], tr)
    want = PD.concatenate(st, tables)
    for k, g in zip(keys, got):
        assert g.dtype == dt and g.shape[0] == 80
        assert np.array_equal(g.numpy().view(np.uint8), np.ascontiguousarray(want[k]).view(np.uint8)), k
    assert duplicate_minibatch(*[torch.tensor(st[k]) for k in keys[:5]], None, tr)[5] is None
