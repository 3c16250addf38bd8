"""mocca_ppo_grad without a GPU: the ABI's declaration, binding and export, the transposed fragment order of the weights' second copy,
the reference's hand-written per-row formulas against autograd, and the unchanged image of DevicePolicy.pack().  The checker is
tests/ppo_reference.py."""
import os
import re
import subprocess

import numpy as np
import pytest

import ppo_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "mocca.h")).read()


def test_header_declares_and_binding_lists_mocca_ppo_grad():
    from mocca_envs_amd import lib
    assert re.search(r"\bint mocca_ppo_grad\(mocca_handle h,", _header())
    res, args = lib.SYMBOLS["mocca_ppo_grad"]
    assert len(args) == 17       # h, obs, stride, action, old_logp, adv, returns, old_value, idx, n_rows, 3 doubles, value_clip, grad, stats, stream


def test_abi_version_is_still_8():
    from mocca_envs_amd import lib
    assert re.search(r"#define MOCCA_ABI_VERSION 8\b", _header()) and lib.ABI_VERSION == 8


def test_library_exports_mocca_ppo_grad():
    from mocca_envs_amd.build import build_lib
    names = subprocess.run(["nm", "-D", "--defined-only", build_lib()], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT mocca_ppo_grad\b", names)


@pytest.mark.parametrize("n_in,n_out", [(5, 16), (52, 256), (256, 21), (336, 256)])
def test_transposed_fragment_order_round_trips(n_in, n_out):
    """the second copy is layer_image's order of W.T: lane l of block (row block of in, column block of out) holds W.T[16 rb + l % 16][16 cb +
    4 (l // 16) + 0..3]; checked element by element against W.T, then through the inverse"""
    from mocca_envs_amd.controller import _round16, layer_image_transposed, unpack_transposed
    w = np.random.default_rng(n_in).normal(size=(n_out, n_in)).astype(np.float32)
    image = layer_image_transposed(w)
    p_in, p_out = _round16(n_in), _round16(n_out)
    assert image.shape == (p_in * p_out,)
    wt = np.zeros((p_in, p_out), np.float32)
    wt[:n_in, :n_out] = w.T
    blocks = image.reshape(p_in // 16, p_out // 16, 64, 4)
    for rb, cb, lane in ((0, 0, 0), (p_in // 16 - 1, p_out // 16 - 1, 63), (p_in // 32, p_out // 32, 37)):
        assert np.array_equal(blocks[rb, cb, lane], wt[16 * rb + lane % 16, 16 * cb + 4 * (lane // 16):][:4])
    i = np.arange(image.size)
    rb, rem = i // (p_out * 16), i % (p_out * 16)
    cb, lane, j = rem // 256, (rem % 256) // 4, rem % 4
    assert np.array_equal(image, wt[16 * rb + lane % 16, 16 * cb + 4 * (lane // 16) + j])     # the repack kernel's index arithmetic
    assert np.array_equal(unpack_transposed(image, n_in, n_out), w)


@pytest.mark.parametrize("value_clip", [False, True])
@pytest.mark.parametrize("act", ["identity", "relu", "tanh", "softsign"])
def test_hand_formulas_equal_autograd_in_f64(act, value_clip):
    """every activation, both value_clip settings, rows on both sides of both clip bounds (make_storage's ratios) and, for value_clip, on
    both sides of the value clamp: 1e-12 relative to the largest gradient entry of each tensor"""
    p = R.make_policy("mixed", norm=True, seed=3, acts=[act, act, act])
    st = R.make_storage(p, 64, seed=1)
    ratio = np.exp(R.loss_autograd(p, st).logp - st["old_logp"])
    assert (ratio < 0.8).any() and ((ratio > 0.8) & (ratio < 1)).any() and ((ratio > 1) & (ratio < 1.2)).any() and (ratio > 1.2).any()
    kw = dict(value_coef=0.5, entropy_coef=0.01, value_clip=value_clip)
    want, got = R.loss_autograd(p, st, **kw).grad, R.grad_by_hand(p, st, **kw)
    assert R.tensor_errors(p, got, want).max() <= 1e-12


def test_pack_image_is_unchanged():
    """DevicePolicy.pack()'s image: what pack_nets gives for the layers, then log_std [32], flags [4], mean and inv_std [in_pad] -- the
    transposed copies are not part of it"""
    from mocca_envs_amd.controller import pack_nets
    from mocca_envs_amd.policy import DevicePolicy
    p = R.make_policy("ppo", norm=True, seed=2)
    dp = DevicePolicy(p.actor, p.critic, p.log_std, obs_mean=p.obs_mean, inv_std=p.inv_std, clip=p.clip)
    image, table, off = dp.pack()
    params, want_table = pack_nets(dp.actor, dp.critic)
    tail = np.zeros(32 + 4 + 2 * 64, np.float32)
    tail[:21], tail[32] = p.log_std, 1.0
    tail[36:36 + 52], tail[100:100 + 52] = p.obs_mean, p.inv_std
    assert image.tobytes() == np.concatenate([params, tail]).tobytes() and np.array_equal(table, want_table)
    assert off["log_std"] == params.size and image.size == params.size + tail.size


def test_n_head_and_split_grad():
    from mocca_envs_amd.policy import DevicePolicy
    p = R.make_policy("mixed", norm=True)
    dp = DevicePolicy(p.actor, p.critic, p.log_std, obs_mean=p.obs_mean, inv_std=p.inv_std, clip=p.clip)
    flat = dp.flat_params()
    assert dp.n_head() == flat.size - 2 * dp.in_dim == R.flat_params(p).size
    parts = dp.split_grad(flat)
    for name, net in (("actor", dp.actor), ("critic", dp.critic)):
        for (w, b), (w0, b0, _) in zip(parts[name], net):
            assert np.array_equal(w, w0) and np.array_equal(b, b0)
    assert np.array_equal(parts["log_std"], dp.log_std)
    parts["log_std"][:] = 7.0      # views, not copies
    assert (flat[dp.n_head() - dp.act_dim:dp.n_head()] == 7.0).all()
