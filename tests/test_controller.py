"""The planner envs' base controller without a GPU: `mocca_envs_amd.controller.BaseController` (forward, constructors, files, the packed
image), the ABI's new entry points on a NULL handle, and the checker the GPU tests rely on (tests/controller_reference.py): its float64
forward agrees with torch, its factory exercises both branches of the reward's max(1, value), its mutation controls are far outside any
rounding bound."""
import ctypes as C

import numpy as np
import pytest

import controller_reference as R


@pytest.fixture(scope="module")
def lib():
    from mocca_envs_amd.build import build_lib
    from mocca_envs_amd import lib as L
    build_lib()
    return L.load()


def test_new_entry_points_refuse_a_null_handle(lib):
    from mocca_envs_amd import lib as L
    assert L.ABI_VERSION == 8 and lib.mocca_abi_version() == 8
    params, table = np.zeros(4, np.float32), np.zeros((2, 8), np.int32)
    assert lib.mocca_set_base_controller(None, params.ctypes.data_as(C.c_void_p), params.size, table.ctypes.data_as(C.c_void_p), 2, 2.0) == -1
    assert lib.mocca_set_base_controller(None, None, 0, None, 0, 0.0) == -1
    assert lib.mocca_plan_step(None, None, None, None, None, None, None) == -1
    assert lib.mocca_get_base_outputs(None, None, None, None) == -1
    assert lib.mocca_plan_dim(None) == -1


@pytest.mark.parametrize("kind", sorted(R.SHAPES))
def test_f64_helper_agrees_with_torch_and_the_factory_covers_both_reward_branches(kind):
    import torch
    ctrl = R.random_controller(kind, seed=3)
    assert ctrl.actor[0][0].shape[1] == 65 and ctrl.actor[-1][0].shape[0] == 21 and ctrl.critic[-1][0].shape[0] == 1
    assert len(ctrl.actor) <= 8 and len(ctrl.critic) <= 8
    rs, plan = R.plausible_inputs(1000, seed=11)
    v64, a64 = R.forward64(ctrl, rs, plan)
    # torch CPU float32 forward (how the reference runs the controller): the yardstick of the GPU parity test
    acts = {"relu": torch.relu, "tanh": torch.tanh, "softsign": torch.nn.functional.softsign, "identity": lambda t: t}

    def net32(layers, x):
        for w, b, act in layers:
            x = acts[act](torch.nn.functional.linear(x, torch.from_numpy(w), torch.from_numpy(b)))
        return x.numpy()

    x = torch.from_numpy(R.base_obs(rs, plan).astype(np.float32))
    e = np.concatenate([R.error_units(net32(ctrl.actor, x), a64).ravel(), R.error_units(net32(ctrl.critic, x)[:, 0], v64)])
    med, p99, mx = R.triple(e)
    assert med < 1.0 and mx < 50.0, (med, p99, mx)          # float32 rounding, nothing else
    frac = float((v64 > 1.0).mean())
    assert 0.1 <= frac <= 0.9, frac                          # both branches of max(1, value)
    # the mutation controls are errors of another order than rounding
    for how in ("bias", "activation"):
        if how == "activation" and not any(a in ("relu", "softsign") for _, _, a in ctrl.actor + ctrl.critic):
            continue
        vm, am = R.forward64(R.mutated(ctrl, how), rs, plan)
        assert R.triple(np.concatenate([R.error_units(am, a64).ravel(), R.error_units(vm, v64)]))[1] > 1000.0, how
    v1, a1 = R.forward64(ctrl, rs, plan, action_scale=1.0)
    assert R.triple(np.concatenate([R.error_units(a1, a64).ravel(), R.error_units(v1, v64)]))[1] > 1000.0


def test_multi_handle_envs_refuse_a_base_controller():
    from mocca_envs_amd.multi import SubBatchedVecEnv
    with pytest.raises(ValueError):
        SubBatchedVecEnv("MikePlannerEnv-v0", 64, sub_batches=2, device=0, base_controller=R.random_controller("small"))


def _bc(kind, seed=3):
    from mocca_envs_amd.controller import BaseController
    c = R.random_controller(kind, seed=seed)
    return BaseController.from_layers(c.actor, c.critic)


@pytest.mark.parametrize("kind", sorted(R.SHAPES))
def test_base_controller_forward_is_the_f64_forward_to_f32_rounding(kind):
    ctrl = _bc(kind)
    rs, plan = R.plausible_inputs(1000, seed=5)
    x = R.base_obs(rs, plan).astype(np.float32)
    value, action = ctrl(x)
    assert value.dtype == np.float32 and action.dtype == np.float32 and value.shape == (1000,) and action.shape == (1000, 21)
    v64, a64 = R.forward64(ctrl, rs, plan)
    med, p99, mx = R.triple(np.concatenate([R.error_units(action, a64).ravel(), R.error_units(value, v64)]))
    # float32 rounding through at most 8 layers of width <= 256: well under one unit (1e-6 relative) at the median, a few units at worst
    assert med < 0.5 and mx < 20.0, (med, p99, mx)
    v1, a1 = ctrl(x[7])                                     # one observation: the single-env protocol (value scalar, action[21])
    assert np.shape(v1) == () and a1.shape == (21,)
    assert abs(float(v1) - float(value[7])) <= 1e-5 * (1 + abs(float(value[7]))) and np.allclose(a1, action[7], rtol=1e-5, atol=1e-5)
    with pytest.raises(ValueError):
        ctrl(np.zeros(64, np.float32))


def test_from_torch_equals_from_layers_and_refuses_other_modules():
    import torch
    from torch import nn
    from mocca_envs_amd.controller import BaseController
    torch.manual_seed(0)
    actor = nn.Sequential(nn.Linear(65, 32), nn.Softsign(), nn.Linear(32, 64), nn.ReLU(), nn.Linear(64, 21), nn.Tanh())
    critic = nn.Sequential(nn.Linear(65, 16), nn.ReLU(), nn.Linear(16, 1))
    a = BaseController.from_torch(actor, critic)
    lay = lambda seq, acts: [(m.weight.detach().numpy(), m.bias.detach().numpy(), act) for m, act in zip([m for m in seq if isinstance(m, nn.Linear)], acts)]
    b = BaseController.from_layers(lay(actor, ["softsign", "relu", "tanh"]), lay(critic, ["relu", "identity"]))
    for na, nb in ((a.actor, b.actor), (a.critic, b.critic)):
        assert len(na) == len(nb)
        for (w1, b1, a1), (w2, b2, a2) in zip(na, nb):
            assert a1 == a2 and np.array_equal(w1, w2) and np.array_equal(b1, b2)
    x = R.base_obs(*R.plausible_inputs(50, seed=2)).astype(np.float32)
    with torch.no_grad():
        assert np.allclose(a(x)[1], actor(torch.from_numpy(x)).numpy(), rtol=1e-5, atol=1e-6)
        assert np.allclose(a(x)[0], critic(torch.from_numpy(x)).numpy()[:, 0], rtol=1e-5, atol=1e-6)
    for bad in (nn.Sequential(nn.Linear(65, 16), nn.LayerNorm(16), nn.Linear(16, 21)), nn.Sequential(nn.Linear(65, 16), nn.Sigmoid(), nn.Linear(16, 21)),
                nn.Sequential(nn.ReLU(), nn.Linear(65, 21)), nn.Sequential(nn.Linear(65, 16), nn.ReLU(), nn.Tanh(), nn.Linear(16, 21))):
        with pytest.raises(ValueError):
            BaseController.from_torch(bad, critic)


def test_unsupported_widths_layers_and_activations_raise():
    from mocca_envs_amd.controller import BaseController
    z = lambda o, i: (np.zeros((o, i), np.float32), np.zeros(o, np.float32), "relu")
    head, crit = [z(21, 65)], [z(1, 65)]
    BaseController(head, crit)
    for actor, critic in (([z(40, 65), z(21, 40)], crit),           # hidden width not a multiple of 16
                          ([z(272, 65), z(21, 272)], crit),         # wider than 256
                          ([z(21, 64)], crit),                      # not the 65-float input
                          ([z(20, 65)], crit), (head, [z(2, 65)]),  # wrong heads
                          ([z(16, 65)] * 1 + [z(16, 16)] * 7 + [z(21, 16)], crit),   # 9 layers
                          ([], crit),
                          ([(np.zeros((21, 65)), np.zeros(21), "gelu")], crit),
                          ([(np.zeros((21, 65)), np.zeros(20), "relu")], crit)):
        with pytest.raises(ValueError):
            BaseController(actor, critic)


@pytest.mark.parametrize("kind", sorted(R.SHAPES))
def test_npz_round_trip_is_bit_exact_and_pack_decodes_back(kind, tmp_path):
    from mocca_envs_amd.controller import BaseController
    ctrl = _bc(kind)
    path = str(tmp_path / "ctrl.npz")
    ctrl.save_npz(path)
    back = BaseController.from_npz(path)
    params, table = ctrl.pack()
    unpacked = BaseController.unpack(params, table)
    for other in (back, unpacked):
        for na, nb in ((ctrl.actor, other.actor), (ctrl.critic, other.critic)):
            assert len(na) == len(nb)
            for (w1, b1, a1), (w2, b2, a2) in zip(na, nb):
                assert a1 == a2 and w1.dtype == w2.dtype == np.float32 and np.array_equal(w1.view(np.uint32), w2.view(np.uint32)) \
                    and np.array_equal(b1.view(np.uint32), b2.view(np.uint32))
    # the image: float32, one table row per layer (actor first), every float either a weight, a bias or a zero of the padding
    assert params.dtype == np.float32 and table.dtype == np.int32 and table.shape == (len(ctrl.actor) + len(ctrl.critic), 8)
    assert table[:, 0].tolist() == [0] * len(ctrl.actor) + [1] * len(ctrl.critic)
    assert (table[:, 3] % 16 == 0).all() and (table[:, 4] % 16 == 0).all() and (table[:, 6] % 4 == 0).all() and (table[:, 7] % 4 == 0).all()
    assert table[0, 3] == 80 and table[len(ctrl.actor) - 1, 4] == 32 and table[-1, 4] == 16
    n_real = sum(w.size + b.size for w, b, _ in ctrl.actor + ctrl.critic)
    assert params.size == int((table[:, 3] * table[:, 4] + table[:, 4]).sum())
    assert np.count_nonzero(params) <= n_real and np.count_nonzero(params) == sum(np.count_nonzero(w) + np.count_nonzero(b) for w, b, _ in ctrl.actor + ctrl.critic)
    # lane map of the first block of the first layer: lane l holds row l % 16, columns 4 (l // 16) .. + 3
    w0 = ctrl.actor[0][0]
    blk = params[:256].reshape(64, 4)
    for l in (0, 5, 17, 63):
        assert np.array_equal(blk[l], w0[l % 16, 4 * (l // 16):4 * (l // 16) + 4])
    dirty = params.copy()
    dirty[int(table[0, 6]) + 4 * 256 + 16 * 4 + 1] = 1.0      # block (0, 4), lane 16 (columns 68 ..): padding of the 65-wide input
    with pytest.raises(ValueError):
        BaseController.unpack(dirty, table)
