"""Checker for the planner envs' base controller: an independent numpy float64 forward and a seeded factory of random controllers.

A controller here is a pair (actor, critic) of layer lists [(W[out][in], b[out], activation)] -- what `VecEnv.set_base_controller` takes."""
from types import SimpleNamespace

import numpy as np

ROBOT_STATE, PLAN, ACTION = 50, 15, 21
SHAPES = {
    # the reference's shipped controller as VERDICT recovered it: 65-256x5-21 and 65-256x4-1
    "reference": (([256] * 5, ["softsign"] * 5 + ["identity"]), ([256] * 4, ["relu"] * 4 + ["identity"])),
    "small": (([48], ["tanh", "identity"]), ([16], ["softsign", "identity"])),
    "deep8": (([32, 64, 16, 128, 48, 256, 80], ["relu", "tanh", "softsign", "identity", "relu", "softsign", "tanh", "tanh"]),
              ([16, 256, 32, 32, 112, 64, 16], ["softsign", "relu", "relu", "tanh", "identity", "relu", "softsign", "identity"])),
}


def act64(x, act):
    if act == "relu":
        return np.maximum(x, 0.0)
    if act == "tanh":
        return np.tanh(x)
    if act == "softsign":
        return x / (1.0 + np.abs(x))
    assert act == "identity"
    return x


def net64(layers, x):
    x = np.asarray(x, np.float64)
    for w, b, act in layers:
        x = act64(x @ np.asarray(w, np.float64).T + np.asarray(b, np.float64), act)
    return x


def base_obs(robot_state, plan, action_scale=2.0):
    """[robot_state(50), plan * action_scale] as float32 values (the product is formed in float32, as the env does), in float64."""
    p = (np.asarray(plan, np.float32) * np.float32(action_scale)).astype(np.float32)
    return np.concatenate([np.asarray(robot_state, np.float32), p], axis=-1).astype(np.float64)


def forward64(ctrl, robot_state, plan, action_scale=2.0):
    """-> (value [B], action [B, 21]) in float64."""
    x = base_obs(robot_state, plan, action_scale)
    return net64(ctrl.critic, x)[..., 0], net64(ctrl.actor, x)


def plausible_inputs(n, seed=0):
    """robot states clipped to +-5 (calc_state clips there) and plans ~ N(0, 1)"""
    rng = np.random.default_rng(seed)
    return np.clip(rng.normal(0, 1.5, (n, ROBOT_STATE)), -5, 5).astype(np.float32), rng.normal(0, 1, (n, PLAN)).astype(np.float32)


def random_controller(kind="reference", seed=0):
    """Weights ~ N(0, 1 / fan_in), biases ~ N(0, 0.1^2).  The critic's head bias is then set so that over plausible inputs the value's median
    is 1: both branches of max(1, value) in the reward occur."""
    rng = np.random.default_rng([seed, sorted(SHAPES).index(kind)])

    def net(hidden, acts, out):
        dims, layers = [ROBOT_STATE + PLAN] + list(hidden) + [out], []
        for i, act in enumerate(acts):
            layers.append((rng.normal(0, 1 / np.sqrt(dims[i]), (dims[i + 1], dims[i])).astype(np.float32),
                           rng.normal(0, 0.1, dims[i + 1]).astype(np.float32), act))
        return layers

    (ah, aa), (ch, ca) = SHAPES[kind]
    ctrl = SimpleNamespace(actor=net(ah, aa, ACTION), critic=net(ch, ca, 1))
    rs, plan = plausible_inputs(2000, seed=seed + 1)
    v = forward64(ctrl, rs, plan)[0]
    w, b, act = ctrl.critic[-1]
    ctrl.critic[-1] = (w, (b + np.float32(1.0 - np.median(v))).astype(np.float32), act)
    return ctrl


def mutated(ctrl, how):
    """A controller that differs from `ctrl` the way a kernel bug would: one hidden bias dropped, or relu <-> softsign swapped."""
    actor, critic = [tuple(l) for l in ctrl.actor], [tuple(l) for l in ctrl.critic]
    if how == "bias":
        for net in (actor, critic):
            w, b, act = net[0]
            net[0] = (w, np.zeros_like(b), act)
    elif how == "activation":
        swap = {"relu": "softsign", "softsign": "relu"}
        actor = [(w, b, swap.get(a, a)) for w, b, a in actor]
        critic = [(w, b, swap.get(a, a)) for w, b, a in critic]
    else:
        raise ValueError(how)
    return SimpleNamespace(actor=actor, critic=critic)


def error_units(got, want):
    """|got - want| in units of 1e-6 (1 + |want|)"""
    want = np.asarray(want, np.float64)
    return np.abs(np.asarray(got, np.float64) - want) / (1e-6 * (1.0 + np.abs(want)))


def triple(e):
    e = np.asarray(e).ravel()
    return float(np.median(e)), float(np.percentile(e, 99)), float(e.max())
