"""`BaseController`: the low-level controller of the planner envs as one host object that both env surfaces take.

In Walker3DPlannerEnv / MikePlannerEnv (env_locomotion.py:982-1133) the agent's action is a 15-number plan; `step` feeds
`[robot_state(50), plan * action_scale]` to an actor-critic base controller (:1029-1040, :1093), applies the actor's 21 joint actions and
adds `log(max(1, value)) / 3` to the reward (:1101).  A `BaseController` holds the two MLPs as plain numpy layers:

* `VecEnv(env_id, n, base_controller=ctrl)` / `trainer_api.make_vec_envs(..., base_controller=ctrl)` read `ctrl.actor` / `ctrl.critic` and
  run them on the device (`VecEnv.plan_step`);
* `Walker3DPlannerEnv(base_controller=ctrl)` calls it: `ctrl(base_obs[65]) -> (value, action[21])`, float32 numpy.

A controller trained by this project's own PPO (tools/ppo_demo.py on a Stepper id) also carries observation statistics: `obs_mean` /
`obs_inv_std` over the 65 inputs and `clip`, applied as clamp((x - mean) * inv_std, -clip, clip) in front of both nets
(`BaseController.from_policy_npz`; include/mocca.h mocca_set_base_controller_norm).
"""
from __future__ import annotations

import numpy as np

ACTIVATIONS = ("identity", "relu", "tanh", "softsign")     # index = the activation id of include/mocca.h mocca_set_base_controller
INPUT_DIM, ACTION_DIM, MAX_WIDTH, MAX_LAYERS = 65, 21, 256, 8


def _round16(n):
    return -(-int(n) // 16) * 16


def _net(layers, in_dim, out_dim, name):
    """validated copy of one net: [(W f32 [out][in], b f32 [out], activation)]"""
    layers = list(layers)
    if not 1 <= len(layers) <= MAX_LAYERS:
        raise ValueError(f"{name}: between 1 and {MAX_LAYERS} layers")
    net, fan_in = [], in_dim
    for i, (w, b, act) in enumerate(layers):
        w = np.array(w, dtype=np.float32, order="C")
        b = np.array(b, dtype=np.float32).reshape(-1)
        if act not in ACTIVATIONS:
            raise ValueError(f"{name}[{i}]: unknown activation {act!r} (one of {ACTIVATIONS})")
        if w.ndim != 2 or w.shape[1] != fan_in or b.size != w.shape[0]:
            raise ValueError(f"{name}[{i}]: expected W[out][{fan_in}] and b[out]")
        fan_in = w.shape[0]
        if i + 1 == len(layers):
            if fan_in != out_dim:
                raise ValueError(f"{name}: the last layer has {fan_in} outputs, not {out_dim}")
        elif fan_in % 16 or fan_in > MAX_WIDTH:
            raise ValueError(f"{name}[{i}]: hidden width {fan_in} is not a multiple of 16 up to {MAX_WIDTH}")
        net.append((w, b, act))
    return net


def inv_std_f32(var, eps=1e-8):
    """1 / sqrt(var + eps) in float32: what the kernels multiply by (policy.DevicePolicy and BaseController form it here, so they agree in bits)"""
    return np.float32(1) / np.sqrt(np.array(var, dtype=np.float32).reshape(-1) + np.float32(eps))


def _apply(net, x):
    for w, b, act in net:
        x = x @ w.T + b
        if act == "relu":
            x = np.maximum(x, np.float32(0))
        elif act == "tanh":
            x = np.tanh(x)
        elif act == "softsign":
            x = x / (np.float32(1) + np.abs(x))
    return x


def layer_table(actor, critic, offsets=None):
    """int32 [layers][8], the actor first: net, in, out, in_pad, out_pad, activation id, weight offset, bias offset (include/mocca.h).
    `offsets`: "flat" -- into W[out][in] row-major, then b[out], layer after layer; "image" -- into the layer images below; None -- zeros.
    Checks nothing: the classes' constructors do (_net), and what else reaches the library is the library's to refuse."""
    rows, pos = [], 0
    for net_id, net in enumerate((actor, critic)):
        for w, _, act in net:
            n_out, n_in = np.shape(w)
            p_out, p_in = _round16(n_out), _round16(n_in)
            n_w, n_b = {None: (0, 0), "flat": (n_out * n_in, n_out), "image": (p_out * p_in, p_out)}[offsets]
            rows.append((net_id, n_in, n_out, p_in, p_out, ACTIVATIONS.index(act), pos, pos + n_w))
            pos += n_w + n_b
    return np.array(rows, np.int32).reshape(-1, 8)


def layer_image(w, b):
    """one layer as the kernels read it (csrc/mocca_controller.h) -> (weights float32 [out_pad * in_pad], bias float32 [out_pad]): W padded
    with zeros to multiples of 16 both ways and cut into 16 x 16 blocks [row block][column block][lane 0..63][4] -- lane l of a block holds
    row l % 16, columns 4 (l // 16) .. + 3 -- and the padded bias"""
    n_out, n_in = w.shape
    p_out, p_in = _round16(n_out), _round16(n_in)
    full = np.zeros((p_out, p_in), np.float32)
    full[:n_out, :n_in] = w
    bias = np.zeros(p_out, np.float32)
    bias[:n_out] = b
    blocks = full.reshape(p_out // 16, 16, p_in // 16, 4, 4)                       # [rb][row][cb][quarter][4]
    return blocks.transpose(0, 2, 3, 1, 4).reshape(-1), bias                       # [rb][cb][quarter][row][4]: lane = 16 quarter + row


def layer_image_transposed(w):
    """the second copy of a layer's weights that the PPO backward reads (csrc/mocca_ppo.h: Image): layer_image's fragment order of W.T --
    in and out swap roles and padding -> float32 [in_pad * out_pad]"""
    return layer_image(np.ascontiguousarray(np.asarray(w, np.float32).T), np.zeros(np.shape(w)[1], np.float32))[0]


def unpack_transposed(image, n_in, n_out):
    """layer_image_transposed's inverse -> W float32 [out][in]; non-zero padding is a ValueError"""
    p_in, p_out = _round16(n_in), _round16(n_out)
    full = np.asarray(image, np.float32).reshape(p_in // 16, p_out // 16, 4, 16, 4).transpose(0, 3, 1, 2, 4).reshape(p_in, p_out)
    if full[n_in:].any() or full[:, n_out:].any():
        raise ValueError("padding of a transposed layer image must be zeros")
    return np.ascontiguousarray(full[:n_in, :n_out].T)


def pack_nets(actor, critic):
    """-> (float32 [n]: per layer, actor first, layer_image's weights then its bias; layer_table with the offsets into it)"""
    return np.concatenate([part for w, b, _ in actor + critic for part in layer_image(w, b)]), layer_table(actor, critic, "image")


def unpack_nets(params, table, what):
    """pack_nets' inverse -> [actor, critic]; non-zero padding is a ValueError"""
    params = np.asarray(params, np.float32)
    nets = [[], []]
    for net_id, n_in, n_out, p_in, p_out, act, w_pos, b_pos in np.asarray(table).tolist():
        image = params[w_pos:w_pos + p_in * p_out].reshape(p_out // 16, p_in // 16, 4, 16, 4)
        full = image.transpose(0, 3, 1, 2, 4).reshape(p_out, p_in)
        bias = params[b_pos:b_pos + p_out]
        if full[n_out:].any() or full[:, n_in:].any() or bias[n_out:].any():
            raise ValueError(f"padding of a packed {what} must be zeros")
        nets[net_id].append((full[:n_out, :n_in], bias[:n_out], ACTIVATIONS[act]))
    return nets


def layers_from_sequential(seq, which):
    """a torch.nn.Sequential of Linear, each followed by at most one of ReLU / Tanh / Softsign -> [(W, b, activation)]; any other module
    is a ValueError"""
    from torch import nn
    names = ((nn.ReLU, "relu"), (nn.Tanh, "tanh"), (nn.Softsign, "softsign"))
    out = []
    for mod in seq:
        act = next((n for t, n in names if isinstance(mod, t)), None)
        if isinstance(mod, nn.Linear):
            bias = np.zeros(mod.out_features, np.float32) if mod.bias is None else mod.bias.detach().cpu().numpy()
            out.append((mod.weight.detach().cpu().numpy(), bias, "identity"))
        elif act is not None and out and out[-1][2] == "identity":
            out[-1] = out[-1][:2] + (act,)
        else:
            raise ValueError(f"{which}: {type(mod).__name__} is not supported here (Linear, then at most one of ReLU / Tanh / Softsign)")
    return out


class BaseController:
    def __init__(self, actor, critic, obs_mean=None, obs_inv_std=None, clip=10.0):
        self.actor = _net(actor, INPUT_DIM, ACTION_DIM, "actor")
        self.critic = _net(critic, INPUT_DIM, 1, "critic")
        self.clip = float(clip)
        if not (np.isfinite(self.clip) and self.clip > 0):
            raise ValueError("clip must be finite and positive")
        if (obs_mean is None) != (obs_inv_std is None):
            raise ValueError("obs_mean and obs_inv_std come together, or neither")
        self.obs_mean = self.obs_inv_std = None
        if obs_mean is not None:    # kept as float32 exactly as given
            self.obs_mean = np.array(obs_mean, dtype=np.float32).reshape(-1)
            self.obs_inv_std = np.array(obs_inv_std, dtype=np.float32).reshape(-1)
            if self.obs_mean.size != INPUT_DIM or self.obs_inv_std.size != INPUT_DIM:
                raise ValueError(f"obs_mean / obs_inv_std have {INPUT_DIM} entries")
            if not np.isfinite(self.obs_mean).all() or not np.isfinite(self.obs_inv_std).all() or (self.obs_inv_std < 0).any():
                raise ValueError("obs_mean must be finite, obs_inv_std finite and not negative")

    from_layers = classmethod(lambda cls, actor, critic, **kw: cls(actor, critic, **kw))

    @classmethod
    def from_torch(cls, actor_seq, critic_seq):
        """from two torch.nn.Sequential of Linear / ReLU / Tanh / Softsign; any other module is a ValueError"""
        return cls(layers_from_sequential(actor_seq, "actor"), layers_from_sequential(critic_seq, "critic"))

    @classmethod
    def from_policy_npz(cls, path, eps=1e-8, clip=10.0):
        """from tools/ppo_demo.py's <out>_policy.npz of a Stepper id (65 -> ... -> 21): `pi_<i>_weight` / `pi_<i>_bias` and `vf_*` (tanh between
        the layers, identity heads), `obs_mean`, `obs_var`; inv_std = 1 / sqrt(var + eps) in float32 as policy.DevicePolicy forms it.  A file
        without the critic's `vf_*` arrays is a ValueError: the critic's value is part of the planner envs' reward."""
        with np.load(path, allow_pickle=False) as z:
            def net(prefix):
                idx = sorted(int(k.split("_")[1]) for k in z.files if k.startswith(prefix + "_") and k.endswith("_weight"))
                return [(z[f"{prefix}_{i}_weight"], z[f"{prefix}_{i}_bias"], "identity" if i == idx[-1] else "tanh") for i in idx]
            if not any(k.startswith("pi_") and k.endswith("_weight") for k in z.files):
                raise ValueError(f"{path}: no pi_*_weight arrays: not a policy file of tools/ppo_demo.py")
            if not any(k.startswith("vf_") and k.endswith("_weight") for k in z.files):
                raise ValueError(f"{path}: the critic is missing (no vf_* arrays): a base controller needs the critic the policy was trained with")
            if "obs_mean" not in z.files:
                return cls(net("pi"), net("vf"), clip=clip)
            return cls(net("pi"), net("vf"), obs_mean=z["obs_mean"], obs_inv_std=inv_std_f32(z["obs_var"], eps), clip=clip)

    @classmethod
    def load(cls, path, **kw):
        """either file format, told apart by the keys: save_npz's (`actor/act`) or tools/ppo_demo.py's policy file (`pi_*`)"""
        with np.load(path, allow_pickle=False) as z:
            own = "actor/act" in z.files
        return cls.from_npz(path) if own else cls.from_policy_npz(path, **kw)

    # ---- files: one .npz, arrays "<net>/<i>/W", "<net>/<i>/b" and the activation names "<net>/act" ----
    def save_npz(self, path):
        data = {}
        for which in ("actor", "critic"):
            net = getattr(self, which)
            data[which + "/act"] = np.array([act for _, _, act in net])
            for i, (w, b, _) in enumerate(net):
                data[f"{which}/{i}/W"], data[f"{which}/{i}/b"] = w, b
        if self.obs_mean is not None:
            data["obs_mean"], data["obs_inv_std"], data["clip"] = self.obs_mean, self.obs_inv_std, np.float64(self.clip)
        np.savez(path, **data)

    @classmethod
    def from_npz(cls, path):
        with np.load(path, allow_pickle=False) as z:
            nets = [[(z[f"{which}/{i}/W"], z[f"{which}/{i}/b"], str(act)) for i, act in enumerate(z[which + "/act"])] for which in ("actor", "critic")]
            norm = dict(obs_mean=z["obs_mean"], obs_inv_std=z["obs_inv_std"], clip=float(z["clip"])) if "obs_mean" in z.files else {}
        return cls(*nets, **norm)

    # ---- the callable Walker3DPlannerEnv(base_controller=...) takes ----
    def __call__(self, base_obs):
        x = np.asarray(base_obs, dtype=np.float32)
        if x.shape[-1:] != (INPUT_DIM,):
            raise ValueError(f"base_obs has {INPUT_DIM} entries: robot_state(50) and the scaled plan(15)")
        if self.obs_mean is not None:
            x = np.minimum(np.maximum((x - self.obs_mean) * self.obs_inv_std, np.float32(-self.clip)), np.float32(self.clip))
        return _apply(self.critic, x)[..., 0], _apply(self.actor, x)

    # ---- the image the controller kernel reads (csrc/mocca_controller.h); the library builds the same one from .actor / .critic ----
    def pack(self):
        """-> (params float32 [n], table int32 [layers][8]): per layer, actor first, the weights in fragment order, then the padded bias
        (layer_image); the table's offsets point into params (layer_table)"""
        return pack_nets(self.actor, self.critic)

    @classmethod
    def unpack(cls, params, table):
        """decode pack()'s image back into a controller; non-zero padding is a ValueError"""
        return cls(*unpack_nets(params, table, "controller"))
