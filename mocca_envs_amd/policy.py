"""`DevicePolicy`: a trainer's Gaussian actor-critic as one host object that both env surfaces take.

The reference's trainers (SymmetricRL, ALLSTEPS: pytorch-a2c-ppo-acktr's `Policy`) act with a diagonal-Gaussian actor MLP, a critic MLP, a
state-independent `log_std` and, optionally, a running observation normalisation.  A `DevicePolicy` holds those as plain numpy arrays:

* `VecEnv.set_policy(p)` / `TorchVecEnv.attach_policy(p)` run it on the device, one launch in front of the step kernel
  (`act`, `act_step`; include/mocca.h mocca_act); `update_policy` refreshes the weights once per PPO iteration;
* the single-env gym classes call it: `p(obs[in_dim]) -> (action, logp, value, mean)`, float32 numpy.

With `symmetry=` (symmetry.mirror_tables) the policy is SymmetricRL's symmetric network, mirror-symmetric by construction
(csrc/mocca_policy.h: Symmetry); the tables are not parameters: `flat_params()`, `pack()`, `unpack()` and `table()` do not see them.

A PRIVILEGED CRITIC (an asymmetric actor-critic; csrc/mocca_policy.h: Privileged critic): the critic's first layer may take an input of its
own, `critic_in_dim` floats (inferred from it), with statistics of its own (`critic_obs_mean`, `critic_obs_var` / `critic_inv_std`).  Such a
policy is `asymmetric`: `__call__(obs, critic_obs=...)` feeds the critic its rows, `flat_params()` ends in mean, inv_std, critic_mean,
critic_inv_std (all four or none) and `pack()` carries the two extra arrays behind inv_std.  A plain policy's outputs are unchanged.
"""
from __future__ import annotations

import numpy as np

from .controller import _apply, _net, _round16, inv_std_f32, layer_table, layers_from_sequential, pack_nets, unpack_nets

MAX_IN, MAX_ACTION, FLAG_WORDS = 336, 32, 4       # csrc/mocca_policy.h POL_MAX_IN / POL_MAX_ACTION / POL_FLAG_WORDS
HALF_LOG_2PI = 0.9189385332046727


class DevicePolicy:
    def __init__(self, actor, critic, log_std, obs_mean=None, obs_var=None, eps=1e-8, clip=10.0, inv_std=None, symmetry=None,
                 critic_obs_mean=None, critic_obs_var=None, critic_inv_std=None):
        actor, critic = list(actor), list(critic)
        self.in_dim = int(np.shape(actor[0][0])[1])
        self.critic_in_dim = int(np.shape(critic[0][0])[1])
        self.log_std = np.array(log_std, dtype=np.float32).reshape(-1)
        self.act_dim = int(self.log_std.size)
        if not 1 <= self.in_dim <= MAX_IN or not 1 <= self.act_dim <= MAX_ACTION or not 1 <= self.critic_in_dim <= MAX_IN:
            raise ValueError(f"in_dim and critic_in_dim must be 1 .. {MAX_IN} and act_dim 1 .. {MAX_ACTION}")
        self.actor = _net(actor, self.in_dim, self.act_dim, "actor")
        self.critic = _net(critic, self.critic_in_dim, 1, "critic")
        self.clip = float(clip)
        if not (np.isfinite(self.clip) and self.clip > 0):
            raise ValueError("clip must be finite and positive")
        self.obs_mean = self.inv_std = None
        if obs_mean is not None:
            self.obs_mean = np.array(obs_mean, dtype=np.float32).reshape(-1)
            if inv_std is None:
                inv_std = inv_std_f32(obs_var, eps)
            self.inv_std = np.array(inv_std, dtype=np.float32).reshape(-1)
            if self.obs_mean.size != self.in_dim or self.inv_std.size != self.in_dim:
                raise ValueError(f"obs_mean / obs_var have {self.in_dim} entries")
        self.critic_obs_mean = self.critic_inv_std = None
        if critic_obs_mean is not None:
            self.critic_obs_mean = np.array(critic_obs_mean, dtype=np.float32).reshape(-1)
            if critic_inv_std is None:
                critic_inv_std = inv_std_f32(critic_obs_var, eps)
            self.critic_inv_std = np.array(critic_inv_std, dtype=np.float32).reshape(-1)
            if self.critic_obs_mean.size != self.critic_in_dim or self.critic_inv_std.size != self.critic_in_dim:
                raise ValueError(f"critic_obs_mean / critic_obs_var have {self.critic_in_dim} entries")
        if (self.critic_obs_mean is None) != (self.obs_mean is None) and (self.critic_obs_mean is not None or self.critic_in_dim != self.in_dim):
            raise ValueError("an asymmetric policy carries the statistics of both nets or of neither (one flag switches both)")
        self.symmetry = None
        if symmetry is not None:    # (in_perm, in_sign, act_perm, act_sign)
            from .symmetry import check_tables
            if self.asymmetric:
                raise ValueError("a policy with a privileged critic takes no mirror tables (none are provided for the critic's row)")
            self.symmetry = check_tables(symmetry, self.in_dim, self.act_dim)

    @property
    def asymmetric(self) -> bool:
        """does the critic read rows of its own (include/mocca.h mocca_set_policy_priv): another width, or statistics of its own"""
        return self.critic_in_dim != self.in_dim or self.critic_obs_mean is not None

    def with_symmetry(self, symmetry):
        """a copy of this policy (the arrays are shared) with the mirror tables `symmetry`; None: without any"""
        import copy
        from .symmetry import check_tables
        if symmetry is not None and self.asymmetric:
            raise ValueError("a policy with a privileged critic takes no mirror tables (none are provided for the critic's row)")
        q = copy.copy(self)
        q.symmetry = None if symmetry is None else check_tables(symmetry, self.in_dim, self.act_dim)
        return q

    @classmethod
    def from_layers(cls, actor, critic, log_std, **kw):
        """from layer lists [(W[out][in], b[out], activation)]; keywords as the constructor's"""
        return cls(actor, critic, log_std, **kw)

    @classmethod
    def from_torch(cls, actor_seq, critic_seq, log_std, obs_mean=None, obs_var=None, eps=1e-8, clip=10.0, symmetry=None,
                   critic_obs_mean=None, critic_obs_var=None):
        """from two torch.nn.Sequential of Linear / ReLU / Tanh / Softsign (controller.BaseController.from_torch's grammar), the log_std
        parameter and, optionally, the running observation statistics (tensors or arrays); `symmetry`: the tables a
        symmetry.SymmetricGaussian over the same modules was built with"""
        import torch
        actor, critic = layers_from_sequential(actor_seq, "actor"), layers_from_sequential(critic_seq, "critic")
        arr = lambda x: None if x is None else (x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x))
        return cls(actor, critic, arr(log_std), obs_mean=arr(obs_mean), obs_var=arr(obs_var), eps=eps, clip=clip, symmetry=symmetry,
                   critic_obs_mean=arr(critic_obs_mean), critic_obs_var=arr(critic_obs_var))

    @classmethod
    def from_npz(cls, path, clip=10.0, eps=1e-8):
        """tools/ppo_demo.py's <out>_policy.npz: `pi_<2i>_weight` / `pi_<2i>_bias` (tanh between the layers), `log_std`, `obs_mean`, `obs_var`
        and, when the file has them, the critic's `vf_*`; a file without a critic gets a zero critic (one layer of zeros: value 0)."""
        with np.load(path, allow_pickle=False) as z:
            def net(prefix):
                idx = sorted(int(k.split("_")[1]) for k in z.files if k.startswith(prefix + "_") and k.endswith("_weight"))
                return [(z[f"{prefix}_{i}_weight"], z[f"{prefix}_{i}_bias"], "identity" if i == idx[-1] else "tanh") for i in idx]
            actor = net("pi")
            has_vf = any(k.startswith("vf_") for k in z.files)
            critic = net("vf") if has_vf else [(np.zeros((1, actor[0][0].shape[1]), np.float32), np.zeros(1, np.float32), "identity")]
            mean = z["obs_mean"] if "obs_mean" in z.files else None
            cmean = z["critic_obs_mean"] if "critic_obs_mean" in z.files else None     # save() of an asymmetric policy
            return cls(actor, critic, z["log_std"], obs_mean=mean, obs_var=z["obs_var"] if mean is not None else None, eps=eps, clip=clip,
                       critic_obs_mean=cmean, critic_obs_var=z["critic_obs_var"] if cmean is not None else None)

    def save(self, path, eps=1e-8):
        """write from_npz's file: `pi_<2i>_*` / `vf_<2i>_*`, `log_std` and, with normalisation, `obs_mean` / `obs_var` (and the critic's
        `critic_obs_mean` / `critic_obs_var`); the variances are 1 / inv_std^2 - eps in float32, so inv_std survives the trip to an ulp.
        The file names tanh between the layers: a policy with other activations is a ValueError."""
        d = {"log_std": self.log_std}
        for prefix, net in (("pi", self.actor), ("vf", self.critic)):
            for i, (w, b, act) in enumerate(net):
                if act != ("identity" if i + 1 == len(net) else "tanh"):
                    raise ValueError("save() writes tanh nets with an identity head")
                d[f"{prefix}_{2 * i}_weight"], d[f"{prefix}_{2 * i}_bias"] = w, b
        var = lambda inv: (np.float32(1) / (inv * inv) - np.float32(eps)).astype(np.float32)
        if self.obs_mean is not None:
            d["obs_mean"], d["obs_var"] = self.obs_mean, var(self.inv_std)
        if self.critic_obs_mean is not None:
            d["critic_obs_mean"], d["critic_obs_var"] = self.critic_obs_mean, var(self.critic_inv_std)
        np.savez(path, **d)

    # ---- the callable of the single-env gym classes ----
    def normalise(self, obs):
        x = np.asarray(obs, dtype=np.float32)
        if x.shape[-1] < self.in_dim:
            raise ValueError(f"the policy's input has {self.in_dim} entries")
        return self._normalised(x[..., :self.in_dim])

    def _normalised(self, x):
        if self.obs_mean is not None:
            x = np.clip((x - self.obs_mean) * self.inv_std, np.float32(-self.clip), np.float32(self.clip))
        return x

    def normalise_critic(self, critic_obs):
        x = np.asarray(critic_obs, dtype=np.float32)
        if x.shape[-1] < self.critic_in_dim:
            raise ValueError(f"the critic's input has {self.critic_in_dim} entries")
        x = x[..., :self.critic_in_dim]
        if self.critic_obs_mean is not None:
            x = np.clip((x - self.critic_obs_mean) * self.critic_inv_std, np.float32(-self.clip), np.float32(self.clip))
        return x

    def __call__(self, obs, eps=None, critic_obs=None):
        """-> (action, logp, value, mean), float32; eps None: the deterministic action (the mean).  With a symmetry: the symmetric mean and
        value, the sample and its log-probability under the symmetrised log_std (csrc/mocca_policy.h: Symmetry).  An asymmetric policy
        takes the critic's rows as `critic_obs` [..., >= critic_in_dim]"""
        x = self.normalise(obs)
        if self.asymmetric:
            if critic_obs is None:
                raise ValueError("the policy's critic reads rows of its own: pass critic_obs")
            mean, value = _apply(self.actor, x), _apply(self.critic, self.normalise_critic(critic_obs))[..., 0]
            e = np.zeros_like(mean) if eps is None else np.asarray(eps, np.float32)
            action = mean if eps is None else mean + np.exp(self.log_std) * e
            logp = (np.float32(-0.5) * e * e - self.log_std - np.float32(HALF_LOG_2PI)).sum(-1, dtype=np.float32)
            return action, logp, value, mean
        if critic_obs is not None:
            raise ValueError("a plain policy's critic reads obs: critic_obs is an asymmetric policy's")
        if self.symmetry is not None:
            # the row as given and its mirror image (formed from the RAW row) go through the nets as two arrays of ONE memory layout: the same
            # row then gives the same bits on either side, and policy(M_o x) == (M_a mean, value) holds numerically
            in_perm, in_sign, act_perm, act_sign = self.symmetry
            raw = np.asarray(obs, dtype=np.float32)[..., :self.in_dim]
            x, xm = np.ascontiguousarray(x), np.ascontiguousarray(self._normalised(raw[..., in_perm] * in_sign))
        mean, value, log_std = _apply(self.actor, x), _apply(self.critic, x)[..., 0], self.log_std
        if self.symmetry is not None:
            half = np.float32(0.5)
            mean = half * (mean + _apply(self.actor, xm)[..., act_perm] * act_sign)
            value = half * (value + _apply(self.critic, xm)[..., 0])
            log_std = half * (log_std + log_std[act_perm])
        e = np.zeros_like(mean) if eps is None else np.asarray(eps, np.float32)
        action = mean if eps is None else mean + np.exp(log_std) * e
        logp = (np.float32(-0.5) * e * e - log_std - np.float32(HALF_LOG_2PI)).sum(-1, dtype=np.float32)
        return action, logp, value, mean

    # ---- what the library takes (include/mocca.h mocca_set_policy / mocca_update_policy) ----
    def table(self):
        """int32 [layers][8], the actor first: net, in, out, in_pad, out_pad, activation id, 0, 0"""
        return layer_table(self.actor, self.critic)

    def flat_params(self):
        """float32 [n]: per layer W[out][in] row-major then b[out], then log_std, then (with normalisation) mean and inv_std and, for an
        asymmetric policy, critic_mean and critic_inv_std"""
        parts = [p.reshape(-1) for net in (self.actor, self.critic) for w, b, _ in net for p in (w, b)] + [self.log_std]
        if self.obs_mean is not None:
            parts += [self.obs_mean, self.inv_std]
        if self.critic_obs_mean is not None:
            parts += [self.critic_obs_mean, self.critic_inv_std]
        return np.concatenate(parts).astype(np.float32)

    def n_tail(self):
        """floats of the statistics tail of flat_params() when it carries one: 2 in_dim, asymmetric: + 2 critic_in_dim"""
        return 2 * self.in_dim + (2 * self.critic_in_dim if self.asymmetric else 0)

    def n_head(self):
        """floats of flat_params() ahead of the statistics tail: the layers and log_std -- the length of ppo_grad's gradient"""
        return sum(w.size + b.size for net in (self.actor, self.critic) for w, b, _ in net) + self.act_dim

    def split_grad(self, flat):
        """views into a flat array or tensor of n_head() entries in flat_params()' order (ppo_grad's gradient, or the parameters themselves)
        -> {"actor": [(W[out][in], b[out])], "critic": [...], "log_std": [act_dim]}"""
        if flat.ndim != 1 or flat.shape[0] < self.n_head():
            raise ValueError(f"expected a flat array of at least {self.n_head()} entries")
        out, pos = {}, 0
        for name, net in (("actor", self.actor), ("critic", self.critic)):
            out[name] = []
            for w, b, _ in net:
                out[name].append((flat[pos:pos + w.size].reshape(w.shape), flat[pos + w.size:pos + w.size + b.size]))
                pos += w.size + b.size
        out["log_std"] = flat[pos:pos + self.act_dim]
        return out

    # ---- the image the policy kernel reads (csrc/mocca_policy.h); the library's repack kernel builds the same one from flat_params() ----
    def pack(self):
        """-> (image float32 [n], table int32 [layers][8] with the weight / bias offsets, offsets dict): per layer the controller's fragment
        order (controller.BaseController.pack), then log_std [32], flags [4] (flags[0] = 1: normalise), mean and inv_std [in_pad]"""
        params, table = pack_nets(self.actor, self.critic)
        pos, in_pad = params.size, _round16(self.in_dim)
        tail = np.zeros(MAX_ACTION + FLAG_WORDS + 2 * in_pad, np.float32)
        tail[:self.act_dim] = self.log_std
        if self.obs_mean is not None:
            tail[MAX_ACTION] = 1.0
            tail[MAX_ACTION + FLAG_WORDS:][:self.in_dim] = self.obs_mean
            tail[MAX_ACTION + FLAG_WORDS + in_pad:][:self.in_dim] = self.inv_std
        offsets = {"log_std": pos, "flags": pos + MAX_ACTION, "mean": pos + MAX_ACTION + FLAG_WORDS, "inv_std": pos + MAX_ACTION + FLAG_WORDS + in_pad,
                   "in_dim": self.in_dim, "act_dim": self.act_dim, "clip": self.clip}
        if not self.asymmetric:
            return np.concatenate([params, tail]), table, offsets
        c_pad = _round16(self.critic_in_dim)          # a privileged critic: critic_mean and critic_inv_std [critic_in_pad] behind inv_std
        ctail = np.zeros(2 * c_pad, np.float32)
        if self.critic_obs_mean is not None:
            ctail[:self.critic_in_dim] = self.critic_obs_mean
            ctail[c_pad:c_pad + self.critic_in_dim] = self.critic_inv_std
        offsets.update(critic_mean=pos + tail.size, critic_inv_std=pos + tail.size + c_pad, critic_in_dim=self.critic_in_dim)
        return np.concatenate([params, tail, ctail]), table, offsets

    @classmethod
    def unpack(cls, image, table, offsets):
        """decode pack()'s image back into a policy; non-zero padding is a ValueError"""
        image = np.asarray(image, np.float32)
        nets = unpack_nets(image, table, "policy")
        in_dim, act_dim, in_pad = offsets["in_dim"], offsets["act_dim"], _round16(offsets["in_dim"])
        log_std = image[offsets["log_std"]:offsets["log_std"] + MAX_ACTION]
        mean, inv_std = image[offsets["mean"]:offsets["mean"] + in_pad], image[offsets["inv_std"]:offsets["inv_std"] + in_pad]
        norm = image[offsets["flags"]] != 0
        if log_std[act_dim:].any() or mean[in_dim:].any() or inv_std[in_dim:].any() or image[offsets["flags"] + 1:offsets["flags"] + FLAG_WORDS].any() \
                or (not norm and (mean.any() or inv_std.any())):
            raise ValueError("padding of a packed policy must be zeros")
        kw = {}
        if "critic_in_dim" in offsets:
            c_dim, c_pad = offsets["critic_in_dim"], _round16(offsets["critic_in_dim"])
            cm, ci = image[offsets["critic_mean"]:offsets["critic_mean"] + c_pad], image[offsets["critic_inv_std"]:offsets["critic_inv_std"] + c_pad]
            if cm[c_dim:].any() or ci[c_dim:].any() or (not norm and (cm.any() or ci.any())):
                raise ValueError("padding of a packed policy must be zeros")
            if norm:
                kw = dict(critic_obs_mean=cm[:c_dim], critic_inv_std=ci[:c_dim])
        return cls(nets[0], nets[1], log_std[:act_dim], obs_mean=mean[:in_dim] if norm else None, inv_std=inv_std[:in_dim] if norm else None,
                   clip=offsets["clip"], **kw)
