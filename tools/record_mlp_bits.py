"""Record what the three MFMA MLP kernels compute, bit for bit: one SHA-256 per case over the raw output bytes of act() (policy_kernel, plain
and mirror-symmetric), of plan_step()'s base outputs (controller_kernel) and of ppo_grad() in its four modes (ppo_rows_kernel and the three
launches behind it).  tests/test_gpu_mlp_bits.py recomputes the hashes with the library under test and compares them with the file this tool
wrote from the library of the commit BEFORE a bit-exact change of the layer loop (csrc/mocca_mlp.h):

    python tools/record_mlp_bits.py                 # every case -> tests/golden/mlp_bits.json  (needs the GPU)

MOCCA_LIB_PATH selects the library, as everywhere.  Every input comes from numpy.random.default_rng seeds (tests/policy_reference.py,
tests/controller_reference.py, tests/policy_symmetry_reference.py); torch only carries the bytes to the device and back.

The shapes are the smallest at which the layer loop can still go wrong.  Nets: policy_reference.SHAPES at (52, 21) -- "small": 1 and 2 output
tiles, so waves 1 .. 3 return early; "ppo": 16 tiles, four per wave; "deep8": 4, 2, 1, 8, 3, 16, 5 k-groups, all three exits of the trip of
three -- and "small" at (142, 21) read from rows wider than in_dim.  Batches: one column, a tile and one, four tiles less one."""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import controller_reference as CR  # noqa: E402
import policy_reference as PR  # noqa: E402
import policy_symmetry_reference as PSR  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "mlp_bits.json")
#        (kind, in_dim, act_dim, floats of an input row)
NETS = (("small", 52, 21, 52), ("ppo", 52, 21, 52), ("deep8", 52, 21, 52), ("small", 142, 21, 155))
ACT_N = {"plain": (1, 17, 63), "sym": (1, 9, 63)}      # sym: one env; a tile of 8 and one; four tiles less one
PLAN_N = (1, 17, 63)
PPO_ROWS, PPO_STORAGE = (1, 17, 63), 96
PPO_MODES = ("plain", "sym", "mirror", "dup")
MIRROR_COEF = 0.5
KW = dict(clip=0.2, value_coef=0.5, entropy_coef=0.01)


def _tag(net):
    return f"{net[0]}-{net[1]}" + ("-strided" if net[3] > net[1] else "")


def _policy(net):
    from mocca_envs_amd.policy import DevicePolicy
    p = PR.random_policy(net[0], net[1], net[2], norm=True, seed=1)
    return p, DevicePolicy(p.actor, p.critic, p.log_std, obs_mean=p.obs_mean, inv_std=p.inv_std, clip=p.clip)


def _tables(net):
    return PSR.random_tables(net[1], 11, net[2])


def _rows(x, width):
    """x [n][d] on the device as a view of rows `width` floats wide whose other floats are NaN"""
    import torch
    wide = torch.full((x.shape[0], width), float("nan"), device="cuda")
    wide[:, :x.shape[1]] = torch.from_numpy(x).cuda()
    return wide[:, :x.shape[1]]


def _digest(*tensors):
    import torch
    torch.cuda.synchronize()
    h = hashlib.sha256()
    for t in tensors:
        h.update(np.ascontiguousarray(t.cpu().numpy()).tobytes())
    return h.hexdigest()


def record_act():
    """act(): normalisation on, the mean (deterministic) and the sample under the caller's eps -> action, logp, value, mean"""
    import torch
    from mocca_envs_amd.vec_env import VecEnv
    out = {}
    for n in sorted(set(ACT_N["plain"] + ACT_N["sym"])):
        env = VecEnv("Walker3DCustomEnv-v0", n, seed=3)
        for net in NETS:
            _, dp = _policy(net)
            obs = _rows(PR.plausible_inputs(n, net[1], seed=n), net[3])
            eps = torch.from_numpy(np.random.default_rng([n, 5]).normal(0, 1, (n, net[2])).astype(np.float32)).cuda()
            for form in ("plain", "sym"):
                if n not in ACT_N[form]:
                    continue
                env.set_policy(dp.with_symmetry(_tables(net)) if form == "sym" else dp)
                for how, kw in (("mean", dict(deterministic=True)), ("eps", dict(eps=eps))):
                    mean = torch.full((n, net[2]), float("nan"), device="cuda")
                    o = env.act(obs, out={"mean": mean}, **kw)
                    out[f"act/{_tag(net)}/{form}/n{n}/{how}"] = _digest(o["action"], o["logp"], o["value"], o["mean"])
        env.close()
    return out


def record_plan_step():
    """plan_step()'s base outputs on the second step after a reset, the controller on the raw input and with observation statistics"""
    import torch
    from mocca_envs_amd.vec_env import VecEnv
    out = {}
    for n in PLAN_N:
        env = VecEnv("MikePlannerEnv-v0", n, seed=5)
        plans = np.random.default_rng([n, 1]).normal(0, 1, (2, n, 15)).astype(np.float32)
        for kind in sorted(CR.SHAPES):
            for norm in (False, True):
                env.set_base_controller(CR.random_controller(kind, seed=7))      # (drops the statistics of the one before)
                if norm:
                    rng = np.random.default_rng([n, 9])
                    env.set_base_controller_norm(rng.normal(0, 0.5, 65).astype(np.float32), rng.uniform(0.5, 2.0, 65).astype(np.float32), clip=5.0)
                env.reset()
                for t in range(2):
                    env.plan_step(torch.from_numpy(plans[t]).cuda())
                out[f"plan_step/{kind}/n{n}/{'norm' if norm else 'raw'}"] = _digest(*env.base_outputs())
        env.close()
    return out


def storage(p, net):
    """PPO_STORAGE rollout rows for policy p: actions sampled from it, old_logp and old_value near its own so that the ratio and the value
    clip land on both sides of their bounds"""
    rng = np.random.default_rng([net[1], 13])
    obs = PR.plausible_inputs(PPO_STORAGE, net[1], seed=3)
    mean, value = PR.forward64(p, obs)
    action, logp = PR.sample64(mean, p.log_std, rng.normal(0, 1, mean.shape))
    f = lambda x: np.ascontiguousarray(x, np.float32)
    return dict(obs=obs, action=f(action), old_logp=f(logp + rng.normal(0, 0.15, PPO_STORAGE)), adv=f(rng.normal(0, 1, PPO_STORAGE)),
                returns=f(value + rng.normal(0, 0.5, PPO_STORAGE)), old_value=f(value + rng.normal(0, 0.3, PPO_STORAGE)))


def attach(env, mode, tables):
    """the policy's mirror attachment for ppo_grad's `mode` (None tables: detach it)"""
    if mode == "sym":
        env.set_policy_symmetry(tables)
    elif mode == "mirror":
        env.set_policy_mirror_loss(tables, MIRROR_COEF)
    elif mode == "dup":
        env.set_policy_mirror_dup(tables)


def record_ppo_grad():
    """ppo_grad() in the four modes: the rows gathered through a shuffled idx, value_clip off and on -> grad and the 8 stats"""
    import torch
    from mocca_envs_amd.vec_env import VecEnv
    out = {}
    env = VecEnv("Walker3DCustomEnv-v0", 4, seed=3)
    for net in NETS:
        p, dp = _policy(net)
        st = storage(p, net)
        d = {k: torch.from_numpy(v).cuda() for k, v in st.items()}
        d["obs"] = _rows(st["obs"], net[3])
        env.set_policy(dp)
        for mode in PPO_MODES:
            attach(env, mode, _tables(net))
            for b in PPO_ROWS:
                idx = torch.from_numpy(np.random.default_rng([b, 17]).permutation(PPO_STORAGE)[:b].astype(np.int64)).cuda()
                for value_clip in (False, True):
                    o = env.ppo_grad(d["obs"], d["action"], d["old_logp"], d["adv"], d["returns"], idx=idx, old_value=d["old_value"] if value_clip else None,
                                     value_clip=value_clip, **KW)
                    out[f"ppo_grad/{_tag(net)}/{mode}/b{b}/{'vclip' if value_clip else 'noclip'}"] = _digest(o["grad"], o["stats"])
            attach(env, mode, None)
    env.close()
    return out


GROUPS = {"act": record_act, "plan_step": record_plan_step, "ppo_grad": record_ppo_grad}


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=GOLDEN, help="the JSON file (default: tests/golden/mlp_bits.json)")
    args = ap.parse_args()
    doc = {}
    for group, fn in GROUPS.items():
        doc.update(fn())
        print(group, sum(k.startswith(group + "/") for k in doc), "cases")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
