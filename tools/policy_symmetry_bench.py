"""Launch time of mocca_act, plain and mirror-symmetric (csrc/mocca_policy.h: Symmetry): 4096 envs of Walker3DCustomEnv-v0, the "ppo" shape
(52 -> 256 -> 256 -> 21, critic alike), normalisation on, noise drawn in the kernel.  Per repeat: 20 warm launches, then 200 launches between
two device events; the figure is the median of the repeats, the spread their minimum and maximum.  One JSON line.

    python tools/policy_symmetry_bench.py [--envs 4096] [--launches 200] [--warmup 20] [--repeats 5] [--label NAME]

MOCCA_LIB_PATH selects another build of the library (the parent commit's, for the A/B); one without mocca_set_policy_symmetry is
measured in plain mode only."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--label", default="this")
    a = ap.parse_args()
    import torch
    from mocca_envs_amd import lib as L
    has_sym = hasattr(C.CDLL(L.LIB_PATH), "mocca_set_policy_symmetry")
    if not has_sym:
        L.SYMBOLS.pop("mocca_set_policy_symmetry")
    import policy_reference as R
    from mocca_envs_amd.policy import DevicePolicy
    from mocca_envs_amd.vec_env import VecEnv
    env = VecEnv("Walker3DCustomEnv-v0", a.envs, device=0, seed=1)
    p = R.random_policy("ppo", 52, 21, norm=True, seed=0)
    dp = DevicePolicy(p.actor, p.critic, p.log_std, obs_mean=p.obs_mean, inv_std=p.inv_std, clip=p.clip)
    obs = env.reset().clone()
    out = {"action": torch.empty(a.envs, 21, device="cuda"), "logp": torch.empty(a.envs, device="cuda"), "value": torch.empty(a.envs, device="cuda")}

    def measure():
        times = []
        for _ in range(a.repeats):
            for _ in range(a.warmup):
                env.act(obs, out=out)
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(a.launches):
                env.act(obs, out=out)
            t1.record()
            torch.cuda.synchronize()
            times.append(t0.elapsed_time(t1) * 1e3 / a.launches)
        return {"median_us": float(np.median(times)), "min_us": float(min(times)), "max_us": float(max(times)), "repeats_us": [round(t, 3) for t in times]}

    res = {"label": a.label, "envs": a.envs, "launches": a.launches, "warmup": a.warmup, "repeats": a.repeats, "device": torch.cuda.get_device_name(0)}
    env.set_policy(dp)
    res["plain"] = measure()
    if has_sym:
        env.set_policy(env.symmetric_policy(dp))
        res["symmetric"] = measure()
        env.set_policy(dp)
        res["plain_again"] = measure()
    env.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
