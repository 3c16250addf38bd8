"""Roll M envs for K steps and write what they look like: the stand-in for the reference trainers' `enjoy` scripts.

    python tools/render_rollout.py --env Walker3DCustomEnv-v0 --envs 4 --steps 60 --out frames/ [--policy actor.pt] [--width 320 --height 240]

Actions come from a saved torch module (`--policy`, called on the observation batch) or are uniform random.  Frames go to
<out>/frames.npy (uint8 [K][M][H][W][3]) and, if an image writer can be imported here (imageio, PIL or matplotlib), to PNG files.
`--time` instead times the render launch with device events and prints one JSON line (profiles/render_bench.json).
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mocca_envs_amd.vec_env import VecEnv  # noqa: E402


def png_writer():
    try:
        import imageio.v2 as iio
        return lambda path, img: iio.imwrite(path, img)
    except ImportError:
        pass
    try:
        from PIL import Image
        return lambda path, img: Image.fromarray(img).save(path)
    except ImportError:
        pass
    try:
        import matplotlib.image as mpi
        return lambda path, img: mpi.imsave(path, img)
    except ImportError:
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--env", default="Walker3DCustomEnv-v0")
    ap.add_argument("--envs", type=int, default=4)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--views", type=int, default=None, help="envs rendered per frame (default: all)")
    ap.add_argument("--width", type=int, default=320)
    ap.add_argument("--height", type=int, default=240)
    ap.add_argument("--policy", default=None)
    ap.add_argument("--out", default="render_out")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--time", type=int, default=0, help="time this many render launches (and link_frames launches) instead of writing frames")
    a = ap.parse_args()
    env = VecEnv(a.env, a.envs, device=0, seed=a.seed)
    obs = env.reset()
    policy = torch.load(a.policy, map_location=env.device, weights_only=False) if a.policy else None
    g = torch.Generator(device=env.device).manual_seed(a.seed)
    views = list(range(a.views or a.envs))

    def act(o):
        if policy is not None:
            with torch.no_grad():
                return policy(o).clamp(-1, 1)
        return torch.rand(a.envs, env.act_dim, generator=g, device=env.device) * 2 - 1

    if a.time:
        for _ in range(10):
            obs = env.step(act(obs))[0]
        out = {}
        for what, fn in (("render", lambda: env.render(views, None, a.width, a.height)), ("link_frames", env.link_frames)):
            for _ in range(3):
                fn()
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(a.time + 1)]
            ev[0].record()
            for k in range(a.time):
                fn()
                ev[k + 1].record()
            torch.cuda.synchronize()
            ms = np.array([ev[k].elapsed_time(ev[k + 1]) for k in range(a.time)])
            out[what + "_call_us_median"], out[what + "_call_us_min"] = round(float(np.median(ms)) * 1e3, 1), round(float(ms.min()) * 1e3, 1)
        print(json.dumps(dict(env=a.env, envs=a.envs, views=len(views), width=a.width, height=a.height, launches=a.time,
                              note="whole calls between device events: camera set-up, id check and the kernels", **out)))
        return
    os.makedirs(a.out, exist_ok=True)
    frames = np.zeros((a.steps, len(views), a.height, a.width, 3), np.uint8)
    for k in range(a.steps):
        obs = env.step(act(obs))[0]
        frames[k] = env.render(views, None, a.width, a.height).cpu().numpy()
    np.save(os.path.join(a.out, "frames.npy"), frames)
    write = png_writer()
    if write is not None:
        for k in range(a.steps):
            for v in range(len(views)):
                write(os.path.join(a.out, f"env{v:03d}_{k:05d}.png"), frames[k, v])
    print(json.dumps(dict(env=a.env, frames=list(frames.shape), png=write is not None, out=a.out)))


if __name__ == "__main__":
    main()
