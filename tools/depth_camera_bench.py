"""What the egocentric depth camera costs next to the step kernel, and next to the only way to get its images without it, measured on
the GPU: HIP events, warm-up, one process.

    python tools/depth_camera_bench.py [--envs 4096] [--steps 200] [--rounds 5] [--out profiles/depth_camera.json]

Per env id (Walker3DCustomEnv-v0: the ground plane; Walker3DStepperEnv-v0: planks; Walker3DPlannerEnv-v0: the height-field march, the
divergent case) and with / without see_robot, at 16 x 12 pixels, after a pre-roll of random-action steps:
  step_us         time per step of `step` alone
  camera_us       the camera's launch on its own (fused form, row [obs | depth]), enqueued back to back from Python: for a launch of a
                  few microseconds this is bounded by the host's launch rate, not by the kernel -- read fused_overhead_us instead
  fused_overhead_us  step_camera_us - step_us: what a step pays for the camera
  step_camera_us  time per step of `step` + the camera's launch
  render_path_us  the same images without the sensor: link_frames(), the camera records built from them with torch operations, then
                  render(all envs, records, 16, 12, depth=True) -- mocca_render waits for the stream and launches three kernels
Each figure is the median over `rounds` windows of `steps` calls (the render path: steps / 10), the kinds of window alternating inside a
round so that drift hits them alike; min and max of the windows are kept.  There is no threshold: the figures and their ratios are reported.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WIDTH, HEIGHT = 16, 12


def _window(fn, steps, torch):
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record()
    for t in range(steps):
        fn(t)
    ev1.record()
    ev1.synchronize()
    return ev0.elapsed_time(ev1) * 1e3 / steps      # microseconds per call


def _stats(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


def measure(env_id, see_robot, envs, steps, rounds, preroll):
    import numpy as np
    import torch
    from mocca_envs_amd.perception import DepthCamera
    from mocca_envs_amd.vec_env import VecEnv
    env = VecEnv(env_id, envs, device=0, auto_reset=True, seed=1)
    env.reset()
    cam = DepthCamera(offset=(0.15, 0.0, 0.10), pitch=-35.0, fov_y=90.0, near=0.05, far=6.0, width=WIDTH, height=HEIGHT, see_robot=see_robot)
    env.set_depth_camera(cam)
    p = cam.pack()
    g = torch.Generator(device="cuda").manual_seed(0)
    acts = torch.rand(steps, envs, env.act_dim, device="cuda", generator=g) * 2 - 1
    wide = torch.zeros(envs, env.obs_dim + WIDTH * HEIGHT, device="cuda")
    ids = torch.arange(envs, dtype=torch.int32, device="cuda")
    off = torch.tensor(p["mount"][:3], device="cuda")
    pitch = float(p["mount"][4])
    fwd = torch.tensor([np.cos(pitch), 0.0, -np.sin(pitch)], dtype=torch.float32, device="cuda")
    up = torch.tensor([np.sin(pitch), 0.0, np.cos(pitch)], dtype=torch.float32, device="cuda")
    tail = torch.tensor([np.tan(0.5 * p["fov_y"]), WIDTH / HEIGHT, p["near"], p["far"]], dtype=torch.float32, device="cuda").repeat(envs, 1)

    def render_path(t):      # what a user of the parent commit would write
        fr = env.link_frames()[:, 0]
        R, org = fr[:, 0:9].reshape(envs, 3, 3), fr[:, 9:12]
        f, u = R @ fwd, R @ up
        rec = torch.cat([org + R @ off, torch.cross(f, u, dim=1), u, f, tail], dim=1).contiguous()
        return env.render(ids, rec, WIDTH, HEIGHT, depth=True)

    step = lambda t: env.step(acts[t % steps])
    both = lambda t: env.depth_camera(out=wide, obs=env.step(acts[t % steps])[0])
    camera = lambda t: env.depth_camera(out=wide, obs=env.obs)
    for t in range(preroll):          # warm-up of every launch the windows use; the batch reaches its steady mix of episode phases
        both(t)
    render_path(0)
    torch.cuda.synchronize()
    out = {"step_us": [], "step_camera_us": [], "camera_us": [], "render_path_us": []}
    for _ in range(rounds):
        out["step_us"].append(_window(step, steps, torch))
        out["step_camera_us"].append(_window(both, steps, torch))
        out["camera_us"].append(_window(camera, steps, torch))
        out["render_path_us"].append(_window(render_path, max(1, steps // 10), torch))
    env.close()
    res = {"env_id": env_id, "envs": envs, "width": WIDTH, "height": HEIGHT, "see_robot": see_robot, "steps_per_window": steps, "rounds": rounds}
    res.update({k: _stats(v) for k, v in out.items()})
    res["camera_share_of_step"] = res["camera_us"]["median"] / res["step_us"]["median"]
    res["fused_overhead_share"] = res["step_camera_us"]["median"] / res["step_us"]["median"] - 1.0
    res["fused_overhead_us"] = res["step_camera_us"]["median"] - res["step_us"]["median"]      # what a step pays for the camera
    res["render_path_over_camera"] = res["render_path_us"]["median"] / res["camera_us"]["median"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--preroll", type=int, default=300)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "depth_camera.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("depth_camera_bench needs a GPU: there is nothing to measure without one")
    cases = []
    for env_id in ("Walker3DCustomEnv-v0", "Walker3DStepperEnv-v0", "Walker3DPlannerEnv-v0"):
        for see_robot in (False, True):
            cases.append(measure(env_id, see_robot, args.envs, args.steps, args.rounds, args.preroll))
            print(json.dumps(cases[-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "cases": cases}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
