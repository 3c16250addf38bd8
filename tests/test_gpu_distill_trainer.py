"""Teacher-student distillation on the trainer surface: `make_vec_envs(privileged_scan=...)` keeps the row [obs | scan] beside the
observation row, `attach_teacher` / `teacher_targets` label the states the student visits inside the collection graph, and
tools/ppo_demo.py --distill-from runs."""
import importlib.util
import json
import os

import numpy as np
import pytest

import policy_reference as PR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV_ID, N, T = "Walker3DStepperEnv-v0", 8, 12


def _sensors():
    from mocca_envs_amd.perception import DepthCamera, scan_grid
    cam = DepthCamera(offset=(0.15, 0.0, 0.10), pitch=-35.0, fov_y=90.0, near=0.05, far=6.0, width=4, height=3)
    return cam, dict(points=scan_grid((0.0, 2.0), (-0.5, 0.5), 3, 2), z_above=1.0, max_drop=2.0)


def _dp(p):
    from mocca_envs_amd.policy import DevicePolicy
    return DevicePolicy(p.actor, p.critic, p.log_std, obs_mean=p.obs_mean, inv_std=p.inv_std, clip=p.clip)


def test_privileged_row_is_the_scan_twins_and_the_observation_row_the_camera_twins():
    """under a fixed action tape with auto-reset: `envs.privileged` of an env built with depth_camera= and privileged_scan= equals, bit for
    bit, the rows of a twin built with height_scan= alone, and its observation rows those of a twin built with depth_camera= alone --
    after the reset and after every step, through step() and through step(into=...)"""
    import torch
    from mocca_envs_amd.trainer_api import make_vec_envs
    cam, scan = _sensors()
    envs = make_vec_envs(ENV_ID, 5, N, None, depth_camera=cam, privileged_scan=scan)
    scan_twin = make_vec_envs(ENV_ID, 5, N, None, height_scan=scan)
    cam_twin = make_vec_envs(ENV_ID, 5, N, None, depth_camera=cam)
    d = envs.venv.obs_dim
    assert envs.observation_space.shape == (d + 12,) and envs.privileged.shape == (N, d + 6) and scan_twin.observation_space.shape == (d + 6,)
    o, so, co = envs.reset(), scan_twin.reset(), cam_twin.reset()
    assert torch.equal(envs.privileged, so) and torch.equal(o, co)
    g = torch.Generator(device="cuda").manual_seed(8)
    tape = torch.rand(T, N, 21, device="cuda", generator=g) * 2 - 1
    tape[:, : N // 2] *= 4.0      # half of the envs are thrown about: they fall and reset
    store, resets = torch.zeros(N, d + 12, device="cuda"), 0
    for t in range(T):
        o = envs.step(tape[t], into={"obs": store} if t % 2 else None)[0]
        so, co = scan_twin.step(tape[t])[0], cam_twin.step(tape[t])[0]
        torch.cuda.synchronize()
        assert torch.equal(envs.privileged, so) and torch.equal(o, co), t
        resets += int((envs.done != 0).sum().item())
    print("env resets under the tape:", resets)
    assert resets > 0
    with pytest.raises(ValueError):
        make_vec_envs(ENV_ID, 5, N, None, height_scan=scan, privileged_scan=scan)
    with pytest.raises(NotImplementedError):
        make_vec_envs(ENV_ID, 5, N, None, privileged_scan=scan, sub_batches=2)
    for e in (envs, scan_twin, cam_twin):
        e.close()


def test_act_step_sensors_and_teacher_replay_from_one_graph():
    """act_step -> depth camera -> privileged scan -> teacher_targets, T steps captured in one graph (capture_rollout with the device
    policy; the sink labels each state): the replay equals the eager chain on a twin, bit for bit, in the rows, the actions and the
    teacher's means and values"""
    import torch
    from mocca_envs_amd.trainer_api import make_vec_envs
    cam, scan = _sensors()
    out = []
    for graphed in (True, False):
        envs = make_vec_envs(ENV_ID, 5, N, None, depth_camera=cam, privileged_scan=scan)
        d = envs.venv.obs_dim
        envs.attach_policy(_dp(PR.random_policy("small", d + 12, 21, norm=True, seed=9)))
        envs.attach_teacher(_dp(PR.random_policy("ppo", d + 6, 21, norm=True, seed=4)))
        with pytest.raises(ValueError):
            envs.attach_teacher(_dp(PR.random_policy("small", d + 12, 21, norm=True, seed=4)))      # not the privileged row's width
        rows, act = torch.zeros(T, N, d + 12, device="cuda"), torch.zeros(T, N, 21, device="cuda")
        mean, value = torch.full((T, N, 21), float("nan"), device="cuda"), torch.full((T, N, 1), float("nan"), device="cuda")
        envs.reset()
        envs.act_step()      # one eager step on both: whatever a first call sets up is not inside the capture
        envs.teacher_targets(mean[0], value[0])
        torch.cuda.synchronize()

        def sink(t, ob, rw, m, bm, a):
            rows[t].copy_(ob), act[t].copy_(a)
            envs.teacher_targets(mean[t], value[t])

        if graphed:
            graph = envs.capture_rollout(None, T, sink=sink, warmup=0)
            graph.replay()
        else:
            for t in range(T):
                ob = envs.act_step()[0]
                sink(t, ob, None, None, None, envs.last_act["action"])
        torch.cuda.synchronize()
        out.append([x.cpu().numpy() for x in (rows, act, mean, value, envs.privileged)])
        envs.close()
    for a, b in zip(*out):
        assert np.isfinite(a).all() and a.tobytes() == b.tobytes()
    m64, v64 = PR.forward64(PR.random_policy("ppo", out[0][4].shape[1], 21, norm=True, seed=4), out[0][4])
    assert np.abs(out[0][2][-1] - m64).max() < 1e-4 and np.abs(out[0][3][-1][:, 0] - v64).max() < 1e-4      # the labels are of the LAST state


def test_ppo_demo_distils_a_teacher(tmp_path):
    """tools/ppo_demo.py, imported and driven: one iteration of a --height-scan teacher, then two of a --depth-camera student distilled
    from its policy file, 64 envs x 8 steps: it runs and logs a finite L_d"""
    spec = importlib.util.spec_from_file_location("ppo_demo", os.path.join(ROOT, "tools", "ppo_demo.py"))
    demo = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(demo)
    common = ["--env-id", ENV_ID, "--envs", "64", "--steps", "8", "--device-policy", "--device-returns", "--device-grad", "--device-update"]
    teacher = str(tmp_path / "teacher")
    demo.main(common + ["--iters", "1", "--height-scan", "3,2", "--out", teacher])
    student = str(tmp_path / "student")
    demo.main(common + ["--iters", "2", "--depth-camera", "4,3", "--privileged-scan", "3,2", "--distill-from", teacher + "_policy.npz",
                        "--out", student])
    lines = [json.loads(x) for x in open(student + ".jsonl")]
    assert lines and all(np.isfinite(x["L_d"]) and x["L_d"] > 0 for x in lines)
    assert os.path.exists(student + "_policy.npz")
