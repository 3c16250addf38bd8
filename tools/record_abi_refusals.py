#!/usr/bin/env python
"""Record what the C ABI answers to calls it must refuse -> tests/golden/abi_refusals.json.

    MOCCA_LIB_PATH=<the library to record> python tools/record_abi_refusals.py [--out FILE]

Six handles of 2 envs (the walker, the Stepper, the planner, plain Cassie, and two blobs that only refuse: a Cassie phase env without its
trajectory and a walker with 64-row caps) each run one script of calls: the refusals, and between them the few successful calls (rc 0) that
put an attachment in place so that the checks behind it are reached.  A case is data alone -- entry, arguments, return code, message (null:
the recorded library's refusal set none) -- so tests/test_gpu_abi_refusals.py replays the file against the library it is given and compares
code and message byte for byte.

Arguments as data: numbers and null as they are; "B": a zeroed 1 MiB device buffer; {"B": k}: the same k bytes in; {"f32": [...]} /
{"i32": [...]}: a host array; {"f32n": [n, v]}: n floats v on the host; {"iota": n}: the int32 0 .. n - 1 on the host; {"dev_i32": [...]} /
{"dev_f32n": [n, v]}: a device array; {"rand": [...]}: a
mocca_randomisation.
"""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden", "abi_refusals.json")
N = 2
B = "B"
INF = float("inf")
SENTINEL = "unknown parameter id"   # mocca_set_param(h, 99, 0)
# sites no script reaches, and why
UNREACHED = [
    "HIP_TRY / commit_ready / grow_scratch / mocca_create's hipMalloc and hipMemcpy: need a HIP error",
    "out_of_host_memory (every `catch (const std::bad_alloc&)`): needs a failed host allocation",
    "mocca_set_randomisation 'n_envs x act_dim must stay below 2^31', mocca_set_sensor_noise 'n_envs x dim must stay below 2^31', "
    "mocca_set_history 'n_envs x the block width must stay below 2^31': need a 2^31-sized product",
    "mocca_gae 'normalise needs at least two advantages': n_steps x n_envs >= 2 at 2 envs",
]


def rows(*layers):
    """int32 layer table: (net, in, out, activation) per layer, pads rounded up to 16, offsets W then b, layer after layer"""
    out, pos = [], 0
    for net, n_in, n_out, act in layers:
        out += [net, n_in, n_out, (n_in + 15) // 16 * 16, (n_out + 15) // 16 * 16, act, pos, pos + n_in * n_out]
        pos += n_in * n_out + n_out
    return {"i32": out}, len(layers), pos


def nets(in_dim, act_dim, critic_in=None):
    """-> (layer table, layers, floats of a policy's flat parameters: the layers, then log_std)"""
    table, n_layers, n = rows((0, in_dim, 16, 2), (0, 16, act_dim, 0), (1, critic_in or in_dim, 16, 2), (1, 16, 1, 0))
    return table, n_layers, n + act_dim


def perm_tables(in_dim, act_dim):
    """identity mirror tables"""
    return [{"iota": in_dim}, {"f32n": [in_dim, 1.0]}, {"iota": act_dim}, {"f32n": [act_dim, 1.0]}]


def core_script(od, ad):
    """what every task refuses alike"""
    return [
        ("mocca_set_param", [99, 0.0]), ("mocca_set_param", [9, -1.0]), ("mocca_set_param", [8, 3.0]), ("mocca_set_param", [13, -100.0]),
        ("mocca_set_param", [12, -1.0]), ("mocca_set_param", [11, 3.0]), ("mocca_set_param", [11, 1.5]),
        ("mocca_set_param_v", [3, B, 0, None]), ("mocca_set_param_v", [2, None, 0, None]),
        ("mocca_reset", [None, 0, None, None]), ("mocca_step", [None, None, None, None, None, None]), ("mocca_step", [B, B, B, None, None, None]),
        ("mocca_task_step", [None, None, None, None, None, None, None, None, None]), ("mocca_observe", [None, None]),
        ("mocca_get_state", [None, None]), ("mocca_set_state", [None, None]), ("mocca_get_task", [None, None]), ("mocca_set_task", [None, None]),
        ("mocca_get_terrain", [None, None]), ("mocca_set_terrain", [None, None]), ("mocca_get_link_frames", [None, None]),
        ("mocca_set_draw_tape", [B, 0]),
        ("mocca_set_episode_stats", [None, None, None, B, 0, 64]), ("mocca_set_episode_stats", [None, None, None, {"B": 4}, 1, 64]),
        ("mocca_set_episode_stats", [None, None, None, B, 1, 16]),
        ("mocca_set_trajectory", [None, 0, 1.0, 1.0]), ("mocca_set_trajectory", [{"f32": [0.0]}, 1, 0.0, 1.0]),
        ("mocca_set_heightfield", [None, 8, 8, 1.0]),
    ]


def walker_script(od, ad):
    t, nl, base = nets(od, ad)
    bad_tables = [
        rows((0, od, ad, 0)),                                                             # one layer in all
        rows((2, od, 16, 2), (0, 16, ad, 0), (1, od, 16, 2), (1, 16, 1, 0)),              # net 2
        rows((1, od, 16, 2), (1, 16, 1, 0), (0, od, 16, 2), (0, 16, ad, 0)),              # the critic first
        rows(*([(0, od, 16, 2)] + [(0, 16, 16, 2)] * 8 + [(1, od, 1, 0)])),               # nine actor layers
        rows((0, od + 1, 16, 2), (0, 16, ad, 0), (1, od, 16, 2), (1, 16, 1, 0)),          # first layer's input
        rows((0, od, 16, 2), (0, 32, ad, 0), (1, od, 16, 2), (1, 16, 1, 0)),              # input differs from the previous output
        rows((0, od, 0, 2), (0, 0, ad, 0), (1, od, 16, 2), (1, 16, 1, 0)),                # width 0
        rows((0, od, 16, 9), (0, 16, ad, 0), (1, od, 16, 2), (1, 16, 1, 0)),              # unknown activation
        rows((0, od, 16, 2), (0, 16, ad + 1, 0), (1, od, 16, 2), (1, 16, 1, 0)),          # the actor's head
        rows((0, od, 24, 2), (0, 24, ad, 0), (1, od, 16, 2), (1, 16, 1, 0)),              # hidden width 24
        rows((0, od, 16, 2), (0, 16, ad, 0)),                                             # no critic
    ]
    pads = rows((0, od, 16, 2), (0, 16, ad, 0), (1, od, 16, 2), (1, 16, 1, 0))
    pads[0]["i32"][3] += 16                                                               # in_pad of layer 0
    pol = lambda tab, i=od, a=ad, clip=5.0: ("mocca_set_policy", [tab[0], tab[1], i, a, clip])
    grad = lambda name, **kw: (name, [kw.get("obs", B), kw.get("stride", od), B, B, B, B, kw.get("old_value", None), None, kw.get("n_rows", 2),
                                     kw.get("clip", 0.2), 0.5, 0.0, kw.get("value_clip", 0), kw.get("grad", B), None, None])
    adam = lambda **kw: ("mocca_adam_step", [kw.get("params", B), kw.get("n_floats", base), B, kw.get("n_params", base), B, B, kw.get("lr", 1e-3),
                                             kw.get("beta1", 0.9), 0.999, 1e-8, kw.get("max_norm", 0.5), None])
    upd = lambda name="mocca_ppo_update", rollout=2, mini=2, epochs=1: (name, [B, od, B, B, B, B, None, rollout, mini, epochs, 0.2, 0.5, 0.0, 0, B, base, base, B, B,
                                                                              1e-3, 0.9, 0.999, 1e-8, 0.5, 1, None, None])
    act = lambda name="mocca_act", **kw: (name, [kw.get("inp", B), kw.get("stride", od), None, 1, B, None, kw.get("value", None), None] +
                                         ([B, B, B, None] if name != "mocca_act" else []) + [None])
    upd_priv = ("mocca_ppo_update_priv", [B, od, B, od + 3, B, B, B, B, None, 2, 2, 1, 0.2, 0.5, 0.0, 0, B, base, base, B, B, 1e-3, 0.9, 0.999, 1e-8, 0.5, 1, None, None])
    mir = perm_tables(od, ad)
    mirror = lambda name, tabs=mir, coef=None: (name, list(tabs) + ([coef] if coef is not None else []))
    swapped = [{"i32": [1, 0] + list(range(2, od))}, {"f32": [1.0, -1.0] + [1.0] * (od - 2)}] + mir[2:]
    s = core_script(od, ad) + [
        ("mocca_plan_dim", []), ("mocca_task_step", [B, None, None, None, B, B, B, None, None]),
        ("mocca_set_heightfield_bank", [None, 1, 8, 8, 1.0]), ("mocca_generate_heightfields", [0, 1, 1, 4, 1.0, None]),
        ("mocca_set_env_fields", [None, 0, None]), ("mocca_get_env_fields", [None, None]), ("mocca_get_env_fields", [B, None]),
        ("mocca_get_heightfields", [0, 1, None, None]), ("mocca_get_heightfields", [0, 1, B, None]),
        ("mocca_set_base_controller", [None, 0, None, 0, 1.0]), ("mocca_get_base_outputs", [B, B, None]),
        ("mocca_set_base_controller_norm", [None, None, 5.0]), ("mocca_plan_step", [B, B, B, B, None, None]),
        ("mocca_act_plan_step", [B, od, None, 1, B, None, None, None, B, B, B, None, None]),
        # render, scan, depth
        ("mocca_render", [None, 1, None, 4, 4, None, None, None, None]), ("mocca_render", [B, 0, B, 4, 4, None, None, None, None]),
        ("mocca_render", [B, 1, B, 0, 4, None, None, None, None]), ("mocca_render", [{"dev_i32": [5]}, 1, B, 1, 1, None, B, None, None]),
        ("mocca_height_scan", [B, 8, None, None]),
        ("mocca_set_height_scan", [{"f32": [0.0, 0.0]}, 0, 1.0, 1.0]), ("mocca_set_height_scan", [{"f32": [0.0, 0.0]}, 1, -1.0, 1.0]),
        ("mocca_set_height_scan", [{"f32": [0.0, INF]}, 1, 1.0, 1.0]), ("mocca_set_height_scan", [{"f32": [0.0, 0.0, 1.0, 0.0]}, 2, 1.0, 1.0]),
        ("mocca_height_scan", [None, 8, None, None]), ("mocca_height_scan", [B, 1, None, None]), ("mocca_height_scan", [B, 2, B, None]),
        ("mocca_depth_camera", [B, 64, None, None, None]),
        ("mocca_set_depth_camera", [-1, {"f32": [0.0] * 6}, 4, 4, 1.0, 0.1, 5.0, 0]), ("mocca_set_depth_camera", [0, {"f32": [0.0] * 6}, 0, 4, 1.0, 0.1, 5.0, 0]),
        ("mocca_set_depth_camera", [0, {"f32": [0.0] * 6}, 32, 32, 1.0, 0.1, 5.0, 0]), ("mocca_set_depth_camera", [0, {"f32": [0.0] * 5 + [INF]}, 4, 4, 1.0, 0.1, 5.0, 0]),
        ("mocca_set_depth_camera", [0, {"f32": [0.0] * 6}, 4, 4, 0.0, 0.1, 5.0, 0]), ("mocca_set_depth_camera", [0, {"f32": [0.0] * 6}, 4, 4, 1.0, 0.0, 5.0, 0]),
        ("mocca_set_depth_camera", [0, {"f32": [0.0] * 6}, 4, 4, 1.0, 0.1, 5.0, 8]), ("mocca_set_depth_camera", [0, {"f32": [0.0] * 6}, 4, 4, 1.0, 1.0, 1.0 + 1e-12, 0]),
        ("mocca_set_depth_camera", [0, {"f32": [0.0] * 6}, 4, 4, 1.0, 0.1, 5.0, 0]),
        ("mocca_depth_camera", [None, 64, None, None, None]), ("mocca_depth_camera", [B, 15, None, None, None]),
        # history
        ("mocca_history_dim", []), ("mocca_history", [B, od, None, 0, B, 64, None]),
        ("mocca_set_history", [{"i32": [0]}, 1, 0, 17, 1]), ("mocca_set_history", [{"i32": [0]}, 1, 0, 1, 9]), ("mocca_set_history", [{"i32": [0]}, 1, 33, 1, 1]),
        ("mocca_set_history", [{"i32": [0]}, -1, 0, 1, 1]), ("mocca_set_history", [None, 1, 0, 1, 1]), ("mocca_set_history", [None, 0, 0, 1, 1]),
        ("mocca_set_history", [{"i32": [od]}, 1, 0, 1, 1]), ("mocca_set_history", [{"i32": [0, 0]}, 2, 0, 1, 1]),
        ("mocca_set_history", [{"i32": list(range(od))}, od, 32, 16, 1]),
        ("mocca_set_history", [{"i32": [0, 1]}, 2, 2, 2, 1]),
        ("mocca_history", [None, od, None, 0, B, 64, None]), ("mocca_history", [B, od - 1, None, 0, B, 64, None]), ("mocca_history", [B, od, None, 0, B, 7, None]),
        ("mocca_history", [B, od, B, 1, B, 64, None]),
        # randomisation and sensor noise
        ("mocca_get_effective_action", [B, None]), ("mocca_randomisation_record", [B, 4, None]),
        ("mocca_set_randomisation", [{"rand": [0.0, 1.0, 0, 0, 0, 0.0]}]), ("mocca_set_randomisation", [{"rand": [1.0, 1.0, 2, 1, 0, 0.0]}]),
        ("mocca_set_randomisation", [{"rand": [1.0, 1.0, 0, 8, 0, 0.0]}]), ("mocca_set_randomisation", [{"rand": [1.0, 1.0, 0, 0, 0, -1.0]}]),
        ("mocca_set_randomisation", [{"rand": [1.0, 1.0, 0, 0, -1, 0.0]}]), ("mocca_set_randomisation", [{"rand": [0.5, 1.0, 0, 1, 0, 0.0]}]),
        ("mocca_get_effective_action", [None, None]), ("mocca_randomisation_record", [None, 4, None]), ("mocca_randomisation_record", [B, 3, None]),
        ("mocca_sensor_noise", [B, od, B, od, None]),
        ("mocca_set_sensor_noise", [{"f32n": [od, 0.1]}, od - 1]), ("mocca_set_sensor_noise", [{"f32": [0.1] * (od - 1) + [-1.0]}, od]),
        ("mocca_set_sensor_noise", [{"f32n": [od, 0.1]}, od]),
        ("mocca_sensor_noise", [None, od, B, od, None]), ("mocca_sensor_noise", [B, od - 1, B, od, None]),
        # rollout
        ("mocca_gae", [None, B, B, B, 1, 0.99, 0.95, 1.0, B, B, 0, 1e-5, None, None]), ("mocca_gae", [B, B, B, B, 1, 0.99, 0.95, 1.0, B, None, 1, 1e-5, None, None]),
        ("mocca_gae", [B, B, B, B, 0, 0.99, 0.95, 1.0, B, B, 0, 1e-5, None, None]), ("mocca_gae", [B, B, B, B, 1, INF, 0.95, 1.0, B, B, 0, 1e-5, None, None]),
        ("mocca_gae", [B, B, B, B, 1, 0.99, 0.95, 1.0, B, B, 0, -1.0, None, None]),
        ("mocca_obs_stats", [None, 2, od, od, B, 1e-8, None, None, None]), ("mocca_obs_stats", [B, 2, od, 0, B, 1e-8, None, None, None]),
        ("mocca_obs_stats", [B, 2, od - 1, od, B, 1e-8, None, None, None]), ("mocca_obs_stats", [B, 0, od, od, B, 1e-8, None, None, None]),
        ("mocca_obs_stats", [B, 2, od, od, B, -1.0, None, None, None]),
        # policy slots: nothing attached yet
        ("mocca_update_policy", [B, base, None]), ("mocca_update_teacher", [B, base, None]), act(), ("mocca_teacher_act", [B, od, 2, B, None, None]),
        ("mocca_set_critic_rows", [B, od]), mirror("mocca_set_policy_symmetry"), mirror("mocca_set_policy_mirror_loss", coef=1.0),
        mirror("mocca_set_policy_mirror_dup"), grad("mocca_ppo_grad"), adam(), upd(),
        ("mocca_distill_grad", [B, od, B, None, None, 2, 1.0, 0.5, B, None, None]),
        pol((t, nl), i=0), pol((t, nl), i=337), pol((t, nl), a=0), pol((t, nl), clip=0.0), ("mocca_set_policy_priv", [t, nl, od, 0, ad, 5.0]),
    ] + [pol(tab) for tab in bad_tables] + [pol(pads), pol((t, nl))] + [
        ("mocca_update_policy", [None, base, None]), ("mocca_update_policy", [B, base + 1, None]), act(), grad("mocca_ppo_grad"),
        ("mocca_update_policy", [B, base, None]),
        act(inp=None), act(stride=od - 1), ("mocca_set_param", [6, float(1 << 28)]), act(), ("mocca_set_param", [6, 0.0]),
        ("mocca_act_step", [B, od, None, 1, B, None, None, None, None, B, B, None, None]),
        # the gradient, the optimiser and the loops on the plain policy
        grad("mocca_ppo_grad", obs=None), grad("mocca_ppo_grad", value_clip=1), grad("mocca_ppo_grad", n_rows=0), grad("mocca_ppo_grad", n_rows=(1 << 22) + 1),
        grad("mocca_ppo_grad", stride=od - 1), grad("mocca_ppo_grad", clip=-1.0), grad("mocca_ppo_grad_sym"), grad("mocca_ppo_grad_mirror"), grad("mocca_ppo_grad_dup"),
        ("mocca_ppo_grad_priv", [B, od, B, od, B, B, B, B, None, None, 2, 0.2, 0.5, 0.0, 0, B, None, None]),
        ("mocca_distill_grad", [None, od, B, None, None, 2, 1.0, 0.5, B, None, None]), ("mocca_distill_grad", [B, od, B, None, None, 2, -1.0, 0.5, B, None, None]),
        adam(params=None), adam(n_floats=base + 1), adam(n_params=0), adam(lr=-1.0), adam(beta1=1.0), adam(max_norm=-1.0),
        upd(rollout=0), upd(rollout=(1 << 22) + 1), upd(mini=3), upd(epochs=0), upd_priv,
        ("mocca_ppo_update", [None, od, B, B, B, B, None, 2, 2, 1, 0.2, 0.5, 0.0, 0, B, base, base, B, B, 1e-3, 0.9, 0.999, 1e-8, 0.5, 1, None, None]),
        ("mocca_ppo_update", [B, od, B, B, B, B, None, 2, 2, 1, 0.2, 0.5, 0.0, 0, None, base, base, B, B, 1e-3, 0.9, 0.999, 1e-8, 0.5, 1, None, None]),
        ("mocca_distill_update", [B, od, B, None, 2, 2, 0, 1.0, 0.5, B, base, base, B, B, 1e-3, 0.9, 0.999, 1e-8, 0.5, 1, None, None]),
        ("mocca_distill_update", [B, od, None, None, 2, 2, 1, 1.0, 0.5, B, base, base, B, B, 1e-3, 0.9, 0.999, 1e-8, 0.5, 1, None, None]),
        # mirror tables
        mirror("mocca_set_policy_symmetry", [mir[0], None, mir[2], mir[3]]), mirror("mocca_set_policy_symmetry", [{"i32": [od] + list(range(1, od))}] + mir[1:]),
        mirror("mocca_set_policy_symmetry", [mir[0], {"f32": [0.5] + [1.0] * (od - 1)}] + mir[2:]),
        mirror("mocca_set_policy_symmetry", [{"i32": [1, 2, 0] + list(range(3, od))}] + mir[1:]), mirror("mocca_set_policy_symmetry", swapped),
        mirror("mocca_set_policy_symmetry", mir[:2] + [{"i32": [ad] + list(range(1, ad))}, mir[3]]), mirror("mocca_set_policy_mirror_loss", coef=-1.0),
        mirror("mocca_set_policy_symmetry"), mirror("mocca_set_policy_mirror_loss", coef=1.0), mirror("mocca_set_policy_mirror_dup"),
        grad("mocca_ppo_grad"), grad("mocca_ppo_grad_mirror"), grad("mocca_ppo_grad_dup"), grad("mocca_ppo_grad_sym", n_rows=(1 << 21) + 1), upd(rollout=(1 << 21) + 1),
        ("mocca_distill_grad", [B, od, B, None, None, 2, 1.0, 0.5, B, None, None]), ("mocca_set_policy_priv", [t, nl, od, od, ad, 5.0]),
        mirror("mocca_set_policy_symmetry", [None, None, None, None]),
        mirror("mocca_set_policy_mirror_loss", coef=1.0), mirror("mocca_set_policy_symmetry"), mirror("mocca_set_policy_mirror_dup"), grad("mocca_ppo_grad"),
        grad("mocca_ppo_grad_sym"), ("mocca_set_policy_priv", [t, nl, od, od, ad, 5.0]), mirror("mocca_set_policy_mirror_loss", [None, None, None, None], coef=0.0),
        mirror("mocca_set_policy_mirror_dup"), mirror("mocca_set_policy_symmetry"), mirror("mocca_set_policy_mirror_loss", coef=1.0), grad("mocca_ppo_grad"),
        ("mocca_set_policy_priv", [t, nl, od, od, ad, 5.0]), mirror("mocca_set_policy_mirror_dup", [None, None, None, None]),
        # the teacher
        ("mocca_set_teacher", [t, nl, od, ad, 5.0]), ("mocca_teacher_act", [B, od, 2, B, None, None]), ("mocca_update_teacher", [None, base, None]),
        ("mocca_update_teacher", [B, base, None]), ("mocca_teacher_act", [None, od, 2, B, None, None]), ("mocca_teacher_act", [B, od - 1, 2, B, None, None]),
        ("mocca_teacher_act", [B, od, 0, B, None, None]),
    ]
    # a privileged critic
    tp, nlp, base_p = nets(od, ad, critic_in=od + 3)
    s += [
        ("mocca_set_policy_priv", [tp, nlp, od, od + 3, ad, 5.0]), ("mocca_set_critic_rows", [B, od]), mirror("mocca_set_policy_symmetry"),
        ("mocca_update_policy", [B, base_p, None]), grad("mocca_ppo_grad"), ("mocca_distill_grad", [B, od, B, None, None, 2, 1.0, 0.5, B, None, None]),
        upd(), upd_priv[:1] + ([B, od, None] + upd_priv[1][3:],), ("mocca_ppo_grad_priv", [B, od, None, od + 3, B, B, B, B, None, None, 2, 0.2, 0.5, 0.0, 0, B, None, None]),
        ("mocca_ppo_grad_priv", [B, od, B, od, B, B, B, B, None, None, 2, 0.2, 0.5, 0.0, 0, B, None, None]), act(value=B),
        # another head than the env's
        ("mocca_set_policy", list(nets(od, ad + 1)[:2]) + [od, ad + 1, 5.0]), act("mocca_act_step"),
    ]
    return s


def planner_script(od, ad):
    ci = 65
    t, nl, n = rows((0, ci, 16, 2), (0, 16, 21, 0), (1, ci, 16, 2), (1, 16, 1, 0))
    ctrl = lambda tab, n_floats=n, scale=2.0: ("mocca_set_base_controller", [{"f32n": [max(n_floats, 1), 0.01]}, n_floats, tab[0], tab[1], scale])
    outside = rows((0, ci, 16, 2), (0, 16, 21, 0), (1, ci, 16, 2), (1, 16, 1, 0))
    outside[0]["i32"][6] = n                                                              # layer 0's weights behind the array
    tp, nlp, base = nets(od, 15)
    return core_script(od, ad) + [
        ("mocca_reset", [None, 0, B, None]), ("mocca_render", [B, 1, B, 4, 4, None, B, None, None]),
        ("mocca_set_height_scan", [{"f32": [0.0, 0.0]}, 1, 1.0, 1.0]), ("mocca_height_scan", [B, 1, None, None]),
        ("mocca_set_depth_camera", [0, {"f32": [0.0] * 6}, 4, 4, 1.0, 0.1, 5.0, 0]), ("mocca_depth_camera", [B, 16, None, None, None]),
        ("mocca_set_heightfield_bank", [{"f32n": [64, 0.0]}, 0, 8, 8, 1.0]), ("mocca_set_heightfield_bank", [None, 2000, 8, 8, 1.0]),
        ("mocca_set_heightfield_bank", [None, 1, 1, 8, 1.0]), ("mocca_set_heightfield_bank", [None, 1, 8, 8, 0.0]),
        ("mocca_set_heightfield_bank", [None, 1, 8, 8, 1e6]), ("mocca_set_heightfield_bank", [None, 1, 32768, 32768, 1.0]),
        ("mocca_set_heightfield", [{"f32n": [64, 0.0]}, 1, 8, 1.0]),
        ("mocca_set_heightfield_bank", [None, 1, 4, 4, 1.0]), ("mocca_generate_heightfields", [0, 1, 1, 4, 1.0, None]),
        ("mocca_set_heightfield_bank", [None, 1, 8, 8, 1.0]),
        ("mocca_generate_heightfields", [1, 1, 1, 4, 1.0, None]), ("mocca_generate_heightfields", [0, 0, 1, 4, 1.0, None]),
        ("mocca_generate_heightfields", [0, 1, 1, 0, 1.0, None]), ("mocca_generate_heightfields", [0, 1, 1, 4, 0.0, None]),
        ("mocca_set_env_fields", [{"dev_i32": [0, 3]}, 0, None]), ("mocca_get_heightfields", [0, 2, B, None]),
        ("mocca_plan_step", [None, None, None, None, None, None]), ("mocca_plan_step", [B, B, B, B, None, None]),
        ctrl((t, nl), n_floats=0), ctrl((t, nl), scale=INF),
        ctrl(rows((0, ci + 1, 16, 2), (0, 16, 21, 0), (1, ci, 16, 2), (1, 16, 1, 0))), ctrl(outside),
        ctrl(rows((0, ci, 16, 2), (0, 16, 20, 0), (1, ci, 16, 2), (1, 16, 1, 0))), ctrl((t, nl)),
        ("mocca_set_base_controller_norm", [{"f32n": [ci, 0.0]}, None, 5.0]), ("mocca_set_base_controller_norm", [{"f32": [INF] + [0.0] * (ci - 1)}, {"f32n": [ci, 1.0]}, 5.0]),
        ("mocca_set_base_controller_norm", [{"f32n": [ci, 0.0]}, {"f32": [-1.0] + [1.0] * (ci - 1)}, 5.0]),
        ("mocca_set_base_controller_norm", [{"f32n": [ci, 0.0]}, {"f32n": [ci, 1.0]}, 0.0]),
        ("mocca_plan_step", [B, None, B, B, None, None]),
        ("mocca_act_plan_step", [B, od, None, 1, B, None, None, None, None, B, B, None, None]),
        ("mocca_act_plan_step", [B, od, None, 1, B, None, None, None, B, B, B, None, None]),
        ("mocca_set_policy", list(nets(od, 14)[:2]) + [od, 14, 5.0]), ("mocca_act_plan_step", [B, od, None, 1, B, None, None, None, B, B, B, None, None]),
        ("mocca_set_policy", [tp, nlp, od, 15, 5.0]), ("mocca_act_plan_step", [B, od, None, 1, B, None, None, None, B, B, B, None, None]),
    ]


def cassie_script(od, ad):
    return core_script(od, ad) + [("mocca_set_randomisation", [{"rand": [0.5, 1.0, 0, 0, 0, 0.0]}])]


SCRIPTS = {   # handle -> (env id, blob keywords, its script)
    "walker": ("Walker3DCustomEnv-v0", {}, walker_script),
    "stepper": ("Walker3DStepperEnv-v0", {}, lambda od, ad: core_script(od, ad) + [("mocca_task_step", [B, None, None, None, B, B, B, None, None])]),
    "planner": ("Walker3DPlannerEnv-v0", {}, planner_script),
    "cassie": ("CassieEnv-v0", {}, cassie_script),
    "cassie_phase": ("CassiePhaseMocca2DEnv-v0", {}, lambda od, ad: [("mocca_reset", [None, 0, B, None]), ("mocca_step", [B, B, B, B, None, None]),
                                                                    ("mocca_observe", [B, None])]),
    "walker_wide": ("Walker3DCustomEnv-v0", {"max_rows": 64, "max_contacts": 20}, lambda od, ad: [("mocca_set_param", [11, 1.0])]),
}


class Handles:
    """the handles of SCRIPTS on the current device, and the arguments of a case as ctypes values"""

    def __init__(self):
        import torch
        from mocca_envs_amd import lib as L, vec_env
        self.torch, self.L, self.lib = torch, L, L.load()
        self.B = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda")
        self.keep, self.h = [], {}
        for name, (env_id, kw, _) in SCRIPTS.items():
            m = vec_env.compile_model_for(env_id)
            for k, v in kw.items():
                setattr(m, k, v)
            blob = m.to_bytes()
            h = C.c_void_p()
            L.check(self.lib.mocca_create(blob, len(blob), vec_env.TASKS[env_id], N, torch.cuda.current_device(), C.byref(h)))
            self.h[name] = h

    def dims(self, name):
        return self.lib.mocca_obs_dim(self.h[name]), self.lib.mocca_act_dim(self.h[name])

    def arg(self, a):
        if a == "B":
            return C.c_void_p(self.B.data_ptr())
        if not isinstance(a, dict):
            return a
        (kind, v), = a.items()
        if kind == "B":
            return C.c_void_p(self.B.data_ptr() + v)
        if kind == "rand":
            r = self.L.RandomisationConfig(*v)
            self.keep.append(r)
            return C.cast(C.byref(r), C.c_void_p)
        if kind in ("dev_i32", "dev_f32n"):
            t = self.torch.tensor(v, dtype=self.torch.int32, device="cuda") if kind == "dev_i32" else \
                self.torch.full((v[0],), v[1], dtype=self.torch.float32, device="cuda")
            self.keep.append(t)
            return C.c_void_p(t.data_ptr())
        arr = np.full(v[0], v[1], np.float32) if kind == "f32n" else np.arange(v, dtype=np.int32) if kind == "iota" else \
            np.asarray(v, np.float32 if kind == "f32" else np.int32)
        arr = np.ascontiguousarray(arr if arr.size else np.zeros(1, arr.dtype))
        self.keep.append(arr)
        return C.c_void_p(arr.ctypes.data)

    def call(self, name, entry, args):
        """-> (return code, the message when the call was refused; None: the refusal set none).  A refusal known to set its message -- an
        unknown parameter id -- goes first, so a call that sets none is told from one that repeats the message before it."""
        assert self.lib.mocca_set_param(self.h[name], 99, 0.0) == -1
        rc = getattr(self.lib, entry)(self.h[name], *[self.arg(a) for a in args])
        self.torch.cuda.synchronize()
        if rc >= 0:
            return int(rc), ""
        msg = (self.lib.mocca_last_error(self.h[name]) or b"").decode()
        return int(rc), None if msg == SENTINEL and (entry, args[:1]) != ("mocca_set_param", [99]) else msg

    def close(self):
        self.torch.cuda.synchronize()
        for h in self.h.values():
            self.lib.mocca_destroy(h)
        self.h = {}


def main(argv):
    out = argv[argv.index("--out") + 1] if "--out" in argv else GOLDEN
    hs = Handles()
    cases = []
    for name, (_, _, script) in SCRIPTS.items():
        for entry, args in script(*hs.dims(name)):
            rc, msg = hs.call(name, entry, args)
            cases.append({"handle": name, "entry": entry, "args": args, "rc": rc, "message": msg})
    hs.close()
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        f.write('{"n_envs": %d,\n"unreached": %s,\n"cases": [\n' % (N, json.dumps(UNREACHED)))   # one case to a line
        f.write(",\n".join(json.dumps(c) for c in cases) + "\n]}\n")
    print(f"{out}: {len(cases)} calls, {sum(c['rc'] < 0 for c in cases)} refused")


if __name__ == "__main__":
    main(sys.argv[1:])
