"""Batched environments on one MI355X: the trainer-facing surface over libmocca_hip.so.

`VecEnv` keeps observations / rewards / done flags in PyTorch-ROCm tensors (device memory
and the current HIP stream are the only things torch is used for) and advances all N
environments with one kernel launch per `step()`.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import numpy as np
import torch

from . import lib as _lib
from . import model as M
from . import rollout as _ro
from .controller import ACTIVATIONS, layer_table

TASKS = {
    "Walker3DCustomEnv-v0": M.TASK_WALKER3D_CUSTOM,
    "Walker3DStepperEnv-v0": M.TASK_WALKER3D_STEPPER,
    "CassieEnv-v0": M.TASK_CASSIE,
    # same tree as Walker3D (child3d.xml / mike.xml): new model blobs on the Walker3D kernels
    "Child3DCustomEnv-v0": M.TASK_WALKER3D_CUSTOM,
    "MikeStepperEnv-v0": M.TASK_WALKER3D_STEPPER,
    # planar robots (walker2d.xml / crab2d.xml): own topologies, Custom task with the quirks of env_locomotion.py:285-314
    "Walker2DCustomEnv-v0": M.TASK_WALKER3D_CUSTOM,
    "Crab2DCustomEnv-v0": M.TASK_WALKER3D_CUSTOM,
    # quadruped (laikago_toes_limits.urdf): own topology, four feet, Custom task ending on body contact
    "LaikagoCustomEnv-v0": M.TASK_WALKER3D_CUSTOM,
    # the quadruped on four live planks (env_locomotion.py:893-979): Laikago topology x Stepper task
    "LaikagoStepperEnv-v0": M.TASK_WALKER3D_STEPPER,
    # CassieEnv(planar=True), __init__.py:24-29: the base held in the x-z plane by three bilateral rows
    "Cassie2DEnv-v0": M.TASK_CASSIE,
    # the planar mocap / phase envs (__init__.py:31-43, env_cassie.py:481-660): Cassie topology, mocap targets and reward
    "CassiePhaseMocca2DEnv-v0": M.TASK_CASSIE,
    "CassiePhaseMirror2DEnv-v0": M.TASK_CASSIE,
    # the walkers on the height field (env_locomotion.py:982-1133): Walker3D / Mike tree x Planner task.  step() takes the 21 joint
    # actions of an external base controller; with one attached (base_controller=) plan_step() takes the planner's 15 numbers
    "Walker3DPlannerEnv-v0": M.TASK_WALKER3D_PLANNER,
    "MikePlannerEnv-v0": M.TASK_WALKER3D_PLANNER,
}
# class attributes of the reference envs that are device parameters here
_DEFAULT_PARAMS = {"LaikagoCustomEnv-v0": {_lib.PARAM_RANDOM_POSE: 0},    # robot_random_start = False, env_locomotion.py:863
                   "LaikagoStepperEnv-v0": {_lib.PARAM_RANDOM_POSE: 0}}   # :899

# Since round 4 the step kernel sets its issue priorities from each wave's PACE (PARAM_PACE_TICKS, default: self-calibrating -- 2.6 % to 8.7 %
# faster than the tables below on every env id, profiles/archive/r04_pace_envs.jsonl); the row-count thresholds only serve a handle's first launch
# (no pace sample yet) and handles that switch the pace off.
# Issue-priority thresholds of the step kernel (PARAM_ISSUE_PRIORITY; timing only, results do not depend on them): constraint-row counts
# above which a wave runs at priority 1 / 2 / 3.  The best set follows the batch's row distribution -- measured per env id with
# a threshold sweep on one MI355X (profiles/archive/r03_prio_sweep_v13.txt: the blob v13 physics hold 5.7 rows per substep on the flat-ground walker
# instead of 12.7, and the thresholds of round 2 had stopped selecting anything: -5.5 % on the launch for re-reading them off the new
# distribution); ids not listed keep the library's default (4, 7, 12: the flat-ground walker).  The stepping-stone walkers carry more rows as
# the curriculum rises: their thresholds grow with it (x 1.7 at curriculum 9).
_ISSUE_PRIORITY = {"LaikagoCustomEnv-v0": (2, 4, 7), "LaikagoStepperEnv-v0": (2, 4, 7), "Child3DCustomEnv-v0": (6, 11, 18),
                   "CassieEnv-v0": (18, 23, 27), "Cassie2DEnv-v0": (24, 29, 33), "CassiePhaseMocca2DEnv-v0": (24, 29, 33),
                   "CassiePhaseMirror2DEnv-v0": (24, 29, 33), "Walker3DPlannerEnv-v0": (10, 16, 24), "MikePlannerEnv-v0": (10, 16, 24),
                   "Walker2DCustomEnv-v0": (6, 9, 14), "Crab2DCustomEnv-v0": (8, 12, 18)}
_ISSUE_PRIORITY_CURRICULUM = {"Walker3DStepperEnv-v0": (7, 11, 17), "MikeStepperEnv-v0": (7, 11, 17)}
_ISSUE_PRIORITY_CURRICULUM_GAIN = 0.7   # thresholds x (1 + gain * curriculum / 9)


def _pack_prio(t):
    return int(t[0]) + 64 * int(t[1]) + 4096 * int(t[2])


_MODELS = {
    "Walker3DCustomEnv-v0": lambda **kw: M.compile_walker3d(M.TASK_WALKER3D_CUSTOM, **kw),
    "Walker3DStepperEnv-v0": lambda **kw: M.compile_walker3d(M.TASK_WALKER3D_STEPPER, **kw),   # kw: plank_class = LargePlank | Plank | Pillar
    "CassieEnv-v0": lambda **kw: M.compile_cassie(**kw),
    "Cassie2DEnv-v0": lambda **kw: M.compile_cassie(planar=True, **kw),
    "CassiePhaseMocca2DEnv-v0": lambda **kw: M.compile_cassie(planar=kw.pop("planar", True), mode=M.CASSIE_PHASE_MOCCA, **kw),
    "CassiePhaseMirror2DEnv-v0": lambda **kw: M.compile_cassie(planar=kw.pop("planar", True), mode=M.CASSIE_PHASE_MIRROR, **kw),
    "LaikagoStepperEnv-v0": lambda **kw: M.compile_laikago(stepper=True, **kw),
    "Child3DCustomEnv-v0": M.compile_child3d,
    "MikeStepperEnv-v0": M.compile_mike,
    "Walker2DCustomEnv-v0": M.compile_walker2d,
    "Crab2DCustomEnv-v0": M.compile_crab2d,
    "LaikagoCustomEnv-v0": M.compile_laikago,
    "Walker3DPlannerEnv-v0": lambda **kw: M.compile_walker3d(M.TASK_WALKER3D_PLANNER, **kw),
    "MikePlannerEnv-v0": lambda **kw: M.compile_mike(planner=True, **kw),
}
_DEFAULT_ENV_OF_TASK = {M.TASK_WALKER3D_CUSTOM: "Walker3DCustomEnv-v0", M.TASK_WALKER3D_STEPPER: "Walker3DStepperEnv-v0",
                        M.TASK_CASSIE: "CassieEnv-v0"}


def compile_model_for(env_or_task, **kw) -> M.MoccaModel:
    """Model blob of a registered env id (or, for the three task ids, of the task's original robot)."""
    env_id = env_or_task if isinstance(env_or_task, str) else _DEFAULT_ENV_OF_TASK[int(env_or_task)]
    return _MODELS[env_id](**kw)


def _ptr(x):
    """a tensor's device pointer as the library takes it; None stays None"""
    return None if x is None else C.c_void_p(x.data_ptr())


class VecEnv:
    """N independent copies of a registered env id, stepped together.

    step(actions[N, 21]) -> (obs[N, obs_dim], reward[N], done[N] uint8, info[N] int32), all on
    `device`.  done bit0 = terminated (reference `self.done`), bit1 = TimeLimit (1000 steps,
    /root/reference/mocca_envs/__init__.py:55).  With auto_reset=True a finished env is reset
    inside the same launch and `obs` is the first observation of its next episode; with
    terminal_obs=True `self.terminal_obs[i]` then holds the observation of env i's FINAL state
    (what the reference's step() returns together with done, env_locomotion.py:128-141 -- the
    value a PPO-style trainer bootstraps from on a TimeLimit truncation); rows of envs that did
    not finish in this step keep their old content.
    """

    randomisation = None    # set_randomisation(): the attached randomisation.Randomisation
    hist = None             # set_history(): the attached history.History, and what it resolved to on this env
    _hist_cols, _hist_act = None, 0
    curriculum = None       # set_curriculum(): the attached curriculum.Curriculum, and its per-level totals [10, 4]
    curriculum_totals = None

    def __init__(self, env_id: str = "Walker3DCustomEnv-v0", n_envs: int = 1, device: Optional[int] = None,
                 auto_reset: bool = True, seed: int = 0, model_blob: Optional[bytes] = None, env_offset: int = 0,
                 terminal_obs: bool = False, max_rows: Optional[int] = None, max_contacts: Optional[int] = None, base_controller=None,
                 **model_kw):
        if env_id not in TASKS:
            raise KeyError(f"{env_id!r} has no GPU stepper yet; available: {sorted(TASKS)}")
        if not torch.cuda.is_available():
            raise _lib.MoccaError("no HIP device visible: the stepper only runs on the GPU (no CPU fallback)")
        self.lib = _lib.load()
        self.stream = None    # None: every call goes to torch's CURRENT stream; set to a torch.cuda.Stream to pin this handle's work to it
        self.env_id, self.task_id, self.n_envs = env_id, TASKS[env_id], int(n_envs)
        self.device_index = torch.cuda.current_device() if device is None else int(device)
        self.device = torch.device("cuda", self.device_index)
        if model_blob is None:
            self.model = compile_model_for(env_id, **model_kw)
            model_blob = self.model.to_bytes()
        else:
            self.model = M.MoccaModel.from_bytes(model_blob)
        if max_rows is not None or max_contacts is not None:
            # Solver caps of this batch (MoccaModel.max_rows / max_contacts; Bullet has neither).  A tree without loop closures whose caps are
            # <= 32 rows / <= 10 contacts runs the COMPACT instance of the step kernel (include/mocca.h MOCCA_PARAM_KERNEL_VARIANT: less LDS
            # per env, more resident waves -- what batches beyond one residency round, > 4096 envs per GPU, want); an env that asks for
            # more in a substep keeps its deepest contacts, exactly as under the default 48 / 12 caps (how often: tools/cap_pressure.py).
            # Caps beyond 48 rows / 12 contacts (up to 64 / 20: every lane of the wave a row) run the ACCURACY instance (mocca_r64.hip: 17 KB of LDS
            # per env, two waves per SIMD) -- Bullet has no cap; `max_rows=64` alone asks for its 20 contacts too.
            if max_rows is not None:
                self.model.max_rows = int(max_rows)
            if max_contacts is not None:
                self.model.max_contacts = int(max_contacts)
            elif int(self.model.max_rows) > 48:
                self.model.max_contacts = min(20, int(self.model.max_rows) // 3)
            else:
                self.model.max_contacts = min(int(self.model.max_contacts), int(self.model.max_rows) // 3)
            model_blob = self.model.to_bytes()
        if self.lib.mocca_model_sizeof() != len(model_blob):
            raise _lib.MoccaError("MoccaModel layout mismatch between model.py and libmocca_hip.so")
        self._blob = C.create_string_buffer(model_blob, len(model_blob))
        h = C.c_void_p()
        _lib.check(self.lib.mocca_create(self._blob, len(model_blob), self.task_id, self.n_envs, self.device_index, C.byref(h)))
        self.h = h
        self.obs_dim = self.lib.mocca_obs_dim(h)
        self.act_dim = self.lib.mocca_act_dim(h)
        self.state_dim = self.lib.mocca_state_dim(h)
        f32 = dict(dtype=torch.float32, device=self.device)
        self.obs = torch.zeros(self.n_envs, self.obs_dim, **f32)
        self.rew = torch.zeros(self.n_envs, **f32)
        self.done = torch.zeros(self.n_envs, dtype=torch.uint8, device=self.device)
        self.info = torch.zeros(self.n_envs, dtype=torch.int32, device=self.device)
        self.seed_value = int(seed)
        self.set_param(_lib.PARAM_AUTO_RESET, 1 if auto_reset else 0)
        self.env_offset = int(env_offset)
        self.set_param(_lib.PARAM_ENV_OFFSET, self.env_offset)
        for pid, val in _DEFAULT_PARAMS.get(env_id, {}).items():
            self.set_param(pid, val)
        if env_id in _ISSUE_PRIORITY:
            self.set_param(_lib.PARAM_ISSUE_PRIORITY, _pack_prio(_ISSUE_PRIORITY[env_id]))
        self.terminal_obs = None
        if terminal_obs:
            self.keep_terminal_obs(True)
        self.ep = None        # episode_stats(): Monitor / TimeLimitMask inside the launch
        self.height_field = None
        self.terrain_bank = None   # set_heightfield_bank(): n_fields, rows, cols, scale
        if self.task_id == M.TASK_WALKER3D_PLANNER:
            from .terrain import load_height_field   # self.terrain.reload(data="height_field_map_0.npy"), env_locomotion.py:1015-1021
            self.set_heightfield(*load_height_field())
        self.trajectory = None
        if self.task_id == M.TASK_CASSIE and self.model.cassie_mode != M.CASSIE_PLAIN:
            from .trajectory import CassieTrajectory   # self.traj = CassieTrajectory(), env_cassie.py:576
            self.set_trajectory(CassieTrajectory())
        self.base_controller = None
        self.plan_dim = self.lib.mocca_plan_dim(h) if self.task_id == M.TASK_WALKER3D_PLANNER else 0
        if base_controller is not None:
            self.set_base_controller(base_controller)

    # ------------------------------------------------------------------
    def _stream(self) -> C.c_void_p:
        if self.stream is not None:      # a handle bound to a stream of its own (sub-batches that step independently: multi.SubBatchedVecEnv)
            return C.c_void_p(self.stream.cuda_stream)
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    # A handle pinned to a stream of its own (`self.stream`) runs its C calls there, while the torch operations around them (uploads,
    # .contiguous(), the caller's reads of what a getter returns) run on torch's CURRENT stream.  Every method except step() orders the
    # two, stream against stream, never through the host: _in() before a call that consumes caller tensors, _out() after a call whose
    # result the caller will read.  step() is the hot path and stays unordered on a pinned stream: the caller orders it (SubBatchedVecEnv's
    # step_async / wait do), or passes ready, contiguous float32 device tensors and reads the outputs after a synchronize.  The bracket is
    # written once, in _call(): every entry point that takes a stream goes through it, except the two launchers of the hot path.
    def _in(self):
        if self.stream is not None:
            self.stream.wait_stream(torch.cuda.current_stream(self.device))

    def _out(self):
        if self.stream is not None:
            torch.cuda.current_stream(self.device).wait_stream(self.stream)

    def _sync(self):
        (self.stream if self.stream is not None else torch.cuda.current_stream(self.device)).synchronize()

    def _call(self, fn, *args, wait: bool = True, then: Optional[str] = "out") -> None:
        """The bracket above around one library call that takes a stream: _in() (unless `wait` is False: a call that reads nothing of the
        caller's), `fn(handle, *args, stream)` with every tensor passed as its device pointer (None stays None), then _out(), _sync()
        (`then="sync"`: the caller's temporaries must outlive the launch) or nothing (`then=None`: another call follows).  `args` keeps the
        tensors alive across the call."""
        if wait:
            self._in()
        _lib.check(fn(self.h, *[C.c_void_p(a.data_ptr()) if isinstance(a, torch.Tensor) else a for a in args], self._stream()), self.h)
        if then == "out":
            self._out()
        elif then == "sync":
            self._sync()

    def _rows(self, name: str, t, width: int) -> int:
        """`t` as float32 [n_envs, >= width] rows on this device (rollout.row_view: THE rule) -> its row stride in floats; `name`: what
        the ValueError calls it"""
        return _ro.row_view(name, t, width, self.n_envs, self.device)

    def close(self):
        if getattr(self, "h", None):
            torch.cuda.synchronize(self.device)
            self.lib.mocca_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_param(self, pid: int, value: float):
        _lib.check(self.lib.mocca_set_param(self.h, pid, float(value)), self.h)
        if pid == _lib.PARAM_CURRICULUM and self.env_id in _ISSUE_PRIORITY_CURRICULUM:   # timing only, see _ISSUE_PRIORITY
            k = 1.0 + _ISSUE_PRIORITY_CURRICULUM_GAIN * min(9.0, max(0.0, float(value))) / 9.0
            base = _ISSUE_PRIORITY_CURRICULUM[self.env_id]
            _lib.check(self.lib.mocca_set_param(self.h, _lib.PARAM_ISSUE_PRIORITY, float(_pack_prio([min(63, round(k * t)) for t in base]))), self.h)

    def set_trajectory(self, traj, control_step: float = 0.03):
        """Attach the reference motion of the Cassie mocap / phase envs (include/mocca.h mocca_set_trajectory); the table is
        copied into the handle.  control_step = CassieEnv.control_step (env_cassie.py:287)."""
        tab = np.ascontiguousarray(traj.table(), np.float32)
        _lib.check(self.lib.mocca_set_trajectory(self.h, tab.ctypes.data_as(C.c_void_p), tab.shape[0], float(traj.max_time()),
                                                 float(control_step)), self.h)
        self.trajectory = traj

    def set_heightfield(self, heights, scale: float):
        """Attach the terrain of the planner envs (include/mocca.h mocca_set_heightfield): heights[rows][cols], x along the columns,
        `scale` grid points per metre; copied into the handle, one grid for all envs."""
        hf = np.ascontiguousarray(heights, np.float32)
        if hf.ndim != 2:
            raise ValueError("heights must be a [rows][cols] grid")
        _lib.check(self.lib.mocca_set_heightfield(self.h, hf.ctypes.data_as(C.c_void_p), hf.shape[0], hf.shape[1], float(scale)), self.h)
        self.height_field = (hf, float(scale))
        self.terrain_bank = None

    # ---- the planner envs' terrain bank (include/mocca.h mocca_set_heightfield_bank) ----
    def _need_bank(self, who: str):
        if getattr(self, "terrain_bank", None) is None:
            raise _lib.MoccaError(f"{who} needs a terrain bank (set_heightfield_bank)")
        return self.terrain_bank

    def set_heightfield_bank(self, fields_or_count, scale: float, rows: Optional[int] = None, cols: Optional[int] = None) -> None:
        """Attach a bank of height fields of one shape, every env on one of them (field 0 until set_env_fields says otherwise).
        `fields_or_count`: heights [K][rows][cols], copied into the handle, or an int K with `rows` and `cols` for a bank of zeros
        that generate_heightfields() fills on the device; K = 1 .. 1024.  None detaches.  May synchronise."""
        if fields_or_count is None:
            _lib.check(self.lib.mocca_set_heightfield_bank(self.h, None, 0, 0, 0, 0.0), self.h)
            self.terrain_bank = self.height_field = None
            return
        if isinstance(fields_or_count, (int, np.integer)):
            if rows is None or cols is None:
                raise ValueError("a bank to be generated into needs rows and cols")
            k, rows, cols, ptr = int(fields_or_count), int(rows), int(cols), None
        else:
            hf = np.ascontiguousarray(fields_or_count, np.float32)
            if hf.ndim != 3:
                raise ValueError("fields must be [K][rows][cols] grids")
            if (rows is not None and int(rows) != hf.shape[1]) or (cols is not None and int(cols) != hf.shape[2]):
                raise ValueError("rows / cols differ from the shape of the fields")
            k, rows, cols = hf.shape
            ptr = hf.ctypes.data_as(C.c_void_p)
        if not 1 <= k <= _lib.HF_MAX_FIELDS:
            raise ValueError(f"a terrain bank holds 1 .. {_lib.HF_MAX_FIELDS} fields")
        _lib.check(self.lib.mocca_set_heightfield_bank(self.h, ptr, k, rows, cols, float(scale)), self.h)
        self.terrain_bank = dict(n_fields=k, rows=rows, cols=cols, scale=float(scale))
        self.height_field = None       # (the fields live on the device: height_fields() reads them back)

    def generate_heightfields(self, seed: int, first: int = 0, count: Optional[int] = None, n_peaks: int = 256, gain: float = 1.0) -> None:
        """Fill fields first .. first + count - 1 (default: to the end of the bank) with random terrain on the device: the reference's
        generator (`HeightField.reload(data=None)`), `n_peaks` peaks, the finished field times `gain`.  Asynchronous; nothing synchronises."""
        bank = self._need_bank("generate_heightfields")
        first = int(first)
        count = bank["n_fields"] - first if count is None else int(count)
        if not 1 <= int(n_peaks) <= _lib.HF_MAX_PEAKS:
            raise ValueError(f"n_peaks must be 1 .. {_lib.HF_MAX_PEAKS}")
        if not (np.isfinite(gain) and gain > 0):
            raise ValueError("gain must be finite and > 0")
        if first < 0 or count < 1 or first + count > bank["n_fields"]:
            raise ValueError(f"fields {first} .. {first + count - 1} are not inside the bank of {bank['n_fields']}")
        self._call(self.lib.mocca_generate_heightfields, first, count, int(seed) & 0xFFFFFFFFFFFFFFFF, int(n_peaks), float(gain))

    def set_env_fields(self, ids=None, redraw_at_reset: bool = False) -> None:
        """Put env e on field ids[e] of the bank (None: every env on field 0).  `redraw_at_reset`: every reset, auto-reset included, draws
        the env's field anew (keyed by seed, episode and global env id).  May synchronise: the ids are checked on the host."""
        self._need_bank("set_env_fields")
        ev = None
        if ids is not None:
            ev = torch.as_tensor(ids, dtype=torch.int32).reshape(-1).to(self.device).contiguous()
            if ev.numel() != self.n_envs:
                raise ValueError("set_env_fields: one field index per env")
        self._call(self.lib.mocca_set_env_fields, ev, 1 if redraw_at_reset else 0)

    def env_fields(self) -> torch.Tensor:
        """The field every env stands on: int32 [N] on the device."""
        self._need_bank("env_fields")
        out = torch.empty(self.n_envs, dtype=torch.int32, device=self.device)
        self._call(self.lib.mocca_get_env_fields, out)
        return out

    def height_fields(self, first: int = 0, count: Optional[int] = None) -> torch.Tensor:
        """Fields first .. first + count - 1 of the bank as they are on the device: float32 [count][rows][cols]."""
        bank = self._need_bank("height_fields")
        first = int(first)
        count = bank["n_fields"] - first if count is None else int(count)
        if first < 0 or count < 1 or first + count > bank["n_fields"]:
            raise ValueError(f"fields {first} .. {first + count - 1} are not inside the bank of {bank['n_fields']}")
        out = torch.empty(count, bank["rows"], bank["cols"], dtype=torch.float32, device=self.device)
        self._call(self.lib.mocca_get_heightfields, first, count, out)
        return out

    # ---- the planner envs' base controller (env_locomotion.py:1029-1040, :1091-1101) ----
    def set_base_controller(self, ctrl, action_scale: float = 2.0):
        """Attach the base controller of a planner env (include/mocca.h mocca_set_base_controller; None detaches).  `ctrl`: a
        `controller.BaseController` (or any object with `.actor` and `.critic`, or the pair (actor, critic)); each net a list of layers (W[out][in], b[out], activation) with activation one
        of ACTIVATIONS -- actor 65 -> ... -> 21, critic 65 -> ... -> 1, hidden widths multiples of 16 up to 256, at most 8 layers per net.
        `action_scale` multiplies the plan (Walker3DPlannerEnv.action_scale = 2).  From the next reset() / step() / observe() on the handle
        keeps `robot_state` (the first 50 floats of the last observation) as the controller's input: attach before reset(), or call
        observe() after attaching.  A `ctrl` that carries `obs_mean` / `obs_inv_std` (and `clip`) has them attached too
        (set_base_controller_norm); one without the attributes runs on the raw input."""
        if ctrl is None:
            _lib.check(self.lib.mocca_set_base_controller(self.h, None, 0, None, 0, 0.0), self.h)
            self.base_controller = None
            return
        mean, inv_std = getattr(ctrl, "obs_mean", None), getattr(ctrl, "obs_inv_std", None)
        if (mean is None) != (inv_std is None):
            raise ValueError("a controller carries obs_mean and obs_inv_std together, or neither")
        actor, critic = (ctrl.actor, ctrl.critic) if hasattr(ctrl, "actor") else ctrl
        layers = [(np.asarray(w, np.float32), np.asarray(b, np.float32), act) for w, b, act in list(actor) + list(critic)]
        if any(w.ndim != 2 or b.size != w.shape[0] or act not in ACTIVATIONS for w, b, act in layers):    # the widths are the library's to refuse
            raise ValueError(f"a layer is (W[out][in], b[out], activation in {ACTIVATIONS})")
        params = np.concatenate([x.reshape(-1) for w, b, _ in layers for x in (w, b)] + [np.zeros(0, np.float32)])
        table = layer_table(actor, critic, "flat")
        _lib.check(self.lib.mocca_set_base_controller(self.h, params.ctypes.data_as(C.c_void_p), params.size, table.ctypes.data_as(C.c_void_p),
                                                      table.shape[0], float(action_scale)), self.h)
        self.base_controller = ctrl     # (the library dropped the statistics of the controller this one replaces)
        if mean is not None:
            self.set_base_controller_norm(mean, inv_std, getattr(ctrl, "clip", 10.0))
        f32 = dict(dtype=torch.float32, device=self.device)
        self._base_action, self._base_value = torch.zeros(self.n_envs, self.act_dim, **f32), torch.zeros(self.n_envs, **f32)

    def set_base_controller_norm(self, mean, inv_std, clip: float = 10.0):
        """Observation statistics of the attached base controller (include/mocca.h mocca_set_base_controller_norm; mean None detaches):
        float32 [65] each, over the controller's input row [robot_state(50), plan(15) * action_scale]; the kernel applies
        clamp((x - mean) * inv_std, -clip, clip) in front of both nets.  set_base_controller(ctrl) calls this for a `ctrl` that carries
        `obs_mean` / `obs_inv_std`, and drops the statistics of the controller it replaces."""
        if self.base_controller is None:
            raise _lib.MoccaError("set_base_controller_norm needs a base controller (set_base_controller)")
        if mean is None:
            _lib.check(self.lib.mocca_set_base_controller_norm(self.h, None, None, float(clip)), self.h)
            return
        mean, inv_std = np.ascontiguousarray(mean, np.float32).reshape(-1), np.ascontiguousarray(inv_std, np.float32).reshape(-1)
        if mean.size != 65 or inv_std.size != 65:
            raise ValueError("the statistics of a base controller have 65 entries: robot_state(50) and the scaled plan(15)")
        _lib.check(self.lib.mocca_set_base_controller_norm(self.h, mean.ctypes.data_as(C.c_void_p), inv_std.ctypes.data_as(C.c_void_p), float(clip)), self.h)

    def plan_step(self, plans: torch.Tensor, obs_out: Optional[torch.Tensor] = None,
                  rew_out: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
        """env.step(plan) of the planner envs (include/mocca.h mocca_plan_step): plans [N, 15] -> the attached base controller (one kernel)
        -> the step kernel, on the same stream; the reward is progress + log(max(1, value)) / 3 and that is what episode_stats() sums.
        Same contract as step() otherwise (obs_out / rew_out, streams)."""
        if not self.plan_dim:
            raise ValueError("plan_step: planner envs only")
        return self._launch_step(self.lib.mocca_plan_step, plans, self.plan_dim, "plans", obs_out, rew_out)

    def base_outputs(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """(action [N, 21] before apply_action's clip, value [N]) of the controller in the last plan_step(): copies, on the device."""
        if self.base_controller is None:
            raise _lib.MoccaError("base_outputs needs a base controller (set_base_controller)")
        self._call(self.lib.mocca_get_base_outputs, self._base_action, self._base_value, wait=False)   # (buffers of this object's: nothing to wait for)
        return self._base_action.clone(), self._base_value.clone()

    # ---- the trainer's own policy on the device (include/mocca.h mocca_set_policy / mocca_update_policy / mocca_act / mocca_act_step) ----
    policy = None
    mirror_loss = None   # (tables, coef) while set_policy_mirror_loss has one attached
    mirror_dup = None    # tables while set_policy_mirror_dup has them attached
    teacher = None
    critic_rows = None   # the rows set_critic_rows bound (an asymmetric policy's critic reads them)
    _pol_action = None   # act_step()'s own action buffer, made on first use
    _scan_points = None  # the pattern set_height_scan attached
    _depth_cam = None    # the camera set_depth_camera attached
    _host_np = None      # host_mirror()'s numpy views, made on first use

    def _set_slot(self, fn, policy) -> None:
        """set_policy() / set_teacher(): the layer table and shapes of `policy` (None: detach) to `fn`, mocca_set_policy or mocca_set_teacher"""
        if policy is None:
            _lib.check(fn(self.h, None, 0, 0, 0, 0.0), self.h)
            return
        table = np.ascontiguousarray(policy.table(), np.int32)
        if getattr(policy, "asymmetric", False):      # a privileged critic: the student's slot alone takes one
            if fn is not self.lib.mocca_set_policy:
                raise ValueError("set_teacher: the teacher is a plain policy; one with a privileged critic is not supported")
            _lib.check(self.lib.mocca_set_policy_priv(self.h, table.ctypes.data_as(C.c_void_p), table.shape[0], int(policy.in_dim),
                                                      int(policy.critic_in_dim), int(policy.act_dim), float(policy.clip)), self.h)
            return
        _lib.check(fn(self.h, table.ctypes.data_as(C.c_void_p), table.shape[0], int(policy.in_dim), int(policy.act_dim), float(policy.clip)), self.h)

    def _update_slot(self, fn, params) -> None:
        """update_policy() / update_teacher(): a `DevicePolicy`'s or a flat tensor's weights to `fn`, mocca_update_policy or mocca_update_teacher"""
        flat = torch.from_numpy(params.flat_params()) if hasattr(params, "flat_params") else params
        flat = flat.detach().to(device=self.device, dtype=torch.float32).contiguous().reshape(-1)
        self._call(fn, flat, flat.numel())       # `flat` may be freed (and its memory reused on the current stream) as soon as this returns

    @property
    def _mirrored(self) -> bool:
        """does the attached policy carry a mirror attachment: symmetry, a mirror loss or duplicated rows"""
        return getattr(self.policy, "symmetry", None) is not None or self.mirror_loss is not None or self.mirror_dup is not None

    def set_policy(self, policy) -> None:
        """Attach a `policy.DevicePolicy` (None detaches): its shapes size the kernel's image, its weights are uploaded (update_policy).
        An `asymmetric` policy (a privileged critic: another `critic_in_dim`, or critic statistics) goes through mocca_set_policy_priv:
        bind the critic's rows with set_critic_rows() before act() is asked for a value; the mirror attachments, distill_grad() and
        distill_update() are not provided for it.  May synchronise."""
        self._set_slot(self.lib.mocca_set_policy, policy)
        self.policy, self.mirror_loss, self.mirror_dup = policy, None, None   # mocca_set_policy has dropped every attachment
        self.critic_rows = None                                               # and the critic-row binding
        if policy is None:
            return
        self.update_policy(policy)
        if getattr(policy, "symmetry", None) is not None:      # after the shapes: mocca_set_policy has dropped whatever was attached
            self.set_policy_symmetry(policy.symmetry)

    def set_critic_rows(self, rows: Optional[torch.Tensor]) -> None:
        """Bind the rows an asymmetric policy's critic reads in act() / act_step() / act_plan_step(): `rows` float32 [n_envs, >= critic_in_dim]
        on the env's device with contiguous rows, caller-owned and read AT EVERY LAUNCH from this fixed address (`TorchVecEnv.privileged`), so
        the calls stay capturable; this object keeps a reference.  None detaches.  set_policy() drops the binding."""
        if rows is None:
            _lib.check(self.lib.mocca_set_critic_rows(self.h, None, 0), self.h)
            self.critic_rows = None
            return
        p = self.policy
        if p is None or not getattr(p, "asymmetric", False):
            raise _lib.MoccaError("set_critic_rows needs a policy with a privileged critic (set_policy with an asymmetric DevicePolicy)")
        stride = self._rows("the critic's rows", rows, p.critic_in_dim)
        _lib.check(self.lib.mocca_set_critic_rows(self.h, C.c_void_p(rows.data_ptr()), stride), self.h)
        self.critic_rows = rows

    def _set_policy_mirror(self, name: str, tables, *extra):
        """What the three setters below share: mocca_<name>(tables, *extra) -> the tables as the library took them, or None (detached)."""
        if self.policy is None:
            raise _lib.MoccaError(f"{name} needs a policy (set_policy)")
        fn = getattr(self.lib, "mocca_" + name)
        if tables is None:
            _lib.check(fn(self.h, None, None, None, None, *extra), self.h)   # (a detach reads nothing of `extra`)
            return None
        t = [np.ascontiguousarray(x, d) for x, d in zip(tables, (np.int32, np.float32, np.int32, np.float32))]
        if (t[0].size, t[1].size, t[2].size, t[3].size) != (self.policy.in_dim, self.policy.in_dim, self.policy.act_dim, self.policy.act_dim):
            raise ValueError(f"the mirror tables have {self.policy.in_dim} input and {self.policy.act_dim} action entries")
        _lib.check(fn(self.h, *[x.ctypes.data_as(C.c_void_p) for x in t], *extra), self.h)
        return tuple(t)

    def set_policy_symmetry(self, tables) -> None:
        """Attach mirror tables (symmetry.mirror_tables: in_perm, in_sign, act_perm, act_sign) to the policy set_policy attached: act() and
        act_step() then run the symmetric policy (csrc/mocca_policy.h: Symmetry), still one launch.  None detaches.  set_policy() with a
        `DevicePolicy(symmetry=)` calls this; update_policy() leaves the symmetry alone.  May synchronise."""
        self._set_policy_mirror("set_policy_symmetry", tables)
        if hasattr(self.policy, "with_symmetry"):
            self.policy = self.policy.with_symmetry(tables)

    def set_policy_mirror_loss(self, tables, coef: float = 0.0) -> None:
        """Attach SymmetricRL's mirror-symmetry LOSS to the policy set_policy attached, for the gradient only: `tables` as in
        set_policy_symmetry (`policy_mirror_tables(policy)` gives this env's), `coef` >= 0 the weight of
        mean((actor(obs) - M_a actor(M_o obs))^2) in the loss (0: monitored, not trained on).  act() and act_step() keep running the plain
        policy; ppo_grad() and ppo_update() then differentiate PPO's loss plus the term (mocca_ppo_grad_mirror) and report it in
        stats[7].  None detaches.  Exclusive with a symmetric policy; set_policy() drops it, update_policy() leaves it alone.  May
        synchronise."""
        t = self._set_policy_mirror("set_policy_mirror_loss", tables, float(coef))
        self.mirror_loss = None if t is None else (t, float(coef))

    def set_policy_mirror_dup(self, tables) -> None:
        """Attach SymmetricRL's DUPLICATED TUPLES to the policy set_policy attached, for the gradient only: `tables` as in
        set_policy_symmetry (`policy_mirror_tables(policy)` gives this env's).  act() and act_step() keep running the plain policy;
        ppo_grad() and ppo_update() then differentiate PPO's plain loss over every row AND its mirror image (M_o s, M_a a), 2 B samples
        (mocca_ppo_grad_dup); a twin borrows its row's old_logp, so stats[7], the twins' share of stats[3], measures how far off-policy
        the policy's asymmetry puts them.  None detaches.  Exclusive with a symmetric policy and with a mirror loss; set_policy() drops
        it, update_policy() leaves it alone.  May synchronise."""
        self.mirror_dup = self._set_policy_mirror("set_policy_mirror_dup", tables)

    def policy_mirror_tables(self, policy):
        """The mirror tables (in_perm, in_sign, act_perm, act_sign) of THIS env for `policy` (a `policy.DevicePolicy`): built from
        get_mirror_indices() and, where the policy's input is [obs | scan], [obs | depth] or [obs | scan | depth], the attached scan pattern and
        the attached depth camera's shape (symmetry.mirror_tables; ValueError for a camera outside the robot's sagittal plane).  With a
        history attached (set_history) the policy's input must be the FULL row [obs | scan | depth | hist] of whatever is attached, and the
        tables cover the history block too.  Envs whose reference publishes no six index lists raise NotImplementedError."""
        from .symmetry import mirror_tables
        mi = self.get_mirror_indices()
        if isinstance(mi, dict):
            raise NotImplementedError("the Cassie mocap envs publish a dict of index lists (env_cassie.py:554-571), not get_mirror_indices()'s six")
        scan, cam = self._scan_points, self._depth_cam
        ns, nd = (0 if scan is None else len(scan)), (0 if cam is None else cam.width * cam.height)
        hist = None if self.hist is None else (self._hist_cols, self._hist_act, self.hist.steps)
        if hist is not None:                                                    # [obs | scan | depth | hist]: the full row, nothing else
            if policy.in_dim != self.obs_dim + ns + nd + self.history_dim:
                raise ValueError(f"the policy's input has {policy.in_dim} entries: with a history attached it must be the full row, the env's "
                                 f"observation {self.obs_dim}" + ("" if scan is None else f", its height scan {ns}")
                                 + ("" if cam is None else f", its depth image {nd}") + f" and its history {self.history_dim}")
        elif policy.in_dim == self.obs_dim:                                     # [obs]
            scan = cam = None
        elif scan is not None and cam is not None and ns == nd and policy.in_dim == self.obs_dim + ns:
            raise ValueError(f"the policy's input has {policy.in_dim} entries: [obs | scan] and [obs | depth] are both {self.obs_dim} + {ns} wide here; "
                             "detach the sensor the policy does not read (set_height_scan(None) / set_depth_camera(None))")
        elif scan is not None and policy.in_dim == self.obs_dim + ns:           # [obs | scan]
            cam = None
        elif cam is not None and policy.in_dim == self.obs_dim + nd:            # [obs | depth]
            scan = None
        elif cam is None or policy.in_dim != self.obs_dim + ns + nd:            # [obs | scan | depth]
            raise ValueError(f"the policy's input has {policy.in_dim} entries, the env's observation {self.obs_dim}"
                             + ("" if scan is None else f", its height scan {ns}") + ("" if cam is None else f", its depth image {nd}"))
        if cam is not None and not cam.sagittal:
            raise ValueError("the depth camera does not lie in the robot's sagittal plane (body 0, offset[1] == 0, yaw == roll == 0): "
                             "the mirrored robot does not see the column-flipped image")
        return mirror_tables(mi, self.obs_dim, policy.act_dim, scan_points=scan, depth_shape=None if cam is None else cam.shape, history=hist)

    def symmetric_policy(self, policy):
        """A copy of `policy` (a `policy.DevicePolicy`) with the mirror tables of THIS env (policy_mirror_tables)."""
        return policy.with_symmetry(self.policy_mirror_tables(policy))

    def update_policy(self, params) -> None:
        """New weights for the attached policy, once per PPO iteration: a `DevicePolicy` of the same shapes, or a flat float32 tensor in
        `DevicePolicy.flat_params()`'s order that is already on the device (what a trainer builds with one torch.cat of its parameters,
        log_std and observation statistics).  One repack kernel on the stream; nothing synchronises."""
        if self.policy is None:
            raise _lib.MoccaError("update_policy needs a policy (set_policy)")
        self._update_slot(self.lib.mocca_update_policy, params)

    def _act_args(self, obs, eps, deterministic, out, logp, value):
        """check the tensors of act() / act_step() -> (ctypes arguments in_dev .. mean_dev, the output dict)"""
        p = self.policy
        if p is None:
            raise _lib.MoccaError("act needs a policy (set_policy)")
        n, a = self.n_envs, p.act_dim
        stride = self._rows("the policy's input", obs, p.in_dim)
        if eps is not None:
            if eps.shape != (n, a) or eps.dtype != torch.float32 or eps.device != self.device or not eps.is_contiguous():
                raise ValueError(f"eps must be a contiguous float32 [n_envs, {a}] tensor on the env's device")
        out = dict(out or {})
        f32 = dict(dtype=torch.float32, device=self.device)
        if "action" not in out:
            out["action"] = torch.empty(n, a, **f32)
        if logp and "logp" not in out:
            out["logp"] = torch.empty(n, **f32)
        if value and "value" not in out:
            out["value"] = torch.empty(n, **f32)
        for k, numel in (("action", n * a), ("logp", n), ("value", n), ("mean", n * a)):
            t = out.get(k)
            if t is not None and (t.numel() != numel or t.dtype != torch.float32 or t.device != self.device or not t.is_contiguous()):
                raise ValueError(f"out[{k!r}] must be a contiguous float32 tensor of {numel} elements on the env's device")
        return (_ptr(obs), stride, _ptr(eps), int(bool(deterministic)), _ptr(out["action"]), _ptr(out.get("logp")), _ptr(out.get("value")),
                _ptr(out.get("mean"))), out

    def act(self, obs: torch.Tensor, eps: Optional[torch.Tensor] = None, deterministic: bool = False, out: Optional[dict] = None) -> dict:
        """`actor_critic.act(obs)` as one launch: -> {"action" [N, A], "logp" [N], "value" [N]} (and "mean" [N, A] when `out` has that key),
        float32 on the device.  `obs`: float32 [N, >= in_dim] with contiguous rows (a view of wider storage will do).  `eps` [N, A]: the
        caller's standard-normal noise; `deterministic`: the mean; neither: noise drawn in the kernel from (seed, env id, the env's step and
        episode counters) -- two calls without a step() in between draw the same noise.  `out`: any of the output tensors, caller-owned
        (rows of a trainer's rollout storage; "logp" / "value" may be [N, 1])."""
        args, out = self._act_args(obs, eps, deterministic, out, True, True)
        self._call(self.lib.mocca_act, *args)
        return out

    def act_step(self, obs: torch.Tensor, eps: Optional[torch.Tensor] = None, deterministic: bool = False, action_out: Optional[torch.Tensor] = None,
                 logp_out: Optional[torch.Tensor] = None, value_out: Optional[torch.Tensor] = None, obs_out: Optional[torch.Tensor] = None,
                 rew_out: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
        """act(obs) and step(action) as two launches of one C call (include/mocca.h mocca_act_step): the action, its log-probability and the
        value go to `action_out` / `logp_out` / `value_out` (logp and value only where given; the action to a buffer of this object
        otherwise: `self.last_action`), the step's results are step()'s, bit for bit.  Same contract as step() otherwise."""
        return self._launch_act_step(self.lib.mocca_act_step, obs, eps, deterministic, action_out, logp_out, value_out, obs_out, rew_out)

    def act_plan_step(self, obs: torch.Tensor, eps: Optional[torch.Tensor] = None, deterministic: bool = False, plan_out: Optional[torch.Tensor] = None,
                      logp_out: Optional[torch.Tensor] = None, value_out: Optional[torch.Tensor] = None, obs_out: Optional[torch.Tensor] = None,
                      rew_out: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
        """act_step()'s twin on a planner env (include/mocca.h mocca_act_plan_step): the attached policy's action is the 15-number plan, and
        act(obs), the base controller and the step kernel are three launches of one C call.  The plan goes to `plan_out` (or
        `self.last_action`); the results are those of act() followed by plan_step(plan), bit for bit."""
        if not self.plan_dim:
            raise ValueError("act_plan_step: planner envs only")
        return self._launch_act_step(self.lib.mocca_act_plan_step, obs, eps, deterministic, plan_out, logp_out, value_out, obs_out, rew_out)

    def _launch_act_step(self, entry, obs, eps, deterministic, action_out, logp_out, value_out, obs_out, rew_out):
        """act_step() / act_plan_step(): check the tensors, launch `entry` (mocca_act_step or mocca_act_plan_step: same argument list)"""
        given = {k: v for k, v in (("action", action_out), ("logp", logp_out), ("value", value_out)) if v is not None}
        if "action" not in given and self.policy is not None:
            if self._pol_action is None or self._pol_action.shape[1] != self.policy.act_dim:
                self._pol_action = torch.zeros(self.n_envs, self.policy.act_dim, dtype=torch.float32, device=self.device)
            given["action"] = self._pol_action
        args, out = self._act_args(obs, eps, deterministic, given, False, False)
        self.last_action = out["action"]
        obs_o, rew = (self.obs, self.rew) if obs_out is None and rew_out is None else self._step_out(obs_out, rew_out)
        _lib.check(entry(self.h, *args, C.c_void_p(obs_o.data_ptr()), C.c_void_p(rew.data_ptr()), C.c_void_p(self.done.data_ptr()),
                         C.c_void_p(self.info.data_ptr()), self._stream()), self.h)
        return obs_o, rew, self.done, self.info

    # ---- the end of a rollout on the device (include/mocca.h mocca_gae / mocca_obs_stats) ----
    def finish_rollout(self, reward: torch.Tensor, value: torch.Tensor, masks: torch.Tensor, bad_masks: torch.Tensor, gamma: float = 0.99,
                       lam: float = 0.95, reward_scale: float = 1.0, returns: Optional[torch.Tensor] = None, adv: Optional[torch.Tensor] = None,
                       normalise: bool = True, adv_eps: float = 1e-8, moments: Optional[torch.Tensor] = None) -> dict:
        """`rollouts.compute_returns(next_value, True, gamma, lam, use_proper_time_limits=True)` and the advantage normalisation of
        `ppo.update` as two launches: -> {"returns", "adv" (normalised when `normalise`), "moments" [2] = mean and std of the raw advantages}.
        `reward` [T, N] or [T, N, 1]; `value`, `masks`, `bad_masks` [T + 1, N(, 1)] (value[T] is next_value; rows 1 .. T of the masks are
        read): contiguous float32 on the env's device -- a trainer's rollout storage as it is.  `reward_scale` multiplies the reward.
        `returns` / `adv` / `moments`: caller-owned outputs; allocated where none is given.  The arithmetic is fixed operation by
        operation (include/mocca.h) and the sums have a fixed order: the same bits on every run."""
        T = _ro.gae_args(self.n_envs, self.device, reward, value, masks, bad_masks, gamma, lam, reward_scale, returns, adv, normalise, adv_eps)
        _ro.stats_out("moments", moments, 2, self.device)
        f32 = dict(dtype=torch.float32, device=self.device)
        returns = torch.empty(reward.shape, **f32) if returns is None else returns
        adv = torch.empty(reward.shape, **f32) if adv is None else adv
        moments = torch.empty(2, **f32) if moments is None else moments
        self._call(self.lib.mocca_gae, reward, value, masks, bad_masks, T, float(gamma), float(lam), float(reward_scale), returns, adv,
                   int(bool(normalise)), float(adv_eps), moments)
        return {"returns": returns, "adv": adv, "moments": moments}

    def update_obs_stats(self, stats, rows: torch.Tensor, mean_out: Optional[torch.Tensor] = None, inv_std_out: Optional[torch.Tensor] = None) -> None:
        """VecNormalize's `ob_rms.update` over a whole rollout as two launches: merges `rows` [..., >= stats.dim] (float32 on the env's device,
        contiguous last dimension, one stride between rows: `rollouts.obs[1:]`; only the first `stats.dim` floats of a row are read) into
        the `rollout.ObsStats`' float64 state, and writes float32 mean and 1 / sqrt(var + eps) to `mean_out` / `inv_std_out` where given --
        the tail of the flat parameter tensor `update_policy` takes."""
        if stats.state.device != self.device:
            raise ValueError("the statistics' state must be on the env's device")
        if rows.device != self.device:
            raise ValueError("rows must be on the env's device")
        n_rows, stride = _ro.rows_2d(rows, stats.dim)
        _ro.stats_out("mean_out", mean_out, stats.dim, self.device)
        _ro.stats_out("inv_std_out", inv_std_out, stats.dim, self.device)
        self._call(self.lib.mocca_obs_stats, rows, n_rows, stride, stats.dim, stats.state, float(stats.eps), mean_out, inv_std_out)

    # ---- a PPO minibatch step on the device (include/mocca.h mocca_ppo_grad / mocca_ppo_grad_sym / mocca_ppo_grad_mirror / mocca_ppo_grad_dup) ----
    def ppo_grad(self, obs: torch.Tensor, action: torch.Tensor, old_logp: torch.Tensor, adv: torch.Tensor, returns: torch.Tensor,
                 idx: Optional[torch.Tensor] = None, old_value: Optional[torch.Tensor] = None, clip: float = 0.2, value_coef: float = 0.5,
                 entropy_coef: float = 0.0, value_clip: bool = False, grad: Optional[torch.Tensor] = None,
                 stats: Optional[torch.Tensor] = None, critic_obs: Optional[torch.Tensor] = None) -> dict:
        """The body of `ppo.update`'s minibatch loop up to `optimizer.step()` -- `evaluate_actions`, the clipped surrogate, the value loss,
        `loss.backward()` -- as four launches: -> {"grad" [policy.n_head()] in `DevicePolicy.flat_params()`'s order (`split_grad` gives
        per-layer views), "stats" [8]: mean surrogate, value loss, entropy, mean(old_logp - logp), clip fraction, sum of grad^2, 0, 0}.
        `obs` [R, >= in_dim] or [T, N, >= in_dim] RAW rows with a contiguous last dimension and one stride between rows (`rollouts.obs[:-1]`);
        `action` [.., act_dim], `old_logp`, `adv`, `returns`, `old_value` ([..] or [.., 1]; `old_value` only for `value_clip`): contiguous
        float32 of the same R rows.  `idx` int64 [B]: the minibatch's rows (a chunk of `torch.randperm(R)`), every entry in 0 .. R - 1 -- the
        kernel does not check; None: all R rows.  Reads the weights `update_policy` last wrote.  A policy with mirror tables attached
        (`DevicePolicy(symmetry=)`, `set_policy_symmetry`) takes the symmetric network's gradient, what autograd gives through
        `symmetry.SymmetricGaussian.evaluate_actions` (mocca_ppo_grad_sym: the same four launches on twice the columns; the entropy is the
        symmetrised log_std's).  With a mirror loss attached (`set_policy_mirror_loss`) the loss gains coef * L_m and stats[7] is L_m
        (mocca_ppo_grad_mirror: the plain policy, the same layout as the symmetric call).  With duplicated rows attached
        (`set_policy_mirror_dup`) the plain loss runs over the B rows and their B mirror images, every mean over 2 B, and stats[7] is the
        twins' share of stats[3] (mocca_ppo_grad_dup: the same layout again).  At most 2^21 rows in any of the three cases, 2^22
        otherwise.  `grad` / `stats`: caller-owned outputs, allocated where none is
        given.  The same inputs give the same bits on every run.  An asymmetric policy (a privileged critic) takes `critic_obs`
        [R, >= critic_in_dim] or [T, N, >= critic_in_dim], the storage's RAW critic rows of the same R rows, gathered through the same
        `idx` (mocca_ppo_grad_priv); a plain policy refuses it."""
        if self.policy is None:
            raise _lib.MoccaError("ppo_grad needs a policy (set_policy)")
        priv = self._critic_args(obs, critic_obs)
        symmetric = getattr(self.policy, "symmetry", None) is not None
        mirror, dup = self.mirror_loss is not None, self.mirror_dup is not None
        _, stride, n_batch = _ro.ppo_args(self.policy, self.device, obs, action, old_logp, adv, returns, idx, old_value, clip, value_coef,
                                          entropy_coef, value_clip, grad, stats, symmetric=self._mirrored)
        out = self._grad_out(grad, stats)
        call = self.lib.mocca_ppo_grad_dup if dup else self.lib.mocca_ppo_grad_mirror if mirror else self.lib.mocca_ppo_grad_sym if symmetric else self.lib.mocca_ppo_grad
        if priv:
            call = self.lib.mocca_ppo_grad_priv
        self._call(call, obs, stride, *priv, action, old_logp, adv, returns, old_value, idx, n_batch, float(clip), float(value_coef), float(entropy_coef),
                   int(bool(value_clip)), out["grad"], out["stats"])
        return out

    def _critic_args(self, obs, critic_obs) -> tuple:
        """ppo_grad() / ppo_update(): `critic_obs` against the attached policy -> (critic_obs, its row stride) for an asymmetric policy, ()
        for a plain one; a ValueError where the two do not go together or the rows are not `obs`' rows"""
        asym = getattr(self.policy, "asymmetric", False)
        if not asym:
            if critic_obs is not None:
                raise ValueError("critic_obs goes with an asymmetric policy (a privileged critic); the attached policy's critic reads obs")
            return ()
        if not isinstance(critic_obs, torch.Tensor) or critic_obs.device != self.device:
            raise ValueError("the attached policy has a privileged critic: critic_obs must be a float32 tensor on the env's device")
        n_rows, stride = _ro.rows_2d(critic_obs, self.policy.critic_in_dim)
        if isinstance(obs, torch.Tensor) and obs.dim() >= 1 and n_rows != _ro.rows_2d(obs, self.policy.in_dim)[0]:
            raise ValueError("critic_obs must hold one row per row of obs")
        return (critic_obs, stride)

    def _grad_out(self, grad, stats) -> dict:
        """what ppo_grad() / distill_grad() write and return: the caller's `grad` / `stats`, allocated where none is given"""
        f32 = dict(dtype=torch.float32, device=self.device)
        return {"grad": torch.empty(self.policy.n_head(), **f32) if grad is None else grad, "stats": torch.empty(8, **f32) if stats is None else stats}

    # ---- the optimiser step and the whole update on the device (include/mocca.h mocca_adam_step / mocca_ppo_update) ----
    def adam_step(self, params: torch.Tensor, grad: torch.Tensor, state, n_params: Optional[int] = None, lr: float = 3e-4,
                  betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-5, max_grad_norm: float = 0.5) -> None:
        """`clip_grad_norm_(.., max_grad_norm)`, `optimizer.step()` of torch.optim.Adam and `update_policy(params)` as three launches.
        `params`: the flat float32 tensor `update_policy` takes (with or without the statistics tail), updated IN PLACE; its first
        `n_params` floats are trainable (None: all `policy.n_head()`; `n_head - act_dim` keeps log_std fixed).  `grad`: `ppo_grad`'s
        gradient.  `state`: a `rollout.AdamState(policy.n_head(), device)`.  `max_grad_norm` 0: no clip.  A gradient whose norm is not
        finite skips the step and counts it in `state.clock[3]`.  Nothing synchronises; the arithmetic is fixed operation by operation."""
        if self.policy is None:
            raise _lib.MoccaError("adam_step needs a policy (set_policy)")
        n_params = _ro.adam_args(self.policy, self.device, params, grad, state, n_params, lr, betas, eps, max_grad_norm)
        self._call(self.lib.mocca_adam_step, params, params.numel(), grad, n_params, state.moments, state.clock, float(lr), float(betas[0]),
                   float(betas[1]), float(eps), float(max_grad_norm))

    def ppo_update(self, obs: torch.Tensor, action: torch.Tensor, old_logp: torch.Tensor, adv: torch.Tensor, returns: torch.Tensor,
                   params: torch.Tensor, state, minibatch_rows: int, epochs: int, old_value: Optional[torch.Tensor] = None, clip: float = 0.2,
                   value_coef: float = 0.5, entropy_coef: float = 0.0, value_clip: bool = False, n_params: Optional[int] = None, lr: float = 3e-4,
                   betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-5, max_grad_norm: float = 0.5, seed: int = 0,
                   stats: Optional[torch.Tensor] = None, critic_obs: Optional[torch.Tensor] = None) -> dict:
        """a2c-ppo-acktr's `agent.update(rollouts)` as one call: `epochs` passes over the R rollout rows, each a fresh shuffle cut into
        M = R // minibatch_rows minibatches (the remainder is dropped), each minibatch `ppo_grad` on its rows and `adam_step` on `params`
        -- the same bits as that loop.  The storage tensors are `ppo_grad`'s, `params` / `state` / `n_params` / `lr` .. `max_grad_norm`
        `adam_step`'s; `params` must hold what `update_policy` last received.  The shuffle is keyed by `seed` and the state's step count.
        -> {"stats": [epochs * M, 8]}: `ppo_grad`'s statistics per minibatch, [6] the clip coefficient applied (0: a skipped step), [7] L_m
        with a mirror loss attached, the twins' share of [3] with duplicated rows;
        `stats`: a caller-owned output.  Nothing synchronises or is read on the host; capturable after one warm call of the same shapes
        (the scalars and the seed are baked into the capture).  `critic_obs`: an asymmetric policy's critic rows, as in `ppo_grad`
        (mocca_ppo_update_priv)."""
        if self.policy is None:
            raise _lib.MoccaError("ppo_update needs a policy (set_policy)")
        priv = self._critic_args(obs, critic_obs)
        symmetric = self._mirrored       # each attachment halves the row bound
        n_rows, stride, _ = _ro.ppo_args(self.policy, self.device, obs, action, old_logp, adv, returns, None, old_value, clip, value_coef,
                                         entropy_coef, value_clip, None, None, symmetric=symmetric)
        return self._update_loop(self.lib.mocca_ppo_update_priv if priv else self.lib.mocca_ppo_update,
                                 (obs, stride, *priv, action, old_logp, adv, returns, old_value), n_rows, minibatch_rows, epochs,
                                 (float(clip), float(value_coef), float(entropy_coef), int(bool(value_clip))), params, state, n_params, lr, betas,
                                 eps, max_grad_norm, seed, stats, symmetric)

    def _update_loop(self, fn, data, n_rows, minibatch_rows, epochs, coefs, params, state, n_params, lr, betas, eps, max_grad_norm, seed, stats,
                     symmetric=False) -> dict:
        """ppo_update() / distill_update() behind the check of their storage: the optimiser's and the loop's own checks, the statistics
        [epochs * M, 8] and the call `fn(*data, n_rows, minibatch_rows, epochs, *coefs, adam_step's arguments, seed, stats)`"""
        n_params = _ro.adam_args(self.policy, self.device, params, None, state, n_params, lr, betas, eps, max_grad_norm)
        per_epoch = _ro.update_args(n_rows, minibatch_rows, epochs, seed, stats, self.device, symmetric=symmetric)
        if stats is None:
            stats = torch.empty(int(epochs) * per_epoch, 8, dtype=torch.float32, device=self.device)
        self._call(fn, *data, n_rows, int(minibatch_rows), int(epochs), *coefs, params, params.numel(), n_params, state.moments, state.clock,
                   float(lr), float(betas[0]), float(betas[1]), float(eps), float(max_grad_norm), int(seed), stats)
        return {"stats": stats.view(int(epochs) * per_epoch, 8)}

    # ---- teacher-student distillation on the device (include/mocca.h mocca_distill_grad / mocca_distill_update / mocca_set_teacher ..) ----
    def _no_mirror(self, name: str) -> None:
        if self.policy is None:
            raise _lib.MoccaError(f"{name} needs a policy (set_policy)")
        if self._mirrored:
            raise _lib.MoccaError(f"{name}: the policy has a mirror attachment (symmetry, mirror loss or duplicated rows): detach it first")
        if getattr(self.policy, "asymmetric", False):
            raise _lib.MoccaError(f"{name}: the policy has a privileged critic: distilling into an asymmetric student is not provided")

    def distill_grad(self, obs: torch.Tensor, target: torch.Tensor, value_target: Optional[torch.Tensor] = None,
                     idx: Optional[torch.Tensor] = None, distill_coef: float = 1.0, value_coef: float = 0.5,
                     grad: Optional[torch.Tensor] = None, stats: Optional[torch.Tensor] = None) -> dict:
        """A regression minibatch step (behaviour cloning, DAgger) as `ppo_grad`'s four launches: the gradient of
        `distill_coef * (mean - target).pow(2).mean() + value_coef * 0.5 * (value - value_target).pow(2).mean()` with respect to every
        parameter of the attached PLAIN policy -> {"grad" [policy.n_head()], "stats" [8]: 0, value loss, entropy, 0, 0, sum of grad^2, 0,
        L_d = mean squared error of the actor's mean}.  `obs` and `idx` as in `ppo_grad`; `target` [.., act_dim] and `value_target` ([..] or
        [.., 1], None: the critic gets no gradient) contiguous float32 of the same R rows.  log_std's gradient is exactly 0.  The same
        inputs give the same bits on every run."""
        self._no_mirror("distill_grad")
        _, stride, n_batch = _ro.distill_args(self.policy, self.device, obs, target, value_target, idx, distill_coef, value_coef, grad, stats)
        out = self._grad_out(grad, stats)
        self._call(self.lib.mocca_distill_grad, obs, stride, target, value_target, idx, n_batch, float(distill_coef), float(value_coef),
                   out["grad"], out["stats"])
        return out

    def distill_update(self, obs: torch.Tensor, target: torch.Tensor, params: torch.Tensor, state, minibatch_rows: int, epochs: int,
                       value_target: Optional[torch.Tensor] = None, distill_coef: float = 1.0, value_coef: float = 0.5,
                       n_params: Optional[int] = None, lr: float = 3e-4, betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-5,
                       max_grad_norm: float = 0.5, seed: int = 0, stats: Optional[torch.Tensor] = None) -> dict:
        """`ppo_update`'s loop around `distill_grad`: `epochs` passes over the R stored rows, each a fresh shuffle cut into
        M = R // minibatch_rows minibatches (the remainder is dropped), each minibatch `distill_grad` on its rows and `adam_step` on
        `params` -- the same bits as that loop.  -> {"stats": [epochs * M, 8]}: `distill_grad`'s statistics per minibatch, [6] the clip
        coefficient applied.  Nothing synchronises or is read on the host; capturable after one warm call of the same shapes."""
        self._no_mirror("distill_update")
        n_rows, stride, _ = _ro.distill_args(self.policy, self.device, obs, target, value_target, None, distill_coef, value_coef, None, None)
        return self._update_loop(self.lib.mocca_distill_update, (obs, stride, target, value_target), n_rows, minibatch_rows, epochs,
                                 (float(distill_coef), float(value_coef)), params, state, n_params, lr, betas, eps, max_grad_norm, seed, stats)

    def set_teacher(self, policy) -> None:
        """Attach a frozen `policy.DevicePolicy` as the TEACHER (None detaches): a second image beside the policy of set_policy, which it
        may differ from in in_dim and layers; its weights are uploaded (update_teacher).  A policy carrying `symmetry` is refused.  The
        attached policy, its mirror attachment, act() and the gradient calls are untouched.  May synchronise."""
        if getattr(policy, "symmetry", None) is not None:
            raise ValueError("set_teacher: the teacher is a plain policy; one carrying `symmetry` is not supported")
        self._set_slot(self.lib.mocca_set_teacher, policy)
        self.teacher = policy
        if policy is not None:
            self.update_teacher(policy)

    def update_teacher(self, params) -> None:
        """New weights for the teacher: a `DevicePolicy` of the same shapes or a flat float32 tensor, as `update_policy` takes them."""
        if self.teacher is None:
            raise _lib.MoccaError("update_teacher needs a teacher (set_teacher)")
        self._update_slot(self.lib.mocca_update_teacher, params)

    def teacher_act(self, rows: torch.Tensor, mean: Optional[torch.Tensor] = None, value: Optional[torch.Tensor] = None) -> dict:
        """The teacher's actor mean and value on `rows` [n, >= teacher.in_dim] (float32 on the env's device, contiguous last dimension; any
        n >= 1) in one launch -> {"mean" [n, act_dim], "value" [n]}.  `mean` / `value`: caller-owned outputs (rows of a storage);
        allocated where none is given.  Nothing synchronises."""
        t = self.teacher
        if t is None:
            raise _lib.MoccaError("teacher_act needs a teacher (set_teacher)")
        stride = _ro.row_view("the teacher's input", rows, t.in_dim, None, self.device)
        n = rows.shape[0]
        f32 = dict(dtype=torch.float32, device=self.device)
        mean = torch.empty(n, t.act_dim, **f32) if mean is None else mean
        value = torch.empty(n, **f32) if value is None else value
        _ro.stats_out("mean", mean, n * t.act_dim, self.device)
        _ro.stats_out("value", value, n, self.device)
        self._call(self.lib.mocca_teacher_act, rows, stride, n, mean, value)
        return {"mean": mean, "value": value}

    # ---- the reference's env-level setters, batched (env_base.py:103-118, env_locomotion.py:76-77,224-282) ----
    def set_env_params(self, params_dict):
        """`set_env_params({"curriculum": k})`: one value for all envs or one per env (takes effect at each env's next reset; the
        terminal height follows it at once, env_locomotion.py:628).  Unknown keys are ignored, like the reference's hasattr test."""
        for k, v in params_dict.items():
            if k == "curriculum":
                if np.ndim(v) == 0:
                    self.set_param(_lib.PARAM_CURRICULUM, float(v))
                else:
                    self.set_param_v(_lib.PARAM_CURRICULUM, v)

    def set_robot_params(self, params_dict):
        """`set_robot_params({"applied_gain": g})` (env_base.py:108-115): scalar or one value per env; acts on the next apply_action."""
        if "applied_gain" in params_dict:
            g = params_dict["applied_gain"]
            if np.ndim(g) == 0:
                self.set_param(_lib.PARAM_APPLIED_GAIN, float(g))
            else:
                self.set_param_v(_lib.PARAM_APPLIED_GAIN, g)

    def evaluation_mode(self, on=True):
        """Walker3DCustomEnv.evaluation_mode() (env_locomotion.py:76-77): fixed target 4 m ahead; scalar or one flag per env."""
        if np.ndim(on) == 0:
            self.set_param(_lib.PARAM_EVAL_MODE, 1.0 if on else 0.0)
        else:
            self.set_param_v(_lib.PARAM_EVAL_MODE, on)

    def get_mirror_indices(self):
        """The six index lists SymmetricRL consumes (env_locomotion.py:224-282 / :761-840); see symmetry.MirrorTransform."""
        from . import host_logic as H
        if self.task_id == M.TASK_CASSIE:
            # the Cassie mocap / phase envs publish a DICT of index lists as a class attribute (env_cassie.py:536-571, :627-629), not the walkers'
            # six-tuple; CassieEnv itself publishes nothing
            if self.model.cassie_mode == M.CASSIE_PLAIN:
                raise NotImplementedError("CassieEnv has no mirror indices in the reference (env_cassie.py:284-479)")
            import copy
            from .envs import CassieMoccaEnv
            mi = copy.deepcopy(CassieMoccaEnv.mirror_indices)
            mi["left_obs_inds"] += [40]
            mi["right_obs_inds"] += [41]
            return mi
        return H.mirror_indices(self.model, stepper=self.task_id == M.TASK_WALKER3D_STEPPER)

    def set_param_v(self, pid: int, values, broadcast: bool = False):
        """Per-env curriculum / eval_mode / applied_gain (include/mocca.h mocca_set_param_v); values: [N] (or [1] with broadcast)."""
        v = torch.as_tensor(values, dtype=torch.float32).to(self.device).contiguous().reshape(-1)
        if v.numel() != (1 if broadcast else self.n_envs):
            raise ValueError("values must hold one float per env (or one float with broadcast=True)")
        self._call(self.lib.mocca_set_param_v, pid, v, int(broadcast))       # `v` may be freed (and its memory reused on the current stream) as soon as this returns

    def seed(self, seed: int, rewind: bool = True):
        """Philox key of the in-kernel draws (gym's env.seed(s), env_base.py:164-166).  With rewind (default) the per-env episode
        counters go back to "before the first episode", so that seed(s) followed by reset() replays exactly what a fresh VecEnv created
        with seed=s produces -- the gym contract.  rewind=False only re-keys the stream: the envs continue with new random numbers."""
        self.seed_value = int(seed) & 0xFFFFFFFFFFFFFFFF
        _lib.check(self.lib.mocca_set_seed(self.h, self.seed_value), self.h)
        if rewind:
            tk = self.get_task()
            tk[:, M.TW.EPISODE] = -1   # the next reset is episode 0 (draws are keyed by (seed, global env id, episode, draw))
            tk[:, M.TW.DRAW] = 0
            self.set_task(tk)
        return [seed]

    def set_draw_tape(self, tape) -> None:
        """Uniforms that replace the Philox draws of reset() / task_step(), [N][n] (None detaches); golden replays only."""
        if tape is None:
            self._tape = None
            _lib.check(self.lib.mocca_set_draw_tape(self.h, None, 0), self.h)
            return
        self._tape = torch.as_tensor(tape, dtype=torch.float32).to(self.device).contiguous().reshape(self.n_envs, -1)
        _lib.check(self.lib.mocca_set_draw_tape(self.h, C.c_void_p(self._tape.data_ptr()), self._tape.shape[1]), self.h)

    def keep_terminal_obs(self, on: bool = True, buffer: Optional[torch.Tensor] = None) -> Optional[torch.Tensor]:
        """Attach (or detach) the terminal-observation buffer [N][obs_dim] (include/mocca.h mocca_set_terminal_obs_buffer); `buffer`:
        a caller-owned contiguous float32 [N][obs_dim] tensor on the device (e.g. this handle's rows of a larger batch's buffer)."""
        if on and buffer is not None:
            if buffer.shape != (self.n_envs, self.obs_dim) or buffer.dtype != torch.float32 or not buffer.is_contiguous() or buffer.device != self.device:
                raise ValueError("terminal-observation buffer must be a contiguous float32 [n_envs, obs_dim] tensor on the env's device")
            self.terminal_obs = buffer
        else:
            self.terminal_obs = torch.zeros(self.n_envs, self.obs_dim, dtype=torch.float32, device=self.device) if on else None
        _lib.check(self.lib.mocca_set_terminal_obs_buffer(self.h, C.c_void_p(self.terminal_obs.data_ptr()) if on else None), self.h)
        return self.terminal_obs

    def episode_stats(self, on: bool = True, slots: int = 4, masks=None, bad_masks=None, totals=None, records=None, row0: int = 0) -> Optional[dict]:
        """Monitor + TimeLimitMask inside the launch (include/mocca.h mocca_set_episode_stats): per step and env the PPO loop's `masks` /
        `bad_masks` columns (float32 [N] on the device, 0.0 where the episode ended / ended with the TimeLimit bit), device-side `totals`
        [4] (sums of return, length, episodes, truncated episodes) and, for the envs that finished, a 16-byte record {serial, return,
        length, done bits | info << 8} written by the kernel straight into PINNED HOST memory: `records` int32 [slots][N][4], the k-th
        step() after this call (k = 1, 2, ...) writes slot k % slots with serial k.  Nothing is copied and nothing synchronises; read a
        slot after the stream work of its step has completed.  The four buffers are allocated here unless passed in (a sub-batch gets
        its rows of a whole batch's buffers: `records` is then the whole ring and `row0` this handle's first row).  on=False detaches."""
        if not on:
            _lib.check(self.lib.mocca_set_episode_stats(self.h, None, None, None, None, 0, 0), self.h)
            self.ep = None
            return None
        n = self.n_envs
        f32 = dict(dtype=torch.float32, device=self.device)
        masks = torch.ones(n, **f32) if masks is None else masks
        bad_masks = torch.ones(n, **f32) if bad_masks is None else bad_masks
        totals = torch.zeros(4, **f32) if totals is None else totals
        if records is None:
            records = torch.zeros(int(slots), n, 4, dtype=torch.int32).pin_memory()
        for t, shape in ((masks, (n,)), (bad_masks, (n,)), (totals, (4,))):
            if tuple(t.shape) != shape or t.dtype != torch.float32 or not t.is_contiguous() or t.device != self.device:
                raise ValueError("episode_stats: masks / bad_masks must be contiguous float32 [n_envs] and totals float32 [4] on the env's device")
        if records.dim() != 3 or records.shape[2] != 4 or records.dtype != torch.int32 or not records.is_contiguous() or \
                row0 < 0 or row0 + n > records.shape[1] or not (records.is_cuda or records.is_pinned()):
            raise ValueError("episode_stats: records must be a contiguous int32 [slots][rows >= row0 + n_envs][4] tensor in pinned host (or device) memory")
        self._sync()      # no launch of this handle is in flight while its buffers change
        _lib.check(self.lib.mocca_set_episode_stats(self.h, C.c_void_p(masks.data_ptr()), C.c_void_p(bad_masks.data_ptr()), C.c_void_p(totals.data_ptr()),
                                                    C.c_void_p(records.data_ptr() + 16 * row0), records.shape[0], 16 * records.shape[1]), self.h)
        self.ep = dict(masks=masks, bad_masks=bad_masks, totals=totals, records=records, row0=row0, slots=records.shape[0],
                       first_serial=int(self.lib.mocca_episode_serial(self.h)))
        return self.ep

    def set_debug(self, on: bool = True) -> Optional[torch.Tensor]:
        """Attach (or detach) the per-env debug record: [N][16] int32, words MOCCA_DBG_* (0..11 the active set of the last substep
        incl. the solver's clamp mask / signature, 12..15 cumulative cap pressure: zero the tensor to restart the count)."""
        self.debug = torch.zeros(self.n_envs, _lib.DEBUG_WORDS, dtype=torch.int32, device=self.device) if on else None
        _lib.check(self.lib.mocca_set_debug_buffer(self.h, C.c_void_p(self.debug.data_ptr()) if on else None), self.h)
        return self.debug

    def task_step(self, actions: torch.Tensor, touch, target=None, body=None):
        """env.step()'s task layer on the stored (post-physics) state with caller-supplied contact flags
        (include/mocca.h mocca_task_step): the golden replays of the reference's scripted episodes."""
        actions = actions.to(device=self.device, dtype=torch.float32).contiguous()
        i32 = lambda x: None if x is None else torch.as_tensor(x, dtype=torch.int32).to(self.device).contiguous()
        touch, target, body = i32(touch), i32(target), i32(body)
        self._call(self.lib.mocca_task_step, actions, touch, target, body, self.obs, self.rew, self.done, self.info,
                   then="sync")   # the int32 temporaries above must outlive the launch
        return self.obs, self.rew, self.done, self.info

    def reset(self, mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        if mask is not None:
            mask = mask.to(device=self.device, dtype=torch.uint8).contiguous()
        self._call(self.lib.mocca_reset, mask, self.seed_value, self.obs)
        return self.obs

    def step(self, actions: torch.Tensor, obs_out: Optional[torch.Tensor] = None,
             rew_out: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
        """One env.step of all envs: one kernel launch on torch's current stream (or on `self.stream`, unordered against the current
        stream: see _in / _out above).  `obs_out` / `rew_out`: where THIS launch writes its observations [N, obs_dim] / rewards [N] (or
        [N, 1]) instead of `self.obs` / `self.rew` -- e.g. row t + 1 of a trainer's rollout storage, which PPO reads the next policy input
        from anyway: the kernel's outputs need no copy (mocca_step takes the pointers per call).  Contiguous float32 on the env's device."""
        return self._launch_step(self.lib.mocca_step, actions, self.act_dim, "actions", obs_out, rew_out)

    def _launch_step(self, entry, actions, width, what, obs_out, rew_out):
        """step() / plan_step(): check the tensors, launch `entry` (mocca_step or mocca_plan_step: same argument list)"""
        if actions.device != self.device or actions.dtype != torch.float32 or not actions.is_contiguous():
            actions = actions.to(device=self.device, dtype=torch.float32).contiguous()
        if actions.shape != (self.n_envs, width):
            raise ValueError(f"{what} must be [{self.n_envs}, {width}]")
        obs, rew = (self.obs, self.rew) if obs_out is None and rew_out is None else self._step_out(obs_out, rew_out)
        _lib.check(entry(self.h, C.c_void_p(actions.data_ptr()), C.c_void_p(obs.data_ptr()),
                         C.c_void_p(rew.data_ptr()), C.c_void_p(self.done.data_ptr()),
                         C.c_void_p(self.info.data_ptr()), self._stream()), self.h)
        return obs, rew, self.done, self.info

    def _step_out(self, obs_out, rew_out):
        """step() / plan_step() / act_step() / act_plan_step() with `obs_out` or `rew_out`: check them -> where the launch writes (obs, rew)"""
        obs, rew = self.obs if obs_out is None else obs_out, self.rew if rew_out is None else rew_out
        if obs.shape != (self.n_envs, self.obs_dim) or rew.numel() != self.n_envs or obs.dtype != torch.float32 or rew.dtype != torch.float32 \
                or not obs.is_contiguous() or not rew.is_contiguous() or obs.device != self.device or rew.device != self.device:
            raise ValueError("obs_out / rew_out must be contiguous float32 [n_envs, obs_dim] / [n_envs] tensors on the env's device")
        return obs, rew

    def episode_masks_into(self, masks: torch.Tensor, bad_masks: torch.Tensor) -> None:
        """Point the in-kernel `masks` / `bad_masks` columns of episode_stats() at other buffers FROM THE NEXT LAUNCH ON (e.g. row t + 1 of a
        trainer's rollout storage); totals and records stay where they are.  No synchronisation: launches in flight keep the pointers they
        were issued with.  Contiguous float32, n_envs elements each, on the env's device."""
        if self.ep is None:
            raise _lib.MoccaError("episode_masks_into needs episode_stats(True) first")
        for t in (masks, bad_masks):
            if t.numel() != self.n_envs or t.dtype != torch.float32 or not t.is_contiguous() or t.device != self.device:
                raise ValueError("masks / bad_masks must be contiguous float32 tensors of n_envs elements on the env's device")
        r = self.ep["records"]
        _lib.check(self.lib.mocca_set_episode_stats(self.h, C.c_void_p(masks.data_ptr()), C.c_void_p(bad_masks.data_ptr()),
                                                    C.c_void_p(self.ep["totals"].data_ptr()), C.c_void_p(r.data_ptr() + 16 * self.ep["row0"]),
                                                    r.shape[0], 16 * r.shape[1]), self.h)

    # ---- host-side callers (the single-env gym classes; a trainer that lives on the host) ----
    def host_mirror(self) -> dict:
        """Lay obs / rew / info / state / task / done out in ONE device buffer with ONE pinned host image, so that a caller on the host
        pays one upload, one download and one synchronize per step (`step_host`) instead of one blocking copy per quantity.  The
        tensors `obs`, `rew`, `done`, `info` become views into that buffer.  Returns the numpy views of the host image."""
        if self._host_np is not None:
            return self._host_np
        n = self.n_envs
        parts = [("obs", n * self.obs_dim, torch.float32, np.float32, (n, self.obs_dim)), ("rew", n, torch.float32, np.float32, (n,)),
                 ("info", n, torch.int32, np.int32, (n,)), ("state", n * self.state_dim, torch.float32, np.float32, (n, self.state_dim)),
                 ("task", n * M.TASK_WORDS, torch.int32, np.int32, (n, M.TASK_WORDS))]
        words = sum(p[1] for p in parts)
        total = 4 * words + ((n + 3) // 4) * 4
        self._pack = torch.zeros(total, dtype=torch.uint8, device=self.device)
        self._pack_host = torch.zeros(total, dtype=torch.uint8).pin_memory()
        host = self._pack_host.numpy()
        dev, hnp, off = {}, {}, 0
        for name, cnt, tdt, ndt, shape in parts:
            dev[name] = self._pack[off:off + 4 * cnt].view(tdt).view(*shape)
            hnp[name] = host[off:off + 4 * cnt].view(ndt).reshape(shape)
            off += 4 * cnt
        dev["done"], hnp["done"] = self._pack[off:off + n], host[off:off + n]
        dev["obs"].copy_(self.obs); dev["rew"].copy_(self.rew); dev["info"].copy_(self.info); dev["done"].copy_(self.done)
        self.obs, self.rew, self.info, self.done = dev["obs"], dev["rew"], dev["info"], dev["done"]
        self._dev_views = dev
        self._act_host = torch.zeros(n, self.act_dim, dtype=torch.float32).pin_memory()
        self._act_dev = torch.zeros(n, self.act_dim, dtype=torch.float32, device=self.device)
        self._host_np = hnp
        return hnp

    def _download(self) -> dict:
        d = self._dev_views
        self._call(self.lib.mocca_get_state, d["state"], wait=False, then=None)    # (behind the step / reset / observe that the caller issued)
        self._call(self.lib.mocca_get_task, d["task"], wait=False)
        self._pack_host.copy_(self._pack, non_blocking=True)
        torch.cuda.current_stream(self.device).synchronize()
        return self._host_np

    def step_host(self, actions_np) -> dict:
        """step() for a caller on the host: float32 actions [n_envs, act_dim] in, the host image (obs, rew, done, info AND the state /
        task records after the step) out -- valid until the next call.  One synchronize."""
        hnp = self.host_mirror()
        self._act_host.numpy()[...] = actions_np
        self._act_dev.copy_(self._act_host, non_blocking=True)
        self._in()
        self.step(self._act_dev)
        return self._download()

    def reset_host(self) -> dict:
        self.host_mirror()
        self.reset()
        return self._download()

    def observe_host(self) -> dict:
        self.host_mirror()
        self.observe()
        return self._download()

    def observe(self) -> torch.Tensor:
        """calc_state() + observation tail of the current state, no stepping (include/mocca.h mocca_observe)."""
        self._call(self.lib.mocca_observe, self.obs)
        return self.obs

    # ---- snapshots (saveState/restoreState role; used by the parity tests) ----
    def get_state(self) -> torch.Tensor:
        st = torch.empty(self.n_envs, self.state_dim, dtype=torch.float32, device=self.device)
        self._call(self.lib.mocca_get_state, st)      # (waits first: st's memory may have been in use on the current stream a moment ago)
        return st

    def set_state(self, st) -> None:
        st = torch.as_tensor(st, dtype=torch.float32).to(self.device).contiguous().reshape(self.n_envs, self.state_dim)
        self._call(self.lib.mocca_set_state, st, then="sync")

    def get_task(self) -> torch.Tensor:
        t = torch.empty(self.n_envs, M.TASK_WORDS, dtype=torch.int32, device=self.device)
        self._call(self.lib.mocca_get_task, t)
        return t

    def set_task(self, t: torch.Tensor) -> None:
        t = t.to(device=self.device, dtype=torch.int32).contiguous().reshape(self.n_envs, M.TASK_WORDS)
        self._call(self.lib.mocca_set_task, t, then="sync")

    def get_terrain(self) -> torch.Tensor:
        t = torch.empty(self.n_envs, 128, dtype=torch.float32, device=self.device)
        self._call(self.lib.mocca_get_terrain, t)
        return t

    def set_terrain(self, t) -> None:
        t = torch.as_tensor(t, dtype=torch.float32).to(self.device).contiguous().reshape(self.n_envs, 128)
        self._call(self.lib.mocca_set_terrain, t, then="sync")

    # ---- where the links are, what an env looks like (include/mocca.h mocca_get_link_frames / mocca_render) ----
    def link_frames(self, envs=None) -> torch.Tensor:
        """Link frames of the current state, [N (or len(envs))][n_bodies][15] float32 on the device: per body R (9, row-major,
        world <- body), origin in world (3), centre of mass in world (3) -- the order of the oracle's link_frames.  One small kernel;
        nothing synchronises."""
        fr = torch.empty(self.n_envs, int(self.model.n_bodies), 15, dtype=torch.float32, device=self.device)
        self._call(self.lib.mocca_get_link_frames, fr)
        if envs is None:
            return fr
        return fr[torch.as_tensor(envs, dtype=torch.long).to(self.device)]

    def render(self, envs, camera=None, width: int = 320, height: int = 240, depth: bool = False, ids: bool = False):
        """Ray-cast the listed envs (an env may be listed more than once): rgb uint8 [K][height][width][3] on the device, or the tuple
        (rgb, depth float32 [K][H][W] if depth, ids int32 [K][H][W] if ids).  `camera`: one render.Camera for all views, a
        [K][CAMERA_FLOATS] tensor of records, or None: a follow camera (render.Camera's defaults) per env that looks at the env's base
        position, which is read and turned into camera records on the device.  An env index out of range raises MoccaError."""
        from . import render as R
        ev = torch.as_tensor(envs, dtype=torch.int32).reshape(-1).to(self.device).contiguous()
        k = int(ev.numel())
        if k < 1:
            raise ValueError("render: envs must list at least one env")
        width, height = int(width), int(height)
        if not (1 <= width <= _lib.RENDER_MAX_SIZE and 1 <= height <= _lib.RENDER_MAX_SIZE):   # (before the output tensors are sized by them)
            raise _lib.MoccaError(f"render: width and height must be 1 .. {_lib.RENDER_MAX_SIZE}")
        if camera is None or isinstance(camera, R.Camera):
            if camera is None:
                pos = self.get_state()[ev.long().clamp(0, self.n_envs - 1), 0:3]   # (the library refuses ids out of range below)
                cams = R.follow_cameras(pos, width / height)
            else:
                cams = torch.from_numpy(camera.pack(width / height)).to(self.device).repeat(k, 1).contiguous()
        else:
            cams = torch.as_tensor(camera, dtype=torch.float32).to(self.device).contiguous()
            if tuple(cams.shape) != (k, _lib.CAMERA_FLOATS):
                raise ValueError(f"camera records must be [{k}, {_lib.CAMERA_FLOATS}]")
        rgb = torch.empty(k, height, width, 3, dtype=torch.uint8, device=self.device)
        dep = torch.empty(k, height, width, dtype=torch.float32, device=self.device) if depth else None
        idt = torch.empty(k, height, width, dtype=torch.int32, device=self.device) if ids else None
        self._call(self.lib.mocca_render, ev, k, cams, int(width), int(height), rgb, dep, idt)
        if not depth and not ids:
            return rgb
        return tuple(x for x in (rgb, dep, idt) if x is not None)

    # ---- the terrain height scan (include/mocca.h mocca_set_height_scan / mocca_height_scan) ----
    @property
    def scan_dim(self) -> int:
        """points of the attached scan pattern, 0 when there is none"""
        return int(self.lib.mocca_scan_dim(self.h))

    def set_height_scan(self, points, z_above: float = 1.0, max_drop: float = 2.0) -> None:
        """Attach the pattern of the height scan: `points` [P, 2] metres in the heading frame (x ahead, y to the left; perception.scan_grid
        builds grids), 1 <= P <= 256; the rays start `z_above` over the base and see `max_drop` below it.  None detaches.  The points
        are copied into the handle; may synchronise."""
        if points is None:
            _lib.check(self.lib.mocca_set_height_scan(self.h, None, 0, 0.0, 0.0), self.h)
            self._scan_points = None
            return
        pts = np.ascontiguousarray(points.detach().cpu().numpy() if isinstance(points, torch.Tensor) else points, np.float32)
        if pts.ndim != 2 or pts.shape[1] != 2:
            raise ValueError("height-scan points must be [P, 2]")
        _lib.check(self.lib.mocca_set_height_scan(self.h, pts.ctypes.data_as(C.c_void_p), pts.shape[0], float(z_above), float(max_drop)), self.h)
        self._scan_points = pts.copy()       # symmetric_policy() mirrors the pattern

    def height_scan(self, out: Optional[torch.Tensor] = None, obs: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Terrain heights under the pattern, relative to the base, of the state the handle holds: float32 [N, P] on the device, one launch,
        nothing synchronises.  With `obs` (contiguous float32 [N, obs_dim] on the device, e.g. what step() just returned) the rows are
        [obs | scan], [N, obs_dim + P], written by the same launch.  `out`: where to write -- a float32 [N, >= width] tensor on the device
        whose rows are contiguous (a view of wider storage will do: floats of a row beyond `width` are left untouched; it must not overlap
        `obs`); returned, narrowed to the width written."""
        p = self.scan_dim
        if p == 0:
            raise _lib.MoccaError("height_scan needs a pattern (set_height_scan)")
        return self._sensor_rows(self.lib.mocca_height_scan, p, out, obs)

    def _sensor_rows(self, fn, width: int, out, obs, *extra) -> torch.Tensor:
        """height_scan() / depth_camera(): check `obs` and `out` (allocated where none is given) for a sensor of `width` floats, launch
        `fn(out, row stride, obs, *extra)` -> `out`, narrowed to the width written"""
        if obs is not None:
            if obs.shape != (self.n_envs, self.obs_dim) or obs.dtype != torch.float32 or not obs.is_contiguous() or obs.device != self.device:
                raise ValueError("obs must be a contiguous float32 [n_envs, obs_dim] tensor on the env's device")
            width += self.obs_dim
        if out is None:
            out = torch.empty(self.n_envs, width, dtype=torch.float32, device=self.device)
        self._call(fn, out, self._rows("out", out, width), obs, *extra)
        return out if out.shape[1] == width else out[:, :width]

    # ---- the egocentric depth camera (include/mocca.h mocca_set_depth_camera / mocca_depth_camera) ----
    @property
    def depth_dim(self) -> int:
        """pixels of the attached depth camera, 0 when there is none"""
        return int(self.lib.mocca_depth_dim(self.h))

    @property
    def depth_shape(self):
        """(height, width) of the attached depth camera, None when there is none"""
        return None if self._depth_cam is None else self._depth_cam.shape

    def set_depth_camera(self, cam) -> None:
        """Attach a `perception.DepthCamera` (None detaches).  Nothing is allocated and nothing synchronises."""
        if cam is None:
            _lib.check(self.lib.mocca_set_depth_camera(self.h, 0, None, 0, 0, 0.0, 0.0, 0.0, 0), self.h)
            self._depth_cam = None
            return
        a = cam.pack()
        mount = np.ascontiguousarray(a["mount"], np.float32)
        _lib.check(self.lib.mocca_set_depth_camera(self.h, a["body"], mount.ctypes.data_as(C.c_void_p), a["width"], a["height"], a["fov_y"],
                                                   a["near"], a["far"], a["flags"]), self.h)
        self._depth_cam = cam                # symmetric_policy() mirrors the image

    def depth_camera(self, out: Optional[torch.Tensor] = None, obs: Optional[torch.Tensor] = None,
                     cameras_out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The depth image of the state the handle holds: float32 [N, H * W] on the device (row e reshapes to depth_shape), one launch,
        nothing synchronises.  `out` and `obs` as in height_scan(): with `obs` the rows are [obs | depth].  `cameras_out`: a contiguous
        float32 [N, CAMERA_FLOATS] tensor on the device that receives the camera records the rays were cast from (render() takes them)."""
        p = self.depth_dim
        if p == 0:
            raise _lib.MoccaError("depth_camera needs a camera (set_depth_camera)")
        if cameras_out is not None and (tuple(cameras_out.shape) != (self.n_envs, _lib.CAMERA_FLOATS) or cameras_out.dtype != torch.float32
                                        or not cameras_out.is_contiguous() or cameras_out.device != self.device):
            raise ValueError(f"cameras_out must be a contiguous float32 [n_envs, {_lib.CAMERA_FLOATS}] tensor on the env's device")
        return self._sensor_rows(self.lib.mocca_depth_camera, p, out, obs, cameras_out)

    # ---- domain randomisation (include/mocca.h mocca_set_randomisation .. mocca_randomisation_record; randomisation.Randomisation) ----
    def set_randomisation(self, rand) -> None:
        """Attach a `randomisation.Randomisation` (None detaches both parts): its strength, latency and pushes act in front of every step
        from the next one on (step, plan_step, act_step, act_plan_step: one more small launch each), its `obs_noise` becomes the scales of
        sensor_noise().  May allocate and synchronise; no step does."""
        if rand is None:
            _lib.check(self.lib.mocca_set_randomisation(self.h, None), self.h)
            _lib.check(self.lib.mocca_set_sensor_noise(self.h, None, 0), self.h)
            self.randomisation = None
            return
        scales = rand.noise_scales(self.obs_dim)      # (refused before the handle changes)
        cfg = rand.config()
        _lib.check(self.lib.mocca_set_randomisation(self.h, C.byref(cfg)), self.h)
        self.set_sensor_noise(scales)
        self.randomisation = rand

    def effective_action(self) -> torch.Tensor:
        """what the last step's kernel read in place of the action: float32 [N, act_dim] (the clipped action times the episode's strength,
        `delay` steps late)"""
        out = torch.empty(self.n_envs, self.act_dim, dtype=torch.float32, device=self.device)
        self._call(self.lib.mocca_get_effective_action, out)
        return out

    def set_sensor_noise(self, scales) -> None:
        """the scales of sensor_noise(): one per observation column, float32 [obs_dim] >= 0, copied into the handle; None detaches"""
        if scales is None:
            _lib.check(self.lib.mocca_set_sensor_noise(self.h, None, 0), self.h)
            return
        s = np.ascontiguousarray(scales.detach().cpu().numpy() if isinstance(scales, torch.Tensor) else scales, np.float32).reshape(-1)
        _lib.check(self.lib.mocca_set_sensor_noise(self.h, s.ctypes.data_as(C.c_void_p), int(s.size)), self.h)

    def sensor_noise(self, rows: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """`rows` [N, >= obs_dim] with uniform noise of the attached scales added to the first obs_dim columns, one launch, nothing
        synchronises: into `out` (float32 [N, >= obs_dim] with contiguous rows; columns beyond obs_dim are left untouched), or IN PLACE
        without one.  The noise is keyed by the envs' step and episode counters: two calls without a step in between add the same noise."""
        out = rows if out is None else out
        self._call(self.lib.mocca_sensor_noise, rows, self._rows("rows", rows, self.obs_dim), out, self._rows("out", out, self.obs_dim))
        return out

    def randomisation_record(self, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The plant each env has in the episode it is in now: float32 [N, 4] -- strength, delay, steps until the next push (-1: none),
        0 --, one launch.  `out`: a float32 [N, >= 4] tensor with contiguous rows (the tail of a privileged row); returned narrowed to 4."""
        w = _lib.RAND_WORDS
        if out is None:
            out = torch.empty(self.n_envs, w, dtype=torch.float32, device=self.device)
        self._call(self.lib.mocca_randomisation_record, out, self._rows("out", out, w))
        return out if out.shape[1] == w else out[:, :w]

    # ---- the observation-action history (include/mocca.h mocca_set_history / mocca_history; history.History) ----
    def set_history(self, hist) -> None:
        """Attach a `history.History` (None detaches): history() then writes the last `steps` pairs [obs[columns] | action] of every env,
        newest first.  `actions=True` takes this env's action width -- the plan's on a planner env with its base controller.  May allocate
        and synchronise; history() never does."""
        if hist is None:
            _lib.check(self.lib.mocca_set_history(self.h, None, 0, 0, 0, 0), self.h)
            self.hist, self._hist_cols, self._hist_act = None, None, 0
            return
        plan = getattr(self, "base_controller", None) is not None
        cols, a = hist.resolve(self.obs_dim, self.plan_dim if plan else self.act_dim)      # (refused before the handle changes)
        _lib.check(self.lib.mocca_set_history(self.h, cols.ctypes.data_as(C.c_void_p), int(cols.size), a, hist.steps, hist.stride), self.h)
        self.hist, self._hist_cols, self._hist_act = hist, cols, a

    @property
    def history_dim(self) -> int:
        """floats of the attached history's block, steps * (columns + actions); 0 when there is none"""
        return 0 if self.hist is None else int(self.lib.mocca_history_dim(self.h))

    def history(self, rows: torch.Tensor, act: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Store the frame of `rows` (float32 [N, >= obs_dim] with contiguous rows: what the policy reads NOW), complete the previous frame
        with `act` (float32 [N, >= the history's action width]: the action the policy output on the previous row; None after a reset) and
        write the block [N, history_dim], newest pair first, one launch, nothing synchronises: into `out` (float32 [N, >= history_dim] with
        contiguous rows -- a view of the tail of `rows` itself will do; floats beyond the block are left untouched), or into a new tensor.
        Keyed by the envs' step and episode counters: two calls without a step in between write and return the same words."""
        if self.hist is None:
            raise _lib.MoccaError("history needs a History (set_history)")
        w, n = self.history_dim, self.n_envs
        if out is None:
            out = torch.empty(n, w, dtype=torch.float32, device=self.device)
        self._call(self.lib.mocca_history, rows, self._rows("rows", rows, self.obs_dim), act,
                   0 if act is None else self._rows("act", act, self._hist_act), out, self._rows("out", out, w))
        return out if out.shape[1] == w else out[:, :w]

    # ---- the per-env adaptive curriculum (include/mocca.h mocca_set_curriculum .. mocca_curriculum_apply; curriculum.Curriculum) ----
    def set_curriculum(self, cfg, totals: Optional[torch.Tensor] = None) -> Optional[torch.Tensor]:
        """Attach a `curriculum.Curriculum` (None detaches; Stepper ids only): from the next step on every env's own episodes move its own
        level, one small launch behind each step()'s / act_step()'s kernel while auto-reset is on.  The levels start from the per-env
        levels where those are set (set_env_params with one value per env), else from the scalar level, clamped into the band.  `totals`:
        a contiguous float32 [10, 4] tensor on the env's device, per level {episodes judged, sum of steps_reached, successes, failures},
        which the caller zeroes when it likes; allocated here without one and returned.  While attached a scalar
        set_env_params({"curriculum": k}) is refused: set_param_v(PARAM_CURRICULUM, [k], broadcast=True) writes every env's level.  May
        allocate and synchronise; no step does."""
        if cfg is None:
            _lib.check(self.lib.mocca_set_curriculum(self.h, None, None), self.h)
            self.curriculum, self.curriculum_totals = None, None
            return None
        shape = (_lib.CUR_LEVELS, _lib.CUR_TOTALS)
        if totals is None:
            totals = torch.zeros(shape, dtype=torch.float32, device=self.device)
        elif tuple(totals.shape) != shape or totals.dtype != torch.float32 or not totals.is_contiguous() or totals.device != self.device:
            raise ValueError("set_curriculum: totals must be a contiguous float32 [10, 4] tensor on the env's device")
        c = cfg.config()
        self._sync()      # no launch of this handle is in flight while its buffers change
        _lib.check(self.lib.mocca_set_curriculum(self.h, C.byref(c), C.c_void_p(totals.data_ptr())), self.h)
        self.curriculum, self.curriculum_totals = cfg, totals
        return totals

    def _need_curriculum(self, who: str) -> None:
        if self.curriculum is None:
            raise _lib.MoccaError(f"{who} needs a Curriculum (set_curriculum)")

    def curriculum_levels(self, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """every env's level: int32 [N] on the device, one launch; nothing synchronises until the caller reads it"""
        return self.curriculum_state(level=out)["level"]

    def curriculum_state(self, level: Optional[torch.Tensor] = None) -> dict:
        """-> {"level", "streak", "hold"}: int32 [N] each on the device -- the level, the run of successes (> 0) or failures (< 0) at it,
        and whether the episode in flight is exempt from judgement (its level changed after it was laid out).  One launch."""
        self._need_curriculum("curriculum_state")
        i32 = dict(dtype=torch.int32, device=self.device)
        if level is not None and (level.shape != (self.n_envs,) or level.dtype != torch.int32 or not level.is_contiguous() or level.device != self.device):
            raise ValueError("the levels go to a contiguous int32 [n_envs] tensor on the env's device")
        out = {"level": torch.empty(self.n_envs, **i32) if level is None else level, "streak": torch.empty(self.n_envs, **i32),
               "hold": torch.empty(self.n_envs, **i32)}
        self._call(self.lib.mocca_get_curriculum, out["level"], out["streak"], out["hold"])
        return out

    def curriculum_apply(self, done: torch.Tensor, info: torch.Tensor) -> None:
        """The rule's launch on the caller's `done` (uint8 [N]) and `info` (int32 [N]): for loops that step with auto-reset off and count
        episode ends themselves.  With auto-reset on step() has launched it already."""
        self._need_curriculum("curriculum_apply")
        for t, dt, what in ((done, torch.uint8, "done"), (info, torch.int32, "info")):
            if not isinstance(t, torch.Tensor) or t.shape != (self.n_envs,) or t.dtype != dt or not t.is_contiguous() or t.device != self.device:
                raise ValueError(f"curriculum_apply: {what} must be a contiguous {dt} [n_envs] tensor on the env's device")
        self._call(self.lib.mocca_curriculum_apply, done, info)

    def kernel_info(self) -> dict:
        v = [C.c_int() for _ in range(5)]
        _lib.check(self.lib.mocca_kernel_info(self.h, *[C.byref(x) for x in v]), self.h)
        out = dict(vgprs=v[0].value, lds_bytes=v[2].value, scratch_bytes=v[3].value, max_blocks_per_cu=v[4].value)
        if v[1].value >= 0:      # the HIP runtime reports no scalar-register count (-1)
            out["sgprs"] = v[1].value
        return out


# task-record helpers: the device record is M.TASK_WORDS 32-bit words, floats and ints mixed (M.TASK_RECORD)
def task_to_float64(t: torch.Tensor) -> np.ndarray:
    """int32 view of the device task record -> float64 array in the oracle's get_task() layout."""
    a = (t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)).astype(np.int32)
    out = a.astype(np.float64)
    fl = a.view(np.float32)
    for w in M.TASK_FLOAT_WORDS:
        out[:, w] = fl[:, w]
    return out


def task_from_float64(a: np.ndarray) -> torch.Tensor:
    a = np.asarray(a, np.float64)
    out = a.astype(np.int32)
    fl = out.view(np.float32)
    for w in M.TASK_FLOAT_WORDS:
        fl[:, w] = a[:, w].astype(np.float32)
    return torch.from_numpy(out)
