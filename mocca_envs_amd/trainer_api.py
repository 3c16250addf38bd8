"""The vectorised env surface the reference's trainers drive, over the GPU stepper.

SymmetricRL and ALLSTEPS / SteppingStone (/root/reference/README.md:33-39) are PPO trainers in the pytorch-a2c-ppo-acktr mould: they build
`envs = make_vec_envs(env_name, seed, num_processes, log_dir)` -- N single-env processes (`gym.make(env_name)` + `Monitor` + a TimeLimit mask)
behind baselines' `ShmemVecEnv`, wrapped in `VecPyTorch` -- and then only ever touch this surface:

    obs = envs.reset()                                   # float tensor [N, obs_dim] on the trainer's device
    obs, reward, done, infos = envs.step(action)         # reward [N, 1]; done: bool array [N]; infos: N dicts
    for info in infos: info["episode"]["r"]              # Monitor's episode return / length, in the step that ends the episode
    "bad_transition" in info                             # TimeLimitMask: the episode was cut by max_episode_steps
    envs.observation_space / action_space / num_envs, envs.close()
    env.unwrapped.get_mirror_indices()                   # on a dummy env (SymmetricRL); set_env_params({"curriculum": k}) (ALLSTEPS)

`TorchVecEnv` is that surface with the N processes replaced by ONE `VecEnv` (or `SubBatchedVecEnv`), and with Monitor and the TimeLimit mask
INSIDE the step kernel (`VecEnv.episode_stats`, include/mocca.h mocca_set_episode_stats): the launch accumulates every env's episode return,
writes the PPO loop's `masks` / `bad_masks` columns on the device and, for the few envs that finished, a 16-byte record straight into pinned
host memory.  `step()` therefore is one kernel launch and one event record: no torch arithmetic, no copy, NO SYNCHRONISE.  `done` and `infos`
are lazy views of that step's records -- they wait for THAT step's launch, and only when the trainer looks at them (iterate / index /
np.asarray), and then behave like the bool array and the list of dicts of the contract above.  A loop that logs `infos` one step late
(after it has issued the next step) never lets the GPU run dry.  A trainer that wants no host traffic at all reads `envs.masks` / `envs.bad_masks`
([N, 1] float tensors on the device, what the PPO loop builds from `done` / `infos`), `envs.done` (uint8 [N], bit0 terminated, bit1
TimeLimit) and `envs.episode_totals` ([4] on the device: sums of return, length, episodes, truncated episodes since it last zeroed them),
and never touches `done` / `infos`; that loop can be captured in a `torch.cuda.CUDAGraph` (tests/test_gpu_trainer_api.py).
"""
from __future__ import annotations

import inspect
import weakref
from collections import namedtuple
from typing import Optional

import numpy as np
import torch

from . import gym_shim
from . import lib as _lib
from .multi import make_vec_env


class _StepRecords:
    """The episode records of ONE step (serial k), read from the pinned ring on first use."""

    __slots__ = ("_env", "serial", "_done", "_fin", "_rows", "_idx", "_term", "_stepper", "__weakref__")

    def __init__(self, env: "TorchVecEnv", serial: int):
        self._env, self.serial, self._done, self._fin, self._rows, self._idx, self._term = env, serial, None, None, None, None, None
        self._stepper = env._stepper

    def materialise(self):
        """Wait for THIS step's launch and copy its records out of the ring slot (numpy only: no per-env Python work yet)."""
        if self._done is not None:
            return
        env = self._env
        if env._events is not None:
            env._events[self.serial % env._slots].synchronize()  # the launch of THIS step has completed (later ones may still be queued or running)
        else:
            env.synchronize()                                 # (record_events=False: wait for everything issued so far)
        rec = env._ring[self.serial % env._slots]            # [N][4] int32 view of the pinned slot
        self._idx = np.nonzero(rec[:, 0] == np.array(self.serial, np.uint32).view(np.int32))[0]
        self._rows = rec[self._idx]                          # (a copy: the slot is rewritten `slots` steps from now)
        done = np.zeros(env.num_envs, dtype=bool)
        done[self._idx] = True
        if env._want_terminal and self._idx.size:            # owned copies of the finished envs' terminal observations, gathered once
            # from THIS step's own buffer (its slot's rows): the live buffer of later launches holds other episodes' ends by now
            self._term = env._term_bufs[self.serial % env._slots].index_select(0, torch.from_numpy(self._idx).to(env.device))
        self._done = done
        self._env = None

    def episodes(self) -> dict:
        """The finished envs of the step as arrays: env index, Monitor's r and l, the TimeLimit flag, the step's info word."""
        self.materialise()
        r = self._rows
        flags = r[:, 3].view(np.uint32) if r.size else np.zeros(0, np.uint32)
        return {"env": self._idx, "r": np.ascontiguousarray(r[:, 1]).view(np.float32), "l": r[:, 2], "truncated": (flags & 2) != 0, "info": flags >> 8}

    def fin(self) -> dict:
        """{env index: info dict} of the finished envs, built on first use."""
        if self._fin is None:
            e = self.episodes()
            self._fin = {}
            for j, i in enumerate(e["env"].tolist()):
                info = {"episode": {"r": float(e["r"][j]), "l": int(e["l"][j])}}
                if e["truncated"][j]:                        # TimeLimitMask: done at max_episode_steps (whether or not it also terminated)
                    info["bad_transition"] = True
                    info["TimeLimit.truncated"] = True
                if self._stepper:
                    info["steps_reached"] = int(e["info"][j])     # Walker3DStepperEnv.step's info at done (env_locomotion.py:562-566)
                if self._term is not None:
                    info["terminal_observation"] = self._term[j]
                self._fin[i] = info
        return self._fin


class _LazyDone:
    """`done` of one step: a bool array [N] that is fetched when first looked at (np.asarray(done), iteration, indexing, any attribute of
    numpy.ndarray)."""

    __slots__ = ("_rec",)

    def __init__(self, rec: _StepRecords):
        self._rec = rec

    def numpy(self) -> np.ndarray:
        self._rec.materialise()
        return self._rec._done

    def __array__(self, dtype=None, copy=None):
        a = self.numpy()
        return a if dtype is None else a.astype(dtype)

    def __len__(self):
        return len(self._rec._done) if self._rec._done is not None else self._rec._env.num_envs

    def __iter__(self):
        return iter(self.numpy().tolist())      # Python bools: a trainer's `for d in done` comprehension runs twice as fast over them

    def __getitem__(self, i):
        return self.numpy()[i]

    def __getattr__(self, name):        # .any(), .sum(), .dtype, .shape, .nonzero(), .astype(...), ...
        return getattr(self.numpy(), name)

    def __invert__(self):
        return ~self.numpy()

    def __and__(self, o):
        return self.numpy() & o

    def __or__(self, o):
        return self.numpy() | o

    def __eq__(self, o):
        return self.numpy() == o

    def __ne__(self, o):
        return self.numpy() != o

    __hash__ = None

    def __repr__(self):
        return f"LazyDone({self.numpy()!r})"


class _Infos:
    """List-of-dicts view of one step's infos: {} for envs that go on, Monitor / TimeLimitMask keys for envs that finished."""

    __slots__ = ("_n", "_rec")

    def __init__(self, n: int, rec: _StepRecords):
        self._n, self._rec = n, rec

    def _finished(self) -> dict:
        return self._rec.fin()

    def episodes(self) -> dict:
        """The same information without a dict per env: {"env": indices of the envs that finished in this step, "r": their episode returns,
        "l": lengths, "truncated": ended at the TimeLimit ("bad_transition"), "info": the step's info word (Stepper: steps_reached)} as
        numpy arrays -- what a logging loop over thousands of envs wants."""
        return self._rec.episodes()

    def __len__(self):
        return self._n

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self[k] for k in range(*i.indices(self._n))]
        if i < 0:
            i += self._n
        if not 0 <= i < self._n:
            raise IndexError(i)
        return self._finished().get(i, {})

    def __iter__(self):
        out = [{}] * self._n                    # ONE shared empty dict for the envs that go on (the verbatim loops only read it)
        for i, info in self._finished().items():
            out[i] = info
        return iter(out)

    def finished(self):
        """(env index, info dict) of the envs whose episode ended in this step -- what a trainer's logging loop is after."""
        return self._finished().items()


# What TorchVecEnv's constructor decides once about its rows: `policy` and `privileged`, the blocks of the two rows in order as
# {name: (offset, width)} (empty: no such row), and `launches`, the calls (o, row, act) that follow a reset's or a step's launch, in order
_RowPlan = namedtuple("_RowPlan", "policy privileged launches")


def _blocks(*named) -> dict:
    """(name, width) pairs laid end to end -> {name: (offset, width)}, in order, without the empty ones"""
    out, at = {}, 0
    for name, width in named:
        if width:
            out[name] = (at, width)
            at += width
    return out


class TorchVecEnv:
    """`VecPyTorch`-shaped env batch on one MI355X (module docstring).  kwargs go to the env class (`plank_class=...`) / `VecEnv`
    (`max_rows=...`); `sub_batches=k` steps the batch as k sub-batches on their own HIP streams (`multi.SubBatchedVecEnv`).
    `record_slots`: how many steps' episode records the pinned ring holds; a step's `done` / `infos` that are still referenced when
    their slot comes up for rewriting are fetched then, so they stay correct however late they are read.  `eager_done=True` returns
    `done` as a real numpy array (one synchronise per step -- for code that insists on `isinstance(done, np.ndarray)`); `record_events=False`
    drops the per-step event (for loops that read `masks` / `episode_totals` only).  `terminal_observation=True` gives every record slot
    terminal-observation rows of its own (launch k writes slot k % record_slots), so `infos[i]["terminal_observation"]` is the final
    observation of THAT step's episode however late it is read.
    `terrain_bank=dict(n_fields=K, seed=S, n_peaks=256, gain=1.0, redraw_at_reset=True)` (planner ids): a bank of K random height fields of
    the shipped shape (128 x 128 points, 4 per metre) generated on the device before the first reset (include/mocca.h
    mocca_generate_heightfields), every env on one of them -- with `redraw_at_reset` another one in every episode; refresh_terrain(seed)
    regenerates the bank in place.  Without it the envs stand on the shipped map, as ever.

    THE ROWS.  Five options shape what the policy and a teacher or privileged critic read; each needs one handle, and each costs launches
    behind the step's own, never a torch.cat, a host copy or a synchronise:
    `height_scan=dict(points=[P, 2], z_above=1.0, max_drop=2.0)` (perception.scan_grid builds patterns): the terrain height scan (include/
    mocca.h mocca_height_scan), P floats; `depth_camera=perception.DepthCamera(...)`: the egocentric depth image (mocca_depth_camera),
    width * height floats; `history=history.History(steps, stride, columns, actions)`: the observation-action history (mocca_history),
    `envs.venv.history_dim` floats; `curriculum=curriculum.Curriculum(...)` (Stepper ids): the per-env adaptive curriculum
    (mocca_set_curriculum) -- every env's own episodes move its own level, one small launch behind each step, also inside act_step() and a
    captured rollout; `envs.curriculum_levels` is the int32 [N] levels on the device, `envs.curriculum_totals` the per-level counts [10, 4];
    it adds nothing to the rows; `privileged_scan=dict(...)` (teacher-student distillation; not together with `height_scan=`): the scan
    attached but kept OUT of the policy's row; `randomisation=randomisation.Randomisation(...)`: domain randomisation (mocca_set_randomisation)
    -- per-episode motor strength, action latency and random pushes in front of every step (one more small launch; `envs.effective_action()`
    tells what the step read), with `obs_noise` uniform noise on what the policy sees, and a 4-float record of every env's plant (strength,
    delay, steps until the next push, 0).
    The POLICY's row is [obs | scan | depth | hist], each block only where its option is given: `observation_space` has its width, and
    reset() / step() / step(into=...) / capture_rollout return and fill it, act_step() reads it.  With more than [obs] it is a wide buffer of
    this object's, or `into["obs"]` of the trainer's storage; the step's own observation stays in the handle's buffer.
    The PRIVILEGED row, `envs.privileged`, is [obs | scan | record] and exists with `privileged_scan=`: the row a teacher trained with
    `height_scan=` saw (attach_teacher / teacher_targets evaluate a frozen teacher on it), the record only with
    `Randomisation(privileged=True)`: a privileged critic or a teacher knows the plant, the actor does not.  `envs.randomisation` [N, 4] is
    that tail, or a buffer of its own without `privileged=True`.
    THE ORDER behind every reset and every step, whose launch has produced the observation `o`, on the step's stream (_plan_rows states it
    as a list, once; a captured rollout bakes it into its graph):
      1. the privileged scan: [obs | scan] into `envs.privileged`, from the CLEAN `o`;
      2. the plant's record into `envs.randomisation`;
      3. the policy's row: the height scan's launch copies `o` into the row and appends the scan, the camera's appends the depth image
         (a camera alone copies `o` itself), then the sensor noise is added IN PLACE to the row's first obs_dim columns; with no block but
         [obs] the noise lands on `o` itself, and with a history alone the noise launch writes the noisy `o` into the row -- one device
         copy where there is no noise;
      4. the history, last, on the row the policy will read (noisy with `obs_noise`; `envs.privileged` is not changed): its newest frame is
         that row, and the previous frame takes the action the policy output on it -- none after reset(), the tensor step(actions) handed
         to the launch, act_step()'s action output (`into["action"]` or this object's own buffer).
    Under auto-reset all of it, like the observation, belongs to the new episode's first state."""

    def __init__(self, env_id: str, num_envs: int, seed: int = 0, device: Optional[int] = None, sub_batches: int = 1,
                 terminal_observation: bool = False, record_slots: int = 8, eager_done: bool = False, record_events: bool = True,
                 height_scan: Optional[dict] = None, terrain_bank: Optional[dict] = None, depth_camera=None,
                 privileged_scan: Optional[dict] = None, randomisation=None, history=None, curriculum=None, **kw):
        if curriculum is not None:     # (refused before anything touches a device, like the options below)
            from . import model as M
            from .curriculum import STEPPER_IDS_ONLY
            from .vec_env import TASKS
            if TASKS.get(env_id) != M.TASK_WALKER3D_STEPPER:
                raise ValueError(f"curriculum: {STEPPER_IDS_ONLY} ({env_id!r} is not one)")
        if randomisation is not None and randomisation.privileged and privileged_scan is None:
            raise ValueError("Randomisation(privileged=True) puts the plant's record behind [obs | scan]: that takes privileged_scan=")
        if height_scan is not None and privileged_scan is not None:
            raise ValueError("height_scan= puts the scan into the observation row, privileged_scan= keeps it out of it: one of the two")
        # what lives in ONE handle's device memory -- (option, given, runs behind the step's launch) -- refused before anything touches a device
        parted = sub_batches > 1 or len(kw.get("devices") or ()) > 1      # (what make_vec_env cuts into sub-batches or shards)
        for name, arg, behind in (("randomisation", randomisation, False), ("privileged_scan", privileged_scan, True),
                                  ("depth_camera", depth_camera, True), ("height_scan", height_scan, True), ("history", history, True),
                                  ("terrain_bank", terrain_bank, False), ("curriculum", curriculum, False)):
            if arg is not None and behind and terminal_observation:
                raise NotImplementedError(f"{name} with terminal_observation=True: the sensor runs after the step's launch, when an env that "
                                          "finished already holds its next episode's first state -- the terminal state is gone, so nothing of it "
                                          "can be appended to the terminal observation")
            if arg is not None and parted:
                raise NotImplementedError(f"{name} needs one handle (sub_batches=1)")
        self.venv = make_vec_env(env_id, num_envs, sub_batches=sub_batches, seed=seed, auto_reset=True,
                                 **({"device": device} if device is not None else {}), **kw)
        self.env_id, self.num_envs = env_id, int(num_envs)
        self.device = self.venv.device
        self._terrain = None
        if terrain_bank is not None:
            from . import host_logic as H
            tb = dict(terrain_bank)
            unknown = set(tb) - {"n_fields", "seed", "n_peaks", "gain", "redraw_at_reset"}
            if unknown or "n_fields" not in tb:
                raise ValueError(f"terrain_bank takes n_fields, seed, n_peaks, gain, redraw_at_reset (got {sorted(tb)})")
            self._terrain = dict(n_peaks=int(tb.get("n_peaks", 256)), gain=float(tb.get("gain", 1.0)))
            self.venv.set_heightfield_bank(int(tb["n_fields"]), H.HEIGHT_FIELD_SCALE, rows=H.HEIGHT_FIELD_SIZE[0], cols=H.HEIGHT_FIELD_SIZE[1])
            self.refresh_terrain(int(tb.get("seed", 0)))
            self.venv.set_env_fields(None, redraw_at_reset=bool(tb.get("redraw_at_reset", True)))
        scan = height_scan if height_scan is not None else privileged_scan
        if scan is not None:
            self.venv.set_height_scan(**scan)
        if randomisation is not None:
            self.venv.set_randomisation(randomisation)
        if depth_camera is not None:
            self.venv.set_depth_camera(depth_camera)
        if history is not None:
            self.venv.set_history(history)
        self.curriculum_totals = None                      # [10, 4] per level: episodes judged, sum of steps_reached, successes, failures; zero it when you like
        if curriculum is not None:
            self.curriculum_totals = self.venv.set_curriculum(curriculum)
            self._levels = torch.zeros(self.num_envs, dtype=torch.int32, device=self.device)
        plan = self._row_plan = self._plan_rows(
            scan=self.venv.scan_dim if height_scan is not None else 0, depth=self.venv.depth_dim if depth_camera is not None else 0,
            hist=self.venv.history_dim if history is not None else 0, privileged_scan=self.venv.scan_dim if privileged_scan is not None else 0,
            randomisation=randomisation)
        width = lambda blocks: sum(w for _, w in blocks.values())
        rows = lambda w: torch.zeros(self.num_envs, w, dtype=torch.float32, device=self.device)
        self._wide = rows(width(plan.policy)) if len(plan.policy) > 1 else None
        self.privileged = rows(width(plan.privileged)) if plan.privileged else None
        self.randomisation = None
        if "record" in plan.privileged:
            at, w = plan.privileged["record"]
            self.randomisation = self.privileged[:, at:at + w]
        elif randomisation is not None:
            self.randomisation = rows(_lib.RAND_WORDS)
        high = np.inf * np.ones(width(plan.policy), dtype=np.float32)
        self.observation_space = gym_shim.Box(-high, high, dtype=np.float32)                      # robots.py:18-29, env_locomotion.py:58-60
        self.action_space = gym_shim.Box(-np.ones(self.venv.act_dim, np.float32), np.ones(self.venv.act_dim, np.float32), dtype=np.float32)
        # a planner env with its base controller attached (base_controller=...): the action is the 15-number plan (unbounded box,
        # env_locomotion.py:1006-1009) and every step goes through VecEnv.plan_step
        self._plan = getattr(self.venv, "base_controller", None) is not None
        self._venv_step = self.venv.plan_step if self._plan else self.venv.step
        if self._plan:
            high = np.inf * np.ones(self.venv.plan_dim, dtype=np.float32)
            self.action_space = gym_shim.Box(-high, high, dtype=np.float32)
        ep = self.venv.episode_stats(True, slots=int(record_slots))
        self.masks = ep["masks"].unsqueeze(1)              # [N, 1], 0 where the episode ended in the last step; REWRITTEN IN PLACE by every step
        self.bad_masks = ep["bad_masks"].unsqueeze(1)      # [N, 1], 0 where it ended at the TimeLimit ("bad_transition")
        self.episode_totals = ep["totals"]                 # [4] sums of return / length / episodes / truncated episodes; zero it when you like
        self.done = self.venv.done                         # uint8 [N] on the device: bit0 terminated, bit1 TimeLimit
        self._ring = ep["records"].numpy()                 # [slots][N][4] int32 over the pinned host ring
        self._slots, self._k = ep["slots"], ep["first_serial"]
        self._live = [None] * self._slots                  # weak references to the lazy records of the last `slots` steps
        # an event behind each step's launch: what that step's lazy records wait for.  record_events=False saves the record (a trainer that
        # never looks at `done` / `infos`): records then wait for everything issued so far when they are looked at
        self._events = [torch.cuda.Event() for _ in range(self._slots)] if record_events else None
        self._rew2 = self.venv.rew.unsqueeze(1)
        self._want_terminal = bool(terminal_observation)
        self._term_bufs = self._term_attach = self.rollout_terminal_obs = None
        if self._want_terminal:
            # one terminal-observation buffer per record slot: launch k writes its finished envs' final observations into slot k % slots,
            # which no launch touches again before k + slots -- and step() materialises record k before that launch, so a record's
            # terminal observations are its own however late they are read.  Attaching a buffer is a host-side pointer swap (no kernel)
            self._term_bufs = torch.zeros(self._slots, self.num_envs, self.venv.obs_dim, dtype=torch.float32, device=self.device)
            self._term_attach = [self._attach_terminal(self._term_bufs[s]) for s in range(self._slots)]
        self._eager = bool(eager_done)
        from . import model as M
        self._stepper = self.venv.task_id == M.TASK_WALKER3D_STEPPER

    def refresh_terrain(self, seed: int) -> None:
        """Regenerate the whole terrain bank in place from `seed` (asynchronous, on the current stream, ordered against the steps around it):
        the envs keep their field indices and walk on the new fields from their next step on."""
        if self._terrain is None:
            raise _lib.MoccaError("refresh_terrain needs terrain_bank=dict(...) at construction")
        self.venv.generate_heightfields(int(seed), **self._terrain)

    def _one(self, name: str):
        """The one `VecEnv` behind this object, for `name`, which needs it: sub-batches and shards are handles of their own, each with
        its streams, its policy slots and its sensors."""
        if not hasattr(self.venv, "lib"):
            raise NotImplementedError(f"{name} needs one handle (sub_batches=1)")
        return self.venv

    def _masks_into(self, into: dict) -> None:
        """step(into=) / capture_rollout(into=): the kernel's `masks` / `bad_masks` columns into the caller's tensors, from the next launch on"""
        if "masks" in into or "bad_masks" in into:
            self.masks, self.bad_masks = into.get("masks", self.masks), into.get("bad_masks", self.bad_masks)
            self.venv.episode_masks_into(self.masks, self.bad_masks)

    def _attach_terminal(self, buf: torch.Tensor):
        """Attach `buf` [N, obs_dim] as the terminal-observation buffer of the handle(s) (each sub-batch its rows) and return the
        (function, handle, pointer) calls that attach it again -- what step() replays before its launch."""
        venv = self.venv
        parts = [(venv, buf)] if hasattr(venv, "lib") else [(e, buf[sl]) for e, sl in zip(venv.parts, venv.slices)]
        calls = []
        for e, b in parts:
            e.keep_terminal_obs(True, buffer=b)     # (checks shape, dtype and device once)
            calls.append((e.lib.mocca_set_terminal_obs_buffer, e.h, b.data_ptr()))
        venv.terminal_obs = buf
        return calls

    def _use_terminal(self, slot: int):
        for fn, h, ptr in self._term_attach[slot]:
            _lib.check(fn(h, ptr), h)
        self.venv.terminal_obs = self._term_bufs[slot]

    def synchronize(self):
        """Wait for every launch issued so far (the streams the env steps on)."""
        if hasattr(self.venv, "synchronize"):
            self.venv.synchronize()
        torch.cuda.current_stream(self.device).synchronize()

    # ---- the VecPyTorch surface ----
    def reset(self) -> torch.Tensor:
        obs = self.venv.reset()        # (the reset kernel zeroes the envs' running returns: Monitor.reset)
        return self._fill(obs, obs if self._wide is None else self._wide, None)

    def effective_action(self) -> torch.Tensor:
        """randomisation=: what the last step's kernel read in place of the action, [N, act_dim]: `VecEnv.effective_action`.  One handle only."""
        return self._one("effective_action").effective_action()

    @property
    def curriculum_levels(self) -> torch.Tensor:
        """curriculum=: every env's level NOW, int32 [N] on the device -- one launch into a buffer of this object's, nothing synchronises
        until the caller reads it (at log time, outside the collection loop)."""
        if self.curriculum_totals is None:
            raise _lib.MoccaError("curriculum_levels needs curriculum=Curriculum(...) at construction")
        return self.venv.curriculum_levels(out=self._levels)

    def _plan_rows(self, scan, depth, hist, privileged_scan, randomisation) -> _RowPlan:
        """THE rows and THE order (class docstring) from the widths of the blocks (0: none) and the randomisation (None: none).  A launch
        is called with (o, row, act): the observation the reset or step just produced, the policy's row being filled -- the wide buffer,
        `into["obs"]`, or `o` itself where the row is [obs] -- and the action for the history's previous frame."""
        v, d = self.venv, self.venv.obs_dim
        noisy = randomisation is not None and randomisation.obs_noise is not None
        record = _lib.RAND_WORDS if randomisation is not None and randomisation.privileged else 0
        policy = _blocks(("obs", d), ("scan", scan), ("depth", depth), ("hist", hist))
        privileged = _blocks(("obs", d), ("scan", privileged_scan), ("record", record)) if privileged_scan else {}
        launches = []
        if privileged:
            launches.append(lambda o, row, act: v.height_scan(out=self.privileged, obs=o))
        if randomisation is not None:
            launches.append(lambda o, row, act: v.randomisation_record(out=self.randomisation))
        if scan:
            launches.append(lambda o, row, act: v.height_scan(out=row, obs=o))
            if depth:
                launches.append(lambda o, row, act, at=policy["depth"][0]: v.depth_camera(out=row[:, at:]))
        elif depth:
            launches.append(lambda o, row, act: v.depth_camera(out=row, obs=o))
        elif hist:       # no sensor copies the observation: the noise launch writes the noisy head straight into the row, else one device copy
            launches.append((lambda o, row, act: v.sensor_noise(o, out=row)) if noisy else (lambda o, row, act: row[:, :d].copy_(o)))
            noisy = False
        if noisy:
            launches.append(lambda o, row, act: v.sensor_noise(row))
        if hist:
            launches.append(lambda o, row, act, at=policy["hist"][0]: v.history(row, act, out=row[:, at:]))
        return _RowPlan(policy, privileged, launches)

    def _fill(self, o, row, act):
        """the row plan's launches behind a reset or a step that produced `o` -> `row`, the policy's row"""
        for launch in self._row_plan.launches:
            launch(o, row, act)
        return row

    def _step_obs(self, actions, obs_out=None, rew_out=None, launch=None):
        """the step's launch and the row plan's launches behind it, which write the policy's row (into `obs_out` or this object's own buffer;
        with a wide row the step's own observation stays in the handle's buffer) -> (obs, reward).  `launch`: what steps instead of step() /
        plan_step() (act_step: `actions` is then the policy's input row)"""
        act_launch, launch = launch, launch or self._venv_step
        if self._wide is None:
            if obs_out is None and rew_out is None:      # (the sub-batched step takes the actions only)
                o, r = launch(actions)[:2]
            else:
                o, r = launch(actions, obs_out=obs_out, rew_out=rew_out)[:2]
            return self._fill(o, o, None), r
        wide = self._wide if obs_out is None else obs_out
        if wide.shape != self._wide.shape or not wide.is_contiguous():
            raise ValueError("with a height scan, a depth camera or a history the observation rows are contiguous float32 "
                             "[n_envs, obs_dim + scan_dim + depth_dim + history_dim]")
        o, r = launch(actions, rew_out=rew_out)[:2]
        # the action of the frame the policy acted on: step()'s tensor, or what act_step's policy launch wrote
        return self._fill(o, wide, actions if act_launch is None else self.last_act["action"]), r

    def step(self, actions: torch.Tensor, into: Optional[dict] = None):
        """`into` (one handle only): {"obs": [N, obs_dim], "reward": [N, 1], "masks": [N, 1], "bad_masks": [N, 1]} -- any subset -- tensors of the
        TRAINER's storage that this step's launch writes directly (row t + 1 of the rollout buffers: PPO reads its next policy input from
        there anyway), instead of this object's own buffers: no copy kernels between the env and the storage.  The returned `obs` / `reward`
        are those tensors; `envs.masks` / `envs.bad_masks` keep pointing at the last buffers handed in."""
        if actions.device != self.device or actions.dtype != torch.float32 or not actions.is_contiguous():
            actions = actions.to(device=self.device, dtype=torch.float32).contiguous()
        return self._step(actions, into, None)

    def _step(self, actions, into, launch):
        """step() / act_step(): the record bookkeeping around one launch of `launch` (None: step() / plan_step())"""
        k = self._k
        slot = k % self._slots
        old = self._live[slot]
        if old is not None:
            old = old()
            if old is not None:
                old.materialise()      # its slot is about to be rewritten: fetch it now (its launch finished long ago)
        if self._term_attach is not None:
            self._use_terminal(slot)
        rew = self._rew2
        if into:
            self._one("step(into=...)")
            self._masks_into(into)
            rew = into.get("reward", rew)
            obs = self._step_obs(actions, obs_out=into.get("obs"), rew_out=into.get("reward"), launch=launch)[0]
        else:
            obs = self._step_obs(actions, launch=launch)[0]
        if self._events is not None:
            self._events[slot].record(torch.cuda.current_stream(self.device))
        self._k = k + 1 if k < 0xFFFFFFFF else 1
        rec = _StepRecords(self, k)
        self._live[slot] = weakref.ref(rec)
        return obs, rew, (_LazyDone(rec).numpy() if self._eager else _LazyDone(rec)), _Infos(self.num_envs, rec)

    # ---- the trainer's own policy on the device (VecEnv.set_policy / act_step, include/mocca.h mocca_act_step) ----
    def attach_policy(self, policy) -> None:
        """Attach a `policy.DevicePolicy` whose input is this env's observation row ([obs | scan | depth] with a height scan / a depth camera) and whose actions are
        the env's -- on a planner env with its base controller the 15-number plans, and act_step() goes policy -> base controller -> step
        (VecEnv.act_plan_step); `update_policy(policy_or_flat_tensor)` refreshes its weights once per PPO iteration.  One handle only.  A
        policy with mirror tables (`symmetric_policy(p)`, `DevicePolicy(symmetry=)`) acts as the symmetric network: the tables cover the
        whole row.  An `asymmetric` policy (a privileged critic) needs `privileged_scan=`: its critic reads `envs.privileged` ([obs | scan]),
        which this call binds (VecEnv.set_critic_rows), so act_step()'s value is the privileged critic's; the actor reads the observation
        row as ever."""
        self._one("attach_policy")
        act_dim = self.venv.plan_dim if self._plan else self.venv.act_dim
        if policy is not None and (policy.in_dim != self.observation_space.shape[0] or policy.act_dim != act_dim):
            raise ValueError(f"the policy maps {policy.in_dim} -> {policy.act_dim}, the env {self.observation_space.shape[0]} -> {act_dim}")
        asym = getattr(policy, "asymmetric", False)
        if asym and (self.privileged is None or policy.critic_in_dim != self.privileged.shape[1]):
            raise ValueError(f"the policy's critic reads {policy.critic_in_dim} inputs of its own: " + (
                "that takes privileged_scan= ([obs | scan])" if self.privileged is None
                else f"envs.privileged has {self.privileged.shape[1]} ([obs | scan], with Randomisation(privileged=True) [obs | scan | record])"))
        self.venv.set_policy(policy)
        if asym:
            self.venv.set_critic_rows(self.privileged)
        n, f32 = self.num_envs, dict(dtype=torch.float32, device=self.device)
        self._pol_bufs = None if policy is None else {"action": torch.zeros(n, policy.act_dim, **f32), "logp": torch.zeros(n, 1, **f32),
                                                      "value": torch.zeros(n, 1, **f32)}

    def update_policy(self, params) -> None:
        self.venv.update_policy(params)

    # ---- teacher-student distillation (VecEnv.set_teacher / teacher_act / distill_grad / distill_update) ----
    def attach_teacher(self, policy) -> None:
        """Attach a frozen `policy.DevicePolicy` as the teacher (None detaches): it reads `envs.privileged` ([obs | scan], with
        `privileged_scan=`) or, without one, the env's observation row, and labels the states the student visits (teacher_targets).  One
        handle only."""
        self._one("attach_teacher")
        rows = self._teacher_rows()
        if policy is not None and policy.in_dim != rows.shape[1]:
            raise ValueError(f"the teacher reads {policy.in_dim} inputs, its rows here have {rows.shape[1]}"
                             + (" ([obs | scan], with Randomisation(privileged=True) [obs | scan | record])" if self.privileged is not None else " (the observation row; privileged_scan= gives [obs | scan])"))
        self.venv.set_teacher(policy)

    def _teacher_rows(self):
        if self.privileged is not None:
            return self.privileged
        return self.venv.obs if self._wide is None else self._wide

    def teacher_targets(self, mean_out: Optional[torch.Tensor] = None, value_out: Optional[torch.Tensor] = None) -> dict:
        """The teacher's actor mean [N, A] and value [N] (or [N, 1]) of the state the envs are in now -- after the last reset() / step() /
        act_step() -- into `mean_out` / `value_out` (rows of the trainer's storage; allocated where none is given): one launch on the
        step's stream, capturable behind act_step and the sensors in one graph.  -> {"mean", "value"}"""
        return self.venv.teacher_act(self._teacher_rows(), mean=mean_out, value=value_out)

    # (distill_grad, distill_update, finish_rollout, update_obs_stats, ppo_grad, adam_step, ppo_update, symmetric_policy, policy_mirror_tables,
    # set_policy_mirror_loss and set_policy_mirror_dup are the one handle's: _FORWARDED, below the class)

    def _act_launch(self, into):
        """the launcher _step_obs() calls: act_step with the policy's outputs going to `into`'s "action" / "logp" / "value" (this object's
        own buffers where a key is missing); sets `self.last_act` to the three tensors written"""
        if getattr(self, "_pol_bufs", None) is None:
            raise _lib.MoccaError("act_step needs a device policy (attach_policy)")
        out = {k: (into or {}).get(k, self._pol_bufs[k]) for k in ("action", "logp", "value")}
        self.last_act = out
        if self._plan:       # a planner env: the action is the plan, the base controller runs between the policy and the step
            return lambda row, **kw: self.venv.act_plan_step(row, plan_out=out["action"], logp_out=out["logp"], value_out=out["value"], **kw)
        return lambda row, **kw: self.venv.act_step(row, action_out=out["action"], logp_out=out["logp"], value_out=out["value"], **kw)

    def act_step(self, obs: Optional[torch.Tensor] = None, into: Optional[dict] = None):
        """`value, action, logp = actor_critic.act(obs); envs.step(action)` as two launches and no torch op: the attached policy reads `obs`
        (rollouts.obs[t]; None: the observation the last reset() / step() returned) and writes action [N, A], log-probability and value
        ([N, 1]) into `into["action"]` / `into["logp"]` / `into["value"]` -- rows t of the trainer's storage; this object's own buffers,
        `envs.last_act`, where a key is missing --, then the step runs on that action.  The rest of `into` and the return value are
        step()'s.  The noise comes from the kernel (seed, env, the env's step and episode counters)."""
        launch = self._act_launch(into)
        if obs is None:
            obs = self.venv.obs if self._wide is None else self._wide
        return self._step(obs, into, launch)

    def capture_rollout(self, policy=None, num_steps: int = 1, sink=None, warmup: int = 2, into=None):
        """The collection phase as ONE CUDA graph: `num_steps` x { action = policy(obs); env.step(action); sink(t, obs, reward, masks, bad_masks,
        action) } captured once, replayed with `.replay()` (returns the `torch.cuda.CUDAGraph`).  `policy` maps the observation tensor [N, obs_dim] to
        actions [N, act_dim] with torch ops only (no host reads; `policy(obs, t)` is called with the step index if it takes two arguments);
        `sink` copies what the trainer keeps into ITS pre-allocated rollout storage (`rollouts.obs[t + 1].copy_(obs)` ...: `obs`, `reward` [N, 1], `masks` / `bad_masks` [N, 1] are this env's persistent buffers, rewritten
        by every step).  `mocca_step` keeps no host state per launch (ABI 7), so a replay advances the envs exactly as `num_steps` calls of
        `step()` would -- bit for bit (tests/test_gpu_trainer_api.py).  Episode statistics of a replayed rollout: `episode_totals` (the lazy
        `done` / `infos` of `step()` do not exist inside a graph).  `warmup` eager iterations run first on a side stream, as torch requires before a
        capture: they advance the envs too.  `into`: a callable t -> the `into` dict of `step()`, each with an "obs" entry -- launch t of the
        graph writes its observations / rewards / masks straight into those tensors (row t + 1 of the trainer's storage) and `policy` reads
        `into(t - 1)["obs"]`; `into(-1)["obs"]` is the storage's row 0, which must hold the current observation before every replay (PPO's
        `rollouts.after_update()` copies the last row there; this call leaves it filled): the rollout needs no copy kernels at all.
        `terminal_observation=True`: the graph's launches all write their finished envs' final observations into ONE buffer of their own,
        `envs.rollout_terminal_obs` [N, obs_dim] (apart from the record slots of `step()`; rows of envs that did not finish keep older
        content), which is also `envs.venv.terminal_obs` while `sink` runs -- a sink that wants them copies them at step t.
        `policy=None`: the attached device policy (attach_policy) acts -- every step of the graph is act_step's two launches (three on a
        planner env: act_plan_step); `into(t)` may
        carry "action" / "logp" / "value" rows, and `sink`'s `action` is the tensor the policy wrote.  `update_policy` between replays
        changes what the graph computes: no recapture."""
        venv, dev = self._one("capture_rollout"), self.device       # (sub-batches step on streams of their own)
        if self._want_terminal:          # the graph bakes the buffer's address into its launches: a fixed one, not a record slot of step()
            if self.rollout_terminal_obs is None:
                self.rollout_terminal_obs = torch.zeros_like(self._term_bufs[0])
            self._attach_terminal(self.rollout_terminal_obs)
        obs, rew = (venv.obs if self._wide is None else self._wide), self._rew2
        if policy is None:
            act_of = None
        elif len(inspect.signature(policy).parameters) >= 2:        # policy(obs, t): e.g. to write its action into the storage's row t
            act_of = policy
        else:
            act_of = lambda o, t: policy(o)

        def body(t):
            d = {} if into is None else into(t)
            row = obs if into is None else into(t - 1)["obs"]        # the policy's input: where the last step wrote its observation
            if act_of is None:       # the device policy reads the row itself: the step is act_step's launches
                x, launch = row, self._act_launch(d)
            else:                    # a torch policy has produced the action: the step is step()'s launch
                x, launch = act_of(row, t), None
            self._masks_into(d)
            o, r = self._step_obs(x, obs_out=d.get("obs"), rew_out=d.get("reward"), launch=launch)[:2]
            if into is None:
                o, r = obs, rew
            if sink is not None:
                sink(t, o, r, self.masks, self.bad_masks, self.last_act["action"] if act_of is None else x)

        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side), torch.no_grad():
            if into is not None:
                into(-1)["obs"].copy_(obs)
            for t in range(warmup):
                body(t)
            if into is not None and warmup > 0:
                into(-1)["obs"].copy_(into(warmup - 1)["obs"])      # row 0 <- the observation the warm-up ended on
        torch.cuda.current_stream(dev).wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph), torch.no_grad():
            for t in range(num_steps):
                body(t)
        return graph

    def step_async(self, actions):      # baselines' two-phase form
        self._pending = self.step(actions)

    def step_wait(self):
        out, self._pending = self._pending, None
        return out

    def close(self):
        self.venv.close()

    def seed(self, seed: int):
        return self.venv.seed(seed)

    # ---- what the trainers reach through `envs.venv` / a dummy env ----
    def get_mirror_indices(self):
        return self.venv.get_mirror_indices()

    def set_env_params(self, params_dict):
        self.venv.set_env_params(params_dict)

    def set_robot_params(self, params_dict):
        self.venv.set_robot_params(params_dict)

    def env_method(self, name: str, *args, **kwargs):
        """baselines' `venv.env_method(name, ...)`: one result per env for the methods the reference's envs expose batch-wide."""
        if name in ("set_env_params", "set_robot_params", "evaluation_mode", "get_mirror_indices", "seed"):
            return [getattr(self, name)(*args, **kwargs)] * self.num_envs
        raise AttributeError(f"env_method({name!r}) has no batched counterpart")

    def evaluation_mode(self, on=True):
        self.venv.evaluation_mode(on)


# Methods of the one handle that the trainer calls on `envs` unchanged: name -> what the call is (the arguments and the rest: VecEnv's docstring)
_FORWARDED = {
    "distill_grad": "the regression gradient over stored rows and their targets, four launches",
    "distill_update": "epochs x minibatches of [shuffle, distill_grad, adam_step] over the stored rows as one call",
    "finish_rollout": "returns, advantages (normalised by default) and their moments from the rollout storage, two launches",
    "update_obs_stats": "merge a rollout's observation rows into a `rollout.ObsStats`, two launches",
    "ppo_grad": "PPO's minibatch loss and its gradient over the rollout storage, four launches -- of the symmetric network where the attached "
                "policy carries mirror tables (`symmetric_policy`)",
    "adam_step": "clip_grad_norm_, Adam's step and update_policy on the flat parameter tensor, three launches",
    "ppo_update": "a2c-ppo-acktr's `agent.update(rollouts)` over the rollout storage as one call",
    "symmetric_policy": "a copy of `policy` with this env's mirror tables, the attached height scan's pattern included",
    "policy_mirror_tables": "this env's mirror tables for `policy`, the attached height scan's pattern included",
    "set_policy_mirror_loss": "attach the mirror-symmetry loss for `ppo_grad` / `ppo_update` (None detaches)",
    "set_policy_mirror_dup": "attach the mirror-duplicated rows for `ppo_grad` / `ppo_update` (None detaches)",
}


def _forwarder(name: str, what: str):
    def method(self, *args, **kw):
        return getattr(self._one(name), name)(*args, **kw)
    method.__name__, method.__qualname__ = name, f"TorchVecEnv.{name}"
    method.__doc__ = f"{what}: `VecEnv.{name}`.  One handle only."
    return method


for _name, _what in _FORWARDED.items():
    setattr(TorchVecEnv, _name, _forwarder(_name, _what))


def make_vec_envs(env_name: str, seed: int, num_processes: int, log_dir=None, device=None, **kw) -> TorchVecEnv:
    """Same call as the trainers' `common.envs_utils.make_vec_envs(env_name, seed, num_processes, log_dir)`; `log_dir` (Monitor's csv) is
    accepted and ignored -- episode statistics arrive through `infos` / `envs.episode_totals`."""
    dev = None
    if device is not None:
        dev = torch.device(device).index if not isinstance(device, int) else device
    return TorchVecEnv(env_name, num_processes, seed=seed, device=dev, **kw)
