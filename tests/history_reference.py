"""The observation-action history restated in numpy (include/mocca.h "The rule"; the device's and the host's functions are
csrc/mocca_history.h): a class fed (rows, act or None, T, E) per call that returns the block.  Written the other way round from the
header: whole envs at a time, the ring writes of steps 1 and 2 first, then the block from the ring as they left it -- but for the rule's
one exception, the action part of the pair one step back, which is `act` itself (+0.0 without one: a second call on the same step that
brings no action shows none, though the ring still holds the first call's).  `mutate` names a plausible wrong reading; the tests show
that each differs from the rule on their inputs."""
import numpy as np

MAX_STEPS, MAX_STRIDE, MAX_DIM, MAX_ACT = 16, 8, 1024, 32
NO_T = 0xFFFFFFFF
MUTATIONS = ("oldest_first", "stride_off_by_one", "no_episode_zeroing", "action_late", "ring_of_ks_slots")


class History:
    """n envs, K = steps, s = stride, cols the observation columns, A the action width"""

    def __init__(self, n, steps, stride, cols, act_dim, mutate=None):
        assert mutate is None or mutate in MUTATIONS, mutate
        self.n, self.K, self.s, self.cols, self.A, self.mutate = int(n), int(steps), int(stride), np.asarray(cols, np.int64).reshape(-1), int(act_dim), mutate
        self.C = self.cols.size
        self.W = self.C + self.A
        assert 1 <= self.K <= MAX_STEPS and 1 <= self.s <= MAX_STRIDE and 0 <= self.A <= MAX_ACT and self.W >= 1 and self.K * self.W <= MAX_DIM
        assert np.unique(self.cols).size == self.C
        self.R = self.K * self.s + (0 if mutate == "ring_of_ks_slots" else 1)
        self.ring = np.zeros((self.n, self.R, self.W), np.float32)
        self.tag_e = np.full((self.n, self.R), NO_T, np.int64)
        self.tag_t = np.full((self.n, self.R), NO_T, np.int64)
        self.calls = np.zeros(self.n, np.int64)

    @property
    def dim(self):
        return self.K * self.W

    def _holds(self, e, u):
        """does the slot of step u hold the frame (e, u)?  (u may be negative where the caller masks it)"""
        i = np.arange(self.n)
        slot = np.mod(u, self.R)
        return (self.tag_e[i, slot] == e) & (self.tag_t[i, slot] == u)

    def __call__(self, rows, act, T, E):
        """rows float32 [n, >= obs_dim], act float32 [n, >= A] or None, T and E the envs' task words -> float32 [n, K * (C + A)]"""
        n, C, W, R, i = self.n, self.C, self.W, self.R, np.arange(self.n)
        rows = np.asarray(rows, np.float32)
        t, e = np.asarray(T, np.int64).reshape(n), np.asarray(E, np.int64).reshape(n)
        if self.mutate == "no_episode_zeroing":      # the wrong reading: a ring over the CALLS, whatever episode they belong to
            t, e = self.calls.copy(), np.zeros(n, np.int64)
            self.calls += 1
        # 1. the current frame
        slot = np.mod(t, R)
        self.ring[i, slot, :C] = rows[:, self.cols]
        self.ring[i, slot, C:] = 0.0
        self.tag_e[i, slot], self.tag_t[i, slot] = e, t
        # 2. the previous frame's action
        if act is not None and self.A:
            act = np.asarray(act, np.float32)[:, :self.A]
            if self.mutate == "action_late":         # the wrong reading: a_{t-1} is filed beside o_t
                self.ring[i, slot, C:] = act
            else:
                ok = (t >= 1) & self._holds(e, t - 1)
                self.ring[i[ok], np.mod(t - 1, R)[ok], C:] = act[ok]
        # 3. the block
        out = np.zeros((n, self.K * W), np.float32)
        for j in range(1, self.K + 1):
            back = j * self.s - (1 if self.mutate == "stride_off_by_one" else 0)
            u = t - back
            valid = (t >= back) & self._holds(e, u)
            pair = np.where(valid[:, None], self.ring[i, np.mod(u, R)], np.float32(0.0))
            if back == 1 and self.A and self.mutate != "action_late":      # the exception: the word this call writes is not read back
                pair[:, C:] = np.where(valid[:, None], act, np.float32(0.0)) if act is not None else np.float32(0.0)
            k = self.K - j if self.mutate == "oldest_first" else j - 1
            out[:, k * W:(k + 1) * W] = pair
        return out
