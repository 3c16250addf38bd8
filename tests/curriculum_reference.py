"""The per-env adaptive curriculum restated in numpy (include/mocca.h mocca_set_curriculum; csrc/mocca_curriculum.h): what the header's
cur_thread and the kernel are held to, bit for bit -- all of it integers and whole f32 numbers.  `Rule(...)(done, info, episode)` is one
launch.  MUTATIONS are plausible wrong readings of the rule, for the tests that show the streams tell them apart."""
import numpy as np

MAX_LEVEL, MAX_PATIENCE, LEVELS, TOTALS, DOMAIN = 9, 64, 10, 4, 6
MUTATIONS = ("no_hold", "hold_kept", "streak_kept", "strict", "recycle_by_step")


def philox0(c0, c1, c2, c3, k0, k1):
    """word 0 of Philox4x32-10 over arrays of counters (csrc/mocca_philox.h)"""
    c = [np.asarray(x, np.uint64) & np.uint64(0xFFFFFFFF) for x in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1, m = np.uint64(k0), np.uint64(k1), np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & m, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & m]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & m, (k1 + np.uint64(0xBB67AE85)) & m
    return c[0].astype(np.uint32)


def level_of(words):
    """the level a vector word stands for: truncated, clamped to 0 .. 9 (the step kernel's live_curriculum)"""
    return np.clip(np.trunc(np.asarray(words, np.float32)).astype(np.int64), 0, MAX_LEVEL)


def start_levels(cfg, levels):
    """what mocca_set_curriculum starts from: the levels the envs had, clamped into the band"""
    return np.clip(level_of(levels), cfg["min_level"], cfg["max_level"]).astype(np.float32)


def draw(cfg, seed, gid, episode):
    """the recycle draw of every env: the word w and the level it gives"""
    w = philox0(gid, 0, episode, DOMAIN, seed & 0xFFFFFFFF, seed >> 32)
    span = np.uint64(cfg["max_level"] - cfg["min_level"] + 1)
    return w, cfg["min_level"] + ((w.astype(np.uint64) * span) >> np.uint64(32)).astype(np.int64)


class Rule:
    """state of n envs: `level` f32 [n] (the vector's words), `streak`, `hold` int32 [n], `totals` f32 [10, 4], and `draws`, the recycle words
    taken by the last launch (0 where none was)"""

    def __init__(self, cfg: dict, levels, seed: int = 0, env_offset: int = 0, mutate=None):
        assert mutate is None or mutate in MUTATIONS
        self.cfg, self.seed, self.mutate = dict(cfg), int(seed), mutate
        self.level = np.array(levels, np.float32)
        n = self.level.size
        self.gid = env_offset + np.arange(n)
        self.streak, self.hold = np.zeros(n, np.int32), np.zeros(n, np.int32)
        self.totals = np.zeros((LEVELS, TOTALS), np.float32)
        self.draws = np.zeros(n, np.uint32)

    def __call__(self, done, info, episode, step=None):
        """one launch: done u8 [n], info i32 [n], episode (and, for the reading that keys by it, step) the task records' counters NOW"""
        c, m = self.cfg, self.mutate
        done, info = np.asarray(done) != 0, np.asarray(info, np.int64)
        key = np.asarray(step if m == "recycle_by_step" else episode, np.int64)
        w, recycled = draw(c, self.seed, self.gid, key)
        self.draws[:] = 0
        for e in np.nonzero(done)[0]:
            if self.hold[e] and m != "no_hold":                                        # 1
                if m != "hold_kept":
                    self.hold[e] = 0
                continue
            L, s = int(level_of(self.level[e])), int(info[e])                          # 2
            ok = s > c["promote_at"] if m == "strict" else s >= c["promote_at"]
            bad = s < c["demote_at"] if m == "strict" else s <= c["demote_at"]
            self.totals[L] += np.array([1, s, ok, bad], np.float32)                    # 3
            nxt, run = L, int(self.streak[e])
            if ok:                                                                     # 4
                run = (run if m == "streak_kept" else max(run, 0)) + 1
                if run >= c["patience"]:
                    run = 0
                    if L < c["max_level"]:
                        nxt = L + 1
                    elif c["recycle"]:
                        nxt, self.draws[e] = int(recycled[e]), w[e]
            elif bad:                                                                  # 5
                run = (run if m == "streak_kept" else min(run, 0)) - 1
                if run <= -c["patience"]:
                    run, nxt = 0, max(L - 1, c["min_level"])
            else:                                                                      # 6
                run = 0
            self.streak[e] = run
            if nxt != L:                                                               # 7
                self.level[e], self.hold[e] = np.float32(nxt), 1
        return self

    def levels(self):
        return level_of(self.level).astype(np.int32)


def stream(n: int, launches: int, seed: int = 5, p_done: float = 0.2, s_max: int = 20):
    """random (done, info) streams with the counters a task record would show the launch: per launch (done u8 [n], info i32 [n], episode u32
    [n], step u32 [n]) -- an env that is done has been reset inside the step: its episode counter already counts the next episode, its
    step counter is 0.  Done bytes take 1, 2 and 3 (terminated, TimeLimit, both)."""
    rng = np.random.default_rng(seed)
    episode, step = np.zeros(n, np.int64), np.zeros(n, np.int64)
    out = []
    for _ in range(launches):
        done = (rng.random(n) < p_done).astype(np.uint8) * rng.integers(1, 4, n).astype(np.uint8)
        info = rng.integers(0, s_max + 1, n).astype(np.int32)
        step += 1
        episode[done != 0] += 1
        step[done != 0] = 0
        out.append((done, info, episode.astype(np.uint32), step.astype(np.uint32)))
    return out
