"""The one-substep comparison of tests/test_gpu_substep.py (kernel vs f32 oracle, f32 vs f64 oracle as the yardstick, samples split by
matching active sets) as an accumulator whose verdict is a list of failed bars instead of assertions -- so that a negative control can
show that the comparison DOES fail when the two sides run different blobs.  The bars are the ones of
test_single_substep_parity_with_matching_active_sets -- a copy: a change to a threshold there must be made here too (that test points
here).  TEST INFRASTRUCTURE ONLY."""
import numpy as np


def units(a, b):
    return np.abs(a - b) / (1e-5 * (1.0 + np.abs(b)))


class SubstepStats:
    def __init__(self, nd):
        self.nd = nd
        self.n_same = self.n_diff = self.n_clamp_diff = 0
        self.e_gpu, self.e_f32, self.e_flip, self.e_f32_flip, self.rows = [], [], [], [], []

    def add(self, sg, sc, s6, dg_, dc_, d6_):
        """New states of kernel / f32 oracle / f64 oracle and their debug records (include/mocca.h MOCCA_DBG_*) of one substep."""
        nd = self.nd
        ok = np.isfinite(sc).all(axis=1) & np.isfinite(s6).all(axis=1)
        rows_same = (dg_[:, :8] == dc_[:, :8]).all(axis=1) & ok            # rows, contacts, slot / limit masks
        same = rows_same & (dg_[:, 8:12] == dc_[:, 8:12]).all(axis=1)      # ... and every clamp decision of the solver
        self.n_same += int(same.sum()); self.n_diff += int((~rows_same & ok).sum()); self.n_clamp_diff += int((rows_same & ~same).sum())
        self.rows.append(dc_[ok, 0])
        if same.any():
            self.e_gpu.append(units(sg[same][:, :nd], sc[same][:, :nd]).max(axis=1))
        flip = rows_same & ~same
        if flip.any():
            self.e_flip.append(units(sg[flip][:, :nd], sc[flip][:, :nd]).max(axis=1))
        same64 = (d6_[:, :12] == dc_[:, :12]).all(axis=1) & ok
        if same64.any():
            self.e_f32.append(units(sc[same64][:, :nd], s6[same64][:, :nd]).max(axis=1))
        flip64 = (d6_[:, :8] == dc_[:, :8]).all(axis=1) & ok & ~same64
        if flip64.any():
            self.e_f32_flip.append(units(sc[flip64][:, :nd], s6[flip64][:, :nd]).max(axis=1))
        return ok

    def failures(self):
        """The bars of test_single_substep_parity_with_matching_active_sets that this sample misses (empty: it passes), and a summary."""
        q = lambda x, p: float(np.percentile(x, p))
        bad = []
        total = max(1, self.n_same + self.n_diff + self.n_clamp_diff)
        frac, frac_clamp = self.n_diff / total, self.n_clamp_diff / total
        e_gpu = np.concatenate(self.e_gpu) if self.e_gpu else np.zeros(0)
        e_f32 = np.concatenate(self.e_f32) if self.e_f32 else np.zeros(1)
        rows = np.concatenate(self.rows) if self.rows else np.zeros(1)
        msg = (f"{total} substeps, rows/substep median {np.median(rows):.0f} max {rows.max()}, row sets differ in {100 * frac:.3f} %, clamp patterns "
               f"(same rows) in {100 * frac_clamp:.3f} %")
        if len(e_gpu):
            msg += (f"; same active set, state error in units of 1e-5 (1+|x|): GPU vs f32 oracle median {q(e_gpu, 50):.3g} p90 {q(e_gpu, 90):.3g} "
                    f"p99 {q(e_gpu, 99):.3g} max {e_gpu.max():.3g} | f32 oracle vs f64 oracle median {q(e_f32, 50):.3g} p90 {q(e_f32, 90):.3g} "
                    f"p99 {q(e_f32, 99):.3g} max {e_f32.max():.3g}")
        if frac >= 0.01:
            bad.append(f"active sets differ in {100 * frac:.2f} % of the substeps")
        if self.e_flip:
            e_flip = np.concatenate(self.e_flip)
            yf = np.concatenate(self.e_f32_flip) if self.e_f32_flip else np.zeros(0)
            rate_y = len(yf) / total
            msg += f"; same rows, another clamp pattern: {len(e_flip)} samples, median {q(e_flip, 50):.3g} max {e_flip.max():.3g} (f32 vs f64: {len(yf)})"
            if not frac_clamp <= 2 * rate_y + 5e-4:
                bad.append(f"clamp flips {frac_clamp:.4g} vs the yardstick's {rate_y:.4g}")
            if not e_flip.max() < max(10 * (yf.max() if len(yf) else 0.0), 2e4):
                bad.append(f"flip size {e_flip.max():.3g}")
            if len(e_flip) >= 200 and len(yf) >= 200:
                if not q(e_flip, 99) <= max(30.0, 3 * q(yf, 99)):
                    bad.append(f"flip p99 {q(e_flip, 99):.3g}")
                if not q(e_flip, 90) <= max(10.0, 3 * q(yf, 90)):
                    bad.append(f"flip p90 {q(e_flip, 90):.3g}")
            if len(e_flip) >= 20 and not q(e_flip, 50) < max(100.0, 5 * q(e_f32, 50), 3 * (q(yf, 50) if len(yf) else 0.0)):
                bad.append(f"flip median {q(e_flip, 50):.3g}")
        if not len(e_gpu):
            bad.append("no sample with the same active set")
        else:
            if not q(e_gpu, 50) < max(1.0, 3 * q(e_f32, 50)):
                bad.append(f"median {q(e_gpu, 50):.3g} vs yardstick {q(e_f32, 50):.3g}")
            if not q(e_gpu, 99) < max(10.0, 3 * q(e_f32, 99)):
                bad.append(f"p99 {q(e_gpu, 99):.3g} vs yardstick {q(e_f32, 99):.3g}")
            if not e_gpu.max() < max(30.0, 3 * e_f32.max()):
                bad.append(f"max {e_gpu.max():.3g} vs yardstick {e_f32.max():.3g}")
        return bad, msg
