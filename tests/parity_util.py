"""Per-env tolerance bookkeeping for the HIP-vs-oracle (and kernel-vs-kernel) parity tests.

The step's model is piecewise smooth: a drive saturates, a contact opens, and -- since round 6 -- a joint on its speed limit becomes a
prescribed-rate joint (oracle: dynamics_x), each decided by a predictor.  Two implementations whose predictors differ by rounding decide
differently within rounding of a boundary, and the prescribed-rate switch is a jump in the joint's acceleration of up to ~10^3 rad/s^2:
measured (tools/gpu_probe2.py, 512 envs x 40 resynchronised steps) the fp32 kernels AND the oracle's own fp32 build leave the fp64 oracle's
neighbourhood in 1 - 3 of 10^4 env-steps, while median / p99 / p99.9 of the per-env errors are where they were.  The parity tests bound
rounding, not branch flips (DESIGN.md 6 "knife edges"): every env is held to the stated absolute bars except a counted handful per test."""
import numpy as np


class EnvOutliers:
    def __init__(self, n, share=1.5e-3, floor=3):
        self.n, self.share, self.floor = int(n), float(share), int(floor)
        self.total = 0; self.steps = 0
        self._bad = np.zeros(self.n, bool)
        self.worst = {}

    def close(self, got, ref, atol, rtol=0.0, what="", rows=None):
        """rows of got / ref = envs (reshaped to (n, -1)); marks the envs that exceed atol + rtol |ref| anywhere"""
        g = np.asarray(got, np.float64).reshape(self.n, -1); r = np.asarray(ref, np.float64).reshape(self.n, -1)
        err = np.abs(g - r)
        bad = (err > atol + rtol * np.abs(r)).any(1) | ~np.isfinite(g).all(1)
        if rows is not None:
            bad &= np.asarray(rows, bool)
        ok = ~bad
        if ok.any():
            self.worst[what] = max(self.worst.get(what, 0.0), float(err[ok].max()))
        self._bad |= bad
        return bad

    def mark(self, mask):
        """count the envs of `mask` (n,) bool among this step's envs beyond the bars"""
        self._bad |= np.asarray(mask, bool)

    def marked(self):
        """(n,) bool, a copy: the envs beyond the bars in this step so far"""
        return self._bad.copy()

    def end_step(self):
        self.total += int(self._bad.sum()); self.steps += 1
        self._bad[:] = False

    def finish(self):
        if self._bad.any():
            self.end_step()
        budget = max(self.floor, int(np.ceil(self.share * self.n * max(self.steps, 1))))
        assert self.total <= budget, "%d env-steps beyond the bars (budget %d of %d): not rounding near a switch, a difference -- within-bar worst %s" % (
            self.total, budget, self.n * max(self.steps, 1), self.worst)
