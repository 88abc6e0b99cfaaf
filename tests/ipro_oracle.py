"""TEST INFRASTRUCTURE: numpy restatement of IPRO's outer loop (``multi_policy/ipro/ipro.py``, ``outer_loop.py``) with the hypervolume
and the two trainings as callables.  tests/golden/make_golden_ipro.py checks it against every value recorded from the reference
(``==`` for the sets, 1e-12 for the volumes); the tests then hold the package's ``IPRO`` to it.

``hv(points, ref)``: ``OuterLoop.compute_hypervolume`` -- minimisation frame, points that ``ref`` does not dominate dropped.
``hv_plus(base, point_or_None, ref)``: the hypervolume of ``base`` with one more point (``compute_hvis``) or as it is
(``discarded_hv``); by default ``hv`` of the stacked rows.  ``linear(w)`` and ``oracle(referent, nadir, ideal, sign)`` return the
vector a training would, in the environment's frame.
"""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import metrics_oracle as mo  # noqa: E402


def dominates(a, b):
    return np.logical_and(np.all(a >= b, axis=-1), np.any(a > b, axis=-1))


def strictly(a, b):
    return np.all(np.asarray(a) > np.asarray(b), axis=-1)


def oracle_hv(points, ref):
    """float64 oracle in ``compute_hypervolume``'s frame: metrics_oracle.hypervolume maximises, so both sides are negated."""
    points, ref = np.asarray(points, dtype=np.float64).reshape(-1, len(ref)), np.asarray(ref, dtype=np.float64)
    points = points[dominates(ref, points)]
    if points.size == 0:
        return 0
    return mo.hypervolume(-ref, list(-points))


def non_dominated(c):
    """``common/pareto.py:34-73`` (``filter_pareto_dominated``): maximal rows, the first of equal rows; fewer than two rows pass."""
    c = np.array(c)
    if len(c) < 2:
        return c
    keep = np.ones(len(c), dtype=bool)
    for i in range(len(c)):
        keep[i] = not np.any(dominates(c, c[i])) and not np.any(np.all(c[:i] == c[i], axis=1))
    return c[keep]


def aasf(batch, referent, nadir, ideal, aug=0.0, scale=100):
    """``outer_loop.py:47-51`` on numpy arrays of one dtype."""
    frac = scale * (batch - referent) / (ideal - nadir)
    return np.min(frac, axis=-1) + aug * np.mean(frac, axis=-1, dtype=frac.dtype)


STATE = ("pf", "completed", "robust_points", "lower_points", "upper_points")
SCALARS = ("hv", "dominated_hv", "discarded_hv", "coverage", "error", "replay_triggered")


class Loop:
    def __init__(self, dim, linear, oracle, hv=oracle_hv, hv_plus=None, direction="maximize", offset=1, tolerance=1e-6,
                 max_iterations=None, update_freq=1, seed=1):
        self.dim, self.linear, self.oracle, self.hv_fn = dim, linear, oracle, hv
        self.hv_plus = hv_plus or (lambda base, p, ref: hv(base if p is None else np.vstack((base, p)), ref))
        self.sign = 1 if direction == "maximize" else -1
        self.offset, self.tolerance, self.update_freq = offset, tolerance, update_freq
        self.max_iterations = max_iterations if max_iterations is not None else np.inf
        self.rng = np.random.default_rng(seed)
        self.ref_point = None
        self.log = []            # one dict per iteration: referent, vec, the sets and the scalars
        self.reset()

    def reset(self):
        self.lower_points, self.upper_points = [], []
        self.nadir = self.ideal = None
        self.pf = np.empty((0, self.dim))
        self.robust_points = np.empty((0, self.dim))
        self.completed = np.empty((0, self.dim))
        self.hv = self.total_hv = self.dominated_hv = self.discarded_hv = self.coverage = 0
        self.error = np.inf
        self.replay_triggered = 0

    # -- ipro.py ----------------------------------------------------------------------------------------------------------
    def init_phase(self, extrema=None):
        subsolutions = []
        if extrema is None:
            nadir, ideal, pf = np.zeros(self.dim), np.zeros(self.dim), []
            for i, w in enumerate(np.eye(self.dim)):
                ideal_vec = self.linear(w)
                nadir_vec = self.linear(-1 * w)
                ideal_vec *= self.sign
                nadir_vec *= self.sign
                ideal[i], nadir[i] = ideal_vec[i], nadir_vec[i]
                pf.append(ideal_vec)
                subsolutions.append((w, ideal_vec, None))
            self.pf = non_dominated(np.array(pf))
            self.nadir, self.ideal = np.copy(nadir - self.offset), np.copy(ideal + self.offset)
            if len(self.pf) == 1:
                return subsolutions, True
        else:
            self.nadir, self.ideal = extrema
        self.ref_point = np.copy(self.nadir) if self.ref_point is None else np.array(self.ref_point)
        self.hv = self.hv_fn(-self.sign * self.pf, -self.sign * self.ref_point)
        self.total_hv = abs(np.prod(np.max([self.nadir, self.ideal], axis=0) - np.min([self.nadir, self.ideal], axis=0)))
        self.lower_points = np.array([self.nadir])
        for point in self.pf:
            self.update_lower_points(np.array(point))
        self.upper_points = np.array([self.ideal])
        self.error = max(self.ideal - self.nadir)
        self.compute_hvis()
        return subsolutions, False

    def compute_hvis(self, num=50):
        base = np.vstack((self.pf, self.completed))
        hvis = np.zeros(len(self.lower_points))
        for i in self.rng.choice(len(self.lower_points), min(num, len(self.lower_points)), replace=False):
            hvis[i] = self.hv_plus(base, self.lower_points[i], self.ideal)
        self.last_hvis = hvis
        self.lower_points = self.lower_points[np.argsort(hvis)[::-1]]

    def estimate_error(self):
        if len(self.upper_points) == 0:
            self.error = 0
        else:
            diffs = self.upper_points[:, None, :] - np.array(list(self.pf))[None, :, :]
            self.error = np.max(np.min(np.max(diffs, axis=2), axis=1))

    def _shift(self, points, dominated, vec):
        shifted = np.stack([points[dominated == 1]] * self.dim)
        shifted[range(self.dim), :, range(self.dim)] = np.expand_dims(vec, -1)
        return points[dominated == 0], shifted.reshape(-1, self.dim)

    def update_upper_points(self, vec):
        keep, shifted = self._shift(self.upper_points, strictly(self.upper_points, vec), vec)
        shifted = shifted[np.all(shifted > self.nadir, axis=-1)]
        self.upper_points = non_dominated(np.vstack((keep, shifted)))

    def update_lower_points(self, vec):
        keep, shifted = self._shift(self.lower_points, strictly(vec, self.lower_points), vec)
        shifted = shifted[np.all(self.ideal > shifted, axis=-1)]
        self.lower_points = -non_dominated(-np.vstack((keep, shifted)))

    def update_found(self, vec):
        self.pf = np.vstack((self.pf, vec))
        self.update_lower_points(vec)
        self.update_upper_points(vec)

    def update_not_found(self, referent, vec):
        self.completed = np.vstack((self.completed, referent))
        self.lower_points = self.lower_points[np.any(self.lower_points != referent, axis=1)]
        self.update_upper_points(referent)
        if strictly(vec, self.nadir):
            self.robust_points = np.vstack((self.robust_points, vec))

    def update_excluded_volume(self):
        self.dominated_hv = self.hv_fn(-self.pf, -self.nadir)
        self.discarded_hv = self.hv_plus(np.vstack((self.pf, self.completed)), None, self.ideal)

    # -- outer_loop.py ----------------------------------------------------------------------------------------------------
    def replay(self, vec, pairs):
        """pairs: (referent, vec, sol); ``sol`` is None, or the vector again where the reference stores it (outer_loop.py:340)."""
        triggered, nadir, ideal = self.replay_triggered, self.nadir, self.ideal
        self.reset()
        self.replay_triggered = triggered + 1
        self.init_phase(extrema=(nadir, ideal))
        idx, out = 0, []
        for referent, old_vec, old_sol in pairs:
            idx += 1
            if strictly(old_vec, referent):
                if strictly(vec, old_vec):
                    self.update_found(vec)
                    out.append((referent, vec, None))
                    break
                self.update_found(old_vec)
                out.append((referent, old_vec, old_sol))
            else:
                if strictly(vec, referent):
                    self.update_found(vec)
                    out.append((referent, vec, None))
                    break
                self.update_not_found(referent, old_vec)
                out.append((referent, old_vec, old_vec))
        for referent, old_vec, old_sol in pairs[idx:]:
            found = strictly(old_vec, referent)
            for lower in np.copy(self.lower_points):
                if found and strictly(old_vec, lower):
                    self.update_found(old_vec)
                elif not found and dominates(lower, referent):
                    self.update_not_found(lower, old_vec)
                else:
                    continue
                out.append((lower, old_vec, old_sol))
                break
        return out

    def snapshot(self, referent, vec):
        rec = {k: np.array(getattr(self, k), dtype=np.float64).reshape(-1, self.dim) for k in STATE}
        rec.update({k: float(getattr(self, k)) for k in SCALARS})
        rec["referent"], rec["vec"] = np.array(referent), np.array(vec)
        self.log.append(rec)

    def train(self, ref_point, extrema=None):
        self.ref_point = ref_point
        linear_subsolutions, done = self.init_phase(extrema=extrema)
        if done:
            return self.pareto_set(linear_subsolutions)
        iteration, pairs = 0, []
        while not (1 - self.coverage <= self.tolerance or iteration >= self.max_iterations):
            if iteration % self.update_freq == 0:
                self.compute_hvis()
            referent = self.lower_points[0]
            vec = self.oracle(referent, self.nadir, self.ideal, self.sign)
            if strictly(vec, referent):
                if np.any(strictly(vec, np.vstack((self.pf, self.completed)))):
                    pairs = self.replay(vec, pairs)
                else:
                    self.update_found(vec)
                    pairs.append((referent, vec, None))
            else:
                if np.any(strictly(vec, self.completed)):
                    pairs = self.replay(vec, pairs)
                else:
                    self.update_not_found(referent, vec)
                    pairs.append((referent, vec, None))
            self.update_excluded_volume()
            self.estimate_error()
            self.coverage = (self.dominated_hv + self.discarded_hv) / self.total_hv
            self.hv = self.hv_fn(-self.sign * self.pf, -self.sign * self.ref_point)
            iteration += 1
            self.snapshot(referent, vec)
        self.pf = non_dominated(np.vstack((self.pf, self.robust_points)))
        self.dominated_hv = self.hv_fn(-self.sign * self.pf, -self.sign * self.nadir)
        self.hv = self.hv_fn(-self.sign * self.pf, -self.sign * self.ref_point)
        self.snapshot(np.full(self.dim, np.nan), np.full(self.dim, np.nan))      # the state finish() leaves
        return self.pareto_set(linear_subsolutions + pairs)

    def pareto_set(self, subsolutions):
        return [self.sign * s[1] for s in subsolutions if np.any(np.all(np.isclose(s[1], self.pf), axis=1))]
