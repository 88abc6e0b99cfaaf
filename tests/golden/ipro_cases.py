"""The IPRO fixtures' inputs, shared by tests/golden/make_golden_ipro.py (which records them through the reference) and the tests:
the ``morl_ipro_hvis`` cases, the point-set cases, the scripted Pareto oracle of the traces and the utilities' inputs."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np


# ---- a. morl_ipro_hvis ------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class HvisCase:
    name: str
    n: int
    R: int
    K: int
    seed: int
    kind: str = "cont"        # "cont": uniform coordinates; "int": a small-integer grid (every product exact: compared with ==)
    exact: bool = False


HVIS_CASES = (
    HvisCase("r1", 3, 1, 5, 1), HvisCase("r2", 12, 2, 7, 2), HvisCase("r3", 14, 3, 9, 3), HvisCase("r4", 10, 4, 6, 4),
    HvisCase("r8_n6", 6, 8, 4, 5), HvisCase("n0_k1", 0, 3, 1, 6), HvisCase("k0", 8, 3, 0, 7), HvisCase("n1", 1, 3, 4, 8),
    HvisCase("edges", 10, 3, 8, 9), HvisCase("int_grid", 24, 3, 12, 10, "int", True), HvisCase("k65", 9, 3, 65, 11),
    HvisCase("n511_r2", 511, 2, 3, 12), HvisCase("run_r3", 25, 3, 33, 13), HvisCase("run_r4", 22, 4, 50, 14),
)


def hvis_inputs(c: HvisCase):
    """(base [n][R], cand [K][R], ref [R]) float64.  Minimisation frame: ``ref`` is the upper corner."""
    rng = np.random.default_rng(1000 + c.seed)
    if c.kind == "int":
        ref = np.full(c.R, 6.0)
        base = rng.integers(2, 8, (c.n, c.R)).astype(np.float64)           # some rows reach or pass ref: dropped
        cand = rng.integers(0, 5, (c.K, c.R)).astype(np.float64)
        return base, cand, ref
    ref = rng.uniform(9.0, 10.0, c.R)
    base = rng.uniform(0.0, 9.0, (c.n, c.R))
    cand = rng.uniform(0.0, 9.0, (c.K, c.R))
    if c.R == 1:
        base = 4.0 + base / 2.0                     # (one objective: the base is its smallest value; keep candidates below it)
    if c.name == "edges":
        cand[0] = base[2]                           # a candidate equal to a base point
        cand[1] = base[3] + 0.25                    # dominated by a base point (minimisation: larger is worse)
        cand[2, 1] = ref[1]                         # one coordinate equal to ref: no volume of its own
        cand[3, 0] = ref[0] + 0.5                   # beyond ref in one coordinate: dropped
        cand[4] = cand[5]                           # two equal candidates
        cand[6] = ref                               # ref itself: dropped
        base[0, 2] = ref[2] + 1.0                   # a base point beyond ref: dropped
        base[1, 0] = ref[0]                         # a base point on ref's face
    return base, cand, ref


# ---- b. update_lower_points / update_upper_points ---------------------------------------------------------------------------
POINT_CASES = ("r2", "r3", "r4", "nothing_dominated", "everything_dominated", "fails_bound", "duplicates", "one_row")


def points_inputs(name):
    """(which, points [m][R], vec [R], nadir [R], ideal [R]); which: "lower" or "upper"."""
    rng = np.random.default_rng(sum(map(ord, name)))
    if name in ("r2", "r3", "r4"):
        R = int(name[1])
        nadir, ideal = np.zeros(R), np.full(R, 10.0)
        pts = np.round(rng.uniform(1.0, 6.0, (6, R)), 2)
        return "lower", pts, np.round(rng.uniform(4.0, 9.0, R), 2), nadir, ideal
    R = 3
    nadir, ideal = np.zeros(R), np.full(R, 10.0)
    if name == "nothing_dominated":
        return "lower", np.array([[5.0, 1.0, 1.0], [1.0, 5.0, 1.0], [1.0, 1.0, 5.0]]), np.array([2.0, 2.0, 2.0]), nadir, ideal
    if name == "everything_dominated":
        return "upper", np.array([[9.0, 8.0, 9.0], [8.0, 9.0, 9.5], [9.5, 9.5, 8.0]]), np.array([3.0, 4.0, 5.0]), nadir, ideal
    if name == "fails_bound":       # vec touches the ideal in one objective: the rows shifted there fail `ideal > shifted`
        return "lower", np.array([[1.0, 1.0, 1.0], [2.0, 0.5, 3.0]]), np.array([10.0, 4.0, 5.0]), nadir, ideal
    if name == "duplicates":        # two rows that differ only where the shift writes: equal rows after it
        return "lower", np.array([[1.0, 2.0, 3.0], [0.5, 2.0, 3.0], [1.0, 1.5, 3.0]]), np.array([4.0, 4.0, 4.0]), nadir, ideal
    if name == "one_row":           # the upper set collapses to a single row (the early return of the filter)
        return "upper", np.array([[10.0, 10.0, 10.0]]), np.array([0.0, 0.0, 5.0]), nadir, ideal
    raise KeyError(name)


# ---- c. the scripted Pareto oracle --------------------------------------------------------------------------------------------
def sphere_table(R, count, seed):
    """``count`` points on the positive unit sphere, times 10, rounded to 3 decimals."""
    v = np.abs(np.random.default_rng(seed).standard_normal((count, R)))
    return np.round(10.0 * v / np.linalg.norm(v, axis=1, keepdims=True), 3)


class Scripted:
    """Stands in for the learner: ``linear`` returns the table's arg-max of ``front @ w``, ``oracle`` the table's best AASF --
    and on every ``weak_every``-th query the fourth best, which provokes ``replay``."""

    def __init__(self, table, weak_every, aug=0.1, scale=100):
        self.table, self.weak_every, self.aug, self.scale = np.asarray(table, dtype=np.float64), weak_every, aug, scale
        self.queries = 0

    def linear(self, w):
        return self.table[int(np.argmax(self.table @ np.asarray(w, dtype=np.float64)))].copy()

    def oracle(self, referent, nadir, ideal, sign):
        referent, nadir, ideal = sign * np.asarray(referent), sign * np.asarray(nadir), sign * np.asarray(ideal)
        frac = self.scale * (self.table - referent) / (ideal - nadir)
        score = np.min(frac, axis=-1) + self.aug * np.mean(frac, axis=-1)
        order = np.argsort(-score, kind="stable")
        self.queries += 1
        pick = order[3] if self.weak_every and self.queries % self.weak_every == 0 else order[0]
        return sign * self.table[int(pick)].copy()


TRACES = {
    # name: objectives, table size, table seed, weak answers, iterations, direction, IPRO seed
    "r3": dict(R=3, count=20, table_seed=3, weak_every=4, iterations=30, direction="maximize", seed=1),
    "r4": dict(R=4, count=20, table_seed=4, weak_every=5, iterations=25, direction="maximize", seed=1),
}
LIVE = {
    "r2": dict(R=2, count=12, table_seed=2, weak_every=4, iterations=30, direction="maximize", seed=1),
    # (with direction="minimize" the reference's init_phase puts the ideal below the nadir whatever the learner returns, and its
    # lower set is empty at once: the run starts from given extrema, the signs of everything after it are under test)
    "r3_min": dict(R=3, count=20, table_seed=3, weak_every=4, iterations=20, direction="minimize", seed=1, extrema=True),
}


def trace_extrema(T):
    """None, or (nadir, ideal) in the outer loop's own (maximising) frame: the table's bounding box, one unit wider."""
    if not T.get("extrema"):
        return None
    t = np.abs(trace_table(T))
    return t.min(axis=0) - 1.0, t.max(axis=0) + 1.0


def trace_table(T):
    t = sphere_table(T["R"], T["count"], T["table_seed"])
    return -t if T["direction"] == "minimize" else t       # costs: the minimising run negates them back


# ---- d. utilities ---------------------------------------------------------------------------------------------------------------
def utility_inputs():
    rng = np.random.default_rng(77)
    f32 = lambda a: np.asarray(a, dtype=np.float32)  # noqa: E731
    batch = f32(rng.uniform(-2.0, 8.0, (6, 5, 3)))
    nadir, ideal = f32([-3.0, -2.5, -4.0]), f32([9.0, 8.5, 10.0])
    referent = f32(rng.uniform(0.0, 4.0, 3))
    weights = f32(rng.uniform(-1.0, 1.0, 3))
    return batch, referent, nadir, ideal, weights
