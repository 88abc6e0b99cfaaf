"""Configuration of the LCN fixtures (tests/golden/lcn_*.npz, written by make_golden_lcn.py from the unmodified reference)."""
from dataclasses import dataclass
from typing import Optional

import numpy as np

from pcn_cases import reseed  # noqa: F401  (the LCN traces reseed as the PCN ones do)

MODE_OF = {"pareto": 0, "nondominated": 1, "lambda_lorenz": 2}


@dataclass(frozen=True)
class SelectCase:
    name: str
    N: int
    R: int
    family: str            # "int": small-integer returns, duplicates and ties everywhere; "cont": continuous returns
    distance_ref: str      # "nondominated" (mode 1) or "lambda_lorenz" (mode 2)
    lcn_lambda: Optional[float] = None
    threshold: float = 0.2
    seed: int = 0


def select_returns(N, R, family, seed):
    """float32 [N][R].  Every row is a floor m plus extras whose range shrinks as m grows -- the poorest objective trades against
    the total, so the Lorenz front has more than one point -- in a random objective order, so that different rows share a
    Lorenz vector.  "int": small integers: equal rows, equal Lorenz vectors and tied distances are the normal case; "cont":
    continuous draws of mixed scale, every fifth row repeated from an earlier one."""
    rng = np.random.default_rng(1000 + seed)
    if family == "int":
        m = rng.integers(0, 5, size=(N, 1))
        x = (m + rng.integers(0, 3 * (4 - m) + 1, size=(N, R))).astype(np.float32)
        x[:, 0] = m[:, 0]
    else:
        m = rng.uniform(0.0, 1.0, size=(N, 1))
        x = m + rng.uniform(0.0, 1.0, size=(N, R)) * 3.0 * (1.0 - m)
        x[:, 0] = m[:, 0]
        x = (x * rng.choice([0.1, 1.0, 30.0])).astype(np.float32)
    x = rng.permuted(x, axis=1)
    if family == "cont":
        for i in range(4, N, 5):
            x[i] = x[rng.integers(0, i)]
    return x


# recorded from the reference's own _nlargest: both of its modes, R in {1, 2, 3, 7, 8}, N up to 600 (file size)
SELECT_CASES = [
    SelectCase("int_n65_r2", 65, 2, "int", "nondominated", seed=1),
    SelectCase("int_n257_r3", 257, 3, "int", "nondominated", seed=2),
    SelectCase("int_n500_r3_lam", 500, 3, "int", "lambda_lorenz", lcn_lambda=0.5, seed=3),
    SelectCase("int_n300_r8", 300, 8, "int", "nondominated", seed=4),
    SelectCase("int_n129_r7_lam", 129, 7, "int", "lambda_lorenz", lcn_lambda=0.9, seed=5),     # f32(1 - 0.9) != 1 - f32(0.9)
    SelectCase("cont_n500_r3", 500, 3, "cont", "nondominated", seed=6),
    SelectCase("cont_n257_r8_lam", 257, 8, "cont", "lambda_lorenz", lcn_lambda=0.3, seed=7),
    SelectCase("cont_n65_r7", 65, 7, "cont", "nondominated", seed=8),
    SelectCase("cont_n600_r2_lam", 600, 2, "cont", "lambda_lorenz", lcn_lambda=0.75, seed=9),
    SelectCase("cont_n40_r1", 40, 1, "cont", "nondominated", seed=10),
    SelectCase("int_n33_r1_lam", 33, 1, "int", "lambda_lorenz", lcn_lambda=0.5, seed=11),
    SelectCase("cont_n500_r8", 500, 8, "cont", "nondominated", threshold=0.05, seed=12),
]
SELECT_BY_NAME = {c.name: c for c in SELECT_CASES}

# _choose_commands on a fixed heap: synthetic episodes with integer returns, heap smaller than their number
COMMANDS = dict(seed=31, episodes=40, max_size=24, num_episodes=10, R=3, cd_threshold=0.2,
                variants=dict(nondominated=dict(distance_ref="nondominated", lcn_lambda=None),
                              lambda_lorenz=dict(distance_ref="lambda_lorenz", lcn_lambda=0.5)))


def command_episodes():
    """[(obs, action, reward) per transition] per episode; rewards are small integers, so returns tie."""
    C = COMMANDS
    rng = np.random.default_rng(C["seed"])
    eps = []
    for _ in range(C["episodes"]):
        n = int(rng.integers(3, 8))
        eps.append([(rng.standard_normal(4).astype(np.float32), int(rng.integers(3)),
                     rng.integers(0, 3, size=C["R"]).astype(np.float32)) for _ in range(n)])
    return eps


# seeded train() runs: heaps smaller than the episode count (heappushpop runs), >= 3 iterations, LCN's constructor defaults
# for the learning rate / batch / width
_SC = np.array([0.1, 0.1, 0.1], dtype=np.float32)
TRACE_NONDOMINATED = dict(seed=5, env="TreasureLine", kind="discrete",
                          agent=dict(distance_ref="nondominated"), scaling=_SC,
                          train=dict(total_timesteps=260, num_er_episodes=8, num_step_episodes=12, num_model_updates=6,
                                     max_buffer_size=12, num_points_pf=4, max_return=np.array([5.0, 0.0], dtype=np.float32),
                                     cd_threshold=0.2))
TRACE_LAMBDA = dict(seed=5, env="TreasureLine", kind="discrete",
                    agent=dict(distance_ref="lambda_lorenz", lcn_lambda=0.5), scaling=_SC,
                    train=dict(total_timesteps=260, num_er_episodes=8, num_step_episodes=12, num_model_updates=6,
                               max_buffer_size=12, num_points_pf=4, max_return=np.array([5.0, 0.0], dtype=np.float32),
                               cd_threshold=0.2))
TRACE_CONTINUOUS = dict(seed=6, env="PointReach", kind="continuous",
                        agent=dict(distance_ref="nondominated", noise=0.1), scaling=_SC,
                        train=dict(total_timesteps=280, num_er_episodes=8, num_step_episodes=4, num_model_updates=6,
                                   max_buffer_size=12, num_points_pf=4, max_return=np.array([12.0, 12.0], dtype=np.float32),
                                   cd_threshold=0.2))
TRACES = dict(nondominated=TRACE_NONDOMINATED, lambda_lorenz=TRACE_LAMBDA, continuous=TRACE_CONTINUOUS)
