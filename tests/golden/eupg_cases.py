"""The EUPG fixtures' cases, shared by the generator (make_golden_eupg.py) and the tests."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import torch as th

from ppo_cases import reseed, synthetic_moments  # noqa: F401

EPS = float(np.finfo(np.float32).eps)


def utility(r, w=None):
    """A non-linear utility of a return vector: called on a [T][R] tensor of discounted returns by ``update()`` and on a numpy
    [R] vector with ``weights`` for the episodic return.  The product term keeps it from being any weighted sum."""
    if w is None:
        return 0.5 * r[..., 0] * r[..., 1] + 0.25 * (r * r).sum(-1) + r.sum(-1)
    return float(0.5 * r[0] * r[1] + np.dot(w, r))


@dataclass(frozen=True)
class StepCase:
    name: str
    seed: int
    T: int
    D: int
    R: int
    A: int
    hidden: Tuple[int, ...]
    max_workgroups: int = 0
    head_bias0: Optional[float] = None     # bias of the head's action 0
    gamma: float = 0.97
    lr: float = 1e-3
    step: int = 57                         # Adam steps taken before the recorded one
    obs_scale: float = 2.0                 # observations are obs_scale * N(0, 1): far from integers


STEP_CASES = (
    StepCase("a", 11, 37, 5, 2, 3, (50,)),
    StepCase("b", 12, 16, 3, 3, 2, (32, 32)),
    StepCase("c", 13, 70, 5, 2, 3, (50, 33), max_workgroups=2),
    StepCase("d", 11, 1, 5, 2, 3, (50,)),
    StepCase("e", 15, 33, 4, 2, 3, (50,), head_bias0=-25.0),
)
BY_NAME = {c.name: c for c in STEP_CASES}


def episode(c: StepCase):
    """The episode a step case trains on: (obs [T][D] float32, NOT integers; accrued rewards [T][R]; actions [T]; rewards [T][R]).
    The accrued reward of a row is the sum of the rewards before it, as train() forms it."""
    g = th.Generator().manual_seed(c.seed + 1000)
    obs = (c.obs_scale * th.randn(c.T, c.D, generator=g)).numpy()
    rewards = th.randn(c.T, c.R, generator=g).numpy()
    actions = th.randint(0, c.A, (c.T,), generator=g).numpy().astype(np.int32)
    acc = np.zeros((c.T, c.R), dtype=np.float32)
    run = th.zeros(c.R)
    for t in range(c.T):
        acc[t] = run.numpy()
        run += th.from_numpy(rewards[t])
    return obs, acc, actions, rewards


TRACE = dict(seed=5, env=dict(obs_dim=4, n_actions=3, reward_dim=2, horizon=11, seed=3), episodes=4,
             agent=dict(net_arch=[50], gamma=0.95, learning_rate=3e-3), weights=(0.7, 0.3))
