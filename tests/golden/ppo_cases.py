"""Configuration of the MO-PPO fixtures (tests/golden/ppo_*.npz, written by make_golden_ppo.py from the unmodified reference)."""
import random
from dataclasses import dataclass
from typing import Tuple

import numpy as np
import torch as th


@dataclass(frozen=True)
class StepCase:
    name: str
    D: int                     # obs_dim
    A: int                     # action_dim
    R: int                     # reward_dim
    hidden: Tuple[int, ...]
    M: int                     # minibatch rows (the whole synthetic rollout, visited in a shuffled order)
    seed: int
    clip_vloss: bool = True
    norm_adv: bool = True
    ent_coef: float = 0.0
    step: int = 5              # optimiser steps taken before the recorded one (non-zero Adam state)
    lr: float = 3e-4
    clip_coef: float = 0.2
    vf_coef: float = 0.5
    max_grad_norm: float = 0.5
    perturb: float = 0.15      # size of the parameter perturbation the old log-probs / old values come from
    obs_scale: float = 1.0
    ret_scale: float = 1.0     # size of (returns - old values)
    logstd: float = 0.0        # actor_logstd of the recorded parameters
    clip_active: bool = True   # the gradient norm is above max_grad_norm


STEP_CASES = [
    StepCase("a_m37", D=11, A=3, R=2, hidden=(64, 64), M=37, seed=31, perturb=0.07),                                   # partial last tile
    StepCase("b_m16_h32", D=5, A=1, R=3, hidden=(32,), M=16, seed=32),                                   # one hidden layer, one tile
    StepCase("c_m50_h128_96", D=17, A=6, R=4, hidden=(128, 96), M=50, seed=33, clip_vloss=False, norm_adv=False, ent_coef=0.01,
             perturb=0.03),
    StepCase("d_m37_small", D=11, A=3, R=2, hidden=(64, 64), M=37, seed=34, obs_scale=0.05, ret_scale=0.05, logstd=1.5,
             clip_active=False),                                                                         # below max_grad_norm
]
BY_NAME = {c.name: c for c in STEP_CASES}

GAE = dict(seed=41, T=24, E=4, R=2, D=7, A=2, hidden=(32,), gamma=0.995, gae_lambda=0.95, done_rate=0.1)

# a whole update(): 96 rows, 4 minibatches of 24, 3 epochs; once to the end, once stopped by target_kl after the second epoch
UPDATE = dict(seed=58, T=24, E=4, D=7, A=2, R=2, hidden=(64, 64), num_minibatches=4, update_epochs=3, lr=3e-3, gamma=0.995,
              gae_lambda=0.95, perturb=0.05)
UPDATE_KINDS = dict(full=None, kl=0.05)

# a seeded train(): two iterations of 16 steps x 4 envs on tests/ppo_env.py
TRACE = dict(seed=61, env=dict(num_envs=4, obs_dim=5, action_dim=2, reward_dim=2, horizon=9, seed=7), hidden=(32, 32),
             weights=np.array([0.7, 0.3], dtype=np.float32), iterations=2,
             agent=dict(steps_per_iteration=16, num_minibatches=4, update_epochs=2, learning_rate=1e-3, anneal_lr=True))


def reseed(seed):
    random.seed(seed)
    np.random.seed(seed)
    th.manual_seed(seed)


def synthetic_moments(seed, P):
    """Flat Adam moments of a learner some steps into training (sizes typical of clipped gradients)."""
    g = th.Generator().manual_seed(seed + 2000)
    m = th.randn(P, generator=g) * 1e-3
    v = th.rand(P, generator=g) * 1e-5 + 1e-8
    return m.numpy(), v.numpy()
