"""Configuration of the PCN fixtures (tests/golden/pcn_*.npz, written by make_golden_pcn.py from the unmodified reference)."""
import random
from dataclasses import dataclass

import numpy as np
import torch as th


@dataclass(frozen=True)
class PCNCase:
    name: str
    D: int                 # state_dim
    R: int                 # reward_dim
    A: int                 # action_dim
    B: int                 # batch_size
    H: int                 # hidden_dim
    continuous: bool
    seed: int
    step: int = 3          # optimiser steps taken before the recorded one (non-zero Adam state)
    lr: float = 1e-3
    episodes: int = 12     # synthetic replay: episodes of 3..9 transitions


UPDATE_CASES = [
    PCNCase("disc_b256", D=9, R=2, A=4, B=256, H=64, continuous=False, seed=11),      # the reference's default batch and width
    PCNCase("disc_b50", D=2, R=2, A=4, B=50, H=64, continuous=False, seed=12),        # not a multiple of the 16-row tile
    PCNCase("cont_b256", D=11, R=3, A=3, B=256, H=64, continuous=True, seed=13),
    PCNCase("cont_b37_h128", D=5, R=2, A=2, B=37, H=128, continuous=True, seed=14, step=7),
]
BY_NAME = {c.name: c for c in UPDATE_CASES}

# 50 back-to-back updates (num_model_updates of pcn.py:399) on a replay of random TreasureLine episodes
LOOP = dict(seed=21, n=50, B=256, H=64, lr=1e-3, episodes=20, scaling=np.array([0.1, 0.1, 0.1], dtype=np.float32))

# seeded train() runs: small heaps (max_buffer_size below the episode count, so heappushpop runs), >= 3 iterations
TRACE_DISCRETE = dict(seed=5, env="TreasureLine", agent=dict(learning_rate=3e-3, batch_size=32, hidden_dim=64),
                      scaling=np.array([0.1, 0.1, 0.1], dtype=np.float32),
                      train=dict(total_timesteps=260, num_er_episodes=8, num_step_episodes=12, num_model_updates=6,
                                 max_buffer_size=12, num_points_pf=4, max_return=np.array([5.0, 0.0], dtype=np.float32)))
TRACE_CONTINUOUS = dict(seed=6, env="PointReach", agent=dict(learning_rate=3e-3, batch_size=32, hidden_dim=64, noise=0.1),
                        scaling=np.array([0.1, 0.1, 0.1], dtype=np.float32),
                        train=dict(total_timesteps=280, num_er_episodes=8, num_step_episodes=4, num_model_updates=6,
                                   max_buffer_size=12, num_points_pf=4, max_return=np.array([12.0, 12.0], dtype=np.float32)))
TRACES = dict(discrete=TRACE_DISCRETE, continuous=TRACE_CONTINUOUS)

PARAM_NAMES = ("s_emb.0.weight", "s_emb.0.bias", "c_emb.0.weight", "c_emb.0.bias", "fc.0.weight", "fc.0.bias", "fc.2.weight",
               "fc.2.bias")


def reseed(seed):
    """torch, numpy's global generator (the continuous model's exploration noise, pcn.py:313) and ``random``."""
    random.seed(seed)
    np.random.seed(seed)
    th.manual_seed(seed)


def scaling_of(c: PCNCase):
    return np.linspace(0.1, 0.02, c.R + 1).astype(np.float32)


def synthetic_episodes(c: PCNCase):
    """[(obs, action, reward) per transition] per episode: what the generator stores in the reference's replay (rewards BEFORE
    the return-to-go accumulation of pcn.py:240-241)."""
    rng = np.random.default_rng(c.seed + 1000)
    eps = []
    for _ in range(c.episodes):
        n = int(rng.integers(3, 10))
        ep = []
        for _ in range(n):
            obs = rng.standard_normal(c.D).astype(np.float32)
            action = rng.uniform(-1, 1, c.A).astype(np.float32) if c.continuous else int(rng.integers(c.A))
            reward = rng.standard_normal(c.R).astype(np.float32)
            ep.append((obs, action, reward))
        eps.append(ep)
    return eps


def synthetic_moments(c: PCNCase, shapes):
    """Adam moments of a learner ``c.step`` steps into training (sizes typical of this model's gradients)."""
    g = th.Generator().manual_seed(c.seed + 2000)
    m = [th.randn(s, generator=g) * 1e-3 for s in shapes]
    v = [th.rand(s, generator=g) * 1e-5 + 1e-8 for s in shapes]
    return m, v
