"""Configuration of the NL-MO-PPO fixtures (tests/golden/nlppo_*.npz, written by make_golden_nlppo.py from the unmodified reference)."""
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import torch as th

from ppo_cases import reseed, synthetic_moments  # noqa: F401  (the same seeding and synthetic Adam state as MO-PPO's fixtures)

HIDDEN = (64, 64)          # the reference's Agent is 64-64 by construction


def utility(referent, scale):
    """The non-linear utility of these fixtures, in the achievement-scalarising form: with t_k = scale_k * (v_k - referent_k), the
    scaled improvement of objective k over the referent,  u(v) = min_k t_k + 0.1 * mean_k t_k.  Its gradient puts the weight
    scale_k on the objective that is worst off (plus 0.1 * scale / R on every objective), so it changes with v."""
    referent, scale = np.asarray(referent, dtype=np.float32), np.asarray(scale, dtype=np.float32)

    def u(v):
        t = (v - th.as_tensor(referent, dtype=v.dtype)) * th.as_tensor(scale, dtype=v.dtype)
        return t.min() + 0.1 * t.mean()

    u.terms = lambda v: (np.asarray(v, dtype=np.float64) - referent) * scale      # what the min ranges over
    return u


def linear(weights):
    """u(v) = w . v: loss weights that are exactly ``weights`` (the case with a negative one)."""
    w = np.asarray(weights, dtype=np.float32)
    return lambda v: (v * th.as_tensor(w, dtype=v.dtype)).sum()


@dataclass(frozen=True)
class StepCase:
    name: str
    D: int                     # obs_dim
    A: int                     # n_actions
    R: int                     # reward_dim
    pref_dim: int
    M: int                     # minibatch rows (the whole synthetic rollout, visited in a shuffled order)
    seed: int
    with_pref: bool = True     # False: pref=None, the preference columns are zero-filled
    referent: Optional[Tuple[float, ...]] = None       # utility(referent, scale) ...
    scale: Optional[Tuple[float, ...]] = None
    weights: Optional[Tuple[float, ...]] = None        # ... or linear(weights)
    clip_vloss: bool = True
    norm_adv: bool = True
    ent_coef: float = 0.01
    step: int = 5              # optimiser steps taken before the recorded one (non-zero Adam state)
    lr: float = 2.5e-4
    clip_coef: float = 0.2
    vf_coef: float = 0.5
    max_grad_norm: float = 0.5
    mc_k: int = 4              # rows of init_obs
    perturb: float = 0.1       # size of the parameter perturbation the old log-probs / old values come from
    obs_scale: float = 1.0
    ret_scale: float = 1.0     # size of (returns - old values)
    clip_active: bool = True   # the gradient norm is above max_grad_norm

    def u_func(self):
        return linear(self.weights) if self.weights is not None else utility(self.referent, self.scale)


STEP_CASES = [
    StepCase("a", D=6, A=3, R=2, pref_dim=2, M=37, seed=131, referent=(0.1, -0.2), scale=(1.0, 1.5)),          # partial last tile
    StepCase("b", D=4, A=2, R=3, pref_dim=3, M=16, seed=132, with_pref=False, referent=(0.0, 0.1, -0.1), scale=(1.0, 0.8, 1.2)),
    StepCase("c", D=9, A=31, R=4, pref_dim=0, M=50, seed=135, clip_vloss=False, norm_adv=False, weights=(0.6, -0.35, 0.5, 0.25)),
    StepCase("d", D=6, A=3, R=2, pref_dim=2, M=37, seed=134, referent=(0.1, -0.2), scale=(0.02, 0.03), obs_scale=0.05,
             ret_scale=0.05, clip_active=False),                                                                # below max_grad_norm
]
BY_NAME = {c.name: c for c in STEP_CASES}

GAE = dict(seed=141, T=24, E=4, R=3, gamma=0.99, gae_lambda=0.95, done_rate=0.1)

# a whole update(): 96 rows, 4 minibatches of 24, 3 epochs; once to the end, once stopped by target_kl after the second epoch
UPDATE = dict(seed=162, T=24, E=4, D=7, A=4, R=2, pref_dim=2, num_minibatches=4, update_epochs=3, lr=3e-3, gamma=0.99,
              gae_lambda=0.95, perturb=0.03, mc_k=6, referent=(0.05, -0.05), scale=(1.0, 1.3))
UPDATE_KINDS = dict(full=None, kl=0.007)

# a seeded train(): two iterations of 16 steps x 4 envs on tests/nlppo_env.py, pref = the utility's referent
TRACE = dict(seed=161, env=dict(obs_dim=5, n_actions=3, reward_dim=2, horizon=9, seed=7), num_envs=4, iterations=2, eval_episodes=3,
             referent=(0.2, -0.1), scale=(1.0, 0.7),
             agent=dict(num_steps=16, total_timesteps=2 * 16 * 4, num_minibatches=4, update_epochs=2, learning_rate=1e-3,
                        anneal_lr=True, mc_k=6))
