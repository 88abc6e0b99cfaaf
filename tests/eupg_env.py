"""TEST INFRASTRUCTURE: a small linear multi-objective environment for the EUPG tests.

The action index enters the linear dynamics as a one-hot vector; observations are clipped to [-3, 3] and are NOT integers (the
reference's episode buffer truncates them to int32, so ``update()`` trains on other inputs than acting saw), rewards are linear and
the horizon is FIXED, so no ``done`` depends on rounding.  The spaces are ``momdp``'s, which subclass gymnasium's when one is
imported (the reference tells them apart with ``isinstance``).
"""
import types

import numpy as np

import momdp


class LinearEnv:
    def __init__(self, obs_dim=4, n_actions=3, reward_dim=2, horizon=11, seed=0, env_id="eupg-linear-v0"):
        self.obs_dim, self.n_actions, self.reward_dim, self.horizon = obs_dim, n_actions, reward_dim, horizon
        rng = np.random.default_rng(seed)
        f32 = lambda a: np.asarray(a, dtype=np.float32)  # noqa: E731
        self.Ax = f32(0.9 * np.eye(obs_dim) + 0.1 * rng.standard_normal((obs_dim, obs_dim)))
        self.Au = f32(0.8 * rng.standard_normal((n_actions, obs_dim)))
        self.Cx = f32(0.2 * rng.standard_normal((obs_dim, reward_dim)))
        self.Cu = f32(0.3 * rng.standard_normal((n_actions, reward_dim)))
        self.start = f32(1.5 * rng.standard_normal(obs_dim))
        self.observation_space = momdp.BoxSpace(-3.0, 3.0, (obs_dim,))
        self.action_space = momdp.DiscreteSpace(n_actions)
        self.reward_space = momdp.BoxSpace(-10.0, 10.0, (reward_dim,))
        self.unwrapped = self
        self.spec = types.SimpleNamespace(id=env_id)
        self.action_log, self.reward_log = [], []
        self.obs, self.t = self.start.copy(), 0

    def reset(self, seed=None, options=None):
        self.obs, self.t = self.start.copy(), 0
        return self.obs.copy(), {}

    def step(self, action):
        a = np.eye(self.n_actions, dtype=np.float32)[int(action)]
        self.action_log.append(int(action))
        reward = (self.obs @ self.Cx + a @ self.Cu).astype(np.float32)
        self.obs = np.clip(self.obs @ self.Ax + a @ self.Au, -3.0, 3.0).astype(np.float32)
        self.t += 1
        self.reward_log.append(reward.copy())
        return self.obs.copy(), reward, self.t >= self.horizon, False, {}
