"""TEST INFRASTRUCTURE: a small deterministic vector environment for the MO-PPO ``train()`` trace.

Smooth linear dynamics with clipped observations, linear vector rewards and a FIXED horizon: no ``done`` depends on rounding, so a
replay whose actions differ from the recorded ones by rounding sees the same episode boundaries and rewards that differ by rounding.
The interface is what ``MOPPO`` needs of a vector env: ``num_envs``, ``reset(seed=)`` and ``step(actions)``.
"""
import numpy as np


class LinearVecEnv:
    def __init__(self, num_envs=4, obs_dim=5, action_dim=2, reward_dim=2, horizon=9, seed=0):
        self.num_envs, self.obs_dim, self.action_dim, self.reward_dim, self.horizon = num_envs, obs_dim, action_dim, reward_dim, horizon
        rng = np.random.default_rng(seed)
        f32 = lambda a: np.asarray(a, dtype=np.float32)  # noqa: E731
        self.Ax = f32(0.9 * np.eye(obs_dim) + 0.05 * rng.standard_normal((obs_dim, obs_dim)))
        self.Au = f32(0.3 * rng.standard_normal((action_dim, obs_dim)))
        self.Cx = f32(0.5 * rng.standard_normal((obs_dim, reward_dim)))
        self.Cu = f32(0.2 * rng.standard_normal((action_dim, reward_dim)))
        self.start = f32(0.5 * rng.standard_normal((num_envs, obs_dim)))
        self.action_log, self.reward_log = [], []
        self.obs, self.t = self.start.copy(), np.zeros(num_envs, dtype=np.int64)

    def reset(self, seed=None):
        self.obs = self.start.copy()
        self.t = np.arange(self.num_envs, dtype=np.int64) % 3          # the envs' episodes end at different steps
        return self.obs.copy(), {}

    def step(self, actions):
        a = np.asarray(actions, dtype=np.float32).reshape(self.num_envs, self.action_dim)
        self.action_log.append(a.copy())
        reward = (self.obs @ self.Cx + a @ self.Cu).astype(np.float32)
        self.obs = np.clip(self.obs @ self.Ax + a @ self.Au, -2.0, 2.0).astype(np.float32)
        self.t += 1
        terminated = self.t >= self.horizon
        self.obs[terminated] = self.start[terminated]                  # auto-reset, as a vector env does
        self.t[terminated] = 0
        self.reward_log.append(reward.copy())
        return self.obs.copy(), reward, terminated, np.zeros(self.num_envs, dtype=bool), {}
