"""TEST INFRASTRUCTURE: the environments of the PGMORL tests.

``PGVecEnv`` is ``ppo_env.LinearVecEnv`` with the spaces ``PGMORL`` reads its shapes from and a constant added to the rewards
(returns away from zero: the predictor's neighbourhoods are relative to the evaluation); ``PGEvalEnv`` is its single-env twin
for ``policy_eval`` (the same linear dynamics and rewards, MO-Gymnasium's ``reset()`` / ``step(action)`` signature, a fixed
horizon).  Neither draws random numbers after construction, so ``reset(seed)`` determines the episode stream."""
import numpy as np

import momdp
from ppo_env import LinearVecEnv


class PGVecEnv(LinearVecEnv):
    def __init__(self, offset=None, **kw):
        super().__init__(**kw)
        self.offset = np.zeros(self.reward_dim, dtype=np.float32) if offset is None else np.asarray(offset, dtype=np.float32)
        self.single_observation_space = momdp.BoxSpace(-2.0, 2.0, (self.obs_dim,))
        self.single_action_space = momdp.BoxSpace(-10.0, 10.0, (self.action_dim,))
        self.reward_space = momdp.BoxSpace(-10.0, 10.0, (self.reward_dim,))

    def step(self, actions):
        obs, reward, terminated, truncated, info = super().step(actions)
        reward = (reward + self.offset).astype(np.float32)
        self.reward_log[-1] = reward.copy()
        return obs, reward, terminated, truncated, info

    def close(self):
        pass


class PGEvalEnv:
    """Env 0 of a ``LinearVecEnv`` with the same construction arguments, one episode of ``horizon`` steps per ``reset()``."""

    def __init__(self, offset=None, **kw):
        v = LinearVecEnv(**kw)
        self.Ax, self.Au, self.Cx, self.Cu, self.start, self.horizon = v.Ax, v.Au, v.Cx, v.Cu, v.start[0].copy(), v.horizon
        self.offset = np.zeros(v.reward_dim, dtype=np.float32) if offset is None else np.asarray(offset, dtype=np.float32)
        self.observation_space = momdp.BoxSpace(-2.0, 2.0, (v.obs_dim,))
        self.action_space = momdp.BoxSpace(-10.0, 10.0, (v.action_dim,))
        self.reward_space = momdp.BoxSpace(-10.0, 10.0, (v.reward_dim,))
        self.unwrapped = self
        self.obs, self.t = self.start.copy(), 0

    def reset(self, seed=None, options=None):
        self.obs, self.t = self.start.copy(), 0
        return self.obs.copy(), {}

    def step(self, action):
        a = np.asarray(action, dtype=np.float32).reshape(-1)
        reward = (self.obs @ self.Cx + a @ self.Cu + self.offset).astype(np.float32)
        self.obs = np.clip(self.obs @ self.Ax + a @ self.Au, -2.0, 2.0).astype(np.float32)
        self.t += 1
        return self.obs.copy(), reward, self.t >= self.horizon, False, {}

    def close(self):
        pass
