"""TEST INFRASTRUCTURE: the discrete twin of ``ppo_env.LinearVecEnv`` for the NL-MO-PPO tests.

The action index enters the linear dynamics as a one-hot vector; observations are clipped, rewards are linear and the horizon is
FIXED, so no ``done`` depends on rounding.  ``DiscreteLinearVecEnv`` has what ``NLMOPPO`` needs of a vector env (``num_envs``,
``single_observation_space``, ``single_action_space.n``, ``reward_space``, ``reset(seed=)``, ``step(actions)``);
``DiscreteLinearEnv`` is the one-env form that ``policy_evaluate`` steps with a plain action index.
"""
import types

import numpy as np


def _matrices(obs_dim, n_actions, reward_dim, seed):
    rng = np.random.default_rng(seed)
    f32 = lambda a: np.asarray(a, dtype=np.float32)  # noqa: E731
    return types.SimpleNamespace(
        Ax=f32(0.9 * np.eye(obs_dim) + 0.05 * rng.standard_normal((obs_dim, obs_dim))),
        Au=f32(0.3 * rng.standard_normal((n_actions, obs_dim))),
        Cx=f32(0.5 * rng.standard_normal((obs_dim, reward_dim))),
        Cu=f32(0.2 * rng.standard_normal((n_actions, reward_dim))),
        rng=rng)


def _spaces(env, obs_dim, n_actions, reward_dim):
    env.single_observation_space = env.observation_space = types.SimpleNamespace(shape=(obs_dim,))
    env.single_action_space = env.action_space = types.SimpleNamespace(n=n_actions, shape=())
    env.reward_space = types.SimpleNamespace(shape=(reward_dim,))


class DiscreteLinearVecEnv:
    def __init__(self, num_envs=4, obs_dim=5, n_actions=3, reward_dim=2, horizon=9, seed=0):
        self.num_envs, self.obs_dim, self.n_actions, self.reward_dim, self.horizon = num_envs, obs_dim, n_actions, reward_dim, horizon
        self.m = _matrices(obs_dim, n_actions, reward_dim, seed)
        self.start = np.asarray(0.5 * self.m.rng.standard_normal((num_envs, obs_dim)), dtype=np.float32)
        _spaces(self, obs_dim, n_actions, reward_dim)
        self.action_log, self.reward_log = [], []
        self.obs, self.t = self.start.copy(), np.zeros(num_envs, dtype=np.int64)

    def reset(self, seed=None):
        # (the seed shifts the start states, so the reset(seed + i) calls that build init_obs see different observations)
        shift = np.float32(0.0 if seed is None else 0.01 * (int(seed) % 7))
        self.obs = (self.start + shift).astype(np.float32)
        self.t = np.arange(self.num_envs, dtype=np.int64) % 3          # the envs' episodes end at different steps
        return self.obs.copy(), {}

    def step(self, actions):
        idx = np.asarray(actions, dtype=np.int64).reshape(self.num_envs)
        self.action_log.append(idx.copy())
        a = np.eye(self.n_actions, dtype=np.float32)[idx]
        reward = (self.obs @ self.m.Cx + a @ self.m.Cu).astype(np.float32)
        self.obs = np.clip(self.obs @ self.m.Ax + a @ self.m.Au, -2.0, 2.0).astype(np.float32)
        self.t += 1
        terminated = self.t >= self.horizon
        self.obs[terminated] = self.start[terminated]                  # auto-reset, as a vector env does
        self.t[terminated] = 0
        self.reward_log.append(reward.copy())
        return self.obs.copy(), reward, terminated, np.zeros(self.num_envs, dtype=bool), {}


class SpacesVecEnv:
    """Spaces and a seeded ``reset`` only (no dynamics): what constructing a learner for a fixture's shapes needs -- the
    constructor draws ``init_obs`` from ``reset(seed=seed + i)``."""

    def __init__(self, num_envs, obs_dim, n_actions, reward_dim, obs_scale=1.0):
        self.num_envs, self.obs_dim, self.obs_scale = num_envs, obs_dim, obs_scale
        _spaces(self, obs_dim, n_actions, reward_dim)

    def reset(self, seed=None):
        rng = np.random.default_rng(seed)
        return (self.obs_scale * rng.standard_normal((self.num_envs, self.obs_dim))).astype(np.float32), {}


class DiscreteLinearEnv:
    """One env of the same dynamics: ``reset(seed=)`` -> (obs [D], {}), ``step(int)`` -> (obs, reward [R], terminated, truncated, {})."""

    def __init__(self, obs_dim=5, n_actions=3, reward_dim=2, horizon=9, seed=0):
        self.obs_dim, self.n_actions, self.reward_dim, self.horizon = obs_dim, n_actions, reward_dim, horizon
        self.m = _matrices(obs_dim, n_actions, reward_dim, seed)
        self.start = np.asarray(0.5 * self.m.rng.standard_normal(obs_dim), dtype=np.float32)
        _spaces(self, obs_dim, n_actions, reward_dim)
        self.action_log = []
        self.obs, self.t = self.start.copy(), 0

    def reset(self, seed=None):
        self.obs, self.t = self.start.copy(), 0
        return self.obs.copy(), {}

    def step(self, action):
        a = np.eye(self.n_actions, dtype=np.float32)[int(action)]
        self.action_log.append(int(action))
        reward = (self.obs @ self.m.Cx + a @ self.m.Cu).astype(np.float32)
        self.obs = np.clip(self.obs @ self.m.Ax + a @ self.m.Au, -2.0, 2.0).astype(np.float32)
        self.t += 1
        return self.obs.copy(), reward, self.t >= self.horizon, False, {}
