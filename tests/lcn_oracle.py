"""TEST INFRASTRUCTURE: a numpy restatement of what Lorenz Conditioned Networks (``multi_policy/lcn/lcn.py`` of the reference) add
to PCN -- ``lorenz_vector``, ``_nlargest``, ``_choose_commands`` and the training loop's arguments -- independent of the package
under test.  Everything LCN shares with PCN (model, update, acting, heap) is imported from ``tests/pcn_oracle.py``.
``tests/golden/make_golden_lcn.py`` pins it to the unmodified reference with exact equality; the kernel tests, the agent tests
and ``bench_ac.py``'s numpy leg are measured against it.
"""
from __future__ import annotations

import heapq

import numpy as np

import pcn_oracle as po
from pcn_oracle import crowding_distance, get_non_dominated_inds

MODES = {"pareto": 0, "nondominated": 1, "lambda_lorenz": 2}


def lorenz_vector(points, proportional=False):
    """lcn.py:26-45."""
    sorted_points = np.sort(points, axis=1)
    lv = np.cumsum(sorted_points, axis=1)
    if proportional:
        lv = lv / np.sum(points, axis=1, keepdims=True)
    return lv


def front_mask(returns, mode, lcn_lambda=None):
    """The dominance filter of lcn.py:226-236 (mode 0: PCN's, pcn.py:255) and the rows the distances are taken on."""
    if mode == 2:
        assert lcn_lambda is not None, "lcn_lambda must be set when using distance_ref='lambda_lorenz'"
        returns = np.sort(returns, axis=1)
        lv = lorenz_vector(returns)
        fv = lcn_lambda * returns + (1 - lcn_lambda) * lv
        return get_non_dominated_inds(fv), returns
    if mode == 1:
        return get_non_dominated_inds(lorenz_vector(returns)), returns
    return get_non_dominated_inds(returns), returns


def score(returns, threshold, mode, lcn_lambda=None, crowded=None):
    """lcn.py:221-252 on an array of returns: (l2, front mask, crowded mask).  ``crowded``: use these flags instead of the
    crowding distance (which the reference cannot form for a single point)."""
    if crowded is None:
        distances = crowding_distance(returns)
        sma = np.argwhere(distances <= threshold).flatten()
    else:
        sma = np.nonzero(crowded)[0]
    non_dominated_i, returns = front_mask(returns, mode, lcn_lambda)
    mask = non_dominated_i.copy()
    non_dominated = returns[non_dominated_i]
    returns_exp = np.tile(np.expand_dims(returns, 1), (1, len(non_dominated), 1))
    l2 = np.min(np.linalg.norm(returns_exp - non_dominated, axis=-1), axis=-1) * -1
    non_dominated_i = np.nonzero(non_dominated_i)[0]
    _, unique_i = np.unique(non_dominated, axis=0, return_index=True)
    unique_i = non_dominated_i[unique_i]
    duplicates = np.ones(len(l2), dtype=bool)
    duplicates[unique_i] = False
    l2[duplicates] -= 1e-5
    l2[sma] *= 2
    crowded = np.zeros(len(l2), dtype=np.uint8)
    crowded[sma] = 1
    return l2, mask, crowded


def nlargest(replay, n, threshold=0.2, distance_ref="nondominated", lcn_lambda=None):
    """lcn.py:213-260 (re-scores and re-heapifies ``replay`` in place)."""
    returns = np.array([e[2][0].reward for e in replay])
    l2, _, _ = score(returns, threshold, MODES[distance_ref], lcn_lambda)
    sorted_i = np.argsort(l2)
    largest = [replay[i] for i in sorted_i[-n:]]
    for i in range(len(l2)):
        replay[i] = (l2[i], replay[i][1], replay[i][2])
    heapq.heapify(replay)
    return largest


def choose_commands(replay, np_random, num_episodes, cd_threshold, distance_ref="nondominated", lcn_lambda=None):
    """lcn.py:262-282: the second filter is strict Lorenz dominance whatever ``distance_ref`` is."""
    episodes = nlargest(replay, num_episodes, cd_threshold, distance_ref, lcn_lambda)
    returns, horizons = list(zip(*[(e[2][0].reward, len(e[2])) for e in episodes]))
    lv = lorenz_vector(np.array(returns))
    nd_i = get_non_dominated_inds(lv)
    returns = np.array(returns)[nd_i]
    horizons = np.array(horizons)[nd_i]
    r_i = np_random.integers(0, len(returns))
    desired_horizon = np.float32(horizons[r_i] - 2)
    _, s = np.mean(returns, axis=0), np.std(returns, axis=0)
    desired_return = returns[r_i].copy()
    r_i = np_random.integers(0, len(desired_return))
    desired_return[r_i] += np_random.uniform(high=s[r_i])
    return np.float32(desired_return), desired_horizon


class Agent(po.Agent):
    """lcn.py:69-146, 342-358, 372-529 without logging / checkpoint files."""

    def __init__(self, env, scaling_factor, learning_rate=1e-2, gamma=1.0, batch_size=32, hidden_dim=64, noise=0.1,
                 distance_ref="nondominated", lcn_lambda=None, seed=None, act_dtype=None):
        super().__init__(env, scaling_factor, learning_rate=learning_rate, gamma=gamma, batch_size=batch_size, hidden_dim=hidden_dim,
                         noise=noise, seed=seed, act_dtype=act_dtype)
        self.distance_ref, self.lcn_lambda = distance_ref, lcn_lambda

    def evaluate(self, env, max_return, n=10):
        """lcn.py:342-358."""
        n = min(n, len(self.replay))
        episodes = nlargest(self.replay, n, self.cd_threshold, self.distance_ref, self.lcn_lambda)
        returns, horizons = list(zip(*[(e[2][0].reward, len(e[2])) for e in episodes]))
        returns, horizons = np.float32(returns), np.float32(horizons)
        e_returns = []
        for i in range(n):
            transitions = self.run_episode(env, returns[i], np.float32(horizons[i]), max_return, eval_mode=True)
            for i in reversed(range(len(transitions) - 1)):
                transitions[i].reward += self.gamma * transitions[i + 1].reward
            e_returns.append(transitions[0].reward)
        return e_returns

    def train(self, total_timesteps, eval_env, num_er_episodes=500, num_step_episodes=10, num_model_updates=100, max_return=None,
              max_buffer_size=500, num_points_pf=100, cd_threshold=0.2):
        """lcn.py:405-527."""
        n_checkpoints = 0
        R = self.env.unwrapped.reward_space.shape[0]
        max_return = max_return if max_return is not None else np.full(R, 100.0, dtype=np.float32)
        step = 0
        self.cd_threshold = cd_threshold
        self.replay = []
        for _ in range(num_er_episodes):
            transitions = []
            obs, _ = self.env.reset()
            done = False
            while not done:
                action = self.env.action_space.sample()
                n_obs, reward, terminated, truncated, _ = self.env.step(action)
                transitions.append(po.Transition(obs, action, np.float32(reward).copy(), n_obs, terminated))
                done = terminated or truncated
                obs = n_obs
                step += 1
            po.add_episode(self.replay, transitions, max_buffer_size, step, self.gamma)
        while step < total_timesteps:
            po.update_loop(self.learner, self.replay, self.np_random, self.batch_size, num_model_updates)
            desired_return, desired_horizon = choose_commands(self.replay, self.np_random, num_er_episodes, self.cd_threshold,
                                                              self.distance_ref, self.lcn_lambda)
            self.commands.append((desired_return.copy(), np.float32(desired_horizon)))
            for _ in range(num_step_episodes):
                transitions = self.run_episode(self.env, desired_return, desired_horizon, max_return)
                step += len(transitions)
                po.add_episode(self.replay, transitions, max_buffer_size, step, self.gamma)
            if step >= (n_checkpoints + 1) * total_timesteps / 100:
                n_checkpoints += 1
                self.evaluate(eval_env, max_return, n=num_points_pf)
        return step
