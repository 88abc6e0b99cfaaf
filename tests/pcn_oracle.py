"""TEST INFRASTRUCTURE: a torch / numpy restatement of Pareto Conditioned Networks (``multi_policy/pcn/pcn.py`` of the
reference), independent of the package under test.  ``tests/test_pcn_oracle_golden.py`` pins it to fixtures recorded from the
unmodified reference with exact equality on the CPU; the kernel tests, the agent tests and ``bench_ac.py``'s eager-torch leg
(``device=`` a GPU) are measured against it.

Parameters are a list of eight tensors in the reference's ``model.parameters()`` order without the frozen ``scaling_factor``:
``s_emb.0`` (W, b), ``c_emb.0`` (W, b), ``fc.0`` (W, b), ``fc.2`` (W, b).
"""
from __future__ import annotations

import heapq
from dataclasses import dataclass
from typing import List, Union

import numpy as np
import torch as th
import torch.nn.functional as F
from torch import nn


# ---- model (pcn.py:51-103) -------------------------------------------------------------------------------------------
def init_params(state_dim, reward_dim, action_dim, hidden_dim):
    """The four ``nn.Linear`` layers in the order the reference's default models construct them (pcn.py:81-88 / :97-103), default
    initialisation: a seeded call draws the reference's initial parameters."""
    layers = [nn.Linear(state_dim, hidden_dim), nn.Linear(reward_dim + 1, hidden_dim), nn.Linear(hidden_dim, hidden_dim),
              nn.Linear(hidden_dim, action_dim)]
    return [p.detach().clone() for l in layers for p in (l.weight, l.bias)]


def forward(params, scaling, state, desired_return, desired_horizon, continuous, dtype=None):
    """pcn.py:63-72 (+ LogSoftmax(dim=1) of the discrete model, :87).  ``dtype``: evaluate in that precision (float64: the
    accumulation-robustness check of the trace generator) from the same fp32 parameters."""
    Ws, bs, Wc, bc, W1, b1, W2, b2 = params
    if dtype is not None:
        Ws, bs, Wc, bc, W1, b1, W2, b2 = (p.to(dtype) for p in params)
        scaling, state, desired_return, desired_horizon = (t.to(dtype) for t in (scaling, state, desired_return, desired_horizon))
    c = th.cat((desired_return, desired_horizon), dim=-1)
    c = c * scaling
    s = th.sigmoid(F.linear(state.float() if dtype is None else state, Ws, bs))
    c = th.sigmoid(F.linear(c, Wc, bc))
    out = F.linear(F.relu(F.linear(s * c, W1, b1)), W2, b2)
    return out if continuous else F.log_softmax(out, dim=1)


def loss_of(prediction, actions, continuous):
    """pcn.py:225-232."""
    if continuous:
        return F.mse_loss(actions.float(), prediction)
    onehot = F.one_hot(actions.long(), len(prediction[0]))
    return th.sum(-onehot * prediction, -1).mean()


class Learner:
    """Parameters + ``th.optim.Adam`` (pcn.py:181), optionally resumed at a non-zero step count."""

    def __init__(self, params, scaling, continuous, lr=1e-3, device="cpu", exp_avg=None, exp_avg_sq=None, step=0):
        self.params = [p.detach().clone().to(device).requires_grad_(True) for p in params]
        self.scaling = th.as_tensor(np.asarray(scaling)).float().to(device)
        self.continuous = continuous
        self.opt = th.optim.Adam(self.params, lr=lr)
        if step > 0:
            for p, m, v in zip(self.params, exp_avg, exp_avg_sq):
                self.opt.state[p] = {"step": th.tensor(float(step)), "exp_avg": m.detach().clone().to(device),
                                     "exp_avg_sq": v.detach().clone().to(device)}

    def forward(self, obs, desired_return, desired_horizon, dtype=None):
        with th.no_grad():
            return forward(self.params, self.scaling, obs, desired_return, desired_horizon, self.continuous, dtype)

    def update(self, obs, actions, desired_return, desired_horizon):
        """pcn.py:217-236 on an already gathered batch; returns (loss, prediction)."""
        prediction = forward(self.params, self.scaling, obs, desired_return, desired_horizon, self.continuous)
        self.opt.zero_grad()
        l = loss_of(prediction, actions, self.continuous)
        l.backward()
        self.opt.step()
        return l.detach(), prediction.detach()

    def moments(self):
        return ([self.opt.state[p]["exp_avg"] for p in self.params], [self.opt.state[p]["exp_avg_sq"] for p in self.params])


# ---- replay (pcn.py:22-48, 238-300) ----------------------------------------------------------------------------------
def get_non_dominated_inds(solutions):
    """common/pareto.py:128-137."""
    is_efficient = np.ones(solutions.shape[0], dtype=bool)
    for i, c in enumerate(solutions):
        if is_efficient[i]:
            is_efficient[is_efficient] = np.any(solutions[is_efficient] > c, axis=1)
            is_efficient[i] = 1
    return is_efficient


def crowding_distance(points):
    """pcn.py:22-37."""
    points = (points - points.min(axis=0)) / (np.ptp(points, axis=0) + 1e-8)
    dim_sorted = np.argsort(points, axis=0)
    point_sorted = np.take_along_axis(points, dim_sorted, axis=0)
    distances = np.abs(point_sorted[:-2] - point_sorted[2:])
    distances = np.pad(distances, ((1,), (0,)), constant_values=1)
    crowding = np.zeros(points.shape)
    crowding[dim_sorted, np.arange(points.shape[-1])] = distances
    return np.sum(crowding, axis=-1)


@dataclass
class Transition:
    observation: np.ndarray
    action: Union[float, int]
    reward: np.ndarray
    next_observation: np.ndarray
    terminal: bool


def add_episode(replay, transitions: List[Transition], max_size, step, gamma=1.0):
    """pcn.py:238-248."""
    for i in reversed(range(len(transitions) - 1)):
        transitions[i].reward += gamma * transitions[i + 1].reward
    if len(replay) == max_size:
        heapq.heappushpop(replay, (1, step, transitions))
    else:
        heapq.heappush(replay, (1, step, transitions))


def nlargest(replay, n, threshold=0.2):
    """pcn.py:250-279 (re-scores and re-heapifies ``replay`` in place)."""
    returns = np.array([e[2][0].reward for e in replay])
    distances = crowding_distance(returns)
    sma = np.argwhere(distances <= threshold).flatten()
    non_dominated_i = get_non_dominated_inds(returns)
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
    sorted_i = np.argsort(l2)
    largest = [replay[i] for i in sorted_i[-n:]]
    for i in range(len(l2)):
        replay[i] = (l2[i], replay[i][1], replay[i][2])
    heapq.heapify(replay)
    return largest


def choose_commands(replay, np_random, num_episodes):
    """pcn.py:281-300."""
    episodes = nlargest(replay, num_episodes)
    returns, horizons = list(zip(*[(e[2][0].reward, len(e[2])) for e in episodes]))
    nd_i = get_non_dominated_inds(np.array(returns))
    returns = np.array(returns)[nd_i]
    horizons = np.array(horizons)[nd_i]
    r_i = np_random.integers(0, len(returns))
    desired_horizon = np.float32(horizons[r_i] - 2)
    _, s = np.mean(returns, axis=0), np.std(returns, axis=0)
    desired_return = returns[r_i].copy()
    r_i = np_random.integers(0, len(desired_return))
    desired_return[r_i] += np_random.uniform(high=s[r_i])
    return np.float32(desired_return), desired_horizon


def heap_summary(replay):
    """(distance, step, return of the first transition, length) of every heap slot, in heap order."""
    return (np.array([float(e[0]) for e in replay], dtype=np.float64), np.array([e[1] for e in replay], dtype=np.int64),
            np.array([e[2][0].reward for e in replay], dtype=np.float32), np.array([len(e[2]) for e in replay], dtype=np.int64))


# ---- update() on the replay (pcn.py:202-236) -------------------------------------------------------------------------
def draw_batch(replay, np_random, batch_size):
    """pcn.py:206-216: the (episode, time step) draws of one update, in the reference's order of calls on ``np_random``."""
    s_i = np_random.choice(np.arange(len(replay)), size=batch_size, replace=True)
    picks = []
    for i in s_i:
        ep = replay[i][2]
        t = np_random.integers(0, len(ep))
        picks.append((int(i), int(t)))
    return picks


def gather(replay, picks, device="cpu"):
    """pcn.py:214-222: the tensors ``update()`` hands the model, and the stored actions."""
    batch = []
    for i, t in picks:
        ep = replay[i][2]
        batch.append((ep[t].observation, ep[t].action, np.float32(ep[t].reward), np.float32(len(ep) - t)))
    obs, actions, desired_return, desired_horizon = zip(*batch)
    return (th.tensor(np.array(obs)).to(device), th.tensor(np.array(actions)).to(device),
            th.tensor(np.array(desired_return)).to(device), th.tensor(np.array(desired_horizon)).unsqueeze(1).to(device))


def flatten_replay(replay, state_dim, reward_dim, action_width):
    """One row per stored transition: obs | action | return-to-go | steps left; and the first row of every episode."""
    rows, starts = [], []
    for _, _, ep in replay:
        starts.append(len(rows))
        for t, tr in enumerate(ep):
            rows.append(np.concatenate([np.asarray(tr.observation, dtype=np.float32).reshape(-1),
                                        np.asarray(tr.action, dtype=np.float32).reshape(-1), np.float32(tr.reward).reshape(-1),
                                        np.array([len(ep) - t], dtype=np.float32)]))
    tab = np.stack(rows).astype(np.float32)
    assert tab.shape[1] == state_dim + action_width + reward_dim + 1
    return tab, np.asarray(starts, dtype=np.int64)


def update_loop(learner: Learner, replay, np_random, batch_size, n):
    """``n`` consecutive ``update()`` calls: per-step losses, the last prediction, and the (episode, step) picks of every update."""
    losses, all_picks, pred = [], [], None
    for _ in range(n):
        picks = draw_batch(replay, np_random, batch_size)
        l, pred = learner.update(*gather(replay, picks, learner.scaling.device))
        losses.append(l)
        all_picks.append(picks)
    return th.stack(losses), pred, all_picks


# ---- the training loop (pcn.py:302-349, 390-538), without logging / checkpoints ------------------------------------------
class Agent:
    def __init__(self, env, scaling_factor, learning_rate=1e-3, gamma=1.0, batch_size=256, hidden_dim=64, noise=0.1, seed=None,
                 act_dtype=None):
        self.env = env
        self.continuous = not hasattr(env.action_space, "n")
        D = env.observation_space.shape[0]
        A = env.action_space.shape[0] if self.continuous else env.action_space.n
        R = env.unwrapped.reward_space.shape[0]
        self.np_random = np.random.default_rng(seed)
        self.learner = Learner(init_params(D, R, A, hidden_dim), scaling_factor, self.continuous, lr=learning_rate)
        self.gamma, self.batch_size, self.noise, self.act_dtype = gamma, batch_size, noise, act_dtype
        self.replay = []
        self.logps, self.commands = [], []

    def act(self, obs, desired_return, desired_horizon, eval_mode=False):
        """pcn.py:302-322."""
        prediction = self.learner.forward(th.tensor(np.array([obs])).float(), th.tensor(np.array([desired_return])).float(),
                                          th.tensor(np.array([desired_horizon])).unsqueeze(1).float(), self.act_dtype)
        prediction = prediction.float().numpy()[0]
        if not eval_mode:
            self.logps.append(prediction.copy())
        if self.continuous:
            return prediction if eval_mode else prediction + np.random.normal(0.0, self.noise)
        if eval_mode:
            return np.argmax(prediction)
        return self.np_random.choice(np.arange(len(prediction)), p=np.exp(prediction))

    def run_episode(self, env, desired_return, desired_horizon, max_return, eval_mode=False):
        """pcn.py:324-349."""
        transitions = []
        obs, _ = env.reset()
        done = False
        while not done:
            action = self.act(obs, desired_return, desired_horizon, eval_mode)
            n_obs, reward, terminated, truncated, _ = env.step(action)
            done = terminated or truncated
            transitions.append(Transition(obs, action, np.float32(reward).copy(), n_obs, terminated))
            obs = n_obs
            desired_return = np.clip(desired_return - reward, None, max_return, dtype=np.float32)
            desired_horizon = np.float32(max(desired_horizon - 1, 1.0))
        return transitions

    def evaluate(self, env, max_return, n=10):
        """pcn.py:360-376: greedy episodes towards the returns of the n best stored episodes.  It consumes no random numbers, but
        its ``_nlargest`` call re-scores and re-heapifies the replay, which the next update's episode draws index into."""
        n = min(n, len(self.replay))
        episodes = nlargest(self.replay, n)
        returns, horizons = list(zip(*[(e[2][0].reward, len(e[2])) for e in episodes]))
        returns, horizons = np.float32(returns), np.float32(horizons)
        e_returns = []
        for i in range(n):
            transitions = self.run_episode(env, returns[i], np.float32(horizons[i]), max_return, eval_mode=True)
            for i in reversed(range(len(transitions) - 1)):
                transitions[i].reward += self.gamma * transitions[i + 1].reward
            e_returns.append(transitions[0].reward)
        return e_returns

    def train(self, total_timesteps, eval_env, num_er_episodes=20, num_step_episodes=10, num_model_updates=50, max_return=None,
              max_buffer_size=100, num_points_pf=100):
        """pcn.py:419-528."""
        n_checkpoints = 0
        R = self.env.unwrapped.reward_space.shape[0]
        max_return = max_return if max_return is not None else np.full(R, 100.0, dtype=np.float32)
        step = 0
        self.replay = []
        for _ in range(num_er_episodes):
            transitions = []
            obs, _ = self.env.reset()
            done = False
            while not done:
                action = self.env.action_space.sample()
                n_obs, reward, terminated, truncated, _ = self.env.step(action)
                transitions.append(Transition(obs, action, np.float32(reward).copy(), n_obs, terminated))
                done = terminated or truncated
                obs = n_obs
                step += 1
            add_episode(self.replay, transitions, max_buffer_size, step, self.gamma)
        while step < total_timesteps:
            update_loop(self.learner, self.replay, self.np_random, self.batch_size, num_model_updates)
            desired_return, desired_horizon = choose_commands(self.replay, self.np_random, num_er_episodes)
            self.commands.append((desired_return.copy(), np.float32(desired_horizon)))
            for _ in range(num_step_episodes):
                transitions = self.run_episode(self.env, desired_return, desired_horizon, max_return)
                step += len(transitions)
                add_episode(self.replay, transitions, max_buffer_size, step, self.gamma)
            if step >= (n_checkpoints + 1) * total_timesteps / 1000:
                n_checkpoints += 1
                self.evaluate(eval_env, max_return, n=num_points_pf)
        return step
