"""TEST INFRASTRUCTURE: a torch restatement of EUPG (``single_policy/esr/eupg.py``) -- the policy network, the reverse discounted
scan, one ``update()`` and ``train()``.

With ``local=False`` it uses the reference's own operations (the sigmoids divided by their sum over the WHOLE batch, ``Categorical``,
autograd, ``optim.Adam``) on the CPU in float32; ``tests/golden/make_golden_eupg.py`` asserts that it reproduces every value it
records from the unmodified reference bit for bit.  With ``local=True`` every row is normalised by its own sum, which is what the
kernels compute: ``test_eupg_oracle_golden.py`` holds that form to the contract against the reference's fixtures, and in
``th.float64`` it is the shape sweep's reference.  ``bench_ac.py --workload eupg`` moves it to the device as the eager leg.
"""
from __future__ import annotations

import copy
from typing import Sequence

import numpy as np
import torch as th
from torch import nn, optim
from torch.distributions import Categorical

from ppo_oracle import adam_flat, flat_np, load_flat, params_np, set_adam_state  # noqa: F401  (the same flat-vector helpers)


EPS32 = float(np.finfo(np.float32).eps)


def _layer_init(layer):
    if isinstance(layer, nn.Linear):
        th.nn.init.orthogonal_(layer.weight, gain=1)
        th.nn.init.constant_(layer.bias, 0)


class PolicyNet(nn.Module):
    """``PolicyNet`` (``eupg.py:22-75``): every ``Linear`` is built with torch's default initialisation first, then ``apply``
    re-initialises them in module order, so a seeded construction draws the reference's parameters."""

    def __init__(self, obs_dim: int, n_actions: int, rew_dim: int, net_arch: Sequence[int] = (50,), local: bool = False):
        super().__init__()
        self.obs_dim, self.action_dim, self.rew_dim, self.local = obs_dim, n_actions, rew_dim, local
        mods, w = [], obs_dim + rew_dim
        for h in net_arch:
            mods += [nn.Linear(w, h), nn.Tanh()]
            w = h
        mods.append(nn.Linear(w, n_actions))
        self.net = nn.Sequential(*mods)
        self.apply(_layer_init)

    def forward(self, obs, acc_reward):
        if self.local:          # (any input dtype: the float64 form is fed float64 rows)
            dtype = self.net[0].weight.dtype
            obs, acc_reward = obs.to(dtype), acc_reward.to(dtype)
        s = th.sigmoid(self.net(th.cat((obs, acc_reward), dim=acc_reward.dim() - 1)))
        probas = s / s.sum(dim=-1, keepdim=True) if self.local else s / th.sum(s)
        return probas.view(-1, self.action_dim)

    def distribution(self, obs, acc_reward):
        return Categorical(self.forward(obs, acc_reward))


def truncate_obs(obs) -> np.ndarray:
    """What ``update()`` sees of the observations: the reference's buffer is created with ``obs_dtype=np.int32``, and numpy's
    assignment cast truncates towards zero."""
    buf = np.zeros(np.shape(obs), dtype=np.int32)
    buf[...] = np.asarray(obs)
    return buf


def forward_cumulative_rewards(rewards: th.Tensor, gamma: float) -> th.Tensor:
    """``_forward_cumulative_rewards`` (``eupg.py:263-270``)."""
    flip = rewards.flip(dims=[0])
    cum = th.zeros(rewards.shape[1], dtype=rewards.dtype, device=rewards.device)
    for i in range(len(rewards)):
        cum = gamma * cum + flip[i]
        flip[i] = cum
    return flip.flip(dims=[0])


def update(net: PolicyNet, opt, obs, acc_rewards, actions, rewards, gamma, scalarization, apply=True):
    """``EUPG.update()`` (``eupg.py:227-251``) on the episode's tensors as ``get_all_data`` hands them over: ``obs`` int32 (or any
    dtype: fed untruncated floats it shows what the truncation changes), ``actions`` [T][1] int32.
    Returns (loss, returns [T][R], scalarised values [T], probabilities of the rows [T][A], log-probs [T])."""
    G = forward_cumulative_rewards(rewards, gamma)
    u = scalarization(G)
    if net.local:
        # Categorical clamps with the eps of ITS dtype; the kernels' (and the reference's) is float32's whatever this one is
        probs = net.forward(obs, acc_rewards)
        logits = th.log(th.clamp(probs, EPS32, 1.0 - EPS32))
        logp = logits.gather(-1, actions.long().reshape(-1, 1)).reshape(-1)
        dist = type("Rows", (), {"probs": probs})
    else:
        dist = net.distribution(obs, acc_rewards)
        logp = dist.log_prob(actions.squeeze())
    loss = -th.mean(logp * u)
    if apply:
        opt.zero_grad()
        loss.backward()
        opt.step()
    return loss.detach(), G, u.detach(), dist.probs.detach(), logp.detach()


def to_dtype(net: PolicyNet, dtype, local=None) -> PolicyNet:
    out = copy.deepcopy(net).to(dtype)
    if local is not None:
        out.local = local
    return out


def step_f64(p0, m0, v0, step, lr, shape, obs, acc_rewards, actions, rewards, gamma, scalarization):
    """One ``update()`` in float64 with each row normalised locally, from flat parameters and Adam state.  ``shape`` =
    (obs_dim, n_actions, rew_dim, net_arch).  Returns dict(loss, G, u, probs, logp, p1, m1, v1)."""
    D, A, R, arch = shape
    net = PolicyNet(D, A, R, arch, local=True).to(th.float64)
    load_flat(net, np.asarray(p0, dtype=np.float64))
    opt = optim.Adam(net.parameters(), lr=lr)
    if m0 is not None:
        set_adam_state(opt, net, np.asarray(m0, dtype=np.float64), np.asarray(v0, dtype=np.float64), step)
    T64 = lambda a: th.as_tensor(np.asarray(a, dtype=np.float64))  # noqa: E731
    loss, G, u, probs, logp = update(net, opt, T64(obs), T64(acc_rewards), th.as_tensor(np.asarray(actions)).long().reshape(-1, 1),
                                     T64(rewards), float(np.float32(gamma)), scalarization)
    m1, v1 = adam_flat(opt, net)
    return dict(loss=float(loss), G=G.numpy(), u=u.numpy(), probs=probs.numpy(), logp=logp.numpy(), p1=flat_np(net), m1=m1, v1=v1)


class Learner:
    """``EUPG`` restated (constructor subset, ``train``, ``update``): what the recorded trace replays.  ``env`` is a single
    environment with ``observation_space``, ``action_space.n`` and ``reward_space``."""

    def __init__(self, env, scalarization, weights=np.ones(2), net_arch=(50,), gamma=0.99, learning_rate=1e-3):
        self.env, self.scalarization, self.weights, self.gamma = env, scalarization, weights, gamma
        self.D, self.A, self.R = env.observation_space.shape[0], int(env.action_space.n), env.reward_space.shape[0]
        self.net = PolicyNet(self.D, self.A, self.R, net_arch)
        self.opt = optim.Adam(self.net.parameters(), lr=learning_rate)
        self.rows = []
        self.losses, self.action_log = [], []
        self.global_step = self.num_episodes = 0

    def update(self):
        obs = th.tensor(truncate_obs(np.stack([r[0] for r in self.rows])))
        acc = th.tensor(np.stack([r[1] for r in self.rows]).astype(np.float32))
        actions = th.tensor(np.asarray([[r[2]] for r in self.rows], dtype=np.int32))
        rewards = th.tensor(np.stack([r[3] for r in self.rows]).astype(np.float32))
        loss = update(self.net, self.opt, obs, acc, actions, rewards, self.gamma, self.scalarization)[0]
        self.losses.append(float(loss))

    def train(self, total_timesteps, after_update=None):
        obs, _ = self.env.reset()
        acc = th.zeros(self.R, dtype=th.float32)
        for _ in range(total_timesteps):
            self.global_step += 1
            with th.no_grad():
                action = self.net.distribution(th.Tensor(obs), acc).sample().item()
            self.action_log.append(action)
            next_obs, reward, terminated, truncated, _ = self.env.step(action)
            self.rows.append((np.array(obs).copy(), acc.numpy().copy(), action, np.array(reward).copy()))
            acc += th.from_numpy(reward)
            if terminated or truncated:
                self.update()
                self.rows = []
                obs, _ = self.env.reset()
                self.num_episodes += 1
                acc = th.zeros(self.R).float()
                if after_update is not None:
                    after_update(self.num_episodes)
            else:
                obs = next_obs
