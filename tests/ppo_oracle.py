"""TEST INFRASTRUCTURE: a torch restatement of MO-PPO (``single_policy/ser/mo_ppo.py``) -- the network, ``get_action_and_value``,
``__compute_advantages``, one minibatch step of ``update()``, the whole ``update()`` and ``train()``.

It uses autograd, ``clip_grad_norm_`` and ``optim.Adam(eps=1e-5)`` exactly as the reference does, on the CPU in float32;
``tests/golden/make_golden_ppo.py`` asserts that it reproduces every value it records from the unmodified reference bit for bit.
``dtype=th.float64`` evaluates the same step in double: the generator uses it to refuse fixtures in which a clip decision depends
on rounding.  ``bench_ac.py --workload ppo`` moves it to the device as the eager comparison leg.
"""
from __future__ import annotations

import copy
from typing import List, Optional

import numpy as np
import torch as th
from torch import nn, optim
from torch.distributions import Normal

STAT_NAMES = ("loss", "pg_loss", "v_loss", "entropy", "old_approx_kl", "approx_kl", "clipfrac", "grad_norm")


def _init(layer, gain, bias=0.0):
    if isinstance(layer, nn.Linear):
        th.nn.init.orthogonal_(layer.weight, gain=gain)
        th.nn.init.constant_(layer.bias, bias)


def _mlp(inp, out, arch):
    mods = [nn.Linear(inp, arch[0]), nn.Tanh()]
    for i in range(len(arch) - 1):
        mods += [nn.Linear(arch[i], arch[i + 1]), nn.Tanh()]
    mods.append(nn.Linear(arch[-1], out))
    return nn.Sequential(*mods)


class Net(nn.Module):
    """``MOPPONet`` (``mo_ppo.py:160-235``): same construction order, so a seeded construction draws the same parameters."""

    def __init__(self, obs_dim: int, action_dim: int, reward_dim: int, net_arch: List[int] = [64, 64]):
        super().__init__()
        self.obs_shape, self.action_shape, self.reward_dim, self.net_arch = (obs_dim,), (action_dim,), reward_dim, list(net_arch)
        self.critic = _mlp(obs_dim, reward_dim, net_arch)
        self.critic.apply(lambda l: _init(l, np.sqrt(2)))
        _init(list(self.critic.modules())[-1], 1.0)
        self.actor_mean = _mlp(obs_dim, action_dim, net_arch)
        self.actor_mean.apply(lambda l: _init(l, np.sqrt(2)))
        _init(list(self.actor_mean.modules())[-1], 0.01)
        self.actor_logstd = nn.Parameter(th.zeros(1, action_dim))

    def get_value(self, obs):
        return self.critic(obs)

    def get_action_and_value(self, obs, action=None):
        mean = self.actor_mean(obs)
        std = th.exp(self.actor_logstd.expand_as(mean))
        probs = Normal(mean, std)
        if action is None:
            action = probs.sample()
        return action, probs.log_prob(action).sum(1), probs.entropy().sum(1), self.critic(obs)


def params_np(net) -> List[np.ndarray]:
    return [p.detach().cpu().numpy().copy() for p in net.parameters()]


def flat_np(net) -> np.ndarray:
    return np.concatenate([p.reshape(-1) for p in params_np(net)])


def load_flat(net, flat):
    o = 0
    with th.no_grad():
        for p in net.parameters():
            n = p.numel()
            p.copy_(th.as_tensor(np.asarray(flat[o:o + n])).reshape(p.shape).to(p.dtype))
            o += n
    assert o == len(flat)


def set_adam_state(opt, net, exp_avg, exp_avg_sq, step):
    """Install flat moments and a step count (the single-step fixtures start at a non-zero Adam step)."""
    o = 0
    for p in net.parameters():
        n = p.numel()
        opt.state[p] = {"step": th.tensor(float(step)),
                        "exp_avg": th.as_tensor(np.asarray(exp_avg[o:o + n])).reshape(p.shape).to(p.dtype).clone(),
                        "exp_avg_sq": th.as_tensor(np.asarray(exp_avg_sq[o:o + n])).reshape(p.shape).to(p.dtype).clone()}
        o += n


def adam_flat(opt, net):
    m = np.concatenate([opt.state[p]["exp_avg"].detach().cpu().numpy().reshape(-1) for p in net.parameters()])
    v = np.concatenate([opt.state[p]["exp_avg_sq"].detach().cpu().numpy().reshape(-1) for p in net.parameters()])
    return m, v


def compute_advantages(rewards, dones, values, next_value, next_done, weights, gamma, gae_lambda, gae):
    """``mo_ppo.py:439-476``.  rewards / values [T][E][R], dones [T][E], next_value [E][R], next_done [E], weights [R]."""
    T, E, R = rewards.shape
    ext = lambda t: t.unsqueeze(1).repeat(1, R)  # noqa: E731
    if gae:
        advantages = th.zeros_like(rewards)
        lastgaelam = 0
        for t in reversed(range(T)):
            if t == T - 1:
                nextnonterminal, nextvalues = 1.0 - next_done, next_value
            else:
                nextnonterminal, nextvalues = 1.0 - dones[t + 1], values[t + 1]
            nextnonterminal = ext(nextnonterminal)
            delta = rewards[t] + gamma * nextvalues * nextnonterminal - values[t]
            advantages[t] = lastgaelam = delta + gamma * gae_lambda * nextnonterminal * lastgaelam
        returns = advantages + values
    else:
        returns = th.zeros_like(rewards)
        for t in reversed(range(T)):
            if t == T - 1:
                nextnonterminal, next_return = 1.0 - next_done, next_value
            else:
                nextnonterminal, next_return = 1.0 - dones[t + 1], returns[t + 1]
            nextnonterminal = ext(nextnonterminal)
            returns[t] = rewards[t] + gamma * nextnonterminal * next_return
        advantages = returns - values
    return returns, advantages @ weights


class Cfg:
    def __init__(self, clip_coef=0.2, ent_coef=0.0, vf_coef=0.5, clip_vloss=True, max_grad_norm=0.5, norm_adv=True):
        self.clip_coef, self.ent_coef, self.vf_coef = clip_coef, ent_coef, vf_coef
        self.clip_vloss, self.max_grad_norm, self.norm_adv = clip_vloss, max_grad_norm, norm_adv


def minibatch_step(net, opt, cfg: Cfg, b_obs, b_actions, b_logprobs, b_advantages, b_returns, b_values, mb_inds, apply=True):
    """``mo_ppo.py:509-554``.  Returns the step's statistics (0-dim tensors, ``STAT_NAMES``) and the rows' ratio / new values."""
    R = net.reward_dim
    _, newlogprob, entropy, newvalue = net.get_action_and_value(b_obs[mb_inds], b_actions[mb_inds])
    logratio = newlogprob - b_logprobs[mb_inds]
    ratio = logratio.exp()
    with th.no_grad():
        old_approx_kl = (-logratio).mean()
        approx_kl = ((ratio - 1) - logratio).mean()
        clipfrac = ((ratio - 1.0).abs() > cfg.clip_coef).float().mean()
    mb_advantages = b_advantages[mb_inds]
    if cfg.norm_adv:
        mb_advantages = (mb_advantages - mb_advantages.mean()) / (mb_advantages.std() + 1e-8)
    pg_loss1 = -mb_advantages * ratio
    pg_loss2 = -mb_advantages * th.clamp(ratio, 1 - cfg.clip_coef, 1 + cfg.clip_coef)
    pg_loss = th.max(pg_loss1, pg_loss2).mean()
    newvalue = newvalue.view(-1, R)
    if cfg.clip_vloss:
        v_loss_unclipped = (newvalue - b_returns[mb_inds]) ** 2
        v_clipped = b_values[mb_inds] + th.clamp(newvalue - b_values[mb_inds], -cfg.clip_coef, cfg.clip_coef)
        v_loss_clipped = (v_clipped - b_returns[mb_inds]) ** 2
        v_loss = 0.5 * th.max(v_loss_unclipped, v_loss_clipped).mean()
    else:
        v_loss = 0.5 * ((newvalue - b_returns[mb_inds]) ** 2).mean()
    entropy_loss = entropy.mean()
    loss = pg_loss - cfg.ent_coef * entropy_loss + v_loss * cfg.vf_coef
    grad_norm = th.zeros(())
    if apply:
        opt.zero_grad()
        loss.backward()
        grad_norm = nn.utils.clip_grad_norm_(net.parameters(), cfg.max_grad_norm)
        opt.step()
    stats = (loss, pg_loss, v_loss, entropy_loss, old_approx_kl, approx_kl, clipfrac, grad_norm)
    return [s.detach() for s in stats], ratio.detach(), newvalue.detach()


def update(net, opt, cfg: Cfg, np_random, batch, num_minibatches, update_epochs, target_kl=None, observer=None):
    """``MOPPO.update()`` (``mo_ppo.py:494-558``) on ``batch`` = (obs, actions, logprobs, advantages, returns, values), flattened.
    Returns (stats [steps][8] float32, idx [steps][M] int32); ``observer(ratio, newvalue, mb_inds)`` sees every step."""
    b_obs, b_actions, b_logprobs, b_advantages, b_returns, b_values = batch
    batch_size = b_obs.shape[0]
    minibatch_size = int(batch_size // num_minibatches)
    b_inds = np.arange(batch_size)
    stats, idx = [], []
    for _ in range(update_epochs):
        np_random.shuffle(b_inds)
        for start in range(0, batch_size, minibatch_size):
            mb_inds = b_inds[start:start + minibatch_size]
            s, ratio, newvalue = minibatch_step(net, opt, cfg, b_obs, b_actions, b_logprobs, b_advantages, b_returns, b_values,
                                                mb_inds)
            stats.append([float(x) for x in s])
            idx.append(mb_inds.copy())
            if observer is not None:
                observer(ratio, newvalue, mb_inds)
        if target_kl is not None and stats[-1][5] > target_kl:
            break
    return np.asarray(stats, dtype=np.float32), np.asarray(idx, dtype=np.int32)


class Agent:
    """``MOPPO`` restated (constructor subset, ``train``, ``update``, ``eval``): what the recorded ``train()`` trace replays."""

    def __init__(self, net: Net, weights: np.ndarray, envs, steps_per_iteration=2048, num_minibatches=32, update_epochs=10,
                 learning_rate=3e-4, gamma=0.995, anneal_lr=False, clip_coef=0.2, ent_coef=0.0, vf_coef=0.5, clip_vloss=True,
                 max_grad_norm=0.5, norm_adv=True, target_kl=None, gae=True, gae_lambda=0.95, seed=42, rng=None):
        self.net, self.envs, self.num_envs, self.seed = net, envs, envs.num_envs, seed
        self.np_random = rng if rng is not None else np.random.default_rng(seed)
        self.weights = th.from_numpy(weights)
        self.steps_per_iteration, self.num_minibatches, self.update_epochs = steps_per_iteration, num_minibatches, update_epochs
        self.learning_rate, self.gamma, self.anneal_lr, self.gae, self.gae_lambda = learning_rate, gamma, anneal_lr, gae, gae_lambda
        self.target_kl = target_kl
        self.cfg = Cfg(clip_coef, ent_coef, vf_coef, clip_vloss, max_grad_norm, norm_adv)
        self.opt = optim.Adam(net.parameters(), lr=learning_rate, eps=1e-5)
        self.global_step = 0
        self.stats = []

    def train(self, current_iteration, max_iterations):
        T, E, R = self.steps_per_iteration, self.num_envs, self.net.reward_dim
        next_obs, _ = self.envs.reset(seed=self.seed)
        obs = th.Tensor(next_obs)
        done = th.zeros(E)
        if self.anneal_lr:
            self.opt.param_groups[0]["lr"] = (1.0 - (current_iteration - 1.0) / max_iterations) * self.learning_rate
        b = {k: [] for k in ("obs", "actions", "logprobs", "rewards", "dones", "values")}
        for _ in range(T):
            self.global_step += E
            with th.no_grad():
                action, logprob, _, value = self.net.get_action_and_value(obs)
            n_obs, reward, terminated, truncated, info = self.envs.step(action.numpy())
            for k, v in zip(b, (obs, action, logprob, th.tensor(reward).view(E, R), done, value.view(E, R))):
                b[k].append(v)
            obs, done = th.Tensor(n_obs), th.Tensor(terminated)
        b = {k: th.stack(v) for k, v in b.items()}
        with th.no_grad():
            next_value = self.net.get_value(obs).reshape(E, -1)
            self.returns, self.advantages = compute_advantages(b["rewards"], b["dones"], b["values"], next_value, done,
                                                               self.weights, self.gamma, self.gae_lambda, self.gae)
        self.batch = b
        flat = (b["obs"].reshape(T * E, -1), b["actions"].reshape(T * E, -1), b["logprobs"].reshape(-1),
                self.advantages.reshape(-1), self.returns.reshape(-1, R), b["values"].reshape(-1, R))
        s, _ = update(self.net, self.opt, self.cfg, self.np_random, flat, self.num_minibatches, self.update_epochs, self.target_kl)
        self.stats.append(s)


def to_dtype(net: Net, dtype) -> Net:
    return copy.deepcopy(net).to(dtype)
