"""TEST INFRASTRUCTURE: a torch restatement of NL-MO-PPO (``single_policy/ser/nl_mo_ppo.py``) -- the agent network, the GAE scan
that keeps the advantage vector, the loss weights ``du/dv`` at ``v(s0)``, one minibatch step of ``update()``, the whole ``update()``
and ``train()``.

It uses autograd, ``Categorical``, ``clip_grad_norm_`` and ``optim.Adam(eps=1e-5)`` exactly as the reference does, on the CPU in
float32; ``tests/golden/make_golden_nlppo.py`` asserts that it reproduces every value it records from the unmodified reference bit
for bit.  In ``th.float64`` the same step is the shape sweep's reference, and the generator uses it to refuse fixtures in which a
clip decision depends on rounding.  ``bench_ac.py --workload nlppo`` moves it to the device as the eager comparison leg.
"""
from __future__ import annotations

import copy
from math import ceil
from typing import Optional, Sequence

import numpy as np
import torch as th
from torch import nn, optim
from torch.distributions.categorical import Categorical

from ppo_oracle import adam_flat, flat_np, load_flat, params_np, set_adam_state  # noqa: F401  (the same flat-vector helpers)

STAT_NAMES = ("loss", "pg_loss", "v_loss", "entropy", "old_approx_kl", "approx_kl", "clipfrac", "grad_norm")


def _layer(inp, out, std=np.sqrt(2)):
    layer = nn.Linear(inp, out)
    th.nn.init.orthogonal_(layer.weight, std)
    th.nn.init.constant_(layer.bias, 0.0)
    return layer


def _mlp(inp, out, arch, head_std):
    mods, w = [], inp
    for h in arch:
        mods += [_layer(w, h), nn.Tanh()]
        w = h
    mods.append(_layer(w, out, head_std))
    return nn.Sequential(*mods)


class Agent(nn.Module):
    """``Agent`` (``nl_mo_ppo.py:26-108``): the critic is built before the actor, layer by layer, so a seeded construction draws
    the reference's parameters.  ``net_arch`` is (64, 64) in the reference."""

    def __init__(self, obs_dim: int, n_actions: int, num_objectives: int, pref_dim: int, net_arch: Sequence[int] = (64, 64)):
        super().__init__()
        self.obs_dim, self.n_actions, self.num_objectives, self.pref_dim = obs_dim, n_actions, num_objectives, pref_dim
        self.net_arch = tuple(net_arch)
        in_dim = obs_dim + num_objectives + pref_dim
        self.critic = _mlp(in_dim, num_objectives, self.net_arch, 1.0)
        self.actor = _mlp(in_dim, n_actions, self.net_arch, 0.01)

    def aug(self, x, acc_reward, pref):
        dtype = self.critic[0].weight.dtype
        x, acc_reward = x.to(dtype), acc_reward.to(dtype)
        if x.ndim < 2:
            parts = [x, acc_reward]
            if self.pref_dim > 0:
                parts.append(th.zeros(self.pref_dim, dtype=dtype) if pref is None else pref.to(dtype).view(-1))
            return th.cat(parts, dim=-1)
        if acc_reward.ndim == 1:
            acc_reward = acc_reward.expand(x.shape[0], -1)
        parts = [x, acc_reward]
        if self.pref_dim > 0:
            if pref is None:
                parts.append(th.zeros((x.shape[0], self.pref_dim), dtype=dtype))
            else:
                pref = pref.to(dtype)
                parts.append(pref.expand(x.shape[0], -1) if (pref.ndim == 1 or pref.shape[0] != x.shape[0]) else pref)
        return th.cat(parts, dim=-1)

    def get_value(self, x, acc_reward, pref=None):
        return self.critic(self.aug(x, acc_reward, pref))

    def logits(self, x, acc_reward, pref=None):
        return self.actor(self.aug(x, acc_reward, pref))

    def get_action_and_value(self, x, acc_reward, action=None, pref=None):
        aug = self.aug(x, acc_reward, pref)
        probs = Categorical(logits=self.actor(aug))
        if action is None:
            action = probs.sample()
        return action, probs.log_prob(action), probs.entropy(), self.critic(aug)

    def get_greedy_action(self, x, acc_reward, pref=None):
        return th.argmax(self.actor(self.aug(x, acc_reward, pref)), dim=-1)


def compute_advantages(rewards, dones, values, next_value, next_done, gamma, gae_lambda):
    """``nl_mo_ppo.py:290-308``.  rewards / values [T][E][R], dones [T][E], next_value [E][R], next_done [E] -> (advantages, returns)."""
    T = rewards.shape[0]
    advantages = th.zeros_like(rewards)
    lastgaelam = th.zeros_like(rewards[0])
    for t in reversed(range(T)):
        if t == T - 1:
            nextnonterminal, nextvalues = (1.0 - next_done).unsqueeze(-1), next_value
        else:
            nextnonterminal, nextvalues = (1.0 - dones[t + 1]).unsqueeze(-1), values[t + 1]
        delta = rewards[t] + gamma * nextvalues * nextnonterminal - values[t]
        lastgaelam = delta + gamma * gae_lambda * nextnonterminal * lastgaelam
        advantages[t] = lastgaelam
    return advantages, advantages + values


def loss_weights(net: Agent, init_obs, pref, u_func):
    """``_compute_loss_weights`` (``nl_mo_ppo.py:310-323``): du/dv at the mean value of ``init_obs`` with zero accrued reward."""
    zero_acc = th.zeros((init_obs.shape[0], net.num_objectives), dtype=init_obs.dtype)
    v0 = net.get_value(init_obs, acc_reward=zero_acc, pref=pref).mean(0).detach().requires_grad_(True)
    (w,) = th.autograd.grad(u_func(v0), v0)
    return w.detach(), v0.detach()


class Cfg:
    def __init__(self, clip_coef=0.2, ent_coef=0.01, vf_coef=0.5, clip_vloss=True, max_grad_norm=0.5, norm_adv=True):
        self.clip_coef, self.ent_coef, self.vf_coef = clip_coef, ent_coef, vf_coef
        self.clip_vloss, self.max_grad_norm, self.norm_adv = clip_vloss, max_grad_norm, norm_adv


def minibatch_step(net: Agent, opt, cfg: Cfg, batch, weights, mb_inds, apply=True):
    """``nl_mo_ppo.py:348-393``.  ``batch`` = (obs, acc_rewards, actions, logprobs, advantages [B][R], returns, values, pref | None).
    Returns the step's statistics (0-dim tensors, ``STAT_NAMES``) and a dict of per-row quantities."""
    b_obs, b_acc, b_actions, b_logprobs, b_advantages, b_returns, b_values, pref = batch
    b_prefs = pref.expand(b_obs.shape[0], -1) if pref is not None else None
    _, newlogprob, entropy, newvalue = net.get_action_and_value(b_obs[mb_inds], acc_reward=b_acc[mb_inds], action=b_actions.long()[mb_inds],
                                                                pref=b_prefs[mb_inds] if b_prefs is not None else None)
    logratio = newlogprob - b_logprobs[mb_inds]
    ratio = logratio.exp()
    with th.no_grad():
        old_approx_kl = (-logratio).mean()
        approx_kl = ((ratio - 1) - logratio).mean()
        clipfrac = ((ratio - 1.0).abs() > cfg.clip_coef).float().mean()
    mb_adv = b_advantages[mb_inds]
    if cfg.norm_adv:
        mb_adv = (mb_adv - mb_adv.mean(dim=0, keepdim=True)) / (mb_adv.std(dim=0, keepdim=True) + 1e-8)
    pg_loss1 = -mb_adv * ratio.unsqueeze(-1)
    pg_loss2 = -mb_adv * th.clamp(ratio, 1 - cfg.clip_coef, 1 + cfg.clip_coef).unsqueeze(-1)
    per_obj_pg = th.max(pg_loss1, pg_loss2).mean(dim=0)
    pg_loss = (per_obj_pg * weights).sum()
    if cfg.clip_vloss:
        v_loss_unclipped = (newvalue - b_returns[mb_inds]) ** 2
        v_clipped = b_values[mb_inds] + th.clamp(newvalue - b_values[mb_inds], -cfg.clip_coef, cfg.clip_coef)
        v_loss_clipped = (v_clipped - b_returns[mb_inds]) ** 2
        v_loss = 0.5 * th.max(v_loss_unclipped, v_loss_clipped).mean()
    else:
        v_loss = 0.5 * ((newvalue - b_returns[mb_inds]) ** 2).mean()
    entropy_loss = entropy.mean()
    loss = pg_loss - cfg.ent_coef * entropy_loss + cfg.vf_coef * v_loss
    grad_norm = th.zeros(())
    if apply:
        opt.zero_grad()
        loss.backward()
        grad_norm = nn.utils.clip_grad_norm_(net.parameters(), cfg.max_grad_norm)
        opt.step()
    stats = (loss, pg_loss, v_loss, entropy_loss, old_approx_kl, approx_kl, clipfrac, grad_norm)
    rows = dict(ratio=ratio.detach(), newvalue=newvalue.detach(), adv=mb_adv.detach(), pg1=pg_loss1.detach(), pg2=pg_loss2.detach())
    return [s.detach() for s in stats], rows


def update(net: Agent, opt, cfg: Cfg, rng, batch, weights, num_minibatches, update_epochs, target_kl=None, observer=None):
    """``NLMOPPO.update()`` (``nl_mo_ppo.py:339-398``) after its loss weights.  Returns (stats [steps][8] float32, idx [steps][M] int32);
    ``observer(rows, mb_inds)`` sees every step."""
    batch_size = batch[0].shape[0]
    minibatch_size = int(batch_size // num_minibatches)
    b_inds = np.arange(batch_size)
    stats, idx = [], []
    for _ in range(update_epochs):
        rng.shuffle(b_inds)
        for start in range(0, batch_size, minibatch_size):
            mb_inds = b_inds[start:start + minibatch_size]
            s, rows = minibatch_step(net, opt, cfg, batch, weights, mb_inds)
            stats.append([float(x) for x in s])
            idx.append(mb_inds.copy())
            if observer is not None:
                observer(rows, mb_inds)
        if target_kl is not None and stats[-1][5] > target_kl:
            break
    return np.asarray(stats, dtype=np.float32), np.asarray(idx, dtype=np.int32)


def returned_tuple(stats):
    """What ``update()`` returns: v_loss, pg_loss, entropy, old_approx_kl, approx_kl of the LAST step, the mean clipfrac."""
    last = stats[-1]
    return (last[2], last[1], last[3], last[4], last[5], float(np.mean([float(c) for c in stats[:, 6]])))


class Learner:
    """``NLMOPPO`` restated (constructor subset, ``train``, ``update``, ``policy_evaluate``): what the recorded trace replays."""

    def __init__(self, envs, total_timesteps=500000, learning_rate=2.5e-4, num_steps=128, anneal_lr=True, gamma=0.99, gae_lambda=0.95,
                 num_minibatches=4, update_epochs=4, norm_adv=True, clip_coef=0.2, clip_vloss=True, ent_coef=0.01, vf_coef=0.5,
                 max_grad_norm=0.5, target_kl=None, mc_k=32, seed=1, rng=None, net_arch=(64, 64)):
        self.envs, self.seed, self.num_envs = envs, seed, envs.num_envs
        self.rng = rng or np.random.default_rng(seed)
        self.total_timesteps, self.learning_rate, self.num_steps, self.anneal_lr = total_timesteps, learning_rate, num_steps, anneal_lr
        self.gamma, self.gae_lambda, self.num_minibatches, self.update_epochs = gamma, gae_lambda, num_minibatches, update_epochs
        self.target_kl, self.net_arch = target_kl, net_arch
        self.cfg = Cfg(clip_coef, ent_coef, vf_coef, clip_vloss, max_grad_norm, norm_adv)
        self.num_objectives = envs.reward_space.shape[0]
        self.batch_size = int(self.num_envs * num_steps)
        self.num_iterations = total_timesteps // self.batch_size
        self.init_obs = th.as_tensor(np.concatenate([envs.reset(seed=seed + i)[0] for i in range(ceil(mc_k / self.num_envs))])[:mc_k],
                                     dtype=th.float32)
        self.pref = None
        self.reset_agent(self.num_objectives)
        self.stats, self.weights_log, self.lr_log = [], [], []
        self.global_step = 0

    def reset_agent(self, pref_dim):
        obs_dim = int(np.array(self.envs.single_observation_space.shape).prod())
        self.agent = Agent(obs_dim, self.envs.single_action_space.n, self.num_objectives, pref_dim, self.net_arch)
        self.opt = optim.Adam(self.agent.parameters(), lr=self.learning_rate, eps=1e-5)
        self.u_func, self.pref = None, None

    def policy_evaluate(self, eval_env, eval_episodes=100, deterministic=False):
        point = np.zeros(self.num_objectives)
        for _ in range(eval_episodes):
            obs, _ = eval_env.reset(seed=self.seed)
            terminated = truncated = False
            accrued, timestep = np.zeros(self.num_objectives, dtype=np.float32), 0
            while not (terminated or truncated):
                with th.no_grad():
                    o, a = th.as_tensor(obs, dtype=th.float32), th.as_tensor(accrued, dtype=th.float32)
                    if deterministic:
                        action = self.agent.get_greedy_action(o, acc_reward=a, pref=self.pref).item()
                    else:
                        action = self.agent.get_action_and_value(o, acc_reward=a, pref=self.pref)[0].item()
                obs, reward, terminated, truncated, _ = eval_env.step(action)
                accrued += (self.gamma ** timestep) * reward
                timestep += 1
            point += accrued
        return point / eval_episodes

    def train(self, eval_env, u_func, pref=None, deterministic=False, after_iteration=None):
        T, E, R = self.num_steps, self.num_envs, self.num_objectives
        self.u_func = u_func
        self.pref = None if pref is None else th.as_tensor(pref, dtype=th.float32)
        next_obs = th.as_tensor(self.envs.reset(seed=self.seed)[0], dtype=th.float32)
        next_acc = th.zeros((E, R), dtype=th.float32)
        next_done = th.zeros(E, dtype=th.float32)
        timestep = th.zeros((E, 1), dtype=th.int32)
        for iteration in range(1, self.num_iterations + 1):
            if self.anneal_lr:
                self.opt.param_groups[0]["lr"] = (1.0 - (iteration - 1.0) / self.num_iterations) * self.learning_rate
            self.lr_log.append(self.opt.param_groups[0]["lr"])
            b = {k: [] for k in ("obs", "acc", "dones", "values", "actions", "logprobs", "rewards")}
            for _ in range(T):
                self.global_step += E
                with th.no_grad():
                    action, logprob, _, value = self.agent.get_action_and_value(next_obs, acc_reward=next_acc, pref=self.pref)
                n_obs, reward, term, trunc, _ = self.envs.step(action.numpy())
                reward = th.as_tensor(reward, dtype=th.float32)
                for k, v in zip(b, (next_obs, next_acc, next_done, value, action, logprob, reward)):
                    b[k].append(v)
                next_obs = th.as_tensor(n_obs, dtype=th.float32)
                next_done = th.as_tensor(np.logical_or(term, trunc), dtype=th.float32)
                next_acc = (next_acc + (self.gamma ** timestep) * reward) * (1.0 - next_done.unsqueeze(-1))
                timestep = (timestep + 1) * (1 - next_done.int().unsqueeze(-1))
            b = {k: th.stack(v) for k, v in b.items()}
            with th.no_grad():
                next_value = self.agent.get_value(next_obs, next_acc, self.pref).reshape(E, R)
                adv, ret = compute_advantages(b["rewards"], b["dones"], b["values"], next_value, next_done, self.gamma, self.gae_lambda)
            w, _ = loss_weights(self.agent, self.init_obs, self.pref, self.u_func)
            self.weights_log.append(w.numpy().copy())
            flat = (b["obs"].reshape(T * E, -1), b["acc"].reshape(T * E, R), b["actions"].reshape(-1), b["logprobs"].reshape(-1),
                    adv.reshape(T * E, R), ret.reshape(T * E, R), b["values"].reshape(T * E, R), self.pref)
            s, _ = update(self.agent, self.opt, self.cfg, self.rng, flat, w, self.num_minibatches, self.update_epochs, self.target_kl)
            self.stats.append(s)
            if after_iteration is not None:
                after_iteration(iteration)
        return self.policy_evaluate(eval_env, deterministic=deterministic)


def to_dtype(net: Agent, dtype) -> Agent:
    return copy.deepcopy(net).to(dtype)
