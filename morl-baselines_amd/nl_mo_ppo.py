"""Non-linear multi-objective PPO on the HIP library (``single_policy/ser/nl_mo_ppo.py``), the learner IPRO calls for every
Pareto-oracle query.

The policy is categorical; actor and critic read ``obs | accrued discounted reward | preference``.  GAE keeps one advantage per
objective, each objective's clipped surrogate is formed on its own, and the objectives are combined by ``loss_weights = du/dv`` at
``v(s0)`` -- the weights of the non-linear policy-gradient theorem, recomputed by every ``update()``.

The two networks' parameters live in one flat device tensor in the order of ``Agent.parameters()`` (``critic.*``, ``actor.*``).
``train()`` collects a rollout with one ``morl_nlppo_forward`` launch per vector step, ``morl_nlppo_gae`` runs the reverse scan on
the device, and ``update()`` draws the epochs' shuffles from ``rng`` exactly as the reference does and makes ONE
``morl_nlppo_update_n`` call for all ``update_epochs x num_minibatches`` steps (one launch per step; with ``target_kl`` set, one call
per epoch and one read of that epoch's last ``approx_kl``).  ``u_func`` and its gradient stay on the host: one read of ``mc_k x R``
values per ``update()``.

Actions are sampled on the host, ``Categorical(logits=...).sample()`` from torch's CPU generator on the log-probabilities the
launch returns, so a seeded run consumes the generator's stream as the reference does on the CPU.  The stored log-prob is the
launch's own entry of the sampled action, which the next minibatch step reproduces bit for bit.

Not here: W&B logging, and ``envs`` is any object with ``num_envs``, ``single_observation_space.shape``, ``single_action_space.n``,
``reward_space.shape``, ``reset(seed=)`` and ``step(actions)``.
"""
from __future__ import annotations

from math import ceil
from typing import Callable, Optional, Sequence, Union

import numpy as np
import torch as th
from torch import nn
from torch.distributions.categorical import Categorical

from .acnets import FlatAdam, bind_flat
from .api import MOPolicy
from .mo_ppo import STAT_NAMES, SUPPORTED_HIDDEN, run_epochs
from .native import Context, NativeLib, _ptr, load_library


def _layer_init(layer: nn.Linear, std: float = np.sqrt(2), bias_const: float = 0.0) -> nn.Linear:
    th.nn.init.orthogonal_(layer.weight, std)
    th.nn.init.constant_(layer.bias, bias_const)
    return layer


def _mlp(in_dim: int, out_dim: int, net_arch: Sequence[int], head_std: float) -> nn.Sequential:
    mods, width = [], in_dim
    for h in net_arch:
        mods += [_layer_init(nn.Linear(width, h)), nn.Tanh()]
        width = h
    mods.append(_layer_init(nn.Linear(width, out_dim), std=head_std))
    return nn.Sequential(*mods)


class Agent(nn.Module):
    """Parameter shell with the reference's module tree (``nl_mo_ppo.py:26-56``): ``critic`` then ``actor``, each layer
    initialised as it is built (orthogonal, gains sqrt(2) / 1.0 for the critic's head / 0.01 for the actor's), so a seeded
    construction draws the reference's initial parameters.  The forward pass is ``morl_nlppo_forward``; the shell only holds the
    parameters, which ``NLMOPPO`` turns into views of its flat device tensor."""

    def __init__(self, envs, num_objectives: int, pref_dim: int, net_arch: Sequence[int] = (64, 64)):
        super().__init__()
        self.num_objectives, self.pref_dim, self.net_arch = num_objectives, pref_dim, tuple(int(h) for h in net_arch)
        self.obs_dim = int(np.array(envs.single_observation_space.shape).prod())
        self.n_actions = int(envs.single_action_space.n)
        in_dim = self.obs_dim + num_objectives + pref_dim
        self.critic = _mlp(in_dim, num_objectives, self.net_arch, 1.0)
        self.actor = _mlp(in_dim, self.n_actions, self.net_arch, 0.01)


class NLMOPPO(MOPolicy):
    """The constructor, ``reset_agent``, ``train``, ``update``, ``eval`` and ``policy_evaluate`` of the reference class
    (``nl_mo_ppo.py:111-490``)."""

    def __init__(self, id: int, envs, log: bool = False, experiment_name: Optional[str] = "NLMOPPO",
                 wandb_project_name: str = "MORL-Baselines", wandb_entity: Optional[str] = None, wandb_mode: str = "online",
                 total_timesteps: int = 500000, learning_rate: float = 2.5e-4, num_steps: int = 128, anneal_lr: bool = True,
                 gamma: float = 0.99, gae_lambda: float = 0.95, num_minibatches: int = 4, update_epochs: int = 4,
                 norm_adv: bool = True, clip_coef: float = 0.2, clip_vloss: bool = True, ent_coef: float = 0.01, vf_coef: float = 0.5,
                 max_grad_norm: float = 0.5, target_kl: Optional[float] = None, mc_k: int = 32,
                 device: Union[th.device, str] = "auto", seed: int = 1, rng: Optional[np.random.Generator] = None,
                 lib: Optional[NativeLib] = None, net_arch: Sequence[int] = (64, 64)):
        super().__init__(id, device)
        if log:
            raise NotImplementedError("NLMOPPO: W&B logging is not available here (log=True); the step statistics are in last_stats")
        self.device = th.device(self.device)
        self.lib = lib or load_library()
        self.envs, self.seed = envs, seed
        self.rng = rng or np.random.default_rng(seed)
        self.log, self.experiment_name = log, experiment_name
        self.wandb_project_name, self.wandb_entity, self.wandb_mode = wandb_project_name, wandb_entity, wandb_mode
        self.total_timesteps, self.learning_rate, self.num_envs, self.num_steps = total_timesteps, learning_rate, envs.num_envs, num_steps
        self.anneal_lr, self.gamma, self.gae_lambda = anneal_lr, gamma, gae_lambda
        self.num_minibatches, self.update_epochs, self.norm_adv, self.clip_coef = num_minibatches, update_epochs, norm_adv, clip_coef
        self.clip_vloss, self.ent_coef, self.vf_coef, self.max_grad_norm, self.target_kl = (clip_vloss, ent_coef, vf_coef,
                                                                                            max_grad_norm, target_kl)
        self.net_arch = [int(h) for h in net_arch]
        if not 1 <= len(self.net_arch) <= 2:
            raise ValueError(f"NLMOPPO: net_arch {self.net_arch} is not supported by the kernels: one or two hidden layers")
        if any(h not in SUPPORTED_HIDDEN for h in self.net_arch):
            raise ValueError(f"NLMOPPO: net_arch {self.net_arch} is not supported by the kernels (widths from {SUPPORTED_HIDDEN})")
        if len(envs.single_observation_space.shape) != 1:
            raise NotImplementedError("NLMOPPO: image observations are not supported: flat vectors only")

        self.num_objectives = int(envs.reward_space.shape[0])
        self.batch_size = int(self.num_envs * self.num_steps)
        self.minibatch_size = int(self.batch_size // self.num_minibatches)
        if self.minibatch_size < 1:
            raise ValueError(f"NLMOPPO: {num_minibatches} minibatches of a batch of {self.batch_size} rows")
        self.num_iterations = self.total_timesteps // self.batch_size

        # seed observations of the utility-gradient evaluation (nl_mo_ppo.py:207-211)
        self.init_obs = th.as_tensor(
            np.concatenate([envs.reset(seed=self.seed + i)[0] for i in range(ceil(mc_k / self.num_envs))])[:mc_k],
            device=self.device, dtype=th.float32)
        self.pref: Optional[th.Tensor] = None
        self._ctx = None
        self.last_stats = None           # [steps][8] device tensor of the last update(): STAT_NAMES per step
        self.last_loss_weights = None    # [R] host tensor of the last update()
        self.reset_agent(pref_dim=self.num_objectives)
        self._setup_storage()

    def _destroy(self):
        if self._ctx:
            self._ctx.close()

    def reset_agent(self, pref_dim: int):
        """``nl_mo_ppo.py:219-224``: a freshly initialised agent (and context) for ``pref_dim``, zero Adam state, no utility."""
        self._destroy()
        self.agent = Agent(self.envs, self.num_objectives, pref_dim=pref_dim, net_arch=self.net_arch)
        arch = self.net_arch
        shape = (self.agent.obs_dim, self.agent.n_actions, self.num_objectives, int(pref_dim), len(arch), arch[0],
                 arch[1] if len(arch) > 1 else 0)
        P = self.lib.family_param_count("nlppo", *shape, error=ValueError)
        self._ctx = Context(self.lib, "nlppo", *shape, self.minibatch_size)
        self._dims = (self.agent.obs_dim, self.agent.n_actions, self.num_objectives, int(pref_dim))
        self.params = th.zeros(P, dtype=th.float32, device=self.device)
        self.exp_avg = th.zeros_like(self.params)
        self.exp_avg_sq = th.zeros_like(self.params)
        bind_flat(self.agent, self.params)
        self.optimizer = FlatAdam(self.learning_rate, 1e-5, [p.shape for p in self.agent.parameters()], self.params, self.exp_avg,
                                  self.exp_avg_sq)
        self.u_func = None
        self.pref = None

    def _setup_storage(self):
        T, E, R, dev = self.num_steps, self.num_envs, self.num_objectives, self.device
        self.obs = th.zeros((T, E) + tuple(self.envs.single_observation_space.shape), device=dev, dtype=th.float32)
        self.acc_rewards = th.zeros((T, E, R), device=dev, dtype=th.float32)
        self.actions = th.zeros((T, E), device=dev, dtype=th.long)
        self.logprobs = th.zeros((T, E), device=dev, dtype=th.float32)
        self.rewards = th.zeros((T, E, R), device=dev, dtype=th.float32)
        self.dones = th.zeros((T, E), device=dev, dtype=th.float32)
        self.values = th.zeros((T, E, R), device=dev, dtype=th.float32)
        self.returns = None
        self.advantages = None

    # -- the device side -------------------------------------------------------------------------------------------------
    def _pref_dev(self, pref) -> Optional[th.Tensor]:
        if pref is None or self._dims[3] == 0:
            return None
        return th.as_tensor(pref).to(self.device, th.float32).reshape(-1)[:self._dims[3]].contiguous()

    def _forward(self, obs, acc_reward, pref, value_only: bool = False):
        """One launch: (normalised log-probabilities [rows][A] or None, values [rows][R]) on the device."""
        D, A, R, _ = self._dims
        obs = th.as_tensor(obs).to(self.device, th.float32).reshape(-1, D).contiguous()
        rows = obs.shape[0]
        acc = th.as_tensor(acc_reward).to(self.device, th.float32).reshape(-1, R).expand(rows, R).contiguous()
        pref_d = self._pref_dev(pref)
        value = th.empty(rows, R, dtype=th.float32, device=self.device)
        logp = None if value_only else th.empty(rows, A, dtype=th.float32, device=self.device)
        self.lib.check_device(self.params, obs, acc, pref_d, value)
        self.lib.check(self.lib.lib.morl_nlppo_forward(self._ctx, self.params.data_ptr(), obs.data_ptr(), acc.data_ptr(), _ptr(pref_d),
                                                       rows, int(value_only), _ptr(logp), value.data_ptr(), self.lib.stream_of(value)))
        return logp, value

    def _sample(self, obs, acc_reward, pref):
        """``get_action_and_value`` without an action: (action [rows] on the host, its log-prob [rows], value [rows][R])."""
        logp, value = self._forward(obs, acc_reward, pref)
        action = Categorical(logits=logp.cpu()).sample()
        logprob = logp.gather(1, action.to(self.device).unsqueeze(1)).squeeze(1)
        return action, logprob, value

    def _greedy(self, obs, acc_reward, pref) -> th.Tensor:
        """``get_greedy_action``: the arg-max of the log-probabilities, the first index on a tie."""
        logp, _ = self._forward(obs, acc_reward, pref)
        return th.from_numpy(np.argmax(logp.cpu().numpy(), axis=-1))

    def _collect_rollouts(self, next_obs, next_acc_reward, next_done, timestep, global_step):
        """``nl_mo_ppo.py:248-288``."""
        for step in range(self.num_steps):
            global_step += self.num_envs
            self.obs[step] = next_obs
            self.acc_rewards[step] = next_acc_reward
            self.dones[step] = next_done
            action, logprob, value = self._sample(next_obs, next_acc_reward, self.pref)
            self.values[step] = value
            self.actions[step] = action.to(self.device)
            self.logprobs[step] = logprob
            next_obs_np, reward_np, term_np, trunc_np, infos = self.envs.step(action.numpy())
            next_done_np = np.logical_or(term_np, trunc_np)
            self.rewards[step] = th.as_tensor(reward_np, device=self.device, dtype=th.float32)
            next_obs = th.as_tensor(next_obs_np, device=self.device, dtype=th.float32)
            next_done = th.as_tensor(next_done_np, device=self.device, dtype=th.float32)
            # accrued discounted reward and the step count of each env (nl_mo_ppo.py:274-275)
            next_acc_reward = (next_acc_reward + (self.gamma ** timestep) * self.rewards[step]) * (1.0 - next_done.unsqueeze(-1))
            timestep = (timestep + 1) * (1 - next_done.int().unsqueeze(-1))
        return next_obs, next_acc_reward, next_done, timestep, global_step

    def _compute_advantages_and_returns(self, next_obs, next_acc_reward, next_done):
        """``nl_mo_ppo.py:290-308``: uploads the rollout into the context's table and runs the reverse scan there.
        Returns (advantages [T][E][R], returns [T][E][R])."""
        T, E, R = self.num_steps, self.num_envs, self.num_objectives
        _, next_value = self._forward(next_obs, next_acc_reward, self.pref, value_only=True)
        cols = [self.obs.reshape(T * E, -1), self.acc_rewards, self.actions.to(th.int32), self.logprobs, self.rewards, self.dones,
                self.values]
        cols = [t.contiguous() for t in cols]
        pref_d = self._pref_dev(self.pref)
        next_done = th.as_tensor(next_done).to(self.device, th.float32).contiguous()
        advantages = th.empty(T, E, R, dtype=th.float32, device=self.device)
        returns = th.empty(T, E, R, dtype=th.float32, device=self.device)
        self.lib.check_device(*cols, pref_d, next_done, returns)
        stream = self.lib.stream_of(returns)
        self.lib.check(self.lib.lib.morl_nlppo_set_rollout(self._ctx, *[t.data_ptr() for t in cols],
                                                           None if pref_d is None else pref_d.data_ptr(), T, E, stream))
        self.lib.check(self.lib.lib.morl_nlppo_gae(self._ctx, next_value.data_ptr(), next_done.data_ptr(), float(self.gamma),
                                                   float(self.gae_lambda), returns.data_ptr(), advantages.data_ptr(), stream))
        self._keep = (cols, pref_d, next_value, next_done)       # (alive until the launches on the stream have read them)
        return advantages, returns

    def _compute_loss_weights(self) -> th.Tensor:
        """``nl_mo_ppo.py:310-323``: w = du/dv at v(s0), the mean value of ``init_obs`` with zero accrued reward.  The values come
        from one ``value_only`` launch; their mean, ``u_func`` and its gradient are evaluated on the host."""
        zero_acc = th.zeros((self.init_obs.shape[0], self.num_objectives), device=self.device, dtype=th.float32)
        _, value = self._forward(self.init_obs, zero_acc, self.pref, value_only=True)
        v0 = value.cpu().mean(0).detach().requires_grad_(True)
        u = self.u_func(v0)
        (w,) = th.autograd.grad(u, v0, retain_graph=False, create_graph=False)
        return w.detach()

    def _update_n(self, idx: np.ndarray, weights: th.Tensor) -> th.Tensor:
        n, M = idx.shape
        idx_dev = th.from_numpy(np.ascontiguousarray(idx, dtype=np.int32)).to(self.device)
        stats = th.empty(n, len(STAT_NAMES), dtype=th.float32, device=self.device)
        self.lib.check_device(self.params, self.exp_avg, self.exp_avg_sq, idx_dev, weights, stats)
        self.lib.check(self.lib.lib.morl_nlppo_update_n(
            self._ctx, self.params.data_ptr(), self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr(), n, idx_dev.data_ptr(), M,
            weights.data_ptr(), float(self.optimizer.param_groups[0]["lr"]), self.optimizer.steps, float(self.clip_coef),
            float(self.ent_coef), float(self.vf_coef), float(self.max_grad_norm), int(bool(self.clip_vloss)), int(bool(self.norm_adv)),
            stats.data_ptr(), self.lib.stream_of(stats)))
        self.optimizer.steps += n
        return stats

    def update(self):
        """``nl_mo_ppo.py:325-398``.  The rollout, its returns and advantages are the ones the last
        ``_compute_advantages_and_returns`` put into the context's table.  The shuffles are drawn from ``rng`` call for call; the
        steps of all epochs go to the device in one ``morl_nlppo_update_n`` call (``target_kl``: one call per epoch, and one read of
        the epoch's last ``approx_kl``).  Returns the reference's tuple: v_loss, pg_loss, entropy, old_approx_kl and approx_kl of
        the last minibatch (0-dim tensors) and the mean clipfrac of all steps."""
        loss_weights = self._compute_loss_weights()
        self.last_loss_weights = loss_weights
        w_dev = loss_weights.to(self.device, th.float32).contiguous()
        self.last_stats = run_epochs(self.rng, self.batch_size, self.minibatch_size, self.update_epochs, self.target_kl,
                                     lambda idx: self._update_n(idx, w_dev))
        self._keep_w = w_dev
        host = self.last_stats.cpu()
        last = host[-1]
        clipfrac = float(np.mean([float(c) for c in host[:, STAT_NAMES.index("clipfrac")]]))
        return last[2], last[1], last[3], last[4], last[5], clipfrac

    def eval(self, obs, disc_vec_return, pref=None):
        """``nl_mo_ppo.py:400-405``: one sampled action for the observation(s)."""
        obs = th.as_tensor(obs, dtype=th.float32)
        action, _, _ = self._sample(obs, th.as_tensor(disc_vec_return, dtype=th.float32), pref)
        return action if obs.ndim >= 2 else action[0]

    def policy_evaluate(self, eval_env, eval_episodes: int = 100, deterministic: bool = False):
        """``nl_mo_ppo.py:407-442``: the mean accrued discounted return of ``eval_episodes`` episodes from ``reset(seed=seed)``."""
        pareto_point = np.zeros(self.num_objectives)
        for _ in range(eval_episodes):
            obs, _ = eval_env.reset(seed=self.seed)
            terminated = truncated = False
            accrued_reward = np.zeros(self.num_objectives, dtype=np.float32)
            timestep = 0
            while not (terminated or truncated):
                if deterministic:
                    action = int(self._greedy(obs, accrued_reward, self.pref)[0])
                else:
                    action = int(self._sample(obs, accrued_reward, self.pref)[0][0])
                obs, reward, terminated, truncated, _ = eval_env.step(action)
                accrued_reward += (self.gamma ** timestep) * reward
                timestep += 1
            pareto_point += accrued_reward
        return pareto_point / eval_episodes

    def train(self, eval_env, u_func: Callable[[th.Tensor], th.Tensor], pref=None, deterministic: bool = False) -> np.ndarray:
        """``nl_mo_ppo.py:444-490``."""
        self.u_func = u_func
        self.pref = None if pref is None else th.as_tensor(pref, device=self.device, dtype=th.float32)
        global_step = 0
        next_obs, _ = self.envs.reset(seed=self.seed)
        next_obs = th.as_tensor(next_obs, device=self.device, dtype=th.float32)
        next_acc_reward = th.zeros((self.num_envs, self.num_objectives), dtype=th.float32, device=self.device)
        next_done = th.zeros(self.num_envs, device=self.device, dtype=th.float32)
        timestep = th.zeros((self.num_envs, 1), dtype=th.int32, device=self.device)
        for iteration in range(1, self.num_iterations + 1):
            if self.anneal_lr:
                frac = 1.0 - (iteration - 1.0) / self.num_iterations
                self.optimizer.param_groups[0]["lr"] = frac * self.learning_rate
            next_obs, next_acc_reward, next_done, timestep, global_step = self._collect_rollouts(
                next_obs, next_acc_reward, next_done, timestep, global_step)
            self.global_step = global_step
            self.advantages, self.returns = self._compute_advantages_and_returns(next_obs, next_acc_reward, next_done)
            self.update()
        return self.policy_evaluate(eval_env, deterministic=deterministic)
