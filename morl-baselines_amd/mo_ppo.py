"""Multi-objective PPO on the HIP library (``single_policy/ser/mo_ppo.py``).

The networks' parameters live in one flat device tensor in the order of ``MOPPONet.parameters()`` (``actor_logstd``, ``critic.*``,
``actor_mean.*``).  ``train()`` collects a rollout with one ``morl_ppo_forward`` launch per vector step, ``morl_ppo_gae`` runs the
reverse scan of ``__compute_advantages`` on the device, and ``update()`` draws the epochs' shuffles from ``np_random`` exactly as
the reference does and makes ONE ``morl_ppo_update_n`` call for all ``update_epochs x num_minibatches`` steps (one launch per
step; with ``target_kl`` set, one call per epoch and one read of that epoch's last ``approx_kl``).

The exploration noise is drawn on the host with ``th.normal`` of the reference's shape, so a seeded run consumes the CPU
generator's stream exactly as ``Normal.sample()`` does in the reference on the CPU.

Not here: ``make_env`` and its gymnasium wrappers (``envs`` is any object with ``num_envs``, ``reset(seed=)`` and
``step(actions)``), image observations, W&B logging.
"""
from __future__ import annotations

from copy import deepcopy
from typing import Callable, List, Optional, Union

import numpy as np
import torch as th
from torch import nn

from .acnets import FlatAdam, bind_flat
from .api import MOPolicy
from .native import Context, NativeLib, _ptr, load_library

SUPPORTED_HIDDEN = (32, 64, 96, 128)
STAT_NAMES = ("loss", "pg_loss", "v_loss", "entropy", "old_approx_kl", "approx_kl", "clipfrac", "grad_norm")


def _layer_init(layer, weight_gain: float, bias_const: float = 0.0) -> None:
    if isinstance(layer, nn.Linear):
        th.nn.init.orthogonal_(layer.weight, gain=weight_gain)
        th.nn.init.constant_(layer.bias, bias_const)


def _mlp(input_dim: int, output_dim: int, net_arch: List[int]) -> nn.Sequential:
    modules = [nn.Linear(input_dim, net_arch[0]), nn.Tanh()]
    for i in range(len(net_arch) - 1):
        modules += [nn.Linear(net_arch[i], net_arch[i + 1]), nn.Tanh()]
    modules.append(nn.Linear(net_arch[-1], output_dim))
    return nn.Sequential(*modules)


class MOPPONet(nn.Module):
    """Parameter shell with the reference's module tree (``mo_ppo.py:160-203``): ``critic``, ``actor_mean``, ``actor_logstd``.

    The layers are built and initialised in the reference's order (orthogonal, gains sqrt(2) / 1.0 for the critic's head / 0.01
    for the actor's, zero ``actor_logstd``), so a seeded construction draws the reference's initial parameters.  The forward pass
    is ``morl_ppo_forward``; the shell only holds the parameters, which ``MOPPO`` turns into views of its flat device tensor."""

    def __init__(self, obs_shape: tuple, action_shape: tuple, reward_dim: int, net_arch: List = [64, 64]):
        super().__init__()
        self.obs_shape, self.action_shape, self.reward_dim, self.net_arch = obs_shape, action_shape, reward_dim, net_arch
        obs_dim, action_dim = int(np.array(obs_shape).prod()), int(np.array(action_shape).prod())
        self.critic = _mlp(obs_dim, reward_dim, list(net_arch))
        self.critic.apply(lambda layer: _layer_init(layer, np.sqrt(2)))
        _layer_init(list(self.critic.modules())[-1], 1.0)
        self.actor_mean = _mlp(obs_dim, action_dim, list(net_arch))
        self.actor_mean.apply(lambda layer: _layer_init(layer, np.sqrt(2)))
        _layer_init(list(self.actor_mean.modules())[-1], 0.01)
        self.actor_logstd = nn.Parameter(th.zeros(1, action_dim))


class PPOReplayBuffer:
    """``mo_ppo.py:22-104``: the rollout of one iteration, [size][num_envs][...] on the device."""

    def __init__(self, size: int, num_envs: int, obs_shape: tuple, action_shape: tuple, reward_dim: int, device):
        self.size, self.ptr, self.num_envs, self.device = size, 0, num_envs, device
        self.obs = th.zeros((size, num_envs) + tuple(obs_shape), device=device)
        self.actions = th.zeros((size, num_envs) + tuple(action_shape), device=device)
        self.logprobs = th.zeros((size, num_envs), device=device)
        self.rewards = th.zeros((size, num_envs, reward_dim), dtype=th.float32, device=device)
        self.dones = th.zeros((size, num_envs), device=device)
        self.values = th.zeros((size, num_envs, reward_dim), dtype=th.float32, device=device)

    def add(self, obs, actions, logprobs, rewards, dones, values):
        for dst, src in ((self.obs, obs), (self.actions, actions), (self.logprobs, logprobs), (self.rewards, rewards),
                         (self.dones, dones), (self.values, values)):
            dst[self.ptr] = src
        self.ptr = (self.ptr + 1) % self.size

    def get(self, step: int):
        return (self.obs[step], self.actions[step], self.logprobs[step], self.rewards[step], self.dones[step], self.values[step])

    def get_all(self):
        return (self.obs, self.actions, self.logprobs, self.rewards, self.dones, self.values)


def epoch_steps(rng: np.random.Generator, b_inds: np.ndarray, minibatch_size: int) -> list:
    """One epoch of the reference's loop: shuffle ``b_inds`` in place, cut it into minibatches (copies; the last may be shorter)."""
    rng.shuffle(b_inds)
    return [b_inds[s:s + minibatch_size].copy() for s in range(0, len(b_inds), minibatch_size)]


def by_size(groups: list, steps: list) -> list:
    """Consecutive minibatches of one size form a call (a batch that ``num_minibatches`` does not divide ends every epoch with
    a shorter one, as in the reference: a call takes steps of one size)."""
    for mb in steps:
        if groups and len(groups[-1][-1]) == len(mb):
            groups[-1].append(mb)
        else:
            groups.append([mb])
    return groups


def run_epochs(rng: np.random.Generator, batch_size: int, minibatch_size: int, epochs: int, target_kl: Optional[float],
               update_n: Callable[[np.ndarray], th.Tensor]) -> th.Tensor:
    """The PPO learners' epoch schedule: the shuffles are drawn from ``rng`` call for call as the reference draws them and the
    steps of all epochs go to ``update_n(idx [n][M]) -> stats [n][8]`` in one call per run of equal-sized minibatches
    (``target_kl``: the calls of one epoch, then one read of its last ``approx_kl``, which may end the loop).  Returns the
    statistics of every step, concatenated."""
    b_inds = np.arange(batch_size)
    calls, stats = [], []
    for _ in range(epochs):
        by_size(calls, epoch_steps(rng, b_inds, minibatch_size))
        if target_kl is not None:
            stats += [update_n(np.stack(c)) for c in calls]
            calls = []
            if float(stats[-1][-1, STAT_NAMES.index("approx_kl")]) > target_kl:
                break
    stats += [update_n(np.stack(c)) for c in calls]
    return stats[0] if len(stats) == 1 else th.cat(stats)


class MOPPO(MOPolicy):
    """Modified PPO with a multi-objective value net and weighted-sum scalarisation of the advantages -- the constructor,
    ``train``, ``update``, ``eval``, ``change_weights`` and ``__deepcopy__`` of the reference class (``mo_ppo.py:238-608``)."""

    def __init__(self, id: int, networks: MOPPONet, weights: np.ndarray, envs, log: bool = False, steps_per_iteration: int = 2048,
                 num_minibatches: int = 32, update_epochs: int = 10, learning_rate: float = 3e-4, gamma: float = 0.995,
                 anneal_lr: bool = False, clip_coef: float = 0.2, ent_coef: float = 0.0, vf_coef: float = 0.5,
                 clip_vloss: bool = True, max_grad_norm: float = 0.5, norm_adv: bool = True, target_kl: Optional[float] = None,
                 gae: bool = True, gae_lambda: float = 0.95, device: Union[th.device, str] = "auto", seed: int = 42,
                 rng: Optional[np.random.Generator] = None, lib: Optional[NativeLib] = None):
        super().__init__(id, device)
        if log:
            raise NotImplementedError("MOPPO: W&B logging is not available here (log=True); the step statistics are in last_stats")
        self.device = th.device(self.device)
        self.lib = lib or load_library()
        self.id, self.envs, self.num_envs, self.networks, self.seed = id, envs, envs.num_envs, networks, seed
        self.np_random = rng if rng is not None else np.random.default_rng(self.seed)

        self.steps_per_iteration = steps_per_iteration
        self.np_weights = weights
        self.weights = th.from_numpy(weights).to(self.device)
        self.batch_size = int(self.num_envs * self.steps_per_iteration)
        self.num_minibatches = num_minibatches
        self.minibatch_size = int(self.batch_size // num_minibatches)
        self.update_epochs, self.learning_rate, self.gamma, self.anneal_lr = update_epochs, learning_rate, gamma, anneal_lr
        self.clip_coef, self.vf_coef, self.ent_coef, self.max_grad_norm = clip_coef, vf_coef, ent_coef, max_grad_norm
        self.norm_adv, self.target_kl, self.clip_vloss, self.gae_lambda, self.log, self.gae = (norm_adv, target_kl, clip_vloss,
                                                                                              gae_lambda, log, gae)

        if len(networks.obs_shape) != 1 or len(networks.action_shape) != 1:
            raise NotImplementedError("MOPPO: image observations / shaped actions are not supported: flat vectors only")
        arch = [int(h) for h in networks.net_arch]
        if not 1 <= len(arch) <= 2:
            raise ValueError(f"MOPPO: net_arch {arch} is not supported by the MO-PPO kernels: one or two hidden layers")
        if any(h not in SUPPORTED_HIDDEN for h in arch):
            raise ValueError(f"MOPPO: net_arch {arch} is not supported by the MO-PPO kernels (widths from {SUPPORTED_HIDDEN})")
        if self.minibatch_size < 1:
            raise ValueError(f"MOPPO: {num_minibatches} minibatches of a batch of {self.batch_size} rows")
        D, A, R = int(networks.obs_shape[0]), int(networks.action_shape[0]), int(networks.reward_dim)
        if len(np.asarray(weights).reshape(-1)) != R or np.asarray(weights).dtype != np.float32:
            raise ValueError(f"MOPPO: weights must be {R} float32 entries (they multiply float32 advantages, mo_ppo.py:475)")
        shape = (D, A, R, len(arch), arch[0], arch[1] if len(arch) > 1 else 0)
        P = self.lib.family_param_count("ppo", *shape, error=ValueError)
        self._ctx = Context(self.lib, "ppo", *shape, self.minibatch_size)
        self._dims = (D, A, R)
        self.params = th.zeros(P, dtype=th.float32, device=self.device)
        self.exp_avg = th.zeros_like(self.params)
        self.exp_avg_sq = th.zeros_like(self.params)
        bind_flat(self.networks, self.params)
        self.optimizer = FlatAdam(self.learning_rate, 1e-5, [p.shape for p in networks.parameters()], self.params, self.exp_avg,
                                  self.exp_avg_sq)
        self.last_stats = None           # [steps][8] device tensor of the last update(): STAT_NAMES per step

        self.batch = PPOReplayBuffer(self.steps_per_iteration, self.num_envs, networks.obs_shape, networks.action_shape, R,
                                     self.device)

    # -- parameters ----------------------------------------------------------------------------------------------------
    def __deepcopy__(self, memo):
        """``mo_ppo.py:343-376``: a copy of the networks and the rollout behind a context, parameter vector and (fresh, as in the
        reference) optimiser state of its own."""
        copied_net = deepcopy(self.networks)
        copied = type(self)(self.id, copied_net, self.weights.detach().cpu().numpy(), self.envs, self.log, self.steps_per_iteration,
                            self.num_minibatches, self.update_epochs, self.learning_rate, self.gamma, self.anneal_lr, self.clip_coef,
                            self.ent_coef, self.vf_coef, self.clip_vloss, self.max_grad_norm, self.norm_adv, self.target_kl, self.gae,
                            self.gae_lambda, self.device, lib=self.lib)
        copied.global_step = self.global_step
        copied.batch = deepcopy(self.batch)
        return copied

    def change_weights(self, new_weights: np.ndarray):
        """``mo_ppo.py:378-384``."""
        self.weights = th.from_numpy(deepcopy(new_weights)).to(self.device)

    # -- the device side -------------------------------------------------------------------------------------------------
    def _forward(self, obs: th.Tensor, eps: Optional[th.Tensor]):
        """``get_action_and_value`` (``eps`` [rows][A] standard-normal noise) or, with ``eps=None``, ``get_value``: one launch.
        Returns (action, logprob, value) device tensors; action and logprob are None for ``get_value``."""
        D, A, R = self._dims
        obs = obs.to(self.device, th.float32).reshape(-1, D).contiguous()
        rows = obs.shape[0]
        value = th.empty(rows, R, dtype=th.float32, device=self.device)
        action = logprob = eps_d = None
        if eps is not None:
            eps_d = eps.to(self.device, th.float32).reshape(rows, A).contiguous()
            action = th.empty(rows, A, dtype=th.float32, device=self.device)
            logprob = th.empty(rows, dtype=th.float32, device=self.device)
        self.lib.check_device(self.params, obs, value, eps_d)
        self.lib.check(self.lib.lib.morl_ppo_forward(self._ctx, self.params.data_ptr(), obs.data_ptr(), _ptr(eps_d), rows,
                                                     int(eps is None), _ptr(action), _ptr(logprob), value.data_ptr(),
                                                     self.lib.stream_of(value)))
        return action, logprob, value

    def _noise(self) -> th.Tensor:
        """The draw of ``Normal.sample()`` (``mo_ppo.py:225-227``) for ``num_envs`` rows, from torch's CPU generator."""
        shape = (self.num_envs, self._dims[1])
        return th.normal(th.zeros(shape), th.ones(shape))

    def _collect_samples(self, obs: th.Tensor, done: th.Tensor):
        """``mo_ppo.py:390-435``."""
        R = self._dims[2]
        for _ in range(self.steps_per_iteration):
            self.global_step += 1 * self.num_envs
            action, logprob, value = self._forward(obs, self._noise())
            next_obs, reward, next_terminated, next_truncated, info = self.envs.step(action.cpu().numpy())
            reward = th.tensor(reward).to(self.device).view(self.num_envs, R)
            self.batch.add(obs, action, logprob, reward, done, value)
            obs, done = th.Tensor(next_obs).to(self.device), th.Tensor(next_terminated).to(self.device)
        return obs, done

    def _compute_advantages(self, next_obs: th.Tensor, next_done: th.Tensor):
        """``mo_ppo.py:437-476``: uploads the rollout into the context's table and runs the reverse scan there.
        Returns (returns [T][E][R], scalarised advantages [T][E])."""
        D, A, R = self._dims
        T, E = self.steps_per_iteration, self.num_envs
        _, _, next_value = self._forward(next_obs, None)
        cols = [t.to(th.float32).contiguous() for t in self.batch.get_all()]
        obs, actions, logprobs, rewards, dones, values = cols
        next_done = next_done.to(self.device, th.float32).contiguous()
        weights = self.weights.to(th.float32).contiguous()
        returns = th.empty(T, E, R, dtype=th.float32, device=self.device)
        advantages = th.empty(T, E, dtype=th.float32, device=self.device)
        self.lib.check_device(*cols, next_done, weights, returns)
        stream = self.lib.stream_of(returns)
        self.lib.check(self.lib.lib.morl_ppo_set_rollout(self._ctx, obs.data_ptr(), actions.data_ptr(), logprobs.data_ptr(),
                                                         rewards.data_ptr(), dones.data_ptr(), values.data_ptr(), T, E, stream))
        self.lib.check(self.lib.lib.morl_ppo_gae(self._ctx, next_value.data_ptr(), next_done.data_ptr(), weights.data_ptr(),
                                                 float(self.gamma), float(self.gae_lambda), int(bool(self.gae)), returns.data_ptr(),
                                                 advantages.data_ptr(), stream))
        self._keep = (cols, next_value, next_done, weights)      # (alive until the launches on the stream have read them)
        return returns, advantages

    def eval(self, obs: np.ndarray, w=None):
        """``mo_ppo.py:478-490``: the observation repeated ``num_envs`` times, one sample, row 0."""
        obs = th.as_tensor(obs).float().to(self.device)
        obs = obs.unsqueeze(0).repeat(self.num_envs, 1)
        action, _, _ = self._forward(obs, self._noise())
        return action[0].detach().cpu().numpy()

    def _update_n(self, idx: np.ndarray) -> th.Tensor:
        n, M = idx.shape
        idx_dev = th.from_numpy(np.ascontiguousarray(idx, dtype=np.int32)).to(self.device)
        stats = th.empty(n, len(STAT_NAMES), dtype=th.float32, device=self.device)
        self.lib.check_device(self.params, self.exp_avg, self.exp_avg_sq, idx_dev, stats)
        self.lib.check(self.lib.lib.morl_ppo_update_n(
            self._ctx, self.params.data_ptr(), self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr(), n, idx_dev.data_ptr(), M,
            float(self.optimizer.param_groups[0]["lr"]), self.optimizer.steps, float(self.clip_coef), float(self.ent_coef),
            float(self.vf_coef), float(self.max_grad_norm), int(bool(self.clip_vloss)), int(bool(self.norm_adv)), stats.data_ptr(),
            self.lib.stream_of(stats)))
        self.optimizer.steps += n
        return stats

    def update(self):
        """``mo_ppo.py:492-558``.  The rollout, its returns and advantages are the ones the last ``_compute_advantages`` put into
        the context's table.  The shuffles are drawn from ``np_random`` call for call; the steps of all epochs go to the device
        in one ``morl_ppo_update_n`` call (``target_kl``: one call per epoch, and one read of the epoch's last ``approx_kl``)."""
        self.last_stats = run_epochs(self.np_random, self.batch_size, self.minibatch_size, self.update_epochs, self.target_kl,
                                     self._update_n)

    def train(self, start_time, current_iteration: int, max_iterations: int):
        """``mo_ppo.py:576-608``: one iteration of ``steps_per_iteration * num_envs`` environment steps and one ``update()``."""
        next_obs, _ = self.envs.reset(seed=self.seed)
        next_obs = th.Tensor(next_obs).to(self.device)
        next_done = th.zeros(self.num_envs).to(self.device)
        if self.anneal_lr:
            frac = 1.0 - (current_iteration - 1.0) / max_iterations
            self.optimizer.param_groups[0]["lr"] = frac * self.learning_rate
        next_obs, next_done = self._collect_samples(next_obs, next_done)
        self.returns, self.advantages = self._compute_advantages(next_obs, next_done)
        self.update()
