"""Expected Utility Policy Gradient on the HIP library (``single_policy/esr/eupg.py``), the reference's ESR learner.

The policy reads ``obs | accrued reward`` and ends in a sigmoid normalised over the actions.  Once per episode ``update()`` uploads the
packed episode in ONE copy and makes two launches with the user's ``scalarization`` between them: ``morl_eupg_returns`` (the reverse
discounted scan) and ``morl_eupg_update`` (forward, ``-mean(logp * u)``, backward and Adam).  ``scalarization`` is called on the
device tensor of the returns, as the reference calls it on its tensor, and its result never leaves the device.

What the reference does by accident is kept: its episode buffer holds the observations as ``int32``, so ``update()`` trains on
observations truncated towards zero while acting sees them as floats.  The cast is numpy's assignment cast, on the host.

Actions are sampled on the host, ``Categorical(probs=...).sample()`` from torch's CPU generator on the probabilities the forward
launch returns, so a seeded run consumes the generator's stream as the reference does on the CPU.

Not here: W&B logging.  ``__deepcopy__`` copies the parameters and the optimiser's state (the reference's copy starts from a
freshly initialised network and steps an orphaned one).
"""
from __future__ import annotations

import time
from copy import deepcopy
from typing import Callable, List, Optional, Union

import numpy as np
import torch as th
from torch import nn
from torch.distributions import Categorical

from .acnets import FlatAdam, bind_flat
from .api import MOAgent, MOPolicy
from .native import Context, NativeLib, load_library

MAX_HIDDEN = 128


def _layer_init(layer) -> None:
    if isinstance(layer, nn.Linear):
        th.nn.init.orthogonal_(layer.weight, gain=1)
        th.nn.init.constant_(layer.bias, 0)


class PolicyNet(nn.Module):
    """Parameter shell with the reference's module tree (``eupg.py:22-44``): ``net``, an MLP with Tanh.  Every ``Linear`` is built
    with its default initialisation and ``apply`` then re-initialises them in module order (orthogonal, gain 1, zero bias), so a
    seeded construction draws the reference's initial parameters.  The forward pass is ``morl_eupg_forward``; the shell only holds
    the parameters, which ``EUPG`` turns into views of its flat device tensor."""

    def __init__(self, obs_shape, action_dim: int, rew_dim: int, net_arch: List[int]):
        super().__init__()
        self.obs_shape, self.action_dim, self.rew_dim = obs_shape, action_dim, rew_dim
        mods, width = [], obs_shape[0] + rew_dim
        for h in net_arch:
            mods += [nn.Linear(width, h), nn.Tanh()]
            width = h
        mods.append(nn.Linear(width, action_dim))
        self.net = nn.Sequential(*mods)
        self.apply(_layer_init)


class EpisodeBuffer:
    """The episode's rows on the host, with the interface of the reference's ``AccruedRewardReplayBuffer`` as EUPG uses it.
    Observations and actions are held as ``int32``: numpy's assignment cast truncates a float observation towards zero."""

    def __init__(self, obs_shape, action_shape, rew_dim: int = 1, max_size: int = 100000):
        self.max_size, self.ptr, self.size = max_size, 0, 0
        self.obs = np.zeros((max_size,) + tuple(obs_shape), dtype=np.int32)
        self.next_obs = np.zeros((max_size,) + tuple(obs_shape), dtype=np.int32)
        self.actions = np.zeros((max_size,) + tuple(action_shape), dtype=np.int32)
        self.rewards = np.zeros((max_size, rew_dim), dtype=np.float32)
        self.accrued_rewards = np.zeros((max_size, rew_dim), dtype=np.float32)
        self.dones = np.zeros((max_size, 1), dtype=np.float32)

    def add(self, obs, accrued_reward, action, reward, next_obs, done):
        i = self.ptr
        self.obs[i], self.next_obs[i], self.actions[i] = np.array(obs), np.array(next_obs), np.array(action)
        self.rewards[i], self.accrued_rewards[i], self.dones[i] = np.array(reward), np.array(accrued_reward), np.array(done)
        self.ptr = (self.ptr + 1) % self.max_size
        self.size = min(self.size + 1, self.max_size)

    def cleanup(self):
        self.size, self.ptr = 0, 0

    def get_all_data(self, to_tensor: bool = False, device=None):
        n = self.size
        out = (self.obs[:n], self.accrued_rewards[:n], self.actions[:n], self.rewards[:n], self.next_obs[:n], self.dones[:n])
        return tuple(th.tensor(x).to(device) for x in out) if to_tensor else tuple(x.copy() for x in out)

    def __len__(self):
        return self.size


class EUPG(MOPolicy, MOAgent):
    """Expected Utility Policy Gradient (Roijers, Steckelmacher & Nowe, 2018) -- the constructor, ``train``, ``update``, ``eval``,
    ``get_save_dict`` / ``load``, ``get_config`` and ``__deepcopy__`` of the reference class (``eupg.py:78-398``)."""

    def __init__(self, env, scalarization: Callable, weights: np.ndarray = np.ones(2), id: Optional[int] = None,
                 buffer_size: int = int(1e5), net_arch: List = [50], gamma: float = 0.99, learning_rate: float = 1e-3,
                 project_name: str = "MORL-Baselines", experiment_name: str = "EUPG", wandb_entity: Optional[str] = None,
                 log: bool = True, log_every: int = 1000, device: Union[th.device, str] = "auto", seed: Optional[int] = None,
                 parent_rng: Optional[np.random.Generator] = None, lib: Optional[NativeLib] = None):
        MOAgent.__init__(self, env, device, seed=seed)
        MOPolicy.__init__(self, None, device)
        if log:
            raise NotImplementedError("EUPG: W&B logging is not available here (log=True); the loss is in last_loss and the episode's "
                                      "scalarised return in last_scalarized_return")
        self.device = th.device(self.device)
        self.lib = lib or load_library()
        self.seed, self.parent_rng = seed, parent_rng
        self.np_random = parent_rng if parent_rng is not None else np.random.default_rng(self.seed)
        self.env, self.id = env, id
        self.scalarization, self.weights, self.gamma = scalarization, weights, gamma
        self.buffer_size, self.learning_rate = buffer_size, learning_rate
        self.net_arch = [int(h) for h in net_arch]
        if not 1 <= len(self.net_arch) <= 2:
            raise ValueError(f"EUPG: net_arch {self.net_arch} is not supported by the kernels: one or two hidden layers")
        if any(not 1 <= h <= MAX_HIDDEN for h in self.net_arch):
            raise ValueError(f"EUPG: net_arch {self.net_arch} is not supported by the kernels (widths from 1 to {MAX_HIDDEN})")
        if len(self.observation_shape) != 1:
            raise NotImplementedError("EUPG: image observations are not supported: flat vectors only")
        self.project_name, self.experiment_name, self.log, self.log_every = project_name, experiment_name, log, log_every
        self.buffer = EpisodeBuffer(self.observation_shape, self.action_shape, rew_dim=self.reward_dim, max_size=self.buffer_size)

        self._ctx, self._max_rows = None, 0
        self.net = PolicyNet(self.observation_shape, int(self.action_dim), self.reward_dim, self.net_arch)
        arch = self.net_arch
        self._shape = (int(self.observation_shape[0]), int(self.action_dim), int(self.reward_dim), len(arch), arch[0],
                       arch[1] if len(arch) > 1 else 0)
        P = self.lib.family_param_count("eupg", *self._shape, error=ValueError)
        self.params = th.zeros(P, dtype=th.float32, device=self.device)
        self.exp_avg = th.zeros_like(self.params)
        self.exp_avg_sq = th.zeros_like(self.params)
        bind_flat(self.net, self.params)
        self.optimizer = FlatAdam(self.learning_rate, 1e-8, [p.shape for p in self.net.parameters()], self.params, self.exp_avg,
                                  self.exp_avg_sq)
        self._reserve(1024)
        self.last_loss = None                  # 0-dim device tensor of the last update()
        self.last_scalarized_return = None     # scalarization(episodic return, weights) of the last update()
        self.last_returns = None               # [T][R] device tensor: the discounted returns of the last update()

    def _destroy(self):
        if self._ctx:
            self._ctx.close()

    def _reserve(self, rows: int):
        """A context whose table holds an episode of ``rows`` steps (episodes have no length limit in the reference)."""
        if rows <= self._max_rows:
            return
        self._destroy()
        rows = max(rows, 2 * self._max_rows)
        self._ctx, self._max_rows = Context(self.lib, "eupg", *self._shape, rows, 0), rows

    # -- the device side -------------------------------------------------------------------------------------------------
    def _probs(self, obs, acc_reward) -> th.Tensor:
        """One launch: the policy's probabilities [rows][A] on the device."""
        D, A, R = self._shape[:3]
        obs = th.as_tensor(obs).to(self.device, th.float32).reshape(-1, D).contiguous()
        rows = obs.shape[0]
        acc = th.as_tensor(acc_reward).to(self.device, th.float32).reshape(-1, R).expand(rows, R).contiguous()
        probs = th.empty(rows, A, dtype=th.float32, device=self.device)
        self.lib.check_device(self.params, obs, acc, probs)
        self.lib.check(self.lib.lib.morl_eupg_forward(self._ctx, self.params.data_ptr(), obs.data_ptr(), acc.data_ptr(), rows,
                                                      probs.data_ptr(), self.lib.stream_of(probs)))
        return probs

    def _choose_action(self, obs, accrued_reward) -> int:
        return Categorical(probs=self._probs(obs, accrued_reward).cpu()).sample().item()

    # -- the reference's interface -----------------------------------------------------------------------------------------
    def get_policy_net(self) -> nn.Module:
        return self.net

    def get_buffer(self):
        return self.buffer

    def set_buffer(self, buffer):
        raise Exception("On-policy algorithms should not share buffer.")

    def set_weights(self, weights: np.ndarray):
        self.weights = weights

    @th.no_grad()
    def eval(self, obs: np.ndarray, accrued_reward: Optional[np.ndarray]) -> Union[int, np.ndarray]:
        if type(obs) is int:
            obs = [obs]
        return self._choose_action(obs, th.as_tensor(accrued_reward).float())

    def update(self):
        """``eupg.py:227-251``: one optimiser step on the episode in the buffer."""
        obs, acc, actions, rewards, _, _ = self.buffer.get_all_data()
        T = len(obs)
        if T < 1:
            raise RuntimeError("EUPG.update(): the episode buffer is empty")
        D, A, R = self._shape[:3]
        self._reserve(T)
        # the scalarised episodic return stays on the host, from the rewards the buffer holds (eupg.py:237-239)
        episodic_return = th.sum(th.from_numpy(rewards), dim=0)
        self.last_scalarized_return = self.scalarization(episodic_return.numpy(), self.weights)
        # one upload: obs (the buffer's int32, as floats) | accrued rewards | actions (int32 words) | rewards
        packed = np.empty(T * (D + 2 * R + 1), dtype=np.float32)
        o_acc, o_act, o_rew = T * D, T * (D + R), T * (D + R + 1)
        packed[:o_acc] = obs.reshape(-1)
        packed[o_acc:o_act] = acc.reshape(-1)
        packed[o_act:o_rew].view(np.int32)[:] = actions.reshape(-1)
        packed[o_rew:] = rewards.reshape(-1)
        dev = th.from_numpy(packed).to(self.device)
        returns = th.empty(T, R, dtype=th.float32, device=self.device)
        loss = th.empty((), dtype=th.float32, device=self.device)
        self.lib.check_device(dev, returns, loss, self.params, self.exp_avg, self.exp_avg_sq)
        stream, base = self.lib.stream_of(dev), dev.data_ptr()
        self.lib.check(self.lib.lib.morl_eupg_set_episode(self._ctx, base, base + 4 * o_acc, base + 4 * o_act, base + 4 * o_rew, T, stream))
        self.lib.check(self.lib.lib.morl_eupg_returns(self._ctx, float(self.gamma), returns.data_ptr(), stream))
        u = self.scalarization(returns)
        u = th.as_tensor(u, device=self.device).to(th.float32).reshape(-1).contiguous()
        if u.numel() != T:
            raise ValueError(f"EUPG: scalarization returned {u.numel()} values for {T} rows")
        self.lib.check_device(u)
        self.lib.check(self.lib.lib.morl_eupg_update(self._ctx, self.params.data_ptr(), self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr(),
                                                     u.data_ptr(), float(self.optimizer.param_groups[0]["lr"]), self.optimizer.steps,
                                                     loss.data_ptr(), stream))
        self.optimizer.steps += 1
        self._keep = (dev, u)                  # (alive until the launches on the stream have read them)
        self.last_loss, self.last_returns = loss, returns

    def get_save_dict(self, save_replay_buffer: bool = True) -> dict:
        save_dict = {
            "policy_net_state_dict": {k: v.detach().clone() for k, v in self.net.state_dict().items()},
            "optimizer_state_dict": self.optimizer.state_dict(),
            "policy_weights": self.weights,
        }
        if save_replay_buffer:
            save_dict["replay_buffer"] = self.get_buffer()
        return save_dict

    def load(self, save_dict: Optional[dict] = None, path: Optional[str] = None, load_replay_buffer: bool = True):
        if save_dict is None:
            assert path is not None, "Either save_dict or path must be provided."
            save_dict = th.load(path, weights_only=False)
        with th.no_grad():
            sd = save_dict["policy_net_state_dict"]
            for name, p in self.net.named_parameters():     # (in place: the parameters stay views of the flat tensor)
                p.data.copy_(sd[name].to(p.device))
        self.optimizer.load_state_dict(save_dict["optimizer_state_dict"])
        self.weights = save_dict["policy_weights"]
        if load_replay_buffer and "replay_buffer" in save_dict:
            self.buffer = save_dict["replay_buffer"]

    def __deepcopy__(self, memo):
        copied = type(self)(self.env, self.scalarization, self.weights, self.id, self.buffer_size, self.net_arch, self.gamma,
                            self.learning_rate, self.project_name, self.experiment_name, log=self.log, device=self.device,
                            parent_rng=self.parent_rng, lib=self.lib)
        copied.global_step = self.global_step
        copied.params.copy_(self.params)
        copied.exp_avg.copy_(self.exp_avg)
        copied.exp_avg_sq.copy_(self.exp_avg_sq)
        copied.optimizer.steps = self.optimizer.steps
        copied.optimizer.param_groups[0]["lr"] = self.optimizer.param_groups[0]["lr"]
        copied.buffer = deepcopy(self.buffer)
        return copied

    def train(self, total_timesteps: int, eval_env=None, eval_freq: int = 1000, start_time=None):
        """``eupg.py:305-387``."""
        if start_time is None:
            start_time = time.time()
        obs, _ = self.env.reset()
        accrued_reward = th.zeros(self.reward_dim, dtype=th.float32)
        for _ in range(1, total_timesteps + 1):
            self.global_step += 1
            if type(obs) is int:
                obs = [obs]
            action = self._choose_action(th.Tensor(obs), accrued_reward)
            next_obs, vec_reward, terminated, truncated, info = self.env.step(action)
            self.buffer.add(obs, accrued_reward.numpy(), action, vec_reward, next_obs, terminated)
            accrued_reward += th.from_numpy(np.asarray(vec_reward))
            if terminated or truncated:
                self.update()                  # the network is updated at the end of each episode
                self.buffer.cleanup()
                obs, _ = self.env.reset()
                self.num_episodes += 1
                accrued_reward = th.zeros(self.reward_dim).float()
            else:
                obs = next_obs

    def get_config(self) -> dict:
        return {"env_id": self.env.unwrapped.spec.id, "learning_rate": self.learning_rate, "buffer_size": self.buffer_size,
                "gamma": self.gamma, "net_arch": self.net_arch, "seed": self.seed}
