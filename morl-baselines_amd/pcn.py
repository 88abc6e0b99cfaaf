"""Pareto Conditioned Networks on the HIP library (``multi_policy/pcn/pcn.py``).

The model's parameters live in one flat device tensor (``s_emb.0``, ``c_emb.0``, ``fc.0``, ``fc.2``, each weight before its
bias); ``update_n(n)`` draws the batches of ``n`` updates from ``np_random`` exactly as ``n`` calls of the reference's
``update()`` would (``pcn.py:206-212``), turns every draw into a row of the device-resident transition table and makes ONE
``morl_pcn_update_n`` call: gather, forward, loss, backward and Adam of every step run on the device, one launch per step,
nothing in between comes back to the host.  Acting goes through ``morl_pcn_forward``; sampling the action from the
log-probabilities stays on the host because the reference draws it from ``np_random`` (``pcn.py:321``).

The experience replay is the reference's host heap of ``(distance, step, transitions)`` -- at most ``max_buffer_size`` = 100
episodes, touched once per training iteration -- restated here line by line; whenever it changes it is flattened once into the
transition table (one row per stored transition: ``obs | action | return-to-go | steps left``).
"""
from __future__ import annotations

import heapq
import os
from dataclasses import dataclass
from typing import List, Optional, Type, Union

import numpy as np
import torch as th
from torch import nn

from .acnets import bind, flat_views
from .api import MOAgent, MOPolicy
from .native import Context, NativeLib, load_library
from .pareto import get_non_dominated_inds

SUPPORTED_HIDDEN = (32, 64, 96, 128)


def crowding_distance(points):
    """``pcn.py:22-37``."""
    points = (points - points.min(axis=0)) / (np.ptp(points, axis=0) + 1e-8)
    dim_sorted = np.argsort(points, axis=0)
    point_sorted = np.take_along_axis(points, dim_sorted, axis=0)
    distances = np.abs(point_sorted[:-2] - point_sorted[2:])
    distances = np.pad(distances, ((1,), (0,)), constant_values=1)
    crowding = np.zeros(points.shape)
    crowding[dim_sorted, np.arange(points.shape[-1])] = distances
    crowding = np.sum(crowding, axis=-1)
    return crowding


@dataclass
class Transition:
    """``pcn.py:40-48``."""

    observation: np.ndarray
    action: Union[float, int]
    reward: np.ndarray
    next_observation: np.ndarray
    terminal: bool


class PCNModel(nn.Module):
    """Parameter shell with the reference's module tree (``pcn.py:51-103``): ``scaling_factor``, ``s_emb``, ``c_emb``, ``fc``.

    The layers are built in the reference's order with ``nn.Linear``'s default initialisation (PCN does not re-initialise), so a
    seeded construction draws the reference's initial parameters.  The forward pass is ``morl_pcn_forward``; the shell only holds
    the parameters (as views of the agent's flat device tensor) and is what ``save`` pickles."""

    def __init__(self, state_dim: int, action_dim: int, reward_dim: int, scaling_factor: np.ndarray, hidden_dim: int,
                 continuous: bool):
        super().__init__()
        self.state_dim, self.action_dim, self.reward_dim, self.hidden_dim = state_dim, action_dim, reward_dim, hidden_dim
        self.continuous = continuous
        self.scaling_factor = nn.Parameter(th.tensor(scaling_factor).float(), requires_grad=False)
        self.s_emb = nn.Sequential(nn.Linear(state_dim, hidden_dim), nn.Sigmoid())
        self.c_emb = nn.Sequential(nn.Linear(reward_dim + 1, hidden_dim), nn.Sigmoid())
        head = [nn.Linear(hidden_dim, hidden_dim), nn.ReLU(), nn.Linear(hidden_dim, action_dim)]
        if not continuous:
            head.append(nn.LogSoftmax(dim=1))
        self.fc = nn.Sequential(*head)


class PCN(MOAgent, MOPolicy):
    """Pareto Conditioned Networks (Reymond, Bargiacchi & Nowe, AAMAS 2022) -- constructor, ``get_config``, ``train``, ``evaluate``,
    ``save`` / ``load`` of the reference class."""

    def __init__(self, env, scaling_factor: np.ndarray, learning_rate: float = 1e-3, gamma: float = 1.0, batch_size: int = 256,
                 hidden_dim: int = 64, noise: float = 0.1, project_name: str = "MORL-Baselines", experiment_name: str = "PCN",
                 wandb_entity: Optional[str] = None, log: bool = True, seed: Optional[int] = None,
                 device: Union[th.device, str] = "auto", model_class: Optional[Type] = None,
                 lib: Optional[NativeLib] = None) -> None:
        MOAgent.__init__(self, env, device=device, seed=seed)
        MOPolicy.__init__(self, device=device)
        if model_class is not None:
            raise NotImplementedError("a custom model_class has no HIP kernels: PCN runs the reference's default models only")
        if len(self.observation_shape) != 1:
            raise NotImplementedError("image observations are not supported: PCN takes flat observation vectors")
        if hidden_dim not in SUPPORTED_HIDDEN:
            raise ValueError(f"hidden_dim {hidden_dim} is not supported by the PCN kernels (one of {SUPPORTED_HIDDEN})")
        self.device = th.device(self.device)
        self.lib = lib or load_library()
        self.experience_replay = []  # List of (distance, time_step, transition)
        self.batch_size = batch_size
        self.gamma = gamma
        self.learning_rate = learning_rate
        self.hidden_dim = hidden_dim
        self.scaling_factor = scaling_factor
        self.desired_return = None
        self.desired_horizon = None
        self.continuous_action = not hasattr(self.env.action_space, "n")
        self.noise = noise

        D, A, R, H = int(self.observation_dim), int(self.action_dim), int(self.reward_dim), int(hidden_dim)
        if len(np.asarray(scaling_factor).reshape(-1)) != R + 1:
            raise ValueError(f"scaling_factor needs reward_dim + 1 = {R + 1} entries")
        P = self.lib.family_param_count("pcn", D, R, A, H, error=ValueError)
        self._ctx = Context(self.lib, "pcn", D, R, A, H, int(self.continuous_action), int(batch_size))
        self._dims = (D, R, A, H)
        self.params = th.zeros(P, dtype=th.float32, device=self.device)
        self.exp_avg = th.zeros_like(self.params)
        self.exp_avg_sq = th.zeros_like(self.params)
        self._adam_step = 0
        self.model = PCNModel(D, A, R, np.asarray(scaling_factor), H, self.continuous_action)   # the reference's draw order
        self._bind_model()
        self._table_rows = None          # (offset of every stored episode in the device table; None: replay changed since)
        self._table_keep = None

        self.log = log
        if log:
            experiment_name += " continuous action" if self.continuous_action else ""
            self.setup_wandb(project_name, experiment_name, wandb_entity)

    # -- parameters ----------------------------------------------------------------------------------------------------
    def _views(self, flat: th.Tensor):
        D, R, A, H = self._dims
        return flat_views(flat, [(H, D), (H,), (H, R + 1), (H,), (H, H), (H,), (A, H), (A,)])

    def _bind_model(self):
        bind(self.model, [self.model.scaling_factor.detach().to(self.device)] + self._views(self.params))
        self._scaling = self.model.scaling_factor.data.contiguous()

    def parameter_views(self):
        """The eight trainable tensors in the reference's ``model.parameters()`` order (views of the flat buffer)."""
        return self._views(self.params)

    def get_config(self) -> dict:
        """``pcn.py:188-200``."""
        return {
            "env_id": self.env.unwrapped.spec.id,
            "batch_size": self.batch_size,
            "gamma": self.gamma,
            "learning_rate": self.learning_rate,
            "hidden_dim": self.hidden_dim,
            "scaling_factor": self.scaling_factor,
            "continuous_action": self.continuous_action,
            "noise": self.noise,
            "seed": self.seed,
        }

    # -- the device side ---------------------------------------------------------------------------------------------------
    def _forward(self, obs: np.ndarray, desired_return: np.ndarray, desired_horizon: np.ndarray) -> np.ndarray:
        """``model(obs, desired_return, desired_horizon)`` for ``rows >= 1`` rows: one ``morl_pcn_forward`` launch."""
        D, R, A, H = self._dims
        f32 = lambda a, w: th.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float32).reshape(-1, w))).to(self.device)  # noqa: E731
        o, dr, dh = f32(obs, D), f32(desired_return, R), f32(desired_horizon, 1)
        if not (o.shape[0] == dr.shape[0] == dh.shape[0]):
            raise ValueError("obs, desired_return and desired_horizon need one row each per query")
        out = th.empty(o.shape[0], A, dtype=th.float32, device=self.device)
        self.lib.check_device(self.params, o, out)
        self.lib.check(self.lib.lib.morl_pcn_forward(self._ctx, self.params.data_ptr(), self._scaling.data_ptr(), o.data_ptr(),
                                                     dr.data_ptr(), dh.data_ptr(), o.shape[0], out.data_ptr(),
                                                     self.lib.stream_of(out)))
        return out.cpu().numpy()

    def _sync_table(self):
        """Flatten the replay into the device table -- once per change of the replay, not once per update."""
        if self._table_rows is not None and self._table_keep is self.experience_replay:
            return
        if len(self.experience_replay) == 0:
            raise RuntimeError("PCN.update: the experience replay is empty (train() fills it with random episodes first)")
        D, R, A, H = self._dims
        aw = A if self.continuous_action else 1
        n = sum(len(e[2]) for e in self.experience_replay)
        tab = np.empty((n, D + aw + R + 1), dtype=np.float32)
        starts, r = [], 0
        for _, _, ep in self.experience_replay:
            starts.append(r)
            for t, tr in enumerate(ep):
                tab[r, :D] = np.asarray(tr.observation, dtype=np.float32).reshape(-1)
                tab[r, D:D + aw] = np.asarray(tr.action, dtype=np.float32).reshape(-1)
                tab[r, D + aw:D + aw + R] = np.float32(tr.reward)          # return-to-go (pcn.py:214, 240-241)
                tab[r, D + aw + R] = np.float32(len(ep) - t)
                r += 1
        dev = th.from_numpy(tab).to(self.device)
        self.lib.check_device(dev)
        self.lib.check(self.lib.lib.morl_pcn_set_table(self._ctx, dev.data_ptr(), n, self.lib.stream_of(dev)))
        self._table_dev = dev            # (alive until the copy on the stream has run)
        self._table_rows = np.asarray(starts, dtype=np.int64)
        self._table_len = n
        self._table_keep = self.experience_replay

    def _replay_changed(self):
        self._table_rows = None

    def _draw_indices(self, n: int) -> np.ndarray:
        """The draws of ``n`` consecutive ``update()`` calls (``pcn.py:206-212``): per update one ``choice(size=B)``, then B scalar
        ``integers`` calls in batch order.  Returns the table rows, [n][B] int32."""
        n_ep = len(self.experience_replay)
        lens = [len(e[2]) for e in self.experience_replay]
        idx = np.empty((n, self.batch_size), dtype=np.int32)
        for k in range(n):
            s_i = self.np_random.choice(np.arange(n_ep), size=self.batch_size, replace=True)
            for b, i in enumerate(s_i):
                t = self.np_random.integers(0, lens[i])
                idx[k, b] = self._table_rows[i] + t
        return idx

    def update_n(self, n: int):
        """``n`` calls of the reference's ``update()``: returns (losses [n], entropies [n] or None, last predictions [B][A]),
        device tensors; nothing is read back here."""
        if n < 1:
            raise ValueError("update_n needs n >= 1")
        self._sync_table()
        idx = self._draw_indices(n)
        assert 0 <= int(idx.min()) and int(idx.max()) < self._table_len
        D, R, A, H = self._dims
        idx_dev = th.from_numpy(idx).to(self.device)
        loss = th.empty(n, dtype=th.float32, device=self.device)
        ent = None if self.continuous_action else th.empty(n, dtype=th.float32, device=self.device)
        pred = th.empty(self.batch_size, A, dtype=th.float32, device=self.device)
        self.lib.check_device(self.params, self.exp_avg, self.exp_avg_sq, idx_dev, loss, pred)
        self.lib.check(self.lib.lib.morl_pcn_update_n(
            self._ctx, self.params.data_ptr(), self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr(), self._scaling.data_ptr(), n,
            idx_dev.data_ptr(), self.batch_size, float(self.learning_rate), self._adam_step, loss.data_ptr(),
            None if ent is None else ent.data_ptr(), pred.data_ptr(), self.lib.stream_of(loss)))
        self._adam_step += n
        return loss, ent, pred

    def update(self):
        """``pcn.py:202-236``: one update; returns (loss, prediction) like the reference."""
        loss, _, pred = self.update_n(1)
        return loss[0], pred

    # -- experience replay (host heap, pcn.py:238-300) -------------------------------------------------------------------
    def _add_episode(self, transitions: List[Transition], max_size: int, step: int) -> None:
        """``pcn.py:238-248``."""
        for i in reversed(range(len(transitions) - 1)):
            transitions[i].reward += self.gamma * transitions[i + 1].reward
        if len(self.experience_replay) == max_size:
            heapq.heappushpop(self.experience_replay, (1, step, transitions))
        else:
            heapq.heappush(self.experience_replay, (1, step, transitions))
        self._replay_changed()

    def _nlargest(self, n, threshold=0.2):
        """``pcn.py:250-279``."""
        returns = np.array([e[2][0].reward for e in self.experience_replay])
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
        largest = [self.experience_replay[i] for i in sorted_i[-n:]]
        for i in range(len(l2)):
            self.experience_replay[i] = (l2[i], self.experience_replay[i][1], self.experience_replay[i][2])
        heapq.heapify(self.experience_replay)
        self._replay_changed()
        return largest

    def _choose_commands(self, num_episodes: int):
        """``pcn.py:281-300``."""
        episodes = self._nlargest(num_episodes)
        returns, horizons = list(zip(*[(e[2][0].reward, len(e[2])) for e in episodes]))
        nd_i = get_non_dominated_inds(np.array(returns))
        returns = np.array(returns)[nd_i]
        horizons = np.array(horizons)[nd_i]
        r_i = self.np_random.integers(0, len(returns))
        desired_horizon = np.float32(horizons[r_i] - 2)
        _, s = np.mean(returns, axis=0), np.std(returns, axis=0)
        desired_return = returns[r_i].copy()
        r_i = self.np_random.integers(0, len(desired_return))
        desired_return[r_i] += self.np_random.uniform(high=s[r_i])
        desired_return = np.float32(desired_return)
        return desired_return, desired_horizon

    # -- acting (pcn.py:302-358) -----------------------------------------------------------------------------------------
    def _act(self, obs: np.ndarray, desired_return, desired_horizon, eval_mode=False):
        """``pcn.py:302-322``."""
        prediction = self._forward(np.array([obs]), np.array([desired_return]), np.array([desired_horizon]))
        self.last_prediction = prediction[0]
        if self.continuous_action:
            action = prediction[0]
            if not eval_mode:
                # the reference draws this from the GLOBAL numpy generator, not from np_random (pcn.py:313)
                action = action + np.random.normal(0.0, self.noise)
            return action
        log_probs = prediction[0]
        if eval_mode:
            action = np.argmax(log_probs)
        else:
            action = self.np_random.choice(np.arange(len(log_probs)), p=np.exp(log_probs))
        return action

    def _run_episode(self, env, desired_return, desired_horizon, max_return, eval_mode=False):
        """``pcn.py:324-349``."""
        transitions = []
        obs, _ = env.reset()
        done = False
        while not done:
            action = self._act(obs, desired_return, desired_horizon, eval_mode)
            n_obs, reward, terminated, truncated, _ = env.step(action)
            done = terminated or truncated
            transitions.append(Transition(observation=obs, action=action, reward=np.float32(reward).copy(),
                                          next_observation=n_obs, terminal=terminated))
            obs = n_obs
            desired_return = np.clip(desired_return - reward, None, max_return, dtype=np.float32)
            desired_horizon = np.float32(max(desired_horizon - 1, 1.0))
        return transitions

    def set_desired_return_and_horizon(self, desired_return: np.ndarray, desired_horizon: int):
        """``pcn.py:351-354``."""
        self.desired_return = desired_return
        self.desired_horizon = desired_horizon

    def eval(self, obs, w=None):
        """``pcn.py:356-358``."""
        return self._act(obs, self.desired_return, self.desired_horizon, eval_mode=True)

    def evaluate(self, env, max_return, n=10):
        """``pcn.py:360-376``."""
        n = min(n, len(self.experience_replay))
        episodes = self._nlargest(n)
        returns, horizons = list(zip(*[(e[2][0].reward, len(e[2])) for e in episodes]))
        returns = np.float32(returns)
        horizons = np.float32(horizons)
        e_returns = []
        for i in range(n):
            transitions = self._run_episode(env, returns[i], np.float32(horizons[i]), max_return, eval_mode=True)
            for i in reversed(range(len(transitions) - 1)):
                transitions[i].reward += self.gamma * transitions[i + 1].reward
            e_returns.append(transitions[0].reward)
        distances = np.linalg.norm(np.array(returns) - np.array(e_returns), axis=-1)
        return e_returns, np.array(returns), distances

    # -- persistence (pcn.py:378-388) -----------------------------------------------------------------------------------------
    def save(self, filename: str = "PCN_model", save_dir: str = "weights"):
        """``pcn.py:378-382``: the whole model object."""
        if not os.path.isdir(save_dir):
            os.makedirs(save_dir)
        th.save(self.model, f"{save_dir}/{filename}.pt")

    def load(self, path: str):
        """``pcn.py:384-388``; the loaded parameters (ours or a reference model's ``state_dict`` names) move into the flat buffer."""
        if not os.path.isfile(path):
            raise FileNotFoundError(f"Model file {path} does not exist.")
        loaded = th.load(path, map_location="cpu", weights_only=False)
        sd = loaded.state_dict()
        names = ["s_emb.0.weight", "s_emb.0.bias", "c_emb.0.weight", "c_emb.0.bias", "fc.0.weight", "fc.0.bias", "fc.2.weight",
                 "fc.2.bias"]
        with th.no_grad():
            for v, k in zip(self._views(self.params), names):
                if tuple(sd[k].shape) != tuple(v.shape):
                    raise ValueError(f"{path}: {k} has shape {tuple(sd[k].shape)}, this agent needs {tuple(v.shape)}")
                v.copy_(sd[k].to(self.device))
            self.model.scaling_factor.data.copy_(sd["scaling_factor"].to(self.device))
        self._scaling = self.model.scaling_factor.data.contiguous()

    # -- training loop (pcn.py:390-538) --------------------------------------------------------------------------------------
    def train(self, total_timesteps: int, eval_env, ref_point: np.ndarray, known_pareto_front: Optional[List[np.ndarray]] = None,
              num_eval_weights_for_eval: int = 50, num_er_episodes: int = 20, num_step_episodes: int = 10,
              num_model_updates: int = 50, max_return: np.ndarray = None, max_buffer_size: int = 100, num_points_pf: int = 100):
        """``pcn.py:390-538``; the ``num_model_updates`` updates of an iteration are one ``update_n`` call."""
        max_return = max_return if max_return is not None else np.full(self.reward_dim, 100.0, dtype=np.float32)
        if self.log:
            self.register_additional_config({
                "total_timesteps": total_timesteps, "ref_point": ref_point.tolist(), "known_front": known_pareto_front,
                "num_eval_weights_for_eval": num_eval_weights_for_eval, "num_er_episodes": num_er_episodes,
                "num_step_episodes": num_step_episodes, "num_model_updates": num_model_updates,
                "max_return": max_return.tolist(), "max_buffer_size": max_buffer_size, "num_points_pf": num_points_pf})
        self.global_step = 0
        total_episodes = num_er_episodes
        n_checkpoints = 0
        self.command_log = []            # every (desired_return, desired_horizon) chosen, in order

        # fill buffer with random episodes
        self.experience_replay = []
        self._replay_changed()
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
                self.global_step += 1
            self._add_episode(transitions, max_size=max_buffer_size, step=self.global_step)

        while self.global_step < total_timesteps:
            losses, entropies, _ = self.update_n(num_model_updates)
            loss = list(losses.cpu().numpy())                       # the per-update values the reference collects
            entropy = [] if entropies is None else list(entropies.cpu().numpy())

            desired_return, desired_horizon = self._choose_commands(num_er_episodes)
            self.command_log.append((desired_return.copy(), np.float32(desired_horizon)))

            # get all leaves, contain biggest elements, experience_replay got heapified in choose_commands
            leaves_r = np.array([e[2][0].reward for e in self.experience_replay[len(self.experience_replay) // 2:]])

            if self.log:
                import wandb
                from .performance_indicators import hypervolume
                wandb.log({"train/hypervolume": hypervolume(ref_point, leaves_r), "train/loss": np.mean(loss),
                           "global_step": self.global_step})
                if not self.continuous_action:
                    wandb.log({"train/entropy": np.mean(entropy), "global_step": self.global_step})

            returns = []
            horizons = []
            for _ in range(num_step_episodes):
                transitions = self._run_episode(self.env, desired_return, desired_horizon, max_return)
                self.global_step += len(transitions)
                self._add_episode(transitions, max_size=max_buffer_size, step=self.global_step)
                returns.append(transitions[0].reward)
                horizons.append(len(transitions))

            total_episodes += num_step_episodes
            if self.log:
                import wandb
                wandb.log({"train/episode": total_episodes, "train/horizon_desired": desired_horizon,
                           "train/mean_horizon_distance": np.linalg.norm(np.mean(horizons) - desired_horizon),
                           "global_step": self.global_step})
                for i in range(self.reward_dim):
                    wandb.log({f"train/desired_return_{i}": desired_return[i],
                               f"train/mean_return_{i}": np.mean(np.array(returns)[:, i]),
                               f"train/mean_return_distance_{i}": np.linalg.norm(np.mean(np.array(returns)[:, i]) - desired_return[i]),
                               "global_step": self.global_step})
            print(f"step {self.global_step} \t return {np.mean(returns, axis=0)}, ({np.std(returns, axis=0)}) \t "
                  f"loss {np.mean(loss):.3E} \t horizons {np.mean(horizons)}")

            if self.global_step >= (n_checkpoints + 1) * total_timesteps / 1000:
                self.save()
                n_checkpoints += 1
                e_returns, _, _ = self.evaluate(eval_env, max_return, n=num_points_pf)

                if self.log:
                    from morl_baselines.common.evaluation import log_all_multi_policy_metrics   # (logging needs the reference + wandb)
                    log_all_multi_policy_metrics(current_front=e_returns, hv_ref_point=ref_point, reward_dim=self.reward_dim,
                                                 global_step=self.global_step, n_sample_weights=num_eval_weights_for_eval,
                                                 ref_front=known_pareto_front)
