"""Lorenz Conditioned Networks on the HIP library (``multi_policy/lcn/lcn.py``).

LCN is PCN with another rule for which stored episodes are worth conditioning on: returns are compared by their Lorenz vectors
(the cumulative sums of their sorted objectives), strictly or blended with the sorted returns by ``lcn_lambda``.  The model, its
update and acting are PCN's kernels through PCN's methods (``morl_pcn_update_n``, ``morl_pcn_forward``); what this file adds is the
reference's selection, restated line by line, with its all-pairs part -- dominance, distance to the closest front point, the
duplicate penalty, the crowding factor -- as ONE ``morl_lcn_select`` launch per ``_nlargest``.  With LCN's defaults the heap holds
500 episodes and is re-scored every training iteration and in every ``evaluate()``.

The kernel reproduces numpy's float32 arithmetic bit for bit (rounding order, summation order, a correctly rounded square root):
the heap keys, ``np.argsort``'s tie order, the commands and with them the action stream of a seeded ``train()`` hang on those
bits.  The crowding distance stays on the host: the reference forms it with an unstable ``np.argsort`` over ties, whose order is
numpy's implementation and nothing a kernel can restate; the host uploads its N flags.
"""
from __future__ import annotations

import heapq
import os
from typing import List, Optional, Type, Union

import numpy as np
import torch as th

from .native import NativeLib
from .pcn import PCN, Transition, crowding_distance

MAX_EPISODES = 2048                 # MORL_LCN_MAX_N of include/morl_hip.h
MODES = {"pareto": 0, "nondominated": 1, "lambda_lorenz": 2}


def lorenz_vector(points: np.ndarray, proportional: bool = False) -> np.ndarray:
    """``lcn.py:26-45``."""
    sorted_points = np.sort(points, axis=1)
    lv = np.cumsum(sorted_points, axis=1)
    if proportional:
        lv = lv / np.sum(points, axis=1, keepdims=True)
    return lv


class LCN(PCN):
    """Lorenz Conditioned Networks (Michailidis, Ropke, Roijers, Ghebreab & Santos, JAIR 85, 2026) -- constructor, ``get_config``,
    ``train``, ``evaluate``, ``save`` / ``load`` of the reference class."""

    def __init__(self, env, scaling_factor: np.ndarray, learning_rate: float = 1e-2, gamma: float = 1.0, batch_size: int = 32,
                 hidden_dim: int = 64, noise: float = 0.1, distance_ref: str = "nondominated", lcn_lambda: Optional[float] = None,
                 project_name: str = "MORL-Baselines", experiment_name: str = "LCN", wandb_entity: Optional[str] = None,
                 log: bool = True, seed: Optional[int] = None, device: Union[th.device, str] = "auto",
                 model_class: Optional[Type] = None, lib: Optional[NativeLib] = None) -> None:
        if distance_ref not in ("nondominated", "lambda_lorenz"):
            raise ValueError(f"distance_ref {distance_ref!r}: LCN knows 'nondominated' (strict Lorenz dominance) and 'lambda_lorenz'")
        if distance_ref == "lambda_lorenz" and lcn_lambda is None:
            raise ValueError("lcn_lambda must be set when using distance_ref='lambda_lorenz'")      # lcn.py:227
        self.distance_ref = distance_ref
        self.lcn_lambda = lcn_lambda
        self.cd_threshold = 0.2             # (train() sets it, lcn.py:428; the reference's default for callers that skip train())
        PCN.__init__(self, env, scaling_factor, learning_rate=learning_rate, gamma=gamma, batch_size=batch_size,
                     hidden_dim=hidden_dim, noise=noise, project_name=project_name, experiment_name=experiment_name,
                     wandb_entity=wandb_entity, log=log, seed=seed, device=device, model_class=model_class, lib=lib)

    def get_config(self) -> dict:
        """``lcn.py:148-163``."""
        return {
            "env_id": self.env.unwrapped.spec.id,
            "reward_dim": self.reward_dim,
            "batch_size": self.batch_size,
            "gamma": self.gamma,
            "learning_rate": self.learning_rate,
            "hidden_dim": self.hidden_dim,
            "scaling_factor": self.scaling_factor,
            "continuous_action": self.continuous_action,
            "noise": self.noise,
            "distance_ref": self.distance_ref,
            "lcn_lambda": self.lcn_lambda,
            "seed": self.seed,
        }

    # -- the device side -----------------------------------------------------------------------------------------------
    def _select(self, returns: np.ndarray, mode: int, crowded: Optional[np.ndarray] = None):
        """One ``morl_lcn_select`` launch on ``returns`` [N][R]: (l2 [N] float32 or None, front mask [N] bool).  Without ``crowded``
        only the mask is computed."""
        returns = np.ascontiguousarray(returns, dtype=np.float32)
        if returns.ndim != 2:
            raise ValueError("returns need one row per episode")
        N, R = returns.shape
        if not 1 <= N <= MAX_EPISODES:
            raise ValueError(f"{N} episodes: the selection kernel holds 1..{MAX_EPISODES}")
        ret = th.from_numpy(returns).to(self.device)
        nd = th.empty(N, dtype=th.uint8, device=self.device)
        sma = l2 = None
        if crowded is not None:
            sma = th.from_numpy(np.ascontiguousarray(crowded, dtype=np.uint8)).to(self.device)
            l2 = th.empty(N, dtype=th.float32, device=self.device)
        self.lib.check_device(ret, nd, sma, l2)
        lam = 0.0 if self.lcn_lambda is None else float(self.lcn_lambda)
        self.lib.check(self.lib.lib.morl_lcn_select(ret.data_ptr(), N, R, mode, lam, None if sma is None else sma.data_ptr(),
                                                    None if l2 is None else l2.data_ptr(), nd.data_ptr(),
                                                    self.lib.stream_of(nd)))
        if l2 is None:
            return None, nd.cpu().numpy().astype(bool)
        out = th.cat((l2.view(th.uint8), nd)).cpu().numpy()          # one read-back
        return out[:4 * N].view(np.float32).copy(), out[4 * N:].astype(bool)

    # -- experience replay (lcn.py:213-282) --------------------------------------------------------------------------------
    def _nlargest(self, n: int, threshold: float = 0.2):
        """``lcn.py:213-260``; lines 226-252 (dominance, distances, penalties) are the ``morl_lcn_select`` launch."""
        returns = np.array([e[2][0].reward for e in self.experience_replay])
        # crowding distance of each point, check ones that are too close together
        distances = crowding_distance(returns)
        sma = np.argwhere(distances <= threshold).flatten()
        crowded = np.zeros(len(returns), dtype=np.uint8)
        crowded[sma] = 1

        l2, _ = self._select(returns, MODES[self.distance_ref], crowded)

        sorted_i = np.argsort(l2)
        largest = [self.experience_replay[i] for i in sorted_i[-n:]]
        # before returning largest elements, update all distances in heap
        for i in range(len(l2)):
            self.experience_replay[i] = (l2[i], self.experience_replay[i][1], self.experience_replay[i][2])
        heapq.heapify(self.experience_replay)
        self._replay_changed()
        return largest

    def _choose_commands(self, num_episodes: int):
        """``lcn.py:262-282``."""
        # get best episodes, according to their crowding distance
        episodes = self._nlargest(num_episodes, self.cd_threshold)
        returns, horizons = list(zip(*[(e[2][0].reward, len(e[2])) for e in episodes]))
        # keep only Lorenz-non-dominated returns (strict Lorenz dominance whatever distance_ref is, lcn.py:267-268)
        _, nd_i = self._select(np.array(returns), MODES["nondominated"])
        returns = np.array(returns)[nd_i]
        horizons = np.array(horizons)[nd_i]
        # pick random return from random best episode
        r_i = self.np_random.integers(0, len(returns))
        desired_horizon = np.float32(horizons[r_i] - 2)
        # mean and std per objective
        _, s = np.mean(returns, axis=0), np.std(returns, axis=0)
        # desired return is sampled from [M, M+S], to try to do better than mean return
        desired_return = returns[r_i].copy()
        # random objective
        r_i = self.np_random.integers(0, len(desired_return))
        desired_return[r_i] += self.np_random.uniform(high=s[r_i])
        desired_return = np.float32(desired_return)
        return desired_return, desired_horizon

    def evaluate(self, env, max_return, n=10):
        """``lcn.py:342-358``."""
        n = min(n, len(self.experience_replay))
        episodes = self._nlargest(n, self.cd_threshold)
        returns, horizons = list(zip(*[(e[2][0].reward, len(e[2])) for e in episodes]))
        returns = np.float32(returns)
        horizons = np.float32(horizons)
        e_returns = []
        for i in range(n):
            transitions = self._run_episode(env, returns[i], np.float32(horizons[i]), max_return, eval_mode=True)
            # compute return
            for i in reversed(range(len(transitions) - 1)):
                transitions[i].reward += self.gamma * transitions[i + 1].reward
            e_returns.append(transitions[0].reward)

        distances = np.linalg.norm(np.array(returns) - np.array(e_returns), axis=-1)
        return e_returns, np.array(returns), distances

    # -- persistence (lcn.py:360-370) ----------------------------------------------------------------------------------------
    def save(self, filename: str = "LCN_model", save_dir: str = "weights"):
        """``lcn.py:360-364``: the whole model object."""
        if not os.path.isdir(save_dir):
            os.makedirs(save_dir)
        th.save(self.model, f"{save_dir}/{filename}.pt")

    def load(self, path: str):
        """``lcn.py:366-370``; the loaded parameters (ours or a reference model's ``state_dict`` names) move into the flat buffer."""
        PCN.load(self, path)

    # -- training loop (lcn.py:372-529) ----------------------------------------------------------------------------------------
    def train(self, total_timesteps: int, eval_env, ref_point: np.ndarray, known_pareto_front: Optional[List[np.ndarray]] = None,
              num_eval_weights_for_eval: int = 50, num_er_episodes: int = 500, num_step_episodes: int = 10,
              num_model_updates: int = 100, max_return: np.ndarray = None, max_buffer_size: int = 500, num_points_pf: int = 100,
              save_dir: str = "weights", cd_threshold: float = 0.2):
        """``lcn.py:372-529``; the ``num_model_updates`` updates of an iteration are one ``update_n`` call."""
        if not 1 <= max_buffer_size <= MAX_EPISODES:
            raise ValueError(f"max_buffer_size {max_buffer_size}: the selection kernel holds 1..{MAX_EPISODES} episodes")
        max_return = max_return if max_return is not None else np.full(self.reward_dim, 100.0, dtype=np.float32)
        if self.log:
            self.register_additional_config({
                "total_timesteps": total_timesteps, "ref_point": ref_point.tolist(), "known_front": known_pareto_front,
                "num_eval_weights_for_eval": num_eval_weights_for_eval, "num_er_episodes": num_er_episodes,
                "num_step_episodes": num_step_episodes, "num_model_updates": num_model_updates,
                "max_return": max_return.tolist(), "max_buffer_size": max_buffer_size, "num_points_pf": num_points_pf,
                "save_dir": save_dir, "distance_ref": self.distance_ref, "lcn_lambda": self.lcn_lambda,
                "cd_threshold": cd_threshold})
        self.global_step = 0
        total_episodes = num_er_episodes
        n_checkpoints = 0
        self.cd_threshold = cd_threshold
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
            # add episode in-place
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

            if self.global_step >= (n_checkpoints + 1) * total_timesteps / 100:
                self.save(save_dir=save_dir, filename=f"LCN_model_{n_checkpoints}")
                n_checkpoints += 1
                e_returns, _, _ = self.evaluate(eval_env, max_return, n=num_points_pf)

                if self.log:
                    from morl_baselines.common.evaluation import log_all_multi_policy_metrics   # (logging needs the reference + wandb)
                    log_all_multi_policy_metrics(current_front=e_returns, hv_ref_point=ref_point, reward_dim=self.reward_dim,
                                                 global_step=self.global_step, n_sample_weights=num_eval_weights_for_eval,
                                                 ref_front=known_pareto_front)

        self.env.close()
