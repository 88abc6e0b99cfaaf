"""Prediction-guided multi-objective RL on the HIP library (``multi_policy/pgmorl/pgmorl.py``).

``PerformancePredictor``, ``generate_weights``, ``PerformanceBuffer2d`` / ``PerformanceBuffer3d`` and ``PGMORL`` (constructor
arguments, ``get_config``, ``train``: warm-up, evaluation, task / weight selection, evolutionary generations) follow the
reference.  The agents are ``MOPPO`` objects (``mo_ppo.py``); what this file adds to them is the POPULATION: the ``pop_size``
learners of an iteration are independent, so their acting, advantage scan and minibatch steps go to the device as one launch per
step for all of them (``morl_ppo_forward_pop`` / ``morl_ppo_gae_pop`` / ``morl_ppo_update_n_pop``: the learner axis is a grid
axis, and every learner computes bit for bit what its own ``MOPPO.train()`` would).

Where this differs from the reference:

* Environments.  ``make_env`` and its gymnasium wrappers are not here (as in ``mo_ppo.py``): the constructor takes ``make_envs``,
  a callable returning a vector env (``num_envs``, ``reset(seed=)``, ``step(actions)``, ``single_observation_space`` /
  ``single_action_space`` or ``observation_space`` / ``action_space`` of ONE env, and ``reward_space``), instead of ``env_id``.
  The reference runs all agents on ONE vector env and re-seeds it at the start of each agent's rollout; here ``make_envs`` is
  called ``pop_size`` times and agent slot i always steps copy i.  The two are the same computation when ``reset(seed)``
  determines the episode stream, i.e. when a re-seeded env forgets what it did before.  ``log=True`` raises.
* Lock-step collection.  One ``morl_ppo_forward_pop`` launch and one host read per vector step serve all agents.  The exploration
  noise of an iteration is drawn BEFORE the loop, in agent order, one ``th.normal`` call of shape ``(num_envs, A)`` per step as
  ``MOPPO._noise`` draws it, so torch's CPU generator is consumed as ``pop_size`` sequential ``train()`` calls consume it (one
  large ``th.normal`` call would draw other numbers).  This needs environments that do not draw from torch's generator.
* Population update.  The epochs' shuffles are drawn from each agent's ``np_random`` in the reference's order (agent 0's epochs,
  then agent 1's, ...; in the warm-up the agents share one generator), then ONE ``morl_ppo_update_n_pop`` call is made per
  iteration (two where ``num_minibatches`` does not divide the batch: a call takes steps of one size).  With ``target_kl`` set:
  one call per epoch over the learners still active and one read of each active learner's last ``approx_kl`` -- unless agents
  share a generator: how many shuffles an agent consumes then depends on its KL, so the next agent's first shuffle is not known
  before the previous agent has finished, and the agents run their own ``update()`` one after the other.
* Hypervolume and sparsity in the task selection are this package's ``performance_indicators`` (no pymoo).
* Evaluation (``policy_eval``, five episodes per agent) is sequential as in the reference: its noise draws interleave with the
  environment's steps.
* ``pop_size`` above the number of generated weights is refused (the reference indexes past the end of the weight list).
"""
from __future__ import annotations

import ctypes as C
import time
from copy import deepcopy
from itertools import product
from typing import Callable, List, Optional, Tuple, Union

import numpy as np
import torch as th
from scipy.optimize import least_squares

from .api import MOAgent
from .mo_ppo import MOPPO, MOPPONet, STAT_NAMES, by_size, epoch_steps
from .native import NativeLib, load_library
from .pareto import ParetoArchive
from .performance_indicators import hypervolume, sparsity


class PerformancePredictor:
    """``pgmorl.py:27-202``: stores (weight, evaluation before, evaluation after) of every trained policy and fits, per objective,
    a hyperbolic model weight -> delta on the neighbours of the evaluation asked about."""

    def __init__(self, neighborhood_threshold: float = 0.1, sigma: float = 0.03, A_bound_min: float = 1.0,
                 A_bound_max: float = 500.0, f_scale: float = 20.0):
        self.previous_performance, self.next_performance, self.used_weight = [], [], []
        self.neighborhood_threshold = neighborhood_threshold
        self.A_bound_min, self.A_bound_max, self.f_scale, self.sigma = A_bound_min, A_bound_max, f_scale, sigma

    def add(self, weight: np.ndarray, eval_before_pg: np.ndarray, eval_after_pg: np.ndarray) -> None:
        self.previous_performance.append(eval_before_pg)
        self.next_performance.append(eval_after_pg)
        self.used_weight.append(weight)

    def _build_model_and_predict(self, training_weights, training_deltas, training_next_perfs, current_dim, current_eval,
                                 weight_candidate, sigma):
        """``pgmorl.py:80-148``: f = A (exp(a (x - b)) - 1) / (exp(a (x - b)) + 1) + c, soft-l1 least squares, the samples
        weighted by their distance to ``current_eval``."""
        def f(x, A, a, b, c):
            return A * (np.exp(a * (x - b)) - 1) / (np.exp(a * (x - b)) + 1) + c

        def hyperbolic_model(params, x, y):
            return (params[0] * (np.exp(params[1] * (x - params[2])) - 1.0) / (np.exp(params[1] * (x - params[2])) + 1)
                    + params[3] - y) * w

        def jacobian(params, x, y):
            A, a, b, _ = params[0], params[1], params[2], params[3]
            J = np.zeros([len(params), len(x)])
            J[0] = ((np.exp(a * (x - b)) - 1) / (np.exp(a * (x - b)) + 1)) * w
            J[1] = (A * (x - b) * (2.0 * np.exp(a * (x - b))) / ((np.exp(a * (x - b)) + 1) ** 2)) * w
            J[2] = (A * (-a) * (2.0 * np.exp(a * (x - b))) / ((np.exp(a * (x - b)) + 1) ** 2)) * w
            J[3] = w
            return np.transpose(J)

        train_x, train_y, w = [], [], []
        for i in range(len(training_weights)):
            train_x.append(training_weights[i][current_dim])
            train_y.append(training_deltas[i][current_dim])
            diff = np.abs(training_next_perfs[i] - current_eval)
            dist = np.linalg.norm(diff / np.abs(current_eval))
            w.append(np.exp(-((dist / sigma) ** 2) / 2.0))
        train_x, train_y, w = np.array(train_x), np.array(train_y), np.array(w)
        A_upperbound = np.clip(np.max(train_y) - np.min(train_y), 1.0, 500.0)
        res_robust = least_squares(hyperbolic_model, np.ones(4), loss="soft_l1", f_scale=self.f_scale, args=(train_x, train_y),
                                   jac=jacobian, bounds=([0, 0.1, -5.0, -500.0], [A_upperbound, 20.0, 5.0, 500.0]))
        return f(weight_candidate[current_dim], *res_robust.x)

    def predict_next_evaluation(self, weight_candidate: np.ndarray, policy_eval: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
        """``pgmorl.py:150-202``: (delta prediction, predicted next evaluation); the neighbourhood doubles until it holds four
        samples with distinct next evaluations."""
        neighbor_weights, neighbor_deltas, neighbor_next_perf = [], [], []
        current_sigma = self.sigma / 2.0
        current_neighb_threshold = self.neighborhood_threshold / 2.0
        while len(neighbor_weights) < 4:
            current_sigma *= 2.0
            current_neighb_threshold *= 2.0
            if current_neighb_threshold == np.inf or current_sigma == np.inf:
                raise ValueError("Cannot find at least 4 neighbors by enlarging the neighborhood.")
            for previous_perf, next_perf, neighb_w in zip(self.previous_performance, self.next_performance, self.used_weight):
                if np.all(np.abs(previous_perf - policy_eval) < current_neighb_threshold * np.abs(policy_eval)) and tuple(
                        next_perf) not in list(map(tuple, neighbor_next_perf)):
                    neighbor_weights.append(neighb_w)
                    neighbor_deltas.append(next_perf - previous_perf)
                    neighbor_next_perf.append(next_perf)
        delta_predictions = np.array([
            self._build_model_and_predict(neighbor_weights, neighbor_deltas, neighbor_next_perf, obj_num, policy_eval,
                                          weight_candidate, current_sigma)
            for obj_num in range(weight_candidate.size)])
        return delta_predictions, delta_predictions + policy_eval


def generate_weights(delta_weight: float, dimensions: int = 2) -> np.ndarray:
    """``pgmorl.py:205-223``: the float32 weight vectors on the grid of spacing ``delta_weight`` that sum to 1."""
    possible_weights = np.arange(0.0, 1.0 + delta_weight, delta_weight, dtype=np.float32)
    weight_combinations = np.array(list(product(possible_weights, repeat=dimensions)), dtype=np.float32)
    return weight_combinations[np.isclose(weight_combinations.sum(axis=1), 1.0)]


class _PerformanceBuffer:
    """What the 2-D and the 3-D buffer share (``pgmorl.py:247-296``): bins of at most ``max_size`` individuals in ascending order
    of the centred evaluation's norm; a full bin drops its first (worst) entry."""

    max_size: int
    origin: np.ndarray
    bins: list
    bins_evals: list

    @property
    def evaluations(self) -> List[np.ndarray]:
        return [e for l in self.bins_evals for e in l]

    @property
    def individuals(self) -> list:
        return [i for l in self.bins for i in l]

    def _center(self, evaluation):
        return np.clip(evaluation + self.origin, 0.0, float("inf"))      # objectives must be positive

    def _insert(self, buffer_id: int, candidate, evaluation: np.ndarray, norm_eval):
        inserted = False
        for idx, existing_eval in enumerate(self.bins_evals[buffer_id]):
            if norm_eval < np.linalg.norm(self._center(existing_eval)):
                self.bins[buffer_id].insert(idx, deepcopy(candidate))
                self.bins_evals[buffer_id].insert(idx, evaluation)
                inserted = True
                break
        if not inserted:
            self.bins[buffer_id].append(deepcopy(candidate))
            self.bins_evals[buffer_id].append(evaluation)
        if len(self.bins[buffer_id]) > self.max_size:
            self.bins[buffer_id].pop(0)
            self.bins_evals[buffer_id].pop(0)


class PerformanceBuffer2d(_PerformanceBuffer):
    """``pgmorl.py:226-296``: the population, ``num_bins`` angular bins over the positive quadrant."""

    def __init__(self, num_bins: int, max_size: int, origin: np.ndarray):
        self.num_bins, self.max_size, self.origin = num_bins, max_size, -origin
        self.dtheta = np.pi / 2.0 / self.num_bins
        self.bins = [[] for _ in range(self.num_bins)]
        self.bins_evals = [[] for _ in range(self.num_bins)]

    def add(self, candidate, evaluation: np.ndarray):
        centered_eval = self._center(evaluation)
        norm_eval = np.linalg.norm(centered_eval)
        theta = np.arccos(np.clip(centered_eval[1] / (norm_eval + 1e-3), -1.0, 1.0))
        buffer_id = int(theta // self.dtheta)
        if buffer_id < 0 or buffer_id >= self.num_bins:
            return
        self._insert(buffer_id, candidate, evaluation, norm_eval)


class PerformanceBuffer3d(_PerformanceBuffer):
    """``pgmorl.py:299-368``: bins around the unit vectors of ``generate_weights(1 / (num_bins - 1), 3)``."""

    def __init__(self, num_bins: int, max_size: int, origin: np.ndarray):
        self.max_size, self.origin = max_size, -origin
        self.pbuffer_vec = generate_weights(1.0 / (num_bins - 1), 3)
        for i in range(len(self.pbuffer_vec)):
            self.pbuffer_vec[i] = self.pbuffer_vec[i] / np.linalg.norm(self.pbuffer_vec[i])
        self.num_bins = len(self.pbuffer_vec)
        self.bins = [[] for _ in range(self.num_bins)]
        self.bins_evals = [[] for _ in range(self.num_bins)]

    def add(self, candidate, evaluation: np.ndarray):
        centered_eval = self._center(evaluation)
        norm_eval = np.linalg.norm(centered_eval)
        max_dot, buffer_id = -np.inf, -1
        for i in range(self.num_bins):
            dot = np.dot(self.pbuffer_vec[i], centered_eval)
            if dot > max_dot:
                max_dot, buffer_id = dot, i
        self._insert(buffer_id, candidate, evaluation, norm_eval)


def select_tasks(predictor: PerformancePredictor, population_eval: List[np.ndarray], candidate_weights: np.ndarray,
                 current_front: List[np.ndarray], n_tasks: int, ref_point: np.ndarray, sparsity_coef: float,
                 hv: Callable = hypervolume):
    """The selection loop of ``__task_weight_selection`` (``pgmorl.py:657-719``) on evaluations alone: for each of ``n_tasks``
    workers the (individual, weight) pair whose predicted evaluation adds most hypervolume + ``sparsity_coef`` * sparsity to the
    front; pairs already taken are skipped and each choice's prediction joins the front.  Returns a list of
    (index into ``population_eval``, weight, predicted evaluation)."""
    current_front = list(current_front)
    selected_tasks, out = [], []
    for _ in range(n_tasks):
        max_improv, best = float("-inf"), None
        for ci, last_candidate_eval in enumerate(population_eval):
            weights = [w for w in candidate_weights if (tuple(last_candidate_eval), tuple(w)) not in selected_tasks]
            predicted_evals = [predictor.predict_next_evaluation(w, last_candidate_eval)[1] for w in weights]
            mixture = [hv(ref_point, current_front + [p]) + sparsity_coef * sparsity(current_front + [p]) for p in predicted_evals]
            k = int(np.argmax(np.array(mixture)))
            if max_improv < np.max(np.array(mixture)):
                max_improv = np.max(np.array(mixture))
                best = (ci, weights[k], predicted_evals[k])
        selected_tasks.append((tuple(population_eval[best[0]]), tuple(best[1])))
        current_front.append(best[2])
        out.append(best)
    return out


# -- the population on the device ----------------------------------------------------------------------------------------------
def _ptrs(tensors):
    return (C.c_void_p * len(tensors))(*[None if t is None else t.data_ptr() for t in tensors])


def _handles(agents):
    return (C.c_void_p * len(agents))(*[a._ctx.value for a in agents])


def population_forward(lib: NativeLib, agents: List[MOPPO], obs: th.Tensor, eps: Optional[th.Tensor]):
    """``get_action_and_value`` (``eps`` [P][rows][A]) or ``get_value`` (``eps=None``) of every agent on its ``obs[i]``
    ([P][rows][D], device) in one launch.  Returns (action [P][rows][A], logprob [P][rows], value [P][rows][R]) device tensors."""
    D, A, R = agents[0]._dims
    P, rows = len(agents), obs.shape[1]
    dev = obs.device
    value = th.empty(P, rows, R, dtype=th.float32, device=dev)
    action = logprob = None
    if eps is not None:
        action = th.empty(P, rows, A, dtype=th.float32, device=dev)
        logprob = th.empty(P, rows, dtype=th.float32, device=dev)
    lib.check_device(obs, value, eps, *[a.params for a in agents])
    each = lambda t: None if t is None else _ptrs([t[i] for i in range(P)])  # noqa: E731
    lib.check(lib.lib.morl_ppo_forward_pop(P, _handles(agents), _ptrs([a.params for a in agents]), each(obs), each(eps), rows,
                                           int(eps is None), each(action), each(logprob), each(value), lib.stream_of(value)))
    return action, logprob, value


def population_update_n(lib: NativeLib, agents: List[MOPPO], idx: List[np.ndarray]) -> List[th.Tensor]:
    """``idx[i]`` [n][M]: n minibatch steps of every agent, one launch per step for all of them.  Returns each agent's statistics
    [n][8] (device) and advances its Adam step count."""
    a0 = agents[0]
    n, M = idx[0].shape
    P = len(agents)
    idx_dev = th.from_numpy(np.ascontiguousarray(np.stack(idx), dtype=np.int32)).to(a0.device)
    stats = th.empty(P, n, len(STAT_NAMES), dtype=th.float32, device=a0.device)
    lib.check_device(idx_dev, stats, *[t for a in agents for t in (a.params, a.exp_avg, a.exp_avg_sq)])
    lib.check(lib.lib.morl_ppo_update_n_pop(
        P, _handles(agents), _ptrs([a.params for a in agents]), _ptrs([a.exp_avg for a in agents]),
        _ptrs([a.exp_avg_sq for a in agents]), n, _ptrs([idx_dev[i] for i in range(P)]), M,
        (C.c_double * P)(*[float(a.optimizer.param_groups[0]["lr"]) for a in agents]),
        (C.c_int * P)(*[int(a.optimizer.steps) for a in agents]), float(a0.clip_coef), float(a0.ent_coef), float(a0.vf_coef),
        float(a0.max_grad_norm), int(bool(a0.clip_vloss)), int(bool(a0.norm_adv)), _ptrs([stats[i] for i in range(P)]),
        lib.stream_of(stats)))
    for a in agents:
        a.optimizer.steps += n
    return [stats[i] for i in range(P)]


_SHARED = ("steps_per_iteration", "num_envs", "num_minibatches", "update_epochs", "clip_coef", "ent_coef", "vf_coef", "max_grad_norm",
           "clip_vloss", "norm_adv", "target_kl", "gamma", "gae_lambda", "gae", "_dims")


def train_population(lib: NativeLib, agents: List[MOPPO], current_iteration: int, max_iterations: int, global_step: int) -> int:
    """One iteration of every agent -- ``MOPPO.train()`` of each, in agent order, to the bit -- with the device work of all agents
    in shared launches.  ``global_step`` is the count before agent 0's rollout; returns the count after the last agent's."""
    a0 = agents[0]
    for a in agents[1:]:
        if any(getattr(a, k) != getattr(a0, k) for k in _SHARED):
            raise ValueError("train_population: the agents of a population share their shapes and PPO hyper-parameters")
    if len({id(a.envs) for a in agents}) != len(agents):
        raise ValueError("train_population: every agent steps a vector env of its own")
    P, T, E = len(agents), a0.steps_per_iteration, a0.num_envs
    D, A, R = a0._dims
    dev = a0.device

    # -- rollouts in lock-step (MOPPO.train / _collect_samples) --------------------------------------------------------------
    next_obs = []
    for a in agents:
        a.global_step = global_step
        global_step += T * E
        obs, _ = a.envs.reset(seed=a.seed)
        next_obs.append(th.Tensor(obs))
        if a.anneal_lr:
            a.optimizer.param_groups[0]["lr"] = (1.0 - (current_iteration - 1.0) / max_iterations) * a.learning_rate
    noise = [[a._noise() for _ in range(T)] for a in agents]          # agent order, one draw per step: torch's stream as P train() calls
    obs = th.stack(next_obs).to(dev, th.float32).reshape(P, E, D).contiguous()
    done = th.zeros(P, E, device=dev)
    for t in range(T):
        eps = th.stack([noise[i][t] for i in range(P)]).to(dev, th.float32).contiguous()
        action, logprob, value = population_forward(lib, agents, obs, eps)
        action_host = action.cpu().numpy()                              # the one read of this vector step
        nobs, ndone = [], []
        for i, a in enumerate(agents):
            a.global_step += 1 * E
            o, reward, terminated, truncated, info = a.envs.step(action_host[i])
            reward = th.tensor(reward).to(dev).view(E, R)
            a.batch.add(obs[i], action[i], logprob[i], reward, done[i], value[i])
            nobs.append(th.Tensor(o))
            ndone.append(th.Tensor(terminated))
        obs = th.stack(nobs).to(dev, th.float32).reshape(P, E, D).contiguous()
        done = th.stack(ndone).to(dev)

    # -- advantages (MOPPO._compute_advantages): one get_value launch, the tables, one scan launch --------------------------
    _, _, next_value = population_forward(lib, agents, obs, None)
    next_done = done.to(th.float32).contiguous()
    weights = th.stack([a.weights.to(th.float32) for a in agents]).contiguous()
    returns = th.empty(P, T, E, R, dtype=th.float32, device=dev)
    advantages = th.empty(P, T, E, dtype=th.float32, device=dev)
    stream = lib.stream_of(returns)
    keep = []
    for a in agents:
        cols = [c.to(th.float32).contiguous() for c in a.batch.get_all()]
        lib.check_device(*cols)
        lib.check(lib.lib.morl_ppo_set_rollout(a._ctx, *[c.data_ptr() for c in cols], T, E, stream))
        keep.append(cols)
    each = lambda t: _ptrs([t[i] for i in range(P)])  # noqa: E731
    lib.check(lib.lib.morl_ppo_gae_pop(P, _handles(agents), each(next_value), each(next_done), each(weights), float(a0.gamma),
                                       float(a0.gae_lambda), int(bool(a0.gae)), each(returns), each(advantages), stream))
    for i, a in enumerate(agents):
        a.returns, a.advantages = returns[i], advantages[i]
        a._keep = (keep[i], next_value, next_done, weights)      # (alive until the launches on the stream have read them)

    update_population(lib, agents)
    return global_step


def update_population(lib: NativeLib, agents: List[MOPPO]):
    """``MOPPO.update()`` of every agent, in agent order, as population calls (see the module docstring)."""
    a0 = agents[0]
    if a0.target_kl is None:
        groups = []
        for a in agents:                                   # agent 0's epochs, then agent 1's: the generators' order of use
            b_inds, g = np.arange(a.batch_size), []
            for _ in range(a.update_epochs):
                by_size(g, epoch_steps(a.np_random, b_inds, a.minibatch_size))
            groups.append(g)
        stats = [[] for _ in agents]
        for k in range(len(groups[0])):
            for s, new in zip(stats, population_update_n(lib, agents, [np.stack(g[k]) for g in groups])):
                s.append(new)
        for a, s in zip(agents, stats):
            a.last_stats = s[0] if len(s) == 1 else th.cat(s)
        return
    if len({id(a.np_random) for a in agents}) != len(agents):
        for a in agents:                                   # a shared generator and a data-dependent number of draws per agent
            a.update()
        return
    kl = STAT_NAMES.index("approx_kl")
    b_inds = [np.arange(a.batch_size) for a in agents]
    stats = [[] for _ in agents]
    active = list(range(len(agents)))
    for _ in range(a0.update_epochs):
        groups = [by_size([], epoch_steps(agents[i].np_random, b_inds[i], agents[i].minibatch_size)) for i in active]
        act = [agents[i] for i in active]
        for k in range(len(groups[0])):
            for i, new in zip(active, population_update_n(lib, act, [np.stack(g[k]) for g in groups])):
                stats[i].append(new)
        last = th.stack([stats[i][-1][-1, kl] for i in active]).cpu().numpy()      # one read for the active learners
        active = [i for i, v in zip(active, last) if not float(v) > a0.target_kl]
        if not active:
            break
    for a, s in zip(agents, stats):
        a.last_stats = s[0] if len(s) == 1 else th.cat(s)


class PGMORL(MOAgent):
    """Prediction Guided Multi-Objective Reinforcement Learning (``pgmorl.py:371-819``): J. Xu, Y. Tian, P. Ma, D. Rus, S. Sueda,
    W. Matusik, "Prediction-Guided Multi-Objective Reinforcement Learning for Continuous Robot Control", ICML 2020.
    The post-processing phase is not implemented (as in the reference).  See the module docstring for ``make_envs``."""

    def __init__(self, make_envs: Callable, origin: np.ndarray, num_envs: int = 4, pop_size: int = 6, warmup_iterations: int = 80,
                 steps_per_iteration: int = 2048, evolutionary_iterations: int = 20, num_weight_candidates: int = 7,
                 num_performance_buffer: int = 100, performance_buffer_size: int = 2, min_weight: float = 0.0,
                 max_weight: float = 1.0, delta_weight: float = 0.2, sparsity_coef: float = -1.0, env=None, gamma: float = 0.995,
                 project_name: str = "MORL-baselines", experiment_name: str = "PGMORL", wandb_entity: Optional[str] = None,
                 seed: Optional[int] = None, log: bool = False, net_arch: List = [64, 64], num_minibatches: int = 32,
                 update_epochs: int = 10, learning_rate: float = 3e-4, anneal_lr: bool = False, clip_coef: float = 0.2,
                 ent_coef: float = 0.0, vf_coef: float = 0.5, clip_vloss: bool = True, max_grad_norm: float = 0.5,
                 norm_adv: bool = True, target_kl: Optional[float] = None, gae: bool = True, gae_lambda: float = 0.95,
                 device: Union[th.device, str] = "auto", group: Optional[str] = None, lib: Optional[NativeLib] = None):
        if log:
            raise NotImplementedError("PGMORL: W&B logging is not available here (log=True)")
        if env is not None:
            raise ValueError("Environments should be vectorized for PPO. You should provide make_envs instead.")
        super().__init__(None, device=device, seed=seed)
        self.device = th.device(self.device)
        self.lib = lib or load_library()
        self.make_envs, self.num_envs, self.pop_size = make_envs, num_envs, pop_size
        self.envs = [make_envs() for _ in range(pop_size)]
        e0 = self.envs[0]
        if any(e.num_envs != num_envs for e in self.envs):
            raise ValueError(f"PGMORL: make_envs() returned a vector env of {e0.num_envs} envs, num_envs is {num_envs}")
        space = lambda single, name: getattr(e0, single) if hasattr(e0, single) else getattr(e0, name)  # noqa: E731
        osp, asp = space("single_observation_space", "observation_space"), space("single_action_space", "action_space")
        rsp = e0.reward_space if hasattr(e0, "reward_space") else e0.unwrapped.reward_space
        assert not hasattr(asp, "n"), "only continuous action space is supported"
        self.env = e0
        self.observation_shape, self.observation_dim = tuple(osp.shape), osp.shape[0]
        self.action_space, self.action_shape, self.action_dim = asp, tuple(asp.shape), asp.shape[0]
        self.reward_dim = rsp.shape[0]
        self.gamma = gamma

        # EA parameters
        self.warmup_iterations, self.steps_per_iteration = warmup_iterations, steps_per_iteration
        self.evolutionary_iterations, self.num_weight_candidates = evolutionary_iterations, num_weight_candidates
        self.min_weight, self.max_weight, self.delta_weight, self.sparsity_coef = min_weight, max_weight, delta_weight, sparsity_coef
        self.num_performance_buffer, self.performance_buffer_size = num_performance_buffer, performance_buffer_size
        self.archive = ParetoArchive(lib=self.lib, device=self.device)
        if self.reward_dim == 2:
            self.population = PerformanceBuffer2d(self.num_performance_buffer, self.performance_buffer_size, origin)
        elif self.reward_dim == 3:
            self.population = PerformanceBuffer3d(self.num_performance_buffer, self.performance_buffer_size, origin)
        else:
            raise ValueError("Only 2D and 3D objectives are supported.")
        self.predictor = PerformancePredictor()

        # PPO parameters
        self.net_arch = net_arch
        self.batch_size = int(self.num_envs * self.steps_per_iteration)
        self.num_minibatches = num_minibatches
        self.minibatch_size = int(self.batch_size // self.num_minibatches)
        self.update_epochs, self.learning_rate, self.anneal_lr = update_epochs, learning_rate, anneal_lr
        self.clip_coef, self.vf_coef, self.ent_coef, self.max_grad_norm = clip_coef, vf_coef, ent_coef, max_grad_norm
        self.norm_adv, self.target_kl, self.clip_vloss, self.gae_lambda, self.gae = norm_adv, target_kl, clip_vloss, gae_lambda, gae
        self.log = log

        weights = generate_weights(self.delta_weight, self.reward_dim)
        if self.pop_size > len(weights):
            raise ValueError(f"PGMORL: pop_size {self.pop_size} exceeds the {len(weights)} weight vectors of delta_weight "
                             f"{self.delta_weight} in {self.reward_dim} objectives (one warm-up weight per agent)")
        self.networks = [MOPPONet(self.observation_shape, self.action_space.shape, self.reward_dim, self.net_arch)
                         for _ in range(self.pop_size)]
        self.agents = [
            MOPPO(i, self.networks[i], weights[i], self.envs[i], log=self.log, gamma=self.gamma, device=self.device, seed=self.seed,
                  steps_per_iteration=self.steps_per_iteration, num_minibatches=self.num_minibatches,
                  update_epochs=self.update_epochs, learning_rate=self.learning_rate, anneal_lr=self.anneal_lr,
                  clip_coef=self.clip_coef, ent_coef=self.ent_coef, vf_coef=self.vf_coef, clip_vloss=self.clip_vloss,
                  max_grad_norm=self.max_grad_norm, norm_adv=self.norm_adv, target_kl=self.target_kl, gae=self.gae,
                  gae_lambda=self.gae_lambda, rng=self.np_random, lib=self.lib)
            for i in range(self.pop_size)]

    def get_config(self) -> dict:
        return {
            "env_id": getattr(getattr(self.env, "spec", None), "id", type(self.env).__name__), "num_envs": self.num_envs,
            "pop_size": self.pop_size, "warmup_iterations": self.warmup_iterations,
            "evolutionary_iterations": self.evolutionary_iterations, "num_weight_candidates": self.num_weight_candidates,
            "num_performance_buffer": self.num_performance_buffer, "performance_buffer_size": self.performance_buffer_size,
            "min_weight": self.min_weight, "max_weight": self.max_weight, "delta_weight": self.delta_weight,
            "sparsity_coef": self.sparsity_coef, "gamma": self.gamma, "seed": self.seed, "net_arch": self.net_arch,
            "batch_size": self.batch_size, "minibatch_size": self.minibatch_size, "update_epochs": self.update_epochs,
            "learning_rate": self.learning_rate, "anneal_lr": self.anneal_lr, "clip_coef": self.clip_coef, "vf_coef": self.vf_coef,
            "ent_coef": self.ent_coef, "max_grad_norm": self.max_grad_norm, "norm_adv": self.norm_adv, "target_kl": self.target_kl,
            "clip_vloss": self.clip_vloss, "gae": self.gae, "gae_lambda": self.gae_lambda,
        }

    def _train_all_agents(self, iteration: int, max_iterations: int):
        """``__train_all_agents`` (``pgmorl.py:612-616``) with the agents' device work in shared launches."""
        self.global_step = train_population(self.lib, self.agents, iteration, max_iterations, self.global_step)

    def _eval_all_agents(self, eval_env, evaluations_before_train: List[np.ndarray], ref_point: np.ndarray,
                         known_pareto_front: Optional[List[np.ndarray]] = None, add_to_prediction: bool = True):
        """``pgmorl.py:618-638``: evaluates every agent and stores it in the population buffer and the Pareto archive."""
        for i, agent in enumerate(self.agents):
            _, _, _, discounted_reward = agent.policy_eval(eval_env, weights=agent.np_weights, log=self.log)
            self.population.add(agent, discounted_reward)
            self.archive.add(agent, discounted_reward)
            if add_to_prediction:
                self.predictor.add(agent.weights.detach().cpu().numpy(), evaluations_before_train[i], discounted_reward)
            evaluations_before_train[i] = discounted_reward

    def _task_weight_selection(self, ref_point: np.ndarray):
        """``pgmorl.py:652-731``: the agents and weights of the next generation."""
        candidate_weights = generate_weights(self.delta_weight / 2.0, self.reward_dim)
        self.np_random.shuffle(candidate_weights)
        population, population_eval = self.population.individuals, self.population.evaluations
        hv = lambda ref, pts: hypervolume(ref, pts, lib=self.lib, device=self.device)  # noqa: E731
        tasks = select_tasks(self.predictor, population_eval, candidate_weights, deepcopy(self.archive.evaluations),
                             len(self.agents), ref_point, self.sparsity_coef, hv=hv)
        self.selected_tasks = [(ci, np.array(w)) for ci, w, _ in tasks]
        for i, (ci, weight, _) in enumerate(tasks):
            copied_agent = deepcopy(population[ci])
            copied_agent.global_step = self.agents[i].global_step
            copied_agent.id = i
            copied_agent.change_weights(deepcopy(weight))
            copied_agent.envs = self.envs[i]              # worker slot i steps env copy i (see the module docstring)
            self.agents[i] = copied_agent

    def train(self, total_timesteps: int, eval_env, ref_point: np.ndarray, known_pareto_front: Optional[List[np.ndarray]] = None,
              num_eval_weights_for_eval: int = 50):
        """``pgmorl.py:733-819``."""
        self.num_eval_weights_for_eval = num_eval_weights_for_eval
        # 1 iteration is a full batch for each agent -> steps_per_iteration * num_envs * pop_size timesteps
        max_iterations = total_timesteps // self.steps_per_iteration // self.num_envs // self.pop_size
        iteration = 0
        current_evaluations = [np.zeros(self.reward_dim) for _ in range(len(self.agents))]
        self._eval_all_agents(eval_env, current_evaluations, ref_point, known_pareto_front, add_to_prediction=False)
        self.start_time = time.time()

        for _ in range(1, self.warmup_iterations + 1):
            self._train_all_agents(iteration, max_iterations)
            iteration += 1
        self._eval_all_agents(eval_env, current_evaluations, ref_point, known_pareto_front)

        max_iterations = max(max_iterations, self.warmup_iterations + self.evolutionary_iterations)
        while iteration < max_iterations:
            self._task_weight_selection(ref_point)
            for _ in range(self.evolutionary_iterations):
                self._train_all_agents(iteration, max_iterations)
                iteration += 1
            self._eval_all_agents(eval_env, current_evaluations, ref_point, known_pareto_front)
        for e in self.envs:
            if hasattr(e, "close"):
                e.close()
