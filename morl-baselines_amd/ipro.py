"""IPRO on the HIP library (``multi_policy/ipro/ipro.py`` and ``outer_loop.py``): the iterated Pareto-referent outer loop over
``NLMOPPO``, for three or more objectives.

The outer loop is box bookkeeping on a few hundred points and stays numpy, line for line the reference's.  What it computes in bulk
is hypervolume: ``compute_hvis`` scores up to 50 lower points per call, each the hypervolume of the SAME base set (``pf`` and
``completed``) plus one point, against the same reference point (``ideal``).  Here that is ONE ``morl_ipro_hvis`` call
(``csrc/ipro_kernels.h``): one upload of base, candidates and reference, two launches whatever the sizes are, one read-back.  The
bits of a score depend on (base, candidate, ideal) only, so equal candidates tie exactly and the reference's
``np.argsort(hvis)[::-1]`` -- an unstable sort whose tie order no kernel can restate -- runs on the host on the kernel's values.
``discarded_hv`` is the same entry with no candidates; ``dominated_hv`` and ``hv`` are ``hypervolume_device``; the final
``filter_pareto_dominated`` of the point-set updates is ``morl_pareto_mask``.  ``estimate_error`` stays in numpy.

The hypervolumes are pinned to the float64 oracle, not to pymoo (which the reference imports at module level and this package
does not need): ``compute_hypervolume``'s frame -- a point counts only if the reference point dominates it, no normalisation -- is
restated from pymoo's documented behaviour.

Not here: ``IPRO2D`` (two-objective box lists on ``sortedcontainers``, no array work) and populations of learners.  W&B calls exist
only behind ``log=True``.
"""
from __future__ import annotations

import time
from dataclasses import dataclass
from functools import partial
from typing import Any, Callable, Iterable, List, Optional, Tuple, Union

import numpy as np
import torch as th

from . import pareto
from . import performance_indicators as pi
from .api import MOAgent
from .native import NativeLib, load_library
from .nl_mo_ppo import NLMOPPO


@dataclass
class Subproblem:
    """``outer_loop.py:29-35``."""

    referent: np.ndarray
    nadir: np.ndarray
    ideal: np.ndarray


class Box:
    """``ipro/box.py:6-25``: what the outer loop reads of the bounding box."""

    def __init__(self, point1, point2):
        self.bounds = np.array([point1, point2])
        self.nadir = np.min(self.bounds, axis=0)
        self.ideal = np.max(self.bounds, axis=0)
        self.volume = abs(np.prod(self.ideal - self.nadir))


Subsolution = Tuple[Subproblem, np.ndarray, Any]
IPROCallback = Callable[[int, float, float, float, float, float], Any]


def linear_scalarization(batch: th.Tensor, weights: th.Tensor) -> th.Tensor:
    """``outer_loop.py:42-44``."""
    return th.sum(batch * weights, dim=-1)


def aasf(batch, referent, nadir, ideal, aug=0.0, scale=100):
    """``outer_loop.py:47-51``: the augmented achievement scalarising function."""
    pos_vec = ideal - nadir
    frac_improvement = scale * (batch - referent) / pos_vec
    return th.min(frac_improvement, dim=-1)[0] + aug * th.mean(frac_improvement, dim=-1)


def strict_pareto_dominates(a, b) -> np.bool_:
    """``common/pareto.py:17-21``."""
    return np.all(np.array(a) > np.array(b))


def pareto_dominates(a, b) -> np.bool_:
    """``common/pareto.py:10-14``."""
    a, b = np.array(a), np.array(b)
    return np.all(a >= b) and np.any(a > b)


def batched_strict_pareto_dominates(p1, p2) -> np.ndarray:
    """``common/pareto.py:24-26``."""
    return np.all(p1 > p2, axis=-1)


def batched_pareto_dominates(p1, p2) -> np.ndarray:
    """``common/pareto.py:29-31``."""
    return np.logical_and(np.all(p1 >= p2, axis=-1), np.any(p1 > p2, axis=-1))


class OuterLoop(MOAgent):
    """``outer_loop.py:54-460``.  Not meant to be used directly."""

    def __init__(self, env, method: str = "IPRO", direction: str = "maximize", offset: float = 1, tolerance: float = 1e-1,
                 max_iterations: Optional[int] = None, aug: float = 0.1, scale: float = 100, reset_agent: bool = False,
                 log: bool = False, experiment_name: Optional[str] = None, project_name: Optional[str] = None,
                 wandb_entity: Optional[str] = None, wandb_mode: str = "online", seed: Optional[int] = None,
                 lib: Optional[NativeLib] = None, **kwargs):
        MOAgent.__init__(self, env, device=kwargs["device"], seed=seed)
        self.lib = lib or load_library()
        self.device = th.device(self.device)
        # where the outer loop's own kernels run: the learner's device
        self._hv_device = self.device if self.lib.is_device_build else th.device("cpu")
        self.env = env
        self.dim = self.env.reward_space.shape[0]
        self.nadir, self.ideal = None, None
        self.agent = self._make_learner(env, seed, **kwargs)

        self.method = method
        self.direction = direction
        self.ref_point = None
        self.offset = offset
        self.tolerance = tolerance
        self.max_iterations = max_iterations if max_iterations is not None else np.inf
        self.aug = aug
        self.scale = scale
        self.reset_agent = reset_agent

        self.sign = 1 if direction == "maximize" else -1
        self.bounding_box = None
        self.ideal = None
        self.nadir = None
        self.pf = np.empty((0, self.dim))
        self.robust_points = np.empty((0, self.dim))
        self.completed = np.empty((0, self.dim))

        self.hv = 0
        self.total_hv = 0
        self.dominated_hv = 0
        self.discarded_hv = 0
        self.coverage = 0
        self.error = np.inf
        self.replay_triggered = 0

        self.track = log
        self.run_id = None
        self.exp_name = experiment_name
        self.wandb_project_name = project_name
        self.wandb_entity = wandb_entity
        self.wandb_mode = wandb_mode

        self.seed = seed

    def _make_learner(self, env, seed, **kwargs):
        """``outer_loop.py:101``: the learner every oracle query trains."""
        return NLMOPPO(0, env, seed=seed, lib=self.lib, **kwargs)

    def reset(self):
        """``outer_loop.py:138-153``."""
        self.bounding_box = None
        self.ideal = None
        self.nadir = None
        self.pf = np.empty((0, self.dim))
        self.robust_points = np.empty((0, self.dim))
        self.completed = np.empty((0, self.dim))

        self.hv = 0
        self.total_hv = 0
        self.dominated_hv = 0
        self.discarded_hv = 0
        self.coverage = 0
        self.error = np.inf
        self.replay_triggered = 0

    def get_config(self) -> dict:
        """``outer_loop.py:155-164``."""
        return {
            "method": self.method,
            "env_id": self.env.spec.id,
            "dimensions": self.dim,
            "tolerance": self.tolerance,
            "max_iterations": self.max_iterations,
            "seed": self.seed,
        }

    def setup(self) -> float:
        """``outer_loop.py:166-184``."""
        if self.track:
            import wandb
            super().setup_wandb(project_name=self.wandb_project_name, experiment_name=self.exp_name, entity=self.wandb_entity,
                                mode=self.wandb_mode)
            wandb.define_metric("iteration")
            for name in ("hypervolume", "dominated_hv", "discarded_hv", "coverage", "error"):
                wandb.define_metric(f"outer/{name}", step_metric="iteration")
            self.run_id = wandb.run.id
        return time.time()

    def get_pareto_set(self, subsolutions: List[Subsolution]) -> List[Tuple[np.ndarray, Any]]:
        """``outer_loop.py:186-192``."""
        pareto_set = []
        for subsolution in subsolutions:
            if np.any(np.all(np.isclose(subsolution[1], self.pf), axis=1)):
                pareto_set.append((self.sign * subsolution[1], subsolution[2]))
        return pareto_set

    def get_pareto_front(self) -> np.ndarray:
        """``outer_loop.py:194-196``."""
        return self.pf * self.sign

    def _filter_pareto_dominated(self, candidates: np.ndarray) -> np.ndarray:
        """``common/pareto.py:60-73`` on ``morl_pareto_mask``: bit-exact, the first of equal rows kept."""
        return pareto.filter_pareto_dominated(candidates, lib=self.lib, device=self._hv_device)

    def finish(self, start_time: float, iteration: int):
        """``outer_loop.py:198-209``."""
        self.pf = self._filter_pareto_dominated(np.vstack((self.pf, self.robust_points)))
        self.dominated_hv = self.compute_hypervolume(-self.sign * self.pf, -self.sign * self.nadir)
        self.hv = self.compute_hypervolume(-self.sign * self.pf, -self.sign * self.ref_point)
        self.log_iteration(iteration + 1)

        end_str = f"Iterations {iteration + 1} | Time {time.time() - start_time:.2f} | "
        end_str += f"HV {self.hv:.2f} | PF size {len(self.pf)} |"
        print(end_str)

        self.close_wandb()

    def close_wandb(self):
        """``outer_loop.py:211-217``."""
        if self.track:
            import wandb
            pf_table = wandb.Table(data=self.pf, columns=[f"obj_{i}" for i in range(self.dim)])
            wandb.log({"pareto_front": pf_table})
            wandb.run.summary["PF_size"] = len(self.pf)
            wandb.finish()

    def log_iteration(self, iteration: int, subproblem: Optional[Subproblem] = None, pareto_point: Optional[np.ndarray] = None):
        """``outer_loop.py:219-248``."""
        if self.track:
            import wandb
            wandb.log({"outer/hypervolume": self.hv, "outer/dominated_hv": self.dominated_hv,
                       "outer/discarded_hv": self.discarded_hv, "outer/coverage": self.coverage, "outer/error": self.error,
                       "iteration": iteration})
            if subproblem is not None:
                wandb.run.summary[f"referent_{iteration}"] = self.sign * subproblem.referent
                wandb.run.summary[f"ideal_{iteration}"] = self.sign * subproblem.ideal
                wandb.run.summary[f"pareto_point_{iteration}"] = self.sign * pareto_point
            wandb.run.summary["hypervolume"] = self.hv
            wandb.run.summary["PF_size"] = len(self.pf)
            wandb.run.summary["replay_triggered"] = self.replay_triggered

    def compute_hypervolume(self, points: np.ndarray, ref: np.ndarray) -> float:
        """``outer_loop.py:250-256``: pymoo's minimisation frame -- the volume of the union of the boxes [p, ref] over the points
        ``ref`` dominates; the rest are dropped.  ``hypervolume_device`` maximises, so both sides are negated."""
        points, ref = np.asarray(points, dtype=np.float64), np.asarray(ref, dtype=np.float64)
        points = points[batched_pareto_dominates(ref, points)]
        if points.size == 0:
            return 0
        flat = th.from_numpy(np.concatenate([-points.reshape(-1), -ref])).to(self._hv_device)
        return float(pi.hypervolume_device(flat[points.size:], flat[:points.size].view(points.shape), self.lib).item())

    def init_phase(self, extrema=None, deterministic: bool = False, eval_env=None) -> Tuple[List[Subsolution], bool]:
        raise NotImplementedError

    def is_done(self, step: int) -> bool:
        """``outer_loop.py:267-269``."""
        return 1 - self.coverage <= self.tolerance or step >= self.max_iterations

    def decompose_problem(self, iteration: int, method: str = "first") -> Subproblem:
        raise NotImplementedError

    def update_found(self, subproblem: Subproblem, vec: np.ndarray):
        raise NotImplementedError

    def update_not_found(self, subproblem: Subproblem, vec: np.ndarray):
        raise NotImplementedError

    def update_excluded_volume(self):
        raise NotImplementedError

    def estimate_error(self):
        raise NotImplementedError

    def get_iterable_for_replay(self) -> Iterable[Any]:
        raise NotImplementedError

    def maybe_add_solution(self, subproblem: Subproblem, vec: np.ndarray, item: Any):
        raise NotImplementedError

    def maybe_add_completed(self, subproblem: Subproblem, vec: np.ndarray, item: Any):
        raise NotImplementedError

    def replay(self, vec: np.ndarray, sol: Any, iter_pairs: List[Subsolution]) -> List[Subsolution]:
        """``outer_loop.py:313-356``: rebuild the sets after an answer that shows an earlier one was not optimal."""
        replay_triggered = self.replay_triggered
        nadir, ideal = self.nadir, self.ideal
        self.reset()
        self.replay_triggered = replay_triggered + 1
        self.init_phase(extrema=(nadir, ideal), eval_env=None)
        idx = 0
        new_subsolutions = []

        for old_subproblem, old_vec, old_sol in iter_pairs:  # replay the points that were added correctly
            idx += 1
            if strict_pareto_dominates(old_vec, old_subproblem.referent):
                if strict_pareto_dominates(vec, old_vec):
                    self.update_found(old_subproblem, vec)
                    new_subsolutions.append((old_subproblem, vec, sol))
                    break
                else:
                    self.update_found(old_subproblem, old_vec)
                    new_subsolutions.append((old_subproblem, old_vec, old_sol))
            else:
                if strict_pareto_dominates(vec, old_subproblem.referent):
                    self.update_found(old_subproblem, vec)
                    new_subsolutions.append((old_subproblem, vec, sol))
                    break
                else:
                    self.update_not_found(old_subproblem, old_vec)
                    new_subsolutions.append((old_subproblem, old_vec, old_vec))        # (sic: outer_loop.py:340)

        for old_subproblem, old_vec, old_sol in iter_pairs[idx:]:  # the remaining points: can they still be added?
            items = self.get_iterable_for_replay()
            if strict_pareto_dominates(old_vec, old_subproblem.referent):
                maybe_add = self.maybe_add_solution
            else:
                maybe_add = self.maybe_add_completed
            for item in items:
                res = maybe_add(old_subproblem, old_vec, item)
                if res:
                    new_subsolutions.append((res, old_vec, old_sol))
                    break

        return new_subsolutions

    def eval(self, obs, disc_vec_return, pref=None):
        """``outer_loop.py:358-360``."""
        return self.agent.eval(obs, disc_vec_return, pref=pref)

    def linear_train(self, weight_vec: np.ndarray, deterministic: bool, eval_env) -> Tuple[np.ndarray, Any]:
        """``outer_loop.py:362-375``."""
        if self.reset_agent:
            self.agent.reset_agent(pref_dim=self.dim)

        # (NLMOPPO evaluates u_func and its gradient on the host, on the mean value it read back: the tensors bound into the
        # utility are host tensors; the preference goes to the learner's device inside train())
        weights = th.tensor(weight_vec, dtype=th.float32)
        u_func = partial(linear_scalarization, weights=weights)
        vec = self.agent.train(eval_env, u_func, pref=weights, deterministic=deterministic)
        return vec, self.agent.agent

    def oracle_train(self, referent: np.ndarray, deterministic: bool, eval_env) -> Tuple[np.ndarray, Any]:
        """``outer_loop.py:377-394``."""
        if self.reset_agent:
            self.agent.reset_agent(pref_dim=self.dim)

        referent = self.sign * th.tensor(referent, dtype=th.float32)
        nadir = self.sign * th.tensor(self.nadir, dtype=th.float32)
        ideal = self.sign * th.tensor(self.ideal, dtype=th.float32)

        u_func = partial(aasf, referent=referent, nadir=nadir, ideal=ideal, aug=self.aug, scale=self.scale)
        vec = self.agent.train(eval_env, u_func, pref=referent, deterministic=deterministic)
        vec *= self.sign
        return vec, self.agent.agent

    def train(self, eval_env, ref_point: np.ndarray, deterministic: bool = False, extrema=None,
              callback: Optional[IPROCallback] = None, verbose: bool = True) -> List[Tuple[np.ndarray, Any]]:
        """``outer_loop.py:396-460``."""
        self.ref_point = ref_point
        say = print if verbose else (lambda *a, **k: None)

        start = self.setup()
        linear_subsolutions, done = self.init_phase(extrema=extrema, deterministic=deterministic, eval_env=eval_env)
        iteration = 0

        if done:
            say("The problem is solved in the initial phase.")
            pareto_set = self.get_pareto_set(linear_subsolutions)
            return pareto_set

        self.log_iteration(iteration)
        subsolutions = []

        while not self.is_done(iteration):
            begin_loop = time.time()
            say(f"Iter {iteration} - Covered {self.coverage:.5f}% - Error {self.error:.5f}")

            subproblem = self.decompose_problem(iteration)
            vec, sol = self.oracle_train(referent=subproblem.referent, deterministic=deterministic, eval_env=eval_env)

            if strict_pareto_dominates(vec, subproblem.referent):
                if np.any(batched_strict_pareto_dominates(vec, np.vstack((self.pf, self.completed)))):
                    subsolutions = self.replay(vec, sol, subsolutions)
                else:
                    self.update_found(subproblem, vec)
                    subsolutions.append((subproblem, vec, sol))
            else:
                if np.any(batched_strict_pareto_dominates(vec, self.completed)):
                    subsolutions = self.replay(vec, sol, subsolutions)
                else:
                    self.update_not_found(subproblem, vec)
                    subsolutions.append((subproblem, vec, sol))

            self.update_excluded_volume()
            self.estimate_error()
            self.coverage = (self.dominated_hv + self.discarded_hv) / self.total_hv
            self.hv = self.compute_hypervolume(-self.sign * self.pf, -self.sign * self.ref_point)

            iteration += 1
            self.log_iteration(iteration, subproblem=subproblem, pareto_point=vec)

            if callback is not None:
                callback(iteration, self.hv, self.dominated_hv, self.discarded_hv, self.coverage, self.error)

            duration = time.time() - begin_loop
            say(f"Ref {self.sign * subproblem.referent} - Found {self.sign * vec} - Time {duration:.2f}s")
            say("---------------------")

        self.finish(start, iteration)
        pareto_set = self.get_pareto_set(linear_subsolutions + subsolutions)
        return pareto_set


class IPRO(OuterLoop):
    """``ipro.py:23-333``: the constructor's signature and defaults are the reference's, plus ``lib``."""

    def __init__(self, env, direction: str = "maximize", offset: float = 1, tolerance: float = 1e-6,
                 max_iterations: Optional[int] = None, update_freq: int = 1, reset_agent: bool = False, aug: float = 0.1,
                 scale: float = 100, iter_total_timesteps: int = 500000, learning_rate: float = 2.5e-4, num_steps: int = 128,
                 anneal_lr: bool = True, gamma: float = 0.99, gae_lambda: float = 0.95, num_minibatches: int = 4,
                 update_epochs: int = 4, norm_adv: bool = True, clip_coef: float = 0.2, clip_vloss: bool = True,
                 ent_coef: float = 0.01, vf_coef: float = 0.5, max_grad_norm: float = 0.5, target_kl: Optional[float] = None,
                 mc_k: int = 32, device: Union[th.device, str] = "auto", log: bool = False, experiment_name: Optional[str] = "IPRO",
                 project_name: str = "MORL-Baselines", wandb_entity: Optional[str] = None, wandb_mode: str = "online",
                 seed: int = 1, rng: Optional[np.random.Generator] = None, lib: Optional[NativeLib] = None):
        super().__init__(env, method="IPRO", direction=direction, offset=offset, tolerance=tolerance, max_iterations=max_iterations,
                         reset_agent=reset_agent, aug=aug, scale=scale, total_timesteps=iter_total_timesteps,
                         learning_rate=learning_rate, num_steps=num_steps, anneal_lr=anneal_lr, gamma=gamma, gae_lambda=gae_lambda,
                         num_minibatches=num_minibatches, update_epochs=update_epochs, norm_adv=norm_adv, clip_coef=clip_coef,
                         clip_vloss=clip_vloss, ent_coef=ent_coef, vf_coef=vf_coef, max_grad_norm=max_grad_norm, target_kl=target_kl,
                         mc_k=mc_k, device=device, log=log, experiment_name=experiment_name, project_name=project_name,
                         wandb_entity=wandb_entity, wandb_mode=wandb_mode, seed=seed, rng=rng, lib=lib)
        self.update_freq = update_freq
        self.lower_points = []
        self.upper_points = []

        self.rng = rng if rng is not None else np.random.default_rng(seed)

    def reset(self):
        """``ipro.py:140-144``."""
        self.lower_points = []
        self.upper_points = []
        super().reset()

    def init_phase(self, extrema=None, deterministic: bool = False, eval_env=None):
        """``ipro.py:146-210``: the bounding box from 2 d linear problems, then the first lower and upper sets."""
        subsolutions = []

        if extrema is None:
            nadir = np.zeros(self.dim)
            ideal = np.zeros(self.dim)
            pf = []
            weight_vecs = np.eye(self.dim)

            for i, weight_vec in enumerate(weight_vecs):
                ideal_vec, ideal_sol = self.linear_train(weight_vec=weight_vec, deterministic=deterministic, eval_env=eval_env)
                print(f"Found solution {ideal_vec} for weight vector {weight_vec}")
                nadir_vec, _ = self.linear_train(weight_vec=-1 * weight_vec, deterministic=deterministic, eval_env=eval_env)
                ideal_vec *= self.sign
                nadir_vec *= self.sign
                ideal[i] = ideal_vec[i]
                nadir[i] = nadir_vec[i]
                pf.append(ideal_vec)
                subsolutions.append((weight_vec, ideal_vec, ideal_sol))

            self.pf = self._filter_pareto_dominated(np.array(pf))
            nadir = nadir - self.offset  # every Pareto optimal point strictly dominates the nadir
            ideal = ideal + self.offset
            self.nadir = np.copy(nadir)
            self.ideal = np.copy(ideal)

            if len(self.pf) == 1:  # the Pareto front is the ideal
                return subsolutions, True
        else:
            self.nadir, self.ideal = extrema

        self.ref_point = np.copy(self.nadir) if self.ref_point is None else np.array(self.ref_point)
        self.hv = self.compute_hypervolume(-self.sign * self.pf, -self.sign * self.ref_point)

        self.bounding_box = Box(self.nadir, self.ideal)
        self.total_hv = self.bounding_box.volume
        self.lower_points = np.array([self.nadir])

        for point in self.pf:  # initialise the lower points
            self.update_lower_points(np.array(point))

        self.upper_points = np.array([self.ideal])  # initialise the upper points
        self.error = max(self.ideal - self.nadir)
        self.compute_hvis()

        return subsolutions, False

    def compute_hvis(self, num=50):
        """``ipro.py:212-226``: the hypervolume improvements of (at most ``num``) lower points, and the lower points in their
        descending order.  The draw is made every time -- also when every point is scored -- as the reference makes it; the scores
        of the drawn points, in the drawn order, are one ``morl_ipro_hvis`` call."""
        discarded_extrema = np.vstack((self.pf, self.completed))
        hvis = np.zeros(len(self.lower_points))

        ids = self.rng.choice(len(self.lower_points), min(num, len(self.lower_points)), replace=False)
        scores = pi.ipro_hvis(self.ideal, discarded_extrema, self.lower_points[ids], lib=self.lib, device=self._hv_device)
        hvis[ids] = scores[:len(ids)]  # the difference to the base is not needed: it is the same for every point

        sorted_args = np.argsort(hvis)[::-1]
        self.lower_points = self.lower_points[sorted_args]

    def max_hypervolume_improvement(self):
        """``ipro.py:228-231``."""
        self.compute_hvis()
        return self.lower_points[0]

    def estimate_error(self):
        """``ipro.py:233-241``: numpy -- a max-min-max over a few thousand by a few tens of rows."""
        if len(self.upper_points) == 0:
            error = 0
        else:
            pf = np.array(list(self.pf))
            diffs = self.upper_points[:, None, :] - pf[None, :, :]
            error = np.max(np.min(np.max(diffs, axis=2), axis=1))
        self.error = error

    def update_upper_points(self, vec):
        """``ipro.py:243-253``."""
        strict_dominates = batched_strict_pareto_dominates(self.upper_points, vec)
        to_keep = self.upper_points[strict_dominates == 0]
        shifted = np.stack([self.upper_points[strict_dominates == 1]] * self.dim)
        shifted[range(self.dim), :, range(self.dim)] = np.expand_dims(vec, -1)
        shifted = shifted.reshape(-1, self.dim)
        shifted = shifted[np.all(shifted > self.nadir, axis=-1)]

        new_upper_points = np.vstack((to_keep, shifted))
        self.upper_points = self._filter_pareto_dominated(new_upper_points)

    def update_lower_points(self, vec):
        """``ipro.py:255-265``."""
        strict_dominates = batched_strict_pareto_dominates(vec, self.lower_points)
        to_keep = self.lower_points[strict_dominates == 0]
        shifted = np.stack([self.lower_points[strict_dominates == 1]] * self.dim)
        shifted[range(self.dim), :, range(self.dim)] = np.expand_dims(vec, -1)
        shifted = shifted.reshape(-1, self.dim)
        shifted = shifted[np.all(self.ideal > shifted, axis=-1)]

        new_lower_points = np.vstack((to_keep, shifted))
        self.lower_points = -self._filter_pareto_dominated(-new_lower_points)

    def select_referent(self, method="random"):
        """``ipro.py:267-274``."""
        if method == "random":
            return self.lower_points[self.rng.integers(0, len(self.lower_points))]
        if method == "first":
            return self.lower_points[0]
        else:
            raise ValueError(f"Unknown method {method}")

    def get_iterable_for_replay(self):
        """``ipro.py:276-278``."""
        return np.copy(self.lower_points)

    def maybe_add_solution(self, subproblem: Subproblem, point: np.ndarray, lower: np.ndarray):
        """``ipro.py:280-292``."""
        if strict_pareto_dominates(point, lower):
            new_subproblem = Subproblem(referent=lower, nadir=self.nadir, ideal=self.ideal)
            self.update_found(new_subproblem, point)
            return new_subproblem
        else:
            return False

    def maybe_add_completed(self, subproblem: Subproblem, point: np.ndarray, lower: np.ndarray):
        """``ipro.py:294-306``."""
        if pareto_dominates(lower, subproblem.referent):
            new_subproblem = Subproblem(referent=lower, nadir=self.nadir, ideal=self.ideal)
            self.update_not_found(new_subproblem, point)
            return new_subproblem
        else:
            return False

    def update_found(self, subproblem, vec):
        """``ipro.py:308-312``."""
        self.pf = np.vstack((self.pf, vec))
        self.update_lower_points(vec)
        self.update_upper_points(vec)

    def update_not_found(self, subproblem, vec):
        """``ipro.py:314-320``."""
        self.completed = np.vstack((self.completed, subproblem.referent))
        self.lower_points = self.lower_points[np.any(self.lower_points != subproblem.referent, axis=1)]
        self.update_upper_points(subproblem.referent)
        if strict_pareto_dominates(vec, self.nadir):
            self.robust_points = np.vstack((self.robust_points, vec))

    def decompose_problem(self, iteration, method="first"):
        """``ipro.py:322-328``."""
        if iteration % self.update_freq == 0:
            self.compute_hvis()
        referent = self.select_referent(method=method)
        subproblem = Subproblem(referent=referent, nadir=self.nadir, ideal=self.ideal)
        return subproblem

    def update_excluded_volume(self):
        """``ipro.py:330-333``: ``discarded_hv`` is ``morl_ipro_hvis`` with no candidates."""
        self.dominated_hv = self.compute_hypervolume(-self.pf, -self.nadir)
        self.discarded_hv = float(pi.ipro_hvis(self.ideal, np.vstack((self.pf, self.completed)), np.empty((0, self.dim)),
                                               lib=self.lib, device=self._hv_device)[0])
