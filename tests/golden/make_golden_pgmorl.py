"""PGMORL fixtures from the UNMODIFIED reference module (multi_policy/pgmorl/pgmorl.py), CPU:

* pgmorl_weights.npz      generate_weights for delta 0.2 / 0.25 / 0.5 and 2 / 3 objectives
* pgmorl_buffer2d.npz     40 PerformanceBuffer2d.add calls (evaluations outside the bins, equal norms, overflowing bins): the bins'
* pgmorl_buffer3d.npz     contents and order after every add; the same for PerformanceBuffer3d
* pgmorl_predictor.npz    a predictor memory of 12 samples, (weight, evaluation) queries and predict_next_evaluation's answers,
                          and a memory of three distinct samples on which it raises ValueError
* pgmorl_selection.npz    __task_weight_selection from a recorded state: population evaluations, predictor memory, archive front,
                          shuffled candidate weights -> the selected (individual, weight) pairs
* pgmorl_trace.npz        a seeded PGMORL.train(): pop 4, two warm-up iterations and one evolutionary generation of one iteration
                          on tests/pgmorl_env.py

Stand-ins.  ``ref_harness.install_stubs`` supplies gymnasium / mo_gymnasium / wandb / pymoo; on top of it, as in
make_golden_ppo.py, ``mo_gym.make`` returns the single-env twin ``pgmorl_env.PGEvalEnv``, ``make_env`` returns nothing and
``MOSyncVectorEnv`` returns a ``pgmorl_env.PGVecEnv``.  pymoo is absent, so the name ``hypervolume`` in the reference module is bound
to ``oracle/metrics_oracle.hypervolume``, the exact CPU restatement tests/test_metrics.py holds the device kernel against.  The
selection fixtures are 2-objective, where the hypervolume is a sum of rectangles; hypervolume parity with pymoo stays unpinned.

The restatement in morl-baselines_amd/pgmorl.py is checked against every recorded value on the way, and the largest difference of
the predictor's answers is stored in the fixture (``restatement_max_rel_diff``).  A seed is refused when the selected tasks change
with every evaluation perturbed by 1e-4 relative (ten times the project's 1e-5 contract): the recorded decisions do not hang on
rounding.

    PYTHONDONTWRITEBYTECODE=1 python -B tests/golden/make_golden_pgmorl.py
"""
from __future__ import annotations

import copy
import os
import sys
import types

import numpy as np
import torch as th

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, ROOT)

import ref_harness as rh  # noqa: E402
import metrics_oracle  # noqa: E402
import pgmorl_cases as gc  # noqa: E402
from make_golden_pcn import save_npz  # noqa: E402
from make_golden_ppo import flat, import_reference as import_reference_ppo  # noqa: E402


def import_reference():
    import_reference_ppo()                      # the stubs, and the names mo_ppo.py needs at import
    import pgmorl_env                           # (after the stubs: its spaces then subclass the stand-in gymnasium's Box)
    from morl_baselines.multi_policy.pgmorl import pgmorl as ref
    ref.hypervolume = metrics_oracle.hypervolume
    ref.mo_gym.make = lambda env_id, **k: pgmorl_env.PGEvalEnv(**gc.TRACE["env"])
    ref.make_env = lambda *a, **k: None
    ref.mo_gym.wrappers.vector.MOSyncVectorEnv = lambda envs: pgmorl_env.PGVecEnv(**gc.TRACE["env"])
    ref.print = lambda *a, **k: None            # (the predictor prints its neighbourhood at every call)
    return ref, pgmorl_env


def ours():
    import simlib
    import morl_baselines_amd.pgmorl as mine
    return mine, simlib.load_sim()


# ---------------------------------------------------------------------------------------------------------------------
def weights_case(ref, mine):
    out = {}
    for delta in gc.WEIGHT_DELTAS:
        for dim in (2, 3):
            w = ref.generate_weights(delta, dim)
            assert np.array_equal(w, mine.generate_weights(delta, dim)) and w.dtype == np.float32
            out[gc.weights_key(delta, dim)] = w
    save_npz(os.path.join(HERE, "pgmorl_weights.npz"), out)
    print("pgmorl_weights:", {k: v.shape for k, v in out.items()})


def bins_state(buf, width):
    ids = [(b, c) for b, l in enumerate(buf.bins) for c in l]
    a = -np.ones((width, 2), dtype=np.int64)
    a[:len(ids)] = np.asarray(ids, dtype=np.int64).reshape(-1, 2)
    return a


def buffer_case(ref, mine, dim):
    B = gc.BUFFER[dim]
    evals = gc.buffer_evals(dim)
    cls, mcls = (ref.PerformanceBuffer2d, mine.PerformanceBuffer2d) if dim == 2 else (ref.PerformanceBuffer3d, mine.PerformanceBuffer3d)
    buf, mbuf = cls(B["num_bins"], B["max_size"], np.asarray(B["origin"])), mcls(B["num_bins"], B["max_size"], np.asarray(B["origin"]))
    width = buf.num_bins * B["max_size"]
    states, dropped, replaced = [], 0, 0
    for i, e in enumerate(evals):
        before = len(buf.individuals)
        buf.add(i, e)
        mbuf.add(i, e)
        states.append(bins_state(buf, width))
        assert np.array_equal(states[-1], bins_state(mbuf, width)), f"restatement differs after add {i}"
        assert all(np.array_equal(a, b) for a, b in zip(buf.evaluations, mbuf.evaluations))
        if len(buf.individuals) == before and i not in buf.individuals:
            dropped += 1                        # outside the bins, or the worst of a full bin
        if len(buf.individuals) == before and i in buf.individuals:
            replaced += 1                       # a full bin took it and dropped its worst
    assert dropped > 0 and replaced > 0, "the sequence must hold rejected evaluations and overflowing bins"
    out = dict(evals=evals, states=np.stack(states), num_bins=np.asarray(buf.num_bins))
    save_npz(os.path.join(HERE, f"pgmorl_buffer{dim}d.npz"), out)
    print(f"pgmorl_buffer{dim}d: {len(evals)} adds, {len(buf.individuals)} kept at the end, {dropped} not kept, {replaced} replaced the worst "
          f"of a full bin")


def fill_predictor(p, mem):
    for w, a, b in zip(mem["weights"], mem["before"], mem["after"]):
        p.add(w, a, b)
    return p


def predictor_case(ref, mine):
    mem, queries = gc.predictor_memory(gc.PREDICTOR["seed"]), gc.predictor_queries(gc.PREDICTOR["seed"])
    p, mp = fill_predictor(ref.PerformancePredictor(), mem), fill_predictor(mine.PerformancePredictor(), mem)
    deltas, nexts, worst = [], [], 0.0
    for w, e in zip(queries["weights"], queries["evals"]):
        d, n = p.predict_next_evaluation(w, e)
        md, mn = mp.predict_next_evaluation(w, e)
        worst = max(worst, float(np.max(np.abs(md - d) / np.abs(d))), float(np.max(np.abs(mn - n) / np.abs(n))))
        deltas.append(d)
        nexts.append(n)
    few = {k: v[:3] for k, v in mem.items()}
    for cls in (ref.PerformancePredictor, mine.PerformancePredictor):
        try:
            fill_predictor(cls(), few).predict_next_evaluation(queries["weights"][0], queries["evals"][0])
            raise AssertionError("three distinct samples must not be enough")
        except ValueError as err:
            assert "at least 4 neighbors" in str(err)
    out = dict(mem_weights=mem["weights"], mem_before=mem["before"], mem_after=mem["after"], q_weights=queries["weights"],
               q_evals=queries["evals"], deltas=np.stack(deltas), nexts=np.stack(nexts), restatement_max_rel_diff=np.asarray(worst))
    save_npz(os.path.join(HERE, "pgmorl_predictor.npz"), out)
    print(f"pgmorl_predictor: {len(deltas)} queries, restatement max relative difference {worst:.3e}")


class Individual:
    def __init__(self, tag):
        self.tag, self.global_step, self.id, self.w = tag, 0, -1, None

    def change_weights(self, w):
        self.w = np.array(w)


def reference_selection(ref, state, n_tasks, ref_point, delta_weight, rng_seed, sparsity_coef=-1.0):
    """The reference's __task_weight_selection on a bare instance holding ``state``; returns [(individual index, weight)]."""
    obj = object.__new__(ref.PGMORL)
    obj.delta_weight, obj.reward_dim, obj.sparsity_coef, obj.log, obj.global_step = delta_weight, 2, sparsity_coef, False, 0
    obj.np_random = np.random.default_rng(rng_seed)
    obj.archive = types.SimpleNamespace(evaluations=[e for e in state["front"]])
    obj.population = types.SimpleNamespace(individuals=[Individual(i) for i in range(len(state["pop_evals"]))],
                                           evaluations=[e for e in state["pop_evals"]])
    obj.predictor = fill_predictor(ref.PerformancePredictor(), dict(weights=state["mem_weights"], before=state["mem_before"],
                                                                    after=state["mem_after"]))
    obj.agents = [Individual(-1) for _ in range(n_tasks)]
    obj._PGMORL__task_weight_selection(ref_point=ref_point)
    return [(a.tag, a.w) for a in obj.agents]


def restated_selection(mine, state, candidate_weights, n_tasks, ref_point, scale=None, sparsity_coef=-1.0):
    """``select_tasks`` of the restatement with the CPU hypervolume; ``scale``: every evaluation multiplied by (1 + scale * sign)."""
    s = {k: np.array(v, dtype=np.float64) for k, v in state.items()}
    if scale is not None:
        rng = np.random.default_rng(99)
        for k in ("pop_evals", "front", "mem_before", "mem_after"):
            s[k] = s[k] * (1.0 + scale * rng.choice([-1.0, 1.0], size=s[k].shape))
    pred = fill_predictor(mine.PerformancePredictor(), dict(weights=state["mem_weights"], before=s["mem_before"], after=s["mem_after"]))
    got = mine.select_tasks(pred, list(s["pop_evals"]), candidate_weights, list(s["front"]), n_tasks, ref_point, sparsity_coef,
                            hv=metrics_oracle.hypervolume)
    return [(ci, np.array(w)) for ci, w, _ in got]


def same_tasks(a, b):
    return len(a) == len(b) and all(x[0] == y[0] and np.array_equal(x[1], y[1]) for x, y in zip(a, b))


def robust(mine, state, cw, n_tasks, ref_point, want):
    return all(same_tasks(want, restated_selection(mine, state, cw, n_tasks, ref_point, scale=sc)) for sc in (None, 1e-4, -1e-4))


def selection_case(ref, mine):
    S = gc.SELECTION
    for seed in range(S["seed"], S["seed"] + 32):
        state = gc.selection_state(seed)
        picked = reference_selection(ref, state, S["n_tasks"], S["ref_point"], S["delta_weight"], seed)
        cw = gc.shuffled_candidates(mine.generate_weights, S["delta_weight"], seed)
        if robust(mine, state, cw, S["n_tasks"], S["ref_point"], picked) and len({p[0] for p in picked}) > 1:
            break
        print(f"pgmorl_selection: seed {seed} refused (the selection changes under a 1e-4 perturbation, or picks one individual)")
    else:
        raise AssertionError("no seed of 32 gives a robust selection")
    out = dict(state, candidate_weights=cw, picked_idx=np.asarray([p[0] for p in picked]), picked_w=np.stack([p[1] for p in picked]),
               seed=np.asarray(seed))
    save_npz(os.path.join(HERE, "pgmorl_selection.npz"), out)
    print(f"pgmorl_selection: seed {seed}, picked {[(p[0], p[1].tolist()) for p in picked]}")


def trace_case(ref, mine, pgmorl_env):
    Tr = gc.TRACE
    for seed in range(Tr["seed"], Tr["seed"] + 16):
        out = trace_attempt(ref, mine, pgmorl_env, seed)
        if out is not None:
            break
        print(f"pgmorl_trace: seed {seed} refused (the selection changes under a 1e-4 perturbation)")
    else:
        raise AssertionError("no seed of 16 gives a robust trace")
    save_npz(os.path.join(HERE, "pgmorl_trace.npz"), out)
    print(f"pgmorl_trace: seed {seed}, picked {out['picked_idx'].tolist()} {out['picked_w'].tolist()}, archive of {len(out['archive'])}, "
          f"global_step {int(out['global_step'])}")


def trace_attempt(ref, mine, pgmorl_env, seed):
    Tr = gc.TRACE
    gc.reseed(seed)
    algo = ref.PGMORL("pgmorl-fixture-v0", np.asarray(Tr["origin"]), seed=seed, log=False, device="cpu", **Tr["algo"])
    out = {"seed": np.asarray(seed)}
    for i, a in enumerate(algo.agents):
        out[f"init_{i}"] = flat(a.networks)
    rec = dict(it=0, evals=[], sel=None)
    train_all, eval_all, select = (algo._PGMORL__train_all_agents, algo._PGMORL__eval_all_agents, algo._PGMORL__task_weight_selection)

    def train_all_rec(iteration, max_iterations):
        train_all(iteration=iteration, max_iterations=max_iterations)
        rec["it"] += 1
        for i, a in enumerate(algo.agents):
            out[f"params_{rec['it']}_{i}"] = flat(a.networks)
            out[f"steps_{rec['it']}_{i}"] = np.asarray(a.global_step)

    def eval_all_rec(**kw):
        eval_all(**kw)
        rec["evals"].append(np.stack([np.asarray(e, dtype=np.float64) for e in kw["evaluations_before_train"]]))

    def select_rec(ref_point):
        state = dict(pop_evals=np.stack(algo.population.evaluations), front=np.stack(algo.archive.evaluations),
                     mem_weights=np.stack(algo.predictor.used_weight), mem_before=np.stack(algo.predictor.previous_performance),
                     mem_after=np.stack(algo.predictor.next_performance))
        rng_state = copy.deepcopy(algo.np_random.bit_generator.state)
        pop_params = [flat(ind.networks) for ind in algo.population.individuals]
        select(ref_point=ref_point)
        cw = mine.generate_weights(algo.delta_weight / 2.0, 2)
        rng = np.random.default_rng()
        rng.bit_generator.state = rng_state
        rng.shuffle(cw)
        picked = []
        for a in algo.agents:                  # a copy of a population member: found again by its parameters
            k = [j for j, p in enumerate(pop_params) if np.array_equal(p, flat(a.networks))]
            picked.append((k[0], a.weights.detach().cpu().numpy().copy()))
        rec["sel"] = (state, cw, picked, robust(mine, state, cw, len(algo.agents), ref_point, picked))

    algo._PGMORL__train_all_agents, algo._PGMORL__eval_all_agents, algo._PGMORL__task_weight_selection = (train_all_rec, eval_all_rec,
                                                                                                          select_rec)
    eval_env = pgmorl_env.PGEvalEnv(**Tr["env"])
    gc.reseed(seed + 1)
    algo.train(Tr["total_timesteps"], eval_env, np.asarray(Tr["ref_point"]))
    state, cw, picked, ok = rec["sel"]
    if not ok:
        return None
    assert rec["it"] == 3 and len(rec["evals"]) == 3
    out.update(evals=np.stack(rec["evals"]), candidate_weights=cw, picked_idx=np.asarray([p[0] for p in picked]),
               picked_w=np.stack([p[1] for p in picked]), archive=np.stack([np.asarray(e, dtype=np.float64) for e in algo.archive.evaluations]),
               population=np.stack([np.asarray(e, dtype=np.float64) for e in algo.population.evaluations]),
               global_step=np.asarray(algo.global_step), agent_global_step=np.asarray([a.global_step for a in algo.agents]),
               **{f"sel_{k}": v for k, v in state.items()})
    return out


def main():
    if not rh.reference_available():
        raise RuntimeError("reference tree not found")
    ref, pgmorl_env = import_reference()
    mine, _ = ours()
    th.set_num_threads(1)
    weights_case(ref, mine)
    buffer_case(ref, mine, 2)
    buffer_case(ref, mine, 3)
    predictor_case(ref, mine)
    selection_case(ref, mine)
    trace_case(ref, mine, pgmorl_env)


if __name__ == "__main__":
    main()
