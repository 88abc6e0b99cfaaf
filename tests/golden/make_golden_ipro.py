"""IPRO fixtures from the UNMODIFIED reference classes (multi_policy/ipro/ipro.py, outer_loop.py), CPU:

* ipro_hvis_<case>.npz    inputs of one morl_ipro_hvis call and the float64 oracle's values (through the reference's own
                          compute_hypervolume, whose pymoo indicator is the oracle on negated inputs here)
* ipro_points_<case>.npz  update_lower_points / update_upper_points of the reference, before and after
* ipro_trace_r3/_r4.npz   whole train() runs with the scripted oracle of ipro_cases.py, the state after every iteration
* ipro_utility.npz        aasf and linear_scalarization on float32 inputs

pymoo is absent: the process adds ``pymoo.config.Config`` and a ``pymoo.indicators.hv.Hypervolume`` over
oracle/metrics_oracle.hypervolume to the stubs, and replaces the learner in ``outer_loop`` by a dummy (it is not under test here).
A trace is refused -- and the next seed tried -- when two sampled scores of a compute_hvis call are closer than 1e-9 relative (exact
ties included) or a strict comparison of a returned vector is decided by less than 1e-9: the recorded order then survives the
kernel's 1e-12.  tests/ipro_oracle.py is checked against every recorded value on the way.  Arrays only, fixed zip timestamps.

    PYTHONDONTWRITEBYTECODE=1 python -B tests/golden/make_golden_ipro.py
"""
from __future__ import annotations

import contextlib
import io
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

import metrics_oracle as mo  # noqa: E402
import ref_harness as rh  # noqa: E402
import ipro_cases as ic  # noqa: E402
import ipro_oracle as io_  # noqa: E402
from make_golden_pcn import save_npz  # noqa: E402

GAP = 1e-9


class Refused(Exception):
    pass


def import_reference():
    rh.install_stubs()
    cfg = types.ModuleType("pymoo.config")
    cfg.Config = type("Config", (), {"warnings": {}})
    sys.modules["pymoo.config"] = cfg

    class Hypervolume:           # pymoo's minimisation indicator without pf / ideal / nadir: no normalisation
        def __init__(self, ref_point):
            self.ref_point = np.asarray(ref_point, dtype=np.float64)

        def __call__(self, points):
            return mo.hypervolume(-self.ref_point, list(-np.asarray(points, dtype=np.float64)))

    sys.modules["pymoo.indicators.hv"].Hypervolume = Hypervolume
    from morl_baselines.multi_policy.ipro import ipro, outer_loop
    outer_loop.NLMOPPO = lambda *a, **k: types.SimpleNamespace(agent=None)
    return ipro, outer_loop


def bare(ipro, R, **kw):
    return ipro.IPRO(rh.FakeEnv(obs_dim=4, n_actions=3, reward_dim=R), device="cpu", log=False, **kw)


def hvis_case(ipro, c):
    base, cand, ref = ic.hvis_inputs(c)
    ag = bare(ipro, c.R)
    want = [ag.compute_hypervolume(np.vstack((base, p)), ref) for p in cand] + [ag.compute_hypervolume(base, ref)]
    want = np.asarray(want, dtype=np.float64)
    mine = np.asarray([io_.oracle_hv(np.vstack((base, p)), ref) for p in cand] + [io_.oracle_hv(base, ref)], dtype=np.float64)
    assert np.array_equal(want, mine), c.name
    if c.exact:
        assert np.array_equal(want, np.round(want)) and len(np.unique(want)) > 3, "an integer grid with distinct integer volumes"
    save_npz(os.path.join(HERE, f"ipro_hvis_{c.name}.npz"), dict(base=base, cand=cand, ref=ref, want=want))
    print(f"ipro_hvis_{c.name}: n {c.n} R {c.R} K {c.K}, base {want[-1]:.6g}, distinct {len(np.unique(want))}")


def points_case(ipro, name):
    which, pts, vec, nadir, ideal = ic.points_inputs(name)
    R = len(vec)
    ag = bare(ipro, R)
    ag.nadir, ag.ideal = nadir.copy(), ideal.copy()
    lo = io_.Loop(R, None, None)
    lo.nadir, lo.ideal = nadir.copy(), ideal.copy()
    if which == "lower":
        ag.lower_points = pts.copy()
        ag.update_lower_points(vec.copy())
        after = ag.lower_points
        lo.lower_points = pts.copy()
        lo.update_lower_points(vec.copy())
        mine = lo.lower_points
    else:
        ag.upper_points = pts.copy()
        ag.update_upper_points(vec.copy())
        after = ag.upper_points
        lo.upper_points = pts.copy()
        lo.update_upper_points(vec.copy())
        mine = lo.upper_points
    after = np.asarray(after, dtype=np.float64).reshape(-1, R)
    assert np.array_equal(after, np.asarray(mine).reshape(-1, R)), name
    save_npz(os.path.join(HERE, f"ipro_points_{name}.npz"),
             dict(lower=np.asarray(which == "lower"), before=pts, vec=vec, nadir=nadir, ideal=ideal, after=after))
    print(f"ipro_points_{name}: {which} {len(pts)} -> {len(after)} rows")


def check_gap(values, what):
    v = np.sort(np.asarray(values, dtype=np.float64))
    if len(v) > 1:
        gap = np.min(np.diff(v) / np.maximum(np.abs(v[1:]), 1e-300))
        if gap < GAP:
            raise Refused(f"{what}: two scores {gap:.3g} apart")
        return gap
    return np.inf


def check_margin(vec, rows, what):
    d = np.abs(np.asarray(rows, dtype=np.float64).reshape(-1, len(vec)) - vec)
    if np.any((d > 0) & (d < GAP)):
        raise Refused(f"{what}: a strict comparison decided by less than {GAP}")


def trace_case(ipro, name, write=True):
    T = ic.TRACES[name]
    R, table = T["R"], ic.trace_table(T)
    for seed in range(T["seed"], T["seed"] + 12):
        try:
            out = trace_run(ipro, T, R, table, seed)
        except Refused as e:
            print(f"ipro_trace_{name}: seed {seed} refused ({e})")
            continue
        if write:
            save_npz(os.path.join(HERE, f"ipro_trace_{name}.npz"), out)
        print(f"ipro_trace_{name}: seed {seed}, {int(out['iterations'])} iterations, replays {int(out['replay_triggered'][-1])}, "
              f"lower points up to {int(out['lower_points_rows'].max())}, smallest score gap {float(out['min_gap']):.3g}")
        return
    raise RuntimeError(f"ipro_trace_{name}: no seed passed")


def trace_run(ipro, T, R, table, seed):
    ag = bare(ipro, R, direction=T["direction"], max_iterations=T["iterations"], seed=seed)
    script = ic.Scripted(table, T["weak_every"], aug=ag.aug, scale=ag.scale)
    gaps = []

    def linear_train(weight_vec, deterministic, eval_env):
        return script.linear(weight_vec), None

    def oracle_train(referent, deterministic, eval_env):
        vec = script.oracle(referent, ag.nadir, ag.ideal, ag.sign)
        check_margin(vec, np.vstack((referent[None], ag.pf, ag.completed)), "oracle answer")
        return vec, None

    compute_hvis = ag.compute_hvis

    def compute_hvis_checked(num=50):
        # the scores the reference is about to sort: recomputed here from the same generator state
        state = ag.rng.bit_generator.state
        ids = ag.rng.choice(len(ag.lower_points), min(num, len(ag.lower_points)), replace=False)
        ag.rng.bit_generator.state = state
        base = np.vstack((ag.pf, ag.completed))
        gaps.append(check_gap([ag.compute_hypervolume(np.vstack((base, ag.lower_points[i])), ag.ideal) for i in ids], "compute_hvis"))
        return compute_hvis(num)

    log = []

    def callback(iteration, hv, dominated_hv, discarded_hv, coverage, error):
        log.append(dict(pf=ag.pf.copy(), completed=ag.completed.copy(), robust_points=ag.robust_points.copy(),
                        lower_points=np.asarray(ag.lower_points).copy().reshape(-1, R),
                        upper_points=np.asarray(ag.upper_points).copy().reshape(-1, R), hv=hv, dominated_hv=dominated_hv,
                        discarded_hv=discarded_hv, coverage=coverage, error=error, replay_triggered=ag.replay_triggered))

    referents, vecs = [], []
    decompose = ag.decompose_problem

    def decompose_logged(iteration, method="first"):
        sub = decompose(iteration, method)
        referents.append(sub.referent.copy())
        return sub

    oracle_plain = oracle_train

    def oracle_logged(referent, deterministic, eval_env):
        vec, sol = oracle_plain(referent, deterministic, eval_env)
        vecs.append(vec.copy())
        return vec, sol

    ag.linear_train, ag.oracle_train, ag.compute_hvis, ag.decompose_problem = linear_train, oracle_logged, compute_hvis_checked, decompose_logged
    with contextlib.redirect_stdout(io.StringIO()):
        pareto_set = ag.train(None, None, callback=callback)
    # the restatement, with the oracle's hypervolume
    script2 = ic.Scripted(table, T["weak_every"], aug=ag.aug, scale=ag.scale)
    lo = io_.Loop(R, script2.linear, script2.oracle, direction=T["direction"], max_iterations=T["iterations"], seed=seed)
    mine = lo.train(None)
    assert len(lo.log) == len(log) + 1 and len(mine) == len(pareto_set)
    for a, b in zip(mine, pareto_set):
        assert np.array_equal(a, b[0])
    out = {"seed": np.asarray(seed), "iterations": np.asarray(len(log)), "referents": np.stack(referents), "vecs": np.stack(vecs),
           "pareto_set": np.stack([p[0] for p in pareto_set]).reshape(-1, R), "nadir": ag.nadir, "ideal": ag.ideal,
           "min_gap": np.asarray(min(gaps))}
    final = dict(pf=ag.pf, completed=ag.completed, robust_points=ag.robust_points, lower_points=np.asarray(ag.lower_points).reshape(-1, R),
                 upper_points=np.asarray(ag.upper_points).reshape(-1, R), hv=ag.hv, dominated_hv=ag.dominated_hv,
                 discarded_hv=ag.discarded_hv, coverage=ag.coverage, error=ag.error, replay_triggered=ag.replay_triggered)
    for k in io_.STATE:
        rows = [rec[k] for rec in log + [final]]
        out[k] = np.concatenate(rows).reshape(-1, R)
        out[f"{k}_rows"] = np.asarray([len(r) for r in rows], dtype=np.int64)
        for it, (r, m) in enumerate(zip(rows, lo.log)):
            assert np.array_equal(r, m[k]), (k, it)
    for k in io_.SCALARS:
        out[k] = np.asarray([rec[k] for rec in log + [final]], dtype=np.float64)
        mine_k = np.asarray([m[k] for m in lo.log])
        assert np.allclose(out[k], mine_k, rtol=1e-12, atol=0.0), k
    assert np.array_equal(out["referents"], np.stack([m["referent"] for m in lo.log[:-1]]))
    assert np.array_equal(out["vecs"], np.stack([m["vec"] for m in lo.log[:-1]]))
    assert ag.rng.bit_generator.state == lo.rng.bit_generator.state
    return out


def utility_case(outer_loop):
    batch, referent, nadir, ideal, weights = ic.utility_inputs()
    T = th.tensor
    out = dict(batch=batch, referent=referent, nadir=nadir, ideal=ideal, weights=weights)
    for sign in (1, -1):
        for aug in (0.0, 0.1):
            got = outer_loop.aasf(T(batch), sign * T(referent), sign * T(nadir), sign * T(ideal), aug=aug, scale=100)
            out[f"aasf_sign{sign}_aug{aug}"] = got.numpy()
            mine = io_.aasf(batch, sign * referent, sign * nadir, sign * ideal, aug=np.float32(aug), scale=np.float32(100))
            assert np.allclose(mine, got.numpy(), rtol=1e-5, atol=1e-5)
    out["linear"] = outer_loop.linear_scalarization(T(batch), T(weights)).numpy()
    save_npz(os.path.join(HERE, "ipro_utility.npz"), out)
    print("ipro_utility: float32", out["linear"].shape)


def main():
    if not rh.reference_available():
        raise RuntimeError("reference tree not found")
    ipro, outer_loop = import_reference()
    only = sys.argv[1:] or ["hvis", "points", "trace", "utility"]
    if "hvis" in only:
        for c in ic.HVIS_CASES:
            hvis_case(ipro, c)
    if "points" in only:
        for name in ic.POINT_CASES:
            points_case(ipro, name)
    if "trace" in only:
        for name in ic.TRACES:
            trace_case(ipro, name)
    if "utility" in only:
        utility_case(outer_loop)


if __name__ == "__main__":
    main()
