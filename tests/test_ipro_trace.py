"""``IPRO.train()`` with the scripted Pareto oracle of tests/golden/ipro_cases.py.

* Against tests/golden/ipro_trace_r3 / _r4 (recorded from the reference): every set equal element for element and in order, the
  volumes, coverage and error to 1e-12 relative, ``replay_triggered`` and the final Pareto set equal.  The generator refused runs in
  which two scores of a ``compute_hvis`` call were closer than 1e-9, so the recorded order survives the kernel's 1e-12.
* At two objectives every run has exactly tied scores, so there is no recorded trace: the same run is compared live against the
  restatement (tests/ipro_oracle.py) with the package's own hypervolume functions plugged in -- both sides then sort the same bits.
  One three-objective run with ``direction="minimize"`` is compared in the same manner."""
import contextlib
import io

import numpy as np
import pytest

import ipro_cases as ic
import ipro_common as icm
import ipro_oracle as io_
from test_ipro_oracle_golden import compare_trace


@pytest.fixture(scope="module", params=icm.BACKENDS)
def be(request):
    return icm.backend(request.param)


def run(be, T, seed):
    """(agent, log, pareto_set): one scripted ``train()``, the state after every iteration and after ``finish``."""
    script = ic.Scripted(ic.trace_table(T), T["weak_every"])
    ag = icm.scripted_agent(be, script, T["R"], direction=T["direction"], max_iterations=T["iterations"], seed=seed)
    assert not ag.is_done(0), "is_done is evaluated before the first iteration: coverage 0, no iteration made"
    log, pending = [], {}
    decompose, oracle = ag.decompose_problem, ag.oracle_train

    def snapshot(referent, vec):
        rec = {k: np.array(getattr(ag, k), dtype=np.float64).reshape(-1, T["R"]) for k in io_.STATE}
        rec.update({k: float(getattr(ag, k)) for k in io_.SCALARS})
        rec["referent"], rec["vec"] = np.array(referent), np.array(vec)
        log.append(rec)

    def decompose_logged(iteration, method="first"):
        sub = decompose(iteration, method)
        pending["referent"] = sub.referent.copy()
        return sub

    def oracle_logged(referent, deterministic, eval_env):
        vec, sol = oracle(referent, deterministic, eval_env)
        pending["vec"] = vec.copy()
        return vec, sol

    ag.decompose_problem, ag.oracle_train = decompose_logged, oracle_logged
    with contextlib.redirect_stdout(io.StringIO()):
        pareto_set = ag.train(None, None, extrema=ic.trace_extrema(T), callback=lambda *a: snapshot(pending["referent"], pending["vec"]))
    snapshot(np.full(T["R"], np.nan), np.full(T["R"], np.nan))
    return ag, log, [p[0] for p in pareto_set]


@pytest.mark.parametrize("name", list(ic.TRACES))
def test_recorded_trace(be, name):
    T, g = ic.TRACES[name], icm.load(f"trace_{name}")
    ag, log, pareto_set = run(be, T, int(g["seed"].item()))
    compare_trace(g, log, pareto_set)
    assert np.array_equal(ag.ref_point, ag.nadir) and ag.ref_point is not ag.nadir, "ref_point=None falls back to a copy of the nadir"
    assert ag.reward_dim == T["R"] + 1 and ag.dim == T["R"], "MOAgent reads env.unwrapped.reward_space, the outer loop env.reward_space"
    assert ag.replay_triggered == g["replay_triggered"][-1] >= 1


@pytest.mark.parametrize("name", list(ic.LIVE))
def test_live_against_the_restatement_on_the_same_bits(be, name):
    from morl_baselines_amd import performance_indicators as pi
    lib, dev = be
    T = ic.LIVE[name]
    ag, log, pareto_set = run(be, T, T["seed"])

    def hv_plus(base, p, ref):
        cand = np.empty((0, len(ref))) if p is None else np.asarray(p)[None]
        return float(pi.ipro_hvis(ref, base, cand, lib=lib, device=dev)[0])

    script = ic.Scripted(ic.trace_table(T), T["weak_every"])
    lo = io_.Loop(T["R"], script.linear, script.oracle, hv=ag.compute_hypervolume, hv_plus=hv_plus, direction=T["direction"],
                  max_iterations=T["iterations"], seed=T["seed"])
    mine = lo.train(None, extrema=ic.trace_extrema(T))
    assert len(log) == len(lo.log) > 5
    for it, (a, b) in enumerate(zip(log, lo.log)):
        for k in io_.STATE + ("referent", "vec"):
            assert np.array_equal(a[k], b[k], equal_nan=True), (k, it)
        for k in io_.SCALARS:
            assert a[k] == b[k], (k, it, a[k], b[k])
    assert len(mine) == len(pareto_set) and all(np.array_equal(a, b) for a, b in zip(mine, pareto_set))
    assert ag.rng.bit_generator.state == lo.rng.bit_generator.state
    # and the volumes are the oracle's to 1e-12: the same restatement on the float64 oracle, while its order agrees
    lo64 = io_.Loop(T["R"], ic.Scripted(ic.trace_table(T), T["weak_every"]).linear, None, direction=T["direction"], seed=T["seed"])
    lo64.init_phase(extrema=ic.trace_extrema(T))
    first = io_.Loop(T["R"], script.linear, None, hv=ag.compute_hypervolume, hv_plus=hv_plus, direction=T["direction"], seed=T["seed"])
    first.init_phase(extrema=ic.trace_extrema(T))
    icm.close_rel("init_phase hv", first.hv, lo64.hv, rtol=1e-12)
    icm.close_rel("init_phase scores", np.sort(first.last_hvis), np.sort(lo64.last_hvis), rtol=1e-12)
