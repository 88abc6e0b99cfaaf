"""The ``IPRO`` class of the package: its point-set updates against the reference's recorded ones (exact), its utilities against the
recorded float32 values, the generator stream of ``compute_hvis``, its launch count, the constructor's defaults, and one
end-to-end run with the real ``NLMOPPO`` learner (a smoke run: a replay of the reference through six back-to-back trainings would
stack the learner's per-step tolerance past what the outer loop's strict comparisons allow)."""
import contextlib
import ctypes as C
import inspect
import io

import numpy as np
import pytest
import torch as th

import ipro_cases as ic
import ipro_common as icm
import ipro_oracle as io_
import nlppo_env


@pytest.fixture(scope="module", params=icm.BACKENDS)
def be(request):
    return icm.backend(request.param)


def bare(be, R, **kw):
    return icm.scripted_agent(be, ic.Scripted(ic.sphere_table(R, 8, 1), 0), R, **kw)


def test_constructor_signature_is_the_references():
    from morl_baselines_amd.ipro import IPRO, OuterLoop
    p = inspect.signature(IPRO.__init__).parameters
    want = dict(direction="maximize", offset=1, tolerance=1e-6, max_iterations=None, update_freq=1, reset_agent=False, aug=0.1,
                scale=100, iter_total_timesteps=500000, learning_rate=2.5e-4, num_steps=128, anneal_lr=True, gamma=0.99,
                gae_lambda=0.95, num_minibatches=4, update_epochs=4, norm_adv=True, clip_coef=0.2, clip_vloss=True, ent_coef=0.01,
                vf_coef=0.5, max_grad_norm=0.5, target_kl=None, mc_k=32, device="auto", log=False, experiment_name="IPRO",
                project_name="MORL-Baselines", wandb_entity=None, wandb_mode="online", seed=1, rng=None, lib=None)
    assert list(p)[:2] == ["self", "env"] and list(p)[2:] == list(want)
    assert {k: p[k].default for k in want} == want
    assert inspect.signature(OuterLoop.__init__).parameters["tolerance"].default == 1e-1
    import morl_baselines_amd
    assert morl_baselines_amd.IPRO is IPRO


@pytest.mark.parametrize("name", ic.POINT_CASES)
def test_point_set_updates(be, name):
    g = icm.load(f"points_{name}")
    R = g["before"].shape[1]
    ag = bare(be, R)
    ag.nadir, ag.ideal = g["nadir"].copy(), g["ideal"].copy()
    if bool(g["lower"].item()):
        ag.lower_points = g["before"].copy()
        ag.update_lower_points(g["vec"].copy())
        got = ag.lower_points
    else:
        ag.upper_points = g["before"].copy()
        ag.update_upper_points(g["vec"].copy())
        got = ag.upper_points
    assert np.array_equal(np.asarray(got).reshape(-1, R), g["after"]), "rows, and their order: kept first, then shifted objective-major"


def test_utilities(be):
    from morl_baselines_amd.ipro import aasf, linear_scalarization
    lib, dev = be
    g = icm.load("utility")
    T = lambda a: th.tensor(a).to(dev)  # noqa: E731

    def same(name, got, want):
        got = got.cpu().numpy()
        assert got.dtype == want.dtype == np.float32 and got.shape == want.shape
        if dev.type == "cpu":
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), name
        else:
            np.testing.assert_allclose(got, want, rtol=1e-6, atol=1e-6 * np.abs(want).max(), err_msg=name)

    for sign in (1, -1):
        for aug in (0.0, 0.1):
            got = aasf(T(g["batch"]), sign * T(g["referent"]), sign * T(g["nadir"]), sign * T(g["ideal"]), aug=aug, scale=100)
            same(f"aasf sign {sign} aug {aug}", got, g[f"aasf_sign{sign}_aug{aug}"])
    same("linear_scalarization", linear_scalarization(T(g["batch"]), T(g["weights"])), g["linear"])


@pytest.mark.parametrize("L", (3, 60))
def test_compute_hvis_leaves_the_generator_where_the_reference_does(be, L):
    """The draw is made also when every point is scored (L <= num)."""
    R, seed = 3, 5
    rng = np.random.default_rng(L)
    lower = rng.uniform(0.0, 5.0, (L, R))
    # (no base point dominates a lower point -- as in a run -- so no two drawn scores tie)
    pf, completed, ideal = rng.uniform(5.0, 8.0, (4, R)), rng.uniform(5.0, 7.0, (2, R)), np.full(R, 9.0)
    ag = bare(be, R, seed=seed)
    lo = io_.Loop(R, None, None, seed=seed)
    for o in (ag, lo):
        o.pf, o.completed, o.ideal, o.lower_points = pf.copy(), completed.copy(), ideal.copy(), lower.copy()
    before = ag.rng.bit_generator.state
    ag.compute_hvis()
    lo.compute_hvis()
    assert ag.rng.bit_generator.state == lo.rng.bit_generator.state != before
    assert np.array_equal(ag.lower_points, lo.lower_points), "scores distinct by far more than 1e-12: the same order"
    if L > 50:
        assert (lo.last_hvis == 0).sum() == L - 50, "the points that were not drawn keep the score 0"


def test_compute_hvis_launch_count_does_not_depend_on_the_candidates():
    import simlib
    be = (simlib.load_sim(), th.device("cpu"))
    count = be[0].lib.hipsim_launch_count
    count.restype = C.c_longlong
    seen = []
    for L in (3, 50):
        R = 3
        rng = np.random.default_rng(L)
        ag = bare(be, R)
        ag.pf, ag.completed, ag.ideal = rng.uniform(2.0, 8.0, (20, R)), rng.uniform(0.0, 3.0, (5, R)), np.full(R, 9.0)
        ag.lower_points = rng.uniform(0.0, 5.0, (L, R))
        c0 = count()
        ag.compute_hvis()
        seen.append(count() - c0)
    assert seen[0] == seen[1] and 1 <= seen[0] <= 3, seen


def test_estimate_error_with_an_empty_upper_set_and_update_not_found(be):
    ag = bare(be, 3)
    ag.pf, ag.upper_points = np.array([[1.0, 2.0, 3.0]]), np.empty((0, 3))
    ag.estimate_error()
    assert ag.error == 0
    # update_not_found drops the lower points with np.any(lower != referent, axis=1): only rows equal to the referent everywhere
    ag.nadir, ag.ideal = np.zeros(3), np.full(3, 10.0)
    ag.lower_points = np.array([[1.0, 2.0, 3.0], [1.0, 2.0, 4.0], [1.0, 2.0, 3.0]])
    ag.upper_points = np.array([[10.0, 10.0, 10.0]])
    from morl_baselines_amd.ipro import Subproblem
    ag.update_not_found(Subproblem(np.array([1.0, 2.0, 3.0]), ag.nadir, ag.ideal), np.array([0.5, 0.5, 0.5]))
    assert np.array_equal(ag.lower_points, [[1.0, 2.0, 4.0]]) and np.array_equal(ag.completed, [[1.0, 2.0, 3.0]])
    assert np.array_equal(ag.robust_points, [[0.5, 0.5, 0.5]]), "a vector that strictly dominates the nadir is kept as robust"
    assert ag.get_config()["method"] == "IPRO" and ag.get_config()["dimensions"] == 3


def test_end_to_end_with_the_real_learner(be):
    from morl_baselines_amd.ipro import IPRO
    lib, dev = be
    th.manual_seed(3)
    env = nlppo_env.DiscreteLinearVecEnv(num_envs=2, obs_dim=5, n_actions=3, reward_dim=2, horizon=4, seed=3)
    env.unwrapped = env
    eval_env = nlppo_env.DiscreteLinearEnv(obs_dim=5, n_actions=3, reward_dim=2, horizon=4, seed=3)
    ag = IPRO(env, iter_total_timesteps=2 * 2 * 8, num_steps=8, num_minibatches=2, update_epochs=2, mc_k=4, max_iterations=2,
              device=dev, lib=lib, seed=2)
    start = ag.agent.params.clone()
    returned = []
    evaluate = ag.agent.policy_evaluate

    def evaluate_logged(eval_env, eval_episodes=100, deterministic=False):
        vec = evaluate(eval_env, eval_episodes=2, deterministic=deterministic)      # (deterministic: every episode is the same)
        returned.append(np.array(vec))
        return vec

    ag.agent.policy_evaluate = evaluate_logged

    def check(pareto_set):
        assert len(pareto_set) >= 1
        for vec, _ in pareto_set:
            assert any(np.array_equal(vec, r) for r in returned), "a Pareto-set vector no policy_evaluate returned"
        assert 0 <= ag.coverage <= 1
        for low in np.asarray(ag.lower_points).reshape(-1, ag.dim):
            assert not np.any(np.all(low > ag.pf, axis=1)), "a lower point strictly dominates a front point"

    with contextlib.redirect_stdout(io.StringIO()):
        pareto_set = ag.train(eval_env, ref_point=None, deterministic=True)
    assert len(returned) in (2 * ag.dim, 2 * ag.dim + 2), "2 d linear trainings, then max_iterations oracle queries unless the front is one point"
    check(pareto_set)
    assert not th.equal(start, ag.agent.params), "the learner's parameters did not change"
    # a learner this small may find one point in both linear problems, which ends the run in the initial phase: the two oracle
    # queries are then made from a given bounding box
    n0 = len(returned)
    ag.reset()
    with contextlib.redirect_stdout(io.StringIO()):
        pareto_set = ag.train(eval_env, ref_point=None, deterministic=True, extrema=(np.full(2, -20.0), np.full(2, 20.0)))
    assert len(returned) == n0 + 2 and len(ag.pf) + len(ag.completed) >= 1 and ag.total_hv == 1600.0
    check(pareto_set)
