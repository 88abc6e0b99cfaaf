"""The PCN host mirror (morl-baselines_amd/pcn.py): constructor / config parity with the reference class, seeded initial
parameters, replay / heap / command selection and the consumption of ``np_random`` against the fixtures and the restatement,
persistence, and the loud refusals.  ``sim``: kernel sources under the wave emulator; ``hip``: the gfx950 library (-m gpu)."""
import copy
import inspect

import numpy as np
import pytest
import torch as th

import pcn_cases as pc
import pcn_common as pcm
import pcn_oracle as po

import morl_baselines_amd.native as native


@pytest.fixture(scope="module", params=pcm.BACKENDS)
def be(request):
    lib, dev = pcm.backend(request.param)
    native.use_library(lib if request.param == "sim" else None)
    yield lib, dev
    native.use_library(None)


def agent_for(be, c, **kw):
    from morl_baselines_amd.pcn import PCN
    lib, dev = be
    pc.reseed(c.seed)
    env = pcm.SpacesEnv(c.D, c.A, c.R, c.continuous)
    args = dict(learning_rate=c.lr, batch_size=c.B, hidden_dim=c.H, log=False, seed=c.seed, device=dev, lib=lib)
    args.update(kw)
    return PCN(env, pc.scaling_of(c), **args)


def fill(ag, c, Transition, add, max_size=100):
    step = 0
    for ep in pc.synthetic_episodes(c):
        step += len(ep)
        add([Transition(o, a, r.copy(), o, False) for o, a, r in ep], max_size, step)


def test_constructor_and_config_match_the_reference(be):
    from morl_baselines_amd.pcn import PCN
    sig = inspect.signature(PCN.__init__)
    got = [(n, p.default) for n, p in sig.parameters.items() if n != "self"]
    want = [("env", inspect.Parameter.empty), ("scaling_factor", inspect.Parameter.empty), ("learning_rate", 1e-3),      # pcn.py:120-136
            ("gamma", 1.0), ("batch_size", 256), ("hidden_dim", 64), ("noise", 0.1), ("project_name", "MORL-Baselines"),
            ("experiment_name", "PCN"), ("wandb_entity", None), ("log", True), ("seed", None), ("device", "auto"),
            ("model_class", None)]
    assert got[:len(want)] == want
    assert [n for n, _ in got[len(want):]] == ["lib"]
    c = pc.BY_NAME["disc_b50"]
    ag = agent_for(be, c)
    cfg = ag.get_config()
    assert list(cfg) == ["env_id", "batch_size", "gamma", "learning_rate", "hidden_dim", "scaling_factor", "continuous_action",
                         "noise", "seed"]                                                                               # pcn.py:188-200
    assert cfg["batch_size"] == c.B and cfg["continuous_action"] is False and cfg["seed"] == c.seed
    assert [tuple(v.shape) for v in ag.parameter_views()] == [(64, 2), (64,), (64, 3), (64,), (64, 64), (64,), (4, 64), (4,)]
    assert sorted(ag.model.state_dict()) == sorted(["scaling_factor"] + list(pc.PARAM_NAMES))


@pytest.mark.parametrize("c", pc.UPDATE_CASES, ids=lambda c: c.name)
def test_seeded_initial_parameters_and_update_against_the_fixture(be, c):
    """A seeded construction draws the reference's initial parameters; fed the fixture's episodes, the agent builds the
    fixture's table, draws the fixture's rows, leaves ``np_random`` where the reference's update() left it, and steps to the
    fixture's parameters."""
    from morl_baselines_amd.pcn import Transition
    g = pcm.load(c.name)
    ag = agent_for(be, c)
    for i, v in enumerate(ag.parameter_views()):
        assert np.array_equal(v.cpu().numpy(), g[f"p0_{i}"]), f"initial parameter {i}"
    with pytest.raises(RuntimeError, match="experience replay is empty"):
        ag.update()
    fill(ag, c, Transition, lambda tr, m, s: ag._add_episode(tr, max_size=m, step=s))
    ag.exp_avg.copy_(th.tensor(pcm.flat(g, "m0")))
    ag.exp_avg_sq.copy_(th.tensor(pcm.flat(g, "v0")))
    ag._adam_step = c.step
    ag._sync_table()
    assert np.array_equal(ag._table_dev.cpu().numpy(), g["table"]) and np.array_equal(ag._table_rows, g["starts"])
    rng = copy.deepcopy(ag.np_random)
    assert np.array_equal(ag._draw_indices(1)[0], g["idx"])
    ag.np_random = rng
    loss, pred = ag.update()
    assert str(ag.np_random.bit_generator.state["state"]["state"]) == str(g["rng_after"].reshape(-1)[0])
    pcm.close_rel("loss", loss.cpu().numpy(), g["loss"], 1e-5)
    pcm.close_rel("prediction", pred.cpu().numpy(), g["pred"], 1e-5, 1e-6)
    pcm.close_rel("parameters", ag.params.cpu().numpy(), pcm.flat(g, "p1"), 2e-5, 0.02 * c.lr)


def test_rng_state_after_update_n_equals_the_oracle_loop(be):
    from morl_baselines_amd.pcn import Transition
    c = pc.BY_NAME["disc_b50"]
    ag = agent_for(be, c)
    fill(ag, c, Transition, lambda tr, m, s: ag._add_episode(tr, max_size=m, step=s))
    replay, rng = [], np.random.default_rng(c.seed)
    fill(None, c, po.Transition, lambda tr, m, s: po.add_episode(replay, tr, m, s))
    learner = po.Learner([v.cpu() for v in ag.parameter_views()], pc.scaling_of(c), False, lr=c.lr)
    o_losses, o_pred, _ = po.update_loop(learner, replay, rng, c.B, 5)
    losses, ents, pred = ag.update_n(5)
    assert ag.np_random.bit_generator.state == rng.bit_generator.state
    pcm.close_rel("losses", losses.cpu().numpy(), o_losses.numpy(), 1e-5)
    pcm.close_rel("prediction", pred.cpu().numpy(), o_pred.numpy(), 1e-5, 1e-6)
    assert ents.shape == (5,) and ag._adam_step == 5


def test_replay_heap_and_commands_are_bit_identical(be):
    """Scripted: episodes into a heap smaller than their number (heappushpop), commands chosen in between (re-scoring,
    heapify), against the restatement the fixtures pin to the reference."""
    from morl_baselines_amd.pcn import Transition
    c = pc.BY_NAME["disc_b50"]
    ag = agent_for(be, c)
    replay, rng = [], np.random.default_rng(c.seed)
    eps, step = pc.synthetic_episodes(c), 0
    for k, ep in enumerate(eps):
        step += len(ep)
        ag._add_episode([Transition(o, a, r.copy(), o, False) for o, a, r in ep], max_size=7, step=step)
        po.add_episode(replay, [po.Transition(o, a, r.copy(), o, False) for o, a, r in ep], 7, step)
        if k in (3, 6, 8, 11):
            got, want = ag._choose_commands(4), po.choose_commands(replay, rng, 4)
            assert np.array_equal(got[0], want[0]) and got[0].dtype == np.float32 and got[1] == want[1]
        for got, want in zip(po.heap_summary(ag.experience_replay), po.heap_summary(replay)):
            assert np.array_equal(got, want)
    assert ag.np_random.bit_generator.state == rng.bit_generator.state
    from morl_baselines_amd.pareto import get_non_dominated_inds
    pts = np.array([[1.0, 2.0], [2.0, 1.0], [1.0, 2.0], [0.5, 0.5], [2.0, 1.0]])
    assert get_non_dominated_inds(pts).tolist() == po.get_non_dominated_inds(pts).tolist() == [True, True, False, False, False]


def test_acting_and_save_load_round_trip(be, tmp_path):
    c = pc.BY_NAME["cont_b37_h128"]
    g = pcm.load(c.name)
    ag = agent_for(be, c)
    obs, dr, dh = g["table"][0, :c.D], g["table"][0, c.D + c.A:c.D + c.A + c.R], g["table"][0, -1]
    ag.set_desired_return_and_horizon(dr, dh)
    a0 = ag.eval(obs)
    want = po.forward([th.tensor(g[f"p0_{i}"]) for i in range(8)], th.tensor(g["scaling"]), th.tensor(obs[None]),
                      th.tensor(dr[None]), th.tensor([[dh]]), True).numpy()[0]
    pcm.close_rel("eval action", a0, want, 1e-5, 1e-6)
    np.random.seed(3)
    noisy = ag._act(obs, dr, dh)
    np.random.seed(3)
    assert np.array_equal(noisy, a0 + np.random.normal(0.0, ag.noise))          # the GLOBAL generator, one scalar (pcn.py:313)
    ag.save(filename="m", save_dir=str(tmp_path / "w"))
    other = agent_for(be, c, seed=c.seed + 1)
    pc.reseed(99)
    other = agent_for(be, pc.PCNCase("x", c.D, c.R, c.A, c.B, c.H, True, seed=99))
    assert not np.array_equal(other.params.cpu().numpy(), ag.params.cpu().numpy())
    other.load(str(tmp_path / "w" / "m.pt"))
    assert np.array_equal(other.params.cpu().numpy(), ag.params.cpu().numpy())
    other.set_desired_return_and_horizon(dr, dh)
    assert np.array_equal(other.eval(obs), a0)
    with pytest.raises(FileNotFoundError):
        other.load(str(tmp_path / "missing.pt"))


def test_discrete_acting_draws_from_np_random(be):
    c = pc.BY_NAME["disc_b50"]
    g = pcm.load(c.name)
    ag = agent_for(be, c)
    obs, dr, dh = g["table"][0, :c.D], g["table"][0, c.D + 1:c.D + 1 + c.R], g["table"][0, -1]
    logp = ag._forward(obs[None], dr[None], np.array([dh]))[0]
    assert ag._act(obs, dr, dh, eval_mode=True) == np.argmax(logp)
    rng = copy.deepcopy(ag.np_random)
    assert ag._act(obs, dr, dh) == rng.choice(np.arange(c.A), p=np.exp(logp))     # pcn.py:321
    assert ag.np_random.bit_generator.state == rng.bit_generator.state


def test_loud_refusals(be):
    c = pc.BY_NAME["disc_b50"]
    with pytest.raises(NotImplementedError, match="model_class"):
        agent_for(be, c, model_class=th.nn.Module)
    with pytest.raises(ValueError, match="hidden_dim"):
        agent_for(be, c, hidden_dim=48)
    ag = agent_for(be, c)
    with pytest.raises(RuntimeError, match="experience replay is empty"):
        ag.update_n(3)
    import morl_baselines_amd
    assert morl_baselines_amd.PCN is type(ag)
