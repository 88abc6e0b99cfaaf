"""The LCN host mirror (morl-baselines_amd/lcn.py): constructor / config parity with the reference class, the refusals,
``_choose_commands`` on a fixed heap against the fixture recorded from the reference (tests/golden/lcn_commands.npz), and
persistence under the reference's names.  ``sim``: kernel sources under the wave emulator; ``hip``: the gfx950 library (-m gpu)."""
import inspect

import numpy as np
import pytest
import torch as th

import lcn_cases as lc
import lcn_common as lcm
import lcn_oracle as lo
import pcn_cases as pc
import pcn_common as pcm
import pcn_oracle as po

import morl_baselines_amd.native as native


@pytest.fixture(scope="module", params=lcm.BACKENDS)
def be(request):
    lib, dev = lcm.backend(request.param)
    native.use_library(lib if request.param == "sim" else None)
    yield lib, dev
    native.use_library(None)


def agent_for(be, R=3, D=4, A=3, continuous=False, seed=31, **kw):
    from morl_baselines_amd.lcn import LCN
    lib, dev = be
    pc.reseed(seed)
    env = pcm.SpacesEnv(D, A, R, continuous, env_id="lcn-fixture-v0")
    args = dict(log=False, seed=seed, device=dev, lib=lib)
    args.update(kw)
    return LCN(env, np.full(R + 1, 0.1, dtype=np.float32), **args)


def test_constructor_and_config_match_the_reference(be):
    from morl_baselines_amd.lcn import LCN, lorenz_vector
    from morl_baselines_amd.pcn import PCN
    sig = inspect.signature(LCN.__init__)
    got = [(n, p.default) for n, p in sig.parameters.items() if n != "self"]
    want = [("env", inspect.Parameter.empty), ("scaling_factor", inspect.Parameter.empty), ("learning_rate", 1e-2),      # lcn.py:69-87
            ("gamma", 1.0), ("batch_size", 32), ("hidden_dim", 64), ("noise", 0.1), ("distance_ref", "nondominated"),
            ("lcn_lambda", None), ("project_name", "MORL-Baselines"), ("experiment_name", "LCN"), ("wandb_entity", None),
            ("log", True), ("seed", None), ("device", "auto"), ("model_class", None)]
    assert got[:len(want)] == want
    assert [n for n, _ in got[len(want):]] == ["lib"]
    tr = inspect.signature(LCN.train).parameters                                                                       # lcn.py:372-387
    assert [(n, tr[n].default) for n in ("num_er_episodes", "num_step_episodes", "num_model_updates", "max_buffer_size",
                                         "num_points_pf", "save_dir", "cd_threshold")] == \
        [("num_er_episodes", 500), ("num_step_episodes", 10), ("num_model_updates", 100), ("max_buffer_size", 500),
         ("num_points_pf", 100), ("save_dir", "weights"), ("cd_threshold", 0.2)]
    ag = agent_for(be, distance_ref="lambda_lorenz", lcn_lambda=0.25)
    assert isinstance(ag, PCN) and ag.batch_size == 32 and ag.learning_rate == 1e-2
    cfg = ag.get_config()
    assert list(cfg) == ["env_id", "reward_dim", "batch_size", "gamma", "learning_rate", "hidden_dim", "scaling_factor",
                         "continuous_action", "noise", "distance_ref", "lcn_lambda", "seed"]                            # lcn.py:148-163
    assert cfg["reward_dim"] == 3 and cfg["distance_ref"] == "lambda_lorenz" and cfg["lcn_lambda"] == 0.25 and cfg["seed"] == 31
    pts = np.array([[3.0, 1.0, 2.0], [0.5, 0.5, 4.0]], dtype=np.float32)
    assert np.array_equal(lorenz_vector(pts), [[1.0, 3.0, 6.0], [0.5, 1.0, 5.0]])
    assert np.array_equal(lorenz_vector(pts, proportional=True), lo.lorenz_vector(pts, proportional=True))
    import morl_baselines_amd
    assert morl_baselines_amd.LCN is LCN


def test_loud_refusals(be):
    with pytest.raises(ValueError, match="distance_ref"):
        agent_for(be, distance_ref="pareto")
    with pytest.raises(ValueError, match="lcn_lambda must be set"):
        agent_for(be, distance_ref="lambda_lorenz")
    with pytest.raises(NotImplementedError, match="model_class"):
        agent_for(be, model_class=th.nn.Module)
    with pytest.raises(ValueError, match="hidden_dim"):
        agent_for(be, hidden_dim=48)
    ag = agent_for(be)
    with pytest.raises(ValueError, match="max_buffer_size 2049"):
        ag.train(10, None, np.zeros(3), max_buffer_size=2049)
    with pytest.raises(ValueError, match="2049 episodes"):
        ag._select(np.zeros((2049, 3), dtype=np.float32), 1)


@pytest.mark.parametrize("variant", list(lc.COMMANDS["variants"]))
def test_choose_commands_on_a_fixed_heap(be, variant):
    """Episodes into a heap smaller than their number (heappushpop), commands chosen in between (the launch, argsort, the heap
    rewrite, heapify, the second strict-Lorenz filter): commands, heap and generator state of the reference."""
    from morl_baselines_amd.pcn import Transition
    C, g = lc.COMMANDS, lcm.load("commands")
    v = C["variants"][variant]
    ag = agent_for(be, R=C["R"], seed=C["seed"], **v)
    ag.cd_threshold = C["cd_threshold"]
    thresholds = []
    nlargest = ag._nlargest
    ag._nlargest = lambda n, threshold=0.2: (thresholds.append(threshold), nlargest(n, threshold))[1]
    replay, rng = [], np.random.default_rng(C["seed"])
    step, cmds = 0, []
    for k, ep in enumerate(lc.command_episodes()):
        step += len(ep)
        ag._add_episode([Transition(o, a, r.copy(), o, False) for o, a, r in ep], max_size=C["max_size"], step=step)
        po.add_episode(replay, [po.Transition(o, a, r.copy(), o, False) for o, a, r in ep], C["max_size"], step)
        if k % 8 == 7:
            got = ag._choose_commands(C["num_episodes"])
            want = lo.choose_commands(replay, rng, C["num_episodes"], C["cd_threshold"], v["distance_ref"], v["lcn_lambda"])
            assert np.array_equal(got[0], want[0]) and got[0].dtype == np.float32 and got[1] == want[1]
            cmds.append(got)
    assert thresholds == [C["cd_threshold"]] * len(cmds), "_choose_commands passes self.cd_threshold (lcn.py:264)"
    assert np.array_equal(np.stack([c[0] for c in cmds]), g[f"{variant}_returns"])
    assert np.array_equal(np.asarray([c[1] for c in cmds], dtype=np.float32), g[f"{variant}_horizons"])
    for got, key in zip(po.heap_summary(ag.experience_replay), ("distance", "step", "return", "length")):
        assert np.array_equal(got, g[f"{variant}_heap_{key}"]), key
    assert str(ag.np_random.bit_generator.state["state"]["state"]) == str(g[f"{variant}_rng_after"].reshape(-1)[0])
    assert all(isinstance(e[0], np.float32) for e in ag.experience_replay), "the heap keys are numpy's float32 l2"


def test_evaluate_passes_the_threshold_of_train(be):
    from morl_baselines_amd.pcn import Transition
    ag = agent_for(be, R=3)
    for k, ep in enumerate(lc.command_episodes()[:6]):
        ag._add_episode([Transition(o, a, r.copy(), o, False) for o, a, r in ep], max_size=10, step=k)
    seen = []
    ag._nlargest = lambda n, threshold=0.2: (seen.append((n, threshold)), [])[1]
    ag.cd_threshold = 0.35
    with pytest.raises(ValueError):          # (zip(*[]) of the stubbed selection: only the call's arguments matter here)
        ag.evaluate(None, None, n=50)
    assert seen == [(6, 0.35)]                                                                                          # lcn.py:344-345


class ReferenceShaped(th.nn.Module):
    """A model whose state_dict carries the reference's names (ContinuousActionsDefaultModel, pcn.py:91-103) and nothing of ours."""

    def __init__(self):
        super().__init__()
        self.scaling_factor = th.nn.Parameter(th.full((3,), 0.2), requires_grad=False)
        self.s_emb = th.nn.Sequential(th.nn.Linear(5, 128), th.nn.Sigmoid())
        self.c_emb = th.nn.Sequential(th.nn.Linear(3, 128), th.nn.Sigmoid())
        self.fc = th.nn.Sequential(th.nn.Linear(128, 128), th.nn.ReLU(), th.nn.Linear(128, 2))


def test_save_load_round_trip_and_reference_names(be, tmp_path):
    ag = agent_for(be, R=2, D=5, A=2, continuous=True, hidden_dim=128, seed=14)
    ag.save(save_dir=str(tmp_path / "w"))
    assert (tmp_path / "w" / "LCN_model.pt").is_file()                                                                  # lcn.py:360-364
    other = agent_for(be, R=2, D=5, A=2, continuous=True, hidden_dim=128, seed=99)
    assert not np.array_equal(other.params.cpu().numpy(), ag.params.cpu().numpy())
    other.load(str(tmp_path / "w" / "LCN_model.pt"))
    assert np.array_equal(other.params.cpu().numpy(), ag.params.cpu().numpy())
    obs, dr = np.linspace(-1, 1, 5).astype(np.float32), np.array([1.0, 2.0], dtype=np.float32)
    ag.set_desired_return_and_horizon(dr, np.float32(4.0))
    other.set_desired_return_and_horizon(dr, np.float32(4.0))
    assert np.array_equal(other.eval(obs), ag.eval(obs))
    with pytest.raises(FileNotFoundError):
        other.load(str(tmp_path / "missing.pt"))

    th.manual_seed(5)
    m = ReferenceShaped()
    assert sorted(m.state_dict()) == sorted(["scaling_factor"] + list(pc.PARAM_NAMES))
    th.save(m, str(tmp_path / "ref.pt"))
    other.load(str(tmp_path / "ref.pt"))
    for v, k in zip(other.parameter_views(), pc.PARAM_NAMES):
        assert np.array_equal(v.cpu().numpy(), m.state_dict()[k].numpy()), k
    assert np.array_equal(other.model.scaling_factor.data.cpu().numpy(), np.full(3, 0.2, dtype=np.float32))
