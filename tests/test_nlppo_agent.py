"""The ``NLMOPPO`` agent (morl-baselines_amd/nl_mo_ppo.py) against fixtures recorded from the reference class: seeded
construction, the loss weights, a whole ``update()`` with and without the ``target_kl`` stop and the tuple it returns,
``reset_agent(pref_dim=0)``, ``eval`` and the greedy action."""
import numpy as np
import pytest
import torch as th

import nlppo_cases as nc
import nlppo_common as nm
import nlppo_env
import nlppo_oracle as no


@pytest.fixture(scope="module", params=nm.BACKENDS)
def be(request):
    return nm.backend(request.param)


def make_agent(be, target_kl=None, **kw):
    from morl_baselines_amd.nl_mo_ppo import NLMOPPO
    lib, dev = be
    U = nc.UPDATE
    envs = nlppo_env.SpacesVecEnv(U["E"], U["D"], U["A"], U["R"])
    args = dict(num_steps=U["T"], total_timesteps=U["T"] * U["E"], num_minibatches=U["num_minibatches"], update_epochs=U["update_epochs"],
                learning_rate=U["lr"], gamma=U["gamma"], gae_lambda=U["gae_lambda"], target_kl=target_kl, mc_k=U["mc_k"], device=dev,
                seed=U["seed"], lib=lib)
    args.update(kw)
    nc.reseed(U["seed"])
    with nm.one_thread():
        return NLMOPPO(0, envs, **args)


def fill(ag, g):
    """The fixture's rollout, preference and recorded initial parameters (a seeded construction gives them to QR rounding only)."""
    U = nc.UPDATE
    ag.params.copy_(th.tensor(g["p0"]))
    for k in ("obs", "acc_rewards", "logprobs", "rewards", "dones", "values"):
        getattr(ag, k).copy_(th.tensor(g[k]))
    ag.actions.copy_(th.tensor(g["actions"]).long())
    ag.pref = th.tensor(g["pref"]).to(ag.device)
    ag.u_func = nc.utility(U["referent"], U["scale"])
    ag.advantages, ag.returns = ag._compute_advantages_and_returns(th.tensor(g["next_obs"]), th.tensor(g["next_acc"]),
                                                                   th.tensor(g["next_done"]))


# orthogonal_ is a QR factorisation in LAPACK, whose rounding differs between CPUs: against the recorded parameters the bound is
# that of a Householder QR of an n x n matrix in float32, n * 2^-23 * gain with n <= 64 and gain <= sqrt(2)
QR_ATOL = 64 * 2.0 ** -23 * 2.0 ** 0.5


def test_seeded_construction_draws_the_reference_parameters(be):
    g, U = nm.load("update_full"), nc.UPDATE
    with nm.one_thread():
        nc.reseed(U["seed"])
        onet = no.Agent(U["D"], U["A"], U["R"], U["pref_dim"], nc.HIDDEN)
        want_state = th.get_rng_state()
    ag = make_agent(be)
    assert th.equal(th.get_rng_state(), want_state), "construction consumed torch's generator differently"
    got = ag.params.cpu().numpy()
    assert np.array_equal(got, no.flat_np(onet))
    nm.close_rel("recorded parameters", got, g["p0"], 0.0, QR_ATOL)
    assert np.array_equal(got == 0.0, g["p0"] == 0.0), "biases"
    names = [n for n, _ in ag.agent.named_parameters()]
    assert names[:2] == ["critic.0.weight", "critic.0.bias"] and names[-1] == "actor.4.bias" and len(names) == 12
    for p in ag.agent.parameters():         # the module's parameters are views of the flat vector
        assert p.data.untyped_storage().data_ptr() == ag.params.untyped_storage().data_ptr()
    assert np.array_equal(ag.init_obs.cpu().numpy(), g["init_obs"])
    assert ag.batch_size == 96 and ag.minibatch_size == 24 and ag.num_iterations == 1 and ag.num_objectives == U["R"]


def test_loss_weights_match_the_reference(be):
    g = nm.load("update_full")
    ag = make_agent(be)
    fill(ag, g)
    w = ag._compute_loss_weights()
    assert w.dtype == th.float32 and tuple(w.shape) == (nc.UPDATE["R"],)
    nm.close_rel("loss weights", w.numpy(), g["weights"], 1e-5)


@pytest.mark.parametrize("kind", list(nc.UPDATE_KINDS))
def test_update_matches_the_reference(be, kind):
    g, U = nm.load(f"update_{kind}"), nc.UPDATE
    ag = make_agent(be, target_kl=nc.UPDATE_KINDS[kind])
    fill(ag, g)
    nm.close_rel("returns", ag.returns.cpu().numpy(), g["returns"], 1e-5, 1e-6 * float(np.abs(g["returns"]).max()))
    nm.close_rel("advantages", ag.advantages.cpu().numpy(), g["advantages"], 1e-5, 1e-6 * float(np.abs(g["advantages"]).max()))
    out = ag.update()
    n = 8 if kind == "kl" else 12
    assert ag.optimizer.steps == n == len(g["stats"]) and tuple(ag.last_stats.shape) == (n, 8)
    nm.close_rel("loss weights", ag.last_loss_weights.numpy(), g["weights"], 1e-5)
    stats = ag.last_stats.cpu().numpy()
    assert np.array_equal(stats[:, 6], g["stats"][:, 6]), "clipfrac"
    nm.check_stats(stats[0], g["stats"][0], g["weights"], "step 0 ")
    nm.close_rel("parameters", ag.params.cpu().numpy(), g["p1"], 2e-5, 0.02 * U["lr"] * n)
    # the returned tuple: the last minibatch's v_loss, pg_loss, entropy and KLs (to what the drift of n steps allows), the mean clipfrac
    assert len(out) == 6 and all(isinstance(x, th.Tensor) and x.ndim == 0 for x in out[:5]) and isinstance(out[5], float)
    nm.close_rel("returned losses", [float(x) for x in out[:5]], g["returned"][:5], 1e-3, 1e-5)
    assert out[5] == g["returned"][5]
    # the shuffles came from rng call for call: the generator is where the reference's is
    rng = np.random.default_rng(U["seed"])
    for _ in range(n // U["num_minibatches"]):
        rng.shuffle(np.arange(U["T"] * U["E"]))
    assert ag.rng.bit_generator.state == rng.bit_generator.state


def test_reset_agent_without_a_preference(be):
    U = nc.UPDATE
    ag = make_agent(be)
    ag.optimizer.steps = 5
    ag.u_func, ag.pref = (lambda v: v.sum()), th.zeros(U["R"])
    with nm.one_thread():
        nc.reseed(7)
        ag.reset_agent(pref_dim=0)
        nc.reseed(7)
        onet = no.Agent(U["D"], U["A"], U["R"], 0, nc.HIDDEN)
    assert ag._ctx and ag.u_func is None and ag.pref is None and ag.optimizer.steps == 0
    assert ag.agent.pref_dim == 0 and ag.agent.critic[0].weight.shape == (64, U["D"] + U["R"])
    assert np.array_equal(ag.params.cpu().numpy(), no.flat_np(onet)) and not ag.exp_avg.any() and not ag.exp_avg_sq.any()
    obs, acc = th.randn(5, U["D"]), th.randn(5, U["R"])
    logp, value = ag._forward(obs, acc, th.ones(U["R"]))           # a preference handed to a pref_dim = 0 agent is not read
    with th.no_grad():
        want_logp = th.log_softmax(onet.logits(obs, acc, None), dim=-1)
        want_value = onet.get_value(obs, acc, None)
    nm.close_rel("log-probs", logp.cpu().numpy(), want_logp.numpy(), 1e-5)
    nm.close_rel("values", value.cpu().numpy(), want_value.numpy(), 1e-5, 1e-6)


def test_eval_consumes_one_categorical_draw(be):
    g, U = nm.load("update_full"), nc.UPDATE
    ag = make_agent(be)
    ag.params.copy_(th.tensor(g["p0"]))
    ag.params[-U["A"]:] = th.tensor([0.0, 1.5, -0.5, 0.7][:U["A"]])           # a policy that is not uniform
    obs, acc, pref = np.linspace(-1, 1, U["D"]).astype(np.float32), np.array([0.3, -0.2], dtype=np.float32), g["pref"]
    th.manual_seed(7)
    action = ag.eval(obs, acc, pref)
    after = th.get_rng_state()
    logp, _ = ag._forward(obs, acc, pref)
    th.manual_seed(7)
    want = th.distributions.Categorical(logits=logp.cpu()).sample()
    assert th.equal(th.get_rng_state(), after), "eval drew something other than one categorical sample"
    assert action.shape == () and int(action) == int(want[0])
    th.manual_seed(7)
    many = ag.eval(np.stack([obs] * 3), np.stack([acc] * 3), pref)
    assert many.shape == (3,) and many.dtype == th.int64


def test_greedy_action_takes_the_first_index_on_a_tie(be):
    U = nc.UPDATE
    ag = make_agent(be)
    ag.params.zero_()                                              # every logit 0: all actions tie
    obs, acc = np.ones((3, U["D"]), dtype=np.float32), np.zeros((3, U["R"]), dtype=np.float32)
    assert ag._greedy(obs, acc, None).tolist() == [0, 0, 0]
    ag.params[-U["A"]:] = th.tensor([0.0, 2.0, 2.0, 1.0][:U["A"]])  # the head's bias: actions 1 and 2 tie for the maximum
    assert ag._greedy(obs, acc, None).tolist() == [1, 1, 1]
    env = nlppo_env.DiscreteLinearEnv(obs_dim=U["D"], n_actions=U["A"], reward_dim=U["R"], horizon=4, seed=3)
    point = ag.policy_evaluate(env, eval_episodes=2, deterministic=True)
    assert env.action_log == [1] * 8 and point.shape == (U["R"],)


def test_refusals(be):
    from morl_baselines_amd.nl_mo_ppo import NLMOPPO
    lib, dev = be
    kw = dict(num_steps=8, num_minibatches=2, mc_k=2, device=dev, lib=lib)
    with pytest.raises(ValueError, match="net_arch"):
        NLMOPPO(0, nlppo_env.SpacesVecEnv(2, 4, 3, 2), net_arch=(48, 64), **kw)
    with pytest.raises(ValueError, match="one or two hidden layers"):
        NLMOPPO(0, nlppo_env.SpacesVecEnv(2, 4, 3, 2), net_arch=(64, 64, 64), **kw)
    with pytest.raises(ValueError, match="input width"):
        NLMOPPO(0, nlppo_env.SpacesVecEnv(2, 125, 3, 2), **kw)
    with pytest.raises(ValueError, match="n_actions"):
        NLMOPPO(0, nlppo_env.SpacesVecEnv(2, 4, 33, 2), **kw)
    with pytest.raises(NotImplementedError, match="log=True"):
        NLMOPPO(0, nlppo_env.SpacesVecEnv(2, 4, 3, 2), log=True, **kw)
    ag = NLMOPPO(0, nlppo_env.SpacesVecEnv(2, 4, 3, 2), net_arch=(32,), **kw)
    with pytest.raises(ValueError, match="pref_dim"):
        ag.reset_agent(pref_dim=1)
