"""``tests/nlppo_oracle.py`` against the NL-MO-PPO fixtures recorded from the unmodified reference: exact equality, on the CPU."""
import numpy as np
import pytest
import torch as th

import nlppo_cases as nc
import nlppo_common as nm
import nlppo_env
import nlppo_oracle as no


def t(a):
    return th.tensor(np.asarray(a))


@pytest.fixture(autouse=True)
def recorded_thread_count():
    with nm.one_thread():
        yield


def pref_of(g):
    return t(g["pref"]) if "pref" in g else None


def flat_batch(g, n):
    return (t(g["obs"]).reshape(n, -1), t(g["acc_rewards"]).reshape(n, -1), t(g["actions"]).reshape(-1).long(), t(g["logprobs"]).reshape(-1),
            t(g["advantages"]).reshape(n, -1), t(g["returns"]).reshape(n, -1), t(g["values"]).reshape(n, -1), pref_of(g))


def seeded(net, recorded):
    """A seeded construction gives the recorded parameters to the rounding of orthogonal_'s QR factorisation (LAPACK: it differs
    between CPUs; n * 2^-23 * gain with n <= 64); everything after it starts from the recorded ones and is exact."""
    nm.close_rel("seeded parameters", no.flat_np(net), recorded, 0.0, 64 * 2.0 ** -23 * 2.0 ** 0.5)
    no.load_flat(net, recorded)


@pytest.mark.parametrize("c", nc.STEP_CASES, ids=lambda c: c.name)
def test_single_step_is_exact(c):
    g = nm.load(c.name)
    nc.reseed(c.seed)
    net = no.Agent(c.D, c.A, c.R, c.pref_dim, nc.HIDDEN)
    seeded(net, g["p0"])
    batch = flat_batch(g, c.M)
    with th.no_grad():
        logp = th.distributions.Categorical(logits=net.logits(batch[0], batch[1], batch[7])).logits
        value = net.get_value(batch[0], batch[1], batch[7])
        greedy = net.get_greedy_action(batch[0], batch[1], batch[7])
    assert np.array_equal(logp.numpy(), g["fwd_logp"]) and np.array_equal(value.numpy(), g["fwd_value"])
    assert np.array_equal(greedy.numpy(), g["fwd_greedy"])
    adv, ret = no.compute_advantages(t(g["rewards"])[:, None], th.zeros(c.M, 1), t(g["values"])[:, None], th.zeros(1, c.R), th.zeros(1), 0.0, 0.0)
    assert np.array_equal(adv.reshape(c.M, c.R).numpy(), g["advantages"]) and np.array_equal(ret.reshape(c.M, c.R).numpy(), g["returns"])
    w, v0 = no.loss_weights(net, t(g["init_obs"]), batch[7], c.u_func())
    assert np.array_equal(w.numpy(), g["weights"]) and np.array_equal(v0.numpy(), g["v_s0"])
    opt = th.optim.Adam(net.parameters(), lr=c.lr, eps=1e-5)
    no.set_adam_state(opt, net, *nc.synthetic_moments(c.seed, len(g["p0"])), c.step)
    cfg = no.Cfg(c.clip_coef, c.ent_coef, c.vf_coef, c.clip_vloss, c.max_grad_norm, c.norm_adv)
    stats, _ = no.minibatch_step(net, opt, cfg, batch, w, g["idx"].astype(np.int64))
    assert np.array_equal(np.asarray([float(s) for s in stats], dtype=np.float32), g["stats"])
    assert np.array_equal(no.flat_np(net), g["p1"])
    m1, v1 = no.adam_flat(opt, net)
    assert np.array_equal(m1, g["m1"]) and np.array_equal(v1, g["v1"])
    assert np.array_equal(np.asarray(no.returned_tuple(g["stats"][None]), dtype=np.float64), g["returned"])


def test_advantages_are_exact():
    g, G = nm.load("gae"), nc.GAE
    adv, ret = no.compute_advantages(t(g["rewards"]), t(g["dones"]), t(g["values"]), t(g["next_value"]), t(g["next_done"]), G["gamma"],
                                     G["gae_lambda"])
    assert np.array_equal(adv.numpy(), g["advantages"]) and np.array_equal(ret.numpy(), g["returns"])


@pytest.mark.parametrize("kind", list(nc.UPDATE_KINDS))
def test_whole_update_is_exact(kind):
    g, U = nm.load(f"update_{kind}"), nc.UPDATE
    nc.reseed(U["seed"])
    net = no.Agent(U["D"], U["A"], U["R"], U["pref_dim"], nc.HIDDEN)
    seeded(net, g["p0"])
    opt = th.optim.Adam(net.parameters(), lr=U["lr"], eps=1e-5)
    batch = flat_batch(g, U["T"] * U["E"])
    adv, ret = no.compute_advantages(t(g["rewards"]), t(g["dones"]), t(g["values"]), t(g["next_value"]), t(g["next_done"]), U["gamma"],
                                     U["gae_lambda"])
    assert np.array_equal(adv.numpy(), g["advantages"]) and np.array_equal(ret.numpy(), g["returns"])
    w, _ = no.loss_weights(net, t(g["init_obs"]), batch[7], nc.utility(U["referent"], U["scale"]))
    assert np.array_equal(w.numpy(), g["weights"])
    stats, idx = no.update(net, opt, no.Cfg(), np.random.default_rng(U["seed"]), batch, w, U["num_minibatches"], U["update_epochs"],
                           nc.UPDATE_KINDS[kind])
    assert np.array_equal(idx, g["idx"]) and np.array_equal(stats, g["stats"])
    assert len(stats) == (8 if kind == "kl" else 12)
    assert np.array_equal(no.flat_np(net), g["p1"])
    assert np.array_equal(np.asarray(no.returned_tuple(stats), dtype=np.float64), g["returned"])


def test_train_trace_is_exact():
    g, Tr = nm.load("trace"), nc.TRACE
    env = nlppo_env.DiscreteLinearVecEnv(num_envs=Tr["num_envs"], **Tr["env"])
    eval_env = nlppo_env.DiscreteLinearEnv(**Tr["env"])
    nc.reseed(Tr["seed"])
    oa = no.Learner(env, seed=Tr["seed"], **Tr["agent"])
    seeded(oa.agent, g["init"])
    evaluate = oa.policy_evaluate
    oa.policy_evaluate = lambda e, deterministic=False: evaluate(e, eval_episodes=Tr["eval_episodes"], deterministic=deterministic)
    nc.reseed(Tr["seed"] + 1)
    params = []
    result = oa.train(eval_env, nc.utility(Tr["referent"], Tr["scale"]), pref=np.asarray(Tr["referent"], dtype=np.float32),
                      deterministic=True, after_iteration=lambda it: params.append(no.flat_np(oa.agent)))
    for it, p in enumerate(params, 1):
        assert np.array_equal(p, g[f"params_{it}"]), it
    assert np.array_equal(np.stack(env.action_log), g["actions"]) and np.array_equal(np.stack(env.reward_log), g["rewards"])
    assert np.array_equal(np.stack(oa.weights_log), g["weights"]) and np.array_equal(np.asarray(oa.lr_log), g["lr"])
    assert np.array_equal(np.asarray(eval_env.action_log), g["eval_actions"]) and np.array_equal(result, g["result"])
