"""``tests/ppo_oracle.py`` against the MO-PPO fixtures recorded from the unmodified reference: exact equality, on the CPU."""
import copy

import numpy as np
import pytest
import torch as th

import ppo_cases as pc
import ppo_common as pm
import ppo_env
import ppo_oracle as po


def t(a):
    return th.tensor(np.asarray(a))


def step_batch(g):
    return tuple(t(g[k]) for k in ("obs", "actions", "logprobs", "advantages", "returns", "values"))


@pytest.fixture(autouse=True)
def recorded_thread_count():
    with pm.one_thread():
        yield


@pytest.mark.parametrize("c", pc.STEP_CASES, ids=lambda c: c.name)
def test_single_step_is_exact(c):
    g = pm.load(c.name)
    net = po.Net(c.D, c.A, c.R, list(c.hidden))
    po.load_flat(net, g["p0"])
    with th.no_grad():
        obs, eps = t(g["obs"]), t(g["fwd_eps"])
        action = net.actor_mean(obs) + th.exp(net.actor_logstd) * eps
        _, logprob, _, value = net.get_action_and_value(obs, action)
    assert np.array_equal(action.numpy(), g["fwd_action"]) and np.array_equal(logprob.numpy(), g["fwd_logprob"])
    assert np.array_equal(value.numpy(), g["fwd_value"])
    opt = th.optim.Adam(net.parameters(), lr=c.lr, eps=1e-5)
    po.set_adam_state(opt, net, *pc.synthetic_moments(c.seed, len(g["p0"])), c.step)
    cfg = po.Cfg(c.clip_coef, c.ent_coef, c.vf_coef, c.clip_vloss, c.max_grad_norm, c.norm_adv)
    stats, _, _ = po.minibatch_step(net, opt, cfg, *step_batch(g), g["idx"].astype(np.int64))
    assert np.array_equal(np.asarray([float(s) for s in stats], dtype=np.float32), g["stats"])
    assert np.array_equal(po.flat_np(net), g["p1"])
    m1, v1 = po.adam_flat(opt, net)
    assert np.array_equal(m1, g["m1"]) and np.array_equal(v1, g["v1"])


def seeded(net, recorded):
    """A seeded construction gives the recorded parameters to the rounding of orthogonal_'s QR factorisation (LAPACK: it differs
    between CPUs; n * 2^-23 * gain with n <= 64); everything after it starts from the recorded ones and is exact."""
    pm.close_rel("seeded parameters", po.flat_np(net), recorded, 0.0, 64 * 2.0 ** -23 * 2.0 ** 0.5)
    po.load_flat(net, recorded)


@pytest.mark.parametrize("use_gae", [True, False], ids=["gae", "mc"])
def test_advantages_are_exact(use_gae):
    g, G = pm.load("gae"), pc.GAE
    ret, adv = po.compute_advantages(t(g["rewards"]), t(g["dones"]), t(g["values"]), t(g["next_value"]), t(g["next_done"]),
                                     t(g["weights"]), G["gamma"], G["gae_lambda"], use_gae)
    tag = "gae" if use_gae else "mc"
    assert np.array_equal(ret.numpy(), g[f"returns_{tag}"]) and np.array_equal(adv.numpy(), g[f"advantages_{tag}"])


@pytest.mark.parametrize("kind", list(pc.UPDATE_KINDS))
def test_whole_update_is_exact(kind):
    g, U = pm.load(f"update_{kind}"), pc.UPDATE
    pc.reseed(U["seed"])
    net = po.Net(U["D"], U["A"], U["R"], list(U["hidden"]))
    seeded(net, g["p0"])
    opt = th.optim.Adam(net.parameters(), lr=U["lr"], eps=1e-5)
    n = U["T"] * U["E"]
    batch = (t(g["obs"]).reshape(n, -1), t(g["actions"]).reshape(n, -1), t(g["logprobs"]).reshape(-1),
             t(g["advantages"]).reshape(-1), t(g["returns"]).reshape(n, -1), t(g["values"]).reshape(n, -1))
    stats, idx = po.update(net, opt, po.Cfg(), np.random.default_rng(U["seed"]), batch, U["num_minibatches"], U["update_epochs"],
                           pc.UPDATE_KINDS[kind])
    assert np.array_equal(idx, g["idx"]) and np.array_equal(stats, g["stats"])
    assert len(stats) == int(g["adam_steps"].reshape(-1)[0]) == (8 if kind == "kl" else 12)
    assert np.array_equal(po.flat_np(net), g["p1"])


def test_train_trace_is_exact():
    g, Tr = pm.load("trace"), pc.TRACE
    e = Tr["env"]
    pc.reseed(Tr["seed"])
    net = po.Net(e["obs_dim"], e["action_dim"], e["reward_dim"], list(Tr["hidden"]))
    seeded(net, g["init"])
    env = ppo_env.LinearVecEnv(**e)
    agent = po.Agent(net, Tr["weights"].copy(), env, seed=Tr["seed"], **Tr["agent"])
    pc.reseed(Tr["seed"] + 1)
    for it in range(1, Tr["iterations"] + 1):
        agent.train(it, Tr["iterations"])
        assert np.array_equal(po.flat_np(net), g[f"params_{it}"])
    assert np.array_equal(np.stack(env.action_log), g["actions"]) and np.array_equal(np.stack(env.reward_log), g["rewards"])
