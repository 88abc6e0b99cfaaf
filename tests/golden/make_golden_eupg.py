"""EUPG fixtures from the UNMODIFIED reference class (single_policy/esr/eupg.py), CPU, one intra-op thread:

* eupg_<case>.npz   one update() on a synthetic episode at a non-zero Adam step count: the episode (observations as train() hands
                    them to the buffer: floats), the discounted returns, the scalarised values, the loss, the rows' normalised
                    probabilities and log-probs before the step, parameters before and after, moments after (the ones before
                    are ppo_cases.synthetic_moments)
* eupg_trace.npz    a seeded train() of a few episodes on tests/eupg_env.py with a non-linear utility

The restatement in tests/eupg_oracle.py is checked against every recorded value on the way (exact equality).  A seed that breaks
one of the conditions below is refused before anything is written; they are checked on the reference alone:

* cases a to d: the taken action's probability of every row lies in [1e-3, 1 - 1e-3], far from Categorical's clamp
* case a: at least half of the observation entries change by more than 0.1 under the buffer's int32 truncation
* case e: action 0 has a probability below eps in EVERY row; at least 10 % of the rows take action 0 (their log-prob is log(eps)
  exactly) and at least 10 % do not
* trace: the reference re-run with the network's outputs scaled by 1 +- 1e-4 samples the same actions

    PYTHONDONTWRITEBYTECODE=1 python -B tests/golden/make_golden_eupg.py
"""
from __future__ import annotations

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

import ref_harness as rh  # noqa: E402

rh.install_stubs()             # (before momdp: its spaces subclass the stand-in gymnasium's)

import eupg_cases as ec  # noqa: E402
import eupg_env  # noqa: E402
import eupg_oracle as eo  # noqa: E402
from make_golden_pcn import save_npz  # noqa: E402
from pcn_common import SpacesEnv  # noqa: E402


def import_reference():
    from morl_baselines.single_policy.esr import eupg as ref
    return ref


def flat(net):
    return np.concatenate([p.detach().numpy().reshape(-1) for p in net.parameters()]).copy()


def recording(seen):
    """``utility`` that also notes the [T][R] tensors it is called on."""
    def f(r, w=None):
        if w is None:
            seen.append(r.detach().clone())
        return ec.utility(r, w)
    return f


def capture_log(ref):
    """The reference logs its loss through wandb.log and nowhere else: route the stand-in's log into a list."""
    logged = []
    ref.wandb.log = lambda d, *a, **k: logged.append(d)
    return logged


def reference_learner(ref, seed, env, scalarization, **kw):
    """(reference learner, oracle network with the same seeded parameters)"""
    ec.reseed(seed)
    ag = ref.EUPG(env, scalarization, log=False, device="cpu", seed=seed, **kw)
    D, A, R = env.observation_space.shape[0], env.action_space.n, env.reward_space.shape[0]
    ec.reseed(seed)
    onet = eo.PolicyNet(D, A, R, kw["net_arch"])
    assert [n for n, _ in ag.net.named_parameters()] == [n for n, _ in onet.named_parameters()]
    assert np.array_equal(flat(ag.net), flat(onet)), "the oracle's seeded construction differs from the reference's"
    return ag, onet


def step_case(ref, c: ec.StepCase):
    env = SpacesEnv(c.D, c.A, c.R, False, env_id="eupg-fixture-v0")
    seen = []
    ag, onet = reference_learner(ref, c.seed, env, recording(seen), weights=np.ones(c.R), net_arch=list(c.hidden), gamma=c.gamma,
                                 learning_rate=c.lr)
    if c.head_bias0 is not None:
        with th.no_grad():
            list(ag.net.parameters())[-1][0] = c.head_bias0
            list(onet.parameters())[-1][0] = c.head_bias0
    obs, acc, actions, rewards = ec.episode(c)
    for t in range(c.T):
        ag.buffer.add(obs[t], acc[t], int(actions[t]), rewards[t], obs[t], t == c.T - 1)
    P = len(flat(onet))
    m0, v0 = ec.synthetic_moments(c.seed, P)
    eo.set_adam_state(ag.optimizer, ag.net, m0, v0, c.step)
    opt = th.optim.Adam(onet.parameters(), lr=c.lr)
    eo.set_adam_state(opt, onet, m0, v0, c.step)
    p0 = flat(ag.net)

    b_obs, b_acc, b_act, b_rew, _, _ = ag.buffer.get_all_data(to_tensor=True, device="cpu")
    assert b_obs.dtype == th.int32 and np.array_equal(b_obs.numpy(), eo.truncate_obs(obs))
    with th.no_grad():
        dist = ag.net.distribution(b_obs, b_acc)
        probs = dist.probs.numpy().copy()
        logp = dist.log_prob(b_act.squeeze()).numpy().copy().reshape(c.T)

    logged = capture_log(ref)
    ag.log = True
    ag.update()
    ag.log = False
    loss = float(logged[-1]["losses/loss"].detach())
    G = seen[-1]

    o_loss, o_G, o_u, o_probs, o_logp = eo.update(onet, opt, th.tensor(eo.truncate_obs(obs)), th.tensor(acc), th.tensor(actions.reshape(-1, 1)),
                                                  th.tensor(rewards), c.gamma, ec.utility)
    assert float(o_loss) == loss, (c.name, float(o_loss), loss)
    assert th.equal(o_G, G) and np.array_equal(o_probs.numpy(), probs) and np.array_equal(o_logp.numpy().reshape(c.T), logp), c.name
    assert np.array_equal(flat(ag.net), flat(onet)), c.name
    m1, v1 = eo.adam_flat(ag.optimizer, ag.net)
    om1, ov1 = eo.adam_flat(opt, onet)
    assert np.array_equal(m1, om1) and np.array_equal(v1, ov1), c.name

    pa = probs[np.arange(c.T), actions]
    if c.head_bias0 is None:
        assert pa.min() >= 1e-3 and pa.max() <= 1 - 1e-3, f"{c.name}: a taken action's probability is {pa.min():.2e} / {pa.max():.6f}; pick another seed"
    else:
        took0 = actions == 0
        assert (probs[:, 0] < ec.EPS).all(), f"{c.name}: action 0 reaches probability {probs[:, 0].max():.2e}"
        assert took0.mean() >= 0.1 and (~took0).mean() >= 0.1, f"{c.name}: {took0.mean():.2f} of the rows take action 0"
        assert (logp[took0] == np.log(np.float32(ec.EPS))).all(), c.name
    if c.name == "a":
        moved = np.abs(obs - eo.truncate_obs(obs)) > 0.1
        assert moved.mean() >= 0.5, f"{c.name}: the truncation moves {moved.mean():.2f} of the observation entries"
    print(f"eupg_{c.name}: loss {loss:.6f}, taken-action probability {pa.min():.3e} .. {pa.max():.4f}, |G| up to {float(G.abs().max()):.3f}")
    out = dict(obs=obs, acc_rewards=acc, actions=actions, rewards=rewards, returns=G.numpy(), u=o_u.numpy(), loss=np.float32(loss),
               probs=probs, logp=logp, p0=p0, p1=flat(ag.net), m1=m1, v1=v1)
    save_npz(os.path.join(HERE, f"eupg_{c.name}.npz"), out)


def trace_run(ref, scale):
    """One seeded train() of the reference; the network's outputs scaled by ``scale``."""
    Tr = ec.TRACE
    env = eupg_env.LinearEnv(**Tr["env"])
    ec.reseed(Tr["seed"])
    ag = ref.EUPG(env, ec.utility, weights=np.asarray(Tr["weights"]), log=False, device="cpu", seed=Tr["seed"], log_every=10 ** 9,
                  **Tr["agent"])
    if scale != 1.0:
        ag.net.net.register_forward_hook(lambda mod, inp, outp: outp * scale)
    init = flat(ag.net)
    logged = capture_log(ref)
    params, inner = [], ag.update

    def update():
        inner()
        params.append(flat(ag.net))

    ag.update = update
    ag.log = True
    ec.reseed(Tr["seed"] + 1)
    ag.train(total_timesteps=Tr["episodes"] * Tr["env"]["horizon"])
    losses = [float(d["losses/loss"].detach()) for d in logged if "losses/loss" in d]
    scal = [float(d["metrics/scalarized_episodic_return"]) for d in logged if "losses/loss" in d]
    return types.SimpleNamespace(ag=ag, env=env, init=init, params=params, losses=losses, scal=scal)


def trace_case(ref):
    Tr = ec.TRACE
    base = trace_run(ref, 1.0)
    assert len(base.params) == Tr["episodes"]
    for s in (1.0 + 1e-4, 1.0 - 1e-4):
        other = trace_run(ref, s)
        assert base.env.action_log == other.env.action_log, f"a sampled action changes when the outputs are scaled by {s}; pick another seed"
    env = eupg_env.LinearEnv(**Tr["env"])
    ec.reseed(Tr["seed"])
    oa = eo.Learner(env, ec.utility, weights=np.asarray(Tr["weights"]), **Tr["agent"])
    assert np.array_equal(base.init, flat(oa.net))
    o_params = []
    ec.reseed(Tr["seed"] + 1)
    oa.train(Tr["episodes"] * Tr["env"]["horizon"], after_update=lambda ep: o_params.append(flat(oa.net)))
    for a, b in zip(base.params, o_params):
        assert np.array_equal(a, b), "oracle training differs from the reference"
    assert base.env.action_log == env.action_log and base.losses == oa.losses
    counts = np.bincount(base.env.action_log, minlength=Tr["env"]["n_actions"])
    assert (counts > 0).all(), f"an action is never sampled: {counts}"
    out = {"init": base.init, "actions": np.asarray(base.env.action_log, dtype=np.int32), "rewards": np.stack(base.env.reward_log),
           "losses": np.asarray(base.losses, dtype=np.float64), "scalarized_returns": np.asarray(base.scal, dtype=np.float64)}
    for ep, p in enumerate(base.params, 1):
        out[f"params_{ep}"] = p
    save_npz(os.path.join(HERE, "eupg_trace.npz"), out)
    print(f"eupg_trace: {len(base.env.action_log)} steps, actions {counts}, losses {base.losses}")


def main():
    if not rh.reference_available():
        raise RuntimeError("reference tree not found")
    ref = import_reference()
    th.set_num_threads(1)
    only = set(sys.argv[1:])
    want = lambda name: not only or name in only  # noqa: E731
    for c in ec.STEP_CASES:
        if want(c.name):
            step_case(ref, c)
    if want("trace"):
        trace_case(ref)
    largest = max(os.path.getsize(os.path.join(HERE, f)) for f in os.listdir(HERE) if f.startswith("nlppo_") and f.endswith(".npz"))
    for f in sorted(os.listdir(HERE)):
        if f.startswith("eupg_") and f.endswith(".npz"):
            size = os.path.getsize(os.path.join(HERE, f))
            assert size <= largest, f"{f}: {size} bytes, the largest nlppo_*.npz is {largest}"


if __name__ == "__main__":
    main()
