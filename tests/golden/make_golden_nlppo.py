"""NL-MO-PPO fixtures from the UNMODIFIED reference class (single_policy/ser/nl_mo_ppo.py), CPU, one intra-op thread:

* nlppo_<case>.npz          one minibatch step at a non-zero Adam step count: the rollout rows, the visiting order, the loss weights,
                            the step's statistics, parameters before and after, moments after (the ones before are
                            ppo_cases.synthetic_moments), and the normalised log-probabilities / values of the rows before the step
* nlppo_gae.npz             _compute_advantages_and_returns
* nlppo_update_<kind>.npz   a whole update(): 3 epochs x 4 minibatches, to the end and stopped by target_kl after the second epoch
* nlppo_trace.npz           a seeded train() of two iterations on tests/nlppo_env.py and the final policy_evaluate

The restatement in tests/nlppo_oracle.py is checked against every recorded value on the way (exact equality).  A seed that breaks
one of the conditions below is refused before anything is written:

* every recorded step: no ratio within 1e-4 of a clip boundary and no |v - old| within 1e-4 of c, in float32 and in float64
* single steps a to c: at least 10 % of the rows have the ratio clipped and at least 10 % unclipped; in at least 5 % of the rows
  the objectives disagree on the active surrogate branch; the gradient norm is above max_grad_norm (in d: below it)
* loss weights: the terms inside the utility's min differ by at least 1e-3 relative whenever _compute_loss_weights runs
* trace: the reference re-run with the actor's logits scaled by 1 +- 1e-4 samples the same actions
* target_kl: every epoch-end approx_kl is at least 10 % away from it

    PYTHONDONTWRITEBYTECODE=1 python -B tests/golden/make_golden_nlppo.py
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

import ref_harness as rh  # noqa: E402
import nlppo_cases as nc  # noqa: E402
import nlppo_env  # noqa: E402
import nlppo_oracle as no  # noqa: E402
from make_golden_pcn import save_npz  # noqa: E402

MARGIN = 1e-4


def import_reference():
    rh.install_stubs()
    from morl_baselines.single_policy.ser import nl_mo_ppo as ref
    return ref


def flat(net):
    return np.concatenate([p.detach().numpy().reshape(-1) for p in net.parameters()]).copy()


def recording(u, seen):
    """``u`` that also notes the value vector it is evaluated at."""
    def f(v):
        seen.append(v.detach().numpy().astype(np.float64).copy())
        return u(v)
    return f


def check_min_terms(name, u, seen):
    if not hasattr(u, "terms"):
        return
    assert seen, name
    for v in seen:
        t = np.sort(u.terms(v))
        assert t[1] - t[0] >= 1e-3 * np.abs(t).max(), f"{name}: the utility's min is within 1e-3 of a tie at v(s0) = {v}; pick another seed"


def reference_learner(ref, seed, envs, pref_dim, **kw):
    """(reference learner, oracle agent with the same seeded parameters)"""
    nc.reseed(seed)
    ag = ref.NLMOPPO(0, envs, log=False, device="cpu", seed=seed, **kw)
    R = envs.reward_space.shape[0]
    if pref_dim != R:
        nc.reseed(seed)
        ag.reset_agent(pref_dim=pref_dim)
    D, A = envs.single_observation_space.shape[0], envs.single_action_space.n
    # the oracle draws what the reference's LAST construction drew
    nc.reseed(seed)
    onet = no.Agent(D, A, R, pref_dim, nc.HIDDEN)
    assert [n for n, _ in ag.agent.named_parameters()] == [n for n, _ in onet.named_parameters()]
    assert np.array_equal(flat(ag.agent), flat(onet)), "the oracle's seeded construction differs from the reference's"
    return ag, onet


def synthetic_rollout(net, seed, T, E, perturb, pref, obs_scale=1.0, done_rate=0.1):
    """obs and accrued rewards, and actions / log-probs / values of a PERTURBED copy of ``net`` (the behaviour policy), rewards, dones."""
    D, A, R = net.obs_dim, net.n_actions, net.num_objectives
    g = th.Generator().manual_seed(seed + 1000)
    gp = th.Generator().manual_seed(seed + 1001)
    old = copy.deepcopy(net)
    with th.no_grad():
        for p in old.parameters():
            p.add_(perturb * th.randn(p.shape, generator=gp))
    obs = obs_scale * th.randn(T * E, D, generator=g)
    acc = obs_scale * 0.5 * th.randn(T * E, R, generator=g)
    with th.no_grad():
        logp = th.log_softmax(old.logits(obs, acc, pref), dim=-1)
        actions = th.multinomial(logp.exp(), 1, generator=g).reshape(-1)
        _, logprobs, _, values = old.get_action_and_value(obs, acc, action=actions, pref=pref)
    rewards = th.randn(T * E, R, generator=g)
    dones = (th.rand(T * E, generator=g) < done_rate).float()
    return dict(obs=obs.view(T, E, D), acc_rewards=acc.view(T, E, R), actions=actions.view(T, E), logprobs=logprobs.view(T, E),
                rewards=rewards.view(T, E, R), dones=dones.view(T, E), values=values.view(T, E, R)), g


def fill(ag, roll):
    for k, v in roll.items():
        getattr(ag, k).copy_(v)


def batch_of(roll, advantages, returns, pref):
    T, E = roll["logprobs"].shape
    R = roll["values"].shape[-1]
    return (roll["obs"].reshape(T * E, -1), roll["acc_rewards"].reshape(T * E, R), roll["actions"].reshape(-1), roll["logprobs"].reshape(-1),
            advantages.reshape(T * E, R), returns.reshape(T * E, R), roll["values"].reshape(T * E, R), pref)


def margins(c, rows, oldv, clip_vloss):
    r = rows["ratio"].double().numpy()
    m = min(np.abs(r - (1 - c)).min(), np.abs(r - (1 + c)).min())
    if clip_vloss:
        m = min(m, np.abs(np.abs(rows["newvalue"].double().numpy() - oldv.double().numpy()) - c).min())
    return float(m)


def check_margins(name, onet0, cfg, lr, batch, weights, idx, f32_seen, m0=None, v0=None, step=0):
    """No row of any recorded step within MARGIN of a clip boundary -- float32 (as recorded) and float64 (the same steps in double)."""
    worst = min(f32_seen)
    net64 = no.to_dtype(onet0, th.float64)
    opt64 = th.optim.Adam(net64.parameters(), lr=lr, eps=1e-5)
    if m0 is not None:
        no.set_adam_state(opt64, net64, m0, v0, step)
    b64 = batch_of_dtype(batch, th.float64)
    for mb in idx:
        mb = mb.astype(np.int64)
        _, rows = no.minibatch_step(net64, opt64, cfg, b64, weights.double(), mb)
        worst = min(worst, margins(cfg.clip_coef, rows, b64[6][mb], cfg.clip_vloss))
    assert worst >= MARGIN, f"{name}: a row lies {worst:.2e} from a clip boundary; pick another seed"
    return worst


def batch_of_dtype(batch, dtype):
    return tuple(x if (x is None or x.dtype == th.int64) else x.to(dtype) for x in batch)


def run_update(name, ag, onet, cfg, lr, roll, pref, u, num_minibatches, update_epochs, target_kl, m0=None, v0=None, step=0):
    """Runs the reference's update() and the oracle's on the same rollout; asserts they agree exactly; returns what to record."""
    seen_v = []
    ag.u_func = recording(u, seen_v)
    ag.pref = pref
    if m0 is not None:
        no.set_adam_state(ag.optimizer, ag.agent, m0, v0, step)
    p0 = flat(ag.agent)
    batch = batch_of(roll, ag.advantages, ag.returns, pref)
    onet0 = copy.deepcopy(onet)
    opt = th.optim.Adam(onet.parameters(), lr=lr, eps=1e-5)
    if m0 is not None:
        no.set_adam_state(opt, onet, m0, v0, step)
    w, v_s0 = no.loss_weights(onet, ag.init_obs, pref, u)
    seen, rows_log = [], []

    def observer(rows, mb):
        seen.append(margins(cfg.clip_coef, rows, batch[6][mb], cfg.clip_vloss))
        rows_log.append(rows)

    stats, idx = no.update(onet, opt, cfg, copy.deepcopy(ag.rng), batch, w, num_minibatches, update_epochs, target_kl, observer)
    got = ag.update()
    check_min_terms(name, u, seen_v)
    want = no.returned_tuple(stats)
    assert np.array_equal(np.asarray([float(x.detach()) for x in got[:5]], dtype=np.float32), np.asarray(want[:5], dtype=np.float32)), (name, got, want)
    assert got[5] == want[5], (name, got[5], want[5])
    assert np.array_equal(flat(ag.agent), flat(onet)), name
    m1, v1 = no.adam_flat(ag.optimizer, ag.agent)
    om1, ov1 = no.adam_flat(opt, onet)
    assert np.array_equal(m1, om1) and np.array_equal(v1, ov1), name
    worst = check_margins(name, onet0, cfg, lr, batch, w, idx, seen, m0, v0, step)
    out = dict(p0=p0, p1=flat(ag.agent), m1=m1, v1=v1, stats=stats, idx=idx, weights=w.numpy(), v_s0=v_s0.numpy(),
               init_obs=ag.init_obs.numpy(), returned=np.asarray([float(x.detach()) for x in got[:5]] + [got[5]], dtype=np.float64))
    return out, rows_log, worst, onet0


def step_case(ref, c: nc.StepCase):
    envs = nlppo_env.SpacesVecEnv(1, c.D, c.A, c.R, c.obs_scale)
    ag, onet = reference_learner(ref, c.seed, envs, c.pref_dim, num_steps=c.M, total_timesteps=c.M, num_minibatches=1, update_epochs=1,
                                 learning_rate=c.lr, gamma=0.0, gae_lambda=0.0, clip_coef=c.clip_coef, ent_coef=c.ent_coef,
                                 vf_coef=c.vf_coef, clip_vloss=c.clip_vloss, max_grad_norm=c.max_grad_norm, norm_adv=c.norm_adv,
                                 mc_k=c.mc_k)
    gp = th.Generator().manual_seed(c.seed + 3000)
    pref = th.rand(c.R, generator=gp) if (c.with_pref and c.pref_dim) else None
    roll, g = synthetic_rollout(onet, c.seed, c.M, 1, c.perturb, pref, c.obs_scale)
    # advantages and returns as a rollout of M steps of one env gives them with gamma = 0: advantages = rewards - values,
    # returns = advantages + values -- what a test reproduces through morl_nlppo_set_rollout + morl_nlppo_gae
    roll["rewards"] = roll["values"] + c.ret_scale * th.randn(c.M, 1, c.R, generator=g)
    roll["dones"] = th.zeros(c.M, 1)
    fill(ag, roll)
    ag.pref = pref
    ag.advantages, ag.returns = ag._compute_advantages_and_returns(th.zeros(1, c.D), th.zeros(1, c.R), th.zeros(1))
    o_adv, o_ret = no.compute_advantages(roll["rewards"], roll["dones"], roll["values"], th.zeros(1, c.R), th.zeros(1), 0.0, 0.0)
    assert th.equal(ag.advantages, o_adv) and th.equal(ag.returns, o_ret)

    out = {}
    obs, acc = roll["obs"].reshape(c.M, c.D), roll["acc_rewards"].reshape(c.M, c.R)
    with th.no_grad():
        aug = ag.agent._build_aug_obs(obs, acc, pref)
        f_logp = ref.Categorical(logits=ag.agent.actor(aug)).logits
        f_value = ag.agent.get_value(obs, acc, pref)
        assert th.equal(f_logp, th.distributions.Categorical(logits=onet.logits(obs, acc, pref)).logits)
        greedy = ag.agent.get_greedy_action(obs, acc, pref)
    out.update(fwd_logp=f_logp.numpy(), fwd_value=f_value.numpy(), fwd_greedy=greedy.numpy())

    cfg = no.Cfg(c.clip_coef, c.ent_coef, c.vf_coef, c.clip_vloss, c.max_grad_norm, c.norm_adv)
    m0, v0 = nc.synthetic_moments(c.seed, len(flat(onet)))
    rec, rows_log, worst, _ = run_update(f"nlppo_{c.name}", ag, onet, cfg, c.lr, roll, pref, c.u_func(), 1, 1, None, m0, v0, c.step)
    rows = rows_log[0]
    ratio = rows["ratio"].numpy()
    rclip = float((np.abs(ratio - 1.0) > c.clip_coef).mean())
    inside = ((ratio >= 1 - c.clip_coef) & (ratio <= 1 + c.clip_coef))[:, None]
    active = inside | (rows["pg1"].numpy() > rows["pg2"].numpy())
    disagree = float((active.any(axis=1) & ~active.all(axis=1)).mean())
    stats = rec["stats"][0]
    print(f"nlppo_{c.name}: loss {stats[0]:.5f} grad norm {stats[7]:.4f} ratio clipped {rclip:.2f} objectives disagree {disagree:.2f} "
          f"weights {rec['weights']} margin {worst:.2e}")
    if c.clip_active:
        assert 0.1 <= rclip <= 0.9, f"{c.name}: {rclip:.2f} of the rows have the ratio clipped"
        assert disagree >= 0.05, f"{c.name}: the objectives disagree on the active branch in {disagree:.2f} of the rows"
        assert stats[7] > c.max_grad_norm, f"{c.name}: gradient norm {stats[7]} does not reach the clip"
    else:
        assert stats[7] < c.max_grad_norm, f"{c.name}: gradient norm {stats[7]} is clipped"
    if c.weights is not None:
        assert np.array_equal(rec["weights"], np.asarray(c.weights, dtype=np.float32)) and (rec["weights"] < 0).sum() == 1
    batch = batch_of(roll, ag.advantages, ag.returns, pref)
    rec["stats"], rec["idx"] = rec["stats"][0], rec["idx"][0]
    out.update(rec)
    out.update(obs=batch[0].numpy(), acc_rewards=batch[1].numpy(), actions=batch[2].numpy().astype(np.int32), logprobs=batch[3].numpy(),
               advantages=batch[4].numpy(), returns=batch[5].numpy(), values=batch[6].numpy(), rewards=roll["rewards"].reshape(c.M, c.R).numpy())
    if pref is not None:
        out["pref"] = pref.numpy()
    save_npz(os.path.join(HERE, f"nlppo_{c.name}.npz"), out)


def gae_case(ref):
    G = nc.GAE
    T, E, R = G["T"], G["E"], G["R"]
    envs = nlppo_env.SpacesVecEnv(E, 3, 2, R)
    ag, onet = reference_learner(ref, G["seed"], envs, R, num_steps=T, total_timesteps=T * E, gamma=G["gamma"], gae_lambda=G["gae_lambda"], mc_k=4)
    roll, g = synthetic_rollout(onet, G["seed"], T, E, 0.1, None, done_rate=G["done_rate"])
    fill(ag, roll)
    next_obs, next_acc = th.randn(E, 3, generator=g), th.randn(E, R, generator=g)
    next_done = th.tensor([0.0, 1.0, 0.0, 0.0])
    assert 0.04 < float(roll["dones"].mean()) < 0.2
    adv, ret = ag._compute_advantages_and_returns(next_obs, next_acc, next_done)
    with th.no_grad():
        next_value = ag.agent.get_value(next_obs, next_acc, None).reshape(E, R)
    o_adv, o_ret = no.compute_advantages(roll["rewards"], roll["dones"], roll["values"], next_value, next_done, G["gamma"], G["gae_lambda"])
    assert th.equal(adv, o_adv) and th.equal(ret, o_ret)
    out = {k: roll[k].numpy() for k in ("rewards", "dones", "values")}
    out.update(next_value=next_value.numpy(), next_done=next_done.numpy(), advantages=adv.numpy(), returns=ret.numpy())
    save_npz(os.path.join(HERE, "nlppo_gae.npz"), out)
    print("nlppo_gae: done fraction", float(roll["dones"].mean()))


def update_case(ref, kind, target_kl):
    U = nc.UPDATE
    T, E, R = U["T"], U["E"], U["R"]
    envs = nlppo_env.SpacesVecEnv(E, U["D"], U["A"], R)
    ag, onet = reference_learner(ref, U["seed"], envs, U["pref_dim"], num_steps=T, total_timesteps=T * E,
                                 num_minibatches=U["num_minibatches"], update_epochs=U["update_epochs"], learning_rate=U["lr"],
                                 gamma=U["gamma"], gae_lambda=U["gae_lambda"], target_kl=target_kl, mc_k=U["mc_k"])
    pref = th.tensor(U["referent"], dtype=th.float32)
    roll, g = synthetic_rollout(onet, U["seed"], T, E, U["perturb"], pref)
    fill(ag, roll)
    ag.pref = pref
    next_obs, next_acc, next_done = th.randn(E, U["D"], generator=g), th.randn(E, R, generator=g), th.zeros(E)
    with th.no_grad():
        next_value = ag.agent.get_value(next_obs, next_acc, pref).reshape(E, R)
    ag.advantages, ag.returns = ag._compute_advantages_and_returns(next_obs, next_acc, next_done)
    cfg = no.Cfg()
    rec, _, worst, _ = run_update(f"nlppo_update_{kind}", ag, onet, cfg, U["lr"], roll, pref, nc.utility(U["referent"], U["scale"]),
                                  U["num_minibatches"], U["update_epochs"], target_kl)
    stats = rec["stats"]
    per_epoch = U["num_minibatches"]
    kls = stats[per_epoch - 1::per_epoch, 5]
    print(f"nlppo_update_{kind}: {len(stats)} steps, epoch-end approx_kl {kls}, weights {rec['weights']}, margin {worst:.2e}")
    if target_kl is None:
        assert len(stats) == U["update_epochs"] * per_epoch
    else:
        assert len(stats) == 2 * per_epoch, f"target_kl {target_kl} stops after {len(stats)} steps, not after the second epoch"
        assert all(abs(float(k) - target_kl) >= 0.1 * target_kl for k in kls), (kls, target_kl)
    out = {k: v.numpy() for k, v in roll.items()}
    out["actions"] = out["actions"].astype(np.int32)
    out.update(rec)
    out.update(next_obs=next_obs.numpy(), next_acc=next_acc.numpy(), next_value=next_value.numpy(), next_done=next_done.numpy(),
               pref=pref.numpy(), advantages=ag.advantages.numpy(),
               returns=ag.returns.numpy())
    save_npz(os.path.join(HERE, f"nlppo_update_{kind}.npz"), out)


def trace_run(ref, logit_scale):
    """One seeded train() of the reference; returns (learner, vector env, eval env, result, per-iteration parameters, u inputs)."""
    Tr = nc.TRACE
    seed = Tr["seed"]
    env = nlppo_env.DiscreteLinearVecEnv(num_envs=Tr["num_envs"], **Tr["env"])
    eval_env = nlppo_env.DiscreteLinearEnv(**Tr["env"])
    nc.reseed(seed)
    ag = ref.NLMOPPO(0, env, log=False, device="cpu", seed=seed, **Tr["agent"])
    if logit_scale != 1.0:
        ag.agent.actor.register_forward_hook(lambda mod, inp, outp: outp * logit_scale)
    init = flat(ag.agent)
    evaluate = ag.policy_evaluate
    ag.policy_evaluate = lambda e, deterministic=False: evaluate(e, eval_episodes=Tr["eval_episodes"], deterministic=deterministic)
    params, seen_v, weights = [], [], []
    inner_update = ag.update

    def update():
        weights.append(ag._compute_loss_weights().numpy().copy())
        seen_v.pop()                               # (the extra evaluation above is not one of update()'s)
        r = inner_update()
        params.append(flat(ag.agent))
        return r

    ag.update = update
    u = nc.utility(Tr["referent"], Tr["scale"])
    nc.reseed(seed + 1)
    result = ag.train(eval_env, recording(u, seen_v), pref=np.asarray(Tr["referent"], dtype=np.float32), deterministic=True)
    return types.SimpleNamespace(ag=ag, env=env, eval_env=eval_env, result=result, params=params, seen_v=seen_v, weights=weights, init=init, u=u)


def trace_case(ref):
    Tr = nc.TRACE
    seed = Tr["seed"]
    base = trace_run(ref, 1.0)
    check_min_terms("nlppo_trace", base.u, base.seen_v)
    for s in (1.0 + 1e-4, 1.0 - 1e-4):
        other = trace_run(ref, s)
        assert np.array_equal(np.stack(base.env.action_log), np.stack(other.env.action_log)), \
            f"a sampled action changes when the logits are scaled by {s}; pick another seed"
        assert base.eval_env.action_log == other.eval_env.action_log, f"a greedy action changes when the logits are scaled by {s}"
    # the oracle's replay
    env = nlppo_env.DiscreteLinearVecEnv(num_envs=Tr["num_envs"], **Tr["env"])
    eval_env = nlppo_env.DiscreteLinearEnv(**Tr["env"])
    nc.reseed(seed)
    oa = no.Learner(env, seed=seed, **Tr["agent"])
    assert np.array_equal(base.init, flat(oa.agent))
    evaluate = oa.policy_evaluate
    oa.policy_evaluate = lambda e, deterministic=False: evaluate(e, eval_episodes=Tr["eval_episodes"], deterministic=deterministic)
    o_params = []
    nc.reseed(seed + 1)
    o_result = oa.train(eval_env, base.u, pref=np.asarray(Tr["referent"], dtype=np.float32), deterministic=True,
                        after_iteration=lambda it: o_params.append(flat(oa.agent)))
    for a, b in zip(base.params, o_params):
        assert np.array_equal(a, b), "oracle training differs from the reference"
    assert np.array_equal(np.stack(base.env.action_log), np.stack(env.action_log))
    assert np.array_equal(base.result, o_result)
    assert np.array_equal(np.stack(base.weights), np.stack(oa.weights_log))
    out = {"init": base.init, "actions": np.stack(base.env.action_log).astype(np.int32), "rewards": np.stack(base.env.reward_log),
           "eval_actions": np.asarray(base.eval_env.action_log, dtype=np.int32), "result": np.asarray(base.result, dtype=np.float64),
           "weights": np.stack(base.weights), "lr": np.asarray(oa.lr_log, dtype=np.float64), "global_step": np.asarray(oa.global_step),
           "steps": np.asarray([len(s) for s in oa.stats]), "stats": np.concatenate(oa.stats)}
    for it, p in enumerate(base.params, 1):
        out[f"params_{it}"] = p
    save_npz(os.path.join(HERE, "nlppo_trace.npz"), out)
    print(f"nlppo_trace: {out['actions'].shape[0]} vector steps, optimiser steps per iteration {out['steps']}, loss weights "
          f"{out['weights'].tolist()}, result {out['result']}")


def main():
    if not rh.reference_available():
        raise RuntimeError("reference tree not found")
    ref = import_reference()
    th.set_num_threads(1)
    only = set(sys.argv[1:])                      # e.g. "update trace": those fixtures alone (while looking for a seed)
    want = lambda name: not only or name in only  # noqa: E731
    for c in nc.STEP_CASES:
        if want(c.name):
            step_case(ref, c)
    if want("gae"):
        gae_case(ref)
    for kind, target_kl in nc.UPDATE_KINDS.items():
        if want("update"):
            update_case(ref, kind, target_kl)
    if want("trace"):
        trace_case(ref)
    largest = max(os.path.getsize(os.path.join(HERE, f)) for f in os.listdir(HERE) if f.startswith("ppo_") and f.endswith(".npz"))
    for f in sorted(os.listdir(HERE)):
        if f.startswith("nlppo_") and f.endswith(".npz"):
            size = os.path.getsize(os.path.join(HERE, f))
            assert size <= largest, f"{f}: {size} bytes, the largest ppo_*.npz is {largest}"


if __name__ == "__main__":
    main()
