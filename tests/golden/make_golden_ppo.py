"""MO-PPO fixtures from the UNMODIFIED reference class (single_policy/ser/mo_ppo.py), CPU:

* ppo_<case>.npz          one minibatch step at a non-zero Adam step count: the rollout rows, the visiting order, the step's
                          statistics, parameters before and after, moments after (the ones before are
                          ppo_cases.synthetic_moments), and a seeded get_action_and_value on the rows
* ppo_gae.npz             __compute_advantages with gae on and off
* ppo_update_<kind>.npz   a whole update(): 3 epochs x 4 minibatches, to the end and stopped by target_kl after the second epoch
* ppo_trace.npz           a seeded train() of two iterations on tests/ppo_env.py

The reference's statistics are read from what update() hands to ``wandb.log`` (the harness's stand-in is replaced by a recorder).
The restatement in tests/ppo_oracle.py is checked against every recorded value on the way (exact equality).  A seed that breaks one
of the conditions below is refused before anything is written:

* single steps a to c: at least 10 % of the rows have the ratio clipped and at least 10 % unclipped (and the same for the value
  clip where it is on); the gradient norm is above max_grad_norm in a to c and below it in d
* every recorded step: no row within 1e-4 of a clip boundary, evaluated in float32 and in float64
* target_kl: every epoch-end approx_kl is at least 10 % away from it

    PYTHONDONTWRITEBYTECODE=1 python -B tests/golden/make_golden_ppo.py
"""
from __future__ import annotations

import copy
import os
import sys
import time
import types

import numpy as np
import torch as th

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import ref_harness as rh  # noqa: E402
import ppo_cases as pc  # noqa: E402
import ppo_env  # noqa: E402
import ppo_oracle as po  # noqa: E402
from make_golden_pcn import save_npz  # noqa: E402

MARGIN = 1e-4
LOGGED = []


def import_reference():
    rh.install_stubs()
    # two names mo_ppo.py needs at import that the harness's stand-ins lack
    sys.modules["mo_gymnasium.wrappers"].MORecordEpisodeStatistics = type("MORecordEpisodeStatistics", (), {})
    vector = types.ModuleType("gymnasium.vector")
    vector.SyncVectorEnv = type("SyncVectorEnv", (), {})
    sys.modules["gymnasium.vector"] = vector
    sys.modules["gymnasium"].vector = vector
    sys.modules["wandb"].log = lambda d, *a, **k: LOGGED.append(dict(d))
    from morl_baselines.single_policy.ser import mo_ppo as ref
    return ref


def flat(net):
    return np.concatenate([p.detach().numpy().reshape(-1) for p in net.parameters()]).copy()


def seeded_nets(ref, seed, D, A, R, hidden):
    pc.reseed(seed)
    net = ref.MOPPONet((D,), (A,), R, list(hidden))
    pc.reseed(seed)
    onet = po.Net(D, A, R, list(hidden))
    assert [n for n, _ in net.named_parameters()] == [n for n, _ in onet.named_parameters()]
    assert np.array_equal(flat(net), flat(onet)), "the oracle's seeded construction differs from the reference's"
    return net, onet


def perturbed(net, seed, size):
    g = th.Generator().manual_seed(seed)
    old = copy.deepcopy(net)
    with th.no_grad():
        for p in old.parameters():
            p.add_(size * th.randn(p.shape, generator=g))
    return old


def synthetic_rollout(net, seed, T, E, perturb, obs_scale=1.0, done_rate=0.1):
    """obs, and actions / log-probs / values of a PERTURBED copy of ``net`` (the behaviour policy), rewards, dones."""
    D, A, R = net.obs_shape[0], net.action_shape[0], net.reward_dim
    g = th.Generator().manual_seed(seed + 1000)
    old = perturbed(net, seed + 1001, perturb)
    obs = obs_scale * th.randn(T * E, D, generator=g)
    with th.no_grad():
        noise = th.randn(T * E, A, generator=g)
        actions = old.actor_mean(obs) + th.exp(old.actor_logstd) * noise
        _, logprobs, _, values = old.get_action_and_value(obs, actions)
    rewards = th.randn(T * E, R, generator=g)
    dones = (th.rand(T * E, generator=g) < done_rate).float()
    return dict(obs=obs.view(T, E, D), actions=actions.view(T, E, A), logprobs=logprobs.view(T, E), rewards=rewards.view(T, E, R),
                dones=dones.view(T, E), values=values.view(T, E, R)), g


def fill(ag, roll):
    for k, v in roll.items():
        getattr(ag.batch, k).copy_(v)


def margins(c, ratio, newvalue, oldv, clip_vloss):
    r = ratio.double().numpy()
    m = min(np.abs(r - (1 - c)).min(), np.abs(r - (1 + c)).min())
    if clip_vloss:
        m = min(m, np.abs(np.abs(newvalue.double().numpy() - oldv.double().numpy()) - c).min())
    return float(m)


def batch_of(roll, returns, advantages, dtype=None):
    T, E = roll["logprobs"].shape
    R = roll["values"].shape[-1]
    b = (roll["obs"].reshape(T * E, -1), roll["actions"].reshape(T * E, -1), roll["logprobs"].reshape(-1),
         advantages.reshape(-1), returns.reshape(-1, R), roll["values"].reshape(-1, R))
    return tuple(x.to(dtype) for x in b) if dtype is not None else b


def check_margins(name, onet0, cfg, batch, idx, clip_vloss, f32_seen):
    """No row of any recorded step within MARGIN of a clip boundary -- float32 (as recorded) and float64 (the same steps in double)."""
    worst = min(f32_seen)
    net64 = po.to_dtype(onet0, th.float64)
    opt64 = th.optim.Adam(net64.parameters(), lr=cfg.lr, eps=1e-5)
    b64 = tuple(x.double() for x in batch)
    for mb in idx:
        _, ratio, nv = po.minibatch_step(net64, opt64, cfg, *b64, mb.astype(np.int64))
        worst = min(worst, margins(cfg.clip_coef, ratio, nv, b64[5][mb.astype(np.int64)], clip_vloss))
    assert worst >= MARGIN, f"{name}: a row lies {worst:.2e} from a clip boundary; pick another seed"
    return worst


def step_case(ref, c: pc.StepCase):
    net, onet = seeded_nets(ref, c.seed, c.D, c.A, c.R, c.hidden)
    out = {}
    with th.no_grad():
        net.actor_logstd.fill_(c.logstd)
    roll, g = synthetic_rollout(net, c.seed, c.M, 1, c.perturb, c.obs_scale)
    # returns and advantages as a rollout of M steps of one env gives them with gamma = 0 and no GAE: returns = rewards,
    # advantages = (returns - values) @ weights -- what a test reproduces through morl_ppo_set_rollout + morl_ppo_gae
    roll["rewards"] = roll["values"] + c.ret_scale * th.randn(c.M, 1, c.R, generator=g)
    roll["dones"] = th.zeros(c.M, 1)
    weights = np.full(c.R, 1.0 / c.R, dtype=np.float32)
    p0 = flat(net)
    m0, v0 = pc.synthetic_moments(c.seed, len(p0))
    po.load_flat(onet, p0)

    # a seeded get_action_and_value on the rows, before the step
    obs = roll["obs"].reshape(c.M, c.D)
    pc.reseed(c.seed + 7)
    with th.no_grad():
        f_action, f_logprob, _, f_value = net.get_action_and_value(obs)
    pc.reseed(c.seed + 7)
    eps = th.normal(th.zeros(c.M, c.A), th.ones(c.M, c.A))
    with th.no_grad():
        assert th.equal(onet.actor_mean(obs) + th.exp(onet.actor_logstd) * eps, f_action), "noise stream differs from Normal.sample()"
    out.update(fwd_eps=eps.numpy(), fwd_action=f_action.numpy(), fwd_logprob=f_logprob.numpy(), fwd_value=f_value.numpy())

    envs = types.SimpleNamespace(num_envs=1)
    ag = ref.MOPPO(0, net, weights, envs, log=True, steps_per_iteration=c.M, num_minibatches=1, update_epochs=1, gamma=0.0,
                   gae=False, learning_rate=c.lr, clip_coef=c.clip_coef, ent_coef=c.ent_coef, vf_coef=c.vf_coef,
                   clip_vloss=c.clip_vloss, max_grad_norm=c.max_grad_norm, norm_adv=c.norm_adv, device="cpu", seed=c.seed)
    fill(ag, roll)
    returns, advantages = ag._MOPPO__compute_advantages(th.zeros(1, c.D), th.zeros(1))
    assert th.equal(returns, roll["rewards"])
    ag.returns, ag.advantages = returns, advantages
    po.set_adam_state(ag.optimizer, net, m0, v0, c.step)

    cfg = po.Cfg(c.clip_coef, c.ent_coef, c.vf_coef, c.clip_vloss, c.max_grad_norm, c.norm_adv)
    cfg.lr = c.lr
    onet0 = copy.deepcopy(onet)
    opt = th.optim.Adam(onet.parameters(), lr=c.lr, eps=1e-5)
    po.set_adam_state(opt, onet, m0, v0, c.step)
    batch = batch_of(roll, returns, advantages)
    seen, rows = [], {}

    def observer(ratio, newvalue, mb):
        seen.append(margins(c.clip_coef, ratio, newvalue, batch[5][mb], c.clip_vloss))
        rows["ratio"], rows["dv"] = ratio.numpy(), (newvalue - batch[5][mb]).numpy()

    stats, idx = po.update(onet, opt, cfg, copy.deepcopy(ag.np_random), batch, 1, 1, observer=observer)

    LOGGED.clear()
    ag.update()
    log = LOGGED[-1]
    got = [log[f"losses_0/{k}"] for k in ("policy_loss", "value_loss", "entropy", "old_approx_kl", "approx_kl", "clipfrac")]
    assert np.array_equal(np.asarray(got, dtype=np.float32), stats[0][[1, 2, 3, 4, 5, 6]]), (c.name, got, stats[0])
    assert np.array_equal(flat(net), flat(onet)), c.name
    m1, v1 = po.adam_flat(ag.optimizer, net)
    om1, ov1 = po.adam_flat(opt, onet)
    assert np.array_equal(m1, om1) and np.array_equal(v1, ov1), c.name

    rclip = float((np.abs(rows["ratio"] - 1.0) > c.clip_coef).mean())
    vclip = float((np.abs(rows["dv"]) > c.clip_coef).mean())
    worst = check_margins(c.name, onet0, cfg, batch, idx, c.clip_vloss, seen)
    print(f"ppo_{c.name}: loss {stats[0][0]:.5f} grad norm {stats[0][7]:.4f} ratio clipped {rclip:.2f} value clipped {vclip:.2f} "
          f"margin {worst:.2e}")
    if c.clip_active:
        assert 0.1 <= rclip <= 0.9, f"{c.name}: {rclip:.2f} of the rows have the ratio clipped"
        assert not c.clip_vloss or 0.1 <= vclip <= 0.9, f"{c.name}: {vclip:.2f} of the values are clipped"
        assert stats[0][7] > c.max_grad_norm, f"{c.name}: gradient norm {stats[0][7]} does not reach the clip"
    else:
        assert stats[0][7] < c.max_grad_norm, f"{c.name}: gradient norm {stats[0][7]} is clipped"
    out.update(p0=p0, p1=flat(net), m1=m1, v1=v1, stats=stats[0], idx=idx[0], obs=batch[0].numpy(),
               actions=batch[1].numpy(), logprobs=batch[2].numpy(), advantages=batch[3].numpy(), returns=batch[4].numpy(),
               values=batch[5].numpy(), weights=weights)
    save_npz(os.path.join(HERE, f"ppo_{c.name}.npz"), out)


def gae_case(ref):
    G = pc.GAE
    T, E, R = G["T"], G["E"], G["R"]
    net, onet = seeded_nets(ref, G["seed"], G["D"], G["A"], R, G["hidden"])
    roll, g = synthetic_rollout(net, G["seed"], T, E, 0.1, done_rate=G["done_rate"])
    next_obs = th.randn(E, G["D"], generator=g)
    next_done = th.tensor([0.0, 1.0, 0.0, 0.0])
    weights = np.array([0.3, 0.7], dtype=np.float32)
    out = {k: v.numpy() for k, v in roll.items() if k in ("rewards", "dones", "values")}
    with th.no_grad():
        next_value = net.get_value(next_obs).reshape(E, -1)
    out.update(next_obs=next_obs.numpy(), next_value=next_value.numpy(), next_done=next_done.numpy(), weights=weights)
    assert 0.04 < float(roll["dones"].mean()) < 0.2
    for use_gae in (True, False):
        ag = ref.MOPPO(0, net, weights, types.SimpleNamespace(num_envs=E), log=False, steps_per_iteration=T, gamma=G["gamma"],
                       gae=use_gae, gae_lambda=G["gae_lambda"], device="cpu", seed=G["seed"])
        fill(ag, roll)
        returns, adv = ag._MOPPO__compute_advantages(next_obs, next_done)
        o_ret, o_adv = po.compute_advantages(roll["rewards"], roll["dones"], roll["values"], next_value, next_done,
                                             th.from_numpy(weights), G["gamma"], G["gae_lambda"], use_gae)
        assert th.equal(returns, o_ret) and th.equal(adv, o_adv)
        tag = "gae" if use_gae else "mc"
        out[f"returns_{tag}"], out[f"advantages_{tag}"] = returns.numpy(), adv.numpy()
    save_npz(os.path.join(HERE, "ppo_gae.npz"), out)
    print("ppo_gae: done fraction", float(roll["dones"].mean()))


def update_case(ref, kind, target_kl):
    U = pc.UPDATE
    T, E, R = U["T"], U["E"], U["R"]
    net, onet = seeded_nets(ref, U["seed"], U["D"], U["A"], R, U["hidden"])
    roll, g = synthetic_rollout(net, U["seed"], T, E, U["perturb"])
    next_obs, next_done = th.randn(E, U["D"], generator=g), th.zeros(E)
    weights = np.array([0.6, 0.4], dtype=np.float32)
    ag = ref.MOPPO(0, net, weights, types.SimpleNamespace(num_envs=E), log=True, steps_per_iteration=T,
                   num_minibatches=U["num_minibatches"], update_epochs=U["update_epochs"], learning_rate=U["lr"], gamma=U["gamma"],
                   gae_lambda=U["gae_lambda"], target_kl=target_kl, device="cpu", seed=U["seed"])
    fill(ag, roll)
    with th.no_grad():
        next_value = net.get_value(next_obs).reshape(E, -1)
    ag.returns, ag.advantages = ag._MOPPO__compute_advantages(next_obs, next_done)
    out = {k: v.numpy() for k, v in roll.items()}
    out.update(next_obs=next_obs.numpy(), next_value=next_value.numpy(), next_done=next_done.numpy(), weights=weights,
               returns=ag.returns.numpy(),
               advantages=ag.advantages.numpy(), p0=flat(net))
    cfg = po.Cfg()
    cfg.lr = U["lr"]
    onet0 = copy.deepcopy(onet)
    opt = th.optim.Adam(onet.parameters(), lr=U["lr"], eps=1e-5)
    batch = batch_of(roll, ag.returns, ag.advantages)
    seen = []
    stats, idx = po.update(onet, opt, cfg, copy.deepcopy(ag.np_random), batch, U["num_minibatches"], U["update_epochs"], target_kl,
                           observer=lambda ratio, nv, mb: seen.append(margins(cfg.clip_coef, ratio, nv, batch[5][mb], True)))
    LOGGED.clear()
    ag.update()
    log = LOGGED[-1]
    got = [log[f"losses_0/{k}"] for k in ("policy_loss", "value_loss", "entropy", "old_approx_kl", "approx_kl")]
    assert np.array_equal(np.asarray(got, dtype=np.float32), stats[-1][[1, 2, 3, 4, 5]]), (kind, got, stats[-1])
    assert np.float32(log["losses_0/clipfrac"]) == np.float32(np.mean(stats[:, 6].astype(np.float64)))
    assert np.array_equal(flat(net), flat(onet)), kind
    m1, v1 = po.adam_flat(ag.optimizer, net)
    om1, ov1 = po.adam_flat(opt, onet)
    assert np.array_equal(m1, om1) and np.array_equal(v1, ov1), kind
    per_epoch = U["num_minibatches"]
    kls = stats[per_epoch - 1::per_epoch, 5]
    worst = check_margins(f"update_{kind}", onet0, cfg, batch, idx, True, seen)
    print(f"ppo_update_{kind}: {len(stats)} steps, epoch-end approx_kl {kls}, margin {worst:.2e}")
    if target_kl is None:
        assert len(stats) == U["update_epochs"] * per_epoch
    else:
        assert len(stats) == 2 * per_epoch, f"target_kl {target_kl} stops after {len(stats)} steps, not after the second epoch"
        assert all(abs(float(k) - target_kl) >= 0.1 * target_kl for k in kls), (kls, target_kl)
    out.update(p1=flat(net), m1=m1, v1=v1, stats=stats, idx=idx, adam_steps=np.asarray(len(stats)))
    save_npz(os.path.join(HERE, f"ppo_update_{kind}.npz"), out)


def trace_case(ref):
    Tr = pc.TRACE
    seed, e = Tr["seed"], Tr["env"]
    net, onet = seeded_nets(ref, seed, e["obs_dim"], e["action_dim"], e["reward_dim"], Tr["hidden"])
    env, o_env = ppo_env.LinearVecEnv(**e), ppo_env.LinearVecEnv(**e)
    ag = ref.MOPPO(0, net, Tr["weights"].copy(), env, log=False, device="cpu", seed=seed, **Tr["agent"])
    oa = po.Agent(onet, Tr["weights"].copy(), o_env, seed=seed, **Tr["agent"])
    out = {"init": flat(net)}
    pc.reseed(seed + 1)
    for it in range(1, Tr["iterations"] + 1):
        ag.train(time.time(), it, Tr["iterations"])
        out[f"params_{it}"] = flat(net)
    pc.reseed(seed + 1)
    for it in range(1, Tr["iterations"] + 1):
        oa.train(it, Tr["iterations"])
        assert np.array_equal(out[f"params_{it}"], flat(onet)), "oracle training differs from the reference"
    out["actions"], out["rewards"] = np.stack(env.action_log), np.stack(env.reward_log)
    assert np.array_equal(out["actions"], np.stack(o_env.action_log))
    out["global_step"] = np.asarray(ag.global_step)
    out["steps"] = np.asarray([len(s) for s in oa.stats])
    out["stats"] = np.concatenate(oa.stats)
    save_npz(os.path.join(HERE, "ppo_trace.npz"), out)
    print(f"ppo_trace: {out['actions'].shape[0]} vector steps, optimiser steps per iteration {out['steps']}")


def main():
    if not rh.reference_available():
        raise RuntimeError("reference tree not found")
    ref = import_reference()
    th.set_num_threads(1)
    for c in pc.STEP_CASES:
        step_case(ref, c)
    gae_case(ref)
    for kind, target_kl in pc.UPDATE_KINDS.items():
        update_case(ref, kind, target_kl)
    trace_case(ref)


if __name__ == "__main__":
    main()
