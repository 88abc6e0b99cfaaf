"""PCN fixtures from the UNMODIFIED reference class (multi_policy/pcn/pcn.py), CPU:

* pcn_<case>.npz        one update() at a non-zero Adam step count: transition table, picked rows, loss, prediction, parameters
                        and moments before and after
* pcn_loop50.npz        50 back-to-back updates on a replay of random TreasureLine episodes
* pcn_trace_<kind>.npz  a seeded train() on tests/momdp.py: parameters, action stream, commands, final heap, acting log-probs

Every agent is constructed after an explicit reseed of torch, numpy and random; the archives are written with fixed zip
timestamps, so two runs give identical bytes.  The restatement in tests/pcn_oracle.py is checked against every recorded value on
the way (exact equality), and each trace's action stream is re-derived with it in float32 and with float64 evaluation of the
acting forward pass: a seed whose actions depend on accumulation order is refused here, before anything is committed.

    PYTHONDONTWRITEBYTECODE=1 python -B tests/golden/make_golden_pcn.py
"""
from __future__ import annotations

import copy
import io
import os
import sys
import tempfile
import zipfile

import numpy as np
import torch as th

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import ref_harness as rh  # noqa: E402
import pcn_cases as pc  # noqa: E402
import pcn_oracle as po  # noqa: E402


def save_npz(path, arrays):
    """np.savez with fixed member timestamps (np.savez stamps the wall clock into the archive)."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def trainable(agent):
    return [p for n, p in agent.model.named_parameters() if n != "scaling_factor"]


def params_np(agent):
    return [p.detach().numpy().copy() for p in trainable(agent)]


def dump(out, prefix, arrs):
    for i, a in enumerate(arrs):
        out[f"{prefix}_{i}"] = np.asarray(a)


def same(a, b):
    return all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(a, b))


def update_case(ref, c: pc.PCNCase):
    pc.reseed(c.seed)
    env = rh.FakeEnv(obs_dim=c.D, n_actions=c.A, reward_dim=c.R, act_dim=(c.A if c.continuous else None))
    scaling = pc.scaling_of(c)
    ag = ref.PCN(env, scaling, learning_rate=c.lr, batch_size=c.B, hidden_dim=c.H, log=False, seed=c.seed, device="cpu")
    assert ag.continuous_action == c.continuous
    # the oracle's seeded construction draws the same initial parameters
    pc.reseed(c.seed)
    init = po.init_params(c.D, c.R, c.A, c.H)
    assert same(init, params_np(ag)), "initial parameters differ from the reference's"
    m0, v0 = pc.synthetic_moments(c, [tuple(p.shape) for p in init])
    for p, m, v in zip(trainable(ag), m0, v0):
        ag.opt.state[p] = {"step": th.tensor(float(c.step)), "exp_avg": m.clone(), "exp_avg_sq": v.clone()}
    step = 0
    for ep in pc.synthetic_episodes(c):
        step += len(ep)
        ag._add_episode([ref.Transition(o, a, r.copy(), o, False) for o, a, r in ep], max_size=100, step=step)
    out = {}
    dump(out, "p0", params_np(ag))
    dump(out, "m0", m0)
    dump(out, "v0", v0)
    table, starts = po.flatten_replay(ag.experience_replay, c.D, c.R, c.A if c.continuous else 1)
    picks = po.draw_batch(ag.experience_replay, copy.deepcopy(ag.np_random), c.B)
    out["table"], out["starts"] = table, starts
    out["idx"] = np.asarray([starts[i] + t for i, t in picks], dtype=np.int32)
    out["scaling"] = scaling

    learner = po.Learner(init, scaling, c.continuous, lr=c.lr, exp_avg=m0, exp_avg_sq=v0, step=c.step)
    rng = copy.deepcopy(ag.np_random)
    o_loss, o_pred, o_picks = po.update_loop(learner, copy.deepcopy(ag.experience_replay), rng, c.B, 1)

    loss, pred = ag.update()
    out["loss"] = loss.detach().numpy()
    out["pred"] = pred.detach().numpy()
    dump(out, "p1", params_np(ag))
    dump(out, "m1", [ag.opt.state[p]["exp_avg"].numpy() for p in trainable(ag)])
    dump(out, "v1", [ag.opt.state[p]["exp_avg_sq"].numpy() for p in trainable(ag)])
    out["rng_after"] = np.asarray(ag.np_random.bit_generator.state["state"]["state"]).astype(str)

    assert o_picks[0] == picks
    assert np.array_equal(o_loss[0].numpy(), out["loss"]) and np.array_equal(o_pred.numpy(), out["pred"]), c.name
    assert same([p.detach().numpy() for p in learner.params], params_np(ag)), c.name
    assert str(rng.bit_generator.state["state"]["state"]) == str(out["rng_after"])
    save_npz(os.path.join(HERE, f"pcn_{c.name}.npz"), out)
    print(f"pcn_{c.name}: loss {float(loss.detach()):.6f}")


def make_env(kind, seed, stub_spaces):
    import momdp
    env = getattr(momdp, kind)(seed)
    if kind == "PointReach" and stub_spaces:
        # the reference tells a continuous action space by ``type(space) is gym.spaces.Box`` (pcn.py:166): give it the stand-in's
        # own class, drawing the stream momdp.BoxSpace(seed) draws
        box = sys.modules["gymnasium.spaces"].Box(-1.0, 1.0, (1,))
        box._rng = np.random.default_rng(seed)
        env.action_space = box
    return env


def loop_case(ref):
    L = pc.LOOP
    pc.reseed(L["seed"])
    env = make_env("TreasureLine", L["seed"], True)
    ag = ref.PCN(env, L["scaling"], learning_rate=L["lr"], batch_size=L["B"], hidden_dim=L["H"], log=False, seed=L["seed"],
                 device="cpu")
    step = 0
    for _ in range(L["episodes"]):
        transitions, done = [], False
        obs, _ = env.reset()
        while not done:
            action = env.action_space.sample()
            n_obs, reward, terminated, truncated, _ = env.step(action)
            transitions.append(ref.Transition(obs, action, np.float32(reward).copy(), n_obs, terminated))
            done, obs, step = terminated or truncated, n_obs, step + 1
        ag._add_episode(transitions, max_size=100, step=step)
    out = {}
    dump(out, "p0", params_np(ag))
    table, starts = po.flatten_replay(ag.experience_replay, 9, 2, 1)
    out["table"], out["starts"], out["scaling"] = table, starts, L["scaling"]
    learner = po.Learner([th.tensor(p) for p in params_np(ag)], L["scaling"], False, lr=L["lr"])
    o_losses, o_pred, picks = po.update_loop(learner, copy.deepcopy(ag.experience_replay), copy.deepcopy(ag.np_random), L["B"],
                                             L["n"])
    out["idx"] = np.asarray([[starts[i] + t for i, t in step_picks] for step_picks in picks], dtype=np.int32)
    losses = []
    for _ in range(L["n"]):
        l, pred = ag.update()
        losses.append(l.detach().numpy())
    out["losses"] = np.asarray(losses)
    out["pred"] = pred.detach().numpy()
    dump(out, "p1", params_np(ag))
    assert np.array_equal(o_losses.numpy(), out["losses"]) and np.array_equal(o_pred.numpy(), out["pred"])
    assert same([p.detach().numpy() for p in learner.params], params_np(ag))
    save_npz(os.path.join(HERE, "pcn_loop50.npz"), out)
    print(f"pcn_loop50: loss {losses[0]:.5f} -> {losses[-1]:.5f}")


def trace_case(ref, kind):
    T = pc.TRACES[kind]
    seed = T["seed"]
    pc.reseed(seed)
    env, eval_env = make_env(T["env"], seed, True), make_env(T["env"], seed + 1, True)
    ag = ref.PCN(env, T["scaling"], log=False, seed=seed, device="cpu", **T["agent"])
    out = {}
    dump(out, "init", params_np(ag))
    logps, commands, state = [], [], {"eval": False}
    choose, evaluate, act = ag._choose_commands, ag.evaluate, ag._act

    def act_logged(obs, desired_return, desired_horizon, eval_mode=False):
        if not state["eval"]:      # the model's output at this acting step (pcn.py:303-307), evaluated once more: no RNG involved
            with th.no_grad():
                logps.append(ag.model(th.tensor(np.array([obs])).float(), th.tensor(np.array([desired_return])).float(),
                                      th.tensor(np.array([desired_horizon])).unsqueeze(1).float()).numpy()[0].copy())
        return act(obs, desired_return, desired_horizon, eval_mode)

    def choose_logged(n):
        r, h = choose(n)
        commands.append((r.copy(), np.float32(h)))
        return r, h

    def evaluate_flagged(*a, **k):
        state["eval"] = True
        try:
            return evaluate(*a, **k)
        finally:
            state["eval"] = False

    ag._choose_commands, ag.evaluate, ag._act = choose_logged, evaluate_flagged, act_logged
    pc.reseed(seed + 1)
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:       # train() checkpoints with self.save() into ./weights
        os.chdir(tmp)
        try:
            ag.train(eval_env=eval_env, ref_point=np.zeros(2), **{k: (v.copy() if isinstance(v, np.ndarray) else v)
                                                                  for k, v in T["train"].items()})
        finally:
            os.chdir(cwd)
    dump(out, "final", params_np(ag))
    actions = np.asarray(env.action_log, dtype=np.int8) if kind == "discrete" else np.asarray(env.action_log, dtype=np.float32)
    out["actions"] = actions
    out["eval_actions"] = (np.asarray(eval_env.action_log, dtype=np.int8) if kind == "discrete"
                           else np.asarray(eval_env.action_log, dtype=np.float32))
    out["command_returns"] = np.stack([c[0] for c in commands])
    out["command_horizons"] = np.asarray([c[1] for c in commands], dtype=np.float32)
    out["heap_distance"], out["heap_step"], out["heap_return"], out["heap_length"] = po.heap_summary(ag.experience_replay)
    out["logps"] = np.stack(logps)
    out["global_step"] = np.asarray(ag.global_step)
    assert len(commands) >= 3, "a trace covers at least three training iterations"

    # the restatement alone: float32 as the reference computes it, and with the acting forward pass evaluated in float64
    robust = {}
    for tag, dtype in (("f32", None), ("f64", th.float64)):
        pc.reseed(seed)
        o_env = make_env(T["env"], seed, False)
        oa = po.Agent(o_env, T["scaling"], seed=seed, act_dtype=dtype, **T["agent"])
        pc.reseed(seed + 1)
        tr = {k: v for k, v in T["train"].items()}
        oa.train(eval_env=make_env(T["env"], seed + 1, False), **tr)
        got = np.asarray(o_env.action_log)
        if kind == "discrete" or dtype is None:
            ok = got.shape == actions.shape and np.array_equal(got.astype(actions.dtype), actions)
        else:    # continuous actions are the network's fp32 outputs: float64 evaluation moves them by rounding, never by more
            ok = got.shape == actions.shape and float(np.abs(got - actions).max()) <= 5e-5
        ok = ok and [len(e[2]) for e in oa.replay] == list(out["heap_length"]) and [e[1] for e in oa.replay] == list(out["heap_step"])
        robust[tag] = ok
        if dtype is None:
            assert same([p.detach().numpy() for p in oa.learner.params], params_np(ag)), "oracle training differs from the reference"
            assert np.array_equal(np.stack(oa.logps), out["logps"])
    assert robust["f32"] and robust["f64"], f"{kind}: seed {seed} is not robust to accumulation order ({robust}); pick another"
    out["robust_f32_f64"] = np.asarray([robust["f32"], robust["f64"]])
    save_npz(os.path.join(HERE, f"pcn_trace_{kind}.npz"), out)
    print(f"pcn_trace_{kind}: {int(ag.global_step)} steps, {len(commands)} iterations, {len(logps)} acting steps, robust {robust}")


def main():
    rh.install_stubs()
    if not rh.reference_available():
        raise RuntimeError("reference tree not found")
    from morl_baselines.multi_policy.pcn import pcn as ref
    th.set_num_threads(1)
    for c in pc.UPDATE_CASES:
        update_case(ref, c)
    loop_case(ref)
    for kind in pc.TRACES:
        trace_case(ref, kind)


if __name__ == "__main__":
    main()
