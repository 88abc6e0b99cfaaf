"""LCN fixtures from the UNMODIFIED reference class (multi_policy/lcn/lcn.py), CPU:

* lcn_select_<case>.npz   one _nlargest() of the reference on a heap with the given returns: returns, threshold, mode, lambda;
                          the reference's l2 (the heap keys it wrote), its np.argsort order, and the front mask recomputed with the
                          reference's own lorenz_vector / get_non_dominated_inds
* lcn_commands.npz        _choose_commands() on a fixed heap in both modes: commands, heap afterwards, generator state
* lcn_trace_<kind>.npz    a seeded train() on tests/momdp.py: parameters, action stream, commands, final heap, acting log-probs

Every agent is constructed after an explicit reseed of torch, numpy and random; the archives are written with fixed zip
timestamps, so two runs give identical bytes.  The restatement in tests/lcn_oracle.py is checked against every recorded value on
the way (exact equality), and each trace's action stream is re-derived with it in float32 and with float64 evaluation of the
acting forward pass: a seed whose actions depend on accumulation order is refused here, before anything is committed.

    PYTHONDONTWRITEBYTECODE=1 python -B tests/golden/make_golden_lcn.py
"""
from __future__ import annotations

import copy
import os
import sys
import tempfile

import numpy as np
import torch as th

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import ref_harness as rh  # noqa: E402
import lcn_cases as lc  # noqa: E402
import lcn_oracle as lo  # noqa: E402
import pcn_oracle as po  # noqa: E402
from make_golden_pcn import dump, make_env, params_np, same, save_npz  # noqa: E402


def bare_agent(ref, R, distance_ref, lcn_lambda, seed=0):
    env = rh.FakeEnv(obs_dim=4, n_actions=3, reward_dim=R)
    return ref.LCN(env, np.full(R + 1, 0.1, dtype=np.float32), distance_ref=distance_ref, lcn_lambda=lcn_lambda, log=False,
                   seed=seed, device="cpu")


def select_case(ref, pareto, c: lc.SelectCase):
    returns = lc.select_returns(c.N, c.R, c.family, c.seed)
    ag = bare_agent(ref, c.R, c.distance_ref, c.lcn_lambda)
    obs = np.zeros(4, dtype=np.float32)
    ag.experience_replay = [(1, i, [ref.Transition(obs, 0, returns[i].copy(), obs, True)]) for i in range(c.N)]
    before = list(ag.experience_replay)
    largest = ag._nlargest(c.N, c.threshold)
    # _nlargest wrote l2[i] into slot i and heapified: recover l2 in the original order through the step field
    l2 = np.empty(c.N, dtype=np.float32)
    for key, step, _ in ag.experience_replay:
        assert isinstance(key, np.float32)
        l2[step] = key
    order = np.asarray([e[1] for e in largest], dtype=np.int64)          # sorted_i[-N:] = np.argsort(l2)
    assert np.array_equal(order, np.argsort(l2))
    mode = lc.MODE_OF[c.distance_ref]
    if mode == 2:
        s = np.sort(returns, axis=1)
        mask = pareto.get_non_dominated_inds(c.lcn_lambda * s + (1 - c.lcn_lambda) * ref.lorenz_vector(s))
    else:
        mask = pareto.get_non_dominated_inds(ref.lorenz_vector(returns))
    o_l2, o_mask, o_crowded = lo.score(returns, c.threshold, mode, c.lcn_lambda)
    assert o_l2.dtype == np.float32 and np.array_equal(o_l2.view(np.uint32), l2.view(np.uint32)), c.name
    assert np.array_equal(o_mask, mask), c.name
    replay = list(before)
    o_largest = lo.nlargest(replay, c.N, c.threshold, c.distance_ref, c.lcn_lambda)
    assert [e[1] for e in o_largest] == list(order) and [e[1] for e in replay] == [e[1] for e in ag.experience_replay]
    save_npz(os.path.join(HERE, f"lcn_select_{c.name}.npz"),
             dict(returns=returns, threshold=np.asarray(c.threshold), mode=np.asarray(mode),
                  lcn_lambda=np.asarray(np.nan if c.lcn_lambda is None else c.lcn_lambda), l2=l2, order=order,
                  mask=mask.astype(np.uint8), crowded=o_crowded))
    print(f"lcn_select_{c.name}: front {int(mask.sum())} of {c.N}, crowded {int(o_crowded.sum())}, "
          f"distinct keys {len(np.unique(l2))}")


def commands_case(ref):
    C = lc.COMMANDS
    out = {}
    for tag, v in C["variants"].items():
        ag = bare_agent(ref, C["R"], v["distance_ref"], v["lcn_lambda"], seed=C["seed"])
        ag.cd_threshold = C["cd_threshold"]
        replay, rng = [], copy.deepcopy(ag.np_random)
        step, cmds = 0, []
        for k, ep in enumerate(lc.command_episodes()):
            step += len(ep)
            ag._add_episode([ref.Transition(o, a, r.copy(), o, False) for o, a, r in ep], max_size=C["max_size"], step=step)
            po.add_episode(replay, [po.Transition(o, a, r.copy(), o, False) for o, a, r in ep], C["max_size"], step)
            if k % 8 == 7:
                got = ag._choose_commands(C["num_episodes"])
                want = lo.choose_commands(replay, rng, C["num_episodes"], C["cd_threshold"], v["distance_ref"], v["lcn_lambda"])
                assert np.array_equal(got[0], want[0]) and got[1] == want[1], tag
                cmds.append(got)
        for a, b in zip(po.heap_summary(ag.experience_replay), po.heap_summary(replay)):
            assert np.array_equal(a, b), tag
        assert ag.np_random.bit_generator.state == rng.bit_generator.state
        out[f"{tag}_returns"] = np.stack([c[0] for c in cmds])
        out[f"{tag}_horizons"] = np.asarray([c[1] for c in cmds], dtype=np.float32)
        (out[f"{tag}_heap_distance"], out[f"{tag}_heap_step"], out[f"{tag}_heap_return"],
         out[f"{tag}_heap_length"]) = po.heap_summary(ag.experience_replay)
        out[f"{tag}_rng_after"] = np.asarray(ag.np_random.bit_generator.state["state"]["state"]).astype(str)
    save_npz(os.path.join(HERE, "lcn_commands.npz"), out)
    print(f"lcn_commands: {len(cmds)} commands per mode")


def trace_case(ref, name, seed=None, write=True):
    T = lc.TRACES[name]
    seed = T["seed"] if seed is None else seed
    kind = T["kind"]
    lc.reseed(seed)
    env, eval_env = make_env(T["env"], seed, True), make_env(T["env"], seed + 1, True)
    ag = ref.LCN(env, T["scaling"], log=False, seed=seed, device="cpu", **T["agent"])
    out = {}
    dump(out, "init", params_np(ag))
    logps, commands, state = [], [], {"eval": False}
    choose, evaluate, act = ag._choose_commands, ag.evaluate, ag._act

    def act_logged(obs, desired_return, desired_horizon, eval_mode=False):
        if not state["eval"]:      # the model's output at this acting step (lcn.py:285-289), evaluated once more: no RNG involved
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
    lc.reseed(seed + 1)
    with tempfile.TemporaryDirectory() as tmp:       # train() checkpoints into save_dir
        ag.train(eval_env=eval_env, ref_point=np.zeros(2), save_dir=tmp,
                 **{k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in T["train"].items()})
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
    assert T["train"]["max_buffer_size"] < T["train"]["num_er_episodes"] + len(commands) * T["train"]["num_step_episodes"]

    # the restatement alone: float32 as the reference computes it, and with the acting forward pass evaluated in float64
    robust = {}
    for tag, dtype in (("f32", None), ("f64", th.float64)):
        lc.reseed(seed)
        o_env = make_env(T["env"], seed, False)
        oa = lo.Agent(o_env, T["scaling"], seed=seed, act_dtype=dtype, **T["agent"])
        lc.reseed(seed + 1)
        oa.train(eval_env=make_env(T["env"], seed + 1, False), **dict(T["train"]))
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
            assert np.array_equal(po.heap_summary(oa.replay)[0], out["heap_distance"])
    if not write:
        return robust["f32"] and robust["f64"]
    assert robust["f32"] and robust["f64"], f"{name}: seed {seed} is not robust to accumulation order ({robust}); pick another"
    out["robust_f32_f64"] = np.asarray([robust["f32"], robust["f64"]])
    save_npz(os.path.join(HERE, f"lcn_trace_{name}.npz"), out)
    print(f"lcn_trace_{name}: {int(ag.global_step)} steps, {len(commands)} iterations, {len(logps)} acting steps, robust {robust}")
    return True


def main():
    rh.install_stubs()
    if not rh.reference_available():
        raise RuntimeError("reference tree not found")
    from morl_baselines.common import pareto
    from morl_baselines.multi_policy.lcn import lcn as ref
    th.set_num_threads(1)
    if len(sys.argv) > 2 and sys.argv[1] == "--search":      # first seed of a trace configuration that passes the robustness check
        for seed in range(1, 60):
            try:
                ok = trace_case(ref, sys.argv[2], seed=seed, write=False)
            except AssertionError as e:
                ok = False
                print(seed, "assert", e)
            print(f"seed {seed}: {'robust' if ok else 'refused'}", flush=True)
            if ok:
                return
        return
    for c in lc.SELECT_CASES:
        select_case(ref, pareto, c)
    commands_case(ref)
    for name in lc.TRACES:
        trace_case(ref, name)


if __name__ == "__main__":
    main()
