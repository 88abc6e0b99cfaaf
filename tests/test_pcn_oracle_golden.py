"""tests/pcn_oracle.py is pinned to the fixtures recorded from the unmodified reference PCN: exact equality, CPU."""
import numpy as np
import pytest
import torch as th

import momdp
import pcn_cases as pc
import pcn_common as pcm
import pcn_oracle as po


def batch_of(g, idx, D, R, A, continuous):
    table = g["table"]
    aw = A if continuous else 1
    rows = table[idx]
    actions = th.tensor(rows[:, D:D + aw]) if continuous else th.tensor(rows[:, D].astype(np.int64))
    return (th.tensor(rows[:, :D]), actions, th.tensor(rows[:, D + aw:D + aw + R]), th.tensor(rows[:, -1]).unsqueeze(1))


def pieces(g, prefix):
    return [th.tensor(g[f"{prefix}_{i}"]) for i in range(8)]


@pytest.mark.parametrize("c", pc.UPDATE_CASES, ids=lambda c: c.name)
def test_single_update(c):
    th.set_num_threads(1)
    g = pcm.load(c.name)
    learner = po.Learner(pieces(g, "p0"), g["scaling"], c.continuous, lr=c.lr, exp_avg=pieces(g, "m0"),
                         exp_avg_sq=pieces(g, "v0"), step=c.step)
    loss, pred = learner.update(*batch_of(g, g["idx"], c.D, c.R, c.A, c.continuous))
    assert np.array_equal(loss.numpy().reshape(-1), g["loss"].reshape(-1))
    assert np.array_equal(pred.numpy(), g["pred"])
    m, v = learner.moments()
    for i in range(8):
        assert np.array_equal(learner.params[i].detach().numpy(), g[f"p1_{i}"]), f"parameter {i}"
        assert np.array_equal(m[i].numpy(), g[f"m1_{i}"]) and np.array_equal(v[i].numpy(), g[f"v1_{i}"]), f"moments {i}"


def test_fifty_update_loop():
    th.set_num_threads(1)
    g, L = pcm.load("loop50"), pc.LOOP
    learner = po.Learner(pieces(g, "p0"), g["scaling"], False, lr=L["lr"])
    losses = []
    for k in range(L["n"]):
        loss, pred = learner.update(*batch_of(g, g["idx"][k], 9, 2, 4, False))
        losses.append(loss.numpy())
    assert np.array_equal(np.asarray(losses), g["losses"]) and np.array_equal(pred.numpy(), g["pred"])
    for i in range(8):
        assert np.array_equal(learner.params[i].detach().numpy(), g[f"p1_{i}"]), f"parameter {i}"


@pytest.mark.parametrize("kind", list(pc.TRACES))
def test_training_trace(kind):
    """The restated host loop (replay heap, commands, RNG consumption order, evaluate's re-heapify) replays the reference's seeded
    train(): same actions, same commands, same heap, same log-probabilities, same parameters -- bit for bit."""
    th.set_num_threads(1)
    T, g = pc.TRACES[kind], pcm.load(f"trace_{kind}")
    assert g["robust_f32_f64"].all()
    pc.reseed(T["seed"])
    env, eval_env = getattr(momdp, T["env"])(T["seed"]), getattr(momdp, T["env"])(T["seed"] + 1)
    ag = po.Agent(env, T["scaling"], seed=T["seed"], **T["agent"])
    for i in range(8):
        assert np.array_equal(ag.learner.params[i].detach().numpy(), g[f"init_{i}"])
    pc.reseed(T["seed"] + 1)
    ag.train(eval_env=eval_env, **T["train"])
    assert np.array_equal(np.asarray(env.action_log, dtype=g["actions"].dtype), g["actions"])
    assert np.array_equal(np.stack([c[0] for c in ag.commands]), g["command_returns"])
    assert np.array_equal(np.asarray([c[1] for c in ag.commands]), g["command_horizons"])
    for got, key in zip(po.heap_summary(ag.replay), ("heap_distance", "heap_step", "heap_return", "heap_length")):
        assert np.array_equal(got, g[key]), key
    assert np.array_equal(np.stack(ag.logps), g["logps"])
    for i in range(8):
        assert np.array_equal(ag.learner.params[i].detach().numpy(), g[f"final_{i}"])
