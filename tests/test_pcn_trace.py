"""End-to-end PCN training against the reference's seeded train() (tests/golden/pcn_trace_*.npz): the HIP agent -- kernel sources
under the wave emulator on the CPU, the gfx950 library under -m gpu -- runs the same environment with the same seeds and must
take the same actions, choose the same commands, end with the same heap and, within the bound tests/test_train_traces.py applies
to the actor-critic traces (1e-4 absolute), the same parameters.

Discrete actions are compared exactly, with no mismatch budget: the generator only commits a seed whose action stream the
restatement reproduces both in float32 and with the acting forward pass evaluated in float64 (``robust_f32_f64`` in the fixture).
Continuous actions are the network's fp32 outputs plus noise; they are held to the 5e-5 the actor-critic traces use, and what
is derived from them to that bound propagated: PointReach moves 0.25 * a per step and pays 0.5 * (1 +- x) per step over 12
steps, so a return-to-go moves by at most 0.5 * 0.25 * (1 + 2 + ... + 12) * 5e-5 = 4.9e-4 (COMMAND_TOL)."""
import numpy as np
import pytest

import momdp
import pcn_cases as pc
import pcn_common as pcm

import morl_baselines_amd.native as native

PARAM_TOL = 1e-4       # tests/test_train_traces.py: check_final(..., atol=1e-4) of the MOSAC / GPI traces
ACTION_TOL = 5e-5      # tests/test_train_traces.py: continuous action streams
COMMAND_TOL = 5e-4     # ACTION_TOL through PointReach's return (module docstring)


@pytest.fixture(scope="module", params=pcm.BACKENDS)
def be(request):
    lib, dev = pcm.backend(request.param)
    native.use_library(lib if request.param == "sim" else None)
    yield lib, dev
    native.use_library(None)


@pytest.mark.parametrize("kind", list(pc.TRACES))
def test_pcn_trace(be, kind, tmp_path, monkeypatch):
    from morl_baselines_amd.pcn import PCN
    lib, dev = be
    monkeypatch.chdir(tmp_path)                      # train() checkpoints with save() into ./weights
    T, g = pc.TRACES[kind], pcm.load(f"trace_{kind}")
    assert g["robust_f32_f64"].all(), "the fixture's seed was not checked for accumulation-order robustness"
    pc.reseed(T["seed"])
    env, eval_env = getattr(momdp, T["env"])(T["seed"]), getattr(momdp, T["env"])(T["seed"] + 1)
    ag = PCN(env, T["scaling"], log=False, seed=T["seed"], device=dev, lib=lib, **T["agent"])
    for i, v in enumerate(ag.parameter_views()):
        assert np.array_equal(v.cpu().numpy(), g[f"init_{i}"]), f"initial parameter {i}"

    logps, state = [], {"eval": False}
    fwd, evaluate = ag._forward, ag.evaluate

    def fwd_logged(*a):
        out = fwd(*a)
        if not state["eval"]:
            logps.append(out[0].copy())
        return out

    def evaluate_flagged(*a, **k):
        state["eval"] = True
        try:
            return evaluate(*a, **k)
        finally:
            state["eval"] = False

    ag._forward, ag.evaluate = fwd_logged, evaluate_flagged
    pc.reseed(T["seed"] + 1)
    ag.train(eval_env=eval_env, ref_point=np.zeros(2), **{k: (v.copy() if isinstance(v, np.ndarray) else v)
                                                          for k, v in T["train"].items()})

    want = g["actions"]
    got = np.asarray(env.action_log, dtype=want.dtype)
    n = min(len(got), len(want))
    diff = (got[:n] != want[:n]) if kind == "discrete" else (np.abs(got[:n] - want[:n]).reshape(n, -1).max(1) > ACTION_TOL)
    if diff.any() or len(got) != len(want):
        k = int(np.argmax(diff)) if diff.any() else n
        # acting steps follow the num_er_episodes random episodes, whose length the first command's position gives
        warm = len(want) - len(g["logps"])
        j = k - warm
        detail = (f"; model output there: ours {logps[j]} reference {g['logps'][j]}" if 0 <= j < min(len(logps), len(g["logps"]))
                  else "")
        pytest.fail(f"{kind}: action stream differs first at environment step {k} of {len(want)} "
                    f"(ours {got[k] if k < len(got) else None}, reference {want[k] if k < len(want) else None}){detail}")
    if kind == "continuous":
        print(f"max action deviation {np.abs(got - want).max():.2e}")
    assert int(ag.global_step) == int(g["global_step"].reshape(-1)[0])

    cr = np.stack([c[0] for c in ag.command_log])
    ch = np.asarray([c[1] for c in ag.command_log], dtype=np.float32)
    dist, step, ret, length = (np.asarray([float(e[0]) for e in ag.experience_replay]),
                               np.asarray([e[1] for e in ag.experience_replay]),
                               np.asarray([e[2][0].reward for e in ag.experience_replay], dtype=np.float32),
                               np.asarray([len(e[2]) for e in ag.experience_replay]))
    assert np.array_equal(ch, g["command_horizons"])
    assert np.array_equal(step, g["heap_step"]) and np.array_equal(length, g["heap_length"])
    if kind == "discrete":
        assert np.array_equal(cr, g["command_returns"])
        assert np.array_equal(dist, g["heap_distance"]) and np.array_equal(ret, g["heap_return"])
    else:
        np.testing.assert_allclose(cr, g["command_returns"], rtol=0, atol=COMMAND_TOL)
        np.testing.assert_allclose(ret, g["heap_return"], rtol=0, atol=COMMAND_TOL)
        np.testing.assert_allclose(dist, g["heap_distance"], rtol=0, atol=4 * COMMAND_TOL)   # a doubled (crowded) L2 distance of two returns
    worst = 0.0
    for i, v in enumerate(ag.parameter_views()):
        err = float(np.abs(v.cpu().numpy() - g[f"final_{i}"]).max())
        worst = max(worst, err)
        assert err <= PARAM_TOL, f"final parameter {i}: max |diff| {err:.3e}"
    lp = np.abs(np.stack(logps) - g["logps"]).max()
    print(f"\nPCN {kind}: {len(want)} steps, {len(ag.command_log)} iterations, max parameter deviation {worst:.2e}, "
          f"max model-output deviation {lp:.2e}")
