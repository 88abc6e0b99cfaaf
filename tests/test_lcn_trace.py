"""End-to-end LCN training against the reference's seeded train() (tests/golden/lcn_trace_*.npz): the HIP agent -- kernel sources
under the wave emulator on the CPU, the gfx950 library under -m gpu -- runs the same environment with the same seeds and must
take the same actions, choose the same commands, end with the same heap and, within the bound tests/test_pcn_trace.py applies,
the same parameters.  The comparisons and bounds are that file's, unchanged: discrete action streams, commands and heap
distances exact (the fixtures' seeds are checked for accumulation-order robustness by the generator); continuous ones within
ACTION_TOL / COMMAND_TOL as derived there; parameters within PARAM_TOL."""
import numpy as np
import pytest

import lcn_cases as lc
import lcn_common as lcm
import momdp
from test_pcn_trace import ACTION_TOL, COMMAND_TOL, PARAM_TOL

import morl_baselines_amd.native as native


@pytest.fixture(scope="module", params=lcm.BACKENDS)
def be(request):
    lib, dev = lcm.backend(request.param)
    native.use_library(lib if request.param == "sim" else None)
    yield lib, dev
    native.use_library(None)


@pytest.mark.parametrize("name", list(lc.TRACES))
def test_lcn_trace(be, name, tmp_path):
    from morl_baselines_amd.lcn import LCN
    lib, dev = be
    T, g = lc.TRACES[name], lcm.load(f"trace_{name}")
    kind = T["kind"]
    assert g["robust_f32_f64"].all(), "the fixture's seed was not checked for accumulation-order robustness"
    lc.reseed(T["seed"])
    env, eval_env = getattr(momdp, T["env"])(T["seed"]), getattr(momdp, T["env"])(T["seed"] + 1)
    ag = LCN(env, T["scaling"], log=False, seed=T["seed"], device=dev, lib=lib, **T["agent"])
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
    lc.reseed(T["seed"] + 1)
    ag.train(eval_env=eval_env, ref_point=np.zeros(2), save_dir=str(tmp_path / "weights"),
             **{k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in T["train"].items()})
    assert ag.cd_threshold == T["train"]["cd_threshold"]
    assert (tmp_path / "weights" / "LCN_model_0.pt").is_file(), "train() checkpoints as LCN_model_<k> into save_dir"

    want = g["actions"]
    got = np.asarray(env.action_log, dtype=want.dtype)
    n = min(len(got), len(want))
    diff = (got[:n] != want[:n]) if kind == "discrete" else (np.abs(got[:n] - want[:n]).reshape(n, -1).max(1) > ACTION_TOL)
    if diff.any() or len(got) != len(want):
        k = int(np.argmax(diff)) if diff.any() else n
        warm = len(want) - len(g["logps"])
        j = k - warm
        detail = (f"; model output there: ours {logps[j]} reference {g['logps'][j]}" if 0 <= j < min(len(logps), len(g["logps"]))
                  else "")
        pytest.fail(f"{name}: action stream differs first at environment step {k} of {len(want)} "
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
    print(f"\nLCN {name}: {len(want)} steps, {len(ag.command_log)} iterations, max parameter deviation {worst:.2e}, "
          f"max model-output deviation {lp:.2e}")
