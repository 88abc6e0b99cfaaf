"""MO-PPO through the C ABI (``morl_ppo_*``) against fixtures recorded from the reference.

``sim`` runs the unmodified kernel sources under the host wave emulator (CPU), ``hip`` the gfx950 library (-m gpu).
Tolerances are the project's contract as ``test_pcn_kernels_parity.py`` applies it: losses, log-probs, values, actions and entropy
1e-5 relative; stepped parameters within 2e-5 relative + 0.02 * lr per optimiser step; ``clipfrac`` exact.  ``approx_kl`` and
``old_approx_kl`` are means of differences of O(1) log-probabilities, and ``pg_loss`` under ``norm_adv`` is the mean of
``-adv * ratio`` over advantages whose mean is zero (the terms are O(1), their mean is not): these get PCN's ``PRED_ATOL`` = 1e-6
as an absolute term, and so does ``loss``, which contains ``pg_loss``.  The gradient norm is a 2-norm over every parameter: 1e-5
relative."""
import ctypes as C

import numpy as np
import pytest
import torch as th

import ppo_cases as pc
import ppo_common as pm

ATOL = 1e-6
STAT_ATOL = {"loss": ATOL, "pg_loss": ATOL, "old_approx_kl": ATOL, "approx_kl": ATOL}


@pytest.fixture(scope="module", params=pm.BACKENDS)
def be(request):
    return pm.backend(request.param)


def check_stats(got, want, tag=""):
    for i, name in enumerate(pm.STATS):
        if name == "clipfrac":
            assert np.array_equal(got[..., i], want[..., i]), (tag, name, got[..., i], want[..., i])
        else:
            pm.close_rel(f"{tag}{name}", got[..., i], want[..., i], 1e-5, STAT_ATOL.get(name, 0.0))


def step_ctx(be, c, g):
    lib, dev = be
    m0, v0 = pc.synthetic_moments(c.seed, len(g["p0"]))
    ctx = pm.Ctx(lib, dev, c.D, c.A, c.R, c.hidden, c.M, g["p0"], m0, v0, steps_done=c.step)
    ret, adv = ctx.set_batch(g)
    assert np.array_equal(ret, g["returns"])
    pm.close_rel("advantages", adv, g["advantages"], 1e-5, 1e-6 * float(np.abs(g["advantages"]).max()))
    return ctx


def step_kwargs(c):
    return dict(clip_coef=c.clip_coef, ent_coef=c.ent_coef, vf_coef=c.vf_coef, max_grad_norm=c.max_grad_norm,
                clip_vloss=c.clip_vloss, norm_adv=c.norm_adv)


@pytest.mark.parametrize("c", pc.STEP_CASES, ids=lambda c: c.name)
def test_single_step_matches_the_reference(be, c):
    g = pm.load(c.name)
    ctx = step_ctx(be, c, g)
    try:
        act, lp, val = ctx.forward(g["obs"], g["fwd_eps"])
        pm.close_rel("action", act, g["fwd_action"], 1e-5, ATOL)
        pm.close_rel("log-prob", lp, g["fwd_logprob"], 1e-5)
        pm.close_rel("value", val, g["fwd_value"], 1e-5, ATOL)
        stats = ctx.update_n(g["idx"][None], c.lr, **step_kwargs(c))
        check_stats(stats[0], g["stats"])
        assert (g["stats"][7] > c.max_grad_norm) == c.clip_active
        pm.close_rel("parameters", ctx.params.cpu().numpy(), g["p1"], 2e-5, 0.02 * c.lr)
        pm.close_rel("exp_avg", ctx.m.cpu().numpy(), g["m1"], 1e-4, 2e-5 * float(np.abs(g["m1"]).max()))
        pm.close_rel("exp_avg_sq", ctx.v.cpu().numpy(), g["v1"], 2e-4, 2e-5 * float(np.abs(g["v1"]).max()))
    finally:
        ctx.close()


@pytest.mark.parametrize("use_gae", [True, False], ids=["gae", "mc"])
def test_advantages_match_the_reference(be, use_gae):
    g, G = pm.load("gae"), pc.GAE
    lib, dev = be
    T, E, R = G["T"], G["E"], G["R"]
    P = int(lib.lib.morl_ppo_param_count(G["D"], G["A"], R, *pm.hidden_args(G["hidden"])))
    ctx = pm.Ctx(lib, dev, G["D"], G["A"], R, G["hidden"], 8, np.zeros(P))
    try:
        z = np.zeros
        ctx.set_rollout(z((T * E, G["D"])), z((T * E, G["A"])), z(T * E), g["rewards"], g["dones"], g["values"], T, E)
        ret, adv = ctx.gae(g["next_value"], g["next_done"], g["weights"], G["gamma"], G["gae_lambda"], use_gae)
        tag = "gae" if use_gae else "mc"
        want_ret, want_adv = g[f"returns_{tag}"].reshape(T * E, R), g[f"advantages_{tag}"].reshape(-1)
        pm.close_rel("returns", ret, want_ret, 1e-5, 1e-6 * float(np.abs(want_ret).max()))
        pm.close_rel("advantages", adv, want_adv, 1e-5, 1e-6 * float(np.abs(want_adv).max()))
    finally:
        ctx.close()


def update_ctx(be, g):
    U = pc.UPDATE
    lib, dev = be
    T, E = U["T"], U["E"]
    ctx = pm.Ctx(lib, dev, U["D"], U["A"], U["R"], U["hidden"], T * E // U["num_minibatches"], g["p0"])
    ctx.set_rollout(g["obs"], g["actions"], g["logprobs"], g["rewards"], g["dones"], g["values"], T, E)
    ret, adv = ctx.gae(g["next_value"], g["next_done"], g["weights"], U["gamma"], U["gae_lambda"], True)
    return ctx, ret, adv


@pytest.mark.parametrize("kind", list(pc.UPDATE_KINDS))
def test_whole_update_matches_the_reference(be, kind):
    g, U = pm.load(f"update_{kind}"), pc.UPDATE
    ctx, ret, adv = update_ctx(be, g)
    try:
        want_ret, want_adv = g["returns"].reshape(-1, U["R"]), g["advantages"].reshape(-1)
        pm.close_rel("returns", ret, want_ret, 1e-5, 1e-6 * float(np.abs(want_ret).max()))
        pm.close_rel("advantages", adv, want_adv, 1e-5, 1e-6 * float(np.abs(want_adv).max()))
        n = len(g["idx"])
        stats = ctx.update_n(g["idx"], U["lr"])
        # step k starts from parameters that already differ from the reference's by up to 0.02 * lr * k per entry; the first
        # step's statistics are held to the single-step contract, the last one's to what that drift allows: 1e-3 relative
        check_stats(stats[0], g["stats"][0], "step 0 ")
        for i, name in enumerate(pm.STATS):
            if name == "clipfrac":
                assert np.array_equal(stats[:, i], g["stats"][:, i])
            else:
                pm.close_rel(f"all steps {name}", stats[:, i], g["stats"][:, i], 1e-3, 1e-5)
        pm.close_rel("parameters", ctx.params.cpu().numpy(), g["p1"], 2e-5, 0.02 * U["lr"] * n)
    finally:
        ctx.close()


def test_update_n_is_n_single_steps_and_runs_are_bit_identical(be):
    g, U = pm.load("update_full"), pc.UPDATE
    n = 6
    runs = []
    for split in (False, False, True):
        ctx, _, _ = update_ctx(be, g)
        try:
            if split:
                stats = np.concatenate([ctx.update_n(g["idx"][k:k + 1], U["lr"]) for k in range(n)])
            else:
                stats = ctx.update_n(g["idx"][:n], U["lr"])
            runs.append((stats, ctx.params.cpu().numpy(), ctx.m.cpu().numpy(), ctx.v.cpu().numpy()))
        finally:
            ctx.close()
    for name, a, b, c in zip(("statistics", "parameters", "exp_avg", "exp_avg_sq"), *runs):
        assert np.array_equal(a, b), f"{name}: two identical runs differ"
        assert np.array_equal(a, c), f"{name}: update_n({n}) differs from {n} x update_n(1)"


def test_forward_rows_and_get_value(be):
    c = pc.BY_NAME["c_m50_h128_96"]
    g = pm.load(c.name)
    lib, dev = be
    ctx = pm.Ctx(lib, dev, c.D, c.A, c.R, c.hidden, c.M, g["p0"])
    try:
        full = ctx.forward(g["obs"], g["fwd_eps"])
        for rows in (1, 15, 16, 17, 33):
            part = ctx.forward(g["obs"][:rows], g["fwd_eps"][:rows])
            for a, b in zip(part, full):
                assert np.array_equal(a, b[:rows]), rows
            _, _, val = ctx.forward(g["obs"][:rows], value_only=True)
            assert np.array_equal(val, full[2][:rows]), rows
    finally:
        ctx.close()


def test_refusals(be):
    lib, dev = be
    count, err = lib.lib.morl_ppo_param_count, lib.lib.morl_last_error
    assert count(0, 3, 2, 2, 64, 64) == -1 and b"obs_dim" in err()
    assert count(129, 3, 2, 2, 64, 64) == -1 and b"obs_dim" in err()
    assert count(4, 33, 2, 2, 64, 64) == -1 and b"action_dim" in err()
    assert count(4, 3, 9, 2, 64, 64) == -1 and b"reward_dim" in err()
    assert count(4, 3, 2, 3, 64, 64) == -1 and b"hidden layers" in err()
    assert count(4, 3, 2, 2, 48, 64) == -1 and b"hidden width 48" in err()
    assert count(4, 3, 2, 2, 64, 160) == -1 and b"hidden width 160" in err()
    assert count(4, 3, 2, 1, 64, 7) == 3 + (4 * 64 + 64 + 2 * 64 + 2) + (4 * 64 + 64 + 3 * 64 + 3)
    assert count(4, 3, 2, 2, 128, 96) > 0
    h = C.c_void_p()
    assert lib.lib.morl_ppo_create(C.byref(h), 4, 3, 2, 2, 64, 48, 8) != 0 and b"hidden width 48" in err()
    P = int(count(4, 3, 2, 2, 64, 32))
    ctx = pm.Ctx(lib, dev, 4, 3, 2, (64, 32), 8, np.zeros(P))
    try:
        with pytest.raises(RuntimeError, match="no rollout"):
            ctx.update_n(np.zeros((1, 8), dtype=np.int32), 1e-3)
        z = np.zeros
        ctx.set_rollout(z((8, 4)), z((8, 3)), z(8), z((8, 2)), z(8), z((8, 2)), 8, 1)
        with pytest.raises(RuntimeError, match="no advantages"):
            ctx.update_n(np.zeros((1, 8), dtype=np.int32), 1e-3)
        ctx.gae(z((1, 2)), z(1), np.ones(2), 0.99, 0.95)
        with pytest.raises(RuntimeError, match="minibatch"):
            ctx.update_n(np.zeros((1, 9), dtype=np.int32), 1e-3)
        with pytest.raises(RuntimeError, match="norm_adv"):
            ctx.update_n(np.zeros((1, 1), dtype=np.int32), 1e-3)
        assert ctx.update_n(np.zeros((1, 1), dtype=np.int32), 1e-3, norm_adv=False).shape == (1, 8)
    finally:
        ctx.close()
