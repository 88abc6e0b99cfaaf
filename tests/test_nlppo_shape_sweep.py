"""Seeded sweep of the NL-MO-PPO kernels (``morl_nlppo_*``) over shapes, tile counts and context reuse, against
``tests/nlppo_oracle.py`` in float64 (tests/nlppo_sweep.py builds the cases and explains the tolerances).

What the fixtures of test_nlppo_kernels_parity.py never reach and this module runs: an input of 128 columns, 2 and 32 actions, 1
and 8 objectives, one hidden layer of 32 and two of 128 / 96, minibatches of 2, 15, 17 and 129 rows (nine gradient partials), rows
whose logits spread by 60, a second GAE block, a smaller launch after a larger one on one context, rollout reallocation, ragged
epochs, and the launch counts.  Every output of every call has sentinel rows behind it (``nlppo_common.Ctx``).

``sim`` runs the unmodified kernel sources under the host wave emulator (CPU), ``hip`` the gfx950 library (-m gpu)."""
import ctypes

import numpy as np
import pytest
import torch as th

import nlppo_cases as nc
import nlppo_common as nm
import nlppo_oracle as no
import nlppo_sweep as sw


@pytest.fixture(scope="module", params=nm.BACKENDS)
def be(request):
    return nm.backend(request.param), request.param


def case_ctx(lib, dev, c, p0, max_minibatch, m0=None, v0=None, steps_done=0):
    return nm.Ctx(lib, dev, c.obs, c.A, c.R, c.pref_dim, c.hidden, max_minibatch, p0, m0, v0, steps_done=steps_done)


# ---------------------------------------------------------------------------------------------------------------------
# 1. single minibatch step
# ---------------------------------------------------------------------------------------------------------------------
def run_step(be, c, moments):
    (lib, dev), backend = be
    inp = sw.step_inputs(c)
    want, o32 = sw.step_oracle(c, th.float64, moments), sw.step_oracle(c, th.float32, moments)
    m0, v0 = nc.synthetic_moments(c.seed, len(inp["p0"])) if moments else (None, None)
    rep = sw.Report(f"{c.name}{'+moments' if moments else ''} [{backend}]")
    print(f"{rep.tag}: {(c.M + 15) // 16} tiles, ratio clipped {inp['rclip']:.2f}, objectives disagree {want['disagree']:.2f}, "
          f"gradient norm {want['stats'][7]:.3f}")
    if c.R > 1 and c.M > 2:
        assert want["disagree"] >= 0.05, c.name
    ctx = case_ctx(lib, dev, c, inp["p0"], c.M, m0, v0, 5 if moments else 0)
    try:
        ret, adv = ctx.set_batch(sw.as_fixture(inp))
        rep.close("advantages", adv, want["adv"], o32["adv"], 1e-5, 1e-6 * float(np.abs(want["adv"]).max()))
        rep.close("returns", ret, want["ret"], o32["ret"], 1e-5, 1e-6 * float(np.abs(want["ret"]).max()))
        w = inp["weights"].numpy()
        stats = ctx.update_n(inp["idx"][None], w, c.lr, **nm.step_kwargs(c))
        assert np.isfinite(stats).all() and np.isfinite(ctx.params.cpu().numpy()).all()
        sw.report_stats(rep, stats[0], want["stats"], o32["stats"], w)
        bounds = sw.tensor_bounds(inp["net"])
        rep.per_tensor("exp_avg", bounds, ctx.m.cpu().numpy(), want["m1"], o32["m1"], 1e-4, 2e-5)
        rep.per_tensor("exp_avg_sq", bounds, ctx.v.cpu().numpy(), want["v1"], o32["v1"], 2e-4, 2e-5)
        rep.close("parameters", ctx.params.cpu().numpy(), want["p1"], o32["p1"], 2e-5, 0.02 * c.lr)
    finally:
        ctx.close()
    rep.finish()


@pytest.mark.parametrize("c", sw.STEP_CASES, ids=lambda c: c.name)
def test_step_from_zero_adam_state(be, c):
    run_step(be, c, False)


@pytest.mark.parametrize("c", [c for c in sw.STEP_CASES if c.moments], ids=lambda c: c.name)
def test_step_from_synthetic_moments(be, c):
    run_step(be, c, True)


def test_the_step_cases_cover_what_they_are_for():
    cs = sw.STEP_CASES
    assert sum(c.D_in == 128 for c in cs) >= 4 and {c.M for c in cs} >= {2, 15, 17, 129}
    assert {(c.A, c.R) for c in cs if c.D_in == 128} >= {(32, 8), (2, 1), (32, 1), (2, 8)}
    assert {c.hidden for c in cs} >= {(32,), (128, 96)} and {c.pref_dim for c in cs if c.D_in == 128} >= {0, 1, 8}
    assert any(c.spread == 60.0 for c in cs) and any(c.negative_weight and not c.norm_adv for c in cs)
    assert sum(c.moments for c in cs) >= 3 and any(not c.with_pref for c in cs)


# ---------------------------------------------------------------------------------------------------------------------
# 2. GAE
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,E,R,gamma,lam,done_rate", sw.GAE_CASES, ids=lambda v: str(v))
def test_advantages_and_returns(be, T, E, R, gamma, lam, done_rate):
    (lib, dev), backend = be
    inp = sw.gae_inputs(T, E, R, done_rate)
    res = {}
    for dtype in (th.float64, th.float32):
        t = {k: v.to(dtype) for k, v in inp.items()}
        adv, ret = no.compute_advantages(t["rewards"], t["dones"], t["values"], t["next_value"], t["next_done"], gamma, lam)
        res[dtype] = (adv.reshape(T * E, R).double().numpy(), ret.reshape(T * E, R).double().numpy())
    P = int(lib.lib.morl_nlppo_param_count(3, 2, R, 0, 1, 32, 0))
    ctx = nm.Ctx(lib, dev, 3, 2, R, 0, (32,), 8, np.zeros(P))
    rep = sw.Report(f"gae T{T} E{E} R{R} [{backend}]")
    try:
        z, g = np.zeros, {k: v.numpy() for k, v in inp.items()}
        ctx.set_rollout(z((T * E, 3)), z((T * E, R)), z(T * E), z(T * E), g["rewards"], g["dones"], g["values"], None, T, E)
        ret, adv = ctx.gae(g["next_value"], g["next_done"], gamma, lam)
        (wa, wr), (oa, orr) = res[th.float64], res[th.float32]
        rep.close("advantages", adv, wa, oa, 1e-5, 1e-6 * float(np.abs(wa).max()))
        rep.close("returns", ret, wr, orr, 1e-5, 1e-6 * float(np.abs(wr).max()))
        # NULL outputs: the table alone is written (and a step can follow)
        nv, nd = ctx.T(g["next_value"]), ctx.T(g["next_done"])
        lib.check(lib.lib.morl_nlppo_gae(ctx.h, nv.data_ptr(), nd.data_ptr(), float(gamma), float(lam), None, None,
                                         lib.stream_of(ctx.params)))
        stats = ctx.update_n(np.zeros((1, 1), dtype=np.int32), np.ones(R), 1e-3, norm_adv=False)      # (reads back: nv, nd outlive the scan)
        assert np.isfinite(stats).all()
    finally:
        ctx.close()
    rep.finish()


# ---------------------------------------------------------------------------------------------------------------------
# 3. forward
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(sw.FORWARD_CASES)), ids=["limits", "two_actions", "smallest"])
def test_forward_against_float64_with_guard_rows(be, i):
    (lib, dev), backend = be
    f = sw.forward_case(i)
    ctx = nm.Ctx(lib, dev, f["obs"], f["A"], f["R"], f["pref_dim"], f["hidden"], 16, f["p0"])
    rep = sw.Report(f"forward obs{f['obs']} A{f['A']} R{f['R']} [{backend}]")
    try:
        for rows in sw.FORWARD_ROWS:
            logp, val = ctx.forward(f["obs_rows"][:rows], f["acc"][:rows], f["pref"])
            (wl, wv), (ol, ov) = f["want"], f["o32"]
            rep.close(f"rows {rows} log-probs", logp, wl[:rows], ol[:rows], 1e-5, nm.ATOL)
            rep.close(f"rows {rows} value", val, wv[:rows], ov[:rows], 1e-5, nm.ATOL)
            _, val_only = ctx.forward(f["obs_rows"][:rows], f["acc"][:rows], f["pref"], value_only=True)
            assert np.array_equal(val_only, val), rows
    finally:
        ctx.close()
    rep.finish()


# ---------------------------------------------------------------------------------------------------------------------
# 4. one context, many calls (the kernel against itself, fresh against reused: bit-exact)
# ---------------------------------------------------------------------------------------------------------------------
def state_of(ctx):
    return ctx.params.cpu().numpy().copy(), ctx.m.cpu().numpy().copy(), ctx.v.cpu().numpy().copy(), ctx.steps_done


def reuse_ctx(be, max_minibatch, state):
    (lib, dev), _ = be
    n = sw.REUSE_NET
    p, m, v, steps = state
    return nm.Ctx(lib, dev, n["obs"], n["A"], n["R"], n["pref_dim"], n["hidden"], max_minibatch, p, m, v, steps_done=steps)


def load_rollout(ctx, r, check_refusal=False):
    ctx.set_rollout(r["obs"], r["acc_rewards"], r["actions"], r["logprobs"], r["rewards"], r["dones"], r["values"], r["pref"], r["T"], r["E"])
    if check_refusal:
        with pytest.raises(RuntimeError, match="no advantages"):
            ctx.update_n(np.zeros((1, 2), dtype=np.int32), r["weights"], 3e-4)
    ctx.gae(r["next_value"], r["next_done"], 0.99, 0.95)


def same_bits(what, a, b):
    for name, x, y in zip(("statistics", "parameters", "exp_avg", "exp_avg_sq"), a, b):
        assert np.array_equal(x, y), f"{what}: {name} differ between the reused context and a fresh one"


@pytest.mark.parametrize("sizes", [(129, 17), (17, 129)], ids=["large_then_small", "small_then_large"])
def test_minibatch_sizes_share_a_context(be, sizes):
    """A launch of fewer tiles leaves the gradient and loss partials of the larger launch in place: they must not be read."""
    r = sw.reuse_rollout(401, 100, 2)
    first, second = r["perm"][:sizes[0]], r["perm"][::-1][:sizes[1]].copy()
    zero = np.zeros_like(r["p0"])
    ctx = reuse_ctx(be, 129, (r["p0"], zero, zero, 0))
    try:
        load_rollout(ctx, r)
        ctx.update_n(first[None], r["weights"], 3e-4)
        mid = state_of(ctx)
        reused = (ctx.update_n(second[None], r["weights"], 3e-4),) + state_of(ctx)[:3]
    finally:
        ctx.close()
    assert mid[3] == 1
    ctx = reuse_ctx(be, sizes[1], mid)
    try:
        load_rollout(ctx, r)
        fresh = (ctx.update_n(second[None], r["weights"], 3e-4),) + state_of(ctx)[:3]
    finally:
        ctx.close()
    same_bits(f"M = {sizes[1]} after M = {sizes[0]}", reused, fresh)


def test_rollout_grows_and_shrinks(be):
    """40 rows, 400 rows (reallocation), 40 rows again (below capacity, over old data): every step equals a fresh context's."""
    rolls = [sw.reuse_rollout(411, 20, 2), sw.reuse_rollout(412, 100, 4), sw.reuse_rollout(413, 8, 5)]
    zero = np.zeros_like(rolls[0]["p0"])
    ctx = reuse_ctx(be, 40, (rolls[0]["p0"], zero, zero, 0))
    try:
        for k, r in enumerate(rolls):
            idx = r["perm"][-40:][None] if k == 1 else r["perm"][:24 + 8 * k][None]     # (the 400-row step reads high rows)
            before = state_of(ctx)
            load_rollout(ctx, r, check_refusal=True)
            reused = (ctx.update_n(idx, r["weights"], 3e-4),) + state_of(ctx)[:3]
            other = reuse_ctx(be, 40, before)
            try:
                load_rollout(other, r, check_refusal=True)
                fresh = (other.update_n(idx, r["weights"], 3e-4),) + state_of(other)[:3]
            finally:
                other.close()
            same_bits(f"rollout {k} ({r['T'] * r['E']} rows)", reused, fresh)
    finally:
        ctx.close()


def test_ragged_epochs_as_the_agent_sends_them(be):
    """38 rows in 4 minibatches: 9, 9, 9, 9, 2 per epoch, two epochs, one ``update_n`` per run of equal sizes (``NLMOPPO.update``),
    against the oracle's loop under the whole-update test's drift rule."""
    (lib, dev), backend = be
    G, case = sw.RAGGED, sw.ragged_case()
    g, want, o32 = case["inp"], case["want"], case["o32"]
    print(f"ragged epoch: seed {case['seed']}, margin {case['margin']:.2e}")
    ctx = nm.Ctx(lib, dev, G["obs"], G["A"], G["R"], G["pref_dim"], G["hidden"], 9, case["p0"])
    rep = sw.Report(f"ragged [{backend}]")
    try:
        ctx.set_rollout(g["obs"], g["acc_rewards"], g["actions"], g["logprobs"], g["rewards"], g["dones"], g["values"], g["pref"],
                        G["T"], G["E"])
        ret, adv = ctx.gae(g["next_value"], g["next_done"], G["gamma"], G["gae_lambda"])
        nm.close_rel("returns", ret, want["ret"], 1e-5, 1e-6 * float(np.abs(want["ret"]).max()))
        nm.close_rel("advantages", adv, want["adv"], 1e-5, 1e-6 * float(np.abs(want["adv"]).max()))
        calls = []
        for mb in want["idx"]:
            if calls and len(calls[-1][-1]) == len(mb):
                calls[-1].append(mb)
            else:
                calls.append([mb])
        assert [(len(c), len(c[0])) for c in calls] == [(4, 9), (1, 2), (4, 9), (1, 2)]
        stats = np.concatenate([ctx.update_n(np.stack(c), g["weights"], G["lr"]) for c in calls])
        n = len(stats)
        assert n == 10 and ctx.steps_done == 10
        sw.report_stats(rep, stats[0], want["stats"][0], o32["stats"][0], g["weights"], "step 0 ")
        for i, name in enumerate(nm.STATS):
            if name == "clipfrac":
                assert np.array_equal(stats[:, i], want["stats"][:, i].astype(np.float32))
            else:
                nm.close_rel(f"all steps {name}", stats[:, i], want["stats"][:, i], 1e-3, 1e-5)
        nm.close_rel("parameters", ctx.params.cpu().numpy(), want["p1"], 2e-5, 0.02 * G["lr"] * n)
    finally:
        ctx.close()
    rep.finish()


# ---------------------------------------------------------------------------------------------------------------------
# 5. launch counts (the emulator counts them)
# ---------------------------------------------------------------------------------------------------------------------
def test_launch_counts():
    """n steps cost n launches, a forward one, the scan one, set_rollout one (the pack)."""
    lib, dev = nm.backend("sim")
    count = lib.lib.hipsim_launch_count
    count.restype = ctypes.c_longlong
    r = sw.reuse_rollout(401, 100, 2)
    zero = np.zeros_like(r["p0"])
    ctx = reuse_ctx(((lib, dev), "sim"), 40, (r["p0"], zero, zero, 0))
    try:
        c0 = count()
        ctx.set_rollout(r["obs"], r["acc_rewards"], r["actions"], r["logprobs"], r["rewards"], r["dones"], r["values"], r["pref"], 100, 2)
        assert count() - c0 == 1
        c0 = count()
        ctx.gae(r["next_value"], r["next_done"], 0.99, 0.95)
        assert count() - c0 == 1
        idx = np.stack([r["perm"][k * 40:(k + 1) * 40] for k in range(5)])
        c0 = count()
        ctx.update_n(idx, r["weights"], 3e-4)
        assert count() - c0 == 5
        for value_only in (False, True):
            c0 = count()
            ctx.forward(r["obs"][:33], r["acc_rewards"][:33], r["pref"], value_only=value_only)
            assert count() - c0 == 1
    finally:
        ctx.close()
