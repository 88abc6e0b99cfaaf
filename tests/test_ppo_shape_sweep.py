"""Seeded sweep of the MO-PPO kernels (``morl_ppo_*``) over shapes, tile counts and context reuse, against ``tests/ppo_oracle.py``
in float64 (tests/ppo_sweep.py builds the cases and explains the tolerances).

What the fixtures of test_ppo_kernels_parity.py never reach and this module runs: five and more gradient partials (the last
workgroup's four-at-a-time sum and each remainder after it), minibatches of more than 256 rows (the second pass of the advantage
normalisation), obs_dim 128 / action_dim 32 / reward_dim 8 and the other ends of those ranges, 96-wide and widening hidden layers,
a second GAE block, a smaller launch after a larger one on one context, rollout reallocation, and writes behind an output.

``sim`` runs the unmodified kernel sources under the host wave emulator (CPU), ``hip`` the gfx950 library (-m gpu)."""
import numpy as np
import pytest
import torch as th

import ppo_cases as pc
import ppo_common as pm
import ppo_sweep as sw


@pytest.fixture(scope="module", params=pm.BACKENDS)
def be(request):
    return pm.backend(request.param), request.param


# ---------------------------------------------------------------------------------------------------------------------
# 1. single minibatch step
# ---------------------------------------------------------------------------------------------------------------------
def run_step(be, c, moments):
    (lib, dev), backend = be
    inp = sw.step_inputs(c)
    want, o32 = sw.step_oracle(c, th.float64, moments), sw.step_oracle(c, th.float32, moments)
    m0, v0 = pc.synthetic_moments(c.seed, len(inp["p0"])) if moments else (None, None)
    rep = sw.Report(f"{c.name}{'+moments' if moments else ''} [{backend}]")
    print(f"{rep.tag}: {c.tiles} tiles, ratio clipped {inp['rclip']:.2f}, value clipped {inp['vclip']:.2f}, margin "
          f"{inp['margin']:.2e}, gradient norm {want['stats'][7]:.3f}")
    ctx = sw.Ctx(lib, dev, c.D, c.A, c.R, c.hidden, c.M, inp["p0"], m0, v0, steps_done=5 if moments else 0)
    try:
        g = {k: inp[k].numpy() for k in ("obs", "actions", "logprobs", "returns", "values", "weights")}
        ret, adv = ctx.set_batch(g)
        assert np.array_equal(ret, g["returns"])
        rep.close("advantages", adv, want["adv"], o32["adv"], 1e-5, 1e-6 * float(np.abs(want["adv"]).max()))
        stats = ctx.update_n(inp["idx"][None], c.lr, **c.kwargs())
        rep.stats(stats[0], want["stats"], o32["stats"])
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
    """Tile counts with every remainder of the four-at-a-time sum after at least one full group, M > 256, and the declared limits."""
    tiles = {c.tiles for c in sw.STEP_CASES}
    assert {5, 6, 7, 8, 9, 17, 19} <= tiles and {(t - 1) % 4 for t in tiles if t >= 5} == {0, 1, 2, 3}
    assert any(c.M > 256 and c.norm_adv for c in sw.STEP_CASES)
    assert any((c.D, c.A, c.R, c.hidden) == (128, 32, 8, (128, 128)) for c in sw.STEP_CASES)
    assert {1} <= {c.D for c in sw.STEP_CASES} and {1, 8} <= {c.R for c in sw.STEP_CASES}
    assert {(96, 64), (32, 128), (128,), (96,)} <= {c.hidden for c in sw.STEP_CASES}
    assert sum(c.moments for c in sw.STEP_CASES) >= 4 and sw.STEP_CASES[0].moments


# ---------------------------------------------------------------------------------------------------------------------
# 2. GAE and discounted returns
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_gae", [True, False], ids=["gae", "mc"])
@pytest.mark.parametrize("T,E,R,gamma,lam,done_rate", sw.GAE_CASES, ids=lambda v: str(v))
def test_advantages_and_returns(be, T, E, R, gamma, lam, done_rate, use_gae):
    (lib, dev), backend = be
    inp = sw.gae_inputs(T, E, R, done_rate)
    g = {k: v.numpy() for k, v in inp.items() if isinstance(v, th.Tensor)}
    want_ret, want_adv = sw.gae_oracle(inp, T, E, R, gamma, lam, use_gae)
    n = sw.GAE_NET
    M = len(inp["idx"])
    runs = []
    for outputs in (True, False):
        ctx = sw.Ctx(lib, dev, n["D"], n["A"], R, n["hidden"], M, inp["p0"])
        try:
            ctx.set_rollout(g["obs"], g["actions"], g["logprobs"], g["rewards"], g["dones"], g["values"], T, E)
            if outputs:
                ret, adv = ctx.gae(g["next_value"], g["next_done"], g["weights"], gamma, lam, use_gae)
                pm.close_rel("returns", ret, want_ret.numpy(), 1e-5, 1e-6 * float(want_ret.abs().max()))
                pm.close_rel("advantages", adv, want_adv.numpy(), 1e-5, 1e-6 * float(want_adv.abs().max()))
            else:
                ctx.gae_into_the_table_only(g["next_value"], g["next_done"], g["weights"], gamma, lam, use_gae)
            stats = ctx.update_n(inp["idx"][None], 3e-4, clip_vloss=False, norm_adv=False)
            runs.append((stats, ctx.params.cpu().numpy(), ctx.m.cpu().numpy(), ctx.v.cpu().numpy()))
        finally:
            ctx.close()
    # the table holds what the copies hold: pg_loss is continuous in the advantages, v_loss (unclipped) in the returns
    rep = sw.Report(f"gae T{T} E{E} R{R} {'gae' if use_gae else 'mc'} [{backend}]")
    pg64, v64 = sw.gae_step_losses(inp, want_ret, want_adv, th.float64)
    pg32, v32 = sw.gae_step_losses(inp, *sw.gae_oracle(inp, T, E, R, gamma, lam, use_gae, th.float32), th.float32)
    rep.close("pg_loss", runs[0][0][0, 1], pg64, pg32, 1e-5, sw.ATOL)
    rep.close("v_loss", runs[0][0][0, 2], v64, v32, 1e-5)
    rep.finish()
    # and the NULL-output call leaves the same table: the step that follows gives the same bits
    for name, a, b in zip(("statistics", "parameters", "exp_avg", "exp_avg_sq"), *runs):
        assert np.array_equal(a, b), f"{name}: a step after morl_ppo_gae without output copies differs"


# ---------------------------------------------------------------------------------------------------------------------
# 3. forward and guard rows
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(sw.FORWARD_CASES)), ids=["limits", "ones"])
def test_forward_against_float64_with_guard_rows(be, i):
    (lib, dev), backend = be
    f = sw.forward_case(i)
    ctx = sw.Ctx(lib, dev, f["D"], f["A"], f["R"], f["hidden"], 16, f["p0"])
    rep = sw.Report(f"forward D{f['D']} A{f['A']} R{f['R']} [{backend}]")
    try:
        for rows in sw.FORWARD_ROWS:
            act, lp, val = ctx.forward(f["obs"][:rows], f["eps"][:rows], guard_rows=16)
            (wa, wl, wv), (oa, ol, ov) = f["want"], f["o32"]
            rep.close(f"rows {rows} action", act, wa[:rows], oa[:rows], 1e-5, sw.ATOL)
            rep.close(f"rows {rows} log-prob", lp, wl[:rows], ol[:rows], 1e-5)
            rep.close(f"rows {rows} value", val, wv[:rows], ov[:rows], 1e-5, sw.ATOL)
            _, _, val_only = ctx.forward(f["obs"][:rows], value_only=True, guard_rows=16)
            assert np.array_equal(val_only, val), rows
    finally:
        ctx.close()
    rep.finish()


def test_statistics_stay_inside_their_rows(be):
    (lib, dev), _ = be
    c = sw.STEP_BY_NAME["t2_m17_unclipped"]
    inp = sw.step_inputs(c)
    ctx = sw.Ctx(lib, dev, c.D, c.A, c.R, c.hidden, c.M, inp["p0"])
    try:
        ctx.set_batch({k: inp[k].numpy() for k in ("obs", "actions", "logprobs", "returns", "values", "weights")})
        idx = np.stack([inp["idx"], inp["idx"][::-1]])
        stats = ctx.update_n(idx, c.lr, guard_rows=1, **c.kwargs())
        assert stats.shape == (2, 8) and np.isfinite(stats).all() and (stats[:, 7] > 0).all()
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. one context, many calls (the kernel against itself, fresh against reused: bit-exact)
# ---------------------------------------------------------------------------------------------------------------------
def state_of(ctx):
    return ctx.params.cpu().numpy().copy(), ctx.m.cpu().numpy().copy(), ctx.v.cpu().numpy().copy(), ctx.steps_done


def reuse_ctx(be, max_minibatch, state):
    (lib, dev), _ = be
    n = sw.REUSE_NET
    p, m, v, steps = state
    return sw.Ctx(lib, dev, n["D"], n["A"], n["R"], n["hidden"], max_minibatch, p, m, v, steps_done=steps)


def load_rollout(ctx, r, check_refusal=False):
    ctx.set_rollout(r["obs"], r["actions"], r["logprobs"], r["rewards"], r["dones"], r["values"], r["T"], r["E"])
    if check_refusal:
        with pytest.raises(RuntimeError, match="no advantages"):
            ctx.update_n(np.zeros((1, 2), dtype=np.int32), 3e-4)
    ctx.gae(r["next_value"], r["next_done"], r["weights"], 0.995, 0.95)


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
        ctx.update_n(first[None], 3e-4)
        mid = state_of(ctx)
        reused = (ctx.update_n(second[None], 3e-4),) + state_of(ctx)[:3]
    finally:
        ctx.close()
    assert mid[3] == 1
    ctx = reuse_ctx(be, sizes[1], mid)
    try:
        load_rollout(ctx, r)
        fresh = (ctx.update_n(second[None], 3e-4),) + state_of(ctx)[:3]
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
            reused = (ctx.update_n(idx, 3e-4),) + state_of(ctx)[:3]
            other = reuse_ctx(be, 40, before)
            try:
                load_rollout(other, r, check_refusal=True)
                fresh = (other.update_n(idx, 3e-4),) + state_of(other)[:3]
            finally:
                other.close()
            same_bits(f"rollout {k} ({r['T'] * r['E']} rows)", reused, fresh)
    finally:
        ctx.close()


def test_ragged_epochs_as_the_agent_sends_them(be):
    """38 rows in 4 minibatches: 9, 9, 9, 9, 2 per epoch, two epochs, one ``update_n`` per run of equal sizes (``MOPPO.update``),
    against ``po.update`` under the whole-update test's drift rule."""
    (lib, dev), backend = be
    G, case = sw.RAGGED, sw.ragged_case()
    g, want, o32 = case["inp"], case["want"], case["o32"]
    print(f"ragged epoch: seed {case['seed']}, margin {case['margin']:.2e}")
    ctx = sw.Ctx(lib, dev, G["D"], G["A"], G["R"], G["hidden"], 9, case["p0"])
    rep = sw.Report(f"ragged [{backend}]")
    try:
        ctx.set_rollout(g["obs"], g["actions"], g["logprobs"], g["rewards"], g["dones"], g["values"], G["T"], G["E"])
        ret, adv = ctx.gae(g["next_value"], g["next_done"], g["weights"], G["gamma"], G["gae_lambda"], True)
        pm.close_rel("returns", ret, want["ret"], 1e-5, 1e-6 * float(np.abs(want["ret"]).max()))
        pm.close_rel("advantages", adv, want["adv"], 1e-5, 1e-6 * float(np.abs(want["adv"]).max()))
        calls = []
        for mb in want["idx"]:
            if calls and len(calls[-1][-1]) == len(mb):
                calls[-1].append(mb)
            else:
                calls.append([mb])
        assert [(len(c), len(c[0])) for c in calls] == [(4, 9), (1, 2), (4, 9), (1, 2)]
        stats = np.concatenate([ctx.update_n(np.stack(c), G["lr"]) for c in calls])
        n = len(stats)
        assert n == 10 and ctx.steps_done == 10
        rep.stats(stats[0], want["stats"][0], o32["stats"][0], "step 0 ")
        for i, name in enumerate(pm.STATS):
            if name == "clipfrac":
                assert np.array_equal(stats[:, i], want["stats"][:, i].astype(np.float32))
            else:
                pm.close_rel(f"all steps {name}", stats[:, i], want["stats"][:, i], 1e-3, 1e-5)
        pm.close_rel("parameters", ctx.params.cpu().numpy(), want["p1"], 2e-5, 0.02 * G["lr"] * n)
    finally:
        ctx.close()
    rep.finish()
