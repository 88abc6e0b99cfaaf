"""NL-MO-PPO through the C ABI (``morl_nlppo_*``) against fixtures recorded from the reference.

``sim`` runs the unmodified kernel sources under the host wave emulator (CPU), ``hip`` the gfx950 library (-m gpu).
Tolerances are the project's contract as ``test_ppo_kernels_parity.py`` states it: losses, log-probs, values and entropy 1e-5
relative; stepped parameters within 2e-5 relative + 0.02 * lr per optimiser step; ``clipfrac`` exact; the gradient norm 1e-5
relative.  Absolute terms (``nlppo_common.stat_atol``): 1e-6 for the two KLs, and 1e-6 * max(1, sum_k |w_k|) for ``pg_loss`` and
``loss``, whose terms are O(sum_k |w_k|) while their mean is not."""
import ctypes as C

import numpy as np
import pytest
import torch as th

import nlppo_cases as nc
import nlppo_common as nm

ATOL = nm.ATOL


@pytest.fixture(scope="module", params=nm.BACKENDS)
def be(request):
    return nm.backend(request.param)


def step_ctx(be, c, g, max_minibatch=None):
    lib, dev = be
    m0, v0 = nc.synthetic_moments(c.seed, len(g["p0"]))
    ctx = nm.Ctx(lib, dev, c.D, c.A, c.R, c.pref_dim, nc.HIDDEN, max_minibatch or c.M, g["p0"], m0, v0, steps_done=c.step)
    ret, adv = ctx.set_batch(g)
    # (the scan's operations are the reference's: with gamma = 0 nothing is left to round differently)
    assert np.array_equal(adv, g["advantages"]) and np.array_equal(ret, g["returns"])
    return ctx


@pytest.mark.parametrize("c", nc.STEP_CASES, ids=lambda c: c.name)
def test_single_step_matches_the_reference(be, c):
    g = nm.load(c.name)
    ctx = step_ctx(be, c, g)
    try:
        pref = g["pref"] if "pref" in g else None
        logp, val = ctx.forward(g["obs"], g["acc_rewards"], pref)
        nm.close_rel("log-probs", logp, g["fwd_logp"], 1e-5)
        nm.close_rel("value", val, g["fwd_value"], 1e-5, ATOL)
        assert np.array_equal(np.argmax(logp, axis=1), g["fwd_greedy"])
        stats = ctx.update_n(g["idx"][None], g["weights"], c.lr, **nm.step_kwargs(c))
        nm.check_stats(stats[0], g["stats"], g["weights"])
        assert (g["stats"][7] > c.max_grad_norm) == c.clip_active
        nm.close_rel("parameters", ctx.params.cpu().numpy(), g["p1"], 2e-5, 0.02 * c.lr)
        nm.close_rel("exp_avg", ctx.m.cpu().numpy(), g["m1"], 1e-4, 2e-5 * float(np.abs(g["m1"]).max()))
        nm.close_rel("exp_avg_sq", ctx.v.cpu().numpy(), g["v1"], 2e-4, 2e-5 * float(np.abs(g["v1"]).max()))
    finally:
        ctx.close()


def test_advantages_match_the_reference(be):
    g, G = nm.load("gae"), nc.GAE
    lib, dev = be
    T, E, R = G["T"], G["E"], G["R"]
    P = int(lib.lib.morl_nlppo_param_count(3, 2, R, R, 1, 32, 0))
    ctx = nm.Ctx(lib, dev, 3, 2, R, R, (32,), 8, np.zeros(P))
    try:
        z = np.zeros
        ctx.set_rollout(z((T * E, 3)), z((T * E, R)), z(T * E), z(T * E), g["rewards"], g["dones"], g["values"], None, T, E)
        ret, adv = ctx.gae(g["next_value"], g["next_done"], G["gamma"], G["gae_lambda"])
        want_ret, want_adv = g["returns"].reshape(T * E, R), g["advantages"].reshape(T * E, R)
        nm.close_rel("returns", ret, want_ret, 1e-5, 1e-6 * float(np.abs(want_ret).max()))
        nm.close_rel("advantages", adv, want_adv, 1e-5, 1e-6 * float(np.abs(want_adv).max()))
    finally:
        ctx.close()


def update_ctx(be, g):
    U = nc.UPDATE
    lib, dev = be
    T, E = U["T"], U["E"]
    ctx = nm.Ctx(lib, dev, U["D"], U["A"], U["R"], U["pref_dim"], nc.HIDDEN, T * E // U["num_minibatches"], g["p0"])
    ctx.set_rollout(g["obs"], g["acc_rewards"], g["actions"], g["logprobs"], g["rewards"], g["dones"], g["values"], g["pref"], T, E)
    ret, adv = ctx.gae(g["next_value"], g["next_done"], U["gamma"], U["gae_lambda"])
    return ctx, ret, adv


@pytest.mark.parametrize("kind", list(nc.UPDATE_KINDS))
def test_whole_update_matches_the_reference(be, kind):
    g, U = nm.load(f"update_{kind}"), nc.UPDATE
    ctx, ret, adv = update_ctx(be, g)
    try:
        want_ret, want_adv = g["returns"].reshape(-1, U["R"]), g["advantages"].reshape(-1, U["R"])
        nm.close_rel("returns", ret, want_ret, 1e-5, 1e-6 * float(np.abs(want_ret).max()))
        nm.close_rel("advantages", adv, want_adv, 1e-5, 1e-6 * float(np.abs(want_adv).max()))
        n = len(g["idx"])
        assert n == (12 if kind == "full" else 8)
        stats = ctx.update_n(g["idx"], g["weights"], U["lr"])
        # step k starts from parameters that already differ from the reference's by up to 0.02 * lr * k per entry; the first
        # step's statistics are held to the single-step contract, the later ones' to what that drift allows: 1e-3 relative
        nm.check_stats(stats[0], g["stats"][0], g["weights"], "step 0 ")
        for i, name in enumerate(nm.STATS):
            if name == "clipfrac":
                assert np.array_equal(stats[:, i], g["stats"][:, i])
            else:
                nm.close_rel(f"all steps {name}", stats[:, i], g["stats"][:, i], 1e-3, 1e-5)
        nm.close_rel("parameters", ctx.params.cpu().numpy(), g["p1"], 2e-5, 0.02 * U["lr"] * n)
    finally:
        ctx.close()


def test_update_n_is_n_single_steps_and_runs_are_bit_identical(be):
    g, U = nm.load("update_full"), nc.UPDATE
    n = 6
    runs = []
    for split in (False, False, True):
        ctx, _, _ = update_ctx(be, g)
        try:
            if split:
                stats = np.concatenate([ctx.update_n(g["idx"][k:k + 1], g["weights"], U["lr"]) for k in range(n)])
            else:
                stats = ctx.update_n(g["idx"][:n], g["weights"], U["lr"])
            runs.append((stats, ctx.params.cpu().numpy(), ctx.m.cpu().numpy(), ctx.v.cpu().numpy()))
        finally:
            ctx.close()
    for name, a, b, c in zip(("statistics", "parameters", "exp_avg", "exp_avg_sq"), *runs):
        assert np.array_equal(a, b), f"{name}: two identical runs differ"
        assert np.array_equal(a, c), f"{name}: update_n({n}) differs from {n} x update_n(1)"


@pytest.mark.parametrize("name", ["a", "c"])
def test_a_step_reproduces_the_log_probs_the_forward_stored(be, name):
    """The log-prob of an action gathered from ``morl_nlppo_forward`` at the step's own parameters is what the step recomputes."""
    c = nc.BY_NAME[name]
    g = dict(nm.load(c.name))
    lib, dev = be
    ctx = nm.Ctx(lib, dev, c.D, c.A, c.R, c.pref_dim, nc.HIDDEN, c.M, g["p0"])
    try:
        logp, _ = ctx.forward(g["obs"], g["acc_rewards"], g.get("pref"))
        g["logprobs"] = logp[np.arange(c.M), g["actions"]]
        ctx.set_batch(g)
        stats = ctx.update_n(g["idx"][None], g["weights"], c.lr, **nm.step_kwargs(c))[0]
        assert stats[4] == 0.0 and stats[5] == 0.0 and stats[6] == 0.0, stats
    finally:
        ctx.close()


def test_forward_rows_and_get_value(be):
    c = nc.BY_NAME["c"]
    g = nm.load(c.name)
    lib, dev = be
    ctx = nm.Ctx(lib, dev, c.D, c.A, c.R, c.pref_dim, nc.HIDDEN, c.M, g["p0"])
    try:
        full = ctx.forward(g["obs"], g["acc_rewards"])
        for rows in (1, 15, 16, 17, 33):
            part = ctx.forward(g["obs"][:rows], g["acc_rewards"][:rows])
            for a, b in zip(part, full):
                assert np.array_equal(a, b[:rows]), rows
            none, val = ctx.forward(g["obs"][:rows], g["acc_rewards"][:rows], value_only=True)
            assert none is None and np.array_equal(val, full[1][:rows]), rows
    finally:
        ctx.close()


def test_a_null_preference_is_a_zero_preference(be):
    c = nc.BY_NAME["a"]
    g = nm.load(c.name)
    lib, dev = be
    ctx = nm.Ctx(lib, dev, c.D, c.A, c.R, c.pref_dim, nc.HIDDEN, c.M, g["p0"])
    try:
        a = ctx.forward(g["obs"], g["acc_rewards"], None)
        b = ctx.forward(g["obs"], g["acc_rewards"], np.zeros(c.pref_dim))
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        assert not np.array_equal(a[0], ctx.forward(g["obs"], g["acc_rewards"], g["pref"])[0])
    finally:
        ctx.close()


def test_refusals(be):
    lib, dev = be
    count, err = lib.lib.morl_nlppo_param_count, lib.lib.morl_last_error
    assert count(0, 3, 2, 2, 2, 64, 64) == -1 and b"obs_dim" in err()
    assert count(125, 3, 2, 2, 2, 64, 64) == -1 and b"input width" in err()
    assert count(124, 3, 2, 2, 2, 64, 64) > 0
    assert count(4, 1, 2, 2, 2, 64, 64) == -1 and b"n_actions" in err()
    assert count(4, 33, 2, 2, 2, 64, 64) == -1 and b"n_actions" in err()
    assert count(4, 3, 0, 0, 2, 64, 64) == -1 and b"reward_dim" in err()
    assert count(4, 3, 9, 0, 2, 64, 64) == -1 and b"reward_dim" in err()
    assert count(4, 3, 3, 2, 2, 64, 64) == -1 and b"pref_dim" in err()
    assert count(4, 3, 2, 2, 3, 64, 64) == -1 and b"hidden layers" in err()
    assert count(4, 3, 2, 2, 2, 48, 64) == -1 and b"hidden width 48" in err()
    assert count(4, 3, 2, 2, 2, 64, 160) == -1 and b"hidden width 160" in err()
    assert count(4, 3, 2, 0, 1, 64, 7) == (6 * 64 + 64 + 2 * 64 + 2) + (6 * 64 + 64 + 3 * 64 + 3)
    h = C.c_void_p()
    assert lib.lib.morl_nlppo_create(C.byref(h), 4, 3, 2, 1, 2, 64, 64, 8) != 0 and b"pref_dim" in err()
    assert lib.lib.morl_nlppo_create(C.byref(h), 4, 3, 2, 2, 2, 64, 64, 0) != 0 and b"max_minibatch" in err()
    P = int(count(4, 3, 2, 2, 2, 64, 32))
    ctx = nm.Ctx(lib, dev, 4, 3, 2, 2, (64, 32), 8, np.full(P, 0.01))
    launches = getattr(lib.lib, "hipsim_launch_count", None)        # the emulator counts launches: a refused call makes none
    if launches is not None:
        launches.restype = C.c_longlong
    refused_at = []
    try:
        w = np.ones(2)
        with pytest.raises(RuntimeError, match="no rollout"):
            ctx.update_n(np.zeros((1, 8), dtype=np.int32), w, 1e-3)
        z = np.zeros
        ctx.set_rollout(z((8, 4)), z((8, 2)), z(8), z(8), z((8, 2)), z(8), z((8, 2)), None, 8, 1)
        with pytest.raises(RuntimeError, match="no advantages"):
            ctx.update_n(np.zeros((1, 8), dtype=np.int32), w, 1e-3)
        ctx.gae(z((1, 2)), z(1), 0.99, 0.95)
        before = ctx.params.cpu().numpy()
        refused_at.append(launches() if launches is not None else 0)
        with pytest.raises(RuntimeError, match="minibatch"):
            ctx.update_n(np.zeros((1, 9), dtype=np.int32), w, 1e-3)
        with pytest.raises(RuntimeError, match="norm_adv"):
            ctx.update_n(np.zeros((1, 1), dtype=np.int32), w, 1e-3)
        with pytest.raises(RuntimeError, match="rows"):
            ctx.lib.check(lib.lib.morl_nlppo_forward(ctx.h, ctx.params.data_ptr(), ctx.params.data_ptr(), ctx.params.data_ptr(), None,
                                                     0, 1, None, ctx.params.data_ptr(), None))
        refused_at.append(launches() if launches is not None else 0)
        assert refused_at[0] == refused_at[1], "a refused call launched a kernel"
        assert np.array_equal(before, ctx.params.cpu().numpy()), "a refused call changed the parameters"
        assert ctx.update_n(np.zeros((1, 1), dtype=np.int32), w, 1e-3, norm_adv=False).shape == (1, 8)
    finally:
        ctx.close()


def test_action_indices_outside_the_range_are_clamped(be):
    c = nc.BY_NAME["a"]
    g = dict(nm.load(c.name))
    lib, dev = be
    runs = []
    for lo, hi in ((0, c.A - 1), (-5, c.A + 40)):
        acts = g["actions"].copy()
        gg = dict(g, actions=np.where(acts == 0, lo, np.where(acts == c.A - 1, hi, acts)).astype(np.int32))
        ctx = nm.Ctx(lib, dev, c.D, c.A, c.R, c.pref_dim, nc.HIDDEN, c.M, g["p0"])
        try:
            ctx.set_batch(gg)
            stats = ctx.update_n(g["idx"][None], g["weights"], c.lr, **nm.step_kwargs(c))
            runs.append((stats, ctx.params.cpu().numpy()))
        finally:
            ctx.close()
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])
