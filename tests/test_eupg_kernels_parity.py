"""EUPG through the C ABI (``morl_eupg_*``) against fixtures recorded from the reference.

``sim`` runs the unmodified kernel sources under the host wave emulator (CPU), ``hip`` the gfx950 library (-m gpu).
Tolerances are the project's contract as ``test_pcn_kernels_parity.py`` states it: probabilities and loss 1e-5 relative (+ 1e-6
near 0); stepped parameters within 2e-5 relative + 0.02 * lr; the moments as there.  The returns of the scan are EXACT."""
import numpy as np
import pytest

import eupg_cases as ec
import eupg_common as em


@pytest.fixture(scope="module", params=em.BACKENDS)
def be(request):
    return em.backend(request.param)


def step_ctx(be, c, g, max_workgroups=None, p0=None, moments=True):
    lib, dev = be
    m0, v0 = ec.synthetic_moments(c.seed, len(g["p0"])) if moments else (None, None)
    ctx = em.Ctx(lib, dev, c.D, c.A, c.R, c.hidden, g["p0"] if p0 is None else p0, m0, v0, steps_done=c.step if moments else 0,
                 max_rows=max(c.T, 1), max_workgroups=c.max_workgroups if max_workgroups is None else max_workgroups)
    ctx.set_episode(g["obs"], g["acc_rewards"], g["actions"], g["rewards"])
    return ctx


def run_step(be, c, g, **kw):
    ctx = step_ctx(be, c, g, **kw)
    try:
        G = ctx.returns(c.gamma)
        loss = ctx.update(g["u"], c.lr)
        return G, ctx.state(loss, ctx.step_probs())
    finally:
        ctx.close()


@pytest.mark.parametrize("c", ec.STEP_CASES, ids=lambda c: c.name)
def test_single_step_matches_the_reference(be, c):
    g = em.load(c.name)
    ctx = step_ctx(be, c, g)
    try:
        G = ctx.returns(c.gamma)
        assert np.array_equal(G, g["returns"]), "the scan's returns are not the reference's bit for bit"
        fwd = ctx.forward(em.eo.truncate_obs(g["obs"]), g["acc_rewards"])
        em.close_rel("forward probabilities", fwd, g["probs"], 1e-5, em.ATOL)
        # the utility is the caller's: torch, on the scan's output
        u = ec.utility(em.th.tensor(G)).numpy()
        assert np.array_equal(u, g["u"])
        loss = ctx.update(u, c.lr)
        em.check_step(ctx.state(loss, ctx.step_probs()), g, c.lr)
    finally:
        ctx.close()


def test_clamped_rows_contribute_nothing(be):
    """Case e: action 0 has a probability below eps in every row.  The rows that took it have logp = log(eps) and no gradient: the
    step from the episode equals (within the contract) the reference's, and the head's bias of action 0 -- whose gradient comes
    through the normaliser of the other rows alone -- moves as the reference's does."""
    c = ec.BY_NAME["e"]
    g = em.load("e")
    took0 = g["actions"] == 0
    assert took0.mean() >= 0.1 and (~took0).mean() >= 0.1 and (g["probs"][:, 0] < ec.EPS).all()
    assert (g["logp"][took0] == np.log(np.float32(ec.EPS))).all()
    _, got = run_step(be, c, g)
    em.check_step(got, g, c.lr)
    # with u = 0 on every row that did NOT take action 0, nothing is left: the loss is -mean(log(eps) * u) and no gradient flows
    u = np.where(took0, g["u"], 0.0).astype(np.float32)
    ctx = step_ctx(be, c, g, moments=False)
    try:
        loss = ctx.update(u, c.lr)
        want = -np.sum(np.log(np.float64(ec.EPS)) * u.astype(np.float64)) / c.T
        em.close_rel("loss of clamped rows", loss, want, 1e-5, em.ATOL)
        assert np.array_equal(ctx.params.cpu().numpy(), g["p0"]), "a clamped row moved a parameter"
        assert not ctx.m.cpu().numpy().any() and not ctx.v.cpu().numpy().any()
    finally:
        ctx.close()


@pytest.mark.parametrize("name", ["a", "c"])
def test_two_runs_are_bit_identical(be, name):
    c, g = ec.BY_NAME[name], em.load(name)
    (G1, a), (G2, b) = run_step(be, c, g), run_step(be, c, g)
    assert np.array_equal(G1, G2)
    for k in a:
        assert np.array_equal(a[k], b[k]), f"{k}: two identical runs differ"


def test_grid_sizes_agree_within_the_contract(be):
    """70 rows are 5 tiles: one workgroup owns all of them, two own 3 + 2, the default grid one each.  The partials are added in
    another order, so the results need not be equal bit for bit; each is held to the contract."""
    c, g = ec.BY_NAME["c"], em.load("c")
    runs = [run_step(be, c, g, max_workgroups=w)[1] for w in (1, 2, 0)]
    for r in runs:
        em.check_step(r, g, c.lr)
    for r in runs[1:]:
        assert np.array_equal(r["probs"], runs[0]["probs"]), "the rows' probabilities do not depend on the grid"
        em.close_rel("parameters across grids", r["p1"], runs[0]["p1"], 2e-5, 0.02 * c.lr)


@pytest.mark.parametrize("name", ["a", "c", "d"])
def test_a_step_forms_the_probabilities_the_forward_returns(be, name):
    """While the parameters are unchanged, the forward launch on the episode's rows gives the step kernel's probabilities bit for
    bit (one device function normalises the rows in both)."""
    c, g = ec.BY_NAME[name], em.load(name)
    ctx = step_ctx(be, c, g)
    try:
        fwd = ctx.forward(em.eo.truncate_obs(g["obs"]), g["acc_rewards"])
        for rows in (1, 15, 16, 17, 33):
            if rows <= c.T:
                assert np.array_equal(ctx.forward(em.eo.truncate_obs(g["obs"])[:rows], g["acc_rewards"][:rows]), fwd[:rows]), rows
        with pytest.raises(RuntimeError, match="no step"):
            ctx.step_probs()
        ctx.update(g["u"], c.lr)
        assert np.array_equal(ctx.step_probs(), fwd)
        assert not np.array_equal(ctx.forward(em.eo.truncate_obs(g["obs"]), g["acc_rewards"]), fwd), "the step changed nothing"
    finally:
        ctx.close()


def test_action_indices_outside_the_range_are_clamped(be):
    c, g = ec.BY_NAME["a"], dict(em.load("a"))
    acts = g["actions"]
    wild = np.where(acts == 0, -5, np.where(acts == c.A - 1, c.A + 40, acts)).astype(np.int32)
    a = run_step(be, c, g)[1]
    b = run_step(be, c, dict(g, actions=wild))[1]
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def test_a_context_is_reused_across_episodes(be):
    """A shorter episode after a longer one in the same context: nothing of the longer one is left in the step."""
    c, g = ec.BY_NAME["a"], em.load("a")
    d, gd = ec.BY_NAME["d"], em.load("d")
    assert (c.D, c.A, c.R, c.hidden) == (d.D, d.A, d.R, d.hidden)
    lib, dev = be
    m0, v0 = ec.synthetic_moments(d.seed, len(gd["p0"]))
    ctx = em.Ctx(lib, dev, c.D, c.A, c.R, c.hidden, g["p0"], max_rows=c.T)
    try:
        ctx.set_episode(g["obs"], g["acc_rewards"], g["actions"], g["rewards"])
        ctx.update(g["u"], c.lr)
        ctx.params, ctx.m, ctx.v, ctx.steps_done = ctx.T(gd["p0"]), ctx.T(m0), ctx.T(v0), d.step
        ctx.set_episode(gd["obs"], gd["acc_rewards"], gd["actions"], gd["rewards"])
        assert np.array_equal(ctx.returns(d.gamma), gd["returns"])
        loss = ctx.update(gd["u"], d.lr)
        em.check_step(ctx.state(loss, ctx.step_probs()), gd, d.lr)
    finally:
        ctx.close()
