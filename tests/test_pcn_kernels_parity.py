"""PCN updates through the C ABI (``morl_pcn_update_n`` / ``morl_pcn_forward``) against fixtures recorded from the reference.

``sim`` runs the unmodified kernel sources under the host wave emulator (CPU), ``hip`` the gfx950 library (-m gpu).
Tolerances are the project's contract for every fused update: loss and predictions 1e-5 relative; stepped parameters within
0.02 * lr per optimiser step (an Adam step moves an entry by at most ~lr, and an entry whose gradient is rounding-sized turns a
1e-9 gradient difference into a fraction of that); indices and greedy actions exact."""
import numpy as np
import pytest

import pcn_cases as pc
import pcn_common as pcm

PRED_ATOL = 1e-6     # log-probabilities / actions that are ~0: 1e-5 relative of the O(1) logits they are differences of


@pytest.fixture(scope="module", params=pcm.BACKENDS)
def be(request):
    return pcm.backend(request.param)


def make_ctx(be, c, g, **kw):
    lib, dev = be
    ctx = pcm.Ctx(lib, dev, c.D, c.R, c.A, c.H, c.continuous, c.B, pcm.flat(g, "p0"), g["scaling"], pcm.flat(g, "m0"),
                  pcm.flat(g, "v0"), steps_done=c.step, **kw)
    ctx.set_table(g["table"])
    return ctx


@pytest.mark.parametrize("c", pc.UPDATE_CASES, ids=lambda c: c.name)
def test_single_update_matches_the_reference(be, c):
    g = pcm.load(c.name)
    ctx = make_ctx(be, c, g)
    try:
        table, idx = g["table"], g["idx"]
        aw = c.A if c.continuous else 1
        # the no-grad forward on the batch's rows is the update's prediction (same parameters, before the step)
        fwd = ctx.forward(table[idx, :c.D], table[idx, c.D + aw:c.D + aw + c.R], table[idx, -1])
        loss, ent, pred = ctx.update_n(idx[None], c.lr, want_entropy=not c.continuous)
        pcm.close_rel("forward", fwd, g["pred"], 1e-5, PRED_ATOL)
        pcm.close_rel("prediction", pred, g["pred"], 1e-5, PRED_ATOL)
        assert np.array_equal(fwd, pred), "the update's forward pass and morl_pcn_forward differ"
        pcm.close_rel("loss", loss[0], g["loss"], 1e-5)
        if not c.continuous:
            assert np.array_equal(pred.argmax(1), g["pred"].argmax(1))
            want_ent = np.sum(-np.exp(g["pred"].astype(np.float64)) * g["pred"])           # pcn.py:463
            pcm.close_rel("entropy", ent[0], want_ent, 1e-5)
        pcm.close_rel("parameters", ctx.params.cpu().numpy(), pcm.flat(g, "p1"), 2e-5, 0.02 * c.lr)
        m_scale = float(np.abs(pcm.flat(g, "m1")).max())
        v_scale = float(np.abs(pcm.flat(g, "v1")).max())
        pcm.close_rel("exp_avg", ctx.m.cpu().numpy(), pcm.flat(g, "m1"), 1e-4, 2e-5 * m_scale)
        pcm.close_rel("exp_avg_sq", ctx.v.cpu().numpy(), pcm.flat(g, "v1"), 2e-4, 2e-5 * v_scale)
    finally:
        ctx.close()


def loop_ctx(be, g):
    L = pc.LOOP
    lib, dev = be
    ctx = pcm.Ctx(lib, dev, 9, 2, 4, L["H"], False, L["B"], pcm.flat(g, "p0"), g["scaling"])
    ctx.set_table(g["table"])
    return ctx


def test_fifty_update_loop_matches_the_reference(be):
    g, L = pcm.load("loop50"), pc.LOOP
    ctx = loop_ctx(be, g)
    try:
        losses, _, pred = ctx.update_n(g["idx"], L["lr"])
        pcm.close_rel("losses", losses, g["losses"], 1e-5)
        pcm.close_rel("last prediction", pred, g["pred"], 1e-5, PRED_ATOL)
        pcm.close_rel("parameters", ctx.params.cpu().numpy(), pcm.flat(g, "p1"), 2e-5, 0.02 * L["lr"] * L["n"])
    finally:
        ctx.close()


def test_update_n_is_n_single_updates_and_runs_are_bit_identical(be):
    """One entry for n steps == n entries for one step each, bit for bit; and the same call twice gives the same bits (fixed
    reduction order, no floating-point atomics)."""
    g, L = pcm.load("loop50"), pc.LOOP
    n = 6
    idx = g["idx"][:n]
    runs = []
    for split in (False, False, True):
        ctx = loop_ctx(be, g)
        try:
            if split:
                out = [ctx.update_n(idx[k:k + 1], L["lr"], want_entropy=True) for k in range(n)]
                losses, ents, pred = np.concatenate([o[0] for o in out]), np.concatenate([o[1] for o in out]), out[-1][2]
            else:
                losses, ents, pred = ctx.update_n(idx, L["lr"], want_entropy=True)
            runs.append((losses, ents, pred, ctx.params.cpu().numpy(), ctx.m.cpu().numpy(), ctx.v.cpu().numpy()))
        finally:
            ctx.close()
    for name, a, b, c in zip(("loss", "entropy", "prediction", "parameters", "exp_avg", "exp_avg_sq"), *runs):
        assert np.array_equal(a, b), f"{name}: two identical runs differ"
        assert np.array_equal(a, c), f"{name}: update_n({n}) differs from {n} x update_n(1)"


def test_forward_rows_and_refusals(be):
    """Row counts around the 16-row tile, and the loud refusals of the C ABI."""
    import ctypes as C
    lib, dev = be
    c = pc.BY_NAME["disc_b50"]
    g = pcm.load(c.name)
    ctx = make_ctx(be, c, g)
    try:
        table, idx = g["table"], g["idx"]
        args = (table[idx, :c.D], table[idx, c.D + 1:c.D + 1 + c.R], table[idx, -1])
        full = ctx.forward(*args)
        for rows in (1, 15, 16, 17, 33):
            part = ctx.forward(*(a[:rows] for a in args))
            assert np.array_equal(part, full[:rows]), rows
        with pytest.raises(RuntimeError, match="batch"):
            ctx.update_n(np.zeros((1, c.B + 1), dtype=np.int32), c.lr)
    finally:
        ctx.close()
    assert lib.lib.morl_pcn_param_count(4, 2, 3, 48) == -1 and b"hidden_dim" in lib.lib.morl_last_error()
    assert lib.lib.morl_pcn_param_count(129, 2, 3, 64) == -1 and b"state_dim" in lib.lib.morl_last_error()
    assert lib.lib.morl_pcn_param_count(4, 9, 3, 64) == -1 and b"reward_dim" in lib.lib.morl_last_error()
    assert lib.lib.morl_pcn_param_count(4, 2, 33, 64) == -1 and b"action_dim" in lib.lib.morl_last_error()
    h = C.c_void_p()
    assert lib.lib.morl_pcn_create(C.byref(h), 4, 2, 3, 64, 0, 8) == 0
    try:    # no table yet
        one = pcm.Ctx.__new__(pcm.Ctx)
        one.lib, one.dev, one.A, one.h, one.steps_done = lib, dev, 3, h.value, 0
        import torch as th
        one.params = th.zeros(int(lib.lib.morl_pcn_param_count(4, 2, 3, 64)), device=dev)
        one.m, one.v, one.scaling = th.zeros_like(one.params), th.zeros_like(one.params), th.ones(3, device=dev)
        with pytest.raises(RuntimeError, match="transition table"):
            one.update_n(np.zeros((1, 8), dtype=np.int32), 1e-3)
    finally:
        lib.lib.morl_pcn_destroy(h)
