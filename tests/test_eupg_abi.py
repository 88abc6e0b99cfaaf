"""Argument validation of the ``morl_eupg_*`` entries: every refusal is ``MORL_ERR_ARG`` (-1) with a message, launches nothing and
leaves the context usable.  No GPU: the shape checks run on the gfx950 library too (they come before any device call), the ones
that need a context on the host-emulated build."""
import ctypes as C

import numpy as np
import pytest

import eupg_common as em
import simlib

ERR_ARG = -1


@pytest.fixture(scope="module")
def sim():
    return simlib.load_sim()


def libs(sim):
    from morl_baselines_amd.native import load_library
    return [sim, load_library()]


def test_shapes_outside_the_limits_are_refused(sim):
    for lib in libs(sim):
        count, create, err = lib.lib.morl_eupg_param_count, lib.lib.morl_eupg_create, lib.lib.morl_last_error
        h = C.c_void_p()
        assert count(4, 3, 2, 1, 50, 0) == (6 * 50 + 50) + (3 * 50 + 3)
        assert count(4, 3, 2, 2, 50, 33) == (6 * 50 + 50) + (50 * 33 + 33) + (3 * 33 + 3)
        assert count(4, 3, 2, 1, 1, 0) > 0 and count(4, 3, 2, 1, 128, 0) > 0 and count(126, 32, 2, 2, 128, 128) > 0
        for bad, word in (((4, 3, 2, 1, 0, 0), b"hidden width 0"), ((4, 3, 2, 1, 129, 0), b"hidden width 129"),
                          ((4, 3, 2, 2, 50, 0), b"hidden width 0"), ((4, 3, 2, 2, 50, 129), b"hidden width 129"),
                          ((4, 33, 2, 1, 50, 0), b"n_actions"), ((4, 1, 2, 1, 50, 0), b"n_actions"),
                          ((0, 3, 2, 1, 50, 0), b"obs_dim"), ((127, 3, 2, 1, 50, 0), b"input width"),
                          ((4, 3, 0, 1, 50, 0), b"reward_dim"), ((4, 3, 9, 1, 50, 0), b"reward_dim"),
                          ((4, 3, 2, 0, 50, 0), b"hidden layers"), ((4, 3, 2, 3, 50, 50), b"hidden layers")):
            assert count(*bad) == -1 and word in err(), (bad, err())
            h.value = 123
            assert create(C.byref(h), *bad, 0, 0) == ERR_ARG and word in err(), (bad, err())
            assert h.value is None, "a refused create left a handle"
        assert create(None, 4, 3, 2, 1, 50, 0, 0, 0) == ERR_ARG and b"NULL" in err()
        assert create(C.byref(h), 4, 3, 2, 1, 50, 0, -1, 0) == ERR_ARG and b"max_rows" in err()
        assert create(C.byref(h), 4, 3, 2, 1, 50, 0, 0, -1) == ERR_ARG and b"max_workgroups" in err()
        assert create(C.byref(h), 4, 3, 2, 1, 50, 0, 0, 1025) == ERR_ARG and b"max_workgroups" in err()
        assert lib.lib.morl_eupg_destroy(None) == 0


def test_calls_on_a_context_are_refused_before_anything_is_launched(sim):
    import torch as th
    L = sim.lib
    err = L.morl_last_error
    launches = L.hipsim_launch_count
    launches.restype = C.c_longlong
    P = int(L.morl_eupg_param_count(4, 3, 2, 1, 50, 0))
    ctx = em.Ctx(sim, th.device("cpu"), 4, 3, 2, (50,), np.full(P, 0.01), max_rows=8)
    try:
        z = lambda *s: th.zeros(*s)  # noqa: E731
        obs, acc, act, rew, out, u = z(9, 4), z(9, 2), z(9).int(), z(9, 2), z(9, 3), z(9)
        p = [t.data_ptr() for t in (obs, acc, act, rew)]
        before, n0 = ctx.params.clone(), launches()
        assert L.morl_eupg_returns(ctx.h, 0.9, out.data_ptr(), None) != 0 and b"no episode" in err()
        assert L.morl_eupg_update(ctx.h, ctx.params.data_ptr(), ctx.m.data_ptr(), ctx.v.data_ptr(), u.data_ptr(), 1e-3, 0,
                                  out.data_ptr(), None) != 0 and b"no episode" in err()
        assert L.morl_eupg_set_episode(ctx.h, *p, 9, None) == ERR_ARG and b"max_rows 8" in err()
        assert L.morl_eupg_set_episode(ctx.h, *p, 0, None) == ERR_ARG and b"max_rows 8" in err()
        for i in range(4):
            q = list(p)
            q[i] = None
            assert L.morl_eupg_set_episode(ctx.h, *q, 8, None) == ERR_ARG and b"NULL" in err(), i
        assert L.morl_eupg_set_episode(None, *p, 8, None) == ERR_ARG and b"NULL" in err()
        assert L.morl_eupg_returns(None, 0.9, out.data_ptr(), None) == ERR_ARG and L.morl_eupg_returns(ctx.h, 0.9, None, None) == ERR_ARG
        assert L.morl_eupg_step_probs(ctx.h, None, None) == ERR_ARG and L.morl_eupg_step_probs(None, out.data_ptr(), None) == ERR_ARG
        assert L.morl_eupg_forward(ctx.h, ctx.params.data_ptr(), obs.data_ptr(), acc.data_ptr(), 0, out.data_ptr(), None) == ERR_ARG \
            and b"rows" in err()
        assert L.morl_eupg_forward(ctx.h, None, obs.data_ptr(), acc.data_ptr(), 1, out.data_ptr(), None) == ERR_ARG and b"NULL" in err()
        assert L.morl_eupg_forward(ctx.h, ctx.params.data_ptr(), obs.data_ptr(), acc.data_ptr(), 1, None, None) == ERR_ARG
        assert launches() == n0, "a refused call launched a kernel"
        ctx.set_episode(np.zeros((8, 4)), np.zeros((8, 2)), np.zeros(8), np.ones((8, 2)))
        args = [ctx.h, ctx.params.data_ptr(), ctx.m.data_ptr(), ctx.v.data_ptr(), u.data_ptr(), 1e-3, 0, out.data_ptr(), None]
        n1 = launches()
        for i in (0, 1, 2, 3, 4, 7):
            q = list(args)
            q[i] = None
            assert L.morl_eupg_update(*q) == ERR_ARG and b"NULL" in err(), i
        q = list(args)
        q[6] = -1
        assert L.morl_eupg_update(*q) == ERR_ARG and b"steps_done" in err()
        assert launches() == n1 and th.equal(before, ctx.params), "a refused call launched a kernel or changed the parameters"
        # the context is still usable
        assert ctx.returns(0.5).shape == (8, 2) and np.isfinite(ctx.update(np.ones(8), 1e-3))
    finally:
        ctx.close()
