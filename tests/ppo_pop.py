"""TEST INFRASTRUCTURE: a thin driver of the population entries of the ``morl_ppo_*`` C ABI (``morl_ppo_update_n_pop``,
``morl_ppo_forward_pop``, ``morl_ppo_gae_pop``) over ``ppo_common.Ctx`` objects, and seeded learners to run them on.

The population tests compare two code paths of the same arithmetic bit for bit, so the inputs only have to be finite and
different per learner: they are drawn from a seeded numpy generator, nothing is recorded."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch as th

import ppo_common as pm

CHUNK = 16      # PPO_POP_CHUNK of csrc/ppo_kernels.h: learners per launch


def ptrs(tensors):
    """A host array of device pointers (None -> NULL)."""
    return (C.c_void_p * len(tensors))(*[None if t is None else t.data_ptr() for t in tensors])


def handles(ctxs):
    return (C.c_void_p * len(ctxs))(*[c.h for c in ctxs])


def param_count(lib, D, A, R, hidden):
    return int(lib.lib.morl_ppo_param_count(D, A, R, *pm.hidden_args(hidden)))


def make_learner(lib, dev, seed, D, A, R, hidden, T, E, max_minibatch, steps_done=0, with_moments=False, gae=True):
    """A context with seeded parameters (and moments), a seeded rollout of T x E rows and, with ``gae``, its advantages."""
    rng = np.random.default_rng(seed)
    P = param_count(lib, D, A, R, hidden)
    params = (0.1 * rng.standard_normal(P)).astype(np.float32)
    m = (0.01 * rng.standard_normal(P)).astype(np.float32) if with_moments else None
    v = (1e-4 * rng.random(P)).astype(np.float32) if with_moments else None
    c = pm.Ctx(lib, dev, D, A, R, hidden, max_minibatch, params, m, v, steps_done=steps_done)
    n = T * E
    c.roll_np = dict(obs=rng.standard_normal((n, D)), actions=rng.standard_normal((n, A)),
                     logprobs=-0.5 * A - 0.5 * rng.random(n) * A, rewards=rng.standard_normal((n, R)),
                     dones=(rng.random(n) < 0.2).astype(np.float32), values=rng.standard_normal((n, R)))
    c.gae_np = dict(next_value=rng.standard_normal((E, R)), next_done=(rng.random(E) < 0.5).astype(np.float32),
                    weights=rng.random(R) + 0.1)
    c.TE = (T, E)
    r = c.roll_np
    c.set_rollout(r["obs"], r["actions"], r["logprobs"], r["rewards"], r["dones"], r["values"], T, E)
    if gae:
        c.gae(c.gae_np["next_value"], c.gae_np["next_done"], c.gae_np["weights"], 0.99, 0.95)
    return c


def state(c):
    """(params, exp_avg, exp_avg_sq) as numpy."""
    return tuple(t.cpu().numpy().copy() for t in (c.params, c.m, c.v))


def update_n_pop_raw(lib, ctxs, idx_dev, stats_dev, M, n, lrs, steps, clip_coef=0.2, ent_coef=0.0, vf_coef=0.5, max_grad_norm=0.5,
                     clip_vloss=True, norm_adv=True, handle_array=None):
    """The bare call; returns its status code (nothing is checked or read back)."""
    P = len(ctxs)
    return lib.lib.morl_ppo_update_n_pop(
        P, handle_array if handle_array is not None else handles(ctxs), ptrs([c.params for c in ctxs]), ptrs([c.m for c in ctxs]),
        ptrs([c.v for c in ctxs]), n, ptrs(idx_dev), M, (C.c_double * P)(*[float(x) for x in lrs]), (C.c_int * P)(*[int(s) for s in steps]),
        float(clip_coef), float(ent_coef), float(vf_coef), float(max_grad_norm), int(clip_vloss), int(norm_adv), ptrs(stats_dev),
        lib.stream_of(ctxs[0].params))


def update_n_pop(lib, ctxs, idx, lrs, **kw):
    """idx: per learner [n][M]; one ``morl_ppo_update_n_pop`` call; returns the learners' statistics, each [n][8], as numpy."""
    dev = ctxs[0].dev
    idx = [np.ascontiguousarray(i, dtype=np.int32) for i in idx]
    n, M = idx[0].shape
    idx_dev = [th.tensor(i).to(dev) for i in idx]
    stats = [th.zeros(n, 8, dtype=th.float32, device=dev) for _ in ctxs]
    lib.check(update_n_pop_raw(lib, ctxs, idx_dev, stats, M, n, lrs, [c.steps_done for c in ctxs], **kw))
    for c in ctxs:
        c.steps_done += n
    return [s.cpu().numpy() for s in stats]


def forward_pop(lib, ctxs, obs, eps=None, value_only=False):
    """obs / eps per learner; returns per learner (action, logprob, value) as numpy (None, None, value with ``value_only``)."""
    dev = ctxs[0].dev
    o = [c.T(x, (-1, c.D)) for c, x in zip(ctxs, obs)]
    rows = o[0].shape[0]
    val = [th.zeros(rows, c.R, dtype=th.float32, device=dev) for c in ctxs]
    P = len(ctxs)
    if value_only:
        lib.check(lib.lib.morl_ppo_forward_pop(P, handles(ctxs), ptrs([c.params for c in ctxs]), ptrs(o), None, rows, 1, None, None,
                                               ptrs(val), lib.stream_of(val[0])))
        return [(None, None, v.cpu().numpy()) for v in val]
    e = [c.T(x, (rows, c.A)) for c, x in zip(ctxs, eps)]
    act = [th.zeros(rows, c.A, dtype=th.float32, device=dev) for c in ctxs]
    lp = [th.zeros(rows, dtype=th.float32, device=dev) for c in ctxs]
    lib.check(lib.lib.morl_ppo_forward_pop(P, handles(ctxs), ptrs([c.params for c in ctxs]), ptrs(o), ptrs(e), rows, 0, ptrs(act),
                                           ptrs(lp), ptrs(val), lib.stream_of(val[0])))
    return [(a.cpu().numpy(), l.cpu().numpy(), v.cpu().numpy()) for a, l, v in zip(act, lp, val)]


def gae_pop(lib, ctxs, gamma, gae_lambda, use_gae=True):
    """The learners' own ``gae_np`` inputs; returns per learner (returns, advantages) as numpy."""
    dev = ctxs[0].dev
    nv = [c.T(c.gae_np["next_value"], (-1, c.R)) for c in ctxs]
    nd = [c.T(c.gae_np["next_done"], (-1,)) for c in ctxs]
    w = [c.T(c.gae_np["weights"], (c.R,)) for c in ctxs]
    ret = [th.zeros(c.n_rows, c.R, dtype=th.float32, device=dev) for c in ctxs]
    adv = [th.zeros(c.n_rows, dtype=th.float32, device=dev) for c in ctxs]
    lib.check(lib.lib.morl_ppo_gae_pop(len(ctxs), handles(ctxs), ptrs(nv), ptrs(nd), ptrs(w), float(gamma), float(gae_lambda),
                                       int(use_gae), ptrs(ret), ptrs(adv), lib.stream_of(ret[0])))
    return [(r.cpu().numpy(), a.cpu().numpy()) for r, a in zip(ret, adv)]
