"""Shared by the NL-MO-PPO tests: fixtures, the backend selector, the tolerances and a thin driver of the ``morl_nlppo_*`` C ABI."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np
import torch as th

from pcn_common import BACKENDS, backend, close_rel  # noqa: F401  (re-exported: one selector for every family)
from ppo_common import hidden_args, one_thread  # noqa: F401

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
STATS = ("loss", "pg_loss", "v_loss", "entropy", "old_approx_kl", "approx_kl", "clipfrac", "grad_norm")
ATOL = 1e-6
GUARD = 7            # rows of a sentinel behind every output
SENTINEL = -777.0


def load(name):
    return np.load(os.path.join(GOLDEN_DIR, f"nlppo_{name}.npz"))


def stat_atol(weights):
    """The absolute terms of the contract: 1e-6 for the two KLs (means of differences of O(1) log-probabilities) and
    1e-6 * max(1, sum_k |w_k|) for pg_loss and loss, whose terms are O(sum |w_k|) while their mean is not."""
    wa = ATOL * max(1.0, float(np.abs(np.asarray(weights, dtype=np.float64)).sum()))
    return {"loss": wa, "pg_loss": wa, "old_approx_kl": ATOL, "approx_kl": ATOL}


def check_stats(got, want, weights, tag=""):
    atol = stat_atol(weights)
    for i, name in enumerate(STATS):
        if name == "clipfrac":
            assert np.array_equal(got[..., i], want[..., i]), (tag, name, got[..., i], want[..., i])
        else:
            close_rel(f"{tag}{name}", got[..., i], want[..., i], 1e-5, atol.get(name, 0.0))


class Ctx:
    """One ``morl_nlppo_ctx`` with its flat parameter / moment tensors on ``dev``.  Every output buffer has ``GUARD`` sentinel rows
    behind it, which every call checks."""

    def __init__(self, lib, dev, D, A, R, pref_dim, hidden, max_minibatch, params, exp_avg=None, exp_avg_sq=None, steps_done=0):
        self.lib, self.dev, self.D, self.A, self.R, self.pref_dim = lib, dev, D, A, R, pref_dim
        P = int(lib.lib.morl_nlppo_param_count(D, A, R, pref_dim, *hidden_args(hidden)))
        assert P == len(params), (P, len(params))
        h = C.c_void_p()
        lib.check(lib.lib.morl_nlppo_create(C.byref(h), D, A, R, pref_dim, *hidden_args(hidden), max_minibatch))
        self.h = h.value
        self.params = self.T(params)
        self.m = self.T(exp_avg) if exp_avg is not None else th.zeros_like(self.params)
        self.v = self.T(exp_avg_sq) if exp_avg_sq is not None else th.zeros_like(self.params)
        self.steps_done = steps_done

    def T(self, a, shape=None, dtype=np.float32):
        a = np.ascontiguousarray(np.asarray(a, dtype=dtype))
        return th.tensor(a if shape is None else a.reshape(shape)).to(self.dev)

    def out(self, rows, width=None):
        shape = (rows + GUARD,) if width is None else (rows + GUARD, width)
        return th.full(shape, SENTINEL, dtype=th.float32, device=self.dev)

    @staticmethod
    def take(buf, rows):
        a = buf.cpu().numpy()
        assert (a[rows:] == SENTINEL).all(), "a kernel wrote behind its output"
        return a[:rows]

    def close(self):
        if self.h:
            self.lib.lib.morl_nlppo_destroy(self.h)
            self.h = None

    def set_rollout(self, obs, acc_rewards, actions, logprobs, rewards, dones, values, pref, T, E):
        n = T * E
        self.roll = [self.T(obs, (n, self.D)), self.T(acc_rewards, (n, self.R)), self.T(actions, (n,), np.int32), self.T(logprobs, (n,)),
                     self.T(rewards, (n, self.R)), self.T(dones, (n,)), self.T(values, (n, self.R))]
        self.pref = None if (pref is None or self.pref_dim == 0) else self.T(pref, (self.pref_dim,))
        self.n_rows = n
        self.lib.check(self.lib.lib.morl_nlppo_set_rollout(self.h, *[t.data_ptr() for t in self.roll],
                                                           None if self.pref is None else self.pref.data_ptr(), T, E,
                                                           self.lib.stream_of(self.params)))

    def gae(self, next_value, next_done, gamma, gae_lambda):
        """Returns (returns [T*E][R], advantages [T*E][R]) as numpy."""
        nv, nd = self.T(next_value, (-1, self.R)), self.T(next_done, (-1,))
        ret, adv = self.out(self.n_rows, self.R), self.out(self.n_rows, self.R)
        self.lib.check(self.lib.lib.morl_nlppo_gae(self.h, nv.data_ptr(), nd.data_ptr(), float(gamma), float(gae_lambda), ret.data_ptr(),
                                                   adv.data_ptr(), self.lib.stream_of(ret)))
        return self.take(ret, self.n_rows), self.take(adv, self.n_rows)

    def set_batch(self, g):
        """A single-step fixture's rows.  Their advantages and returns are those of a rollout of M steps of one env with gamma = 0
        (advantages = rewards - values, returns = advantages + values), which is how they get into the table here."""
        M = len(g["logprobs"])
        self.set_rollout(g["obs"], g["acc_rewards"], g["actions"], g["logprobs"], g["rewards"], np.zeros(M), g["values"],
                         g["pref"] if "pref" in g else None, M, 1)
        return self.gae(np.zeros((1, self.R)), np.zeros(1), 0.0, 0.0)

    def update_n(self, idx, weights, lr, clip_coef=0.2, ent_coef=0.01, vf_coef=0.5, max_grad_norm=0.5, clip_vloss=True, norm_adv=True):
        """idx [n][M]; returns the steps' statistics [n][8] as numpy."""
        idx = np.ascontiguousarray(idx, dtype=np.int32).reshape(-1, np.asarray(idx).shape[-1])
        n, M = idx.shape
        idx_d = th.tensor(idx).to(self.dev)
        w = self.T(weights, (self.R,))
        stats = self.out(n, 8)
        self.lib.check(self.lib.lib.morl_nlppo_update_n(self.h, self.params.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), n,
                                                        idx_d.data_ptr(), M, w.data_ptr(), float(lr), self.steps_done, float(clip_coef),
                                                        float(ent_coef), float(vf_coef), float(max_grad_norm), int(clip_vloss),
                                                        int(norm_adv), stats.data_ptr(), self.lib.stream_of(stats)))
        self.steps_done += n
        return self.take(stats, n)

    def forward(self, obs, acc_reward, pref=None, value_only=False):
        """(logp [rows][A], value [rows][R]) as numpy; ``value_only``: (None, value)."""
        o = self.T(obs, (-1, self.D))
        rows = o.shape[0]
        a = self.T(acc_reward, (rows, self.R))
        p = None if (pref is None or self.pref_dim == 0) else self.T(pref, (self.pref_dim,))
        val = self.out(rows, self.R)
        lp = None if value_only else self.out(rows, self.A)
        self.lib.check(self.lib.lib.morl_nlppo_forward(self.h, self.params.data_ptr(), o.data_ptr(), a.data_ptr(),
                                                       None if p is None else p.data_ptr(), rows, int(value_only),
                                                       None if lp is None else lp.data_ptr(), val.data_ptr(), self.lib.stream_of(val)))
        return (None if lp is None else self.take(lp, rows)), self.take(val, rows)


def step_kwargs(c):
    return dict(clip_coef=c.clip_coef, ent_coef=c.ent_coef, vf_coef=c.vf_coef, max_grad_norm=c.max_grad_norm, clip_vloss=c.clip_vloss,
                norm_adv=c.norm_adv)
