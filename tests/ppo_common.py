"""Shared by the MO-PPO tests: fixtures, the backend selector and a thin driver of the ``morl_ppo_*`` C ABI."""
from __future__ import annotations

import contextlib
import ctypes as C
import os

import numpy as np
import torch as th

from pcn_common import BACKENDS, backend, close_rel  # noqa: F401  (re-exported: one selector for both families)

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
STATS = ("loss", "pg_loss", "v_loss", "entropy", "old_approx_kl", "approx_kl", "clipfrac", "grad_norm")


def load(name):
    return np.load(os.path.join(GOLDEN_DIR, f"ppo_{name}.npz"))


@contextlib.contextmanager
def one_thread():
    """The fixtures were recorded with one intra-op thread: ``orthogonal_`` (a QR factorisation) and the larger matrix products
    give the same bits only at the same thread count.  Restores the count on exit."""
    n = th.get_num_threads()
    th.set_num_threads(1)
    try:
        yield
    finally:
        th.set_num_threads(n)


def hidden_args(hidden):
    return len(hidden), int(hidden[0]), int(hidden[1]) if len(hidden) > 1 else 0


class Ctx:
    """One ``morl_ppo_ctx`` with its flat parameter / moment tensors on ``dev``."""

    def __init__(self, lib, dev, D, A, R, hidden, max_minibatch, params, exp_avg=None, exp_avg_sq=None, steps_done=0):
        self.lib, self.dev, self.D, self.A, self.R = lib, dev, D, A, R
        P = int(lib.lib.morl_ppo_param_count(D, A, R, *hidden_args(hidden)))
        assert P == len(params), (P, len(params))
        h = C.c_void_p()
        lib.check(lib.lib.morl_ppo_create(C.byref(h), D, A, R, *hidden_args(hidden), max_minibatch))
        self.h = h.value
        self.params = self.T(params)
        self.m = self.T(exp_avg) if exp_avg is not None else th.zeros_like(self.params)
        self.v = self.T(exp_avg_sq) if exp_avg_sq is not None else th.zeros_like(self.params)
        self.steps_done = steps_done

    def T(self, a, shape=None):
        a = np.ascontiguousarray(np.asarray(a, dtype=np.float32))
        return th.tensor(a if shape is None else a.reshape(shape)).to(self.dev)

    def close(self):
        if self.h:
            self.lib.lib.morl_ppo_destroy(self.h)
            self.h = None

    def set_rollout(self, obs, actions, logprobs, rewards, dones, values, T, E):
        n = T * E
        self.roll = [self.T(obs, (n, self.D)), self.T(actions, (n, self.A)), self.T(logprobs, (n,)), self.T(rewards, (n, self.R)),
                     self.T(dones, (n,)), self.T(values, (n, self.R))]
        self.n_rows = n
        self.lib.check(self.lib.lib.morl_ppo_set_rollout(self.h, *[t.data_ptr() for t in self.roll], T, E,
                                                         self.lib.stream_of(self.params)))

    def gae(self, next_value, next_done, weights, gamma, gae_lambda, use_gae=True):
        """Returns (returns [T*E][R], scalarised advantages [T*E]) as numpy."""
        nv, nd, w = self.T(next_value, (-1, self.R)), self.T(next_done, (-1,)), self.T(weights, (self.R,))
        ret = th.zeros(self.n_rows, self.R, dtype=th.float32, device=self.dev)
        adv = th.zeros(self.n_rows, dtype=th.float32, device=self.dev)
        self.lib.check(self.lib.lib.morl_ppo_gae(self.h, nv.data_ptr(), nd.data_ptr(), w.data_ptr(), float(gamma), float(gae_lambda),
                                                 int(use_gae), ret.data_ptr(), adv.data_ptr(), self.lib.stream_of(ret)))
        return ret.cpu().numpy(), adv.cpu().numpy()

    def set_batch(self, g):
        """A single-step fixture's rows.  Their returns and advantages are those of a rollout of M steps of one env with gamma = 0
        and no GAE (returns = rewards, advantage = (returns - values) @ weights), which is how they get into the table here."""
        M = len(g["logprobs"])
        self.set_rollout(g["obs"], g["actions"], g["logprobs"], g["returns"], np.zeros(M), g["values"], M, 1)
        return self.gae(np.zeros((1, self.R)), np.zeros(1), g["weights"], 0.0, 0.0, use_gae=False)

    def update_n(self, idx, lr, clip_coef=0.2, ent_coef=0.0, vf_coef=0.5, max_grad_norm=0.5, clip_vloss=True, norm_adv=True):
        """idx [n][M]; returns the steps' statistics [n][8] as numpy."""
        idx = np.ascontiguousarray(idx, dtype=np.int32).reshape(-1, np.asarray(idx).shape[-1])
        n, M = idx.shape
        idx_d = th.tensor(idx).to(self.dev)
        stats = th.zeros(n, 8, dtype=th.float32, device=self.dev)
        self.lib.check(self.lib.lib.morl_ppo_update_n(self.h, self.params.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), n,
                                                      idx_d.data_ptr(), M, float(lr), self.steps_done, float(clip_coef),
                                                      float(ent_coef), float(vf_coef), float(max_grad_norm), int(clip_vloss),
                                                      int(norm_adv), stats.data_ptr(), self.lib.stream_of(stats)))
        self.steps_done += n
        return stats.cpu().numpy()

    def forward(self, obs, eps=None, value_only=False):
        """(action [rows][A], logprob [rows], value [rows][R]) as numpy; ``value_only``: (None, None, value)."""
        o = self.T(obs, (-1, self.D))
        rows = o.shape[0]
        val = th.zeros(rows, self.R, dtype=th.float32, device=self.dev)
        if value_only:
            self.lib.check(self.lib.lib.morl_ppo_forward(self.h, self.params.data_ptr(), o.data_ptr(), None, rows, 1, None, None,
                                                         val.data_ptr(), self.lib.stream_of(val)))
            return None, None, val.cpu().numpy()
        e = self.T(eps, (rows, self.A))
        act = th.zeros(rows, self.A, dtype=th.float32, device=self.dev)
        lp = th.zeros(rows, dtype=th.float32, device=self.dev)
        self.lib.check(self.lib.lib.morl_ppo_forward(self.h, self.params.data_ptr(), o.data_ptr(), e.data_ptr(), rows, 0,
                                                     act.data_ptr(), lp.data_ptr(), val.data_ptr(), self.lib.stream_of(val)))
        return act.cpu().numpy(), lp.cpu().numpy(), val.cpu().numpy()
