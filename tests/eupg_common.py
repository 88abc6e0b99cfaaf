"""Shared by the EUPG tests: fixtures, the backend selector, the contract's checks and a thin driver of the ``morl_eupg_*`` C ABI."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np
import torch as th

import eupg_oracle as eo
from pcn_common import BACKENDS, backend, close_rel  # noqa: F401  (re-exported: one selector for every family)
from ppo_common import hidden_args, one_thread  # noqa: F401

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ATOL = 1e-6
GUARD = 7            # rows of a sentinel behind every output
SENTINEL = -777.0


def load(name):
    return np.load(os.path.join(GOLDEN_DIR, f"eupg_{name}.npz"))


def check_step(got, want, lr, tag=""):
    """The single-step contract of ``test_pcn_kernels_parity.py``: probabilities and loss 1e-5 relative (+ 1e-6 near 0), stepped
    parameters 2e-5 relative + 0.02 * lr, the moments as there.  ``got`` / ``want``: dicts with probs, loss, p1, m1, v1."""
    close_rel(f"{tag}probabilities", got["probs"], want["probs"], 1e-5, ATOL)
    close_rel(f"{tag}loss", got["loss"], want["loss"], 1e-5, ATOL)
    close_rel(f"{tag}parameters", got["p1"], want["p1"], 2e-5, 0.02 * lr)
    close_rel(f"{tag}exp_avg", got["m1"], want["m1"], 1e-4, 2e-5 * float(np.abs(want["m1"]).max()))
    close_rel(f"{tag}exp_avg_sq", got["v1"], want["v1"], 2e-4, 2e-5 * float(np.abs(want["v1"]).max()))


class Ctx:
    """One ``morl_eupg_ctx`` with its flat parameter / moment tensors on ``dev``.  Every output buffer has ``GUARD`` sentinel rows
    behind it, which every call checks."""

    def __init__(self, lib, dev, D, A, R, hidden, params, exp_avg=None, exp_avg_sq=None, steps_done=0, max_rows=0, max_workgroups=0):
        self.lib, self.dev, self.D, self.A, self.R = lib, dev, D, A, R
        P = int(lib.lib.morl_eupg_param_count(D, A, R, *hidden_args(hidden)))
        assert P == len(params), (P, len(params))
        h = C.c_void_p()
        lib.check(lib.lib.morl_eupg_create(C.byref(h), D, A, R, *hidden_args(hidden), max_rows, max_workgroups))
        self.h = h.value
        self.params = self.T(params)
        self.m = self.T(exp_avg) if exp_avg is not None else th.zeros_like(self.params)
        self.v = self.T(exp_avg_sq) if exp_avg_sq is not None else th.zeros_like(self.params)
        self.steps_done = steps_done
        self.n_rows = 0

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
            self.lib.lib.morl_eupg_destroy(self.h)
            self.h = None

    def set_episode(self, obs, acc_rewards, actions, rewards, truncate=True):
        """``obs`` as ``train()`` hands them to the buffer; ``truncate``: the buffer's int32 cast, on the host."""
        obs = np.asarray(obs, dtype=np.float32).reshape(-1, self.D)
        n = obs.shape[0]
        if truncate:
            obs = eo.truncate_obs(obs)
        self.ep = [self.T(obs, (n, self.D)), self.T(acc_rewards, (n, self.R)), self.T(actions, (n,), np.int32), self.T(rewards, (n, self.R))]
        self.lib.check(self.lib.lib.morl_eupg_set_episode(self.h, *[t.data_ptr() for t in self.ep], n, self.lib.stream_of(self.params)))
        self.n_rows = n

    def returns(self, gamma):
        out = self.out(self.n_rows, self.R)
        self.lib.check(self.lib.lib.morl_eupg_returns(self.h, float(gamma), out.data_ptr(), self.lib.stream_of(out)))
        return self.take(out, self.n_rows)

    def update(self, u, lr):
        """One step on the scalarised values ``u`` [T]; returns the loss (numpy float32)."""
        u_d = self.T(u, (self.n_rows,))
        loss = self.out(1)
        self.lib.check(self.lib.lib.morl_eupg_update(self.h, self.params.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), u_d.data_ptr(),
                                                     float(lr), self.steps_done, loss.data_ptr(), self.lib.stream_of(loss)))
        self.steps_done += 1
        return self.take(loss, 1)[0]

    def step_probs(self):
        out = self.out(self.n_rows, self.A)
        self.lib.check(self.lib.lib.morl_eupg_step_probs(self.h, out.data_ptr(), self.lib.stream_of(out)))
        return self.take(out, self.n_rows)

    def forward(self, obs, acc_reward):
        o = self.T(obs, (-1, self.D))
        rows = o.shape[0]
        a = self.T(acc_reward, (rows, self.R))
        out = self.out(rows, self.A)
        self.lib.check(self.lib.lib.morl_eupg_forward(self.h, self.params.data_ptr(), o.data_ptr(), a.data_ptr(), rows, out.data_ptr(),
                                                      self.lib.stream_of(out)))
        return self.take(out, rows)

    def state(self, loss, probs):
        return dict(loss=loss, probs=probs, p1=self.params.cpu().numpy(), m1=self.m.cpu().numpy(), v1=self.v.cpu().numpy())
