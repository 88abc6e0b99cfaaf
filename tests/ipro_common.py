"""Shared by the IPRO tests: fixtures, the backend selector, a thin driver of ``morl_ipro_hvis`` and an ``IPRO`` whose learner is the
scripted Pareto oracle of tests/golden/ipro_cases.py."""
from __future__ import annotations

import os
import types

import numpy as np
import torch as th

from pcn_common import BACKENDS, GOLDEN_DIR, backend, close_rel  # noqa: F401

MAX_POINTS, MAX_K = 512, 1024          # MORL_IPRO_MAX_POINTS, MORL_IPRO_MAX_K of include/morl_hip.h


def load(name):
    return np.load(os.path.join(GOLDEN_DIR, f"ipro_{name}.npz"))


def hvis_rc(lib, dev, base, cand, ref):
    """One ``morl_ipro_hvis`` call on host arrays: (status, out [K + 1] float64)."""
    ref = np.ascontiguousarray(ref, dtype=np.float64)
    R = ref.shape[0]
    base = np.ascontiguousarray(base, dtype=np.float64).reshape(-1, R)
    cand = np.ascontiguousarray(cand, dtype=np.float64).reshape(-1, R)
    n, K = len(base), len(cand)
    T = lambda a: th.tensor(a).to(dev) if a.size else th.zeros(1, dtype=th.float64, device=dev)  # noqa: E731
    b, c, r = T(base), T(cand), T(ref)
    words = int(lib.lib.morl_ipro_hvis_workspace_doubles(n, K, R))
    ws = th.zeros(max(words, 1), dtype=th.float64, device=dev)
    out = th.full((K + 1,), -1.0, dtype=th.float64, device=dev)
    rc = lib.lib.morl_ipro_hvis(b.data_ptr() if n else None, n, c.data_ptr() if K else None, K, R, r.data_ptr(), ws.data_ptr(),
                                out.data_ptr(), lib.stream_of(out))
    return rc, out.cpu().numpy()


def hvis(lib, dev, base, cand, ref):
    rc, out = hvis_rc(lib, dev, base, cand, ref)
    lib.check(rc)
    return out


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


class SpacesEnv:
    """Spaces only.  ``MOAgent`` reads ``action_space`` and ``unwrapped.reward_space``; the outer loop reads ``reward_space``: the
    two are different objects here, and only the second has the run's objective count."""

    def __init__(self, R, env_id="ipro-scripted-v0"):
        self.observation_space = types.SimpleNamespace(shape=(4,))
        self.action_space = types.SimpleNamespace(n=3, shape=())
        self.reward_space = types.SimpleNamespace(shape=(R,))
        self.unwrapped = types.SimpleNamespace(reward_space=types.SimpleNamespace(shape=(R + 1,)))
        self.spec = types.SimpleNamespace(id=env_id)


def scripted_agent(be, script, R, **kw):
    """``IPRO`` with the learner replaced by ``script`` (an ``ipro_cases.Scripted``): the outer loop and its kernels are under test."""
    from morl_baselines_amd.ipro import IPRO
    lib, dev = be

    class ScriptedIPRO(IPRO):
        def _make_learner(self, env, seed, **kwargs):
            self.learner_kwargs = kwargs
            return types.SimpleNamespace(agent=None)

        def linear_train(self, weight_vec, deterministic, eval_env):
            return script.linear(weight_vec), None

        def oracle_train(self, referent, deterministic, eval_env):
            return script.oracle(referent, self.nadir, self.ideal, self.sign), None

    return ScriptedIPRO(SpacesEnv(R), device=dev, lib=lib, **kw)
