"""Shared by the LCN tests: fixtures, the backend selector, a thin driver of ``morl_lcn_select`` and the exact comparison."""
from __future__ import annotations

import os

import numpy as np
import torch as th

from pcn_common import BACKENDS, GOLDEN_DIR, backend  # noqa: F401

MAX_N = 2048          # MORL_LCN_MAX_N of include/morl_hip.h


def load(name):
    return np.load(os.path.join(GOLDEN_DIR, f"lcn_{name}.npz"))


def select_rc(lib, dev, returns, mode, lcn_lambda=0.0, crowded=None):
    """One ``morl_lcn_select`` call: (status, l2 [N] float32 | None, mask [N] uint8)."""
    returns = np.ascontiguousarray(returns, dtype=np.float32)
    N, R = returns.shape
    ret = th.tensor(returns).to(dev) if returns.size else th.zeros(1, device=dev)
    nd = th.zeros(max(N, 1), dtype=th.uint8, device=dev)
    sma = l2 = None
    if crowded is not None:
        sma = th.tensor(np.ascontiguousarray(crowded, dtype=np.uint8)).to(dev)
        l2 = th.zeros(max(N, 1), dtype=th.float32, device=dev)
    rc = lib.lib.morl_lcn_select(ret.data_ptr(), N, R, mode, float(lcn_lambda), None if sma is None else sma.data_ptr(),
                                 None if l2 is None else l2.data_ptr(), nd.data_ptr(), lib.stream_of(nd))
    return rc, (None if l2 is None else l2.cpu().numpy()), nd.cpu().numpy()


def select(lib, dev, returns, mode, lcn_lambda=0.0, crowded=None):
    rc, l2, nd = select_rc(lib, dev, returns, mode, lcn_lambda, crowded)
    lib.check(rc)
    return l2, nd


def assert_same_bits(name, got, want):
    """Exact equality of two float32 arrays, bit patterns included (-0.0 is not 0.0); a mismatch names the first index."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape, (name, got.dtype, want.dtype, got.shape, want.shape)
    gb, wb = got.view(np.uint32), want.view(np.uint32)
    if not np.array_equal(gb, wb):
        k = int(np.argmax(gb != wb))
        raise AssertionError(f"{name}: {int((gb != wb).sum())} of {gb.size} differ, first at index {k}: got {got[k]!r} "
                             f"(0x{int(gb[k]):08x}), want {want[k]!r} (0x{int(wb[k]):08x})")


def assert_same_mask(name, got, want):
    got, want = np.asarray(got).astype(bool), np.asarray(want).astype(bool)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    if not np.array_equal(got, want):
        k = int(np.argmax(got != want))
        raise AssertionError(f"{name}: {int((got != want).sum())} of {got.size} flags differ, first at index {k}: got {got[k]}, "
                             f"want {want[k]}")
