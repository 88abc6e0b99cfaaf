"""TEST INFRASTRUCTURE shared by tests/test_ens_sweep.py: shapes, numpy-drawn inputs, the float64 oracle of a case
(``oracle/ens_oracle.py`` on float64 copies of the float32 inputs, computed once per case and shared by both backends) and
one step through ``ProbabilisticEnsemble`` with everything -- weights, non-zero biases, bounds, input statistics, Adam
moments -- loaded through its own ``state_dict`` / buffers.

Gradients are recovered without an ABI change: with zero moments at step 1 the engine leaves
``exp_avg = float32(0.1) * (g + wd_l * p)``, so ``g = exp_avg / float32(0.1) - wd_l * p`` per layer and
``g = bounds_m / float32(0.1)`` for the two bound vectors (no decay)."""
import functools
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import pytest
import torch as th

import ens_oracle as eo

from morl_baselines_amd.dynamics import DECAYS, ProbabilisticEnsemble

BACKENDS = ["sim", pytest.param("hip", marks=pytest.mark.gpu)]

LR = 1e-3
LOSS_RTOL = 1e-5              # the north star of every parity file
GRAD_TOL_FRAC = 2e-6          # of the tensor's largest float64 entry: grad_tol_frac of tests/test_ac_kernels_parity.py
ONE_MINUS_B1 = float(np.float32(0.1))

WORST = {}                    # backend name -> (fraction, tag): the worst gradient fraction seen so far


def backend(name):
    if name == "sim":
        import simlib
        return simlib.load_sim(), th.device("cpu")
    from morl_baselines_amd.native import load_library
    return load_library(), th.device("cuda:0")


def backend_name(be):
    return "sim" if be[1].type == "cpu" else "hip"


@dataclass(frozen=True)
class Case:
    E: int
    I: int
    O: int
    arch: Tuple[int, ...]
    rows: int
    seeded: bool = False

    @property
    def name(self):
        return f"E{self.E}_in{self.I}_out{self.O}_{'x'.join(map(str, self.arch))}_r{self.rows}"

    @property
    def dims(self):
        return [self.I] + list(self.arch) + [2 * self.O]

    @property
    def NL(self):
        return len(self.arch) + 1


ANCHOR = Case(3, 7, 6, (16, 16), 16)
WIDE_OUT = Case(7, 5, 64, (20, 12, 36, 8), 37, seeded=True)
CASES = [
    ANCHOR,                                       # the fixture's shape
    Case(1, 1, 1, (4,), 1),                       # every dimension at its minimum
    Case(3, 3, 5, (17, 5), 9),                    # widths / inputs no multiple of 4 (ld padding, the zeroed tail of dhead),
    Case(2, 33, 2, (1, 7, 3), 5),                 # rows not divisible by 4
    WIDE_OUT,                                     # output_dim at ENS_MAX_OUT, five layers (all decay slots), 65 partial blocks
    Case(5, 13, 11, (64,), 263),                  # 329 partial blocks: past the 256-thread stride of the loss sum
    Case(2, 9, 3, (200, 200), 150, seeded=True),  # the reference's default width
]
FWD = Case(3, 6, 4, (20, 12), 70)                 # forward / holdout / state tests; rows varies below max_rows = 70
FWD_ROWS = (1, 3, 4, 5, 63, 64, 65, 70)

EDGES = ("clamped", "mixed", "softplus_max", "softplus_min")


def _seed(c: Case, norm: bool, edge: Optional[str]) -> int:
    s = 1000003 * c.E + 10007 * c.I + 101 * c.O + 13 * c.rows + sum((i + 2) * h for i, h in enumerate(c.arch))
    return 4 * s + 2 * int(norm) + (0 if edge is None else 97 * (1 + EDGES.index(edge)))


def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def inputs(c: Case, norm: bool, edge: Optional[str] = None):
    """float32 inputs of one case, numpy only: W[l] (E, in, out), b[l] (E, 1, out), bounds (1, O), x, y, mu, sigma."""
    rng = np.random.default_rng(_seed(c, norm, edge))
    f = np.float32
    d = c.dims
    W = [(rng.standard_normal((c.E, d[l], d[l + 1])) * np.sqrt(2.0 / d[l])).astype(f) for l in range(c.NL)]
    b = [(0.1 * rng.standard_normal((c.E, 1, d[l + 1]))).astype(f) for l in range(c.NL)]
    max_lv, min_lv = np.full((1, c.O), 0.5, dtype=f), np.full((1, c.O), -10.0, dtype=f)
    if edge == "clamped":                         # every variance about 3e-7: below gaussian_nll_loss's eps
        max_lv[:], min_lv[:] = -15.0, -20.0
    elif edge == "mixed":                         # alternate outputs: both branches meet inside one wave
        max_lv[:, 0::2], min_lv[:, 0::2] = -15.0, -20.0
    elif edge == "softplus_max":                  # max - raw > 20: the first softplus passes its argument through
        b[-1][:, :, c.O:] -= 25.0
    elif edge == "softplus_min":                  # lv1 - min > 20: the second one does
        min_lv[:] = -25.0
        b[-1][:, :, c.O:] += 15.0
    if edge in ("softplus_max", "softplus_min"):  # a quarter of the log-variance head's spread: every entry takes the branch
        W[-1][:, :, c.O:] *= f(0.25)
    x = rng.standard_normal((c.E, c.rows, c.I)).astype(f)
    y = rng.standard_normal((c.E, c.rows, c.O)).astype(f)
    mu = (0.3 * rng.standard_normal((1, c.I))).astype(f) if norm else None
    sigma = rng.uniform(0.5, 1.5, (1, c.I)).astype(f) if norm else None
    inp = dict(W=W, b=b, max_lv=max_lv, min_lv=min_lv, x=x, y=y, mu=mu, sigma=sigma)
    _ro(*W, *b, max_lv, min_lv, x, y, *([mu, sigma] if norm else []))
    return inp


def t64(a):
    return None if a is None else th.tensor(np.asarray(a, dtype=np.float64))


def raw_head(inp):
    """float64 head output (mean | raw log-variance) before the bounds: what the edge tests look at to name their branch."""
    h = t64(inp["x"])
    if inp["mu"] is not None:
        h = (h - t64(inp["mu"])) / t64(inp["sigma"])
    for l in range(len(inp["W"]) - 1):
        h = th.relu(h @ t64(inp["W"][l]) + t64(inp["b"][l]))
    return h @ t64(inp["W"][-1]) + t64(inp["b"][-1])


@functools.lru_cache(maxsize=None)
def oracle_step1(c: Case, norm: bool, edge: Optional[str] = None):
    """float64 loss and gradients (W0, b0, W1, b1, ..., max_lv, min_lv) of the case."""
    inp = inputs(c, norm, edge)
    W = [t64(w).requires_grad_(True) for w in inp["W"]]
    b = [t64(v).requires_grad_(True) for v in inp["b"]]
    mx, mn = t64(inp["max_lv"]).requires_grad_(True), t64(inp["min_lv"]).requires_grad_(True)
    loss = eo.loss_fn(W, b, mx, mn, t64(inp["x"]), t64(inp["y"]), t64(inp["mu"]), t64(inp["sigma"]))
    params = [p for pair in zip(W, b) for p in pair] + [mx, mn]
    grads = [g.numpy() for g in th.autograd.grad(loss, params)]
    _ro(*grads)
    return float(loss.detach()), grads


@functools.lru_cache(maxsize=None)
def moments(c: Case, norm: bool, k: int):
    """float32 Adam moments to pre-seed step k with, in the optimiser's order (W0, b0, ..., max_lv, min_lv)."""
    rng = np.random.default_rng(_seed(c, norm, None) + 7919 * k)
    d = c.dims
    shapes = [s for l in range(c.NL) for s in ((c.E, d[l], d[l + 1]), (c.E, 1, d[l + 1]))] + [(1, c.O), (1, c.O)]
    m = [(1e-3 * rng.standard_normal(s)).astype(np.float32) for s in shapes]
    v = [(1e-6 * rng.uniform(0.25, 4.0, s)).astype(np.float32) for s in shapes]
    _ro(*m, *v)
    return m, v


@functools.lru_cache(maxsize=None)
def oracle_seeded(c: Case, norm: bool, k: int):
    """float64 ``ens_oracle.train_step`` as step k from the pre-seeded moments: (loss, params, exp_avg, exp_avg_sq), each in
    the optimiser's order."""
    inp = inputs(c, norm)
    m, v = moments(c, norm, k)
    st = dict(W=[t64(w) for w in inp["W"]], b=[t64(x) for x in inp["b"]], max_lv=t64(inp["max_lv"]), min_lv=t64(inp["min_lv"]),
              m=[t64(a) for a in m], v=[t64(a) for a in v])
    if norm:
        st["mu"], st["sigma"] = t64(inp["mu"]), t64(inp["sigma"])
    loss = eo.train_step(st, t64(inp["x"]), t64(inp["y"]), k, LR)
    p = [a.numpy() for pair in zip(st["W"], st["b"]) for a in pair] + [st["max_lv"].numpy(), st["min_lv"].numpy()]
    m1, v1 = [a.numpy() for a in st["m"]], [a.numpy() for a in st["v"]]
    _ro(*p, *m1, *v1)
    return float(loss), p, m1, v1


# -- the engine ------------------------------------------------------------------------------------------------------------
def make_model(be, c: Case, norm: bool, inp=None, max_rows: Optional[int] = None, decays=DECAYS):
    lib, dev = be
    model = ProbabilisticEnsemble(c.I, c.O, ensemble_size=c.E, arch=list(c.arch), normalize_inputs=norm, device=dev, lib=lib,
                                  learning_rate=LR, max_rows=max_rows or c.rows)
    model.decays = list(decays)                   # as fit() does
    if inp is not None:
        load_inputs(model, inp)
    return model


def load_inputs(model, inp):
    sd = model.state_dict()
    for l in range(len(inp["W"])):
        sd[f"layers.{l}.W"], sd[f"layers.{l}.b"] = th.tensor(inp["W"][l]), th.tensor(inp["b"][l])
    sd["max_logvar"], sd["min_logvar"] = th.tensor(inp["max_lv"]), th.tensor(inp["min_lv"])
    if inp["mu"] is not None:
        sd["inputs_mu"], sd["inputs_sigma"] = th.tensor(inp["mu"]), th.tensor(inp["sigma"])
    model.load_state_dict(sd)


def unpack(model, buf, bounds_buf):
    """A flat (E, Pm) engine buffer and its (2 * O) bounds companion in the optimiser's order and the reference's layouts."""
    out = []
    for w, b in model._layer_views(buf):
        out += [w.transpose(1, 2).cpu().numpy().copy(), b.unsqueeze(1).cpu().numpy().copy()]
    O = model._O
    return out + [bounds_buf[:O].view(1, -1).cpu().numpy().copy(), bounds_buf[O:].view(1, -1).cpu().numpy().copy()]


def pack(model, buf, bounds_buf, tensors):
    """The inverse of ``unpack``: write reference-layout arrays into the engine's buffers."""
    with th.no_grad():
        for l, (w, b) in enumerate(model._layer_views(buf)):
            w.copy_(th.tensor(tensors[2 * l]).to(buf.device).transpose(1, 2))
            b.copy_(th.tensor(tensors[2 * l + 1]).to(buf.device).squeeze(1))
        bounds_buf.copy_(th.cat([th.tensor(tensors[-2]).reshape(-1), th.tensor(tensors[-1]).reshape(-1)]).to(buf.device))


def step(model, inp, x=None, y=None):
    dev = model.device
    x = th.tensor(inp["x"] if x is None else x).to(dev)
    y = th.tensor(inp["y"] if y is None else y).to(dev)
    return float(model.train_step(x, y, want_loss=True).cpu())


def state_of(model):
    """Everything a step reads or writes, as host copies (for bit-for-bit comparisons)."""
    return dict(flat=model.flat.cpu().clone(), exp_avg=model.exp_avg.cpu().clone(), exp_avg_sq=model.exp_avg_sq.cpu().clone(),
                bounds=model.bounds.cpu().clone(), bounds_m=model.bounds_m.cpu().clone(), bounds_v=model.bounds_v.cpu().clone(),
                adam_step=model._adam_step)


def set_state(model, st):
    with th.no_grad():
        for k in ("flat", "exp_avg", "exp_avg_sq", "bounds", "bounds_m", "bounds_v"):
            getattr(model, k).copy_(st[k].to(model.device))
    model._adam_step = st["adam_step"]


def same_state(a, b):
    return all(th.equal(a[k], b[k]) for k in ("flat", "exp_avg", "exp_avg_sq", "bounds", "bounds_m", "bounds_v"))


def recovered_grads(model, inp, decays=DECAYS):
    """float64 gradients the engine used in a first step from zero moments, in the optimiser's order."""
    m = unpack(model, model.exp_avg, model.bounds_m)
    p0 = [a for pair in zip(inp["W"], inp["b"]) for a in pair]
    out = []
    for i, mi in enumerate(m[:-2]):
        wd = float(np.float32(decays[i // 2]))            # the engine's coefficient is a float
        out.append(mi.astype(np.float64) / ONE_MINUS_B1 - wd * p0[i].astype(np.float64))
    return out + [mi.astype(np.float64) / ONE_MINUS_B1 for mi in m[-2:]]


def names(c: Case):
    return [f"{k}{l}" for l in range(c.NL) for k in ("W", "b")] + ["max_logvar", "min_logvar"]


def check_step1(be, tag, c: Case, got_loss, got_grads, want_loss, want_grads):
    """Loss at 1e-5 relative, every gradient tensor within 2e-6 of its largest float64 entry; records the worst fraction."""
    name = backend_name(be)
    worst, where = 0.0, ""
    fails = []
    for n, g, w in zip(names(c), got_grads, want_grads):
        assert g.shape == w.shape, (tag, n, g.shape, w.shape)
        err, scale = float(np.abs(g - w).max()), float(np.abs(w).max())
        frac = err / scale if scale > 0 else (0.0 if err == 0 else float("inf"))
        if frac > worst:
            worst, where = frac, n
        if not frac <= GRAD_TOL_FRAC:
            fails.append(f"{n}: |diff| {err:.3e} = {frac:.3e} of the largest entry {scale:.3e}")
    rel = abs(got_loss - want_loss) / abs(want_loss)
    print(f"[{name}] {tag}: loss rel {rel:.2e}; worst gradient fraction {worst:.2e} ({where})")
    if worst > WORST.get(name, (0.0, ""))[0] and np.isfinite(worst):
        WORST[name] = (worst, f"{tag} {where}")
    assert rel <= LOSS_RTOL, f"{tag}: loss {got_loss!r} vs {want_loss!r} (rel {rel:.3e})"
    assert not fails, f"{tag}: " + "; ".join(fails)


def close_rel(name, got, want, rtol, atol=0.0):
    """The contract of tests/test_pcn_kernels_parity.py: |got - want| <= atol + rtol * |want|, entry by entry."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    err = np.abs(got - want)
    tol = atol + rtol * np.abs(want)
    worst = int(np.argmax(err - tol))
    assert (err <= tol).all(), f"{name}: |diff| {err.reshape(-1)[worst]:.3e} > {tol.reshape(-1)[worst]:.3e}"
