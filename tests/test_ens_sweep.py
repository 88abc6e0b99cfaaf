"""Shape and edge sweep of the probabilistic dynamics ensemble (``csrc/ens_kernels.h``, the ``morl_ens_*`` entries,
``dynamics.py``) against ``oracle/ens_oracle.py`` in float64 on the same float32 inputs.  ``sim`` = wave emulator, ``hip`` =
gfx950 (-m gpu).  tests/test_ens_parity.py pins the oracle to the unmodified reference at one shape; this file leaves that
shape: minimum dimensions, widths / inputs / rows that are no multiple of 4, ``output_dim`` at ENS_MAX_OUT with five layers,
65 and 329 partial blocks of ``ens_nll_kernel`` (past a wave and past the 256-thread stride of ``ens_bounds_step_kernel``),
the reference's 200-wide layers; clamped and mixed variances (``F.gaussian_nll_loss`` clamps the variance under no_grad, so
the log-variance gradient passes straight through the clamp), both softplus pass-through branches; the shared-input and
per-member forward, the holdout MSE, stale workspace rows, run-to-run determinism, both GEMM engines, refused arguments.

A first step from zero moments leaves ``exp_avg = float32(0.1) * (g + wd * p)``, which gives the gradients back
(tests/ens_common.py); the "seeded" cases add a step k in {2, 5} from pre-seeded moments, checked with the contract of
tests/test_pcn_kernels_parity.py.

Tolerances: loss 1e-5 relative; every gradient tensor within 2e-6 of its largest float64 entry (``grad_tol_frac`` of
tests/test_ac_kernels_parity.py, same MFMA engines).  Gradient fraction observed over this file, per case:
  emulator  2.3e-7 to 1.55e-6     MI355X  2.2e-7 to 1.55e-6     (loss: at most 6.0e-7 relative on both)
the worst being ``max_logvar`` of (2, 33, 2, [1, 7, 3], 5), a sum of ten terms.  The last test prints the figure of the backend
it ran on.

What is left is float32 itself: ``min + softplus(lv1 - min)`` rounds at the magnitude of ``min`` (about 1e-6 absolute on the
log-variance with min = -10, so 1e-6 relative on the variance).  Inputs are He-scaled, so raw log-variances reach 12 below the
upper bound; there ``1 - sigmoid`` by subtraction -- what float32 autograd does, and what ``ens_nll_kernel`` did -- keeps two or
three digits.  With that subtraction (and the clamp already fixed) the bound gradients of these inputs were up to 1.4e-4 of
their largest entry off on the emulator, 19 of this file's cases failing, and the float32 torch oracle up to 3.7e-4 from the
float64 one; the kernel now takes the complement from the exponential (``ens_sigmoid_comp``), which is what the 2e-6 on the
two bound vectors holds it to."""
import ctypes as C

import numpy as np
import pytest
import torch as th

import ens_common as ec
import ens_oracle as eo

from morl_baselines_amd.native import EnsCfg, EnsDesc

MEAN_TOL_FRAC = 2e-6          # forward mean: of the largest entry
LOGVAR_ATOL = 1e-5            # forward log-variance: absolute
MSE_RTOL = 1e-5


@pytest.fixture(scope="module", params=ec.BACKENDS)
def be(request):
    return ec.backend(request.param)


def run_step1(be, c, norm, edge=None, decays=ec.DECAYS):
    inp = ec.inputs(c, norm, edge)
    model = ec.make_model(be, c, norm, inp, decays=decays)
    loss = ec.step(model, inp)
    return model, loss, ec.recovered_grads(model, inp, decays)


# -- shapes ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("norm", [True, False], ids=["norm", "raw"])
@pytest.mark.parametrize("c", ec.CASES, ids=lambda c: c.name)
def test_loss_and_gradients(be, c, norm):
    want_loss, want = ec.oracle_step1(c, norm)
    assert all(np.abs(w).max() > 0 for w in want), "a tensor without gradient checks nothing"
    _, loss, got = run_step1(be, c, norm)
    ec.check_step1(be, f"{c.name} norm={int(norm)}", c, loss, got, want_loss, want)


@pytest.mark.parametrize("k", [2, 5])
@pytest.mark.parametrize("norm", [True, False], ids=["norm", "raw"])
@pytest.mark.parametrize("c", [c for c in ec.CASES if c.seeded], ids=lambda c: c.name)
def test_step_from_seeded_moments(be, c, norm, k):
    """Step k from non-zero moments: parameters, both moments and both bounds against the float64 optimiser step.  The
    ``max`` of the moments' absolute term is taken over the weights and biases of all layers (one flat vector in the engine,
    as PCN's) and over the two bound vectors (the engine's other buffer)."""
    inp = ec.inputs(c, norm)
    m0, v0 = ec.moments(c, norm, k)
    want_loss, p1, m1, v1 = ec.oracle_seeded(c, norm, k)
    model = ec.make_model(be, c, norm, inp)
    ec.pack(model, model.exp_avg, model.bounds_m, m0)
    ec.pack(model, model.exp_avg_sq, model.bounds_v, v0)
    model._adam_step = k - 1
    loss = ec.step(model, inp)
    assert abs(loss - want_loss) <= ec.LOSS_RTOL * abs(want_loss), (loss, want_loss)
    got_p = ec.unpack(model, model.flat, model.bounds)
    got_m = ec.unpack(model, model.exp_avg, model.bounds_m)
    got_v = ec.unpack(model, model.exp_avg_sq, model.bounds_v)
    for part in (slice(0, -2), slice(-2, None)):
        m_scale = max(float(np.abs(a).max()) for a in m1[part])
        v_scale = max(float(np.abs(a).max()) for a in v1[part])
        for n, gp, gm, gv, wp, wm, wv in zip(ec.names(c)[part], got_p[part], got_m[part], got_v[part], p1[part], m1[part], v1[part]):
            ec.close_rel(f"{c.name} k={k} {n}", gp, wp, 2e-5, 0.02 * ec.LR)
            ec.close_rel(f"{c.name} k={k} exp_avg {n}", gm, wm, 1e-4, 2e-5 * m_scale)
            ec.close_rel(f"{c.name} k={k} exp_avg_sq {n}", gv, wv, 2e-4, 2e-5 * v_scale)


def test_each_layer_takes_its_own_decay(be):
    """The reference's third and fourth coefficients are equal; five distinct (and larger) ones tell every slot apart: a layer
    that took a neighbour's coefficient would be off by 0.01 * |p|."""
    c, norm = ec.WIDE_OUT, False
    decays = (0.01, 0.02, 0.03, 0.04, 0.05)
    want_loss, want = ec.oracle_step1(c, norm)
    _, loss, got = run_step1(be, c, norm, decays=decays)
    ec.check_step1(be, f"{c.name} distinct decays", c, loss, got, want_loss, want)


# -- variance clamp and softplus thresholds -------------------------------------------------------------------------------------
def oracle_branches(c, norm, edge):
    """(raw log-variance, lv1 after the upper bound, bounded log-variance, variance) of the float64 oracle."""
    inp = ec.inputs(c, norm, edge)
    raw = ec.raw_head(inp)[..., c.O:]
    mx, mn = ec.t64(inp["max_lv"]), ec.t64(inp["min_lv"])
    lv1 = mx - th.nn.functional.softplus(mx - raw)
    _, lv = eo.forward([ec.t64(w) for w in inp["W"]], [ec.t64(b) for b in inp["b"]], mx, mn, ec.t64(inp["x"]),
                       ec.t64(inp["mu"]), ec.t64(inp["sigma"]))
    return raw, lv1, lv, th.exp(lv)


@pytest.mark.parametrize("norm", [True, False], ids=["norm", "raw"])
@pytest.mark.parametrize("edge", ec.EDGES)
@pytest.mark.parametrize("c", [ec.ANCHOR, ec.WIDE_OUT], ids=lambda c: c.name)
def test_variance_and_softplus_edges(be, c, edge, norm):
    inp = ec.inputs(c, norm, edge)
    raw, lv1, lv, var = oracle_branches(c, norm, edge)
    want_loss, want = ec.oracle_step1(c, norm, edge)
    # the oracle alone: the branch this case is named after is the one taken
    if edge == "clamped":
        assert bool((var < 1e-6).all())
        for g, reg in ((want[-2], 0.01), (want[-1], -0.01)):      # a kernel that returns only the regulariser must fail
            assert float(np.abs(g - reg).max()) > 1e-3 * float(np.abs(g).max()) > 0
    elif edge == "mixed":
        clamped = float((var < 1e-6).double().mean())
        assert clamped >= 0.25 and 1.0 - clamped >= 0.25, clamped
    elif edge == "softplus_max":
        assert bool((ec.t64(inp["max_lv"]) - raw > 20).all())
    else:
        assert bool((lv1 - ec.t64(inp["min_lv"]) > 20).all())
    _, loss, got = run_step1(be, c, norm, edge)
    ec.check_step1(be, f"{c.name} {edge} norm={int(norm)}", c, loss, got, want_loss, want)


def test_bounds_that_clamp_everything_and_nothing():
    """(-15, -20) puts every variance below eps = 1e-6 (e^-15 = 3.1e-7); (-12, -20) none (e^-12 = 6.1e-6, and the raw
    log-variances of these inputs are far above -12, so the bounded ones sit just under the upper bound)."""
    c = ec.ANCHOR
    assert bool((oracle_branches(c, True, "clamped")[3] < 1e-6).all())
    inp = dict(ec.inputs(c, True, "clamped"))
    inp["max_lv"] = np.full((1, c.O), -12.0, dtype=np.float32)
    _, lv = eo.forward([ec.t64(w) for w in inp["W"]], [ec.t64(b) for b in inp["b"]], ec.t64(inp["max_lv"]), ec.t64(inp["min_lv"]),
                       ec.t64(inp["x"]), ec.t64(inp["mu"]), ec.t64(inp["sigma"]))
    assert bool((th.exp(lv) > 1e-6).all())


# -- forward and holdout -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[True, False], ids=["norm", "raw"])
def fwd(be, request):
    """One model of the forward shape, its inputs, and the full 70-row calls every row count is compared with."""
    c, norm = ec.FWD, request.param
    inp = ec.inputs(c, norm)
    model = ec.make_model(be, c, norm, inp)
    x_shared = th.tensor(inp["x"][0])                                  # (70, in)
    x_member = th.tensor(inp["x"])                                     # (E, 70, in)
    a = [ec.t64(w) for w in inp["W"]], [ec.t64(b) for b in inp["b"]], ec.t64(inp["max_lv"]), ec.t64(inp["min_lv"])
    stats = ec.t64(inp["mu"]), ec.t64(inp["sigma"])
    want_shared = eo.forward(*a, ec.t64(inp["x"][0]), *stats)
    want_member = eo.forward(*a, ec.t64(inp["x"]), *stats)
    full_shared = [t.cpu() for t in model.predict(x_shared)]
    full_member = [t.cpu() for t in model.predict(x_member, per_member=True)]
    return dict(c=c, inp=inp, model=model, x_shared=x_shared, x_member=x_member, oracle_args=(a, stats),
                want_shared=want_shared, want_member=want_member, full_shared=full_shared, full_member=full_member)


def check_forward(tag, got, want, rows):
    mean, logvar = (t.cpu().double() for t in got)
    w_mean, w_logvar = want[0][:, :rows], want[1][:, :rows]
    assert mean.shape == w_mean.shape and logvar.shape == w_logvar.shape, (tag, mean.shape, w_mean.shape)
    err = float((mean - w_mean).abs().max())
    assert err <= MEAN_TOL_FRAC * float(w_mean.abs().max()), (tag, err)
    assert float((logvar - w_logvar).abs().max()) <= LOGVAR_ATOL, tag


@pytest.mark.parametrize("rows", ec.FWD_ROWS)
def test_forward_shared_and_per_member(be, fwd, rows):
    model, E = fwd["model"], fwd["c"].E
    shared = model.predict(fwd["x_shared"][:rows])
    check_forward(f"shared rows={rows}", shared, fwd["want_shared"], rows)
    member = model.predict(fwd["x_member"][:, :rows].contiguous(), per_member=True)
    check_forward(f"per-member rows={rows}", member, fwd["want_member"], rows)
    # a prefix of rows is the prefix of the full call, bit for bit
    for got, full in ((shared, fwd["full_shared"]), (member, fwd["full_member"])):
        for g, f in zip(got, full):
            assert th.equal(g.cpu(), f[:, :rows]), f"rows={rows}: a prefix differs from the 70-row call"
    # the shared rows replicated per member: each member equals the shared call, bit for bit
    repl = model.predict(fwd["x_shared"][:rows].unsqueeze(0).repeat(E, 1, 1).contiguous(), per_member=True)
    for g, s in zip(repl, shared):
        assert th.equal(g, s), f"rows={rows}: per-member call on replicated rows differs from the shared call"


@pytest.mark.parametrize("rows", ec.FWD_ROWS)
def test_holdout_mse(be, fwd, rows):
    model, inp = fwd["model"], fwd["inp"]
    (a, stats) = fwd["oracle_args"]
    x, y = inp["x"][0][:rows], inp["y"][0][:rows]
    want = eo.mse_losses(*a, ec.t64(x), ec.t64(y), *stats).numpy()
    got = model.holdout_mse(th.tensor(x).to(model.device), th.tensor(y).to(model.device)).cpu().numpy().astype(np.float64)
    assert got.shape == want.shape
    assert (np.abs(got - want) <= MSE_RTOL * np.abs(want)).all(), (rows, got, want)


# -- state and determinism ------------------------------------------------------------------------------------------------------------
def test_small_step_after_a_big_one_sees_no_stale_rows(be):
    """70 rows, then 5 on the same context, against the 5-row step on a fresh context from the same state: stale tape rows or
    partial sums of the bigger step would show in the bits."""
    c, norm = ec.FWD, True
    inp = ec.inputs(c, norm)
    used = ec.make_model(be, c, norm, inp)
    ec.step(used, inp)
    mid = ec.state_of(used)
    x5, y5 = np.ascontiguousarray(inp["x"][:, 20:25]), np.ascontiguousarray(inp["y"][:, 20:25])
    loss_used = ec.step(used, inp, x5, y5)
    fresh = ec.make_model(be, c, norm, inp)
    ec.set_state(fresh, mid)
    loss_fresh = ec.step(fresh, inp, x5, y5)
    assert loss_used == loss_fresh
    assert ec.same_state(ec.state_of(used), ec.state_of(fresh))
    assert not ec.same_state(ec.state_of(used), mid), "the small step changed nothing"


def test_a_step_repeats_itself_bit_for_bit(be):
    c, norm = ec.CASES[5], True                     # 329 partial blocks: the longest reductions of the sweep
    inp = ec.inputs(c, norm)
    runs = []
    for _ in range(2):
        model = ec.make_model(be, c, norm, inp)
        runs.append((ec.step(model, inp), ec.state_of(model)))
    assert runs[0][0] == runs[1][0] and ec.same_state(runs[0][1], runs[1][1])


def test_both_gemm_engines_meet_the_oracle(be):
    """LDS tiles (mode 1) and wave tiles (mode 2): each within the oracle's tolerances and each reproducing itself."""
    lib, _ = be
    c, norm = ec.ANCHOR, True
    inp = ec.inputs(c, norm)
    want_loss, want = ec.oracle_step1(c, norm)
    try:
        for mode in (1, 2):
            lib.check(lib.lib.morl_ac_set_gemm_mode(mode))
            runs = []
            for _ in range(2):
                model, loss, got = run_step1(be, c, norm)
                ec.check_step1(be, f"{c.name} gemm mode {mode}", c, loss, got, want_loss, want)
                runs.append((loss, ec.state_of(model)))
            assert runs[0][0] == runs[1][0] and ec.same_state(runs[0][1], runs[1][1]), f"gemm mode {mode} run to run"
    finally:
        lib.lib.morl_ac_set_gemm_mode(0)


# -- refusals ------------------------------------------------------------------------------------------------------------------------
def desc(I=6, O=4, arch=(20, 12), E=3, max_rows=8, n_hidden=None):
    d = EnsDesc()
    d.input_dim, d.output_dim, d.ensemble_size, d.max_rows = I, O, E, max_rows
    d.n_hidden = len(arch) if n_hidden is None else n_hidden
    for i, h in enumerate(arch):
        d.hidden[i] = h
    return d


def test_bad_arguments_are_refused(be):
    lib, dev = be
    L, err = lib.lib, lib.lib.morl_last_error
    launches = None
    if dev.type == "cpu":
        launches = L.hipsim_launch_count
        launches.restype = C.c_longlong
    c, norm = ec.Case(3, 6, 4, (20, 12), 8), True
    model = ec.make_model(be, c, norm, ec.inputs(c, norm))          # (built before counting: nothing below may launch)
    E, I, O, cap = c.E, c.I, c.O, c.rows
    z = lambda *s: th.zeros(*s, dtype=th.float32, device=dev)  # noqa: E731
    x, y, out = z(E, cap + 1, I), z(E, cap + 1, O), z(E, cap + 1, O)
    mse, loss = z(E), z(1)
    before = ec.state_of(model)
    n0 = launches() if launches else 0

    bad = [(desc(O=0), b"out=0"), (desc(O=65), b"out=65"), (desc(E=0), b"ensemble_size 0"), (desc(E=65), b"ensemble_size 65"),
           (desc(arch=(), n_hidden=0), b"n_hidden 0"), (desc(arch=(20, 0)), b"hidden[1] = 0")]
    for d, text in bad:
        assert L.morl_ens_param_count(C.byref(d)) == -1 and text in err(), (text, err())
        h = C.c_void_p()
        assert L.morl_ens_create(C.byref(h), C.byref(d)) != 0 and text in err() and not h.value, (text, err())
    h = C.c_void_p()                               # the parameter count does not depend on max_rows: only create sees it
    assert L.morl_ens_create(C.byref(h), C.byref(desc(max_rows=0))) != 0 and b"max_rows 0" in err() and not h.value

    cfg = EnsCfg()
    cfg.lr, cfg.beta1, cfg.beta2, cfg.eps, cfg.adam_step = ec.LR, 0.9, 0.999, 1e-8, 1
    P = lambda t: t.data_ptr()  # noqa: E731
    mu, sg = P(model.inputs_mu), P(model.inputs_sigma)

    def forward(rows, mu, sg):
        return L.morl_ens_forward(model._h, P(model.flat), P(model.bounds), mu, sg, P(x), 1, rows, P(out), P(out), None)

    def train(rows, mu, sg):
        return L.morl_ens_train_step(model._h, P(model.flat), P(model.exp_avg), P(model.exp_avg_sq), P(model.bounds),
                                     P(model.bounds_m), P(model.bounds_v), mu, sg, P(x), P(y), rows, C.byref(cfg), P(loss), None)

    def holdout(rows, mu, sg):
        return L.morl_ens_mse(model._h, P(model.flat), P(model.bounds), mu, sg, P(x), P(y), rows, P(mse), None)

    for entry in (forward, train, holdout):
        for rows in (cap + 1, 0):
            assert entry(rows, mu, sg) != 0 and f"rows {rows} outside".encode() in err(), (entry.__name__, rows, err())
        for only in ((mu, None), (None, sg)):
            assert entry(cap, *only) != 0 and b"mu and sigma" in err(), (entry.__name__, err())
    # the wrapper turns the status into an exception
    with pytest.raises(RuntimeError, match="max_rows"):
        model.predict(x, per_member=True)
    with pytest.raises(RuntimeError, match="max_rows"):
        model.holdout_mse(x[0], y[0])
    if launches:
        assert launches() == n0, "a refused call launched a kernel"
    assert ec.same_state(ec.state_of(model), before)


def test_worst_gradient_fraction_report(be):
    """Prints the worst gradient fraction the tests above saw on this backend (the figure quoted in the module docstring)."""
    name = ec.backend_name(be)
    worst, where = ec.WORST.get(name, (0.0, "no gradient test ran"))
    print(f"[{name}] worst gradient fraction of the sweep: {worst:.2e} ({where}); bound {ec.GRAD_TOL_FRAC:.0e}")
    assert worst <= ec.GRAD_TOL_FRAC
