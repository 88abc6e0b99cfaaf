"""Front metrics: the device hypervolume / expected utility against the oracle (closed forms, the 2-D sweep, a Monte-Carlo
estimate -- hypervolume parity with pymoo itself is UNPINNED, see oracle/metrics_oracle.py) and the numpy metrics against
golden values of the unmodified reference functions (tests/golden/metrics.npz)."""
import os
import sys

import numpy as np
import pytest
import torch as th

import metrics_oracle as mo
import momdp

import morl_baselines_amd.native as native
from morl_baselines_amd import performance_indicators as pi

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_golden_metrics as mg  # noqa: E402
import make_golden_hv as mh  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "metrics.npz")


@pytest.fixture(scope="module", params=["sim", pytest.param("hip", marks=pytest.mark.gpu)])
def be(request):
    if request.param == "sim":
        import simlib
        lib = simlib.load_sim()
        native.use_library(lib)
        yield lib, th.device("cpu")
        native.use_library(None)
        return
    yield native.load_library(), th.device("cuda:0")


def test_oracle_hypervolume_closed_forms_and_monte_carlo():
    assert mo.hypervolume(np.zeros(3), [np.array([1.0, 2.0, 3.0])]) == pytest.approx(6.0, rel=1e-15)
    # two overlapping boxes: |A| + |B| - |A n B|
    assert mo.hypervolume(np.zeros(2), [np.array([3.0, 1.0]), np.array([1.0, 2.0])]) == pytest.approx(3 + 2 - 1, rel=1e-15)
    # staircase in 3-D by inclusion-exclusion
    a, b = np.array([2.0, 1.0, 1.0]), np.array([1.0, 2.0, 2.0])
    assert mo.hypervolume(np.zeros(3), [a, b]) == pytest.approx(2 + 4 - 1, rel=1e-15)
    # a point that is not better than ref in one objective contributes nothing; dominated / duplicate points change nothing
    assert mo.hypervolume(np.zeros(2), [np.array([3.0, -1.0]), np.array([1.0, 1.0]), np.array([1.0, 1.0]), np.array([0.5, 0.5])]) == 1.0
    rng = np.random.default_rng(0)
    pts = rng.uniform(0.2, 1.0, (25, 4))
    x = rng.uniform(0.0, 1.0, (400000, 4))
    mc = (x[:, None, :] <= pts[None, :, :]).all(-1).any(-1).mean()
    assert mo.hypervolume(np.zeros(4), list(pts)) == pytest.approx(mc, rel=5e-3)
    for seed in range(5):
        p2 = np.random.default_rng(seed).uniform(-1, 2, (30, 2))
        assert mo.hypervolume(np.array([-0.5, 0.0]), list(p2)) == pytest.approx(momdp.hypervolume_2d(p2, [-0.5, 0.0]), rel=1e-13)


def test_numpy_metrics_match_reference_golden():
    g = np.load(GOLD)
    for k, case in enumerate(mg.CASES):
        front, weights, ref_set = mg.case_inputs(*case)
        for mod in (mo, pi):
            assert mod.sparsity(list(front)) == pytest.approx(float(g[f"sparsity_{k}"]), rel=1e-14, abs=0)
            assert mod.maximum_utility_loss(list(front), list(ref_set), weights) == pytest.approx(float(g[f"mul_{k}"]), rel=1e-14)
            assert mod.cardinality(list(front)) == float(g[f"card_{k}"])
        assert mo.expected_utility(list(front), list(weights)) == pytest.approx(float(g[f"eum_{k}"]), rel=1e-14)
    z, a = mg.case_inputs(3, 20, 5, 9)[0], mg.case_inputs(3, 20, 5, 10)[0]
    assert pi.igd(list(z), list(a)) == mo.igd(list(z), list(a)) > 0.0


@pytest.mark.parametrize("R,N", [(1, 9), (2, 1), (2, 64), (3, 100), (4, 60), (5, 18), (8, 6), (2, 512)])
def test_device_hypervolume_matches_oracle(be, R, N):
    lib, dev = be
    rng = np.random.default_rng(100 * R + N)
    pts = rng.uniform(-0.5, 2.0, (N, R))
    pts[N // 3] = pts[0]                                   # a duplicate
    if N > 4:
        pts[1, 0] = -2.0                                   # below the reference point in one objective
        pts[2] = pts[3] - 0.1                              # dominated
    ref = rng.uniform(-1.0, -0.2, R)
    want = mo.hypervolume(ref, list(pts))
    got = pi.hypervolume(ref, list(pts), lib=lib, device=dev)
    assert got == pytest.approx(want, rel=1e-12)
    # invariances: order of the points, dominated extras
    perm = rng.permutation(N)
    assert pi.hypervolume(ref, list(pts[perm]), lib=lib, device=dev) == pytest.approx(want, rel=1e-12)
    if N < 512:
        extra = np.vstack([pts, pts[:1] - 0.01])
        assert pi.hypervolume(ref, list(extra), lib=lib, device=dev) == pytest.approx(want, rel=1e-12)


# Deep Sea Treasure (Vamplew et al. 2011): the ten treasures and the steps needed to reach them.  The hypervolume of this Pareto
# front w.r.t. the reference point (0, -25) is the figure the MORL literature quotes for the environment -- 1155 (e.g. Van
# Moffaert & Nowe, JMLR 2014, Pareto Q-learning) -- an anchor that is independent of this repository and of pymoo.
DST_FRONT = [(1, -1), (2, -3), (3, -5), (5, -7), (8, -8), (16, -9), (24, -13), (50, -14), (74, -17), (124, -19)]


def test_hypervolume_of_the_deep_sea_treasure_front_is_the_published_1155(be):
    lib, dev = be
    pts = [np.array(p, dtype=np.float64) for p in DST_FRONT]
    ref = np.array([0.0, -25.0])
    assert mo.hypervolume(ref, pts) == 1155.0
    assert pi.hypervolume(ref, pts, lib=lib, device=dev) == 1155.0
    # dominated policies of a learning agent's archive do not change it
    assert pi.hypervolume(ref, pts + [np.array([7.0, -9.0]), np.array([1.0, -2.0])], lib=lib, device=dev) == 1155.0


@pytest.mark.skipif(not (os.path.exists(mh.OUT) or mh.pymoo_available()),
                    reason="needs pymoo, which is not installed, or tests/golden/hv.npz, which only a machine with pymoo can write: "
                           "hypervolume parity with pymoo stays UNPINNED (run tests/golden/make_golden_hv.py wherever pymoo exists)")
def test_hypervolume_pinned_to_pymoo(be):
    """The pin against the reference's own hypervolume (pymoo's HV through ``performance_indicators.hypervolume``): values
    committed by tests/golden/make_golden_hv.py wherever pymoo was importable, or computed live when it is importable here.
    Skips -- loudly, before any work -- while neither exists: the hypervolume then stays "unpinned against pymoo"."""
    lib, dev = be
    if os.path.exists(mh.OUT):
        want = {k: float(v) for k, v in np.load(mh.OUT).items()}
    else:
        want = {k: float(v) for k, v in mh.compute().items()}
    for k, (R, N, seed) in enumerate(mh.CASES):
        ref, pts = mh.case_inputs(R, N, seed)
        assert mo.hypervolume(ref, list(pts)) == pytest.approx(want[f"hv_{k}"], rel=1e-12)
        assert pi.hypervolume(ref, list(pts), lib=lib, device=dev) == pytest.approx(want[f"hv_{k}"], rel=1e-12)
    ref, pts = mh.dst_front()
    assert want["hv_dst"] == pytest.approx(1155.0, rel=1e-14)
    assert pi.hypervolume(ref, list(pts), lib=lib, device=dev) == pytest.approx(want["hv_dst"], rel=1e-12)


def test_hypervolume_of_a_large_archive(be):
    """More points than the LDS-staged kernel holds (the reference's pymoo HV takes any N): 1 500 points of which most are
    dominated -- pruned on the device first -- and a 700-point non-dominated 2-D front that stays above the staged size."""
    lib, dev = be
    rng = np.random.default_rng(7)
    pts = rng.uniform(0.0, 1.0, (1500, 3))
    ref = np.full(3, -0.1)
    want = mo.hypervolume(ref, list(pts[momdp.non_dominated(pts)])) if hasattr(momdp, "non_dominated") else mo.hypervolume(ref, list(pts))
    assert pi.hypervolume(ref, list(pts), lib=lib, device=dev) == pytest.approx(want, rel=1e-12)
    x = np.sort(rng.uniform(0.0, 1.0, 700))
    front = np.stack([x, 1.0 - x ** 2], axis=1)                      # strictly decreasing: all non-dominated
    want2 = momdp.hypervolume_2d(front, [-0.5, -0.5])
    assert pi.hypervolume(np.array([-0.5, -0.5]), list(front), lib=lib, device=dev) == pytest.approx(want2, rel=1e-12)


def test_device_hypervolume_edges(be):
    lib, dev = be
    assert pi.hypervolume(np.zeros(2), [np.array([-1.0, 5.0])], lib=lib, device=dev) == 0.0          # nothing above ref
    assert pi.hypervolume(np.zeros(3), [np.array([1.0, 2.0, 3.0])], lib=lib, device=dev) == 6.0
    assert float(pi.hypervolume_device(th.zeros(2, dtype=th.float64, device=dev), th.zeros((0, 2), dtype=th.float64, device=dev),
                                       lib).item()) == 0.0
    # 513 copies of one point: beyond the LDS-staged size, pruned to a single point on the device first
    assert pi.hypervolume(np.zeros(2), list(np.ones((513, 2))), lib=lib, device=dev) == 1.0
    with pytest.raises(Exception):                                                                    # 200^7 boxes: refused, loudly
        pi.hypervolume_device(th.zeros(8, dtype=th.float64, device=dev),
                              th.rand((200, 8), dtype=th.float64, device=dev) + 0.5, lib)


def test_device_expected_utility_matches_reference_golden(be):
    lib, dev = be
    g = np.load(GOLD)
    for k, case in enumerate(mg.CASES):
        front, weights, _ = mg.case_inputs(*case)
        got = pi.expected_utility(list(front), list(weights), lib=lib, device=dev)
        assert got == pytest.approx(float(g[f"eum_{k}"]), rel=1e-13)
    f32 = [p.astype(np.float32) for p in mg.case_inputs(3, 12, 9, 5)[0]]
    w = list(mg.case_inputs(3, 12, 9, 5)[1])
    assert pi.expected_utility(f32, w, lib=lib, device=dev) == pytest.approx(mo.expected_utility(f32, w), rel=1e-13)
    tch = lambda w_, p: -np.max(w_ * np.abs(p - 3.0))  # noqa: E731  (a non-linear utility takes the reference's host loop)
    assert pi.expected_utility(f32, w, utility=tch, lib=lib, device=dev) == mo.expected_utility(f32, w, utility=tch)


def test_multi_policy_metrics_dict(be):
    lib, dev = be
    from morl_baselines_amd import evaluation as ev
    from morl_baselines_amd.pareto import filter_pareto_dominated
    front, weights, ref_set = mg.case_inputs(3, 40, 50, 1)
    m = ev.multi_policy_metrics(list(front), np.full(3, -1.5), list(weights), ref_front=list(ref_set), lib=lib, device=dev)
    nd = list(filter_pareto_dominated(list(front), lib=lib, device=dev))
    assert m["eval/cardinality"] == len(nd) < 40
    assert m["eval/hypervolume"] == pytest.approx(mo.hypervolume(np.full(3, -1.5), list(front)), rel=1e-12)   # dominated points add nothing
    assert m["eval/eum"] == pytest.approx(mo.expected_utility(nd, list(weights)), rel=1e-13)
    assert m["eval/igd"] == mo.igd(list(ref_set), nd) and m["eval/mul"] == pytest.approx(mo.maximum_utility_loss(nd, list(ref_set), weights))
