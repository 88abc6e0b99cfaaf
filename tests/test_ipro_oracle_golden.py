"""tests/ipro_oracle.py -- the numpy restatement of IPRO's outer loop the other IPRO tests lean on -- against what
tests/golden/make_golden_ipro.py recorded from the unmodified reference: the point-set updates and the whole scripted runs exactly,
the volumes to 1e-12, the utilities to float32 rounding.  CPU only, no library."""
import numpy as np
import pytest

import ipro_cases as ic
import ipro_common as icm
import ipro_oracle as io_


@pytest.mark.parametrize("name", ic.POINT_CASES)
def test_point_set_updates(name):
    g = icm.load(f"points_{name}")
    which, pts, vec, nadir, ideal = ic.points_inputs(name)
    assert np.array_equal(pts, g["before"]) and np.array_equal(vec, g["vec"]) and bool(g["lower"].item()) == (which == "lower")
    lo = io_.Loop(len(vec), None, None)
    lo.nadir, lo.ideal = nadir, ideal
    if which == "lower":
        lo.lower_points = pts.copy()
        lo.update_lower_points(vec)
        got = lo.lower_points
    else:
        lo.upper_points = pts.copy()
        lo.update_upper_points(vec)
        got = lo.upper_points
    assert np.array_equal(np.asarray(got).reshape(-1, len(vec)), g["after"])


def rows(g, key, it):
    n = g[f"{key}_rows"]
    start = int(n[:it].sum())
    return g[key][start:start + int(n[it])]


def compare_trace(g, log, pareto_set, rtol=1e-12):
    assert len(log) == int(g["iterations"].item()) + 1
    for it, rec in enumerate(log):
        for k in io_.STATE:
            assert np.array_equal(rec[k], rows(g, k, it)), (k, it)
        for k in ("hv", "dominated_hv", "discarded_hv", "coverage", "error"):
            assert abs(rec[k] - g[k][it]) <= rtol * abs(g[k][it]), (k, it, rec[k], g[k][it])
        assert rec["replay_triggered"] == g["replay_triggered"][it]
        if it < int(g["iterations"].item()):
            assert np.array_equal(rec["referent"], g["referents"][it]) and np.array_equal(rec["vec"], g["vecs"][it]), it
    assert np.array_equal(np.asarray(pareto_set).reshape(-1, g["pareto_set"].shape[1]), g["pareto_set"])


@pytest.mark.parametrize("name", list(ic.TRACES))
def test_scripted_runs(name):
    T, g = ic.TRACES[name], icm.load(f"trace_{name}")
    script = ic.Scripted(ic.trace_table(T), T["weak_every"])
    lo = io_.Loop(T["R"], script.linear, script.oracle, direction=T["direction"], max_iterations=T["iterations"], seed=int(g["seed"].item()))
    pareto_set = lo.train(None)          # ref_point=None: a copy of the nadir
    compare_trace(g, lo.log, pareto_set)
    assert g["replay_triggered"][-1] >= 1, "the trace goes through replay"
    if name == "r4":
        assert g["lower_points_rows"].max() > 50, "the num=50 sub-sampling is exercised"


def test_utilities():
    g = icm.load("utility")
    batch, referent, nadir, ideal, weights = ic.utility_inputs()
    assert np.array_equal(batch, g["batch"]) and np.array_equal(weights, g["weights"])
    for sign in (1, -1):
        for aug in (0.0, 0.1):
            got = io_.aasf(batch, sign * referent, sign * nadir, sign * ideal, aug=np.float32(aug), scale=np.float32(100))
            assert got.dtype == np.float32
            np.testing.assert_allclose(got, g[f"aasf_sign{sign}_aug{aug}"], rtol=2e-6, atol=2e-5)
    np.testing.assert_allclose((batch * weights).sum(-1), g["linear"], rtol=2e-6, atol=2e-6)
