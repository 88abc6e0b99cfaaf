"""The EUPG restatement (``tests/eupg_oracle.py``) against the fixtures recorded from the unmodified reference.

The generator asserts that the restatement with the reference's own operations equals the reference bit for bit.  Here the form the
kernels compute -- every row normalised by its OWN sum, not by the batch's -- is held to the single-step contract in float64, which
is what entitles the shape sweep to use it as its reference.  No GPU."""
import numpy as np
import pytest
import torch as th

import eupg_cases as ec
import eupg_common as em
import eupg_oracle as eo


def oracle_step(c, g, obs):
    m0, v0 = ec.synthetic_moments(c.seed, len(g["p0"]))
    return eo.step_f64(g["p0"], m0, v0, c.step, c.lr, (c.D, c.A, c.R, c.hidden), obs, g["acc_rewards"], g["actions"], g["rewards"],
                       c.gamma, ec.utility)


@pytest.mark.parametrize("c", ec.STEP_CASES, ids=lambda c: c.name)
def test_row_local_normalisation_stays_inside_the_contract(c):
    g = em.load(c.name)
    with em.one_thread():
        o = oracle_step(c, g, eo.truncate_obs(g["obs"]))
    # two roundings of 2^-24 relative per step, each carried on with weight gamma^k: at most 2 * 2^-24 / (1 - gamma) of max |G|
    em.close_rel("returns", o["G"], g["returns"], 0.0, 2.0 ** -23 / (1.0 - c.gamma) * float(np.abs(g["returns"]).max()))
    em.close_rel("log-probs", o["logp"], g["logp"], 1e-5, em.ATOL)
    em.check_step(o, g, c.lr)


def test_the_int32_truncation_of_the_observations_is_part_of_the_fixture():
    """Fed the observations as acting saw them (floats), the same oracle must FAIL fixture a."""
    c, g = ec.BY_NAME["a"], em.load("a")
    assert (np.abs(g["obs"] - eo.truncate_obs(g["obs"])) > 0.1).mean() >= 0.5
    with em.one_thread():
        o = oracle_step(c, g, g["obs"])
    with pytest.raises(AssertionError):
        em.close_rel("probabilities", o["probs"], g["probs"], 1e-5, em.ATOL)
    with pytest.raises(AssertionError):
        em.close_rel("parameters", o["p1"], g["p1"], 2e-5, 0.02 * c.lr)


def test_truncation_is_numpys_assignment_cast():
    obs = np.array([[-1.9, -0.2, 0.7, 2.999, -3.0]], dtype=np.float32)
    assert eo.truncate_obs(obs).tolist() == [[-1, 0, 0, 2, -3]] and eo.truncate_obs(obs).dtype == np.int32


def test_the_scan_is_a_multiply_then_an_add_in_float32():
    g, c = em.load("c"), ec.BY_NAME["c"]
    G = eo.forward_cumulative_rewards(th.tensor(g["rewards"]), c.gamma).numpy()
    assert np.array_equal(G, g["returns"])
    gam, run = np.float32(c.gamma), np.zeros(c.R, dtype=np.float32)
    for t in reversed(range(c.T)):
        run = (gam * run).astype(np.float32) + g["rewards"][t]
        assert np.array_equal(run, g["returns"][t]), t
