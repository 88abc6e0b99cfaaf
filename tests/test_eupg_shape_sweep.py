"""EUPG kernels over shapes and episode lengths, against the float64 restatement that ``test_eupg_oracle_golden.py`` pins to the
reference's fixtures.  Widths that are no multiple of anything (1, 31, 50), the limits (128 inputs, 128 units, 32 actions), episodes
of less than a tile, exactly one, one row more and several; the same single-step contract as the fixtures.

The utility here is positive (1 + |G|^2 / 4), so the loss is a sum of terms of one sign and its relative bound means what it says."""
import numpy as np
import pytest
import torch as th

import eupg_cases as ec
import eupg_common as em
import eupg_oracle as eo

LR, STEP, GAMMA = 1e-3, 57, 0.9
LENGTHS = (1, 15, 16, 17, 33)


def utility(r, w=None):
    return 1.0 + 0.25 * (r * r).sum(-1)


@pytest.fixture(scope="module", params=em.BACKENDS)
def be(request):
    return em.backend(request.param)


def random_params(rng, D, A, hidden):
    """Flat parameters in the order of PolicyNet.parameters(): weights N(0, 1 / fan_in), small biases."""
    out, w = [], D
    for h in tuple(hidden) + (A,):
        out += [rng.standard_normal((h, w)) / np.sqrt(w), 0.1 * rng.standard_normal(h)]
        w = h
    return np.concatenate([a.reshape(-1) for a in out]).astype(np.float32)


def episode(rng, T, obs_dim, R, A):
    obs = rng.integers(-2, 3, size=(T, obs_dim)).astype(np.float32)      # (as the buffer holds them)
    rewards = rng.standard_normal((T, R)).astype(np.float32)
    acc = np.concatenate([np.zeros((1, R), np.float32), np.cumsum(rewards, axis=0, dtype=np.float32)[:-1]])
    return obs, acc, rng.integers(0, A, size=T).astype(np.int32), rewards


def check(be, seed, T, obs_dim, R, A, hidden, p0, ep=None, max_workgroups=0):
    lib, dev = be
    rng = np.random.default_rng(seed)
    obs, acc, actions, rewards = ep or episode(rng, T, obs_dim, R, A)
    m0, v0 = ec.synthetic_moments(seed, len(p0))
    with em.one_thread():
        want = eo.step_f64(p0, m0, v0, STEP, LR, (obs_dim, A, R, hidden), obs, acc, actions, rewards, GAMMA, utility)
    ctx = em.Ctx(lib, dev, obs_dim, A, R, hidden, p0, m0, v0, steps_done=STEP, max_rows=T, max_workgroups=max_workgroups)
    try:
        ctx.set_episode(obs, acc, actions, rewards)
        G = ctx.returns(GAMMA)
        # two roundings of 2^-24 relative per step, each carried on with weight gamma^k: at most 2 * 2^-24 / (1 - gamma) of max |G|
        em.close_rel("returns", G, want["G"], 0.0, 2.0 ** -23 / (1.0 - GAMMA) * float(np.abs(want["G"]).max()))
        loss = ctx.update(utility(th.tensor(G)).numpy(), LR)
        em.check_step(ctx.state(loss, ctx.step_probs()), want, LR, f"T={T} ")
    finally:
        ctx.close()
    return want


@pytest.mark.parametrize("width", [1, 31, 50, 128])
@pytest.mark.parametrize("A", [2, 32])
@pytest.mark.parametrize("DR", [2, 128])
def test_one_hidden_layer(be, width, A, DR):
    R = 1 if DR == 2 else 8
    obs_dim = DR - R
    p0 = random_params(np.random.default_rng(width * 1000 + A * 10 + DR), DR, A, (width,))
    for T in LENGTHS:
        check(be, 100 * width + T, T, obs_dim, R, A, (width,), p0)


@pytest.mark.parametrize("hidden", [(31, 1), (1, 50), (128, 31), (50, 128)])
def test_two_hidden_layers(be, hidden):
    obs_dim, R, A = 5, 2, 3
    p0 = random_params(np.random.default_rng(sum(hidden)), obs_dim + R, A, hidden)
    for T, wgs in ((17, 0), (33, 2), (33, 1)):
        check(be, hidden[0] + T, T, obs_dim, R, A, hidden, p0, max_workgroups=wgs)


def test_a_row_at_the_upper_clamp(be):
    """z_1 = -25 tanh(5 x_0) and z_0 = 0 up to small noise: a row with x_0 = 1 has p_0 > 1 - eps (upper clamp when it took action
    0, lower clamp when it took action 1), a row with x_0 = 0 or -1 is far inside.  The margins are checked on the oracle."""
    obs_dim, R, A, H, T = 3, 1, 2, 31, 33
    rng = np.random.default_rng(7)
    D = obs_dim + R
    W0, b0 = 0.01 * rng.standard_normal((H, D)), np.zeros(H)
    Wo, bo = 0.01 * rng.standard_normal((A, H)), np.zeros(A)
    W0[0] = 0.0
    W0[0, 0] = 5.0
    Wo[:, 0] = (0.0, -25.0)
    p0 = np.concatenate([a.reshape(-1) for a in (W0, b0, Wo, bo)]).astype(np.float32)
    obs, acc, actions, rewards = episode(rng, T, obs_dim, R, A)
    obs[:, 0] = rng.integers(-1, 2, size=T)
    want = check(be, 7, T, obs_dim, R, A, (H,), p0, ep=(obs, acc, actions, rewards))
    pa = want["probs"][np.arange(T), actions]
    upper, lower = pa > 1 - ec.EPS, pa < ec.EPS
    assert upper.sum() >= 3 and lower.sum() >= 3 and (~upper & ~lower).sum() >= 10, (upper.sum(), lower.sum())
    assert (want["logp"][upper] == np.log(1 - np.float64(ec.EPS))).all() and (want["logp"][lower] == np.log(np.float64(ec.EPS))).all()
    inside = pa[~upper & ~lower]
    assert inside.min() > 1e-3 and inside.max() < 1 - 1e-3, "a row lies near a clamp boundary"
    assert (1 - pa[upper]).max() < 1e-9 and pa[lower].max() < 1e-9
