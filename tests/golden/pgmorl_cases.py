"""Configuration and seeded inputs of the PGMORL fixtures (tests/golden/pgmorl_*.npz, written by make_golden_pgmorl.py from the
unmodified reference).  The inputs are data: the fixtures store them next to the recorded outputs."""
import random

import numpy as np
import torch as th

WEIGHT_DELTAS = (0.2, 0.25, 0.5)


def weights_key(delta, dim):
    return f"w_{int(round(delta * 100))}_{dim}"


def reseed(seed):
    random.seed(seed)
    np.random.seed(seed)
    th.manual_seed(seed)


# -- performance buffers: few bins of two places, so that 40 evaluations overflow them
BUFFER = {2: dict(num_bins=6, max_size=2, origin=(-1.0, -1.0), seed=21), 3: dict(num_bins=4, max_size=2, origin=(-1.0, -1.0, -1.0), seed=22)}


def buffer_evals(dim, n=40):
    rng = np.random.default_rng(BUFFER[dim]["seed"])
    e = rng.uniform(0.0, 10.0, size=(n, dim))
    e[5] = -3.0                       # below the origin in every objective: centred to zero (2-D: outside the bins)
    e[11, 0] = -2.0                   # clipped in one objective
    e[17] = e[3]                      # equal norms: the later one goes behind the earlier one
    e[23] = e[9]
    e[29] = e[9][::-1] if dim == 2 else np.roll(e[9], 1)     # the same norm in another bin
    e[31] = 0.5 * e[12]               # the same direction, a smaller norm
    return e


# -- predictor: evaluations on a front-like arc, deltas that grow with the weight of the objective
PREDICTOR = dict(seed=31)


def predictor_memory(seed, n=12):
    rng = np.random.default_rng(seed)
    t = rng.uniform(0.15, 0.85, size=n)
    w = np.stack([t, 1.0 - t], axis=1).astype(np.float32)
    angle = rng.uniform(0.2, 1.35, size=n)
    before = 18.0 * np.stack([np.cos(angle), np.sin(angle)], axis=1) + rng.normal(0.0, 0.3, size=(n, 2))
    after = before + 3.0 * w.astype(np.float64) + rng.normal(0.0, 0.2, size=(n, 2))
    return dict(weights=w, before=before, after=after)


def predictor_queries(seed, n=6):
    rng = np.random.default_rng(seed + 1)
    t = rng.uniform(0.0, 1.0, size=n)
    w = np.stack([t, 1.0 - t], axis=1).astype(np.float32)
    angle = rng.uniform(0.2, 1.35, size=n)
    return dict(weights=w, evals=18.0 * np.stack([np.cos(angle), np.sin(angle)], axis=1))


# -- task / weight selection from a synthetic state
SELECTION = dict(seed=41, n_tasks=4, ref_point=np.zeros(2), delta_weight=0.25)


def selection_state(seed):
    rng = np.random.default_rng(seed + 100)
    mem = predictor_memory(seed + 200, n=14)
    angle = np.sort(rng.uniform(0.2, 1.35, size=5))
    pop = 18.0 * np.stack([np.cos(angle), np.sin(angle)], axis=1) + rng.normal(0.0, 0.3, size=(5, 2))
    return dict(pop_evals=pop, front=pop.copy(), mem_weights=mem["weights"], mem_before=mem["before"], mem_after=mem["after"])


def shuffled_candidates(generate_weights, delta_weight, seed):
    cw = generate_weights(delta_weight / 2.0, 2)
    np.random.default_rng(seed).shuffle(cw)
    return cw


# -- a seeded train(): pop 4, two warm-up iterations, one evolutionary generation of one iteration
TRACE = dict(seed=71, env=dict(num_envs=4, obs_dim=5, action_dim=2, reward_dim=2, horizon=9, seed=7, offset=(2.0, 2.0)),
             origin=(0.0, 0.0), ref_point=(0.0, 0.0), total_timesteps=3 * 4 * 8 * 4,
             algo=dict(num_envs=4, pop_size=4, warmup_iterations=2, steps_per_iteration=8, evolutionary_iterations=1,
                       delta_weight=0.25, net_arch=[32, 32], num_minibatches=2, update_epochs=2, learning_rate=1e-3, gamma=0.99,
                       num_performance_buffer=10, performance_buffer_size=2))
