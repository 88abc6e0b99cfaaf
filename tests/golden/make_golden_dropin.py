"""Checkpoints written by the UNMODIFIED reference agents, for the drop-in checkpoint tests (tests/test_dropin_reference.py).

    PYTHONDONTWRITEBYTECODE=1 python -B tests/golden/make_golden_dropin.py

Needs the reference tree (oracle/ref_harness.py's stubs stand in for gymnasium / wandb / pymoo).  The reference's ``Envelope``
(net [32, 32], 6 observations, 3 actions, 2 objectives, PER) takes three ``update()`` steps on 64 seeded transitions and its
``CAPQL`` (net [32, 32], 5 observations, 2 action dimensions, 2 objectives) one step on 32; each is saved with the reference's own
``save()``.  Outputs: ``tests/golden/dropin_envelope_ref.tar``, ``tests/golden/dropin_capql_ref.tar``.
"""
from __future__ import annotations

import os
import sys
import tempfile

import numpy as np
import torch as th

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import ref_harness as rh  # noqa: E402


def main():
    rh.install_stubs()
    from morl_baselines.multi_policy.capql.capql import CAPQL as RefCAPQL
    from morl_baselines.multi_policy.envelope.envelope import Envelope as RefEnvelope

    cpu = th.device("cpu")
    tmp = tempfile.mkdtemp()
    env = rh.FakeEnv(obs_dim=6, n_actions=3, reward_dim=2)
    th.manual_seed(0)
    np.random.seed(0)
    ref = RefEnvelope(env, net_arch=[32, 32], batch_size=8, num_sample_w=4, buffer_size=256, per=True, learning_starts=0,
                      log=False, seed=0, device=cpu)
    rng = np.random.default_rng(0)
    for _ in range(64):
        ref.replay_buffer.add(rng.standard_normal(6).astype(np.float32), rng.integers(3), rng.standard_normal(2).astype(np.float32),
                              rng.standard_normal(6).astype(np.float32), rng.random() < 0.1)
    ref.global_step = 5
    for _ in range(3):
        ref.update()
        ref.global_step += 1
    ref.save(save_replay_buffer=False, save_dir=tmp, filename="env")

    cenv = rh.FakeEnv(obs_dim=5, reward_dim=2, act_dim=2, env_id="fake-hopper-v0")
    th.manual_seed(0)
    np.random.seed(0)
    cap = RefCAPQL(cenv, net_arch=[32, 32], batch_size=8, buffer_size=128, learning_starts=0, log=False, seed=0, device=cpu)
    rng = np.random.default_rng(0)
    for _ in range(32):
        w = rng.dirichlet(np.ones(2)).astype(np.float32)
        cap.replay_buffer.push(rng.standard_normal(5).astype(np.float32), rng.uniform(-1, 1, 2).astype(np.float32), w,
                               rng.standard_normal(2).astype(np.float32), rng.standard_normal(5).astype(np.float32), False)
    cap.update()
    cap.save(save_dir=tmp, filename="cap", save_replay_buffer=False)

    for src, dst in (("env.tar", "dropin_envelope_ref.tar"), ("cap.tar", "dropin_capql_ref.tar")):
        ck = th.load(os.path.join(tmp, src), weights_only=False)
        th.save(ck, os.path.join(HERE, dst))
        print("wrote", dst, sorted(ck))


if __name__ == "__main__":
    main()
