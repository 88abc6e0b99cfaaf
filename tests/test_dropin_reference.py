"""The drop-in claim, held by a test: with the reference package importable (here: the unmodified tree at /root/reference
behind the import stubs of oracle/ref_harness.py), the HIP agents ARE subclasses of the reference's own
``MOAgent`` / ``MOPolicy`` (``common/morl_algorithm.py:23-337``), train through ``update()``, and exchange checkpoints with the
reference's agents in both directions (``envelope.py:230-261``; ``capql.py`` save / load).  The package decides its base
classes at import time, so the scenario runs in a fresh interpreter (emulated kernel library: no GPU needed).
Skipped where the reference tree is absent (the GPU box).

The checkpoint exchange is also held without the reference: ``tests/golden/dropin_*_ref.tar`` are checkpoints the reference's own
agents wrote (``tests/golden/make_golden_dropin.py``).  The HIP agents load them, train on from them, and write checkpoints of the
same layout -- the keys, shapes and dtypes the reference's ``load()`` hands to ``load_state_dict``."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch as th

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import ref_harness  # noqa: E402


SCRIPT = r'''
import os, sys, tempfile
ROOT = sys.argv[1]
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]
import numpy as np, torch as th
import ref_harness
ref_harness.install_stubs()                      # gymnasium / wandb / pymoo stand-ins, /root/reference on sys.path
from morl_baselines.common.morl_algorithm import MOAgent as RefMOAgent, MOPolicy as RefMOPolicy
import simlib
import morl_baselines_amd.native as native
lib = simlib.load_sim()
native.use_library(lib)
import morl_baselines_amd.api as api
assert api.HAVE_REFERENCE_API, "the reference's base classes were not picked up"
assert api.MOAgent is RefMOAgent and api.MOPolicy is RefMOPolicy
from morl_baselines_amd.envelope import Envelope
from test_host_api import _fill

cpu = th.device("cpu")
# ---- Envelope ------------------------------------------------------------------------------------------------------------
env = ref_harness.FakeEnv(obs_dim=6, n_actions=3, reward_dim=2)     # spaces of the (stubbed) gymnasium types
env.D, env.A, env.R = 6, 3, 2
th.manual_seed(0); np.random.seed(0)
ag = Envelope(env, net_arch=[32, 32], batch_size=8, num_sample_w=4, buffer_size=256, per=True, learning_starts=0, log=False,
              seed=0, device=cpu, lib=lib)
assert isinstance(ag, RefMOAgent) and isinstance(ag, RefMOPolicy)
_fill(ag.replay_buffer, 64, env.D, env.A, env.R)
ag.global_step = 5
for _ in range(3):
    ag.update(); ag.global_step += 1
assert np.isfinite(ag.last_loss())
tmp = tempfile.mkdtemp()
ag.save(save_replay_buffer=False, save_dir=tmp, filename="hip")
from morl_baselines.multi_policy.envelope.envelope import Envelope as RefEnvelope
ref = RefEnvelope(env, net_arch=[32, 32], batch_size=8, num_sample_w=4, buffer_size=256, per=True, learning_starts=0,
                  log=False, seed=1, device=cpu)
ref.load(os.path.join(tmp, "hip.tar"), load_replay_buffer=False)      # HIP checkpoint -> reference agent
ours = ag.q_net.state_dict()
for k, v in ref.q_net.state_dict().items():
    assert th.equal(v, ours[k].cpu()), k
assert len(ref.q_optim.state_dict()["state"]) == len(ours)              # Adam moments travelled too
for p_ref, (name, _) in zip(ref.q_net.parameters(), ref.q_net.named_parameters()):
    st = ref.q_optim.state[p_ref]
    assert int(float(st["step"])) == 3 and float(st["exp_avg"].abs().sum()) > 0.0
# the reference keeps training from it
ref.replay_buffer = None
# reverse direction: reference checkpoint -> HIP agent
th.manual_seed(3)
ref2 = RefEnvelope(env, net_arch=[32, 32], batch_size=8, num_sample_w=4, buffer_size=256, per=True, learning_starts=0,
                   log=False, seed=2, device=cpu)
ref2.save(save_replay_buffer=False, save_dir=tmp, filename="ref")
ag.load(os.path.join(tmp, "ref.tar"), load_replay_buffer=False)
want = ref2.q_net.state_dict()
for k, v in ag.q_net.state_dict().items():
    assert th.equal(v.cpu(), want[k]), k
for k, v in ag.target_q_net.state_dict().items():
    assert th.equal(v.cpu(), want[k]), k
ag.update()                                                            # and the HIP agent trains on from it
print("envelope drop-in ok")

# ---- one actor-critic agent: CAPQL ---------------------------------------------------------------------------------------
from morl_baselines_amd.capql import CAPQL
from morl_baselines.multi_policy.capql.capql import CAPQL as RefCAPQL
cenv = ref_harness.FakeEnv(obs_dim=5, reward_dim=2, act_dim=2, env_id="fake-hopper-v0")
th.manual_seed(0); np.random.seed(0)
cap = CAPQL(cenv, net_arch=[32, 32], batch_size=8, buffer_size=128, learning_starts=0, log=False, seed=0, device=cpu, lib=lib)
assert isinstance(cap, RefMOAgent) and isinstance(cap, RefMOPolicy)
rng = np.random.default_rng(0)
for _ in range(32):
    w = rng.dirichlet(np.ones(2)).astype(np.float32)
    cap.replay_buffer.push(rng.standard_normal(5).astype(np.float32), rng.uniform(-1, 1, 2).astype(np.float32), w,
                           rng.standard_normal(2).astype(np.float32), rng.standard_normal(5).astype(np.float32), False)
cap.update()
cap.save(save_dir=tmp, filename="cap_hip", save_replay_buffer=False)
rcap = RefCAPQL(cenv, net_arch=[32, 32], batch_size=8, buffer_size=128, learning_starts=0, log=False, seed=5, device=cpu)
rcap.load(os.path.join(tmp, "cap_hip.tar"), load_replay_buffer=False)
for mine, theirs in ((cap.policy, rcap.policy), (cap.q_nets[0], rcap.q_nets[0]), (cap.q_nets[1], rcap.q_nets[1])):
    a, b = mine.state_dict(), theirs.state_dict()
    assert list(a.keys()) == list(b.keys())
    for k in a:
        assert th.equal(a[k].cpu(), b[k]), k
print("capql drop-in ok")
'''


@pytest.mark.skipif(not ref_harness.reference_available(), reason="reference tree not mounted")
def test_hip_agents_are_reference_subclasses_and_exchange_checkpoints():
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    r = subprocess.run([sys.executable, "-c", SCRIPT, ROOT], capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + "\n" + r.stderr[-4000:]
    assert "envelope drop-in ok" in r.stdout and "capql drop-in ok" in r.stdout


GOLDEN = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def sim():
    import morl_baselines_amd.native as native
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import simlib
    lib = simlib.load_sim()
    native.use_library(lib)
    yield lib
    native.use_library(None)


def _same_layout(mine, ref, path="ckpt"):
    """Same keys, tensor shapes and dtypes, list lengths and leaf types all the way down.  An optimiser's param group is matched
    as torch's ``Optimizer.load_state_dict`` matches it: the same parameter indices; of its options, those both sides carry (a
    newer torch adds option keys, and fills the ones a checkpoint lacks with the optimiser's defaults)."""
    if isinstance(ref, dict) and "params" in ref and "lr" in ref:
        assert isinstance(mine, dict) and mine.get("params") == ref["params"], (path, mine, ref)
        for k in set(ref) & set(mine):
            _same_layout(mine[k], ref[k], f"{path}[{k!r}]")
    elif isinstance(ref, dict):
        assert isinstance(mine, dict) and sorted(mine, key=str) == sorted(ref, key=str), (path, list(mine), list(ref))
        for k in ref:
            _same_layout(mine[k], ref[k], f"{path}[{k!r}]")
    elif isinstance(ref, (list, tuple)):
        assert isinstance(mine, (list, tuple)) and len(mine) == len(ref), path
        for i, (a, b) in enumerate(zip(mine, ref)):
            _same_layout(a, b, f"{path}[{i}]")
    elif isinstance(ref, th.Tensor):
        assert isinstance(mine, th.Tensor) and mine.shape == ref.shape and mine.dtype == ref.dtype, (path, mine, ref)
    else:
        assert type(mine) is type(ref) or (isinstance(ref, (int, float)) and isinstance(mine, (int, float))), (path, mine, ref)


def _adam_steps(opt_sd):
    return {int(float(st["step"])) for st in opt_sd["state"].values()}


def test_envelope_loads_a_reference_checkpoint_and_writes_its_layout(sim, tmp_path):
    from morl_baselines_amd.envelope import Envelope
    from test_host_api import _fill
    ref = th.load(os.path.join(GOLDEN, "dropin_envelope_ref.tar"), weights_only=False)
    assert _adam_steps(ref["q_net_optimizer_state_dict"]) == {3}
    env = ref_harness.FakeEnv(obs_dim=6, n_actions=3, reward_dim=2)
    th.manual_seed(0)
    np.random.seed(0)
    ag = Envelope(env, net_arch=[32, 32], batch_size=8, num_sample_w=4, buffer_size=256, per=True, learning_starts=0, log=False,
                  seed=0, device=th.device("cpu"), lib=sim)
    ag.load(os.path.join(GOLDEN, "dropin_envelope_ref.tar"), load_replay_buffer=False)      # reference checkpoint -> HIP agent
    for net in (ag.q_net, ag.target_q_net):
        mine = net.state_dict()
        assert list(mine) == list(ref["q_net_state_dict"])
        for k, v in ref["q_net_state_dict"].items():
            assert th.equal(mine[k].cpu(), v), k
    assert ag._adam_step == 3
    ref_state = ref["q_net_optimizer_state_dict"]["state"]
    for i, prm in enumerate(ag.q_net.ordered_parameters()):       # Adam's moments arrived in the flat buffers the kernels update
        st = ag.q_optim.state[prm]
        assert th.equal(st["exp_avg"].cpu(), ref_state[i]["exp_avg"]) and th.equal(st["exp_avg_sq"].cpu(), ref_state[i]["exp_avg_sq"])
    _fill(ag.replay_buffer, 64, 6, 3, 2)
    ag.global_step = 8
    p0 = ag.q_net.flat.clone()
    ag.update()                                                    # and the HIP agent trains on from it
    assert np.isfinite(ag.last_loss()) and ag._adam_step == 4 and not th.equal(ag.q_net.flat, p0)
    ag.save(save_replay_buffer=False, save_dir=str(tmp_path), filename="hip")
    mine = th.load(os.path.join(tmp_path, "hip.tar"), weights_only=False)
    _same_layout(mine, ref)                                        # what the reference's load() reads, key for key
    assert _adam_steps(mine["q_net_optimizer_state_dict"]) == {4}
    for k, v in ag.q_net.state_dict().items():
        assert th.equal(mine["q_net_state_dict"][k], v.cpu()), k


def test_capql_loads_a_reference_checkpoint_and_writes_its_layout(sim, tmp_path):
    from morl_baselines_amd.capql import CAPQL
    ref = th.load(os.path.join(GOLDEN, "dropin_capql_ref.tar"), weights_only=False)
    cenv = ref_harness.FakeEnv(obs_dim=5, reward_dim=2, act_dim=2, env_id="fake-hopper-v0")
    th.manual_seed(0)
    np.random.seed(0)
    cap = CAPQL(cenv, net_arch=[32, 32], batch_size=8, buffer_size=128, learning_starts=0, log=False, seed=0, device=th.device("cpu"),
                lib=sim)
    cap.load(os.path.join(GOLDEN, "dropin_capql_ref.tar"), load_replay_buffer=False)       # reference checkpoint -> HIP agent
    nets = [("policy_state_dict", cap.policy)] + [(f"q_net_{i}_state_dict", q) for i, q in enumerate(cap.q_nets)] + \
           [(f"target_q_net_{i}_state_dict", q) for i, q in enumerate(cap.target_q_nets)]
    for key, net in nets:
        mine = net.state_dict()
        assert list(mine) == list(ref[key]), key
        for k, v in ref[key].items():
            assert th.equal(mine[k].cpu(), v), (key, k)
    rng = np.random.default_rng(0)
    for _ in range(32):
        w = rng.dirichlet(np.ones(2)).astype(np.float32)
        cap.replay_buffer.push(rng.standard_normal(5).astype(np.float32), rng.uniform(-1, 1, 2).astype(np.float32), w,
                               rng.standard_normal(2).astype(np.float32), rng.standard_normal(5).astype(np.float32), False)
    p0 = {k: v.clone() for k, v in cap.policy.state_dict().items()}
    cap.update()                                                   # and the HIP agent trains on from it
    assert any(not th.equal(v.cpu(), p0[k].cpu()) for k, v in cap.policy.state_dict().items())
    cap.save(save_dir=str(tmp_path), filename="cap_hip", save_replay_buffer=False)
    mine = th.load(os.path.join(tmp_path, "cap_hip.tar"), weights_only=False)
    _same_layout(mine, ref)                                        # what the reference's load() reads, key for key
    for key in ("policy_optimizer_state_dict", "q_nets_optimizer_state_dict"):
        assert _adam_steps(mine[key]) == {s + 1 for s in _adam_steps(ref[key])}, key
