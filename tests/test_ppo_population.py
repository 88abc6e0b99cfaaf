"""A population of MO-PPO learners in one launch (``morl_ppo_update_n_pop`` / ``_forward_pop`` / ``_gae_pop``) is P independent
learners, bit for bit: every comparison here is ``np.array_equal`` between the population call and the single-learner entries
run one learner after the other from the same start.  No tolerance: the contract is identical arithmetic per learner."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch as th

import ppo_common as pm
import ppo_pop as pp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D, A, R = 5, 2, 2
T, E = 10, 3               # 30 table rows per learner
STEPS = (0, 7, 19)         # Adam steps taken before the call, per learner
LRS = (3e-4, 1e-3, 5e-5)


def learners(lib, dev, hidden, seeds, max_minibatch=20, steps=STEPS, **kw):
    return [pp.make_learner(lib, dev, s, D, A, R, hidden, T, E, max_minibatch, steps_done=st, with_moments=st > 0, **kw)
            for s, st in zip(seeds, steps)]


def shuffles(seed, P, n, M, rows=T * E):
    rng = np.random.default_rng(seed)
    return [np.stack([rng.permutation(rows)[:M] for _ in range(n)]).astype(np.int32) for _ in range(P)]


def close_all(*groups):
    for g in groups:
        for c in g:
            c.close()


def assert_same(tag, pop, seq, stats_pop, stats_seq):
    for i, (a, b) in enumerate(zip(pop, seq)):
        for name, x, y in zip(("params", "exp_avg", "exp_avg_sq"), pp.state(a), pp.state(b)):
            assert np.array_equal(x, y), f"{tag}: learner {i} {name} differs (max |diff| {np.abs(x - y).max():.3e})"
        assert np.array_equal(stats_pop[i], stats_seq[i]), f"{tag}: learner {i} statistics differ"
        assert np.isfinite(stats_pop[i]).all() and (stats_pop[i][:, 7] > 0).all(), f"{tag}: learner {i} took no real step"


@pytest.mark.parametrize("hidden", [(32,), (64, 32)], ids=["h32", "h64_32"])
@pytest.mark.parametrize("norm_adv", [True, False], ids=["norm", "raw"])
@pytest.mark.parametrize("clip_vloss", [True, False], ids=["vclip", "vplain"])
@pytest.mark.parametrize("param", pm.BACKENDS)
def test_population_step_is_three_learners(param, hidden, norm_adv, clip_vloss):
    """P = 3, n = 3 steps of M = 20 (two tiles, the second with 4 valid rows); parameters, rollouts, idx, Adam step counts
    (0, 7, 19) and learning rates all differ between the learners."""
    lib, dev = pm.backend(param)
    seeds = (11, 12, 13)
    pop, seq = learners(lib, dev, hidden, seeds), learners(lib, dev, hidden, seeds)
    idx = shuffles(5, 3, 3, 20)
    kw = dict(norm_adv=norm_adv, clip_vloss=clip_vloss, ent_coef=0.01)
    try:
        sp = pp.update_n_pop(lib, pop, idx, LRS, **kw)
        ss = [c.update_n(i, lr, **kw) for c, i, lr in zip(seq, idx, LRS)]
        assert_same("step", pop, seq, sp, ss)
        # the learners are different learners: a launch that stepped one of them three times would also be "equal to itself"
        assert not np.array_equal(pp.state(pop[0])[0], pp.state(pop[1])[0])
        assert [c.steps_done for c in pop] == [3, 10, 22]
    finally:
        close_all(pop, seq)


@pytest.mark.parametrize("param", pm.BACKENDS)
def test_population_of_one_is_update_n(param):
    lib, dev = pm.backend(param)
    pop, seq = learners(lib, dev, (32,), (21,), steps=(4,)), learners(lib, dev, (32,), (21,), steps=(4,))
    idx = shuffles(6, 1, 3, 20)
    try:
        sp = pp.update_n_pop(lib, pop, idx, LRS[:1])
        ss = [seq[0].update_n(idx[0], LRS[0])]
        assert_same("P=1", pop, seq, sp, ss)
    finally:
        close_all(pop, seq)


@pytest.mark.parametrize("param", pm.BACKENDS)
def test_learner_order_does_not_matter(param):
    lib, dev = pm.backend(param)
    seeds = (31, 32, 33)
    a, b = learners(lib, dev, (64, 32), seeds), learners(lib, dev, (64, 32), seeds)
    idx = shuffles(7, 3, 3, 20)
    order = [2, 0, 1]
    try:
        sa = pp.update_n_pop(lib, a, idx, LRS)
        sb = pp.update_n_pop(lib, [b[i] for i in order], [idx[i] for i in order], [LRS[i] for i in order])
        sb = [sb[order.index(i)] for i in range(3)]
        assert_same("order", a, b, sa, sb)
    finally:
        close_all(a, b)


@pytest.mark.parametrize("param", pm.BACKENDS)
def test_chunk_boundary(param):
    """P = chunk + 1 learners, M = 16 (one tile): the seventeenth learner goes into a launch of its own."""
    lib, dev = pm.backend(param)
    P = pp.CHUNK + 1
    seeds, steps, lrs = range(100, 100 + P), [3 * i for i in range(P)], [1e-4 * (1 + i) for i in range(P)]
    pop = learners(lib, dev, (32,), seeds, max_minibatch=16, steps=steps)
    seq = learners(lib, dev, (32,), seeds, max_minibatch=16, steps=steps)
    idx = shuffles(8, P, 2, 16)
    try:
        sp = pp.update_n_pop(lib, pop, idx, lrs)
        ss = [c.update_n(i, lr) for c, i, lr in zip(seq, idx, lrs)]
        assert_same("chunk", pop, seq, sp, ss)
    finally:
        close_all(pop, seq)


@pytest.mark.parametrize("param", pm.BACKENDS)
def test_population_of_64(param):
    """The largest population the entries promise (four launches per step), two of its learners checked against ``update_n``."""
    lib, dev = pm.backend(param)
    P = 64
    seeds, steps, lrs = range(300, 300 + P), [i % 5 for i in range(P)], [3e-4] * P
    pop = learners(lib, dev, (32,), seeds, max_minibatch=16, steps=steps)
    check = [0, 17, 63]
    seq = learners(lib, dev, (32,), [seeds[i] for i in check], max_minibatch=16, steps=[steps[i] for i in check])
    idx = shuffles(9, P, 1, 16)
    try:
        sp = pp.update_n_pop(lib, pop, idx, lrs)
        ss = [c.update_n(idx[i], lrs[i]) for c, i in zip(seq, check)]
        assert_same("P=64", [pop[i] for i in check], seq, [sp[i] for i in check], ss)
    finally:
        close_all(pop, seq)


@pytest.mark.parametrize("param", pm.BACKENDS)
def test_back_to_back_calls_without_a_synchronisation(param):
    """Two calls queued on one stream with different idx and statistics tensors, and the host arrays of the first call freed
    before the second: a queued launch reads its own copy of the records, and each learner's ticket is re-armed in between."""
    lib, dev = pm.backend(param)
    seeds = (41, 42, 43)
    pop, seq = learners(lib, dev, (32,), seeds), learners(lib, dev, (32,), seeds)
    idx1, idx2 = shuffles(9, 3, 3, 20), shuffles(10, 3, 2, 20)
    try:
        dev_idx = [[th.tensor(i).to(dev) for i in idx] for idx in (idx1, idx2)]
        stats = [[th.zeros(n, 8, dtype=th.float32, device=dev) for _ in pop] for n in (3, 2)]
        lib.check(pp.update_n_pop_raw(lib, pop, dev_idx[0], stats[0], 20, 3, LRS, STEPS))
        lib.check(pp.update_n_pop_raw(lib, pop, dev_idx[1], stats[1], 20, 2, LRS, [s + 3 for s in STEPS]))
        sp = [np.concatenate([a.cpu().numpy(), b.cpu().numpy()]) for a, b in zip(*stats)]
        ss = [np.concatenate([c.update_n(i1, lr), c.update_n(i2, lr)]) for c, i1, i2, lr in zip(seq, idx1, idx2, LRS)]
        assert_same("back to back", pop, seq, sp, ss)
    finally:
        close_all(pop, seq)


@pytest.mark.parametrize("rows", [4, 17])
@pytest.mark.parametrize("param", pm.BACKENDS)
def test_forward_pop(param, rows):
    lib, dev = pm.backend(param)
    ctxs = learners(lib, dev, (64, 32), (51, 52, 53), gae=False)
    rng = np.random.default_rng(rows)
    obs = [rng.standard_normal((rows, D)) for _ in ctxs]
    eps = [rng.standard_normal((rows, A)) for _ in ctxs]
    try:
        got = pp.forward_pop(lib, ctxs, obs, eps)
        got_v = pp.forward_pop(lib, ctxs, obs, value_only=True)
        for i, c in enumerate(ctxs):
            want = c.forward(obs[i], eps[i])
            for name, x, y in zip(("action", "logprob", "value"), got[i], want):
                assert np.array_equal(x, y), f"learner {i} {name}"
            assert np.array_equal(got_v[i][2], c.forward(obs[i], value_only=True)[2]), f"learner {i} value_only"
        assert not np.array_equal(got[0][2], got[1][2])
    finally:
        close_all(ctxs)


@pytest.mark.parametrize("use_gae", [True, False], ids=["gae", "returns"])
@pytest.mark.parametrize("TE", [(5, 3), (3, 65)], ids=["5x3", "3x65"])
@pytest.mark.parametrize("param", pm.BACKENDS)
def test_gae_pop(param, TE, use_gae):
    """(3, 65) is two blocks of the scan.  Weights, dones and next values are per learner.  The table is read back through a
    step each: the advantages and returns the scan left there are the ones the step trains on."""
    lib, dev = pm.backend(param)
    t, e = TE
    mk = lambda: [pp.make_learner(lib, dev, s, D, A, R, (32,), t, e, 8, gae=False) for s in (61, 62, 63)]  # noqa: E731
    pop, seq = mk(), mk()
    idx = shuffles(11, 3, 1, 8, rows=t * e)
    try:
        got = pp.gae_pop(lib, pop, 0.97, 0.9, use_gae)
        for i, c in enumerate(seq):
            want = c.gae(c.gae_np["next_value"], c.gae_np["next_done"], c.gae_np["weights"], 0.97, 0.9, use_gae)
            assert np.array_equal(got[i][0], want[0]), f"learner {i} returns"
            assert np.array_equal(got[i][1], want[1]), f"learner {i} advantages"
        assert not np.array_equal(got[0][1], got[1][1])
        sp = pp.update_n_pop(lib, pop, idx, LRS)       # (gae_pop marked every context's advantages as present)
        ss = [c.update_n(i, lr) for c, i, lr in zip(seq, idx, LRS)]
        assert_same("gae table", pop, seq, sp, ss)
    finally:
        close_all(pop, seq)


_COUNT_SNIPPET = r"""
import ctypes, os, sys
ROOT = sys.argv[1]
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np
import ppo_common as pm, ppo_pop as pp, test_ppo_population as t
lib, dev = pm.backend("sim")
count = lib.lib.hipsim_launch_count
count.restype = ctypes.c_longlong
out = {}
for P in (3, pp.CHUNK, pp.CHUNK + 1):
    ctxs = t.learners(lib, dev, (32,), range(P), max_minibatch=16, steps=[0] * P)
    idx = t.shuffles(1, P, 3, 16)
    c0 = count(); pp.update_n_pop(lib, ctxs, idx, [3e-4] * P); pop = count() - c0
    c0 = count()
    for c, i in zip(ctxs, idx):
        c.update_n(i, 3e-4)
    out[P] = (pop, count() - c0)
print("LAUNCHES", out)
"""


def test_launch_count():
    """n steps for P learners cost n * ceil(P / chunk) launches; the sequential form costs n * P (counted by the emulator)."""
    r = subprocess.run([sys.executable, "-c", _COUNT_SNIPPET, ROOT], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0 and "LAUNCHES" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    got = eval(r.stdout.split("LAUNCHES")[1].strip())
    n = 3
    assert got == {P: (n * -(-P // pp.CHUNK), n * P) for P in (3, pp.CHUNK, pp.CHUNK + 1)}, got


@pytest.mark.parametrize("param", pm.BACKENDS)
def test_refusals_leave_the_contexts_usable(param):
    lib, dev = pm.backend(param)
    seeds = (71, 72, 73)
    pop, seq = learners(lib, dev, (32,), seeds), learners(lib, dev, (32,), seeds)
    other = pp.make_learner(lib, dev, 74, D, A, R, (64,), T, E, 20)                   # another network shape
    small = pp.make_learner(lib, dev, 75, D, A, R, (32,), T, E, 8)                    # max_minibatch 8 < M
    bare = pm.Ctx(lib, dev, D, A, R, (32,), 20, np.zeros(pp.param_count(lib, D, A, R, (32,)), dtype=np.float32))   # no rollout
    nogae = pp.make_learner(lib, dev, 76, D, A, R, (32,), T, E, 20, gae=False)
    shape2 = pp.make_learner(lib, dev, 77, D, A, R, (32,), T + 1, E, 20)              # another T
    idx = shuffles(12, 3, 2, 20)
    idx_dev = [th.tensor(i).to(dev) for i in idx]
    stats = [th.zeros(2, 8, dtype=th.float32, device=dev) for _ in pop]
    ARG, STATE = -1, -3                                                                 # MORL_ERR_ARG, MORL_ERR_STATE

    def refused(rc, code, text):
        assert rc == code, (rc, code, lib.lib.morl_last_error())
        assert text.encode() in lib.lib.morl_last_error(), lib.lib.morl_last_error()

    def upd(ctxs, **kw):
        return pp.update_n_pop_raw(lib, ctxs, idx_dev[:len(ctxs)], stats[:len(ctxs)], 20, 2, LRS[:len(ctxs)], [0] * len(ctxs), **kw)

    try:
        before = [pp.state(c) for c in pop]
        refused(upd([pop[0], pop[1], pop[0]]), ARG, "same context twice")
        refused(upd(pop, handle_array=(C.c_void_p * 3)(pop[0].h, None, pop[2].h)), ARG, "ctxs[1] is NULL")
        refused(upd([pop[0], other]), ARG, "other network shapes")
        refused(lib.lib.morl_ppo_update_n_pop(0, None, None, None, None, 1, None, 20, None, None, 0.2, 0.0, 0.5, 0.5, 1, 1, None, None),
                ARG, "population of 0")
        refused(upd([pop[0], small]), STATE, "max_minibatch")
        refused(upd([pop[0], bare]), STATE, "no rollout")
        refused(upd([pop[0], nogae]), STATE, "no advantages")
        refused(lib.lib.morl_ppo_update_n_pop(2, pp.handles(pop[:2]), pp.ptrs([pop[0].params, None]), pp.ptrs([c.m for c in pop[:2]]),
                                              pp.ptrs([c.v for c in pop[:2]]), 2, pp.ptrs(idx_dev[:2]), 20, (C.c_double * 2)(1e-3, 1e-3),
                                              (C.c_int * 2)(0, 0), 0.2, 0.0, 0.5, 0.5, 1, 1, pp.ptrs(stats[:2]), None), ARG, "params[1] is NULL")
        # forward_pop / gae_pop: the same checks of the population, and gae_pop's own
        h3 = pp.handles([pop[0], pop[1], pop[0]])
        p3 = pp.ptrs([pop[0].params] * 3)
        refused(lib.lib.morl_ppo_forward_pop(3, h3, p3, p3, p3, 4, 0, p3, p3, p3, None), ARG, "same context twice")
        refused(lib.lib.morl_ppo_forward_pop(0, h3, p3, p3, p3, 4, 0, p3, p3, p3, None), ARG, "population of 0")
        refused(lib.lib.morl_ppo_forward_pop(2, pp.handles([pop[0], other]), p3, p3, p3, 4, 0, p3, p3, p3, None), ARG, "other network shapes")
        refused(lib.lib.morl_ppo_gae_pop(3, h3, p3, p3, p3, 0.99, 0.95, 1, None, None, None), ARG, "same context twice")
        refused(lib.lib.morl_ppo_gae_pop(2, pp.handles([pop[0], shape2]), p3, p3, p3, 0.99, 0.95, 1, None, None, None), STATE, "11 x 3")
        refused(lib.lib.morl_ppo_gae_pop(2, pp.handles([pop[0], bare]), p3, p3, p3, 0.99, 0.95, 1, None, None, None), STATE, "no rollout")
        refused(lib.lib.morl_ppo_gae_pop(2, pp.handles(pop[:2]), p3, None, p3, 0.99, 0.95, 1, None, None, None), ARG, "next_done is NULL")
        # nothing was launched, and the contexts still work
        for c, b in zip(pop, before):
            assert all(np.array_equal(x, y) for x, y in zip(pp.state(c), b))
        sp = pp.update_n_pop(lib, pop, idx, LRS)
        ss = [c.update_n(i, lr) for c, i, lr in zip(seq, idx, LRS)]
        assert_same("after refusals", pop, seq, sp, ss)
    finally:
        close_all(pop, seq, [other, small, bare, nogae, shape2])
