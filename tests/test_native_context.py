"""The host layer the learners share: ``native.Context`` (the one owner of a library context), ``acnets.flat_views`` and the PPO
epoch schedule of ``mo_ppo.run_epochs``.  ``sim``: kernel sources under the wave emulator; ``hip``: the gfx950 library (-m gpu)."""
import copy
import gc
import pickle

import numpy as np
import pytest
import torch as th

import pcn_common as pcm

import morl_baselines_amd.native as native
from morl_baselines_amd.acnets import flat_views
from morl_baselines_amd.mo_ppo import STAT_NAMES, run_epochs
from morl_baselines_amd.native import Context

D, R, A, H, MAX_BATCH = 3, 2, 2, 32, 4              # the smallest legal PCN shapes
PCN_ARGS = (D, R, A, H, 0, MAX_BATCH)
PPO_ARGS = (3, 2, 2, 1, 32, 0, 4)                   # D, A, R, one hidden layer of 32, max_minibatch


@pytest.fixture(scope="module", params=pcm.BACKENDS)
def be(request):
    lib, dev = pcm.backend(request.param)
    native.use_library(lib if request.param == "sim" else None)
    yield lib, dev, request.param
    native.use_library(None)


def pcn_forward(lib, dev, ctx):
    """One ``morl_pcn_forward`` of 2 rows with ``ctx`` in the context slot: (return code, output bytes)."""
    gen = th.Generator().manual_seed(5)
    P = lib.family_param_count("pcn", D, R, A, H)
    params = (0.1 * th.randn(P, generator=gen)).to(dev)
    scaling = th.ones(R + 1).to(dev)
    obs, dr, dh = th.randn(2, D, generator=gen).to(dev), th.randn(2, R, generator=gen).to(dev), th.ones(2, 1).to(dev)
    out = th.zeros(2, A, device=dev)
    rc = lib.lib.morl_pcn_forward(ctx, params.data_ptr(), scaling.data_ptr(), obs.data_ptr(), dr.data_ptr(), dh.data_ptr(), 2,
                                  out.data_ptr(), lib.stream_of(out))
    return rc, out.cpu().numpy().tobytes()


def test_a_fresh_context_is_the_pointer_it_owns(be):
    lib, dev, _ = be
    ctx = Context(lib, "pcn", *PCN_ARGS)
    assert ctx and isinstance(ctx.value, int) and ctx.value != 0
    rc_obj, through_object = pcn_forward(lib, dev, ctx)
    rc_int, through_integer = pcn_forward(lib, dev, ctx.value)
    assert rc_obj == 0 and rc_int == 0
    assert through_object == through_integer and np.isfinite(np.frombuffer(through_object, dtype=np.float32)).all()
    assert ctx.close()


def test_close_is_idempotent_and_a_closed_context_is_null(be):
    lib, dev, _ = be
    ctx = Context(lib, "pcn", *PCN_ARGS)
    assert ctx.close() is True
    assert ctx.close() is False and not ctx and ctx.value is None
    with pytest.raises(RuntimeError, match="NULL argument"):         # (the argument check: no kernel is launched)
        lib.check(pcn_forward(lib, dev, ctx)[0])
    del ctx
    gc.collect()
    ctx = Context(lib, "ppo", *PPO_ARGS)                              # never closed by hand: __del__ does it
    del ctx
    gc.collect()


def test_a_refused_create_raises_and_leaves_nothing_to_destroy(be):
    lib, _, _ = be
    with pytest.raises(RuntimeError, match="libmorl_hip error"):
        Context(lib, "pcn", D, R, A, 33, 0, MAX_BATCH)               # (33 is not a hidden width of the PCN kernels)
    gc.collect()
    with pytest.raises(ValueError) as refused:
        lib.family_param_count("pcn", D, R, A, 33, error=ValueError)
    assert "libmorl_hip error" not in str(refused.value) and str(refused.value)
    with pytest.raises(RuntimeError, match="libmorl_hip error"):
        lib.family_param_count("pcn", D, R, A, 33)


@pytest.mark.parametrize("family,args", [("pcn", PCN_ARGS), ("ppo", PPO_ARGS)])
def test_a_context_refuses_copy_deepcopy_and_pickle(be, family, args):
    lib, _, _ = be
    ctx = Context(lib, family, *args)
    for duplicate in (copy.copy, copy.deepcopy, pickle.dumps):
        with pytest.raises(TypeError, match=f"morl_{family}"):
            duplicate(ctx)
    with pytest.raises(TypeError, match=f"morl_{family}"):
        copy.deepcopy({"_ctx": ctx})                                  # (whatever holds one cannot be deep-copied generically)
    assert ctx.close()                                                # (still the one owner)


def test_owners_without_a_deepcopy_of_their_own_refuse_it():
    """``PCN`` and ``GPIEngine`` have no ``__deepcopy__``: the default one stops at the library or the context, whichever it
    reaches first, so no second object ever holds the pointer; the original keeps working.  A host-side property: on the
    emulator only."""
    import simlib
    lib, dev = simlib.load_sim(), th.device("cpu")
    from morl_baselines_amd.gpi_engine import GPIEngine
    from morl_baselines_amd.pcn import PCN
    th.manual_seed(0)
    ag = PCN(pcm.SpacesEnv(D, A, R, False), np.ones(R + 1, dtype=np.float32), batch_size=MAX_BATCH, hidden_dim=H, log=False,
             seed=0, device=dev, lib=lib)
    eng = GPIEngine(D, A, R, [32, 32], max_rows=4, device=dev, lib=lib)
    for owner in (ag, eng):
        with pytest.raises(TypeError, match="cannot be copied"):
            copy.deepcopy(owner)
        del owner.lib                                                 # (with the library out of the way: the context refuses)
        with pytest.raises(TypeError, match="context cannot be copied"):
            copy.deepcopy(owner)
        owner.lib = lib
    assert ag._ctx and eng._h
    out = ag._forward(np.zeros((2, D)), np.ones((2, R)), np.ones((2, 1)))
    assert out.shape == (2, A) and np.isfinite(out).all()


# -- flat_views (no library) ----------------------------------------------------------------------------------------------------
def test_flat_views_alias_the_flat_tensor():
    flat = th.arange(11, dtype=th.float32)
    w, b, s = flat_views(flat, [(2, 3), (3,), th.Size([2])])
    assert tuple(w.shape) == (2, 3) and tuple(b.shape) == (3,) and tuple(s.shape) == (2,)
    assert th.equal(w, flat[:6].view(2, 3)) and th.equal(b, flat[6:9]) and th.equal(s, flat[9:])
    assert w.data_ptr() == flat.data_ptr() and b.data_ptr() == flat[6:].data_ptr() and s.data_ptr() == flat[9:].data_ptr()
    b.fill_(-1.0)
    w[1, 2] = 7.0
    assert flat[5] == 7.0 and (flat[6:9] == -1.0).all()
    flat[10] = 42.0
    assert s[1] == 42.0


@pytest.mark.parametrize("shapes", [[(2, 3), (3,)], [(2, 3), (3,), (3,)], []], ids=["under", "over", "none"])
def test_flat_views_refuses_shapes_that_do_not_consume_the_buffer(shapes):
    with pytest.raises(ValueError, match="do not match"):
        flat_views(th.zeros(11), shapes)


# -- the epoch schedule (no library) ---------------------------------------------------------------------------------------------
BATCH, MINIBATCH, EPOCHS, SEED = 10, 4, 3, 7
KL = STAT_NAMES.index("approx_kl")


def reference_minibatches(rng, epochs=EPOCHS):
    """The reference's loop (``mo_ppo.py:500-506``), literally: every minibatch is used before the next shuffle."""
    seen = []
    b_inds = np.arange(BATCH)
    for epoch in range(epochs):
        rng.shuffle(b_inds)
        for start in range(0, BATCH, MINIBATCH):
            end = start + MINIBATCH
            mb_inds = b_inds[start:end]
            seen.append(mb_inds.tolist())
    return seen


class FakeUpdate:
    """Records the calls; step k of the run reports ``approx_kl = kl_of_step(k)`` and its own number as the loss."""

    def __init__(self, kl_of_step=lambda k: 0.0):
        self.calls, self.steps, self.kl_of_step = [], 0, kl_of_step

    def __call__(self, idx):
        assert isinstance(idx, np.ndarray) and idx.ndim == 2
        self.calls.append(idx.copy())
        stats = th.zeros(len(idx), len(STAT_NAMES))
        for row in stats:
            row[0], row[KL] = self.steps, self.kl_of_step(self.steps)
            self.steps += 1
        return stats


@pytest.mark.parametrize("target_kl", [None, 1e9], ids=["one-pass", "per-epoch"])
def test_the_epoch_schedule_is_the_reference_loop(target_kl):
    want_rng = np.random.default_rng(SEED)
    want = reference_minibatches(want_rng)
    rng, fake = np.random.default_rng(SEED), FakeUpdate()
    stats = run_epochs(rng, BATCH, MINIBATCH, EPOCHS, target_kl, fake)
    assert [mb.tolist() for call in fake.calls for mb in call] == want
    assert rng.bit_generator.state == want_rng.bit_generator.state
    assert [call.shape for call in fake.calls] == [(2, 4), (1, 2)] * 3          # [4,4] [2] [4,4] [2] [4,4] [2]
    assert tuple(stats.shape) == (9, len(STAT_NAMES)) and stats[:, 0].tolist() == list(range(9))


def test_the_epoch_schedule_stops_on_target_kl():
    want_rng = np.random.default_rng(SEED)
    want = reference_minibatches(want_rng, epochs=2)
    rng, fake = np.random.default_rng(SEED), FakeUpdate(lambda k: 0.02 if k >= 3 else 0.0)      # (epoch 2 is steps 3, 4, 5)
    stats = run_epochs(rng, BATCH, MINIBATCH, EPOCHS, 0.01, fake)
    assert [mb.tolist() for call in fake.calls for mb in call] == want
    assert rng.bit_generator.state == want_rng.bit_generator.state, "not exactly two shuffles were drawn"
    assert [call.shape for call in fake.calls] == [(2, 4), (1, 2)] * 2
    assert tuple(stats.shape) == (6, len(STAT_NAMES)) and stats[:, 0].tolist() == list(range(6))


def test_a_batch_the_minibatches_divide_goes_to_the_device_in_one_call():
    want_rng = np.random.default_rng(SEED)
    b_inds, want = np.arange(8), []
    for _ in range(3):
        want_rng.shuffle(b_inds)
        want += [b_inds[:4].tolist(), b_inds[4:].tolist()]
    rng, fake = np.random.default_rng(SEED), FakeUpdate()
    stats = run_epochs(rng, 8, 4, 3, None, fake)
    assert len(fake.calls) == 1 and fake.calls[0].tolist() == want and tuple(stats.shape) == (6, len(STAT_NAMES))
    assert rng.bit_generator.state == want_rng.bit_generator.state
