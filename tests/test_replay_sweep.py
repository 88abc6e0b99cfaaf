"""Seeded sweep of the replay kernels (csrc/replay_kernels.h) over tree depths, batch sizes and edge draws, every case on the
emulator and on the GPU, every result against a plain numpy float64 oracle in the reference's operation order:

  * sum trees: ``envelope_oracle.SumTree`` (``set`` / ``batch_set`` / ``sample_from_uniforms``; pinned to the reference's own
    trace by tests/test_oracle_golden.py); trees built directly are adjacent pairs summed level by level from zero-padded leaves;
  * gathers: ``rec[np.clip(idx, 0, rows - 1), off:off + width]``.

Indices, gathered rows and tree nodes are compared with ``array_equal``.  The only tolerance is the ``rtol=3e-7`` that
``test_sumtree_trace_bit_exact`` already allows between the device's ``powf`` and numpy's float32 power; the tree arithmetic behind
it is still compared bit for bit (the device's own priorities go to the oracle).

Sizes: no tensor exceeds the 2^21-double tree of the deepest case (16 MB).  A record store therefore has at most ``MAX_ROWS`` rows;
trees with more leaves than that sample through the gathers' ``[0, rows)`` clamp, which is what the kernels document (the raw
index is written, the clamped row is read)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch as th

import envelope_oracle as orc
from test_kernels_parity import be  # noqa: F401  (be: the backend fixture)

import morl_baselines_amd.ops as ops

POW_RTOL = 3e-7          # test_sumtree_trace_bit_exact's bound on device powf against numpy's float32 power
MAX_ROWS = 32768         # rows of the largest record store: 32768 x 72 floats = 9.4 MB
GUARD = 8                # NaN rows on either side of the guarded record store


# ---- helpers --------------------------------------------------------------------------------------------------------------------
def levels_of(cap):
    return int(np.ceil(np.log2(cap))) + 1


def build_levels(leaves, n_levels):
    """Levels (root first) of the tree over ``leaves``: zero-padded to 2^(n_levels-1), adjacent pairs summed level by level."""
    full = np.zeros(2 ** (n_levels - 1))
    full[:len(leaves)] = leaves
    levels = [full]
    while len(levels[0]) > 1:
        levels.insert(0, levels[0].reshape(-1, 2).sum(1))
    assert len(levels) == n_levels
    return levels


def oracle_tree(cap, levels):
    t = orc.SumTree(cap)
    assert len(t.nodes) == len(levels)
    t.nodes = [lv.copy() for lv in levels]
    return t


def assert_tree(tree_d, tree_o, tag):
    got = tree_d.cpu().numpy()
    assert got.shape == (2 ** len(tree_o.nodes) - 1,)
    for l, nodes in enumerate(tree_o.nodes):
        assert np.array_equal(got[2 ** l - 1: 2 ** (l + 1) - 1], nodes), (tag, "level", l)


@functools.lru_cache(maxsize=4)
def records_np(rows, D, R, Ad, int_valued_actions, seed=0):
    """(rows, 2D+R+1+Ad) float32 records, read-only and shared by the cases of one shape."""
    rng = np.random.default_rng(seed)
    rec = rng.standard_normal((rows, 2 * D + R + 1 + Ad)).astype(np.float32)
    rec[:, 2 * D + R] = rng.random(rows) < 0.1
    if int_valued_actions:
        rec[:, 2 * D + R + 1:] = rng.integers(-3, 7, (rows, Ad))
    rec.setflags(write=False)
    return rec


def check_batch(out, rec, rows_idx, D, R, Ad, int_actions, tag):
    """``out`` = (obs, actions, rewards, next_obs, dones, ...) of gather_batch / sample_gather against ``rec[rows_idx]``."""
    obs, act, rew, nobs, done = (t.cpu().numpy() for t in out[:5])
    r = rec[rows_idx]
    o = 2 * D + R
    assert np.array_equal(obs, r[:, :D]), (tag, "obs")
    assert np.array_equal(nobs, r[:, D:2 * D]), (tag, "next_obs")
    assert np.array_equal(rew, r[:, 2 * D:o]), (tag, "rewards")
    assert np.array_equal(done[:, 0], r[:, o]), (tag, "dones")
    if int_actions:
        want = r[:, o + 1:].astype(np.int32)
        assert act.dtype == np.int32
        assert np.array_equal(act, want[:, 0] if Ad == 1 else want), (tag, "actions")
    else:
        assert act.dtype == np.float32
        assert np.array_equal(act, r[:, o + 1:]), (tag, "actions")


# ---- 1. the descent: sumtree_sample and sample_gather(tree=...), both against the oracle ----------------------------------------
DESCENT_CAPS = [1, 2, 3, 31, 32, 33, 1024, 1025, 2049, 70_000, 2 ** 20]
FILLS = ["ints", "reals", "sparse"]
DESCENT_B = 261
N_TIES = 30


def fill_leaves(rng, cap, fill):
    if fill == "ints":
        return rng.integers(1, 50, cap).astype(np.float64)
    if fill == "reals":
        return rng.random(cap) ** 4 + 1e-5
    leaves = np.where(rng.random(cap) < 1.0 / 7.0, rng.random(cap) + 0.01, 0.0)
    leaves[int(rng.integers(cap))] = 0.37            # (never an all-zero tree: the tie draws divide by the root)
    return leaves


def descent_uniforms(rng, leaves, root):
    k = rng.integers(len(leaves), size=N_TIES)
    k[0] = len(leaves) - 1
    cs = np.cumsum(leaves)
    ties = np.minimum(cs[k] / root, 1.0)             # (the sequential cumsum may exceed the pairwise root by an ulp)
    head = [0.0, 1.0, np.nextafter(1.0, 0.0), 0.5, 0.25, np.nextafter(0.5, 1.0)]
    u = np.concatenate([head, ties, rng.random(DESCENT_B - len(head) - N_TIES)])
    assert u.shape == (DESCENT_B,)
    return u, k, cs


DESCENT_CASES = [(cap, fill, False) for cap in DESCENT_CAPS for fill in FILLS] + [(1025, "reals", True)]


@pytest.mark.parametrize("cap,fill,int_actions", DESCENT_CASES,
                         ids=[f"cap{c}_L{levels_of(c)}_{f}{'_intact' if i else ''}" for c, f, i in DESCENT_CASES])
def test_descent_matches_the_oracle(be, cap, fill, int_actions):
    """Both descents (one load per level; five levels per wave-wide load) against ``SumTree.sample_from_uniforms`` at depths whose
    last chunk has every length 1..5, with u = 0, 1, nextafter(1, 0), exact ties (q == left) and zero-priority subtrees; the rows
    ``sample_gather`` returns are the records at the clamped index (72 floats: two trips of the lane loop)."""
    lib, dev, _ = be
    rng = np.random.default_rng(1000 + 7 * cap + FILLS.index(fill))
    L = levels_of(cap)
    leaves = fill_leaves(rng, cap, fill)
    lv = build_levels(leaves, L)
    tree_o = oracle_tree(cap, lv)
    u, k, cs = descent_uniforms(rng, leaves, lv[0][0])
    want = tree_o.sample_from_uniforms(u)
    assert want[0] == 0                              # u = 0: q = 0 is never > left
    if fill == "ints":                               # the premise of the tie draws: integer sums are exact, so draw 6 + j is
        t = slice(6, 6 + N_TIES)                     # exactly cumsum[k_j], meets q == left once on its way, and ends on leaf k_j
        exact = lv[0][0] * u[t] == cs[k]
        assert exact.any() and np.array_equal(want[t][exact], k[exact])
    tree_d = th.tensor(np.concatenate(lv)).to(dev)
    u_d = th.tensor(u).to(dev)

    got = ops.sumtree_sample(lib, tree_d, L, u_d).cpu().numpy()
    assert np.array_equal(got, want), "sumtree_sample"

    D, R, Ad = 33, 3, (1 if int_actions else 2)
    rows = min(cap, MAX_ROWS)
    rec = records_np(rows, D, R, Ad, int_actions)
    out = ops.sample_gather(lib, th.tensor(rec).to(dev), DESCENT_B, D, R, Ad, int_actions, tree=tree_d, n_levels=L,
                            u01_ptr=u_d.data_ptr())
    assert np.array_equal(out[5].cpu().numpy(), want), "sample_gather idx"
    check_batch(out, rec, np.clip(want, 0, rows - 1), D, R, Ad, int_actions, "sample_gather")
    assert np.array_equal(tree_d.cpu().numpy(), np.concatenate(lv))          # sampling writes nothing into the tree


# ---- 2. the gathers behind guard rows -------------------------------------------------------------------------------------------
G_CAP, G_B, G_W = 37, 4200, 150                      # 150 floats: three lane trips, the last partial; 4200 > 1024 workgroups x 4 rows
G_D, G_R, G_AD = 70, 4, 5                            # field boundaries at lanes 70, 140, 144, 145
FIELDS8 = [(0, 1), (1, 63), (64, 1), (65, 64), (129, 20), (149, 1), (3, 70), (60, 10)]


def guarded(dev, rec):
    """``rec`` as a contiguous view into the middle of a larger allocation whose other rows are NaN: an index that escapes the
    clamp by up to GUARD rows reads a NaN instead of memory outside the allocation."""
    big = th.full((rec.shape[0] + 2 * GUARD, rec.shape[1]), float("nan"), dtype=th.float32)
    big[GUARD:GUARD + rec.shape[0]] = th.tensor(rec)
    big = big.to(dev)
    view = big[GUARD:GUARD + rec.shape[0]]
    assert view.is_contiguous() and view.stride(0) == rec.shape[1] and view.shape == rec.shape
    return big, view


def gather_indices():
    rng = np.random.default_rng(31)
    idx = rng.integers(-5, G_CAP + 5, G_B)
    idx[:6] = [0, G_CAP - 1, -5, G_CAP + 4, -1, G_CAP]
    assert idx.min() == -5 and idx.max() == G_CAP + 4 and GUARD >= 5
    return idx


@pytest.mark.parametrize("int_actions", [False, True], ids=["float_actions", "int_actions"])
@pytest.mark.parametrize("entry", ["gather_batch", "sample_gather_idx"])
def test_gathers_clamp_and_stride_wide_records(be, entry, int_actions):
    lib, dev, _ = be
    assert 2 * G_D + G_R + 1 + G_AD == G_W
    rec = records_np(G_CAP, G_D, G_R, G_AD, int_actions, seed=3)
    big, view = guarded(dev, rec)
    idx = gather_indices()
    idx_d = th.tensor(idx, dtype=th.int64).to(dev)
    if entry == "gather_batch":
        out = ops.gather_batch(lib, view, idx_d, G_D, G_R, G_AD, int_actions=int_actions)
    else:
        out = ops.sample_gather(lib, view, G_B, G_D, G_R, G_AD, int_actions, idx_ptr=idx_d.data_ptr())
        assert np.array_equal(out[5].cpu().numpy(), idx)                     # the raw index is what is written
    check_batch(out, rec, np.clip(idx, 0, G_CAP - 1), G_D, G_R, G_AD, int_actions, entry)


@pytest.mark.parametrize("fields", [FIELDS8, [(60, 10)]], ids=["eight_fields", "one_field"])
def test_gather_fields_widths_overlaps_and_lane_edges(be, fields):
    lib, dev, _ = be
    rec = records_np(G_CAP, G_D, G_R, G_AD, False, seed=3)
    big, view = guarded(dev, rec)
    idx = gather_indices()
    outs = ops.gather_fields(lib, view, th.tensor(idx, dtype=th.int64).to(dev), fields)
    rows = rec[np.clip(idx, 0, G_CAP - 1)]
    assert len(outs) == len(fields)
    for (off, w), o in zip(fields, outs):
        assert np.array_equal(o.cpu().numpy(), rows[:, off:off + w]), (off, w)


@pytest.mark.parametrize("fields", [[], FIELDS8 + [(5, 5)], [(0, 4), (149, 2)], [(0, 151)], [(-1, 3)], [(7, 0)]],
                         ids=["no_field", "nine_fields", "field_past_the_record", "field_wider_than_the_record",
                              "negative_offset", "zero_width"])
def test_gather_fields_refuses_bad_field_lists(be, fields):
    """An error code and no launch: the outputs keep their sentinel."""
    lib, dev, _ = be
    rec = records_np(G_CAP, G_D, G_R, G_AD, False, seed=3)
    big, view = guarded(dev, rec)
    idx_d = th.tensor(gather_indices()[:64], dtype=th.int64).to(dev)
    with pytest.raises(RuntimeError, match="gather_fields"):
        ops.gather_fields(lib, view, idx_d, fields)
    n = len(fields)
    outs = [th.full((64, G_W + 2), -7.0, dtype=th.float32, device=dev) for _ in range(max(n, 1))]
    offs = (C.c_int32 * max(n, 1))(*[o for o, _ in fields])
    wids = (C.c_int32 * max(n, 1))(*[w for _, w in fields])
    ptrs = (C.c_void_p * max(n, 1))(*[o.data_ptr() for o in outs])
    rc = lib.lib.morl_gather_fields(view.data_ptr(), G_W, G_CAP, idx_d.data_ptr(), 64, n, offs, wids, ptrs, lib.stream_of(view))
    assert rc != 0
    if dev.type == "cuda":
        th.cuda.synchronize()
    assert all(bool((o == -7.0).all()) for o in outs)


# ---- 3. sumtree_update: the three priority forms, straight into the kernel ------------------------------------------------------
UPDATE_PAIRS = [(1, 1), (1, 1024), (5, 1024), (33, 1023), (300, 257), (1024, 1024), (4096, 1024), (70_000, 1024), (2 ** 20, 1000)]
PATTERNS = ["distinct", "random_dups", "one_index_repeated", "descending_clustered"]
FORMS = ["raw_alpha-1", "alpha0.6", "clamped0.01_alpha0.6"]
ALPHA, CLAMP = 0.6, 0.01


def update_indices(rng, cap, B, pattern):
    if pattern == "distinct":                        # (as distinct as the capacity allows)
        return rng.permutation(cap)[:B] if cap >= B else rng.permutation(np.arange(B) % cap)
    if pattern == "random_dups":
        idx = rng.integers(cap, size=B)
        if B > 1:
            idx[-1] = idx[0]                         # at least one duplicate, far from its first occurrence
        return idx
    if pattern == "one_index_repeated":
        return np.full(B, cap - 1)
    few = rng.choice(cap, size=min(3, cap), replace=False)
    return np.sort(rng.choice(few, size=B))[::-1].copy()


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("cap,B", UPDATE_PAIRS, ids=[f"cap{c}_L{levels_of(c)}_B{b}" for c, b in UPDATE_PAIRS])
def test_sumtree_update_forms_match_batch_set(be, cap, B, form):
    """Four updates in sequence on one tree (distinct / duplicated / one index B times / descending clusters), each compared
    level by level with ``SumTree.batch_set``, whose ``np.unique(return_index=True)`` defines "first occurrence wins"."""
    lib, dev, _ = be
    rng = np.random.default_rng(5000 + 13 * cap + B + 100 * FORMS.index(form))
    L = levels_of(cap)
    lv = build_levels(rng.random(cap) + 0.05, L)
    tree_o = oracle_tree(cap, lv)
    tree_d = th.tensor(np.concatenate(lv)).to(dev)
    rmax = 0.5 if form == FORMS[0] else 1e-5
    rmax_d = th.tensor([rmax], dtype=th.float64, device=dev)
    for n, pattern in enumerate(PATTERNS):
        tag = (cap, B, form, pattern)
        idx = update_indices(rng, cap, B, pattern)
        raw = (rng.random(B) * 2 * (n + 1)).astype(np.float32)
        if form == FORMS[0] and pattern == "one_index_repeated":
            raw = (rng.random(B) * np.float32(0.5 * rmax)).astype(np.float32)     # nothing exceeds the running maximum
            assert raw.max() < rmax
        if form == FORMS[2]:
            pos = (np.arange(B) + n) % 5
            raw[pos == 0] = 0.0
            raw[pos == 1] = (rng.random(int((pos == 1).sum())) * CLAMP).astype(np.float32)  # below the clamp
        if B > 1 and len(np.unique(idx)) < B:        # duplicates carry different priorities: the first occurrence must win
            assert len(np.unique(raw)) > 1
        idx_d, raw_d = th.tensor(idx, dtype=th.int64).to(dev), th.tensor(raw).to(dev)
        pr_d = th.full((B,), -1.0, dtype=th.float64, device=dev)
        if form == FORMS[0]:
            ops.sumtree_update(lib, tree_d, L, idx_d, raw_d, -1.0, rmax_d, pr_d)
            pr_dev = pr_d.cpu().numpy()
            assert np.array_equal(pr_dev, raw.astype(np.float64)), tag
        else:
            if form == FORMS[1]:
                ops.sumtree_update(lib, tree_d, L, idx_d, raw_d, ALPHA, rmax_d, pr_d)
                pr_o = (raw + np.float32(rmax)) ** np.float32(ALPHA)
            else:
                ops.sumtree_update_clamped(lib, tree_d, L, idx_d, raw_d, ALPHA, CLAMP, rmax_d, pr_d)
                pr_o = np.maximum(raw, np.float32(CLAMP)) ** np.float32(ALPHA)
            assert pr_o.dtype == np.float32
            pr_dev = pr_d.cpu().numpy()
            np.testing.assert_allclose(pr_dev, pr_o.astype(np.float64), rtol=POW_RTOL, err_msg=str(tag))
        pr32 = pr_dev.astype(np.float32)
        assert np.array_equal(pr32.astype(np.float64), pr_dev), tag               # priorities are float32 values
        new_rmax = max(rmax, float(pr32.max()))
        if form == FORMS[0] and pattern == "one_index_repeated":
            assert new_rmax == rmax
        rmax = new_rmax
        assert float(rmax_d.cpu()[0]) == rmax, tag
        tree_o.batch_set(idx, pr32)
        assert_tree(tree_d, tree_o, tag)


def test_sumtree_update_refuses_bad_arguments(be):
    """B = 0, B = 1025, and on the clamped entry clamp_min = 0 and alpha < 0: an error, and the tree, the running maximum and the
    priority output stay as they were."""
    lib, dev, _ = be
    cap, L = 300, levels_of(300)
    lv = build_levels(np.random.default_rng(8).random(cap), L)
    tree0 = np.concatenate(lv)
    tree_d = th.tensor(tree0).to(dev)
    rmax_d = th.tensor([0.25], dtype=th.float64, device=dev)
    idx_d = th.tensor(np.arange(1025) % cap, dtype=th.int64).to(dev)
    raw_d = th.full((1025,), 3.0, dtype=th.float32, device=dev)
    pr_d = th.full((1025,), -1.0, dtype=th.float64, device=dev)
    s = lib.stream_of(tree_d)
    with pytest.raises(RuntimeError, match="B=1025"):
        ops.sumtree_update(lib, tree_d, L, idx_d, raw_d, ALPHA, rmax_d, pr_d)
    with pytest.raises(RuntimeError, match="B=1025"):
        ops.sumtree_update_clamped(lib, tree_d, L, idx_d, raw_d, ALPHA, CLAMP, rmax_d, pr_d)
    with pytest.raises(RuntimeError):
        ops.sumtree_update(lib, tree_d, L, idx_d[:0], raw_d[:0], ALPHA, rmax_d, pr_d)
    with pytest.raises(RuntimeError):
        ops.sumtree_update_clamped(lib, tree_d, L, idx_d[:0], raw_d[:0], ALPHA, CLAMP, rmax_d, pr_d)
    # B = 0 with every array present: the size check itself refuses
    assert lib.lib.morl_sumtree_update(tree_d.data_ptr(), L, idx_d.data_ptr(), raw_d.data_ptr(), 0, ALPHA, rmax_d.data_ptr(),
                                       pr_d.data_ptr(), s) != 0
    assert b"B=0" in lib.lib.morl_last_error()
    assert lib.lib.morl_sumtree_update_clamped(tree_d.data_ptr(), L, idx_d.data_ptr(), raw_d.data_ptr(), 0, ALPHA, CLAMP,
                                               rmax_d.data_ptr(), pr_d.data_ptr(), s) != 0
    assert b"B=0" in lib.lib.morl_last_error()
    for alpha, clamp in ((ALPHA, 0.0), (-1.0, CLAMP), (ALPHA, -0.5), (float("nan"), CLAMP)):
        with pytest.raises(RuntimeError, match="clamp_min"):
            ops.sumtree_update_clamped(lib, tree_d, L, idx_d[:64], raw_d[:64], alpha, clamp, rmax_d, pr_d)
    if dev.type == "cuda":
        th.cuda.synchronize()
    assert np.array_equal(tree_d.cpu().numpy(), tree0)
    assert float(rmax_d.cpu()[0]) == 0.25 and bool((pr_d == -1.0).all())


# ---- 4. sumtree_set with explicit values ----------------------------------------------------------------------------------------
SET_CAPS = [1, 2, 50, 4097]
SET_CALLS = ["n1", "n2_same_leaf", "ring_wraps"]
SET_RMAX = 0.75


@pytest.mark.parametrize("call", SET_CALLS)
@pytest.mark.parametrize("cap", SET_CAPS, ids=[f"cap{c}_L{levels_of(c)}" for c in SET_CAPS])
def test_sumtree_set_explicit_values(be, cap, call):
    """Sequential ``SumTree.set`` with a value array in which every third entry is -1.0 ("the running maximum"), then one call
    with ``value=None`` on the same tree."""
    lib, dev, _ = be
    rng = np.random.default_rng(900 + cap + 10 * SET_CALLS.index(call))
    L = levels_of(cap)
    lv = build_levels(rng.random(cap), L)
    tree_o = oracle_tree(cap, lv)
    tree_d = th.tensor(np.concatenate(lv)).to(dev)
    rmax_d = th.tensor([SET_RMAX], dtype=th.float64, device=dev)
    if call == "n1":
        ptr = np.array([cap - 1])
    elif call == "n2_same_leaf":
        ptr = np.array([cap // 2, cap // 2])
    else:
        n = 3 * cap + 1 if cap <= 50 else 130
        ptr = (7 * np.arange(n) + 3) % cap           # at the small capacities: wraps past the end of the ring and revisits
        assert cap > 50 or len(np.unique(ptr)) < n   # leaves inside one call; at 4097: 130 distinct leaves of a 14-level tree
    n = len(ptr)
    value = rng.random(n) * 3
    value[2::3] = -1.0
    if call == "n2_same_leaf":
        value[:] = [-1.0, 1.625]                     # the second set sees the first one's leaf
    for p, v in zip(ptr, value):
        tree_o.set(int(p), SET_RMAX if v < 0 else float(v))
    ptr_d = th.tensor(ptr, dtype=th.int64).to(dev)
    ops.sumtree_set(lib, tree_d, L, ptr_d, th.tensor(value).to(dev), rmax_d)
    assert_tree(tree_d, tree_o, (cap, call, "values"))
    for p in ptr[::-1]:
        tree_o.set(int(p), SET_RMAX)
    ops.sumtree_set(lib, tree_d, L, th.tensor(ptr[::-1].copy(), dtype=th.int64).to(dev), None, rmax_d)
    assert_tree(tree_d, tree_o, (cap, call, "value=None"))
    assert float(rmax_d.cpu()[0]) == SET_RMAX        # set reads the running maximum, never writes it


# ---- 5. a short mixed trace at the workload's depth -----------------------------------------------------------------------------
def test_mixed_trace_at_the_workload_depth(be):
    """Capacity 100 000 (18 levels), D = 32, R = 3, Ad = 1 (69 floats): three rounds of set (200 new leaves) / sample_gather
    (B = 256) / sumtree_update (alpha 0.6); indices, rows and every tree level against the oracle after every round.  The ring
    pointer starts 300 short of the capacity, so it wraps in the second round and the high leaves read the clamped last row."""
    lib, dev, _ = be
    cap, D, R, Ad, B = 100_000, 32, 3, 1, 256
    L = levels_of(cap)
    assert L == 18
    rng = np.random.default_rng(77)
    rows = MAX_ROWS
    rec = records_np(rows, D, R, Ad, True, seed=5)
    rec_d = th.tensor(rec).to(dev)
    tree_o = orc.SumTree(cap)
    tree_d = th.zeros(2 ** L - 1, dtype=th.float64, device=dev)
    minp, ptr = 1e-5, cap - 300
    rmax_d = th.tensor([minp], dtype=th.float64, device=dev)
    for rnd in range(3):
        ptrs = (ptr + np.arange(200)) % cap
        ptr = int((ptr + 200) % cap)
        for p in ptrs:
            tree_o.set(int(p), minp)
        ops.sumtree_set(lib, tree_d, L, th.tensor(ptrs, dtype=th.int64).to(dev), None, rmax_d)
        assert_tree(tree_d, tree_o, (rnd, "set"))
        u = rng.random(B)
        u[:3] = [0.0, 1.0, np.nextafter(1.0, 0.0)]
        want = tree_o.sample_from_uniforms(u)
        u_d = th.tensor(u).to(dev)
        out = ops.sample_gather(lib, rec_d, B, D, R, Ad, True, tree=tree_d, n_levels=L, u01_ptr=u_d.data_ptr())
        assert np.array_equal(out[5].cpu().numpy(), want), (rnd, "idx")
        assert want.max() >= rows or rnd > 0         # (the first round samples only leaves beyond the record store)
        check_batch(out, rec, np.clip(want, 0, rows - 1), D, R, Ad, True, (rnd, "rows"))
        raw = (rng.random(B) * 2).astype(np.float32)
        pr_o = (raw + np.float32(minp)) ** np.float32(ALPHA)
        pr_d = th.empty(B, dtype=th.float64, device=dev)
        ops.sumtree_update(lib, tree_d, L, out[5], th.tensor(raw).to(dev), ALPHA, rmax_d, pr_d)
        pr_dev = pr_d.cpu().numpy()
        np.testing.assert_allclose(pr_dev, pr_o.astype(np.float64), rtol=POW_RTOL)
        pr32 = pr_dev.astype(np.float32)
        assert np.array_equal(pr32.astype(np.float64), pr_dev)
        minp = max(minp, float(pr32.max()))
        assert float(rmax_d.cpu()[0]) == minp
        tree_o.batch_set(want, pr32)
        assert_tree(tree_d, tree_o, (rnd, "update"))
