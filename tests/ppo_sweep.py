"""TEST INFRASTRUCTURE: seeded cases of the MO-PPO shape sweep (tests/test_ppo_shape_sweep.py) and their float64 evaluation.

Nothing here is recorded: a case is built from its seed the way ``tests/golden/make_golden_ppo.py::synthetic_rollout`` builds the
fixtures (a seeded ``po.Net``, a perturbed copy as the behaviour policy, returns = old values + noise), and the value a kernel is
held to is ``tests/ppo_oracle.py`` in ``torch.float64`` on the CPU.  The fixture tests pin that file to the reference bit for bit.

A builder asserts what makes its case worth running (``MARGIN``, clip fractions, which side of ``max_grad_norm`` the gradient norm
lies on); a case that misses a condition fails.

Absolute terms.  The project's tolerances are a relative term plus, for some quantities, a fixed absolute one.  The large shapes
sum up to 128 products per output and 300 rows per statistic, so the absolute term of a quantity is the larger of the project's
value and ``FLOOR`` = 4 x the largest deviation of the float32 oracle (the same code in float32) from the float64 one for that
quantity in that case: kernel and torch differ in summation order and libm only, so their errors share one distribution.  The
floor is measured on the oracle alone, never on a kernel."""
from __future__ import annotations

import copy
import functools
from dataclasses import dataclass
from typing import Tuple

import numpy as np
import torch as th

import ppo_cases as pc
import ppo_common as pm
import ppo_oracle as po

MARGIN = 1e-4          # make_golden_ppo.MARGIN: no row this close to a clip boundary
FLOOR = 4.0
ATOL = 1e-6            # test_ppo_kernels_parity.ATOL
STAT_ATOL = {"loss": ATOL, "pg_loss": ATOL, "old_approx_kl": ATOL, "approx_kl": ATOL}


@dataclass(frozen=True)
class Case:
    name: str
    D: int
    A: int
    R: int
    hidden: Tuple[int, ...]
    N: int                     # rows of the rollout table
    M: int                     # rows of the minibatch: a shuffled choice of the N
    seed: int
    perturb: float             # size of the parameter perturbation the old log-probs / old values come from
    clip_vloss: bool = True
    norm_adv: bool = True
    ent_coef: float = 0.0
    lr: float = 3e-4
    clip_coef: float = 0.2
    vf_coef: float = 0.5
    max_grad_norm: float = 0.5
    logstd: float = 0.0
    dup: bool = False          # idx[1] = idx[-1] = idx[0]
    moments: bool = False      # also run from pc.synthetic_moments at Adam step 5

    @property
    def tiles(self):
        return (self.M + 15) // 16

    @property
    def clip_active(self):
        return self.max_grad_norm < 1e8

    def cfg(self):
        return po.Cfg(self.clip_coef, self.ent_coef, self.vf_coef, self.clip_vloss, self.max_grad_norm, self.norm_adv)

    def kwargs(self):
        return dict(clip_coef=self.clip_coef, ent_coef=self.ent_coef, vf_coef=self.vf_coef, max_grad_norm=self.max_grad_norm,
                    clip_vloss=self.clip_vloss, norm_adv=self.norm_adv)


# tiles: the last workgroup adds the partials of tiles 1 .. tiles - 1 four at a time, then one at a time
STEP_CASES = [
    # every declared limit at once; 4 unrolled groups + 2; the normalisation loops' second pass
    Case("limits_m300", 128, 32, 8, (128, 128), N=400, M=300, seed=101, perturb=0.015, moments=True),
    Case("t5_m65_h32", 7, 2, 1, (32,), N=100, M=65, seed=102, perturb=0.08, clip_vloss=False, moments=True),   # one group, no remainder
    Case("t9_d1_h96_64", 1, 1, 1, (96, 64), N=200, M=129, seed=123, perturb=0.1, ent_coef=0.01),
    Case("t17_d33_h64_128", 33, 5, 3, (64, 128), N=300, M=257, seed=104, perturb=0.03, moments=True),          # K chunk of one column
    Case("t6_d127_h96", 127, 17, 8, (96,), N=90, M=81, seed=105, perturb=0.02),                                # group + 1
    Case("t7_h128", 20, 4, 2, (128,), N=120, M=97, seed=106, perturb=0.05, norm_adv=False),                    # group + 2
    Case("t8_h32_128_all", 9, 3, 2, (32, 128), N=128, M=128, seed=107, perturb=0.05, moments=True),            # group + 3, M = N
    # (with the log-prob's 31 terms summed in float this case's old_approx_kl was 1.47e-6 off on the GPU, 1.37e-6 allowed)
    Case("t3_a31_dup", 31, 31, 7, (128, 32), N=64, M=48, seed=108, perturb=0.03, dup=True),
    Case("m2", 4, 2, 2, (32, 32), N=40, M=2, seed=109, perturb=0.15),
    Case("m1", 4, 2, 2, (32, 32), N=40, M=1, seed=110, perturb=0.15, norm_adv=False),
    Case("t2_m17_unclipped", 12, 6, 4, (64, 64), N=80, M=17, seed=111, perturb=0.1, logstd=1.5, max_grad_norm=1e9),
]
STEP_BY_NAME = {c.name: c for c in STEP_CASES}


SENTINEL = -12345.0       # what guard rows behind an output hold: a kernel that writes past the rows it was given changes them


class Ctx(pm.Ctx):
    """``ppo_common.Ctx`` with sentinel rows behind the outputs and a ``morl_ppo_gae`` call without output copies."""

    def guarded(self, rows, cols, guard_rows):
        """A zeroed [rows][cols] output followed by ``guard_rows`` rows of SENTINEL ([rows] when ``cols`` is None)."""
        shape = (rows + guard_rows,) if cols is None else (rows + guard_rows, cols)
        t = th.zeros(shape, dtype=th.float32, device=self.dev)
        t[rows:] = SENTINEL
        return t

    @staticmethod
    def unguard(name, t, rows):
        a = t.cpu().numpy()
        assert (a[rows:] == np.float32(SENTINEL)).all(), f"{name}: written behind its {rows} rows"
        return a[:rows]

    def gae_into_the_table_only(self, next_value, next_done, weights, gamma, gae_lambda, use_gae=True):
        """``morl_ppo_gae`` with NULL for ``returns_out`` and ``advantages_out``."""
        nv, nd, w = self.T(next_value, (-1, self.R)), self.T(next_done, (-1,)), self.T(weights, (self.R,))
        self.lib.check(self.lib.lib.morl_ppo_gae(self.h, nv.data_ptr(), nd.data_ptr(), w.data_ptr(), float(gamma), float(gae_lambda),
                                                 int(use_gae), None, None, self.lib.stream_of(nv)))
        if self.dev.type == "cuda":      # (the arguments of a call that returns nothing to read back must outlive its kernel)
            th.cuda.synchronize()

    def update_n(self, idx, lr, clip_coef=0.2, ent_coef=0.0, vf_coef=0.5, max_grad_norm=0.5, clip_vloss=True, norm_adv=True,
                 guard_rows=0):
        """idx [n][M]; the steps' statistics [n][8] as numpy, with ``guard_rows`` sentinel rows behind them asserted untouched."""
        idx = np.ascontiguousarray(idx, dtype=np.int32).reshape(-1, np.asarray(idx).shape[-1])
        n, M = idx.shape
        idx_d = th.tensor(idx).to(self.dev)
        stats = self.guarded(n, 8, guard_rows)
        self.lib.check(self.lib.lib.morl_ppo_update_n(self.h, self.params.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), n,
                                                      idx_d.data_ptr(), M, float(lr), self.steps_done, float(clip_coef),
                                                      float(ent_coef), float(vf_coef), float(max_grad_norm), int(clip_vloss),
                                                      int(norm_adv), stats.data_ptr(), self.lib.stream_of(stats)))
        self.steps_done += n
        return self.unguard("stats_out", stats, n)

    def forward(self, obs, eps=None, value_only=False, guard_rows=0):
        """(action [rows][A], logprob [rows], value [rows][R]) as numpy; ``value_only``: (None, None, value) with the actor's
        outputs passed as NULL.  ``guard_rows`` sentinel rows follow each output and are asserted untouched."""
        o = self.T(obs, (-1, self.D))
        rows = o.shape[0]
        val = self.guarded(rows, self.R, guard_rows)
        if value_only:
            self.lib.check(self.lib.lib.morl_ppo_forward(self.h, self.params.data_ptr(), o.data_ptr(), None, rows, 1, None, None,
                                                         val.data_ptr(), self.lib.stream_of(val)))
            return None, None, self.unguard("value_out", val, rows)
        e = self.T(eps, (rows, self.A))
        act, lp = self.guarded(rows, self.A, guard_rows), self.guarded(rows, None, guard_rows)
        self.lib.check(self.lib.lib.morl_ppo_forward(self.h, self.params.data_ptr(), o.data_ptr(), e.data_ptr(), rows, 0,
                                                     act.data_ptr(), lp.data_ptr(), val.data_ptr(), self.lib.stream_of(val)))
        return self.unguard("action_out", act, rows), self.unguard("logprob_out", lp, rows), self.unguard("value_out", val, rows)


def oracle_update(net, opt, cfg, np_random, batch, num_minibatches, update_epochs, observer=None):
    """``po.update()`` for a batch that ``num_minibatches`` does not divide: ``po.update`` stacks the minibatches' indices into one
    array, which the shorter minibatch at the end of every epoch does not allow.  The same loop over ``po.minibatch_step``
    (``ragged_case`` asserts that on a batch that divides it gives the bits of ``po.update``); idx comes back as a list."""
    batch_size = batch[0].shape[0]
    minibatch_size = int(batch_size // num_minibatches)
    b_inds = np.arange(batch_size)
    stats, idx = [], []
    for _ in range(update_epochs):
        np_random.shuffle(b_inds)
        for start in range(0, batch_size, minibatch_size):
            mb_inds = b_inds[start:start + minibatch_size]
            s, ratio, newvalue = po.minibatch_step(net, opt, cfg, *batch, mb_inds)
            stats.append([float(x) for x in s])
            idx.append(mb_inds.astype(np.int32))
            if observer is not None:
                observer(ratio, newvalue, mb_inds)
    return np.asarray(stats, dtype=np.float32), idx


def seeded_net(seed, D, A, R, hidden, logstd=0.0):
    pc.reseed(seed)
    net = po.Net(D, A, R, list(hidden))
    with th.no_grad():
        net.actor_logstd.fill_(logstd)
    return net


def behaviour_rows(net, seed, rows, perturb):
    """obs, and actions / log-probs / values of a perturbed copy of ``net`` (the behaviour policy); the generator to go on with."""
    D, A = net.obs_shape[0], net.action_shape[0]
    g, gp = th.Generator().manual_seed(seed + 1000), th.Generator().manual_seed(seed + 1001)
    old = copy.deepcopy(net)
    with th.no_grad():
        for p in old.parameters():
            p.add_(perturb * th.randn(p.shape, generator=gp))
        obs = th.randn(rows, D, generator=g)
        actions = old.actor_mean(obs) + th.exp(old.actor_logstd) * th.randn(rows, A, generator=g)
        _, logprobs, _, values = old.get_action_and_value(obs, actions)
    return obs, actions, logprobs, values, g


def random_weights(R, g):
    w = th.rand(R, generator=g) + 0.1
    return w / w.sum()


def tensor_bounds(net):
    """[start, end) of every parameter tensor in the flat vector, in ``parameters()`` order, with its name."""
    out, o = [], 0
    for name, p in net.named_parameters():
        out.append((name, o, o + p.numel()))
        o += p.numel()
    return out


def clip_margin(clip_coef, ratio, dv, clip_vloss):
    """How close any row comes to a clip boundary (make_golden_ppo.margins)."""
    r = ratio.double().numpy()
    m = min(np.abs(r - (1 - clip_coef)).min(), np.abs(r - (1 + clip_coef)).min())
    if clip_vloss:
        m = min(m, np.abs(np.abs(dv.double().numpy()) - clip_coef).min())
    return float(m)


def one_env_advantages(returns, values, weights):
    """What ``Ctx.set_batch`` puts into the table: a rollout of N steps of one env with gamma = 0 and no GAE."""
    N, R = returns.shape
    z = lambda *s: th.zeros(*s, dtype=returns.dtype)  # noqa: E731
    ret, adv = po.compute_advantages(returns.view(N, 1, R), z(N, 1), values.view(N, 1, R), z(1, R), z(1), weights, 0.0, 0.0, False)
    assert th.equal(ret.view(N, R), returns)
    return adv.reshape(-1)


@functools.lru_cache(maxsize=None)
def step_inputs(c: Case):
    """The case's float32 inputs (a dict of tensors and the net), with the builder's conditions asserted in float64."""
    with pm.one_thread():
        net = seeded_net(c.seed, c.D, c.A, c.R, c.hidden, c.logstd)
        obs, actions, logprobs, values, g = behaviour_rows(net, c.seed, c.N, c.perturb)
        returns = values + th.randn(c.N, c.R, generator=g)
        weights = random_weights(c.R, g)
        idx = th.randperm(c.N, generator=g)[:c.M].clone()
        if c.dup:
            idx[1] = idx[-1] = idx[0]
        # old log-probs and old values are inputs: a row within MARGIN of a clip boundary is moved off it
        net64 = po.to_dtype(net, th.float64)
        with th.no_grad():
            _, nlp, _, nv = net64.get_action_and_value(obs.double()[idx], actions.double()[idx])
        nv = nv.view(c.M, c.R)
        for _ in range(100):
            ratio = (nlp - logprobs.double()[idx]).exp()
            dv = nv - values.double()[idx]
            bad_r = ((ratio - (1 - c.clip_coef)).abs() < MARGIN) | ((ratio - (1 + c.clip_coef)).abs() < MARGIN)
            bad_v = ((dv.abs() - c.clip_coef).abs() < MARGIN) if c.clip_vloss else th.zeros_like(dv, dtype=th.bool)
            if not bad_r.any() and not bad_v.any():
                break
            logprobs[idx[bad_r]] += 0.01
            rows, cols = bad_v.nonzero(as_tuple=True)
            values[idx[rows], cols] += 1e-3
        margin = clip_margin(c.clip_coef, ratio, dv, c.clip_vloss)
        assert margin >= MARGIN, f"{c.name}: a row lies {margin:.2e} from a clip boundary"
        rclip = float(((ratio - 1.0).abs() > c.clip_coef).double().mean())
        vclip = float((dv.abs() > c.clip_coef).double().mean())
        if c.clip_active and c.M > 2:
            assert 0.1 <= rclip <= 0.9, f"{c.name}: {rclip:.2f} of the rows have the ratio clipped"
            assert not c.clip_vloss or 0.1 <= vclip <= 0.9, f"{c.name}: {vclip:.2f} of the values are clipped"
        p0 = po.flat_np(net)
        return dict(net=net, obs=obs, actions=actions, logprobs=logprobs, values=values, returns=returns, weights=weights,
                    idx=idx.numpy().astype(np.int64), p0=p0, rclip=rclip, vclip=vclip, margin=margin)


@functools.lru_cache(maxsize=None)
def step_oracle(c: Case, dtype, moments: bool):
    """One minibatch step of ``ppo_oracle`` in ``dtype`` from the case's float32 inputs: statistics, advantages, parameters and
    moments after the step, as float64 numpy.  ``moments``: from pc.synthetic_moments at Adam step 5, else from zero state."""
    inp = step_inputs(c)
    with pm.one_thread():
        net = po.to_dtype(inp["net"], dtype)
        opt = th.optim.Adam(net.parameters(), lr=c.lr, eps=1e-5)
        if moments:
            m0, v0 = pc.synthetic_moments(c.seed, len(inp["p0"]))
            po.set_adam_state(opt, net, m0, v0, 5)
        t = {k: inp[k].to(dtype) for k in ("obs", "actions", "logprobs", "values", "returns", "weights")}
        adv = one_env_advantages(t["returns"], t["values"], t["weights"])
        stats, _, _ = po.minibatch_step(net, opt, c.cfg(), t["obs"], t["actions"], t["logprobs"], adv, t["returns"], t["values"],
                                        inp["idx"])
        m1, v1 = po.adam_flat(opt, net)
    f = lambda a: np.asarray(a, dtype=np.float64)  # noqa: E731
    out = dict(stats=f([float(s) for s in stats]), adv=f(adv.numpy()), p1=f(po.flat_np(net)), m1=f(m1), v1=f(v1))
    if dtype == th.float64:
        gn = out["stats"][7]
        assert (gn > c.max_grad_norm) == c.clip_active, f"{c.name}: gradient norm {gn} against max_grad_norm {c.max_grad_norm}"
    return out


class Report:
    """Compares quantities of one case with the float64 oracle, prints kernel error, float32-oracle error and what is allowed,
    and keeps the worst error-to-allowance ratio."""

    def __init__(self, tag):
        self.tag, self.worst, self.where, self.floored, self.failed = tag, 0.0, "", [], []

    def close(self, name, got, want, o32, rtol, atol=None):
        """|got - want| <= rtol |want| + max(atol, FLOOR * max |o32 - want|); ``atol=None``: the quantity has no absolute term."""
        got, want, o32 = (np.asarray(a, dtype=np.float64).reshape(-1) for a in (got, want, o32))
        assert got.shape == want.shape == o32.shape, (name, got.shape, want.shape, o32.shape)
        err, dev = np.abs(got - want), float(np.abs(o32 - want).max())
        a = 0.0
        if atol is not None:
            a = max(atol, FLOOR * dev)
            if FLOOR * dev > atol:
                self.floored.append(name)
        tol = a + rtol * np.abs(want)
        ratio = np.where(tol > 0, err / np.where(tol > 0, tol, 1.0), np.where(err > 0, np.inf, 0.0))
        i = int(np.argmax(ratio))
        print(f"{self.tag} {name}: kernel |diff| {err[i]:.3e}, float32 oracle max |diff| {dev:.3e}, allowed {tol[i]:.3e} "
              f"(ratio {ratio[i]:.3f}{', floor' if atol is not None and FLOOR * dev > atol else ''})")
        if ratio[i] > self.worst:
            self.worst, self.where = float(ratio[i]), name
        if not ratio[i] <= 1.0:
            self.failed.append(f"{name}: |diff| {err[i]:.3e} > {tol[i]:.3e}")

    def stats(self, got, want, o32, prefix=""):
        for i, name in enumerate(pm.STATS):
            if name == "clipfrac":
                assert got[i] == np.float32(want[i]), (self.tag, prefix, name, got[i], want[i])
            else:
                self.close(prefix + name, got[i], want[i], o32[i], 1e-5, STAT_ATOL.get(name))

    def per_tensor(self, name, bounds, got, want, o32, rtol, rel_atol):
        for tname, lo, hi in bounds:
            self.close(f"{name}[{tname}]", got[lo:hi], want[lo:hi], o32[lo:hi], rtol, rel_atol * float(np.abs(want[lo:hi]).max()))

    def finish(self):
        print(f"SWEEP {self.tag}: worst error / allowed {self.worst:.3f} ({self.where}); 4 x float32-oracle floor decided: "
              f"{', '.join(self.floored) if self.floored else 'none'}")
        assert not self.failed, (self.tag, self.failed)


# ---------------------------------------------------------------------------------------------------------------------
# GAE / discounted returns
# ---------------------------------------------------------------------------------------------------------------------
# (T, E, R, gamma, gae_lambda, done rate)
GAE_CASES = [(1, 1, 1, 0.99, 0.95, 0.1), (2, 63, 8, 1.0, 1.0, 0.5), (33, 65, 3, 0.995, 0.0, 0.1), (7, 130, 8, 0.9, 0.95, 1.0),
             (16, 64, 5, 0.99, 0.95, 0.0)]
GAE_NET = dict(D=3, A=2, hidden=(32,))


@functools.lru_cache(maxsize=None)
def gae_inputs(T, E, R, done_rate):
    """A rollout of a small net's behaviour policy with random rewards, dones, ``next_done`` and non-uniform weights."""
    seed = 7000 + 131 * T + E
    with pm.one_thread():
        net = seeded_net(seed, GAE_NET["D"], GAE_NET["A"], R, GAE_NET["hidden"])
        obs, actions, logprobs, values, g = behaviour_rows(net, seed, T * E, 0.1)
        rewards = th.randn(T * E, R, generator=g)
        dones = (th.rand(T * E, generator=g) < done_rate).float()
        next_value = th.randn(E, R, generator=g)
        next_done = (th.rand(E, generator=g) < 0.5).float()
        weights = random_weights(R, g)
        M = min(T * E, 40)
        idx = th.randperm(T * E, generator=g)[:M].numpy().astype(np.int64)
    if done_rate in (0.0, 1.0):
        assert (dones == done_rate).all()
    return dict(net=net, obs=obs, actions=actions, logprobs=logprobs, values=values, rewards=rewards, dones=dones,
                next_value=next_value, next_done=next_done, weights=weights, idx=idx, p0=po.flat_np(net))


def gae_oracle(inp, T, E, R, gamma, gae_lambda, use_gae, dtype=th.float64):
    t = {k: inp[k].to(dtype) for k in ("rewards", "dones", "values", "next_value", "next_done", "weights")}
    ret, adv = po.compute_advantages(t["rewards"].view(T, E, R), t["dones"].view(T, E), t["values"].view(T, E, R), t["next_value"],
                                     t["next_done"], t["weights"], gamma, gae_lambda, use_gae)
    return ret.reshape(T * E, R), adv.reshape(-1)


def gae_step_losses(inp, ret, adv, dtype):
    """(pg_loss, v_loss) of a ``norm_adv=False``, ``clip_vloss=False`` step on ``inp['idx']``: continuous in the table's
    advantages and returns, so they read both back."""
    net = po.to_dtype(inp["net"], dtype)
    cfg = po.Cfg(clip_vloss=False, norm_adv=False)
    t = {k: inp[k].to(dtype) for k in ("obs", "actions", "logprobs", "values")}
    with th.no_grad():
        stats, _, _ = po.minibatch_step(net, None, cfg, t["obs"], t["actions"], t["logprobs"], adv.to(dtype), ret.to(dtype),
                                        t["values"], inp["idx"], apply=False)
    return float(stats[1]), float(stats[2])


# ---------------------------------------------------------------------------------------------------------------------
# forward
# ---------------------------------------------------------------------------------------------------------------------
FORWARD_CASES = [dict(D=128, A=32, R=8, hidden=(128, 96), logstd=-2.0, seed=201), dict(D=1, A=1, R=1, hidden=(32,), logstd=0.0, seed=202)]
FORWARD_ROWS = (1, 15, 16, 17, 33)


@functools.lru_cache(maxsize=None)
def forward_case(i):
    """Parameters, 33 observations and noise rows, and (action, log-prob, value) of the oracle in float64 and float32."""
    f = FORWARD_CASES[i]
    with pm.one_thread():
        net = seeded_net(f["seed"], f["D"], f["A"], f["R"], f["hidden"], f["logstd"])
        g = th.Generator().manual_seed(f["seed"] + 1)
        with th.no_grad():     # (the actor's head is initialised with gain 0.01: perturbed, its means are not all near zero)
            for p in net.parameters():
                p.add_(0.05 * th.randn(p.shape, generator=g))
        obs, eps = th.randn(max(FORWARD_ROWS), f["D"], generator=g), th.randn(max(FORWARD_ROWS), f["A"], generator=g)
        out = {}
        for dtype in (th.float64, th.float32):
            n = po.to_dtype(net, dtype)
            with th.no_grad():
                action = n.actor_mean(obs.to(dtype)) + th.exp(n.actor_logstd) * eps.to(dtype)
                _, lp, _, value = n.get_action_and_value(obs.to(dtype), action)
            out[dtype] = tuple(a.double().numpy() for a in (action, lp, value))
    return dict(p0=po.flat_np(net), obs=obs.numpy(), eps=eps.numpy(), want=out[th.float64], o32=out[th.float32], **f)


# ---------------------------------------------------------------------------------------------------------------------
# one context, many calls
# ---------------------------------------------------------------------------------------------------------------------
REUSE_NET = dict(D=9, A=3, R=2, hidden=(64, 64))


@functools.lru_cache(maxsize=None)
def reuse_rollout(seed, T, E):
    """A rollout (``seed``) of one net's behaviour policy for the bit-exact comparisons of a reused context with a fresh one."""
    n = REUSE_NET
    with pm.one_thread():
        net = seeded_net(400, n["D"], n["A"], n["R"], n["hidden"])
        obs, actions, logprobs, values, g = behaviour_rows(net, seed, T * E, 0.05)
        rewards = th.randn(T * E, n["R"], generator=g)
        dones = (th.rand(T * E, generator=g) < 0.1).float()
        out = dict(obs=obs, actions=actions, logprobs=logprobs, values=values, rewards=rewards, dones=dones,
                   next_value=th.randn(E, n["R"], generator=g), next_done=(th.rand(E, generator=g) < 0.5).float(),
                   weights=random_weights(n["R"], g), perm=th.randperm(T * E, generator=g))
    out = {k: v.numpy() for k, v in out.items()}
    out.update(p0=po.flat_np(net), T=T, E=E)
    return out


RAGGED = dict(base_seed=301, T=19, E=2, D=6, A=2, R=3, hidden=(64, 32), num_minibatches=4, update_epochs=2, lr=3e-4, gamma=0.995,
              gae_lambda=0.95, perturb=0.05)


def ragged_attempt(seed):
    G = RAGGED
    T, E, R = G["T"], G["E"], G["R"]
    net = seeded_net(seed, G["D"], G["A"], R, G["hidden"])
    obs, actions, logprobs, values, g = behaviour_rows(net, seed, T * E, G["perturb"])
    inp = dict(obs=obs, actions=actions, logprobs=logprobs, values=values, rewards=th.randn(T * E, R, generator=g),
               dones=(th.rand(T * E, generator=g) < 0.1).float(), next_value=th.randn(E, R, generator=g),
               next_done=(th.rand(E, generator=g) < 0.5).float(), weights=random_weights(R, g))
    cfg, res, worst = po.Cfg(), {}, np.inf
    for dtype in (th.float64, th.float32):
        t = {k: v.to(dtype) for k, v in inp.items()}
        n = po.to_dtype(net, dtype)
        opt = th.optim.Adam(n.parameters(), lr=G["lr"], eps=1e-5)
        ret, adv = po.compute_advantages(t["rewards"].view(T, E, R), t["dones"].view(T, E), t["values"].view(T, E, R),
                                         t["next_value"], t["next_done"], t["weights"], G["gamma"], G["gae_lambda"], True)
        batch = (t["obs"], t["actions"], t["logprobs"], adv.reshape(-1), ret.reshape(-1, R), t["values"])
        seen = []
        stats, idx = oracle_update(n, opt, cfg, np.random.default_rng(seed), batch, G["num_minibatches"], G["update_epochs"],
                                   observer=lambda ratio, nv, mb: seen.append(clip_margin(cfg.clip_coef, ratio, nv - batch[5][mb], True)))
        worst = min(worst, min(seen))
        res[dtype] = dict(stats=stats.astype(np.float64), idx=idx, p1=po.flat_np(n).astype(np.float64),
                          ret=ret.reshape(-1, R).double().numpy(), adv=adv.reshape(-1).double().numpy())
    assert [len(i) for i in res[th.float64]["idx"]] == [9, 9, 9, 9, 2] * 2
    assert all(np.array_equal(a, b) for a, b in zip(res[th.float64]["idx"], res[th.float32]["idx"]))
    return worst, dict(inp={k: v.numpy() for k, v in inp.items()}, p0=po.flat_np(net), want=res[th.float64], o32=res[th.float32],
                       seed=seed, margin=worst)


def oracle_update_is_po_update():
    """On 36 rows in 4 minibatches, two epochs, ``oracle_update`` and ``po.update`` give the same statistics, indices and
    parameters to the bit."""
    G, out = RAGGED, []
    for fn in (po.update, oracle_update):
        net = seeded_net(G["base_seed"], G["D"], G["A"], G["R"], G["hidden"])
        obs, actions, logprobs, values, g = behaviour_rows(net, G["base_seed"], 36, G["perturb"])
        returns = values + th.randn(36, G["R"], generator=g)
        batch = (obs, actions, logprobs, one_env_advantages(returns, values, random_weights(G["R"], g)), returns, values)
        opt = th.optim.Adam(net.parameters(), lr=G["lr"], eps=1e-5)
        stats, idx = fn(net, opt, po.Cfg(), np.random.default_rng(5), batch, 4, 2)
        out.append((stats, np.stack(idx), po.flat_np(net)))
    assert all(np.array_equal(a, b) for a, b in zip(*out)), "oracle_update differs from po.update on a batch that divides"


@functools.lru_cache(maxsize=None)
def ragged_case():
    """38 rows in 4 minibatches: 9, 9, 9, 9, 2 per epoch.  Nudging inputs cannot keep later steps off a clip boundary, so the
    builder walks seeds upward from the base seed and takes the first whose every step, in float32 and in float64, keeps MARGIN."""
    with pm.one_thread():
        oracle_update_is_po_update()
        for seed in range(RAGGED["base_seed"], RAGGED["base_seed"] + 32):
            worst, case = ragged_attempt(seed)
            if worst >= MARGIN:
                return case
    raise AssertionError("ragged epoch: no seed of 32 keeps every step 1e-4 away from a clip boundary")
