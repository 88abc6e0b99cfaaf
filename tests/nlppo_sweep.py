"""TEST INFRASTRUCTURE: seeded cases of the NL-MO-PPO shape sweep (tests/test_nlppo_shape_sweep.py) and their float64 evaluation.

Nothing here is recorded: a case is built from its seed the way ``tests/golden/make_golden_nlppo.py::synthetic_rollout`` builds the
fixtures (a seeded ``no.Agent``, a perturbed copy as the behaviour policy, rewards = old values + noise), and the value a kernel is
held to is ``tests/nlppo_oracle.py`` in ``torch.float64`` on the CPU.  The fixture tests pin that file to the reference bit for bit.

A builder asserts what makes its case worth running (no row within ``MARGIN`` of a clip boundary, clip fractions, objectives that
disagree on the active branch); a case that misses a condition fails.

Tolerances are the contract of ``test_nlppo_kernels_parity.py`` with ``ppo_sweep.Report``'s rule for the absolute terms: the
larger of the contract's value and 4 x the largest deviation of the float32 oracle (the same code in float32) from the float64
one for that quantity in that case -- measured on the oracle alone, never on a kernel."""
from __future__ import annotations

import copy
import functools
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import torch as th

import nlppo_cases as nc
import nlppo_common as nm
import nlppo_oracle as no
from ppo_sweep import Report, tensor_bounds  # noqa: F401

MARGIN = 1e-4


@dataclass(frozen=True)
class Case:
    name: str
    obs: int
    A: int
    R: int
    pref_dim: int
    hidden: Tuple[int, ...]
    N: int                     # rows of the rollout table
    M: int                     # rows of the minibatch: a shuffled choice of the N
    seed: int
    perturb: float
    with_pref: bool = True
    clip_vloss: bool = True
    norm_adv: bool = True
    ent_coef: float = 0.01
    lr: float = 2.5e-4
    clip_coef: float = 0.2
    vf_coef: float = 0.5
    max_grad_norm: float = 0.5
    negative_weight: bool = False
    spread: Optional[float] = None     # the actor head's biases run from 0 down to -spread: every row's logits spread that far
    moments: bool = False              # also run from synthetic moments at Adam step 5

    @property
    def D_in(self):
        return self.obs + self.R + self.pref_dim

    def cfg(self):
        return no.Cfg(self.clip_coef, self.ent_coef, self.vf_coef, self.clip_vloss, self.max_grad_norm, self.norm_adv)


STEP_CASES = [
    Case("din128_a32_r8_h128_96_m129", 112, 32, 8, 8, (128, 96), N=160, M=129, seed=501, perturb=0.036, moments=True),
    Case("din128_a2_r1_h32_m17", 126, 2, 1, 1, (32,), N=40, M=17, seed=502, perturb=0.09, moments=True),
    Case("din128_a32_r1_nopref_h32_m15", 127, 32, 1, 0, (32,), N=40, M=15, seed=503, perturb=0.06),
    Case("din128_a2_r8_h128_96_m2", 112, 2, 8, 8, (128, 96), N=20, M=2, seed=504, perturb=0.16, with_pref=False),
    Case("a4_r3_m129_raw_adv", 5, 4, 3, 3, (64, 64), N=200, M=129, seed=505, perturb=0.08, clip_vloss=False, norm_adv=False,
         negative_weight=True, moments=True),
    Case("a32_r8_nopref_m15", 20, 32, 8, 0, (128, 96), N=30, M=15, seed=506, perturb=0.05),
    Case("a6_r2_spread60_m40", 7, 6, 2, 2, (64, 64), N=60, M=40, seed=507, perturb=0.05, spread=60.0, moments=True),
]
STEP_BY_NAME = {c.name: c for c in STEP_CASES}


def seeded_agent(c: Case):
    nc.reseed(c.seed)
    net = no.Agent(c.obs, c.A, c.R, c.pref_dim, c.hidden)
    if c.spread is not None:
        with th.no_grad():      # three likely actions, the others down to -spread
            bias = th.linspace(0.0, -c.spread, c.A)
            bias[:3] = th.tensor([0.0, -0.3, -0.8])
            net.actor[-1].bias.copy_(bias)
    return net


@functools.lru_cache(maxsize=None)
def step_inputs(c: Case):
    """The case's float32 inputs, with the builder's conditions asserted in float64."""
    with nm.one_thread():
        net = seeded_agent(c)
        g, gp = th.Generator().manual_seed(c.seed + 1000), th.Generator().manual_seed(c.seed + 1001)
        old = copy.deepcopy(net)
        with th.no_grad():
            for p in old.parameters():
                p.add_(c.perturb * th.randn(p.shape, generator=gp))
        pref = (th.rand(c.R, generator=g) if (c.with_pref and c.pref_dim) else None)
        obs, acc = th.randn(c.N, c.obs, generator=g), 0.5 * th.randn(c.N, c.R, generator=g)
        with th.no_grad():
            logp = th.log_softmax(old.logits(obs, acc, pref), dim=-1)
            actions = th.multinomial(logp.exp(), 1, generator=g).reshape(-1)
            if c.spread is not None:
                actions[::13] = c.A - 1          # a few rows took the action whose probability is e^-spread
            _, logprobs, _, values = old.get_action_and_value(obs, acc, action=actions, pref=pref)
        rewards = values + th.randn(c.N, c.R, generator=g)
        weights = th.rand(c.R, generator=g) + 0.2
        if c.negative_weight:
            weights[1] = -weights[1]
        idx = th.randperm(c.N, generator=g)[:c.M].clone()
        # old log-probs and old values are inputs: a row within MARGIN of a clip boundary is moved off it
        net64 = no.to_dtype(net, th.float64)
        p64 = None if pref is None else pref.double()
        with th.no_grad():
            _, nlp, _, nv = net64.get_action_and_value(obs.double()[idx], acc.double()[idx], action=actions[idx], pref=p64)
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
        assert not bad_r.any() and not bad_v.any(), c.name
        rclip = float(((ratio - 1.0).abs() > c.clip_coef).double().mean())
        if c.M > 2:
            assert 0.1 <= rclip <= 0.9, f"{c.name}: {rclip:.2f} of the rows have the ratio clipped"
        if c.spread is not None:
            with th.no_grad():
                z = net64.logits(obs.double()[idx], acc.double()[idx], p64)
            assert float((z.max(1).values - z.min(1).values).min()) >= c.spread - 1.0, c.name
        return dict(net=net, obs=obs, acc_rewards=acc, actions=actions, logprobs=logprobs, values=values, rewards=rewards, pref=pref,
                    weights=weights, idx=idx.numpy().astype(np.int64), p0=no.flat_np(net), rclip=rclip)


def as_fixture(inp):
    """The dict ``nlppo_common.Ctx.set_batch`` takes."""
    g = {k: inp[k].numpy() for k in ("obs", "acc_rewards", "logprobs", "values", "rewards")}
    g["actions"] = inp["actions"].numpy().astype(np.int32)
    if inp["pref"] is not None:
        g["pref"] = inp["pref"].numpy()
    return g


@functools.lru_cache(maxsize=None)
def step_oracle(c: Case, dtype, moments: bool):
    """One minibatch step of ``nlppo_oracle`` in ``dtype`` from the case's float32 inputs, as float64 numpy."""
    inp = step_inputs(c)
    with nm.one_thread():
        net = no.to_dtype(inp["net"], dtype)
        opt = th.optim.Adam(net.parameters(), lr=c.lr, eps=1e-5)
        if moments:
            no.set_adam_state(opt, net, *nc.synthetic_moments(c.seed, len(inp["p0"])), 5)
        t = {k: inp[k].to(dtype) for k in ("obs", "acc_rewards", "logprobs", "values", "rewards", "weights")}
        N, R = c.N, c.R
        z = lambda *s: th.zeros(*s, dtype=dtype)  # noqa: E731
        adv, ret = no.compute_advantages(t["rewards"].view(N, 1, R), z(N, 1), t["values"].view(N, 1, R), z(1, R), z(1), 0.0, 0.0)
        batch = (t["obs"], t["acc_rewards"], inp["actions"], t["logprobs"], adv.view(N, R), ret.view(N, R), t["values"],
                 None if inp["pref"] is None else inp["pref"].to(dtype))
        stats, rows = no.minibatch_step(net, opt, c.cfg(), batch, t["weights"], inp["idx"])
        m1, v1 = no.adam_flat(opt, net)
    f = lambda a: np.asarray(a, dtype=np.float64)  # noqa: E731
    inside = ((rows["ratio"] >= 1 - c.clip_coef) & (rows["ratio"] <= 1 + c.clip_coef))[:, None]
    active = inside | (rows["pg1"] > rows["pg2"])
    return dict(stats=f([float(s) for s in stats]), adv=f(adv.view(N, R).numpy()), ret=f(ret.view(N, R).numpy()), p1=f(no.flat_np(net)),
                m1=f(m1), v1=f(v1), disagree=float((active.any(1) & ~active.all(1)).double().mean()))


def report_stats(rep: Report, got, want, o32, weights, prefix=""):
    atol = nm.stat_atol(weights)
    for i, name in enumerate(nm.STATS):
        if name == "clipfrac":
            assert got[i] == np.float32(want[i]), (rep.tag, prefix, name, got[i], want[i])
        else:
            rep.close(prefix + name, got[i], want[i], o32[i], 1e-5, atol.get(name))


# ---------------------------------------------------------------------------------------------------------------------
# forward
# ---------------------------------------------------------------------------------------------------------------------
FORWARD_CASES = [dict(obs=112, A=32, R=8, pref_dim=8, hidden=(128, 96), seed=601), dict(obs=126, A=2, R=1, pref_dim=1, hidden=(32,), seed=602),
                 dict(obs=1, A=2, R=1, pref_dim=0, hidden=(32,), seed=603)]
FORWARD_ROWS = (1, 15, 16, 17, 33)


@functools.lru_cache(maxsize=None)
def forward_case(i):
    f = FORWARD_CASES[i]
    with nm.one_thread():
        nc.reseed(f["seed"])
        net = no.Agent(f["obs"], f["A"], f["R"], f["pref_dim"], f["hidden"])
        g = th.Generator().manual_seed(f["seed"] + 1)
        with th.no_grad():     # (the actor's head is initialised with gain 0.01: perturbed, its logits are not all near zero)
            for p in net.parameters():
                p.add_(0.05 * th.randn(p.shape, generator=g))
        rows = max(FORWARD_ROWS)
        obs, acc = th.randn(rows, f["obs"], generator=g), th.randn(rows, f["R"], generator=g)
        pref = th.rand(f["R"], generator=g) if f["pref_dim"] else None
        out = {}
        for dtype in (th.float64, th.float32):
            n = no.to_dtype(net, dtype)
            p = None if pref is None else pref.to(dtype)
            with th.no_grad():
                logp = th.log_softmax(n.logits(obs.to(dtype), acc.to(dtype), p), dim=-1)
                value = n.get_value(obs.to(dtype), acc.to(dtype), p)
            out[dtype] = (logp.double().numpy(), value.double().numpy())
    return dict(p0=no.flat_np(net), obs_rows=obs.numpy(), acc=acc.numpy(), pref=None if pref is None else pref.numpy(),
                want=out[th.float64], o32=out[th.float32], **f)


# ---------------------------------------------------------------------------------------------------------------------
# GAE
# ---------------------------------------------------------------------------------------------------------------------
# (T, E, R, gamma, gae_lambda, done rate)
GAE_CASES = [(1, 1, 1, 0.99, 0.95, 0.1), (2, 63, 8, 1.0, 1.0, 0.5), (33, 65, 3, 0.995, 0.0, 0.1), (7, 130, 8, 0.9, 0.95, 1.0)]


@functools.lru_cache(maxsize=None)
def gae_inputs(T, E, R, done_rate):
    g = th.Generator().manual_seed(7100 + 131 * T + E)
    out = dict(rewards=th.randn(T, E, R, generator=g), values=th.randn(T, E, R, generator=g),
               dones=(th.rand(T, E, generator=g) < done_rate).float(), next_value=th.randn(E, R, generator=g),
               next_done=(th.rand(E, generator=g) < 0.5).float())
    return out


# ---------------------------------------------------------------------------------------------------------------------
# one context, many calls
# ---------------------------------------------------------------------------------------------------------------------
REUSE_NET = dict(obs=9, A=5, R=2, pref_dim=2, hidden=(64, 64))


@functools.lru_cache(maxsize=None)
def reuse_rollout(seed, T, E):
    """A rollout (``seed``) of one agent's behaviour policy for the bit-exact comparisons of a reused context with a fresh one."""
    n = REUSE_NET
    with nm.one_thread():
        nc.reseed(400)
        net = no.Agent(n["obs"], n["A"], n["R"], n["pref_dim"], n["hidden"])
        g = th.Generator().manual_seed(seed)
        rows = T * E
        obs, acc, pref = th.randn(rows, n["obs"], generator=g), th.randn(rows, n["R"], generator=g), th.rand(n["R"], generator=g)
        with th.no_grad():
            logp = th.log_softmax(net.logits(obs, acc, pref), dim=-1) + 0.1 * th.randn(rows, n["A"], generator=g)
            actions = th.multinomial(th.softmax(logp, -1), 1, generator=g).reshape(-1)
            logprobs = th.log_softmax(logp, -1).gather(1, actions[:, None]).squeeze(1)
            values = net.get_value(obs, acc, pref) + 0.1 * th.randn(rows, n["R"], generator=g)
        out = dict(obs=obs, acc_rewards=acc, actions=actions.int(), logprobs=logprobs, values=values, pref=pref,
                   rewards=th.randn(rows, n["R"], generator=g), dones=(th.rand(rows, generator=g) < 0.1).float(),
                   next_value=th.randn(E, n["R"], generator=g), next_done=(th.rand(E, generator=g) < 0.5).float(),
                   weights=th.tensor([0.9, -0.4]), perm=th.randperm(rows, generator=g))
    out = {k: v.numpy() for k, v in out.items()}
    out.update(p0=no.flat_np(net), T=T, E=E)
    return out


RAGGED = dict(base_seed=701, T=19, E=2, obs=6, A=3, R=3, pref_dim=3, hidden=(64, 32), num_minibatches=4, update_epochs=2, lr=3e-4,
              gamma=0.99, gae_lambda=0.95, perturb=0.05)


def ragged_update(net, opt, cfg, rng, batch, weights, num_minibatches, update_epochs, observer):
    """``no.update`` for a batch that ``num_minibatches`` does not divide (the shorter minibatch at the end of every epoch cannot be
    stacked with the others): the same loop over ``no.minibatch_step``; idx comes back as a list."""
    batch_size = batch[0].shape[0]
    minibatch_size = int(batch_size // num_minibatches)
    b_inds = np.arange(batch_size)
    stats, idx = [], []
    for _ in range(update_epochs):
        rng.shuffle(b_inds)
        for start in range(0, batch_size, minibatch_size):
            mb = b_inds[start:start + minibatch_size]
            s, rows = no.minibatch_step(net, opt, cfg, batch, weights, mb)
            stats.append([float(x) for x in s])
            idx.append(mb.astype(np.int32))
            observer(rows, mb)
    return np.asarray(stats, dtype=np.float64), idx


def ragged_attempt(seed):
    G = RAGGED
    T, E, R = G["T"], G["E"], G["R"]
    nc.reseed(seed)
    net = no.Agent(G["obs"], G["A"], R, G["pref_dim"], G["hidden"])
    g, gp = th.Generator().manual_seed(seed + 1000), th.Generator().manual_seed(seed + 1001)
    old = copy.deepcopy(net)
    with th.no_grad():
        for p in old.parameters():
            p.add_(G["perturb"] * th.randn(p.shape, generator=gp))
    rows = T * E
    obs, acc, pref = th.randn(rows, G["obs"], generator=g), 0.5 * th.randn(rows, R, generator=g), th.rand(R, generator=g)
    with th.no_grad():
        actions = th.multinomial(th.softmax(old.logits(obs, acc, pref), -1), 1, generator=g).reshape(-1)
        _, logprobs, _, values = old.get_action_and_value(obs, acc, action=actions, pref=pref)
    inp = dict(obs=obs, acc_rewards=acc, logprobs=logprobs, values=values, rewards=th.randn(rows, R, generator=g),
               dones=(th.rand(rows, generator=g) < 0.1).float(), next_value=th.randn(E, R, generator=g),
               next_done=(th.rand(E, generator=g) < 0.5).float(), weights=th.rand(R, generator=g) + 0.2, pref=pref)
    cfg, res, worst = no.Cfg(), {}, np.inf
    for dtype in (th.float64, th.float32):
        t = {k: v.to(dtype) for k, v in inp.items()}
        n = no.to_dtype(net, dtype)
        opt = th.optim.Adam(n.parameters(), lr=G["lr"], eps=1e-5)
        adv, ret = no.compute_advantages(t["rewards"].view(T, E, R), t["dones"].view(T, E), t["values"].view(T, E, R), t["next_value"],
                                         t["next_done"], G["gamma"], G["gae_lambda"])
        batch = (t["obs"], t["acc_rewards"], actions, t["logprobs"], adv.reshape(rows, R), ret.reshape(rows, R), t["values"], t["pref"])
        seen = []

        def observer(r, mb):
            ratio, dv = r["ratio"].double(), (r["newvalue"] - batch[6][mb]).double()
            seen.append(float(min((ratio - 0.8).abs().min(), (ratio - 1.2).abs().min(), (dv.abs() - 0.2).abs().min())))

        stats, idx = ragged_update(n, opt, cfg, np.random.default_rng(seed), batch, t["weights"], G["num_minibatches"], G["update_epochs"],
                                   observer)
        worst = min(worst, min(seen))
        res[dtype] = dict(stats=stats, idx=idx, p1=no.flat_np(n).astype(np.float64), ret=ret.reshape(rows, R).double().numpy(),
                          adv=adv.reshape(rows, R).double().numpy())
    assert [len(i) for i in res[th.float64]["idx"]] == [9, 9, 9, 9, 2] * 2
    inp_np = {k: v.numpy() for k, v in inp.items()}
    inp_np["actions"] = actions.numpy().astype(np.int32)
    return worst, dict(inp=inp_np, p0=no.flat_np(net), want=res[th.float64], o32=res[th.float32], seed=seed, margin=worst)


@functools.lru_cache(maxsize=None)
def ragged_case():
    """38 rows in 4 minibatches: 9, 9, 9, 9, 2 per epoch.  The builder walks seeds upward from the base seed and takes the first
    whose every step, in float32 and in float64, keeps MARGIN from every clip boundary."""
    with nm.one_thread():
        for seed in range(RAGGED["base_seed"], RAGGED["base_seed"] + 32):
            worst, case = ragged_attempt(seed)
            if worst >= MARGIN:
                return case
    raise AssertionError("ragged epoch: no seed of 32 keeps every step 1e-4 away from a clip boundary")
