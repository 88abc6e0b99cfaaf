"""Actor-critic update benchmark (the "next" rows of SURVEY.md section 8: C3 CAPQL, M1/M2 MOSAC / MORL-D, G7 GPI-PD
continuous) on one MI355X.  bench.py stays the north-star (Envelope) line the driver runs; this script measures the
widened rows with the same conventions:

    python bench_ac.py --workload capql|mosac|morld|gpipd|gpi|ens|pcn|lcn|ipro|ppo|nlppo|eupg [--pop 64] [--steps K] [--warmup W] [--no-cpu-baseline]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
           bench_ac.py --workload morld --gpus N --pop 64      # the population's learners are independent units: pop / N per
                                                                # GPU, no data-path collective ("replicas only", weak scaling)

One "step" = one gradient update of every learner in the job (``update()`` body of the reference agent; for ``morld``
one pass of ``MORLD.__update_others`` over ``pop`` sub-problem learners, morld.py:423-433), on synthetic transitions
resident in HBM, reference-default shapes (batch 128, net [256, 256], twin critics).  ``value`` = learner-updates/s.
"""
from __future__ import annotations

import argparse
import copy
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import numpy as np
import torch as th

PEAK_FP32_MFMA_TFLOPS = 157.3
RESULT_OUT = sys.stdout

SHAPES = {  # obs dim, action dim, objectives of the environments BASELINE.json names
    "capql": dict(D=17, Ad=6, R=2, env="mo-halfcheetah-v4"),
    "mosac": dict(D=11, Ad=3, R=3, env="mo-hopper-v4"),
    "morld": dict(D=11, Ad=3, R=3, env="mo-hopper-v4"),
    "gpipd": dict(D=11, Ad=3, R=3, env="mo-hopper-v4"),
    "gpi": dict(D=7, Ad=6, R=3, env="mo-minecart-v0 (GPI-PD, discrete: 6 actions)"),
    "ens": dict(D=7, Ad=6, R=3, env="mo-minecart-v0 (GPI-PD Dyna model: one-hot action in, next-obs delta + reward out)"),
    "pcn": dict(D=9, Ad=4, R=2, env="treasure-line (discrete head) / mo-hopper-v4 shapes 11-3-3 (continuous head)"),
    "lcn": dict(D=9, Ad=4, R=3, env="heaps of 500 / 2048 episode returns in 3 / 8 objectives (LCN's selection)"),
    "ipro": dict(D=0, Ad=0, R=4, env="fronts of 22 .. 100 points in 3 / 4 objectives, 33 / 50 lower points (IPRO's compute_hvis)"),
    "ppo": dict(D=17, Ad=6, R=2, env="mo-halfcheetah-v4"),
    "pgmorl": dict(D=17, Ad=6, R=2, env="mo-halfcheetah-v4"),
    "nlppo": dict(D=7, Ad=6, R=3, env="mo-minecart-v0 (NL-MO-PPO, discrete: 6 actions)"),
    "eupg": dict(D=1, Ad=2, R=2, env="fishwood-v0 (EUPG, discrete: 2 actions)"),
}
ARCH = [256, 256]
B = 128


def mlp_macs(dims):
    return sum(a * b for a, b in zip(dims[:-1], dims[1:]))


def update_flop(workload, D, Ad, R, rows, policy_iters, do_policy=True):
    """Algorithmic flop of one learner's update: 2 * MACs per row for a forward, dX backward (all layers but the first,
    plus the first for the actor path) and dW backward; element-wise work not counted."""
    w_in = 0 if workload in ("mosac", "morld") else R
    heads = 1 if workload == "gpipd" else 2
    q = [D + Ad + w_in] + ARCH + [R]
    p = [D + w_in] + ARCH + [heads * Ad]
    fq, fp = mlp_macs(q), mlp_macs(p)
    dxq, dxp = fq - q[0] * q[1], fp - p[0] * p[1]
    macs = fp + 2 * fq                 # a' and the twin target critics
    macs += 2 * (fq + dxq + fq)        # twin critics: forward, dX, dW
    if do_policy:
        per_iter = fp + 2 * fq + 2 * fq + (dxp + fp)      # actor fwd, critics fwd, critics dX (incl. layer 0), actor bwd
        if workload in ("mosac", "morld"):
            per_iter += fp                                  # fresh log-prob for the alpha step
        macs += policy_iters * per_iter
    return 2.0 * macs * rows


def cpu_baseline(workload, shp, pop, budget_s=20.0):
    """The oracle (torch-CPU restatement of the reference update) on this box's host cores, bounded sample."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import ac_oracle as ac

    D, Ad, R = shp["D"], shp["Ad"], shp["R"]
    gen = th.Generator().manual_seed(0)
    rnd = lambda *s: th.randn(*s, generator=gen)  # noqa: E731
    w_in = workload not in ("mosac", "morld")
    qspec = ac.MlpSpec(D + Ad + (R if w_in else 0), tuple(ARCH), R, layer_norm=(workload == "gpipd"),
                       drop_rate=0.01 if workload == "gpipd" else 0.0)
    trunk = ac.MlpSpec(D + (R if w_in else 0), tuple(ARCH))
    heads = 1 if workload == "gpipd" else 2
    q = [ac.init_mlp_params(qspec, gen) for _ in range(2)]
    tq = [ac.clone(n) for n in q]
    pol = ac.init_mlp_params(trunk, gen)
    for _ in range(heads):
        pol += [rnd(Ad, ARCH[-1]) * 0.05, th.zeros(Ad)]
    tpol = ac.clone(pol)
    qs = dict(exp_avg=ac.zeros_like(q[0] + q[1]), exp_avg_sq=ac.zeros_like(q[0] + q[1]))
    ps = dict(exp_avg=ac.zeros_like(pol), exp_avg_sq=ac.zeros_like(pol))
    als = dict(exp_avg=[th.zeros(1)], exp_avg_sq=[th.zeros(1)])
    la = th.zeros(1)
    scale, bias = th.ones(Ad), th.zeros(Ad)
    wv = th.softmax(rnd(B, R), dim=1)
    obs, act, rew, nobs, done = rnd(B, D), th.tanh(rnd(B, Ad)), rnd(B, R), rnd(B, D), (th.rand(B, 1, generator=gen) < 0.05).float()

    def one(step):
        if workload == "capql":
            ac.capql_update(qspec, trunk, q, tq, pol, qs, ps, (obs, act, wv, rew, nobs, done.reshape(-1)), rnd(B, Ad),
                            rnd(B, Ad), scale, bias, gamma=0.99, alpha=0.2, lr=3e-4, tau=0.005, step=step)
        elif workload in ("mosac", "morld"):
            ac.mosac_update(qspec, trunk, q, tq, pol, la, qs, ps, als, (obs, act, rew, nobs, done), wv[0], rnd(B, Ad),
                            [rnd(B, Ad), rnd(B, Ad)], [rnd(B, Ad), rnd(B, Ad)], scale, bias, gamma=0.99, tau=0.005,
                            q_lr=1e-3, policy_lr=3e-4, q_step=step, a_step=2 * step - 1, policy_freq=2, do_policy=True,
                            do_target=True, autotune=True, alpha=float(la.exp()), target_entropy=-float(Ad))
        else:
            rows = 2 * B
            rep = lambda x: x.repeat(2, 1)  # noqa: E731
            keep = lambda: [(th.rand(rows, h, generator=gen) >= 0.01).float() for h in ARCH]  # noqa: E731
            drop = {k: [keep(), keep()] for k in ("target", "q", "q_pi")}
            ac.gpipd_cont_update(qspec, trunk, q, tq, pol, tpol, qs, ps, [rep(obs), rep(act), rep(rew), rep(nobs), rep(done)],
                                 rep(wv), rnd(rows, Ad), drop, scale, bias, gamma=0.99, lr=3e-4, tau=0.005, q_step=step,
                                 p_step=step, do_policy=True, n_per=B)

    # these nets are small: torch's default (all cores) is far from the best thread count -- probe a few and keep the best
    one(1)
    step, best = 2, (None, float("inf"))
    for nt in (1, 4, 16, th.get_num_threads()):
        th.set_num_threads(nt)
        one(step); step += 1
        t0 = time.perf_counter()
        for _ in range(3):
            one(step); step += 1
        dt = (time.perf_counter() - t0) / 3
        if dt < best[1]:
            best = (nt, dt)
    th.set_num_threads(best[0])
    times = []
    t_end = time.perf_counter() + budget_s
    while time.perf_counter() < t_end and len(times) < 300:
        t0 = time.perf_counter()
        one(step)
        times.append(time.perf_counter() - t0)
        step += 1
    med = float(np.median(times))
    return {"value": 1.0 / med, "unit": "learner-updates/s", "cores": best[0], "kind": "port",
            "sample": f"{len(times)} timed single-learner updates of oracle/ac_oracle.py on torch-CPU at the best of 1/4/16/all "
                      f"threads ({best[0]}), median; the reference advances a population of {pop} sequentially, i.e. at this rate"}


def bench_gpi(a):
    """GPI-PD with discrete actions: one ``morl_gpi_update`` (batch 128 doubled to 256 rows, ensemble of 2 conditioned
    Q-nets [256]*4 with LayerNorm + Dropout, envelope target over K = 5 weights) per step."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    from morl_baselines_amd.gpi_engine import GPIEngine

    dev = th.device("cuda", 0)
    shp = SHAPES["gpi"]
    D, A, R, K, rows, arch = shp["D"], shp["Ad"], shp["R"], 5, 2 * B, [256, 256, 256, 256]
    eng = GPIEngine(D, A, R, arch, max_rows=rows, max_support=K, device=dev)
    gen = th.Generator(device=dev).manual_seed(0)
    rnd = lambda *s: th.randn(*s, generator=gen, device=dev)  # noqa: E731
    with th.no_grad():
        eng.q.copy_(rnd(*eng.q.shape) * 0.05)
        for n in range(2):
            v = eng.views(eng.q, n)
            for k in (6, 10, 14):
                v[k].fill_(1.0)
        eng.q_target.copy_(eng.q)
    obs, nobs, rew = rnd(rows, D), rnd(rows, D), rnd(rows, R)
    act = th.randint(0, A, (rows,), generator=gen, device=dev)
    done = (th.rand(rows, generator=gen, device=dev) < 0.05).float()
    w = th.softmax(rnd(rows, R), dim=-1).contiguous()
    sw = th.softmax(rnd(K, R), dim=-1).contiguous()
    st = {"n": 0}

    def step():
        st["n"] += 1
        eng.update(obs=obs, actions=act, rewards=rew, next_obs=nobs, dones=done, w=w, sampled_w=sw, adam_step=st["n"],
                   gpi_pd=True, n_per=B, dropout_seed=st["n"], want=("critic_loss", "gtd_error"))

    for _ in range(a.warmup):
        step()
    th.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        step()
    th.cuda.synchronize()
    wall = time.perf_counter() - t0
    macs = D * 256 + 3 * 256 * 256 + 256 * A * R             # per row and net (the R-input weight embedding not counted)
    flop = 2.0 * macs * 2 * (rows + rows * K + 3 * rows)      # target, envelope target, online forward + dX + dW
    ms = wall * 1e3 / a.steps
    tf = flop / (ms * 1e-3) / 1e12
    out = {"metric": "GPI-PD gradient updates/sec", "value": a.steps / wall, "unit": "updates/s", "n_gpus": 1,
           "steps": a.steps, "warmup": a.warmup, "ms_per_step": ms, "higher_is_better": True, "scaling": "weak",
           "vs_baseline": None, "dtype": "f32", "data": "synthetic",
           "config": {"workload": f"GPIPD.update() body: batch {B} doubled to {rows} rows, 2 conditioned Q-nets {arch} "
                                  f"(LayerNorm, Dropout 0.01), envelope target over {K} weights, PER errors; shapes of "
                                  f"{shp['env']}"},
           "roofline": {"bound": "mfma", "kernel": "gemm_batched / gemm_wave_batched", "achieved": tf,
                        "peak": PEAK_FP32_MFMA_TFLOPS, "unit": "TFLOP/s", "frac": tf / PEAK_FP32_MFMA_TFLOPS, "traffic": None,
                        "note": "algorithmic GEMM flop of the update / wall time (launch-latency-bound workload)"},
           "algorithmic_flop_per_step": flop}
    # the reference's default configuration: prioritised replay, 20 gradient updates per environment step -- ONE library entry
    # (morl_gpi_update_n_per: per iteration tree descent + gather, update, max(|gtd|, min) ** alpha back into the tree)
    from morl_baselines_amd.replay import PrioritizedReplayBuffer
    G = 20
    buf = PrioritizedReplayBuffer((D,), 1, rew_dim=R, max_size=32768, action_dtype=np.int32, device=dev)
    rng = np.random.default_rng(0)
    buf.add_batch(rng.standard_normal((20000, D)).astype(np.float32), rng.integers(0, A, (20000, 1)).astype(np.int32),
                  rng.standard_normal((20000, R)).astype(np.float32), rng.standard_normal((20000, D)).astype(np.float32),
                  (rng.random((20000, 1)) < 0.05).astype(np.float32))
    sc = (th.empty(rows, D, device=dev), th.empty(rows, dtype=th.int32, device=dev), th.empty(rows, R, device=dev),
          th.empty(rows, D, device=dev), th.empty(rows, device=dev))

    def per_step():
        items = []
        for _ in range(G):
            st["n"] += 1
            items.append(dict(obs=sc[0], actions=sc[1], rewards=sc[2], next_obs=sc[3], dones=sc[4], w=w, sampled_w=sw,
                              adam_step=st["n"], gpi_pd=True, n_per=B, dropout_seed=st["n"],
                              want=("critic_loss", "td_error", "gtd_error")))
        eng.update_n_per(items, buffer=buf, u01=np.random.random_sample((G, B)), doubled=True, use_gtd=True, alpha=0.6,
                         min_priority=0.01)

    for _ in range(3):
        per_step()
    th.cuda.synchronize()
    n_loops = max(3, a.steps // G)
    enq, t0 = [], time.perf_counter()
    for _ in range(n_loops):
        t1 = time.perf_counter()
        per_step()
        enq.append(time.perf_counter() - t1)
    th.cuda.synchronize()
    loop_ms = (time.perf_counter() - t0) * 1e3 / n_loops
    out["per_loop"] = {"what": f"GPIPD.update() with per=True: {G} gradient updates per environment step through ONE library "
                               "entry (morl_gpi_update_n_per: per iteration sum-tree descent + gather, update, priorities "
                               "back into the tree); buffer of 20 000 transitions",
                       "ms_per_env_step": loop_ms, "ms_per_update": loop_ms / G,
                       "host_enqueue_ms_per_env_step": float(np.median(enq)) * 1e3, "library_entries_per_env_step": 1}
    if not a.no_cpu_baseline:
        import gpi_oracle as go
        from ac_oracle import clone

        spec = go.GpiSpec(D, R, A, tuple(arch), True, 0.01)
        q = [[p.cpu().clone() for p in eng.views(eng.q, n)] for n in range(2)]
        tq = [clone(n) for n in q]
        flat = [p for n in q for p in n]
        state = dict(exp_avg=[th.zeros_like(p) for p in flat], exp_avg_sq=[th.zeros_like(p) for p in flat])
        batch = [obs.cpu(), act.cpu().float().reshape(-1, 1), rew.cpu(), nobs.cpu(), done.cpu().reshape(-1, 1)]
        g2 = th.Generator().manual_seed(0)
        keep = lambda n_: [[(th.rand(n_, h, generator=g2) >= 0.01).float() for h in arch[1:]] for _ in range(2)]  # noqa: E731
        k, best = 0, (None, float("inf"))
        for nt in (1, 4, 16, th.get_num_threads()):        # small nets: all cores is not the fastest setting
            th.set_num_threads(nt)
            drop = dict(target=keep(rows), env=keep(rows * K), q=keep(rows))
            t1 = time.perf_counter()
            for _ in range(2):
                k += 1
                go.gpi_update(spec, q, tq, state, batch, w.cpu(), sw.cpu(), drop, gamma=0.99, lr=3e-4, step=k,
                              min_priority=0.01, gpi_pd=True, n_per=B)
            dt = (time.perf_counter() - t1) / 2
            if dt < best[1]:
                best = (nt, dt)
        th.set_num_threads(best[0])
        times = []
        t_end = time.perf_counter() + 15.0
        while time.perf_counter() < t_end and len(times) < 100:
            k += 1
            drop = dict(target=keep(rows), env=keep(rows * K), q=keep(rows))
            t1 = time.perf_counter()
            go.gpi_update(spec, q, tq, state, batch, w.cpu(), sw.cpu(), drop, gamma=0.99, lr=3e-4, step=k, min_priority=0.01,
                          gpi_pd=True, n_per=B)
            times.append(time.perf_counter() - t1)
        med = float(np.median(times[1:] or times))
        out["cpu_baseline"] = {"value": 1.0 / med, "unit": "updates/s", "cores": best[0], "kind": "port",
                               "sample": f"{len(times)} timed updates of oracle/gpi_oracle.py on torch-CPU at the best of "
                                         f"1/4/16/all threads ({best[0]}), median"}
        out["speedup_vs_cpu_baseline"] = out["value"] / out["cpu_baseline"]["value"]
    print(json.dumps(out), file=RESULT_OUT, flush=True)


def bench_ens(a):
    """Dyna model of GPI-PD: one optimiser step of ``ProbabilisticEnsemble.fit`` (probabilistic_ensemble.py:248-252) --
    5 members x batch 256, net [256, 256, 256] (gpi_pd.py defaults), Gaussian NLL with bounded log-variance, Adam with
    per-layer weight decay -- per step."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    from morl_baselines_amd.dynamics import DECAYS, ProbabilisticEnsemble

    dev = th.device("cuda", 0)
    shp = SHAPES["ens"]
    E, rows, arch = 5, 256, [256, 256, 256]
    din, dout = shp["D"] + shp["Ad"], shp["D"] + shp["R"]
    th.manual_seed(0)
    ens = ProbabilisticEnsemble(din, dout, ensemble_size=E, arch=arch, device=dev, max_rows=rows)
    ens.decays = list(DECAYS)
    gen = th.Generator(device=dev).manual_seed(0)
    x = th.randn(E, rows, din, generator=gen, device=dev)
    y = th.randn(E, rows, dout, generator=gen, device=dev) * 0.1
    ens.inputs_mu = th.zeros((1, din), device=dev)
    ens.inputs_sigma = th.ones((1, din), device=dev)
    p0 = ens.flat.clone()
    for _ in range(a.warmup):
        ens.train_step(x, y)
    th.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        ens.train_step(x, y)
    th.cuda.synchronize()
    wall = time.perf_counter() - t0
    dims = [din] + arch + [2 * dout]
    macs = sum(i * o for i, o in zip(dims[:-1], dims[1:]))
    flop = 2.0 * macs * E * rows * 3 - 2.0 * dims[0] * dims[1] * E * rows     # forward + dX + dW (no dX for the input layer)
    ms = wall * 1e3 / a.steps
    tf = flop / (ms * 1e-3) / 1e12
    out = {"metric": "dynamics-ensemble optimiser steps/sec", "value": a.steps / wall, "unit": "steps/s", "n_gpus": 1,
           "steps": a.steps, "warmup": a.warmup, "ms_per_step": ms, "higher_is_better": True, "scaling": "weak",
           "vs_baseline": None, "dtype": "f32", "data": "synthetic",
           "config": {"workload": f"ProbabilisticEnsemble.fit() inner step: {E} members x batch {rows}, net {arch}, "
                                  f"in {din} / out 2x{dout}; shapes of {shp['env']}"},
           "roofline": {"bound": "mfma", "kernel": "gemm_batched / gemm_wave_batched", "achieved": tf,
                        "peak": PEAK_FP32_MFMA_TFLOPS, "unit": "TFLOP/s", "frac": tf / PEAK_FP32_MFMA_TFLOPS, "traffic": None,
                        "note": "algorithmic GEMM flop of the step / wall time (launch-latency-bound workload)"},
           "algorithmic_flop_per_step": flop}
    if not a.no_cpu_baseline:
        import ens_oracle as eo

        views = ens._layer_views(p0)
        state = dict(W=[w.transpose(1, 2).contiguous().cpu() for w, _ in views],
                     b=[b.reshape(E, 1, -1).contiguous().cpu() for _, b in views],
                     max_lv=th.ones(1, dout) / 2.0, min_lv=-th.ones(1, dout) * 10.0, mu=th.zeros(1, din),
                     sigma=th.ones(1, din))
        order = [p for pair in zip(state["W"], state["b"]) for p in pair] + [state["max_lv"], state["min_lv"]]
        state["m"], state["v"] = [th.zeros_like(p) for p in order], [th.zeros_like(p) for p in order]
        xc, yc = x.cpu(), y.cpu()
        k, best = 0, (None, float("inf"))
        for nt in (1, 4, 16, th.get_num_threads()):
            th.set_num_threads(nt)
            t1 = time.perf_counter()
            for _ in range(3):
                k += 1
                eo.train_step(state, xc, yc, k)
            dt = (time.perf_counter() - t1) / 3
            if dt < best[1]:
                best = (nt, dt)
        th.set_num_threads(best[0])
        times, t_end = [], time.perf_counter() + 15.0
        while time.perf_counter() < t_end and len(times) < 200:
            k += 1
            t1 = time.perf_counter()
            eo.train_step(state, xc, yc, k)
            times.append(time.perf_counter() - t1)
        med = float(np.median(times[1:] or times))
        out["cpu_baseline"] = {"value": 1.0 / med, "unit": "steps/s", "cores": best[0], "kind": "port",
                               "sample": f"{len(times)} timed steps of oracle/ens_oracle.py::train_step on torch-CPU at the "
                                         f"best of 1/4/16/all threads ({best[0]}), median"}
        out["speedup_vs_cpu_baseline"] = out["value"] / out["cpu_baseline"]["value"]
    print(json.dumps(out), file=RESULT_OUT, flush=True)


def bench_pcn(a):
    """PCN (multi_policy/pcn/pcn.py): the ``num_model_updates = 50`` back-to-back ``update()`` calls of one training iteration
    (pcn.py:458-459) at the reference's defaults -- batch 256, hidden 64 -- as ONE ``morl_pcn_update_n`` call, on the discrete and
    the continuous head; next to it the same 50 updates as eager torch ops on the same GPU (tests/pcn_oracle.py moved to the
    device: index the device table, forward, loss, autograd, ``th.optim.Adam``).  The two legs alternate, ``--steps`` loops per
    timed window, five windows each; the figure is the median window."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import ctypes as C

    import pcn_oracle as po
    from morl_baselines_amd.native import load_library

    lib, dev = load_library(), th.device("cuda", 0)
    n_upd, B, H, lr = 50, 256, 64, 1e-3
    loops = max(1, a.steps)
    heads = {}
    for head, (D, R, A, cont) in (("discrete", (9, 2, 4, False)), ("continuous", (11, 3, 3, True))):
        rng = np.random.default_rng(0)
        aw = A if cont else 1
        rows = 2000                                     # ~100 stored episodes of ~20 transitions (max_buffer_size = 100)
        table = rng.standard_normal((rows, D + aw + R + 1)).astype(np.float32)
        table[:, D:D + aw] = rng.uniform(-1, 1, (rows, aw)) if cont else rng.integers(0, A, (rows, 1))
        table[:, -1] = rng.integers(1, 20, rows)
        idx = rng.integers(0, rows, (n_upd, B)).astype(np.int32)
        scaling = np.linspace(0.1, 0.02, R + 1).astype(np.float32)
        th.manual_seed(0)
        init = po.init_params(D, R, A, H)
        table_d, idx_d, scaling_d = th.tensor(table).to(dev), th.tensor(idx).to(dev), th.tensor(scaling).to(dev)
        idx_l = idx_d.long()

        h = C.c_void_p()
        lib.check(lib.lib.morl_pcn_create(C.byref(h), D, R, A, H, int(cont), B))
        lib.check(lib.lib.morl_pcn_set_table(h, table_d.data_ptr(), rows, lib.stream_of(table_d)))
        flat0 = th.cat([p.reshape(-1) for p in init]).to(dev)
        state = dict(p=flat0.clone(), m=th.zeros_like(flat0), v=th.zeros_like(flat0), steps=0)
        loss_d = th.zeros(n_upd, device=dev)
        pred_d = th.zeros(B, A, device=dev)

        def fused_loop():
            lib.check(lib.lib.morl_pcn_update_n(h, state["p"].data_ptr(), state["m"].data_ptr(), state["v"].data_ptr(),
                                                scaling_d.data_ptr(), n_upd, idx_d.data_ptr(), B, lr, state["steps"],
                                                loss_d.data_ptr(), None, pred_d.data_ptr(), lib.stream_of(loss_d)))
            state["steps"] += n_upd

        learner = po.Learner(init, scaling, cont, lr=lr, device=dev)
        eager_losses = []

        def eager_loop():
            eager_losses.clear()
            for k in range(n_upd):
                rows_k = table_d[idx_l[k]]
                actions = rows_k[:, D:D + aw] if cont else rows_k[:, D].long()
                l, _ = learner.update(rows_k[:, :D], actions, rows_k[:, D + aw:D + aw + R], rows_k[:, -1:])
                eager_losses.append(l)

        # same inputs, same start: the first loop of each leg must agree before anything is timed
        fused_loop()
        eager_loop()
        th.cuda.synchronize()
        dev_loss = float((loss_d - th.stack(eager_losses)).abs().max() / th.stack(eager_losses).abs().max())
        for _ in range(max(1, a.warmup // 10)):
            fused_loop()
            eager_loop()
        th.cuda.synchronize()
        t = {"fused": [], "eager": []}
        for _ in range(5):
            for name, fn, reps in (("fused", fused_loop, loops), ("eager", eager_loop, max(1, loops // 10))):
                th.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(reps):
                    fn()
                th.cuda.synchronize()
                t[name].append((time.perf_counter() - t0) * 1e3 / (reps * n_upd))
        lib.lib.morl_pcn_destroy(h)
        fused, eager = float(np.median(t["fused"])), float(np.median(t["eager"]))
        heads[head] = {"shape": dict(state_dim=D, reward_dim=R, action_dim=A, batch=B, hidden=H, updates_per_loop=n_upd),
                       "fused_ms_per_update": fused, "fused_windows_ms": t["fused"], "eager_torch_ms_per_update": eager,
                       "eager_windows_ms": t["eager"], "eager_over_fused": eager / fused,
                       "first_loop_loss_rel_diff": dev_loss, "loops_per_window": {"fused": loops, "eager": max(1, loops // 10)}}
    d = heads["discrete"]
    out = {"metric": "PCN optimiser updates/sec (one-entry 50-update loop, discrete head)", "value": 1e3 / d["fused_ms_per_update"],
           "unit": "updates/s", "n_gpus": 1, "steps": loops, "warmup": a.warmup, "ms_per_step": d["fused_ms_per_update"],
           "higher_is_better": True, "vs_baseline": None, "dtype": "f32", "data": "synthetic",
           "config": {"workload": "PCN.train() inner loop: 50 x update() at batch 256, hidden 64 (pcn.py:399, 458-459), one "
                                  "morl_pcn_update_n call per loop; comparison: the same updates as eager torch ops on the same GPU"},
           "heads": heads,
           "roofline": {"bound": "latency", "kernel": "pcn_step_kernel", "achieved": None, "peak": None, "unit": None, "frac": None,
                        "traffic": None, "note": "~10 MFLOP and < 1 MB per update: launch- and dependency-latency-bound"}}
    print(json.dumps(out), file=RESULT_OUT, flush=True)


def bench_lcn(a):
    """LCN (multi_policy/lcn/lcn.py): the scoring of ``_nlargest`` (lcn.py:226-252) as ONE ``morl_lcn_select`` launch, at LCN's
    default heap (N = 500, R = 3) and at the kernel's limit (N = 2048, R = 8): timed end to end as ``LCN._select`` uses it
    (upload of the returns and the crowding flags, the launch, one read-back) and as the launch alone; next to it the numpy
    selection of tests/lcn_oracle.py (the reference's lines, crowding distance excluded on both sides) on this machine's host,
    and for scale the 100 ``update()`` calls between two selections (batch 32, hidden 64) as one ``morl_pcn_update_n`` call.
    The legs alternate, ``--steps`` calls per timed window, five windows each; the figure is the median window."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import ctypes as C

    import lcn_cases as lc
    import lcn_oracle as lo
    import pcn_oracle as po
    from morl_baselines_amd.native import load_library

    lib, dev = load_library(), th.device("cuda", 0)
    loops = max(1, a.steps)
    L = lib.lib.morl_lcn_select

    # -- the update loop of one iteration (lcn.py:449-455): 100 updates, batch 32, hidden 64, treasure-line shapes -------------------
    n_upd, Bu, H, lr, (D, R, A) = 100, 32, 64, 1e-2, (9, 2, 4)
    rng = np.random.default_rng(0)
    rows = 10000                                        # ~500 stored episodes of ~20 transitions (max_buffer_size = 500)
    table = rng.standard_normal((rows, D + 1 + R + 1)).astype(np.float32)
    table[:, D] = rng.integers(0, A, rows)
    table[:, -1] = rng.integers(1, 20, rows)
    idx_d = th.tensor(rng.integers(0, rows, (n_upd, Bu)).astype(np.int32)).to(dev)
    table_d = th.tensor(table).to(dev)
    scaling_d = th.tensor(np.linspace(0.1, 0.02, R + 1).astype(np.float32)).to(dev)
    th.manual_seed(0)
    flat0 = th.cat([p.reshape(-1) for p in po.init_params(D, R, A, H)]).to(dev)
    h = C.c_void_p()
    lib.check(lib.lib.morl_pcn_create(C.byref(h), D, R, A, H, 0, Bu))
    lib.check(lib.lib.morl_pcn_set_table(h, table_d.data_ptr(), rows, lib.stream_of(table_d)))
    st = dict(p=flat0.clone(), m=th.zeros_like(flat0), v=th.zeros_like(flat0), steps=0)
    loss_d, ent_d, pred_d = th.zeros(n_upd, device=dev), th.zeros(n_upd, device=dev), th.zeros(Bu, A, device=dev)

    def update_loop():
        lib.check(lib.lib.morl_pcn_update_n(h, st["p"].data_ptr(), st["m"].data_ptr(), st["v"].data_ptr(), scaling_d.data_ptr(), n_upd,
                                            idx_d.data_ptr(), Bu, lr, st["steps"], loss_d.data_ptr(), ent_d.data_ptr(),
                                            pred_d.data_ptr(), lib.stream_of(loss_d)))
        st["steps"] += n_upd
        return loss_d.cpu(), ent_d.cpu()                # train() reads both back every iteration

    shapes = {}
    for tag, (N, Rs, mode, lam) in (("n500_r3", (500, 3, 1, 0.0)), ("n2048_r8", (2048, 8, 1, 0.0)),
                                    ("n500_r3_lambda", (500, 3, 2, 0.5))):
        returns = lc.select_returns(N, Rs, "cont", seed=N + Rs)
        want_l2, want_mask, crowded = lo.score(returns, 0.2, mode, lam)
        ret_d, sma_d = th.tensor(returns).to(dev), th.tensor(crowded).to(dev)
        l2_d, nd_d = th.empty(N, device=dev), th.empty(N, dtype=th.uint8, device=dev)

        def launch_only():
            lib.check(L(ret_d.data_ptr(), N, Rs, mode, lam, sma_d.data_ptr(), l2_d.data_ptr(), nd_d.data_ptr(), lib.stream_of(nd_d)))

        def end_to_end():
            r, s = th.from_numpy(returns).to(dev), th.from_numpy(crowded).to(dev)
            l2, nd = th.empty(N, device=dev), th.empty(N, dtype=th.uint8, device=dev)
            lib.check(L(r.data_ptr(), N, Rs, mode, lam, s.data_ptr(), l2.data_ptr(), nd.data_ptr(), lib.stream_of(nd)))
            out = th.cat((l2.view(th.uint8), nd)).cpu().numpy()
            return out[:4 * N].view(np.float32), out[4 * N:]

        def numpy_leg():
            return lo.score(returns, 0.2, mode, lam, crowded=crowded)

        # same inputs: the device's l2 is numpy's, bit for bit, before anything is timed
        got_l2, got_nd = end_to_end()
        exact = bool(np.array_equal(got_l2.view(np.uint32), want_l2.view(np.uint32)) and np.array_equal(got_nd.astype(bool), want_mask))
        if not exact:
            raise SystemExit(f"bench_ac lcn {tag}: the device selection differs from numpy's")
        for _ in range(max(1, a.warmup)):
            launch_only()
            end_to_end()
        numpy_leg()
        update_loop()
        th.cuda.synchronize()
        t = {"launch": [], "end_to_end": [], "numpy": [], "update_loop": []}
        for _ in range(5):
            for name, fn, reps, sync in (("launch", launch_only, loops, True), ("end_to_end", end_to_end, loops, False),
                                         ("numpy", numpy_leg, max(1, loops // 10), False),
                                         ("update_loop", update_loop, max(1, loops // 10), False)):
                th.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(reps):
                    fn()
                if sync:
                    th.cuda.synchronize()
                t[name].append((time.perf_counter() - t0) * 1e6 / reps)
        med = {k: float(np.median(v)) for k, v in t.items()}
        shapes[tag] = {"shape": dict(N=N, R=Rs, mode=mode, lcn_lambda=lam, front=int(want_mask.sum()), crowded=int(crowded.sum())),
                       "bit_identical_to_numpy": exact,
                       "device_end_to_end_us": med["end_to_end"], "device_launch_only_us": med["launch"],
                       "numpy_host_us": med["numpy"], "numpy_over_device_end_to_end": med["numpy"] / med["end_to_end"],
                       "update_loop_100x_batch32_us": med["update_loop"],
                       "windows_us": t, "calls_per_window": {"launch": loops, "end_to_end": loops, "numpy": max(1, loops // 10),
                                                            "update_loop": max(1, loops // 10)}}
    lib.lib.morl_pcn_destroy(h)
    d = shapes["n500_r3"]
    out = {"metric": "LCN selections/sec (morl_lcn_select end to end: upload, one launch, read-back; N = 500, R = 3)",
           "value": 1e6 / d["device_end_to_end_us"], "unit": "selections/s", "n_gpus": 1, "steps": loops, "warmup": a.warmup,
           "ms_per_step": d["device_end_to_end_us"] / 1e3, "higher_is_better": True, "vs_baseline": None, "dtype": "f32",
           "data": "synthetic",
           "config": {"workload": "LCN._nlargest's scoring (lcn.py:226-252) at the default heap of 500 episodes and at the kernel's "
                                  "limit; comparison: the same lines in numpy on this host (tests/lcn_oracle.py), and the 100-update "
                                  "loop of one training iteration (morl_pcn_update_n, batch 32, hidden 64, losses and entropies read "
                                  "back) for scale"},
           "shapes": shapes,
           "roofline": {"bound": "latency", "kernel": "lcn_select_kernel", "achieved": None, "peak": None, "unit": None, "frac": None,
                        "traffic": None, "note": "one workgroup, N^2 pair tests on LDS broadcasts; the end-to-end call is two "
                                                 "uploads, a launch and a blocking read-back"}}
    print(json.dumps(out), file=RESULT_OUT, flush=True)


def bench_ipro(a):
    """IPRO (multi_policy/ipro/ipro.py): one ``compute_hvis`` (ipro.py:212-226) -- the hypervolume of ``pf`` and ``completed`` plus
    one lower point, for every drawn lower point -- as ONE ``morl_ipro_hvis`` call, timed end to end as ``IPRO.compute_hvis`` uses
    it (one upload of base, candidates and reference, two launches, one read-back) and as the launches alone.  Next to it what the
    package offered for the same scores before: K + 1 ``hypervolume_device`` calls in a loop, each with its upload (with one
    read-back per call, as ``compute_hypervolume`` makes it, and with a single read-back at the end), and the float64 oracle
    (tests/ipro_oracle.py) on this machine's host.  Every device result is checked against the oracle (1e-12) before anything is
    timed.  The legs alternate, ``--steps`` calls per timed window, five windows each; the figure is the median window."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import ipro_oracle as io_
    from morl_baselines_amd import performance_indicators as pi
    from morl_baselines_amd.native import load_library

    lib, dev = load_library(), th.device("cuda", 0)
    loops = max(1, a.steps)
    shapes = {}
    for n, R, K in ((25, 3, 33), (22, 4, 50), (100, 3, 50), (60, 4, 50)):
        tag = f"n{n}_r{R}_k{K}"
        rng = np.random.default_rng(100 * n + R)
        # a run's geometry: the base is a front of mutually non-dominated points, the candidates lie below it, ref is the ideal
        v = np.abs(rng.standard_normal((n + K, R)))
        v = 10.0 * v / np.linalg.norm(v, axis=1, keepdims=True)
        ref = np.full(R, 11.0)
        base, cand = 11.0 - v[:n], 11.0 - 1.3 * v[n:] * rng.uniform(0.6, 1.0, (K, 1))
        want = np.asarray([io_.oracle_hv(np.vstack((base, c)), ref) for c in cand] + [io_.oracle_hv(base, ref)])
        flat_d = th.from_numpy(np.concatenate([base.reshape(-1), cand.reshape(-1), ref])).to(dev)
        base_d, cand_d, ref_d = flat_d[:n * R].view(n, R), flat_d[n * R:(n + K) * R].view(K, R), flat_d[(n + K) * R:]
        sets = [np.concatenate([-np.vstack((base, c)).reshape(-1), -ref]) for c in cand] + [np.concatenate([-base.reshape(-1), -ref])]

        def launch_only():
            return pi.ipro_hvis_device(ref_d, base_d, cand_d, lib)

        def end_to_end():
            return pi.ipro_hvis(ref, base, cand, lib=lib, device=dev)

        def one_hv(flat):
            t = th.from_numpy(flat).to(dev)
            rows = (flat.size - R) // R
            return pi.hypervolume_device(t[rows * R:], t[:rows * R].view(rows, R), lib)

        def loop_sync_each():
            return np.asarray([float(one_hv(f).item()) for f in sets])

        def loop_one_readback():
            return th.stack([one_hv(f) for f in sets]).cpu().numpy()

        def oracle_leg():
            return [io_.oracle_hv(np.vstack((base, c)), ref) for c in cand] + [io_.oracle_hv(base, ref)]

        worst = {}
        for name, got in (("batched", end_to_end()), ("loop", loop_sync_each()), ("loop_one_readback", loop_one_readback())):
            worst[name] = float(np.max(np.abs(got - want) / np.abs(want)))
            if not worst[name] <= 1e-12:
                raise SystemExit(f"bench_ac ipro {tag}: the {name} leg is {worst[name]:.3g} relative off the float64 oracle")
        for _ in range(max(1, a.warmup)):
            launch_only()
            end_to_end()
        loop_sync_each()
        loop_one_readback()
        th.cuda.synchronize()
        legs = (("launch", launch_only, loops, True), ("end_to_end", end_to_end, loops, False),
                ("loop", loop_sync_each, max(1, loops // 10), False), ("loop_one_readback", loop_one_readback, max(1, loops // 10), False),
                ("oracle", oracle_leg, 1, False))
        t = {name: [] for name, *_ in legs}
        for window in range(5):
            for name, fn, reps, sync in legs:
                if name == "oracle" and window >= 2:        # (seconds per call at 60 points in 4 objectives: two windows of one call)
                    continue
                th.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(reps):
                    fn()
                if sync:
                    th.cuda.synchronize()
                t[name].append((time.perf_counter() - t0) * 1e6 / reps)
        med = {k: float(np.median(v)) for k, v in t.items()}
        shapes[tag] = {"shape": dict(n=n, R=R, K=K), "max_rel_error_vs_oracle": worst,
                       "batched_end_to_end_us": med["end_to_end"], "batched_launches_only_us": med["launch"],
                       "loop_of_hypervolume_device_us": med["loop"], "loop_one_readback_us": med["loop_one_readback"],
                       "host_oracle_us": med["oracle"], "loop_over_batched": med["loop"] / med["end_to_end"],
                       "loop_one_readback_over_batched": med["loop_one_readback"] / med["end_to_end"],
                       "host_oracle_over_batched": med["oracle"] / med["end_to_end"], "windows_us": t,
                       "calls_per_window": {name: reps for name, _, reps, _ in legs}}
    d = shapes["n22_r4_k50"]
    out = {"metric": "IPRO compute_hvis calls/sec (morl_ipro_hvis end to end: one upload, two launches, one read-back; n = 22, R = 4, K = 50)",
           "value": 1e6 / d["batched_end_to_end_us"], "unit": "calls/s", "n_gpus": 1, "steps": loops, "warmup": a.warmup,
           "ms_per_step": d["batched_end_to_end_us"] / 1e3, "higher_is_better": True, "vs_baseline": None, "dtype": "f64",
           "data": "synthetic",
           "config": {"workload": "IPRO.compute_hvis (ipro.py:212-226) at the shapes scripted runs reach and at larger fronts; "
                                  "comparison: K + 1 separate hypervolume_device calls (the package before morl_ipro_hvis) and the "
                                  "float64 oracle on this host"},
           "shapes": shapes,
           "roofline": {"bound": "latency", "kernel": "ipro_hvis_kernel", "achieved": None, "peak": None, "unit": None, "frac": None,
                        "traffic": None, "note": "one workgroup per candidate on LDS-staged points; the end-to-end call is one "
                                                 "upload, two launches and a blocking read-back"}}
    print(json.dumps(out), file=RESULT_OUT, flush=True)


def bench_ppo(a):
    """MO-PPO (single_policy/ser/mo_ppo.py): one ``MOPPO.update()`` at PGMORL's defaults -- 4 envs x 2048 steps = 8192 rows,
    10 epochs x 32 minibatches of 256 rows = 320 optimiser steps, net [64, 64], mo-halfcheetah shapes 17-6-2 -- as ONE
    ``morl_ppo_update_n`` call, and the GAE scan over 2048 x 4; next to it the same steps as eager torch ops on the same GPU
    (tests/ppo_oracle.py moved to the device, with the reference's host read of ``clipfrac`` per minibatch).  The two legs
    alternate, ``--steps`` updates per timed window, five windows each; the figure is the median window."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import ctypes as C

    import ppo_oracle as po
    from morl_baselines_amd.native import load_library

    lib, dev = load_library(), th.device("cuda", 0)
    T, E, D, A, R, hidden = 2048, 4, 17, 6, 2, [64, 64]
    epochs, n_mb, lr, gamma, lam = 10, 32, 3e-4, 0.995, 0.95
    rows, M, n_steps = T * E, T * E // n_mb, epochs * n_mb
    loops = max(1, a.steps)
    th.manual_seed(0)
    net = po.Net(D, A, R, hidden)
    g = th.Generator().manual_seed(1)
    old = copy.deepcopy(net)
    with th.no_grad():
        for p in old.parameters():
            p.add_(0.02 * th.randn(p.shape, generator=g))
        obs = th.randn(rows, D, generator=g)
        actions = old.actor_mean(obs) + th.exp(old.actor_logstd) * th.randn(rows, A, generator=g)
        _, logprobs, _, values = old.get_action_and_value(obs, actions)
    rewards = th.randn(rows, R, generator=g)
    dones = (th.rand(rows, generator=g) < 0.001).float()
    next_value, next_done = th.randn(E, R, generator=g), th.zeros(E)
    weights = th.tensor([0.5, 0.5])
    rng = np.random.default_rng(0)
    b_inds, idx = np.arange(rows), []
    for _ in range(epochs):
        rng.shuffle(b_inds)
        idx += [b_inds[s:s + M].copy() for s in range(0, rows, M)]
    idx = np.stack(idx).astype(np.int32)
    to = lambda t: t.to(dev).contiguous()  # noqa: E731
    obs_d, act_d, lp_d, rew_d, done_d, val_d = (to(t) for t in (obs, actions, logprobs, rewards, dones, values))
    nv_d, nd_d, w_d, idx_d = to(next_value), to(next_done), to(weights), th.tensor(idx).to(dev)
    idx_l = idx_d.long()

    h = C.c_void_p()
    lib.check(lib.lib.morl_ppo_create(C.byref(h), D, A, R, 2, hidden[0], hidden[1], M))
    stream = lib.stream_of(obs_d)
    lib.check(lib.lib.morl_ppo_set_rollout(h, obs_d.data_ptr(), act_d.data_ptr(), lp_d.data_ptr(), rew_d.data_ptr(), done_d.data_ptr(),
                                           val_d.data_ptr(), T, E, stream))
    ret_d, adv_d = th.zeros(rows, R, device=dev), th.zeros(rows, device=dev)

    def fused_gae():
        lib.check(lib.lib.morl_ppo_gae(h, nv_d.data_ptr(), nd_d.data_ptr(), w_d.data_ptr(), gamma, lam, 1, ret_d.data_ptr(),
                                       adv_d.data_ptr(), stream))

    def eager_gae():
        return po.compute_advantages(rew_d.view(T, E, R), done_d.view(T, E), val_d.view(T, E, R), nv_d, nd_d, w_d, gamma, lam, True)

    fused_gae()
    e_ret, e_adv = eager_gae()
    th.cuda.synchronize()
    gae_diff = float((adv_d - e_adv.reshape(-1)).abs().max() / e_adv.abs().max())

    flat0 = th.cat([p.detach().reshape(-1) for p in net.parameters()]).to(dev)
    state = dict(p=flat0.clone(), m=th.zeros_like(flat0), v=th.zeros_like(flat0), steps=0)
    stats_d = th.zeros(n_steps, 8, device=dev)

    def fused_update():
        lib.check(lib.lib.morl_ppo_update_n(h, state["p"].data_ptr(), state["m"].data_ptr(), state["v"].data_ptr(), n_steps,
                                            idx_d.data_ptr(), M, lr, state["steps"], 0.2, 0.0, 0.5, 0.5, 1, 1, stats_d.data_ptr(),
                                            stream))
        state["steps"] += n_steps

    e_net = copy.deepcopy(net).to(dev)
    opt = th.optim.Adam(e_net.parameters(), lr=lr, eps=1e-5)
    cfg = po.Cfg()
    batch = (obs_d, act_d, lp_d, e_adv.reshape(-1), e_ret.reshape(-1, R), val_d)
    eager_losses = []

    def eager_update():
        eager_losses.clear()
        clipfracs = []
        for k in range(n_steps):
            s, _, _ = po.minibatch_step(e_net, opt, cfg, *batch, idx_l[k])
            clipfracs.append(s[6].item())            # the reference's host read per minibatch (mo_ppo.py:522)
            eager_losses.append(s[0])

    # same inputs, same start: the first update of each leg must agree before anything is timed
    fused_update()
    eager_update()
    th.cuda.synchronize()
    e_loss = th.stack(eager_losses)
    first = slice(0, n_mb)                           # the first epoch: later steps start from parameters that have drifted apart
    loss_diff = float((stats_d[first, 0] - e_loss[first]).abs().max() / e_loss[first].abs().max())
    for _ in range(max(1, a.warmup // 10)):
        fused_update()
        eager_update()
    th.cuda.synchronize()
    t = {"fused": [], "eager": [], "fused_gae": [], "eager_gae": []}
    for _ in range(5):
        for name, fn, reps, per in (("fused", fused_update, loops, n_steps), ("eager", eager_update, max(1, loops // 10), n_steps),
                                    ("fused_gae", fused_gae, loops, 1), ("eager_gae", eager_gae, 1, 1)):
            th.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            th.cuda.synchronize()
            t[name].append((time.perf_counter() - t0) * 1e3 / (reps * per))
    lib.lib.morl_ppo_destroy(h)
    med = {k: float(np.median(v)) for k, v in t.items()}
    out = {"metric": "MO-PPO optimiser steps/sec (one-entry 320-step update())", "value": 1e3 / med["fused"], "unit": "steps/s",
           "n_gpus": 1, "steps": loops, "warmup": a.warmup, "ms_per_step": med["fused"], "higher_is_better": True, "vs_baseline": None,
           "dtype": "f32", "data": "synthetic",
           "config": {"workload": "MOPPO.update() at PGMORL's defaults: 8192-row rollout (4 envs x 2048 steps), 10 epochs x 32 "
                                  "minibatches of 256, net [64, 64], shapes 17-6-2 (mo-halfcheetah); one morl_ppo_update_n call per "
                                  "update(); comparison: the same steps as eager torch ops on the same GPU"},
           "shape": dict(obs_dim=D, action_dim=A, reward_dim=R, hidden=hidden, rollout_rows=rows, minibatch=M, steps_per_update=n_steps),
           "fused_us_per_step": med["fused"] * 1e3, "eager_torch_us_per_step": med["eager"] * 1e3,
           "eager_over_fused": med["eager"] / med["fused"], "fused_windows_ms": t["fused"], "eager_windows_ms": t["eager"],
           "first_epoch_loss_rel_diff": loss_diff,
           "gae": {"fused_ms": med["fused_gae"], "eager_torch_ms": med["eager_gae"], "eager_over_fused": med["eager_gae"] / med["fused_gae"],
                   "advantage_rel_diff": gae_diff, "fused_windows_ms": t["fused_gae"], "eager_windows_ms": t["eager_gae"]},
           "loops_per_window": {"fused": loops, "eager": max(1, loops // 10)},
           "roofline": {"bound": "latency", "kernel": "ppo_step_kernel", "achieved": None, "peak": None, "unit": None, "frac": None,
                        "traffic": None, "note": "~20 MFLOP and < 1 MB per step: launch- and dependency-latency-bound"}}
    print(json.dumps(out), file=RESULT_OUT, flush=True)


def bench_nlppo(a):
    """NL-MO-PPO (single_policy/ser/nl_mo_ppo.py): one ``NLMOPPO.update()`` at the class defaults -- 4 envs x 128 steps = 512 rows,
    4 epochs x 4 minibatches of 128 rows = 16 optimiser steps, net [64, 64], mo-minecart shapes (obs 7, 6 actions, 3 objectives,
    pref_dim 3) -- as ONE ``morl_nlppo_update_n`` call, and the GAE scan over 128 x 4; next to it the same steps as eager torch ops
    on the same GPU (tests/nlppo_oracle.py moved to the device, with the reference's host read of ``clipfrac`` per minibatch).  The
    loss weights are fixed: ``_compute_loss_weights`` is one forward launch and a host gradient in both legs.  The two legs
    alternate, ``--steps`` updates per timed window, five windows each; the figure is the median window."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import ctypes as C

    import nlppo_oracle as no
    from morl_baselines_amd.native import load_library

    lib, dev = load_library(), th.device("cuda", 0)
    T, E, D, A, R, Pd, hidden = 128, 4, 7, 6, 3, 3, [64, 64]
    epochs, n_mb, lr, gamma, lam = 4, 4, 2.5e-4, 0.99, 0.95
    rows, M, n_steps = T * E, T * E // n_mb, epochs * n_mb
    loops = max(1, a.steps)
    th.manual_seed(0)
    net = no.Agent(D, A, R, Pd, hidden)
    g = th.Generator().manual_seed(1)
    old = copy.deepcopy(net)
    with th.no_grad():
        for p in old.parameters():
            p.add_(0.05 * th.randn(p.shape, generator=g))
        obs, acc, pref = th.randn(rows, D, generator=g), 0.5 * th.randn(rows, R, generator=g), th.rand(R, generator=g)
        actions = th.multinomial(th.softmax(old.logits(obs, acc, pref), -1), 1, generator=g).reshape(-1)
        _, logprobs, _, values = old.get_action_and_value(obs, acc, action=actions, pref=pref)
    rewards = th.randn(rows, R, generator=g)
    dones = (th.rand(rows, generator=g) < 0.01).float()
    next_value, next_done = th.randn(E, R, generator=g), th.zeros(E)
    weights = th.tensor([1.05, 0.035, -0.2])
    rng = np.random.default_rng(0)
    b_inds, idx = np.arange(rows), []
    for _ in range(epochs):
        rng.shuffle(b_inds)
        idx += [b_inds[s:s + M].copy() for s in range(0, rows, M)]
    idx = np.stack(idx).astype(np.int32)
    to = lambda t: t.to(dev).contiguous()  # noqa: E731
    obs_d, acc_d, lp_d, rew_d, done_d, val_d, pref_d = (to(t) for t in (obs, acc, logprobs, rewards, dones, values, pref))
    act_d, act_l = to(actions.int()), to(actions)
    nv_d, nd_d, w_d, idx_d = to(next_value), to(next_done), to(weights), th.tensor(idx).to(dev)
    idx_l = idx_d.long()

    h = C.c_void_p()
    lib.check(lib.lib.morl_nlppo_create(C.byref(h), D, A, R, Pd, 2, hidden[0], hidden[1], M))
    stream = lib.stream_of(obs_d)
    lib.check(lib.lib.morl_nlppo_set_rollout(h, obs_d.data_ptr(), acc_d.data_ptr(), act_d.data_ptr(), lp_d.data_ptr(), rew_d.data_ptr(),
                                             done_d.data_ptr(), val_d.data_ptr(), pref_d.data_ptr(), T, E, stream))
    ret_d, adv_d = th.zeros(rows, R, device=dev), th.zeros(rows, R, device=dev)

    def fused_gae():
        lib.check(lib.lib.morl_nlppo_gae(h, nv_d.data_ptr(), nd_d.data_ptr(), gamma, lam, ret_d.data_ptr(), adv_d.data_ptr(), stream))

    def eager_gae():
        return no.compute_advantages(rew_d.view(T, E, R), done_d.view(T, E), val_d.view(T, E, R), nv_d, nd_d, gamma, lam)

    fused_gae()
    e_adv, e_ret = eager_gae()
    th.cuda.synchronize()
    gae_diff = float((adv_d - e_adv.reshape(rows, R)).abs().max() / e_adv.abs().max())

    flat0 = th.cat([p.detach().reshape(-1) for p in net.parameters()]).to(dev)
    state = dict(p=flat0.clone(), m=th.zeros_like(flat0), v=th.zeros_like(flat0), steps=0)
    stats_d = th.zeros(n_steps, 8, device=dev)

    def fused_update():
        lib.check(lib.lib.morl_nlppo_update_n(h, state["p"].data_ptr(), state["m"].data_ptr(), state["v"].data_ptr(), n_steps,
                                              idx_d.data_ptr(), M, w_d.data_ptr(), lr, state["steps"], 0.2, 0.01, 0.5, 0.5, 1, 1,
                                              stats_d.data_ptr(), stream))
        state["steps"] += n_steps

    e_net = copy.deepcopy(net).to(dev)
    e_net.aug = lambda x, ar, p: th.cat([x, ar, p], dim=-1)      # (the rows, already on the device)
    opt = th.optim.Adam(e_net.parameters(), lr=lr, eps=1e-5)
    cfg = no.Cfg()
    batch = (obs_d, acc_d, act_l, lp_d, e_adv.reshape(rows, R), e_ret.reshape(rows, R), val_d, pref_d)
    eager_losses = []

    def eager_update():
        eager_losses.clear()
        clipfracs = []
        for k in range(n_steps):
            s, _ = no.minibatch_step(e_net, opt, cfg, batch, w_d, idx_l[k])
            clipfracs.append(s[6].item())            # the reference's host read per minibatch (nl_mo_ppo.py:362)
            eager_losses.append(s[0])

    # same inputs, same start: the first update of each leg must agree before anything is timed
    fused_update()
    eager_update()
    th.cuda.synchronize()
    e_loss = th.stack(eager_losses)
    first = slice(0, n_mb)                           # the first epoch: later steps start from parameters that have drifted apart
    loss_diff = float((stats_d[first, 0] - e_loss[first]).abs().max() / e_loss[first].abs().max())
    for _ in range(max(1, a.warmup // 10)):
        fused_update()
        eager_update()
    th.cuda.synchronize()
    t = {"fused": [], "eager": [], "fused_gae": [], "eager_gae": []}
    for _ in range(5):
        for name, fn, reps, per in (("fused", fused_update, loops, n_steps), ("eager", eager_update, max(1, loops // 10), n_steps),
                                    ("fused_gae", fused_gae, loops, 1), ("eager_gae", eager_gae, max(1, loops // 10), 1)):
            th.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            th.cuda.synchronize()
            t[name].append((time.perf_counter() - t0) * 1e3 / (reps * per))
    lib.lib.morl_nlppo_destroy(h)
    med = {k: float(np.median(v)) for k, v in t.items()}
    out = {"metric": "NL-MO-PPO optimiser steps/sec (one-entry 16-step update())", "value": 1e3 / med["fused"], "unit": "steps/s",
           "n_gpus": 1, "steps": loops, "warmup": a.warmup, "ms_per_step": med["fused"], "higher_is_better": True, "vs_baseline": None,
           "dtype": "f32", "data": "synthetic",
           "config": {"workload": "NLMOPPO.update() at the class defaults: 512-row rollout (4 envs x 128 steps), 4 epochs x 4 "
                                  "minibatches of 128, net [64, 64], shapes of mo-minecart (obs 7, 6 actions, 3 objectives, pref_dim 3); "
                                  "one morl_nlppo_update_n call per update(); comparison: the same steps as eager torch ops on the "
                                  "same GPU"},
           "shape": dict(obs_dim=D, n_actions=A, reward_dim=R, pref_dim=Pd, hidden=hidden, rollout_rows=rows, minibatch=M,
                         steps_per_update=n_steps),
           "fused_us_per_step": med["fused"] * 1e3, "eager_torch_us_per_step": med["eager"] * 1e3,
           "eager_over_fused": med["eager"] / med["fused"], "fused_windows_ms": t["fused"], "eager_windows_ms": t["eager"],
           "first_epoch_loss_rel_diff": loss_diff,
           "gae": {"fused_ms": med["fused_gae"], "eager_torch_ms": med["eager_gae"], "eager_over_fused": med["eager_gae"] / med["fused_gae"],
                   "advantage_rel_diff": gae_diff, "fused_windows_ms": t["fused_gae"], "eager_windows_ms": t["eager_gae"]},
           "loops_per_window": {"fused": loops, "eager": max(1, loops // 10)},
           "roofline": {"bound": "latency", "kernel": "nlppo_step_kernel", "achieved": None, "peak": None, "unit": None, "frac": None,
                        "traffic": None, "note": "8 tiles of 16 rows, ~5 MFLOP and < 1 MB per step: launch- and dependency-latency-bound"}}
    print(json.dumps(out), file=RESULT_OUT, flush=True)


def bench_eupg(a):
    """EUPG (single_policy/esr/eupg.py): one ``EUPG.update()`` at the shapes of the reference's example (examples/eupg_fishwood.py:
    obs 1, 2 actions, 2 objectives, net [50], an episode of 200 steps, the example's utility min(fish, wood // 2)) -- the scan
    launch, the utility as torch ops on the device tensor, the step launch; next to it the same update as eager torch ops on the
    same GPU (tests/eupg_oracle.py moved to the device: the reference's 200-iteration scan loop, Categorical, autograd, Adam).  The
    episode is resident on the device in both legs.  The two legs alternate, ``--steps`` updates per timed window (a tenth of that
    for the eager leg), five windows each; the figure is the median window.  The legs' first losses must agree to 1e-5."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import ctypes as C

    import eupg_oracle as eo
    from morl_baselines_amd.native import load_library

    lib, dev = load_library(), th.device("cuda", 0)
    T, D, A, R, hidden, lr, gamma = 200, 1, 2, 2, [50], 1e-3, 0.99
    loops = max(1, a.steps)

    def utility(r, w=None):
        return th.min(r[:, 0], r[:, 1] // 2)

    th.manual_seed(0)
    net = eo.PolicyNet(D, A, R, hidden)
    g = th.Generator().manual_seed(1)
    obs = th.randint(0, 2, (T, D), generator=g).int()                          # fishwood's state: at the river or in the woods
    actions = th.randint(0, A, (T, 1), generator=g).int()
    rewards = (th.rand(T, R, generator=g) < 0.3).float()                        # a fish or a piece of wood now and then
    acc = th.cat([th.zeros(1, R), th.cumsum(rewards, 0)[:-1]])
    to = lambda t: t.to(dev).contiguous()  # noqa: E731
    obs_d, obs_f, acc_d, act_d, rew_d = to(obs), to(obs.float()), to(acc), to(actions), to(rewards)

    h = C.c_void_p()
    lib.check(lib.lib.morl_eupg_create(C.byref(h), D, A, R, 1, hidden[0], 0, T, 0))
    stream = lib.stream_of(obs_d)
    lib.check(lib.lib.morl_eupg_set_episode(h, obs_f.data_ptr(), acc_d.data_ptr(), act_d.data_ptr(), rew_d.data_ptr(), T, stream))
    flat0 = th.cat([p.detach().reshape(-1) for p in net.parameters()]).to(dev)
    state = dict(p=flat0.clone(), m=th.zeros_like(flat0), v=th.zeros_like(flat0), steps=0)
    ret_d, loss_d = th.zeros(T, R, device=dev), th.zeros(1, device=dev)

    def fused_update():
        lib.check(lib.lib.morl_eupg_returns(h, gamma, ret_d.data_ptr(), stream))
        u = utility(ret_d).contiguous()
        lib.check(lib.lib.morl_eupg_update(h, state["p"].data_ptr(), state["m"].data_ptr(), state["v"].data_ptr(), u.data_ptr(), lr,
                                           state["steps"], loss_d.data_ptr(), stream))
        state["steps"] += 1
        state["u"] = u                       # (alive until the launch has read it)

    e_net = copy.deepcopy(net).to(dev)
    opt = th.optim.Adam(e_net.parameters(), lr=lr)
    eager = {}

    def eager_update():
        eager["loss"], eager["G"] = eo.update(e_net, opt, obs_d, acc_d, act_d, rew_d, gamma, utility)[:2]

    # same inputs, same start: the first update of each leg must agree before anything is timed
    fused_update()
    eager_update()
    th.cuda.synchronize()
    loss_diff = float((loss_d[0] - eager["loss"]).abs() / eager["loss"].abs())
    returns_equal = bool(th.equal(ret_d, eager["G"]))
    if not loss_diff <= 1e-5:
        raise RuntimeError(f"eupg: the fused and the eager leg's first losses differ by {loss_diff:.3e} relative (allowed 1e-5)")
    for _ in range(max(1, a.warmup // 10)):
        fused_update()
        eager_update()
    th.cuda.synchronize()
    t = {"fused": [], "eager": []}
    for _ in range(5):
        for name, fn, reps in (("fused", fused_update, loops), ("eager", eager_update, max(1, loops // 10))):
            th.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            th.cuda.synchronize()
            t[name].append((time.perf_counter() - t0) * 1e3 / reps)
    lib.lib.morl_eupg_destroy(h)
    med = {k: float(np.median(v)) for k, v in t.items()}
    out = {"metric": "EUPG updates/sec (one episode of 200 steps per update())", "value": 1e3 / med["fused"], "unit": "updates/s",
           "n_gpus": 1, "steps": loops, "warmup": a.warmup, "ms_per_step": med["fused"], "higher_is_better": True, "vs_baseline": None,
           "dtype": "f32", "data": "synthetic",
           "config": {"workload": "EUPG.update() at the shapes of examples/eupg_fishwood.py: obs 1, 2 actions, 2 objectives, net [50], an "
                                  "episode of 200 steps, utility min(fish, wood // 2); the scan launch, the utility in torch on the "
                                  "device, the step launch; comparison: the same update as eager torch ops on the same GPU"},
           "shape": dict(obs_dim=D, n_actions=A, reward_dim=R, hidden=hidden, episode_rows=T, tiles=(T + 15) // 16),
           "fused_us_per_update": med["fused"] * 1e3, "eager_torch_us_per_update": med["eager"] * 1e3,
           "eager_over_fused": med["eager"] / med["fused"], "fused_windows_ms": t["fused"], "eager_windows_ms": t["eager"],
           "fused_slowest_below_eager_fastest": bool(max(t["fused"]) < min(t["eager"])),
           "first_loss_rel_diff": loss_diff, "returns_bit_equal": returns_equal,
           "loops_per_window": {"fused": loops, "eager": max(1, loops // 10)},
           "roofline": {"bound": "latency", "kernel": "eupg_step_kernel", "achieved": None, "peak": None, "unit": None, "frac": None,
                        "traffic": None, "note": "13 tiles of 16 rows, ~0.1 MFLOP and < 100 KB per update: launch- and dependency-latency-bound"}}
    print(json.dumps(out), file=RESULT_OUT, flush=True)


def bench_pgmorl(a):
    """PGMORL's population (multi_policy/pgmorl/pgmorl.py, ``pop_size`` MOPPO learners) at the ``ppo`` row's shapes: every learner
    has its own parameters, rollout and shuffles.  Three pairs, each timed in the same process in interleaved windows (five per leg,
    the figure is the median window): the 320 minibatch steps of an iteration as ONE ``morl_ppo_update_n_pop`` call against P
    back-to-back ``morl_ppo_update_n`` calls; ``morl_ppo_gae_pop`` against P ``morl_ppo_gae`` calls; one lock-step acting step
    (``morl_ppo_forward_pop`` on 4 rows per learner and one host read) against P ``morl_ppo_forward`` calls with a read each.
    Before anything is timed both legs run one update from the same start and must leave bit-identical parameters."""
    import ctypes as C

    from morl_baselines_amd.mo_ppo import MOPPONet
    from morl_baselines_amd.native import load_library

    lib, dev = load_library(), th.device("cuda", 0)
    P = a.pop or 6
    T, E, D, A, R, hidden = 2048, 4, 17, 6, 2, [64, 64]
    epochs, n_mb, lr, gamma, lam = 10, 32, 3e-4, 0.995, 0.95
    rows, M, n_steps = T * E, T * E // n_mb, epochs * n_mb
    loops = max(1, a.steps)
    ptrs = lambda ts: (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])  # noqa: E731
    th.manual_seed(0)
    g = th.Generator().manual_seed(1)
    rng = np.random.default_rng(0)
    to = lambda t: t.to(dev).contiguous()  # noqa: E731
    p0, roll, idx, nv, nd, w = [], [], [], [], [], []
    for i in range(P):
        net = MOPPONet((D,), (A,), R, hidden)
        p0.append(to(th.cat([p.detach().reshape(-1) for p in net.parameters()])))
        obs, act = th.randn(rows, D, generator=g), th.randn(rows, A, generator=g)
        # (old log-probs near those of a unit-variance policy with a small mean, old values near the critic's: steps of ordinary size)
        logp = -0.5 * (act ** 2).sum(1) - A * 0.9189385 + 0.02 * th.randn(rows, generator=g)
        roll.append([to(t) for t in (obs, act, logp, th.randn(rows, R, generator=g), (th.rand(rows, generator=g) < 0.001).float(),
                                     0.1 * th.randn(rows, R, generator=g))])
        nv.append(to(th.randn(E, R, generator=g)))
        nd.append(to(th.zeros(E)))
        w.append(to(th.tensor([i / max(P - 1, 1), 1.0 - i / max(P - 1, 1)])))
        b_inds, steps = np.arange(rows), []
        for _ in range(epochs):
            rng.shuffle(b_inds)
            steps += [b_inds[s_:s_ + M].copy() for s_ in range(0, rows, M)]
        idx.append(th.tensor(np.stack(steps).astype(np.int32)).to(dev))
    stream = lib.stream_of(p0[0])

    def make_leg():
        hs = []
        for i in range(P):
            h = C.c_void_p()
            lib.check(lib.lib.morl_ppo_create(C.byref(h), D, A, R, 2, hidden[0], hidden[1], M))
            lib.check(lib.lib.morl_ppo_set_rollout(h, *[t.data_ptr() for t in roll[i]], T, E, stream))
            hs.append(h.value)
        return dict(h=hs, p=[t.clone() for t in p0], m=[th.zeros_like(t) for t in p0], v=[th.zeros_like(t) for t in p0], steps=0,
                    stats=[th.zeros(n_steps, 8, device=dev) for _ in range(P)], ret=[th.zeros(rows, R, device=dev) for _ in range(P)],
                    adv=[th.zeros(rows, device=dev) for _ in range(P)])

    pop, seq = make_leg(), make_leg()
    pop_h = (C.c_void_p * P)(*pop["h"])

    def pop_gae():
        lib.check(lib.lib.morl_ppo_gae_pop(P, pop_h, ptrs(nv), ptrs(nd), ptrs(w), gamma, lam, 1, ptrs(pop["ret"]), ptrs(pop["adv"]), stream))

    def seq_gae():
        for i in range(P):
            lib.check(lib.lib.morl_ppo_gae(seq["h"][i], nv[i].data_ptr(), nd[i].data_ptr(), w[i].data_ptr(), gamma, lam, 1,
                                           seq["ret"][i].data_ptr(), seq["adv"][i].data_ptr(), stream))

    def pop_update():
        lib.check(lib.lib.morl_ppo_update_n_pop(P, pop_h, ptrs(pop["p"]), ptrs(pop["m"]), ptrs(pop["v"]), n_steps, ptrs(idx), M,
                                                (C.c_double * P)(*[lr] * P), (C.c_int * P)(*[pop["steps"]] * P), 0.2, 0.0, 0.5, 0.5, 1, 1,
                                                ptrs(pop["stats"]), stream))
        pop["steps"] += n_steps

    def seq_update():
        for i in range(P):
            lib.check(lib.lib.morl_ppo_update_n(seq["h"][i], seq["p"][i].data_ptr(), seq["m"][i].data_ptr(), seq["v"][i].data_ptr(),
                                                n_steps, idx[i].data_ptr(), M, lr, seq["steps"], 0.2, 0.0, 0.5, 0.5, 1, 1,
                                                seq["stats"][i].data_ptr(), stream))
        seq["steps"] += n_steps

    obs_a, eps_a = to(th.randn(P, E, D, generator=g)), to(th.randn(P, E, A, generator=g))
    act_o, lp_o, val_o = th.zeros(P, E, A, device=dev), th.zeros(P, E, device=dev), th.zeros(P, E, R, device=dev)
    each = lambda t: ptrs([t[i] for i in range(P)])  # noqa: E731

    def pop_act():
        lib.check(lib.lib.morl_ppo_forward_pop(P, pop_h, ptrs(pop["p"]), each(obs_a), each(eps_a), E, 0, each(act_o), each(lp_o),
                                               each(val_o), stream))
        return act_o.cpu()

    def seq_act():
        out = []
        for i in range(P):
            lib.check(lib.lib.morl_ppo_forward(seq["h"][i], seq["p"][i].data_ptr(), obs_a[i].data_ptr(), eps_a[i].data_ptr(), E, 0,
                                               act_o[i].data_ptr(), lp_o[i].data_ptr(), val_o[i].data_ptr(), stream))
            out.append(act_o[i].cpu())
        return out

    # same inputs, same start: both legs must leave the same bits before anything is timed
    pop_gae()
    seq_gae()
    pop_update()
    seq_update()
    th.cuda.synchronize()
    same = all(th.equal(x, y) for k in ("p", "m", "v", "stats", "ret", "adv") for x, y in zip(pop[k], seq[k]))
    if not same:
        raise SystemExit("bench_pgmorl: the population call and the sequential calls left different bits")
    finite = all(bool(th.isfinite(s).all()) for s in pop["stats"])
    a_pop, a_seq = pop_act(), seq_act()
    if not all(th.equal(a_pop[i], a_seq[i]) for i in range(P)):
        raise SystemExit("bench_pgmorl: forward_pop and forward gave different actions")
    for _ in range(max(1, a.warmup // 10)):
        pop_update()
        seq_update()
    th.cuda.synchronize()
    t = {k: [] for k in ("pop", "seq", "pop_gae", "seq_gae", "pop_act", "seq_act")}
    for _ in range(5):
        for name, fn, reps, per in (("pop", pop_update, loops, n_steps), ("seq", seq_update, loops, n_steps), ("pop_gae", pop_gae, loops, 1),
                                    ("seq_gae", seq_gae, loops, 1), ("pop_act", pop_act, 20 * loops, 1), ("seq_act", seq_act, 20 * loops, 1)):
            th.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            th.cuda.synchronize()
            t[name].append((time.perf_counter() - t0) * 1e3 / (reps * per))
    th.cuda.synchronize()
    same_after = all(th.equal(x, y) for k in ("p", "m", "v") for x, y in zip(pop[k], seq[k]))
    for h in pop["h"] + seq["h"]:
        lib.lib.morl_ppo_destroy(h)
    med = {k: float(np.median(v)) for k, v in t.items()}
    spread = lambda v: (max(v) - min(v)) / float(np.median(v))  # noqa: E731
    pair = lambda p_, s_: {"population_ms": med[p_], "sequential_ms": med[s_], "sequential_over_population": med[s_] / med[p_],  # noqa: E731
                           "population_windows_ms": t[p_], "sequential_windows_ms": t[s_], "sequential_window_spread": spread(t[s_])}
    out = {"metric": f"PGMORL population minibatch steps/sec ({P} learners per step, one launch)", "value": 1e3 / med["pop"],
           "unit": "population steps/s", "n_gpus": 1, "steps": loops, "warmup": a.warmup, "ms_per_step": med["pop"],
           "higher_is_better": True, "vs_baseline": med["seq"] / med["pop"], "dtype": "f32", "data": "synthetic",
           "config": {"workload": f"PGMORL's {P} MOPPO learners at its defaults: each an 8192-row rollout (4 envs x 2048 steps), 10 epochs x "
                                  "32 minibatches of 256, net [64, 64], shapes 17-6-2 (mo-halfcheetah), own parameters / rollout / "
                                  "shuffles; one morl_ppo_update_n_pop call per iteration; baseline: the same steps as P back-to-back "
                                  "morl_ppo_update_n calls (the parent's way), same process, interleaved windows"},
           "shape": dict(pop=P, obs_dim=D, action_dim=A, reward_dim=R, hidden=hidden, rollout_rows=rows, minibatch=M,
                         steps_per_update=n_steps, workgroups_per_launch=P * ((M + 15) // 16)),
           "update": pair("pop", "seq"), "gae": pair("pop_gae", "seq_gae"), "acting": pair("pop_act", "seq_act"),
           "bit_identical_before_timing": same, "bit_identical_after_timing": same_after, "statistics_finite": finite,
           "loops_per_window": {"update": loops, "gae": loops, "acting": 20 * loops},
           "roofline": {"bound": "latency", "kernel": "ppo_pop_step_kernel", "achieved": None, "peak": None, "unit": None, "frac": None,
                        "traffic": None, "note": "a step is a chain of dependent launches of one tile's latency each; the population "
                                                 "fills idle CUs, it does not shorten the chain"}}
    print(json.dumps(out), file=RESULT_OUT, flush=True)


def _claim_stdout():
    """stdout must carry exactly ONE line, rank 0's JSON: C libraries (RCCL prints a version banner to stdout, flushed
    at exit, i.e. after the JSON) and the other ranks are moved to stderr; the result is written to the saved descriptor."""
    sys.stdout.flush()
    real = os.fdopen(os.dup(1), "w")
    os.dup2(2, 1)
    return real


def bench_morld_contexts(a, D, Ad, R, pop, rows, shp):
    """``MORLD(devices=[...])``'s hot path (``__update_others``, morld.py:423-433) with the population split over ``a.devices`` contexts
    of ONE process: context g holds pop / G learners in its own ACEngine on GPU min(g, visible - 1); a step enqueues every context's
    update (independent learners: no exchange), the step ends when all devices are done."""
    from morl_baselines_amd.ac_engine import ALGO_MOSAC, ACEngine
    G = a.devices
    if pop % G:
        raise SystemExit(f"--pop {pop} must be divisible by --devices {G}")
    visible = th.cuda.device_count()
    devs = [th.device("cuda", min(g, visible - 1)) for g in range(G)]
    iters, ctxs = 2, []
    for g, dev in enumerate(devs):
        n = pop // G
        with th.cuda.device(dev):
            eng = ACEngine(ALGO_MOSAC, D, Ad, R, ARCH, action_low=-1.0, action_high=1.0, max_rows=rows, population=n, device=dev,
                           device_steps=True)
            gen = th.Generator(device=dev).manual_seed(g)
            rnd = lambda *s_, gen=gen, dev=dev: th.randn(*s_, generator=gen, device=dev)  # noqa: E731
            with th.no_grad():
                eng.q.copy_(rnd(*eng.q.shape) * 0.05)
                eng.pol.copy_(rnd(*eng.pol.shape) * 0.05)
                eng.q_target.copy_(eng.q)
            data = dict(obs=rnd(n, rows, D), next_obs=rnd(n, rows, D), actions=th.tanh(rnd(n, rows, Ad)), rewards=rnd(n, rows, R),
                        dones=(th.rand(n, rows, generator=gen, device=dev) < 0.05).float(),
                        w=th.softmax(rnd(n, 1, R), dim=-1).contiguous())
        ctxs.append((dev, eng, data, n))

    def step():
        for dev, eng, data, n in ctxs:
            with th.cuda.device(dev):
                cfg = eng.make_cfg(q_lr=1e-3, policy_iters=iters, autotune=True, target_entropy=-float(Ad))
                eps = th.randn((1 + 2 * iters, n, rows, Ad), dtype=th.float32, device=dev)
                eng.update(cfg, eps_next=eps[0], eps_pi=eps[1:1 + iters], eps_alpha=eps[1 + iters:], want=("critic_loss",), **data)

    sync = lambda: [th.cuda.synchronize(d) for d in set(devs)]  # noqa: E731
    for _ in range(a.warmup):
        step()
    sync()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        step()
    sync()
    wall = time.perf_counter() - t0
    ms = wall * 1e3 / a.steps
    flop = update_flop("morld", D, Ad, R, rows, iters) * pop
    tf = flop / (ms * 1e-3) / 1e12
    distinct = len(set(devs))
    out = {"metric": "actor-critic learner updates/sec", "value": pop * a.steps / wall, "unit": "learner-updates/s",
           "rows_per_s": pop * rows * a.steps / wall, "n_gpus": distinct, "steps": a.steps, "warmup": a.warmup, "ms_per_step": ms,
           "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
           "config": {"workload": f"morld: {pop} learners x batch {B} ({rows} rows), net {ARCH}, shapes of {shp['env']}; one pass of "
                                  f"MORLD.__update_others per step, the population split over {G} device contexts of one process",
                      "population": pop, "contexts": G, "learners_per_context": pop // G, "distinct_gpus": distinct,
                      "parallelism": f"{G} contexts (one ACEngine each) on {distinct} GPU(s); independent learners, no data-path collective",
                      "measured": (f"all {G} contexts on their own GPU" if distinct == G else
                                   f"FUNCTIONAL beyond {distinct} GPU(s): this box shows {visible}, so {G - distinct + 1} contexts share "
                                   "a device -- the multi-GPU figure is UNMEASURED")},
           "roofline": {"bound": "mfma", "kernel": "gemm_batched (exact-fp32 MFMA layers of all nets / learners)", "achieved": tf,
                        "peak": PEAK_FP32_MFMA_TFLOPS * distinct, "unit": "TFLOP/s", "frac": tf / (PEAK_FP32_MFMA_TFLOPS * distinct),
                        "traffic": None},
           "algorithmic_flop_per_step": flop}
    print(json.dumps(out), file=RESULT_OUT, flush=True)


def main():
    global RESULT_OUT
    RESULT_OUT = _claim_stdout()
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="morld", choices=sorted(SHAPES))
    ap.add_argument("--pop", type=int, default=None)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--gemm-mode", type=int, default=0, help="0 auto, 1 LDS tiles, 2 wave tiles (morl_ac_set_gemm_mode)")
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--devices", type=int, default=1,
                    help="morld in ONE process: the population split over this many device contexts (MORLD(devices=[...]): pop / N "
                         "learners per ACEngine, one context per visible GPU -- all on cuda:0 when the box has fewer, and the record "
                         "says how many distinct GPUs it really used)")
    ap.add_argument("--force-dp", action="store_true",
                    help="capql on ONE rank through the data-parallel path (gradient hook + RCCL all-reduce with itself)")
    a = ap.parse_args()
    if not th.cuda.is_available():
        raise SystemExit("bench_ac.py needs an MI355X (no CPU fallback exists)")
    rank, local_rank, world = (int(os.environ.get(k, d)) for k, d in (("RANK", 0), ("LOCAL_RANK", 0), ("WORLD_SIZE", 1)))
    if a.gpus != world:
        raise SystemExit(f"--gpus {a.gpus} needs torch.distributed.run with --nproc-per-node {a.gpus}")
    dev = th.device("cuda", local_rank)
    th.cuda.set_device(dev)
    dist = None
    if world > 1 or a.force_dp:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
        if world > 1 and a.workload not in ("morld", "capql"):
            raise SystemExit("--gpus N: the MORL/D population shards as independent learners (no collective); CAPQL runs "
                             "data-parallel (gradient all-reduce inside the update)")
    if a.workload == "gpi":
        return bench_gpi(a)
    if a.workload == "ens":
        return bench_ens(a)
    if a.workload == "pcn":
        return bench_pcn(a)
    if a.workload == "lcn":
        return bench_lcn(a)
    if a.workload == "ipro":
        return bench_ipro(a)
    if a.workload == "ppo":
        return bench_ppo(a)
    if a.workload == "nlppo":
        return bench_nlppo(a)
    if a.workload == "eupg":
        return bench_eupg(a)
    if a.workload == "pgmorl":
        return bench_pgmorl(a)
    from morl_baselines_amd.ac_engine import ALGO_CAPQL, ALGO_MOSAC, ALGO_TD3, ACEngine

    wl, shp = a.workload, SHAPES[a.workload]
    D, Ad, R = shp["D"], shp["Ad"], shp["R"]
    pop = a.pop if a.pop is not None else (64 if wl == "morld" else 1)
    pop_total = pop
    dp = (world > 1 or a.force_dp) and wl == "capql"         # data-parallel: every rank B rows of the job's world * B batch, grads averaged
    if world > 1 and not dp:
        if pop % world:
            raise SystemExit(f"--pop {pop} must be divisible by the number of GPUs")
        pop = pop // world                       # this rank's learners
    algo = {"capql": ALGO_CAPQL, "mosac": ALGO_MOSAC, "morld": ALGO_MOSAC, "gpipd": ALGO_TD3}[wl]
    rows = 2 * B if wl == "gpipd" else B
    if a.devices > 1:
        if wl != "morld" or world > 1:
            raise SystemExit("--devices N is the single-process MORL/D population over N device contexts")
        return bench_morld_contexts(a, D, Ad, R, pop, rows, shp)
    eng = ACEngine(algo, D, Ad, R, ARCH, action_low=-1.0, action_high=1.0, max_rows=rows, population=pop, device=dev,
                   q_layer_norm=(wl == "gpipd"), q_drop_rate=(0.01 if wl == "gpipd" else 0.0), device_steps=True)
    eng.lib.check(eng.lib.lib.morl_ac_set_gemm_mode(a.gemm_mode))
    gen = th.Generator(device=dev).manual_seed(0)
    rnd = lambda *s: th.randn(*s, generator=gen, device=dev)  # noqa: E731
    with th.no_grad():                          # orthogonal-ish scale; the values do not matter for timing
        eng.q.copy_(rnd(*eng.q.shape) * 0.05)
        eng.pol.copy_(rnd(*eng.pol.shape) * 0.05)
        if eng.layer_norm:
            for p_ in range(pop):
                for n in range(2):
                    v = eng.q_views(eng.q, p_, n)
                    for k in (2, 6):
                        v[k].fill_(1.0)
        eng.q_target.copy_(eng.q)
        if eng.pol_target is not None:
            eng.pol_target.copy_(eng.pol)
    obs, nobs = rnd(pop, rows, D), rnd(pop, rows, D)
    act, rew = th.tanh(rnd(pop, rows, Ad)), rnd(pop, rows, R)
    done = (th.rand(pop, rows, generator=gen, device=dev) < 0.05).float()
    w = th.softmax(rnd(pop, rows if eng.w_input else 1, R), dim=-1).contiguous()
    iters = 2 if algo == ALGO_MOSAC else 1
    state = {"seed": 0}
    sync = None
    if dp:
        from morl_baselines_amd.distributed import average_gradients
        sync = average_gradients(dist)
        for buf in (eng.q, eng.pol, eng.q_target):
            dist.broadcast(buf, src=0)

    def step():
        state["seed"] += 1
        cfg = eng.make_cfg(q_lr=1e-3 if algo == ALGO_MOSAC else 3e-4, policy_iters=iters, autotune=(algo == ALGO_MOSAC),
                           target_entropy=-float(Ad), n_per=(B if wl == "gpipd" else 0), dropout_seed=state["seed"])
        eps = th.randn((1 + 2 * iters, pop, rows, Ad), dtype=th.float32, device=dev)      # the host agents draw these too
        eng.update(cfg, obs=obs, actions=act, rewards=rew, next_obs=nobs, dones=done, w=w, eps_next=eps[0],
                   eps_pi=eps[1:1 + iters], eps_alpha=eps[1 + iters:], want=("critic_loss",), grad_sync=sync)

    for _ in range(a.warmup):
        step()
    th.cuda.synchronize()
    if dist is not None:
        dist.barrier()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        step()
    th.cuda.synchronize()
    if dist is not None:
        dist.barrier()
    wall = time.perf_counter() - t0
    if dist is not None:
        t = th.tensor([wall], device=dev, dtype=th.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        wall = float(t.item())
        pop = pop_total
        if dp:
            rows = rows * world              # the job's batch
        if rank != 0:
            dist.destroy_process_group()
            return
    ms = wall * 1e3 / a.steps
    flop = update_flop(wl, D, Ad, R, rows, iters) * pop
    tf = flop / (ms * 1e-3) / 1e12
    out = {
        "metric": "actor-critic learner updates/sec", "value": pop * a.steps / wall, "unit": "learner-updates/s",
        "rows_per_s": pop * rows * a.steps / wall,
        "n_gpus": world, "steps": a.steps, "warmup": a.warmup, "ms_per_step": ms, "higher_is_better": True,
        "scaling": "weak" if (world == 1 or dp) else "strong", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
        "config": {"workload": f"{wl}: {pop} learner(s) x batch {B} ({rows} rows), net {ARCH}, twin critics, shapes of "
                               f"{shp['env']} (obs {D}, act {Ad}, {R} objectives); one morl_ac_update per step",
                   "population": pop, "rows": rows,
                   "parallelism": "single GPU" if world == 1 else
                                  (f"data-parallel over {world} GPUs: {rows // world} rows each, critic and actor gradients "
                                   "all-reduced (RCCL) inside the update, identical Adam steps" if dp else
                                   f"population split over {world} GPUs ({pop // world} learners each), independent "
                                   "replicas, no data-path collective")},
        "roofline": {"bound": "mfma", "kernel": "gemm_batched (exact-fp32 MFMA layers of all nets / learners)",
                     "achieved": tf, "peak": PEAK_FP32_MFMA_TFLOPS, "unit": "TFLOP/s", "frac": tf / PEAK_FP32_MFMA_TFLOPS,
                     "traffic": None,
                     "note": "algorithmic GEMM flop of the whole update / wall time of the step (launch-latency included): "
                             "a lower bound of the kernels' own rate; per-kernel durations in profiles/"},
        "algorithmic_flop_per_step": flop,
    }
    if not a.no_cpu_baseline and world == 1:
        out["cpu_baseline"] = cpu_baseline(wl, shp, pop)
        out["speedup_vs_cpu_baseline"] = out["value"] / out["cpu_baseline"]["value"]
    print(json.dumps(out), file=RESULT_OUT, flush=True)
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
