"""A seeded ``NLMOPPO.train()`` of two iterations on ``tests/nlppo_env.py`` against the trace recorded from the reference class.

The environment's horizon is fixed, so the episode boundaries are the recorded ones whatever the rounding.  The generator refused
seeds at which a logit change of 1e-4 relative moves a sampled action, so the sampled actions are held to the recorded ones
exactly; rewards to 1e-5 relative + 1e-6, the parameters after each iteration to the per-step bound of
``test_nlppo_kernels_parity.py`` (2e-5 relative + 0.02 * lr per optimiser step) times the steps taken so far, the loss weights of
each update to 1e-4 relative, the final ``policy_evaluate`` vector to 1e-5."""
import numpy as np
import pytest
import torch as th

import nlppo_cases as nc
import nlppo_common as nm
import nlppo_env


@pytest.mark.parametrize("be_name", nm.BACKENDS)
def test_train_trace_matches_the_reference(be_name):
    from morl_baselines_amd.nl_mo_ppo import NLMOPPO
    lib, dev = nm.backend(be_name)
    g, Tr = nm.load("trace"), nc.TRACE
    env = nlppo_env.DiscreteLinearVecEnv(num_envs=Tr["num_envs"], **Tr["env"])
    eval_env = nlppo_env.DiscreteLinearEnv(**Tr["env"])
    nc.reseed(Tr["seed"])
    with nm.one_thread():
        ag = NLMOPPO(0, env, log=False, device=dev, seed=Tr["seed"], lib=lib, **Tr["agent"])
    # (orthogonal_ is a LAPACK QR whose rounding differs between CPUs: the seeded construction is held to that rounding --
    # n * 2^-23 * gain, n <= 64 -- and the replay starts from the recorded parameters)
    nm.close_rel("initial parameters", ag.params.cpu().numpy(), g["init"], 0.0, 64 * 2.0 ** -23 * 2.0 ** 0.5)
    ag.params.copy_(th.tensor(g["init"]))
    evaluate = ag.policy_evaluate
    ag.policy_evaluate = lambda e, deterministic=False: evaluate(e, eval_episodes=Tr["eval_episodes"], deterministic=deterministic)
    inner_update, seen = ag.update, []

    def update():
        lr = ag.optimizer.param_groups[0]["lr"]
        out = inner_update()
        seen.append((ag.params.cpu().numpy().copy(), ag.last_loss_weights.numpy().copy(), lr, ag.optimizer.steps))
        return out

    ag.update = update
    nc.reseed(Tr["seed"] + 1)
    result = ag.train(eval_env, nc.utility(Tr["referent"], Tr["scale"]), pref=np.asarray(Tr["referent"], dtype=np.float32),
                      deterministic=True)
    assert np.array_equal(np.stack(env.action_log), g["actions"]), "sampled actions"
    nm.close_rel("rewards", np.stack(env.reward_log), g["rewards"], 1e-5, 1e-6)
    assert len(seen) == Tr["iterations"]
    steps, base_lr = 0, Tr["agent"]["learning_rate"]
    for it, (params, weights, lr, done) in enumerate(seen, 1):
        steps += int(g["steps"][it - 1])
        assert done == steps and lr == float(g["lr"][it - 1])
        nm.close_rel(f"parameters after iteration {it}", params, g[f"params_{it}"], 2e-5 * steps, 0.02 * base_lr * steps)
        nm.close_rel(f"loss weights of update {it}", weights, g["weights"][it - 1], 1e-4)
    assert ag.optimizer.param_groups[0]["lr"] == 0.5 * base_lr           # anneal_lr: the second of two iterations
    assert ag.global_step == int(g["global_step"].reshape(-1)[0])
    assert np.array_equal(np.asarray(eval_env.action_log), g["eval_actions"]), "greedy actions of policy_evaluate"
    nm.close_rel("policy_evaluate", result, g["result"], 1e-5)
