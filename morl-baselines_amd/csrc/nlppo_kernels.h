// Non-linear multi-objective PPO (single_policy/ser/nl_mo_ppo.py), the learner behind every Pareto-oracle query of IPRO: one
// minibatch step of NLMOPPO.update() (nl_mo_ppo.py:346-393) as ONE launch, the reverse scan of _compute_advantages_and_returns
// (nl_mo_ppo.py:290-308) and the no-grad get_action_and_value / get_value (nl_mo_ppo.py:90-108).  fp32 throughout.
//
//   input:       obs | accrued discounted reward [R] | preference [pref_dim] (zeros when there is none)          D = D_in
//   critic:      input -> hidden (Tanh) -> [R]          actor: input -> hidden (Tanh) -> logits [A]
//   logp       = logits - logsumexp(logits);  newlogprob = logp[action];  ratio = exp(newlogprob - old log-prob)
//   per_obj_k  = mean_b max(-adv_bk ratio, -adv_bk clamp(ratio, 1 - c, 1 + c))      (adv_k normalised per objective over the minibatch)
//   pg         = sum_k w_k per_obj_k                                                 (w = du/dv at v(s0): any sign)
//   v          = 0.5 mean_{b,k} max((v - ret)^2, (old + clamp(v - old, -c, c) - ret)^2)        (or the unclipped square alone)
//   loss       = pg - ent_coef * mean_b H_b + vf_coef * v,  H_b = -sum_j p_j logp_j;  clip_grad_norm_;  Adam(eps = 1e-5)
//
// Structure: that of ppo_kernels.h, whose MLP forward / backward, transposed product and tile state are used as they are.  What
// is new: the categorical head (its entropy back-propagates through the actor, so every row has its own entropy gradient), the
// [R] advantages of a row with one mean / std per objective, and the per-objective choice of the surrogate's active branch.  The
// value loss, the ticket and the last workgroup's reduction, clip scale and Adam step are ppo_kernels.h's functions, called
// without the log-std tensor.
#pragma once
#include "ppo_kernels.h"

namespace morl {

constexpr int NLPPO_NPART = PPO_MAX_R + 5;   // per-tile sums: surrogate of objective k [8], v, -logratio, (ratio - 1) - logratio, clipped rows, entropy
constexpr int NLPPO_SEG = 32;                // work-items that share the sums of one objective
constexpr int NLPPO_MAX_TENSORS = 12;        // 2 networks x 3 layers x (weight, bias)
static_assert(NLPPO_SEG * PPO_MAX_R == PPO_THREADS, "one segment of the reduction per objective");
static_assert(NLPPO_MAX_TENSORS <= PPO_MAX_TENSORS, "the per-tensor sums of squares reuse PpoLds::w as MO-PPO's do");

struct NlppoLds {
    PpoLds p;                                // MO-PPO's tile state: ppo_mlp_forward / ppo_mlp_backward work on it
    float adv[PPO_TB * PPO_MAX_R];           // the rows' advantages
    float rs[PPO_TB * NLPPO_NPART];          // per-row loss terms
    float amean[PPO_MAX_R], astd[PPO_MAX_R]; // per objective: mean and std + 1e-8 of the minibatch's advantages
    float w[PPO_MAX_R];                      // loss weights
    int action[PPO_TB];
};
static_assert(sizeof(NlppoLds) <= 64 * 1024, "NL-MO-PPO tile state must fit 64 KB of static LDS");

// the input widths; n.D of the PpoNet is their sum
struct NlppoIn {
    int obs_dim, pref_dim;
};

// In place: z[j] <- z[j] - (max + log(sum_j exp(z[j] - max))), the sum in index order (torch.logsumexp).  Both kernels call this,
// so a stored log-prob is reproduced bit for bit while the parameters are unchanged.
__device__ __forceinline__ void nlppo_log_softmax(float* z, int A) {
    float m = z[0];
    for (int j = 1; j < A; ++j) m = fmaxf(m, z[j]);
    float s = 0.0f;
    for (int j = 0; j < A; ++j) s = __fadd_rn(s, expf(__fsub_rn(z[j], m)));
    const float lse = __fadd_rn(m, logf(s));
    for (int j = 0; j < A; ++j) z[j] = __fsub_rn(z[j], lse);
}

// sums within each aligned group of NLPPO_SEG entries by a fixed tree (the same bits in every workgroup); returns the sum of
// the caller's own group
__device__ __forceinline__ float nlppo_seg_sum(float* red, float v) {
    const int tid = (int)threadIdx.x, lane = tid & (NLPPO_SEG - 1);
    __syncthreads();
    red[tid] = v;
    __syncthreads();
    for (int s = NLPPO_SEG / 2; s > 0; s >>= 1) {
        if (lane < s) red[tid] = __fadd_rn(red[tid], red[tid + s]);
        __syncthreads();
    }
    return red[tid - lane];
}

// ---------------------------------------------------------------------------------------------------------------------
// no-grad get_action_and_value / get_value / get_greedy_action: value_out [rows][R], logp_out [rows][A] (normalised)
// ---------------------------------------------------------------------------------------------------------------------
static __global__ __launch_bounds__(PPO_THREADS) void nlppo_forward_kernel(PpoNet n, NlppoIn in, const float* __restrict__ params,
                                                                          const float* __restrict__ obs,
                                                                          const float* __restrict__ acc_reward,
                                                                          const float* __restrict__ pref, int rows, int value_only,
                                                                          float* __restrict__ logp_out,
                                                                          float* __restrict__ value_out) {
    __shared__ PpoLds L;
    const int tid = (int)threadIdx.x, row0 = (int)blockIdx.x * PPO_TB;
    const int ro = in.obs_dim, po = in.obs_dim + n.R;
    for (int o = tid; o < PPO_TB * n.D; o += PPO_THREADS) {
        const int r = o / n.D, d = o - r * n.D;
        float v = 0.0f;
        if (row0 + r < rows) {
            if (d < ro) v = obs[(size_t)(row0 + r) * in.obs_dim + d];
            else if (d < po) v = acc_reward[(size_t)(row0 + r) * n.R + (d - ro)];
            else if (pref != nullptr) v = pref[d - po];
        }
        L.x[o] = v;
    }
    ppo_mlp_forward(L, n, n.c, params, n.R);
    for (int o = tid; o < PPO_TB * n.R; o += PPO_THREADS) {
        const int r = o / n.R;
        if (row0 + r < rows) value_out[(size_t)row0 * n.R + o] = L.out[o];
    }
    if (value_only) return;
    ppo_mlp_forward(L, n, n.a, params, n.A);
    if (tid < PPO_TB) nlppo_log_softmax(L.out + tid * n.A, n.A);
    __syncthreads();
    for (int o = tid; o < PPO_TB * n.A; o += PPO_THREADS) {
        const int r = o / n.A;
        if (row0 + r < rows) logp_out[(size_t)row0 * n.A + o] = L.out[o];
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// rollout table: one row per (step, env):  input [D] | action | old log-prob | advantages [R] | returns [R] | old values [R]
// ---------------------------------------------------------------------------------------------------------------------
static __global__ __launch_bounds__(256) void nlppo_pack_kernel(int obs_dim, int R, int pref_dim, int row_w, int rows,
                                                                const float* __restrict__ obs, const float* __restrict__ acc_rewards,
                                                                const int* __restrict__ actions, const float* __restrict__ logprobs,
                                                                const float* __restrict__ values, const float* __restrict__ pref,
                                                                float* __restrict__ table) {
    const int D = obs_dim + R + pref_dim;
    const long long total = (long long)rows * row_w;
    for (long long o = (long long)blockIdx.x * blockDim.x + threadIdx.x; o < total; o += (long long)gridDim.x * blockDim.x) {
        const int row = (int)(o / row_w), c = (int)(o - (long long)row * row_w);
        float v = 0.0f;                                         // advantages and returns: written by nlppo_gae_kernel
        if (c < obs_dim) v = obs[(size_t)row * obs_dim + c];
        else if (c < obs_dim + R) v = acc_rewards[(size_t)row * R + (c - obs_dim)];
        else if (c < D) v = (pref != nullptr) ? pref[c - obs_dim - R] : 0.0f;
        else if (c == D) v = (float)actions[row];               // (an index below 2^24: exact)
        else if (c == D + 1) v = logprobs[row];
        else if (c >= D + 2 + 2 * R) v = values[(size_t)row * R + (c - (D + 2 + 2 * R))];
        table[o] = v;
    }
}

// _compute_advantages_and_returns: one work-item per env runs the reverse scan of all its objectives, in ppo_gae_scan's operation
// order, and keeps the advantage VECTOR:
//   delta = r + (gamma * next_v) * nonterminal - v;  adv = delta + ((gamma * gae_lambda) * nonterminal) * adv';  returns = adv + v
static __global__ __launch_bounds__(64) void nlppo_gae_kernel(int T, int E, int R, int row_w, int adv_col, float* __restrict__ table,
                                                              const float* __restrict__ rewards, const float* __restrict__ dones,
                                                              const float* __restrict__ next_value,
                                                              const float* __restrict__ next_done, float gamma, float gamma_lambda,
                                                              float* __restrict__ returns_out, float* __restrict__ adv_out) {
    const int e = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (e >= E) return;
    float carry[PPO_MAX_R], nextv[PPO_MAX_R];
#pragma unroll
    for (int k = 0; k < PPO_MAX_R; ++k) {
        carry[k] = 0.0f;
        nextv[k] = (k < R) ? next_value[e * R + k] : 0.0f;
    }
    float nonterminal = __fsub_rn(1.0f, next_done[e]);
    for (int t = T - 1; t >= 0; --t) {
        const size_t row = (size_t)t * E + e;
        float* trow = table + row * row_w + adv_col;          // advantages [R] | returns [R] | values [R]
#pragma unroll
        for (int k = 0; k < PPO_MAX_R; ++k) {
            if (k < R) {
                const float r = rewards[row * R + k], v = trow[2 * R + k];
                const float delta = __fsub_rn(__fadd_rn(r, __fmul_rn(__fmul_rn(gamma, nextv[k]), nonterminal)), v);
                const float adv = __fadd_rn(delta, __fmul_rn(__fmul_rn(gamma_lambda, nonterminal), carry[k]));
                const float ret = __fadd_rn(adv, v);
                carry[k] = adv;
                nextv[k] = v;
                trow[k] = adv;
                trow[R + k] = ret;
                if (adv_out != nullptr) adv_out[row * R + k] = adv;
                if (returns_out != nullptr) returns_out[row * R + k] = ret;
            }
        }
        nonterminal = __fsub_rn(1.0f, dones[row]);            // what step t - 1 sees as its successor's done flag
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// one minibatch step
// ---------------------------------------------------------------------------------------------------------------------
struct NlppoStepArgs {
    PpoStepArgs s;                 // n.D = D_in, n.oLs is not used; lpart is [ntiles][NLPPO_NPART]
    const float* loss_weights;     // [R]
};

static __global__ __launch_bounds__(PPO_THREADS) void nlppo_step_kernel(NlppoStepArgs args) {
    __shared__ NlppoLds S;
    PpoLds& L = S.p;
    const PpoStepArgs& a = args.s;
    const PpoNet& n = a.n;
    const int tid = (int)threadIdx.x, tile = (int)blockIdx.x, row0 = tile * PPO_TB;
    const int valid = min(PPO_TB, a.M - row0);
    const float* p = a.params;
    const int ac = n.D, lo = n.D + 1, adv_col = n.D + 2, ro = adv_col + n.R, vo = ro + n.R;

    // ---- gather (nl_mo_ppo.py:348-365): table row idx[b] -> input, action, old log-prob, advantages, returns, old values
    for (int o = tid; o < PPO_TB * n.D; o += PPO_THREADS) {
        const int r = o / n.D, d = o - r * n.D;
        float v = 0.0f;
        if (r < valid) {
            const int row = ppo_table_row(a.idx, row0 + r, a.table_rows);
            v = a.table[(size_t)row * a.row_w + d];
        }
        L.x[o] = v;
    }
    for (int o = tid; o < PPO_TB * n.R; o += PPO_THREADS) {
        const int r = o / n.R, k = o - r * n.R;
        float adv = 0.0f, ret = 0.0f, ov = 0.0f;
        if (r < valid) {
            const int row = ppo_table_row(a.idx, row0 + r, a.table_rows);
            adv = a.table[(size_t)row * a.row_w + adv_col + k];
            ret = a.table[(size_t)row * a.row_w + ro + k];
            ov = a.table[(size_t)row * a.row_w + vo + k];
        }
        S.adv[o] = adv;
        L.ret[o] = ret;
        L.oldv[o] = ov;
    }
    if (tid < PPO_TB) {
        float lp = 0.0f;
        int act = 0;
        if (tid < valid) {
            const int row = ppo_table_row(a.idx, row0 + tid, a.table_rows);
            lp = a.table[(size_t)row * a.row_w + lo];
            act = min(max((int)a.table[(size_t)row * a.row_w + ac], 0), n.A - 1);
        }
        L.row[tid * 4] = lp;
        S.action[tid] = act;
    }
    if (tid < PPO_MAX_R) S.w[tid] = (tid < n.R) ? args.loss_weights[tid] : 0.0f;

    // ---- advantage normalisation (nl_mo_ppo.py:366-369): per objective the mean and unbiased std of all M advantages, read in
    // minibatch order; objective k belongs to the work-items [32 k, 32 k + 32), whose sums meet in a fixed tree
    if (a.norm_adv) {
        const int k = tid / NLPPO_SEG, lane = tid - k * NLPPO_SEG;
        float s = 0.0f;
        if (k < n.R)
            for (int b = lane; b < a.M; b += NLPPO_SEG) {
                const int row = ppo_table_row(a.idx, b, a.table_rows);
                s = __fadd_rn(s, a.table[(size_t)row * a.row_w + adv_col + k]);
            }
        const float mean = __fdiv_rn(nlppo_seg_sum(L.red, s), a.fM);
        float q = 0.0f;
        if (k < n.R)
            for (int b = lane; b < a.M; b += NLPPO_SEG) {
                const int row = ppo_table_row(a.idx, b, a.table_rows);
                const float dlt = __fsub_rn(a.table[(size_t)row * a.row_w + adv_col + k], mean);
                q = fmaf(dlt, dlt, q);
            }
        const float var = __fmul_rn(nlppo_seg_sum(L.red, q), a.inv_Mm1);
        if (lane == 0 && k < n.R) {
            S.amean[k] = mean;
            S.astd[k] = __fadd_rn(__fsqrt_rn(var), 1e-8f);
        }
    }
    __syncthreads();

    float* part = a.part + (size_t)tile * n.P;

    // ---- critic: forward, value loss (nl_mo_ppo.py:378-385) and its gradient, backward
    ppo_mlp_forward(L, n, n.c, p, n.R);
    if (tid < PPO_TB) S.rs[tid * NLPPO_NPART + PPO_MAX_R] = ppo_value_loss_row(L, a, tid, valid);
    __syncthreads();
    ppo_mlp_backward(L, n, n.c, p, part, n.R);

    // ---- actor: forward, categorical log-prob and entropy, ratio, per-objective surrogate (nl_mo_ppo.py:349-375), the gradient
    // at the logits, backward
    ppo_mlp_forward(L, n, n.a, p, n.A);
    if (tid < PPO_TB) {
        const int r = tid;
        float* z = L.out + r * n.A;
        float* dz = L.dout + r * n.A;
        float* rs = S.rs + r * NLPPO_NPART;
        float nlr = 0.0f, kl = 0.0f, cf = 0.0f, ent = 0.0f;
        for (int k = 0; k < PPO_MAX_R; ++k) rs[k] = 0.0f;
        if (r < valid) {
            nlppo_log_softmax(z, n.A);
            float plp = 0.0f;
            for (int j = 0; j < n.A; ++j) {
                const float pj = expf(z[j]);
                dz[j] = pj;
                if (pj > 0.0f) plp = __fadd_rn(plp, __fmul_rn(pj, z[j]));          // p == 0 contributes 0
            }
            ent = -plp;
            const int act = S.action[r];
            const float logratio = __fsub_rn(z[act], L.row[r * 4]);
            const float ratio = expf(logratio);
            const float rc = fminf(fmaxf(ratio, a.clip_lo), a.clip_hi);
            // torch.max splits a tie evenly: inside the clip range both branches are the same number with the derivative -adv;
            // outside, the clipped branch has none.  Which branch is the larger depends on the sign of adv_k: per objective.
            const bool inside = ratio >= a.clip_lo && ratio <= a.clip_hi;
            float s = 0.0f;
            for (int k = 0; k < n.R; ++k) {
                float adv = S.adv[r * n.R + k];
                if (a.norm_adv) adv = __fdiv_rn(__fsub_rn(adv, S.amean[k]), S.astd[k]);
                const float pg1 = __fmul_rn(-adv, ratio);
                const float pg2 = __fmul_rn(-adv, rc);
                rs[k] = fmaxf(pg1, pg2);
                if (inside || pg1 > pg2) s = fmaf(S.w[k], -adv, s);
            }
            const float dlp = __fmul_rn(__fmul_rn(s, ratio), a.inv_M);
            const float ec = __fmul_rn(a.ent_coef, a.inv_M);
            // d loss / d z_j = dlp (delta_aj - p_j) + (ent_coef / M) p_j (logp_j + H)
            for (int j = 0; j < n.A; ++j) {
                const float pj = dz[j];
                const float onehot = (j == act) ? 1.0f : 0.0f;
                const float ge = (pj > 0.0f) ? __fmul_rn(__fmul_rn(ec, pj), __fadd_rn(z[j], ent)) : 0.0f;
                dz[j] = fmaf(dlp, __fsub_rn(onehot, pj), ge);
            }
            nlr = -logratio;
            kl = __fsub_rn(__fsub_rn(ratio, 1.0f), logratio);
            cf = (fabsf(__fsub_rn(ratio, 1.0f)) > a.clip_coef) ? 1.0f : 0.0f;
        } else {
            for (int j = 0; j < n.A; ++j) dz[j] = 0.0f;
        }
        rs[PPO_MAX_R + 1] = nlr;
        rs[PPO_MAX_R + 2] = kl;
        rs[PPO_MAX_R + 3] = cf;
        rs[PPO_MAX_R + 4] = ent;
    }
    __syncthreads();
    if (tid < NLPPO_NPART) {
        float s = 0.0f;
        for (int r = 0; r < PPO_TB; ++r) s = __fadd_rn(s, S.rs[r * NLPPO_NPART + tid]);
        a.lpart[tile * NLPPO_NPART + tid] = s;
    }
    ppo_mlp_backward(L, n, n.a, p, part, n.A);

    // ---- the last workgroup to arrive owns the step
    if (!pcn_last_arrival(a.ticket, a.ntiles, L.last)) return;
    const PpoLearner l = ppo_own_learner(a);
    const float total = ppo_grad_clip(L, a, l, false);
    if (tid == 0) {
        *a.ticket = 0u;                                        // re-armed for the next launch on the stream
        float ls[NLPPO_NPART];
        for (int i = 0; i < NLPPO_NPART; ++i) ls[i] = 0.0f;
        for (int t = 0; t < a.ntiles; ++t)
            for (int i = 0; i < NLPPO_NPART; ++i) ls[i] = __fadd_rn(ls[i], a.lpart[t * NLPPO_NPART + i]);
        float pg = 0.0f;                                       // (per_obj_pg * loss_weights).sum()
        for (int k = 0; k < n.R; ++k) pg = __fadd_rn(pg, __fmul_rn(__fdiv_rn(ls[k], a.fM), S.w[k]));
        const float v = __fmul_rn(0.5f, __fdiv_rn(ls[PPO_MAX_R], a.fMR));
        const float ent = __fdiv_rn(ls[PPO_MAX_R + 4], a.fM);
        a.stats_out[0] = __fadd_rn(__fsub_rn(pg, __fmul_rn(a.ent_coef, ent)), __fmul_rn(a.vf_coef, v));
        a.stats_out[1] = pg;
        a.stats_out[2] = v;
        a.stats_out[3] = ent;
        a.stats_out[4] = __fdiv_rn(ls[PPO_MAX_R + 1], a.fM);
        a.stats_out[5] = __fdiv_rn(ls[PPO_MAX_R + 2], a.fM);
        a.stats_out[6] = __fdiv_rn(ls[PPO_MAX_R + 3], a.fM);
        a.stats_out[7] = total;
    }
    __syncthreads();
    ppo_adam_sweep(L, a, l);
}

}  // namespace morl
