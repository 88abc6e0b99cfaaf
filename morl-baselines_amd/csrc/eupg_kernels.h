// Expected Utility Policy Gradient (single_policy/esr/eupg.py): the whole of EUPG.update() (eupg.py:227-251) as TWO launches with
// the user's scalarisation between them -- the reverse discounted scan of _forward_cumulative_rewards (eupg.py:263-270), then
// forward, loss, backward and Adam of the episode as ONE launch -- and the no-grad forward behind every action (eupg.py:46-61).
// fp32 throughout.
//
//   input:  obs | accrued reward [R]                                                                         D = obs_dim + R
//   net:    input -> hidden (Tanh) -> z [A];   s_j = sigmoid(z_j);   p_j = s_j / sum_j s_j
//   logp_t = log(clamp(p_t[a_t], eps, 1 - eps)),  eps = 2^-23          (Categorical(probs=...).log_prob)
//   loss   = -mean_t(logp_t * u_t),  u = scalarization(G),  G_t = gamma * G_{t+1} + r_t
//   dz_j   = -(u_t / T) s_j (1 - s_j) (delta_aj / s_a - 1 / sum_j s_j);  a row whose p_a leaves [eps, 1 - eps] has no gradient
//   Adam, torch defaults (eps 1e-8); no gradient clipping
//
// The reference divides the sigmoids by their sum over the WHOLE batch and lets Categorical divide by the row sum; the batch-wide
// factor cancels, and each row is normalised on its own here (eupg_normalise_row, shared by both kernels).
//
// Structure: that of ppo_kernels.h, whose MLP forward / backward and tile state are used as they are.  What is new: the episode
// is ONE batch of any length, so the grid is capped (max_workgroups) and a workgroup walks the tiles wg, wg + nwg, ... in order,
// adding each tile's weight-gradient partial onto its own full-length partial.  The workgroup that draws the last ticket sums the
// partials in workgroup order, applies Adam, writes the loss and re-arms the ticket.  No grid barrier, no floating-point atomics.
#pragma once
#include "ppo_kernels.h"

namespace morl {

constexpr float EUPG_EPS = 1.1920928955078125e-07f;   // torch.finfo(float32).eps: Categorical clamps probs to [eps, 1 - eps]

struct EupgLds {
    PpoLds p;                 // MO-PPO's tile state: ppo_mlp_forward / ppo_mlp_backward work on it
    float u[PPO_TB];          // the rows' scalarised returns
    float term[PPO_TB];       // logp_t * u_t
    int action[PPO_TB];
};
static_assert(sizeof(EupgLds) <= 64 * 1024, "EUPG tile state must fit 64 KB of static LDS");

// s[j] = sigmoid(z[j]), p[j] = s[j] / sum_j s[j], the sum in index order; returns the sum.  Both kernels call this, so the
// probabilities a step forms are the forward launch's bit for bit while the parameters are unchanged.  (s may be z.)
__device__ __forceinline__ float eupg_normalise_row(const float* z, float* s, float* p, int A) {
    float sum = 0.0f;
    for (int j = 0; j < A; ++j) {
        const float sj = pcn_sigmoid(z[j]);
        s[j] = sj;
        sum = __fadd_rn(sum, sj);
    }
    for (int j = 0; j < A; ++j) p[j] = __fdiv_rn(s[j], sum);
    return sum;
}

// _forward_cumulative_rewards: G_t = gamma * G_{t+1} + r_t, one work-item per objective, a multiply then an add as torch forms it
static __global__ __launch_bounds__(64) void eupg_return_kernel(int T, int R, const float* __restrict__ rewards, float gamma,
                                                                float* __restrict__ out) {
    const int k = (int)threadIdx.x;
    if (k >= R) return;
    float G = 0.0f;
    for (int t = T - 1; t >= 0; --t) {
        G = __fadd_rn(__fmul_rn(gamma, G), rewards[(size_t)t * R + k]);
        out[(size_t)t * R + k] = G;
    }
}

// episode table: one row per step:  obs [obs_dim] | accrued reward [R] | action (an index below 2^24: exact as a float)
static __global__ __launch_bounds__(256) void eupg_pack_kernel(int obs_dim, int R, int row_w, int rows, const float* __restrict__ obs,
                                                               const float* __restrict__ acc_rewards, const int* __restrict__ actions,
                                                               float* __restrict__ table) {
    const long long total = (long long)rows * row_w;
    for (long long o = (long long)blockIdx.x * blockDim.x + threadIdx.x; o < total; o += (long long)gridDim.x * blockDim.x) {
        const int row = (int)(o / row_w), c = (int)(o - (long long)row * row_w);
        float v;
        if (c < obs_dim) v = obs[(size_t)row * obs_dim + c];
        else if (c < obs_dim + R) v = acc_rewards[(size_t)row * R + (c - obs_dim)];
        else v = (float)actions[row];
        table[o] = v;
    }
}

// no-grad PolicyNet.forward: probs_out [rows][A]
static __global__ __launch_bounds__(PPO_THREADS) void eupg_forward_kernel(PpoNet n, int obs_dim, const float* __restrict__ params,
                                                                         const float* __restrict__ obs,
                                                                         const float* __restrict__ acc_reward, int rows,
                                                                         float* __restrict__ probs_out) {
    __shared__ PpoLds L;
    const int tid = (int)threadIdx.x, row0 = (int)blockIdx.x * PPO_TB;
    for (int o = tid; o < PPO_TB * n.D; o += PPO_THREADS) {
        const int r = o / n.D, d = o - r * n.D;
        float v = 0.0f;
        if (row0 + r < rows) v = (d < obs_dim) ? obs[(size_t)(row0 + r) * obs_dim + d] : acc_reward[(size_t)(row0 + r) * n.R + (d - obs_dim)];
        L.x[o] = v;
    }
    ppo_mlp_forward(L, n, n.a, params, n.A);
    if (tid < PPO_TB) eupg_normalise_row(L.out + tid * n.A, L.dout + tid * n.A, L.out + tid * n.A, n.A);
    __syncthreads();
    for (int o = tid; o < PPO_TB * n.A; o += PPO_THREADS) {
        const int r = o / n.A;
        if (row0 + r < rows) probs_out[(size_t)row0 * n.A + o] = L.out[o];
    }
}

struct EupgStepArgs {
    PpoNet n;                      // n.D = obs_dim + R; the network is n.a, n.c is not used
    float* params;                 // [P]  read by every tile, stepped by the last workgroup
    float* exp_avg;                // [P]
    float* exp_avg_sq;             // [P]
    const float* table;            // [T][row_w]
    const float* u;                // [T] scalarised returns
    int row_w, T, ntiles, nwg;
    float* part;                   // [nwg][P] the workgroups' gradient partials
    float* tpart;                  // [nwg][P] the partial of the tile a workgroup is working on
    float* lpart;                  // [nwg] sums of logp_t * u_t
    float* probs;                  // [T][A] the probabilities this step formed
    unsigned int* ticket;          // arrival counter, zero between launches
    float* loss_out;
    float fT;                      // a mean is a sum DIVIDED by its count, as torch forms it
    float one_minus_b1, b2, one_minus_b2, neg_step_size, bc2_sqrt, eps;
};

static __global__ __launch_bounds__(PPO_THREADS) void eupg_step_kernel(EupgStepArgs a) {
    __shared__ EupgLds S;
    PpoLds& L = S.p;
    const PpoNet& n = a.n;
    const int tid = (int)threadIdx.x, wg = (int)blockIdx.x;
    const float* p = a.params;
    float* part = a.part + (size_t)wg * n.P;
    float* tpart = a.tpart + (size_t)wg * n.P;
    float lsum = 0.0f;                                         // (work-item 0's)

    for (int tile = wg; tile < a.ntiles; tile += a.nwg) {
        const int row0 = tile * PPO_TB, valid = min(PPO_TB, a.T - row0);
        // ---- gather: episode rows [row0, row0 + valid) -> input, action, scalarised return
        for (int o = tid; o < PPO_TB * n.D; o += PPO_THREADS) {
            const int r = o / n.D, d = o - r * n.D;
            L.x[o] = (r < valid) ? a.table[(size_t)(row0 + r) * a.row_w + d] : 0.0f;
        }
        if (tid < PPO_TB) {
            float u = 0.0f;
            int act = 0;
            if (tid < valid) {
                u = a.u[row0 + tid];
                act = min(max((int)a.table[(size_t)(row0 + tid) * a.row_w + n.D], 0), n.A - 1);
            }
            S.u[tid] = u;
            S.action[tid] = act;
        }

        // ---- forward, the normalised sigmoid, log-prob of the taken action, the gradient at z (eupg.py:244-247)
        ppo_mlp_forward(L, n, n.a, p, n.A);
        if (tid < PPO_TB) {
            const int r = tid;
            float* z = L.out + r * n.A;
            float* dz = L.dout + r * n.A;
            float term = 0.0f;
            if (r < valid) {
                const float sum = eupg_normalise_row(z, dz, z, n.A);       // dz: the sigmoids, z: the probabilities
                const int act = S.action[r];
                const float pa = z[act], sa = dz[act], u = S.u[r];
                const bool clamped = pa < EUPG_EPS || pa > __fsub_rn(1.0f, EUPG_EPS);
                const float logp = logf(fminf(fmaxf(pa, EUPG_EPS), __fsub_rn(1.0f, EUPG_EPS)));
                term = __fmul_rn(logp, u);
                const float c = clamped ? 0.0f : __fdiv_rn(-u, a.fT);
                const float inv_sa = __fdiv_rn(1.0f, sa), inv_sum = __fdiv_rn(1.0f, sum);
                for (int j = 0; j < n.A; ++j) {
                    const float sj = dz[j];
                    const float g = __fmul_rn(__fmul_rn(sj, __fsub_rn(1.0f, sj)), __fsub_rn((j == act) ? inv_sa : 0.0f, inv_sum));
                    dz[j] = clamped ? 0.0f : __fmul_rn(c, g);
                }
            } else {
                for (int j = 0; j < n.A; ++j) dz[j] = 0.0f;
            }
            S.term[r] = term;
        }
        __syncthreads();
        for (int o = tid; o < valid * n.A; o += PPO_THREADS) a.probs[(size_t)row0 * n.A + o] = L.out[o];
        if (tid == 0) {
            float s = 0.0f;
            for (int r = 0; r < PPO_TB; ++r) s = __fadd_rn(s, S.term[r]);
            lsum = __fadd_rn(lsum, s);
        }

        // ---- backward: the workgroup's first tile writes its partial, a later one is added onto it (tile order)
        const bool first = tile == wg;
        ppo_mlp_backward(L, n, n.a, p, first ? part : tpart, n.A);
        if (!first)
            for (int q = tid; q < n.P; q += PPO_THREADS) part[q] = __fadd_rn(part[q], tpart[q]);
    }
    if (tid == 0) a.lpart[wg] = lsum;

    // ---- the last workgroup to arrive owns the step
    if (!pcn_last_arrival(a.ticket, a.nwg, L.last)) return;
    if (tid == 0) {
        *a.ticket = 0u;                                        // re-armed for the next launch on the stream
        float s = 0.0f;
        for (int w = 0; w < a.nwg; ++w) s = __fadd_rn(s, a.lpart[w]);
        *a.loss_out = -__fdiv_rn(s, a.fT);
    }
    // the partials summed in workgroup order (four loads in flight, added in order), then Adam with torch's defaults
    for (int q = tid; q < n.P; q += PPO_THREADS) {
        float g = a.part[q];
        int w = 1;
        for (; w + 4 <= a.nwg; w += 4) {
            const float g0 = a.part[(size_t)w * n.P + q], g1 = a.part[(size_t)(w + 1) * n.P + q];
            const float g2 = a.part[(size_t)(w + 2) * n.P + q], g3 = a.part[(size_t)(w + 3) * n.P + q];
            g = __fadd_rn(__fadd_rn(__fadd_rn(__fadd_rn(g, g0), g1), g2), g3);
        }
        for (; w < a.nwg; ++w) g = __fadd_rn(g, a.part[(size_t)w * n.P + q]);
        pcn_adam(g, a.params[q], a.exp_avg[q], a.exp_avg_sq[q], a.one_minus_b1, a.b2, a.one_minus_b2, a.neg_step_size, a.bc2_sqrt,
                 a.eps);
    }
}

}  // namespace morl
