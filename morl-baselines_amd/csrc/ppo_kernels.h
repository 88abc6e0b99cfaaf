// Multi-objective PPO (single_policy/ser/mo_ppo.py): one minibatch step of MOPPO.update() (mo_ppo.py:509-554) as ONE launch, the
// reverse scan of __compute_advantages (mo_ppo.py:439-476) and the no-grad get_action_and_value (mo_ppo.py:215-235).  fp32; the
// terms of a row's log-prob are added in double (ppo_logprob_add).
//
//   critic:      obs -> hidden (Tanh) -> [R]          actor_mean: obs -> hidden (Tanh) -> [A]          actor_logstd [1][A]
//   newlogprob = sum_a Normal(mean, exp(logstd)).log_prob(action),  ratio = exp(newlogprob - old log-prob)
//   pg   = mean_b max(-adv ratio, -adv clamp(ratio, 1 - c, 1 + c))                       (adv normalised over the minibatch)
//   v    = 0.5 mean_{b,k} max((v - ret)^2, (old + clamp(v - old, -c, c) - ret)^2)        (or the unclipped square alone)
//   loss = pg - ent_coef * entropy + vf_coef * v;  clip_grad_norm_(max_grad_norm);  Adam(eps = 1e-5)
//
// Structure: that of pcn_kernels.h.  A workgroup owns PPO_TB = 16 rows of the minibatch: it gathers them from the rollout table,
// runs the critic forward and backward, then the actor forward and backward through the same LDS buffers, and writes its share of
// the gradient -- a full-length partial -- to part[tile][P].  The workgroup that draws the last ticket sums the partials in tile
// order, forms the clip scale, applies Adam, writes the step's statistics and re-arms the ticket.  No grid barrier, no
// floating-point atomics, nobody waits.  Unlike pcn_kernels.h the transposed products of the backward pass read their weights
// from an LDS stage (ppo_dense_t), not one L2 load per FMA, and the last workgroup loads four partials before it adds them.
#pragma once
#include "pcn_kernels.h"

namespace morl {

constexpr int PPO_THREADS = PCN_THREADS;
constexpr int PPO_TB = PCN_TB;          // minibatch rows per workgroup
constexpr int PPO_MAX_H = 128;          // a hidden width (a multiple of 32)
constexpr int PPO_MAX_D = 128;          // obs_dim
constexpr int PPO_MAX_A = 32;           // action_dim
constexpr int PPO_MAX_R = 8;            // reward_dim (MORL_MAX_OBJ)
constexpr int PPO_MAX_TENSORS = 13;     // actor_logstd + 2 networks x 3 layers x (weight, bias)
constexpr int PPO_NSTATS = 8;           // loss, pg_loss, v_loss, entropy, old_approx_kl, approx_kl, clipfrac, grad_norm
constexpr int PPO_NPART = 5;            // per-tile sums: pg, v, -logratio, (ratio - 1) - logratio, clipped rows
constexpr float PPO_HALF_LOG_2PI = 0.91893853320467274178f;   // log(sqrt(2 pi))
constexpr double PPO_HALF_LOG_2PI_D = 0.91893853320467274178;
static_assert(PPO_MAX_H <= PCN_MAX_H && PPO_THREADS == 256 && PPO_TB == 16, "pcn_dense / pcn_dw are shared");

// one of the two MLPs as a map into the flat parameter vector; with one hidden layer W1 / b1 are absent (H2 == H1, nh == 1)
struct PpoMlp {
    int oW0, ob0, oW1, ob1, oWo, obo;
};
// the flat vector in the order of MOPPONet.parameters(): actor_logstd, critic.*, actor_mean.*
struct PpoNet {
    int D, A, R, nh, H1, H2;   // H2: width of the last hidden layer
    int oLs;
    PpoMlp c, a;
    int P, ntensors;
    int tstart[PPO_MAX_TENSORS + 1];   // tensor boundaries (clip_grad_norm_ takes the 2-norm of the per-tensor 2-norms)
};

struct PpoLds {
    float w[PCN_MAX_H * PCN_WLD];     // staged weight chunk; the last workgroup's per-tensor sums of squares
    float x[PPO_TB * PPO_MAX_D];      // observations
    float h1[PPO_TB * PPO_MAX_H];     // tanh(layer 0)
    float h2[PPO_TB * PPO_MAX_H];     // tanh(layer 1); backward: d/d(its pre-activation)
    float d[PPO_TB * PPO_MAX_H];      // backward: d/d(a hidden activation), then d/d(layer 0 pre-activation)
    float out[PPO_TB * PPO_MAX_A];    // value [R] or action mean [A] of a row
    float dout[PPO_TB * PPO_MAX_A];   // d loss / d out
    float act[PPO_TB * PPO_MAX_A];    // the stored action; forward kernel: the noise
    float row[PPO_TB * 4];            // per row: old log-prob, advantage, d loss / d newlogprob
    float ret[PPO_TB * PPO_MAX_R], oldv[PPO_TB * PPO_MAX_R];
    float red[PPO_THREADS];
    float rs[PPO_TB * PPO_NPART];     // per-row loss terms
    float stat[4];                    // advantage mean, 1 / (std + 1e-8), clip scale, total norm
    int last;
};
static_assert(sizeof(PpoLds) <= 64 * 1024, "PPO tile state must fit 64 KB of static LDS");
static_assert(PPO_MAX_TENSORS * PPO_THREADS <= PCN_MAX_H * PCN_WLD, "per-tensor sums of squares reuse the weight stage");
static_assert(32 * (PPO_MAX_H + 1) <= PCN_MAX_H * PCN_WLD, "transposed stage: 32 rows of a weight");

// A row's log-prob is a sum of up to 32 terms of O(1) each, and the statistics approx_kl / old_approx_kl are means of its
// DIFFERENCE to the old log-prob: summed in float, the running sum's rounding (an ulp of up to 4e-6 per term at action_dim 31)
// and the 31-fold rounding of log(sqrt(2 pi)) are 1e-6 of those means.  The terms are formed in float as torch forms them and
// added in double; the sum is rounded to float once, so an unchanged policy still reproduces its stored log-prob bit for bit.
__device__ __forceinline__ double ppo_logprob_add(double lp, float t, float sd) {
    return lp + (((double)t - (double)logf(sd)) - PPO_HALF_LOG_2PI_D);
}

// forward of one MLP on the tile's rows in L.x: tanh activations in L.h1 (/ L.h2), the head's output in L.out [16][N]
__device__ __forceinline__ void ppo_mlp_forward(PpoLds& L, const PpoNet& n, const PpoMlp& m, const float* __restrict__ p, int N) {
    const int tid = (int)threadIdx.x;
    pcn_dense(L.w, p + m.oW0, p + m.ob0, n.H1, n.D, L.x, n.D, L.h1, n.H1);
    for (int o = tid; o < PPO_TB * n.H1; o += PPO_THREADS) L.h1[o] = tanhf(L.h1[o]);
    const float* hl = L.h1;
    if (n.nh == 2) {
        pcn_dense(L.w, p + m.oW1, p + m.ob1, n.H2, n.H1, L.h1, n.H1, L.h2, n.H2);
        for (int o = tid; o < PPO_TB * n.H2; o += PPO_THREADS) L.h2[o] = tanhf(L.h2[o]);
        hl = L.h2;
    }
    pcn_dense(L.w, p + m.oWo, p + m.obo, N, n.H2, hl, n.H2, L.out, N);
}

// z[r][k] = sum_j dz[r][j] W[j][k] for the 16 rows (W [N][K] row-major, global): W goes through LDS 32 rows at a time, a
// work-item owns column k of four rows, products are accumulated in j order.  Ends with a barrier.
__device__ __forceinline__ void ppo_dense_t(float* sw, const float* __restrict__ W, int N, int K, const float* dz, int ldz, float* z) {
    const int tid = (int)threadIdx.x, ld = K + 1;
    for (int j0 = 0; j0 < N; j0 += 32) {
        const int jc = min(32, N - j0);
        __syncthreads();
        for (int o = tid; o < jc * K; o += PPO_THREADS) {
            const int jj = o / K, k = o - jj * K;
            sw[jj * ld + k] = W[(size_t)(j0 + jj) * K + k];
        }
        __syncthreads();
        for (int o = tid; o < 4 * K; o += PPO_THREADS) {
            const int rg = o / K, k = o - rg * K;
            float acc[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) acc[u] = (j0 == 0) ? 0.0f : z[(rg * 4 + u) * K + k];
            for (int jj = 0; jj < jc; ++jj) {
                const float w = sw[jj * ld + k];
#pragma unroll
                for (int u = 0; u < 4; ++u) acc[u] = fmaf(dz[(rg * 4 + u) * ldz + j0 + jj], w, acc[u]);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) z[(rg * 4 + u) * K + k] = acc[u];
        }
    }
    __syncthreads();
}

// backward of one MLP from L.dout [16][N]: writes the tile's weight-gradient partial (row order) into part
__device__ __forceinline__ void ppo_mlp_backward(PpoLds& L, const PpoNet& n, const PpoMlp& m, const float* __restrict__ p,
                                                 float* __restrict__ part, int N) {
    const int tid = (int)threadIdx.x;
    float* hl = (n.nh == 2) ? L.h2 : L.h1;
    pcn_dw(part + m.oWo, L.dout, N, hl, n.H2, N, n.H2);
    pcn_db(part + m.obo, L.dout, N, N);
    ppo_dense_t(L.w, p + m.oWo, N, n.H2, L.dout, N, L.d);
    if (n.nh == 2) {
        for (int o = tid; o < PPO_TB * n.H2; o += PPO_THREADS) {
            const float t = L.h2[o];
            L.h2[o] = __fmul_rn(L.d[o], __fsub_rn(1.0f, __fmul_rn(t, t)));
        }
        __syncthreads();
        pcn_dw(part + m.oW1, L.h2, n.H2, L.h1, n.H1, n.H2, n.H1);
        pcn_db(part + m.ob1, L.h2, n.H2, n.H2);
        ppo_dense_t(L.w, p + m.oW1, n.H2, n.H1, L.h2, n.H2, L.d);
    }
    for (int o = tid; o < PPO_TB * n.H1; o += PPO_THREADS) {
        const float t = L.h1[o];
        L.d[o] = __fmul_rn(L.d[o], __fsub_rn(1.0f, __fmul_rn(t, t)));
    }
    __syncthreads();
    pcn_dw(part + m.oW0, L.d, n.H1, L.x, n.D, n.H1, n.D);
    pcn_db(part + m.ob0, L.d, n.H1, n.H1);
    __syncthreads();
}

// sum of red[0 .. 255] by a fixed tree: the same bits in every workgroup
__device__ __forceinline__ float ppo_tree_sum(float* red, float v) {
    const int tid = (int)threadIdx.x;
    __syncthreads();
    red[tid] = v;
    __syncthreads();
    for (int s = PPO_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] = __fadd_rn(red[tid], red[tid + s]);
        __syncthreads();
    }
    return red[0];
}

// ---------------------------------------------------------------------------------------------------------------------
// no-grad get_action_and_value / get_value
// ---------------------------------------------------------------------------------------------------------------------
// the body of ppo_forward_kernel / ppo_pop_forward_kernel: rows [tile * 16, tile * 16 + 16) of one learner
__device__ __forceinline__ void ppo_forward_tile(PpoLds& L, const PpoNet& n, int tile, const float* __restrict__ params,
                                                 const float* __restrict__ obs, const float* __restrict__ eps, int rows,
                                                 int value_only, float* __restrict__ action_out, float* __restrict__ logprob_out,
                                                 float* __restrict__ value_out) {
    const int tid = (int)threadIdx.x, row0 = tile * PPO_TB;
    for (int o = tid; o < PPO_TB * n.D; o += PPO_THREADS) {
        const int r = o / n.D, d = o - r * n.D;
        L.x[o] = (row0 + r < rows) ? obs[(size_t)(row0 + r) * n.D + d] : 0.0f;
    }
    ppo_mlp_forward(L, n, n.c, params, n.R);
    for (int o = tid; o < PPO_TB * n.R; o += PPO_THREADS) {
        const int r = o / n.R;
        if (row0 + r < rows) value_out[(size_t)row0 * n.R + o] = L.out[o];
    }
    if (value_only) return;
    for (int o = tid; o < PPO_TB * n.A; o += PPO_THREADS) {
        const int r = o / n.A;
        L.act[o] = (row0 + r < rows) ? eps[(size_t)row0 * n.A + o] : 0.0f;
    }
    ppo_mlp_forward(L, n, n.a, params, n.A);
    if (tid < PPO_TB && row0 + tid < rows) {
        const int r = tid;
        double lp = 0.0;
        for (int k = 0; k < n.A; ++k) {
            const float sd = expf(params[n.oLs + k]), mean = L.out[r * n.A + k];
            const float act = __fadd_rn(mean, __fmul_rn(sd, L.act[r * n.A + k]));        // Normal.sample(): loc + eps * scale
            const float diff = __fsub_rn(act, mean);
            const float var = __fmul_rn(sd, sd);
            const float t = __fdiv_rn(-__fmul_rn(diff, diff), __fmul_rn(2.0f, var));
            lp = ppo_logprob_add(lp, t, sd);
            action_out[(size_t)(row0 + r) * n.A + k] = act;
        }
        logprob_out[row0 + r] = (float)lp;
    }
}


static __global__ __launch_bounds__(PPO_THREADS) void ppo_forward_kernel(PpoNet n, const float* __restrict__ params,
                                                                        const float* __restrict__ obs,
                                                                        const float* __restrict__ eps, int rows, int value_only,
                                                                        float* __restrict__ action_out,
                                                                        float* __restrict__ logprob_out,
                                                                        float* __restrict__ value_out) {
    __shared__ PpoLds L;
    ppo_forward_tile(L, n, (int)blockIdx.x, params, obs, eps, rows, value_only, action_out, logprob_out, value_out);
}

// One launch for a population: blockIdx.y is the learner, a chunk of at most PPO_POP_CHUNK of them.  The records travel BY VALUE
// in the kernel argument, so a launch that is still queued keeps its own copy whatever the host does next.
constexpr int PPO_POP_CHUNK = 16;
struct PpoFwdLearner {
    const float *params, *obs, *eps;
    float *action_out, *logprob_out, *value_out;
};
struct PpoPopFwdArgs {
    PpoNet n;
    int rows, value_only;
    PpoFwdLearner l[PPO_POP_CHUNK];
};
static __global__ __launch_bounds__(PPO_THREADS) void ppo_pop_forward_kernel(PpoPopFwdArgs a) {
    __shared__ PpoLds L;
    const PpoFwdLearner& l = a.l[blockIdx.y];
    ppo_forward_tile(L, a.n, (int)blockIdx.x, l.params, l.obs, l.eps, a.rows, a.value_only, l.action_out, l.logprob_out, l.value_out);
}

// ---------------------------------------------------------------------------------------------------------------------
// rollout table: one row per (step, env):  obs [D] | action [A] | old log-prob | scalarised advantage | returns [R] | old values [R]
// ---------------------------------------------------------------------------------------------------------------------
static __global__ __launch_bounds__(256) void ppo_pack_kernel(int D, int A, int R, int row_w, int rows,
                                                              const float* __restrict__ obs, const float* __restrict__ actions,
                                                              const float* __restrict__ logprobs, const float* __restrict__ values,
                                                              float* __restrict__ table) {
    const long long total = (long long)rows * row_w;
    for (long long o = (long long)blockIdx.x * blockDim.x + threadIdx.x; o < total; o += (long long)gridDim.x * blockDim.x) {
        const int row = (int)(o / row_w), c = (int)(o - (long long)row * row_w);
        float v = 0.0f;                                         // advantage and returns: written by ppo_gae_kernel
        if (c < D) v = obs[(size_t)row * D + c];
        else if (c < D + A) v = actions[(size_t)row * A + (c - D)];
        else if (c == D + A) v = logprobs[row];
        else if (c >= D + A + 2 + R) v = values[(size_t)row * R + (c - (D + A + 2 + R))];
        table[o] = v;
    }
}

// __compute_advantages: one work-item per env runs the reverse scan of all its objectives
//   gae:  delta = r + gamma * next_v * nonterminal - v;  last = delta + (gamma * gae_lambda) * nonterminal * last;  returns = last + v
//   else: returns = r + gamma * nonterminal * next_return;  advantage = returns - v
// and scalarises: advantages @ weights, summed over the objectives in index order
__device__ __forceinline__ void ppo_gae_scan(int T, int E, int R, int row_w, int adv_col, float* __restrict__ table,
                                             const float* __restrict__ rewards, const float* __restrict__ dones,
                                             const float* __restrict__ next_value, const float* __restrict__ next_done,
                                             const float* __restrict__ weights, float gamma, float gamma_lambda, int use_gae,
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
        float* trow = table + row * row_w + adv_col;          // advantage | returns [R] | values [R]
        float s = 0.0f;
#pragma unroll
        for (int k = 0; k < PPO_MAX_R; ++k) {
            if (k < R) {
                const float r = rewards[row * R + k], v = trow[1 + R + k];
                float adv, ret;
                if (use_gae) {
                    const float delta = __fsub_rn(__fadd_rn(r, __fmul_rn(__fmul_rn(gamma, nextv[k]), nonterminal)), v);
                    adv = __fadd_rn(delta, __fmul_rn(__fmul_rn(gamma_lambda, nonterminal), carry[k]));
                    carry[k] = adv;
                    ret = __fadd_rn(adv, v);
                    nextv[k] = v;
                } else {
                    const float nr = (t == T - 1) ? nextv[k] : carry[k];
                    ret = __fadd_rn(r, __fmul_rn(__fmul_rn(gamma, nonterminal), nr));
                    carry[k] = ret;
                    adv = __fsub_rn(ret, v);
                }
                trow[1 + k] = ret;
                if (returns_out != nullptr) returns_out[row * R + k] = ret;
                s = __fadd_rn(s, __fmul_rn(adv, weights[k]));
            }
        }
        trow[0] = s;
        if (adv_out != nullptr) adv_out[row] = s;
        nonterminal = __fsub_rn(1.0f, dones[row]);            // what step t - 1 sees as its successor's done flag
    }
}


static __global__ __launch_bounds__(64) void ppo_gae_kernel(int T, int E, int R, int row_w, int adv_col, float* __restrict__ table,
                                                            const float* __restrict__ rewards, const float* __restrict__ dones,
                                                            const float* __restrict__ next_value, const float* __restrict__ next_done,
                                                            const float* __restrict__ weights, float gamma, float gamma_lambda,
                                                            int use_gae, float* __restrict__ returns_out, float* __restrict__ adv_out) {
    ppo_gae_scan(T, E, R, row_w, adv_col, table, rewards, dones, next_value, next_done, weights, gamma, gamma_lambda, use_gae,
                 returns_out, adv_out);
}

struct PpoGaeLearner {
    float* table;
    const float *rewards, *dones, *next_value, *next_done, *weights;
    float *returns_out, *adv_out;
};
struct PpoPopGaeArgs {
    int T, E, R, row_w, adv_col, use_gae;
    float gamma, gamma_lambda;
    PpoGaeLearner l[PPO_POP_CHUNK];
};
static __global__ __launch_bounds__(64) void ppo_pop_gae_kernel(PpoPopGaeArgs a) {
    const PpoGaeLearner& l = a.l[blockIdx.y];
    ppo_gae_scan(a.T, a.E, a.R, a.row_w, a.adv_col, l.table, l.rewards, l.dones, l.next_value, l.next_done, l.weights, a.gamma,
                 a.gamma_lambda, a.use_gae, l.returns_out, l.adv_out);
}

// ---------------------------------------------------------------------------------------------------------------------
// one minibatch step
// ---------------------------------------------------------------------------------------------------------------------
struct PpoStepArgs {
    PpoNet n;
    float* params;                 // [P]  read by every tile, stepped by the last workgroup
    float* exp_avg;                // [P]
    float* exp_avg_sq;             // [P]
    const float* table;            // [table_rows][row_w]
    int table_rows, row_w;
    const int* idx;                // [M] rows of the table, this step's minibatch
    int M, ntiles;
    float* part;                   // [ntiles][P] gradient partials
    float* lpart;                  // [ntiles][PPO_NPART] loss partial sums
    unsigned int* ticket;          // arrival counter, zero between launches
    float* stats_out;              // [PPO_NSTATS]
    float clip_lo, clip_hi, clip_coef, ent_coef, vf_coef, max_grad_norm;
    int clip_vloss, norm_adv;
    float inv_M, inv_MR, inv_Mm1, fM, fMR;    // fM = M, fMR = M * R: a mean is a sum DIVIDED by its count, as torch forms it
    float one_minus_b1, b2, one_minus_b2, neg_step_size, bc2_sqrt, eps;
};

// what differs between the learners of a population; everything else of PpoStepArgs is shared
struct PpoLearner {
    float *params, *exp_avg, *exp_avg_sq;
    const float* table;
    const int* idx;
    float *part, *lpart;
    unsigned int* ticket;
    float* stats_out;
    int table_rows;
    float neg_step_size, bc2_sqrt;
};

// a single learner's record: the per-learner fields of its own argument block
__device__ __forceinline__ PpoLearner ppo_own_learner(const PpoStepArgs& a) {
    return PpoLearner{a.params, a.exp_avg, a.exp_avg_sq, a.table, a.idx, a.part, a.lpart, a.ticket, a.stats_out, a.table_rows,
                      a.neg_step_size, a.bc2_sqrt};
}

// the table row of minibatch entry b, clamped into the table
__device__ __forceinline__ int ppo_table_row(const int* __restrict__ idx, int b, int table_rows) {
    return min(max(idx[b], 0), table_rows - 1);
}

// The value loss (mo_ppo.py:535-547, nl_mo_ppo.py:378-385) of row r of the tile, from the critic's output in L.out, L.ret and
// L.oldv: writes the row's d loss / d value to L.dout and returns the row's sum over the objectives of max(unclipped, clipped)
// squares (or of the unclipped square alone), 0 for a row past the minibatch.
__device__ __forceinline__ float ppo_value_loss_row(PpoLds& L, const PpoStepArgs& a, int r, int valid) {
    const int R = a.n.R;
    float vsum = 0.0f;
    const float gscale = __fmul_rn(__fmul_rn(0.5f, a.vf_coef), a.inv_MR);
    for (int k = 0; k < R; ++k) {
        const float v = L.out[r * R + k], ret = L.ret[r * R + k], ov = L.oldv[r * R + k];
        float g = 0.0f;
        if (r < valid) {
            const float du = __fsub_rn(v, ret);
            const float u = __fmul_rn(du, du);
            g = __fmul_rn(2.0f, du);
            float m = u;
            if (a.clip_vloss) {
                const float dv = __fsub_rn(v, ov);
                const float vc = __fadd_rn(ov, fminf(fmaxf(dv, -a.clip_coef), a.clip_coef));
                const float dc = __fsub_rn(vc, ret);
                const float cl = __fmul_rn(dc, dc);
                m = fmaxf(u, cl);
                // inside the range both branches have the derivative 2 (v - ret); outside, the clipped branch has none
                const bool inside = dv >= -a.clip_coef && dv <= a.clip_coef;
                if (!inside) g = (u > cl) ? g : ((u == cl) ? du : 0.0f);
            }
            vsum = __fadd_rn(vsum, m);
        }
        L.dout[r * R + k] = __fmul_rn(g, gscale);
    }
    return vsum;
}

// The last workgroup's reduction: the gradient partials summed in tile order (four loads in flight, added in order) into tile
// 0's slot, and clip_grad_norm_ (mo_ppo.py:553, nl_mo_ppo.py:392): the 2-norm of the per-tensor 2-norms; scale = max_norm /
// (total + 1e-6) clamped to 1.  With `logstd`, tensor 0 is actor_logstd and takes the entropy's share, -ent_coef per entry.
// Work-item 0 writes L.stat[2] = scale and L.stat[3] = total and returns the total norm (the others return 0); there is NO
// barrier after that: the caller's work-item 0 writes its statistics and re-arms the ticket, then the barrier, then
// ppo_adam_sweep.
__device__ __forceinline__ float ppo_grad_clip(PpoLds& L, const PpoStepArgs& a, const PpoLearner& l, bool logstd) {
    const PpoNet& n = a.n;
    const int tid = (int)threadIdx.x;
    for (int t = 0; t < n.ntensors; ++t) {
        float sq = 0.0f;
        for (int q = n.tstart[t] + tid; q < n.tstart[t + 1]; q += PPO_THREADS) {
            float g = l.part[q];
            int tl = 1;
            for (; tl + 4 <= a.ntiles; tl += 4) {
                const float g0 = l.part[(size_t)tl * n.P + q], g1 = l.part[(size_t)(tl + 1) * n.P + q];
                const float g2 = l.part[(size_t)(tl + 2) * n.P + q], g3 = l.part[(size_t)(tl + 3) * n.P + q];
                g = __fadd_rn(__fadd_rn(__fadd_rn(__fadd_rn(g, g0), g1), g2), g3);
            }
            for (; tl < a.ntiles; ++tl) g = __fadd_rn(g, l.part[(size_t)tl * n.P + q]);
            if (logstd && t == 0) g = __fsub_rn(g, a.ent_coef);      // d(-ent_coef * entropy) / d logstd_k
            l.part[q] = g;
            sq = fmaf(g, g, sq);
        }
        L.w[t * PPO_THREADS + tid] = sq;
    }
    __syncthreads();
    if (tid < n.ntensors) {
        float s = 0.0f;
        for (int i = 0; i < PPO_THREADS; ++i) s = __fadd_rn(s, L.w[tid * PPO_THREADS + i]);
        L.red[tid] = __fsqrt_rn(s);
    }
    __syncthreads();
    float total = 0.0f;
    if (tid == 0) {
        float s = 0.0f;
        for (int t = 0; t < n.ntensors; ++t) s = fmaf(L.red[t], L.red[t], s);
        total = __fsqrt_rn(s);
        L.stat[2] = fminf(__fdiv_rn(a.max_grad_norm, __fadd_rn(total, 1e-6f)), 1.0f);
        L.stat[3] = total;
    }
    return total;
}

// the clipped gradient (tile 0's slot times L.stat[2]) through torch _single_tensor_adam with eps 1e-5 (mo_ppo.py:331, 554)
__device__ __forceinline__ void ppo_adam_sweep(const PpoLds& L, const PpoStepArgs& a, const PpoLearner& l) {
    const float scale = L.stat[2];
    for (int q = (int)threadIdx.x; q < a.n.P; q += PPO_THREADS)
        pcn_adam(__fmul_rn(l.part[q], scale), l.params[q], l.exp_avg[q], l.exp_avg_sq[q], a.one_minus_b1, a.b2, a.one_minus_b2,
                 l.neg_step_size, l.bc2_sqrt, a.eps);
}

// the body of ppo_step_kernel / ppo_pop_step_kernel: tile `tile` of learner `l`'s minibatch.  The shared fields are read from
// `a`, the per-learner ones from `l` only.
__device__ __forceinline__ void ppo_step_tile(PpoLds& L, const PpoStepArgs& a, const PpoLearner& l, int tile) {
    const PpoNet& n = a.n;
    const int tid = (int)threadIdx.x, row0 = tile * PPO_TB;
    const int valid = min(PPO_TB, a.M - row0);
    const float* p = l.params;
    const int ao = n.D, lo = n.D + n.A, adv_col = lo + 1, ro = lo + 2, vo = ro + n.R;

    // ---- gather (mo_ppo.py:509-511): table row idx[b] -> observation, action, old log-prob, advantage, returns, old values
    for (int o = tid; o < PPO_TB * n.D; o += PPO_THREADS) {
        const int r = o / n.D, d = o - r * n.D;
        float v = 0.0f;
        if (r < valid) {
            const int row = ppo_table_row(l.idx, row0 + r, l.table_rows);
            v = l.table[(size_t)row * a.row_w + d];
        }
        L.x[o] = v;
    }
    for (int o = tid; o < PPO_TB * n.A; o += PPO_THREADS) {
        const int r = o / n.A, k = o - r * n.A;
        float v = 0.0f;
        if (r < valid) {
            const int row = ppo_table_row(l.idx, row0 + r, l.table_rows);
            v = l.table[(size_t)row * a.row_w + ao + k];
        }
        L.act[o] = v;
    }
    for (int o = tid; o < PPO_TB * n.R; o += PPO_THREADS) {
        const int r = o / n.R, k = o - r * n.R;
        float ret = 0.0f, ov = 0.0f;
        if (r < valid) {
            const int row = ppo_table_row(l.idx, row0 + r, l.table_rows);
            ret = l.table[(size_t)row * a.row_w + ro + k];
            ov = l.table[(size_t)row * a.row_w + vo + k];
        }
        L.ret[o] = ret;
        L.oldv[o] = ov;
    }
    if (tid < PPO_TB) {
        float lp = 0.0f, adv = 0.0f;
        if (tid < valid) {
            const int row = ppo_table_row(l.idx, row0 + tid, l.table_rows);
            lp = l.table[(size_t)row * a.row_w + lo];
            adv = l.table[(size_t)row * a.row_w + adv_col];
        }
        L.row[tid * 4] = lp;
        L.row[tid * 4 + 1] = adv;
    }

    // ---- advantage normalisation (mo_ppo.py:527-528): mean and unbiased std of all M advantages, read in minibatch order and
    // reduced by the same tree in every workgroup
    if (a.norm_adv) {
        float s = 0.0f;
        for (int b = tid; b < a.M; b += PPO_THREADS) {
            const int row = ppo_table_row(l.idx, b, l.table_rows);
            s = __fadd_rn(s, l.table[(size_t)row * a.row_w + adv_col]);
        }
        const float mean = __fdiv_rn(ppo_tree_sum(L.red, s), a.fM);
        float q = 0.0f;
        for (int b = tid; b < a.M; b += PPO_THREADS) {
            const int row = ppo_table_row(l.idx, b, l.table_rows);
            const float dlt = __fsub_rn(l.table[(size_t)row * a.row_w + adv_col], mean);
            q = fmaf(dlt, dlt, q);
        }
        const float var = __fmul_rn(ppo_tree_sum(L.red, q), a.inv_Mm1);
        if (tid == 0) {
            L.stat[0] = mean;
            L.stat[1] = __fadd_rn(__fsqrt_rn(var), 1e-8f);
        }
    }
    __syncthreads();

    float* part = l.part + (size_t)tile * n.P;

    // ---- critic: forward, value loss (mo_ppo.py:535-547) and its gradient, backward
    ppo_mlp_forward(L, n, n.c, p, n.R);
    if (tid < PPO_TB) L.rs[tid * PPO_NPART + 1] = ppo_value_loss_row(L, a, tid, valid);
    __syncthreads();
    ppo_mlp_backward(L, n, n.c, p, part, n.R);

    // ---- actor: forward, log-prob, ratio, policy loss (mo_ppo.py:513-533) and its gradient, backward
    ppo_mlp_forward(L, n, n.a, p, n.A);
    if (tid < PPO_TB) {
        const int r = tid;
        float pg = 0.0f, nlr = 0.0f, kl = 0.0f, cf = 0.0f, dlp = 0.0f;
        if (r < valid) {
            double lp = 0.0;
            for (int k = 0; k < n.A; ++k) {
                const float sd = expf(p[n.oLs + k]);
                const float diff = __fsub_rn(L.act[r * n.A + k], L.out[r * n.A + k]);
                const float t = __fdiv_rn(-__fmul_rn(diff, diff), __fmul_rn(2.0f, __fmul_rn(sd, sd)));
                lp = ppo_logprob_add(lp, t, sd);
            }
            const float logratio = __fsub_rn((float)lp, L.row[r * 4]);
            const float ratio = expf(logratio);
            float adv = L.row[r * 4 + 1];
            if (a.norm_adv) adv = __fdiv_rn(__fsub_rn(adv, L.stat[0]), L.stat[1]);
            const float pg1 = __fmul_rn(-adv, ratio);
            const float pg2 = __fmul_rn(-adv, fminf(fmaxf(ratio, a.clip_lo), a.clip_hi));
            pg = fmaxf(pg1, pg2);
            // torch.max splits a tie evenly: inside the clip range both branches are the same number with the derivative -adv;
            // outside, the clipped branch has none
            const bool inside = ratio >= a.clip_lo && ratio <= a.clip_hi;
            const float dratio = (inside || pg1 > pg2) ? -adv : 0.0f;
            dlp = __fmul_rn(__fmul_rn(dratio, ratio), a.inv_M);
            nlr = -logratio;
            kl = __fsub_rn(__fsub_rn(ratio, 1.0f), logratio);
            cf = (fabsf(__fsub_rn(ratio, 1.0f)) > a.clip_coef) ? 1.0f : 0.0f;
        }
        L.row[r * 4 + 2] = dlp;
        L.rs[r * PPO_NPART] = pg;
        L.rs[r * PPO_NPART + 2] = nlr;
        L.rs[r * PPO_NPART + 3] = kl;
        L.rs[r * PPO_NPART + 4] = cf;
    }
    __syncthreads();
    // d newlogprob / d mean_k = (action - mean) / var;  d / d logstd_k = (action - mean)^2 / var - 1
    for (int o = tid; o < PPO_TB * n.A; o += PPO_THREADS) {
        const int r = o / n.A, k = o - r * n.A;
        const float sd = expf(p[n.oLs + k]);
        const float var = __fmul_rn(sd, sd);
        const float diff = __fsub_rn(L.act[o], L.out[o]);
        const float dlp = L.row[r * 4 + 2];
        L.dout[o] = __fmul_rn(dlp, __fdiv_rn(diff, var));
        L.act[o] = __fmul_rn(dlp, __fsub_rn(__fdiv_rn(__fmul_rn(diff, diff), var), 1.0f));
    }
    __syncthreads();
    pcn_db(part + n.oLs, L.act, n.A, n.A);            // (the entropy's share, -ent_coef per entry, is added once by the last workgroup)
    if (tid < PPO_NPART) {
        float s = 0.0f;
        for (int r = 0; r < PPO_TB; ++r) s = __fadd_rn(s, L.rs[r * PPO_NPART + tid]);
        l.lpart[tile * PPO_NPART + tid] = s;
    }
    ppo_mlp_backward(L, n, n.a, p, part, n.A);

    // ---- the last workgroup to arrive owns the step
    if (!pcn_last_arrival(l.ticket, a.ntiles, L.last)) return;
    const float total = ppo_grad_clip(L, a, l, true);
    if (tid == 0) {
        *l.ticket = 0u;                                        // re-armed for the next launch on the stream
        float ls[PPO_NPART];
        for (int i = 0; i < PPO_NPART; ++i) ls[i] = 0.0f;
        for (int t = 0; t < a.ntiles; ++t)
            for (int i = 0; i < PPO_NPART; ++i) ls[i] = __fadd_rn(ls[i], l.lpart[t * PPO_NPART + i]);
        float ent = 0.0f;                                      // Normal.entropy(): 0.5 + 0.5 log(2 pi) + log(scale), the same in every row
        for (int k = 0; k < n.A; ++k) ent = __fadd_rn(ent, __fadd_rn(__fadd_rn(0.5f, PPO_HALF_LOG_2PI), logf(expf(p[n.oLs + k]))));
        const float pg = __fdiv_rn(ls[0], a.fM), v = __fmul_rn(0.5f, __fdiv_rn(ls[1], a.fMR));
        l.stats_out[0] = __fadd_rn(__fsub_rn(pg, __fmul_rn(a.ent_coef, ent)), __fmul_rn(v, a.vf_coef));
        l.stats_out[1] = pg;
        l.stats_out[2] = v;
        l.stats_out[3] = ent;
        l.stats_out[4] = __fdiv_rn(ls[2], a.fM);
        l.stats_out[5] = __fdiv_rn(ls[3], a.fM);
        l.stats_out[6] = __fdiv_rn(ls[4], a.fM);
        l.stats_out[7] = total;
    }
    __syncthreads();
    ppo_adam_sweep(L, a, l);
}


static __global__ __launch_bounds__(PPO_THREADS) void ppo_step_kernel(PpoStepArgs a) {
    __shared__ PpoLds L;
    ppo_step_tile(L, a, ppo_own_learner(a), (int)blockIdx.x);
}

// blockIdx.y is the learner: its own parameters, moments, table, idx, partials, ticket, statistics row and Adam scalars.  The
// last workgroup to arrive FOR THAT LEARNER (its ticket counts to ntiles) owns that learner's step; nothing crosses learners.
struct PpoPopStepArgs {
    PpoStepArgs s;                      // the shared fields; its per-learner fields are not read
    PpoLearner l[PPO_POP_CHUNK];
};
static_assert(sizeof(PpoPopStepArgs) <= 4096 && sizeof(PpoPopFwdArgs) <= 4096 && sizeof(PpoPopGaeArgs) <= 4096,
              "population records travel in the kernel argument");
static __global__ __launch_bounds__(PPO_THREADS) void ppo_pop_step_kernel(PpoPopStepArgs a) {
    __shared__ PpoLds L;
    ppo_step_tile(L, a.s, a.l[blockIdx.y], (int)blockIdx.x);
}

}  // namespace morl
