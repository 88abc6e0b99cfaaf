// Pareto Conditioned Networks (multi_policy/pcn/pcn.py): the whole optimiser step of PCN.update() (pcn.py:202-236) as ONE launch,
// and the no-grad forward of PCN._act (pcn.py:302-322) as one launch.  fp32 throughout.
//
//   c = cat(desired_return, desired_horizon) * scaling_factor      (pcn.py:65-67)
//   s = sigmoid(Ws x + bs),  e = sigmoid(Wc c + bc)                (pcn.py:68-69, s_emb / c_emb)
//   h = relu(W1 (s o e) + b1),  out = W2 h + b2                    (pcn.py:71, fc)      [+ log_softmax: discrete model, pcn.py:87]
//   loss = mean_b(-logp[b, a_b])  |  mean over B*A of (a - out)^2  (pcn.py:225-232)
//   Adam, torch defaults (pcn.py:181, 234); scaling_factor is frozen (pcn.py:60)
//
// Structure.  A workgroup owns PCN_TB = 16 rows of the batch: it gathers them from the device-resident transition table, runs
// forward and backward with every activation in LDS, and writes its share of the weight gradient -- a full-length partial -- to
// part[tile][P].  The workgroups then take a ticket from an integer counter; the one that draws the last ticket sums the partials
// IN TILE ORDER (the same bits on every run: no floating-point atomics anywhere), applies Adam, reduces the loss and re-arms the
// counter.  Nobody waits for anybody: there is no grid barrier, so a workgroup that is scheduled late only delays the step.
// The batch is 256 rows and the widest layer 64 x 64 in the reference's configuration (16 workgroups, ~10 MFLOP per step):
// the step is bound by launch and by the dependent LDS / L2 round trips of six small layers, not by arithmetic, so the
// matrix products are plain VALU FMAs out of LDS ("PCN").
#pragma once
#include "morl_device.h"

namespace morl {

constexpr int PCN_THREADS = 256;
constexpr int PCN_TB = 16;            // batch rows per workgroup
constexpr int PCN_KC = 32;            // columns of a weight matrix staged in LDS at a time
constexpr int PCN_WLD = PCN_KC + 1;   // row stride of the staged chunk (odd: lanes that differ in the row hit different banks)
constexpr int PCN_MAX_H = 128;        // hidden_dim (a multiple of 32)
constexpr int PCN_MAX_D = 128;        // state_dim
constexpr int PCN_MAX_A = 32;         // action_dim
constexpr int PCN_MAX_R = 8;          // reward_dim (MORL_MAX_OBJ)
constexpr int PCN_CLD = 12;           // row stride of the command rows (reward_dim + 1 <= 9)

// the model as a map into the flat parameter vector: s_emb.0, c_emb.0, fc.0, fc.2 -- each weight before its bias (the order of
// model.parameters() minus the frozen scaling_factor)
struct PcnNet {
    int D, R, A, H, C;        // C = R + 1 command inputs
    int continuous;           // 0: log_softmax head + cross entropy, 1: linear head + MSE
    int oWs, obs, oWc, obc, oW1, ob1, oW2, ob2, P;
};

struct PcnLds {
    float w[PCN_MAX_H * PCN_WLD];     // staged weight chunk [N][PCN_KC]
    float x[PCN_TB * PCN_MAX_D];      // observations
    float c[PCN_TB * PCN_CLD];        // scaled commands
    float s[PCN_TB * PCN_MAX_H];      // sigmoid(s_emb)
    float e[PCN_TB * PCN_MAX_H];      // sigmoid(c_emb)
    float g[PCN_TB * PCN_MAX_H];      // s o e; backward: d/d(s_emb pre-activation)
    float h[PCN_TB * PCN_MAX_H];      // relu(fc.0); backward: d/d(fc.0 pre-activation), then d/d(c_emb pre-activation)
    float out[PCN_TB * PCN_MAX_A];    // prediction
    float dout[PCN_TB * PCN_MAX_A];   // d loss / d(fc.2 output)
    float act[PCN_TB * PCN_MAX_A];    // the stored action (discrete: its index in column 0)
    float red[2 * PCN_TB];
    int last;
};
static_assert(sizeof(PcnLds) <= 64 * 1024, "PCN tile state must fit 64 KB of static LDS");

// z[r][j] = b[j] + sum_k W[j][k] xin[r][k] for the 16 rows of the tile.  W ([N][K] row-major, global) goes through LDS in chunks
// of PCN_KC columns; a work-item owns column j of four rows, so one weight read feeds four FMAs.  Products are accumulated in k
// order on top of the bias.  Ends with a barrier: z is complete and L.w is free.
__device__ __forceinline__ void pcn_dense(float* sw, const float* __restrict__ W, const float* __restrict__ b, int N, int K,
                                          const float* xin, int ldx, float* z, int ldz) {
    const int tid = (int)threadIdx.x;
    for (int k0 = 0; k0 < K; k0 += PCN_KC) {
        const int kc = min(PCN_KC, K - k0);
        __syncthreads();
        for (int o = tid; o < N * kc; o += PCN_THREADS) {
            const int j = o / kc, kk = o - j * kc;
            sw[j * PCN_WLD + kk] = W[(size_t)j * K + k0 + kk];
        }
        __syncthreads();
        for (int o = tid; o < 4 * N; o += PCN_THREADS) {
            const int rg = o / N, j = o - rg * N;
            float acc[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) acc[u] = (k0 == 0) ? b[j] : z[(rg * 4 + u) * ldz + j];
            for (int kk = 0; kk < kc; ++kk) {
                const float w = sw[j * PCN_WLD + kk];
#pragma unroll
                for (int u = 0; u < 4; ++u) acc[u] = fmaf(w, xin[(rg * 4 + u) * ldx + k0 + kk], acc[u]);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) z[(rg * 4 + u) * ldz + j] = acc[u];
        }
    }
    __syncthreads();
}

__device__ __forceinline__ float pcn_sigmoid(float z) { return __fdiv_rn(1.0f, __fadd_rn(1.0f, expf(-z))); }

// forward of the tile whose inputs are in L.x / L.c: leaves s, e, s o e (L.g), relu(fc.0) (L.h) and the prediction (L.out)
__device__ __forceinline__ void pcn_tile_forward(PcnLds& L, const PcnNet& n, const float* __restrict__ p) {
    const int tid = (int)threadIdx.x, H = n.H;
    pcn_dense(L.w, p + n.oWs, p + n.obs, H, n.D, L.x, n.D, L.s, H);
    pcn_dense(L.w, p + n.oWc, p + n.obc, H, n.C, L.c, PCN_CLD, L.e, H);
    for (int o = tid; o < PCN_TB * H; o += PCN_THREADS) {
        const float s = pcn_sigmoid(L.s[o]), e = pcn_sigmoid(L.e[o]);
        L.s[o] = s;
        L.e[o] = e;
        L.g[o] = __fmul_rn(s, e);
    }
    pcn_dense(L.w, p + n.oW1, p + n.ob1, H, H, L.g, H, L.h, H);
    for (int o = tid; o < PCN_TB * H; o += PCN_THREADS) L.h[o] = fmaxf(L.h[o], 0.0f);
    pcn_dense(L.w, p + n.oW2, p + n.ob2, n.A, H, L.h, H, L.out, n.A);
    if (!n.continuous) {
        if (tid < PCN_TB) {                       // log_softmax over the actions of row tid
            float* z = L.out + tid * n.A;
            float m = z[0];
            for (int a = 1; a < n.A; ++a) m = fmaxf(m, z[a]);
            float sum = 0.0f;
            for (int a = 0; a < n.A; ++a) sum += expf(z[a] - m);
            const float lse = logf(sum);
            for (int a = 0; a < n.A; ++a) z[a] = (z[a] - m) - lse;
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// no-grad forward: out[rows][A] = model(obs, desired_return, desired_horizon)
// ---------------------------------------------------------------------------------------------------------------------
static __global__ __launch_bounds__(PCN_THREADS) void pcn_forward_kernel(PcnNet n, const float* __restrict__ params,
                                                                        const float* __restrict__ scaling,
                                                                        const float* __restrict__ obs,
                                                                        const float* __restrict__ desired_return,
                                                                        const float* __restrict__ desired_horizon, int rows,
                                                                        float* __restrict__ out) {
    __shared__ PcnLds L;
    const int tid = (int)threadIdx.x, row0 = (int)blockIdx.x * PCN_TB;
    for (int o = tid; o < PCN_TB * n.D; o += PCN_THREADS) {
        const int r = o / n.D, d = o - r * n.D;
        L.x[o] = (row0 + r < rows) ? obs[(size_t)(row0 + r) * n.D + d] : 0.0f;
    }
    for (int o = tid; o < PCN_TB * n.C; o += PCN_THREADS) {
        const int r = o / n.C, k = o - r * n.C;
        float v = 0.0f;
        if (row0 + r < rows) v = (k < n.R) ? desired_return[(size_t)(row0 + r) * n.R + k] : desired_horizon[row0 + r];
        L.c[r * PCN_CLD + k] = __fmul_rn(v, scaling[k]);
    }
    pcn_tile_forward(L, n, params);
    for (int o = tid; o < PCN_TB * n.A; o += PCN_THREADS) {
        const int r = o / n.A;
        if (row0 + r < rows) out[(size_t)row0 * n.A + o] = L.out[o];
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// one optimiser step
// ---------------------------------------------------------------------------------------------------------------------
struct PcnStepArgs {
    PcnNet n;
    float* params;                 // [P]  read by every tile, stepped by the last workgroup
    float* exp_avg;                // [P]
    float* exp_avg_sq;             // [P]
    const float* scaling;          // [C]
    const float* table;            // [table_rows][row_w]: obs | action | return-to-go | steps left
    int table_rows, row_w, act_w;  // act_w: 1 (the action's index) or A
    const int* idx;                // [B] rows of the table, this step's batch
    int B, ntiles;
    float* part;                   // [ntiles][P] weight-gradient partials
    float* lpart;                  // [ntiles][2] loss / entropy partial sums
    unsigned int* ticket;          // arrival counter, zero between launches
    float* loss_out;               // this step's loss
    float* ent_out;                // this step's sum_b sum_a -p log p (discrete), or NULL
    float* pred_out;               // [B][A] predictions of this step, or NULL
    float inv_count;               // 1 / B (discrete), 1 / (B * A) (continuous)
    float one_minus_b1, b2, one_minus_b2, neg_step_size, bc2_sqrt, eps;
};

// part[o] = sum_r dz[r][j] * a[r][k] over the tile's rows in row order, o = j * K + k (the layout of the weight itself)
__device__ __forceinline__ void pcn_dw(float* __restrict__ dst, const float* dz, int ldz, const float* a, int lda, int N, int K) {
    for (int o = (int)threadIdx.x; o < N * K; o += PCN_THREADS) {
        const int j = o / K, k = o - j * K;
        float acc = 0.0f;
#pragma unroll
        for (int r = 0; r < PCN_TB; ++r) acc = fmaf(dz[r * ldz + j], a[r * lda + k], acc);
        dst[o] = acc;
    }
}
__device__ __forceinline__ void pcn_db(float* __restrict__ dst, const float* dz, int ldz, int N) {
    for (int j = (int)threadIdx.x; j < N; j += PCN_THREADS) {
        float acc = 0.0f;
#pragma unroll
        for (int r = 0; r < PCN_TB; ++r) acc += dz[r * ldz + j];
        dst[j] = acc;
    }
}

// The ticket (shared with ppo_kernels.h / nlppo_kernels.h): a workgroup fences what it wrote, work-item 0 draws a ticket and tells
// the others through LDS (`last`) whether it was the last of `ntiles`.  True in every work-item of that one workgroup, which has
// fenced again and may read what the others wrote; whoever re-arms the ticket is its caller.
__device__ __forceinline__ bool pcn_last_arrival(unsigned int* ticket, int ntiles, int& last) {
    __threadfence();
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned int prev = atomicAdd(ticket, 1u);
        last = (prev + 1u == (unsigned int)ntiles) ? 1 : 0;
    }
    __syncthreads();
    if (!last) return false;
    __threadfence();
    return true;
}

// torch _single_tensor_adam on one element with the gradient g: lerp_, mul_ + addcmul_, addcdiv_ -- the operation order of
// optim_kernels.h.  neg_step_size = -lr / (1 - b1^t) and bc2_sqrt = sqrt(1 - b2^t) are formed on the host in float64.
__device__ __forceinline__ void pcn_adam(float g, float& param, float& exp_avg, float& exp_avg_sq, float one_minus_b1, float b2,
                                         float one_minus_b2, float neg_step_size, float bc2_sqrt, float eps) {
    float m = exp_avg, v = exp_avg_sq;
    m = fmaf(one_minus_b1, __fsub_rn(g, m), m);
    v = __fadd_rn(__fmul_rn(v, b2), __fmul_rn(__fmul_rn(one_minus_b2, g), g));
    const float denom = __fadd_rn(__fdiv_rn(__fsqrt_rn(v), bc2_sqrt), eps);
    param = __fadd_rn(param, __fmul_rn(neg_step_size, __fdiv_rn(m, denom)));
    exp_avg = m;
    exp_avg_sq = v;
}

static __global__ __launch_bounds__(PCN_THREADS) void pcn_step_kernel(PcnStepArgs a) {
    __shared__ PcnLds L;
    const PcnNet& n = a.n;
    const int tid = (int)threadIdx.x, tile = (int)blockIdx.x, row0 = tile * PCN_TB, H = n.H;
    const int valid = min(PCN_TB, a.B - row0);
    const float* p = a.params;

    // ---- gather (pcn.py:206-222): table row idx[b] -> observation, action, scaled command
    const int ao = n.D, ro = n.D + a.act_w;
    for (int o = tid; o < PCN_TB * n.D; o += PCN_THREADS) {
        const int r = o / n.D, d = o - r * n.D;
        float v = 0.0f;
        if (r < valid) {
            const int row = min(max(a.idx[row0 + r], 0), a.table_rows - 1);
            v = a.table[(size_t)row * a.row_w + d];
        }
        L.x[o] = v;
    }
    for (int o = tid; o < PCN_TB * n.C; o += PCN_THREADS) {
        const int r = o / n.C, k = o - r * n.C;
        float v = 0.0f;
        if (r < valid) {
            const int row = min(max(a.idx[row0 + r], 0), a.table_rows - 1);
            v = a.table[(size_t)row * a.row_w + ro + k];
        }
        L.c[r * PCN_CLD + k] = __fmul_rn(v, a.scaling[k]);
    }
    for (int o = tid; o < PCN_TB * a.act_w; o += PCN_THREADS) {
        const int r = o / a.act_w, k = o - r * a.act_w;
        float v = 0.0f;
        if (r < valid) {
            const int row = min(max(a.idx[row0 + r], 0), a.table_rows - 1);
            v = a.table[(size_t)row * a.row_w + ao + k];
        }
        L.act[r * PCN_MAX_A + k] = v;
    }

    pcn_tile_forward(L, n, p);

    // ---- loss and its gradient at the head's output (pcn.py:225-232)
    if (tid < PCN_TB) {
        const int r = tid;
        float loss = 0.0f, ent = 0.0f;
        const float* z = L.out + r * n.A;
        float* dz = L.dout + r * n.A;
        if (r >= valid) {
            for (int k = 0; k < n.A; ++k) dz[k] = 0.0f;
        } else if (n.continuous) {
            for (int k = 0; k < n.A; ++k) {
                const float diff = __fsub_rn(z[k], L.act[r * PCN_MAX_A + k]);
                loss = fmaf(diff, diff, loss);
                dz[k] = __fmul_rn(__fmul_rn(2.0f, diff), a.inv_count);
            }
        } else {
            const int ab = min(max((int)L.act[r * PCN_MAX_A], 0), n.A - 1);
            for (int k = 0; k < n.A; ++k) {
                const float pk = expf(z[k]);
                ent = __fsub_rn(ent, __fmul_rn(pk, z[k]));
                dz[k] = __fmul_rn(__fsub_rn(pk, k == ab ? 1.0f : 0.0f), a.inv_count);
            }
            loss = -z[ab];
        }
        L.red[r] = loss;
        L.red[PCN_TB + r] = ent;
    }
    __syncthreads();
    if (tid == 0) {
        float loss = 0.0f, ent = 0.0f;
        for (int r = 0; r < PCN_TB; ++r) { loss += L.red[r]; ent += L.red[PCN_TB + r]; }
        a.lpart[2 * tile] = loss;
        a.lpart[2 * tile + 1] = ent;
    }
    if (a.pred_out != nullptr)
        for (int o = tid; o < valid * n.A; o += PCN_THREADS) a.pred_out[(size_t)row0 * n.A + o] = L.out[o];

    // ---- backward; every product of a weight gradient is summed over the tile's rows in row order
    float* part = a.part + (size_t)tile * n.P;
    pcn_dw(part + n.oW2, L.dout, n.A, L.h, H, n.A, H);
    pcn_db(part + n.ob2, L.dout, n.A, n.A);
    __syncthreads();
    // d/dh = dout W2, through the ReLU, in place over h (lanes run along k: W2's rows are read coalesced)
    for (int o = tid; o < PCN_TB * H; o += PCN_THREADS) {
        const int r = o / H, k = o - r * H;
        float acc = 0.0f;
        for (int j = 0; j < n.A; ++j) acc = fmaf(L.dout[r * n.A + j], p[n.oW2 + j * H + k], acc);
        L.h[o] = (L.h[o] > 0.0f) ? acc : 0.0f;
    }
    __syncthreads();
    pcn_dw(part + n.oW1, L.h, H, L.g, H, H, H);
    pcn_db(part + n.ob1, L.h, H, H);
    __syncthreads();
    // d/d(s o e) = dz1 W1, then through the product and the two sigmoids: d/d(s_emb pre-activation) over L.g now, the c_emb
    // one held in registers until every reader of L.h (dz1) is done
    float de[PCN_TB * PCN_MAX_H / PCN_THREADS];
#pragma unroll
    for (int it = 0; it < PCN_TB * PCN_MAX_H / PCN_THREADS; ++it) {
        const int o = tid + it * PCN_THREADS;
        de[it] = 0.0f;
        if (o < PCN_TB * H) {
            const int r = o / H, k = o - r * H;
            float acc = 0.0f;
            for (int j = 0; j < H; ++j) acc = fmaf(L.h[r * H + j], p[n.oW1 + j * H + k], acc);
            const float s = L.s[o], e = L.e[o];
            L.g[o] = __fmul_rn(__fmul_rn(acc, e), __fmul_rn(__fsub_rn(1.0f, s), s));
            de[it] = __fmul_rn(__fmul_rn(acc, s), __fmul_rn(__fsub_rn(1.0f, e), e));
        }
    }
    __syncthreads();
#pragma unroll
    for (int it = 0; it < PCN_TB * PCN_MAX_H / PCN_THREADS; ++it) {
        const int o = tid + it * PCN_THREADS;
        if (o < PCN_TB * H) L.h[o] = de[it];
    }
    __syncthreads();
    pcn_dw(part + n.oWs, L.g, H, L.x, n.D, H, n.D);
    pcn_db(part + n.obs, L.g, H, H);
    pcn_dw(part + n.oWc, L.h, H, L.c, PCN_CLD, H, n.C);
    pcn_db(part + n.obc, L.h, H, H);

    // ---- the last workgroup to arrive owns the step
    if (!pcn_last_arrival(a.ticket, a.ntiles, L.last)) return;
    if (tid == 0) {
        *a.ticket = 0u;                                        // re-armed for the next launch on the stream
        float loss = 0.0f, ent = 0.0f;
        for (int t = 0; t < a.ntiles; ++t) { loss += a.lpart[2 * t]; ent += a.lpart[2 * t + 1]; }
        *a.loss_out = __fmul_rn(loss, a.inv_count);
        if (a.ent_out != nullptr) *a.ent_out = ent;
    }
    // the partials summed in tile order, then Adam with torch's defaults (pcn.py:181, 234)
    for (int q = tid; q < n.P; q += PCN_THREADS) {
        float g = a.part[q];
        for (int t = 1; t < a.ntiles; ++t) g += a.part[(size_t)t * n.P + q];
        pcn_adam(g, a.params[q], a.exp_avg[q], a.exp_avg_sq[q], a.one_minus_b1, a.b2, a.one_minus_b2, a.neg_step_size, a.bc2_sqrt,
                 a.eps);
    }
}

}  // namespace morl
