// LCN's episode selection (multi_policy/lcn/lcn.py:221-252, the scoring half of LCN._nlargest): Lorenz / lambda-Lorenz / Pareto
// dominance, the distance of every return to its closest front point, the duplicate penalty and the crowding factor -- one
// launch, every fp32 operation rounded where numpy rounds it, so that l2 is numpy's l2 bit for bit.
#pragma once
#include "morl_device.h"
#include "morl_hip.h"

namespace morl {

// One workgroup: the front must be complete before any distance is taken and the first-occurrence flags need the front, two
// block-wide dependencies that one launch can only honour inside a workgroup.  Both row sets stay in LDS for the whole
// call: LCN_MAX_N * MORL_MAX_OBJ * 4 B = 64 KiB each, plus the flags and the two index lists 12 KiB: 140 KiB of the CU's
// 160 KiB.  That is what sets LCN_MAX_N.
//
// One CU retires a 64-lane instruction per SIMD every four cycles, so the N^2 pair tests are what the call costs, and the
// front is found in two rounds that rarely need all of them:
//   A  every candidate against the first LCN_PIVOTS rows only; one that meets a dominator is settled for good (a Lorenz
//      front is a small part of the heap, so most are)
//   B  the S survivors against all N rows, transposed: every work-item keeps its own two rows in registers, the survivor's
//      row is an LDS broadcast, a ballot tells whether any row dominates it or is an earlier copy of it -- S * N tests spread
//      evenly over the workgroup however few the survivors are
// and the distances run over the compacted front list, F rows per candidate.  All of it is N^2 at worst (mode 0 in eight
// objectives, where half the heap is the front), N * (LCN_PIVOTS + S + F) otherwise.
constexpr int LCN_MAX_N = 2048;
constexpr int LCN_THREADS = 1024;
constexpr int LCN_ROWS = LCN_MAX_N / LCN_THREADS;      // rows a work-item owns: i = tid + k * LCN_THREADS
constexpr int LCN_PIVOTS = 64;

// np.linalg.norm(a - b, axis=-1)**2 of two rows as numpy forms it: the difference, the square and every add rounded on their
// own; add.reduce over a contiguous axis of n < 8 floats is a sequential loop, of n == 8 the eight-accumulator pairwise block
// ((s0+s1)+(s2+s3))+((s4+s5)+(s6+s7)).
template <int R>
__device__ __forceinline__ float lcn_sumsq(const float (&a)[R], const float* __restrict__ b) {
    float s[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const float d = __fsub_rn(a[r], b[r]);
        s[r] = __fmul_rn(d, d);
    }
    if constexpr (R == 8) {
        return __fadd_rn(__fadd_rn(__fadd_rn(s[0], s[1]), __fadd_rn(s[2], s[3])),
                         __fadd_rn(__fadd_rn(s[4], s[5]), __fadd_rn(s[6], s[7])));
    } else {
        float acc = s[0];
#pragma unroll
        for (int r = 1; r < R; ++r) acc = __fadd_rn(acc, s[r]);
        return acc;
    }
}

// mode 0: t = x = raw row.  mode 1: t = cumsum(sort(row)), x = raw row.  mode 2: s = sort(row), c = cumsum(s),
// t = f32(lam * s) + f32(oml * c), x = s (lcn.py:229 rebinds `returns` to the sorted rows).
// nd[i]   = no j with t_j >= t_i everywhere and t_j != t_i somewhere, and no j < i with t_j == t_i   (get_non_dominated_inds)
// l2[i]   = -sqrt(min over j with nd[j] of |x_i - x_j|^2); the square root is correctly rounded, hence monotone, hence taken
//           once after the min
// uniq[i] = nd[i] and no j < i with nd[j] and x_j == x_i (np.unique(..., return_index=True): first occurrences);
// l2[i] -= 1e-5f where !uniq[i]; l2[i] *= 2 where crowded[i].
// crowded == NULL or l2_out == NULL: only nd_out is written.
template <int R>
__global__ __launch_bounds__(LCN_THREADS) void lcn_select_kernel(const float* __restrict__ returns, int N, int mode, float lam,
                                                                 float oml, const uint8_t* __restrict__ crowded,
                                                                 float* __restrict__ l2_out, uint8_t* __restrict__ nd_out) {
    __shared__ __attribute__((aligned(16))) float s_t[LCN_MAX_N * R];      // dominance rows
    __shared__ __attribute__((aligned(16))) float s_x[LCN_MAX_N * R];      // distance rows
    __shared__ uint8_t s_nd[LCN_MAX_N];              // front flags, by row
    __shared__ uint8_t s_out[LCN_MAX_N];             // round B's verdicts, by survivor
    __shared__ unsigned short s_surv[LCN_MAX_N];     // rows that round A did not settle (any order)
    __shared__ unsigned short s_front[LCN_MAX_N];    // rows of the front (any order: min and "an earlier copy exists" do not care)
    __shared__ int s_cnt[2];                         // lengths of the two lists
    const int tid = (int)threadIdx.x;

    // ---- the row transform; a work-item keeps the dominance rows it owns in registers --------------------------------------
    float tk[LCN_ROWS][R];
    if (tid < 2) s_cnt[tid] = 0;
#pragma unroll
    for (int k = 0; k < LCN_ROWS; ++k) {
        const int i = tid + k * LCN_THREADS;
        float raw[R], s[R], c[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            raw[r] = s[r] = (i < N) ? returns[(size_t)i * R + r] : 0.f;
            c[r] = 0.f;
        }
        if (mode != 0) {
            // insertion sort on registers (ascending); the compare-exchange form keeps every index a compile-time constant
#pragma unroll
            for (int a = 1; a < R; ++a)
#pragma unroll
                for (int b = a; b > 0; --b) {
                    const float lo = s[b - 1], hi = s[b];
                    const bool swap = hi < lo;
                    s[b - 1] = swap ? hi : lo;
                    s[b] = swap ? lo : hi;
                }
            c[0] = s[0];
#pragma unroll
            for (int r = 1; r < R; ++r) c[r] = __fadd_rn(c[r - 1], s[r]);     // np.cumsum: left to right
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            float t = raw[r], x = raw[r];
            if (mode == 1) t = c[r];
            if (mode == 2) {
                t = __fadd_rn(__fmul_rn(lam, s[r]), __fmul_rn(oml, c[r]));
                x = s[r];
            }
            tk[k][r] = t;
            if (i < N) {
                s_t[i * R + r] = t;
                s_x[i * R + r] = x;
            }
        }
        if (i < N) s_nd[i] = 0;
    }
    __syncthreads();

    // ---- round A: own rows against the pivots (LDS broadcasts); what no pivot dominates goes on the survivor list ------------
    const int n_piv = min(N, LCN_PIVOTS);
#pragma unroll
    for (int k = 0; k < LCN_ROWS; ++k) {
        const int i = tid + k * LCN_THREADS;
        bool dominated = false;
        for (int j = 0; j < n_piv; ++j) {
            bool ge = true, eq = true;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const float tj = s_t[j * R + r];
                ge = ge && (tj >= tk[k][r]);
                eq = eq && (tj == tk[k][r]);
            }
            dominated = dominated || (ge && !eq);
        }
        if (i < N && !dominated) {
            const int pos = atomicAdd(&s_cnt[0], 1);          // pos < N: one entry per row at most
            s_surv[pos] = (unsigned short)i;
            s_out[pos] = 0;
        }
    }
    __syncthreads();

    // ---- round B: every survivor against all rows; the rows are the work-items' own, the survivor is the broadcast -------------
    const int S = s_cnt[0];
    for (int s = 0; s < S; ++s) {          // (S and s are uniform over the workgroup: every wave reaches every ballot)
        const int i = (int)s_surv[s];
        float ti[R];
#pragma unroll
        for (int r = 0; r < R; ++r) ti[r] = s_t[i * R + r];
        bool hit = false;                  // one of my rows dominates row i, or equals it and comes before it
#pragma unroll
        for (int k = 0; k < LCN_ROWS; ++k) {
            const int j = tid + k * LCN_THREADS;
            bool ge = true, eq = true;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                ge = ge && (tk[k][r] >= ti[r]);
                eq = eq && (tk[k][r] == ti[r]);
            }
            hit = hit || (j < N && ((ge && !eq) || (eq && j < i)));
        }
        if (__ballot(hit) != 0ull && (tid & 63) == 0) s_out[s] = 1;      // (every writer stores the same 1)
    }
    __syncthreads();
    for (int s = tid; s < S; s += LCN_THREADS)
        if (!s_out[s]) {
            const int i = (int)s_surv[s];
            s_nd[i] = 1;
            s_front[atomicAdd(&s_cnt[1], 1)] = (unsigned short)i;      // at most S <= N entries
        }
    __syncthreads();

    for (int i = tid; i < N; i += LCN_THREADS) nd_out[i] = s_nd[i];
    if (!l2_out || !crowded) return;        // (kernel arguments: uniform over the block)

    // ---- distance to the closest front point, first occurrences, penalties ---------------------------------------------
    const int F = s_cnt[1];                 // >= 1: dominance is a strict partial order and the first copy of a row is kept
    for (int i = tid; i < N; i += LCN_THREADS) {
        float xi[R];
#pragma unroll
        for (int r = 0; r < R; ++r) xi[r] = s_x[i * R + r];
        float best = 0.f;
        bool seen_before = false;
        for (int f = 0; f < F; ++f) {
            const int j = (int)s_front[f];  // (the same in every lane)
            const float* xj = &s_x[j * R];
            const float d2 = lcn_sumsq<R>(xi, xj);
            best = (f == 0 || d2 < best) ? d2 : best;
            bool eq = true;
#pragma unroll
            for (int r = 0; r < R; ++r) eq = eq && (xj[r] == xi[r]);
            seen_before = seen_before || (eq && j < i);
        }
        float l2 = -(float)sqrt((double)best);      // a double root rounded to float is the correctly rounded float root (53 >= 2 * 24 + 2)
        const bool uniq = s_nd[i] && !seen_before;
        if (!uniq) l2 = __fsub_rn(l2, 1e-5f);
        if (crowded[i]) l2 = __fmul_rn(l2, 2.f);
        l2_out[i] = l2;
    }
}

}  // namespace morl
