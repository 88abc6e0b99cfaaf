// IPRO's hypervolume-improvement scores in one batch (gfx950, wave64): multi_policy/ipro/ipro.py:212-226 asks, on every
// iteration, for the hypervolume of ONE base set (pf u completed) plus ONE candidate lower point, for up to 50 candidates, all
// against the same reference point (the ideal).  Frame: OuterLoop.compute_hypervolume (outer_loop.py:250-256), pymoo's
// minimisation frame without normalisation -- a point p counts only if ref >= p everywhere and > somewhere (anything else is
// dropped, not clipped), and the value is the volume of the union of the boxes [p, ref].
//
// Form: HV(base u {c}) = HV(base) + EXCL(c), where EXCL(c) is the part of the box [c, ref] no base point covers.
//   * HV(base) is shared by all candidates: a slab decomposition as in metrics_kernels.h, in the minimisation frame, spread
//     over a number of workgroups that depends on (n, R) alone;
//   * EXCL(c) needs only the base points as they look from inside [c, ref]: on an axis d < R-1 a coordinate p_d <= c_d
//     collapses onto c_d and a coordinate p_d >= ref_d can never cover, so one workgroup per candidate COMPACTS, in LDS, the
//     cut coordinates of every axis to those strictly inside (c_d, ref_d).  The slabs of the compacted grid are independent
//     (one work-item per slab, strided); inside a slab the base covers a single interval of the last axis,
//     [min{ p_last : p <= slab's lower corner }, ref_last], and the candidate adds what lies between c_last and that minimum.
//     The staged points are ordered by their last coordinate, so the first point that covers a slab is that minimum.
//     Every term is non-negative: nothing cancels.
// Cost per candidate: prod_d (m_d + 1) slabs, m_d = base coordinates strictly inside (c_d, ref_d), times at most n point tests
// (the walk stops at the first covering point); the uncompacted form costs (n + 1)^(R-1) slabs of n + 1 tests for every
// candidate.
//
// A candidate's slabs are shared by ipro_cand_blocks(n, R) workgroups and the base's by ipro_base_blocks(n, R): with one
// workgroup a candidate, 60 base points in 4 objectives took 4 ms (226 981 slabs on four waves, every point test an LDS round
// trip), the time of the 51 separate morl_hypervolume calls it replaces.
//
// Determinism: a candidate's workgroups have a fixed size and a fixed sum order (slab-strided partials, butterfly, ordered wave
// partials, ordered workgroup partials) and read nothing but (base, cand[k], ref); both splits are functions of (n, R).  So the
// bits of out[k] depend on (base, cand[k], ref) only -- not on k, K or the grid -- and two equal candidates tie exactly.
#pragma once
#include "metrics_kernels.h"

namespace morl {

constexpr int IPRO_THREADS = 256;
constexpr int IPRO_MAX_N = HV_MAX_N - 1;       // base points: with the candidate, the LDS-staged size of metrics_kernels.h
constexpr int IPRO_MAX_K = 1024;               // candidates per call
constexpr int IPRO_MAX_BASE_BLOCKS = 64;       // workgroups that share the base set's own hypervolume
constexpr int IPRO_MAX_CAND_BLOCKS = 16;       // workgroups that share one candidate's slabs

// workgroups of the base's hypervolume: one per 16 slabs a work-item, from the uncompacted slab count -- a function of (n, R)
inline int ipro_base_blocks(int n, int R) {
    double slabs = 1.0;
    for (int d = 0; d < R - 1; ++d) slabs *= (double)(n > 0 ? n : 1);
    const double want = slabs / (16.0 * IPRO_THREADS);
    return want <= 1.0 ? 1 : (want >= (double)IPRO_MAX_BASE_BLOCKS ? IPRO_MAX_BASE_BLOCKS : (int)want);
}

// workgroups of one candidate: one per 4 slabs a work-item (a candidate's point walks are the long ones: they start at the far
// corner of the box), from the slab count of n + 1 points, at most 16 -- a function of (n, R)
inline int ipro_cand_blocks(int n, int R) {
    double slabs = 1.0;
    for (int d = 0; d < R - 1; ++d) slabs *= (double)(n + 1);
    const double want = slabs / (4.0 * IPRO_THREADS);
    return want <= 1.0 ? 1 : (want >= (double)IPRO_MAX_CAND_BLOCKS ? IPRO_MAX_CAND_BLOCKS : (int)want);
}

// blockIdx.x < K * S: share blockIdx.x % S of EXCL(cand[blockIdx.x / S]);  otherwise share blockIdx.x - K * S of HV(base);
// either way -> part[blockIdx.x]
template <int R>
__global__ __launch_bounds__(IPRO_THREADS) void ipro_hvis_kernel(const double* __restrict__ base, int n,
                                                                 const double* __restrict__ cand, int K, int S,
                                                                 const double* __restrict__ ref, double* __restrict__ part) {
    constexpr int A = R - 1;                                  // cut axes
    constexpr int AX = A > 0 ? A : 1;
    __shared__ double s_pts[HV_MAX_N * R];                    // counted base points [m][R], ascending in the last coordinate
    __shared__ double s_co[HV_MAX_N * AX];                    // [A][HV_MAX_N]: first the sort keys, then the compacted cuts
    __shared__ int s_m;                                       // counted base points
    __shared__ int s_md[AX];                                  // cuts per axis
    __shared__ double s_red[IPRO_THREADS / 64];
    const int tid = (int)threadIdx.x;
    const bool is_base = (int)blockIdx.x >= K * S;
    const int share = is_base ? (int)blockIdx.x - K * S : (int)blockIdx.x % S, shares = is_base ? (int)gridDim.x - K * S : S;
    const int k = is_base ? 0 : (int)blockIdx.x / S;

    double r[R], c[R];
#pragma unroll
    for (int d = 0; d < R; ++d) r[d] = ref[d];
    if (!is_base) {                                           // (workgroup-uniform: every work-item reads the same row)
        bool all_le = true, any_lt = false;
#pragma unroll
        for (int d = 0; d < R; ++d) {
            c[d] = cand[(size_t)k * R + d];
            all_le = all_le && (c[d] <= r[d]);
            any_lt = any_lt || (c[d] < r[d]);
        }
        if (!(all_le && any_lt)) {                            // the candidate is dropped: base u {c} is base
            if (tid == 0) part[blockIdx.x] = 0.0;
            return;
        }
    }

    // 1. sort key of every base point: its last coordinate, +inf when the point is dropped
    for (int t = tid; t < n; t += IPRO_THREADS) {
        bool all_le = true, any_lt = false;
#pragma unroll
        for (int d = 0; d < R; ++d) {
            const double v = base[(size_t)t * R + d];
            all_le = all_le && (v <= r[d]);
            any_lt = any_lt || (v < r[d]);
        }
        s_co[t] = (all_le && any_lt) ? base[(size_t)t * R + A] : INFINITY;
    }
    __syncthreads();
    // 2. rank sort (ties by index) into s_pts; the counted points come first
    if (tid == 0) {
        int m = 0;
        for (int j = 0; j < n; ++j) m += (s_co[j] < INFINITY) ? 1 : 0;
        s_m = m;
    }
    for (int t = tid; t < n; t += IPRO_THREADS) {
        const double v = s_co[t];
        int rank = 0;
        for (int j = 0; j < n; ++j) {
            const double u = s_co[j];
            rank += (u < v || (u == v && j < t)) ? 1 : 0;
        }
#pragma unroll
        for (int d = 0; d < R; ++d) s_pts[rank * R + d] = base[(size_t)t * R + d];
    }
    __syncthreads();
    const int m = s_m;
    if (is_base) {                                            // the base's own box starts at its component-wise minimum
#pragma unroll
        for (int d = 0; d < R; ++d) c[d] = r[d];
        for (int j = 0; j < m; ++j) {
#pragma unroll
            for (int d = 0; d < R; ++d) c[d] = fmin(c[d], s_pts[j * R + d]);
        }
    }
    // 3. per axis: the coordinates strictly inside (c_d, ref_d), ascending (rank sort among themselves, ties by index)
#pragma unroll
    for (int d = 0; d < A; ++d) {
        if (tid != d) continue;                               // (one work-item per axis counts; d stays a constant index)
        int cnt = 0;
        for (int j = 0; j < m; ++j) {
            const double u = s_pts[j * R + d];
            cnt += (u > c[d] && u < r[d]) ? 1 : 0;
        }
        s_md[d] = cnt;
    }
#pragma unroll
    for (int d = 0; d < A; ++d) {
        for (int t = tid; t < m; t += IPRO_THREADS) {
            const double v = s_pts[t * R + d];
            if (!(v > c[d] && v < r[d])) continue;
            int rank = 0;
            for (int j = 0; j < m; ++j) {
                const double u = s_pts[j * R + d];
                rank += ((u > c[d] && u < r[d]) && (u < v || (u == v && j < t))) ? 1 : 0;
            }
            s_co[d * HV_MAX_N + rank] = v;                    // (the keys of step 1 are dead: step 2 ended with a barrier)
        }
    }
    __syncthreads();
    int md[AX];
    long long n_slabs = 1;
#pragma unroll
    for (int d = 0; d < A; ++d) {
        md[d] = s_md[d];
        n_slabs *= (long long)(md[d] + 1);
    }

    // 4. the slabs
    const bool narrow = n_slabs <= 0x7fffffffLL;
    double acc = 0.0;
    for (long long b = (long long)share * IPRO_THREADS + tid; b < n_slabs; b += (long long)shares * IPRO_THREADS) {
        double lo[AX];
        double vol = 1.0;
        long long rem = b;
#pragma unroll
        for (int d = 0; d < A; ++d) {
            int i;
            if (narrow) {                                     // (a 64-bit division is a long routine on the device)
                const unsigned q = (unsigned)rem;
                i = (int)(q % (unsigned)(md[d] + 1));
                rem = (long long)(q / (unsigned)(md[d] + 1));
            } else {
                i = (int)(rem % (md[d] + 1));
                rem /= (md[d] + 1);
            }
            lo[d] = (i > 0) ? s_co[d * HV_MAX_N + i - 1] : c[d];
            const double hi = (i < md[d]) ? s_co[d * HV_MAX_N + i] : r[d];
            vol *= (hi - lo[d]);
        }
        if (!(vol > 0.0)) continue;                           // an empty slab (a repeated coordinate, or c_d == ref_d)
        double bottom = r[A];                                 // where the base's cover of this slab starts on the last axis
        for (int j = 0; j < m; ++j) {
            const double pl = s_pts[j * R + A];
            if (!(pl < bottom)) break;                        // ascending: nothing further reaches below ref_last
            bool covers = true;
#pragma unroll
            for (int d = 0; d < A; ++d) covers = covers && (s_pts[j * R + d] <= lo[d]);
            if (covers) { bottom = pl; break; }
        }
        const double len = is_base ? (r[A] - bottom) : fmax(bottom - c[A], 0.0);
        acc += vol * len;
    }
    acc = wave_sum(acc);
    if (lane_id() == 0) s_red[wave_id()] = acc;
    __syncthreads();
    if (tid == 0) {
        double t = 0.0;
        for (int w = 0; w < IPRO_THREADS / 64; ++w) t += s_red[w];
        part[blockIdx.x] = t;
    }
}

// out[k] = HV(base) + EXCL(cand[k]) for k < K, out[K] = HV(base); both are the sums of their shares in index order
__global__ __launch_bounds__(IPRO_THREADS) void ipro_finish_kernel(const double* __restrict__ part, int K, int S, int shares,
                                                                   double* __restrict__ out) {
    const int k = (int)blockIdx.x * IPRO_THREADS + (int)threadIdx.x;
    if (k > K) return;
    double hv = 0.0;
    for (int s = 0; s < shares; ++s) hv += part[(size_t)K * S + s];
    if (k < K) {
        double excl = 0.0;
        for (int s = 0; s < S; ++s) excl += part[(size_t)k * S + s];
        hv += excl;
    }
    out[k] = hv;
}

}  // namespace morl
