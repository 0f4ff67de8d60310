// pf_linear.hpp - PF_HID_LINEAR_MAT: x' = b + A x + s e (full D x D transition matrix, constant per-filter scale s, e ~ N(0, I))
// under a linear-Gaussian observation y ~ N(b_o + A_o x, diag(s_o^2)), 1 <= D <= 8, 1 <= O <= 8 - the stand-alone model
// kernels of the step-by-step route (pf_sample_and_weight / pf_pre_weight; the fused and column kernels never see this kind).
//
// Parameter row (include/pf_amd.h): [A D*D | b D | s D | A_o O*D | b_o O | s_o O],  NP = D^2 + 2D + O D + 2 O.
//
// With a constant s per filter every piece of the optimal proposal that does not depend on the particle is a per-filter
// constant (proposals/utils.py:219-267 / linear.py:38-86):
//   precision  P = diag(s^-2) + A_o^T diag(s_o^-2) A_o,  C = P^-1 = L L^T,  K = C diag(s^-2),  c = C A_o^T diag(s_o^-2) (y - b_o)
//   APF / LGO: innovation covariance S = diag(s_o^2) + A_o diag(s^2) A_o^T = Ls Ls^T
// They are formed once per workgroup in LDS, in float64 (D, O <= 8: at most 8 x 8 Cholesky factors), and per particle the work
// is plane streaming: m = b + A x, mu = K m + c, x' = mu + L z, then the three log-densities.  The matrices are read from LDS
// with indices that are compile-time constants after unrolling (D is a template parameter, O is looped to 8 with a predicate),
// so no register array is indexed at run time (no scratch).
#pragma once
#include "pf_models.hpp"

#define PF_LIN_MAXD 8
#define PF_LIN_MAXO 8

namespace pf {

// The parameter row [A | b | s | A_o | b_o | s_o]: its length, and where each block after A starts (macros: pf_models.hpp's note)
#define PF_LINMAT_ROW_LEN(D, O) ((D) * (D) + 2 * (D) + (O) * (D) + 2 * (O))
#define PF_LINMAT_B_AT(D) ((D) * (D))
#define PF_LINMAT_S_AT(D) ((D) * (D) + (D))
#define PF_LINMAT_AO_AT(D) ((D) * (D) + 2 * (D))
#define PF_LINMAT_BO_AT(D, O) ((D) * (D) + 2 * (D) + (O) * (D))
#define PF_LINMAT_SO_AT(D, O) ((D) * (D) + 2 * (D) + (O) * (D) + (O))

// per-filter constants of the arithmetic type, as the per-particle loop reads them (LDS, broadcast reads)
template <typename T> struct LinConsts {
    T A[PF_LIN_MAXD * PF_LIN_MAXD];   // transition matrix, row-major D x D
    T b[PF_LIN_MAXD];
    T s[PF_LIN_MAXD];                 // transition scale
    T inv_s[PF_LIN_MAXD];
    T Ao[PF_LIN_MAXO * PF_LIN_MAXD];  // observation matrix, row-major O x D
    T yb[PF_LIN_MAXO];                // y - b_o of this step
    T i2so[PF_LIN_MAXO];              // 1 / (2 s_o^2)
    T K[PF_LIN_MAXD * PF_LIN_MAXD];   // C diag(s^-2)
    T c[PF_LIN_MAXD];                 // C A_o^T diag(s_o^-2) (y - b_o)
    T L[PF_LIN_MAXD * PF_LIN_MAXD];   // Cholesky factor of C
    T Ls[PF_LIN_MAXO * PF_LIN_MAXO];  // Cholesky factor of S
    T inv_ls[PF_LIN_MAXO];            // 1 / diag(Ls)
    T k_obs;    // sum_o log s_o + O log sqrt(2 pi)
    T k_trans;  // sum_d log s_d + D log sqrt(2 pi)
    T k_q;      // sum_d log L_dd + D log sqrt(2 pi)   (log q = -|z|^2 / 2 - k_q)
    T k_pre;    // sum_o log Ls_oo + O log sqrt(2 pi)
};

// float64 work space of the per-filter algebra
struct LinWork {
    double A[PF_LIN_MAXD * PF_LIN_MAXD], b[PF_LIN_MAXD], s[PF_LIN_MAXD];
    double Ao[PF_LIN_MAXO * PF_LIN_MAXD], bo[PF_LIN_MAXO], so[PF_LIN_MAXO], yb[PF_LIN_MAXO];
    double P[PF_LIN_MAXD * PF_LIN_MAXD];  // precision, then its Cholesky factor
    double C[PF_LIN_MAXD * PF_LIN_MAXD];  // covariance, then (lower part) its Cholesky factor
    double S[PF_LIN_MAXO * PF_LIN_MAXO];  // innovation covariance, then its Cholesky factor
    double r[PF_LIN_MAXD];                // A_o^T diag(s_o^-2) (y - b_o)
};

// in-place lower Cholesky factor of the n x n matrix at m (row stride ld), one thread; the strict upper part is zeroed
__device__ inline void lin_chol_inplace(double* m, int n, int ld) {
    for (int j = 0; j < n; ++j) {
        double d = m[j * ld + j];
        for (int k = 0; k < j; ++k) d -= m[j * ld + k] * m[j * ld + k];
        const double ljj = sqrt(d);
        m[j * ld + j] = ljj;
        for (int i = j + 1; i < n; ++i) {
            double t = m[i * ld + j];
            for (int k = 0; k < j; ++k) t -= m[i * ld + k] * m[j * ld + k];
            m[i * ld + j] = t / ljj;
        }
        for (int i = 0; i < j; ++i) m[i * ld + j] = 0.0;
    }
}

// Forms the per-filter constants of column b into `lc` (every thread of the workgroup calls it; ends with a barrier).
// `lgo`: the optimal proposal's algebra is needed (sample_and_weight) / `pre`: the innovation covariance is needed (pre_weight).
// Always inlined: left to the inliner's budget, the forecast kernels' further call sites turned the one in
// k_linmat_sample_and_weight into a call (100 -> 168 VGPRs at float D = 8; profiles/forecast_linear_kernel_resources.txt).
template <typename T, int D>
__device__ __forceinline__ void lin_prepare(LinConsts<T>& lc, LinWork& w, const T* __restrict__ row, int O, const T* __restrict__ yrow,
                                   bool lgo, bool pre) {
    const int tid = threadIdx.x;
    const int NP = PF_LINMAT_ROW_LEN(D, O);
    const T* ao = row + PF_LINMAT_AO_AT(D);  // the observation block [A_o | b_o | s_o] from its own start
    if (tid < NP) {  // (NP <= 64 + 16 + 64 + 16 < PF_BLOCK)
        const double v = (double)row[tid];
        if (tid < PF_LINMAT_B_AT(D)) w.A[tid] = v;
        else if (tid < PF_LINMAT_S_AT(D)) w.b[tid - PF_LINMAT_B_AT(D)] = v;
        else if (tid < PF_LINMAT_AO_AT(D)) w.s[tid - PF_LINMAT_S_AT(D)] = v;
        else if (tid < PF_LINMAT_BO_AT(D, O)) w.Ao[tid - PF_LINMAT_AO_AT(D)] = v;
        else if (tid < PF_LINMAT_SO_AT(D, O)) w.bo[tid - PF_LINMAT_AO_AT(D) - O * D] = v;
        else w.so[tid - PF_LINMAT_AO_AT(D) - O * D - O] = v;
    }
    __syncthreads();
    if (tid < O) w.yb[tid] = yrow ? (double)yrow[tid] - (double)ao[O * D + tid] : 0.0;
    if (lgo && tid >= 64 && tid < 64 + D * D) {  // precision (a second wave: overlaps the first's innovation covariance)
        const int i = (tid - 64) / D, j = (tid - 64) % D;
        double v = (i == j) ? 1.0 / (w.s[i] * w.s[i]) : 0.0;
        for (int o = 0; o < O; ++o) v += w.Ao[o * D + i] * w.Ao[o * D + j] / (w.so[o] * w.so[o]);
        w.P[i * D + j] = v;
    }
    if (pre && tid < O * O) {
        const int o = tid / O, p = tid % O;
        double v = (o == p) ? w.so[o] * w.so[o] : 0.0;
        for (int d = 0; d < D; ++d) v += w.Ao[o * D + d] * (w.s[d] * w.s[d]) * w.Ao[p * D + d];
        w.S[o * O + p] = v;
    }
    __syncthreads();
    if (lgo && tid < D) {  // A_o^T diag(s_o^-2) (y - b_o)
        double v = 0.0;
        for (int o = 0; o < O; ++o) v += w.Ao[o * D + tid] * (w.yb[o] / (w.so[o] * w.so[o]));
        w.r[tid] = v;
    }
    if (lgo && tid == 64) lin_chol_inplace(w.P, D, D);
    if (pre && tid == 128) lin_chol_inplace(w.S, O, O);
    __syncthreads();
    if (lgo && tid < D) {  // column `tid` of C = P^-1: P c = e_j through the factor (forward, then backward substitution)
        const int j = tid;
        double v[D];
#pragma unroll
        for (int i = 0; i < D; ++i) {
            double t = (i == j) ? 1.0 : 0.0;
#pragma unroll
            for (int k = 0; k < i; ++k) t -= w.P[i * D + k] * v[k];
            v[i] = t / w.P[i * D + i];
        }
#pragma unroll
        for (int i = D - 1; i >= 0; --i) {
            double t = v[i];
#pragma unroll
            for (int k = i + 1; k < D; ++k) t -= w.P[k * D + i] * v[k];
            v[i] = t / w.P[i * D + i];
        }
#pragma unroll
        for (int i = 0; i < D; ++i) w.C[i * D + j] = v[i];
    }
    __syncthreads();
    if (lgo && tid < D * D) {  // K = C diag(s^-2), written before C is factorised in place
        const int i = tid / D, j = tid % D;
        lc.K[tid] = (T)(w.C[i * D + j] / (w.s[j] * w.s[j]));
    }
    if (lgo && tid >= 64 && tid < 64 + D) {
        const int i = tid - 64;
        double v = 0.0;
        for (int j = 0; j < D; ++j) v += w.C[i * D + j] * w.r[j];
        lc.c[i] = (T)v;
    }
    __syncthreads();
    if (lgo && tid == 0) {
        // (the factor reads the lower triangle of C only)
        lin_chol_inplace(w.C, D, D);
        double k = 0.0;
        for (int d = 0; d < D; ++d) k += log(w.C[d * D + d]);
        lc.k_q = (T)(k + D * PF_LOG_SQRT_2PI);
    }
    if (tid == 64) {
        double k = 0.0;
        for (int d = 0; d < D; ++d) k += log(w.s[d]);
        lc.k_trans = (T)(k + D * PF_LOG_SQRT_2PI);
        double ko = 0.0;
        for (int o = 0; o < O; ++o) ko += log(w.so[o]);
        lc.k_obs = (T)(ko + O * PF_LOG_SQRT_2PI);
        if (pre) {
            double kp = 0.0;
            for (int o = 0; o < O; ++o) kp += log(w.S[o * O + o]);
            lc.k_pre = (T)(kp + O * PF_LOG_SQRT_2PI);
        }
    }
    if (tid >= 128 && tid < 128 + D * D) lc.A[tid - 128] = (T)w.A[tid - 128];
    if (tid >= 192 && tid < 192 + O * D) lc.Ao[tid - 192] = (T)w.Ao[tid - 192];
    if (tid < D) {
        lc.b[tid] = (T)w.b[tid];
        lc.s[tid] = (T)w.s[tid];
        lc.inv_s[tid] = (T)(1.0 / w.s[tid]);
    }
    if (tid >= 32 && tid < 32 + O) {
        const int o = tid - 32;
        lc.yb[o] = (T)w.yb[o];
        lc.i2so[o] = (T)(0.5 / (w.so[o] * w.so[o]));
    }
    __syncthreads();
    if (lgo && tid < D * D) {
        const int i = tid / D, j = tid % D;
        lc.L[tid] = (T)(j <= i ? w.C[i * D + j] : 0.0);
    }
    if (pre && tid >= 64 && tid < 64 + O * O) {
        const int q = tid - 64, o = q / O, p = q % O;
        lc.Ls[o * PF_LIN_MAXO + p] = (T)(p <= o ? w.S[o * O + p] : 0.0);
        if (p == o) lc.inv_ls[o] = (T)(1.0 / w.S[o * O + o]);
    }
    __syncthreads();
}

// log N(y; b_o + A_o x, diag(s_o^2)) - the observation density of the model (bootstrap.py:12-14)
template <typename T, int D>
__device__ __forceinline__ T lin_obs_lp(const LinConsts<T>& lc, int O, const T (&x)[D]) {
    T lp = -lc.k_obs;
#pragma unroll
    for (int o = 0; o < PF_LIN_MAXO; ++o) {
        if (o < O) {
            T r = lc.yb[o];
#pragma unroll
            for (int d = 0; d < D; ++d) r -= lc.Ao[o * D + d] * x[d];
            lp -= (r * r) * lc.i2so[o];
        }
    }
    return lp;
}

// m = b + A x
template <typename T, int D>
__device__ __forceinline__ void lin_mean(const LinConsts<T>& lc, const T (&x)[D], T (&m)[D]) {
#pragma unroll
    for (int i = 0; i < D; ++i) {
        T t = lc.b[i];
#pragma unroll
        for (int j = 0; j < D; ++j) t += lc.A[i * D + j] * x[j];
        m[i] = t;
    }
}

template <typename T, int D>
__global__ __launch_bounds__(PF_BLOCK) void k_linmat_sample_and_weight(const T* __restrict__ params, int O, int proposal, int weigh,
                                                                       const T* __restrict__ x, const T* __restrict__ y, int y_rows,
                                                                       const T* __restrict__ z, uint64_t seed, uint32_t step,
                                                                       T* __restrict__ x_out, T* __restrict__ w_out, int64_t N, int B) {
    __shared__ LinConsts<T> lc;
    __shared__ LinWork wk;
    const int b = blockIdx.y;
    const int NP = PF_LINMAT_ROW_LEN(D, O);
    const bool lgo = weigh && proposal == PF_PROP_LGO;  // (weigh = 0: propagate only, from the dynamics)
    lin_prepare<T, D>(lc, wk, params + (int64_t)b * NP, O, (weigh && y) ? y + (int64_t)(y_rows == 1 ? 0 : b) * O : nullptr, lgo, false);
    const int64_t plane = (int64_t)B * N;
    for (int64_t i = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x; i < N; i += (int64_t)gridDim.x * PF_BLOCK) {
        // (the constants are re-read from LDS in every iteration - broadcast reads - instead of being hoisted out of the loop into
        // some hundred registers: the compiler may not assume the LDS unchanged across this point)
        asm volatile("" ::: "memory");
        const int64_t e = (int64_t)b * N + i;
        T xv[D], zv[D], m[D], xn[D];
#pragma unroll
        for (int d = 0; d < D; ++d) xv[d] = x[d * plane + e];
        if (z) {
#pragma unroll
            for (int d = 0; d < D; ++d) zv[d] = z[d * plane + e];
        } else {
            NormalDraw<T, D>::draw(seed, PF_STREAM_NORMAL, step, (uint64_t)e, zv);
        }
        lin_mean<T, D>(lc, xv, m);
        if (!lgo) {
#pragma unroll
            for (int d = 0; d < D; ++d) xn[d] = m[d] + lc.s[d] * zv[d];
            if (weigh) w_out[e] = lin_obs_lp<T, D>(lc, O, xn);
        } else {
            // mu = K m + c;  x' = mu + L z;  log w = log p(y | x') + log p(x' | x) - log q(x')
            T zz = T(0), lt = -lc.k_trans;
#pragma unroll
            for (int r = 0; r < D; ++r) {
                T t = lc.c[r];
#pragma unroll
                for (int j = 0; j < D; ++j) t += lc.K[r * D + j] * m[j];
#pragma unroll
                for (int j = 0; j <= r; ++j) t += lc.L[r * D + j] * zv[j];
                xn[r] = t;
                const T eps = (t - m[r]) * lc.inv_s[r];
                lt -= T(0.5) * (eps * eps);
                zz += zv[r] * zv[r];
            }
            w_out[e] = lin_obs_lp<T, D>(lc, O, xn) + lt - (-T(0.5) * zz - lc.k_q);
        }
#pragma unroll
        for (int d = 0; d < D; ++d) x_out[d * plane + e] = xn[d];
    }
}

template <typename T, int D>
__global__ __launch_bounds__(PF_BLOCK) void k_linmat_pre_weight(const T* __restrict__ params, int O, int proposal, const T* __restrict__ x,
                                                                const T* __restrict__ y, int y_rows, T* __restrict__ out, int64_t N, int B) {
    __shared__ LinConsts<T> lc;
    __shared__ LinWork wk;
    const int b = blockIdx.y;
    const int NP = PF_LINMAT_ROW_LEN(D, O);
    const bool lgo = proposal == PF_PROP_LGO;
    lin_prepare<T, D>(lc, wk, params + (int64_t)b * NP, O, y + (int64_t)(y_rows == 1 ? 0 : b) * O, false, lgo);
    const int64_t plane = (int64_t)B * N;
    for (int64_t i = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x; i < N; i += (int64_t)gridDim.x * PF_BLOCK) {
        // (the constants are re-read from LDS in every iteration - broadcast reads - instead of being hoisted out of the loop into
        // some hundred registers: the compiler may not assume the LDS unchanged across this point)
        asm volatile("" ::: "memory");
        const int64_t e = (int64_t)b * N + i;
        T xv[D];
#pragma unroll
        for (int d = 0; d < D; ++d) xv[d] = x[d * plane + e];
        if (!lgo) {  // Bootstrap: log p(y | b + A x)  (the default pre-weight function: the one-step mean)
            T m[D];
            lin_mean<T, D>(lc, xv, m);
            out[e] = lin_obs_lp<T, D>(lc, O, m);
        } else {
            // LinearGaussianObservations.pre_weight (linear.py:57-86): log N(y; b_o + A_o x, S) at the UN-propagated particle
            T v[PF_LIN_MAXO];
            T quad = T(0);
#pragma unroll
            for (int o = 0; o < PF_LIN_MAXO; ++o) {
                T t = T(0);
                if (o < O) {
                    t = lc.yb[o];
#pragma unroll
                    for (int d = 0; d < D; ++d) t -= lc.Ao[o * D + d] * xv[d];
#pragma unroll
                    for (int k = 0; k < o; ++k) t -= lc.Ls[o * PF_LIN_MAXO + k] * v[k];
                    t *= lc.inv_ls[o];
                    quad += t * t;
                }
                v[o] = t;
            }
            out[e] = -T(0.5) * quad - lc.k_pre;
        }
    }
}

}  // namespace pf
