// pf_forecast_linear.hpp - forecasting from a filter state for PF_HID_LINEAR_MAT under PF_OBS_LINEAR, 1 <= D, O <= 8: pf_forecast.hpp's
// scheme and conventions (read its header first: one launch for the whole horizon, a thread walks its consecutive particles through
// all H steps in registers, per-STEP accumulators reduced across the workgroup into a slab that a small second launch adds in a
// fixed order; normalised weights, pivoted sums in double, a NaN poisons its row, nothing particle-sized written without paths)
// for the model family of pf_linear.hpp, with predictive COVARIANCES as a template switch.
//
// Per step and particle:   x <- b + A x + s * z                        (lin_mean; the per-filter constants: lin_prepare, in LDS,
//                          m_o = b_o + sum_d A_o[o][d] x_d, scale s_o   re-read per particle as k_linmat_sample_and_weight does)
// and in double            sum W, sum W (x_d - c_d), sum W (x_d - c_d)^2, sum W (m_o - k_o), sum W ((m_o - k_o)^2 + s_o^2)
// COV adds                 sum W (x_i - c_i)(x_j - c_j), i > j
// about the pivots c = the INPUT cloud's first particle of the column walked the same moves with zero draws - in T, through the
// same function a particle goes through - and k = b_o + A_o c.
//
// k_forecast_linmat_final forms, with r = mean - c:   cov_ij = P_ij - r_i P1_j - r_j P1_i + r_i r_j S0   (both triangles from the one
// sum; the diagonal IS x_var).  y_cov is Rao-Blackwellised like y_var - the covariance of the conditional means plus
// S0 diag(s_o^2) - and is NOT accumulated: m - k = A_o (x - c), so the centred sums of x carry it,
//     y_cov = A_o P A_o^T - r_y (A_o P1)^T - (A_o P1) r_y^T + r_y r_y^T S0 + S0 diag(s_o^2),     r_y = y_mean - k,
// in double for any sum W.  The COV instantiation so keeps 1 + 2 D + D (D - 1) / 2 + 2 MAXO accumulators (61 doubles at D = 8).
//
// Slab: (H, Q, B, tiles) with the rows of THIS (D, O): [W | X D | XX D | M O | MM O | P D (D - 1) / 2], Q = linfc_q(D, O, cov).
// Draws: pf_forecast.hpp's streams and addressing - normal number (b N + i) D + d of PF_STREAM_FORECAST_Z at counter step h, number
// (b N + i) PF_LIN_MAXO + o of PF_STREAM_FORECAST_E (only when y paths are stored) - addressed by the particle alone: a result is a
// function of the seed, not of LinFc<D>::ITEMS, the tile geometry, paths or COV.
#pragma once

namespace pf {

// consecutive particles per thread: the state, its draws and the weights of ITEMS particles stay in registers beside the
// accumulators (profiles/forecast_linear_kernel_resources.txt)
template <int D> struct LinFc { static constexpr int ITEMS = D <= 4 ? 4 : 2; };
__host__ __device__ constexpr int linfc_items(int D) { return D <= 4 ? 4 : 2; }
__host__ __device__ constexpr int linfc_q(int D, int O, bool cov) { return 1 + 2 * D + 2 * O + (cov ? D * (D - 1) / 2 : 0); }

// pivoted_variance's off-diagonal: Pij = sum W (x_i - c_i)(x_j - c_j), r = mean - c.  Not contracted into fmas either: one particle
// of weight 1 gives Pij = r_i P1_j = r_j P1_i = r_i r_j S0 rounded alike, and a covariance of exactly 0.
__device__ __forceinline__ double pivoted_covariance(double s0, double p1i, double p1j, double pij, double ri, double rj) {
#pragma clang fp contract(off)
    return pij - ri * p1j - rj * p1i + (ri * rj) * s0;
}

// one move of the hidden process in place (a pivot: z = 0)
template <typename T, int D>
__device__ __forceinline__ void linfc_move(const LinConsts<T>& lc, T (&x)[D], const T (&z)[D]) {
    T m[D];
    lin_mean<T, D>(lc, x, m);
#pragma unroll
    for (int d = 0; d < D; ++d) x[d] = m[d] + lc.s[d] * z[d];
}

// the observation's conditional mean (b_o, s_o: lin_prepare's float64 copies of the row, which widen and narrow exactly)
template <typename T, int D>
__device__ __forceinline__ void linfc_obs_mean(const LinConsts<T>& lc, const LinWork& wk, int O, const T (&x)[D], T (&m)[PF_LIN_MAXO]) {
#pragma unroll
    for (int o = 0; o < PF_LIN_MAXO; ++o) {
        T t = T(0);
        if (o < O) {
            t = (T)wk.bo[o];
#pragma unroll
            for (int d = 0; d < D; ++d) t += lc.Ao[o * D + d] * x[d];
        }
        m[o] = t;
    }
}

// the normals of a thread's IT particles at step h: tape rows (planes of B N numbers) or Philox (forecast_normals for any IT)
template <typename T, int K, int IT>
__device__ __forceinline__ void linfc_normals(const T* __restrict__ tape, int planes, uint64_t seed, uint32_t stream, int h, int64_t plane,
                                              int64_t col0, int64_t left, bool whole, T (&v)[IT][K]) {
    if (tape) {
#pragma unroll
        for (int k = 0; k < IT; ++k)
#pragma unroll
            for (int c = 0; c < K; ++c) v[k][c] = (k < left && c < planes) ? tape[((int64_t)h * planes + c) * plane + col0 + k] : T(0);
        return;
    }
    if (whole) draw_normals<T, K, IT>(seed, stream, (uint32_t)h, (uint64_t)col0, v);
    else draw_normals_ragged<T, K, IT>(seed, stream, (uint32_t)h, (uint64_t)col0, v);
}

// the pivot of column b's sums (ForecastPivot): the input cloud's first particle, moved as a particle whose draw is 0
template <typename T, int D> struct LinFcPivot {
    T xp[D], km[PF_LIN_MAXO];
    __device__ __forceinline__ void start(const T* __restrict__ x, int b, int B, int64_t N) {
#pragma unroll
        for (int d = 0; d < D; ++d) xp[d] = x[((int64_t)d * B + b) * N];
    }
    __device__ __forceinline__ void step(const LinConsts<T>& lc, const LinWork& wk, int O) {
        T zero[D];
#pragma unroll
        for (int d = 0; d < D; ++d) zero[d] = T(0);
        asm volatile("" ::: "memory");
        linfc_move<T, D>(lc, xp, zero);
        linfc_obs_mean<T, D>(lc, wk, O, xp, km);
    }
};

template <typename T, int D, bool COV>
__global__ __launch_bounds__(PF_BLOCK) void k_forecast_linmat_part(const T* __restrict__ params, int O, int H, const T* __restrict__ x,
                                                                   const T* __restrict__ W, const T* __restrict__ z,
                                                                   const T* __restrict__ e, uint64_t seed, double* __restrict__ part,
                                                                   T* __restrict__ x_path, T* __restrict__ y_path, int64_t N, int B) {
    constexpr int MAXO = PF_LIN_MAXO, IT = LinFc<D>::ITEMS, NC = COV ? D * (D - 1) / 2 : 0;
    constexpr int A_X = 1, A_XX = 1 + D, A_M = 1 + 2 * D, A_MM = A_M + MAXO, A_P = A_MM + MAXO, QA = A_P + NC;
    __shared__ LinConsts<T> lc;
    __shared__ LinWork wk;
    __shared__ double red[QA * PF_NWAVES];
    __shared__ T pvx[D], pvk[MAXO];  // the pivot of the current step: kept by the first thread, read by everyone (not in registers)
    const int b = blockIdx.y, tiles = gridDim.x;
    const int NP = PF_LINMAT_ROW_LEN(D, O);
    lin_prepare<T, D>(lc, wk, params + (int64_t)b * NP, O, nullptr, false, false);
    const int64_t plane = (int64_t)B * N;
    const int64_t i0 = ((int64_t)blockIdx.x * PF_BLOCK + threadIdx.x) * IT;
    const int64_t col0 = (int64_t)b * N + i0;
    const int64_t left = N - i0;  // particles of this thread: min(left, IT), none when <= 0
    const bool whole = (N % IT) == 0;
    if (threadIdx.x == 0) {
        LinFcPivot<T, D> pv;
        pv.start(x, b, B, N);
#pragma unroll
        for (int d = 0; d < D; ++d) pvx[d] = pv.xp[d];
    }

    T xv[IT][D];
    double w[IT];
#pragma unroll
    for (int k = 0; k < IT; ++k) {
        const bool on = k < left;
#pragma unroll
        for (int d = 0; d < D; ++d) xv[k][d] = on ? x[((int64_t)d * B + b) * N + i0 + k] : T(0);
        w[k] = on ? (W ? (double)W[col0 + k] : 1.0 / (double)N) : 0.0;
    }

    for (int h = 0; h < H; ++h) {
        T zv[IT][D];
        linfc_normals<T, D, IT>(z, D, seed, PF_STREAM_FORECAST_Z, h, plane, col0, left, whole, zv);
        if (threadIdx.x == 0) {  // (the readers of the last step's pivot are behind block_sum's barriers)
            LinFcPivot<T, D> pv;
#pragma unroll
            for (int d = 0; d < D; ++d) pv.xp[d] = pvx[d];
            pv.step(lc, wk, O);
#pragma unroll
            for (int d = 0; d < D; ++d) pvx[d] = pv.xp[d];
#pragma unroll
            for (int o = 0; o < MAXO; ++o) pvk[o] = pv.km[o];
        }
        __syncthreads();
        double acc[QA];
#pragma unroll
        for (int q = 0; q < QA; ++q) acc[q] = 0.0;
#pragma unroll
        for (int k = 0; k < IT; ++k) {
            // (the constants are re-read from LDS for every particle - broadcast reads - instead of being hoisted into some
            // hundred registers beside the accumulators: the compiler may not assume the LDS unchanged across this point)
            asm volatile("" ::: "memory");
            linfc_move<T, D>(lc, xv[k], zv[k]);
            T m[MAXO];
            linfc_obs_mean<T, D>(lc, wk, O, xv[k], m);
            if (k < left) {  // (a lane without a particle holds arbitrary numbers: it adds and stores nothing)
                acc[0] += w[k];
                double xd[D];
#pragma unroll
                for (int d = 0; d < D; ++d) {
                    xd[d] = (double)xv[k][d] - (double)pvx[d];
                    acc[A_X + d] += w[k] * xd[d];
                    acc[A_XX + d] += w[k] * xd[d] * xd[d];
                    if (x_path) x_path[((int64_t)h * D + d) * plane + col0 + k] = xv[k][d];
                }
                if constexpr (COV) {
#pragma unroll
                    for (int i = 1; i < D; ++i) {
                        const double wi = w[k] * xd[i];
#pragma unroll
                        for (int j = 0; j < i; ++j) acc[A_P + i * (i - 1) / 2 + j] += wi * xd[j];
                    }
                }
#pragma unroll
                for (int o = 0; o < MAXO; ++o) {
                    if (o < O) {
                        const double mo = (double)m[o] - (double)pvk[o], so = wk.so[o];
                        acc[A_M + o] += w[k] * mo;
                        acc[A_MM + o] += w[k] * (mo * mo + so * so);
                    }
                }
                if (y_path) {
                    // the observation noise, one particle at a time: its MAXO numbers start on a call boundary (MAXO is a multiple
                    // of the numbers per call), so the particle's own calls are the aligned ones and none is drawn twice
                    T ev[1][MAXO];
                    linfc_normals<T, MAXO, 1>(e, O, seed, PF_STREAM_FORECAST_E, h, plane, col0 + k, 1, true, ev);
#pragma unroll
                    for (int o = 0; o < MAXO; ++o)
                        if (o < O) y_path[((int64_t)h * O + o) * plane + col0 + k] = m[o] + (T)wk.so[o] * ev[0][o];
                }
            }
        }
        block_sum<QA>(acc, red);
        if (threadIdx.x == 0) {
            const int64_t stride = (int64_t)B * tiles;
            double* row = part + (int64_t)h * linfc_q(D, O, COV) * stride + (int64_t)b * tiles + blockIdx.x;
            row[0] = acc[0];
#pragma unroll
            for (int d = 0; d < D; ++d) {
                row[(1 + d) * stride] = acc[A_X + d];
                row[(1 + D + d) * stride] = acc[A_XX + d];
            }
#pragma unroll
            for (int o = 0; o < MAXO; ++o) {
                if (o < O) {
                    row[(1 + 2 * D + o) * stride] = acc[A_M + o];
                    row[(1 + 2 * D + O + o) * stride] = acc[A_MM + o];
                }
            }
#pragma unroll
            for (int c = 0; c < NC; ++c) row[(1 + 2 * D + 2 * O + c) * stride] = acc[A_P + c];
        }
    }
}

// k_forecast_linmat_final's LDS: the slab rows of its step and filter added over the tiles (the slab's row order), and what its
// first thread hands the threads that form y_cov
struct LinFcFinal {
    double sum[1 + 2 * PF_LIN_MAXD + 2 * PF_LIN_MAXO + PF_LIN_MAXD * (PF_LIN_MAXD - 1) / 2];
    double p[PF_LIN_MAXD * PF_LIN_MAXD], ry[PF_LIN_MAXO];
};

// grid (H, B): the tiles' sums of one step and filter -> x_mean, x_var (H, B, D), y_mean, y_var (H, B, O) and, with COV,
// x_cov (H, B, D, D), y_cov (H, B, O, O)   (params, x: k_forecast_linmat_part's, for the pivots - thread 0 walks the pivot to its step)
// The rows are added one after the other (a run-time loop, one accumulator) and kept in LDS, where a run-time row number may
// index them: nothing here is per-thread state of the size of the slab.
template <typename T, int D, bool COV>
__global__ __launch_bounds__(PF_BLOCK) void k_forecast_linmat_final(const T* __restrict__ params, int O, const T* __restrict__ x,
                                                                    const double* __restrict__ part, T* __restrict__ x_mean,
                                                                    T* __restrict__ x_var, T* __restrict__ y_mean, T* __restrict__ y_var,
                                                                    T* __restrict__ x_cov, T* __restrict__ y_cov, int64_t N, int B, int tiles) {
    constexpr int MAXO = PF_LIN_MAXO;
    __shared__ LinConsts<T> lc;
    __shared__ LinWork wk;
    __shared__ double red[PF_NWAVES];
    __shared__ LinFcFinal fin;
    const int h = blockIdx.x, b = blockIdx.y;
    const int NP = PF_LINMAT_ROW_LEN(D, O);
    lin_prepare<T, D>(lc, wk, params + (int64_t)b * NP, O, nullptr, false, false);
    const int Q = linfc_q(D, O, COV);
    const int R_M = 1 + 2 * D, R_MM = R_M + O, R_P = R_MM + O;  // rows of the slab
    const int64_t stride = (int64_t)B * tiles;
    const double* row = part + (int64_t)h * Q * stride + (int64_t)b * tiles;
#pragma unroll 1
    for (int q = 0; q < Q; ++q) {
        double acc[1] = {0.0};
        for (int t = threadIdx.x; t < tiles; t += PF_BLOCK) acc[0] += row[q * stride + t];
        block_sum<1>(acc, red);
        if (threadIdx.x == 0) fin.sum[q] = acc[0];
    }
    const int64_t hb = (int64_t)h * B + b;
    if (threadIdx.x == 0) {
        // (a pivot that differed from k_forecast_linmat_part's in its last bit would move the mean by that bit and the second
        // moments not at all: c enters mean - c only through c (S0 - 1))
        LinFcPivot<T, D> pv;
        pv.start(x, b, B, N);
        for (int s = 0; s <= h; ++s) pv.step(lc, wk, O);
        const double s0 = fin.sum[0];
        double r[D];
#pragma unroll
        for (int d = 0; d < D; ++d) {
            const double c = (double)pv.xp[d], p1 = fin.sum[1 + d], p2 = fin.sum[1 + D + d];
            r[d] = c * (s0 - 1.0) + p1;  // mean - c  (mean = sum W x: k_moments_final)
            const T var = (T)pivoted_variance(s0, p1, p2, r[d]);
            x_mean[hb * D + d] = (T)(c + r[d]);
            x_var[hb * D + d] = var;
            if constexpr (COV) {
                x_cov[(hb * D + d) * D + d] = var;
                fin.p[d * D + d] = p2;
            }
        }
        if constexpr (COV) {
#pragma unroll
            for (int i = 1; i < D; ++i)
#pragma unroll
                for (int j = 0; j < i; ++j) {
                    const double pij = fin.sum[R_P + i * (i - 1) / 2 + j];
                    const T cov = (T)pivoted_covariance(s0, fin.sum[1 + i], fin.sum[1 + j], pij, r[i], r[j]);
                    x_cov[(hb * D + i) * D + j] = cov;
                    x_cov[(hb * D + j) * D + i] = cov;
                    fin.p[i * D + j] = pij;
                    fin.p[j * D + i] = pij;
                }
        }
#pragma unroll
        for (int o = 0; o < MAXO; ++o) {
            if (o < O) {
                const double k = (double)pv.km[o], m1 = fin.sum[R_M + o];
                const double ry = k * (s0 - 1.0) + m1;
                y_mean[hb * O + o] = (T)(k + ry);
                y_var[hb * O + o] = (T)pivoted_variance(s0, m1, fin.sum[R_MM + o], ry);
                if constexpr (COV) fin.ry[o] = ry;
            }
        }
    }
    if constexpr (COV) {
        __syncthreads();
        const int o = threadIdx.x / MAXO, p = threadIdx.x % MAXO;
        if (o < O && p <= o) {  // one entry of the lower triangle per thread, mirrored; float64 from lin_prepare's copies of the row
            const double s0 = fin.sum[0];
            double pop = 0.0, m1o = 0.0, m1p = 0.0;
            for (int i = 0; i < D; ++i) {
                double v = 0.0;
                for (int j = 0; j < D; ++j) v += fin.p[i * D + j] * wk.Ao[p * D + j];
                pop += wk.Ao[o * D + i] * v;
                m1o += wk.Ao[o * D + i] * fin.sum[1 + i];
                m1p += wk.Ao[p * D + i] * fin.sum[1 + i];
            }
            double cov = pop - fin.ry[o] * m1p - fin.ry[p] * m1o + fin.ry[o] * fin.ry[p] * s0;
            if (o == p) {
                cov += s0 * wk.so[o] * wk.so[o];
                cov = cov < 0.0 ? 0.0 : cov;  // (a NaN stays)
            }
            y_cov[(hb * O + o) * O + p] = (T)cov;
            y_cov[(hb * O + p) * O + o] = (T)cov;
        }
    }
}

}  // namespace pf
