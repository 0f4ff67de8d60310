// pf_forecast.hpp - forecasting from a filter state for the built-in model kinds of the stand-alone model kernels: the weighted
// particle cloud walked H moves of the hidden process ahead, with the predictive mean and variance of the state and of the
// observation at every one of them.  In torch that is H x (propagate, build_density, sample, two weighted sums) over full-size
// tensors and a (H, N, [B], [D]) result whether or not anyone wants paths.  Here: ONE launch for the whole horizon - a thread keeps
// PF_FC_ITEMS consecutive particles and their weights in registers and walks them through all H steps - plus one small launch that
// adds the tiles' partial sums.  Nothing particle-sized is written unless paths are asked for.
//
// Per step and particle:   x <- loc(x) + scale(x) * inc * z          (mean_scale / the ColConsts closed forms: Bootstrap's move)
//                          m_o(x), s_o(x): the observation's conditional mean and scale
//                              linear: b + A x, s        stochastic volatility: b, x
// and in double            sum W, sum W (x_d - c_d), sum W (x_d - c_d)^2, sum W (m_o - k_o), sum W ((m_o - k_o)^2 + s_o^2)
// about pivots every tile and launch geometry agrees on (ForecastPivot): c = the INPUT cloud's first particle of the column walked
// the same H moves WITHOUT noise (so it drifts with the cloud: an AR(1) at a level loses 1 % of it per step), k = its image under
// the observation's conditional mean (s_o^2 is a genuine second moment and is not pivoted).  The pivot is a function of the
// parameters and of that one particle alone.  A cloud far from zero keeps its variance to rounding; the subtraction is in double.
// The observation's moments are Rao-Blackwellised (the law of total variance): no observation noise is drawn for them.
// Conventions of k_moments_final: the weights are taken as normalised (no division by sum W): mean = c S0 + P1, the variance
// P2 - 2 (mean - c) P1 + (mean - c)^2 S0 is clamped at 0, a NaN poisons its row.
//
// No per-thread array is indexed by the run-time step or by a run-time dimension (such arrays live in scratch memory): the
// accumulators are per STEP - reduced across the workgroup and stored at the end of each step - not per horizon.  The tiles'
// sums meet in a slab (H, PF_FC_Q, B, tiles) that k_forecast_final adds in a fixed order: no float atomics, the result does not
// depend on scheduling.
//
// Draws: tapes z (H, D, B, N) / e (H, O, B, N), or Philox - standard normal number (b N + i) D + d of stream PF_STREAM_FORECAST_Z at
// counter step h (NormalDraw's addressing: a thread's consecutive particles share calls), and number (b N + i) MAXO + o of
// PF_STREAM_FORECAST_E for the observation noise, which is drawn only when y paths are stored.  A draw is addressed by its
// particle alone, so a result is a function of the seed - not of the tile geometry, and the same with or without paths.
#pragma once

namespace pf {

#define PF_FC_ITEMS 4  // consecutive particles per thread
#define PF_FC_TILE (PF_BLOCK * PF_FC_ITEMS)

// rows of the slab: fixed slots for any (D, O) - k_forecast_part writes, and k_forecast_final reads, the rows of its D and O only
enum { FC_W = 0, FC_X = 1, FC_XX = FC_X + PF_MAXD, FC_M = FC_XX + PF_MAXD, FC_MM = FC_M + PF_MAXO, PF_FC_Q = FC_MM + PF_MAXO };

// one move of the hidden process in place: Bootstrap's branch of sample_and_weight
template <typename T, int D>
__device__ __forceinline__ void forecast_move(const ModelDesc& md, const ColParams<T, D>& cp, const ColConsts<T, D>& cc, T (&x)[D],
                                              const T (&z)[D]) {
    if constexpr (D == 1) {
        if (cc.fast) {
            x[0] = cc.loc1(md, cp, x[0]) + cc.g * (z[0] * cc.inc);
            return;
        }
    }
    T loc[D], scale[D];
    mean_scale<T, D>(md, cp, x, loc, scale);
    const T inc = (T)md.inc_scale;
#pragma unroll
    for (int d = 0; d < D; ++d) x[d] = loc[d] + scale[d] * (z[d] * inc);
}

// the normals of a thread's PF_FC_ITEMS particles at step h: tape rows (planes of B N numbers) or Philox
template <typename T, int K>
__device__ __forceinline__ void forecast_normals(const T* __restrict__ tape, int planes, uint64_t seed, uint32_t stream, int h, int64_t plane,
                                                 int64_t col0, int64_t left, bool whole, T (&v)[PF_FC_ITEMS][K]) {
    if (tape) {
#pragma unroll
        for (int k = 0; k < PF_FC_ITEMS; ++k)
#pragma unroll
            for (int c = 0; c < K; ++c) v[k][c] = (k < left && c < planes) ? tape[((int64_t)h * planes + c) * plane + col0 + k] : T(0);
        return;
    }
    // (whole: N % PF_FC_ITEMS == 0, so every thread starts at a multiple of PF_FC_ITEMS - draw_normals' aligned form)
    if (whole) draw_normals<T, K, PF_FC_ITEMS>(seed, stream, (uint32_t)h, (uint64_t)col0, v);
    else draw_normals_ragged<T, K, PF_FC_ITEMS>(seed, stream, (uint32_t)h, (uint64_t)col0, v);
}

// the pivot of column b's sums: start() reads the input cloud's first particle, step() moves it as forecast_move moves a particle
// whose draw is 0 and takes the observation's conditional mean of it
template <typename T, int D> struct ForecastPivot {
    static constexpr int MAXO = ObsDim<D>::MAXO;
    T xp[D];
    double cx[D], cm[MAXO];
    __device__ __forceinline__ void start(const T* __restrict__ x, int b, int B, int64_t N) {
#pragma unroll
        for (int d = 0; d < D; ++d) xp[d] = x[((int64_t)d * B + b) * N];
    }
    __device__ __forceinline__ void step(const ModelDesc& md, const ColParams<T, D>& cp, const ColConsts<T, D>& cc, bool sv) {
        T zero[D];
#pragma unroll
        for (int d = 0; d < D; ++d) zero[d] = T(0);
        forecast_move<T, D>(md, cp, cc, xp, zero);
#pragma unroll
        for (int d = 0; d < D; ++d) cx[d] = (double)xp[d];
#pragma unroll
        for (int o = 0; o < MAXO; ++o) {
            T lo = cp.ob[o];
#pragma unroll
            for (int d = 0; d < D; ++d) lo += cp.A[o][d] * xp[d];
            cm[o] = (double)(sv ? cp.ob[o] : lo);
        }
    }
};

template <typename T, int D>
__global__ __launch_bounds__(PF_BLOCK) void k_forecast_part(ModelDesc md, const T* __restrict__ params, int H, const T* __restrict__ x,
                                                            const T* __restrict__ W, const T* __restrict__ z, const T* __restrict__ e,
                                                            uint64_t seed, double* __restrict__ part, T* __restrict__ x_path,
                                                            T* __restrict__ y_path, int64_t N, int B) {
    constexpr int MAXO = ObsDim<D>::MAXO, IT = PF_FC_ITEMS, Q = 1 + 2 * D + 2 * MAXO;
    __shared__ double red[Q * PF_NWAVES];
    const int b = blockIdx.y, tiles = gridDim.x;
    const int O = md.obs_dim;
    const int NP = PF_BUILTIN_ROW_LEN(D, O);
    ColParams<T, D> cp;
    cp.load(params + (int64_t)b * NP, O, nullptr);  // (no observation: its entries are 0 and nothing here reads them)
    ColConsts<T, D> cc;
    cc.prepare(md, cp);
    const bool sv = md.obs_kind == PF_OBS_SV;
    const int64_t plane = (int64_t)B * N;
    const int64_t i0 = ((int64_t)blockIdx.x * PF_BLOCK + threadIdx.x) * IT;
    const int64_t col0 = (int64_t)b * N + i0;
    const int64_t left = N - i0;  // particles of this thread: min(left, IT), none when <= 0
    const bool whole = (N % IT) == 0;
    ForecastPivot<T, D> pv;
    pv.start(x, b, B, N);

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
        T zv[IT][D], ev[IT][MAXO];
        forecast_normals<T, D>(z, D, seed, PF_STREAM_FORECAST_Z, h, plane, col0, left, whole, zv);
        if (y_path) forecast_normals<T, MAXO>(e, O, seed, PF_STREAM_FORECAST_E, h, plane, col0, left, whole, ev);
        pv.step(md, cp, cc, sv);
        double acc[Q];
#pragma unroll
        for (int q = 0; q < Q; ++q) acc[q] = 0.0;
#pragma unroll
        for (int k = 0; k < IT; ++k) {
            forecast_move<T, D>(md, cp, cc, xv[k], zv[k]);
            T m[MAXO], s[MAXO];
#pragma unroll
            for (int o = 0; o < MAXO; ++o) {
                T lo = cp.ob[o];
#pragma unroll
                for (int d = 0; d < D; ++d) lo += cp.A[o][d] * xv[k][d];
                m[o] = sv ? cp.ob[o] : lo;
                s[o] = sv ? xv[k][0] : cp.os[o];
            }
            if (k < left) {  // (a lane without a particle holds arbitrary numbers: it adds and stores nothing)
                acc[0] += w[k];
#pragma unroll
                for (int d = 0; d < D; ++d) {
                    const double xd = (double)xv[k][d] - pv.cx[d];
                    acc[1 + d] += w[k] * xd;
                    acc[1 + D + d] += w[k] * xd * xd;
                    if (x_path) x_path[((int64_t)h * D + d) * plane + col0 + k] = xv[k][d];
                }
#pragma unroll
                for (int o = 0; o < MAXO; ++o) {
                    if (o < O) {
                        const double mo = (double)m[o] - pv.cm[o], so = (double)s[o];
                        acc[1 + 2 * D + o] += w[k] * mo;
                        acc[1 + 2 * D + MAXO + o] += w[k] * (mo * mo + so * so);
                        if (y_path) y_path[((int64_t)h * O + o) * plane + col0 + k] = m[o] + s[o] * ev[k][o];
                    }
                }
            }
        }
        block_sum<Q>(acc, red);
        if (threadIdx.x == 0) {
            double* row = part + (int64_t)h * PF_FC_Q * B * tiles + (int64_t)b * tiles + blockIdx.x;
            const int64_t stride = (int64_t)B * tiles;
            row[FC_W * stride] = acc[0];
#pragma unroll
            for (int d = 0; d < D; ++d) {
                row[(FC_X + d) * stride] = acc[1 + d];
                row[(FC_XX + d) * stride] = acc[1 + D + d];
            }
#pragma unroll
            for (int o = 0; o < MAXO; ++o) {
                if (o < O) {
                    row[(FC_M + o) * stride] = acc[1 + 2 * D + o];
                    row[(FC_MM + o) * stride] = acc[1 + 2 * D + MAXO + o];
                }
            }
        }
    }
}

// grid (H, B): the tiles' sums of one step and filter -> x_mean, x_var (H, B, D) and y_mean, y_var (H, B, O)
// (params, x: k_forecast_part's, for the pivots of its sums - thread 0 walks the pivot to its step)
template <typename T, int D>
__global__ __launch_bounds__(PF_BLOCK) void k_forecast_final(ModelDesc md, const T* __restrict__ params, const T* __restrict__ x,
                                                             const double* __restrict__ part, T* __restrict__ x_mean, T* __restrict__ x_var,
                                                             T* __restrict__ y_mean, T* __restrict__ y_var, int64_t N, int B, int tiles) {
    __shared__ double red[PF_FC_Q * PF_NWAVES];
    const int h = blockIdx.x, b = blockIdx.y;
    const int O = md.obs_dim;
    const int64_t stride = (int64_t)B * tiles;
    const double* row = part + (int64_t)h * PF_FC_Q * stride + (int64_t)b * tiles;
    double acc[PF_FC_Q];
#pragma unroll
    for (int q = 0; q < PF_FC_Q; ++q) {
        // (the rows of the components this model has; the others were never written)
        const bool used = q == FC_W || (q < FC_XX ? q - FC_X < D : q < FC_M ? q - FC_XX < D : q < FC_MM ? q - FC_M < O : q - FC_MM < O);
        acc[q] = 0.0;
        if (used)
            for (int t = threadIdx.x; t < tiles; t += PF_BLOCK) acc[q] += row[q * stride + t];
    }
    block_sum<PF_FC_Q>(acc, red);
    if (threadIdx.x == 0) {
        const int64_t hb = (int64_t)h * B + b;
        ColParams<T, D> cp;
        cp.load(params + (int64_t)b * PF_BUILTIN_ROW_LEN(D, O), O, nullptr);
        ColConsts<T, D> cc;
        cc.prepare(md, cp);
        // (a pivot that differed from k_forecast_part's in its last bit would move the mean by that bit and the variance not at
        // all: c enters mean - c only through c (S0 - 1))
        ForecastPivot<T, D> pv;
        pv.start(x, b, B, N);
        for (int s = 0; s <= h; ++s) pv.step(md, cp, cc, md.obs_kind == PF_OBS_SV);
        const double (&cx)[D] = pv.cx;
        const double (&cm)[ObsDim<D>::MAXO] = pv.cm;
#pragma unroll
        for (int d = 0; d < D; ++d) {
            const double r = cx[d] * (acc[FC_W] - 1.0) + acc[FC_X + d];  // mean - c  (mean = sum W x: k_moments_final)
            x_mean[hb * D + d] = (T)(cx[d] + r);
            x_var[hb * D + d] = (T)pivoted_variance(acc[FC_W], acc[FC_X + d], acc[FC_XX + d], r);
        }
#pragma unroll
        for (int o = 0; o < ObsDim<D>::MAXO; ++o) {
            if (o < O) {
                const double r = cm[o] * (acc[FC_W] - 1.0) + acc[FC_M + o];
                const double mu = cm[o] + r;
                const double v = pivoted_variance(acc[FC_W], acc[FC_M + o], acc[FC_MM + o], r);
                y_mean[hb * O + o] = (T)mu;
                y_var[hb * O + o] = (T)v;
            }
        }
    }
}

}  // namespace pf
