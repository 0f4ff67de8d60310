// pf_smooth.hpp - the smoothing kernels of the built-in model kinds: k_trace_ancestors ("fl") and k_ffbs ("ffbs").  Their
// PF_HID_LINEAR_MAT counterpart is pf_linear_smooth.hpp's k_ffbs_linmat, the O(N K) method pf_smooth_mh.hpp.
#pragma once
#include "pf_models.hpp"
#include "pf_philox.hpp"

namespace pf {

// ---------------------------------------------------------------------------------------------------------------
// smoothing over a recorded state history (pyfilter/filters/particle/base.py:105-157), S states, time-major:
//   x_hist (S, D, B, N), logw_hist / anc_hist (S, B, N); anc_hist[t] = the ancestors in state t - 1 of state t's particles.
// ---------------------------------------------------------------------------------------------------------------

// "fl" (_do_sample_fl, :136-152): every particle of the last state walks its ancestral line backwards.  One thread per
// trajectory; the walk is a chain of dependent gathers (latency-bound, N B chains in flight hide it).
template <typename T>
__global__ __launch_bounds__(PF_BLOCK) void k_trace_ancestors(const T* __restrict__ x_hist,
                                                              const int32_t* __restrict__ anc_hist, T* __restrict__ out,
                                                              int64_t S, int64_t N, int B, int D) {
    const int b = blockIdx.y;
    const int64_t plane = (int64_t)B * N;
    for (int64_t i = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x; i < N; i += (int64_t)gridDim.x * PF_BLOCK) {
        int64_t idx = i;
        for (int64_t t = S - 1; t >= 0; --t) {
            for (int d = 0; d < D; ++d)
                out[(t * D + d) * plane + (int64_t)b * N + i] = x_hist[(t * D + d) * plane + (int64_t)b * N + idx];
            if (t > 0) idx = anc_hist[t * plane + (int64_t)b * N + idx];
        }
    }
}

// "ffbs" (_do_sample_ffbs, :105-134): backward simulation.  Trajectory j holds x_{t+1}^{(j)} and draws its state-t particle
// from Categorical(logits_i = logw_t^{(i)} + log p(x_{t+1}^{(j)} | x_t^{(i)})) - an N x N evaluation per step that the
// reference materialises as an (N, N, [B]) tensor.  Here: one thread per trajectory for the WHOLE backward pass
// (trajectories are independent given the recorded states); the workgroup stages 256 candidates (one-step mean, scale and
// weight of particle i) in LDS and every thread scans them twice - (max, sum exp) of its logits, then the inverse-CDF walk
// with ONE uniform per (trajectory, step) (tape `u` (S - 1, B, N) or Philox).  O(N^2 S) flops, O(N S) memory.
template <typename T, int D>
__global__ __launch_bounds__(PF_BLOCK) void k_ffbs(ModelDesc md, const T* __restrict__ params, const T* __restrict__ x_hist,
                                                    const T* __restrict__ logw_hist, const T* __restrict__ x_last,
                                                    const T* __restrict__ u, uint64_t seed, T* __restrict__ out, int64_t S,
                                                    int64_t N, int B) {
    __shared__ T s_loc[D][PF_BLOCK], s_i2[D][PF_BLOCK], s_c[PF_BLOCK];
    const int b = blockIdx.y;
    const int O = md.obs_dim;
    const int NP = PF_BUILTIN_ROW_LEN(D, O);
    ColParams<T, D> cp;
    cp.load(params + (int64_t)b * NP, O, nullptr);
    const int64_t plane = (int64_t)B * N;
    const int64_t j = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    const bool on = j < N;
    const T inc = (T)md.inc_scale;
    T xj[D];
#pragma unroll
    for (int d = 0; d < D; ++d) {
        xj[d] = on ? x_last[((int64_t)d * B + b) * N + j] : T(0);
        if (on) out[((S - 1) * D + d) * plane + (int64_t)b * N + j] = xj[d];
    }
    const int64_t tiles = (N + PF_BLOCK - 1) / PF_BLOCK;
    for (int64_t t = S - 2; t >= 0; --t) {
        const T* xt = x_hist + t * D * plane;
        const T* wt = logw_hist + t * plane + (int64_t)b * N;
        // candidate i of a tile: its one-step mean / scale (model.hidden.build_density(state), :112) and its log-weight
        auto stage = [&](int64_t tile) {
            const int64_t i = tile * PF_BLOCK + threadIdx.x;
            T xi[D], loc[D], sc[D];
#pragma unroll
            for (int d = 0; d < D; ++d) xi[d] = i < N ? xt[((int64_t)d * B + b) * N + i] : T(0);
            mean_scale<T, D>(md, cp, xi, loc, sc);
            T c = i < N ? sanitize_logw(wt[i]) : -Lim<T>::inf();
            if (c == Lim<T>::lowest()) c = -Lim<T>::inf();  // a -inf weight stays out of the draw
#pragma unroll
            for (int d = 0; d < D; ++d) {
                const T sd = sc[d] * inc;
                s_loc[d][threadIdx.x] = loc[d];
                s_i2[d][threadIdx.x] = T(0.5) / (sd * sd);
                c -= pf_log(pf_abs(sd)) + T(PF_LOG_SQRT_2PI);
            }
            s_c[threadIdx.x] = c;
        };
        auto logit = [&](int q) {
            T l = s_c[q];
#pragma unroll
            for (int d = 0; d < D; ++d) {
                const T r = xj[d] - s_loc[d][q];
                l -= r * r * s_i2[d][q];
            }
            return l;
        };
        // pass 1: running (max, sum exp) over all candidates
        T m = -Lim<T>::inf();
        double ssum = 0.0;
        for (int64_t tile = 0; tile < tiles; ++tile) {
            __syncthreads();
            stage(tile);
            __syncthreads();
            const int cnt = (int)((tile + 1) * PF_BLOCK <= N ? PF_BLOCK : N - tile * PF_BLOCK);
            for (int q = 0; q < cnt; ++q) {
                const T l = logit(q);
                if (l > m) {
                    ssum = (m == -Lim<T>::inf()) ? 0.0 : ssum * (double)pf_exp(m - l);
                    m = l;
                }
                if (l != -Lim<T>::inf()) ssum += (double)pf_exp(l - m);
            }
        }
        // pass 2: inverse CDF - the first candidate whose running sum reaches u * total
        T uj;
        if (u) uj = on ? u[t * plane + (int64_t)b * N + j] : T(0);
        else uj = uniform_draw<T>(seed, PF_STREAM_SMOOTH, (uint32_t)t, (uint64_t)((int64_t)b * N + (on ? j : 0)));
        const double target = (double)uj * ssum;
        double run = 0.0;
        int64_t pick = -1, last_pos = 0;
        for (int64_t tile = 0; tile < tiles; ++tile) {
            __syncthreads();
            stage(tile);
            __syncthreads();
            const int cnt = (int)((tile + 1) * PF_BLOCK <= N ? PF_BLOCK : N - tile * PF_BLOCK);
            for (int q = 0; q < cnt; ++q) {
                const T l = logit(q);
                if (l != -Lim<T>::inf()) {
                    const double e = (double)pf_exp(l - m);
                    if (e > 0.0) last_pos = tile * PF_BLOCK + q;
                    run += e;
                    if (pick < 0 && run > target) pick = tile * PF_BLOCK + q;
                }
            }
        }
        if (pick < 0) pick = last_pos;  // u = 1 - eps against a rounded-down total
        if (on) {
#pragma unroll
            for (int d = 0; d < D; ++d) {
                xj[d] = xt[((int64_t)d * B + b) * N + pick];
                out[(t * D + d) * plane + (int64_t)b * N + j] = xj[d];
            }
        }
    }
}

}  // namespace pf
