// pf_smooth_mh.hpp - backward simulation by Metropolis-Hastings (Bunch & Godsill 2013, "Improved particle approximations to the
// joint smoothing distribution using Markov chain Monte Carlo"): the O(N K) way between "fl" (ancestor tracing, K = 0) and "ffbs"
// (k_ffbs / k_ffbs_linmat: every trajectory scans all N candidates twice per step, K -> inf).
//
// Per filter column b and trajectory j over a history of S states (layouts of pf_smooth.hpp):
//   k_{S-1} = idx_last[b][j], out[S-1][j] = x_hist[S-1][k_{S-1}];
//   for t = S-2 .. 0, with x+ = out[t+1][j]:
//     start  i = anc_hist[t+1][b][k_{t+1}], l = l_t(i) - or -inf when the candidate's sanitised log-weight is -inf;
//     K rounds, uniforms (u1, u2) each: the proposal i' is the first candidate with cdf_t[i'] > u1 cdf_t[N-1] (none: the last
//            candidate of positive mass - cpu_ref.ffbs_backward_step's convention); accepted iff l = -inf or
//            log(u2) < l_t(i') - l, in T; then i, l <- i', l_t(i');
//     k_t = i, out[t][j] = x_hist[t][k_t], idx_out[t][b][j] = k_t.
//   l_t(i) = sum_d [ -(x+_d - loc_d(x_t^i))^2 / (2 sd_d^2) - log|sd_d| ], sd = scale inc_scale: k_ffbs' logit without the weight and
//   without log sqrt(2 pi).  PF_HID_LINEAR_MAT: the log|sd| term is a constant of the filter and is left out.
//   cdf_t = the inclusive running sum, in double, of exp(sanitised logw_t - max), max and exp in T.
//
// Two kernels.  k_smooth_mh_cdf: one workgroup per (t < S - 1, b) - the column maximum, then a tile-by-tile workgroup scan with a
// running carry into the workspace (S - 1, B, N) of doubles; behind it one int64 per (t, b): the last candidate of positive mass
// (N - 1 when there is none).  The sums are added in another order than a sequential scan adds them: N additions of 2^-53 - and
// the entry of a candidate without mass need not be bit-equal to its predecessor's, so the search's answer is checked (below).
// k_smooth_mh<T, D, MAT>: one lane per trajectory for the whole backward pass, as in k_ffbs.  Per round: one Philox call (or
// two tape reads), a binary search of the cdf column, D gathers of the proposed particle, its one-step mean and the
// log-density.  A chain of dependent loads: latency-bound, hidden by the N B lanes in flight.
//
// Draws: tape u (S - 1, K, 2, B, N) in T - [t][r][0] proposes, [t][r][1] accepts - or Philox: one call per round, call number
// (b N + j) K + r of (seed, PF_STREAM_SMOOTH_MH, step t); float: u1 = u01(word 0), u2 = u01(word 1); double: u01_d(words 0, 1), u01_d(words 2, 3).
#pragma once
#include "pf_linear.hpp"
#include "pf_models.hpp"
#include "pf_philox.hpp"

namespace pf {

// a recorded log-weight as a backward draw takes it: NaN, +inf, -inf and the dtype's lowest finite value are -inf (no mass)
template <typename T> __device__ __forceinline__ T smooth_mh_logw(T v) {
    const T c = sanitize_logw(v);
    return c == Lim<T>::lowest() ? -Lim<T>::inf() : c;
}

// grid ((S - 1) B): workgroup w serves state t = w / B, column b = w % B.  cdf (S - 1, B, N), last_pos (S - 1, B).
template <typename T>
__global__ __launch_bounds__(PF_BLOCK) void k_smooth_mh_cdf(const T* __restrict__ logw_hist, double* __restrict__ cdf,
                                                             int64_t* __restrict__ last_pos, int64_t N) {
    __shared__ T red_m[PF_NWAVES];
    __shared__ double red_s[PF_NWAVES];
    __shared__ int red_l[PF_NWAVES];
    const T* w = logw_hist + (int64_t)blockIdx.x * N;  // (logw_hist (S, B, N): row t B + b)
    double* c = cdf + (int64_t)blockIdx.x * N;
    T m = -Lim<T>::inf();
    for (int64_t i = threadIdx.x; i < N; i += PF_BLOCK) {
        const T v = smooth_mh_logw(w[i]);
        m = v > m ? v : m;
    }
    m = block_max(m, red_m);
    double carry = 0.0;
    int last = -1;  // (N <= 2^30: bad_shape)
    const int64_t tiles = (N + PF_BLOCK - 1) / PF_BLOCK;
    for (int64_t tile = 0; tile < tiles; ++tile) {
        const int64_t i = tile * PF_BLOCK + threadIdx.x;
        const T v = i < N ? smooth_mh_logw(w[i]) : -Lim<T>::inf();
        const double e = v == -Lim<T>::inf() ? 0.0 : (double)pf_exp(v - m);
        if (e > 0.0) last = (int)i;
        double total;
        const double excl = block_scan_excl(e, red_s, total);
        if (i < N) c[i] = carry + (excl + e);
        carry += total;
    }
    // the last candidate of positive mass: the largest index any thread saw
    for (int off = 32; off >= 1; off >>= 1) {
        const int o = __shfl_xor(last, off);
        last = o > last ? o : last;
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red_l[threadIdx.x >> 6] = last;
    __syncthreads();
    if (threadIdx.x == 0) {
        int r = red_l[0];
        for (int k = 1; k < PF_NWAVES; ++k) r = red_l[k] > r ? red_l[k] : r;
        last_pos[blockIdx.x] = r < 0 ? N - 1 : r;
    }
}

// grid (ceil(N / 256), B).  MAT: PF_HID_LINEAR_MAT (row [A D*D | b D | s D | ...], pf_linear.hpp), else a built-in kind of D <= 3.
template <typename T, int D, bool MAT>
__global__ __launch_bounds__(PF_BLOCK) void k_smooth_mh(ModelDesc md, const T* __restrict__ params, const T* __restrict__ x_hist,
                                                         const T* __restrict__ logw_hist, const int32_t* __restrict__ anc_hist,
                                                         const int32_t* __restrict__ idx_last, const T* __restrict__ u, uint64_t seed,
                                                         int K, const double* __restrict__ cdf, const int64_t* __restrict__ last_pos,
                                                         T* __restrict__ out, int32_t* __restrict__ idx_out, int64_t S, int64_t N,
                                                         int B) {
    constexpr int DP = MAT ? 1 : D;  // (ColParams is the built-in kinds' row: D <= 3)
    __shared__ T s_A[MAT ? D * D : 1], s_b[MAT ? D : 1];
    const int b = blockIdx.y;
    const int O = md.obs_dim;
    ColParams<T, DP> cp;
    T i2[D];  // MAT: 1 / (2 s_d^2)
    if constexpr (MAT) {
        const T* row = params + (int64_t)b * PF_LINMAT_ROW_LEN(D, O);
        if (threadIdx.x < D * D) s_A[threadIdx.x] = row[threadIdx.x];
        if (threadIdx.x >= 64 && threadIdx.x < 64 + D) s_b[threadIdx.x - 64] = row[PF_LINMAT_B_AT(D) + threadIdx.x - 64];
#pragma unroll
        for (int d = 0; d < D; ++d) {
            const T sd = row[PF_LINMAT_S_AT(D) + d];
            i2[d] = T(0.5) / (sd * sd);
        }
        __syncthreads();
    } else {
        cp.load(params + (int64_t)b * PF_BUILTIN_ROW_LEN(D, O), O, nullptr);
    }
    const T inc = (T)md.inc_scale;
    const int64_t plane = (int64_t)B * N, col = (int64_t)b * N;
    const int64_t j = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    if (j >= N) return;  // (no workgroup barrier below)
    // an index a caller handed in is held inside the column, whatever it says
    auto inside = [&](int64_t i) { return i < 0 ? (int64_t)0 : (i >= N ? N - 1 : i); };

    int64_t k = inside(idx_last[col + j]);
    T xj[D];
#pragma unroll
    for (int d = 0; d < D; ++d) {
        xj[d] = x_hist[((S - 1) * D + d) * plane + col + k];
        out[((S - 1) * D + d) * plane + col + j] = xj[d];
    }
    if (idx_out) idx_out[(S - 1) * plane + col + j] = (int32_t)k;

    for (int64_t t = S - 2; t >= 0; --t) {
        const T* xt = x_hist + t * D * plane + col;
        const T* wt = logw_hist + t * plane + col;
        const double* ct = cdf + t * plane + col;
        // l_t(i): the log-density of x+ = xj given candidate i of state t, up to a constant of the filter
        auto ell = [&](int64_t i) {
            T xi[D], l = T(0);
#pragma unroll
            for (int d = 0; d < D; ++d) xi[d] = xt[(int64_t)d * plane + i];
            if constexpr (MAT) {
#pragma unroll
                for (int d = 0; d < D; ++d) {
                    T mu = s_A[d * D] * xi[0];
#pragma unroll
                    for (int q = 1; q < D; ++q) mu += s_A[d * D + q] * xi[q];
                    const T r = xj[d] - (s_b[d] + mu);
                    l -= r * r * i2[d];
                }
            } else {
                T loc[D], sc[D];
                mean_scale<T, D>(md, cp, xi, loc, sc);
#pragma unroll
                for (int d = 0; d < D; ++d) {
                    const T sd = sc[d] * inc, r = xj[d] - loc[d];
                    l -= r * r * (T(0.5) / (sd * sd)) + pf_log(pf_abs(sd));
                }
            }
            return l;
        };
        int64_t i = inside(anc_hist[(t + 1) * plane + col + k]);
        T l = smooth_mh_logw(wt[i]) == -Lim<T>::inf() ? -Lim<T>::inf() : ell(i);
        const double total = ct[N - 1];
        const int64_t fallback = inside(last_pos[t * B + b]);
        for (int r = 0; r < K; ++r) {
            T u1, u2;
            if (u) {
                const T* ur = u + ((t * K + r) * 2) * plane + col + j;
                u1 = ur[0];
                u2 = ur[plane];
            } else {
                const uint64_t c = (uint64_t)(col + j) * (uint64_t)K + (uint64_t)r;
                const Philox4 w = philox4x32_10((uint32_t)c, (uint32_t)(c >> 32), (uint32_t)t, PF_STREAM_SMOOTH_MH, (uint32_t)seed,
                                                (uint32_t)(seed >> 32));
                if constexpr (sizeof(T) == 4) {
                    u1 = u01(w.x);
                    u2 = u01(w.y);
                } else {
                    u1 = u01_d(w.x, w.y);
                    u2 = u01_d(w.z, w.w);
                }
            }
            // the first candidate whose running sum exceeds u1 x total
            const double target = (double)u1 * total;
            int64_t lo = 0, hi = N;
            while (lo < hi) {
                const int64_t mid = (lo + hi) >> 1;
                if (ct[mid] > target) hi = mid;
                else lo = mid + 1;
            }
            int64_t ip = fallback;
            if (lo < N) {
                // a candidate without mass owns no interval of the exact cdf, but the workgroup scan adds the prefixes of two
                // neighbours in different groupings and can leave it an ulp: step back to the live candidate it follows
                ip = lo;
                while (ip > 0 && smooth_mh_logw(wt[ip]) == -Lim<T>::inf()) --ip;
            }
            const T lp = ell(ip);
            if (l == -Lim<T>::inf() || pf_log(u2) < lp - l) {
                i = ip;
                l = lp;
            }
        }
        k = i;
#pragma unroll
        for (int d = 0; d < D; ++d) {
            xj[d] = xt[(int64_t)d * plane + k];
            out[(t * D + d) * plane + col + j] = xj[d];
        }
        if (idx_out) idx_out[t * plane + col + j] = (int32_t)k;
    }
}

}  // namespace pf
