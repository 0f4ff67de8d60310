// pf_jitter.hpp - the parameter mutation of NESS (Crisan & Miguez' nested particle filter) as two small kernels.
//
// An update of the online algorithm (pyfilter/inference/sequential/kernels/online.py:29-45) resamples the B theta-particles,
// fits a jittering kernel to the weighted particles (kernels/jittering.py:51-89 `robust_var`, :141-225 the kernel families) and
// moves every particle to its ancestor's location plus std * eps (jittering.py:14-26 `_jitter`), through the priors' bijections
// into the parameter tensors the model holds.  As torch operations that is a sort per parameter, a cumsum, two argmin, gathers,
// a diag, masked writes and the bijections - several dozen launches of a few microseconds each next to a filter move of one
// launch.  Here: pf_jitter_fit (one workgroup per parameter: weights, ESS, mean, variance, the two quartiles of the robust
// variance out of an LDS sort) and pf_jitter_apply (one thread per theta-particle).  Conventions of pf_theta.hpp: all arithmetic
// in double whatever the tensors' type, values read and written in the caller's type; what the two kernels hand each other
// (mean, scale, clamped std, ESS per parameter) stays in double, so a result is rounded to the caller's type exactly once.
#pragma once

namespace pf {

// sorted order of the LDS sort: ascending values, NaN last, equal values in the order of their index - the order of a STABLE
// sort, so that the weights of tied values accumulate in one defined order (the quartile pick reads the running sum)
__device__ __forceinline__ bool jitter_before(double a, int ia, double b, int ib) {
    const bool an = a != a, bn = b != b;
    if (an || bn) return an == bn ? ia < ib : bn;
    return a < b || (a == b && ia < ib);
}

// One workgroup per parameter p.  fit (4, P) doubles <- row 0: weighted mean, row 1: scale (bandwidth factor * robust standard
// deviation - the second value `JitterKernel.fit` returns), row 2: std = max(scale, min_std) (`scale.clamp(min_std, INFTY)`,
// jittering.py:131), row 3: ESS of the weights.  mean_out / scale_out (P, the caller's type, or null): rows 0 and 1 once more.
//   weights: pyfilter.utils.normalize of logw exactly as k_theta_fit has it (NaN / +inf carry none; nothing finite: equal weights)
//   robust variance (jittering.py:51-89): the column sorted, the weights accumulated in sorted order, the FIRST index that
//   minimises |cdf - 0.25| and likewise 0.75; iqr = (x_hi - x_lo) / 1.349; var <- iqr^2 where iqr^2 <= var.
// kind PF_JITTER_CONSTANT: scale = par, or scale_in[p] when given (no statistics needed: nothing is sorted).
// Dynamic LDS: next_pow2(B) * 12 bytes (a double and an int per particle; B <= PF_JITTER_MAXB = 8192: 96 KiB).
template <typename T>
__global__ __launch_bounds__(PF_BLOCK) void k_jitter_fit(const T* __restrict__ values, const T* __restrict__ logw, int B, int P, int n2,
                                                         int kind, double par, const T* __restrict__ scale_in, double min_std,
                                                         double bw_lo, double bw_hi, double* __restrict__ fit,
                                                         T* __restrict__ mean_out, T* __restrict__ scale_out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char pfj_lds[];
    __shared__ double red[4 * PF_NWAVES];
    __shared__ double redm[PF_NWAVES];
    __shared__ double best_d[2 * PF_BLOCK];
    __shared__ int best_i[2 * PF_BLOCK];
    const int p = blockIdx.x, tid = threadIdx.x;
    auto finish = [&](double mean, double scale, double ess) {
        fit[p] = mean;
        fit[P + p] = scale;
        fit[2 * P + p] = scale < min_std ? min_std : scale;  // (clamp: a NaN scale stays NaN, as torch's clamp leaves it)
        fit[3 * P + p] = ess;
        if (mean_out) mean_out[p] = (T)mean;
        if (scale_out) scale_out[p] = (T)scale;
    };
    if (kind == PF_JITTER_CONSTANT) {
        if (tid == 0) finish(0.0, scale_in ? (double)scale_in[p] : par, 0.0);
        return;
    }
    double mx = -__builtin_huge_val();
    for (int i = tid; i < B; i += PF_BLOCK) {
        const double v = (double)logw[i];
        const double s = (v != v || v == __builtin_huge_val()) ? -__builtin_huge_val() : v;
        mx = s > mx ? s : mx;
    }
    mx = block_max<double>(mx, redm);
    const bool uniform = !(mx > -__builtin_huge_val());
    auto weight = [&](int i) -> double {
        if (uniform) return 1.0;
        const double v = (double)logw[i];
        return (v != v || v == __builtin_huge_val()) ? 0.0 : exp(v - mx);
    };
    double acc[3] = {0.0, 0.0, 0.0};  // sum w, sum w^2, sum w x
    for (int i = tid; i < B; i += PF_BLOCK) {
        const double w = weight(i);
        acc[0] += w;
        acc[1] += w * w;
        acc[2] += w * (double)values[(int64_t)i * P + p];
    }
    block_sum<3>(acc, red);
    const double wsum = acc[0];
    const double ess = 1.0 / (acc[1] / (wsum * wsum));
    const double mean = acc[2] / wsum;
    double sq[1] = {0.0};
    for (int i = tid; i < B; i += PF_BLOCK) {
        const double c = (double)values[(int64_t)i * P + p] - mean;
        sq[0] += (weight(i) / wsum) * c * c;
    }
    __syncthreads();
    block_sum<1>(sq, red);
    double var = sq[0];

    // the column and its indices in LDS, padded to a power of two with entries that sort behind everything; bitonic sort
    double* sv = reinterpret_cast<double*>(pfj_lds);
    int* si = reinterpret_cast<int*>(pfj_lds + (size_t)n2 * sizeof(double));
    for (int i = tid; i < n2; i += PF_BLOCK) {
        sv[i] = i < B ? (double)values[(int64_t)i * P + p] : __builtin_nan("");
        si[i] = i;
    }
    __syncthreads();
    for (int k = 2; k <= n2; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < (n2 >> 1); t += PF_BLOCK) {
                const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;  // (lo < hi < n2: n2 is a power of two)
                const bool up = (lo & k) == 0;
                const double a = sv[lo], b = sv[hi];
                const int ia = si[lo], ib = si[hi];
                if (jitter_before(b, ib, a, ia) == up) {
                    sv[lo] = b;
                    sv[hi] = a;
                    si[lo] = ib;
                    si[hi] = ia;
                }
            }
            __syncthreads();
        }
    }
    // the running sum of the normalised weights in sorted order (contiguous chunk per thread) and, on the way, the first index
    // that minimises |cdf - q| for both quartiles
    const int chunk = (B + PF_BLOCK - 1) / PF_BLOCK;
    const int c0 = tid * chunk < B ? tid * chunk : B, c1 = c0 + chunk < B ? c0 + chunk : B;
    double local = 0.0;
    for (int j = c0; j < c1; ++j) local += weight(si[j]) / wsum;
    double total;
    double run = block_scan_excl(local, red, total);
    double d_lo = __builtin_huge_val(), d_hi = __builtin_huge_val();
    int i_lo = 0x7fffffff, i_hi = 0x7fffffff;
    for (int j = c0; j < c1; ++j) {
        const double before = run;
        run += weight(si[j]) / wsum;
        // (a particle whose weight does not move the running sum repeats its predecessor's cdf, so it is never the FIRST
        // minimiser - unless it has no predecessor; skipped, because across a chunk boundary the predecessor's sum and this
        // thread's starting offset are equal only up to rounding)
        if (run == before && j > 0) continue;
        const double a = fabs(run - 0.25), b = fabs(run - 0.75);
        if (a < d_lo) {
            d_lo = a;
            i_lo = j;
        }
        if (b < d_hi) {
            d_hi = b;
            i_hi = j;
        }
    }
    best_d[tid] = d_lo;
    best_i[tid] = i_lo;
    best_d[PF_BLOCK + tid] = d_hi;
    best_i[PF_BLOCK + tid] = i_hi;
    __syncthreads();
    if (tid == 0) {
        int q[2];
        for (int h = 0; h < 2; ++h) {  // (the threads' chunks are in index order: a strict `<` keeps the first minimiser)
            double d = __builtin_huge_val();
            int at = 0;
            for (int t = 0; t < PF_BLOCK; ++t)
                if (best_d[h * PF_BLOCK + t] < d) {
                    d = best_d[h * PF_BLOCK + t];
                    at = best_i[h * PF_BLOCK + t];
                }
            q[h] = at < B ? at : 0;
        }
        const double iqr = (sv[q[1]] - sv[q[0]]) / 1.349;
        const double iqr2 = iqr * iqr;
        if (iqr2 <= var) var = iqr2;
        double bw = 1.59 * pow(ess, -1.0 / 3.0);  // (1.59 * ess ** (-1 / 3)).clamp(EPS, 1 - EPS), jittering.py:160
        bw = bw < bw_lo ? bw_lo : (bw > bw_hi ? bw_hi : bw);
        const double fac = kind == PF_JITTER_LIUWEST ? sqrt(1.0 - par * par) : bw;
        finish(mean, fac * sqrt(var), ess);
    }
}

struct JitterDraws {  // where the draws of one update come from
    const void* eps;     // (B, P) standard normals of the caller's type - or null: Philox
    const void* select;  // (B) the Bernoulli draws (0 / 1) of `discrete` - or null: Philox
    unsigned long long seed, counter;  // Philox key and the update counter
};

// One thread per theta-particle i with ancestor j = anc[i] (online.py:29-45 around jittering.py:119-133):
//   location (P): x[j] (non-shrinking, constant) | mean + beta (x[j] - mean), beta = sqrt(1 - bw^2) (shrinking) |
//                 a x[j] + (1 - a) mean (Liu-West)
//   u = location + std * eps;   discrete: u = (1 - s) x[j] + s u with s ~ Bernoulli(prob)
//   u_out (B, P) <- u;  x_out[p] (B) <- the prior's bijection of u (theta_prior).
// Draws without tapes: Philox keyed by the seed, counter words (particle, parameter, update counter) - eps from the first two
// 53-bit uniforms of a call (Box-Muller in double), the Bernoulli uniform of particle i from the call of "parameter" P.
template <typename T>
__global__ __launch_bounds__(PF_BLOCK) void k_jitter_apply(ThetaPriors pr, const T* __restrict__ values, const int64_t* __restrict__ anc,
                                                           const double* __restrict__ fit, int B, int kind, double par, double bw_lo,
                                                           double bw_hi, int discrete, double prob, JitterDraws dr,
                                                           T* __restrict__ u_out, ThetaOut out) {
    const int i = blockIdx.x * PF_BLOCK + threadIdx.x;
    if (i >= B) return;
    const int P = pr.P;
    int64_t j = anc[i];
    j = j < 0 ? 0 : (j >= B ? B - 1 : j);  // (a caller's index tensor: never outside the values)
    const T* eps = reinterpret_cast<const T*>(dr.eps);
    const T* sel = reinterpret_cast<const T*>(dr.select);
    auto philox = [&](uint32_t q) {
        return philox4x32_10((uint32_t)i, q, (uint32_t)dr.counter, PF_STREAM_JITTER ^ (uint32_t)(dr.counter >> 32), (uint32_t)dr.seed,
                             (uint32_t)(dr.seed >> 32));
    };
    double s = 1.0;
    if (discrete) {
        if (sel) {
            s = (double)sel[i];
        } else {
            const Philox4 r = philox((uint32_t)P);
            s = u01_d(r.x, r.y) < prob ? 1.0 : 0.0;
        }
    }
#pragma unroll
    for (int p = 0; p < PF_THETA_MAXP; ++p) {
        if (p < P) {
            const double xj = (double)values[j * P + p];
            const double mean = fit[p], std = fit[2 * P + p];
            double loc = xj;
            if (kind == PF_JITTER_SHRINKING) {
                double bw = 1.59 * pow(fit[3 * P + p], -1.0 / 3.0);
                bw = bw < bw_lo ? bw_lo : (bw > bw_hi ? bw_hi : bw);
                loc = mean + sqrt(1.0 - bw * bw) * (xj - mean);
            } else if (kind == PF_JITTER_LIUWEST) {
                loc = xj * par + (1.0 - par) * mean;
            }
            double e;
            if (eps) {
                e = (double)eps[(int64_t)i * P + p];
            } else {
                const Philox4 r = philox((uint32_t)p);
                double e1;
                box_muller(u01_open0_d(r.x, r.y), u01_d(r.z, r.w), e, e1);
            }
            double u = loc + std * e;
            if (discrete) u = (1.0 - s) * xj + s * u;
            double x, lp;
            theta_prior<T>(pr.kind[p], pr.a[p], pr.b[p], u, x, lp);
            u_out[(int64_t)i * P + p] = (T)u;
            reinterpret_cast<T*>(out.x[p])[i] = (T)x;
        }
    }
}

}  // namespace pf
