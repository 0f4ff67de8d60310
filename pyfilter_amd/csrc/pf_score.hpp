// pf_score.hpp - the complete-data log-likelihood of smoothed trajectories and its gradient with respect to the parameter row
// (Fisher's identity: the score of the marginal likelihood is the smoothed expectation of this gradient), for the built-in model
// kinds of the stand-alone model kernels.  The reference differentiates the expression with torch autograd over (S, N, B, D)
// tensors (inference/batch/mcmc/proposals/gradient.py:9-32, particle/base.py:176-210): a forward and a backward pass of ~30 small
// ops, each with a full-size intermediate.  Here: ONE streaming pass - every path element is read once, nothing particle-sized is
// written - plus one small launch that adds the workgroups' partial sums.
//
// paths (S, D, B, N): pf_smooth_ffbs' output.  y (S - 1, By, O), By in {1, B}: row t - 1 observes state t.  Per filter b
//     value[b]   = 1/N sum_j sum_{t=1..S-1} [ log p(x_t^j | x_{t-1}^j) + log p(y_t | x_t^j) ]
//     grad[b][k] = d value[b] / d row[b][k]       row = [ hp0[D] hp1[D] hp2[D] hp3[D] | A[O x D] | b[O] | s[O] ]
// With (loc, scale) = mean_scale(x_{t-1}), s = scale * inc and e = (x_t - loc) / s a transition contributes
//     d / d loc_d = e_d / s_d          d / d scale_d = (e_d^2 - 1) / scale_d
// chained to the kind's d loc / d hp and d scale / d hp (slots a kind never reads keep gradient 0); the linear observation, with
// r_o = y_o - b_o - sum_d A_od x_d:  dA_od = r_o x_d / s_o^2,  db_o = r_o / s_o^2,  ds_o = (r_o^2 / s_o^2 - 1) / s_o;  PF_OBS_SV
// (y ~ N(mu, x)): the b[0] slot alone, (y - mu) / x^2.
// An observation row that is NaN in ALL its elements contributes no observation term (the filters skip it); a row NaN in only
// some of them makes the value and the whole gradient row of the filters it belongs to NaN.
//
// All of the per-term arithmetic is in double, whatever T: the residual x_t - loc cancels (a diffusion moves by a fraction of its
// level per step), and a float loc would put its rounding, amplified by 1 / s^2, into every term.  T is the storage type only.
//
// A thread owns one particle (consecutive threads - consecutive particles: coalesced planes) and walks the time axis with
// x_{t-1} in registers; its accumulators are named per row slot by compile-time indices (no per-thread array is indexed by a
// run-time value: pf_forecast.hpp's note on scratch memory).  The workgroup reduces ONCE, after the walk.  When N * B alone
// cannot fill the chip the time axis is cut into chunks on the grid's third dimension (a chunk re-reads its boundary state):
// score_plan, a function of the shape alone.  The partial sums go to a slab (1 + NP, B, chunks * tiles) that k_score_final adds
// in a fixed order - no float atomics: a result is a function of its inputs and shape, not of scheduling.
#pragma once

namespace pf {

#define PF_SCORE_Q (1 + 4 * PF_MAXD + PF_MAXO * PF_MAXD + 2 * PF_MAXO)  // slab rows of the largest shape: the value + NP slots
#define PF_SCORE_TARGET 1024  // workgroups a launch aims for (four per compute unit) before it stops cutting the time axis
#define PF_SCORE_MINLEN 8     // transitions a chunk holds at least (each chunk re-reads one boundary state)
#define PF_SCORE_MAXCHUNKS 1024

struct ScorePlan {
    int64_t tiles;
    int chunks, len;  // chunk c walks the transitions 1 + c len .. min(S - 1, (c + 1) len)
};
static inline ScorePlan score_plan(int64_t N, int64_t B, int64_t S) {
    ScorePlan p;
    p.tiles = (N + PF_BLOCK - 1) / PF_BLOCK;
    const int64_t steps = S - 1;
    const int64_t want = (PF_SCORE_TARGET + p.tiles * B - 1) / (p.tiles * B);
    const int64_t most = steps / PF_SCORE_MINLEN;  // (floor: evened out below, no chunk but a ragged last one holds fewer)
    int64_t chunks = want < most ? want : most;
    if (chunks > PF_SCORE_MAXCHUNKS) chunks = PF_SCORE_MAXCHUNKS;
    if (chunks < 1) chunks = 1;
    p.len = (int)((steps + chunks - 1) / chunks);
    p.chunks = (int)((steps + p.len - 1) / p.len);
    return p;
}

template <typename T, int D>
__global__ __launch_bounds__(PF_BLOCK) void k_score_part(ModelDesc md, const T* __restrict__ params, const T* __restrict__ paths,
                                                         const T* __restrict__ y, int y_rows, double* __restrict__ part, int S,
                                                         int len, int64_t N, int B) {
    constexpr int MAXO = ObsDim<D>::MAXO, Q = 1 + 4 * D + MAXO * D + 2 * MAXO;
    __shared__ double red[Q * PF_NWAVES];
    const int b = blockIdx.y;
    const int O = md.obs_dim;
    const int NP = PF_BUILTIN_ROW_LEN(D, O);
    const bool sv = md.obs_kind == PF_OBS_SV;
    const int kind = md.hid_kind;
    const double dt = md.dt, inc = md.inc_scale;
    const double kt = log(inc) + PF_LOG_SQRT_2PI;

    // the parameter row in double
    const T* row = params + (int64_t)b * NP;
    double hp[4][D], A[MAXO][D], ob[MAXO], os[MAXO];
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int d = 0; d < D; ++d) hp[k][d] = (double)row[k * D + d];
#pragma unroll
    for (int o = 0; o < MAXO; ++o) {
        const bool on = o < O;
#pragma unroll
        for (int d = 0; d < D; ++d) A[o][d] = on ? (double)row[PF_BUILTIN_AO_AT(D) + o * D + d] : 0.0;
        ob[o] = on ? (double)row[PF_BUILTIN_BO_AT(D, O) + o] : 0.0;
        os[o] = on ? (double)row[PF_BUILTIN_SO_AT(D, O) + o] : 1.0;
    }
    // Ornstein-Uhlenbeck: what depends on the parameters alone - e^{-kappa dt}, sqrt v with v = (1 - e^{-2 kappa dt}) / (2 kappa),
    // d sqrt v / d kappa = (2 kappa dt e^{-2 kappa dt} - (1 - e^{-2 kappa dt})) / (2 kappa^2) / (2 sqrt v)
    double ou_e[D], ou_sv[D], ou_dsv[D];
#pragma unroll
    for (int d = 0; d < D; ++d) {
        ou_e[d] = ou_sv[d] = ou_dsv[d] = 0.0;
        if (kind == PF_HID_OU) {
            const double kappa = hp[0][d], e2 = exp(-2.0 * kappa * dt);
            ou_e[d] = exp(-kappa * dt);
            ou_sv[d] = sqrt((1.0 - e2) / (2.0 * kappa));
            ou_dsv[d] = (2.0 * kappa * dt * e2 - (1.0 - e2)) / (2.0 * kappa * kappa) / (2.0 * ou_sv[d]);
        }
    }

    // every kind but Verhulst has a transition scale that does not depend on the state: its reciprocals and logarithm are
    // evaluated once per thread, not once per term
    const bool fixed = kind != PF_HID_VERHULST_EM;
    const double iinc = 1.0 / inc;
    double f_isc[D], f_lg[D];  // 1 / scale_d, log |scale_d|
#pragma unroll
    for (int d = 0; d < D; ++d) {
        const double sc = kind == PF_HID_LINEAR ? hp[2][d] : kind == PF_HID_SINE_EM ? hp[1][d] : kind == PF_HID_LORENZ63_EM ? hp[3][d]
                                                                                                  : hp[2][d] * ou_sv[d];
        f_isc[d] = fixed ? 1.0 / sc : 0.0;
        f_lg[d] = fixed ? log(fabs(sc)) : 0.0;
    }

    double o_is[MAXO], o_lg[MAXO];  // the linear observation: 1 / s_o, log s_o
#pragma unroll
    for (int o = 0; o < MAXO; ++o) {
        o_is[o] = 1.0 / os[o];
        o_lg[o] = log(os[o]);
    }

    const int64_t plane = (int64_t)B * N;
    const int64_t i = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    const bool on = i < N;
    const int t0 = 1 + (int)blockIdx.z * len;
    const int t1 = (t0 + len < S) ? t0 + len : S;
    const T* col = paths + (int64_t)b * N + (on ? i : 0);

    double val = 0.0, ghp[4][D], gA[MAXO][D], gb[MAXO], gs[MAXO];
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int d = 0; d < D; ++d) ghp[k][d] = 0.0;
#pragma unroll
    for (int o = 0; o < MAXO; ++o) {
#pragma unroll
        for (int d = 0; d < D; ++d) gA[o][d] = 0.0;
        gb[o] = gs[o] = 0.0;
    }
    bool poison = false;  // (uniform over the workgroup: it depends on y alone)

    double xp[D];
#pragma unroll
    for (int d = 0; d < D; ++d) xp[d] = on ? (double)col[((int64_t)(t0 - 1) * D + d) * plane] : 1.0;

    for (int t = t0; t < t1; ++t) {
        double xn[D];
#pragma unroll
        for (int d = 0; d < D; ++d) xn[d] = on ? (double)col[((int64_t)t * D + d) * plane] : 1.0;

        // ---- the transition x_{t-1} -> x_t ----
        double loc[D], cs[D];  // cs: cos(x - gamma) of the sine kind (one argument reduction serves sine and cosine)
        double lz_f[3] = {0.0, 0.0, 0.0};
        switch (kind) {
            case PF_HID_LINEAR:
#pragma unroll
                for (int d = 0; d < D; ++d) loc[d] = hp[0][d] + hp[1][d] * xp[d];
                break;
            case PF_HID_SINE_EM:
#pragma unroll
                for (int d = 0; d < D; ++d) {
                    double sn;
                    sincos(xp[d] - hp[0][d], &sn, &cs[d]);
                    loc[d] = xp[d] + sn * dt;
                }
                break;
            case PF_HID_VERHULST_EM:
#pragma unroll
                for (int d = 0; d < D; ++d) loc[d] = xp[d] + hp[0][d] * (hp[1][d] - xp[d]) * xp[d] * dt;
                break;
            case PF_HID_LORENZ63_EM:
                if constexpr (D == 3) {
                    lz_f[0] = -hp[0][0] * (xp[0] - xp[1]);
                    lz_f[1] = hp[1][0] * xp[0] - xp[1] - xp[0] * xp[2];
                    lz_f[2] = xp[0] * xp[1] - hp[2][0] * xp[2];
#pragma unroll
                    for (int d = 0; d < D; ++d) loc[d] = xp[d] + lz_f[d] * dt;
                } else {
#pragma unroll
                    for (int d = 0; d < D; ++d) loc[d] = 0.0;  // (refused on the host: check_model)
                }
                break;
            default:  // PF_HID_OU
#pragma unroll
                for (int d = 0; d < D; ++d) loc[d] = hp[1][d] + (xp[d] - hp[1][d]) * ou_e[d];
                break;
        }
        double gl[D], gsc[D], lp = 0.0;
#pragma unroll
        for (int d = 0; d < D; ++d) {
            double isc = f_isc[d], lg = f_lg[d];
            if (!fixed) {  // Verhulst: scale = sigma x
                const double sc = hp[2][d] * xp[d];
                isc = 1.0 / sc;
                lg = log(fabs(sc));
            }
            const double is = isc * iinc;  // 1 / (scale inc)
            const double e = (xn[d] - loc[d]) * is;
            lp += -0.5 * e * e - kt - lg;
            gl[d] = e * is;
            gsc[d] = (e * e - 1.0) * isc;
        }
        switch (kind) {
            case PF_HID_LINEAR:
#pragma unroll
                for (int d = 0; d < D; ++d) {
                    ghp[0][d] += gl[d];
                    ghp[1][d] += gl[d] * xp[d];
                    ghp[2][d] += gsc[d];
                }
                break;
            case PF_HID_SINE_EM:
#pragma unroll
                for (int d = 0; d < D; ++d) {
                    ghp[0][d] -= gl[d] * (cs[d] * dt);
                    ghp[1][d] += gsc[d];
                }
                break;
            case PF_HID_VERHULST_EM:
#pragma unroll
                for (int d = 0; d < D; ++d) {
                    ghp[0][d] += gl[d] * ((hp[1][d] - xp[d]) * xp[d] * dt);
                    ghp[1][d] += gl[d] * (hp[0][d] * xp[d] * dt);
                    ghp[2][d] += gsc[d] * xp[d];
                }
                break;
            case PF_HID_LORENZ63_EM:
                if constexpr (D == 3) {
                    ghp[0][0] -= gl[0] * ((xp[0] - xp[1]) * dt);
                    ghp[1][0] += gl[1] * (xp[0] * dt);
                    ghp[2][0] -= gl[2] * (xp[2] * dt);
#pragma unroll
                    for (int d = 0; d < D; ++d) ghp[3][d] += gsc[d];
                }
                break;
            default:  // PF_HID_OU: kappa enters loc and scale
#pragma unroll
                for (int d = 0; d < D; ++d) {
                    ghp[0][d] += gsc[d] * (hp[2][d] * ou_dsv[d]) - gl[d] * ((xp[d] - hp[1][d]) * dt * ou_e[d]);
                    ghp[1][d] += gl[d] * (1.0 - ou_e[d]);
                    ghp[2][d] += gsc[d] * ou_sv[d];
                }
                break;
        }

        // ---- the observation of x_t: row t - 1 of y ----
        const T* yrow = y + ((int64_t)(t - 1) * y_rows + (y_rows == 1 ? 0 : b)) * O;
        double yv[MAXO];
        int nans = 0;
#pragma unroll
        for (int o = 0; o < MAXO; ++o) {
            yv[o] = (o < O) ? (double)yrow[o] : 0.0;
            nans += (o < O && yv[o] != yv[o]) ? 1 : 0;
        }
        if (nans == 0) {
            if (sv) {
                const double r = yv[0] - ob[0], ix = 1.0 / xn[0];
                lp += -0.5 * (r * ix) * (r * ix) - log(xn[0]) - PF_LOG_SQRT_2PI;
                gb[0] += r * ix * ix;
            } else {
#pragma unroll
                for (int o = 0; o < MAXO; ++o) {
                    if (o < O) {
                        double r = yv[o] - ob[o];
#pragma unroll
                        for (int d = 0; d < D; ++d) r -= A[o][d] * xn[d];
                        const double is = o_is[o], z = r * is;
                        lp += -0.5 * z * z - o_lg[o] - PF_LOG_SQRT_2PI;
                        const double w = z * is;  // r / s^2
#pragma unroll
                        for (int d = 0; d < D; ++d) gA[o][d] += w * xn[d];
                        gb[o] += w;
                        gs[o] += (z * z - 1.0) * is;
                    }
                }
            }
        } else if (nans < O) {
            poison = true;
        }
        val += lp;
#pragma unroll
        for (int d = 0; d < D; ++d) xp[d] = xn[d];
    }

    // ---- one reduction over the workgroup, then its row of the slab ----
    double acc[Q];
    acc[0] = on ? val : 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int d = 0; d < D; ++d) acc[1 + k * D + d] = on ? ghp[k][d] : 0.0;
#pragma unroll
    for (int o = 0; o < MAXO; ++o) {
#pragma unroll
        for (int d = 0; d < D; ++d) acc[1 + 4 * D + o * D + d] = on ? gA[o][d] : 0.0;
        acc[1 + 4 * D + MAXO * D + o] = on ? gb[o] : 0.0;
        acc[1 + 4 * D + MAXO * D + MAXO + o] = on ? gs[o] : 0.0;
    }
    block_sum<Q>(acc, red);
    if (threadIdx.x == 0) {
        const int64_t parts = (int64_t)gridDim.x * gridDim.z;
        const int64_t stride = (int64_t)B * parts;  // between slab rows
        double* out = part + (int64_t)b * parts + (int64_t)blockIdx.z * gridDim.x + blockIdx.x;
        const double bad = poison ? __builtin_nan("") : 0.0;
        out[0] = acc[0] + bad;
#pragma unroll
        for (int q = 0; q < 4 * D; ++q) out[(1 + q) * stride] = acc[1 + q] + bad;
#pragma unroll
        for (int o = 0; o < MAXO; ++o) {
            if (o < O) {
#pragma unroll
                for (int d = 0; d < D; ++d) out[(1 + 4 * D + o * D + d) * stride] = acc[1 + 4 * D + o * D + d] + bad;
                out[(1 + 4 * D + O * D + o) * stride] = acc[1 + 4 * D + MAXO * D + o] + bad;
                out[(1 + 4 * D + O * D + O + o) * stride] = acc[1 + 4 * D + MAXO * D + MAXO + o] + bad;
            }
        }
    }
}

// grid (1 + NP, B): slab row q of filter b -> value[b] (q = 0) or grad[b][q - 1], divided by N.  Every thread adds its parts in
// index order and the workgroup's tree is fixed: the same shape gives the same bits.
__global__ __launch_bounds__(PF_BLOCK) void k_score_final(const double* __restrict__ part, double* __restrict__ value,
                                                          double* __restrict__ grad, int64_t parts, int64_t N, int B) {
    __shared__ double red[PF_NWAVES];
    const int q = blockIdx.x, b = blockIdx.y, NP = (int)gridDim.x - 1;
    const double* row = part + ((int64_t)q * B + b) * parts;
    double acc[1] = {0.0};
    for (int64_t p = threadIdx.x; p < parts; p += PF_BLOCK) acc[0] += row[p];
    block_sum<1>(acc, red);
    if (threadIdx.x == 0) {
        const double r = acc[0] / (double)N;
        if (q == 0) value[b] = r;
        else grad[(int64_t)b * NP + (q - 1)] = r;
    }
}

}  // namespace pf
