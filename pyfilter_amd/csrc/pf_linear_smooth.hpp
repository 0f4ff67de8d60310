// pf_linear_smooth.hpp - PF_HID_LINEAR_MAT after the filter: backward simulation over a recorded history (k_ffbs_linmat) and the
// path score of smoothed trajectories (k_score_linmat_part + k_score_linmat_final).  The model is pf_linear.hpp's:
// x' = b + A x + s e with a full D x D matrix, y ~ N(b_o + A_o x, diag(s_o^2)), 1 <= D, O <= 8, parameter row
// [A D*D | b D | s D | A_o O*D | b_o O | s_o O] (include/pf_amd.h), one row per filter.
//
// k_ffbs_linmat is k_ffbs' scheme (pf_smooth.hpp) with this kind's candidate: one thread per trajectory for the whole backward
// pass, the workgroup stages 256 candidates - loc_i = b + A x_t^i and the sanitised log-weight - in LDS and every thread scans
// the tiles twice, (max, sum exp) and then the inverse-CDF walk with one uniform per (trajectory, step).  s is constant per
// filter: 1 / (2 s_d^2) is a per-filter register value, and -sum log s_d - D log sqrt(2 pi), the same for every candidate, is
// left out of the logits.  The matrix-vector product of the stage is D^2 FMAs per candidate per tile against 256 x 2 D per
// candidate in the scan: it is redone in both passes instead of being kept in planes of memory.  LDS: 256 x (D + 1) values of
// T plus the matrix - 18 KiB at D = 8 in double.
//
// k_score_linmat_part is pf_score.hpp's scheme: one thread per path walks the time axis with x_{t-1} in registers, per-term
// arithmetic in double whatever T, one workgroup reduction after the walk, partial sums to a slab that a second kernel adds
// in a fixed order, the time axis cut by score_plan.  The row has up to NP = 160 slots - 320 VGPRs as double accumulators - so a
// workgroup takes a GROUP of PF_LSCORE_R output rows: rows d of (A_d., b_d, s_d) or rows o of (A_o., b_o, s_o), D + 2
// accumulators each.  The groups are indexed on the grid's third dimension next to the time chunks; a group re-reads the path
// planes (small: they sit in L2 / Infinity Cache).  Transition and observation rows are the same arithmetic:
//     e = (target - off - sum_k M_k src_k) / sc      d M_k = e src_k / sc    d off = e / sc    d sc = (e^2 - 1) / sc
// with (target, src) = (x_{t,d}, x_{t-1}) or (y_o, x_t), and each group adds its own rows' -e^2 / 2 - log sc - log sqrt(2 pi) to
// the value.  Accumulators and states are named by compile-time indices (pf_score.hpp's and pf_forecast.hpp's note): the row a
// group starts at is a run-time value, so the target of a transition row is picked from x_t by a chain of selects, not by an
// index.  An observation row NaN in all its elements contributes no observation term; NaN in only some: every group of the
// filter poisons its sums.
#pragma once
#include "pf_linear.hpp"
#include "pf_score.hpp"

namespace pf {

template <typename T, int D>
__global__ __launch_bounds__(PF_BLOCK) void k_ffbs_linmat(const T* __restrict__ params, int O, const T* __restrict__ x_hist,
                                                           const T* __restrict__ logw_hist, const T* __restrict__ x_last,
                                                           const T* __restrict__ u, uint64_t seed, T* __restrict__ out, int64_t S,
                                                           int64_t N, int B) {
    __shared__ T s_loc[D][PF_BLOCK], s_c[PF_BLOCK], s_A[D * D], s_b[D];
    const int b = blockIdx.y;
    const int NP = PF_LINMAT_ROW_LEN(D, O);
    const T* row = params + (int64_t)b * NP;
    if (threadIdx.x < D * D) s_A[threadIdx.x] = row[threadIdx.x];
    if (threadIdx.x >= 64 && threadIdx.x < 64 + D) s_b[threadIdx.x - 64] = row[PF_LINMAT_B_AT(D) + threadIdx.x - 64];
    T i2[D];  // 1 / (2 s_d^2)
#pragma unroll
    for (int d = 0; d < D; ++d) {
        const T sd = row[PF_LINMAT_S_AT(D) + d];
        i2[d] = T(0.5) / (sd * sd);
    }
    const int64_t plane = (int64_t)B * N;
    const int64_t j = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    const bool on = j < N;
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
        // candidate i of a tile: its one-step mean b + A x_t^i (model.hidden.build_density(state), :112) and its log-weight
        auto stage = [&](int64_t tile) {
            const int64_t i = tile * PF_BLOCK + threadIdx.x;
            T xi[D];
#pragma unroll
            for (int d = 0; d < D; ++d) xi[d] = i < N ? xt[((int64_t)d * B + b) * N + i] : T(0);
#pragma unroll
            for (int d = 0; d < D; ++d) {
                T m = s_A[d * D] * xi[0];
#pragma unroll
                for (int k = 1; k < D; ++k) m += s_A[d * D + k] * xi[k];
                s_loc[d][threadIdx.x] = s_b[d] + m;
            }
            T c = i < N ? sanitize_logw(wt[i]) : -Lim<T>::inf();
            if (c == Lim<T>::lowest()) c = -Lim<T>::inf();  // a -inf weight stays out of the draw
            s_c[threadIdx.x] = c;
        };
        auto logit = [&](int q) {
            T l = s_c[q];
#pragma unroll
            for (int d = 0; d < D; ++d) {
                const T r = xj[d] - s_loc[d][q];
                l -= r * r * i2[d];
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
        if (pick < 0) pick = last_pos;  // u = 1 - eps against a rounded-down total: the last candidate of positive mass
        if (on) {
#pragma unroll
            for (int d = 0; d < D; ++d) {
                xj[d] = xt[((int64_t)d * B + b) * N + pick];
                out[(t * D + d) * plane + (int64_t)b * N + j] = xj[d];
            }
        }
    }
}

// ---- path score ----------------------------------------------------------------------------------------------------------
#define PF_LSCORE_R 2  // output rows per group: 2 (D + 2) + 1 <= 21 double accumulators per thread

// groups of transition rows, of observation rows; slab rows of one group (its share of the value, then its rows' slots)
static inline int lscore_groups(int rows) { return (rows + PF_LSCORE_R - 1) / PF_LSCORE_R; }
static inline int lscore_q(int D) { return 1 + PF_LSCORE_R * (D + 2); }

// grid (tiles, B, chunks * G), G = groups of D + groups of O: group g of chunk c at blockIdx.z = c G + g.
// slab `part` (G, 1 + R (D + 2), B, chunks * tiles).
template <typename T, int D>
__global__ __launch_bounds__(PF_BLOCK) void k_score_linmat_part(const T* __restrict__ params, int O, const T* __restrict__ paths,
                                                                 const T* __restrict__ y, int y_rows, double* __restrict__ part, int S,
                                                                 int len, int groups, int64_t N, int B) {
    constexpr int R = PF_LSCORE_R, Q = 1 + R * (D + 2);
    __shared__ double red[Q * PF_NWAVES];
    const int b = blockIdx.y;
    const int g = (int)blockIdx.z % groups, chunk = (int)blockIdx.z / groups;
    const int gt = (D + R - 1) / R;
    const bool obs = g >= gt;              // (uniform over the workgroup)
    const int r0 = (obs ? g - gt : g) * R;  // the group's first row
    const int lim = obs ? O : D;
    const int NP = PF_LINMAT_ROW_LEN(D, O);
    const T* row = params + (int64_t)b * NP;
    const T* mrow = obs ? row + PF_LINMAT_AO_AT(D) : row;                             // the matrix the rows come from
    const T* orow = obs ? row + PF_LINMAT_AO_AT(D) + O * D : row + PF_LINMAT_B_AT(D);  // ... their offsets (b_o behind A_o)
    const T* srow = orow + lim;                                                       // ... their scales

    double M[R][D], off[R], isc[R], lg[R];
    bool act[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        act[r] = r0 + r < lim;
        const int rr = act[r] ? r0 + r : 0;
#pragma unroll
        for (int k = 0; k < D; ++k) M[r][k] = (double)mrow[rr * D + k];
        off[r] = (double)orow[rr];
        const double sc = (double)srow[rr];
        isc[r] = 1.0 / sc;
        lg[r] = log(sc) + PF_LOG_SQRT_2PI;
    }

    const int64_t plane = (int64_t)B * N;
    const int64_t i = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    const bool on = i < N;
    const int t0 = 1 + chunk * len;
    const int t1 = (t0 + len < S) ? t0 + len : S;
    const T* col = paths + (int64_t)b * N + (on ? i : 0);

    double val = 0.0, gM[R][D], goff[R], gsc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
#pragma unroll
        for (int k = 0; k < D; ++k) gM[r][k] = 0.0;
        goff[r] = gsc[r] = 0.0;
    }
    bool poison = false;  // (uniform over the workgroup: it depends on y alone)

    double xp[D];
#pragma unroll
    for (int d = 0; d < D; ++d) xp[d] = (double)col[((int64_t)(t0 - 1) * D + d) * plane];

    for (int t = t0; t < t1; ++t) {
        double xn[D];
#pragma unroll
        for (int d = 0; d < D; ++d) xn[d] = (double)col[((int64_t)t * D + d) * plane];

        // row t - 1 of y: how much of it is there (every group looks: a half-observed row poisons all of the filter's sums)
        const T* yrow = y + ((int64_t)(t - 1) * y_rows + (y_rows == 1 ? 0 : b)) * O;
        int nans = 0;
#pragma unroll
        for (int o = 0; o < PF_LIN_MAXO; ++o) {
            if (o < O) {
                const T v = yrow[o];
                nans += (v != v) ? 1 : 0;
            }
        }
        if (nans > 0 && nans < O) poison = true;
        const bool use = !obs || nans == 0;
        double src[D];  // what the rows multiply: x_{t-1} (transition) or x_t (observation)
#pragma unroll
        for (int k = 0; k < D; ++k) src[k] = obs ? xn[k] : xp[k];

#pragma unroll
        for (int r = 0; r < R; ++r) {
            // the row's target: x_{t, r0 + r} (selected, not indexed) or y_{r0 + r}
            double tgt = 0.0;
#pragma unroll
            for (int d = 0; d < D; ++d) tgt = (d == r0 + r) ? xn[d] : tgt;
            if (obs) tgt = act[r] ? (double)yrow[r0 + r] : 0.0;
            double loc = off[r];
#pragma unroll
            for (int k = 0; k < D; ++k) loc += M[r][k] * src[k];
            if (use && act[r]) {
                const double is = isc[r], e = (tgt - loc) * is;
                val += -0.5 * e * e - lg[r];
                const double w = e * is;
#pragma unroll
                for (int k = 0; k < D; ++k) gM[r][k] += w * src[k];
                goff[r] += w;
                gsc[r] += (e * e - 1.0) * is;
            }
        }
#pragma unroll
        for (int d = 0; d < D; ++d) xp[d] = xn[d];
    }

    // ---- one reduction over the workgroup, then the group's rows of the slab ----
    double acc[Q];
    acc[0] = on ? val : 0.0;
#pragma unroll
    for (int r = 0; r < R; ++r) {
#pragma unroll
        for (int k = 0; k < D; ++k) acc[1 + r * (D + 2) + k] = on ? gM[r][k] : 0.0;
        acc[1 + r * (D + 2) + D] = on ? goff[r] : 0.0;
        acc[1 + r * (D + 2) + D + 1] = on ? gsc[r] : 0.0;
    }
    block_sum<Q>(acc, red);
    if (threadIdx.x == 0) {
        const int64_t parts = (int64_t)gridDim.x * (gridDim.z / groups);
        const int64_t stride = (int64_t)B * parts;  // between slab rows
        double* out = part + (int64_t)g * Q * stride + (int64_t)b * parts + (int64_t)chunk * gridDim.x + blockIdx.x;
        const double bad = poison ? __builtin_nan("") : 0.0;
#pragma unroll
        for (int q = 0; q < Q; ++q) out[q * stride] = acc[q] + bad;
    }
}

// grid (1 + NP, B): value[b] (q = 0: every group's share, groups in index order) or grad[b][q - 1] (the slab row of the one group
// that holds the slot), divided by N.  Every thread adds its parts in index order and the workgroup's tree is fixed: the same
// shape gives the same bits.
__global__ __launch_bounds__(PF_BLOCK) void k_score_linmat_final(const double* __restrict__ part, double* __restrict__ value,
                                                                  double* __restrict__ grad, int D, int O, int64_t parts, int64_t N,
                                                                  int B) {
    constexpr int R = PF_LSCORE_R;
    __shared__ double red[PF_NWAVES];
    const int q = blockIdx.x, b = blockIdx.y, NP = (int)gridDim.x - 1;
    const int Q = 1 + R * (D + 2), gt = (D + R - 1) / R, groups = gt + (O + R - 1) / R;
    const int64_t stride = (int64_t)B * parts;
    double acc[1] = {0.0};
    if (q == 0) {
        for (int g = 0; g < groups; ++g) {
            const double* row = part + (int64_t)g * Q * stride + (int64_t)b * parts;
            for (int64_t p = threadIdx.x; p < parts; p += PF_BLOCK) acc[0] += row[p];
        }
    } else {
        // slot k of the row [A D*D | b D | s D | A_o O*D | b_o O | s_o O] -> (row of its block, column: 0 .. D - 1, D = offset, D + 1 = scale)
        int k = q - 1, base = 0, rr, c;
        if (k >= PF_LINMAT_AO_AT(D)) {
            k -= PF_LINMAT_AO_AT(D);  // (the observation block [A_o | b_o | s_o] from its own start)
            base = gt;
            if (k < O * D) { rr = k / D; c = k % D; }
            else if (k < O * D + O) { rr = k - O * D; c = D; }
            else { rr = k - O * D - O; c = D + 1; }
        } else {
            if (k < PF_LINMAT_B_AT(D)) { rr = k / D; c = k % D; }
            else if (k < PF_LINMAT_S_AT(D)) { rr = k - PF_LINMAT_B_AT(D); c = D; }
            else { rr = k - PF_LINMAT_S_AT(D); c = D + 1; }
        }
        const int g = base + rr / R, l = 1 + (rr % R) * (D + 2) + c;
        const double* row = part + ((int64_t)g * Q + l) * stride + (int64_t)b * parts;
        for (int64_t p = threadIdx.x; p < parts; p += PF_BLOCK) acc[0] += row[p];
    }
    block_sum<1>(acc, red);
    if (threadIdx.x == 0) {
        const double r = acc[0] / (double)N;
        if (q == 0) value[b] = r;
        else grad[(int64_t)b * NP + (q - 1)] = r;
    }
}

}  // namespace pf
