// pf_search.hpp - the ancestor search both the stand-alone resampler (pf_kernels.hip) and the fused kernels (pf_fused.hpp, pf_column.hpp,
// pf_cluster.hpp) are built on: lower bounds over a cdf, the systematic grid and its closed-form inversion, the LDS window search.
#pragma once
#include "pf_device.hpp"

namespace pf {

// ---------------------------------------------------------------------------------------------------------------
// wave-cooperative lower_bound over a non-decreasing array: first j in [0, n) with c[j] >= p (clamped to n-1).
// 64-ary search: each round the 64 lanes probe 64 equally spaced elements and a ballot picks the sub-range.
// ---------------------------------------------------------------------------------------------------------------
template <typename T> __device__ __forceinline__ int wave_lower_bound(const T* __restrict__ c, int n, T p, int lane) {
    int lo = 0, hi = n;
    while (hi - lo > PF_WAVE) {
        const int len = hi - lo;
        const int step = (len + PF_WAVE - 1) / PF_WAVE;
        int probe = lo + (lane + 1) * step - 1;
        if (probe > hi - 1) probe = hi - 1;
        const bool ge = c[probe] >= p;
        const unsigned long long bal = __ballot(ge);
        if (bal == 0ull) return n - 1;  // p above every element (or NaNs): clamp
        const int f = __ffsll((long long)bal) - 1;
        int nhi = lo + (f + 1) * step;
        if (nhi > hi) nhi = hi;
        lo = lo + f * step;
        hi = nhi;
    }
    const int idx = lo + lane;
    const bool ge = (idx < hi) ? (c[idx] >= p) : true;
    const unsigned long long bal = __ballot(ge);
    const int f = __ffsll((long long)bal) - 1;
    int r = lo + f;
    return r > n - 1 ? n - 1 : r;
}

// plain per-thread lower_bound on global memory in [lo, hi)
template <typename T> __device__ __forceinline__ int thread_lower_bound(const T* __restrict__ c, int lo, int hi, T p) {
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (c[mid] < p) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// searchsorted position of the systematic grid: (i + u) / N evaluated exactly as resampling.py:44-46 does in T
template <typename T> __device__ __forceinline__ T grid_position(int64_t i, T u, T n_as_t) { return (T(i) + u) / n_as_t; }

// ---------------------------------------------------------------------------------------------------------------
// The systematic grid inverted: K(c) = #{ i in [0, N) : grid_position(i) <= c }.  With it the ancestor of position i is
// the entry j with K(cdf_{j-1}) <= i < K(cdf_j) - the same relation searchsorted(side=left) defines - and no search
// is needed: every cdf entry computes its own offspring range in closed form (branch-free, so weight degeneracy does
// not make lanes diverge).  Exactness: the candidate floor(c N - u) + 1 is at most one off the true K (both the fma
// and the rounding of grid_position move the decision for at most one i while N * eps <= 1/4, i.e. N <= 2^22 in
// float, any N in double), so evaluating the grid position - with exactly the arithmetic of grid_position - at the two
// neighbouring indices settles it.  Larger float grids walk from the candidate to the exact boundary (step kernel).
// POW2: N is a power of two - the division is an exact multiplication by `rcN` = 1 / N.
// ---------------------------------------------------------------------------------------------------------------
template <typename T, bool POW2> __device__ __forceinline__ T grid_value(T x_plus_u, T nT, T rcN) {
    return POW2 ? x_plus_u * rcN : x_plus_u / nT;
}
template <typename T, bool POW2> __device__ __forceinline__ int grid_count(T c, T u, T nT, T rcN, int N) {
    T t = __builtin_fma(c, nT, -u);
    t = __builtin_fmin(__builtin_fmax(t, T(-1)), nT);  // +inf (beyond the column) -> N; NaN -> -1
    const T fl = __builtin_floor(t);
    const T pa = grid_value<T, POW2>(fl + u, nT, rcN), pb = grid_value<T, POW2>((fl + T(1)) + u, nT, rcN);
    const int K = (int)fl + ((pa <= c) ? 1 : 0) + ((pb <= c) ? 1 : 0);
    return K < 0 ? 0 : (K > N ? N : K);
}
// offspring counts relative to the round's first position r0, clamped to the round: [0, RE]
template <typename T, int VEC, bool POW2>
__device__ __forceinline__ void grid_counts_local(const T (&c)[VEC], T u, T nT, T rcN, int N, int r0, int RE,
                                                  int (&out)[VEC]) {
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
        const int k = grid_count<T, POW2>(c[j], u, nT, rcN, N) - r0;
        out[j] = k < 0 ? 0 : (k > RE ? RE : k);
    }
}

// One round of 256 * VEC consecutive systematic grid positions [r0, r0 + RE) against the 2 * 256 * VEC cdf entries
// starting at ws that the threads hold in registers (c0: entries ws + tid * VEC + j, c1: the same + 256 * VEC; +inf
// beyond the column).  Every entry computes how many of the round's positions lie at or below it (grid_count); entry q
// owns positions [K_{q-1}, K_q) and writes q + 1 at the head of that range in `hd`; a running maximum over the round's
// positions spreads the heads.  No search, no divergence.  `hd` (RE + 64 ints) must have its first RE entries zeroed before
// the call (the first barrier inside orders that against the scatter); `fallback(i, from)` resolves positions the
// window does not reach (from = first index not staged, or 0 when - defensively - no head precedes the position).
// sh_cl: 2 * PF_NWAVES ints, sh_wm: PF_NWAVES ints.  Three barriers.
#define PF_MAX_WINDOWS 12
// ints `hd` must hold for a round of RE positions: the RE heads and one dump slot per lane behind them (`dump = RE + lane` below)
constexpr int inverse_grid_heads(int round_elems) { return round_elems + PF_WAVE; }
// `next_window(it, d0, d1)` stages the cdf entries [ws + it * S, ws + (it + 1) * S) the same way (returns false when
// the column ends before them).  It is only called when the windows so far do not account for all RE positions - a
// stretch of negligible weights - and lets the workgroup walk on window by window (up to PF_MAX_WINDOWS) before the
// remaining positions fall back to per-position binary searches, whose ~20 dependent loads would set the duration of
// the whole kernel.
// V1: entries per thread of the window's second part.  A window is S = 256 * (VEC + V1) entries: thread t holds entries
// t * VEC + j (c0) and 256 * VEC + t * V1 + j (c1).  V1 = VEC is the 2 x 256 x VEC window of the stand-alone resampler;
// the fused step kernel uses V1 = 1 - 256 * VEC positions rarely need more than 256 * (VEC + 1) entries when the window
// starts within tile / 64 of the first ancestor, and every entry staged is an entry read, mapped and counted.
template <typename T, int VEC, int V1, typename NextWindow, typename Fallback>
__device__ __forceinline__ void inverse_grid_round(const T (&c0)[VEC], const T (&c1)[V1], int ws, int r0i, int RE, int N,
                                                   T ub, T nT, T rcN, bool pow2, int64_t i0, int* hd, int* sh_cl, int* sh_wm,
                                                   NextWindow&& next_window, Fallback&& fallback, int (&idx)[VEC]) {
    constexpr int S = PF_BLOCK * (VEC + V1);
    const int tid = threadIdx.x;
    const int lane = tid & 63, wid = tid >> 6;
    const int dump = RE + lane;
    // counts of one staged window -> heads; returns the number of positions accounted for so far
    auto scatter_window = [&](const T (&w0)[VEC], const T (&w1)[V1], int qbase, int covered_before) -> int {
        int cn0[VEC], cn1[V1];
        if (pow2) {
            grid_counts_local<T, VEC, true>(w0, ub, nT, rcN, N, r0i, RE, cn0);
            grid_counts_local<T, V1, true>(w1, ub, nT, rcN, N, r0i, RE, cn1);
        } else {
            grid_counts_local<T, VEC, false>(w0, ub, nT, rcN, N, r0i, RE, cn0);
            grid_counts_local<T, V1, false>(w1, ub, nT, rcN, N, r0i, RE, cn1);
        }
        if (lane == 63) {
            sh_cl[wid] = cn0[VEC - 1];
            sh_cl[PF_NWAVES + wid] = cn1[V1 - 1];
        }
        __syncthreads();  // the wave-boundary counts are visible; `hd` is zeroed
        int pv0 = wave_prev(cn0[VEC - 1], 0), pv1 = wave_prev(cn1[V1 - 1], 0);
        if (lane == 0) {
            pv0 = wid ? sh_cl[wid - 1] : covered_before;  // entries before the first window own no position of this round
            pv1 = sh_cl[PF_NWAVES + wid - 1];              // wave 0: the first part's last entry
        }
        const int covered = sh_cl[2 * PF_NWAVES - 1];
        // branch-free scatter: entries without offspring in this round write to a per-lane dump slot behind the RE heads
        // (exec-mask juggling per conditional store costs ~5 scalar instructions, a v_cndmask one vector instruction)
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            const int lo0 = j ? cn0[j - 1] : pv0;
            hd[(cn0[j] > lo0) ? lo0 : dump] = qbase + tid * VEC + j + 1;
        }
#pragma unroll
        for (int j = 0; j < V1; ++j) {
            const int lo1 = j ? cn1[j - 1] : pv1;
            hd[(cn1[j] > lo1) ? lo1 : dump] = qbase + PF_BLOCK * VEC + tid * V1 + j + 1;
        }
        return covered;
    };
    int covered = scatter_window(c0, c1, 0, 0);  // positions of this round the window(s) account for
    int windows = 1;
    for (; windows < PF_MAX_WINDOWS && covered < RE; ++windows) {  // uniform: `covered` comes from LDS
        __syncthreads();                                            // everyone has read sh_cl
        T d0[VEC], d1[V1];
        if (!next_window(windows, d0, d1)) break;
        covered = scatter_window(d0, d1, windows * S, covered);
    }
    __syncthreads();
    int h[VEC];
    if (VEC == 1) h[0] = hd[tid]; else load_vec<int, VEC>(hd + tid * VEC, h);
#pragma unroll
    for (int j = 1; j < VEC; ++j) h[j] = imax(h[j], h[j - 1]);
    const int inc = wave_scan_max(h[VEC - 1]);
    if (lane == 63) sh_wm[wid] = inc;
    __syncthreads();
    int carry = wave_prev(inc, 0);
#pragma unroll
    for (int w = 0; w < PF_NWAVES - 1; ++w) carry = (w < wid) ? imax(carry, sh_wm[w]) : carry;
    const int64_t beyond = (int64_t)ws + (int64_t)windows * S;
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
        const int64_t i = i0 + j;
        const int q = imax(carry, h[j]);
        int res = ws + q - 1;
        if (i < N && (tid * VEC + j >= covered || q == 0)) res = fallback(i, (q == 0) ? 0 : (int)(beyond < N ? beyond : N));
        idx[j] = (i < N && res < N) ? res : N - 1;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// Window search shared by the stand-alone resampler and the fused step kernel.
// For one round of 256*VEC consecutive grid positions: stage cdf[j0, j0 + WIN) in LDS, every thread lower_bounds its
// VEC positions inside the window (falling back to a global binary search beyond it), and the ancestor of the
// round's last position becomes the next round's window start (ancestors are non-decreasing).
// ---------------------------------------------------------------------------------------------------------------
template <typename T, int VEC> struct SearchWin {
    static constexpr int WIN = 2 * PF_BLOCK * VEC;
};

// Branch-free lower_bound of VEC values in the LDS window (WIN a power of two): log2(WIN) + 1 rounds of "probe, compare,
// advance" with all VEC probes of a round in flight together.  The same instruction stream for every lane - no
// exec-mask juggling (the galloping search above spends as many scalar as vector instructions on divergent loops).
// Returns positions in [0, WIN] (WIN = beyond the window).
template <typename T, int WIN, int VEC>
__device__ __forceinline__ void window_lower_bound_flat(const T* win, const T (&p)[VEC], int (&out)[VEC]) {
    static_assert((WIN & (WIN - 1)) == 0, "window size must be a power of two");
    // positions as BYTE offsets: a probe is one ds_read with an immediate offset, a round compare + select + add per position
    // (element indices cost a shift and an add more per probe: 21 against 16 VALU per round of four positions)
    const unsigned char* const wb = reinterpret_cast<const unsigned char*>(win);
#pragma unroll
    for (int j = 0; j < VEC; ++j) out[j] = 0;
#pragma unroll
    for (int step = WIN / 2; step >= 1; step >>= 1) {
        T v[VEC];
#pragma unroll
        for (int j = 0; j < VEC; ++j) v[j] = *reinterpret_cast<const T*>(wb + out[j] + (step - 1) * (int)sizeof(T));
#pragma unroll
        for (int j = 0; j < VEC; ++j) out[j] += (v[j] < p[j]) ? step * (int)sizeof(T) : 0;
    }
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
        out[j] += (*reinterpret_cast<const T*>(wb + out[j]) < p[j]) ? (int)sizeof(T) : 0;
        out[j] /= (int)sizeof(T);
    }
}

}  // namespace pf
