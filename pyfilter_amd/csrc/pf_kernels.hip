// pf_kernels.hip - hand-written HIP kernels (gfx950 / CDNA4, wave64) + the C ABI of libpfamd.so.
//
// One workgroup (256 threads) owns one *tile* of one *column* (= one filter of the batch dim); a tile is R rounds of
// 256*VEC consecutive particles (pf_device.hpp).  Every per-column global dependency (max / sum / scan total) is
// carried through per-tile *partials* in the workspace that the next kernel re-reduces at its start, so no kernel
// needs inter-workgroup communication inside a launch (the kernel boundary is the only synchronisation).
//
// HBM-bound by design: no MFMA anywhere - there is no dense contraction on this path.
// This is the main unit (pf_main.o): the stand-alone primitives and every extern "C" entry.  The fused runs' kernels are compiled in
// the other units (pf_step.hip, pf_column.hip, pf_cluster.hip); filter_run_checked, at the end of this file, checks a run's arguments
// and hands it to the route that takes it.
#include "pf_host.hpp"

namespace pf {

template <typename T, int VEC>
__device__ __forceinline__ void systematic_round(const T* __restrict__ cdf_col, int N, int64_t i0, T u,
                                                 const T* __restrict__ u_elem, T* win, int* sh_j0, int (&idx)[VEC]) {
    constexpr int WIN = SearchWin<T, VEC>::WIN;  // 2 * 256 * VEC cdf values cover the round's 256 * VEC positions
    const int tid = threadIdx.x;
    const int j0 = *sh_j0;
    const int ws = j0 - (j0 % VEC);  // window start, aligned to the vector width (N % VEC == 0)
    // stage the window: two vector loads per thread, both issued before the first LDS store; +inf beyond the column
    {
        T v0[VEC], v1[VEC];
        const int ja = ws + tid * VEC, jb = ws + (PF_BLOCK + tid) * VEC;
        const bool ina = ja < N, inb = jb < N;
        if (ina) { if (VEC == 1) v0[0] = cdf_col[ja]; else load_vec<T, VEC>(cdf_col + ja, v0); }
        if (inb) { if (VEC == 1) v1[0] = cdf_col[jb]; else load_vec<T, VEC>(cdf_col + jb, v1); }
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            if (!ina) v0[j] = Lim<T>::inf();
            if (!inb) v1[j] = Lim<T>::inf();
        }
        if (VEC == 1) { win[tid] = v0[0]; win[PF_BLOCK + tid] = v1[0]; }
        else { store_vec<T, VEC>(win + tid * VEC, v0); store_vec<T, VEC>(win + (PF_BLOCK + tid) * VEC, v1); }
    }
    __syncthreads();
    const T nT = T(N);
    T pp[VEC];
    int qq[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) pp[j] = (i0 + j < N) ? grid_position<T>(i0 + j, u_elem ? u_elem[i0 + j] : u, nT) : T(0);
    window_lower_bound_flat<T, WIN, VEC>(win, pp, qq);
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
        const int64_t i = i0 + j;
        int res = N - 1;
        if (i < N) {
            res = (qq[j] < WIN) ? ws + qq[j] : thread_lower_bound<T>(cdf_col, ws + WIN < N ? ws + WIN : N, N, pp[j]);
            if (res > N - 1) res = N - 1;
        }
        idx[j] = res;
    }
    __syncthreads();  // everyone is done with `win` and has read sh_j0
    if (tid == PF_BLOCK - 1) *sh_j0 = idx[VEC - 1];
    __syncthreads();
}

// ---------------------------------------------------------------------------------------------------------------
// stand-alone primitives
// ---------------------------------------------------------------------------------------------------------------

// per-tile online (max, sum exp, sum exp^2) of log-weights; optional in-place sanitise
// (the primitives' bodies are device functions of (column b, tile k): the kernels below run one per workgroup; the one-launch
// variants for columns of ONE tile - k_resample_one_tile / k_normalize_one_tile - run them back to back in one workgroup)
template <typename T, int VEC>
__device__ __forceinline__ void reduce_logw_body(T* __restrict__ logw, int sanitize, const uint8_t* colmask,
                                                 double* __restrict__ part, const Geom& g, int b, int k) {
    __shared__ double red[4 * PF_NWAVES];
    __shared__ T redm[PF_NWAVES];
    if (colmask && !colmask[b]) return;
    T* col = logw + (int64_t)b * g.N;
    OnlineLse<T> acc;
    acc.init();
    double q = 0.0;
    const int64_t base = (int64_t)k * g.tile_elems;
    for (int r = 0; r < g.rounds_per_tile; ++r) {
        const int64_t i0 = base + (int64_t)r * g.round_elems + threadIdx.x * VEC;
        if (i0 >= g.N) break;
        T v[VEC];
        if (VEC == 1) v[0] = col[i0]; else load_vec<T, VEC>(col + i0, v);
        bool changed = false;
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            const T s = sanitize_logw(v[j]);
            if (sanitize) { changed |= !(s == v[j]); v[j] = s; }
            double rs, e;
            acc.push(v[j], rs, e);
            q = q * rs * rs + e * e;
        }
        if (sanitize && changed) {
            if (VEC == 1) col[i0] = v[0]; else store_vec<T, VEC>(col + i0, v);
        }
    }
    const T M = block_max<T>(acc.m, redm);
    const double f = exp_diff((double)acc.m, (double)M);
    double sums[2] = {acc.s * f, q * f * f};
    block_sum<2>(sums, red);
    if (threadIdx.x == 0) {
        const int64_t stride = (int64_t)g.B * g.tiles;
        const int64_t o = (int64_t)b * g.tiles + k;
        part[PQ_M1 * stride + o] = (double)M;
        part[PQ_S1 * stride + o] = sums[0];
        part[PQ_Q1 * stride + o] = sums[1];
    }
}
template <typename T, int VEC>
__global__ __launch_bounds__(PF_BLOCK) void k_reduce_logw(T* __restrict__ logw, int sanitize, const uint8_t* colmask,
                                                          double* __restrict__ part, Geom g) {
    reduce_logw_body<T, VEC>(logw, sanitize, colmask, part, g, blockIdx.y, blockIdx.x);
}

// combine the (m, s[, q]) partials of one column; every thread gets the results
struct ColLse {
    double M, S, Q;
    double prefix;  // sum of the rescaled tile sums strictly before tile k (un-normalised)
};
// (T: the filter's arithmetic type - float columns take the fast float exp for the tile factors exp(m_t - M), as the fused kernels'
// tables do: the factors multiply float-precision tile sums, and four double-precision exp() per thread were most of what a
// workgroup of k_normalize_write / k_scan spent at 1 024 tiles per column)
template <typename T = double>
__device__ __forceinline__ ColLse combine_partials(const double* __restrict__ part, int slot_m, int slot_s, int slot_q,
                                                   int b, int k, int B, int tiles, double* red, double* redm) {
    const int64_t stride = (int64_t)B * tiles;
    const double* pm = part + slot_m * stride + (int64_t)b * tiles;
    const double* ps = part + slot_s * stride + (int64_t)b * tiles;
    const double* pq = (slot_q >= 0) ? part + slot_q * stride + (int64_t)b * tiles : nullptr;
    double m = -__builtin_huge_val();
    for (int t = threadIdx.x; t < tiles; t += PF_BLOCK) m = fmax(m, pm[t]);
    const double M = block_max<double>(m, redm);
    double v[3] = {0.0, 0.0, 0.0};
    for (int t = threadIdx.x; t < tiles; t += PF_BLOCK) {
        const double f = exp_diff_t<T>(pm[t], M);
        const double s = ps[t] * f;
        v[0] += s;
        if (pq) v[1] += pq[t] * f * f;
        if (t < k) v[2] += s;
    }
    block_sum<3>(v, red);
    ColLse r;
    r.M = M;
    r.S = v[0];
    r.Q = v[1];
    r.prefix = v[2];
    return r;
}

template <typename T, int VEC>
__device__ __forceinline__ void normalize_write_body(const T* __restrict__ logw, T* __restrict__ W, T* __restrict__ lse,
                                                     T* __restrict__ ess, const double* __restrict__ part, const Geom& g, int b, int k) {
    __shared__ double red[4 * PF_NWAVES];
    __shared__ double redm[PF_NWAVES];
    // (the sums of squares serve the ESS, which tile 0's workgroup alone reports: the others skip a third of the records)
    const ColLse c = combine_partials<T>(part, PQ_M1, PQ_S1, (k == 0 && ess) ? PQ_Q1 : -1, b, k, g.B, g.tiles, red, redm);
    if (k == 0 && threadIdx.x == 0) {
        if (lse) lse[b] = (T)(c.M + log(c.S));
        if (ess) ess[b] = (T)(c.S * c.S / c.Q);
    }
    if (!W) return;
    const T* col = logw + (int64_t)b * g.N;
    T* out = W + (int64_t)b * g.N;
    const T M = (T)c.M;
    const T S = (T)c.S;
    const int64_t base = (int64_t)k * g.tile_elems;
    for (int r = 0; r < g.rounds_per_tile; ++r) {
        const int64_t i0 = base + (int64_t)r * g.round_elems + threadIdx.x * VEC;
        if (i0 >= g.N) break;
        T v[VEC];
        if (VEC == 1) v[0] = col[i0]; else load_vec<T, VEC>(col + i0, v);
#pragma unroll
        for (int j = 0; j < VEC; ++j) v[j] = pf_exp(v[j] - M) / S;
        if (VEC == 1) out[i0] = v[0]; else store_vec<T, VEC>(out + i0, v);
    }
}
template <typename T, int VEC>
__global__ __launch_bounds__(PF_BLOCK) void k_normalize_write(const T* __restrict__ logw, T* __restrict__ W,
                                                              T* __restrict__ lse, T* __restrict__ ess,
                                                              const double* __restrict__ part, Geom g) {
    normalize_write_body<T, VEC>(logw, W, lse, ess, part, g, blockIdx.y, blockIdx.x);
}
// pf_normalize for columns of ONE tile: both passes in one launch (same arithmetic, same values)
template <typename T, int VEC>
__global__ __launch_bounds__(PF_BLOCK) void k_normalize_one_tile(T* __restrict__ logw, T* __restrict__ W, T* __restrict__ lse,
                                                                 T* __restrict__ ess, double* __restrict__ part, Geom g) {
    reduce_logw_body<T, VEC>(logw, 1, nullptr, part, g, blockIdx.y, 0);
    __threadfence_block();
    __syncthreads();  // the tile's record and the sanitised log-weights (this workgroup's own writes) are visible
    normalize_write_body<T, VEC>(logw, W, lse, ess, part, g, blockIdx.y, 0);
}

// per-tile fp64 sums of already-normalised weights (systematic, normalized=True path)
template <typename T, int VEC>
__device__ __forceinline__ void tile_sum_body(const T* __restrict__ W, const uint8_t* colmask, double* __restrict__ part,
                                              const Geom& g, int b, int k) {
    __shared__ double red[PF_NWAVES];
    if (colmask && !colmask[b]) return;
    const T* col = W + (int64_t)b * g.N;
    double s[1] = {0.0};
    const int64_t base = (int64_t)k * g.tile_elems;
    for (int r = 0; r < g.rounds_per_tile; ++r) {
        const int64_t i0 = base + (int64_t)r * g.round_elems + threadIdx.x * VEC;
        if (i0 >= g.N) break;
        T v[VEC];
        if (VEC == 1) v[0] = col[i0]; else load_vec<T, VEC>(col + i0, v);
#pragma unroll
        for (int j = 0; j < VEC; ++j) s[0] += (double)v[j];
    }
    block_sum<1>(s, red);
    if (threadIdx.x == 0) {
        const int64_t stride = (int64_t)g.B * g.tiles;
        part[PQ_M1 * stride + (int64_t)b * g.tiles + k] = 0.0;  // "max" 0 -> exp_diff = 1
        part[PQ_S1 * stride + (int64_t)b * g.tiles + k] = s[0];
    }
}
template <typename T, int VEC>
__global__ __launch_bounds__(PF_BLOCK) void k_tile_sum(const T* __restrict__ W, const uint8_t* colmask,
                                                       double* __restrict__ part, Geom g) {
    tile_sum_body<T, VEC>(W, colmask, part, g, blockIdx.y, blockIdx.x);
}

// Scan of one tile: cdf_i = T( P_k + f_k * sum_{j <= i in tile} e_j ), carried in fp64 and rounded per element -
// the same value torch's CPU cumsum produces (double accumulator, per-element round; SURVEY.md §0 finding 1).
//   FROM_W   : e_j = W_j,                 f_k = 1,                     P_k = sum of previous tile sums
//   otherwise: e_j = exp(logw_j - m_k),   f_k = exp(m_k - M) / S,      P_k = normalised prefix
template <typename T, int VEC, bool FROM_W>
__device__ __forceinline__ void scan_tile(const T* __restrict__ src_col, T* __restrict__ cdf_col, const Geom& g, int k,
                                          T tile_max, double Pk, double fk, double Pnext, double* red, const T (&v_first)[VEC],
                                          T* __restrict__ tree_col = nullptr) {
    const int tree_levels = tree_col ? cdf_tree_levels(g.N) : 0;
    double carry = 0.0;
    const int64_t base = (int64_t)k * g.tile_elems;
    for (int r = 0; r < g.rounds_per_tile; ++r) {
        const int64_t r0 = base + (int64_t)r * g.round_elems;
        if (r0 >= g.N) break;  // uniform across the workgroup
        const int64_t i0 = r0 + threadIdx.x * VEC;
        const bool on = i0 < g.N;
        T v[VEC];
        double e[VEC];
        if (r == 0) {  // (loaded by the caller BEFORE it combined the tile records: one round trip to memory instead of two in a row)
#pragma unroll
            for (int j = 0; j < VEC; ++j) v[j] = v_first[j];
        } else
        if (on) {
            if (VEC == 1) v[0] = src_col[i0]; else load_vec<T, VEC>(src_col + i0, v);
        }
        double local = 0.0;
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            double ej = 0.0;
            if (on) ej = FROM_W ? (double)v[j] : ((v[j] == -Lim<T>::inf()) ? 0.0 : (double)pf_exp_w(v[j] - tile_max));
            local += ej;
            e[j] = local;  // thread-local inclusive
        }
        double total;
        const double excl = block_scan_excl(local, red, total);
        if (on) {
            T outv[VEC];
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
                double c = Pk + fk * (carry + excl + e[j]);
                if (!FROM_W && c > Pnext) c = Pnext;
                outv[j] = (i0 + j == g.N - 1) ? T(1) : (T)c;  // cumsum[..., -1] = 1.0  (resampling.py:49)
            }
            if (VEC == 1) cdf_col[i0] = outv[0]; else store_vec<T, VEC>(cdf_col + i0, outv);
            if (tree_col) {  // (pf_multinomial) the entries that close a block of 16, 256, ... - and the column's last one every level
#pragma unroll
                for (int j = 0; j < VEC; ++j) {
                    const int64_t i = i0 + j;
                    int64_t n = (g.N + 15) >> 4;  // level 0's size; `o` its offset
                    int o = 0;
                    if (i == g.N - 1) {
                        for (int l = 0; l < tree_levels; ++l) {
                            tree_col[o + n - 1] = outv[j];
                            o += (int)((n + 15) & ~(int64_t)15);
                            n = (n + 15) >> 4;
                        }
                    } else if (((i + 1) & 15) == 0) {
                        int64_t m = (i + 1) >> 4;
                        tree_col[m - 1] = outv[j];
                        for (int l = 1; l < tree_levels && (m & 15) == 0; ++l) {
                            o += (int)((n + 15) & ~(int64_t)15);
                            n = (n + 15) >> 4;
                            m >>= 4;
                            tree_col[o + m - 1] = outv[j];
                        }
                    }
                }
            }
        }
        carry += total;
    }
}

template <typename T, int VEC, bool FROM_W>
__device__ __forceinline__ void scan_body(const T* __restrict__ src, T* __restrict__ cdf, const uint8_t* colmask,
                                          const double* __restrict__ part, const Geom& g, int b, int k, T* __restrict__ tree = nullptr) {
    __shared__ double red[4 * PF_NWAVES];
    __shared__ double redm[PF_NWAVES];
    if (colmask && !colmask[b]) return;
    // the tile's first round of elements: issued now, used after the tile records are combined
    T v_first[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) v_first[j] = T(0);
    {
        const int64_t i0 = (int64_t)k * g.tile_elems + threadIdx.x * VEC;
        if (i0 < g.N) {
            const T* sc = src + (int64_t)b * g.N;
            if (VEC == 1) v_first[0] = sc[i0]; else load_vec<T, VEC>(sc + i0, v_first);
        }
    }
    ColLse c;
    if constexpr (FROM_W) {
        // normalised weights: every tile record is (max 0, plain sum) - the prefix is the plain sum of the tile sums before k, in
        // combine_partials' order (its factors exp(0 - 0) are exactly 1: identical values) without the maxima's exchange and
        // four double-precision exp() per thread: k_scan at 2^20 x 1 (1 024 tile records per workgroup) 10.3 -> see
        // profiles/r05_primitives_baseline_shapes.txt
        const double* ps = part + PQ_S1 * ((int64_t)g.B * g.tiles) + (int64_t)b * g.tiles;
        double v[2] = {0.0, 0.0};
        for (int t = threadIdx.x; t < g.tiles; t += PF_BLOCK) {
            const double sv = ps[t];
            v[0] += sv;
            if (t < k) v[1] += sv;
        }
        block_sum<2>(v, red);
        c.M = 0.0;
        c.S = v[0];
        c.Q = 0.0;
        c.prefix = v[1];
    } else {
        c = combine_partials<T>(part, PQ_M1, PQ_S1, -1, b, k, g.B, g.tiles, red, redm);
    }
    const int64_t stride = (int64_t)g.B * g.tiles;
    const double mk = part[PQ_M1 * stride + (int64_t)b * g.tiles + k];
    const double sk = part[PQ_S1 * stride + (int64_t)b * g.tiles + k];
    double Pk, fk, Pnext;
    if (FROM_W) {
        Pk = c.prefix;
        fk = 1.0;
        Pnext = Pk + sk;
    } else {
        fk = exp_diff_t<T>(mk, c.M) / c.S;  // (the factor combine_partials<T> gives this tile inside the later tiles' prefixes)
        Pk = c.prefix / c.S;
        Pnext = Pk + sk * fk;
    }
    scan_tile<T, VEC, FROM_W>(src + (int64_t)b * g.N, cdf + (int64_t)b * g.N, g, k, (T)mk, Pk, fk, Pnext, red, v_first,
                              tree ? tree + (int64_t)b * cdf_tree_total(g.N) : nullptr);
}
template <typename T, int VEC, bool FROM_W>
__global__ __launch_bounds__(PF_BLOCK) void k_scan(const T* __restrict__ src, T* __restrict__ cdf,
                                                   const uint8_t* colmask, const double* __restrict__ part, Geom g, T* tree) {
    scan_body<T, VEC, FROM_W>(src, cdf, colmask, part, g, blockIdx.y, blockIdx.x, tree);
}

// ancestors from the cdf: systematic grid (u per column) or iid uniforms (multinomial)
// MN: iid multinomial draws (pf_multinomial) instead of the systematic grid - a template parameter so that the systematic
// instantiations do not carry the draws' registers (four 16-entry groups in flight per thread)
template <typename T, int VEC, bool MN>
__device__ __forceinline__ void search_body(const T* __restrict__ cdf, const T* __restrict__ u, int u_per_elem,
                                            const T* __restrict__ v, uint64_t seed, uint32_t step,
                                            const uint8_t* colmask, int32_t* __restrict__ idx, const Geom& g, int force_search,
                                            int b, int k, const T* __restrict__ tree = nullptr) {
    __shared__ __attribute__((aligned(32))) T win[SearchWin<T, VEC>::WIN];
    __shared__ int sh_j0;
    if (colmask && !colmask[b]) return;
    const T* col = cdf + (int64_t)b * g.N;
    int32_t* out = idx + (int64_t)b * g.N;
    const int N = (int)g.N;
    const int64_t base = (int64_t)k * g.tile_elems;
    const int lane = threadIdx.x & 63;

    if constexpr (!MN) {
        const T* u_elem = u_per_elem ? u + (int64_t)b * g.N : nullptr;
        const T ub = u_per_elem ? u_elem[base < g.N ? base : 0] : u[b];
        // (the whole workgroup bracketing the answer with 256 or 1 024 counted probes per round - two or three dependent round
        // trips instead of one wave's four or five - measured SLOWER: k_search 6.3 -> 8.3 / 9.8 us at 2^20 x 1, 13.6 -> 15.9 / 21.9
        // at 64 x 65 536: 1 024 workgroups x 1 024 probes is traffic, and two barriers per round; profiles/r05h_primitives_ab.txt)
        if (threadIdx.x < PF_WAVE) {
            const int j0 = wave_lower_bound<T>(col, N, grid_position<T>(base, ub, T(N)), lane);
            if (lane == 0) sh_j0 = j0;
        }
        __syncthreads();
        // one u per column and a grid the closed form is exact for: ancestors from the inverted grid, no search
        const bool inverse = !u_per_elem && !force_search && !(sizeof(T) == 4 && N > (1 << 22));
        if (inverse) {
            __shared__ int sh_cl[2 * PF_NWAVES], sh_wm[PF_NWAVES];
            int* hd = reinterpret_cast<int*>(win);
            const int tid = threadIdx.x;
            const T nT = T(N), rcN = T(1) / nT;
            const bool pow2 = (N & (N - 1)) == 0;
            for (int r = 0; r < g.rounds_per_tile; ++r) {
                const int64_t r0 = base + (int64_t)r * g.round_elems;
                if (r0 >= g.N) break;
                const int64_t i0 = r0 + tid * VEC;
                const int j0 = sh_j0;
                const int ws = j0 - (j0 % VEC);
                {
                    int zero[VEC];
#pragma unroll
                    for (int j = 0; j < VEC; ++j) zero[j] = 0;
                    if (VEC == 1) hd[tid] = 0; else store_vec<int, VEC>(hd + tid * VEC, zero);
                }
                // the window: 256 (VEC + 1) entries from the round's exact start (the fused step kernel's geometry, round 5 - the
                // ancestors of 256 VEC consecutive grid positions span at most 256 VEC + 1 entries; every staged entry is an entry
                // read and counted: 2 x 256 VEC cost k_search a third more per round); a stretch the window does not reach walks on
                // window by window inside inverse_grid_round
                constexpr int V1 = 1;
                constexpr int STAGED = PF_BLOCK * (VEC + V1);
                T c0[VEC], c1[V1];
                const int ja = ws + tid * VEC, jb = ws + PF_BLOCK * VEC + tid * V1;
                if (ja < N) { if (VEC == 1) c0[0] = col[ja]; else load_vec<T, VEC>(col + ja, c0); }
                if (jb < N) c1[0] = col[jb];
#pragma unroll
                for (int j = 0; j < VEC; ++j)
                    if (!(ja < N)) c0[j] = Lim<T>::inf();
                if (!(jb < N)) c1[0] = Lim<T>::inf();
                int res[VEC];
                inverse_grid_round<T, VEC, V1>(c0, c1, ws, (int)r0, g.round_elems, N, ub, nT, rcN, pow2, i0, hd, sh_cl, sh_wm,
                                           [&](int it, T (&d0)[VEC], T (&d1)[V1]) -> bool {
                                               const int w0 = ws + it * STAGED;
                                               if (w0 >= N) return false;
                                               const int wja = w0 + tid * VEC, wjb = w0 + PF_BLOCK * VEC + tid * V1;
#pragma unroll
                                               for (int j = 0; j < VEC; ++j) d0[j] = Lim<T>::inf();
                                               d1[0] = Lim<T>::inf();
                                               if (wja < N) { if (VEC == 1) d0[0] = col[wja]; else load_vec<T, VEC>(col + wja, d0); }
                                               if (wjb < N) d1[0] = col[wjb];
                                               return true;
                                           },
                                           [&](int64_t i, int from) { return thread_lower_bound<T>(col, from, N, grid_position<T>(i, ub, nT)); },
                                           res);
                if (i0 < g.N) {
                    if (VEC == 1) out[i0] = res[0]; else store_vec<int, VEC>(out + i0, res);
                }
                if (tid == PF_BLOCK - 1) sh_j0 = res[VEC - 1];  // next round's window starts at this round's last ancestor
                __syncthreads();
            }
            return;
        }
        for (int r = 0; r < g.rounds_per_tile; ++r) {
            const int64_t r0 = base + (int64_t)r * g.round_elems;
            if (r0 >= g.N) break;
            const int64_t i0 = r0 + threadIdx.x * VEC;
            int res[VEC];
            systematic_round<T, VEC>(col, N, i0, ub, u_elem, win, &sh_j0, res);
            if (i0 < g.N) {
                if (VEC == 1) out[i0] = res[0]; else store_vec<int, VEC>(out + i0, res);
            }
        }
    } else {
        // iid draws (the reference's torch.multinomial order: unsorted), each a lower_bound over the whole column.  A bisection of
        // N entries moves a 64-byte sector per 4-byte probe, ~10 of them per draw beyond what the caches hold, and that traffic -
        // not the chain of dependent loads - is what bounds it (4M x 1: 358 us; a two-level bisection with the thread's four
        // draws side by side was SLOWER, profiles/r06_systematic_two_launches.txt).  So the search is 16-ary over tables the scan
        // kernel leaves (cdf_tree_*: the cdf at every 16th, 256th, ... entry): a level is ONE aligned 64-byte group of 16 entries per
        // draw, counted in registers; the top levels (<= 4 096 entries) live in the caches, the 256-stride one in L2, and a draw
        // touches one or two lines beyond them instead of ten.
        const int levels = cdf_tree_levels(g.N);
        const T* tcol = tree + (int64_t)b * cdf_tree_total(g.N);
        // entries of the 16-group at `row` that are < p; `nv` of them exist (a level's padding / the column's end: never counted)
        auto count16 = [&](const T* __restrict__ row, int nv, T p, bool vector_ok) -> int {
            int cnt = 0;
            if (vector_ok) {
#pragma unroll
                for (int q4 = 0; q4 < 4; ++q4) {
                    T e[4];
                    load_vec<T, 4>(row + 4 * q4, e);
#pragma unroll
                    for (int i = 0; i < 4; ++i) cnt += (4 * q4 + i < nv && e[i] < p) ? 1 : 0;
                }
            } else {
                for (int i = 0; i < nv; ++i) cnt += (row[i] < p) ? 1 : 0;
            }
            return cnt;
        };
        // The top levels - as many as the window array holds (2 048 / 512 entries) - are copied into LDS once per workgroup: every
        // lane of a global load names its own line, and at 2^20 x 1 those per-lane requests (20 of them per draw through five levels,
        // ~1 per clock and CU) were what bounded the kernel; LDS serves the same 16-entry groups without them.
        constexpr int WIN = SearchWin<T, VEC>::WIN;
        int lds_from = levels;  // levels [lds_from, levels) sit in `win`, the top one first, each padded to 16 entries
        {
            int cum = 0;
            for (int l = levels - 1; l >= 0; --l) {
                int size, off;
                cdf_tree_level(g.N, l, size, off);
                const int pad = (size + 15) & ~15;
                if (cum + pad > WIN) break;
                for (int i = threadIdx.x; i < pad; i += PF_BLOCK) win[cum + i] = tcol[off + i];
                cum += pad;
                lds_from = l;
            }
        }
        __syncthreads();
        for (int r = 0; r < g.rounds_per_tile; ++r) {
            const int64_t i0 = base + (int64_t)r * g.round_elems + threadIdx.x * VEC;
            if (i0 >= g.N) break;
            T p[VEC];
            int grp[VEC];
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
                const int64_t e = (int64_t)b * g.N + i0 + j;
                p[j] = v ? v[e] : uniform_draw<T>(seed, PF_STREAM_MULTINOMIAL, step, (uint64_t)e);
                grp[j] = 0;
            }
            for (int l = levels - 1, cum = 0; l >= lds_from; --l) {
                int size, off;
                cdf_tree_level(g.N, l, size, off);
#pragma unroll
                for (int j = 0; j < VEC; ++j) {
                    const int at = grp[j] * 16;
                    const int nv = size - at > 16 ? 16 : size - at;
                    const T* row = win + cum + at;
                    int cnt = 0;
#pragma unroll
                    for (int i = 0; i < 16; ++i) cnt += (i < nv && row[i] < p[j]) ? 1 : 0;
                    grp[j] = at + cnt < size ? at + cnt : size - 1;
                }
                cum += (size + 15) & ~15;
            }
            for (int l = lds_from - 1; l >= 0; --l) {  // (the thread's VEC draws level by level: independent loads side by side)
                int size, off;
                cdf_tree_level(g.N, l, size, off);
#pragma unroll
                for (int j = 0; j < VEC; ++j) {
                    const int at = grp[j] * 16;  // (< size: the clamp below)
                    const int nv = size - at > 16 ? 16 : size - at;
                    const int nxt = at + count16(tcol + off + at, nv, p[j], true);
                    // (a group's last entry is >= p by the level above, so nxt names an entry of this level - unless NaNs broke the
                    // order: the clamp keeps every address inside its table)
                    grp[j] = nxt < size ? nxt : size - 1;
                }
            }
            int res[VEC];
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
                const int at = grp[j] * 16;  // (< N)
                const int nv = N - at > 16 ? 16 : N - at;
                const int a = at + count16(col + at, nv, p[j], VEC == 4 && nv == 16);
                res[j] = a > N - 1 ? N - 1 : a;
            }
            if (VEC == 1) out[i0] = res[0]; else store_vec<int, VEC>(out + i0, res);
        }
    }
}
template <typename T, int VEC, bool MN>
__global__ __launch_bounds__(PF_BLOCK) void k_search(const T* __restrict__ cdf, const T* __restrict__ u,
                                                     int u_per_elem, const T* __restrict__ v, uint64_t seed,
                                                     uint32_t step, const uint8_t* colmask, int32_t* __restrict__ idx,
                                                     Geom g, int force_search, const T* tree) {
    search_body<T, VEC, MN>(cdf, u, u_per_elem, v, seed, step, colmask, idx, g, force_search, blockIdx.y, blockIdx.x, tree);
}
// ---------------------------------------------------------------------------------------------------------------
// systematic(W) WITHOUT a materialised cdf (pf_systematic with cdf == NULL): two launches instead of three, 12 bytes per particle
// instead of 21.  The three-launch form is a chain tile sums -> cdf in memory -> search; here the cdf values a workgroup needs
// are rebuilt where they are used, from the weights themselves:
//   k_chunk_scan   every tile scans its weights once (fp64) and leaves, per CHUNK of 256 particles (one wave x 4), the sum of the
//                  tile's weights before the chunk (`cb`), and the tile's sum;
//   k_chunk_search every workgroup (a tile of grid positions) builds the column's tile-prefix table in LDS (<= 1 024 tile sums),
//                  finds the chunk its first position falls into - a count over the table, a count over that tile's `cb` -,
//                  and then per round stages FIVE chunks of WEIGHTS from there: a wave re-scans its chunk (the same DPP scan in the
//                  same lanes as k_chunk_scan) and has its 256 cdf values in registers,
//                         cdf_j = T( P_tile + ( cb_chunk + ( lanes before + own elements up to j ) ) ),   cdf_{N-1} = 1,
//                  one rounding to T per element like k_scan's; the ancestors come from the inverted systematic grid
//                  (grid_count: every entry's offspring range in closed form, heads scattered into LDS, a running maximum) as in
//                  k_search.  A stretch the five chunks do not cover walks on; a window that brings no progress (a long stretch of
//                  weightless particles) JUMPS: the chunk of the first position not yet covered is found like the first one.
// A cdf value is a deterministic function of (column, j) - whichever workgroup evaluates it gets the same bits -, so ancestors are
// consistent across tiles; against k_scan's values they differ in the association of the fp64 sum only (exact for float weights
// of ordinary dynamic range: tests/test_primitives_gpu.py).
// ---------------------------------------------------------------------------------------------------------------
#define PF_CHUNK (PF_WAVE * 4)
#define PF_CHUNK_WINDOW 5  // chunks staged per window: 256 (alignment slack) + 1 024 positions + 1 <= 1 280 entries

// what an element adds to the running sum: the weight itself, or exp(logw - tile maximum) (k_scan's addend: 0 for -inf)
template <typename T, bool FROM_W> __device__ __forceinline__ double chunk_addend(T v, T mk, bool on) {
    if constexpr (FROM_W) return (double)v;
    return (on && v != -Lim<T>::inf()) ? (double)pf_exp_w(v - mk) : 0.0;
}

// FROM_W: normalised weights, e_j = W_j.  Otherwise log-weights (pf_systematic_logw): sanitised IN PLACE (utils.py:57), then
// e_j = exp(logw_j - m_k) against the tile's own maximum m_k - the tile record is (m_k, sum e), as k_reduce_logw leaves it.
template <typename T, bool FROM_W>
__global__ __launch_bounds__(PF_BLOCK) void k_chunk_scan(T* __restrict__ W, const uint8_t* colmask, double* __restrict__ part,
                                                         double* __restrict__ cb, Geom g, int nchunks) {
    __shared__ double red[PF_NWAVES];
    __shared__ T redm[PF_NWAVES];
    const int b = blockIdx.y, k = blockIdx.x;
    if (colmask && !colmask[b]) return;
    T* col = W + (int64_t)b * g.N;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int64_t base = (int64_t)k * g.tile_elems;
    T mk = T(0);
    if constexpr (!FROM_W) {
        T m = -Lim<T>::inf();
        for (int r = 0; r < g.rounds_per_tile; ++r) {
            const int64_t i0 = base + (int64_t)r * g.round_elems + threadIdx.x * 4;
            if (i0 >= g.N) break;
            T v[4];
            load_vec<T, 4>(col + i0, v);
            bool changed = false;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const T sv = sanitize_logw(v[j]);
                changed |= !(sv == v[j]);
                v[j] = sv;
                m = sv > m ? sv : m;
            }
            if (changed) store_vec<T, 4>(col + i0, v);  // (read back below by the thread that wrote it)
        }
        mk = block_max<T>(m, redm);
    }
    double carry = 0.0;
    for (int r = 0; r < g.rounds_per_tile; ++r) {
        const int64_t r0 = base + (int64_t)r * g.round_elems;
        if (r0 >= g.N) break;
        const int64_t i0 = r0 + threadIdx.x * 4;
        const bool on = i0 < g.N;
        T v[4] = {T(0), T(0), T(0), T(0)};
        if (on) load_vec<T, 4>(col + i0, v);
        double run = 0.0;
#pragma unroll
        for (int j = 0; j < 4; ++j) run += chunk_addend<T, FROM_W>(v[j], mk, on);
        double total;
        const double excl = block_scan_excl(run, red, total);
        const int64_t c = r0 / PF_CHUNK + wid;
        if (lane == 0 && c < nchunks) cb[(int64_t)b * nchunks + c] = carry + excl;
        carry += total;
    }
    if (threadIdx.x == 0) {
        const int64_t stride = (int64_t)g.B * g.tiles;
        part[PQ_M1 * stride + (int64_t)b * g.tiles + k] = FROM_W ? 0.0 : (double)mk;
        part[PQ_S1 * stride + (int64_t)b * g.tiles + k] = carry;
    }
}

// the 4 cdf values lane `lane` holds of chunk c (entries c * 256 + lane * 4 + j); +inf beyond the column.  All 64 lanes call.
// Two phases so that a wave with two chunks to rebuild (the window's fifth) has both loads in flight before it scans the first.
template <typename T> struct ChunkLoad {
    T v[4];
    double basec;
    bool live, in;
    int j0;
};
template <typename T>
__device__ __forceinline__ ChunkLoad<T> chunk_load(const T* __restrict__ col, const double* __restrict__ cbcol, int c, int nchunks, int N,
                                                   int lane) {
    ChunkLoad<T> q;
    q.j0 = c * PF_CHUNK + lane * 4;
    q.live = c < nchunks;  // wave-uniform
    q.in = q.live && q.j0 < N;
#pragma unroll
    for (int j = 0; j < 4; ++j) q.v[j] = T(0);
    if (q.in) load_vec<T, 4>(col + q.j0, q.v);
    q.basec = q.live ? cbcol[c] : 0.0;
    return q;
}
// (P, f, Pn, m): the chunk's tile - prefix, factor (1 for weights), the next tile's prefix (the clamp k_scan applies to log-weight
// tiles: the exps of a tile never carry it past the next one's start), maximum
template <typename T, bool FROM_W>
__device__ __forceinline__ void chunk_cdf4(const ChunkLoad<T>& q, double P, double f, double Pn, T m, int N, int lane, T (&out)[4]) {
    double e[4];
    double run = 0.0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        run += chunk_addend<T, FROM_W>(q.v[j], m, q.in);
        e[j] = run;
    }
    const double wex = wave_scan_incl(run, lane) - run;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        double cv = FROM_W ? P + (q.basec + (wex + e[j])) : P + f * (q.basec + (wex + e[j]));
        if (!FROM_W && cv > Pn) cv = Pn;
        out[j] = q.in ? ((q.j0 + j == N - 1) ? T(1) : (T)cv) : Lim<T>::inf();
    }
}

#ifdef PF_DEVTOOLS  // (the instrumented build: cycle stamps of the middle workgroup of column 0, tools/chunk_search_stages.py)
#define PF_CSTAMP_ARG , unsigned long long* dbg
#define PF_CSTAMP(slot)                                                                                       \
    do {                                                                                                      \
        if (dbg && threadIdx.x == 0 && blockIdx.y == 0 && blockIdx.x == (unsigned)g.tiles / 2) dbg[slot] = (unsigned long long)clock64(); \
    } while (0)
#else
#define PF_CSTAMP_ARG
#define PF_CSTAMP(slot) do { } while (0)
#endif
template <typename T, bool FROM_W>
__global__ __launch_bounds__(PF_BLOCK) void k_chunk_search(const T* __restrict__ W, const T* __restrict__ u, const uint8_t* colmask,
                                                           const double* __restrict__ part, const double* __restrict__ cb,
                                                           int32_t* __restrict__ idx, Geom g, int nchunks PF_CSTAMP_ARG) {
    __shared__ double ptab[PF_MAX_TILES + 4];
    __shared__ double ftab[FROM_W ? 1 : PF_MAX_TILES];  // log-weights: the tiles' factors exp(m_t - M) / S and maxima
    __shared__ T mtab[FROM_W ? 1 : PF_MAX_TILES];
    __shared__ T redm[PF_NWAVES];
    __shared__ double red[PF_NWAVES];
    __shared__ int hd[PF_BLOCK * 4 + PF_WAVE];
    __shared__ __attribute__((aligned(32))) T c1buf[PF_CHUNK];
    __shared__ int sh_cl[2 * PF_NWAVES], sh_wm[PF_NWAVES], sh_cnt[PF_NWAVES], sh_j0;
    const int b = blockIdx.y, k = blockIdx.x;
    if (colmask && !colmask[b]) return;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int N = (int)g.N, tiles = g.tiles;
    PF_CSTAMP(0);
    const int cpt = g.rounds_per_tile * (g.round_elems / PF_CHUNK);  // chunks per tile (<= PF_BLOCK: the host checks)
    const T* col = W + (int64_t)b * g.N;
    const double* cbcol = cb + (int64_t)b * nchunks;
    int32_t* out = idx + (int64_t)b * g.N;
    const int64_t base = (int64_t)k * g.tile_elems;
    // ---- the column's tile-prefix table: P_t = sum of the tile sums before t (the same bits in every workgroup) ----
    // (log-weights: of the tile sums rescaled to the column's maximum, over their total - the normalised prefix k_scan uses)
    {
        const int64_t stride = (int64_t)g.B * tiles;
        const double* ps = part + PQ_S1 * stride + (int64_t)b * tiles;
        double s[4], f[4] = {1.0, 1.0, 1.0, 1.0};
#pragma unroll
        for (int j = 0; j < 4; ++j) s[j] = (tid * 4 + j < tiles) ? ps[tid * 4 + j] : 0.0;
        if constexpr (!FROM_W) {
            const double* pm = part + PQ_M1 * stride + (int64_t)b * tiles;
            double m[4];
            T mx = -Lim<T>::inf();
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                m[j] = (tid * 4 + j < tiles) ? pm[tid * 4 + j] : -__builtin_huge_val();
                mx = (T)m[j] > mx ? (T)m[j] : mx;
            }
            const double M = (double)block_max<T>(mx, redm);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                f[j] = exp_diff_t<T>(m[j], M);
                s[j] *= f[j];
                mtab[tid * 4 + j] = (T)m[j];
            }
        }
        double total;
        const double excl = block_scan_excl((s[0] + s[1]) + (s[2] + s[3]), red, total);
        const double inv = FROM_W ? 1.0 : 1.0 / total;
        ptab[tid * 4 + 0] = excl * inv;
        ptab[tid * 4 + 1] = (excl + s[0]) * inv;
        ptab[tid * 4 + 2] = (excl + (s[0] + s[1])) * inv;
        ptab[tid * 4 + 3] = (excl + ((s[0] + s[1]) + s[2])) * inv;
        if (tid == PF_BLOCK - 1) ptab[PF_MAX_TILES] = FROM_W ? total : 1.0;  // (the end of a column of PF_MAX_TILES tiles)
        if constexpr (!FROM_W) {
#pragma unroll
            for (int j = 0; j < 4; ++j) ftab[tid * 4 + j] = f[j] * inv;
        }
    }
    __syncthreads();
    PF_CSTAMP(1);
    const T ub = u[b];
    const T nT = T(N), rcN = T(1) / nT;
    const bool pow2 = (N & (N - 1)) == 0;
    // workgroup-wide count of up to four predicates per thread (uniform result; ballots, no cross-lane data movement)
    auto block_count = [&](bool p0, bool p1, bool p2, bool p3) -> int {
        const int w = (__popcll(__ballot(p0)) + __popcll(__ballot(p1))) + (__popcll(__ballot(p2)) + __popcll(__ballot(p3)));
        __syncthreads();  // (sh_cnt's previous readers)
        if (lane == 0) sh_cnt[wid] = w;
        __syncthreads();
        return (sh_cnt[0] + sh_cnt[1]) + (sh_cnt[2] + sh_cnt[3]);
    };
    // the chunk holding the first entry with cdf >= p: the last tile, then the last chunk of it, that starts below p
    auto find_chunk = [&](T p) -> int {
        bool below[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) below[j] = tid * 4 + j < tiles && (T)ptab[tid * 4 + j] < p;
        int t = block_count(below[0], below[1], below[2], below[3]) - 1;
        t = t < 0 ? 0 : t;
        const int c = t * cpt + tid;
        const bool in = tid < cpt && c < nchunks;
        const double v = in ? cbcol[c] : 0.0;
        int cc = block_count(in && (T)(ptab[t] + (FROM_W ? v : ftab[FROM_W ? 0 : t] * v)) < p, false, false, false) - 1;
        cc = cc < 0 ? 0 : cc;
        return t * cpt + cc;
    };
    const int RE = g.round_elems;
    for (int r = 0; r < g.rounds_per_tile; ++r) {
        const int64_t r0 = base + (int64_t)r * RE;
        if (r0 >= g.N) break;
        const int64_t i0 = r0 + tid * 4;
        const int need = (g.N - r0 < RE) ? (int)(g.N - r0) : RE;
        int chunk = (r == 0) ? find_chunk(grid_position<T>(r0, ub, nT)) : sh_j0 / PF_CHUNK;
        PF_CSTAMP(2);
        {
            const int zero[4] = {0, 0, 0, 0};
            store_vec<int, 4>(hd + tid * 4, zero);
        }
        const int dump = RE + lane;
        int covered = 0, stalled = 0;
        for (;;) {  // every branch below is workgroup-uniform
            T c0[4], c1[4];
            // (a window of five chunks from offset `off` in tile t0 reaches at most into tile t0 + 1: off + 4 < 2 cpt, cpt >= 4)
            const int t0 = chunk / cpt, off = chunk - t0 * cpt;
            const ChunkLoad<T> la = chunk_load<T>(col, cbcol, chunk + wid, nchunks, N, lane);
            ChunkLoad<T> lb;
            if (wid == 0) lb = chunk_load<T>(col, cbcol, chunk + 4, nchunks, N, lane);
            // (entries past the last tile are beyond the column: +inf whatever the tables hold - the index is only kept in range)
            const int ta = t0 + (off + wid >= cpt ? 1 : 0) < tiles ? t0 + (off + wid >= cpt ? 1 : 0) : tiles - 1;
            const int tb = t0 + (off + 4 >= cpt ? 1 : 0) < tiles ? t0 + (off + 4 >= cpt ? 1 : 0) : tiles - 1;
            chunk_cdf4<T, FROM_W>(la, ptab[ta], FROM_W ? 1.0 : ftab[FROM_W ? 0 : ta], ptab[ta + 1], FROM_W ? T(0) : mtab[FROM_W ? 0 : ta], N, lane, c0);
            if (wid == 0) {
                chunk_cdf4<T, FROM_W>(lb, ptab[tb], FROM_W ? 1.0 : ftab[FROM_W ? 0 : tb], ptab[tb + 1], FROM_W ? T(0) : mtab[FROM_W ? 0 : tb], N, lane, c1);
                store_vec<T, 4>(c1buf + lane * 4, c1);
            }
            __syncthreads();  // c1buf is written (and, first window: hd is zeroed)
            PF_CSTAMP(3);
            T d1[1] = {c1buf[tid]};
            int cn0[4], cn1[1];
            if (pow2) {
                grid_counts_local<T, 4, true>(c0, ub, nT, rcN, N, (int)r0, RE, cn0);
                grid_counts_local<T, 1, true>(d1, ub, nT, rcN, N, (int)r0, RE, cn1);
            } else {
                grid_counts_local<T, 4, false>(c0, ub, nT, rcN, N, (int)r0, RE, cn0);
                grid_counts_local<T, 1, false>(d1, ub, nT, rcN, N, (int)r0, RE, cn1);
            }
            if (lane == 63) {
                sh_cl[wid] = cn0[3];
                sh_cl[PF_NWAVES + wid] = cn1[0];
            }
            __syncthreads();
            int pv0 = wave_prev(cn0[3], 0), pv1 = wave_prev(cn1[0], 0);
            if (lane == 0) {
                pv0 = wid ? sh_cl[wid - 1] : covered;  // entries before the window own no position not covered yet
                pv1 = sh_cl[PF_NWAVES + wid - 1];      // (wave 0: the first part's last entry)
            }
            const int covered_now = sh_cl[2 * PF_NWAVES - 1];
            const int q0 = chunk * PF_CHUNK + tid * 4 + 1, q1 = (chunk + 4) * PF_CHUNK + tid + 1;  // entry index + 1
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int lo = j ? cn0[j - 1] : pv0;
                hd[(cn0[j] > lo) ? lo : dump] = q0 + j;
            }
            hd[(cn1[0] > pv1) ? pv1 : dump] = q1;
            stalled = (covered_now > covered) ? 0 : stalled + 1;
            covered = covered_now > covered ? covered_now : covered;
            PF_CSTAMP(4);
            if (covered >= need || stalled >= 2 || (int64_t)(chunk + PF_CHUNK_WINDOW) * PF_CHUNK >= g.N) break;
            __syncthreads();  // everyone has read sh_cl / c1buf
            // no progress: the next entry that owns a position is far away - look it up; else walk on
            chunk = stalled ? find_chunk(grid_position<T>(r0 + covered, ub, nT)) : chunk + PF_CHUNK_WINDOW;
        }
        __syncthreads();
        int h[4];
        load_vec<int, 4>(hd + tid * 4, h);
#pragma unroll
        for (int j = 1; j < 4; ++j) h[j] = imax(h[j], h[j - 1]);
        const int inc = wave_scan_max(h[3]);
        if (lane == 63) sh_wm[wid] = inc;
        __syncthreads();
        int carry = wave_prev(inc, 0);
#pragma unroll
        for (int w = 0; w < PF_NWAVES - 1; ++w) carry = (w < wid) ? imax(carry, sh_wm[w]) : carry;
        int res[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int q = imax(carry, h[j]);
            const bool ok = (tid * 4 + j < covered) && q > 0 && q <= N;  // (not covered: NaN weights - the clamp searchsorted gives)
            res[j] = ok ? q - 1 : N - 1;
        }
        if (i0 < g.N) store_vec<int, 4>(out + i0, res);
        if (tid == PF_BLOCK - 1) sh_j0 = res[3];  // the next round's window starts at this round's last ancestor
        __syncthreads();
        PF_CSTAMP(5);
    }
}
#undef PF_CSTAMP
#undef PF_CSTAMP_ARG

// systematic / multinomial resampling of columns of ONE tile (filters of up to a few thousand particles, or many filters:
// 1 024 x 8 192 is one 8-round tile per column) in ONE launch: tile record -> scan -> ancestors, the three kernels' bodies back
// to back in the column's workgroup (same arithmetic: identical cdf and ancestors; the cdf goes through memory between
// the stages exactly as between the launches, it is just never re-read from another CU)
template <typename T, int VEC, bool FROM_W, bool MN>
__global__ __launch_bounds__(PF_BLOCK) void k_resample_one_tile(T* __restrict__ src, const T* __restrict__ u, int u_per_elem,
                                                                const T* __restrict__ v, uint64_t seed,
                                                                uint32_t step, const uint8_t* colmask, T* __restrict__ cdf,
                                                                int32_t* __restrict__ idx, double* __restrict__ part, Geom g, T* tree) {
    const int b = blockIdx.y;
    if (FROM_W) tile_sum_body<T, VEC>(src, colmask, part, g, b, 0);
    else reduce_logw_body<T, VEC>(src, 1, colmask, part, g, b, 0);
    __threadfence_block();
    __syncthreads();
    scan_body<T, VEC, FROM_W>(src, cdf, colmask, part, g, b, 0, MN ? tree : nullptr);
    __threadfence_block();
    __syncthreads();
    search_body<T, VEC, MN>(cdf, u, u_per_elem, v, seed, step, colmask, idx, g, 0, b, 0, tree);
}

template <typename T>
__global__ __launch_bounds__(PF_BLOCK) void k_gather(const T* __restrict__ x, const int32_t* __restrict__ idx,
                                                     const uint8_t* colmask, T* __restrict__ out, int64_t N, int B,
                                                     int D) {
    const int b = blockIdx.y;
    const bool on = !colmask || colmask[b];
    for (int64_t i = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x; i < N; i += (int64_t)gridDim.x * PF_BLOCK) {
        const int64_t a = on ? (int64_t)idx[(int64_t)b * N + i] : i;
        for (int d = 0; d < D; ++d) {
            const int64_t o = ((int64_t)d * B + b) * N;
            out[o + i] = x[o + a];
        }
    }
}

// Whole-column moves along the batch dim (FilterResult / ParticleFilterCorrection resample + exchange).  A column is a
// contiguous run of N elements; a workgroup moves PF_COLCHUNK bytes of one column of one plane with 16-byte accesses
// (8 / 4-byte ones when the column size or the base addresses are not 16-byte multiples).  idx == nullptr: identity
// (exchange); mask == nullptr: every column.
#define PF_COLCHUNK (PF_BLOCK * 16 * 8)
typedef unsigned int pf_v4u __attribute__((ext_vector_type(4)));
typedef unsigned int pf_v2u __attribute__((ext_vector_type(2)));
template <typename V>
__global__ __launch_bounds__(PF_BLOCK) void k_columns_move(const char* __restrict__ src, const int64_t* __restrict__ idx,
                                                           const uint8_t* __restrict__ mask, char* __restrict__ dst,
                                                           int64_t col_bytes, int B) {
    const int b = blockIdx.y, p = blockIdx.z;
    if (mask && !mask[b]) return;
    int64_t from = idx ? idx[b] : (int64_t)b;
    if (from < 0) from += B;  // torch-style negative indices
    const V* s = reinterpret_cast<const V*>(src + ((int64_t)p * B + from) * col_bytes);
    V* d = reinterpret_cast<V*>(dst + ((int64_t)p * B + b) * col_bytes);
    const int64_t n = col_bytes / (int64_t)sizeof(V);
    const int64_t per_wg = PF_COLCHUNK / (int64_t)sizeof(V);
    const int64_t lo = (int64_t)blockIdx.x * per_wg;
    const int64_t hi = lo + per_wg < n ? lo + per_wg : n;
    // eight independent 16-byte loads in flight per thread before the first store
    for (int64_t i = lo + threadIdx.x; i < hi; i += 8 * PF_BLOCK) {
        V v[8];
#pragma unroll
        for (int q = 0; q < 8; ++q)
            if (i + q * PF_BLOCK < hi) v[q] = __builtin_nontemporal_load(s + i + q * PF_BLOCK);
#pragma unroll
        for (int q = 0; q < 8; ++q)
            if (i + q * PF_BLOCK < hi) __builtin_nontemporal_store(v[q], d + i + q * PF_BLOCK);
    }
}

// log_likelihood partials: online max of v with companion sum W * exp(v - max)
template <typename T>
__global__ __launch_bounds__(PF_BLOCK) void k_loglik_part(const T* __restrict__ v, const T* __restrict__ W,
                                                          double* __restrict__ part, Geom g) {
    __shared__ double red[PF_NWAVES];
    __shared__ T redm[PF_NWAVES];
    const int b = blockIdx.y, k = blockIdx.x;
    const int64_t base = (int64_t)k * g.tile_elems;
    const int64_t end = (base + g.tile_elems < g.N) ? base + g.tile_elems : g.N;
    T m = -Lim<T>::inf();
    double s = 0.0;
    bool nan_seen = false;
    for (int64_t i = base + threadIdx.x; i < end; i += PF_BLOCK) {
        const T vi = v[(int64_t)b * g.N + i];
        const double wi = W ? (double)W[(int64_t)b * g.N + i] : 1.0 / (double)g.N;
        if (vi != vi) nan_seen = true;
        if (vi > m) {
            s *= (m == -Lim<T>::inf()) ? 0.0 : (double)pf_exp(m - vi);
            m = vi;
        }
        s += (vi == -Lim<T>::inf()) ? 0.0 : wi * (double)pf_exp(vi - m);
    }
    if (nan_seen) s = __builtin_nan("");
    const T M = block_max<T>(m, redm);
    double sums[1] = {s * exp_diff((double)m, (double)M)};
    if (nan_seen) sums[0] = __builtin_nan("");
    block_sum<1>(sums, red);
    if (threadIdx.x == 0) {
        const int64_t stride = (int64_t)g.B * g.tiles;
        part[PQ_M1 * stride + (int64_t)b * g.tiles + k] = (double)M;
        part[PQ_S1 * stride + (int64_t)b * g.tiles + k] = sums[0];
    }
}

template <typename T>
__global__ __launch_bounds__(PF_BLOCK) void k_loglik_final(const double* __restrict__ part, T* __restrict__ out,
                                                           Geom g) {
    __shared__ double red[4 * PF_NWAVES];
    __shared__ double redm[PF_NWAVES];
    const int b = blockIdx.x;
    const ColLse c = combine_partials<T>(part, PQ_M1, PQ_S1, -1, b, 0, g.B, g.tiles, red, redm);
    // (a column that is -inf throughout: NaN, the reference's -inf + log sum exp(-inf - -inf) - not the -inf of M + log 0)
    if (threadIdx.x == 0) out[b] = (T)(c.M == -__builtin_huge_val() ? __builtin_nan("") : c.M + log(c.S));
}

// the variance about the mean from sums about a pivot c: S0 = sum W, P1 = sum W (x - c), P2 = sum W (x - c)^2, r = mean - c.
// Not contracted into fmas: one particle of weight 1 gives P2 = r P1 = r^2 S0 rounded alike, and a variance of exactly 0.
__device__ __forceinline__ double pivoted_variance(double s0, double p1, double p2, double r) {
#pragma clang fp contract(off)
    const double v = p2 - 2.0 * r * p1 + r * r * s0;
    return v < 0.0 ? 0.0 : v;  // (a NaN stays)
}

// moments partials from normalised weights about the pivot c_d = the column's first particle (every tile of a column reads the
// same one; the subtraction in double, after widening): sum W, sum W (x_d - c_d), sum W (x_d - c_d)^2
template <typename T>
__global__ __launch_bounds__(PF_BLOCK) void k_moments_part(const T* __restrict__ x, const T* __restrict__ W,
                                                           double* __restrict__ part, Geom g, int D) {
    __shared__ double red[(1 + 2 * PF_MAXD) * PF_NWAVES];
    const int b = blockIdx.y, k = blockIdx.x;
    const int64_t base = (int64_t)k * g.tile_elems;
    const int64_t end = (base + g.tile_elems < g.N) ? base + g.tile_elems : g.N;
    double acc[1 + 2 * PF_MAXD];
#pragma unroll
    for (int q = 0; q < 1 + 2 * PF_MAXD; ++q) acc[q] = 0.0;
    double c[PF_MAXD];
#pragma unroll
    for (int d = 0; d < PF_MAXD; ++d) c[d] = d < D ? (double)x[((int64_t)d * g.B + b) * g.N] : 0.0;
    for (int64_t i = base + threadIdx.x; i < end; i += PF_BLOCK) {
        const double w = (double)W[(int64_t)b * g.N + i];
        acc[0] += w;
#pragma unroll
        for (int d = 0; d < PF_MAXD; ++d) {
            if (d < D) {
                const double xv = (double)x[((int64_t)d * g.B + b) * g.N + i] - c[d];
                acc[1 + d] += w * xv;
                acc[1 + PF_MAXD + d] += w * xv * xv;
            }
        }
    }
    block_sum<1 + 2 * PF_MAXD>(acc, red);
    if (threadIdx.x == 0) {
        const int64_t stride = (int64_t)g.B * g.tiles;
        const int64_t o = (int64_t)b * g.tiles + k;
#pragma unroll
        for (int q = 0; q < 1 + 2 * PF_MAXD; ++q) part[q * stride + o] = acc[q];
    }
}

// (D here: the planes of this launch, <= PF_MAXD; pf_moments launches once per group of PF_MAXD planes and the row of a column
// in mean / var is `ld` long, the group's first plane at `d0`)
// With S0 = sum W and P1, P2 the sums about the pivot c (k_moments_part; x: the group's planes, for c):
//   mean = c S0 + P1 = sum W x (the reference does not divide by sum W),
//   var = P2 - 2 (mean - c) P1 + (mean - c)^2 S0 = sum W (x - mean)^2, clamped at 0 - it does not cancel however far the cloud
//   sits from zero.  A NaN in a component (under any weight, 0 included) makes that component's mean and variance NaN.
template <typename T>
__global__ __launch_bounds__(PF_BLOCK) void k_moments_final(const double* __restrict__ part, const T* __restrict__ x,
                                                            T* __restrict__ mean, T* __restrict__ var, Geom g, int D, int d0,
                                                            int ld) {
    __shared__ double red[(1 + 2 * PF_MAXD) * PF_NWAVES];
    const int b = blockIdx.x;
    const int64_t stride = (int64_t)g.B * g.tiles;
    double acc[1 + 2 * PF_MAXD];
#pragma unroll
    for (int q = 0; q < 1 + 2 * PF_MAXD; ++q) {
        acc[q] = 0.0;
        for (int t = threadIdx.x; t < g.tiles; t += PF_BLOCK) acc[q] += part[q * stride + (int64_t)b * g.tiles + t];
    }
    block_sum<1 + 2 * PF_MAXD>(acc, red);
    if (threadIdx.x == 0) {
        for (int d = 0; d < D; ++d) {
            const double c = (double)x[((int64_t)d * g.B + b) * g.N];
            const double r = c * (acc[0] - 1.0) + acc[1 + d];  // mean - c
            const double mu = c + r;
            mean[(int64_t)b * ld + d0 + d] = (T)mu;
            var[(int64_t)b * ld + d0 + d] = (T)pivoted_variance(acc[0], acc[1 + d], acc[1 + PF_MAXD + d], r);
        }
    }
}

// elementwise model kernels (un-fused path)
template <typename T, int D>
__global__ __launch_bounds__(PF_BLOCK) void k_pre_weight(ModelDesc md, const T* __restrict__ params, int proposal,
                                                         const T* __restrict__ x, const T* __restrict__ y,
                                                         int y_rows, T* __restrict__ out, int64_t N, int B) {
    const int b = blockIdx.y;
    const int O = md.obs_dim;
    const int NP = PF_BUILTIN_ROW_LEN(D, O);
    ColParams<T, D> cp;
    cp.load(params + (int64_t)b * NP, O, y + (int64_t)(y_rows == 1 ? 0 : b) * O);
    ColConsts<T, D> cc;
    cc.prepare(md, cp);
    for (int64_t i = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x; i < N; i += (int64_t)gridDim.x * PF_BLOCK) {
        T xv[D];
#pragma unroll
        for (int d = 0; d < D; ++d) xv[d] = x[((int64_t)d * B + b) * N + i];
        out[(int64_t)b * N + i] = pre_weight<T, D>(md, proposal, cp, cc, xv);
    }
}

template <typename T, int D>
__device__ __forceinline__ void draw_z(const T* __restrict__ z, uint64_t seed, uint32_t step, int64_t N, int B, int b,
                                       int64_t i, T (&zv)[D]) {
    if (z) {
#pragma unroll
        for (int d = 0; d < D; ++d) zv[d] = z[((int64_t)d * B + b) * N + i];
    } else {
        NormalDraw<T, D>::draw(seed, PF_STREAM_NORMAL, step, (uint64_t)((int64_t)b * N + i), zv);
    }
}

template <typename T, int D>
__global__ __launch_bounds__(PF_BLOCK) void k_sample_and_weight(ModelDesc md, const T* __restrict__ params,
                                                                int proposal, int weigh, const T* __restrict__ x,
                                                                const T* __restrict__ y, int y_rows,
                                                                const T* __restrict__ z, uint64_t seed, uint32_t step,
                                                                T* __restrict__ x_out, T* __restrict__ w_out,
                                                                int64_t N, int B) {
    const int b = blockIdx.y;
    const int O = md.obs_dim;
    const int NP = PF_BUILTIN_ROW_LEN(D, O);
    ColParams<T, D> cp;
    cp.load(params + (int64_t)b * NP, O, (weigh && y) ? y + (int64_t)(y_rows == 1 ? 0 : b) * O : nullptr);
    ColConsts<T, D> cc;
    cc.prepare(md, cp);
    for (int64_t i = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x; i < N; i += (int64_t)gridDim.x * PF_BLOCK) {
        T xv[D], zv[D], xn[D];
#pragma unroll
        for (int d = 0; d < D; ++d) xv[d] = x[((int64_t)d * B + b) * N + i];
        draw_z<T, D>(z, seed, step, N, B, b, i, zv);
        const T w = sample_and_weight<T, D>(md, weigh ? proposal : PF_PROP_BOOTSTRAP, cp, cc, xv, zv, xn);
#pragma unroll
        for (int d = 0; d < D; ++d) x_out[((int64_t)d * B + b) * N + i] = xn[d];
        if (weigh && w_out) w_out[(int64_t)b * N + i] = w;
    }
}

template <typename T>
__global__ __launch_bounds__(PF_BLOCK) void k_initial_sample(double m0a, double m0b, double m0c, double s0a,
                                                             double s0b, double s0c, const T* __restrict__ z,
                                                             uint64_t seed, T* __restrict__ x, int64_t N, int B,
                                                             int D, uint32_t group) {
    const int b = blockIdx.y;
    for (int64_t i = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x; i < N; i += (int64_t)gridDim.x * PF_BLOCK) {
        T zv[4] = {T(0), T(0), T(0), T(0)};
        if (!z) NormalDraw<T, 4>::draw(seed, PF_STREAM_INIT, group, (uint64_t)((int64_t)b * N + i), zv);
#pragma unroll
        for (int d = 0; d < PF_MAXD; ++d) {
            if (d < D) {
                const int64_t o = ((int64_t)d * B + b) * N + i;
                const T zz = z ? z[o] : zv[d];
                x[o] = (T)(d == 0 ? m0a : (d == 1 ? m0b : m0c)) + (T)(d == 0 ? s0a : (d == 1 ? s0b : s0c)) * zz;
            }
        }
    }
}

// ... with one initial mean / scale per filter: element (b, d) at m0[b * mb + d * md] (strides in elements, 0 = broadcast)
template <typename T>
__global__ __launch_bounds__(PF_BLOCK) void k_initial_sample_cols(const T* __restrict__ m0, int64_t mb, int64_t md, const T* __restrict__ s0,
                                                                  int64_t sb, int64_t sd, const T* __restrict__ z, uint64_t seed,
                                                                  T* __restrict__ x, int64_t N, int B, int D, uint32_t group) {
    const int b = blockIdx.y;
    for (int64_t i = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x; i < N; i += (int64_t)gridDim.x * PF_BLOCK) {
        T zv[4] = {T(0), T(0), T(0), T(0)};
        if (!z) NormalDraw<T, 4>::draw(seed, PF_STREAM_INIT, group, (uint64_t)((int64_t)b * N + i), zv);
#pragma unroll
        for (int d = 0; d < PF_MAXD; ++d) {
            if (d < D) {
                const int64_t o = ((int64_t)d * B + b) * N + i;
                const T zz = z ? z[o] : zv[d];
                // (two roundings - product, then sum; not contracted into an fma - the torch expression `m + s * z` this
                // replaces, to the last bit)
                {
#pragma clang fp contract(off)
                    const T sz = s0[b * sb + d * sd] * zz;
                    x[o] = m0[b * mb + d * md] + sz;
                }
            }
        }
    }
}

// Test support (pf_debug_draw_normals): the standard normals the fused step kernel draws for steps step0 .. - the same
// draw_normals<T, D, VEC> call, addressed as the step kernel addresses it (thread = VEC consecutive particles).
template <typename T, int D, int VEC>
__global__ __launch_bounds__(PF_BLOCK) void k_debug_normals(uint64_t seed, uint32_t step0, T* __restrict__ out, int64_t N,
                                                            int B) {
    const int b = blockIdx.y;
    const uint32_t s = blockIdx.z;
    const int64_t i0 = ((int64_t)blockIdx.x * PF_BLOCK + threadIdx.x) * VEC;
    if (i0 >= N) return;
    T zt[VEC][D];
    draw_normals<T, D, VEC>(seed, PF_STREAM_NORMAL, step0 + s, (uint64_t)((int64_t)b * N + i0), zt);
#pragma unroll
    for (int d = 0; d < D; ++d)
#pragma unroll
        for (int j = 0; j < VEC; ++j)
            if (i0 + j < N) out[(((int64_t)s * D + d) * B + b) * N + i0 + j] = zt[j][d];
}

}  // namespace pf

// =================================================================================================================
// C ABI
// =================================================================================================================
#ifndef PF_SOURCE_SHA256
#error "pf_kernels.hip: -DPF_SOURCE_SHA256='\"<digest>\"' is required (__graft_entry__.unit_command passes the tree's source_digest())"
#endif
#define PF_STR2(x) #x
#define PF_STR(x) PF_STR2(x)
extern "C" const char* pf_version(void) { return "pfamd 0.2.0 (gfx950) abi " PF_STR(PF_ABI_VERSION) " src:" PF_SOURCE_SHA256; }
extern "C" int pf_abi_version(void) { return PF_ABI_VERSION; }

extern "C" const char* pf_error_string(int code) {
    switch (code) {
        case PF_OK: return "ok";
        case PF_EINVAL: return "invalid argument";
        case PF_EWORKSPACE: return "workspace too small";
        case PF_EUNSUPPORTED: return "unsupported configuration";
        default: return code > 0 ? hipGetErrorString((hipError_t)code) : "unknown error";
    }
}



#ifdef PF_DEVTOOLS  // (the instrumented build only - tools/pmc_stages.py --build: where the workspace keeps the development timestamps)
extern "C" int pf_debug_offset(int64_t N, int64_t B, size_t* off) {
    if (!off || bad_shape(N, B)) return PF_EINVAL;
    *off = make_ws(make_geom(N, B)).off_dbg;
    return PF_OK;
}
#endif

// (any D: pf_moments reduces the planes in groups of PF_MAXD, so the stand-alone primitives need no more than a PF_MAXD problem)
extern "C" int pf_workspace_bytes(int64_t N, int64_t B, int64_t D, size_t* bytes) {
    if (!bytes || bad_shape(N, B) || D < 1) return PF_EINVAL;
    *bytes = ws_bound(N, B);
    return PF_OK;
}

// the tile-geometry primitives' launch context: geometry, workspace layout (its size the caller checks), partials, stream, grid
struct TileLaunch {
    Geom g;
    WsLayout wl;
    double* part;
    hipStream_t st;
    dim3 grid;
    TileLaunch(int64_t N, int64_t B, void* ws, void* stream)
        : g(make_geom(N, B)), wl(make_ws(g)), part((double*)((char*)ws + wl.off_part)), st((hipStream_t)stream), grid(g.tiles, g.B) {}
};

extern "C" int pf_normalize(void* logw, void* W, void* lse, void* ess, int64_t N, int64_t B, int dtype, void* ws,
                            size_t ws_bytes, void* stream) {
    if (!logw || !ws || bad_shape(N, B)) return PF_EINVAL;
    const TileLaunch p(N, B, ws, stream);
    if (ws_bytes < p.wl.total) return PF_EWORKSPACE;
    return with_dtype(dtype, [&](auto t) {
        return with_vec(p.g.vec, [&](auto v) {
            using T = decltype(t);
            constexpr int V = decltype(v)::value;
            if (p.g.tiles == 1) {  // one tile per column: both passes in one launch
                hipLaunchKernelGGL((k_normalize_one_tile<T, V>), p.grid, dim3(PF_BLOCK), 0, p.st, (T*)logw, (T*)W, (T*)lse, (T*)ess, p.part, p.g);
            } else {
                hipLaunchKernelGGL((k_reduce_logw<T, V>), p.grid, dim3(PF_BLOCK), 0, p.st, (T*)logw, 1, (const uint8_t*)nullptr, p.part, p.g);
                hipLaunchKernelGGL((k_normalize_write<T, V>), p.grid, dim3(PF_BLOCK), 0, p.st, (const T*)logw, (T*)W, (T*)lse, (T*)ess,
                                   (const double*)p.part, p.g);
            }
            return launch_status();
        });
    });
}

// pf_systematic without a cdf (k_chunk_scan + k_chunk_search): columns of several tiles of whole 4-vectors, one u per column, a
// tile's chunk bases within one workgroup's reach, and a grid the closed-form inversion is exact for (float: N <= 2^22)
static inline bool cdf_free_applies(const Geom& g, int dtype, int u_per_elem) {
    if (dtype != PF_F32 && dtype != PF_F64) return false;
    return g.tiles > 1 && g.vec == 4 && !u_per_elem && g.rounds_per_tile * (g.round_elems / PF_CHUNK) <= PF_BLOCK &&
           g.N < ((int64_t)1 << 31) - 4096 && !(dtype == PF_F32 && g.N > ((int64_t)1 << 22));
}
extern "C" int pf_systematic_cdf_free(int64_t N, int64_t B, int dtype, int u_per_element, int* yes) {
    if (!yes || bad_shape(N, B)) return PF_EINVAL;
    *yes = cdf_free_applies(make_geom(N, B), dtype, u_per_element) ? 1 : 0;
    return PF_OK;
}

static int systematic_impl(void* src, bool from_w, const void* u, int u_per_elem, const void* v, int multinomial, uint64_t seed,
                           uint32_t step, const uint8_t* colmask, void* cdf, int32_t* idx, int64_t N, int64_t B,
                           int dtype, void* ws, size_t ws_bytes, void* stream) {
    if (!src || !idx || !ws || bad_shape(N, B) || (!multinomial && !u)) return PF_EINVAL;
    const TileLaunch p(N, B, ws, stream);
    const Geom& g = p.g;
    if (ws_bytes < p.wl.total) return PF_EWORKSPACE;
    if (!cdf) {  // no cdf wanted: the two-launch form where it applies (pf_systematic_cdf_free), nothing else
        if (multinomial || !cdf_free_applies(g, dtype, u_per_elem)) return PF_EINVAL;
        double* cb = (double*)((char*)ws + p.wl.off_ctab);
        const int nchunks = (int)((N + PF_CHUNK - 1) / PF_CHUNK);
#ifdef PF_DEVTOOLS  // (the instrumented build: cycle stamps of the middle workgroup of column 0, tools/chunk_search_stages.py)
#define PF_CHUNK_DBG , (unsigned long long*)((char*)ws + p.wl.off_dbg)
#else
#define PF_CHUNK_DBG
#endif
        return with_dtype(dtype, [&](auto t) {
            return with_bool(from_w, [&](auto fw) {
                using T = decltype(t);
                constexpr bool FW = decltype(fw)::value;
                hipLaunchKernelGGL((k_chunk_scan<T, FW>), p.grid, dim3(PF_BLOCK), 0, p.st, (T*)src, colmask, p.part, cb, g, nchunks);
                hipLaunchKernelGGL((k_chunk_search<T, FW>), p.grid, dim3(PF_BLOCK), 0, p.st, (const T*)src, (const T*)u, colmask,
                                   (const double*)p.part, (const double*)cb, idx, g, nchunks PF_CHUNK_DBG);
                return launch_status();
            });
        });
#undef PF_CHUNK_DBG
    }
    void* tree = multinomial ? (void*)((char*)ws + p.wl.off_tree) : nullptr;  // (the iid draws' 16-ary search tables, written by the scan)
    return with_dtype(dtype, [&](auto t) {
        return with_vec(g.vec, [&](auto vec_c) {
            return with_bool(multinomial, [&](auto mn) {
                using T = decltype(t);
                constexpr int V = decltype(vec_c)::value;
                constexpr bool MN = decltype(mn)::value;
                if (g.tiles == 1) {  // one tile per column: record -> scan -> ancestors in one launch
                    with_bool(from_w, [&](auto fw) {
                        hipLaunchKernelGGL((k_resample_one_tile<T, V, decltype(fw)::value, MN>), p.grid, dim3(PF_BLOCK), 0, p.st, (T*)src,
                                           (const T*)u, u_per_elem, (const T*)v, seed, step, colmask, (T*)cdf, idx, p.part, g, (T*)tree);
                        return PF_OK;
                    });
                } else {
                    if (from_w) {
                        hipLaunchKernelGGL((k_tile_sum<T, V>), p.grid, dim3(PF_BLOCK), 0, p.st, (const T*)src, colmask, p.part, g);
                        hipLaunchKernelGGL((k_scan<T, V, true>), p.grid, dim3(PF_BLOCK), 0, p.st, (const T*)src, (T*)cdf, colmask,
                                           (const double*)p.part, g, (T*)tree);
                    } else {
                        hipLaunchKernelGGL((k_reduce_logw<T, V>), p.grid, dim3(PF_BLOCK), 0, p.st, (T*)src, 1, colmask, p.part, g);
                        hipLaunchKernelGGL((k_scan<T, V, false>), p.grid, dim3(PF_BLOCK), 0, p.st, (const T*)src, (T*)cdf, colmask,
                                           (const double*)p.part, g, (T*)tree);
                    }
                    hipLaunchKernelGGL((k_search<T, V, MN>), p.grid, dim3(PF_BLOCK), 0, p.st, (const T*)cdf, (const T*)u, u_per_elem,
                                       (const T*)v, seed, step, colmask, idx, g, /*force_search*/ 0, (const T*)tree);
                }
                return launch_status();
            });
        });
    });
}

extern "C" int pf_systematic(const void* W, const void* u, int u_per_element, const uint8_t* colmask, void* cdf,
                             int32_t* idx, int64_t N, int64_t B, int dtype, void* ws, size_t ws_bytes, void* stream) {
    return systematic_impl((void*)W, true, u, u_per_element, nullptr, 0, 0, 0, colmask, cdf, idx, N, B, dtype, ws,
                           ws_bytes, stream);
}

extern "C" int pf_systematic_logw(void* logw, const void* u, int u_per_element, const uint8_t* colmask, void* cdf,
                                  int32_t* idx, int64_t N, int64_t B, int dtype, void* ws, size_t ws_bytes,
                                  void* stream) {
    return systematic_impl(logw, false, u, u_per_element, nullptr, 0, 0, 0, colmask, cdf, idx, N, B, dtype, ws,
                           ws_bytes, stream);
}

extern "C" int pf_multinomial(const void* W, const void* v, uint64_t seed, uint32_t step, const uint8_t* colmask,
                              void* cdf, int32_t* idx, int64_t N, int64_t B, int dtype, void* ws, size_t ws_bytes,
                              void* stream) {
    return systematic_impl((void*)W, true, nullptr, 0, v, 1, seed, step, colmask, cdf, idx, N, B, dtype, ws, ws_bytes,
                           stream);
}

static inline int ew_blocks(int64_t N) {
    int64_t nb = (N + PF_BLOCK - 1) / PF_BLOCK;
    return (int)(nb > 2048 ? 2048 : nb);
}

extern "C" int pf_gather(const void* x, const int32_t* idx, const uint8_t* colmask, void* out, int64_t N, int64_t B,
                         int64_t D, int dtype, void* stream) {
    if (!x || !idx || !out || bad_shape(N, B) || D < 1 || x == out) return PF_EINVAL;
    const dim3 grid(ew_blocks(N), (int)B);
    hipStream_t st = (hipStream_t)stream;
    return with_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((k_gather<T>), grid, dim3(PF_BLOCK), 0, st, (const T*)x, idx, colmask, (T*)out, N, (int)B, (int)D);
        return launch_status();
    });
}

static int columns_move(const void* src, const int64_t* idx, const uint8_t* mask, void* dst, int64_t N, int64_t B,
                        int64_t planes, int elem_bytes, void* stream) {
    if (!src || !dst || bad_shape(N, B) || planes < 1 || planes > 65535 || (elem_bytes != 4 && elem_bytes != 8)) return PF_EINVAL;
    const int64_t col_bytes = N * elem_bytes;
    const dim3 grid((unsigned)((col_bytes + PF_COLCHUNK - 1) / PF_COLCHUNK), (unsigned)B, (unsigned)planes);
    hipStream_t st = (hipStream_t)stream;
    const uintptr_t al = (uintptr_t)src | (uintptr_t)dst | (uintptr_t)col_bytes;
    const char* s = (const char*)src;
    char* d = (char*)dst;
    if ((al & 15) == 0) hipLaunchKernelGGL((k_columns_move<pf_v4u>), grid, dim3(PF_BLOCK), 0, st, s, idx, mask, d, col_bytes, (int)B);
    else if ((al & 7) == 0) hipLaunchKernelGGL((k_columns_move<pf_v2u>), grid, dim3(PF_BLOCK), 0, st, s, idx, mask, d, col_bytes, (int)B);
    else hipLaunchKernelGGL((k_columns_move<uint32_t>), grid, dim3(PF_BLOCK), 0, st, s, idx, mask, d, col_bytes, (int)B);
    PF_CHECK_LAUNCH();
    return PF_OK;
}

extern "C" int pf_columns_gather(const void* src, const int64_t* idx, void* dst, int64_t N, int64_t B, int64_t planes,
                                 int elem_bytes, void* stream) {
    if (!idx || src == dst) return PF_EINVAL;  // out of place only: a gather may read columns it has already overwritten
    return columns_move(src, idx, nullptr, dst, N, B, planes, elem_bytes, stream);
}

extern "C" int pf_columns_exchange(void* dst, const void* src, const uint8_t* mask, int64_t N, int64_t B, int64_t planes,
                                   int elem_bytes, void* stream) {
    if (!mask) return PF_EINVAL;
    return columns_move(src, nullptr, mask, dst, N, B, planes, elem_bytes, stream);
}

extern "C" int pf_loglik(const void* v, const void* W, void* out, int64_t N, int64_t B, int dtype, void* ws,
                         size_t ws_bytes, void* stream) {
    if (!v || !out || !ws || bad_shape(N, B)) return PF_EINVAL;
    const TileLaunch p(N, B, ws, stream);
    if (ws_bytes < p.wl.total) return PF_EWORKSPACE;
    return with_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((k_loglik_part<T>), p.grid, dim3(PF_BLOCK), 0, p.st, (const T*)v, (const T*)W, p.part, p.g);
        hipLaunchKernelGGL((k_loglik_final<T>), dim3(p.g.B), dim3(PF_BLOCK), 0, p.st, (const double*)p.part, (T*)out, p.g);
        return launch_status();
    });
}

extern "C" int pf_moments(const void* x, const void* W, void* mean, void* var, int64_t N, int64_t B, int64_t D,
                          int dtype, void* ws, size_t ws_bytes, void* stream) {
    if (!x || !W || !mean || !var || !ws || bad_shape(N, B) || D < 1) return PF_EINVAL;
    return with_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        const TileLaunch p(N, B, ws, stream);
        if (ws_bytes < p.wl.total) return PF_EWORKSPACE;
        // the planes in groups of PF_MAXD (one pair of launches per group, the same partial slots reused in stream order)
        const int64_t plane = N * B;
        for (int64_t d0 = 0; d0 < D; d0 += PF_MAXD) {
            const int dg = (int)((D - d0) < PF_MAXD ? (D - d0) : PF_MAXD);
            hipLaunchKernelGGL((k_moments_part<T>), p.grid, dim3(PF_BLOCK), 0, p.st, (const T*)x + d0 * plane, (const T*)W, p.part, p.g, dg);
            hipLaunchKernelGGL((k_moments_final<T>), dim3(p.g.B), dim3(PF_BLOCK), 0, p.st, (const double*)p.part, (const T*)x + d0 * plane, (T*)mean, (T*)var, p.g,
                               dg, (int)d0, (int)D);
            PF_CHECK_LAUNCH();
        }
        return PF_OK;
    });
}



extern "C" int pf_pre_weight(const pf_model* model, int proposal, const void* x, const void* y, int64_t y_rows,
                             void* out, int64_t N, int64_t B, int dtype, void* stream) {
    int rc = check_model(model);
    if (rc) return rc;
    if (!x || !y || !out || bad_shape(N, B) || (y_rows != 1 && y_rows != B)) return PF_EINVAL;
    if (proposal == PF_PROP_LGO && model->obs_kind != PF_OBS_LINEAR) return PF_EUNSUPPORTED;
    const ModelDesc md = to_desc(model);
    const dim3 grid(ew_blocks(N), (int)B);
    hipStream_t st = (hipStream_t)stream;
    return with_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        if (model->hid_kind == PF_HID_LINEAR_MAT)
            return with_d8(model->dim, [&](auto d) {
                hipLaunchKernelGGL((k_linmat_pre_weight<T, decltype(d)::value>), grid, dim3(PF_BLOCK), 0, st, (const T*)model->params,
                                   (int)model->obs_dim, proposal, (const T*)x, (const T*)y, (int)y_rows, (T*)out, N, (int)B);
                return launch_status();
            });
        return with_d3(model->dim, [&](auto d) {
            hipLaunchKernelGGL((k_pre_weight<T, decltype(d)::value>), grid, dim3(PF_BLOCK), 0, st, md, (const T*)model->params, proposal,
                               (const T*)x, (const T*)y, (int)y_rows, (T*)out, N, (int)B);
            return launch_status();
        });
    });
}

extern "C" int pf_sample_and_weight(const pf_model* model, int proposal, int weigh, const void* x, const void* y,
                                    int64_t y_rows, const void* z, uint64_t seed, uint32_t step, void* x_out,
                                    void* w_out, int64_t N, int64_t B, int dtype, void* stream) {
    int rc = check_model(model);
    if (rc) return rc;
    if (!x || !x_out || bad_shape(N, B) || (weigh && (!y || !w_out)) || (y_rows != 1 && y_rows != B)) return PF_EINVAL;
    if (proposal == PF_PROP_LGO && model->obs_kind != PF_OBS_LINEAR) return PF_EUNSUPPORTED;
    const ModelDesc md = to_desc(model);
    const dim3 grid(ew_blocks(N), (int)B);
    hipStream_t st = (hipStream_t)stream;
    return with_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        if (model->hid_kind == PF_HID_LINEAR_MAT)
            return with_d8(model->dim, [&](auto d) {
                hipLaunchKernelGGL((k_linmat_sample_and_weight<T, decltype(d)::value>), grid, dim3(PF_BLOCK), 0, st, (const T*)model->params,
                                   (int)model->obs_dim, proposal, weigh, (const T*)x, (const T*)y, (int)y_rows, (const T*)z, seed, step,
                                   (T*)x_out, (T*)w_out, N, (int)B);
                return launch_status();
            });
        return with_d3(model->dim, [&](auto d) {
            hipLaunchKernelGGL((k_sample_and_weight<T, decltype(d)::value>), grid, dim3(PF_BLOCK), 0, st, md, (const T*)model->params,
                               proposal, weigh, (const T*)x, (const T*)y, (int)y_rows, (const T*)z, seed, step, (T*)x_out, (T*)w_out, N,
                               (int)B);
            return launch_status();
        });
    });
}

// ---- the nested proposal (pf_nested.hpp) --------------------------------------------------------------------------------
#include "pf_nested.hpp"
extern "C" int pf_nested_sample_and_weight(const pf_model* model, int num_samples, const void* x, const void* y, int64_t y_rows,
                                           const void* z, const void* v, uint64_t seed, uint32_t step, void* x_out, void* w_out,
                                           int32_t* pick_out, int64_t N, int64_t B, int dtype, void* stream) {
    int rc = check_model(model);
    if (rc) return rc;
    if (model->hid_kind == PF_HID_LINEAR_MAT) return PF_EUNSUPPORTED;  // (the callers' torch route)
    if (!x || !y || !x_out || !w_out || bad_shape(N, B) || (y_rows != 1 && y_rows != B) || num_samples < 1 ||
        num_samples > PF_NESTED_MAX)
        return PF_EINVAL;
    const ModelDesc md = to_desc(model);
    const dim3 grid(ew_blocks(N), (int)B);
    hipStream_t st = (hipStream_t)stream;
    return with_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        return with_d3(model->dim, [&](auto d) {
            hipLaunchKernelGGL((k_nested_sample_and_weight<T, decltype(d)::value>), grid, dim3(PF_BLOCK), 0, st, md, (const T*)model->params,
                               num_samples, (const T*)x, (const T*)y, (int)y_rows, (const T*)z, (const T*)v, seed, step, (T*)x_out,
                               (T*)w_out, pick_out, N, (int)B);
            return launch_status();
        });
    });
}

// ---- forecasting (pf_forecast.hpp) ----------------------------------------------------------------------------------------
#include "pf_forecast.hpp"
static inline int64_t forecast_tiles(int64_t N) { return (N + PF_FC_TILE - 1) / PF_FC_TILE; }
// the built-in kinds of the stand-alone model kernels with D, O <= 3; everything else is PF_EINVAL here (the callers' torch route)
static inline bool forecast_takes(const pf_model* m) {
    return m && m->params && m->hid_kind != PF_HID_LINEAR_MAT && m->hid_kind != PF_HID_USER_AFFINE && check_model(m) == PF_OK;
}
extern "C" int pf_forecast_workspace_bytes(int64_t N, int64_t B, int steps, size_t* bytes) {
    if (!bytes || bad_shape(N, B) || steps < 1) return PF_EINVAL;
    *bytes = sizeof(double) * (size_t)steps * PF_FC_Q * (size_t)B * (size_t)forecast_tiles(N);
    return PF_OK;
}
extern "C" int pf_forecast(const pf_model* model, int steps, const void* x, const void* W, const void* z, const void* e, uint64_t seed,
                           void* x_mean, void* x_var, void* y_mean, void* y_var, void* x_path, void* y_path, void* ws, size_t ws_bytes,
                           int64_t N, int64_t B, int dtype, void* stream) {
    if (!forecast_takes(model) || steps < 1 || !x || !x_mean || !x_var || !y_mean || !y_var || !ws || bad_shape(N, B)) return PF_EINVAL;
    size_t need = 0;
    pf_forecast_workspace_bytes(N, B, steps, &need);
    if (ws_bytes < need) return PF_EWORKSPACE;
    const ModelDesc md = to_desc(model);
    const int tiles = (int)forecast_tiles(N);
    hipStream_t st = (hipStream_t)stream;
    return with_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        return with_d3(model->dim, [&](auto d) {
            hipLaunchKernelGGL((k_forecast_part<T, decltype(d)::value>), dim3(tiles, (int)B), dim3(PF_BLOCK), 0, st, md, (const T*)model->params,
                               steps, (const T*)x, (const T*)W, (const T*)z, (const T*)e, seed, (double*)ws, (T*)x_path, (T*)y_path, N, (int)B);
            hipLaunchKernelGGL((k_forecast_final<T, decltype(d)::value>), dim3(steps, (int)B), dim3(PF_BLOCK), 0, st, md, (const T*)model->params,
                               (const T*)x, (const double*)ws, (T*)x_mean, (T*)x_var, (T*)y_mean, (T*)y_var, N, (int)B, tiles);
            return launch_status();
        });
    });
}

// ---- path score (pf_score.hpp) ----------------------------------------------------------------------------------------------
#include "pf_score.hpp"
extern "C" int pf_path_score_workspace_bytes(int64_t N, int64_t B, int64_t S, size_t* bytes) {
    if (!bytes || bad_shape(N, B) || S < 2 || S > INT32_MAX) return PF_EINVAL;
    const ScorePlan p = score_plan(N, B, S);
    *bytes = sizeof(double) * (size_t)PF_SCORE_Q * (size_t)B * (size_t)p.tiles * (size_t)p.chunks;
    return PF_OK;
}
extern "C" int pf_path_score(const pf_model* model, const void* paths, const void* y, int64_t y_rows, double* value, double* grad,
                             void* ws, size_t ws_bytes, int64_t S, int64_t N, int64_t B, int dtype, void* stream) {
    if (!model || !model->params || !paths || !y || !value || !grad || !ws) return PF_EINVAL;
    if (model->hid_kind == PF_HID_LINEAR_MAT || model->hid_kind == PF_HID_USER_AFFINE) return PF_EUNSUPPORTED;
    int rc = check_model(model);  // (D or O above 3, an unknown kind: PF_EUNSUPPORTED)
    if (rc) return rc;
    if (S < 2 || S > INT32_MAX || bad_shape(N, B) || (y_rows != 1 && y_rows != B)) return PF_EINVAL;
    size_t need = 0;
    pf_path_score_workspace_bytes(N, B, S, &need);
    if (ws_bytes < need) return PF_EWORKSPACE;
    const ModelDesc md = to_desc(model);
    const ScorePlan p = score_plan(N, B, S);
    const int NP = PF_BUILTIN_ROW_LEN(model->dim, model->obs_dim);
    hipStream_t st = (hipStream_t)stream;
    return with_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        return with_d3(model->dim, [&](auto d) {
            hipLaunchKernelGGL((k_score_part<T, decltype(d)::value>), dim3((unsigned)p.tiles, (unsigned)B, (unsigned)p.chunks), dim3(PF_BLOCK), 0,
                               st, md, (const T*)model->params, (const T*)paths, (const T*)y, (int)y_rows, (double*)ws, (int)S, p.len, N,
                               (int)B);
            hipLaunchKernelGGL(k_score_final, dim3(1 + NP, (unsigned)B), dim3(PF_BLOCK), 0, st, (const double*)ws, value, grad,
                               p.tiles * p.chunks, N, (int)B);
            return launch_status();
        });
    });
}

// ---- PF_HID_LINEAR_MAT after the filter (pf_linear_smooth.hpp) -------------------------------------------------------------
#include "pf_smooth.hpp"  // (k_trace_ancestors, k_ffbs: their entries are in the smoothing section below)
#include "pf_linear_smooth.hpp"
// the one model these entry points serve: PF_HID_LINEAR_MAT under PF_OBS_LINEAR with 1 <= D, O <= 8
static inline int check_linmat(const pf_model* m) {
    if (!m || !m->params) return PF_EINVAL;
    if (m->hid_kind != PF_HID_LINEAR_MAT) return PF_EUNSUPPORTED;
    return check_model(m);
}
extern "C" int pf_path_score_linear_workspace_bytes(int64_t N, int64_t B, int64_t S, int64_t D, int64_t O, size_t* bytes) {
    if (!bytes || bad_shape(N, B) || S < 2 || S > INT32_MAX) return PF_EINVAL;
    if (D < 1 || D > PF_LIN_MAXD || O < 1 || O > PF_LIN_MAXO) return PF_EUNSUPPORTED;
    const ScorePlan p = score_plan(N, B, S);
    const size_t groups = (size_t)(lscore_groups((int)D) + lscore_groups((int)O));
    *bytes = sizeof(double) * groups * (size_t)lscore_q((int)D) * (size_t)B * (size_t)p.tiles * (size_t)p.chunks;
    return PF_OK;
}
extern "C" int pf_path_score_linear(const pf_model* model, const void* paths, const void* y, int64_t y_rows, double* value,
                                    double* grad, void* ws, size_t ws_bytes, int64_t S, int64_t N, int64_t B, int dtype,
                                    void* stream) {
    if (!model || !model->params || !paths || !y || !value || !grad || !ws) return PF_EINVAL;
    int rc = check_linmat(model);
    if (rc) return rc;
    if (S < 2 || S > INT32_MAX || bad_shape(N, B) || (y_rows != 1 && y_rows != B)) return PF_EINVAL;
    const int D = model->dim, O = model->obs_dim;
    size_t need = 0;
    pf_path_score_linear_workspace_bytes(N, B, S, D, O, &need);
    if (ws_bytes < need) return PF_EWORKSPACE;
    const ScorePlan p = score_plan(N, B, S);
    const int groups = lscore_groups(D) + lscore_groups(O);
    const int NP = PF_LINMAT_ROW_LEN(D, O);
    hipStream_t st = (hipStream_t)stream;
    return with_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        return with_d8(D, [&](auto d) {
            trace_launch(0, (int)sizeof(T), D, 1, 0, 0, 0, PF_TRACE_SCORE_LINEAR, 0, 0);
            hipLaunchKernelGGL((k_score_linmat_part<T, decltype(d)::value>), dim3((unsigned)p.tiles, (unsigned)B, (unsigned)(p.chunks * groups)),
                               dim3(PF_BLOCK), 0, st, (const T*)model->params, O, (const T*)paths, (const T*)y, (int)y_rows, (double*)ws,
                               (int)S, p.len, groups, N, (int)B);
            hipLaunchKernelGGL(k_score_linmat_final, dim3(1 + NP, (unsigned)B), dim3(PF_BLOCK), 0, st, (const double*)ws, value, grad, D, O,
                               p.tiles * p.chunks, N, (int)B);
            return launch_status();
        });
    });
}

// ---- forecasting for PF_HID_LINEAR_MAT (pf_forecast_linear.hpp) -----------------------------------------------------------------
#include "pf_forecast_linear.hpp"
static inline int64_t linfc_tiles(int64_t N, int D) { return (N + PF_BLOCK * linfc_items(D) - 1) / (PF_BLOCK * linfc_items(D)); }
extern "C" int pf_forecast_linear_workspace_bytes(int64_t N, int64_t B, int steps, int64_t D, int64_t O, int covariance, size_t* bytes) {
    if (!bytes || bad_shape(N, B) || steps < 1) return PF_EINVAL;
    if (D < 1 || D > PF_LIN_MAXD || O < 1 || O > PF_LIN_MAXO) return PF_EUNSUPPORTED;
    *bytes = sizeof(double) * (size_t)steps * (size_t)linfc_q((int)D, (int)O, covariance != 0) * (size_t)B * (size_t)linfc_tiles(N, (int)D);
    return PF_OK;
}
extern "C" int pf_forecast_linear(const pf_model* model, int steps, const void* x, const void* W, const void* z, const void* e,
                                  uint64_t seed, void* x_mean, void* x_var, void* y_mean, void* y_var, void* x_cov, void* y_cov,
                                  void* x_path, void* y_path, void* ws, size_t ws_bytes, int64_t N, int64_t B, int dtype, void* stream) {
    if (!model || !model->params || steps < 1 || !x || !x_mean || !x_var || !y_mean || !y_var || !ws || (!x_cov) != (!y_cov)) return PF_EINVAL;
    int rc = check_linmat(model);
    if (rc) return rc;
    if (bad_shape(N, B)) return PF_EINVAL;
    const int D = model->dim, O = model->obs_dim;
    const bool cov = x_cov != nullptr;
    size_t need = 0;
    rc = pf_forecast_linear_workspace_bytes(N, B, steps, D, O, cov, &need);
    if (rc) return rc;
    if (ws_bytes < need) return PF_EWORKSPACE;
    const int tiles = (int)linfc_tiles(N, D);
    hipStream_t st = (hipStream_t)stream;
    return with_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        return with_d8(D, [&](auto d) {
            return with_bool(cov, [&](auto c) {
                constexpr int DD = decltype(d)::value;
                constexpr bool CV = decltype(c)::value;
                hipLaunchKernelGGL((k_forecast_linmat_part<T, DD, CV>), dim3(tiles, (int)B), dim3(PF_BLOCK), 0, st, (const T*)model->params, O,
                                   steps, (const T*)x, (const T*)W, (const T*)z, (const T*)e, seed, (double*)ws, (T*)x_path, (T*)y_path, N,
                                   (int)B);
                hipLaunchKernelGGL((k_forecast_linmat_final<T, DD, CV>), dim3(steps, (int)B), dim3(PF_BLOCK), 0, st, (const T*)model->params, O,
                                   (const T*)x, (const double*)ws, (T*)x_mean, (T*)x_var, (T*)y_mean, (T*)y_var, (T*)x_cov, (T*)y_cov, N,
                                   (int)B, tiles);
                return launch_status();
            });
        });
    });
}

extern "C" int pf_initial_sample(const double* m0, const double* s0, const void* z, uint64_t seed, void* x, int64_t N,
                                 int64_t B, int64_t D, int dtype, void* stream) {
    if (!m0 || !s0 || !x || bad_shape(N, B) || D < 1) return PF_EINVAL;
    const dim3 grid(ew_blocks(N), (int)B);
    hipStream_t st = (hipStream_t)stream;
    // planes in groups of PF_MAXD; group k draws its Philox normals at step k (group 0: the draws of a D <= 3 state)
    const int64_t plane = N * B;
    return with_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        for (int64_t d0 = 0; d0 < D; d0 += PF_MAXD) {
            const int dg = (int)((D - d0) < PF_MAXD ? (D - d0) : PF_MAXD);
            double m[3] = {0, 0, 0}, s[3] = {0, 0, 0};
            for (int d = 0; d < dg; ++d) { m[d] = m0[d0 + d]; s[d] = s0[d0 + d]; }
            const uint32_t grp = (uint32_t)(d0 / PF_MAXD);
            hipLaunchKernelGGL((k_initial_sample<T>), grid, dim3(PF_BLOCK), 0, st, m[0], m[1], m[2], s[0], s[1], s[2],
                               z ? (const T*)z + d0 * plane : nullptr, seed, (T*)x + d0 * plane, N, (int)B, dg, grp);
            PF_CHECK_LAUNCH();
        }
        return PF_OK;
    });
}


extern "C" int pf_initial_sample_cols(const void* m0, int64_t m0_stride_b, int64_t m0_stride_d, const void* s0, int64_t s0_stride_b,
                                      int64_t s0_stride_d, const void* z, uint64_t seed, void* x, int64_t N, int64_t B, int64_t D,
                                      int dtype, void* stream) {
    if (!m0 || !s0 || !x || bad_shape(N, B) || D < 1 || m0_stride_b < 0 || m0_stride_d < 0 || s0_stride_b < 0 ||
        s0_stride_d < 0)
        return PF_EINVAL;
    const dim3 grid(ew_blocks(N), (int)B);
    hipStream_t st = (hipStream_t)stream;
    // (the plane groups of pf_initial_sample, the same draws)
    const int64_t plane = N * B;
    return with_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        for (int64_t d0 = 0; d0 < D; d0 += PF_MAXD) {
            const int dg = (int)((D - d0) < PF_MAXD ? (D - d0) : PF_MAXD);
            const uint32_t grp = (uint32_t)(d0 / PF_MAXD);
            hipLaunchKernelGGL((k_initial_sample_cols<T>), grid, dim3(PF_BLOCK), 0, st, (const T*)m0 + d0 * m0_stride_d, m0_stride_b,
                               m0_stride_d, (const T*)s0 + d0 * s0_stride_d, s0_stride_b, s0_stride_d,
                               z ? (const T*)z + d0 * plane : nullptr, seed, (T*)x + d0 * plane, N, (int)B, dg, grp);
            PF_CHECK_LAUNCH();
        }
        return PF_OK;
    });
}

extern "C" int pf_observed_flags(const void* y, int64_t steps, int64_t row_elems, int dtype, uint8_t* out, void* stream) {
    if (!y || !out || steps < 0 || row_elems < 1 || steps > 0x7fffffff) return PF_EINVAL;
    if (steps == 0) return PF_OK;
    hipStream_t st = (hipStream_t)stream;
    return with_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((k_observed_flags<T>), dim3((unsigned)steps), dim3(PF_WAVE), 0, st, (const T*)y, row_elems, out);
        return launch_status();
    });
}

// ---- theta-level kernels (pf_theta.hpp) ---------------------------------------------------------------------------------
#include "pf_theta.hpp"
extern "C" int pf_theta_fit(const void* values, const void* logw, int64_t B, int32_t P, double scale, int dtype, void* mean,
                            void* chol, void* stream) {
    if (!values || !mean || !chol || B < 1 || P < 1 || P > PF_THETA_MAXP) return PF_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    return with_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((k_theta_fit<T>), dim3(1), dim3(PF_BLOCK), 0, st, (const T*)values, (const T*)logw, B, (int)P, scale, (T*)mean,
                           (T*)chol);
        return launch_status();
    });
}

extern "C" int pf_theta_propose(const pf_theta_priors* priors, const void* mean, const void* chol, const void* eps, int64_t B,
                                int dtype, void* u_out, void* const* x_out, void* prior_out, void* stream) {
    if (!priors || !mean || !chol || !eps || !u_out || !x_out || !prior_out || B < 1 || priors->P < 1 || priors->P > PF_THETA_MAXP)
        return PF_EINVAL;
    ThetaPriors pr;
    ThetaOut out;
    pr.P = priors->P;
    for (int p = 0; p < PF_THETA_MAXP; ++p) {
        pr.kind[p] = p < pr.P ? priors->kind[p] : 0;
        pr.a[p] = p < pr.P ? priors->a[p] : 0.0;
        pr.b[p] = p < pr.P ? priors->b[p] : 1.0;
        out.x[p] = p < pr.P ? x_out[p] : nullptr;
        if (p < pr.P && (!x_out[p] || pr.kind[p] < 0 || pr.kind[p] > PF_PRIOR_UNIFORM)) return PF_EINVAL;
    }
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)((B + PF_BLOCK - 1) / PF_BLOCK));
    return with_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((k_theta_propose<T>), grid, dim3(PF_BLOCK), 0, st, pr, (const T*)mean, (const T*)chol, (const T*)eps, B,
                           (T*)u_out, out, (T*)prior_out);
        return launch_status();
    });
}

extern "C" int pf_theta_accept(const void* u_cur, const void* u_star, const void* mean_f, const void* chol_f, const void* mean_r,
                               const void* chol_r, const void* prior_cur, const void* prior_star, const void* ll_cur,
                               const void* ll_star, const void* unif, int64_t B, int32_t P, int dtype, void* log_acc,
                               uint8_t* accepted, void* rate, void* stream) {
    if (!u_cur || !u_star || !mean_f || !chol_f || !mean_r || !chol_r || !prior_cur || !prior_star || !ll_cur || !ll_star || !unif ||
        !log_acc || !accepted || !rate || B < 1 || P < 1 || P > PF_THETA_MAXP)
        return PF_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    return with_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((k_theta_accept<T>), dim3(1), dim3(PF_BLOCK), 0, st, (const T*)u_cur, (const T*)u_star, (const T*)mean_f,
                           (const T*)chol_f, (const T*)mean_r, (const T*)chol_r, (const T*)prior_cur, (const T*)prior_star,
                           (const T*)ll_cur, (const T*)ll_star, (const T*)unif, B, (int)P, (T*)log_acc, accepted, (T*)rate);
        return launch_status();
    });
}

extern "C" int pf_theta_path(const void* w0, const void* ll, int64_t n, int64_t B, int dtype, void* w_path, void* stats,
                             void* host_rows, uint64_t seq, const int32_t* status, void* stream) {
    if (!w0 || !ll || !w_path || !stats || B < 1 || n < 0 || n > 65535 || ((uintptr_t)host_rows & 7) != 0) return PF_EINVAL;
    if (n == 0) return PF_OK;
    hipStream_t st = (hipStream_t)stream;
    return with_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((k_theta_path<T>), dim3((unsigned)n), dim3(PF_BLOCK), 0, st, (const T*)w0, (const T*)ll, B, (T*)w_path,
                           (T*)stats, (double*)host_rows, (unsigned long long)seq, (T*)nullptr, (const int*)status, 1);
        return launch_status();
    });
}

extern "C" int pf_theta_step(void* w, const void* ll, int64_t B, int dtype, void* stats, void* host_slot, uint64_t seq, void* acc,
                             const int32_t* status, void* stream) {
    if (!w || !ll || !stats || B < 1 || ((uintptr_t)host_slot & 7) != 0) return PF_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    return with_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((k_theta_path<T>), dim3(1), dim3(PF_BLOCK), 0, st, (const T*)w, (const T*)ll, B, (T*)w, (T*)stats,
                           (double*)host_slot, (unsigned long long)seq, (T*)acc, (const int*)status);
        return launch_status();
    });
}

extern "C" int pf_host_alloc(size_t bytes, void** out) {
    if (!out || bytes == 0) return PF_EINVAL;
    *out = nullptr;
    // coherent (fine-grained) + mapped: a device store with system scope is visible to a polling host thread while the stream runs on
    const hipError_t e = hipHostMalloc(out, bytes, hipHostMallocCoherent | hipHostMallocMapped);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        *out = nullptr;
        return (int)e;  // (a HIP error code, like a failed launch)
    }
    memset(*out, 0, bytes);
    return PF_OK;
}

extern "C" int pf_host_free(void* p) {
    if (!p) return PF_OK;
    const hipError_t e = hipHostFree(p);
    if (e != hipSuccess) (void)hipGetLastError();
    return e == hipSuccess ? PF_OK : (int)e;
}

extern "C" int pf_theta_resample(const void* logw, int64_t B, double u, int dtype, int64_t* ancestors, void* cdf_scratch,
                                 void* stream) {
    if (!logw || !ancestors || !cdf_scratch || B < 1 || !(u >= 0.0 && u <= 1.0)) return PF_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    return with_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((k_theta_resample<T>), dim3(1), dim3(PF_BLOCK), 0, st, (const T*)logw, B, u, ancestors, (T*)cdf_scratch);
        return launch_status();
    });
}

// ---- NESS: the jittering kernels (pf_jitter.hpp) ---------------------------------------------------------------------------
#include "pf_jitter.hpp"
static inline bool jitter_kind_ok(int kind, double par) {
    if (kind < PF_JITTER_NONSHRINKING || kind > PF_JITTER_CONSTANT) return false;
    return kind != PF_JITTER_LIUWEST || (par >= 0.0 && par <= 1.0);
}

extern "C" int pf_jitter_fit(const void* values, const void* logw, int64_t B, int32_t P, int32_t kind, double par, const void* scale,
                             double min_std, double bw_lo, double bw_hi, int dtype, double* fit, void* mean, void* scale_out,
                             void* stream) {
    if (!values || !logw || !fit || B < 1 || B > PF_JITTER_MAXB || P < 1 || P > PF_THETA_MAXP || !jitter_kind_ok(kind, par))
        return PF_EINVAL;
    int n2 = 1;
    while (n2 < (int)B) n2 <<= 1;
    const size_t lds = kind == PF_JITTER_CONSTANT ? 0 : (size_t)n2 * (sizeof(double) + sizeof(int));
    hipStream_t st = (hipStream_t)stream;
    return with_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        auto kernel = k_jitter_fit<T>;
        if (lds > 64 * 1024 && hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
            (void)hipGetLastError();
            return (int)PF_EINVAL;
        }
        hipLaunchKernelGGL(kernel, dim3((unsigned)P), dim3(PF_BLOCK), lds, st, (const T*)values, (const T*)logw, (int)B, (int)P, n2,
                           (int)kind, par, (const T*)scale, min_std, bw_lo, bw_hi, fit, (T*)mean, (T*)scale_out);
        return launch_status();
    });
}

extern "C" int pf_jitter_apply(const pf_theta_priors* priors, const void* values, const int64_t* ancestors, const double* fit, int64_t B,
                               int32_t kind, double par, double bw_lo, double bw_hi, int32_t discrete, const void* eps,
                               const void* select, uint64_t seed, uint64_t counter, int dtype, void* u_out, void* const* x_out,
                               void* stream) {
    if (!priors || !values || !ancestors || !fit || !u_out || !x_out || B < 1 || B > 0x7fffffff || priors->P < 1 ||
        priors->P > PF_THETA_MAXP || !jitter_kind_ok(kind, par))
        return PF_EINVAL;
    ThetaPriors pr;
    ThetaOut out;
    pr.P = priors->P;
    for (int p = 0; p < PF_THETA_MAXP; ++p) {
        pr.kind[p] = p < pr.P ? priors->kind[p] : 0;
        pr.a[p] = p < pr.P ? priors->a[p] : 0.0;
        pr.b[p] = p < pr.P ? priors->b[p] : 1.0;
        out.x[p] = p < pr.P ? x_out[p] : nullptr;
        if (p < pr.P && (!x_out[p] || pr.kind[p] < 0 || pr.kind[p] > PF_PRIOR_UNIFORM)) return PF_EINVAL;
    }
    JitterDraws dr;
    dr.eps = eps;
    dr.select = select;
    dr.seed = (unsigned long long)seed;
    dr.counter = (unsigned long long)counter;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)((B + PF_BLOCK - 1) / PF_BLOCK));
    return with_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((k_jitter_apply<T>), grid, dim3(PF_BLOCK), 0, st, pr, (const T*)values, ancestors, fit, (int)B, (int)kind, par,
                           bw_lo, bw_hi, (int)discrete, 1.0 / sqrt((double)B), dr, (T*)u_out, out);
        return launch_status();
    });
}

extern "C" int pf_theta_ess(const void* logw, int64_t rows, int64_t B, int dtype, void* out, void* stream) {
    if (!logw || !out || B < 1 || rows < 0 || rows > 0x7fffffff) return PF_EINVAL;
    if (rows == 0) return PF_OK;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)rows);
    return with_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((k_theta_ess<T>), grid, dim3(PF_BLOCK), 0, st, (const T*)logw, B, (T*)out);
        return launch_status();
    });
}



// ---- smoothing ---------------------------------------------------------------------------------------------------------
extern "C" int pf_smooth_fixed_lag(const void* x_hist, const int32_t* anc_hist, void* out, int64_t S, int64_t N, int64_t B,
                                   int64_t D, int dtype, void* stream) {
    if (!x_hist || !anc_hist || !out || S < 1 || bad_shape(N, B) || D < 1) return PF_EINVAL;  // (any D: the planes are looped)
    const dim3 grid(ew_blocks(N), (int)B);
    hipStream_t st = (hipStream_t)stream;
    return with_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((k_trace_ancestors<T>), grid, dim3(PF_BLOCK), 0, st, (const T*)x_hist, anc_hist, (T*)out, S, N, (int)B, (int)D);
        return launch_status();
    });
}

extern "C" int pf_smooth_ffbs(const pf_model* model, const void* x_hist, const void* logw_hist, const void* x_last,
                              const void* u, uint64_t seed, void* out, int64_t S, int64_t N, int64_t B, int dtype,
                              void* stream) {
    if (!model || !x_hist || !logw_hist || !x_last || !out || S < 1 || bad_shape(N, B)) return PF_EINVAL;
    int rc = check_model(model);
    if (rc) return rc;
    if (model->hid_kind == PF_HID_LINEAR_MAT) return PF_EUNSUPPORTED;  // (the callers' torch-logits route: no k_ffbs of this kind)
    const ModelDesc md = to_desc(model);
    const dim3 grid((unsigned)((N + PF_BLOCK - 1) / PF_BLOCK), (int)B);
    hipStream_t st = (hipStream_t)stream;
    return with_dtype(dtype, [&](auto t) {
        return with_d3(model->dim, [&](auto d) {
            using T = decltype(t);
            hipLaunchKernelGGL((k_ffbs<T, decltype(d)::value>), grid, dim3(PF_BLOCK), 0, st, md, (const T*)model->params, (const T*)x_hist,
                               (const T*)logw_hist, (const T*)x_last, (const T*)u, seed, (T*)out, S, N, (int)B);
            return launch_status();
        });
    });
}

extern "C" int pf_smooth_ffbs_linear(const pf_model* model, const void* x_hist, const void* logw_hist, const void* x_last,
                                     const void* u, uint64_t seed, void* out, int64_t S, int64_t N, int64_t B, int dtype,
                                     void* stream) {
    if (!model || !x_hist || !logw_hist || !x_last || !out || S < 1 || bad_shape(N, B)) return PF_EINVAL;
    int rc = check_linmat(model);
    if (rc) return rc;
    const dim3 grid((unsigned)((N + PF_BLOCK - 1) / PF_BLOCK), (int)B);
    hipStream_t st = (hipStream_t)stream;
    return with_dtype(dtype, [&](auto t) {
        return with_d8(model->dim, [&](auto d) {
            using T = decltype(t);
            trace_launch(0, (int)sizeof(T), model->dim, 1, 0, 0, 0, PF_TRACE_FFBS_LINEAR, 0, 0);
            hipLaunchKernelGGL((k_ffbs_linmat<T, decltype(d)::value>), grid, dim3(PF_BLOCK), 0, st, (const T*)model->params, model->obs_dim,
                               (const T*)x_hist, (const T*)logw_hist, (const T*)x_last, (const T*)u, seed, (T*)out, S, N, (int)B);
            return launch_status();
        });
    });
}

// ---- backward simulation by Metropolis-Hastings (pf_smooth_mh.hpp) ----------------------------------------------------------
#include "pf_smooth_mh.hpp"
// the cdf planes (S - 1, B, N) of doubles, then one int64 per (t, b)
extern "C" int pf_smooth_mh_workspace_bytes(int64_t N, int64_t B, int64_t S, size_t* bytes) {
    if (!bytes || bad_shape(N, B) || S < 1) return PF_EINVAL;
    *bytes = sizeof(double) * (size_t)(S - 1) * (size_t)B * ((size_t)N + 1);
    return PF_OK;
}
extern "C" int pf_smooth_mh(const pf_model* model, const void* x_hist, const void* logw_hist, const int32_t* anc_hist,
                            const int32_t* idx_last, const void* u, uint64_t seed, int mcmc_steps, void* out, int32_t* idx_out,
                            int64_t S, int64_t N, int64_t B, int dtype, void* ws, size_t ws_bytes, void* stream) {
    if (!model || !x_hist || !logw_hist || !anc_hist || !idx_last || !out || mcmc_steps < 0 || S < 1 || bad_shape(N, B)) return PF_EINVAL;
    if (dtype != PF_F32 && dtype != PF_F64) return PF_EINVAL;
    int rc = check_model(model);
    if (rc) return rc;
    size_t need = 0;
    pf_smooth_mh_workspace_bytes(N, B, S, &need);
    if (need > 0 && (!ws || ws_bytes < need)) return PF_EINVAL;
    if ((S - 1) * B > INT32_MAX) return PF_EUNSUPPORTED;  // (the cdf kernel's grid)
    const bool mat = model->hid_kind == PF_HID_LINEAR_MAT;
    const ModelDesc md = to_desc(model);
    const dim3 grid((unsigned)((N + PF_BLOCK - 1) / PF_BLOCK), (int)B);
    double* cdf = (double*)ws;
    int64_t* last_pos = (int64_t*)(cdf + (S - 1) * B * N);
    hipStream_t st = (hipStream_t)stream;
    return with_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        trace_launch(0, (int)sizeof(T), model->dim, 1, 0, 0, 0, PF_TRACE_SMOOTH_MH, 0, 0);
        if (S > 1) {
            hipLaunchKernelGGL((k_smooth_mh_cdf<T>), dim3((unsigned)((S - 1) * B)), dim3(PF_BLOCK), 0, st, (const T*)logw_hist, cdf, last_pos, N);
            PF_CHECK_LAUNCH();
        }
        auto launch = [&](auto d, auto m) {
            hipLaunchKernelGGL((k_smooth_mh<T, decltype(d)::value, decltype(m)::value>), grid, dim3(PF_BLOCK), 0, st, md, (const T*)model->params,
                               (const T*)x_hist, (const T*)logw_hist, anc_hist, idx_last, (const T*)u, seed, mcmc_steps, (const double*)cdf,
                               (const int64_t*)last_pos, (T*)out, idx_out, S, N, (int)B);
            return launch_status();
        };
        if (mat) return with_d8(model->dim, [&](auto d) { return launch(d, std::true_type{}); });
        return with_d3(model->dim, [&](auto d) { return launch(d, std::false_type{}); });
    });
}

// ---- test support ----------------------------------------------------------------------------------------------------
extern "C" int pf_debug_draw_normals(uint64_t seed, uint32_t step0, int64_t n_steps, void* out, int64_t N, int64_t B,
                                     int64_t D, int dtype, void* stream) {
    if (!out || bad_shape(N, B) || D < 1 || D > PF_MAXD || n_steps < 1 || n_steps > 65535) return PF_EINVAL;
    const Geom g = make_geom(N, B);
    const dim3 grid((unsigned)((N + g.round_elems - 1) / g.round_elems), (unsigned)B, (unsigned)n_steps);
    hipStream_t st = (hipStream_t)stream;
    return with_dtype(dtype, [&](auto t) {
        return with_vec(g.vec, [&](auto v) {
            return with_d3(D, [&](auto d) {
                using T = decltype(t);
                hipLaunchKernelGGL((k_debug_normals<T, decltype(d)::value, decltype(v)::value>), grid, dim3(PF_BLOCK), 0, st, seed, step0,
                                   (T*)out, N, (int)B);
                return launch_status();
            });
        });
    });
}

LaunchTrace& launch_trace() {
    static thread_local LaunchTrace t = {};
    return t;
}
extern "C" int pf_debug_launch_trace_fields(int32_t* out, int max_records, int fields) {
    if (!out || max_records < 0 || fields < 1 || fields > PF_TRACE_FIELDS) return PF_EINVAL;
    const LaunchTrace& t = launch_trace();
    const uint64_t have = t.count < PF_TRACE_LEN ? t.count : PF_TRACE_LEN;
    const int n = (uint64_t)max_records < have ? max_records : (int)have;
    for (int i = 0; i < n; ++i)  // oldest of the last n first
        for (int f = 0; f < fields; ++f) out[i * fields + f] = t.rec[(t.count - n + i) % PF_TRACE_LEN][f];
    return n;
}
// (the record the ABI has documented since its first version: ten fields - callers size their buffers by it)
extern "C" int pf_debug_launch_trace(int32_t* out, int max_records) { return pf_debug_launch_trace_fields(out, max_records, 10); }

extern "C" int pf_debug_leaf_residency(int proposal, int mk, int* blocks_per_cu, int* cus) {
    if (!blocks_per_cu || !cus) return PF_EINVAL;
    return leaf_residency(proposal, mk, blocks_per_cu, cus);
}

// theta: pf_filter_observe's theta update, which the cluster route folds into its launch (null: none)
static int filter_run_checked(const pf_filter_args* A, int64_t t0, int64_t n_steps, int finalize, void* stream,
                              float* kernel_ms, ThetaFold* theta);

extern "C" int pf_filter_run(const pf_filter_args* A, int64_t t0, int64_t n_steps, int finalize, void* stream) {
    return filter_run_checked(A, t0, n_steps, finalize, stream, nullptr, nullptr);
}

extern "C" int pf_filter_observe(const pf_filter_args* A, int64_t t0, int64_t n_steps, int finalize, void* w, const void* ll, void* stats,
                                 void* host_slot, uint64_t seq, void* acc, void* stream) {
    if (!A || !w || !ll || !stats || ((uintptr_t)host_slot & 7) != 0) return PF_EINVAL;
    ThetaFold tf{w, ll, stats, host_slot, seq, acc, 0};
    const int rc = filter_run_checked(A, t0, n_steps, finalize, stream, nullptr, &tf);
    if (rc != PF_OK) return rc;
    if (tf.folded) return PF_OK;  // (the column-cluster launch did the update itself)
    return pf_theta_step(w, ll, A->B, A->dtype, stats, host_slot, seq, acc, A->status, stream);
}

extern "C" int pf_filter_run_timed(const pf_filter_args* A, int64_t t0, int64_t n_steps, int finalize, void* stream,
                                   float* kernel_ms) {
    if (!kernel_ms) return PF_EINVAL;
    return filter_run_checked(A, t0, n_steps, finalize, stream, kernel_ms, nullptr);
}

// ---- hipGraph variant: the whole launch sequence of a run captured once, replayed with one host call -----------------
struct PfGraph {
    hipGraph_t graph;
    hipGraphExec_t exec;
};

extern "C" int pf_filter_graph_create(const pf_filter_args* A, int64_t t0, int64_t n_steps, int finalize, void* stream,
                                      void** handle) {
    if (!handle) return PF_EINVAL;
    *handle = nullptr;
    (void)stream;
    // capture on a private stream (the caller's may be the legacy default stream, which cannot capture); the graph is
    // replayed on whatever stream pf_filter_graph_launch is given
    hipStream_t st = nullptr;
    hipError_t e = hipStreamCreateWithFlags(&st, hipStreamNonBlocking);
    if (e != hipSuccess) return (int)e;
    e = hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal);
    if (e != hipSuccess) {
        (void)hipStreamDestroy(st);
        return (int)e;
    }
    const int rc = filter_run_checked(A, t0, n_steps, finalize, (void*)st, nullptr, nullptr);
    hipGraph_t graph = nullptr;
    e = hipStreamEndCapture(st, &graph);
    (void)hipStreamDestroy(st);
    if (rc != PF_OK) {
        if (graph) (void)hipGraphDestroy(graph);
        return rc;
    }
    if (e != hipSuccess) return (int)e;
    hipGraphExec_t exec = nullptr;
    e = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
    if (e != hipSuccess) {
        (void)hipGraphDestroy(graph);
        return (int)e;
    }
    PfGraph* g = new PfGraph{graph, exec};
    *handle = g;
    return PF_OK;
}

extern "C" int pf_filter_graph_launch(void* handle, void* stream) {
    if (!handle) return PF_EINVAL;
    const hipError_t e = hipGraphLaunch(((PfGraph*)handle)->exec, (hipStream_t)stream);
    return e == hipSuccess ? PF_OK : (int)e;
}

extern "C" int pf_filter_graph_destroy(void* handle) {
    if (!handle) return PF_OK;
    PfGraph* g = (PfGraph*)handle;
    (void)hipGraphExecDestroy(g->exec);
    (void)hipGraphDestroy(g->graph);
    delete g;
    return PF_OK;
}

static int filter_run_checked(const pf_filter_args* A, int64_t t0, int64_t n_steps, int finalize, void* stream,
                              float* kernel_ms, ThetaFold* theta) {
    if (!A || A->struct_size != sizeof(pf_filter_args)) return PF_EINVAL;  // (another ABI version: include/pf_amd.h)
    if (A->hints.route < 0 || A->hints.route > PF_ROUTE_PER_STEP_GENERIC || A->hints.column_max_n < 0 || A->hints.tile_target < 0 ||
        A->hints.cluster_patience < -1 || A->hints.cluster_patience > (1 << 30) || A->hints.cluster_generation < 0)
        return PF_EINVAL;
    int rc = check_model(&A->model, true);
    if (rc) return rc;
    if (bad_shape(A->N, A->B) || t0 < 0 || n_steps < 0) return PF_EINVAL;
    if (A->ring < 0 || A->ring == 1) return PF_EINVAL;
    if (A->hints.prepare_next != 0) {  // (see pf_run_hints: what the last step would have to evaluate must be in the kernels' reach)
        if (A->filter != PF_FILTER_APF || finalize || n_steps < 1) return PF_EINVAL;
        if (A->model.hid_kind == PF_HID_USER_AFFINE && (A->proposal != PF_PROP_LGO || !A->user_scale_per_column)) return PF_EINVAL;
    }
    if (!A->x[0] || !A->logw[0] || (A->ring < 3 && (!A->x[1] || !A->logw[1])) || !A->anc || !A->cdf || !A->means || !A->vars ||
        !A->ll_steps || !A->ll_total || !A->ws)
        return PF_EINVAL;
    if (n_steps > 0 && (!A->y || (!A->observed && !A->observed_dev && n_steps > PF_AUTO_FLAGS))) return PF_EINVAL;
    if (A->y_rows != 1 && A->y_rows != A->B) return PF_EINVAL;
    if (A->proposal == PF_PROP_LGO && A->model.obs_kind != PF_OBS_LINEAR) return PF_EUNSUPPORTED;
    if (A->model.hid_kind == PF_HID_USER_AFFINE) {  // the planes describe ONE incoming state: one step per call, no history
        if (!A->user_loc || !A->user_scale) return PF_EINVAL;
        if (n_steps > 1 || A->ring >= 3) return PF_EUNSUPPORTED;
    }
    if (A->filter != PF_FILTER_SISR && A->filter != PF_FILTER_APF) return PF_EUNSUPPORTED;
    if (!A->pos) return PF_EINVAL;
    const Geom g = make_geom(A->N, A->B, A->hints.tile_target);
    const WsLayout wl = make_ws(g);
    if (A->ws_bytes < wl.total) return PF_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    if (!column_eligible(A, g, n_steps, finalize) && cluster_eligible(A, g, n_steps, finalize) && wl.clu_bytes != 0) {
        if (A->dtype != PF_F32 && A->dtype != PF_F64) return PF_EINVAL;
        rc = A->dtype == PF_F32 ? pf_run_cluster_f32(A, g, wl, t0, n_steps, st, kernel_ms, theta)
                                : pf_run_cluster_f64(A, g, wl, t0, n_steps, st, kernel_ms, theta);
        if (rc != PF_CLUSTER_INFEASIBLE) return rc;  // (else: no slot for one filter's workgroups / LDS refused - the per-step route)
    }
    if (column_eligible(A, g, n_steps, finalize)) {
        if (A->dtype == PF_F32) return pf_run_column_f32(A, g, wl, t0, n_steps, st, kernel_ms);
        if (A->dtype == PF_F64) return pf_run_column_f64(A, g, wl, t0, n_steps, st, kernel_ms);
        return PF_EINVAL;
    }
    return with_dtype(A->dtype, [&](auto t) {  // the per-step route's leaf (filter_run_impl's explicit instantiations)
        return with_d3(A->model.dim, [&](auto d) {
            return with_vec(g.vec, [&](auto v) {
                return with_bool(g.rounds_per_tile > 1, [&](auto multi) {
                    return filter_run_impl<decltype(t), decltype(d)::value, decltype(v)::value, decltype(multi)::value>(A, g, wl, t0, n_steps,
                                                                                                                  finalize, st, kernel_ms);
                });
            });
        });
    });
}
