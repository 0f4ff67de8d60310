// pf_host.hpp - the host side that more than one translation unit of libpfamd.so needs: tile geometry and workspace layout, the
// launch helpers, the launch trace, what the fused-run routes share (argument block, observed flags, timing window), which run
// takes which route, and the declarations of the route entries.  Includes the kernels' headers: whoever includes this file can
// launch any fused kernel.  The units: pf_kernels.hip (C ABI, stand-alone primitives, dispatch), pf_step.hip (per-step route),
// pf_column.hip, pf_cluster.hip (the persistent routes) - __graft_entry__.build_units says which object is which source.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <vector>

#include <type_traits>

#include "../../include/pf_amd.h"
#include "pf_device.hpp"
#include "pf_models.hpp"
#include "pf_philox.hpp"
#include "pf_linear.hpp"

namespace pf {

// ---------------------------------------------------------------------------------------------------------------
// geometry
// ---------------------------------------------------------------------------------------------------------------
#define PF_MAX_TILES 1024
#define PF_TARGET_WGS 1024
#define PF_AUTO_FLAGS 128  // steps whose observed flags pf_filter_run derives itself (workspace slot)

struct Geom {
    int64_t N;
    int B;
    int vec;            // 4 when N % 4 == 0 else 1
    int round_elems;    // 256 * vec
    int rounds_per_tile;
    int tile_elems;
    int tiles;          // per column
};

// `target`: workgroups per launch the tile size aims at (pf_run_hints.tile_target; 0 = PF_TARGET_WGS)
static inline Geom make_geom(int64_t N, int64_t B, int64_t target = 0) {
    Geom g;
    g.N = N;
    g.B = (int)B;
    g.vec = (N % 4 == 0) ? 4 : 1;
    g.round_elems = PF_BLOCK * g.vec;
    const int64_t rounds_total = (N + g.round_elems - 1) / g.round_elems;
    // Tile size: every workgroup pays a fixed price (column combine, constants, reductions), so tiles grow until the
    // grid is down to ~PF_TARGET_WGS workgroups (4 per CU) - but never more than PF_MAX_TILES tiles per column.
    int min_r = (g.vec == 4) ? 1 : 4;  // >= 1024-particle tiles
    if (target <= 0) target = PF_TARGET_WGS;
    int64_t r = (rounds_total * B) / target;
    if (r > rounds_total) r = rounds_total;
    const int64_t r_cap = (rounds_total + PF_MAX_TILES - 1) / PF_MAX_TILES;
    if (r < r_cap) r = r_cap;
    if (r < min_r) r = min_r;
    g.rounds_per_tile = (int)r;
    g.tile_elems = g.rounds_per_tile * g.round_elems;
    g.tiles = (int)((N + g.tile_elems - 1) / g.tile_elems);
    return g;
}

// per-column bookkeeping that survives between steps (lives in the workspace)
struct ColStat {
    double lse_w;      // log sum exp of the current log-weights
    double base_lse;   // ll_t = lse(logw'_t) - base_lse   (see DESIGN.md "log-likelihood bookkeeping")
    int resample;      // this step resamples this column
    int prev_observed; // the previous step was a weighted (observed) step
    int ll_done;       // the previous step's log-likelihood was already flushed by a finalize-only pass
    int flat_pending;  // (per-step route) the previous step was a SISR move that weighed on top of a column whose log-weights were
                       // all -inf / lowest: its increment is re-evaluated from the particles (column_bookkeeping)
};

// workspace carve-up (all offsets 256-byte aligned)
struct WsLayout {
    size_t off_part;   // double partials[2][(6 + 2 PF_MAXD)][B][tiles]
    size_t part_elems;
    size_t off_stat;   // ColStat[B]
    size_t off_poison; // int32 [4][B]
    size_t off_ctr;    // int32 [4] (reserved) | at +64: uint8 [PF_AUTO_FLAGS] observed flags derived on the device
    size_t off_dbg;    // uint64 [32]: development timestamps (clock64) of workgroup (0, 0)
    size_t off_cpack;  // T [B][PK_N] (sized for double): the run's closed-form records
    size_t off_piv0;   // double [B][PF_MAXD]: the run's moment pivots
    size_t off_ctab;   // double [2][B][tiles * rounds_per_tile * 4][2]: per-chunk (offset, factor) of the chunk-local scans
    size_t ctab_elems;
    size_t off_clu;    // cluster route (pf_cluster.hpp; columns of PF_CLUSTER_MIN_N < N <= PF_CLUSTER_MAX_N particles): int32 error
                       // word (256 B) | granule records [2][B][PF_CLUSTER_NG][64] x 16 B; absent (clu_bytes = 0) otherwise
    size_t clu_bytes;
    size_t off_tree;   // T [B][cdf_tree_total(N)]: the cdf sampled at every 16th, 256th, ... entry (the stand-alone multinomial's search tables)
    size_t total;
};

// pf_multinomial's search tables (the "cdf tree"): level l holds the LAST cdf entry of every block of 16^(l+1) entries (the column's last
// entry, 1, closes every level); levels are padded to 16 entries, the top one has at most 16.  N <= 2^30: at most 7 levels, N / 15
// entries in all.  Sizes and offsets are recomputed where they are used (a handful of scalar shifts): kept in per-thread arrays indexed
// by a run-time level they were promoted to LDS / scratch - 18 KB of LDS in k_scan.
__host__ __device__ static inline int cdf_tree_levels(int64_t N) {
    int levels = 0;
    int64_t n = N;
    do {
        n = (n + 15) >> 4;
        ++levels;
    } while (n > 16 && levels < 8);
    return levels;
}
__host__ __device__ static inline void cdf_tree_level(int64_t N, int l, int& size, int& off) {
    int64_t n = (N + 15) >> 4;
    int o = 0;
    for (int i = 0; i < l; ++i) {
        o += (int)((n + 15) & ~(int64_t)15);
        n = (n + 15) >> 4;
    }
    size = (int)n;
    off = o;
}
__host__ __device__ static inline int cdf_tree_total(int64_t N) {  // entries per column
    int size, off;
    cdf_tree_level(N, cdf_tree_levels(N) - 1, size, off);
    return off + ((size + 15) & ~15);
}

// the cluster route's column sizes: above what one workgroup holds (pf_column.hpp), at most 64 chunks of 256 particles
#define PF_CLUSTER_MIN_N 2048
#define PF_CLUSTER_MAX_N 16384
#define PF_CLUSTER_NG 8  // granules per chunk record, the largest instantiation (double, D = 3: 24 words)

static inline size_t align256(size_t v) { return (v + 255) & ~size_t(255); }

static inline WsLayout make_ws(const Geom& g) {  // (partials sized for PF_MAXD states)
    WsLayout w;
    size_t o = 0;
    w.off_part = o;  // two copies (the fused pipeline double-buffers them by state parity)
    w.part_elems = (size_t)(6 + 2 * PF_MAXD) * g.B * g.tiles;
    o = align256(o + 2 * sizeof(double) * w.part_elems);
    w.off_stat = o;
    o = align256(o + sizeof(ColStat) * (size_t)g.B);
    w.off_poison = o;
    o = align256(o + sizeof(int32_t) * 4 * (size_t)g.B);
    w.off_ctr = o;
    o = align256(o + 64 + PF_AUTO_FLAGS);
    w.off_dbg = o;
    o = align256(o + 256);
    w.off_cpack = o;
    o = align256(o + sizeof(double) * (size_t)g.B * 24);
    w.off_piv0 = o;
    o = align256(o + sizeof(double) * (size_t)g.B * PF_MAXD);
    w.off_ctab = o;
    w.ctab_elems = (size_t)g.B * g.tiles * g.rounds_per_tile * PF_NWAVES * 2;
    o = align256(o + 2 * sizeof(double) * w.ctab_elems);
    w.off_clu = o;
    // (16 KB per column - reserved only for batches the route can take in a handful of launches: <= 8 192 member workgroups)
    w.clu_bytes = (g.N > PF_CLUSTER_MIN_N && g.N <= PF_CLUSTER_MAX_N && g.N % 4 == 0 && ((g.N + 1023) / 1024) * (int64_t)g.B <= 8192)
                      ? 256 + (size_t)2 * g.B * PF_CLUSTER_NG * 64 * 16 : 0;
    o = align256(o + w.clu_bytes);
    w.off_tree = o;  // pf_multinomial: 16-ary search tables over the cdf (cdf_tree_*), sized for double
    o = align256(o + sizeof(double) * (size_t)g.B * cdf_tree_total(g.N));
    w.total = o;
    return w;
}

// Upper bound of make_ws(...).total over every tile geometry make_geom can produce for (N, B) (any `target`): the partials
// are largest with the most tiles per column (the smallest tiles), the chunk table never holds more than
// rounds_total + one tile's rounds per column.
static inline size_t ws_bound(int64_t N, int64_t B) {
    Geom g = make_geom(N, B, (int64_t)1 << 40);  // a huge target = the smallest tiles = the most tiles per column
    const int64_t rounds_total = (N + g.round_elems - 1) / g.round_elems;
    const size_t most_tiles = make_ws(g).total;
    g.tiles = 1;
    g.rounds_per_tile = (int)(2 * rounds_total + 2);  // tiles * rounds_per_tile <= rounds_total + rounds_per_tile <= 2 rounds_total
    const size_t most_chunks = make_ws(g).total;
    return most_tiles + most_chunks;
}

// partial slots
// E: sum of the tile's Exp(1) spacings (sorted-uniform multinomial); MX[d] at 6+d, MXX[d] at 6+D+d
enum { PQ_M1 = 0, PQ_S1 = 1, PQ_Q1 = 2, PQ_M2 = 3, PQ_S2 = 4, PQ_E = 5, PQ_MX = 6 };

}  // namespace pf

#include "pf_search.hpp"
#include "pf_fused.hpp"
#include "pf_colwave.hpp"
#include "pf_column.hpp"
#include "pf_cluster.hpp"

namespace pf {
// pf_filter_observe -> the route that carries the run: what the theta update needs (the cluster route folds it into its launch and
// says so; every other route leaves it to a pf_theta_step launch)
struct ThetaFold {
    void* w;
    const void* ll;
    void* stats;
    void* slot;
    uint64_t seq;
    void* acc;
    int folded;
};
}  // namespace pf

using namespace pf;

// PF_OK, or the error of the launches since the last check (hipGetLastError)
static inline int launch_status() {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? PF_OK : (int)e;
}
#define PF_CHECK_LAUNCH()                          \
    do {                                           \
        if (const int e_ = launch_status()) return e_; \
    } while (0)

// Run-time values as compile-time constants: each with_* calls the generic lambda `f` with a tag of the value and returns its result
template <int V> using int_c = std::integral_constant<int, V>;
// the C ABI's element type: f(float{}) or f(double{}); PF_EINVAL (nothing called) for any other dtype
template <typename F> static inline int with_dtype(int dtype, F&& f) {
    if (dtype == PF_F32) return f(float{});
    if (dtype == PF_F64) return f(double{});
    return PF_EINVAL;
}
// particles per lane of a tile geometry (Geom::vec): 4, else 1
template <typename F> static inline int with_vec(int vec, F&& f) { return vec == 4 ? f(int_c<4>{}) : f(int_c<1>{}); }
// the state dimension of the built-in models: 1, 2, else 3 (check_model bounds it)
template <typename F> static inline int with_d3(int64_t D, F&& f) {
    return D == 1 ? f(int_c<1>{}) : D == 2 ? f(int_c<2>{}) : f(int_c<3>{});
}
// ... of PF_HID_LINEAR_MAT: 1 .. 8 (PF_LIN_MAXD), PF_EUNSUPPORTED otherwise
template <typename F> static inline int with_d8(int64_t D, F&& f) {
    switch (D) {
        case 1: return f(int_c<1>{}); case 2: return f(int_c<2>{}); case 3: return f(int_c<3>{}); case 4: return f(int_c<4>{});
        case 5: return f(int_c<5>{}); case 6: return f(int_c<6>{}); case 7: return f(int_c<7>{}); case 8: return f(int_c<8>{});
        default: return PF_EUNSUPPORTED;
    }
}
template <typename F> static inline int with_bool(bool b, F&& f) { return b ? f(std::true_type{}) : f(std::false_type{}); }

static inline bool bad_shape(int64_t N, int64_t B) { return N < 1 || B < 1 || N > (int64_t)1 << 30 || B > 65535; }

// `fused`: the call is a fused filter run - the only place a user-defined affine process (whose mean / scale planes
// travel in pf_filter_args) can be evaluated; the stand-alone model kernels take built-in kinds only
static inline int check_model(const pf_model* m, bool fused = false) {
    if (!m || !m->params) return PF_EINVAL;
    if (m->hid_kind == PF_HID_USER_AFFINE && !fused) return PF_EUNSUPPORTED;
    if (m->hid_kind == PF_HID_LINEAR_MAT) {  // the stand-alone model kernels only (pf_linear.hpp): no fused / column route
        if (fused || m->dim < 1 || m->dim > PF_LIN_MAXD || m->obs_dim < 1 || m->obs_dim > PF_LIN_MAXO || m->obs_kind != PF_OBS_LINEAR)
            return PF_EUNSUPPORTED;
        return PF_OK;
    }
    if (m->dim < 1 || m->dim > PF_MAXD || m->obs_dim < 1 || m->obs_dim > PF_MAXO) return PF_EUNSUPPORTED;
    if (m->dim == 1 && m->obs_dim != 1) return PF_EUNSUPPORTED;
    if (m->hid_kind < 0 || m->hid_kind > PF_HID_USER_AFFINE) return PF_EUNSUPPORTED;
    if (m->hid_kind == PF_HID_LORENZ63_EM && m->dim != 3) return PF_EUNSUPPORTED;
    if (m->obs_kind != PF_OBS_LINEAR && m->obs_kind != PF_OBS_SV) return PF_EUNSUPPORTED;
    if (m->obs_kind == PF_OBS_SV && m->dim != 1) return PF_EUNSUPPORTED;
    return PF_OK;
}

static inline ModelDesc to_desc(const pf_model* m) {
    ModelDesc d;
    d.hid_kind = m->hid_kind;
    d.obs_kind = m->obs_kind;
    d.obs_dim = m->obs_dim;
    d.dt = m->dt;
    d.inc_scale = m->inc_scale;
    return d;
}

// Test support: which step-kernel instantiation each launch of the calling thread's most recent fused runs selected
// (pf_debug_launch_trace).  A per-thread ring, written on the host at launch time - nothing a kernel ever reads.
#define PF_TRACE_LEN 2048
#define PF_TRACE_FIELDS 11
struct LaunchTrace {
    int32_t rec[PF_TRACE_LEN][PF_TRACE_FIELDS];
    uint64_t count;
};
LaunchTrace& launch_trace();
// leaf: the launch took the one-column leaf of the step kernel (k_fused_step<..., ONECOL = true>) - the other fields say which one
static inline void trace_launch(int step, int tbytes, int d, int vec, int mode, int prop, int fast, int spec, int mk, int multi, int leaf = 0) {
    LaunchTrace& t = launch_trace();
    int32_t* r = t.rec[t.count % PF_TRACE_LEN];
    r[0] = step; r[1] = tbytes; r[2] = d; r[3] = vec; r[4] = mode; r[5] = prop; r[6] = fast; r[7] = spec; r[8] = mk; r[9] = multi;
    r[10] = leaf;
    ++t.count;
}
// The entry points besides pf_filter_run that leave a record, one per call (ops.TRACE_ENTRY names them).  Their codes occupy the
// record's SPEC field, so they must stay above every SPEC that a filter run writes (pf_step.hip: a step kernel's specialisation).
enum { PF_TRACE_FFBS_LINEAR = 20, PF_TRACE_SCORE_LINEAR = 21, PF_TRACE_SMOOTH_MH = 22 };

// the launch arguments every fused kernel shares, from the C ABI's argument block
template <typename T>
static FusedArgs<T> make_fused_args(const pf_filter_args* A, const Geom& g, const WsLayout& wl, int64_t t0) {
    FusedArgs<T> a;
    a.md = to_desc(&A->model);
    a.params = (const T*)A->model.params;
    a.filter = A->filter;
    a.proposal = A->proposal;
    a.resampler = A->resampler;
    a.g = g;
    a.thr_abs = A->ess_threshold * (double)A->N;
    a.logN = log((double)A->N);
    a.rcN = T(1) / T(A->N);
    a.seed = A->seed;
    a.seed_dev = (const uint64_t*)A->step_counter;
    a.x[0] = (T*)A->x[0];
    a.x[1] = (T*)A->x[1];
    a.logw[0] = (T*)A->logw[0];
    a.logw[1] = (T*)A->logw[1];
    a.anc = A->anc;
    a.anc_prev = nullptr;
    a.cdf = (T*)A->cdf;
    a.pos = (T*)A->pos;
    a.y = (const T*)A->y;
    a.y_rows = (int)A->y_rows;
    a.z_tape = (const T*)A->z_tape;
    a.u_tape = (const T*)A->u_tape;
    a.user_loc = (const T*)A->user_loc;
    a.user_scale = (const T*)A->user_scale;
    a.user_scale_percol = A->user_scale_per_column != 0 ? 1 : 0;
    a.user_dt = (T)A->user_dt;
    a.means = (T*)A->means;
    a.vars = (T*)A->vars;
    a.ll_steps = (T*)A->ll_steps;
    a.ll_total = (T*)A->ll_total;
    a.part = (double*)((char*)A->ws + wl.off_part);
    a.part_stride = (int64_t)wl.part_elems;
    a.stat = (ColStat*)((char*)A->ws + wl.off_stat);
    a.poison = (int32_t*)((char*)A->ws + wl.off_poison);
    a.dbg = (unsigned long long*)((char*)A->ws + wl.off_dbg);
    a.cpack = (T*)((char*)A->ws + wl.off_cpack);
    a.piv0 = (double*)((char*)A->ws + wl.off_piv0);
    a.ctab = (double*)((char*)A->ws + wl.off_ctab);
    a.ctab_stride = (int64_t)wl.ctab_elems;
    static_assert(PK_N == 24, "workspace layout reserves 24 slots per column record");
    a.finalize_only = 0;
    a.t0 = (int)t0;
    a.debug_cut = 0;
    a.keep_state = 1;  // (the per-step route sets it per launch: filter_run_impl)
#ifdef PF_DEVTOOLS  // (the instrumented build of tools/pmc_stages.py: stage cuts / cycle stamps selected per process)
    if (const char* dc = getenv("PF_DEBUG_CUT")) a.debug_cut = atoi(dc);
#endif
    return a;
}

// The one-column leaf's launch header (OneColHeader) for the launch `a` describes: B = 1, so a column offset is zero and a row
// of the partials is `tiles` long; every address is the one the generic kernel derives from the argument block for a.step
template <typename T>
static OneColHeader<T> make_onecol_header(const FusedArgs<T>& a) {
    OneColHeader<T> h;
    const int s = a.step;
    const int64_t stride = (int64_t)a.g.tiles;
    h.pm2 = a.part + (int64_t)(s & 1) * a.part_stride + PQ_M2 * stride;
    h.ps2 = a.part + (int64_t)(s & 1) * a.part_stride + PQ_S2 * stride;
    h.part_out = a.part + (int64_t)((s + 1) & 1) * a.part_stride;
    h.l_in = (s & 1) ? a.pos : a.cdf;
    h.l_out = (s & 1) ? a.cdf : a.pos;
    h.x_in = a.x[s & 1];
    h.x_out = a.x[(s & 1) ^ 1];
    h.seed_dev = a.seed_dev;
    h.seed = a.seed;
    h.cpack = a.cpack;
    h.y_t = a.y + (int64_t)s * a.y_rows;  // (scalar observations: check_model)
    h.piv_mean = (s - 1 >= a.t0) ? a.means + (s - 1) : nullptr;
    h.piv0 = a.piv0;
    h.u_t = a.u_tape ? a.u_tape + s : nullptr;
    h.poison_cur = a.poison + (s & 3);
    h.poison_next = a.poison + ((s + 1) & 3);
    h.N = (int)a.g.N;
    h.tiles = a.g.tiles;
    h.kmap = a.kmap;
    h.step = s;
    h.rcN = a.rcN;
    h.y_rows = a.y_rows;
    return h;
}

// A run's observed flags: the caller's host array (A->observed), the caller's device array (A->observed_dev), or - neither given -
// derived from y on the device into the workspace slot at off_ctr + 64 (runs of <= PF_AUTO_FLAGS steps); a run of ONE step on a
// shared observation row (the online move) has its kernels look at the row itself instead: no launch derives a flag byte
template <typename T>
struct ObsFlags {
    const uint8_t* host;  // A->observed
    const uint8_t* dev;   // the flags the kernels read on the device, indexed by the absolute step (null: host or inline)
    bool inline_y;        // the kernels read the flag off y (FusedArgs::obs = -2, ColumnRun::inline_y)
    bool derive;          // dev is the workspace slot: a launch of the route derives it (launch_derive / launch_zero)
    uint8_t* slot;
    int64_t row;          // elements of y per step
    const T* y;           // (derive) the run's first observation row

    ObsFlags(const pf_filter_args* A, const WsLayout& wl, int64_t t0, int64_t n_steps) {
        const bool none = !A->observed && !A->observed_dev && n_steps > 0;
        host = A->observed;
        inline_y = none && n_steps == 1 && A->y_rows == 1;
        derive = none && !inline_y;
        slot = (uint8_t*)A->ws + wl.off_ctr + 64;
        row = A->y_rows * (int64_t)A->model.obs_dim;
        y = derive ? (const T*)A->y + t0 * row : nullptr;
        dev = derive ? slot - t0 : A->observed_dev;
    }
    // FusedArgs::obs of step t
    int obs(int64_t t) const { return inline_y ? -2 : dev ? -1 : (host[t] != 0); }
    // the derivation in a launch of its own: one wave per step
    void launch_derive(int64_t n_steps, hipStream_t st) const {
        hipLaunchKernelGGL((k_observed_flags<T>), dim3((unsigned)n_steps), dim3(PF_WAVE), 0, st, y, row, slot);
    }
    // clears `words` words at p - with `flags`, the derivation rides along: one launch (a kernel, not hipMemsetAsync: captured as a
    // memset node the fill stopped clearing these records after ~195 replays of the same executable graph on ROCm 7.2 - every
    // log-likelihood of the run came back NaN, "poisoned" - tools/graph_replays.py)
    void launch_zero(uint32_t* p, size_t words, bool flags, int64_t n_steps, hipStream_t st) const {
        const unsigned zb = (unsigned)((words + PF_BLOCK - 1) / PF_BLOCK);
        if (flags)
            hipLaunchKernelGGL((k_zero_and_flags<T>), dim3(zb + (unsigned)n_steps), dim3(PF_BLOCK), 0, st, p, words, zb, y, row, slot);
        else
            hipLaunchKernelGGL((k_zero_words<uint32_t>), dim3(zb), dim3(PF_BLOCK), 0, st, p, words);
    }
    // a persistent launch's piece (pf_column.hpp, pf_cluster.hpp): up to 32 * PFC_OBS_WORDS steps from the absolute step t
    ColumnRun piece(int64_t t, int64_t left) const {
        ColumnRun r;
        r.t0 = (int)t;
        r.n_steps = (int)(left < 32 * PFC_OBS_WORDS ? left : 32 * PFC_OBS_WORDS);
        r.use_bits = (dev == nullptr && !inline_y) ? 1 : 0;
        r.inline_y = inline_y ? 1 : 0;
        for (int w = 0; w < PFC_OBS_WORDS; ++w) r.obs_bits[w] = 0u;
        if (r.use_bits)
            for (int q = 0; q < r.n_steps; ++q)
                if (host[r.t0 + q]) r.obs_bits[q >> 5] |= 1u << (q & 31);
        return r;
    }
};

// pf_filter_run_timed: HIP events on the caller's stream around a route's timed window (none without kernel_ms), released on every path
struct KernelTimer {
    float* kernel_ms;
    hipStream_t st;
    hipEvent_t ev[2] = {nullptr, nullptr};
    bool failed = false;  // hipEventCreate failed: the route returns rc
    int rc = PF_OK;
    KernelTimer(float* kernel_ms_, hipStream_t st_) : kernel_ms(kernel_ms_), st(st_) {
        if (!kernel_ms) return;
        for (auto& e : ev)
            if (hipEventCreate(&e) != hipSuccess) {
                failed = true;
                rc = (int)hipGetLastError();
                return;
            }
        (void)hipEventRecord(ev[0], st);
    }
    ~KernelTimer() {
        for (auto& e : ev)
            if (e) (void)hipEventDestroy(e);
    }
    void stop() const {
        if (kernel_ms) (void)hipEventRecord(ev[1], st);
    }
    // waits for the stream: kernel_ms[0] = kernel_ms[2] = the window per time step, kernel_ms[1] = 0 (the planning kernel of
    // earlier versions: folded into the step kernel's prologue)
    int finish(int64_t n_steps) const {
        if (!kernel_ms) return PF_OK;
        const hipError_t se = hipStreamSynchronize(st);
        if (se != hipSuccess) return (int)se;
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, ev[0], ev[1]);
        kernel_ms[0] = kernel_ms[2] = n_steps > 0 ? ms / (float)n_steps : 0.f;
        kernel_ms[1] = 0.f;
        return PF_OK;
    }
};

// The persistent routes' folded instantiations (pf_column.hpp / pf_cluster.hpp: KIND / FILT / PROP): a run on Philox normals of one
// of the model kinds KINDS calls f(kind, filter, proposal) - each a std::integral_constant - and returns true; any other run calls
// nothing and returns false.  A kind comes with its observations and proposals: the Verhulst process with stochastic-volatility
// observations and Bootstrap, every other kind with linear observations and Bootstrap or LGO.
template <int... KINDS, typename F>
static bool with_folded(const pf_filter_args* A, F&& f) {
    bool hit = false;
    auto with_kind = [&](auto kind_c) {
        constexpr bool SV = decltype(kind_c)::value == PF_HID_VERHULST_EM;
        if (hit || A->model.hid_kind != decltype(kind_c)::value || A->model.obs_kind != (SV ? PF_OBS_SV : PF_OBS_LINEAR)) return;
        if (A->proposal != PF_PROP_BOOTSTRAP && (SV || A->proposal != PF_PROP_LGO)) return;
        hit = true;
        auto with_prop = [&](auto filt_c) {
            if constexpr (!SV) {
                if (A->proposal == PF_PROP_LGO) return f(kind_c, filt_c, int_c<PF_PROP_LGO>{});
            }
            f(kind_c, filt_c, int_c<PF_PROP_BOOTSTRAP>{});
        };
        if (A->filter == PF_FILTER_APF) with_prop(int_c<PF_FILTER_APF>{});
        else with_prop(int_c<PF_FILTER_SISR>{});
    };
    if (!A->z_tape) (with_kind(int_c<KINDS>{}), ...);
    return hit;
}

// The per-step route of one arithmetic type / state dimension / vector width / tile geometry: defined in pf_step.hip, each of whose
// objects instantiates the leaves it owns (PF_STEP_KERNELS / PF_STEP_MULTI); pf_kernels.hip dispatches to them (filter_run_checked)
template <typename T, int D, int VEC, bool MULTI>
int filter_run_impl(const pf_filter_args* A, const Geom& g, const WsLayout& wl, int64_t t0, int64_t n_steps, int finalize,
                    hipStream_t st, float* kernel_ms);

// (test support, pf_debug_leaf_residency: resident workgroups per CU of the one-column leaf k_fused_step<float, 1, 4, 0, proposal, true,
// 1, mk, false, true> at PF_BLOCK threads and no dynamic LDS, and the device's CU count - defined by the object that owns the leaf)
int leaf_residency(int proposal, int mk, int* blocks_per_cu, int* cus);

// ---- the column-persistent route (pf_column.hpp): filters of a few hundred .. a few thousand particles -----------------
// One launch per run (per PFC_OBS_WORDS * 32 steps): no reduce / bookkeeping launches, no per-column records.
static inline int column_threads(int64_t N, int vec) {
    const int64_t need = (N + vec - 1) / vec;
    return (int)(((need + PF_WAVE - 1) / PF_WAVE) * PF_WAVE);
}
// Particles per lane on the column route: four - for scalar states also when N % 4 != 0 (the per-step geometry's
// one-particle lanes need four times the waves per filter, and past 256 of them the 1024-thread kernel: 1 000 x 333 ran
// 16.3 us per step against 5.4 for 1 000 x 400): the kernel handles the ragged last lane and the unaligned columns itself
// (pf_column.hpp: `ragged`).  D > 1 keeps the geometry's width.  The state's layout in HBM and the Philox addressing do not
// depend on it.  (One particle per lane for ALIGNED columns measured <= 16 % faster below 512 filters x 256 particles and
// up to 3x slower above: profiles/r03_column_vec1_vs_vec4.txt - not adopted.)
#define PF_COLUMN_VEC 4
static inline size_t column_lds_bytes(int64_t N, int D, size_t tsize, int vec) {
    int64_t np2 = 64;
    while (np2 < N) np2 <<= 1;
    const int64_t NP = ((N + vec - 1) / vec) * vec;  // (the kernel's padded plane stride)
    const size_t planes = (((size_t)(np2 + PF_LB_PAD + (int64_t)D * NP) * tsize) + 15) & ~(size_t)15;  // (cdf + the search's pad | particle planes)
    return planes + sizeof(double) * (2 + 2 * (4 + 2 * D)) * PFC_MAXW + 16;  // scan records + the state's records (x 2)
}
// (measured, profiles/r03_column_route.txt: 1024 x 2048 runs 21 us per step here against 29 on the per-step route, 1024 x
// 4096 56 against 42 - sixteen waves of one workgroup issue-bound on one CU)
#define PF_COLUMN_MAX_N 2048
// Which runs take it: self-contained runs (finalize: the last state's row is flushed by the same call), no state history,
// a column that fits one workgroup.  pf_run_hints.route = PF_ROUTE_PER_STEP keeps everything on the per-step route (tests compare the two).
static inline bool column_eligible(const pf_filter_args* A, const Geom& g, int64_t n_steps, int finalize) {
    if (!finalize || n_steps < 1 || A->ring >= 3) return false;
    if (A->hints.route == PF_ROUTE_PER_STEP || A->hints.route == PF_ROUTE_PER_STEP_GENERIC) return false;
    const int64_t max_n = A->hints.column_max_n > 0 ? A->hints.column_max_n : PF_COLUMN_MAX_N;
    if (A->N > max_n || column_threads(A->N, PF_COLUMN_VEC) > 1024) return false;
    return column_lds_bytes(A->N, A->model.dim, A->dtype == PF_F64 ? 8 : 4, PF_COLUMN_VEC) <= 64 * 1024;  // (the default dynamic-LDS limit)
}

// the route's entries, one per arithmetic type, each in the unit that compiles its kernels
int pf_run_column_f32(const pf_filter_args* A, const Geom& g, const WsLayout& wl, int64_t t0, int64_t n_steps, hipStream_t st, float* kernel_ms);
int pf_run_column_f64(const pf_filter_args* A, const Geom& g, const WsLayout& wl, int64_t t0, int64_t n_steps, hipStream_t st, float* kernel_ms);

// ---- the column-cluster route (pf_cluster.hpp): filters of 2 049 .. 16 384 particles, c workgroups per filter, one launch per
// run and group of columns -------------------------------------------------------------------------------------------------------
#define PFK_HOST_VEC 4  // particles per lane of the cluster kernels 
#define PF_CLUSTER_INFEASIBLE (-1000)  // internal: the cluster kernel cannot be launched here (no launch was issued)
static inline size_t cluster_lds_bytes(int D, size_t tsize) {
    return (size_t)(PFK_WIN_P2 + D * PFK_WIN) * tsize + 2 * PFK_FOLD * sizeof(double);  // window planes | the folds of two states
}
// Opt-in (pf_run_hints.route == PF_ROUTE_CLUSTER): the members of a column wait for each other - a launch that cannot make
// progress reports it through pf_filter_args.status instead of a result, and the caller re-issues the piece on the per-step
// route (include/pf_amd.h: PF_ROUTE_CLUSTER); the all-zero hints of the C ABI never take it.
static inline bool cluster_eligible(const pf_filter_args* A, const Geom& g, int64_t n_steps, int finalize) {
    if (A->hints.route != PF_ROUTE_CLUSTER && A->hints.route != PF_ROUTE_CLUSTER_ALWAYS && A->hints.route != PF_ROUTE_CLUSTER_SPREAD) return false;
    if (!finalize || n_steps < 1 || A->ring >= 3) return false;
    if (A->N <= PF_CLUSTER_MIN_N || A->N > PF_CLUSTER_MAX_N || A->N % PFK_HOST_VEC != 0) return false;
    if (A->resampler != PF_RESAMPLE_SYSTEMATIC || A->model.hid_kind == PF_HID_USER_AFFINE) return false;
    // Where it pays (same-box A/Bs, profiles/r05_cluster_route.txt): a launch holds ~1 024 resident member workgroups (2^20
    // particles) and larger batches run as consecutive launches of ~8.5 us per step each, while a per-step launch of 2^21+
    // particles costs 33 us and grows by 3 us per 2^20 more - two launches' worth is the break-even
    const int64_t members = ((A->N + PFK_TPB * PFK_HOST_VEC - 1) / (PFK_TPB * PFK_HOST_VEC)) * A->B;
    if (A->hints.route == PF_ROUTE_CLUSTER && members > 2 * 1024) return false;
    (void)g;
    return true;
}
int pf_run_cluster_f32(const pf_filter_args* A, const Geom& g, const WsLayout& wl, int64_t t0, int64_t n_steps, hipStream_t st, float* kernel_ms,
                       ThetaFold* theta);
int pf_run_cluster_f64(const pf_filter_args* A, const Geom& g, const WsLayout& wl, int64_t t0, int64_t n_steps, hipStream_t st, float* kernel_ms,
                       ThetaFold* theta);
