// pf_step.hip - the per-step route of the fused runs (pf_fused.hpp: k_fused_reduce, k_fused_step per time step, k_fused_book):
// filter_run_impl and the explicit instantiations one object owns.  Two selection macros, both required:
//   -DPF_STEP_KERNELS=f32d1_v4 | f32d1_v1 | f32dn | f64   float scalar states at four / one particle(s) per lane, float D > 1
//                                                         states, double (the last two: both vector widths)
//   -DPF_STEP_MULTI=0 | 1                                 single-round / multi-round tiles (the MULTI template argument)
// -> pf_<PF_STEP_KERNELS>_m<PF_STEP_MULTI>.o
#include "pf_host.hpp"

#define PF_STEP_KERNELS_f32d1_v4 1
#define PF_STEP_KERNELS_f32d1_v1 2
#define PF_STEP_KERNELS_f32dn 3
#define PF_STEP_KERNELS_f64 4
#define PF_STEP_CAT2(a, b) a##b
#define PF_STEP_CAT(a, b) PF_STEP_CAT2(a, b)
#ifndef PF_STEP_KERNELS
#error "pf_step.hip: -DPF_STEP_KERNELS=f32d1_v4|f32d1_v1|f32dn|f64 is required"
#endif
#define PF_STEP_SET PF_STEP_CAT(PF_STEP_KERNELS_, PF_STEP_KERNELS)  // (any other name: an undefined macro, 0)
#if PF_STEP_SET < 1 || PF_STEP_SET > 4
#error "pf_step.hip: PF_STEP_KERNELS must be one of f32d1_v4, f32d1_v1, f32dn, f64"
#endif
#ifndef PF_STEP_MULTI
#error "pf_step.hip: -DPF_STEP_MULTI=0|1 is required"
#endif
#if PF_STEP_MULTI != 0 && PF_STEP_MULTI != 1
#error "pf_step.hip: PF_STEP_MULTI must be 0 or 1"
#endif

// Columns of fewer tiles than this keep their books inline (the column's last step workgroup, after its own work).  Since
// the bookkeepers are dispatched LAST (the grid's slowest axis is the tile index, see below) they cost nothing on the critical path and inline lost at every
// shape measured, single-tile columns included (1 024 x 8 192: 65.5 -> 59.1 us per step; 256 x 8 192 27.3 -> 22.1;
// profiles/r04c_step_kernel_book_inline_threshold_ab.txt): 1 = never.  (Round 2's rule was 8.)
#define PF_BOOK_INLINE_TILES 1
template <typename T, int D, int VEC, bool MULTI>
int filter_run_impl(const pf_filter_args* A, const Geom& g, const WsLayout& wl, int64_t t0, int64_t n_steps, int finalize,
                    hipStream_t st, float* kernel_ms) {
    FusedArgs<T> a = make_fused_args<T>(A, g, wl, t0);

    const dim3 grid_tiles(g.tiles, g.B), block(PF_BLOCK);
    // the step kernel: one workgroup per tile + one bookkeeper per column, dispatched after all step workgroups
    // (PF_BOOK_INLINE=0/1 overrides in the development build: 1 = the column's last step workgroup keeps the books)
    a.book_inline = g.tiles < PF_BOOK_INLINE_TILES ? 1 : 0;
#ifdef PF_DEVTOOLS
    if (const char* bi = getenv("PF_BOOK_INLINE")) a.book_inline = atoi(bi);  // (2: nobody keeps the books - timing experiments)
#endif
    // Grid (B, tiles + 1), x = the column: blocks are dispatched in linear order and a 2^20-particle step of the generic kernel
    // fills every resident slot of the chip (1 024 = 4 per CU: 33 KB of LDS, 97 - 128 VGPRs) - with the tile index slowest the
    // bookkeepers (y == tiles) come after ALL step workgroups and fill slots as they free up.  For ONE column that means: the
    // bookkeeper starts when the first step workgroup retires and runs on alone - which is why the one-column leaf is built for
    // 5 per CU (1 280 slots: PF_WAVES_LEAF, StepLds) and its bookkeeper starts with the step workgroups.  As block (tiles, b) of a (tiles + 1, B) grid
    // they sat between the columns, took slots first, and the last columns' step workgroups started 2 - 3 us late
    // (profiles/r04c_step_kernel_bookkeepers_last_ab.txt).  B = 1 is the same linear order either way.
    a.kmap = 0u;
    if (g.B == 1 && g.tiles >= 16 && (g.tiles & (g.tiles - 1)) == 0) {  // one column of 2^q tiles: an eighth of it per XCD
        unsigned q = 0;
        while ((1 << q) < g.tiles) ++q;
        a.kmap = 7u | ((q - 3u) << 8) | (3u << 16);
    }
    const dim3 grid(g.B, g.tiles + (a.book_inline ? 0 : 1));
    const ObsFlags<T> flags(A, wl, t0, n_steps);
    if (t0 == 0) {
        // fresh filter: no previous step to account for (column records + poison flags); the derived flags ride along
        const size_t words = (wl.off_ctr - wl.off_stat) / sizeof(uint32_t);  // (256-byte aligned regions)
        flags.launch_zero((uint32_t*)((char*)A->ws + wl.off_stat), words, flags.derive, n_steps, st);
    }
    // state history: slot pointers per launch (the kernels keep addressing "buffer step & 1 is read, the other written")
    const int64_t ring = A->ring >= 3 ? A->ring : 0;
    auto place = [&](int64_t t) {  // launch of step t: reads state t, writes state t + 1
        if (!ring) return;
        const int64_t rs = t % ring, wsl = (t + 1) % ring, bn = (int64_t)g.B * g.N;
        a.x[t & 1] = (T*)A->x[0] + rs * D * bn;
        a.x[(t + 1) & 1] = (T*)A->x[0] + wsl * D * bn;
        a.logw[t & 1] = (T*)A->logw[0] + rs * bn;
        a.logw[(t + 1) & 1] = (T*)A->logw[0] + wsl * bn;
        a.anc = A->anc + wsl * bn;
        a.anc_prev = A->anc + rs * bn;
    };
    place(t0);
    // partials of the incoming state (afterwards every step kernel leaves the partials of the state it wrote)
    a.step = (int)t0;
    a.obs_dev = flags.dev;
    if (flags.derive && t0 != 0) flags.launch_derive(n_steps, st);
    a.obs = n_steps > 0 ? flags.obs(t0) : 0;
    a.obs_next = 0;
    // (pf_run_hints.resume: the previous call on this argument block ended with a SISR step that left the partials and local
    // scans of exactly this state in the workspace - the pass is redundant)
    // (an APF leaves them when its last step ran with pf_run_hints.prepare_next: the caller's promise)
    const bool resumed = A->hints.resume != 0 && t0 > 0 && A->ring < 3;
    const bool prepare_next = A->hints.prepare_next != 0 && A->filter == PF_FILTER_APF && !finalize && n_steps > 0;
    if (!resumed) hipLaunchKernelGGL((k_fused_reduce<T, D, VEC>), grid_tiles, block, 0, st, a);

    // ancestor stage of the step kernel: 0 inverted grid (systematic), 1 multinomial, 2 systematic by search - float
    // grids beyond 2^22 positions, where the closed form is not exact (PF_FORCE_SEARCH=1 selects it for testing)
    const bool force_search = A->hints.ancestor_search != 0;
    const int mode = (A->resampler == PF_RESAMPLE_MULTINOMIAL)
                         ? 1
                         : ((sizeof(T) == 4 && (g.N > ((int64_t)1 << 22) || force_search)) ? 2 : 0);
    // steady-state specialisation of this launch (float only: the double kernels are the parity path): see SPEC
    auto spec_of = [&]() -> int {
        if (sizeof(T) != 4 || a.z_tape || a.obs != 1) return 0;
        if (a.md.hid_kind == PF_HID_USER_AFFINE && a.filter == PF_FILTER_APF) return 0;  // (its steady state is not instantiated)
        if (a.filter == PF_FILTER_APF) return a.obs_next == 1 ? 1 : 0;
        return 2;
    };
    auto launch_step_as = [&](auto prop_c, auto fast_c) {
        constexpr int PROP = decltype(prop_c)::value;
        constexpr bool FAST = decltype(fast_c)::value;
        auto go = [&](auto mode_c, auto spec_c) {
            constexpr int MODE = decltype(mode_c)::value;
            constexpr int SPEC = decltype(spec_c)::value;
            auto launch = [&](auto mk_c) {
                constexpr int MK = decltype(mk_c)::value;
                // The one-column leaf (OneColHeader): the APF steady state of ONE column of 2^q >= 16 single-round tiles on the
                // closed-form kernels, writing an interior state - every address such a launch needs travels ready made in a
                // packed header.  A normal tape, a state history (keep_state), flags the host does not know (SPEC), a batch, the
                // run's last step: the generic kernel, as under PF_ROUTE_PER_STEP_GENERIC.
                if constexpr (sizeof(T) == 4 && D == 1 && VEC == 4 && !MULTI && MODE == 0 && FAST && SPEC == 1 && (MK == 1 || MK == 2)) {
                    if (A->hints.route != PF_ROUTE_PER_STEP_GENERIC && g.B == 1 && a.kmap != 0u && g.N <= ((int64_t)1 << 22) &&
                        !a.z_tape && !ring && a.obs == 1 && a.obs_next == 1 && a.keep_state == 0 && !a.book_inline && a.debug_cut <= 0) {  // (< 0: stamps only, development build)
                        trace_launch((int)a.step, (int)sizeof(T), D, VEC, MODE, PROP, 1, SPEC, MK, 0, 1);
                        hipLaunchKernelGGL((k_fused_step<T, D, VEC, MODE, PROP, FAST, SPEC, MK, MULTI, true>), grid, block, 0, st,
                                           OneColLaunch<T>{make_onecol_header<T>(a), a});
                        return;
                    }
                }
                trace_launch((int)a.step, (int)sizeof(T), D, VEC, MODE, PROP, FAST ? 1 : 0, SPEC, MK, MULTI ? 1 : 0);
                hipLaunchKernelGGL((k_fused_step<T, D, VEC, MODE, PROP, FAST, SPEC, MK, MULTI>), grid, block, 0, st, a);
            };
            // model kinds folded at compile time for the stochastic-volatility built-in (float runs; for Lorenz-63 the
            // same specialisation measured no gain)
            if constexpr (!FAST) {  // user-defined affine process: the parent's (loc, scale) come from the caller's planes
                if (a.md.hid_kind == PF_HID_USER_AFFINE) {
                    // (one step per run: no next step, so the APF steady-state specialisation never applies - not instantiated)
                    if constexpr (SPEC != 1) launch(std::integral_constant<int, 3>{});
                    return;
                }
            }
            if constexpr (sizeof(T) == 4 && !FAST && D == 1) {
                if (a.md.hid_kind == PF_HID_VERHULST_EM && a.md.obs_kind == PF_OBS_SV) return launch(std::integral_constant<int, 1>{});
            }
            if constexpr (sizeof(T) == 4 && !FAST && D == 3) {  // Lorenz-63
                if (a.md.hid_kind == PF_HID_LORENZ63_EM && a.md.obs_kind == PF_OBS_LINEAR)
                    return launch(std::integral_constant<int, 4>{});
            }
            if constexpr (sizeof(T) == 4 && FAST && D == 1) {  // shape of the one-step mean of the closed-form models
                if (a.md.hid_kind == PF_HID_SINE_EM) return launch(std::integral_constant<int, 2>{});
                return launch(std::integral_constant<int, 1>{});
            }
            launch(std::integral_constant<int, 0>{});
        };
        auto with_mode = [&](auto mode_c) {
            if constexpr (sizeof(T) == 4) {
                const int sp = spec_of();
                if (sp == 1) return go(mode_c, std::integral_constant<int, 1>{});
                // (the SISR specialisation spills in the multinomial variant and in the closed-form kernels: measured
                // slower than the generic kernel there)
                if (sp == 2) return go(mode_c, std::integral_constant<int, 2>{});
            }
            go(mode_c, std::integral_constant<int, 0>{});
        };
        if (mode == 0) with_mode(std::integral_constant<int, 0>{});
        else if (mode == 1) with_mode(std::integral_constant<int, 1>{});
        else if constexpr (sizeof(T) == 4) go(std::integral_constant<int, 2>{}, std::integral_constant<int, 0>{});
    };
    auto launch_step = [&]() {
        // scalar closed-form models: the proposal is a run-time switch inside one lean kernel (FAST); everything else gets
        // the proposal as a template constant so that Bootstrap runs do not carry the optimal proposal's registers
        bool fast = false;
        if constexpr (D == 1)
            fast = a.md.obs_kind == PF_OBS_LINEAR && a.md.hid_kind != PF_HID_VERHULST_EM && a.md.hid_kind != PF_HID_USER_AFFINE;
        if (fast) {
            if constexpr (D == 1) {
                if (a.proposal == PF_PROP_BOOTSTRAP) launch_step_as(std::integral_constant<int, PF_PROP_BOOTSTRAP>{}, std::true_type{});
                else launch_step_as(std::integral_constant<int, PF_PROP_LGO>{}, std::true_type{});
            }
        } else if (a.proposal == PF_PROP_BOOTSTRAP) {
            launch_step_as(std::integral_constant<int, PF_PROP_BOOTSTRAP>{}, std::false_type{});
        } else {
            launch_step_as(std::integral_constant<int, PF_PROP_LGO>{}, std::false_type{});
        }
    };
    const KernelTimer timer(kernel_ms, st);  // (around the whole step loop)
    if (timer.failed) return timer.rc;
    for (int64_t s = 0; s < n_steps; ++s) {
        const int64_t t = t0 + s;
        a.step = (int)t;
        place(t);
        a.obs = flags.obs(t);
        a.obs_next = (s + 1 < n_steps) ? flags.obs(t + 1) : (prepare_next ? 1 : 0);
        // Which states are read by somebody other than the next launch: every recorded one (state history) and the last of this
        // call - the caller's latest state, the next piece's k_fused_reduce, an online move - whatever finalize, resume or
        // prepare_next say.  The step kernel skips the stores of an interior state's planes that would be overwritten unread.
        a.keep_state = (ring != 0 || s + 1 == n_steps) ? 1 : 0;
#ifdef PF_DEVTOOLS
        if (a.debug_cut > 0) a.keep_state = 1;  // (the stage cuts 2 / 4 / 5 write through lw_out / anc_col)
        // stage cuts on ONE launch (the last but one step) when PF_DEBUG_CUT_AT_END is set: the state entering it is
        // valid, so per-dispatch PMC rows of that launch profile the stages on real data.  The stamps (PF_DEBUG_CUT < 0) likewise: every
        // stamping launch overwrites the one before, and a run's LAST launch writes a kept state - it is never the one-column leaf
        static const bool cut_at_end = getenv("PF_DEBUG_CUT_AT_END") != nullptr;
        const int cut_all = a.debug_cut;
        if (cut_at_end && cut_all != 0 && s != n_steps - 2) a.debug_cut = 0;
#endif
        launch_step();
#ifdef PF_DEVTOOLS
        a.debug_cut = cut_all;
#endif
    }
    timer.stop();
    if (finalize) {
        a.step = (int)(t0 + n_steps);
        a.obs = a.obs_next = 0;
        a.finalize_only = 1;
        hipLaunchKernelGGL((k_fused_book<T, D>), dim3(1, g.B), block, 0, st, a);
    }
    // (one kernel per step: the in-sequence time of a step IS the step kernel's launch-to-launch duration)
    if (const int rc = timer.finish(n_steps)) return rc;
    return launch_status();
}

#if PF_STEP_SET == PF_STEP_KERNELS_f32d1_v4 && PF_STEP_MULTI == 0
// pf_debug_leaf_residency (pf_kernels.hip): what the runtime says about the one-column leaf's instantiations, which this object owns
int leaf_residency(int proposal, int mk, int* blocks_per_cu, int* cus) {
    if ((proposal != PF_PROP_BOOTSTRAP && proposal != PF_PROP_LGO) || (mk != 1 && mk != 2)) return PF_EINVAL;
    auto ask = [&](auto prop_c, auto mk_c) -> int {
        int dev = 0;
        if (const hipError_t e = hipGetDevice(&dev)) return (int)e;
        if (const hipError_t e = hipDeviceGetAttribute(cus, hipDeviceAttributeMultiprocessorCount, dev)) return (int)e;
        return (int)hipOccupancyMaxActiveBlocksPerMultiprocessor(
            blocks_per_cu, k_fused_step<float, 1, 4, 0, decltype(prop_c)::value, true, 1, decltype(mk_c)::value, false, true>, PF_BLOCK, 0);
    };
    auto with_mk = [&](auto prop_c) {
        return mk == 1 ? ask(prop_c, std::integral_constant<int, 1>{}) : ask(prop_c, std::integral_constant<int, 2>{});
    };
    return proposal == PF_PROP_BOOTSTRAP ? with_mk(std::integral_constant<int, PF_PROP_BOOTSTRAP>{})
                                         : with_mk(std::integral_constant<int, PF_PROP_LGO>{});
}
#endif

// explicit instantiations: the leaves this object owns
#define PF_LEAF_AT(T, D, VEC, MULTI) \
    template int filter_run_impl<T, D, VEC, MULTI>(const pf_filter_args*, const Geom&, const WsLayout&, int64_t, int64_t, int, hipStream_t, float*);
#define PF_LEAF(T, D, VEC) PF_LEAF_AT(T, D, VEC, PF_STEP_MULTI != 0)
#if PF_STEP_SET == PF_STEP_KERNELS_f32d1_v4
PF_LEAF(float, 1, 4)
#elif PF_STEP_SET == PF_STEP_KERNELS_f32d1_v1
PF_LEAF(float, 1, 1)
#elif PF_STEP_SET == PF_STEP_KERNELS_f32dn
PF_LEAF(float, 2, 4) PF_LEAF(float, 3, 4) PF_LEAF(float, 2, 1) PF_LEAF(float, 3, 1)
#else
PF_LEAF(double, 1, 4) PF_LEAF(double, 2, 4) PF_LEAF(double, 3, 4) PF_LEAF(double, 1, 1) PF_LEAF(double, 2, 1) PF_LEAF(double, 3, 1)
#endif
#undef PF_LEAF
#undef PF_LEAF_AT
