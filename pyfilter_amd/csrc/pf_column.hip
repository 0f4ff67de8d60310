// pf_column.hip - the column-persistent route of the fused runs (pf_column.hpp: k_fused_column, one workgroup per filter runs the whole
// time loop): column_run_impl and the route's entry of one arithmetic type.
// One selection macro, required: -DPF_COLUMN_BITS=32 | 64, the arithmetic type (float / double) -> pf_col_f32.o / pf_col_f64.o
#include "pf_host.hpp"

#ifndef PF_COLUMN_BITS
#error "pf_column.hip: -DPF_COLUMN_BITS=32|64 is required"
#endif
#if PF_COLUMN_BITS != 32 && PF_COLUMN_BITS != 64
#error "pf_column.hip: PF_COLUMN_BITS must be 32 or 64"
#endif

template <typename T, int D>
static int column_run_impl(const pf_filter_args* A, const Geom& g, const WsLayout& wl, int64_t t0, int64_t n_steps,
                           hipStream_t st, float* kernel_ms) {
    constexpr int VEC = PF_COLUMN_VEC;  // (four particles per lane whatever N: columns of N % 4 != 0 take the RAGGED instantiations)
    FusedArgs<T> a = make_fused_args<T>(A, g, wl, t0);
    const int nt = column_threads(A->N, VEC);
    const size_t lds = column_lds_bytes(A->N, D, sizeof(T), VEC);
    const ObsFlags<T> flags(A, wl, t0, n_steps);
    a.obs_dev = flags.dev;
    if (flags.derive) flags.launch_derive(n_steps, st);
    const KernelTimer timer(kernel_ms, st);
    if (timer.failed) return timer.rc;
    // the folded instantiations: float, four particles per lane - scalar states of the closed-form models and of Verhulst + SV,
    // Lorenz-63 on whole 4-vectors (any workgroup size: the 256- or the 1024-thread bound); PF_ROUTE_COLUMN_GENERIC keeps the
    // run-time kernel (tests compare the two)
    auto with_column_folded = [&](auto&& f) {
        if (A->hints.route == PF_ROUTE_COLUMN_GENERIC) return false;
        if constexpr (sizeof(T) == 4 && D == 1) return with_folded<PF_HID_LINEAR, PF_HID_SINE_EM, PF_HID_OU, PF_HID_VERHULST_EM>(A, f);
        if constexpr (sizeof(T) == 4 && D == 3) return A->N % VEC == 0 && with_folded<PF_HID_LORENZ63_EM>(A, f);
        return false;
    };
    for (int64_t done = 0; done < n_steps;) {
        const ColumnRun r = flags.piece(t0 + done, n_steps - done);
        a.step = r.t0;
        // k_fused_column with KIND / FILT / PROP folded (KIND = -1: the run-time kernel), at the 256- or the 1024-thread bound;
        // columns of N % 4 != 0 particles take the RAGGED instantiations (the folded Lorenz-63 set has none)
        // (a 512-thread bound would lift the scratch of the D > 1 kernels - but at > 128 VGPRs only ONE 8-wave workgroup fits
        // a CU instead of two: 1024 x 2048 measured 33 us per step against 21)
        auto launch = [&](auto user_c, auto kind_c, auto filt_c, auto prop_c) {
            constexpr int KIND = decltype(kind_c)::value;
            trace_launch(r.t0, (int)sizeof(T), D, VEC, A->resampler == PF_RESAMPLE_MULTINOMIAL ? 1 : 0, A->proposal, KIND >= 0 ? 1 : 0,
                         /*SPEC*/ 9, KIND >= 0 ? KIND : 0, 0);
            auto go = [&](auto tpb_c, auto rag_c) {
                hipLaunchKernelGGL((k_fused_column<T, D, VEC, decltype(tpb_c)::value, decltype(user_c)::value, KIND, decltype(filt_c)::value,
                                                   decltype(prop_c)::value, decltype(rag_c)::value>), dim3(g.B), dim3(nt), lds, st, a, r);
            };
            auto with_rag = [&](auto tpb_c) {
                if constexpr (KIND < 0 || D == 1) {
                    if (A->N % VEC != 0) return go(tpb_c, std::true_type{});
                }
                go(tpb_c, std::false_type{});
            };
            if (nt <= 256) with_rag(int_c<256>{});
            else with_rag(int_c<1024>{});
        };
        if (!with_column_folded([&](auto kind_c, auto filt_c, auto prop_c) { launch(std::false_type{}, kind_c, filt_c, prop_c); })) {
            if (A->model.hid_kind == PF_HID_USER_AFFINE) launch(std::true_type{}, int_c<-1>{}, int_c<-1>{}, int_c<-1>{});
            else launch(std::false_type{}, int_c<-1>{}, int_c<-1>{}, int_c<-1>{});
        }
        done += r.n_steps;
    }
    timer.stop();
    if (const int rc = timer.finish(n_steps)) return rc;  // (the run's one kernel, per time step)
    return launch_status();
}
// the route's entry of this object's arithmetic type
#if PF_COLUMN_BITS == 32
int pf_run_column_f32(const pf_filter_args* A, const Geom& g, const WsLayout& wl, int64_t t0, int64_t n_steps, hipStream_t st, float* kernel_ms) {
    return with_d3(A->model.dim, [&](auto d) { return column_run_impl<float, decltype(d)::value>(A, g, wl, t0, n_steps, st, kernel_ms); });
}
#else
int pf_run_column_f64(const pf_filter_args* A, const Geom& g, const WsLayout& wl, int64_t t0, int64_t n_steps, hipStream_t st, float* kernel_ms) {
    return with_d3(A->model.dim, [&](auto d) { return column_run_impl<double, decltype(d)::value>(A, g, wl, t0, n_steps, st, kernel_ms); });
}
#endif
