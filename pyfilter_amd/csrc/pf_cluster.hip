// pf_cluster.hip - the column-cluster route of the fused runs (pf_cluster.hpp: k_fused_cluster, ceil(N / 1024) workgroups per filter run
// the whole time loop): cluster_run_impl and the route's entry of one arithmetic type.
// One selection macro, required: -DPF_CLUSTER_BITS=32 | 64, the arithmetic type (float / double) -> pf_clu_f32.o / pf_clu_f64.o
#include "pf_host.hpp"

#ifndef PF_CLUSTER_BITS
#error "pf_cluster.hip: -DPF_CLUSTER_BITS=32|64 is required"
#endif
#if PF_CLUSTER_BITS != 32 && PF_CLUSTER_BITS != 64
#error "pf_cluster.hip: PF_CLUSTER_BITS must be 32 or 64"
#endif

// resident workgroups of `kernel` on the current device: CUs x min(occupancy query, 6) - the query can be one block per CU high
// near the SGPR-limited edges (MI355X_MICROARCH.md, "Residency and cooperative launch"); 6 is below every such edge
// (asked once per kernel, LDS size and device: an online move is one such run per observation, and the three queries cost as much
// host time as a launch)
template <typename K> static inline int cluster_slots(K kernel, size_t lds) {
    struct Seen { const void* k; size_t lds; int dev, slots; };
    static Seen seen[32];
    static std::atomic<int> n_seen{0};
    static std::mutex mu;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 0;
    const int have = n_seen.load(std::memory_order_acquire);
    for (int i = 0; i < have; ++i)
        if (seen[i].k == (const void*)kernel && seen[i].lds == lds && seen[i].dev == dev) return seen[i].slots;
    int cus = 0, per_cu = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, PFK_TPB, lds) != hipSuccess) return 0;
    if (per_cu > 6) per_cu = 6;
    std::lock_guard<std::mutex> lock(mu);
    const int at = n_seen.load(std::memory_order_relaxed);
    if (at < 32) {
        seen[at] = Seen{(const void*)kernel, lds, dev, cus * per_cu};
        n_seen.store(at + 1, std::memory_order_release);
    }
    return cus * per_cu;
}
template <typename T, int D>
static int cluster_run_impl(const pf_filter_args* A, const Geom& g, const WsLayout& wl, int64_t t0, int64_t n_steps,
                            hipStream_t st, float* kernel_ms, ThetaFold* theta) {
    constexpr int VEC = PFK_HOST_VEC;
    FusedArgs<T> a = make_fused_args<T>(A, g, wl, t0);
    const size_t lds = cluster_lds_bytes(D, sizeof(T));
    const ObsFlags<T> flags(A, wl, t0, n_steps);  // (derived by the launch that clears the first piece's records: k_zero_and_flags)
    a.obs_dev = flags.dev;
    // the caller numbers its launches (pf_run_hints.cluster_generation): tagged records, nothing to clear
    bool numbered = A->hints.cluster_generation != 0 && A->status != nullptr && n_steps <= 32 * PFC_OBS_WORDS;
    if (numbered) {
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(st, &cap) != hipSuccess || cap != hipStreamCaptureStatusNone) numbered = false;  // (a replay repeats the number)
        (void)hipGetLastError();
    }
    const int c = (int)((A->N + PFK_TPB * VEC - 1) / (PFK_TPB * VEC));
    const int nchunks = (int)((A->N + 64 * VEC - 1) / (64 * VEC));
    int rc = PF_OK;
    const KernelTimer timer(kernel_ms, st);
    if (timer.failed) return timer.rc;
    // the run on one instantiation of k_fused_cluster: KIND = -1 the run-time kernel, else the folded one
    auto run = [&](auto kernel, int kind) {
        // (nothing has been launched yet: PF_CLUSTER_INFEASIBLE sends the caller - filter_run_checked - to the per-step route)
        if (lds > 64 * 1024 && hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
            (void)hipGetLastError();
            rc = PF_CLUSTER_INFEASIBLE;
            return;
        }
        const int slots = cluster_slots(kernel, lds);
        int per_launch = slots / c;  // columns whose members are all resident at once
        if (per_launch >= 8) per_launch &= ~7;
        if (per_launch < 1) {
            rc = PF_CLUSTER_INFEASIBLE;
            return;
        }
        unsigned char* clu = (unsigned char*)A->ws + wl.off_clu;
        for (int64_t done = 0; done < n_steps;) {
            const ColumnRun r = flags.piece(t0 + done, n_steps - done);
            a.step = r.t0;
            // fresh tags for this piece: error word + every record of the batch (a kernel, not a memset node - see k_zero_words)
            // (only what this instantiation's records occupy: NG granule rows of 1 KB per column and parity, after the error word)
            const size_t ng = ((size_t)(5 + 2 * D) * (sizeof(T) / 4) + 2 + 2) / 3;
            size_t words = (256 + (size_t)2 * g.B * PF_CLUSTER_NG * 64 * 16) / sizeof(uint32_t);
            if (g.B <= per_launch) words = (256 + (size_t)2 * g.B * ng * 64 * 16) / sizeof(uint32_t);  // (one group: its block is compact)
            const bool with_flags = flags.derive && done == 0;
            if (with_flags || !numbered) flags.launch_zero((uint32_t*)clu, words, with_flags, n_steps, st);
            trace_launch(r.t0, (int)sizeof(T), D, VEC, 0, A->proposal, kind >= 0 ? 1 : 0, /*SPEC*/ 10, kind >= 0 ? kind : 0, c);
            for (int b0 = 0; b0 < g.B; b0 += per_launch) {
                ClusterRun cr;
                cr.b0 = b0;
                cr.nb = (g.B - b0 < per_launch) ? g.B - b0 : per_launch;
                cr.nbp = (cr.nb + 7) & ~7;
                cr.c = c;
                cr.nchunks = nchunks;
                // (numbered launches: the workspace's error word is never cleared - the caller's status word, which it clears itself, is both)
                cr.err = numbered ? A->status : (int*)clu;
                cr.status = numbered ? nullptr : A->status;
                cr.tag_base = numbered ? (unsigned)(A->hints.cluster_generation & 0xFFFFF) * 4096u : 0u;
                cr.patience = A->hints.cluster_patience != 0 ? A->hints.cluster_patience : PFK_SPIN_LIMIT;
                cr.spread = A->hints.route == PF_ROUTE_CLUSTER_SPREAD ? 1 : 0;
                cr.th = ClusterTheta{};
                if (theta != nullptr && g.B <= per_launch && done + r.n_steps == n_steps && done == 0) {
                    // (one launch carries the whole run and every column: its last column to finish does the theta update)
                    cr.th.enabled = 1;
                    cr.th.w = theta->w;
                    cr.th.ll = theta->ll;
                    cr.th.stats = theta->stats;
                    cr.th.slot = (double*)theta->slot;
                    cr.th.seq = (unsigned long long)theta->seq;
                    cr.th.acc = theta->acc;
                    cr.th.arrive = (unsigned*)clu + 16;
                    theta->folded = 1;
                }
                cr.rec = clu + 256 + (size_t)b0 * 2 * PF_CLUSTER_NG * 64 * 16;  // (this group's [2][nb][NG][64] block)
                hipLaunchKernelGGL(kernel, dim3((unsigned)(cr.nbp * c)), dim3(PFK_TPB), lds, st, a, r, cr);
            }
            done += r.n_steps;
        }
    };
    // float runs of the built-in scalar closed-form models take KIND / FILT / PROP folded (as on the column route)
    bool folded = false;
    if constexpr (sizeof(T) == 4 && D == 1)
        folded = with_folded<PF_HID_LINEAR, PF_HID_SINE_EM, PF_HID_OU>(A, [&](auto kind_c, auto filt_c, auto prop_c) {
            run(k_fused_cluster<T, D, VEC, decltype(kind_c)::value, decltype(filt_c)::value, decltype(prop_c)::value>, decltype(kind_c)::value);
        });
    if (!folded) run(k_fused_cluster<T, D, VEC, -1, -1, -1>, -1);
    if (rc != PF_OK) return rc;
    timer.stop();
    if ((rc = timer.finish(n_steps)) != PF_OK) return rc;
    return launch_status();
}
// the route's entry of this object's arithmetic type
#if PF_CLUSTER_BITS == 32
int pf_run_cluster_f32(const pf_filter_args* A, const Geom& g, const WsLayout& wl, int64_t t0, int64_t n_steps, hipStream_t st, float* kernel_ms,
                       ThetaFold* theta) {
    return with_d3(A->model.dim, [&](auto d) { return cluster_run_impl<float, decltype(d)::value>(A, g, wl, t0, n_steps, st, kernel_ms, theta); });
}
#else
int pf_run_cluster_f64(const pf_filter_args* A, const Geom& g, const WsLayout& wl, int64_t t0, int64_t n_steps, hipStream_t st, float* kernel_ms,
                       ThetaFold* theta) {
    return with_d3(A->model.dim, [&](auto d) { return cluster_run_impl<double, decltype(d)::value>(A, g, wl, t0, n_steps, st, kernel_ms, theta); });
}
#endif
