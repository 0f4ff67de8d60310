// pf_colwave.hpp - what the two persistent kernels share, once: k_fused_column (pf_column.hpp: one workgroup per filter) and
// k_fused_cluster (pf_cluster.hpp: several workgroups per filter) run the same filter step and differ in how a column's waves
// EXCHANGE their sums.  Helpers take values and register arrays and return values.  A helper belongs here only if every kernel
// compiles to the instructions it had with the code written out in place (tools/isa_identity.py).
#pragma once

namespace pf {

// Workgroup barrier for LDS exchanges ONLY: waits for this wave's outstanding LDS operations (lgkmcnt), not for its global
// ones.  __syncthreads() carries a workgroup-scope fence, i.e. an `s_waitcnt vmcnt(0)` - it would make every step wait for
// the result rows thread 0 has just stored (means / variances / log-likelihood: never read in this launch) and for the
// next step's observation that was requested a step ahead precisely so that nobody waits for it.  A single-wave workgroup
// needs no barrier at all (its LDS operations execute in order): a compiler fence.
__device__ __forceinline__ void pfc_barrier(int nw) {
    if (nw > 1) asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    else asm volatile("" ::: "memory");
}

// exclusive scan of one double per thread across a workgroup of `nw` waves (1 .. 16); a single wave never touches LDS
__device__ __forceinline__ double cb_scan_excl(double v, double* red, int nw, double& total) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const double incl = wave_scan_incl(v, lane);
    if (nw == 1) {
        total = lane_get(incl, 63);
        return incl - v;
    }
    pfc_barrier(nw);
    if (lane == 63) red[wid] = incl;
    pfc_barrier(nw);
    double off = 0.0, tot = 0.0;
    for (int w = 0; w < nw; ++w) {
        const double s = red[w];
        if (w < wid) off += s;
        tot += s;
    }
    total = tot;
    return off + incl - v;
}

// log of a column sum / reciprocal of one, at the precision the filter's type needs: float filters take the hardware
// log2 / rcp (their results are rounded to float anyway), double filters the exact forms (the parity path)
template <typename T> __device__ __forceinline__ double log_sum(double s) {
    if constexpr (sizeof(T) == 4) return (double)pf_log_g((float)s);
    else return log(s);
}
template <typename T> __device__ __forceinline__ double inv_sum(double s) {
    if constexpr (sizeof(T) == 4) {
        double r = (double)__builtin_amdgcn_rcpf((float)s);
        r = __builtin_fma(__builtin_fma(-s, r, 1.0), r, r);  // one Newton step: ~2^-46
        return r;
    } else {
        return 1.0 / s;
    }
}

// KIND >= 0 (the host selects these instantiations for exactly such runs): the model's kinds as compile-time constants - scalar
// states on a linear-Gaussian observation, Verhulst on the stochastic-volatility built-in, Lorenz-63 - and, once the column's
// constants are prepared, what that says about them
template <int KIND, int D> __device__ __forceinline__ void fold_model_kind(ModelDesc& md) {
    if constexpr (KIND >= 0) {
        static_assert((D == 1) == (KIND != PF_HID_LORENZ63_EM), "specialised persistent kernels: built-in models");
        md.hid_kind = KIND;
        md.obs_kind = (KIND == PF_HID_VERHULST_EM) ? PF_OBS_SV : PF_OBS_LINEAR;
        if constexpr (D == 1) md.obs_dim = 1;
    }
}
template <int KIND, typename T, int D> __device__ __forceinline__ void assume_folded_kind(const ColConsts<T, D>& cc) {
    if constexpr (KIND >= 0) __builtin_assume(cc.fast == (D == 1 && KIND != PF_HID_VERHULST_EM));
}

// log-sum-exp over a wave's VEC sanitised values per lane (-inf: no contribution), as its parts: the wave's maximum mw and the
// sum s of exp(v - mw).  Off the common path: the log-likelihood terms of a column whose log-weights carry no information
// (`flat` in k_fused_column's loop has the account).
template <typename T, int VEC> __device__ __forceinline__ void wave_lse_parts(const T (&v)[VEC], T& mw, T& s) {
    T m = v[0];
#pragma unroll
    for (int j = 1; j < VEC; ++j) m = v[j] > m ? v[j] : m;
    mw = wave_max<T>(m);
    s = T(0);
#pragma unroll
    for (int j = 0; j < VEC; ++j) s += (v[j] == -Lim<T>::inf()) ? T(0) : pf_exp_w(v[j] - mw);
    s = wave_sum<T>(s);
}

}  // namespace pf
