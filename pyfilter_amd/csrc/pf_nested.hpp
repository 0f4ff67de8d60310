// pf_nested.hpp - the nested proposal (pyfilter/filters/particle/proposals/nested.py:27-47, Naesseth et al. 2019) for the
// built-in model kinds of the stand-alone model kernels: per particle M candidates from the transition, each weighed with
// p(y | candidate); one of them is kept with probability proportional to that weight and the particle's importance weight is
// log mean_j p(y | candidate_j).  In the reference: a (M, N, B, [D]) sample, a log_prob, a softmax, a Categorical draw, a
// take_along_dim and an exp / mean / log - eight launches over M-fold tensors.  Here: one thread per particle, everything in
// registers, nothing M-fold in memory.
//
// M is a run-time value and there is NO per-thread array of candidates (an array indexed by a run-time M lives in scratch memory).
// The draws are counter-based, so the kernel walks them twice instead:
//   pass 1  running maximum and running sum of exp(lp_j - max)  (online log-sum-exp)          -> the weight
//   pass 2  the same z_j again (Philox regenerates them, a tape is re-read), the running sum of exp(lp_j - max) up to the
//           first j with cum_j > v * sum                                                      -> the kept candidate
// Both loops make all M trips in every lane (the trip count is wave-uniform, the pick a predicated select).
//
// Arithmetic: mean_scale / obs_logpdf / the ColConsts closed forms - exactly what k_sample_and_weight evaluates for Bootstrap,
// so M = 1 on the same z IS Bootstrap's sample_and_weight (the same bits wherever the weight is finite).
// Differences from the reference: the weight in the max-shifted form max + log(sum / M) - the reference's
// log(mean(exp(lp))) is -inf once every lp underflows exp() - and the pick by inverse CDF from ONE uniform per particle.
#pragma once

namespace pf {

// Philox streams of the nested proposal (pf_philox.hpp):
//   normals   (seed, PF_STREAM_NESTED_Z, step, (b N + i) M + j)   - candidate j of particle i of filter b
//   the pick  (seed, PF_STREAM_NESTED_PICK, step, b N + i)

// What a particle's M candidates share: the one-step mean and the transition scale of its parent.
template <typename T, int D> struct NestedParent {
    T loc[D], scale[D], inc;
    bool fast;

    __device__ __forceinline__ void init(const ModelDesc& md, const ColParams<T, D>& cp, const ColConsts<T, D>& cc, const T (&x)[D]) {
        fast = false;
        inc = (T)md.inc_scale;
        if constexpr (D == 1) {
            if (cc.fast) {  // (the scalar closed forms of sample_and_weight: loc1, the hoisted scale g)
                fast = true;
                loc[0] = cc.loc1(md, cp, x[0]);
                scale[0] = cc.g;
                inc = cc.inc;
                return;
            }
        }
        mean_scale<T, D>(md, cp, x, loc, scale);
    }
    // candidate c = loc + scale * (z * inc) and log p(y | c) with NaN / +inf -> -inf (the reference's nan_to_num(-inf, -inf):
    // a stochastic-volatility candidate <= 0 is no scale of a Normal)
    __device__ __forceinline__ T propose(const ModelDesc& md, const ColParams<T, D>& cp, const ColConsts<T, D>& cc, const T (&z)[D],
                                         T (&c)[D]) const {
#pragma unroll
        for (int d = 0; d < D; ++d) c[d] = loc[d] + scale[d] * (z[d] * inc);
        T lp;
        if constexpr (D == 1) {
            lp = fast ? cc.obs_lp(c[0]) : obs_logpdf<T, D>(md, cp, c);
        } else {
            lp = cc.lin_fast ? cc.obs_lp_lin(cp, c, false) : obs_logpdf<T, D>(md, cp, c);
        }
        return lp;
    }
};

template <typename T> __device__ __forceinline__ T nested_sanitise(T lp) {
    return (lp != lp || lp == T(INFINITY)) ? -T(INFINITY) : lp;
}

// The normals of ONE particle, candidate after candidate: the tape (M, D, B, N) - `plane` = B N - or Philox.  Candidate j's normal d
// is number n = ((b N + i) M + j) D + d of the stream, i.e. NormalDraw::draw at element (b N + i) M + j; a particle's numbers are
// consecutive, so one Philox call serves NPC of them in a row (4 in float, 2 in double) instead of one: the buffer is refilled
// when n crosses a multiple of NPC - for M D a multiple of NPC in every lane at once.
template <typename T, int D> struct NestedNormals {
    static constexpr int NPC = NormalCall<T>::NPC;
    const T* __restrict__ z;
    uint64_t seed, n;
    uint32_t step;
    int64_t plane, col;
    T buf[NPC];

    __device__ __forceinline__ void rewind(int M) {
        n = (uint64_t)col * (uint64_t)M * D;
        if (!z && (n % NPC) != 0) NormalCall<T>::call(seed, PF_STREAM_NESTED_Z, step, n / NPC, buf);
    }
    __device__ __forceinline__ void next(int j, T (&zv)[D]) {
        if (z) {
#pragma unroll
            for (int d = 0; d < D; ++d) zv[d] = z[((int64_t)j * D + d) * plane + col];
            return;
        }
#pragma unroll
        for (int d = 0; d < D; ++d) {
            const int q = (int)(n % NPC);
            if (q == 0) NormalCall<T>::call(seed, PF_STREAM_NESTED_Z, step, n / NPC, buf);
            T val = buf[0];
#pragma unroll
            for (int k = 1; k < NPC; ++k) val = (q == k) ? buf[k] : val;
            zv[d] = val;
            ++n;
        }
    }
};

template <typename T, int D>
__global__ __launch_bounds__(PF_BLOCK) void k_nested_sample_and_weight(ModelDesc md, const T* __restrict__ params, int M,
                                                                       const T* __restrict__ x, const T* __restrict__ y, int y_rows,
                                                                       const T* __restrict__ z, const T* __restrict__ v, uint64_t seed,
                                                                       uint32_t step, T* __restrict__ x_out, T* __restrict__ w_out,
                                                                       int32_t* __restrict__ pick_out, int64_t N, int B) {
    const int b = blockIdx.y;
    const int O = md.obs_dim;
    const int NP = PF_BUILTIN_ROW_LEN(D, O);
    ColParams<T, D> cp;
    cp.load(params + (int64_t)b * NP, O, y + (int64_t)(y_rows == 1 ? 0 : b) * O);
    ColConsts<T, D> cc;
    cc.prepare(md, cp);
    const int64_t plane = (int64_t)B * N;
    const T ninf = -T(INFINITY);
    for (int64_t i = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x; i < N; i += (int64_t)gridDim.x * PF_BLOCK) {
        const int64_t col = (int64_t)b * N + i;
        T xv[D];
#pragma unroll
        for (int d = 0; d < D; ++d) xv[d] = x[((int64_t)d * B + b) * N + i];
        NestedParent<T, D> par;
        par.init(md, cp, cc, xv);
        NestedNormals<T, D> draws;
        draws.z = z, draws.seed = seed, draws.step = step, draws.plane = plane, draws.col = col;

        // pass 1: online log-sum-exp of the M observation log-densities
        T mx = ninf, sum = T(0);
        draws.rewind(M);
        for (int j = 0; j < M; ++j) {
            T zv[D], c[D];
            draws.next(j, zv);
            const T lp = nested_sanitise(par.propose(md, cp, cc, zv, c));
            const T nm = lp > mx ? lp : mx;
            const T s = sum * pf_exp(mx - nm) + pf_exp(lp - nm);  // (NaN while nothing finite was seen: -inf - -inf)
            sum = nm > ninf ? s : T(0);
            mx = nm;
        }
        const bool dead = !(mx > ninf);  // every candidate invalid: weight -inf, a uniform pick (the reference's 1 / M fill)
        const T vv = v ? v[col] : uniform_draw<T>(seed, PF_STREAM_NESTED_PICK, step, (uint64_t)col);
        int jd = (int)((double)vv * (double)M);  // floor(v M), exact in double for either type's v
        jd = jd < M - 1 ? jd : M - 1;
        const T target = vv * sum, shift = dead ? T(0) : mx;

        // pass 2: the same draws; candidate j is the current choice while the running sum has not passed v * sum and it carries
        // weight - the first j with cum_j > v sum (or, should rounding leave cum_M <= v sum, the last one of positive weight)
        T keep[D], cum = T(0);
#pragma unroll
        for (int d = 0; d < D; ++d) keep[d] = T(0);
        int pick = 0;
        bool found = false;
        draws.rewind(M);
        for (int j = 0; j < M; ++j) {
            T zv[D], c[D];
            draws.next(j, zv);
            const T lp = nested_sanitise(par.propose(md, cp, cc, zv, c));
            const T e = pf_exp(lp - shift);
            cum += e;
            const bool take = dead ? (j == jd) : (!found && e > T(0));
#pragma unroll
            for (int d = 0; d < D; ++d) keep[d] = take ? c[d] : keep[d];
            pick = take ? j : pick;
            found = found || cum > target;
        }
#pragma unroll
        for (int d = 0; d < D; ++d) x_out[((int64_t)d * B + b) * N + i] = keep[d];
        w_out[col] = dead ? ninf : mx + pf_log(sum / (T)M);
        if (pick_out) pick_out[col] = pick;
    }
}

}  // namespace pf
