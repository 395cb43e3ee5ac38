/*
 * hhmm_scan.h -- the parallel scan over T of the forward-backward recursion
 * (SURVEY §8 A16): scan_prod_kernel, scan_bound_kernel, seg_summary_kernel and
 * fb_scan_kernel, which runs fb_sweep (hhmm_fb.h) over one T-chunk.
 */
#pragma once
#include "hhmm_fb.h"

namespace hhmm {

/* ------------------------------------------------------------------ */
/* Parallel scan over T                                  */
/* ------------------------------------------------------------------ */
/*
 * For long series with few pairs (C5: Tayal, T = 1e6).  The forward filter is
 * linear: f_t = f_{t-1} F_t with F_t(i,j) = Abar_t(i,j) e_t(j), Abar = A with
 * the columns the forward mask switches off set to 1; the backward pass is
 * beta_{t-1} = B_t beta_t with B_t(j,i) = Abar'_t(j,i) e_t(i), Abar' = A with
 * the ROWS the backward mask switches off set to 1 (Tayal, Q6; the other
 * programs' backward passes are unmasked, Q7).  All entries are
 * non-negative, so chunk products keep every entry's relative precision (no
 * cancellation), like the sequential recursion.
 *   phase 1  lane = (pair, T-chunk c): Pf_c = prod_{t in c} F_t and
 *            Qb_c = prod_{t in c} B_t (chunk 0 starts from the model's init f_0,
 *            so its row 0 is f at the chunk's end)
 *   phase 2  lane = pair: f entering every chunk (a left scan over Pf), beta
 *            at every chunk's last step (a right scan over Qb), loglik
 *   phase 3  lane = (pair, T-chunk): fb_sweep over the chunk from those vectors
 * Each product is renormalised by an exact power of two after every step;
 * the exponents and the Gaussian log-scale sum of the chunk travel with it.
 */

/* Whole-matrix power-of-two renormalisation (max entry into [0.5, 1)). */
template <int K>
__device__ __forceinline__ void renorm_mat(double (&M)[K][K], int &ex)
{
    double mx = M[0][0];
#pragma unroll
    for (int i = 0; i < K; ++i)
#pragma unroll
        for (int j = 0; j < K; ++j)
            mx = fmax(mx, M[i][j]);
    const int e = __builtin_amdgcn_frexp_exp(mx);
#pragma unroll
    for (int i = 0; i < K; ++i)
#pragma unroll
        for (int j = 0; j < K; ++j)
            M[i][j] = ldexp(M[i][j], -e);
    ex += e;
}

/* q <- q B_t for a row vector q: q'(i) = e(i) sum_j q(j) Abar'(j,i), with the
 * model's BACKWARD mask (hhmm-tayal2009.stan:109-111: the predicate on the
 * previous state j; unmasked otherwise). */
template <int MODEL, int K, int SG = -1>
__device__ __forceinline__ void bwd_row_raw(double (&q)[K], const PairParams<MODEL, K> &pp, const double (&e)[K],
                                            const Obs &o)
{
    if constexpr (SG > 0 && ModelTraits<MODEL>::kTayal) {
        /* the sign class is known: the off rows' terms (0 x A, + 0) dropped,
         * the rest in the same order -- the same bits */
        double qoff = 0.0;
#pragma unroll
        for (int j = 0; j < K; ++j)
            if (!tayal_on(SG, j))
                qoff += q[j];
        double s[K];
#pragma unroll
        for (int i = 0; i < K; ++i) {
            double acc = 0.0;
            bool first = true;
#pragma unroll
            for (int j = 0; j < K; ++j) {
                if (tayal_on(SG, j) && tayal_nz(j, i)) {
                    acc = first ? q[j] * pp.A[j][i] : fma(q[j], pp.A[j][i], acc);
                    first = false;
                }
            }
            s[i] = acc + qoff;
        }
#pragma unroll
        for (int i = 0; i < K; ++i)
            q[i] = s[i] * e[i];
        return;
    }
    double qon[K];
    double qoff = 0.0;
#pragma unroll
    for (int j = 0; j < K; ++j) {
        bool on = true;
        if constexpr (ModelTraits<MODEL>::kTayal)
            on = tayal_pred(o.aux, j);
        qon[j] = on ? q[j] : 0.0;
        qoff += on ? 0.0 : q[j];
    }
    double s[K];
#pragma unroll
    for (int i = 0; i < K; ++i) {
        double acc = qon[0] * pp.A[0][i];
#pragma unroll
        for (int j = 1; j < K; ++j)
            acc = fma(qon[j], pp.A[j][i], acc);
        s[i] = acc + qoff;
    }
#pragma unroll
    for (int i = 0; i < K; ++i)
        q[i] = s[i] * e[i];
}

/* Observation of step t (clamped, unconditional). */
template <int MODEL, bool AUX>
__device__ __forceinline__ Obs load_obs(const SeriesPtrs &sp, int t)
{
    Obs o[1];
    load_chunk<MODEL, 1, AUX>(o, sp, t);
    return o[0];
}

/* The chunk products in HBM, pair-major: chunk c of pair p is the K*K
 * record at sc_mat, its exponents / log scale the 3 doubles at sc_mxi. */
template <int K>
__device__ __forceinline__ int64_t sc_mat(const DevArgs &a, int64_t p, int c)
{
    return (p * a.scan_nc + c) * (int64_t)(K * K);
}
__device__ __forceinline__ int64_t sc_mxi(const DevArgs &a, int64_t p, int c, int f)
{
    return (p * a.scan_nc + c) * 3 + f;
}

template <int MODEL, int K, bool BWD>
__global__ void __launch_bounds__(kBlock) scan_prod_kernel(const DevArgs a)
{
    constexpr bool AUX = ModelTraits<MODEL>::kAux;
    constexpr int KP = (K + 1) / 2;
    HIP_DYNAMIC_SHARED(double2, lds)
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int64_t G = a.P * (int64_t)a.scan_nc;
    const int64_t g = min((int64_t)blockIdx.x * blockDim.x + threadIdx.x, G - 1);
    const int64_t p = g % a.P;
    const int c = (int)(g / a.P);
    int64_t n, d;
    pair_coords(a, p, n, d);
    const int Tp = pair_len(a, n);
    const int t0 = c * a.scan_cl;
    const int t1 = min(t0 + a.scan_cl, Tp);
    PairParams<MODEL, K> pp;
    load_params<MODEL, K, false>(pp, a, d);
    const double2 *slab = lds + (size_t)wave * a.L * KP * 64 + lane;
    if constexpr (ModelTraits<MODEL>::kDiscrete)
        pp.skip_ok &= fill_table<K, false>(lds + (size_t)wave * a.L * KP * 64 + lane, a, d);
    const SeriesPtrs sp = series_ptrs<MODEL, AUX>(a, n);

    double F[K][K], Q[K][K];
#pragma unroll
    for (int i = 0; i < K; ++i)
#pragma unroll
        for (int j = 0; j < K; ++j) {
            F[i][j] = (i == j) ? 1.0 : 0.0;
            Q[i][j] = F[i][j];
        }
    int fex = 0, qex = 0;
    double lsc = 0.0;
    int tb = t0;
    if (c == 0 && !a.seg_nofirst) { /* chunk 0 enters from the model's init vector f_0 (every row) */
        const Obs o0 = load_obs<MODEL, AUX>(sp, 0);
        Em<K> em;
        emit_prob<MODEL, K>(pp, slab, a.L, o0, em);
        double f0[K];
        fwd_init<MODEL, K>(f0, pp, em, o0, lsc, fex);
#pragma unroll
        for (int i = 0; i < K; ++i)
#pragma unroll
            for (int j = 0; j < K; ++j)
                F[i][j] = f0[j];
        tb = 1;
    }
    auto prods = [&](auto sgc, const Obs &o, const Em<K> &em) {
        constexpr int SG = decltype(sgc)::value;
#pragma unroll
        for (int r = 0; r < K; ++r)
            fwd_step_raw<MODEL, K, SG>(F[r], F[r], pp, em.e, o);
        if constexpr (BWD) {
#pragma unroll
            for (int r = 0; r < K; ++r)
                bwd_row_raw<MODEL, K, SG>(Q[r], pp, em.e, o);
        }
    };
    auto step = [&](const Obs &o, bool rn) {
        Em<K> em;
        emit_prob<MODEL, K>(pp, slab, a.L, o, em);
        lsc += em.m;
        /* a wave whose lanes share the step's sign (one series under many
         * draws: C5) takes the masks as constants (round 4) */
        tayal_dispatch<MODEL>(o, pp.skip_ok, [&](auto sgc) { prods(sgc, o, em); });
        if (rn) {
            renorm_mat<K>(F, fex);
            if constexpr (BWD)
                renorm_mat<K>(Q, qex);
        }
    };
    /* Discrete emissions renormalise the products every kBigRenorm-th step
     * (and every step of the chunk's ragged tail) where the pair's parameters
     * bound the shrink (renorm_sparse_safe, FB_BIG's argument: the max stays
     * above 2^-156 between renormalisations; a step grows it by at most K);
     * a wave holding an unsafe pair renormalises every step.  The exponents
     * are exact powers of two either way (round 4: a quarter of the
     * renormalisations, which were a sixth of the phase's VALU at C5). */
    bool sparse = false;
    if constexpr (ModelTraits<MODEL>::kDiscrete)
        sparse = !wave_any(!renorm_sparse_safe<MODEL, K>(pp, slab, a.L));
    Obs onx = load_obs<MODEL, AUX>(sp, tb);
    int t = tb;
    if (sparse) {
        constexpr int G = kBigRenorm;
        Obs og[G];
#pragma unroll
        for (int u = 0; u < G; ++u)
            og[u] = load_obs<MODEL, AUX>(sp, tb + u);
        for (; t + G <= t1; t += G) {
            Obs on[G];
#pragma unroll
            for (int u = 0; u < G; ++u)
                on[u] = load_obs<MODEL, AUX>(sp, t + G + u);
#pragma unroll
            for (int u = 0; u < G; ++u)
                step(og[u], u == G - 1);
#pragma unroll
            for (int u = 0; u < G; ++u)
                og[u] = on[u];
        }
        onx = og[0];
    }
    for (; t < t1; ++t) {
        const Obs o = onx;
        onx = load_obs<MODEL, AUX>(sp, t + 1);
        step(o, true);
    }
    /* pair-major records (sc_mat / sc_mxi): a lane writes whole lines, and
     * the boundary scan's lanes (consecutive chunks of one pair) read
     * consecutive lines */
    double *mf = a.sc_mf + sc_mat<K>(a, p, c);
#pragma unroll
    for (int i = 0; i < K; ++i)
#pragma unroll
        for (int j = 0; j < K; ++j) {
            mf[i * K + j] = F[i][j];
            if constexpr (BWD)
                a.sc_qb[sc_mat<K>(a, p, c) + i * K + j] = Q[i][j];
        }
    a.sc_mx[sc_mxi(a, p, c, 0)] = (double)fex;
    a.sc_mx[sc_mxi(a, p, c, 1)] = lsc;
    a.sc_mx[sc_mxi(a, p, c, 2)] = (double)qex;
}

template <int K>
__device__ __forceinline__ void load_mat(const double *base, const DevArgs &a, int c, int64_t p, double (&M)[K][K])
{
    const double *m = base + sc_mat<K>(a, p, c);
#pragma unroll
    for (int i = 0; i < K; ++i)
#pragma unroll
        for (int j = 0; j < K; ++j)
            M[i][j] = m[i * K + j];
}

/* Phase 2: one wave per pair scans its chunk products, 64 chunks per step of
 * the walk, lane-parallel.  Lane l holds chunk cb + l's product; a
 * Hillis-Steele prefix over the lanes (six levels of K x K products, the
 * partner's matrix by __shfl_up) gives every lane the product of the block's
 * chunks up to its own, and every lane applies it to the vector entering the
 * block, so the vectors entering all 64 chunks come out at once and are
 * stored by their own lanes.  The serial walk (one chunk per ~700 cycles of
 * dependent latency, lane 0 storing) took 2.4 ms at C5.
 * Products of the non-negative chunk matrices keep every entry's relative
 * precision; the partial products carry one exact power-of-two exponent PER
 * ROW (a row is the map from one entering state, and rows can drift apart by
 * more than the double range over a block), as lks_bound_kernel's exponents
 * do at large K.  The reassociated sums change the boundary vectors by a few
 * ulps against the serial walk, far inside the 1e-9 parity tolerance. */
constexpr int kNoExp = -(1 << 30);

template <int K>
struct RowMat {
    double m[K][K]; /* rows with max in [0.5, 1), or zero */
    int rs[K];      /* row i of the value is 2^rs[i] m[i] */
    double ls;      /* additive log scale (nats): the Gaussian emission shifts */
};

/* out 2^ex = f diag(2^rs) m (f any non-negative vector): the terms scaled to
 * the largest entering exponent, out renormalised into [0.5, 1). f == 0:
 * out = 0, ex unchanged. */
template <int K>
__device__ __forceinline__ void vec_rowmat(const double (&f)[K], const double (&m)[K][K], const int (&rs)[K],
                                           double (&out)[K], int &ex)
{
    int E = kNoExp;
#pragma unroll
    for (int i = 0; i < K; ++i)
        E = (f[i] != 0.0) ? max(E, __builtin_amdgcn_frexp_exp(f[i]) + rs[i]) : E;
    double g[K];
#pragma unroll
    for (int i = 0; i < K; ++i)
        g[i] = (f[i] != 0.0) ? ldexp(f[i], rs[i] - E) : 0.0;
#pragma unroll
    for (int j = 0; j < K; ++j) {
        double acc = g[0] * m[0][j];
#pragma unroll
        for (int i = 1; i < K; ++i)
            acc = fma(g[i], m[i][j], acc);
        out[j] = acc;
    }
    int e2 = 0;
    renorm<K>(out, e2);
    ex += (E == kNoExp) ? 0 : E + e2;
}

/* A chunk product as stored by scan_prod_kernel (one exponent for the whole
 * matrix; TR: transposed, the backward map applied to a row vector), fetched
 * a block ahead; `ident` (past the walk's end): the identity. */
template <int K>
struct RawMat {
    double m[K][K];
    double ex, ls;
};

template <int K, bool TR>
__device__ __forceinline__ void rawmat_fetch(const double *base, const DevArgs &a, int c, int64_t p, int xf,
                                             RawMat<K> &R)
{
    const double *m = base + sc_mat<K>(a, p, c);
#pragma unroll
    for (int i = 0; i < K; ++i)
#pragma unroll
        for (int j = 0; j < K; ++j)
            R.m[i][j] = m[(TR ? j : i) * K + (TR ? i : j)];
    R.ex = a.sc_mx[sc_mxi(a, p, c, xf)];
    R.ls = a.sc_mx[sc_mxi(a, p, c, 1)];
}

/* ... in the row-scaled form */
template <int K>
__device__ __forceinline__ void rowmat_from(const RawMat<K> &M, bool ident, RowMat<K> &R)
{
#pragma unroll
    for (int i = 0; i < K; ++i) {
        double mx = 0.0;
#pragma unroll
        for (int j = 0; j < K; ++j) {
            const double v = ident ? (i == j ? 1.0 : 0.0) : M.m[i][j];
            R.m[i][j] = v;
            mx = fmax(mx, v);
        }
        const int e = __builtin_amdgcn_frexp_exp(mx); /* 0 for a zero row */
#pragma unroll
        for (int j = 0; j < K; ++j)
            R.m[i][j] = ldexp(R.m[i][j], -e);
        R.rs[i] = ident ? e : e + (int)M.ex;
    }
    R.ls = ident ? 0.0 : M.ls;
}

/* R = X Y (X the earlier chunks). */
template <int K>
__device__ __forceinline__ void rowmat_mul(const RowMat<K> &X, const RowMat<K> &Y, RowMat<K> &R)
{
#pragma unroll
    for (int i = 0; i < K; ++i) {
        int e = 0;
        vec_rowmat<K>(X.m[i], Y.m, Y.rs, R.m[i], e);
        R.rs[i] = X.rs[i] + e;
    }
    R.ls = X.ls + Y.ls;
}

template <int K>
__device__ __forceinline__ void rowmat_shfl_up(const RowMat<K> &S, RowMat<K> &D, int d)
{
#pragma unroll
    for (int i = 0; i < K; ++i) {
#pragma unroll
        for (int j = 0; j < K; ++j)
            D.m[i][j] = __shfl_up(S.m[i][j], d);
        D.rs[i] = __shfl_up(S.rs[i], d);
    }
    D.ls = __shfl_up(S.ls, d);
}

/* Inclusive prefix product over the wave's lanes: P_l = M_0 M_1 ... M_l, for
 * the first nb lanes (wave-uniform; ceil(log2 nb) levels). */
template <int K>
__device__ __forceinline__ void rowmat_prefix(RowMat<K> &P, int lane, int nb = 64)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        if (d < nb) { /* wave-uniform; a guard, not a break, so the six levels unroll */
            RowMat<K> X, R;
            rowmat_shfl_up<K>(P, X, d);
            rowmat_mul<K>(X, P, R);
            if (lane >= d)
                P = R;
        }
    }
}

/* One block of the boundary walk: lane l holds the (row-scaled) map of the
 * block's chunk l (identity past the walk's end); v / vsc enter the block
 * (wave-uniform) and leave it after its last live chunk nb - 1.  Lane l
 * returns the vector leaving its chunk, normalised, and its log scale. */
template <int K>
__device__ __forceinline__ void bound_block(RowMat<K> &P, int lane, int nb, double (&v)[K], double &vsc,
                                            double (&out)[K], double &osc)
{
    rowmat_prefix<K>(P, lane, nb);
    int ex = 0;
    vec_rowmat<K>(v, P.m, P.rs, out, ex);
    osc = vsc + (P.ls + kLn2 * ex);
#pragma unroll
    for (int k = 0; k < K; ++k)
        v[k] = __shfl(out[k], nb - 1);
    vsc = __shfl(osc, nb - 1);
}

/* The boundary walk of one direction over items i = 0 .. n-1 (item i is chunk
 * c0 + i forward, chunk ncp-1-i backward), split over the workgroup's
 * kBoundWaves waves (round 4): each wave first multiplies its own range's
 * chunk products into one total (block prefixes, the block totals chained),
 * the totals meet in LDS, each wave forms the vector entering its range from
 * the ones before it, then walks its range storing every boundary vector --
 * twice the products of one wave walking everything, on four waves. */
#ifndef HHMM_BOUND_WAVES
#define HHMM_BOUND_WAVES 4 /* build knob: waves per (pair, direction) of the boundary scan */
#endif
constexpr int kBoundWaves = HHMM_BOUND_WAVES;
/* A walk of at most one block (n <= 64 items: C1's 16 chunks per pair) runs on
 * wave 0 alone, without the range totals: one prefix of ceil(log2 n) levels
 * instead of two six-level prefixes and a workgroup barrier on every wave
 * (C1 0.107 -> 0.121 ms with the four-wave scan).  Build knob. */
#ifndef HHMM_BOUND_SHORT
#define HHMM_BOUND_SHORT 1
#endif

/* ADJ (backward only): the maps are the FORWARD chunk products, beta_{t-1} =
 * F_t beta_t -- the adjoint of the forward pass, which the E-step sweeps
 * (hhmm_estep_scan.hip): sc_mf with its exponent, and no sc_qb at all. */
template <int K, bool BW, bool ADJ = false>
__device__ __forceinline__ void bound_walk(const DevArgs &a, int64_t p, int ncp, int c0, int n, double (&v)[K],
                                           double &vsc, RowMat<K> *tot)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool one = HHMM_BOUND_SHORT && n <= 64; /* workgroup-uniform */
    if (one && wave > 0)
        return;
    const int nw = one ? 1 : kBoundWaves;
    const int lo = (int)((int64_t)n * wave / nw), hi = (int)((int64_t)n * (wave + 1) / nw);
    const double *base = (BW && !ADJ) ? a.sc_qb : a.sc_mf;
    auto chunk = [&](int i) { return BW ? ncp - 1 - i : c0 + i; };
    auto fetch = [&](int ib, RawMat<K> &r) { /* item ib + lane, clamped into the range */
        rawmat_fetch<K, BW>(base, a, chunk(max(min(ib + lane, hi - 1), 0)), p, (BW && !ADJ) ? 2 : 0, r);
    };
    RawMat<K> nx;
    if (!one) {
    /* ---- 1. the range's total ---- */
    RowMat<K> T;
    {
        RawMat<K> id;
        rowmat_from<K>(id, true, T);
    }
    if (lo < hi)
        fetch(lo, nx);
    for (int ib = lo; ib < hi; ib += 64) {
        RowMat<K> P;
        rowmat_from<K>(nx, ib + lane >= hi, P);
        fetch(ib + 64, nx);
        rowmat_prefix<K>(P, lane, min(hi - ib, 64));
        RowMat<K> B, R;
        const int last = min(hi - ib, 64) - 1;
#pragma unroll
        for (int i = 0; i < K; ++i) {
#pragma unroll
            for (int j = 0; j < K; ++j)
                B.m[i][j] = __shfl(P.m[i][j], last);
            B.rs[i] = __shfl(P.rs[i], last);
        }
        B.ls = __shfl(P.ls, last);
        rowmat_mul<K>(T, B, R);
        T = R;
    }
    if (lane == 0)
        tot[wave] = T;
    __syncthreads();
    /* ---- 2. the vector entering this wave's range ---- */
    for (int w = 0; w < wave; ++w) {
        const RowMat<K> &U = tot[w];
        double o[K];
        int ex = 0;
        vec_rowmat<K>(v, U.m, U.rs, o, ex);
        vsc += U.ls + kLn2 * ex;
#pragma unroll
        for (int k = 0; k < K; ++k)
            v[k] = o[k];
    }
    }
    /* ---- 3. the walk, every boundary vector stored by its own lane ---- */
    if (lo < hi)
        fetch(lo, nx);
    for (int ib = lo; ib < hi; ib += 64) {
        const int i = ib + lane;
        RowMat<K> P;
        rowmat_from<K>(nx, i >= hi, P);
        fetch(ib + 64, nx);
        double out[K], osc;
        bound_block<K>(P, lane, min(hi - ib, 64), v, vsc, out, osc);
        const int c = chunk(i);
        if (!BW && i < hi && c + 1 < ncp) {
#pragma unroll
            for (int k = 0; k < K; ++k)
                a.sc_st[p + a.P * (int64_t)((c + 1) * K + k)] = out[k];
            a.sc_sl[p + a.P * (int64_t)(c + 1)] = osc;
        }
        if (BW && i < hi) {
#pragma unroll
            for (int k = 0; k < K; ++k)
                a.sc_be[p + a.P * (int64_t)((c - 1) * K + k)] = out[k];
            a.sc_bl[p + a.P * (int64_t)(c - 1)] = osc;
        }
    }
}

/* One workgroup of kBoundWaves waves per (pair, direction): blockIdx.y == 0
 * the forward walk (f entering chunks c0 .. ncp-1, the loglik), 1 the
 * backward walk (beta leaving chunks ncp-1 .. 0; chunk c's map applied to a
 * row vector is Q_c^T).  The two are independent.  ADJ: the backward walk takes
 * the forward products (bound_walk). */
template <int MODEL, int K, bool BWD, bool ADJ = false>
__global__ void __launch_bounds__(64 * kBoundWaves) scan_bound_kernel(const DevArgs a)
{
    __shared__ RowMat<K> tot[kBoundWaves];
    const int64_t p = blockIdx.x;
    const bool t0 = threadIdx.x == 0;
    int64_t n, d;
    pair_coords(a, p, n, d);
    const int Tp = pair_len(a, n);
    const int ncp = (Tp + a.scan_cl - 1) / a.scan_cl;
    auto mx = [&](int c, int f) { return a.sc_mx[sc_mxi(a, p, c, f)]; };

    if (blockIdx.y == 0) {
        double f[K];
        double sc;
        int c0;
        if (!a.seg_nofirst) {
            /* chunk 0's product has every row equal to the filter leaving it */
#pragma unroll
            for (int j = 0; j < K; ++j)
                f[j] = a.sc_mf[sc_mat<K>(a, p, 0) + j];
            sc = mx(0, 1) + kLn2 * mx(0, 0);
            c0 = 1;
        } else {
            /* a segment window: chunk 0 enters from the caller's state, which then
             * goes through chunk 0's product like every later chunk */
#pragma unroll
            for (int j = 0; j < K; ++j)
                f[j] = a.seg_enter[p + a.P * (int64_t)j];
            sc = a.seg_enter[p + a.P * (int64_t)K];
            c0 = 0;
        }
        if (t0 && c0 < ncp) {
#pragma unroll
            for (int k = 0; k < K; ++k)
                a.sc_st[p + a.P * (int64_t)(c0 * K + k)] = f[k];
            a.sc_sl[p + a.P * (int64_t)c0] = sc;
        }
        bound_walk<K, false>(a, p, ncp, c0, max(ncp - c0, 0), f, sc, tot);
        /* the last wave leaves with the filter after chunk ncp-1 (wave 0 alone
         * on a short walk; the others returned from it) */
        const int nlast = (HHMM_BOUND_SHORT && ncp - c0 <= 64) ? 0 : kBoundWaves - 1;
        if ((threadIdx.x == 64 * nlast) && (a.outputs & HHMM_OUT_LOGLIK) && a.loglik && !a.seg_nolast)
            a.loglik[p] = log(vsum<K>(f)) + sc;
        return;
    }

    if constexpr (BWD) {
        double b[K];
        /* beta at the last step: unbeta_tk[T] = 1 (Q1), or a segment window's
         * beta leaving it (the caller's) */
        double bsc = a.seg_nolast ? a.seg_leave[p + a.P * (int64_t)K] : 0.0;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            b[k] = a.seg_nolast ? a.seg_leave[p + a.P * (int64_t)k] : 1.0;
            if (t0)
                a.sc_be[p + a.P * (int64_t)((ncp - 1) * K + k)] = b[k];
        }
        if (t0)
            a.sc_bl[p + a.P * (int64_t)(ncp - 1)] = bsc;
        bound_walk<K, true, ADJ>(a, p, ncp, 0, max(ncp - 1, 0), b, bsc, tot);
    }
}

/* Segment summary (hhmm_segment): one lane per pair multiplies its window's
 * chunk products in order, SF = F_0 F_1 ... and SQ = Q_0 Q_1 ..., each
 * renormalised by an exact power of two after every product, the exponents
 * and the Gaussian log scales summed alongside (the K x K
 * summary a rank contributes to the all-gather). */
template <int K>
__device__ __forceinline__ void mat_mul_acc(double (&S)[K][K], const double (&M)[K][K])
{
    double R[K][K];
#pragma unroll
    for (int i = 0; i < K; ++i)
#pragma unroll
        for (int j = 0; j < K; ++j) {
            double acc = S[i][0] * M[0][j];
#pragma unroll
            for (int l = 1; l < K; ++l)
                acc = fma(S[i][l], M[l][j], acc);
            R[i][j] = acc;
        }
#pragma unroll
    for (int i = 0; i < K; ++i)
#pragma unroll
        for (int j = 0; j < K; ++j)
            S[i][j] = R[i][j];
}

template <int MODEL, int K, bool BWD>
__global__ void __launch_bounds__(kBlock) seg_summary_kernel(const DevArgs a)
{
    const int64_t p = min((int64_t)blockIdx.x * blockDim.x + threadIdx.x, a.P - 1);
    int64_t n, d;
    pair_coords(a, p, n, d);
    const int ncp = (pair_len(a, n) + a.scan_cl - 1) / a.scan_cl;
    double SF[K][K], SQ[K][K], M[K][K];
    load_mat<K>(a.sc_mf, a, 0, p, SF);
    if constexpr (BWD)
        load_mat<K>(a.sc_qb, a, 0, p, SQ);
    double fex = a.sc_mx[sc_mxi(a, p, 0, 0)], lsc = a.sc_mx[sc_mxi(a, p, 0, 1)], qex = a.sc_mx[sc_mxi(a, p, 0, 2)];
    for (int c = 1; c < ncp; ++c) {
        int e = 0;
        load_mat<K>(a.sc_mf, a, c, p, M);
        mat_mul_acc<K>(SF, M);
        renorm_mat<K>(SF, e);
        fex += a.sc_mx[sc_mxi(a, p, c, 0)] + e;
        lsc += a.sc_mx[sc_mxi(a, p, c, 1)];
        if constexpr (BWD) {
            e = 0;
            load_mat<K>(a.sc_qb, a, c, p, M);
            mat_mul_acc<K>(SQ, M);
            renorm_mat<K>(SQ, e);
            qex += a.sc_mx[sc_mxi(a, p, c, 2)] + e;
        }
    }
    if constexpr (!BWD) {
#pragma unroll
        for (int i = 0; i < K; ++i)
#pragma unroll
            for (int j = 0; j < K; ++j)
                SQ[i][j] = (i == j) ? 1.0 : 0.0;
    }
#pragma unroll
    for (int i = 0; i < K; ++i)
#pragma unroll
        for (int j = 0; j < K; ++j) {
            a.seg_sum[p + a.P * (int64_t)(i * K + j)] = SF[i][j];
            a.seg_sum[p + a.P * (int64_t)(K * K + i * K + j)] = SQ[i][j];
        }
    a.seg_sum[p + a.P * (int64_t)(2 * K * K + 0)] = fex;
    a.seg_sum[p + a.P * (int64_t)(2 * K * K + 1)] = lsc;
    a.seg_sum[p + a.P * (int64_t)(2 * K * K + 2)] = qex;
}

/* Phase 3: the forward-backward sweep of one (pair, T-chunk). */
template <int MODEL, int K, int MODE>
__global__ void __launch_bounds__(kBlock) fb_scan_kernel(const DevArgs a)
{
    constexpr bool AUX = ModelTraits<MODEL>::kAux;
    constexpr int KP = (K + 1) / 2;
    constexpr int C = fb_chunk(K);
    HIP_DYNAMIC_SHARED(double2, lds)
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    /* lane g = pp + Pp * c with Pp = P rounded up to whole waves: every wave
     * lies in ONE T-chunk, so the sweep's wave-uniform chunk bounds (and its
     * unconditional checkpoint prefetches) stay inside that chunk's rows.
     * Lanes pp >= P redo pair P-1 (identical values, benign duplicate stores). */
    const int64_t Pp = scan_lanes_per_chunk(a.P);
    const int64_t G = Pp * (int64_t)a.scan_nc;
    const int64_t g = min((int64_t)blockIdx.x * blockDim.x + threadIdx.x, G - 1);
    const int64_t p = min(g % Pp, a.P - 1);
    const int c = (int)(g / Pp);
    int64_t n, d;
    pair_coords(a, p, n, d);
    const int Tpair = pair_len(a, n);
    FbLane<MODEL, K> ln;
    ln.p = p;
    ln.L = a.L;
    ln.t0 = c * a.scan_cl;
    ln.Tp = max(min(ln.t0 + a.scan_cl, Tpair), ln.t0); /* chunks past the pair's end do nothing */
    ln.cb = ln.t0 / C;
    ln.q = g;
    ln.Qs = G;
    ln.slab = lds + (size_t)wave * a.L * KP * 64 + lane;
    load_params<MODEL, K, false>(ln.pp, a, d);
    if constexpr (ModelTraits<MODEL>::kDiscrete)
        ln.pp.skip_ok &= fill_table<K, false>(lds + (size_t)wave * a.L * KP * 64 + lane, a, d);
    const SeriesPtrs sp = series_ptrs<MODEL, AUX>(a, n);
    const bool live = ln.t0 < Tpair;
    /* a segment window's chunk 0 enters from the state scan_bound_kernel stored */
    const bool entered = c > 0 || a.seg_nofirst;
    ln.noinit = a.seg_nofirst != 0;
    double al[K], be[K];
    double lsa = 0.0, lsb = 0.0;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        al[k] = (entered && live) ? a.sc_st[p + a.P * (int64_t)(c * K + k)] : 0.0;
        be[k] = 1.0;
        if (fb_base(MODE) != FB_FWD && live)
            be[k] = a.sc_be[p + a.P * (int64_t)(c * K + k)];
    }
    if (entered && live)
        lsa = a.sc_sl[p + a.P * (int64_t)c];
    if (fb_base(MODE) != FB_FWD && live)
        lsb = a.sc_bl[p + a.P * (int64_t)c];
    fb_sweep<MODEL, K, MODE, true>(a, ln, sp, al, lsa, be, lsb);
}

} // namespace hhmm
