// Fused circular rational-quadratic spline with its backward, for the training path
// (Algorithm 2).  One thread per spline element (sample x
// feature); the knots are rebuilt from the unnormalised parameters in registers in
// both passes, so the backward stores nothing but the inputs.
//
// Forward: unconstrained_rational_quadratic_spline, circular-tail branch
// (NF/normflows/utils/splines.py:16-88) + rational_quadratic_spline (:91-222): identity
// and log-det 0 outside [-B, B]; inside: softmax -> min-width affine -> cumsum -> [-B, B]
// with pinned ends (all in double from the float exponentials on, each knot rounded once);
// derivatives 1e-3 + softplus; searchsorted with the eps on the last knot; the
// rational-quadratic map (forward) or its quadratic-root inverse (the root in its
// cancellation-free form, pinned to [0, 1]), and the log|det|.
// Backward: reverse-mode by hand.  Forward direction: through theta = (x - cw_b)/w_b.
// Inverse direction: the root theta* solves F(theta) = y, so its adjoint reaches y and
// the knot values through -F_q / F_theta (implicit function theorem).  Knot adjoints go
// back through the pinned cumsum (suffix sums), the min-width affine and softmax;
// derivative adjoints through softplus (threshold 20, as torch).
//
// There is one spline family.  The arithmetic of an element in its bin (rqs_bin_theta, rqs_bin,
// rqs_bin_bwd) does not depend on the bin count; the knot builder, the bin search and the
// per-element functions are written once over the bin-count policy Bins<KT> (compile-time K, or
// K a run-time value up to kAnyMaxK), and so are the coupling-layer kernels further down.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <stdlib.h>

#include <atomic>
#include <type_traits>

#include "fs_internal.h"

#pragma clang fp contract(off)

namespace fs {

constexpr float kMin = 1e-3f;  // DEFAULT_MIN_BIN_WIDTH / HEIGHT / DERIVATIVE (splines.py:6-8)

// ---------------------------------------------------------------------------
// The bin count of everything below: Bins<KT> is a compile-time K = KT (5, 8, 15, 32), Bins<0> a
// run-time one, 1 <= K <= kAnyMaxK (fs_rqs_*_any_impl and fs_coupling.any_k: the general-shape
// mode's training step at a bin count no kernel is instantiated for).  Every spline primitive, row
// function and kernel is written once over it.  With a compile-time K the loops over the bins
// unroll whole and the per-thread arrays stay registers; with a run-time K they have kAnyMaxK
// entries in private memory and the loops run to K.  What else differs lies behind
// `if constexpr (B::fixed)`: how a bin's knots are read (pick_bin), where the adjoints are stored
// (adj_dst), and both shapes of one statement sequence in knots_pair and density_bwd_row4.  Both
// policies do the same operations in the same order ('General-shape mode'), so at K in
// {5, 8, 15, 32} Bins<0> gives what Bins<K> gives up to the compiler's choice of instructions.
constexpr int kAnyMaxK = 32;

template <int KT>
struct Bins {
    static constexpr int kt = KT;
    static constexpr bool fixed = KT > 0;
    static constexpr int cap = fixed ? KT : kAnyMaxK;  // of an array over the bins
    static constexpr int unroll = fixed ? KT + 1 : 4;   // whole loop (at most K + 1 trips) / four scratch loads in flight
    int rt;  // the run-time K (Bins<0> only)
    __device__ __forceinline__ int k() const { return fixed ? KT : rt; }
};

// for (int k = 0; k < n; ++k) { body } in a function templated on the policy B: unrolled whole with a
// compile-time K (the arrays it indexes stay registers), left to the compiler with a run-time one.
// A macro, because where a function that took the body is inlined changes the instantiated
// kernels' instruction streams.
#define FS_BINS_FOR(k, n, ...)                                              \
    {                                                                       \
        if constexpr (B::fixed) {                                           \
            _Pragma("unroll") for (int k = 0; k < (n); ++k) { __VA_ARGS__ } \
        } else {                                                            \
            for (int k = 0; k < (n); ++k) { __VA_ARGS__ }                   \
        }                                                                   \
    }

// Where rqs_point_bwd's adjoints go.  With a compile-time K they are collected in registers and
// stored to their rows afterwards; with a run-time K the arrays are private memory anyway, so those
// that are stored as they are are written straight to their rows (adj_dst) and only the rescaled
// ones are left to store.
template <class B>
__device__ __forceinline__ float *adj_dst(float *reg, float *row) {
    return B::fixed ? reg : row;
}

template <class B>
struct Knots {
    float c[B::cap + 1];  // cumulative knots, pinned ends
    float p[B::cap];      // softmax probabilities
};

template <class B>
__device__ __forceinline__ void build_knots(B bins, const float *u, float bound, Knots<B> &kn) {
    const int K = bins.k();
    float m = u[0];
#pragma unroll B::unroll
    for (int k = 1; k < K; ++k) m = fmaxf(m, u[k]);
    // From the float exponentials on, the knots are built in double and rounded once (as the
    // inference passes build theirs, flow_device.h).  In float, next to one logit far above the
    // others the normaliser adds K - 1 equal small terms to ~1, each rounded the same way: at
    // K = 32 every knot behind the wide bin was off by 42 ulp(B); and a cumulative sum rounded to
    // float before the affine map leaves each knot 1 - 2 ulp(B) off, which a steep bin turns into
    // 1e-3 of the log-det's gradients (tests/spline_sharp_cases.py).
    double sd = 0.0;
#pragma unroll B::unroll
    for (int k = 0; k < K; ++k) {
        kn.p[k] = expf(u[k] - m);
        sd += (double)kn.p[k];
    }
    const double inv = 1.0 / sd;
    const double c1 = 1.0 - 1e-3 * (double)K;
    double cs = 0.0;
    kn.c[0] = -bound;
#pragma unroll B::unroll
    for (int k = 0; k < K; ++k) {
        const double pk = (double)kn.p[k] * inv;
        kn.p[k] = (float)pk;
        cs += 1e-3 + c1 * pk;
        if (k < K - 1) kn.c[k + 1] = (float)((2.0 * (double)bound) * cs - (double)bound);
    }
    kn.c[K] = bound;
}

__device__ __forceinline__ float softplus(float v) { return v > 20.f ? v : log1pf(expf(v)); }
__device__ __forceinline__ float softplus_grad(float v) {
    if (v > 20.f) return 1.f;
    const float z = expf(v);
    return z / (z + 1.f);
}

// knots c[b], c[b+1] of bin b: with a compile-time K by a register scan (a dynamically indexed
// array would live in scratch memory), with a run-time K the array is there anyway
template <class B>
__device__ __forceinline__ void pick_bin(const float *c, int b, float &lo, float &hi) {
    if constexpr (B::fixed) {
        lo = c[0];
        hi = c[1];
#pragma unroll
        for (int k = 1; k < B::kt; ++k) {
            if (k == b) {
                lo = c[k];
                hi = c[k + 1];
            }
        }
    } else {
        lo = c[b];
        hi = c[b + 1];
    }
}

// the bin that contains x (searchsorted over `knots`, eps on the last one)
template <class B>
__device__ __forceinline__ int find_bin(B bins, float x, const float *knots) {
    const int K = bins.k();
    int b = -1;
#pragma unroll B::unroll
    for (int k = 0; k <= K; ++k) {
        const float kv = (k == K) ? knots[K] + 1e-6f : knots[k];
        b += (x >= kv) ? 1 : 0;
    }
    return b < 0 ? 0 : (b > K - 1 ? K - 1 : b);
}

// ---------------------------------------------------------------------------
// One element in its bin: knots (icw, cw1) x (ich, ch1), end derivatives d0, d1.  Nothing here
// depends on the bin count.

// theta in [0, 1]: forward (x - cw_b) / w_b, inverse the root of the quadratic (a NaN
// discriminant sets *nan_flag, nullable, right here: reporting it to the caller instead moves the
// branch and with it the instruction stream of every inverse kernel)
template <bool INV>
__device__ __forceinline__ float rqs_bin_theta(float xv, float icw, float ibw, float ich, float ih, float s, float d0,
                                               float d1, int32_t *nan_flag) {
    if (INV) {
        const float sdd = d0 + d1 - 2.f * s;
        const float a = (xv - ich) * sdd + ih * (s - d0);
        const float bb = ih * d0 - (xv - ich) * sdd;
        const float c = -s * (xv - ich);
        const float disc = fabsf(bb * bb - 4.f * a * c);
        if (disc != disc && nan_flag) atomicOr(nan_flag, 1);
        // The reference takes 2 c / (-bb - sqrt(disc)) whatever the sign of bb.  For bb < 0 that
        // subtracts two nearly equal numbers; the same root as (-bb + sqrt(disc)) / (2 a) does not.
        // The exact root lies in [0, 1]: pinned there, the logarithms of the log-det keep positive
        // arguments where the discriminant itself cancels (flow_device.h, rqs_eval).  A NaN stays NaN.
        const float sq = sqrtf(disc);
        const float root = bb >= 0.f ? (2.f * c) / (-bb - sq) : (sq - bb) / (2.f * a);
        return root > 1.f ? 1.f : (root < 0.f ? 0.f : root);
    }
    return (xv - icw) / ibw;
}

// the rational-quadratic map (forward) or its inverse, and the log|det|
template <bool INV>
__device__ __forceinline__ void rqs_bin(float xv, float icw, float cw1, float ich, float ch1, float d0, float d1,
                                        float &out, float &lad, int32_t *nan_flag) {
    const float ibw = cw1 - icw, ih = ch1 - ich;
    const float s = ih / ibw;
    const float th = rqs_bin_theta<INV>(xv, icw, ibw, ich, ih, s, d0, d1, nan_flag);
    const float t = th * (1.f - th);
    const float den = s + (d0 + d1 - 2.f * s) * t;
    const float A = d1 * th * th + 2.f * s * t + d0 * (1.f - th) * (1.f - th);
    const float l = logf(s * s * A) - 2.f * logf(den);
    if (INV) {
        out = th * ibw + icw;
        lad = -l;
    } else {
        out = ich + ih * (s * th * th + d0 * t) / den;
        lad = l;
    }
}

// rqs_bin's adjoints from those of out (go) and lad (gl): of x, of the bin's lower knots and its
// width and height (ibw = cw1 - icw, ih = ch1 - ich), and of d0 and d1
struct BinGrads {
    float gx, g_icw, g_ibw, g_ich, g_ih, g_d0, g_d1;
};

template <bool INV>
__device__ __forceinline__ BinGrads rqs_bin_bwd(float xv, float icw, float cw1, float ich, float ch1, float d0,
                                                float d1, float go, float gl) {
    const float ibw = cw1 - icw, ih = ch1 - ich;
    const float s = ih / ibw;
    const float th = rqs_bin_theta<INV>(xv, icw, ibw, ich, ih, s, d0, d1, nullptr);
    const float t = th * (1.f - th);
    const float omt = 1.f - th;
    const float Nn = s * th * th + d0 * t;
    const float den = s + (d0 + d1 - 2.f * s) * t;
    const float A = d1 * th * th + 2.f * s * t + d0 * omt * omt;
    const float dnum = s * s * A;
    float g_th = 0.f, g_s = 0.f, g_t = 0.f, g_d0 = 0.f, g_d1 = 0.f;
    float g_icw = 0.f, g_ibw = 0.f, g_ich = 0.f, g_ih = 0.f, g_x = 0.f;
    // log-det part: l = log(dnum) - 2 log(den); forward lad = l, inverse lad = -l
    const float gll = INV ? -gl : gl;
    {
        const float g_dnum = gll / dnum;
        const float g_den = -2.f * gll / den;
        const float g_A = g_dnum * s * s;
        g_s += g_dnum * 2.f * s * A + g_A * 2.f * t;
        g_d1 += g_A * th * th;
        g_d0 += g_A * omt * omt;
        g_th += g_A * (2.f * d1 * th - 2.f * d0 * omt);
        g_t += g_A * 2.f * s;
        g_s += g_den * (1.f - 2.f * t);
        g_d0 += g_den * t;
        g_d1 += g_den * t;
        g_t += g_den * (d0 + d1 - 2.f * s);
    }
    if (INV) {
        // out = theta * w_b + cw_b
        g_th += go * ibw;
        g_icw += go;
        g_ibw += go * th;
        g_th += g_t * (1.f - 2.f * th);
        // theta* solves F(theta) = y, F = ch_b + h_b * N / den
        const float N_th = 2.f * s * th + d0 * (1.f - 2.f * th);
        const float den_th = (d0 + d1 - 2.f * s) * (1.f - 2.f * th);
        const float F_th = ih * (N_th * den - Nn * den_th) / (den * den);
        const float F_s = ih * (th * th * den - Nn * (1.f - 2.f * t)) / (den * den);
        const float F_d0 = ih * (t * den - Nn * t) / (den * den);
        const float F_d1 = -ih * Nn * t / (den * den);
        const float wgt = g_th / F_th;
        g_x += wgt;
        g_ich -= wgt;
        g_ih -= wgt * Nn / den;
        g_s -= wgt * F_s;
        g_d0 -= wgt * F_d0;
        g_d1 -= wgt * F_d1;
    } else {
        // out = ch_b + h_b * N / den
        const float g_num = go / den;
        const float g_den = -go * (ih * Nn) / (den * den);
        g_ich += go;
        g_ih += g_num * Nn;
        const float g_N = g_num * ih;
        g_s += g_N * th * th;
        g_th += g_N * 2.f * s * th;
        g_d0 += g_N * t;
        g_t += g_N * d0;
        g_s += g_den * (1.f - 2.f * t);
        g_d0 += g_den * t;
        g_d1 += g_den * t;
        g_t += g_den * (d0 + d1 - 2.f * s);
        g_th += g_t * (1.f - 2.f * th);
        // theta = (x - cw_b) / w_b
        g_x += g_th / ibw;
        g_icw -= g_th / ibw;
        g_ibw -= g_th * th / ibw;
    }
    // s = h_b / w_b
    g_ih += g_s / ibw;
    g_ibw -= g_s * s / ibw;
    return BinGrads{g_x, g_icw, g_ibw, g_ich, g_ih, g_d0, g_d1};
}

// ---------------------------------------------------------------------------
// one element from its built knots (wc: width knots, hc: height knots); x inside [-B, B]
template <bool INV, class B>
__device__ __forceinline__ void rqs_eval_knots(B bins, float xv, const float *wc, const float *hc, const float *dd,
                                               float &out, float &lad, int32_t *nan_flag) {
    const int b = find_bin(bins, xv, INV ? hc : wc);
    const float d0 = kMin + softplus(dd[b]), d1 = kMin + softplus(dd[b + 1]);
    float icw, cw1, ich, ch1;
    pick_bin<B>(wc, b, icw, cw1);
    pick_bin<B>(hc, b, ich, ch1);
    rqs_bin<INV>(xv, icw, cw1, ich, ch1, d0, d1, out, lad, nan_flag);
}

// one element: x inside [-B, B] (callers route the outside identity themselves)
template <bool INV, class B>
__device__ __forceinline__ void rqs_point(B bins, float xv, const float *uw, const float *uh, const float *dd,
                                          float bound, float &out, float &lad, int32_t *nan_flag) {
    Knots<B> W, Hh;
    build_knots(bins, uw, bound, W);
    build_knots(bins, uh, bound, Hh);
    rqs_eval_knots<INV>(bins, xv, W.c, Hh.c, dd, out, lad, nan_flag);
}

// KT: Bins<KT>, with Krt the run-time bin count of Bins<0> (last, so that the instantiated
// kernels' other arguments keep their offsets)
template <int KT, bool INV>
__global__ __launch_bounds__(256) void rqs_forward_kernel(int64_t M, const float *__restrict__ x, const float *__restrict__ uw,
                                   const float *__restrict__ uh, const float *__restrict__ ud, float bound,
                                   float *__restrict__ out, float *__restrict__ lad, int32_t *__restrict__ nan_flag,
                                   int Krt) {
    const Bins<KT> bins{Krt};
    const int K = bins.k();
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M) return;
    const float xv = x[i];
    if (!(xv >= -bound && xv <= bound)) {
        out[i] = xv;
        lad[i] = 0.f;
        return;
    }
    rqs_point<INV>(bins, xv, uw + i * K, uh + i * K, ud + i * (K + 1), bound, out[i], lad[i], nan_flag);
}

// The knot adjoints of one element: only knots b and b + 1 of its bin carry one (gw0 / gw1 of the
// width knots, gh0 / gh1 of the height knots).
struct BinAdjoint {
    int b;
    float gw0, gw1, gh0, gh1;
};

// knot adjoints (g_b at knot b, g_b1 at knot b + 1, zero elsewhere) -> unnormalised-parameter adjoints
template <class B>
__device__ __forceinline__ void knots_backward(B bins, const Knots<B> &kn, int b, float g_b, float g_b1, float bound,
                                               float *gu) {
    const int K = bins.k();
    const float c1 = 1.f - kMin * (float)K;
    // c[k] = 2B * C[k] - B (k = 1..K-1), C[k] = sum_{j<k} w_j; c[0], c[K] pinned.  The adjoint of w_j is
    // v_j = Gb + Gb1 (j < b), Gb1 (j == b), 0 (j > b)
    const float Gb = b >= 1 ? (2.f * bound) * g_b : 0.f;
    const float Gb1 = b + 1 <= K - 1 ? (2.f * bound) * g_b1 : 0.f;
    // softmax: gu_j = p_j c1 (v_j - sum_i p_i v_i).  Next to a p_i near 1 that difference cancels
    // (1 % of the gradient at a logit 12 above the others).  With sum_i p_i = 1 it is
    // sum_i p_i (v_j - v_i): over the three levels of v, sums of the p below, at and above bin b.
    float plt = 0.f, pb = 0.f, pgt = 0.f;
#pragma unroll B::unroll
    for (int j = 0; j < K; ++j) {
        plt += j < b ? kn.p[j] : 0.f;
        pb = j == b ? kn.p[j] : pb;
        pgt += j > b ? kn.p[j] : 0.f;
    }
    const float below = Gb * pb + (Gb + Gb1) * pgt;      // j < b
    const float at = Gb1 * pgt - Gb * plt;               // j == b
    const float above = -((Gb + Gb1) * plt + Gb1 * pb);  // j > b
#pragma unroll B::unroll
    for (int j = 0; j < K; ++j) gu[j] = kn.p[j] * (c1 * (j < b ? below : (j == b ? at : above)));
}

// the adjoint core of one element inside [-B, B] from its built knots: gx, the bin's knot adjoints
// and the derivative logits' adjoints gud[0..K]
template <bool INV, class B>
__device__ __forceinline__ BinAdjoint rqs_bwd_core(B bins, float xv, const float *wc, const float *hc,
                                                   const float *dd, float go, float gl, float &gx, float *gud) {
    const int K = bins.k();
    const int b = find_bin(bins, xv, INV ? hc : wc);
    const float e0 = dd[b], e1 = dd[b + 1];
    const float d0 = kMin + softplus(e0), d1 = kMin + softplus(e1);
    float icw, cw1, ich, ch1;
    pick_bin<B>(wc, b, icw, cw1);
    pick_bin<B>(hc, b, ich, ch1);
    const BinGrads r = rqs_bin_bwd<INV>(xv, icw, cw1, ich, ch1, d0, d1, go, gl);
    gx = r.gx;
    FS_BINS_FOR(k, K + 1,
                float g = 0.f;
                if (k == b) g = r.g_d0 * softplus_grad(e0);
                if (k == b + 1) g = r.g_d1 * softplus_grad(e1);
                gud[k] = g;)
    return BinAdjoint{b, r.g_icw - r.g_ibw, r.g_ibw, r.g_ich - r.g_ih, r.g_ih};
}

// adjoints of one element inside [-B, B]: gx, guw[K], guh[K], gud[K+1]
template <bool INV, class B>
__device__ __forceinline__ void rqs_point_bwd(B bins, float xv, const float *uw, const float *uh, const float *dd,
                                              float bound, float go, float gl, float &gx, float *guw, float *guh,
                                              float *gud) {
    Knots<B> W, Hh;
    build_knots(bins, uw, bound, W);
    build_knots(bins, uh, bound, Hh);
    const BinAdjoint a = rqs_bwd_core<INV>(bins, xv, W.c, Hh.c, dd, go, gl, gx, gud);
    knots_backward(bins, W, a.b, a.gw0, a.gw1, bound, guw);
    knots_backward(bins, Hh, a.b, a.gh0, a.gh1, bound, guh);
}

template <int KT, bool INV>
__global__ __launch_bounds__(256) void rqs_backward_kernel(int64_t M, const float *__restrict__ x, const float *__restrict__ uw,
                                    const float *__restrict__ uh, const float *__restrict__ ud, float bound,
                                    const float *__restrict__ g_out, const float *__restrict__ g_lad,
                                    float *__restrict__ gx, float *__restrict__ guw, float *__restrict__ guh,
                                    float *__restrict__ gud, int Krt) {
    using B = Bins<KT>;
    const B bins{Krt};
    const int K = bins.k();
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M) return;
    const float xv = x[i];
    const float go = g_out ? g_out[i] : 0.f, gl = g_lad ? g_lad[i] : 0.f;
    // with a run-time K the adjoints go straight to their rows (adj_dst); the pointers are formed
    // here, before the branch, and only then: either way moved changes the other policy's kernels
    float *pw = nullptr, *ph = nullptr, *pd = nullptr;
    if constexpr (!B::fixed) {
        pw = guw + i * K;
        ph = guh + i * K;
        pd = gud + i * (K + 1);
    }
    if (!(xv >= -bound && xv <= bound)) {
        gx[i] = go;
        FS_BINS_FOR(k, K, guw[i * K + k] = 0.f; guh[i * K + k] = 0.f;)
        FS_BINS_FOR(k, K + 1, gud[i * (K + 1) + k] = 0.f;)
        return;
    }
    float a[B::cap], b[B::cap], d[B::cap + 1];
    rqs_point_bwd<INV>(bins, xv, uw + i * K, uh + i * K, ud + i * (K + 1), bound, go, gl, gx[i], adj_dst<B>(a, pw),
                       adj_dst<B>(b, ph), adj_dst<B>(d, pd));
    if constexpr (B::fixed) {
        FS_BINS_FOR(k, K, guw[i * K + k] = a[k]; guh[i * K + k] = b[k];)
        FS_BINS_FOR(k, K + 1, gud[i * (K + 1) + k] = d[k];)
    }
}

// ---------------------------------------------------------------------------
// One coupling layer of the training path around its conditioner: the feature gather,
// periodic features (nn.py:120-137), the conditional and unconditional splines, the
// half-roll and the log-det sums (coupling.py:71-134, wrapper.py:269-275) in one launch
// per side of the conditioner instead of ~30 torch kernels.  One wave per sample row,
// lane = feature j (j += 64); log-det sums are wave reductions read from lane 0.
struct CouplingArgs {
    int64_t rows;
    int D, n, split;
    int K;  // the bin count, read by the Bins<0> kernels only (in what was padding)
    const int64_t *id, *tr;
    float bound, scale, sq;
};

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return __shfl(v, 0);
}

template <class B>
__device__ __forceinline__ void cond_params(B bins, const float *p, float sq, float *w, float *h) {
    const int K = bins.k();
#pragma unroll B::unroll
    for (int k = 0; k < K; ++k) {
        w[k] = p[k] / sq;  // params[..., :K] / sqrt(H) (coupling.py:340-342)
        h[k] = p[K + k] / sq;
    }
}

#ifndef FS_CPL_ROWS
#define FS_CPL_ROWS 1  // A/B at batch 256 (profiles/r02/train/cpl_rows_ab.log): 1 row ~1 % ahead of 2 or 4
#endif
// sample rows (one wave each) per workgroup of the coupling kernels
constexpr int kCplRows = FS_CPL_ROWS;

// density direction forward (Coupling.forward), after the conditioner: both splines,
// rolled output, lq_out = lq_in + (sum lad_cond + sum lad_uncond)
struct DensityFwdArgs {
    const float *x, *params, *uw, *uh, *ud, *lq_in;
    float *out, *lq_out;
};

template <class B>
__device__ __forceinline__ void density_fwd_row(B bins, const CouplingArgs &c, const DensityFwdArgs &d, int64_t row,
                                                float *rb = nullptr) {
    const int lane = threadIdx.x & 63, K = bins.k();
    const float *xr = d.x + row * c.D;
    float sc = 0.f, su = 0.f;
    for (int j = lane; j < c.n; j += 64) {
        const int pi = (int)c.id[j], pt = (int)c.tr[j];
        const float xi = xr[pi], xt = xr[pt];
        float yt = xt, lt = 0.f;
        if (xt >= -c.bound && xt <= c.bound) {
            const float *p = d.params + (row * c.n + j) * (3 * K + 1);
            float w[B::cap], h[B::cap];
            cond_params(bins, p, c.sq, w, h);
            rqs_point<false>(bins, xt, w, h, p + 2 * K, c.bound, yt, lt, nullptr);
        }
        float yi = xi, li = 0.f;
        if (xi >= -c.bound && xi <= c.bound)
            rqs_point<false>(bins, xi, d.uw + j * K, d.uh + j * K, d.ud + j * (K + 1), c.bound, yi, li, nullptr);
        d.out[row * c.D + (pt + c.D - c.split) % c.D] = yt;
        d.out[row * c.D + (pi + c.D - c.split) % c.D] = yi;
        if (rb) {  // the row for the next layer's features in the same launch
            rb[(pt + c.D - c.split) % c.D] = yt;
            rb[(pi + c.D - c.split) % c.D] = yi;
        }
        sc += lt;
        su += li;
    }
    sc = wave_sum(sc);
    su = wave_sum(su);
    if (lane == 0) d.lq_out[row] = (d.lq_in ? d.lq_in[row] : 0.f) + (sc + su);
}

// KT: Bins<KT>, with c.K the run-time bin count of Bins<0>
template <int KT>
__global__ __launch_bounds__(256) void coupling_density_fwd_kernel(CouplingArgs c, DensityFwdArgs d) {
    const int64_t row = (int64_t)blockIdx.x * kCplRows + (threadIdx.x >> 6);
    if (row < c.rows) density_fwd_row(Bins<KT>{c.K}, c, d, row);
}

// density_fwd_row's adjoints: gx (both halves, spline part), g_params [rows][n][3K+1], g_u the
// per-row unconditional adjoints [rows][n][3K+1] (summed over rows by the caller)
// two waves per row: wave part 0 takes the conditional spline's adjoints, part 1 the
// unconditional one's (each lane one feature), so the row's work is spread twice as wide.
// gor: the row of g_out (nullable: no output gradient)
template <class B>
__device__ __forceinline__ void density_bwd_row(B bins, const CouplingArgs &c, const float *__restrict__ x,
                                                const float *__restrict__ params, const float *__restrict__ uw,
                                                const float *__restrict__ uh, const float *__restrict__ ud,
                                                const float *gor, const float *__restrict__ g_lq, float *gx,
                                                float *g_params, float *g_u, int64_t row, int part) {
    const int lane = threadIdx.x & 63, K = bins.k();
    const float *xr = x + row * c.D;
    const float gl = g_lq ? g_lq[row] : 0.f;
    const int P = 3 * K + 1;
    for (int j = lane; j < c.n; j += 64) {
        const int pi = (int)c.id[j], pt = (int)c.tr[j];
        const float xi = xr[pi], xt = xr[pt];
        const float got = gor ? gor[(pt + c.D - c.split) % c.D] : 0.f;
        const float goi = gor ? gor[(pi + c.D - c.split) % c.D] : 0.f;
        float *gp = g_params + (row * c.n + j) * P;
        // g_u row: [uw n*K | uh n*K | ud n*(K+1)], the parameters' own layouts back to back
        float *guw = g_u + row * c.n * P + j * K;
        float *guh = guw + c.n * K;
        float *gud = g_u + row * c.n * P + 2 * c.n * K + j * (K + 1);
        float gw[B::cap], gh[B::cap], gd[B::cap + 1];
        if (part == 1) {
        } else if (xt >= -c.bound && xt <= c.bound) {
            const float *p = params + (row * c.n + j) * P;
            float w[B::cap], h[B::cap];
            cond_params(bins, p, c.sq, w, h);
            float g;
            rqs_point_bwd<false>(bins, xt, w, h, p + 2 * K, c.bound, got, gl, g, gw, gh, adj_dst<B>(gd, gp + 2 * K));
            gx[row * c.D + pt] = g;
            FS_BINS_FOR(k, K, gp[k] = gw[k] / c.sq; gp[K + k] = gh[k] / c.sq;)
            if constexpr (B::fixed) FS_BINS_FOR(k, K + 1, gp[2 * K + k] = gd[k];)
        } else {
            gx[row * c.D + pt] = got;
            FS_BINS_FOR(k, P, gp[k] = 0.f;)
        }
        if (part == 0) {
        } else if (xi >= -c.bound && xi <= c.bound) {
            float g;
            rqs_point_bwd<false>(bins, xi, uw + j * K, uh + j * K, ud + j * (K + 1), c.bound, goi, gl, g,
                                  adj_dst<B>(gw, guw), adj_dst<B>(gh, guh), adj_dst<B>(gd, gud));
            gx[row * c.D + pi] = g;
            if constexpr (B::fixed) {
                FS_BINS_FOR(k, K, guw[k] = gw[k]; guh[k] = gh[k];)
                FS_BINS_FOR(k, K + 1, gud[k] = gd[k];)
            }
        } else {
            gx[row * c.D + pi] = goi;
            FS_BINS_FOR(k, K, guw[k] = 0.f; guh[k] = 0.f;)
            FS_BINS_FOR(k, K + 1, gud[k] = 0.f;)
        }
    }
}

template <int KT>
__global__ __launch_bounds__(256) void coupling_density_bwd_kernel(
    CouplingArgs c, const float *__restrict__ x, const float *__restrict__ params, const float *__restrict__ uw,
    const float *__restrict__ uh, const float *__restrict__ ud, const float *__restrict__ g_out,
    const float *__restrict__ g_lq, float *gx, float *g_params, float *g_u) {
    const int wv = threadIdx.x >> 6;
    const int64_t row = (int64_t)blockIdx.x * kCplRows + (wv >> 1);
    if (row >= c.rows) return;
    density_bwd_row(Bins<KT>{c.K}, c, x, params, uw, uh, ud, g_out ? g_out + row * c.D : nullptr, g_lq, gx, g_params,
                    g_u, row, wv & 1);
}

// density direction, before the conditioner: t = [cos(s x_id), sin(s x_id)]
__device__ __forceinline__ void features_row(const CouplingArgs &c, const float *__restrict__ x, float *t, int64_t row,
                                             const float *xr = nullptr) {
    const int lane = threadIdx.x & 63;
    if (!xr) xr = x + row * c.D;
    for (int j = lane; j < c.n; j += 64) {
        const float v = c.scale * xr[c.id[j]];
        t[row * 2 * c.n + j] = cosf(v);
        t[row * 2 * c.n + c.n + j] = sinf(v);
    }
}

__global__ __launch_bounds__(256) void coupling_features_fwd_kernel(CouplingArgs c, const float *__restrict__ x,
                                                                    float *t) {
    const int64_t row = (int64_t)blockIdx.x * kCplRows + (threadIdx.x >> 6);
    if (row < c.rows) features_row(c, x, t, row);
}

// adjoint of the periodic features t = [cos(s x_id), sin(s x_id)]: gx at the identity
// positions, 0 at the transform positions (+ gx_add, the splines' gradient of the same x)
__device__ __forceinline__ void features_bwd_row(const CouplingArgs &c, const float *__restrict__ x,
                                                 const float *__restrict__ g_t, float *gx,
                                                 const float *__restrict__ gx_add, int64_t row, float *rb = nullptr) {
    const int lane = threadIdx.x & 63;
    for (int j = lane; j < c.n; j += 64) {
        const int pi = (int)c.id[j], pt = (int)c.tr[j];
        const float v = c.scale * x[row * c.D + pi];
        const float gc = g_t[row * 2 * c.n + j] * -sinf(v), gs = g_t[row * 2 * c.n + c.n + j] * cosf(v);
        const float ai = gx_add ? gx_add[row * c.D + pi] : 0.f, at = gx_add ? gx_add[row * c.D + pt] : 0.f;
        const float gi = (gc * c.scale + gs * c.scale) + ai;
        gx[row * c.D + pi] = gi;
        gx[row * c.D + pt] = at;
        if (rb) {
            rb[pi] = gi;
            rb[pt] = at;
        }
    }
}

__global__ __launch_bounds__(256) void coupling_features_bwd_kernel(CouplingArgs c, const float *__restrict__ x,
                                                                    const float *__restrict__ g_t, float *gx,
                                                                    const float *__restrict__ gx_add) {
    const int64_t row = (int64_t)blockIdx.x * kCplRows + (threadIdx.x >> 6);
    if (row >= c.rows) return;
    features_bwd_row(c, x, g_t, gx, gx_add, row);
}

// The backward between two layers of the density pass in one launch (fs_coupling_bwd_step):
// layer l's features adjoint (its input gradient, = the output gradient of layer l - 1,
// kept in LDS and also written to gx) and then layer l - 1's spline adjoints on that row,
// each exactly as fs_coupling_features_bwd then fs_coupling_density_bwd compute them.
constexpr int kCplMaxDB = 256;

template <int KT>
__global__ __launch_bounds__(256) void coupling_bwd_step_kernel(CouplingArgs cf, const float *__restrict__ xf,
                                                                const float *__restrict__ g_t, float *gxf,
                                                                const float *__restrict__ gx_add, CouplingArgs c,
                                                                const float *__restrict__ x,
                                                                const float *__restrict__ params,
                                                                const float *__restrict__ uw,
                                                                const float *__restrict__ uh,
                                                                const float *__restrict__ ud,
                                                                const float *__restrict__ g_lq, float *gx,
                                                                float *g_params, float *g_u) {
    __shared__ float rbuf[kCplRows][kCplMaxDB];
    const int wv = threadIdx.x >> 6;
    float *rb = rbuf[wv >> 1];
    const int64_t row = (int64_t)blockIdx.x * kCplRows + (wv >> 1);
    const bool live = row < c.rows;
    if (live && (wv & 1) == 0) features_bwd_row(cf, xf, g_t, gxf, gx_add, row, rb);
    __syncthreads();
    if (!live) return;
    density_bwd_row(Bins<KT>{c.K}, c, x, params, uw, uh, ud, rb, g_lq, gx, g_params, g_u, row, wv & 1);
}

// sampling direction (Coupling.inverse), forward only: roll, unconditional inverse spline
// of the identity half, features of its output; out holds the new identity values and
// the untouched transform half; lad_u[row] = its log-det sum
struct SamplePreArgs {
    const float *z, *uw, *uh, *ud;
    float *t, *out, *lad_u;
    int32_t *nan_flag;
};

template <class B>
__device__ __forceinline__ void sample_pre_row(B bins, const CouplingArgs &c, const SamplePreArgs &s, int64_t row,
                                               const float *zr = nullptr) {
    const int lane = threadIdx.x & 63, K = bins.k();
    if (!zr) zr = s.z + row * c.D;
    float su = 0.f;
    for (int j = lane; j < c.n; j += 64) {
        const int pi = (int)c.id[j], pt = (int)c.tr[j];
        const float xi = zr[(pi + c.split) % c.D];
        float yi = xi, li = 0.f;
        if (xi >= -c.bound && xi <= c.bound)
            rqs_point<true>(bins, xi, s.uw + j * K, s.uh + j * K, s.ud + j * (K + 1), c.bound, yi, li, s.nan_flag);
        const float v = c.scale * yi;
        s.t[row * 2 * c.n + j] = cosf(v);
        s.t[row * 2 * c.n + c.n + j] = sinf(v);
        s.out[row * c.D + pi] = yi;
        s.out[row * c.D + pt] = zr[(pt + c.split) % c.D];
        su += li;
    }
    su = wave_sum(su);
    if (lane == 0) s.lad_u[row] = su;
}

template <int KT>
__global__ __launch_bounds__(256) void coupling_sample_pre_kernel(CouplingArgs c, SamplePreArgs s) {
    const int64_t row = (int64_t)blockIdx.x * kCplRows + (threadIdx.x >> 6);
    if (row < c.rows) sample_pre_row(Bins<KT>{c.K}, c, s, row);
}

// ... then the conditional inverse spline of the transform half in place;
// lq_out = lq_in - (lad_u + sum lad_cond)
struct SamplePostArgs {
    const float *params, *lad_u, *lq_in;
    float *out, *lq_out;
    int32_t *nan_flag;
};

template <class B>
__device__ __forceinline__ void sample_post_row(B bins, const CouplingArgs &c, const SamplePostArgs &s, int64_t row,
                                                float *rb = nullptr) {
    const int lane = threadIdx.x & 63, K = bins.k();
    float sc = 0.f;
    for (int j = lane; j < c.n; j += 64) {
        const int pt = (int)c.tr[j];
        if (rb) {
            const int pi = (int)c.id[j];
            rb[pi] = s.out[row * c.D + pi];  // written by this layer's pre launch
        }
        const float xt = s.out[row * c.D + pt];
        float yt = xt, lt = 0.f;
        if (xt >= -c.bound && xt <= c.bound) {
            const float *p = s.params + (row * c.n + j) * (3 * K + 1);
            float w[B::cap], h[B::cap];
            cond_params(bins, p, c.sq, w, h);
            rqs_point<true>(bins, xt, w, h, p + 2 * K, c.bound, yt, lt, s.nan_flag);
        }
        s.out[row * c.D + pt] = yt;
        if (rb) rb[pt] = yt;
        sc += lt;
    }
    sc = wave_sum(sc);
    if (lane == 0) s.lq_out[row] = (s.lq_in ? s.lq_in[row] : 0.f) - (s.lad_u[row] + sc);
}

template <int KT>
__global__ __launch_bounds__(256) void coupling_sample_post_kernel(CouplingArgs c, SamplePostArgs s) {
    const int64_t row = (int64_t)blockIdx.x * kCplRows + (threadIdx.x >> 6);
    if (row < c.rows) sample_post_row(Bins<KT>{c.K}, c, s, row);
}

// The training step's two passes side by side (fs_coupling_pair_pre / _post): workgroups
// [0, nb0) run the sampling pass's layer (rows of cs), the rest the density pass's layer
// (rows of cd), each row exactly as the single-pass kernels compute it.
// (both layers have the same bin count: cs.K)
template <int KT>
__global__ __launch_bounds__(256) void coupling_pair_pre_kernel(CouplingArgs cs, SamplePreArgs s, CouplingArgs cd,
                                                                const float *__restrict__ x, float *t, unsigned nb0) {
    const bool dens = blockIdx.x >= nb0;
    const int64_t row = (int64_t)(dens ? blockIdx.x - nb0 : blockIdx.x) * kCplRows + (threadIdx.x >> 6);
    if (!dens) {
        if (row < cs.rows) sample_pre_row(Bins<KT>{cs.K}, cs, s, row);
    } else if (row < cd.rows) {
        features_row(cd, x, t, row);
    }
}

template <int KT>
__global__ __launch_bounds__(256) void coupling_pair_post_kernel(CouplingArgs cs, SamplePostArgs s, CouplingArgs cd,
                                                                 DensityFwdArgs d, unsigned nb0) {
    const Bins<KT> bins{cs.K};
    const bool dens = blockIdx.x >= nb0;
    const int64_t row = (int64_t)(dens ? blockIdx.x - nb0 : blockIdx.x) * kCplRows + (threadIdx.x >> 6);
    if (!dens) {
        if (row < cs.rows) sample_post_row(bins, cs, s, row);
    } else if (row < cd.rows) {
        density_fwd_row(bins, cd, d, row);
    }
}

// One launch between two layers of the training step's passes (fs_coupling_pair_step):
// the post launch of layer l (sampling: conditional inverse spline; density: both splines,
// roll, log-det) and, on the row it just produced (kept in LDS), the pre launch of the
// next layer (sampling: roll + unconditional inverse spline + features; density: the
// features).  Each row exactly as fs_coupling_pair_post then fs_coupling_pair_pre compute
// it; one launch and one HBM round trip of the rows fewer per layer.
constexpr int kCplMaxD = 256;

template <int KT>
__global__ __launch_bounds__(256) void coupling_pair_step_kernel(CouplingArgs cs, SamplePostArgs s, CouplingArgs cs2,
                                                                 SamplePreArgs s2, CouplingArgs cd, DensityFwdArgs d,
                                                                 CouplingArgs cd2, float *t_d2, unsigned nb0) {
    const Bins<KT> bins{cs.K};
    __shared__ float rbuf[kCplRows][kCplMaxD];
    float *rb = rbuf[threadIdx.x >> 6];
    const bool dens = blockIdx.x >= nb0;
    const int64_t row = (int64_t)(dens ? blockIdx.x - nb0 : blockIdx.x) * kCplRows + (threadIdx.x >> 6);
    const bool live = dens ? row < cd.rows : row < cs.rows;
    if (live) {
        if (!dens)
            sample_post_row(bins, cs, s, row, rb);
        else
            density_fwd_row(bins, cd, d, row, rb);
    }
    __syncthreads();  // the row's LDS copy, written by every lane of its wave
    if (!live) return;
    if (!dens)
        sample_pre_row(bins, cs2, s2, row, rb);
    else
        features_row(cd2, d.out, t_d2, row, rb);
}

// ---------------------------------------------------------------------------
// The same two launches with each row's splines spread over more waves
// (fs_set_coupling_waves, default on).  A spline's cost is mostly building its two knot
// sets (softmax + cumulative sum over K, each element a precise division), one lane per
// feature in a serial chain; here wave h of a pair builds one set (h = 0 widths, h = 1
// heights), the pair swaps the knots through LDS and finishes the element from them.
// Every value comes from the same device functions on the same operands, so the
// results are bit-identical to coupling_pair_step_kernel / coupling_bwd_step_kernel
// (tests/test_gpu_train.py).

// this wave's knot set (own) into slot w of kx (K + 1 knots of 64 lanes each, lane-major:
// conflict-free; the kernels reserve B::cap + 1 per slot) and, with its partner's (slot w ^ 1),
// back as (width, height) knots
template <class B>
__device__ __forceinline__ void knots_pair(B bins, float *kx, int w, int h, const float *own, float *wc, float *hc) {
    const int lane = threadIdx.x & 63, K = bins.k();
#pragma unroll B::unroll
    for (int k = 0; k <= K; ++k) kx[(w * (K + 1) + k) * 64 + lane] = own[k];
    __syncthreads();
    if constexpr (B::fixed) {  // all the partner's knots first, then the selects
        float oc[B::cap + 1];
#pragma unroll
        for (int k = 0; k <= K; ++k) oc[k] = kx[((w ^ 1) * (K + 1) + k) * 64 + lane];
#pragma unroll
        for (int k = 0; k <= K; ++k) {
            wc[k] = h == 0 ? own[k] : oc[k];
            hc[k] = h == 0 ? oc[k] : own[k];
        }
    } else {
#pragma unroll 4
        for (int k = 0; k <= K; ++k) {
            const float oc = kx[((w ^ 1) * (K + 1) + k) * 64 + lane];
            wc[k] = h == 0 ? own[k] : oc;
            hc[k] = h == 0 ? oc : own[k];
        }
    }
}

// sample_post_row on a wave pair (h: this wave's knot set); the lower wave stores
template <class B>
__device__ __forceinline__ void sample_post_row2(B bins, const CouplingArgs &c, const SamplePostArgs &s, int64_t row,
                                                 float *rb, float *kx, int h) {
    const int lane = threadIdx.x & 63, K = bins.k();
    float sc = 0.f;
    for (int j0 = 0; j0 < c.n; j0 += 64) {  // uniform trip count: the pair meets at its barriers
        const int j = j0 + lane;
        const bool on = j < c.n;
        const int jj = on ? j : 0;
        const int pt = (int)c.tr[jj];
        if (h == 0 && on) {
            const int pi = (int)c.id[jj];
            rb[pi] = s.out[row * c.D + pi];  // written by this layer's pre launch
        }
        const float xt = s.out[row * c.D + pt];
        const float *p = s.params + (row * c.n + jj) * (3 * K + 1);
        Knots<B> kn;
        {
            float u[B::cap];
            FS_BINS_FOR(k, K, u[k] = p[h * K + k] / c.sq;)  // cond_params' half
            build_knots(bins, u, c.bound, kn);
        }
        float wc[B::cap + 1], hc[B::cap + 1];
        knots_pair(bins, kx, h, h, kn.c, wc, hc);
        float yt = xt, lt = 0.f;
        if (on && xt >= -c.bound && xt <= c.bound)
            rqs_eval_knots<true>(bins, xt, wc, hc, p + 2 * K, yt, lt, h == 0 ? s.nan_flag : nullptr);
        if (h == 0 && on) {
            s.out[row * c.D + pt] = yt;
            rb[pt] = yt;
        }
        sc += on ? lt : 0.f;
        __syncthreads();  // the partner has read this round's knots
    }
    sc = wave_sum(sc);
    if (h == 0 && lane == 0) s.lq_out[row] = (s.lq_in ? s.lq_in[row] : 0.f) - (s.lad_u[row] + sc);
}

// sample_pre_row on a wave pair: the lower wave stores the cosines and the row, the upper
// one the sines
template <class B>
__device__ __forceinline__ void sample_pre_row2(B bins, const CouplingArgs &c, const SamplePreArgs &s, int64_t row,
                                                const float *zr, float *kx, int h) {
    const int lane = threadIdx.x & 63, K = bins.k();
    float su = 0.f;
    for (int j0 = 0; j0 < c.n; j0 += 64) {
        const int j = j0 + lane;
        const bool on = j < c.n;
        const int jj = on ? j : 0;
        const int pi = (int)c.id[jj], pt = (int)c.tr[jj];
        const float xi = zr[(pi + c.split) % c.D];
        Knots<B> kn;
        build_knots(bins, (h == 0 ? s.uw : s.uh) + jj * K, c.bound, kn);
        float wc[B::cap + 1], hc[B::cap + 1];
        knots_pair(bins, kx, h, h, kn.c, wc, hc);
        float yi = xi, li = 0.f;
        if (on && xi >= -c.bound && xi <= c.bound)
            rqs_eval_knots<true>(bins, xi, wc, hc, s.ud + jj * (K + 1), yi, li, h == 0 ? s.nan_flag : nullptr);
        const float v = c.scale * yi;
        if (on) {
            if (h == 0) {
                s.t[row * 2 * c.n + j] = cosf(v);
                s.out[row * c.D + pi] = yi;
                s.out[row * c.D + pt] = zr[(pt + c.split) % c.D];
            } else {
                s.t[row * 2 * c.n + c.n + j] = sinf(v);
            }
        }
        su += on ? li : 0.f;
        __syncthreads();
    }
    su = wave_sum(su);
    if (h == 0 && lane == 0) s.lad_u[row] = su;
}

// density_fwd_row on a wave pair: wave 0 the conditional spline of the transform half,
// wave 1 the unconditional one of the identity half; the log-det sums meet in red
template <class B>
__device__ __forceinline__ float density_fwd_row2(B bins, const CouplingArgs &c, const DensityFwdArgs &d, int64_t row,
                                                  float *rb, float *red, int h) {
    const int lane = threadIdx.x & 63, K = bins.k();
    const float *xr = d.x + row * c.D;
    float sl = 0.f;
    for (int j = lane; j < c.n; j += 64) {
        if (h == 0) {
            const int pt = (int)c.tr[j];
            const float xt = xr[pt];
            float yt = xt, lt = 0.f;
            if (xt >= -c.bound && xt <= c.bound) {
                const float *p = d.params + (row * c.n + j) * (3 * K + 1);
                float w[B::cap], hh[B::cap];
                cond_params(bins, p, c.sq, w, hh);
                rqs_point<false>(bins, xt, w, hh, p + 2 * K, c.bound, yt, lt, nullptr);
            }
            d.out[row * c.D + (pt + c.D - c.split) % c.D] = yt;
            rb[(pt + c.D - c.split) % c.D] = yt;
            sl += lt;
        } else {
            const int pi = (int)c.id[j];
            const float xi = xr[pi];
            float yi = xi, li = 0.f;
            if (xi >= -c.bound && xi <= c.bound)
                rqs_point<false>(bins, xi, d.uw + j * K, d.uh + j * K, d.ud + j * (K + 1), c.bound, yi, li, nullptr);
            d.out[row * c.D + (pi + c.D - c.split) % c.D] = yi;
            rb[(pi + c.D - c.split) % c.D] = yi;
            sl += li;
        }
    }
    sl = wave_sum(sl);
    if (h == 1 && lane == 0) red[0] = sl;
    return sl;
}

template <int KT>
__global__ __launch_bounds__(128) void coupling_pair_step2_kernel(CouplingArgs cs, SamplePostArgs s, CouplingArgs cs2,
                                                                  SamplePreArgs s2, CouplingArgs cd, DensityFwdArgs d,
                                                                  CouplingArgs cd2, float *t_d2, unsigned nb0) {
    const Bins<KT> bins{cs.K};
    __shared__ float rb[kCplMaxD];
    __shared__ float kx[2 * (Bins<KT>::cap + 1) * 64];
    __shared__ float red[1];
    const int h = (int)(threadIdx.x >> 6);
    const bool dens = blockIdx.x >= nb0;
    const int64_t row = (int64_t)(dens ? blockIdx.x - nb0 : blockIdx.x);
    if (!dens) {
        if (row >= cs.rows) return;  // whole workgroup: no barrier is left waiting
        sample_post_row2(bins, cs, s, row, rb, kx, h);
        __syncthreads();  // the row in LDS
        sample_pre_row2(bins, cs2, s2, row, rb, kx, h);
        return;
    }
    if (row >= cd.rows) return;
    const float sl = density_fwd_row2(bins, cd, d, row, rb, red, h);
    __syncthreads();  // the row in LDS, the unconditional log-det sum in red
    const int lane = threadIdx.x & 63;
    if (h == 0 && lane == 0) d.lq_out[row] = (d.lq_in ? d.lq_in[row] : 0.f) + (sl + red[0]);  // density_fwd_row's order
    for (int j = lane; j < cd2.n; j += 64) {  // features_row, cosines on wave 0, sines on wave 1
        const float v = cd2.scale * rb[cd2.id[j]];
        if (h == 0)
            t_d2[row * 2 * cd2.n + j] = cosf(v);
        else
            t_d2[row * 2 * cd2.n + cd2.n + j] = sinf(v);
    }
}

// density_bwd_row on four waves: part = wave >> 1 (0: the conditional spline's adjoints,
// 1: the unconditional one's, as in density_bwd_row), h = wave & 1 the knot set it builds
// and back-propagates (0 widths, 1 heights); the core adjoints are computed by both waves
// of a part from the swapped knots
template <class B>
__device__ __forceinline__ void density_bwd_row4(B bins, const CouplingArgs &c, const float *__restrict__ x,
                                                 const float *__restrict__ params, const float *__restrict__ uw,
                                                 const float *__restrict__ uh, const float *__restrict__ ud,
                                                 const float *gor, const float *__restrict__ g_lq, float *gx,
                                                 float *g_params, float *g_u, int64_t row, float *kx) {
    const int lane = threadIdx.x & 63, wv = (int)(threadIdx.x >> 6), part = wv >> 1, h = wv & 1, K = bins.k();
    const float *xr = x + row * c.D;
    const float gl = g_lq ? g_lq[row] : 0.f;
    const int P = 3 * K + 1;
    for (int j0 = 0; j0 < c.n; j0 += 64) {
        const int j = j0 + lane;
        const bool on = j < c.n;
        const int jj = on ? j : 0;
        const int pi = (int)c.id[jj], pt = (int)c.tr[jj];
        const int pos = part == 0 ? pt : pi;
        const float xv = xr[pos];
        const float go = gor ? gor[(pos + c.D - c.split) % c.D] : 0.f;
        const float *p = params + (row * c.n + jj) * P;
        Knots<B> kn;
        if (part == 0) {
            float u[B::cap];
            FS_BINS_FOR(k, K, u[k] = p[h * K + k] / c.sq;)  // cond_params' half
            build_knots(bins, u, c.bound, kn);
        } else {
            build_knots(bins, (h == 0 ? uw : uh) + jj * K, c.bound, kn);
        }
        float wc[B::cap + 1], hc[B::cap + 1];
        knots_pair(bins, kx, wv, h, kn.c, wc, hc);
        const bool inside = xv >= -c.bound && xv <= c.bound;
        float *gp = g_params + (row * c.n + jj) * P;
        // g_u row: [uw n*K | uh n*K | ud n*(K+1)], the parameters' own layouts back to back
        float *guw = g_u + row * c.n * P + jj * K;
        float *guh = guw + c.n * K;
        float *gud = g_u + row * c.n * P + 2 * c.n * K + jj * (K + 1);
        // each wave stores its knot set's parameter adjoints and, on h == 0, gx and the derivative
        // logits' adjoints.  The stores keep the shape each policy had as a separate copy
        if constexpr (B::fixed) {
            if (on && inside) {
                float g, gd[B::cap + 1], gk[B::cap];
                const BinAdjoint a = rqs_bwd_core<false>(bins, xv, wc, hc, part == 0 ? p + 2 * K : ud + jj * (K + 1),
                                                         go, gl, g, gd);
                knots_backward(bins, kn, a.b, h == 0 ? a.gw0 : a.gh0, h == 0 ? a.gw1 : a.gh1, c.bound, gk);
                if (part == 0) {
#pragma unroll
                    for (int k = 0; k < K; ++k) gp[h * K + k] = gk[k] / c.sq;
                    if (h == 0) {
                        gx[row * c.D + pt] = g;
#pragma unroll
                        for (int k = 0; k <= K; ++k) gp[2 * K + k] = gd[k];
                    }
                } else {
                    float *gu = h == 0 ? guw : guh;
#pragma unroll
                    for (int k = 0; k < K; ++k) gu[k] = gk[k];
                    if (h == 0) {
                        gx[row * c.D + pi] = g;
#pragma unroll
                        for (int k = 0; k <= K; ++k) gud[k] = gd[k];
                    }
                }
            } else if (on) {
                if (part == 0) {
#pragma unroll
                    for (int k = 0; k < K; ++k) gp[h * K + k] = 0.f;
                    if (h == 0) {
                        gx[row * c.D + pt] = go;
#pragma unroll
                        for (int k = 0; k <= K; ++k) gp[2 * K + k] = 0.f;
                    }
                } else {
                    float *gu = h == 0 ? guw : guh;
#pragma unroll
                    for (int k = 0; k < K; ++k) gu[k] = 0.f;
                    if (h == 0) {
                        gx[row * c.D + pi] = go;
#pragma unroll
                        for (int k = 0; k <= K; ++k) gud[k] = 0.f;
                    }
                }
            }
        } else {
            float *gk_out = part == 0 ? gp + h * K : (h == 0 ? guw : guh);
            float *gd_out = part == 0 ? gp + 2 * K : gud;
            if (on && inside) {
                float g, gd[B::cap + 1], gk[B::cap];
                const BinAdjoint a = rqs_bwd_core<false>(bins, xv, wc, hc, part == 0 ? p + 2 * K : ud + jj * (K + 1),
                                                         go, gl, g, gd);
                knots_backward(bins, kn, a.b, h == 0 ? a.gw0 : a.gh0, h == 0 ? a.gw1 : a.gh1, c.bound, gk);
                for (int k = 0; k < K; ++k) gk_out[k] = part == 0 ? gk[k] / c.sq : gk[k];
                if (h == 0) {
                    gx[row * c.D + pos] = g;
                    for (int k = 0; k <= K; ++k) gd_out[k] = gd[k];
                }
            } else if (on) {
                for (int k = 0; k < K; ++k) gk_out[k] = 0.f;
                if (h == 0) {
                    gx[row * c.D + pos] = go;
                    for (int k = 0; k <= K; ++k) gd_out[k] = 0.f;
                }
            }
        }
        __syncthreads();  // the partners have read this round's knots
    }
}

template <int KT>
__global__ __launch_bounds__(256) void coupling_bwd_step4_kernel(CouplingArgs cf, const float *__restrict__ xf,
                                                                 const float *__restrict__ g_t, float *gxf,
                                                                 const float *__restrict__ gx_add, CouplingArgs c,
                                                                 const float *__restrict__ x,
                                                                 const float *__restrict__ params,
                                                                 const float *__restrict__ uw,
                                                                 const float *__restrict__ uh,
                                                                 const float *__restrict__ ud,
                                                                 const float *__restrict__ g_lq, float *gx,
                                                                 float *g_params, float *g_u) {
    __shared__ float rb[kCplMaxDB];
    __shared__ float kx[4 * (Bins<KT>::cap + 1) * 64];
    const int64_t row = blockIdx.x;
    if (row >= c.rows) return;  // whole workgroup
    if (threadIdx.x < 64) features_bwd_row(cf, xf, g_t, gxf, gx_add, row, rb);
    __syncthreads();
    density_bwd_row4(Bins<KT>{c.K}, c, x, params, uw, uh, ud, rb, g_lq, gx, g_params, g_u, row, kx);
}

// ---------------------------------------------------------------------------
// Adjoints of the sampling direction (Coupling.inverse, coupling.py:104-134; reverse_kld,
// core.py:105-142), in two launches around the conditioner's backward.  One wave per row,
// lane = feature j (j += 64), as the forward kernels.  With zi = z[(id_j + split) % D],
// yi = uinv(zi), t = [cos(s yi), sin(s yi)], params = C(t), xt = z[(tr_j + split) % D],
// yt = cinv(xt; params) and lq_out = lq_in - (sum li + sum lt):
//   bwd_post (before the conditioner's backward): the conditional inverse spline's adjoints
//     from g_out at the transform positions and -g_lq: gz at (tr_j + split) % D and
//     g_params [rows][n][3K+1] (widths and heights / sq), density_bwd_row's layout;
//   bwd_pre (after it): g_yi = g_out at the identity position + the features' adjoint
//     (features_bwd_row's expression on yi = out[id_j]), then the unconditional inverse
//     spline's adjoints: gz at (id_j + split) % D and the per-row g_u [uw | uh | ud].
// The two write disjoint halves of gz (nullable: the input needs no gradient).  gor: the
// row of g_out (nullable = 0).  xt is read from the layer input z: post overwrote it in out.
struct SampleBwdPostArgs {
    const float *z, *params, *g_lq;
    float *gz, *g_params;
};

struct SampleBwdPreArgs {
    const float *z, *out, *uw, *uh, *ud, *g_t, *g_lq;
    float *gz, *g_u;
};

template <class B>
__device__ __forceinline__ void sample_bwd_post_row(B bins, const CouplingArgs &c, const SampleBwdPostArgs &s,
                                                    const float *gor, int64_t row) {
    const int lane = threadIdx.x & 63, K = bins.k();
    const float *zr = s.z + row * c.D;
    const float gl = s.g_lq ? -s.g_lq[row] : 0.f;  // lq_out = lq_in - (... + lt)
    const int P = 3 * K + 1;
    for (int j = lane; j < c.n; j += 64) {
        const int pt = (int)c.tr[j];
        const int qt = (pt + c.split) % c.D;
        const float xt = zr[qt];
        const float got = gor ? gor[pt] : 0.f;
        float *gp = s.g_params + (row * c.n + j) * P;
        float g = got;
        if (xt >= -c.bound && xt <= c.bound) {
            const float *p = s.params + (row * c.n + j) * P;
            float w[B::cap], h[B::cap], gw[B::cap], gh[B::cap], gd[B::cap + 1];
            cond_params(bins, p, c.sq, w, h);
            rqs_point_bwd<true>(bins, xt, w, h, p + 2 * K, c.bound, got, gl, g, gw, gh, adj_dst<B>(gd, gp + 2 * K));
            FS_BINS_FOR(k, K, gp[k] = gw[k] / c.sq; gp[K + k] = gh[k] / c.sq;)
            if constexpr (B::fixed) FS_BINS_FOR(k, K + 1, gp[2 * K + k] = gd[k];)
        } else {
            FS_BINS_FOR(k, P, gp[k] = 0.f;)
        }
        if (s.gz) s.gz[row * c.D + qt] = g;
    }
}

// rb (the fused launch): the row's whole gz, this half as computed and the other half as
// this layer's bwd_post launch wrote it (s.gz is not null then)
template <class B>
__device__ __forceinline__ void sample_bwd_pre_row(B bins, const CouplingArgs &c, const SampleBwdPreArgs &s,
                                                   const float *gor, int64_t row, float *rb = nullptr) {
    const int lane = threadIdx.x & 63, K = bins.k();
    const float *zr = s.z + row * c.D;
    const float gl = s.g_lq ? -s.g_lq[row] : 0.f;  // lq_out = lq_in - (li + ...)
    const int P = 3 * K + 1;
    for (int j = lane; j < c.n; j += 64) {
        const int pi = (int)c.id[j];
        const int qi = (pi + c.split) % c.D;
        const float zi = zr[qi];
        const float v = c.scale * s.out[row * c.D + pi];
        const float gc = s.g_t[row * 2 * c.n + j] * -sinf(v), gs = s.g_t[row * 2 * c.n + c.n + j] * cosf(v);
        const float gyi = (gc * c.scale + gs * c.scale) + (gor ? gor[pi] : 0.f);
        // g_u row: [uw n*K | uh n*K | ud n*(K+1)], the parameters' own layouts back to back
        float *guw = s.g_u + row * c.n * P + j * K;
        float *guh = guw + c.n * K;
        float *gud = s.g_u + row * c.n * P + 2 * c.n * K + j * (K + 1);
        float g = gyi;
        if (zi >= -c.bound && zi <= c.bound) {
            float gw[B::cap], gh[B::cap], gd[B::cap + 1];
            rqs_point_bwd<true>(bins, zi, s.uw + j * K, s.uh + j * K, s.ud + j * (K + 1), c.bound, gyi, gl, g,
                                 adj_dst<B>(gw, guw), adj_dst<B>(gh, guh), adj_dst<B>(gd, gud));
            if constexpr (B::fixed) {
                FS_BINS_FOR(k, K, guw[k] = gw[k]; guh[k] = gh[k];)
                FS_BINS_FOR(k, K + 1, gud[k] = gd[k];)
            }
        } else {
            FS_BINS_FOR(k, K, guw[k] = 0.f; guh[k] = 0.f;)
            FS_BINS_FOR(k, K + 1, gud[k] = 0.f;)
        }
        if (s.gz) s.gz[row * c.D + qi] = g;
        if (rb) {
            const int qt = ((int)c.tr[j] + c.split) % c.D;
            rb[qi] = g;
            rb[qt] = s.gz[row * c.D + qt];
        }
    }
}

template <int KT>
__global__ __launch_bounds__(256) void coupling_sample_bwd_post_kernel(CouplingArgs c, SampleBwdPostArgs s,
                                                                       const float *__restrict__ g_out) {
    const int64_t row = (int64_t)blockIdx.x * kCplRows + (threadIdx.x >> 6);
    if (row < c.rows) sample_bwd_post_row(Bins<KT>{c.K}, c, s, g_out ? g_out + row * c.D : nullptr, row);
}

template <int KT>
__global__ __launch_bounds__(256) void coupling_sample_bwd_pre_kernel(CouplingArgs c, SampleBwdPreArgs s,
                                                                      const float *__restrict__ g_out) {
    const int64_t row = (int64_t)blockIdx.x * kCplRows + (threadIdx.x >> 6);
    if (row < c.rows) sample_bwd_pre_row(Bins<KT>{c.K}, c, s, g_out ? g_out + row * c.D : nullptr, row);
}

// The backward between two layers of the sampling pass in one launch
// (fs_coupling_sample_bwd_step): layer l's bwd_pre, whose row of gz (kept in LDS, and written
// out) is the output gradient of layer l - 1, then layer l - 1's bwd_post on that row, each
// exactly as the two launches compute it.
template <int KT>
__global__ __launch_bounds__(256) void coupling_sample_bwd_step_kernel(CouplingArgs c, SampleBwdPreArgs s,
                                                                       const float *__restrict__ g_out,
                                                                       CouplingArgs cp, SampleBwdPostArgs sp) {
    const Bins<KT> bins{c.K};
    __shared__ float rbuf[kCplRows][kCplMaxDB];
    float *rb = rbuf[threadIdx.x >> 6];
    const int64_t row = (int64_t)blockIdx.x * kCplRows + (threadIdx.x >> 6);
    const bool live = row < c.rows;
    if (live) sample_bwd_pre_row(bins, c, s, g_out ? g_out + row * c.D : nullptr, row, rb);
    __syncthreads();
    if (live) sample_bwd_post_row(bins, cp, sp, rb, row);
}
#undef FS_BINS_FOR

}  // namespace fs

using namespace fs;

// launch(Bins<KT>{}) with the bin-count policy of (K, any_k): Bins<0> with any_k (K in the run-time
// kernels' range; capi.cpp checks it with a message), else the instantiation for K;
// hipErrorInvalidValue where there is none
template <class F>
static hipError_t with_bins(int K, bool any_k, F launch) {
    if (any_k) {
        if (K < 1 || K > kAnyMaxK) return hipErrorInvalidValue;
        launch(Bins<0>{});
    } else {
        switch (K) {
        case 5: launch(Bins<5>{}); break;
        case 8: launch(Bins<8>{}); break;
        case 15: launch(Bins<15>{}); break;
        case 32: launch(Bins<32>{}); break;
        default: return hipErrorInvalidValue;
        }
    }
    return hipGetLastError();
}
#define FS_KT decltype(bins)::kt  // inside with_bins' launch(auto bins)

static hipError_t rqs_forward_launch(bool any_k, int64_t M, int K, int inverse, const float *x, const float *uw,
                                     const float *uh, const float *ud, float B, float *out, float *lad,
                                     int32_t *nan_flag, hipStream_t st) {
    if (M <= 0) return hipSuccess;
    const dim3 grid((unsigned)((M + 255) / 256)), block(256);
    return with_bins(K, any_k, [&](auto bins) {
        if (inverse)
            hipLaunchKernelGGL((rqs_forward_kernel<FS_KT, true>), grid, block, 0, st, M, x, uw, uh, ud, B, out, lad,
                               nan_flag, K);
        else
            hipLaunchKernelGGL((rqs_forward_kernel<FS_KT, false>), grid, block, 0, st, M, x, uw, uh, ud, B, out, lad,
                               nan_flag, K);
    });
}

static hipError_t rqs_backward_launch(bool any_k, int64_t M, int K, int inverse, const float *x, const float *uw,
                                      const float *uh, const float *ud, float B, const float *g_out,
                                      const float *g_lad, float *gx, float *guw, float *guh, float *gud,
                                      hipStream_t st) {
    if (M <= 0) return hipSuccess;
    const dim3 grid((unsigned)((M + 255) / 256)), block(256);
    return with_bins(K, any_k, [&](auto bins) {
        if (inverse)
            hipLaunchKernelGGL((rqs_backward_kernel<FS_KT, true>), grid, block, 0, st, M, x, uw, uh, ud, B, g_out,
                               g_lad, gx, guw, guh, gud, K);
        else
            hipLaunchKernelGGL((rqs_backward_kernel<FS_KT, false>), grid, block, 0, st, M, x, uw, uh, ud, B, g_out,
                               g_lad, gx, guw, guh, gud, K);
    });
}

hipError_t fs_rqs_forward_impl(int64_t M, int K, int inverse, const float *x, const float *uw, const float *uh,
                               const float *ud, float B, float *out, float *lad, int32_t *nan_flag,
                               hipStream_t st) {
    return rqs_forward_launch(false, M, K, inverse, x, uw, uh, ud, B, out, lad, nan_flag, st);
}

hipError_t fs_rqs_backward_impl(int64_t M, int K, int inverse, const float *x, const float *uw, const float *uh,
                                const float *ud, float B, const float *g_out, const float *g_lad, float *gx,
                                float *guw, float *guh, float *gud, hipStream_t st) {
    return rqs_backward_launch(false, M, K, inverse, x, uw, uh, ud, B, g_out, g_lad, gx, guw, guh, gud, st);
}

hipError_t fs_rqs_forward_any_impl(int64_t M, int K, int inverse, const float *x, const float *uw, const float *uh,
                                   const float *ud, float B, float *out, float *lad, int32_t *nan_flag,
                                   hipStream_t st) {
    return rqs_forward_launch(true, M, K, inverse, x, uw, uh, ud, B, out, lad, nan_flag, st);
}

hipError_t fs_rqs_backward_any_impl(int64_t M, int K, int inverse, const float *x, const float *uw, const float *uh,
                                    const float *ud, float B, const float *g_out, const float *g_lad, float *gx,
                                    float *guw, float *guh, float *gud, hipStream_t st) {
    return rqs_backward_launch(true, M, K, inverse, x, uw, uh, ud, B, g_out, g_lad, gx, guw, guh, gud, st);
}

// the training step's coupling launches on two / four waves per row (1, default, or
// FS_COUPLING_WAVES / fs_set_coupling_waves) or one / two (0); bit-identical either way
static std::atomic<int> g_cpl_waves{-1};
static bool coupling_waves() {
    int v = g_cpl_waves.load(std::memory_order_relaxed);
    if (v < 0) {
        const char *e = getenv("FS_COUPLING_WAVES");
        int expect = -1;
        g_cpl_waves.compare_exchange_strong(expect, (e && e[0] == '0') ? 0 : 1);
        v = g_cpl_waves.load(std::memory_order_relaxed);
    }
    return v != 0;
}

int32_t fs_set_coupling_waves_impl(int32_t on) {
    const int32_t prev = coupling_waves() ? 1 : 0;
    if (on >= 0) g_cpl_waves.store(on ? 1 : 0, std::memory_order_relaxed);
    return prev;
}

static fs::CouplingArgs coupling_args(const fs_coupling *c) {
    fs::CouplingArgs a;
    a.rows = c->rows;
    a.D = c->D;
    a.n = c->D / 2;
    a.split = c->D / 2;
    a.id = c->identity_features;
    a.tr = c->transform_features;
    a.bound = (float)c->tail_bound;
    a.scale = (float)(M_PI / c->tail_bound);  // scale * ident with the Python-float scale (nn.py:133)
    a.sq = (float)sqrt((double)c->hidden);     // np.sqrt(num_hidden_channels) (coupling.py:340)
    a.K = c->K;
    return a;
}

// any_k descriptors: K in the Bins<0> kernels' range (capi.cpp checks it with a message)
static bool any_k_ok(const fs_coupling *c) { return c->K >= 1 && c->K <= kAnyMaxK; }

// with descriptor c's bin-count policy
template <class F>
static hipError_t with_bins(const fs_coupling *c, F launch) {
    return with_bins(c->K, c->any_k != 0, launch);
}

// one wave per row (an any_k descriptor's K is refused before the 0-row return, an
// uninstantiated K after it)
#define FS_COUPLING_LAUNCH(KERNEL, ...)                                                                    \
    const fs::CouplingArgs a = coupling_args(cp);                                                          \
    if (cp->any_k && !any_k_ok(cp)) return hipErrorInvalidValue;                                           \
    if (a.rows <= 0) return hipSuccess;                                                                    \
    const dim3 grid((unsigned)((a.rows + kCplRows - 1) / kCplRows)), block(64 * kCplRows);                 \
    return with_bins(cp, [&](auto bins) {                                                                  \
        hipLaunchKernelGGL((KERNEL##_kernel<FS_KT>), grid, block, 0, st, a, __VA_ARGS__);                  \
    });

hipError_t fs_coupling_density_fwd_impl(const fs_coupling *cp, const float *x, const float *params, const float *uw,
                                        const float *uh, const float *ud, const float *lq_in, float *out, float *lq_out,
                                        hipStream_t st) {
    const DensityFwdArgs d{x, params, uw, uh, ud, lq_in, out, lq_out};
    FS_COUPLING_LAUNCH(coupling_density_fwd, d)
}

hipError_t fs_coupling_density_bwd_impl(const fs_coupling *cp, const float *x, const float *params, const float *uw,
                                        const float *uh, const float *ud, const float *g_out, const float *g_lq,
                                        float *gx, float *g_params, float *g_u, hipStream_t st) {
    static_assert(2 * kCplRows <= 4, "launch bounds: two waves per row");
    const fs::CouplingArgs a = coupling_args(cp);
    if (a.rows <= 0) return hipSuccess;
    const unsigned grid = (unsigned)((a.rows + kCplRows - 1) / kCplRows);
    return with_bins(cp, [&](auto bins) {
        hipLaunchKernelGGL(coupling_density_bwd_kernel<FS_KT>, dim3(grid), dim3(128 * kCplRows), 0, st, a, x, params, uw,
                           uh, ud, g_out, g_lq, gx, g_params, g_u);
    });
}

hipError_t fs_coupling_bwd_step_impl(const fs_coupling *fp, const float *xf, const float *g_t, float *gxf,
                                     const float *gx_add, const fs_coupling *cp, const float *x, const float *params,
                                     const float *uw, const float *uh, const float *ud, const float *g_lq, float *gx,
                                     float *g_params, float *g_u, hipStream_t st) {
    const fs::CouplingArgs af = coupling_args(fp), a = coupling_args(cp);
    if (af.rows != a.rows || af.D != a.D || a.D > kCplMaxDB) return hipErrorInvalidValue;
    if (a.rows <= 0) return hipSuccess;
    const unsigned grid = (unsigned)((a.rows + kCplRows - 1) / kCplRows);
    const bool four = coupling_waves() && a.rows <= 0x7fffffff;
    return with_bins(cp, [&](auto bins) {
        if (four)
            hipLaunchKernelGGL(coupling_bwd_step4_kernel<FS_KT>, dim3((unsigned)a.rows), dim3(256), 0, st, af, xf, g_t,
                               gxf, gx_add, a, x, params, uw, uh, ud, g_lq, gx, g_params, g_u);
        else
            hipLaunchKernelGGL(coupling_bwd_step_kernel<FS_KT>, dim3(grid), dim3(128 * kCplRows), 0, st, af, xf, g_t,
                               gxf, gx_add, a, x, params, uw, uh, ud, g_lq, gx, g_params, g_u);
    });
}

hipError_t fs_coupling_sample_pre_impl(const fs_coupling *cp, const float *z, const float *uw, const float *uh,
                                       const float *ud, float *t, float *out, float *lad_u, int32_t *nan_flag,
                                       hipStream_t st) {
    const SamplePreArgs s{z, uw, uh, ud, t, out, lad_u, nan_flag};
    FS_COUPLING_LAUNCH(coupling_sample_pre, s)
}

hipError_t fs_coupling_sample_post_impl(const fs_coupling *cp, const float *params, const float *lad_u,
                                        const float *lq_in, float *out, float *lq_out, int32_t *nan_flag,
                                        hipStream_t st) {
    const SamplePostArgs s{params, lad_u, lq_in, out, lq_out, nan_flag};
    FS_COUPLING_LAUNCH(coupling_sample_post, s)
}

hipError_t fs_coupling_sample_bwd_post_impl(const fs_coupling *cp, const float *z, const float *params,
                                            const float *g_out, const float *g_lq, float *gz, float *g_params,
                                            hipStream_t st) {
    const SampleBwdPostArgs s{z, params, g_lq, gz, g_params};
    FS_COUPLING_LAUNCH(coupling_sample_bwd_post, s, g_out)
}

hipError_t fs_coupling_sample_bwd_pre_impl(const fs_coupling *cp, const float *z, const float *out, const float *uw,
                                           const float *uh, const float *ud, const float *g_t, const float *g_out,
                                           const float *g_lq, float *gz, float *g_u, hipStream_t st) {
    const SampleBwdPreArgs s{z, out, uw, uh, ud, g_t, g_lq, gz, g_u};
    FS_COUPLING_LAUNCH(coupling_sample_bwd_pre, s, g_out)
}

// cp: layer l (bwd_pre), pp: layer l - 1 (bwd_post on the row of gz)
hipError_t fs_coupling_sample_bwd_step_impl(const fs_coupling *cp, const float *z, const float *out, const float *uw,
                                            const float *uh, const float *ud, const float *g_t, const float *g_out,
                                            const float *g_lq, float *gz, float *g_u, const fs_coupling *pp,
                                            const float *z_prev, const float *params_prev, const float *g_lq_prev,
                                            float *gz_prev, float *g_params_prev, hipStream_t st) {
    const fs::CouplingArgs ap = coupling_args(pp);
    if (ap.rows != cp->rows || ap.D != cp->D || ap.D > kCplMaxDB || pp->K != cp->K || !pp->any_k != !cp->any_k || !gz)
        return hipErrorInvalidValue;
    const SampleBwdPreArgs s{z, out, uw, uh, ud, g_t, g_lq, gz, g_u};
    const SampleBwdPostArgs sp{z_prev, params_prev, g_lq_prev, gz_prev, g_params_prev};
    FS_COUPLING_LAUNCH(coupling_sample_bwd_step, s, g_out, ap, sp)
}
#undef FS_COUPLING_LAUNCH

// the sampling layer's rows on workgroups [0, nb0), the density layer's after them; WAVES per
// row, kCplRows rows per workgroup (one in the two-wave kernel)
#define FS_PAIR_LAUNCH(KERNEL, WAVES, ...)                                                                     \
    const fs::CouplingArgs as = coupling_args(sp), ad = coupling_args(dp);                                     \
    if (sp->K != dp->K || !sp->any_k != !dp->any_k || as.rows < 0 || ad.rows < 0) return hipErrorInvalidValue; \
    if (sp->any_k && !any_k_ok(sp)) return hipErrorInvalidValue;                                               \
    constexpr int wg_rows = WAVES == 1 ? kCplRows : 1;                                                         \
    const unsigned nb0 = (unsigned)((as.rows + wg_rows - 1) / wg_rows);                                        \
    const unsigned nb = nb0 + (unsigned)((ad.rows + wg_rows - 1) / wg_rows);                                   \
    if (nb == 0) return hipSuccess;                                                                            \
    return with_bins(sp, [&](auto bins) {                                                                      \
        hipLaunchKernelGGL((KERNEL##_kernel<FS_KT>), dim3(nb), dim3(64 * WAVES * wg_rows), 0, st, __VA_ARGS__, \
                           nb0);                                                                               \
    });

hipError_t fs_coupling_pair_pre_impl(const fs_coupling *sp, const float *z, const float *uw, const float *uh,
                                     const float *ud, float *t, float *out, float *lad_u, int32_t *nan_flag,
                                     const fs_coupling *dp, const float *x, float *td, hipStream_t st) {
    const SamplePreArgs s{z, uw, uh, ud, t, out, lad_u, nan_flag};
    FS_PAIR_LAUNCH(coupling_pair_pre, 1, as, s, ad, x, td)
}

hipError_t fs_coupling_pair_post_impl(const fs_coupling *sp, const float *params, const float *lad_u,
                                      const float *lq_in, float *out, float *lq_out, int32_t *nan_flag,
                                      const fs_coupling *dp, const float *x, const float *params_d, const float *uw,
                                      const float *uh, const float *ud, const float *lq_in_d, float *out_d,
                                      float *lq_out_d, hipStream_t st) {
    const SamplePostArgs s{params, lad_u, lq_in, out, lq_out, nan_flag};
    const DensityFwdArgs d{x, params_d, uw, uh, ud, lq_in_d, out_d, lq_out_d};
    FS_PAIR_LAUNCH(coupling_pair_post, 1, as, s, ad, d)
}

hipError_t fs_coupling_pair_step_impl(const fs_coupling *sp, const float *params, const float *lad_u,
                                      const float *lq_in, float *out, float *lq_out, int32_t *nan_flag,
                                      const fs_coupling *sp2, const float *uw2, const float *uh2, const float *ud2,
                                      float *t2, float *out2, float *lad_u2, const fs_coupling *dp, const float *x,
                                      const float *params_d, const float *uw, const float *uh, const float *ud,
                                      const float *lq_in_d, float *out_d, float *lq_out_d, const fs_coupling *dp2,
                                      float *t_d2, hipStream_t st) {
    const SamplePostArgs s{params, lad_u, lq_in, out, lq_out, nan_flag};
    const SamplePreArgs s2{out, uw2, uh2, ud2, t2, out2, lad_u2, nan_flag};
    const DensityFwdArgs d{x, params_d, uw, uh, ud, lq_in_d, out_d, lq_out_d};
    const fs::CouplingArgs as2 = coupling_args(sp2), ad2 = coupling_args(dp2);
    if (sp2->K != sp->K || as2.rows != sp->rows || ad2.rows != dp->rows || sp->D > kCplMaxD || dp->D > kCplMaxD ||
        sp2->D != sp->D || dp2->D != dp->D)
        return hipErrorInvalidValue;
    if (coupling_waves() && sp->rows + dp->rows <= 0x7fffffff) {  // one row per two-wave workgroup
        FS_PAIR_LAUNCH(coupling_pair_step2, 2, as, s, as2, s2, ad, d, ad2, t_d2)
    }
    FS_PAIR_LAUNCH(coupling_pair_step, 1, as, s, as2, s2, ad, d, ad2, t_d2)
}
#undef FS_PAIR_LAUNCH
#undef FS_KT

hipError_t fs_coupling_features_fwd_impl(const fs_coupling *cp, const float *x, float *t, hipStream_t st) {
    const fs::CouplingArgs a = coupling_args(cp);
    if (a.rows <= 0) return hipSuccess;
    hipLaunchKernelGGL(coupling_features_fwd_kernel, dim3((unsigned)((a.rows + kCplRows - 1) / kCplRows)), dim3(64 * kCplRows), 0, st, a, x, t);
    return hipGetLastError();
}

hipError_t fs_coupling_features_bwd_impl(const fs_coupling *cp, const float *x, const float *g_t, float *gx,
                                         const float *gx_add, hipStream_t st) {
    const fs::CouplingArgs a = coupling_args(cp);
    if (a.rows <= 0) return hipSuccess;
    hipLaunchKernelGGL(coupling_features_bwd_kernel, dim3((unsigned)((a.rows + kCplRows - 1) / kCplRows)), dim3(64 * kCplRows), 0, st, a, x, g_t,
                       gx, gx_add);
    return hipGetLastError();
}
