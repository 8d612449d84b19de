// General-shape flow pass (fs_flow_dims.precision = 4, "f32-general"): the coupling stack
// of flow_kernels.hip for ANY hidden width H <= 512 and bin count K <= 32 on one
// runtime-shaped kernel per pass mode, instead of one instantiation per (H, K) pair.
//
// Same structure as the instantiated kernel, with every shape a run-time value:
//   * one workgroup = 8 waves carries R chains (rows) through all L layers, coordinates
//     and activations in LDS, nothing in HBM between layers.  R = 64 while the padded
//     width Hp = 32 ceil(H / 32) is <= 256, else 32: the R x Hp trunk output is then at
//     most 16 32x32 tiles, two per wave, so the residual stream and a GEMM result stay in
//     the accumulator registers of the wave that owns their tiles (gen_rows);
//   * the conditioner runs as exact-f32 v_mfma_f32_32x32x2_f32 GEMMs.  H and the 2N input
//     features are zero-padded to multiples of 32 at pack time: a padded unit has zero
//     incoming and outgoing weights and zero epilogue vectors, so it contributes exact
//     zeros.  Eval BatchNorm is folded and the widths / heights carry log2(e) / sqrt(H)
//     with the TRUE H (fs_flow_pack_vec: the vector section and the unconditional knots
//     are the instantiated image's own);
//   * the final layer is never materialised: per transform feature, the widths and the
//     heights are one transposed 32-column tile each (lane = chain after
//     v_permlane32_swap), the two derivative logits the chain's bin needs are per-lane dot
//     products with gathered rows, then that feature's spline runs, one lane per chain
//     (rqs_eval, softplus_t and the double-precision knot normalisation of flow_device.h;
//     K is a loop bound against arrays of kMaxK).  With R = 32 the two lane halves of a
//     wave take two different features of the same 32 chains.
// A row's result depends on its own inputs only and every reduction has a fixed order,
// so it is bit-identical whatever the batch size and the row's position.  No host
// synchronisation, no allocation, no global scratch: capture-safe.  Small batches run the
// same pass phase by phase on 32-row tiles ("Wide path" below), bit-identical.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

#include <atomic>
#include <map>
#include <mutex>
#include <utility>

#include "flow_device.h"
#include "flow_layout.h"
#include "fs_internal.h"

namespace fs {

constexpr int kGenMaxH = 512;

// rows per workgroup: the trunk output [R][Hp] is at most 16 tiles of 32 x 32
FS_HD int gen_rows(int Hp) { return Hp <= 256 ? 64 : 32; }

// Packed image of one layer (offsets in floats).  GEMM operands are 1 KiB fragments
// [tile (32 output columns)][k-group (8 inputs)][lane][4]: lane l (c = l & 31, h = l >> 5)
// holds W[32 tile + c][8 g + 4 h + j], j = 0..3 (PackLayout's fragment, natural j order).
struct GenLayout {
    int Hp, kin_p;     // H and 2N padded to multiples of 32
    int kg_in, kg_h;   // k-groups of the initial layer / of an H-input layer (multiples of 4)
    int ct_h;          // column tiles of the trunk (Hp / 32)
    int rows;          // chains per workgroup
    int64_t win;       // [ct_h][kg_in] fragments
    int64_t blocks;    // nb x { W0 [ct_h][kg_h], W1 [ct_h][kg_h] }
    int64_t block_stride;
    int64_t wf;        // final layer, per feature: 2 tiles (widths, heights) x [kg_h]
    int64_t wd;        // final-layer derivative rows, per feature: [Hp / 4][K + 1][4]
    int64_t vec;       // PackLayout's vector section (pack_vec_kernel), true H
    int64_t v_blocks, v_bf, v_bd;
    int64_t unc;       // PackLayout's unconditional knots
    int64_t stride;
};

FS_HD GenLayout gen_layout(int N, int H, int nb, int K) {
    GenLayout g;
    const PackLayout p = pack_layout(N, H, nb, K);
    g.Hp = (int)rup(H, 32);
    g.kin_p = (int)rup(2 * N, 32);
    g.kg_in = g.kin_p / 8;
    g.kg_h = g.Hp / 8;
    g.ct_h = g.Hp / 32;
    g.rows = gen_rows(g.Hp);
    g.win = 0;
    g.blocks = g.win + (int64_t)g.ct_h * g.kg_in * 256;
    g.block_stride = 2 * (int64_t)g.ct_h * g.kg_h * 256;
    g.wf = g.blocks + nb * g.block_stride;
    g.wd = g.wf + (int64_t)N * 2 * g.kg_h * 256;
    g.vec = rup(g.wd + (int64_t)N * g.Hp * (K + 1), 64);
    g.v_blocks = p.v_blocks;
    g.v_bf = p.v_bf;
    g.v_bd = p.v_bd;
    g.unc = g.vec + (p.unc - p.vec);
    g.stride = rup(g.unc + (int64_t)N * 3 * (K + 1), 64);
    return g;
}

// LDS: activations [R][xs], coordinates [R][2N + 1], log-det partials [8 waves][64 lanes]
struct GenLds {
    int x, coord, ld, total;  // byte offsets
    int xs, cstride;
};

FS_HD GenLds gen_lds(int N, int Hp, int kin_p, int rows) {
    GenLds l;
    l.xs = (Hp > kin_p ? Hp : kin_p) + 4;  // + one 16-byte slot: conflict-free ds_read_b128 fragments
    l.cstride = 2 * N + 1;
    l.x = 0;
    l.coord = rows * l.xs * 4;
    l.ld = (int)rup(l.coord + rows * l.cstride * 4, 16);
    l.total = l.ld + kWaves * 64 * 4 + 16;
    return l;
}

// acc += X[32 rt .. 32 rt + 31][0 : 8 kg] . W[tile] (TR: the transposed tile, W^T . X^T:
// accumulator lane = chain, registers = output columns).  Wt: the tile's [kg][64][4]
// fragments; kg is a multiple of 4.  The fragments of the next four k-groups are loaded
// while the MFMAs of the current four run.
template <bool TR>
__device__ __forceinline__ void gen_gemm_tile(const float *__restrict__ X, int XS, const float *__restrict__ Wt, int kg,
                                              int rt, f32x16 &acc) {
    const int lane = threadIdx.x & 63;
    const int h = lane >> 5, r = lane & 31;
    const float *xa = X + (32 * rt + r) * XS + 4 * h;
    const f32x4 *wb = (const f32x4 *)Wt + lane;
    f32x4 b[4], bn[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) b[s] = bn[s] = wb[s * 64];
    for (int g0 = 0; g0 < kg; g0 += 4) {
        if (g0 + 4 < kg) {
#pragma unroll
            for (int s = 0; s < 4; ++s) bn[s] = wb[(g0 + 4 + s) * 64];
        }
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const f32x4 av = *(const f32x4 *)(xa + 8 * (g0 + s));
#pragma unroll
            for (int j = 0; j < 4; ++j)
                acc = TR ? __builtin_amdgcn_mfma_f32_32x32x2f32(b[s][j], av[j], acc, 0, 0, 0)
                         : __builtin_amdgcn_mfma_f32_32x32x2f32(av[j], b[s][j], acc, 0, 0, 0);
        }
#pragma unroll
        for (int s = 0; s < 4; ++s) b[s] = bn[s];
    }
}

#pragma clang fp contract(off)

// knots_from_logits (flow_device.h) with K a loop bound: the same operations in the same
// order on the first K logits; knots K..kMaxK are the upper bound
__device__ __forceinline__ void gen_knots(const float (&u)[kMaxK], float (&kn)[kMaxK + 1], int K, double minb,
                                          const FlowArgs &a) {
    float m = u[0];
#pragma unroll
    for (int k = 1; k < kMaxK; ++k)
        if (k < K) m = fmaxf(m, u[k]);
    float e[kMaxK];
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < kMaxK; ++k) {
        e[k] = 0.f;
        if (k < K) {  // logits carry log2(e) (folded at pack time)
            e[k] = __builtin_amdgcn_exp2f(u[k] - m);
            s += (double)e[k];
        }
    }
    const double sc = (1.0 - minb * (double)K) / s;
    double cs = 0.0;
    kn[0] = a.negB;
#pragma unroll
    for (int k = 0; k < kMaxK; ++k) {
        if (k < K - 1) {
            cs += __builtin_fma((double)e[k], sc, minb);
            kn[k + 1] = (float)__builtin_fma(a.twoBd, cs, -a.Bd);
        } else {
            kn[k + 1] = a.B;
        }
    }
}

// widths or heights logits of this lane's (chain, feature): the transposed tile of feature
// f0 on row tile 0 and of feature f1 on row tile rt1, biases preset in the accumulators,
// turned lane-per-chain.  Rows 64: f0 = f1, rt1 = 1 (lane = chain).  Rows 32: rt1 = 0,
// lanes 0..31 get feature f0 and lanes 32..63 feature f1 of chains 0..31.
__device__ __forceinline__ void gen_logits(const float *__restrict__ X, int XS, const float *__restrict__ Wf, int kg,
                                           const float *__restrict__ Bf, int f0, int f1, int rt1, int which,
                                           float (&u)[kMaxK]) {
    const int h = (threadIdx.x >> 5) & 1;
    const float *b0 = Bf + 96 * f0 + 32 * which, *b1 = Bf + 96 * f1 + 32 * which;
    f32x16 t0, t1;
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            t0[4 * g + j] = b0[8 * g + 4 * h + j];
            t1[4 * g + j] = b1[8 * g + 4 * h + j];
        }
    gen_gemm_tile<true>(X, XS, Wf + (int64_t)(2 * f0 + which) * kg * 256, kg, 0, t0);
    gen_gemm_tile<true>(X, XS, Wf + (int64_t)(2 * f1 + which) * kg * 256, kg, rt1, t1);
    lanes_to_chains(t0, t1);
#pragma unroll
    for (int k = 0; k < kMaxK; ++k) u[k] = tile_row(t0, t1, k);
}

// Final layer + conditional spline of one (chain, feature) per lane; inactive lanes
// (act = false: a feature index past N, clamped to N - 1 by the caller) only compute.
template <bool INV>
__device__ __forceinline__ float gen_cond_spline(const float *__restrict__ X, int XS, const float *__restrict__ P,
                                                 const GenLayout &GL, int f0, int f1, int rt1, int jl, bool act,
                                                 int chain, float *CO, int cs, int p, int K, const FlowArgs &a,
                                                 bool &nan_any) {
    const float *V = P + GL.vec;
    const float x = CO[chain * cs + p];
    const bool inside = (x >= a.negB) && (x <= a.B);
    constexpr int TS = INV ? 1 : 0;  // searched tile: 0 widths, 1 heights
    int bin = 0;
    float s0, s1, o0, o1;
    {
        float u[kMaxK], ks[kMaxK + 1];
        gen_logits(X, XS, P + GL.wf, GL.kg_h, V + GL.v_bf, f0, f1, rt1, TS, u);
        gen_knots(u, ks, K, INV ? kMinHd : kMinWd, a);
        // searchsorted (splines.py:11-13): the last k with x >= knot[k]
        s0 = ks[0];
        s1 = ks[1];
#pragma unroll
        for (int k = 1; k < kMaxK; ++k)
            if (k < K && x >= ks[k]) {
                bin = k;
                s0 = ks[k];
                s1 = ks[k + 1];
            }
    }
    {
        float u[kMaxK], ko[kMaxK + 1];
        gen_logits(X, XS, P + GL.wf, GL.kg_h, V + GL.v_bf, f0, f1, rt1, 1 - TS, u);
        gen_knots(u, ko, K, INV ? kMinWd : kMinHd, a);
        o0 = ko[0];
        o1 = ko[1];
#pragma unroll
        for (int k = 1; k < kMaxK; ++k)
            if (k == bin) {
                o0 = ko[k];
                o1 = ko[k + 1];
            }
    }
    // d_bin, d_bin+1 = bias + row . h over the padded hidden vector (rows bin, bin + 1 <= K
    // of the [Hp / 4][K + 1][4] section; the pad's weights are zero)
    const float *bd = V + GL.v_bd + jl * (K + 1);
    const f32x4 *wq = (const f32x4 *)(P + GL.wd) + (int64_t)jl * (GL.Hp / 4) * (K + 1) + bin;
    const float *xr = X + chain * XS;
    float ua = bd[bin], ub = bd[bin + 1], va = 0.f, vb = 0.f;
    for (int q = 0; q < GL.Hp / 4; q += 2) {
        const f32x4 ra0 = wq[(int64_t)q * (K + 1)], rb0 = wq[(int64_t)q * (K + 1) + 1];
        const f32x4 ra1 = wq[(int64_t)(q + 1) * (K + 1)], rb1 = wq[(int64_t)(q + 1) * (K + 1) + 1];
        const f32x4 h0 = *(const f32x4 *)(xr + 4 * q), h1 = *(const f32x4 *)(xr + 4 * q + 4);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            ua = fmaf(ra0[i], h0[i], ua);
            ub = fmaf(rb0[i], h0[i], ub);
            va = fmaf(ra1[i], h1[i], va);
            vb = fmaf(rb1[i], h1[i], vb);
        }
    }
    const float icw = INV ? o0 : s0, cw1 = INV ? o1 : s1;
    const float ich = INV ? s0 : o0, ch1 = INV ? s1 : o1;
    const float d0 = kMinD + softplus_t(ua + va);
    const float d1 = kMinD + softplus_t(ub + vb);
    float y, l;
    bool nd;
    rqs_eval<INV>(x, icw, cw1 - icw, ich, ch1 - ich, d0, d1, y, l, nd);
    if (inside && act) {
        CO[chain * cs + p] = y;
        nan_any |= nd;
        return l;
    }
    return 0.f;
}

// uncond_spline_w (flow_device.h) with K a loop bound; slot = this lane's first identity
// feature, step = features per round of the workgroup
template <bool INV>
__device__ __forceinline__ float gen_uncond_spline(const float *__restrict__ U, float *CO, int cs, int N, int D,
                                                   int off, int K, const FlowArgs &a, bool &nan_any, int slot,
                                                   int step, int chain) {
    const int K1 = K + 1;
    float ld = 0.f;
    for (int f = slot; f < N; f += step) {
        const float *T = U + (size_t)f * 3 * K1;
        const int p = (2 * f + off) % D;
        const float x = CO[chain * cs + p];
        const bool inside = (x >= a.negB) && (x <= a.B);
        const float *kn = INV ? T + K1 : T;
        int bin = -1;
        for (int k = 0; k < K; ++k) bin += (x >= kn[k]) ? 1 : 0;
        bin = bin < 0 ? 0 : (bin > K - 1 ? K - 1 : bin);
        const float icw = T[bin], cw1 = T[bin + 1];
        const float ich = T[K1 + bin], ch1 = T[K1 + bin + 1];
        const float d0 = T[2 * K1 + bin], d1 = T[2 * K1 + bin + 1];
        float y, l;
        bool nd;
        rqs_eval<INV>(x, icw, cw1 - icw, ich, ch1 - ich, d0, d1, y, l, nd);
        if (inside) {
            CO[chain * cs + p] = y;
            ld += l;
            nan_any |= nd;
        }
    }
    return ld;
}

#pragma clang fp contract(on)

template <int MODE>
__global__ void __launch_bounds__(kThreads) flow_general_kernel(FlowArgs a, int H) {
    constexpr bool INV = MODE != MODE_DENSITY;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int N = a.N, D = 2 * N, K = a.K;
    const GenLayout GL = gen_layout(N, H, a.nb, K);
    const int R = GL.rows;
    const GenLds LL = gen_lds(N, GL.Hp, GL.kin_p, R);
    const int XS = LL.xs, cs = LL.cstride;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int h = lane >> 5, r = lane & 31;
    float *X = (float *)(smem + LL.x);
    float *CO = (float *)(smem + LL.coord);
    float *LDP = (float *)(smem + LL.ld);
    const int64_t row0 = (int64_t)blockIdx.x * R;
    // spline phases: lane -> (chain, feature slot).  R = 64: lane = chain, one feature per
    // wave and round; R = 32: the lane halves take two features of chains 0..31
    const int S = 64 / R;
    const int chain = R == 64 ? lane : r;
    const int sub = R == 64 ? 0 : h;
    const bool row_valid = row0 + chain < a.nrows;
    // trunk: tile t = wid * tpw + s -> (column tile t / RT, row tile t % RT)
    const int RT = R / 32, NTt = RT * GL.ct_h;
    const int tpw = NTt > kWaves ? 2 : 1;
    bool tv[2];
    int tct[2], trt[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const int t = wid * tpw + s;
        tv[s] = s < tpw && t < NTt;
        tct[s] = tv[s] ? t / RT : 0;
        trt[s] = tv[s] ? t % RT : 0;
    }

    // ---- inputs -> CO (logical order == physical order at offset 0)
    if (MODE == MODE_PROPOSE) {
        const int nq = (D + 3) / 4;
        for (int e = tid; e < R * nq; e += kThreads) {
            const int rr = e / nq, q = e - rr * nq;
            // the instantiated kernels' Philox key (global chain, step)
            const int64_t lr = row0 + rr, rpc = a.rows_per_counter;
            const uint64_t ctr = rpc > 0 ? a.counter + (uint64_t)(lr / rpc) : a.counter;
            const uint64_t gr = (uint64_t)(a.row_offset + (rpc > 0 ? lr % rpc : lr));
            uint4 c = make_uint4((uint32_t)gr, (uint32_t)(gr >> 32) ^ (uint32_t)(ctr >> 32), (uint32_t)ctr,
                                 (uint32_t)q);
            uint4 o = philox4x32(c, make_uint2((uint32_t)a.seed, (uint32_t)(a.seed >> 32)));
            const uint32_t w[4] = {o.x, o.y, o.z, o.w};
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int i = 4 * q + t;
                if (i < D) {
                    const float u = (float)(w[t] >> 8) * 5.9604644775390625e-08f;  // [0,1)
                    CO[rr * cs + i] = u * a.twoB + a.negB;
                }
            }
        }
    } else {
        for (int e = tid; e < R * D; e += kThreads) {
            const int rr = e / D, i = e - rr * D;
            const int64_t gr = row0 + rr;
            CO[rr * cs + i] = (gr < a.nrows) ? a.in[gr * D + i] : 0.f;
        }
    }
    float ld = 0.f;
    bool nan_any = false;
    int off = 0;
    __syncthreads();

    for (int s = 0; s < a.L; ++s) {
        const int layer = (MODE == MODE_DENSITY) ? a.L - 1 - s : s;
        const float *P = a.packed + (int64_t)layer * GL.stride;
        const float *V = P + GL.vec;
        if (MODE != MODE_DENSITY) {
            off = (off + N) % D;  // Coupling.inverse rolls first (coupling.py:113-114)
            ld += gen_uncond_spline<true>(P + GL.unc, CO, cs, N, D, off, K, a, nan_any, wid * S + sub, kWaves * S,
                                          chain);
            __syncthreads();
        }
        // periodic features [cos(s x_id) | sin(s x_id)] (nn.py:120-137) -> X, zero pad to kin_p
        for (int e = tid; e < R * N; e += kThreads) {
            const int rr = e / N, f = e - rr * N;
            const float sv = a.scale_pf * CO[rr * cs + (2 * f + off) % D];
            X[rr * XS + f] = cosf(sv);
            X[rr * XS + N + f] = sinf(sv);
        }
        const int npad = GL.kin_p - D;
        for (int e = tid; e < R * npad; e += kThreads) {
            const int rr = e / npad, c = e - rr * npad;
            X[rr * XS + D + c] = 0.f;
        }
        __syncthreads();

        // ResidualNet: hr = the residual stream without its biases (deferred into the
        // folded epilogue vectors and s_h by pack_vec_kernel, as in flow_pass_kernel)
        f32x16 hr[2], acc[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
#pragma unroll
            for (int i = 0; i < 16; ++i) hr[t][i] = 0.f;
            if (tv[t])
                gen_gemm_tile<false>(X, XS, P + GL.win + (int64_t)tct[t] * GL.kg_in * 256, GL.kg_in, trt[t], hr[t]);
        }
        for (int jb = 0; jb < a.nb; ++jb) {  // ResidualBlock (resnet.py:37-50), eval BN folded
            const float *VB = V + GL.v_blocks + (int64_t)4 * H * jb;
            const float *W0 = P + GL.blocks + jb * GL.block_stride;
            const float *W1 = W0 + GL.block_stride / 2;
            __syncthreads();  // every wave has read X
#pragma unroll
            for (int t = 0; t < 2; ++t)
                if (tv[t]) {
                    const int col = 32 * tct[t] + r;
                    const bool on = col < H;
                    const float e0 = on ? VB[col] : 0.f, e1 = on ? VB[H + col] : 0.f;
#pragma unroll
                    for (int i = 0; i < 16; ++i)
                        X[acc_row(trt[t], i, h) * XS + col] = fmaxf(fmaf(hr[t][i], e0, e1), 0.f);
                }
            __syncthreads();
#pragma unroll
            for (int t = 0; t < 2; ++t) {
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[t][i] = 0.f;
                if (tv[t])
                    gen_gemm_tile<false>(X, XS, W0 + (int64_t)tct[t] * GL.kg_h * 256, GL.kg_h, trt[t], acc[t]);
            }
            __syncthreads();
#pragma unroll
            for (int t = 0; t < 2; ++t)
                if (tv[t]) {
                    const int col = 32 * tct[t] + r;
                    const bool on = col < H;
                    const float e2 = on ? VB[2 * H + col] : 0.f, e3 = on ? VB[3 * H + col] : 0.f;
#pragma unroll
                    for (int i = 0; i < 16; ++i)
                        X[acc_row(trt[t], i, h) * XS + col] = fmaxf(fmaf(acc[t][i], e2, e3), 0.f);
                }
            __syncthreads();
#pragma unroll
            for (int t = 0; t < 2; ++t)
                if (tv[t])  // h += Lin1(t)
                    gen_gemm_tile<false>(X, XS, W1 + (int64_t)tct[t] * GL.kg_h * 256, GL.kg_h, trt[t], hr[t]);
        }
        __syncthreads();
#pragma unroll
        for (int t = 0; t < 2; ++t)
            if (tv[t]) {  // X <- h (+ the deferred biases) for the final layer
                const int col = 32 * tct[t] + r;
                const float sh = col < H ? V[col] : 0.f;
#pragma unroll
                for (int i = 0; i < 16; ++i) X[acc_row(trt[t], i, h) * XS + col] = hr[t][i] + sh;
            }
        __syncthreads();

        // final layer + conditional spline, feature by feature
        for (int j0 = wid * S; j0 < N; j0 += kWaves * S) {
            const int f0 = j0;
            const int f1 = (S == 2 && j0 + 1 < N) ? j0 + 1 : j0;
            const int jraw = j0 + sub;
            const bool act = jraw < N;
            const int jl = act ? jraw : N - 1;
            ld += gen_cond_spline<INV>(X, XS, P, GL, f0, f1, S == 2 ? 0 : 1, jl, act, chain, CO, cs,
                                       (2 * jl + 1 + off) % D, K, a, nan_any);
        }
        if (MODE == MODE_DENSITY) {
            ld += gen_uncond_spline<false>(P + GL.unc, CO, cs, N, D, off, K, a, nan_any, wid * S + sub, kWaves * S,
                                           chain);
            off = (off + N) % D;  // Coupling.forward rolls last (coupling.py:100-101)
        }
        __syncthreads();
    }

    // ---- outputs: the 8 x S partials of a chain summed in slot order
    LDP[wid * 64 + lane] = ld;
    if (nan_any && row_valid && a.err) atomicOr(a.err, 1);
    __syncthreads();
    if (tid < R) {
        float tot = 0.f;
        for (int w = 0; w < kWaves; ++w)
            for (int q = 0; q < S; ++q) tot += LDP[w * 64 + q * R + tid];
        float outv = tot;
        if (MODE == MODE_DENSITY && a.add_base) {
            bool inb = true;
            for (int i = 0; i < D; ++i) {
                const float z = CO[tid * cs + i];
                inb = inb && (z >= a.negB) && (z <= a.B);
            }
            outv = tot + (inb ? a.base_lp : -INFINITY);
        }
        // single-pass log q (FS_MH_SINGLE_PASS): log q(x') = log q0(z) - sum log|dx/dz|
        if (MODE == MODE_PROPOSE && a.add_base) outv = a.base_lp - tot;
        if (row0 + tid < a.nrows && a.scalar_out) a.scalar_out[row0 + tid] = outv;
    }
    for (int e = tid; e < R * D; e += kThreads) {
        const int rr = e / D, i = e - rr * D;
        const int64_t gr = row0 + rr;
        if (gr >= a.nrows) continue;
        const float v = CO[rr * cs + (i + off) % D];
        if (a.out) a.out[gr * D + i] = v;
        if (MODE == MODE_PROPOSE) {
            const float cfg = v + a.B;  // a_ + HALF_BOX in float32 (main_algorithm_1.py:343)
            if (a.config) a.config[gr * D + i] = cfg;
            if (a.centered) a.centered[gr * D + i] = (float)((double)cfg - a.half_width);
        }
    }
}

// ---------------------------------------------------------------------------
// Wide path (small batches): the same pass phase by phase over the whole batch
// ---------------------------------------------------------------------------
// The fused kernel launches ceil(B / R) workgroups, 16 for a 1000-row batch at R = 64.
// The wide path runs each coupling layer as two launches over 32-row tiles (a trunk
// launch per tile, a final-layer launch per tile and group of kGenWideFeat transform
// features) and ends with an output launch, 2 L + 1 launches, with the coordinates, the
// trunk output and the log-det terms in a global workspace between them:
//   CO  [rows][2N]   coordinates (physical order; the half-roll stays the `off` argument)
//   X   [rows][Hp]   the trunk output h + s_h of the current layer
//   TC  [rows][N]    the current layer's conditional log-det terms, one per feature
//   TU  [rows][16]   (density) the current layer's unconditional slot sums
//   LDP [rows][16]   the fused kernel's per-(chain, slot) log-det partials
// Every value is computed by the fused kernel's own device functions on the same operands
// (an MFMA tile element depends on its own row and column only, the spline is per chain
// and feature), and the log-det is summed in the fused kernel's order: slot q = wid S + sub
// of a chain (S = 64 / gen_rows(Hp), the FLOW's S, not the 32-row tile's) accumulates
// from +0, layer by layer, the unconditional slot sum and the conditional terms of
// features q, q + 8 S, ...; the output launch adds the 8 S slots in slot order.  The
// fold of a layer's terms into LDP runs in the next trunk launch's prologue (the output
// launch for the last layer).  So the results are bit-identical to flow_general_kernel's.
constexpr int kGenWideRows = 32;       // rows per tile
constexpr int kGenWideSlots = 16;      // 8 S <= 16 log-det slots per chain
constexpr int kGenWideFinalWaves = 4;  // waves per final-launch workgroup
constexpr int kGenWideFeat = 2 * kGenWideFinalWaves;  // transform features per final-launch workgroup

struct GenWideArgs {
    FlowArgs a;
    float *CO, *X, *TC, *TU, *LDP;
    int H;
    int layer;  // packed layer of this launch
    int off;    // coordinate offset (half-roll) of this launch
    int first;  // first step of the pass: inputs instead of workspace coordinates, no fold
};

// LDP of (chain, slot) after folding in one layer's terms, in the fused kernel's order
template <bool INV>
__device__ __forceinline__ float gen_wide_fold(float p, const float *__restrict__ tc, const float *__restrict__ tu,
                                               int N, int slot, int step) {
    for (int j = slot; j < N; j += step) p += tc[j];
    if (!INV) p += tu[slot];
    return p;
}

template <int MODE>
__global__ void __launch_bounds__(kThreads) gen_wide_trunk_kernel(GenWideArgs w) {
    constexpr bool INV = MODE != MODE_DENSITY;
    constexpr int R = kGenWideRows;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const FlowArgs &a = w.a;
    const int N = a.N, D = 2 * N, K = a.K, H = w.H;
    const GenLayout GL = gen_layout(N, H, a.nb, K);
    const GenLds LL = gen_lds(N, GL.Hp, GL.kin_p, R);
    const int XS = LL.xs, cs = LL.cstride;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int h = lane >> 5, r = lane & 31;
    float *X = (float *)(smem + LL.x);
    float *CO = (float *)(smem + LL.coord);
    const int64_t row0 = (int64_t)blockIdx.x * R;
    // log-det slots of the flow's own fused arrangement: S = 2 (flow R = 32): the lane halves
    // are slots 2 wid, 2 wid + 1; S = 1 (flow R = 64): slot wid, on the lower lane half
    const int S = 64 / GL.rows;
    const int chain = r;
    const int slot = wid * S + (S == 2 ? h : 0), step = kWaves * S;
    const bool slot_on = S == 2 || h == 0;
    const bool row_valid = row0 + chain < a.nrows;
    // trunk: one row tile, column tile t = wid * tpw + s
    const int tpw = GL.ct_h > kWaves ? 2 : 1;
    bool tv[2];
    int tct[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const int t = wid * tpw + s;
        tv[s] = s < tpw && t < GL.ct_h;
        tct[s] = tv[s] ? t : 0;
    }

    // ---- coordinates -> CO: the pass inputs (flow_general_kernel's input phase) or the workspace
    if (w.first && MODE == MODE_PROPOSE) {
        const int nq = (D + 3) / 4;
        for (int e = tid; e < R * nq; e += kThreads) {
            const int rr = e / nq, q = e - rr * nq;
            const int64_t lr = row0 + rr, rpc = a.rows_per_counter;
            const uint64_t ctr = rpc > 0 ? a.counter + (uint64_t)(lr / rpc) : a.counter;
            const uint64_t gr = (uint64_t)(a.row_offset + (rpc > 0 ? lr % rpc : lr));
            uint4 c = make_uint4((uint32_t)gr, (uint32_t)(gr >> 32) ^ (uint32_t)(ctr >> 32), (uint32_t)ctr,
                                 (uint32_t)q);
            uint4 o = philox4x32(c, make_uint2((uint32_t)a.seed, (uint32_t)(a.seed >> 32)));
            const uint32_t u4[4] = {o.x, o.y, o.z, o.w};
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int i = 4 * q + t;
                if (i < D) {
                    const float u = (float)(u4[t] >> 8) * 5.9604644775390625e-08f;  // [0,1)
                    CO[rr * cs + i] = u * a.twoB + a.negB;
                }
            }
        }
    } else if (w.first) {
        for (int e = tid; e < R * D; e += kThreads) {
            const int rr = e / D, i = e - rr * D;
            const int64_t gr = row0 + rr;
            CO[rr * cs + i] = (gr < a.nrows) ? a.in[gr * D + i] : 0.f;
        }
    } else {
        for (int e = tid; e < R * D; e += kThreads) {
            const int rr = e / D, i = e - rr * D;
            CO[rr * cs + i] = w.CO[(row0 + rr) * D + i];
        }
    }
    bool nan_any = false;
    const int off = w.off;
    const float *P = a.packed + (int64_t)w.layer * GL.stride;
    const float *V = P + GL.vec;
    __syncthreads();

    // ---- log-det partial of (chain, slot): fold the previous layer, then (sampling
    // direction) this layer's unconditional spline on the identity features
    float ldp = 0.f;
    if (slot_on && !w.first)
        ldp = gen_wide_fold<INV>(w.LDP[(row0 + chain) * kGenWideSlots + slot], w.TC + (row0 + chain) * N,
                                 w.TU + (row0 + chain) * kGenWideSlots, N, slot, step);
    if (INV) {
        if (slot_on) ldp += gen_uncond_spline<true>(P + GL.unc, CO, cs, N, D, off, K, a, nan_any, slot, step, chain);
        __syncthreads();
    }
    if (slot_on) w.LDP[(row0 + chain) * kGenWideSlots + slot] = ldp;

    // periodic features -> X, zero pad to kin_p
    for (int e = tid; e < R * N; e += kThreads) {
        const int rr = e / N, f = e - rr * N;
        const float sv = a.scale_pf * CO[rr * cs + (2 * f + off) % D];
        X[rr * XS + f] = cosf(sv);
        X[rr * XS + N + f] = sinf(sv);
    }
    const int npad = GL.kin_p - D;
    for (int e = tid; e < R * npad; e += kThreads) {
        const int rr = e / npad, c = e - rr * npad;
        X[rr * XS + D + c] = 0.f;
    }
    __syncthreads();
    if (!INV) {
        // density direction: the layer's unconditional spline acts on the identity features
        // only, after the conditioner has read them; its slot sum is folded after the
        // layer's conditional terms
        if (slot_on)
            w.TU[(row0 + chain) * kGenWideSlots + slot] =
                gen_uncond_spline<false>(P + GL.unc, CO, cs, N, D, off, K, a, nan_any, slot, step, chain);
    }
    if (nan_any && row_valid && a.err) atomicOr(a.err, 1);

    // ResidualNet: flow_general_kernel's R = 32 arrangement
    f32x16 hr[2], acc[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
#pragma unroll
        for (int i = 0; i < 16; ++i) hr[t][i] = 0.f;
        if (tv[t]) gen_gemm_tile<false>(X, XS, P + GL.win + (int64_t)tct[t] * GL.kg_in * 256, GL.kg_in, 0, hr[t]);
    }
    for (int jb = 0; jb < a.nb; ++jb) {
        const float *VB = V + GL.v_blocks + (int64_t)4 * H * jb;
        const float *W0 = P + GL.blocks + jb * GL.block_stride;
        const float *W1 = W0 + GL.block_stride / 2;
        __syncthreads();  // every wave has read X
#pragma unroll
        for (int t = 0; t < 2; ++t)
            if (tv[t]) {
                const int col = 32 * tct[t] + r;
                const bool on = col < H;
                const float e0 = on ? VB[col] : 0.f, e1 = on ? VB[H + col] : 0.f;
#pragma unroll
                for (int i = 0; i < 16; ++i) X[acc_row(0, i, h) * XS + col] = fmaxf(fmaf(hr[t][i], e0, e1), 0.f);
            }
        __syncthreads();
#pragma unroll
        for (int t = 0; t < 2; ++t) {
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[t][i] = 0.f;
            if (tv[t]) gen_gemm_tile<false>(X, XS, W0 + (int64_t)tct[t] * GL.kg_h * 256, GL.kg_h, 0, acc[t]);
        }
        __syncthreads();
#pragma unroll
        for (int t = 0; t < 2; ++t)
            if (tv[t]) {
                const int col = 32 * tct[t] + r;
                const bool on = col < H;
                const float e2 = on ? VB[2 * H + col] : 0.f, e3 = on ? VB[3 * H + col] : 0.f;
#pragma unroll
                for (int i = 0; i < 16; ++i) X[acc_row(0, i, h) * XS + col] = fmaxf(fmaf(acc[t][i], e2, e3), 0.f);
            }
        __syncthreads();
#pragma unroll
        for (int t = 0; t < 2; ++t)
            if (tv[t]) gen_gemm_tile<false>(X, XS, W1 + (int64_t)tct[t] * GL.kg_h * 256, GL.kg_h, 0, hr[t]);
    }
    // h (+ the deferred biases) -> workspace X for the final launch
#pragma unroll
    for (int t = 0; t < 2; ++t)
        if (tv[t]) {
            const int col = 32 * tct[t] + r;
            const float sh = col < H ? V[col] : 0.f;
#pragma unroll
            for (int i = 0; i < 16; ++i) w.X[(row0 + acc_row(0, i, h)) * GL.Hp + col] = hr[t][i] + sh;
        }
    // coordinates -> workspace (the inputs on the first step, the identity features the
    // unconditional spline moved on every step)
    __syncthreads();
    for (int e = tid; e < R * D; e += kThreads) {
        const int rr = e / D, i = e - rr * D;
        w.CO[(row0 + rr) * D + i] = CO[rr * cs + i];
    }
}

// Final layer + conditional spline: blockIdx.x = 32-row tile, blockIdx.y = group of
// kGenWideFeat transform features, two per wave on the lane halves (gen_cond_spline's
// S == 2 form).  One writer per (row, feature) coordinate and log-det term.
template <bool INV>
__global__ void __launch_bounds__(64 * kGenWideFinalWaves) gen_wide_final_kernel(GenWideArgs w) {
    constexpr int R = kGenWideRows;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const FlowArgs &a = w.a;
    const int N = a.N, D = 2 * N, K = a.K;
    const GenLayout GL = gen_layout(N, w.H, a.nb, K);
    const int XS = GL.Hp + 4;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int h = lane >> 5, chain = lane & 31;
    float *X = (float *)smem;
    const int64_t row0 = (int64_t)blockIdx.x * R;
    const int q4 = GL.Hp / 4;
    for (int e = tid; e < R * q4; e += 64 * kGenWideFinalWaves) {
        const int rr = e / q4, q = e - rr * q4;
        *(f32x4 *)(X + rr * XS + 4 * q) = *(const f32x4 *)(w.X + (row0 + rr) * GL.Hp + 4 * q);
    }
    __syncthreads();
    const int j0 = blockIdx.y * kGenWideFeat + 2 * wid;
    if (j0 >= N) return;
    const int f0 = j0, f1 = j0 + 1 < N ? j0 + 1 : j0;
    const int jraw = j0 + h;
    const bool act = jraw < N;
    const int jl = act ? jraw : N - 1;
    bool nan_any = false;
    const float *P = a.packed + (int64_t)w.layer * GL.stride;
    const float l = gen_cond_spline<INV>(X, XS, P, GL, f0, f1, 0, jl, act, chain, w.CO + row0 * D, D,
                                         (2 * jl + 1 + w.off) % D, K, a, nan_any);
    if (act) w.TC[(row0 + chain) * N + jl] = l;
    if (nan_any && row0 + chain < a.nrows && a.err) atomicOr(a.err, 1);
}

// Output phase: fold the last layer, add a chain's slots in slot order, write the results
// (flow_general_kernel's output phase).  One thread per row for the scalar, all for `out`.
template <int MODE>
__global__ void __launch_bounds__(256) gen_wide_output_kernel(GenWideArgs w) {
    constexpr bool INV = MODE != MODE_DENSITY;
    constexpr int R = kGenWideRows;
    const FlowArgs &a = w.a;
    const int N = a.N, D = 2 * N;
    const int tid = threadIdx.x, off = w.off;
    const int64_t row0 = (int64_t)blockIdx.x * R;
    const int nslots = kWaves * (64 / gen_rows((int)rup(w.H, 32)));
    if (tid < R && row0 + tid < a.nrows) {
        const int64_t gr = row0 + tid;
        float tot = 0.f;
        for (int q = 0; q < nslots; ++q)
            tot += gen_wide_fold<INV>(w.LDP[gr * kGenWideSlots + q], w.TC + gr * N, w.TU + gr * kGenWideSlots, N, q,
                                      nslots);
        float outv = tot;
        if (MODE == MODE_DENSITY && a.add_base) {
            bool inb = true;
            for (int i = 0; i < D; ++i) {
                const float z = w.CO[gr * D + i];
                inb = inb && (z >= a.negB) && (z <= a.B);
            }
            outv = tot + (inb ? a.base_lp : -INFINITY);
        }
        if (MODE == MODE_PROPOSE && a.add_base) outv = a.base_lp - tot;
        if (a.scalar_out) a.scalar_out[gr] = outv;
    }
    for (int e = tid; e < R * D; e += 256) {
        const int rr = e / D, i = e - rr * D;
        const int64_t gr = row0 + rr;
        if (gr >= a.nrows) continue;
        const float v = w.CO[gr * D + (i + off) % D];
        if (a.out) a.out[gr * D + i] = v;
        if (MODE == MODE_PROPOSE) {
            const float cfg = v + a.B;
            if (a.config) a.config[gr * D + i] = cfg;
            if (a.centered) a.centered[gr * D + i] = (float)((double)cfg - a.half_width);
        }
    }
}

// ---------------------------------------------------------------------------
// Packing
// ---------------------------------------------------------------------------
// Fragments of a Linear W[nout][kin] for all layers (blockIdx.y) and blocks (blockIdx.z);
// kind 0: plain (output column = row of W); kind 1: final-layer widths / heights, 2 tiles
// per feature, scaled by sc.  Columns past nout (K) and inputs past kin are zero.
__global__ void gen_pack_linear_kernel(float *__restrict__ dst, const float *__restrict__ src, int kin, int kg,
                                       int ntiles, int nout, int kind, int K, float sc, int64_t sl, int64_t dl,
                                       int64_t sz, int64_t dz) {
    src += blockIdx.y * sl + blockIdx.z * sz;
    dst += blockIdx.y * dl + blockIdx.z * dz;
    const int64_t total = (int64_t)ntiles * kg * 256;
    const int P = 3 * K + 1;
    for (int64_t idx = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; idx < total;
         idx += (int64_t)gridDim.x * blockDim.x) {
        const int j = idx & 3;
        const int lane = (idx >> 2) & 63;
        const int64_t tg = idx >> 8;
        const int g = (int)(tg % kg);
        const int tile = (int)(tg / kg);
        const int k = 8 * g + 4 * (lane >> 5) + j;
        const int c = lane & 31;
        int64_t row = -1;
        if (kind == 0) {
            const int col = 32 * tile + c;
            row = col < nout ? col : -1;
        } else {
            const int feat = tile / 2, t = tile % 2;
            if (c < K) row = (int64_t)feat * P + t * K + c;
        }
        float v = 0.f;
        if (row >= 0 && k < kin) v = kind == 0 ? src[row * kin + k] : src[row * kin + k] * sc;
        dst[idx] = v;
    }
}

// derivative rows d_0..d_K of every feature (final-layer rows 2K..3K, unscaled) as
// [N][Hp / 4][K + 1][4], zero past H
__global__ void gen_pack_deriv_kernel(float *__restrict__ dst, const float *__restrict__ src, int N, int H, int Hp,
                                      int K, int64_t sl, int64_t dl) {
    src += blockIdx.y * sl;
    dst += blockIdx.y * dl;
    const int K1 = K + 1, P = 3 * K + 1;
    const int64_t total = (int64_t)N * Hp * K1;
    for (int64_t idx = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; idx < total;
         idx += (int64_t)gridDim.x * blockDim.x) {
        const int i = idx & 3;
        const int64_t t = idx >> 2;
        const int b = (int)(t % K1);
        const int64_t fq = t / K1;
        const int q = (int)(fq % (Hp / 4));
        const int feat = (int)(fq / (Hp / 4));
        const int k = 4 * q + i;
        dst[idx] = k < H ? src[((int64_t)feat * P + 2 * K + b) * H + k] : 0.f;
    }
}

}  // namespace fs

using namespace fs;

bool fs_flow_general_supported(const fs_flow_dims *d, char *why, size_t n) {
    if (d->N < 1 || d->N > kMaxN) {
        snprintf(why, n, "precision 4 (general shape): N=%d outside 1..%d", d->N, kMaxN);
        return false;
    }
    if (d->L < 1) {
        snprintf(why, n, "precision 4 (general shape): L=%d, at least 1 layer", d->L);
        return false;
    }
    if (d->nb < 0) {
        snprintf(why, n, "precision 4 (general shape): nb=%d is negative", d->nb);
        return false;
    }
    if (d->H < 1 || d->H > kGenMaxH) {
        snprintf(why, n, "precision 4 (general shape): H=%d outside 1..%d", d->H, kGenMaxH);
        return false;
    }
    if (d->K < 1 || d->K > kMaxK) {
        snprintf(why, n, "precision 4 (general shape): K=%d outside 1..%d", d->K, kMaxK);
        return false;
    }
    if (!(d->tail_bound > 0)) {
        snprintf(why, n, "precision 4 (general shape): tail_bound=%g must be positive", d->tail_bound);
        return false;
    }
    const GenLayout GL = gen_layout(d->N, d->H, d->nb, d->K);
    if (gen_lds(d->N, GL.Hp, GL.kin_p, GL.rows).total > 163840) {  // (never within the range above)
        snprintf(why, n, "precision 4 (general shape): LDS budget exceeded for N=%d H=%d", d->N, d->H);
        return false;
    }
    return true;
}

int64_t fs_flow_general_packed_bytes(const fs_flow_dims *d) {
    return gen_layout(d->N, d->H, d->nb, d->K).stride * d->L * 4;
}

hipError_t fs_flow_general_pack(const fs_flow_dims *d, const float *raw, float *packed, hipStream_t st) {
    const int N = d->N, H = d->H, nb = d->nb, K = d->K;
    const RawLayout R = raw_layout(N, H, nb, K);
    const GenLayout GL = gen_layout(N, H, nb, K);
    const PackLayout PL = pack_layout(N, H, nb, K);
    hipError_t e = hipMemsetAsync(packed, 0, (size_t)GL.stride * d->L * 4, st);
    if (e != hipSuccess) return e;
    if (d->L > 65535 || nb > 65535) return hipErrorInvalidValue;  // grid y / z
    const unsigned NL = (unsigned)d->L;
    const int64_t sl = R.stride, dl = GL.stride;
    auto lin = [&](float *o, const float *w, int kin, int kg, int ntiles, int nout, int kind, unsigned nz, int64_t sz,
                   int64_t dz) {
        const int64_t tot = (int64_t)ntiles * kg * 256;
        int blocks = (int)((tot + 255) / 256);
        if (blocks > 1024) blocks = 1024;
        hipLaunchKernelGGL(gen_pack_linear_kernel, dim3(blocks, NL, nz), dim3(256), 0, st, o, w, kin, kg, ntiles,
                           nout, kind, K, (float)(1.4426950408889634 / sqrt((double)H)), sl, dl, sz, dz);
    };
    lin(packed + GL.win, raw + R.win, 2 * N, GL.kg_in, GL.ct_h, H, 0, 1, 0, 0);
    if (nb > 0) {
        lin(packed + GL.blocks, raw + R.blocks + RawLayout::w0(H), H, GL.kg_h, GL.ct_h, H, 0, (unsigned)nb,
            R.block_stride, GL.block_stride);
        lin(packed + GL.blocks + GL.block_stride / 2, raw + R.blocks + RawLayout::w1(H), H, GL.kg_h, GL.ct_h, H, 0,
            (unsigned)nb, R.block_stride, GL.block_stride);
    }
    lin(packed + GL.wf, raw + R.wf, H, GL.kg_h, 2 * N, 0, 1, 1, 0, 0);
    {
        const int64_t tot = (int64_t)N * GL.Hp * (K + 1);
        int blocks = (int)((tot + 255) / 256);
        if (blocks > 1024) blocks = 1024;
        hipLaunchKernelGGL(gen_pack_deriv_kernel, dim3(blocks, NL), dim3(256), 0, st, packed + GL.wd, raw + R.wf, N, H,
                           GL.Hp, K, sl, dl);
    }
    if (e = hipGetLastError(); e != hipSuccess) return e;
    // biases, folded BatchNorm and unconditional knots: the instantiated image's own
    // vector section (true H), placed where this image keeps it
    for (int l = 0; l < d->L; ++l) {
        e = fs_flow_pack_vec(packed + (int64_t)l * GL.stride + (GL.vec - PL.vec), raw + (int64_t)l * R.stride, d, st);
        if (e != hipSuccess) return e;
    }
    return hipGetLastError();
}

template <int MODE>
static hipError_t launch_general(const FlowArgs &a, int N, int H, hipStream_t st) {
    auto kfn = flow_general_kernel<MODE>;
    static std::atomic<unsigned long long> attr_set{0};  // per instantiation, bit d = device d
    if (hipError_t e = fs_set_max_lds_once((const void *)kfn, attr_set); e != hipSuccess) return e;
    const GenLayout GL = gen_layout(N, H, a.nb, a.K);
    const int64_t blocks = (a.nrows + GL.rows - 1) / GL.rows;
    if (blocks > 0x7fffffff) return hipErrorInvalidValue;
    hipLaunchKernelGGL(kfn, dim3((unsigned)blocks), dim3(kThreads), gen_lds(N, GL.Hp, GL.kin_p, GL.rows).total, st, a,
                       H);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// wide path: host side
// ---------------------------------------------------------------------------
constexpr int64_t kGenWideMaxRows = 65536;  // the workspace never grows beyond this many rows
// the measured default (tools/general_wide_ab.py, DESIGN.md 'General-shape mode'): the largest
// row count at which the wide path beat the fused kernel at every measured shape
#ifndef FS_GENERAL_WIDE_ROWS_DEFAULT
#define FS_GENERAL_WIDE_ROWS_DEFAULT 1024
#endif

// Largest batch that takes the wide path (FS_GENERAL_WIDE_ROWS, or
// fs_set_general_wide_rows(); 0 disables it)
static std::atomic<int64_t> g_gen_wide_rows{-1};
static std::atomic<int64_t> g_gen_wide_passes{0};
static int64_t gen_wide_rows_limit() {
    int64_t lim = g_gen_wide_rows.load(std::memory_order_relaxed);
    if (lim < 0) {
        const char *e = getenv("FS_GENERAL_WIDE_ROWS");
        lim = e ? atoll(e) : FS_GENERAL_WIDE_ROWS_DEFAULT;
        lim = lim < 0 ? 0 : (lim > kGenWideMaxRows ? kGenWideMaxRows : lim);
        int64_t expect = -1;
        g_gen_wide_rows.compare_exchange_strong(expect, lim);
        lim = g_gen_wide_rows.load(std::memory_order_relaxed);
    }
    return lim;
}

int64_t fs_set_general_wide_rows_impl(int64_t rows) {
    const int64_t prev = gen_wide_rows_limit();
    if (rows >= 0) g_gen_wide_rows.store(rows > kGenWideMaxRows ? kGenWideMaxRows : rows, std::memory_order_relaxed);
    return prev;
}

int64_t fs_general_wide_passes_impl() { return g_gen_wide_passes.load(std::memory_order_relaxed); }

// Workspace of the general wide path, one per (device, stream), allocated once (never
// freed or moved: a captured graph may hold its address).  nullptr when it would have to
// be allocated during stream capture or the first allocation (of `cap` bytes) is smaller
// than the `bytes` this pass needs.
static void *gen_wide_workspace(size_t bytes, size_t cap, hipStream_t st) {
    static std::mutex mu;
    static std::map<std::pair<int, hipStream_t>, std::pair<void *, size_t>> ws;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    std::lock_guard<std::mutex> g(mu);
    auto &e = ws[{dev, st}];
    if (e.first && e.second >= bytes) return e.first;
    if (e.first) return nullptr;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) return nullptr;
    void *p = nullptr;
    if (hipMalloc(&p, cap) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    e = {p, cap};
    return p;
}

// compute units of the current device (cached per device)
static int gen_device_cus() {
    static std::atomic<int> cus[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
    int v = cus[dev].load(std::memory_order_relaxed);
    if (v <= 0) {
        if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0) v = 256;
        cus[dev].store(v, std::memory_order_relaxed);
    }
    return v;
}

// CO, X, TC, TU, LDP of R rows (a multiple of 32), each section 256-byte aligned
static size_t gen_wide_bytes(int64_t R, int N, int Hp) {
    return (size_t)(rup(R * 2 * N * 4, 256) + rup(R * Hp * 4, 256) + rup(R * N * 4, 256) +
                    2 * rup(R * kGenWideSlots * 4, 256));
}

// The pass as 2 L + 1 launches on the stream; used = false (and nothing launched) when the
// workspace is not available or too small: the caller then launches the fused kernel.
template <int MODE>
static hipError_t gen_wide_pass(const FlowArgs &a, int N, int H, hipStream_t st, bool &used) {
    constexpr bool INV = MODE != MODE_DENSITY;
    used = false;
    const GenLayout GL = gen_layout(N, H, a.nb, a.K);
    const int64_t R = rup(a.nrows, kGenWideRows);
    // one allocation per (device, stream), sized for at least 16384 rows at the widest shape
    // (~46 MiB) or the current limit if larger
    const int64_t lim = gen_wide_rows_limit() < 16384 ? 16384 : gen_wide_rows_limit();
    const size_t cap = gen_wide_bytes(rup(lim, kGenWideRows), kMaxN, kGenMaxH);
    const size_t need = gen_wide_bytes(R, N, GL.Hp);
    if (need > cap) return hipSuccess;
    char *p = (char *)gen_wide_workspace(need, cap, st);
    if (!p) return hipSuccess;
    auto ktr = gen_wide_trunk_kernel<MODE>;
    auto kfi = gen_wide_final_kernel<INV>;
    {
        static std::atomic<unsigned long long> tr_set{0}, fi_set{0};  // per instantiation, bit d = device d
        if (hipError_t e = fs_set_max_lds_once((const void *)ktr, tr_set); e != hipSuccess) return e;
        if (hipError_t e = fs_set_max_lds_once((const void *)kfi, fi_set); e != hipSuccess) return e;
    }
    const int D = 2 * N;
    GenWideArgs w;
    memset(&w, 0, sizeof(w));
    w.a = a;
    w.H = H;
    w.CO = (float *)p;
    p += rup(R * D * 4, 256);
    w.X = (float *)p;
    p += rup(R * GL.Hp * 4, 256);
    w.TC = (float *)p;
    p += rup(R * N * 4, 256);
    w.TU = (float *)p;
    p += rup(R * kGenWideSlots * 4, 256);
    w.LDP = (float *)p;
    const unsigned tiles = (unsigned)(R / kGenWideRows);
    const unsigned groups = (unsigned)((N + kGenWideFeat - 1) / kGenWideFeat);
    const unsigned tr_lds = (unsigned)gen_lds(N, GL.Hp, GL.kin_p, kGenWideRows).total;
    const unsigned fi_lds = (unsigned)(kGenWideRows * (GL.Hp + 4) * 4);
    int off = 0;
    for (int s = 0; s < a.L; ++s) {
        w.layer = INV ? s : a.L - 1 - s;
        if (INV) off = (off + N) % D;  // Coupling.inverse rolls first
        w.off = off;
        w.first = s == 0;
        hipLaunchKernelGGL(ktr, dim3(tiles), dim3(kThreads), tr_lds, st, w);
        hipLaunchKernelGGL(kfi, dim3(tiles, groups), dim3(64 * kGenWideFinalWaves), fi_lds, st, w);
        if (!INV) off = (off + N) % D;  // Coupling.forward rolls last
    }
    w.off = off;
    w.first = 0;
    hipLaunchKernelGGL(gen_wide_output_kernel<MODE>, dim3(tiles), dim3(256), 0, st, w);
    used = true;
    g_gen_wide_passes.fetch_add(1, std::memory_order_relaxed);
    return hipGetLastError();
}

hipError_t fs_flow_general_pass(const FlowArgs &a, int mode, int N, int H, int K, hipStream_t st) {
    (void)K;
    const int R = gen_rows((int)rup(H, 32));
    if (a.nrows <= gen_wide_rows_limit() && (a.nrows + R - 1) / R < 2 * gen_device_cus()) {
        // small batch: the wide path (bit-identical results), when its workspace is available
        bool used = false;
        hipError_t e = mode == MODE_DENSITY  ? gen_wide_pass<MODE_DENSITY>(a, N, H, st, used)
                       : mode == MODE_SAMPLE ? gen_wide_pass<MODE_SAMPLE>(a, N, H, st, used)
                                             : gen_wide_pass<MODE_PROPOSE>(a, N, H, st, used);
        if (e != hipSuccess || used) return e;
    }
    if (mode == MODE_DENSITY) return launch_general<MODE_DENSITY>(a, N, H, st);
    if (mode == MODE_SAMPLE) return launch_general<MODE_SAMPLE>(a, N, H, st);
    return launch_general<MODE_PROPOSE>(a, N, H, st);
}
