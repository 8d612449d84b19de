// Analysis reductions of the Algorithm-1 driver on MI355X:
//   * classify_particles + the per-configuration part of calculate_well_statistics
//     (hybrid_NF_MCMC/utils.py:61-141): well A / B / outside per particle, the
//     all-in-A / all-in-B flag and np.mean(config[:, 0]) per configuration;
//   * the pair-distance histogram and the g(r) mean of calculate_pair_correlation
//     (utils.py:530-574).
// numpy's scalar promotion is reproduced: with a float32 array every Python float
// (centres, box, radius**2, 2*bound) is rounded to float32 first (NEP 50 weak
// scalars, comparisons included) and the arithmetic stays float32; with float64
// it is float64.  Sums follow numpy's pairwise order in the array's dtype.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "fs_internal.h"

#pragma clang fp contract(off)

namespace fs {

// numpy pairwise_sum (loops_utils.h) of load(0..n-1), accumulating in T: blocks of
// <= 128 use 8 partial sums (sequential below 8); larger blocks split at n2 = n/2
// rounded down to a multiple of 8 and add the halves.  The recursion runs on an
// explicit stack (depth <= log2(n/128) + 1).
template <typename T, typename Load>
__device__ T pairwise_leaf(Load load, int64_t off, int64_t n) {
    if (n < 8) {
        T res = T(0);
        for (int64_t i = 0; i < n; ++i) res += load(off + i);
        return res;
    }
    T r[8];
    for (int j = 0; j < 8; ++j) r[j] = load(off + j);
    int64_t i = 8;
    for (; i < n - (n % 8); i += 8)
        for (int j = 0; j < 8; ++j) r[j] += load(off + i + j);
    T res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; ++i) res += load(off + i);
    return res;
}

template <typename T, typename Load>
__device__ T pairwise_sum_dev(Load load, int64_t n) {
    struct Frame {
        int64_t off, n;
        T left;
        int stage;  // 0 new, 1 left half pending, 2 right half pending
    };
    auto half = [](int64_t k) { return k / 2 - (k / 2) % 8; };
    Frame st[48];
    int sp = 0;
    st[0] = {0, n, T(0), 0};
    while (true) {
        Frame &f = st[sp];
        if (f.n > 128) {
            f.stage = 1;
            st[sp + 1] = {f.off, half(f.n), T(0), 0};
            ++sp;
            continue;
        }
        T val = pairwise_leaf<T>(load, f.off, f.n);
        while (true) {  // hand the finished block to its parents
            if (sp == 0) return val;
            --sp;
            Frame &p = st[sp];
            if (p.stage == 1) {
                p.left = val;
                p.stage = 2;
                const int64_t n2 = half(p.n);
                st[sp + 1] = {p.off + n2, p.n - n2, T(0), 0};
                ++sp;
                break;
            }
            val = p.left + val;
        }
    }
}

// classify_particles' per-particle test (utils.py:104-141) in the array dtype T:
// box = halfbox*2 for both axes, centres (box/4, box/2) and (3box/4, box/2), radius
// r0*1.1, each a Python float rounded into T (numpy 2 weak scalars)
template <typename T>
struct WellTest {
    T bx, by, lcx, lcy, rcx, rcy, rad2;
    __device__ WellTest(double half_box, double r0) {
        const double box = half_box * 2.0, radius = r0 * 1.1;
        bx = (T)box;
        by = (T)box;
        lcx = (T)(box / 4.0);
        lcy = (T)(box / 2.0);
        rcx = (T)(3.0 * box / 4.0);
        rcy = (T)(box / 2.0);
        rad2 = (T)(radius * radius);  // radius ** 2 (Python float), compared in T
    }
    __device__ bool in_circle(T x, T y, T cx, T cy) const {
        T dx = x - cx, dy = y - cy;
        dx -= bx * (T)rint(dx / bx);
        dy -= by * (T)rint(dy / by);
        const T dx2 = dx * dx, dy2 = dy * dy;
        return (dx2 + dy2) <= rad2;
    }
    // 0 = 'A' (left), 1 = 'B' (right), 2 = 'Outside'
    __device__ int classify(T x, T y) const {
        if (in_circle(x, y, lcx, lcy)) return 0;
        return in_circle(x, y, rcx, rcy) ? 1 : 2;
    }
};

// one wave per configuration, lane loop over particles
template <typename T>
__global__ void __launch_bounds__(256) classify_kernel(const T *__restrict__ pos, int64_t M, int N, double half_box,
                                                       double r0, uint8_t *__restrict__ cls,
                                                       uint8_t *__restrict__ state, double *__restrict__ avg_x) {
    const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t m = (int64_t)blockIdx.x * 4 + wid;
    if (m >= M) return;
    const WellTest<T> w(half_box, r0);
    const T *q = pos + m * (int64_t)N * 2;
    bool allA = true, allB = true;
    for (int i = lane; i < N; i += 64) {
        const int k = w.classify(q[2 * i], q[2 * i + 1]);
        if (cls) cls[m * N + i] = (uint8_t)k;
        allA &= k == 0;
        allB &= k == 1;
    }
    allA = __all(allA);
    allB = __all(allB);
    if (lane == 0) {
        if (state) state[m] = allA ? 1 : (allB ? 2 : 0);
        if (avg_x) {  // np.mean(config[:, 0]) in the array dtype: pairwise sum / N
            const T s = pairwise_sum_dev<T>([&](int64_t i) { return q[2 * i]; }, N);
            avg_x[m] = (double)(s / (T)N);
        }
    }
}

// calculate_well_statistics' all-in-A / all-in-B counts (utils.py:73-86) for the
// batched engine's live chain states: state f64 [C][N][2] holding each chain's
// values, classified in that chain's reference dtype (float32 after an accepted big
// move, monte_carlo.py:296), one wave per chain.
__global__ void __launch_bounds__(256) well_stats_kernel(const double *__restrict__ pos,
                                                         const uint8_t *__restrict__ is_f32, int64_t C, int N,
                                                         double half_box, double r0,
                                                         long long *__restrict__ counts) {
    const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t c = (int64_t)blockIdx.x * 4 + wid;
    if (c >= C) return;
    const double *q = pos + c * (int64_t)N * 2;
    bool allA = true, allB = true;
    if (is_f32 && is_f32[c]) {
        const WellTest<float> w(half_box, r0);
        for (int i = lane; i < N; i += 64) {
            const int k = w.classify((float)q[2 * i], (float)q[2 * i + 1]);
            allA &= k == 0;
            allB &= k == 1;
        }
    } else {
        const WellTest<double> w(half_box, r0);
        for (int i = lane; i < N; i += 64) {
            const int k = w.classify(q[2 * i], q[2 * i + 1]);
            allA &= k == 0;
            allB &= k == 1;
        }
    }
    allA = __all(allA);
    allB = __all(allB);
    if (lane == 0) {
        counts[3 * c] += allA;
        counts[3 * c + 1] += (!allA && allB);
        counts[3 * c + 2] += 1;
    }
}

// pair-distance histogram of one configuration per wave (utils.py:546-556): all
// ordered pairs i != j, distance != 0, bins [e_k, e_k+1) with the last bin closed
template <typename T>
__global__ void __launch_bounds__(256) pair_hist_kernel(const T *__restrict__ pos, int64_t M, int N, double bound,
                                                        const double *__restrict__ edges, int nb,
                                                        int32_t *__restrict__ counts) {
    __shared__ int32_t h[4][128];
    __shared__ T sx[4][256], sy[4][256];
    const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t m = (int64_t)blockIdx.x * 4 + wid;
    if (m >= M) return;
    for (int k = lane; k < nb; k += 64) h[wid][k] = 0;
    const T *q = pos + m * (int64_t)N * 2;
    for (int i = lane; i < N; i += 64) {
        sx[wid][i] = q[2 * i];
        sy[wid][i] = q[2 * i + 1];
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const T tb = (T)(2.0 * bound);
    const double e0 = edges[0], elast = edges[nb];
    for (int i = lane; i < N; i += 64) {
        const T xi = sx[wid][i], yi = sy[wid][i];
        for (int j = 0; j < N; ++j) {
            T dx = xi - sx[wid][j], dy = yi - sy[wid][j];
            dx = dx - tb * (T)rint(dx / tb);
            dy = dy - tb * (T)rint(dy / tb);
            const T s0 = dx * dx, s1 = dy * dy;
            const T s = s0 + s1;
            const double d = (double)(T)sqrt(s);
            if (d == 0.0 || d < e0 || d > elast) continue;
            // searchsorted: k with edges[k] <= d < edges[k+1], last bin right-inclusive
            int lo = 0, hi = nb;
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (edges[mid] <= d) lo = mid;
                else hi = mid;
            }
            atomicAdd(&h[wid][lo], 1);
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    for (int k = lane; k < nb; k += 64) counts[m * nb + k] = h[wid][k];
}

// g(r) = mean over configurations of counts / denom (utils.py:558-566): the
// per-configuration ratio in float64, then pandas' mean = pairwise sum / M
__global__ void rdf_mean_kernel(const int32_t *__restrict__ counts, int64_t M, int nb, const double *__restrict__ denom,
                                double *__restrict__ g) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nb) return;
    const double dk = denom[k];
    const double s =
        pairwise_sum_dev<double>([&](int64_t m) { return (double)counts[m * nb + k] / dk; }, M);
    g[k] = s / (double)M;
}

// One analysis batch of the Algorithm-2 checkpoint cycle (main_algorithm_2.py:493-525)
// in one launch, float32 as the reference's numpy arrays are:
//   a_  = a + HALF_BOX          -> out (the rows of samples.npy)
//   c   = a_ - HALF_BOX         (HALF_BOX rounded to float32 both times: weak scalar)
//   np.histogram2d(c)           -> hist += (hist2d_lds_kernel's rule on (double)c)
//   pair-distance counts of c   -> counts (pair_hist_kernel<float>'s arithmetic)
// One wave per configuration, four per workgroup, the workgroup striding over the
// batch; the 2-D histogram is private to the workgroup in LDS (uint32: a workgroup bins
// far fewer than 2^32 particles) and its non-empty bins are flushed once at the end.
// All LDS is dynamic (16-byte carve offsets): at nb = 120 it passes 64 KiB.
constexpr int kSaRBins = 128, kSaN = 256;  // pair_hist_kernel's bounds (nb <= 120 as hist2d_lds_kernel: capi.cpp)

struct SaLds {
    int e2, er, h2, hp, sx, sy, bytes;
};
__host__ __device__ inline SaLds sa_lds(int nb, int nr) {
    auto up = [](int v) { return (v + 15) & ~15; };
    SaLds L;
    int o = 0;
    L.e2 = o, o = up(o + (nb + 1) * 8);
    L.er = o, o = up(o + (nr + 1) * 8);
    L.h2 = o, o = up(o + nb * nb * 4);
    L.hp = o, o += 4 * kSaRBins * 4;
    L.sx = o, o += 4 * kSaN * 4;
    L.sy = o, o += 4 * kSaN * 4;
    L.bytes = o;
    return L;
}

// k with e[k] <= v < e[k+1], for sorted edges e[0..n] and e[0] <= v < e[n]: the bin an
// evenly spaced grid would give (inv_w = n / (e[n] - e[0])), then steps along the edges
// until the inequalities hold.  The result is searchsorted's for any sorted edges; with
// linspace / arange edges it takes two or three LDS reads instead of a binary search's
// log2(n) dependent ones.
__device__ inline int bin_near(const double *e, int n, double inv_w, double v) {
    int k = (int)((v - e[0]) * inv_w);
    k = k < 0 ? 0 : (k > n - 1 ? n - 1 : k);
    while (k > 0 && e[k] > v) --k;
    while (k < n - 1 && e[k + 1] <= v) ++k;
    return k;
}

__global__ void __launch_bounds__(256) sample_analysis_kernel(const float *__restrict__ z, int64_t M, int N,
                                                              double half_box, const double *__restrict__ edges2,
                                                              int nb, const double *__restrict__ edges_r, int nr,
                                                              float *__restrict__ out,
                                                              unsigned long long *__restrict__ hist,
                                                              int32_t *__restrict__ counts) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const SaLds L = sa_lds(nb, nr);
    double *e2 = (double *)(smem + L.e2), *er = (double *)(smem + L.er);
    unsigned int *h2 = (unsigned int *)(smem + L.h2);
    const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int32_t *hp = (int32_t *)(smem + L.hp) + wid * kSaRBins;
    float *sx = (float *)(smem + L.sx) + wid * kSaN, *sy = (float *)(smem + L.sy) + wid * kSaN;
    for (int i = threadIdx.x; i < nb * nb; i += blockDim.x) h2[i] = 0u;
    for (int i = threadIdx.x; i <= nb; i += blockDim.x) e2[i] = edges2[i];
    for (int i = threadIdx.x; i <= nr; i += blockDim.x) er[i] = edges_r[i];
    __syncthreads();
    const double inv2 = (double)nb / (e2[nb] - e2[0]);
    auto bin_of = [&](double v) {  // np.searchsorted(edges, v, 'right') - 1, last edge inclusive
        if (!(v >= e2[0])) return -1;
        if (v >= e2[nb]) return v == e2[nb] ? nb - 1 : nb;
        return bin_near(e2, nb, inv2, v);
    };
    const float hb = (float)half_box, tb = (float)(2.0 * half_box);
    const double e0 = er[0], elast = er[nr];
    const double invr = (double)nr / (elast - e0);
    for (int64_t m0 = (int64_t)blockIdx.x * 4; m0 < M; m0 += (int64_t)gridDim.x * 4) {
        const int64_t m = m0 + wid;
        if (m >= M) continue;  // wave-uniform
        for (int k = lane; k < nr; k += 64) hp[k] = 0;
        const float *q = z + m * (int64_t)N * 2;
        float *o = out + m * (int64_t)N * 2;
        for (int i = lane; i < N; i += 64) {
            const float ax = q[2 * i] + hb, ay = q[2 * i + 1] + hb;
            o[2 * i] = ax;
            o[2 * i + 1] = ay;
            const float cx = ax - hb, cy = ay - hb;
            sx[i] = cx;
            sy[i] = cy;
            const int bx = bin_of((double)cx), by = bin_of((double)cy);
            if (bx >= 0 && bx < nb && by >= 0 && by < nb) atomicAdd(&h2[bx * nb + by], 1u);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        for (int i = lane; i < N; i += 64) {
            const float xi = sx[i], yi = sy[i];
            for (int j = 0; j < N; ++j) {
                float dx = xi - sx[j], dy = yi - sy[j];
                dx = dx - tb * (float)rint(dx / tb);
                dy = dy - tb * (float)rint(dy / tb);
                const float s0 = dx * dx, s1 = dy * dy;
                const float s = s0 + s1;
                const double d = (double)(float)sqrt(s);
                if (d == 0.0 || d < e0 || d > elast) continue;
                // edges[lo] <= d < edges[lo+1], last bin right-inclusive
                const int lo = d >= elast ? nr - 1 : bin_near(er, nr, invr, d);
                atomicAdd(&hp[lo], 1);
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        for (int k = lane; k < nr; k += 64) counts[m * nr + k] = hp[k];
        // the next configuration of this wave reuses hp / sx / sy
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nb * nb; i += blockDim.x)
        if (h2[i]) atomicAdd(&hist[i], (unsigned long long)h2[i]);
}

// ---------------------------------------------------------------- importance weights
// Log-weights lw = -beta E - (double)log_q of flow samples against the Boltzmann target and
// their running statistics (include/flowstate.h 'Importance weights').  Two stream-ordered
// launches per batch: iw_partial_kernel (one slot of partial sums per workgroup, shifted by
// the workgroup's own maximum) and the one-wave iw_finish_kernel, which folds the slots in
// workgroup order into the running block.  The launch boundary is the hand-off; no float
// atomics, so the same inputs in the same batches give the same bits on any device.
constexpr int kIwSlots = 1024;  // workgroups of the partial launch (grid-stride beyond 256 * 1024 rows)

struct IwHeader {  // the first 64 bytes of the state block (flowstate.h)
    double max_lw, s1, s2, sum_lw;
    long long n, n_zero, n_bad, reserved;
};
struct IwSlot {
    double max_lw, s1, s2, sum_lw;
    long long n_zero, n_bad, pad0, pad1;
};
static_assert(sizeof(IwHeader) == 64 && sizeof(IwSlot) == 64, "state block layout");

__device__ inline double wave_max(double v) {
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    return v;
}
// lane 0 ends with ((..) + (..)): a fixed tree over the 64 lanes
__device__ inline double wave_sum(double v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}
__device__ inline long long wave_sum_i(long long v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

// thread 0 returns the sum over the 256 threads: wave trees, then the four waves in order
__device__ inline double block_sum(double v, double *red) {
    const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63;
    v = wave_sum(v);
    __syncthreads();  // red may still be read from the previous call
    if (lane == 0) red[wid] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

// exp(a - b) for a <= b, 0 when a is -inf (b = -inf included: no inf - inf)
__device__ inline double exp_shift(double a, double b) { return a == -INFINITY ? 0.0 : exp(a - b); }

__global__ void iw_reset_kernel(IwHeader *h) {
    if (threadIdx.x == 0) *h = IwHeader{-INFINITY, 0.0, 0.0, 0.0, 0, 0, 0, 0};
}

__global__ void __launch_bounds__(256) iw_partial_kernel(double beta, int64_t M, const double *__restrict__ E,
                                                         const float *__restrict__ log_q, double *log_w,
                                                         IwSlot *__restrict__ slots) {
    __shared__ double red[4];
    __shared__ long long redi[2][4];
    const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t first = (int64_t)blockIdx.x * 256 + threadIdx.x, step = (int64_t)gridDim.x * 256;
    const double nbeta = -beta;
    double tmax = -INFINITY, tsum = 0.0;
    long long nz = 0, nb = 0;
    for (int64_t m = first; m < M; m += step) {
        const double e = E[m];
        const float q = log_q[m];
        double lw;
        if (!(q == q) || q == INFINITY || q == -INFINITY || !(e == e) || e == -INFINITY) {
            lw = -INFINITY;  // bad row: never reaches a sum
            ++nb;
        } else {
            const double t = nbeta * e;
            lw = t - (double)q;
            if (lw == -INFINITY) ++nz;  // hard-core overlap: weight 0
            else tsum += lw;
        }
        log_w[m] = lw;
        tmax = fmax(tmax, lw);
    }
    double wmax = wave_max(tmax);
    if (lane == 0) red[wid] = wmax;
    __syncthreads();
    wmax = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
    double s1 = 0.0, s2 = 0.0;
    for (int64_t m = first; m < M; m += step) {
        const double w = exp_shift(log_w[m], wmax);  // this thread's own store above
        s1 += w;
        s2 += w * w;
    }
    s1 = block_sum(s1, red);
    s2 = block_sum(s2, red);
    tsum = block_sum(tsum, red);
    nz = wave_sum_i(nz);
    nb = wave_sum_i(nb);
    if (lane == 0) {
        redi[0][wid] = nz;
        redi[1][wid] = nb;
    }
    __syncthreads();
    if (threadIdx.x == 0)
        slots[blockIdx.x] = IwSlot{wmax, s1, s2, tsum, redi[0][0] + redi[0][1] + redi[0][2] + redi[0][3],
                                   redi[1][0] + redi[1][1] + redi[1][2] + redi[1][3], 0, 0};
}

// one wave: the batch's maximum, every slot and the old sums rescaled to it once, then the
// slots added in workgroup order by lane 0
__global__ void __launch_bounds__(64) iw_finish_kernel(IwHeader *h, const IwSlot *__restrict__ slots, int P,
                                                       int64_t M) {
    __shared__ double a1[kIwSlots], a2[kIwSlots];
    const int lane = threadIdx.x;
    const double old_max = h->max_lw;
    double mx = old_max;
    for (int p = lane; p < P; p += 64) mx = fmax(mx, slots[p].max_lw);
    mx = wave_max(mx);
    for (int p = lane; p < P; p += 64) {
        const double f = exp_shift(slots[p].max_lw, mx);
        a1[p] = slots[p].s1 * f;
        a2[p] = slots[p].s2 * (f * f);
    }
    __syncthreads();
    if (lane != 0) return;
    const double f = exp_shift(old_max, mx);  // 1 exactly while the maximum stands
    double s1 = h->s1 * f, s2 = h->s2 * (f * f), sl = h->sum_lw;
    long long nz = h->n_zero, nb = h->n_bad;
    for (int p = 0; p < P; ++p) {
        s1 += a1[p];
        s2 += a2[p];
        sl += slots[p].sum_lw;
        nz += slots[p].n_zero;
        nb += slots[p].n_bad;
    }
    *h = IwHeader{mx, s1, s2, sl, h->n + (long long)M, nz, nb, 0};
}

// normalised weight exp(lw - max_lw) / S1 of a row; 0 for lw = -inf (or NaN) rows and while S1 = 0
__device__ inline double iw_weight(double lw, double mx, double s1) {
    if (!(lw > -INFINITY) || !(s1 > 0.0)) return 0.0;
    return exp(lw - mx) / s1;
}

// Weighted g(r) and well populations: workgroup k < nr sums w~_m counts[m][k] / denom[k],
// workgroup nr the three scalars.  Thread t adds its rows t, t + 256, .. in order, then
// block_sum's fixed tree: bit-reproducible.
__global__ void __launch_bounds__(256) weighted_reduce_kernel(const int32_t *__restrict__ counts, int64_t M, int nr,
                                                              const double *__restrict__ denom,
                                                              const uint8_t *__restrict__ wstate,
                                                              const double *__restrict__ avg_x,
                                                              const double *__restrict__ log_w,
                                                              const IwHeader *__restrict__ h,
                                                              double *__restrict__ g_w, double *__restrict__ scalars) {
    __shared__ double red[4];
    const double mx = h->max_lw, s1 = h->s1;
    const int k = blockIdx.x;
    if (k < nr) {
        const double dk = denom[k];
        double s = 0.0;
        for (int64_t m = threadIdx.x; m < M; m += 256) {
            const double w = iw_weight(log_w[m], mx, s1);
            if (w > 0.0) s += w * ((double)counts[m * nr + k] / dk);
        }
        s = block_sum(s, red);
        if (threadIdx.x == 0) g_w[k] = s;
        return;
    }
    double pa = 0.0, pb = 0.0, ax = 0.0;
    for (int64_t m = threadIdx.x; m < M; m += 256) {
        const double w = iw_weight(log_w[m], mx, s1);
        if (!(w > 0.0)) continue;
        const int st = wstate[m];
        if (st == 1) pa += w;
        if (st == 2) pb += w;
        ax += w * avg_x[m];
    }
    pa = block_sum(pa, red);
    pb = block_sum(pb, red);
    ax = block_sum(ax, red);
    if (threadIdx.x == 0) {
        scalars[0] = pa;
        scalars[1] = pb;
        scalars[2] = (pa > 0.0 && pb > 0.0) ? log(pb / pa) : 0.0;  // utils.py:92-96
        scalars[3] = ax;
    }
}

// Weighted 2-D histogram of the configurations (the rows of samples.npy): sample_analysis_kernel's
// arrangement and binning rule on (double)(cfg - fl32(half_box)), the workgroup's bins float64
// in LDS (nb * nb * 8 bytes), non-zero bins flushed by float64 atomic adds.
__host__ __device__ inline int wh_lds_bytes(int nb) { return (((nb + 1) * 8 + 15) & ~15) + nb * nb * 8; }

__global__ void __launch_bounds__(256) weighted_hist2d_kernel(const float *__restrict__ cfg, int64_t M, int N,
                                                              double half_box, const double *__restrict__ edges2,
                                                              int nb, const double *__restrict__ log_w,
                                                              const IwHeader *__restrict__ h,
                                                              double *__restrict__ hist) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double *e2 = (double *)smem;
    double *h2 = (double *)(smem + (((nb + 1) * 8 + 15) & ~15));
    const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int i = threadIdx.x; i < nb * nb; i += blockDim.x) h2[i] = 0.0;
    for (int i = threadIdx.x; i <= nb; i += blockDim.x) e2[i] = edges2[i];
    __syncthreads();
    const double inv2 = (double)nb / (e2[nb] - e2[0]);
    auto bin_of = [&](double v) {  // sample_analysis_kernel's
        if (!(v >= e2[0])) return -1;
        if (v >= e2[nb]) return v == e2[nb] ? nb - 1 : nb;
        return bin_near(e2, nb, inv2, v);
    };
    const float hb = (float)half_box;
    const double mx = h->max_lw, s1 = h->s1;
    for (int64_t m0 = (int64_t)blockIdx.x * 4; m0 < M; m0 += (int64_t)gridDim.x * 4) {
        const int64_t m = m0 + wid;
        if (m >= M) continue;  // wave-uniform
        const double w = iw_weight(log_w[m], mx, s1);
        if (!(w > 0.0)) continue;  // wave-uniform
        const float *q = cfg + m * (int64_t)N * 2;
        int bin = -1;  // N <= 64: one particle per lane
        if (lane < N) {
            const float cx = q[2 * lane] - hb, cy = q[2 * lane + 1] - hb;
            const int bx = bin_of((double)cx), by = bin_of((double)cy);
            if (bx >= 0 && bx < nb && by >= 0 && by < nb) bin = bx * nb + by;
        }
        // the configuration's particles of one bin are counted first and added once, as
        // w~ * count by the first of their lanes: one rounded add per configuration and bin
        int cnt = 0;
        bool first = true;
        for (int l = 0; l < N; ++l) {
            const int other = __builtin_amdgcn_readlane(bin, l);  // l is wave-uniform: v_readlane_b32
            if (other == bin) {
                ++cnt;
                first = first && l >= lane;
            }
        }
        if (bin >= 0 && first) atomicAdd(&h2[bin], w * (double)cnt);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nb * nb; i += blockDim.x)
        if (h2[i] != 0.0) atomicAdd(&hist[i], h2[i]);
}

// ---------------------------------------------------------------------------------------
// Chain diagnostics (flowstate.h, "Chain diagnostics"; not in the reference): a recorded
// [T][C] series per observable of the batched engine's chains, and of those the per-chain
// autocovariance, Sokal's windowed autocorrelation time, the pooled curve / R-hat terms and
// the well hops.
// ---------------------------------------------------------------------------------------

__device__ inline bool finite_d(double v) { return fabs(v) < INFINITY; }  // false for NaN

__device__ inline int wave_sum_int(int v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// every thread returns the sum over the 256 threads
__device__ inline long long block_sum_i(long long v, long long *redi) {
    const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63;
    v = wave_sum_i(v);
    __syncthreads();
    if (lane == 0) redi[wid] = v;
    __syncthreads();
    return redi[0] + redi[1] + redi[2] + redi[3];
}

// classify_kernel<T>'s classes and mean x of one chain whose values sit in float64 storage
template <typename T>
__device__ inline void observe_chain(const double *q, int N, int lane, double half_box, double r0, bool want_avg,
                                     int &n_a, int &n_b, double &avg_x) {
    const WellTest<T> w(half_box, r0);
    int a = 0, b = 0;
    for (int i = lane; i < N; i += 64) {
        const int k = w.classify((T)q[2 * i], (T)q[2 * i + 1]);
        a += k == 0;
        b += k == 1;
    }
    n_a = wave_sum_int(a);
    n_b = wave_sum_int(b);
    if (want_avg && lane == 0) {
        const T s = pairwise_sum_dev<T>([&](int64_t i) { return (T)q[2 * i]; }, N);
        avg_x = (double)(s / (T)N);
    }
}

// row t of the series from the engine's live arrays: well_stats_kernel's arrangement, one
// wave per chain in that chain's reference dtype
__global__ void __launch_bounds__(256) chain_observe_kernel(const double *__restrict__ pos,
                                                            const uint8_t *__restrict__ is_f32,
                                                            const double *__restrict__ E,
                                                            const double *__restrict__ W,
                                                            const uint8_t *__restrict__ accept, int64_t C, int N,
                                                            double half_box, double r0, int64_t t, int64_t ld,
                                                            fs_chain_series out) {
    const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t c = (int64_t)blockIdx.x * 4 + wid;
    if (c >= C) return;
    const int64_t row = t * ld + c;
    if (out.avg_x || out.n_a || out.n_b) {
        const double *q = pos + c * (int64_t)N * 2;
        int n_a = 0, n_b = 0;
        double avg_x = 0.0;
        if (is_f32 && is_f32[c]) observe_chain<float>(q, N, lane, half_box, r0, out.avg_x != nullptr, n_a, n_b, avg_x);
        else observe_chain<double>(q, N, lane, half_box, r0, out.avg_x != nullptr, n_a, n_b, avg_x);
        if (lane == 0) {
            if (out.avg_x) out.avg_x[row] = avg_x;
            if (out.n_a) out.n_a[row] = (uint8_t)n_a;
            if (out.n_b) out.n_b[row] = (uint8_t)n_b;
        }
    }
    if (lane == 0) {
        if (out.E) out.E[row] = E[c];
        if (out.W) out.W[row] = W[c];
        if (out.accept) out.accept[row] = accept[c];
    }
}

// Per-chain mean and autocovariance.  A workgroup owns 64 chains (lane = chain: a row of the
// series is one coalesced 512-byte read) and one block of kAcLagBlock lags; each of its 8
// waves owns kAcR of those lags with their accumulators in registers for the whole series, so
// the order of every (chain, lag) sum is the definition's whatever the tiling.  Per time tile
// the workgroup stages the deviations d_t of the tile's rows and of the lag block's shifted
// rows in LDS; a wave then reads d_t and ONE new shifted value per step and keeps the other
// kAcR - 1 in a rotating register window (the step loop is unrolled kAcR times, so the window
// is renamed, never moved).  Steps near the end of the series, where some of the wave's lags
// have run out of rows, take the per-lag guarded loop.  Every wave sums the mean itself (the
// same bits in each; the other seven hit the cache), so nothing is handed over.
constexpr int kAcWaves = 8, kAcR = 16, kAcTile = 64;
constexpr int kAcLagBlock = kAcWaves * kAcR;           // 128 lags per workgroup
constexpr int kAcShRows = kAcTile + kAcLagBlock - 1;   // shifted rows a tile can touch
constexpr int kAcLdsBytes = (kAcTile + kAcShRows) * 64 * 8;  // 130,560
static_assert(kAcTile % kAcR == 0 && kAcLdsBytes <= 160 * 1024, "autocovariance tiling");

template <typename X>
__global__ void __launch_bounds__(kAcWaves * 64) chain_autocov_kernel(const X *__restrict__ x, int64_t T, int64_t C,
                                                                      int64_t ld, int W, double *__restrict__ mean,
                                                                      double *__restrict__ acov) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double *base = (double *)smem;        // [kAcTile][64]    d of rows t0 + r
    double *sh = base + kAcTile * 64;     // [kAcShRows][64]  d of rows t0 + kb + r
    const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t c = (int64_t)blockIdx.x * 64 + lane;
    const bool live = c < C;
    const X *col = x + (live ? c : C - 1);  // idle lanes read the last chain and store nothing

    const double x0 = (double)col[0];
    double s = x0, mn = x0, mx = x0;  // min / max keep a NaN once seen
#pragma unroll 8
    for (int64_t t = 1; t < T; ++t) {
        const double v = (double)col[t * ld];
        s += v;
        mn = (v < mn || v != v) ? v : mn;
        mx = (v > mx || v != v) ? v : mx;
    }
    const bool constant = mn == mx;
    const double m = constant ? x0 : s / (double)T;

    const int kb = (int)blockIdx.y * kAcLagBlock, k0 = kb + wid * kAcR;
    const bool active = k0 <= W;  // wave-uniform
    double a[kAcR];
#pragma unroll
    for (int j = 0; j < kAcR; ++j) a[j] = 0.0;
    const double *bp = base + lane, *sp = sh + wid * kAcR * 64 + lane;

    for (int64_t t0 = 0; t0 < T - kb; t0 += kAcTile) {  // while the block's first lag has rows left
        __syncthreads();
        for (int r = wid; r < kAcTile; r += kAcWaves) {
            const int64_t g = t0 + r;
            base[r * 64 + lane] = g < T ? (double)col[g * ld] - m : 0.0;
        }
        for (int r = wid; r < kAcShRows; r += kAcWaves) {
            const int64_t g = t0 + kb + r;
            sh[r * 64 + lane] = g < T ? (double)col[g * ld] - m : 0.0;
        }
        __syncthreads();
        if (!active) continue;
        // step i of the tile has rows for lag k0 + j while i + j < lim
        const int64_t lim = T - k0 - t0, limf = lim - (kAcR - 1);
        const int nstep = lim >= kAcTile ? kAcTile : (lim > 0 ? (int)lim : 0);
        const int nfast = limf >= kAcTile ? kAcTile : (limf > 0 ? (int)(limf / kAcR) * kAcR : 0);
        if (nfast > 0) {
            double w[kAcR];  // w[(u + j) % kAcR] = shifted row i + u + j at step i + u
#pragma unroll
            for (int j = 0; j < kAcR - 1; ++j) w[j] = sp[j * 64];
            w[kAcR - 1] = 0.0;
            for (int i = 0; i < nfast; i += kAcR) {
#pragma unroll
                for (int u = 0; u < kAcR; ++u) {
                    w[(u + kAcR - 1) % kAcR] = sp[(i + u + kAcR - 1) * 64];
                    const double d = bp[(i + u) * 64];
#pragma unroll
                    for (int j = 0; j < kAcR; ++j) {
                        const double p = d * w[(u + j) % kAcR];
                        a[j] += p;
                    }
                }
            }
        }
        for (int i = nfast; i < nstep; ++i) {
            const double d = bp[i * 64];
#pragma unroll
            for (int j = 0; j < kAcR; ++j)
                if (i + j < lim) {
                    const double p = d * sp[(i + j) * 64];
                    a[j] += p;
                }
        }
    }
    if (!live) return;
    if (blockIdx.y == 0 && wid == 0) mean[c] = m;
    if (active) {
#pragma unroll
        for (int j = 0; j < kAcR; ++j)
            if (k0 + j <= W) acov[(int64_t)(k0 + j) * C + c] = constant ? 0.0 : a[j] / (double)T;
    }
}

// Sokal's automatic window, one lane per chain
__global__ void __launch_bounds__(256) chain_tau_kernel(const double *__restrict__ mean,
                                                        const double *__restrict__ acov, int64_t C, int W,
                                                        double c_window, double *__restrict__ tau,
                                                        int32_t *__restrict__ window, uint8_t *__restrict__ flags) {
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    const double v0 = acov[c];
    double t = 0.0;
    int win = 0;
    uint8_t fl;
    if (!finite_d(mean[c]) || !finite_d(v0)) fl = 4;
    else if (v0 == 0.0) fl = 1;
    else {
        fl = 2;
        win = W;
        t = 0.5;
        for (int k = 1; k <= W; ++k) {
            t += acov[(int64_t)k * C + c] / v0;
            if ((double)k >= c_window * t) {
                win = k;
                fl = 0;
                break;
            }
        }
    }
    tau[c] = t;
    window[c] = win;
    flags[c] = fl;
}

// Across chains: workgroup k <= W the pooled autocovariance of lag k, workgroup W + 1 the
// R-hat terms.  weighted_reduce_kernel's fixed order (thread t adds chains t, t + 256, .., then
// block_sum's tree); chains with a non-finite mean or variance are skipped everywhere.
__global__ void __launch_bounds__(256) chain_pool_kernel(const double *__restrict__ mean,
                                                         const double *__restrict__ acov, int64_t C, int W,
                                                         int64_t T, double *__restrict__ pooled,
                                                         double *__restrict__ scalars) {
    __shared__ double red[4];
    __shared__ long long redi[4];
    auto used = [&](int64_t c) { return finite_d(mean[c]) && finite_d(acov[c]); };
    long long cnt = 0;
    for (int64_t c = threadIdx.x; c < C; c += 256) cnt += used(c);
    const long long n = block_sum_i(cnt, redi);
    const double dn = (double)n;
    const int k = blockIdx.x;
    if (k <= W) {
        double s = 0.0;
        for (int64_t c = threadIdx.x; c < C; c += 256)
            if (used(c)) s += acov[(int64_t)k * C + c];
        s = block_sum(s, red);
        if (threadIdx.x == 0) pooled[k] = n > 0 ? s / dn : 0.0;
        return;
    }
    double sm = 0.0, sw = 0.0;
    const double dT = (double)T, dT1 = (double)(T - 1);
    for (int64_t c = threadIdx.x; c < C; c += 256)
        if (used(c)) {
            sm += mean[c];
            if (T >= 2) sw += acov[c] * dT / dT1;
        }
    sm = block_sum(sm, red);
    sw = block_sum(sw, red);
    const double gm = n > 0 ? sm / dn : 0.0;
    double sv = 0.0;
    for (int64_t c = threadIdx.x; c < C; c += 256)
        if (used(c)) {
            const double d = mean[c] - gm;
            sv += d * d;
        }
    sv = block_sum(sv, red);
    if (threadIdx.x == 0) {
        scalars[0] = gm;
        scalars[1] = n >= 2 ? sv / (double)(n - 1) : 0.0;
        scalars[2] = n > 0 ? sw / dn : 0.0;
        scalars[3] = dn;
    }
}

// calculate_well_statistics' all-in-A / all-in-B rule along time, one lane per chain
__global__ void __launch_bounds__(256) chain_transitions_kernel(const uint8_t *__restrict__ n_a,
                                                                const uint8_t *__restrict__ n_b, int64_t T, int64_t C,
                                                                int64_t ld, int N, long long *__restrict__ out) {
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    long long steps[3] = {0, 0, 0}, ab = 0, ba = 0;  // steps: neither, A, B
    int last = 0;
#pragma unroll 4
    for (int64_t t = 0; t < T; ++t) {
        const int st = n_a[t * ld + c] == N ? 1 : (n_b[t * ld + c] == N ? 2 : 0);
        steps[0] += st == 0;
        steps[1] += st == 1;
        steps[2] += st == 2;
        if (st != 0) {
            if (last != 0 && st != last) {
                ab += st == 2;
                ba += st == 1;
            }
            last = st;
        }
    }
    long long *o = out + c * 6;
    o[0] = steps[1];
    o[1] = steps[2];
    o[2] = steps[0];
    o[3] = ab;
    o[4] = ba;
    o[5] = last;
}

}  // namespace fs

using namespace fs;

hipError_t fs_sample_analysis_impl(const float *z, int64_t M, int N, double half_box, const double *edges2, int nb,
                                   const double *edges_r, int nr, float *out, int64_t *hist, int32_t *counts,
                                   hipStream_t st) {
    if (M <= 0) return hipSuccess;
    static std::atomic<unsigned long long> lds_done{0};
    if (hipError_t e = fs_set_max_lds_once((const void *)sample_analysis_kernel, lds_done); e != hipSuccess) return e;
    int dev = 0, cus = 256;
    if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    const int64_t want = (M + 3) / 4, cap = 2 * (int64_t)cus;
    const unsigned blocks = (unsigned)(want < cap ? want : cap);
    hipLaunchKernelGGL(sample_analysis_kernel, dim3(blocks), dim3(256), (size_t)sa_lds(nb, nr).bytes, st, z, M, N,
                       half_box, edges2, nb, edges_r, nr, out, (unsigned long long *)hist, counts);
    return hipGetLastError();
}

hipError_t fs_classify_wells_impl(const void *pos, int f32, int64_t M, int N, double half_box, double r0,
                                  uint8_t *cls, uint8_t *state, double *avg_x, hipStream_t st) {
    if (M <= 0) return hipSuccess;
    const dim3 grid((unsigned)((M + 3) / 4));
    if (f32)
        hipLaunchKernelGGL(classify_kernel<float>, grid, dim3(256), 0, st, (const float *)pos, M, N, half_box, r0, cls,
                           state, avg_x);
    else
        hipLaunchKernelGGL(classify_kernel<double>, grid, dim3(256), 0, st, (const double *)pos, M, N, half_box, r0,
                           cls, state, avg_x);
    return hipGetLastError();
}

hipError_t fs_well_stats_impl(const double *pos, const uint8_t *is_f32, int64_t C, int N, double half_box, double r0,
                              int64_t *counts, hipStream_t st) {
    if (C <= 0) return hipSuccess;
    hipLaunchKernelGGL(well_stats_kernel, dim3((unsigned)((C + 3) / 4)), dim3(256), 0, st, pos, is_f32, C, N, half_box,
                       r0, (long long *)counts);
    return hipGetLastError();
}

hipError_t fs_pair_hist_impl(const void *pos, int f32, int64_t M, int N, double bound, const double *edges, int nb,
                             int32_t *counts, hipStream_t st) {
    if (M <= 0) return hipSuccess;
    const dim3 grid((unsigned)((M + 3) / 4));
    if (f32)
        hipLaunchKernelGGL(pair_hist_kernel<float>, grid, dim3(256), 0, st, (const float *)pos, M, N, bound, edges, nb,
                           counts);
    else
        hipLaunchKernelGGL(pair_hist_kernel<double>, grid, dim3(256), 0, st, (const double *)pos, M, N, bound, edges,
                           nb, counts);
    return hipGetLastError();
}

hipError_t fs_rdf_mean_impl(const int32_t *counts, int64_t M, int nb, const double *denom, double *g, hipStream_t st) {
    if (nb <= 0) return hipSuccess;
    hipLaunchKernelGGL(rdf_mean_kernel, dim3((unsigned)((nb + 63) / 64)), dim3(64), 0, st, counts, M, nb, denom, g);
    return hipGetLastError();
}

int64_t fs_iw_state_bytes_impl() { return (int64_t)sizeof(IwHeader) + (int64_t)kIwSlots * (int64_t)sizeof(IwSlot); }

hipError_t fs_iw_reset_impl(void *state, hipStream_t st) {
    hipLaunchKernelGGL(iw_reset_kernel, dim3(1), dim3(64), 0, st, (IwHeader *)state);
    return hipGetLastError();
}

hipError_t fs_importance_weights_impl(double beta, int64_t M, const double *E, const float *log_q, double *log_w,
                                      void *state, hipStream_t st) {
    if (M <= 0) return hipSuccess;
    IwHeader *h = (IwHeader *)state;
    IwSlot *slots = (IwSlot *)(h + 1);
    // the grid is a function of M alone (never of the CU count): the same bits on any device
    const int64_t want = (M + 255) / 256;
    const int P = (int)(want < kIwSlots ? want : kIwSlots);
    hipLaunchKernelGGL(iw_partial_kernel, dim3((unsigned)P), dim3(256), 0, st, beta, M, E, log_q, log_w, slots);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    hipLaunchKernelGGL(iw_finish_kernel, dim3(1), dim3(64), 0, st, h, (const IwSlot *)slots, P, M);
    return hipGetLastError();
}

hipError_t fs_weighted_reduce_impl(const int32_t *counts, int64_t M, int nr, const double *denom,
                                   const uint8_t *wstate, const double *avg_x, const double *log_w, const void *state,
                                   double *g_w, double *scalars, hipStream_t st) {
    if (M <= 0) return hipSuccess;
    hipLaunchKernelGGL(weighted_reduce_kernel, dim3((unsigned)(nr + 1)), dim3(256), 0, st, counts, M, nr, denom, wstate,
                       avg_x, log_w, (const IwHeader *)state, g_w, scalars);
    return hipGetLastError();
}

hipError_t fs_weighted_hist2d_impl(const float *cfg, int64_t M, int N, double half_box, const double *edges2, int nb,
                                   const double *log_w, const void *state, double *hist, hipStream_t st) {
    if (M <= 0) return hipSuccess;
    static std::atomic<unsigned long long> lds_done{0};
    if (hipError_t e = fs_set_max_lds_once((const void *)weighted_hist2d_kernel, lds_done); e != hipSuccess) return e;
    int dev = 0, cus = 256;
    if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    const int64_t want = (M + 3) / 4, cap = 2 * (int64_t)cus;  // the one sum whose order is free
    const unsigned blocks = (unsigned)(want < cap ? want : cap);
    hipLaunchKernelGGL(weighted_hist2d_kernel, dim3(blocks), dim3(256), (size_t)wh_lds_bytes(nb), st, cfg, M, N,
                       half_box, edges2, nb, log_w, (const IwHeader *)state, hist);
    return hipGetLastError();
}

hipError_t fs_chain_observe_impl(const double *state, const uint8_t *is_f32, const double *E, const double *W,
                                 const uint8_t *accept, int64_t C, int N, double half_box, double r0, int64_t t,
                                 int64_t ld, const fs_chain_series *out, hipStream_t st) {
    if (C <= 0) return hipSuccess;
    hipLaunchKernelGGL(chain_observe_kernel, dim3((unsigned)((C + 3) / 4)), dim3(256), 0, st, state, is_f32, E, W,
                       accept, C, N, half_box, r0, t, ld, *out);
    return hipGetLastError();
}

hipError_t fs_chain_autocov_impl(const void *x, int dtype, int64_t T, int64_t C, int64_t ld, int W, double *mean,
                                 double *acov, hipStream_t st) {
    if (C <= 0) return hipSuccess;
    static std::atomic<unsigned long long> lds_f64{0}, lds_u8{0};
    const dim3 grid((unsigned)((C + 63) / 64), (unsigned)(W / kAcLagBlock + 1));
    if (dtype == 0) {
        if (hipError_t e = fs_set_max_lds_once((const void *)chain_autocov_kernel<double>, lds_f64); e != hipSuccess)
            return e;
        hipLaunchKernelGGL(chain_autocov_kernel<double>, grid, dim3(kAcWaves * 64), (size_t)kAcLdsBytes, st,
                           (const double *)x, T, C, ld, W, mean, acov);
    } else {
        if (hipError_t e = fs_set_max_lds_once((const void *)chain_autocov_kernel<uint8_t>, lds_u8); e != hipSuccess)
            return e;
        hipLaunchKernelGGL(chain_autocov_kernel<uint8_t>, grid, dim3(kAcWaves * 64), (size_t)kAcLdsBytes, st,
                           (const uint8_t *)x, T, C, ld, W, mean, acov);
    }
    return hipGetLastError();
}

hipError_t fs_chain_tau_impl(const double *mean, const double *acov, int64_t C, int W, double c_window, double *tau,
                             int32_t *window, uint8_t *flags, hipStream_t st) {
    if (C <= 0) return hipSuccess;
    hipLaunchKernelGGL(chain_tau_kernel, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, st, mean, acov, C, W,
                       c_window, tau, window, flags);
    return hipGetLastError();
}

hipError_t fs_chain_pool_impl(const double *mean, const double *acov, int64_t C, int W, int64_t T, double *pooled,
                              double *scalars, hipStream_t st) {
    if (C <= 0) return hipSuccess;
    hipLaunchKernelGGL(chain_pool_kernel, dim3((unsigned)(W + 2)), dim3(256), 0, st, mean, acov, C, W, T, pooled,
                       scalars);
    return hipGetLastError();
}

hipError_t fs_chain_transitions_impl(const uint8_t *n_a, const uint8_t *n_b, int64_t T, int64_t C, int64_t ld, int N,
                                     int64_t *out, hipStream_t st) {
    if (C <= 0) return hipSuccess;
    hipLaunchKernelGGL(chain_transitions_kernel, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, st, n_a, n_b, T, C,
                       ld, N, (long long *)out);
    return hipGetLastError();
}
