// Evaluation metrics on device: what engines/eval.py:31-93 (eval_one_view) and engines/trainer.py:172-195 (the i_print
// block) compute on the host after copying the render off the device -- SSIM (utils/ssim.py:17-38,66-73), the k-means
// clustering of the semantic map (utils/misc.py:40-52, sklearn KMeans) and the adjusted Rand index (sklearn
// adjusted_rand_score).  No float atomics anywhere: every reduction runs in a fixed order, so results are bitwise identical
// from run to run.
#include <math.h>

#include "common.h"

namespace {
constexpr int kThreads = 256;

// ------------------------------------------------------------------------------------------------------------------ SSIM
// One workgroup per 32x16 output tile of one (image, channel) plane.  The zero-padded input tile (halo = window/2, as
// conv2d(padding=window//2)) goes to LDS; the 1-D window is applied horizontally to the five moments (x, y, x^2, y^2, xy) of
// every halo row, in fp64, into LDS, then vertically per output pixel.  The map is formed in registers (fp64) and each block
// writes the fp64 sum of its pixels into a slab; ssim_finish_kernel adds the slab in a fixed order.
constexpr int kSsimTW = 32, kSsimTH = 16;
struct SsimWin {
    float g[32];
};

template <int RMAX>
__global__ __launch_bounds__(kThreads) void ssim_tile_kernel(const float* __restrict__ img1, const float* __restrict__ img2, int H,
                                                             int W, int R, SsimWin win, float* __restrict__ map,
                                                             double* __restrict__ part) {
    constexpr int IW = kSsimTW + 2 * RMAX, IH = kSsimTH + 2 * RMAX;
    __shared__ float sx[IH][IW], sy[IH][IW];
    __shared__ double hs[5][IH][kSsimTW];
    __shared__ double wave_part[kThreads / 64];
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * kSsimTW, y0 = blockIdx.y * kSsimTH;
    const int64_t plane = blockIdx.z;
    const float* a = img1 + plane * H * W;
    const float* b = img2 + plane * H * W;
    const int iw = kSsimTW + 2 * R, ih = kSsimTH + 2 * R, taps = 2 * R + 1;
    for (int i = tid; i < ih * iw; i += kThreads) {
        const int r = i / iw, c = i - r * iw;
        const int gy = y0 - R + r, gx = x0 - R + c;
        const bool in = gy >= 0 && gy < H && gx >= 0 && gx < W;
        sx[r][c] = in ? a[(int64_t)gy * W + gx] : 0.0f;
        sy[r][c] = in ? b[(int64_t)gy * W + gx] : 0.0f;
    }
    __syncthreads();
    for (int i = tid; i < ih * kSsimTW; i += kThreads) {
        const int r = i / kSsimTW, c = i - r * kSsimTW;
        double m0 = 0.0, m1 = 0.0, m2 = 0.0, m3 = 0.0, m4 = 0.0;
        for (int k = 0; k < taps; ++k) {
            const double w = (double)win.g[k], p = (double)sx[r][c + k], q = (double)sy[r][c + k];
            m0 += w * p;
            m1 += w * q;
            m2 += w * (p * p);
            m3 += w * (q * q);
            m4 += w * (p * q);
        }
        hs[0][r][c] = m0;
        hs[1][r][c] = m1;
        hs[2][r][c] = m2;
        hs[3][r][c] = m3;
        hs[4][r][c] = m4;
    }
    __syncthreads();
    double acc = 0.0;
    const double C1 = 0.01 * 0.01, C2 = 0.03 * 0.03;
    for (int i = tid; i < kSsimTH * kSsimTW; i += kThreads) {
        const int r = i / kSsimTW, c = i - r * kSsimTW;
        const int gy = y0 + r, gx = x0 + c;
        if (gy >= H || gx >= W) continue;
        double m[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
        for (int k = 0; k < taps; ++k) {
            const double w = (double)win.g[k];
            for (int q = 0; q < 5; ++q) m[q] += w * hs[q][r + k][c];
        }
        const double mu1 = m[0], mu2 = m[1], mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu12 = mu1 * mu2;
        const double s1 = m[2] - mu1_sq, s2 = m[3] - mu2_sq, s12 = m[4] - mu12;
        const double v = ((2.0 * mu12 + C1) * (2.0 * s12 + C2)) / ((mu1_sq + mu2_sq + C1) * (s1 + s2 + C2));
        if (map) map[plane * H * W + (int64_t)gy * W + gx] = (float)v;
        acc += v;
    }
    acc = nsos_wave_sum(acc);
    if ((tid & 63) == 0) wave_part[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0)
        part[(plane * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = ((wave_part[0] + wave_part[1]) + wave_part[2]) + wave_part[3];
}

// block g sums the slab entries [g * per, (g + 1) * per) in a fixed order; out[g] = sum / count (fp32, as the reference's mean)
__global__ __launch_bounds__(kThreads) void ssim_finish_kernel(const double* __restrict__ part, int64_t per, double count,
                                                               float* __restrict__ out) {
    __shared__ double wave_part[kThreads / 64];
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < per; i += kThreads) s += part[blockIdx.x * per + i];
    s = nsos_wave_sum(s);
    if ((threadIdx.x & 63) == 0) wave_part[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) out[blockIdx.x] = (float)((((wave_part[0] + wave_part[1]) + wave_part[2]) + wave_part[3]) / count);
}

// ------------------------------------------------------------------------------------------------------------------- ARI
// Contingency table of labels in [0, 64) x [0, 64): per block in LDS (uint32), flushed with integer atomics into a uint64
// table (order-free: integer sums are exact).  Pairs of labels < 4 -- the common 2-class case -- are counted with one ballot
// and popcount per bin instead of contended LDS atomics.
constexpr int kAriL = 64;
constexpr int kAriBlocks = 512;

template <typename T>
__device__ __forceinline__ int ari_label(T v) {
    return (v >= (T)0 && v < (T)kAriL) ? (int)v : -1;
}
template <>
__device__ __forceinline__ int ari_label<uint8_t>(uint8_t v) {
    return v < kAriL ? (int)v : -1;
}
template <>
__device__ __forceinline__ int ari_label<float>(float v) {
    return (v >= 0.0f && v < (float)kAriL && v == floorf(v)) ? (int)v : -1;   // NaN fails the first test
}

template <typename T>
__global__ __launch_bounds__(kThreads) void ari_count_kernel(const T* __restrict__ lt, const T* __restrict__ lp, int64_t n,
                                                             unsigned long long* __restrict__ table) {
    __shared__ unsigned int tab[kAriL * kAriL];
    __shared__ unsigned int bad;
    for (int i = threadIdx.x; i < kAriL * kAriL; i += kThreads) tab[i] = 0u;
    if (threadIdx.x == 0) bad = 0u;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    unsigned int small = 0u, nbad = 0u;
    const int64_t stride = (int64_t)gridDim.x * kThreads;
    // every lane runs the same trip count: the ballots below need the whole wave
    const int64_t base0 = (int64_t)blockIdx.x * kThreads + (threadIdx.x & ~63);
    for (int64_t base = base0; base < n; base += stride) {
        const int64_t i = base + lane;
        int code = -2;   // -2: no element, -1: invalid, 0..15: both < 4, 16: table atomics
        if (i < n) {
            const int t = ari_label<T>(lt[i]), p = ari_label<T>(lp[i]);
            if (t < 0 || p < 0) code = -1;
            else if (t < 4 && p < 4) code = t * 4 + p;
            else {
                code = 16;
                atomicAdd(&tab[t * kAriL + p], 1u);
            }
        }
        if (code == -1) ++nbad;
        for (int bin = 0; bin < 16; ++bin) {
            const unsigned long long m = __ballot(code == bin);
            if (lane == bin) small += (unsigned int)__popcll(m);
        }
    }
    if (lane < 16 && small) atomicAdd(&tab[(lane >> 2) * kAriL + (lane & 3)], small);
    if (nbad) atomicAdd(&bad, nbad);
    __syncthreads();
    for (int i = threadIdx.x; i < kAriL * kAriL; i += kThreads)
        if (tab[i]) atomicAdd(&table[i], (unsigned long long)tab[i]);
    if (threadIdx.x == 0 && bad) atomicAdd(&table[kAriL * kAriL], (unsigned long long)bad);
}

// sklearn.metrics.adjusted_rand_score via pair_confusion_matrix (ordered pair counts):
//   tp = sum n_ij^2 - n, fp = sum n_ij n_.j - sum n_ij^2, fn = sum n_ij n_i. - sum n_ij^2, tn = n^2 - fp - fn - sum n_ij^2;
//   fn == fp == 0 -> 1.0, else 2 * (tp tn - fn fp) / ((tp + fn)(fn + tn) + (tp + fp)(fp + tn)) with Python's int -> float roundings.
__device__ double ari_from_counts(long long n, long long ss, long long sk, long long sc) {
    const long long tp = ss - n, fp = sk - ss, fn = sc - ss, tn = n * n - fp - fn - ss;
    if (fn == 0 && fp == 0) return 1.0;
    const __int128 num = (__int128)tp * tn - (__int128)fn * fp;
    const __int128 den = (__int128)(tp + fn) * (fn + tn) + (__int128)(tp + fp) * (fp + tn);
    return (2.0 * (double)num) / (double)den;
}

__global__ __launch_bounds__(kThreads) void ari_finish_kernel(const unsigned long long* __restrict__ table, int subset,
                                                              double* __restrict__ out) {
    __shared__ long long rows[kAriL], cols[kAriL];
    __shared__ unsigned long long acc[6];
    const int tid = threadIdx.x;
    if (tid < 6) acc[tid] = 0ull;
    if (tid < kAriL) {
        long long s = 0;
        for (int j = 0; j < kAriL; ++j) s += (long long)table[tid * kAriL + j];
        rows[tid] = s;
    } else if (tid < 2 * kAriL) {
        long long s = 0;
        for (int i = 0; i < kAriL; ++i) s += (long long)table[i * kAriL + tid - kAriL];
        cols[tid - kAriL] = s;
    }
    __syncthreads();
    long long ss = 0, sk = 0, sc = 0, ss_f = 0, sc_f = 0;
    for (int e = tid; e < kAriL * kAriL; e += kThreads) {
        const long long v = (long long)table[e];
        if (!v) continue;
        const int i = e / kAriL, j = e - i * kAriL;
        ss += v * v;
        sk += v * cols[j];
        sc += v * rows[i];
        if (i == subset) {   // the table restricted to labels_true == subset: one row; its column sums are the row itself
            ss_f += v * v;
            sc_f += v * rows[i];
        }
    }
    atomicAdd(&acc[0], (unsigned long long)ss);
    atomicAdd(&acc[1], (unsigned long long)sk);
    atomicAdd(&acc[2], (unsigned long long)sc);
    atomicAdd(&acc[3], (unsigned long long)ss_f);
    atomicAdd(&acc[4], (unsigned long long)sc_f);
    __syncthreads();
    if (tid == 0) {
        long long n = 0;
        for (int i = 0; i < kAriL; ++i) n += rows[i];
        const long long nf = (subset >= 0 && subset < kAriL) ? rows[subset] : 0;
        const bool bad = table[kAriL * kAriL] != 0ull;
        const double full = ari_from_counts(n, (long long)acc[0], (long long)acc[1], (long long)acc[2]);
        const double fg = ari_from_counts(nf, (long long)acc[3], (long long)acc[3], (long long)acc[4]);
        out[0] = bad ? __longlong_as_double(0x7ff8000000000000ll) : full;
        out[1] = bad ? __longlong_as_double(0x7ff8000000000000ll) : fg;
    }
}

// ---------------------------------------------------------------------------------------------------------------- k-means
// sklearn 1.x KMeans(algorithm="lloyd") on B independent problems x [B,N,C].  Every Lloyd step is split into the same two
// block-level pieces in both regimes:
//   km_assign_chunk: one workgroup, 1024 points (point = chunk*1024 + j*256 + thread, j = 0..3): nearest center (fp32 squared
//     distance, ties to the lowest index), label change count, and per-cluster fp64 sums / counts reduced in a fixed order into
//     the chunk's record of the slab;
//   km_finish: one workgroup adds the records in chunk order, relocates empty clusters, forms the new centers, tests convergence.
// The workgroup regime (km_wg_kernel) runs both in one launch per problem; the grid regime launches one assign pass over all
// chunks and one finish per iteration.  Same functions, same orders: the two regimes give bitwise-equal results.
constexpr int kKmMaxK = 16, kKmMaxC = 16;
constexpr int kKmChunk = 4 * kThreads;
constexpr int kKmGroup = 8;   // grid regime: iterations launched between two reads of the done word

struct KmState {
    float centers[kKmMaxK * kKmMaxC];
    double tol;      // tol * mean of the per-feature variances of X
    int32_t iter, done, strict, pad;
    int32_t perm[kKmMaxK];
};
constexpr size_t kKmStateBytes = (sizeof(KmState) + 15) / 16 * 16;

__host__ __device__ inline int64_t km_chunks(int64_t n) { return (n + kKmChunk - 1) / kKmChunk; }
__host__ __device__ constexpr int km_rec(int K, int C) { return K * C + K + 2; }   // sums [K*C], counts [K], changed, inertia
__host__ __device__ inline size_t km_problem_bytes(int64_t n, int K, int C) {
    return kKmStateBytes + (size_t)((n + 3) / 4 * 4) * sizeof(float) + (size_t)km_chunks(n) * km_rec(K, C) * sizeof(double);
}

struct KmProblem {
    const float* x;
    int32_t* labels;
    KmState* st;
    float* dist;
    double* slab;
};
__device__ inline KmProblem km_problem(const float* x, int32_t* labels, unsigned char* ws, int64_t b, int64_t n, int K, int C) {
    unsigned char* base = ws + (size_t)b * km_problem_bytes(n, K, C);
    KmProblem p;
    p.x = x + b * n * C;
    p.labels = labels + b * n;
    p.st = reinterpret_cast<KmState*>(base);
    p.dist = reinterpret_cast<float*>(base + kKmStateBytes);
    p.slab = reinterpret_cast<double*>(base + kKmStateBytes + (size_t)((n + 3) / 4 * 4) * sizeof(float));
    return p;
}

// The random stream of the k-means++ seeding: a counter-based hash (splitmix64's finaliser) of
// (seed, problem, round, trial, point):  s = mix(mix(mix(seed) ^ problem) ^ (round << 8 | trial)),
// u = ((mix(s ^ point) >> 40) + 1) / 2^24, uniform on (0, 1].
__device__ __forceinline__ uint64_t km_mix(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}
__device__ __forceinline__ float km_uniform(uint64_t stream, int64_t i) {
    return (float)((km_mix(stream ^ (uint64_t)i) >> 40) + 1ull) * (1.0f / 16777216.0f);
}

__device__ __forceinline__ float km_d2(const float* __restrict__ x, const float* c, int C) {
    float d = 0.0f;
    for (int k = 0; k < C; ++k) {
        const float t = x[k] - c[k];
        d += t * t;
    }
    return d;
}

// block-wide sum of v (fixed order: wave sums, then the four waves in order); every thread receives it
__device__ double km_block_sum(double v, double* red) {
    v = nsos_wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

// (key, index) minimum, ties to the lowest index
__device__ __forceinline__ void km_argmin_merge(float& k, int64_t& i, float k2, int64_t i2) {
    if (k2 < k || (k2 == k && i2 < i)) {
        k = k2;
        i = i2;
    }
}
__device__ void km_block_argmin(float& key, int64_t& idx, float* rk, int64_t* ri) {
    for (int off = 32; off >= 1; off >>= 1) {
        const float k2 = __shfl_xor(key, off);
        const int64_t i2 = __shfl_xor(idx, off);
        km_argmin_merge(key, idx, k2, i2);
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) {
        rk[threadIdx.x >> 6] = key;
        ri[threadIdx.x >> 6] = idx;
    }
    __syncthreads();
    key = rk[0];
    idx = ri[0];
    for (int w = 1; w < kThreads / 64; ++w) km_argmin_merge(key, idx, rk[w], ri[w]);
}

struct KmShared {
    float centers[kKmMaxK * kKmMaxC];
    double vals[kThreads / 64][km_rec(kKmMaxK, kKmMaxC)];
    double tot[km_rec(kKmMaxK, kKmMaxC)];
    double red[kThreads / 64];
    float rk[kThreads / 64];
    int64_t ri[kThreads / 64];
    int64_t picked[kKmMaxK];
    double pot[8];
    int64_t cand[8];
};

// tol scaling, labels = -1, initial centers (given, or greedy k-means++ with n_trials candidates per round)
__device__ void km_seed(const KmProblem& p, int64_t n, int C, int K, const float* init, uint64_t seed, int64_t problem,
                        int n_trials, double tol, int max_iter, KmShared& sh) {
    const int tid = threadIdx.x;
    for (int64_t i = tid; i < n; i += kThreads) p.labels[i] = -1;
    // sklearn _tolerance: mean over features of var(X[:, f]), times tol (two-pass, fp64)
    double var_sum = 0.0;
    for (int c = 0; c < C; ++c) {
        double s = 0.0;
        for (int64_t i = tid; i < n; i += kThreads) s += (double)p.x[i * C + c];
        const double mean = km_block_sum(s, sh.red) / (double)n;
        double q = 0.0;
        for (int64_t i = tid; i < n; i += kThreads) {
            const double d = (double)p.x[i * C + c] - mean;
            q += d * d;
        }
        var_sum += km_block_sum(q, sh.red) / (double)n;
    }
    if (init) {
        for (int v = tid; v < K * C; v += kThreads) p.st->centers[v] = init[v];
    } else {
        const uint64_t s0 = km_mix(km_mix(seed) ^ (uint64_t)problem);
        // first center: uniform (the race with equal weights)
        float key = INFINITY;
        int64_t idx = n;
        {
            const uint64_t stream = km_mix(s0 ^ 0ull);
            for (int64_t i = tid; i < n; i += kThreads) km_argmin_merge(key, idx, -logf(km_uniform(stream, i)), i);
        }
        km_block_argmin(key, idx, sh.rk, sh.ri);
        if (tid < C) sh.centers[tid] = p.x[idx * C + tid];
        __syncthreads();
        for (int64_t i = tid; i < n; i += kThreads) p.dist[i] = km_d2(p.x + i * C, sh.centers, C);
        for (int r = 1; r < K; ++r) {
            // n_trials candidates, each drawn with probability ~ D^2 by the exponential race argmin_i -ln(u_i) / D^2_i
            for (int t = 0; t < n_trials; ++t) {
                const uint64_t stream = km_mix(s0 ^ (uint64_t)((r << 8) | t));
                key = INFINITY;
                idx = n;
                for (int64_t i = tid; i < n; i += kThreads) {
                    const float w = p.dist[i];
                    km_argmin_merge(key, idx, w > 0.0f ? -logf(km_uniform(stream, i)) / w : INFINITY, i);
                }
                km_block_argmin(key, idx, sh.rk, sh.ri);
                if (tid == 0) sh.cand[t] = idx;
            }
            __syncthreads();
            // the potential of each candidate; keep the lowest (first on ties)
            for (int t = 0; t < n_trials; ++t) {
                const float* cx = p.x + sh.cand[t] * C;
                double q = 0.0;
                for (int64_t i = tid; i < n; i += kThreads) q += (double)fminf(p.dist[i], km_d2(p.x + i * C, cx, C));
                q = km_block_sum(q, sh.red);
                if (tid == 0) sh.pot[t] = q;
            }
            __syncthreads();
            int best = 0;
            for (int t = 1; t < n_trials; ++t)
                if (sh.pot[t] < sh.pot[best]) best = t;
            const float* bx = p.x + sh.cand[best] * C;
            if (tid < C) sh.centers[r * C + tid] = bx[tid];
            for (int64_t i = tid; i < n; i += kThreads) p.dist[i] = fminf(p.dist[i], km_d2(p.x + i * C, bx, C));
            __syncthreads();
        }
        for (int v = tid; v < K * C; v += kThreads) p.st->centers[v] = sh.centers[v];
    }
    if (tid == 0) {
        p.st->tol = var_sum / (double)C * tol;
        p.st->iter = 0;
        p.st->done = max_iter == 0;   // seeding only (sklearn.cluster.kmeans_plusplus)
        p.st->strict = 0;
    }
    __syncthreads();
}

// assignment of one chunk (mode 0: Lloyd step, labels updated and change counted; mode 1: final -- relabel unless the loop
// converged strictly, and the inertia of the final labels); writes the chunk's record
__device__ void km_assign_chunk(const KmProblem& p, int64_t n, int C, int K, int64_t chunk, int mode, KmShared& sh) {
    const int tid = threadIdx.x, R = km_rec(K, C);
    for (int v = tid; v < K * C; v += kThreads) sh.centers[v] = p.st->centers[v];
    __syncthreads();
    const bool relabel = mode == 0 || !p.st->strict;
    int lab[4];
    float dmin[4];
    int changed = 0;
    for (int j = 0; j < 4; ++j) {
        const int64_t i = chunk * kKmChunk + j * kThreads + tid;
        lab[j] = -1;
        dmin[j] = 0.0f;
        if (i >= n) continue;
        const float* xi = p.x + i * C;
        if (relabel) {
            int best = 0;
            float bd = km_d2(xi, sh.centers, C);
            for (int k = 1; k < K; ++k) {
                const float d = km_d2(xi, sh.centers + k * C, C);
                if (d < bd) {
                    bd = d;
                    best = k;
                }
            }
            if (p.labels[i] != best) ++changed;
            p.labels[i] = best;
            lab[j] = best;
            dmin[j] = bd;
        } else {
            lab[j] = p.labels[i];
            dmin[j] = km_d2(xi, sh.centers + lab[j] * C, C);
        }
    }
    const int w = tid >> 6;
    for (int v = 0; v < R; ++v) {
        double s = 0.0;
        if (v < K * C) {
            const int k = v / C, c = v - k * C;
            for (int j = 0; j < 4; ++j)
                if (lab[j] == k) s += (double)p.x[(chunk * kKmChunk + j * kThreads + tid) * C + c];
        } else if (v < K * C + K) {
            for (int j = 0; j < 4; ++j) s += lab[j] == v - K * C ? 1.0 : 0.0;
        } else if (v == K * C + K) {
            s = (double)changed;
        } else {
            for (int j = 0; j < 4; ++j) s += (double)dmin[j];
        }
        s = nsos_wave_sum(s);
        if ((tid & 63) == 0) sh.vals[w][v] = s;
    }
    __syncthreads();
    double* rec = p.slab + chunk * R;
    for (int v = tid; v < R; v += kThreads) rec[v] = ((sh.vals[0][v] + sh.vals[1][v]) + sh.vals[2][v]) + sh.vals[3][v];
    __syncthreads();
}

// the records of all chunks added in chunk order into sh.tot (thread v owns value v)
__device__ void km_total(const KmProblem& p, int64_t n, int C, int K, KmShared& sh) {
    const int R = km_rec(K, C);
    const int64_t nch = km_chunks(n);
    for (int v = threadIdx.x; v < R; v += kThreads) {
        double s = 0.0;
        for (int64_t ch = 0; ch < nch; ++ch) s += p.slab[ch * R + v];
        sh.tot[v] = s;
    }
    __syncthreads();
}

// end of one Lloyd step: relocate empty clusters (sklearn _relocate_empty_clusters_dense: the n_empty points farthest from
// their assigned center, largest first, ties to the lowest index), new centers, strict / tol convergence, max_iter
__device__ void km_finish(const KmProblem& p, int64_t n, int C, int K, int max_iter, KmShared& sh) {
    const int tid = threadIdx.x;
    km_total(p, n, C, K, sh);
    for (int v = tid; v < K * C; v += kThreads) sh.centers[v] = p.st->centers[v];
    __syncthreads();
    int n_empty = 0, empty[kKmMaxK];   // listed before any relocation changes the counts (every thread reads the same LDS)
    for (int k = 0; k < K; ++k)
        if (sh.tot[K * C + k] == 0.0) empty[n_empty++] = k;
    for (int e = 0; e < n_empty; ++e) {
        const int k_new = empty[e];
        float key = INFINITY;
        int64_t idx = n;
        for (int64_t i = tid; i < n; i += kThreads) {
            bool taken = false;
            for (int q = 0; q < e; ++q) taken |= sh.picked[q] == i;
            if (taken) continue;
            km_argmin_merge(key, idx, -km_d2(p.x + i * C, sh.centers + p.labels[i] * C, C), i);
        }
        km_block_argmin(key, idx, sh.rk, sh.ri);
        if (tid == 0) {
            sh.picked[e] = idx;
            const int k_old = p.labels[idx];
            for (int c = 0; c < C; ++c) {
                const double xv = (double)p.x[idx * C + c];
                sh.tot[k_old * C + c] -= xv;
                sh.tot[k_new * C + c] = xv;
            }
            sh.tot[K * C + k_new] = 1.0;
            sh.tot[K * C + k_old] -= 1.0;
        }
        __syncthreads();
    }
    if (tid == 0) {
        double shift = 0.0;
        for (int k = 0; k < K; ++k) {
            const double cnt = sh.tot[K * C + k];
            for (int c = 0; c < C; ++c) {
                const double s = sh.tot[k * C + c];
                const float nc = (float)(cnt > 0.0 ? s / cnt : s);
                const double d = (double)nc - (double)sh.centers[k * C + c];
                shift += d * d;
                p.st->centers[k * C + c] = nc;
            }
        }
        const int it = p.st->iter + 1;
        p.st->iter = it;
        if (sh.tot[K * C + K] == 0.0) {
            p.st->strict = 1;
            p.st->done = 1;
        } else if (shift <= p.st->tol || it >= max_iter) {
            p.st->done = 1;
        }
    }
    __syncthreads();
}

// canonical order (ascending lexicographic order of the final centers, stable) and the outputs; sh.tot holds the final totals
__device__ void km_canon(const KmProblem& p, int C, int K, int64_t b, int max_iter, float* centers_out, double* inertia_out,
                         int32_t* n_iter_out, KmShared& sh) {
    if (threadIdx.x == 0) {
        int order[kKmMaxK];
        for (int k = 0; k < K; ++k) order[k] = k;
        for (int a = 1; a < K && max_iter > 0; ++a) {   // seeding only: the seeds stay in draw order   // insertion sort: stable
            const int cur = order[a];
            int j = a - 1;
            while (j >= 0) {
                const float* u = p.st->centers + order[j] * C;
                const float* v = p.st->centers + cur * C;
                int cmp = 0;
                for (int c = 0; c < C && !cmp; ++c) cmp = u[c] < v[c] ? -1 : (u[c] > v[c] ? 1 : 0);
                if (cmp <= 0) break;
                order[j + 1] = order[j];
                --j;
            }
            order[j + 1] = cur;
        }
        for (int r = 0; r < K; ++r) {
            p.st->perm[order[r]] = r;
            if (centers_out)
                for (int c = 0; c < C; ++c) centers_out[(b * K + r) * C + c] = p.st->centers[order[r] * C + c];
        }
        if (inertia_out) inertia_out[b] = sh.tot[K * C + K + 1];
        if (n_iter_out) n_iter_out[b] = p.st->iter;
    }
    __syncthreads();
}

__device__ void km_relabel_chunk(const KmProblem& p, int64_t n, int64_t chunk) {
    for (int j = 0; j < 4; ++j) {
        const int64_t i = chunk * kKmChunk + j * kThreads + threadIdx.x;
        if (i < n) p.labels[i] = p.st->perm[p.labels[i]];
    }
}

struct KmArgs {
    const float* x;
    const float* init;
    int32_t* labels;
    float* centers;
    double* inertia;
    int32_t* n_iter;
    unsigned char* ws;   // header (alldone word) + per-problem blocks
    int64_t n, batch, problem_base, per_stream;
    uint64_t seed;
    double tol;
    int C, K, n_trials, max_iter;
};
constexpr size_t kKmHeader = 64;

__device__ inline KmProblem km_problem_of(const KmArgs& a, int64_t b) {
    return km_problem(a.x, a.labels, a.ws + kKmHeader, b, a.n, a.K, a.C);
}

// workgroup regime: one workgroup runs problem blockIdx.x from seeding to canonical labels
__global__ __launch_bounds__(kThreads) void km_wg_kernel(KmArgs a) {
    __shared__ KmShared sh;
    const int64_t b = blockIdx.x;
    const KmProblem p = km_problem_of(a, b);
    km_seed(p, a.n, a.C, a.K, a.init ? a.init + b * a.K * a.C : nullptr, a.seed, a.problem_base + b / a.per_stream,
            a.n_trials, a.tol, a.max_iter, sh);
    const int64_t nch = km_chunks(a.n);
    while (!p.st->done) {   // written by thread 0 of this workgroup before the barrier that ends km_finish
        for (int64_t ch = 0; ch < nch; ++ch) km_assign_chunk(p, a.n, a.C, a.K, ch, 0, sh);
        km_finish(p, a.n, a.C, a.K, a.max_iter, sh);
    }
    for (int64_t ch = 0; ch < nch; ++ch) km_assign_chunk(p, a.n, a.C, a.K, ch, 1, sh);
    km_total(p, a.n, a.C, a.K, sh);
    km_canon(p, a.C, a.K, b, a.max_iter, a.centers, a.inertia, a.n_iter, sh);
    for (int64_t ch = 0; ch < nch; ++ch) km_relabel_chunk(p, a.n, ch);
}

// grid regime: seeding (one workgroup per problem), then per iteration an assign pass over all chunks and a one-workgroup finish;
// both return at once when the problem's done word is set
__global__ __launch_bounds__(kThreads) void km_seed_kernel(KmArgs a) {
    __shared__ KmShared sh;
    const int64_t b = blockIdx.x;
    km_seed(km_problem_of(a, b), a.n, a.C, a.K, a.init ? a.init + b * a.K * a.C : nullptr, a.seed, a.problem_base + b / a.per_stream,
            a.n_trials, a.tol, a.max_iter, sh);
}
__global__ __launch_bounds__(kThreads) void km_assign_kernel(KmArgs a, int mode) {
    __shared__ KmShared sh;
    const KmProblem p = km_problem_of(a, blockIdx.y);
    if (mode == 0 && p.st->done) return;
    km_assign_chunk(p, a.n, a.C, a.K, blockIdx.x, mode, sh);
}
__global__ __launch_bounds__(kThreads) void km_finish_kernel(KmArgs a) {
    __shared__ KmShared sh;
    const KmProblem p = km_problem_of(a, blockIdx.x);
    if (p.st->done) return;
    km_finish(p, a.n, a.C, a.K, a.max_iter, sh);
}
__global__ __launch_bounds__(64) void km_alldone_kernel(KmArgs a) {
    int notdone = 0;
    for (int64_t b = threadIdx.x; b < a.batch; b += 64) notdone += km_problem_of(a, b).st->done ? 0 : 1;
    for (int off = 32; off >= 1; off >>= 1) notdone += __shfl_xor(notdone, off);
    if (threadIdx.x == 0) *reinterpret_cast<int32_t*>(a.ws) = notdone == 0;
}
__global__ __launch_bounds__(kThreads) void km_canon_kernel(KmArgs a) {
    __shared__ KmShared sh;
    const int64_t b = blockIdx.x;
    const KmProblem p = km_problem_of(a, b);
    km_total(p, a.n, a.C, a.K, sh);
    km_canon(p, a.C, a.K, b, a.max_iter, a.centers, a.inertia, a.n_iter, sh);
}
__global__ __launch_bounds__(kThreads) void km_relabel_kernel(KmArgs a) {
    km_relabel_chunk(km_problem_of(a, blockIdx.y), a.n, blockIdx.x);
}
}  // namespace

// ----------------------------------------------------------------------------------------------------------------- C ABI
extern "C" size_t nsos_ssim_workspace_bytes(int64_t batch, int64_t channels, int64_t height, int64_t width) {
    if (batch <= 0 || channels <= 0 || height <= 0 || width <= 0) return 0;
    const int64_t tiles = ((width + kSsimTW - 1) / kSsimTW) * ((height + kSsimTH - 1) / kSsimTH);
    return (size_t)(batch * channels * tiles) * sizeof(double);
}

extern "C" int32_t nsos_ssim(const float* img1, const float* img2, int64_t batch, int64_t channels, int64_t height, int64_t width,
                             int32_t window_size, const float* window, int32_t size_average, float* out, float* ssim_map,
                             void* workspace, size_t workspace_bytes, void* stream) {
    NSOS_REQUIRE(img1 && img2 && out && workspace, NSOS_ERR_NULL_POINTER);
    NSOS_REQUIRE(batch > 0 && channels > 0 && height > 0 && width > 0, NSOS_ERR_BAD_SHAPE);
    NSOS_REQUIRE(window_size >= 1 && window_size <= 31 && (window_size & 1), NSOS_ERR_UNSUPPORTED);
    NSOS_REQUIRE(height <= (int64_t)65535 * kSsimTH && width <= (int64_t)1 << 30 && batch * channels <= 65535, NSOS_ERR_UNSUPPORTED);
    NSOS_REQUIRE(((uintptr_t)workspace & 7) == 0, NSOS_ERR_MISALIGNED);
    const size_t need = nsos_ssim_workspace_bytes(batch, channels, height, width);
    NSOS_REQUIRE(workspace_bytes >= need, NSOS_ERR_BUFFER_TOO_SMALL);
    // utils/ssim.py:7-9 gaussian(window_size, 1.5): exp() in double, stored as fp32, divided by its sum (torch's vectorised fp32
    // sum: the caller passes that window; without one the sum is accumulated in fp64 and rounded once)
    SsimWin win = {};
    if (window) {
        for (int k = 0; k < window_size; ++k) win.g[k] = window[k];
    } else {
        double sum = 0.0;
        for (int k = 0; k < window_size; ++k) {
            const double d = (double)(k - window_size / 2);
            win.g[k] = (float)exp(-(d * d) / (2.0 * 1.5 * 1.5));
            sum += (double)win.g[k];
        }
        for (int k = 0; k < window_size; ++k) win.g[k] = win.g[k] / (float)sum;
    }
    const int R = window_size / 2;
    const dim3 grid((unsigned)((width + kSsimTW - 1) / kSsimTW), (unsigned)((height + kSsimTH - 1) / kSsimTH), (unsigned)(batch * channels));
    double* part = static_cast<double*>(workspace);
    hipStream_t s = (hipStream_t)stream;
    if (R <= 7)
        hipLaunchKernelGGL(ssim_tile_kernel<7>, grid, dim3(kThreads), 0, s, img1, img2, (int)height, (int)width, R, win, ssim_map, part);
    else
        hipLaunchKernelGGL(ssim_tile_kernel<15>, grid, dim3(kThreads), 0, s, img1, img2, (int)height, (int)width, R, win, ssim_map, part);
    const int64_t tiles = (int64_t)grid.x * grid.y;
    if (size_average)
        hipLaunchKernelGGL(ssim_finish_kernel, dim3(1), dim3(kThreads), 0, s, part, batch * channels * tiles,
                           (double)(batch * channels * height * width), out);
    else
        hipLaunchKernelGGL(ssim_finish_kernel, dim3((unsigned)batch), dim3(kThreads), 0, s, part, channels * tiles,
                           (double)(channels * height * width), out);
    return nsos_launch_status();
}

extern "C" size_t nsos_adjusted_rand_workspace_bytes(void) { return (size_t)(kAriL * kAriL + 1) * sizeof(unsigned long long); }

extern "C" int32_t nsos_adjusted_rand(const void* labels_true, const void* labels_pred, int64_t n, int32_t dtype, int32_t subset_label,
                                      double* out, void* workspace, void* stream) {
    NSOS_REQUIRE(out && workspace, NSOS_ERR_NULL_POINTER);
    NSOS_REQUIRE(n >= 0, NSOS_ERR_BAD_SHAPE);
    NSOS_REQUIRE(n == 0 || (labels_true && labels_pred), NSOS_ERR_NULL_POINTER);
    NSOS_REQUIRE(dtype >= NSOS_LABEL_INT32 && dtype <= NSOS_LABEL_FLOAT32, NSOS_ERR_UNSUPPORTED);
    NSOS_REQUIRE(n <= (int64_t)1 << 31, NSOS_ERR_UNSUPPORTED);   // pair counts n^2 stay inside int64 products' range
    NSOS_REQUIRE(((uintptr_t)workspace & 7) == 0, NSOS_ERR_MISALIGNED);
    hipStream_t s = (hipStream_t)stream;
    auto* table = static_cast<unsigned long long*>(workspace);
    hipError_t e = hipMemsetAsync(table, 0, nsos_adjusted_rand_workspace_bytes(), s);
    if (e != hipSuccess) return (int32_t)e;
    if (n > 0) {
        const int64_t need = (n + kThreads - 1) / kThreads;
        const dim3 grid((unsigned)(need < kAriBlocks ? need : kAriBlocks));
        switch (dtype) {
            case NSOS_LABEL_INT32:
                hipLaunchKernelGGL(ari_count_kernel<int32_t>, grid, dim3(kThreads), 0, s, (const int32_t*)labels_true,
                                   (const int32_t*)labels_pred, n, table);
                break;
            case NSOS_LABEL_INT64:
                hipLaunchKernelGGL(ari_count_kernel<int64_t>, grid, dim3(kThreads), 0, s, (const int64_t*)labels_true,
                                   (const int64_t*)labels_pred, n, table);
                break;
            case NSOS_LABEL_UINT8:
                hipLaunchKernelGGL(ari_count_kernel<uint8_t>, grid, dim3(kThreads), 0, s, (const uint8_t*)labels_true,
                                   (const uint8_t*)labels_pred, n, table);
                break;
            default:
                hipLaunchKernelGGL(ari_count_kernel<float>, grid, dim3(kThreads), 0, s, (const float*)labels_true,
                                   (const float*)labels_pred, n, table);
                break;
        }
    }
    hipLaunchKernelGGL(ari_finish_kernel, dim3(1), dim3(kThreads), 0, s, table, (int)subset_label, out);
    return nsos_launch_status();
}

extern "C" size_t nsos_kmeans_workspace_bytes(int64_t batch, int64_t n_points, int32_t n_features, int32_t n_clusters) {
    if (batch <= 0 || n_points <= 0 || n_features < 1 || n_features > kKmMaxC || n_clusters < 1 || n_clusters > kKmMaxK) return 0;
    return kKmHeader + (size_t)batch * km_problem_bytes(n_points, n_clusters, n_features);
}

extern "C" int32_t nsos_kmeans(const float* x, int64_t batch, int64_t n_points, int32_t n_features, int32_t n_clusters,
                               const float* init_centers, uint64_t seed, int64_t problem_base, int64_t problems_per_stream,
                               int32_t n_local_trials,
                               int32_t max_iter, double tol, int32_t mode, int32_t* labels, float* centers, double* inertia,
                               int32_t* n_iter, void* workspace, size_t workspace_bytes, void* stream) {
    NSOS_REQUIRE(x && labels && workspace, NSOS_ERR_NULL_POINTER);
    NSOS_REQUIRE(batch > 0 && n_points > 0 && n_features > 0 && n_clusters > 0 && max_iter >= 0 && problem_base >= 0 &&
                     problems_per_stream > 0, NSOS_ERR_BAD_SHAPE);
    NSOS_REQUIRE(n_features <= kKmMaxC && n_clusters <= kKmMaxK, NSOS_ERR_UNSUPPORTED);
    NSOS_REQUIRE(n_points >= n_clusters, NSOS_ERR_BAD_SHAPE);
    NSOS_REQUIRE(n_local_trials >= 0 && n_local_trials <= 8 && mode >= 0 && mode <= 2 && tol >= 0.0, NSOS_ERR_UNSUPPORTED);
    NSOS_REQUIRE(batch <= 65535 && km_chunks(n_points) <= ((int64_t)1 << 31) - 1, NSOS_ERR_UNSUPPORTED);
    NSOS_REQUIRE(((uintptr_t)workspace & 15) == 0, NSOS_ERR_MISALIGNED);
    NSOS_REQUIRE(workspace_bytes >= nsos_kmeans_workspace_bytes(batch, n_points, n_features, n_clusters), NSOS_ERR_BUFFER_TOO_SMALL);
    KmArgs a;
    a.x = x;
    a.init = init_centers;
    a.labels = labels;
    a.centers = centers;
    a.inertia = inertia;
    a.n_iter = n_iter;
    a.ws = static_cast<unsigned char*>(workspace);
    a.n = n_points;
    a.batch = batch;
    a.problem_base = problem_base;
    a.per_stream = problems_per_stream;
    a.seed = seed;
    a.tol = tol;
    a.C = n_features;
    a.K = n_clusters;
    // sklearn _kmeans_plusplus: 2 + int(log(n_clusters)) local trials
    a.n_trials = n_local_trials ? n_local_trials : 2 + (int)log((double)n_clusters);
    a.max_iter = max_iter;
    hipStream_t s = (hipStream_t)stream;
    const bool grid_regime = mode == 2 || (mode == 0 && n_points > NSOS_KMEANS_WG_MAX_POINTS);
    if (!grid_regime) {
        hipLaunchKernelGGL(km_wg_kernel, dim3((unsigned)batch), dim3(kThreads), 0, s, a);
        return nsos_launch_status();
    }
    const dim3 chunks((unsigned)km_chunks(n_points), (unsigned)batch);
    hipLaunchKernelGGL(km_seed_kernel, dim3((unsigned)batch), dim3(kThreads), 0, s, a);
    for (int it = 0; it < max_iter;) {
        for (int g = 0; g < kKmGroup && it < max_iter; ++g, ++it) {
            hipLaunchKernelGGL(km_assign_kernel, chunks, dim3(kThreads), 0, s, a, 0);
            hipLaunchKernelGGL(km_finish_kernel, dim3((unsigned)batch), dim3(kThreads), 0, s, a);
        }
        int32_t st = nsos_launch_status();
        if (st != NSOS_OK) return st;
        if (it >= max_iter) break;
        hipLaunchKernelGGL(km_alldone_kernel, dim3(1), dim3(64), 0, s, a);
        int32_t all_done = 0;
        hipError_t e = hipMemcpyAsync(&all_done, a.ws, sizeof(all_done), hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) return (int32_t)e;
        if (all_done) break;
    }
    hipLaunchKernelGGL(km_assign_kernel, chunks, dim3(kThreads), 0, s, a, 1);
    hipLaunchKernelGGL(km_canon_kernel, dim3((unsigned)batch), dim3(kThreads), 0, s, a);
    hipLaunchKernelGGL(km_relabel_kernel, chunks, dim3(kThreads), 0, s, a);
    return nsos_launch_status();
}
