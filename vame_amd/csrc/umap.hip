// UMAP of the latent vectors (vame/analysis/umap_visualization.py:47-111: umap.UMAP(n_components=2, min_dist, n_neighbors,
// random_state).fit_transform): exact Euclidean kNN, smooth-kNN calibration + membership weights, the fuzzy union of the two directions
// of the kNN graph, and one deterministic SGD epoch of the 2-D layout.  Definitions: McInnes, Healy, Melville 2018 (arXiv:1802.03426)
// with umap-learn's published defaults; the host side (graph assembly, spectral init, epoch loop) is vame_amd/analysis/umap_hip.py.
#include "vame_common.h"

#ifdef VAME_EMU
#define UMAP_ALLOW_LDS(kernel, bytes)
#else      // > 64 KiB of dynamic LDS must be granted per kernel
#define UMAP_ALLOW_LDS(kernel, bytes) \
    VAME_CHECK_ARG(hipFuncSetAttribute(reinterpret_cast<const void*>(&kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)(bytes)) == hipSuccess, \
                   VAME_E_HIP, "knn: cannot reserve %d bytes of LDS", (int)(bytes))
#endif

__device__ __forceinline__ uint32_t f32_bits(float v) { return __builtin_bit_cast(uint32_t, v); }
__device__ __forceinline__ float bits_f32(uint32_t u) { return __builtin_bit_cast(float, u); }

// --------------------------------------------------------------------------------- exact kNN
// A workgroup owns KNN_ROWS query rows (in LDS, zero padded to DP) and streams all N points past them, KNN_THREADS at a time: a thread
// holds one point in registers and scores it against every query row (LDS broadcast reads), so each point is read once per KNN_ROWS
// queries.  A candidate is the 64-bit key (bits of the squared distance << 32 | point index): for non-negative floats the bit pattern
// orders like the value, so keys order by distance, then by index (the lower index wins a tie) -- a total order, which makes the
// selection exact and independent of the order candidates arrive in.  Each row keeps the KS = k - 1 best keys so far at the front of an
// LDS buffer of KNN_CAP keys and a threshold (its KS-th best key); a point below the threshold is appended with an LDS atomic.  Before
// a tile could overflow a row's buffer (or after the last tile) a bitonic sort, one row per wave, shrinks it back to KS keys and
// tightens the threshold.  The point itself is never a candidate: it goes to slot 0 at distance 0, so duplicates of it cannot take
// its place.  Tiles are visited starting at the workgroup's own rows and wrapping round: in time-ordered latents the neighbours of a
// frame are mostly nearby frames, so the threshold tightens within the first tiles and few later points get through.
#define KNN_THREADS 256
#define KNN_ROWS 16
#define KNN_CAP 512            // >= KS + KNN_THREADS: a row compacted below KNN_CAP - KNN_THREADS keys can take one more tile

static size_t knn_lds_bytes(int DP) {
    return (size_t)KNN_ROWS * KNN_CAP * 8 + KNN_ROWS * 8 + (size_t)KNN_ROWS * DP * 4 + (KNN_ROWS + KNN_ROWS + 1) * 4;
}

template <int DP>
__global__ __launch_bounds__(KNN_THREADS) void knn_kernel(const float* __restrict__ X, int N, int D, int k, int* __restrict__ idx,
                                                          float* __restrict__ dist) {
    VAME_DYN_SMEM(smem_raw);
    unsigned long long* cand = reinterpret_cast<unsigned long long*>(smem_raw);      // [KNN_ROWS][KNN_CAP]
    unsigned long long* thr = cand + KNN_ROWS * KNN_CAP;                                // [KNN_ROWS]
    float* qs = reinterpret_cast<float*>(thr + KNN_ROWS);                               // [KNN_ROWS][DP]
    int* cnt = reinterpret_cast<int*>(qs + KNN_ROWS * DP);                              // [KNN_ROWS]
    int* need = cnt + KNN_ROWS;                                                         // [KNN_ROWS] rows to compact, [KNN_ROWS] = their count
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int KS = k - 1;
    const int q0 = blockIdx.x * KNN_ROWS;
    const int nq = N - q0 < KNN_ROWS ? N - q0 : KNN_ROWS;
    for (int i = tid; i < KNN_ROWS * DP; i += KNN_THREADS) {
        const int r = i / DP, j = i % DP;
        qs[i] = (r < nq && j < D) ? X[(int64_t)(q0 + r) * D + j] : 0.f;
    }
    for (int i = tid; i < KNN_ROWS * KNN_CAP; i += KNN_THREADS) cand[i] = ~0ull;
    if (tid < KNN_ROWS) { thr[tid] = ~0ull; cnt[tid] = 0; }
    __syncthreads();
    const int ntiles = (N + KNN_THREADS - 1) / KNN_THREADS;
    const int t0 = q0 / KNN_THREADS;
    for (int t = 0; t < ntiles; ++t) {
        const int tile = t0 + t < ntiles ? t0 + t : t0 + t - ntiles;
        const int p = tile * KNN_THREADS + tid;
        if (p < N) {
            float x[DP];
            const float* xp = X + (int64_t)p * D;
#pragma unroll
            for (int j = 0; j < DP; ++j) x[j] = j < D ? xp[j] : 0.f;
#pragma unroll 2
            for (int r = 0; r < nq; ++r) {
                const float4* q4 = reinterpret_cast<const float4*>(qs + r * DP);
                float d = 0.f;                               // sum of (x - q)^2 in dimension order (padding adds exact zeros)
#pragma unroll
                for (int c = 0; c < DP / 4; ++c) {
                    const float4 q = q4[c];
                    float u = x[4 * c] - q.x;
                    d = fmaf(u, u, d);
                    u = x[4 * c + 1] - q.y;
                    d = fmaf(u, u, d);
                    u = x[4 * c + 2] - q.z;
                    d = fmaf(u, u, d);
                    u = x[4 * c + 3] - q.w;
                    d = fmaf(u, u, d);
                }
                const unsigned long long key = ((unsigned long long)f32_bits(d) << 32) | (unsigned)p;
                if (key < thr[r] && q0 + r != p) {
                    const int pos = atomicAdd(&cnt[r], 1);   // < KNN_CAP: cnt <= KNN_CAP - KNN_THREADS before the tile
                    cand[r * KNN_CAP + pos] = key;
                }
            }
        }
        __syncthreads();
        const bool last = t == ntiles - 1;
        if (tid == 0) {
            int m = 0;
            for (int r = 0; r < nq; ++r)
                if (last || cnt[r] > KNN_CAP - KNN_THREADS) need[m++] = r;
            need[KNN_ROWS] = m;
        }
        __syncthreads();
        const int m = need[KNN_ROWS];
        for (int g = 0; g < m; g += 4) {                     // four rows at a time, one per wave; every wave keeps the barriers
            const int r = g + wave < m ? need[g + wave] : -1;
            unsigned long long* c = cand + (r < 0 ? 0 : r) * KNN_CAP;
            for (int size = 2; size <= KNN_CAP; size <<= 1) {
                for (int stride = size >> 1; stride > 0; stride >>= 1) {
                    if (r >= 0) {
                        for (int i = lane; i < KNN_CAP / 2; i += VAME_WAVE) {
                            const int lo = 2 * i - (i & (stride - 1)), hi = lo + stride;
                            const unsigned long long u = c[lo], v = c[hi];
                            if ((u > v) == ((lo & size) == 0)) { c[lo] = v; c[hi] = u; }
                        }
                    }
                    __syncthreads();
                }
            }
            if (r >= 0) {
                for (int i = KS + lane; i < KNN_CAP; i += VAME_WAVE) c[i] = ~0ull;
                if (lane == 0) {
                    cnt[r] = cnt[r] < KS ? cnt[r] : KS;
                    thr[r] = c[KS - 1];
                }
            }
            __syncthreads();
        }
    }
    for (int i = tid; i < nq * k; i += KNN_THREADS) {
        const int r = i / k, s = i % k;
        int j = q0 + r;
        float dd = 0.f;
        if (s > 0) {
            const unsigned long long key = cand[r * KNN_CAP + s - 1];
            j = (int)(unsigned)(key & 0xffffffffull);
            dd = sqrtf(bits_f32((uint32_t)(key >> 32)));
        }
        idx[(int64_t)q0 * k + i] = j;
        dist[(int64_t)q0 * k + i] = dd;
    }
}

extern "C" int vame_knn_f32(const float* X, int64_t N, int D, int k, int* idx, float* dist, void* stream) {
    VAME_CHECK_ARG(X && idx && dist, VAME_E_BADARG, "knn: null pointer");
    VAME_CHECK_ARG(D >= 1 && D <= 64, VAME_E_UNSUPPORTED, "knn: D=%d outside 1..64", D);
    VAME_CHECK_ARG(k >= 2 && k <= 256, VAME_E_UNSUPPORTED, "knn: k=%d outside 2..256", k);
    VAME_CHECK_ARG(N >= k, VAME_E_SHAPE, "knn: k=%d neighbours of N=%lld points", k, (long long)N);
    VAME_CHECK_ARG(N * (int64_t)k < ((int64_t)1 << 31), VAME_E_SHAPE, "knn: N*k = %lld >= 2^31", (long long)(N * k));
    const dim3 grid((unsigned)cdiv64(N, KNN_ROWS));
    const int DP = D <= 8 ? 8 : D <= 16 ? 16 : D <= 32 ? 32 : 64;
    const size_t sh = knn_lds_bytes(DP);
    if (DP == 8) {
        UMAP_ALLOW_LDS(knn_kernel<8>, sh);
        hipLaunchKernelGGL(knn_kernel<8>, grid, dim3(KNN_THREADS), sh, (hipStream_t)stream, X, (int)N, D, k, idx, dist);
    } else if (DP == 16) {
        UMAP_ALLOW_LDS(knn_kernel<16>, sh);
        hipLaunchKernelGGL(knn_kernel<16>, grid, dim3(KNN_THREADS), sh, (hipStream_t)stream, X, (int)N, D, k, idx, dist);
    } else if (DP == 32) {
        UMAP_ALLOW_LDS(knn_kernel<32>, sh);
        hipLaunchKernelGGL(knn_kernel<32>, grid, dim3(KNN_THREADS), sh, (hipStream_t)stream, X, (int)N, D, k, idx, dist);
    } else {
        UMAP_ALLOW_LDS(knn_kernel<64>, sh);
        hipLaunchKernelGGL(knn_kernel<64>, grid, dim3(KNN_THREADS), sh, (hipStream_t)stream, X, (int)N, D, k, idx, dist);
    }
    VAME_LAUNCH_CHECK("knn");
    return VAME_OK;
}

// --------------------------------------------------------------------------------- smooth-kNN calibration + membership weights
// One row per wave, the row's k distances over the lanes (slots lane + 64c).  rho = smallest non-zero distance; sigma by bisection
// (64 steps, float64) so that sum_{s>=1} exp(-max(0, d_s - rho) / sigma) = log2 k to 1e-5, floored at 1e-3 x the row's mean distance
// (rho > 0) or 1e-3 x the mean over all rows (rho = 0).  The sum is a xor butterfly, whose result is the same bits in every lane, so
// the bisection's branches are wave-uniform.
__device__ __forceinline__ double shfl_xor_f64(double v, int m) {
    const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
    const int lo = __shfl_xor((int)(unsigned)u, m), hi = __shfl_xor((int)(unsigned)(u >> 32), m);
    return __builtin_bit_cast(double, ((unsigned long long)(unsigned)hi << 32) | (unsigned)lo);
}
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += shfl_xor_f64(v, m);
    return v;
}

__global__ __launch_bounds__(256) void umap_membership_kernel(const float* __restrict__ dist, const int* __restrict__ idx, int N, int k,
                                                              double mean_all, float* __restrict__ rho_out, float* __restrict__ sigma_out,
                                                              float* __restrict__ w) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= N) return;                                      // the whole wave
    const float* d = dist + (int64_t)i * k;
    float v[4];
    float nz = 3.4e38f;
    double rowsum = 0.0;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int s = lane + 64 * c;
        v[c] = s < k ? d[s] : 0.f;
        if (s < k && v[c] > 0.f && v[c] < nz) nz = v[c];
        rowsum += v[c];
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) nz = fminf(nz, __shfl_xor(nz, m));
    rowsum = wave_sum_f64(rowsum);
    const double rho = nz < 3.4e38f ? (double)nz : 0.0;
    const double target = log2((double)k);
    double lo = 0.0, hi = INFINITY, mid = 1.0;
    for (int it = 0; it < 64; ++it) {
        double ps = 0.0;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int s = lane + 64 * c;
            if (s >= 1 && s < k) {
                const double dd = (double)v[c] - rho;
                ps += dd > 0.0 ? exp(-dd / mid) : 1.0;
            }
        }
        ps = wave_sum_f64(ps);
        if (fabs(ps - target) < 1e-5) break;
        if (ps > target) {
            hi = mid;
            mid = (lo + hi) * 0.5;
        } else {
            lo = mid;
            mid = hi == INFINITY ? mid * 2.0 : (lo + hi) * 0.5;
        }
    }
    const double floor_ = 1e-3 * (rho > 0.0 ? rowsum / k : mean_all);
    if (mid < floor_) mid = floor_;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int s = lane + 64 * c;
        if (s < k) {
            const double dd = (double)v[c] - rho;
            const float wv = idx[(int64_t)i * k + s] == i ? 0.f : (dd <= 0.0 || mid == 0.0) ? 1.f : (float)exp(-dd / mid);
            w[(int64_t)i * k + s] = wv;
        }
    }
    if (lane == 0) {
        rho_out[i] = (float)rho;
        sigma_out[i] = (float)mid;
    }
}

extern "C" int vame_umap_membership_f32(const float* dist, const int* idx, int64_t N, int k, double mean_dist, float* rho, float* sigma,
                                        float* w, void* stream) {
    VAME_CHECK_ARG(dist && idx && rho && sigma && w, VAME_E_BADARG, "umap_membership: null pointer");
    VAME_CHECK_ARG(k >= 2 && k <= 256, VAME_E_UNSUPPORTED, "umap_membership: k=%d outside 2..256", k);
    VAME_CHECK_ARG(N >= 1 && N * (int64_t)k < ((int64_t)1 << 31), VAME_E_SHAPE, "umap_membership: N=%lld, k=%d", (long long)N, k);
    hipLaunchKernelGGL(umap_membership_kernel, dim3((unsigned)cdiv64(N, 4)), dim3(256), 0, (hipStream_t)stream, dist, idx, (int)N, k,
                       mean_dist, rho, sigma, w);
    VAME_LAUNCH_CHECK("umap_membership");
    return VAME_OK;
}

// --------------------------------------------------------------------------------- fuzzy union P = W + W^T - W o W^T
// (1) each kNN row sorted by point index (rank of an entry = number of smaller indices in its row; a row's indices are distinct), so
// (2) the reverse weight w_ji of an entry (i, j) is a binary search for i in row j.  p[i, s] = w + w_ji - w w_ji (the same bits for
// (i, j) and (j, i): both operand orders round alike), rev[i, s] = 1 if i is among j's neighbours (the pair then appears in both rows).
__global__ __launch_bounds__(256) void umap_rowsort_kernel(const int* __restrict__ idx, const float* __restrict__ w, int N, int k,
                                                           int* __restrict__ sidx, float* __restrict__ sw) {
    __shared__ int row[4][256];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int i = blockIdx.x * 4 + wv;
    const bool ok = i < N;
    for (int s = lane; s < k; s += VAME_WAVE) row[wv][s] = ok ? idx[(int64_t)i * k + s] : 0;
    __syncthreads();
    if (ok) {
        for (int s = lane; s < k; s += VAME_WAVE) {
            const int me = row[wv][s];
            int rank = 0;
            for (int t = 0; t < k; ++t) rank += row[wv][t] < me;
            sidx[(int64_t)i * k + rank] = me;
            sw[(int64_t)i * k + rank] = w[(int64_t)i * k + s];
        }
    }
}

__global__ __launch_bounds__(256) void umap_union_kernel(const int* __restrict__ idx, const float* __restrict__ w, const int* __restrict__ sidx,
                                                         const float* __restrict__ sw, int N, int k, float* __restrict__ p, int* __restrict__ rev) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (int64_t)N * k) return;
    const int i = (int)(e / k), j = idx[e];
    const float a = w[e];
    float b = 0.f;
    int found = 0;
    if (j != i && j >= 0 && j < N) {
        const int* r = sidx + (int64_t)j * k;
        int lo = 0, hi = k;                                  // first position with r[pos] >= i
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (r[mid] < i) lo = mid + 1;
            else hi = mid;
        }
        if (lo < k && r[lo] == i) {
            found = 1;
            b = sw[(int64_t)j * k + lo];
        }
    }
    p[e] = j == i ? 0.f : a + b - a * b;
    rev[e] = found;
}

extern "C" int64_t vame_umap_union_ws_bytes(int64_t N, int k) { return N * (int64_t)k * 8; }

extern "C" int vame_umap_fuzzy_union_f32(const int* idx, const float* w, int64_t N, int k, float* p, int* rev, void* ws, int64_t ws_bytes,
                                         void* stream) {
    VAME_CHECK_ARG(idx && w && p && rev && ws, VAME_E_BADARG, "umap_fuzzy_union: null pointer");
    VAME_CHECK_ARG(k >= 2 && k <= 256, VAME_E_UNSUPPORTED, "umap_fuzzy_union: k=%d outside 2..256", k);
    VAME_CHECK_ARG(N >= 1 && N * (int64_t)k < ((int64_t)1 << 31), VAME_E_SHAPE, "umap_fuzzy_union: N=%lld, k=%d", (long long)N, k);
    VAME_CHECK_ARG(ws_bytes >= vame_umap_union_ws_bytes(N, k), VAME_E_SHAPE, "umap_fuzzy_union: ws holds %lld bytes, needs %lld",
                   (long long)ws_bytes, (long long)vame_umap_union_ws_bytes(N, k));
    int* sidx = reinterpret_cast<int*>(ws);
    float* sw = reinterpret_cast<float*>(sidx + N * k);
    hipLaunchKernelGGL(umap_rowsort_kernel, dim3((unsigned)cdiv64(N, 4)), dim3(256), 0, (hipStream_t)stream, idx, w, (int)N, k, sidx, sw);
    VAME_LAUNCH_CHECK("umap_rowsort");
    hipLaunchKernelGGL(umap_union_kernel, dim3((unsigned)cdiv64(N * k, 256)), dim3(256), 0, (hipStream_t)stream, idx, w, sidx, sw, (int)N, k,
                       p, rev);
    VAME_LAUNCH_CHECK("umap_fuzzy_union");
    return VAME_OK;
}

// --------------------------------------------------------------------------------- one SGD epoch of the 2-D layout
// Gather form, bitwise reproducible: a lane owns vertex i, reads every other vertex from the previous epoch's positions (yin) and walks
// its CSR row in order, updating its own position in registers after each step.  Edge e (rate r_e = p_e / max P) is due in epoch n
// when floor((n + 1) r_e) > floor(n r_e), i.e. every 1 / r_e epochs; (i, j) and (j, i) carry the same weight, so both are due in the
// same epochs.  A due edge gives i two attractive pulls towards y_j (the head and the tail update of the reference's two directed
// copies of the edge) and then UMAP_NEG negative samples, k = Philox(counter = (e, epoch, draw / 4), key = seed)[draw % 4] mod N.
// Gradient components are clipped to +-4; a negative sample that is i itself is skipped, one at distance 0 pushes by +4.
#define UMAP_NEG 5

__device__ __forceinline__ float clip4(float v) { return fminf(fmaxf(v, -4.f), 4.f); }

__global__ __launch_bounds__(256) void umap_epoch_kernel(const float* __restrict__ yin, float* __restrict__ yout, int N,
                                                         const int64_t* __restrict__ indptr, const int* __restrict__ indices,
                                                         const float* __restrict__ rate, int epoch, float alpha, float a, float b,
                                                         uint32_t seed_lo, uint32_t seed_hi) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    float y0 = yin[2 * i], y1 = yin[2 * i + 1];
    const float fn = (float)epoch, fn1 = (float)(epoch + 1);
    const float two_ab = 2.f * a * b, two_b = 2.f * b, bm1 = b - 1.f;
    const int64_t e1 = indptr[i + 1];
    for (int64_t e = indptr[i]; e < e1; ++e) {
        const float r = rate[e];
        if (!(floorf(fn1 * r) > floorf(fn * r))) continue;
        const int j = indices[e];
        const float o0 = yin[2 * j], o1 = yin[2 * j + 1];
#pragma unroll
        for (int pull = 0; pull < 2; ++pull) {
            const float d0 = y0 - o0, d1 = y1 - o1;
            const float d2 = fmaf(d0, d0, d1 * d1);
            const float g = d2 > 0.f ? -two_ab * powf(d2, bm1) / (a * powf(d2, b) + 1.f) : 0.f;
            y0 += clip4(g * d0) * alpha;
            y1 += clip4(g * d1) * alpha;
        }
        uint32_t rr[4];
#pragma unroll
        for (int s = 0; s < UMAP_NEG; ++s) {
            if ((s & 3) == 0) philox4x32_10((uint32_t)e, (uint32_t)((uint64_t)e >> 32), (uint32_t)epoch, (uint32_t)(s >> 2), seed_lo, seed_hi, rr);
            const int kk = (int)(rr[s & 3] % (uint32_t)N);
            if (kk == i) continue;
            const float d0 = y0 - yin[2 * kk], d1 = y1 - yin[2 * kk + 1];
            const float d2 = fmaf(d0, d0, d1 * d1);
            if (d2 > 0.f) {
                const float g = two_b / ((0.001f + d2) * (a * powf(d2, b) + 1.f));
                y0 += clip4(g * d0) * alpha;
                y1 += clip4(g * d1) * alpha;
            } else {
                y0 += 4.f * alpha;
                y1 += 4.f * alpha;
            }
        }
    }
    yout[2 * i] = y0;
    yout[2 * i + 1] = y1;
}

extern "C" int vame_umap_epoch_f32(const float* yin, float* yout, int64_t N, const int64_t* indptr, const int* indices, const float* rate,
                                   int epoch, float alpha, float a, float b, uint64_t seed, void* stream) {
    VAME_CHECK_ARG(yin && yout && indptr && indices && rate, VAME_E_BADARG, "umap_epoch: null pointer");
    VAME_CHECK_ARG(yin != yout, VAME_E_BADARG, "umap_epoch: positions must be double-buffered (yin == yout)");
    VAME_CHECK_ARG(N >= 1 && N < ((int64_t)1 << 31) && epoch >= 0, VAME_E_SHAPE, "umap_epoch: N=%lld, epoch=%d", (long long)N, epoch);
    hipLaunchKernelGGL(umap_epoch_kernel, dim3((unsigned)cdiv64(N, 256)), dim3(256), 0, (hipStream_t)stream, yin, yout, (int)N, indptr,
                       indices, rate, epoch, alpha, a, b, (uint32_t)seed, (uint32_t)(seed >> 32));
    VAME_LAUNCH_CHECK("umap_epoch");
    return VAME_OK;
}
