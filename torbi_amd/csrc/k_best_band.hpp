// k_best_band.hpp -- the band route of k-best decoding (torbi_hip_k_best_band*, torbi_amd/k_best.py, KBEST.md "Band route"):
// k_best.hpp's lists, bit for bit, for a matrix that holds ONE value outside a band, at the cost of the band.
//
// With A[j][i] = background for i outside [j - reach_left, j + reach_right], every out-of-band candidate of every state j is
// d(i, r) = fl(L_{t-1}(i)[r] + background).  The lists are sorted and fl(x + a) is monotone, so
//     dmax = max over ALL prev-states i of d(i, 0)
// bounds every one of them (one workgroup reduction per item and frame; taking in-band states in is conservative).  State j
// builds its list from its W = reach_left + reach_right + 1 in-band prev-states in ascending i with the dense scan's rules
// (k_best.hpp: insert while the list is short, then only on a strict '>' against the k-th entry, the first rank of i that
// fails ends i).  FAST PATH: the list is full and its k-th value is strictly greater than dmax -- no out-of-band candidate
// can enter it (an equal one never enters a full list), so it is the dense list.  FALLBACK otherwise (a NaN dmax fails the
// comparison and lands here too): the state scans all S prev-states in ascending i again, reading `background` in place of
// the matrix outside the band, which IS the dense scan.  One code path for a finite background and for -inf.
// Before the scan (k >= 2) a pass over the in-band rank-0 candidates keeps their k largest values; the k-th is a floor no list
// entry lies below, and the scan leaves candidates below it out (it changes what is inserted on the way, not the list).
//
// One launch runs every frame of G items: the lists of the previous frame sit in LDS, rank-major with halos,
//     lists [2][G][k][reach_left + S + reach_right] fp32      (frame t reads buffer (t - 1) & 1 and writes t & 1)
// a thread owns next-states j = tid + threads * m and keeps the G lists of one state in registers.  Each frame writes its
// pointer rows ([B][T-1][k][S], (i << 5) | r: kb_walk_kernel's format), and an item's last frame writes its lists where
// kb_final_kernel reads them.  The diagonals diag[kk][j] = A[j][j - reach_left + kk], [W][S], come from
// banddiag::prepare_kernel (band_diagonals.hpp; its alarm word is the matrix flag kb_final_kernel reads) and stream from L2,
// each load shared by the G items.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

#include "band_diagonals.hpp"
#include "k_best.hpp"
#include "wave_reduce.hpp"

namespace kbb {

using kb::insert;
using kb::kth_of;
using kb::list_length;

constexpr int kMaxGroup = 4;                      // items per workgroup: instances <KMAX, 4 | 2 | 1> with G * KMAX <= 16
constexpr int kMaxThreads = 768;                  // twelve waves, three to a SIMD: up to 168 VGPRs each
constexpr int kMaxLdsBytes = banddiag::kMaxLdsBytes;   // (the reduction's partials go beside the dynamic part)
constexpr int kWorkgroups = 256;                  // G is halved until the launch has this many (one per CU of an MI355X)

__host__ __device__ inline size_t row_words(int S, int reach_left, int reach_right) { return (size_t)S + reach_left + reach_right; }

// dynamic LDS of kb_band_forward_kernel<KMAX, G>
__host__ __device__ inline size_t lds_bytes(int G, int S, int k, int reach_left, int reach_right) {
    return (size_t)2 * G * k * row_words(S, reach_left, reach_right) * sizeof(float);
}

// threads of a forward workgroup: the states in the fewest passes of at most kMaxThreads, whole waves (1440 states: 768)
inline int forward_threads(int S) {
    const int passes = (S + kMaxThreads - 1) / kMaxThreads;
    return ((S + passes - 1) / passes + 63) / 64 * 64;
}

// kb::layout with the diagonals in place of the transposed matrix, and the verdict word.  Of `vals` the forward writes only
// each item's final lists (frame F_b - 1, in the plane of that frame's parity).
struct Layout {
    float *vals, *diag;
    int32_t *ptrs, *count, *flag, *ok;
    kb::Final *final_;
    size_t total;
};

inline Layout layout(char *base, int B, int T, int S, int k, int reach_left, int reach_right) {
    Scratch a(base);
    Layout l;
    l.vals = a.take<float>((size_t)2 * B * k * S);
    l.ptrs = a.take<int32_t>((size_t)B * (T - 1) * k * S);
    l.diag = a.take<float>(((size_t)reach_left + reach_right + 1) * S);
    l.final_ = a.take<kb::Final>((size_t)B * k);
    l.count = a.take<int32_t>((size_t)B);
    l.flag = a.take<int32_t>((size_t)B + 1);     // [0]: matrix flag, [1 + b]: item flag
    l.ok = a.take<int32_t>(1);
    l.total = a.bytes + 256;                     // (room to align the caller's base)
    return l;
}

// after kb_final_kernel: a broken promise (ok[0] == 0) flags every item, whatever its frames
__global__ __launch_bounds__(256) void kb_band_verdict_kernel(const int32_t *__restrict__ ok, int32_t *__restrict__ count,
                                                              int32_t *__restrict__ flag, int B) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b < B && ok[0] == 0) { count[b] = 0; flag[1 + b] = 1; }
}

// The candidates of prev-state i for the lists of G items: col[(g * k + r) * RW] = L_{t-1}(i)[r] of item g, `a` the matrix
// entry, take[g] whether this lane's list of item g is being built from i.  The dense scan's rules; the wave skips the
// insertion code where no lane inserts.  `floor`: prev-states whose rank 0 lies below it are left out (the threshold of the
// first pass; -inf leaves nothing out).
template <int KMAX, int G>
__device__ __forceinline__ void scan_prev_state(float (&v)[G][KMAX], int (&p)[G][KMAX], int (&sz)[G], float (&kth)[G],
                                                const float *col, size_t RW, float a, int i, const bool (&take)[G], int k,
                                                int n, const float (&floor)[G]) {
    float c0[G];
    bool enter[G];
    bool any = false;
#pragma unroll
    for (int g = 0; g < G; ++g) {
        c0[g] = col[(size_t)g * k * RW] + a;
        enter[g] = take[g] && !(c0[g] < floor[g]) && (sz[g] < k || c0[g] > kth[g]);
        any |= enter[g];
    }
    if (__ballot(any) == 0) return;
#pragma unroll
    for (int g = 0; g < G; ++g) {
        if (!enter[g]) continue;
        float c = c0[g];
        for (int r = 0; r < n; ++r) {
            if (r > 0) {
                c = col[((size_t)g * k + r) * RW] + a;
                if (sz[g] >= k && !(c > kth[g])) break;
            }
            insert<KMAX>(v[g], p[g], c, (i << 5) | r, sz[g], k);
            sz[g] = min(sz[g] + 1, k);
            kth[g] = kth_of<KMAX>(v[g], k);
        }
    }
}

// a value into a sorted list of k values that started as -inf, after every entry >= c (nothing where c is not greater
// than the k-th)
template <int KMAX>
__device__ __forceinline__ void insert_value(float (&w)[KMAX], float c, int k) {
#pragma unroll
    for (int q = KMAX - 1; q >= 0; --q) {
        if (q < k) {
            const float above = w[q > 0 ? q - 1 : 0];
            const bool shift = q > 0 && c > above;
            w[q] = shift ? above : (c > w[q] ? c : w[q]);
        }
    }
}

// the workgroup's maximum of x per item, NaN if any thread holds one: partial[g][wave] now, combined after a barrier
template <int G>
__device__ __forceinline__ void reduce_partials(const float (&x)[G], const bool (&nan)[G], float (*partial)[kMaxThreads / 64],
                                                int lane, int wave) {
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const float m = wavered::wave_reduce_f32(x[g], wavered::MaxOp());
        const bool any = __any(nan[g]);
        if (lane == 0) partial[g][wave] = any ? __builtin_nanf("") : m;
    }
}

template <int KMAX, int G>
__global__ __launch_bounds__(kMaxThreads) void kb_band_forward_kernel(const float *__restrict__ obs, const int32_t *__restrict__ frames,
                                                                      const float *__restrict__ diag, const float *__restrict__ initial,
                                                                      float background, int reach_left, int reach_right,
                                                                      float *__restrict__ vals, int32_t *__restrict__ ptrs, int B,
                                                                      int T, int S, int k) {
    extern __shared__ float lists[];                                  // [2][G][k][RW]
    __shared__ float partial[2][G][kMaxThreads / 64];                 // d(i, 0) maxima of the waves, by frame parity
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int threads = blockDim.x, waves = threads >> 6;
    const int b0 = blockIdx.x * G;
    const int W = reach_left + reach_right + 1;
    const size_t RW = row_words(S, reach_left, reach_right);
    const size_t buffer = (size_t)G * k * RW;
    const int passes = (S + threads - 1) / threads;
    int F[G];
    int Fmax = 0;
#pragma unroll
    for (int g = 0; g < G; ++g) {
        F[g] = b0 + g < B ? min(max(frames[b0 + g], 1), T) : 0;
        Fmax = max(Fmax, F[g]);
    }
    for (size_t x = tid; x < 2 * buffer; x += threads) lists[x] = -INFINITY;        // (the halos; never used as candidates)
    __syncthreads();
    // frame 0: L_0(j) = [fl(o_0[j] + pi[j])]
    {
        float top[G];
        bool nan[G];
#pragma unroll
        for (int g = 0; g < G; ++g) {
            top[g] = -INFINITY;
            nan[g] = false;
            if (F[g] == 0) continue;
            const int b = b0 + g;
            for (int j = tid; j < S; j += threads) {
                const float x = obs[(size_t)b * T * S + j] + initial[j];
                lists[(size_t)g * k * RW + reach_left + j] = x;
                if (F[g] == 1) vals[(size_t)b * k * S + j] = x;
                const float d = x + background;
                nan[g] |= d != d;
                top[g] = fmaxf(top[g], d);
            }
        }
        reduce_partials<G>(top, nan, partial[0], lane, wave);
    }
    __syncthreads();
    for (int t = 1; t < Fmax; ++t) {
        const float *cur = lists + (size_t)((t - 1) & 1) * buffer;
        float *nxt = lists + (size_t)(t & 1) * buffer;
        const int n = list_length(k, S, t - 1), m = list_length(k, S, t);
        bool act[G];
        float dmax[G], top[G];
        bool nan[G];
#pragma unroll
        for (int g = 0; g < G; ++g) {
            act[g] = t < F[g];
            top[g] = -INFINITY;
            nan[g] = false;
            float x = -INFINITY;
            bool bad = false;
            for (int w = 0; w < waves; ++w) {
                const float y = partial[(t - 1) & 1][g][w];
                bad |= y != y;
                x = fmaxf(x, y);
            }
            dmax[g] = bad ? __builtin_nanf("") : x;
        }
        for (int pass = 0; pass < passes; ++pass) {
            const int j = tid + pass * threads;
            const bool in = j < S;
            const int jr = in ? j : S - 1;
            float v[G][KMAX];
            int p[G][KMAX];
            int sz[G];
            float kth[G];
            bool take[G];
#pragma unroll
            for (int g = 0; g < G; ++g) {
                sz[g] = 0;
                kth[g] = -INFINITY;
#pragma unroll
                for (int q = 0; q < KMAX; ++q) { v[g][q] = -INFINITY; p[g][q] = 0; }
            }
            // prev-state i = jr - reach_left + kk sits at lists[.. + jr + kk]; U diagonal entries in flight
            const float *dj = diag + jr;
            const float *pj = cur + jr;
            constexpr int U = G == 4 ? 4 : 8;
            float an[U];
            // ---- the threshold: the k-th largest of the in-band rank-0 candidates, values alone, taken from the main diagonal
            // outwards (a band matrix peaks there, so the list settles after a few prev-states; any order gives the same
            // value).  At least k candidates are no smaller, so a candidate below it is in no list: the scan below leaves
            // those out and inserts about k prev-states instead of every new maximum of an ascending run.
            float low[G];
#pragma unroll
            for (int g = 0; g < G; ++g) low[g] = -INFINITY;
            if constexpr (KMAX > 1) {
                float w[G][KMAX];
#pragma unroll
                for (int g = 0; g < G; ++g)
#pragma unroll
                    for (int q = 0; q < KMAX; ++q) w[g][q] = -INFINITY;
                auto outwards = [&](int x) { return x <= reach_left ? reach_left - x : x; };
#pragma unroll
                for (int u = 0; u < U; ++u) an[u] = u < W ? dj[(size_t)outwards(u) * S] : 0.f;
                for (int x = 0; x < W; x += U) {
                    float a[U];
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        a[u] = an[u];
                        an[u] = x + U + u < W ? dj[(size_t)outwards(x + U + u) * S] : 0.f;
                    }
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        if (x + u >= W) break;
                        const int kk = outwards(x + u), i = jr - reach_left + kk;
                        const bool valid = in && i >= 0 && i < S;
                        float c[G];
                        bool any = false;
#pragma unroll
                        for (int g = 0; g < G; ++g) {
                            c[g] = pj[(size_t)g * k * RW + kk] + a[u];
                            any |= valid && act[g] && c[g] > low[g];
                        }
                        if (__ballot(any) == 0) continue;
#pragma unroll
                        for (int g = 0; g < G; ++g) {
                            if (!(valid && act[g] && c[g] > low[g])) continue;
                            insert_value<KMAX>(w[g], c[g], k);
                            low[g] = kth_of<KMAX>(w[g], k);
                        }
                    }
                }
            }
            // ---- the band in ascending i
#pragma unroll
            for (int u = 0; u < U; ++u) an[u] = u < W ? dj[(size_t)u * S] : 0.f;
            for (int kk = 0; kk < W; kk += U) {
                float a[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    a[u] = an[u];
                    an[u] = kk + U + u < W ? dj[(size_t)(kk + U + u) * S] : 0.f;
                }
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    if (kk + u >= W) break;
                    const int i = jr - reach_left + kk + u;
                    const bool valid = in && i >= 0 && i < S;
#pragma unroll
                    for (int g = 0; g < G; ++g) take[g] = valid && act[g];
                    scan_prev_state<KMAX, G>(v, p, sz, kth, pj + kk + u, RW, a[u], i, take, k, n, low);
                }
            }
            // ---- fast path or fallback
            bool again = false;
#pragma unroll
            for (int g = 0; g < G; ++g) {
                take[g] = in && act[g] && !(sz[g] == k && kth[g] > dmax[g]);
                again |= take[g];
            }
            if (__ballot(again) != 0) {
#pragma unroll
                for (int g = 0; g < G; ++g) {
                    if (!take[g]) continue;
                    sz[g] = 0;
                    kth[g] = -INFINITY;
#pragma unroll
                    for (int q = 0; q < KMAX; ++q) { v[g][q] = -INFINITY; p[g][q] = 0; }
                }
#pragma unroll
                for (int g = 0; g < G; ++g) low[g] = -INFINITY;
                for (int i = 0; i < S; ++i) {
                    const int kk = i - jr + reach_left;
                    float a = background;
                    if (again && kk >= 0 && kk < W) a = dj[(size_t)kk * S];
                    scan_prev_state<KMAX, G>(v, p, sz, kth, cur + reach_left + i, RW, a, i, take, k, n, low);
                }
            }
            // ---- frame t's rows of state j
            if (in) {
#pragma unroll
                for (int g = 0; g < G; ++g) {
                    if (!act[g]) continue;
                    const int b = b0 + g;
                    const float o = obs[((size_t)b * T + t) * S + j];
                    int32_t *pt = ptrs + ((size_t)b * (T - 1) + (t - 1)) * k * S + j;
                    float *fin = vals + ((size_t)(t & 1) * B + b) * k * S + j;
                    const bool last = t == F[g] - 1;
#pragma unroll
                    for (int q = 0; q < KMAX; ++q) {
                        if (q < m) {
                            const float x = o + v[g][q];
                            nxt[((size_t)g * k + q) * RW + reach_left + j] = x;
                            pt[(size_t)q * S] = p[g][q];
                            if (last) fin[(size_t)q * S] = x;
                        }
                    }
                    const float d = (o + v[g][0]) + background;
                    nan[g] |= d != d;
                    top[g] = fmaxf(top[g], d);
                }
            }
        }
        reduce_partials<G>(top, nan, partial[t & 1], lane, wave);
        __syncthreads();
    }
}

}  // namespace kbb
