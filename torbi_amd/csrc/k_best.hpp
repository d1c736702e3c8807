// k_best.hpp -- k-best (list) Viterbi decoding with exact path scores (torbi_hip_k_best*, torbi_amd/k_best.py, KBEST.md).
//
// Every state j of frame t keeps a list L_t(j) of up to k entries (value, back-pointer (i, r)), sorted by the candidate
// order of KBEST.md: c = fl(L_{t-1}(i)[r] + A[j][i]) descending, then i ascending, then r ascending; the stored value is
// fl(o_t[j] + c).  Rank 0 of every list is the existing decoder's cell (value and lowest-index backpointer), so rank 0 of
// the result is torbi_hip_viterbi_decode's path.  Every list of a frame has the same length n_t = min(k, S^t).
//
// Workspace (kb::layout):
//     vals  [2][B][k][S] fp32    the lists of the previous and the current frame, rank-major (rank r of all states is a row)
//     ptrs  [B][T-1][k][S] int32 back-pointers (i << 5) | r of frames 1 .. T-1 (general route)
//           [B][T-1][k]    int32 the same, shared by every state (uniform route)
//     tt    [S][S] fp32          the matrix transposed ([prev][next]), so that a wave reads one prev-state's row coalesced
//     final [B][k] {float, int, int}  the selected (score, state, rank) of each result rank; count and item flag after them
//
// General route, per call: kb_prepare_kernel (transpose; NaN / +inf flag of the matrix), kb_first_kernel (frame 0),
// one kb_step_kernel per frame 1 .. T-1, kb_final_kernel (item flag, selection over (j, r)), kb_walk_kernel (backtrace).
// Uniform route: kb_uniform_kernel (one wave per item, the whole time loop and the final selection), kb_walk_kernel.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include "scratch.hpp"

namespace kb {

constexpr int kMaxK = 32;                 // ranks; a back-pointer keeps r in its low 5 bits
constexpr int kMaxStates = 16384;
constexpr int kThreads = 256;
constexpr int kRowLdsBytes = 64 * 1024;   // rank-0 rows of the G items of a step workgroup
constexpr int kStepWorkgroups = 512;     // the step launch halves G until it has this many (two per CU of an MI355X)
constexpr int kU = 8;                     // matrix entries in flight per thread (step kernel) / rows per lane (uniform)

struct Final {
    float score;
    int32_t state, rank;
};

struct Layout {
    float *vals, *tt;
    int32_t *ptrs, *count, *flag;
    Final *final_;
    size_t total;
};

// `base`: the caller's workspace aligned up to 256 bytes, or null for the byte count alone.
// The uniform route uses layout(base, B, T, 1, k): its pointers have no state axis and it needs neither vals nor tt.
inline Layout layout(char *base, int B, int T, int S, int k) {
    Scratch a(base);
    Layout l;
    l.vals = a.take<float>((size_t)2 * B * k * S);
    l.ptrs = a.take<int32_t>((size_t)B * (T - 1) * k * S);
    l.tt = a.take<float>((size_t)S * S);
    l.final_ = a.take<Final>((size_t)B * k);
    l.count = a.take<int32_t>((size_t)B);
    l.flag = a.take<int32_t>((size_t)B + 1);     // [0]: matrix flag, [1 + b]: item flag
    l.total = a.bytes + 256;                     // (room to align the caller's base)
    return l;
}

// n_t = min(k, S^t)
__host__ __device__ inline int list_length(int k, int S, int t) {
    long long n = 1;
    for (int s = 0; s < t && n < k; ++s) n *= S;
    return n < k ? (int)n : k;
}

__device__ __forceinline__ bool bad_value(float x) { return !(x < INFINITY); }     // NaN or +inf

// Insert (c, ptr) into the sorted list v[0 .. sz) of capacity k, after every entry >= c.  Precondition: sz < k, or
// sz == k and c > v[k - 1] (the last entry drops out).  Fully unrolled: the lists stay in registers.
template <int KMAX>
__device__ __forceinline__ void insert(float (&v)[KMAX], int (&p)[KMAX], float c, int ptr, int sz, int k) {
#pragma unroll
    for (int q = KMAX - 1; q >= 0; --q) {
        if (q < k && q <= sz) {
            const bool shift = q > 0 && c > v[q > 0 ? q - 1 : 0];
            const bool here = !shift && (q == sz || c > v[q]);
            const float pv = v[q > 0 ? q - 1 : 0];
            const int pp = p[q > 0 ? q - 1 : 0];
            v[q] = shift ? pv : (here ? c : v[q]);
            p[q] = shift ? pp : (here ? ptr : p[q]);
        }
    }
}

// v[k - 1] of a full list: the minimum of its first k entries (a select of v[k - 1] would become a dynamic index, and the
// list would leave the registers)
template <int KMAX>
__device__ __forceinline__ float kth_of(const float (&v)[KMAX], int k) {
    float x = v[0];
#pragma unroll
    for (int q = 1; q < KMAX; ++q) x = fminf(x, q < k ? v[q] : INFINITY);
    return x;
}

// tt[i][j] = A[j][i]; flag[0] = 1 if the matrix holds a NaN or +inf (flag[0] zeroed by the host before)
__global__ __launch_bounds__(256) void kb_prepare_kernel(const float *__restrict__ A, float *__restrict__ tt,
                                                         int32_t *__restrict__ flag, int S) {
    __shared__ float tile[32][33];
    const int x = threadIdx.x & 31, y = threadIdx.x >> 5;
    const int i0 = blockIdx.x * 32, j0 = blockIdx.y * 32;
    bool bad = false;
    for (int r = y; r < 32; r += 8) {
        const int j = j0 + r, i = i0 + x;
        float a = 0.f;
        if (j < S && i < S) {
            a = A[(size_t)j * S + i];
            bad |= bad_value(a);
        }
        tile[r][x] = a;
    }
    __syncthreads();
    for (int r = y; r < 32; r += 8) {
        const int i = i0 + r, j = j0 + x;
        if (i < S && j < S) tt[(size_t)i * S + j] = tile[x][r];
    }
    if (bad) flag[0] = 1;
}

// frame 0: L_0(j) = [fl(o_0[j] + pi[j])]
__global__ __launch_bounds__(256) void kb_first_kernel(const float *__restrict__ obs, const float *__restrict__ initial,
                                                       float *__restrict__ vals, int T, int S, int k) {
    const int b = blockIdx.x;
    const int j = blockIdx.y * 256 + threadIdx.x;
    if (j < S) vals[(size_t)b * k * S + j] = obs[(size_t)b * T * S + j] + initial[j];
}

// Frame t >= 1 of G items: thread j builds L_t(j) of every item in registers.  prev / cur: vals of frames t - 1 and t.
// n: n_{t-1}; m: n_t.  Candidates are scanned i ascending, r ascending; once a list is full, a candidate enters only if
// it is strictly greater than the k-th entry, and the first rank r of i that does not enter ends i (its later ranks are
// no greater).  Rank 0 of every prev-state comes from LDS; later ranks, read only on insertion, from global memory.
template <int KMAX, int G>
__global__ __launch_bounds__(kThreads) void kb_step_kernel(const float *__restrict__ obs, const int32_t *__restrict__ frames,
                                                           const float *__restrict__ tt, const float *__restrict__ prev,
                                                           float *__restrict__ cur, int32_t *__restrict__ ptrs, int t, int B,
                                                           int T, int S, int k, int n, int m) {
    extern __shared__ float rows[];          // [S][G]: rank 0 of every prev-state, the G items of one i side by side
    const int b0 = blockIdx.x * G;
    bool live[G];
    bool any_live = false;
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const int b = b0 + g;
        live[g] = b < B && t < min(max(frames[b], 1), T);
        any_live |= live[g];
    }
    if (!any_live) return;
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const int b = b0 + g < B ? b0 + g : B - 1;
        for (int i = threadIdx.x; i < S; i += kThreads) rows[(size_t)i * G + g] = prev[(size_t)b * k * S + i];
    }
    __syncthreads();
    const int j = blockIdx.y * kThreads + threadIdx.x;
    const bool in = j < S;
    const int jr = in ? j : S - 1;
    float v[G][KMAX];
    int p[G][KMAX];
    float kth[G];
#pragma unroll
    for (int g = 0; g < G; ++g) {
        kth[g] = -INFINITY;
#pragma unroll
        for (int q = 0; q < KMAX; ++q) { v[g][q] = -INFINITY; p[g][q] = 0; }
    }
    // while the lists fill (the first k candidates, the same for every lane): insert every candidate in order
    int i = 0;
    for (int scanned = 0; i < S && scanned < k; ++i) {
        const float a = tt[(size_t)i * S + jr];
        for (int r = 0; r < n; ++r, ++scanned) {
            const int sz = min(scanned, k);
#pragma unroll
            for (int g = 0; g < G; ++g) {
                const int b = b0 + g < B ? b0 + g : B - 1;
                const float c = (r == 0 ? rows[(size_t)i * G + g] : prev[((size_t)b * k + r) * S + i]) + a;
                if (sz < k || c > kth[g]) {
                    insert<KMAX>(v[g], p[g], c, (i << 5) | r, sz, k);
                    kth[g] = kth_of<KMAX>(v[g], k);
                }
            }
        }
    }
    // full lists: one add and one compare per (item, prev-state) unless a lane of the wave inserts.  The matrix entries of
    // the next kU prev-states are loaded while the current ones are scanned.
    float an[kU];
#pragma unroll
    for (int u = 0; u < kU; ++u) an[u] = i + u < S ? tt[(size_t)(i + u) * S + jr] : 0.f;
    for (; i < S; i += kU) {
        float a[kU];
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            a[u] = an[u];
            an[u] = i + kU + u < S ? tt[(size_t)(i + kU + u) * S + jr] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            const int ii = i + u;
            if (ii >= S) break;
            bool enter[G];
            bool any = false;
#pragma unroll
            for (int g = 0; g < G; ++g) {
                enter[g] = in && rows[(size_t)ii * G + g] + a[u] > kth[g];
                any |= enter[g];
            }
            if (__ballot(any) == 0) continue;
#pragma unroll
            for (int g = 0; g < G; ++g) {
                if (!enter[g]) continue;
                const int b = b0 + g < B ? b0 + g : B - 1;
                float c = rows[(size_t)ii * G + g] + a[u];
                for (int r = 0; r < n; ++r) {
                    if (r > 0) {
                        c = prev[((size_t)b * k + r) * S + ii] + a[u];
                        if (!(c > kth[g])) break;
                    }
                    insert<KMAX>(v[g], p[g], c, (ii << 5) | r, k, k);
                    kth[g] = kth_of<KMAX>(v[g], k);
                }
            }
        }
    }
    if (!in) return;
#pragma unroll
    for (int g = 0; g < G; ++g) {
        if (!live[g]) continue;
        const int b = b0 + g;
        const float o = obs[((size_t)b * T + t) * S + j];
        int32_t *pt = ptrs + ((size_t)b * (T - 1) + (t - 1)) * k * S + j;
#pragma unroll
        for (int q = 0; q < KMAX; ++q) {
            if (q < m) {
                cur[((size_t)b * k + q) * S + j] = o + v[g][q];
                pt[(size_t)q * S] = p[g][q];
            }
        }
    }
}

// order of the final selection and of the uniform route's candidates: value descending, then state, then rank ascending
__device__ __forceinline__ bool before(float v, int s, int r, float w, int s2, int r2) {
    return v > w || (v == w && (s < s2 || (s == s2 && r < r2)));
}

__device__ __forceinline__ void wave_best(float &v, int &s, int &r) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float ov = __shfl_xor(v, off, 64);
        const int os = __shfl_xor(s, off, 64), orr = __shfl_xor(r, off, 64);
        if (before(ov, os, orr, v, s, r)) { v = ov; s = os; r = orr; }
    }
}

// One workgroup per item: the item flag (NaN or +inf in its observation rows t < F, the initial distribution, or the
// matrix when F >= 2), then the first min(k, S^F) entries (L_{F-1}(j)[r], j, r) in the order of `before`, one round each.
__global__ __launch_bounds__(kThreads) void kb_final_kernel(const float *__restrict__ obs, const int32_t *__restrict__ frames,
                                                            const float *__restrict__ initial, const float *__restrict__ vals,
                                                            Final *__restrict__ final_, int32_t *__restrict__ count,
                                                            int32_t *__restrict__ flag, int B, int T, int S, int k) {
    __shared__ float sv[kThreads / 64];
    __shared__ int ss[kThreads / 64], sr[kThreads / 64];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int F = min(max(frames[b], 1), T);
    bool bad = F >= 2 && flag[0] != 0;
    for (int j = tid; j < S; j += kThreads) bad |= bad_value(initial[j]);
    const float *o = obs + (size_t)b * T * S;
    for (size_t x = tid; x < (size_t)F * S; x += kThreads) bad |= bad_value(o[x]);
    bad = __syncthreads_or(bad);
    if (bad) {
        if (tid == 0) { count[b] = 0; flag[1 + b] = 1; }
        return;
    }
    const int n = list_length(k, S, F - 1);
    const float *L = vals + ((size_t)((F - 1) & 1) * B + b) * k * S;
    const int m = (int)min((long long)k, (long long)S * n);
    float pv = INFINITY;
    int ps = -1, pr = -1;
    for (int q = 0; q < m; ++q) {
        float bv = -INFINITY;
        int bs = 0x7fffffff, br = 0x7fffffff;
        for (int r = 0; r < n; ++r)
            for (int j = tid; j < S; j += kThreads) {
                const float x = L[(size_t)r * S + j];
                if (before(pv, ps, pr, x, j, r) && before(x, j, r, bv, bs, br)) { bv = x; bs = j; br = r; }
            }
        wave_best(bv, bs, br);
        if (lane == 0) { sv[w] = bv; ss[w] = bs; sr[w] = br; }
        __syncthreads();
        bv = sv[0]; bs = ss[0]; br = sr[0];
#pragma unroll
        for (int x = 1; x < kThreads / 64; ++x)
            if (before(sv[x], ss[x], sr[x], bv, bs, br)) { bv = sv[x]; bs = ss[x]; br = sr[x]; }
        __syncthreads();
        if (tid == 0) final_[(size_t)b * k + q] = Final{bv, bs, br};
        pv = bv; ps = bs; pr = br;
    }
    if (tid == 0) { count[b] = m; flag[1 + b] = 0; }
}

// Uniform matrix: every next-state sees the same candidates fl(L_{t-1}(i)[r] + u), so one list of (c, i, r) per item and
// frame serves all states (L_t(j)[q] = fl(o_t[j] + c_q)).  One wave per item runs the whole time loop: every lane keeps
// its own top-k of its prev-states (i = lane, lane + 64, ...) with the early exit, and k rounds of a wave arg-max merge
// the 64 lane lists.  The final selection is the same merge over fl(o_{F-1}[j] + c_r) without the add of u.
template <int KMAX>
__global__ __launch_bounds__(64) void kb_uniform_kernel(const float *__restrict__ obs, const int32_t *__restrict__ frames,
                                                        float u, const float *__restrict__ initial,
                                                        int32_t *__restrict__ ptrs, Final *__restrict__ final_,
                                                        int32_t *__restrict__ count, int32_t *__restrict__ flag, int B, int T,
                                                        int S, int k) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int F = min(max(frames[b], 1), T);
    const float *o = obs + (size_t)b * T * S;
    bool bad = F >= 2 && bad_value(u);
    for (int j = lane; j < S; j += 64) bad |= bad_value(initial[j]) || bad_value(o[j]);
    // the shared list of frame t - 1 (the same for every lane); frame 0's entry of state i is o_0[i] + pi[i]
    __shared__ float cs[kMaxK];
    int n = 1;
    for (int t = 1; t <= F; ++t) {
        const bool last = t == F;                      // the final selection: over L_{F-1}, no add
        const float *row = o + (size_t)(t - 1) * S;
        float v[KMAX];
        int p[KMAX];
#pragma unroll
        for (int q = 0; q < KMAX; ++q) { v[q] = -INFINITY; p[q] = 0; }
        int sz = 0;
        float kth = -INFINITY;
        for (int i0 = lane; i0 < S; i0 += 64 * kU) {
            float xs[kU];
#pragma unroll
            for (int w = 0; w < kU; ++w) {
                const int i = i0 + 64 * w;
                xs[w] = i < S ? (t == 1 ? row[i] + initial[i] : row[i]) : 0.f;
                if (i < S && t >= 2) bad |= bad_value(row[i]);     // (row 0 was checked above)
            }
#pragma unroll
            for (int w = 0; w < kU; ++w) {
                const int i = i0 + 64 * w;
                if (i >= S) break;
                for (int r = 0; r < n; ++r) {
                    const float L = t == 1 ? xs[w] : xs[w] + cs[r];
                    const float cand = last ? L : L + u;
                    if (sz >= k && !(cand > kth)) break;
                    insert<KMAX>(v, p, cand, (i << 5) | r, sz, k);
                    sz = min(sz + 1, k);
                    kth = kth_of<KMAX>(v, k);
                }
            }
        }
        // merge: round q takes the best head of the 64 lane lists; the lane that gave it pops it (its list moves up one)
        const int mm = (int)min((long long)k, (long long)S * n);
        float nc[KMAX];
        int np[KMAX];
#pragma unroll
        for (int q = 0; q < KMAX; ++q) {
            nc[q] = 0.f;
            np[q] = 0;
            if (q >= mm) continue;
            const bool has = sz > 0;
            const int hs = has ? p[0] >> 5 : 0x7fffffff, hr = has ? p[0] & 31 : 0x7fffffff;
            float bv = has ? v[0] : -INFINITY;
            int bs = hs, br = hr;
            wave_best(bv, bs, br);
            if (has && bs == hs && br == hr) {
#pragma unroll
                for (int x = 0; x + 1 < KMAX; ++x) { v[x] = v[x + 1]; p[x] = p[x + 1]; }
                --sz;
            }
            nc[q] = bv;
            np[q] = (bs << 5) | br;
        }
        if (last) {
            if (lane == 0) {
#pragma unroll
                for (int q = 0; q < KMAX; ++q)
                    if (q < mm) final_[(size_t)b * k + q] = Final{nc[q], np[q] >> 5, np[q] & 31};
            }
            n = mm;
            break;
        }
#pragma unroll
        for (int q = 0; q < KMAX; ++q)
            if (q < mm && lane == q) ptrs[((size_t)b * (T - 1) + (t - 1)) * k + q] = np[q];
        // the new shared list holds c_q (without o_t[j], which the next frame adds per state)
        __syncthreads();
        if (lane == 0) {
#pragma unroll
            for (int q = 0; q < KMAX; ++q)
                if (q < mm) cs[q] = nc[q];
        }
        __syncthreads();
        n = mm;
    }
    bad = __any(bad);
    if (lane == 0) {
        count[b] = bad ? 0 : n;
        flag[1 + b] = bad ? 1 : 0;
    }
}

// One wave per item: lane q walks result rank q back through the stored pointers, writes its row of indices (padding
// t >= F with the last state) and its score.  Missing ranks: score -inf, indices -1; a flagged item: NaN scores, -1.
template <bool UNIFORM>
__global__ __launch_bounds__(64) void kb_walk_kernel(const int32_t *__restrict__ frames, const int32_t *__restrict__ ptrs,
                                                     const Final *__restrict__ final_, const int32_t *__restrict__ count,
                                                     const int32_t *__restrict__ flag, int32_t *__restrict__ indices,
                                                     float *__restrict__ scores, int T, int S, int k) {
    const int b = blockIdx.x, q = threadIdx.x;
    if (q >= k) return;
    const int F = min(max(frames[b], 1), T);
    const bool bad = flag[1 + b] != 0;
    const int m = count[b];
    int32_t *row = indices + ((size_t)b * k + q) * T;
    if (bad || q >= m) {
        scores[(size_t)b * k + q] = bad ? __builtin_nanf("") : -INFINITY;
        for (int t = 0; t < T; ++t) row[t] = -1;
        return;
    }
    const Final f = final_[(size_t)b * k + q];
    scores[(size_t)b * k + q] = f.score;
    // (in range by construction, like the pointers below: a selection round that found no entry would leave its start
    // values here, 0x7fffffff, and the first pointer read would leave the workspace)
    int s = min(max(f.state, 0), S - 1), r = min(max(f.rank, 0), k - 1);
    for (int t = F; t < T; ++t) row[t] = s;
    for (int t = F - 1; t >= 1; --t) {
        row[t] = s;
        const size_t at = ((size_t)b * (T - 1) + (t - 1)) * k + r;
        const int e = UNIFORM ? ptrs[at] : ptrs[at * S + s];
        s = min(max(e >> 5, 0), S - 1);          // (in range by construction; kept so that no read can leave the arrays)
        r = min(e & 31, k - 1);
    }
    row[0] = s;
}

}  // namespace kb
