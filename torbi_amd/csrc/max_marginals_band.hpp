// max_marginals_band.hpp -- the band route of max-marginals (torbi_hip_max_marginals_band*, torbi_amd/margins.py,
// MARGINALS.md "Band route"): max_marginals.hpp's values, by ==, for a matrix that holds ONE value outside a band, at the
// cost of the band.
//
// A is [next j][prev i] with A[j][i] == background (bit for bit) wherever i < j - reach_left or i > j + reach_right.  Rounding
// is monotone, so max_i fl(v[i] + background) = fl(max_i v[i] + background), and with pre[x] = max(v[0..x]),
// suf[x] = max(v[x..S-1]), pre[-1] = suf[S] = -inf:
//     forward   inner_t[j] = max( max_{i in band of j} fl(alpha_{t-1}[i] + A[j][i]),
//                                 fl(max(pre[j-rl-1], suf[j+rr+1]) + background) )        pre / suf over alpha_{t-1}
//               alpha_t[j] = fl(o_t[j] + inner_t[j])
//     backward  w[j] = fl(o_{t+1}[j] + beta_{t+1}[j])
//               beta_t[i]  = max( max_{j in band of i} fl(A[j][i] + w[j]),
//                                 fl(background + max(pre[i-rr-1], suf[i+rl+1])) )        pre / suf over w
// A row without an out-of-band column gets -inf from the second term.  Everything else is max_marginals.hpp's contract.
//
// Per call: banddiag::prepare_kernel (band_diagonals.hpp: the diagonals Df[k][j] = A[j][j - rl + k], [W][S]; the promise about
// the entries outside the band, one stray bit clears ok[0]; the matrix alarm), ONE mmb_kernel<G, SCAN> launch that runs every
// frame of both passes, mmb_final_kernel (NaN rows and a NaN score for alarmed items, and for every item where the promise is
// broken).
//
// mmb_kernel: a workgroup of kThreads owns G whole items, a thread owns states tid, tid + kThreads, ... of every item of the
// tile in both passes, so it reads back only alpha values it stored itself.  The previous row of each item (alpha_{t-1}
// forward, w backward) lives in LDS in two buffers with -inf halos of max(rl, rr) on both sides; the diagonals stream from
// L2, every load shared by the G items.  The backward pass has no second arrangement of the diagonals: with k = i - j + rl
// it reads Df[k][i + rl - k], consecutive lanes at consecutive addresses; where j = i + rl - k is no state the address still
// lies inside [0, W * S) (it is k (S - 1) + i + rl <= W S - rr - 1) and the value meets a -inf halo.  (That keeps the
// workspace at one [W][S] region and the backward loop at one more address register.)  With a finite background (SCAN) the
// prefix and suffix maxima of the G rows are built per frame as stream_band_forward_kernel builds its scans -- a run per
// thread, a wave scan, the wave totals --, values only; with background == -inf the second term is -inf and both scans are
// skipped.  The cell is dense_forward.hpp's add, add, max3 per two columns.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

#include "band_diagonals.hpp"
#include "scratch.hpp"
#include "wave_reduce.hpp"

namespace mmb {

constexpr int kMaxGroup = 4;                      // items per workgroup: instances <4>, <2>, <1>
constexpr int kThreads = 1024;                    // sixteen waves hide the L2 latency of the diagonals: at most 128 VGPRs
constexpr int kWaves = kThreads / 64;
constexpr int kMaxLdsBytes = banddiag::kMaxLdsBytes;   // (the wave totals go beside the dynamic part)
constexpr int kWorkgroups = 256;                  // G is halved until the launch has this many (one per CU of an MI355X)

__host__ __device__ inline int halo_of(int reach_left, int reach_right) { return reach_left > reach_right ? reach_left : reach_right; }
__host__ __device__ inline size_t row_words(int S, int halo) { return (size_t)S + 2 * (size_t)halo; }

// dynamic LDS of mmb_kernel<G>: rows [2][G][halo + S + halo] fp32, then per item the scans pre [S], suf [S]
__host__ __device__ inline size_t lds_bytes(int G, int S, int reach_left, int reach_right) {
    return ((size_t)2 * G * row_words(S, halo_of(reach_left, reach_right)) + (size_t)2 * G * S) * sizeof(float);
}

struct Layout {
    float *diag;                                  // [W][S]
    int32_t *alarm;                               // [B + 1] ([B]: the matrix)
    int32_t *ok;                                  // the verdict word
    size_t total;
};

// `base`: the caller's workspace aligned up to 256 bytes, or null for the byte count alone
inline Layout layout(char *base, int B, int S, int reach_left, int reach_right) {
    Scratch a(base);
    Layout l;
    l.diag = a.take<float>(((size_t)reach_left + reach_right + 1) * S);
    l.alarm = a.take<int32_t>((size_t)B + 1);
    l.ok = a.take<int32_t>(1);
    l.total = a.bytes + 256;                      // (room to align the caller's base)
    return l;
}

using banddiag::nonfinite;                        // NaN or +inf

// inclusive maximum over the lanes of a wave, towards higher lanes (UP) or lower ones
template <bool UP>
__device__ __forceinline__ float wave_scan_max(float v, int lane) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const float o = UP ? __shfl_up(v, off, 64) : __shfl_down(v, off, 64);
        if (UP ? lane >= off : lane + off < 64) v = fmaxf(v, o);
    }
    return v;
}

// pre[g][x] = max(row_g[0..x]), suf[g][x] = max(row_g[x..S-1]) for the items with live[g]: each thread a run of consecutive
// states [lo, hi), the runs joined by a wave scan and the sixteen wave totals.  cur: the rows, cur[g * RW + i]; scan: [G][2][S].
// Two barriers inside, none before (the caller's rows are published) and none after the last write's barrier.
template <int G>
__device__ __forceinline__ void scans(const float *cur, size_t RW, float *scan, float (*tot)[G][kWaves], const bool (&live)[G],
                                      int lo, int hi, int S, int lane, int wave) {
    float xv[G], yv[G];
#pragma unroll
    for (int g = 0; g < G; ++g) {
        xv[g] = yv[g] = -INFINITY;
        if (!live[g]) continue;
        const float *p = cur + (size_t)g * RW;
        float *pv = scan + (size_t)g * 2 * S, *sv = pv + S;
        float v = -INFINITY;
        for (int i = lo; i < hi; ++i) {
            v = fmaxf(v, p[i]);
            pv[i] = v;
        }
        const float ev = wave_scan_max<true>(v, lane);
        if (lane == 63) tot[0][g][wave] = ev;
        const float below = __shfl_up(ev, 1, 64);                 // this thread's offset within its wave: the lanes below
        xv[g] = lane == 0 ? -INFINITY : below;
        v = -INFINITY;
        for (int i = hi - 1; i >= lo; --i) {
            v = fmaxf(v, p[i]);
            sv[i] = v;
        }
        const float fv = wave_scan_max<false>(v, lane);
        if (lane == 0) tot[1][g][wave] = fv;
        const float above = __shfl_down(fv, 1, 64);
        yv[g] = lane == 63 ? -INFINITY : above;
    }
    __syncthreads();
#pragma unroll
    for (int g = 0; g < G; ++g) {
        if (!live[g]) continue;
        float *pv = scan + (size_t)g * 2 * S, *sv = pv + S;
        float x = xv[g], y = yv[g];
        for (int w = 0; w < wave; ++w) x = fmaxf(x, tot[0][g][w]);
        for (int w = wave + 1; w < kWaves; ++w) y = fmaxf(y, tot[1][g][w]);
        for (int i = lo; i < hi; ++i) {
            pv[i] = fmaxf(pv[i], x);
            sv[i] = fmaxf(sv[i], y);
        }
    }
    __syncthreads();
}

// acc[g] = max_k fl(row_g[k * RSTEP] + dq[k * dstep]) over the W diagonals, add, add, max3 per two of them; U loads of the
// diagonals in flight, each shared by the G items.  pj: the first in-band row entry of this state in item 0.
template <int G, int RSTEP>
__device__ __forceinline__ void band_max(float (&acc)[G], const float *pj, size_t RW, const float *dq, size_t dstep, int W) {
    constexpr int U = G == 4 ? 4 : 8;
    int k = 0;
    for (; k + U <= W; k += U) {
        float dv[U];
#pragma unroll
        for (int u = 0; u < U; ++u) dv[u] = dq[(size_t)(k + u) * dstep];
#pragma unroll
        for (int u = 0; u < U; u += 2)
#pragma unroll
            for (int g = 0; g < G; ++g)
                acc[g] = fmaxf(fmaxf(acc[g], pj[(ptrdiff_t)(g * RW) + (k + u) * RSTEP] + dv[u]),
                               pj[(ptrdiff_t)(g * RW) + (k + u + 1) * RSTEP] + dv[u + 1]);
    }
    for (; k < W; ++k) {
        const float dv = dq[(size_t)k * dstep];
#pragma unroll
        for (int g = 0; g < G; ++g) acc[g] = fmaxf(acc[g], pj[(ptrdiff_t)(g * RW) + k * RSTEP] + dv);
    }
}

// Every frame of both passes of G items.  grid (ceil(B / G)), block kThreads, dynamic LDS lds_bytes(G, ...).
//   forward   marg[b][t] = alpha_t (t < F), -inf (t >= F); the observation and initial alarms; scores[b] = max_j alpha_{F-1}[j]
//   backward  marg[b][t] = fl(alpha_t + beta_t) for t < F - 1, in place
template <int G, bool SCAN>
__global__ __launch_bounds__(kThreads) void mmb_kernel(const float *__restrict__ obs, const int32_t *__restrict__ frames,
                                                       const float *__restrict__ diag, const float *__restrict__ initial,
                                                       float background, int reach_left, int reach_right,
                                                       float *__restrict__ marg, float *__restrict__ scores,
                                                       int32_t *__restrict__ alarm, int B, int T, int S) {
    extern __shared__ float lds_f[];
    __shared__ float tot[2][G][kWaves];
    __shared__ float part[G][kWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b0 = blockIdx.x * G;
    const int W = reach_left + reach_right + 1;
    const int H = halo_of(reach_left, reach_right);
    const size_t RW = row_words(S, H);
    const size_t buffer = (size_t)G * RW;
    float *const rows = lds_f;                                   // [2][G][RW]
    float *const scan = lds_f + 2 * buffer;                      // [G][2][S]
    int F[G];
    int Fmax = 0;
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const int f = b0 + g < B ? frames[b0 + g] : 0;
        F[g] = b0 + g < B ? (f < 1 ? 1 : (f > T ? T : f)) : 0;
        Fmax = max(Fmax, F[g]);
    }
    for (size_t x = tid; x < 2 * buffer; x += kThreads) rows[x] = -INFINITY;          // (the halos stay -inf throughout)
    // rows t >= F
#pragma unroll
    for (int g = 0; g < G; ++g) {
        if (F[g] == 0) continue;
        float *const item = marg + (size_t)(b0 + g) * T * S;
        const size_t end = (size_t)T * S;
        for (size_t e = (size_t)F[g] * S + tid; e < end; e += kThreads) item[e] = -INFINITY;
    }
    __syncthreads();
    const int chunk = (S + kThreads - 1) / kThreads;
    const int lo = min(tid * chunk, S), hi = min(lo + chunk, S);
    bool seen[G];
#pragma unroll
    for (int g = 0; g < G; ++g) seen[g] = false;

    // ---- forward
    for (int t = 0; t < Fmax; ++t) {
        const float *cur = rows + (size_t)((t + 1) & 1) * buffer + H;            // cur[g * RW + i], i in -H .. S + H - 1
        float *nxt = rows + (size_t)(t & 1) * buffer + H;
        bool live[G];
#pragma unroll
        for (int g = 0; g < G; ++g) live[g] = t < F[g];
        if (SCAN && t > 0) scans<G>(cur, RW, scan, tot, live, lo, hi, S, lane, wave);
        float top[G];
#pragma unroll
        for (int g = 0; g < G; ++g) top[g] = -INFINITY;
        for (int j = tid; j < S; j += kThreads) {
            float acc[G], o[G];
#pragma unroll
            for (int g = 0; g < G; ++g) {                        // (the frame's observation is in flight beside the diagonals)
                acc[g] = -INFINITY;
                o[g] = live[g] ? obs[((size_t)(b0 + g) * T + t) * S + j] : 0.f;
            }
            if (t > 0) {
                band_max<G, 1>(acc, cur + j - reach_left, RW, diag + j, (size_t)S, W);
                if (SCAN) {
                    const int e0 = j - reach_left - 1, e1 = j + reach_right + 1;
#pragma unroll
                    for (int g = 0; g < G; ++g) {
                        const float *pv = scan + (size_t)g * 2 * S, *sv = pv + S;
                        const float out = fmaxf(e0 >= 0 ? pv[e0] : -INFINITY, e1 < S ? sv[e1] : -INFINITY);
                        acc[g] = fmaxf(acc[g], out + background);
                    }
                }
            }
            const float pi = t == 0 ? initial[j] : 0.f;
#pragma unroll
            for (int g = 0; g < G; ++g) {
                if (!live[g]) continue;
                const size_t at = ((size_t)(b0 + g) * T + t) * S + j;
                seen[g] |= nonfinite(o[g]) || nonfinite(pi);
                const float a = o[g] + (t == 0 ? pi : acc[g]);
                marg[at] = a;
                nxt[(size_t)g * RW + j] = a;
                top[g] = fmaxf(top[g], a);
            }
        }
#pragma unroll
        for (int g = 0; g < G; ++g) {
            if (t != F[g] - 1) continue;                                        // (the same for the whole workgroup)
            const float m = wavered::wave_reduce_f32(top[g], wavered::MaxOp());
            if (lane == 0) part[g][wave] = m;
        }
        __syncthreads();
#pragma unroll
        for (int g = 0; g < G; ++g) {
            if (t != F[g] - 1 || tid != 0) continue;
            float m = part[g][0];
            for (int w = 1; w < kWaves; ++w) m = fmaxf(m, part[g][w]);
            scores[b0 + g] = m;
        }
    }
#pragma unroll
    for (int g = 0; g < G; ++g)
        if (seen[g]) alarm[b0 + g] = 1;

    // ---- backward: phase t reads w_{t+1} = fl(o_{t+1} + beta_{t+1}) from buffer (t + 1) & 1 and leaves w_t in buffer t & 1
    for (int t = Fmax - 1; t >= 0; --t) {
        const float *cur = rows + (size_t)((t + 1) & 1) * buffer + H;
        float *nxt = rows + (size_t)(t & 1) * buffer + H;
        bool live[G];
        bool any = false;
#pragma unroll
        for (int g = 0; g < G; ++g) {
            live[g] = t < F[g] - 1;
            any |= live[g];
        }
        if (SCAN && any) scans<G>(cur, RW, scan, tot, live, lo, hi, S, lane, wave);
        for (int i = tid; i < S; i += kThreads) {
            float acc[G], o[G], a[G];
#pragma unroll
            for (int g = 0; g < G; ++g) {                        // (o_t and alpha_t are in flight beside the diagonals)
                acc[g] = -INFINITY;
                const size_t at = ((size_t)(b0 + g) * T + t) * S + i;
                o[g] = (t > 0 && t <= F[g] - 1) ? obs[at] : 0.f;
                a[g] = live[g] ? marg[at] : 0.f;
            }
            if (any) {
                // j = i + reach_left - k: the row backwards from i + reach_left, diag[k][j] at k (S - 1) + i + reach_left
                band_max<G, -1>(acc, cur + i + reach_left, RW, diag + i + reach_left, (size_t)S - 1, W);
                if (SCAN) {
                    const int e0 = i - reach_right - 1, e1 = i + reach_left + 1;
#pragma unroll
                    for (int g = 0; g < G; ++g) {
                        const float *pv = scan + (size_t)g * 2 * S, *sv = pv + S;
                        const float out = fmaxf(e0 >= 0 ? pv[e0] : -INFINITY, e1 < S ? sv[e1] : -INFINITY);
                        acc[g] = fmaxf(acc[g], background + out);
                    }
                }
            }
#pragma unroll
            for (int g = 0; g < G; ++g) {
                if (t > F[g] - 1) continue;
                const size_t at = ((size_t)(b0 + g) * T + t) * S + i;
                float beta = 0.f;
                if (live[g]) {
                    beta = acc[g];
                    marg[at] = a[g] + beta;
                }
                if (t > 0) nxt[(size_t)g * RW + i] = o[g] + beta;
            }
        }
        __syncthreads();
    }
}

// An alarmed item gets NaN in its rows t < F and a NaN score; so does every item, whatever its frames, where the promise is
// broken (ok[0] == 0).  Rows t >= F stay -inf.  grid (B), block 256.
__global__ __launch_bounds__(256) void mmb_final_kernel(const int32_t *__restrict__ frames, const int32_t *__restrict__ alarm,
                                                        const int32_t *__restrict__ ok, float *__restrict__ marg,
                                                        float *__restrict__ scores, int B, int T, int S) {
    const int b = blockIdx.x;
    const int f0 = frames[b];
    const int f = f0 < 1 ? 1 : (f0 > T ? T : f0);
    if (!(alarm[b] != 0 || (alarm[B] != 0 && f >= 2) || ok[0] == 0)) return;
    float *const item = marg + (size_t)b * T * S;
    const size_t n = (size_t)f * S;
    for (size_t e = threadIdx.x; e < n; e += 256) item[e] = NAN;
    if (threadIdx.x == 0) scores[b] = NAN;
}

}  // namespace mmb
