// path_entropy_log_band.hpp -- path entropy in LOG SPACE for a transition matrix that is -inf outside a band of up to 512
// entries (torbi_hip_path_entropy_log_band, torbi_amd/entropy.py forward_entropy_log_banded, ENTROPY.md "Log-space band
// route").
//
// Every other path-entropy kernel carries the scaled float32 row a_t: a filtered row that spans more than float32's range
// loses the states that would win later, and with them their share of the entropy.  This one runs the forward rows of
// forward_backward_log_band.hpp -- la_t, M_t, Z_t = sum_j exp(la_t[j]) and L, the same operations in the same order, so L is
// fb_log_band_kernel's bit for bit -- and beside them the conditional entropies h_t (natural logs in the contract, A
// [next][prev]):
//     h_0[j] = 0
//     e_i = A[j,i] + la_{t-1}[i]    lse_j = log sum_i exp(e_i)    q_i = exp(e_i - lse_j)            (i in the band of j)
//     h_t[j] = sum_i q_i (h_{t-1}[i] - log q_i)              (0 where lse_j = -inf; a term with q_i = 0 contributes 0)
//     prefix_t = log Z_t + (sum_j exp(la_t[j]) (h_t[j] - la_t[j])) / Z_t                            H = prefix_{F-1}
// which is entropy.py's recursion (h = log d + (D2 - D3) / d) with the constant of each row cancelled: q is the same
// whatever la_{t-1} is shifted by.  -q log q is not linear in the matrix, so the split "band minus constant, constant over
// everything" does not carry over: the background is -inf.
//
// Inside the launch everything is in BASE 2 (v_exp_f32 and v_log_f32 are base 2): rows and pack as in fbl, and the entropies
// in BITS, hb = h / ln 2, so that a term is w (hb - log2 w) with no constant in it; ln 2 comes in once per frame, where
// prefix_t is stored.
//
// Launches: fbl's pack of pass 0 alone (with the flag reset), fbl's verify, then ONE launch that runs every frame; a
// workgroup of 1024 threads owns G whole items, nothing waits across workgroups.  Plan, pack order and the way a lane walks
// the band are forward_backward_wide_band.hpp's.
//
// Phase A extends fbl::band_lse from a running pair to a running triple (m, s, k) per (state, item): with r = ref_of(m)
// and w_i = 2^(e2_i - r),
//     s = sum_i w_i                  k = sum_i w_i (hb_i - (e2_i - r))         (w_i == 0: the term is 0 by selection, so
//                                                                               0 x inf is never formed; a NaN propagates)
// m and s by fbl's operations in fbl's order, k beside them.  Where the reference moves from r to r', once per dquad, with
// f = 2^(m - r') (0 for m = -inf): s' = f s and k' = f (k + (r' - r) s); both references are finite by ref_of.  Per dquad a
// lane reads one more 16-byte LDS piece per item (the hb row) and spends the same 1.25 exponentials per term.
// Phase B, one thread per state (tid, tid + 1024, ...): the slices' triples combined in slice order by the same rule,
//     hb_t[j] = k / s + log2 s        (0 where m = -inf)
// then fbl's row steps: observation, x to the row in place | row maximum | la to the row, Z_t = sum 2^la, and the prefix
// numerator sum_j 2^la (hb - la), each term fp32, summed over the row in fp64 as peb::frame_sums sums v.
// prefix_t = ln 2 (log2 Z_t + numerator / Z_t) in fp64, rounded once.
//
// LDS of a tile: the head (fbl's: sum M_t in fp64, Z_{F-1}, L; then H), the fp64 wave sums of the numerator [G][16], two rows
// [G][stride] each (la with its -inf halo, hb whose halo is never weighted), the slice triples [KS][G][3][S4], the wave values
// [2][G][16] (row max, row sum).  Workspace: one pack, the prefix rows where the caller passes none, one flag.
//
// The order of every operation of an item is fixed by (S, band) alone: an item's bits depend neither on G nor on its tile
// nor on the batch.  No float atomics, vector stores only.
#pragma once

#include "forward_backward_log_band.hpp"
#include "path_entropy_band.hpp"

namespace pel {

using fbw::f4;
using fbw::Plan;
using fbw::barrier;
using fbl::ex2;
using fbl::lg2;
using fbl::ref_of;
constexpr int kThreads = fbl::kThreads, kWaves = fbl::kWaves;
constexpr int kMaxStates = fbl::kMaxStates, kMaxWindow = fbl::kMaxWindow;
constexpr int kMaxGroup = 2;                 // items per workgroup (4, at 12 G running values a lane, needs scratch within 128 VGPRs)
constexpr int kMaxLdsBytes = fbl::kMaxLdsBytes;
constexpr int kBlockStates = fbl::kBlockStates;
constexpr int kParts = 2;                    // wave values of a frame: row max, row sum

struct Layout : Plan { float *Pf, *prefix; int32_t *flag; size_t total; };

// `base`: the caller's workspace aligned up to 256 bytes, or null for the byte count alone
inline Layout layout(char *base, int B, int T, int S, int reach_left, int reach_right) {
    Layout l;
    static_cast<Plan &>(l) = fbw::plan_of(S, reach_left, reach_right);
    Scratch a(base);
    l.Pf = a.take<float>(fbw::pack_floats(l, 0));
    l.prefix = a.take<float>((size_t)B * T);
    l.flag = a.take<int32_t>(1);
    l.total = a.bytes + 256;                 // (room to align the caller's base)
    return l;
}

constexpr int kHeadBytes = fbl::kHeadBytes + fbl::kMaxGroup * 4;         // fbl's head, then H [kMaxGroup]
__host__ __device__ inline size_t lds_bytes(int G, const Plan &p) {
    return kHeadBytes + (size_t)G * kWaves * 8 +
           (size_t)G * 4 * ((size_t)2 * p.stride + (size_t)3 * p.slices * p.S4 + kParts * kWaves);
}

// host: pass 0 of fbl's pack (no backward pack is written: the grid has one pass), then fbl's check of the promise
inline hipError_t pack_and_verify(const float *A, const Layout &l, int S, hipStream_t st) {
    const int most = l.Dq[0] > l.Dq[1] ? l.Dq[0] : l.Dq[1];
    hipLaunchKernelGGL(fbl::fb_log_pack_kernel, dim3((unsigned)(l.blocks * most), 1), dim3(256), 0, st, A, l.Pf,
                       static_cast<float *>(nullptr), l.flag, -INFINITY, static_cast<const Plan &>(l), S);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(fbl::fb_log_verify_kernel, dim3(S), dim3(64), 0, st, A, l.flag, -INFINITY, l.reach_left, l.reach_right, S);
    return hipGetLastError();
}

// One tile: fbl's (the frames of the items, the head, the la rows, the wave values), with the hb rows, the triples and H
template <int G>
struct Tile : fbl::Tile<G> {
    float *Hs, *hrows, *slice;               // [kMaxGroup] prefix_{F-1}; [G][stride]; [KS][G][3][S4]
    double *vsum;                            // [G][16] wave sums of the prefix numerator
    __device__ __forceinline__ Tile(unsigned char *lds, const Plan &p) : fbl::Tile<G>(lds, p) {
        Hs = reinterpret_cast<float *>(lds + fbl::kHeadBytes);
        vsum = reinterpret_cast<double *>(lds + kHeadBytes);
        this->rows = reinterpret_cast<float *>(vsum + G * kWaves);       // (16-byte aligned: 80 + 128 G bytes on)
        hrows = this->rows + (size_t)G * p.stride;
        slice = hrows + (size_t)G * p.stride;
        this->smax = this->ssum = nullptr;
        this->part = slice + (size_t)p.slices * G * 3 * p.S4;
    }
};

// Whether a lane keeps the next dquad of band in flight and the upper pieces of both row windows for the next dquad: both
// instantiated tiles do (119 VGPRs at G = 2).  A tile of 4 needs scratch with or without, so there is none.
constexpr bool keeps_ahead(int G) { return G <= 2; }

// ---- phase A of one lane: for its 4 states n and every item g the triple (m, s, k) over the dquads [q_lo, q_hi) and their
// diagonals c, the terms e2 = P[q][c][n] + la_g[4 q + c + n] weighting hb_g[4 q + c + n] ----
// `pack`: the lane's first piece of its block (piece (q, c) 64 (4 q + c) f4 on); `row`: item 0's la row at the lane's first
// state (item g: g * stride floats on; the hb row of the same item `hofs` floats on).  q_lo < q_hi, the same in every lane.
template <int G>
__device__ __forceinline__ void band_entropy(const f4 *__restrict__ pack, const float *row, int hofs, int stride, int q_lo,
                                             int q_hi, float (&m)[G][4], float (&s)[G][4], float (&k)[G][4]) {
    constexpr bool kAhead = keeps_ahead(G);
    f4 band[4], next[4], lo[kAhead ? G : 1], hlo[kAhead ? G : 1];
#pragma unroll
    for (int c = 0; c < 4; ++c) band[c] = pack[(size_t)(4 * q_lo + c) * 64];
    if (kAhead) {
#pragma unroll
        for (int g = 0; g < G; ++g) {
            lo[g] = *reinterpret_cast<const f4 *>(row + g * stride + 4 * q_lo);
            hlo[g] = *reinterpret_cast<const f4 *>(row + hofs + g * stride + 4 * q_lo);
        }
    }
    for (int q = q_lo; q < q_hi; ++q) {
        const int qn = q + 1 < q_hi ? q + 1 : q_hi - 1;                  // (past the slice: its last dquad again)
        if (kAhead) {
#pragma unroll
            for (int c = 0; c < 4; ++c) next[c] = pack[(size_t)(4 * qn + c) * 64];
        }
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const f4 low = kAhead ? lo[g] : *reinterpret_cast<const f4 *>(row + g * stride + 4 * q);
            const f4 hi = *reinterpret_cast<const f4 *>(row + g * stride + 4 * q + 4);
            const f4 hlow = kAhead ? hlo[g] : *reinterpret_cast<const f4 *>(row + hofs + g * stride + 4 * q);
            const f4 hhi = *reinterpret_cast<const f4 *>(row + hofs + g * stride + 4 * q + 4);
            const float v[8] = {low.x, low.y, low.z, low.w, hi.x, hi.y, hi.z, hi.w};
            const float hb[8] = {hlow.x, hlow.y, hlow.z, hlow.w, hhi.x, hhi.y, hhi.z, hhi.w};
#pragma unroll
            for (int n = 0; n < 4; ++n) {
                float term[4];
#pragma unroll
                for (int c = 0; c < 4; ++c) term[c] = band[c][n] + v[n + c];
                const float top = __builtin_fmaxf(__builtin_fmaxf(term[0], term[1]), __builtin_fmaxf(term[2], term[3]));
                const float now = __builtin_fmaxf(m[g][n], top), ref = ref_of(now);
                const float f = ex2(m[g][n] - ref);
                float sum = s[g][n] * f;
                float ent = f * (k[g][n] + (ref - ref_of(m[g][n])) * s[g][n]);
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const float d = term[c] - ref, w = ex2(d);           // (a NaN term loses the maximum and wins here)
                    sum += w;
                    ent += w == 0.f ? 0.f : w * (hb[n + c] - d);
                }
                m[g][n] = now;
                s[g][n] = sum;
                k[g][n] = ent;
            }
            if (kAhead) {
                lo[g] = hi;
                hlo[g] = hhi;
            }
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) band[c] = kAhead ? next[c] : pack[(size_t)(4 * qn + c) * 64];
    }
}

// phase A of the workgroup: every owning wave's slice triples to tile.slice (the caller's barrier follows)
template <int G>
__device__ __forceinline__ void band_phase(const Tile<G> &tile, const Plan &p, const float *__restrict__ Pf, int S) {
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (wave >= p.blocks * p.slices) return;
    const int blk = wave % p.blocks, sl = wave / p.blocks, Dq = p.Dq[0];
    const int per = (Dq + p.slices - 1) / p.slices;
    const int q_lo = sl * per, q_hi = q_lo + per < Dq ? q_lo + per : Dq;
    const int x0 = kBlockStates * blk + 4 * lane;
    if (x0 >= S) return;
    float m[G][4], s[G][4], k[G][4];
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            m[g][n] = -INFINITY;
            s[g][n] = k[g][n] = 0.f;
        }
    if (q_lo < q_hi)
        band_entropy<G>(reinterpret_cast<const f4 *>(Pf) + (size_t)blk * Dq * 256 + lane, tile.rows + x0, G * p.stride, p.stride,
                        q_lo, q_hi, m, s, k);
#pragma unroll
    for (int g = 0; g < G; ++g) {
        float *out = tile.slice + ((size_t)sl * G + g) * 3 * p.S4 + x0;
        *reinterpret_cast<f4 *>(out) = f4{m[g][0], m[g][1], m[g][2], m[g][3]};
        *reinterpret_cast<f4 *>(out + p.S4) = f4{s[g][0], s[g][1], s[g][2], s[g][3]};
        *reinterpret_cast<f4 *>(out + 2 * p.S4) = f4{k[g][0], k[g][1], k[g][2], k[g][3]};
    }
}

// state j of item g from the slices in their order: `band` = log2 of the band sum, by fbl::product_of's operations; `hb`
template <int G>
__device__ __forceinline__ void combine(const Tile<G> &tile, const Plan &p, int g, int j, float &band, float &hb) {
    const float *part = tile.slice + (size_t)g * 3 * p.S4 + j;
    const size_t step = (size_t)G * 3 * p.S4;
    float m = part[0];
    for (int i = 1; i < p.slices; ++i) m = __builtin_fmaxf(m, part[i * step]);
    const float ref = ref_of(m);
    float s = 0.f, k = 0.f;
    for (int i = 0; i < p.slices; ++i) {
        const float mi = part[i * step], si = part[i * step + p.S4], ki = part[i * step + 2 * p.S4];
        const float f = ex2(mi - ref);
        s += si * f;
        k += f * (ki + (ref - ref_of(mi)) * si);
    }
    const float l = lg2(s);                                              // (s >= 1, or 0 with m = -inf, or NaN)
    band = ref + l;
    hb = m == -INFINITY ? 0.f : k / s + l;                               // (0 where no path reaches j)
}

// ---- every frame of G items per workgroup; grid ceil(B / G), dynamic LDS lds_bytes(G, plan) ----
template <int G>
__global__ __launch_bounds__(kThreads) void pe_log_band_kernel(const float *__restrict__ obs, const int32_t *__restrict__ frames,
                                                               const float *__restrict__ initial, const float *__restrict__ Pf,
                                                               const int32_t *__restrict__ flag, float *__restrict__ prefix,
                                                               float *__restrict__ entropy, float *__restrict__ loglik, Plan p,
                                                               int B, int T, int S) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    Tile<G> tile(lds_raw, p);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, stride = p.stride;
    const int b0 = tile.b0 = blockIdx.x * G;
    int Fmax = 1;
#pragma unroll
    for (int g = 0; g < G; ++g) {
        tile.F[g] = b0 + g < B ? fb::frames_of(frames, b0 + g, T) : 0;   // (0: an item beyond the batch never takes a step)
        Fmax = tile.F[g] > Fmax ? tile.F[g] : Fmax;
    }
    const int *F = tile.F;
    for (int e = tid; e < G * stride; e += kThreads) {                   // (the halos stay as they are all pass long)
        tile.rows[e] = -INFINITY;
        tile.hrows[e] = 0.f;
    }
#pragma unroll
    for (int g = 0; g < G; ++g) {                                        // prefix entries an item does not have
        if (b0 + g >= B) continue;
        for (int t = F[g] + tid; t < T; t += kThreads) prefix[(size_t)(b0 + g) * T + t] = 0.f;
    }
    if (tid < G) {
        tile.Msum[tid] = 0.;
        tile.Zlast[tid] = 0.f;
        tile.Hs[tid] = 0.f;
    }
    barrier();

    float *const cur = tile.rows + p.left4[0], *const hcur = tile.hrows + p.left4[0];
    for (int t = 0; t < Fmax; ++t) {
        if (t > 0) {
            band_phase(tile, p, Pf, S);
            barrier();
        }
        float top[G];
#pragma unroll
        for (int g = 0; g < G; ++g) top[g] = -INFINITY;
        for (int j = tid; j < S; j += kThreads)
#pragma unroll
            for (int g = 0; g < G; ++g) {
                if (t >= F[g]) continue;
                const float o = obs[((size_t)(b0 + g) * T + t) * S + j];
                float band = 0.f, hb = 0.f;
                if (t > 0) combine(tile, p, g, j, band, hb);
                const float x = t == 0 ? (initial[j] + o) * fbl::kLog2e : o * fbl::kLog2e + band;
                cur[g * stride + j] = x;
                hcur[g * stride + j] = hb;
                top[g] = fb::nan_max(top[g], x);
            }
        fbl::to_waves<G, true>(tile, 0, top);
        barrier();
        fbl::from_waves<G, true>(tile, 0, top);
        float sum[G];
        double vacc[G];
#pragma unroll
        for (int g = 0; g < G; ++g) {
            top[g] = ref_of(top[g]);
            if (tid == 0 && t < F[g]) tile.Msum[g] += (double)top[g];
            sum[g] = 0.f;
            vacc[g] = 0.;
        }
        for (int j = tid; j < S; j += kThreads)
#pragma unroll
            for (int g = 0; g < G; ++g) {
                if (t >= F[g]) continue;
                const float la = cur[g * stride + j] - top[g];
                cur[g * stride + j] = la;
                const float e = ex2(la);
                sum[g] += e;
                vacc[g] += (double)(e == 0.f ? 0.f : e * (hcur[g * stride + j] - la));
            }
        fbl::to_waves<G, false>(tile, 1, sum);
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const double v = fbb::wave_sum(vacc[g]);
            if (lane == 0) tile.vsum[g * kWaves + wave] = v;
        }
        barrier();
        fbl::from_waves<G, false>(tile, 1, sum);                         // (a butterfly: every lane takes part)
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const double v = peb::sum16(tile.vsum[g * kWaves + (tid & 15)]);
            if (tid == 0 && t == F[g] - 1) tile.Zlast[g] = sum[g];
            if (tid == g * 64 && t < F[g]) {                             // prefix_t, rounded once
                const float h = (float)((log2((double)sum[g]) + v / (double)sum[g]) * fbl::kLn2D);
                prefix[(size_t)(b0 + g) * T + t] = h;
                if (t == F[g] - 1) tile.Hs[g] = h;
            }
        }
    }

    // ---- L = ln 2 (sum M_t + log2 Z_{F-1}), fbl's; NaN when that is NaN or +inf, or the promise is broken ----
    if (tid == 0) {
        const bool broken = *flag != 0;
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const double L = (tile.Msum[g] + log2((double)tile.Zlast[g])) * fbl::kLn2D;
            const float out = (L != L || L == (double)INFINITY || broken) ? NAN : (float)L;
            tile.L[g] = out;
            if (b0 + g < B) loglik[b0 + g] = out;
        }
    }
    barrier();                                                           // (L, H and the prefix entries of other threads)
    // an item whose L is not finite (or a broken promise: L is NaN then): a NaN entropy and NaN in its prefix entries t < F
#pragma unroll
    for (int g = 0; g < G; ++g) {
        if (b0 + g >= B) continue;
        const bool bad = !isfinite(tile.L[g]);
        if (tid == 0) entropy[b0 + g] = bad ? NAN : tile.Hs[g];
        if (!bad) continue;
        for (int t = tid; t < F[g]; t += kThreads) prefix[(size_t)(b0 + g) * T + t] = NAN;
    }
}

}  // namespace pel
