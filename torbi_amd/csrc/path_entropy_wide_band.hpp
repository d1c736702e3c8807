// path_entropy_wide_band.hpp -- path entropy for a transition matrix that holds ONE value outside a band of up to 512
// entries (torbi_hip_path_entropy_wide_band, torbi_amd/entropy.py forward_entropy_wide_banded, ENTROPY.md "Wide band route").
//
// The model, the contract, the deferred division by c_t, the non-finite rules and the promise flag are path_entropy_band.hpp's,
// term for term: with ebg = exp(background), gbg = ebg * background (both 0 for -inf), Df = E - ebg and Dg = G - gbg over the
// band (G = E o A, 0 where A = -inf), c = c_{t-1},
//     d  = (Df a) / c + ebg      D2 = (Df v + log c * Df a) / c + ebg * prefix_{t-1}      D3 = (Dg a) / c + gbg
//     h_t[j] = log d + (D2 - D3) / d   (0 where d = 0)      a_t[j] = e_t[j] d[j]      v_t[j] = a_t[j] h_t[j] - xlogx(a_t[j])
// New is how the three band sums of a frame are done: forward_backward_wide_band.hpp's pack in lane order, its register tile of
// 4 states x G items a lane and its aligned 16-byte LDS pieces (fbw::Plan, pass 0 alone), carrying the pair (a, v) against the
// two matrices at once.  pe_band_kernel issues two 4-byte L2 loads and one 8-byte LDS read per 3 G multiply-adds; here a dquad
// is 8 x 16 B of band and 2 G x 16 B of rows for 48 G.
//
// Pack (once per call; clipped positions are 0), both in fb_wide_pack_kernel's layout:
//     Pf[256-state block b][dquad q][diagonal c of the quad][lane l][4 states] = E(x = 256 b + 4 l + n, diagonal 4 q + c) - ebg
//     Pg likewise with G - gbg                                                  1.08 MB each at 1440 states and 175 diagonals
//
// A frame takes two phases and two barriers:
//   A  Wave w < blocks * slices owns block w % blocks and slice w / blocks of the dquads; a lane owns 4 consecutive states x
//      the G items.  Per dquad it loads 4 x 16 B of Pf and 4 x 16 B of Pg (global_load_dwordx4, half a dquad ahead of
//      its use) and per item ONE new 16-byte piece of the a row and one of the v row (the upper halves of the last
//      ones are kept), for 48 G multiply-adds: sa += Pf a, sv += Pf v, sg += Pg a.  The slice's three sums go to LDS.
//   B  a thread per state (tid, tid + 1024, ...): the slices of a state are added in slice order, then the formulas above; a and
//      v are written in place (every reader is behind the barrier) and summed for c_t and prefix_t.
// The observation of a thread's first states is asked for before phase A.
//
// LDS of a tile: the a rows [G][stride] and the v rows [G][stride] (TWO float rows, not pe_band_kernel's 8-byte pairs, so that
// a lane's 16-byte piece is four consecutive states of one quantity; state x at left4[0] + x, zeros elsewhere), the slice sums
// [KS][G][3][S4], the wave sums of a (fp32) and of v (fp64) by parity of t, H [G] and fbb's fp64 sums of L.
//
// Reductions and the end of the call are pe_band_kernel's own code (peb::frame_sums, fbb::log_likelihood): c_t in fp32 and
// sum_j v_t[j] in fp64 by the same butterflies, prefix_t in fp64 from the two, rounded once.  The order of every sum of an item
// is fixed by (S, band) alone: dquads ascending and diagonals ascending within a slice, slices ascending, a thread's states in
// order, then the butterflies.  An item's bits depend neither on G nor on its tile nor on the batch.  No float atomics, vector
// stores only, nothing waits across workgroups.
//
// Packed fp32: the kernels carry fbw's no-packed-fp32-ops attribute.  The three sums of a state are independent chains that a
// packing compiler would gladly pair (sa with sv share Pf), and a paired multiply-add need not round as two scalar fmaf do in
// every form; the bits an item gets are promised not to depend on how the compiler groups items or sums, so every multiply-add
// stays one scalar v_fma_f32.  The price is fbw's: everything the kernels call is forced inline, the barrier is fbw::barrier,
// 16-byte pieces are fbw::f4.  profiles/path_entropy_wide_band_kernel_registers.txt counts the calls and the packed
// instructions in the ISA: none.
#pragma once

#include "forward_backward_wide_band.hpp"
#include "path_entropy_band.hpp"

namespace pew {

using fbw::f4;
using fbw::Plan;

constexpr int kThreads = fbb::kThreads, kWaves = fbb::kWaves;
constexpr int kMaxStates = fbw::kMaxStates;
constexpr int kMaxWindow = fbw::kMaxWindow;
constexpr int kMaxGroup = 2;                 // items per workgroup (4, at 12 G sums and 8 G row halves a lane, needs scratch within 128 VGPRs)
constexpr int kMaxLdsBytes = 160 * 1024;     // the LDS of a compute unit (a workgroup of 1024 threads is alone on it anyway)

#if defined(__HIP_DEVICE_COMPILE__)
#define PEW_KERNEL __global__ __attribute__((target("no-packed-fp32-ops")))
#else
#define PEW_KERNEL __global__
#endif

struct Layout : Plan { float *Pf, *Pg, *m, *c, *prefix; int32_t *flag; size_t total; };

// `base`: the caller's workspace aligned up to 256 bytes, or null for the byte count alone
inline Layout layout(char *base, int B, int T, int S, int reach_left, int reach_right) {
    Layout l;
    static_cast<Plan &>(l) = fbw::plan_of(S, reach_left, reach_right);
    Scratch a(base);
    l.Pf = a.take<float>(fbw::pack_floats(l, 0));
    l.Pg = a.take<float>(fbw::pack_floats(l, 0));
    l.m = a.take<float>((size_t)B * T);
    l.c = a.take<float>((size_t)B * T);
    l.prefix = a.take<float>((size_t)B * T);
    l.flag = a.take<int32_t>(1);
    l.total = a.bytes + 256;                 // (room to align the caller's base)
    return l;
}

// LDS of a tile of G items, in this order: fp64 wave sums of L [G][16] and L [G]; fp64 wave sums of v [2][G][16]; a rows
// [G][stride]; v rows [G][stride]; slices [KS][G][3][S4]; wave sums of a [2][G][16]; H [G]
__host__ __device__ inline size_t lds_bytes(int G, const Plan &p) {
    return fbw::rows_offset(G) + (size_t)G * 2 * kWaves * 8 +
           (size_t)G * 4 * ((size_t)2 * p.stride + (size_t)3 * p.slices * p.S4 + 2 * kWaves + 1);
}

// ---- both packs, E - ebg and G - gbg; resets the promise flag.  grid blocks * Dq[0], block 256 = 4 diagonals x 64 lanes ----
PEW_KERNEL __launch_bounds__(256) void pe_wide_pack_kernel(const float *__restrict__ A, float *__restrict__ Pf,
                                                            float *__restrict__ Pg, int32_t *__restrict__ flag, float ebg,
                                                            float gbg, Plan p, int S) {
    if (blockIdx.x == 0 && threadIdx.x == 0) *flag = 0;
    const int Dq = p.Dq[0], blk = (int)blockIdx.x / Dq, q = (int)blockIdx.x - blk * Dq;
    const int c = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int k = 4 * q + c - (p.left4[0] - p.left[0]);                  // the diagonal of the band, 0 <= k < W
    float f[4], g[4];
#pragma unroll
    for (int n = 0; n < 4; ++n) {
        const int x = fbw::kBlockStates * blk + 4 * lane + n, y = x - p.left[0] + k;     // next state, prev state
        f[n] = g[n] = 0.f;
        if (k >= 0 && k < p.W && x < S && y >= 0 && y < S) {
            const float a = A[(size_t)x * S + y], e = expf(a);
            f[n] = e - ebg;
            g[n] = (a == -INFINITY ? 0.f : e * a) - gbg;
        }
    }
    const size_t at = (((size_t)blk * Dq + q) * 4 + c) * 64 + lane;
    reinterpret_cast<f4 *>(Pf)[at] = f4{f[0], f[1], f[2], f[3]};
    reinterpret_cast<f4 *>(Pg)[at] = f4{g[0], g[1], g[2], g[3]};
}

// host: the packs, then fb_band_verify_kernel's check of the promise (which sets the flag the launch above reset)
inline hipError_t pack_and_verify(const float *A, const Layout &l, float ebg, float gbg, float background, int S, hipStream_t st) {
    hipLaunchKernelGGL(pe_wide_pack_kernel, dim3((unsigned)(l.blocks * l.Dq[0])), dim3(256), 0, st, A, l.Pf, l.Pg, l.flag, ebg, gbg,
                       static_cast<const Plan &>(l), S);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(fbb::fb_band_verify_kernel, dim3(S), dim3(64), 0, st, A, l.flag, background, l.reach_left, l.reach_right, S);
    return hipGetLastError();
}

// phase-B states of a thread whose observation is asked for before phase A (a tile of 2 has no registers to hold them)
constexpr int early_states(int G) { return G <= 1 ? 2 : 0; }

// One tile: pe_band_kernel's (the frames of the items, the sums of L, of a and of v, H), with this kernel's rows and slices
template <int G>
struct Tile : peb::Tile<G> {
    float *arow, *vrow, *slice;              // [G][stride] each; [KS][G][3][S4]
    __device__ __forceinline__ Tile(unsigned char *lds, const Plan &p, int S) : peb::Tile<G>(lds, 0, 0, S) {
        this->lsum = reinterpret_cast<double *>(lds);
        this->Ls = this->lsum + G * kWaves;
        this->vsum = reinterpret_cast<double *>(lds + fbw::rows_offset(G));
        arow = reinterpret_cast<float *>(this->vsum + 2 * G * kWaves);   // (16-byte aligned: rows_offset is, 256 G bytes on)
        vrow = arow + (size_t)G * p.stride;
        slice = vrow + (size_t)G * p.stride;
        this->asum = slice + (size_t)p.slices * G * 3 * p.S4;
        this->Hs = this->asum + 2 * G * kWaves;
        this->rows = arow;
        this->pairs = nullptr;
        this->stride = p.stride;
    }
};

// ---- phase A of one lane: over the dquads [q_lo, q_hi), for n < 4 and every item g,
//     sa[g][n] += Pf[q][c][n] * a_g[4 q + c + n]      sv[g][n] += Pf[q][c][n] * v_g[4 q + c + n]      sg[g][n] += Pg[q][c][n] * a_g[..]
// `pf`, `pg`: the lane's first piece of its block (piece (q, c) 64 (4 q + c) f4 on); `arow`: item 0's a row at the lane's first
// state (item g: g * stride floats on; the v row of the same item `vofs` floats on).  q_lo < q_hi, the same in every lane.
// A lane holds 16 registers of Pf and 16 of Pg and multiplies one while the other is on its way: Pg of this dquad during the
// Pf half, Pf of the next dquad during the Pg half ----
template <int G>
__device__ __forceinline__ void band_sums(const f4 *__restrict__ pf, const f4 *__restrict__ pg, const float *arow, int vofs,
                                          int stride, int q_lo, int q_hi, float (&sa)[G][4], float (&sv)[G][4],
                                          float (&sg)[G][4]) {
    f4 bf[4], bg[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        bf[c] = pf[(size_t)(4 * q_lo + c) * 64];
        bg[c] = pg[(size_t)(4 * q_lo + c) * 64];
    }
    f4 alo[G], vlo[G];
#pragma unroll
    for (int g = 0; g < G; ++g) {
        alo[g] = *reinterpret_cast<const f4 *>(arow + g * stride + 4 * q_lo);
        vlo[g] = *reinterpret_cast<const f4 *>(arow + vofs + g * stride + 4 * q_lo);
    }
    for (int q = q_lo; q < q_hi; ++q) {
        const int qn = q + 1 < q_hi ? q + 1 : q_hi - 1;                  // (past the slice: its last dquad again)
        f4 ahi[G];
        // the Pf half: sa and sv
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const f4 hi = ahi[g] = *reinterpret_cast<const f4 *>(arow + g * stride + 4 * q + 4);
            const f4 vhi = *reinterpret_cast<const f4 *>(arow + vofs + g * stride + 4 * q + 4);
            const float a[8] = {alo[g].x, alo[g].y, alo[g].z, alo[g].w, hi.x, hi.y, hi.z, hi.w};
            const float v[8] = {vlo[g].x, vlo[g].y, vlo[g].z, vlo[g].w, vhi.x, vhi.y, vhi.z, vhi.w};
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const float f[4] = {bf[c].x, bf[c].y, bf[c].z, bf[c].w};
#pragma unroll
                for (int n = 0; n < 4; ++n) {
                    sa[g][n] = fmaf(f[n], a[n + c], sa[g][n]);
                    sv[g][n] = fmaf(f[n], v[n + c], sv[g][n]);
                }
            }
            vlo[g] = vhi;
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) bf[c] = pf[(size_t)(4 * qn + c) * 64];
        // the Pg half: sg
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const f4 hi = ahi[g];
            const float a[8] = {alo[g].x, alo[g].y, alo[g].z, alo[g].w, hi.x, hi.y, hi.z, hi.w};
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const float w[4] = {bg[c].x, bg[c].y, bg[c].z, bg[c].w};
#pragma unroll
                for (int n = 0; n < 4; ++n) sg[g][n] = fmaf(w[n], a[n + c], sg[g][n]);
            }
            alo[g] = hi;
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) bg[c] = pg[(size_t)(4 * qn + c) * 64];
    }
}

// phase A of the workgroup: every owning wave's three slice sums to tile.slice (the caller's barrier follows)
template <int G>
__device__ __forceinline__ void band_phase(const Tile<G> &tile, const Plan &p, const float *__restrict__ Pf,
                                           const float *__restrict__ Pg, int S) {
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (wave >= p.blocks * p.slices) return;
    const int blk = wave % p.blocks, sl = wave / p.blocks, Dq = p.Dq[0];
    const int per = (Dq + p.slices - 1) / p.slices;
    const int q_lo = sl * per, q_hi = q_lo + per < Dq ? q_lo + per : Dq;
    const int x0 = fbw::kBlockStates * blk + 4 * lane;
    if (x0 >= S) return;
    float sa[G][4], sv[G][4], sg[G][4];
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
        for (int n = 0; n < 4; ++n) sa[g][n] = sv[g][n] = sg[g][n] = 0.f;
    if (q_lo < q_hi) {
        const size_t first = (size_t)blk * Dq * 256 + lane;
        band_sums<G>(reinterpret_cast<const f4 *>(Pf) + first, reinterpret_cast<const f4 *>(Pg) + first, tile.arow + x0,
                     G * p.stride, p.stride, q_lo, q_hi, sa, sv, sg);
    }
#pragma unroll
    for (int g = 0; g < G; ++g) {
        float *out = tile.slice + ((size_t)sl * G + g) * 3 * p.S4 + x0;
        *reinterpret_cast<f4 *>(out) = f4{sa[g][0], sa[g][1], sa[g][2], sa[g][3]};
        *reinterpret_cast<f4 *>(out + p.S4) = f4{sv[g][0], sv[g][1], sv[g][2], sv[g][3]};
        *reinterpret_cast<f4 *>(out + 2 * p.S4) = f4{sg[g][0], sg[g][1], sg[g][2], sg[g][3]};
    }
}

// ---- every frame of G items per workgroup; grid ceil(B / G), dynamic LDS lds_bytes(G, plan) ----
template <int G>
PEW_KERNEL __launch_bounds__(kThreads) void pe_wide_band_kernel(const float *__restrict__ obs, const int32_t *__restrict__ frames,
                                                                const float *__restrict__ initial, const float *__restrict__ Pf,
                                                                const float *__restrict__ Pg, const float *__restrict__ m,
                                                                float *__restrict__ cbuf, const int32_t *__restrict__ flag,
                                                                float *__restrict__ prefix, float *__restrict__ entropy,
                                                                float *__restrict__ loglik, float ebg, float gbg, Plan p, int B,
                                                                int T, int S) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    constexpr int kEarly = early_states(G);
    Tile<G> tile(lds_raw, p, S);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int stride = p.stride, S4 = p.S4, KS = p.slices, b0 = blockIdx.x * G;
    tile.b0 = b0;
    tile.Fmax = 1;
#pragma unroll
    for (int g = 0; g < G; ++g) {
        tile.F[g] = b0 + g < B ? fb::frames_of(frames, b0 + g, T) : 0;    // (0: an item beyond the batch never takes a step)
        tile.Fmax = tile.F[g] > tile.Fmax ? tile.F[g] : tile.Fmax;
    }
    const int *F = tile.F;
    const int Fmax = tile.Fmax;
    for (int e = tid; e < 2 * G * stride; e += kThreads) tile.arow[e] = 0.f;     // (both rows; all but the states stay zero)
    // prefix entries an item does not have
#pragma unroll
    for (int g = 0; g < G; ++g) {
        if (b0 + g >= B) continue;
        for (int t = F[g] + tid; t < T; t += kThreads) prefix[(size_t)(b0 + g) * T + t] = 0.f;
    }
    fbw::barrier();

    float *const acur = tile.arow + p.left4[0], *const vcur = tile.vrow + p.left4[0];
    for (int t = 0; t < Fmax; ++t) {
        float mt[G], early[kEarly > 0 ? kEarly : 1][G];
        if (kEarly > 0) {
#pragma unroll
            for (int g = 0; g < G; ++g) mt[g] = t < F[g] ? m[(size_t)(b0 + g) * T + t] : 0.f;
        }
#pragma unroll
        for (int g = 0; g < G; ++g)
#pragma unroll
            for (int it = 0; it < kEarly; ++it) {
                const int j = tid + it * kThreads;
                early[it][g] = (j < S && t < F[g]) ? obs[((size_t)(b0 + g) * T + t) * S + j] : 0.f;
            }
        float rc[G], logc[G], eb[G], gb[G], ep[G], acc[G];
        double vacc[G];
        if (t > 0) {
            band_phase(tile, p, Pf, Pg, S);
            fbw::barrier();
            float cprev[G], svprev[G];
            peb::frame_sums(tile, t - 1, cbuf, prefix, T, cprev, svprev);
#pragma unroll
            for (int g = 0; g < G; ++g) {
                // (after a zero-probability frame: every a_t is 0, or NaN from NaN, and the background brings nothing back)
                const bool dead = cprev[g] == 0.f;
                rc[g] = dead ? 0.f : 1.f / cprev[g];
                logc[g] = dead ? 0.f : logf(cprev[g]);
                eb[g] = dead ? 0.f : ebg;
                gb[g] = dead ? 0.f : gbg;
                ep[g] = ebg != 0.f ? eb[g] * fmaf(svprev[g], rc[g], logc[g]) : 0.f;    // ebg * prefix_{t-1}
            }
        }
        if (kEarly == 0) {
#pragma unroll
            for (int g = 0; g < G; ++g) mt[g] = t < F[g] ? m[(size_t)(b0 + g) * T + t] : 0.f;
        }
#pragma unroll
        for (int g = 0; g < G; ++g) {
            acc[g] = 0.f;
            vacc[g] = 0.;
        }
        // one state of every item of the tile; `ot`: its observations where they were asked for early
        auto state = [&](int j, const float *ot) __attribute__((always_inline)) {
#pragma unroll
            for (int g = 0; g < G; ++g) {
                if (t >= F[g]) continue;
                const float o = ot ? ot[g] : obs[((size_t)(b0 + g) * T + t) * S + j];
                float a, h = 0.f;
                if (t == 0) {
                    a = expf(initial[j] + o - mt[g]);
                } else {
                    const float *part = tile.slice + (size_t)g * 3 * S4 + j;
                    float sa = part[0], sv = part[S4], sg = part[2 * S4];
                    for (int k = 1; k < KS; ++k) {                       // the slices in their order
                        part += (size_t)G * 3 * S4;
                        sa += part[0];
                        sv += part[S4];
                        sg += part[2 * S4];
                    }
                    // d = E p, D2 = E u and D3 = G p of the normalised rows, each the band over c_{t-1} plus its constant
                    const float d = fmaf(sa, rc[g], eb[g]);
                    const float D2 = fmaf(fmaf(logc[g], sa, sv), rc[g], ep[g]);
                    const float D3 = fmaf(sg, rc[g], gb[g]);
                    a = expf(o - mt[g]) * d;
                    if (d > 0.f) h = logf(d) + (D2 - D3) / d;            // (0 where no path reaches j)
                }
                const float v = a * h - pe::xlogx(a);
                acur[g * stride + j] = a;
                vcur[g * stride + j] = v;
                acc[g] += a;
                vacc[g] += (double)v;
            }
        };
#pragma unroll
        for (int it = 0; it < kEarly; ++it)
            if (tid + it * kThreads < S) state(tid + it * kThreads, early[it]);
        for (int j = tid + kEarly * kThreads; j < S; j += kThreads) state(j, nullptr);
        float *pa = tile.asum + (size_t)(t & 1) * G * kWaves;
        double *pv = tile.vsum + (size_t)(t & 1) * G * kWaves;
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const float a = fbb::wave_sum(acc[g]);
            const double v = fbb::wave_sum(vacc[g]);
            if (lane == 0) {
                pa[g * kWaves + wave] = a;
                pv[g * kWaves + wave] = v;
            }
        }
        fbw::barrier();
    }
    {
        float c[G], sv[G];
        peb::frame_sums(tile, Fmax - 1, cbuf, prefix, T, c, sv);
    }
    fbw::barrier();                                                      // (c_t, prefix_t and Hs are read by others below)
    fbb::log_likelihood(tile, m, cbuf, flag, loglik, B, T);
    fbw::barrier();
    // an item whose L is not finite (or a broken promise: L is NaN then): a NaN entropy and NaN in its prefix entries t < F
#pragma unroll
    for (int g = 0; g < G; ++g) {
        if (b0 + g >= B) continue;
        const bool bad = !isfinite(tile.Ls[g]);
        if (tid == 0) entropy[b0 + g] = bad ? NAN : tile.Hs[g];
        if (!bad) continue;
        for (int t = tid; t < F[g]; t += kThreads) prefix[(size_t)(b0 + g) * T + t] = NAN;
    }
}

#undef PEW_KERNEL

}  // namespace pew
