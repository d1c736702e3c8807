// sample_log_band.hpp -- posterior path sampling in LOG SPACE for a transition matrix that is -inf outside a band of up to
// 512 entries (torbi_hip_sample_log_band, torbi_amd/sampling.py forward_sample_log_banded, SAMPLING.md "Log-space band
// route").
//
// Every other sampler draws from the scaled float32 filter a_t: a filtered row that spans more than float32's range has
// already flushed the states a later frame would have favoured, and the draws come from another distribution -- or, where a
// whole window underflows, are -1.  This one filters and draws on logarithms (natural logs in the contract, A [next][prev]):
//     la_t = the filtered row in logs, its maximum 0 (forward_backward_log_band.hpp)
//     t = F-1:   w[i] = exp(la_{F-1}[i])                                          over the whole row
//     t < F-1:   x[i] = A[j][i] + la_t[i],  m = max_i x[i],  w[i] = exp(x[i] - m)    j = j_{t+1}, i in [lo, hi] of j
//     j_t = the smallest slot with cumulative weight > u Z and weight > 0, else the last slot of weight > 0
// m is the maximum of THIS draw's window, so its largest weight is 1 wherever the window lies under the row's maximum: no
// window underflows, and Z >= 1.
//
// fb_log_band_filter_kernel<G> is the forward half of fbl::fb_log_band_kernel<G> as a kernel of its own: the same pack,
// verify, plan and tile, the same phase A / phase B and reductions through that header's device functions, operation for
// operation, so L has that kernel's bits.  It writes la_t (base 2) to filter rows of S4 floats (S up to 4), so that every
// 4-aligned piece of a row is one aligned 16-byte load whatever S is.  Rows t >= F_b are never written and never read; the
// padding of a row is never written and never weighted.
//
// sample_log_band_backward_kernel<NP, VEC>: one wave per draw, sample::kWaves waves per workgroup, no LDS; the window as
// 4-state pieces in NP rounds of 256 states, the geometry of fbw::sample_wide_band_backward_kernel (NP = 1 takes W + 3 <= 256,
// NP = 2 up to 512, NP = 3 the rest).  Per frame a lane issues NP 16-byte loads of la_t and NP loads of A[j][..] from the
// caller's matrix (16 bytes with VEC: S % 4 == 0 and A 16-byte aligned; four scalars otherwise), all as soon as j is known; u is
// loaded a frame ahead.  A lane forms x = fl(A[j][i] log2e) + la_t[i], the pack's own bits of the matrix, the wave takes m by
// a butterfly, and Zband, the prefix and the search run in fbw's fixed tree over slots ascending (fbw::Round, pick_in_round,
// pick_in_band).  Clipped slots and slots with x = -inf get weight 0 by selection.  Frame F-1 is sample::Streamed on the
// padded row.  No float atomics, vector stores only, nothing waits across workgroups; a draw's bits depend on its item and
// its own row of uniforms alone.
#pragma once

#include "forward_backward_log_band.hpp"
#include "sample_wide_band.hpp"

namespace fbls {

using fbw::f4;
using fbw::Plan;
using fbw::barrier;
using fbl::ex2;
using fbl::ref_of;

struct SampleLayout : fbl::Layout {
    float *rows;                             // la_t [B][T][S4] fp32, base 2
};

// the log posterior route's workspace, then the filter rows
inline SampleLayout sample_layout(char *base, int B, int T, int S, int reach_left, int reach_right) {
    SampleLayout l;
    static_cast<fbl::Layout &>(l) = fbl::layout(base, S, reach_left, reach_right);
    Scratch a(base, l.total - 256);
    l.rows = a.take<float>((size_t)B * T * l.S4);
    l.total = a.bytes + 256;                 // (room to align the caller's base)
    return l;
}

// ---- the forward pass of G items per workgroup; grid ceil(B / G), dynamic LDS fbl::lds_bytes(G, plan).  The background is
// -inf: fbl::product_of's band term alone ----
template <int G>
__global__ __launch_bounds__(fbl::kThreads) void fb_log_band_filter_kernel(
    const float *__restrict__ obs, const int32_t *__restrict__ frames, const float *__restrict__ initial,
    const float *__restrict__ Pf, const int32_t *__restrict__ flag, float *__restrict__ filter, float *__restrict__ loglik,
    Plan p, int B, int T, int S) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    fbl::Tile<G> tile(lds_raw, p);
    const int tid = threadIdx.x, stride = p.stride;
    const int b0 = tile.b0 = blockIdx.x * G;
    int Fmax = 1;
#pragma unroll
    for (int g = 0; g < G; ++g) {
        tile.F[g] = b0 + g < B ? fb::frames_of(frames, b0 + g, T) : 0;   // (0: an item beyond the batch never takes a step)
        Fmax = tile.F[g] > Fmax ? tile.F[g] : Fmax;
    }
    const int *F = tile.F;
    float *const rows = tile.rows;
    for (int e = tid; e < G * stride; e += fbl::kThreads) rows[e] = -INFINITY;   // (the halos stay -inf all pass long)
    if (tid < G) {
        tile.Msum[tid] = 0.;
        tile.Zlast[tid] = 0.f;
    }
    barrier();

    float *const cur = rows + p.left4[0];
    for (int t = 0; t < Fmax; ++t) {
        if (t > 0) {
            fbl::band_phase(tile, p, 0, Pf, S);
            barrier();
        }
        float top[G];
#pragma unroll
        for (int g = 0; g < G; ++g) top[g] = -INFINITY;
        for (int j = tid; j < S; j += fbl::kThreads)
#pragma unroll
            for (int g = 0; g < G; ++g) {
                if (t >= F[g]) continue;
                const float o = obs[((size_t)(b0 + g) * T + t) * S + j];
                const float x = t == 0 ? (initial[j] + o) * fbl::kLog2e : o * fbl::kLog2e + fbl::product_of(tile, p, g, j, false, 0.f);
                cur[g * stride + j] = x;
                top[g] = fb::nan_max(top[g], x);
            }
        fbl::to_waves<G, true>(tile, 0, top);
        barrier();
        fbl::from_waves<G, true>(tile, 0, top);
        float sum[G];
#pragma unroll
        for (int g = 0; g < G; ++g) {
            top[g] = ref_of(top[g]);
            if (tid == 0 && t < F[g]) tile.Msum[g] += (double)top[g];
            sum[g] = 0.f;
        }
        for (int j = tid; j < S; j += fbl::kThreads)
#pragma unroll
            for (int g = 0; g < G; ++g) {
                if (t >= F[g]) continue;
                const float la = cur[g * stride + j] - top[g];
                cur[g * stride + j] = la;
                filter[((size_t)(b0 + g) * T + t) * p.S4 + j] = la;
                sum[g] += ex2(la);
            }
        fbl::to_waves<G, false>(tile, 1, sum);
        barrier();
        fbl::from_waves<G, false>(tile, 1, sum);                         // (a butterfly: every lane takes part)
#pragma unroll
        for (int g = 0; g < G; ++g)
            if (tid == 0 && t == F[g] - 1) tile.Zlast[g] = sum[g];
    }

    // ---- L = ln 2 (sum M_t + log2 Z_{F-1}), fbl's; NaN when that is NaN or +inf, or the promise is broken ----
    if (tid == 0) {
        const bool broken = *flag != 0;
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const double L = (tile.Msum[g] + log2((double)tile.Zlast[g])) * fbl::kLn2D;
            if (b0 + g < B) loglik[b0 + g] = (L != L || L == (double)INFINITY || broken) ? NAN : (float)L;
        }
    }
}

// 256 states of a padded filter row (stride S4, so the load is aligned) as weights 2^la; 0 from S on
__device__ __forceinline__ sample::Lane<true> exp_block(const float *__restrict__ row, int q, int S, int lane) {
    sample::Lane<true> x;
    const int j = 4 * (lane + 64 * q);
    const f4 v = j < S ? *reinterpret_cast<const f4 *>(row + j) : f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int n = 0; n < 4; ++n) x.v[n] = j + n < S ? ex2(v[n]) : 0.f;
    return x;
}

// ---- backward sampling on logarithms, every frame in one launch: one wave per draw, grid (B, ceil(N / sample::kWaves)) ----
// `filter`: rows of S4 floats, base-2 logs.  A is the caller's matrix [next][prev] (row stride S), natural logs.
template <int NP, bool VEC>
__global__ __launch_bounds__(64 * sample::kWaves) void sample_log_band_backward_kernel(
    const float *__restrict__ filter, const float *__restrict__ A, const int32_t *__restrict__ frames,
    const float *__restrict__ loglik, const float *__restrict__ uniforms, int32_t *__restrict__ indices, int reach_left,
    int reach_right, int T, int S, int N) {
    const int b = blockIdx.x, n = blockIdx.y * sample::kWaves + threadIdx.x / 64, lane = threadIdx.x & 63;
    if (n >= N) return;
    const float L = loglik[b];
    const int F = fb::frames_of(frames, b, T);
    const size_t draw = (size_t)b * N + n;
    int32_t *const out = indices + draw * T;
    const float *const us = uniforms + draw * T;
    if (!isfinite(L)) {
        sample::fill_row(out, 0, T, -1, lane);
        return;
    }
    const int S4 = (S + 3) & ~3;
    const float *const rows = filter + (size_t)b * T * S4;
    sample::IndexRun run;
    run.keep = -1;
    bool bad = false;
    int j;
    {   // frame F-1: the whole row, weights 2^la_{F-1} (the row's maximum is 0: one weight is 1)
        const float *const arow = rows + (size_t)(F - 1) * S4;
        auto weights = [&](int q) __attribute__((always_inline)) { return exp_block(arow, q, S, lane); };
        const float u = sample::read_uniform(us[F - 1]);
        sample::Streamed s;
        s.total<true>(weights, S, lane);
        j = -1;
        if (s.Z > 0.f && isfinite(s.Z)) j = __builtin_amdgcn_readfirstlane(s.pick<true>(weights, u, lane));
        bad = j < 0;
        if (!bad) {
            sample::fill_row(out, F, T, j, lane);
            run.put(out, F - 1, j, F, lane);
        }
    }
    float unext = F > 1 ? us[F - 2] : 0.f;                               // (u does not depend on the draw so far: a frame ahead)
    for (int t = F - 2; t >= 0 && !bad; --t) {
        const int lo = j - reach_left < 0 ? 0 : j - reach_left, hi = j + reach_right > S - 1 ? S - 1 : j + reach_right;
        const int lo4 = lo & ~3;
        const float *const arow = rows + (size_t)t * S4;
        const float *const jrow = A + (size_t)j * S;
        f4 la[NP], aj[NP];
#pragma unroll
        for (int r = 0; r < NP; ++r) {
            const int i = lo4 + 4 * (64 * r + lane);                     // (i <= hi < S: the piece ends before S4, and before S with VEC)
            la[r] = i <= hi ? *reinterpret_cast<const f4 *>(arow + i) : f4{0.f, 0.f, 0.f, 0.f};
            if constexpr (VEC) {
                aj[r] = i <= hi ? *reinterpret_cast<const f4 *>(jrow + i) : f4{0.f, 0.f, 0.f, 0.f};
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) aj[r][k] = i + k >= lo && i + k <= hi ? jrow[i + k] : 0.f;
            }
        }
        const float u = sample::read_uniform(unext);
        if (t > 0) unext = us[t - 1];
        // x in base 2 with the pack's rounding of the matrix; -inf where the slot is clipped
        float x[NP][4], top = -INFINITY;
#pragma unroll
        for (int r = 0; r < NP; ++r) {
            const int i = lo4 + 4 * (64 * r + lane);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const bool in = i + k >= lo && i + k <= hi;
                x[r][k] = in ? (float)((double)aj[r][k] * fbl::kLog2eD) + la[r][k] : -INFINITY;
                top = fb::nan_max(top, x[r][k]);
            }
        }
        const float m = wavered::wave_reduce_f32(top, sample::NanMaxOp());
        if (!(m < INFINITY)) {                                           // (a NaN or +inf in the window; L finite rules it out)
            bad = true;
            break;
        }
        const float ref = ref_of(m);
        fbw::Round w[NP];
        float tot[NP], Zband = 0.f;
#pragma unroll
        for (int r = 0; r < NP; ++r) {
            float s = 0.f;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                w[r].v[k] = x[r][k] != -INFINITY ? ex2(x[r][k] - ref) : 0.f;
                s += w[r].v[k];
            }
            w[r].s = s;
            w[r].incl = sample::wave_prefix(s, lane);
            tot[r] = sample::read_lane(w[r].incl, 63);
            Zband += tot[r];
        }
        if (!(Zband > 0.f) || !isfinite(Zband)) {
            bad = true;
            break;
        }
        // (where rounding leaves no slot above the target, pick_in_band takes the last slot of weight > 0)
        const int k = fbw::pick_in_band<NP>(w, tot, u * Zband, lane);
        j = __builtin_amdgcn_readfirstlane(k < 0 ? -1 : lo4 + k);
        if (j < 0) {                                                     // (Zband > 0 leaves a weight > 0; kept so no row is read at -1)
            bad = true;
            break;
        }
        run.put(out, t, j, F, lane);
    }
    if (bad) sample::fill_row(out, 0, T, -1, lane);
}

}  // namespace fbls
