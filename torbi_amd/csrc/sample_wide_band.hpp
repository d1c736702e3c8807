// sample_wide_band.hpp -- posterior path sampling for a transition matrix that holds ONE value outside a band of up to 512
// entries (torbi_hip_sample_wide_band, torbi_amd/sampling.py forward_sample_wide_banded, SAMPLING.md "Wide band route").
//
// The draw rule is sample_band.hpp's, word for word: frame F-1 draws from the whole row a_{F-1}; frame t < F-1 with
// j = j_{t+1}, lo = max(0, j - reach_left), hi = min(S-1, j + reach_right) draws from the concatenated weights
//     [ v[lo] .. v[hi] ,  ebg * a_t[0] .. ebg * a_t[S-1] ]          v[i] = a_t[i] * max(expf(A[j][i]) - ebg, 0)
// with Z = Zband + ebg * c_t.  New is the arithmetic on both sides.
//
// fb_wide_band_filter_kernel<G> is the forward half of fb_wide_band_kernel<G>: the same pack, tile and wide_forward, then
// fbb::log_likelihood, so a_t, c_t and L have that kernel's bits.  It writes a_t to filter rows of S4 floats (S up to 4), so
// that every 4-aligned piece of a row is one aligned 16-byte load whatever S is; the padding of a row is never written and
// never used, and rows t >= F_b are neither.
//
// sample_wide_band_backward_kernel<NP, VEC>: one wave per draw, sample::kWaves waves per workgroup.  Where the narrow sampler
// holds one slot per lane, this one holds the window as 4-state pieces: with lo4 = lo down to 4, piece 64 r + lane of round
// r < NP covers states lo4 + 4 (64 r + lane) .. + 3, a round 256 states.  NP = 1 takes W + 3 <= 256, NP = 2 up to 512, NP = 3
// the rest.  Per frame a lane issues NP 16-byte loads of a_t and NP loads of A[j][..] from the caller's matrix, whose rows are
// contiguous in i (16-byte loads with VEC: S % 4 == 0 and A 16-byte aligned; four scalars otherwise), all as soon as j is
// known; u and c_t are loaded a frame ahead.  States outside [lo, hi] get weight 0 by selection, not by a product.
//
// Zband and the search run in one fixed tree over slots ascending: a lane's four states in order, sample::wave_prefix over
// the lanes of a round, the rounds in order.  The search finds the round (wave-uniform), a ballot finds the lane, then the
// state within the lane; a member of weight 0 is left out at every level, and "the last slot of weight > 0" follows the same
// order in reverse.  The whole-row part -- frame F-1, and u Z >= Zband with ebg != 0 -- is sample::Streamed on the padded row.
// No LDS, no atomics, vector stores only, nothing waits across workgroups.
#pragma once

#include "forward_backward_wide_band.hpp"
#include "sample.hpp"

namespace fbw {

#if defined(__HIP_DEVICE_COMPILE__)
#define FBW_KERNEL __global__ __attribute__((target("no-packed-fp32-ops")))
#else
#define FBW_KERNEL __global__
#endif

struct SampleLayout : Layout {
    float *rows;                             // a_t [B][T][S4] fp32
};

// the wide route's workspace, then the filter rows
inline SampleLayout sample_layout(char *base, int B, int T, int S, int reach_left, int reach_right) {
    SampleLayout l;
    static_cast<Layout &>(l) = layout(base, B, T, S, reach_left, reach_right);
    Scratch a(base, l.total - 256);
    l.rows = a.take<float>((size_t)B * T * l.S4);
    l.total = a.bytes + 256;                 // (room to align the caller's base)
    return l;
}

// rounds of 256 states that hold the window from lo4 on: W + 3 states at the most
inline int sample_rounds(const Plan &p) { return (p.W + 3 + kBlockStates - 1) / kBlockStates; }

// ---- the forward pass of G items per workgroup; grid ceil(B / G), dynamic LDS lds_bytes(G, plan) ----
template <int G>
FBW_KERNEL __launch_bounds__(kThreads) void fb_wide_band_filter_kernel(
    const float *__restrict__ obs, const int32_t *__restrict__ frames, const float *__restrict__ initial,
    const float *__restrict__ Pf, const float *__restrict__ m, float *__restrict__ cbuf, const int32_t *__restrict__ flag,
    float *__restrict__ filter, float *__restrict__ loglik, float ebg, Plan p, int B, int T, int S) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    Tile<G> tile(lds_raw, p, S);
    tile_begin(tile, frames, B, T);
    barrier();
    wide_forward(tile, obs, initial, Pf, m, cbuf, filter, p.S4, ebg, p, T, S);
    fbb::log_likelihood(tile, m, cbuf, flag, loglik, B, T);
}

// 256 states of a padded filter row (stride S4, so the load is aligned), scaled; 0 from S on
__device__ __forceinline__ sample::Lane<true> padded_block(const float *__restrict__ row, int q, int S, int lane, float scale) {
    sample::Lane<true> x;
    const int j = 4 * (lane + 64 * q);
    const f4 v = j < S ? *reinterpret_cast<const f4 *>(row + j) : f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int n = 0; n < 4; ++n) x.v[n] = j + n < S ? v[n] * scale : 0.f;
    return x;
}

// One round of the window in a lane: its four weights, their sum in order and the inclusive prefix of the sums over the wave
struct Round {
    float v[4], s, incl;
};

// The slot of one round (4 lane + n) for the residual target `resid`, or -1 when the round has no weight > 0.  resid = +inf
// takes the round's last slot of weight > 0.
__device__ __forceinline__ int pick_in_round(const Round &w, float resid, int lane) {
    const unsigned long long some = __ballot(w.s > 0.f);
    if (some == 0) return -1;
    const unsigned long long over = __ballot(w.s > 0.f && w.incl > resid);
    const int l = __builtin_amdgcn_readfirstlane(over ? __builtin_ctzll(over) : 63 - __builtin_clzll(some));
    float p = l == 0 ? 0.f : sample::read_lane(w.incl, l - 1);
    int pick = -1, last = -1;
#pragma unroll
    for (int n = 0; n < 4; ++n) {
        const float x = sample::read_lane(w.v[n], l);
        p += x;
        if (x > 0.f) {
            last = n;
            if (pick < 0 && over && p > resid) pick = n;
        }
    }
    return 4 * l + (pick < 0 ? last : pick);
}

// The slot of the band part (256 r + 4 lane + n) for `target`, or -1 when no slot has weight > 0; tot[r] is round r's total.
// target = +inf takes the last slot of weight > 0.  The chosen round is copied where the scan decides, never indexed.
template <int NP>
__device__ __forceinline__ int pick_in_band(const Round (&w)[NP], const float (&tot)[NP], float target, int lane) {
    int rs = -1, rlast = -1;
    float c = 0.f, resid = INFINITY;
    Round chosen = w[0], last = w[0];
#pragma unroll
    for (int r = 0; r < NP; ++r) {
        const float next = c + tot[r];
        const bool some = tot[r] > 0.f, take = some && rs < 0 && next > target;
        if (some) {
            rlast = r;
            last = w[r];
        }
        if (take) {
            rs = r;
            resid = target - c;
            chosen = w[r];
        }
        c = next;
    }
    if (rlast < 0) return -1;
    if (rs < 0) {
        rs = rlast;
        chosen = last;
    }
    const int off = pick_in_round(chosen, resid, lane);
    return off < 0 ? -1 : kBlockStates * rs + off;
}

// ---- backward sampling on the wide band, every frame in one launch: one wave per draw, grid (B, ceil(N / sample::kWaves)) ----
// `filter`: rows of S4 floats.  A is the caller's matrix [next][prev] (row stride S).
template <int NP, bool VEC>
FBW_KERNEL __launch_bounds__(64 * sample::kWaves) void sample_wide_band_backward_kernel(
    const float *__restrict__ filter, const float *__restrict__ A, const float *__restrict__ cbuf,
    const int32_t *__restrict__ frames, const float *__restrict__ loglik, const float *__restrict__ uniforms,
    int32_t *__restrict__ indices, float ebg, int reach_left, int reach_right, int T, int S, int N) {
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
    const float *const cs = cbuf + (size_t)b * T;
    sample::IndexRun run;
    run.keep = -1;
    bool bad = false;
    int j;
    {   // frame F-1: the whole row a_{F-1}
        const float *const arow = rows + (size_t)(F - 1) * S4;
        auto weights = [&](int q) __attribute__((always_inline)) { return padded_block(arow, q, S, lane, 1.f); };
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
    // (u and c_t do not depend on the draw so far: they are loaded a frame ahead of the loads that do)
    float unext = 0.f, cnext = 0.f;
    if (F > 1) {
        unext = us[F - 2];
        if (ebg != 0.f) cnext = cs[F - 2];
    }
    for (int t = F - 2; t >= 0 && !bad; --t) {
        const int lo = j - reach_left < 0 ? 0 : j - reach_left, hi = j + reach_right > S - 1 ? S - 1 : j + reach_right;
        const int lo4 = lo & ~3;
        const float *const arow = rows + (size_t)t * S4;
        const float *const jrow = A + (size_t)j * S;
        f4 at[NP], aj[NP];
#pragma unroll
        for (int r = 0; r < NP; ++r) {
            const int i = lo4 + 4 * (64 * r + lane);                     // (i <= hi < S: the piece ends before S4, and before S with VEC)
            at[r] = i <= hi ? *reinterpret_cast<const f4 *>(arow + i) : f4{0.f, 0.f, 0.f, 0.f};
            if constexpr (VEC) {
                aj[r] = i <= hi ? *reinterpret_cast<const f4 *>(jrow + i) : f4{0.f, 0.f, 0.f, 0.f};
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) aj[r][k] = i + k >= lo && i + k <= hi ? jrow[i + k] : 0.f;
            }
        }
        const float u = sample::read_uniform(unext), ct = cnext;
        if (t > 0) {
            unext = us[t - 1];
            if (ebg != 0.f) cnext = cs[t - 1];
        }
        Round w[NP];
        float tot[NP], Zband = 0.f;
#pragma unroll
        for (int r = 0; r < NP; ++r) {
            const int i = lo4 + 4 * (64 * r + lane);
            float s = 0.f;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const bool in = i + k >= lo && i + k <= hi;
                w[r].v[k] = in ? at[r][k] * fmaxf(expf(aj[r][k]) - ebg, 0.f) : 0.f;
                s += w[r].v[k];
            }
            w[r].s = s;
            w[r].incl = sample::wave_prefix(s, lane);
            tot[r] = sample::read_lane(w[r].incl, 63);
            Zband += tot[r];
        }
        const float Z = ebg != 0.f ? Zband + ebg * ct : Zband;
        if (!(Z > 0.f) || !isfinite(Z)) {
            bad = true;
            break;
        }
        const float target = u * Z;
        int next = -1;
        if (target < Zband) {
            const int k = pick_in_band<NP>(w, tot, target, lane);
            next = k < 0 ? -1 : lo4 + k;
        } else if (ebg != 0.f) {
            // behind the band part: the constant over the whole row, against the residual
            auto weights = [&](int q) __attribute__((always_inline)) { return padded_block(arow, q, S, lane, ebg); };
            sample::Streamed s;
            s.total<true>(weights, S, lane);
            next = s.pick_target<true>(weights, target - Zband, lane);
        }
        if (next < 0) {                                                  // the band's last slot of weight > 0
            const int k = pick_in_band<NP>(w, tot, INFINITY, lane);
            next = k < 0 ? -1 : lo4 + k;
        }
        j = __builtin_amdgcn_readfirstlane(next);
        if (j < 0) {
            bad = true;
            break;
        }
        run.put(out, t, j, F, lane);
    }
    if (bad) sample::fill_row(out, 0, T, -1, lane);
}

#undef FBW_KERNEL

}  // namespace fbw
