// sample_band.hpp -- posterior path sampling for a transition matrix that holds ONE value outside a band
// (torbi_hip_sample_band, torbi_amd/sampling.py forward_sample_banded, SAMPLING.md "Band route").
//
// The model, a_t, c_t, m_t and E = exp(A) are forward_backward_band.hpp's, the reading of the uniforms and the draw rule
// sample.hpp's.  The caller states a band j - reach_left <= i <= j + reach_right of A [next j][prev i] and a `background`;
// ebg = exp(background) (0 for -inf).  Frame F-1 draws from the whole row a_{F-1}.  Frame t < F-1 with j = j_{t+1},
// lo = max(0, j - reach_left), hi = min(S-1, j + reach_right) draws from the concatenated weights
//     [ v[lo] .. v[hi] ,  ebg * a_t[0] .. ebg * a_t[S-1] ]          v[i] = a_t[i] * max(E[j][i] - ebg, 0)
// -- the band minus the constant, then the constant over everything: the mixture the band split of the filter uses --, and
// j_t is the state of the chosen slot.  Z = Zband + ebg * c_t with c_t as the filter stored it.
//
// fb_band_filter_kernel<G> is the forward half of fb_band_kernel<G>, the same functions: it leaves a_t in the filter rows
// [B][T][S] and c_t in cbuf.  sample_band_backward_kernel<VEC> then draws every path, one wave per draw: lane k owns in-band
// slot lo + k (at most 64 of them), so a frame costs one load of a_t[lo .. hi] and one of A[j][lo .. hi], both issued as soon
// as j is known.  The whole row is read only at frame F-1 and where u Z falls behind the band part (ebg != 0), with
// sample.hpp's streamed search.  Vector stores only, no atomics, no LDS in the sampler, nothing waits across workgroups.
#pragma once

#include "forward_backward_band.hpp"
#include "sample.hpp"

namespace fbb {

struct SampleLayout : Layout {
    float *rows;                             // a_t [B][T][S] fp32
};

// the band route's workspace, then the filter rows
inline SampleLayout sample_layout(char *base, int B, int T, int S, int reach_left, int reach_right) {
    SampleLayout l;
    static_cast<Layout &>(l) = layout(base, B, T, S, reach_left, reach_right);
    Scratch a(base, l.total - 256);
    l.rows = a.take<float>((size_t)B * T * S);
    l.total = a.bytes + 256;                 // (room to align the caller's base)
    return l;
}

// ---- the forward pass of G items per workgroup; grid ceil(B / G), dynamic LDS lds_bytes(G, S, halo) ----
template <int G>
__global__ __launch_bounds__(kThreads) void fb_band_filter_kernel(const float *__restrict__ obs, const int32_t *__restrict__ frames,
                                                                  const float *__restrict__ initial, const float *__restrict__ Df,
                                                                  const float *__restrict__ m, float *__restrict__ cbuf,
                                                                  const int32_t *__restrict__ flag, float *__restrict__ filter,
                                                                  float *__restrict__ loglik, float ebg, int reach_left,
                                                                  int reach_right, int W, int Sd, int B, int T, int S) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    Tile<G> tile(lds_raw, reach_left, reach_right, S);
    tile_begin(tile, frames, blockIdx.x * G, B, T);
    __syncthreads();
    forward_pass(tile, obs, initial, Df, m, cbuf, filter, ebg, reach_left, W, Sd, T, S);
    log_likelihood(tile, m, cbuf, flag, loglik, B, T);
}

// ---- backward sampling on the band, every frame in one launch: one wave per draw, grid (B, ceil(N / sample::kWaves)) ----
// A is the caller's matrix [next][prev] (row stride S): row j's in-band entries A[j][lo .. hi] are contiguous, one or two
// cache lines, where diagonal storage would spread them over W lines; expf(.) - ebg gives the bits of Df.
template <bool VEC>
__global__ __launch_bounds__(64 * sample::kWaves) void sample_band_backward_kernel(
    const float *__restrict__ filter, const float *__restrict__ A, const float *__restrict__ cbuf,
    const int32_t *__restrict__ frames, const float *__restrict__ loglik, const float *__restrict__ uniforms,
    int32_t *__restrict__ indices, float ebg, int reach_left, int reach_right, int T, int S, int N) {
    using sample::Lane;
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
    const float *const rows = filter + (size_t)b * T * S;
    const float *const cs = cbuf + (size_t)b * T;
    sample::IndexRun run;
    run.keep = -1;
    bool bad = false;
    int j;
    {   // frame F-1: the whole row a_{F-1}
        const float *const arow = rows + (size_t)(F - 1) * S;
        auto weights = [&](int q) { return sample::load_block<VEC>(arow, q, S, lane); };
        const float u = sample::read_uniform(us[F - 1]);
        sample::Streamed s;
        s.total<VEC>(weights, S, lane);
        j = -1;
        if (s.Z > 0.f && isfinite(s.Z)) j = __builtin_amdgcn_readfirstlane(s.pick<VEC>(weights, u, lane));
        bad = j < 0;
        if (!bad) {
            sample::fill_row(out, F, T, j, lane);
            run.put(out, F - 1, j, F, lane);
        }
    }
    // (u and c_t do not depend on the draw so far: they are loaded a frame ahead of the two loads that do)
    float unext = 0.f, cnext = 0.f;
    if (F > 1) {
        unext = us[F - 2];
        if (ebg != 0.f) cnext = cs[F - 2];
    }
    for (int t = F - 2; t >= 0 && !bad; --t) {
        const int lo = j - reach_left < 0 ? 0 : j - reach_left, hi = j + reach_right > S - 1 ? S - 1 : j + reach_right;
        const int i = lo + lane;
        const bool mine = i <= hi;
        const float *const arow = rows + (size_t)t * S;
        const float at = mine ? arow[i] : 0.f;
        const float aji = mine ? A[(size_t)j * S + i] : -INFINITY;
        const float u = sample::read_uniform(unext), ct = cnext;
        if (t > 0) {
            unext = us[t - 1];
            if (ebg != 0.f) cnext = cs[t - 1];
        }
        const float v = mine ? at * fmaxf(expf(aji) - ebg, 0.f) : 0.f;
        const float Zband = wavered::wave_reduce_f32(v, sample::SumOp());
        const float Z = ebg != 0.f ? Zband + ebg * ct : Zband;
        if (!(Z > 0.f) || !isfinite(Z)) {
            bad = true;
            break;
        }
        const float target = u * Z;
        const float incl = sample::wave_prefix(v, lane);
        const unsigned long long some = __ballot(v > 0.f);
        int k = some ? 63 - __builtin_clzll(some) : -1;                  // the band's last slot of weight > 0
        int next = -1;
        if (target < Zband) {
            const unsigned long long over = __ballot(v > 0.f && incl > target);
            if (over) k = __builtin_ctzll(over);
        } else if (ebg != 0.f) {
            // behind the band part: the constant over the whole row, against the residual
            auto weights = [&](int q) {
                Lane<VEC> w = sample::load_block<VEC>(arow, q, S, lane);
#pragma unroll
                for (int r = 0; r < Lane<VEC>::kPer; ++r) w.v[r] *= ebg;
                return w;
            };
            sample::Streamed s;
            s.total<VEC>(weights, S, lane);
            next = s.pick_target<VEC>(weights, target - Zband, lane);
        }
        if (next < 0) next = k < 0 ? -1 : lo + k;
        j = __builtin_amdgcn_readfirstlane(next);
        if (j < 0) {
            bad = true;
            break;
        }
        run.put(out, t, j, F, lane);
    }
    if (bad) sample::fill_row(out, 0, T, -1, lane);
}

}  // namespace fbb
