// sample.hpp -- posterior path sampling: forward filtering, backward sampling on the HMM the decoder decodes
// (torbi_hip_sample / _uniform, torbi_amd/sampling.py, SAMPLING.md).
//
// The filter is the forward half of forward_backward.hpp: it leaves the unnormalised rows a_t [B][T][S] and E = exp(A)
// ([next][prev], row stride Sp) in the workspace.  One launch then draws every path, one wave per draw, from the last
// frame down:
//     t = F-1:  w[i] = a_{F-1}[i]             t < F-1:  w[i] = a_t[i] * E[j_{t+1}][i]
//     Z = sum w;  j_t = the smallest i with prefix(i) > u * Z and w[i] > 0, else the largest i with w[i] > 0
// Row a_{t-1} does not depend on the draw and is loaded a frame ahead; row j_{t+1} of E is the dependent load.
//
// The search is hierarchical and its summation tree depends on S alone.  A block is the 64 * PER consecutive states one
// load instruction of the wave covers (PER = 4 with float4 loads, lane l holds states 4 l .. 4 l + 3 of the block; PER = 1
// with scalar loads):
//     block totals   the lane sums (w0 + w1) + (w2 + w3), reduced over the wave on DPP (wave_reduce.hpp)
//     the block      in-order sums C_q of the totals; the first block with C_q > u Z and a total > 0 (wave-uniform scan)
//     the lane       inclusive wave prefix of the lane sums against the residual u Z - C_{q-1}, a ballot over lanes whose own
//                    sum is > 0
//     the state      the lane's values in order, behind the prefix of the lanes before it
// At every level a member of weight 0 is left out of the ballot explicitly, and where rounding leaves no member above the
// target the last member of weight > 0 is taken: a state of weight 0 is never returned.
//
// HELD form (S <= kHeldStates): the frame's weights stay in registers.  STREAMED form (up to fb::kMaxStates): block totals
// and their prefixes are kept one per lane, and the chosen block is read again.
// Vector stores only, no atomics, no LDS, nothing waits across workgroups.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include "forward_backward.hpp"
#include "wave_reduce.hpp"

namespace sample {

constexpr int kWaves = 4;                    // draws per workgroup of sample_backward_kernel
constexpr int kMaxDraws = 4096;
constexpr int kHeldStates = 4096;            // up to here a frame's weights stay in registers (float4 loads)
constexpr int kHeldStatesScalar = 2048;      // the same with scalar loads: 32 blocks of 64 states
constexpr int kUniformHeldStates = 2048;     // the same for a row of the uniform route
constexpr float kMaxUniform = 0x1.fffffep-1f;  // 1 - 2^-24

using fb::f32x4;

struct SumOp {
    __device__ __forceinline__ float operator()(float a, float b) const { return a + b; }
};

struct NanMaxOp {                            // NaN wins, as in the filter's row maxima
    __device__ __forceinline__ float operator()(float a, float b) const { return fb::nan_max(a, b); }
};

// u as the contract reads it: clamped to [0, 1 - 2^-24], NaN reads as 0 (fmaxf drops the NaN)
__device__ __forceinline__ float read_uniform(float u) { return fminf(fmaxf(u, 0.f), kMaxUniform); }

// the values of one block that a lane holds
template <bool VEC>
struct Lane {
    static constexpr int kPer = VEC ? 4 : 1;
    static constexpr int kBlock = 64 * kPer;
    float v[kPer];
    __device__ __forceinline__ float sum() const {
        if constexpr (VEC) return (v[0] + v[1]) + (v[2] + v[3]);
        else return v[0];
    }
};

// block q of a row of S floats (0 beyond S); VEC: S % 4 == 0 and the row is 16-byte aligned
template <bool VEC>
__device__ __forceinline__ Lane<VEC> load_block(const float *__restrict__ row, int q, int S, int lane, float fill = 0.f) {
    Lane<VEC> x;
    if constexpr (VEC) {
        const int j = 4 * (lane + 64 * q);
        const f32x4 v = j < S ? *reinterpret_cast<const f32x4 *>(row + j) : f32x4{fill, fill, fill, fill};
#pragma unroll
        for (int r = 0; r < 4; ++r) x.v[r] = v[r];
    } else {
        const int j = lane + 64 * q;
        x.v[0] = j < S ? row[j] : fill;
    }
    return x;
}

template <int N>
__device__ __forceinline__ float row_shr(float x) {      // lane l of a 16-lane row reads lane l - N of it, 0 before the row
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0x110 + N, 0xf, 0xf, true));
}

// inclusive prefix sum over the wave's lanes in a fixed tree: within 16-lane rows on DPP, then the rows before in order
__device__ __forceinline__ float wave_prefix(float x, int lane) {
    x += row_shr<1>(x);
    x += row_shr<2>(x);
    x += row_shr<4>(x);
    x += row_shr<8>(x);
    const int xi = __builtin_bit_cast(int, x);
    const float r0 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(xi, 15));
    const float r1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(xi, 31));
    const float r2 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(xi, 47));
    const int row = lane >> 4;
    const float before = row == 0 ? 0.f : row == 1 ? r0 : row == 2 ? r0 + r1 : (r0 + r1) + r2;
    return row == 0 ? x : before + x;
}

__device__ __forceinline__ float read_lane(float x, int l) {    // l wave-uniform
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x), l));
}

// The state of one block (as an offset into it) for the residual target `resid`, or -1 when the block has no weight > 0.
// resid = +inf takes the block's last state of weight > 0.
template <bool VEC>
__device__ __forceinline__ int pick_in_block(const Lane<VEC> &w, float resid, int lane) {
    const float s = w.sum();
    const float incl = wave_prefix(s, lane);
    const unsigned long long some = __ballot(s > 0.f);
    if (some == 0) return -1;
    const unsigned long long over = __ballot(s > 0.f && incl > resid);
    const int l = __builtin_amdgcn_readfirstlane(over ? __builtin_ctzll(over) : 63 - __builtin_clzll(some));
    if constexpr (!VEC) {
        return l;
    } else {
        float p = l == 0 ? 0.f : read_lane(incl, l - 1);
        int pick = -1, last = -1;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float x = read_lane(w.v[r], l);
            p += x;
            if (x > 0.f) {
                last = r;
                if (pick < 0 && over && p > resid) pick = r;
            }
        }
        return 4 * l + (pick < 0 ? last : pick);
    }
}

// ---- HELD form: NB blocks of weights in registers, their totals wave-uniform ----
template <bool VEC, int NB>
struct Held {
    Lane<VEC> w[NB];
    float tot[NB];
    float Z;

    __device__ __forceinline__ void total(int S) {
        float z = 0.f;
#pragma unroll
        for (int q = 0; q < NB; ++q) {
            tot[q] = q * Lane<VEC>::kBlock < S ? wavered::wave_reduce_f32(w[q].sum(), SumOp()) : 0.f;
            z += tot[q];
        }
        Z = z;
    }

    // the state for uniform u (already read through read_uniform); Z > 0 and finite
    __device__ __forceinline__ int pick(float u, int lane) const {
        const float target = u * Z;
        // (the chosen block's values are copied where the scan decides, never indexed by the block number: the blocks stay
        // in registers)
        int qs = -1, qlast = -1;
        float c = 0.f, resid = INFINITY;
        Lane<VEC> chosen = w[0], last = w[0];
#pragma unroll
        for (int q = 0; q < NB; ++q) {
            const float next = c + tot[q];
            const bool some = tot[q] > 0.f, take = some && qs < 0 && next > target;
            if (some) qlast = q;
            if (take) {
                qs = q;
                resid = target - c;
            }
#pragma unroll
            for (int r = 0; r < Lane<VEC>::kPer; ++r) {
                last.v[r] = some ? w[q].v[r] : last.v[r];
                chosen.v[r] = take ? w[q].v[r] : chosen.v[r];
            }
            c = next;
        }
        if (qlast < 0) return -1;
        if (qs < 0) {
            qs = qlast;
            chosen = last;
        }
        const int off = pick_in_block<VEC>(chosen, resid, lane);
        return off < 0 ? -1 : qs * Lane<VEC>::kBlock + off;
    }
};

// ---- STREAMED form: block q's total and the sum of the totals before it live in lane q & 63 of register q >> 6 ----
constexpr int kStreamRegs = fb::kMaxStates / (64 * 64);      // 4: up to 256 blocks of 64 states
struct Streamed {
    float before[kStreamRegs], tot[kStreamRegs];
    float Z;

    template <bool VEC, class W>
    __device__ __forceinline__ void total(W &&weights, int S, int lane) {
        const int blocks = (S + Lane<VEC>::kBlock - 1) / Lane<VEC>::kBlock;
        float c = 0.f;
#pragma unroll
        for (int g = 0; g < kStreamRegs; ++g) {
            before[g] = 0.f;
            tot[g] = 0.f;
            for (int q0 = 0; q0 < 64 && 64 * g + q0 < blocks; ++q0) {
                const Lane<VEC> w = weights(64 * g + q0);
                const float t = wavered::wave_reduce_f32(w.sum(), SumOp());
                if (lane == q0) {
                    before[g] = c;
                    tot[g] = t;
                }
                c += t;
            }
        }
        Z = c;
    }

    template <bool VEC, class W>
    __device__ __forceinline__ int pick(W &&weights, float u, int lane) const {
        return pick_target<VEC>(weights, u * Z, lane);
    }

    // the same search against a target the caller formed (sample_band.hpp: the residual behind the band part)
    template <bool VEC, class W>
    __device__ __forceinline__ int pick_target(W &&weights, float target, int lane) const {
        int qs = -1;
        float resid = INFINITY;
#pragma unroll
        for (int g = 0; g < kStreamRegs; ++g) {
            const unsigned long long over = __ballot(tot[g] > 0.f && before[g] + tot[g] > target);
            if (qs < 0 && over) {
                const int l = __builtin_ctzll(over);
                qs = 64 * g + l;
                resid = target - read_lane(before[g], l);
            }
        }
        if (qs < 0) {
#pragma unroll
            for (int g = kStreamRegs - 1; g >= 0; --g) {
                const unsigned long long some = __ballot(tot[g] > 0.f);
                if (qs < 0 && some) qs = 64 * g + 63 - __builtin_clzll(some);
            }
        }
        if (qs < 0) return -1;
        qs = __builtin_amdgcn_readfirstlane(qs);
        const int off = pick_in_block<VEC>(weights(qs), resid, lane);
        return off < 0 ? -1 : qs * Lane<VEC>::kBlock + off;
    }
};

// One wave's 64 most recent indices, lane t & 63 holds frame t; written out as whole runs
struct IndexRun {
    int32_t keep;
    __device__ __forceinline__ void put(int32_t *__restrict__ out, int t, int j, int F, int lane) {
        if (lane == (t & 63)) keep = j;
        if ((t & 63) == 0 && t + lane < F) out[t + lane] = keep;
    }
};

__device__ __forceinline__ void fill_row(int32_t *__restrict__ out, int from, int T, int value, int lane) {
    for (int t = from + lane; t < T; t += 64) out[t] = value;
}

// ---- backward sampling, every frame in one launch: one wave per draw, grid (B, ceil(N / kWaves)) ----
// NB > 0: the HELD form with NB blocks; NB == 0: the STREAMED form.
template <bool VEC, int NB>
__global__ __launch_bounds__(64 * kWaves) void sample_backward_kernel(const float *__restrict__ filter, const float *__restrict__ E,
                                                                      const int32_t *__restrict__ frames,
                                                                      const float *__restrict__ loglik,
                                                                      const float *__restrict__ uniforms,
                                                                      int32_t *__restrict__ indices, int T, int S, int N) {
    const int b = blockIdx.x, n = blockIdx.y * kWaves + threadIdx.x / 64, lane = threadIdx.x & 63;
    if (n >= N) return;
    const float L = loglik[b];
    const int F = fb::frames_of(frames, b, T);
    const size_t draw = (size_t)b * N + n;
    int32_t *const out = indices + draw * T;
    const float *const us = uniforms + draw * T;
    if (!isfinite(L)) {
        fill_row(out, 0, T, -1, lane);
        return;
    }
    const int Sp = fb::padded_states(S);
    const float *const rows = filter + (size_t)b * T * S;
    IndexRun run;
    run.keep = -1;
    bool bad = false;
    int j = 0;
    if constexpr (NB > 0) {
        Lane<VEC> a[NB];
#pragma unroll
        for (int q = 0; q < NB; ++q) a[q] = load_block<VEC>(rows + (size_t)(F - 1) * S, q, S, lane);
        for (int t = F - 1; t >= 0; --t) {
            Held<VEC, NB> h;
            const float *const e = E + (size_t)j * Sp;
#pragma unroll
            for (int q = 0; q < NB; ++q) {
                if (t < F - 1) h.w[q] = load_block<VEC>(e, q, S, lane);
                else
#pragma unroll
                    for (int r = 0; r < Lane<VEC>::kPer; ++r) h.w[q].v[r] = 1.f;
            }
            const float u = read_uniform(us[t]);
            Lane<VEC> ahead[NB];
            if (t > 0) {
#pragma unroll
                for (int q = 0; q < NB; ++q) ahead[q] = load_block<VEC>(rows + (size_t)(t - 1) * S, q, S, lane);
            }
#pragma unroll
            for (int q = 0; q < NB; ++q) {
#pragma unroll
                for (int r = 0; r < Lane<VEC>::kPer; ++r) h.w[q].v[r] = a[q].v[r] * h.w[q].v[r];
            }
            h.total(S);
            if (!(h.Z > 0.f) || !isfinite(h.Z)) {
                bad = true;
                break;
            }
            j = __builtin_amdgcn_readfirstlane(h.pick(u, lane));
            if (j < 0) {                         // (Z > 0 leaves a weight > 0; kept so that no row of E is ever read at -1)
                bad = true;
                break;
            }
            if (t == F - 1) fill_row(out, F, T, j, lane);
            run.put(out, t, j, F, lane);
            if (t > 0) {
#pragma unroll
                for (int q = 0; q < NB; ++q) a[q] = ahead[q];
            }
        }
    } else {
        for (int t = F - 1; t >= 0; --t) {
            const float *const arow = rows + (size_t)t * S;
            const float *const erow = E + (size_t)j * Sp;
            const bool last = t == F - 1;
            auto weights = [&](int q) {
                Lane<VEC> w = load_block<VEC>(arow, q, S, lane);
                if (!last) {
                    const Lane<VEC> e = load_block<VEC>(erow, q, S, lane);
#pragma unroll
                    for (int r = 0; r < Lane<VEC>::kPer; ++r) w.v[r] *= e.v[r];
                }
                return w;
            };
            const float u = read_uniform(us[t]);
            Streamed s;
            s.total<VEC>(weights, S, lane);
            if (!(s.Z > 0.f) || !isfinite(s.Z)) {
                bad = true;
                break;
            }
            j = __builtin_amdgcn_readfirstlane(s.pick<VEC>(weights, u, lane));
            if (j < 0) {
                bad = true;
                break;
            }
            if (last) fill_row(out, F, T, j, lane);
            run.put(out, t, j, F, lane);
        }
    }
    if (bad) fill_row(out, 0, T, -1, lane);
}

// ---- uniform transition: frames are independent, j_0 ~ softmax(pi + o_0), j_t ~ softmax(o_t) ----
// One wave per row (b, t): one read of the row serves all N draws.  lse[b][t] = m + log(sum exp(x - m)) in fp64 (what
// fb_uniform_loglik_kernel sums); the wave of row F_b - 1 also writes columns t >= F_b.  Rows t >= F_b are not read.
template <bool VEC>
__global__ __launch_bounds__(256) void sample_uniform_rows_kernel(const float *__restrict__ obs, const int32_t *__restrict__ frames,
                                                                  const float *__restrict__ initial,
                                                                  const float *__restrict__ uniforms,
                                                                  int32_t *__restrict__ indices, double *__restrict__ lse, int B,
                                                                  int T, int S, int N) {
    constexpr int NB = kUniformHeldStates / Lane<VEC>::kBlock;
    const size_t rowi = (size_t)blockIdx.x * (blockDim.x / 64) + threadIdx.x / 64;
    const int lane = threadIdx.x & 63;
    if (rowi >= (size_t)B * T) return;
    const int b = (int)(rowi / T), t = (int)(rowi % T);
    const int F = fb::frames_of(frames, b, T);
    if (t >= F) return;
    const float *const o = obs + rowi * S;
    const bool first = t == 0, tail = t == F - 1;
    auto scores = [&](int q) {
        Lane<VEC> x = load_block<VEC>(o, q, S, lane, -INFINITY);
        if (first) {
            const Lane<VEC> p = load_block<VEC>(initial, q, S, lane, 0.f);
#pragma unroll
            for (int r = 0; r < Lane<VEC>::kPer; ++r) x.v[r] += p.v[r];
        }
        return x;
    };
    auto store = [&](int n, int j) {
        int32_t *const out = indices + ((size_t)b * N + n) * T;
        if (lane == 0) out[t] = j;
        if (tail) fill_row(out, F, T, j, lane);
    };
    const float *const us = uniforms + (size_t)b * N * T + t;
    if (S <= kUniformHeldStates) {
        Held<VEC, NB> h;
        float mx = -INFINITY;
#pragma unroll
        for (int q = 0; q < NB; ++q) {
            h.w[q] = scores(q);
#pragma unroll
            for (int r = 0; r < Lane<VEC>::kPer; ++r) mx = fb::nan_max(mx, h.w[q].v[r]);
        }
        mx = wavered::wave_reduce_f32(mx, NanMaxOp());
        const float mu = mx == -INFINITY ? 0.f : mx;
#pragma unroll
        for (int q = 0; q < NB; ++q) {
#pragma unroll
            for (int r = 0; r < Lane<VEC>::kPer; ++r) h.w[q].v[r] = expf(h.w[q].v[r] - mu);
        }
        h.total(S);
        if (lane == 0) lse[rowi] = (double)mu + log((double)h.Z);
        const bool ok = h.Z > 0.f && isfinite(h.Z);
        for (int n = 0; n < N; ++n) store(n, ok ? h.pick(read_uniform(us[(size_t)n * T]), lane) : -1);
        return;
    }
    // longer rows: the maximum, the block totals, and per draw the chosen block again (from L1 / L2)
    const int blocks = (S + Lane<VEC>::kBlock - 1) / Lane<VEC>::kBlock;
    float mx = -INFINITY;
    for (int q = 0; q < blocks; ++q) {
        const Lane<VEC> x = scores(q);
#pragma unroll
        for (int r = 0; r < Lane<VEC>::kPer; ++r) mx = fb::nan_max(mx, x.v[r]);
    }
    mx = wavered::wave_reduce_f32(mx, NanMaxOp());
    const float mu = mx == -INFINITY ? 0.f : mx;
    auto weights = [&](int q) {
        Lane<VEC> x = scores(q);
#pragma unroll
        for (int r = 0; r < Lane<VEC>::kPer; ++r) x.v[r] = expf(x.v[r] - mu);
        return x;
    };
    Streamed s;
    s.total<VEC>(weights, S, lane);
    if (lane == 0) lse[rowi] = (double)mu + log((double)s.Z);
    const bool ok = s.Z > 0.f && isfinite(s.Z);
    for (int n = 0; n < N; ++n) store(n, ok ? s.pick<VEC>(weights, read_uniform(us[(size_t)n * T]), lane) : -1);
}

// every column of every draw of an item whose L is not finite is -1; one workgroup per item
__global__ void sample_mask_kernel(const float *__restrict__ loglik, int32_t *__restrict__ indices, size_t per_item) {
    const int b = blockIdx.x;
    if (isfinite(loglik[b])) return;
    for (size_t e = threadIdx.x; e < per_item; e += blockDim.x) indices[(size_t)b * per_item + e] = -1;
}

}  // namespace sample
