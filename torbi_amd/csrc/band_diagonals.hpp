// band_diagonals.hpp -- the matrix side of the max-plus band routes (stream_band.hpp, k_best_band.hpp,
// max_marginals_band.hpp): the shapes and bands they take, the diagonals they read, and the one place where a caller's
// statement about their matrix -- every entry outside the band equals `background` bit for bit -- is believed or not.
// Nothing here knows about rows, scans or tiles.
//
// Per matrix (streaming) or per call (k-best, max-marginals), two launches in this order (`prepare`):
//     verdict_kernel   ok[0] = 1
//     prepare_kernel   diag[k][j] = A[j][j - reach_left + k], [W][S], W = reach_left + reach_right + 1, so that lanes over j
//                      read coalesced; ok[0] = 0 on a stray entry; alarm[0] = 1 on a NaN or +inf where the route has an alarm
// The sum-product family (forward_backward_band.hpp) prepares other diagonals and checks the same promise with
// stray_in_row.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

namespace banddiag {

// what viterbi.band_over can answer: S % 4 == 0 with kMinStates <= S <= kMaxStates, reach_left + reach_right + 4 <= kMaxWindow
constexpr int kMinStates = 64, kMaxStates = 3072;
constexpr int kMaxWindow = 512;
constexpr int kMaxLdsBytes = 159 * 1024;          // of the 160 KB: a forward kernel's few static words go beside the dynamic part
constexpr int kPrepareThreads = 256;

inline bool states_ok(int S) { return S % 4 == 0 && S >= kMinStates && S <= kMaxStates; }
inline bool window_ok(int reach_left, int reach_right) {
    return reach_left >= 0 && reach_right >= 0 && (long long)reach_left + reach_right + 4 <= kMaxWindow;
}
// the shapes and bands the routes take; each adds its own term (k, the LDS of one item or stream)
inline bool shape_ok(int S, int reach_left, int reach_right) { return states_ok(S) && window_ok(reach_left, reach_right); }

inline size_t diagonals_bytes(int S, int reach_left, int reach_right) {
    return ((size_t)reach_left + reach_right + 1) * S * sizeof(float);
}

__device__ __forceinline__ bool nonfinite(float x) { return !(x < INFINITY); }     // NaN or +inf

// The promise, one thread's share of row j (`row` = A + j * S; the thread looks at columns first, first + stride, ...):
// whether an entry outside [j - reach_left, j + reach_right] differs from the background (`want_bits`) in any bit.
__device__ __forceinline__ bool stray_in_row(const float *__restrict__ row, int j, int reach_left, int reach_right, int S,
                                             unsigned want_bits, int first, int stride) {
    bool stray = false;
    for (int i = first; i < S; i += stride)
        if ((i < j - reach_left || i > j + reach_right) && __float_as_uint(row[i]) != want_bits) stray = true;
    return stray;
}

// ok[0] = 1 (a launch of one thread before prepare_kernel, which only ever writes 0)
__global__ void verdict_kernel(int32_t *__restrict__ ok) { ok[0] = 1; }

// Row j of the matrix per workgroup: diag[k][j] = A[j][j - reach_left + k] (0 where that column does not exist: the forward
// kernels meet it with a halo or never use it); ok[0] = 0 where the promise is broken; alarm[0] = 1 where the row holds a
// NaN or +inf (zeroed before) -- `alarm` is null for a route without a matrix alarm, and then nothing else is written.
__global__ __launch_bounds__(kPrepareThreads) void prepare_kernel(const float *__restrict__ trans, float *__restrict__ diag,
                                                                  int32_t *__restrict__ ok, int32_t *__restrict__ alarm,
                                                                  float background, int reach_left, int reach_right, int S) {
    const int j = blockIdx.x, tid = threadIdx.x;
    const int W = reach_left + reach_right + 1;
    const float *row = trans + (size_t)j * S;
    for (int k = tid; k < W; k += kPrepareThreads) {
        const int i = j - reach_left + k;
        diag[(size_t)k * S + j] = (i >= 0 && i < S) ? row[i] : 0.f;
    }
    if (stray_in_row(row, j, reach_left, reach_right, S, __float_as_uint(background), tid, kPrepareThreads)) ok[0] = 0;
    if (alarm) {
        bool bad = false;
        for (int i = tid; i < S; i += kPrepareThreads) bad |= nonfinite(row[i]);
        if (bad) alarm[0] = 1;
    }
}

// host: the two launches above on `st`, in this order.  `alarm`: the route's matrix alarm word (zeroed by the caller), or null.
inline hipError_t prepare(const float *trans, float *diag, int32_t *ok, int32_t *alarm, float background, int reach_left,
                          int reach_right, int S, hipStream_t st) {
    hipLaunchKernelGGL(verdict_kernel, dim3(1), dim3(1), 0, st, ok);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(prepare_kernel, dim3(S), dim3(kPrepareThreads), 0, st, trans, diag, ok, alarm, background, reach_left,
                       reach_right, S);
    return hipGetLastError();
}

}  // namespace banddiag
