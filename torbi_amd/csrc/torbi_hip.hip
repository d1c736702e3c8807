// torbi_hip.hip -- MI355X (gfx950 / CDNA4) batched Viterbi decoder behind a plain C ABI.
//
// Written from scratch for wave64 / LDS / 256-CU CDNA4; not derived from the reference's
// CUDA kernels.  The reference functions each piece replaces are cited by file:line
// (paths relative to /root/reference/torbi/csrc/).
//
//   forward recurrence   viterbi.cpp:65-108 (oracle semantics) / cuda/viterbi.cu:48-130
//   final argmax + fill  viterbi.cpp:218-221                   / cuda/viterbi.cu:347-350
//   backtrace            viterbi.cpp:140-160                   / cuda/viterbi.cu:150-176
//   orchestration        viterbi.cpp:182-234                   / cuda/viterbi.cu:309-362
//
// The forward recurrence is a (max,+) matrix product per timestep,
//     post'[b,j] = obs[b,t,j] + max_i ( post[b,i] + trans[j,i] ),   bp[b,t,j] = first argmax_i
// i.e. a GEMM-shaped contraction over i with M = batch, N = K = states, in the (max,+)
// semiring: VALU work (MFMA cannot evaluate it), 2 fp32 roundings per cell in a fixed order.
// See DESIGN.md for the roofline analysis and kernel inventory.

#include <hip/hip_runtime.h>
#include <algorithm>
#include <atomic>
#include <mutex>
#include <type_traits>
#include <vector>
#include <stdint.h>
#include <stddef.h>
#include <math.h>
#include <stdlib.h>

#include "torbi_hip.h"
#include "scratch.hpp"
#include "dispatch.hpp"
#include "dense_forward.hpp"
#include "lazy_backtrace.hpp"
#include "uniform_decode.hpp"
#include "pruned_forward.hpp"
#include "resident_forward.hpp"
#include "small_batch_forward.hpp"
#include "held_matrix_forward.hpp"
#include "small_states.hpp"
#include "band_forward.hpp"
#include "band_tile_forward.hpp"
#include "stream.hpp"
#include "stream_band.hpp"
#include "stream_posterior.hpp"
#include "forward_backward.hpp"
#include "forward_backward_band.hpp"
#include "stream_posterior_band.hpp"
#include "counts_band.hpp"
#include "counts.hpp"
#include "k_best.hpp"
#include "k_best_band.hpp"
#include "sample.hpp"
#include "sample_band.hpp"
#include "max_marginals.hpp"
#include "max_marginals_band.hpp"
#include "path_statistics.hpp"
#include "path_entropy.hpp"
#include "path_entropy_band.hpp"

namespace {

constexpr int kWave = 64;

// ---------------------------------------------------------------------------------------
// helpers
// ---------------------------------------------------------------------------------------

// (value, index) comparator of the reference CPU scan (viterbi.cpp:94-100): a candidate
// replaces the incumbent only if strictly greater; among equal values the lower index wins.
__device__ __forceinline__ void take_better(float &v, int &i, float ov, int oi) {
    if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
}

__device__ __forceinline__ void wave_argmax(float &v, int &i) {
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) {
        const float ov = __shfl_down(v, off, kWave);
        const int oi = __shfl_down(i, off, kWave);
        take_better(v, i, ov, oi);
    }
}

// ---------------------------------------------------------------------------------------
// t = 0 : post[b,i] = obs[b,0,i] + initial[i]                       (viterbi.cpp:72-76)
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void init_posterior_kernel(
    const float *__restrict__ obs, const float *__restrict__ initial, float *__restrict__ post0,
    int B, int T, int S) {
    const size_t n = (size_t)B * S;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < n;
         e += (size_t)gridDim.x * blockDim.x) {
        const int b = (int)(e / S);
        const int i = (int)(e - (size_t)b * S);
        post0[e] = obs[(size_t)b * T * S + i] + initial[i];
    }
}

// ---------------------------------------------------------------------------------------
// One timestep, small-batch form: grid = (state tiles, batch items); each wave owns 4
// next-states, its 64 lanes stride the prev-state axis (coalesced transition-row reads,
// posterior row staged once in LDS), then a wave (value,index) reduction that keeps the
// lowest index among equal maxima.
// ---------------------------------------------------------------------------------------
constexpr int kRowsPerWave = 4;
constexpr int kRowsPerBlock = 16;

__global__ __launch_bounds__(256) void step_rows_kernel(
    const float *__restrict__ obs, const int32_t *__restrict__ frames,
    const float *__restrict__ trans, const float *__restrict__ pcur, float *__restrict__ pnext,
    int32_t *__restrict__ trellis, int B, int T, int S, int t, int b0) {
    extern __shared__ __attribute__((aligned(16))) float pl[];
    const int b = b0 + blockIdx.y;            // (gridDim.y holds at most 65535 items: larger batches take several launches)
    if (t >= frames[b]) return;
    const int tid = threadIdx.x;
    for (int i = tid; i < S; i += 256) pl[i] = pcur[(size_t)b * S + i];
    __syncthreads();

    const int lane = tid & 63, wave = tid >> 6;
    const int jb = blockIdx.x * kRowsPerBlock + wave * kRowsPerWave;
    if (jb >= S) return;
    const float *rows[kRowsPerWave];
    float best[kRowsPerWave];
    int arg[kRowsPerWave];
#pragma unroll
    for (int r = 0; r < kRowsPerWave; ++r) {
        const int j = min(jb + r, S - 1);
        rows[r] = trans + (size_t)j * S;
        best[r] = -INFINITY;
        arg[r] = 0x7fffffff;   // lanes that saw no candidate must lose index ties
    }
    for (int i = lane; i < S; i += kWave) {
        const float p = pl[i];
#pragma unroll
        for (int r = 0; r < kRowsPerWave; ++r) {
            const float c = p + rows[r][i];
            if (c > best[r]) { best[r] = c; arg[r] = i; }
            else if (arg[r] == 0x7fffffff) { arg[r] = i; best[r] = c; }  // first candidate, incl. -inf
        }
    }
#pragma unroll
    for (int r = 0; r < kRowsPerWave; ++r) wave_argmax(best[r], arg[r]);
    if (lane == 0) {
        const size_t row = ((size_t)b * T + t) * S;
#pragma unroll
        for (int r = 0; r < kRowsPerWave; ++r) {
            const int j = jb + r;
            if (j < S) {
                trellis[row + j] = arg[r];
                pnext[(size_t)b * S + j] = obs[row + j] + best[r];
            }
        }
    }
}

// Small-batch timestep, vector form (S % 4 == 0, 16-byte aligned rows): one next-state per wave,
// 4 per block, so a batch-1 step spreads over S/4 workgroups; each lane owns 4 consecutive
// prev-states per 256-wide stripe (ascending per lane, like the reference scan) and loads the
// transition row as float4.
__global__ __launch_bounds__(256) void step_rows4_kernel(
    const float *__restrict__ obs, const int32_t *__restrict__ frames,
    const float *__restrict__ trans, const float *__restrict__ pcur, float *__restrict__ pnext,
    int32_t *__restrict__ trellis, int B, int T, int S, int t, int b0) {
    extern __shared__ __attribute__((aligned(16))) float pl[];
    const int b = b0 + blockIdx.y;
    if (t >= frames[b]) return;
    const int tid = threadIdx.x;
    {
        const float4 *src = reinterpret_cast<const float4 *>(pcur + (size_t)b * S);
        float4 *dst = reinterpret_cast<float4 *>(pl);
        for (int i = tid; i < S / 4; i += 256) dst[i] = src[i];
    }
    __syncthreads();
    const int lane = tid & 63, wave = tid >> 6;
    const int j = blockIdx.x * 4 + wave;
    if (j >= S) return;
    const float *row = trans + (size_t)j * S;
    float best = -INFINITY;
    int arg = 0x7fffffff;
    for (int i = 4 * lane; i < S; i += 256) {
        const float4 q = *reinterpret_cast<const float4 *>(row + i);
        const float4 p = *reinterpret_cast<const float4 *>(pl + i);
        const float c[4] = {p.x + q.x, p.y + q.y, p.z + q.z, p.w + q.w};
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (c[u] > best) { best = c[u]; arg = i + u; }
            else if (arg == 0x7fffffff) { arg = i + u; best = c[u]; }
        }
    }
    wave_argmax(best, arg);
    if (lane == 0) {
        const size_t e = ((size_t)b * T + t) * S + j;
        trellis[e] = arg;
        pnext[(size_t)b * S + j] = obs[e] + best;
    }
}

// ---------------------------------------------------------------------------------------
// Final state + tail fill + backtrace, one wave per batch item.
//   final = first argmax of the item's last posterior row           (viterbi.cpp:218)
//   out[b, t] = final for t >= frames-1                               (viterbi.cpp:219-221)
//   for t = frames-1 .. 1: idx = bp[b,t,idx]; out[b,t-1] = idx        (viterbi.cpp:153-157)
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void finalize_kernel(
    const float *__restrict__ post0, const float *__restrict__ post1,
    const int32_t *__restrict__ frames, const int32_t *__restrict__ trellis,
    int32_t *__restrict__ out, int B, int T, int S) {
    const int b = blockIdx.x;
    const int lane = threadIdx.x;
    int f = frames[b];
    f = f < 1 ? 1 : (f > T ? T : f);
    const float *post = (((f - 1) & 1) ? post1 : post0) + (size_t)b * S;

    float best = -INFINITY;
    int arg = 0x7fffffff;
    for (int i = lane; i < S; i += kWave) {
        const float v = post[i];
        if (v > best) { best = v; arg = i; }
        else if (arg == 0x7fffffff) { arg = i; best = v; }
    }
    wave_argmax(best, arg);
    const int fin = __shfl(arg, 0, kWave);

    int32_t *o = out + (size_t)b * T;
    for (int tt = f - 1 + lane; tt < T; tt += kWave) o[tt] = fin;
    if (lane == 0) {
        const int32_t *tr = trellis + (size_t)b * T * S;
        int idx = fin;
        for (int tt = f - 1; tt >= 1; --tt) {
            idx = tr[(size_t)tt * S + idx];
            o[tt - 1] = idx;
        }
    }
}

// ---------------------------------------------------------------------------------------
// The chase in parallel (a handful of long sequences: one lane following 500 dependent loads at ~265 ns each is 0.13 ms,
// an eighth of a whole batch-of-one decode).  A backpointer row is a function S -> S and the path is their composition
// applied to the final state, so the timesteps are cut into chunks of kChaseChunk:
//   chase_maps_kernel     every chunk at once, every state at once: where does a path that is in state s at the chunk's
//                         upper end stand at its lower end (kChaseChunk dependent lookups, all rows L1/L2-resident);
//   chase_entries_kernel  one wave per item: final argmax + tail fill as in finalize_kernel, the top partial chunk
//                         directly, then chunk map after chunk map: the state at every chunk boundary;
//   chase_chunks_kernel   every chunk at once: the path inside the chunk from its upper boundary state.
// Three short launches instead of T dependent loads: 1 x 500 x 1440 in ~40 us instead of 132 us.  Same indices.
// ---------------------------------------------------------------------------------------
constexpr int kChaseChunk = 32;
constexpr int kChaseMinSteps = 128;        // below this the plain chase is as fast
inline int chase_chunks(int T) { return (T - 1 + kChaseChunk - 1) / kChaseChunk; }

__device__ __forceinline__ int clamped_frames(const int32_t *frames, int b, int T) {
    const int f = frames[b];
    return f < 1 ? 1 : (f > T ? T : f);
}

// grid = (chunks, B, ceil(S / 256)), block = 256: maps[b][k][s] = state at time k * C of the path that is in s at time (k + 1) * C
__global__ __launch_bounds__(256) void chase_maps_kernel(const int32_t *__restrict__ frames, const int32_t *__restrict__ trellis,
                                                         int32_t *__restrict__ maps, int B, int T, int S, int chunks) {
    const int k = blockIdx.x, b = blockIdx.y;
    const int s = blockIdx.z * 256 + threadIdx.x;
    const int last = clamped_frames(frames, b, T) - 1;          // the path ends at time `last`
    const int hi = (k + 1) * kChaseChunk;
    if (hi > last || s >= S) return;                            // only chunks the path crosses completely
    const int32_t *tr = trellis + (size_t)b * T * S;
    int idx = s;
    for (int t = hi; t > k * kChaseChunk; --t) idx = tr[(size_t)t * S + idx];
    maps[((size_t)b * chunks + k) * S + s] = idx;
}

// grid = B, block = 64
__global__ __launch_bounds__(64) void chase_entries_kernel(const float *__restrict__ post0, const float *__restrict__ post1,
                                                           const int32_t *__restrict__ frames, const int32_t *__restrict__ trellis,
                                                           const int32_t *__restrict__ maps, int32_t *__restrict__ entries,
                                                           int32_t *__restrict__ out, int B, int T, int S, int chunks) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int f = clamped_frames(frames, b, T);
    const float *post = (((f - 1) & 1) ? post1 : post0) + (size_t)b * S;
    float best = -INFINITY;
    int arg = 0x7fffffff;
    for (int i = lane; i < S; i += kWave) {
        const float v = post[i];
        if (v > best) { best = v; arg = i; }
        else if (arg == 0x7fffffff) { arg = i; best = v; }
    }
    wave_argmax(best, arg);
    const int fin = __shfl(arg, 0, kWave);
    int32_t *o = out + (size_t)b * T;
    for (int tt = f - 1 + lane; tt < T; tt += kWave) o[tt] = fin;
    if (lane == 0) {
        const int32_t *tr = trellis + (size_t)b * T * S;
        const int last = f - 1;
        const int k0 = last / kChaseChunk;                      // complete chunks below the path's end: 0 .. k0 - 1
        int idx = fin;
        for (int tt = last; tt > k0 * kChaseChunk; --tt) {      // the partial chunk at the top, directly
            idx = tr[(size_t)tt * S + idx];
            o[tt - 1] = idx;
        }
        for (int k = k0 - 1; k >= 0; --k) {                     // idx = state at time (k + 1) * C
            entries[(size_t)b * chunks + k] = idx;
            idx = maps[((size_t)b * chunks + k) * S + idx];
            o[k * kChaseChunk] = idx;
        }
    }
}

// grid = (chunks, B), block = 64: the path inside chunk k from its upper boundary state
__global__ __launch_bounds__(64) void chase_chunks_kernel(const int32_t *__restrict__ frames, const int32_t *__restrict__ trellis,
                                                          const int32_t *__restrict__ entries, int32_t *__restrict__ out,
                                                          int B, int T, int S, int chunks) {
    const int k = blockIdx.x, b = blockIdx.y;
    const int last = clamped_frames(frames, b, T) - 1;
    if ((k + 1) * kChaseChunk > last || threadIdx.x != 0) return;
    const int32_t *tr = trellis + (size_t)b * T * S;
    int32_t *o = out + (size_t)b * T;
    int idx = entries[(size_t)b * chunks + k];
    for (int t = (k + 1) * kChaseChunk; t > k * kChaseChunk + 1; --t) {
        idx = tr[(size_t)t * S + idx];
        o[t - 1] = idx;
    }
}

// final posterior rows of the last decode, whatever path it took (route record): the generic path keeps them in its
// ping-pong buffers, every value-only path as row frames-1 of the history at the start of the workspace
__global__ __launch_bounds__(256) void gather_final_kernel(const int32_t *__restrict__ route, const float *__restrict__ hist,
                                                           const float *__restrict__ post0, const float *__restrict__ post1,
                                                           const int32_t *__restrict__ frames, float *__restrict__ dst,
                                                           int B, int T, int S) {
    const bool generic = *route == 0 || *route == 6 || *route == 7;       // trellis kernels: per-timestep, held-matrix, one wavefront
    const size_t n = (size_t)B * S;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (size_t)gridDim.x * blockDim.x) {
        const int b = (int)(e / S);
        const int i = (int)(e - (size_t)b * S);
        int f = frames[b];
        f = f < 1 ? 1 : (f > T ? T : f);
        dst[e] = generic ? (((f - 1) & 1) ? post1 : post0)[e] : hist[((size_t)b * T + (f - 1)) * S + i];
    }
}

// scan statistics of the last decode by its route record: time-resident forms (and the held kernel's give-ups), else zeros
__global__ __launch_bounds__(128) void gather_stats_kernel(const int32_t *__restrict__ route, const unsigned *__restrict__ resident_stats,
                                                           const unsigned *__restrict__ held_control, unsigned *__restrict__ dst) {
    const int r = *route;
    const unsigned *src = (r == 3 || r == 5 || r == 8) ? resident_stats : nullptr;      // (band launches count their give-ups in [127] too)
    unsigned v = src ? src[threadIdx.x] : 0u;
    // held-matrix launch: [127] = workgroups that gave up waiting (the decode was then repaired; 0 on any sane run)
    if (r == 6 && held_control && threadIdx.x == 127) v = held_control[1];
    // dense launches: [120], [121] = shader-clock / 100 MHz wall-clock ticks of workgroup 0 of the last timestep's launch (the
    // time-resident and band kernels leave theirs in the statistics themselves)
    if (r == 1 && (threadIdx.x == 120 || threadIdx.x == 121)) v = (unsigned)route[2 + (threadIdx.x - 120)];
    dst[threadIdx.x] = v;
}

// x <- log(exp(x) + tiny), the epsilon clamp of from_probabilities (torbi/core.py:193-197)
__global__ __launch_bounds__(256) void epsilon_clamp_kernel(float *__restrict__ x, uint64_t count) {
    const float tiny = 1.17549435e-38f;   // torch.finfo(torch.float32).tiny
    const uint64_t n4 = count / 4;
    float4 *x4 = reinterpret_cast<float4 *>(x);
    for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n4;
         e += (uint64_t)gridDim.x * blockDim.x) {
        float4 v = x4[e];
        v.x = logf(expf(v.x) + tiny);
        v.y = logf(expf(v.y) + tiny);
        v.z = logf(expf(v.z) + tiny);
        v.w = logf(expf(v.w) + tiny);
        x4[e] = v;
    }
    for (uint64_t e = n4 * 4 + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < count;
         e += (uint64_t)gridDim.x * blockDim.x)
        x[e] = logf(expf(x[e]) + tiny);
}

// y = log(exp(log(p)) + tiny): the log() of probability inputs (torbi/core.py:189-191) and the epsilon clamp behind it
// (core.py:193-197) in one pass, out of place like upstream's torch.log -- or in place (y == p: every element is read and
// written by one thread; the many-file driver's staged batches)
__global__ __launch_bounds__(256) void log_epsilon_clamp_kernel(const float *p, float *y, uint64_t count) {
    const float tiny = 1.17549435e-38f;
    const uint64_t n4 = count / 4;
    const float4 *p4 = reinterpret_cast<const float4 *>(p);
    float4 *y4 = reinterpret_cast<float4 *>(y);
    for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n4;
         e += (uint64_t)gridDim.x * blockDim.x) {
        float4 v = p4[e];
        v.x = logf(expf(logf(v.x)) + tiny);
        v.y = logf(expf(logf(v.y)) + tiny);
        v.z = logf(expf(logf(v.z)) + tiny);
        v.w = logf(expf(logf(v.w)) + tiny);
        y4[e] = v;
    }
    for (uint64_t e = n4 * 4 + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < count;
         e += (uint64_t)gridDim.x * blockDim.x)
        y[e] = logf(expf(logf(p[e])) + tiny);
}

// deterministic synthetic scores, same function as torbi_amd/synth.py::scores
__global__ __launch_bounds__(256) void fill_synthetic_kernel(float *__restrict__ dst,
                                                             uint64_t count, uint64_t start,
                                                             uint64_t stream_key) {
    for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < count;
         e += (uint64_t)gridDim.x * blockDim.x) {
        uint64_t z = (start + e) + stream_key;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        z = z ^ (z >> 31);
        const uint32_t u = (uint32_t)(z >> 40);
        dst[e] = 0.0f - (float)u * 0x1p-20f;
    }
}

// ---------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------
struct DeviceGuard {
    int prev = -1;
    hipError_t err;
    explicit DeviceGuard(int device) {
        err = hipGetDevice(&prev);
        if (err == hipSuccess && prev != device) err = hipSetDevice(device);
    }
    ~DeviceGuard() {
        int cur = -1;
        if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
    }
};

// Compute units of a device (tiling plans are functions of (B, S, CUs)); queried once per device.
constexpr int kMaxDevices = 64;
std::atomic<int> g_cus[kMaxDevices];
inline int cu_count(int device) {
    if (device < 0 || device >= kMaxDevices) return 256;
    int v = g_cus[device].load(std::memory_order_relaxed);
    if (v > 0) return v;
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || n <= 0) n = 256;
    g_cus[device].store(n, std::memory_order_relaxed);
    return n;
}

// hipFuncAttributeMaxDynamicSharedMemorySize is per (kernel, device): set once, and again only for a larger request
struct LdsGrant { const void *fn; int device; size_t bytes; };
std::mutex g_lds_mutex;
std::vector<LdsGrant> g_lds_grants;
inline hipError_t ensure_dynamic_lds(const void *fn, size_t bytes) {
    int device = 0;
    hipError_t e = hipGetDevice(&device);
    if (e != hipSuccess) return e;
    std::lock_guard<std::mutex> hold(g_lds_mutex);
    for (auto &g : g_lds_grants)
        if (g.fn == fn && g.device == device) {
            if (g.bytes >= bytes) return hipSuccess;
            e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
            if (e == hipSuccess) g.bytes = bytes;
            return e;
        }
    e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e == hipSuccess) g_lds_grants.push_back(LdsGrant{fn, device, bytes});
    return e;
}
// (for the very pointer a launch site launches: dispatch.hpp)
template <class... A>
inline hipError_t ensure_dynamic_lds(void (*kernel)(A...), size_t bytes) {
    return ensure_dynamic_lds(reinterpret_cast<const void *>(kernel), bytes);
}

// Decodes of this library that may still be running on a device, by stream: the end of every decode is marked with an
// event on its stream.  Read by AUTO before it picks the held-matrix kernel, whose workgroups must all be resident at
// once (held_matrix_forward.hpp): beside a launch on ANOTHER stream that holds the compute units -- a time-resident
// launch group takes all of them for tens of milliseconds, a second held launch can leave both partly resident -- its
// workgroups would spin until their time budget runs out and the slow repair kernel would decode the call.  With another
// stream busy a handful of sequences take the per-timestep kernels instead, which simply queue behind the other work.
// (Work this library did not launch is invisible here; the time budget and the repair kernel cover it.)
struct StreamMark { hipStream_t stream; hipEvent_t done; };
std::mutex g_marks_mutex;
std::vector<StreamMark> g_marks[kMaxDevices];
constexpr size_t kMaxMarks = 64;

// `s` is being captured into a HIP graph: nothing may be asked of an event (hipEventQuery invalidates a capture), and an
// event recorded now becomes a node of the graph that no later query may name
inline bool capturing(hipStream_t s) {
    hipStreamCaptureStatus status = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &status) != hipSuccess) { (void)hipGetLastError(); return false; }
    return status != hipStreamCaptureStatusNone;
}

inline void mark_decode_end(int device, hipStream_t s) {
    if (device < 0 || device >= kMaxDevices || capturing(s)) return;
    std::lock_guard<std::mutex> hold(g_marks_mutex);
    auto &marks = g_marks[device];
    StreamMark *slot = nullptr;
    for (auto &m : marks)
        if (m.stream == s) { slot = &m; break; }
    if (!slot && marks.size() >= kMaxMarks) {           // full: take over the mark of a stream that has gone quiet
        for (auto &m : marks)
            if (hipEventQuery(m.done) == hipSuccess) { slot = &m; break; }
        if (!slot) return;
        slot->stream = s;
    }
    if (!slot) {
        hipEvent_t ev;
        if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) { (void)hipGetLastError(); return; }
        marks.push_back(StreamMark{s, ev});
        slot = &marks.back();
    }
    if (hipEventRecord(slot->done, s) != hipSuccess) (void)hipGetLastError();
}

inline bool other_streams_busy(int device, hipStream_t s) {
    // (while capturing: what the replays will run beside is unknown anyway; the held kernel's bounded waits and its
    // repair launch cover a busy device)
    if (device < 0 || device >= kMaxDevices || capturing(s)) return false;
    std::lock_guard<std::mutex> hold(g_marks_mutex);
    for (auto &m : g_marks[device])
        if (m.stream != s) {
            const hipError_t q = hipEventQuery(m.done);
            if (q == hipErrorNotReady) return true;
            if (q != hipSuccess) (void)hipGetLastError();
        }
    return false;
}

// name of the forward kernel the calling thread's most recent decode launched, spelled as rocprofv3 prints it
// (torbi_hip_last_forward_kernel: bench.py matches it against the committed counter summaries)
thread_local char g_last_kernel[160] = "";
#include <stdio.h>
#define TORBI_NOTE_KERNEL(...) snprintf(g_last_kernel, sizeof(g_last_kernel), __VA_ARGS__)

// Which forward recurrence runs.  GENERIC and HELD materialise the int32 trellis like the reference does; the others
// keep the posterior history and recompute backpointers along the decoded path (lazy_backtrace.hpp).  (2 was the
// per-timestep tile kernel of the pruned recurrence, removed in round 4: no route has the number any more.)
enum Route { ROUTE_GENERIC = 0, ROUTE_DENSE = 1, ROUTE_PRUNED = 2, ROUTE_RESIDENT = 3, ROUTE_ROWS = 4, ROUTE_CLUSTER = 5,
             ROUTE_HELD = 6, ROUTE_SMALL = 7, ROUTE_BAND = 8 };

inline bool use_dense(int B, int S) { return B >= 32 && S >= 64; }

// process-wide default path: torbi_hip_set_forward_path / TORBI_HIP_FORWARD=dense|pruned|resident (read once).
// A call that carries a path in its flags ignores it.
std::atomic<int> g_forward_path{-1};
inline int default_path() {
    int v = g_forward_path.load(std::memory_order_relaxed);
    if (v < 0) {
        const char *e = getenv("TORBI_HIP_FORWARD");
        v = !e ? TORBI_HIP_FORWARD_AUTO
               : e[0] == 'd' ? TORBI_HIP_FORWARD_DENSE
               : e[0] == 'p' ? TORBI_HIP_FORWARD_PRUNED
               : e[0] == 'r' ? TORBI_HIP_FORWARD_RESIDENT
               : e[0] == 'c' ? TORBI_HIP_FORWARD_CLUSTER
               : e[0] == 'h' ? TORBI_HIP_FORWARD_HELD
               : e[0] == 'b' ? TORBI_HIP_FORWARD_BAND : TORBI_HIP_FORWARD_AUTO;
        g_forward_path.store(v, std::memory_order_relaxed);
    }
    return v;
}
// path carried by the flags of a call ((path + 1) << 4), else the process default
inline int requested_path(unsigned flags) {
    const unsigned f = (flags >> 4) & 7u;
    return f ? (int)f - 1 : default_path();
}
constexpr unsigned kKnownFlags = TORBI_HIP_REUSE_TRANSITION | TORBI_HIP_COLLECT_STATS | (7u << 4) | TORBI_HIP_SHORTEST_FIRST |
                                 TORBI_HIP_FEW_SEEDS | TORBI_HIP_MANY_SEEDS;
inline bool flags_ok(unsigned flags) {
    return !(flags & ~kKnownFlags) && ((flags >> 4) & 7u) <= (unsigned)TORBI_HIP_FORWARD_BAND + 1u;
}

constexpr int kMaxGroupTiles = 16384;     // 16-item tiles one launch group may hold (262 144 items)
// tiles of a batch in the time-resident kernel: 16 items each, 8 above 2048 states
inline int tiles_of(int B, int S) { const int ni = resident::tile_items(S); return (B + ni - 1) / ni; }
inline bool resident_fits(int S, int tiles) { return resident::supported(S) && tiles <= kMaxGroupTiles; }

// members per cluster for a launch of `tiles` 16-item tiles: 1 (every workgroup owns a whole tile) once the tiles give
// at least half the compute units a workgroup, else as many as the compute units allow (<= kMaxR, <= one row group each)
inline int cluster_members(int tiles, int S, int cus) {
    if (tiles < 1 || 2 * tiles > cus) return 1;
    int R = cus / tiles;
    const int nrg = (S + resident::pass_rows(S) - 1) / resident::pass_rows(S);
    R = std::min(R, std::min(resident::kMaxR, nrg));
    return R < 2 ? 1 : R;
}

// AUTO takes the held-matrix kernel up to this many items.  tools/held_probe.py,
// ms per decode against the best per-timestep kernel (profiles/r03_held_probe.txt): 500 frames x 1440 states 1 item
// 1.10 / 2.41, 2 items 1.38 / 2.52, 3 items 2.16 / 2.69, 4 items 2.83 / 2.85, 8 items 5.44 / 4.31; 300 frames x 4096 states
// 1 item 1.28 / 3.87, 2 items 1.86 / 4.20, 4 items 3.79 / 5.95, 8 items 7.41 / 9.34.  A timestep of the kernel costs one
// hand-off (~1.5 us) for up to two sequences and ~1.3 us of instruction issue for every further one; a launch of the
// per-timestep kernels 4.4 us plus ~0.3 us per item.
inline bool held_auto(int B, int S) { return B <= (S > held::kSmallS ? 8 : 3); }

// route of ONE batch.  AUTO: the time-resident kernel -- whole tiles per workgroup when the batch alone gives at least
// half the compute units a workgroup, tiles split over clusters of workgroups for smaller batches of >= 17 items --
// else the sorted-row scan / held-matrix kernel for a handful of sequences, else the dense (max,+) GEMM, else generic.
inline bool small_block_auto(int B, int S, int cus) {
    // (value-only since round 5: ahead of the time-resident kernels at every batch size up to 192 states -- 8192 x 200 x 128
    // 2.0 against 4.0 ms, 8192 x 100 x 192 2.8 against 3.0 -- and up to ~3000 sequences at 256: 2048 x 200 x 256 1.6 against
    // 2.3 ms, 4096 x 200 x 256 3.2 against 2.9.  The limit: 12 x 65536 cells per compute unit)
    return small::block_supported(S) && (S <= 192 || (long long)B * S * S <= (12ll << 16) * cus);
}
inline Route route_for(int path, int B, int S, int cus, bool allow_held = true) {
    if (path == TORBI_HIP_FORWARD_BAND) path = TORBI_HIP_FORWARD_AUTO;     // (a band is known to torbi_hip_viterbi_decode_banded only)
    const bool fits = resident_fits(S, tiles_of(B, S));
    // up to 64 states a wavefront decodes a sequence on its own, time loop and backtrace in one launch (small_states.hpp)
    // ... up to 256 a workgroup does (the matrix in the registers of one compute unit), while the batch is not so large that
    // the time-resident forms' pruning overtakes it: tools/small_states_probe.py, 500 frames, small / resident ms --
    // 4096 x 128: 3.7 / 4.2, 512 x 256: 2.3 / 3.5 (cluster), 1024 x 256: 4.2 / 3.4, 4096 x 256: 19.2 / 6.0 -- B S^2 <= 3 * 2^16 per
    // compute unit (768 items at 256 states, 3072 at 128: the kernel runs one workgroup, or four, per unit at a time)
    if (path == TORBI_HIP_FORWARD_AUTO && (small::supported(S) || small_block_auto(B, S, cus))) return ROUTE_SMALL;
    if (path == TORBI_HIP_FORWARD_RESIDENT && fits) return ROUTE_RESIDENT;
    if (path == TORBI_HIP_FORWARD_CLUSTER && fits) return cluster_members(tiles_of(B, S), S, cus) > 1 ? ROUTE_CLUSTER : ROUTE_RESIDENT;
    if (path == TORBI_HIP_FORWARD_AUTO && fits && 2 * tiles_of(B, S) > cus) return ROUTE_RESIDENT;
    // (one batch, AUTO: clusters for every batch of more than 16 items -- with one seed per item and one polling wave per
    // workgroup the cluster form is at least as fast as the per-timestep kernel from 17 items on: 12.8 against 14.5 us per
    // timestep at 17 items, 15.6 against 20.2 at 512, 20.4 against 34.9 at 768 (profiles/r03_cluster_sweep_one_poller.txt);
    // 128 x 2000 x 4096 on 8-item tiles 54.2 against 55.9 ms)
    if (path == TORBI_HIP_FORWARD_AUTO && fits && B > 16 && cluster_members(tiles_of(B, S), S, cus) > 1)
        return ROUTE_CLUSTER;
    // PRUNED named for more than 16 items: the pruned recurrence in its time-resident form (its per-timestep tile kernel was
    // removed in round 4; up to 16 items PRUNED means the sorted-row scan below)
    if (path == TORBI_HIP_FORWARD_PRUNED && fits && B > 16)
        return cluster_members(tiles_of(B, S), S, cus) > 1 ? ROUTE_CLUSTER : ROUTE_RESIDENT;
    // a handful of sequences: the whole time loop in one launch, the matrix held in registers across the chip
    // (held_matrix_forward.hpp) -- AUTO up to three items, eight above 2048 states (held_auto); any B <= 16 when named
    if (held::supported(B, S, cus) &&
        (path == TORBI_HIP_FORWARD_HELD || (path == TORBI_HIP_FORWARD_AUTO && allow_held && held_auto(B, S))))
        return ROUTE_HELD;
    // up to 16 items the sorted-row scan's time grows with items x states, the cluster form's (one tile, sixteen members)
    // does not: 12 x 1440 rows 5.1 / cluster 5.3 ms per 500 frames, 16 x 1440 6.1 / 5.3, 12 x 2048 4.6 / 4.2 per 300,
    // 12 x 4096 8.7 / 4.8 per 200, 16 x 4096 10.9 / 4.8 -- but 16 x 512 2.4 / 3.6 (tools/few_items_probe.py)
    if (path == TORBI_HIP_FORWARD_AUTO && fits && (long long)B * S > 12ll * 1440 &&
        cluster_members(tiles_of(B, S), S, cus) > 1)
        return ROUTE_CLUSTER;
    if ((path == TORBI_HIP_FORWARD_PRUNED && rowscan::supported(B, S)) ||
        (path != TORBI_HIP_FORWARD_DENSE && rowscan::profitable(B, S)))
        return ROUTE_ROWS;
    // a named path that does not cover the shape falls back as AUTO would (DENSE named below 32 items: the generic kernels)
    if (path != TORBI_HIP_FORWARD_AUTO && path != TORBI_HIP_FORWARD_DENSE)
        return route_for(TORBI_HIP_FORWARD_AUTO, B, S, cus, allow_held);
    return use_dense(B, S) ? ROUTE_DENSE : ROUTE_GENERIC;
}

// ---- workspace layouts: the (B,T,S) history / trellis first, the per-transition preparation behind it ---------
// Every layout states each region once, as a take of a Scratch (scratch.hpp), and its `bytes` are the cursor behind the last
// of them; a size query lays the same regions out on a null base.
struct Workspace {
    float *post[2];     // (B,S) ping-pong posterior rows
    int32_t *trellis;   // (B,T,S) backpointers; rows t >= 1 of valid frames are written
    held::u64 *xchg;    // [2][B][S] {posterior, timestep} words of the held-matrix kernel (B <= 16, S <= 2048), else null
    unsigned *control;  // [64] its control words ([1]: workgroups that gave up waiting)
    int32_t *maps;      // [B][chunks][S] chunk maps of the parallel chase (B <= 16, S <= 4096, T >= 129), else null
    int32_t *entries;   // [B][chunks]    the path's state at every chunk boundary
    int32_t *arrive;    // [B][8] ends of the backtrace's speculative segments (65 .. 256 states, B <= 1024), else null
    size_t bytes;
};

inline Workspace carve(void *base, int B, int T, int S) {
    Scratch a(base);
    Workspace w{};
    w.trellis = a.take<int32_t>((size_t)B * T * S);
    for (float *&post : w.post) post = a.take<float>((size_t)B * S);
    if (B <= held::kMaxB && S <= held::kMaxS) {
        w.control = a.take<unsigned>(64);
        w.xchg = a.take<held::u64>(held::exchange_bytes(B, S) / sizeof(held::u64));
    }
    if (B <= held::kMaxB && S <= held::kMaxS && T - 1 >= kChaseMinSteps) {
        const size_t chunks = (size_t)chase_chunks(T);
        w.maps = a.take<int32_t>((size_t)B * chunks * S);
        w.entries = a.take<int32_t>((size_t)B * chunks);
    }
    if (small::block_supported(S) && B <= 1024) w.arrive = a.take<int32_t>((size_t)B * 8);
    w.bytes = a.bytes;
    return w;
}

// The per-transition preparation of the list scans: every row sorted and arranged (pruned::sort_rows_kernel; a row holds SpP
// entries, the sort works on NPOW), and for the time-resident routes the transposed matrix and the rows' finite ranges.
struct ListShape { int SpP, NPOW; };
inline ListShape list_shape(int S) {
    ListShape l{(S + 15) / 16 * 16 + pruned::kPad, 64};
    while (l.NPOW < S) l.NPOW *= 2;
    return l;
}
struct PreparedLists { float2 *sorted; float *tt; int32_t *row_range; };
inline PreparedLists lay_preparation(Scratch &a, int S) {
    PreparedLists l;
    l.sorted = a.take<float2>((size_t)S * list_shape(S).SpP);
    l.tt = a.take<float>((size_t)S * S);
    l.row_range = a.take<int32_t>(2 * (size_t)S);
    return l;
}
inline size_t preparation_bytes(int S) { Scratch a(nullptr); lay_preparation(a, S); return a.bytes; }

// the time-resident path: history, tile map, row maxima, sorted lists / transposed matrix, cluster exchange
struct ResidentWorkspace : PreparedLists, ListShape {
    float *hist;
    int32_t *order;       // [B] this batch's items by descending length
    float *rowmax;        // [B][T] largest entry of every posterior row (left by the forward kernel for the backtrace)
    int32_t *lengths_hist;  // [T + 2] items per length (batches above resident::kMaxOrdered items only, else null)
    size_t lengths_hist_bytes;
    int32_t *tile_map;    // [kMaxGroupTiles] workgroup -> tile of the launch group (first batch's workspace)
    unsigned *stats;      // [128] scan statistics of the last launch group (first batch's workspace)
    // cluster form (first batch's workspace): exchange buffers of up to cus / 2 tiles, and ONE block of `nflags` words that
    // order_tiles_kernel zeroes as a whole -- the parts of resident::Cluster
    float *xchg;          // [tiles][kSlots] slots
    unsigned *flags, *control, *failed, *where;      // [tiles][kMaxR], [16], [tiles], [tiles][kMaxR]
    int nflags;
    size_t bytes;
};

// The per-transition preparation of the time-resident routes may live OUTSIDE the workspace
// (torbi_hip_viterbi_decode_batches_prepared): a caller that allocates a workspace per call
// -- the reference's own calling pattern, torbi/core.py:200-206 -- keeps 25 MB per matrix instead of rebuilding it
// (0.25 ms per call at 1440 states).  Travels as an argument from the entry point to the one layout that reads it.
struct Preparation {
    void *pointer;
    size_t bytes;
    bool valid;      // holds this matrix's preparation (the caller's promise, or filled by this call)
};

// the serial number of the decode this host thread is launching: what its kernels raise their NaN / +inf alarms with
// (nonfinite.hpp; never 0, never repeated within a process: no alarm word has to be cleared between decodes)
static std::atomic<unsigned> g_serial_counter{(unsigned)(std::chrono::steady_clock::now().time_since_epoch().count() * 2654435761u)};
thread_local int t_serial = 0;          // of the decode this host thread is launching
inline int new_serial() {
    unsigned v;
    do { v = ++g_serial_counter; } while (v == 0u);
    t_serial = (int)v;
    return t_serial;
}

// `kept`: the caller's preparation buffer (run_resident only; every other layout of a workspace is the plain one)
inline ResidentWorkspace carve_resident(void *base, int B, int T, int S, int cus, const Preparation *kept = nullptr) {
    Scratch a(base);
    ResidentWorkspace w{};
    static_cast<ListShape &>(w) = list_shape(S);
    w.hist = a.take<float>((size_t)B * T * S);
    w.tile_map = a.take<int32_t>(kMaxGroupTiles);      // ahead of the preparation: offsets depend on B and T only
    w.stats = a.take<unsigned>(128);
    w.order = a.take<int32_t>((size_t)B);
    if (B > resident::kMaxOrdered) {
        const size_t hist_at = a.bytes;
        w.lengths_hist = a.take<int32_t>((size_t)T + 2);
        w.lengths_hist_bytes = a.bytes - hist_at;      // (what assemble_group clears: to the end of the region)
    }
    w.rowmax = a.take<float>((size_t)B * T);
    static_cast<PreparedLists &>(w) = lay_preparation(a, S);      // (the span stays in the workspace either way)
    if (base && kept && kept->bytes >= preparation_bytes(S)) {      // (the caller keeps it: see above)
        Scratch theirs(kept->pointer);
        static_cast<PreparedLists &>(w) = lay_preparation(theirs, S);
    }
    const size_t ctiles = (size_t)std::max(cus / 2, 1);                 // a cluster launch holds at most this many tiles
    w.xchg = a.take<float>(ctiles * resident::kSlots * resident::cluster_slot_bytes(S) / sizeof(float));
    const size_t flags_at = a.bytes;
    w.flags = a.take<unsigned>(2 * ctiles * resident::kMaxR + 16 + ctiles);
    w.control = behind(w.flags, ctiles * resident::kMaxR);
    w.failed = behind(w.control, 16);
    w.where = behind(w.failed, ctiles);
    w.nflags = (int)((a.bytes - flags_at) / sizeof(unsigned));      // (to the end of the block)
    w.bytes = a.bytes;
    return w;
}

// the band route (band_forward.hpp): the time-resident layout's history, tile map, statistics and item order, and BEHIND that
// layout the batch's exchange buffers and (first batch of a launch) the tickets and the give-up flags of the tiles
inline bool band_shape(int S) { return S % 4 == 0 && resident::supported(S) && S <= 64 * band::kMaxBlocks * band::kMaxR; }
struct BandWorkspace {
    ResidentWorkspace base;
    char *xchg;
    // ONE block of words that band::clear_exchange_kernel zeroes from its start
    unsigned *words, *failed, *tickets;      // [16], [kMaxGroupTiles], [8] per launch of the group
    float *tpack;         // whole tiles (band_tile_forward.hpp): the band as the lanes read it
    size_t bytes;
};
constexpr size_t kBandWords = 16 + 2 * (size_t)kMaxGroupTiles + 64;
inline BandWorkspace carve_band(void *base, int B, int T, int S, int cus) {
    BandWorkspace w{};
    w.base = carve_resident(base, B, T, S, cus);     // (the band route keeps nothing in a caller's preparation buffer)
    Scratch a(base, w.base.bytes);
    w.xchg = a.take<char>(band::xchg_bytes(B, S));
    w.words = a.take<unsigned>(kBandWords);
    w.failed = behind(w.words, 16);
    w.tickets = behind(w.failed, kMaxGroupTiles);
    w.tpack = a.take<float>(band::tile_pack_bytes_max(S) / sizeof(float));
    w.bytes = a.bytes;
    return w;
}

// small batches (B <= 16): history + sorted rows (small_batch_forward.hpp)
struct RowsWorkspace : ListShape {
    float *hist;
    float2 *sorted;
    int32_t *row_range;
    float *rowmax;     // [B][T] largest entry of every posterior row (step_rows_sorted_kernel leaves it for the backtrace)
    size_t bytes;
};

inline RowsWorkspace carve_rows(void *base, int B, int T, int S) {
    Scratch a(base);
    RowsWorkspace w{};
    static_cast<ListShape &>(w) = list_shape(S);
    w.hist = a.take<float>((size_t)B * T * S);
    w.sorted = a.take<float2>((size_t)S * w.SpP);
    w.row_range = a.take<int32_t>(2 * (size_t)S);
    w.rowmax = a.take<float>((size_t)B * T);
    w.bytes = a.bytes;
    return w;
}

struct DenseWorkspace {
    dense::Plan plan;
    float *hist;       // [B][T][S]      posterior history (replaces the int32 trellis)
    float *panel[2];   // [n_bt][Kp][BT] posterior panels (ping-pong)
    float *trp;        // [n_jt][Kp][W]  packed transition panels
    int32_t *chunks;   // [n_jt][NCH+1]  per-tile lists of chunks that are not all -inf
    int32_t *ranges;   // [S][2] finite range of every transition row, and in the same block ...
    int32_t *widest;   // ... [64], first word: the widest row window
    size_t bytes;
};

inline DenseWorkspace carve_dense(void *base, int B, int T, int S, int cus) {
    Scratch a(base);
    DenseWorkspace w{};
    w.plan = dense::make_plan(B, S, cus);
    w.hist = a.take<float>((size_t)B * T * S);
    for (float *&panel : w.panel) panel = a.take<float>((size_t)w.plan.n_bt * w.plan.Kp * w.plan.BT);
    w.trp = a.take<float>((size_t)w.plan.n_jt * w.plan.Kp * w.plan.W);
    w.chunks = a.take<int32_t>((size_t)w.plan.n_jt * (w.plan.NCH + 1));
    w.ranges = a.take<int32_t>(2 * (size_t)S + 64);
    w.widest = behind(w.ranges, 2 * (size_t)S);
    w.bytes = a.bytes;
    return w;
}

// scratch a (B,T,S) problem needs on a device with `cus` compute units, whichever path runs ...
inline size_t layout_bytes(int B, int T, int S, int cus) {
    size_t need = carve(nullptr, B, T, S).bytes;
    if (use_dense(B, S)) need = std::max(need, carve_dense(nullptr, B, T, S, cus).bytes);
    if (resident::supported(S)) need = std::max(need, carve_resident(nullptr, B, T, S, cus).bytes);
    if (rowscan::supported(B, S)) need = std::max(need, carve_rows(nullptr, B, T, S).bytes);
    if (band_shape(S)) need = std::max(need, carve_band(nullptr, B, T, S, cus).bytes);
    return need;
}
// ... plus the ROUTE RECORD behind every layout: the forward path the last decode with this workspace actually took
// (a Route), written on the stream by that decode and read ON THE DEVICE by torbi_hip_read_posterior /
// torbi_hip_scan_stats -- a batch decoded inside a launch group takes the group's route, not the one its own shape
// and flags would give it.
// ... and behind the record the two posterior rows per item of nonfinite::repair_kernel (NaN / +inf inputs: nonfinite.hpp)
inline size_t nonfinite_rows_bytes(int B, int S) { return align_up(sizeof(float) * 2 * (size_t)B * S, 256); }
inline size_t need_bytes(int B, int T, int S, int cus) { return layout_bytes(B, T, S, cus) + 256 + nonfinite_rows_bytes(B, S); }
inline int32_t *route_record(const void *workspace, int B, int T, int S, int cus) {
    return reinterpret_cast<int32_t *>(static_cast<char *>(const_cast<void *>(workspace)) + layout_bytes(B, T, S, cus));
}
__global__ void stamp_route_kernel(int32_t *record, int route) { *record = route; }
__global__ void fill_pair_kernel(int32_t *pair, int a, int b) { pair[0] = a; pair[1] = b; }
inline hipError_t stamp_route(int32_t *record, Route route, hipStream_t s) {
    // (a one-thread kernel: hipMemsetD32Async costs ~0.17 ms per call on this stack)
    hipLaunchKernelGGL(stamp_route_kernel, dim3(1), dim3(1), 0, s, record, (int)route);
    return hipGetLastError();
}

// ... on the device with the most demanding plan (devices of one node are normally identical)
inline size_t need_bytes_any_device(int B, int T, int S) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return need_bytes(B, T, S, 256);
    size_t need = 0;
    for (int d = 0; d < n && d < kMaxDevices; ++d) {
        const int cus = cu_count(d);
        bool seen = false;
        for (int e = 0; e < d; ++e) seen = seen || cu_count(e) == cus;
        if (!seen) need = std::max(need, need_bytes(B, T, S, cus));
    }
    return need;
}

int check_args(const void *a, const void *b, const void *c, const void *d, const void *e,
               const void *ws, size_t ws_bytes, int B, int T, int S, int device) {
    if (B < 0 || T < 1 || S < 1) return TORBI_HIP_EINVAL;
    if (B == 0) return TORBI_HIP_OK;
    if (!a || !b || !c || !d || !e || !ws) return TORBI_HIP_EINVAL;
    if ((size_t)B * T * S > (size_t)1 << 40) return TORBI_HIP_ERANGE;
    if (ws_bytes < need_bytes(B, T, S, cu_count(device))) return TORBI_HIP_EWORKSPACE;
    if (reinterpret_cast<uintptr_t>(ws) & 255) return TORBI_HIP_EINVAL;     // (the decode layouts start at the caller's base)
    return TORBI_HIP_OK;
}

// ---- generic path ---------------------------------------------------------------------
hipError_t launch_forward(const float *obs, const int32_t *frames, const float *trans,
                          const float *init, const Workspace &w, int B, int T, int S,
                          hipStream_t stream, int *launches) {
    {
        const size_t n = (size_t)B * S;
        const int grid = (int)((n + 255) / 256 < 2048 ? (n + 255) / 256 : 2048);
        hipLaunchKernelGGL(init_posterior_kernel, dim3(grid), dim3(256), 0, stream, obs, init,
                           w.post[0], B, T, S);
    }
    // one workgroup per (rows, item).  (Rounds 1-3 had a 64 x 64 tile kernel here for many items over fewer than 64
    // states; those shapes are decoded in one launch by small_states.hpp now.)
    int n = 0;
    for (int t = 1; t < T; ++t) {
        const float *pc = w.post[(t - 1) & 1];
        float *pn = w.post[t & 1];
        // (the item index is gridDim.y, which holds at most 65535: a larger batch -- S == 1 under AUTO, DENSE named below
        // 64 states -- takes its timestep in slices of that many items)
        for (int b0 = 0; b0 < B; b0 += 65535) {
            const int nb = std::min(65535, B - b0);
            if (S % 4 == 0 && S >= 256 && (reinterpret_cast<uintptr_t>(trans) & 15) == 0) {
                dim3 grid((S + 3) / 4, nb);
                hipLaunchKernelGGL(step_rows4_kernel, grid, dim3(256), sizeof(float) * (size_t)S,
                                   stream, obs, frames, trans, pc, pn, w.trellis, B, T, S, t, b0);
            } else {
                dim3 grid((S + kRowsPerBlock - 1) / kRowsPerBlock, nb);
                hipLaunchKernelGGL(step_rows_kernel, grid, dim3(256), sizeof(float) * (size_t)S,
                                   stream, obs, frames, trans, pc, pn, w.trellis, B, T, S, t, b0);
            }
        }
        ++n;
    }
    if (launches) *launches = n;
    return hipGetLastError();
}

// THE held-matrix instance for S states (all six share one signature): what the occupancy query asks about and what the
// launch launches -- a kernel whose workgroups wait for each other must be the one whose residency was checked.
using HeldKernel = decltype(&held::held_forward_kernel<1, 8, 512, true>);
struct HeldLaunch { HeldKernel kernel; int grid, block; };
inline HeldLaunch held_instance(int S) {
    const int K = (S + held::threads(S) - 1) / held::threads(S);
    const HeldKernel kernel =
        S <= held::kSmallS
            ? by_value<1, 2, 3, 4>(K, [](auto k) -> HeldKernel { return &held::held_forward_kernel<decltype(k)::value, 8, 512, true>; })
            : by_value<3, 4>(K, [](auto k) -> HeldKernel { return &held::held_forward_kernel<decltype(k)::value, 16, 1024, false>; });
    return HeldLaunch{kernel, held::workgroups(S), held::block_threads(S)};
}
// Can every workgroup of that launch be resident at once on `device`?  The runtime's occupancy answer for the very
// kernel (registers, LDS, waves), queried once per (kernel, device) -- held::supported()'s "two workgroups per compute
// unit up to 2048 states" is an assumption about this build on an MI355X, this is the check.
inline bool held_resident(int S, int device, int cus) {
    struct Known { HeldKernel kernel; int device; int per_cu; };
    static std::mutex mu;
    static std::vector<Known> known;
    const HeldLaunch h = held_instance(S);
    std::lock_guard<std::mutex> hold(mu);
    for (auto &k : known)
        if (k.kernel == h.kernel && k.device == device) return h.grid <= k.per_cu * cus;
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reinterpret_cast<const void *>(h.kernel), h.block, 0) != hipSuccess) {
        (void)hipGetLastError();
        per_cu = 0;
    }
    known.push_back(Known{h.kernel, device, per_cu});
    return h.grid <= per_cu * cus;
}

// the same outputs from ONE launch: the time loop inside the kernel, the matrix in registers (held_matrix_forward.hpp)
hipError_t launch_held_forward(const float *obs, const int32_t *frames, const float *trans, const float *init,
                               const Workspace &w, int B, int T, int S, hipStream_t stream, int *launches) {
    {
        const size_t n = (size_t)B * S;
        const int grid = (int)((n + 255) / 256 < 2048 ? (n + 255) / 256 : 2048);
        hipLaunchKernelGGL(held::prepare_kernel, dim3(grid), dim3(256), 0, stream, obs, init, w.post[0], w.xchg, w.control,
                           B, T, S);
    }
    if (launches) *launches = 1;
    if (T < 2) return hipGetLastError();
    // how long a workgroup waits for the others before it gives up (ticks of the 100 MHz wall clock): 20 x T x 2.5 us, at
    // least 2 ms -- 25 ms for 500 frames, against the ~1 ms the launch takes when it is resident.  TORBI_HIP_HELD_SPIN_LIMIT
    // overrides (polls of ~1 us; 0 forces the repair path in the tests).
    unsigned long long wait_ticks = std::max<unsigned long long>(200000ull, 5000ull * (unsigned long long)T);
    if (const char *polls = getenv("TORBI_HIP_HELD_SPIN_LIMIT")) wait_ticks = 100ull * strtoull(polls, nullptr, 10);
    const HeldLaunch h = held_instance(S);
    hipLaunchKernelGGL(h.kernel, dim3(h.grid), dim3(h.block), 0, stream, obs, frames, trans, w.post[0], w.post[1], w.trellis, w.xchg,
                       w.control, B, T, S, wait_ticks);
    // does nothing unless a workgroup above gave up waiting (held_matrix_forward.hpp)
    hipLaunchKernelGGL(held::repair_kernel, dim3(B), dim3(1024), 2 * sizeof(float) * (size_t)S, stream, obs, frames, trans, init,
                       w.post[0], w.post[1], w.trellis, w.control, B, T, S);
    return hipGetLastError();
}

hipError_t launch_finalize(const int32_t *frames, const Workspace &w, int32_t *out, int B, int T,
                           int S, hipStream_t stream) {
    if (w.maps) {        // a handful of long sequences: the chase in parallel (chase_*_kernel above)
        const int chunks = chase_chunks(T);
        hipLaunchKernelGGL(chase_maps_kernel, dim3(chunks, B, (S + 255) / 256), dim3(256), 0, stream, frames, w.trellis, w.maps,
                           B, T, S, chunks);
        hipLaunchKernelGGL(chase_entries_kernel, dim3(B), dim3(64), 0, stream, w.post[0], w.post[1], frames, w.trellis, w.maps,
                           w.entries, out, B, T, S, chunks);
        hipLaunchKernelGGL(chase_chunks_kernel, dim3(chunks, B), dim3(64), 0, stream, frames, w.trellis, w.entries, out,
                           B, T, S, chunks);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(finalize_kernel, dim3(B), dim3(64), 0, stream, w.post[0], w.post[1],
                       frames, w.trellis, out, B, T, S);
    return hipGetLastError();
}

// ---- up to 64 states: one wavefront per sequence, one launch per decode (small_states.hpp) ----------------------------
// The value-only form (no backpointers, lazy argmax on the path, the matrix shared through the LDS) from 32 padded states
// and 2 x compute-units sequences up -- tools/small_value_probe.py, ms per decode, backpointers / value-only:
// 512 x 500 x 40 0.259 / 0.233, 512 x 500 x 64 0.343 / 0.294, 4096 x 500 x 64 0.848 / 0.713, 4096 x 500 x 40 0.553 / 0.450;
// below 32 states the walk back costs more than the cells save (512 x 500 x 3 0.121 / 0.171, 8192 x 500 x 16 0.468 / 0.495).
// TORBI_HIP_SMALL_VALUE=0|1 forces either form (read per launch: the tests switch it).
inline bool small_value_form(int B, int S, int cus) {
    if (const char *e = getenv("TORBI_HIP_SMALL_VALUE")) return atoi(e) != 0;
    return small::padded_states(S) >= 32 && (long long)B >= 2ll * cus;
}
hipError_t launch_small(const float *obs, const int32_t *frames, const float *trans, const float *init, const Workspace &w,
                        int32_t *out, int32_t *record, int B, int T, int S, hipStream_t stream, int *launches, int cus = 256) {
    if (launches) *launches += 1;
    const bool value_form = small_value_form(B, S, cus);
    return by_value<4, 8, 16, 24, 32, 40, 48, 56, 64>(small::padded_states(S), [&](auto sp) {
        constexpr int SP = decltype(sp)::value, CH = SP <= 16 ? 16 : SP <= 40 ? 8 : 4;
        if (value_form) {
            auto *kernel = &small::decode_value_kernel<SP, CH>;
            TORBI_NOTE_KERNEL("small::decode_value_kernel<%d, %d>", SP, CH);
            hipLaunchKernelGGL(kernel, dim3((B + 3) / 4), dim3(256), 0, stream, obs, frames, trans, init, out,
                               reinterpret_cast<float *>(w.trellis), w.post[0], w.post[1], record, (int)ROUTE_SMALL, B, T, S, t_serial);
        } else {
            auto *kernel = &small::decode_kernel<SP, CH>;
            TORBI_NOTE_KERNEL("small::decode_kernel<%d, %d>", SP, CH);
            hipLaunchKernelGGL(kernel, dim3(B), dim3(64), 0, stream, obs, frames, trans, init, out,
                               reinterpret_cast<uint32_t *>(w.trellis), w.post[0], w.post[1], record, (int)ROUTE_SMALL, B, T, S, t_serial);
        }
        return hipGetLastError();
    });
}

// 65 .. 256 states: the value-only workgroup kernel + backtrace launches of their own (small_states.hpp, block_value_kernel)
inline int backtrace_segments(int items);
hipError_t launch_backtrace_on(const float *hist, const float *trans, const int32_t *frames, int32_t *out,
                               int B, int T, int S, hipStream_t stream, const int32_t *ranges, const int32_t *widest);
hipError_t launch_block(const float *obs, const int32_t *frames, const float *trans, const float *init, const Workspace &w,
                        int32_t *out, int32_t *record, int B, int T, int S, hipStream_t stream, int *launches, int cus) {
    const bool narrow = small::block_row_registers(S) == 48;
    if (launches) *launches += 2;
    const int NB = (S + 63) / 64;
    // (PQ, L): 2 or 3 splits with 48 or 64 row registers, 4 splits with 64
    const hipError_t e = by_value<2, 3, 4>(small::block_splits(S), [&](auto pq) { return by_flag(narrow, [&](auto narrow_) {
        constexpr int PQ = decltype(pq)::value, L = decltype(narrow_)::value && PQ < 4 ? 48 : 64;
        // two sequences per workgroup once the compute units are full without it: a 9- or 16-wave workgroup has a unit to
        // itself (512 x 500 x 256: 1.07 -> 1.03 ms, 2048 x 200 x 192: 1.33 -> 1.19), several 4-wave workgroups share one and
        // overlap anyway (512 x 500 x 128: 0.44 -> 0.64, but 4096 x 200 x 128: 0.95 -> 0.89).  TORBI_HIP_BLOCK_PAIRS=0 / 1 overrides
        const char *env = getenv("TORBI_HIP_BLOCK_PAIRS");
        return by_flag(env ? atoi(env) != 0 : B > cus * (NB * PQ >= 9 ? 1 : 8), [&](auto pairs) {
            constexpr int NSEQ = decltype(pairs)::value ? 2 : 1;
            auto *kernel = &small::block_value_kernel<PQ, L, NSEQ>;
            TORBI_NOTE_KERNEL("small::block_value_kernel<%d, %d, %d>", PQ, L, NSEQ);
            hipLaunchKernelGGL(kernel, dim3((B + NSEQ - 1) / NSEQ), dim3(64 * NB * PQ), 0, stream, obs, frames, trans, init,
                               reinterpret_cast<float *>(w.trellis), w.post[0], w.post[1], record, (int)ROUTE_SMALL, B, T, S, NB,
                               t_serial);
            return hipGetLastError();
        });
    }); });
    if (e != hipSuccess) return e;
    const float *hist = reinterpret_cast<const float *>(w.trellis);
    const bool vec = (S % 4 == 0) && ((reinterpret_cast<uintptr_t>(trans) & 15) == 0);
    const int K = (vec && w.arrive) ? std::min(backtrace_segments(B), 8) : 1;
    if (K > 1) {      // few paths: speculative segments (lazy_backtrace.hpp, chase_segment)
        hipLaunchKernelGGL(lazy::segment_rows_kernel<1>, dim3(B * K), dim3(64), 0, stream, hist, trans, frames, out, B, T, S, K,
                           w.arrive);
        hipLaunchKernelGGL(lazy::stitch_rows_kernel<1>, dim3(B), dim3(64), 0, stream, hist, trans, frames, out, B, T, S, K, w.arrive);
        return hipGetLastError();
    }
    return launch_backtrace_on(hist, trans, frames, out, B, T, S, stream, nullptr, nullptr);
}

// ---- dense path -----------------------------------------------------------------------
template <int BL, int JL, int NW, int KC, int MSL>
hipError_t launch_dense_steps(const float *obs, const int32_t *frames, const DenseWorkspace &w,
                              int B, int T, int S, hipStream_t stream, int *launches, unsigned *clock_out) {
    const dense::Plan &pl = w.plan;
    const size_t lds = dense::lds_bytes<BL, JL, NW, KC, MSL>();
    auto *kernel = &dense::step_dense_kernel<BL, JL, NW, KC, MSL>;
    hipError_t e = ensure_dynamic_lds(kernel, lds);
    if (e != hipSuccess) return e;
    TORBI_NOTE_KERNEL("dense::step_dense_kernel<%d, %d, %d, %d, %d>", BL, JL, NW, KC, MSL);
    const int ntiles = pl.n_bt * pl.n_jt;
    const int grid = 8 * ((ntiles + 7) / 8);
    int n = 0;
    for (int t = 1; t < T; ++t) {
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(64 * NW), lds, stream, obs, frames, w.trp, w.panel[(t - 1) & 1],
                           w.panel[t & 1], w.hist, w.chunks, B, T, S, t, pl.n_bt, pl.n_jt, pl.JT, pl.Kp, pl.NCH, pl.RB, clock_out);
        ++n;
    }
    if (launches) *launches = n;
    return hipGetLastError();
}

hipError_t launch_dense_forward(const float *obs, const int32_t *frames, const float *trans,
                                const float *init, const DenseWorkspace &w, int B, int T, int S,
                                hipStream_t stream, int *launches, bool reuse, unsigned *clock_out) {
    const dense::Plan &pl = w.plan;
    if (!reuse) {      // per-transition preparation: packed panels + per-tile lists of chunks that are not all -inf
        hipLaunchKernelGGL(dense::pack_transition_kernel, dim3((pl.Kp + 63) / 64, pl.n_jt), dim3(256), 0,
                           stream, trans, w.trp, S, pl.JT, pl.W, pl.Kp);
        hipLaunchKernelGGL(dense::build_chunk_lists_kernel, dim3(pl.n_jt), dim3(256),
                           sizeof(int) * (size_t)pl.NCH, stream, w.trp, w.chunks, S, pl.JT, pl.W, pl.Kp, pl.NCH,
                           pl.KC);
        // for the backtrace: the finite range of every row and the widest of them (lazy_backtrace.hpp)
        hipLaunchKernelGGL(stamp_route_kernel, dim3(1), dim3(1), 0, stream, w.widest, 0);
        hipLaunchKernelGGL(lazy::row_ranges_kernel, dim3(S), dim3(64), 0, stream, trans, w.ranges, w.widest, S);
    }
    {
        const size_t n = (size_t)pl.n_bt * pl.BT * pl.Kp;
        const int grid = (int)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
        hipLaunchKernelGGL(dense::init_panels_kernel, dim3(grid), dim3(256), 0, stream, obs, init,
                           w.panel[0], w.panel[1], w.hist, B, T, S, pl.n_bt, pl.BT, pl.Kp);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return by_value<6, 4, 2>(pl.JL, [&](auto jl) {
        constexpr int BL = 8, JL = decltype(jl)::value, NW = 8, KC = 12, MSL = 8;
        // (a plan no instance matches)
        if (pl.BL != BL || pl.JL != JL || pl.NW != NW || pl.KC != KC || pl.MSL != MSL) return hipErrorInvalidValue;
        return launch_dense_steps<BL, JL, NW, KC, MSL>(obs, frames, w, B, T, S, stream, launches, clock_out);
    });
}

// per-transition preparation shared by the pruned and the time-resident paths: descending rows with their
// prev-states as byte offsets into a [prev-state][items] posterior tile, block arrangement, transposed copy
void launch_list_preparation(const float *trans, float2 *sorted, int32_t *row_range, float *tt, int S, int SpP, int NPOW,
                             int items_per_tile, hipStream_t stream) {
    hipLaunchKernelGGL(pruned::sort_rows_kernel, dim3(S), dim3(256), sizeof(float) * 2 * (size_t)NPOW, stream, trans,
                       sorted, row_range, S, SpP, NPOW, items_per_tile * 4);
    if (items_per_tile == pruned::kNB) {
        const int n = (S / 4) * (SpP / pruned::kBlk);
        hipLaunchKernelGGL(pruned::arrange_blocks_kernel<4>, dim3((n + 63) / 64), dim3(64), 0, stream, sorted, S, SpP);
    } else {
        const int n = (S / 8) * (SpP / pruned::kBlk);
        hipLaunchKernelGGL(pruned::arrange_blocks_kernel<8>, dim3((n + 63) / 64), dim3(64), 0, stream, sorted, S, SpP);
    }
    hipLaunchKernelGGL(pruned::transpose_kernel, dim3((S + 31) / 32, (S + 31) / 32), dim3(256), 0, stream, trans, tt, S);
}

// (`ranges` / `widest`: the finite range of every transition row and the widest window, or null; with them a banded
// matrix is decoded by backtrace_ranged_kernel and the whole-row kernel returns at once -- decided on the device)
hipError_t launch_backtrace_on(const float *hist, const float *trans, const int32_t *frames, int32_t *out,
                               int B, int T, int S, hipStream_t stream, const int32_t *ranges = nullptr,
                               const int32_t *widest = nullptr) {
    const bool vec = (S % 4 == 0) && ((reinterpret_cast<uintptr_t>(trans) & 15) == 0);
    if (vec && S <= 256 * 16) {
        if (!ranges) widest = nullptr;
        // (three steps, no <8>: 1537 .. 2048 states take the <16> instances here)
        by_state_count<2, 6, 16>(S, [&](auto nq) {
            constexpr int NQ = decltype(nq)::value;
            if (ranges)
                hipLaunchKernelGGL(lazy::backtrace_ranged_kernel<NQ>, dim3(B), dim3(64), 0, stream, hist, trans, ranges,
                                   widest, frames, out, B, T, S);
            hipLaunchKernelGGL(lazy::backtrace_prefetch_kernel<NQ>, dim3(B), dim3(64), 0, stream, hist,
                               trans, frames, out, B, T, S, widest);
        });
        return hipGetLastError();
    }
    if (vec)
        hipLaunchKernelGGL(lazy::backtrace_kernel<4>, dim3(B), dim3(64), 0, stream, hist, trans,
                           frames, out, B, T, S);
    else
        hipLaunchKernelGGL(lazy::backtrace_kernel<1>, dim3(B), dim3(64), 0, stream, hist, trans,
                           frames, out, B, T, S);
    return hipGetLastError();
}

// backtrace over the SORTED transition rows the sorted-row scan prepared (lazy_backtrace.hpp): a path step reads 0.5-1 KB of
// list and the posteriors it points at instead of the posterior row + a whole transition row.  `rowmax`: the row maxima the
// forward pass left, which bound the walk down a list.
hipError_t launch_backtrace_sorted(const float *hist, const float2 *sorted, int SpP, int items_per_tile,
                                   const float *trans, const int32_t *frames, int32_t *out, int B, int T, int S,
                                   hipStream_t stream, const float *rowmax) {
    if (S % 4 != 0 || S > 256 * 16)
        return launch_backtrace_on(hist, trans, frames, out, B, T, S, stream);
    const int shift = items_per_tile == pruned::kNB ? 6 : 5;      // list offsets = prev-state * 4 * items per tile
    by_state_count(S, [&](auto nq) {
        hipLaunchKernelGGL(lazy::backtrace_gather_kernel<decltype(nq)::value>, dim3(B), dim3(64), 0, stream, hist, rowmax, sorted,
                           SpP, shift, frames, out, B, T, S);
    });
    return hipGetLastError();
}

// ---- time-resident path: several batches, one forward launch, one backtrace launch -------------------------
struct HostBatch {
    const float *obs;
    const int32_t *frames;
    int32_t *out;
    void *workspace;
    int B, T;
    int32_t *record;      // the workspace's route record (route_record: behind every layout)
};

// seeds per item of a time-resident launch (3, or 1: `few`) from the call's flags: FEW -> one, MANY -> three, neither -> one
// in the cluster form, three with whole tiles
inline bool few_seeds(unsigned flags, bool clusters) {
    if (flags & TORBI_HIP_FEW_SEEDS) return true;
    if (flags & TORBI_HIP_MANY_SEEDS) return false;
    return clusters;
}

// THE time-resident instance: one pointer for the LDS grant and the launch, one set of constants for the reported name.
// KR: seeds per item (3, or 1: `few`); NI: items per tile (16, 8 above 2048 states) -- both chosen once, in run_resident, for
// the forward launch and the repair launch behind a cluster launch (REPAIR: whole tiles, only where Group::only is set)
template <int KW, int MAXP, int KR, bool CLUSTER, int NI, bool REPAIR = false>
hipError_t launch_resident_kernel(const resident::Group &grp, const resident::Cluster &clu, int workgroups,
                                  const ResidentWorkspace &w, const float *init, int S, hipStream_t stream) {
    const size_t lds = resident::lds_bytes(S, KR + 1);
    auto *kernel = &resident::resident_forward_kernel<KW, MAXP, true, KR, CLUSTER, NI, REPAIR>;
    const hipError_t e = ensure_dynamic_lds(kernel, lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kernel, dim3(workgroups), dim3(64 * KW), lds, stream, grp, clu, w.tt, w.sorted, init, S, w.SpP);
    if (!REPAIR)
        TORBI_NOTE_KERNEL("resident::resident_forward_kernel<%d, %d, true, %d, %s, %d, false>", KW, MAXP, KR,
                          CLUSTER ? "true" : "false", NI);
    return hipGetLastError();
}

// waves per workgroup of the whole-tile, one-seed, 16-item instance at 73 .. 96 row groups (1153 .. 1536 states).  Twelve
// waves of eight passes hold 137 registers each, three to a SIMD; sixteen waves of six passes hold 111, FOUR to a SIMD, and
// still leave 64 of its 512 registers to the other stream's backtrace and preparation (resident_forward.hpp,
// "Item bases"): a launch group's forward pass 13.6 -> 13.1 ms at 8 x 512 x 200 x 1440 (HISTORY.md).  Taken where
// the launch's tiles fill more than half the compute units -- the condition under which AUTO picks whole tiles; launches of
// fewer tiles keep twelve waves.  Fifteen waves (up to 90 row groups: every wave six passes at 1440 states, three waves on
// one SIMD) measured between the two and are reachable through the switch only.
// TORBI_HIP_WHOLE_TILE_WAVES=12|15|16 names the instance whatever the tile count (read per launch: the tests switch it); a
// count that does not cover the launch's row groups is ignored, as is any for three seeds or 8-item tiles.
inline int whole_tile_waves(int nrg, int tiles, int cus) {
    constexpr int kFullWaves = 16;                 // where the tiles fill more than half the compute units
    if (nrg <= 72 || nrg > 96) return 12;
    int waves = 2 * tiles > cus ? kFullWaves : 12;
    if (const char *e = getenv("TORBI_HIP_WHOLE_TILE_WAVES")) {
        const int asked = atoi(e);
        if (asked == 12 || asked == 15 || asked == 16) waves = asked;
    }
    if (waves == 15 && nrg > 90) waves = 12;       // (fifteen waves x six passes)
    return waves;
}

// every workgroup owns a whole tile (resident_forward_kernel without clusters)
template <int KR, int NI>
hipError_t launch_whole_tiles(const resident::Group &grp, const resident::Cluster &clu, int tiles, const ResidentWorkspace &w,
                              const float *init, int S, int cus, hipStream_t s) {
    const int nrg = (S + resident::pass_rows(S) - 1) / resident::pass_rows(S);
    if constexpr (NI != resident::kNI) {       // 8-item tiles (2048 < S <= 4096)
        // (eight waves x 16 passes with 256 registers each measured slower than twelve x 8-11 at 168: 197 against 183 us per
        // timestep at 4096 states with a third of the units busy, equal on a full chip)
        if (nrg <= 96) return launch_resident_kernel<12, 8, KR, false, NI>(grp, clu, tiles, w, init, S, s);
        return launch_resident_kernel<12, 11, KR, false, NI>(grp, clu, tiles, w, init, S, s);
    } else {
        if (nrg <= 72) return launch_resident_kernel<12, 6, KR, false, NI>(grp, clu, tiles, w, init, S, s);
        if constexpr (KR == 1) {               // (three seeds spill at 128 registers: they stay on twelve waves)
            const int waves = whole_tile_waves(nrg, tiles, cus);
            if (waves == 16) return launch_resident_kernel<16, 6, KR, false, NI>(grp, clu, tiles, w, init, S, s);
            if (waves == 15) return launch_resident_kernel<15, 6, KR, false, NI>(grp, clu, tiles, w, init, S, s);
        }
        if (nrg <= 96) return launch_resident_kernel<12, 8, KR, false, NI>(grp, clu, tiles, w, init, S, s);
        return launch_resident_kernel<12, 11, KR, false, NI>(grp, clu, tiles, w, init, S, s);
    }
}

// segments per path of the backtrace behind a time-resident forward launch: 8 while the launch holds few paths (a wave per
// path leaves the chip idle and pays its steps' latency one after the other); 1 = whole paths, which a launch group's
// thousands of paths are walked as (bound by the bytes they move).  TORBI_HIP_BACKTRACE_SEGMENTS overrides (1 = off).
inline int backtrace_segments(int items) {
    const char *e = getenv("TORBI_HIP_BACKTRACE_SEGMENTS");         // (read per launch: the tests switch it)
    const int wanted = e ? atoi(e) : 8;
    if (wanted <= 1 || items > 1024) return 1;
    return std::max(2, std::min(wanted, 2048 / std::max(items, 1)));        // (items x K <= 2048 waves: 512 items -> 4)
}

// ---- NaN / +inf inputs (nonfinite.hpp): alarms raised with the decode's serial number, a repair launch behind the decode ----
// Ahead of a decode's forward launches: the matrix and the initial vector; the observations too for the routes whose
// forward kernels do not look at what they produce (a launch per timestep: generic, held, rows, dense).
inline hipError_t nonfinite_begin(const HostBatch *hb, int n, const float *trans, const float *init, int S, hipStream_t s,
                                  bool scan_observations, int reach_left = -1, int reach_right = -1, bool scan_matrix = true,
                                  float background = -INFINITY) {
    const int serial = new_serial();
    if (!scan_matrix) return hipSuccess;            // (the small-state kernels hold the whole matrix: they look themselves)
    nonfinite::Records recs{};
    recs.n = n;
    for (int k = 0; k < n; ++k) recs.record[k] = hb[k].record;
    const size_t cells = (size_t)S * S;
    hipLaunchKernelGGL(nonfinite::matrix_kernel, dim3((unsigned)std::max<size_t>(1, std::min<size_t>(1024, (cells + 2047) / 2048))),
                       dim3(256), 0, s, trans, init, S, recs, serial, reach_left, reach_right, background);
    if (scan_observations)
        for (int k = 0; k < n; ++k) {
            const size_t count = (size_t)hb[k].B * hb[k].T * S;
            hipLaunchKernelGGL(nonfinite::observation_kernel,
                               dim3((unsigned)std::max<size_t>(1, std::min<size_t>(2048, (count + 4095) / 4096))), dim3(256), 0, s,
                               hb[k].obs, count, recs.record[k], serial);
        }
    return hipGetLastError();
}
// Behind the decode's backtrace: does nothing unless an alarm carries this decode's serial number.
inline hipError_t nonfinite_end(const HostBatch *hb, int n, const float *trans, const float *init, int S, hipStream_t s) {
    nonfinite::RepairJobs jobs{};
    jobs.n = n;
    int items = 0;
    for (int k = 0; k < n; ++k) {
        jobs.obs[k] = hb[k].obs;
        jobs.frames[k] = hb[k].frames;
        jobs.out[k] = hb[k].out;
        jobs.trellis[k] = static_cast<int32_t *>(hb[k].workspace);
        jobs.record[k] = hb[k].record;
        jobs.rows[k] = reinterpret_cast<float *>(reinterpret_cast<char *>(jobs.record[k]) + 256);
        jobs.B[k] = hb[k].B;
        jobs.T[k] = hb[k].T;
        jobs.item0[k] = items;
        items += hb[k].B;
    }
    hipLaunchKernelGGL(nonfinite::repair_kernel, dim3(items), dim3(256), 0, s, jobs, trans, init, S, t_serial);
    return hipGetLastError();
}

// how long the members of a cluster (time-resident and band forms) wait for each other before they give their tile up, in
// ticks of the 100 MHz wall clock.  TORBI_HIP_CLUSTER_WAIT_US overrides (read per launch: the tests switch it).
inline unsigned long long cluster_wait_ticks() {
    const char *e = getenv("TORBI_HIP_CLUSTER_WAIT_US");
    return e ? 100ull * strtoull(e, nullptr, 10) : resident::kClusterWaitTicks;
}

// A table of batches (B > 0 each) as ONE launch group, ready for a forward launch over its tiles: `grp` filled from the
// time-resident layout of every batch's workspace (tile map and statistics in the first batch's), and on the stream the
// launches that rank every batch's items by length, cut them into tiles of `items_per_tile` and rank the tiles -- the first of
// which stamps `route` into every batch's route record, the last of which zeroes the `nflags` cluster words at `flags`.
// Behind a nonfinite_begin (the group carries that decode's serial number).
struct LaunchGroup {
    resident::Group grp;
    int tiles, items;
};
hipError_t assemble_group(const HostBatch *hb, int n, int S, int cus, hipStream_t s, bool ascending, int items_per_tile,
                          Route route, unsigned *flags, int nflags, LaunchGroup &g) {
    resident::Group &grp = g.grp;
    resident::OrderJobs jobs{};
    grp = resident::Group{};
    grp.n = n;
    grp.serial = t_serial;
    int tiles = 0, items = 0, widest = 0;
    for (int k = 0; k < n; ++k) {
        resident::Batch &b = grp.batch[k];
        const ResidentWorkspace wk = carve_resident(hb[k].workspace, hb[k].B, hb[k].T, S, cus);
        b.alarm = hb[k].record + nonfinite::kAlarmWord;
        b.obs = hb[k].obs;
        b.frames = hb[k].frames;
        b.out = hb[k].out;
        b.hist = wk.hist;
        b.order = wk.order;
        b.rowmax = wk.rowmax;
        jobs.job[k] = resident::OrderJob{hb[k].frames, wk.order, hb[k].B, hb[k].T, tiles, wk.lengths_hist, hb[k].record, (int)route};
        widest = std::max(widest, hb[k].B);
        b.B = hb[k].B;
        b.T = hb[k].T;
        b.tile0 = tiles;
        b.item0 = items;
        tiles += (hb[k].B + items_per_tile - 1) / items_per_tile;
        items += hb[k].B;
    }
    if (tiles > kMaxGroupTiles) return hipErrorInvalidValue;
    g.tiles = tiles;
    g.items = items;
    const ResidentWorkspace w = carve_resident(hb[0].workspace, hb[0].B, hb[0].T, S, cus);
    grp.tile_map = w.tile_map;
    grp.stats = w.stats;
    jobs.ascending = ascending ? 1 : 0;
    jobs.stats = w.stats;
    jobs.n = n;
    jobs.tiles = tiles;
    jobs.tile_map = w.tile_map;
    jobs.ni = items_per_tile;
    jobs.flags = flags;
    jobs.nflags = nflags;
    hipLaunchKernelGGL(resident::order_items_kernel, dim3((widest + 255) / 256, n), dim3(256), 0, s, jobs);
    for (int k = 0; k < n; ++k) {            // batches too large for the all-pairs ranking: counting sort over the lengths
        const resident::OrderJob &jb = jobs.job[k];
        if (jb.B <= resident::kMaxOrdered) continue;
        const ResidentWorkspace wk = carve_resident(hb[k].workspace, hb[k].B, hb[k].T, S, cus);
        hipError_t me = hipMemsetAsync(wk.lengths_hist, 0, wk.lengths_hist_bytes, s);
        if (me != hipSuccess) return me;
        hipLaunchKernelGGL(resident::order_large_count_kernel, dim3((jb.B + 255) / 256), dim3(256), 0, s, jb);
        hipLaunchKernelGGL(resident::order_large_scan_kernel, dim3(1), dim3(1024), 0, s, jb, jobs.ascending);
        hipLaunchKernelGGL(resident::order_large_place_kernel, dim3((jb.B + 255) / 256), dim3(256), 0, s, jb);
    }
    hipLaunchKernelGGL(resident::order_tiles_kernel, dim3((tiles + 255) / 256), dim3(256), 0, s, jobs);
    return hipSuccess;
}

// batches with B > 0 only; the preparation lives in the first batch's workspace, or in `kept` (marked valid once this call
// has enqueued its filling)
hipError_t run_resident(const HostBatch *hb, int n, const float *trans, const float *init, int S, int cus, hipStream_t s,
                        hipEvent_t *ev, int *launches, bool reuse, bool ascending, bool clusters, bool few,
                        Preparation *kept) {
    {
        const hipError_t ne = nonfinite_begin(hb, n, trans, init, S, s, false);
        if (ne != hipSuccess) return ne;
    }
    int tiles = 0;
    for (int k = 0; k < n; ++k) tiles += tiles_of(hb[k].B, S);
    const ResidentWorkspace w = carve_resident(hb[0].workspace, hb[0].B, hb[0].T, S, cus, kept);
    // cluster form: R workgroups per tile (exchange buffers in the first batch's workspace, flags and tickets zeroed)
    const int R = clusters ? cluster_members(tiles, S, cus) : 1;
    // Above 2048 states (8-item tiles) the sorted lists are what the launch fetches -- 134 MB at 4096 states, far beyond an
    // XCD's 4 MB L2, walked by every tile: 232 GB per 128 x 2000 x 4096 decode against 8.4 GB algorithmic
    // (profiles/r06_c5_pmc.json).  Member m of EVERY tile on one XCD keeps that member's rows' lists in its L2; the exchange
    // then crosses XCDs (write-through), which costs less than it saves there: 19.8 -> 17.3 us per timestep at 128 items,
    // 34.3 -> 30.6 at 256; up to 2048 states it loses 1-3 % (profiles/r06_c5_spread.txt).
    const int spread = (R % 8 == 0 && resident::tile_items(S) == 8) ? 1 : 0;
    resident::Cluster clu{w.xchg, w.where, tiles, w.control, w.failed, R, cluster_wait_ticks(), spread};
    if (ev) (void)hipEventRecord(ev[0], s);
    if (kept) reuse = kept->valid;       // the caller's buffer: the promise is about IT, whichever batch
    if (!reuse) launch_list_preparation(trans, w.sorted, w.row_range, w.tt, S, w.SpP, w.NPOW, resident::tile_items(S), s);
    if (kept) kept->valid = true;
    LaunchGroup group;
    hipError_t e = assemble_group(hb, n, S, cus, s, ascending, resident::tile_items(S), R > 1 ? ROUTE_CLUSTER : ROUTE_RESIDENT,
                                  w.flags, R > 1 ? w.nflags : 0, group);
    if (e != hipSuccess) return e;
    const resident::Group &grp = group.grp;
    const int items = group.items;
    if (ev) (void)hipEventRecord(ev[3], s);
    const int nrg = (S + resident::pass_rows(S) - 1) / resident::pass_rows(S);
    const bool small = resident::tile_items(S) != resident::kNI;       // 8-item tiles (2048 < S <= 4096)
    e = by_flag(few, [&](auto few_) { return by_flag(small, [&](auto small_) {
        constexpr int KR = decltype(few_)::value ? 1 : 3, NI = decltype(small_)::value ? 8 : resident::kNI;
        if (R <= 1) return launch_whole_tiles<KR, NI>(grp, clu, tiles, w, init, S, cus, s);
        {       // the slots this launch uses start out absent (resident_forward.hpp, cluster_slot_bytes)
            const size_t granules = (size_t)tiles * resident::kSlots * resident::cluster_slot_bytes(S) / 16;
            hipLaunchKernelGGL(resident::absent_kernel, dim3((unsigned)std::min<size_t>((granules + 255) / 256, 2048)), dim3(256),
                               0, s, reinterpret_cast<uint4 *>(w.xchg), granules);
        }
        const int passes = ((nrg + R - 1) / R + 11) / 12;       // row groups of the largest share over 12 waves
        // (eight dispatch classes of R x ceil(tiles / 8) workgroups each: resident_forward.hpp, struct Cluster)
        const int grid = 8 * ((tiles + 7) / 8) * R;
        const int share = (nrg + R - 1) / R;                    // row groups of the largest share
        hipError_t ce;
        if constexpr (NI == 8) {
            // 8-item tiles, at most 16 row groups a member: EIGHT waves (256 registers each: the twelve-wave instances of
            // the 8-item tile spill 20-80 registers at 168, and every scratch reload waits for the write-through stores
            // ahead of it); 128 x 4096 (16 tiles x 16 members, 8 row groups each) kept four of twelve waves idle anyway
            if (share <= 8) ce = launch_resident_kernel<8, 1, KR, true, NI>(grp, clu, grid, w, init, S, s);
            else if (share <= 16) ce = launch_resident_kernel<8, 2, KR, true, NI>(grp, clu, grid, w, init, S, s);
            // (more than 16 row groups a member: at least two passes of twelve waves)
            else if (passes <= 2) ce = launch_resident_kernel<12, 2, KR, true, NI>(grp, clu, grid, w, init, S, s);
            else if (passes <= 4) ce = launch_resident_kernel<12, 4, KR, true, NI>(grp, clu, grid, w, init, S, s);
            else ce = launch_resident_kernel<12, 6, KR, true, NI>(grp, clu, grid, w, init, S, s);
        } else if (passes <= 1) ce = launch_resident_kernel<12, 1, KR, true, NI>(grp, clu, grid, w, init, S, s);
        else if (passes <= 2) ce = launch_resident_kernel<12, 2, KR, true, NI>(grp, clu, grid, w, init, S, s);
        else if (passes <= 4) ce = launch_resident_kernel<12, 4, KR, true, NI>(grp, clu, grid, w, init, S, s);
        else ce = launch_resident_kernel<12, 6, KR, true, NI>(grp, clu, grid, w, init, S, s);
        if (ce != hipSuccess) return ce;
        // a cluster that could not complete in time (resident_forward.hpp: CLUSTER_WAIT_TICKS) has flagged its tile: the
        // launch behind decodes those tiles again, whole -- it returns at once wherever nothing was flagged (every run so far);
        // ONE instance per seed count and tile size (eleven passes cover every supported state count)
        resident::Group again = grp;
        again.only = clu.failed;
        return launch_resident_kernel<12, 11, KR, false, NI, true>(again, clu, tiles, w, init, S, s);
    }); });
    if (launches) *launches = 1;
    if (ev) (void)hipEventRecord(ev[1], s);
    if (e != hipSuccess) return e;
    // the backtrace gathers the posteriors the lists point at instead of staging whole rows in the LDS: half the bytes, and
    // faster from one batch (0.58 against 0.80 ms) to eight (1.86 against 3.11 ms; profiles/r03_backtrace_gather.txt).
    // few paths (one batch): every path in speculative segments, K waves per item, then one wave per item at the joints
    // (lazy_backtrace.hpp, chase_segment); the forward launch is done with the tile map, which holds the segments' ends
    const int K = backtrace_segments(items);
    if (S % 4 == 0 && K > 1) {
        int32_t *const arrive = w.tile_map;
        by_state_count(S, [&](auto nq) {
            constexpr int NQ = decltype(nq)::value;
            hipLaunchKernelGGL(resident::group_segment_gather_kernel<NQ>, dim3(items * K), dim3(64), 0, s, grp, w.sorted, w.SpP, S, K,
                               arrive);
            hipLaunchKernelGGL(resident::group_stitch_gather_kernel<NQ>, dim3(items), dim3(64), 0, s, grp, w.sorted, w.SpP, S, K, arrive);
        });
    } else if (S % 4 == 0) {
        by_state_count(S, [&](auto nq) {
            hipLaunchKernelGGL(resident::group_backtrace_gather_kernel<decltype(nq)::value>, dim3(items), dim3(64), 0, s, grp, w.sorted,
                               w.SpP, S);
        });
    } else
        hipLaunchKernelGGL(resident::group_backtrace_kernel<1>, dim3(items), dim3(64), 0, s, grp, trans, S);
    {
        const hipError_t ne = nonfinite_end(hb, n, trans, init, S, s);
        if (ne != hipSuccess) return ne;
    }
    if (ev) (void)hipEventRecord(ev[2], s);
    return hipGetLastError();
}


// ---- band route: several batches, one forward launch (band_forward.hpp), one backtrace launch ------------------------
inline int band_tiles(int B) { return (B + band::kNI - 1) / band::kNI; }

// batches with B > 0 only; tile map, statistics, tickets and give-up flags live in the first batch's workspace
// The one value outside a band: neither NaN nor +inf; the forward-backward kernels read its exp (0 for -inf).
static bool background_ok(float background) { return background == background && background != INFINITY; }
static float exp_background(float background) { return background == -INFINITY ? 0.f : expf(background); }

// What the band route does with a launch group: whole tiles (band_tile_forward.hpp: one workgroup per tile, once the group
// has a tile for at least every other compute unit) or tiles split over R members (band_forward.hpp), `cap` tiles per
// launch -- every member of a launch resident at once, because they wait for each other inside it.
struct BandChoice {
    band::Plan pl;          // split form (pl.R members per tile); whole tiles: S, hl, hr and R = 1 only
    band::TilePlan tile;
    bool whole;
    int cap;                // tiles per launch (split form)
    float background;      // every entry outside the band: -inf, or ONE constant (whole tiles only: band_tile_forward.hpp)
};
inline bool choose_band(int S, int hl, int hr, int tiles, int cus, BandChoice &c, float background = -INFINITY) {
    c = BandChoice{};
    c.background = background;
    if (tiles < 1 || !background_ok(background)) return false;
    const char *force = getenv("TORBI_HIP_BAND_FORM");            // experiments: "tile" / "split"
    const char *tw = getenv("TORBI_HIP_TILE_WAVES");              // experiments: 8 / 12 waves per workgroup
    const bool tile_ok = band::make_tile_plan(S, hl, hr, c.tile, tw ? atoi(tw) : 0) && !(force && force[0] == 's');
    // Whole tiles need a tile for (almost) every compute unit to pay: a whole-tile timestep takes ~5 x a split one (36 against
    // 7.4 us at 1440 states, reach 87) whatever the tile count, a split launch decodes 32 tiles at a time.  Measured, -inf
    // band, launch groups of 512-item batches (tools/pitch_tiny_probe.py): 4 batches = 128 tiles 56 M whole against 67 M split,
    // 8 batches 109 M against 72 M; the rates cross near 157 tiles.  Where there is no split form (a constant outside the band;
    // reaches or state counts it does not cover) the alternative is the cluster form (34-40 M): whole tiles from half the units up.
    band::Plan split{};
    const bool split_ok = !(force && force[0] == 't' && tile_ok) && band::make_plan(S, hl, hr, tiles, cus, split, background) &&
                          band::tiles_per_launch(split, cus) >= 1;
    // (a split launch decodes `per` tiles in ~1.6 / R of a whole-tile timestep: whole tiles once the split launches of the group
    // add up to more -- 8 * launches >= 5 * R, which is 8 * tiles >= 5 * CUs for groups that fill their launches)
    const int per = split_ok ? std::max(1, std::min(band::tiles_per_launch(split, cus), kMaxGroupTiles)) : 1;
    const bool enough = split_ok ? 8 * ((tiles + per - 1) / per) >= 5 * split.R : 2 * tiles >= cus;
    if (tile_ok && (enough || (force && force[0] == 't'))) {
        c.whole = true;
        c.pl.S = S; c.pl.hl = hl; c.pl.hr = hr; c.pl.R = 1;
        c.cap = tiles;
        c.tile.background = background;
        return true;
    }
    if (!split_ok) return false;
    c.pl = split;
    c.cap = std::min(band::tiles_per_launch(c.pl, cus), kMaxGroupTiles);
    return true;
}

hipError_t run_band(const HostBatch *hb, int n, const float *trans, const float *init, int S, const BandChoice &choice, int cus,
                    hipStream_t s, hipEvent_t *ev, int *launches, bool ascending) {
    const band::Plan &pl = choice.pl;
    band::Exchange ex{};
    band::ClearJobs clear{};
    {
        const hipError_t ne = nonfinite_begin(hb, n, trans, init, S, s, false, pl.hl, pl.hr, true, choice.background);     // (and the band's promise)
        if (ne != hipSuccess) return ne;
    }
    size_t most = 0;
    for (int k = 0; k < n; ++k) {
        const BandWorkspace wk = carve_band(hb[k].workspace, hb[k].B, hb[k].T, S, cus);
        ex.xchg[k] = wk.xchg;
        clear.xchg[k] = wk.xchg;
        clear.bytes[k] = pl.R > 1 && !choice.whole ? band::xchg_bytes(hb[k].B, S) : 0;      // (whole tiles exchange nothing)
        most = std::max(most, clear.bytes[k]);
    }
    const BandWorkspace w = carve_band(hb[0].workspace, hb[0].B, hb[0].T, S, cus);
    if (ev) (void)hipEventRecord(ev[0], s);
    LaunchGroup group;
    hipError_t e = assemble_group(hb, n, S, cus, s, ascending, band::kNI, ROUTE_BAND, nullptr, 0, group);
    if (e != hipSuccess) return e;
    const resident::Group &grp = group.grp;
    const int tiles = group.tiles, items = group.items;
    const int nlaunch = choice.whole ? 1 : (tiles + choice.cap - 1) / choice.cap;
    ex.failed = w.failed;
    ex.wait_ticks = cluster_wait_ticks();
    clear.words = w.words;
    clear.nwords = 16 + kMaxGroupTiles + 8 * nlaunch;
    clear.n = n;
    if (choice.whole) {
        // whole tiles: the band packed in the lanes' reading order (1 MB at 1440 states, reach 87: ~10 us), then ONE launch
        const band::TilePlan &tp = choice.tile;
        hipLaunchKernelGGL(band::pack_band_kernel, dim3(tp.nblk * tp.Dq4), dim3(64), 0, s, trans, w.tpack, S, tp.hl, tp.hr, tp.Dq,
                           tp.Dq4);
        if (ev) (void)hipEventRecord(ev[3], s);
        // (bpw, waves of the instance): (1, 12), (2, 12), (2, 8), (3, 8) -- a workgroup of twelve waves holds at most two blocks a
        // wave (make_tile_plan), and one block a wave runs the twelve-wave instance whatever the workgroup's size
        e = by_value<1, 2, 3>(tp.bpw, [&](auto bpw) { return by_flag(tp.waves == 12, [&](auto twelve) {
            return by_flag(tp.background != -INFINITY, [&](auto bg) {
                constexpr int BPW = decltype(bpw)::value, NW = BPW == 1 || (BPW == 2 && decltype(twelve)::value) ? 12 : 8;
                constexpr bool BG = decltype(bg)::value;
                auto *kernel = &band::band_tile_kernel<BPW, NW, BG>;
                const hipError_t le = ensure_dynamic_lds(kernel, (size_t)tp.lds_bytes);
                if (le != hipSuccess) return le;
                TORBI_NOTE_KERNEL("band::band_tile_kernel<%d, %d, %s>", BPW, NW, BG ? "true" : "false");
                hipLaunchKernelGGL(kernel, dim3(tiles), dim3(64 * tp.waves), (size_t)tp.lds_bytes, s, grp, tp, w.tpack, init);
                return hipSuccess;
            });
        }); });
        if (e != hipSuccess) return e;
    } else {
        {
            const size_t blocks = std::max<size_t>(1, std::min<size_t>(2048, (most / 16 + 255) / 256));
            hipLaunchKernelGGL(band::clear_exchange_kernel, dim3((unsigned)blocks, n), dim3(256), 0, s, clear);
        }
        if (ev) (void)hipEventRecord(ev[3], s);
        e = by_flag(choice.background != -INFINITY, [&](auto bg) {
            constexpr bool BG = decltype(bg)::value;
            auto *kernel = &band::band_forward_kernel<BG>;
            const hipError_t le = ensure_dynamic_lds(kernel, (size_t)pl.lds_bytes);
            if (le != hipSuccess) return le;
            TORBI_NOTE_KERNEL("band::band_forward_kernel<%s>", BG ? "true" : "false");
            // (R > 1: eight dispatch classes of R x ceil(tiles / 8) workgroups each -- band_forward.hpp, membership; a launch
            // never holds more members than one XCD has units for its class: choose_band)
            for (int l = 0; l < nlaunch; ++l) {
                ex.tile0 = l * choice.cap;
                ex.tiles = std::min(tiles, ex.tile0 + choice.cap);
                ex.control = w.tickets + 8 * l;
                const int here = ex.tiles - ex.tile0;
                const int grid = pl.R > 1 ? 8 * ((here + 7) / 8) * pl.R : here;
                hipLaunchKernelGGL(kernel, dim3(grid), dim3(64 * pl.waves), (size_t)pl.lds_bytes, s, grp, ex, pl, trans, init);
            }
            return hipSuccess;
        });
        if (e != hipSuccess) return e;
        if (pl.R > 1) {          // does nothing unless a member gave up waiting (band_forward.hpp)
            const size_t lds = 32 * (size_t)S;
            e = ensure_dynamic_lds(&band::band_repair_kernel, lds);
            if (e != hipSuccess) return e;
            hipLaunchKernelGGL(band::band_repair_kernel, dim3(tiles), dim3(1024), lds, s, grp, ex.failed, trans, init, S, pl.hl,
                               pl.hr, choice.background);
        }
    }
    if (launches) *launches = nlaunch;
    if (ev) (void)hipEventRecord(ev[1], s);
    const int K = backtrace_segments(items);          // (few paths: speculative segments, as behind run_resident)
    int32_t *const arrive = w.base.tile_map;
    by_state_count(S, [&](auto nq) {
        constexpr int NQ = decltype(nq)::value;
        if (K > 1) {
            hipLaunchKernelGGL(band::group_segment_band_kernel<NQ>, dim3(items * K), dim3(64), 0, s, grp, trans, S, pl.hl, pl.hr, K,
                               arrive, choice.background);
            hipLaunchKernelGGL(band::group_stitch_band_kernel<NQ>, dim3(items), dim3(64), 0, s, grp, trans, S, pl.hl, pl.hr, K, arrive,
                               choice.background);
        } else {
            hipLaunchKernelGGL(band::group_backtrace_band_kernel<NQ>, dim3(items), dim3(64), 0, s, grp, trans, S, pl.hl, pl.hr,
                               choice.background);
        }
    });
    {
        const hipError_t ne = nonfinite_end(hb, n, trans, init, S, s);
        if (ne != hipSuccess) return ne;
    }
    if (ev) (void)hipEventRecord(ev[2], s);
    return hipGetLastError();
}

// AUTO takes the band kernel for a promised band when its plan covers the group -- except for shapes a wavefront or a
// workgroup decodes alone (small_states.hpp) and for the handful of sequences of the held-matrix kernel
inline bool band_plan_for(const HostBatch *hb, int n, int S, int hl, int hr, int cus, int path, BandChoice &pl,
                          float background = -INFINITY) {
    if (path != TORBI_HIP_FORWARD_AUTO && path != TORBI_HIP_FORWARD_BAND) return false;
    if (!band_shape(S)) return false;
    int tiles = 0;
    long long items = 0;
    for (int k = 0; k < n; ++k) tiles += band_tiles(hb[k].B), items += hb[k].B;
    if (tiles < 1 || tiles > kMaxGroupTiles) return false;
    if (path == TORBI_HIP_FORWARD_AUTO) {
        if (small::supported(S) || small_block_auto((int)std::min(items, 1ll << 30), S, cus)) return false;
        if (n == 1 && held::supported(hb[0].B, S, cus) && held_auto(hb[0].B, S)) return false;
    }
    return choose_band(S, hl, hr, tiles, cus, pl, background);
}

// one decode on `s`; optional events bracket the forward and backtrace phases (ev[3]: end of the preparation).
// `kept`: the caller's preparation buffer, which only the time-resident routes use
hipError_t run_decode(const HostBatch &hb, const float *trans, const float *init, int S, int device, hipStream_t s,
                      hipEvent_t *ev, int *launches, bool reuse, int path, unsigned seed_flags, Route *taken,
                      Preparation *kept) {
    const float *const obs = hb.obs;
    const int32_t *const frames = hb.frames;
    int32_t *const out = hb.out;
    void *const workspace = hb.workspace;
    const int B = hb.B, T = hb.T;
    hipError_t e;
    const int cus = cu_count(device);
    Route route = route_for(path, B, S, cus);
    // AUTO keeps away from the held-matrix kernel while another stream of the device is busy (see mark_decode_end)
    if (route == ROUTE_HELD && path == TORBI_HIP_FORWARD_AUTO && other_streams_busy(device, s))
        route = route_for(path, B, S, cus, false);
    // ... and, named or not, from a launch the device cannot hold as a whole (occupancy of this very kernel)
    if (route == ROUTE_HELD && !held_resident(S, device, cus))
        route = route_for(path == TORBI_HIP_FORWARD_HELD ? TORBI_HIP_FORWARD_AUTO : path, B, S, cus, false);
    if (taken) *taken = route;
    if (route == ROUTE_RESIDENT || route == ROUTE_CLUSTER)
        return run_resident(&hb, 1, trans, init, S, cus, s, ev, launches, reuse, false, route == ROUTE_CLUSTER,
                            few_seeds(seed_flags, route == ROUTE_CLUSTER), kept);
    if (kept) reuse = false;       // (the promise was about the caller's buffer; this route prepares in the workspace)
    if (ev) (void)hipEventRecord(ev[0], s);
    if (ev) (void)hipEventRecord(ev[3], s);
    // NaN / +inf inputs (nonfinite.hpp): the small-state kernels look at the values they produce; the routes below get
    // their observations looked at by a launch of its own (they launch a kernel per timestep anyway)
    e = nonfinite_begin(&hb, 1, trans, init, S, s, route != ROUTE_SMALL, -1, -1, route != ROUTE_SMALL);
    if (e != hipSuccess) return e;
    if (route == ROUTE_SMALL) {             // one launch: recurrence, backtrace and the route record
        // (the byte plane lies where the generic path's trellis does and is never larger: small_states.hpp)
        // (and so does the value-only form's fp32 history: the trellis region itself)
        const Workspace w = carve(workspace, B, T, S);
        e = small::supported(S) ? launch_small(obs, frames, trans, init, w, out, hb.record, B, T, S, s, launches, cus)
                                : launch_block(obs, frames, trans, init, w, out, hb.record, B, T, S, s, launches, cus);
        if (ev) (void)hipEventRecord(ev[1], s);
        if (e == hipSuccess) e = nonfinite_end(&hb, 1, trans, init, S, s);
        if (ev) (void)hipEventRecord(ev[2], s);
        return e;
    }
    e = stamp_route(hb.record, route, s);
    if (e != hipSuccess) return e;
    if (route == ROUTE_DENSE) {
        const DenseWorkspace w = carve_dense(workspace, B, T, S, cus);
        // (the route record's words [2], [3]: shader-clock and wall-clock ticks of the last timestep's workgroup 0)
        e = launch_dense_forward(obs, frames, trans, init, w, B, T, S, s, launches, reuse,
                                 reinterpret_cast<unsigned *>(hb.record) + 2);
        if (ev) (void)hipEventRecord(ev[1], s);
        if (e == hipSuccess)
            e = launch_backtrace_on(w.hist, trans, frames, out, B, T, S, s, w.ranges, w.widest);
    } else if (route == ROUTE_ROWS) {
        TORBI_NOTE_KERNEL("rowscan::step_rows_sorted_kernel");
        const RowsWorkspace w = carve_rows(workspace, B, T, S);
        if (!reuse)       // per-transition preparation: descending rows, prev-states as byte offsets of a 16-item tile row
            hipLaunchKernelGGL(pruned::sort_rows_kernel, dim3(S), dim3(256), sizeof(float) * 2 * (size_t)w.NPOW, s, trans,
                               w.sorted, w.row_range, S, w.SpP, w.NPOW, pruned::kNB * 4);
        {
            const size_t n = (size_t)B * S;
            const int grid = (int)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
            hipLaunchKernelGGL(pruned::init_history_kernel, dim3(grid), dim3(256), 0, s, obs, init, w.hist, B, T, S);
        }
        int n = 0;
        for (int t = 1; t < T; ++t, ++n)
            hipLaunchKernelGGL(rowscan::step_rows_sorted_kernel,
                               dim3((S + rowscan::kRowsPerBlock - 1) / rowscan::kRowsPerBlock, B), dim3(256),
                               sizeof(float) * (size_t)S, s, obs, frames, w.sorted, w.hist, w.rowmax, B, T, S, t, w.SpP, 6);
        if (launches) *launches = n;
        e = hipGetLastError();
        if (ev) (void)hipEventRecord(ev[1], s);
        if (e == hipSuccess)
            e = launch_backtrace_sorted(w.hist, w.sorted, w.SpP, pruned::kNB, trans, frames, out, B, T, S, s, w.rowmax);
    } else {
        const Workspace w = carve(workspace, B, T, S);
        TORBI_NOTE_KERNEL(route == ROUTE_HELD ? "held::held_forward_kernel" : "step_rows_kernel / step_rows4_kernel");
        e = route == ROUTE_HELD ? launch_held_forward(obs, frames, trans, init, w, B, T, S, s, launches)
                                : launch_forward(obs, frames, trans, init, w, B, T, S, s, launches);
        if (ev) (void)hipEventRecord(ev[1], s);
        if (e == hipSuccess) e = launch_finalize(frames, w, out, B, T, S, s);
    }
    if (e == hipSuccess) e = nonfinite_end(&hb, 1, trans, init, S, s);
    if (ev) (void)hipEventRecord(ev[2], s);
    return e;
}

// the four events of a profiled call; of a call that asks for no phases none is created and nothing synchronises
struct PhaseEvents {
    hipEvent_t ev[4] = {};
    hipError_t err = hipSuccess;
    const bool wanted;
    explicit PhaseEvents(bool wanted_) : wanted(wanted_) {
        for (auto &x : ev)
            if (wanted && err == hipSuccess) err = hipEventCreate(&x);
    }
    ~PhaseEvents() {
        for (auto &x : ev)
            if (x) (void)hipEventDestroy(x);
    }
    hipEvent_t *events() { return wanted ? ev : nullptr; }
    // forward (incl. preparation), argmax + backtrace, preparation alone -- after synchronising on the last event
    hipError_t read(float *phase_ms) {
        hipError_t e = hipEventSynchronize(ev[2]);
        if (e != hipSuccess) return e;
        (void)hipEventElapsedTime(&phase_ms[0], ev[0], ev[1]);
        (void)hipEventElapsedTime(&phase_ms[1], ev[1], ev[2]);
        (void)hipEventElapsedTime(&phase_ms[4], ev[0], ev[3]);
        return hipSuccess;
    }
};

// ---- the ONE way from a Viterbi decode entry point with a transition matrix to the kernels ---------------------------
struct BandPromise { int reach_left, reach_right; float background; };
struct DecodeCall {             // everything of a call that is not a batch
    const float *transition, *initial;
    int S, device;
    void *stream;
    unsigned flags;
    float *phase_ms;            // null: no events are created, nothing synchronises
    const BandPromise *band;    // null, or what the caller promises about the matrix (torbi_hip_viterbi_decode_banded_over)
    Preparation *preparation;   // null, or the caller-kept buffer (torbi_hip_viterbi_decode_batches_prepared)
};

// the entry points that take a batch table turn a missing table or model down before they look at any batch (an empty
// batch of torbi_hip_viterbi_decode_ex needs neither)
inline bool table_given(const torbi_hip_batch *batches, int count, const float *transition, const float *initial) {
    return count == 0 || (batches && transition && initial);
}

int decode_group(const torbi_hip_batch *batches, int count, const DecodeCall &call) {
    const float *const transition = call.transition, *const initial = call.initial;
    const int S = call.S, device = call.device;
    const unsigned flags = call.flags;
    float *const phase_ms = call.phase_ms;
    if (!flags_ok(flags) || count < 0 || count > TORBI_HIP_MAX_BATCHES || S < 1) return TORBI_HIP_EINVAL;
    if (count == 0) return TORBI_HIP_OK;
    if (!batches) return TORBI_HIP_EINVAL;
    if (phase_ms)
        for (int i = 0; i < 6; ++i) phase_ms[i] = 0.0f;
    const int cus = cu_count(device);
    HostBatch hb[TORBI_HIP_MAX_BATCHES];
    int n = 0, tiles = 0;
    for (int k = 0; k < count; ++k) {
        const torbi_hip_batch &b = batches[k];
        const int rc = check_args(b.observation, b.batch_frames, transition, initial, b.indices_out, b.workspace,
                                  b.workspace_bytes, b.B, b.T, S, device);
        if (rc != TORBI_HIP_OK) return rc;
        if (b.B == 0) continue;
        hb[n++] = HostBatch{b.observation, b.batch_frames, b.indices_out, b.workspace, b.B, b.T,
                            route_record(b.workspace, b.B, b.T, S, cus)};
        tiles += tiles_of(b.B, S);
    }
    if (n == 0) return TORBI_HIP_OK;
    DeviceGuard guard(device);
    if (guard.err != hipSuccess) return (int)guard.err;
    hipStream_t s = static_cast<hipStream_t>(call.stream);
    int path = requested_path(flags);
    // a promised band: the band kernel when its plan covers the group, else whatever the call does without the promise
    // (BAND named: as AUTO)
    BandChoice band_choice;
    bool banded = false;
    if (call.band) {
        bool vec = (reinterpret_cast<uintptr_t>(transition) & 15) == 0;       // (16-byte reads of matrix rows and observation rows)
        for (int k = 0; k < n; ++k) vec = vec && (reinterpret_cast<uintptr_t>(hb[k].obs) & 15) == 0;
        banded = vec && band_plan_for(hb, n, S, call.band->reach_left, call.band->reach_right, cus, path, band_choice,
                                      call.band->background);
        if (!banded && path == TORBI_HIP_FORWARD_BAND) path = TORBI_HIP_FORWARD_AUTO;
    }
    const bool reuse = (flags & TORBI_HIP_REUSE_TRANSITION) != 0;
    // ONE time-resident launch for the whole group: named (whole tiles per workgroup, or clusters), or AUTO with enough
    // items -- half the compute units' worth of tiles, or fewer tiles split over clusters (batches of >= 17 items)
    int largest = 0;
    long long items = 0;
    for (int k = 0; k < n; ++k) largest = std::max(largest, hb[k].B), items += hb[k].B;
    const bool split = cluster_members(tiles, S, cus) > 1;
    const bool together = resident_fits(S, tiles) &&
                          (path == TORBI_HIP_FORWARD_RESIDENT || path == TORBI_HIP_FORWARD_CLUSTER ||
                           (path == TORBI_HIP_FORWARD_AUTO && !small::supported(S) && !small_block_auto((int)std::min(items, 1ll << 30), S, cus) &&      // (a wavefront / workgroup per sequence)
                            (2 * tiles > cus || (split && largest > 16))));
    const bool clusters = together && split && path != TORBI_HIP_FORWARD_RESIDENT;
    const bool ascending = (flags & TORBI_HIP_SHORTEST_FIRST) != 0;
    PhaseEvents pe(phase_ms != nullptr);
    if (pe.err != hipSuccess) return (int)pe.err;
    int launches = 0, covered = n;
    Route taken = ROUTE_BAND;
    hipError_t e = hipSuccess;
    if (banded) {
        e = run_band(hb, n, transition, initial, S, band_choice, cus, s, pe.events(), &launches, ascending);
    } else if (together) {
        e = run_resident(hb, n, transition, initial, S, cus, s, pe.events(), &launches, reuse, ascending, clusters,
                         few_seeds(flags, clusters), call.preparation);
        taken = clusters ? ROUTE_CLUSTER : ROUTE_RESIDENT;
    } else {
        // one batch after the other, each on the path it would take alone (route_for); phases and route of the LAST batch
        // only; the reuse promise covers the first batch's workspace only
        for (int k = 0; k < n && e == hipSuccess; ++k)
            e = run_decode(hb[k], transition, initial, S, device, s, k == n - 1 ? pe.events() : nullptr, &launches,
                           reuse && k == 0, path, flags, &taken, call.preparation);
        covered = 1;
    }
    mark_decode_end(device, s);
    if (phase_ms) {
        if (e == hipSuccess) e = pe.read(phase_ms);
        phase_ms[2] = (float)launches;
        phase_ms[3] = (float)taken;
        phase_ms[5] = (float)covered;
    }
    return (int)e;
}

}  // namespace

// ---------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------
extern "C" {

int torbi_hip_abi_version(void) { return TORBI_HIP_ABI_VERSION; }

const char *torbi_hip_error_string(int code) {
    switch (code) {
        case TORBI_HIP_OK: return "success";
        case TORBI_HIP_EINVAL: return "invalid argument (null pointer, non-positive dimension, unknown flag or a decode workspace that is not 256-byte aligned)";
        case TORBI_HIP_EWORKSPACE: return "workspace smaller than torbi_hip_workspace_bytes()";
        case TORBI_HIP_ERANGE: return "problem dimensions out of range for this build";
        case TORBI_HIP_ENODEVICE: return "no usable HIP device";
        case TORBI_HIP_EUNSUPPORTED: return "shape not covered by this specialised entry point";
        default: break;
    }
    if (code > 0) return hipGetErrorString(static_cast<hipError_t>(code));
    return "unknown torbi_hip error";
}

int torbi_hip_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int torbi_hip_compute_units(int device) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) return TORBI_HIP_ENODEVICE;
    return cu_count(device);
}

size_t torbi_hip_workspace_bytes(int B, int T, int S) {
    if (B <= 0 || T <= 0 || S <= 0) return 256;
    return need_bytes_any_device(B, T, S);
}

int torbi_hip_last_forward_kernel(char *name_out, size_t capacity) {
    if (!name_out || capacity == 0) return TORBI_HIP_EINVAL;
    snprintf(name_out, capacity, "%s", g_last_kernel);
    return TORBI_HIP_OK;
}

int torbi_hip_set_forward_path(int path) {
    if (path < TORBI_HIP_FORWARD_AUTO || path > TORBI_HIP_FORWARD_BAND) return TORBI_HIP_EINVAL;
    g_forward_path.store(path, std::memory_order_relaxed);
    return TORBI_HIP_OK;
}

int torbi_hip_forward_path(int B, int S) { return torbi_hip_forward_path_on(B, S, 0, 0u); }

int torbi_hip_forward_path_on(int B, int S, int device, unsigned flags) {
    if (B <= 0 || S <= 0 || !flags_ok(flags)) return TORBI_HIP_EINVAL;
    return (int)route_for(requested_path(flags), B, S, cu_count(device));
}

int torbi_hip_viterbi_decode(const float *observation, const int32_t *batch_frames,
                             const float *transition, const float *initial,
                             int32_t *indices_out, void *workspace, size_t workspace_bytes,
                             int B, int T, int S, int device, void *stream) {
    return torbi_hip_viterbi_decode_ex(observation, batch_frames, transition, initial, indices_out, workspace,
                                       workspace_bytes, B, T, S, device, stream, 0u);
}

int torbi_hip_viterbi_decode_ex(const float *observation, const int32_t *batch_frames,
                                const float *transition, const float *initial,
                                int32_t *indices_out, void *workspace, size_t workspace_bytes,
                                int B, int T, int S, int device, void *stream, unsigned flags) {
    if (!flags_ok(flags)) return TORBI_HIP_EINVAL;
    const torbi_hip_batch one{observation, batch_frames, indices_out, workspace, workspace_bytes, B, T};
    // (a batch on its own has no order among batches to choose: TORBI_HIP_SHORTEST_FIRST belongs to the table entry points)
    return decode_group(&one, 1, DecodeCall{transition, initial, S, device, stream, flags & ~(unsigned)TORBI_HIP_SHORTEST_FIRST,
                                            nullptr, nullptr, nullptr});
}

int torbi_hip_viterbi_decode_batches(const torbi_hip_batch *batches, int count, const float *transition,
                                     const float *initial, int S, int device, void *stream, unsigned flags,
                                     float *phase_ms) {
    if (!table_given(batches, count, transition, initial)) return TORBI_HIP_EINVAL;
    return decode_group(batches, count, DecodeCall{transition, initial, S, device, stream, flags, phase_ms, nullptr, nullptr});
}


extern "C++" {
namespace {
// `background_out` null: -inf is what counts as outside; else: the matrix's corner entry, whatever it is
int band_reach_impl(const float *transition, int S, int device, void *stream, int *reach_left_out, int *reach_right_out,
                    float *background_out) {
    if (!transition || S < 1 || !reach_left_out || !reach_right_out) return TORBI_HIP_EINVAL;
    DeviceGuard guard(device);
    if (guard.err != hipSuccess) return (int)guard.err;
    hipStream_t s = static_cast<hipStream_t>(stream);
    // a few bytes of device scratch per host thread and device, kept for the life of the thread: hipMalloc / hipFree per call
    // synchronise the whole device (round-5 advisor) and stall other streams' decodes
    thread_local int32_t *scratch[kMaxDevices] = {};
    if (device < 0 || device >= kMaxDevices) return TORBI_HIP_EINVAL;
    hipError_t e = hipSuccess;
    if (!scratch[device]) e = hipMalloc(reinterpret_cast<void **>(&scratch[device]), 4 * sizeof(int32_t));
    if (e != hipSuccess) return (int)e;
    int32_t *const dev = scratch[device];
    int32_t host[4] = {-1, -1, 0, 0};
    hipLaunchKernelGGL(fill_pair_kernel, dim3(1), dim3(1), 0, s, dev, -1, -1);     // (-1, -1: what a matrix without an entry inside leaves)
    hipLaunchKernelGGL(fill_pair_kernel, dim3(1), dim3(1), 0, s, dev + 2, 0, 0);
    hipLaunchKernelGGL(band::band_reach_kernel, dim3(S), dim3(64), 0, s, transition, dev, S, background_out ? 1 : 0);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(host, dev, sizeof(host), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return (int)e;
    *reach_left_out = host[0];
    *reach_right_out = host[1];
    if (background_out) {
        union { int32_t i; float f; } bits;
        bits.i = host[2];
        *background_out = bits.f;
        // a FINITE constant is taken only from matrices whose every other entry lies ABOVE it (a pitch matrix: log(tiny) against
        // at least -10.5 inside the band) and that have such entries: where the band reaches down to the constant, the outputs
        // next to a row's maximum cannot be decided from the maximum alone, and the launch would be decoded again every time
        if (bits.f != -INFINITY && (host[3] != 0 || host[0] < 0)) *reach_left_out = *reach_right_out = S - 1;
    }
    return TORBI_HIP_OK;
}
}  // namespace
}  // extern "C++"

int torbi_hip_band_reach(const float *transition, int S, int device, void *stream, int *reach_left_out, int *reach_right_out) {
    return band_reach_impl(transition, S, device, stream, reach_left_out, reach_right_out, nullptr);
}

int torbi_hip_band_reach_over(const float *transition, int S, int device, void *stream, int *reach_left_out, int *reach_right_out,
                              float *background_out) {
    if (!background_out) return TORBI_HIP_EINVAL;
    return band_reach_impl(transition, S, device, stream, reach_left_out, reach_right_out, background_out);
}

int torbi_hip_band_members_over(int items, int S, int reach_left, int reach_right, float background, int device) {
    if (items < 1 || S < 1 || reach_left < 0 || reach_right < 0) return TORBI_HIP_EINVAL;
    BandChoice c;
    if (!band_shape(S) || !choose_band(S, reach_left, reach_right, band_tiles(items), cu_count(device), c, background)) return 0;
    return c.pl.R;
}

int torbi_hip_band_members(int items, int S, int reach_left, int reach_right, int device) {
    return torbi_hip_band_members_over(items, S, reach_left, reach_right, -INFINITY, device);
}

int torbi_hip_viterbi_decode_banded(const torbi_hip_batch *batches, int count, const float *transition, const float *initial,
                                    int S, int reach_left, int reach_right, int device, void *stream, unsigned flags,
                                    float *phase_ms) {
    return torbi_hip_viterbi_decode_banded_over(batches, count, transition, initial, S, reach_left, reach_right, -INFINITY, device,
                                                stream, flags, phase_ms);
}

int torbi_hip_viterbi_decode_banded_over(const torbi_hip_batch *batches, int count, const float *transition, const float *initial,
                                         int S, int reach_left, int reach_right, float background, int device, void *stream,
                                         unsigned flags, float *phase_ms) {
    if (reach_left < 0 || reach_right < 0 || !table_given(batches, count, transition, initial)) return TORBI_HIP_EINVAL;
    const BandPromise band{reach_left, reach_right, background};
    return decode_group(batches, count, DecodeCall{transition, initial, S, device, stream, flags, phase_ms, &band, nullptr});
}

size_t torbi_hip_preparation_bytes(int S) { return S > 0 ? preparation_bytes(S) : 256; }

int torbi_hip_viterbi_decode_batches_prepared(const torbi_hip_batch *batches, int count, const float *transition,
                                              const float *initial, int S, int device, void *stream, unsigned flags,
                                              float *phase_ms, void *preparation, size_t preparation_bytes_given,
                                              int *filled) {
    if (filled) *filled = 0;
    if (preparation && (S < 1 || preparation_bytes_given < preparation_bytes(S) || (reinterpret_cast<uintptr_t>(preparation) & 255)))
        return TORBI_HIP_EWORKSPACE;
    if (!table_given(batches, count, transition, initial)) return TORBI_HIP_EINVAL;
    Preparation kept{preparation, preparation_bytes_given, preparation && (flags & TORBI_HIP_REUSE_TRANSITION)};
    const int rc = decode_group(batches, count, DecodeCall{transition, initial, S, device, stream, flags, phase_ms, nullptr,
                                                           preparation ? &kept : nullptr});
    if (filled && rc == TORBI_HIP_OK) *filled = kept.valid ? 1 : 0;
    return rc;
}

int torbi_hip_scan_stats(const void *workspace, size_t workspace_bytes, int B, int T, int S,
                         unsigned *stats_out, int device, void *stream, unsigned flags) {
    if (B < 1 || T < 1 || S < 1 || !workspace || !stats_out || !flags_ok(flags)) return TORBI_HIP_EINVAL;
    DeviceGuard guard(device);
    if (guard.err != hipSuccess) return (int)guard.err;
    if (workspace_bytes < need_bytes(B, T, S, cu_count(device))) return TORBI_HIP_EWORKSPACE;
    // which statistics: decided on the device by the route the last decode with this workspace took
    const int cus = cu_count(device);
    const unsigned *resident_stats = resident::supported(S) ? carve_resident(const_cast<void *>(workspace), B, T, S, cus).stats : nullptr;
    const unsigned *held_control = carve(const_cast<void *>(workspace), B, T, S).control;
    if (!resident_stats && !held_control) return TORBI_HIP_EUNSUPPORTED;
    hipLaunchKernelGGL(gather_stats_kernel, dim3(1), dim3(2 * pruned::kStatSlots), 0, static_cast<hipStream_t>(stream),
                       route_record(workspace, B, T, S, cus), resident_stats ? resident_stats : held_control, held_control,
                       stats_out);
    return (int)hipGetLastError();
}

extern "C++" {
namespace {
template <bool PROBS>
int decode_uniform_as(const float *observation, const int32_t *batch_frames, float log_transition, const float *initial,
                      int32_t *indices_out, int B, int T, int S, int device, void *stream) {
    if (B < 0 || T < 1 || S < 1) return TORBI_HIP_EINVAL;
    if (B == 0) return TORBI_HIP_OK;
    if (!observation || !batch_frames || !initial || !indices_out) return TORBI_HIP_EINVAL;
    if (S % 4 != 0 || S > 4096 || (reinterpret_cast<uintptr_t>(observation) & 15) ||
        (reinterpret_cast<uintptr_t>(initial) & 15))
        return TORBI_HIP_EUNSUPPORTED;
    DeviceGuard guard(device);
    if (guard.err != hipSuccess) return (int)guard.err;
    hipStream_t s = static_cast<hipStream_t>(stream);
    // a wave per observation row, the reductions off the dependent chain (uniform_decode.hpp); R rows per wave and chunk:
    // 1, 2 and 3 run alike (0.27 ms at 512 x 500 x 1440), 4 spills
    // at most one workgroup per compute unit: the rows in flight per item are the only parallelism there is -- 16 waves
    // per workgroup (8 above 2048 states: 128 registers a lane do not hold two rows there).  tools/uniform_probe.py, ms per
    // 500 x 1440 decode, 16 / 4 waves: 1 item 0.081 / 0.148, 128: 0.107 / 0.160, 256: 0.141 / 0.206; two 8-wave workgroups
    // per unit for 257..512 items run like the 4-wave ones
    const bool few = B <= cu_count(device);
    // NQW float4 of a row per lane and pass (S <= 4096: the last instance covers what got here)
    by_state_count<1, 2, 4, 6, 8, 12, 16>(S, [&](auto nqw) {
        constexpr int NQW = decltype(nqw)::value, NWF = NQW <= 8 ? 16 : 8, R = NQW <= 8 ? 2 : 1;
        if (few) {
            auto *kernel = &uniform::uniform_rows_kernel<NQW, 1, PROBS, NWF>;
            hipLaunchKernelGGL(kernel, dim3(B), dim3(64 * NWF), 0, s, observation, batch_frames, initial, log_transition, indices_out,
                               B, T, S);
        } else {
            auto *kernel = &uniform::uniform_rows_kernel<NQW, R, PROBS>;
            hipLaunchKernelGGL(kernel, dim3(B), dim3(256), 0, s, observation, batch_frames, initial, log_transition, indices_out, B,
                               T, S);
        }
    });
    hipLaunchKernelGGL(uniform::uniform_repair_kernel<PROBS>, dim3(B), dim3(256), 0, s, observation, batch_frames, initial,
                       log_transition, indices_out, B, T, S);     // (items that read a NaN / +inf)
    mark_decode_end(device, s);
    return (int)hipGetLastError();
}
}  // namespace
}  // extern "C++"

int torbi_hip_viterbi_decode_uniform(const float *observation, const int32_t *batch_frames,
                                     float log_transition, const float *initial,
                                     int32_t *indices_out, int B, int T, int S, int device,
                                     void *stream) {
    return decode_uniform_as<false>(observation, batch_frames, log_transition, initial, indices_out, B, T, S, device, stream);
}

int torbi_hip_viterbi_decode_uniform_probabilities(const float *probabilities, const int32_t *batch_frames,
                                                   float log_transition, const float *initial, int32_t *indices_out,
                                                   int B, int T, int S, int device, void *stream) {
    return decode_uniform_as<true>(probabilities, batch_frames, log_transition, initial, indices_out, B, T, S, device, stream);
}

int torbi_hip_viterbi_decode_profiled(const float *observation, const int32_t *batch_frames,
                                      const float *transition, const float *initial,
                                      int32_t *indices_out, void *workspace,
                                      size_t workspace_bytes, int B, int T, int S, int device,
                                      void *stream, unsigned flags, float *phase_ms) {
    if (!phase_ms || !flags_ok(flags) || !transition || !initial) return TORBI_HIP_EINVAL;
    const torbi_hip_batch one{observation, batch_frames, indices_out, workspace, workspace_bytes, B, T};
    // a table of one: the group decision of decode_group() counts the 16-item tiles of the group, which for one batch is what
    // route_for() does, so the routing is that of torbi_hip_viterbi_decode_ex for this shape
    unsigned f = flags;
    if (((flags >> 4) & 7u) == 0) f |= TORBI_HIP_PATH_FLAG(default_path());
    return decode_group(&one, 1, DecodeCall{transition, initial, S, device, stream, f, phase_ms, nullptr, nullptr});
}

int torbi_hip_read_posterior(const void *workspace, size_t workspace_bytes,
                             const int32_t *batch_frames, float *posterior_out, int B, int T,
                             int S, int device, void *stream, unsigned flags) {
    if (B < 0 || T < 1 || S < 1 || !flags_ok(flags)) return TORBI_HIP_EINVAL;
    if (B == 0) return TORBI_HIP_OK;
    if (!workspace || !batch_frames || !posterior_out) return TORBI_HIP_EINVAL;
    DeviceGuard guard(device);
    if (guard.err != hipSuccess) return (int)guard.err;
    if (workspace_bytes < need_bytes(B, T, S, cu_count(device))) return TORBI_HIP_EWORKSPACE;
    const size_t n = (size_t)B * S;
    const int grid = (int)((n + 255) / 256 < 2048 ? (n + 255) / 256 : 2048);
    const Workspace w = carve(const_cast<void *>(workspace), B, T, S);
    hipLaunchKernelGGL(gather_final_kernel, dim3(grid), dim3(256), 0, static_cast<hipStream_t>(stream),
                       route_record(workspace, B, T, S, cu_count(device)), static_cast<const float *>(workspace), w.post[0],
                       w.post[1], batch_frames, posterior_out, B, T, S);
    return (int)hipGetLastError();
}

int torbi_hip_epsilon_clamp(float *x, uint64_t count, int device, void *stream) {
    if (count == 0) return TORBI_HIP_OK;
    if (!x || (reinterpret_cast<uintptr_t>(x) & 15)) return TORBI_HIP_EINVAL;
    DeviceGuard guard(device);
    if (guard.err != hipSuccess) return (int)guard.err;
    const uint64_t blocks = (count / 4 + 255) / 256 + 1;
    const int grid = (int)(blocks < 16384 ? blocks : 16384);
    hipLaunchKernelGGL(epsilon_clamp_kernel, dim3(grid), dim3(256), 0, static_cast<hipStream_t>(stream), x,
                       count);
    return (int)hipGetLastError();
}

int torbi_hip_log_epsilon_clamp(const float *probabilities, float *out, uint64_t count, int device, void *stream) {
    if (count == 0) return TORBI_HIP_OK;
    if (!probabilities || !out || ((reinterpret_cast<uintptr_t>(probabilities) | reinterpret_cast<uintptr_t>(out)) & 15))
        return TORBI_HIP_EINVAL;
    DeviceGuard guard(device);
    if (guard.err != hipSuccess) return (int)guard.err;
    const uint64_t blocks = (count / 4 + 255) / 256 + 1;
    const int grid = (int)(blocks < 16384 ? blocks : 16384);
    hipLaunchKernelGGL(log_epsilon_clamp_kernel, dim3(grid), dim3(256), 0, static_cast<hipStream_t>(stream), probabilities,
                       out, count);
    return (int)hipGetLastError();
}

int torbi_hip_fill_synthetic(float *dst, uint64_t count, uint64_t start, int stream_id, int seed,
                             int device, void *stream) {
    if (count == 0) return TORBI_HIP_OK;
    if (!dst) return TORBI_HIP_EINVAL;
    DeviceGuard guard(device);
    if (guard.err != hipSuccess) return (int)guard.err;
    const uint64_t key =
        ((uint64_t)(uint32_t)stream_id + (uint64_t)(uint32_t)seed * 1000003ull) * 0x9E3779B97F4A7C15ull;
    const uint64_t blocks = (count + 255) / 256;
    const int grid = (int)(blocks < 8192 ? blocks : 8192);
    hipLaunchKernelGGL(fill_synthetic_kernel, dim3(grid), dim3(256), 0,
                       static_cast<hipStream_t>(stream), dst, count, start, key);
    return (int)hipGetLastError();
}

// ---- streaming decode (stream.hpp) ----

// the state of B streams: posterior rows [B][capacity][S], memo [B][capacity], backpointers [B][S]; 4-byte words, packed
struct StreamState { float *ring; int32_t *memo, *bp; size_t bytes; };
static StreamState stream_state(void *state, int B, int S, int capacity) {
    Scratch a(state);
    StreamState st;
    st.ring = a.take<float>((size_t)B * capacity * S, 4);
    st.memo = a.take<int32_t>((size_t)B * capacity, 4);
    st.bp = a.take<int32_t>((size_t)B * S, 4);
    st.bytes = a.bytes;
    return st;
}

size_t torbi_hip_stream_state_bytes(int B, int S, int capacity) {
    if (B < 1 || S < 1 || capacity < 1) return 0;
    return stream_state(nullptr, B, S, capacity).bytes;
}

static int stream_args_ok(const void *info, const void *transition, const void *state, size_t state_bytes, int capacity,
                          const void *indices_out, int out_capacity, const void *counts_out, int B, int S) {
    if (B < 1 || S < 1 || capacity < 1 || out_capacity < 1) return TORBI_HIP_EINVAL;
    if (!info || !transition || !state || !indices_out || !counts_out) return TORBI_HIP_EINVAL;
    if (S > stream::kMaxStates) return TORBI_HIP_ERANGE;
    if (state_bytes < torbi_hip_stream_state_bytes(B, S, capacity)) return TORBI_HIP_EWORKSPACE;
    return TORBI_HIP_OK;
}

// the per-push arguments of torbi_hip_stream_push_lag and torbi_hip_stream_band_push; `inputs`: nothing that a push with
// frames reads is null
static int stream_push_args_ok(int Tc, bool inputs, int max_lag, const void *forced_out) {
    return Tc < 0 || (Tc > 0 && !inputs) || max_lag < -1 || (max_lag >= 0 && !forced_out) ? TORBI_HIP_EINVAL : TORBI_HIP_OK;
}

// Streams per workgroup of a push's forward kernel (stream_forward_kernel<G, *>): as many as the double-buffered rows let
// share one pass over the matrix, but no fewer workgroups than compute units while there are streams for them.
static int stream_tile(int B, int S, int device) {
    if (B < 1 || S < 1) return TORBI_HIP_EINVAL;
    if (S > stream::kMaxStates) return TORBI_HIP_ERANGE;
    return items_per_workgroup(16, B, 1, cu_count(device),
                               [&](int G) { return (size_t)2 * G * S * sizeof(float) <= (size_t)stream::kMaxLdsBytes; });
}

int torbi_hip_stream_tile(int B, int S, int device) { return stream_tile(B, S, device); }

int torbi_hip_stream_push(const float *observation, int Tc, const int32_t *info, const float *transition,
                          const float *transition_t, const float *initial, void *state, size_t state_bytes, int capacity,
                          int32_t *indices_out, int out_capacity, int32_t *counts_out, int B, int S, int device, void *stream) {
    return torbi_hip_stream_push_lag(observation, Tc, info, transition, transition_t, initial, state, state_bytes, capacity,
                                     indices_out, out_capacity, counts_out, -1, nullptr, B, S, device, stream);
}

// max_lag = -1: no bound (torbi_hip_stream_push); >= 0: the walk's bounded arm, forced_out[b] of counts_out[b] frames forced
int torbi_hip_stream_push_lag(const float *observation, int Tc, const int32_t *info, const float *transition,
                              const float *transition_t, const float *initial, void *state, size_t state_bytes, int capacity,
                              int32_t *indices_out, int out_capacity, int32_t *counts_out, int max_lag, int32_t *forced_out,
                              int B, int S, int device, void *stream) {
    int code = stream_args_ok(info, transition, state, state_bytes, capacity, indices_out, out_capacity, counts_out, B, S);
    if (code == TORBI_HIP_OK) code = stream_push_args_ok(Tc, observation && transition_t && initial, max_lag, forced_out);
    if (code != TORBI_HIP_OK) return code;
    DeviceGuard guard(device);
    if (guard.err != hipSuccess) return (int)guard.err;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const stream::Info *in = reinterpret_cast<const stream::Info *>(info);
    const StreamState ss = stream_state(state, B, S, capacity);
    float *const ring = ss.ring;
    int32_t *const memo = ss.memo, *const bp = ss.bp;
    if (Tc > 0) {
        const int G = stream_tile(B, S, device);
        const int room = capacity < out_capacity ? capacity : out_capacity;
        const bool vec = S % 4 == 0 && (reinterpret_cast<uintptr_t>(transition_t) & 15) == 0;
        const dim3 grid((B + G - 1) / G);
        const size_t lds = (size_t)2 * G * S * sizeof(float);
        by_value<16, 8, 4, 2, 1>(G, [&](auto g) { by_flag(vec, [&](auto vec_) {
            auto *kernel = &stream::stream_forward_kernel<decltype(g)::value, decltype(vec_)::value ? 4 : 1>;
            hipLaunchKernelGGL(kernel, grid, dim3(stream::kThreads), lds, st, observation, Tc, in, transition_t, initial, ring, memo,
                               capacity, room, B, S);
        }); });
        if ((code = (int)hipGetLastError()) != hipSuccess) return code;
        if (S > 1) {
            hipLaunchKernelGGL(stream::stream_first_step_kernel, dim3((S + 3) / 4, B), dim3(stream::kThreads), 0, st, in,
                               transition, ring, bp, capacity, room, Tc, S);
            if ((code = (int)hipGetLastError()) != hipSuccess) return code;
        }
    }
    by_flag(max_lag >= 0, [&](auto lag) {
        hipLaunchKernelGGL((stream::stream_walk_kernel<false, decltype(lag)::value>), dim3(B), dim3(stream::kThreads),
                           (size_t)2 * S * sizeof(int32_t), st, in, transition, ring, memo, bp, capacity, indices_out, out_capacity,
                           counts_out, Tc, S, max_lag, forced_out);
    });
    return (int)hipGetLastError();
}

int torbi_hip_stream_flush(const int32_t *info, const float *transition, void *state, size_t state_bytes, int capacity,
                           int32_t *indices_out, int out_capacity, int32_t *counts_out, int B, int S, int device, void *stream) {
    const int code = stream_args_ok(info, transition, state, state_bytes, capacity, indices_out, out_capacity, counts_out, B, S);
    if (code != TORBI_HIP_OK) return code;
    DeviceGuard guard(device);
    if (guard.err != hipSuccess) return (int)guard.err;
    const StreamState ss = stream_state(state, B, S, capacity);
    hipLaunchKernelGGL(stream::stream_walk_kernel<true>, dim3(B), dim3(stream::kThreads), (size_t)2 * S * sizeof(int32_t),
                       static_cast<hipStream_t>(stream), reinterpret_cast<const stream::Info *>(info), transition, ss.ring,
                       ss.memo, ss.bp, capacity, indices_out, out_capacity, counts_out, 0, S, -1, nullptr);
    return (int)hipGetLastError();
}

// ---- streaming decode on a band with one constant outside it (stream_band.hpp) ----

// the band route's view of the same bytes: backpointers [B][capacity][S], memo [B][capacity], the carried rows [B][S]
struct StreamBandState { int32_t *ring, *memo; float *carried; };
static StreamBandState stream_band_state(void *state, int B, int S, int capacity) {
    Scratch a(state);
    StreamBandState st;
    st.ring = a.take<int32_t>((size_t)B * capacity * S, 4);
    st.memo = a.take<int32_t>((size_t)B * capacity, 4);
    st.carried = a.take<float>((size_t)B * S, 4);
    return st;
}

// the shapes and bands the band route takes (no wider than what torbi_hip_band_reach_over's callers ask about)
static bool stream_band_shape(int S, int reach_left, int reach_right) {
    return banddiag::shape_ok(S, reach_left, reach_right) &&
           stream_band::lds_bytes(1, S, reach_left, reach_right) <= (size_t)stream_band::kMaxLdsBytes;
}

int torbi_hip_stream_band_covers(int B, int S, int reach_left, int reach_right, float background, int device) {
    (void)device;
    if (B < 1 || !stream_band_shape(S, reach_left, reach_right)) return 0;
    return background_ok(background) ? 1 : 0;
}

// Streams per workgroup of stream_band_forward_kernel<G>: stream_tile's rule with the band kernel's LDS (rows with halos,
// double-buffered, and the two scans of every stream)
int torbi_hip_stream_band_tile(int B, int S, int reach_left, int reach_right, int device) {
    if (B < 1 || S < 1 || reach_left < 0 || reach_right < 0) return TORBI_HIP_EINVAL;
    if (!stream_band_shape(S, reach_left, reach_right)) return TORBI_HIP_EUNSUPPORTED;
    return items_per_workgroup(stream_band::kMaxGroup, B, 1, cu_count(device), [&](int G) {
        return stream_band::lds_bytes(G, S, reach_left, reach_right) <= (size_t)stream_band::kMaxLdsBytes;
    });
}

size_t torbi_hip_stream_band_diagonals_bytes(int S, int reach_left, int reach_right) {
    if (S < 1 || reach_left < 0 || reach_right < 0) return 0;
    return banddiag::diagonals_bytes(S, reach_left, reach_right);
}

int torbi_hip_stream_band_prepare(const float *transition, int S, int reach_left, int reach_right, float background,
                                  float *diagonals_out, int32_t *ok_out, int device, void *stream) {
    if (S < 1 || reach_left < 0 || reach_right < 0 || !transition || !diagonals_out || !ok_out) return TORBI_HIP_EINVAL;
    if (!torbi_hip_stream_band_covers(1, S, reach_left, reach_right, background, device)) return TORBI_HIP_EUNSUPPORTED;
    DeviceGuard guard(device);
    if (guard.err != hipSuccess) return (int)guard.err;
    // (no matrix alarm on this route: the verdict is the only word written beside the diagonals)
    return (int)banddiag::prepare(transition, diagonals_out, ok_out, nullptr, background, reach_left, reach_right, S,
                                  static_cast<hipStream_t>(stream));
}

int torbi_hip_stream_band_push(const float *observation, int Tc, const int32_t *info, const float *diagonals, const float *initial,
                               int reach_left, int reach_right, float background, void *state, size_t state_bytes, int capacity,
                               int32_t *indices_out, int out_capacity, int32_t *counts_out, int max_lag, int32_t *forced_out,
                               int B, int S, int device, void *stream) {
    // torbi_hip_stream_push_lag's argument rules, the diagonals standing where its matrix stands; then the band's own
    int code = stream_args_ok(info, diagonals, state, state_bytes, capacity, indices_out, out_capacity, counts_out, B, S);
    if (code == TORBI_HIP_OK) code = stream_push_args_ok(Tc, observation && initial, max_lag, forced_out);
    if (code != TORBI_HIP_OK) return code;
    if (reach_left < 0 || reach_right < 0) return TORBI_HIP_EINVAL;
    if (!torbi_hip_stream_band_covers(B, S, reach_left, reach_right, background, device)) return TORBI_HIP_EUNSUPPORTED;
    DeviceGuard guard(device);
    if (guard.err != hipSuccess) return (int)guard.err;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const stream::Info *in = reinterpret_cast<const stream::Info *>(info);
    const StreamBandState ss = stream_band_state(state, B, S, capacity);
    int32_t *const ring = ss.ring, *const memo = ss.memo;
    float *const carried = ss.carried;
    if (Tc > 0) {
        const int G = torbi_hip_stream_band_tile(B, S, reach_left, reach_right, device);
        const int room = capacity < out_capacity ? capacity : out_capacity;
        const dim3 grid((B + G - 1) / G);
        const size_t lds = stream_band::lds_bytes(G, S, reach_left, reach_right);
        hipError_t e = by_value<4, 2, 1>(G, [&](auto g) {
            auto *kernel = &stream_band::stream_band_forward_kernel<decltype(g)::value>;
            const hipError_t granted = ensure_dynamic_lds(kernel, lds);
            if (granted != hipSuccess) return granted;
            hipLaunchKernelGGL(kernel, grid, dim3(stream_band::kForwardThreads), lds, st, observation, Tc, in, diagonals, initial, background,
                               reach_left, reach_right, ring, memo, carried, capacity, room, B, S);
            return hipGetLastError();
        });
        if (e != hipSuccess) return (int)e;
    }
    by_flag(max_lag >= 0, [&](auto lag) {
        hipLaunchKernelGGL((stream_band::stream_band_walk_kernel<false, decltype(lag)::value>), dim3(B), dim3(stream_band::kThreads),
                           (size_t)2 * S * sizeof(int32_t), st, in, ring, memo, carried, capacity, indices_out, out_capacity,
                           counts_out, Tc, S, max_lag, forced_out);
    });
    return (int)hipGetLastError();
}

int torbi_hip_stream_band_flush(const int32_t *info, void *state, size_t state_bytes, int capacity, int32_t *indices_out,
                                int out_capacity, int32_t *counts_out, int B, int S, int device, void *stream) {
    // (the flush reads no matrix: `info` stands in for torbi_hip_stream_flush's)
    const int code = stream_args_ok(info, info, state, state_bytes, capacity, indices_out, out_capacity, counts_out, B, S);
    if (code != TORBI_HIP_OK) return code;
    if (!banddiag::states_ok(S)) return TORBI_HIP_EUNSUPPORTED;
    DeviceGuard guard(device);
    if (guard.err != hipSuccess) return (int)guard.err;
    const StreamBandState ss = stream_band_state(state, B, S, capacity);
    hipLaunchKernelGGL(stream_band::stream_band_walk_kernel<true>, dim3(B), dim3(stream_band::kThreads),
                       (size_t)2 * S * sizeof(int32_t), static_cast<hipStream_t>(stream),
                       reinterpret_cast<const stream::Info *>(info), ss.ring, ss.memo, ss.carried, capacity, indices_out, out_capacity,
                       counts_out, 0, S, -1, nullptr);
    return (int)hipGetLastError();
}

// ---- streaming posteriors: filtering and fixed-lag smoothing (stream_posterior.hpp) ----

namespace sp = stream_posterior;

// the state of B streams: running sums [B][2] words, a and e [B][capacity][S], c and m [B][capacity]; 4-byte words, packed
struct StreamPosteriorState { int32_t *L; float *a, *e, *c, *m; size_t bytes; };
static StreamPosteriorState stream_posterior_state(void *state, int B, int S, int capacity) {
    Scratch s(state);
    StreamPosteriorState st;
    st.L = s.take<int32_t>((size_t)B * 2, 4);
    st.a = s.take<float>((size_t)B * capacity * S, 4);
    st.e = s.take<float>((size_t)B * capacity * S, 4);
    st.c = s.take<float>((size_t)B * capacity, 4);
    st.m = s.take<float>((size_t)B * capacity, 4);
    st.bytes = s.bytes;
    return st;
}

size_t torbi_hip_stream_posterior_state_size(int B, int S, int capacity) {
    if (B < 1 || S < 1 || capacity < 1) return 0;
    return stream_posterior_state(nullptr, B, S, capacity).bytes;
}

// Streams per workgroup of sp_forward_kernel / sp_backward_kernel: stream_tile's rule with this route's LDS
int torbi_hip_stream_posterior_tile(int B, int S, int device) {
    if (B < 1 || S < 1) return TORBI_HIP_EINVAL;
    if (S > sp::kMaxStates) return TORBI_HIP_ERANGE;
    return items_per_workgroup(sp::kMaxGroup, B, 1, cu_count(device), [&](int G) { return sp::fits(G, S); });
}

static int stream_posterior_args_ok(const void *info, const void *expa, const void *state, size_t state_bytes, int capacity,
                                    const void *posterior_out, int out_capacity, int lag, int B, int S) {
    if (B < 1 || S < 1 || capacity < 1 || out_capacity < 1 || lag < 0) return TORBI_HIP_EINVAL;
    if (!info || !expa || !state || !posterior_out) return TORBI_HIP_EINVAL;
    if (S > sp::kMaxStates) return TORBI_HIP_ERANGE;
    if (state_bytes < torbi_hip_stream_posterior_state_size(B, S, capacity)) return TORBI_HIP_EWORKSPACE;
    return TORBI_HIP_OK;
}

// the backward sweep of a push (Tc >= 0) or a flush (Tc < 0)
static int stream_posterior_sweep(const int32_t *info, int Tc, const float *expa, const StreamPosteriorState &ss, int capacity,
                                  float *posterior_out, int out_capacity, int32_t *counts_out, int lag, int B, int S, int device,
                                  hipStream_t st) {
    const int G = torbi_hip_stream_posterior_tile(B, S, device);
    const bool vec = S % 4 == 0 && (reinterpret_cast<uintptr_t>(expa) & 15) == 0;
    by_value<16, 8, 4, 2, 1>(G, [&](auto g) { by_flag(vec, [&](auto vec_) {
        auto *kernel = &sp::sp_backward_kernel<decltype(g)::value, decltype(vec_)::value ? 4 : 1>;
        hipLaunchKernelGGL(kernel, dim3((B + G - 1) / G), dim3(sp::kThreads), sp::lds_bytes(G, S), st,
                           reinterpret_cast<const stream::Info *>(info), Tc, expa, ss.L, ss.a, ss.e, ss.c, capacity, posterior_out,
                           out_capacity, counts_out, lag, B, S);
    }); });
    return (int)hipGetLastError();
}

int torbi_hip_stream_posterior_push(const float *observation, int Tc, const int32_t *info, const float *expa, const float *expa_t,
                                    const float *initial, void *state, size_t state_bytes, int capacity, float *posterior_out,
                                    int out_capacity, int32_t *counts_out, int lag, int B, int S, int device, void *stream) {
    int code = stream_posterior_args_ok(info, expa, state, state_bytes, capacity, posterior_out, out_capacity, lag, B, S);
    if (code != TORBI_HIP_OK) return code;
    if (Tc < 0 || (Tc > 0 && (!observation || !expa_t || !initial))) return TORBI_HIP_EINVAL;
    DeviceGuard guard(device);
    if (guard.err != hipSuccess) return (int)guard.err;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const StreamPosteriorState ss = stream_posterior_state(state, B, S, capacity);
    if (Tc > 0) {
        const int G = torbi_hip_stream_posterior_tile(B, S, device);
        const bool vec = S % 4 == 0 && (reinterpret_cast<uintptr_t>(expa_t) & 15) == 0;
        by_value<16, 8, 4, 2, 1>(G, [&](auto g) { by_flag(vec, [&](auto vec_) {
            auto *kernel = &sp::sp_forward_kernel<decltype(g)::value, decltype(vec_)::value ? 4 : 1>;
            hipLaunchKernelGGL(kernel, dim3((B + G - 1) / G), dim3(sp::kThreads), sp::lds_bytes(G, S), st, observation, Tc,
                               reinterpret_cast<const stream::Info *>(info), expa_t, initial, ss.L, ss.a, ss.e, ss.c, ss.m,
                               capacity, out_capacity, lag, B, S);
        }); });
        if ((code = (int)hipGetLastError()) != hipSuccess) return code;
    }
    return stream_posterior_sweep(info, Tc, expa, ss, capacity, posterior_out, out_capacity, counts_out, lag, B, S, device, st);
}

int torbi_hip_stream_posterior_flush(const int32_t *info, const float *expa, void *state, size_t state_bytes, int capacity,
                                     float *posterior_out, int out_capacity, int32_t *counts_out, int B, int S, int device,
                                     void *stream) {
    const int code = stream_posterior_args_ok(info, expa, state, state_bytes, capacity, posterior_out, out_capacity, 0, B, S);
    if (code != TORBI_HIP_OK) return code;
    DeviceGuard guard(device);
    if (guard.err != hipSuccess) return (int)guard.err;
    return stream_posterior_sweep(info, -1, expa, stream_posterior_state(state, B, S, capacity), capacity, posterior_out,
                                  out_capacity, counts_out, 0, B, S, device, static_cast<hipStream_t>(stream));
}

// ---- streaming posteriors on a band with one constant outside it (stream_posterior_band.hpp) ----

// the matrices the band route takes: torbi_hip_forward_backward_band_covers' rule for (S, band, background)
static bool stream_smooth_band_shape(int S, int reach_left, int reach_right) {
    if (S < 1 || S > spb::kMaxStates || reach_left < 0 || reach_right < 0) return false;
    const int W = fbb::band_of(S, reach_left, reach_right).W;
    return (W < S ? W : S) <= spb::kMaxWindow;               // at most 64 in-band entries in a matrix row
}

int torbi_hip_stream_smooth_band_covers(int B, int S, int reach_left, int reach_right, float background, int device) {
    (void)device;
    if (B < 1 || !stream_smooth_band_shape(S, reach_left, reach_right)) return 0;
    return background_ok(background) ? 1 : 0;
}

// Streams per workgroup of spb_forward_kernel<G> / spb_backward_kernel<G>: stream_tile's rule with the band kernels' LDS
int torbi_hip_stream_smooth_band_tile(int B, int S, int reach_left, int reach_right, int device) {
    if (B < 1 || S < 1 || reach_left < 0 || reach_right < 0) return TORBI_HIP_EINVAL;
    if (!stream_smooth_band_shape(S, reach_left, reach_right)) return TORBI_HIP_EUNSUPPORTED;
    const int halo = fbb::band_of(S, reach_left, reach_right).halo;
    return items_per_workgroup(spb::kMaxGroup, B, 1, cu_count(device),
                               [&](int G) { return spb::lds_bytes(G, S, halo) <= (size_t)spb::kMaxLdsBytes; });
}

size_t torbi_hip_stream_smooth_band_diagonals_size(int S, int reach_left, int reach_right) {
    if (S < 1 || reach_left < 0 || reach_right < 0) return 0;
    const fbb::Band band = fbb::band_of(S, reach_left, reach_right);
    return (size_t)2 * band.W * band.Sd * sizeof(float);
}

int torbi_hip_stream_smooth_band_prepare(const float *transition, int S, int reach_left, int reach_right, float background,
                                         float *diagonals_out, int32_t *ok_out, int device, void *stream) {
    if (S < 1 || reach_left < 0 || reach_right < 0 || !transition || !diagonals_out || !ok_out) return TORBI_HIP_EINVAL;
    if (!torbi_hip_stream_smooth_band_covers(1, S, reach_left, reach_right, background, device)) return TORBI_HIP_EUNSUPPORTED;
    DeviceGuard guard(device);
    if (guard.err != hipSuccess) return (int)guard.err;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const fbb::Band band = fbb::band_of(S, reach_left, reach_right);
    const hipError_t e = fbb::prepare_and_verify(transition, band, diagonals_out, diagonals_out + (size_t)band.W * band.Sd, ok_out,
                                                 exp_background(background), background, S, st);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(spb::spb_verdict_kernel, dim3(1), dim3(1), 0, st, ok_out);
    return (int)hipGetLastError();
}

// the argument rules of both calls: the dense entries' with `diagonals` where their matrix stands, then the band's own
static int stream_smooth_band_args_ok(const void *info, const void *diagonals, int reach_left, int reach_right, float background,
                                      const void *state, size_t state_bytes, int capacity, const void *posterior_out,
                                      int out_capacity, int lag, int B, int S, int device) {
    const int code = stream_posterior_args_ok(info, diagonals, state, state_bytes, capacity, posterior_out, out_capacity, lag, B, S);
    if (code != TORBI_HIP_OK) return code;
    if (reach_left < 0 || reach_right < 0) return TORBI_HIP_EINVAL;
    if (!torbi_hip_stream_smooth_band_covers(B, S, reach_left, reach_right, background, device)) return TORBI_HIP_EUNSUPPORTED;
    return TORBI_HIP_OK;
}

// the backward sweep of a push (Tc >= 0) or a flush (Tc < 0)
static int stream_smooth_band_sweep(const int32_t *info, int Tc, const float *diagonals, const fbb::Band &band, float ebg, int G,
                                    const StreamPosteriorState &ss, int capacity, float *posterior_out, int out_capacity,
                                    int32_t *counts_out, int lag, int B, int S, hipStream_t st) {
    by_value<8, 4, 2, 1>(G, [&](auto g) {
        auto *kernel = &spb::spb_backward_kernel<decltype(g)::value>;
        hipLaunchKernelGGL(kernel, dim3((B + G - 1) / G), dim3(spb::kThreads), spb::lds_bytes(G, S, band.halo), st,
                           reinterpret_cast<const stream::Info *>(info), Tc, diagonals + (size_t)band.W * band.Sd, ss.L, ss.a, ss.e,
                           ss.c, ebg, band.reach_left, band.halo, band.W, band.Sd, capacity, posterior_out, out_capacity,
                           counts_out, lag, B, S);
    });
    return (int)hipGetLastError();
}

int torbi_hip_stream_smooth_band_push(const float *observation, int Tc, const int32_t *info, const float *diagonals, int reach_left,
                                      int reach_right, float background, const float *initial, void *state, size_t state_bytes,
                                      int capacity, float *posterior_out, int out_capacity, int32_t *counts_out, int lag, int B,
                                      int S, int device, void *stream) {
    int code = stream_smooth_band_args_ok(info, diagonals, reach_left, reach_right, background, state, state_bytes, capacity,
                                          posterior_out, out_capacity, lag, B, S, device);
    if (code != TORBI_HIP_OK) return code;
    if (Tc < 0 || (Tc > 0 && (!observation || !initial))) return TORBI_HIP_EINVAL;
    DeviceGuard guard(device);
    if (guard.err != hipSuccess) return (int)guard.err;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const StreamPosteriorState ss = stream_posterior_state(state, B, S, capacity);
    const fbb::Band band = fbb::band_of(S, reach_left, reach_right);
    const float ebg = exp_background(background);
    const int G = torbi_hip_stream_smooth_band_tile(B, S, reach_left, reach_right, device);
    if (Tc > 0) {
        by_value<8, 4, 2, 1>(G, [&](auto g) {
            auto *kernel = &spb::spb_forward_kernel<decltype(g)::value>;
            hipLaunchKernelGGL(kernel, dim3((B + G - 1) / G), dim3(spb::kThreads), spb::lds_bytes(G, S, band.halo), st, observation,
                               Tc, reinterpret_cast<const stream::Info *>(info), diagonals, initial, ss.L, ss.a, ss.e, ss.c, ss.m,
                               ebg, band.reach_left, band.halo, band.W, band.Sd, capacity, out_capacity, lag, B, S);
        });
        if ((code = (int)hipGetLastError()) != hipSuccess) return code;
    }
    return stream_smooth_band_sweep(info, Tc, diagonals, band, ebg, G, ss, capacity, posterior_out, out_capacity, counts_out, lag, B,
                                    S, st);
}

int torbi_hip_stream_smooth_band_flush(const int32_t *info, const float *diagonals, int reach_left, int reach_right,
                                       float background, void *state, size_t state_bytes, int capacity, float *posterior_out,
                                       int out_capacity, int32_t *counts_out, int B, int S, int device, void *stream) {
    const int code = stream_smooth_band_args_ok(info, diagonals, reach_left, reach_right, background, state, state_bytes, capacity,
                                                posterior_out, out_capacity, 0, B, S, device);
    if (code != TORBI_HIP_OK) return code;
    DeviceGuard guard(device);
    if (guard.err != hipSuccess) return (int)guard.err;
    return stream_smooth_band_sweep(info, -1, diagonals, fbb::band_of(S, reach_left, reach_right), exp_background(background),
                                    torbi_hip_stream_smooth_band_tile(B, S, reach_left, reach_right, device),
                                    stream_posterior_state(state, B, S, capacity), capacity, posterior_out, out_capacity, counts_out,
                                    0, B, S, static_cast<hipStream_t>(stream));
}

// ---- forward-backward: state posteriors and log-likelihood (forward_backward.hpp) ----

size_t torbi_hip_forward_backward_workspace_bytes(int B, int T, int S) {
    if (B < 1 || T < 1 || S < 1 || S > fb::kMaxStates) return 256;
    return fb::layout(nullptr, B, T, S).total;
}

// what the grids of the forward-backward kernels hold, dense or band: 32-item tiles on grid y of the step kernels, rows / 4
// workgroups on grid x of the row kernels
static bool fb_shape_in_range(int B, int T, int S) {
    return S <= fb::kMaxStates && (size_t)B * T * S <= (size_t)1 << 40 && (B + 31) / 32 <= 65535 && (size_t)B * T <= (size_t)1 << 32;
}

static int fb_args_ok(const void *obs, const void *frames, const void *matrix, const void *initial, const void *post,
                      const void *loglik, const void *ws, size_t ws_bytes, int B, int T, int S) {
    if (B < 0 || T < 1 || S < 1) return TORBI_HIP_EINVAL;
    if (B == 0) return TORBI_HIP_OK;
    if (!obs || !frames || !matrix || !initial || !post || !loglik || !ws) return TORBI_HIP_EINVAL;
    if (!fb_shape_in_range(B, T, S)) return TORBI_HIP_ERANGE;
    if (ws_bytes < torbi_hip_forward_backward_workspace_bytes(B, T, S)) return TORBI_HIP_EWORKSPACE;
    return TORBI_HIP_OK;
}

static char *fb_base(void *workspace) {
    return reinterpret_cast<char *>((reinterpret_cast<uintptr_t>(workspace) + 255) & ~(uintptr_t)255);
}

// One step launch: 32 x 32 tiles (states x items).  With at least two tiles per compute unit, four waves per tile stage the
// operands through LDS; with fewer, K is split over as many waves as bring the launch to two per SIMD (at most 16 per
// workgroup), each reading its chunks from global memory.
extern "C++" template <bool BACKWARD>
static hipError_t fb_step(const float *obs, const int32_t *frames, const float *mat, const float *m, const float *cbuf,
                          float *partial, const float *loglik, float *post, const float *x_in, float *w_out, int t, int B,
                          int T, int S, bool vec, int cus, hipStream_t st) {
    const unsigned tiles = (unsigned)((S + 31) / 32) * (unsigned)((B + 31) / 32);
    const dim3 grid((S + 31) / 32, (B + 31) / 32);
    const bool staged = tiles >= 2u * cus;
    int KS = staged ? 4 : 1;
    while (!staged && KS * 2 <= fb::kMaxWaves && (long long)tiles * KS < 8LL * cus && 8 * KS * 2 <= S) KS *= 2;
    by_flag(staged, [&](auto staged_) { by_flag(vec, [&](auto vec_) {
        auto *kernel = &fb::fb_step_kernel<decltype(staged_)::value, BACKWARD, decltype(vec_)::value>;
        hipLaunchKernelGGL(kernel, grid, dim3(64 * KS), 0, st, obs, frames, mat, m, cbuf, partial, loglik, post, x_in, w_out, t, B, T,
                           S, KS);
    }); });
    return hipGetLastError();
}

// Expected-count outputs of torbi_hip_forward_backward_counts; null for the plain call.
struct FbCounts {
    const float *weights;
    float *counts, *initial_counts;
};

// The forward half of the dense route, shared by forward-backward and path sampling: E = exp(A) and its transpose, the row
// maxima, the unnormalised filtered rows a_t into `rows` ([B][T][S]; their 32-row partial sums into the workspace) and L.
static int fb_forward(const float *observation, const int32_t *batch_frames, const float *transition, const float *initial,
                      float *rows, float *loglik_out, const fb::Layout &l, int B, int T, int S, bool vec, int cus,
                      hipStream_t st) {
    float *const E = l.E, *const Et = l.Et, *const m = l.m, *const cbuf = l.c, *const partial = l.partial;
    hipError_t e;
    {
        const size_t n = (size_t)fb::padded_rows(S) * fb::padded_states(S);
        const int grid = (int)std::min<size_t>((n + 255) / 256, 4096);
        hipLaunchKernelGGL(fb::fb_prepare_kernel, dim3(grid), dim3(256), 0, st, transition, E, Et, S);
        if ((e = hipGetLastError()) != hipSuccess) return (int)e;
    }
    const size_t nrows = (size_t)B * T;
    hipLaunchKernelGGL(fb::fb_rowmax_kernel, dim3((unsigned)((nrows + 3) / 4)), dim3(256), 0, st, observation, batch_frames,
                       initial, m, B, T, S);
    if ((e = hipGetLastError()) != hipSuccess) return (int)e;
    hipLaunchKernelGGL(fb::fb_forward_first_kernel, dim3(B, (S + 255) / 256), dim3(256), 0, st, observation, initial, m,
                       rows, partial, T, S);
    if ((e = hipGetLastError()) != hipSuccess) return (int)e;
    for (int t = 1; t < T; ++t)
        if ((e = fb_step<false>(observation, batch_frames, E, m, cbuf, partial, loglik_out, rows, rows, nullptr, t, B, T, S, vec,
                                cus, st)) != hipSuccess)
            return (int)e;
    hipLaunchKernelGGL(fb::fb_loglik_kernel, dim3(B), dim3(256), 0, st, batch_frames, m, partial, cbuf, loglik_out, T, S);
    return (int)hipGetLastError();
}

// The dense route.  With `counts`, one fb_counts_kernel launch for pair t + 1 goes in front of backward step t (the
// kernels that produce posterior and log-likelihood are the same launches with the same arguments either way).
static int fb_dense(const float *observation, const int32_t *batch_frames, const float *transition, const float *initial,
                    float *posterior_out, float *loglik_out, void *workspace, int B, int T, int S, int device,
                    void *stream, const FbCounts *counts) {
    DeviceGuard guard(device);
    if (guard.err != hipSuccess) return (int)guard.err;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const fb::Layout l = fb::layout(fb_base(workspace), B, T, S);
    float *const E = l.E, *const Et = l.Et, *const m = l.m, *const cbuf = l.c, *const partial = l.partial, *const w = l.w;
    const size_t wrow = (size_t)B * fb::padded_states(S);
    const int cus = cu_count(device);
    hipError_t e;
    const bool vec = S % 4 == 0 && (reinterpret_cast<uintptr_t>(posterior_out) & 15) == 0;
    const int rc = fb_forward(observation, batch_frames, transition, initial, posterior_out, loglik_out, l, B, T, S, vec, cus, st);
    if (rc != TORBI_HIP_OK) return rc;
    hipLaunchKernelGGL(fb::fb_backward_last_kernel, dim3(B, (S + 255) / 256), dim3(256), 0, st, observation, batch_frames, m,
                       cbuf, loglik_out, posterior_out, w, B, T, S);
    if ((e = hipGetLastError()) != hipSuccess) return (int)e;
    const dim3 cgrid((S + fb::kCountsTile - 1) / fb::kCountsTile, (S + fb::kCountsTile - 1) / fb::kCountsTile);
    for (int t = T - 2; t >= 0; --t) {
        if (counts) {
            const float *wt = w + ((t + 1) & 1) * wrow;
            const int first = t == T - 2;
            by_flag(vec, [&](auto vec_) {
                auto *kernel = &fb::fb_counts_kernel<decltype(vec_)::value>;
                hipLaunchKernelGGL(kernel, cgrid, dim3(256), 0, st, batch_frames, counts->weights, loglik_out, cbuf, posterior_out,
                                   wt, counts->counts, t + 1, B, T, S, first);
            });
            if ((e = hipGetLastError()) != hipSuccess) return (int)e;
        }
        if ((e = fb_step<true>(observation, batch_frames, Et, m, cbuf, partial, loglik_out, posterior_out,
                               w + ((t + 1) & 1) * wrow, w + (t & 1) * wrow, t, B, T, S, true, cus, st)) != hipSuccess)
            return (int)e;
    }
    if (counts) {
        const size_t n = (size_t)S * S;
        const int grid = (int)std::min<size_t>((n + 255) / 256, 4096);
        hipLaunchKernelGGL(fb::fb_counts_finalize_kernel, dim3(grid), dim3(256), 0, st, E, counts->counts, S, T > 1 ? 1 : 0);
        if ((e = hipGetLastError()) != hipSuccess) return (int)e;
        hipLaunchKernelGGL(fb::fb_initial_counts_kernel, dim3((S + 255) / 256), dim3(256), 0, st, counts->weights,
                           loglik_out, posterior_out, counts->initial_counts, B, T, S);
        if ((e = hipGetLastError()) != hipSuccess) return (int)e;
    }
    return TORBI_HIP_OK;
}

int torbi_hip_forward_backward(const float *observation, const int32_t *batch_frames, const float *transition,
                               const float *initial, float *posterior_out, float *loglik_out, void *workspace,
                               size_t workspace_bytes, int B, int T, int S, int device, void *stream) {
    const int rc = fb_args_ok(observation, batch_frames, transition, initial, posterior_out, loglik_out, workspace,
                              workspace_bytes, B, T, S);
    if (rc != TORBI_HIP_OK || B == 0) return rc;
    return fb_dense(observation, batch_frames, transition, initial, posterior_out, loglik_out, workspace, B, T, S, device,
                    stream, nullptr);
}

size_t torbi_hip_forward_backward_counts_workspace_bytes(int B, int T, int S) {
    return torbi_hip_forward_backward_workspace_bytes(B, T, S);
}

int torbi_hip_forward_backward_counts(const float *observation, const int32_t *batch_frames, const float *transition,
                                      const float *initial, const float *item_weights, float *posterior_out,
                                      float *loglik_out, float *counts_out, float *initial_counts_out, void *workspace,
                                      size_t workspace_bytes, int B, int T, int S, int device, void *stream) {
    if (B > 0 && (!counts_out || !initial_counts_out)) return TORBI_HIP_EINVAL;
    const int rc = fb_args_ok(observation, batch_frames, transition, initial, posterior_out, loglik_out, workspace,
                              workspace_bytes, B, T, S);
    if (rc != TORBI_HIP_OK || B == 0) return rc;
    const FbCounts counts{item_weights, counts_out, initial_counts_out};
    return fb_dense(observation, batch_frames, transition, initial, posterior_out, loglik_out, workspace, B, T, S, device,
                    stream, &counts);
}

int torbi_hip_forward_backward_uniform(const float *observation, const int32_t *batch_frames, float uniform_value,
                                       const float *initial, float *posterior_out, float *loglik_out, void *workspace,
                                       size_t workspace_bytes, int B, int T, int S, int device, void *stream) {
    const int rc = fb_args_ok(observation, batch_frames, initial /* (no matrix) */, initial, posterior_out, loglik_out,
                              workspace, workspace_bytes, B, T, S);
    if (rc != TORBI_HIP_OK || B == 0) return rc;
    DeviceGuard guard(device);
    if (guard.err != hipSuccess) return (int)guard.err;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    double *lse = reinterpret_cast<double *>(fb_base(workspace));
    const size_t rows = (size_t)B * T;
    const bool vec = S % 4 == 0 && ((reinterpret_cast<uintptr_t>(observation) | reinterpret_cast<uintptr_t>(posterior_out)) & 15) == 0;
    by_flag(vec, [&](auto vec_) {
        auto *kernel = &fb::fb_uniform_rows_kernel<decltype(vec_)::value>;
        hipLaunchKernelGGL(kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, observation, batch_frames, initial,
                           posterior_out, lse, B, T, S);
    });
    hipError_t e;
    if ((e = hipGetLastError()) != hipSuccess) return (int)e;
    hipLaunchKernelGGL(fb::fb_uniform_loglik_kernel, dim3(B), dim3(256), 0, st, batch_frames, lse, uniform_value,
                       posterior_out, loglik_out, T, S);
    return (int)hipGetLastError();
}

// ---- posterior path sampling: forward filtering, backward sampling (sample.hpp) ----

// forward_backward's layout, then the filter rows a_t [B][T][S]
struct SampleLayout {
    fb::Layout fb;
    float *rows;
    size_t total;
};

static SampleLayout sample_layout(char *base, int B, int T, int S) {
    SampleLayout l;
    l.fb = fb::layout(base, B, T, S);
    Scratch a(base, l.fb.total - 256);
    l.rows = a.take<float>((size_t)B * T * S);
    l.total = a.bytes + 256;                 // (room to align the caller's base)
    return l;
}

size_t torbi_hip_sample_workspace_bytes(int B, int T, int S, int N, int uniform) {
    if (B < 1 || T < 1 || S < 1 || S > fb::kMaxStates || N < 1) return 256;
    if (uniform) return align_up((size_t)B * T * sizeof(double), 256) + 256;
    return sample_layout(nullptr, B, T, S).total;
}

static int sample_args_ok(const void *obs, const void *frames, const void *matrix, const void *initial, const void *uniforms,
                          const void *indices, const void *loglik, const void *ws, size_t ws_bytes, int B, int T, int S, int N,
                          int uniform) {
    if (B < 0 || T < 1 || S < 1 || N < 1 || N > sample::kMaxDraws) return TORBI_HIP_EINVAL;
    if (B == 0) return TORBI_HIP_OK;
    if (!obs || !frames || !matrix || !initial || !uniforms || !indices || !loglik || !ws) return TORBI_HIP_EINVAL;
    if (!fb_shape_in_range(B, T, S) || (size_t)B * N * T > (size_t)1 << 32) return TORBI_HIP_ERANGE;
    if (ws_bytes < torbi_hip_sample_workspace_bytes(B, T, S, N, uniform)) return TORBI_HIP_EWORKSPACE;
    return TORBI_HIP_OK;
}

int torbi_hip_sample(const float *observation, const int32_t *batch_frames, const float *transition, const float *initial,
                     const float *uniforms, int32_t *indices_out, float *loglik_out, void *workspace, size_t workspace_bytes,
                     int B, int T, int S, int N, int device, void *stream) {
    const int rc = sample_args_ok(observation, batch_frames, transition, initial, uniforms, indices_out, loglik_out, workspace,
                                  workspace_bytes, B, T, S, N, 0);
    if (rc != TORBI_HIP_OK || B == 0) return rc;
    DeviceGuard guard(device);
    if (guard.err != hipSuccess) return (int)guard.err;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const SampleLayout l = sample_layout(fb_base(workspace), B, T, S);
    const bool vec = S % 4 == 0;             // (the rows are 256-byte aligned in the workspace: fb_dense's rule)
    const int fwd = fb_forward(observation, batch_frames, transition, initial, l.rows, loglik_out, l.fb, B, T, S, vec,
                               cu_count(device), st);
    if (fwd != TORBI_HIP_OK) return fwd;
    // the HELD instance whose blocks cover S (a block: 256 states with float4 loads, 64 with scalar ones), else STREAMED
    const int block = vec ? 256 : 64, blocks = (S + block - 1) / block;
    int NB = 0;
    if (S <= (vec ? sample::kHeldStates : sample::kHeldStatesScalar))
        for (NB = 1; NB < blocks; NB *= 2) {}
    const dim3 grid(B, (N + sample::kWaves - 1) / sample::kWaves);
    auto launch = [&](auto *kernel) {
        hipLaunchKernelGGL(kernel, grid, dim3(64 * sample::kWaves), 0, st, l.rows, l.fb.E, batch_frames, loglik_out, uniforms,
                           indices_out, T, S, N);
    };
    if (vec) by_value<1, 2, 4, 8, 16, 0>(NB, [&](auto nb) { launch(&sample::sample_backward_kernel<true, decltype(nb)::value>); });
    else by_value<1, 2, 4, 8, 16, 32, 0>(NB, [&](auto nb) { launch(&sample::sample_backward_kernel<false, decltype(nb)::value>); });
    return (int)hipGetLastError();
}

int torbi_hip_sample_uniform(const float *observation, const int32_t *batch_frames, float uniform_value, const float *initial,
                             const float *uniforms, int32_t *indices_out, float *loglik_out, void *workspace,
                             size_t workspace_bytes, int B, int T, int S, int N, int device, void *stream) {
    const int rc = sample_args_ok(observation, batch_frames, initial /* (no matrix) */, initial, uniforms, indices_out,
                                  loglik_out, workspace, workspace_bytes, B, T, S, N, 1);
    if (rc != TORBI_HIP_OK || B == 0) return rc;
    DeviceGuard guard(device);
    if (guard.err != hipSuccess) return (int)guard.err;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    double *lse = reinterpret_cast<double *>(fb_base(workspace));
    const size_t rows = (size_t)B * T;
    const bool vec = S % 4 == 0 && ((reinterpret_cast<uintptr_t>(observation) | reinterpret_cast<uintptr_t>(initial)) & 15) == 0;
    by_flag(vec, [&](auto vec_) {
        auto *kernel = &sample::sample_uniform_rows_kernel<decltype(vec_)::value>;
        hipLaunchKernelGGL(kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, observation, batch_frames, initial, uniforms,
                           indices_out, lse, B, T, S, N);
    });
    hipError_t e;
    if ((e = hipGetLastError()) != hipSuccess) return (int)e;
    hipLaunchKernelGGL(fb::fb_uniform_loglik_kernel, dim3(B), dim3(256), 0, st, batch_frames, lse, uniform_value,
                       static_cast<float *>(nullptr), loglik_out, T, S);
    if ((e = hipGetLastError()) != hipSuccess) return (int)e;
    hipLaunchKernelGGL(sample::sample_mask_kernel, dim3(B), dim3(256), 0, st, loglik_out, indices_out, (size_t)N * T);
    return (int)hipGetLastError();
}

// ---- forward-backward on a band with one constant outside it (forward_backward_band.hpp) ----

// The checks of a band entry, in the order every one of them answers.  `pointers`: none of the entry's pointers is null;
// `covers` and `need`: what its own _covers and _workspace_bytes say; `valid` and `in_range`: what it asks beside the shape
// and the band.  TORBI_HIP_OK at B == 0 too, where the entry returns without a launch.
static int fb_band_args_ok(int B, int T, int S, int reach_left, int reach_right, bool pointers, int covers, size_t need,
                           size_t workspace_bytes, bool valid = true, bool in_range = true) {
    if (B < 0 || T < 1 || S < 1 || reach_left < 0 || reach_right < 0 || !valid) return TORBI_HIP_EINVAL;
    if (B == 0) return TORBI_HIP_OK;
    if (!pointers) return TORBI_HIP_EINVAL;
    if (!fb_shape_in_range(B, T, S) || !in_range) return TORBI_HIP_ERANGE;
    if (!covers) return TORBI_HIP_EUNSUPPORTED;
    if (workspace_bytes < need) return TORBI_HIP_EWORKSPACE;
    return TORBI_HIP_OK;
}

// What every band entry does first: switch to the device, then launch the diagonals of E - ebg with the promise flag, the
// check of the promise and the row maxima.  Holds the device for the entry's own launches; hands back ebg = exp(background)
// (0 for -inf) and the halo of the LDS rows.
struct BandPreamble {
    DeviceGuard guard;
    float ebg;
    int halo;
    hipError_t err;
    BandPreamble(const fbb::Layout &l, const float *observation, const int32_t *batch_frames, const float *transition,
                 const float *initial, float background, int B, int T, int S, int device, hipStream_t st)
        : guard(device), ebg(exp_background(background)), halo(l.halo), err(guard.err) {
        if (err != hipSuccess) return;
        if ((err = fbb::prepare_and_verify(transition, l, l.Df, l.Db, l.flag, ebg, background, S, st)) != hipSuccess) return;
        const size_t rows = (size_t)B * T;
        hipLaunchKernelGGL(fb::fb_rowmax_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, observation, batch_frames,
                           initial, l.m, B, T, S);
        err = hipGetLastError();
    }
};

// Items per workgroup of fb_band_kernel<G>: as many as the LDS rows let share one load of every diagonal, but no fewer
// workgroups than compute units while there are items for them.
static int fb_band_tile(int B, int S, int halo, int cus) {
    return items_per_workgroup(fbb::kMaxGroup, B, 1, cus, [&](int G) { return fbb::lds_bytes(G, S, halo) <= (size_t)fbb::kMaxLdsBytes; });
}

int torbi_hip_forward_backward_band_covers(int B, int T, int S, int reach_left, int reach_right, float background,
                                           int device) {
    (void)device;
    if (B < 1 || T < 1 || S < 1 || S > fbb::kMaxStates || reach_left < 0 || reach_right < 0) return 0;
    if (!background_ok(background)) return 0;
    if (!fb_shape_in_range(B, T, S)) return 0;
    const int W = fbb::band_of(S, reach_left, reach_right).W;
    return (W < S ? W : S) <= fbb::kMaxWindow ? 1 : 0;       // at most 64 in-band entries in a matrix row
}

size_t torbi_hip_forward_backward_band_workspace_bytes(int B, int T, int S, int reach_left, int reach_right) {
    if (B < 1 || T < 1 || S < 1 || S > fbb::kMaxStates || reach_left < 0 || reach_right < 0) return 256;
    return fbb::layout(nullptr, B, T, S, reach_left, reach_right).total;
}

int torbi_hip_forward_backward_band(const float *observation, const int32_t *batch_frames, const float *transition,
                                    const float *initial, int reach_left, int reach_right, float background,
                                    float *posterior_out, float *loglik_out, void *workspace, size_t workspace_bytes, int B,
                                    int T, int S, int device, void *stream) {
    const int rc = fb_band_args_ok(
        B, T, S, reach_left, reach_right,
        observation && batch_frames && transition && initial && posterior_out && loglik_out && workspace,
        torbi_hip_forward_backward_band_covers(B, T, S, reach_left, reach_right, background, device),
        torbi_hip_forward_backward_band_workspace_bytes(B, T, S, reach_left, reach_right), workspace_bytes);
    if (rc != TORBI_HIP_OK || B == 0) return rc;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const fbb::Layout l = fbb::layout(fb_base(workspace), B, T, S, reach_left, reach_right);
    const BandPreamble pre(l, observation, batch_frames, transition, initial, background, B, T, S, device, st);
    if (pre.err != hipSuccess) return (int)pre.err;
    const float ebg = pre.ebg;
    const int halo = pre.halo;
    const int G = fb_band_tile(B, S, halo, cu_count(device));
    const dim3 grid((B + G - 1) / G);
    const size_t lds = fbb::lds_bytes(G, S, halo);
    by_value<8, 4, 2, 1>(G, [&](auto g) {
        auto *kernel = &fbb::fb_band_kernel<decltype(g)::value>;
        hipLaunchKernelGGL(kernel, grid, dim3(fbb::kThreads), lds, st, observation, batch_frames, initial, l.Df, l.Db, l.m, l.c,
                           l.flag, posterior_out, loglik_out, ebg, l.reach_left, l.reach_right, l.W, l.Sd, B, T, S);
    });
    return (int)hipGetLastError();
}

// ---- expected counts on a band (counts_band.hpp) ----

// Items per workgroup of fb_band_counts_kernel<G>: fb_band_tile's rule with the plane beside the rows.
static int fb_band_counts_tile(int B, int S, int halo, int W, int cus) {
    return items_per_workgroup(fbb::kMaxGroup, B, 1, cus, [&](int G) {
        const size_t rows = fbb::lds_bytes(G, S, halo);
        return rows <= (size_t)fbb::kMaxLdsBytes && rows + fbb::plane_bytes(W, S) <= (size_t)fbb::kCountsLdsBytes;
    });
}

int torbi_hip_forward_backward_counts_band_covers(int B, int T, int S, int reach_left, int reach_right, float background,
                                                  int device) {
    if (!torbi_hip_forward_backward_band_covers(B, T, S, reach_left, reach_right, background, device)) return 0;
    const fbb::Band band = fbb::band_of(S, reach_left, reach_right);
    return fbb::lds_bytes(1, S, band.halo) + fbb::plane_bytes(band.W, S) <= (size_t)fbb::kCountsLdsBytes ? 1 : 0;
}

size_t torbi_hip_forward_backward_counts_band_workspace_bytes(int B, int T, int S, int reach_left, int reach_right) {
    if (B < 1 || T < 1 || S < 1 || S > fbb::kMaxStates || reach_left < 0 || reach_right < 0) return 256;
    return fbb::counts_layout(nullptr, B, T, S, reach_left, reach_right).total;
}

int torbi_hip_forward_backward_counts_band(const float *observation, const int32_t *batch_frames, const float *transition,
                                           const float *initial, int reach_left, int reach_right, float background,
                                           const float *item_weights, float *posterior_out, float *loglik_out,
                                           float *band_counts_out, float *initial_counts_out, void *workspace,
                                           size_t workspace_bytes, int B, int T, int S, int device, void *stream) {
    const int rc = fb_band_args_ok(
        B, T, S, reach_left, reach_right,
        observation && batch_frames && transition && initial && posterior_out && loglik_out && band_counts_out &&
            initial_counts_out && workspace,
        torbi_hip_forward_backward_counts_band_covers(B, T, S, reach_left, reach_right, background, device),
        torbi_hip_forward_backward_counts_band_workspace_bytes(B, T, S, reach_left, reach_right), workspace_bytes);
    if (rc != TORBI_HIP_OK || B == 0) return rc;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const fbb::CountsLayout l = fbb::counts_layout(fb_base(workspace), B, T, S, reach_left, reach_right);
    const BandPreamble pre(l, observation, batch_frames, transition, initial, background, B, T, S, device, st);
    if (pre.err != hipSuccess) return (int)pre.err;
    const float ebg = pre.ebg;
    const int halo = pre.halo;
    hipError_t e;
    const int G = fb_band_counts_tile(B, S, halo, l.W, cu_count(device));
    const int grid = std::min((B + G - 1) / G, fbb::kCountsWorkgroups);           // (<= l.planes)
    const size_t lds = fbb::lds_bytes(G, S, halo) + fbb::plane_bytes(l.W, S);
    e = by_value<8, 4, 2, 1>(G, [&](auto g) {
        auto *kernel = &fbb::fb_band_counts_kernel<decltype(g)::value>;
        const hipError_t le = ensure_dynamic_lds(kernel, lds);
        if (le != hipSuccess) return le;
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(fbb::kThreads), lds, st, observation, batch_frames, initial, l.Df, l.Db, l.m,
                           l.c, l.flag, item_weights, posterior_out, loglik_out, l.partial, ebg, l.reach_left, l.reach_right,
                           l.W, l.Sd, B, T, S);
        return hipGetLastError();
    });
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(fb::fb_initial_counts_kernel, dim3((S + 255) / 256), dim3(256), 0, st, item_weights, loglik_out,
                       posterior_out, initial_counts_out, B, T, S);
    if ((e = hipGetLastError()) != hipSuccess) return (int)e;
    hipLaunchKernelGGL(fbb::fb_band_counts_finalize_kernel, dim3((unsigned)(((size_t)l.W * S + 255) / 256)), dim3(256), 0, st,
                       transition, l.partial, l.flag, band_counts_out, initial_counts_out, grid, l.reach_left, l.W, l.Sd, S);
    return (int)hipGetLastError();
}

// ---- posterior path sampling on a band (sample_band.hpp) ----

int torbi_hip_sample_band_covers(int B, int T, int S, int N, int reach_left, int reach_right, float background, int device) {
    if (N < 1 || N > sample::kMaxDraws) return 0;
    return torbi_hip_forward_backward_band_covers(B, T, S, reach_left, reach_right, background, device);
}

size_t torbi_hip_sample_band_workspace_bytes(int B, int T, int S, int N, int reach_left, int reach_right) {
    (void)N;
    if (B < 1 || T < 1 || S < 1 || S > fbb::kMaxStates || reach_left < 0 || reach_right < 0) return 256;
    return fbb::sample_layout(nullptr, B, T, S, reach_left, reach_right).total;
}

int torbi_hip_sample_band(const float *observation, const int32_t *batch_frames, const float *transition, const float *initial,
                          int reach_left, int reach_right, float background, const float *uniforms, int32_t *indices_out,
                          float *loglik_out, void *workspace, size_t workspace_bytes, int B, int T, int S, int N, int device,
                          void *stream) {
    const int rc = fb_band_args_ok(
        B, T, S, reach_left, reach_right,
        observation && batch_frames && transition && initial && uniforms && indices_out && loglik_out && workspace,
        torbi_hip_sample_band_covers(B, T, S, N, reach_left, reach_right, background, device),
        torbi_hip_sample_band_workspace_bytes(B, T, S, N, reach_left, reach_right), workspace_bytes,
        N >= 1 && N <= sample::kMaxDraws, (size_t)B * N * T <= (size_t)1 << 32);
    if (rc != TORBI_HIP_OK || B == 0) return rc;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const fbb::SampleLayout l = fbb::sample_layout(fb_base(workspace), B, T, S, reach_left, reach_right);
    const BandPreamble pre(l, observation, batch_frames, transition, initial, background, B, T, S, device, st);
    if (pre.err != hipSuccess) return (int)pre.err;
    const float ebg = pre.ebg;
    const int halo = pre.halo;
    hipError_t e;
    const int G = fb_band_tile(B, S, halo, cu_count(device));            // (fb_band_kernel's tile: the same LDS rows)
    by_value<8, 4, 2, 1>(G, [&](auto g) {
        auto *kernel = &fbb::fb_band_filter_kernel<decltype(g)::value>;
        hipLaunchKernelGGL(kernel, dim3((B + G - 1) / G), dim3(fbb::kThreads), fbb::lds_bytes(G, S, halo), st, observation,
                           batch_frames, initial, l.Df, l.m, l.c, l.flag, l.rows, loglik_out, ebg, l.reach_left, l.reach_right,
                           l.W, l.Sd, B, T, S);
    });
    if ((e = hipGetLastError()) != hipSuccess) return (int)e;
    const dim3 grid(B, (N + sample::kWaves - 1) / sample::kWaves);
    by_flag(S % 4 == 0, [&](auto vec_) {          // (the rows are 256-byte aligned in the workspace)
        auto *kernel = &fbb::sample_band_backward_kernel<decltype(vec_)::value>;
        hipLaunchKernelGGL(kernel, grid, dim3(64 * sample::kWaves), 0, st, l.rows, transition, l.c, batch_frames, loglik_out,
                           uniforms, indices_out, ebg, l.reach_left, l.reach_right, T, S, N);
    });
    return (int)hipGetLastError();
}

// ---- k-best Viterbi decoding (k_best.hpp) ----

size_t torbi_hip_k_best_workspace_bytes(int B, int T, int S, int k) {
    if (B < 1 || T < 1 || S < 1 || S > kb::kMaxStates || k < 1 || k > kb::kMaxK) return 256;
    return kb::layout(nullptr, B, T, S, k).total;
}

static int kb_args_ok(const void *obs, const void *frames, const void *matrix, const void *initial, const void *indices,
                      const void *scores, const void *ws, size_t ws_bytes, int B, int T, int S, int k, int wS) {
    if (B < 0 || T < 1 || S < 1 || k < 1 || k > kb::kMaxK) return TORBI_HIP_EINVAL;
    if (B == 0) return TORBI_HIP_OK;
    if (!obs || !frames || !matrix || !initial || !indices || !scores || !ws) return TORBI_HIP_EINVAL;
    if (S > kb::kMaxStates || (size_t)B * T * S > (size_t)1 << 40 || (size_t)B * T > (size_t)1 << 32)
        return TORBI_HIP_ERANGE;
    if (ws_bytes < torbi_hip_k_best_workspace_bytes(B, T, wS, k)) return TORBI_HIP_EWORKSPACE;
    return TORBI_HIP_OK;
}

// One frame of the general route: KMAX = k rounded up to a power of two, G items per workgroup (G * KMAX <= 16 list
// entries per thread, at most 8 items, G rank-0 rows of LDS <= 64 KB: at most 129 VGPRs), but no fewer than
// kb::kStepWorkgroups workgroups while G > 1.  The rule depends on the shape and k only, not on the device.
static hipError_t kb_step(const float *obs, const int32_t *frames, const float *tt, const float *prev, float *cur,
                          int32_t *ptrs, int t, int B, int T, int S, int k, hipStream_t st) {
    int KMAX = 1;
    while (KMAX < k) KMAX *= 2;
    const int jblocks = (S + kb::kThreads - 1) / kb::kThreads;
    const int G = items_per_workgroup(std::min(8, std::max(1, 16 / KMAX)), B, jblocks, kb::kStepWorkgroups,
                                      [&](int g) { return (size_t)g * S * sizeof(float) <= (size_t)kb::kRowLdsBytes; });
    const int n = kb::list_length(k, S, t - 1), m = kb::list_length(k, S, t);
    const dim3 grid((B + G - 1) / G, jblocks);
    const size_t lds = (size_t)G * S * sizeof(float);
    by_value<1, 2, 4, 8, 16, 32>(KMAX, [&](auto kmax) { by_value<8, 4, 2, 1>(G, [&](auto g) {
        // an instance <KMAX, G> exists only while G * KMAX <= 16 list entries fit a thread; the host's G never exceeds that
        // (max_g above), so the clamp only keeps the other pairs of the two lists from being compiled
        constexpr int KM = decltype(kmax)::value, GI = decltype(g)::value * KM <= 16 ? decltype(g)::value : 1;
        auto *kernel = &kb::kb_step_kernel<KM, GI>;
        hipLaunchKernelGGL(kernel, grid, dim3(kb::kThreads), lds, st, obs, frames, tt, prev, cur, ptrs, t, B, T, S, k, n, m);
    }); });
    return hipGetLastError();
}

int torbi_hip_k_best(const float *observation, const int32_t *batch_frames, const float *transition, const float *initial,
                     int32_t *indices_out, float *scores_out, void *workspace, size_t workspace_bytes, int B, int T, int S,
                     int k, int device, void *stream) {
    const int rc = kb_args_ok(observation, batch_frames, transition, initial, indices_out, scores_out, workspace,
                              workspace_bytes, B, T, S, k, S);
    if (rc != TORBI_HIP_OK || B == 0) return rc;
    DeviceGuard guard(device);
    if (guard.err != hipSuccess) return (int)guard.err;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const kb::Layout l = kb::layout(fb_base(workspace), B, T, S, k);
    float *const vals = l.vals, *const tt = l.tt;
    int32_t *const ptrs = l.ptrs, *const count = l.count, *const flag = l.flag;
    kb::Final *const fin = l.final_;
    const size_t plane = (size_t)B * k * S;
    hipError_t e;
    if ((e = hipMemsetAsync(flag, 0, sizeof(int32_t), st)) != hipSuccess) return (int)e;
    hipLaunchKernelGGL(kb::kb_prepare_kernel, dim3((S + 31) / 32, (S + 31) / 32), dim3(256), 0, st, transition, tt, flag, S);
    if ((e = hipGetLastError()) != hipSuccess) return (int)e;
    hipLaunchKernelGGL(kb::kb_first_kernel, dim3(B, (S + 255) / 256), dim3(256), 0, st, observation, initial, vals, T, S, k);
    if ((e = hipGetLastError()) != hipSuccess) return (int)e;
    for (int t = 1; t < T; ++t)
        if ((e = kb_step(observation, batch_frames, tt, vals + ((t - 1) & 1) * plane, vals + (t & 1) * plane, ptrs, t, B,
                         T, S, k, st)) != hipSuccess)
            return (int)e;
    hipLaunchKernelGGL(kb::kb_final_kernel, dim3(B), dim3(kb::kThreads), 0, st, observation, batch_frames, initial, vals, fin,
                       count, flag, B, T, S, k);
    if ((e = hipGetLastError()) != hipSuccess) return (int)e;
    hipLaunchKernelGGL(kb::kb_walk_kernel<false>, dim3(B), dim3(64), 0, st, batch_frames, ptrs, fin, count, flag, indices_out,
                       scores_out, T, S, k);
    return (int)hipGetLastError();
}

int torbi_hip_k_best_uniform(const float *observation, const int32_t *batch_frames, float uniform_value,
                             const float *initial, int32_t *indices_out, float *scores_out, void *workspace,
                             size_t workspace_bytes, int B, int T, int S, int k, int device, void *stream) {
    const int rc = kb_args_ok(observation, batch_frames, initial /* (no matrix) */, initial, indices_out, scores_out,
                              workspace, workspace_bytes, B, T, S, k, 1);
    if (rc != TORBI_HIP_OK || B == 0) return rc;
    DeviceGuard guard(device);
    if (guard.err != hipSuccess) return (int)guard.err;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const kb::Layout l = kb::layout(fb_base(workspace), B, T, 1, k);
    int32_t *const ptrs = l.ptrs, *const count = l.count, *const flag = l.flag;
    kb::Final *const fin = l.final_;
    int KMAX = 1;
    while (KMAX < k) KMAX *= 2;
    by_value<1, 2, 4, 8, 16, 32>(KMAX, [&](auto kmax) {
        auto *kernel = &kb::kb_uniform_kernel<decltype(kmax)::value>;
        hipLaunchKernelGGL(kernel, dim3(B), dim3(64), 0, st, observation, batch_frames, uniform_value, initial, ptrs, fin, count, flag,
                           B, T, S, k);
    });
    hipError_t e;
    if ((e = hipGetLastError()) != hipSuccess) return (int)e;
    hipLaunchKernelGGL(kb::kb_walk_kernel<true>, dim3(B), dim3(64), 0, st, batch_frames, ptrs, fin, count, flag, indices_out,
                       scores_out, T, S, k);
    return (int)hipGetLastError();
}

// ---- k-best decoding on a band with one constant outside it (k_best_band.hpp) ----

int torbi_hip_k_best_band_covers(int B, int T, int S, int k, int reach_left, int reach_right, float background, int device) {
    (void)device;
    if (B < 1 || T < 1 || k < 1 || k > kb::kMaxK || reach_left < 0 || reach_right < 0) return 0;
    if (!banddiag::shape_ok(S, reach_left, reach_right)) return 0;
    if (kbb::lds_bytes(1, S, k, reach_left, reach_right) > (size_t)kbb::kMaxLdsBytes) return 0;
    return background_ok(background) ? 1 : 0;
}

size_t torbi_hip_k_best_band_workspace_bytes(int B, int T, int S, int k, int reach_left, int reach_right) {
    // (S up to the dense route's limit: the byte count of a shape the band route does not cover is still an answer)
    if (B < 1 || T < 1 || S < 1 || S > kb::kMaxStates || k < 1 || k > kb::kMaxK || !banddiag::window_ok(reach_left, reach_right))
        return 256;
    return kbb::layout(nullptr, B, T, S, k, reach_left, reach_right).total;
}

// Items per workgroup of kb_band_forward_kernel<KMAX, G>: from min(4, 16 / KMAX) (G * KMAX <= 16 list entries per thread),
// halved while the lists of G items do not fit the LDS, then while the launch has fewer than kbb::kWorkgroups workgroups.
// The rule reads the shape, k and the band only, not the device.
static int kb_band_items(int B, int S, int k, int KMAX, int reach_left, int reach_right) {
    return items_per_workgroup(std::min(kbb::kMaxGroup, std::max(1, 16 / KMAX)), B, 1, kbb::kWorkgroups, [&](int g) {
        return kbb::lds_bytes(g, S, k, reach_left, reach_right) <= (size_t)kbb::kMaxLdsBytes;
    });
}

int torbi_hip_k_best_band(const float *observation, const int32_t *batch_frames, const float *transition, const float *initial,
                          int reach_left, int reach_right, float background, int32_t *indices_out, float *scores_out,
                          void *workspace, size_t workspace_bytes, int B, int T, int S, int k, int device, void *stream) {
    if (B < 0 || T < 1 || S < 1 || k < 1 || k > kb::kMaxK || reach_left < 0 || reach_right < 0) return TORBI_HIP_EINVAL;
    if (B == 0) return TORBI_HIP_OK;
    if (!observation || !batch_frames || !transition || !initial || !indices_out || !scores_out || !workspace)
        return TORBI_HIP_EINVAL;
    if (!torbi_hip_k_best_band_covers(B, T, S, k, reach_left, reach_right, background, device)) return TORBI_HIP_EUNSUPPORTED;
    if ((size_t)B * T * S > (size_t)1 << 40 || (size_t)B * T > (size_t)1 << 32) return TORBI_HIP_ERANGE;
    if (workspace_bytes < torbi_hip_k_best_band_workspace_bytes(B, T, S, k, reach_left, reach_right)) return TORBI_HIP_EWORKSPACE;
    DeviceGuard guard(device);
    if (guard.err != hipSuccess) return (int)guard.err;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const kbb::Layout l = kbb::layout(fb_base(workspace), B, T, S, k, reach_left, reach_right);
    hipError_t e;
    if ((e = hipMemsetAsync(l.flag, 0, sizeof(int32_t), st)) != hipSuccess) return (int)e;
    if ((e = banddiag::prepare(transition, l.diag, l.ok, l.flag, background, reach_left, reach_right, S, st)) != hipSuccess)
        return (int)e;
    int KMAX = 1;
    while (KMAX < k) KMAX *= 2;
    const int G = kb_band_items(B, S, k, KMAX, reach_left, reach_right);
    const size_t lds = kbb::lds_bytes(G, S, k, reach_left, reach_right);
    const dim3 grid((B + G - 1) / G), block(kbb::forward_threads(S));
    e = by_value<1, 2, 4, 8, 16, 32>(KMAX, [&](auto kmax) { return by_value<4, 2, 1>(G, [&](auto g) {
        // (an instance <KMAX, G> exists only while G * KMAX <= 16; kb_band_items never exceeds that, so the clamp only keeps
        // the other pairs of the two lists from being compiled)
        constexpr int KM = decltype(kmax)::value, GI = decltype(g)::value * KM <= 16 ? decltype(g)::value : 1;
        auto *kernel = &kbb::kb_band_forward_kernel<KM, GI>;
        const hipError_t granted = ensure_dynamic_lds(kernel, lds);
        if (granted != hipSuccess) return granted;
        hipLaunchKernelGGL(kernel, grid, block, lds, st, observation, batch_frames, l.diag, initial, background, reach_left,
                           reach_right, l.vals, l.ptrs, B, T, S, k);
        return hipGetLastError();
    }); });
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(kb::kb_final_kernel, dim3(B), dim3(kb::kThreads), 0, st, observation, batch_frames, initial, l.vals,
                       l.final_, l.count, l.flag, B, T, S, k);
    if ((e = hipGetLastError()) != hipSuccess) return (int)e;
    hipLaunchKernelGGL(kbb::kb_band_verdict_kernel, dim3((B + 255) / 256), dim3(256), 0, st, l.ok, l.count, l.flag, B);
    if ((e = hipGetLastError()) != hipSuccess) return (int)e;
    hipLaunchKernelGGL(kb::kb_walk_kernel<false>, dim3(B), dim3(64), 0, st, batch_frames, l.ptrs, l.final_, l.count, l.flag,
                       indices_out, scores_out, T, S, k);
    return (int)hipGetLastError();
}

// ---- max-marginals: the best path score through every frame and state (max_marginals.hpp) ----

size_t torbi_hip_max_marginals_workspace_size(int B, int T, int S, int uniform) {
    if (B < 1 || T < 1 || S < 1 || S > mm::kMaxStates) return 256;
    return mm::layout(nullptr, B, T, S, uniform != 0).total;
}

static int mm_args_ok(const void *obs, const void *frames, const void *matrix, const void *initial, const void *marginals,
                      const void *scores, const void *ws, size_t ws_bytes, int B, int T, int S, int uniform) {
    if (B < 0 || T < 1 || S < 1) return TORBI_HIP_EINVAL;
    if (B == 0) return TORBI_HIP_OK;
    if (!obs || !frames || !matrix || !initial || !marginals || !scores || !ws) return TORBI_HIP_EINVAL;
    if (S > mm::kMaxStates || (size_t)B * T * S > (size_t)1 << 40 || (size_t)B * T > (size_t)1 << 32) return TORBI_HIP_ERANGE;
    if (ws_bytes < torbi_hip_max_marginals_workspace_size(B, T, S, uniform)) return TORBI_HIP_EWORKSPACE;
    return TORBI_HIP_OK;
}

int torbi_hip_max_marginals(const float *observation, const int32_t *batch_frames, const float *transition, const float *initial,
                            float *marginals_out, float *scores_out, void *workspace, size_t workspace_bytes, int B, int T,
                            int S, int device, void *stream) {
    const int rc = mm_args_ok(observation, batch_frames, transition, initial, marginals_out, scores_out, workspace,
                              workspace_bytes, B, T, S, 0);
    if (rc != TORBI_HIP_OK || B == 0) return rc;
    DeviceGuard guard(device);
    if (guard.err != hipSuccess) return (int)guard.err;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const mm::Layout l = mm::layout(fb_base(workspace), B, T, S, false);
    hipError_t e;
    if ((e = hipMemsetAsync(l.alarm, 0, ((size_t)B + 1) * sizeof(int32_t), st)) != hipSuccess) return (int)e;
    if (T > 1) {
        hipLaunchKernelGGL(mm::mm_prepare_kernel, dim3((S + 31) / 32, (S + 31) / 32), dim3(256), 0, st, transition, l.at,
                           l.alarm + B, S);
        if ((e = hipGetLastError()) != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(mm::mm_first_kernel, dim3(B, (S + 255) / 256), dim3(256), 0, st, observation, initial, marginals_out,
                       l.alarm, T, S);
    if ((e = hipGetLastError()) != hipSuccess) return (int)e;
    const dim3 grid((B + mm::kItemTile - 1) / mm::kItemTile, (S + mm::kRowTile - 1) / mm::kRowTile);
    const int groups = mm::step_groups((long)grid.x * grid.y);
    auto step = [&](auto backward, const float *panel, int t) {
        by_value<1, 2, 4>(groups, [&](auto kg) {
            auto *kernel = &mm::mm_step_kernel<decltype(backward)::value, decltype(kg)::value>;
            hipLaunchKernelGGL(kernel, grid, dim3(mm::kThreads * decltype(kg)::value), 0, st, observation, batch_frames, panel,
                               marginals_out, l.beta, l.alarm, t, B, T, S);
        });
        return hipGetLastError();
    };
    for (int t = 1; t < T; ++t)
        if ((e = step(std::false_type(), l.at, t)) != hipSuccess) return (int)e;
    for (int t = T - 2; t >= 0; --t)
        if ((e = step(std::true_type(), transition, t)) != hipSuccess) return (int)e;
    hipLaunchKernelGGL(mm::mm_final_kernel, dim3(B), dim3(256), 0, st, batch_frames, l.alarm, marginals_out, scores_out, B, T, S);
    return (int)hipGetLastError();
}

int torbi_hip_max_marginals_uniform(const float *observation, const int32_t *batch_frames, float uniform_value,
                                    const float *initial, float *marginals_out, float *scores_out, void *workspace,
                                    size_t workspace_bytes, int B, int T, int S, int device, void *stream) {
    const int rc = mm_args_ok(observation, batch_frames, initial /* (no matrix) */, initial, marginals_out, scores_out,
                              workspace, workspace_bytes, B, T, S, 1);
    if (rc != TORBI_HIP_OK || B == 0) return rc;
    DeviceGuard guard(device);
    if (guard.err != hipSuccess) return (int)guard.err;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const mm::Layout l = mm::layout(fb_base(workspace), B, T, S, true);
    hipError_t e;
    if ((e = hipMemsetAsync(l.alarm, 0, ((size_t)B + 1) * sizeof(int32_t), st)) != hipSuccess) return (int)e;
    const size_t rows = (size_t)B * T;
    const bool vec = S % 4 == 0 && ((reinterpret_cast<uintptr_t>(observation) | reinterpret_cast<uintptr_t>(marginals_out) |
                                     reinterpret_cast<uintptr_t>(initial)) & 15) == 0;
    by_flag(vec, [&](auto vec_) {
        auto *kernel = &mm::mm_uniform_rows_kernel<decltype(vec_)::value>;
        hipLaunchKernelGGL(kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, observation, batch_frames, initial, l.rows,
                           l.alarm, B, T, S);
    });
    if ((e = hipGetLastError()) != hipSuccess) return (int)e;
    hipLaunchKernelGGL(mm::mm_uniform_scan_kernel, dim3((B + 63) / 64), dim3(64), 0, st, batch_frames, l.rows, l.c, l.ubeta,
                       l.alarm, scores_out, uniform_value, !(uniform_value < INFINITY) ? 1 : 0, B, T);
    if ((e = hipGetLastError()) != hipSuccess) return (int)e;
    const size_t passes = (rows * S / (vec ? 4 : 1) + 255) / 256;
    const unsigned blocks = (unsigned)std::min<size_t>(std::max<size_t>(passes, 1), (size_t)cu_count(device) * 32);
    by_flag(vec, [&](auto vec_) {
        auto *kernel = &mm::mm_uniform_write_kernel<decltype(vec_)::value>;
        hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), 0, st, observation, batch_frames, initial, l.c, l.ubeta, l.alarm,
                           marginals_out, B, T, S);
    });
    return (int)hipGetLastError();
}

// ---- max-marginals on a band with one constant outside it (max_marginals_band.hpp) ----

int torbi_hip_max_marginals_band_covers(int B, int T, int S, int reach_left, int reach_right, float background, int device) {
    (void)device;
    if (B < 1 || T < 1 || reach_left < 0 || reach_right < 0) return 0;
    if (!banddiag::shape_ok(S, reach_left, reach_right)) return 0;
    if (mmb::lds_bytes(1, S, reach_left, reach_right) > (size_t)mmb::kMaxLdsBytes) return 0;
    return background_ok(background) ? 1 : 0;
}

size_t torbi_hip_max_marginals_band_workspace_size(int B, int T, int S, int reach_left, int reach_right) {
    // (S up to the dense route's limit, as torbi_hip_k_best_band_workspace_bytes)
    if (B < 1 || T < 1 || S < 1 || S > mm::kMaxStates || !banddiag::window_ok(reach_left, reach_right)) return 256;
    return mmb::layout(nullptr, B, S, reach_left, reach_right).total;
}

// Items per workgroup of mmb_kernel<G>: from mmb::kMaxGroup, halved while the rows and scans of G items do not fit the LDS,
// then while the launch has fewer than mmb::kWorkgroups workgroups.  The rule reads the shape and the band only.
static int mm_band_items(int B, int S, int reach_left, int reach_right) {
    return items_per_workgroup(mmb::kMaxGroup, B, 1, mmb::kWorkgroups, [&](int g) {
        return mmb::lds_bytes(g, S, reach_left, reach_right) <= (size_t)mmb::kMaxLdsBytes;
    });
}

int torbi_hip_max_marginals_band(const float *observation, const int32_t *batch_frames, const float *transition,
                                 const float *initial, int reach_left, int reach_right, float background, float *marginals_out,
                                 float *scores_out, void *workspace, size_t workspace_bytes, int B, int T, int S, int device,
                                 void *stream) {
    if (B < 0 || T < 1 || S < 1 || reach_left < 0 || reach_right < 0) return TORBI_HIP_EINVAL;
    if (B == 0) return TORBI_HIP_OK;
    if (!observation || !batch_frames || !transition || !initial || !marginals_out || !scores_out || !workspace)
        return TORBI_HIP_EINVAL;
    if (S > mm::kMaxStates || (size_t)B * T * S > (size_t)1 << 40 || (size_t)B * T > (size_t)1 << 32) return TORBI_HIP_ERANGE;
    if (!torbi_hip_max_marginals_band_covers(B, T, S, reach_left, reach_right, background, device)) return TORBI_HIP_EUNSUPPORTED;
    if (workspace_bytes < torbi_hip_max_marginals_band_workspace_size(B, T, S, reach_left, reach_right)) return TORBI_HIP_EWORKSPACE;
    DeviceGuard guard(device);
    if (guard.err != hipSuccess) return (int)guard.err;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const mmb::Layout l = mmb::layout(fb_base(workspace), B, S, reach_left, reach_right);
    hipError_t e;
    if ((e = hipMemsetAsync(l.alarm, 0, ((size_t)B + 1) * sizeof(int32_t), st)) != hipSuccess) return (int)e;
    if ((e = banddiag::prepare(transition, l.diag, l.ok, l.alarm + B, background, reach_left, reach_right, S, st)) != hipSuccess)
        return (int)e;
    const int G = mm_band_items(B, S, reach_left, reach_right);
    const size_t lds = mmb::lds_bytes(G, S, reach_left, reach_right);
    e = by_flag(background != -INFINITY, [&](auto scan) { return by_value<4, 2, 1>(G, [&](auto g) {
        auto *kernel = &mmb::mmb_kernel<decltype(g)::value, decltype(scan)::value>;
        const hipError_t granted = ensure_dynamic_lds(kernel, lds);
        if (granted != hipSuccess) return granted;
        hipLaunchKernelGGL(kernel, dim3((B + G - 1) / G), dim3(mmb::kThreads), lds, st, observation, batch_frames, l.diag, initial,
                           background, reach_left, reach_right, marginals_out, scores_out, l.alarm, B, T, S);
        return hipGetLastError();
    }); });
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(mmb::mmb_final_kernel, dim3(B), dim3(256), 0, st, batch_frames, l.alarm, l.ok, marginals_out, scores_out,
                       B, T, S);
    return (int)hipGetLastError();
}

// ---- path statistics: exact scores and counts of given state paths (path_statistics.hpp) ----

size_t torbi_hip_path_statistics_workspace_size(int B, int T, int S, int K, int counts) {
    if (!counts) return 0;
    if (B < 1 || T < 1 || S < 1 || K < 1 || S > ps::kMaxStates) return 256;
    return ps::layout(nullptr, S, true).total;
}

int torbi_hip_path_statistics(const float *observation, const int32_t *batch_frames, const float *transition, float uniform_value,
                              const float *initial, const int32_t *indices, const float *path_weights, float *scores_out,
                              float *transition_counts_out, float *initial_counts_out, void *workspace, size_t workspace_bytes,
                              int B, int T, int S, int K, int device, void *stream) {
    if (B < 0 || T < 1 || S < 1 || K < 1) return TORBI_HIP_EINVAL;
    const bool counting = transition_counts_out != nullptr;
    if (counting != (initial_counts_out != nullptr) || (!counting && !scores_out)) return TORBI_HIP_EINVAL;
    if (!batch_frames || !indices || (scores_out && (!observation || !initial)) || (counting && !workspace))
        return TORBI_HIP_EINVAL;
    if (B == 0) return TORBI_HIP_OK;
    const size_t paths = (size_t)B * K;
    if (S > ps::kMaxStates || paths > ((size_t)1 << 31) - ps::kWaves || paths * T > (size_t)1 << 40 ||
        (size_t)B * T * S > (size_t)1 << 40)
        return TORBI_HIP_ERANGE;
    if (workspace_bytes < torbi_hip_path_statistics_workspace_size(B, T, S, K, counting ? 1 : 0)) return TORBI_HIP_EWORKSPACE;
    DeviceGuard guard(device);
    if (guard.err != hipSuccess) return (int)guard.err;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const ps::Layout l = ps::layout(counting ? fb_base(workspace) : nullptr, S, counting);
    hipError_t e;
    if (counting && (e = hipMemsetAsync(l.x, 0, l.zeroed, st)) != hipSuccess) return (int)e;
    hipLaunchKernelGGL(ps::ps_kernel, dim3((unsigned)((paths + ps::kWaves - 1) / ps::kWaves)), dim3(ps::kThreads), 0, st,
                       observation, batch_frames, transition, uniform_value, initial, indices, path_weights, scores_out, l.x, l.i,
                       B, T, S, K);
    if ((e = hipGetLastError()) != hipSuccess || !counting) return (int)e;
    const size_t passes = ((size_t)S * S + S + 255) / 256;
    const unsigned blocks = (unsigned)std::min<size_t>(passes, (size_t)cu_count(device) * 32);
    hipLaunchKernelGGL(ps::ps_round_kernel, dim3(blocks), dim3(256), 0, st, l.x, l.i, transition_counts_out, initial_counts_out, S);
    return (int)hipGetLastError();
}

// ---- path entropy: the entropy of the posterior over whole state paths (path_entropy.hpp) ----

size_t torbi_hip_path_entropy_workspace_size(int B, int T, int S, int uniform) {
    if (B < 1 || T < 1 || S < 1 || S > pe::kMaxStates) return 256;
    return pe::layout(nullptr, B, T, S, uniform != 0).total;
}

static int pe_args_ok(const void *obs, const void *frames, const void *matrix, const void *initial, const void *entropy,
                      const void *loglik, const void *ws, size_t ws_bytes, int B, int T, int S, int uniform) {
    if (B < 0 || T < 1 || S < 1) return TORBI_HIP_EINVAL;
    if (B == 0) return TORBI_HIP_OK;
    if (!obs || !frames || !matrix || !initial || !entropy || !loglik || !ws) return TORBI_HIP_EINVAL;
    if (!fb_shape_in_range(B, T, S)) return TORBI_HIP_ERANGE;
    if (ws_bytes < torbi_hip_path_entropy_workspace_size(B, T, S, uniform)) return TORBI_HIP_EWORKSPACE;
    return TORBI_HIP_OK;
}

int torbi_hip_path_entropy(const float *observation, const int32_t *batch_frames, const float *transition, const float *initial,
                           float *entropy_out, float *prefix_out, float *loglik_out, void *workspace, size_t workspace_bytes,
                           int B, int T, int S, int device, void *stream) {
    const int rc = pe_args_ok(observation, batch_frames, transition, initial, entropy_out, loglik_out, workspace,
                              workspace_bytes, B, T, S, 0);
    if (rc != TORBI_HIP_OK || B == 0) return rc;
    DeviceGuard guard(device);
    if (guard.err != hipSuccess) return (int)guard.err;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const pe::Layout l = pe::layout(fb_base(workspace), B, T, S, false);
    float *const prefix = prefix_out ? prefix_out : l.prefix;
    const size_t xrow = (size_t)B * fb::padded_states(S), prow = (size_t)B * fb::partials_of(S);
    hipError_t e;
    if (T > 1) {
        const size_t n = (size_t)fb::padded_rows(S) * fb::padded_states(S);
        const int grid = (int)std::min<size_t>((n + 255) / 256, 4096);
        hipLaunchKernelGGL(pe::pe_prepare_kernel, dim3(grid), dim3(256), 0, st, transition, l.E, l.G, S);
        if ((e = hipGetLastError()) != hipSuccess) return (int)e;
    }
    const size_t nrows = (size_t)B * T;
    hipLaunchKernelGGL(fb::fb_rowmax_kernel, dim3((unsigned)((nrows + 3) / 4)), dim3(256), 0, st, observation, batch_frames,
                       initial, l.m, B, T, S);
    if ((e = hipGetLastError()) != hipSuccess) return (int)e;
    hipLaunchKernelGGL(pe::pe_first_kernel, dim3(B, (S + 255) / 256), dim3(256), 0, st, observation, initial, l.m, l.p, l.u,
                       l.partial, T, S);
    if ((e = hipGetLastError()) != hipSuccess) return (int)e;
    // One step launch: 32 x 32 tiles (states x items).  With at least two tiles per compute unit, four waves per tile stage
    // the operands through LDS; with fewer, the waves read their chunks from global memory.  K is split over pe::waves_of(S)
    // waves in both forms, chunk by chunk alike, so an item's bits do not depend on the form, that is on the batch size.
    const unsigned tiles = (unsigned)((S + 31) / 32) * (unsigned)((B + 31) / 32);
    const dim3 grid((S + 31) / 32, (B + 31) / 32);
    const int KS = pe::waves_of(S);
    const bool staged = KS == pe::kMaxWaves && tiles >= 2u * cu_count(device);
    for (int t = 0; t < T; ++t) {
        const int now = t & 1, before = now ^ 1;
        if (t > 0) {
            by_flag(staged, [&](auto staged_) {
                auto *kernel = &pe::pe_step_kernel<decltype(staged_)::value>;
                hipLaunchKernelGGL(kernel, grid, dim3(64 * KS), 0, st, observation, batch_frames, l.E, l.G, l.m, l.p + before * xrow,
                                   l.u + before * xrow, l.p + now * xrow, l.u + now * xrow, l.partial + now * prow, t, B, T, S, KS);
            });
            if ((e = hipGetLastError()) != hipSuccess) return (int)e;
        }
        hipLaunchKernelGGL(pe::pe_item_kernel, dim3(B), dim3(256), 0, st, batch_frames, l.partial + now * prow, l.p + now * xrow,
                           l.u + now * xrow, l.c, prefix, t, T, S);
        if ((e = hipGetLastError()) != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(pe::pe_final_kernel, dim3(B), dim3(256), 0, st, batch_frames, l.m, l.c, prefix, entropy_out, loglik_out, T);
    return (int)hipGetLastError();
}

int torbi_hip_path_entropy_uniform(const float *observation, const int32_t *batch_frames, float uniform_value,
                                   const float *initial, float *entropy_out, float *prefix_out, float *loglik_out,
                                   void *workspace, size_t workspace_bytes, int B, int T, int S, int device, void *stream) {
    const int rc = pe_args_ok(observation, batch_frames, initial /* (no matrix) */, initial, entropy_out, loglik_out, workspace,
                              workspace_bytes, B, T, S, 1);
    if (rc != TORBI_HIP_OK || B == 0) return rc;
    DeviceGuard guard(device);
    if (guard.err != hipSuccess) return (int)guard.err;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const pe::Layout l = pe::layout(fb_base(workspace), B, T, S, true);
    const size_t rows = (size_t)B * T;
    const bool vec = S % 4 == 0 && (reinterpret_cast<uintptr_t>(observation) & 15) == 0;
    by_flag(vec, [&](auto vec_) {
        auto *kernel = &pe::pe_uniform_rows_kernel<decltype(vec_)::value>;
        hipLaunchKernelGGL(kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, observation, batch_frames, initial, l.rowh,
                           l.lse, B, T, S);
    });
    hipError_t e;
    if ((e = hipGetLastError()) != hipSuccess) return (int)e;
    hipLaunchKernelGGL(pe::pe_uniform_scan_kernel, dim3((B + 63) / 64), dim3(64), 0, st, batch_frames, l.rowh, l.lse,
                       uniform_value, entropy_out, prefix_out, loglik_out, B, T);
    return (int)hipGetLastError();
}

// ---- path entropy on a band with one constant outside it (path_entropy_band.hpp) ----

int torbi_hip_path_entropy_band_covers(int B, int T, int S, int reach_left, int reach_right, float background, int device) {
    if (!torbi_hip_forward_backward_band_covers(B, T, S, reach_left, reach_right, background, device)) return 0;
    // (one item's rows: true of every shape the window admits, peb::kMaxLdsBytes says why)
    return peb::lds_bytes(1, S, fbb::band_of(S, reach_left, reach_right).halo) <= (size_t)peb::kMaxLdsBytes ? 1 : 0;
}

size_t torbi_hip_path_entropy_band_workspace_size(int B, int T, int S, int reach_left, int reach_right) {
    if (B < 1 || T < 1 || S < 1 || S > peb::kMaxStates || reach_left < 0 || reach_right < 0) return 256;
    return peb::layout(nullptr, B, T, S, reach_left, reach_right).total;
}

// Items per workgroup of pe_band_kernel<G>: fb_band_tile's rule with the pairs in the place of the rows.
static int pe_band_tile(int B, int S, int halo, int cus) {
    return items_per_workgroup(peb::kMaxGroup, B, 1, cus, [&](int G) { return peb::lds_bytes(G, S, halo) <= (size_t)peb::kMaxLdsBytes; });
}

int torbi_hip_path_entropy_band(const float *observation, const int32_t *batch_frames, const float *transition,
                                const float *initial, int reach_left, int reach_right, float background, float *entropy_out,
                                float *prefix_out, float *loglik_out, void *workspace, size_t workspace_bytes, int B, int T, int S,
                                int device, void *stream) {
    const int rc = fb_band_args_ok(
        B, T, S, reach_left, reach_right,
        observation && batch_frames && transition && initial && entropy_out && loglik_out && workspace,
        torbi_hip_path_entropy_band_covers(B, T, S, reach_left, reach_right, background, device),
        torbi_hip_path_entropy_band_workspace_size(B, T, S, reach_left, reach_right), workspace_bytes);
    if (rc != TORBI_HIP_OK || B == 0) return rc;
    DeviceGuard guard(device);
    if (guard.err != hipSuccess) return (int)guard.err;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const peb::Layout l = peb::layout(fb_base(workspace), B, T, S, reach_left, reach_right);
    const float ebg = exp_background(background), gbg = background == -INFINITY ? 0.f : ebg * background;
    hipError_t e;
    if ((e = peb::prepare_and_verify(transition, l, ebg, gbg, background, S, st)) != hipSuccess) return (int)e;
    const size_t rows = (size_t)B * T;
    hipLaunchKernelGGL(fb::fb_rowmax_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, observation, batch_frames, initial,
                       l.m, B, T, S);
    if ((e = hipGetLastError()) != hipSuccess) return (int)e;
    const int G = pe_band_tile(B, S, l.halo, cu_count(device));
    const size_t lds = peb::lds_bytes(G, S, l.halo);
    float *const prefix = prefix_out ? prefix_out : l.prefix;
    e = by_value<4, 2, 1>(G, [&](auto g) {
        auto *kernel = &peb::pe_band_kernel<decltype(g)::value>;
        const hipError_t granted = ensure_dynamic_lds(kernel, lds);
        if (granted != hipSuccess) return granted;
        hipLaunchKernelGGL(kernel, dim3((B + G - 1) / G), dim3(peb::kThreads), lds, st, observation, batch_frames, initial, l.Df,
                           l.Dg, l.m, l.c, l.flag, prefix, entropy_out, loglik_out, ebg, gbg, l.reach_left, l.reach_right, l.W,
                           l.Sd, B, T, S);
        return hipGetLastError();
    });
    return (int)e;
}

}  // extern "C"

#ifdef BAND_STAMP
// instrumentation build only (tools/band_stamps.py); not part of include/torbi_hip.h
extern "C" int torbi_hip_debug_band_phases(unsigned long long *host, size_t count) {
    return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(band::g_phase), count * sizeof(unsigned long long));
}
#endif
#ifdef RESIDENT_STAMP
// instrumentation build only (tools/resident_stamps.py); not part of include/torbi_hip.h
extern "C" int torbi_hip_debug_phases(unsigned long long *host, size_t count) {
    return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(resident::g_phase), count * sizeof(unsigned long long));
}
extern "C" int torbi_hip_debug_wgtime(unsigned long long *host, size_t count) {
    return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(resident::g_wgtime), count * sizeof(unsigned long long));
}
#endif
