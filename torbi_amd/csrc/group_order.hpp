// group_order.hpp -- the order a launch group is decoded in: every batch's items ranked by length, the group's tiles ranked
// by the length of their longest item.  assemble_group (torbi_hip.hip) runs these kernels ahead of the forward launch of the
// time-resident route (resident_forward.hpp) and of the band route alike; they stay in namespace `resident`, where they
// were written.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace resident {

constexpr int kMaxBatches = 16;    // batches one launch can carry

// once per decode: order[rank] = item, items ranked by descending (clamped) length, ties by item number.  A tile of
// 16 consecutive ranks then loops to the longest of 16 items of SIMILAR length -- a ragged batch costs recurrence
// steps for its valid frames only (collate pads every item of a 512-batch to the batch maximum: reference
// torbi/data/collate.py:24-31) -- and the longest tiles are dispatched first.  Results do not depend on the order.
// grid = (ceil(max B / 256), batches), block = 256; O(B^2) compares up to kMaxOrdered items; larger batches are ranked by
// a counting sort over the lengths (order_large_* below: items of equal length in arrival order of their atomics --
// which of two equally long items lands in which tile changes nothing, neither results nor work).
constexpr int kMaxOrdered = 8192;
struct OrderJob { const int32_t *frames; int32_t *order; int B, T, tile0; int32_t *hist; int32_t *route_record; int route; };
struct OrderJobs { OrderJob job[kMaxBatches]; int ascending; int n; int tiles; int32_t *tile_map; unsigned *stats;
                   unsigned *flags; int nflags;         // cluster form: the flag / ticket words to zero (else nflags = 0)
                   int ni; };                           // items per tile (16, or 8 above kMaxS16 states)

// (The clamped lengths are staged in the LDS, kOrderChunk at a time, and every thread ranks its item against the chunk from
// there, four lengths a read: a thread that read frames[o] from memory for every o took 35 us for 512 items.)
constexpr int kOrderChunk = 2048;
__global__ __launch_bounds__(256) void order_items_kernel(OrderJobs jobs) {
    __shared__ __align__(16) int s_len[kOrderChunk];
    const OrderJob &jb = jobs.job[blockIdx.y];
    const int b = blockIdx.x * 256 + threadIdx.x;
    const int B = jb.B, T = jb.T;
    if (b == 0 && jb.route_record) *jb.route_record = jb.route;      // the route this batch's decode takes (torbi_hip.hip)
    if ((int)blockIdx.x * 256 >= B) return;          // (the whole block: nobody is missed at the barriers below)
    if (B > kMaxOrdered) return;                     // order_large_* rank this batch
    int f = b < B ? jb.frames[b] : 1;
    f = f < 1 ? 1 : (f > T ? T : f);
    int rank = 0;
    for (int o0 = 0; o0 < B; o0 += kOrderChunk) {
        const int n = min(kOrderChunk, B - o0), n4 = (n + 3) / 4 * 4;
        if (o0) __syncthreads();
        for (int o = threadIdx.x; o < n4; o += 256) {
            int g = o < n ? jb.frames[o0 + o] : 0;   // (length 0 ranks behind every item: the chunk's padding counts nothing)
            s_len[o] = o < n ? (g < 1 ? 1 : (g > T ? T : g)) : 0;
        }
        __syncthreads();
        for (int o = 0; o < n4; o += 4) {
            const int4 g = *reinterpret_cast<const int4 *>(&s_len[o]);
            rank += (g.x > f) || (g.x == f && o0 + o < b);
            rank += (g.y > f) || (g.y == f && o0 + o + 1 < b);
            rank += (g.z > f) || (g.z == f && o0 + o + 2 < b);
            rank += (g.w > f) || (g.w == f && o0 + o + 3 < b);
        }
    }
    if (b < B) jb.order[jobs.ascending ? B - 1 - rank : rank] = b;
}

// Batches above kMaxOrdered items: hist[f] = items of (clamped) length f (zeroed by the host), turned into the first rank
// of every length by one block, then every item takes the next rank of its length.
__global__ __launch_bounds__(256) void order_large_count_kernel(OrderJob jb) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= jb.B) return;
    int f = jb.frames[b];
    f = f < 1 ? 1 : (f > jb.T ? jb.T : f);
    atomicAdd(&jb.hist[f], 1);
}

__global__ __launch_bounds__(1024) void order_large_scan_kernel(OrderJob jb, int ascending) {
    // hist[f] <- number of items that rank before the items of length f (longer ones; shorter ones when ascending)
    __shared__ int part[1024];
    const int T = jb.T, tid = threadIdx.x;
    const int per = (T + 1024) / 1024;                       // lengths 1..T in 1024 contiguous chunks, in rank order
    auto length_at = [&](int k) { return ascending ? 1 + k : T - k; };      // k-th length in rank order
    int sum = 0;
    for (int k = tid * per; k < (tid + 1) * per && k < T; ++k) sum += jb.hist[length_at(k)];
    part[tid] = sum;
    __syncthreads();
    if (tid == 0) {
        int run = 0;
        for (int i = 0; i < 1024; ++i) { const int v = part[i]; part[i] = run; run += v; }
    }
    __syncthreads();
    int run = part[tid];
    for (int k = tid * per; k < (tid + 1) * per && k < T; ++k) {
        const int f = length_at(k), v = jb.hist[f];
        jb.hist[f] = run;
        run += v;
    }
}

__global__ __launch_bounds__(256) void order_large_place_kernel(OrderJob jb) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= jb.B) return;
    int f = jb.frames[b];
    f = f < 1 ? 1 : (f > jb.T ? jb.T : f);
    jb.order[atomicAdd(&jb.hist[f], 1)] = b;
}

// ... and the group's TILES by descending length of their longest item: workgroup w decodes tile_map[w].  The GPU hands
// workgroup i to shader engine i mod 32 and waits, in launch order, for a free CU THERE (tools/dispatch_probe.hip,
// tools/resident_wgtime.py): with batch-major numbering the rank-c tiles of all batches -- all of one length -- meet on
// one engine, the engine of the longest tiles is the one the first workgroup beyond the 256th waits for, and nothing
// behind it starts until those finish (measured: 28.3 ms for a ragged 16-batch group that has 16.5 ms of work per CU).
// Ranked across the whole group, every engine holds an even spread of lengths and frees a CU early.
// One thread per tile; grid = ceil(tiles / 256); O(tiles^2) compares.  Runs after order_items_kernel.
// (Every tile's length is two dependent loads, frames[order[.]]: the block fetches them once, kOrderChunk tiles at a time,
// into the LDS and ranks from there -- a thread that fetched all of them itself took 60 us for 256 tiles.)
__global__ __launch_bounds__(256) void order_tiles_kernel(OrderJobs jobs) {
    __shared__ __align__(16) int s_len[kOrderChunk];
    const int w = blockIdx.x * 256 + threadIdx.x;
    if (w < 128) jobs.stats[w] = 0u;                 // the forward launch that follows accumulates into them
    for (int k = w; k < jobs.nflags; k += gridDim.x * 256) jobs.flags[k] = 0u;     // cluster flags and tickets start at zero
    if ((int)blockIdx.x * 256 >= jobs.tiles) return;          // (the whole block)
    auto batch_of_tile = [&](int v) {
        int k = 0;
        for (int q = 1; q < jobs.n; ++q)
            if (v >= jobs.job[q].tile0) k = q;
        return k;
    };
    auto tile_length = [&](int k, int j) {
        const OrderJob &jb = jobs.job[k];
        // the longest item of tile j: its first in descending order, its last (within the batch) in ascending order
        const int last = jobs.ni * j + jobs.ni - 1 < jb.B ? jobs.ni * j + jobs.ni - 1 : jb.B - 1;
        int f = jb.frames[jb.order[jobs.ascending ? last : jobs.ni * j]];
        return f < 1 ? 1 : (f > jb.T ? jb.T : f);
    };
    const bool live = w < jobs.tiles;
    const int k = live ? batch_of_tile(w) : 0;
    const int j = w - jobs.job[k].tile0;
    const int mine = live ? tile_length(k, j) : 1;
    int rank = 0;
    for (int v0 = 0; v0 < jobs.tiles; v0 += kOrderChunk) {
        const int n = min(kOrderChunk, jobs.tiles - v0), n4 = (n + 3) / 4 * 4;
        if (v0) __syncthreads();
        for (int v = threadIdx.x; v < n4; v += 256) {
            const int kv = v < n ? batch_of_tile(v0 + v) : 0;
            s_len[v] = v < n ? tile_length(kv, v0 + v - jobs.job[kv].tile0) : 0;      // (0: behind every tile, counts nothing)
        }
        __syncthreads();
        for (int v = 0; v < n4; v += 4) {
            const int4 g = *reinterpret_cast<const int4 *>(&s_len[v]);
            rank += (g.x > mine) || (g.x == mine && v0 + v < w);
            rank += (g.y > mine) || (g.y == mine && v0 + v + 1 < w);
            rank += (g.z > mine) || (g.z == mine && v0 + v + 2 < w);
            rank += (g.w > mine) || (g.w == mine && v0 + v + 3 < w);
        }
    }
    if (live) jobs.tile_map[jobs.ascending ? jobs.tiles - 1 - rank : rank] = (k << 20) | j;
}

}  // namespace resident
