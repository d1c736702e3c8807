// scratch.hpp -- the one way a device workspace is cut into regions: every layout of the library states each region once, as a
// take<T>(count), and reads its byte count off the cursor.  A null base lays out nothing and only counts (the size queries).
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>

__host__ __device__ inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

struct Scratch {
    char *base;        // null: a size query
    size_t bytes;      // the cursor: where the next region starts, and behind the last take the layout's total
    explicit Scratch(void *base_, size_t from = 0) : base(static_cast<char *>(base_)), bytes(from) {}
    // `count` elements of T at the cursor; the cursor moves on to the next multiple of 256 (`align`: the streaming state packs)
    template <typename T>
    T *take(size_t count, size_t align = 256) {
        T *const here = base ? reinterpret_cast<T *>(base + bytes) : nullptr;
        bytes = align_up(bytes + count * sizeof(T), align);
        return here;
    }
};

// a named part of a region that was taken as one run: `n` elements behind its start (null stays null)
template <typename T>
inline T *behind(T *region, size_t n) { return region ? region + n : nullptr; }
