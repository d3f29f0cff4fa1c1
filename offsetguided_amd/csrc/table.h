// Tensor tables: what the one-launch-over-many-tensors kernels share (optim.hip, fold.hip, range.hip; the host side is
// offsetguided_amd/_table.py).  A table is `rows` (a fixed number of int64 words per row: addresses as integers, sizes, flags)
// followed by `prefix`, an int32 running sum of the rows' workgroup counts with prefix[0] = 0 and prefix[n_rows] = the grid.  The host
// fills it in pinned memory and copies it once; workgroup `wg` finds its row by bisection and is workgroup wg - prefix[row] of it.
#pragma once
#include "og_common.h"

// A table holds addresses as integers: the pointers made from them are given the global address space, so the loads and stores are
// global_* instructions and not flat_* ones (a generic pointer would be checked against the LDS and scratch apertures).
typedef __attribute__((address_space(1))) void gvoid;
typedef __attribute__((address_space(1))) unsigned char gu8;
typedef __attribute__((address_space(1))) unsigned short gu16;
typedef __attribute__((address_space(1))) unsigned int gu32;
typedef __attribute__((address_space(1))) float gfloat;
typedef float f4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) f4 gf4;
typedef unsigned int u4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) u4 gu4;

// Row of workgroup `wg`: the largest r < n_rows with prefix[r] <= wg.  Rows without workgroups (prefix[r] == prefix[r + 1]) are
// passed over: of a run of equal prefix values the last row is taken, and that one has workgroups.
__device__ __forceinline__ int og_find_row(const int32_t *prefix, int n_rows, int wg)
{
    int lo = 0, hi = n_rows;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (prefix[mid] <= wg) lo = mid;
        else hi = mid;
    }
    return lo;
}

// The 16-byte frame over a run of n elements at p (any element-aligned address): elements [0, head) up to the first 16-byte boundary,
// n_vec whole vectors from there, elements [tail, n) behind them.  Every vector lies inside the run: nothing outside it is read.
struct OgFrame {
    int head, n_vec, tail;
};

// elem_bytes: 4 or 2
__device__ __forceinline__ OgFrame og_frame(const gvoid *p, int n, int elem_bytes)
{
    const int shift = elem_bytes == 4 ? 2 : 1;
    const int to_boundary = (int)(((16u - (unsigned)((uintptr_t)p & 15u)) & 15u) >> shift);
    OgFrame f;
    f.head = to_boundary < n ? to_boundary : n;
    const int per = 16 >> shift;
    f.n_vec = (n - f.head) / per;
    f.tail = f.head + f.n_vec * per;
    return f;
}

// The scalar element of this thread, or -1: the head on threads 0.., the tail on threads 64.. (another wave).  Each edge is shorter
// than a vector, so no thread has two.
__device__ __forceinline__ int og_frame_edge(const OgFrame &f, int n)
{
    const int t = threadIdx.x;
    int e = -1;
    if (t < f.head) e = t;
    if (t >= 64 && t - 64 < n - f.tail) e = f.tail + t - 64;
    return e;
}

// Entry-point check of a table launch; count: the workgroups (chunks) of the launch.
static inline int og_check_table(const char *name, const void *rows, const void *prefix, int n_rows, int count)
{
    OG_REQUIRE(rows && prefix, OG_EINVAL, "%s: null table", name);
    OG_REQUIRE(((uintptr_t)rows & 7u) == 0 && ((uintptr_t)prefix & 3u) == 0, OG_EINVAL, "%s: misaligned table", name);
    OG_REQUIRE(n_rows > 0 && count >= 0, OG_EINVAL, "%s: bad table size (%d rows, %d workgroups)", name, n_rows, count);
    return OG_OK;
}
