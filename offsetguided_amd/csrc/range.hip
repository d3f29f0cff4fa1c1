// Range report (include/og_decoder.h, "range report"): how many elements of a tensor are NaN, inf, zero, overflow / flush / go
// subnormal when rounded to the engine's 16-bit type, and the largest and smallest finite magnitudes -- nine int64 words per stats
// row, accumulated.  A pure read stream: a workgroup of 256 threads owns chunks of RANGE_CHUNK elements, reads each as 16-byte loads
// between a scalar head and tail (any element-aligned address), classifies every element on its BIT PATTERN with integer compares
// (the fp32 denormal mode of the device cannot change a count), reduces per wave (shuffles) and per workgroup (LDS), and sends one
// set of ordinary vector atomics to the row: a 64-bit add for words 0..6, a 64-bit max for words 7 and 8, identity contributions
// skipped.  All nine words are order-independent: exact and run-to-run identical, no finishing pass, no workspace.  Two entry points
// over one device body: a table of tensors in device memory (og_range_stats: every weight of a model in one launch) and one tensor
// given as kernel arguments (og_range_probe: an activation inside a graph capture).  tests/range_common.py restates the nine words
// in numpy; the GPU test asks for equality.
#include "table.h"

namespace {

constexpr int RANGE_THREADS = 256;
constexpr int RANGE_CHUNK = 8192;            // elements of one chunk: 16 KB of a 16-bit source, 32 KB of fp32
constexpr int RANGE_PROBE_MAX_WG = 1024;     // og_range_probe: at most this many workgroups, each strides over the chunks
constexpr int RANGE_ROW_WORDS = 4;
constexpr int SRC_F32 = 0, SRC_F16 = 1, SRC_BF16 = 2;

constexpr uint32_t F32_INF = 0x7f800000u;
constexpr uint32_t F16_OVER = 0x477ff000u;       // 65520: the smallest magnitude that rounds to fp16's inf
constexpr uint32_t F16_FLUSH = 0x33000000u;      // 2^-25: the largest magnitude that rounds to fp16's zero (the tie goes to even)
constexpr uint32_t F16_NORMAL = 0x387fe000u;     // 1023.5 * 2^-24: the smallest magnitude that rounds to a normal fp16 (the tie, to 2^-14)

struct Acc {
    uint32_t nan, inf, over, zero, flush, sub, mx, mn;
};

__device__ __forceinline__ void seen_finite(uint32_t m, bool fin, Acc &a)
{
    const uint32_t big = fin ? m : 0u, small = (fin && m != 0u) ? F32_INF - m : 0u;
    a.mx = a.mx > big ? a.mx : big;
    a.mn = a.mn > small ? a.mn : small;
}

// one fp32 element, target fp16 (F16) or bf16 (to_lp of csrc/fold.hip: u += 0x7fff + ((u >> 16) & 1); u >>= 16)
template <bool F16>
__device__ __forceinline__ void classify32(uint32_t u, Acc &a)
{
    const uint32_t m = u & 0x7fffffffu;
    const bool fin = m < F32_INF;
    a.nan += m > F32_INF;
    a.inf += m == F32_INF;
    a.zero += m == 0u;
    if (F16) {
        a.over += fin && m >= F16_OVER;
        a.flush += m != 0u && m <= F16_FLUSH;
        a.sub += m > F16_FLUSH && m < F16_NORMAL;
    } else {
        const uint32_t y = (m + 0x7fffu + ((m >> 16) & 1u)) >> 16;
        a.over += fin && y >= 0x7f80u;
        a.flush += m != 0u && y == 0u;
        a.sub += y >= 1u && y < 0x80u;
    }
    seen_finite(m, fin, a);
}

// one 16-bit element of the target type itself: nothing rounds (over = flush = 0); the magnitude is widened exactly to fp32 bits
template <bool F16>
__device__ __forceinline__ void classify16(uint32_t h, Acc &a)
{
    const uint32_t m = h & 0x7fffu;
    const uint32_t inf = F16 ? 0x7c00u : 0x7f80u, normal = F16 ? 0x0400u : 0x0080u;
    const bool fin = m < inf;
    a.nan += m > inf;
    a.inf += m == inf;
    a.zero += m == 0u;
    a.sub += m != 0u && m < normal;
    uint32_t wide;
    if (F16) {
        if (m >= normal) {
            wide = (((m >> 10) + 112u) << 23) | ((m & 0x3ffu) << 13);
        } else {                    // m * 2^-24, m in 1 .. 1023: leading bit p -> exponent p - 24 (m == 0: wide is not used)
            const int p = 31 - __builtin_clz(m | 1u);
            wide = ((uint32_t)(p + 103) << 23) | ((m << (23 - p)) & 0x7fffffu);
        }
        if (m == 0u) wide = 0u;
    } else {
        wide = m << 16;
    }
    seen_finite(wide, fin, a);
}

template <bool F16, int S>
__device__ __forceinline__ void classify_word(uint32_t w, Acc &a)
{
    if (S == SRC_F32) {
        classify32<F16>(w, a);
    } else {
        classify16<F16>(w & 0xffffu, a);
        classify16<F16>(w >> 16, a);
    }
}

// The chunks first, first + stride, ... of one tensor of source type S into `a`; -> the elements seen (the same on every thread)
template <bool F16, int S>
__device__ __forceinline__ long scan_chunks(const gu8 *base, long numel, long first, long stride, Acc &a)
{
    constexpr int SHIFT = S == SRC_F32 ? 2 : 1;
    const long n_chunks = (numel + RANGE_CHUNK - 1) / RANGE_CHUNK;
    long seen = 0;
    for (long c = first; c < n_chunks; c += stride) {
        const long lo = c * RANGE_CHUNK;
        const int n = numel - lo < RANGE_CHUNK ? (int)(numel - lo) : RANGE_CHUNK;
        seen += n;
        const gu8 *p = base + (lo << SHIFT);
        const OgFrame f = og_frame(p, n, 1 << SHIFT);
        const gu4 *v = (const gu4 *)(p + ((long)f.head << SHIFT));     // 16-byte aligned; every vector lies inside [lo, lo + n)
#pragma unroll 4
        for (int k = threadIdx.x; k < f.n_vec; k += RANGE_THREADS) {
            const u4 q = v[k];
            classify_word<F16, S>(q.x, a);
            classify_word<F16, S>(q.y, a);
            classify_word<F16, S>(q.z, a);
            classify_word<F16, S>(q.w, a);
        }
        const int e = og_frame_edge(f, n);
        if (e >= 0) {
            if (S == SRC_F32) classify32<F16>(((const gu32 *)p)[e], a);
            else classify16<F16>(((const gu16 *)p)[e], a);
        }
    }
    return seen;
}

template <bool F16>
__device__ __forceinline__ void range_body(const gu8 *base, long numel, int stype, long first, long stride, unsigned long long *row)
{
    __shared__ uint32_t part[RANGE_THREADS / 64][8];
    Acc a = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
    long seen = 0;
    if (stype == SRC_F32) seen = scan_chunks<F16, SRC_F32>(base, numel, first, stride, a);
    else if (stype == (F16 ? SRC_F16 : SRC_BF16)) seen = scan_chunks<F16, SRC_F16>(base, numel, first, stride, a);     // the 16-bit source is the target type
    if (seen == 0) return;          // no chunk of this workgroup's, or a source type the launch does not serve: nothing is touched (uniform)

    uint32_t v[8] = {a.nan, a.inf, a.over, a.zero, a.flush, a.sub, a.mx, a.mn};
#pragma unroll
    for (int j = 0; j < 8; ++j) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const uint32_t o = (uint32_t)__shfl_down((int)v[j], off, 64);
            v[j] = j < 6 ? v[j] + o : (v[j] > o ? v[j] : o);
        }
    }
    const int t = threadIdx.x;
    if ((t & 63) == 0) {
#pragma unroll
        for (int j = 0; j < 8; ++j) part[t >> 6][j] = v[j];
    }
    __syncthreads();
    if (t < 9) {
        unsigned long long w = (unsigned long long)seen;
        if (t > 0) {
            w = 0;
            for (int k = 0; k < RANGE_THREADS / 64; ++k) {
                const unsigned long long o = part[k][t - 1];
                w = t <= 6 ? w + o : (w > o ? w : o);
            }
        }
        if (w != 0) {               // zero is the identity of the add and of the max
            if (t <= 6) atomicAdd(row + t, w);
            else atomicMax(row + t, w);
        }
    }
}

template <bool F16>
__global__ __launch_bounds__(RANGE_THREADS) void range_table_kernel(const int64_t *__restrict__ rows, const int32_t *__restrict__ prefix,
                                                                    int n_rows, unsigned long long *stats)
{
    const int r = og_find_row(prefix, n_rows, blockIdx.x);
    const int64_t *e = rows + (size_t)r * RANGE_ROW_WORDS;
    const long numel = e[1], out = e[3];
    const int first = (int)blockIdx.x - prefix[r], share = prefix[r + 1] - prefix[r];
    if (numel <= 0 || out < 0 || first < 0 || first >= share) return;         // a table that does not match its prefix
    range_body<F16>((const gu8 *)(uintptr_t)e[0], numel, (int)e[2], first, share, stats + out * OG_RANGE_WORDS);
}

template <bool F16>
__global__ __launch_bounds__(RANGE_THREADS) void range_probe_kernel(const void *x, long numel, int stype, unsigned long long *row)
{
    range_body<F16>((const gu8 *)(uintptr_t)x, numel, stype, blockIdx.x, gridDim.x, row);
}

}  // namespace

OG_API int og_range_chunk_elems(void) { return RANGE_CHUNK; }

OG_API int og_range_stats(const int64_t *rows, const int32_t *wg_prefix, int n_rows, int n_workgroups, int target, int64_t *stats,
                          void *stream)
{
    const char *name = "og_range_stats";
    if (int rc = og_check_table(name, rows, wg_prefix, n_rows, n_workgroups)) return rc;
    OG_REQUIRE(stats && ((uintptr_t)stats & 7u) == 0, OG_EINVAL, "%s: null or misaligned stats", name);
    OG_REQUIRE(target == OG_RANGE_F16 || target == OG_RANGE_BF16, OG_EINVAL, "%s: target type %d is neither fp16 nor bf16", name, target);
    if (n_workgroups == 0) return OG_OK;
    unsigned long long *out = (unsigned long long *)stats;
    if (target == OG_RANGE_F16)
        hipLaunchKernelGGL(range_table_kernel<true>, dim3(n_workgroups), dim3(RANGE_THREADS), 0, (hipStream_t)stream, rows, wg_prefix, n_rows, out);
    else
        hipLaunchKernelGGL(range_table_kernel<false>, dim3(n_workgroups), dim3(RANGE_THREADS), 0, (hipStream_t)stream, rows, wg_prefix, n_rows, out);
    OG_LAUNCH_CHECK(name);
    return OG_OK;
}

OG_API int og_range_probe(const void *x, int64_t numel, int source, int target, int64_t *stats_row, void *stream)
{
    const char *name = "og_range_probe";
    OG_REQUIRE(target == OG_RANGE_F16 || target == OG_RANGE_BF16, OG_EINVAL, "%s: target type %d is neither fp16 nor bf16", name, target);
    OG_REQUIRE(source == OG_RANGE_F32 || source == target, OG_EINVAL,
               "%s: source type %d is neither fp32 nor the target type %d", name, source, target);
    OG_REQUIRE(numel >= 0, OG_EINVAL, "%s: negative element count", name);
    OG_REQUIRE(stats_row && ((uintptr_t)stats_row & 7u) == 0, OG_EINVAL, "%s: null or misaligned stats row", name);
    if (numel == 0) return OG_OK;
    OG_REQUIRE(x && ((uintptr_t)x & (source == OG_RANGE_F32 ? 3u : 1u)) == 0, OG_EINVAL, "%s: null or misaligned tensor", name);
    const int64_t chunks = (numel + RANGE_CHUNK - 1) / RANGE_CHUNK;
    const int grid = (int)(chunks < RANGE_PROBE_MAX_WG ? chunks : RANGE_PROBE_MAX_WG);
    unsigned long long *out = (unsigned long long *)stats_row;
    if (target == OG_RANGE_F16)
        hipLaunchKernelGGL(range_probe_kernel<true>, dim3(grid), dim3(RANGE_THREADS), 0, (hipStream_t)stream, x, (long)numel, source, out);
    else
        hipLaunchKernelGGL(range_probe_kernel<false>, dim3(grid), dim3(RANGE_THREADS), 0, (hipStream_t)stream, x, (long)numel, source, out);
    OG_LAUNCH_CHECK(name);
    return OG_OK;
}
