// BatchNorm fold + 16-bit cast of every layer of a model in ONE launch (include/og_decoder.h, "weight refresh"): what
// models/engine.py:_fold + .to(dtype) + .contiguous(channels_last) compute with torch ops when an engine is built, written into
// the buffers an engine already has.  A memory-bound streaming kernel over a table of layers: a workgroup of 256 threads owns a slab
// of output channels of one layer; per output channel it reads the cin * kh * kw fp32 weights as one contiguous run (16-byte loads
// where the address allows, scalar head and tail), multiplies by the channel's scale, and writes the run of 16-bit values in
// (kh, kw, cin) order.  An OIHW source is permuted through LDS: the contiguous loads are scattered into a [tap][channel] image (row
// pitch + 8 floats: the taps of one channel fall on different banks), the image is read back in rows and leaves in 16-byte stores.
// A channels-last source (or a 1x1 layer) has one tap and nothing to permute: where its runs are whole 16-byte groups the slab is
// streamed straight through registers, no LDS image and one barrier (the channels' scales); otherwise it is the same code with one
// tap.  The arithmetic is the header's list of individually rounded fp32 operations (-ffp-contract=off, correctly rounded divide and
// sqrt): tests/engine_refresh_common.py restates it in numpy and the GPU test compares bit for bit.
#include "table.h"

namespace {

constexpr int FOLD_THREADS = 256;
constexpr int FOLD_LDS_FLOATS = 8192;        // 32 KB: the [tap][channel] image of one pass
constexpr int FOLD_PAD = 8;                  // floats added to the image's row pitch
constexpr int FOLD_ROW_WORDS = 16;

struct Layer {
    const gfloat *w, *bias, *gamma, *beta, *mean, *var;
    gu16 *dw;
    gfloat *db32;
    gu16 *db;
    int cout, cin, taps, src_cl;
    float eps;
    int partner, slab;
};

__device__ __forceinline__ Layer load_layer(const int64_t *rows, int r)
{
    const int64_t *e = rows + (size_t)r * FOLD_ROW_WORDS;
    Layer l;
    l.w = (const gfloat *)(uintptr_t)e[0];
    l.bias = (const gfloat *)(uintptr_t)e[1];
    l.gamma = (const gfloat *)(uintptr_t)e[2];
    l.beta = (const gfloat *)(uintptr_t)e[3];
    l.mean = (const gfloat *)(uintptr_t)e[4];
    l.var = (const gfloat *)(uintptr_t)e[5];
    l.dw = (gu16 *)(uintptr_t)e[6];
    l.db32 = (gfloat *)(uintptr_t)e[7];
    l.db = (gu16 *)(uintptr_t)e[8];
    l.cout = (int)e[9];
    l.cin = (int)e[10];
    l.taps = (int)e[11];
    l.src_cl = (int)(e[12] & 1);
    l.eps = __builtin_bit_cast(float, (uint32_t)e[13]);
    l.partner = (int)e[14];
    l.slab = (int)e[15];
    return l;
}

// fp32 -> the 16-bit type, round to nearest even.  fp16: the hardware conversion (overflow -> inf, subnormals kept); bf16: on the
// bit pattern, a NaN becomes the quiet NaN 0x7fc0 (torch's c10::BFloat16).
template <bool F16>
__device__ __forceinline__ unsigned short to_lp(float f)
{
    if (F16) return __builtin_bit_cast(unsigned short, (_Float16)f);
    if (f != f) return (unsigned short)0x7fc0;
    uint32_t u = __builtin_bit_cast(uint32_t, f);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (unsigned short)(u >> 16);
}

__device__ __forceinline__ float bn_scale(const Layer &l, int o)
{
    const float s = l.var[o] + l.eps;
    const float r = sqrtf(s);
    return l.gamma[o] / r;
}

// b' of the header: (bias - mean) * scale + beta, or the bias itself (0 without one) for a layer without BatchNorm
__device__ __forceinline__ float folded_bias(const Layer &l, int o)
{
    const float bias = l.bias ? l.bias[o] : 0.f;
    if (!l.gamma) return bias;
    const float d = bias - l.mean[o];
    const float m = d * bn_scale(l, o);
    return m + l.beta[o];
}

// One output channel's weights, channels [i0, i0 + ic) of it: n = ic * TAPS consecutive source floats -> tile[tap * pitch + channel],
// scaled.  T = the tap count as a constant (0: the run-time value `taps`).
template <int T>
__device__ __forceinline__ void load_pass(const gfloat *src, int n, int taps, int pitch, bool has_scale, float scale, float *tile)
{
    const int K = T ? T : taps;
    const OgFrame f = og_frame(src, n, 4);
    auto put = [&](int s, float v) {
        if (has_scale) v = v * scale;
        const int ch = s / K, tap = s - ch * K;
        tile[tap * pitch + ch] = v;
    };
    for (int k = threadIdx.x; k < f.n_vec; k += FOLD_THREADS) {
        const int s = f.head + 4 * k;
        const f4 v = *(const gf4 *)(src + s);
        put(s, v.x);
        put(s + 1, v.y);
        put(s + 2, v.z);
        put(s + 3, v.w);
    }
    const int e = og_frame_edge(f, n);
    if (e >= 0) put(e, src[e]);
}

// tile -> the runs dst[tap * cin + i0 + (0 .. ic)], tap by tap: eight values per 16-byte store where `vec`, else one by one
template <bool F16>
__device__ __forceinline__ void store_pass(const float *tile, int taps, int pitch, int ic, gu16 *dst, int cin, int i0, bool vec)
{
    if (vec) {
        const int per = ic >> 3;
        for (int v = threadIdx.x; v < taps * per; v += FOLD_THREADS) {
            const int tap = v / per, j = (v - tap * per) << 3;
            const f4 a = *reinterpret_cast<const f4 *>(tile + tap * pitch + j);
            const f4 b = *reinterpret_cast<const f4 *>(tile + tap * pitch + j + 4);
            u4 out;
            out.x = (unsigned)to_lp<F16>(a.x) | ((unsigned)to_lp<F16>(a.y) << 16);
            out.y = (unsigned)to_lp<F16>(a.z) | ((unsigned)to_lp<F16>(a.w) << 16);
            out.z = (unsigned)to_lp<F16>(b.x) | ((unsigned)to_lp<F16>(b.y) << 16);
            out.w = (unsigned)to_lp<F16>(b.z) | ((unsigned)to_lp<F16>(b.w) << 16);
            *(gu4 *)(dst + (size_t)tap * cin + i0 + j) = out;
        }
    } else {
        for (int v = threadIdx.x; v < taps * ic; v += FOLD_THREADS) {
            const int tap = v / ic, j = v - tap * ic;
            dst[(size_t)tap * cin + i0 + j] = to_lp<F16>(tile[tap * pitch + j]);
        }
    }
}

template <bool F16>
__global__ __launch_bounds__(FOLD_THREADS) void fold_kernel(const int64_t *__restrict__ rows, const int32_t *__restrict__ prefix, int n_rows)
{
    __shared__ __attribute__((aligned(16))) float tile[FOLD_LDS_FLOATS];
    const int r = og_find_row(prefix, n_rows, blockIdx.x);
    const Layer l = load_layer(rows, r);
    if (l.slab <= 0 || l.cout <= 0 || l.cin <= 0 || l.taps <= 0) return;
    const long first = (long)(blockIdx.x - prefix[r]) * l.slab;
    if (first < 0 || first >= l.cout) return;          // a table that does not match its prefix
    const int o_lo = (int)first, o_hi = l.cout - o_lo > l.slab ? o_lo + l.slab : l.cout;

    // a channels-last source already has the destination's order: one tap of cin * taps channels
    const int taps = (l.src_cl || l.taps == 1) ? 1 : l.taps;
    const int cin = (l.src_cl || l.taps == 1) ? l.cin * l.taps : l.cin;
    int ic_max = FOLD_LDS_FLOATS / taps - FOLD_PAD;     // channels of one pass: taps * (ic_max + FOLD_PAD) floats of LDS
    if (ic_max >= 8) ic_max &= ~7;                      // whole 16-byte groups, so that every pass starts on one
    if (ic_max < 8) return;                             // more taps than the image holds (> 512): not a convolution of this model
    const long per_cout = (long)cin * taps;
    const bool has_scale = l.gamma != nullptr;

    // Nothing to permute (one tap), whole 16-byte groups and an aligned destination: the slab is ONE run of source floats and one
    // run of 16-bit values.  The scales of its channels go to LDS once (one barrier); then every thread streams groups of eight:
    // two 16-byte loads (eight scalar ones where the source is off its boundary), one 16-byte store.
    const int n_o = o_hi - o_lo;
    if (taps == 1 && (per_cout & 7) == 0 && n_o <= FOLD_LDS_FLOATS && (long)n_o * per_cout < (1L << 31) &&
        ((uintptr_t)(l.dw + (size_t)o_lo * per_cout) & 15u) == 0) {
        if (has_scale) {
            for (int i = threadIdx.x; i < n_o; i += FOLD_THREADS) tile[i] = bn_scale(l, o_lo + i);
            __syncthreads();
        }
        const gfloat *src = l.w + (size_t)o_lo * per_cout;
        gu16 *dst = l.dw + (size_t)o_lo * per_cout;
        const bool src_vec = ((uintptr_t)src & 15u) == 0;
        const long groups = (long)n_o * (per_cout >> 3);
        for (long g = threadIdx.x; g < groups; g += FOLD_THREADS) {
            const long e = g << 3;
            f4 a, b;
            if (src_vec) {
                a = *(const gf4 *)(src + e);
                b = *(const gf4 *)(src + e + 4);
            } else {
                a.x = src[e], a.y = src[e + 1], a.z = src[e + 2], a.w = src[e + 3];
                b.x = src[e + 4], b.y = src[e + 5], b.z = src[e + 6], b.w = src[e + 7];
            }
            if (has_scale) {
                const float s = tile[(unsigned)e / (unsigned)per_cout];       // a group never straddles two channels: per_cout % 8 == 0
                a.x = a.x * s, a.y = a.y * s, a.z = a.z * s, a.w = a.w * s;
                b.x = b.x * s, b.y = b.y * s, b.z = b.z * s, b.w = b.w * s;
            }
            u4 out;
            out.x = (unsigned)to_lp<F16>(a.x) | ((unsigned)to_lp<F16>(a.y) << 16);
            out.y = (unsigned)to_lp<F16>(a.z) | ((unsigned)to_lp<F16>(a.w) << 16);
            out.z = (unsigned)to_lp<F16>(b.x) | ((unsigned)to_lp<F16>(b.y) << 16);
            out.w = (unsigned)to_lp<F16>(b.z) | ((unsigned)to_lp<F16>(b.w) << 16);
            *(gu4 *)(dst + e) = out;
        }
    } else {
        for (int o = o_lo; o < o_hi; ++o) {
            const float scale = has_scale ? bn_scale(l, o) : 1.f;
            gu16 *dst = l.dw + (size_t)o * per_cout;
            const bool dst_vec = ((uintptr_t)dst & 15u) == 0 && (cin & 7) == 0;
            for (int i0 = 0; i0 < cin; i0 += ic_max) {
                const int ic = cin - i0 < ic_max ? cin - i0 : ic_max;
                const int pitch = ((ic + 7) & ~7) + FOLD_PAD;
                const gfloat *src = l.w + (size_t)o * per_cout + (size_t)i0 * taps;
                __syncthreads();                            // the previous pass has been read
                switch (taps) {
                case 1: load_pass<1>(src, ic * taps, taps, pitch, has_scale, scale, tile); break;
                case 9: load_pass<9>(src, ic * taps, taps, pitch, has_scale, scale, tile); break;
                case 49: load_pass<49>(src, ic * taps, taps, pitch, has_scale, scale, tile); break;
                default: load_pass<0>(src, ic * taps, taps, pitch, has_scale, scale, tile); break;
                }
                __syncthreads();
                store_pass<F16>(tile, taps, pitch, ic, dst, cin, i0, dst_vec && (ic & 7) == 0);
            }
        }
    }

    // the biases of the slab: b32 = b' (+ b' of the partner row: the layer whose output is added before the activation)
    for (int o = o_lo + threadIdx.x; o < o_hi; o += FOLD_THREADS) {
        float b = folded_bias(l, o);
        if (l.partner >= 0 && l.partner < n_rows) {
            const Layer p = load_layer(rows, l.partner);
            const float b2 = folded_bias(p, o);
            b = b + b2;
        }
        if (l.db32) l.db32[o] = b;
        if (l.db) l.db[o] = to_lp<F16>(b);
    }
}

}  // namespace

OG_API int og_fold_row_words(void) { return FOLD_ROW_WORDS; }

OG_API int og_fold_bn_w16(const int64_t *rows, const int32_t *wg_prefix, int n_rows, int n_workgroups, int f16, void *stream)
{
    const char *name = "og_fold_bn_w16";
    if (int rc = og_check_table(name, rows, wg_prefix, n_rows, n_workgroups)) return rc;
    if (n_workgroups == 0) return OG_OK;
    if (f16)
        hipLaunchKernelGGL(fold_kernel<true>, dim3(n_workgroups), dim3(FOLD_THREADS), 0, (hipStream_t)stream, rows, wg_prefix, n_rows);
    else
        hipLaunchKernelGGL(fold_kernel<false>, dim3(n_workgroups), dim3(FOLD_THREADS), 0, (hipStream_t)stream, rows, wg_prefix, n_rows);
    OG_LAUNCH_CHECK(name);
    return OG_OK;
}
