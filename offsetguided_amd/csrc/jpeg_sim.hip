// JpegCompression (transforms/image.py:31-41: PIL save as JPEG, load again) on the device: a lossy round trip of the warped uint8 crop
// with the SHAPE of baseline JPEG at 4:2:0 -- colour transform, chroma subsampling, 8 x 8 DCT, quality-scaled Annex K quantisation and
// back -- in integer arithmetic OF THIS LIBRARY'S OWN, held bit for bit to the numpy restatement tests/photometric_common.py.  No bit
// parity with libjpeg is claimed (its DCTs, its chroma filters and its rounding differ); how close the result is to PIL's round trip is
// measured by tests/test_photometric_cpu.py (profiles/photometric_parity.json).  No entropy coding happens: it is lossless.
//
// og_jpeg_roundtrip_batch_u8 reads the (N,S,S,3) bytes og_warp_affine_photo_batch_u8 left in out_u8 and, for the SELECTED images only,
// overwrites their fp32 NCHW planes with normalise(epilogue(jpeg(v))), epilogue = csrc/photometric.h.
//
// One MCU = 16 x 16 pixels at (16 my, 16 mx); pixel (y, x) of it is v[min(16 my + y, S - 1)][min(16 mx + x, S - 1)]: a partial MCU is
// padded by replicating the last row and column, as an encoder does.  Every value an int32, every shift arithmetic:
//   1. Y  = ( 19595 R + 38470 G +  7471 B + 2^15) >> 16
//      Cb = (-11059 R - 21709 G + 32768 B + 128 * 2^16 + 2^15 - 1) >> 16
//      Cr = ( 32768 R - 27439 G -  5329 B + 128 * 2^16 + 2^15 - 1) >> 16                        (16-bit fixed point, all in [0, 255])
//   2. chroma: the mean of each 2 x 2 square, (a + b + c + d + 2) >> 2.  Four Y blocks, one Cb and one Cr block of 8 x 8 per MCU.
//   3. level shift: p = value - 128.
//   4. forward DCT, T[u][x] = rint(a(u) cos((2x + 1) u pi / 16) * 2^13), a(0) = sqrt(1/8), a(u) = 1/2 (the table below):
//        t[y][u] = (sum_x T[u][x] p[y][x] + 2^9)  >> 10        F[v][u] = (sum_y T[v][y] t[y][u] + 2^15) >> 16
//   5. quantise and dequantise with Q[v][u]: F' = sign(F) * ((|F| + (Q >> 1)) / Q) * Q             (round half away from zero)
//      Q = clamp((base * scale + 50) / 100, 1, 255), scale = 5000 / quality if quality < 50 else 200 - 2 quality (integer divisions),
//      base = the luminance / chrominance tables of Annex K (below, row-major): libjpeg's scaling, equal to the tables PIL writes.
//   6. inverse DCT: t[y][u] = (sum_v T[v][y] F'[v][u] + 2^9) >> 10        p[y][x] = (sum_u T[u][x] t[y][u] + 2^15) >> 16
//      value = clamp(p + 128, 0, 255).
//   7. chroma back by BOX upsampling: pixel (y, x) takes chroma (y >> 1, x >> 1) of its own MCU; no MCU needs a neighbour.
//   8. R = Y + ((91881 cr + 2^15) >> 16),  G = Y + ((-22554 cb - 46802 cr + 2^15) >> 16),  B = Y + ((116130 cb + 2^15) >> 16)
//      with cb = Cb - 128, cr = Cr - 128; each clamped to [0, 255].
//   No overflow: a row of |T| sums to at most 23168 (rows 0 and 4), a column to 21641.  Step 4: |sum| <= 128 * 23168 = 2 965 504, so
//   |t| <= 2896; then |sum| <= 2896 * 23168 = 67 094 528, so |F| <= 1024.  Step 5: |F'| <= |F| + Q / 2 <= 1151.  Step 6: |sum| <=
//   1151 * 23168 = 26 666 368, so |t| <= 26041; then |sum| + 2^15 <= 26041 * 23168 + 32768 = 603 350 656 < 2^31.  Steps 1 and 8:
//   32768 * 255 + 128 * 2^16 + 2^15 < 2^24;  116130 * 128 + 2^15 < 2^24.
//
// Shape: one workgroup of 256 threads per MCU of one selected image (blockIdx.y), thread (ty, tx) owns pixel (ty, tx).  The six blocks
// of coefficients live in LDS (1536 bytes) and are transformed in place: a pass computes its up to two outputs per thread into
// registers, then the workgroup synchronises, stores, synchronises.  The 2 x 2 chroma sums come from two lane exchanges (a wave holds
// four rows of the MCU).  T, both Q tables and the tint's division tables sit in LDS as well.  Every global read uses clamped
// coordinates, so it lies inside the crop; every store is predicated on the crop bounds.
#include "og_common.h"
#include "photometric.h"

namespace {

constexpr int kJpegBatchMax = 32;

constexpr short kDct[64] = {2896, 2896,  2896,  2896,  2896,  2896,  2896,  2896,  4017, 3406,  2276,  799,   -799,  -2276, -3406, -4017,
                            3784, 1567,  -1567, -3784, -3784, -1567, 1567,  3784,  3406, -799,  -4017, -2276, 2276,  4017,  799,   -3406,
                            2896, -2896, -2896, 2896,  2896,  -2896, -2896, 2896,  2276, -4017, 799,   3406,  -3406, -799,  4017,  -2276,
                            1567, -3784, 3784,  -1567, -1567, 3784,  -3784, 1567,  799,  -2276, 3406,  -4017, 4017,  -3406, 2276,  -799};
constexpr int kQuantLuma[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,  69,  56,
                                14, 17, 22, 29, 51,  87,  80,  62,  18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,
                                49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
constexpr int kQuantChroma[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
                                  47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                                  99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};

// by value in the kernel arguments: the transform table, the two quality-scaled tables, the selected images and their descriptors
struct JpegArgs {
    short dct[64];
    unsigned char quant[2][64];
    int image[kJpegBatchMax];
    photo::Desc d[kJpegBatchMax];
    float mean[3], stdv[3];
};

// One in-place pass over the six blocks.  ROW: out[r][c] = sum_k T(c, k) in[r][k], else out[r][c] = sum_k T(r, k) in[k][c]; T(i, k) =
// dct[i][k] forward, dct[k][i] inverse.  QUANT: step 5 on the result.  The caller's blocks are complete on entry and on exit.
template <bool ROW, bool INVERSE, int SHIFT, bool QUANT>
__device__ __forceinline__ void dct_pass(int (*blk)[64], const short *dct, const unsigned char (*quant)[64])
{
    int res[2];
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        const int e = threadIdx.x + it * 256;                  // 384 outputs
        res[it] = 0;
        if (e < 384) {
            const int bl = e >> 6, r = (e >> 3) & 7, c = e & 7, i = ROW ? c : r;
            int acc = 0;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int t = INVERSE ? dct[k * 8 + i] : dct[i * 8 + k];
                acc += t * (ROW ? blk[bl][r * 8 + k] : blk[bl][k * 8 + c]);
            }
            acc = (acc + (1 << (SHIFT - 1))) >> SHIFT;
            if (QUANT) {
                const int q = quant[bl >= 4][e & 63], mag = ((acc < 0 ? -acc : acc) + (q >> 1)) / q * q;
                acc = acc < 0 ? -mag : mag;
            }
            res[it] = acc;
        }
    }
    __syncthreads();
    blk[threadIdx.x >> 6][threadIdx.x & 63] = res[0];
    if (threadIdx.x < 128) blk[4 + (threadIdx.x >> 6)][threadIdx.x & 63] = res[1];
    __syncthreads();
}

__global__ void __launch_bounds__(256)
jpeg_roundtrip_kernel(const unsigned char *__restrict__ u8, JpegArgs a, int S, int mcus_x, float *__restrict__ out)
{
    __shared__ int blk[6][64];
    __shared__ short dct[64];
    __shared__ unsigned char quant[2][64];
    __shared__ int divs[2][256];
    const int tid = threadIdx.x;
    photo::build_tables(divs[0], divs[1], tid);
    if (tid < 64) dct[tid] = a.dct[tid];
    if (tid < 128) quant[tid >> 6][tid & 63] = a.quant[tid >> 6][tid & 63];
    const int n = a.image[blockIdx.y];
    const int mx = blockIdx.x % mcus_x, my = blockIdx.x / mcus_x;
    const int tx = tid & 15, ty = tid >> 4;
    const int X = mx * 16 + tx, Y = my * 16 + ty;
    const unsigned char *px = u8 + (((size_t)n * S + min(Y, S - 1)) * S + min(X, S - 1)) * 3;   // clamped: always inside the crop
    const int R = px[0], G = px[1], B = px[2];
    // steps 1-3
    const int lum = (19595 * R + 38470 * G + 7471 * B + (1 << 15)) >> 16;
    int cb = (-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16;
    int cr = (32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16;
    cb += __shfl_xor(cb, 1);                                   // lanes (ty & 3) * 16 + tx: the x neighbour, then the y neighbour
    cr += __shfl_xor(cr, 1);
    cb += __shfl_xor(cb, 16);
    cr += __shfl_xor(cr, 16);
    blk[(ty >> 3) * 2 + (tx >> 3)][(ty & 7) * 8 + (tx & 7)] = lum - 128;
    if (!(tx & 1) && !(ty & 1)) {
        blk[4][(ty >> 1) * 8 + (tx >> 1)] = ((cb + 2) >> 2) - 128;
        blk[5][(ty >> 1) * 8 + (tx >> 1)] = ((cr + 2) >> 2) - 128;
    }
    __syncthreads();
    dct_pass<true, false, 10, false>(blk, dct, quant);         // steps 4, 5
    dct_pass<false, false, 16, true>(blk, dct, quant);
    dct_pass<false, true, 10, false>(blk, dct, quant);         // step 6
    dct_pass<true, true, 16, false>(blk, dct, quant);
    if (X >= S || Y >= S) return;                              // (after the last barrier)
    // steps 6-8
    const int y2 = photo::clampi(blk[(ty >> 3) * 2 + (tx >> 3)][(ty & 7) * 8 + (tx & 7)] + 128, 0, 255);
    const int cb2 = photo::clampi(blk[4][(ty >> 1) * 8 + (tx >> 1)] + 128, 0, 255) - 128;
    const int cr2 = photo::clampi(blk[5][(ty >> 1) * 8 + (tx >> 1)] + 128, 0, 255) - 128;
    int rgb[3] = {photo::clampi(y2 + ((91881 * cr2 + (1 << 15)) >> 16), 0, 255),
                  photo::clampi(y2 + ((-22554 * cb2 - 46802 * cr2 + (1 << 15)) >> 16), 0, 255),
                  photo::clampi(y2 + ((116130 * cb2 + (1 << 15)) >> 16), 0, 255)};
    photo::apply(rgb[0], rgb[1], rgb[2], a.d[blockIdx.y], divs[0], divs[1]);
#pragma unroll
    for (int c = 0; c < 3; ++c)
        out[(((size_t)n * 3 + c) * S + Y) * S + X] = ((float)rgb[c] / 255.f - a.mean[c]) / a.stdv[c];   // ToTensor, Normalize
}

}  // namespace

OG_API int og_jpeg_roundtrip_batch_u8(const unsigned char *u8, int N, int S, const int *selected, int n_selected, int quality,
                                      const int *photo4, const float *mean3, const float *std3, float *out, void *stream)
{
    const char *name = "og_jpeg_roundtrip_batch_u8";
    OG_REQUIRE(u8 && mean3 && std3 && out && (selected || n_selected == 0), OG_EINVAL, "%s: null pointer", name);
    OG_REQUIRE(N > 0 && S > 0 && S <= 16384 && n_selected >= 0, OG_EINVAL, "%s: bad shape", name);
    OG_REQUIRE(quality >= 1 && quality <= 100, OG_EINVAL, "%s: quality outside [1, 100]", name);
    for (int i = 0; i < n_selected; ++i) {
        OG_REQUIRE(selected[i] >= 0 && selected[i] < N, OG_EINVAL, "%s: selected[%d] outside [0, N)", name, i);
        OG_REQUIRE(!photo4 || photo::desc_ok(photo4 + selected[i] * 4), OG_EINVAL, "%s: image %d: bad photometric descriptor", name,
                   selected[i]);
    }
    JpegArgs a = {};
    const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    for (int k = 0; k < 64; ++k) {
        a.dct[k] = kDct[k];
        const int ql = (kQuantLuma[k] * scale + 50) / 100, qc = (kQuantChroma[k] * scale + 50) / 100;
        a.quant[0][k] = (unsigned char)(ql < 1 ? 1 : ql > 255 ? 255 : ql);
        a.quant[1][k] = (unsigned char)(qc < 1 ? 1 : qc > 255 ? 255 : qc);
    }
    for (int c = 0; c < 3; ++c) { a.mean[c] = mean3[c]; a.stdv[c] = std3[c]; }
    const int mcus = (S + 15) / 16;
    for (int first = 0; first < n_selected; first += kJpegBatchMax) {
        const int m = n_selected - first < kJpegBatchMax ? n_selected - first : kJpegBatchMax;
        for (int i = 0; i < kJpegBatchMax; ++i) {
            const int j = selected[first + (i < m ? i : 0)];
            a.image[i] = j;
            a.d[i] = photo4 ? photo::Desc{photo4[j * 4], photo4[j * 4 + 1], photo4[j * 4 + 2], photo4[j * 4 + 3]} : photo::Desc{0, 0, 0, 0};
        }
        hipLaunchKernelGGL(jpeg_roundtrip_kernel, dim3((unsigned)(mcus * mcus), (unsigned)m), dim3(256), 0, (hipStream_t)stream, u8, a, S,
                           mcus, out);
        OG_LAUNCH_CHECK(name);
    }
    return OG_OK;
}
