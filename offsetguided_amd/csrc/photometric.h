// Photometric augmentation on one warped pixel: ColorTint (transforms/image.py:68-86) and Gray (:55-65) of the reference as ONE
// __device__ function between the warp (or the JPEG round trip) and the normalisation: uint8 RGB in, uint8 RGB out, tint then gray.
//
// Both steps are a SPECIFICATION OF THIS LIBRARY'S OWN in integer arithmetic, held bit for bit to the numpy restatement
// tests/photometric_common.py.  The tint has the shape of OpenCV's 8-bit RGB <-> HSV conversion, not a claim about its bits: cv2 is
// absent from the build, parity with cv2.cvtColor(COLOR_RGB2HSV / COLOR_HSV2RGB) is UNPINNED.  Gray is PIL's `L` conversion (what
// RandomGrayscale(p=1) yields on three channels) and IS pinned to PIL (tests/test_photometric_cpu.py).
//
// Per image a descriptor {mode, dh, ds, dv}: mode bit 0 = tint, bit 1 = gray; dh, ds, dv the tint's deltas.
//
// Tint of (r, g, b), every value an int32:
//   1. V = max(r, g, b), diff = V - min(r, g, b).
//      S = (diff * sdiv[V] + 2^11) >> 12,  sdiv[0] = 0, sdiv[i] = rint((255 << 12) / i) = (2 * (255 << 12) + i) / (2 i) in integers
//      (no ties: 255 * 2^13 = (2k + 1) i has no solution with i < 2^13).
//      x = g - b if V == r, else b - r + 2 diff if V == g, else r - g + 4 diff      (the tests in this order)
//      H = (x * hdiv[diff] + 2^11) >> 12 (arithmetic shift), hdiv[0] = 0, hdiv[i] = rint((180 << 12) / (6 i))
//        = (2 * (180 << 12) + 6 i) / (12 i) in integers (no ties below i = 2^14);  H += 180 if H < 0.   H lies in [0, 180).
//   2. H = clamp(H + dh, 0, 179) -- clamped, NOT wrapped, as the reference does --, S = clamp(S + ds, 0, 255), V = clamp(V + dv, 0, 255).
//   3. sector = H / 30 (0..5), f = H - 30 sector;  rounding integer divisions of non-negative numerators:
//        p = (V (255 - S) + 127) / 255,  q = (V (7650 - S f) + 3825) / 7650,  t = (V (7650 - S (30 - f)) + 3825) / 7650
//      (r, g, b) = (V,t,p), (q,V,p), (p,V,t), (p,q,V), (t,p,V), (V,p,q) for sector 0..5.  No float operation anywhere.
//   No overflow: |x| <= 5 * 255 and hdiv <= 122880, so |x * hdiv| + 2^11 <= 156 674 048; diff * sdiv <= 255 * 1 044 480 = 266 342 400;
//   V * 7650 + 3825 <= 1 954 575: all below 2^31.
//   How far the zero tint moves a colour (asserted on a lattice by the CPU test): the largest channel comes back exactly (V).  S is
//   off by at most 1/2 + 255 / 2^13 = 0.531 of its 1/255 step, so the smallest channel p = V - V S / 255 is off by at most 0.531 + 1/2:
//   1 as an integer.  H (2-degree steps) is off by at most 1/2 + 5 * 255 / 2^13 = 0.656 steps, which moves the middle channel by
//   diff * 0.656 / 30 <= 5.58; with S's 0.531 and the final rounding 1/2 that is 6.61: |tint(0,0,0)(rgb) - rgb| <= 6 per channel.
//
// Gray: y = (19595 r + 38470 g + 7471 b + 2^15) >> 16 (the coefficients sum to 2^16: y <= 255, the sum < 2^24), (r, g, b) = (y, y, y).
#pragma once
#include "og_common.h"

namespace photo {

constexpr int kTint = 1, kGray = 2;

struct Desc {
    int mode, dh, ds, dv;
};

// the two division tables, 256 entries each, built by a 256-thread workgroup into LDS (the caller synchronises)
__device__ __forceinline__ void build_tables(int *sdiv, int *hdiv, int i)
{
    sdiv[i] = i ? (2 * (255 << 12) + i) / (2 * i) : 0;
    hdiv[i] = i ? (2 * (180 << 12) + 6 * i) / (12 * i) : 0;
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

__device__ __forceinline__ void tint(int &r, int &g, int &b, const Desc &d, const int *sdiv, const int *hdiv)
{
    int V = max(max(r, g), b);
    const int diff = V - min(min(r, g), b);
    int S = (diff * sdiv[V] + (1 << 11)) >> 12;
    const int x = V == r ? g - b : V == g ? b - r + 2 * diff : r - g + 4 * diff;
    int H = (x * hdiv[diff] + (1 << 11)) >> 12;
    H += H < 0 ? 180 : 0;
    H = clampi(H + d.dh, 0, 179);
    S = clampi(S + d.ds, 0, 255);
    V = clampi(V + d.dv, 0, 255);
    const int sector = H / 30, f = H - 30 * sector;
    const int p = (V * (255 - S) + 127) / 255;
    const int q = (V * (7650 - S * f) + 3825) / 7650;
    const int t = (V * (7650 - S * (30 - f)) + 3825) / 7650;
    r = sector == 0 || sector == 5 ? V : sector == 1 ? q : sector == 4 ? t : p;
    g = sector == 1 || sector == 2 ? V : sector == 0 ? t : sector == 3 ? q : p;
    b = sector == 3 || sector == 4 ? V : sector == 2 ? t : sector == 5 ? q : p;
}

// the epilogue: tint, then gray
__device__ __forceinline__ void apply(int &r, int &g, int &b, const Desc &d, const int *sdiv, const int *hdiv)
{
    if (d.mode & kTint) tint(r, g, b, d, sdiv, hdiv);
    if (d.mode & kGray) r = g = b = (19595 * r + 38470 * g + 7471 * b + (1 << 15)) >> 16;
}

// host: a descriptor the kernels can take (the deltas cannot leave the ranges the overflow bound assumes)
inline bool desc_ok(const int *p4) { return (p4[0] & ~3) == 0 && abs(p4[1]) <= 180 && abs(p4[2]) <= 255 && abs(p4[3]) <= 255; }

}  // namespace photo
