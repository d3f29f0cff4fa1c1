// COCO keypoint scoring (COCOeval, iouType='keypoints'): the OKS of every (detection, ground truth) pair of every image in one launch,
// the greedy matching of every (image, area range, threshold) in a second one.  See include/og_decoder.h for the operation order.
// All arithmetic is IEEE double; the file is compiled with -ffp-contract=off and without fast-math like the rest of the library.
// Small, latency-shaped work: what it replaces is pycocotools' Python loop over image x area range x threshold x detection x ground truth.
#include "og_common.h"

namespace {

constexpr int kK = 17;             // COCO person keypoints
constexpr int kMaxDet = 64;        // detections per image the ABI accepts (COCOeval keeps 20)
constexpr int kLdsPairs = 1024;    // an image's OKS block is staged in LDS up to this many pairs (8 KB), read from global memory above
constexpr int kMaskGts = 64;       // the per-lane matched set is a 64-bit mask up to this many ground truths, a workspace slice above

struct Sigmas {
    double var[kK];                // (2 sigma)^2
};

struct MatchParams {
    double lo[16], hi[16];         // area ranges
    double thr[16];                // min(t, 1 - 1e-10)
};

// First image i in [0, I) with pair_off[i + 1] > p (images without pairs are stepped over).
__device__ __forceinline__ int image_of_pair(const int64_t *pair_off, int I, int64_t p)
{
    int lo = 0, hi = I - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (pair_off[mid + 1] > p) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

__global__ __launch_bounds__(256) void oks_matrix_kernel(const double *__restrict__ dets, const double *__restrict__ gts,
                                                         const double *__restrict__ gt_area, const double *__restrict__ gt_bbox,
                                                         const int32_t *__restrict__ det_off, const int32_t *__restrict__ gt_off,
                                                         const int64_t *__restrict__ pair_off, Sigmas sig, int I, int D, int G,
                                                         int64_t n_pairs, double *__restrict__ oks)
{
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_pairs) return;
    const int i = image_of_pair(pair_off, I, p);
    const int64_t local = p - pair_off[i];
    const int g_i = gt_off[i + 1] - gt_off[i], d_i = det_off[i + 1] - det_off[i];
    if (local < 0 || g_i <= 0 || local >= (int64_t)d_i * g_i) return;        // tables that disagree with each other: nothing is read
    const int d = det_off[i] + (int)(local / g_i), g = gt_off[i] + (int)(local % g_i);
    if (d < 0 || d >= D || g < 0 || g >= G) return;
    const double *dk = dets + (size_t)d * kK * 3, *gk = gts + (size_t)g * kK * 3;
    int k1 = 0;
    for (int k = 0; k < kK; ++k) k1 += gk[3 * k + 2] > 0.0;
    const double denom = gt_area[g] + 2.220446049250313e-16;                  // np.spacing(1)
    double sum = 0.0;
    if (k1 > 0) {
        for (int k = 0; k < kK; ++k) {
            if (!(gk[3 * k + 2] > 0.0)) continue;
            const double dx = dk[3 * k] - gk[3 * k], dy = dk[3 * k + 1] - gk[3 * k + 1];
            const double e = (dx * dx + dy * dy) / sig.var[k] / denom / 2.0;
            sum += exp(-e);
        }
        oks[p] = sum / (double)k1;
    } else {
        const double bx = gt_bbox[4 * (size_t)g], by = gt_bbox[4 * (size_t)g + 1], bw = gt_bbox[4 * (size_t)g + 2],
                     bh = gt_bbox[4 * (size_t)g + 3];
        const double x0 = bx - bw, x1 = bx + bw * 2.0, y0 = by - bh, y1 = by + bh * 2.0;
        for (int k = 0; k < kK; ++k) {
            const double xd = dk[3 * k], yd = dk[3 * k + 1];
            const double dx = fmax(0.0, x0 - xd) + fmax(0.0, xd - x1), dy = fmax(0.0, y0 - yd) + fmax(0.0, yd - y1);
            const double e = (dx * dx + dy * dy) / sig.var[k] / denom / 2.0;
            sum += exp(-e);
        }
        oks[p] = sum / (double)kK;
    }
}

// The matched set of one lane: MASK = a register bit mask (g_i <= 64), otherwise bytes ws[g * lanes + lane] of the caller's workspace.
template <bool MASK>
struct Matched {
    unsigned long long bits;
    unsigned char *ws;
    int lanes;
    __device__ __forceinline__ bool get(int g) const { return MASK ? (bits >> g) & 1ull : ws[(size_t)g * lanes] != 0; }
    __device__ __forceinline__ void set(int g)
    {
        if (MASK) bits |= 1ull << g;
        else ws[(size_t)g * lanes] = 1;
    }
};

// One lane = one (area range, threshold); every lane walks the same detections and ground truths in the same order, so every
// load below has one address per wave.  `o` is the image's d_i x g_i block (LDS or global memory).
template <bool MASK, typename OksPtr>
__device__ __forceinline__ void match_image(OksPtr o, int d_i, int g_i, const double *__restrict__ area, const unsigned char *__restrict__ ign,
                                            const unsigned char *__restrict__ crowd, const double *__restrict__ det_area, double lo, double hi,
                                            double thr, Matched<MASK> matched, int32_t *__restrict__ dtm, unsigned char *__restrict__ dtig)
{
    for (int d = 0; d < d_i; ++d) {
        double best = thr;
        int m = -1;
        bool m_ig = false;
        // COCOeval visits the ground truths sorted (stably) by their ignore flag: pass 0 the ones that count, pass 1 the ignored ones.
        // Its stop rule -- a match that counts is not given up for an ignored ground truth -- ends the walk at the start of pass 1.
        for (int pass = 0; pass < 2; ++pass) {
            if (pass == 1 && m >= 0) break;
            for (int g = 0; g < g_i; ++g) {
                const double ar = area[g];
                const bool ig = ign[g] != 0 || ar < lo || ar > hi;
                if (ig != (pass == 1)) continue;
                if (matched.get(g) && crowd[g] == 0) continue;
                const double v = o[(size_t)d * g_i + g];
                if (v < best) continue;
                best = v;                      // an equal OKS replaces: the later ground truth wins a tie
                m = g;
                m_ig = ig;
            }
        }
        if (m >= 0) {
            matched.set(m);
            dtm[d] = m + 1;
            dtig[d] = m_ig;
        } else {
            const double da = det_area[d];
            dtm[d] = 0;
            dtig[d] = da < lo || da > hi;
        }
    }
}

__global__ __launch_bounds__(64) void oks_match_kernel(const double *__restrict__ oks, const int32_t *__restrict__ det_off,
                                                       const int32_t *__restrict__ gt_off, const int64_t *__restrict__ pair_off,
                                                       const double *__restrict__ gt_area, const unsigned char *__restrict__ gt_ignore,
                                                       const unsigned char *__restrict__ gt_crowd, const double *__restrict__ det_area,
                                                       MatchParams prm, int A, int T, int D, int G, int64_t n_pairs,
                                                       int32_t *__restrict__ dt_match, unsigned char *__restrict__ dt_ignore,
                                                       unsigned char *__restrict__ gt_ignore_a, unsigned char *__restrict__ workspace)
{
    __shared__ double s_oks[kLdsPairs];
    const int i = blockIdx.x, lane = threadIdx.x, lanes = A * T;
    const int d0 = det_off[i], g0 = gt_off[i];
    int d_i = det_off[i + 1] - d0, g_i = gt_off[i + 1] - g0;
    const int64_t p0 = pair_off[i];
    // (tables that disagree with the totals: the image is treated as empty instead of read out of bounds)
    if (d0 < 0 || g0 < 0 || d_i < 0 || g_i < 0 || d_i > kMaxDet || d0 + d_i > D || g0 + g_i > G || p0 < 0 ||
        p0 + (int64_t)d_i * g_i > n_pairs)
        d_i = g_i = 0;
    const int n_i = d_i * g_i;
    const bool staged = n_i <= kLdsPairs;
    if (staged)
        for (int j = lane; j < n_i; j += 64) s_oks[j] = oks[p0 + j];
    for (int j = lane; j < A * g_i; j += 64) {
        const int a = j / g_i, g = j - a * g_i;
        const double ar = gt_area[g0 + g];
        gt_ignore_a[(size_t)a * G + g0 + g] = gt_ignore[g0 + g] != 0 || ar < prm.lo[a] || ar > prm.hi[a];
    }
    const bool mask = g_i <= kMaskGts;
    unsigned char *ws = workspace + (size_t)g0 * lanes + lane;
    if (!mask && lane < lanes)
        for (int g = 0; g < g_i; ++g) ws[(size_t)g * lanes] = 0;      // a lane reads back only what it wrote itself
    __syncthreads();
    if (lane >= lanes || d_i == 0) return;
    const int a = lane / T, t = lane - a * T;
    const double lo = prm.lo[a], hi = prm.hi[a], thr = prm.thr[t];
    int32_t *dtm = dt_match + (size_t)lane * D + d0;
    unsigned char *dtig = dt_ignore + (size_t)lane * D + d0;
    const double *area = gt_area + g0, *dar = det_area + d0;
    const unsigned char *ign = gt_ignore + g0, *crowd = gt_crowd + g0;
    if (mask) {
        Matched<true> set{0ull, nullptr, lanes};
        if (staged) match_image<true>((const double *)s_oks, d_i, g_i, area, ign, crowd, dar, lo, hi, thr, set, dtm, dtig);
        else match_image<true>(oks + p0, d_i, g_i, area, ign, crowd, dar, lo, hi, thr, set, dtm, dtig);
    } else {
        Matched<false> set{0ull, ws, lanes};
        if (staged) match_image<false>((const double *)s_oks, d_i, g_i, area, ign, crowd, dar, lo, hi, thr, set, dtm, dtig);
        else match_image<false>(oks + p0, d_i, g_i, area, ign, crowd, dar, lo, hi, thr, set, dtm, dtig);
    }
}

// A pinned (host-visible) table can be read here; any other pointer gives NULL and is not an error of the call.
template <typename T>
const T *host_view(const T *p)
{
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, p) == hipSuccess && attr.type == hipMemoryTypeHost && attr.hostPointer)
        return static_cast<const T *>(attr.hostPointer);
    (void)hipGetLastError();
    return nullptr;
}

int check_tables(const char *name, const int32_t *det_off, const int32_t *gt_off, const int64_t *pair_off, int I, int D, int G,
                 int64_t n_pairs)
{
    const int32_t *dh = host_view(det_off), *gh = host_view(gt_off);
    const int64_t *ph = host_view(pair_off);
    for (int i = 0; i < I; ++i) {
        if (dh) {
            OG_REQUIRE(dh[i + 1] >= dh[i], OG_EINVAL, "%s: det_off decreases at image %d", name, i);
            OG_REQUIRE(dh[i + 1] - dh[i] <= kMaxDet, OG_EINVAL, "%s: image %d has %d detections (at most %d)", name, i, dh[i + 1] - dh[i],
                       kMaxDet);
        }
        if (gh) OG_REQUIRE(gh[i + 1] >= gh[i], OG_EINVAL, "%s: gt_off decreases at image %d", name, i);
        if (ph) OG_REQUIRE(ph[i + 1] >= ph[i], OG_EINVAL, "%s: pair_off decreases at image %d", name, i);
        if (dh && gh && ph)
            OG_REQUIRE(ph[i + 1] - ph[i] == (int64_t)(dh[i + 1] - dh[i]) * (gh[i + 1] - gh[i]), OG_EINVAL,
                       "%s: pair_off of image %d is not d_i * g_i", name, i);
    }
    if (dh) OG_REQUIRE(dh[0] == 0 && dh[I] == D, OG_EINVAL, "%s: det_off does not run from 0 to D", name);
    if (gh) OG_REQUIRE(gh[0] == 0 && gh[I] == G, OG_EINVAL, "%s: gt_off does not run from 0 to G", name);
    if (ph) OG_REQUIRE(ph[0] == 0 && ph[I] == n_pairs, OG_EINVAL, "%s: pair_off does not run from 0 to n_pairs", name);
    return OG_OK;
}

}  // namespace

OG_API int og_oks_matrix_f64(const double *dets, const double *gts, const double *gt_area, const double *gt_bbox, const int32_t *det_off,
                             const int32_t *gt_off, const int64_t *pair_off, const double *sigmas, int I, int D, int G, int64_t n_pairs,
                             double *oks, void *stream)
{
    const char *name = "og_oks_matrix_f64";
    OG_REQUIRE(dets && gts && gt_area && gt_bbox && det_off && gt_off && pair_off && sigmas && oks, OG_EINVAL, "%s: null pointer", name);
    OG_REQUIRE(I > 0, OG_EINVAL, "%s: I must be positive (got %d)", name, I);
    OG_REQUIRE(D >= 0 && G >= 0 && n_pairs >= 0 && n_pairs < ((int64_t)1 << 38), OG_EINVAL, "%s: bad totals", name);
    const int rc = check_tables(name, det_off, gt_off, pair_off, I, D, G, n_pairs);
    if (rc != OG_OK) return rc;
    if (n_pairs == 0) return OG_OK;
    Sigmas sig;
    for (int k = 0; k < kK; ++k) {
        OG_REQUIRE(sigmas[k] > 0.0, OG_EINVAL, "%s: sigmas[%d] must be positive", name, k);
        sig.var[k] = (sigmas[k] * 2.0) * (sigmas[k] * 2.0);
    }
    const unsigned blocks = (unsigned)((n_pairs + 255) / 256);
    hipLaunchKernelGGL(oks_matrix_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, dets, gts, gt_area, gt_bbox, det_off, gt_off,
                       pair_off, sig, I, D, G, n_pairs, oks);
    OG_LAUNCH_CHECK(name);
    return OG_OK;
}

OG_API size_t og_oks_match_workspace_bytes(int G, int A, int T)
{
    if (G < 0 || A < 1 || T < 1 || A > 16 || T > 16 || A * T > 64) return 0;
    return og_align_up((size_t)G * A * T, 16) + 16;
}

OG_API int og_oks_match_i32(const double *oks, const int32_t *det_off, const int32_t *gt_off, const int64_t *pair_off,
                            const double *gt_area, const unsigned char *gt_ignore, const unsigned char *gt_crowd, const double *det_area,
                            const double *area_ranges, int A, const double *thresholds, int T, int I, int D, int G, int64_t n_pairs,
                            int32_t *dt_match, unsigned char *dt_ignore, unsigned char *gt_ignore_a, void *workspace,
                            size_t workspace_bytes, void *stream)
{
    const char *name = "og_oks_match_i32";
    OG_REQUIRE(oks && det_off && gt_off && pair_off && gt_area && gt_ignore && gt_crowd && det_area && area_ranges && thresholds &&
                   dt_match && dt_ignore && gt_ignore_a && workspace,
               OG_EINVAL, "%s: null pointer", name);
    OG_REQUIRE(I > 0, OG_EINVAL, "%s: I must be positive (got %d)", name, I);
    OG_REQUIRE(A >= 1 && A <= 16 && T >= 1 && T <= 16 && A * T <= 64, OG_EINVAL,
               "%s: A and T must lie in 1..16 with A * T <= 64 (got %d, %d)", name, A, T);
    OG_REQUIRE(D >= 0 && G >= 0 && n_pairs >= 0 && n_pairs < ((int64_t)1 << 38), OG_EINVAL, "%s: bad totals", name);
    const int rc = check_tables(name, det_off, gt_off, pair_off, I, D, G, n_pairs);
    if (rc != OG_OK) return rc;
    OG_REQUIRE(workspace_bytes >= og_oks_match_workspace_bytes(G, A, T), OG_ENOSPC, "%s: workspace %zu < %zu bytes", name, workspace_bytes,
               og_oks_match_workspace_bytes(G, A, T));
    MatchParams prm = {};
    for (int a = 0; a < A; ++a) {
        prm.lo[a] = area_ranges[2 * a];
        prm.hi[a] = area_ranges[2 * a + 1];
    }
    for (int t = 0; t < T; ++t) prm.thr[t] = thresholds[t] < 1.0 - 1e-10 ? thresholds[t] : 1.0 - 1e-10;
    hipLaunchKernelGGL(oks_match_kernel, dim3((unsigned)I), dim3(64), 0, (hipStream_t)stream, oks, det_off, gt_off, pair_off, gt_area,
                       gt_ignore, gt_crowd, det_area, prm, A, T, D, G, n_pairs, dt_match, dt_ignore, gt_ignore_a,
                       static_cast<unsigned char *>(workspace));
    OG_LAUNCH_CHECK(name);
    return OG_OK;
}
