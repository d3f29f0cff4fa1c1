// mask_miss / mask_all of a batch of COCO images from their person annotations' polygons and run-length encodings (the reference's
// CocoKeypoints.mask_mask, data/dataset.py:136-197, which calls pycocotools' annToMask).  See include/og_decoder.h for the operation
// order; tests/coco_mask_common.py restates it in numpy in the sort-and-merge run-length form.
// Every polygon and every RLE ("piece") owns a column-major bit plane of its image in the workspace, 32 bits to a word:
//   coco_zero_kernel     clears the planes,
//   coco_toggle_kernel   XORs the toggle positions into them (vector atomics on words; integer XOR commutes: deterministic),
//   coco_fill_kernel     turns toggles into filled bits: bit a = XOR of the toggles at positions <= a, across column ends,
//   coco_compose_kernel  reads bit x h + y of the image's planes per output pixel and writes the two row-major uint8 planes.
// Small, latency-shaped work (a few hundred edges, a few hundred thousand pixels): no roofline fraction is claimed for it.
// All polygon arithmetic is IEEE double; the file is compiled with -ffp-contract=off and without fast-math like the rest.
#include <math.h>

#include "og_common.h"

namespace {

constexpr int kThreads = 256;
constexpr double kScale = 5.0;                     // maskApi's upsampling of the polygon grid
constexpr double kCoordLimit = 1048576.0;          // |vertex coordinate| <= 2^20: 5 p + .5 and every walk along an edge fit int32
constexpr int64_t kMaxPixels = (int64_t)1 << 28;

struct Point {
    int u, v;
};

// Vertex j of a polygon on the x5 grid: (int)(5 p + .5), the product rounded before the sum, truncated toward zero.
__device__ __forceinline__ Point grid_vertex(const double *__restrict__ xy, int j)
{
    const double px = xy[2 * j] * kScale, py = xy[2 * j + 1] * kScale;
    return Point{(int)(px + .5), (int)(py + .5)};
}

struct Edge {
    int xs, ys, n;        // start after the flip, n = max(dx, dy): the edge emits n + 1 points
    double s;
    bool along_x, flip;
};

__device__ __forceinline__ Edge make_edge(Point a, Point b)
{
    int xs = a.u, ys = a.v, xe = b.u, ye = b.v;
    const int dx = abs(xe - xs), dy = abs(ys - ye);
    Edge e;
    e.along_x = dx >= dy;
    e.flip = (dx >= dy && xs > xe) || (dx < dy && ys > ye);
    if (e.flip) {
        int t = xs; xs = xe; xe = t;
        t = ys; ys = ye; ye = t;
    }
    e.xs = xs;
    e.ys = ys;
    e.n = e.along_x ? dx : dy;
    e.s = e.n == 0 ? 0.0 : (e.along_x ? (double)(ye - ys) / (double)dx : (double)(xe - xs) / (double)dy);
    return e;
}

// Point number i (0..n, in emission order) of an edge.
__device__ __forceinline__ Point edge_point(const Edge &e, int i)
{
    if (e.n == 0) return Point{e.xs, e.ys};
    const int t = e.flip ? e.n - i : i;
    const double st = e.s * (double)t;
    if (e.along_x) return Point{e.xs + t, (int)(((double)e.ys + st) + .5)};
    return Point{(int)(((double)e.xs + st) + .5), e.ys + t};
}

__global__ __launch_bounds__(kThreads) void coco_zero_kernel(uint4 *__restrict__ ws, size_t n16)
{
    for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < n16; i += (size_t)gridDim.x * kThreads) ws[i] = make_uint4(0, 0, 0, 0);
}

// One workgroup per piece.  Polygon: edge by edge, the lanes over the edge's points; a point's predecessor in the one sequence of all
// edges is the point before it on its edge or the last point of the edge before.  RLE: the lanes over the cumulative sums.
__global__ __launch_bounds__(kThreads) void coco_toggle_kernel(const OgCocoImage *__restrict__ images, const OgCocoPiece *__restrict__ pieces,
                                                               const double *__restrict__ vertices, const uint32_t *__restrict__ cums,
                                                               int n_images, unsigned *__restrict__ ws)
{
    const OgCocoPiece pc = pieces[blockIdx.x];
    if (pc.image < 0 || pc.image >= n_images || pc.count <= 0) return;
    const int h = images[pc.image].h, w = images[pc.image].w;
    const unsigned hw = (unsigned)h * (unsigned)w;
    unsigned *plane = ws + pc.word_off;
    if (pc.kind == OG_COCO_RLE) {
        const uint32_t *c = cums + pc.first;
        for (int i = threadIdx.x; i < pc.count; i += kThreads) {
            const unsigned a = c[i];
            if (a < hw) atomicXor(plane + (a >> 5), 1u << (a & 31));
        }
        return;
    }
    const double *xy = vertices + 2 * (size_t)pc.first;
    const int k = pc.count;
    for (int j = 0; j < k; ++j) {
        const Edge e = make_edge(grid_vertex(xy, j), grid_vertex(xy, j + 1 == k ? 0 : j + 1));
        Point last_before = Point{0, 0};
        if (j > 0) {
            const Edge b = make_edge(grid_vertex(xy, j - 1), grid_vertex(xy, j));
            last_before = edge_point(b, b.n);
        }
        for (int i = threadIdx.x; i <= e.n; i += kThreads) {
            if (i == 0 && j == 0) continue;                    // the first point of the sequence has no predecessor
            const Point p = edge_point(e, i), q = i > 0 ? edge_point(e, i - 1) : last_before;
            if (p.u == q.u) continue;
            double xd = (double)(p.u < q.u ? p.u : p.u - 1);
            xd = (xd + .5) / kScale - .5;
            if (floor(xd) != xd || xd < 0.0 || xd > (double)(w - 1)) continue;
            double yd = (double)(p.v < q.v ? p.v : q.v);
            yd = (yd + .5) / kScale - .5;
            if (yd < 0.0) yd = 0.0;
            else if (yd > (double)h) yd = (double)h;
            yd = ceil(yd);
            const unsigned a = (unsigned)(int)xd * (unsigned)h + (unsigned)(int)yd;
            if (a < hw) atomicXor(plane + (a >> 5), 1u << (a & 31));        // a toggle at h w has no effect
        }
    }
}

// One workgroup per piece: bit a of the plane becomes the XOR of the toggles at positions <= a.  In a word five shift-XOR steps; the
// words' parities are scanned over the wave with a ballot, over the workgroup through LDS, and carried from chunk to chunk.
__global__ __launch_bounds__(kThreads) void coco_fill_kernel(const OgCocoImage *__restrict__ images, const OgCocoPiece *__restrict__ pieces,
                                                             int n_images, unsigned *__restrict__ ws)
{
    __shared__ unsigned s_par[2][kThreads / 64];
    const OgCocoPiece pc = pieces[blockIdx.x];
    if (pc.image < 0 || pc.image >= n_images) return;
    const unsigned hw = (unsigned)images[pc.image].h * (unsigned)images[pc.image].w;
    const unsigned n_words = (hw + 31) >> 5;
    unsigned *plane = ws + pc.word_off;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned carry = 0;
    int turn = 0;
    for (unsigned base = 0; base < n_words; base += kThreads, turn ^= 1) {
        const unsigned idx = base + threadIdx.x;
        unsigned x = idx < n_words ? plane[idx] : 0u;
        x ^= x << 1;
        x ^= x << 2;
        x ^= x << 4;
        x ^= x << 8;
        x ^= x << 16;
        const unsigned long long odd = __ballot(x >> 31);
        unsigned before = __popcll(odd & ((1ull << lane) - 1ull)) & 1u;
        if (lane == 0) s_par[turn][wave] = __popcll(odd) & 1u;
        __syncthreads();
        unsigned all = 0;
        for (int v = 0; v < kThreads / 64; ++v) {
            const unsigned p = s_par[turn][v];
            if (v < wave) before ^= p;
            all ^= p;
        }
        if (before ^ carry) x = ~x;
        if (idx < n_words) plane[idx] = x;
        carry ^= all;
    }
}

// One thread per output pixel of image blockIdx.y; the annotations in list order (include/og_decoder.h: composition).
__global__ __launch_bounds__(kThreads) void coco_compose_kernel(const OgCocoImage *__restrict__ images, const OgCocoAnn *__restrict__ anns,
                                                                const OgCocoPiece *__restrict__ pieces, int n_anns, int n_pieces,
                                                                const unsigned *__restrict__ ws, unsigned char *__restrict__ mask_miss,
                                                                unsigned char *__restrict__ mask_all)
{
    const OgCocoImage im = images[blockIdx.y];
    const unsigned hw = (unsigned)im.h * (unsigned)im.w;
    const unsigned p = blockIdx.x * kThreads + threadIdx.x;
    if (p >= hw) return;
    const unsigned y = p / (unsigned)im.w, x = p - y * (unsigned)im.w;
    const unsigned a = x * (unsigned)im.h + y;
    const unsigned word = a >> 5, bit = a & 31;
    unsigned persons = 0, miss = 0, crowd = 0;
    for (int j = 0; j < im.n_anns; ++j) {
        const int ai = im.ann_first + j;
        if (ai < 0 || ai >= n_anns) break;
        const OgCocoAnn an = anns[ai];
        unsigned m = 0;
        for (int q = 0; q < an.n_pieces; ++q) {
            const int pi = an.piece_first + q;
            if (pi < 0 || pi >= n_pieces) break;
            m |= ws[pieces[pi].word_off + word] >> bit;
        }
        m &= 1u;
        if (an.flags & OG_COCO_CROWD) {
            crowd |= m & ~persons;
        } else {
            persons |= m;
            if (an.flags & OG_COCO_MISS) miss |= m;
        }
    }
    mask_miss[im.out_off + p] = (miss | crowd) ? 0 : 255;
    if (mask_all) mask_all[im.out_off + p] = (persons | crowd) ? 255 : 0;
}

struct Tables {
    const OgCocoImage *images;
    const OgCocoAnn *anns;
    const OgCocoPiece *pieces;
    const double *vertices;
    const uint32_t *cums;
};

Tables tables_at(const OgCocoMaskDesc *d, const void *base)
{
    const char *b = static_cast<const char *>(base);
    return Tables{reinterpret_cast<const OgCocoImage *>(b + d->images_at), reinterpret_cast<const OgCocoAnn *>(b + d->anns_at),
                  reinterpret_cast<const OgCocoPiece *>(b + d->pieces_at), reinterpret_cast<const double *>(b + d->vertices_at),
                  reinterpret_cast<const uint32_t *>(b + d->cums_at)};
}

size_t plane_words(const OgCocoImage &im) { return ((size_t)im.h * (size_t)im.w + 31) / 32; }

// The descriptor and the host copy of the tables; *words receives the planes' total size and *max_hw the largest image.
int validate(const char *name, const OgCocoMaskDesc *d, size_t *words, int64_t *max_hw)
{
    OG_REQUIRE(d, OG_EINVAL, "%s: null pointer", name);
    OG_REQUIRE(d->size == sizeof(OgCocoMaskDesc), OG_EINVAL, "%s: descriptor size %u, this library's OgCocoMaskDesc has %zu bytes", name,
               d->size, sizeof(OgCocoMaskDesc));
    OG_REQUIRE(d->tables_host, OG_EINVAL, "%s: null pointer", name);
    OG_REQUIRE(d->stages >= 0 && d->stages <= 15, OG_EINVAL, "%s: stages must lie in 0..15 (got %d)", name, d->stages);
    OG_REQUIRE(d->n_images > 0 && d->n_images <= 65535, OG_EINVAL, "%s: n_images must lie in 1..65535 (got %d)", name, d->n_images);
    OG_REQUIRE(d->n_anns >= 0 && d->n_pieces >= 0 && d->n_vertices >= 0 && d->n_cums >= 0 && d->n_pieces <= (1 << 24), OG_EINVAL,
               "%s: negative count (or more than 2^24 pieces)", name);
    const size_t need[5] = {(size_t)d->n_images * sizeof(OgCocoImage), (size_t)d->n_anns * sizeof(OgCocoAnn),
                            (size_t)d->n_pieces * sizeof(OgCocoPiece), (size_t)d->n_vertices * 16, (size_t)d->n_cums * 4};
    const size_t at[5] = {d->images_at, d->anns_at, d->pieces_at, d->vertices_at, d->cums_at};
    for (int s = 0; s < 5; ++s)
        OG_REQUIRE(at[s] % 16 == 0 && at[s] <= d->table_bytes && need[s] <= d->table_bytes - at[s], OG_EINVAL,
                   "%s: table section %d is not 16-byte aligned or leaves the %zu table bytes", name, s, d->table_bytes);
    const Tables t = tables_at(d, d->tables_host);
    int ann_next = 0, piece_next = 0;
    *words = 0;
    *max_hw = 0;
    for (int i = 0; i < d->n_images; ++i) {
        const OgCocoImage &im = t.images[i];
        OG_REQUIRE(im.h > 0 && im.w > 0, OG_EINVAL, "%s: image %d has size %d x %d", name, i, im.h, im.w);
        const int64_t hw = (int64_t)im.h * im.w;
        OG_REQUIRE(hw <= kMaxPixels, OG_EINVAL, "%s: image %d has h w = %lld beyond 2^28", name, i, (long long)hw);
        OG_REQUIRE(im.out_off >= 0 && (uint64_t)im.out_off + (uint64_t)hw <= (uint64_t)d->out_bytes, OG_EINVAL,
                   "%s: the planes of image %d leave the %zu output bytes", name, i, d->out_bytes);
        OG_REQUIRE(im.ann_first == ann_next && im.n_anns >= 0 && im.n_anns <= d->n_anns - ann_next, OG_EINVAL,
                   "%s: the annotations of image %d do not follow those of the image before", name, i);
        ann_next += im.n_anns;
        if (hw > *max_hw) *max_hw = hw;
        for (int j = im.ann_first; j < ann_next; ++j) {
            const OgCocoAnn &an = t.anns[j];
            OG_REQUIRE(an.piece_first == piece_next && an.n_pieces >= 0 && an.n_pieces <= d->n_pieces - piece_next, OG_EINVAL,
                       "%s: the pieces of annotation %d do not follow those of the annotation before", name, j);
            OG_REQUIRE((an.flags & ~(OG_COCO_CROWD | OG_COCO_MISS)) == 0, OG_EINVAL, "%s: annotation %d has flags %d", name, j, an.flags);
            piece_next += an.n_pieces;
            for (int q = an.piece_first; q < piece_next; ++q) {
                const OgCocoPiece &pc = t.pieces[q];
                OG_REQUIRE(pc.image == i, OG_EINVAL, "%s: piece %d names image %d, its annotation belongs to image %d", name, q, pc.image, i);
                OG_REQUIRE(pc.word_off == (int64_t)*words, OG_EINVAL, "%s: the plane of piece %d does not follow the plane before", name, q);
                *words += plane_words(im);
                if (pc.kind == OG_COCO_POLYGON) {
                    OG_REQUIRE(pc.count >= 1, OG_EINVAL, "%s: polygon %d has fewer than 1 vertex", name, q);
                    OG_REQUIRE(pc.first >= 0 && pc.first <= d->n_vertices - pc.count, OG_EINVAL, "%s: polygon %d leaves the vertex table", name,
                               q);
                    for (int v = 2 * pc.first; v < 2 * (pc.first + pc.count); ++v) {
                        OG_REQUIRE(__builtin_isfinite(t.vertices[v]), OG_EINVAL, "%s: polygon %d has a non-finite vertex", name, q);
                        OG_REQUIRE(fabs(t.vertices[v]) <= kCoordLimit, OG_EINVAL, "%s: polygon %d has a coordinate beyond 2^20", name, q);
                    }
                } else if (pc.kind == OG_COCO_RLE) {
                    OG_REQUIRE(pc.count >= 1 && pc.first >= 0 && pc.first <= d->n_cums - pc.count, OG_EINVAL,
                               "%s: RLE %d is empty or leaves the table of cumulative sums", name, q);
                    uint32_t prev = 0;
                    for (int c = pc.first; c < pc.first + pc.count; ++c) {
                        OG_REQUIRE(t.cums[c] >= prev, OG_EINVAL, "%s: RLE %d has a negative run", name, q);
                        prev = t.cums[c];
                    }
                    OG_REQUIRE((int64_t)prev == hw, OG_EINVAL, "%s: the runs of RLE %d sum to %u, not to h w = %lld", name, q, prev,
                               (long long)hw);
                } else {
                    OG_REQUIRE(false, OG_EINVAL, "%s: piece %d has kind %d", name, q, pc.kind);
                }
            }
        }
    }
    OG_REQUIRE(ann_next == d->n_anns && piece_next == d->n_pieces, OG_EINVAL, "%s: the images own %d of %d annotations, %d of %d pieces",
               name, ann_next, d->n_anns, piece_next, d->n_pieces);
    return OG_OK;
}

size_t bytes_of_words(size_t words) { return og_align_up(words * 4, 16) + 16; }

}  // namespace

OG_API size_t og_coco_mask_workspace_bytes(const OgCocoMaskDesc *desc)
{
    size_t words = 0;
    int64_t max_hw = 0;
    if (validate("og_coco_mask_workspace_bytes", desc, &words, &max_hw) != OG_OK) return 0;
    return bytes_of_words(words);
}

OG_API int og_coco_masks_u8(const OgCocoMaskDesc *desc, void *workspace, size_t workspace_bytes, void *stream)
{
    const char *name = "og_coco_masks_u8";
    size_t words = 0;
    int64_t max_hw = 0;
    const int rc = validate(name, desc, &words, &max_hw);
    if (rc != OG_OK) return rc;
    OG_REQUIRE(desc->tables_dev && desc->mask_miss && workspace, OG_EINVAL, "%s: null pointer", name);
    OG_REQUIRE((uintptr_t)workspace % 16 == 0 && (uintptr_t)desc->tables_dev % 16 == 0, OG_EINVAL,
               "%s: workspace and tables must be 16-byte aligned", name);
    OG_REQUIRE(workspace_bytes >= bytes_of_words(words), OG_ENOSPC, "%s: workspace %zu < %zu bytes", name, workspace_bytes,
               bytes_of_words(words));
    const Tables t = tables_at(desc, desc->tables_dev);
    hipStream_t st = (hipStream_t)stream;
    unsigned *ws = static_cast<unsigned *>(workspace);
    const int stages = desc->stages ? desc->stages : 15;
    if (desc->n_pieces > 0 && (stages & 1)) {
        const size_t n16 = og_align_up(words * 4, 16) / 16;
        const unsigned blocks = (unsigned)((n16 + kThreads - 1) / kThreads < 4096 ? (n16 + kThreads - 1) / kThreads : 4096);
        hipLaunchKernelGGL(coco_zero_kernel, dim3(blocks), dim3(kThreads), 0, st, static_cast<uint4 *>(workspace), n16);
        OG_LAUNCH_CHECK(name);
    }
    if (desc->n_pieces > 0 && (stages & 2)) {
        hipLaunchKernelGGL(coco_toggle_kernel, dim3((unsigned)desc->n_pieces), dim3(kThreads), 0, st, t.images, t.pieces, t.vertices, t.cums,
                           desc->n_images, ws);
        OG_LAUNCH_CHECK(name);
    }
    if (desc->n_pieces > 0 && (stages & 4)) {
        hipLaunchKernelGGL(coco_fill_kernel, dim3((unsigned)desc->n_pieces), dim3(kThreads), 0, st, t.images, t.pieces, desc->n_images, ws);
        OG_LAUNCH_CHECK(name);
    }
    if (stages & 8) {
        const unsigned bx = (unsigned)((max_hw + kThreads - 1) / kThreads);
        hipLaunchKernelGGL(coco_compose_kernel, dim3(bx, (unsigned)desc->n_images), dim3(kThreads), 0, st, t.images, t.anns, t.pieces,
                           desc->n_anns, desc->n_pieces, ws, desc->mask_miss, desc->mask_all);
        OG_LAUNCH_CHECK(name);
    }
    return OG_OK;
}
