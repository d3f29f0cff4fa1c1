// Multi-tensor optimizer step without a host wait (include/og_decoder.h, "training step"): the sum of squares of every gradient,
// the device-side gradient scale (clip coefficient and batch drop in one number) and the Adam / SGD update, each ONE launch over a
// table of tensors.  Memory-bound streaming kernels: one workgroup of 256 threads per chunk of OPTIM_CHUNK elements of one tensor,
// 16-byte loads and stores wherever a tensor's address allows them, a scalar head and tail where it does not.  The arithmetic is the
// header's list of individually rounded fp32 operations (the library is built with -ffp-contract=off, correctly rounded divide and
// sqrt): tests/optim_common.py restates it in numpy and the GPU tests compare bit for bit.  No float atomics anywhere: the sum of
// squares goes through per-chunk partials in double and a fixed-order reduction.  There is ONE update kernel, update_kernel<Rule,
// EMA>: the rule (AdamRule, SgdRule<HAS_BUF>) says which moment columns exist and holds the per-element arithmetic, the kernel
// walks, loads and stores.  With EMA a row that has an average (the `ema` address table) folds e' = e + omd * (p' - e) into the
// store of p', 8 B per parameter more and no second pass over p.  ema_lerp_kernel, the same three lines over the tensors no update
// touches, is a kernel of its own on the shared helpers: its rows are (e, x, numel) and its frame is e's, which as a rule would put
// a row-layout branch into every update.  There is ONE scale block, step_scale_kernel<AMP>: the plain form is the scaler form with
// S = 1, static, and touches no scaler word.
#include "table.h"

namespace {

constexpr int OPTIM_THREADS = 256;
constexpr int OPTIM_CHUNK = 8192;            // elements of one tensor per workgroup: 8 float4 per thread
constexpr int OPTIM_STATE_BYTES = 16;        // [scale f32, norm f32, dropped i32, pad]; the double partials follow
constexpr int SCALE_THREADS = 1024;

struct Row {
    gfloat *p;
    const gfloat *g;
    gfloat *m;
    gfloat *v;
    long n;
    int index;         // the row's place in the table (and in the `ema` address table beside it)
};

struct Span {          // what a workgroup owns: elements [lo, hi) of its row; vectors of four from element vs, f.n_vec of them
    long lo, hi, vs;
    OgFrame f;
};

// false: nothing to do (an offset at or past the row's end -- a table that does not match its prefix)
__device__ __forceinline__ bool span_of(const int32_t *prefix, int r, int chunk, long n, Span &s)
{
    s.lo = (long)(chunk - prefix[r]) * OPTIM_CHUNK;
    if (s.lo < 0 || s.lo >= n) return false;
    s.hi = n - s.lo > OPTIM_CHUNK ? s.lo + OPTIM_CHUNK : n;
    return true;
}

__device__ __forceinline__ bool locate(const int64_t *rows, const int32_t *prefix, int n_rows, int chunk, Row &row, Span &s)
{
    const int r = og_find_row(prefix, n_rows, chunk);
    const int64_t *e = rows + (size_t)r * 5;
    row.p = (gfloat *)(uintptr_t)e[0];
    row.g = (const gfloat *)(uintptr_t)e[1];
    row.m = (gfloat *)(uintptr_t)e[2];
    row.v = (gfloat *)(uintptr_t)e[3];
    row.n = e[4];
    row.index = r;
    return span_of(prefix, r, chunk, row.n, s);
}

// The vector frame of a span (table.h) is anchored on `anchor` (p for the updates, g for the sum of squares, e for the lerp), given
// at element lo.
__device__ __forceinline__ void frame(const gfloat *anchor, Span &s)
{
    s.f = og_frame(anchor, (int)(s.hi - s.lo), 4);
    s.vs = s.lo + s.f.head;
}

__device__ __forceinline__ bool aligned16(const gfloat *q) { return ((uintptr_t)q & 15u) == 0; }

__device__ __forceinline__ f4 load4(const gfloat *q, bool vec)
{
    if (vec) return *(const gf4 *)q;
    f4 x;
    x.x = q[0];
    x.y = q[1];
    x.z = q[2];
    x.w = q[3];
    return x;
}

__device__ __forceinline__ void store4(gfloat *q, bool vec, f4 x)
{
    if (vec) {
        *(gf4 *)q = x;
    } else {
        q[0] = x.x;
        q[1] = x.y;
        q[2] = x.z;
        q[3] = x.w;
    }
}

// The scalar element of this thread as an element of the row, or -1
__device__ __forceinline__ long edge_element(const Span &s)
{
    const int e = og_frame_edge(s.f, (int)(s.hi - s.lo));
    return e < 0 ? -1 : s.lo + e;
}

// ---- sum of squares ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(OPTIM_THREADS) void grad_sumsq_kernel(const int64_t *__restrict__ rows, const int32_t *__restrict__ prefix,
                                                                   int n_rows, double *__restrict__ partials)
{
    __shared__ double wave_sum[OPTIM_THREADS / 64];
    Row row;
    Span s;
    double acc = 0.0;
    if (locate(rows, prefix, n_rows, blockIdx.x, row, s)) {
        frame(row.g + s.lo, s);
        for (int k = threadIdx.x; k < s.f.n_vec; k += OPTIM_THREADS) {
            const f4 g = *(const gf4 *)(row.g + s.vs + 4L * k);
            acc += (double)g.x * (double)g.x;
            acc += (double)g.y * (double)g.y;
            acc += (double)g.z * (double)g.z;
            acc += (double)g.w * (double)g.w;
        }
        const long e = edge_element(s);
        if (e >= 0) {
            const double g = (double)row.g[e];
            acc += g * g;
        }
    }
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partials[blockIdx.x] = ((wave_sum[0] + wave_sum[1]) + wave_sum[2]) + wave_sum[3];
}

// ---- the scale block -----------------------------------------------------------------------------------------------------------
// One workgroup.  Thread t sums its contiguous share of the partials in index order; the 1024 thread sums are added in index order
// sixteen at a time by wave 0, whose lanes are folded by a shuffle tree: one fixed order for a given number of partials.  True on
// thread 0 alone, which then holds the sum in n2.
__device__ __forceinline__ bool sum_partials(const double *__restrict__ partials, int n_partials, double &n2)
{
    __shared__ double sums[SCALE_THREADS];
    const int per = (n_partials + SCALE_THREADS - 1) / SCALE_THREADS;
    const int first = threadIdx.x * per;
    const int last = first + per < n_partials ? first + per : n_partials;
    double acc = 0.0;
    for (int i = first; i < last; ++i) acc += partials[i];
    sums[threadIdx.x] = acc;
    __syncthreads();
    if (threadIdx.x >= 64) return false;
    double a = 0.0;
    for (int i = 0; i < SCALE_THREADS / 64; ++i) a += sums[threadIdx.x * (SCALE_THREADS / 64) + i];
    for (int off = 32; off > 0; off >>= 1) a += __shfl_down(a, off, 64);
    n2 = a;
    return threadIdx.x == 0;
}

// c of torch.nn.utils.clip_grad_norm_ from the fp32 norm
__device__ __forceinline__ float clip_coefficient(float norm, float max_norm)
{
    if (!isfinite(max_norm)) return 1.f;
    const float den = norm + 1e-6f;
    const float c = max_norm / den;
    return c < 1.f ? c : 1.f;
}

struct AmpArgs {
    int dynamic;
    float factor;
    int window;
    float min_scale, max_scale;
};

// Thread 0 turns the sum of squares into the state block the updates read.  AMP (header: og_step_scale_amp_f32): the gradients
// carry the factor S = scaler[0]; the scale unscales and clips in one number, an overflow skips the step and moves S.  Without AMP
// (og_step_scale_f32) S = 1, static: the same lines, `scaler` is never touched and `a` is never read.  Plain loads and stores.
template <bool AMP>
__global__ __launch_bounds__(SCALE_THREADS) void step_scale_kernel(const double *__restrict__ partials, int n_partials,
                                                                   const float *__restrict__ loss, float loss_limit, float max_norm,
                                                                   float *__restrict__ state, float *__restrict__ scaler, AmpArgs a)
{
    double n2;
    if (!sum_partials(partials, n_partials, n2)) return;
    int *words = reinterpret_cast<int *>(scaler);          // [1] unskipped, [2] overflows, [3] last_overflow
    const float S = AMP ? scaler[0] : 1.f;
    const bool dynamic = AMP && a.dynamic;
    const bool overflow = !isfinite(n2);
    const double root = sqrt(n2);
    const double unscaled = root / (double)S;
    const float norm = (float)unscaled;
    // a dynamic scaler answers for an overflow itself (a skipped step, not an exploding batch); everything else that zeroes the
    // scale is ONE dropped step
    const bool drop = overflow ? !dynamic : (loss != nullptr && *loss > loss_limit);
    float scale = 0.f;
    if (!overflow && !drop) {
        const float inv = 1.f / S;
        const float c = clip_coefficient(norm, max_norm);
        scale = c * inv;
    }
    state[0] = scale;
    state[1] = norm;
    if (drop) reinterpret_cast<int *>(state)[2] += 1;
    if (AMP) words[3] = overflow;
    if (dynamic) {
        float next = S;
        int u = words[1];
        if (overflow) {
            const float t = S / a.factor;
            next = t < a.min_scale ? a.min_scale : t;
            u = 0;
            words[2] += 1;
        } else {
            u = u + 1;
            if (u == a.window) {
                const float t = S * a.factor;
                next = t > a.max_scale ? a.max_scale : t;
                u = 0;
            }
        }
        scaler[0] = next;
        words[1] = u;
    }
}

// ---- updates -------------------------------------------------------------------------------------------------------------------
// A rule: HAS_M / HAS_V (which moment columns of the row exist: they are written when they do), reads_m() (m is also read) and
// element(), the header's list for ONE element, every line one individually rounded fp32 operation.
struct AdamArgs {
    float lr, b1, b2, omb1, omb2, eps, wd, bc1, bc2;
    int adam_w_mode;
};

struct AdamRule {
    static constexpr bool HAS_M = true, HAS_V = true;
    AdamArgs a;

    __device__ __forceinline__ bool reads_m() const { return true; }

    __device__ __forceinline__ void element(float scale, float &p, float g, float &m, float &v) const
    {
        float ge = (scale == 0.f) ? 0.f : g * scale;
        if (a.wd != 0.f && !a.adam_w_mode) {
            const float t = a.wd * p;
            ge = ge + t;
        }
        const float x = a.b1 * m;
        const float y = a.omb1 * ge;
        m = x + y;
        const float c = a.b2 * v;
        const float d = a.omb2 * ge;
        const float e = d * ge;
        v = c + e;
        const float mh = m / a.bc1;
        const float q = v / a.bc2;
        const float r = sqrtf(q);
        const float den = r + a.eps;
        float u = mh / den;
        if (a.wd != 0.f && a.adam_w_mode) {
            const float t = a.wd * p;
            u = u + t;
        }
        const float s = a.lr * u;
        p = p - s;
    }
};

struct SgdArgs {
    float lr, mom, wd;
    int first;
};

// m is the momentum buffer: read only when HAS_BUF && !first, written only when HAS_BUF
template <bool HAS_BUF>
struct SgdRule {
    static constexpr bool HAS_M = HAS_BUF, HAS_V = false;
    SgdArgs a;

    __device__ __forceinline__ bool reads_m() const { return HAS_BUF && !a.first; }

    __device__ __forceinline__ void element(float scale, float &p, float g, float &m, float &) const
    {
        float ge = (scale == 0.f) ? 0.f : g * scale;
        if (a.wd != 0.f) {
            const float t = a.wd * p;
            ge = ge + t;
        }
        float step = ge;
        if (HAS_BUF) {
            if (!a.first) {
                const float t = a.mom * m;
                step = t + ge;
            }
            m = step;
        }
        const float s = a.lr * step;
        p = p - s;
    }
};

// The average behind an update (header: "weight average"): x is p' as it is stored, three individually rounded operations.
__device__ __forceinline__ float ema_element(float omd, float x, float e)
{
    const float d = x - e;
    const float t = omd * d;
    return e + t;
}

__device__ __forceinline__ void ema4(float omd, const f4 &x, f4 &e)
{
#pragma unroll
    for (int c = 0; c < 4; ++c) e[c] = ema_element(omd, x[c], e[c]);
}

// The frame is p's; g, the moments and the average take 16-byte accesses on their own alignment.  A row whose `ema` address is 0
// is stepped without an average; without EMA the `ema` table is never read.
template <class Rule, bool EMA>
__global__ __launch_bounds__(OPTIM_THREADS) void update_kernel(const int64_t *__restrict__ rows, const int32_t *__restrict__ prefix,
                                                               int n_rows, int chunk_first, const float *__restrict__ state, Rule rule,
                                                               const int64_t *__restrict__ ema, float omd)
{
    Row row;
    Span s;
    if (!locate(rows, prefix, n_rows, chunk_first + blockIdx.x, row, s)) return;
    const float scale = state ? state[0] : 1.f;
    frame(row.p + s.lo, s);
    const bool gv = aligned16(row.g + s.vs), mv = Rule::HAS_M && aligned16(row.m + s.vs), vv = Rule::HAS_V && aligned16(row.v + s.vs);
    const bool read_m = rule.reads_m();
    gfloat *const avg = EMA ? (gfloat *)(uintptr_t)ema[row.index] : nullptr;
    const bool has_avg = EMA && avg != nullptr, ev = has_avg && aligned16(avg + s.vs);
#pragma unroll 2
    for (int k = threadIdx.x; k < s.f.n_vec; k += OPTIM_THREADS) {
        const long i = s.vs + 4L * k;
        f4 p = *(const gf4 *)(row.p + i);
        const f4 g = load4(row.g + i, gv);
        f4 m = {0.f, 0.f, 0.f, 0.f}, v = m, e = m;
        if (read_m) m = load4(row.m + i, mv);
        if (Rule::HAS_V) v = load4(row.v + i, vv);
        if (has_avg) e = load4(avg + i, ev);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            float p_ = p[c], m_ = m[c], v_ = v[c];
            rule.element(scale, p_, g[c], m_, v_);
            p[c] = p_, m[c] = m_, v[c] = v_;
        }
        *(gf4 *)(row.p + i) = p;
        if (Rule::HAS_M) store4(row.m + i, mv, m);
        if (Rule::HAS_V) store4(row.v + i, vv, v);
        if (has_avg) {
            ema4(omd, p, e);
            store4(avg + i, ev, e);
        }
    }
    const long j = edge_element(s);
    if (j >= 0) {
        float p = row.p[j], m = read_m ? row.m[j] : 0.f, v = Rule::HAS_V ? row.v[j] : 0.f;
        rule.element(scale, p, row.g[j], m, v);
        row.p[j] = p;
        if (Rule::HAS_M) row.m[j] = m;
        if (Rule::HAS_V) row.v[j] = v;
        if (has_avg) avg[j] = ema_element(omd, p, avg[j]);
    }
}

// ---- the average of what no update touches ---------------------------------------------------------------------------------------
// rows (e, x, numel); the vector frame is anchored on e, the tensor that is written.
__global__ __launch_bounds__(OPTIM_THREADS) void ema_lerp_kernel(const int64_t *__restrict__ rows, const int32_t *__restrict__ prefix,
                                                                 int n_rows, float omd)
{
    const int r = og_find_row(prefix, n_rows, blockIdx.x);
    const int64_t *w = rows + (size_t)r * 3;
    gfloat *const avg = (gfloat *)(uintptr_t)w[0];
    const gfloat *const x = (const gfloat *)(uintptr_t)w[1];
    Span s;
    if (!span_of(prefix, r, blockIdx.x, w[2], s)) return;
    frame(avg + s.lo, s);
    const bool xv = aligned16(x + s.vs);
#pragma unroll 2
    for (int k = threadIdx.x; k < s.f.n_vec; k += OPTIM_THREADS) {
        const long i = s.vs + 4L * k;
        f4 e = *(const gf4 *)(avg + i);
        const f4 src = load4(x + i, xv);
        ema4(omd, src, e);
        *(gf4 *)(avg + i) = e;
    }
    const long i = edge_element(s);
    if (i >= 0) {
        avg[i] = ema_element(omd, x[i], avg[i]);
    }
}

}  // namespace

OG_API int og_optim_chunk_elems(void) { return OPTIM_CHUNK; }

OG_API size_t og_optim_workspace_bytes(int n_chunks)
{
    return n_chunks < 0 ? 0 : (size_t)OPTIM_STATE_BYTES + (size_t)n_chunks * sizeof(double);
}

// ---- what the entry points share -------------------------------------------------------------------------------------------------
// The workspace of n_chunks chunks and its two parts
static int split_workspace(const char *name, int n_chunks, void *workspace, size_t workspace_bytes, float *&state, double *&partials)
{
    OG_REQUIRE(workspace && ((uintptr_t)workspace & 7u) == 0, OG_EINVAL, "%s: null or misaligned workspace", name);
    OG_REQUIRE(workspace_bytes >= og_optim_workspace_bytes(n_chunks), OG_ENOSPC, "%s: workspace of %zu bytes, %zu needed", name,
               workspace_bytes, og_optim_workspace_bytes(n_chunks));
    state = static_cast<float *>(workspace);
    partials = reinterpret_cast<double *>(static_cast<char *>(workspace) + OPTIM_STATE_BYTES);
    return OG_OK;
}

static int check_scale(const char *name, int n_chunks, const float *loss, float loss_limit, float max_norm, void *workspace,
                       size_t workspace_bytes, float *&state, double *&partials)
{
    OG_REQUIRE(n_chunks >= 0, OG_EINVAL, "%s: negative chunk count", name);
    if (int rc = split_workspace(name, n_chunks, workspace, workspace_bytes, state, partials)) return rc;
    OG_REQUIRE(!(max_norm != max_norm) && !(loss_limit != loss_limit), OG_EINVAL, "%s: NaN max_norm or loss_limit", name);
    OG_REQUIRE(((uintptr_t)loss & 3u) == 0, OG_EINVAL, "%s: misaligned loss", name);
    return OG_OK;
}

// with_ema: the _ema form of an update's entry point, which alone looks at `ema` and `omd`
static int check_update(const char *name, bool with_ema, const int64_t *rows, const int32_t *chunk_prefix, int n_rows, int chunk_first,
                        int n_chunks, const void *state, const int64_t *ema, float omd)
{
    if (int rc = og_check_table(name, rows, chunk_prefix, n_rows, n_chunks)) return rc;
    OG_REQUIRE(chunk_first >= 0, OG_EINVAL, "%s: negative first chunk %d", name, chunk_first);
    OG_REQUIRE(((uintptr_t)state & 3u) == 0, OG_EINVAL, "%s: misaligned state block", name);
    if (with_ema) {
        OG_REQUIRE(ema && ((uintptr_t)ema & 7u) == 0, OG_EINVAL, "%s: null or misaligned ema table", name);
        OG_REQUIRE(omd >= 0.f && omd <= 1.f, OG_EINVAL, "%s: omd = 1 - decay must lie in [0, 1] (got %g)", name, omd);      // a NaN fails it
    }
    return OG_OK;
}

// Behind check_update: with_ema == false launches the instantiation that never reads `ema`.
template <class Rule>
static int launch_update(const char *name, bool with_ema, const int64_t *rows, const int32_t *chunk_prefix, int n_rows, int chunk_first,
                         int n_chunks, const void *state, const Rule &rule, const int64_t *ema, float omd, void *stream)
{
    if (n_chunks == 0) return OG_OK;
    const auto kernel = with_ema ? update_kernel<Rule, true> : update_kernel<Rule, false>;
    hipLaunchKernelGGL(kernel, dim3(n_chunks), dim3(OPTIM_THREADS), 0, (hipStream_t)stream, rows, chunk_prefix, n_rows, chunk_first,
                       static_cast<const float *>(state), rule, ema, omd);
    OG_LAUNCH_CHECK(name);
    return OG_OK;
}

// ---- entry points ----------------------------------------------------------------------------------------------------------------
OG_API int og_grad_sumsq_f32(const int64_t *rows, const int32_t *chunk_prefix, int n_rows, int n_chunks, void *workspace,
                             size_t workspace_bytes, void *stream)
{
    const char *name = "og_grad_sumsq_f32";
    float *state;
    double *partials;
    if (int rc = og_check_table(name, rows, chunk_prefix, n_rows, n_chunks)) return rc;
    if (int rc = split_workspace(name, n_chunks, workspace, workspace_bytes, state, partials)) return rc;
    if (n_chunks == 0) return OG_OK;
    hipLaunchKernelGGL(grad_sumsq_kernel, dim3(n_chunks), dim3(OPTIM_THREADS), 0, (hipStream_t)stream, rows, chunk_prefix, n_rows,
                       partials);
    OG_LAUNCH_CHECK(name);
    return OG_OK;
}

OG_API int og_step_scale_f32(int n_chunks, const float *loss, float loss_limit, float max_norm, void *workspace, size_t workspace_bytes,
                             void *stream)
{
    const char *name = "og_step_scale_f32";
    float *state;
    double *partials;
    if (int rc = check_scale(name, n_chunks, loss, loss_limit, max_norm, workspace, workspace_bytes, state, partials)) return rc;
    hipLaunchKernelGGL(step_scale_kernel<false>, dim3(1), dim3(SCALE_THREADS), 0, (hipStream_t)stream, partials, n_chunks, loss,
                       loss_limit, max_norm, state, static_cast<float *>(nullptr), AmpArgs{});
    OG_LAUNCH_CHECK(name);
    return OG_OK;
}

OG_API int og_step_scale_amp_f32(int n_chunks, const float *loss, float loss_limit, float max_norm, void *scaler, int dynamic,
                                 float scale_factor, int scale_window, float min_scale, float max_scale, void *workspace,
                                 size_t workspace_bytes, void *stream)
{
    const char *name = "og_step_scale_amp_f32";
    float *state;
    double *partials;
    if (int rc = check_scale(name, n_chunks, loss, loss_limit, max_norm, workspace, workspace_bytes, state, partials)) return rc;
    OG_REQUIRE(scaler && ((uintptr_t)scaler & 15u) == 0, OG_EINVAL, "%s: null or misaligned scaler block", name);
    // written so that a NaN fails each of them
    OG_REQUIRE(scale_factor > 1.f && scale_factor <= 3.4028234664e38f, OG_EINVAL, "%s: scale_factor must be a finite number above 1 (got %g)",
               name, scale_factor);
    OG_REQUIRE(scale_window >= 1, OG_EINVAL, "%s: scale_window must be at least 1 (got %d)", name, scale_window);
    OG_REQUIRE(min_scale > 0.f, OG_EINVAL, "%s: min_scale must be positive (got %g)", name, min_scale);
    OG_REQUIRE(max_scale >= min_scale && max_scale <= 3.4028234664e38f, OG_EINVAL, "%s: max_scale must be finite and not below min_scale (got %g, %g)",
               name, max_scale, min_scale);
    const AmpArgs a{dynamic != 0, scale_factor, scale_window, min_scale, max_scale};
    hipLaunchKernelGGL(step_scale_kernel<true>, dim3(1), dim3(SCALE_THREADS), 0, (hipStream_t)stream, partials, n_chunks, loss,
                       loss_limit, max_norm, state, static_cast<float *>(scaler), a);
    OG_LAUNCH_CHECK(name);
    return OG_OK;
}

static int adam_step(const char *name, bool with_ema, const int64_t *rows, const int32_t *chunk_prefix, int n_rows, int chunk_first,
                     int n_chunks, const void *state, const AdamArgs &a, const int64_t *ema, float omd, void *stream)
{
    if (int rc = check_update(name, with_ema, rows, chunk_prefix, n_rows, chunk_first, n_chunks, state, ema, omd)) return rc;
    OG_REQUIRE(a.bc1 > 0.f && a.bc2 > 0.f, OG_EINVAL, "%s: bias corrections must be positive (bc1 %g, bc2 %g)", name, a.bc1, a.bc2);
    return launch_update(name, with_ema, rows, chunk_prefix, n_rows, chunk_first, n_chunks, state, AdamRule{a}, ema, omd, stream);
}

OG_API int og_adam_step_f32(const int64_t *rows, const int32_t *chunk_prefix, int n_rows, int chunk_first, int n_chunks,
                            const void *state, float lr, float b1, float b2, float omb1, float omb2, float eps, float wd, float bc1,
                            float bc2, int adam_w_mode, void *stream)
{
    const AdamArgs a{lr, b1, b2, omb1, omb2, eps, wd, bc1, bc2, adam_w_mode != 0};
    return adam_step("og_adam_step_f32", false, rows, chunk_prefix, n_rows, chunk_first, n_chunks, state, a, nullptr, 0.f, stream);
}

OG_API int og_adam_step_ema_f32(const int64_t *rows, const int32_t *chunk_prefix, int n_rows, int chunk_first, int n_chunks,
                                const void *state, float lr, float b1, float b2, float omb1, float omb2, float eps, float wd, float bc1,
                                float bc2, int adam_w_mode, const int64_t *ema, float omd, void *stream)
{
    const AdamArgs a{lr, b1, b2, omb1, omb2, eps, wd, bc1, bc2, adam_w_mode != 0};
    return adam_step("og_adam_step_ema_f32", true, rows, chunk_prefix, n_rows, chunk_first, n_chunks, state, a, ema, omd, stream);
}

// mom == 0: the rule without a buffer
static int sgd_step(const char *name, bool with_ema, const int64_t *rows, const int32_t *chunk_prefix, int n_rows, int chunk_first,
                    int n_chunks, const void *state, const SgdArgs &a, const int64_t *ema, float omd, void *stream)
{
    if (int rc = check_update(name, with_ema, rows, chunk_prefix, n_rows, chunk_first, n_chunks, state, ema, omd)) return rc;
    if (a.mom != 0.f)
        return launch_update(name, with_ema, rows, chunk_prefix, n_rows, chunk_first, n_chunks, state, SgdRule<true>{a}, ema, omd, stream);
    return launch_update(name, with_ema, rows, chunk_prefix, n_rows, chunk_first, n_chunks, state, SgdRule<false>{a}, ema, omd, stream);
}

OG_API int og_sgd_step_f32(const int64_t *rows, const int32_t *chunk_prefix, int n_rows, int chunk_first, int n_chunks, const void *state,
                           float lr, float mom, float wd, int first, void *stream)
{
    const SgdArgs a{lr, mom, wd, first != 0};
    return sgd_step("og_sgd_step_f32", false, rows, chunk_prefix, n_rows, chunk_first, n_chunks, state, a, nullptr, 0.f, stream);
}

OG_API int og_sgd_step_ema_f32(const int64_t *rows, const int32_t *chunk_prefix, int n_rows, int chunk_first, int n_chunks,
                               const void *state, float lr, float mom, float wd, int first, const int64_t *ema, float omd, void *stream)
{
    const SgdArgs a{lr, mom, wd, first != 0};
    return sgd_step("og_sgd_step_ema_f32", true, rows, chunk_prefix, n_rows, chunk_first, n_chunks, state, a, ema, omd, stream);
}

OG_API int og_ema_lerp_f32(const int64_t *rows, const int32_t *chunk_prefix, int n_rows, int n_chunks, float omd, void *stream)
{
    const char *name = "og_ema_lerp_f32";
    if (int rc = og_check_table(name, rows, chunk_prefix, n_rows, n_chunks)) return rc;
    OG_REQUIRE(omd >= 0.f && omd <= 1.f, OG_EINVAL, "%s: omd = 1 - decay must lie in [0, 1] (got %g)", name, omd);      // a NaN fails it
    if (n_chunks == 0) return OG_OK;
    hipLaunchKernelGGL(ema_lerp_kernel, dim3(n_chunks), dim3(OPTIM_THREADS), 0, (hipStream_t)stream, rows, chunk_prefix, n_rows, omd);
    OG_LAUNCH_CHECK(name);
    return OG_OK;
}
