// Halo-tiled 3x3 convolution ("tiled"): TWO independent 4-wave workgroups per CU instead of one 8-wave workgroup that owns
// the CU (the first halo kernel; DESIGN.md section 4, C1).  Included by conv3x3.hip (namespace-scope code first, then the C ABI).
//
// What the first kernel's measurements said: per work item 1.2 us set-up + 6-8.5 us wait for the
// first halo / weight tiles + 3.1 us epilogue around a 29-31 us main loop, with nothing else resident on the CU to use
// the matrix pipe meanwhile (160 KiB of LDS per workgroup); 16 ds_read_b128 per 32 MFMA with a 2-way bank conflict on the
// padded halo image (34 % of the LDS-active cycles); two barriers per 32-MFMA phase for the hand-made ping-pong of the two
// waves of a SIMD.  Here:
//   * a workgroup is 4 waves (one per SIMD) and needs <= 80 KiB of LDS and <= 256 VGPRs, so two workgroups share a CU:
//     one's prologue, epilogue, barrier and LDS latencies are the other's MFMA time, and the dispatcher interleaves the
//     workgroups of concurrent launches at half the granularity;
//   * K advances in 32-channel chunks (one v_mfma_f32_16x16x32 K step per (chunk, tap)): the halo image of a chunk is
//     (TW+2) x (TH+2) pixels x 80 B (64 B of channels + 16 B pad), double-buffered; the 128-cout x 32-channel weight tile
//     of a step is 8 KiB in a 3-deep ring; 2 x 28 + 3 x 8 = 80 KiB for 16 x 16 pixels;
//   * every wave owns 64 pixels x ALL 128 couts (WM = 4) or 128 pixels x 64 couts: 12 fragment reads per 32 MFMA instead
//     of 16, and the pixel fragments of step s+1 are read during the MFMAs of step s (they do not depend on the weight ring);
//   * pixel fragments are read as two ds_read_b64 per lane -- k = {4 fk .. 4 fk + 3} and {16 + 4 fk ..} -- which are
//     conflict-free on the 80-B pitch (5 slots of 16 B, odd: the 16 pixels of a fragment fall on 16 different slots, the
//     two fk of a 32-lane group on the two 8-B halves of a slot); ds_read_b128 cannot be made conflict-free on any
//     tap-invariant linear pitch (its lane groups mix fk and fk + 1 over interleaved pixel ranges);
//   * the weights are PRE-TILED once (og_conv3x3_pack_w16): [cout tile][chunk][tap] -> the 8 KiB LDS image itself, k order
//     matching the pixel fragments, 16-B slots XOR-swizzled for conflict-free ds_read_b128, so that a stage is filled by
//     8 contiguous 1-KiB LDS-DMA pieces (full cache lines, no per-row gather) and a step's tiles follow each other in
//     memory.
// One barrier per step: wait (counted vmcnt: everything but the youngest weight stage and, at most, one halo piece) |
// barrier | issue the DMA of weights(s+2) and one halo piece of the next chunk | read weights(s) and pixels(s+1) | 32 MFMA.

template <int N, int I = 0, class F>
__device__ __forceinline__ void og_static_for(F &&f)
{
    if constexpr (I < N) {
        f(std::integral_constant<int, I>());
        og_static_for<N, I + 1>(f);
    }
}

// ---- weight pre-tiling ---------------------------------------------------------------------------------------
// packed[((nt * chunks + q) * 9 + tap) * 8192 + r * 64 + (j ^ tiled_swz(r)) * 16 + e * 2]
//   = w[(nt * 128 + r)][tap][q * 32 + (e < 4 ? 4 * j + e : 16 + 4 * j + e - 4)],   r = 0..127, j = 0..3, e = 0..7
// slot swizzle by (row >> 2) & 3 -> {0, 3, 2, 1}: the four 16-lane groups of a ds_read_b128 ({fk 0: rows 0-3, 12-15; fk 1: rows
// 4-11}, ...) then fall on 16 different 16-B slots of the 256-B bank row
__host__ __device__ __forceinline__ constexpr int tiled_swz(int row) { return (4 - ((row >> 2) & 3)) & 3; }

__global__ void __launch_bounds__(256)
conv3x3_pack_kernel(const unsigned short *w, unsigned short *packed, int Cin, int Cout, int order)
{
    const long slot = (long)blockIdx.x * 256 + threadIdx.x;       // one 16-B slot of the packed image per thread
    const int taps = order >= 2 ? 1 : 9, rows = order == 3 ? 64 : 128;    // rows of a cout tile
    const long total = (long)Cout * taps * Cin / 8;
    if (slot >= total) return;
    const int chunks = Cin >> 5;
    const int in_stage = (int)(slot % (rows * 4));                // rows * 4 slots per stage (8 KiB for 128 rows)
    long stage = slot / (rows * 4);
    // order 0: 3x3, taps as they are (stride 1); order 1: 3x3 in the sequence the stride-2 kernel's phase groups consume;
    // order 2 / 3: 1x1 (Cout, Cin) in cout tiles of 128 / 64 rows, k in its natural order (the pointwise kernel loads its
    // pixel fragments as 16 contiguous bytes)
    const int kS2[9] = {0, 2, 6, 8, 3, 5, 1, 7, 4};
    const int tslot = (int)(stage % taps), tap = order == 1 ? kS2[tslot] : tslot;
    stage /= taps;
    const int q = (int)(stage % chunks), nt = (int)(stage / chunks);
    const int r = in_stage >> 2, jp = in_stage & 3, j = jp ^ tiled_swz(r);
    const unsigned short *src = w + ((size_t)(nt * rows + r) * taps + tap) * Cin + q * 32;
    u16x8 v;
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = src[order >= 2 ? 8 * j + e : (e < 4 ? 4 * j + e : 16 + 4 * j + (e - 4))];
    *reinterpret_cast<u16x8 *>(packed + slot * 8) = v;
}

// Pixel fragment of the tiled kernels: two ds_read_b64 per lane (k = 4 fk .. 4 fk + 3 and 16 + 4 fk ..), written as inline asm -- left
// to the compiler the pair becomes ONE ds_read2_b64 (two accesses 32 B apart), which runs at half the rate and banks modulo 32 dwords
// (MI355X_MICROARCH, LDS).  The compiler does not count these reads: their consumer is the MFMA block of the NEXT step, behind that
// step's lgkmcnt(0) (wait_vm_lgkm0) -- nothing else may touch the result in between (hence no register copies at a chunk seam).
template <int IMM>
__device__ __forceinline__ bf16x8 ds_read_b64_pair(uint32_t addr)
{
    typedef unsigned long long u64;
    typedef u64 u64x2 __attribute__((ext_vector_type(2)));
    u64 lo, hi;
    asm volatile("ds_read_b64 %0, %1 offset:%2" : "=v"(lo) : "v"(addr), "i"(IMM));
    asm volatile("ds_read_b64 %0, %1 offset:%2" : "=v"(hi) : "v"(addr), "i"(IMM + 32));
    u64x2 v;
    v[0] = lo;
    v[1] = hi;
    return __builtin_bit_cast(bf16x8, v);
}

// ---- tile shapes ------------------------------------------------------------------------------------------------
// The stride-1 kernel's forms, indexed by `kind` (tiled_kind: what og_conv3x3_tiled_supported returns): tile width and height in pixels,
// waves along the pixels (4 / wm along the couts), stages of the weight ring.
// ring: 3 stages where a step is 32 MFMA per wave (16 x 16 tiles: two steps cover the L2 latency); 6 at the 20-wide level, whose steps
// are 10 MFMA per wave = 70 ns: with two steps of look-ahead every step waited for most of an L2 round trip; 4 at the 40-wide level.
struct TiledShape {
    int tw, th, wm, ring;
};
constexpr TiledShape kTiledShapes[4] = {{0, 0, 0, 0}, {16, 16, 4, 3}, {40, 4, 2, 4}, {20, 4, 1, 6}};
constexpr int tiled_ring(int tw)
{
    for (const TiledShape &s : kTiledShapes)
        if (s.tw == tw) return s.ring;
    return 0;
}
// LDS of a workgroup: [weight ring | two halo images of a 32-channel chunk, 80 B per pixel, whole KiB | 1 KiB dump]
constexpr int tiled_halo_bytes(int tw, int th) { return ((tw + 2) * (th + 2) * 5 * 16 + 1023) / 1024 * 1024; }
constexpr int tiled_lds_bytes(int tw, int th) { return tiled_ring(tw) * 128 * 64 + 2 * tiled_halo_bytes(tw, th) + 1024; }
// the stride-2 kernel: the weight ring + a ring of three phase images of three 4-KiB pieces
constexpr int kS2LdsBytes = 3 * 128 * 64 + 3 * 3 * 4096;

// 1 = 16 x 16 (H, W multiples of 16), 2 = 40 x 4 (W == 40, H % 4 == 0), 3 = 20 x 4 (W == 20, H % 4 == 0), 0 = none
static int tiled_kind(int H, int W, int Cin, int Cout)
{
    if (Cout % 128 || Cin % 64) return 0;
    if (H % 16 == 0 && W % 16 == 0) return 1;
    for (int k = 2; k <= 3; ++k)      // one tile across
        if (W == kTiledShapes[k].tw && H % kTiledShapes[k].th == 0) return k;
    return 0;
}
static long tiled_items(int kind, int N, int H, int W, int Cout)
{
    return (long)N * (H / kTiledShapes[kind].th) * (W / kTiledShapes[kind].tw) * (Cout / 128);
}

// K slices for a level with few output tiles (< 200 workgroups against the chip's 512 slots), from the measurements of
// profiles/r03_ksplit.log (batch 8, us per layer, 1 / 2 / 3 slices):
//   40x40 384->256 (160 tiles of 40x4):  37.8 / 37.6 / 33.4    -> 3 slices where the chunks divide by 6
//   40x40 256->256 (160 tiles, 8 chunks): 27.4 / 30.5 / --      -> no split (320 workgroups do not pay for 80 KiB slabs)
//   40x40 384->384 (240 tiles):           43.5 / 43.9 / 51.7    -> no split: that level moves 7.8 KB of LDS-DMA per MFLOP
//                                                                  and sits at the ~7 TB/s the L2 -> LDS path delivers either way
//   20x20 384->384 (120 tiles of 20x4):   25.0 / 20.0 / 20.4    -> 2 slices (the split-K GEMM kernel: 21.6)
// A slice always has an even number of chunks.
static int tiled_ksplit(int kind, long items, int Cin)
{
    const int chunks = Cin / 32;
    if (items >= 200) return 1;
    if (kind == 3) return chunks % 4 == 0 ? 2 : 1;
    if (kind == 2) return chunks % 6 == 0 ? 3 : 1;
    return 1;
}
// The K split in the terms of ws_layout: the work items are the tiles, a slab holds a tile's tw * th pixels x 128 couts in fp32
// (a split has fewer than 200 items: far below kMaxTiles).
static Plan tiled_plan(int kind, int N, int H, int W, int Cin, int Cout)
{
    const long items = tiled_items(kind, N, H, W, Cout);
    Plan p = {};
    p.ksplit = tiled_ksplit(kind, items, Cin);
    p.bm = kTiledShapes[kind].tw * kTiledShapes[kind].th;
    p.bn = 128;
    p.m_tiles = p.ksplit > 1 ? (int)items : 0;
    p.n_tiles = 1;
    return p;
}

// Every wave of the four (one per SIMD) owns 64 x 128 or 128 x 64 outputs in <= 256 registers.  The schedule of a step is fixed per tile
// width (kWfRot below); the tuning variants that lost their A/Bs -- no s_setprio, DMA issue in front of the fragment reads, no XCD-aware
// order, weight fragments read in the step that uses them, 8-wave workgroups, the timing-only ablations, a chained launch of dependent
// layers (tools/experiments/conv3x3_tiled_chain.patch) -- are described in EXPERIMENTS.md and DESIGN.md section 4.
template <int TW, int TH, int WM>
__device__ __forceinline__ void conv3x3_tiled_body(const ConvArgs &a, const int bid, const int nblk)
{
    constexpr int BN = 128, WN = 4 / WM, kThr = 256, kPieceB = kThr * 16;
    constexpr int kHaloW = TW + 2, kHaloPx = (TW + 2) * (TH + 2), kPitch = 80;
    constexpr int NPA = (kHaloPx * 5 + kThr - 1) / kThr;     // halo DMA pieces per thread and chunk (5 slots per pixel)
    // halo buffer: the pieces' 1-KiB wave blocks up to the one that holds the last slot; the blocks of the last piece that
    // lie beyond it go to a shared 1-KiB dump region (zeros from out-of-range lanes)
    constexpr int kABytes = tiled_halo_bytes(TW, TH), kBBytes = BN * 64;
    // weight ring (tiled_ring): the weight FRAGMENTS of step s + 1 are read during the MFMAs of step s, like the pixel fragments (a step of
    // 10 MFMA per wave does not cover the LDS latency of its own fragment reads); the stage of step s is then free behind the barrier of
    // step s, and a stage is issued kAhead = kRing steps before its use
    constexpr int kRing = tiled_ring(TW);
    // kWfRot (16 x 16 tiles): NT + 1 fragment register sets used in rotation instead of 2 NT (250 of 256 VGPRs are taken) -- fragment n of
    // step s + 1 goes where fragment n - 1 of step s was, right behind the last MFMA that read it, fragment 0 into the spare set
    constexpr bool kWfRot = TW == 16;
    constexpr int kAhead = kRing;
    constexpr int kWin = kRing - 2;      // steps whose DMA may still be in flight behind a step's wait
    // the ring slot of step (chunk q, tap): 9 q + tap mod kRing is a compile-time function of (q & 1, tap) for 3 and 6 stages; with 4
    // stages it is that function XOR 2 in every other chunk PAIR (18 = 2 mod 4): the two halves of the ring swap per pair (ring_off below)
    static_assert(kRing == 3 || kRing == 4 || kRing == 6, "ring sizes the slot arithmetic serves");
    constexpr int kDump = kRing * kBBytes + 2 * kABytes;
    constexpr int PW = kBBytes / kPieceB;                    // weight pieces per thread per step
    constexpr int MT = TW * TH / 16 / WM, NT = 8 / WN;
    static_assert(TW * TH % (16 * WM) == 0 && 4 % WM == 0 && 8 % WN == 0 && PW >= 1, "unsupported tile");
    static_assert(NPA <= 8 - kWin, "the last halo piece must be older than everything tap 8's wait leaves in flight (the steps 8 - kWin .. 7)");
    static_assert(kDump + 1024 == tiled_lds_bytes(TW, TH) && kDump + 1024 <= 80 * 1024, "what the launcher asks for; two workgroups per CU");
    extern __shared__ __attribute__((aligned(1024))) unsigned char lds[];
    unsigned char *const bufB = lds, *const bufA = lds + kRing * kBBytes;   // [B0 B1 B2 | A0 A1]: all read offsets < 64 KiB

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const unsigned warm_v = og_warm_touch(a.warm, (unsigned)bid * kThr + (unsigned)tid);   // the next layer's weights: first in the queue
#ifdef OG_TILED_STAMPS
    {   // marks go to memory at once (the kernel has no scalar registers to spare): [workgroup][wave][16] u64
        unsigned long long rt_entry;
        asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(rt_entry));
        if (a.stamps) a.stamps[((size_t)blockIdx.x * 4 + wave) * 16 + 7] = rt_entry;
    }
#endif
    // XCD-aware order: the hardware deals workgroup ids round-robin over the 8 XCDs; consecutive WORK items (the cout
    // tiles of one pixel tile, then the neighbouring pixel tiles: shared halo, shared weights) go to one XCD's L2
    const int wid = (nblk & 7) == 0 ? og_xcd_remap(bid, nblk) : bid;
    // K split (a.ksplit > 1, levels whose tiles would not fill the chip): consecutive work ids are the K slices of one
    // output tile; slice `split` runs chunks [q0, q_end) and the slices meet in the last arriver (below)
    const int ksplit = a.ksplit, item = wid / ksplit, split = wid - item * ksplit;
    const int tiles_x = a.W / TW, tiles_y = a.H / TH, chunks = a.Cin >> 5;
    const int q0 = split * (chunks / ksplit), q_end = q0 + chunks / ksplit;      // both even (host-checked)
    const int nt_i = item % a.n_tiles;
    int t = item / a.n_tiles;
    const int tx = t % tiles_x;
    t /= tiles_x;
    const int ty = t % tiles_y, img = t / tiles_y;
    const int n0 = nt_i * BN;

    const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned short *>(a.x), 0, a.x_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t wr = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned short *>(a.w), 0, a.w_bytes, 0x00020000);
    // halo loader: slot p = tid + 256 i -> halo pixel p / 5, 16-B slot p % 5 (slot 4 = pad); out-of-image pixels, the pad and
    // slots past the halo read out of range = zeros
    uint32_t a_off[NPA];
#pragma unroll
    for (int i = 0; i < NPA; ++i) {
        const int p = tid + kThr * i, hp = p / 5, c = p - hp * 5;
        const int hy = hp / kHaloW, hx = hp - hy * kHaloW;
        const int gy = ty * TH - 1 + hy, gx = tx * TW - 1 + hx;
        const bool ok = c < 4 && hp < kHaloPx && gy >= 0 && gy < a.H && gx >= 0 && gx < a.W;
        a_off[i] = ok ? (uint32_t)((((img * a.H + gy) * a.W + gx) * a.Cin + c * 8) * 2) : kOobOffset;
    }
    const int piece = wave * 64 * 16;
    const uint32_t w_voff = (uint32_t)tid * 16;
    const uint32_t w_tile = (uint32_t)nt_i * (uint32_t)(chunks * 9 * kBBytes);
    auto issue_a = [&](int i, int q, int buf) {
        const int blk = i * kPieceB + piece;                  // this wave's 1-KiB block of piece i (wave-uniform)
        blds16(xr, a_off[i], q * 64, blk < kABytes ? bufA + buf * kABytes + blk : lds + kDump);
    };
    int ring_lo = 0, ring_hi = 2 * kBBytes;          // (4 stages) byte offsets of the ring's halves as the current chunk pair sees them
    auto ring_off = [&](int slot) { return kRing == 4 ? (slot < 2 ? ring_lo : ring_hi) + (slot & 1) * kBBytes : slot * kBBytes; };
    auto issue_b = [&](int step, int ring_bytes) {
#pragma unroll
        for (int i = 0; i < PW; ++i)
            blds16(wr, w_voff, w_tile + step * kBBytes + i * kPieceB, bufB + ring_bytes + piece + i * kPieceB);
    };

    // ---- fragment addresses
    const int wm = wave / WN, wn = wave % WN;
    const int fcol = lane & 15, fk = lane >> 4;
    const int w_rd = ((wn * NT) * 16 + fcol) * 64 + ((fk ^ tiled_swz(fcol)) << 4);   // + n * 1024 + ring * kBBytes
    int px_off[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        const int lp = (wm * MT + m) * 16 + fcol;
        px_off[m] = ((lp / TW) * kHaloW + lp % TW) * kPitch + fk * 8;
    }

    // pixel fragments (ds_read_b64_pair)
    const uint32_t lds_a = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) unsigned char *)bufA;
    uint32_t px_addr[TW == 16 ? 1 : MT];
#pragma unroll
    for (int m = 0; m < (TW == 16 ? 1 : MT); ++m) px_addr[m] = lds_a + px_off[m];
    auto read_px1 = [&](auto m_tag, auto off_tag, uint32_t buf_off, bf16x8 (&pf)[MT]) {
        constexpr int OFF = decltype(off_tag)::value, m = decltype(m_tag)::value;
        // TW == 16: the fragments of a wave are consecutive tile rows -> one address register, immediates for the rest
        constexpr int imm = OFF + (TW == 16 ? m * kHaloW * kPitch : 0);
        pf[m] = ds_read_b64_pair<imm>(px_addr[TW == 16 ? 0 : m] + buf_off);
    };
    auto read_px = [&](auto off_tag, uint32_t buf_off, bf16x8 (&pf)[MT]) {
        og_static_for<MT>([&](auto m_tag) { read_px1(m_tag, off_tag, buf_off, pf); });
    };

    // ---- residual operand = initial accumulators (its loads are the oldest vector-memory operations of the wave)
    f32x4 acc[NT][MT];
    if (a.skip && split == 0) {
        // 16 bytes per lane and load instead of 8: the lanes of an even fragment row (fk) fetch the 8 channels that they and their odd
        // neighbour row hold of cout block 2 np, the odd rows those of block 2 np + 1 (64 contiguous bytes per pixel and instruction
        // instead of 32, half the requests); v_permlane16_swap then trades the halves that belong to the other row.  (The operand costs
        // a 160x160 layer 29 of its 217 us wherever it is loaded -- moved to the epilogue: the same 25-28 us, profiles/r05_skip_operand.log --:
        // 105 MB that no register or LDS space is left to fetch ahead.)
        static_assert(NT % 2 == 0, "cout blocks in pairs");
        u16x8 sk2[NT / 2][MT];
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            const int lp = (wm * MT + m) * 16 + fcol;
            const size_t opx = (size_t)(img * a.H + ty * TH + lp / TW) * a.W + tx * TW + lp % TW;
#pragma unroll
            for (int np = 0; np < NT / 2; ++np)
                // non-temporal: read once -- with the default policy these 105 MB per 160x160 layer pushed weights and halos out of L2 / the
                // memory-side cache (nothing alone, -1.0 % of the network step, three of three: profiles/r05_skip_operand.log)
                sk2[np][m] = __builtin_nontemporal_load(reinterpret_cast<const u16x8 *>(a.skip + opx * a.Cout + n0 + (wn * NT + 2 * np + (fk & 1)) * 16 + (fk >> 1) * 8));
        }
#pragma unroll
        for (int i = 0; i < NPA; ++i) issue_a(i, q0, 0);
#pragma unroll
        for (int i = 0; i < kAhead; ++i) issue_b(9 * q0 + i, (i % kRing) * kBBytes);
#pragma unroll
        for (int np = 0; np < NT / 2; ++np)
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                typedef uint32_t u32x4s __attribute__((ext_vector_type(4)));
                typedef uint32_t u32x2s __attribute__((ext_vector_type(2)));
                const u32x4s v = __builtin_bit_cast(u32x4s, sk2[np][m]);
                const auto r0 = __builtin_amdgcn_permlane16_swap(v[0], v[2], false, false);   // first' = block 2 np, second' = block 2 np + 1
                const auto r1 = __builtin_amdgcn_permlane16_swap(v[1], v[3], false, false);
                const u16x4 lo = __builtin_bit_cast(u16x4, (u32x2s){r0[0], r1[0]}), hi = __builtin_bit_cast(u16x4, (u32x2s){r0[1], r1[1]});
                acc[2 * np][m] = (f32x4){bf2f(lo[0]), bf2f(lo[1]), bf2f(lo[2]), bf2f(lo[3])};
                acc[2 * np + 1][m] = (f32x4){bf2f(hi[0]), bf2f(hi[1]), bf2f(hi[2]), bf2f(hi[3])};
            }
    } else {
#pragma unroll
        for (int i = 0; i < NPA; ++i) issue_a(i, q0, 0);
#pragma unroll
        for (int i = 0; i < kAhead; ++i) issue_b(9 * q0 + i, (i % kRing) * kBBytes);
#pragma unroll
        for (int n = 0; n < NT; ++n)
#pragma unroll
            for (int m = 0; m < MT; ++m) acc[n][m] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }

    constexpr int kSets = NT == 8 ? 9 : NT == 4 ? 6 : 3, kFree = kSets - NT;      // (18 NT) mod kSets == 0: the rotation closes over a chunk pair
    static_assert(!kWfRot || ((18 * NT) % kSets == 0 && kFree >= 1 && NT * (MT - 1) >= kFree + 1 + MT), "rotating fragment sets");
    bf16x8 pf[2][MT], wf[kWfRot ? 1 : 2][kWfRot ? kSets : NT];
#ifdef OG_TILED_STAMPS
    // diagnostic build (tools/c1_stamps.py): per wave, shader-clock sums of the three phases of a step -- counted wait | barrier |
    // fragment reads + DMA issue + MFMA block -- from s_memtime marks whose results are collected behind the NEXT step's
    // lgkmcnt(0) (no wait of its own; the mark behind the MFMA block is the issue of the last MFMA)
    unsigned long long st_end, st_w, st_b, st_prev;
    uint32_t sum_wait = 0, sum_bar = 0, sum_body = 0, n_st = 0;
    {
        unsigned long long mt0, rt0;
        asm volatile("s_memtime %0\n\ts_memrealtime %1\n\ts_waitcnt lgkmcnt(0)" : "=s"(mt0), "=s"(rt0));
        st_end = st_w = st_b = st_prev = mt0;
        if (a.stamps) {
            a.stamps[((size_t)blockIdx.x * 4 + wave) * 16 + 4] = mt0;
            a.stamps[((size_t)blockIdx.x * 4 + wave) * 16 + 5] = rt0;
        }
    }
#endif
    // pixel fragments of step 0: the halo of chunk 0 must have landed (everything but the weight stages behind the first) and be visible
    wait_vm_lgkm0<(kAhead - 1) * PW>();      // (weights(0) too: step 0's own wait asks for no less)
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
#ifdef OG_TILED_STAMPS
    {
        unsigned long long rt_first;
        asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(rt_first));
        if (a.stamps) a.stamps[((size_t)blockIdx.x * 4 + wave) * 16 + 9] = rt_first;
    }
#endif
    read_px(std::integral_constant<int, 0>(), 0u, pf[0]);
#pragma unroll
    for (int n = 0; n < NT; ++n) wf[0][n] = *reinterpret_cast<const bf16x8 *>(bufB + w_rd + n * 1024);

    // One chunk = 9 steps.  MORE: a chunk follows (its halo trickles in during taps 0..NPA-1, weights(s+2) always exist);
    // the last chunk stops issuing at its last two steps.  PAR: the fragment set of the chunk's first step (9 is odd, so
    // it alternates from chunk to chunk: the chunk loop runs over pairs).
    auto chunk_body = [&](auto more_tag, auto par_tag, int q) {
        constexpr bool MORE = decltype(more_tag)::value;
        constexpr int PAR = decltype(par_tag)::value;
        const uint32_t cur_off = (uint32_t)((q & 1) * kABytes), nxt_off = (uint32_t)(((q + 1) & 1) * kABytes);
        og_static_for<9>([&](auto tap_tag) {
            constexpr int tap = decltype(tap_tag)::value;
            constexpr int kSlot0 = kRing == 6 ? 3 * PAR : kRing == 4 ? PAR : 0;
            const int s = q * 9 + tap;
            // weights(s) were issued kAhead steps ago;
            // lgkmcnt(0): the pixel fragments of this step (read during the previous one) are in their registers
            // younger than the stage this step needs (weights(s + 1)) = what the steps s - kWin .. s - 1 issued: a
            // halo piece each where the step is one of the first NPA of a chunk that has a successor (the steps of the chunk BEFORE this one
            // that fall in the window are its last kWin: none of them issues a halo piece), a weight stage each where step + kAhead exists
            {
                constexpr int kYounger = [] {
                    int n = 0;
                    for (int j = 1; j <= kWin; ++j) {
                        const int t = tap - j;
                        if (t < 0) n += PW;
                        else n += ((MORE && t < NPA) ? 1 : 0) + ((MORE || t + kAhead < 9) ? PW : 0);
                    }
                    return n;
                }();
                wait_vm_lgkm0<kYounger>();
            }
#ifdef OG_TILED_STAMPS
            asm volatile("" : "+s"(st_end), "+s"(st_w), "+s"(st_b));
            sum_wait += (uint32_t)st_w - (uint32_t)st_prev;      // (first step: all marks equal -> zeros)
            sum_bar += (uint32_t)st_b - (uint32_t)st_w;
            sum_body += (uint32_t)st_end - (uint32_t)st_b;
            st_prev = st_end;
            ++n_st;
            asm volatile("s_memtime %0" : "=s"(st_w));
#endif
            __builtin_amdgcn_s_barrier();
#ifdef OG_TILED_STAMPS
            asm volatile("s_memtime %0" : "=s"(st_b));
#endif
            __builtin_amdgcn_sched_barrier(0);
            auto issue_dma = [&]() {
                if (MORE && tap < NPA) issue_a(tap, q + 1, (q + 1) & 1);
                // ring slot of step s = q * 9 + tap: (kSlot0 + tap) % kRing with kSlot0 = 9 q mod kRing = 0 (3 or 9 stages) or 3 (q & 1) (6; q & 1
                // = PAR: a slice starts at an even chunk)
                if (MORE || tap + kAhead < 9) issue_b(s + kAhead, ring_off((kSlot0 + tap + kAhead) % kRing));
            };
            const unsigned char *wB = bufB + ring_off((kSlot0 + tap + 1) % kRing);      // the NEXT step's stage
            if constexpr (kWfRot) {
                constexpr bool kNext = MORE || tap < 8;
                constexpr int t18 = PAR * 9 + tap, cur = (PAR + tap) & 1, nxt = cur ^ 1;
                __builtin_amdgcn_s_setprio(1);
                og_static_for<NT * MT>([&](auto i_tag) {
                    constexpr int i = decltype(i_tag)::value, n = i / MT, m = i % MT;
                    acc[n][m] = OG_LP_MFMA(wf[0][(t18 * NT + n) % kSets], pf[cur][m], acc[n][m]);
                    if constexpr (m == MT - 1) {                      // the set of fragment n is free now: next step's fragment n + kFree
                        constexpr int j = n + kFree;
                        if constexpr (j < NT && kNext)
                            wf[0][((t18 + 1) * NT + j) % kSets] = *reinterpret_cast<const bf16x8 *>(wB + w_rd + j * 1024);
                    } else {
                        constexpr int k = n * (MT - 1) + m;          // the other gaps, in order: fragments 0 .. kFree - 1 (spare sets), the DMA, pixels
                        if constexpr (k < kFree) {
                            if constexpr (kNext) wf[0][((t18 + 1) * NT + k) % kSets] = *reinterpret_cast<const bf16x8 *>(wB + w_rd + k * 1024);
                        } else if constexpr (k == kFree) {
                            issue_dma();
                        } else if constexpr (k - kFree - 1 < MT) {
                            constexpr int pm = k - kFree - 1;
                            if constexpr (tap < 8)
                                read_px1(std::integral_constant<int, pm>(), std::integral_constant<int, (((tap + 1) / 3) * kHaloW + (tap + 1) % 3) * kPitch>(),
                                         cur_off, pf[nxt]);
                            else if constexpr (MORE)
                                read_px1(std::integral_constant<int, pm>(), std::integral_constant<int, 0>(), nxt_off, pf[nxt]);
                        }
                    }
                    __builtin_amdgcn_sched_barrier(0);
                });
                __builtin_amdgcn_s_setprio(0);
            } else {
                // Every fragment this step reads is the NEXT step's: the reads and the DMA issue go BETWEEN this step's MFMAs (one item
                // behind each of the first 1 + MT + NT: an MFMA holds the vector issue for 8 of its 16 cycles), instead of in front of
                // them -- with one wave per SIMD (this level has fewer workgroups than the chip has CUs) nothing else hides their issue time
                static_assert(NT * MT >= 1 + MT + NT, "an MFMA gap per issue item");
                constexpr bool kNext = MORE || tap < 8;
                constexpr int cur = (PAR + tap) & 1, nxt = cur ^ 1;
                __builtin_amdgcn_s_setprio(1);
                og_static_for<NT * MT>([&](auto i_tag) {
                    constexpr int i = decltype(i_tag)::value, n = i / MT, m = i % MT;
                    acc[n][m] = OG_LP_MFMA(wf[cur][n], pf[cur][m], acc[n][m]);
                    if constexpr (i == 0) {
                        issue_dma();
                    } else if constexpr (i - 1 < MT) {
                        if constexpr (tap < 8)
                            read_px1(std::integral_constant<int, i - 1>(), std::integral_constant<int, (((tap + 1) / 3) * kHaloW + (tap + 1) % 3) * kPitch>(),
                                     cur_off, pf[nxt]);
                        else if constexpr (MORE)
                            read_px1(std::integral_constant<int, i - 1>(), std::integral_constant<int, 0>(), nxt_off, pf[nxt]);
                    } else if constexpr (i - 1 - MT < NT) {
                        if constexpr (kNext) wf[nxt][i - 1 - MT] = *reinterpret_cast<const bf16x8 *>(wB + w_rd + (i - 1 - MT) * 1024);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                });
                __builtin_amdgcn_s_setprio(0);
            }
#ifdef OG_TILED_STAMPS
            asm volatile("s_memtime %0" : "=s"(st_end));
#endif
        });
    };
    const std::true_type yes;
    const std::false_type no;
    const std::integral_constant<int, 0> even;
    const std::integral_constant<int, 1> odd;
    int q = q0;
#pragma unroll 1
    for (; q + 2 < q_end; q += 2) {           // an even number of chunks per slice
        chunk_body(yes, even, q);
        chunk_body(yes, odd, q + 1);
        if constexpr (kRing == 4) {
            const int t = ring_lo;
            ring_lo = ring_hi;
            ring_hi = t;
        }
    }
    chunk_body(yes, even, q);
    chunk_body(no, odd, q + 1);

#ifdef OG_TILED_STAMPS
    {
        unsigned long long mt1, rt1;
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_memtime %0\n\ts_memrealtime %1\n\ts_waitcnt lgkmcnt(0)" : "=s"(mt1), "=s"(rt1));
        asm volatile("" : "+s"(st_end), "+s"(st_w), "+s"(st_b));
        sum_wait += (uint32_t)st_w - (uint32_t)st_prev;
        sum_bar += (uint32_t)st_b - (uint32_t)st_w;
        sum_body += (uint32_t)st_end - (uint32_t)st_b;
        if (a.stamps && lane == 0) {
            unsigned long long *o = a.stamps + ((size_t)blockIdx.x * 4 + wave) * 16;
            o[0] = sum_wait; o[1] = sum_bar; o[2] = sum_body; o[3] = n_st; o[12] = mt1; o[6] = rt1;
            o[10] = __builtin_amdgcn_s_getreg((4) | (0 << 6) | (31 << 11));    // HW_REG_HW_ID
            o[11] = __builtin_amdgcn_s_getreg((20) | (0 << 6) | (31 << 11));   // HW_REG_XCC_ID
        }
    }
#endif
    // ---- K-split meeting point (as conv3x3_kernel): every slice publishes its fp32 tile as a lane-linear slab with
    // write-through (sc1) stores -> vmcnt(0) -> barrier -> relaxed agent-scope ticket; the slice that arrives last adds the
    // others' slabs (sc1 loads, one slab per round trip) and runs the epilogue.  Correct for any placement over XCDs.
    if (ksplit > 1) {
        constexpr int F = NT * MT;
        constexpr uint32_t kSlabBytes = F * kThr * 16;
        uint64_t slab_base = reinterpret_cast<uint64_t>(a.partial) + (uint64_t)item * ksplit * kSlabBytes;
        slab_base = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(slab_base >> 32)) << 32) |
                    (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)slab_base);
        const __amdgpu_buffer_rsrc_t slabs = __builtin_amdgcn_make_buffer_rsrc(
            reinterpret_cast<char *>(slab_base), 0, __builtin_amdgcn_readfirstlane((int)(ksplit * kSlabBytes)), 0x00020000);
        const uint32_t own_off = __builtin_amdgcn_readfirstlane(split * kSlabBytes);
#pragma unroll
        for (int n = 0; n < NT; ++n)
#pragma unroll
            for (int m = 0; m < MT; ++m)
                store_b128_sc1(slabs, (n * MT + m) * kThr * 16 + tid * 16, own_off, acc[n][m]);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        int *flag = reinterpret_cast<int *>(lds);
        if (tid == 0) {
            const int old = __hip_atomic_fetch_add(a.counters + item, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const int last = old == ksplit - 1;
            if (last) __hip_atomic_store(a.counters + item, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // for the next launch
            *flag = last;
        }
        __syncthreads();
        if (!*flag) return;
        // the sum runs over ALL slabs in slice order, the own one re-read like the others: the result does not depend on which
        // slice happened to arrive last (fp32 addition is not associative; 0.5 us for the extra slab)
#pragma unroll
        for (int n = 0; n < NT; ++n)
#pragma unroll
            for (int m = 0; m < MT; ++m) acc[n][m] = (f32x4){0.f, 0.f, 0.f, 0.f};
        for (int sp = 0; sp < ksplit; ++sp) {
            const uint32_t soff = __builtin_amdgcn_readfirstlane(sp * kSlabBytes);
            f32x4 part[F];
#pragma unroll
            for (int i = 0; i < F; ++i)
                part[i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(slabs, i * kThr * 16 + tid * 16, soff, 16));
#pragma unroll
            for (int n = 0; n < NT; ++n)
#pragma unroll
                for (int m = 0; m < MT; ++m) acc[n][m] += part[n * MT + m];
        }
    }

    // ---- epilogue: bias + ReLU + the one rounding in the accumulator layout, the 16-bit tile through LDS
    // ([tile pixel][128 couts], pitch 272 B) so that the global stores are 16 B per lane, 256 B contiguous per pixel
    constexpr int kOPitch = BN * 2 + 16, kTilePx = TW * TH, kPerPx = BN / 8;
    static_assert(kTilePx * kOPitch <= kDump + 1024, "output staging must fit the LDS of the main loop");
    f32x4 bias_r[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n) bias_r[n] = *reinterpret_cast<const f32x4 *>(a.bias + n0 + (wn * NT + n) * 16 + fk * 4);
    __syncthreads();   // every wave is done reading the last stage
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        const int px = (wm * MT + m) * 16 + fcol;
#pragma unroll
        for (int n = 0; n < NT; ++n) {
            const int cl = (wn * NT + n) * 16 + fk * 4;
            const f32x4 v = acc[n][m] + bias_r[n];
            u16x4 o;
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) o[jj] = f2bf(a.relu ? fmaxf(v[jj], 0.f) : v[jj]);
            *reinterpret_cast<u16x4 *>(lds + px * kOPitch + cl * 2) = o;
        }
    }
    __syncthreads();
    if (a.up) {
        // merge of the hourglass level above: up[2y + dy][2x + dx] += this tile's (y, x), four 16-B read-modify-writes per
        // 16-B piece of the tile (256 B contiguous per pixel); two pieces = eight loads in flight per thread
        const int W2 = 2 * a.W;
        const size_t up_tile = ((size_t)img * 2 * a.H + 2 * ty * TH) * W2 + 2 * tx * TW;
        constexpr int kPieces = kTilePx * kPerPx;
        static_assert(kPieces % kThr == 0, "whole rounds");
        for (int g0 = tid; g0 < kPieces; g0 += 2 * kThr) {
            u16x8 lo[2], hi[2][4];
            size_t off[2];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int g = min(g0 + u * kThr, kPieces - kThr + tid), px = g / kPerPx, cg = g % kPerPx;   // (an odd last round does its piece twice: u = 1 is skipped below)
                off[u] = (up_tile + (size_t)(2 * (px / TW)) * W2 + 2 * (px % TW)) * a.Cout + n0 + cg * 8;
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    hi[u][q] = *reinterpret_cast<const u16x8 *>(a.up + off[u] + ((size_t)(q >> 1) * W2 + (q & 1)) * a.Cout);
                lo[u] = *reinterpret_cast<const u16x8 *>(lds + px * kOPitch + cg * 16);
            }
#pragma unroll
            for (int u = 0; u < 2; ++u)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    if (u == 1 && g0 + kThr >= kPieces) continue;   // uniform
                    u16x8 o;
#pragma unroll
                    for (int j = 0; j < 8; ++j) o[j] = f2bf(bf2f(hi[u][q][j]) + bf2f(lo[u][j]));
                    *reinterpret_cast<u16x8 *>(a.up + off[u] + ((size_t)(q >> 1) * W2 + (q & 1)) * a.Cout) = o;
                }
        }
    } else {
        const size_t tile_px = (size_t)(img * a.H + ty * TH) * a.W + tx * TW;
        for (int g = tid; g < kTilePx * kPerPx; g += kThr) {
            const int px = g / kPerPx, cg = g % kPerPx;
            const size_t off = (tile_px + (size_t)(px / TW) * a.W + (px % TW)) * a.Cout + n0 + cg * 8;
            *reinterpret_cast<u16x8 *>(a.out + off) = *reinterpret_cast<const u16x8 *>(lds + px * kOPitch + cg * 16);
        }
    }
#ifdef OG_TILED_STAMPS
    if (a.stamps && lane == 0) {
        unsigned long long rt_end;
        asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(rt_end));
        a.stamps[((size_t)blockIdx.x * 4 + wave) * 16 + 8] = rt_end;      // stores issued (not yet acknowledged)
    }
#endif
    og_warm_sink(warm_v);
}

template <int TW, int TH, int WM>
__global__ void __launch_bounds__(256, 2)
conv3x3_tiled_kernel(ConvArgs a)
{
    conv3x3_tiled_body<TW, TH, WM>(a, blockIdx.x, gridDim.x);
}

// ---------------------------------------------------------------------------------------------------------------
// Stride-2 3x3 convolution (residual.conv1 of the down-sampling blocks, models/hourglass_104.py:54-57 with stride 2) on the
// same structure: 4-wave workgroups, two (or more) per CU, 32-channel K steps, pre-tiled weights, one barrier per step.
//
// Input pixel of output (y, x) and tap (dy, dx): (2y + dy, 2x + dx).  By the PARITY of its row and column an input pixel
// belongs to one of four phase images; inside a phase image a tap is a constant pixel shift, exactly as in the stride-1
// kernel, and 16 consecutive output pixels read 16 consecutive phase pixels (conflict-free ds_read_b64 on the 80-B pitch):
//   OO (odd row, odd col):  rows 2(y0-1+r)+1, r = 0..TH;  cols 2(x0-1+c)+1, c = 0..TW   taps (-1,-1) (-1,+1) (+1,-1) (+1,+1)
//   EO (even row, odd col): rows 2(y0+r),     r = 0..TH-1; cols as OO                    taps (0,-1) (0,+1)
//   OE (odd row, even col): rows as OO;       cols 2(x0+c), c = 0..TW-1                  taps (-1,0) (+1,0)
//   EE:                                                                                  tap  (0,0)
// A 32-channel chunk is therefore four GROUPS of 4 + 2 + 2 + 1 steps, each with its own small LDS image ((TH+1) x (TW+1)
// pixels at most: 12 KiB for 16 x 8 outputs) gathered straight from the NHWC input by the per-lane source addresses of the
// LDS-DMA (no phase-split copy of the activations exists).  The images live in a ring of three: group g+2's image is
// issued during group g (every piece has at least two steps to land, like the weight stages).  The weights are pre-tiled
// in the order the steps consume them (og_conv3x3_pack_w16, order 1): taps 0 2 6 8 | 3 5 | 1 7 | 4.
// Static schedule of the halo pieces per chunk step t = 0..8 (3 pieces per image and thread):
//   t 0 1 2: OE(q) one each | t 4: EE(q) two, t 5: one | t 6: OO(q+1) three | t 8: EO(q+1) three.
// TW == 16: a 16-pixel MFMA fragment is one output row of the tile (one address register per image width, the rest immediates);
// otherwise (40 x 2 tiles for the 40-wide level) fragments run on across rows and every fragment has its own address.
template <int TW, int TH, int WM>
__global__ void __launch_bounds__(256, 2)
conv3x3s2_tiled_kernel(ConvArgs a)
{
    constexpr int BN = 128, WN = 4 / WM;
    constexpr bool kRowFrag = TW == 16;
    constexpr int kPitch = 80, kImgPx = (TW + 1) * (TH + 1);
    constexpr int NPA = (kImgPx * 5 + 255) / 256;            // pieces per thread and phase image
    constexpr int kABytes = NPA * 256 * 16, kBBytes = BN * 64, kRing = 3;
    constexpr int PW = kBBytes / (256 * 16);
    constexpr int MT = TW * TH / 16 / WM, NT = 8 / WN;
    static_assert(TW * TH % (16 * WM) == 0 && 4 % WM == 0, "unsupported tile");
    static_assert(NPA == 3, "the static halo schedule below issues three pieces per phase image");
    static_assert(kRing * kBBytes + 3 * kABytes == kS2LdsBytes && kS2LdsBytes <= 80 * 1024, "what the launcher asks for; two workgroups per CU");
    extern __shared__ __attribute__((aligned(1024))) unsigned char lds[];
    unsigned char *const bufB = lds, *const bufA = lds + kRing * kBBytes;

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const unsigned warm_v = og_warm_touch(a.warm, blockIdx.x * 256u + (unsigned)tid);   // the next layer's weights: first in the queue (sunk at the end)
    const int nblk = gridDim.x;
    const int item = (nblk & 7) == 0 ? og_xcd_remap(blockIdx.x, nblk) : blockIdx.x;
    const int tiles_x = a.W / TW, tiles_y = a.H / TH, chunks = a.Cin >> 5;     // a.H, a.W: OUTPUT size; input = a.Hin x a.Win
    const int nt_i = item % a.n_tiles;
    int t_ = item / a.n_tiles;
    const int tx = t_ % tiles_x;
    t_ /= tiles_x;
    const int ty = t_ % tiles_y, img = t_ / tiles_y;
    const int n0 = nt_i * BN, y0 = ty * TH, x0 = tx * TW;

    const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned short *>(a.x), 0, a.x_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t wr = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned short *>(a.w), 0, a.w_bytes, 0x00020000);
    // phase p = 0 OO, 1 EO, 2 OE, 3 EE: image width (pixels) and per-lane source offsets of its three pieces
    uint32_t a_off[4][NPA];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int odd_r = (p == 0 || p == 2), odd_c = (p == 0 || p == 1);
        const int pw = TW + odd_c, phh = TH + odd_r;
#pragma unroll
        for (int i = 0; i < NPA; ++i) {
            const int sl = tid + 256 * i, hp = sl / 5, c = sl - hp * 5;
            const int ri = hp / pw, ci = hp - ri * pw;
            const int iy = 2 * (y0 + ri) - odd_r, ix = 2 * (x0 + ci) - odd_c;
            const bool ok = c < 4 && ri < phh && iy >= 0 && iy < a.Hin && ix >= 0 && ix < a.Win;
            a_off[p][i] = ok ? (uint32_t)((((img * a.Hin + iy) * a.Win + ix) * a.Cin + c * 8) * 2) : kOobOffset;
        }
    }
    const int piece = wave * 64 * 16;
    const uint32_t w_voff = (uint32_t)tid * 16;
    const uint32_t w_tile = (uint32_t)nt_i * (uint32_t)(chunks * 9 * kBBytes);
    auto issue_h = [&](int p, int i, int q, uint32_t buf_off) { blds16(xr, a_off[p][i], q * 64, bufA + buf_off + piece + i * 4096); };
    auto issue_b = [&](int step, int ring) {
#pragma unroll
        for (int i = 0; i < PW; ++i)
            blds16(wr, w_voff, w_tile + step * kBBytes + i * 4096, bufB + ring * kBBytes + piece + i * 4096);
    };

    const int wm = wave / WN, wn = wave % WN;
    const int fcol = lane & 15, fk = lane >> 4;
    const int w_rd = ((wn * NT) * 16 + fcol) * 64 + ((fk ^ tiled_swz(fcol)) << 4);
    const uint32_t lds_a = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) unsigned char *)bufA;
    // lane's pixel in a phase image of width PWID: tile pixel tp = (wm * MT + m) * 16 + fcol at (tp / TW + dr, tp % TW + dc)
    uint32_t pxE[kRowFrag ? 1 : MT], pxO[kRowFrag ? 1 : MT];      // images TW / TW + 1 pixels wide
#pragma unroll
    for (int m = 0; m < (kRowFrag ? 1 : MT); ++m) {
        const int tp = (wm * MT + m) * 16 + fcol, r = tp / TW, c = tp - r * TW;
        pxE[m] = lds_a + (uint32_t)((r * TW + c) * kPitch + fk * 8);
        pxO[m] = lds_a + (uint32_t)((r * (TW + 1) + c) * kPitch + fk * 8);
    }
    auto read_px1 = [&](auto m_tag, auto pw_tag, auto off_tag, uint32_t buf_off, bf16x8 (&pf)[MT]) {
        constexpr int PWID = decltype(pw_tag)::value, OFF = decltype(off_tag)::value, m = decltype(m_tag)::value;
        constexpr int imm = OFF + (kRowFrag ? m * PWID * kPitch : 0);
        pf[m] = ds_read_b64_pair<imm>((PWID == TW ? pxE[kRowFrag ? 0 : m] : pxO[kRowFrag ? 0 : m]) + buf_off);
    };
    auto read_px = [&](auto pw_tag, auto off_tag, uint32_t buf_off, bf16x8 (&pf)[MT]) {
        og_static_for<MT>([&](auto m_tag) { read_px1(m_tag, pw_tag, off_tag, buf_off, pf); });
    };

    f32x4 acc[NT][MT];
    if (a.skip) {
        u16x4 sk[NT][MT];
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            const int tp = (wm * MT + m) * 16 + fcol;
            const size_t opx = (size_t)(img * a.H + y0 + tp / TW) * a.W + x0 + tp % TW;
#pragma unroll
            for (int n = 0; n < NT; ++n)
                sk[n][m] = *reinterpret_cast<const u16x4 *>(a.skip + opx * a.Cout + n0 + (wn * NT + n) * 16 + fk * 4);
        }
#pragma unroll
        for (int n = 0; n < NT; ++n)
#pragma unroll
            for (int m = 0; m < MT; ++m)
                acc[n][m] = (f32x4){bf2f(sk[n][m][0]), bf2f(sk[n][m][1]), bf2f(sk[n][m][2]), bf2f(sk[n][m][3])};
    } else {
#pragma unroll
        for (int n = 0; n < NT; ++n)
#pragma unroll
            for (int m = 0; m < MT; ++m) acc[n][m] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
    // prologue: images of groups 0 (OO) and 1 (EO) of chunk 0 into ring slots 0 and 1, weights of steps 0 and 1
#pragma unroll
    for (int i = 0; i < NPA; ++i) issue_h(0, i, 0, 0);
#pragma unroll
    for (int i = 0; i < NPA; ++i) issue_h(1, i, 0, kABytes);
    issue_b(0, 0);
    issue_b(1, 1);

    bf16x8 pf[2][MT], wf[NT];
    wait_vm_lgkm0<PW>();
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    const std::integral_constant<int, TW> w16;
    const std::integral_constant<int, TW + 1> w17;
    read_px(w17, std::integral_constant<int, 0>(), 0u, pf[0]);

    // step t of a chunk: phase group, image width, (row, column) shift of the tap inside the image
    //   t:      0  1  2  3 | 4  5 | 6  7 | 8
    //   group:  OO OO OO OO| EO EO| OE OE| EE
    auto chunk_body = [&](auto more_tag, auto par_tag, int q) {
        constexpr bool MORE = decltype(more_tag)::value;
        constexpr int PAR = decltype(par_tag)::value;
        const int b0 = (4 * q) % 3;                                  // ring slot of this chunk's OO image
        uint32_t boff[6];                                            // ring slot (bytes) of group 4q + j, j = 0..5
#pragma unroll
        for (int j = 0; j < 6; ++j) boff[j] = (uint32_t)(((b0 + j) % 3) * kABytes);
        og_static_for<9>([&](auto t_tag) {
            constexpr int t = decltype(t_tag)::value;
            const int s = q * 9 + t;
            // outstanding at the top of step t: what step t-1 issued (its halo pieces + weights(s+1))
            constexpr int h_more[9] = {1, 1, 1, 0, 2, 1, 3, 0, 3}, h_last[9] = {1, 1, 1, 0, 2, 1, 0, 0, 0};
            constexpr int prev_h = t == 0 ? h_more[8] : (MORE ? h_more[t - 1] : h_last[t - 1]);
            constexpr int prev_b = (t == 0 || MORE || t - 1 < 7) ? PW : 0;
            wait_vm_lgkm0<prev_h + prev_b>();
            __builtin_amdgcn_s_barrier();
            __builtin_amdgcn_sched_barrier(0);
            auto issue_dma = [&]() {
                if constexpr (t < 3) issue_h(2, t, q, boff[2]);                                   // OE(q)
                if constexpr (t == 4) { issue_h(3, 0, q, boff[3]); issue_h(3, 1, q, boff[3]); }   // EE(q)
                if constexpr (t == 5) issue_h(3, 2, q, boff[3]);
                if constexpr (MORE && t == 6) { issue_h(0, 0, q + 1, boff[4]); issue_h(0, 1, q + 1, boff[4]); issue_h(0, 2, q + 1, boff[4]); }
                if constexpr (MORE && t == 8) { issue_h(1, 0, q + 1, boff[5]); issue_h(1, 1, q + 1, boff[5]); issue_h(1, 2, q + 1, boff[5]); }
                if (MORE || t < 7) issue_b(s + 2, (t + 2) % kRing);
            };
            // pixel fragment m of step t + 1 (shift of its tap inside its phase image)
            constexpr int kP = kPitch;
            auto px_next = [&](auto m_tag) {
                bf16x8(&nx)[MT] = pf[(PAR + t + 1) & 1];
                if constexpr (t == 0) read_px1(m_tag, w17, std::integral_constant<int, 1 * kP>(), boff[0], nx);                 // OO (0,1)
                if constexpr (t == 1) read_px1(m_tag, w17, std::integral_constant<int, (TW + 1) * kP>(), boff[0], nx);          // OO (1,0)
                if constexpr (t == 2) read_px1(m_tag, w17, std::integral_constant<int, (TW + 2) * kP>(), boff[0], nx);          // OO (1,1)
                if constexpr (t == 3) read_px1(m_tag, w17, std::integral_constant<int, 0>(), boff[1], nx);                      // EO (0,0)
                if constexpr (t == 4) read_px1(m_tag, w17, std::integral_constant<int, 1 * kP>(), boff[1], nx);                 // EO (0,1)
                if constexpr (t == 5) read_px1(m_tag, w16, std::integral_constant<int, 0>(), boff[2], nx);                      // OE (0,0)
                if constexpr (t == 6) read_px1(m_tag, w16, std::integral_constant<int, TW * kP>(), boff[2], nx);                // OE (1,0)
                if constexpr (t == 7) read_px1(m_tag, w16, std::integral_constant<int, 0>(), boff[3], nx);                      // EE
                if constexpr (t == 8 && MORE) read_px1(m_tag, w17, std::integral_constant<int, 0>(), boff[4], nx);              // OO(q+1) (0,0)
            };
            const unsigned char *wB = bufB + (t % kRing) * kBBytes;
            // (the stride-1 kernel's interleaved issue -- DMA and fragment reads between the MFMAs -- was tried here too: -1 % alone, +0.35 %
            // in the network over five repeats, profiles/r05_c1_interleave_ab.log: not kept)
            og_static_for<MT>([&](auto m_tag) { px_next(m_tag); });
#pragma unroll
            for (int n = 0; n < NT; ++n) wf[n] = *reinterpret_cast<const bf16x8 *>(wB + w_rd + n * 1024);
            issue_dma();       // behind the fragment reads: measured 1-4 % faster than in front of them
            __builtin_amdgcn_s_setprio(1);
#pragma unroll
            for (int n = 0; n < NT; ++n)
#pragma unroll
                for (int m = 0; m < MT; ++m) acc[n][m] = OG_LP_MFMA(wf[n], pf[(PAR + t) & 1][m], acc[n][m]);
            __builtin_amdgcn_s_setprio(0);
        });
    };
    const std::true_type yes;
    const std::false_type no;
    const std::integral_constant<int, 0> even;
    const std::integral_constant<int, 1> odd;
    int q = 0;
#pragma unroll 1
    for (; q + 2 < chunks; q += 2) {
        chunk_body(yes, even, q);
        chunk_body(yes, odd, q + 1);
    }
    chunk_body(yes, even, q);
    chunk_body(no, odd, q + 1);

    // ---- epilogue (as the stride-1 kernel)
    constexpr int kOPitch = BN * 2 + 16, kTilePx = TW * TH, kPerPx = BN / 8;
    static_assert(kTilePx * kOPitch <= kRing * kBBytes + 3 * kABytes, "output staging must fit the LDS of the main loop");
    f32x4 bias_r[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n) bias_r[n] = *reinterpret_cast<const f32x4 *>(a.bias + n0 + (wn * NT + n) * 16 + fk * 4);
    __syncthreads();
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        const int px = (wm * MT + m) * 16 + fcol;
#pragma unroll
        for (int n = 0; n < NT; ++n) {
            const int cl = (wn * NT + n) * 16 + fk * 4;
            const f32x4 v = acc[n][m] + bias_r[n];
            u16x4 o;
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) o[jj] = f2bf(a.relu ? fmaxf(v[jj], 0.f) : v[jj]);
            *reinterpret_cast<u16x4 *>(lds + px * kOPitch + cl * 2) = o;
        }
    }
    __syncthreads();
    const size_t tile_px = (size_t)(img * a.H + y0) * a.W + x0;
    for (int g = tid; g < kTilePx * kPerPx; g += 256) {
        const int px = g / kPerPx, cg = g % kPerPx;
        const size_t off = (tile_px + (size_t)(px / TW) * a.W + (px % TW)) * a.Cout + n0 + cg * 8;
        *reinterpret_cast<u16x8 *>(a.out + off) = *reinterpret_cast<const u16x8 *>(lds + px * kOPitch + cg * 16);
    }
    og_warm_sink(warm_v);
}

// ---------------------------------------------------------------------------------------------------------------
// Pointwise (1x1) convolutions of the large levels on the same building blocks: the inters_ / cnvs_ junction
// relu(W1 x1 + W2 x2 + b) (models/hourglass_104.py:239-250, :291-292) as ONE launch over the concatenated K, the 1x1 (stride 1
// or 2) projection `skip` of the large residuals (:63-67), and all heads of the decoded stack (models/heads.py:48-70,
// :116-142) with fp32 NCHW outputs -- the layout the decoder kernels stream -- written straight from the accumulators.
//
// A workgroup is 4 waves x (64 pixels x BN couts); nothing of the pixel operand is shared between waves, so it never
// touches LDS: every lane loads its MFMA B fragments (16 B = 8 channels of its pixel) from global memory one K step
// (64 channels) AHEAD into a second register set, by inline-asm buffer loads that the compiler does not count (their
// consumer sits behind the next step's counted vmcnt).  Only the weights, which all four waves share, go through the
// 3-deep LDS-DMA ring (two 32-channel images of the tiled format per 64-channel step; og_conv3x3_pack_w16 order 2 =
// one tap, natural k order).  Out-of-range pixels of the last tile read zeros through the buffer descriptor.
struct PwArgs {
    const unsigned short *x1, *x2;   // (N,H1,W1,C1), (N,H2,W2,C2) or null; output pixel (y, x) reads (y * s, x * s)
    const unsigned short *w;         // packed [Cout / BN][(C1 + C2) / 32][BN rows x 64 B]
    const float *bias;               // fp32[Cout] or null
    const unsigned short *skip;      // (N,H,W,Cout) 16-bit residual or null (mode 0)
    unsigned short *out;             // mode 0: (N,H,W,Cout) 16-bit
    float *outf[4];                  // mode 1: up to four dense (N,cnt,H,W) fp32 tensors, channels [first[i], first[i+1])
    int first[5];
    int N, H, W, Cout, M;            // output size
    int C1, H1, W1, s1, C2, H2, W2, s2;
    int x1_bytes, x2_bytes, w_bytes, n_tiles, relu;
    int items;                       // work items (pixel tiles x cout tiles); a launch of fewer workgroups walks them (persistent form)
    unsigned long long *stamps;      // diagnostic build (-DOG_PW_STAMPS): [workgroup][wave][8] s_memrealtime marks, or null
};

template <int BN, int MODE, int D = 1>
__global__ void __launch_bounds__(256, 2)
conv1x1_tiled_kernel(PwArgs a)
{
    constexpr int MT = 4, NT = BN / 16, kHalf = BN * 64, kStage = 2 * kHalf, kRing = 3;
    constexpr int PW = kStage / 4096;        // weight pieces per thread and step
    static_assert(PW >= 1 && kRing * kStage <= 64 * 1024, "LDS");
    extern __shared__ __attribute__((aligned(1024))) unsigned char lds[];

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
#ifdef OG_PW_STAMPS
#define PW_STAMP(i)                                                                                            \
    do {                                                                                                       \
        unsigned long long t_;                                                                                 \
        asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_));                                   \
        if (a.stamps) a.stamps[((size_t)stamp_id * 4 + wave) * 8 + (i)] = t_;                                   \
    } while (0)
#else
#define PW_STAMP(i)
#endif
    int stamp_id = blockIdx.x;
    (void)stamp_id;
    // Persistent form: the launch has at most two workgroups per CU; workgroup b walks the work items b, b + gridDim.x, ... (a new
    // workgroup costs 3-9 us from its entry to its first loads -- wave launch, kernel arguments, address set-up beside a resident
    // workgroup's K loop: profiles/r04_pw_stamps.log -- against a 7.6 us K loop).  XCD-aware order over the VIRTUAL ids: gridDim.x and the
    // item count are multiples of 8 where the remap applies, so a workgroup stays on its XCD's contiguous range of items, and of
    // 8 n_tiles, so it keeps its cout tile (the weights stay the same L2 lines).
    const int fcol = lane & 15, fk = lane >> 4;
    for (int vid = blockIdx.x; vid < a.items; vid += gridDim.x) {
    const int item = (a.items & 7) == 0 && (gridDim.x & 7) == 0 ? og_xcd_remap(vid, a.items) : vid;
    const int nt_i = item % a.n_tiles, m0 = (item / a.n_tiles) * 256, n0 = nt_i * BN;
    if (vid != (int)blockIdx.x) __syncthreads();      // the previous item's output staging has been read: the ring may be refilled
    stamp_id = vid;
    PW_STAMP(0);
    const int steps1 = a.C1 >> 6, steps = steps1 + (a.C2 >> 6);

    typedef int rsrc_t __attribute__((ext_vector_type(4)));
    // raw buffer descriptors as plain SGPR quads for the inline-asm loads: base, base_hi (stride 0), bytes, flags
    auto mk_rsrc = [](const void *p, int bytes) {
        const uint64_t b = reinterpret_cast<uint64_t>(p);
        rsrc_t r;
        r[0] = (int)(uint32_t)b;
        r[1] = (int)((uint32_t)(b >> 32) & 0xffffu);
        r[2] = bytes;
        r[3] = 0x00020000;
        return r;
    };
    const rsrc_t x1r = mk_rsrc(a.x1, a.x1_bytes), x2r = mk_rsrc(a.x2 ? a.x2 : a.x1, a.x2 ? a.x2_bytes : 0);
    const __amdgpu_buffer_rsrc_t wr = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned short *>(a.w), 0, a.w_bytes, 0x00020000);
    // byte offset of this lane's pixel (fragment m) in x1 / x2, + fk * 16; pixels past M read out of range
    // (a second input has the geometry of the first -- host-checked -- so one set of offsets serves both)
    uint32_t p1[MT];
    if (a.s1 == 1 && a.H1 == a.H && a.W1 == a.W) {
        // input and output pixels coincide (junction, heads, same-size projections): no (n, y, x) to recover -- the two divisions per
        // fragment row cost a work item 2-3 us of address set-up beside a resident workgroup's K loop (round 6 stamps)
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            const int p = m0 + wave * 64 + m * 16 + fcol;
            p1[m] = p < a.M ? (uint32_t)p * (uint32_t)(a.C1 * 2) + (uint32_t)(fk * 16) : kOobOffset;
        }
    } else {
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            const int p = m0 + wave * 64 + m * 16 + fcol;
            const int t = p / a.W, x = p - t * a.W, n = t / a.H, y = t - n * a.H;
            p1[m] = p < a.M ? (uint32_t)((((n * a.H1 + y * a.s1) * a.W1 + x * a.s1) * a.C1) * 2 + fk * 16) : kOobOffset;
        }
    }
    typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
    // pixel fragments of half h (channels 32 h .. 32 h + 31) of K step s into pf[m]; a step past the end reads out of range
    // (zeros, no memory traffic): the loop issues the same loads in every step and its counted waits are constants
    auto load_px = [&](int s, auto half_tag, bf16x8 (&pf)[MT]) {
        constexpr int HALF = decltype(half_tag)::value;
        const bool second = s >= steps1;
        const uint32_t soff = (uint32_t)((second ? s - steps1 : s) * 128);
        const uint32_t beyond = s >= steps ? kOobOffset : 0u;
        const rsrc_t r = second ? x2r : x1r;
        og_static_for<MT>([&](auto m_tag) {
            constexpr int m = decltype(m_tag)::value;
            u32x4 v;
            asm volatile("buffer_load_dwordx4 %0, %1, %2, %3 offen offset:%4" : "=v"(v) : "v"(p1[m] | beyond), "s"(r), "s"(soff), "i"(HALF * 64));
            pf[m] = __builtin_bit_cast(bf16x8, v);
        });
    };
    const int piece = wave * 64 * 16;
    const uint32_t w_voff = (uint32_t)tid * 16;
    const uint32_t w_tile = (uint32_t)nt_i * (uint32_t)((a.C1 + a.C2) / 32 * kHalf);
    auto issue_b = [&](int s, int ring) {
        const uint32_t voff = w_voff | (s >= steps ? kOobOffset : 0u);
#pragma unroll
        for (int i = 0; i < PW; ++i)
            blds16(wr, voff, w_tile + s * kStage + i * 4096, lds + ring * kStage + piece + i * 4096);
    };
    const int w_rd = fcol * 64 + ((fk ^ tiled_swz(fcol)) << 4);       // + n * 1024 + half * kHalf + ring * kStage

    f32x4 acc[NT][MT];
#pragma unroll
    for (int n = 0; n < NT; ++n)
#pragma unroll
        for (int m = 0; m < MT; ++m) acc[n][m] = (f32x4){0.f, 0.f, 0.f, 0.f};
    bf16x8 pfL[D][MT], pfH[D][MT], wf[4];
    // D register sets per half, used in turn: the loads of step s + D are issued right behind the MFMAs that consumed step s's
    // values.  D = 1 (an odd number of steps): a load has half a step (32 MFMAs, ~0.25 us) to land, so every step waits out most of
    // a memory round trip; D = 2: a step and a half -- twice the bytes in flight per wave (the 160x160 layers are HBM-bound:
    // 2.5 TB/s with one set).  Issue sequence, the same in the prologue and in every step (steps past the end read zeros):
    //   B(0) lo(0) hi(0) [B(1) lo(1) hi(1)] | step s: B(s + D) .. lo(s + D) .. hi(s + D)
    //   top of step s:  B(s), lo(s) landed  <=> outstanding at most hi(s) + the D - 1 steps issued after it
    //   before half 1:  hi(s) landed        <=> at most those + B(s + D) + lo(s + D)
    // (the weight ring is 3 deep: slot (s + D) % 3 was last read in step s + D - 3 < s)
    const std::integral_constant<int, 0> h0;
    const std::integral_constant<int, 1> h1;
    issue_b(0, 0);
    load_px(0, h0, pfL[0]);
    load_px(0, h1, pfH[0]);
    if constexpr (D == 2) {
        issue_b(1, 1);
        load_px(1, h0, pfL[1]);
        load_px(1, h1, pfH[1]);
    }
    PW_STAMP(1);
    auto step_body = [&](auto set_tag, int s) {
        constexpr int SET = decltype(set_tag)::value;
        wait_vm_lgkm0<MT + (D - 1) * (PW + 2 * MT)>();
        if (s == 0) PW_STAMP(2);
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
        issue_b(s + D, (s + D) % kRing);
        const unsigned char *wB = lds + (s % kRing) * kStage;
        // weight fragments four at a time: the register budget has no room for eight
#pragma unroll
        for (int nb = 0; nb < NT; nb += 4) {
#pragma unroll
            for (int n = 0; n < 4; ++n) wf[n] = *reinterpret_cast<const bf16x8 *>(wB + w_rd + (nb + n) * 1024);
#pragma unroll
            for (int n = 0; n < 4; ++n)
#pragma unroll
                for (int m = 0; m < MT; ++m) acc[nb + n][m] = OG_LP_MFMA(wf[n], pfL[SET][m], acc[nb + n][m]);
        }
        __builtin_amdgcn_sched_barrier(0);
        load_px(s + D, h0, pfL[SET]);
        wait_vm_lgkm0<(D - 1) * (PW + 2 * MT) + PW + MT>();
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int nb = 0; nb < NT; nb += 4) {
#pragma unroll
            for (int n = 0; n < 4; ++n) wf[n] = *reinterpret_cast<const bf16x8 *>(wB + kHalf + w_rd + (nb + n) * 1024);
#pragma unroll
            for (int n = 0; n < 4; ++n)
#pragma unroll
                for (int m = 0; m < MT; ++m) acc[nb + n][m] = OG_LP_MFMA(wf[n], pfH[SET][m], acc[nb + n][m]);
        }
        __builtin_amdgcn_sched_barrier(0);
        load_px(s + D, h1, pfH[SET]);
    };
#pragma unroll 1
    for (int s = 0; s < steps; s += D) {
        step_body(h0, s);
        if constexpr (D == 2) step_body(h1, s + 1);
    }
    PW_STAMP(3);
    wait_vm_lgkm0<0>();     // the zero loads of the steps past the end: their registers are free only now
    PW_STAMP(4);

    // ---- epilogue.  lane = pixel fcol of fragment m, couts n * 16 + 4 fk .. + 3 in acc[n][m]
    f32x4 bias_r[NT];      // once, in ONE round trip (inside the m loop below they cost one per pixel row block)
#pragma unroll
    for (int n = 0; n < NT; ++n)
        bias_r[n] = a.bias ? *reinterpret_cast<const f32x4 *>(a.bias + n0 + n * 16 + fk * 4) : (f32x4){0.f, 0.f, 0.f, 0.f};
    if constexpr (MODE == 0) {
        // 16-bit output: the tile goes through LDS ([tile pixel][BN couts], pitch 2 BN + 16 B) so that the global stores are 16 B
        // per lane and 2 BN contiguous bytes per pixel -- straight from the accumulators they are 8 B per lane, 32-B runs, four
        // times the write requests (the 160x160 layers are bound by memory requests: 85 -> 66 us without their stores)
        constexpr int kOPitch = BN * 2 + 16, kPerPx = BN / 8;
        __syncthreads();   // every wave is done reading the weight ring
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            __builtin_amdgcn_sched_barrier(0);   // one pixel row block at a time: hoisting all residual loads would spill
            const int px = wave * 64 + m * 16 + fcol, p = m0 + px;
#pragma unroll
            for (int n = 0; n < NT; ++n) {
                f32x4 v = acc[n][m] + bias_r[n];
                if (a.skip && p < a.M) {
                    const u16x4 sk = *reinterpret_cast<const u16x4 *>(a.skip + (size_t)p * a.Cout + n0 + n * 16 + fk * 4);
#pragma unroll
                    for (int j = 0; j < 4; ++j) v[j] += bf2f(sk[j]);
                }
                u16x4 o;
#pragma unroll
                for (int j = 0; j < 4; ++j) o[j] = f2bf(a.relu ? fmaxf(v[j], 0.f) : v[j]);
                *reinterpret_cast<u16x4 *>(lds + px * kOPitch + (n * 16 + fk * 4) * 2) = o;
            }
        }
        __syncthreads();
#pragma unroll 4
        for (int g = tid; g < 256 * kPerPx; g += 256) {
            const int px = g / kPerPx, cg = g % kPerPx, p = m0 + px;
            if (p < a.M)
                *reinterpret_cast<u16x8 *>(a.out + (size_t)p * a.Cout + n0 + cg * 8) = *reinterpret_cast<const u16x8 *>(lds + px * kOPitch + cg * 16);
        }
    } else {
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            __builtin_amdgcn_sched_barrier(0);
            const int p = m0 + wave * 64 + m * 16 + fcol;
            if (p >= a.M) continue;
            const int hw = a.H * a.W, img = p / hw, pix = p - img * hw;
#pragma unroll
            for (int n = 0; n < NT; ++n) {
                const int co = n0 + n * 16 + fk * 4;
                const f32x4 v = acc[n][m] + bias_r[n];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int c = co + j;
#pragma unroll
                    for (int hd = 0; hd < 4; ++hd)
                        if (c >= a.first[hd] && c < a.first[hd + 1])
                            a.outf[hd][((size_t)img * (a.first[hd + 1] - a.first[hd]) + (c - a.first[hd])) * hw + pix] = v[j];
                }
            }
        }
    }
    PW_STAMP(5);
    }      // work items
#undef PW_STAMP
}
