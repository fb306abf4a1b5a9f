// The model's FIRST Conv block (reference yolov8.yaml:738 `Conv [64, 3, 2]` through nn/modules/conv.py:50-79): 3 input channels, 3x3,
// stride 2, on the float32 NCHW image the caller hands over - as direct kernels, forward AND backward, that never store the raw
// convolution output.
//
// Why: this layer has 27 products per output and 3.3 M x 32 outputs at bs 32, 640 x 640: it is pure memory traffic.  Through the generic
// path it cost a layout pass (NCHW float32 -> NHWC bfloat16, channels padded to 8), an implicit GEMM whose K axis is 62 % padding, and the
// four BatchNorm passes of every Conv block over a 210 MB raw output - 515 us of a 13 ms step for 0.4 % of its FLOPs.  Recomputing the
// convolution is cheaper than reading it back, so here the raw output exists only in registers:
//   forward   K1  image (float32 NCHW, 157 MB) -> BatchNorm partial sums of the bfloat16-rounded outputs; by-product: the image as
//                 NHWC bfloat16 with 4 channels (26 MB, "x4"), the form every later kernel reads
//             --  finalize (ymi_bn_finalize, csrc/elementwise.hip)
//             K2  x4 -> convolution again -> scale / shift / SiLU -> the block's output (210 MB)
//   backward  K3  x4, dout -> convolution again -> partial sums of dz and dz * xhat  (dz = dout * act'(z))
//             --  final sums + apply coefficients (ymi_bn_bwd_final, csrc/reduce_bwd.hip)
//             K4  x4, dout -> convolution again -> d(raw) = dz c0 - raw c1 - c2 (rounded to bfloat16 as the generic path stores it)
//                 -> dW[k][co] += x[pixel, k] * d(raw)[pixel, co] by MFMA with the pixels as the K axis -> float32 slabs per workgroup,
//                 summed by the batched slab sum of csrc/wgrad.hip (deterministic).  The image gets no gradient.
// A workgroup owns a tile of TH x TW output pixels of one image; the (2 TH + 1) x (2 TW + 1) input patch sits in LDS as bfloat16
// [row][col][4] (8 bytes per pixel, the 4th channel zero).  K is ordered (kh, kw, c') with c' in 0..3, so every 8-byte LDS read is one
// input pixel's channels and K = 36, padded to 64: two 16x16x32 MFMAs per 16 pixels x 16 channels (the MFMA pipe is idle in these
// HBM-bound kernels anyway).  Arithmetic: bfloat16 products accumulated in float32 over the 27 taps, rounded to bfloat16 - exactly
// what the generic path computes and stores, so every consumer of the recomputed value sees the stored value's bits.
// (Handing dz from K3 to K4 instead of recomputing SiLU' there was measured: as bfloat16 it puts 2e-2 on dW - d(raw) cancels - and as
// float32 its 420 MB cost K3 more than K4 gained, 167 + 191 against 100 + 190 us.)
//
// K1..K4 are ONE tile walk (first_conv_kernel: weight fragments, tiles, patch, rows, 16-pixel groups, the convolution) around four pass
// types (FcStats, FcApply, FcBwdReduce, FcBwdWgrad).  A pass owns its arguments, its per-lane state, its rows of the constant table, its
// share of LDS and its hooks: per 16-pixel group and channel tile, per wave row, per tile, per workgroup.  The walk reads the pass's rows of
// the constant table itself and hands `red` over as the array it is: through a pointer the compiler assumed 16-byte alignment for the
// table reads and paired the `red` accesses otherwise (other instructions than these kernels had, profiles/first_conv_refactor_ab.txt).
// The split costs 87 code lines against the one-body kernel (profiles/first_conv_refactor_ab.txt: four argument structs where one served, a
// signature and the constants of every hook).
#include "common.h"

namespace {

constexpr int FC_TH = 8, FC_TW = 64;                   // output tile: two rows per wave
constexpr int FC_PR = 2 * FC_TH + 1;                   // patch rows
constexpr int FC_ROWB = (2 * FC_TW + 2) * 8;           // bytes per patch row: 8 bytes per pixel; col 0 unused, col 1 = left halo, cols 2.. = the tile's 2 TW columns
                                                       // (so that the aligned groups of the interior start on 16-byte boundaries)
constexpr int FC_WG_TILES = 4;                         // tiles per workgroup of the weight-gradient kernel, one slab each (2 and 8: slower, profiles/r04_first_conv_ab.txt)
constexpr int FC_CROWS = 5;                            // rows of the per-channel constant table [FC_CROWS][CO]; a pass names and fills the ones it reads

struct FcGeom {            // the same in every pass of a call (fc_geometry)
    int N, C, H, W, Ho, Wo;
    int tiles_h, tiles_w, total;
};
struct FcStatsArgs {
    FcGeom g;
    const float* img;      // float32 NCHW image
    const float* w;        // float32 OIHW weight (every pass)
    bf16_t* x4;            // NHWC bfloat16, 4 channels: written here, read by the other passes
    float* partials;       // [unit][2][CO]
};
struct FcApplyArgs {
    FcGeom g;
    const float* w;
    const bf16_t* x4;
    bf16_t* out;           // the block's output, NHWC with `ldout` elements per pixel
    int64_t ldout;
    const float* scale;    // [CO] each
    const float* shift;
    int act;
};
struct FcBwdReduceArgs {
    FcGeom g;
    const float* w;
    const bf16_t* x4;
    const bf16_t* dout;    // NHWC with `ldout` elements per pixel
    int64_t ldout;
    float* partials;       // [unit][2][CO]
    const float* gamma;    // [CO] each; gamma / beta may be null (1 / 0)
    const float* beta;
    const float* mean;
    const float* invstd;
    int act;
};
struct FcBwdWgradArgs {
    FcGeom g;
    const float* w;
    const bf16_t* x4;
    const bf16_t* dout;
    int64_t ldout;
    const float* coef;     // [5][CO] of ymi_bn_bwd_final: a0 | a1 | c0 | c1 | c2
    float* slab;           // [workgroup][CO][72] float32
    int act;
};

struct FcLane {            // a thread's places in its workgroup, wave and MFMA fragments; the LDS its hooks reach
    int tid, lane, wave, l15, l4;
    const char* patch;
    char* my;              // this wave's staging bytes
};
struct FcRow {             // a wave's output row of a tile
    int ohl, ow0;          // row within the tile; the tile's first column
    bool ok;               // inside the map
    int64_t pix;           // pixel index of (n, row, ow0) in the NHWC output map
};

// SiLU or identity (the host refuses other activations: GELU's erf would double these kernels' code for a case no model has)
__device__ __forceinline__ float fc_act(float x, int act) { return act == YMI_ACT_SILU ? silu_f(x) : x; }
__device__ __forceinline__ float fc_act_grad(float x, int act) { return act == YMI_ACT_SILU ? silu_grad_f(x) : 1.0f; }

// ---- transposed fragment read of a swizzled image (common.h: tr_frag_addr; SW = 2: 64-byte rows, SW = 0: 128-byte rows) through the builtin:
// the reads are ordered against this kernel's own plain LDS stores, which the compiler sees
template <int SW> __device__ __forceinline__ bf16x8 fc_tr_load(const char* img, int rowb, int c0, int lane) {
    typedef __attribute__((ext_vector_type(4))) short s16x4;
    typedef __attribute__((ext_vector_type(8))) short s16x8;
    const TrFragAddr ad = tr_frag_addr<SW>(img, rowb, c0, lane);
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)ad.lo);
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)ad.hi);
    const s16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return __builtin_bit_cast(bf16x8, v);
}

// ---- the input patch of tile (n, oh0, ow0) into LDS -----------------------------------------------------------------------------------
// from the float32 NCHW image (and, by the way, the tile's own pixels out to x4) ...
__device__ __forceinline__ void fc_load_patch(const FcStatsArgs& a, char* patch, int n, int oh0, int ow0, int tid) {
    const FcGeom& g = a.g;
    const float* src = a.img + (int64_t)n * g.C * g.H * g.W;
    const int64_t plane = (int64_t)g.H * g.W;
    const int ih0 = 2 * oh0 - 1;
    constexpr int ITEMS = FC_PR * (2 * FC_TW / 4);     // an item = one patch row x 4 consecutive image columns (16-byte aligned in the planes)
    constexpr int PASSES = (ITEMS + 255) / 256;
    f32x4 v[PASSES][3];
#pragma unroll
    for (int p = 0; p < PASSES; ++p) {
        const int it = tid + 256 * p;
        const int r = it / (2 * FC_TW / 4), gr = it % (2 * FC_TW / 4);
        const int ih = ih0 + r, iw = 2 * ow0 + 4 * gr;
        const bool ok = it < ITEMS && (unsigned)ih < (unsigned)g.H && iw < g.W;
#pragma unroll
        for (int c = 0; c < 3; ++c) v[p][c] = (ok && c < g.C) ? *reinterpret_cast<const f32x4*>(src + c * plane + (int64_t)ih * g.W + iw) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
    float halo = 0.f;                                  // left halo column (iw = 2 ow0 - 1): scalar loads by the first threads
    const int hr = tid / 4, hc = tid % 4;
    if (tid < FC_PR * 4) {
        const int ih = ih0 + hr, iw = 2 * ow0 - 1;
        if (hc < g.C && (unsigned)ih < (unsigned)g.H && iw >= 0) halo = src[hc * plane + (int64_t)ih * g.W + iw];
    }
#pragma unroll
    for (int p = 0; p < PASSES; ++p) {
        const int it = tid + 256 * p;
        if (it < ITEMS) {
            const int r = it / (2 * FC_TW / 4), gr = it % (2 * FC_TW / 4);
            char* dst = patch + r * FC_ROWB + (4 * gr + 2) * 8;
            *reinterpret_cast<u32x4*>(dst) = u32x4{pack_bf16x2(v[p][0][0], v[p][1][0]), pack_bf16x2(v[p][2][0], 0.f), pack_bf16x2(v[p][0][1], v[p][1][1]), pack_bf16x2(v[p][2][1], 0.f)};
            *reinterpret_cast<u32x4*>(dst + 16) = u32x4{pack_bf16x2(v[p][0][2], v[p][1][2]), pack_bf16x2(v[p][2][2], 0.f), pack_bf16x2(v[p][0][3], v[p][1][3]), pack_bf16x2(v[p][2][3], 0.f)};
        }
    }
    if (tid < FC_PR * 4) *reinterpret_cast<bf16_t*>(patch + hr * FC_ROWB + 1 * 8 + hc * 2) = (bf16_t)halo;
    if (g.C == 4) {  // (rare: a fourth input channel - filled in with scalar loads; the 16-byte stores above wrote zeros there)
        __syncthreads();
        for (int e = tid; e < FC_PR * 2 * FC_TW; e += 256) {
            const int r = e / (2 * FC_TW), cc = e % (2 * FC_TW);
            const int ih = ih0 + r, iw = 2 * ow0 + cc;
            if ((unsigned)ih < (unsigned)g.H && iw < g.W) *reinterpret_cast<bf16_t*>(patch + r * FC_ROWB + (cc + 2) * 8 + 6) = (bf16_t)src[3 * plane + (int64_t)ih * g.W + iw];
        }
    }
    __syncthreads();
    // x4: the image pixels this tile owns (rows 2 oh0 .. 2 oh0 + 2 TH - 1, cols 2 ow0 .. 2 ow0 + 2 TW - 1), two pixels per 16-byte store
#pragma unroll 4
    for (int e = tid; e < 2 * FC_TH * FC_TW; e += 256) {
        const int r = e / FC_TW, cc = 2 * (e - r * FC_TW);
        const int ih = 2 * oh0 + r, iw = 2 * ow0 + cc;
        if (ih < g.H && iw < g.W) *reinterpret_cast<u32x4*>(a.x4 + (((int64_t)n * g.H + ih) * g.W + iw) * 4) = *reinterpret_cast<const u32x4*>(patch + (r + 1) * FC_ROWB + (cc + 2) * 8);
    }
}
// ... or from x4 (already in the patch's own form: 8 bytes per pixel)
template <typename Args> __device__ __forceinline__ void fc_load_patch(const Args& a, char* patch, int n, int oh0, int ow0, int tid) {
    const FcGeom& g = a.g;
    const int ih0 = 2 * oh0 - 1;
    constexpr int ITEMS = FC_PR * FC_TW;               // an item = one patch row x 2 consecutive image columns (16 bytes)
    constexpr int PASSES = (ITEMS + 255) / 256;
    u32x4 v[PASSES];
#pragma unroll
    for (int p = 0; p < PASSES; ++p) {
        const int it = tid + 256 * p;
        const int r = it / FC_TW, gr = it % FC_TW;
        const int ih = ih0 + r, iw = 2 * ow0 + 2 * gr;
        const bool ok = it < ITEMS && (unsigned)ih < (unsigned)g.H && iw < g.W;
        v[p] = ok ? *reinterpret_cast<const u32x4*>(a.x4 + (((int64_t)n * g.H + ih) * g.W + iw) * 4) : u32x4{0u, 0u, 0u, 0u};
    }
    u32x2 halo = u32x2{0u, 0u};
    if (tid < FC_PR) {
        const int ih = ih0 + tid, iw = 2 * ow0 - 1;
        if ((unsigned)ih < (unsigned)g.H && iw >= 0) halo = *reinterpret_cast<const u32x2*>(a.x4 + (((int64_t)n * g.H + ih) * g.W + iw) * 4);
    }
#pragma unroll
    for (int p = 0; p < PASSES; ++p) {
        const int it = tid + 256 * p;
        if (it < ITEMS) *reinterpret_cast<u32x4*>(patch + (it / FC_TW) * FC_ROWB + (2 * (it % FC_TW) + 2) * 8) = v[p];
    }
    if (tid < FC_PR) *reinterpret_cast<u32x2*>(patch + tid * FC_ROWB + 8) = halo;
    __syncthreads();
}

// ---- 16 pixels x CO channels of the convolution from the patch: acc[ct][r] = channel ct*16 + 4*l4 + r of pixel mt*16 + l15 of the wave's
// output row, float32 -----------------------------------------------------------------------------------------------------------------
template <int NCT>
__device__ __forceinline__ void fc_conv_group(const char* patch, int ohl, int mt, int l15, int l4, const bf16x8 (&wf)[NCT][2], f32x4 (&acc)[NCT]) {
    const int owl = mt * 16 + l15;
    // K half 0: half-groups q = 2 l4, 2 l4 + 1 (all < 9); K half 1: q = 8 + 2 l4, 9 + 2 l4 - only q = 8 exists.  Patch column of
    // (output column owl, tap kw): image column 2 (ow0 + owl) + kw - 1 = patch column 2 owl + kw + 1
    const int q0 = 2 * l4, q1 = 2 * l4 + 1;
    const u32x2 lo0 = *reinterpret_cast<const u32x2*>(patch + (2 * ohl + q0 / 3) * FC_ROWB + (2 * owl + q0 % 3 + 1) * 8);
    const u32x2 hi0 = *reinterpret_cast<const u32x2*>(patch + (2 * ohl + q1 / 3) * FC_ROWB + (2 * owl + q1 % 3 + 1) * 8);
    u32x2 lo1 = u32x2{0u, 0u};
    if (l4 == 0) lo1 = *reinterpret_cast<const u32x2*>(patch + (2 * ohl + 2) * FC_ROWB + (2 * owl + 2 + 1) * 8);
    const bf16x8 x0 = __builtin_bit_cast(bf16x8, u32x4{lo0[0], lo0[1], hi0[0], hi0[1]});
    const bf16x8 x1 = __builtin_bit_cast(bf16x8, u32x4{lo1[0], lo1[1], 0u, 0u});
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) {
        acc[ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[ct][0], x0, f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
        acc[ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[ct][1], x1, acc[ct], 0, 0, 0);
    }
}

// ---- pieces that two passes share ---------------------------------------------------------------------------------------------------------
// what a pass says of itself unless it says otherwise, and the hooks it leaves empty
struct FcPass {
    static constexpr int TILES = 1;                    // tiles per workgroup
    static constexpr int STAGE_WAVE_BYTES = 0;         // LDS staging bytes of a wave
    static constexpr int RED_FLOATS = 0;               // floats of LDS the waves combine through
    static constexpr bool READS_DOUT = false;
    static constexpr int CROWS = 0;                    // rows of the constant table it reads
    template <typename Args> static __device__ __forceinline__ void constants(const Args&, int, float (&)[FC_CROWS]) {}
    template <typename Args> __device__ __forceinline__ void wave_row(const Args&, const FcLane&, const FcRow&) {}
    template <typename Args, int N> __device__ __forceinline__ void tile(const Args&, const FcLane&, float (&)[N], int) {}
    template <typename Args, int N> __device__ __forceinline__ void workgroup(const Args&, const FcLane&, float (&)[N], int) {}
};
constexpr int fc_lds_len(int n) { return n > 0 ? n : 1; }  // (an array a pass does not use still needs a length; the compiler drops it)

// the two backward passes: dout of a 16-pixel group (8-byte pieces: this lane's 4 channels of its pixel, per channel tile) is requested
// one group ahead of its use; zero outside the map
template <int NCT> struct FcDoutAhead {
    bf16x4 cur[NCT], nxt[NCT];
    template <typename Args> __device__ __forceinline__ void request(const Args& a, const FcLane& ln, const FcRow& row, int mt, bf16x4 (&dst)[NCT]) {
        const int owl = mt * 16 + ln.l15;
        const bool ok = row.ok && row.ow0 + owl < a.g.Wo;
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct)
            dst[ct] = ok ? *reinterpret_cast<const bf16x4*>(a.dout + row.pix * a.ldout + (int64_t)owl * a.ldout + ct * 16 + 4 * ln.l4) : bf16x4{(bf16_t)0.f, (bf16_t)0.f, (bf16_t)0.f, (bf16_t)0.f};
    }
    __device__ __forceinline__ void advance() {
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) cur[ct] = nxt[ct];
    }
};

// the two reducing passes: a lane's two partial sums per channel, and their way out after a tile - over the 16 pixels of a DPP row,
// the four waves through `red`, one row of partials[unit][2][CO]
template <int CO> struct FcSums {
    static constexpr int NCT = CO / 16;
    // [channel tile][r], as vectors like the accumulator fragment.  As float[NCT][4] members the compiler paired these additions otherwise
    // than for the arrays the kernel used to declare itself, and with the pairing changed which dz * xh products are fused into s2:
    // other last bits in dgamma / dbeta at 48 channels (profiles/first_conv_refactor_ab.txt)
    f32x4 s1[NCT], s2[NCT];
    __device__ __forceinline__ FcSums() {
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) s1[ct] = s2[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    __device__ __forceinline__ void store(float* partials, const FcLane& ln, float (&red)[4 * 2 * CO], int unit) {
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float t1 = row16_sum(s1[ct][r]), t2s = row16_sum(s2[ct][r]);
                if (ln.l15 == 0) {
                    float* dst = &red[ln.wave * 2 * CO + ct * 16 + 4 * ln.l4 + r];  // (one address, two offsets: the pair leaves as one ds_write2_b32)
                    dst[0] = t1;
                    dst[CO] = t2s;
                }
            }
        __syncthreads();
        if (ln.tid < 2 * CO) {
            const int which = ln.tid / CO, ch = ln.tid % CO;
            partials[((int64_t)unit * 2 + which) * CO + ch] = (red[(0 * 2 + which) * CO + ch] + red[(1 * 2 + which) * CO + ch]) + (red[(2 * 2 + which) * CO + ch] + red[(3 * 2 + which) * CO + ch]);
        }
    }
};

// ---- the four passes.  group(): channels ch0 .. ch0 + 3 (channel tile ct) of pixel owl of the wave's row; raw = the convolution rounded to
// bfloat16, ok = the pixel is inside the map, k = the pass's CROWS rows of the constant table at ch0 (one unused row for a pass that has
// none), dy = its dout (passes that read it) -----------------------------------------------------------------------------------------------
// K1: sums of raw and raw^2
template <int CO> struct FcStats : FcPass {
    typedef FcStatsArgs Args;
    static constexpr int RED_FLOATS = 4 * 2 * CO;
    FcSums<CO> sums;
    __device__ __forceinline__ void group(const Args&, const FcLane&, int ct, int, int, bool ok, const float (&raw)[4], const f32x4 (&)[1], const bf16x4&) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float v = ok ? raw[r] : 0.f;
            sums.s1[ct][r] += v;
            sums.s2[ct][r] += v * v;
        }
    }
    __device__ __forceinline__ void tile(const Args& a, const FcLane& ln, float (&red)[RED_FLOATS], int unit) { sums.store(a.partials, ln, red, unit); }
};

// K2: act(raw * scale + shift) -> the block's output
template <int CO> struct FcApply : FcPass {
    typedef FcApplyArgs Args;
    enum { SCALE, SHIFT, CROWS };                      // rows of the constant table
    static constexpr int CPP = CO / 8;                 // 16-byte chunks per output pixel
    static constexpr int STAGE_WAVE_BYTES = FC_TW * CO * 2;  // one wave's output row segment
    static __device__ __forceinline__ void constants(const Args& a, int ch, float (&c)[FC_CROWS]) {
        c[SCALE] = a.scale[ch];
        c[SHIFT] = a.shift[ch];
    }
    __device__ __forceinline__ void group(const Args& a, const FcLane& ln, int, int ch0, int owl, bool, const float (&raw)[4], const f32x4 (&k)[CROWS], const bf16x4&) {
        bf16x4 o;
#pragma unroll
        for (int r = 0; r < 4; ++r) o[r] = (bf16_t)fc_act(raw[r] * k[SCALE][r] + k[SHIFT][r], a.act);
        *reinterpret_cast<bf16x4*>(ln.my + (owl * CO + ch0) * 2) = o;
    }
    // the wave's 64 pixels x CO channels leave as 16-byte chunks: consecutive lanes, consecutive bytes of the NHWC row
    // (the staging area is this wave's own: its LDS writes and reads are ordered by the wave's program order)
    __device__ __forceinline__ void wave_row(const Args& a, const FcLane& ln, const FcRow& row) {
        if (row.ok) {
#pragma unroll
            for (int it = 0; it < FC_TW * CPP / 64; ++it) {
                const int q = it * 64 + ln.lane;
                const int px = q / CPP, cc = q % CPP;
                if (row.ow0 + px < a.g.Wo) *reinterpret_cast<u32x4*>(a.out + row.pix * a.ldout + (int64_t)px * a.ldout + cc * 8) = *reinterpret_cast<const u32x4*>(ln.my + q * 16);
            }
        }
    }
};

// K3: sums of dz and dz * xhat
template <int CO> struct FcBwdReduce : FcPass {
    typedef FcBwdReduceArgs Args;
    enum { INV, OFF, GAMMA, BETA, CROWS };             // xhat = raw * INV + OFF ; z = xhat * GAMMA + BETA
    static constexpr int RED_FLOATS = 4 * 2 * CO;
    static constexpr bool READS_DOUT = true;
    FcSums<CO> sums;
    static __device__ __forceinline__ void constants(const Args& a, int ch, float (&c)[FC_CROWS]) {
        const float g = a.gamma ? a.gamma[ch] : 1.f, bb = a.beta ? a.beta[ch] : 0.f, mu = a.mean[ch], iv = a.invstd[ch];
        c[INV] = iv;
        c[OFF] = -mu * iv;
        c[GAMMA] = g;
        c[BETA] = bb;
    }
    __device__ __forceinline__ void group(const Args& a, const FcLane&, int ct, int, int, bool, const float (&raw)[4], const f32x4 (&k)[CROWS], const bf16x4& dy) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float xh = raw[r] * k[INV][r] + k[OFF][r];
            const float dz = (float)dy[r] * fc_act_grad(xh * k[GAMMA][r] + k[BETA][r], a.act);  // (dout = 0 outside the image)
            sums.s1[ct][r] += dz;
            sums.s2[ct][r] += dz * xh;
        }
    }
    __device__ __forceinline__ void tile(const Args& a, const FcLane& ln, float (&red)[RED_FLOATS], int unit) { sums.store(a.partials, ln, red, unit); }
};

// K4: d(raw) of a wave row into the wave's [pixel][channel] image, the row's weight gradient by MFMA, one slab per workgroup
template <int CO> struct FcBwdWgrad : FcPass {
    typedef FcBwdWgradArgs Args;
    enum { A0, A1, C0, C1, C2, CROWS };                    // z = raw A0 + A1 ; d(raw) = dz C0 - raw C1 - C2   (the rows of Args::coef)
    static constexpr int NCT = CO / 16;
    static constexpr int DROWB = CO <= 32 ? 64 : 128, DSW = tr_swz_mode(DROWB);  // row bytes / swizzle mode of the [pixel][channel] image
    static constexpr int TILES = FC_WG_TILES;
    static constexpr int STAGE_WAVE_BYTES = FC_TW * DROWB;
    static constexpr int RED_FLOATS = 48 * CO;         // the [k][co] image the four waves' sums meet in
    static constexpr bool READS_DOUT = true;
    f32x4 dwa[3][NCT];                                 // dW[k = kt*16 + 4*l4 + r][co = ct*16 + l15]
    __device__ __forceinline__ FcBwdWgrad() {
#pragma unroll
        for (int kt = 0; kt < 3; ++kt)
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct) dwa[kt][ct] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    static __device__ __forceinline__ void constants(const Args& a, int ch, float (&c)[FC_CROWS]) {
        c[A0] = a.coef[ch];
        c[A1] = a.coef[CO + ch];
        c[C0] = a.coef[2 * CO + ch];
        c[C1] = a.coef[3 * CO + ch];
        c[C2] = a.coef[4 * CO + ch];
    }
    // d(raw), rounded to bfloat16 as the generic path stores it, into this wave's [pixel][channel] image (one 8-byte store;
    // the weight-gradient MFMAs read it transposed: fc_tr_load)
    __device__ __forceinline__ void group(const Args& a, const FcLane& ln, int, int ch0, int owl, bool ok, const float (&raw)[4], const f32x4 (&k)[CROWS], const bf16x4& dy) {
        bf16x4 o;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float dz = (float)dy[r] * fc_act_grad(raw[r] * k[A0][r] + k[A1][r], a.act);
            o[r] = (bf16_t)(ok ? dz * k[C0][r] - (raw[r] * k[C1][r] + k[C2][r]) : 0.f);
        }
        *reinterpret_cast<bf16x4*>(ln.my + owl * DROWB + ((ch0 >> 2) ^ (tr_swz<DSW>(owl) << 2)) * 8) = o;
    }
    // dW[k][co] += sum over the row's 64 pixels of x[pixel, k] * d(raw)[pixel, co]: pixels are the MFMA's K axis (two halves of 32).
    // A fragment (rows = k): lane (k = kt*16 + l15, pixels 32 h + 8 l4 + j): patch[(2 ohl + kh)][2 pixel + kw + 1][c'], k = (kh*3 + kw)*4 + c'
    // B fragment (cols = co): lane (co = ct*16 + l15, the same 8 pixels): transposed read of the [pixel][channel] image
    __device__ __forceinline__ void wave_row(const Args&, const FcLane& ln, const FcRow& row) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            bf16x8 df[NCT];
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct) df[ct] = fc_tr_load<DSW>(ln.my + 32 * h * DROWB, DROWB, ct * 16, ln.lane);
#pragma unroll
            for (int kt = 0; kt < 3; ++kt) {
                const int k = kt * 16 + ln.l15, q = k >> 2, c = k & 3;
                bf16x8 xf;
                if (q < 9) {
                    const char* base = ln.patch + (2 * row.ohl + q / 3) * FC_ROWB + (q % 3 + 1) * 8 + c * 2 + (32 * h + 8 * ln.l4) * 16;
#pragma unroll
                    for (int j = 0; j < 8; ++j) xf[j] = *reinterpret_cast<const bf16_t*>(base + j * 16);
                } else {
#pragma unroll
                    for (int j = 0; j < 8; ++j) xf[j] = (bf16_t)0.f;
                }
#pragma unroll
                for (int ct = 0; ct < NCT; ++ct) dwa[kt][ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xf, df[ct], dwa[kt][ct], 0, 0, 0);
            }
        }
    }
    // the four waves' sums -> one float32 slab [co][tap * 8 + c] per workgroup (the layout of wgrad_kernel's slabs for 8 padded input
    // channels: the batched slab sum of csrc/wgrad.hip adds the workgroups' slabs in a fixed order and scatters into OIHW)
    __device__ __forceinline__ void workgroup(const Args& a, const FcLane& ln, float (&red)[RED_FLOATS], int wg_unit) {
        for (int wv = 0; wv < 4; ++wv) {  // wave after wave into one [k][co] image (fixed order: deterministic)
            if (ln.wave == wv) {
#pragma unroll
                for (int kt = 0; kt < 3; ++kt)
#pragma unroll
                    for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            float* dst = &red[(kt * 16 + 4 * ln.l4 + r) * CO + ct * 16 + ln.l15];
                            *dst = wv == 0 ? dwa[kt][ct][r] : *dst + dwa[kt][ct][r];
                        }
            }
            __syncthreads();
        }
        float* slab = a.slab + (int64_t)wg_unit * CO * 72;
        for (int e = ln.tid; e < CO * 72; e += 256) {
            const int co = e / 72, col = e % 72, tap = col >> 3, c = col & 7;
            slab[e] = c < 4 ? red[(tap * 4 + c) * CO + co] : 0.f;
        }
    }
};

// ---- the walk: no pass arithmetic in it ----------------------------------------------------------------------------------------------------
template <int CO, template <int> class PassOf>
__global__ __launch_bounds__(256, 4) void first_conv_kernel(typename PassOf<CO>::Args a) {  // (4 waves per SIMD where LDS allows: these kernels live on latency hiding)
    typedef PassOf<CO> Pass;
    constexpr int NCT = CO / 16;                       // channel tiles of 16
    __shared__ __attribute__((aligned(16))) char patch[FC_PR * FC_ROWB];
    __shared__ __attribute__((aligned(16))) char stage[fc_lds_len(4 * Pass::STAGE_WAVE_BYTES)];  // (wave-private: no barrier guards it)
    __shared__ __attribute__((aligned(16))) bf16_t wtab[CO * 64];  // [co][k], k = (kh * 3 + kw) * 4 + c'
    __shared__ __attribute__((aligned(16))) float ctab[FC_CROWS * CO];
    __shared__ float red[fc_lds_len(Pass::RED_FLOATS)];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l15 = lane & 15, l4 = lane >> 4;

    // ---- the weight table (float32 OIHW parameter -> bfloat16 [co][k]) and the per-channel constants (fetched from LDS per
    // 16-pixel group: as five register arrays per lane they cost two waves per SIMD)
#pragma unroll
    for (int i = 0; i < CO * 64 / 256; ++i) {
        const int e = tid + 256 * i, co = e >> 6, k = e & 63, q = k >> 2, c = k & 3;
        wtab[e] = (bf16_t)((q < 9 && c < a.g.C) ? a.w[(co * a.g.C + c) * 9 + q] : 0.f);
    }
    if (tid < CO) {
        float c[FC_CROWS] = {0.f, 0.f, 0.f, 0.f, 0.f};
        Pass::constants(a, tid, c);
#pragma unroll
        for (int r = 0; r < FC_CROWS; ++r) ctab[r * CO + tid] = c[r];
    }
    __syncthreads();
    bf16x8 wf[NCT][2];                                 // this lane's weight fragments (A operand: rows = output channels)
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
        for (int h = 0; h < 2; ++h) wf[ct][h] = *reinterpret_cast<const bf16x8*>(wtab + (ct * 16 + l15) * 64 + 32 * h + 8 * l4);

    Pass pass;
    const FcLane ln{tid, lane, wave, l15, l4, patch, stage + wave * Pass::STAGE_WAVE_BYTES};
    // XCD ownership of the pixel order (common.h): consecutive units - tiles of one image, image after image - run on one XCD
    const int wg_unit = xcd_unit(blockIdx.x, gridDim.x);
#pragma unroll 1
    for (int ti = 0; ti < Pass::TILES; ++ti) {
        const int unit = wg_unit * Pass::TILES + ti;
        if (unit >= a.g.total) break;                  // (workgroup-uniform)
        const int tw = unit % a.g.tiles_w;
        const int t2 = unit / a.g.tiles_w;
        const int th = t2 % a.g.tiles_h, n = t2 / a.g.tiles_h;
        const int oh0 = th * FC_TH, ow0 = tw * FC_TW;
        if (ti > 0) __syncthreads();                   // everybody has finished reading the previous tile's patch
        fc_load_patch(a, patch, n, oh0, ow0, tid);

#pragma unroll 1
        for (int rr = 0; rr < FC_TH / 4; ++rr) {       // this wave's output rows: wave, wave + 4
            const int ohl = ln.wave + 4 * rr;
            const int oh = oh0 + ohl;
            const FcRow row{ohl, ow0, oh < a.g.Ho, ((int64_t)n * a.g.Ho + oh) * a.g.Wo + ow0};
            FcDoutAhead<NCT> dy;
            if constexpr (Pass::READS_DOUT) dy.request(a, ln, row, 0, dy.cur);
            // The group loop is NOT unrolled: unrolled, the compiler interleaves the four groups and needs 211 registers
            // (two waves per SIMD; a scheduling barrier per group did not stop it) - rolled, 90.
#pragma unroll 1
            for (int mt = 0; mt < 4; ++mt) {
                const int owl = mt * 16 + ln.l15;
                const bool ok = row.ok && ow0 + owl < a.g.Wo;
                if constexpr (Pass::READS_DOUT) {
                    if (mt + 1 < 4) dy.request(a, ln, row, mt + 1, dy.nxt);
                }
                f32x4 acc[NCT];
                fc_conv_group<NCT>(patch, ohl, mt, ln.l15, ln.l4, wf, acc);
#pragma unroll
                for (int ct = 0; ct < NCT; ++ct) {
                    int ch0 = ct * 16 + 4 * ln.l4;
                    asm volatile("" : "+v"(ch0));  // the constants are re-read from LDS per group: hoisted out of the loop they are 40 registers per lane
                    float raw[4];
#pragma unroll
                    for (int r = 0; r < 4; ++r) raw[r] = (float)(bf16_t)acc[ct][r];  // the value the generic path stores
                    f32x4 k[fc_lds_len(Pass::CROWS)];
#pragma unroll
                    for (int r = 0; r < Pass::CROWS; ++r) k[r] = *reinterpret_cast<const f32x4*>(ctab + r * CO + ch0);
                    pass.group(a, ln, ct, ch0, owl, ok, raw, k, dy.cur[ct]);
                }
                if constexpr (Pass::READS_DOUT) dy.advance();
            }
            pass.wave_row(a, ln, row);
        }
        pass.tile(a, ln, red, unit);
    }
    pass.workgroup(a, ln, red, wg_unit);
}

template <template <int> class PassOf>
int fc_launch(const typename PassOf<16>::Args& a, int64_t cout, unsigned blocks, hipStream_t s) {
    void (*const kernels[4])(typename PassOf<16>::Args) = {first_conv_kernel<16, PassOf>, first_conv_kernel<32, PassOf>, first_conv_kernel<48, PassOf>, first_conv_kernel<64, PassOf>};
    hipLaunchKernelGGL(kernels[cout / 16 - 1], dim3(blocks), dim3(256), 0, s, a);
    YMI_CHECK_LAUNCH("first_conv");
    return YMI_OK;
}

int fc_geometry(FcGeom& g, int64_t n, int64_t c, int64_t h, int64_t w, int64_t cout, int act) {
    YMI_CHECK_ARG(c >= 1 && c <= 4 && (cout == 16 || cout == 32 || cout == 48 || cout == 64), "first_conv: c <= 4 input channels, 16 / 32 / 48 / 64 output channels");
    YMI_CHECK_ARG(act == YMI_ACT_SILU || act == YMI_ACT_NONE, "first_conv: SiLU or no activation");
    YMI_CHECK_ARG(w % 4 == 0 && h % 2 == 0 && n > 0, "first_conv: even height, width a multiple of 4");
    const int64_t ho = h / 2, wo = w / 2;
    YMI_CHECK_ARG(n * ho * wo * cout < (1ll << 31) && n * h * w * 4 < (1ll << 31), "first_conv: too large for 32-bit indexing");
    g.N = (int)n; g.C = (int)c; g.H = (int)h; g.W = (int)w; g.Ho = (int)ho; g.Wo = (int)wo;
    g.tiles_h = (int)((ho + FC_TH - 1) / FC_TH); g.tiles_w = (int)((wo + FC_TW - 1) / FC_TW);
    g.total = (int)(n * g.tiles_h * g.tiles_w);
    return YMI_OK;
}

// the backward workspace, carved for a null base (its size) and for the caller's: the reduce pass's partial rows, the apply coefficients, the
// weight-gradient slabs and, on the next 64-byte address, the one-record table of the slab sum (1024 bytes cover the step and the record)
struct FcBwdSpace {
    float *part, *coef, *slab;
    ymi_wgrad_pending* table;
    int64_t wgs, bytes;
};
FcBwdSpace fc_bwd_carve(void* workspace, int64_t blocks, int64_t cout) {
    uintptr_t at = (uintptr_t)workspace;
    auto floats = [&](int64_t n) {
        float* r = reinterpret_cast<float*>(at);
        at += (uintptr_t)n * sizeof(float);
        return r;
    };
    FcBwdSpace v;
    v.wgs = (blocks + FC_WG_TILES - 1) / FC_WG_TILES;
    v.part = floats(blocks * 2 * cout);
    v.coef = floats(FC_CROWS * cout);
    v.slab = floats(v.wgs * cout * 72);
    v.table = reinterpret_cast<ymi_wgrad_pending*>((at + 63) & ~(uintptr_t)63);
    v.bytes = (int64_t)(at - (uintptr_t)workspace) + 1024;
    return v;
}

}  // namespace

extern "C" int64_t ymi_first_conv_stat_blocks(int64_t n, int64_t h, int64_t w) {
    const int64_t ho = h / 2, wo = w / 2;
    return n * ((ho + FC_TH - 1) / FC_TH) * ((wo + FC_TW - 1) / FC_TW);
}

// forward: statistics pass, finalize, apply pass.  x4: receives the image as NHWC bfloat16 [n, 4, h, w] (saved for the backward pass, which
// reads nothing else of the input).  out: bfloat16 [n, cout, h/2, w/2] NHWC.  workspace: (2 cout + (blocks + BN_STAGE_ROWS) 2 cout) floats.
extern "C" int ymi_first_conv_bn_act_fwd(const float* img_nchw, int64_t n, int64_t c, int64_t h, int64_t w, const float* weight_oihw, int64_t cout,
                                         const float* gamma, const float* beta, float* running_mean, float* running_var, float momentum, float eps,
                                         int32_t act, const ymi_tensor* x4, const ymi_tensor* out, float* save_mean, float* save_invstd,
                                         void* workspace, size_t workspace_bytes, void* stream) {
    YMI_CHECK_ARG(img_nchw && weight_oihw && ymi_tensor_ok(out) && ymi_tensor_ok(x4) && workspace, "first_conv: bad argument");
    YMI_CHECK_ARG(((uintptr_t)img_nchw & 15) == 0, "first_conv: 16-byte aligned image");
    FcGeom g{};
    int rc = fc_geometry(g, n, c, h, w, cout, act);
    if (rc) return rc;
    YMI_CHECK_ARG(out->dtype == YMI_BF16 && out->n == n && out->h == g.Ho && out->w == g.Wo && out->c == cout && out->ld % 8 == 0 && ((uintptr_t)out->data & 15) == 0,
                  "first_conv: output must be bfloat16 [n, cout, h/2, w/2] NHWC with 16-byte aligned rows");
    YMI_CHECK_ARG(x4->dtype == YMI_BF16 && x4->n == n && x4->h == h && x4->w == w && x4->c == 4 && x4->ld == 4 && ((uintptr_t)x4->data & 15) == 0,
                  "first_conv: the image copy must be dense bfloat16 [n, 4, h, w] NHWC");
    const int64_t blocks = g.total;
    const size_t need = (size_t)(2 * cout + (blocks + BN_STAGE_ROWS) * 2 * cout) * sizeof(float);
    if (workspace_bytes < need) {
        ymi_set_error("first_conv: workspace %zu < %zu bytes", workspace_bytes, need);
        return YMI_EWORKSPACE;
    }
    float* scale = reinterpret_cast<float*>(workspace);
    float* shift = scale + cout;
    float* partials = shift + cout;
    bf16_t* x4p = reinterpret_cast<bf16_t*>(x4->data);
    hipStream_t s = (hipStream_t)stream;
    rc = fc_launch<FcStats>(FcStatsArgs{g, img_nchw, weight_oihw, x4p, partials}, cout, (unsigned)blocks, s);
    if (rc) return rc;
    rc = ymi_bn_finalize(partials, blocks, n * g.Ho * g.Wo, cout, gamma, beta, running_mean, running_var, momentum, eps, scale, shift, save_mean, save_invstd, stream);
    if (rc) return rc;
    return fc_launch<FcApply>(FcApplyArgs{g, weight_oihw, x4p, reinterpret_cast<bf16_t*>(out->data), out->ld, scale, shift, act}, cout, (unsigned)blocks, s);
}

extern "C" int64_t ymi_first_conv_bwd_workspace(int64_t n, int64_t h, int64_t w, int64_t cout) {
    return fc_bwd_carve(nullptr, ymi_first_conv_stat_blocks(n, h, w), cout).bytes;
}

// backward of the block w.r.t. its parameters (the image receives no gradient): dgamma, dbeta [cout] and the weight gradient.
// pending == NULL: dw_oihw [cout, c, 3, 3] is complete when the stream reaches this point; else the slab sum is left to
// ymi_wgrad_reduce_batch with the record written to *pending (as ymi_conv2d_bwd_weight_deferred).  workspace: ymi_first_conv_bwd_workspace.
extern "C" int ymi_first_conv_bn_act_bwd(const ymi_tensor* x4, const float* weight_oihw, int64_t c, int64_t cout, const float* gamma, const float* beta,
                                         const float* save_mean, const float* save_invstd, int32_t act, const ymi_tensor* dout, float* dgamma,
                                         float* dbeta, float* dw_oihw, void* workspace, size_t workspace_bytes, ymi_wgrad_pending* pending, void* stream) {
    YMI_CHECK_ARG(ymi_tensor_ok(x4) && ymi_tensor_ok(dout) && weight_oihw && save_mean && save_invstd && dgamma && dbeta && dw_oihw && workspace, "first_conv_bwd: bad argument");
    FcGeom g{};
    int rc = fc_geometry(g, x4->n, c, x4->h, x4->w, cout, act);
    if (rc) return rc;
    YMI_CHECK_ARG(x4->dtype == YMI_BF16 && x4->c == 4 && x4->ld == 4 && ((uintptr_t)x4->data & 15) == 0, "first_conv_bwd: the image copy must be dense bfloat16 [n, 4, h, w] NHWC");
    YMI_CHECK_ARG(dout->dtype == YMI_BF16 && dout->n == x4->n && dout->h == g.Ho && dout->w == g.Wo && dout->c == cout && dout->ld % 4 == 0 && ((uintptr_t)dout->data & 7) == 0,
                  "first_conv_bwd: dout must be bfloat16 [n, cout, h/2, w/2] NHWC");
    const int64_t blocks = g.total;
    const FcBwdSpace ws = fc_bwd_carve(workspace, blocks, cout);
    if ((int64_t)workspace_bytes < ws.bytes) {
        ymi_set_error("first_conv_bwd: workspace too small");
        return YMI_EWORKSPACE;
    }
    const bf16_t* x4p = reinterpret_cast<const bf16_t*>(x4->data);
    const bf16_t* doutp = reinterpret_cast<const bf16_t*>(dout->data);
    hipStream_t s = (hipStream_t)stream;
    rc = fc_launch<FcBwdReduce>(FcBwdReduceArgs{g, weight_oihw, x4p, doutp, dout->ld, ws.part, gamma, beta, save_mean, save_invstd, act}, cout, (unsigned)blocks, s);
    if (rc) return rc;
    rc = ymi_bn_bwd_final(ws.part, (int)blocks, (int)cout, gamma, beta, save_mean, save_invstd, 1.0f / (float)((int64_t)x4->n * g.Ho * g.Wo), dgamma, dbeta, ws.coef, s);
    if (rc) return rc;
    rc = fc_launch<FcBwdWgrad>(FcBwdWgradArgs{g, weight_oihw, x4p, doutp, dout->ld, ws.coef, ws.slab, act}, cout, (unsigned)ws.wgs, s);
    if (rc) return rc;
    const ymi_wgrad_pending rec = ymi_wgrad_record(ws.slab, dw_oihw, cout * 72, (int)ws.wgs, 72, 8, (int)cout, (int)c, 9, false, nullptr, nullptr);
    if (pending) {
        *pending = rec;
        return YMI_OK;
    }
    return ymi_wgrad_reduce_batch(&rec, 1, ws.table, stream);
}
