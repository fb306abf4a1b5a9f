// Weight gradient of the NHWC convolution as a split-K MFMA GEMM:
//
//   dW[co][(tap, ci)] = sum over output pixels m of  dY[m][co] * X[pixel(m, tap)][ci]
//
// Both operands are "K-major" in memory (the reduction index m is the slow one), so tiles are staged
// in LDS exactly as they lie in HBM ([pixel][channel] rows, filled by 16-byte LDS-DMA) and the MFMA
// fragments are read TRANSPOSED with ds_read_b64_tr_b16 (bf16) or plain ds_read_b32 (f32 parity
// mode, 16x16x4 MFMA).  The pixel axis is split across workgroups; each split writes a slab of partial
// sums, a second kernel sums the slabs in float32 in a fixed order (deterministic, no atomics) and scatters
// into the reference's OIHW layout.  Slabs are float32 in parity mode and bfloat16 in the bf16 path:
// the first-level partials of a split - a sum over >= 256 pixels held in float32 registers -
// are rounded once on their way out, the second level stays float32.  That halves the slab traffic
// (36 MB -> 18 MB written per launch at bs 32, and the batched reduce reads half as much).
#include <stdlib.h>

#include <mutex>
#include <type_traits>

#include "common.h"

struct WgradArgs {
    const void* x;
    const void* dy;
    void* slab;
    int slab_bf16;
    float* bias_slab;  // optional [splits][CoutP]: column sums of dY per split (the bias gradient's partials), formed by the tiles of column block 0
    const void* zero;
    int64_t ldx, ldy;
    int Mpix, H, W, Ho, Wo;
    int stride, pad, KW;
    int CoutP, Cin, NG;
    int pix_per_split;
    int nx, ny, splits, xcd_map;  // launch geometry (set by the launcher)
    int pw_shift;                 // PATCH kernels: a K step is a (32 >> pw_shift) x (1 << pw_shift) patch of output pixels (see wgrad_kernel)
    uint32_t x_bytes, y_bytes;    // ... and the operands as buffers (sizes in bytes, < 2^31)
    uint32_t wo_mul, wo_shr, ho_mul, ho_shr;  // n / Wo, n / Ho by multiply-high (wg_fast_div)
};

// n / d for 0 <= n < 2^31 as (umulhi(n, mul) + n) >> shr with mul = floor(2^32 (2^shr - d) / d) + 1, shr = ceil(log2 d)
// (Granlund-Montgomery; exact also for d = 1 and powers of two, so the K loop needs no special case and no branch)
__device__ __forceinline__ int wg_fast_div(int n, uint32_t mul, uint32_t shr) { return (int)((__umulhi((uint32_t)n, mul) + (uint32_t)n) >> shr); }

constexpr int WG_BN = 128;   // tile columns ((tap, ci)); the rows (co) are the kernel's BM
constexpr int WG_BK = 32;    // pixels per K step (64 was measured 10-15 % slower: half as many resident workgroups per CU)
constexpr int WG_NS = 2;     // LDS ring stages of the bf16 kernels (three and four: +9 %, profiles/r05_wgrad_patch_walk_ab.txt)
constexpr int WG_WAVES = 5;  // waves per SIMD the 64-row tile's register allocation must allow (4 and 6: no better, profiles/r04_wgrad_targets_sweep.txt)

// the LDS ring of a launch: WG_NS stages of a [WG_BK][BM] dY image and a [WG_BK][WG_BN] X image (the kernel asserts what else must fit in it)
template <typename T, int BM> constexpr size_t wgrad_lds_bytes() { return (size_t)WG_NS * WG_BK * (BM + WG_BN) * sizeof(T); }

// `buffer_load_dwordx4 ... lds`: 16 bytes per lane from base + voff + soff into LDS (lane-linear behind `dst`), zeros for lanes whose offset is
// outside [0, bytes).  The resource is rebuilt from (base, bytes) at every call - four scalar moves - because a local of the resource type in a
// kernel TEMPLATE makes the host pass drop the instantiation's launch stub without a word (ROCm 7.2 clang): the type stays inside this function.
__device__ __forceinline__ void wg_buffer_to_lds(const void* base, uint32_t bytes, lptr_t dst, uint32_t voff, uint32_t soff) {
#if defined(__HIP_DEVICE_COMPILE__)
    __builtin_amdgcn_raw_ptr_buffer_load_lds(__builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, bytes, 0x00020000), dst, 16, voff, soff, 0, 0);
#endif
}
// `global_load_lds_dwordx4`: 16 bytes per lane from each lane's own address.  Behind a device-only function for the same reason: called from a member
// of a class template, the builtin makes the host pass drop the launch stub of every kernel instantiation but the first that uses that member.
__device__ __forceinline__ void wg_global_to_lds(const void* src, lptr_t dst) {
#if defined(__HIP_DEVICE_COMPILE__)
    __builtin_amdgcn_global_load_lds((gptr_t)src, dst, 16, 0, 0);
#endif
}
template <typename T> struct WFrag;

template <> struct WFrag<bf16_t> {
    // a fragment = 8 k-values (pixels 8g..8g+7) for column c0+i of a [pixel][col] LDS image (common.h: tr_frag_addr)
    // The reads are written as inline assembly.  Through the builtin the compiler sees LDS reads that may alias the LDS-DMA pieces
    // issued a few instructions earlier and puts `s_waitcnt vmcnt(0)` in front of them: every K step then waited for the pieces of the NEXT
    // step before it read its own fragments - the whole load latency exposed in every wave, every step.  The ring's protocol (counted wait +
    // barrier at the top of a step, pieces only into the stage nobody reads) is what orders the two; the compiler cannot know and must not
    // add to it.
    static __device__ __forceinline__ void read2(bf16x8& f, const TrFragAddr& ad) {  // two transposed 8-byte reads fill one 8-value fragment
        typedef __attribute__((ext_vector_type(2))) uint32_t u2;
        u2 lo, hi;
        asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(lo) : "v"((uint32_t)(uintptr_t)ad.lo));
        asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(hi) : "v"((uint32_t)(uintptr_t)ad.hi));
        const u32x4 v = {lo[0], lo[1], hi[0], hi[1]};
        f = __builtin_bit_cast(bf16x8, v);
    }
    template <int BM, int TR, int TC, bool BIAS>
    static __device__ __forceinline__ void step(const char* Ys, const char* Xs, int r0, int c0, int lane, f32x4 (&acc)[TR][TC], bool bias, f32x4 (&accb)[BIAS ? TR : 1]) {
        static_assert(WG_BK == 32, "one 32-deep sub-step");
        bf16x8 af[TR], bfr[TC];
        // addresses first (plain arithmetic), then every read of the step back to back: X fragments, then the dY fragments in the
        // order the MFMA rows use them
        TrFragAddr ay[TR], ax[TC];
#pragma unroll
        for (int t = 0; t < TR; ++t) ay[t] = tr_frag_addr<tr_swz_mode(BM * 2)>(Ys, BM * 2, r0 + t * 16, lane);
#pragma unroll
        for (int t = 0; t < TC; ++t) ax[t] = tr_frag_addr<tr_swz_mode(WG_BN * 2)>(Xs, WG_BN * 2, c0 + t * 16, lane);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int t = 0; t < TC; ++t) read2(bfr[t], ax[t]);
#pragma unroll
        for (int t = 0; t < TR; ++t) read2(af[t], ay[t]);
#pragma unroll
        for (int a = 0; a < TR; ++a) {
            // row a needs the X fragments and dY fragment a: the 2 * (TR - 1 - a) younger reads may still be in flight
            __builtin_amdgcn_sched_barrier(0);
            if (a == 0) asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(2 * (TR - 1)) : "memory");
            else if (a == 1) asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(TR > 2 ? 2 * (TR - 2) : 0) : "memory");
            else if (a == 2) asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(TR > 3 ? 2 * (TR - 3) : 0) : "memory");
            else asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            asm volatile("" : "+v"(af[a]));
            if (a == 0) {
#pragma unroll
                for (int b = 0; b < TC; ++b) asm volatile("" : "+v"(bfr[b]));
            }
#pragma unroll
            for (int b = 0; b < TC; ++b)
                acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bfr[b], af[a], acc[a][b], 0, 0, 0);  // operands swapped: see the epilogue
            if (BIAS && bias) {  // (wave-uniform) column sums of dY: a row of ones against the dY fragment already in registers - one more MFMA per row
                typedef __attribute__((ext_vector_type(8))) short s16x8;
                const s16x8 one8 = {0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80};  // 1.0 in bfloat16
                const bf16x8 ones = __builtin_bit_cast(bf16x8, one8);
                if constexpr (BIAS) accb[a] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ones, af[a], accb[a], 0, 0, 0);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
    }
};
template <> struct WFrag<float> {
    template <int BM, int TR, int TC, bool BIAS>
    static __device__ __forceinline__ void step(const char* Ys, const char* Xs, int r0, int c0, int lane, f32x4 (&acc)[TR][TC], bool bias, f32x4 (&accb)[BIAS ? TR : 1]) {
        const int kq = lane >> 4, i = lane & 15;
#pragma unroll
        for (int ks = 0; ks < WG_BK / 4; ++ks) {
            float af[TR], bfr[TC];
#pragma unroll
            for (int t = 0; t < TR; ++t) af[t] = *reinterpret_cast<const float*>(Ys + ((4 * ks + kq) * BM + r0 + t * 16 + i) * 4);
#pragma unroll
            for (int t = 0; t < TC; ++t) bfr[t] = *reinterpret_cast<const float*>(Xs + ((4 * ks + kq) * WG_BN + c0 + t * 16 + i) * 4);
#pragma unroll
            for (int a = 0; a < TR; ++a)
#pragma unroll
                for (int b = 0; b < TC; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(bfr[b], af[a], acc[a][b], 0, 0, 0);
            if (BIAS && bias) {
#pragma unroll
                for (int a = 0; a < (BIAS ? TR : 1); ++a) accb[a] = __builtin_amdgcn_mfma_f32_16x16x4f32(1.0f, af[a], accb[a], 0, 0, 0);
            }
        }
    }
};

// ---- a workgroup's tile and its loader map ---------------------------------------------------------------------------------------------------
// BM = output channels per workgroup tile: 64, or 128 for layers with >= 128 output channels (16 instead of 8 MFMAs per
// wave and K step against the same address arithmetic: the K loop is instruction-issue-bound, not MFMA-bound), or 32 for the
// layers with <= 32 output channels (the 320x320 / 160x160 maps: millions of pixels against a 32 x 72..288 weight matrix; the
// 64-row tile spent half its MFMAs on padding rows)
// (a 128x256 tile - 4 or 8 waves - measured 1.17-1.66x slower, profiles/r02_conv_bench_wgrad256.txt)
// ... and what both pixel walks share: the thread -> (row, 16-byte chunk) map of the loader and the LDS slot of a piece.
// A thread fetches the same chunk column of rows y_row(i), i < NY, of the dY image and of rows x_row(i), i < NX, of the X image.  bf16: LDS position
// (row, chunk') holds source chunk chunk' ^ (swizzle(row) << 1); the row bits the swizzle uses are the same for all of a thread's rows.  The X chunk
// column fixes the thread's tap and input channel.
template <typename T, int BM> struct WgTile {
    static constexpr int NT = 256;
    static constexpr int CH = ElemTraits<T>::CH, ES = (int)sizeof(T);
    static constexpr int YCW = BM * ES / 16, XCW = WG_BN * ES / 16;  // 16-byte chunks per tile row
    // threads that cover one dY load of the workgroup (32-channel tile: 128 - the other two waves fetch the SAME chunks to the SAME LDS bytes, so every
    // wave issues the same number of loads and the counted waits stay uniform)
    static constexpr int YT = WG_BK * YCW < NT ? WG_BK * YCW : NT;
    static constexpr int NY = (WG_BK * YCW + NT - 1) / NT, NX = WG_BK * XCW / NT;  // 16-byte pieces per thread per K step
    static constexpr int WCOLS = WG_BN / 64, WROWS = (NT / 64) / WCOLS;            // wave grid: every wave owns a (BM / WROWS) x 64 tile ...
    static constexpr int WM = BM / WROWS, TR = WM / 16, TC = 4;                    // ... of TR x TC MFMA tiles
    static constexpr int YBYTES = WG_BK * BM * ES, XBYTES = WG_BK * WG_BN * ES, STAGE = YBYTES + XBYTES;  // a ring stage: the dY image, then the X image
    static_assert(NY >= 1 && NX >= 1, "tile too small");
    static constexpr bool SWZ = std::is_same<T, bf16_t>::value;
    static_assert(NT / XCW >= 16 || !SWZ, "bf16: a block-wide load covers >= 16 rows, so a thread's rows share the row bits the swizzle uses");
    int yrow0, ych;         // first dY row; output channel of the chunk
    bool y_cok, x_cok;      // the chunk lies inside the padded channels / inside (tap, ci)
    int xrow0, ci, dh, dw;  // first X row; input channel and tap shift of the chunk
    __device__ __forceinline__ WgTile(const WgradArgs& a, int tid, int j0, int co0) {
        const int ytid = tid % YT;
        yrow0 = ytid / YCW;
        const int ycc = SWZ ? ((ytid % YCW) ^ (tr_swz<tr_swz_mode(YCW * 16)>(yrow0) << 1)) : (ytid % YCW);
        ych = co0 + ycc * CH;
        y_cok = ych < a.CoutP;
        xrow0 = tid / XCW;
        const int xcc = SWZ ? ((tid % XCW) ^ (tr_swz<tr_swz_mode(XCW * 16)>(xrow0) << 1)) : (tid % XCW);
        const int j = j0 + xcc * CH;
        x_cok = j < a.NG;
        const int tap = x_cok ? j / a.Cin : 0;
        ci = x_cok ? j - tap * a.Cin : 0;
        dh = tap / a.KW - a.pad;
        dw = tap % a.KW - a.pad;
    }
    __device__ __forceinline__ int y_row(int i) const { return yrow0 + i * (NT / YCW); }
    __device__ __forceinline__ int x_row(int i) const { return xrow0 + i * (NT / XCW); }
    // LDS-DMA writes a wave's 64 pieces lane-linear behind a wave-uniform address
    static __device__ __forceinline__ lptr_t y_slot(char* Ys, int i, int wave) { return (lptr_t)(Ys + (i * NT + (wave * 64) % YT) * 16); }
    static __device__ __forceinline__ lptr_t x_slot(char* Xs, int i, int wave) { return (lptr_t)(Xs + (i * NT + wave * 64) * 16); }
};

// ---- the raster walk: the K axis runs over the output pixels m_begin, m_begin + 1, ... of the split -------------------------------------------
// Address state of this thread's rows, advanced by WG_BK pixels per K step with adds and compares only (the pixel ->
// (n, ho, wo) decomposition by two multiply-highs and five multiplies per piece and step cost ~160 cycles per piece: the
// issue phase was half of a K step, stamps in profiles/r02_igemm_phase_stamps.txt section 6).  issue() is called for
// consecutive steps m_begin, m_begin + WG_BK, ...: it uses the state and then moves it one step on.
//   X row: ws = wo * stride, hs = ho * stride (input coordinates of the tap-(0,0) pixel), x_off = element offset of that pixel
//          + this thread's tap shift and channel; a step adds (q, r) = divmod(WG_BK, Wo) rows / columns, then wraps.
//   Y row: element offset m * ldy + channel.
// Pieces outside the split, the map or the channels read the zero page.
template <typename T, int BM> struct WgRasterWalk {
    using G = WgTile<T, BM>;
    const WgradArgs& a;
    const G& ld;
    const int wave, m_end;
    const int s_ = a.stride, ldx32 = (int)a.ldx, ldy32 = (int)a.ldy;
    const int q_ = WG_BK / a.Wo, r_ = WG_BK - q_ * a.Wo;                              // scalar
    const uint32_t d_step = (uint32_t)((q_ * s_ * a.W + r_ * s_) * ldx32);            // offset change of (ho += q, wo += r)
    const uint32_t d_wwrap = (uint32_t)((s_ * a.W - a.Wo * s_) * ldx32);              // ... of (wo -= Wo, ho += 1)
    const uint32_t d_hwrap = (uint32_t)((a.H * a.W - a.Ho * s_ * a.W) * ldx32);       // ... of (ho -= Ho, n += 1)
    const uint32_t y_step = (uint32_t)(WG_BK * ldy32);
    const int ws_lim = a.Wo * s_, hs_lim = a.Ho * s_;
    int x_ws[G::NX], x_hs[G::NX];
    uint32_t x_off[G::NX], y_off[G::NY];
    __device__ __forceinline__ WgRasterWalk(const WgradArgs& a_, const G& ld_, int wave_, int m_begin)
        : a(a_), ld(ld_), wave(wave_), m_end(min(a_.Mpix, m_begin + a_.pix_per_split)) {
#pragma unroll
        for (int i = 0; i < G::NX; ++i) {
            const int m = m_begin + ld.x_row(i);
            const int t = wg_fast_div(m, a.wo_mul, a.wo_shr);
            const int wo = m - t * a.Wo;
            const int n = wg_fast_div(t, a.ho_mul, a.ho_shr);
            const int ho = t - n * a.Ho;
            x_ws[i] = wo * s_;
            x_hs[i] = ho * s_;
            x_off[i] = (uint32_t)(((n * a.H + ho * s_ + ld.dh) * a.W + wo * s_ + ld.dw) * ldx32 + ld.ci);
        }
#pragma unroll
        for (int i = 0; i < G::NY; ++i) y_off[i] = (uint32_t)((m_begin + ld.y_row(i)) * ldy32 + ld.ych);
    }
    __device__ __forceinline__ void issue(char* Ys, int mk) {
        const T* __restrict__ xg = reinterpret_cast<const T*>(a.x);
        const T* __restrict__ yg = reinterpret_cast<const T*>(a.dy);
        const T* zero = reinterpret_cast<const T*>(a.zero);
        char* Xs = Ys + G::YBYTES;
        const int left = m_end - mk;  // scalar: rows below it are inside this split
#pragma unroll
        for (int i = 0; i < G::NY; ++i) {
            const bool ok = ld.y_cok && ld.y_row(i) < left;
            const T* src = ok ? yg + y_off[i] : zero;
            wg_global_to_lds(src, ld.y_slot(Ys, i, wave));
            y_off[i] += y_step;
        }
#pragma unroll
        for (int i = 0; i < G::NX; ++i) {
            const bool ok = ld.x_cok && ld.x_row(i) < left && (unsigned)(x_hs[i] + ld.dh) < (unsigned)a.H && (unsigned)(x_ws[i] + ld.dw) < (unsigned)a.W;
            const T* src = ok ? xg + x_off[i] : zero;
            wg_global_to_lds(src, ld.x_slot(Xs, i, wave));
            // one K step on
            x_ws[i] += r_ * s_;
            x_hs[i] += q_ * s_;
            x_off[i] += d_step;
            if (x_ws[i] >= ws_lim) {
                x_ws[i] -= ws_lim;
                x_hs[i] += s_;
                x_off[i] += d_wwrap;
            }
            while (x_hs[i] >= hs_lim) {  // at most once unless the map has fewer rows than a K step covers
                x_hs[i] -= hs_lim;
                x_off[i] += d_hwrap;
            }
        }
    }
};

// ---- the patch walk: the K axis runs over the output pixels in PATCH order instead of raster order --------------------------------------------
// Step k is a ph x pw patch (ph * pw = 32, pw a power of two dividing Wo, ph dividing Ho) whose origin (n, ho0, wo0) is SCALAR state.  A lane's
// row of the step is a fixed (pr, pc) inside the patch, so its source offset is a per-thread constant plus a scalar: the pieces become
// `buffer_load_dwordx4 ... lds` with the constant in the vector offset and the patch origin in the scalar offset, padding taps are lanes whose
// vector offset is pushed out of range (the buffer unit writes zeros to LDS for them: tools/probes/bar/buffer_lds_probe.hip), and the per-lane
// (ho, wo) walk with its wraps - as many issue slots as the MFMAs (profiles/r05_wgrad_patch_walk_ab.txt) - is five vector instructions per X
// piece and none per dY piece.  Any fixed order of the pixel sum is as good as raster order; maps that do not tile into such patches (20 x 20)
// keep the raster walk.  Splits are whole patches (the launcher: Mpix % WG_BK == 0), so no piece is cut by the split's end.
template <typename T, int BM> struct WgPatchWalk {
    using G = WgTile<T, BM>;
    static constexpr uint32_t OOR = 0x80000000u;  // a vector offset beyond any buffer of < 2^31 bytes (vector + scalar offset stays below 2^32)
    static constexpr int ES = G::ES;
    const WgradArgs& a;
    const int wave;
    const int s_ = a.stride, ldx32 = (int)a.ldx, ldy32 = (int)a.ldy;
    const int pw = 1 << a.pw_shift, ph = WG_BK >> a.pw_shift;
    const uint32_t xbias = (uint32_t)((a.W + 1) * ldx32 * ES);  // keeps the (dh, dw) = (-1, -1) offsets non-negative
    uint32_t pvx[G::NX], pvy[G::NY];  // per-thread constants: vector byte offsets of the pieces inside a patch ...
    int pch[G::NX], pcw[G::NX];       // ... and the X pieces' input row / column relative to the patch origin's
    int p_wo, p_ho;                   // scalar: the next patch's origin
    uint32_t p_sx, p_sy;              // scalar byte offsets of that origin in X (tap (0, 0), channel 0) and dY
    __device__ __forceinline__ WgPatchWalk(const WgradArgs& a_, const G& ld, int wave_, int m_begin) : a(a_), wave(wave_) {
#pragma unroll
        for (int i = 0; i < G::NX; ++i) {
            const int row = ld.x_row(i);
            const int pr = row >> a.pw_shift, pc = row & (pw - 1);
            pch[i] = pr * s_ + ld.dh;
            pcw[i] = pc * s_ + ld.dw;
            pvx[i] = ld.x_cok ? (uint32_t)(((pch[i] * a.W + pcw[i]) * ldx32 + ld.ci) * ES) + xbias : OOR;
        }
#pragma unroll
        for (int i = 0; i < G::NY; ++i) {
            const int row = ld.y_row(i);
            const int pr = row >> a.pw_shift, pc = row & (pw - 1);
            pvy[i] = ld.y_cok ? (uint32_t)(((pr * a.Wo + pc) * ldy32 + ld.ych) * ES) : OOR;
        }
        const int pidx = __builtin_amdgcn_readfirstlane(m_begin / WG_BK);  // first patch of this split
        const int npw = a.Wo >> a.pw_shift, nph = a.Ho / ph;
        const int t = pidx / npw, wp = pidx - t * npw;
        const int n = t / nph, hp = t - n * nph;
        p_wo = wp * pw;
        p_ho = hp * ph;
        p_sx = (uint32_t)(((n * a.H + p_ho * s_) * a.W + p_wo * s_) * ldx32 * ES);
        p_sy = (uint32_t)(((n * a.Ho + p_ho) * a.Wo + p_wo) * ldy32 * ES);
    }
    __device__ __forceinline__ void issue(char* Ys, int) {
        char* Xs = Ys + G::YBYTES;
        const char* xbase = reinterpret_cast<const char*>(a.x) - xbias;
        const uint32_t sx = __builtin_amdgcn_readfirstlane(p_sx), sy = __builtin_amdgcn_readfirstlane(p_sy);  // (scalar by construction; said so)
#pragma unroll
        for (int i = 0; i < G::NY; ++i) wg_buffer_to_lds(a.dy, a.y_bytes, G::y_slot(Ys, i, wave), pvy[i], sy);
        const int hs0 = __builtin_amdgcn_readfirstlane(p_ho * s_), ws0 = __builtin_amdgcn_readfirstlane(p_wo * s_);
#pragma unroll
        for (int i = 0; i < G::NX; ++i) {
            const bool ok = (unsigned)(hs0 + pch[i]) < (unsigned)a.H && (unsigned)(ws0 + pcw[i]) < (unsigned)a.W;
            wg_buffer_to_lds(xbase, a.x_bytes + xbias, G::x_slot(Xs, i, wave), ok ? pvx[i] : OOR, sx);
        }
        // one patch on (scalar)
        p_wo += pw;
        p_sx += (uint32_t)(pw * s_ * ldx32 * ES);
        p_sy += (uint32_t)(pw * ldy32 * ES);
        if (p_wo == a.Wo) {
            p_wo = 0;
            p_ho += ph;
            p_sx += (uint32_t)((ph * s_ * a.W - a.Wo * s_) * ldx32 * ES);
            p_sy += (uint32_t)((ph * a.Wo - a.Wo) * ldy32 * ES);
            if (p_ho == a.Ho) {
                p_ho = 0;
                p_sx += (uint32_t)((a.H * a.W - a.Ho * s_ * a.W) * ldx32 * ES);
            }
        }
    }
};

// ---- the LDS-staged slab store of the bf16 kernels -----------------------------------------------------------------------------------------------
// Written straight from the accumulators, a store instruction covers 16 rows x 32 bytes (bfloat16 slabs) - sixteen partial lines - and those stores
// cost 8 % of the family's time (0.7 ms per step if nothing hid them: profiles/r05_wgrad_slab_stores_ab.txt).  Each wave drops RP 16-row tiles x 64
// columns of its accumulators, converted to the slab's element type S, into a private padded image in the ring and stores it back as whole row
// segments of 64 columns, 16 bytes per lane.  Same values, same rounding.
template <typename S, int TR> struct SlabStage {
    static constexpr int ES = (int)sizeof(S);
    static constexpr int SROW = 64 * ES + 16;              // padded row: 16 rows hit 16 distinct bank groups
    static constexpr int CPR = 64 * ES / 16;               // 16-byte chunks = lanes per row segment (128 bytes of bfloat16, 256 of float32)
    static constexpr int RPI = 64 / CPR;                   // rows per store instruction: 8 / 4
    static constexpr int RP = TR < 4 / ES ? TR : 4 / ES;   // 16-row tiles per pass: up to 32 rows x 128 bytes or 16 rows x 256 bytes
    static constexpr int BYTES = RP * 16 * SROW;           // of the ring, per wave
    static_assert(TR % RP == 0, "whole passes");
};
// slab: this split's [CoutP][NG] slab; (row0, col0): the wave's first output channel and (tap, ci) column.  NG is a multiple of 8.
template <typename S, int TR, int TC>
__device__ __forceinline__ void wg_store_slab_staged(char* ring, int wave, int lane, const f32x4 (&acc)[TR][TC], S* slab, int row0, int col0, int CoutP, int NG) {
    using St = SlabStage<S, TR>;
    constexpr int ES = St::ES, SROW = St::SROW, RP = St::RP;
    static_assert(TC * 16 == 64, "a wave's tile is 64 columns wide");
    __syncthreads();  // the other waves may still read the last K step's stage
    // the lane is made opaque here: its pieces below use the lane bits the fragment addresses use, and formed once, ahead of the K loop, they hold a
    // VGPR across it (the 64-row raster kernel then takes 82 VGPRs instead of 80 and loses its sixth wave per SIMD)
    asm volatile("" : "+v"(lane));
    char* st = ring + wave * St::BYTES;
    const int l15 = lane & 15, l4 = lane >> 4;
    const int srow = lane / St::CPR, sch = lane % St::CPR;
    const int col = col0 + sch * (16 / ES);
#pragma unroll
    for (int r0 = 0; r0 < TR; r0 += RP) {
#pragma unroll
        for (int rr = 0; rr < RP; ++rr)
#pragma unroll
            for (int c = 0; c < TC; ++c) {
                char* p = st + (rr * 16 + l15) * SROW + (c * 16 + 4 * l4) * ES;
                if constexpr (std::is_same<S, float>::value) {
                    *reinterpret_cast<f32x4*>(p) = acc[r0 + rr][c];
                } else {
                    const bf16x4 v = {(bf16_t)acc[r0 + rr][c][0], (bf16_t)acc[r0 + rr][c][1], (bf16_t)acc[r0 + rr][c][2], (bf16_t)acc[r0 + rr][c][3]};
                    *reinterpret_cast<bf16x4*>(p) = v;
                }
            }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
        for (int k = 0; k < RP * 16 / St::RPI; ++k) {
            const int row = k * St::RPI + srow;
            const u32x4 u = *reinterpret_cast<const u32x4*>(st + row * SROW + sch * 16);
            const int co = row0 + r0 * 16 + row;
            if (co < CoutP && col < NG) *reinterpret_cast<u32x4*>(slab + (int64_t)co * NG + col) = u;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
}

// ---- which tile a workgroup runs -------------------------------------------------------------------------------------------------------------
// -> (bx, by, bz) = column block, row block, pixel split; false: a padding id of the XCD-mapped grid.  first: workgroups ahead of the tiles (riders).
__device__ __forceinline__ bool wg_tile_of_block(const WgradArgs& a, int first, int& bx, int& by, int& bz) {
    if (a.xcd_map) {
        const int id = (int)blockIdx.x - first, xcd = id & 7, seq = id >> 3, nxy = a.nx * a.ny;
        const int zi = seq / nxy, t = seq - zi * nxy;
        const int spx = (a.splits + 7) >> 3;
        bz = xcd * spx + zi;
        if (zi >= spx || bz >= a.splits) return false;
        by = t / a.nx;
        bx = t - by * a.nx;
    } else {
        bx = blockIdx.x; by = blockIdx.y; bz = blockIdx.z;
    }
    return true;
}

// ---- the kernel ------------------------------------------------------------------------------------------------------------------------------
// BIAS: the instantiation that also forms the bias gradient's partials (its own code object: the 4 * TR accumulator registers and the branch
// cost the bias-free launches 3-4 % when they were a run-time option of one kernel)
// PATCH: the patch walk instead of the raster walk
// the final pass of a BatchNorm backward as a rider (common.h: BnRider): the first rider.nwg workgroups of the 1-D grid run bn_final_block, the function
// chan_reduce_final_kernel runs as its own launch (reduce_bwd.hip), on the ring's LDS - a thread plays four of the 32 row slices - and leave.
template <typename T, int BM, bool BIAS, bool PATCH>
__global__ __launch_bounds__(256, (BM == 128 ? 3 : WG_WAVES)) void wgrad_kernel(WgradArgs a, BnRider rider) {
    using G = WgTile<T, BM>;
    constexpr int NT = G::NT, TR = G::TR, TC = G::TC, WM = G::WM, STAGE = G::STAGE, NS = WG_NS;
    constexpr int LDS = (int)wgrad_lds_bytes<T, BM>();  // what the launcher gives
    static_assert(LDS == NS * STAGE, "the launcher's LDS bytes are the ring");
    static_assert(LDS >= (NT / 64) * SlabStage<bf16_t, TR>::BYTES && LDS >= (NT / 64) * SlabStage<float, TR>::BYTES, "the staged slab stores use the ring");
    static_assert(LDS >= BN_FINAL_RED * (int)sizeof(double), "a rider workgroup sums its slices in the ring");
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave / G::WCOLS, wc = wave % G::WCOLS;
    // XCD-aware order (xcd_map): workgroup ids are dealt round-robin to the 8 XCDs; all tiles of one pixel split read the
    // same dY / X rows (the nine taps are the same pixels, shifted), so a split's tiles are given to ONE XCD, back to
    // back, and its rows are fetched into that L2 once.  An XCD gets CONSECUTIVE splits, z = xcd * ceil(splits / 8) + i: its
    // eighth of the pixel order (common.h, XCD ownership of the pixel axis) - the BatchNorm apply pass wrote those dY rows from
    // this XCD a launch ago (dealt z = 8 i + xcd, every split's rows came from the other seven L2s).
    int bx, by, bz;
    if (rider.nwg && (int)blockIdx.x < rider.nwg) {  // (only in the 1-D XCD-mapped grid; workgroup-uniform)
        if ((int)blockIdx.x * 32 < rider.f.C) bn_final_block<NT, false>(rider.f, (int)blockIdx.x, reinterpret_cast<double*>(smem));  // (else: a padding workgroup of the rider block)
        return;
    }
    if (!wg_tile_of_block(a, rider.nwg, bx, by, bz)) return;  // padding ids leave before any barrier
    const int j0 = bx * WG_BN, co0 = by * BM;
    const int m_begin = bz * a.pix_per_split;
    const int m_end = min(a.Mpix, m_begin + a.pix_per_split);
    const G ld(a, tid, j0, co0);
    typename std::conditional<PATCH, WgPatchWalk<T, BM>, WgRasterWalk<T, BM>>::type walk(a, ld, wave, m_begin);

    f32x4 acc[TR][TC];
#pragma unroll
    for (int r = 0; r < TR; ++r)
#pragma unroll
        for (int c = 0; c < TC; ++c) acc[r][c] = f32x4{0.f, 0.f, 0.f, 0.f};

    // bias gradient (column sums of dY): formed by the waves of column block 0 that own the first 64 columns - every (row block, split) once
    const bool do_bias = BIAS && bx == 0 && wc == 0;  // (wave-uniform)
    f32x4 accb[BIAS ? TR : 1];
#pragma unroll
    for (int r = 0; r < (BIAS ? TR : 1); ++r) accb[r] = f32x4{0.f, 0.f, 0.f, 0.f};
    // NS-stage LDS ring, one raw barrier per K step, loads of NS-2 younger steps stay in flight (see igemm.hip); every wave issues NY + NX
    // pieces per step in both walks - the counted wait depends on it
    const int nk = (m_end - m_begin + WG_BK - 1) / WG_BK;
    constexpr int LPT = G::NY + G::NX;
#pragma unroll
    for (int s = 0; s < NS - 1; ++s)
        if (s < nk) walk.issue(smem + s * STAGE, m_begin + s * WG_BK);
    for (int kt = 0; kt < nk; ++kt) {
        if (kt + NS - 2 < nk) wait_vmcnt_barrier<LPT * (NS - 2)>();
        else wait_vmcnt_barrier<0>();
        if (kt + NS - 1 < nk) walk.issue(smem + ((kt + NS - 1) % NS) * STAGE, m_begin + (kt + NS - 1) * WG_BK);
        const char* Ys = smem + (kt % NS) * STAGE;
        WFrag<T>::template step<BM, TR, TC, BIAS>(Ys, Ys + G::YBYTES, wr * WM, wc * 64, lane, acc, do_bias, accb);
    }

    const int64_t slab_off = (int64_t)bz * a.CoutP * a.NG;
    const int row0 = co0 + wr * WM, col0 = j0 + wc * 64;  // of this wave's tile
    // The MFMA operands are swapped (A = the X fragment, B = the dY fragment), so a lane's four accumulator values are four
    // CONSECUTIVE (tap, ci) columns of one output channel: one 16-byte store instead of four 4-byte stores to four rows
    // (stores are issue-bound on this chip: 8 / 16 instructions per lane instead of 32 / 64).  NG is a multiple of 4.
    const int l15 = lane & 15, l4 = lane >> 4;
    if (BIAS && do_bias && l4 == 0) {  // every row of the ones product holds the same sums: lanes 0-15 write their output channel's
#pragma unroll
        for (int r = 0; r < (BIAS ? TR : 1); ++r) {
            const int co = row0 + r * 16 + l15;
            if (co < a.CoutP) a.bias_slab[(int64_t)bz * a.CoutP + co] = accb[r][0];
        }
    }
    if constexpr (std::is_same<T, bf16_t>::value) {  // bfloat16 slabs from 16 splits up (the launcher), float32 slabs below
        if (a.slab_bf16) wg_store_slab_staged<bf16_t>(smem, wave, lane, acc, reinterpret_cast<bf16_t*>(a.slab) + slab_off, row0, col0, a.CoutP, a.NG);
        else wg_store_slab_staged<float>(smem, wave, lane, acc, reinterpret_cast<float*>(a.slab) + slab_off, row0, col0, a.CoutP, a.NG);
    } else {  // f32 parity mode: float32 slabs straight from the accumulators
#pragma unroll
        for (int r = 0; r < TR; ++r) {
            const int co = row0 + r * 16 + l15;
#pragma unroll
            for (int c = 0; c < TC; ++c) {
                const int col = col0 + c * 16 + 4 * l4;
                if (co < a.CoutP && col < a.NG) *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(a.slab) + slab_off + (int64_t)co * a.NG + col) = acc[r][c];
            }
        }
    }
}

// ---- backward of a 1x1 stride-1 Conv block in one kernel: BatchNorm apply, data gradient and weight gradient --------------------------------------
// draw - the gradient of the block's raw convolution output - has exactly two readers, the data-gradient and the weight-gradient GEMM, and for a
// 1x1 stride-1 convolution each uses every element once.  This kernel forms draw on the operand path instead: a workgroup owns a pixel split and a
// 128-wide block of input channels and holds ALL output channels (BM = Cout = 64 or 128).  Per 32-pixel step its threads load dout and raw rows
// into registers, apply bn_bwd_apply_one (the apply pass's arithmetic, coefficients of the thread's channel group in registers), round to
// bfloat16 and store into the ring's dY image exactly where the LDS-DMA pieces of wgrad_kernel would have landed; X rows come in by LDS-DMA.  The
// image then feeds two products: dW += draw^T X (WFrag::step, accumulators in registers for the whole split, slab store and slab sum as wgrad_kernel's)
// and dx[32][128] = draw W, with W the data-gradient operand [Cin][Cout] held in registers as MFMA A fragments (the draw fragments are plain
// 16-byte reads of the same image), summed with up to two addends in float32, rounded once and stored as whole 256-byte row segments through LDS.
// draw never reaches HBM.  Column blocks beyond the first recompute draw from rows their XCD's L2 already holds (a split's tiles run back to back).
struct Conv1x1BwdArgs {
    WgradArgs w;  // x, slab, Mpix, CoutP (= BM), Cin (= NG), split and grid geometry; dy is unused
    const void* dout;
    const void* raw;
    int64_t ld_dout, ld_raw;
    const float* coef;  // [a0 | a1 | c0 | c1 | c2][Cout]
    const void* wd;     // data-gradient operand [Cin][Cout] bfloat16
    void* dx;
    const void* add1;
    const void* add2;
    int64_t ld_dx, ld_a1, ld_a2;
};
constexpr int C1_DROW = WG_BN * 4 + 16;  // a float32 row of the dx stage, padded
template <int BM> constexpr size_t conv1x1_bwd_lds_bytes() { return wgrad_lds_bytes<bf16_t, BM>() + (size_t)WG_BK * C1_DROW; }

// LDS accesses of the K loop as inline assembly, for WFrag's reason: the compiler puts `s_waitcnt vmcnt(0)` in front of LDS accesses that follow
// LDS-DMA pieces and would wait for the NEXT step's loads in every step.  The loop's own waits and barriers order them.
__device__ __forceinline__ u32x4 c1_lds_read16(const char* p) {
    u32x4 v;
    asm volatile("ds_read_b128 %0, %1" : "=v"(v) : "v"((uint32_t)(uintptr_t)(lptr_t)p));
    return v;
}
// (the value comes straight out of an MFMA: the compiler does not know that this statement is an LDS instruction reading it and leaves out the
// wait states an XDL result needs before a DS read - up to 19 for a 16-pass MFMA - so they are written here)
__device__ __forceinline__ void c1_lds_write16_mfma(char* p, f32x4 v) {
    asm volatile("s_nop 15\n\ts_nop 3\n\tds_write_b128 %0, %1" ::"v"((uint32_t)(uintptr_t)(lptr_t)p), "v"(v) : "memory");
}

template <int BM, int ACT>
__global__ __launch_bounds__(256, (BM == 128 ? 2 : 3)) void conv1x1_bwd_kernel(Conv1x1BwdArgs p) {
    using T = bf16_t;
    using G = WgTile<T, BM>;
    constexpr int NT = G::NT, TR = G::TR, TC = G::TC, WM = G::WM, STAGE = G::STAGE, NS = WG_NS, NY = G::NY, NX = G::NX;
    constexpr int RING = NS * STAGE;
    constexpr int KK = BM / 32;  // 32-deep steps of the data-gradient product's reduction over the output channels
    static_assert(G::YT == NT && WG_BK == 32 && NS == 2, "every thread owns NY chunks of the dY image; two stages");
    static_assert(RING >= (NT / 64) * SlabStage<bf16_t, TR>::BYTES && RING >= (NT / 64) * SlabStage<float, TR>::BYTES, "the staged slab stores use the ring");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* dxs = smem + RING;  // [32][C1_DROW]: a step's dx tile in float32

    const WgradArgs& a = p.w;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave / G::WCOLS, wc = wave % G::WCOLS;
    int bx, by, bz;
    if (!wg_tile_of_block(a, 0, bx, by, bz)) return;
    const int j0 = bx * WG_BN;
    const int m_begin = bz * a.pix_per_split;
    const int m_end = min(a.Mpix, m_begin + a.pix_per_split);
    const G ld(a, tid, j0, 0);

    // this thread's channel group of the dY image and its coefficients
    float k0[8], k1[8], k2[8], k3[8], k4[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const int c = ld.ych + r;
        k0[r] = p.coef[c];
        k1[r] = p.coef[BM + c];
        k2[r] = p.coef[2 * BM + c];
        k3[r] = p.coef[3 * BM + c];
        k4[r] = p.coef[4 * BM + c];
    }
    // W as A fragments: this wave's two 16-channel tiles of the column block; lane = (input channel, 8 consecutive output channels)
    bf16x8 wf[2][KK];
#pragma unroll
    for (int ct = 0; ct < 2; ++ct) {
        const int ci = j0 + (2 * wave + ct) * 16 + (lane & 15);
#pragma unroll
        for (int kk = 0; kk < KK; ++kk) {
            u32x4 v = {0u, 0u, 0u, 0u};
            if (ci < a.Cin) v = *reinterpret_cast<const u32x4*>(reinterpret_cast<const T*>(p.wd) + (int64_t)ci * BM + kk * 32 + (lane >> 4) * 8);
            wf[ct][kk] = __builtin_bit_cast(bf16x8, v);
        }
    }
    // The pixel order of the sum is wgrad_kernel's for the same tensors (pw_shift by the same host rule), so a split's partial - and with it the
    // rounded slab and dW - is bit for bit what the three launches give: row r of a step is pixel origin + r in raster order, and pixel
    // (r >> pw_shift, r & (pw - 1)) of a ph x pw patch in patch order (WgPatchWalk; stride 1 and one tap here: a pixel is one row of every
    // tensor).  Splits are whole patches in patch order, so only raster order meets rows beyond the split's end.
    const bool patch = a.pw_shift >= 0;  // (uniform)
    const int pw = patch ? 1 << a.pw_shift : WG_BK, ph = WG_BK / pw;
    auto row_off = [&](int row) { return patch ? (row >> a.pw_shift) * a.W + (row & (pw - 1)) : row; };
    struct { int m, wo, ho; } org, nxt;  // origin pixel of the current step and of the next (scalar)
    org.m = m_begin; org.wo = org.ho = 0;
    if (patch) {
        const int pidx = m_begin / WG_BK, npw = a.W >> a.pw_shift, nph = a.H / ph;
        const int t = pidx / npw, wp = pidx - t * npw;
        const int n = t / nph, hp = t - n * nph;
        org.wo = wp * pw; org.ho = hp * ph;
        org.m = (n * a.H + org.ho) * a.W + org.wo;
    }
    auto advance = [&](auto o) {
        if (!patch) { o.m += WG_BK; return o; }
        o.wo += pw; o.m += pw;
        if (o.wo == a.W) {
            o.wo = 0; o.ho += ph; o.m += (ph - 1) * a.W;
            if (o.ho == a.H) o.ho = 0;
        }
        return o;
    };
    // X pieces: row x_row(i) of the step, this thread's chunk; out-of-range lanes (padding columns, rows beyond the tensor) read zeros
    uint32_t xv[NX];
#pragma unroll
    for (int i = 0; i < NX; ++i) xv[i] = ld.x_cok ? (uint32_t)((row_off(ld.x_row(i)) * (int)a.ldx + ld.ci) * 2) : 0x80000000u;
    int yo[NY];  // pixel offsets of this thread's dY rows
#pragma unroll
    for (int i = 0; i < NY; ++i) yo[i] = row_off(ld.y_row(i));
    // the dx tile's store map: a thread owns 8 channels (chunk) of rows drow, drow + 16
    const int dch = tid & 15, drow = tid >> 4;
    const bool d_cok = j0 + dch * 8 < a.Cin;
    const int dro[2] = {row_off(drow), row_off(drow + 16)};

    f32x4 acc[TR][TC];
#pragma unroll
    for (int r = 0; r < TR; ++r)
#pragma unroll
        for (int c = 0; c < TC; ++c) acc[r][c] = f32x4{0.f, 0.f, 0.f, 0.f};
    f32x4 accb[1] = {f32x4{0.f, 0.f, 0.f, 0.f}};

    const int nk = (m_end - m_begin + WG_BK - 1) / WG_BK;
    u32x4 rd[NY], rr[NY];
    auto load_rows = [&](int mo) {  // dout / raw chunks of the step with origin mo (masked: rows beyond the split's end are not read)
#pragma unroll
        for (int i = 0; i < NY; ++i) {
            const int m = mo + yo[i];
            rd[i] = rr[i] = u32x4{0u, 0u, 0u, 0u};
            if (patch || m < m_end) {
                rd[i] = *reinterpret_cast<const u32x4*>(reinterpret_cast<const T*>(p.dout) + (int64_t)m * p.ld_dout + ld.ych);
                rr[i] = *reinterpret_cast<const u32x4*>(reinterpret_cast<const T*>(p.raw) + (int64_t)m * p.ld_raw + ld.ych);
            }
        }
    };
    auto issue_x = [&](int s, int mo) {
        char* Xs = smem + s * STAGE + G::YBYTES;
        const uint32_t soff = __builtin_amdgcn_readfirstlane((uint32_t)mo * (uint32_t)a.ldx * 2u);
#pragma unroll
        for (int i = 0; i < NX; ++i) wg_buffer_to_lds(a.x, a.x_bytes, G::x_slot(Xs, i, wave), xv[i], soff);
    };
    load_rows(org.m);
    issue_x(0, org.m);
    for (int kt = 0; kt < nk; ++kt, org = nxt) {
        const int mk = org.m;
        nxt = advance(org);
        char* Ys = smem + (kt & 1) * STAGE;
        // draw of this step from the rows in registers -> the dY image; rows beyond the split's end hold zeros (after the arithmetic: -c2 otherwise)
#pragma unroll
        for (int i = 0; i < NY; ++i) {
            const bf16x8 d = __builtin_bit_cast(bf16x8, rd[i]), x = __builtin_bit_cast(bf16x8, rr[i]);
            const bool ok = patch || mk + yo[i] < m_end;
            bf16x8 o;
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                const float v = bn_bwd_apply_one<ACT>((float)d[r], (float)x[r], k0[r], k1[r], k2[r], k3[r], k4[r]);
                o[r] = (bf16_t)(ok ? v : 0.0f);
            }
            *reinterpret_cast<bf16x8*>(Ys + (i * NT + tid) * 16) = o;
        }
        // the image and this step's X pieces are in LDS for every wave; every wave is through the previous step
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
        // loads of the next step fly under this step's products
        if (kt + 1 < nk) {
            issue_x((kt + 1) & 1, nxt.m);
            load_rows(nxt.m);
        }
        // product 1: dW += draw^T X
        WFrag<T>::template step<BM, TR, TC, false>(Ys, Ys + G::YBYTES, wr * WM, wc * 64, lane, acc, false, accb);
        // product 2: dx^T[ci][px] = W^T draw^T - operands swapped as in product 1, so a lane's four values are consecutive input channels of one pixel
#pragma unroll
        for (int pt = 0; pt < 2; ++pt) {  // 16 pixels at a time: the draw fragments of one half stay in registers
            u32x4 bq[KK];
            const int px = pt * 16 + (lane & 15);
            const int sw = tr_swz<tr_swz_mode(BM * 2)>(px) << 1;
#pragma unroll
            for (int kk = 0; kk < KK; ++kk) bq[kk] = c1_lds_read16(Ys + px * (BM * 2) + (((kk * 4 + (lane >> 4)) ^ sw) << 4));
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
            for (int kk = 0; kk < KK; ++kk) asm volatile("" : "+v"(bq[kk]));
#pragma unroll
            for (int ct = 0; ct < 2; ++ct) {
                f32x4 d = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int kk = 0; kk < KK; ++kk) d = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[ct][kk], __builtin_bit_cast(bf16x8, bq[kk]), d, 0, 0, 0);
                c1_lds_write16_mfma(dxs + px * C1_DROW + ((2 * wave + ct) * 16 + 4 * (lane >> 4)) * 4, d);
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        // the dx tile: + addends (read before the store: an addend may be dx itself), one rounding, whole row segments.  The addends are read
        // here, behind the next step's loads: held in registers across the products they cost the kernel a workgroup per CU.
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int row = drow + 16 * h, m = mk + dro[h];
            const bool ok = (patch || m < m_end) && d_cok;
            u32x4 ra[2] = {u32x4{0u, 0u, 0u, 0u}, u32x4{0u, 0u, 0u, 0u}};  // both addends of a row in flight together
            if (ok && p.add1) ra[0] = *reinterpret_cast<const u32x4*>(reinterpret_cast<const T*>(p.add1) + (int64_t)m * p.ld_a1 + j0 + dch * 8);
            if (ok && p.add2) ra[1] = *reinterpret_cast<const u32x4*>(reinterpret_cast<const T*>(p.add2) + (int64_t)m * p.ld_a2 + j0 + dch * 8);
            u32x4 lo = c1_lds_read16(dxs + row * C1_DROW + dch * 32), hi = c1_lds_read16(dxs + row * C1_DROW + dch * 32 + 16);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            asm volatile("" : "+v"(lo), "+v"(hi));
            const f32x4 flo = __builtin_bit_cast(f32x4, lo), fhi = __builtin_bit_cast(f32x4, hi);
            float v[8] = {flo[0], flo[1], flo[2], flo[3], fhi[0], fhi[1], fhi[2], fhi[3]};
#pragma unroll
            for (int q = 0; q < 2; ++q) {  // (a missing addend is zeros: x + 0 is x)
                const bf16x8 t = __builtin_bit_cast(bf16x8, ra[q]);
#pragma unroll
                for (int r = 0; r < 8; ++r) v[r] += (float)t[r];
            }
            if (ok) Pack<T, 8>::store(reinterpret_cast<T*>(p.dx) + (int64_t)m * p.ld_dx + j0 + dch * 8, v);
        }
    }

    const int64_t slab_off = (int64_t)bz * a.CoutP * a.NG;
    const int row0 = wr * WM, col0 = j0 + wc * 64;
    if (a.slab_bf16) wg_store_slab_staged<bf16_t>(smem, wave, lane, acc, reinterpret_cast<bf16_t*>(a.slab) + slab_off, row0, col0, a.CoutP, a.NG);
    else wg_store_slab_staged<float>(smem, wave, lane, acc, reinterpret_cast<float*>(a.slab) + slab_off, row0, col0, a.CoutP, a.NG);
}

// ---- the slab sums -----------------------------------------------------------------------------------------------------------------------------
// the sum of the `splits` values p[e], p[e + stride], ... in a fixed order (deterministic): four independent chains keep the split loads in flight,
// the tail goes into chain 0, combined as (s0 + s1) + (s2 + s3)
template <typename S> __device__ __forceinline__ float wg_split_sum(const S* __restrict__ p, int64_t e, int64_t stride, int splits) {
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    int k = 0;
    for (; k + 3 < splits; k += 4) {
        s0 += (float)p[e + (int64_t)k * stride];
        s1 += (float)p[e + (int64_t)(k + 1) * stride];
        s2 += (float)p[e + (int64_t)(k + 2) * stride];
        s3 += (float)p[e + (int64_t)(k + 3) * stride];
    }
    for (; k < splits; ++k) s0 += (float)p[e + (int64_t)k * stride];
    return (s0 + s1) + (s2 + s3);
}

// Per-layer slab reduction (ymi_conv2d_bwd_weight, the non-deferred entry point): one thread per output element, coalesced along (tap, ci).
// dw[co][ci][kh][kw] = sum_s slab[s][co][tap*Cin + ci]  (scatter into OIHW).  BF: bfloat16 slabs, else float32.
template <bool BF>
__global__ void wgrad_reduce_kernel(const void* __restrict__ slab, int splits, int CoutP, int NG, int Cin, int cout_real, int cin_real, int ntaps,
                                    float* __restrict__ dw) {
    typedef typename std::conditional<BF, bf16_t, float>::type S;
    // 32-bit index arithmetic (a weight tensor has < 2^31 elements)
    const uint32_t total = (uint32_t)cout_real * (uint32_t)ntaps * (uint32_t)cin_real;
    const int64_t sstride = (int64_t)CoutP * NG;
    for (uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += gridDim.x * blockDim.x) {
        const uint32_t t = idx / (uint32_t)cin_real;
        const uint32_t ci = idx - t * (uint32_t)cin_real;
        const uint32_t co = t / (uint32_t)ntaps;
        const uint32_t tap = t - co * (uint32_t)ntaps;
        const int64_t e = (int64_t)co * NG + tap * Cin + ci;
        dw[((int64_t)co * cin_real + ci) * ntaps + tap] = wg_split_sum(reinterpret_cast<const S*>(slab), e, sstride, splits);
    }
}

// dbias[co] = sum over the splits of the bias partials [split][coutp]
__device__ __forceinline__ void bias_slab_sum(const float* __restrict__ bs, int splits, int coutp, float* __restrict__ db, int tid, int nthr) {
    for (int co = tid; co < coutp; co += nthr) db[co] = wg_split_sum(bs, co, coutp, splits);
}
__global__ void wgrad_bias_reduce_kernel(const float* __restrict__ bs, int splits, int coutp, float* __restrict__ db) {
    bias_slab_sum(bs, splits, coutp, db, (int)(blockIdx.x * blockDim.x + threadIdx.x), (int)(gridDim.x * blockDim.x));
}
// All pending slab reductions of a backward pass in ONE launch (ymi_wgrad_reduce_batch): a 256-thread workgroup finds its
// tensor by binary search over the table's first_block column, then sums `lanes` interleaved split chains per output
// element in a fixed order (deterministic) and scatters into OIHW.  By the end of the backward pass the slabs have left the
// caches: this kernel streams them from HBM, 4 elements per lane and load, four split chains in flight per lane.
template <bool BF> __device__ __forceinline__ void reduce_batch_body(const ymi_wgrad_pending& e, f32x4* red) {
    // the record's first workgroup also sums the bias partials (a few KB)
    if (e.bias_slab && (int)blockIdx.x == e.first_block) bias_slab_sum(e.bias_slab, e.splits, (int)(e.elems / e.ng), e.dbias, (int)threadIdx.x, 256);
    // a lane owns EPT consecutive elements: 8 (one 16-byte load per split) of a bfloat16 slab, 4 of a float32 slab
    constexpr int EPT = BF ? 8 : 4, Q = EPT / 4;
    const int SL = e.lanes, OUTS = 256 / SL;              // OUTS groups of EPT consecutive elements per workgroup
    const int ol = threadIdx.x % OUTS, lane = threadIdx.x / OUTS;
    const int64_t el = ((int64_t)((int)blockIdx.x - e.first_block) * OUTS + ol) * EPT;  // first element of this lane's group
    f32x4 s0[Q], s1[Q], s2[Q], s3[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) s0[q] = s1[q] = s2[q] = s3[q] = f32x4{0.f, 0.f, 0.f, 0.f};
    auto add_split = [&](f32x4 (&acc)[Q], int k) {
        const int64_t off = el + (int64_t)k * e.elems;
        if constexpr (BF) {
            const bf16x8 v = *reinterpret_cast<const bf16x8*>(reinterpret_cast<const bf16_t*>(e.slab) + off);
            acc[0] += f32x4{(float)v[0], (float)v[1], (float)v[2], (float)v[3]};
            acc[1] += f32x4{(float)v[4], (float)v[5], (float)v[6], (float)v[7]};
        } else {
            acc[0] += *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(e.slab) + off);
        }
    };
    if (el < e.elems) {  // elems is a multiple of 8
        int k = lane;
        for (; k + 3 * SL < e.splits; k += 4 * SL) {  // four split chains in flight per lane
            add_split(s0, k);
            add_split(s1, k + SL);
            add_split(s2, k + 2 * SL);
            add_split(s3, k + 3 * SL);
        }
        for (; k < e.splits; k += SL) add_split(s0, k);
    }
#pragma unroll
    for (int q = 0; q < Q; ++q) red[(q * SL + lane) * OUTS + ol] = (s0[q] + s1[q]) + (s2[q] + s3[q]);
    __syncthreads();
    if (lane == 0 && el < e.elems) {
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            f32x4 s = {0.f, 0.f, 0.f, 0.f};
            for (int c = 0; c < SL; ++c) s += red[(q * SL + c) * OUTS + ol];
            const uint32_t eu = (uint32_t)el + 4u * q;  // < 2^31; 4 elements share (co, tap): ng and cin are multiples of 4
            const int co = (int)(eu / (uint32_t)e.ng), col = (int)(eu - (uint32_t)co * (uint32_t)e.ng);
            const int tap = (int)((uint32_t)col / (uint32_t)e.cin), ci = col - tap * e.cin;
            if (co < e.cout_real) {
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (ci + r < e.cin_real) e.dw[((int64_t)co * e.cin_real + ci + r) * e.ntaps + tap] = s[r];
            }
        }
    }
}
__global__ __launch_bounds__(256) void wgrad_reduce_batch_kernel(const ymi_wgrad_pending* __restrict__ tab, int n) {
    __shared__ f32x4 red[512];
    int lo = 0, hi = n - 1;  // last entry whose first_block <= blockIdx.x
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (tab[mid].first_block <= (int)blockIdx.x) lo = mid;
        else hi = mid - 1;
    }
    const ymi_wgrad_pending e = tab[lo];
    if (e.slab_bf16) reduce_batch_body<true>(e, red);  // (workgroup-uniform)
    else reduce_batch_body<false>(e, red);
}

// magic numbers for wg_fast_div
static void wg_find_divisor(int d, uint32_t* mul, uint32_t* shr) {
    int lg = 0;
    while ((1 << lg) < d) ++lg;
    *mul = (uint32_t)((((uint64_t)1 << 32) * (((uint64_t)1 << lg) - (uint64_t)d)) / (uint64_t)d + 1);
    *shr = (uint32_t)lg;
}

struct WgradPlan {
    int splits, pix_per_split;
    size_t slab_bytes;
};
// row-tile choice.  Measured: with the same workgroup target as the 64-row tile the 128-row tile is 5-45 % SLOWER (the
// pixel axis is split twice as often, doubling the slab traffic); with HALF the workgroups (same split count, 16 MFMAs
// per wave and K step) it is 7-12 % faster on every layer with >= 128 output channels.
static int wgrad_bm(int64_t coutp, bool bf16) {
    if (!bf16) return 64;
    if (coutp <= 32) return 32;
    return (coutp >= 128 && coutp % 128 == 0) || coutp >= 256 ? 128 : 64;
}
static WgradPlan wgrad_plan(int64_t mpix, int64_t coutp, int64_t ng, int bm, size_t slab_esize) {
    const int64_t tiles = ((ng + WG_BN - 1) / WG_BN) * ((coutp + bm - 1) / bm);
    // workgroups to aim for (tuning knobs; the in-situ optimum differs from the isolated one: see profiles/r03_wgrad_targets.txt).
    // Swept inside the step (profiles/r04_wgrad_targets_sweep.txt): ONE RESIDENT ROUND - 5 workgroups per CU for the 64-row tile
    // (its launch bounds), 3 for the 128-row tile - is 0.09 ms/step faster than 1024 / 640; a fourth 128-row workgroup per CU costs 0.3 ms
    const int target64 = ymi_opt(OPT_WGRAD_BLOCKS);
    const int target128 = ymi_opt(OPT_WGRAD_BLOCKS128);
    const int target = bm == 128 ? target128 : target64;
    int64_t s = (target + tiles - 1) / tiles;
    const int64_t smax = (mpix + 255) / 256;
    if (s > smax) s = smax;
    if (s < 1) s = 1;
    if (s >= 8) s = (s + 7) / 8 * 8 <= smax ? (s + 7) / 8 * 8 : s / 8 * 8;  // splits are dealt to the 8 XCDs (see the kernel): keep them balanced
    int64_t pps = (mpix + s - 1) / s;
    pps = (pps + WG_BK - 1) / WG_BK * WG_BK;
    s = (mpix + pps - 1) / pps;
    WgradPlan p;
    p.splits = (int)s;
    p.pix_per_split = (int)pps;
    p.slab_bytes = ((size_t)s * coutp * ng * slab_esize + 255) / 256 * 256;
    return p;
}

static int64_t pad_to(int64_t v, int64_t m) { return (v + m - 1) / m * m; }
// rows [padded Cout] of bias partials the workspace has room for behind the slabs: a launch with a bias gradient has at most that many splits
constexpr int64_t WG_BIAS_ROWS = 2048 * 2 + 1;

extern "C" size_t ymi_conv2d_bwd_weight_workspace(int64_t m_rows, int64_t cout, int64_t cin, int64_t kh, int64_t kw) {
    // upper bound over both dtypes' channel padding (8), plus room for the bias-gradient partials
    const int64_t coutp = pad_to(cout, 8), cinp = pad_to(cin, 8);
    WgradPlan p = wgrad_plan(m_rows, coutp, kh * kw * cinp, 64, 4);  // (float32 slabs: the larger of the two dtypes' needs)
    const WgradPlan p128 = wgrad_plan(m_rows, coutp, kh * kw * cinp, 128, 4);  // the 128-row tile splits the pixel axis further
    if (p128.slab_bytes > p.slab_bytes) p = p128;
    return p.slab_bytes + (size_t)WG_BIAS_ROWS * coutp * sizeof(float) + 256;
}

static int wgrad_impl(const ymi_tensor* x, const ymi_tensor* dy, int64_t cout_real, int64_t cin_real, int64_t kh, int64_t kw, int64_t stride,
                      float* dw_oihw, float* dbias, void* workspace, size_t workspace_bytes, ymi_wgrad_pending* pending, void* stream);
static int wgrad_slab_sum(const WgradArgs& a, int64_t cout_real, int64_t cin_real, int64_t ntaps, float* dw_oihw, float* dbias, ymi_wgrad_pending* pending,
                          hipStream_t s);
// the patch order of the pixel sum for these operands (bfloat16, the operands as buffers below 2^31 bytes, whole 32-pixel steps): log2 of the widest
// power-of-two patch width that divides Wo with a height that divides Ho; -1: raster order.  ONE rule: every kernel that sums these pixels uses it.
static int wgrad_patch_shift(const ymi_tensor* x, const ymi_tensor* dy) {
    const int64_t xb = ymi_pixels(x) * x->ld * ymi_esize(x->dtype), yb = ymi_pixels(dy) * dy->ld * ymi_esize(dy->dtype);
    const int64_t margin = (x->w + 2) * x->ld * (int64_t)ymi_esize(x->dtype);
    if (!(x->dtype == YMI_BF16 && ymi_opt(OPT_WGRAD_PATCH) && xb + margin < (1ll << 31) && yb < (1ll << 31) && ymi_pixels(dy) % WG_BK == 0)) return -1;
    for (int sh = 5; sh >= 0; --sh) {
        const int pw = 1 << sh, ph = WG_BK >> sh;
        if (dy->w % pw == 0 && dy->h % ph == 0) return sh;
    }
    return -1;
}

// ---- a launch, possibly held back (common.h: BnRider) ------------------------------------------------------------------------------------
struct WgradLaunch {
    WgradArgs a;
    dim3 grid;
    int bm;
    bool bf16;
    hipStream_t s;
    double flop, bytes;
};
// one row tile: the BIAS instantiation where the launch forms the bias partials, the PATCH one where the map tiles into patches (bfloat16 only:
// parity mode keeps the raster walk, pw_shift is -1 for float32 operands)
// (the ring is at most 48 KB: no launch needs the opt-in for more than 64 KB of dynamic LDS)
template <typename T, int BM> static void wgrad_launch_tile(const WgradArgs& a, const BnRider& r, dim3 grid, hipStream_t s) {
    constexpr size_t lds = wgrad_lds_bytes<T, BM>();
    static_assert(lds <= 64 * 1024, "a larger ring needs hipFuncAttributeMaxDynamicSharedMemorySize");
    void (*kernel)(WgradArgs, BnRider) = a.bias_slab ? wgrad_kernel<T, BM, true, false> : wgrad_kernel<T, BM, false, false>;
    if constexpr (std::is_same<T, bf16_t>::value) {
        if (a.pw_shift >= 0) kernel = a.bias_slab ? wgrad_kernel<T, BM, true, true> : wgrad_kernel<T, BM, false, true>;
    }
    hipLaunchKernelGGL(kernel, grid, dim3(256), lds, s, a, r);
}
static void wgrad_launch(const WgradLaunch& h, const BnFinal* rider) {
    BnRider r{};
    dim3 grid = h.grid;
    if (rider && h.a.xcd_map) {  // rider workgroups at the front of the 1-D grid
        r.f = *rider;
        r.nwg = ((rider->C + 31) / 32 + 7) / 8 * 8;
        grid.x += (unsigned)r.nwg;
    }
    int prof = -1;
    if (ymi_prof_enabled()) prof = ymi_prof_start(h.s, 1, h.flop, h.bytes, h.bf16 ? 2500.0 : 157.3);
    if (!h.bf16) wgrad_launch_tile<float, 64>(h.a, r, grid, h.s);  // (wgrad_bm: parity mode has the 64-row tile only)
    else if (h.bm == 128) wgrad_launch_tile<bf16_t, 128>(h.a, r, grid, h.s);
    else if (h.bm == 32) wgrad_launch_tile<bf16_t, 32>(h.a, r, grid, h.s);
    else wgrad_launch_tile<bf16_t, 64>(h.a, r, grid, h.s);
    ymi_prof_stop(h.s, prof);
}
// The held launch (ymi_wgrad_hold): at most one, always a deferred one with the 1-D XCD-mapped grid a rider can join, remembered with the device that
// was current when it was held - it is issued there, whoever's call issues it.
static struct WgradHeld {
    std::mutex mu;
    bool on = false;     // mode 1: deferred launches are held
    bool valid = false;  // `launch` is waiting
    WgradLaunch launch;
    int device = 0;
} g_held;
static int wgrad_current_device() {
    int d = 0;
    (void)hipGetDevice(&d);
    return d;
}
// (g_held.mu taken) issue the held launch, if any, on its device; the caller's device is current again afterwards
static void wgrad_flush_held_locked(const BnFinal* rider = nullptr) {
    if (!g_held.valid) return;
    g_held.valid = false;
    const int cur = wgrad_current_device();
    if (cur != g_held.device) (void)hipSetDevice(g_held.device);
    wgrad_launch(g_held.launch, rider);
    if (cur != g_held.device) (void)hipSetDevice(cur);
}
bool ymi_wgrad_issue_held(const BnFinal* f, hipStream_t stream) {
    std::lock_guard<std::mutex> lk(g_held.mu);
    if (!g_held.valid || g_held.launch.s != stream || g_held.device != wgrad_current_device()) return false;
    wgrad_flush_held_locked(f);
    return true;
}
// mode 1: hold deferred weight-gradient launches for riders; 0: stop holding (a held launch is issued as it is); 2: forget a held launch (after a
// backward pass that raised: its operands are gone), the mode stays
extern "C" int ymi_wgrad_hold(int32_t mode) {
    std::lock_guard<std::mutex> lk(g_held.mu);
    if (mode == 2) {
        g_held.valid = false;
        return YMI_OK;
    }
    YMI_CHECK_ARG(mode == 0 || mode == 1, "wgrad_hold: mode 0, 1 or 2");
    if (mode == 0) wgrad_flush_held_locked();
    g_held.on = mode == 1;
    return hipGetLastError() == hipSuccess ? YMI_OK : YMI_ELAUNCH;
}

extern "C" int ymi_conv2d_bwd_weight(const ymi_tensor* x, const ymi_tensor* dy, int64_t cout_real, int64_t cin_real, int64_t kh, int64_t kw,
                                     int64_t stride, float* dw_oihw, float* dbias, void* workspace, size_t workspace_bytes, void* stream) {
    return wgrad_impl(x, dy, cout_real, cin_real, kh, kw, stride, dw_oihw, dbias, workspace, workspace_bytes, nullptr, stream);
}

extern "C" int ymi_conv2d_bwd_weight_deferred(const ymi_tensor* x, const ymi_tensor* dy, int64_t cout_real, int64_t cin_real, int64_t kh, int64_t kw,
                                              int64_t stride, float* dw_oihw, float* dbias, void* workspace, size_t workspace_bytes,
                                              ymi_wgrad_pending* pending, void* stream) {
    YMI_CHECK_ARG(pending, "conv2d_bwd_weight_deferred: null pending record");
    return wgrad_impl(x, dy, cout_real, cin_real, kh, kw, stride, dw_oihw, dbias, workspace, workspace_bytes, pending, stream);
}

ymi_wgrad_pending ymi_wgrad_record(const void* slab, float* dw, int64_t elems, int splits, int ng, int cin, int cout_real, int cin_real, int ntaps,
                                   bool slab_bf16, const float* bias_slab, float* dbias) {
    const int lanes = splits > 128 ? 32 : splits > 32 ? 16 : splits > 8 ? 8 : 4;
    const int outs = 256 / lanes, ept = slab_bf16 ? 8 : 4;  // a workgroup sums `outs` groups of `ept` consecutive elements
    return ymi_wgrad_pending{slab, dw, elems, splits, ng, cin, cout_real, cin_real, ntaps, lanes, 0, (int32_t)((elems / ept + outs - 1) / outs), slab_bf16 ? 1 : 0,
                             bias_slab, dbias};
}

// the records travel to the device table in kernel ARGUMENTS (by value): no host staging buffer, so the launches are
// graph-capturable (a captured host-to-device copy would re-read its host buffer at replay time)
constexpr int WG_TABLE_CHUNK = 48;  // 48 x 80 B = 3.75 KB of kernel arguments
static_assert(sizeof(ymi_wgrad_pending) == 80, "ymi_wgrad_pending layout (mirrored in _lib.py)");
struct WgradTableChunk {
    ymi_wgrad_pending e[WG_TABLE_CHUNK];
};
__global__ void wgrad_table_write_kernel(WgradTableChunk c, int n, ymi_wgrad_pending* __restrict__ table) {
    const int i = threadIdx.x;
    if (i < n) table[i] = c.e[i];
}

extern "C" int ymi_wgrad_reduce_batch(const ymi_wgrad_pending* host_records, int32_t n, ymi_wgrad_pending* device_table, void* stream) {
    YMI_CHECK_ARG(host_records && device_table && n > 0, "wgrad_reduce_batch: args");
    hipStream_t s = (hipStream_t)stream;
    {   // a launch still held back for a rider (ymi_wgrad_hold): its slabs are summed below
        std::lock_guard<std::mutex> lk(g_held.mu);
        wgrad_flush_held_locked();
    }
    int64_t total = 0;
    for (int base = 0; base < n; base += WG_TABLE_CHUNK) {
        WgradTableChunk c{};
        const int m = n - base < WG_TABLE_CHUNK ? n - base : WG_TABLE_CHUNK;
        for (int i = 0; i < m; ++i) {
            c.e[i] = host_records[base + i];
            YMI_CHECK_ARG(c.e[i].slab && c.e[i].dw && c.e[i].blocks > 0 && (c.e[i].lanes == 4 || c.e[i].lanes == 8 || c.e[i].lanes == 16 || c.e[i].lanes == 32),
                          "wgrad_reduce_batch: record %d", base + i);
            c.e[i].first_block = (int32_t)total;
            total += c.e[i].blocks;
        }
        hipLaunchKernelGGL(wgrad_table_write_kernel, dim3(1), dim3(64), 0, s, c, m, device_table + base);
    }
    YMI_CHECK_ARG(total < (1ll << 31), "wgrad_reduce_batch: too many workgroups");
    hipLaunchKernelGGL(wgrad_reduce_batch_kernel, dim3((unsigned)total), dim3(256), 0, s, (const ymi_wgrad_pending*)device_table, (int)n);
    YMI_CHECK_LAUNCH("wgrad_reduce_batch");
    return YMI_OK;
}

static int wgrad_impl(const ymi_tensor* x, const ymi_tensor* dy, int64_t cout_real, int64_t cin_real, int64_t kh, int64_t kw, int64_t stride,
                      float* dw_oihw, float* dbias, void* workspace, size_t workspace_bytes, ymi_wgrad_pending* pending, void* stream) {
    YMI_CHECK_ARG(ymi_tensor_ok(x) && ymi_tensor_ok(dy) && dw_oihw && workspace, "conv2d_bwd_weight: bad argument");
    YMI_CHECK_ARG(x->dtype == dy->dtype, "conv2d_bwd_weight: dtype mismatch");
    const int ch = x->dtype == YMI_BF16 ? 8 : 4;
    YMI_CHECK_ARG(x->c % ch == 0 && x->ld % ch == 0 && dy->c % ch == 0 && dy->ld % ch == 0, "conv2d_bwd_weight: channels must be multiples of %d", ch);
    YMI_CHECK_ARG(kh == kw && (kh == 1 || kh == 3) && (stride == 1 || stride == 2), "conv2d_bwd_weight: k in {1,3}, stride in {1,2}");
    const int64_t pad = kh / 2;
    YMI_CHECK_ARG(dy->n == x->n && dy->h == (x->h + 2 * pad - kh) / stride + 1 && dy->w == (x->w + 2 * pad - kw) / stride + 1, "conv2d_bwd_weight: shapes");
    YMI_CHECK_ARG(cout_real <= dy->c && cin_real <= x->c, "conv2d_bwd_weight: real channel counts");
    YMI_CHECK_ARG(ymi_pixels(x) * x->ld < (1ll << 31) && ymi_pixels(dy) * dy->ld < (1ll << 31), "conv2d_bwd_weight: too large");
    const int64_t mpix = ymi_pixels(dy);
    const int64_t ng = kh * kw * x->c;
    const bool bf16 = x->dtype == YMI_BF16;
    const int bm = wgrad_bm(dy->c, bf16), bn = WG_BN;
    WgradPlan p = wgrad_plan(mpix, dy->c, ng, bm, bf16 ? 2 : 4);
    // bfloat16 first-level slabs only where there are many of them: a handful of rounded partials, each covering a large part of the pixel
    // sum, put 1.7e-3 on dW (the 20 x 20 maps at small batch, tests/test_gpu_bf16_matched.py); from 16 splits up the roundings average
    // out (<= 2e-3 asserted at the bs-32 shapes), and launches with few splits write little slab traffic to save anyway
    const bool slab_bf16 = bf16 && p.splits >= 16;
    if (bf16 && !slab_bf16) p = wgrad_plan(mpix, dy->c, ng, bm, 4);
    size_t need = p.slab_bytes + (dbias ? (size_t)WG_BIAS_ROWS * dy->c * sizeof(float) : 0);
    if (workspace_bytes < need) {
        ymi_set_error("conv2d_bwd_weight: workspace %zu < %zu bytes", workspace_bytes, need);
        return YMI_EWORKSPACE;
    }
    WgradArgs a{};
    a.x = x->data; a.dy = dy->data; a.slab = workspace; a.slab_bf16 = slab_bf16 ? 1 : 0; a.zero = ymi_zero_page();
    // bias gradient: per-split column sums of dY come out of the GEMM itself (a ones row against the dY fragments), behind the slabs
    a.bias_slab = dbias ? reinterpret_cast<float*>(reinterpret_cast<char*>(workspace) + p.slab_bytes) : nullptr;
    YMI_CHECK_ARG(!dbias || p.splits <= WG_BIAS_ROWS, "conv2d_bwd_weight: too many splits for the bias partials");
    a.ldx = x->ld; a.ldy = dy->ld;
    a.Mpix = (int)mpix; a.H = (int)x->h; a.W = (int)x->w; a.Ho = (int)dy->h; a.Wo = (int)dy->w;
    a.stride = (int)stride; a.pad = (int)pad; a.KW = (int)kw;
    a.CoutP = (int)dy->c; a.Cin = (int)x->c; a.NG = (int)ng; a.pix_per_split = p.pix_per_split;
    wg_find_divisor(a.Wo, &a.wo_mul, &a.wo_shr);
    wg_find_divisor(a.Ho, &a.ho_mul, &a.ho_shr);
    a.nx = (int)((ng + bn - 1) / bn); a.ny = (int)((dy->c + bm - 1) / bm); a.splits = p.splits;
    // patch order of the pixel sum (see wgrad_kernel): the widest power-of-two patch width that divides Wo with a height that divides Ho
    a.pw_shift = wgrad_patch_shift(x, dy);
    if (a.pw_shift >= 0) {
        a.x_bytes = (uint32_t)(ymi_pixels(x) * x->ld * ymi_esize(x->dtype));
        a.y_bytes = (uint32_t)(ymi_pixels(dy) * dy->ld * ymi_esize(dy->dtype));
    }
    a.xcd_map = p.splits >= 8 ? 1 : 0;  // (all tiles of a pixel split on one XCD: 275 -> 105 MB of HBM reads per launch)
    dim3 grid((unsigned)a.nx, (unsigned)a.ny, (unsigned)p.splits);
    if (a.xcd_map) grid = dim3((unsigned)(8 * ((p.splits + 7) / 8) * a.nx * a.ny), 1, 1);
    hipStream_t s = (hipStream_t)stream;
    const double es = (double)ymi_esize(x->dtype);
    WgradLaunch h{a, grid, bm, bf16, s, 2.0 * (double)mpix * (double)dy->c * (double)ng,
                  ((double)ymi_pixels(x) * x->c + (double)mpix * dy->c) * es + (double)dy->c * ng * 4.0};
    {
        std::lock_guard<std::mutex> lk(g_held.mu);
        wgrad_flush_held_locked();  // (at most one launch is held)
        if (pending && g_held.on && a.xcd_map) {
            // held back: the next BatchNorm backward of this stream issues it with its final pass riding along (or the next deferred call / the
            // batched slab sum / ymi_wgrad_hold(0) as it is).  The caller keeps operands and workspace alive until the slab sum anyway.
            g_held.launch = h;
            g_held.device = wgrad_current_device();
            g_held.valid = true;
        } else {
            wgrad_launch(h, nullptr);
        }
    }
    YMI_CHECK_LAUNCH("wgrad");
    return wgrad_slab_sum(a, cout_real, cin_real, kh * kw, dw_oihw, dbias, pending, s);
}

// what follows a launch that wrote the slabs of `a`: the record of the batched sum, or the per-launch sums
static int wgrad_slab_sum(const WgradArgs& a, int64_t cout_real, int64_t cin_real, int64_t ntaps, float* dw_oihw, float* dbias, ymi_wgrad_pending* pending,
                          hipStream_t s) {
    if (pending) {  // the slab sum is left to ymi_wgrad_reduce_batch (one launch for every layer of the backward pass)
        *pending = ymi_wgrad_record(a.slab, dw_oihw, (int64_t)a.CoutP * a.NG, a.splits, a.NG, a.Cin, (int)cout_real, (int)cin_real, (int)ntaps, a.slab_bf16 != 0,
                                    a.bias_slab, dbias);
    } else {
        const int64_t total = cout_real * ntaps * cin_real;
        int64_t gb = (total + 255) / 256;
        if (gb > 2048) gb = 2048;
        hipLaunchKernelGGL(a.slab_bf16 ? wgrad_reduce_kernel<true> : wgrad_reduce_kernel<false>, dim3((unsigned)gb), dim3(256), 0, s, (const void*)a.slab, a.splits,
                           a.CoutP, a.NG, a.Cin, (int)cout_real, (int)cin_real, (int)ntaps, dw_oihw);
    }
    YMI_CHECK_LAUNCH("wgrad_reduce");
    if (dbias && !pending) {
        // bias gradient: the sum of the per-split column sums, written straight into the caller's buffer of CoutP floats (the real channels come first)
        hipLaunchKernelGGL(wgrad_bias_reduce_kernel, dim3((unsigned)((a.CoutP + 255) / 256)), dim3(256), 0, s, (const float*)a.bias_slab, a.splits, a.CoutP, dbias);
        YMI_CHECK_LAUNCH("wgrad_bias_reduce");
    }
    return YMI_OK;
}

// ---- the fused backward of a 1x1 stride-1 Conv block (conv1x1_bwd_kernel) ------------------------------------------------------------------------
// scope: bfloat16, Cout in {64, 128} dense in dout / raw (they may be channel slices), Cin a multiple of 8 up to 512 = x's and dx's channels
static bool conv1x1_bwd_scope(const ymi_tensor* dout, const ymi_tensor* raw, const ymi_tensor* x, const ymi_tensor* add1, const ymi_tensor* add2,
                              const ymi_tensor* dx) {
    if (!(ymi_tensor_ok(dout) && ymi_tensor_ok(raw) && ymi_tensor_ok(x) && ymi_tensor_ok(dx))) return false;
    if (add2 && !add1) return false;
    const ymi_tensor* all[6] = {dout, raw, x, dx, add1, add2};
    for (const ymi_tensor* t : all)
        if (t && !(ymi_tensor_ok(t) && t->dtype == YMI_BF16 && t->c % 8 == 0 && t->ld % 8 == 0 && (uintptr_t)t->data % 16 == 0 && ymi_pixels(t) * t->ld < (1ll << 30))) return false;
    if (!(ymi_same_shape(dout, raw) && (dout->c == 64 || dout->c == 128))) return false;
    if (!(x->n == dout->n && x->h == dout->h && x->w == dout->w && x->c <= 512 && ymi_same_shape(x, dx))) return false;
    return (!add1 || ymi_same_shape(add1, dx)) && (!add2 || ymi_same_shape(add2, dx));
}
extern "C" int ymi_conv1x1_bn_act_bwd_ok(const ymi_tensor* dout, const ymi_tensor* raw, const ymi_tensor* x, const ymi_tensor* add1, const ymi_tensor* add2,
                                         const ymi_tensor* dx) {
    return conv1x1_bwd_scope(dout, raw, x, add1, add2, dx) ? 1 : 0;
}
extern "C" size_t ymi_conv1x1_bn_act_bwd_workspace(int64_t m_rows, int64_t cout, int64_t cin) {
    const int rblocks = 2048;  // (an upper bound of the reduce pass's rows, as ymi_bn_act_bwd's callers size it)
    const size_t bn = (((size_t)rblocks * 2 * cout + 6 * (size_t)cout) * sizeof(float) + 64 * (size_t)cout * sizeof(double) + 255) / 256 * 256;
    return bn + ymi_conv2d_bwd_weight_workspace(m_rows, cout, cin, 1, 1);
}
extern "C" int ymi_conv1x1_bn_act_bwd(const ymi_tensor* dout, const ymi_tensor* raw, const float* gamma, const float* save_mean, const float* save_invstd,
                                      const float* beta, int32_t act, const ymi_tensor* x, const void* w_dgrad_packed, const ymi_tensor* add1,
                                      const ymi_tensor* add2, const ymi_tensor* dx, float* dgamma, float* dbeta, float* dw_oihw, void* workspace,
                                      size_t workspace_bytes, ymi_wgrad_pending* pending, void* stream) {
    YMI_CHECK_ARG(conv1x1_bwd_scope(dout, raw, x, add1, add2, dx), "conv1x1_bn_act_bwd: outside the fused kernel's scope (ymi_conv1x1_bn_act_bwd_ok)");
    YMI_CHECK_ARG(w_dgrad_packed && (uintptr_t)w_dgrad_packed % 16 == 0 && dw_oihw && workspace, "conv1x1_bn_act_bwd: bad argument");
    const int64_t mpix = ymi_pixels(dout);
    const int bm = (int)dout->c, cin = (int)x->c;
    const size_t need = ymi_conv1x1_bn_act_bwd_workspace(mpix, bm, cin);
    if (workspace_bytes < need) {
        ymi_set_error("conv1x1_bn_act_bwd: workspace %zu < %zu bytes", workspace_bytes, need);
        return YMI_EWORKSPACE;
    }
    hipStream_t s = (hipStream_t)stream;
    const size_t bn_bytes = need - ymi_conv2d_bwd_weight_workspace(mpix, bm, cin, 1, 1);
    const float* coef = nullptr;
    int rc = ymi_bn_act_bwd_coef(dout, raw, gamma, save_mean, save_invstd, beta, GammaBeta2{nullptr, nullptr, 0}, act, dgamma, dbeta, workspace, bn_bytes, s, &coef);
    if (rc) return rc;
    WgradPlan p = wgrad_plan(mpix, bm, cin, bm, 2);
    const bool slab_bf16 = p.splits >= 16;  // (wgrad_impl's rule)
    if (!slab_bf16) p = wgrad_plan(mpix, bm, cin, bm, 4);
    Conv1x1BwdArgs k{};
    WgradArgs& a = k.w;
    a.x = x->data; a.slab = reinterpret_cast<char*>(workspace) + bn_bytes; a.slab_bf16 = slab_bf16 ? 1 : 0;
    a.ldx = x->ld; a.Mpix = (int)mpix; a.H = a.Ho = (int)x->h; a.W = a.Wo = (int)x->w;
    a.stride = 1; a.pad = 0; a.KW = 1;
    a.CoutP = bm; a.Cin = cin; a.NG = cin; a.pix_per_split = p.pix_per_split;
    a.nx = (cin + WG_BN - 1) / WG_BN; a.ny = 1; a.splits = p.splits;
    a.x_bytes = (uint32_t)(((mpix - 1) * x->ld + x->c) * 2);  // X as a buffer: pieces beyond it (the last step's rows past the tensor) read zeros
    a.xcd_map = p.splits >= 8 ? 1 : 0;
    a.pw_shift = wgrad_patch_shift(x, dout);  // (the choice ymi_conv2d_bwd_weight makes for x and a draw of dout's shape: inside this kernel's scope the byte limits never decide)
    k.dout = dout->data; k.raw = raw->data; k.ld_dout = dout->ld; k.ld_raw = raw->ld;
    k.coef = coef; k.wd = w_dgrad_packed;
    k.dx = dx->data; k.ld_dx = dx->ld;
    k.add1 = add1 ? add1->data : nullptr; k.ld_a1 = add1 ? add1->ld : 0;
    k.add2 = add2 ? add2->data : nullptr; k.ld_a2 = add2 ? add2->ld : 0;
    dim3 grid((unsigned)a.nx, 1, (unsigned)p.splits);
    if (a.xcd_map) grid = dim3((unsigned)(8 * ((p.splits + 7) / 8) * a.nx), 1, 1);
    int prof = -1;
    if (ymi_prof_enabled())  // both products' FLOP; dout + raw + x in, dx (+ addends) out, the weight gradient
        prof = ymi_prof_start(s, 1, 4.0 * (double)mpix * bm * cin, ((double)mpix * (2.0 * bm + (2.0 + (add1 ? 1 : 0) + (add2 ? 1 : 0)) * cin)) * 2.0 + (double)bm * cin * 4.0,
                              2500.0);
    dispatch_dtype_act(YMI_BF16, act, [&](auto, auto ac) {
        constexpr int ACT = decltype(ac)::value;
        if (bm == 128) hipLaunchKernelGGL((conv1x1_bwd_kernel<128, ACT>), grid, dim3(256), conv1x1_bwd_lds_bytes<128>(), s, k);
        else hipLaunchKernelGGL((conv1x1_bwd_kernel<64, ACT>), grid, dim3(256), conv1x1_bwd_lds_bytes<64>(), s, k);
    });
    ymi_prof_stop(s, prof);
    YMI_CHECK_LAUNCH("conv1x1_bn_act_bwd");
    return wgrad_slab_sum(a, bm, cin, 1, dw_oihw, nullptr, pending, s);
}
