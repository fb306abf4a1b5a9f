// SwinBlock's second half as ONE kernel per direction:  out = x + fc2(gelu(fc1(LayerNorm2(x))))   (reference nn/modules/swin_block.py:31-35,53)
//
// The unfused path (igemm.hip: ymi_swin_mlp_fwd / _bwd_data) runs fc1 and fc2 as two token GEMMs that stream the [T, 4C] hidden matrix
// (115 MB at the model's 56,448 x 1024) through HBM: written twice, read once in the forward, read and written again in the backward -
// 87 + 54 us forward and 107 + 54 us of data gradients per block against 18 us bounds (profiles/r04_per_launch_bounds.txt).  Here the
// hidden activations of a token never leave the registers of the wave that owns the token:
//
//  * a workgroup = 256 tokens, a wave = 32 tokens (512 threads, one workgroup per CU).  Waves split ROWS only, so nothing but the weights
//    is shared: W1 / W2 stream through a three-stage LDS ring in chunks of 32 hidden units (16 KB + 16 KB per chunk, filled by LDS-DMA);
//    the two halves of the workgroup run one phase apart (matrix phase beside vector phase on every SIMD: see the schedule note below).
//  * LayerNorm-2 is the prologue: a lane holds half a token row (16 x 16 bytes), the statistics need one cross-half exchange, and the
//    normalised row IS the B operand of fc1 (v_mfma_f32_32x32x16_bf16, operands swapped: weights are A, tokens are B, so the 32 x 32
//    result holds a token per lane and 16 hidden units in its registers).
//  * bias + exact-erf GELU act on those registers; rounded to bf16 they are - with no lane movement and no LDS - the B operand of fc2
//    (cdna_hip_programming.md, "An accumulator tile as the next MFMA's operand"): the k order inside a 16-deep step is permuted
//    (element j of lane half h is hidden unit 16 s + 8 (j >> 2) + 4 h + (j & 3)), so W2 is packed with the same permutation.
//  * fc2 accumulates the [32 tokens x 256 channels] output tile in 128 accumulator registers over all 32 chunks; the epilogue adds bias
//    and the skip (the block's input, re-read from L2) before the single bf16 rounding and leaves through LDS in whole 512-byte rows.
//  * training: the normalised tokens u (weight gradient of fc1), the LayerNorm statistics and the bf16 pre-activations are stored once;
//    the pre-activations in the register order of the kernel (a private layout the backward kernel reads back with 512-byte contiguous
//    wave accesses).  The backward kernel recomputes gelu / gelu' from them, forms d_pre = (d_out W2) * gelu'(pre) and d_u = d_pre W1 in
//    the same one-pass form, and writes post = gelu(pre) and d_pre row-major for the two weight-gradient GEMMs.
//  (The figures in these points are those of C = 256, the width the schedule was shaped on; "Widths" below says what follows C.)
//
// Arithmetic and rounding points are those of the unfused path (u, pre, post, out stored / consumed as bf16; f32 accumulation), so the
// bf16 parity bounds of tests/test_gpu_bf16_matched.py are unchanged.  bf16, C = 128, 256 or 384 (the three widths the model files give a
// SwinBlock), hidden a multiple of 32 up to the LDS cap of the width; other shapes keep the unfused path.
//
// Widths.  The kernels are templates on C (MlpCfg<C> holds everything that follows it); per hidden chunk of 32 units
//                    k-steps  tiles  image    ring stage  ring     waves  tokens / workgroup  output staging  hidden <=
//   C = 128          8        4      8 KB     16 KB       48 KB    8      256                 64 KB           8192
//   C = 256          16       8      16 KB    32 KB       96 KB    8      256                 128 KB          8192
//   C = 384          24       12     24 KB    48 KB       144 KB   4      128                 96 KB           4096
// (k-steps = C / 16 fragments of the rows form = operand fragments of a lane; tiles = C / 32 accumulator tiles of a wave, two fragments of
// the cols form each; image = 32 C bf16; hidden is capped so that ring / staging + the b1 vector fit the CU's 160 KB of LDS.)
// At 384 a wave's output tile is 192 accumulator registers and its fc1 operand 96 more: beyond the 256 a wave gets at two waves per SIMD.
// That width therefore runs FOUR waves of 32 tokens per workgroup, one per SIMD, each with the whole 512-entry file (the accumulators in
// AGPRs); the weights are still one chunk shared by the workgroup through the same ring, every wave still reads a whole chunk per 32
// tokens (the LDS bytes per FLOP of the other widths), and the phases stay but are no longer paired: all four waves run the matrix phase,
// then the vector phase.  A 128-token workgroup divides the 256-token padding of ymi_swin_ln_mlp_pre_elems, so the private layout and
// the rows the backward stores beyond T stay inside the caller's buffers.
// The private pre-activation layout is [tile][chunk][wave][g = 0, 1][lane][8] bf16 at every width, with the tile and the wave count of the
// width's workgroup: 256 tokens x 8 waves at C = 128 / 256, 128 tokens x 4 waves at C = 384 (element = hidden unit 32 chunk + 16 (lane >> 5) +
// 8 g + e of token tile base + 32 wave + (lane & 31)); a tile is always tokens x hidden elements.
#include <type_traits>

#include "common.h"

typedef __attribute__((ext_vector_type(16))) float f32x16;

// compile-time loop: f(std::integral_constant<int, 0>{}) ... f(std::integral_constant<int, N-1>{})
template <int I, int N, class F> __device__ __forceinline__ void static_for(F&& f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        static_for<I + 1, N>(f);
    }
}

constexpr int MLP_PAD = 256;       // tokens the caller's pre / post / d_pre buffers are padded to: every width's workgroup tile divides it
constexpr int MLP_HC = 32;         // hidden units per chunk
constexpr int MLP_LDS_MAX = 160 * 1024;  // LDS of a CU (one workgroup per CU)
template <int C> struct MlpCfg {
    static_assert(C == 128 || C == 256 || C == 384, "SwinBlock widths of the model files");
    static constexpr int NW = C > 256 ? 4 : 8;     // waves per workgroup (32 tokens each): 8 = two per SIMD, run one phase apart; 4 = one per SIMD
    static constexpr int WPS = NW / 4;             // waves per SIMD (the register budget: 512 / WPS)
    static constexpr bool HALVES = NW == 8;
    static constexpr int NT = NW * 64;             // threads
    static constexpr int BM = NW * 32;             // tokens per workgroup
    static constexpr int KS = C / 16;              // k-steps of the rows form = operand fragments per lane
    static constexpr int CT = C / 32;              // accumulator tiles of a wave
    static constexpr int IMG = 32 * C * 2;         // bytes of one fragment-major chunk image
    static constexpr int STAGE = 2 * IMG;          // bytes per ring stage: a rows image and a cols image
    static constexpr int PIECES = IMG / 16 / NT;   // 16-byte LDS-DMA pieces per thread and image
    static constexpr int ROWB = 2 * C;             // bytes of an output row
    static constexpr int STORE = NW * 32 * ROWB;   // the output staging image: [wave][32 rows][ROWB]
    static constexpr int LDS_TILE = 3 * STAGE > STORE ? 3 * STAGE : STORE;  // the ring (3 stages) and, afterwards, the staging image share it
    static constexpr int HIDDEN_MAX = (MLP_LDS_MAX - LDS_TILE) / 4 < 8192 ? (MLP_LDS_MAX - LDS_TILE) / 4 : 8192;  // b1 [hidden] floats behind the tile
    static_assert(IMG % (16 * NT) == 0 && MLP_PAD % BM == 0 && HIDDEN_MAX % MLP_HC == 0, "");
};

// Which hidden unit sits where is this file's choice (it fixes the row order of the fc1 weight image): the unit in row rho of a chunk's 32 x 32
// result tile is mlp_unit_of_row(rho), chosen so that the 16 results a lane holds (rows 8 q + 4 h + r of the MFMA's C/D layout) are 16
// CONSECUTIVE hidden units, 16 h + 4 q + r: the bias is four 16-byte loads, the saved pre-activations / post / d_pre leave as 16-byte stores,
// and the second product's k-step s takes from lane half h the units 16 h + 8 s + 0..7 - 16 contiguous bytes of the natural weight row.
__host__ __device__ __forceinline__ int mlp_unit_of_row(int rho) { return 16 * ((rho >> 2) & 1) + 4 * (rho >> 3) + (rho & 3); }
// position p (0..31) of the second product's k order (k-step s = p >> 4, lane half h = (p >> 3) & 1, element j = p & 7) -> hidden unit of the chunk
__host__ __device__ __forceinline__ int mlp_unit_of_pos(int p) { return 16 * ((p >> 3) & 1) + 8 * (p >> 4) + (p & 7); }

// ---- weight operands ---------------------------------------------------------------------------------------------------------------
// w1 [hidden][C], w2 [C][hidden] (float32, the nn.Linear layouts) -> four bf16 images of hidden * C elements each, all FRAGMENT-MAJOR: a
// chunk of 32 hidden units is 32 C elements (8 / 16 / 24 KB at C = 128 / 256 / 384) laid out as the MFMA A fragments the kernels read - [k-step or tile][lane 0..63][8 elements] - so the
// global image, the LDS image and the lane order coincide: LDS-DMA copies it linearly, a wave's ds_read_b128 of one fragment is 1 KB
// contiguous (conflict-free, no swizzle), and every LDS address is one per-lane base plus an immediate.
//   [0] w1f  rows form  [hidden/32][C/16 k-steps][64 lanes][8]:  A[row = lane & 31 (hidden unit mlp_unit_of_row(row))][k = 16 s + 8 (lane >> 5) + j (channel)] = w1
//   [1] w2f  cols form  [hidden/32][C/32 tiles][2 steps][64][8]: A[row = 32 ct + (lane & 31) (channel)][k = position 16 s + 8 (lane >> 5) + j] = w2,
//                                                              position p <-> hidden unit mlp_unit_of_pos(p) of the chunk
//   [2] w2tf rows form of w2 transposed (d_post = d_out W2):   A[hidden unit][channel] = w2[channel][hidden unit]
//   [3] w1tf cols form of w1 transposed (d_u = d_pre W1):      A[channel][position] = w1[hidden unit of the position][channel]
__global__ __launch_bounds__(256) void swin_mlp_pack_kernel(const float* __restrict__ w1, const float* __restrict__ w2, int C, int hidden, bf16_t* __restrict__ dst) {
    const int64_t n = (int64_t)C * hidden;
    for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int j = (int)(i & 7), lane = (int)((i >> 3) & 63);
        const int64_t blk = i >> 9;  // 512-element fragment blocks
        const int ks = C / 16;  // 512-element fragment blocks per chunk, either form
        {   // rows form: blk = jc * (C / 16) + s
            const int s = (int)(blk % ks), jc = (int)(blk / ks);
            const int hu = jc * 32 + mlp_unit_of_row(lane & 31), c = 16 * s + 8 * (lane >> 5) + j;
            dst[i] = (bf16_t)w1[(int64_t)hu * C + c];
            dst[2 * n + i] = (bf16_t)w2[(int64_t)c * hidden + hu];
        }
        {   // cols form: blk = (jc * (C / 32) + ct) * 2 + s
            const int s = (int)(blk & 1), ct = (int)((blk % ks) >> 1), jc = (int)(blk / ks);
            const int c = 32 * ct + (lane & 31), hu = jc * 32 + mlp_unit_of_pos(16 * s + 8 * (lane >> 5) + j);
            dst[n + i] = (bf16_t)w2[(int64_t)c * hidden + hu];
            dst[3 * n + i] = (bf16_t)w1[(int64_t)hu * C + c];
        }
    }
}

struct MlpFwdArgs {
    const bf16_t* x;  // block input tokens [T][ldx]: LayerNorm-2's input and the skip
    int64_t ldx;
    const float* gamma;
    const float* beta;
    float eps;
    const bf16_t* w1p;
    const bf16_t* w2q;
    const float* b1;
    const float* b2;
    bf16_t* u;  // [T][ldu] normalised tokens (training) or nullptr
    int64_t ldu;
    float* mean;
    float* rstd;
    bf16_t* pre;  // private layout (training) or nullptr
    bf16_t* out;
    int64_t ldo;
    int T, hidden;
};

__device__ __forceinline__ float bf16_lo(uint32_t v) { return __builtin_bit_cast(float, v << 16); }
__device__ __forceinline__ float bf16_hi(uint32_t v) { return __builtin_bit_cast(float, v & 0xffff0000u); }

// gelu(x) = max(x, 0) - |x| * (0.5 * (1 - erf(|x| / sqrt 2))), the complementary term by Abramowitz-Stegun 7.1.26 (common.h: erf_as; the
// same six-term form with the halving folded into the coefficients and the argument scalings into the constants): 11 issue slots + two
// transcendentals per element - the vector phases of these kernels are bound by exactly this count.
__device__ __forceinline__ float gelu_fast(float x, float* half_erfc = nullptr, float* e_out = nullptr) {
    const float ax = fabsf(x);                                                                // (a source modifier, no instruction)
    const float t = __builtin_amdgcn_rcpf(fmaf(0.3275911f * 0.70710678118654752440f, ax, 1.0f));
    const float s = ax * 0.84932180028801904272f;                                              // sqrt(0.5 log2 e) |x|
    const float e = __builtin_amdgcn_exp2f(-(s * s));                                          // e^(-x^2 / 2)
    float p = 0.5f * 1.061405429f;
    p = fmaf(p, t, -0.5f * 1.453152027f);
    p = fmaf(p, t, 0.5f * 1.421413741f);
    p = fmaf(p, t, -0.5f * 0.284496736f);
    p = fmaf(p, t, 0.5f * 0.254829592f);
    const float w = p * t * e;  // 0.5 * erfc(|x| / sqrt 2)
    if (half_erfc) *half_erfc = w;
    if (e_out) *e_out = e;
    float relu;
    asm("v_max_f32 %0, 0, %1" : "=v"(relu) : "v"(x));  // (fmaxf would first canonicalise x with a second v_max)
    return fmaf(-ax, w, relu);
}

// issue the LDS-DMA pieces of hidden chunk jc into ring stage `stage`: two fragment-major images of 32 C elements, copied linearly, 16 bytes per
// thread and piece - 2 PIECES per thread: 2 at C = 128 (8 KB images, 512 threads), 4 at 256 (16 KB), 12 at 384 (24 KB, 256 threads)
template <int C> __device__ __forceinline__ void mlp_issue(const bf16_t* rows_img, const bf16_t* cols_img, int jc, char* stage, int tid, int wave) {
    using K = MlpCfg<C>;
    const bf16_t* a = rows_img + (size_t)jc * 32 * C + tid * 8;
    const bf16_t* b = cols_img + (size_t)jc * 32 * C + tid * 8;
#pragma unroll
    for (int i = 0; i < K::PIECES; ++i) __builtin_amdgcn_global_load_lds((gptr_t)(a + i * K::NT * 8), (lptr_t)(stage + (i * K::NT + wave * 64) * 16), 16, 0, 0);
#pragma unroll
    for (int i = 0; i < K::PIECES; ++i)
        __builtin_amdgcn_global_load_lds((gptr_t)(b + i * K::NT * 8), (lptr_t)(stage + K::IMG + (i * K::NT + wave * 64) * 16), 16, 0, 0);
}

// The two products of a chunk with the fragment reads kept AHEAD of the MFMAs.  hipcc places an LDS read right before its use, waits with
// lgkmcnt(0) and - at 250 live registers - recycles ONE fragment buffer: an exposed LDS round trip (~130 cycles) per 32-cycle MFMA.  So the
// reads and their counted waits are written out (as igemm.hip's K step): four fragment buffers rotate, three reads stay in flight behind
// every MFMA.  (Other LDS operations the compiler interleaves only make a counted wait stricter: LDS operations return in order.)
#define MLP_RD(F, ADDR, OFF) asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(F) : "v"(ADDR), "n"(OFF))
#define MLP_WAIT(N)                                                    \
    do {                                                               \
        __builtin_amdgcn_sched_barrier(0);                             \
        asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(N) : "memory");     \
    } while (0)
__device__ __forceinline__ uint32_t lds_u32(const void* p) { return (uint32_t)(uintptr_t)(lptr_t)p; }
// d += A(rows image: KS k-steps of 1 KB from `addr`) . b[0..KS-1]
template <int KS> __device__ __forceinline__ void mlp_rows_product(uint32_t addr, const bf16x8 (&b)[KS], f32x16& d) {
    bf16x8 f[4] = {};
    MLP_RD(f[0], addr, 0);
    MLP_RD(f[1], addr, 1024);
    MLP_RD(f[2], addr, 2048);
    MLP_RD(f[3], addr, 3072);
    static_for<0, KS>([&](auto sc) {
        constexpr int s = decltype(sc)::value;
        const uint32_t ad = addr;  // (an odr-use outside the asm operand: clang does not capture a variable it only sees there)
        MLP_WAIT((KS - 1 - s) < 3 ? (KS - 1 - s) : 3);
        asm volatile("" : "+v"(f[s & 3]));
        d = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f[s & 3], b[s], d, 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (s + 4 < KS) MLP_RD(f[s & 3], ad, (s + 4) * 1024);
    });
}
// acc = 0.  At C = 384 the tiles are AGPRs by name (mlp_cols_product) from their first value on - an MFMA of zero operands onto the constant 0 -
// so that no copy of the 192 registers ever lives in VGPRs
template <int CT> __device__ __forceinline__ void mlp_zero_acc(f32x16 (&acc)[CT]) {
    if constexpr (CT > 8) {
        const bf16x8 z = {};
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) asm volatile("s_nop 4\n\tv_mfma_f32_32x32x16_bf16 %0, %1, %1, 0" : "=a"(acc[ct]) : "v"(z));  // (wait states: z is freshly written, and 0 x stale bits may be NaN)
    } else {
#pragma unroll
        for (int ct = 0; ct < CT; ++ct)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[ct][r] = 0.f;
    }
}
// acc[ct] += A(cols image: CT tiles x 2 steps of 1 KB from `addr`) . hv[0..1]
template <int CT> __device__ __forceinline__ void mlp_cols_product(uint32_t addr, const bf16x8 (&hv)[2], f32x16 (&acc)[CT]) {
    bf16x8 f[4] = {};
    MLP_RD(f[0], addr, 0);
    MLP_RD(f[1], addr, 1024);
    MLP_RD(f[2], addr, 2048);
    MLP_RD(f[3], addr, 3072);
    static_for<0, 2 * CT>([&](auto ic) {
        constexpr int i = decltype(ic)::value;  // i = 2 ct + s
        const uint32_t ad = addr;
        MLP_WAIT((2 * CT - 1 - i) < 3 ? (2 * CT - 1 - i) : 3);
        asm volatile("" : "+v"(f[i & 3]));
        if constexpr (CT > 8) {
            // (C = 384, one wave per SIMD: the 192 accumulator registers are NAMED as AGPRs - a wave has at most 256 of either kind, and left to
            // itself hipcc keeps part of this tile in VGPRs and spills 128 registers per chunk.  Each tile takes two MFMAs back to back, then rests
            // until the next chunk; the epilogue reads it long after the last one: past a barrier, further than any MFMA result latency.)
            // (i < 2: the first reads of hv[0] / hv[1], which vector instructions wrote; an MFMA in inline assembly gets no wait states from the
            // compiler after a vector write of its operand - the zeroing MFMAs below read stale bits without them)
            if constexpr (i < 2) asm volatile("s_nop 4\n\tv_mfma_f32_32x32x16_bf16 %0, %1, %2, %0" : "+a"(acc[i >> 1]) : "v"(f[i & 3]), "v"(hv[i & 1]));
            else asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, %0" : "+a"(acc[i >> 1]) : "v"(f[i & 3]), "v"(hv[i & 1]));
        } else {
            acc[i >> 1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f[i & 3], hv[i & 1], acc[i >> 1], 0, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (i + 4 < 2 * CT) MLP_RD(f[i & 3], ad, (i + 4) * 1024);
    });
}

// 16-byte chunk `idx` of image row `r` (0..31) sits at chunk mlp_swz<C>(idx, r) of that row.  A row of 256 channels is 32 chunks and the XOR
// with the whole row number stays inside it; rows of 16 (C = 128) or 48 (C = 384) chunks are no power of two that covers 0..31, so there the XOR
// takes the row's low four bits only: a bijection on every aligned group of 16 chunks, whatever the number of groups.  Bank behaviour
// (MI355X_MICROARCH.md, LDS: ds_write_b64 goes 16 lanes at a time over 32 banks, ds_read_b128 16 lanes over 64): the 16 lanes of a write group
// hold 16 rows px & 15 all different, one chunk index - 16 different chunks of a 256-byte span, 8 bytes each, two lanes per bank pair, as with
// the 5-bit XOR (a 2-way store conflict costs nothing beside the store's own transfer cycles); a read group inside one row takes 16 chunks
// of it that differ in the low four bits of the index, and the XOR permutes those: conflict-free, again as at 256.
template <int C> __device__ __forceinline__ int mlp_swz(int idx, int r) { return C == 256 ? idx ^ r : idx ^ (r & 15); }

// the output tile of a wave ([32 tokens][C channels] in the 32x32 accumulator layout) -> `dst` rows as whole lines of 2 C bytes, through the
// wave's own 32 rows of LDS: v[ct][r] + bias (+ the skip, gathered in the accumulator layout) is rounded once, dropped as 8-byte pieces into
// a [32][2 C bytes] image (16-byte chunks swizzled by the row), read back row-contiguous and stored 1 KB per wave instruction
// C = 384: the accumulators' MFMAs are inline assembly (mlp_cols_product), which the compiler's hazard pass does not see; before it reads the tiles,
// give the last 16-pass MFMA the 18 wait states a vector read of its result needs (CDNA3 ISA, 4.5: XDL write VGPR -> VALU read)
template <int CT> __device__ __forceinline__ void mlp_settle_acc() {
    if constexpr (CT > 8) asm volatile("s_nop 7\n\ts_nop 7\n\ts_nop 1" ::: "memory");
}

template <int C, bool SKIP>
__device__ __forceinline__ void mlp_store_tile(f32x16 (&acc)[C / 32], const float* bias, const bf16_t* skip, int64_t ldskip, bf16_t* dst, int64_t ldd, int row0,
                                               int T, char* img, int lane) {
    constexpr int ROWB = 2 * C, CPR = C / 8;  // bytes and 16-byte chunks per row
    const int px = lane & 31, h = lane >> 5;
    const int row = row0 + px;
    const bool rok = row < T;
    const int rowc = rok ? row : T - 1;
#pragma unroll
    for (int ct = 0; ct < C / 32; ++ct) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int ch = 32 * ct + 8 * q + 4 * h;
            float v[4];
            const f32x4 bb = bias ? *reinterpret_cast<const f32x4*>(bias + ch) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = acc[ct][4 * q + r] + bb[r];
            if (SKIP) {
                const u32x2 s = *reinterpret_cast<const u32x2*>(skip + (int64_t)rowc * ldskip + ch);
                v[0] += bf16_lo(s[0]); v[1] += bf16_hi(s[0]); v[2] += bf16_lo(s[1]); v[3] += bf16_hi(s[1]);
            }
            u32x2 o;
            o[0] = pack_bf16x2(v[0], v[1]);
            o[1] = pack_bf16x2(v[2], v[3]);
            *reinterpret_cast<u32x2*>(img + px * ROWB + 16 * mlp_swz<C>(4 * ct + q, px) + 8 * h) = o;
        }
    }
    // (a wave's own LDS writes are visible to its own later reads in program order: no barrier)
#pragma unroll
    for (int i = 0; i < C / 16; ++i) {
        // this lane: row r of the wave's tile, 16-byte chunk cl - piece 64 i + lane of the 32 CPR the image holds
        const int r = CPR == 32 ? 2 * i + h : (64 * i + lane) / CPR, cl = CPR == 32 ? px : (64 * i + lane) % CPR;
        const u32x4 val = *reinterpret_cast<const u32x4*>(img + r * ROWB + 16 * mlp_swz<C>(cl, r));
        if (row0 + r < T) *reinterpret_cast<u32x4*>(dst + (int64_t)(row0 + r) * ldd + cl * 8) = val;
    }
}

// C = 384 only: the three passes of LayerNorm over a lane's 192 values each convert bf16 -> f32 again.  hipcc otherwise keeps the 192 converted
// values of the first pass alive beside the 96 packed registers for the later passes - more than a wave's 256 VGPRs - and spills.
template <int KS> __device__ __forceinline__ void mlp_forget(bf16x8 (&v)[KS]) {
    if constexpr (KS > 16) {
#pragma unroll
        for (int s = 0; s < KS; ++s) asm volatile("" : "+v"(v[s]));
    }
}

// Schedule (both kernels; C = 128 and 256).  A workgroup is 8 waves = 256 tokens, one workgroup per CU; waves w and w + 4 share a SIMD.  A wave's chunk
// is a MATRIX phase (fc2 of the previous chunk + fc1 of this one: 32 MFMAs, fragment reads) followed by a VECTOR phase (bias / GELU /
// roundings / stores: ~270 VALU instructions), and the two halves of the workgroup (waves 0-3, waves 4-7) run ONE PHASE APART, every
// phase ending at a workgroup barrier: each SIMD always holds one wave in its matrix phase beside one in its vector phase - the
// arrangement MI355X_MICROARCH.md "Two waves per SIMD" describes - instead of two waves that drift into the same phase (the first form
// of this kernel, two independent 4-wave workgroups per CU, measured 24 % MFMA-busy with 37 % of the wave cycles issue-stalled:
// profiles/r05_swin_mlp_fused.txt).  Global phase t: half 0 runs matrix phases at even t, half 1 at odd t.  Weight chunk c (32 KB) is
// copied into ring stage c % 3 at the start of phase 2c - 2 (its previous tenant, chunk c - 3, was last read in phase 2c - 3), every
// wave retires its pieces before the barrier that ends phase 2c - 1, and the first read is in phase 2c.
// C = 384 (four waves, one per SIMD): there is no second half.  Every wave is "half 0" - matrix phases at even t, vector phases at odd t - and the
// ring protocol above holds word for word.  In the backward kernel the lines that belong to half 1 compile away; the forward kernel states its
// chunk loop a second time for this form (see there).
// Counted waits.  A wave retires its LDS-DMA pieces of chunk c by waiting until only the vector-memory operations it issued AFTER them are still
// outstanding.  That count does not change with the width - the pieces themselves (2, 4 or 12 per thread: mlp_issue) are what is waited for, not
// what is counted - and is the same in both halves: forward, the 2 pre-activation stores of a vector phase (0 in evaluation); backward, the 2
// pre-activation loads of a matrix phase + the 4 post / d_pre stores of a vector phase = 6.  The comment at each wait lists them.  (The
// forward's one-wave-per-SIMD loop waits with vmcnt(0) ahead of its stores instead.)
__device__ __forceinline__ void mlp_barrier() { asm volatile("s_barrier" ::: "memory"); }

template <int C> __global__ __launch_bounds__(MlpCfg<C>::NT, MlpCfg<C>::WPS) void swin_mlp_fwd_kernel(MlpFwdArgs a) {
    using K = MlpCfg<C>;
    constexpr int KS = K::KS, CT = K::CT, NW = K::NW, MLP_STAGE = K::STAGE;
    const bool TRAIN = a.u != nullptr;  // (kernel argument: uniform) save u, the LayerNorm statistics and the pre-activations
    extern __shared__ __attribute__((aligned(16))) char smem[];  // [3 stages][STAGE] (the output staging image afterwards: NW x 32 rows) | b1 [hidden] floats
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int half = K::HALVES ? wave >> 2 : 0;  // (waves w and w + 4 share a SIMD: pairing by wave & 1 or (wave >> 1) & 1 measured 25 % slower)
    const int px = lane & 31, h = lane >> 5;
    const int row0 = blockIdx.x * K::BM + wave * 32;
    const int row = row0 + px;
    const bool rok = row < a.T;
    const int rowc = rok ? row : a.T - 1;
    float* b1s = reinterpret_cast<float*>(smem + K::LDS_TILE);
    const int nch = a.hidden / MLP_HC;

    mlp_issue<C>(a.w1p, a.w2q, 0, smem, tid, wave);
    if (nch > 1) mlp_issue<C>(a.w1p, a.w2q, 1, smem + MLP_STAGE, tid, wave);
    for (int i = tid; i < a.hidden; i += K::NT) b1s[i] = a.b1[i];

    // ---- LayerNorm-2 (swin_block.py:53 norm2): lane (px, h) holds channels 16 s + 8 h + 0..7 of token row0 + px, s = 0..C/16-1 ------
    bf16x8 uf[KS];
    {
        const bf16_t* xr = a.x + (int64_t)rowc * a.ldx + 8 * h;
        float sum = 0.f;
#pragma unroll
        for (int s = 0; s < KS; ++s) uf[s] = *reinterpret_cast<const bf16x8*>(xr + 16 * s);
#pragma unroll
        for (int s = 0; s < KS; ++s)
#pragma unroll
            for (int i = 0; i < 8; ++i) sum += (float)uf[s][i];
        sum += __shfl_xor(sum, 32, 64);
        const float mu = sum * (1.0f / C);
        mlp_forget<KS>(uf);
        float q = 0.f;
#pragma unroll
        for (int s = 0; s < KS; ++s)
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const float d = (float)uf[s][i] - mu;
                q += d * d;
            }
        q += __shfl_xor(q, 32, 64);
        mlp_forget<KS>(uf);
        const float rs = rsqrtf(q * (1.0f / C) + a.eps);
        if (TRAIN && rok && h == 0) {
            a.mean[row] = mu;
            a.rstd[row] = rs;
        }
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            const int c = 16 * s + 8 * h;
            const f32x4 g0 = *reinterpret_cast<const f32x4*>(a.gamma + c), g1 = *reinterpret_cast<const f32x4*>(a.gamma + c + 4);
            const f32x4 e0 = *reinterpret_cast<const f32x4*>(a.beta + c), e1 = *reinterpret_cast<const f32x4*>(a.beta + c + 4);
            bf16x8 o;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                o[i] = (bf16_t)(((float)uf[s][i] - mu) * rs * g0[i] + e0[i]);
                o[4 + i] = (bf16_t)(((float)uf[s][4 + i] - mu) * rs * g1[i] + e1[i]);
            }
            uf[s] = o;
            if (TRAIN && rok) *reinterpret_cast<bf16x8*>(a.u + (int64_t)row * a.ldu + c) = o;
        }
    }

    f32x16 acc[CT];
    mlp_zero_acc<CT>(acc);

    // saved pre-activations, private layout [tile of BM tokens][chunk][wave 0..NW-1][g = 0, 1][lane][8]: units 16 h + 8 g + 0..7 of the chunk for
    // token px of the wave (a tile is BM * hidden elements: 256-token tiles of 8 waves at C = 128 / 256, 128-token tiles of 4 waves at 384)
    bf16_t* prew = TRAIN ? a.pre + ((((size_t)blockIdx.x * nch) * NW + wave) * 2 * 64 + lane) * 8 : nullptr;
    bf16x8 hv[2];
    hv[0] = hv[1] = uf[0];  // (defined values; never used before the first vector phase writes them)

    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");  // chunks 0 and 1, the bias vector
    mlp_barrier();
    const uint32_t lds0 = lds_u32(smem) + lane * 16;
    if constexpr (K::HALVES) {
        if (half == 1) mlp_barrier();  // the second half idles one phase
        // iteration jc = this wave's matrix phase (global phase t = 2 jc + half) and vector phase (t + 1) of chunk jc
        for (int jc = 0; jc <= nch; ++jc) {
            // ---- matrix phase: fc2 of chunk jc - 1 (acc[ct][channel 32 ct + 8 (r >> 2) + 4 h + (r & 3)][token px] += over its 32 hidden units), then
            //      fc1 of chunk jc (d1[hidden unit 8 (r >> 2) + 4 h + (r & 3)][token px] over K = C channels, starting at the bias)
            if (half == 0 && jc >= 1 && jc + 1 < nch) mlp_issue<C>(a.w1p, a.w2q, jc + 1, smem + ((jc + 1) % 3) * MLP_STAGE, tid, wave);  // (even global phase)
            __builtin_amdgcn_s_setprio(1);
            if (jc > 0) mlp_cols_product<CT>(lds0 + ((jc - 1) % 3) * MLP_STAGE + K::IMG, hv, acc);
            f32x16 d1;
            {
                const int jb = jc < nch ? jc : nch - 1;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const f32x4 bb = *reinterpret_cast<const f32x4*>(b1s + jb * 32 + 16 * h + 4 * q);
#pragma unroll
                    for (int r = 0; r < 4; ++r) d1[4 * q + r] = bb[r];
                }
            }
            if (jc < nch) mlp_rows_product<KS>(lds0 + (jc % 3) * MLP_STAGE, uf, d1);
            __builtin_amdgcn_s_setprio(0);
            // (odd global phase for the second half) the pieces issued one phase ago have landed: only the two pre-activation stores are younger
            if (half == 1) {
                if (TRAIN) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
                else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            }
            mlp_barrier();
            if (jc == nch) break;
            // ---- vector phase: bf16 rounding of the pre-activation (saved), exact-erf GELU, bf16 again: the B operand of fc2
            if (half == 1 && jc + 2 < nch) mlp_issue<C>(a.w1p, a.w2q, jc + 2, smem + ((jc + 2) % 3) * MLP_STAGE, tid, wave);  // (even global phase)
            uint32_t hf[8], pf[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                pf[i] = pack_bf16x2(d1[2 * i], d1[2 * i + 1]);
                hf[i] = pack_bf16x2(gelu_fast(bf16_lo(pf[i])), gelu_fast(bf16_hi(pf[i])));
            }
            if (TRAIN) {
                *reinterpret_cast<u32x4*>(prew + ((size_t)jc * NW * 2 + 0) * 64 * 8) = u32x4{pf[0], pf[1], pf[2], pf[3]};
                *reinterpret_cast<u32x4*>(prew + ((size_t)jc * NW * 2 + 1) * 64 * 8) = u32x4{pf[4], pf[5], pf[6], pf[7]};
            }
            u32x4 t0 = {hf[0], hf[1], hf[2], hf[3]}, t1 = {hf[4], hf[5], hf[6], hf[7]};
            hv[0] = __builtin_bit_cast(bf16x8, t0);
            hv[1] = __builtin_bit_cast(bf16x8, t1);
            if (half == 0) {  // (odd global phase for the first half) younger than the pieces issued in its matrix phase: the two pre-activation stores
                if (TRAIN) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
                else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            }
            mlp_barrier();
        }
        if (half == 0) mlp_barrier();  // the first half waits out the second half's last phase
    } else {
        // One wave per SIMD (C = 384): the same phases without the second half, written as prologue / loop / nothing else so that the accumulator
        // tiles are updated at ONE place (in the loop above's shape - fc2 under `jc > 0`, the exit in mid-body - hipcc duplicates the vector phase
        // and hands the 192 AGPRs from copy to copy through moves and scratch).  Matrix phase m = fc2 of chunk m - 1 + fc1 of chunk m; chunk m + 1
        // is issued at its start into the stage chunk m - 2 left in matrix phase m - 1, and retired in the vector phase that follows, BEFORE that
        // phase's own two stores: everything older at that point - these pieces, the previous chunk's stores - was issued a matrix phase ago or
        // more, so the wait is vmcnt(0) and there is no count to keep.
        auto bias_tile = [&](int jb, f32x16& d1) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const f32x4 bb = *reinterpret_cast<const f32x4*>(b1s + jb * 32 + 16 * h + 4 * q);
#pragma unroll
                for (int r = 0; r < 4; ++r) d1[4 * q + r] = bb[r];
            }
        };
        f32x16 d1;
        bias_tile(0, d1);
        __builtin_amdgcn_s_setprio(1);
        mlp_rows_product<KS>(lds0, uf, d1);  // matrix phase 0: fc1 of chunk 0
        __builtin_amdgcn_s_setprio(0);
        mlp_barrier();
        for (int jc = 0; jc < nch; ++jc) {
            // ---- vector phase of chunk jc
            uint32_t hf[8], pf[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                pf[i] = pack_bf16x2(d1[2 * i], d1[2 * i + 1]);
                hf[i] = pack_bf16x2(gelu_fast(bf16_lo(pf[i])), gelu_fast(bf16_hi(pf[i])));
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            if (TRAIN) {
                *reinterpret_cast<u32x4*>(prew + ((size_t)jc * NW * 2 + 0) * 64 * 8) = u32x4{pf[0], pf[1], pf[2], pf[3]};
                *reinterpret_cast<u32x4*>(prew + ((size_t)jc * NW * 2 + 1) * 64 * 8) = u32x4{pf[4], pf[5], pf[6], pf[7]};
            }
            u32x4 t0 = {hf[0], hf[1], hf[2], hf[3]}, t1 = {hf[4], hf[5], hf[6], hf[7]};
            hv[0] = __builtin_bit_cast(bf16x8, t0);
            hv[1] = __builtin_bit_cast(bf16x8, t1);
            mlp_barrier();
            // ---- matrix phase jc + 1 (the last one: fc2 only)
            if (jc + 2 < nch) mlp_issue<C>(a.w1p, a.w2q, jc + 2, smem + ((jc + 2) % 3) * MLP_STAGE, tid, wave);
            __builtin_amdgcn_s_setprio(1);
            mlp_cols_product<CT>(lds0 + (jc % 3) * MLP_STAGE + K::IMG, hv, acc);
            if (jc + 1 < nch) {
                bias_tile(jc + 1, d1);
                mlp_rows_product<KS>(lds0 + ((jc + 1) % 3) * MLP_STAGE, uf, d1);
            }
            __builtin_amdgcn_s_setprio(0);
            mlp_barrier();
        }
    }
    // (the last barrier: every wave has finished reading the ring, which becomes the output staging image)
    mlp_settle_acc<CT>();
    mlp_store_tile<C, true>(acc, a.b2, a.x, a.ldx, a.out, a.ldo, row0, a.T, smem + wave * (32 * K::ROWB), lane);
}

// ---- backward, data path ----------------------------------------------------------------------------------------------------------
// d_post = d_out W2 (K = C), d_pre = bf16(d_post) * gelu'(pre) (the unfused epilogue's arithmetic, igemm.hip), d_u += d_pre W1 chunk by
// chunk: the same register hand-over as the forward (d_post's 32 x 32 tile -> the B operand of the second product).  post = gelu(pre)
// (bit for bit what the forward fed to fc2: the same expression on the same stored bf16 pre-activation) and d_pre leave row-major for
// the two weight-gradient GEMMs.
struct MlpBwdArgs {
    const bf16_t* dout;
    int64_t lddo;
    const bf16_t* w2t;
    const bf16_t* w1tq;
    const bf16_t* pre;  // private layout
    bf16_t* post;
    int64_t ldpost;
    bf16_t* dpre;
    int64_t lddpre;
    bf16_t* du;
    int64_t lddu;
    int T, hidden;
};

template <int C> __global__ __launch_bounds__(MlpCfg<C>::NT, MlpCfg<C>::WPS) void swin_mlp_bwd_kernel(MlpBwdArgs a) {
    using K = MlpCfg<C>;
    constexpr int KS = K::KS, CT = K::CT, NW = K::NW, MLP_STAGE = K::STAGE;
    extern __shared__ __attribute__((aligned(16))) char smem[];  // [3 stages][STAGE]; the d_u staging image afterwards (NW x 32 rows)
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int half = K::HALVES ? wave >> 2 : 0;
    const int px = lane & 31, h = lane >> 5;
    const int row0 = blockIdx.x * K::BM + wave * 32;
    const int row = row0 + px;
    const int rowc = row < a.T ? row : a.T - 1;
    const int nch = a.hidden / MLP_HC;

    mlp_issue<C>(a.w2t, a.w1tq, 0, smem, tid, wave);
    if (nch > 1) mlp_issue<C>(a.w2t, a.w1tq, 1, smem + MLP_STAGE, tid, wave);
    bf16x8 df[KS];
    {
        const bf16_t* xr = a.dout + (int64_t)rowc * a.lddo + 8 * h;
#pragma unroll
        for (int s = 0; s < KS; ++s) df[s] = *reinterpret_cast<const bf16x8*>(xr + 16 * s);
    }
    f32x16 acc[CT];
    mlp_zero_acc<CT>(acc);
    // addresses as a wave-uniform base (scalar registers) + a 32-bit per-lane offset: the kernel has no vector registers to spare for pointers
    const char* pre_base = reinterpret_cast<const char*>(a.pre + (((size_t)blockIdx.x * nch) * NW + wave) * 2 * 64 * 8);
    const uint32_t pre_off = (uint32_t)lane * 16u;
    // post / d_pre rows: ALWAYS stored (rows beyond T land in the padding the caller provides), so that every wave issues the same number
    // of vector-memory operations per phase: the counted vmcnt below relies on it.  Both are dense [rows][hidden]: one offset serves both
    const uint32_t row_off = (uint32_t)(((int64_t)row * a.hidden + 16 * h) * 2);
    char* post_base = reinterpret_cast<char*>(a.post);
    char* dpre_base = reinterpret_cast<char*>(a.dpre);
    bf16x8 hv[2];
    hv[0] = hv[1] = df[0];

    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    mlp_barrier();
    const uint32_t lds0 = lds_u32(smem) + lane * 16;
    if (half == 1) mlp_barrier();
    for (int jc = 0; jc <= nch; ++jc) {
        // ---- matrix phase: d_u += d_pre(jc - 1) W1 chunk, then d_post(jc) = d_out W2 chunk; the stored pre-activations of chunk jc are
        //      requested first (two 16-byte loads per lane, used in the vector phase that follows)
        if (half == 0 && jc >= 1 && jc + 1 < nch) mlp_issue<C>(a.w2t, a.w1tq, jc + 1, smem + ((jc + 1) % 3) * MLP_STAGE, tid, wave);
        u32x4 pv[2];
        {
            const int jl = jc < nch ? jc : nch - 1;  // (always two loads: see the counted wait)
#pragma unroll
            for (int g = 0; g < 2; ++g) pv[g] = *reinterpret_cast<const u32x4*>(pre_base + ((size_t)jl * NW * 2 + g) * 64 * 16 + pre_off);
        }
        __builtin_amdgcn_s_setprio(1);
        if (jc > 0) mlp_cols_product<CT>(lds0 + ((jc - 1) % 3) * MLP_STAGE + K::IMG, hv, acc);
        f32x16 d1;
#pragma unroll
        for (int r = 0; r < 16; ++r) d1[r] = 0.f;
        if (jc < nch) mlp_rows_product<KS>(lds0 + (jc % 3) * MLP_STAGE, df, d1);
        __builtin_amdgcn_s_setprio(0);
        // (odd global phase for the second half) the pieces issued one phase ago have landed: younger are only four stores (its vector phase) and
        // these two loads; the first half below: two loads (its matrix phase) and four stores
        if (half == 1) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
        mlp_barrier();
        if (jc == nch) break;
        // ---- vector phase: post = gelu(pre), d_pre = bf16(d_post) * gelu'(pre), both stored row-major; d_pre is the B operand of the d_u product
        if (half == 1 && jc + 2 < nch) mlp_issue<C>(a.w2t, a.w1tq, jc + 2, smem + ((jc + 2) % 3) * MLP_STAGE, tid, wave);
        uint32_t hf[8], of[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {  // registers 2 i, 2 i + 1: units 16 h + 2 i, + 1
            float po[2], dp[2];
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const float x = r ? bf16_hi(pv[i >> 2][i & 3]) : bf16_lo(pv[i >> 2][i & 3]);
                float w, e;
                po[r] = gelu_fast(x, &w, &e);
                const float phi = x >= 0.f ? 1.0f - w : w;
                const float grad = fmaf(x * 0.39894228040143267794f, e, phi);
                dp[r] = to_f32(from_f32<bf16_t>(d1[2 * i + r])) * grad;
            }
            of[i] = pack_bf16x2(po[0], po[1]);
            hf[i] = pack_bf16x2(dp[0], dp[1]);
        }
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            *reinterpret_cast<u32x4*>(post_base + (size_t)(jc * 64 + 16 * g) + row_off) = u32x4{of[4 * g], of[4 * g + 1], of[4 * g + 2], of[4 * g + 3]};
            *reinterpret_cast<u32x4*>(dpre_base + (size_t)(jc * 64 + 16 * g) + row_off) = u32x4{hf[4 * g], hf[4 * g + 1], hf[4 * g + 2], hf[4 * g + 3]};
        }
        u32x4 t0 = {hf[0], hf[1], hf[2], hf[3]}, t1 = {hf[4], hf[5], hf[6], hf[7]};
        hv[0] = __builtin_bit_cast(bf16x8, t0);
        hv[1] = __builtin_bit_cast(bf16x8, t1);
        if (half == 0) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
        mlp_barrier();
    }
    if (K::HALVES && half == 0) mlp_barrier();
    mlp_settle_acc<CT>();
    mlp_store_tile<C, false>(acc, nullptr, nullptr, 0, a.du, a.lddu, row0, a.T, smem + wave * (32 * K::ROWB), lane);
}

// ---- host -------------------------------------------------------------------------------------------------------------------------
// one width's launches: the only place the three instantiations are named
template <int C> static void mlp_launch_fwd(const MlpFwdArgs& a, hipStream_t stream) {
    using K = MlpCfg<C>;
    const size_t lds = K::LDS_TILE + (size_t)a.hidden * sizeof(float);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(swin_mlp_fwd_kernel<C>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(swin_mlp_fwd_kernel<C>, dim3((unsigned)((a.T + K::BM - 1) / K::BM)), dim3(K::NT), lds, stream, a);
}
template <int C> static void mlp_launch_bwd(const MlpBwdArgs& a, hipStream_t stream) {
    using K = MlpCfg<C>;
    const size_t lds = K::LDS_TILE;
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(swin_mlp_bwd_kernel<C>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(swin_mlp_bwd_kernel<C>, dim3((unsigned)((a.T + K::BM - 1) / K::BM)), dim3(K::NT), lds, stream, a);
}
#define MLP_WIDTHS "128, 256 or 384"
static int64_t mlp_hidden_max(int64_t c) { return c == 128 ? MlpCfg<128>::HIDDEN_MAX : c == 256 ? MlpCfg<256>::HIDDEN_MAX : c == 384 ? MlpCfg<384>::HIDDEN_MAX : 0; }

// bfloat16, C = 128 / 256 / 384, hidden a multiple of 32 that leaves the b1 vector room in LDS beside the ring: <= 8192, 8192, 4096
extern "C" int ymi_swin_ln_mlp_supported(int64_t c, int64_t hidden, int32_t dtype) {
    return dtype == YMI_BF16 && hidden % MLP_HC == 0 && hidden >= MLP_HC && hidden <= mlp_hidden_max(c);
}
// elements of the packed weight images (bfloat16) and of the private pre-activation buffer for `tokens` tokens
extern "C" int64_t ymi_swin_ln_mlp_pack_elems(int64_t c, int64_t hidden) { return 4 * c * hidden; }
extern "C" int64_t ymi_swin_ln_mlp_pre_elems(int64_t tokens, int64_t hidden) { return (tokens + MLP_PAD - 1) / MLP_PAD * MLP_PAD * hidden; }

extern "C" int ymi_swin_ln_mlp_pack(const float* w1, const float* w2, int64_t c, int64_t hidden, void* packed, void* stream) {
    YMI_CHECK_ARG(w1 && w2 && packed && ymi_swin_ln_mlp_supported(c, hidden, YMI_BF16),
                  "swin_ln_mlp_pack: C = " MLP_WIDTHS ", hidden a multiple of %d up to %d / %d / %d", MLP_HC, MlpCfg<128>::HIDDEN_MAX, MlpCfg<256>::HIDDEN_MAX,
                  MlpCfg<384>::HIDDEN_MAX);
    YMI_CHECK_ARG(((uintptr_t)packed & 15) == 0, "swin_ln_mlp_pack: 16-byte alignment");
    const int64_t n = c * hidden;
    hipLaunchKernelGGL(swin_mlp_pack_kernel, dim3((unsigned)((n + 255) / 256 < 1024 ? (n + 255) / 256 : 1024)), dim3(256), 0, (hipStream_t)stream, w1, w2, (int)c, (int)hidden,
                       (bf16_t*)packed);
    YMI_CHECK_LAUNCH("swin_ln_mlp_pack");
    return YMI_OK;
}

extern "C" int ymi_swin_ln_mlp_fwd(const ymi_tensor* x, const float* gamma, const float* beta, float eps, const void* packed, const float* b1, const float* b2,
                                   int64_t hidden, const ymi_tensor* u, float* mean, float* rstd, void* pre, const ymi_tensor* out, void* stream) {
    YMI_CHECK_ARG(ymi_tensor_ok(x) && ymi_tensor_ok(out) && gamma && beta && packed && b1 && b2, "swin_ln_mlp_fwd: args");
    YMI_CHECK_ARG(ymi_swin_ln_mlp_supported(x->c, hidden, x->dtype) && out->dtype == x->dtype && out->c == x->c && ymi_pixels(out) == ymi_pixels(x),
                  "swin_ln_mlp_fwd: bfloat16 tokens of " MLP_WIDTHS " channels, hidden a multiple of %d up to %d / %d / %d", MLP_HC, MlpCfg<128>::HIDDEN_MAX,
                  MlpCfg<256>::HIDDEN_MAX, MlpCfg<384>::HIDDEN_MAX);
    const bool train = u != nullptr;
    if (train) YMI_CHECK_ARG(ymi_tensor_ok(u) && u->dtype == x->dtype && u->c == x->c && ymi_pixels(u) == ymi_pixels(x) && mean && rstd && pre, "swin_ln_mlp_fwd: saved tensors");
    YMI_CHECK_ARG(x->ld % 8 == 0 && out->ld % 8 == 0 && (!train || u->ld % 8 == 0) && ((((uintptr_t)x->data) | ((uintptr_t)out->data) | ((uintptr_t)packed) |
                  ((uintptr_t)gamma) | ((uintptr_t)beta) | ((uintptr_t)b1) | ((uintptr_t)b2) | (train ? ((uintptr_t)u->data | (uintptr_t)pre) : 0)) & 15) == 0,
                  "swin_ln_mlp_fwd: 16-byte alignment");
    const int64_t T = ymi_pixels(x);
    YMI_CHECK_ARG(T < (1ll << 31) && T * x->ld < (1ll << 31), "swin_ln_mlp_fwd: too large");
    const int64_t n = x->c * hidden;
    MlpFwdArgs a{};
    a.x = (const bf16_t*)x->data; a.ldx = x->ld;
    a.gamma = gamma; a.beta = beta; a.eps = eps;
    a.w1p = (const bf16_t*)packed; a.w2q = a.w1p + n;
    a.b1 = b1; a.b2 = b2;
    a.u = train ? (bf16_t*)u->data : nullptr; a.ldu = train ? u->ld : 0;
    a.mean = mean; a.rstd = rstd; a.pre = (bf16_t*)pre;
    a.out = (bf16_t*)out->data; a.ldo = out->ld;
    a.T = (int)T; a.hidden = (int)hidden;
    if (x->c == 128) mlp_launch_fwd<128>(a, (hipStream_t)stream);
    else if (x->c == 256) mlp_launch_fwd<256>(a, (hipStream_t)stream);
    else mlp_launch_fwd<384>(a, (hipStream_t)stream);
    YMI_CHECK_LAUNCH("swin_ln_mlp_fwd");
    return YMI_OK;
}

extern "C" int ymi_swin_ln_mlp_bwd_data(const ymi_tensor* dout, const void* packed, const void* pre, int64_t hidden, const ymi_tensor* post, const ymi_tensor* dpre,
                                        const ymi_tensor* du, void* stream) {
    YMI_CHECK_ARG(ymi_tensor_ok(dout) && ymi_tensor_ok(post) && ymi_tensor_ok(dpre) && ymi_tensor_ok(du) && packed && pre, "swin_ln_mlp_bwd_data: args");
    const int64_t T = ymi_pixels(dout);
    YMI_CHECK_ARG(ymi_swin_ln_mlp_supported(dout->c, hidden, dout->dtype) && post->dtype == dout->dtype && dpre->dtype == dout->dtype && du->dtype == dout->dtype &&
                      post->c == hidden && dpre->c == hidden && du->c == dout->c && ymi_pixels(post) == T && ymi_pixels(dpre) == T && ymi_pixels(du) == T,
                  "swin_ln_mlp_bwd_data: shapes (bfloat16 tokens of " MLP_WIDTHS " channels)");
    YMI_CHECK_ARG(dout->ld % 8 == 0 && du->ld % 8 == 0 && post->ld % 4 == 0 && dpre->ld % 4 == 0 &&
                      ((((uintptr_t)dout->data) | ((uintptr_t)du->data) | ((uintptr_t)packed) | ((uintptr_t)pre)) & 15) == 0 &&
                      ((((uintptr_t)post->data) | ((uintptr_t)dpre->data)) & 15) == 0,
                  "swin_ln_mlp_bwd_data: alignment");
    YMI_CHECK_ARG(T < (1ll << 31) && (T + MLP_PAD) * post->ld < (1ll << 31), "swin_ln_mlp_bwd_data: too large");
    YMI_CHECK_ARG(post->ld == hidden && dpre->ld == hidden, "swin_ln_mlp_bwd_data: post / dpre are dense [T][hidden] views of buffers of ymi_swin_ln_mlp_pre_elems elements");
    const int64_t n = dout->c * hidden;
    MlpBwdArgs a{};
    a.dout = (const bf16_t*)dout->data; a.lddo = dout->ld;
    a.w2t = (const bf16_t*)packed + 2 * n; a.w1tq = (const bf16_t*)packed + 3 * n;
    a.pre = (const bf16_t*)pre;
    a.post = (bf16_t*)post->data; a.ldpost = post->ld;
    a.dpre = (bf16_t*)dpre->data; a.lddpre = dpre->ld;
    a.du = (bf16_t*)du->data; a.lddu = du->ld;
    a.T = (int)T; a.hidden = (int)hidden;
    if (dout->c == 128) mlp_launch_bwd<128>(a, (hipStream_t)stream);
    else if (dout->c == 256) mlp_launch_bwd<256>(a, (hipStream_t)stream);
    else mlp_launch_bwd<384>(a, (hipStream_t)stream);
    YMI_CHECK_LAUNCH("swin_ln_mlp_bwd_data");
    return YMI_OK;
}
