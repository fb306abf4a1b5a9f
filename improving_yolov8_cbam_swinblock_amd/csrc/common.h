// Shared device/host helpers for libyolo_mi355.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include <type_traits>

#include "../../include/ymi.h"

typedef __bf16 bf16_t;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(2))) float f32x2;
typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;
typedef __attribute__((ext_vector_type(2))) uint32_t u32x2;

// global-memory source and LDS destination of an LDS-DMA load (__builtin_amdgcn_global_load_lds)
typedef const __attribute__((address_space(1))) void* gptr_t;
typedef __attribute__((address_space(3))) void* lptr_t;

#define YMI_WAVE 64

// ---- error plumbing (host) -------------------------------------------------------------------
void ymi_set_error(const char* fmt, ...);
#define YMI_CHECK_ARG(cond, ...)          \
    do {                                  \
        if (!(cond)) {                    \
            ymi_set_error(__VA_ARGS__);   \
            return YMI_EINVAL;            \
        }                                 \
    } while (0)
#define YMI_CHECK_LAUNCH(what)                                                   \
    do {                                                                         \
        hipError_t e_ = hipGetLastError();                                       \
        if (e_ != hipSuccess) {                                                  \
            ymi_set_error("%s: launch failed: %s", what, hipGetErrorString(e_)); \
            return YMI_ELAUNCH;                                                  \
        }                                                                        \
    } while (0)

static inline bool ymi_tensor_ok(const ymi_tensor* t) {
    return t && t->data && t->n > 0 && t->h > 0 && t->w > 0 && t->c > 0 && t->ld >= t->c && (t->dtype == YMI_F32 || t->dtype == YMI_BF16);
}
static inline int64_t ymi_pixels(const ymi_tensor* t) { return t->n * t->h * t->w; }
// binary point of the fixed-point BatchNorm statistics (igemm.hip statistics epilogue -> elementwise.hip BnFin): 37 - ceil(log2(count)), in [8, 40]
static inline int ymi_stat_fixed_point_shift(int64_t count) {
    int lg = 0;
    while (((int64_t)1 << lg) < count) ++lg;
    const int sh = 37 - lg;
    return sh < 8 ? 8 : sh > 40 ? 40 : sh;
}
// rows that ymi_bn_finalize (elementwise.hip) may stage behind the partial rows it is given when there are many: every caller sizes
// its partials with this many rows more than it writes (the conv block's statistics, first_conv.hip's forward workspace)
constexpr int BN_STAGE_ROWS = 64;
static inline size_t ymi_esize(int dtype) { return dtype == YMI_BF16 ? 2 : 4; }
// 4-element Pack accesses (8 B bf16 / 16 B f32, below) need c, ld and the base on 4-element boundaries (elementwise.hip, cbam.hip)
static inline bool vec4_ok(const ymi_tensor* t) {
    return t->c % 4 == 0 && t->ld % 4 == 0 && ((uintptr_t)t->data % (4 * ymi_esize(t->dtype))) == 0;
}
static inline bool ymi_same_shape(const ymi_tensor* a, const ymi_tensor* b) {
    return a->n == b->n && a->h == b->h && a->w == b->w && a->c == b->c;
}
// Development options (runtime.hip): named integers behind ymi_set_option / ymi_get_option - the "before" arm of a measured change, grid
// sizes for in-step sweeps, forced code paths for tests.  Each starts at its default, or at the value of the environment variable
// YMI_<NAME> when the process starts with one (tools/*.sh sweeps); production code never sets any.
enum YmiOpt {
    OPT_EW_PPT,           // streaming BatchNorm passes: pixels per thread aimed for (64)
    OPT_EW_CAP,           // ... and their workgroup cap (512)
    OPT_RED_CAP,          // BatchNorm backward reduce: workgroup cap (512)
    OPT_XCD_SHIFT,        // streaming passes work on XCD (x + k) % 8's pixels: the anti-affine arrangement (0)
    OPT_ATTN_TILED,       // 1: tiled window attention for every window size (tests) (0)
    OPT_WGRAD_BLOCKS,     // weight gradient: split-K workgroup target, 64-row tiles (1280)
    OPT_WGRAD_BLOCKS128,  // ... 128-row tiles (768)
    OPT_IGEMM_TILE_BM,    // force a GEMM tile (tools/conv_bench.py sweeps); 0: choose_tile
    OPT_IGEMM_TILE_BN,
    OPT_BN_TAIL,          // 1: BatchNorm backward's final pass inside the reduce kernel (last-arriver hand-off: measured slower,
                          //    profiles/r05_bn_tail_ab.txt); 0 (default): its own launch
    OPT_WGRAD_PATCH,      // 1 (default): the weight gradient sums pixels in patch order with scalar addressing where the map tiles; 0: raster walk
    OPT_COUNT
};
int ymi_opt(int id);
static inline int ew_ppt() { return ymi_opt(OPT_EW_PPT); }
static inline int ew_cap() { return ymi_opt(OPT_EW_CAP); }
// workgroups of a streaming pass from the uncapped count: the cap (default 512, runtime.hip), then the same number on every XCD
static inline int64_t ew_capped(int64_t gb) {
    if (gb > ew_cap()) gb = ew_cap();
    return (gb + 7) / 8 * 8;
}
// ONE grid rule for the passes whose threads keep a channel group (affine: elementwise.hip, BatchNorm backward apply: reduce_bwd.hip); a workgroup
// covers `rows` pixels at a time.  Every thread reloads its group's coefficients: give it ~ew_ppt pixels when the tensor allows.  Small maps
// (<= 13 MB here) are pure latency: with 256 blocks a thread walked 3-6 pixels one dependent round trip after the other (10 us for 1.6 MB);
// give them up to one resident round of blocks, i.e. 1-2 pixels per thread
static inline int64_t ew_blocks(int64_t P, int rows) {
    int64_t gb = (P + (int64_t)rows * ew_ppt() - 1) / ((int64_t)rows * ew_ppt());
    if (gb < 1024) gb = (P + rows - 1) / rows < 1024 ? (P + rows - 1) / rows : 1024;
    return ew_capped(gb);
}
// ONE place that turns a run-time dtype / activation into template arguments: f(TypeTag<T>{}) and f(TypeTag<T>{}, ActTag<ACT>{})
template <typename T> struct TypeTag {
    typedef T type;
};
template <int ACT> using ActTag = std::integral_constant<int, ACT>;
template <typename F> static inline void dispatch_dtype(int dtype, F&& f) {
    if (dtype == YMI_BF16) f(TypeTag<bf16_t>{});
    else f(TypeTag<float>{});
}
template <typename F> static inline void dispatch_dtype_act(int dtype, int act, F&& f) {
    dispatch_dtype(dtype, [&](auto t) {
        if (act == YMI_ACT_SILU) f(t, ActTag<YMI_ACT_SILU>{});
        else if (act == YMI_ACT_GELU) f(t, ActTag<YMI_ACT_GELU>{});
        else f(t, ActTag<YMI_ACT_NONE>{});
    });
}
// a 16-byte block of zeros in device memory (source of out-of-bounds im2col taps)
const void* ymi_zero_page();

// ---- element access helpers (device) ----------------------------------------------------------
template <typename T> struct ElemTraits;
template <> struct ElemTraits<float> {
    static constexpr int CH = 4;  // elements per 16-byte chunk
    static constexpr int DT = YMI_F32;
};
template <> struct ElemTraits<bf16_t> {
    static constexpr int CH = 8;
    static constexpr int DT = YMI_BF16;
};

__device__ __forceinline__ float to_f32(float v) { return v; }
__device__ __forceinline__ float to_f32(bf16_t v) { return (float)v; }
template <typename T> __device__ __forceinline__ T from_f32(float v);
template <> __device__ __forceinline__ float from_f32<float>(float v) { return v; }
template <> __device__ __forceinline__ bf16_t from_f32<bf16_t>(float v) { return (bf16_t)v; }  // v_cvt_pk_bf16_f32: RNE, NaN-safe

// load / store a group of G consecutive elements as floats (vector access when aligned by construction)
template <typename T, int G> struct Pack;
template <> struct Pack<float, 4> {
    static __device__ __forceinline__ void load(const float* p, float (&v)[4]) {
        f32x4 t = *reinterpret_cast<const f32x4*>(p);
        v[0] = t[0]; v[1] = t[1]; v[2] = t[2]; v[3] = t[3];
    }
    static __device__ __forceinline__ void store(float* p, const float (&v)[4]) {
        f32x4 t = {v[0], v[1], v[2], v[3]};
        *reinterpret_cast<f32x4*>(p) = t;
    }
};
template <> struct Pack<bf16_t, 4> {
    static __device__ __forceinline__ void load(const bf16_t* p, float (&v)[4]) {
        bf16x4 t = *reinterpret_cast<const bf16x4*>(p);
        v[0] = (float)t[0]; v[1] = (float)t[1]; v[2] = (float)t[2]; v[3] = (float)t[3];
    }
    static __device__ __forceinline__ void store(bf16_t* p, const float (&v)[4]) {
        bf16x4 t = {(bf16_t)v[0], (bf16_t)v[1], (bf16_t)v[2], (bf16_t)v[3]};
        *reinterpret_cast<bf16x4*>(p) = t;
    }
};
template <> struct Pack<bf16_t, 8> {
    static __device__ __forceinline__ void load(const bf16_t* p, float (&v)[8]) {
        bf16x8 t = *reinterpret_cast<const bf16x8*>(p);
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = (float)t[i];
    }
    static __device__ __forceinline__ void store(bf16_t* p, const float (&v)[8]) {
        bf16x8 t;
#pragma unroll
        for (int i = 0; i < 8; ++i) t[i] = (bf16_t)v[i];
        *reinterpret_cast<bf16x8*>(p) = t;
    }
};

// e^x as one v_exp_f32 (2^(x*log2 e)): ~1 ulp, results below 2^-126 flush to zero; no range-reduction code
// four consecutive elements as they lie in memory (8 bytes of bfloat16, 16 bytes of float32) and their conversion
template <typename T> struct Raw4;
template <> struct Raw4<bf16_t> {
    typedef bf16x4 type;
    static __device__ __forceinline__ void to_f32(const bf16x4& r, float (&v)[4]) {
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = (float)r[i];
    }
};
template <> struct Raw4<float> {
    typedef f32x4 type;
    static __device__ __forceinline__ void to_f32(const f32x4& r, float (&v)[4]) {
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = r[i];
    }
};

// Workgroups are dealt round-robin to the 8 XCDs (flat id & 7), each with its own L2.  Work units that read neighbouring bytes
// (the 16-byte channel chunks of one 128-byte line, the heads of one token row) should therefore NOT sit on consecutive flat
// ids: every XCD would fetch the whole line.  xcd_unit() turns the flat workgroup id into a work-unit index such that
// consecutive UNITS run on one XCD, back to back (a permutation of [0, total) when total % 8 == 0, the identity otherwise).
// ---- XCD ownership of the pixel axis (round 4) -----------------------------------------------------------------------------------
// A consumer finds its producer's bytes in its own XCD's L2 - 3.7-6x faster for a latency-shaped reader such as a GEMM's operand
// ring than from another XCD's L2 / the Infinity Cache (profiles/r04_xcd_affinity_probe.txt) - when both kernels give an XCD the
// same part of the tensor.  ONE rule for every kernel that walks pixels (or tokens): the XCD a workgroup runs on (flat id & 7:
// workgroups are dealt round-robin, measured stable from launch to launch) owns the pixels [x * span, (x + 1) * span) of the
// batch-major pixel order, span = ymi_xcd_span(P).  The rule is a FRACTION of the pixel order, so it lines up across resolutions
// (a stride-2 consumer's eighth of the output reads the same eighth of its input), and at batch sizes that are multiples of 8 it is
// whole images.  Placement is a speed matter only: nothing depends on it for correctness.
__host__ __device__ __forceinline__ int64_t ymi_xcd_span(int64_t P) { return (((P + 63) >> 6) + 7) >> 3 << 6; }
// the pixel range [lo, hi) of this workgroup's XCD, the workgroup's index among that XCD's workgroups and their number
// (the launch grid must be a multiple of 8 workgroups)
struct XcdRange {
    int64_t lo, hi;
    int bi, nbx;
};
int64_t ymi_xcd_span_arg(int64_t P);  // host: ymi_xcd_span(P), with the diagnostic shift of YMI_XCD_SHIFT in bits 56..58
__device__ __forceinline__ XcdRange xcd_range(int64_t P, int64_t span_arg) {
    const int id = blockIdx.x, x = ((id & 7) + (int)(span_arg >> 56)) & 7;
    const int64_t span = span_arg & ((1ll << 56) - 1);
    XcdRange r;
    r.lo = x * span;
    r.hi = r.lo + span < P ? r.lo + span : P;
    if (r.lo > P) r.lo = P;
    r.bi = id >> 3;
    r.nbx = gridDim.x >> 3;
    return r;
}

__device__ __forceinline__ int xcd_unit(int flat, int total) { return (total & 7) ? flat : (flat & 7) * (total >> 3) + (flat >> 3); }
__device__ __forceinline__ int flat_block_id() { return blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z); }

// ---- the pixel walk of the streaming BatchNorm passes (affine: elementwise.hip; backward reduce and apply: reduce_bwd.hip) ------------------------
// A thread keeps the four channels at `coff` and visits the pixels p, p + step, ... < end of one or two rows (a; b when `two`: a template fact
// in the reduce pass, which passes a constant that folds after inlining, a uniform run-time fact - is there a residual - in the affine pass).
// U pixels per trip: 2 U independent 8/16-byte loads in flight per lane before the first use; the NEXT trip's loads are issued (raw, unconverted:
// 2 VGPRs each in bf16) before this trip's arithmetic, so a workgroup with several trips does not pay one full memory round trip per trip (4 waves
// per SIMD are not enough to hide it: the arithmetic of a trip is as long as its loads).  The leftover pixels go one at a time.
// use(va, vb, p) gets pixel p's values as floats; vb is zero without a second row.
template <int U, typename T, typename F>
__device__ __forceinline__ void pixel_walk(const T* ap, int64_t lda, const T* bp, int64_t ldb, bool two, int coff, int64_t p, int64_t step, int64_t end, F&& use) {
    typedef typename Raw4<T>::type R4;
    R4 ra[U], rb[U];
    bool have = p + (U - 1) * step < end;
    if (have) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            ra[u] = *reinterpret_cast<const R4*>(ap + (p + u * step) * lda + coff);
            if (two) rb[u] = *reinterpret_cast<const R4*>(bp + (p + u * step) * ldb + coff);
        }
    }
    while (have) {
        float va[U][4], vb[U][4] = {};
#pragma unroll
        for (int u = 0; u < U; ++u) {
            Raw4<T>::to_f32(ra[u], va[u]);
            if (two) Raw4<T>::to_f32(rb[u], vb[u]);
        }
        const int64_t pc = p;
        p += U * step;
        have = p + (U - 1) * step < end;
        if (have) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                ra[u] = *reinterpret_cast<const R4*>(ap + (p + u * step) * lda + coff);
                if (two) rb[u] = *reinterpret_cast<const R4*>(bp + (p + u * step) * ldb + coff);
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) use(va[u], vb[u], pc + u * step);
    }
    for (; p < end; p += step) {
        float va[4], vb[4] = {0.f, 0.f, 0.f, 0.f};
        Pack<T, 4>::load(ap + p * lda + coff, va);
        if (two) Pack<T, 4>::load(bp + p * ldb + coff, vb);
        use(va, vb, p);
    }
}

__device__ __forceinline__ float fast_exp(float x) { return __builtin_amdgcn_exp2f(x * 1.44269504088896340736f); }
// 1 / (1 + e^-x) with v_exp_f32 + v_rcp_f32 (each ~1 ulp) instead of the IEEE division sequence
__device__ __forceinline__ float sigmoidf_(float x) { return __builtin_amdgcn_rcpf(1.0f + fast_exp(-x)); }
__device__ __forceinline__ float silu_f(float x) { return x * sigmoidf_(x); }
__device__ __forceinline__ float silu_grad_f(float x) {
    float s = sigmoidf_(x);
    return s * (1.0f + x * (1.0f - s));
}
// erf(z) by Abramowitz & Stegun 7.1.26: 1 - (a1 t + .. + a5 t^5) e^(-z^2), t = 1 / (1 + p |z|); absolute error <= 1.5e-7 - float32 noise
// next to the 1 the GELU adds it to - in 6 multiply-adds, v_rcp_f32 and v_exp_f32.  libm's erff is ~45 instructions with two branches
// that a wave executes both of; in the Swin MLP's GEMM epilogues (32768 activations per 256 x 128 tile) that was as long as the K loop.
// e2 (optional): receives e^(-z^2), which GELU's derivative needs as well.
__device__ __forceinline__ float erf_as(float z, float* e2 = nullptr) {
    const float az = fabsf(z);
    const float t = __builtin_amdgcn_rcpf(1.0f + 0.3275911f * az);
    const float e = fast_exp(-az * az);
    float p = 1.061405429f;
    p = p * t - 1.453152027f;
    p = p * t + 1.421413741f;
    p = p * t - 0.284496736f;
    p = p * t + 0.254829592f;
    if (e2) *e2 = e;
    return copysignf(1.0f - p * t * e, z);
}
__device__ __forceinline__ float gelu_f(float x) { return 0.5f * x * (1.0f + erf_as(x * 0.70710678118654752440f)); }
__device__ __forceinline__ float gelu_grad_f(float x) {
    const float c = 0.39894228040143267794f;  // 1/sqrt(2 pi)
    float e;                                   // e^(-x^2 / 2)
    const float er = erf_as(x * 0.70710678118654752440f, &e);
    return 0.5f * (1.0f + er) + x * c * e;
}
template <int ACT> __device__ __forceinline__ float apply_act(float x) {
    if (ACT == YMI_ACT_SILU) return silu_f(x);
    if (ACT == YMI_ACT_GELU) return gelu_f(x);
    return x;
}
__device__ __forceinline__ float apply_act_rt(float x, int act) {
    return act == YMI_ACT_SILU ? silu_f(x) : act == YMI_ACT_GELU ? gelu_f(x) : x;
}
template <int ACT> __device__ __forceinline__ float act_grad(float x) {
    if (ACT == YMI_ACT_SILU) return silu_grad_f(x);
    if (ACT == YMI_ACT_GELU) return gelu_grad_f(x);
    return 1.0f;
}
__device__ __forceinline__ float act_grad_rt(float x, int act) {
    return act == YMI_ACT_SILU ? silu_grad_f(x) : act == YMI_ACT_GELU ? gelu_grad_f(x) : 1.0f;
}

// uint8 -> float32 / 255, correctly rounded (bit-identical to img.float() / 255) without the IEEE division sequence: q = u * fl(1/255) is
// within an ulp of the quotient, the residual u - 255 q is exact in one fma, and one correction step lands on the rounded quotient for
// every u in [0, 255] (resize.hip, augment.hip; tests/test_gpu_resize.py compares all 256 values with torch's division).
__device__ __forceinline__ float unit_of_byte(uint32_t u) {
    const float f = (float)u, rc = 1.0f / 255.0f;
    const float q = f * rc;
    const float r = __builtin_fmaf(-q, 255.0f, f);
    return __builtin_fmaf(r, rc, q);
}

// ATen's area_pixel_compute_source_index (align_corners = false, bilinear) and the neighbour / weight rule of upsample_bilinear2d.  Its users
// (resize.hip, maskdec.hip) are compiled with -ffp-contract=off: the coordinate must round as a product and a difference (resize.hip's head).
struct Tap {
    int i0, i1;
    float l0, l1;
};
__device__ __forceinline__ Tap tap_of(int dst, float scale, int in) {
    float s = ((float)dst + 0.5f) * scale - 0.5f;
    s = s < 0.0f ? 0.0f : s;
    Tap t;
    t.i0 = (int)s;  // (s >= 0: truncation is floor)
    t.i0 = t.i0 > in - 1 ? in - 1 : t.i0;  // (never taken for hs <= Hp sizes that ATen accepts; keeps every read in bounds whatever scale is passed)
    t.i1 = t.i0 + (t.i0 < in - 1 ? 1 : 0);
    t.l1 = s - (float)t.i0;
    t.l0 = 1.0f - t.l1;
    return t;
}

// ---- in-launch hand-offs between workgroups (round 5)----------------------------------------------------------------------------
// The per-XCD L2s are not coherent and a CU's L1 is never refreshed by another CU's stores, so a workgroup that consumes another
// workgroup's bytes INSIDE a launch needs them written through and read past its L1.  The form used here (MI355X_MICROARCH.md,
// "Valid forms", first table row; cdna_hip_programming.md Guideline 16 R1): every handed-off byte is stored with an agent-scope relaxed
// atomic store (global_store ... sc1: write-through, no release fence), every storing wave drains with s_waitcnt vmcnt(0), the workgroup
// meets at a barrier, ONE lane takes a ticket with an agent-scope relaxed fetch-add, and the workgroup whose add returned the last
// ticket reads the bytes with agent-scope relaxed atomic loads (global_load ... sc1: past L1).  No __threadfence(), no buffer_wbl2, no
// buffer_inv anywhere: round 4's form of the same idea (every thread of every workgroup fencing twice) cost 130 us per launch.
// Results never depend on who arrives last: the combining workgroup sums fixed rows in fixed order.
__device__ __forceinline__ void st_wt(float* p, float v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st_wt2(float* p, float a, float b) {  // 8-byte aligned pair
    const uint64_t v = (uint64_t)__builtin_bit_cast(uint32_t, a) | ((uint64_t)__builtin_bit_cast(uint32_t, b) << 32);
    __hip_atomic_store(reinterpret_cast<uint64_t*>(p), v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_wt(double* p, double v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ float ld_wt(const float* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ double ld_wt(const double* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void ld_wt2(const float* p, float& a, float& b) {
    const uint64_t v = __hip_atomic_load(reinterpret_cast<const uint64_t*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    a = __builtin_bit_cast(float, (uint32_t)v);
    b = __builtin_bit_cast(float, (uint32_t)(v >> 32));
}
// Ticket: call from EVERY thread of the workgroup after the write-through stores.  `flag` is one LDS word nothing else uses until the
// second barrier.  Returns (workgroup-uniform) whether this workgroup drew ticket `last`; that workgroup also resets the counter, so
// counters are zero between launches (they start zero: __device__ storage, runtime.hip).
__device__ __forceinline__ bool ticket_is_last(unsigned* counter, unsigned last, int* flag) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's write-through stores have left
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned t = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (t == last) __hip_atomic_store(counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // every workgroup has drawn
        *flag = t == last;
    }
    __syncthreads();
    return *flag != 0;
}
// ---- the final pass of a BatchNorm backward: ONE body for its own launch and for the rider (reduce_bwd.hip, wgrad.hip) --------------------
// gamma / beta of the channels >= split come from a second pair of arrays (two BatchNorms behind one convolution: Detect's sibling
// branches run as one, head.py:71-72); split == 0: one pair
struct GammaBeta2 {
    const float* gamma;
    const float* beta;
    int split;
};
// coefficients of the BN backward apply pass, from the finished sums (one set per channel):
//   z = x*a0 + a1 ;  draw = dy*act'(z)*c0 - x*c1 - c2
struct BnCoefArgs {
    const float* gamma;
    const float* beta;
    const float* mean;
    const float* inv;
    float inv_count;
    float* coef;  // [5][C] or nullptr
    GammaBeta2 g2;
};
// the one statement of the apply pass's arithmetic (reduce_bwd.hip: bn_act_bwd_apply_kernel; wgrad.hip: conv1x1_bwd_kernel, which forms draw on its
// operand path): draw = dout * act'(raw * a0 + a1) * c0 - (raw * c1 + c2)
template <int ACT> __device__ __forceinline__ float bn_bwd_apply_one(float d, float x, float a0, float a1, float c0, float c1, float c2) {
    const float dz = d * act_grad<ACT>(x * a0 + a1);
    return dz * c0 - (x * c1 + c2);
}
// a final pass: sum `blocks` partial rows [block][2][C] per channel into out0 (dbeta) / out1 (dgamma), either may be null, and derive bn.coef
struct BnFinal {
    const float* part;
    int blocks, C;
    float* out0;
    float* out1;
    BnCoefArgs bn;
};
// the one statement of "channel >= split takes the second pair, a null pointer means 1 / 0"
__device__ __forceinline__ void bn_affine_of(const float* gamma, const float* beta, const GammaBeta2& g2, int c, float& ga, float& be) {
    const bool second = g2.split > 0 && c >= g2.split;
    const float* gp = second ? g2.gamma : gamma;
    const float* bp = second ? g2.beta : beta;
    const int pc = second ? c - g2.split : c;
    ga = gp ? gp[pc] : 1.0f;
    be = bp ? bp[pc] : 0.0f;
}
// the per-channel parameters the coefficients need (fetched apart from the formulas: the final pass fetches them beside its partial rows)
struct BnChan {
    float ga, be, inv, mean;
};
__device__ __forceinline__ void bn_chan_fetch(const BnCoefArgs& bn, int c, BnChan& p) {
    bn_affine_of(bn.gamma, bn.beta, bn.g2, c, p.ga, p.be);
    p.inv = bn.inv[c];
    p.mean = bn.mean[c];
}
// the one statement of the five coefficients
__device__ __forceinline__ void bn_coef_write(const BnCoefArgs& bn, int C, int c, const BnChan& p, float s0, float s1) {
    const float ga = p.ga, be = p.be;
    const float p0 = p.inv, p1 = -p.mean * p0;
    const float k1 = s0 * bn.inv_count, k2 = s1 * bn.inv_count;
    bn.coef[0 * C + c] = p0 * ga;
    bn.coef[1 * C + c] = p1 * ga + be;
    bn.coef[2 * C + c] = ga * p0;
    bn.coef[3 * C + c] = ga * p0 * p0 * k2;
    bn.coef[4 * C + c] = ga * p0 * (k1 + p1 * k2);
}
// ---- the train-mode statistics rule (elementwise.hip: bn_finalize_kernel and the affine pass's prologue) -----------------------------------------
// from the sums of x and x^2 over `count` pixels: mean, clamped variance, 1 / sqrt(var + eps), all in double.  (The momentum step of the running
// statistics stays written out at both callers: under -ffp-contract=fast its two products and their sum come out fused for some channels and not for
// others, differently for every shape of the code around them, and the stored words follow - profiles/bnstream_refactor_ab.txt.)
struct BnStat {
    double mean, var;
    float inv;
};
__device__ __forceinline__ BnStat bn_stat_of(double sum, double sumsq, double count, float eps) {
    BnStat s;
    s.mean = sum / count;
    s.var = sumsq / count - s.mean * s.mean;
    if (s.var < 0.0) s.var = 0.0;
    s.inv = (float)(1.0 / sqrt(s.var + (double)eps));
    return s;
}
// Workgroup w of NT threads (1024: chan_reduce_final_kernel; 256: a weight-gradient launch's rider workgroups) owns channels [32 w, 32 w + 32).
// The partial rows go to 32 row slices (slice s: rows s, s + 32, ...); a thread plays 1024 / NT of them for its channel.  Per slice: four
// float chains per output at rows b, b + 32, b + 64, b + 96 stepping 128 (loads in flight), the tail steps 32 into the first chain, combined
// as ((a + b) + (c + d)) in double; the slice-0 threads sum the 32 slices in slice order in double and store floats.  The order is the same
// for every NT, so a step gives the same gradients whether its final passes ride or not.  red: [2][32][33] doubles of LDS.
// PREFETCH: the per-channel parameters of the coefficients are fetched before the partial rows, not behind the barrier (the pass is a chain
// of load latencies: there they were a round trip of their own).  Moves no value.  The rider leaves it off: with it the weight-gradient kernels
// with the fewest registers lose a wave per SIMD (profiles/bnfinal_refactor_ab.txt).
constexpr int BN_FINAL_RED = 2 * 32 * 33;  // doubles
template <int NT, bool PREFETCH = true> __device__ __forceinline__ void bn_final_block(const BnFinal& f, int w, double* red) {
    static_assert(NT == 1024 || NT == 256, "32 channels x 32 or 8 thread rows");
    constexpr int SPT = 1024 / NT;  // slices per thread
    const int cl = threadIdx.x & 31, grp = threadIdx.x >> 5;
    const int c = w * 32 + cl, C = f.C;
    BnChan p{1.0f, 0.0f, 0.f, 0.f};
    if (PREFETCH && grp == 0 && c < C && f.bn.coef) bn_chan_fetch(f.bn, c, p);
    int es = 0;
#pragma unroll
    do {  // (a do loop: as a for loop the one-slice form came out of the compiler with two more VGPRs than the loop-free kernel it replaces)
        const int slice = grp * SPT + es;
        double s0 = 0.0, s1 = 0.0;
        if (c < C) {
            float a0 = 0.f, a1 = 0.f, b0 = 0.f, b1 = 0.f, c0 = 0.f, c1 = 0.f, d0 = 0.f, d1 = 0.f;
            int b = slice;
            for (; b + 96 < f.blocks; b += 128) {
                a0 += f.part[((int64_t)b * 2 + 0) * C + c];
                a1 += f.part[((int64_t)b * 2 + 1) * C + c];
                b0 += f.part[((int64_t)(b + 32) * 2 + 0) * C + c];
                b1 += f.part[((int64_t)(b + 32) * 2 + 1) * C + c];
                c0 += f.part[((int64_t)(b + 64) * 2 + 0) * C + c];
                c1 += f.part[((int64_t)(b + 64) * 2 + 1) * C + c];
                d0 += f.part[((int64_t)(b + 96) * 2 + 0) * C + c];
                d1 += f.part[((int64_t)(b + 96) * 2 + 1) * C + c];
            }
            for (; b < f.blocks; b += 32) {
                a0 += f.part[((int64_t)b * 2 + 0) * C + c];
                a1 += f.part[((int64_t)b * 2 + 1) * C + c];
            }
            s0 = ((double)a0 + (double)b0) + ((double)c0 + (double)d0);
            s1 = ((double)a1 + (double)b1) + ((double)c1 + (double)d1);
        }
        red[(0 * 32 + slice) * 33 + cl] = s0;
        red[(1 * 32 + slice) * 33 + cl] = s1;
    } while (++es < SPT);
    __syncthreads();
    if (grp == 0 && c < C) {
        double a0 = 0.0, a1 = 0.0;
#pragma unroll
        for (int q = 0; q < 32; ++q) {
            a0 += red[(0 * 32 + q) * 33 + cl];
            a1 += red[(1 * 32 + q) * 33 + cl];
        }
        if (f.out0) f.out0[c] = (float)a0;
        if (f.out1) f.out1[c] = (float)a1;
        if (f.bn.coef) {
            if (!PREFETCH) bn_chan_fetch(f.bn, c, p);
            bn_coef_write(f.bn, C, c, p, (float)a0, (float)a1);
        }
    }
}
// ---- ... riding in a weight-gradient launch (round 5; wgrad.hip, reduce_bwd.hip) -------------------------------------------------------------
// The final pass of a BatchNorm backward (sum <= 512 partial rows per channel, derive the apply pass's coefficients) is a 1-16 workgroup
// kernel at a dependent-launch latency (~5.4 us, 57 times a step), and it cannot move into its producer or its consumer (a hand-off level
// costs ~2.5 us, profiles/r05_bn_tail_ab.txt).  But the weight-gradient GEMM of the PREVIOUS layer of the backward pass is independent of it
// and sits right beside it in the stream: with ymi_wgrad_hold(1) a deferred weight-gradient launch is held back until the next BatchNorm
// backward has issued its reduce pass and then launched with that layer's final pass - bn_final_block, the same function its own launch
// calls - as extra workgroups at the front of its grid.
struct BnRider {
    BnFinal f;
    int nwg;  // rider workgroups at the front of the grid (a multiple of 8: the XCD dealing of the rest is unchanged); 0: none
};
// issue the weight-gradient launch held on `stream` (and the current device) with final pass `f` riding in it -> true; false when nothing is
// held there (the caller launches its final pass itself)
bool ymi_wgrad_issue_held(const BnFinal* f, hipStream_t stream);

// ---- entry points one source file offers another (host) ---------------------------------------------------------------------------
// profile.hip: per-launch roofline records of the GEMM families (igemm.hip, wgrad.hip)
bool ymi_prof_enabled();
int ymi_prof_start(hipStream_t stream, int family, double flop, double bytes, double peak_tflops);
void ymi_prof_stop(hipStream_t stream, int idx);
// igemm.hip: one GEMM launch from filled arguments; the raw convolution with fixed-point statistics behind ymi_conv2d_bn_silu_fwd_acc (elementwise.hip)
struct IgemmArgs;
int ymi_launch_igemm(const IgemmArgs& a, int dtype, bool stats, int* host_blocks, hipStream_t stream);
int ymi_conv2d_fwd_statacc(const ymi_tensor* x, const void* w_packed, int64_t cout, int64_t kh, int64_t kw, int64_t stride, const ymi_tensor* y,
                           long long* stat_acc, void* stream);

// reduce_bwd.hip: the final pass as its own launch - column sums (out0 / out1, either may be null) and a BatchNorm backward's whose first
// stage ran elsewhere (first_conv.hip)
int ymi_chan_reduce_final(const float* part, int blocks, int C, float* out0, float* out1, hipStream_t stream);
int ymi_bn_bwd_final(const float* part, int blocks, int C, const float* gamma, const float* beta, const float* mean, const float* inv, float inv_count,
                     float* dgamma, float* dbeta, float* coef, hipStream_t stream);

// reduce_bwd.hip: a BatchNorm + activation backward up to the apply pass's coefficients - the reduce pass and the final pass (riding in a held
// weight-gradient launch when there is one).  dgamma / dbeta are written; *coef points at [a0 | a1 | c0 | c1 | c2][C] inside `workspace`
// (ymi_bn_act_bwd's size), valid for later launches of `stream` until the workspace is reused.
int ymi_bn_act_bwd_coef(const ymi_tensor* dout, const ymi_tensor* raw, const float* gamma, const float* save_mean, const float* save_invstd, const float* beta,
                        GammaBeta2 g2, int32_t act, float* dgamma, float* dbeta, void* workspace, size_t workspace_bytes, hipStream_t stream, const float** coef);

// wgrad.hip: the record ymi_wgrad_reduce_batch sums the slabs of one launch from ([splits][elems] slabs, elems = padded Cout * ng, a multiple of 8;
// first_block is filled in by the batched sum).  It sets the sum's geometry: more interleaved split chains per output element the more splits there are,
// and one 16-byte load per lane and split - 8 elements of a bfloat16 slab, 4 of a float32 one.  (first_conv.hip's backward writes such slabs too.)
ymi_wgrad_pending ymi_wgrad_record(const void* slab, float* dw, int64_t elems, int splits, int ng, int cin, int cout_real, int cin_real, int ntaps,
                                   bool slab_bf16, const float* bias_slab, float* dbias);

// a slot of 64 ticket counters for one launch (host; round-robin over 1024 slots, zero between launches)
unsigned* ymi_ticket_slot();

// retire all but the N youngest vector-memory operations of this wave, then meet the workgroup: bytes written
// to LDS by LDS-DMA (global_load_lds) are readable by other waves only after BOTH (counted wait, then barrier).
template <int N> __device__ __forceinline__ void wait_vmcnt_barrier() {
    asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"(N) : "memory");
}

// ---- the swizzled [row][column] bfloat16 LDS image that ds_read_b64_tr_b16 reads transposed (wgrad.hip, first_conv.hip) ---------------------
// A fragment = 8 consecutive ROWS (8g .. 8g + 7 of a 32-row block, g = lane / 16) of column c0 + lane % 16, by two transposed 8-byte reads.
// The instruction is serviced per 32-lane half: 2 groups x (4 rows x 4 eight-byte units); the 8 rows of a half are {r0..r0+3, r0+8..r0+11}.
// With 64-, 128- or 256-byte rows those rows share banks on the plain image, so the 8-byte unit index is XORed with a per-row value that
// spreads them over the 32 unit slots of a 256-byte bank row: position (r, u ^ (tr_swz<SW>(r) << 2)) holds unit u of row r, for writers and
// readers alike.  The XOR never touches bit 0 of the unit index: it permutes 16-byte chunks (chunk ^ (tr_swz << 1)) and can be applied to the
// source address of an LDS-DMA piece.  Wider rows take mode 1 (the XOR stays inside each 256-byte bank row).
// SW by the row width (tr_swz_mode): 0 = 128-byte rows (2 bits), 1 = 256-byte and wider rows (3 bits), 2 = 64-byte rows (rows r and r + 8 of a half share
// banks, rows r .. r + 3 do not: one bit)
constexpr int tr_swz_mode(int row_bytes) { return row_bytes >= 256 ? 1 : row_bytes == 64 ? 2 : 0; }
template <int SW> __device__ __forceinline__ int tr_swz(int row) {
    return SW == 1 ? ((row & 3) | (((row >> 3) & 1) << 2)) : SW == 2 ? ((row >> 3) & 1) : (((row >> 1) & 1) | (((row >> 3) & 1) << 1));
}
// the two read addresses (LDS) of a lane's fragment, rows r_lo and r_lo + 4, in an image with `rowb` bytes per row; each file reads them in
// its own instruction form
struct TrFragAddr {
    lptr_t lo, hi;
};
template <int SW> __device__ __forceinline__ TrFragAddr tr_frag_addr(const char* img, int rowb, int c0, int lane) {
    const int g = lane >> 4, i = lane & 15, q = i >> 2, p = i & 3;
    const int r_lo = 8 * g + q, r_hi = r_lo + 4;
    const int u = (c0 >> 2) + p;  // logical 8-byte unit of this lane's 4 columns
    const int u_lo = u ^ (tr_swz<SW>(r_lo) << 2), u_hi = u ^ (tr_swz<SW>(r_hi) << 2);
    return TrFragAddr{(lptr_t)(img + r_lo * rowb + u_lo * 8), (lptr_t)(img + r_hi * rowb + u_hi * 8)};
}

// sum of a value over the 16 lanes of its DPP row, result in every lane: xor-1 and xor-2 quad permutes, then the half-row and
// row mirrors (each lane already holds its quad's / half-row's total, so the mirrored partner supplies the other one)
// (igemm.hip's statistics epilogue, first_conv.hip's reducing passes)
template <int CTRL> __device__ __forceinline__ float dpp_add(float v) {
    return v + __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, true));
}
__device__ __forceinline__ float row16_sum(float v) {
    v = dpp_add<0xB1>(v);   // quad_perm [1,0,3,2]
    v = dpp_add<0x4E>(v);   // quad_perm [2,3,0,1]
    v = dpp_add<0x141>(v);  // row_half_mirror
    v = dpp_add<0x140>(v);  // row_mirror
    return v;
}
// two floats rounded to bfloat16 in one word, the first in the low half (v_cvt_pk_bf16_f32; swin_mlp.hip, first_conv.hip)
__device__ __forceinline__ uint32_t pack_bf16x2(float a, float b) {
    typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
    const bf16x2 v = {(bf16_t)a, (bf16_t)b};
    return __builtin_bit_cast(uint32_t, v);
}

// wave-level reductions (64 lanes)
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
