// Image rescaling around the model, one read-once / write-once launch each:
//   scale_image_kernel : F.interpolate(mode="bilinear", align_corners=False) of an NCHW uint8 / float32 batch, with the uint8 -> float / 255
//                        conversion before it, the left-right / up-down flip before that and F.pad(value) to the right and below it
//                        (reference utils/torch_utils.py:475-495 scale_img, models/yolo/detect/train.py:100-114 preprocess_batch, and the
//                        x.flip(3) of nn/tasks.py:392), all in the one pass that writes the float32 NCHW destination
//   tta_merge_kernel   : _descale_pred + _clip_augmented + torch.cat of nn/tasks.py:394-439 on up to three decoded Detect outputs
// Both only enqueue on the stream they are given (no allocation, no synchronisation): graph-capturable like the rest of the library.
// This file is compiled with -ffp-contract=off (Makefile): the source coordinate (dst + 0.5) * scale - 0.5 must round as a product and a
// difference, as the plain float32 statement of ATen's formula does; contracted into one fma the coordinate - and with it the weight - moves
// by up to half an ulp OF THE COORDINATE (3e-5 at x = 600), which is above the 1e-5 the interpolated pixels are held to.
#include "common.h"

namespace {

constexpr int RS_THREADS = 256;
constexpr int RS_PX = 4;  // consecutive output pixels of a row per lane: one 16-byte store

// uint8 -> float32 / 255, correctly rounded (bit-identical to img.float() / 255) without the IEEE division sequence: q = u * fl(1/255) is
// within an ulp of the quotient, the residual u - 255 q is exact in one fma, and one correction step lands on the rounded quotient for
// every u in [0, 255] (tests/test_gpu_resize.py compares all 256 values with torch's division).
__device__ __forceinline__ float unit_of_byte(uint32_t u) {
    const float f = (float)u, rc = 1.0f / 255.0f;
    const float q = f * rc;
    const float r = __builtin_fmaf(-q, 255.0f, f);
    return __builtin_fmaf(r, rc, q);
}

template <typename T, bool NORM> __device__ __forceinline__ float px(const T* p) {
    if constexpr (sizeof(T) == 1) return NORM ? unit_of_byte(*p) : (float)*p;
    else return *p;
}

// RS_PX consecutive source elements with one aligned load (4 bytes of uint8, 16 of float32)
template <typename T, bool NORM> __device__ __forceinline__ void load_group(const T* p, float (&v)[RS_PX]) {
    if constexpr (sizeof(T) == 1) {
        const uint32_t w = *reinterpret_cast<const uint32_t*>(p);
#pragma unroll
        for (int i = 0; i < RS_PX; ++i) {
            const uint32_t b = (w >> (8 * i)) & 255u;
            v[i] = NORM ? unit_of_byte(b) : (float)b;
        }
    } else {
        const f32x4 w = *reinterpret_cast<const f32x4*>(p);
#pragma unroll
        for (int i = 0; i < RS_PX; ++i) v[i] = w[i];
    }
}

// ATen's area_pixel_compute_source_index (align_corners = false, bilinear) and the neighbour / weight rule of upsample_bilinear2d
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

struct ScaleArgs {
    const void* src;
    float* dst;
    int H, W, Hp, Wp, hs, ws;
    int wgroups;       // ceil(Wp / 4)
    int64_t total;     // planes * Hp * wgroups lanes of work
    float sy, sx, pad;
    int flip_lr, flip_ud;
    int vec_store;     // Wp % 4 == 0 and dst 16-byte aligned: every group is one aligned 16-byte store
    int vec_load;      // identity width, no left-right flip, W % 4 == 0 and src aligned to 4 elements: a group's sources are one aligned load
};

// One lane: RS_PX consecutive pixels of one destination row.  Interpolated pixels (x < ws, y < hs), padding (the rest) and the row tail
// (x >= Wp when Wp % 4 != 0) are told apart per pixel, so sizes such as ws = 531 in Wp = 544 need no second launch and no fill before.
// IDENT (hs == H and ws == W): the converted source itself, no arithmetic on it.
template <typename T, bool NORM, bool IDENT> __global__ __launch_bounds__(RS_THREADS) void scale_image_kernel(ScaleArgs a) {
    const int64_t gid = (int64_t)blockIdx.x * RS_THREADS + threadIdx.x;
    if (gid >= a.total) return;
    const int xg = (int)(gid % a.wgroups);
    const int64_t row = gid / a.wgroups;
    const int y = (int)(row % a.Hp);
    const int64_t plane = row / a.Hp;
    const T* sp = static_cast<const T*>(a.src) + plane * a.H * a.W;
    float* dp = a.dst + (plane * a.Hp + y) * a.Wp;
    const int x0 = xg * RS_PX;
    float v[RS_PX];
#pragma unroll
    for (int i = 0; i < RS_PX; ++i) v[i] = a.pad;
    if (y < a.hs) {
        if (IDENT) {
            const int ys = a.flip_ud ? a.H - 1 - y : y;
            const T* r = sp + (int64_t)ys * a.W;
            if (a.vec_load) {  // (W % 4 == 0: a group lies wholly inside the source row or wholly in the padding)
                if (x0 < a.ws) load_group<T, NORM>(r + x0, v);
            } else {
#pragma unroll
                for (int i = 0; i < RS_PX; ++i) {
                    const int x = x0 + i;
                    if (x < a.ws) v[i] = px<T, NORM>(r + (a.flip_lr ? a.W - 1 - x : x));
                }
            }
        } else {
            const Tap ty = tap_of(y, a.sy, a.H);
            const T* r0 = sp + (int64_t)(a.flip_ud ? a.H - 1 - ty.i0 : ty.i0) * a.W;
            const T* r1 = sp + (int64_t)(a.flip_ud ? a.H - 1 - ty.i1 : ty.i1) * a.W;
#pragma unroll
            for (int i = 0; i < RS_PX; ++i) {
                const int x = x0 + i;
                if (x < a.ws) {
                    const Tap tx = tap_of(x, a.sx, a.W);
                    const int c0 = a.flip_lr ? a.W - 1 - tx.i0 : tx.i0, c1 = a.flip_lr ? a.W - 1 - tx.i1 : tx.i1;
                    const float p00 = px<T, NORM>(r0 + c0), p01 = px<T, NORM>(r0 + c1), p10 = px<T, NORM>(r1 + c0), p11 = px<T, NORM>(r1 + c1);
                    v[i] = ty.l0 * (tx.l0 * p00 + tx.l1 * p01) + ty.l1 * (tx.l0 * p10 + tx.l1 * p11);
                }
            }
        }
    }
    if (a.vec_store) {
        const f32x4 o = {v[0], v[1], v[2], v[3]};
        *reinterpret_cast<f32x4*>(dp + x0) = o;
    } else {
#pragma unroll
        for (int i = 0; i < RS_PX; ++i)
            if (x0 + i < a.Wp) dp[x0 + i] = v[i];
    }
}

template <typename T, bool NORM> void launch_scale(const ScaleArgs& a, bool ident, unsigned blocks, hipStream_t s) {
    if (ident) hipLaunchKernelGGL((scale_image_kernel<T, NORM, true>), dim3(blocks), dim3(RS_THREADS), 0, s, a);
    else hipLaunchKernelGGL((scale_image_kernel<T, NORM, false>), dim3(blocks), dim3(RS_THREADS), 0, s, a);
}

constexpr int TTA_MAX = 3;
struct TtaArgs {
    const float* src[TTA_MAX];
    int anchors[TTA_MAX];  // A_i: the source's row length
    int lo[TTA_MAX];       // first anchor taken
    int start[TTA_MAX];    // where its anchors begin in an output row
    float scale[TTA_MAX], img_h[TTA_MAX], img_w[TTA_MAX];
    int flip[TTA_MAX];
    int n, rows, total;    // sources, 4 + nc, output anchors
    float* out;
};

// grid (ceil(total / RS_THREADS), rows, batch): one output element per lane, rows of consecutive lanes
__global__ __launch_bounds__(RS_THREADS) void tta_merge_kernel(TtaArgs a) {
    const int j = blockIdx.x * RS_THREADS + threadIdx.x;
    if (j >= a.total) return;
    const int r = blockIdx.y, b = blockIdx.z;
    int k = 0;
#pragma unroll
    for (int i = 1; i < TTA_MAX; ++i)
        if (i < a.n && j >= a.start[i]) k = i;
    float v = a.src[k][((int64_t)b * a.rows + r) * a.anchors[k] + a.lo[k] + (j - a.start[k])];
    if (r < 4) {  // p[:, :4] /= scale, then x -> W - x (flip 3) / y -> H - y (flip 2)
        v = v / a.scale[k];
        if (r == 0 && a.flip[k] == 3) v = a.img_w[k] - v;
        if (r == 1 && a.flip[k] == 2) v = a.img_h[k] - v;
    }
    a.out[((int64_t)b * a.rows + r) * a.total + j] = v;
}

}  // namespace

extern "C" int ymi_scale_image(const void* src, int32_t src_uint8, int64_t planes, int64_t h, int64_t w, float* dst, int64_t hp, int64_t wp, int64_t hs,
                               int64_t ws, float pad_value, int32_t normalize, int32_t flip_lr, int32_t flip_ud, void* stream) {
    YMI_CHECK_ARG(src && dst, "scale_image: null pointer");
    YMI_CHECK_ARG(planes > 0 && h > 0 && w > 0 && hp > 0 && wp > 0, "scale_image: bad shape");
    YMI_CHECK_ARG(hs > 0 && ws > 0 && hs <= hp && ws <= wp, "scale_image: the interpolated size %lld x %lld must lie within the destination %lld x %lld",
                  (long long)hs, (long long)ws, (long long)hp, (long long)wp);
    YMI_CHECK_ARG(h < (1 << 24) && w < (1 << 24) && hp < (1 << 24) && wp < (1 << 24), "scale_image: sides must stay below 2^24 (float32 coordinates)");
    YMI_CHECK_ARG(!normalize || src_uint8, "scale_image: the / 255 conversion belongs to uint8 sources");
    if (((uintptr_t)dst & 3) || (!src_uint8 && ((uintptr_t)src & 3))) {
        ymi_set_error("scale_image: float32 pointers need 4-byte alignment");
        return YMI_EALIGN;
    }
    ScaleArgs a;
    a.src = src;
    a.dst = dst;
    a.H = (int)h; a.W = (int)w; a.Hp = (int)hp; a.Wp = (int)wp; a.hs = (int)hs; a.ws = (int)ws;
    a.wgroups = (int)((wp + RS_PX - 1) / RS_PX);
    a.total = planes * hp * a.wgroups;
    a.sy = (float)h / (float)hs;  // ATen area_pixel_compute_scale with a size (no scale_factor) given
    a.sx = (float)w / (float)ws;
    a.pad = pad_value;
    a.flip_lr = flip_lr != 0;
    a.flip_ud = flip_ud != 0;
    const bool ident = hs == h && ws == w;
    const size_t esz = src_uint8 ? 1 : 4;
    a.vec_store = wp % RS_PX == 0 && ((uintptr_t)dst & 15) == 0;
    a.vec_load = ident && !a.flip_lr && w % RS_PX == 0 && ((uintptr_t)src & (RS_PX * esz - 1)) == 0;
    const int64_t blocks = (a.total + RS_THREADS - 1) / RS_THREADS;
    YMI_CHECK_ARG(blocks < ((int64_t)1 << 31), "scale_image: destination too large for one launch");
    hipStream_t s = (hipStream_t)stream;
    if (!src_uint8) launch_scale<float, false>(a, ident, (unsigned)blocks, s);
    else if (normalize) launch_scale<uint8_t, true>(a, ident, (unsigned)blocks, s);
    else launch_scale<uint8_t, false>(a, ident, (unsigned)blocks, s);
    YMI_CHECK_LAUNCH("scale_image");
    return YMI_OK;
}

extern "C" int ymi_tta_merge(int32_t n, const float* const* src, const int64_t* anchors, const int64_t* lo, const int64_t* hi, const float* scale,
                             const int32_t* flip, const int64_t* img_h, const int64_t* img_w, int64_t batch, int64_t rows, float* out, void* stream) {
    YMI_CHECK_ARG(n >= 1 && n <= TTA_MAX, "tta_merge: 1 to %d sources", TTA_MAX);
    YMI_CHECK_ARG(src && anchors && lo && hi && scale && flip && img_h && img_w && out, "tta_merge: null pointer");
    YMI_CHECK_ARG(batch > 0 && batch < 65536 && rows >= 4 && rows < 65536, "tta_merge: batch and 4 + nc must lie in [1, 65535] ([4, 65535])");
    TtaArgs a = {};
    int64_t total = 0;
    for (int i = 0; i < n; ++i) {
        YMI_CHECK_ARG(src[i] && ((uintptr_t)src[i] & 3) == 0, "tta_merge: source %d is null or misaligned", i);
        YMI_CHECK_ARG(anchors[i] > 0 && anchors[i] < ((int64_t)1 << 31) && 0 <= lo[i] && lo[i] <= hi[i] && hi[i] <= anchors[i],
                      "tta_merge: anchor range [%lld, %lld) of source %d outside [0, %lld]", (long long)lo[i], (long long)hi[i], i, (long long)anchors[i]);
        YMI_CHECK_ARG(flip[i] == 0 || flip[i] == 2 || flip[i] == 3, "tta_merge: flip code %d (0, 2 = up-down, 3 = left-right)", flip[i]);
        YMI_CHECK_ARG(scale[i] > 0.0f, "tta_merge: scale must be positive");
        a.src[i] = src[i];
        a.anchors[i] = (int)anchors[i];
        a.lo[i] = (int)lo[i];
        a.start[i] = (int)total;
        a.scale[i] = scale[i];
        a.flip[i] = flip[i];
        a.img_h[i] = (float)img_h[i];
        a.img_w[i] = (float)img_w[i];
        total += hi[i] - lo[i];
        YMI_CHECK_ARG(total < ((int64_t)1 << 31), "tta_merge: too many anchors");
    }
    if (((uintptr_t)out & 3) != 0) {
        ymi_set_error("tta_merge: out needs 4-byte alignment");
        return YMI_EALIGN;
    }
    if (total == 0) return YMI_OK;
    a.n = n;
    a.rows = (int)rows;
    a.total = (int)total;
    a.out = out;
    hipLaunchKernelGGL(tta_merge_kernel, dim3((unsigned)((total + RS_THREADS - 1) / RS_THREADS), (unsigned)rows, (unsigned)batch), dim3(RS_THREADS), 0,
                       (hipStream_t)stream, a);
    YMI_CHECK_LAUNCH("tta_merge");
    return YMI_OK;
}
