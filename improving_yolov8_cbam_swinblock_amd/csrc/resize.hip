// Image rescaling around the model, one read-once / write-once launch each:
//   scale_image_kernel : F.interpolate(mode="bilinear", align_corners=False) of an NCHW uint8 / float32 batch, with the uint8 -> float / 255
//                        conversion before it, the left-right / up-down flip before that and F.pad(value) to the right and below it
//                        (reference utils/torch_utils.py:475-495 scale_img, models/yolo/detect/train.py:100-114 preprocess_batch, and the
//                        x.flip(3) of nn/tasks.py:392), all in the one pass that writes the float32 NCHW destination
//   tta_merge_kernel   : _descale_pred + _clip_augmented + torch.cat of nn/tasks.py:394-439 on up to three decoded Detect outputs
//   letterbox_kernel   : LetterBox (data/augment.py:1479-1603) + the BGR HWC uint8 -> RGB NCHW float / 255 of engine/predictor.py:144-162 for a
//                        ragged list of images, one launch per 32 images: resize of the byte values, rounding to a grey level, constant border
//   scale_boxes_kernel : scale_boxes + clip_boxes (utils/ops.py:93-127, :335-354) on the (det, count) that ymi_detect_nms leaves
// All only enqueue on the stream they are given (no allocation, no synchronisation): graph-capturable like the rest of the library.
// This file is compiled with -ffp-contract=off (Makefile): the source coordinate (dst + 0.5) * scale - 0.5 must round as a product and a
// difference, as the plain float32 statement of ATen's formula does; contracted into one fma the coordinate - and with it the weight - moves
// by up to half an ulp OF THE COORDINATE (3e-5 at x = 600), which is above the 1e-5 the interpolated pixels are held to.
#include "common.h"

namespace {

constexpr int RS_THREADS = 256;
constexpr int RS_PX = 4;  // consecutive output pixels of a row per lane: one 16-byte store

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

// The image table of one letterbox launch, by value in the kernel arguments (as TtaArgs): no pointer table in device memory.
constexpr int LB_MAX = YMI_LETTERBOX_MAX;
struct LbArgs {
    const uint8_t* src[LB_MAX];
    int h[LB_MAX], w[LB_MAX], hs[LB_MAX], ws[LB_MAX], top[LB_MAX], left[LB_MAX];
    float sy[LB_MAX], sx[LB_MAX];
    float* dst;        // plane 0 of the launch's first image
    int H, W, wgroups; // destination size, ceil(W / 4)
    int rows;          // H * wgroups lanes of work per image
    int pad, bgr, vec_store;
};

// source byte -> destination value: the / 255 of predictor.py:161 (NORM) or the grey level itself
template <bool NORM> __device__ __forceinline__ float of_level(uint32_t u) { return NORM ? unit_of_byte(u) : (float)u; }

// grid (ceil(H * wgroups / RS_THREADS), 1, images): blockIdx.z selects the image, a lane owns RS_PX consecutive pixels of one destination row in
// all three planes (the three channel bytes of a source pixel are adjacent: one lane reads them all) and writes three 16-byte stores.  Inside
// [top, top + hs) x [left, left + ws): the resize of the BYTE VALUES with tap_of and scale_image_kernel's weight expression, rounded to a grey
// level by floorf(v + 0.5f), then converted; hs == h and ws == w: the bytes themselves.  Everywhere else: the pad level, converted the same way.
template <bool NORM> __global__ __launch_bounds__(RS_THREADS) void letterbox_kernel(LbArgs a) {
    const int gid = blockIdx.x * RS_THREADS + threadIdx.x;
    if (gid >= a.rows) return;
    const int k = blockIdx.z;
    const int xg = gid % a.wgroups, y = gid / a.wgroups;
    const int x0 = xg * RS_PX;
    const uint8_t* sp = a.src[k];
    const int h = a.h[k], w = a.w[k], hs = a.hs[k], ws = a.ws[k];
    const int yy = y - a.top[k], xl = x0 - a.left[k];
    const float padv = of_level<NORM>((uint32_t)a.pad);
    float v[3][RS_PX];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int i = 0; i < RS_PX; ++i) v[c][i] = padv;
    if (yy >= 0 && yy < hs && xl + RS_PX > 0 && xl < ws) {
        if (hs == h && ws == w) {
            const uint8_t* r = sp + (int64_t)yy * w * 3;
#pragma unroll
            for (int i = 0; i < RS_PX; ++i) {
                const int xx = xl + i;
                if (xx >= 0 && xx < ws) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) v[c][i] = of_level<NORM>(r[xx * 3 + (a.bgr ? 2 - c : c)]);
                }
            }
        } else {
            const Tap ty = tap_of(yy, a.sy[k], h);
            const uint8_t* r0 = sp + (int64_t)ty.i0 * w * 3;
            const uint8_t* r1 = sp + (int64_t)ty.i1 * w * 3;
#pragma unroll
            for (int i = 0; i < RS_PX; ++i) {
                const int xx = xl + i;
                if (xx >= 0 && xx < ws) {
                    const Tap tx = tap_of(xx, a.sx[k], w);
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        const int cs = a.bgr ? 2 - c : c;
                        const float p00 = (float)r0[tx.i0 * 3 + cs], p01 = (float)r0[tx.i1 * 3 + cs], p10 = (float)r1[tx.i0 * 3 + cs], p11 = (float)r1[tx.i1 * 3 + cs];
                        const float f = ty.l0 * (tx.l0 * p00 + tx.l1 * p01) + ty.l1 * (tx.l0 * p10 + tx.l1 * p11);
                        v[c][i] = of_level<NORM>((uint32_t)floorf(f + 0.5f));
                    }
                }
            }
        }
    }
    float* dp = a.dst + ((int64_t)k * 3 * a.H + y) * a.W + x0;
#pragma unroll
    for (int c = 0; c < 3; ++c, dp += (int64_t)a.H * a.W) {
        if (a.vec_store) {
            const f32x4 o = {v[c][0], v[c][1], v[c][2], v[c][3]};
            *reinterpret_cast<f32x4*>(dp) = o;
        } else {
#pragma unroll
            for (int i = 0; i < RS_PX; ++i)
                if (x0 + i < a.W) dp[i] = v[c][i];
        }
    }
}

struct BoxArgs {
    const float* det;
    const int32_t* count;  // NULL: every row is live
    const float* params;   // [batch][5]: gain, pad_x, pad_y, w0, h0
    float* out;
    int64_t det_ld, out_ld;
    int max_det, cols, padding, xywh;
};

// torch's clamp(lo, hi): min(max(v, lo), hi), a NaN stays a NaN
__device__ __forceinline__ float clamp_to(float v, float hi) {
    v = v < 0.0f ? 0.0f : v;
    return v > hi ? hi : v;
}

// grid (ceil(max_det / RS_THREADS), batch): one row per lane.  boxes[..., i] -= pad; boxes[..., :4] /= gain (IEEE float32 division: what
// `tensor /= python_float` computes - neither a product with the reciprocal nor a double-precision quotient); clip_boxes.
__global__ __launch_bounds__(RS_THREADS) void scale_boxes_kernel(BoxArgs a) {
    const int r = blockIdx.x * RS_THREADS + threadIdx.x, b = blockIdx.y;
    if (r >= a.max_det) return;
    const float* s = a.det + ((int64_t)b * a.max_det + r) * a.det_ld;
    float* d = a.out + ((int64_t)b * a.max_det + r) * a.out_ld;
    if (a.count && r >= a.count[b]) {
        if (d != s)
            for (int c = 0; c < a.cols; ++c) d[c] = 0.0f;
        return;
    }
    const float* p = a.params + (int64_t)b * 5;
    const float gain = p[0], px_ = p[1], py_ = p[2], w0 = p[3], h0 = p[4];
    float x1 = s[0], y1 = s[1], x2 = s[2], y2 = s[3];
    if (a.padding) {
        x1 = x1 - px_;
        y1 = y1 - py_;
        if (!a.xywh) {
            x2 = x2 - px_;
            y2 = y2 - py_;
        }
    }
    x1 = x1 / gain; y1 = y1 / gain; x2 = x2 / gain; y2 = y2 / gain;
    for (int c = 4; c < a.cols; ++c) d[c] = s[c];
    d[0] = clamp_to(x1, w0); d[1] = clamp_to(y1, h0); d[2] = clamp_to(x2, w0); d[3] = clamp_to(y2, h0);
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

extern "C" int ymi_letterbox_batch(const ymi_letterbox_image* images, int64_t n, float* dst, int64_t H, int64_t W, int32_t pad_value, int32_t normalize,
                                   int32_t bgr, void* stream) {
    YMI_CHECK_ARG(images && dst, "letterbox_batch: null pointer");
    YMI_CHECK_ARG(n > 0 && H > 0 && W > 0 && H < (1 << 24) && W < (1 << 24), "letterbox_batch: bad shape");
    YMI_CHECK_ARG(pad_value >= 0 && pad_value <= 255, "letterbox_batch: the pad value is a grey level in [0, 255]");
    if ((uintptr_t)dst & 3) {
        ymi_set_error("letterbox_batch: dst needs 4-byte alignment");
        return YMI_EALIGN;
    }
    const int64_t wgroups = (W + RS_PX - 1) / RS_PX, rows = H * wgroups;
    YMI_CHECK_ARG(rows < ((int64_t)1 << 31), "letterbox_batch: destination too large for one launch");
    for (int64_t i = 0; i < n; ++i) {
        const ymi_letterbox_image& m = images[i];
        YMI_CHECK_ARG(m.src && m.h > 0 && m.w > 0 && m.h < (1 << 24) && m.w < (1 << 24), "letterbox_batch: image %lld: null pointer or bad shape", (long long)i);
        YMI_CHECK_ARG(m.hs > 0 && m.ws > 0 && m.top >= 0 && m.left >= 0 && (int64_t)m.top + m.hs <= H && (int64_t)m.left + m.ws <= W,
                      "letterbox_batch: image %lld: %d x %d at (%d, %d) does not lie within the destination %lld x %lld", (long long)i, m.hs, m.ws, m.top,
                      m.left, (long long)H, (long long)W);
    }
    hipStream_t s = (hipStream_t)stream;
    for (int64_t first = 0; first < n; first += LB_MAX) {
        const int cnt = (int)(n - first < LB_MAX ? n - first : LB_MAX);
        LbArgs a = {};
        for (int i = 0; i < cnt; ++i) {
            const ymi_letterbox_image& m = images[first + i];
            a.src[i] = m.src;
            a.h[i] = m.h; a.w[i] = m.w; a.hs[i] = m.hs; a.ws[i] = m.ws; a.top[i] = m.top; a.left[i] = m.left;
            a.sy[i] = (float)m.h / (float)m.hs;
            a.sx[i] = (float)m.w / (float)m.ws;
        }
        a.dst = dst + first * 3 * H * W;
        a.H = (int)H; a.W = (int)W; a.wgroups = (int)wgroups; a.rows = (int)rows;
        a.pad = pad_value;
        a.bgr = bgr != 0;
        a.vec_store = W % RS_PX == 0 && ((uintptr_t)dst & 15) == 0;
        const dim3 grid((unsigned)((rows + RS_THREADS - 1) / RS_THREADS), 1, (unsigned)cnt);
        if (normalize) hipLaunchKernelGGL(letterbox_kernel<true>, grid, dim3(RS_THREADS), 0, s, a);
        else hipLaunchKernelGGL(letterbox_kernel<false>, grid, dim3(RS_THREADS), 0, s, a);
        YMI_CHECK_LAUNCH("letterbox_batch");
    }
    return YMI_OK;
}

extern "C" int ymi_scale_boxes(const float* det, int64_t det_ld, const int32_t* count, const float* params, int64_t batch, int64_t max_det, int64_t cols,
                               int32_t padding, int32_t xywh, float* out, int64_t out_ld, void* stream) {
    YMI_CHECK_ARG(det && params && out, "scale_boxes: null pointer");
    YMI_CHECK_ARG(batch >= 0 && batch < 65536 && max_det >= 0 && max_det < ((int64_t)1 << 31), "scale_boxes: batch in [0, 65535], rows below 2^31");
    YMI_CHECK_ARG(cols >= 4 && det_ld >= cols && out_ld >= cols, "scale_boxes: rows hold at least 4 columns and a row stride of at least that");
    if (((uintptr_t)det & 3) || ((uintptr_t)out & 3) || ((uintptr_t)params & 3) || ((uintptr_t)count & 3)) {
        ymi_set_error("scale_boxes: pointers need 4-byte alignment");
        return YMI_EALIGN;
    }
    if (batch == 0 || max_det == 0) return YMI_OK;
    BoxArgs a;
    a.det = det; a.count = count; a.params = params; a.out = out;
    a.det_ld = det_ld; a.out_ld = out_ld;
    a.max_det = (int)max_det; a.cols = (int)cols; a.padding = padding != 0; a.xywh = xywh != 0;
    hipLaunchKernelGGL(scale_boxes_kernel, dim3((unsigned)((max_det + RS_THREADS - 1) / RS_THREADS), (unsigned)batch), dim3(RS_THREADS), 0, (hipStream_t)stream, a);
    YMI_CHECK_LAUNCH("scale_boxes");
    return YMI_OK;
}
