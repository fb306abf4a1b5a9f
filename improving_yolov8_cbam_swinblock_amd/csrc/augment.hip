// Training augmentation on the device (reference data/augment.py v8_transforms at perspective = 0), one read of the sources and one write of
// the float32 NCHW batch:
//   augment_kernel       : Mosaic._mosaic4 + RandomPerspective's warpAffine + RandomHSV + RandomFlip + BGR HWC uint8 -> RGB NCHW float / 255.  The
//                          2s x 2s canvas is never built: each bilinear tap resolves by itself to a pixel of one of up to four sources or to
//                          the border level.  One launch per 32 images; the table row of an image is read with uniform (scalar) loads.
//   augment_boxes_kernel : the labels of the batch through the same geometry, box_candidates, flips and normalisation, compacted in order.
// include/ymi.h writes both rules out operation by operation; tests/augment_ref.py restates them.  The random draws and the geometry are
// host Python (data/augment.py, ops/augment.py).  Both only enqueue on the stream they are given.
// The header's rules round every product and sum on its own: the double-precision source coordinate (A[1] * y + A[2]) * 1024 and the float32
// V * (1 - S * f) of the colour round trip move by an ulp when contracted into an fma, and an ulp of the coordinate is a grey level at an edge.
// The image kernel therefore passes every product that feeds a sum through rounded() and does not depend on a compiler flag.  The file is built
// with -ffp-contract=off all the same (Makefile), for the label kernel's float32 steps, which the header also states one operation at a time.
#include <math.h>

#include "common.h"

namespace {

constexpr int AG_THREADS = 256;  // also the length of the division tables: thread t builds entry t
constexpr int AG_PX = 4;         // consecutive output pixels of a row per lane: one 16-byte store per plane

struct AugArgs {
    const ymi_augment_image* table;  // the launch's first row (device)
    float* dst;                      // plane 0 of the launch's first image
    int size, wgroups, rows;         // destination side, ceil(size / 4), size * wgroups lanes of work per image
    int border, bgr, vec_store;
};

// one canvas pixel as b | g << 8 | r << 16: the pixel of the placement that holds (cy, cx), else the border level (header: "resolved by itself").
// The address is chosen first and the three bytes are loaded whatever was found (a tap that no placement holds reads the first source's first
// pixel and drops it), so that the loads of a lane's sixteen taps depend on no branch and are all in flight together.
__device__ __forceinline__ uint32_t canvas_px(const ymi_augment_image& m, int cy, int cx, uint32_t border) {
    const bool inside = (unsigned)cy < (unsigned)m.canvas_h && (unsigned)cx < (unsigned)m.canvas_w;
    typedef const __attribute__((address_space(1))) uint8_t* gbytes_t;  // (sources lie in global memory: global, not flat, loads)
    gbytes_t p = (gbytes_t)m.s[0].src;
    bool found = false;
#pragma unroll
    for (int k = YMI_AUGMENT_MAX_SRC - 1; k >= 0; --k) {  // (descending, so that the first placement that holds the pixel is the one that stays)
        const ymi_augment_source& s = m.s[k];
        const bool hit = inside && k < m.n_src && cx >= s.x1a && cx < s.x2a && cy >= s.y1a && cy < s.y2a;
        gbytes_t q = (gbytes_t)s.src + ((int64_t)(cy - s.y1a + s.y1b) * s.w + (cx - s.x1a + s.x1b)) * 3;
        p = hit ? q : p;
        found = found || hit;
    }
    const uint32_t v = (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16;
    return found ? v : border;
}

// A product that is about to be added to: passed through an empty asm, it is a value the optimiser cannot look behind, so it is rounded on its
// own and never becomes half of an fma - whatever -ffp-contract the file is built with (the header states every rule one rounded operation at a time).
__device__ __forceinline__ double rounded(double x) {
    asm volatile("" : "+v"(x));
    return x;
}
__device__ __forceinline__ float rounded(float x) {
    asm volatile("" : "+v"(x));
    return x;
}

__device__ __forceinline__ int level_of(float t) {  // rn(t * 255) clamped to a grey level
    const int v = __float2int_rn(t * 255.0f);
    return v < 0 ? 0 : v > 255 ? 255 : v;
}

// header step 3: BGR -> HSV in integers, the three tables, HSV -> BGR in float32
__device__ __forceinline__ uint32_t hsv_round_trip(uint32_t bgr, const int* sdiv, const int* hdiv, const uint8_t* lut) {
    const int b = bgr & 255, g = (bgr >> 8) & 255, r = (bgr >> 16) & 255;
    const int v = max(b, max(g, r)), d = v - min(b, min(g, r));
    const int s = (d * sdiv[v] + (1 << 11)) >> 12;
    int h = v == r ? g - b : v == g ? b - r + 2 * d : r - g + 4 * d;
    h = (h * hdiv[d] + (1 << 11)) >> 12;
    h += h < 0 ? 180 : 0;
    const int h2 = lut[h], s2 = lut[256 + s], v2 = lut[512 + v];
    const float V = (float)v2 * (1.0f / 255.0f);
    float tb = V, tg = V, tr = V;
    if (s2 != 0) {
        const float S = (float)s2 * (1.0f / 255.0f);
        float H = rounded((float)h2 * (6.0f / 180.0f));
        int k = (int)floorf(H);
        H = H - (float)k;
        if ((unsigned)k >= 6u) {  // (a hue table entry of 180 or more: not RandomHSV's)
            k = 0;
            H = 0.0f;
        }
        const float t0 = V, t1 = V * (1.0f - S), t2 = V * (1.0f - rounded(S * H)), t3 = V * (1.0f - rounded(S * (1.0f - H)));
        switch (k) {
            case 0: tb = t1; tg = t3; tr = t0; break;
            case 1: tb = t1; tg = t0; tr = t2; break;
            case 2: tb = t3; tg = t0; tr = t1; break;
            case 3: tb = t0; tg = t2; tr = t1; break;
            case 4: tb = t0; tg = t1; tr = t3; break;
            default: tb = t2; tg = t1; tr = t0; break;
        }
    }
    return (uint32_t)level_of(tb) | (uint32_t)level_of(tg) << 8 | (uint32_t)level_of(tr) << 16;
}

// grid (ceil(size * wgroups / AG_THREADS), 1, images): blockIdx.z selects the table row, a lane owns AG_PX consecutive pixels of one destination
// row in all three planes and writes three 16-byte stores.  With a colour stage the workgroup first builds the two division tables and copies
// the image's three 256-byte tables into LDS: every pixel indexes them by value.
template <bool NORM> __global__ __launch_bounds__(AG_THREADS) void augment_kernel(AugArgs a) {
    __shared__ int sdiv[256], hdiv[256];
    __shared__ uint8_t lut[768];
    const ymi_augment_image& m = a.table[blockIdx.z];
    const bool hsv = m.lut != nullptr;
    if (hsv) {
        const int t = threadIdx.x;
        sdiv[t] = t ? __double2int_rn((double)(255 << 12) / (double)t) : 0;
        hdiv[t] = t ? __double2int_rn((double)(180 << 12) / (6.0 * (double)t)) : 0;
#pragma unroll
        for (int i = 0; i < 3; ++i) lut[i * 256 + t] = m.lut[i * 256 + t];
        __syncthreads();
    }
    const int gid = blockIdx.x * AG_THREADS + threadIdx.x;
    if (gid >= a.rows) return;
    const int xg = gid % a.wgroups, y = gid / a.wgroups;
    const int x0 = xg * AG_PX;
    const uint32_t border = (uint32_t)a.border * 0x010101u;
    const int yw = m.flip_ud ? a.size - 1 - y : y;
    const double yd = (double)yw;
    const int bx = __double2int_rn((rounded(m.A[1] * yd) + m.A[2]) * 1024.0), by = __double2int_rn((rounded(m.A[4] * yd) + m.A[5]) * 1024.0);
    float v[3][AG_PX];
#pragma unroll
    for (int i = 0; i < AG_PX; ++i) {
        const int x = x0 + i;
        const int xw = m.flip_lr ? a.size - 1 - x : x;  // (x >= size in the row tail: computed like any pixel - every tap is bounds-checked - and not stored)
        const double xd = (double)xw;
        const int X = (__double2int_rn(m.A[0] * xd * 1024.0) + bx + 16) >> 5, Y = (__double2int_rn(m.A[3] * xd * 1024.0) + by + 16) >> 5;
        const int sx = X >> 5, fx = X & 31, sy = Y >> 5, fy = Y & 31;
        const uint32_t p00 = canvas_px(m, sy, sx, border), p01 = canvas_px(m, sy, sx + 1, border);
        const uint32_t p10 = canvas_px(m, sy + 1, sx, border), p11 = canvas_px(m, sy + 1, sx + 1, border);
        const int w00 = (32 - fx) * (32 - fy), w01 = fx * (32 - fy), w10 = (32 - fx) * fy, w11 = fx * fy;
        uint32_t px = 0;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int sh = 8 * c;
            const int lv = (w00 * (int)((p00 >> sh) & 255) + w01 * (int)((p01 >> sh) & 255) + w10 * (int)((p10 >> sh) & 255) +
                            w11 * (int)((p11 >> sh) & 255) + 512) >> 10;
            px |= (uint32_t)lv << sh;
        }
        if (hsv) px = hsv_round_trip(px, sdiv, hdiv, lut);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const uint32_t lv = (px >> (8 * (a.bgr ? 2 - c : c))) & 255;
            v[c][i] = NORM ? unit_of_byte(lv) : (float)lv;
        }
    }
    float* dp = a.dst + ((int64_t)blockIdx.z * 3 * a.size + y) * a.size + x0;
#pragma unroll
    for (int c = 0; c < 3; ++c, dp += (int64_t)a.size * a.size) {
        if (a.vec_store) {
            const f32x4 o = {v[c][0], v[c][1], v[c][2], v[c][3]};
            *reinterpret_cast<f32x4*>(dp) = o;
        } else {
#pragma unroll
            for (int i = 0; i < AG_PX; ++i)
                if (x0 + i < a.size) dp[i] = v[c][i];
        }
    }
}

constexpr int AB_THREADS = 1024;
struct BoxRowArgs {
    const float* rows;
    const ymi_augment_label_image* images;
    int n, batch;
    float area_thr;
    float* batch_idx;
    float* cls;
    float* bboxes;
    int32_t* keep;
    int32_t* count;
    int32_t* total;
};

__device__ __forceinline__ float clip_to(float v, float hi) {  // numpy's clip(0, hi)
    v = v < 0.0f ? 0.0f : v;
    return v > hi ? hi : v;
}

// header steps 1-7 of one row -> kept?, (b, cls, normalised xywh) in o[6]
__device__ __forceinline__ bool augment_row(const BoxRowArgs& a, int i, float (&o)[6]) {
    const float* r = a.rows + (int64_t)i * 7;
    const float fb = r[0], fk = r[1];
    if (!(fb >= 0.0f && fb < (float)a.batch && fk >= 0.0f && fk < (float)YMI_AUGMENT_MAX_SRC)) return false;
    const int b = (int)fb, k = (int)fk;
    const ymi_augment_label_image& m = a.images[b];
    if (i < m.row_start || i >= m.row_end) return false;
    const float hw = r[5] / 2.0f, hh = r[6] / 2.0f;
    float x1 = r[3] - hw, y1 = r[4] - hh, x2 = r[3] + hw, y2 = r[4] + hh;
    x1 = x1 * m.src_w[k] * m.ratio_w[k] + m.padw[k];
    y1 = y1 * m.src_h[k] * m.ratio_h[k] + m.padh[k];
    x2 = x2 * m.src_w[k] * m.ratio_w[k] + m.padw[k];
    y2 = y2 * m.src_h[k] * m.ratio_h[k] + m.padh[k];
    if (m.canvas > 0.0f) {
        x1 = clip_to(x1, m.canvas); y1 = clip_to(y1, m.canvas); x2 = clip_to(x2, m.canvas); y2 = clip_to(y2, m.canvas);
        if (!((x2 - x1) * (y2 - y1) > 0.0f)) return false;
    }
    const float xs[4] = {x1, x2, x1, x2}, ys[4] = {y1, y2, y2, y1};
    float nx1 = 0, ny1 = 0, nx2 = 0, ny2 = 0;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const float X = m.M[0] * xs[c] + m.M[1] * ys[c] + m.M[2], Y = m.M[3] * xs[c] + m.M[4] * ys[c] + m.M[5];
        nx1 = c ? fminf(nx1, X) : X; nx2 = c ? fmaxf(nx2, X) : X;
        ny1 = c ? fminf(ny1, Y) : Y; ny2 = c ? fmaxf(ny2, Y) : Y;
    }
    nx1 = clip_to(nx1, m.size_w); nx2 = clip_to(nx2, m.size_w); ny1 = clip_to(ny1, m.size_h); ny2 = clip_to(ny2, m.size_h);
    const float eps = 1e-16f;
    const float w1 = x2 * m.scale - x1 * m.scale, h1 = y2 * m.scale - y1 * m.scale;
    const float w2 = nx2 - nx1, h2 = ny2 - ny1;
    const float ar = fmaxf(w2 / (h2 + eps), h2 / (w2 + eps));
    if (!(w2 > 2.0f && h2 > 2.0f && w2 * h2 / (w1 * h1 + eps) > a.area_thr && ar < 100.0f)) return false;
    float cx = (nx1 + nx2) / 2.0f, cy = (ny1 + ny2) / 2.0f;
    if (m.flip_ud) cy = m.size_h - cy;
    if (m.flip_lr) cx = m.size_w - cx;
    o[0] = (float)b; o[1] = r[2];
    o[2] = cx / m.size_w; o[3] = cy / m.size_h; o[4] = w2 / m.size_w; o[5] = h2 / m.size_h;
    return true;
}

// ONE workgroup walks the rows in chunks of AB_THREADS: a ballot gives a kept row its place within its wave, the waves' totals its place within
// the chunk, a running base its place in the output - the rows' own order, whatever the timing.  Then a lane per image sums its rows' flags.
__global__ __launch_bounds__(AB_THREADS) void augment_boxes_kernel(BoxRowArgs a) {
    __shared__ int wave_total[AB_THREADS / YMI_WAVE];
    __shared__ int base;
    const int tid = threadIdx.x, lane = tid & (YMI_WAVE - 1), wave = tid / YMI_WAVE;
    if (tid == 0) base = 0;
    __syncthreads();
    for (int start = 0; start < a.n; start += AB_THREADS) {
        const int i = start + tid;
        float o[6];
        const bool kept = i < a.n && augment_row(a, i, o);
        const unsigned long long ballot = __ballot(kept);
        if (lane == 0) wave_total[wave] = __popcll(ballot);
        __syncthreads();
        int pos = base + __popcll(ballot & ((1ull << lane) - 1ull)), chunk = 0;
        for (int w = 0; w < AB_THREADS / YMI_WAVE; ++w) {
            pos += w < wave ? wave_total[w] : 0;
            chunk += wave_total[w];
        }
        if (i < a.n) a.keep[i] = kept;
        if (kept) {
            a.batch_idx[pos] = o[0];
            a.cls[pos] = o[1];
#pragma unroll
            for (int c = 0; c < 4; ++c) a.bboxes[(int64_t)pos * 4 + c] = o[2 + c];
        }
        __syncthreads();  // everyone has read base and the totals
        if (tid == 0) base += chunk;
        __syncthreads();
    }
    for (int b = tid; b < a.batch; b += AB_THREADS) {  // (keep[] is this workgroup's own: visible after the barrier)
        const ymi_augment_label_image& m = a.images[b];
        int c = 0;
        for (int i = max(m.row_start, 0); i < min(m.row_end, a.n); ++i) c += a.keep[i];
        a.count[b] = c;
    }
    if (tid == 0) *a.total = base;
}

}  // namespace

extern "C" int ymi_augment_batch(const ymi_augment_image* table, const ymi_augment_image* table_d, int64_t n, float* dst, int64_t size, int32_t border,
                                 int32_t normalize, int32_t bgr, void* stream) {
    YMI_CHECK_ARG(table && table_d && dst, "augment_batch: null pointer");
    YMI_CHECK_ARG(n > 0 && size > 0 && size < (1 << 15), "augment_batch: bad shape (the side stays below 32768)");
    YMI_CHECK_ARG(border >= 0 && border <= 255, "augment_batch: the border value is a grey level in [0, 255]");
    if (((uintptr_t)dst & 3) || ((uintptr_t)table_d & 7)) {
        ymi_set_error("augment_batch: dst needs 4-byte, the device table 8-byte alignment");
        return YMI_EALIGN;
    }
    for (int64_t i = 0; i < n; ++i) {
        const ymi_augment_image& m = table[i];
        YMI_CHECK_ARG(m.n_src >= 1 && m.n_src <= YMI_AUGMENT_MAX_SRC && m.canvas_h > 0 && m.canvas_w > 0 && m.canvas_h < (1 << 24) && m.canvas_w < (1 << 24),
                      "augment_batch: image %lld: 1 to %d sources on a canvas with sides in [1, 2^24)", (long long)i, YMI_AUGMENT_MAX_SRC);
        for (int k = 0; k < m.n_src; ++k) {
            const ymi_augment_source& s = m.s[k];
            YMI_CHECK_ARG(s.src && s.h > 0 && s.w > 0 && s.h < (1 << 24) && s.w < (1 << 24), "augment_batch: image %lld source %d: null pointer or bad shape",
                          (long long)i, k);
            if (s.x2a <= s.x1a || s.y2a <= s.y1a) continue;  // an empty placement shows nothing
            YMI_CHECK_ARG(s.x1a >= 0 && s.y1a >= 0 && s.x2a <= m.canvas_w && s.y2a <= m.canvas_h && s.x1b >= 0 && s.y1b >= 0 &&
                              (int64_t)s.x1b + (s.x2a - s.x1a) <= s.w && (int64_t)s.y1b + (s.y2a - s.y1a) <= s.h,
                          "augment_batch: image %lld source %d: the placement leaves the canvas or the %d x %d source", (long long)i, k, s.h, s.w);
        }
        const double far = (double)(size - 1);
        bool ok = true;
        for (int r = 0; r < 2; ++r)  // |coordinate * 1024| stays below 2^30: the two rounded terms and their sum are ints
            ok = ok && fabs(m.A[3 * r]) * far < (double)(1 << 19) && fabs(m.A[3 * r + 1]) * far + fabs(m.A[3 * r + 2]) < (double)(1 << 19);
        YMI_CHECK_ARG(ok, "augment_batch: image %lld: the inverse matrix is not finite or maps a pixel beyond 2^19", (long long)i);  // (a NaN fails every <)
    }
    const int64_t wgroups = (size + AG_PX - 1) / AG_PX, rows = size * wgroups;
    hipStream_t s = (hipStream_t)stream;
    for (int64_t first = 0; first < n; first += YMI_AUGMENT_MAX) {
        const int cnt = (int)(n - first < YMI_AUGMENT_MAX ? n - first : YMI_AUGMENT_MAX);
        AugArgs a;
        a.table = table_d + first;
        a.dst = dst + first * 3 * size * size;
        a.size = (int)size; a.wgroups = (int)wgroups; a.rows = (int)rows;
        a.border = border;
        a.bgr = bgr != 0;
        a.vec_store = size % AG_PX == 0 && ((uintptr_t)dst & 15) == 0;
        const dim3 grid((unsigned)((rows + AG_THREADS - 1) / AG_THREADS), 1, (unsigned)cnt);
        if (normalize) hipLaunchKernelGGL(augment_kernel<true>, grid, dim3(AG_THREADS), 0, s, a);
        else hipLaunchKernelGGL(augment_kernel<false>, grid, dim3(AG_THREADS), 0, s, a);
        YMI_CHECK_LAUNCH("augment_batch");
    }
    return YMI_OK;
}

extern "C" int ymi_augment_boxes(const float* rows, int64_t n, const ymi_augment_label_image* images, int64_t batch, float area_thr, float* batch_idx,
                                 float* cls, float* bboxes, int32_t* keep, int32_t* count, int32_t* total, void* stream) {
    YMI_CHECK_ARG(images && count && total && batch > 0 && batch < (1 << 24), "augment_boxes: null pointer or batch outside [1, 2^24)");
    YMI_CHECK_ARG(n >= 0 && n < (1 << 24) && (n == 0 || (rows && batch_idx && cls && bboxes && keep)), "augment_boxes: null pointer or rows outside [0, 2^24)");
    if (((uintptr_t)rows & 3) || ((uintptr_t)images & 3) || ((uintptr_t)batch_idx & 3) || ((uintptr_t)cls & 3) || ((uintptr_t)bboxes & 3) ||
        ((uintptr_t)keep & 3) || ((uintptr_t)count & 3) || ((uintptr_t)total & 3)) {
        ymi_set_error("augment_boxes: pointers need 4-byte alignment");
        return YMI_EALIGN;
    }
    BoxRowArgs a;
    a.rows = rows; a.images = images; a.n = (int)n; a.batch = (int)batch; a.area_thr = area_thr;
    a.batch_idx = batch_idx; a.cls = cls; a.bboxes = bboxes; a.keep = keep; a.count = count; a.total = total;
    hipLaunchKernelGGL(augment_boxes_kernel, dim3(1), dim3(AB_THREADS), 0, (hipStream_t)stream, a);
    YMI_CHECK_LAUNCH("augment_boxes");
    return YMI_OK;
}
