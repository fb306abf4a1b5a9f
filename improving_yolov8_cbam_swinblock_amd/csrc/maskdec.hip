// Mask decode on the device: process_mask / crop_mask of the reference (utils/ops.py:661-710) and the counts that mask_iou (utils/metrics.py:137)
// needs, on the prototype map as Proto's eval output leaves it (NHWC memory, bfloat16 or float32) and the rows ymi_detect_nms_seg keeps:
//   mask_lowres_kernel   : process_mask(upsample=False): per pixel of the prototype grid the crop test, the 32-term dot, `> 0`
//   mask_upsample_kernel : process_mask(upsample=True): a workgroup takes one row and one UP_TH x UP_TW tile of the output; it forms the cropped
//                          logits of the tile's footprint on the prototype grid (one-pixel halo included) in LDS, then every thread resamples
//                          16 consecutive output pixels from LDS (tap_of: ATen's bilinear rule, align_corners = false), thresholds them and
//                          stores 16 bytes.  Footprint pixels outside the box cost a comparison; a tile whose footprint misses the box stores
//                          zeros without touching proto or LDS.
//   mask_overlap_kernel  : one workgroup per (image, detection) walks the detection's crop on the prototype grid and counts, in ONE LDS
//                          histogram, the pixels with logit > 0 by the value the overlap encoding has there; the workgroup behind an image's
//                          last detection counts the encoding's own values (area_gt).  No mask is ever stored.
// One statement of the crop (crop_of / inside) and of the logit (logit_at) serves all three.  Grids depend on shapes only; the only atomics are
// integer adds (LDS histogram bins, the area of a row), so every result is a function of the input alone, bit for bit.  Indices read from memory
// (img, count, the encoding's values) are range-checked and skipped.
// This file is compiled with -ffp-contract=off (Makefile): the crop edges x1 * float32(mw / iw) and the resampling coordinate must round one
// operation at a time, as the reference's torch statements do.  The dot's terms are explicit fused multiply-adds (one rounding per term).
#include "common.h"

namespace {

constexpr int NM = YMI_MASK_NM;
constexpr int MD_THREADS = 256;
constexpr int LOW_PX = 4;                       // consecutive pixels of the flattened grid per thread: one 4-byte store
constexpr int UP_TH = 16, UP_TW = 256;          // output tile of the upsample form: MD_THREADS threads x 16 bytes
constexpr int UP_FH = UP_TH + 2, UP_FW = UP_TW + 2;  // its footprint on the prototype grid at scales <= 1, halo included
static_assert(UP_TH * UP_TW == MD_THREADS * 16, "every thread of the upsample form stores 16 bytes");
constexpr int MAX_BINS = YMI_MASK_MAX_BINS;

struct ProtoMap {
    const void* data;
    int B, mh, mw;
    int64_t ld;  // elements between pixels (NHWC)
};

// the box scaled to the prototype grid, as process_mask's downsampled_bboxes
struct Crop {
    float x1, y1, x2, y2;
};
__device__ __forceinline__ Crop crop_of(const float* box, float rw, float rh) { return Crop{box[0] * rw, box[1] * rh, box[2] * rw, box[3] * rh}; }
// crop_mask's (r >= x1) * (r < x2) * (c >= y1) * (c < y2)
__device__ __forceinline__ bool inside(const Crop& k, int r, int c) {
    const float fc = (float)c, fr = (float)r;
    return fc >= k.x1 && fc < k.x2 && fr >= k.y1 && fr < k.y2;
}
// integer bounds [lo, hi) that contain every v in [0, n) with v >= a && v < b (NaN edges: empty or everything; `inside` still decides)
__device__ __forceinline__ void span_of(float a, float b, int n, int& lo, int& hi) {
    lo = (int)fminf(fmaxf(ceilf(a), 0.0f), (float)n);
    hi = (int)fminf(fmaxf(ceilf(b), 0.0f), (float)n);
}

struct Coef {
    float v[NM];
};
__device__ __forceinline__ Coef coef_of(const float* row) {
    Coef c;
#pragma unroll
    for (int k = 0; k < NM; ++k) c.v[k] = row[k];
    return c;
}
// masks_in @ protos at pixel (r, c) of image b: the float32 sum of the 32 products in channel order
template <typename T> __device__ __forceinline__ float logit_at(const ProtoMap& p, int b, int r, int c, const Coef& cf) {
    const T* px = static_cast<const T*>(p.data) + (((int64_t)b * p.mh + r) * p.mw + c) * p.ld;
    float acc = 0.0f;
#pragma unroll
    for (int k0 = 0; k0 < NM; k0 += ElemTraits<T>::CH) {
        float v[ElemTraits<T>::CH];
        Pack<T, ElemTraits<T>::CH>::load(px + k0, v);
#pragma unroll
        for (int k = 0; k < ElemTraits<T>::CH; ++k) acc = __builtin_fmaf(cf.v[k0 + k], v[k], acc);
    }
    return acc;
}

// sum of v over the workgroup's lanes added to *dst with one integer atomic per wave
__device__ __forceinline__ void add_count(int* dst, int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, YMI_WAVE);
    if ((threadIdx.x & (YMI_WAVE - 1)) == 0 && v) atomicAdd(dst, v);
}

struct DecodeArgs {
    ProtoMap p;
    const float* box;   // [N][4]
    const float* coef;  // [N][NM]
    const int* img;     // [N]
    uint8_t* mask;      // [N][oh][ow]
    int* area;          // [N], zero before the launch
    int oh, ow;
    int tiles, tiles_x;  // workgroups per row; upsample form: of them per tile row
    float rw, rh;        // float32(mw / iw), float32(mh / ih)
    float sx, sy;        // upsample form: ATen's scales mw / ow, mh / oh
    int vec;             // every store of the form's width is aligned
};

template <typename T> __global__ __launch_bounds__(MD_THREADS) void mask_lowres_kernel(DecodeArgs a) {
    const int row = blockIdx.x / a.tiles, tile = blockIdx.x - row * a.tiles;
    const int b = a.img[row];
    const bool live = b >= 0 && b < a.p.B;
    const Crop k = crop_of(a.box + (size_t)row * 4, a.rw, a.rh);
    const Coef cf = coef_of(a.coef + (size_t)row * NM);
    const int total = a.oh * a.ow;
    const int p0 = (tile * MD_THREADS + (int)threadIdx.x) * LOW_PX;
    uint8_t* out = a.mask + (size_t)row * total;
    uint32_t word = 0;
    int on = 0;
#pragma unroll
    for (int i = 0; i < LOW_PX; ++i) {
        const int p = p0 + i;
        if (p < total && live) {
            const int r = p / a.ow, c = p - r * a.ow;
            if (inside(k, r, c) && logit_at<T>(a.p, b, r, c, cf) > 0.0f) {
                word |= 1u << (8 * i);
                ++on;
            }
        }
    }
    if (a.vec) {
        if (p0 < total) *reinterpret_cast<uint32_t*>(out + p0) = word;
    } else {
#pragma unroll
        for (int i = 0; i < LOW_PX; ++i)
            if (p0 + i < total) out[p0 + i] = (uint8_t)((word >> (8 * i)) & 1u);
    }
    add_count(a.area + row, on);
}

template <typename T> __global__ __launch_bounds__(MD_THREADS) void mask_upsample_kernel(DecodeArgs a) {
    __shared__ float foot[UP_FH][UP_FW + 1];
    const int row = blockIdx.x / a.tiles, tile = blockIdx.x - row * a.tiles;
    const int ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;
    const int y0 = ty * UP_TH, x0 = tx * UP_TW;
    const int y_last = min(y0 + UP_TH, a.oh) - 1, x_last = min(x0 + UP_TW, a.ow) - 1;
    const int b = a.img[row];
    const bool live = b >= 0 && b < a.p.B;
    const Crop k = crop_of(a.box + (size_t)row * 4, a.rw, a.rh);
    // the footprint: first source row / column of the tile's first pixel to the second one of its last (tap_of is monotonic in dst)
    const int r_lo = tap_of(y0, a.sy, a.p.mh).i0, c_lo = tap_of(x0, a.sx, a.p.mw).i0;
    const int fh = min(tap_of(y_last, a.sy, a.p.mh).i1 - r_lo + 1, UP_FH), fw = min(tap_of(x_last, a.sx, a.p.mw).i1 - c_lo + 1, UP_FW);
    // a tile whose footprint holds no pixel of the crop resamples zeros: it stores them without touching proto or LDS (workgroup-uniform)
    int kc0, kc1, kr0, kr1;
    span_of(k.x1, k.x2, a.p.mw, kc0, kc1);
    span_of(k.y1, k.y2, a.p.mh, kr0, kr1);
    const bool hit = live && max(kc0, c_lo) < min(kc1, c_lo + fw) && max(kr0, r_lo) < min(kr1, r_lo + fh);
    if (hit) {
        const Coef cf = coef_of(a.coef + (size_t)row * NM);
        for (int e = threadIdx.x; e < fh * fw; e += MD_THREADS) {
            const int fr = e / fw, fc = e - fr * fw;
            const int r = r_lo + fr, c = c_lo + fc;
            foot[fr][fc] = inside(k, r, c) ? logit_at<T>(a.p, b, r, c, cf) : 0.0f;
        }
    }
    __syncthreads();
    const int y = y0 + (int)threadIdx.x / (UP_TW / 16), xs = x0 + ((int)threadIdx.x % (UP_TW / 16)) * 16;
    int on = 0;
    if (y < a.oh && xs < a.ow && !hit) {
        uint8_t* out = a.mask + ((size_t)row * a.oh + y) * a.ow + xs;
        if (a.vec) {
            const u32x4 o = {0u, 0u, 0u, 0u};
            *reinterpret_cast<u32x4*>(out) = o;
        } else {
#pragma unroll
            for (int i = 0; i < 16; ++i)
                if (xs + i < a.ow) out[i] = 0;
        }
    } else if (y < a.oh && xs < a.ow) {
        const Tap t = tap_of(y, a.sy, a.p.mh);
        const int f0 = min(t.i0 - r_lo, fh - 1), f1 = min(t.i1 - r_lo, fh - 1);
        uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int x = xs + i;
            if (x < a.ow) {
                const Tap u = tap_of(x, a.sx, a.p.mw);
                const int g0 = min(u.i0 - c_lo, fw - 1), g1 = min(u.i1 - c_lo, fw - 1);
                const float v = t.l0 * (u.l0 * foot[f0][g0] + u.l1 * foot[f0][g1]) + t.l1 * (u.l0 * foot[f1][g0] + u.l1 * foot[f1][g1]);
                if (v > 0.0f) {
                    w[i >> 2] |= 1u << (8 * (i & 3));
                    ++on;
                }
            }
        }
        uint8_t* out = a.mask + ((size_t)row * a.oh + y) * a.ow + xs;
        if (a.vec) {  // (ow % 16 == 0: a group lies wholly inside the row)
            const u32x4 o = {w[0], w[1], w[2], w[3]};
            *reinterpret_cast<u32x4*>(out) = o;
        } else {
#pragma unroll
            for (int i = 0; i < 16; ++i)
                if (xs + i < a.ow) out[i] = (uint8_t)((w[i >> 2] >> (8 * (i & 3))) & 1u);
        }
    }
    add_count(a.area + row, on);
}

// the value of the overlap encoding at element i as a bin, or -1 when it names none (float encodings: only whole numbers name a bin, as the
// reference's `gt_masks == index` finds them)
__device__ __forceinline__ int bin_of(const uint8_t* m, size_t i, int n_bins) {
    const int v = m[i];
    return v < n_bins ? v : -1;
}
__device__ __forceinline__ int bin_of(const float* m, size_t i, int n_bins) {
    const float f = m[i];
    if (!(f >= 0.0f && f < (float)n_bins)) return -1;
    const int v = (int)f;
    return (float)v == f ? v : -1;
}

struct OverlapArgs {
    ProtoMap p;
    const float* det;   // [B][max_det][6]
    const float* coef;  // [B][max_det][NM]
    const int* count;   // [B]
    const void* enc;    // [B][mh][mw]
    int max_det, n_bins;
    float rw, rh;
    int* inter;      // [B][max_det][n_bins]
    int* area_pred;  // [B][max_det]
    int* area_gt;    // [B][n_bins]
};

template <typename T, typename M> __global__ __launch_bounds__(MD_THREADS) void mask_overlap_kernel(OverlapArgs a) {
    __shared__ int hist[MAX_BINS + 1];  // the last word: the predicted area
    const int b = blockIdx.x / (a.max_det + 1), d = blockIdx.x - b * (a.max_det + 1);
    const int tid = threadIdx.x;
    const M* enc = static_cast<const M*>(a.enc) + (size_t)b * a.p.mh * a.p.mw;
    for (int i = tid; i <= MAX_BINS; i += MD_THREADS) hist[i] = 0;
    __syncthreads();
    if (d == a.max_det) {  // (workgroup-uniform) the encoding's own counts
        const int total = a.p.mh * a.p.mw;
        for (int i = tid; i < total; i += MD_THREADS) {
            const int v = bin_of(enc, i, a.n_bins);
            if (v >= 0) atomicAdd(&hist[v], 1);
        }
        __syncthreads();
        for (int i = tid; i < a.n_bins; i += MD_THREADS) a.area_gt[(size_t)b * a.n_bins + i] = hist[i];
        return;
    }
    int n = a.count[b];
    n = n < 0 ? 0 : n > a.max_det ? a.max_det : n;
    const size_t slot = (size_t)b * a.max_det + d;
    if (d < n) {  // (workgroup-uniform)
        const Crop k = crop_of(a.det + slot * 6, a.rw, a.rh);
        const Coef cf = coef_of(a.coef + slot * NM);
        int c0, c1, r0, r1;
        span_of(k.x1, k.x2, a.p.mw, c0, c1);
        span_of(k.y1, k.y2, a.p.mh, r0, r1);
        const int w = c1 - c0, cells = w > 0 && r1 > r0 ? w * (r1 - r0) : 0;
        int on = 0;
        for (int e = tid; e < cells; e += MD_THREADS) {
            const int r = r0 + e / w, c = c0 + e % w;
            if (inside(k, r, c) && logit_at<T>(a.p, b, r, c, cf) > 0.0f) {
                ++on;
                const int v = bin_of(enc, (size_t)r * a.p.mw + c, a.n_bins);
                if (v >= 0) atomicAdd(&hist[v], 1);
            }
        }
        add_count(&hist[MAX_BINS], on);
        __syncthreads();
    }
    for (int i = tid; i < a.n_bins; i += MD_THREADS) a.inter[slot * a.n_bins + i] = hist[i];
    if (tid == 0) a.area_pred[slot] = hist[MAX_BINS];
}

// the checks both entry points make of the prototype map
int proto_map_of(const char* who, const ymi_tensor* proto, int64_t ih, int64_t iw, ProtoMap* out) {
    YMI_CHECK_ARG(ymi_tensor_ok(proto), "%s: bad prototype map", who);
    YMI_CHECK_ARG(proto->c == NM, "%s: the mask kernels are built for nm = %d prototypes, got %lld", who, NM, (long long)proto->c);
    YMI_CHECK_ARG(ih > 0 && iw > 0 && ih < (1 << 15) && iw < (1 << 15) && proto->h < (1 << 15) && proto->w < (1 << 15) && proto->n < (1 << 20),
                  "%s: image and prototype sizes below 32768, batch below 2^20", who);
    if (((uintptr_t)proto->data & 15) || ((size_t)proto->ld * ymi_esize(proto->dtype)) % 16) {
        ymi_set_error("%s: the prototype map's pixels need 16-byte alignment", who);
        return YMI_EALIGN;
    }
    *out = ProtoMap{proto->data, (int)proto->n, (int)proto->h, (int)proto->w, proto->ld};
    return YMI_OK;
}

}  // namespace

extern "C" int ymi_process_mask(const ymi_tensor* proto, const float* box, const float* coef, const int32_t* img, int64_t n, int64_t ih, int64_t iw,
                                int32_t upsample, uint8_t* mask, int32_t* area, void* stream) {
    DecodeArgs a = {};
    const int rc = proto_map_of("process_mask", proto, ih, iw, &a.p);
    if (rc != YMI_OK) return rc;
    YMI_CHECK_ARG(n >= 0 && n < (1 << 20), "process_mask: fewer than 2^20 rows");
    if (n == 0) return YMI_OK;
    YMI_CHECK_ARG(box && coef && img && mask && area, "process_mask: null pointer");
    YMI_CHECK_ARG(!upsample || (ih >= proto->h && iw >= proto->w), "process_mask: upsample takes an image at least as large as the prototype map");
    if (((uintptr_t)box & 3) || ((uintptr_t)coef & 3) || ((uintptr_t)img & 3) || ((uintptr_t)area & 3)) {
        ymi_set_error("process_mask: box / coef / img / area need 4-byte alignment");
        return YMI_EALIGN;
    }
    a.box = box, a.coef = coef, a.img = img, a.mask = mask, a.area = area;
    a.rw = (float)((double)proto->w / (double)iw);
    a.rh = (float)((double)proto->h / (double)ih);
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(area, 0, (size_t)n * sizeof(int32_t), s) != hipSuccess) {
        ymi_set_error("process_mask: clearing the areas failed");
        return YMI_ELAUNCH;
    }
    if (upsample) {
        a.oh = (int)ih, a.ow = (int)iw;
        a.sy = (float)proto->h / (float)ih;  // ATen area_pixel_compute_scale with a size (no scale_factor) given
        a.sx = (float)proto->w / (float)iw;
        a.tiles_x = (a.ow + UP_TW - 1) / UP_TW;
        a.tiles = a.tiles_x * ((a.oh + UP_TH - 1) / UP_TH);
        a.vec = a.ow % 16 == 0 && ((uintptr_t)mask & 15) == 0;
    } else {
        a.oh = (int)proto->h, a.ow = (int)proto->w;
        a.tiles = (a.oh * a.ow + MD_THREADS * LOW_PX - 1) / (MD_THREADS * LOW_PX);
        a.vec = (a.oh * a.ow) % LOW_PX == 0 && ((uintptr_t)mask & 3) == 0;
    }
    YMI_CHECK_ARG(n * a.tiles < ((int64_t)1 << 31), "process_mask: %lld rows of %d tiles exceed the grid", (long long)n, a.tiles);
    const dim3 grid((unsigned)(n * a.tiles));
    dispatch_dtype(proto->dtype, [&](auto t) {
        typedef typename decltype(t)::type T;
        if (upsample) hipLaunchKernelGGL(mask_upsample_kernel<T>, grid, dim3(MD_THREADS), 0, s, a);
        else hipLaunchKernelGGL(mask_lowres_kernel<T>, grid, dim3(MD_THREADS), 0, s, a);
    });
    YMI_CHECK_LAUNCH("process_mask");
    return YMI_OK;
}

extern "C" int ymi_mask_overlap(const float* det, const float* coef, const int32_t* count, int64_t batch, int64_t max_det, const ymi_tensor* proto,
                                int64_t ih, int64_t iw, const void* masks, int32_t masks_f32, int64_t masks_h, int64_t masks_w, int64_t n_bins,
                                int32_t* inter, int32_t* area_pred, int32_t* area_gt, void* stream) {
    OverlapArgs a = {};
    const int rc = proto_map_of("mask_overlap", proto, ih, iw, &a.p);
    if (rc != YMI_OK) return rc;
    YMI_CHECK_ARG(det && coef && count && masks && inter && area_pred && area_gt, "mask_overlap: null pointer");
    YMI_CHECK_ARG(batch == proto->n, "mask_overlap: %lld images, %lld prototype maps", (long long)batch, (long long)proto->n);
    YMI_CHECK_ARG(max_det > 0 && max_det <= 2048, "mask_overlap: max_det in [1, 2048]");
    YMI_CHECK_ARG(batch * (max_det + 1) < ((int64_t)1 << 31), "mask_overlap: batch * (max_det + 1) exceeds the grid");
    YMI_CHECK_ARG(n_bins >= 1 && n_bins <= MAX_BINS, "mask_overlap: n_bins in [1, %d]", MAX_BINS);
    YMI_CHECK_ARG(masks_h == proto->h && masks_w == proto->w,
                  "mask_overlap: the overlap encoding is %lld x %lld, the prototype map %lld x %lld (the reference would resample it: not built)",
                  (long long)masks_h, (long long)masks_w, (long long)proto->h, (long long)proto->w);
    if (((uintptr_t)det & 3) || ((uintptr_t)coef & 3) || ((uintptr_t)count & 3) || ((uintptr_t)inter & 3) || ((uintptr_t)area_pred & 3) ||
        ((uintptr_t)area_gt & 3) || (masks_f32 && ((uintptr_t)masks & 3))) {
        ymi_set_error("mask_overlap: det / coef / count / the outputs (and a float32 encoding) need 4-byte alignment");
        return YMI_EALIGN;
    }
    a.det = det, a.coef = coef, a.count = count, a.enc = masks, a.max_det = (int)max_det, a.n_bins = (int)n_bins;
    a.rw = (float)((double)proto->w / (double)iw);
    a.rh = (float)((double)proto->h / (double)ih);
    a.inter = inter, a.area_pred = area_pred, a.area_gt = area_gt;
    const dim3 grid((unsigned)(batch * (max_det + 1)));
    hipStream_t s = (hipStream_t)stream;
    dispatch_dtype(proto->dtype, [&](auto t) {
        typedef typename decltype(t)::type T;
        if (masks_f32) hipLaunchKernelGGL((mask_overlap_kernel<T, float>), grid, dim3(MD_THREADS), 0, s, a);
        else hipLaunchKernelGGL((mask_overlap_kernel<T, uint8_t>), grid, dim3(MD_THREADS), 0, s, a);
    });
    YMI_CHECK_LAUNCH("mask_overlap");
    return YMI_OK;
}
