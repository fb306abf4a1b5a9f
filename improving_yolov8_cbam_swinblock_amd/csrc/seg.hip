// Instance segmentation: the depth-to-space pair of Proto's transposed convolution and the mask term of v8SegmentationLoss.
//
// Depth to space.  nn.ConvTranspose2d(c, c, 2, 2, 0) has no overlapping taps: it is four 1x1 GEMMs, one per output sub-pixel (the MFMA 1x1 path
// with the weight viewed as [4c, c]), whose [N, H, W, 4c] result this file's copy kernel scatters to [N, 2H, 2W, c]; the inverse gathers the
// output gradient back for the data- and weight-gradient GEMMs.  Both move 16-byte chunks and know no dtype.
//
// Mask loss (reference ultralytics/utils/loss.py:349-438, crop_mask utils/ops.py:661-677).  For every foreground anchor a of image b with gt
// index k and target box t (pixels):  logit[p] = sum_c coef[a][c] * proto[b][c][p],  term_a = mean over ALL mask pixels of
// BCE(logit[p], masks[b][p] == k + 1) restricted to the pixels inside t scaled to mask pixels, divided by t's normalised area;
// loss = sum_a term_a / (number of foreground anchors of the batch).
//
// Work decomposition ("Mask loss"): the crop makes the product sparse - an anchor touches only the pixels of its box - so the
// kernels are vector-ALU loops over crops, not a dense [anchors x pixels x 32] MFMA GEMM whose epilogue would pay exp + log on every pixel:
//   compact  one wave per image: foreground anchors in ascending anchor order -> records (box in mask pixels, area, gt id, anchor)
//   forward  one workgroup per record slot: BCE sum over the crop, fixed-order workgroup sum -> one partial per slot
//   final    one workgroup: partials in slot order (double-precision tree), / foreground count, the criterion's [4] + [4] results
//   d coef   one workgroup per record slot: 32 sums over the crop, fixed-order workgroup sums -> the anchor's row of its level's map
//   d proto  one thread per pixel: the image's records in slot order, 64 at a time through LDS -> the pixel's 32 channels
// No atomics: every sum has one owner and a fixed order, so results are bit-identical from run to run.  Every grid is sized by the static
// bound cap = min(A, topk * max_boxes) on the foreground anchors of an image; the counts stay on the device.
#include "common.h"

namespace {
constexpr int SEG_MAXL = 4;
constexpr int NM = 32;        // mask coefficients per anchor = prototype channels
constexpr int REC_TILE = 64;  // records staged in LDS at a time by the prototype-gradient kernel

struct FgRec {
    float x1, y1, x2, y2;  // target box in mask pixels
    float area;            // its normalised area (width * height of the box / image)
    int gt1;               // gt index + 1: the value the overlap-encoded mask holds on this object
    int anchor;
    int pad_;
};

struct SegGeom {
    const void* mc[SEG_MAXL];
    void* dmc[SEG_MAXL];
    int64_t ldm[SEG_MAXL], lddm[SEG_MAXL];
    int H[SEG_MAXL], W[SEG_MAXL], off[SEG_MAXL + 1];
    const void* proto;
    void* dproto;
    int64_t ldp, lddp;
    const void* masks;  // [B, Hm, Wm] uint8 or float32
    int masks_f32, Hm, Wm;
    int nl, B, A, G, cap, mh, mw;
    float img_w, img_h;
};

// the anchor's pixel row in its level's coefficient map (select chains: a dynamically indexed kernel-argument array goes to scratch)
template <typename T, typename V>
__device__ __forceinline__ T* mc_row(const SegGeom& g, V* const (&maps)[SEG_MAXL], const int64_t (&lds)[SEG_MAXL], int b, int a) {
    V* base = maps[0];
    int64_t ld = lds[0];
    int off = 0, hw = g.H[0] * g.W[0];
#pragma unroll
    for (int i = 1; i < SEG_MAXL; ++i)
        if (i < g.nl && a >= g.off[i]) {
            base = maps[i];
            ld = lds[i];
            off = g.off[i];
            hw = g.H[i] * g.W[i];
        }
    return reinterpret_cast<T*>(base) + ((int64_t)b * hw + (a - off)) * ld;
}

// the overlap-encoded gt mask at prototype pixel (y, x): F.interpolate(mode="nearest")'s source index when the sizes differ
__device__ __forceinline__ float mask_at(const SegGeom& g, int b, int y, int x) {
    int sy = y, sx = x;
    if (g.Hm != g.mh || g.Wm != g.mw) {
        sy = min((int)floorf((float)y * ((float)g.Hm / (float)g.mh)), g.Hm - 1);
        sx = min((int)floorf((float)x * ((float)g.Wm / (float)g.mw)), g.Wm - 1);
    }
    const int64_t i = ((int64_t)b * g.Hm + sy) * g.Wm + sx;
    return g.masks_f32 ? reinterpret_cast<const float*>(g.masks)[i] : (float)reinterpret_cast<const uint8_t*>(g.masks)[i];
}

// crop_mask's rule on integer pixel indices: x >= x1 && x < x2  <=>  ceil(x1) <= x < ceil(x2); clamped to the map
struct Crop {
    int xs, ys, cw, n;  // first column / row, width, pixel count (0: empty)
};
__device__ __forceinline__ int clamp_ceil(float v, int hi) { return (int)fminf(fmaxf(ceilf(v), 0.f), (float)hi); }
__device__ __forceinline__ Crop crop_of(const FgRec& r, int mh, int mw) {
    Crop c;
    c.xs = clamp_ceil(r.x1, mw);
    c.ys = clamp_ceil(r.y1, mh);
    const int xe = clamp_ceil(r.x2, mw), ye = clamp_ceil(r.y2, mh);
    c.cw = xe - c.xs;
    c.n = (c.cw > 0 && ye > c.ys) ? c.cw * (ye - c.ys) : 0;
    return c;
}
__device__ __forceinline__ bool inside(const float (&box)[4], int y, int x) {
    return (float)x >= box[0] && (float)x < box[2] && (float)y >= box[1] && (float)y < box[3];
}

template <typename T> __device__ __forceinline__ void load_nm(const T* p, float (&v)[NM]) {
    constexpr int CH = ElemTraits<T>::CH;
#pragma unroll
    for (int i = 0; i < NM; i += CH) {
        float t[CH];
        Pack<T, CH>::load(p + i, t);
#pragma unroll
        for (int j = 0; j < CH; ++j) v[i + j] = t[j];
    }
}
template <typename T> __device__ __forceinline__ void store_nm(T* p, const float (&v)[NM]) {
    constexpr int CH = ElemTraits<T>::CH;
#pragma unroll
    for (int i = 0; i < NM; i += CH) {
        float t[CH];
#pragma unroll
        for (int j = 0; j < CH; ++j) t[j] = v[i + j];
        Pack<T, CH>::store(p + i, t);
    }
}
__device__ __forceinline__ float dot_nm(const float (&a)[NM], const float* b) {
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < NM; ++k) s = fmaf(a[k], b[k], s);
    return s;
}
__device__ __forceinline__ float sigmoid_exact(float x) { return 1.0f / (1.0f + expf(-x)); }

// workgroup sum of 256 threads in a fixed association: the wave's butterfly, then (w0 + w1) + (w2 + w3)
__device__ __forceinline__ float block_sum(float v, float (&sh)[4]) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

// ---- depth to space / space to depth -------------------------------------------------------------------------------------------------
// deep [N, H, W, 4C], channel (2a + b) * C + c  <->  wide [N, 2H, 2W, C] at (2y + a, 2x + b, c); one thread per 16-byte chunk of `deep`
template <bool TO_SPACE>
__global__ __launch_bounds__(256) void d2s_kernel(const char* __restrict__ src, char* __restrict__ dst, int64_t ld_deep, int64_t ld_wide, int W,
                                                  int chunks_c, int64_t total) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const int j = (int)(t % (4 * chunks_c));
    const int64_t pix = t / (4 * chunks_c);  // (n * H + y) * W + x
    const int x = (int)(pix % W);
    const int64_t ny = pix / W;
    const int q = j / chunks_c, cc = j - q * chunks_c;
    const int64_t deep_off = pix * ld_deep + (int64_t)j * 16;
    const int64_t wide_off = ((ny * 2 + (q >> 1)) * (2 * (int64_t)W) + 2 * x + (q & 1)) * ld_wide + (int64_t)cc * 16;
    if (TO_SPACE) *reinterpret_cast<u32x4*>(dst + wide_off) = *reinterpret_cast<const u32x4*>(src + deep_off);
    else *reinterpret_cast<u32x4*>(dst + deep_off) = *reinterpret_cast<const u32x4*>(src + wide_off);
}

int launch_d2s(const ymi_tensor* deep, const ymi_tensor* wide, bool to_space, const char* what, void* stream) {
    YMI_CHECK_ARG(ymi_tensor_ok(deep) && ymi_tensor_ok(wide) && deep->dtype == wide->dtype, "%s: tensors", what);
    YMI_CHECK_ARG(deep->c == 4 * wide->c && wide->n == deep->n && wide->h == 2 * deep->h && wide->w == 2 * deep->w, "%s: [N,H,W,4C] against [N,2H,2W,C]", what);
    const int64_t es = (int64_t)ymi_esize(deep->dtype);
    YMI_CHECK_ARG((wide->c * es) % 16 == 0 && (deep->ld * es) % 16 == 0 && (wide->ld * es) % 16 == 0 && ((uintptr_t)deep->data % 16) == 0 &&
                      ((uintptr_t)wide->data % 16) == 0,
                  "%s: channels and pixel strides in whole 16-byte chunks", what);
    const int chunks_c = (int)(wide->c * es / 16);
    const int64_t total = ymi_pixels(deep) * 4 * chunks_c;
    YMI_CHECK_ARG(deep->w < (1ll << 30) && total < (1ll << 40), "%s: tensor too large", what);
    const dim3 grid((unsigned)((total + 255) / 256));
    if (to_space)
        hipLaunchKernelGGL(d2s_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, (const char*)deep->data, (char*)wide->data, deep->ld * es,
                           wide->ld * es, (int)deep->w, chunks_c, total);
    else
        hipLaunchKernelGGL(d2s_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, (const char*)wide->data, (char*)deep->data, deep->ld * es,
                           wide->ld * es, (int)deep->w, chunks_c, total);
    YMI_CHECK_LAUNCH(what);
    return YMI_OK;
}

// ---- compact: the image's foreground anchors, ascending, as records ----------------------------------------------------------------------
__global__ __launch_bounds__(64) void seg_compact_kernel(SegGeom g, const int* __restrict__ gidx, const float* __restrict__ targets,
                                                         FgRec* __restrict__ recs, int* __restrict__ count) {
    const int b = blockIdx.x, lane = threadIdx.x;
    int base = 0;
    for (int a0 = 0; a0 < g.A; a0 += 64) {
        const int a = a0 + lane;
        int k = a < g.A ? gidx[(int64_t)b * g.A + a] : -1;
        if (k >= g.G) k = -1;
        const bool fg = k >= 0;
        const unsigned long long m = __ballot(fg);
        const int pos = base + __popcll(m & ((1ull << lane) - 1ull));
        if (fg && pos < g.cap) {
            const float* tg = targets + ((int64_t)b * g.G + k) * 5;
            // reference loss.py:412-418: normalise by the image size, area from the normalised box, then scale to mask pixels
            const float nx1 = tg[1] / g.img_w, ny1 = tg[2] / g.img_h, nx2 = tg[3] / g.img_w, ny2 = tg[4] / g.img_h;
            FgRec r;
            r.x1 = nx1 * (float)g.mw;
            r.y1 = ny1 * (float)g.mh;
            r.x2 = nx2 * (float)g.mw;
            r.y2 = ny2 * (float)g.mh;
            r.area = (nx2 - nx1) * (ny2 - ny1);
            r.gt1 = k + 1;
            r.anchor = a;
            r.pad_ = 0;
            recs[(int64_t)b * g.cap + pos] = r;
        }
        base += __popcll(m);
    }
    if (lane == 0) count[b] = min(base, g.cap);
}

// ---- forward: one workgroup per record slot ------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void seg_fwd_kernel(SegGeom g, const FgRec* __restrict__ recs, const int* __restrict__ count,
                                                      float* __restrict__ part) {
    __shared__ float sh[4];
    const int slot = blockIdx.x, b = blockIdx.y;
    const int64_t ir = (int64_t)b * g.cap + slot;
    if (slot >= count[b]) {  // (uniform across the workgroup)
        if (threadIdx.x == 0) part[ir] = 0.f;
        return;
    }
    const FgRec r = recs[ir];
    const Crop c = crop_of(r, g.mh, g.mw);
    float coef[NM];
    const T* cp = mc_row<const T>(g, g.mc, g.ldm, b, r.anchor);
#pragma unroll
    for (int k = 0; k < NM; ++k) coef[k] = to_f32(cp[k]);
    const T* pp = reinterpret_cast<const T*>(g.proto) + (int64_t)b * g.mh * g.mw * g.ldp;
    float sum = 0.f;
    for (int i = threadIdx.x; i < c.n; i += 256) {
        const int dy = i / c.cw;
        const int y = c.ys + dy, x = c.xs + (i - dy * c.cw);
        float pv[NM];
        load_nm<T>(pp + ((int64_t)y * g.mw + x) * g.ldp, pv);
        const float l = dot_nm(pv, coef);
        const float t = mask_at(g, b, y, x) == (float)r.gt1 ? 1.f : 0.f;
        sum += fmaxf(l, 0.f) - l * t + log1pf(expf(-fabsf(l)));
    }
    sum = block_sum(sum, sh);
    if (threadIdx.x == 0) part[ir] = (sum / (float)(g.mh * g.mw)) / r.area;
}

// ---- final: partials in slot order, the foreground count, and the criterion's two results ------------------------------------------------------
// out8[0..3] = (box, seg, cls, dfl) * gain * batch (differentiable result), out8[4..7] = the same * gain (reference loss.py:342-347); box, cls and
// dfl are copied from the detection loss's six results, seg takes the box gain (scale6[0], scale6[3])
__global__ __launch_bounds__(256) void seg_final_kernel(const float* __restrict__ part, int n_part, const int* __restrict__ count, int B,
                                                        const float* __restrict__ det6, const float* __restrict__ scale6, float* __restrict__ out8,
                                                        float* __restrict__ nfg_out) {
    __shared__ double sh[256];
    double acc = 0.0;
    for (int i = threadIdx.x; i < n_part; i += 256) acc += (double)part[i];
    sh[threadIdx.x] = acc;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        int nfg = 0;
        for (int b = 0; b < B; ++b) nfg += count[b];
        const float seg = nfg > 0 ? (float)(sh[0] / (double)nfg) : 0.f;
        nfg_out[0] = (float)nfg;
        out8[0] = det6[0];
        out8[1] = seg * scale6[0];
        out8[2] = det6[1];
        out8[3] = det6[2];
        out8[4] = det6[3];
        out8[5] = seg * scale6[3];
        out8[6] = det6[4];
        out8[7] = det6[5];
    }
}

// d loss / d logit of one pixel of one anchor is (sigmoid(l) - t) * gs / area, with gs = grad * gain * batch / (nfg * pixels)
__device__ __forceinline__ float grad_scale(const SegGeom& g, const float* gout8, const float* scale6, const float* nfg) {
    const float n = nfg[0];
    return n > 0.f ? gout8[1] * scale6[0] / (n * (float)(g.mh * g.mw)) : 0.f;
}

// ---- backward, coefficients: one workgroup per record slot -> the anchor's row (background rows are zeroed by the caller's fill) ---------------
template <typename T>
__global__ __launch_bounds__(256) void seg_bwd_coef_kernel(SegGeom g, const FgRec* __restrict__ recs, const int* __restrict__ count,
                                                           const float* __restrict__ gout8, const float* __restrict__ scale6,
                                                           const float* __restrict__ nfg) {
    __shared__ float sh[NM][4];
    const int slot = blockIdx.x, b = blockIdx.y;
    if (slot >= count[b]) return;  // (uniform)
    const FgRec r = recs[(int64_t)b * g.cap + slot];
    const Crop c = crop_of(r, g.mh, g.mw);
    const float gs = grad_scale(g, gout8, scale6, nfg) / r.area;
    float coef[NM], acc[NM];
    const T* cp = mc_row<const T>(g, g.mc, g.ldm, b, r.anchor);
#pragma unroll
    for (int k = 0; k < NM; ++k) {
        coef[k] = to_f32(cp[k]);
        acc[k] = 0.f;
    }
    const T* pp = reinterpret_cast<const T*>(g.proto) + (int64_t)b * g.mh * g.mw * g.ldp;
    for (int i = threadIdx.x; i < c.n; i += 256) {
        const int dy = i / c.cw;
        const int y = c.ys + dy, x = c.xs + (i - dy * c.cw);
        float pv[NM];
        load_nm<T>(pp + ((int64_t)y * g.mw + x) * g.ldp, pv);
        const float l = dot_nm(pv, coef);
        const float t = mask_at(g, b, y, x) == (float)r.gt1 ? 1.f : 0.f;
        const float d = (sigmoid_exact(l) - t) * gs;
#pragma unroll
        for (int k = 0; k < NM; ++k) acc[k] = fmaf(d, pv[k], acc[k]);
    }
#pragma unroll
    for (int k = 0; k < NM; ++k) {
        const float v = wave_sum(acc[k]);
        if ((threadIdx.x & 63) == 0) sh[k][threadIdx.x >> 6] = v;
    }
    __syncthreads();
    if (threadIdx.x < NM) {
        const int k = threadIdx.x;
        mc_row<T>(g, g.dmc, g.lddm, b, r.anchor)[k] = from_f32<T>((sh[k][0] + sh[k][1]) + (sh[k][2] + sh[k][3]));
    }
}

// ---- backward, prototypes: one thread per pixel, the image's records in slot order ---------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void seg_bwd_proto_kernel(SegGeom g, const FgRec* __restrict__ recs, const int* __restrict__ count,
                                                            const float* __restrict__ gout8, const float* __restrict__ scale6,
                                                            const float* __restrict__ nfg) {
    __shared__ float s_coef[REC_TILE][NM];
    __shared__ float s_box[REC_TILE][4];
    __shared__ float s_gs[REC_TILE];
    __shared__ float s_gt[REC_TILE];
    const int b = blockIdx.y;
    const int p = blockIdx.x * 256 + threadIdx.x;
    const bool live = p < g.mh * g.mw;
    const int y = live ? p / g.mw : 0, x = live ? p - (p / g.mw) * g.mw : 0;
    const int n = count[b];
    const float gs = grad_scale(g, gout8, scale6, nfg);
    float pv[NM], acc[NM];
    const T* pp = reinterpret_cast<const T*>(g.proto) + ((int64_t)b * g.mh * g.mw + (live ? p : 0)) * g.ldp;
    load_nm<T>(pp, pv);
#pragma unroll
    for (int k = 0; k < NM; ++k) acc[k] = 0.f;
    const float mval = mask_at(g, b, y, x);
    for (int t0 = 0; t0 < n; t0 += REC_TILE) {
        const int m = min(REC_TILE, n - t0);
        __syncthreads();  // (the previous tile's readers)
        for (int i = threadIdx.x; i < m * NM; i += 256) {
            const int rr = i / NM, k = i - rr * NM;
            const FgRec& r = recs[(int64_t)b * g.cap + t0 + rr];
            s_coef[rr][k] = to_f32(mc_row<const T>(g, g.mc, g.ldm, b, r.anchor)[k]);
        }
        if ((int)threadIdx.x < m) {
            const FgRec r = recs[(int64_t)b * g.cap + t0 + threadIdx.x];
            s_box[threadIdx.x][0] = r.x1;
            s_box[threadIdx.x][1] = r.y1;
            s_box[threadIdx.x][2] = r.x2;
            s_box[threadIdx.x][3] = r.y2;
            s_gs[threadIdx.x] = gs / r.area;
            s_gt[threadIdx.x] = (float)r.gt1;
        }
        __syncthreads();
        if (live) {
            for (int rr = 0; rr < m; ++rr) {
                const float box[4] = {s_box[rr][0], s_box[rr][1], s_box[rr][2], s_box[rr][3]};
                if (!inside(box, y, x)) continue;
                const float l = dot_nm(pv, s_coef[rr]);
                const float d = (sigmoid_exact(l) - (mval == s_gt[rr] ? 1.f : 0.f)) * s_gs[rr];
#pragma unroll
                for (int k = 0; k < NM; ++k) acc[k] = fmaf(d, s_coef[rr][k], acc[k]);
            }
        }
    }
    if (live) store_nm<T>(reinterpret_cast<T*>(g.dproto) + ((int64_t)b * g.mh * g.mw + p) * g.lddp, acc);
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------------
struct SegState {
    FgRec* recs;  // [B, cap]
    int* count;   // [B]
    float* part;  // [B, cap]
    float* nfg;   // [1] (+ padding)
    size_t bytes;
};
SegState carve_seg(void* state, int64_t B, int64_t cap) {
    char* p = reinterpret_cast<char*>(state);
    size_t used = 0;
    auto take = [&](size_t n) {
        char* r = p + used;
        used += (n + 255) / 256 * 256;
        return r;
    };
    SegState v;
    v.recs = reinterpret_cast<FgRec*>(take((size_t)(B * cap) * sizeof(FgRec)));
    v.count = reinterpret_cast<int*>(take((size_t)B * sizeof(int)));
    v.part = reinterpret_cast<float*>(take((size_t)(B * cap) * sizeof(float)));
    v.nfg = reinterpret_cast<float*>(take(4 * sizeof(float)));
    v.bytes = used;
    return v;
}
int64_t seg_cap(int64_t anchors, int64_t max_boxes, int64_t topk) { return topk * max_boxes < anchors ? topk * max_boxes : anchors; }

int fill_seg(SegGeom& g, int32_t nl, const ymi_tensor* mc, const ymi_tensor* proto, const void* masks, int32_t masks_f32, int64_t Hm, int64_t Wm,
             int64_t max_boxes, int32_t topk, float img_w, float img_h, const char* what) {
    YMI_CHECK_ARG(nl >= 1 && nl <= SEG_MAXL && mc && ymi_tensor_ok(proto) && masks, "%s: 1..%d levels, a prototype map and masks", what, SEG_MAXL);
    YMI_CHECK_ARG(proto->c == NM, "%s: built for %d prototypes (nm)", what, NM);
    YMI_CHECK_ARG(Hm > 0 && Wm > 0 && max_boxes >= 1 && topk >= 1 && img_w > 0.f && img_h > 0.f, "%s: sizes", what);
    g = SegGeom{};
    g.nl = nl;
    const int64_t es = (int64_t)ymi_esize(proto->dtype);
    YMI_CHECK_ARG(((uintptr_t)proto->data % 16) == 0 && (proto->ld * es) % 16 == 0, "%s: prototype map alignment", what);
    int off = 0;
    for (int l = 0; l < nl; ++l) {
        YMI_CHECK_ARG(ymi_tensor_ok(&mc[l]) && mc[l].c == NM && mc[l].n == proto->n && mc[l].dtype == proto->dtype, "%s: coefficient map %d", what, l);
        g.mc[l] = mc[l].data;
        g.ldm[l] = mc[l].ld;
        g.H[l] = (int)mc[l].h;
        g.W[l] = (int)mc[l].w;
        g.off[l] = off;
        off += (int)(mc[l].h * mc[l].w);
    }
    for (int l = nl; l <= SEG_MAXL; ++l) g.off[l] = off;
    g.proto = proto->data;
    g.ldp = proto->ld;
    g.masks = masks;
    g.masks_f32 = masks_f32 ? 1 : 0;
    g.Hm = (int)Hm;
    g.Wm = (int)Wm;
    g.B = (int)proto->n;
    g.A = off;
    g.G = (int)max_boxes;
    g.cap = (int)seg_cap(off, max_boxes, topk);
    g.mh = (int)proto->h;
    g.mw = (int)proto->w;
    g.img_w = img_w;
    g.img_h = img_h;
    YMI_CHECK_ARG((int64_t)g.B * g.A < (1ll << 31) && (int64_t)g.mh * g.mw < (1ll << 30) && (int64_t)g.B * g.cap < (1ll << 31) && g.B <= 65535,
                  "%s: B*A < 2^31, mask pixels < 2^30, B <= 65535", what);
    return YMI_OK;
}
}  // namespace

extern "C" int ymi_depth_to_space2(const ymi_tensor* src, const ymi_tensor* dst, void* stream) {
    return launch_d2s(src, dst, true, "depth_to_space2", stream);
}
extern "C" int ymi_space_to_depth2(const ymi_tensor* src, const ymi_tensor* dst, void* stream) {
    return launch_d2s(dst, src, false, "space_to_depth2", stream);
}

extern "C" int ymi_mask_loss_sizes(int64_t batch, int64_t anchors, int64_t max_boxes, int32_t topk, size_t* state_bytes) {
    YMI_CHECK_ARG(batch > 0 && anchors > 0 && max_boxes > 0 && topk > 0 && state_bytes, "mask_loss_sizes: args");
    *state_bytes = carve_seg(nullptr, batch, seg_cap(anchors, max_boxes, topk)).bytes;
    return YMI_OK;
}

extern "C" int ymi_mask_loss_fwd(int32_t nl, const ymi_tensor* mc_maps, const ymi_tensor* proto, const void* masks, int32_t masks_f32, int64_t masks_h,
                                 int64_t masks_w, const int32_t* gidx, const float* targets, int64_t max_boxes, int32_t topk, float img_w, float img_h,
                                 const float* det_out6, const float* scale6, float* out8, void* state, size_t state_bytes, void* stream) {
    SegGeom g;
    int rc = fill_seg(g, nl, mc_maps, proto, masks, masks_f32, masks_h, masks_w, max_boxes, topk, img_w, img_h, "mask_loss_fwd");
    if (rc) return rc;
    YMI_CHECK_ARG(gidx && targets && det_out6 && scale6 && out8 && state, "mask_loss_fwd: null argument");
    const SegState st = carve_seg(state, g.B, g.cap);
    if (state_bytes < st.bytes) {
        ymi_set_error("mask_loss_fwd: state %zu < %zu bytes", state_bytes, st.bytes);
        return YMI_EWORKSPACE;
    }
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(seg_compact_kernel, dim3(g.B), dim3(64), 0, s, g, (const int*)gidx, targets, st.recs, st.count);
    dispatch_dtype(proto->dtype, [&](auto t) {
        hipLaunchKernelGGL(seg_fwd_kernel<typename decltype(t)::type>, dim3(g.cap, g.B), dim3(256), 0, s, g, (const FgRec*)st.recs, (const int*)st.count,
                           st.part);
    });
    hipLaunchKernelGGL(seg_final_kernel, dim3(1), dim3(256), 0, s, (const float*)st.part, g.B * g.cap, (const int*)st.count, g.B, det_out6, scale6, out8,
                       st.nfg);
    YMI_CHECK_LAUNCH("mask_loss_fwd");
    return YMI_OK;
}

extern "C" int ymi_mask_loss_bwd(int32_t nl, const ymi_tensor* mc_maps, const ymi_tensor* proto, const void* masks, int32_t masks_f32, int64_t masks_h,
                                 int64_t masks_w, int64_t max_boxes, int32_t topk, const void* state, size_t state_bytes, const float* grad_out8,
                                 const float* scale6, const ymi_tensor* dmc_maps, const ymi_tensor* dproto, void* stream) {
    SegGeom g;
    int rc = fill_seg(g, nl, mc_maps, proto, masks, masks_f32, masks_h, masks_w, max_boxes, topk, 1.f, 1.f, "mask_loss_bwd");
    if (rc) return rc;
    YMI_CHECK_ARG(state && grad_out8 && scale6 && dmc_maps && ymi_tensor_ok(dproto) && ymi_same_shape(dproto, proto) && dproto->dtype == proto->dtype,
                  "mask_loss_bwd: arguments");
    const int64_t es = (int64_t)ymi_esize(proto->dtype);
    YMI_CHECK_ARG(((uintptr_t)dproto->data % 16) == 0 && (dproto->ld * es) % 16 == 0, "mask_loss_bwd: prototype gradient alignment");
    for (int l = 0; l < nl; ++l) {
        YMI_CHECK_ARG(ymi_tensor_ok(&dmc_maps[l]) && ymi_same_shape(&dmc_maps[l], &mc_maps[l]) && dmc_maps[l].dtype == proto->dtype,
                      "mask_loss_bwd: coefficient gradient map %d", l);
        g.dmc[l] = dmc_maps[l].data;
        g.lddm[l] = dmc_maps[l].ld;
    }
    g.dproto = dproto->data;
    g.lddp = dproto->ld;
    const SegState st = carve_seg(const_cast<void*>(state), g.B, g.cap);
    YMI_CHECK_ARG(state_bytes >= st.bytes, "mask_loss_bwd: state too small");
    hipStream_t s = (hipStream_t)stream;
    dispatch_dtype(proto->dtype, [&](auto t) {
        typedef typename decltype(t)::type T;
        hipLaunchKernelGGL(seg_bwd_coef_kernel<T>, dim3(g.cap, g.B), dim3(256), 0, s, g, (const FgRec*)st.recs, (const int*)st.count, grad_out8, scale6,
                           (const float*)st.nfg);
        hipLaunchKernelGGL(seg_bwd_proto_kernel<T>, dim3((unsigned)((g.mh * g.mw + 255) / 256), g.B), dim3(256), 0, s, g, (const FgRec*)st.recs,
                           (const int*)st.count, grad_out8, scale6, (const float*)st.nfg);
    });
    YMI_CHECK_LAUNCH("mask_loss_bwd");
    return YMI_OK;
}
