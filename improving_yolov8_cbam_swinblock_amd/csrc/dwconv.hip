// Depthwise convolution (groups == cin == cout), NHWC, k in {3, 5}, stride in {1, 2}, pad k/2: forward (eval epilogue or raw output +
// BatchNorm statistics rows), data gradient, weight gradient.  Reference: the grouped F.conv2d behind DWConv / GhostConv.cv2
// (nn/modules/conv.py:79,91 with g = c1 = c2, conv.py:194-209, :329-371) and its autograd.
//
// A depthwise convolution has no reduction over channels: k*k multiply-adds per output element against one element stored and (with reuse
// through the caches) about one read - a streaming kernel on the vector ALUs, nothing for the matrix pipe.
//
// Work split (all kernels): a workgroup of 256 threads owns a tile of up to DW_CT channels (blockIdx.y) and a share of the pixels
// (blockIdx.x).  Inside, a thread keeps ONE 16-byte channel chunk g for all its pixels and threads are numbered chunk-fastest, so a wave
// covers `chunks` consecutive 16-byte pieces of a pixel and then the next pixel run: with C = 8 in bfloat16 (one chunk a pixel) the 64
// lanes lie on 64 pixel runs, never on channels that do not exist.  The taps of the tile sit in LDS as float32 [tap][channel]
// (25 taps x 8 channels a lane do not fit beside the accumulators); a lane reads its chunk's taps as ds_read_b128, lanes of equal chunk
// broadcast.  Forward / stride-1 data gradient: a thread computes DW_TW consecutive outputs of one row, loading every input chunk of the
// (DW_TW - 1) * stride + k wide span once per tap row.  Every tap is tested against the IMAGE (rows, columns), never against a tile.
//
// Statistics rows: sum and sum of squares of the ROUNDED outputs per thread, combined over the workgroup's pixel rows in LDS in row order
// and stored as row blockIdx.x of [blocks][2][C] - the rows ymi_bn_finalize reads (same contract as ymi_conv2d_fwd).  No atomics.
// Weight gradient: a thread owns (chunk, tap row) and k x chunk accumulators over runs of DW_TW outputs; the workgroup combines its pixel rows
// in LDS in row order, stores one slab row [tap][C], and a second launch adds the rows - eight interleaved chains per element, combined in
// chain order - into dw [C][1][k][k].  Grids depend on the shape only: bit-identical from run to run.
// Taps outside the image read the library's zero page through a select of the ADDRESS: no branch separates the loads of a run.
#include "common.h"

namespace {

constexpr int DW_CT = 256;    // channels per workgroup tile (forward, data gradient): 25 taps x 256 x 4 B = 25.6 kB of LDS
constexpr int DW_CTW = 128;   // ... of the weight gradient: threads are (pixel row, tap row, chunk), k * chunks <= 256
constexpr int DW_TW = 4;      // outputs of one row a thread computes side by side
constexpr int DW_MAX_BLOCKS = 768;   // pixel-axis workgroups: three per CU, one resident round (<= 16 * 64: ymi_bn_finalize sums the rows without a staging pass)
constexpr int DW_WG_BLOCKS = 768;    // ... of the weight gradient (slab rows)

template <typename T> struct Chunk;
template <> struct Chunk<float> { typedef f32x4 type; };
template <> struct Chunk<bf16_t> { typedef bf16x8 type; };

struct DwTensor {
    const void* p;
    int64_t ld;
    int n, h, w;
};
static DwTensor dwt(const ymi_tensor* t) { return DwTensor{t->data, t->ld, (int)t->n, (int)t->h, (int)t->w}; }

struct DwFwdArgs {
    DwTensor x, y;     // input and output (data gradient: dy and dx)
    const void* res;   // optional addend of y's shape (residual / data-gradient addend; may be y itself), row stride res_ld
    int64_t res_ld;
    const float* w;    // [C][1][k][k] float32
    const float* scale;
    const float* bias;
    float* part;       // statistics rows [gridDim.x][2][C], or nullptr
    int C, act;
    int runs_per_row;  // ceil(y.w / TW)
    int64_t runs;      // y.n * y.h * runs_per_row
    const void* zero;  // 16 zero bytes (ymi_zero_page): what a tap outside the image reads
};

// taps of channels [c0, c0 + ct) -> sm[tap][DW_CT] (FLIP: rotated by 180 degrees, the data gradient's order)
template <int KK, bool FLIP> __device__ __forceinline__ void stage_taps(const float* __restrict__ w, int c0, int ct, float* sm) {
    for (int i = threadIdx.x; i < ct * KK; i += blockDim.x) {
        const int cl = i / KK, tap = i - cl * KK;
        sm[(FLIP ? KK - 1 - tap : tap) * DW_CT + cl] = w[(int64_t)c0 * KK + i];
    }
}

// y = act(scale * conv(x, w) + bias) + res, or raw y + statistics rows.  FLIP (stride 1 only): the data gradient, y = conv(x, rot180 w) + res.
template <typename T, int K, int S, bool FLIP, bool STATS>
__global__ __launch_bounds__(256) void dw_fwd_kernel(DwFwdArgs a) {
    constexpr int CH = ElemTraits<T>::CH, KK = K * K, PAD = K / 2, TW = DW_TW, L = (TW - 1) * S + K;
    typedef typename Chunk<T>::type RC;
    __shared__ __attribute__((aligned(16))) float sm[KK * DW_CT > 256 * 2 * CH ? KK * DW_CT : 256 * 2 * CH];
    const int c0 = blockIdx.y * DW_CT;
    const int ct = a.C - c0 < DW_CT ? a.C - c0 : DW_CT;
    const int Gt = ct / CH, rows = 256 / Gt;
    stage_taps<KK, FLIP>(a.w, c0, ct, sm);
    __syncthreads();
    const int r = threadIdx.x / Gt, g = threadIdx.x - r * Gt;
    const bool active = r < rows;
    const int cb = c0 + g * CH;  // this thread's first channel
    const T* xp = reinterpret_cast<const T*>(a.x.p);
    const T* rp = reinterpret_cast<const T*>(a.res);
    const T* zp = reinterpret_cast<const T*>(a.zero);
    T* yp = reinterpret_cast<T*>(const_cast<void*>(a.y.p));
    const int H = a.x.h, W = a.x.w, Ho = a.y.h, Wo = a.y.w;
    float sc[CH], bi[CH], s1[CH], s2[CH];
#pragma unroll
    for (int e = 0; e < CH; ++e) {
        sc[e] = (!STATS && active && a.scale) ? a.scale[cb + e] : 1.0f;
        bi[e] = (!STATS && active && a.bias) ? a.bias[cb + e] : 0.0f;
        s1[e] = s2[e] = 0.f;
    }
    if (active) {
        for (int64_t q = (int64_t)blockIdx.x * rows + r; q < a.runs; q += (int64_t)gridDim.x * rows) {
            const int t = (int)(q % a.runs_per_row);
            const int64_t nr = q / a.runs_per_row;
            const int oh = (int)(nr % Ho), n = (int)(nr / Ho);
            const int ow0 = t * TW;
            float acc[TW][CH];
#pragma unroll
            for (int j = 0; j < TW; ++j)
#pragma unroll
                for (int e = 0; e < CH; ++e) acc[j][e] = 0.f;
#pragma unroll 1  // (one tap row's loads in flight per wave: unrolled, the 40 chunks of a 5x5 run spill; the other waves cover the latency)
            for (int ky = 0; ky < K; ++ky) {
                // every tap is tested against the IMAGE; one outside it reads the library's 16 zero bytes instead (a select of the address,
                // no branch: all loads of the run are in flight together)
                const int ih = oh * S + ky - PAD;
                const bool rowok = (unsigned)ih < (unsigned)H;
                const T* xrow = xp + ((int64_t)n * H + (rowok ? ih : 0)) * W * a.x.ld + cb;
                RC xs[L];
#pragma unroll
                for (int l = 0; l < L; ++l) {
                    const int iw = ow0 * S + l - PAD;
                    const bool ok = rowok && (unsigned)iw < (unsigned)W;
                    const T* src = ok ? xrow + (uint32_t)iw * (uint32_t)a.x.ld : zp;
                    xs[l] = *reinterpret_cast<const RC*>(src);
                }
#pragma unroll
                for (int kx = 0; kx < K; ++kx) {
                    float wv[CH];
#pragma unroll
                    for (int v = 0; v < CH / 4; ++v) {
                        const f32x4 t4 = *reinterpret_cast<const f32x4*>(&sm[(ky * K + kx) * DW_CT + g * CH + v * 4]);
                        wv[v * 4 + 0] = t4[0]; wv[v * 4 + 1] = t4[1]; wv[v * 4 + 2] = t4[2]; wv[v * 4 + 3] = t4[3];
                    }
#pragma unroll
                    for (int j = 0; j < TW; ++j)
#pragma unroll
                        for (int e = 0; e < CH; ++e) acc[j][e] += (float)xs[j * S + kx][e] * wv[e];
                }
            }
#pragma unroll
            for (int j = 0; j < TW; ++j) {
                const int ow = ow0 + j;
                if (ow >= Wo) break;
                const int64_t po = ((int64_t)n * Ho + oh) * Wo + ow;
                RC o;
                if constexpr (STATS) {
#pragma unroll
                    for (int e = 0; e < CH; ++e) {
                        o[e] = from_f32<T>(acc[j][e]);
                        const float v = (float)o[e];  // the statistics are those of the stored (rounded) values
                        s1[e] += v;
                        s2[e] += v * v;
                    }
                } else {
                    RC rr = {};
                    if (rp) rr = *reinterpret_cast<const RC*>(rp + po * a.res_ld + cb);
#pragma unroll
                    for (int e = 0; e < CH; ++e) o[e] = from_f32<T>(apply_act_rt(acc[j][e] * sc[e] + bi[e], a.act) + (float)rr[e]);
                }
                *reinterpret_cast<RC*>(yp + po * a.y.ld + cb) = o;
            }
        }
    }
    if constexpr (STATS) {
        __syncthreads();  // the taps are no longer read: their LDS holds the partial sums now
        if (active) {
#pragma unroll
            for (int e = 0; e < CH; ++e) {
                sm[threadIdx.x * 2 * CH + e] = s1[e];
                sm[threadIdx.x * 2 * CH + CH + e] = s2[e];
            }
        }
        __syncthreads();
        for (int c = threadIdx.x; c < ct; c += 256) {
            const int gg = c / CH, e = c - gg * CH;
            float t1 = 0.f, t2 = 0.f;
            for (int rr = 0; rr < rows; ++rr) {  // fixed order: bit-reproducible rows
                t1 += sm[(rr * Gt + gg) * 2 * CH + e];
                t2 += sm[(rr * Gt + gg) * 2 * CH + CH + e];
            }
            a.part[((int64_t)blockIdx.x * 2 + 0) * a.C + c0 + c] = t1;
            a.part[((int64_t)blockIdx.x * 2 + 1) * a.C + c0 + c] = t2;
        }
    }
}

// (Only GhostBottleneck(s=2) reaches this kernel; it keeps a branch per tap and scalar LDS reads, and no probe has timed it.)
// Stride-S (S > 1) data gradient as a gather: input pixel (ih, iw) receives dy(oh, ow) * w(ky, kx) from the taps with ih + PAD - ky = S * oh,
// iw + PAD - kx = S * ow (the taps whose parity matches), oh / ow inside dy.  One thread per (pixel, chunk); no atomics.  x = dy, y = dx.
template <typename T, int K, int S> __global__ __launch_bounds__(256) void dw_dgrad_gather_kernel(DwFwdArgs a) {
    constexpr int CH = ElemTraits<T>::CH, KK = K * K, PAD = K / 2;
    typedef typename Chunk<T>::type RC;
    __shared__ __attribute__((aligned(16))) float sm[KK * DW_CT];
    const int c0 = blockIdx.y * DW_CT;
    const int ct = a.C - c0 < DW_CT ? a.C - c0 : DW_CT;
    const int Gt = ct / CH, rows = 256 / Gt;
    stage_taps<KK, false>(a.w, c0, ct, sm);
    __syncthreads();
    const int r = threadIdx.x / Gt, g = threadIdx.x - r * Gt;
    if (r >= rows) return;
    const int cb = c0 + g * CH;
    const T* dyp = reinterpret_cast<const T*>(a.x.p);
    const T* rp = reinterpret_cast<const T*>(a.res);
    T* dxp = reinterpret_cast<T*>(const_cast<void*>(a.y.p));
    const int Ho = a.x.h, Wo = a.x.w, H = a.y.h, W = a.y.w;
    for (int64_t p = (int64_t)blockIdx.x * rows + r; p < a.runs; p += (int64_t)gridDim.x * rows) {
        const int iw = (int)(p % W);
        const int64_t nr = p / W;
        const int ih = (int)(nr % H), n = (int)(nr / H);
        float acc[CH];
#pragma unroll
        for (int e = 0; e < CH; ++e) acc[e] = 0.f;
#pragma unroll
        for (int ky = 0; ky < K; ++ky) {
            const int ty = ih + PAD - ky;
            if (ty < 0 || ty % S != 0 || ty / S >= Ho) continue;
            const T* row = dyp + ((int64_t)n * Ho + ty / S) * Wo * a.x.ld + cb;
#pragma unroll
            for (int kx = 0; kx < K; ++kx) {
                const int tx = iw + PAD - kx;
                if (tx < 0 || tx % S != 0 || tx / S >= Wo) continue;
                const RC v = *reinterpret_cast<const RC*>(row + (int64_t)(tx / S) * a.x.ld);
#pragma unroll
                for (int e = 0; e < CH; ++e) acc[e] += (float)v[e] * sm[(ky * K + kx) * DW_CT + g * CH + e];
            }
        }
        RC rr = {}, o;
        if (rp) rr = *reinterpret_cast<const RC*>(rp + p * a.res_ld + cb);
#pragma unroll
        for (int e = 0; e < CH; ++e) o[e] = from_f32<T>(acc[e] + (float)rr[e]);
        *reinterpret_cast<RC*>(dxp + p * a.y.ld + cb) = o;
    }
}

struct DwWgradArgs {
    DwTensor x, dy;
    float* slab;  // [gridDim.x][k*k][C]
    int C;
    int runs_per_row;  // ceil(dy.w / TW)
    int64_t runs;      // dy.n * dy.h * runs_per_row
    const void* zero;
};

// slab[block][tap][c] = sum over the block's output pixels of dy(p, c) * x(tap of p, c).  A thread owns (chunk, tap row ky) and walks runs of
// DW_TW outputs of one row: DW_TW chunks of dy and the (DW_TW - 1) * S + K chunks of the input row under them, K x chunk accumulators.
template <typename T, int K, int S> __global__ __launch_bounds__(256) void dw_wgrad_kernel(DwWgradArgs a) {
    constexpr int CH = ElemTraits<T>::CH, KK = K * K, PAD = K / 2, TW = DW_TW, L = (TW - 1) * S + K;
    typedef typename Chunk<T>::type RC;
    __shared__ float red[256 * K * CH];
    const int c0 = blockIdx.y * DW_CTW;
    const int ct = a.C - c0 < DW_CTW ? a.C - c0 : DW_CTW;
    const int Gt = ct / CH, per = K * Gt, rows = 256 / per;
    const int r = threadIdx.x / per, rem = threadIdx.x - r * per;
    const int ky = rem / Gt, g = rem - ky * Gt;
    const int cb = c0 + g * CH;
    const T* xp = reinterpret_cast<const T*>(a.x.p);
    const T* dyp = reinterpret_cast<const T*>(a.dy.p);
    const T* zp = reinterpret_cast<const T*>(a.zero);
    const int H = a.x.h, W = a.x.w, Ho = a.dy.h, Wo = a.dy.w;
    float acc[K][CH];
#pragma unroll
    for (int kx = 0; kx < K; ++kx)
#pragma unroll
        for (int e = 0; e < CH; ++e) acc[kx][e] = 0.f;
    if (r < rows) {
        for (int64_t q = (int64_t)blockIdx.x * rows + r; q < a.runs; q += (int64_t)gridDim.x * rows) {
            const int t = (int)(q % a.runs_per_row);
            const int64_t nr = q / a.runs_per_row;
            const int oh = (int)(nr % Ho), n = (int)(nr / Ho);
            const int ow0 = t * TW;
            const int ih = oh * S + ky - PAD;
            const bool rowok = (unsigned)ih < (unsigned)H;  // (tested against the image; outside it the taps read zeros)
            const T* xrow = xp + ((int64_t)n * H + (rowok ? ih : 0)) * W * a.x.ld + cb;
            const T* dyrow = dyp + ((int64_t)n * Ho + oh) * Wo * a.dy.ld + cb;
            RC d[TW], xs[L];
#pragma unroll
            for (int j = 0; j < TW; ++j) {
                const T* src = (rowok && ow0 + j < Wo) ? dyrow + (uint32_t)(ow0 + j) * (uint32_t)a.dy.ld : zp;
                d[j] = *reinterpret_cast<const RC*>(src);
            }
#pragma unroll
            for (int l = 0; l < L; ++l) {
                const int iw = ow0 * S + l - PAD;
                const T* src = (rowok && (unsigned)iw < (unsigned)W) ? xrow + (uint32_t)iw * (uint32_t)a.x.ld : zp;
                xs[l] = *reinterpret_cast<const RC*>(src);
            }
#pragma unroll
            for (int j = 0; j < TW; ++j)
#pragma unroll
                for (int kx = 0; kx < K; ++kx)
#pragma unroll
                    for (int e = 0; e < CH; ++e) acc[kx][e] += (float)d[j][e] * (float)xs[j * S + kx][e];
        }
#pragma unroll
        for (int kx = 0; kx < K; ++kx)
#pragma unroll
            for (int e = 0; e < CH; ++e) red[threadIdx.x * (K * CH) + kx * CH + e] = acc[kx][e];
    }
    __syncthreads();
    for (int i = threadIdx.x; i < KK * ct; i += 256) {
        const int tap = i / ct, c = i - tap * ct;
        const int tky = tap / K, tkx = tap - tky * K, gg = c / CH, e = c - gg * CH;
        float s = 0.f;
        for (int rr = 0; rr < rows; ++rr) s += red[((rr * K + tky) * Gt + gg) * (K * CH) + tkx * CH + e];  // fixed order
        a.slab[((int64_t)blockIdx.x * KK + tap) * a.C + c0 + c] = s;
    }
}

// dw[c][tap] = sum over the slab rows in a fixed order: a workgroup owns 32 consecutive (tap, channel) elements, thread row j adds the slab rows
// j, j + 8, ... in order, thread row 0 adds the eight partial sums in order
__global__ __launch_bounds__(256) void dw_wgrad_sum_kernel(const float* __restrict__ slab, int blocks, int KK, int C, float* __restrict__ dw) {
    __shared__ float part[8][32];
    const int el = threadIdx.x & 31, j = threadIdx.x >> 5;
    const int i = blockIdx.x * 32 + el;  // = tap * C + c
    float s = 0.f;
    if (i < KK * C)
        for (int b = j; b < blocks; b += 8) s += slab[(int64_t)b * KK * C + i];
    part[j][el] = s;
    __syncthreads();
    if (j == 0 && i < KK * C) {
        float tot = 0.f;
#pragma unroll
        for (int q = 0; q < 8; ++q) tot += part[q][el];
        const int tap = i / C, c = i - tap * C;
        dw[(int64_t)c * KK + tap] = tot;
    }
}

bool dw_vec_ok(const ymi_tensor* t) {
    const int ch = t->dtype == YMI_BF16 ? 8 : 4;
    return t->c % ch == 0 && t->ld % ch == 0 && ((uintptr_t)t->data & 15) == 0;
}
int64_t dw_out(int64_t h, int64_t k, int64_t s) { return (h + 2 * (k / 2) - k) / s + 1; }
// workgroups along the pixel axis for `units` work units, `chunks` chunks per pixel in the widest channel tile
int dw_blocks(int64_t units, int chunks, int cap) {
    const int rows = 256 / chunks;
    const int64_t b = (units + rows - 1) / rows;
    return (int)(b < 1 ? 1 : b > cap ? cap : b);
}
int dw_tile_chunks(int64_t c, int ct, int ch) { return (int)((c < ct ? c : ct) / ch); }

template <typename T, int K, int S> void launch_fwd(const DwFwdArgs& a, dim3 grid, bool flip, hipStream_t s) {
    if (flip) {
        if constexpr (S == 1) hipLaunchKernelGGL((dw_fwd_kernel<T, K, 1, true, false>), grid, dim3(256), 0, s, a);
    } else if (a.part) hipLaunchKernelGGL((dw_fwd_kernel<T, K, S, false, true>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((dw_fwd_kernel<T, K, S, false, false>), grid, dim3(256), 0, s, a);
}
template <typename T> void launch_fwd_ks(const DwFwdArgs& a, int k, int stride, dim3 grid, bool flip, hipStream_t s) {
    if (k == 3 && stride == 1) launch_fwd<T, 3, 1>(a, grid, flip, s);
    else if (k == 3) launch_fwd<T, 3, 2>(a, grid, flip, s);
    else if (stride == 1) launch_fwd<T, 5, 1>(a, grid, flip, s);
    else launch_fwd<T, 5, 2>(a, grid, flip, s);
}
template <typename T> void launch_wgrad_ks(const DwWgradArgs& a, int k, int stride, dim3 grid, hipStream_t s) {
    if (k == 3 && stride == 1) hipLaunchKernelGGL((dw_wgrad_kernel<T, 3, 1>), grid, dim3(256), 0, s, a);
    else if (k == 3) hipLaunchKernelGGL((dw_wgrad_kernel<T, 3, 2>), grid, dim3(256), 0, s, a);
    else if (stride == 1) hipLaunchKernelGGL((dw_wgrad_kernel<T, 5, 1>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((dw_wgrad_kernel<T, 5, 2>), grid, dim3(256), 0, s, a);
}

// the checks every entry shares: `big` is the stride-1-sized side (x / dx), `small` the output side (y / dy)
int dw_check(const char* what, const ymi_tensor* big, const ymi_tensor* small, const float* w, int64_t k, int64_t stride) {
    YMI_CHECK_ARG(ymi_tensor_ok(big) && ymi_tensor_ok(small) && w, "%s: NULL or malformed tensor", what);
    YMI_CHECK_ARG(k == 3 || k == 5, "%s: k = %lld (depthwise kernels are built for k in {3, 5})", what, (long long)k);
    YMI_CHECK_ARG(stride == 1 || stride == 2, "%s: stride %lld (1 or 2)", what, (long long)stride);
    YMI_CHECK_ARG(big->dtype == small->dtype && big->c == small->c && big->n == small->n, "%s: pure depthwise only (equal channels, batch, dtype)", what);
    YMI_CHECK_ARG(small->h == dw_out(big->h, k, stride) && small->w == dw_out(big->w, k, stride), "%s: output is %lldx%lld, expected %lldx%lld", what,
                  (long long)small->h, (long long)small->w, (long long)dw_out(big->h, k, stride), (long long)dw_out(big->w, k, stride));
    YMI_CHECK_ARG(dw_vec_ok(big) && dw_vec_ok(small), "%s: channels and row strides in whole 16-byte chunks (C %% %d == 0), 16-byte aligned data", what,
                  big->dtype == YMI_BF16 ? 8 : 4);
    for (const ymi_tensor* t : {big, small})  // (the kernels index pixels in 31 bits and a row's elements, w * ld, in 32)
        YMI_CHECK_ARG(ymi_pixels(t) * t->ld < (1ll << 40) && ymi_pixels(t) < (1ll << 31) && t->w * t->ld < (1ll << 31), "%s: tensor too large", what);
    return YMI_OK;
}

}  // namespace

extern "C" int64_t ymi_dwconv2d_stat_blocks(int64_t n, int64_t ho, int64_t wo, int64_t c) {
    if (n <= 0 || ho <= 0 || wo <= 0 || c < 4) return 1;
    // float32 has the most chunks per pixel, hence the fewest pixel rows per workgroup and the most workgroups
    return dw_blocks(n * ho * ((wo + DW_TW - 1) / DW_TW), dw_tile_chunks(c, DW_CT, 4), DW_MAX_BLOCKS);
}

extern "C" int ymi_dwconv2d_fwd(const ymi_tensor* x, const float* w, int64_t k, int64_t stride, const float* scale, const float* bias, int32_t act,
                                const ymi_tensor* residual, const ymi_tensor* y, float* stat_partials, int64_t* host_stat_blocks, void* stream) {
    int rc = dw_check("dwconv2d_fwd", x, y, w, k, stride);
    if (rc) return rc;
    YMI_CHECK_ARG(act == YMI_ACT_NONE || act == YMI_ACT_SILU || act == YMI_ACT_GELU, "dwconv2d_fwd: activation %d", act);
    if (residual)
        YMI_CHECK_ARG(ymi_tensor_ok(residual) && ymi_same_shape(residual, y) && residual->dtype == y->dtype && dw_vec_ok(residual), "dwconv2d_fwd: residual");
    if (stat_partials)
        YMI_CHECK_ARG(!scale && !bias && !residual && act == YMI_ACT_NONE, "dwconv2d_fwd: the statistics form writes the raw output (no scale, bias, activation, residual)");
    const int ch = x->dtype == YMI_BF16 ? 8 : 4;
    DwFwdArgs a{dwt(x), dwt(y), residual ? residual->data : nullptr, residual ? residual->ld : 0, w, scale, bias, stat_partials, (int)x->c, act,
                (int)((y->w + DW_TW - 1) / DW_TW), 0, ymi_zero_page()};
    a.runs = y->n * y->h * a.runs_per_row;
    const dim3 grid((unsigned)dw_blocks(a.runs, dw_tile_chunks(x->c, DW_CT, ch), DW_MAX_BLOCKS), (unsigned)((x->c + DW_CT - 1) / DW_CT));
    if (x->dtype == YMI_BF16) launch_fwd_ks<bf16_t>(a, (int)k, (int)stride, grid, false, (hipStream_t)stream);
    else launch_fwd_ks<float>(a, (int)k, (int)stride, grid, false, (hipStream_t)stream);
    YMI_CHECK_LAUNCH("dwconv2d_fwd");
    if (host_stat_blocks) *host_stat_blocks = grid.x;
    return YMI_OK;
}

extern "C" int ymi_dwconv2d_bn_act_fwd(const ymi_tensor* x, const float* w, int64_t k, int64_t stride, const float* gamma, const float* beta,
                                       float* running_mean, float* running_var, float momentum, float eps, int32_t act, const ymi_tensor* residual,
                                       const ymi_tensor* raw, const ymi_tensor* out, float* save_mean, float* save_invstd, void* workspace,
                                       size_t workspace_bytes, void* stream) {
    YMI_CHECK_ARG(ymi_tensor_ok(raw) && ymi_tensor_ok(out) && workspace, "dwconv2d_bn_act_fwd: NULL or malformed tensor");
    const int64_t c = raw->c, m = ymi_pixels(raw);
    const size_t need = (size_t)(ymi_dwconv2d_stat_blocks(raw->n, raw->h, raw->w, c) * 2 * c + 2 * c) * sizeof(float);
    if (workspace_bytes < need) {
        ymi_set_error("dwconv2d_bn_act_fwd: workspace %zu < %zu bytes", workspace_bytes, need);
        return YMI_EWORKSPACE;
    }
    float* scale = reinterpret_cast<float*>(workspace);
    float* shift = scale + c;
    float* part = shift + c;
    int64_t blocks = 0;
    int rc = ymi_dwconv2d_fwd(x, w, k, stride, nullptr, nullptr, YMI_ACT_NONE, nullptr, raw, part, &blocks, stream);
    if (rc) return rc;
    rc = ymi_bn_finalize(part, blocks, m, c, gamma, beta, running_mean, running_var, momentum, eps, scale, shift, save_mean, save_invstd, stream);
    if (rc) return rc;
    return ymi_scale_shift_act(raw, scale, shift, act, residual, out, stream);
}

extern "C" int ymi_dwconv2d_bwd_data(const ymi_tensor* dy, const float* w, int64_t k, int64_t stride, const ymi_tensor* add, const ymi_tensor* dx,
                                     void* stream) {
    int rc = dw_check("dwconv2d_bwd_data", dx, dy, w, k, stride);
    if (rc) return rc;
    if (add) YMI_CHECK_ARG(ymi_tensor_ok(add) && ymi_same_shape(add, dx) && add->dtype == dx->dtype && dw_vec_ok(add), "dwconv2d_bwd_data: addend");
    const int ch = dx->dtype == YMI_BF16 ? 8 : 4;
    const bool gather = stride != 1;
    // (the kernels call their source x and their destination y)
    DwFwdArgs a{dwt(dy), dwt(dx), add ? add->data : nullptr, add ? add->ld : 0, w, nullptr, nullptr, nullptr, (int)dx->c, YMI_ACT_NONE,
                (int)((dx->w + DW_TW - 1) / DW_TW), 0, ymi_zero_page()};
    a.runs = gather ? ymi_pixels(dx) : dx->n * dx->h * a.runs_per_row;
    const dim3 grid((unsigned)dw_blocks(a.runs, dw_tile_chunks(dx->c, DW_CT, ch), DW_MAX_BLOCKS), (unsigned)((dx->c + DW_CT - 1) / DW_CT));
    hipStream_t s = (hipStream_t)stream;
    if (!gather) {
        if (dx->dtype == YMI_BF16) launch_fwd_ks<bf16_t>(a, (int)k, 1, grid, true, s);
        else launch_fwd_ks<float>(a, (int)k, 1, grid, true, s);
    } else if (dx->dtype == YMI_BF16) {
        if (k == 3) hipLaunchKernelGGL((dw_dgrad_gather_kernel<bf16_t, 3, 2>), grid, dim3(256), 0, s, a);
        else hipLaunchKernelGGL((dw_dgrad_gather_kernel<bf16_t, 5, 2>), grid, dim3(256), 0, s, a);
    } else {
        if (k == 3) hipLaunchKernelGGL((dw_dgrad_gather_kernel<float, 3, 2>), grid, dim3(256), 0, s, a);
        else hipLaunchKernelGGL((dw_dgrad_gather_kernel<float, 5, 2>), grid, dim3(256), 0, s, a);
    }
    YMI_CHECK_LAUNCH("dwconv2d_bwd_data");
    return YMI_OK;
}

static int dw_wgrad_blocks(int64_t pixels) {
    const int64_t b = (pixels + 127) / 128;
    return (int)(b < 1 ? 1 : b > DW_WG_BLOCKS ? DW_WG_BLOCKS : b);
}

extern "C" size_t ymi_dwconv2d_bwd_weight_workspace(int64_t n, int64_t ho, int64_t wo, int64_t c, int64_t k) {
    if (n <= 0 || ho <= 0 || wo <= 0 || c <= 0 || k <= 0) return 0;
    return (size_t)dw_wgrad_blocks(n * ho * wo) * (size_t)(k * k * c) * sizeof(float);
}

extern "C" int ymi_dwconv2d_bwd_weight(const ymi_tensor* x, const ymi_tensor* dy, int64_t k, int64_t stride, float* dw, void* workspace,
                                       size_t workspace_bytes, void* stream) {
    int rc = dw_check("dwconv2d_bwd_weight", x, dy, dw, k, stride);
    if (rc) return rc;
    YMI_CHECK_ARG(workspace && ((uintptr_t)workspace & 3) == 0, "dwconv2d_bwd_weight: NULL or unaligned workspace");
    const size_t need = ymi_dwconv2d_bwd_weight_workspace(dy->n, dy->h, dy->w, dy->c, k);
    if (workspace_bytes < need) {
        ymi_set_error("dwconv2d_bwd_weight: workspace %zu < %zu bytes", workspace_bytes, need);
        return YMI_EWORKSPACE;
    }
    const int blocks = dw_wgrad_blocks(ymi_pixels(dy));
    DwWgradArgs a{dwt(x), dwt(dy), reinterpret_cast<float*>(workspace), (int)x->c, (int)((dy->w + DW_TW - 1) / DW_TW), 0, ymi_zero_page()};
    a.runs = dy->n * dy->h * a.runs_per_row;
    const dim3 grid((unsigned)blocks, (unsigned)((x->c + DW_CTW - 1) / DW_CTW));
    hipStream_t s = (hipStream_t)stream;
    if (x->dtype == YMI_BF16) launch_wgrad_ks<bf16_t>(a, (int)k, (int)stride, grid, s);
    else launch_wgrad_ks<float>(a, (int)k, (int)stride, grid, s);
    YMI_CHECK_LAUNCH("dwconv2d_bwd_weight");
    const int elems = (int)(k * k * x->c);
    hipLaunchKernelGGL(dw_wgrad_sum_kernel, dim3((unsigned)((elems + 31) / 32)), dim3(256), 0, s, a.slab, blocks, (int)(k * k), (int)x->c, dw);
    YMI_CHECK_LAUNCH("dwconv2d_bwd_weight (row sum)");
    return YMI_OK;
}
