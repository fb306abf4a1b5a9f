// CBAM (fork's nn/modules/cbam.py) for NHWC tensors: memory-bound wavefront kernels.
//
//   ca  = sigmoid(W2 relu(W1 avg_p x) + W2 relu(W1 max_p x))          [N][C]
//   x1  = x * ca
//   sm  = [mean_c x1, max_c x1]                                        [N][H][W][2]
//   sa  = sigmoid(conv_kxk(sm))                                        [N][H][W]
//   out = x1 * sa
//
// Forward = 4 launches: pool (x read once, coalesced along C), MLP (one workgroup per image, weights
// in registers/LDS), spatial statistics (one wave per pixel: 64 lanes x 16 B = 512 bf16 channels per
// load, wave-reduce), apply (k*k*2-tap stencil from the tiny f32 map + final scale).  x is streamed
// 3 times (pool, stats, apply) and out written once; the second and third reads hit L2 / Infinity
// Cache for the shapes of this model (26 MB at bs 32).
#include <initializer_list>

#include "common.h"

struct CV {
    const void* p;
    int64_t ld;
};
// every kernel here reads and writes 4-element Packs (common.h: vec4_ok); row p of a view
template <typename T> __device__ __forceinline__ T* row(CV v, int64_t p) { return reinterpret_cast<T*>(const_cast<void*>(v.p)) + p * v.ld; }

// ---- the rules the kernels share ---------------------------------------------------------------------------------------------------
// a wave and its pixel: p = n * HW + q of the batch, the ca row of its image
struct PixWave {
    int lane, n, q;
    int64_t p;
    bool live;
    const float* cap;
};
__device__ __forceinline__ PixWave pix_wave(int64_t p, int n, int HW, int C, const float* ca, bool live = true) {
    return PixWave{(int)(threadIdx.x & 63), n, (int)(p - (int64_t)n * HW), p, live, ca + (int64_t)n * C};
}
// the launches of ceil(NP / 4) workgroups of four waves: wave w of workgroup b has pixel 4 b + w
__device__ __forceinline__ PixWave grid_pix_wave(int64_t NP, int HW, int C, const float* ca) {
    const int64_t p = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    return pix_wave(p, (int)(p / HW), HW, C, ca, p < NP);
}
// a lane's channel groups c .. c + 3: 256 channels a trip
template <typename F> __device__ __forceinline__ void for_chan4(int C, int lane, F&& f) { for (int c = lane * 4; c < C; c += 256) f(c); }
__device__ __forceinline__ bool in_map(int h, int w, int H, int W) { return h >= 0 && h < H && w >= 0 && w < W; }
// f(t, q) for this lane's taps t of the K x K stencil around (h, w) whose neighbour q = hh * W + ww lies in the map; SIGN -1: the adjoint's p - off_t
template <int SIGN, typename F> __device__ __forceinline__ void stencil_taps(int h, int w, int H, int W, int K, int lane, F&& f) {
    for (int t = lane, R = K / 2; t < K * K; t += 64) {
        const int hh = h + SIGN * (t / K - R), ww = w + SIGN * (t % K - R);
        if (in_map(hh, ww, H, W)) f(t, hh * W + ww);
    }
}
// the first maximum: in scan order strictly greater wins; two scans combine by "greater, or equal with the lower index"
__device__ __forceinline__ void first_max_scan(float v, int i, float& m, int& bi) { if (v > m) { m = v; bi = i; } }
__device__ __forceinline__ void first_max_merge(float v, int i, float& m, int& bi) { if (v > m || (v == m && i < bi)) { m = v; bi = i; } }
// the channel MLP's first layer (both MLP kernels): pooled[n] into LDS; hidden unit h of this wave, a = W1[h] avg and m = W1[h] max by lanes,
// then wave_sum.  extra(c) rides in the same trip (the kernels are chains of load latencies: every round of loads is issued together)
__device__ __forceinline__ void stage_pooled(const float* pooled, int n, int C, float* sp) {
    for (int i = threadIdx.x, nt = blockDim.x; i < 2 * C; i += nt) sp[i] = pooled[(int64_t)n * 2 * C + i];
}
template <typename F> __device__ __forceinline__ void hidden_unit(const float* w1, const float* sp, int C, int h, int lane, float& a, float& m, F&& extra) {
    float acc_m = 0.f, acc_a = 0.f;  // (in this order: declared a first, the compiler pairs the two chains as (m, a) and cbam_mlp_kernel takes 66 VGPRs for 60)
    const float* wr = w1 + (int64_t)h * C;
#pragma unroll 8
    for (int c = lane; c < C; c += 64) {
        const float w = wr[c];
        acc_a += w * sp[c];
        acc_m += w * sp[C + c];
        extra(c);
    }
    a = wave_sum(acc_a);
    m = wave_sum(acc_m);
}
__device__ __forceinline__ float relu_sum(float a, float m) { return fmaxf(a, 0.f) + fmaxf(m, 0.f); }

// ---------------------------------------------------------------------------------- forward
// one pixel of a pixel lane's four channels (a function: as a lambda that captures the three arrays the loops' adds and compares come out in another order)
__device__ __forceinline__ void pool_pixel(const float (&v)[4], int p, float (&sum)[4], float (&mx)[4], int (&ix)[4]) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        sum[r] += v[r];
        first_max_scan(v[r], p, mx[r], ix[r]);
    }
}
// grid (ceil(C/CB), N); block 256 = (CB/4 channel groups) x pixel lanes
template <typename T>
__global__ __launch_bounds__(256) void cbam_pool_kernel(CV x, int HW, int C, float* __restrict__ pooled, int* __restrict__ amax) {
    constexpr int CB = 64;            // channels per block
    constexpr int GX = CB / 4;        // 16 channel groups of 4
    constexpr int PY = 256 / GX;      // 16 pixel lanes
    __shared__ float s_sum[PY][CB];
    __shared__ float s_max[PY][CB];
    __shared__ int s_idx[PY][CB];
    const int gx = threadIdx.x % GX, py = threadIdx.x / GX;
    const int n = blockIdx.y, c = blockIdx.x * CB + gx * 4;
    const T* xp = row<T>(x, (int64_t)n * HW);
    float sum[4] = {0.f, 0.f, 0.f, 0.f}, mx[4];
    int ix[4] = {0, 0, 0, 0};
#pragma unroll
    for (int r = 0; r < 4; ++r) mx[r] = -__builtin_inff();
    if (c < C) {
        int p = py;
        for (; p + 3 * PY < HW; p += 4 * PY) {  // four pixels in flight per lane (the loop is a chain of load latencies otherwise)
            float v[4][4];
#pragma unroll
            for (int u = 0; u < 4; ++u) Pack<T, 4>::load(xp + (int64_t)(p + u * PY) * x.ld + c, v[u]);
#pragma unroll
            for (int u = 0; u < 4; ++u) pool_pixel(v[u], p + u * PY, sum, mx, ix);
        }
        for (; p < HW; p += PY) {
            float v[4];
            Pack<T, 4>::load(xp + (int64_t)p * x.ld + c, v);
            pool_pixel(v, p, sum, mx, ix);
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        s_sum[py][gx * 4 + r] = sum[r];
        s_max[py][gx * 4 + r] = mx[r];
        s_idx[py][gx * 4 + r] = ix[r];
    }
    __syncthreads();
    if (threadIdx.x < CB) {
        const int cc = blockIdx.x * CB + threadIdx.x;
        if (cc < C) {
            float s = 0.f, m = -__builtin_inff();
            int bi = 0;
            for (int q = 0; q < PY; ++q) {
                s += s_sum[q][threadIdx.x];
                first_max_merge(s_max[q][threadIdx.x], s_idx[q][threadIdx.x], m, bi);
            }
            pooled[((int64_t)n * 2 + 0) * C + cc] = s / (float)HW;
            pooled[((int64_t)n * 2 + 1) * C + cc] = m;
            amax[(int64_t)n * C + cc] = bi;
        }
    }
}

// one block (any multiple of 64 threads; launched with 1024) per image: hidden = relu(W1 avg) + relu(W1 max); ca = sigmoid(W2 hidden).
// Pure latency: three dependent rounds of loads; every round's loads are issued together (unrolled), one hidden unit or two per wave.
__global__ __launch_bounds__(1024) void cbam_mlp_kernel(const float* __restrict__ pooled, const float* __restrict__ w1, const float* __restrict__ w2,
                                                        int C, int Hd, float* __restrict__ ca) {
    extern __shared__ float sh[];  // [2][C] pooled, [Hd] hidden sum
    float* sp = sh;
    float* hs = sh + 2 * C;
    const int n = blockIdx.x, nt = blockDim.x, nw = nt >> 6;
    stage_pooled(pooled, n, C, sp);
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int h = wave; h < Hd; h += nw) {
        float a, m;
        hidden_unit(w1, sp, C, h, lane, a, m, [](int) {});
        if (lane == 0) hs[h] = relu_sum(a, m);
    }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += nt) {
        float z = 0.f;
        const float* wr = w2 + (int64_t)c * Hd;
#pragma unroll 8
        for (int h = 0; h < Hd; ++h) z += wr[h] * hs[h];
        ca[(int64_t)n * C + c] = sigmoidf_(z);
    }
}

// one wave per pixel: mean / max (+ first arg-max channel) over C of x*ca
template <typename T>
__global__ __launch_bounds__(256) void cbam_stats_kernel(CV x, int64_t NP, int HW, int C, const float* __restrict__ ca, float* __restrict__ smap,
                                                         int* __restrict__ sarg) {
    const PixWave pw = grid_pix_wave(NP, HW, C, ca);
    if (!pw.live) return;
    const T* xp = row<T>(x, pw.p);
    float s = 0.f, m = -__builtin_inff();
    int mi = 0x7fffffff;
    for_chan4(C, pw.lane, [&](int c) {
        float v[4];
        Pack<T, 4>::load(xp + c, v);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float t = v[r] * pw.cap[c + r];
            s += t;
            first_max_scan(t, c + r, m, mi);
        }
    });
    s = wave_sum(s);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) first_max_merge(__shfl_xor(m, o, 64), __shfl_xor(mi, o, 64), m, mi);
    if (pw.lane == 0) {
        smap[pw.p * 2 + 0] = s / (float)C;
        smap[pw.p * 2 + 1] = m;
        sarg[pw.p] = mi;
    }
}

// one wave per pixel: sa = sigmoid(stencil), out = x*ca*sa
template <typename T>
__global__ __launch_bounds__(256) void cbam_apply_kernel(CV x, CV out, int N, int H, int W, int C, const float* __restrict__ ca,
                                                         const float* __restrict__ smap, const float* __restrict__ wsa, int K,
                                                         float* __restrict__ sa_out) {
    const PixWave pw = grid_pix_wave((int64_t)N * H * W, H * W, C, ca);
    if (!pw.live) return;
    const float* sm = smap + (int64_t)pw.n * H * W * 2;
    float u = 0.f;
    stencil_taps<1>(pw.q / W, pw.q % W, H, W, K, pw.lane, [&](int t, int q) { u += wsa[t] * sm[q * 2 + 0] + wsa[K * K + t] * sm[q * 2 + 1]; });
    u = wave_sum(u);
    const float sa = sigmoidf_(u);
    if (pw.lane == 0) sa_out[pw.p] = sa;
    const T* xp = row<T>(x, pw.p);
    T* op = row<T>(out, pw.p);
    for_chan4(C, pw.lane, [&](int c) {
        float v[4];
        Pack<T, 4>::load(xp + c, v);
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = v[r] * pw.cap[c + r] * sa;
        Pack<T, 4>::store(op + c, v);
    });
}

// ---------------------------------------------------------------------------------- host side
template <typename... P, typename... Q> static void launch(void (*kernel)(P...), dim3 grid, dim3 block, size_t lds, hipStream_t s, Q... args) {
    hipLaunchKernelGGL(kernel, grid, block, lds, s, args...);
}
// what the forward and the backward ask of their maps (the first gives shape and dtype) and of hidden / ksa
static int cbam_check(const char* entry, std::initializer_list<const ymi_tensor*> maps, int64_t hidden, int64_t ksa) {
    const ymi_tensor* x = *maps.begin();
    for (const ymi_tensor* t : maps) YMI_CHECK_ARG(ymi_tensor_ok(t) && ymi_same_shape(x, t) && x->dtype == t->dtype, "%s: tensors", entry);
    for (const ymi_tensor* t : maps) YMI_CHECK_ARG(vec4_ok(t), "%s: channels, ld and the base of every tensor must be multiples of 4 elements", entry);
    YMI_CHECK_ARG(hidden >= 1 && hidden <= 1024 && (ksa == 3 || ksa == 7), "%s: hidden/kernel", entry);
    return YMI_OK;
}

extern "C" int ymi_cbam_fwd(const ymi_tensor* x, const float* w1, const float* w2, int64_t hidden, const float* wsa, int64_t ksa,
                            const ymi_tensor* out, float* ca, float* pooled, int32_t* pool_argmax, float* smap, int32_t* smap_argmax,
                            float* sa, void* stream) {
    if (int rc = cbam_check("cbam_fwd", {x, out}, hidden, ksa)) return rc;
    YMI_CHECK_ARG(w1 && w2 && wsa && ca && pooled && pool_argmax && smap && smap_argmax && sa, "cbam_fwd: null buffer");
    hipStream_t s = (hipStream_t)stream;
    const int N = (int)x->n, H = (int)x->h, W = (int)x->w, C = (int)x->c, HW = H * W;
    const int64_t NP = (int64_t)N * HW;
    CV xv{x->data, x->ld}, ov{out->data, out->ld};
    dim3 gp((C + 63) / 64, N), gw((unsigned)((NP + 3) / 4));
    const size_t mlp_lds = (size_t)(2 * C + hidden) * sizeof(float);
    dispatch_dtype(x->dtype, [&](auto t) {
        typedef typename decltype(t)::type T;
        launch(cbam_pool_kernel<T>, gp, dim3(256), 0, s, xv, HW, C, pooled, pool_argmax);
        launch(cbam_mlp_kernel, dim3(N), dim3(1024), mlp_lds, s, pooled, w1, w2, C, (int)hidden, ca);
        launch(cbam_stats_kernel<T>, gw, dim3(256), 0, s, xv, NP, HW, C, ca, smap, smap_argmax);
        launch(cbam_apply_kernel<T>, gw, dim3(256), 0, s, xv, ov, N, H, W, C, ca, smap, wsa, (int)ksa, sa);
    });
    YMI_CHECK_LAUNCH("cbam_fwd");
    return YMI_OK;
}

// --------------------------------------------------------------------------------- backward
// B1: du[p] = (sum_c dout*x*ca) * sa*(1-sa)        (one wave per pixel)
template <typename T>
__global__ __launch_bounds__(256) void cbam_bwd_du_kernel(CV x, CV dout, int64_t NP, int HW, int C, const float* __restrict__ ca,
                                                          const float* __restrict__ sa, float* __restrict__ du) {
    const PixWave pw = grid_pix_wave(NP, HW, C, ca);
    if (!pw.live) return;
    const T* xp = row<T>(x, pw.p);
    const T* dp = row<T>(dout, pw.p);
    float s = 0.f;
    for_chan4(C, pw.lane, [&](int c) {
        float v[4], d[4];
        Pack<T, 4>::load(xp + c, v);
        Pack<T, 4>::load(dp + c, d);
#pragma unroll
        for (int r = 0; r < 4; ++r) s += d[r] * v[r] * pw.cap[c + r];
    });
    s = wave_sum(s);
    if (pw.lane == 0) {
        const float a = sa[pw.p];
        du[pw.p] = s * a * (1.f - a);
    }
}

// B2: dsm[p][j] = sum_t du[p - off_t] * wsa[j][t]   (adjoint stencil), then
//     dx1 = dout*sa + dsm0/C + [c==argmax]*dsm1 ;  dx = dx1*ca ;  dca partial[n][pixel-block][c] += dx1*x
// one wave per pixel; the per-image reduction of dx1*x is done by B3 from `dcap` partials written per pixel group.
template <typename T>
__global__ __launch_bounds__(256) void cbam_bwd_dx_kernel(CV x, CV dout, CV dx, int N, int H, int W, int C, const float* __restrict__ ca,
                                                          const float* __restrict__ sa, const float* __restrict__ du,
                                                          const int* __restrict__ sarg, const float* __restrict__ wsa, int K,
                                                          float* __restrict__ dcap /*[N][PB][C]*/, int PB) {
    __shared__ float part[4][1024 + 4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, HW = H * W;
    // blockIdx.x = n * PB + pb ; each block walks pixels pb*4+wv, +4*PB, ... of image n (wave per pixel)
    const int n = blockIdx.x / PB, pb = blockIdx.x % PB;
    const float* dun = du + (int64_t)n * HW;
    // per-wave accumulation of dx1*x over its pixels, channel c = lane*4 + 256*i + r  (C <= 1024 -> i < 4)
    float acc[4][4] = {};
    for (int q = pb * 4 + wv; q < HW; q += 4 * PB) {
        const PixWave pw = pix_wave((int64_t)n * HW + q, n, HW, C, ca);
        float d0 = 0.f, d1 = 0.f;
        // forward: u[p'] += wsa[j][t] * sm[p' + (ty-R, tx-R)]  =>  dsm[p] gets du[p - off] * wsa[j][t]
        stencil_taps<-1>(q / W, q % W, H, W, K, lane, [&](int t, int nb) {
            const float g = dun[nb];
            d0 += g * wsa[t];
            d1 += g * wsa[K * K + t];
        });
        d0 = wave_sum(d0);
        d1 = wave_sum(d1);
        const float a = sa[pw.p];
        const int am = sarg[pw.p];
        const T* xp = row<T>(x, pw.p);
        const T* dp = row<T>(dout, pw.p);
        T* op = row<T>(dx, pw.p);
        const float dmean = d0 / (float)C;
#pragma unroll
        for (int i = 0; i < 4; ++i) {  // for_chan4's trips with compile-time slots: acc stays in registers
            const int c = lane * 4 + 256 * i;
            if (c < C) {
                float v[4], d[4], o[4];
                Pack<T, 4>::load(xp + c, v);
                Pack<T, 4>::load(dp + c, d);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float dx1 = d[r] * a + dmean + ((c + r == am) ? d1 : 0.f);
                    o[r] = dx1 * pw.cap[c + r];
                    acc[i][r] += dx1 * v[r];
                }
                Pack<T, 4>::store(op + c, o);
            }
        }
    }
    // combine the 4 waves of the block, write one partial row per block
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int c = lane * 4 + 256 * i + r;
            if (c < 1024) part[wv][c] = acc[i][r];
        }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += 256)
        dcap[((int64_t)n * PB + pb) * C + c] = part[0][c] + part[1][c] + part[2][c] + part[3][c];
}

// B3: per image: dca -> dz -> hidden grads -> d_avg, d_max ; stores dz[N][C], hsum[N][Hd], dpre[N][2][Hd]
__global__ __launch_bounds__(1024) void cbam_bwd_mlp_kernel(const float* __restrict__ dcap, int PB, const float* __restrict__ pooled,
                                                            const float* __restrict__ ca, const float* __restrict__ w1,
                                                            const float* __restrict__ w2, int C, int Hd, float* __restrict__ dz,
                                                            float* __restrict__ hsum, float* __restrict__ dpre, float* __restrict__ dpool) {
    extern __shared__ float sh[];  // [2C] pooled | [C] dz | [2Hd] pre (avg,max) | [Hd] dh
    float* sp = sh;
    float* sdz = sh + 2 * C;
    float* pre = sdz + C;
    float* dh = pre + 2 * Hd;
    const int n = blockIdx.x, nt = blockDim.x, nw = nt >> 6;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    stage_pooled(pooled, n, C, sp);
    for (int c = threadIdx.x; c < C; c += nt) {
        float s = 0.f;
#pragma unroll 8
        for (int b = 0; b < PB; ++b) s += dcap[((int64_t)n * PB + b) * C + c];
        const float a = ca[(int64_t)n * C + c];
        const float g = s * a * (1.f - a);
        sdz[c] = g;
        dz[(int64_t)n * C + c] = g;
    }
    __syncthreads();
    for (int h = wave; h < Hd; h += nw) {
        float a, m, g = 0.f;
        hidden_unit(w1, sp, C, h, lane, a, m, [&](int c) { g += w2[(int64_t)c * Hd + h] * sdz[c]; });
        g = wave_sum(g);
        if (lane == 0) {
            pre[h] = a; pre[Hd + h] = m; dh[h] = g;
            hsum[(int64_t)n * Hd + h] = relu_sum(a, m);
            dpre[((int64_t)n * 2 + 0) * Hd + h] = a > 0.f ? g : 0.f;
            dpre[((int64_t)n * 2 + 1) * Hd + h] = m > 0.f ? g : 0.f;
        }
    }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += nt) {
        float da = 0.f, dm = 0.f;
#pragma unroll 8
        for (int h = 0; h < Hd; ++h) {
            const float w = w1[(int64_t)h * C + c];
            da += (pre[h] > 0.f ? dh[h] : 0.f) * w;
            dm += (pre[Hd + h] > 0.f ? dh[h] : 0.f) * w;
        }
        dpool[((int64_t)n * 2 + 0) * C + c] = da;
        dpool[((int64_t)n * 2 + 1) * C + c] = dm;
    }
}

// B4: weight gradients (sum over images, fixed order): dw2[c][h] = sum_n dz[n,c]*hsum[n,h];
//     dw1[h][c] = sum_n dpre[n,0,h]*avg[n,c] + dpre[n,1,h]*max[n,c]
__global__ void cbam_bwd_w_kernel(const float* __restrict__ dz, const float* __restrict__ hsum, const float* __restrict__ dpre,
                                  const float* __restrict__ pooled, int N, int C, int Hd, float* __restrict__ dw1, float* __restrict__ dw2) {
    const int total = C * Hd;
    for (int i2 = blockIdx.x * blockDim.x + threadIdx.x; i2 < 2 * total; i2 += gridDim.x * blockDim.x) {
        const int i = i2 < total ? i2 : i2 - total;
        if (i2 < total) {
            const int c = i / Hd, h = i % Hd;  // dw2 [C][Hd]
            float s = 0.f;
#pragma unroll 8
            for (int n = 0; n < N; ++n) s += dz[(int64_t)n * C + c] * hsum[(int64_t)n * Hd + h];
            dw2[i] = s;
        } else {
            const int h = i / C, c = i % C;  // dw1 [Hd][C]
            float s = 0.f;
#pragma unroll 8
            for (int n = 0; n < N; ++n)
                s += dpre[((int64_t)n * 2 + 0) * Hd + h] * pooled[((int64_t)n * 2 + 0) * C + c] +
                     dpre[((int64_t)n * 2 + 1) * Hd + h] * pooled[((int64_t)n * 2 + 1) * C + c];
            dw1[i] = s;
        }
    }
}

// B5: dwsa[j][t] = sum_{n,p} du[p] * sm[p + off_t][j]   (one block per (j,t))
__global__ __launch_bounds__(1024) void cbam_bwd_wsa_kernel(const float* __restrict__ du, const float* __restrict__ smap, int N, int H, int W, int K,
                                                            float* __restrict__ dwsa) {
    __shared__ float red[16];
    const int t = blockIdx.x % (K * K), j = blockIdx.x / (K * K);
    const int R = K / 2, dy = t / K - R, dx = t % K - R;
    const uint32_t NP = (uint32_t)N * H * W, uw = (uint32_t)W, uh = (uint32_t)H;  // host: N*H*W < 2^31
    const int shift = dy * W + dx;
    float s0 = 0.f, s1 = 0.f;  // two chains: even / odd trips (fixed order: deterministic)
    uint32_t p = threadIdx.x;
    for (; p + blockDim.x < NP; p += 2 * blockDim.x) {
        const uint32_t q = p + blockDim.x;
        const uint32_t r0 = p / uw, r1 = q / uw;
        const int w0 = (int)(p - r0 * uw), h0 = (int)(r0 % uh), w1 = (int)(q - r1 * uw), h1 = (int)(r1 % uh);
        const float a0 = in_map(h0 + dy, w0 + dx, H, W) ? du[p] * smap[((int64_t)p + shift) * 2 + j] : 0.f;
        const float a1 = in_map(h1 + dy, w1 + dx, H, W) ? du[q] * smap[((int64_t)q + shift) * 2 + j] : 0.f;
        s0 += a0;
        s1 += a1;
    }
    if (p < NP) {
        const uint32_t r0 = p / uw;
        const int w0 = (int)(p - r0 * uw), h0 = (int)(r0 % uh);
        if (in_map(h0 + dy, w0 + dx, H, W)) s0 += du[p] * smap[((int64_t)p + shift) * 2 + j];
    }
    float s = wave_sum(s0 + s1);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        float tot = 0.f;
        for (int q = 0; q < (int)(blockDim.x >> 6); ++q) tot += red[q];
        dwsa[blockIdx.x] = tot;
    }
}

// B6: dx[p,c] += d_avg[c]/HW + [p == argmax_p(c)] * d_max[c]
template <typename T>
__global__ void cbam_bwd_pool_kernel(CV dx, int64_t NP, int HW, int C, const float* __restrict__ dpool, const int* __restrict__ amax) {
    const uint32_t groups = (uint32_t)(C / 4), total = (uint32_t)NP * groups, uhw = (uint32_t)HW;  // host: NP * C / 4 < 2^31
    const float inv = 1.f / (float)HW;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        const uint32_t p = i / groups, g = i - p * groups;
        const uint32_t n = p / uhw, q = p - n * uhw;
        T* dp = row<T>(dx, p) + g * 4;
        float v[4];
        Pack<T, 4>::load(dp, v);
        const float4 da = *reinterpret_cast<const float4*>(dpool + ((int64_t)n * 2 + 0) * C + g * 4);
        const float4 dm = *reinterpret_cast<const float4*>(dpool + ((int64_t)n * 2 + 1) * C + g * 4);
        const int4 am = *reinterpret_cast<const int4*>(amax + (int64_t)n * C + g * 4);
        v[0] += da.x * inv + (am.x == (int)q ? dm.x : 0.f);
        v[1] += da.y * inv + (am.y == (int)q ? dm.y : 0.f);
        v[2] += da.z * inv + (am.z == (int)q ? dm.z : 0.f);
        v[3] += da.w * inv + (am.w == (int)q ? dm.w : 0.f);
        Pack<T, 4>::store(dp, v);
    }
}

static int cbam_pb(int HW) {
    int pb = (HW + 31) / 32;  // >= 8 pixels per wave
    if (pb > 64) pb = 64;
    if (pb < 1) pb = 1;
    return pb;
}

// ONE statement of the backward's workspace: du [N*H*W] | dcap [N][PB][C] | dz [N][C] | hsum [N][Hd] | dpre [N][2][Hd] | dpool [N][2][C], each
// sub-buffer on a 16-byte boundary of a 16-byte aligned base (float4 reads of dpool); `floats` counts what the six hold, without the rounding
struct CbamWork {
    float *du, *dcap, *dz, *hsum, *dpre, *dpool;
    int64_t floats;
};
static CbamWork cbam_carve(float* base, int64_t N, int64_t H, int64_t W, int64_t C, int64_t Hd) {
    const int64_t PB = cbam_pb((int)(H * W));
    int64_t off = 0, floats = 0;
    auto take = [&](int64_t cnt) {
        float* p = base ? base + off : nullptr;
        off += (cnt + 3) / 4 * 4;
        floats += cnt;
        return p;
    };
    return CbamWork{take(N * H * W), take(N * PB * C), take(N * C), take(N * Hd), take(2 * N * Hd), take(2 * N * C), floats};  // (braces: left to right)
}
// the carve of a null base, 4 floats of slack for each of the six roundings, 256 bytes for the caller's base alignment
extern "C" size_t ymi_cbam_bwd_workspace(int64_t n, int64_t h, int64_t w, int64_t c, int64_t hidden) {
    return (size_t)(cbam_carve(nullptr, n, h, w, c, hidden).floats + 6 * 4) * sizeof(float) + 256;
}

extern "C" int ymi_cbam_bwd(const ymi_tensor* x, const ymi_tensor* dout, const float* w1, const float* w2, int64_t hidden, const float* wsa,
                            int64_t ksa, const float* ca, const float* pooled, const int32_t* pool_argmax, const float* smap,
                            const int32_t* smap_argmax, const float* sa, const ymi_tensor* dx, float* dw1, float* dw2, float* dwsa,
                            void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = cbam_check("cbam_bwd", {x, dout, dx}, hidden, ksa)) return rc;
    YMI_CHECK_ARG(x->c <= 1024, "cbam_bwd: at most 1024 channels");
    YMI_CHECK_ARG(w1 && w2 && wsa && ca && pooled && pool_argmax && smap && smap_argmax && sa && dw1 && dw2 && dwsa && workspace, "cbam_bwd: null buffer");
    const int N = (int)x->n, H = (int)x->h, W = (int)x->w, C = (int)x->c, HW = H * W, Hd = (int)hidden, K = (int)ksa;
    const size_t need = ymi_cbam_bwd_workspace(N, H, W, C, Hd);
    if (workspace_bytes < need) {
        ymi_set_error("cbam_bwd: workspace %zu < %zu", workspace_bytes, need);
        return YMI_EWORKSPACE;
    }
    const int PB = cbam_pb(HW);
    const int64_t NP = (int64_t)N * HW;
    YMI_CHECK_ARG(NP * (C / 4) < ((int64_t)1 << 31), "cbam_bwd: N*H*W*C/4 must stay below 2^31");
    YMI_CHECK_ARG(((uintptr_t)workspace & 15) == 0, "cbam_bwd: workspace must be 16-byte aligned");
    const CbamWork k = cbam_carve(reinterpret_cast<float*>(workspace), N, H, W, C, Hd);
    hipStream_t s = (hipStream_t)stream;
    CV xv{x->data, x->ld}, dv{dout->data, dout->ld}, ov{dx->data, dx->ld};
    dim3 gw((unsigned)((NP + 3) / 4));
    const size_t lds3 = (size_t)(3 * C + 3 * Hd) * sizeof(float);
    int64_t ge = (NP * (C / 4) + 255) / 256;
    if (ge > 4096) ge = 4096;
    dispatch_dtype(x->dtype, [&](auto t) {
        typedef typename decltype(t)::type T;
        launch(cbam_bwd_du_kernel<T>, gw, dim3(256), 0, s, xv, dv, NP, HW, C, ca, sa, k.du);
        launch(cbam_bwd_dx_kernel<T>, dim3(N * PB), dim3(256), 0, s, xv, dv, ov, N, H, W, C, ca, sa, k.du, smap_argmax, wsa, K, k.dcap, PB);
        launch(cbam_bwd_mlp_kernel, dim3(N), dim3(1024), lds3, s, k.dcap, PB, pooled, ca, w1, w2, C, Hd, k.dz, k.hsum, k.dpre, k.dpool);
        launch(cbam_bwd_w_kernel, dim3((2 * C * Hd + 255) / 256), dim3(256), 0, s, k.dz, k.hsum, k.dpre, pooled, N, C, Hd, dw1, dw2);
        launch(cbam_bwd_wsa_kernel, dim3(2 * K * K), dim3(1024), 0, s, k.du, smap, N, H, W, K, dwsa);
        launch(cbam_bwd_pool_kernel<T>, dim3((unsigned)ge), dim3(256), 0, s, ov, NP, HW, C, k.dpool, pool_argmax);
    });
    YMI_CHECK_LAUNCH("cbam_bwd");
    return YMI_OK;
}
