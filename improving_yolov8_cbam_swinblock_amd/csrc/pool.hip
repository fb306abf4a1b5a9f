// SPPF max-pool cascade (k x k, stride 1, pad k/2 with -inf, three times chained) for NHWC tensors.
//
// Two primitives, each written once: window_max() (maximum of the k positions around an LDS item along one axis) and
// window_first_max() (the same with the offset of the FIRST maximum: PyTorch's tie rule).  Every pool is separable, a row pass
// followed by a column pass, so the four forward passes are calls of the first and the four arg-max passes calls of the second.
//
// Forward, sppf_pool3_kernel<T, NCH, K>: one launch produces y1, y2, y3 from y0.  A workgroup owns a spatial tile x NCH 16-byte
// channel chunks, stages the tile plus a 3*(k/2) halo (clamped to the image) in LDS once and runs the three pools between two
// LDS images, so y0 is read from HBM once and y1..y3 are written once (the algorithmic minimum: 1 read + 3 writes).  Positions
// outside the image are -inf for every stage, which reproduces the chained semantics of nn.MaxPool2d exactly (max is exact in
// any precision -> bit-identical to the f32 reference).  Two forms are launched: the MAP form <T, 1, 5 | 7 | 0> where the whole
// map of one chunk fits LDS (tile = image, no halo, up to 1024 threads; the model's 20x20 - 40x40 maps) and the TILED form
// <T, 4, 0> (64-byte slabs, 256 threads) beyond.
//
// Backward: per stage, g_in[s] += sum over p in window(s) of [argmax_window(p) == s] * g_out[p], as a GATHER (deterministic),
// with the arg-max of every window recomputed in LDS: sppf_bwd_map_kernel<T, K> (whole map, the three stages in one launch) and
// maxpool_bwd_kernel<T> (tiled, one stage per launch).
#include "common.h"

struct PV {
    void* p;
    int64_t ld;
};
static PV pv(const ymi_tensor* t) { return PV{t->data, t->ld}; }

// 16-byte chunk as floats
template <typename T> struct Chunk;
template <> struct Chunk<bf16_t> {
    static constexpr int N = 8;
    static __device__ __forceinline__ void load(const void* p, float (&v)[8]) { Pack<bf16_t, 8>::load(reinterpret_cast<const bf16_t*>(p), v); }
    static __device__ __forceinline__ void store(void* p, const float (&v)[8]) { Pack<bf16_t, 8>::store(reinterpret_cast<bf16_t*>(p), v); }
};
template <> struct Chunk<float> {
    static constexpr int N = 4;
    static __device__ __forceinline__ void load(const void* p, float (&v)[4]) { Pack<float, 4>::load(reinterpret_cast<const float*>(p), v); }
    static __device__ __forceinline__ void store(void* p, const float (&v)[4]) { Pack<float, 4>::store(reinterpret_cast<float*>(p), v); }
};

#define NEG_INF (-__builtin_inff())

// ---- the two window scans.  `base` is an LDS image of 16-byte items, `i` the centre item, `stride` the distance in items between
// neighbours along the scanned axis, `pos` the centre's coordinate on that axis and `extent` the axis length; K is the compiled
// window size (0: the run-time k).  Compiled K: the loop is unrolled over all K positions and one outside [0, extent) reads the
// centre instead of being branched around, so the LDS reads of one item are issued together.  Run-time k: the loop is not unrolled
// and visits the in-range positions only (the address select ahead of every read costs such a loop 13 % of the tiled forward).
template <int K> __device__ __forceinline__ int window_begin(int pos, int r) { return K ? 0 : max(r - pos, 0); }
template <int K> __device__ __forceinline__ int window_end(int pos, int r, int extent, int k) { return K ? K : min(k, extent + r - pos); }

// m = maximum over the window (the centre read again leaves a maximum unchanged)
template <typename T, int K>
__device__ __forceinline__ void window_max(const char* base, int i, int stride, int pos, int extent, int k, float (&m)[Chunk<T>::N]) {
    constexpr int CN = Chunk<T>::N, UN = K ? K : 1;
    const int r = k / 2;
#pragma unroll
    for (int e = 0; e < CN; ++e) m[e] = NEG_INF;
#pragma unroll UN
    for (int d = window_begin<K>(pos, r); d < window_end<K>(pos, r, extent, k); ++d) {
        const int q = pos - r + d;
        const bool ok = !K || (q >= 0 && q < extent);
        float v[CN];
        Chunk<T>::load(base + (size_t)(ok ? i + (d - r) * stride : i) * 16, v);
#pragma unroll
        for (int e = 0; e < CN; ++e) m[e] = fmaxf(m[e], v[e]);
    }
}

// best = maximum over the window, code = offset d (0..k-1, centre = k/2) of its FIRST occurrence.  This is the one statement of
// the tie rule that makes gradients route like nn.MaxPool2d: the first in-range element initialises, then strictly greater wins.
// Applied along rows and then along columns of the row maxima it selects the first maximum of the k x k window in row-major order.
// (Run-time k: `ok` is the constant true, and it is the loop bounds that keep every visited position in range.)
template <typename T, int K>
__device__ __forceinline__ void window_first_max(const char* base, int i, int stride, int pos, int extent, int k, float (&best)[Chunk<T>::N],
                                                 int (&code)[Chunk<T>::N]) {
    constexpr int CN = Chunk<T>::N, UN = K ? K : 1;
    const int r = k / 2;
    float b[CN];  // (locals, copied out below: updated through the references the compare compiles to branches instead of selects)
    int c[CN];
#pragma unroll
    for (int e = 0; e < CN; ++e) { b[e] = NEG_INF; c[e] = -1; }
#pragma unroll UN
    for (int d = window_begin<K>(pos, r); d < window_end<K>(pos, r, extent, k); ++d) {
        const int q = pos - r + d;
        const bool ok = !K || (q >= 0 && q < extent);
        float v[CN];
        Chunk<T>::load(base + (size_t)(ok ? i + (d - r) * stride : i) * 16, v);
#pragma unroll
        for (int e = 0; e < CN; ++e)
            if (ok && (c[e] < 0 || v[e] > b[e])) {
                b[e] = v[e];
                c[e] = d;
            }
    }
#pragma unroll
    for (int e = 0; e < CN; ++e) { best[e] = b[e]; code[e] = c[e]; }
}

// ----------------------------------------------------------------------------------------- forward
struct PoolArgs {
    PV y[4];  // y0 (in), y1..y3 (out)
    int N, H, W, C;
    int k, TH, TW;  // TH x TW: the tile (tiled form; the map form's tile is the image)
};

// LDS of one forward workgroup: two images of the staged region (tile + 6r, clamped to the image; the map form: the image)
static size_t sppf_fwd_lds(int H, int W, int r, int th, int tw, int nch) {
    const int RH = (th + 6 * r < H) ? th + 6 * r : H, RW = (tw + 6 * r < W) ? tw + 6 * r : W;
    return (size_t)RH * RW * nch * 16 * 2;
}

// grid: map form (chunks, images), tiled form (tiles, slabs, images); work units run chunk / slab fastest, then tile, then image
// through xcd_unit(), so the workgroups that share a 128-byte line run on one XCD
template <typename T, int NCH, int K>
__global__ __launch_bounds__(NCH == 1 ? 1024 : 256) void sppf_pool3_kernel(PoolArgs a) {
    constexpr int CN = Chunk<T>::N;
    constexpr bool MAP = NCH == 1;  // launched with tile = image: one tile, no halo, C / CN chunks exactly, every staged item is emitted
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int k = K ? K : a.k, r = k / 2, halo = MAP ? 0 : 3 * r;
    const int TH = MAP ? a.H : a.TH, TW = MAP ? a.W : a.TW;
    const int slabs = MAP ? gridDim.x : gridDim.y, tiles = MAP ? 1 : gridDim.x, tiles_w = (a.W + TW - 1) / TW;
    const int unit = xcd_unit(flat_block_id(), gridDim.x * gridDim.y * gridDim.z);
    const int btile = (unit / slabs) % tiles, n = unit / (slabs * tiles);
    const int c0 = (unit % slabs) * NCH * CN;
    const int th0 = (btile / tiles_w) * TH, tw0 = (btile % tiles_w) * TW;
    const int th1 = min(th0 + TH, a.H), tw1 = min(tw0 + TW, a.W);
    // staged region = tile + 3r halo, clamped to the image
    const int rh0 = max(th0 - halo, 0), rh1 = min(th1 + halo, a.H);
    const int rw0 = max(tw0 - halo, 0), rw1 = min(tw1 + halo, a.W);
    const int RH = rh1 - rh0, RW = rw1 - rw0;
    const int items = RH * RW * NCH;  // (pixel, 16-byte chunk)
    char* A = smem;                            // [RH][RW][NCH][16 B] input of the current stage
    char* B = smem + (size_t)items * 16;       // [RH][RW][NCH][16 B] row maxima
    const int64_t img = (int64_t)n * a.H * a.W;
    const int org = rh0 * a.W + rw0, skip = a.W - RW;  // region pixel px is image pixel org + px + (px / RW) * skip (map form: px)

    const T* src = reinterpret_cast<const T*>(a.y[0].p);
    for (int i = threadIdx.x; i < items; i += blockDim.x) {
        const int ch = i % NCH, px = i / NCH;
        if (MAP || c0 + ch * CN < a.C) {
            *reinterpret_cast<uint4*>(A + (size_t)i * 16) = *reinterpret_cast<const uint4*>(src + (img + org + px + px / RW * skip) * a.y[0].ld + c0 + ch * CN);
        } else {  // the last slab overhangs C
            float v[CN];
#pragma unroll
            for (int e = 0; e < CN; ++e) v[e] = NEG_INF;
            Chunk<T>::store(A + (size_t)i * 16, v);
        }
    }
    __syncthreads();
#pragma unroll 1
    for (int st = 1; st <= 3; ++st) {
        // row max: B[h][w] = max_{|dx|<=r, inside the region} A[h][w+dx]
        for (int i = threadIdx.x; i < items; i += blockDim.x) {
            float m[CN];
            window_max<T, K>(A, i, NCH, (i / NCH) % RW, RW, k, m);
            Chunk<T>::store(B + (size_t)i * 16, m);
        }
        __syncthreads();
        // column max: A[h][w] = max_{|dy|<=r} B[h+dy][w] (A is only read by the row pass: free since the barrier above); emit the tile
        T* dst = reinterpret_cast<T*>(a.y[st].p);
        for (int i = threadIdx.x; i < items; i += blockDim.x) {
            const int ch = i % NCH, px = i / NCH;
            const int hh = px / RW, h = rh0 + hh, w = rw0 + px % RW;
            float m[CN];
            window_max<T, K>(B, i, RW * NCH, hh, RH, k, m);
            Chunk<T>::store(A + (size_t)i * 16, m);
            if (MAP || (h >= th0 && h < th1 && w >= tw0 && w < tw1 && c0 + ch * CN < a.C))
                Chunk<T>::store(dst + (img + org + px + hh * skip) * a.y[st].ld + c0 + ch * CN, m);
        }
        __syncthreads();
    }
    // Note on halo validity: a value of stage s at region position q is exact when q is at least
    // s*r inside the clamped region edge OR that edge is the image border; the tile interior is 3r
    // inside every non-border edge, so all three emitted stages are exact.
}

// ---------------------------------------------------------------------------------------- backward
// Two bodies over window_first_max(), on purpose: their gathers are different arithmetic.  The tiled kernel sums the k x k window
// in row-major order and stores the running gradient in the tensor dtype between its three launches; the map kernel gathers
// separably, column first, and keeps the running gradient in float32.  Merging them would change low bits of bf16 gradients.
struct PoolBwdArgs {
    PV x, gout, gsrc, gin;  // gin = gsrc + route(gout | x)
    int N, H, W, C;
    int k, TH, TW;
};

// CN one-byte arg-max codes of a 16-byte channel chunk, packed: one 8-byte (bf16) / 4-byte (f32) LDS access
template <int CN> __device__ __forceinline__ void store_codes(unsigned char* p, const int (&code)[CN]) {
    uint64_t v = 0;
#pragma unroll
    for (int e = 0; e < CN; ++e) v |= (uint64_t)(code[e] & 255) << (8 * e);
    if (CN == 8) *reinterpret_cast<uint64_t*>(p) = v;
    else *reinterpret_cast<uint32_t*>(p) = (uint32_t)v;
}
template <int CN> __device__ __forceinline__ uint64_t load_codes(const unsigned char* p) {
    return CN == 8 ? *reinterpret_cast<const uint64_t*>(p) : (uint64_t)*reinterpret_cast<const uint32_t*>(p);
}

// LDS of one tiled backward workgroup: x on tile + 4r, gout and the arg-max codes on tile + 2r, row maxima and their column codes
// on (tile + 4r) x (tile + 2r), every extent clamped to the image; 64 value bytes and 4 * cn code bytes per pixel
static size_t maxpool_bwd_lds(int H, int W, int r, int th, int tw, int cn) {
    const int XH = (th + 4 * r < H) ? th + 4 * r : H, XW = (tw + 4 * r < W) ? tw + 4 * r : W;
    const int GH = (th + 2 * r < H) ? th + 2 * r : H, GW = (tw + 2 * r < W) ? tw + 2 * r : W;
    return (size_t)XH * XW * 64 + (size_t)GH * GW * (64 + 4 * cn) + (size_t)XH * GW * (64 + 4 * cn);
}

// one stage (maps too large for the whole-map kernel below): gin[s] = gsrc[s] + sum_{p in window(s)} [argmax(x, window(p)) == s] gout[p]
// for a tile x a 64-byte channel slab.  The arg-max is separable: first the row maximum (and its column code) over the k columns, then
// the first row whose row maximum is the window maximum: 2k LDS reads per window instead of k*k, and the same element as a row-major
// scan.  (A window position is in the image exactly when it is in the staged region: the x region reaches r beyond the gout region.)
template <typename T>
__global__ __launch_bounds__(256) void maxpool_bwd_kernel(PoolBwdArgs a) {
    constexpr int CN = Chunk<T>::N, NCH = 4, CS = CN * NCH;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int r = a.k / 2, k = a.k;
    const int tiles_w = (a.W + a.TW - 1) / a.TW;
    // unit order: channel slab fastest, then tile, then image; consecutive units on one XCD (neighbouring slabs share 128-byte lines)
    const int unit = xcd_unit(flat_block_id(), gridDim.x * gridDim.y * gridDim.z);
    const int bslab = unit % gridDim.y, btile = (unit / gridDim.y) % gridDim.x;
    const int th0 = (btile / tiles_w) * a.TH, tw0 = (btile % tiles_w) * a.TW;
    const int th1 = min(th0 + a.TH, a.H), tw1 = min(tw0 + a.TW, a.W);
    const int c0 = bslab * CS, n = unit / (gridDim.x * gridDim.y);
    // x on tile + 2r, gout / argmax on tile + r (both clamped to the image)
    const int xh0 = max(th0 - 2 * r, 0), xh1 = min(th1 + 2 * r, a.H), xw0 = max(tw0 - 2 * r, 0), xw1 = min(tw1 + 2 * r, a.W);
    const int gh0 = max(th0 - r, 0), gh1 = min(th1 + r, a.H), gw0 = max(tw0 - r, 0), gw1 = min(tw1 + r, a.W);
    const int XH = xh1 - xh0, XW = xw1 - xw0, GH = gh1 - gh0, GW = gw1 - gw0;
    char* X = smem;                                          // [XH][XW][NCH * 16 B]
    char* G = X + (size_t)XH * XW * NCH * 16;                // [GH][GW][NCH * 16 B]
    char* RM = G + (size_t)GH * GW * NCH * 16;               // [XH][GW][NCH * 16 B] row maxima
    unsigned char* IDX = reinterpret_cast<unsigned char*>(RM + (size_t)XH * GW * NCH * 16);  // [GH][GW][CS]
    unsigned char* RC = IDX + (size_t)GH * GW * CS;          // [XH][GW][CS] column code of the row maximum

    const T* xs = reinterpret_cast<const T*>(a.x.p);
    const T* gs = reinterpret_cast<const T*>(a.gout.p);
    for (int i = threadIdx.x; i < XH * XW * NCH; i += 256) {
        const int ch = i % NCH, px = i / NCH;
        const int h = xh0 + px / XW, w = xw0 + px % XW;
        float v[CN];
        if (c0 + ch * CN < a.C) Chunk<T>::load(xs + (((int64_t)n * a.H + h) * a.W + w) * a.x.ld + c0 + ch * CN, v);
        else
#pragma unroll
            for (int e = 0; e < CN; ++e) v[e] = NEG_INF;
        Chunk<T>::store(X + (size_t)i * 16, v);
    }
    for (int i = threadIdx.x; i < GH * GW * NCH; i += 256) {
        const int ch = i % NCH, px = i / NCH;
        const int h = gh0 + px / GW, w = gw0 + px % GW;
        float v[CN];
        if (c0 + ch * CN < a.C) Chunk<T>::load(gs + (((int64_t)n * a.H + h) * a.W + w) * a.gout.ld + c0 + ch * CN, v);
        else
#pragma unroll
            for (int e = 0; e < CN; ++e) v[e] = 0.f;
        Chunk<T>::store(G + (size_t)i * 16, v);
    }
    __syncthreads();
    // row pass: for every staged row and every G column, the maximum over the k columns and its column code
    for (int i = threadIdx.x; i < XH * GW * NCH; i += 256) {
        const int ch = i % NCH, px = i / NCH;
        const int hh = px / GW, wx = gw0 + px % GW - xw0;  // row and column in the x region
        float best[CN];
        int code[CN];
        window_first_max<T, 0>(X, (hh * XW + wx) * NCH + ch, NCH, wx, XW, k, best, code);
        Chunk<T>::store(RM + (size_t)i * 16, best);
        store_codes<CN>(RC + (size_t)px * CS + ch * CN, code);
    }
    __syncthreads();
    // column pass: arg-max code (dy*k + dx) of every window centred in the G region
    for (int i = threadIdx.x; i < GH * GW * NCH; i += 256) {
        const int ch = i % NCH, px = i / NCH;
        const int hx = gh0 + px / GW - xh0, wl = px % GW;  // row in the x region (the row maxima's), column in the G region
        float best[CN];
        int code[CN];
        window_first_max<T, 0>(RM, (hx * GW + wl) * NCH + ch, GW * NCH, hx, XH, k, best, code);
#pragma unroll
        for (int e = 0; e < CN; ++e)  // code = dy: fold in the column code of that row's maximum
            code[e] = code[e] * k + RC[(size_t)((hx + code[e] - r) * GW + wl) * CS + ch * CN + e];
        store_codes<CN>(IDX + (size_t)px * CS + ch * CN, code);
    }
    __syncthreads();
    T* gi = reinterpret_cast<T*>(a.gin.p);
    const int TH = th1 - th0, TW = tw1 - tw0;
    for (int i = threadIdx.x; i < TH * TW * NCH; i += 256) {
        const int ch = i % NCH, px = i / NCH;
        const int h = th0 + px / TW, w = tw0 + px % TW;
        if (c0 + ch * CN >= a.C) continue;
        float acc[CN];
        T* dst = gi + (((int64_t)n * a.H + h) * a.W + w) * a.gin.ld + c0 + ch * CN;
        Chunk<T>::load(reinterpret_cast<const T*>(a.gsrc.p) + (((int64_t)n * a.H + h) * a.W + w) * a.gsrc.ld + c0 + ch * CN, acc);
        for (int ay = -r; ay <= r; ++ay) {
            const int ph = h + ay;
            if (ph < 0 || ph >= a.H) continue;
            for (int ax = -r; ax <= r; ++ax) {
                const int pw = w + ax;
                if (pw < 0 || pw >= a.W) continue;
                const int want = (r - ay) * k + (r - ax);
                const size_t gp = (size_t)(ph - gh0) * GW + (pw - gw0);
                float g[CN];
                Chunk<T>::load(G + (gp * NCH + ch) * 16, g);
                const uint64_t ix = load_codes<CN>(IDX + gp * CS + ch * CN);  // one LDS access for the CN arg-max codes
#pragma unroll
                for (int e = 0; e < CN; ++e)
                    if ((int)((ix >> (8 * e)) & 255) == want) acc[e] += g[e];
            }
        }
        Chunk<T>::store(dst, acc);
    }
}

// ---- whole-map backward: a workgroup owns ONE image x ONE 16-byte channel chunk and keeps the whole map in LDS, as the forward's map
// form does (grid (chunks, images), units chunk-fastest through xcd_unit(), window loops unrolled for K = 5, 7).
struct MapBwdArgs {
    PV y[3];    // y0, y1, y2
    PV dy[4];   // dy0..dy3 (in)
    PV dx;      // out
    int N, H, W, C, k;
};

template <typename T> __device__ __forceinline__ void lds_load_f32(const float* base, int planes_stride, int i, float (&v)[Chunk<T>::N]) {
    // f32 images are kept as planes of 4 floats per pixel (16-byte LDS accesses at unit stride across lanes: conflict-free)
#pragma unroll
    for (int q = 0; q < Chunk<T>::N / 4; ++q) {
        const float4 t = *reinterpret_cast<const float4*>(base + (size_t)q * planes_stride + (size_t)i * 4);
        v[q * 4 + 0] = t.x; v[q * 4 + 1] = t.y; v[q * 4 + 2] = t.z; v[q * 4 + 3] = t.w;
    }
}
template <typename T> __device__ __forceinline__ void lds_store_f32(float* base, int planes_stride, int i, const float (&v)[Chunk<T>::N]) {
#pragma unroll
    for (int q = 0; q < Chunk<T>::N / 4; ++q)
        *reinterpret_cast<float4*>(base + (size_t)q * planes_stride + (size_t)i * 4) = make_float4(v[q * 4 + 0], v[q * 4 + 1], v[q * 4 + 2], v[q * 4 + 3]);
}

// Backward of the cascade in one launch:  g := dy3;  g := dy2 + route(g | y2);  g := dy1 + route(g | y1);  dx = dy0 + route(g | y0),
// the running gradient in f32 in LDS.  route() is a deterministic gather with PyTorch's arg-max rule (first maximum in row-major
// order), and it is SEPARABLE: the arg-max of window p is (first row whose row maximum is the window maximum, that row's first
// maximal column), so  V[hh][w] = sum_{ph} [rowcode(ph, w) -> hh] g[ph][w]  followed by  out[hh][ww] = sum_{pw} [colcode(hh, pw) -> ww]
// V[hh][pw]  visits 2k positions per pixel instead of k*k (the sums associate column-first: exact for the dyadic tie fixtures,
// within f32 rounding of the row-major order otherwise).
template <typename T, int K>
__global__ __launch_bounds__(1024) void sppf_bwd_map_kernel(MapBwdArgs a) {
    constexpr int CN = Chunk<T>::N;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int UN = K ? K : 1;  // unroll count of the window loops (runtime k: not unrolled)
    const int HW = a.H * a.W, k = K ? K : a.k, r = k / 2;
    const int unit = xcd_unit(flat_block_id(), gridDim.x * gridDim.y);
    const int c0 = (unit % gridDim.x) * CN, n = unit / gridDim.x;
    const int PS = HW * 4;                                            // floats per f32 plane
    float* G = reinterpret_cast<float*>(smem);                        // [CN/4][HW][4] running gradient
    char* X = reinterpret_cast<char*>(G + (size_t)HW * CN);           // [HW][16 B] values of the current stage   } later V: [CN/4][HW][4] f32
    char* RM = X + (size_t)HW * 16;                                   // [HW][16 B] row maxima (f32 tensors: V needs X only) }
    float* V = reinterpret_cast<float*>(X);
    unsigned char* RC = reinterpret_cast<unsigned char*>(X + (size_t)HW * 32);  // [HW][CN] column code of the row maximum
    unsigned char* RR = RC + (size_t)HW * CN;                         // [HW][CN] row code of the window maximum
    const int64_t img = (int64_t)n * HW;
    {
        const T* gp = reinterpret_cast<const T*>(a.dy[3].p);
        for (int i = threadIdx.x; i < HW; i += blockDim.x) {
            float v[CN];
            Chunk<T>::load(gp + (img + i) * a.dy[3].ld + c0, v);
            lds_store_f32<T>(G, PS, i, v);
        }
    }
#pragma unroll 1
    for (int st = 2; st >= 0; --st) {
        const T* xp = reinterpret_cast<const T*>(a.y[st].p);
        for (int i = threadIdx.x; i < HW; i += blockDim.x) {
            float v[CN];
            Chunk<T>::load(xp + (img + i) * a.y[st].ld + c0, v);
            Chunk<T>::store(X + (size_t)i * 16, v);
        }
        __syncthreads();
        // row pass: maximum over the k columns around every position and the code (0..k-1) of its first occurrence
        for (int i = threadIdx.x; i < HW; i += blockDim.x) {
            float best[CN];
            int code[CN];
            window_first_max<T, K>(X, i, 1, i % a.W, a.W, k, best, code);
            Chunk<T>::store(RM + (size_t)i * 16, best);
            store_codes<CN>(RC + (size_t)i * CN, code);
        }
        __syncthreads();
        // column pass: code (0..k-1) of the first row whose row maximum is the maximum of the window centred here
        for (int i = threadIdx.x; i < HW; i += blockDim.x) {
            float best[CN];
            int code[CN];
            window_first_max<T, K>(RM, i, a.W, i / a.W, a.H, k, best, code);
            store_codes<CN>(RR + (size_t)i * CN, code);
        }
        __syncthreads();  // X and RM are dead from here: V takes their place
        // vertical gather: V[hh][w] = sum over window centres (ph, w), ph = hh - r + d, whose maximal row is hh (row code 2r - d)
        for (int i = threadIdx.x; i < HW; i += blockDim.x) {
            const int h = i / a.W;
            float acc[CN];
#pragma unroll
            for (int e = 0; e < CN; ++e) acc[e] = 0.f;
#pragma unroll UN
            for (int d = 0; d < k; ++d) {
                const int ph = h - r + d;
                const bool ok = ph >= 0 && ph < a.H;
                const int j = ok ? i + (d - r) * a.W : i;
                const int want = ok ? 2 * r - d : 255;
                float g[CN];
                lds_load_f32<T>(G, PS, j, g);
                const uint64_t rc = load_codes<CN>(RR + (size_t)j * CN);
#pragma unroll
                for (int e = 0; e < CN; ++e)
                    if ((int)((rc >> (8 * e)) & 255) == want) acc[e] += g[e];
            }
            lds_store_f32<T>(V, PS, i, acc);
        }
        __syncthreads();  // G is dead from here: the next running gradient is written over it
        // horizontal gather: out[hh][ww] = dy_st[hh][ww] + sum over pw = ww - r + d with column code 2r - d in row hh of V[hh][pw]
        const T* dp = reinterpret_cast<const T*>(a.dy[st].p);
        T* op = reinterpret_cast<T*>(a.dx.p);
        for (int i = threadIdx.x; i < HW; i += blockDim.x) {
            const int h = i / a.W, w = i - h * a.W;
            float acc[CN];
            Chunk<T>::load(dp + (img + i) * a.dy[st].ld + c0, acc);
#pragma unroll UN
            for (int d = 0; d < k; ++d) {
                const int pw = w - r + d;
                const bool ok = pw >= 0 && pw < a.W;
                const int j = ok ? i - r + d : i;
                const int want = ok ? 2 * r - d : 255;
                float g[CN];
                lds_load_f32<T>(V, PS, j, g);
                const uint64_t rc = load_codes<CN>(RC + (size_t)j * CN);
#pragma unroll
                for (int e = 0; e < CN; ++e)
                    if ((int)((rc >> (8 * e)) & 255) == want) acc[e] += g[e];
            }
            if (st == 0) Chunk<T>::store(op + (img + i) * a.dx.ld + c0, acc);
            else lds_store_f32<T>(G, PS, i, acc);
        }
        __syncthreads();  // V (= X, RM), RC, RR free for the next stage; G complete
    }
}

// LDS of the whole-map backward per pixel: G (4 CN) + X|RM / V (32 B >= 4 CN) + RC + RR (2 CN)
static size_t sppf_bwd_map_lds(int hw, int cn) { return (size_t)hw * (4 * cn + 32 + 2 * cn); }

// ------------------------------------------------------------------------------------------- host
static const size_t POOL_LDS_MAX = 150 * 1024;  // the map forms run where the whole map fits this; the tiled forms halve their tile until it does
static int sppf_map_threads(int hw) { const int t = (hw + 63) / 64 * 64; return t < 64 ? 64 : (t > 1024 ? 1024 : t); }
static int cdiv(int a, int b) { return (a + b - 1) / b; }

// tile of the tiled forms: the image, its longer side halved (down to 8) until bytes(th, tw) fits; false: it does not at 8 x 8
template <typename F> static bool pool_fit_tile(int H, int W, F bytes, int* th, int* tw) {
    *th = H; *tw = W;
    while (bytes(*th, *tw) > POOL_LDS_MAX) {
        if (*th >= *tw && *th > 8) *th = (*th + 1) / 2;
        else if (*tw > 8) *tw = (*tw + 1) / 2;
        else return false;
    }
    return true;
}

template <typename A> static void pool_launch(void (*kern)(A), dim3 grid, dim3 block, size_t lds, hipStream_t s, const A& a) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    hipLaunchKernelGGL(kern, grid, block, lds, s, a);
}

// f(Type<T>{}) for the tensor dtype (the tiled forms: they have the run-time k only); f(Form<T, K>{}) for the dtype and the compiled
// window size K of the map forms (5, 7; 0 for every other k: the run-time one)
template <typename T_> struct Type { using T = T_; };
template <typename T_, int K_> struct Form {
    using T = T_;
    static constexpr int K = K_;
};
template <typename F> static void pool_dispatch_dtype(int dtype, F f) {
    if (dtype == YMI_BF16) f(Type<bf16_t>{});
    else f(Type<float>{});
}
template <typename F> static void pool_dispatch(int dtype, int k, F f) {
    pool_dispatch_dtype(dtype, [&](auto t) {
        using T = typename decltype(t)::T;
        if (k == 5) f(Form<T, 5>{});
        else if (k == 7) f(Form<T, 7>{});
        else f(Form<T, 0>{});
    });
}

// every tensor valid, of y0's shape and dtype, with c, ld and the base on 16-byte boundaries; k odd, at most 13
static int pool_check_args(const char* who, std::initializer_list<const ymi_tensor*> ts, int64_t k) {
    const ymi_tensor* y0 = *ts.begin();
    const int cn = (y0 && y0->dtype == YMI_BF16) ? 8 : 4;
    for (auto t : ts) {
        YMI_CHECK_ARG(ymi_tensor_ok(t) && ymi_same_shape(t, y0) && t->dtype == y0->dtype, "%s: tensors must share shape and dtype", who);
        YMI_CHECK_ARG(t->c % cn == 0 && t->ld % cn == 0 && ((uintptr_t)t->data & 15) == 0, "%s: channels/ld/base must be 16-byte aligned", who);
    }
    YMI_CHECK_ARG(k >= 1 && (k & 1) && k <= 13, "%s: odd k <= 13", who);
    return YMI_OK;
}

static int launch_pool_bwd(const ymi_tensor* x, int k, PV gout, const ymi_tensor* gsrc, PV gin, hipStream_t stream) {
    PoolBwdArgs a{};
    a.x = pv(x); a.gout = gout; a.gsrc = pv(gsrc); a.gin = gin;
    a.N = (int)x->n; a.H = (int)x->h; a.W = (int)x->w; a.C = (int)x->c; a.k = k;
    const int cn = x->dtype == YMI_BF16 ? 8 : 4;
    auto bytes = [&](int th, int tw) { return maxpool_bwd_lds(a.H, a.W, k / 2, th, tw, cn); };
    YMI_CHECK_ARG(pool_fit_tile(a.H, a.W, bytes, &a.TH, &a.TW), "sppf_pool3_bwd: tile does not fit LDS");
    const dim3 grid(cdiv(a.H, a.TH) * cdiv(a.W, a.TW), cdiv(a.C, 4 * cn), a.N);
    pool_dispatch_dtype(x->dtype, [&](auto t) { pool_launch(maxpool_bwd_kernel<typename decltype(t)::T>, grid, dim3(256), bytes(a.TH, a.TW), stream, a); });
    YMI_CHECK_LAUNCH("sppf_pool3_bwd");
    return YMI_OK;
}

extern "C" int64_t ymi_sppf_pool3_bwd_workspace(int64_t n, int64_t h, int64_t w, int64_t c, int dtype) {
    if (sppf_bwd_map_lds((int)(h * w), dtype == YMI_BF16 ? 8 : 4) <= POOL_LDS_MAX) return 0;
    return 2 * n * h * w * c * (int64_t)ymi_esize(dtype);  // the two intermediate gradients of the per-stage path
}

// dx = dy0 + route(dy1 + route(dy2 + route(dy3 | y2) | y1) | y0); no input is modified.
extern "C" int ymi_sppf_pool3_bwd(const ymi_tensor* y0, const ymi_tensor* y1, const ymi_tensor* y2, int64_t k, const ymi_tensor* dy0,
                                  const ymi_tensor* dy1, const ymi_tensor* dy2, const ymi_tensor* dy3, const ymi_tensor* dx, void* workspace,
                                  int64_t workspace_bytes, void* stream) {
    if (int rc = pool_check_args("sppf_pool3_bwd", {y0, y1, y2, dy0, dy1, dy2, dy3, dx}, k)) return rc;
    hipStream_t s = (hipStream_t)stream;
    const int cn = y0->dtype == YMI_BF16 ? 8 : 4, hw = (int)(y0->h * y0->w);
    const size_t lds = sppf_bwd_map_lds(hw, cn);
    if (lds <= POOL_LDS_MAX) {
        MapBwdArgs a{{pv(y0), pv(y1), pv(y2)}, {pv(dy0), pv(dy1), pv(dy2), pv(dy3)}, pv(dx), (int)y0->n, (int)y0->h, (int)y0->w, (int)y0->c, (int)k};
        const dim3 grid((unsigned)(a.C / cn), (unsigned)a.N), block((unsigned)sppf_map_threads(hw));
        pool_dispatch(y0->dtype, a.k, [&](auto f) {
            using F = decltype(f);
            pool_launch(sppf_bwd_map_kernel<typename F::T, F::K>, grid, block, lds, s, a);
        });
        YMI_CHECK_LAUNCH("sppf_pool3_bwd(map)");
        return YMI_OK;
    }
    const int64_t one = y0->n * y0->h * y0->w * y0->c * (int64_t)ymi_esize(y0->dtype);
    YMI_CHECK_ARG(workspace && workspace_bytes >= 2 * one && ((uintptr_t)workspace & 15) == 0, "sppf_pool3_bwd: workspace (see ymi_sppf_pool3_bwd_workspace)");
    const PV g2{workspace, y0->c}, g1{(char*)workspace + one, y0->c};
    int rc = launch_pool_bwd(y2, (int)k, pv(dy3), dy2, g2, s);
    if (rc) return rc;
    rc = launch_pool_bwd(y1, (int)k, g2, dy1, g1, s);
    if (rc) return rc;
    return launch_pool_bwd(y0, (int)k, g1, dy0, pv(dx), s);
}

extern "C" int ymi_sppf_pool3_fwd(const ymi_tensor* y0, int64_t k, const ymi_tensor* y1, const ymi_tensor* y2, const ymi_tensor* y3, void* stream) {
    if (int rc = pool_check_args("sppf_pool3_fwd", {y0, y1, y2, y3}, k)) return rc;
    hipStream_t s = (hipStream_t)stream;
    PoolArgs a{{pv(y0), pv(y1), pv(y2), pv(y3)}, (int)y0->n, (int)y0->h, (int)y0->w, (int)y0->c, (int)k, (int)y0->h, (int)y0->w};
    const int cn = y0->dtype == YMI_BF16 ? 8 : 4, r = a.k / 2;
    const size_t map_lds = sppf_fwd_lds(a.H, a.W, r, a.H, a.W, 1);
    if (map_lds <= POOL_LDS_MAX) {  // whole map per (image, 16-byte chunk) workgroup
        const dim3 grid((unsigned)(a.C / cn), (unsigned)a.N), block((unsigned)sppf_map_threads(a.H * a.W));
        pool_dispatch(y0->dtype, a.k, [&](auto f) {
            using F = decltype(f);
            pool_launch(sppf_pool3_kernel<typename F::T, 1, F::K>, grid, block, map_lds, s, a);
        });
        YMI_CHECK_LAUNCH("sppf_pool3_fwd(map)");
        return YMI_OK;
    }
    auto bytes = [&](int th, int tw) { return sppf_fwd_lds(a.H, a.W, r, th, tw, 4); };
    YMI_CHECK_ARG(pool_fit_tile(a.H, a.W, bytes, &a.TH, &a.TW), "sppf_pool3_fwd: tile does not fit LDS");
    const dim3 grid(cdiv(a.H, a.TH) * cdiv(a.W, a.TW), cdiv(a.C, 4 * cn), a.N);
    pool_dispatch_dtype(y0->dtype, [&](auto t) { pool_launch(sppf_pool3_kernel<typename decltype(t)::T, 4, 0>, grid, dim3(256), bytes(a.TH, a.TW), s, a); });
    YMI_CHECK_LAUNCH("sppf_pool3_fwd");
    return YMI_OK;
}
