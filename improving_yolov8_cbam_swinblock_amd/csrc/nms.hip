// Detection post-processing on the device: non_max_suppression of the reference (utils/ops.py:181-332) on the decoded Detect output
// y [B][4+nc][A] (csrc/loss.hip infer_decode_kernel), as three launches of one workgroup per image, all with grids that depend on shapes only:
//   1. nms_select_kernel : candidates (score > conf) in (anchor, class) order -> one 64-bit key each, score bits high, ~index low; when
//                          more than max_nms exist, a 3-level radix select over the 31 score bits finds the score of rank max_nms first and
//                          only candidates at or above it are written (equal scores: lowest indices first), so the key buffer is max_nms long
//   2. nms_sort_kernel   : bitonic sort of the keys, descending: descending score, then ascending anchor, then ascending class
//   3. nms_scan_kernel   : greedy suppression in sorted order against the kept list in LDS; leaves when max_det are kept
// The kernels take the rows of y per image as an argument: 4 + nc, or 4 + nc + nm for Segment's output (ymi_detect_nms_seg), where only rows
// 4 .. 4 + nc are scores and the scan also writes the kept anchors' nm coefficient rows; no decision depends on nm.
// Integer LDS atomics (histogram counts) are the only atomics: every result is a function of the input alone, bit for bit.
// This file is compiled with -ffp-contract=off (Makefile): area_i + area_j - inter must round as three operations, as in
// torchvision's nms carried out in float32, and the class offset b + cls * max_wh as a product and a sum.  Division is the compiler's IEEE
// sequence.  The threshold is compared in float32 (torchvision's GPU kernel; its CPU kernel compares against a double).
#include "common.h"

namespace {

constexpr int NMS_THREADS = 1024;    // select / sort
constexpr int NMS_WAVES = NMS_THREADS / YMI_WAVE;
constexpr int SELECT_BINS = 2048;    // histogram bins of one radix-select level: the 31 score bits are taken as 11 + 11 + 9
static_assert(SELECT_BINS == 2 * NMS_THREADS, "select_digit gives every thread two bins");
static_assert(SELECT_BINS == 1 << 11, "the digit shifts and masks of nms_select_kernel are written for 11-bit levels");
constexpr int SORT_TILE = 4096;      // keys sorted in LDS at a time (32 KB)
constexpr int SCAN_CHUNK = 256;      // candidates tested per chunk
constexpr int SCAN_SEGS = 4;         // threads per candidate: each walks every fourth kept box
constexpr int SCAN_THREADS = SCAN_CHUNK * SCAN_SEGS;
constexpr int NMS_MAX_NC = 1024;     // classes the filter mask covers
constexpr int NMS_MAX_DET = 2048;    // kept boxes held in LDS (5 floats and an index each)

struct ClassMask {
    uint32_t w[NMS_MAX_NC / 32];
};

__device__ __forceinline__ bool class_allowed(const ClassMask& m, int c) { return (m.w[c >> 5] >> (c & 31)) & 1u; }

// exclusive prefix sum of v over the workgroup's threads in thread order; total: the sum over all threads.  wsum: NMS_WAVES + 1 ints of LDS.
__device__ __forceinline__ int block_excl_scan(int v, int* wsum, int& total) {
    const int lane = threadIdx.x & (YMI_WAVE - 1), wave = threadIdx.x / YMI_WAVE;
    int inc = v;
#pragma unroll
    for (int o = 1; o < YMI_WAVE; o <<= 1) {
        const int t = __shfl_up(inc, o, YMI_WAVE);
        if (lane >= o) inc += t;
    }
    __syncthreads();  // (wsum free for reuse)
    if (lane == YMI_WAVE - 1) wsum[wave] = inc;
    __syncthreads();
    if (threadIdx.x == 0) {
        int run = 0;
        for (int w = 0; w < NMS_WAVES; ++w) {
            const int t = wsum[w];
            wsum[w] = run;
            run += t;
        }
        wsum[NMS_WAVES] = run;
    }
    __syncthreads();
    total = wsum[NMS_WAVES];
    return wsum[wave] + inc - v;
}

// calls f(class, score bits) for every candidate of anchor a, classes ascending (reference ops.py:250,286-295)
template <typename F>
__device__ __forceinline__ void for_candidates(const float* __restrict__ yb, int A, int nc, int a, float conf, bool multi, bool filter,
                                               const ClassMask& mask, F f) {
    const float* s = yb + (size_t)4 * A + a;
    if (multi) {
        for (int c = 0; c < nc; ++c) {
            const float v = s[(size_t)c * A];
            if (v > conf && (!filter || class_allowed(mask, c))) f(c, __float_as_uint(v));
        }
    } else {
        float best = s[0];
        int bc = 0;
        for (int c = 1; c < nc; ++c) {
            const float v = s[(size_t)c * A];
            if (v > best) {  // strict: the first maximum wins
                best = v;
                bc = c;
            }
        }
        if (best > conf && (!filter || class_allowed(mask, bc))) f(bc, __float_as_uint(best));
    }
}

// One radix-select level over hist[SELECT_BINS] (counts of the candidates that match the prefix so far, by their next digit): the digit d with
// (candidates of larger digits) < need <= (candidates of digits >= d).  out[0] = d, out[1] = need - (candidates of larger digits).
__device__ __forceinline__ void select_digit(const int* hist, int need, int* wsum, int* out) {
    const int hi = SELECT_BINS - 1 - 2 * (int)threadIdx.x, lo = hi - 1;  // thread order = descending digits
    const int ch = hist[hi], cl = hist[lo];
    int total;
    const int above = block_excl_scan(ch + cl, wsum, total);
    if (above < need && need <= above + ch) {
        out[0] = hi;
        out[1] = need - above;
    } else if (above + ch < need && need <= above + ch + cl) {
        out[0] = lo;
        out[1] = need - above - ch;
    }
    __syncthreads();
}

__global__ __launch_bounds__(NMS_THREADS) void nms_select_kernel(const float* __restrict__ y, int A, int nc, int rows, float conf, int multi, int filter,
                                                                 ClassMask mask, int max_nms, int npad, uint64_t* __restrict__ keys,
                                                                 int* __restrict__ ncand) {
    __shared__ int hist[SELECT_BINS];
    __shared__ int wsum[NMS_WAVES + 1];
    __shared__ int sel[2];
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* yb = y + (size_t)b * rows * A;
    uint64_t* kb = keys + (size_t)b * npad;

    // the score of rank max_nms: cut (score bits) and, among candidates with exactly that score, how many to take (lowest indices first)
    uint32_t cut = 0;
    int take_eq = 0, n_total = 0;
    {
        for (int i = tid; i < SELECT_BINS; i += NMS_THREADS) hist[i] = 0;
        __syncthreads();
        int mine = 0;
        for (int a = tid; a < A; a += NMS_THREADS)
            for_candidates(yb, A, nc, a, conf, multi, filter, mask, [&](int, uint32_t bits) {
                ++mine;
                atomicAdd(&hist[bits >> 20], 1);
            });
        block_excl_scan(mine, wsum, n_total);
    }
    if (n_total > max_nms) {  // (workgroup-uniform)
        select_digit(hist, max_nms, wsum, sel);
        const uint32_t d1 = sel[0];
        int need = sel[1];
        __syncthreads();
        for (int i = tid; i < SELECT_BINS; i += NMS_THREADS) hist[i] = 0;
        __syncthreads();
        for (int a = tid; a < A; a += NMS_THREADS)
            for_candidates(yb, A, nc, a, conf, multi, filter, mask, [&](int, uint32_t bits) {
                if ((bits >> 20) == d1) atomicAdd(&hist[(bits >> 9) & (SELECT_BINS - 1)], 1);
            });
        __syncthreads();
        select_digit(hist, need, wsum, sel);
        const uint32_t d2 = (d1 << 11) | sel[0];
        need = sel[1];
        __syncthreads();
        for (int i = tid; i < SELECT_BINS; i += NMS_THREADS) hist[i] = 0;
        __syncthreads();
        for (int a = tid; a < A; a += NMS_THREADS)
            for_candidates(yb, A, nc, a, conf, multi, filter, mask, [&](int, uint32_t bits) {
                if ((bits >> 9) == d2) atomicAdd(&hist[bits & 511], 1);
            });
        __syncthreads();
        select_digit(hist, need, wsum, sel);
        cut = (d2 << 9) | sel[0];
        take_eq = sel[1];
        __syncthreads();
    }

    // ordered compaction: anchors in chunks of NMS_THREADS, a thread's candidates in class order behind those of the threads before it
    int base = 0, eq_base = 0;
    for (int a0 = 0; a0 < A; a0 += NMS_THREADS) {
        const int a = a0 + tid;
        int gt = 0, eq = 0;
        if (a < A)
            for_candidates(yb, A, nc, a, conf, multi, filter, mask, [&](int, uint32_t bits) {
                gt += bits > cut;
                eq += bits == cut;
            });
        int eq_total, w_total;
        const int eq_before = eq_base + block_excl_scan(eq, wsum, eq_total);
        int eq_take = take_eq - eq_before;
        eq_take = eq_take < 0 ? 0 : eq_take > eq ? eq : eq_take;
        int pos = base + block_excl_scan(gt + eq_take, wsum, w_total);
        if (a < A && gt + eq_take > 0) {
            int e = 0;
            for_candidates(yb, A, nc, a, conf, multi, filter, mask, [&](int c, uint32_t bits) {
                bool w = bits > cut;
                if (bits == cut) w = e++ < eq_take;
                if (w) kb[pos++] = ((uint64_t)bits << 32) | (uint32_t)~(uint32_t)(a * nc + c);
            });
        }
        base += w_total;
        eq_base += eq_total;
    }
    // zero keys (they sort last) up to the power of two the sort works on
    int np2 = 1;
    while (np2 < base) np2 <<= 1;
    for (int i = base + tid; i < np2; i += NMS_THREADS) kb[i] = 0;
    if (tid == 0) ncand[b] = base;
}

// ---- bitonic sort, descending ------------------------------------------------------------------------------------------------------
// the compare-exchanges of distance j of the merge step k on `cnt` keys at t[0..cnt), whose first key has index g0 in the whole sequence
__device__ __forceinline__ void bitonic_pass(uint64_t* t, int cnt, int g0, int k, int j) {
    for (int p = threadIdx.x; p < cnt / 2; p += NMS_THREADS) {
        const int i = ((p & ~(j - 1)) << 1) | (p & (j - 1)), q = i | j;
        const uint64_t u = t[i], v = t[q];
        const bool desc = ((g0 + i) & k) == 0;
        if (desc ? u < v : u > v) {
            t[i] = v;
            t[q] = u;
        }
    }
}

__global__ __launch_bounds__(NMS_THREADS) void nms_sort_kernel(uint64_t* __restrict__ keys, int npad, const int* __restrict__ ncand) {
    __shared__ uint64_t tile[SORT_TILE];
    const int b = blockIdx.x, tid = threadIdx.x;
    uint64_t* kb = keys + (size_t)b * npad;
    const int n = ncand[b];
    if (n < 2) return;
    int N = 1;
    while (N < n) N <<= 1;
    const int T = N < SORT_TILE ? N : SORT_TILE;
    // every tile sorted on its own (alternating directions, as the steps k <= T of the whole network leave them)
    for (int g0 = 0; g0 < N; g0 += T) {
        for (int i = tid; i < T; i += NMS_THREADS) tile[i] = kb[g0 + i];
        __syncthreads();
        for (int k = 2; k <= T; k <<= 1)
            for (int j = k >> 1; j > 0; j >>= 1) {
                bitonic_pass(tile, T, g0, k, j);
                __syncthreads();
            }
        for (int i = tid; i < T; i += NMS_THREADS) kb[g0 + i] = tile[i];
        __syncthreads();
    }
    // merge steps wider than a tile: distances >= T in global memory (this workgroup's own stores, visible after the barrier), the rest in LDS
    for (int k = 2 * T; k <= N; k <<= 1) {
        for (int j = k >> 1; j >= T; j >>= 1) {
            bitonic_pass(kb, N, 0, k, j);
            __threadfence_block();
            __syncthreads();
        }
        for (int g0 = 0; g0 < N; g0 += T) {
            for (int i = tid; i < T; i += NMS_THREADS) tile[i] = kb[g0 + i];
            __syncthreads();
            for (int j = T >> 1; j > 0; j >>= 1) {
                bitonic_pass(tile, T, g0, k, j);
                __syncthreads();
            }
            for (int i = tid; i < T; i += NMS_THREADS) kb[g0 + i] = tile[i];
            __threadfence_block();
            __syncthreads();
        }
    }
}

// ---- greedy scan ---------------------------------------------------------------------------------------------------------------------
struct Box {
    float x1, y1, x2, y2, area;
};
// torchvision.ops.nms' decision for one pair, one float32 operation per step (this file is compiled without contraction)
__device__ __forceinline__ bool suppresses(const Box& k, const Box& c, float thr) {
    const float xx1 = fmaxf(k.x1, c.x1), yy1 = fmaxf(k.y1, c.y1), xx2 = fminf(k.x2, c.x2), yy2 = fminf(k.y2, c.y2);
    const float w = fmaxf(0.0f, xx2 - xx1), h = fmaxf(0.0f, yy2 - yy1);
    const float inter = w * h;
    if (!(inter > 0.0f)) return false;  // 0 / u is 0 or NaN: never above a threshold >= 0
    const float uni = (k.area + c.area) - inter;
    return inter / uni > thr;
}

// One workgroup per image: SCAN_CHUNK candidates at a time in sorted order.  Phase A (all SCAN_SEGS * SCAN_CHUNK threads): thread (candidate,
// segment) tests its candidate against every SCAN_SEGS-th kept box, so the kept list is walked by four waves per SIMD at once.  Phase B (the first
// wave): resolves the chunk in order, 64 candidates at a time, with wave operations only.  The rows are written at the end, from the kept indices.
// rows: the rows of y per image (4 + nc, or 4 + nc + nm with mask coefficients behind the scores); coef (or null): [B][max_det][nm], the kept anchors'
// coefficient rows, zero past the count.
__global__ __launch_bounds__(SCAN_THREADS) void nms_scan_kernel(const float* __restrict__ y, int A, int nc, int rows, const uint64_t* __restrict__ keys, int npad,
                                                                const int* __restrict__ ncand, float iou_thres, float max_wh, int max_det,
                                                                float* __restrict__ det, int* __restrict__ count, float* __restrict__ coef, int nm) {
    extern __shared__ float kept[];  // [5][max_det]: offset boxes and areas of the kept candidates; then [max_det] their positions in the sorted list
    __shared__ float cbox[5][SCAN_CHUNK];
    __shared__ int calive[SCAN_CHUNK];
    __shared__ int s_nk;
    float *kx1 = kept, *ky1 = kept + max_det, *kx2 = kept + 2 * max_det, *ky2 = kept + 3 * max_det, *kar = kept + 4 * max_det;
    int* kq = reinterpret_cast<int*>(kept + 5 * max_det);
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & (YMI_WAVE - 1);
    const int cand = tid & (SCAN_CHUNK - 1), seg = tid / SCAN_CHUNK;
    const float* yb = y + (size_t)b * rows * A;
    const uint64_t* kb = keys + (size_t)b * npad;
    float* db = det + (size_t)b * max_det * 6;
    const int n = ncand[b];
    int nk = 0;
    for (int base = 0; base < n && nk < max_det; base += SCAN_CHUNK) {
        // phase A
        const int q = base + cand;
        Box c = {0.f, 0.f, 0.f, 0.f, 0.f};
        if (q < n) {
            const uint32_t idx = ~(uint32_t)kb[q];
            const int a = idx / nc, cls = idx - a * nc;
            const float x = yb[a], yy = yb[(size_t)A + a], hw = yb[(size_t)2 * A + a] / 2.0f, hh = yb[(size_t)3 * A + a] / 2.0f;
            const float off = (float)cls * max_wh;
            c.x1 = (x - hw) + off;
            c.y1 = (yy - hh) + off;
            c.x2 = (x + hw) + off;
            c.y2 = (yy + hh) + off;
            c.area = (c.x2 - c.x1) * (c.y2 - c.y1);
        }
        if (seg == 0) {
            cbox[0][cand] = c.x1;
            cbox[1][cand] = c.y1;
            cbox[2][cand] = c.x2;
            cbox[3][cand] = c.y2;
            cbox[4][cand] = c.area;
            calive[cand] = q < n;
        }
        __syncthreads();
        if (q < n) {
            bool sup = false;
            for (int k0 = seg; k0 < nk && !sup; k0 += 4 * SCAN_SEGS) {
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int k = k0 + u * SCAN_SEGS;
                    if (k < nk) {
                        const Box kk = {kx1[k], ky1[k], kx2[k], ky2[k], kar[k]};
                        sup |= suppresses(kk, c, iou_thres);
                    }
                }
            }
            if (sup) calive[cand] = 0;  // (several segments may store the same 0)
        }
        __syncthreads();
        // phase B
        if (tid < YMI_WAVE) {
            const int nk_a = nk;
            for (int s = 0; s < SCAN_CHUNK / YMI_WAVE && nk < max_det; ++s) {
                const int m = s * YMI_WAVE + lane;
                const Box mb = {cbox[0][m], cbox[1][m], cbox[2][m], cbox[3][m], cbox[4][m]};
                bool al = calive[m] != 0;
                for (int k = nk_a; k < nk; ++k) {  // kept by the 64s before this one
                    const Box kk = {kx1[k], ky1[k], kx2[k], ky2[k], kar[k]};
                    if (al && suppresses(kk, mb, iou_thres)) al = false;
                }
                uint64_t live = __ballot(al);
                while (live && nk < max_det) {
                    const int i = __builtin_ctzll(live);
                    const Box kb_ = {__shfl(mb.x1, i, YMI_WAVE), __shfl(mb.y1, i, YMI_WAVE), __shfl(mb.x2, i, YMI_WAVE), __shfl(mb.y2, i, YMI_WAVE),
                                     __shfl(mb.area, i, YMI_WAVE)};
                    if (lane == i) {
                        kx1[nk] = mb.x1;
                        ky1[nk] = mb.y1;
                        kx2[nk] = mb.x2;
                        ky2[nk] = mb.y2;
                        kar[nk] = mb.area;
                        kq[nk] = base + m;
                    }
                    ++nk;
                    if (lane > i && al && suppresses(kb_, mb, iou_thres)) al = false;
                    live = __ballot(al && lane > i);
                }
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");  // this wave's kept[] stores before its next loads of them
                __builtin_amdgcn_wave_barrier();
            }
            if (tid == 0) s_nk = nk;
        }
        __syncthreads();
        nk = s_nk;
    }
    __syncthreads();
    // the rows carry the original boxes, formed as above without the offset
    for (int i = tid; i < nk; i += SCAN_THREADS) {
        const uint64_t key = kb[kq[i]];
        const uint32_t idx = ~(uint32_t)key;
        const int a = idx / nc, cls = idx - a * nc;
        const float x = yb[a], yy = yb[(size_t)A + a], hw = yb[(size_t)2 * A + a] / 2.0f, hh = yb[(size_t)3 * A + a] / 2.0f;
        float* r = db + (size_t)i * 6;
        r[0] = x - hw;
        r[1] = yy - hh;
        r[2] = x + hw;
        r[3] = yy + hh;
        r[4] = __uint_as_float((uint32_t)(key >> 32));
        r[5] = (float)cls;
    }
    for (int i = nk * 6 + tid; i < max_det * 6; i += SCAN_THREADS) db[i] = 0.0f;
    if (coef) {  // (workgroup-uniform)
        float* cb = coef + (size_t)b * max_det * nm;
        for (int e = tid; e < nk * nm; e += SCAN_THREADS) {
            const int i = e / nm, m = e - i * nm;
            const uint32_t idx = ~(uint32_t)kb[kq[i]];
            cb[e] = yb[(size_t)(4 + nc + m) * A + idx / nc];
        }
        for (int e = nk * nm + tid; e < max_det * nm; e += SCAN_THREADS) cb[e] = 0.0f;
    }
    if (tid == 0) count[b] = nk;
}

int next_pow2(int64_t v) {
    int p = 1;
    while (p < v) p <<= 1;
    return p;
}

}  // namespace

extern "C" int ymi_detect_nms_sizes(int64_t batch, int64_t anchors, int64_t nc, int64_t max_nms, int64_t max_det, size_t* workspace_bytes) {
    YMI_CHECK_ARG(batch > 0 && anchors > 0 && nc > 0 && workspace_bytes, "detect_nms_sizes: bad shape");
    YMI_CHECK_ARG(anchors * nc < ((int64_t)1 << 31), "detect_nms_sizes: anchors * nc must fit 31 bits");
    YMI_CHECK_ARG(max_nms > 0 && max_nms <= (1 << 20) && max_det > 0 && max_det <= NMS_MAX_DET, "detect_nms_sizes: max_nms in [1, 2^20], max_det in [1, %d]",
                  NMS_MAX_DET);
    // keys [batch][pow2 >= min(max_nms, anchors * nc)] uint64, then the candidate counts [batch] int32
    const int64_t cap = max_nms < anchors * nc ? max_nms : anchors * nc;
    *workspace_bytes = (size_t)batch * next_pow2(cap) * 8 + (((size_t)batch * 4 + 15) & ~(size_t)15);
    return YMI_OK;
}

namespace {
// the one host body of ymi_detect_nms (nm == 0, coef == NULL) and ymi_detect_nms_seg
int detect_nms_run(const char* who, const float* y, int64_t batch, int64_t nc, int64_t nm, int64_t anchors, float conf_thres, float iou_thres,
                   int32_t multi_label, int32_t agnostic, const int32_t* host_classes, int32_t n_classes, int64_t max_det, int64_t max_nms, float max_wh,
                   float* det, int32_t* count, float* coef, void* workspace, size_t workspace_bytes, void* stream) {
    size_t need = 0;
    const int rc = ymi_detect_nms_sizes(batch, anchors, nc, max_nms, max_det, &need);
    if (rc != YMI_OK) return rc;
    YMI_CHECK_ARG(y && det && count && workspace, "%s: null pointer", who);
    YMI_CHECK_ARG(conf_thres >= 0.0f && conf_thres <= 1.0f, "%s: conf_thres %g outside [0, 1]", who, (double)conf_thres);
    YMI_CHECK_ARG(iou_thres >= 0.0f && iou_thres <= 1.0f, "%s: iou_thres %g outside [0, 1]", who, (double)iou_thres);
    YMI_CHECK_ARG(max_wh >= 0.0f, "%s: max_wh must not be negative", who);
    YMI_CHECK_ARG(n_classes >= 0 && (n_classes == 0 || host_classes), "%s: classes", who);
    YMI_CHECK_ARG(!host_classes || nc <= NMS_MAX_NC, "%s: the class filter covers %d classes", who, NMS_MAX_NC);
    YMI_CHECK_ARG(nm >= 0 && nm <= (1 << 16) && (4 + nc + nm) * anchors < ((int64_t)1 << 31), "%s: nm in [0, 65536] and (4 + nc + nm) * anchors below 2^31", who);
    if (((uintptr_t)y & 3) || ((uintptr_t)det & 3) || ((uintptr_t)count & 3) || ((uintptr_t)coef & 3) || ((uintptr_t)workspace & 7)) {
        ymi_set_error("%s: y / det / count / coef need 4-byte, the workspace 8-byte alignment", who);
        return YMI_EALIGN;
    }
    if (workspace_bytes < need) {
        ymi_set_error("%s: workspace of %zu bytes, %zu needed", who, workspace_bytes, need);
        return YMI_EWORKSPACE;
    }
    ClassMask mask = {};
    for (int i = 0; i < n_classes; ++i) {
        YMI_CHECK_ARG(host_classes[i] >= 0 && host_classes[i] < nc, "%s: class %d outside [0, %lld)", who, host_classes[i], (long long)nc);
        mask.w[host_classes[i] >> 5] |= 1u << (host_classes[i] & 31);
    }
    const int64_t cap = max_nms < anchors * nc ? max_nms : anchors * nc;
    const int npad = next_pow2(cap);
    const int rows = (int)(4 + nc + nm);
    uint64_t* keys = (uint64_t*)workspace;
    int* ncand = (int*)((char*)workspace + (size_t)batch * npad * 8);
    hipStream_t s = (hipStream_t)stream;
    const int multi = multi_label && nc > 1;  // reference ops.py:255
    hipLaunchKernelGGL(nms_select_kernel, dim3((unsigned)batch), dim3(NMS_THREADS), 0, s, y, (int)anchors, (int)nc, rows, conf_thres, multi, host_classes ? 1 : 0,
                       mask, (int)cap, npad, keys, ncand);
    YMI_CHECK_LAUNCH("detect_nms (select)");
    hipLaunchKernelGGL(nms_sort_kernel, dim3((unsigned)batch), dim3(NMS_THREADS), 0, s, keys, npad, ncand);
    YMI_CHECK_LAUNCH("detect_nms (sort)");
    hipLaunchKernelGGL(nms_scan_kernel, dim3((unsigned)batch), dim3(SCAN_THREADS), (size_t)max_det * 6 * sizeof(float), s, y, (int)anchors, (int)nc, rows, keys, npad,
                       ncand, iou_thres, agnostic ? 0.0f : max_wh, (int)max_det, det, count, coef, (int)nm);
    YMI_CHECK_LAUNCH("detect_nms (scan)");
    return YMI_OK;
}
}  // namespace

extern "C" int ymi_detect_nms(const float* y, int64_t batch, int64_t nc, int64_t anchors, float conf_thres, float iou_thres, int32_t multi_label,
                              int32_t agnostic, const int32_t* host_classes, int32_t n_classes, int64_t max_det, int64_t max_nms, float max_wh, float* det,
                              int32_t* count, void* workspace, size_t workspace_bytes, void* stream) {
    return detect_nms_run("detect_nms", y, batch, nc, 0, anchors, conf_thres, iou_thres, multi_label, agnostic, host_classes, n_classes, max_det, max_nms, max_wh,
                          det, count, nullptr, workspace, workspace_bytes, stream);
}

extern "C" int ymi_detect_nms_seg(const float* y, int64_t batch, int64_t nc, int64_t nm, int64_t anchors, float conf_thres, float iou_thres,
                                  int32_t multi_label, int32_t agnostic, const int32_t* host_classes, int32_t n_classes, int64_t max_det, int64_t max_nms,
                                  float max_wh, float* det, int32_t* count, float* coef, void* workspace, size_t workspace_bytes, void* stream) {
    YMI_CHECK_ARG(nm >= 1 && coef, "detect_nms_seg: nm >= 1 and a coefficient output");
    return detect_nms_run("detect_nms_seg", y, batch, nc, nm, anchors, conf_thres, iou_thres, multi_label, agnostic, host_classes, n_classes, max_det, max_nms,
                          max_wh, det, count, coef, workspace, workspace_bytes, stream);
}
