// v8 detection loss on the per-level Detect maps: DFL decode, task-aligned assignment, CIoU + DFL + BCE sums and
// their gradients, in ten small launches instead of several hundred framework ops.
//
// Mathematics follows the reference (ultralytics/utils/loss.py:201-255 v8DetectionLoss.__call__, loss.py:65-120
// DFLoss/BboxLoss, utils/tal.py:14-327 TaskAlignedAssigner, utils/metrics.py:74-134 bbox_iou CIoU) on the layout the
// Detect convolutions already write: per level an NHWC box map [B,H,W,4*reg_max] and class map [B,H,W,nc].
// Anchor a of image b = level l, pixel q = a - off[l] (row-major y,x): exactly the reference's concat order.
//
// Everything is f32 and deterministic (fixed-order block reductions, no atomics).  top-k ties go to the lower anchor
// index (the reference leaves tie order to torch.topk).
//
// Each fact has one statement: side_of (the four-lanes-per-anchor prologue of the decode and loss kernels), pred_box, map_row, ciou,
// the gt_* / centre_inside / clamped_label rules of the dense target rows, topk_offer (the selection rule), block_combine (the
// workgroup reductions), carve_state / carve_work (the buffer layouts), quad_grid / anchor_grid.
//
// Oriented boxes (reference: nn/modules/head.py:211-238 OBB, utils/loss.py:111-132 RotatedBboxLoss, loss.py:607-720 v8OBBLoss, utils/tal.py:329-361
// RotatedTaskAlignedAssigner) run through the same kernels and the same host pipeline.  What reads a box as a box is a policy, AxisBox (xyxy,
// CIoU) or RotBox (xywhr, probiou, the anchors' angle): targets_kernel<Box>, decode_kernel<T, Box>, loss_kernel<T, GRAD, Box> with dfl_target,
// dfl_term and class_branch<T, GRAD> beside it, topk_kernel<Box::Gt>, finalize_kernel<Box::NB>; infer_decode_kernel<T, Tail> writes the three eval
// outputs (NoTail, MaskMaps, AngleTail); loss_fwd_impl<Box>, loss_bwd_impl<Box>, loss_sizes_impl, targets_impl<Box> and decode_impl<Tail> are the
// bodies of the extern "C" entry points, walk_levels the level walk of fill_geom and fill_angle_geom.  Two stages keep a kernel per box kind, on
// purpose: the metric (see obb_metric_kernel) and the gradients of the oriented loss (see obb_loss_kernel).  The forms of the shared code are
// the ones that kept the arithmetic: profiles/loss_box_refactor_ab.txt.
#include "common.h"

namespace {
constexpr int LOSS_MAXL = 4;
constexpr int REG = 16;  // reg_max (DFL bins per side)
constexpr float TAL_EPS = 1e-9f;

struct LossGeom {
    const void* box[LOSS_MAXL];
    const void* cls[LOSS_MAXL];
    void* dbox[LOSS_MAXL];
    void* dcls[LOSS_MAXL];
    int64_t ldb[LOSS_MAXL], ldc[LOSS_MAXL], lddb[LOSS_MAXL], lddc[LOSS_MAXL];
    int H[LOSS_MAXL], W[LOSS_MAXL], off[LOSS_MAXL + 1];
    float stride[LOSS_MAXL];
    int nl, B, A, G, nc;  // G: target rows per image (max_boxes), the forward's only
    int dcw;  // backward: channels of the class-gradient maps (>= nc; the ones beyond nc are written as zeros: padded gradient buffers)
};

struct Anchor {
    int l;
    int64_t pix;  // pixel row inside the level's maps (b, y, x)
    float ax, ay, s;
};

// arr[l] by a select chain: a dynamically indexed kernel-argument array would be copied to scratch memory
template <typename X> __device__ __forceinline__ X pick(const X (&arr)[LOSS_MAXL], int l) {
    X r = arr[0];
#pragma unroll
    for (int i = 1; i < LOSS_MAXL; ++i) r = (l == i) ? arr[i] : r;
    return r;
}

__device__ __forceinline__ Anchor anchor_of(const LossGeom& g, int b, int a) {
    int l = 0, off = 0, w = g.W[0], h = g.H[0];
    float s = g.stride[0];
#pragma unroll
    for (int i = 1; i < LOSS_MAXL; ++i)
        if (i < g.nl && a >= g.off[i]) {
            l = i;
            off = g.off[i];
            w = g.W[i];
            h = g.H[i];
            s = g.stride[i];
        }
    const int q = a - off;
    const int y = q / w, x = q - y * w;
    Anchor r;
    r.l = l;
    r.pix = (int64_t)b * h * w + q;
    r.ax = x + 0.5f;
    r.ay = y + 0.5f;
    r.s = s;
    return r;
}

// the anchor's pixel row in its level's map: map_row<const T>(g.box, g.ldb, an), map_row<T>(g.dcls, g.lddc, an), ...
template <typename T, typename V> __device__ __forceinline__ T* map_row(V* const (&maps)[LOSS_MAXL], const int64_t (&lds)[LOSS_MAXL], const Anchor& an) {
    return reinterpret_cast<T*>(pick(maps, an.l)) + an.pix * pick(lds, an.l);
}

// predicted xyxy box (grid units) from the four side distances (reference dist2bbox, xywh=False)
__device__ __forceinline__ void pred_box(const Anchor& an, const float (&d)[4], float (&b)[4]) {
    b[0] = an.ax - d[0];
    b[1] = an.ay - d[1];
    b[2] = an.ax + d[2];
    b[3] = an.ay + d[3];
}

// CIoU of xyxy boxes, b1 and b2 in the order the reference passes them (metrics.py:74-134, xywh=False, CIoU=True); GRAD: also its
// gradient g[4] with respect to b1 (alpha is a constant, as under the reference's no_grad)
template <bool GRAD = false> __device__ __forceinline__ float ciou(const float (&b1)[4], const float (&b2)[4], float* g = nullptr) {
    const float eps = 1e-7f;
    const float w1 = b1[2] - b1[0], h1 = b1[3] - b1[1] + eps, w2 = b2[2] - b2[0], h2 = b2[3] - b2[1] + eps;
    const float iwr = fminf(b1[2], b2[2]) - fmaxf(b1[0], b2[0]);
    const float ihr = fminf(b1[3], b2[3]) - fmaxf(b1[1], b2[1]);
    const float iw = fmaxf(iwr, 0.f), ih = fmaxf(ihr, 0.f);
    const float inter = iw * ih;
    const float uni = w1 * h1 + w2 * h2 - inter + eps;
    const float iou = inter / uni;
    const float cw = fmaxf(b1[2], b2[2]) - fminf(b1[0], b2[0]);
    const float ch = fmaxf(b1[3], b2[3]) - fminf(b1[1], b2[1]);
    const float c2 = cw * cw + ch * ch + eps;
    const float sx = b2[0] + b2[2] - b1[0] - b1[2], sy = b2[1] + b2[3] - b1[1] - b1[3];
    const float rho2 = (sx * sx + sy * sy) * 0.25f;
    const float u = w1 / h1;
    const float dv = atanf(w2 / h2) - atanf(u);
    const float kk = 0.40528473456935108578f;  // 4 / pi^2
    const float v = kk * dv * dv;
    const float alpha = v / (v - iou + (1.0f + eps));
    if constexpr (GRAD) {
        const float on_w = iwr > 0.f ? 1.f : 0.f, on_h = ihr > 0.f ? 1.f : 0.f;
        float dint[4];
        dint[0] = -(b1[0] > b2[0] ? 1.f : 0.f) * on_w * ih;
        dint[1] = -(b1[1] > b2[1] ? 1.f : 0.f) * on_h * iw;
        dint[2] = (b1[2] < b2[2] ? 1.f : 0.f) * on_w * ih;
        dint[3] = (b1[3] < b2[3] ? 1.f : 0.f) * on_h * iw;
        const float duni[4] = {-h1 - dint[0], -w1 - dint[1], h1 - dint[2], w1 - dint[3]};
        const float dc2[4] = {-(b1[0] < b2[0] ? 1.f : 0.f) * 2.f * cw, -(b1[1] < b2[1] ? 1.f : 0.f) * 2.f * ch,
                              (b1[2] > b2[2] ? 1.f : 0.f) * 2.f * cw, (b1[3] > b2[3] ? 1.f : 0.f) * 2.f * ch};
        const float drho[4] = {-0.5f * sx, -0.5f * sy, -0.5f * sx, -0.5f * sy};
        const float dat = 1.0f / (1.0f + u * u);
        const float du[4] = {-1.0f / h1, w1 / (h1 * h1), 1.0f / h1, -w1 / (h1 * h1)};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float diou = (dint[i] * uni - inter * duni[i]) / (uni * uni);
            const float dpen = (drho[i] * c2 - rho2 * dc2[i]) / (c2 * c2);
            const float dvv = 2.f * kk * dv * (-dat * du[i]);
            g[i] = diou - dpen - alpha * dvv;
        }
    }
    return iou - (rho2 / c2 + v * alpha);
}

// one side's 16 bins as floats, by 16-byte chunks of ElemTraits<T>::CH elements: Pack<T, CH> in a loop.  (store16 says the same on the vector
// type itself: through Pack<bf16_t, 8>::store and the float[8] in between, the bfloat16 gradient kernel's sums pair up differently in the SLP
// vectoriser, other products are fused, and last bits of the box gradients move - profiles/loss_refactor_ab.txt.)
template <typename T> __device__ __forceinline__ void load16(const T* p, float (&v)[REG]) {
    constexpr int CH = ElemTraits<T>::CH;
#pragma unroll
    for (int i = 0; i < REG; i += CH) {
        float t[CH];
        Pack<T, CH>::load(p + i, t);
#pragma unroll
        for (int j = 0; j < CH; ++j) v[i + j] = t[j];
    }
}
template <typename T> __device__ __forceinline__ void store16(T* p, const float (&v)[REG]) {
    constexpr int CH = ElemTraits<T>::CH;
    typedef T Chunk __attribute__((ext_vector_type(CH)));
#pragma unroll
    for (int i = 0; i < REG / CH; ++i) {
        Chunk t;
#pragma unroll
        for (int j = 0; j < CH; ++j) t[j] = from_f32<T>(v[CH * i + j]);
        *reinterpret_cast<Chunk*>(p + CH * i) = t;
    }
}

// softmax over one side's 16 bins -> probabilities p, returns the expectation sum_j j*p_j (reference DFL decode)
__device__ __forceinline__ float softmax_expect(const float (&x)[REG], float (&p)[REG], float* lse) {
    float m = x[0];
#pragma unroll
    for (int j = 1; j < REG; ++j) m = fmaxf(m, x[j]);
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < REG; ++j) {
        p[j] = __expf(x[j] - m);
        s += p[j];
    }
    const float inv = 1.0f / s;
    float e = 0.f;
#pragma unroll
    for (int j = 0; j < REG; ++j) {
        p[j] *= inv;
        e += (float)j * p[j];
    }
    *lse = m + __logf(s);
    return e;
}

// the four side distances of one anchor live in the four lanes of a quad: gather them into every lane
__device__ __forceinline__ void quad_gather(float mine, float (&d)[4]) {
    const int base = (threadIdx.x & 63) & ~3;
#pragma unroll
    for (int k = 0; k < 4; ++k) d[k] = __shfl(mine, base + k, 64);
}

// ---- the prologue of the kernels that give an anchor four lanes, one per box side (decode_kernel, infer_decode_kernel, loss_kernel) ----
// thread -> (anchor, side); the side's 16 logits x, their softmax p, log-sum-exp lse and expectation e; d: the anchor's four expectations.
// Threads past the last anchor are not live: they compute on anchor 0 (the quad shuffles want every lane) and must store nothing.
// x and p stay arrays of the kernel, filled through references: as members of Side the float32 gradient kernel's multiply-adds came out
// fused otherwise than before (same record).
struct Side {
    bool live;
    int b, a, side;
    int64_t ia;  // b * A + a
    Anchor an;
    float lse, e, d[4];
};
template <typename T> __device__ __forceinline__ void side_of(const LossGeom& g, Side& s, float (&x)[REG], float (&p)[REG]) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t quad = t >> 2;
    s.side = (int)(t & 3);
    s.live = quad < (int64_t)g.B * g.A;
    s.b = s.live ? (int)(quad / g.A) : 0;
    s.a = s.live ? (int)(quad - (int64_t)s.b * g.A) : 0;
    s.ia = (int64_t)s.b * g.A + s.a;
    s.an = anchor_of(g, s.b, s.a);
    load16<T>(map_row<const T>(g.box, g.ldb, s.an) + s.side * REG, x);
    s.e = softmax_expect(x, p, &s.lse);
    quad_gather(s.e, s.d);
}

// ---- workgroup combine (256 threads = 4 waves) of N values per thread: the wave's reduction, lane 0 of each wave to sh[n][wave], barrier,
// then every thread combines the four.  An Op states both steps, i.e. the association: (w0 + w1) + (w2 + w3) for sums and maxima, the
// `better` chain in wave order for Best.  A caller that combines again with the same sh puts a barrier between the rounds.
struct SumOp {
    static __device__ __forceinline__ float wave(float v) { return wave_sum(v); }
    static __device__ __forceinline__ float four(const float (&s)[4]) { return (s[0] + s[1]) + (s[2] + s[3]); }
};
struct MaxOp {
    static __device__ __forceinline__ float wave(float v) { return wave_max(v); }
    static __device__ __forceinline__ float four(const float (&s)[4]) { return fmaxf(fmaxf(s[0], s[1]), fmaxf(s[2], s[3])); }
};
struct Best {
    float v;
    int i;
};
__device__ __forceinline__ Best better(Best x, Best y) { return (y.v > x.v || (y.v == x.v && y.i < x.i)) ? y : x; }
struct BestOp {
    static __device__ __forceinline__ Best wave(Best mine) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) mine = better(mine, Best{__shfl_xor(mine.v, o, 64), __shfl_xor(mine.i, o, 64)});
        return mine;
    }
    static __device__ __forceinline__ Best four(const Best (&s)[4]) { return better(better(better(s[0], s[1]), s[2]), s[3]); }
};
template <typename Op, typename V, int N> __device__ __forceinline__ void block_combine(V (&v)[N], V (&sh)[N][4]) {
#pragma unroll
    for (int n = 0; n < N; ++n) {
        v[n] = Op::wave(v[n]);
        if ((threadIdx.x & 63) == 0) sh[n][threadIdx.x >> 6] = v[n];
    }
    __syncthreads();
#pragma unroll
    for (int n = 0; n < N; ++n) v[n] = Op::four(sh[n]);
}

// ---- dense targets [B, G, row]: the class, then the box (targets_kernel below writes them) ------------------------------------------------
constexpr int GT_ROW = 5;   // class, xyxy (pixels)
constexpr int OBB_ROW = 6;  // class, x, y, w, h (pixels), angle
// the label row that fills slot `slot` of image b: the slot-th kept row of that image in row order (stable); -1: an empty slot
template <typename Keep> __device__ __forceinline__ int label_row_of(const float* batch_idx, int n, int b, int slot, Keep keep) {
    int seen = 0;
    for (int i = 0; i < n; ++i) {
        if (keep(i) && (int)batch_idx[i] == b) {
            if (seen == slot) return i;
            ++seen;
        }
    }
    return -1;
}
// the readers of the axis rows: row bg = b * G + k of the dense targets, its box, "is it a label or a padding row", "is the anchor's centre
// inside it" (tal.py:262-283 select_candidates_in_gts), its class as an index of the class map
__device__ __forceinline__ const float* gt_row(const float* targets, int64_t bg) { return targets + bg * GT_ROW; }
__device__ __forceinline__ void gt_box(const float* tg, float (&gt)[4]) {
#pragma unroll
    for (int k = 0; k < 4; ++k) gt[k] = tg[1 + k];
}
__device__ __forceinline__ bool gt_valid(const float (&gt)[4]) { return (gt[0] + gt[1] + gt[2] + gt[3]) > 0.f; }
__device__ __forceinline__ bool centre_inside(const Anchor& an, const float (&gt)[4]) {
    const float px = an.ax * an.s, py = an.ay * an.s;
    const float dmin = fminf(fminf(px - gt[0], py - gt[1]), fminf(gt[2] - px, gt[3] - py));
    return dmin > TAL_EPS;
}
__device__ __forceinline__ int clamped_label(const float* tg, int nc) {
    const int lab = (int)tg[0];
    return lab < 0 ? 0 : (lab >= nc ? nc - 1 : lab);
}

// ---- the rotated forms (reference: utils/tal.py:397-416 dist2rbox, utils/metrics.py:178-239 probiou) ----------------------------------------
// An oriented box is (x, y, w, h, r): centre, extents along its own axes, angle in radians.
struct Rot {
    float cs, sn;
};
__device__ __forceinline__ Rot rot_of(float r) { return Rot{cosf(r), sinf(r)}; }
// dist2rbox: the four side distances, turned by the angle about the anchor -> (x, y, w, h) in grid units
__device__ __forceinline__ void rbox_of(const Anchor& an, const float (&d)[4], const Rot& q, float (&o)[4]) {
    const float xf = (d[2] - d[0]) * 0.5f, yf = (d[3] - d[1]) * 0.5f;
    o[0] = xf * q.cs - yf * q.sn + an.ax;
    o[1] = xf * q.sn + yf * q.cs + an.ay;
    o[2] = d[0] + d[2];
    o[3] = d[1] + d[3];
}
struct Cov {
    float a, b, c;
};
__device__ __forceinline__ Cov cov_of(float w, float h, const Rot& q) {  // metrics.py:178-195
    const float A = w * w / 12.0f, B = h * h / 12.0f;
    const float c2 = q.cs * q.cs, s2 = q.sn * q.sn;
    return Cov{A * c2 + B * s2, A * s2 + B * c2, (A - B) * q.cs * q.sn};
}
// probiou of box 1 (centre x1, y1, covariance c1) and box 2, in the reference's operand order (metrics.py:215-231).  GRAD: also
// gp[5] = d / d(x1, y1, c1.a, c1.b, c1.c).  The clamps pass no gradient outside their range (torch's clamp: the ends included).
template <bool GRAD = false>
__device__ __forceinline__ float probiou_cov(float x1, float y1, const Cov& c1, float x2, float y2, const Cov& c2, float* gp = nullptr) {
    const float eps = 1e-7f;
    const float Sa = c1.a + c2.a, Sb = c1.b + c2.b, Sc = c1.c + c2.c;
    const float dx = x1 - x2, dy = y1 - y2;
    const float D = Sa * Sb - Sc * Sc;
    const float den = D + eps;
    const float N1 = Sa * (dy * dy) + Sb * (dx * dx);
    const float N2 = Sc * (x2 - x1) * (y1 - y2);
    const float t1 = N1 / den * 0.25f;
    const float t2 = N2 / den * 0.5f;
    const float r1 = c1.a * c1.b - c1.c * c1.c, r2 = c2.a * c2.b - c2.c * c2.c;
    const float d1 = fmaxf(r1, 0.f), d2 = fmaxf(r2, 0.f);
    const float sq = sqrtf(d1 * d2);
    const float q = 4.0f * sq + eps;
    const float u = D / q + eps;
    const float t3 = logf(u) * 0.5f;
    const float raw = t1 + t2 + t3;
    const float bd = fminf(fmaxf(raw, eps), 100.0f);
    const float ex = expf(-bd);
    const float hd = sqrtf(1.0f - ex + eps);
    if constexpr (GRAD) {
        const float dbd = (raw >= eps && raw <= 100.0f) ? -ex / (2.0f * hd) : 0.f;  // d iou / d raw
        const float inv = 1.0f / den;
        const float M = (0.25f * N1 + 0.5f * N2) * inv * inv;  // (t1 + t2) / den
        const float l = 0.5f / (u * q);                        // d t3 / d D
        const float gSa = 0.25f * dy * dy * inv - M * Sb + l * Sb;
        const float gSb = 0.25f * dx * dx * inv - M * Sa + l * Sa;
        const float gSc = -0.5f * dx * dy * inv + 2.0f * M * Sc - 2.0f * l * Sc;
        // d t3 / d d1 through q = 4 sqrt(d1 d2) + eps; a degenerate box (d1 d2 = 0, where torch's sqrt has no finite slope) passes nothing
        const float gd1 = (r1 >= 0.f && sq > 0.f) ? (-0.5f * D / (u * q * q)) * (2.0f * d2 / sq) : 0.f;
        gp[0] = dbd * (0.5f * Sb * dx - 0.5f * Sc * dy) * inv;
        gp[1] = dbd * (0.5f * Sa * dy - 0.5f * Sc * dx) * inv;
        gp[2] = dbd * (gSa + gd1 * c1.b);
        gp[3] = dbd * (gSb + gd1 * c1.a);
        gp[4] = dbd * (gSc - 2.0f * gd1 * c1.c);
    }
    return 1.0f - hd;
}
// the chain from the covariance back to (w, h, r): gc = d / d(c.a, c.b, c.c) -> gw, gh, gr
__device__ __forceinline__ void cov_grad(float w, float h, const Rot& q, const Cov& c, const float* gc, float& gw, float& gh, float& gr) {
    const float c2 = q.cs * q.cs, s2 = q.sn * q.sn, cs = q.cs * q.sn;
    const float gA = gc[0] * c2 + gc[1] * s2 + gc[2] * cs;
    const float gB = gc[0] * s2 + gc[1] * c2 - gc[2] * cs;
    gw = gA * w / 6.0f;
    gh = gB * h / 6.0f;
    gr = 2.0f * c.c * (gc[1] - gc[0]) + gc[2] * (w * w / 12.0f - h * h / 12.0f) * (c2 - s2);
}
__device__ __forceinline__ bool obb_valid(const float* tg) { return ((((tg[1] + tg[2]) + tg[3]) + tg[4]) + tg[5]) > 0.f; }  // loss.py:659

// the value of this lane's side among four
__device__ __forceinline__ float side_pick(int side, const float (&o)[4]) { return side == 0 ? o[0] : side == 1 ? o[1] : side == 2 ? o[2] : o[3]; }

// ---- what reads a box as a box: the two policies of targets_kernel, decode_kernel and loss_kernel -------------------------------------------
// NB values per box and how a dense target row is made of a label; the decode's row of the predicted box; for the loss kernel the load of
// the assigned target, its four DFL edges, the box term (an overlap: the loss is (1 - overlap) * weight), the gradient of (1 - overlap) with
// respect to this lane's side distance (AxisBox::dist_grad works the whole gradient out; RotBox has none, see obb_loss_kernel).  The constructor is what
// every anchor pays, foreground() what a foreground anchor adds before either term.  Args: what a policy's kernels take beyond the shared
// arguments, passed by value.  Gt: the policy's view of a label in topk_kernel (with that kernel, below).
// AxisBox: xyxy, CIoU, no arguments of its own (reference BboxLoss, loss.py:88-108).
struct AxisGt;
struct RotGt;
struct AxisBox {
    static constexpr int NB = 4;
    typedef AxisGt Gt;
    struct Args {};
    static __host__ bool args_ok(const Args&) { return true; }
    // targets (loss.py:176-191 preprocess): every label is kept; xywh normalised -> xyxy pixels
    static __device__ __forceinline__ bool keep(const float*, int, float, float) { return true; }
    static __device__ __forceinline__ void label_row(const float* xywh, int row, float img_w, float img_h, float (&o)[NB]) {
        const float cx = xywh[row * 4 + 0] * img_w, cy = xywh[row * 4 + 1] * img_h, bw = xywh[row * 4 + 2] * img_w, bh = xywh[row * 4 + 3] * img_h;
        o[0] = cx - bw / 2;
        o[1] = cy - bh / 2;
        o[2] = cx + bw / 2;
        o[3] = cy + bh / 2;
    }
    // decode: [B, A, 4] xyxy in grid units
    static __device__ __forceinline__ void store_pred(const Args&, const Side& s, float* pb) {
        float o[4];
        pred_box(s.an, s.d, o);
        Pack<float, 4>::store(pb + s.ia * 4, o);
    }
    // loss: DFL edges of the target (loss.py:101-104, 75-83)
    static __device__ __forceinline__ void load(const float* tgt, int64_t ia, float (&tb)[NB]) { Pack<float, 4>::load(tgt + ia * 4, tb); }
    static __device__ __forceinline__ float edge(const Anchor& an, const float (&tb)[NB], int side) {
        return side == 0 ? an.ax - tb[0] : side == 1 ? an.ay - tb[1] : side == 2 ? tb[2] - an.ax : tb[3] - an.ay;
    }
    float pbx[4];
    __device__ __forceinline__ AxisBox(const Args&, const Side& s) { pred_box(s.an, s.d, pbx); }
    __device__ __forceinline__ void foreground(const float (&)[NB]) {}
    __device__ __forceinline__ float overlap(const float (&tb)[NB]) const { return ciou(pbx, tb); }
    // x1 = ax - d0, y1 = ay - d1, x2 = ax + d2, y2 = ay + d3
    __device__ __forceinline__ float dist_grad(const float (&tb)[NB], int side) {
        float gc[4];
        (void)ciou<true>(pbx, tb, gc);
        return side < 2 ? gc[side] : -gc[side];
    }
};
// RotBox: xywhr, probiou; reads the anchors' angle [B, A] (reference RotatedBboxLoss, loss.py:111-132)
struct RotBox {
    static constexpr int NB = 5;
    typedef RotGt Gt;
    struct Args {
        const float* angle;
    };
    static __host__ bool args_ok(const Args& a) { return a.angle != nullptr; }
    // targets (loss.py:652-657): xywh normalised -> pixels, the angle as it is, behind the tiny-box filter - the reference multiplies the WIDTH
    // by the image height and the height by the image width (loss.py:655)
    static __device__ __forceinline__ bool keep(const float* xywhr, int i, float img_w, float img_h) {
        return xywhr[i * 5 + 2] * img_h >= 2.0f && xywhr[i * 5 + 3] * img_w >= 2.0f;
    }
    static __device__ __forceinline__ void label_row(const float* xywhr, int row, float img_w, float img_h, float (&o)[NB]) {
        o[0] = xywhr[row * 5 + 0] * img_w;
        o[1] = xywhr[row * 5 + 1] * img_h;
        o[2] = xywhr[row * 5 + 2] * img_w;
        o[3] = xywhr[row * 5 + 3] * img_h;
        o[4] = xywhr[row * 5 + 4];
    }
    // decode: [B, A, 5] xywh in grid units, r
    static __device__ __forceinline__ void store_pred(const Args& a, const Side& s, float* pb) {
        const float r = a.angle[s.ia];
        float o[4];
        rbox_of(s.an, s.d, rot_of(r), o);
#pragma unroll
        for (int k = 0; k < 4; ++k) pb[s.ia * 5 + k] = o[k];
        pb[s.ia * 5 + 4] = r;
    }
    // loss: DFL against the target's UNROTATED extents, bbox2dist(anchor, xywh2xyxy(target xywh)) (loss.py:126, tal.py:391-394)
    static __device__ __forceinline__ void load(const float* tgt, int64_t ia, float (&tb)[NB]) {
#pragma unroll
        for (int k = 0; k < NB; ++k) tb[k] = tgt[ia * NB + k];
    }
    static __device__ __forceinline__ float edge(const Anchor& an, const float (&tb)[NB], int side) {
        return side == 0   ? an.ax - (tb[0] - tb[2] / 2)
               : side == 1 ? an.ay - (tb[1] - tb[3] / 2)
               : side == 2 ? (tb[0] + tb[2] / 2) - an.ax
                           : (tb[1] + tb[3] / 2) - an.ay;
    }
    // (sine, cosine, dist2rbox and the covariances are taken in foreground(), not for every anchor.  No dist_grad: the gradient kernel of the
    // oriented loss is obb_loss_kernel, see there)
    const Args& a;
    const Side& s;
    Rot q;
    float pbx[4];
    Cov pc, tc;
    __device__ __forceinline__ RotBox(const Args& a, const Side& s) : a(a), s(s) {}
    __device__ __forceinline__ void foreground(const float (&tb)[NB]) {
        q = rot_of(a.angle[s.ia]);
        rbox_of(s.an, s.d, q, pbx);
        pc = cov_of(pbx[2], pbx[3], q);
        tc = cov_of(tb[2], tb[3], rot_of(tb[4]));
    }
    __device__ __forceinline__ float overlap(const float (&tb)[NB]) const { return probiou_cov(pbx[0], pbx[1], pc, tb[0], tb[1], tc); }
};

// ---- targets: ragged (image, class, box) label rows -> dense [B, G, 1 + NB]; empty slots are zero -------------------------------------------
template <typename Box>
__global__ void targets_kernel(const float* __restrict__ batch_idx, const float* __restrict__ cls, const float* __restrict__ boxes, int n, int B, int G,
                               float img_w, float img_h, float* __restrict__ out) {
    constexpr int ROW = 1 + Box::NB;
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= B * G) return;
    const int b = t / G, slot = t - b * G;
    const int row = label_row_of(batch_idx, n, b, slot, [&](int i) { return Box::keep(boxes, i, img_w, img_h); });
    float box[Box::NB];
#pragma unroll
    for (int k = 0; k < Box::NB; ++k) box[k] = 0.f;
    if (row >= 0) Box::label_row(boxes, row, img_w, img_h, box);
    out[(int64_t)t * ROW] = row >= 0 ? cls[row] : 0.f;
#pragma unroll
    for (int k = 0; k < Box::NB; ++k) out[(int64_t)t * ROW + 1 + k] = box[k];
}

// ---- K1: DFL decode -> predicted boxes in grid units [B, A, NB] -------------------------------------------------------------------------------
template <typename T, typename Box>
__global__ __launch_bounds__(256) void decode_kernel(LossGeom g, float* __restrict__ pb, typename Box::Args ba) {
    Side s;
    float x[REG], p[REG];
    side_of<T>(g, s, x, p);
    if (s.live && s.side == 0) Box::store_pred(ba, s, pb);
}

// ---- inference decode: Detect._inference (head.py:103-142, non-export branch), Segment's (head.py:186-208) and OBB's (head.py:222-238) ------
// y[b][0:4][a] = the box in pixels: dist2bbox(DFL(box), anchor, xywh=True) * stride, or dist2rbox * stride ; y[b][4+c][a] = sigmoid(cls[c]) ;
// then the tail's rows.  Output is the reference's [B, 4 + nc + rows, A] float32 tensor (anchor index fastest).  Four lanes per anchor as in
// decode_kernel; the quad then walks the classes.  A-major stores: the 64 lanes of a wave cover 16 consecutive anchors of 4 rows each.
__device__ __forceinline__ void xywh_scaled(const float (&b)[4], float s, float (&o)[4]) {
    o[0] = (b[0] + b[2]) * 0.5f * s;
    o[1] = (b[1] + b[3]) * 0.5f * s;
    o[2] = (b[2] - b[0]) * s;
    o[3] = (b[3] - b[1]) * s;
}
__device__ __forceinline__ float axis_eval_row(const Side& s) {
    float xyxy[4], box[4];
    pred_box(s.an, s.d, xyxy);
    xywh_scaled(xyxy, s.an.s, box);
    return side_pick(s.side, box);
}
// A tail: how many rows follow the classes, this lane's box row, and the store of the tail rows at yt = the first of them.
struct NoTail {
    __device__ __forceinline__ int rows() const { return 0; }
    __device__ __forceinline__ float box_row(const Side& s) const { return axis_eval_row(s); }
    template <typename T> __device__ __forceinline__ void store(const Side&, float*, int64_t) const {}
};
struct MaskMaps {  // Segment: the anchor's nm mask coefficients, copied as they are from the per-level coefficient maps [B, H, W, nm]
    const void* mc[LOSS_MAXL];
    int64_t ld[LOSS_MAXL];
    int nm;
    __device__ __forceinline__ int rows() const { return nm; }
    __device__ __forceinline__ float box_row(const Side& s) const { return axis_eval_row(s); }
    template <typename T> __device__ __forceinline__ void store(const Side& s, float* yt, int64_t A) const {
        const T* mp = map_row<const T>(mc, ld, s.an);
        for (int c = s.side; c < nm; c += 4) yt[(int64_t)c * A] = to_f32(mp[c]);
    }
};
struct AngleTail {  // OBB: one row, the angle [B, A]; the box is the rotated one
    const float* angle;
    __device__ __forceinline__ int rows() const { return 1; }
    __device__ __forceinline__ float box_row(const Side& s) const {
        float o[4];
        rbox_of(s.an, s.d, rot_of(angle[s.ia]), o);
        return side_pick(s.side, o) * s.an.s;
    }
    template <typename T> __device__ __forceinline__ void store(const Side& s, float* yt, int64_t) const {
        if (s.side == 0) yt[0] = angle[s.ia];
    }
};
template <typename T, typename Tail>
__global__ __launch_bounds__(256) void infer_decode_kernel(LossGeom g, float* __restrict__ y, Tail tail) {
    Side s;
    float x[REG], p[REG];
    side_of<T>(g, s, x, p);
    if (!s.live) return;
    float* yo = y + (int64_t)s.b * (4 + g.nc + tail.rows()) * g.A + s.a;
    yo[(int64_t)s.side * g.A] = tail.box_row(s);
    const T* cp = map_row<const T>(g.cls, g.ldc, s.an);
    for (int c = s.side; c < g.nc; c += 4) yo[(int64_t)(4 + c) * g.A] = 1.0f / (1.0f + expf(-to_f32(cp[c])));
    tail.template store<T>(s, yo + (int64_t)(4 + g.nc) * g.A, g.A);
}

// ---- K2: alignment metric and overlaps for every (image, gt, anchor) (tal.py:118-160) -------------------------
template <typename T>
__global__ __launch_bounds__(256) void metric_kernel(LossGeom g, const float* __restrict__ targets, const float* __restrict__ pb,
                                                     float* __restrict__ ov, float* __restrict__ al, uint8_t* __restrict__ mpos, float alpha,
                                                     float beta) {
    const int b = blockIdx.y;
    const int a = blockIdx.x * 256 + threadIdx.x;
    if (a >= g.A) return;
    const Anchor an = anchor_of(g, b, a);
    const f32x4 pq = *reinterpret_cast<const f32x4*>(pb + ((int64_t)b * g.A + a) * 4);
    const float pd[4] = {pq[0] * an.s, pq[1] * an.s, pq[2] * an.s, pq[3] * an.s};
    const T* cp = map_row<const T>(g.cls, g.ldc, an);
    for (int k = 0; k < g.G; ++k) {
        const float* tg = gt_row(targets, (int64_t)b * g.G + k);
        float gt[4];
        gt_box(tg, gt);
        float o = 0.f, m = 0.f;
        if (gt_valid(gt) && centre_inside(an, gt)) {
            const float score = sigmoidf_(to_f32(cp[clamped_label(tg, g.nc)]));
            o = fmaxf(ciou(gt, pd), 0.f);
            // score^alpha * overlap^beta (reference alpha 0.5, beta 6.0): powf keeps other exponents exact too
            m = powf(score, alpha) * powf(o, beta);
        }
        const int64_t idx = ((int64_t)b * g.G + k) * g.A + a;
        ov[idx] = o;
        al[idx] = m;
        mpos[idx] = 0;
    }
}

// ... and of oriented boxes: the rotated inside test (its result is left in inm for the top-k kernel), probiou, the same metric
// (tal.py:329-361 RotatedTaskAlignedAssigner).  Two kernels, not one: a label's facts are worked out once per workgroup, 64 labels at a time, into LDS
// (its sine and cosine would otherwise be taken per anchor); the axis kernel has nothing worth staging, and staging there would change its code.
struct GtAux {
    float valid, x, y, ca, cb, cc;    // label?, centre, covariance
    float px, py, abx, aby, adx, ady;  // corner a, edge vectors ab and ad (tal.py:349-353)
    float nab, nad;
    int lab;
};
__device__ __forceinline__ GtAux gt_aux(const float* tg, int nc) {
    GtAux r;
    r.valid = obb_valid(tg) ? 1.f : 0.f;
    r.lab = clamped_label(tg, nc);
    r.x = tg[1];
    r.y = tg[2];
    const float w = tg[3], h = tg[4];
    const Rot q = rot_of(tg[5]);
    const Cov c = cov_of(w, h, q);
    r.ca = c.a;
    r.cb = c.b;
    r.cc = c.c;
    // xywhr2xyxyxyxy (utils/ops.py:573-601): pt1 = ctr + v1 + v2 (a), pt2 = ctr + v1 - v2 (b), pt4 = ctr - v1 + v2 (d)
    const float v1x = w / 2 * q.cs, v1y = w / 2 * q.sn, v2x = -h / 2 * q.sn, v2y = h / 2 * q.cs;
    const float ax = r.x + v1x + v2x, ay = r.y + v1y + v2y;
    const float bx = r.x + v1x - v2x, by = r.y + v1y - v2y;
    const float ex = r.x - v1x + v2x, ey = r.y - v1y + v2y;
    r.px = ax;
    r.py = ay;
    r.abx = bx - ax;
    r.aby = by - ay;
    r.adx = ex - ax;
    r.ady = ey - ay;
    r.nab = r.abx * r.abx + r.aby * r.aby;
    r.nad = r.adx * r.adx + r.ady * r.ady;
    return r;
}
template <typename T>
__global__ __launch_bounds__(256) void obb_metric_kernel(LossGeom g, const float* __restrict__ targets, const float* __restrict__ pb,
                                                         float* __restrict__ ov, float* __restrict__ al, uint8_t* __restrict__ mpos,
                                                         uint8_t* __restrict__ inm, float alpha, float beta) {
    __shared__ GtAux gs[64];
    const int b = blockIdx.y;
    const int a0 = blockIdx.x * 256 + threadIdx.x;
    const bool live = a0 < g.A;
    const int a = live ? a0 : 0;
    const Anchor an = anchor_of(g, b, a);
    const float* pr = pb + ((int64_t)b * g.A + a) * 5;
    const float px = pr[0] * an.s, py = pr[1] * an.s, pw = pr[2] * an.s, ph = pr[3] * an.s;
    const Cov pc = cov_of(pw, ph, rot_of(pr[4]));
    const float cx = an.ax * an.s, cy = an.ay * an.s;
    const T* cp = map_row<const T>(g.cls, g.ldc, an);
    for (int k0 = 0; k0 < g.G; k0 += 64) {
        __syncthreads();  // (the previous chunk's readers)
        if (threadIdx.x < 64 && k0 + (int)threadIdx.x < g.G) gs[threadIdx.x] = gt_aux(targets + ((int64_t)b * g.G + k0 + threadIdx.x) * OBB_ROW, g.nc);
        __syncthreads();
        const int kn = min(64, g.G - k0);
        for (int kk = 0; kk < kn; ++kk) {
            const GtAux& t = gs[kk];
            const float apx = cx - t.px, apy = cy - t.py;
            const float dab = apx * t.abx + apy * t.aby, dad = apx * t.adx + apy * t.ady;
            const bool in = t.valid != 0.f && dab >= 0.f && dab <= t.nab && dad >= 0.f && dad <= t.nad;  // an edge is inside (tal.py:361)
            float o = 0.f, m = 0.f;
            if (in) {
                const float score = sigmoidf_(to_f32(cp[t.lab]));
                o = fmaxf(probiou_cov(t.x, t.y, Cov{t.ca, t.cb, t.cc}, px, py, pc), 0.f);
                m = powf(score, alpha) * powf(o, beta);
            }
            if (live) {
                const int64_t idx = ((int64_t)b * g.G + k0 + kk) * g.A + a;
                ov[idx] = o;
                al[idx] = m;
                mpos[idx] = 0;
                inm[idx] = in ? 1 : 0;
            }
        }
    }
}

// ---- K3: top-k anchors per gt by alignment metric (tal.py:198-229); one workgroup per (image, gt) --------------
// the selection rule of one round: anchor a of value v is a candidate when it comes strictly after the previous pick in (value desc,
// index asc) order; the thread keeps its best candidate
__device__ __forceinline__ void topk_offer(Best& mine, const Best& prev, float v, int a) {
    const bool cand = v < prev.v || (v == prev.v && a > prev.i);
    if (cand) mine = better(mine, Best{v, a});
}
// What the scan asks of a gt: "is it a label", "is this anchor's centre inside it".  AxisGt: the xyxy row and centre_inside.  RotGt: the
// xywhr row and the inside mask obb_metric_kernel left.
struct AxisGt {
    float gt[4];
    __device__ __forceinline__ AxisGt(const LossGeom&, const float* targets, const uint8_t*, int bg) { gt_box(gt_row(targets, bg), gt); }
    __device__ __forceinline__ bool valid() const { return gt_valid(gt); }
    __device__ __forceinline__ bool inside(const LossGeom& g, int b, int a) const { return centre_inside(anchor_of(g, b, a), gt); }
};
struct RotGt {
    bool v;
    const uint8_t* in;
    __device__ __forceinline__ RotGt(const LossGeom& g, const float* targets, const uint8_t* inm, int bg)
        : v(obb_valid(targets + (int64_t)bg * OBB_ROW)), in(inm + (int64_t)bg * g.A) {}
    __device__ __forceinline__ bool valid() const { return v; }
    __device__ __forceinline__ bool inside(const LossGeom&, int, int a) const { return in[a] != 0; }
};
template <typename Gt>
__global__ __launch_bounds__(256) void topk_kernel(LossGeom g, const float* __restrict__ targets, const uint8_t* __restrict__ inm,
                                                   const float* __restrict__ al, uint8_t* __restrict__ mpos, int topk) {
    __shared__ Best sh[1][4];
    const int bg = blockIdx.x;
    const int b = bg / g.G;
    const Gt gt(g, targets, inm, bg);
    if (!gt.valid()) return;  // padding row: selects nothing (uniform across the block)
    const float* row = al + (int64_t)bg * g.A;
    Best prev{__builtin_inff(), -1};
    // the gt's metric row is read ONCE into registers when it fits (A <= 256 * TOPK_NV: 8400 anchors at 640x640 are 33 values per
    // thread); the k selection rounds then only scan registers.  (Ten passes over the row in L2 took 71 us of the 0.18 ms loss.)
    // A longer row (33600 anchors at 1280x1280) is scanned in memory every round.
    constexpr int TOPK_NV = 40;
    const bool inreg = g.A <= 256 * TOPK_NV;
    float vals[TOPK_NV];
    if (inreg) {
#pragma unroll
        for (int i = 0; i < TOPK_NV; ++i) {
            const int a = threadIdx.x + 256 * i;
            vals[i] = a < g.A ? row[a] : -__builtin_inff();  // (never beats the initial candidate of value -1)
        }
    }
    for (int r = 0; r < topk && r < g.A; ++r) {
        Best mine[1] = {Best{-1.0f, 0x7fffffff}};
        if (inreg) {
#pragma unroll
            for (int i = 0; i < TOPK_NV; ++i) topk_offer(mine[0], prev, vals[i], threadIdx.x + 256 * i);
        } else {
            for (int a = threadIdx.x; a < g.A; a += 256) topk_offer(mine[0], prev, row[a], a);
        }
        __syncthreads();  // (the previous round's readers of sh)
        block_combine<BestOp>(mine, sh);
        const Best win = mine[0];
        if (win.i == 0x7fffffff) break;
        if (threadIdx.x == 0 && gt.inside(g, b, win.i)) mpos[(int64_t)bg * g.A + win.i] = 1;
        prev = win;
    }
}

// ---- K4: one gt per anchor; an anchor claimed by several gts goes to the highest overlap (tal.py:305-327) -----
__global__ __launch_bounds__(256) void assign_kernel(LossGeom g, const float* __restrict__ ov, const uint8_t* __restrict__ mpos,
                                                     int* __restrict__ gidx) {
    const int b = blockIdx.y;
    const int a = blockIdx.x * 256 + threadIdx.x;
    if (a >= g.A) return;
    int cnt = 0, first = -1, best = 0;
    float bo = -1.0f;
    for (int k = 0; k < g.G; ++k) {
        const int64_t idx = ((int64_t)b * g.G + k) * g.A + a;
        if (mpos[idx]) {
            ++cnt;
            if (first < 0) first = k;
        }
        const float o = ov[idx];
        if (o > bo) {
            bo = o;
            best = k;
        }
    }
    gidx[(int64_t)b * g.A + a] = cnt > 1 ? best : first;
}

// ---- K5: per gt, the largest metric and overlap among the anchors assigned to it (tal.py:96-100) ---------------
__global__ __launch_bounds__(256) void posmax_kernel(LossGeom g, const float* __restrict__ ov, const float* __restrict__ al,
                                                     const int* __restrict__ gidx, float* __restrict__ pa, float* __restrict__ po) {
    __shared__ float sh[2][4];
    const int bg = blockIdx.x;
    const int b = bg / g.G, k = bg - b * g.G;
    float m[2] = {0.f, 0.f};  // metric, overlap
    for (int a = threadIdx.x; a < g.A; a += 256) {
        if (gidx[(int64_t)b * g.A + a] == k) {
            m[0] = fmaxf(m[0], al[(int64_t)bg * g.A + a]);
            m[1] = fmaxf(m[1], ov[(int64_t)bg * g.A + a]);
        }
    }
    block_combine<MaxOp>(m, sh);
    if (threadIdx.x == 0) {
        pa[bg] = m[0];
        po[bg] = m[1];
    }
}

// ---- K6: per anchor target box (grid units), weight (= sum of target scores) and label; partial sums of weight --
// NB values per box: 4 (xyxy) or 5 (xywhr: the angle is no length and keeps its value); the dense target rows hold the class in front of them
template <int NB>
__global__ __launch_bounds__(256) void finalize_kernel(LossGeom g, const float* __restrict__ targets, const float* __restrict__ al,
                                                       const int* __restrict__ gidx, const float* __restrict__ pa, const float* __restrict__ po,
                                                       float* __restrict__ tgt, float* __restrict__ wgt, int* __restrict__ lab,
                                                       float* __restrict__ tss_part) {
    __shared__ float sh[1][4];
    const int b = blockIdx.y;
    const int a = blockIdx.x * 256 + threadIdx.x;
    float w[1] = {0.f};
    if (a < g.A) {
        const int64_t ia = (int64_t)b * g.A + a;
        const int k = gidx[ia];
        float tb[NB];
#pragma unroll
        for (int i = 0; i < NB; ++i) tb[i] = 0.f;
        int lb = -1;
        if (k >= 0) {
            const int64_t bg = (int64_t)b * g.G + k;
            const float* tg = targets + bg * (NB + 1);
            const Anchor an = anchor_of(g, b, a);
            w[0] = al[bg * g.A + a] * po[bg] / (pa[bg] + TAL_EPS);
            lb = clamped_label(tg, g.nc);
#pragma unroll
            for (int i = 0; i < NB; ++i) tb[i] = i < 4 ? tg[1 + i] / an.s : tg[1 + i];
        }
        if constexpr (NB == 4) {
            Pack<float, 4>::store(tgt + ia * 4, tb);
        } else {
#pragma unroll
            for (int i = 0; i < NB; ++i) tgt[ia * NB + i] = tb[i];
        }
        wgt[ia] = w[0];
        lab[ia] = lb;
    }
    block_combine<SumOp>(w, sh);
    if (threadIdx.x == 0) tss_part[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = w[0];
}

// ---- K7: loss sums (GRAD = false) or gradients with respect to the maps (GRAD = true) --------------------------
// four lanes per anchor, one per box side; classes are strided over the four lanes.  box: (1 - Box's overlap(pred, target)) * weight;
// DFL and BCE are stated here for both box kinds (the gradients of the oriented loss: obb_loss_kernel, behind this kernel).
// DFL target of one side (loss.py:75-83): the edge clamped into the bins, its left bin and the two weights
struct DflTarget {
    int tl;
    float wl, wr;
};
__device__ __forceinline__ DflTarget dfl_target(float raw_t) {
    const float tt = fminf(fmaxf(raw_t, 0.f), (float)(REG - 1) - 0.01f);
    const int tl = (int)tt;
    const float wl = (float)(tl + 1) - tt;
    return DflTarget{tl, wl, 1.0f - wl};
}
// the side's DFL term: cross entropy against the two bins, a quarter of the weight each side
__device__ __forceinline__ float dfl_term(const float (&x)[REG], float lse, const DflTarget& t, float w) {
    float xl = 0.f, xr = 0.f;
#pragma unroll
    for (int j = 0; j < REG; ++j) {
        xl = j == t.tl ? x[j] : xl;
        xr = j == t.tl + 1 ? x[j] : xr;
    }
    return ((lse - xl) * t.wl + (lse - xr) * t.wr) * 0.25f * w;
}
// classification: BCE with logits against target score (label == c) * weight (loss.py:233) -> this lane's sum, or the gradient row with
// the padding channels of a padded gradient buffer zeroed (the consumer's weight-gradient GEMM reads them)
template <typename T, bool GRAD> __device__ __forceinline__ float class_branch(const LossGeom& g, const Side& s, int lb, float w, float g_cls) {
    float s_cls = 0.f;
    const T* cp = map_row<const T>(g.cls, g.ldc, s.an);
    for (int c = s.side; c < g.nc; c += 4) {
        const float xv = to_f32(cp[c]);
        const float tv = c == lb ? w : 0.f;
        if (!GRAD) s_cls += fmaxf(xv, 0.f) - xv * tv + log1pf(__expf(-fabsf(xv)));
        else map_row<T>(g.dcls, g.lddc, s.an)[c] = from_f32<T>((sigmoidf_(xv) - tv) * g_cls);
    }
    if (GRAD) {
        for (int c = g.nc + s.side; c < g.dcw; c += 4) map_row<T>(g.dcls, g.lddc, s.an)[c] = from_f32<T>(0.f);
    }
    return s_cls;
}
template <typename T, bool GRAD, typename Box>
__global__ __launch_bounds__(256) void loss_kernel(LossGeom g, const float* __restrict__ tgt, const float* __restrict__ wgt,
                                                   const int* __restrict__ lab, const float* __restrict__ scal, const float* __restrict__ gout,
                                                   const float* __restrict__ gscale, float* __restrict__ part, typename Box::Args ba) {
    __shared__ float sh[3][4];
    Side s;
    float x[REG], p[REG];
    side_of<T>(g, s, x, p);
    const Anchor& an = s.an;
    const int side = s.side;
    const float w = wgt[s.ia];
    const int lb = lab[s.ia];
    float tb[Box::NB];
    Box::load(tgt, s.ia, tb);
    Box box(ba, s);
    float s_box = 0.f, s_cls = 0.f, s_dfl = 0.f;
    const DflTarget t = dfl_target(Box::edge(an, tb, side));
    float g_box = 0.f, g_cls = 0.f, g_dfl = 0.f;
    if (GRAD) {
        const float inv_t = 1.0f / fmaxf(scal[0], 1.0f);
        g_box = gout[0] * (gscale ? gscale[0] : 1.0f) * inv_t;
        g_cls = gout[1] * (gscale ? gscale[1] : 1.0f) * inv_t;
        g_dfl = gout[2] * (gscale ? gscale[2] : 1.0f) * inv_t;
    }
    if (lb >= 0) {  // foreground anchor
        box.foreground(tb);
        if constexpr (!GRAD) {
            if (side == 0) s_box = (1.0f - box.overlap(tb)) * w;
            s_dfl = dfl_term(x, s.lse, t, w);
        } else {
            const float gd = box.dist_grad(tb, side) * w * g_box;
            const float kd = 0.25f * w * g_dfl;
            // (the row stands here: behind a function, in any form of its arguments, other products of it are fused in the gradient kernels -
            // profiles/loss_box_refactor_ab.txt)
            float o[REG];
#pragma unroll
            for (int j = 0; j < REG; ++j) {
                const float hot = (j == t.tl ? t.wl : 0.f) + (j == t.tl + 1 ? t.wr : 0.f);
                o[j] = gd * p[j] * ((float)j - s.e) + kd * (p[j] - hot);
            }
            if (s.live) store16<T>(map_row<T>(g.dbox, g.lddb, an) + side * REG, o);
        }
    } else if (GRAD && s.live) {
        float o[REG];
#pragma unroll
        for (int j = 0; j < REG; ++j) o[j] = 0.f;
        store16<T>(map_row<T>(g.dbox, g.lddb, an) + side * REG, o);
    }
    if (s.live) s_cls = class_branch<T, GRAD>(g, s, lb, w, g_cls);
    if (!GRAD) {
        if (!s.live) s_box = s_cls = s_dfl = 0.f;
        float sum[3] = {s_box, s_cls, s_dfl};  // (gathered here: summed in an array from the start, the other product of the DFL term is fused)
        block_combine<SumOp>(sum, sh);
        if (threadIdx.x == 0) {
#pragma unroll
            for (int k = 0; k < 3; ++k) part[(int64_t)blockIdx.x * 3 + k] = sum[k];
        }
    }
}

// ---- the gradients of the oriented loss with respect to the maps and the angle: loss_kernel<T, true, RotBox> is NOT instantiated ------------------
// Deliberately a kernel of its own, with the gradient branch of loss_kernel restated: with the rotated box gradient behind the policy the compiler fuses
// other products of this kernel (cov_grad's gB, then one more that was not found), in every form that was tried, and last bits of the float32 box
// gradients move (profiles/loss_box_refactor_ab.txt).  These statements compile to the text the kernel had before the sharing.
template <typename T>
__global__ __launch_bounds__(256) void obb_loss_kernel(LossGeom g, const float* __restrict__ angle, const float* __restrict__ tgt,
                                                       const float* __restrict__ wgt, const int* __restrict__ lab, const float* __restrict__ scal,
                                                       const float* __restrict__ gout, const float* __restrict__ gscale, float* __restrict__ dangle) {
    Side s;
    float x[REG], p[REG];
    side_of<T>(g, s, x, p);
    const Anchor& an = s.an;
    const int side = s.side;
    const float w = wgt[s.ia];
    const int lb = lab[s.ia];
    float tb[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) tb[k] = tgt[s.ia * 5 + k];
    const float raw_t = side == 0   ? an.ax - (tb[0] - tb[2] / 2)
                        : side == 1 ? an.ay - (tb[1] - tb[3] / 2)
                        : side == 2 ? (tb[0] + tb[2] / 2) - an.ax
                                    : (tb[1] + tb[3] / 2) - an.ay;
    const float tt = fminf(fmaxf(raw_t, 0.f), (float)(REG - 1) - 0.01f);
    const int tl = (int)tt;
    const float wl = (float)(tl + 1) - tt, wr = 1.0f - wl;
    const float inv_t = 1.0f / fmaxf(scal[0], 1.0f);
    const float g_box = gout[0] * (gscale ? gscale[0] : 1.0f) * inv_t;
    const float g_cls = gout[1] * (gscale ? gscale[1] : 1.0f) * inv_t;
    const float g_dfl = gout[2] * (gscale ? gscale[2] : 1.0f) * inv_t;
    if (lb >= 0) {  // foreground anchor
        const float r = angle[s.ia];
        const Rot q = rot_of(r);
        float pbx[4];
        rbox_of(an, s.d, q, pbx);
        const Cov pc = cov_of(pbx[2], pbx[3], q);
        const Cov tc = cov_of(tb[2], tb[3], rot_of(tb[4]));
        float gp[5], gw, gh, gr;
        (void)probiou_cov<true>(pbx[0], pbx[1], pc, tb[0], tb[1], tc, gp);
        cov_grad(pbx[2], pbx[3], q, pc, gp + 2, gw, gh, gr);
        // x = xf cs - yf sn + ax, y = xf sn + yf cs + ay with xf = (d2 - d0) / 2, yf = (d3 - d1) / 2; w = d0 + d2, h = d1 + d3
        const float gx = gp[0], gy = gp[1];
        const float gside = side == 0   ? -0.5f * (gx * q.cs + gy * q.sn) + gw
                            : side == 1 ? 0.5f * (gx * q.sn - gy * q.cs) + gh
                            : side == 2 ? 0.5f * (gx * q.cs + gy * q.sn) + gw
                                        : 0.5f * (gy * q.cs - gx * q.sn) + gh;
        const float gd = -gside * w * g_box;  // loss = (1 - probiou) * w
        const float kd = 0.25f * w * g_dfl;
        float o[REG];
#pragma unroll
        for (int j = 0; j < REG; ++j) {
            const float hot = (j == tl ? wl : 0.f) + (j == tl + 1 ? wr : 0.f);
            o[j] = gd * p[j] * ((float)j - s.e) + kd * (p[j] - hot);
        }
        if (s.live) store16<T>(map_row<T>(g.dbox, g.lddb, an) + side * REG, o);
        // the angle turns the centre about the anchor (d x / d r = -(y - ay), d y / d r = x - ax) and the covariance
        if (s.live && side == 0) dangle[s.ia] = -(gr - gx * (pbx[1] - an.ay) + gy * (pbx[0] - an.ax)) * w * g_box;
    } else if (s.live) {
        float o[REG];
#pragma unroll
        for (int j = 0; j < REG; ++j) o[j] = 0.f;
        store16<T>(map_row<T>(g.dbox, g.lddb, an) + side * REG, o);
        if (side == 0) dangle[s.ia] = 0.f;
    }
    if (s.live) {  // classification, as loss_kernel
        const T* cp = map_row<const T>(g.cls, g.ldc, an);
        for (int c = side; c < g.nc; c += 4) {
            const float xv = to_f32(cp[c]);
            const float tv = c == lb ? w : 0.f;
            map_row<T>(g.dcls, g.lddc, an)[c] = from_f32<T>((sigmoidf_(xv) - tv) * g_cls);
        }
        for (int c = g.nc + side; c < g.dcw; c += 4) map_row<T>(g.dcls, g.lddc, an)[c] = from_f32<T>(0.f);
    }
}

// ---- K8: fixed-order final sums: scal[0] = sum of target scores, loss[k] = sum_k / max(scal[0], 1) ------------
// out_scale (optional, [6]): loss[k] = raw_k * out_scale[k] and loss[3 + k] = raw_k * out_scale[3 + k] - the criterion's two results
// (loss * gains * batch for backward, loss * gains for logging: reference loss.py:250-255) without elementwise launches behind this one
// (a 256-wide tree in double precision over any number of partial rows: not a block_combine)
__global__ __launch_bounds__(256) void loss_final_kernel(const float* __restrict__ tss_part, int n_tss, const float* __restrict__ part, int n_part,
                                                         float* __restrict__ scal, float* __restrict__ loss, const float* __restrict__ out_scale) {
    __shared__ double sh[4][256];
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int i = threadIdx.x; i < n_tss; i += 256) acc[3] += (double)tss_part[i];
    for (int i = threadIdx.x; i < n_part; i += 256) {
        acc[0] += (double)part[(int64_t)i * 3 + 0];
        acc[1] += (double)part[(int64_t)i * 3 + 1];
        acc[2] += (double)part[(int64_t)i * 3 + 2];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) sh[k][threadIdx.x] = acc[k];
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
#pragma unroll
            for (int k = 0; k < 4; ++k) sh[k][threadIdx.x] += sh[k][threadIdx.x + o];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double tss = sh[3][0];
        const double den = tss > 1.0 ? tss : 1.0;
        scal[0] = (float)tss;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float raw = (float)(sh[k][0] / den);
            if (out_scale) {
                loss[k] = raw * out_scale[k];
                loss[3 + k] = raw * out_scale[3 + k];
            } else {
                loss[k] = raw;
            }
        }
    }
}

// ---- the OBB head's angle = (sigmoid(logit) - 0.25) * pi per anchor, in anchor order (head.py:225-227), and its gradient ------------------------
constexpr float PI_F = 3.14159265358979323846f;
struct AngleMaps {  // the one-channel angle logit maps [B, H, W, 1] (rows of padded buffers: a pixel stride) and their gradient maps
    const void* lg[LOSS_MAXL];
    void* dlg[LOSS_MAXL];
    int64_t ld[LOSS_MAXL], ldd[LOSS_MAXL];
    int dcw;  // channels of the gradient maps: the ones behind the first are written as zeros
};
template <typename T, bool GRAD>
__global__ __launch_bounds__(256) void obb_angle_kernel(LossGeom g, AngleMaps am, float* __restrict__ angle, const float* __restrict__ dangle) {
    const int b = blockIdx.y;
    const int a = blockIdx.x * 256 + threadIdx.x;
    if (a >= g.A) return;
    const Anchor an = anchor_of(g, b, a);
    const AngleMaps& cm = am;
    const float x = to_f32(*map_row<const T>(cm.lg, cm.ld, an));
    const float sg = 1.0f / (1.0f + expf(-x));
    const int64_t ia = (int64_t)b * g.A + a;
    if constexpr (!GRAD) {
        angle[ia] = (sg - 0.25f) * PI_F;
    } else {
        T* o = map_row<T>(cm.dlg, cm.ldd, an);
        o[0] = from_f32<T>(dangle[ia] * PI_F * (sg * (1.0f - sg)));
        for (int c = 1; c < am.dcw; ++c) o[c] = from_f32<T>(0.f);
    }
}

// ---- host: grids, buffer layouts, geometry -----------------------------------------------------------------------------------------------
// four lanes per anchor (decode_kernel, infer_decode_kernel, loss_kernel) / one thread per anchor, images along y (metric, assign, finalize)
dim3 quad_grid(int64_t B, int64_t A) { return dim3((unsigned)((B * A * 4 + 255) / 256)); }
dim3 anchor_grid(int64_t B, int64_t A) { return dim3((unsigned)((A + 255) / 256), (unsigned)B); }
template <typename... P, typename... Q> void launch(void (*kernel)(P...), dim3 grid, hipStream_t s, Q... args) {
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, s, args...);
}

struct Carve {
    char* p;
    size_t used;
    template <typename U> U* take(size_t n) {
        U* r = reinterpret_cast<U*>(p + used);
        used += (n * sizeof(U) + 255) / 256 * 256;
        return r;
    }
};

// what the forward leaves for the backward; the size is the carve of a null base
struct StateView {
    float *tgt, *wgt, *scal;
    int* lab;
    size_t bytes;
};
StateView carve_state(void* state, int64_t BA, int nb = 4) {
    Carve c{reinterpret_cast<char*>(state), 0};
    StateView v;
    v.tgt = c.take<float>((size_t)BA * nb);
    v.wgt = c.take<float>((size_t)BA);
    v.lab = c.take<int>((size_t)BA);
    v.scal = c.take<float>(4);
    v.bytes = c.used;
    return v;
}
// the forward's scratch buffers, likewise
struct WorkView {
    float *pb, *ov, *al;  // predicted boxes [B, A, 4] (oriented: [B, A, 5]); overlaps and alignment metric [B, G, A]
    uint8_t* mpos;        // positive mask [B, G, A]
    uint8_t* inm;         // oriented boxes only: "label, and the anchor's centre is inside it" [B, G, A]
    int* gidx;            // gt index per anchor [B, A]
    float *pa, *po;       // per-gt max metric and max overlap [B, G]
    float *tss_part, *part;  // partial sums: weights per finalize workgroup, (box, cls, dfl) per loss workgroup
    size_t bytes;
};
WorkView carve_work(void* workspace, int64_t B, int64_t A, int64_t G, int nb = 4) {
    const int64_t BA = B * A, BGA = BA * G, BG = B * G;
    Carve c{reinterpret_cast<char*>(workspace), 0};
    WorkView v;
    v.pb = c.take<float>((size_t)BA * nb);
    v.ov = c.take<float>((size_t)BGA);
    v.al = c.take<float>((size_t)BGA);
    v.mpos = c.take<uint8_t>((size_t)BGA);
    v.gidx = c.take<int>((size_t)BA);
    v.pa = c.take<float>((size_t)BG);
    v.po = c.take<float>((size_t)BG);
    v.tss_part = c.take<float>((size_t)(BA / 256 + B + 1));
    v.part = c.take<float>((size_t)(BA * 4 / 256 + 2) * 3);
    v.inm = nb == 5 ? c.take<uint8_t>((size_t)BGA) : nullptr;
    v.bytes = c.used;
    return v;
}

// the level walk: map sizes, anchor offsets (the entries past the last level hold A), batch and anchor count, from the maps that give the geometry
int walk_levels(LossGeom& g, int32_t nl, const ymi_tensor* maps, const float* strides, const char* what) {
    g.nl = nl;
    int64_t off = 0;
    for (int l = 0; l < nl; ++l) {
        g.H[l] = (int)maps[l].h;
        g.W[l] = (int)maps[l].w;
        g.off[l] = (int)off;
        g.stride[l] = strides ? strides[l] : 1.0f;
        off += maps[l].h * maps[l].w;
    }
    for (int l = nl; l <= LOSS_MAXL; ++l) g.off[l] = (int)off;
    g.B = (int)maps[0].n;
    g.A = (int)off;
    YMI_CHECK_ARG((int64_t)g.B * off < (1ll << 31), "%s: B*A < 2^31", what);
    return YMI_OK;
}
int fill_geom(LossGeom& g, int32_t nl, const ymi_tensor* box, const ymi_tensor* cls, const float* strides, const char* what) {
    YMI_CHECK_ARG(nl >= 1 && nl <= LOSS_MAXL && box && cls && strides, "%s: 1..%d levels", what, LOSS_MAXL);
    g = LossGeom{};
    for (int l = 0; l < nl; ++l) {
        YMI_CHECK_ARG(ymi_tensor_ok(&box[l]) && ymi_tensor_ok(&cls[l]), "%s: level %d tensors", what, l);
        YMI_CHECK_ARG(box[l].c == 4 * REG, "%s: box maps must have 4*16 channels (reg_max 16)", what);
        YMI_CHECK_ARG(box[l].n == box[0].n && cls[l].n == box[0].n && cls[l].h == box[l].h && cls[l].w == box[l].w && cls[l].c == cls[0].c &&
                          cls[l].dtype == box[0].dtype && box[l].dtype == box[0].dtype,
                      "%s: level %d shapes / dtypes", what, l);
        const int es = (int)ymi_esize(box[l].dtype);
        YMI_CHECK_ARG(((uintptr_t)box[l].data % 16) == 0 && (box[l].ld * es) % 16 == 0, "%s: box map alignment", what);
        g.box[l] = box[l].data;
        g.cls[l] = cls[l].data;
        g.ldb[l] = box[l].ld;
        g.ldc[l] = cls[l].ld;
    }
    g.nc = (int)cls[0].c;
    return walk_levels(g, nl, box, strides, what);
}
// the gradient maps of the backward: shaped as the maps; the class gradients may be wider (one width, dcw, for every level)
int fill_grad_geom(LossGeom& g, const ymi_tensor* box, const ymi_tensor* cls, const ymi_tensor* dbox, const ymi_tensor* dcls, const char* what) {
    YMI_CHECK_ARG(dbox && dcls && ymi_tensor_ok(&dcls[0]), "%s: gradient maps", what);
    g.dcw = (int)dcls[0].c;
    for (int l = 0; l < g.nl; ++l) {
        const ymi_tensor &db = dbox[l], &dc = dcls[l], &cm = cls[l];
        YMI_CHECK_ARG(ymi_tensor_ok(&db) && ymi_tensor_ok(&dc) && ymi_same_shape(&db, &box[l]) && dc.n == cm.n && dc.h == cm.h && dc.w == cm.w &&
                          dc.c >= cm.c && dc.c == g.dcw && db.dtype == box[l].dtype && dc.dtype == cm.dtype,
                      "%s: gradient map %d", what, l);
        const int es = (int)ymi_esize(db.dtype);
        YMI_CHECK_ARG(((uintptr_t)db.data % 16) == 0 && (db.ld * es) % 16 == 0, "%s: gradient map alignment", what);
        g.dbox[l] = db.data;
        g.dcls[l] = dc.data;
        g.lddb[l] = db.ld;
        g.lddc[l] = dc.ld;
    }
    return YMI_OK;
}
// geometry of the angle kernels: the logit maps alone give levels, sizes and anchor order
int fill_angle_geom(LossGeom& g, AngleMaps& am, int32_t nl, const ymi_tensor* maps, const char* what) {
    YMI_CHECK_ARG(nl >= 1 && nl <= LOSS_MAXL && maps, "%s: 1..%d levels", what, LOSS_MAXL);
    g = LossGeom{};
    am = AngleMaps{};
    for (int l = 0; l < nl; ++l) {
        const ymi_tensor& m = maps[l];
        YMI_CHECK_ARG(ymi_tensor_ok(&m) && m.c == 1 && m.n == maps[0].n && m.dtype == maps[0].dtype, "%s: level %d is a one-channel map of the batch", what, l);
        am.lg[l] = m.data;
        am.ld[l] = m.ld;
    }
    return walk_levels(g, nl, maps, nullptr, what);
}

// ---- host: the entry points' bodies, once for both box kinds (what: the entry point's name in error texts) -------------------------------------
template <typename Box>
int targets_impl(const char* what, const float* batch_idx, const float* cls, const float* boxes, int64_t n, int64_t batch, int64_t max_boxes, float img_w,
                 float img_h, float* out, void* stream) {
    YMI_CHECK_ARG(out && batch > 0 && max_boxes > 0 && n >= 0 && (n == 0 || (batch_idx && cls && boxes)), "%s: args", what);
    const int total = (int)(batch * max_boxes);
    hipLaunchKernelGGL(targets_kernel<Box>, dim3((total + 127) / 128), dim3(128), 0, (hipStream_t)stream, batch_idx, cls, boxes, (int)n, (int)batch,
                       (int)max_boxes, img_w, img_h, out);
    YMI_CHECK_LAUNCH(what);
    return YMI_OK;
}

int loss_sizes_impl(int nb, const char* what, int64_t batch, int64_t anchors, int64_t max_boxes, size_t* state_bytes, size_t* workspace_bytes) {
    YMI_CHECK_ARG(batch > 0 && anchors > 0 && max_boxes > 0 && state_bytes && workspace_bytes, "%s: args", what);
    *state_bytes = carve_state(nullptr, batch * anchors, nb).bytes;
    *workspace_bytes = carve_work(nullptr, batch, anchors, max_boxes, nb).bytes;
    return YMI_OK;
}

// the forward's eight launches.  gidx_out (optional, [B, A] int32): the assignment's gt index per anchor (-1: background) is written there
// instead of into the workspace, for a stage that follows the detection loss (the mask loss of seg.hip); everything computed is the same
template <typename Box>
int loss_fwd_impl(const char* what, typename Box::Args ba, int32_t nl, const ymi_tensor* box_maps, const ymi_tensor* cls_maps, const float* strides,
                  const float* targets, int64_t max_boxes, int32_t topk, float alpha, float beta, const float* out_scale, float* loss_out, void* state,
                  size_t state_bytes, void* workspace, size_t workspace_bytes, int32_t* gidx_out, void* stream) {
    LossGeom g;
    int rc = fill_geom(g, nl, box_maps, cls_maps, strides, what);
    if (rc) return rc;
    g.G = (int)max_boxes;
    YMI_CHECK_ARG(max_boxes >= 1 && (int64_t)g.B * g.G * g.A < (1ll << 31), "%s: max_boxes >= 1 and B*G*A < 2^31", what);
    YMI_CHECK_ARG(Box::args_ok(ba) && targets && loss_out && state && workspace && topk >= 1, "%s: null argument", what);
    const StateView st = carve_state(state, (int64_t)g.B * g.A, Box::NB);
    WorkView w = carve_work(workspace, g.B, g.A, g.G, Box::NB);
    if (gidx_out) w.gidx = gidx_out;
    if (state_bytes < st.bytes || workspace_bytes < w.bytes) {
        ymi_set_error("%s: state %zu < %zu or workspace %zu < %zu bytes", what, state_bytes, st.bytes, workspace_bytes, w.bytes);
        return YMI_EWORKSPACE;
    }
    hipStream_t s = (hipStream_t)stream;
    const dim3 qgrid = quad_grid(g.B, g.A), agrid = anchor_grid(g.B, g.A), ggrid((unsigned)(g.B * g.G));
    dispatch_dtype(box_maps[0].dtype, [&](auto t) {
        typedef typename decltype(t)::type T;
        launch(decode_kernel<T, Box>, qgrid, s, g, w.pb, ba);
        if constexpr (Box::NB == 4) launch(metric_kernel<T>, agrid, s, g, targets, w.pb, w.ov, w.al, w.mpos, alpha, beta);
        else launch(obb_metric_kernel<T>, agrid, s, g, targets, w.pb, w.ov, w.al, w.mpos, w.inm, alpha, beta);
        launch(topk_kernel<typename Box::Gt>, ggrid, s, g, targets, (const uint8_t*)w.inm, w.al, w.mpos, (int)topk);
        launch(assign_kernel, agrid, s, g, w.ov, w.mpos, w.gidx);
        launch(posmax_kernel, ggrid, s, g, w.ov, w.al, w.gidx, w.pa, w.po);
        launch(finalize_kernel<Box::NB>, agrid, s, g, targets, w.al, w.gidx, w.pa, w.po, st.tgt, st.wgt, st.lab, w.tss_part);
        launch(loss_kernel<T, false, Box>, qgrid, s, g, st.tgt, st.wgt, st.lab, st.scal, nullptr, nullptr, w.part, ba);
        launch(loss_final_kernel, dim3(1), s, w.tss_part, (int)(agrid.x * agrid.y), w.part, (int)qgrid.x, st.scal, loss_out, out_scale);
    });
    YMI_CHECK_LAUNCH(what);
    return YMI_OK;
}

template <typename Box>
int loss_bwd_impl(const char* what, typename Box::Args ba, float* dangle, int32_t nl, const ymi_tensor* box_maps, const ymi_tensor* cls_maps, const float* strides,
                  const void* state, size_t state_bytes, const float* grad_loss, const float* grad_scale, const ymi_tensor* dbox_maps,
                  const ymi_tensor* dcls_maps, void* stream) {
    LossGeom g;
    int rc = fill_geom(g, nl, box_maps, cls_maps, strides, what);
    if (rc) return rc;
    YMI_CHECK_ARG(Box::args_ok(ba) && (dangle || Box::NB == 4) && state && grad_loss && dbox_maps && dcls_maps, "%s: null argument", what);
    const StateView st = carve_state(const_cast<void*>(state), (int64_t)g.B * g.A, Box::NB);
    YMI_CHECK_ARG(state_bytes >= st.bytes, "%s: state too small", what);
    rc = fill_grad_geom(g, box_maps, cls_maps, dbox_maps, dcls_maps, what);
    if (rc) return rc;
    dispatch_dtype(box_maps[0].dtype, [&](auto t) {
        typedef typename decltype(t)::type T;
        const dim3 qgrid = quad_grid(g.B, g.A);
        hipStream_t s = (hipStream_t)stream;
        if constexpr (Box::NB == 4) launch(loss_kernel<T, true, Box>, qgrid, s, g, st.tgt, st.wgt, st.lab, st.scal, grad_loss, grad_scale, nullptr, ba);
        else launch(obb_loss_kernel<T>, qgrid, s, g, ba.angle, st.tgt, st.wgt, st.lab, st.scal, grad_loss, grad_scale, dangle);
    });
    YMI_CHECK_LAUNCH(what);
    return YMI_OK;
}

// the eval decodes.  have: the entry point's own pointers are there (`missing` names them in the refusal); fill(tail): the tail's maps, checked
// once the geometry stands
template <typename Tail, typename Fill>
int decode_impl(const char* what, bool have, const char* missing, int32_t nl, const ymi_tensor* box_maps, const ymi_tensor* cls_maps, const float* strides,
                float* y, void* stream, Fill fill) {
    LossGeom g;
    int rc = fill_geom(g, nl, box_maps, cls_maps, strides, what);
    if (rc) return rc;
    YMI_CHECK_ARG(y && have, "%s: null %s", what, missing);
    Tail tail{};
    rc = fill(tail);
    if (rc) return rc;
    dispatch_dtype(box_maps[0].dtype,
                   [&](auto t) { launch(infer_decode_kernel<typename decltype(t)::type, Tail>, quad_grid(g.B, g.A), (hipStream_t)stream, g, y, tail); });
    YMI_CHECK_LAUNCH(what);
    return YMI_OK;
}
int fill_mask_maps(MaskMaps& mm, int32_t nl, const ymi_tensor* box_maps, const ymi_tensor* mc_maps) {
    mm.nm = (int)mc_maps[0].c;
    for (int l = 0; l < nl; ++l) {
        const ymi_tensor& m = mc_maps[l];
        YMI_CHECK_ARG(ymi_tensor_ok(&m) && m.n == box_maps[l].n && m.h == box_maps[l].h && m.w == box_maps[l].w && m.c == mm.nm && m.dtype == box_maps[0].dtype,
                      "detect_decode_seg: coefficient map %d", l);
        mm.mc[l] = m.data;
        mm.ld[l] = m.ld;
    }
    return YMI_OK;
}
}  // namespace

extern "C" int ymi_detect_targets(const float* batch_idx, const float* cls, const float* bboxes_xywhn, int64_t n, int64_t batch, int64_t max_boxes,
                                  float img_w, float img_h, float* out, void* stream) {
    return targets_impl<AxisBox>("detect_targets", batch_idx, cls, bboxes_xywhn, n, batch, max_boxes, img_w, img_h, out, stream);
}
extern "C" int ymi_obb_targets(const float* batch_idx, const float* cls, const float* bboxes_xywhr, int64_t n, int64_t batch, int64_t max_boxes,
                               float img_w, float img_h, float* out, void* stream) {
    return targets_impl<RotBox>("obb_targets", batch_idx, cls, bboxes_xywhr, n, batch, max_boxes, img_w, img_h, out, stream);
}

extern "C" int ymi_detect_loss_sizes(int64_t batch, int64_t anchors, int64_t max_boxes, size_t* state_bytes, size_t* workspace_bytes) {
    return loss_sizes_impl(AxisBox::NB, "detect_loss_sizes", batch, anchors, max_boxes, state_bytes, workspace_bytes);
}
extern "C" int ymi_obb_loss_sizes(int64_t batch, int64_t anchors, int64_t max_boxes, size_t* state_bytes, size_t* workspace_bytes) {
    return loss_sizes_impl(RotBox::NB, "obb_loss_sizes", batch, anchors, max_boxes, state_bytes, workspace_bytes);
}

extern "C" int ymi_detect_loss_fwd_assign(int32_t nl, const ymi_tensor* box_maps, const ymi_tensor* cls_maps, const float* strides, const float* targets,
                                          int64_t max_boxes, int32_t topk, float alpha, float beta, const float* out_scale, float* loss_out, void* state,
                                          size_t state_bytes, void* workspace, size_t workspace_bytes, int32_t* gidx_out, void* stream) {
    return loss_fwd_impl<AxisBox>("detect_loss_fwd", AxisBox::Args{}, nl, box_maps, cls_maps, strides, targets, max_boxes, topk, alpha, beta, out_scale,
                                  loss_out, state, state_bytes, workspace, workspace_bytes, gidx_out, stream);
}
extern "C" int ymi_detect_loss_fwd(int32_t nl, const ymi_tensor* box_maps, const ymi_tensor* cls_maps, const float* strides, const float* targets,
                                   int64_t max_boxes, int32_t topk, float alpha, float beta, const float* out_scale, float* loss_out, void* state,
                                   size_t state_bytes, void* workspace, size_t workspace_bytes, void* stream) {
    return ymi_detect_loss_fwd_assign(nl, box_maps, cls_maps, strides, targets, max_boxes, topk, alpha, beta, out_scale, loss_out, state, state_bytes,
                                      workspace, workspace_bytes, nullptr, stream);
}
extern "C" int ymi_obb_loss_fwd(int32_t nl, const ymi_tensor* box_maps, const ymi_tensor* cls_maps, const float* angle, const float* strides,
                                const float* targets, int64_t max_boxes, int32_t topk, float alpha, float beta, const float* out_scale, float* loss_out,
                                void* state, size_t state_bytes, void* workspace, size_t workspace_bytes, void* stream) {
    return loss_fwd_impl<RotBox>("obb_loss_fwd", RotBox::Args{angle}, nl, box_maps, cls_maps, strides, targets, max_boxes, topk, alpha, beta,
                                 out_scale, loss_out, state, state_bytes, workspace, workspace_bytes, nullptr, stream);
}

extern "C" int ymi_detect_loss_bwd(int32_t nl, const ymi_tensor* box_maps, const ymi_tensor* cls_maps, const float* strides, const void* state,
                                   size_t state_bytes, const float* grad_loss, const float* grad_scale, const ymi_tensor* dbox_maps, const ymi_tensor* dcls_maps,
                                   void* stream) {
    return loss_bwd_impl<AxisBox>("detect_loss_bwd", AxisBox::Args{}, nullptr, nl, box_maps, cls_maps, strides, state, state_bytes, grad_loss, grad_scale, dbox_maps,
                                  dcls_maps, stream);
}
extern "C" int ymi_obb_loss_bwd(int32_t nl, const ymi_tensor* box_maps, const ymi_tensor* cls_maps, const float* angle, const float* strides,
                                const void* state, size_t state_bytes, const float* grad_loss, const float* grad_scale, const ymi_tensor* dbox_maps,
                                const ymi_tensor* dcls_maps, float* dangle, void* stream) {
    return loss_bwd_impl<RotBox>("obb_loss_bwd", RotBox::Args{angle}, dangle, nl, box_maps, cls_maps, strides, state, state_bytes, grad_loss, grad_scale,
                                 dbox_maps, dcls_maps, stream);
}

extern "C" int ymi_detect_decode(int32_t nl, const ymi_tensor* box_maps, const ymi_tensor* cls_maps, const float* strides, float* y, void* stream) {
    return decode_impl<NoTail>("detect_decode", true, "output", nl, box_maps, cls_maps, strides, y, stream, [](NoTail&) { return (int)YMI_OK; });
}
extern "C" int ymi_detect_decode_seg(int32_t nl, const ymi_tensor* box_maps, const ymi_tensor* cls_maps, const ymi_tensor* mc_maps, const float* strides,
                                     float* y, void* stream) {
    return decode_impl<MaskMaps>("detect_decode_seg", mc_maps != nullptr, "argument", nl, box_maps, cls_maps, strides, y, stream,
                                 [&](MaskMaps& mm) { return fill_mask_maps(mm, nl, box_maps, mc_maps); });
}
extern "C" int ymi_detect_decode_obb(int32_t nl, const ymi_tensor* box_maps, const ymi_tensor* cls_maps, const float* angle, const float* strides,
                                     float* y, void* stream) {
    return decode_impl<AngleTail>("detect_decode_obb", angle != nullptr, "argument", nl, box_maps, cls_maps, strides, y, stream, [&](AngleTail& t) {
        t.angle = angle;
        return (int)YMI_OK;
    });
}

extern "C" int ymi_obb_angle_fwd(int32_t nl, const ymi_tensor* logit_maps, float* angle, void* stream) {
    LossGeom g;
    AngleMaps am;
    int rc = fill_angle_geom(g, am, nl, logit_maps, "obb_angle_fwd");
    if (rc) return rc;
    YMI_CHECK_ARG(angle, "obb_angle_fwd: null output");
    dispatch_dtype(logit_maps[0].dtype, [&](auto t) {
        launch(obb_angle_kernel<typename decltype(t)::type, false>, anchor_grid(g.B, g.A), (hipStream_t)stream, g, am, angle, (const float*)nullptr);
    });
    YMI_CHECK_LAUNCH("obb_angle_fwd");
    return YMI_OK;
}

extern "C" int ymi_obb_angle_bwd(int32_t nl, const ymi_tensor* logit_maps, const float* dangle, const ymi_tensor* dlogit_maps, void* stream) {
    LossGeom g;
    AngleMaps am;
    int rc = fill_angle_geom(g, am, nl, logit_maps, "obb_angle_bwd");
    if (rc) return rc;
    YMI_CHECK_ARG(dangle && dlogit_maps && ymi_tensor_ok(&dlogit_maps[0]), "obb_angle_bwd: null argument");
    am.dcw = (int)dlogit_maps[0].c;
    for (int l = 0; l < nl; ++l) {
        const ymi_tensor &d = dlogit_maps[l], &m = logit_maps[l];
        YMI_CHECK_ARG(ymi_tensor_ok(&d) && d.n == m.n && d.h == m.h && d.w == m.w && d.c >= 1 && d.c == am.dcw && d.dtype == m.dtype,
                      "obb_angle_bwd: gradient map %d", l);
        am.dlg[l] = d.data;
        am.ldd[l] = d.ld;
    }
    dispatch_dtype(logit_maps[0].dtype, [&](auto t) {
        launch(obb_angle_kernel<typename decltype(t)::type, true>, anchor_grid(g.B, g.A), (hipStream_t)stream, g, am, (float*)nullptr, dangle);
    });
    YMI_CHECK_LAUNCH("obb_angle_bwd");
    return YMI_OK;
}
