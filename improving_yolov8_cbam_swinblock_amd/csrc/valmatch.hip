// Validation statistics on the device: what models/yolo/detect/val.py:174-216 does per image after NMS - the label boxes in pixels (or native
// pixels), box_iou, BaseValidator.match_predictions over all IoU levels, ConfusionMatrix.process_batch - as ONE launch of one workgroup per image
// on det / count as ymi_detect_nms / ymi_scale_boxes leave them and the batch's label table (include/ymi.h: ymi_val_match states every step).
//   pass 1 : the label table goes through LDS in chunks of YMI_VALMATCH_CHUNK rows; the image's own rows are compacted in table order (ballot +
//            wave totals) with their boxes already in pixels; every detection (thread-strided) walks the chunk and keeps, in LDS, the label it
//            claims for tp (largest iou * same_class, first maximum) and the one it claims for the confusion matrix (largest iou)
//   pass 2 : one O(n^2) walk over claim[] / strength[] in LDS gives tp at every level; a second one names the detection that holds each label
//   pass 3 : the table once more, chunk by chunk: labels no detection claims are counted as missed
// No workspace, no allocation, no synchronisation; the only atomics are integer adds into cm, so every result is a function of the input alone.
// This file is compiled with -ffp-contract=off (Makefile): (area_gt + area_pred) - inter + 1e-7f and (cx - w / 2) * W must round one
// operation at a time, as the host path's torch statements do.  Division is the compiler's IEEE sequence.
#include "common.h"

namespace {

constexpr int VM_THREADS = 1024;
constexpr int VM_WAVES = VM_THREADS / YMI_WAVE;
constexpr int VM_CHUNK = YMI_VALMATCH_CHUNK;  // label rows staged at a time: one per thread
constexpr int VM_MAX_DET = 2048;              // detections whose claims are held in LDS (16 bytes each)
static_assert(VM_CHUNK == VM_THREADS, "the staging gives every thread one label row of the chunk");

struct Levels {
    float v[YMI_VALMATCH_MAX_LEVELS];
};

// class id of a float class column (the reference's .int(): truncation) or -1 when it lies outside [0, nc)
__device__ __forceinline__ int class_index(float c, int nc) { return (c > -1.0f && c < (float)nc) ? (int)c : -1; }

// the overlap source of ymi_val_match_masks: the integer counts ymi_mask_overlap leaves (bin j + 1 belongs to the image's j-th label in table order)
struct MaskCounts {
    const int* inter;      // [B][max_det][n_bins]
    const int* area_pred;  // [B][max_det]
    const int* area_gt;    // [B][n_bins]
    int n_bins;
};

// MASKS = false: the overlap of a detection with a label is box_iou of their boxes; true: mask_iou on the counts of `mc` (lab_box, img_w, img_h, native
// and cm are not read: the confusion matrix is box-based).  Everything else - staging, claims, ties, levels - is the one body below.
template <bool MASKS>
__global__ __launch_bounds__(VM_THREADS) void val_match_kernel(const float* __restrict__ det, const int* __restrict__ count, int max_det,
                                                               const int* __restrict__ lab_img, const float* __restrict__ lab_cls,
                                                               const float* __restrict__ lab_box, int n_labels, float img_w, float img_h,
                                                               const float* __restrict__ native, Levels levels, int n_levels, int single_cls,
                                                               uint8_t* __restrict__ tp, int* __restrict__ cm, int nc, float cm_conf, float cm_iou,
                                                               MaskCounts mc) {
    __shared__ float lx1[VM_CHUNK], ly1[VM_CHUNK], lx2[VM_CHUNK], ly2[VM_CHUNK], lar[VM_CHUNK], lcl[VM_CHUNK];  // the image's labels of this chunk
    __shared__ int lid[VM_CHUNK];                                  // their rows in the table (pass 3: the chunk's claimed flags)
    __shared__ int claim[VM_MAX_DET], cclaim[VM_MAX_DET];          // per detection: table row claimed for tp / for the matrix (-1: none)
    __shared__ float strength[VM_MAX_DET], ciou[VM_MAX_DET];       // ... and the overlap it was claimed with
    __shared__ int wtot[VM_WAVES];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & (YMI_WAVE - 1), wave = tid / YMI_WAVE;
    const float* db = det + (size_t)b * max_det * 6;
    uint8_t* tb = tp + (size_t)b * max_det * n_levels;
    int n = count[b];
    n = n < 0 ? 0 : n > max_det ? max_det : n;
    float gain = 1.0f, pad_x = 0.0f, pad_y = 0.0f, w0 = 0.0f, h0 = 0.0f;
    if (native) {
        const float* p = native + (size_t)b * 5;
        gain = p[0], pad_x = p[1], pad_y = p[2], w0 = p[3], h0 = p[4];
    }
    for (int d = tid; d < n; d += VM_THREADS) {
        claim[d] = cclaim[d] = -1;
        strength[d] = ciou[d] = 0.0f;
    }

    // ---- pass 1 ----
    int n_mine = 0;  // labels of this image so far (workgroup-uniform)
    for (int l0 = 0; l0 < n_labels; l0 += VM_CHUNK) {
        const int l = l0 + tid;
        const bool mine = l < n_labels && lab_img[l] == b;
        const uint64_t vote = __ballot(mine);
        __syncthreads();  // the chunk before this one has been read
        if (lane == 0) wtot[wave] = __popcll(vote);
        __syncthreads();
        int pos = __popcll(vote & (((uint64_t)1 << lane) - 1)), total = 0;
        for (int w = 0; w < VM_WAVES; ++w) {
            const int t = wtot[w];
            if (w < wave) pos += t;
            total += t;
        }
        if (MASKS) {
            if (mine) {
                lcl[pos] = single_cls ? 0.0f : lab_cls[l];
                lid[pos] = l;
            }
        } else if (mine) {
            const float* q = lab_box + (size_t)l * 4;
            const float hw = q[2] / 2.0f, hh = q[3] / 2.0f;
            float x1 = (q[0] - hw) * img_w, y1 = (q[1] - hh) * img_h, x2 = (q[0] + hw) * img_w, y2 = (q[1] + hh) * img_h;
            if (native) {
                x1 = fminf(fmaxf((x1 - pad_x) / gain, 0.0f), w0);
                y1 = fminf(fmaxf((y1 - pad_y) / gain, 0.0f), h0);
                x2 = fminf(fmaxf((x2 - pad_x) / gain, 0.0f), w0);
                y2 = fminf(fmaxf((y2 - pad_y) / gain, 0.0f), h0);
            }
            lx1[pos] = x1, ly1[pos] = y1, lx2[pos] = x2, ly2[pos] = y2;
            lar[pos] = (x2 - x1) * (y2 - y1);
            lcl[pos] = single_cls ? 0.0f : lab_cls[l];
            lid[pos] = l;
        }
        __syncthreads();
        for (int d = tid; d < n; d += VM_THREADS) {
            const float* p = db + (size_t)d * 6;
            const float px1 = p[0], py1 = p[1], px2 = p[2], py2 = p[3], pcl = single_cls ? 0.0f : p[5];
            const float par = MASKS ? (float)mc.area_pred[(size_t)b * max_det + d] : (px2 - px1) * (py2 - py1);
            const int* irow = MASKS ? mc.inter + ((size_t)b * max_det + d) * mc.n_bins : nullptr;
            int c = claim[d], cc = cclaim[d];
            float s = strength[d], ci = ciou[d];
            for (int j = 0; j < total; ++j) {
                float iou = 0.0f;
                if (MASKS) {  // mask_iou on integer counts; labels at or beyond n_bins - 1 overlap nothing
                    const int bin = n_mine + j + 1;
                    if (bin < mc.n_bins) {
                        const float inter = (float)irow[bin];
                        iou = inter / ((((float)mc.area_gt[(size_t)b * mc.n_bins + bin] + par) - inter) + 1e-7f);
                    }
                } else {
                    const float w = fmaxf(fminf(lx2[j], px2) - fmaxf(lx1[j], px1), 0.0f), h = fmaxf(fminf(ly2[j], py2) - fmaxf(ly1[j], py1), 0.0f);
                    const float inter = w * h;
                    iou = inter / (((lar[j] + par) - inter) + 1e-7f);
                }
                const float ov = iou * (lcl[j] == pcl ? 1.0f : 0.0f);
                if (c < 0 || ov > s) {  // strict: the first maximum in table order
                    s = ov;
                    c = lid[j];
                }
                if (cc < 0 || iou > ci) {
                    ci = iou;
                    cc = lid[j];
                }
            }
            claim[d] = c, cclaim[d] = cc, strength[d] = s, ciou[d] = ci;
        }
        n_mine += total;
    }
    // matrix claims: only detections above cm_conf take part, and only with an overlap above cm_iou
    for (int d = tid; d < n; d += VM_THREADS)
        if (!cm || !(db[(size_t)d * 6 + 4] > cm_conf) || !(ciou[d] > cm_iou)) cclaim[d] = -1;
    __syncthreads();

    // ---- pass 2 ----
    for (int d = tid; d < max_det; d += VM_THREADS) {
        uint8_t* row = tb + (size_t)d * n_levels;
        if (d >= n || n_mine == 0) {
            for (int t = 0; t < n_levels; ++t) row[t] = 0;
            continue;
        }
        const int c = claim[d];
        const float s = strength[d];
        float m = -INFINITY;  // the largest strength among better-ranked detections with the same claim
        for (int e = 0; e < d; ++e)
            if (claim[e] == c) m = fmaxf(m, strength[e]);
        for (int t = 0; t < n_levels; ++t) row[t] = (s >= levels.v[t] && !(m >= levels.v[t])) ? 1 : 0;
    }
    if (!cm) return;  // (workgroup-uniform)
    const int ld = nc + 1;
    for (int d = tid; d < n; d += VM_THREADS) {
        const float* p = db + (size_t)d * 6;
        if (!(p[4] > cm_conf)) continue;
        const int dc = single_cls ? 0 : class_index(p[5], nc);
        const int c = cclaim[d];
        bool holds = c >= 0;
        if (holds) {  // a label goes to the claimant with the largest iou; equal: the lower detection index
            const float ci = ciou[d];
            for (int e = 0; e < n; ++e)
                if (cclaim[e] == c && (ciou[e] > ci || (ciou[e] == ci && e < d))) holds = false;
        }
        if (dc < 0) continue;
        if (holds) {
            const int gc = single_cls ? 0 : class_index(lab_cls[c], nc);
            if (gc >= 0) atomicAdd(&cm[dc * ld + gc], 1);
        } else {
            atomicAdd(&cm[dc * ld + nc], 1);
        }
    }

    // ---- pass 3 ----
    for (int l0 = 0; l0 < n_labels; l0 += VM_CHUNK) {
        __syncthreads();
        lid[tid] = 0;
        __syncthreads();
        for (int d = tid; d < n; d += VM_THREADS) {
            const int c = cclaim[d];
            if (c >= l0 && c - l0 < VM_CHUNK) lid[c - l0] = 1;  // (several detections may store the same 1)
        }
        __syncthreads();
        const int l = l0 + tid;
        if (l < n_labels && lab_img[l] == b && !lid[tid]) {
            const int gc = single_cls ? 0 : class_index(lab_cls[l], nc);
            if (gc >= 0) atomicAdd(&cm[nc * ld + gc], 1);
        }
    }
}

}  // namespace

extern "C" int ymi_val_match(const float* det, const int32_t* count, int64_t batch, int64_t max_det, const int32_t* lab_img, const float* lab_cls,
                             const float* lab_box, int64_t n_labels, float img_w, float img_h, const float* native, const float* levels,
                             int32_t n_levels, int32_t single_cls, uint8_t* tp, int32_t* cm, int64_t nc, float cm_conf, float cm_iou, void* stream) {
    YMI_CHECK_ARG(batch > 0 && batch < ((int64_t)1 << 31), "val_match: bad batch");
    YMI_CHECK_ARG(max_det > 0 && max_det <= VM_MAX_DET, "val_match: max_det in [1, %d]", VM_MAX_DET);
    YMI_CHECK_ARG(levels && n_levels > 0 && n_levels <= YMI_VALMATCH_MAX_LEVELS, "val_match: 1 to %d IoU levels", YMI_VALMATCH_MAX_LEVELS);
    YMI_CHECK_ARG(n_labels >= 0 && n_labels < ((int64_t)1 << 31) - VM_CHUNK, "val_match: the label table must have fewer than 2^31 rows");
    YMI_CHECK_ARG(det && count && tp, "val_match: null pointer");
    YMI_CHECK_ARG(n_labels == 0 || (lab_img && lab_cls && lab_box), "val_match: null label table");
    YMI_CHECK_ARG(img_w > 0.0f && img_h > 0.0f, "val_match: bad image size");
    YMI_CHECK_ARG(!cm || (nc > 0 && nc <= 32767), "val_match: the confusion matrix takes nc in [1, 32767]");
    if (((uintptr_t)det & 3) || ((uintptr_t)count & 3) || ((uintptr_t)lab_img & 3) || ((uintptr_t)lab_cls & 3) || ((uintptr_t)lab_box & 3) ||
        ((uintptr_t)native & 3) || ((uintptr_t)cm & 3)) {
        ymi_set_error("val_match: det / count / labels / native / cm need 4-byte alignment");
        return YMI_EALIGN;
    }
    Levels lv = {};
    for (int i = 0; i < n_levels; ++i) lv.v[i] = levels[i];
    hipLaunchKernelGGL(val_match_kernel<false>, dim3((unsigned)batch), dim3(VM_THREADS), 0, (hipStream_t)stream, det, count, (int)max_det, lab_img, lab_cls,
                       lab_box, (int)n_labels, img_w, img_h, native, lv, (int)n_levels, single_cls ? 1 : 0, tp, cm, (int)nc, cm_conf, cm_iou, MaskCounts{});
    YMI_CHECK_LAUNCH("val_match");
    return YMI_OK;
}

extern "C" int ymi_val_match_masks(const float* det, const int32_t* count, int64_t batch, int64_t max_det, const int32_t* lab_img, const float* lab_cls,
                                   int64_t n_labels, const int32_t* inter, const int32_t* area_pred, const int32_t* area_gt, int64_t n_bins,
                                   const float* levels, int32_t n_levels, int32_t single_cls, uint8_t* tp_m, void* stream) {
    YMI_CHECK_ARG(batch > 0 && batch < ((int64_t)1 << 31), "val_match_masks: bad batch");
    YMI_CHECK_ARG(max_det > 0 && max_det <= VM_MAX_DET, "val_match_masks: max_det in [1, %d]", VM_MAX_DET);
    YMI_CHECK_ARG(levels && n_levels > 0 && n_levels <= YMI_VALMATCH_MAX_LEVELS, "val_match_masks: 1 to %d IoU levels", YMI_VALMATCH_MAX_LEVELS);
    YMI_CHECK_ARG(n_labels >= 0 && n_labels < ((int64_t)1 << 31) - VM_CHUNK, "val_match_masks: the label table must have fewer than 2^31 rows");
    YMI_CHECK_ARG(det && count && tp_m && inter && area_pred && area_gt, "val_match_masks: null pointer");
    YMI_CHECK_ARG(n_labels == 0 || (lab_img && lab_cls), "val_match_masks: null label table");
    YMI_CHECK_ARG(n_bins >= 1 && n_bins <= YMI_MASK_MAX_BINS, "val_match_masks: n_bins in [1, %d]", YMI_MASK_MAX_BINS);
    if (((uintptr_t)det & 3) || ((uintptr_t)count & 3) || ((uintptr_t)lab_img & 3) || ((uintptr_t)lab_cls & 3) || ((uintptr_t)inter & 3) ||
        ((uintptr_t)area_pred & 3) || ((uintptr_t)area_gt & 3)) {
        ymi_set_error("val_match_masks: det / count / labels / counts need 4-byte alignment");
        return YMI_EALIGN;
    }
    Levels lv = {};
    for (int i = 0; i < n_levels; ++i) lv.v[i] = levels[i];
    const MaskCounts mc = {inter, area_pred, area_gt, (int)n_bins};
    hipLaunchKernelGGL(val_match_kernel<true>, dim3((unsigned)batch), dim3(VM_THREADS), 0, (hipStream_t)stream, det, count, (int)max_det, lab_img, lab_cls,
                       nullptr, (int)n_labels, 1.0f, 1.0f, nullptr, lv, (int)n_levels, single_cls ? 1 : 0, tp_m, nullptr, 0, 0.0f, 0.0f, mc);
    YMI_CHECK_LAUNCH("val_match_masks");
    return YMI_OK;
}
