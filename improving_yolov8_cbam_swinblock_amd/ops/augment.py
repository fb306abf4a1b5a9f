"""Training augmentation on the device (csrc/augment.hip): mosaic, affine warp, HSV and flips of a batch as one launch per 32 images that
writes the float32 NCHW batch, and the labels of the batch through the same geometry as one launch.  The random draws are data.augment's; the
geometry here is host arithmetic that follows the reference statement for statement.  No gradient flows through any of it."""
import ctypes
import math

import numpy as np
import torch

from .._lib import AUGMENT_MAX_SRC, AugmentImage, AugmentLabelImage, AugmentSource
from .base import L, check, ptr, stream_ptr
from .resize import _as_u8_image


def mosaic_placement(i, xc, yc, h, w, s):
    """where image i (0..3, of shape h x w) lies on the 2s x 2s canvas around the centre (xc, yc): Mosaic._mosaic4 (reference
    data/augment.py:692-708), statement for statement -> (x1a, y1a, x2a, y2a, x1b, y1b, padw, padh)."""
    if i == 0:  # top left
        x1a, y1a, x2a, y2a = max(xc - w, 0), max(yc - h, 0), xc, yc  # xmin, ymin, xmax, ymax (large image)
        x1b, y1b, x2b, y2b = w - (x2a - x1a), h - (y2a - y1a), w, h  # xmin, ymin, xmax, ymax (small image)
    elif i == 1:  # top right
        x1a, y1a, x2a, y2a = xc, max(yc - h, 0), min(xc + w, s * 2), yc
        x1b, y1b, x2b, y2b = 0, h - (y2a - y1a), min(w, x2a - x1a), h
    elif i == 2:  # bottom left
        x1a, y1a, x2a, y2a = max(xc - w, 0), yc, xc, min(s * 2, yc + h)
        x1b, y1b, x2b, y2b = w - (x2a - x1a), 0, w, min(y2a - y1a, h)
    elif i == 3:  # bottom right
        x1a, y1a, x2a, y2a = xc, yc, min(xc + w, s * 2), min(s * 2, yc + h)
        x1b, y1b, x2b, y2b = 0, 0, min(w, x2a - x1a), min(y2a - y1a, h)
    else:
        raise ValueError("mosaic_placement: a 2 x 2 mosaic has images 0..3")
    padw = x1a - x1b
    padh = y1a - y1b
    return x1a, y1a, x2a, y2a, x1b, y1b, padw, padh


def rotation_matrix_2d(center, angle, scale):
    """cv2.getRotationMatrix2D by its documented formula, in double -> [2, 3]"""
    a = angle * math.pi / 180
    alpha, beta = math.cos(a) * scale, math.sin(a) * scale
    return np.array([[alpha, beta, (1 - alpha) * center[0] - beta * center[1]], [-beta, alpha, beta * center[0] + (1 - alpha) * center[1]]], dtype=np.float64)


def affine_matrix(shape, border, draws):
    """RandomPerspective.affine_transform's matrix (reference data/augment.py:1042-1071), statement for statement, from the draws that
    data.augment.RandomPerspective made: {"perspective": (px, py), "angle": a, "scale": s, "shear": (sx, sy), "translate": (tx, ty)} - the
    numbers random.uniform returned.  shape: (h, w) of the image that is warped; border: the mosaic border.
    -> (M float32 [3, 3], (w, h) of the output, A: the inverse of M[:2] as six doubles, inverted as warpAffine inverts it)."""
    if draws["perspective"][0] or draws["perspective"][1]:
        raise NotImplementedError("perspective != 0 needs warpPerspective and the division by w (reference data/augment.py:1075, :1107)")
    size = shape[1] + border[1] * 2, shape[0] + border[0] * 2  # w, h
    # Center
    C = np.eye(3, dtype=np.float32)
    C[0, 2] = -shape[1] / 2  # x translation (pixels)
    C[1, 2] = -shape[0] / 2  # y translation (pixels)
    # Perspective
    P = np.eye(3, dtype=np.float32)
    P[2, 0] = draws["perspective"][0]  # x perspective (about y)
    P[2, 1] = draws["perspective"][1]  # y perspective (about x)
    # Rotation and Scale
    R = np.eye(3, dtype=np.float32)
    a = draws["angle"]
    s = draws["scale"]
    R[:2] = rotation_matrix_2d(angle=a, center=(0, 0), scale=s)
    # Shear
    S = np.eye(3, dtype=np.float32)
    S[0, 1] = math.tan(draws["shear"][0] * math.pi / 180)  # x shear (deg)
    S[1, 0] = math.tan(draws["shear"][1] * math.pi / 180)  # y shear (deg)
    # Translation
    T = np.eye(3, dtype=np.float32)
    T[0, 2] = draws["translate"][0] * size[0]  # x translation (pixels)
    T[1, 2] = draws["translate"][1] * size[1]  # y translation (pixels)
    # Combined rotation matrix
    M = T @ S @ R @ P @ C  # order of operations (right to left) is IMPORTANT
    return M, size, invert_affine(M[:2])


def invert_affine(M):
    """the inverse of a forward 2 x 3 matrix as warpAffine forms it before it maps destination to source (double precision, this order of
    operations; include/ymi.h) -> six Python floats"""
    m = [float(v) for v in np.asarray(M, dtype=np.float64).reshape(-1)[:6]]
    D = m[0] * m[4] - m[1] * m[3]
    D = 1.0 / D if D != 0 else 0.0
    A11, A22 = m[4] * D, m[0] * D
    m[0] = A11
    m[1] *= -D
    m[3] *= -D
    m[4] = A22
    b1 = -m[0] * m[2] - m[1] * m[5]
    b2 = -m[3] * m[2] - m[4] * m[5]
    m[2], m[5] = b1, b2
    return m


def hsv_luts(r):
    """RandomHSV's three tables (reference data/augment.py:1372-1377) from its gains r = np.random.uniform(-1, 1, 3) * [hgain, sgain, vgain]
    -> uint8 [768]: hue, saturation, value"""
    dtype = np.uint8
    r = np.asarray(r, dtype=np.float64)
    x = np.arange(0, 256, dtype=r.dtype)
    lut_hue = ((x + r[0] * 180) % 180).astype(dtype)
    lut_sat = np.clip(x * (r[1] + 1), 0, 255).astype(dtype)
    lut_val = np.clip(x * (r[2] + 1), 0, 255).astype(dtype)
    lut_sat[0] = 0  # prevent pure white changing color, introduced in 8.3.79
    return np.concatenate([lut_hue, lut_sat, lut_val])


def _labels_of(sample):
    """-> float32 [n, 5] = (cls, xywh normalised) of a sample given as "labels" [n, 5] or as "cls" [n] / [n, 1] and "bboxes" [n, 4]"""
    if "labels" in sample:
        lab = np.asarray(sample["labels"], dtype=np.float32).reshape(-1, 5)
    else:
        cls = np.asarray(sample["cls"], dtype=np.float32).reshape(-1, 1)
        lab = np.concatenate([cls, np.asarray(sample["bboxes"], dtype=np.float32).reshape(len(cls), 4)], 1)
    return lab


def _align(n, a=16):
    return (n + a - 1) // a * a


class AugmentPlan:
    """a batch packed and uploaded (pack_augment): the host table, the device copy of everything, and where each part lies in it"""

    def __init__(self, table, dev_stage, rows_off, lab_off, tab_off, B, n, s, max_boxes, keepalive):
        self.table, self.dev_stage, self.rows_off, self.lab_off, self.tab_off = table, dev_stage, rows_off, lab_off, tab_off
        self.B, self.n, self.s, self.max_boxes, self.keepalive = B, n, s, max_boxes, keepalive
        self.source_bytes = sum(int(table[b].s[k].h) * int(table[b].s[k].w) * 3 for b in range(B) for k in range(table[b].n_src))

    def images(self, out, bgr=True, normalize=True, border=114):
        """the image launch(es) into out [B, 3, s, s] float32"""
        base = self.dev_stage.data_ptr()
        check(L().ymi_augment_batch(self.table, ctypes.c_void_p(base + self.tab_off), self.B, ptr(out), self.s, int(border), int(bool(normalize)),
                                    int(bool(bgr)), stream_ptr()), "augment_batch")
        return out

    def labels(self, batch_idx, cls, bboxes, keep, count, area_thr=0.10):
        """the label launch; count: int32 [B + 1], the total last"""
        base = self.dev_stage.data_ptr()
        check(L().ymi_augment_boxes(ctypes.c_void_p(base + self.rows_off), self.n, ctypes.c_void_p(base + self.lab_off), self.B, float(area_thr),
                                    ptr(batch_idx), ptr(cls), ptr(bboxes), ptr(keep), ptr(count), ctypes.c_void_p(count.data_ptr() + 4 * self.B),
                                    stream_ptr()), "augment_boxes")


def augment_batch(samples, params, imgsz, bgr=True, normalize=True, border=114, area_thr=0.10, device=None):
    """The reference's v8_transforms (data/augment.py:2375-2439, perspective = 0) of a batch on the device, csrc/augment.hip.
    samples[i]: {"img": (h, w, 3) uint8 BGR numpy array or tensor, host or device; "labels" [n, 5] = (cls, xywh normalised) - or "cls" and
                 "bboxes" -; "mix_labels": three more such samples, the mosaic partners; optional "ori_shape" (h0, w0) and "ratio_pad"
                 ((r_h, r_w), (left, top)) when "img" was letterboxed from an image of that shape (labels refer to the original)}
    params[i]:  what data.augment's classes drew: {"mosaic": None or {"yc", "xc"}, "affine": RandomPerspective's draws, "hsv": None or
                 RandomHSV's gains, "flipud", "fliplr"}
    With "mosaic" the four images go on the 2s x 2s canvas and the warp cuts s x s out of it; without, the image itself is warped (border 0),
    which needs it to be s x s already (engine.trainer.augment_batch letterboxes first, as the reference's pre_transform does).
    Host images, the table, the colour tables and the label rows are packed into ONE pinned staging buffer and uploaded with ONE copy; then
    one launch per 32 images writes the batch and one launch the labels.  Reading the number of kept labels back is the only synchronisation.
    -> {"img" [B, 3, s, s] float32, "batch_idx" [n], "cls" [n, 1], "bboxes" [n, 4] float32 (kept rows, image by image, in their order),
        "count" [B] int32, "keep" [rows] int32, "max_boxes": the largest number of label rows any image STARTED with (a static bound for
        TrainStep)}."""
    plan = pack_augment(samples, params, imgsz, device)
    B, n, device = plan.B, plan.n, plan.dev_stage.device
    img = plan.images(torch.empty((B, 3, plan.s, plan.s), dtype=torch.float32, device=device), bgr, normalize, border)
    batch_idx = torch.empty(max(n, 1), dtype=torch.float32, device=device)
    cls = torch.empty((max(n, 1), 1), dtype=torch.float32, device=device)
    bboxes = torch.empty((max(n, 1), 4), dtype=torch.float32, device=device)
    keep = torch.empty(max(n, 1), dtype=torch.int32, device=device)
    count = torch.empty(B + 1, dtype=torch.int32, device=device)  # [B] per image, then the total
    plan.labels(batch_idx, cls, bboxes, keep, count, area_thr)
    kept = int(count[B].item())  # (the launches that read the plan's buffers have finished when this returns)
    return {"img": img, "batch_idx": batch_idx[:kept], "cls": cls[:kept], "bboxes": bboxes[:kept], "count": count[:B], "keep": keep[:n],
            "max_boxes": plan.max_boxes}


def pack_augment(samples, params, imgsz, device=None):
    """the host side of augment_batch: geometry, table, staging buffer, the one upload -> AugmentPlan"""
    B, s = len(samples), int(imgsz)
    if not B or len(params) != B:
        raise ValueError("augment_batch: one parameter set per sample, at least one sample")
    table = (AugmentImage * B)()
    label_images = (AugmentLabelImage * B)()
    host, host_ims, luts, rows, row_at, all_ims = [], [], [], [], 0, []
    for b, (smp, par) in enumerate(zip(samples, params)):
        row, lab = table[b], label_images[b]
        mos = par.get("mosaic")
        members = [smp] + list(smp.get("mix_labels", ())) if mos is not None else [smp]
        if mos is not None and len(members) != 4:
            raise NotImplementedError("a mosaic takes the sample and three partners in 'mix_labels'; Mosaic-9 is data/augment.py:716-786 of the reference")
        ims = [_as_u8_image(m["img"]) for m in members]
        all_ims += ims
        if device is None:
            device = next((im.device for im, on in ims if on), None)
        if mos is not None:
            canvas_hw, brd = (2 * s, 2 * s), (-s // 2, -s // 2)
        else:
            canvas_hw, brd = tuple(int(v) for v in ims[0][0].shape[:2]), (0, 0)
        M, size, A = affine_matrix(canvas_hw, brd, par["affine"])
        if size != (s, s):
            raise ValueError(f"augment_batch: sample {b} warps to {size[1]} x {size[0]}, not {s} x {s}: without a mosaic the image must be letterboxed to imgsz first")
        row.n_src, row.canvas_h, row.canvas_w = len(members), canvas_hw[0], canvas_hw[1]
        row.flip_ud, row.flip_lr = int(bool(par.get("flipud"))), int(bool(par.get("fliplr")))
        for k in range(6):
            row.A[k] = A[k]
            lab.M[k] = float(M[:2].reshape(-1)[k])
        for k in range(AUGMENT_MAX_SRC):
            lab.src_w[k] = lab.src_h[k] = lab.ratio_w[k] = lab.ratio_h[k] = 1.0
        lab.scale, lab.size_w, lab.size_h, lab.canvas = float(par["affine"]["scale"]), float(size[0]), float(size[1]), float(2 * s if mos is not None else 0)
        lab.flip_ud, lab.flip_lr, lab.row_start = row.flip_ud, row.flip_lr, row_at
        for k, (m, (im, on)) in enumerate(zip(members, ims)):
            h, w = int(im.shape[0]), int(im.shape[1])
            place = mosaic_placement(k, int(mos["xc"]), int(mos["yc"]), h, w, s) if mos is not None else (0, 0, w, h, 0, 0, 0, 0)
            row.s[k] = AugmentSource(im.data_ptr() if on else 0, h, w, *place[:6])
            if not on:
                host.append((b, k))
                host_ims.append(im)
            if mos is None and m.get("ratio_pad") is not None:  # LetterBox._update_labels: the labels refer to the image before the letterbox
                (r_h, r_w), (left, top) = m["ratio_pad"]
                h0, w0 = m["ori_shape"]
                lab.src_w[k], lab.src_h[k], lab.ratio_w[k], lab.ratio_h[k], lab.padw[k], lab.padh[k] = w0, h0, r_w, r_h, left, top
            else:
                lab.src_w[k], lab.src_h[k], lab.padw[k], lab.padh[k] = w, h, place[6], place[7]
            lk = _labels_of(m)
            rows.append(np.concatenate([np.full((len(lk), 1), b, dtype=np.float32), np.full((len(lk), 1), k, dtype=np.float32), lk], 1))
            row_at += len(lk)
        lab.row_end = row_at
        if par.get("hsv") is not None:
            lut = hsv_luts(par["hsv"])
            if int(lut[:256].max()) >= 180:
                raise ValueError("augment_batch: a hue table entry of 180 or more")
            luts.append((b, lut))
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device())
    rows = np.concatenate(rows, 0).astype(np.float32) if rows else np.zeros((0, 7), np.float32)
    n = len(rows)
    # one staging buffer: [host images | colour tables | label rows | label table | image table], one copy
    img_off = np.cumsum([0] + [_align(im.numel()) for im in host_ims])
    lut_off = int(img_off[-1])
    rows_off = lut_off + _align(768 * len(luts))
    lab_off = rows_off + _align(rows.nbytes)
    tab_off = lab_off + _align(ctypes.sizeof(label_images))
    total = tab_off + _align(ctypes.sizeof(table))
    stage = torch.empty(total, dtype=torch.uint8, pin_memory=True)
    dev_stage = torch.empty(total, dtype=torch.uint8, device=device)
    base = dev_stage.data_ptr()
    for (b, k), im, o in zip(host, host_ims, img_off):
        stage[int(o) : int(o) + im.numel()] = im.reshape(-1)
        table[b].s[k].src = base + int(o)
    for j, (b, lut) in enumerate(luts):
        stage[lut_off + 768 * j : lut_off + 768 * (j + 1)] = torch.from_numpy(lut)
        table[b].lut = base + lut_off + 768 * j
    stage_np = stage.numpy()
    stage_np[rows_off : rows_off + rows.nbytes] = rows.reshape(-1).view(np.uint8)
    stage_np[lab_off : lab_off + ctypes.sizeof(label_images)] = np.frombuffer(label_images, dtype=np.uint8)
    stage_np[tab_off : tab_off + ctypes.sizeof(table)] = np.frombuffer(table, dtype=np.uint8)  # (after the device addresses went in)
    dev_stage.copy_(stage, non_blocking=True)
    max_boxes = max([int(label_images[b].row_end - label_images[b].row_start) for b in range(B)] + [1])
    return AugmentPlan(table, dev_stage, rows_off, lab_off, tab_off, B, n, s, max_boxes, (stage, [im for im, _ in all_ims]))
