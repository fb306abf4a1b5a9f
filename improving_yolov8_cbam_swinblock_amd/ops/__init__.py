"""torch.autograd.Function wrappers over the C ABI of libyolo_mi355.so.

PyTorch is plumbing here: it owns device memory, streams and the autograd tape; every tensor
operation on the hot path is a hand-written gfx950 kernel reached through `_lib` (ctypes).  There is
no fallback: without the library, or with CPU tensors, these functions raise.

Tensor convention between ops: logical [N, C, H, W] tensors whose MEMORY is NHWC (channels_last),
possibly a channel slice of a wider buffer (pixel stride ld > C); token matrices are plain [T, C].
Compute dtype is bfloat16 under `torch.autocast("cuda", dtype=torch.bfloat16)` and the input's
dtype (float32 = parity mode) otherwise; parameters stay float32 and are packed per call.
"""
# The op layer as a package (round 5: one 2,300-line module before): base -> weights -> conv -> blocks, each importing only from the ones before it.
# Every name is re-exported here, so `from .. import ops; ops.conv_bn_act(...)` and the tests' `ops._dgrad(...)` read as they always did.  Run-time
# state has two owners: a model's ModelState (its arenas, forward epoch and counters) and the process-wide RUN (the active ModelState, backward passes).
from .._lib import ACT_GELU, ACT_NONE, ACT_SILU, ConvProblem, DgradProblem, as_ymi, check, chunk_elems, empty_nhwc, is_nhwc, ptr, stream_ptr, workspace, ymi_dtype  # noqa: F401
from .base import (  # noqa: F401
    RUN, GradJoin, HOOKS, L, LazyConcatBuffer, OutSlot, _GradBuffer, _GradSlot, _ToInternal, _accumulate, _as4d, _byref, _conv_out_hw,
    _count_batch, _deferred_twice, _dense_ok, _in_backward, _join_plain, _note_use, _prep_adds, _stat_acc, compute_dtype, grad_nhwc, join_of, mark_join,
    round_up, to_internal, to_nchw_float,
)
from .weights import (  # noqa: F401
    ModelState, WeightArena, _PackDesc, _adoptable, _defer_wgrad, _flush_wgrads, _new_dw, _side_stream, _wgrad,
    _wgrad_deferred, _wgrad_maybe_async, async_wgrad, deferred_wgrad, grad_arena, join_side_stream, pack_conv_dgrad, pack_conv_dgrad_pair,
    pack_conv_fwd, pack_conv_fwd_pair, set_weight_arena, wgrad_riders,
)
from .conv import (  # noqa: F401
    DgradJob, FwdProblem, _ChanSlice, _ChanSplit2, _ConvAffineAct, _ConvBnAct, _ConvBnActPair, _DetectTrain, _FirstConvBnAct, _Level, _bn_act_bwd,
    _conv_fwd_multi, _detect_args, _detect_grads, _dgrad, _dgrad_finish, _dgrad_joined, _dgrad_joined_finish, _dgrad_joined_prepare, _dgrad_launch,
    _dgrad_multi, _dgrad_prepare, _per_level, _width_class, chan_split2, conv_affine_act, conv_bn_act, conv_bn_act_pair, detect_train, detect_train_ok,
    first_conv_bn_act, first_conv_ok, linear, padded_grad_like,
)
from .dwconv import _DwConvAffineAct, _DwConvBnAct, dwconv_affine_act, dwconv_bn_act  # noqa: F401
from .blocks import (  # noqa: F401
    _Act, _AddResidual, _C2fSplit, _Cbam, _Concat, _DetectLoss, _LayerNorm, _PsaAttention, _SppfPool, _SwinLnMlp, _SwinMlp, _Upsample2x, _WindowAttention,
    _WindowReverse, _map_array, add_residual, c2f_split, cbam, concat, detect_decode, detect_loss, detect_nms, detect_nms_seg, detect_targets, gelu, layernorm, psa_attention, sppf_pool_cat,
    swin_ln_mlp, swin_ln_mlp_ok, swin_mlp, upsample2x, window_attention, window_pad, window_partition, window_partition_index, window_reverse,
)
from .seg import (  # noqa: F401
    _ConvTranspose2x2, _DetectLossAssign, _MaskLoss, conv_transpose2x2, conv_transpose2x2_ok, depth_to_space2, detect_decode_seg, detect_loss_assign, mask_loss,
    mask_overlap, process_mask, space_to_depth2,
)
from .obb import _ObbAngle, _ObbLoss, detect_decode_obb, obb_angle, obb_loss, obb_targets  # noqa: F401
from .resize import letterbox, letterbox_geometry, scale_boxes, scale_boxes_params, scale_image, scale_rows, tta_clip_ranges, tta_merge  # noqa: F401
from .augment import affine_matrix, augment_batch, hsv_luts, invert_affine, mosaic_placement  # noqa: F401
from .validate import VAL_MATCH_LABEL_CHUNK, val_match, val_match_masks  # noqa: F401
