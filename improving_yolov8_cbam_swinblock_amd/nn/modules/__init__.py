"""Operator modules of the hot path, same names as the reference's ultralytics/nn/modules/__init__.py."""
from .block import C2f, C2PSA, C3, C3k, C3k2, PSA, SPPF, Attention, Bottleneck, C3Ghost, DFL, GhostBottleneck, Proto, PSABlock  # noqa: F401
from .cbam import CBAM, ChannelAttention, SpatialAttention  # noqa: F401
from .conv import Concat, Conv, DWConv, GhostConv, Upsample, autopad  # noqa: F401
from .head import OBB, Detect, OBBPreds, SegPreds, Segment  # noqa: F401
from .swin_block import SwinBlock, window_partition, window_reverse  # noqa: F401
