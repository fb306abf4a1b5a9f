"""LetterBox with the reference's name and constructor (ultralytics/data/augment.py:1479-1603) on ops.letterbox (csrc/resize.hip)."""
from .. import ops


class LetterBox:
    """LetterBox(new_shape, auto, scale_fill, scaleup, center, stride)(image=img) -> the letterboxed image [h', w', 3] float32 on the device,
    grey levels 0..255 in the image's own channel order (what the reference returns as a uint8 array, before the predictor's conversion;
    ops.letterbox does both in one launch for a list).  The `labels` form updates a dataset's Instances, which this package has not."""

    def __init__(self, new_shape=(640, 640), auto=False, scale_fill=False, scaleup=True, center=True, stride=32):
        self.new_shape = new_shape
        self.auto = auto
        self.scale_fill = scale_fill
        self.scaleup = scaleup
        self.stride = stride
        self.center = center  # Put the image in the middle or top-left

    def __call__(self, labels=None, image=None):
        if labels is not None or image is None:
            raise NotImplementedError("LetterBox: the labels form needs the dataset's Instances, which are not built; call it with image=...")
        out, _ = ops.letterbox([image], self.new_shape, auto=self.auto, scale_fill=self.scale_fill, scaleup=self.scaleup, center=self.center,
                               stride=self.stride, bgr=False, normalize=False)
        return out[0].permute(1, 2, 0)
