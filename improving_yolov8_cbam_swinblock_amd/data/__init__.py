"""what the reference keeps under ultralytics/data that this package has: the inference-time LetterBox and the training transforms as the
parameter source of the on-device augmentation."""
from .augment import LetterBox, Mosaic, RandomFlip, RandomHSV, RandomPerspective, V8Transforms, v8_transforms  # noqa: F401
