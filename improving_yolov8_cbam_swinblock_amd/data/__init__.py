"""what the reference keeps under ultralytics/data that this package has: the inference-time LetterBox."""
from .augment import LetterBox  # noqa: F401
