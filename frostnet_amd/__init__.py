"""frostnet_amd -- MI355X-native FrostNet QAT hot path (hand-written HIP for gfx950 behind the reference's
nn.Module / optimizer surface).  See DESIGN.md."""
from ._lib import LIB_PATH, SYMBOLS, load_library  # noqa: F401
from .augment import BaseTransform, SSDAugmentation, identity_plan, pad_images  # noqa: F401
from .cls_augment import ClassificationAugmentation, ClassificationEvalTransform  # noqa: F401
from .seg import SegMeter, SegmentationLoss, seg_reference  # noqa: F401
from .seg_augment import SegmentationAugmentation, SegmentationEvalTransform, pad_pairs  # noqa: F401
from .seg_model import FrostNetSeg, LRASPPHead, frostnet_seg_base_1_0, frostnet_seg_large_1_0, frostnet_seg_small_1_0  # noqa: F401
from .voc_eval import VOCEvaluator  # noqa: F401

__all__ = ["load_library", "LIB_PATH", "SYMBOLS", "VOCEvaluator", "SegmentationLoss", "SegMeter", "seg_reference","SSDAugmentation", "BaseTransform", "identity_plan", "pad_images", "ClassificationAugmentation",
           "ClassificationEvalTransform", "SegmentationAugmentation", "SegmentationEvalTransform", "pad_pairs", "FrostNetSeg", "LRASPPHead",
           "frostnet_seg_large_1_0", "frostnet_seg_base_1_0", "frostnet_seg_small_1_0"]
