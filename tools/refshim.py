"""Dev-container-only loader for the upstream reference (never shipped, never imported by the product).

Imports `/root/reference/{frostnet,frostnet_features,optimizer}.py` *in place* (no copy) behind the
four shims SURVEY.md Appendix D describes, so `tools/gen_golden.py` can run the reference and write
golden input/output vectors into `tests/golden/`.  Nothing under `frostnet_amd/`, `oracle/`, `tests/`,
`bench.py` or `__graft_entry__.py` imports this file; the GPU box has no `/root/reference`.
"""
import importlib.util
import os
import sys
import types

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True

import torch

REF = "/root/reference"
_REGISTRY = {}


def _install_timm_shim():
    if "timm" in sys.modules:
        return
    timm = types.ModuleType("timm")
    data = types.ModuleType("timm.data")
    data.IMAGENET_DEFAULT_MEAN = (0.485, 0.456, 0.406)
    data.IMAGENET_DEFAULT_STD = (0.229, 0.224, 0.225)
    data.IMAGENET_INCEPTION_MEAN = (0.5, 0.5, 0.5)
    data.IMAGENET_INCEPTION_STD = (0.5, 0.5, 0.5)
    models = types.ModuleType("timm.models")
    registry = types.ModuleType("timm.models.registry")

    def register_model(fn):
        _REGISTRY[fn.__name__] = fn
        return fn

    registry.register_model = register_model
    timm.data, timm.models, models.registry = data, models, registry
    sys.modules.update({"timm": timm, "timm.data": data, "timm.models": models,
                        "timm.models.registry": registry})


def _install_fuse_shim():
    """torch<=1.10 `fuse_modules` produced QAT-fusable modules in train mode; modern torch asserts."""
    import torch.ao.quantization as aoq
    if getattr(torch.quantization, "_frost_shim", False):
        return
    orig = aoq.fuse_modules

    def fuse_modules(model, names, inplace=False, **kw):
        if model.training:
            return aoq.fuse_modules_qat(model, names, inplace=inplace, **kw)
        return orig(model, names, inplace=inplace, **kw)

    torch.quantization.fuse_modules = fuse_modules
    torch.quantization._frost_shim = True


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def load_frostnet():
    _install_timm_shim()
    _install_fuse_shim()
    if "ref_frostnet" in sys.modules:
        return sys.modules["ref_frostnet"], _REGISTRY
    return _load("ref_frostnet", f"{REF}/frostnet.py"), _REGISTRY


def load_features():
    _install_fuse_shim()
    if "refpkg.backbones.frostnet_features" in sys.modules:
        return sys.modules["refpkg.backbones.frostnet_features"]
    pkg = types.ModuleType("refpkg"); pkg.__path__ = []
    bb = types.ModuleType("refpkg.backbones"); bb.__path__ = []
    builder = types.ModuleType("refpkg.builder")

    class _Reg:
        def register_module(self):
            return lambda cls: cls

    builder.BACKBONES = _Reg()
    sys.modules.update({"refpkg": pkg, "refpkg.backbones": bb, "refpkg.builder": builder})
    return _load("refpkg.backbones.frostnet_features", f"{REF}/frostnet_features.py")


def load_mobilenetv3():
    """The reference's MobileNetV3 baseline file: only its quantizable `_Hswish` module is used."""
    if "ref_mobilenetv3" in sys.modules:
        return sys.modules["ref_mobilenetv3"]
    return _load("ref_mobilenetv3", f"{REF}/Classification/models/imagenet/mobilenetv3.py")


def load_detection():
    """The reference's SSD loss pieces (Object_Detection/layers): PriorBox and MultiBoxLoss.  cv2 / torchvision are absent here and only
    imported at module level by files we do not execute: stub them."""
    if "layers" not in sys.modules:
        sys.modules.setdefault("cv2", types.ModuleType("cv2"))
        if "torchvision" not in sys.modules:
            tv, tvo = types.ModuleType("torchvision"), types.ModuleType("torchvision.ops")
            tv.ops, tvo.nms = tvo, None
            sys.modules["torchvision"], sys.modules["torchvision.ops"] = tv, tvo
        sys.path.insert(0, f"{REF}/Object_Detection")
    from layers.functions.prior_box import PriorBox
    from layers.modules.multibox_loss import MultiBoxLoss
    return PriorBox, MultiBoxLoss


def load_detect_layer(min_dim, variance):
    """The reference's Detect (Object_Detection/layers/functions/detection.py) for a configuration with this min_dim / variance.  torchvision is absent, so
    its `nms_faster_rcnn` is bound to the reference's own layers.box_utils.nms over all the boxes handed in (the same keep criterion, IoU <= threshold)."""
    load_detection()
    import layers.functions.detection as det
    from layers.box_utils import nms

    def nms_ref(boxes, scores, thresh):
        keep, count = nms(boxes, scores, thresh, top_k=len(boxes))
        return keep[:count]

    det.nms_faster_rcnn = nms_ref
    det.cfg = dict(min_dim=min_dim, variance=list(variance))
    return det.Detect


def load_voc_eval():
    """The reference's `voc_ap` and `voc_eval` (Object_Detection/qeval_convert.py).  The file is a script that imports cv2-dependent modules and never imports the
    `ET` it uses, so it cannot be imported: it is parsed in place, the two function definitions alone are compiled and executed in a namespace that holds numpy
    (with the `np.bool` alias that numpy >= 1.24 dropped), os and pickle.  Nothing is copied or written."""
    import ast
    import pickle
    import numpy as np
    path = f"{REF}/Object_Detection/qeval_convert.py"
    tree = ast.parse(open(path).read(), filename=path)
    tree.body = [node for node in tree.body if isinstance(node, ast.FunctionDef) and node.name in ("voc_ap", "voc_eval")]
    assert [node.name for node in tree.body] == ["voc_ap", "voc_eval"]
    if not hasattr(np, "bool"):
        np.bool = bool
    ns = dict(np=np, os=os, pickle=pickle)
    exec(compile(tree, path, "exec"), ns)
    return ns["voc_ap"], ns["voc_eval"]


def load_segmentation():
    """The reference's segmentation criterion, mean-IoU meter and validation loop (Semantic_Segmentation/loss_fns, utilities): (SegmentationLoss, MIOU, val_seg)."""
    seg = f"{REF}/Semantic_Segmentation"
    if seg not in sys.path:
        sys.path.insert(0, seg)
    from loss_fns.segmentation_loss import SegmentationLoss
    from utilities.metrics.segmentation_miou import MIOU
    from utilities.train_eval_seg import val_seg
    return SegmentationLoss, MIOU, val_seg


def load_seg_head():
    """The reference's Lite R-ASPP head (Semantic_Segmentation/model/layers/LRASPP.py: `_Head` over `_LRASPP`), imported in place."""
    seg = f"{REF}/Semantic_Segmentation"
    if seg not in sys.path:
        sys.path.insert(0, seg)
    from model.layers.LRASPP import _Head
    return _Head


def load_seg_transforms():
    """The reference's segmentation transforms (Semantic_Segmentation/utilities/data_transforms.py), imported in place.  torchvision is absent, so the three things the
    file takes from it are restated with Pillow as torchvision defines them for PIL images: `Pad` (constant fill on (left/right, top/bottom), the palette of a mode-P
    image kept), `functional.crop`, and `functional.to_tensor` / `normalize`; `Image.ANTIALIAS`, gone from Pillow 10, is today's `Image.LANCZOS`."""
    if "ref_seg_transforms" in sys.modules:
        return sys.modules["ref_seg_transforms"]
    import numpy as np
    from PIL import Image
    if not hasattr(Image, "ANTIALIAS"):
        Image.ANTIALIAS = Image.LANCZOS

    class Pad:
        def __init__(self, padding, fill=0, padding_mode="constant"):
            assert padding_mode == "constant" and len(padding) == 2
            self.padding, self.fill = padding, fill

        def __call__(self, img):
            pw, ph = self.padding
            out = Image.new(img.mode, (img.size[0] + 2 * pw, img.size[1] + 2 * ph), self.fill)
            if img.mode == "P" and img.getpalette() is not None:
                out.putpalette(img.getpalette())
            out.paste(img, (pw, ph))
            return out

    def crop(img, top, left, height, width):
        return img.crop((left, top, left + width, top + height))

    def to_tensor(img):
        a = np.array(img, dtype=np.uint8)
        return torch.from_numpy(a.reshape(a.shape[0], a.shape[1], -1)).permute(2, 0, 1).contiguous().to(torch.float32).div(255)

    def normalize(t, mean, std):
        m, s = torch.as_tensor(mean, dtype=t.dtype), torch.as_tensor(std, dtype=t.dtype)
        return t.clone().sub_(m[:, None, None]).div_(s[:, None, None])

    saved = {k: sys.modules.get(k) for k in ("torchvision", "torchvision.transforms", "torchvision.transforms.functional")}
    tv, tvt, tvf = types.ModuleType("torchvision"), types.ModuleType("torchvision.transforms"), types.ModuleType("torchvision.transforms.functional")
    tv.transforms, tvt.functional, tvt.Pad = tvt, tvf, Pad
    tvf.crop, tvf.to_tensor, tvf.normalize = crop, to_tensor, normalize
    sys.modules.update({"torchvision": tv, "torchvision.transforms": tvt, "torchvision.transforms.functional": tvf})
    try:
        return _load("ref_seg_transforms", f"{REF}/Semantic_Segmentation/utilities/data_transforms.py")
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v


def load_optimizer():
    if "ref_optimizer" in sys.modules:
        return sys.modules["ref_optimizer"]
    torch.Tensor.cuda = lambda self, *a, **k: self  # optimizer.py:180 `.cuda()` on a CPU box
    return _load("ref_optimizer", f"{REF}/optimizer.py")


def load_helpers():
    if "ref_helpers" in sys.modules:
        return sys.modules["ref_helpers"]
    return _load("ref_helpers", f"{REF}/Classification/utils/helper_functions.py")


def qat_prepare(model, version=0, backend="qnnpack"):
    """Classification/train.py:171-173 with the qconfig version pinned (SURVEY H-3)."""
    from torch.ao.quantization import get_default_qat_qconfig, prepare_qat
    model.train()
    model.fuse_model()
    model.qconfig = get_default_qat_qconfig(backend, version=version)
    prepare_qat(model, inplace=True)
    return model
