"""Caller-side pieces of the hot path that the reference keeps in its (non-importable) training scripts, restated so a
`Classification/train.py`-style driver runs on the HIP path unchanged in behaviour:

  * `make_param_groups`  -- Classification/train.py:121-137 (one group per tensor; depthwise wd 0, other 4-D wd, rest 0.01*wd)
  * `adjust_learning_rate_cosine` -- Classification/utils/helper_functions.py:231-261 (per-iteration cosine + linear warm-up)
  * `statassist_qat_switch` -- Classification/train.py:149-173 (StatAssist FP epoch(s) with the SAME optimizer, flip
    `is_warmup`, then fuse + prepare_qat keeping Parameter identity so optimizer state survives)
  * `train_one_iter` / `accuracy` -- helper_functions.py:32-46,118-155 (accuracy() fixed for torch>=1.7: reshape, not view)
  * `train` / `val` -- the epoch loops, helper_functions.py:99-163 / 306-350: mean over the iterations of the per-batch loss / top-1 / top-5.  `val`
    only switches to `model.eval()` -- as in the reference the observers stay live and keep moving with validation data.
    The running sums stay on the device: ONE host read per epoch instead of the reference's three `.item()` per iteration.
  * `val_detector` -- the detector's validation pass, Object_Detection/qeval_convert.py:348-396 (`test_net`) as qtrainval.py:314 calls it: detections on the
    device, scored by a `VOCEvaluator` whose state stays on the device; ONE host read per evaluation instead of one per image and class.
  * `train_seg` / `val_seg` -- the segmentation epoch loops, Semantic_Segmentation/utilities/train_eval_seg.py: mean IoU from a `seg.SegMeter` on the device, the
    sample-weighted loss sum on the device; ONE host read per epoch instead of one `.item()` and three host histograms per iteration.
  * `checkpoint_state` / `save_checkpoint` / `load_checkpoint` -- Classification/train.py:193-223, helper_functions.py:400-407: the reference's
    dictionary keys, plus `hip_rng` (dropout Philox seed + draw count; the GradBoost stream resumes from the optimizer's step count).
"""
import math

import torch


class _CEFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target):
        from ._lib import call, ptr, stream
        n, c = logits.shape
        x = logits.contiguous().float()
        loss = torch.zeros((), dtype=torch.float32, device=x.device)
        dlogits = torch.empty_like(x)
        call("frost_softmax_ce", ptr(x), ptr(target.contiguous()), n, c, 1.0 / n, ptr(loss), ptr(dlogits), stream())
        ctx.save_for_backward(dlogits)
        return loss

    @staticmethod
    def backward(ctx, g):
        (dlogits,) = ctx.saved_tensors
        return dlogits * g, None


class CrossEntropyLoss(torch.nn.Module):
    """`nn.CrossEntropyLoss()` (mean reduction; Classification/train.py:147) with forward and backward in ONE hand-written kernel on the
    device (`frost_softmax_ce`): loss and dlogits come out of the same pass, no host synchronisation (capturable).  Every target must be a
    valid class index (the reference's loaders never produce ignore_index); CPU tensors take torch's implementation."""

    def forward(self, logits, target):
        if not logits.is_cuda:
            return torch.nn.functional.cross_entropy(logits, target)
        if target.dtype != torch.int64 or target.dim() != 1 or logits.dim() != 2:
            raise ValueError("CrossEntropyLoss expects (N, C) logits and (N,) int64 class indices")
        return _CEFunction.apply(logits, target)


class EpochMeter:
    """The running sums of an epoch loop -- `record` = four doubles {sum of batch losses, sum of batch top-1 %, sum of batch top-k %, batches}, the sums `_epoch`
    keeps (the mean over the iterations of per-batch values, so a short last batch weighs as it does there) -- accumulated by the loss kernel itself
    (`frost_softmax_ce_metrics`) instead of `accuracy()`'s topk / eq / sum launches behind every step.  The definition, per row: rank of the target =
    #{j : x_j > x_t} + #{j < t : x_j == x_t} (equal logits: the lower class index first, the convention of ssdlite.Detect); top-1 hit: rank == 0; top-k hit:
    rank < min(topk, C); a row whose target is ignored (< 0) or whose target logit is not finite misses both; each row adds loss_row / N and 100 / N per hit.
    On CPU tensors `update` runs that definition as torch code (the yardstick of the kernel's tests).  `reset()` is an asynchronous memset, `read()` the epoch's single
    host read."""

    def __init__(self, device, topk=5):
        if int(topk) < 1:
            raise ValueError("EpochMeter: topk >= 1")
        self.device, self.topk = torch.device(device), int(topk)
        self.record = torch.zeros(4, dtype=torch.float64, device=self.device)

    def reset(self):
        self.record.zero_()

    @staticmethod
    def _check(logits, target):
        if logits.dim() != 2 or target.dim() != 1 or target.dtype != torch.int64 or target.size(0) != logits.size(0) or logits.size(0) < 1 or logits.size(1) < 1:
            raise ValueError("EpochMeter expects (N, C) logits and (N,) int64 class indices")

    def _launch(self, x, target, dlogits):
        """One launch: loss (returned, a new fp32 scalar), dlogits (may be None) and the record's sums."""
        from ._lib import call, ptr, stream
        if x.device != self.record.device or target.device != x.device:
            raise ValueError(f"EpochMeter on {self.record.device}: logits on {x.device}, target on {target.device}")
        n, c = x.shape
        loss = torch.zeros((), dtype=torch.float32, device=x.device)
        with torch.cuda.device(x.device):
            call("frost_softmax_ce_metrics", ptr(x), ptr(target.contiguous()), n, c, 1.0 / n, self.topk, ptr(loss), ptr(dlogits), ptr(self.record), stream())
        return loss

    def update_reference(self, logits, target):
        """The definition in fp64 torch code (any device): adds the batch to the record, returns the batch loss (fp64 scalar)."""
        self._check(logits, target)
        x, t = logits.detach().double(), target.to(logits.device)
        n, c = x.shape
        inv_n = float(torch.tensor(1.0 / n, dtype=torch.float32))              # the kernel's fp32 launch argument
        valid = (t >= 0) & (t < c)
        tc = t.clamp(0, c - 1)
        xt = x.gather(1, tc[:, None])
        rows = torch.where(valid, torch.logsumexp(x, 1) - xt[:, 0], torch.zeros_like(xt[:, 0]))
        idx = torch.arange(c, device=x.device)
        rank = ((x > xt) | ((x == xt) & (idx[None, :] < tc[:, None]))).sum(1)
        ok = valid & torch.isfinite(xt[:, 0])
        loss = rows.sum() * inv_n
        hits1, hitsk = (ok & (rank == 0)).sum().double(), (ok & (rank < min(self.topk, c))).sum().double()
        self.record += torch.stack([loss, hits1 * (100.0 * inv_n), hitsk * (100.0 * inv_n), torch.ones((), dtype=torch.float64, device=x.device)]).to(self.record.device)
        return loss

    def update(self, logits, target, loss=None):
        """Adds a batch: the fused launch on the device, the torch definition on the CPU.  `loss` (a scalar tensor): the batch loss to record in place of the
        cross-entropy of `logits` (a criterion of the caller's own).  Returns the loss that was recorded."""
        if not logits.is_cuda:
            before = self.record[0].clone()
            ce = self.update_reference(logits, target)
        else:
            self._check(logits, target)
            before = self.record[0].clone() if loss is not None else None
            ce = self._launch(logits.detach().contiguous().float(), target, None)
        if loss is None:
            return ce
        self.record[0] = before + loss.detach().double().reshape(())
        return loss

    def read(self):
        """(mean loss, mean top-1 %, mean top-k %) over the batches seen since `reset()`: one device -> host read."""
        loss, a1, ak, nb = self.record.tolist()
        if nb == 0:
            raise ValueError("EpochMeter.read: no batch since reset()")
        return loss / nb, a1 / nb, ak / nb


class _CEMetricsFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target, meter):
        x = logits.contiguous().float()
        dlogits = torch.empty_like(x) if ctx.needs_input_grad[0] else None            # validation under no_grad: loss and metrics only
        loss = meter._launch(x, target, dlogits)
        ctx.save_for_backward(dlogits)
        return loss

    @staticmethod
    def backward(ctx, g):
        (dlogits,) = ctx.saved_tensors
        return dlogits * g, None, None


class CrossEntropyWithMetrics(torch.nn.Module):
    """`CrossEntropyLoss` (same contract: (N, C) fp32 logits, (N,) int64 targets, loss and dlogits from one launch, capturable) whose launch also adds the batch's
    loss, top-1 and top-k hits to `meter` (an `EpochMeter`).  Works under `torch.no_grad()` (no dlogits) and as `parallel.SegmentedStep`'s criterion."""

    def __init__(self, meter):
        super().__init__()
        self.meter = meter

    def forward(self, logits, target):
        if not logits.is_cuda:
            self.meter.update_reference(logits, target)
            return torch.nn.functional.cross_entropy(logits, target, reduction="sum") / logits.size(0)
        if target.dtype != torch.int64 or target.dim() != 1 or logits.dim() != 2:
            raise ValueError("CrossEntropyWithMetrics expects (N, C) logits and (N,) int64 class indices")
        return _CEMetricsFunction.apply(logits, target, self.meter)


def make_param_groups(model, weight_decay):
    groups = []
    others = weight_decay * 0.01
    for _, value in model.named_parameters():
        if len(value.shape) == 4:
            groups.append({"params": [value], "weight_decay": 0.0 if value.shape[1] == 1 else weight_decay})
        else:
            groups.append({"params": [value], "weight_decay": others})
    return groups


def cosine_lr(lr, warmup_lr, warmup_epochs, epochs, epoch, it, dataset_len):
    total_iter = (epochs - warmup_epochs) * dataset_len
    current_iter = it + (epoch - warmup_epochs) * dataset_len
    if epoch < warmup_epochs:
        return warmup_lr + (lr - warmup_lr) * float(it + epoch * dataset_len) / (warmup_epochs * dataset_len)
    return lr / 2 * (math.cos(math.pi * current_iter / total_iter) + 1)


def adjust_learning_rate_cosine(optimizer, epoch, it, dataset_len, args):
    """args: .anneal, .restart_epochs, .epochs, .warmup_epochs, .warmup_lr, .lr (same attribute names as the reference)."""
    if getattr(args, "anneal", False):
        epoch = epoch % args.restart_epochs
        epochs = args.restart_epochs
    else:
        epochs = args.epochs
    lr = cosine_lr(args.lr, args.warmup_lr, args.warmup_epochs, epochs, epoch, it, dataset_len)
    for group in optimizer.param_groups:
        group["lr"] = lr
    return lr


def accuracy(output, target, topk=(1,)):
    with torch.no_grad():
        maxk = max(topk)
        _, pred = output.topk(maxk, 1, True, True)
        correct = pred.t().eq(target.view(1, -1).expand(maxk, -1))
        return [correct[:k].reshape(-1).float().sum(0, keepdim=True).mul_(100.0 / target.size(0)) for k in topk]


def train_one_iter(model, criterion, optimizer, x, target, grad_sync=None):
    """zero_grad -> forward -> loss -> backward -> (DP all-reduce) -> step   (helper_functions.py:139-143)."""
    optimizer.zero_grad(set_to_none=True)
    out = model(x)
    loss = criterion(out, target)
    loss.backward()
    if grad_sync is not None:
        grad_sync.finish()
    optimizer.step()
    return loss, out


def statassist_qat_switch(model, optimizer, qconfig_version=0, backend="qnnpack"):
    """After the FP warm-up epoch(s): turn GradBoost noise on and switch the model to fake-quant mode.  prepare_qat reuses
    the same Parameter objects, so the optimizer's moments / exp_max statistics stay attached."""
    from .frostnet import qat_prepare
    if hasattr(optimizer, "is_warmup"):
        optimizer.is_warmup = False
    before = [id(p) for p in model.parameters()]
    qat_prepare(model, version=qconfig_version, backend=backend)
    assert before == [id(p) for p in model.parameters()], "prepare_qat must keep parameter identity"
    return model


def _device_of(model):
    return next(model.parameters()).device


def _epoch(loader, model, criterion, optimizer, epoch, args, grad_sync, train_mode, transform=None, ema=None):
    dev = _device_of(model)
    sums, n = torch.zeros(3, dtype=torch.float64, device=dev), 0
    for i, batch in enumerate(loader):
        if transform is None:
            inp, target = batch
            inp = inp.to(dev, non_blocking=True)
        else:                                    # (images uint8 [N, Hmax, Wmax, 3], sizes int32 [N, 2], target): the transform runs on the device, in front of the model
            images, sizes, target = batch
            inp = transform(images.to(dev, non_blocking=True), sizes.to(dev, non_blocking=True))
        target = target.to(dev, non_blocking=True)
        if train_mode:
            if args is not None and getattr(args, "lrsch", "cos_lr") == "cos_lr" and hasattr(args, "dataset_len"):
                adjust_learning_rate_cosine(optimizer, epoch, i, args.dataset_len, args)
            loss, out = train_one_iter(model, criterion, optimizer, inp, target, grad_sync)
            if ema is not None:
                ema.update(model)
        else:
            with torch.no_grad():
                out = model(inp)
                loss = criterion(out, target)
        acc1, acc5 = accuracy(out, target, topk=(1, min(5, out.shape[1])))
        sums += torch.stack([loss.detach().double().reshape(()), acc1[0].double(), acc5[0].double()])
        n += 1
    if n == 0:
        raise ValueError("empty loader")
    loss, a1, a5 = (sums / n).tolist()           # the epoch's single device -> host read
    return loss, a1, a5


def train(train_loader, model, criterion, optimizer, epoch, total_ep=None, args=None, grad_sync=None, transform=None, graph=False, ema=None):
    """One training epoch (helper_functions.py:99-163): returns (mean loss, mean top-1, mean top-5) over the iterations.  With a `transform` (a
    `ClassificationAugmentation`) the loader yields (images uint8, sizes, target) in `pad_images`' format and the transform turns them into the model's input on the device.
    `graph`: True drives a `GraphedStep` made for this call (the iteration replayed as one hipGraph, loss and accuracies summed by the loss kernel into an `EpochMeter`);
    pass a `GraphedStep` of your own so that the capture survives across epochs.  `ema` (a `frostnet_amd.ema.ModelEma`): updated after every optimizer step, inside the
    captured iteration when there is one; validate `ema.module`."""
    model.train()
    if graph is not False and graph is not None:
        return _epoch_graphed(train_loader, _graphed(graph, model, criterion, optimizer, transform, grad_sync, ema), epoch, args, True)
    return _epoch(train_loader, model, criterion, optimizer, epoch, args, grad_sync, True, transform, ema)


def val(val_loader, model, criterion, transform=None, graph=False):
    """One validation pass (helper_functions.py:306-350): `model.eval()` only -- BatchNorm uses its running statistics while every FakeQuantize
    observer that has not been disabled explicitly keeps updating, exactly as the reference's val() leaves them.  `transform` (a `ClassificationEvalTransform`): as in `train`.
    `graph`: as in `train` (a `GraphedStep` without an optimizer)."""
    model.eval()
    if graph is not False and graph is not None:
        return _epoch_graphed(val_loader, _graphed(graph, model, criterion, None, transform, None), 0, None, False)
    return _epoch(val_loader, model, criterion, None, 0, None, None, False, transform)


def calibrate(loader, model, transform=None):
    """The calibration loop of the post-training flow (the reference's "Post quantization examples": training images through the prepared model before
    torch.quantization.convert): every batch of `loader` through the PTQ-prepared `model` (frostnet.ptq_prepare) in eval mode under torch.no_grad(), so that
    its HistogramObservers see them -- on the device when the model lives there (frostnet_amd.ptq.PtqRunner: no host synchronisation per batch).  Batches are
    `(input, ...)` tuples or, with a `transform` (a `ClassificationEvalTransform`), `(images uint8, sizes, ...)` as in `val`.  Returns the number of batches."""
    model.eval()
    dev = _device_of(model)
    n = 0
    with torch.no_grad():
        for batch in loader:
            if transform is None:
                inp = (batch[0] if isinstance(batch, (tuple, list)) else batch).to(dev, non_blocking=True)
            else:
                inp = transform(batch[0].to(dev, non_blocking=True), batch[1].to(dev, non_blocking=True))
            model(inp)
            n += 1
    if n == 0:
        raise ValueError("empty loader")
    return n


def val_detector(loader, model, evaluator, top_k=200, conf_thresh=0.01, nms_thresh=0.45):
    """One validation pass of the detector: `model.eval()`, then for every (images, gt [N, G, 5], difficult [N, G], valid [N, G], sizes [N, 2] or None) of the
    loader (ssdlite.pad_targets / voc_eval.pad_difficult turn ragged targets into these) the detections [N, C, top_k, 5] go into `evaluator.update` -- from
    `model.hip_detect_bf16` when the model is the float detector on the device, from `model.hip_detect_int8` when it is the hip_convert()-ed detector on the
    device, from `model.detect` otherwise.  Returns (mean AP, per-class AP list) after the
    evaluation's single read of the results; the evaluator is reset first and keeps the evaluation's state (counts, records) afterwards."""
    model.eval()
    dev = _device_of(model)
    is_qat = getattr(model, "_is_qat_prepared", None)
    bf16 = dev.type == "cuda" and hasattr(model, "hip_detect_bf16") and not (is_qat() if is_qat is not None else False) \
        and not getattr(model, "_hip_converted", False)
    int8 = dev.type == "cuda" and hasattr(model, "hip_detect_int8") and bool(getattr(model, "_hip_converted", False))      # (bit-equal to model.detect)
    detect = model.hip_detect_bf16 if bf16 else (model.hip_detect_int8 if int8 else model.detect)
    evaluator.reset()
    n = 0
    for images, gt, difficult, valid, sizes in loader:
        x = images.to(dev, non_blocking=True)
        det = detect(x, top_k, conf_thresh, nms_thresh)
        evaluator.update(det, gt.to(dev, non_blocking=True), difficult.to(dev, non_blocking=True), valid.to(dev, non_blocking=True),
                         None if sizes is None else sizes.to(dev, non_blocking=True))
        n += 1
    if n == 0:
        raise ValueError("empty loader")
    out = evaluator.compute(check_overflow=False)
    vals = torch.cat([evaluator.overflowed().double().reshape(1), out["mean_ap"].reshape(1), out["ap"]]).tolist()          # the evaluation's single device -> host read
    if vals[0] != 0:
        raise RuntimeError(evaluator.OVERFLOW_MSG)
    return vals[1], vals[2:]


def _seg_epoch(model, loader, optimizer, criterion, num_classes, device, transform=None):
    """The body of train_seg (optimizer given) and val_seg: the counts in a `SegMeter`, the sample-weighted loss sum on the device, ONE host read at the end."""
    from .seg import SegMeter, SegmentationLoss
    dev = device
    if dev is None:
        p = next(model.parameters(), None)
        dev = p.device if p is not None else None
    meter, loss_sum, samples = None, None, 0
    fused = isinstance(criterion, SegmentationLoss)          # the criterion's own launch counts the batch
    saved = criterion.meter if fused else None
    try:
        for batch in loader:
            if transform is None:
                inputs, target = batch
                if dev is not None:
                    inputs, target = inputs.to(dev, non_blocking=True), target.to(dev, non_blocking=True)
            else:                                # (images uint8 [N, Hmax, Wmax, 3], labels uint8 [N, Hmax, Wmax], sizes int32 [N, 2]): the transform runs on the device, in front of the model
                images, labels, sizes = batch
                if dev is not None:
                    images, labels, sizes = images.to(dev, non_blocking=True), labels.to(dev, non_blocking=True), sizes.to(dev, non_blocking=True)
                inputs, target = transform(images, labels, sizes)
            if meter is None:
                meter = SegMeter(num_classes, target.device)
                if fused:
                    criterion.meter = meter
            outputs = model(inputs)
            if isinstance(outputs, list):
                outputs = tuple(outputs)
            if criterion is not None:
                loss = criterion(outputs, target)
                loss = loss.mean() if loss.dim() else loss
                w = loss.detach().double() * inputs.size(0)
                loss_sum = w if loss_sum is None else loss_sum + w
            if not fused:
                meter.update(outputs, target)
            samples += inputs.size(0)
            if optimizer is not None:
                optimizer.zero_grad()
                loss.backward()
                optimizer.step()
    finally:
        if fused:
            criterion.meter = saved
    if meter is None:
        raise ValueError("empty loader")
    miou = meter.compute()
    return miou, (float(loss_sum) / samples if loss_sum is not None else 0)


def train_seg(model, dataset_loader, optimizer, criterion, num_classes, epoch=0, device=None, transform=None):
    """One training epoch of Semantic_Segmentation/utilities/train_eval_seg.py:train_seg for any module that returns logits (or a tuple of them) -> (mean IoU in
    percent over the epoch, sample-weighted mean loss).  With a `seg.SegmentationLoss` criterion the loss launch also counts the batch; any other criterion is
    followed by `SegMeter.update`.  `device` defaults to the model's.  With a `transform` (a `seg_augment.SegmentationAugmentation`) the loader yields (images uint8,
    labels uint8, sizes) in `pad_pairs`' format and the transform turns them into the model's input and the target on the device."""
    model.train()
    return _seg_epoch(model, dataset_loader, optimizer, criterion, num_classes, device, transform)


def val_seg(model, dataset_loader, criterion=None, num_classes=21, device=None, transform=None):
    """train_eval_seg.py:val_seg -> (mean IoU in percent, sample-weighted mean loss, or 0 without a criterion), under `torch.no_grad()`.  `transform` (a
    `seg_augment.SegmentationEvalTransform`): as in `train_seg`."""
    model.eval()
    with torch.no_grad():
        return _seg_epoch(model, dataset_loader, None, criterion, num_classes, device, transform)


def _is_plain_ce(criterion):
    if isinstance(criterion, CrossEntropyLoss):
        return True
    return (type(criterion) is torch.nn.CrossEntropyLoss and criterion.weight is None and criterion.reduction == "mean" and criterion.ignore_index == -100
            and getattr(criterion, "label_smoothing", 0.0) == 0.0)


class _Captured:
    """One captured input signature of a GraphedStep: static inputs, their staging buffers, the graph(s) and what they were captured against."""
    __slots__ = ("statics", "staging", "graph", "seg", "plan", "runner", "training", "logits", "staged", "free", "rows", "dp_in", "ema_plan", "ema_id")


class GraphedStep:
    """One loop iteration as a replayed hipGraph -- what `bench.py` times, for the loops a user calls.

    `step(*batch) -> loss` (a persistent device scalar; nothing synchronises with the host).  With an `optimizer` it is a training iteration (transform -> zero_grad ->
    forward -> loss -> backward -> optimizer launch), without one a validation forward under `no_grad`.  `batch` is what the loader yields: classifier `(inp, target)`, or
    `(images, sizes, target)` with a `transform` (`ClassificationAugmentation` / `ClassificationEvalTransform`); detector (`criterion` is a `ssdlite.MultiBoxLoss`)
    `(images, boxes, valid)`, or `(images, sizes, boxes, valid)` with a `transform` (`SSDAugmentation`).

    The first `eager_warmup` calls of an input signature (shapes and dtypes) run eagerly (descriptor tables, optimizer state, coefficient caches); the next one captures the
    iteration on a side stream (`optimizer.prepare_step()` in front of the capture, `optimizer.launch(plan)` inside it); later calls copy the batch into the graph's static
    inputs, call `optimizer.prepare_step()` and replay.  A pinned host batch travels on a copy stream into a staging buffer while the previous replay runs and from there
    in-stream into the static input; a device batch is copied in-stream.  Graphs exist for at most two signatures (the full batch and a smaller last one); anything else runs
    eagerly.  Live at every replay because they stay outside the graph: per-group lr / weight_decay and `is_warmup` (uploaded by `prepare_step`), the Philox offset, the
    augmentation and dropout stream positions (device words).  The step is captured AGAIN, never replayed stale, when the model's runner is no longer valid, when the
    optimizer's plan changed (`load_state_dict`, `add_param_group`) or when `model.training` differs from the capture.

    `ema` (a `frostnet_amd.ema.ModelEma`): the weight average moves after every optimizer step -- eagerly `ema.update(model)`, on the captured path `ema.prepare_step()` next to
    the optimizer's in front of capture and replay (w = 1 - decay_t is a device word outside the graph, the pointer table is revalidated there) and `ema.launch(plan)`
    recorded right behind `optimizer.launch(plan)`.  The shadow's runner is bound during the eager warm-up calls so that its table settles before the capture; the step is
    captured again when `ema.plan_id` changed.  Data parallel: the launch follows the optimizer's on every rank, no collective (equal parameters, equal shadows).

    Data parallel (`group` given, or a default process group of more than one rank): the body is `parallel.SegmentedStep` (capture / replay / finish, then the optimizer
    launch); collectives are never captured.  A float model (StatAssist warm-up: `FloatRunner`, `FloatSSDRunner`), a CPU model and an optimizer without `prepare_step` /
    `launch` run the same iteration eagerly (the float step measured slower replayed than eager) -- still with the fused metrics.

    Classifier metrics go to `meter` (an `EpochMeter`: the criterion's own when it is a `CrossEntropyWithMetrics`; a plain cross-entropy criterion is replaced by one); the
    logits of the last iteration are `logits`.  Detector: `record` = three device doubles {sum loss_l, sum loss_c, batches}, `loss_terms` = the last (loss_l, loss_c)."""

    def __init__(self, model, criterion, optimizer=None, transform=None, nbuckets=4, group=None, eager_warmup=2, ema=None):
        from .ssdlite import MultiBoxLoss
        self.model, self.optimizer, self.transform, self.nbuckets, self.group = model, optimizer, transform, nbuckets, group
        if ema is not None and optimizer is None:
            raise ValueError("GraphedStep(ema=...) averages the weights after the optimizer step: it needs an optimizer")
        self.ema = ema
        self.eager_warmup = max(int(eager_warmup), 1 if optimizer is not None else 0)          # the optimizer's table is built from the gradients of a first eager step
        self.device = dev = _device_of(model)
        self.detector = isinstance(criterion, MultiBoxLoss)
        self.meter, self.record, self.loss_terms, self._own_loss = None, None, None, False
        if self.detector:
            self.criterion = criterion
            self.record = torch.zeros(3, dtype=torch.float64, device=dev)
            self.loss_terms = torch.zeros(2, dtype=torch.float32, device=dev)
        elif isinstance(criterion, CrossEntropyWithMetrics):
            self.criterion, self.meter = criterion, criterion.meter
        elif _is_plain_ce(criterion):
            self.meter = EpochMeter(dev)
            self.criterion = CrossEntropyWithMetrics(self.meter)
        else:                                         # a criterion of the caller's own: its loss is recorded, the hits come from one metrics-only launch
            self.criterion, self.meter, self._own_loss = criterion, EpochMeter(dev), True
        self.loss = torch.zeros((), dtype=torch.float32, device=dev)
        self.logits = None
        self.capture = True                           # False: the same iteration with eager launches throughout
        self.captures = 0                             # how many times a graph was captured (tests, tools)
        self._graphs, self._seen, self._copy_stream, self._seg_eager = {}, {}, None, None

    # ---- what is captured ----
    def _data_parallel(self):
        if self.optimizer is None:
            return False
        import torch.distributed as dist
        return self.group is not None or (dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1)

    def _capturable(self):
        m, o = self.model, self.optimizer
        if self.device.type != "cuda" or not hasattr(m, "hip_runner") or not m._is_qat_prepared() or getattr(m, "_hip_converted", False):
            return False
        return o is None or (hasattr(o, "prepare_step") and hasattr(o, "launch"))

    def graph_for(self, *batch):
        """The captured graph object of this batch's signature (None while it runs eagerly; a list of segment graphs on the data-parallel path)."""
        g = self._graphs.get(self._signature(batch))
        return None if g is None else (g.graph if g.seg is None else g.seg.graphs)

    @staticmethod
    def _signature(batch):
        return tuple((tuple(t.shape), t.dtype) for t in batch)

    def _split(self, batch):
        """-> (model input, target) from a device batch; the transform runs here, in front of the model."""
        if self.detector:
            if self.transform is None:
                images, boxes, valid = batch
                return images, (boxes, valid)
            images, sizes, boxes, valid = batch
            x, boxes, valid = self.transform(images, sizes, boxes, valid)
            return x, (boxes, valid)
        if self.transform is None:
            return batch
        images, sizes, target = batch
        return self.transform(images, sizes), target

    def _record_detector(self, ll, lc):
        terms = torch.stack([ll.detach(), lc.detach()]).float()
        self.loss_terms.copy_(terms)
        self.record[:2] += terms.double()
        self.record[2] += 1.0

    def _loss_of(self, out, target):
        if self.detector:
            ll, lc = self.criterion(out, target)
            self._record_detector(ll, lc)
            return ll + lc
        loss = self.criterion(out, target)
        if self._own_loss:
            self.meter.update(out, target, loss=loss)
        return loss

    def _forward_backward(self, batch):
        """The iteration without its optimizer step, from a device batch (eager, or recorded into a capture)."""
        x, target = self._split(batch)
        if self.optimizer is None:
            with torch.no_grad():
                out = self.model(x)
                loss = self._loss_of(out, target)
        else:
            self.optimizer.zero_grad(set_to_none=True)
            out = self.model(x)
            loss = self._loss_of(out, target)
            loss.backward()
        self.loss.copy_(loss.detach().reshape(()))
        return None if self.detector else out.detach()

    # ---- data parallel: parallel.SegmentedStep is the body ----
    def _segmented(self):
        from .parallel import SegmentedStep
        runner = self.model.hip_runner()
        if self.detector:
            def maps_loss(maps, target):
                ll, lc = self.criterion(self.model._assemble(maps), target)
                self._record_detector(ll, lc)
                return ll + lc
            return SegmentedStep(runner, nbuckets=self.nbuckets, group=self.group, maps_loss=maps_loss)
        if self._own_loss:
            def crit(logits, target):
                loss = self.criterion(logits, target)
                self.meter.update(logits, target, loss=loss)
                return loss
            return SegmentedStep(runner, crit, nbuckets=self.nbuckets, group=self.group)
        return SegmentedStep(runner, self.criterion, nbuckets=self.nbuckets, group=self.group)

    def _eager_segmented(self, batch):
        if self._seg_eager is None or self._seg_eager.runner is not self.model.hip_runner():
            self._seg_eager = self._segmented()
        x, target = self._split(batch)
        self.loss.copy_(self._seg_eager.run_eager(x, target))
        self._seg_eager.finish()
        self.optimizer.step()
        self._ema_eager()
        self.logits = None
        return self.loss

    # ---- eager ----
    def _to_device(self, batch):
        return tuple(t.to(self.device, non_blocking=True) for t in batch)

    def _eager(self, batch):
        batch = self._to_device(batch)
        if self.optimizer is not None and not self.model.training:
            raise RuntimeError("GraphedStep with an optimizer is a training iteration: call model.train() first")
        if self._data_parallel():
            if not self._capturable():
                raise NotImplementedError("GraphedStep: the data-parallel body (parallel.SegmentedStep) binds the fake-quantised model on the device; run this model "
                                          "through train(..., graph=False, grad_sync=...)")
            return self._eager_segmented(batch)
        self.logits = self._forward_backward(batch)
        if self.optimizer is not None:
            self.optimizer.step()
            self._ema_eager()
        return self.loss

    def _ema_eager(self):
        if self.ema is not None:
            self.ema.bind_shadow()            # (once: the shadow's runner re-aliases its buffers; later calls find it)
            self.ema.update(self.model)

    # ---- input copy ----
    def _load(self, g, batch):
        cur = torch.cuda.current_stream(self.device)
        host = [i for i, t in enumerate(batch) if not t.is_cuda]
        if host:
            if self._copy_stream is None:
                self._copy_stream = torch.cuda.Stream(device=self.device)
            cs = self._copy_stream
            if g.free is not None:
                cs.wait_event(g.free)                 # the previous in-stream copy has read the staging buffers
            with torch.cuda.stream(cs):
                for i in host:
                    g.staging[i].copy_(batch[i], non_blocking=True)          # (a pinned batch: asynchronous, beside the previous replay)
            g.staged.record(cs)
            cur.wait_event(g.staged)
        for i, t in enumerate(batch):
            g.statics[i].copy_(g.staging[i] if not t.is_cuda else t, non_blocking=True)
        if host:
            if g.free is None:
                g.free = torch.cuda.Event()
            g.free.record(cur)

    # ---- capture / replay ----
    def _capture(self, sig, batch, plan, ema_plan=None):
        dev = self.device
        g = _Captured()
        g.statics = [torch.empty(t.shape, dtype=t.dtype, device=dev) for t in batch]
        g.staging = [None if t.is_cuda else torch.empty(t.shape, dtype=t.dtype, device=dev) for t in batch]
        g.staged, g.free, g.graph, g.seg, g.logits, g.dp_in, g.rows = torch.cuda.Event(), None, None, None, None, None, batch[0].size(0)
        g.runner, g.training, g.plan = self.model.hip_runner(), self.model.training, plan
        g.ema_plan, g.ema_id = ema_plan, None if ema_plan is None else ema_plan["id"]
        self._load(g, batch)
        import torch.distributed as dist
        with torch.cuda.device(dev):
            if self._data_parallel():
                g.seg = self._segmented()
                x, target = self._split(tuple(g.statics))          # the transform stays in front of the segments: launched in-stream at every step
                g.dp_in = (x,) + (tuple(target) if isinstance(target, tuple) else (target,))
                g.seg.capture(x, target)
            else:
                side = torch.cuda.Stream(device=dev)
                side.wait_stream(torch.cuda.current_stream(dev))
                with torch.cuda.stream(side):
                    g.graph = torch.cuda.CUDAGraph()
                    # (a process group's watchdog thread polls events concurrently: restrict the capture check to this thread when one exists)
                    with torch.cuda.graph(g.graph, stream=side, capture_error_mode="thread_local" if dist.is_available() and dist.is_initialized() else "global"):
                        g.logits = self._forward_backward(tuple(g.statics))
                        if self.optimizer is not None:
                            self.optimizer.launch(plan)
                        if ema_plan is not None:
                            self.ema.launch(ema_plan)
                torch.cuda.current_stream(dev).wait_stream(side)
        self.captures += 1
        self._graphs[sig] = g
        return g

    def _replay(self, g, captured_now=False):
        if g.seg is not None:
            if self.transform is not None and not captured_now:            # the segments read the transform's output where the capture left it (and just made it)
                x, target = self._split(tuple(g.statics))
                for dst, src in zip(g.dp_in, (x,) + (tuple(target) if isinstance(target, tuple) else (target,))):
                    if dst is not src:
                        dst.copy_(src)
            g.seg.replay()
            g.seg.finish()
            self.optimizer.launch(g.plan)
            if g.ema_plan is not None:
                self.ema.launch(g.ema_plan)
            self.loss.copy_(g.seg.loss)
        else:
            g.graph.replay()
        self.logits = g.logits
        return self.loss

    def step(self, *batch):
        if not self.capture or not self._capturable():
            return self._eager(batch)
        if self.optimizer is not None and not self.model.training:
            raise RuntimeError("GraphedStep with an optimizer is a training iteration: call model.train() first (the training graph is never replayed in eval mode)")
        sig = self._signature(batch)
        runner = self.model.hip_runner()
        if any(c.runner is not runner for c in self._graphs.values()):          # parameters or buffers moved: every graph holds stale pointers, and the new runner starts cold
            self._graphs.clear()
            self._seen.clear()
        g = self._graphs.get(sig)
        if g is not None and g.training != self.model.training:
            del self._graphs[sig]
            g = None
        rows = batch[0].size(0)
        if g is None:
            seen = self._seen.get(sig, 0)
            # a second graph only for a batch no larger than the first one's (the last, partial batch): the engine grows some work buffers on demand, and a
            # larger batch would replace them under the graph that was captured with them -- such a batch runs eagerly, and the graphs are captured again after it
            fits = all(rows <= c.rows for c in self._graphs.values())
            if seen < self.eager_warmup or len(self._graphs) >= 2 or not fits:
                self._seen[sig] = seen + 1
                if not fits:
                    self._graphs.clear()
                return self._eager(batch)
            plan = self.optimizer.prepare_step() if self.optimizer is not None else None
            ema_plan = self.ema.prepare_step(self.model) if self.ema is not None else None
            g = self._capture(sig, batch, plan, ema_plan)
            return self._replay(g, captured_now=True)
        self._load(g, batch)
        if self.optimizer is not None:
            plan = self.optimizer.prepare_step()
            ema_plan = self.ema.prepare_step(self.model) if self.ema is not None else None
            # load_state_dict / add_param_group: the captured launch reads the old table; an EMA plan rebuilt for other entries likewise
            if plan is not g.plan or (ema_plan is not None and (ema_plan is not g.ema_plan or ema_plan["id"] != g.ema_id)):
                del self._graphs[sig]
                return self._replay(self._capture(sig, batch, plan, ema_plan), captured_now=True)
        return self._replay(g)

    __call__ = step

    # ---- the detector's record ----
    def reset_record(self):
        (self.record if self.detector else self.meter.record).zero_()

    def read_record(self):
        """Detector: (mean loss_l, mean loss_c) over the iterations since `reset_record()`; classifier: the meter's triple.  One host read."""
        if not self.detector:
            return self.meter.read()
        sl, sc, nb = self.record.tolist()
        if nb == 0:
            raise ValueError("GraphedStep.read_record: no iteration since reset_record()")
        return sl / nb, sc / nb


def _graphed(graph, model, criterion, optimizer, transform, grad_sync, ema=None):
    if grad_sync is not None:
        raise ValueError("graph=True exchanges the gradients itself (parallel.SegmentedStep between the graph's segments): pass a GraphedStep(..., group=...) "
                         "instead of grad_sync")
    if isinstance(graph, GraphedStep):
        if graph.model is not model or graph.optimizer is not optimizer or graph.transform is not transform:
            raise ValueError("graph=<GraphedStep>: it was built for another model, optimizer or transform")
        if ema is not None and graph.ema is not ema:
            raise ValueError("graph=<GraphedStep>: it was built without this ema (GraphedStep(..., ema=ema))")
        return graph
    return GraphedStep(model, criterion, optimizer, transform, ema=ema)


def _epoch_graphed(loader, step, epoch, args, train_mode):
    step.reset_record()
    n = 0
    for i, batch in enumerate(loader):
        if train_mode and args is not None and getattr(args, "lrsch", "cos_lr") == "cos_lr" and hasattr(args, "dataset_len"):
            adjust_learning_rate_cosine(step.optimizer, epoch, i, args.dataset_len, args)
        step(*batch)
        n += 1
    if n == 0:
        raise ValueError("empty loader")
    return step.read_record()                      # the epoch's single device -> host read


def train_detector(loader, model, criterion, optimizer, start_iter, max_iter, lr, gamma, lr_steps, transform=None, graph=False, ema=None):
    """The detector's training loop (Object_Detection/qtrainval.py:259-304), driven by the iteration count: iterations start_iter .. max_iter - 1, the learning rate set
    to lr * gamma^step_index at every entry of `lr_steps` (:270-272, adjust_learning_rate :336-344), the loader restarted whenever it is exhausted.  The loader yields
    (images, boxes, valid) (ssdlite.pad_targets' format), or (images uint8, sizes, boxes, valid) for a `transform` (an `SSDAugmentation`, on the device in front of the
    model).  `graph`: False = eager launches, True = a `GraphedStep` made here, or a `GraphedStep` of the caller's so that the capture survives across calls.  Returns the
    mean (loss_l, loss_c) over the iterations from one host read.  `ema`: as in `train`."""
    model.train()
    if isinstance(graph, GraphedStep):
        step = _graphed(graph, model, criterion, optimizer, transform, None, ema)
    else:
        step = GraphedStep(model, criterion, optimizer, transform, ema=ema)
        step.capture = bool(graph)
    if not step.detector:
        raise ValueError("train_detector: criterion must be a ssdlite.MultiBoxLoss")
    step.reset_record()
    step_index = sum(1 for s in lr_steps if s < start_iter)
    it_loader = None
    for iteration in range(start_iter, max_iter):
        if iteration in lr_steps:
            step_index += 1
            for group in optimizer.param_groups:
                group["lr"] = lr * (gamma ** step_index)
        try:
            if it_loader is None:
                it_loader = iter(loader)
            batch = next(it_loader)
        except StopIteration:
            it_loader = iter(loader)
            try:
                batch = next(it_loader)
            except StopIteration:
                raise ValueError("empty loader") from None
        step(*batch)
    return step.read_record()


def checkpoint_state(model, optimizer, epoch, ema=None, **scalars):
    """The dictionary Classification/train.py:208-218 saves every epoch (same keys; `scalars` = lossTr, lossVal, acc1Tr, ... , lr, Max_name ...).  With `ema` (a
    `ModelEma`) also `state_dict_ema` -- the shadow's state_dict, the key timm writes and `frostnet_features` prefers on ingest -- and `ema_updates`."""
    state = {"epoch": epoch + 1, "arch": str(type(model).__name__), "state_dict": model.state_dict(), "optimizer": optimizer.state_dict()}
    if ema is not None:
        state["state_dict_ema"] = ema.module.state_dict()
        state["ema_updates"] = ema.updates
    state.update(scalars)
    runner = getattr(model, "_hip_runner", None)
    if runner is not None and hasattr(runner, "rng_state"):
        state["hip_rng"] = runner.rng_state()
    return state


def save_checkpoint(state, filenameCheckpoint="checkpoint.pth.tar"):
    torch.save(state, filenameCheckpoint)


def load_checkpoint(model, optimizer, filenameCheckpoint="checkpoint.pth.tar", map_location=None, ema=None):
    """Resume: parameters / buffers (BN statistics, observer ranges, qparams), optimizer state (GradBoost statistics, step count = Philox offset),
    the dropout stream and, with `ema`, the weight average and its update count.  Returns the checkpoint dictionary (epoch, best accuracies ...)."""
    ck = torch.load(filenameCheckpoint, map_location=map_location, weights_only=False)
    model.load_state_dict(ck["state_dict"])
    if ema is not None:
        if "state_dict_ema" not in ck:
            raise KeyError(f"{filenameCheckpoint} holds no weight average (state_dict_ema)")
        ema.module.load_state_dict(ck["state_dict_ema"])
        ema.updates = int(ck.get("ema_updates", 0))
    if optimizer is not None and "optimizer" in ck:
        optimizer.load_state_dict(ck["optimizer"])
    if "hip_rng" in ck and hasattr(model, "hip_runner"):
        dev = _device_of(model)
        if dev.type == "cuda":
            r = model.hip_runner()
            if hasattr(r, "set_rng_state"):
                r.set_rng_state(ck["hip_rng"])
    return ck
