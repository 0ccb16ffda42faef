"""Fused training step: the loop body of reference trains.py:113-135
(forward, BCEDiceLoss (mean over heads under deep supervision, :118-124), IoU on
the last head, backward, SGD(momentum, wd) :229-231,133 or Adam :225-227) enqueued as ONE hipGraph
replay per step, with no host synchronisation: loss and IoU counts stay on the
device and are read back only when the caller asks (AverageMeter semantics of
utils.py:17-33 are kept by `epoch_stats`).

Data parallel (new capability): one process per GPU, one gradient
all-reduce per step over RCCL, buckets in gradient-ready order. Replica state:
  * parameters, optimiser state and BatchNorm buffers are broadcast from rank 0 when the
    TrainStep is built (what DistributedDataParallel does at construction), so ranks
    that initialised differently or loaded a checkpoint on rank 0 only start identical;
  * BatchNorm batch statistics stay LOCAL to a replica (plain nn.BatchNorm2d semantics,
    archs1.py:19,21: every replica normalises over its own 16 images, exactly like the
    single-GPU reference step); the running statistics therefore drift apart between
    ranks, and the policy is "rank 0's buffers are the model's": sync_bn_buffers()
    broadcasts them before validation / checkpointing (train.py does);
  * p.grad holds the rank-MEAN gradient in every step layout (as DDP leaves it).
"""
import ctypes as C
import math
import os

import torch
import torch.distributed as dist

from . import _lib as L
from . import loss_scale as LS
from .dataset import _check_aug
from .optim_state import flat_to_torch_state, torch_state_to_flat
from .parallel import allreduce_flat_, broadcast_flat_


def dp_layout_from_env(environ):
    """(layout, auto) of the data-parallel step from NUNET_DP_MODE: unset / 'auto' -> (1, True), '1' -> (1, False),
    '3' -> (3, False); any other value raises. No GPU use."""
    mode = environ.get("NUNET_DP_MODE", "auto")
    if mode not in ("auto", "1", "3"):
        raise L.NunetError("TrainStep: NUNET_DP_MODE %r: the data-parallel step layouts are 1, one exchange of the whole gradient "
                           "scratch behind the backward pass, and 3, both bucket exchanges inside the step's graph (or auto)" % (mode,))
    return (1, True) if mode == "auto" else (int(mode), False)


def fused_update_from(arg, environ):
    """The optimiser step layout from TrainStep's fused_update argument, or NUNET_FUSED_UPDATE when that is None: unset -> 2;
    0 and 2 are accepted, any other value raises. No GPU use."""
    v = environ.get("NUNET_FUSED_UPDATE", "2") if arg is None else arg
    if str(v) not in ("0", "2"):
        raise L.NunetError("TrainStep: fused_update %r: the optimiser step layouts are 0, unpack + the flat step on the flat "
                           "gradients, and 2, the step fused into the unpack of the gradient scratch" % (v,))
    return int(v)


class TrainStep:
    def __init__(self, model, batch_shape, lr=1e-3, momentum=0.9, weight_decay=1e-4, nesterov=False,
                 use_graph=True, process_group=None, keep_grads=True, fused_update=None, loss="BCEDiceLoss", input_u8=False,
                 schedule=None, segmented=None, optimizer="SGD", betas=(0.9, 0.999), eps=1e-8, loss_scale=None,
                 clip_grad_norm=None, ema_decay=None, ema_warmup=False, color_aug=False, resize=False, source_capacity=None):
        """loss: 'BCEDiceLoss' (reference losses.py:103-117, the default of trains.py:58), 'LovaszHingeLoss'
        (losses.py:120-129, the loss of the reference's published table README.md:102-108; one class only) or
        'BCEWithLogitsLoss' (torch.nn.BCEWithLogitsLoss(), trains.py:27-28,210-211; any num_classes: its gradient needs no
        sum, so one pass over logits and targets forms it with the partial sums) - all run inside the step's graph and
        under data parallel.
        input_u8: the step's inputs are the DECODED uint8 batch (images [N,H,W,C], masks [N,H,W,K] in {0,255}) plus optional
        per-sample augmentation codes; Normalize, /255, the mask scaling, rot90 / flips and the layout change of the
        reference's sample pipeline (dataset.py:66-74, trains.py:258-266) run as the first two launches of the step's graph
        (step_u8). Only uint8 crosses PCIe and the per-step NCHW->NHWC launch of the float path is gone.
        color_aug (needs input_u8 and input_channels == 3): False - today's two head launches; True - the staging launch is
        nunet_plan_stage_u8_color, which applies one colour op per sample (the OneOf([HueSaturationValue, RandomBrightness,
        RandomContrast]) of trains.py:260-264, modelled on albumentations / OpenCV) to the source pixel it
        fetches, from a static int32 [N,4] device buffer that step_u8(..., color=) fills (dataset.draw_color_augmentation; None:
        every op NONE, bit-identical to color_aug=False). The same number of launches.
        resize (needs input_u8; source_capacity = bytes of each of the two source pools): False - nothing changes. True - the
        step's inputs are RAGGED: every sample at its own size, as a byte pool plus one descriptor per sample for the images and
        for the masks (dataset.pack_ragged, FolderDataset.batch). The two head launches become nunet_plan_stage_u8_resize
        (augment the source, colour op on every fetched tap, bilinear Resize to the plan's H x W, Normalize: the reference's whole
        train transform, trains.py:257-267) and nunet_preprocess_u8_resize (masks, nearest) reading static pool and descriptor
        buffers that step_u8_ragged() fills, so a captured step replays with new sizes. An odd rot90 count needs no square
        source. The same number of launches; sources of the plan's own size give the bits of resize=False.
        How the captured step is executed (all forms are bit-identical, tests/test_net_gpu.py):
          schedule  'lanes' - every op on its block's lane; 'list' - lanes chosen by a list scheduler over the hazard graph with
                    measured per-op costs (nunet_plan_calibrate)
          segmented False - ONE hipGraph, the lanes as parallel branches (ROCm replays those node by node from the host);
                    'flags' - one single-stream graph per lane, cross-lane dependencies as device-side flags (csrc/graph.hip)
        Both None (default): single-process training times the two executors, (False, 'lanes') against ('flags', 'list'), on the
        captured step and keeps the faster (self.executor_choice); data-parallel training keeps (False, 'lanes'), whose graph can
        hold the RCCL exchange. NUNET_SCHEDULE (lanes | list) / NUNET_SEGMENTED (0 | flags) force a form (tools); any other value raises.
        optimizer: 'SGD' (momentum, weight_decay, nesterov; reference trains.py:229-231) or 'Adam' (betas, eps, weight_decay as
        L2 decay in the gradient, amsgrad off; trains.py:225-227). Either runs inside the step in both fused_update layouts;
        Adam keeps flat exp_avg / exp_avg_sq, a device step counter and the step's two bias-correction scalars, refreshed by a
        1-thread launch at the head of every step (nunet_adam_prepare). optimizer_state_dict() / load_optimizer_state_dict()
        speak torch.optim's state-dict format.
        loss_scale: None (default: no scaling), "dynamic" (torch.amp.GradScaler's defaults) or a dict of GradScaler's constructor
        settings (init_scale, growth_factor, backoff_factor, growth_interval). Dynamic loss scaling on the device, inside the
        captured step: the loss gradient is seeded with the scale, the final gradient scratch is checked for inf / NaN, the update
        unscales it - or, on an overflow, writes nothing (the step is skipped) - and a 1-thread launch backs the scale off or grows
        it as torch's scaler.update() does. No host synchronisation per step; scaler_stats() / scaler_state_dict() read the state.
        clip_grad_norm: None (default: no clipping, today's launches) or max_norm > 0 of torch.nn.utils.clip_grad_norm_(params,
        max_norm) over all parameters, applied inside the captured step between the unscale and the optimiser step: one read-only
        pass takes the 2-norm of the final (rank-mean, unscaled) gradient in double, in a fixed summation order; a one-workgroup
        launch forms coef = min(1, max_norm / (norm + 1e-6)) and the statistics; the update reads g * coef. float('inf')
        measures and never clips (bit-identical to None). set_clip_grad_norm() changes the threshold of a captured step,
        grad_norm_stats() reads the norms.
        ema_decay: None (default: no averaging, today's launches) or a decay in [0, 1): an exponential moving average of the
        weights, torch.optim.swa_utils.AveragedModel(model, multi_avg_fn=get_ema_multi_avg_fn(decay), use_buffers=True) with one
        update_parameters(model) per applied step, inside the captured step. self.ema_params / self.ema_bnbuf (flat fp32, the
        order of Engine.flat_params / Engine.bnbuf) start as copies of the live arenas; the first applied step copies, every
        later one moves them by w = float(1 - d_t) towards the updated parameters (in the update launch, which holds them in
        registers) and the BatchNorm running statistics this step's forward left (one small launch); a step skipped by loss
        scaling leaves the average and n_averaged untouched. ema_warmup: d_t = min(decay, (1 + n_averaged) / (10 + n_averaged)).
        num_batches_tracked is NOT averaged: ema_state_dict() carries the live model's value (torch's integer branch truncates
        the average of a counter to nonsense, and the eval forward never reads it). Under data parallel the average is a
        deterministic function of identical parameters: no collective. EvalStep(weights=(ts.ema_params, ts.ema_bnbuf))
        validates the averaged model; ema_state_dict() / load_ema_state_dict() / ema_stats() speak to the host."""
        self.model = model
        self.eng = model.engine()
        dev = self.eng.device
        n, cin, h, w = batch_shape
        self.n, self.h, self.w = n, h, w
        self.ncls = model.num_classes
        x0 = torch.zeros(batch_shape, dtype=torch.float32, device=dev)
        self.pl = model.plan_for(x0)
        env_sched, env_seg = os.environ.get("NUNET_SCHEDULE"), os.environ.get("NUNET_SEGMENTED")
        self.executor_auto = schedule is None and segmented is None and env_sched is None and env_seg is None
        self.executor_choice = None          # {(segmented, schedule): ms per step} when the form was chosen by timing
        self.schedule = schedule or env_sched or "lanes"
        if segmented is None:
            segmented = {"0": False, "2": "flags"}.get(env_seg or "0", env_seg)
        if self.schedule not in ("lanes", "list") or (segmented is not False and segmented != "flags"):
            raise L.NunetError("TrainStep: schedule %r, segmented %r: the executors are (segmented=False, schedule='lanes'), one multi-branch "
                               "hipGraph, and (segmented='flags', schedule='list'), flag-synchronised lanes" % (self.schedule, segmented))
        self._set_schedule(self.schedule)
        self.segmented = segmented
        self._calibrated = False
        self.dp_exec = (False, "lanes")      # executor of the data-parallel layout 1 pass (see _choose_layout)
        self.heads = self.pl.heads
        self.x = x0
        self.t = torch.zeros((n, self.ncls, h, w), dtype=torch.float32, device=dev)
        self.input_u8 = bool(input_u8)
        if self.input_u8:
            import numpy as np
            from .dataset import MEAN, STD
            self.x_u8 = torch.zeros((n, h, w, cin), dtype=torch.uint8, device=dev)
            self.t_u8 = torch.zeros((n, h, w, self.ncls), dtype=torch.uint8, device=dev)
            self.aug = torch.zeros(n, dtype=torch.int32, device=dev)
            self._mean = torch.tensor(np.resize(np.asarray(MEAN, np.float32), cin), device=dev)
            self._std = torch.tensor(np.resize(np.asarray(STD, np.float32), cin), device=dev)
        self.resize = bool(resize)
        if self.resize:
            if not self.input_u8:
                raise L.NunetError("TrainStep: resize=True needs input_u8=True: the resize runs on the uint8 sources the staging launch fetches")
            if source_capacity is None or int(source_capacity) < 1:
                raise L.NunetError("TrainStep: resize=True needs source_capacity, the bytes of the largest batch of sources "
                                   "(got %r)" % (source_capacity,))
            self.source_capacity = int(source_capacity)
            self.img_pool = torch.zeros(self.source_capacity, dtype=torch.uint8, device=dev)
            self.mask_pool = torch.zeros(self.source_capacity, dtype=torch.uint8, device=dev)
            self.img_desc = torch.zeros((n, L.SAMPLE_WORDS), dtype=torch.int32, device=dev)      # nunet_u8_sample per sample
            self.mask_desc = torch.zeros((n, L.SAMPLE_WORDS), dtype=torch.int32, device=dev)
            self._cin = cin
        self.color = None
        if color_aug:
            if not self.input_u8 or cin != 3:
                raise L.NunetError("TrainStep: color_aug=True needs input_u8=True and RGB input (input_channels == 3): the colour ops "
                                   "run on the uint8 pixel the staging launch fetches")
            self.color = torch.zeros((n, L.COLOR_WORDS), dtype=torch.int32, device=dev)     # nunet_color_aug per sample, all NONE
        self.logits = torch.empty((self.heads, n, self.ncls, h, w), dtype=torch.float32, device=dev)
        self.dlogits = torch.empty_like(self.logits)
        self.per = self.ncls * h * w
        kinds = LOSS_KINDS
        if loss not in kinds:
            raise L.NunetError("TrainStep: loss %r is not one of %s" % (loss, sorted(kinds)))
        if loss == "LovaszHingeLoss" and self.ncls != 1:
            raise L.NunetError("LovaszHingeLoss squeezes the class dimension (reference losses.py:126-127): num_classes must be 1")
        self.loss_name, self.loss_kind = loss, kinds[loss]
        from .metrics import iou_logit_threshold
        self.iou_thr = iou_logit_threshold()
        self.loss_ws = torch.empty((L.lib().nunet_loss_step_ws_bytes(n, self.per, self.heads, self.loss_kind) + 7) // 8, dtype=torch.float64, device=dev)
        self.loss_out = torch.zeros(self.heads + 1, dtype=torch.float32, device=dev)   # per head, then their mean
        # device-side epoch meters: [sum of step losses, sum of step IoUs, last intersection, last union]
        self.meters = torch.zeros(4, dtype=torch.float64, device=dev)
        self.lr = torch.full((1,), lr, dtype=torch.float32, device=dev)
        if optimizer not in ("SGD", "Adam"):
            raise L.NunetError("TrainStep: optimizer %r is not 'SGD' or 'Adam'" % (optimizer,))
        self.optimizer = optimizer
        self.momentum, self.wd, self.nesterov = momentum, weight_decay, nesterov
        self.betas, self.eps = (float(betas[0]), float(betas[1])), float(eps)
        if optimizer == "SGD":
            self.mom = torch.zeros_like(self.eng.flat_params)
            self.opt_state = [self.mom]
            self._optim = L.Optim(kind=L.OPT_SGD, momentum=momentum, beta1=0.0, beta2=0.0, eps=0.0, weight_decay=weight_decay,
                                  nesterov=1 if nesterov else 0, lr=L.ptr(self.lr).value, state0=L.ptr(self.mom).value)
        else:
            self.mom = None
            self.exp_avg = torch.zeros_like(self.eng.flat_params)
            self.exp_avg_sq = torch.zeros_like(self.eng.flat_params)
            self.adam_step = torch.zeros(1, dtype=torch.float32, device=dev)      # torch's step, as its capturable form keeps it
            self.adam_scal = torch.zeros(2, dtype=torch.float32, device=dev)      # {lr / (1 - b1^t), 1 / sqrt(1 - b2^t)} of this step
            self.opt_state = [self.exp_avg, self.exp_avg_sq, self.adam_step]
            self._optim = L.Optim(kind=L.OPT_ADAM, momentum=0.0, beta1=self.betas[0], beta2=self.betas[1], eps=self.eps,
                                  weight_decay=weight_decay, nesterov=0, lr=L.ptr(self.lr).value, adam_scal=L.ptr(self.adam_scal).value,
                                  state0=L.ptr(self.exp_avg).value, state1=L.ptr(self.exp_avg_sq).value)
        # dynamic loss scaling: the nunet_scaler words on the device (scale, inv_scale, growth tracker, found_inf, skipped steps)
        self.scaler_cfg = LS.scaler_settings(loss_scale)
        self._scaler = None
        if self.scaler_cfg is not None:
            self._scaler = torch.zeros(L.SCALER_WORDS, dtype=torch.int32, device=dev)
            self._write_scaler(self.scaler_cfg["init_scale"], 0, 0)
        # gradient-norm clipping: the nunet_clip words on the device (max_norm, coef, last norm, peak, fp64 sum, clipped, steps)
        self._clip = None
        if clip_grad_norm is not None:
            if not float(clip_grad_norm) > 0.0:
                raise L.NunetError("TrainStep: clip_grad_norm must be > 0 or None (got %r)" % (clip_grad_norm,))
            self._clip = torch.zeros(L.CLIP_WORDS, dtype=torch.int32, device=dev)
            self._clip[0:2] = torch.tensor([float(clip_grad_norm), 1.0], dtype=torch.float32).view(torch.int32).to(dev)
        # weight EMA: the averaged arenas and the nunet_ema words on the device (decay, warmup, n_averaged, this step's w and mode)
        self._ema = None
        self.ema_params = self.ema_bnbuf = None
        self.ema_decay, self.ema_warmup = None, bool(ema_warmup)
        if ema_decay is not None:
            from . import ema as EMA
            self.ema_decay = EMA.check_decay(ema_decay)
            self.ema_params = self.eng.flat_params.clone()
            self.ema_bnbuf = self.eng.bnbuf.clone()
            self._ema = torch.zeros(L.EMA_WORDS, dtype=torch.int32, device=dev)
            self._write_ema(0)
            self._optim.ema = L.ptr(self._ema).value
            self._optim.ema_params = L.ptr(self.ema_params).value
        if self._scaler is not None:
            self._optim.scaler = L.ptr(self._scaler).value
        if self._clip is not None:
            self._optim.clip = L.ptr(self._clip).value
        self.steps = 0
        self.pg = process_group
        self.world = dist.get_world_size(process_group) if (process_group is not None or dist.is_initialized()) else 1
        # NUNET_FORCE_DP=1: take the data-parallel code path (the gradient exchange of layout 1 or 3) with any world size, so that a
        # one-GPU box can rehearse it over RCCL with a single rank (bench.py initialises the process group)
        self.dp = self.world > 1 or (os.environ.get("NUNET_FORCE_DP") == "1" and dist.is_initialized())
        if self.dp:
            # RCCL's high-priority stream lives in this process: beside it lowest-priority lanes are served in time slices
            L.check(L.lib().nunet_plan_set_lane_priority(self.pl.handle, 0), "plan_set_lane_priority")
        # Data-parallel step layout (NUNET_DP_MODE), two of them. 1 (default): one lane-faithful graph for forward + loss + the
        # whole backward, ONE exchange of the complete gradient scratch, one graph for unpack + the optimiser step.
        # 3: the whole step is ONE graph that contains both exchanges as nodes: the backward pass is issued as phase 1 left open
        # (nunet_plan_backward_phase 1|8: no join), the first bucket's all-reduce goes to a side stream that waits for exactly
        # the kernels producing it, phase 2 continues on the open lanes beside it (2|16), the second bucket and the optimiser
        # step follow the join. Overlap without a fork / join barrier inside the pass and without any host call during the step
        # (RCCL only: a gloo exchange is a host round trip and cannot be captured).
        # NUNET_DP_MODE unset / "auto": with more than one rank, capture() times layouts 1 and 3 on the real exchange and
        # keeps the faster (the decision is all-reduced, so every rank takes the same one); one rank: layout 1.
        self.dp_mode, auto = dp_layout_from_env(os.environ)
        self.dp_auto = auto and self.dp
        if self.dp and self.dp_mode == 3 and dist.get_backend(process_group) == "gloo":
            self.dp_mode = 1             # a gloo exchange is a host round trip: it cannot sit inside the step's graph
        self.dp_choice = None        # {layout: ms per step} when the layout was chosen by measurement
        self.use_graph = use_graph
        # optimiser step layout: 0 = unpack, the flat step, (next forward's) pack as three streaming launches; 2 (default) = unpack
        # with the step as its epilogue (nunet_plan_opt_step: 46 us against 59 us for the pair). The flat OIHW gradients (p.grad
        # views) are materialised with keep_grads=True in the fused layout; in both layouts they hold the rank-MEAN gradient (as
        # DistributedDataParallel leaves p.grad).
        self.fused_update = fused_update_from(fused_update, os.environ)
        if self._clip is not None:       # one double per workgroup of the square-norm launch of this layout
            nb = (L.lib().nunet_plan_grad_sqnorm_ws_bytes(self.pl.handle) if self.fused_update
                  else L.lib().nunet_grad_sqnorm_ws_bytes(self.eng.flat_params.numel()))
            self._clip_ws = torch.zeros(nb // 8, dtype=torch.float64, device=dev)
        self.keep_grads = keep_grads
        self.g_fb = None
        self.g_opt = None
        self._buckets = self._grad_scratch() if self.dp else None
        if self.scaler_cfg is not None and not self.dp:
            self._grad_scratch()             # (self._scratch: what the overflow check reads)
        for p, off in zip(self.eng.module_params, self.eng.param_off):
            p.grad = self.eng.flat_grads[off:off + p.numel()].view(p.shape)
        if self.world > 1:
            self.broadcast_state()

    def broadcast_state(self, src=0):
        """Rank `src`'s parameters, optimiser state (momentum; Adam's moments and step), loss-scaler state, clip state (max_norm
        and statistics), weight EMA (decay, warmup, n_averaged, the averaged parameters and BatchNorm statistics) and BatchNorm
        buffers become every rank's (construction time; also after loading a checkpoint on one rank)."""
        eng = self.eng
        for t in [eng.flat_params] + self.opt_state + [eng.bnbuf] + self._aux_state() + self._ema_arenas():
            broadcast_flat_(t, src, self.pg)
        if self._ema is not None and self.world > 1:
            self.ema_decay, self.ema_warmup = self._read_ema()[:2]
        nbt = eng.nbt.to(torch.float64)          # (gloo / RCCL both take floating tensors; counts are exact in fp64)
        broadcast_flat_(nbt, src, self.pg)
        eng.nbt.copy_(nbt.to(torch.int64))

    def sync_bn_buffers(self, src=0):
        """BatchNorm running statistics policy under data parallel: rank `src`'s buffers are the model's. Call before
        validating or saving a checkpoint (batch statistics, and hence the buffers, are per replica during training)."""
        if self.world > 1:
            eng = self.eng
            broadcast_flat_(eng.bnbuf, src, self.pg)
            if self._ema is not None:        # (the averaged statistics follow the statistics they average: per replica, rank `src`'s win)
                broadcast_flat_(self.ema_bnbuf, src, self.pg)
            nbt = eng.nbt.to(torch.float64)
            broadcast_flat_(nbt, src, self.pg)
            eng.nbt.copy_(nbt.to(torch.int64))

    # -- pieces -------------------------------------------------------------------
    def _fwd_loss(self):
        lib, eng, pl = L.lib(), self.eng, self.pl
        st = L.stream()
        flags = 1
        if self.optimizer == "Adam" and self._scaler is None:     # (under loss scaling: behind the overflow check, _opt)
            # t += 1 and this step's bias corrections, ahead of the forward pass: the update launch of the step is ordered behind it
            L.check(lib.nunet_adam_prepare(L.ptr(self.lr), self.betas[0], self.betas[1], L.ptr(self.adam_step), L.ptr(self.adam_scal), st),
                    "adam_prepare")
        if self.input_u8:
            # the sample pipeline on the device: image -> the plan's padded NHWC tile, mask -> {0,1} fp32 NCHW target
            if self.resize:
                L.check(lib.nunet_plan_stage_u8_resize(pl.handle, L.ptr(self.img_pool), self.source_capacity, L.ptr(self.img_desc), L.ptr(self._mean),
                                                       L.ptr(self._std), L.ptr(self.aug), L.ptr(self.color), 1.0 / 255.0, L.ptr(pl.arena),
                                                       L.nbytes(pl.arena), st), "plan_stage_u8_resize")
                L.check(lib.nunet_preprocess_u8_resize(L.ptr(self.mask_pool), self.source_capacity, L.ptr(self.mask_desc), self.n, self.ncls, self.h,
                                                       self.w, None, None, L.ptr(self.aug), 1.0, L.ptr(self.t), st), "preprocess_u8_resize (masks)")
            elif self.color is not None:
                L.check(lib.nunet_plan_stage_u8_color(pl.handle, L.ptr(self.x_u8), L.ptr(self._mean), L.ptr(self._std), L.ptr(self.aug),
                                                      L.ptr(self.color), 1.0 / 255.0, L.ptr(pl.arena), L.nbytes(pl.arena), st), "plan_stage_u8_color")
            else:
                L.check(lib.nunet_plan_stage_u8(pl.handle, L.ptr(self.x_u8), L.ptr(self._mean), L.ptr(self._std), L.ptr(self.aug), 1.0 / 255.0,
                                                L.ptr(pl.arena), L.nbytes(pl.arena), st), "plan_stage_u8")
            if not self.resize:
                L.check(lib.nunet_preprocess_u8(L.ptr(self.t_u8), self.n, self.h, self.w, self.ncls, None, None, L.ptr(self.aug), 1.0,
                                                L.ptr(self.t), st), "preprocess_u8 (masks)")
            flags |= 4
        L.check(lib.nunet_plan_forward(pl.handle, L.ptr(eng.flat_params), L.ptr(eng.bnbuf), L.ptr(eng.nbt),
                                       L.ptr(self.x), L.ptr(pl.arena), L.nbytes(pl.arena), L.ptr(self.logits), flags, st), "plan_forward")
        if self._scaler is not None:    # dlogits seeded with the loss scale (the scaler's first word)
            L.check(lib.nunet_loss_step_scaled(L.ptr(self.logits), L.ptr(self.t), self.n, self.per, self.heads, self.loss_kind, L.ptr(self.loss_ws),
                                               L.nbytes(self.loss_ws), L.ptr(self.dlogits), L.ptr(self.loss_out), L.ptr(self.meters), self.iou_thr,
                                               L.ptr(self._scaler), st), "loss_step_scaled")
        else:
            L.check(lib.nunet_loss_step(L.ptr(self.logits), L.ptr(self.t), self.n, self.per, self.heads, self.loss_kind, L.ptr(self.loss_ws), L.nbytes(self.loss_ws),
                                        L.ptr(self.dlogits), L.ptr(self.loss_out), L.ptr(self.meters), self.iou_thr, st), "loss_step")
        pl.trained_forward = True

    def _bwd(self, phases):
        eng, pl = self.eng, self.pl
        L.check(L.lib().nunet_plan_backward_phase(pl.handle, L.ptr(eng.flat_params), L.ptr(self.dlogits), L.ptr(pl.arena), L.nbytes(pl.arena),
                                                  L.ptr(eng.flat_grads), 0, phases, L.stream()), "plan_backward_phase")

    def _fwd_bwd(self):
        self._fwd_loss()
        self._bwd(3 if self.fused_update else 7)

    def _aux_state(self):
        """The scaler, clip and EMA words, where present: snapshotted by capture() and broadcast with the replica state."""
        return [t for t in (self._scaler, self._clip, self._ema) if t is not None]

    def _ema_arenas(self):
        """The averaged parameters and BatchNorm statistics, where present (snapshotted and broadcast like the state words)."""
        return [] if self._ema is None else [self.ema_params, self.ema_bnbuf]

    def _clip_coef(self, plan, grad_scale):
        """This step's clip factor: the square norm of the plan's gradient scratch (plan=True) or of the flat gradients, one
        double per workgroup, then the one-workgroup launch that forms the norm, coef and the statistics."""
        lib, eng, pl, st = L.lib(), self.eng, self.pl, L.stream()
        ws = self._clip_ws
        if plan:
            L.check(lib.nunet_plan_grad_sqnorm(pl.handle, L.ptr(pl.arena), L.nbytes(pl.arena), L.ptr(ws), L.nbytes(ws), st), "plan_grad_sqnorm")
        else:
            L.check(lib.nunet_grad_sqnorm(L.ptr(eng.flat_grads), eng.flat_grads.numel(), L.ptr(ws), L.nbytes(ws), st), "grad_sqnorm")
        L.check(lib.nunet_clip_finalize(L.ptr(ws), ws.numel(), grad_scale, L.ptr(self._scaler), L.ptr(self._clip), st), "clip_finalize")

    def _opt(self):
        """The optimiser step, behind the complete (exchanged) gradient scratch. Under loss scaling and / or gradient clipping in
        torch's order: overflow check, Adam's bookkeeping unless skipped, the norm of the unscaled gradient and the clip factor,
        the update (unscaled by inv_scale, clipped by coef; nothing written on a skipped step), the scale update. With a weight
        EMA: its one-thread bookkeeping (this step's w and mode, n_averaged) ahead of the norm, the averaged parameters inside
        the update launch, the averaged BatchNorm statistics behind it."""
        lib, eng, pl, st = L.lib(), self.eng, self.pl, L.stream()
        sc = L.ptr(self._scaler)
        if sc is not None:
            L.check(lib.nunet_scaler_check(L.ptr(self._scratch), self._scratch.numel(), sc, st), "scaler_check")
            if self.optimizer == "Adam":
                L.check(lib.nunet_adam_prepare_scaled(L.ptr(self.lr), self.betas[0], self.betas[1], L.ptr(self.adam_step), L.ptr(self.adam_scal),
                                                      sc, st), "adam_prepare_scaled")
        if self._ema is not None:
            L.check(lib.nunet_ema_prepare(L.ptr(self._ema), sc, st), "ema_prepare")
        if self.fused_update:              # layout 2: gradient scratch -> step in one launch
            if self._clip is not None:
                self._clip_coef(True, 1.0 / self.world)
            L.check(lib.nunet_plan_opt_step(pl.handle, L.ptr(eng.flat_params), C.byref(self._optim), L.ptr(pl.arena), L.nbytes(pl.arena),
                                            1.0 / self.world, L.ptr(eng.flat_grads) if self.keep_grads else None, st), "plan_opt_step")
        else:                              # layout 0: the flat gradients that backward phase 4 unpacked
            if self.world > 1:
                eng.flat_grads.mul_(1.0 / self.world)      # p.grad = rank mean in every layout
            if self._clip is not None:
                self._clip_coef(False, 1.0)
            L.check(lib.nunet_opt_step(L.ptr(eng.flat_params), L.ptr(eng.flat_grads), C.byref(self._optim), eng.flat_params.numel(), 1.0, st),
                    "opt_step")
        if self._ema is not None:
            L.check(lib.nunet_ema_lerp(L.ptr(self.ema_bnbuf), L.ptr(eng.bnbuf), eng.bnbuf.numel(), L.ptr(self._ema), st), "ema_lerp")
        if sc is not None:
            cfg = self.scaler_cfg
            L.check(lib.nunet_scaler_update(sc, cfg["growth_factor"], cfg["backoff_factor"], cfg["growth_interval"], st), "scaler_update")

    def _grad_scratch(self):
        """The plan's native-layout gradient scratch as two fp32 views in gradient-ready order."""
        off, b0, tot = C.c_int64(), C.c_int64(), C.c_int64()
        L.check(L.lib().nunet_plan_grad_scratch(self.pl.handle, C.byref(off), C.byref(b0), C.byref(tot)), "plan_grad_scratch")
        flat = self.pl.arena[off.value:off.value + 4 * tot.value].view(torch.float32)
        self._scratch = flat
        return flat[:b0.value], flat[b0.value:]

    def _exchange(self, t):
        """Sum a gradient bucket over ranks; asynchronous under RCCL so that it overlaps what follows."""
        if dist.get_backend(self.pg) == "gloo":
            allreduce_flat_(t, self.pg)
            return None
        return dist.all_reduce(t, op=dist.ReduceOp.SUM, group=self.pg, async_op=True)

    def _exchange_after_pass_step(self, run_pass, run_opt):
        """Layout 1: forward + loss + the whole backward pass, ONE all-reduce of the complete gradient scratch, then unpack + the
        optimiser step (grad_scale 1/world) on the reduced scratch."""
        run_pass()
        h = self._exchange(self._scratch)
        if h is not None:
            h.wait()
        run_opt()

    def _in_graph_exchange_step(self):
        """Layout 3: forward, loss, the backward pass with both gradient exchanges and the optimiser step as one stream of
        work - captured, one graph. Bucket 0 (heads + the last anti-diagonal, 75 % of the bytes) is all-reduced on a side stream
        ordered behind its producing kernels only, while phase 2 continues on the pass's open lanes."""
        lib, pl = L.lib(), self.pl
        b0, b1 = self._buckets
        self._fwd_loss()
        self._bwd(1 | 8)                                   # phase 1, pass left open: the current stream has waited for nothing
        cur = torch.cuda.current_stream()
        side = torch.cuda.Stream()                         # (a stream this capture has not used: it joins the capture by its waits)
        side.wait_stream(cur)                              # single-lane issue keeps everything on `cur`; with lanes this is the fork point only
        L.check(lib.nunet_plan_bucket0_wait(pl.handle, side.cuda_stream), "plan_bucket0_wait")
        with torch.cuda.stream(side):
            h0 = dist.all_reduce(b0, op=dist.ReduceOp.SUM, group=self.pg, async_op=True)
        self._bwd(2 | 16)                                  # phase 2 on the open lanes, beside the exchange; joins `cur`
        # the second bucket is ISSUED before `cur` waits for the first: the collective stream then never waits on an event that
        # descends from its own tail (the stream-capture pattern ROCm 7.2 crashes on, tests/test_capture_gpu.py); the collective
        # stream is in order, so waiting for the second exchange covers the first
        h1 = dist.all_reduce(b1, op=dist.ReduceOp.SUM, group=self.pg, async_op=True)
        h1.wait()
        self._side, self._h0 = side, h0                    # (kept alive until the next step)
        if not self.fused_update:
            self._bwd(4)
        self._opt()

    def _eager_step(self):
        if self.dp and self.dp_mode == 3:
            return self._in_graph_exchange_step()
        if self.dp:
            self._exchange_after_pass_step(lambda: (self._fwd_loss(), self._bwd(3)),
                                           lambda: (None if self.fused_update else self._bwd(4), self._opt()))
        else:
            self._fwd_bwd()
            self._opt()

    def capture(self, inp, target):
        """Capture forward+loss+backward(+SGD) into hipGraphs. Needs one REAL batch for the
        eager warm-up (an all-zero batch gives degenerate BatchNorm variances). Parameters,
        BN running statistics, momentum, meters and the weight EMA (averaged arenas, n_averaged) are
        snapshotted before and restored after, so warm-up and capture leave no trace in the training trajectory."""
        if not self.use_graph:
            return
        eng = self.eng
        if self.resize:            # ((image pool, descriptors), (mask pool, descriptors)): dataset.pack_ragged's pairs
            self._load_ragged(inp[0], inp[1], target[0], target[1])
            self.aug.zero_()
            if self.color is not None:
                self.color.zero_()
        elif self.input_u8:        # (uint8 images, uint8 masks)
            self.x_u8.copy_(inp)
            self.t_u8.copy_(target)
            self.aug.zero_()
            if self.color is not None:
                self.color.zero_()
        else:
            self.x.copy_(inp)
            self.t.copy_(target)
        state = [eng.flat_params, eng.bnbuf, eng.nbt, self.meters] + self.opt_state + self._aux_state() + self._ema_arenas()
        snap = [t.clone() for t in state]
        steps0 = self.steps
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(2):
                self._eager_step()
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        if self.dp and self.dp_mode == 3 and dist.get_backend(self.pg) == "gloo":
            self.dp_mode = 1                                # a host-side exchange cannot be a graph node
        if not self.dp:
            # the whole step, recorded once on a side stream and replayed on the caller's: as ONE hipGraph, or - segmented='flags' -
            # as one single-stream graph per lane with the cross-lane dependencies as device-side flags (csrc/graph.hip nunet_seg_*:
            # explicit node -> queue placement on lanes chosen by measurement)
            body = lambda: (self._fwd_bwd(), self._opt())
            if self.executor_auto:
                self._choose_executor(s, body)
            else:
                self.g_fb = self._build_executor(s, body, self.segmented, self.schedule)
        else:
            if self.dp_auto:
                self._choose_layout(s)
            if self.dp_mode == 1:
                self._capture_one_pass(s)
            else:
                self._capture_in_graph_exchange(s)
        torch.cuda.synchronize()
        with torch.no_grad():
            for dst, src in zip(state, snap):
                dst.copy_(src)
        self.steps = steps0

    def _set_schedule(self, schedule):
        self.schedule = schedule
        L.check(L.lib().nunet_plan_set_schedule(self.pl.handle, {"lanes": 0, "list": 2}[schedule]), "plan_set_schedule")

    def _build_executor(self, s, body, segmented, schedule):
        """The step body recorded in one of its executable forms (see __init__)."""
        self._set_schedule(schedule)
        self.segmented = segmented
        if schedule == "list" and not self._calibrated:
            # the list scheduler's per-op costs, measured: the step on ONE lane with a device timestamp behind every op
            L.check(L.lib().nunet_plan_calibrate(self.pl.handle, 1), "plan_calibrate")
            try:
                g = _NativeGraph(s, body)
                with torch.cuda.stream(s):
                    for _ in range(3):
                        g.replay()
                torch.cuda.synchronize()
                self._single_lane_ms = self._time(self._as_step_runs(g), 2, 5)     # (with the stamp kernels: an upper bound of the one-lane step)
            finally:
                L.check(L.lib().nunet_plan_calibrate(self.pl.handle, 0), "plan_calibrate")
            # (kept alive while the program below picks its lanes: with the calibration graph - and its launch stream - destroyed
            #  first, 4 of 20 processes came up with a flag program at 4.8 ms per step instead of 1.7; with it alive 0 of 12, like
            #  the capture-time choice, whose first candidate - a native graph - is alive at that point: 0 of 26. Which stream
            #  inherits the freed hardware-queue slot decides; ROCm offers no way to ask.)
            self._calib_graph = g
            self._calibrated = True
        if segmented == "flags" and getattr(self, "_single_lane_ms", None):
            # A flag program is checked against the one-lane step before it is used: which hardware queue a lane inherits is
            # ROCm's choice, and unchecked 1 process in 5 came up at 4.8 ms per step instead of 1.7 (every lane's kernels
            # serialised). Such a program is thrown away and recorded again on newly picked lanes.
            prog = None
            for attempt in range(3):
                prog = _SegProgram(s, body)
                ms = self._time(self._as_step_runs(prog), 2, 8)
                if ms < 0.9 * self._single_lane_ms:
                    break
                print("[nunet] flag-synchronised program came up at %.2f ms per step (one lane: %.2f): picking new lanes (%d)"
                      % (ms, self._single_lane_ms, attempt + 1))
                if attempt < 2:
                    prog = None
                    L.check(L.lib().nunet_plan_reset_lanes(self.pl.handle), "plan_reset_lanes")
        else:
            prog = _SegProgram(s, body) if segmented else _NativeGraph(s, body)
        self._calib_graph = None
        return prog

    @staticmethod
    def _time(run, warm, reps):
        """ms per call of run(): `warm` untimed calls, then `reps` between two events on the caller's stream."""
        for _ in range(warm):
            run()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            run()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    def _as_step_runs(self, g):
        """A recorded program issued the way step() issues it: batch copy + replay from the caller's stream."""
        buf = self.img_pool if self.resize else self.x_u8 if self.input_u8 else self.x
        fresh = buf.clone()
        def one():
            buf.copy_(fresh, non_blocking=True)
            g.replay()
        return one

    def _choose_executor(self, s, body, reps=20):
        """Time the two executable forms of the captured step on this device and keep the faster: the multi-branch hipGraph
        with block lanes, and the flag-synchronised single-stream graphs with list-scheduled lanes. (The caller restores the
        training state.) A form that cannot be recorded or replayed here - e.g. no two streams on distinct hardware queues -
        drops out with a message."""
        forms = [(False, "lanes"), ("flags", "list")]
        progs, times = {}, {}
        for form in forms:
            try:
                g = self._build_executor(s, body, *form)
                # timed the way step() will run it: from the caller's stream, behind the copies of a fresh batch (a stream that
                # shares a hardware queue with one of the lanes shows here, not after the choice)
                torch.cuda.current_stream().wait_stream(s)
                one = self._as_step_runs(g)
                ms = self._time(one, 3, reps)
                one()                            # (a cross-lane wait that timed out fails the NEXT launch)
                torch.cuda.synchronize()
                progs[form], times[form] = g, ms
            except Exception as e:
                if form == forms[0]:
                    raise
                print("[nunet] executor %s/%s is not available here: %s" % (form[0], form[1], e))
        best = min(times, key=times.get)
        self.executor_choice = times
        self.g_fb = progs.pop(best)
        progs.clear()
        self._set_schedule(best[1])
        self.segmented = best[0]

    def _capture_one_pass(self, s):
        """Layout 1: forward + loss + the whole backward as one graph, the exchange between, unpack + the optimiser step as a
        second graph. The pass may run as flag-synchronised list-scheduled lanes (self.dp_exec, chosen by _choose_layout)."""
        body = lambda: (self._fwd_loss(), self._bwd(3))
        self.g_fb = self._build_executor(s, body, *self.dp_exec)
        self.g_opt = _NativeGraph(s, lambda: (None if self.fused_update else self._bwd(4), self._opt()))

    def _capture_in_graph_exchange(self, s):
        """Layout 3: the whole data-parallel step, exchanges included, as one graph."""
        self.g_fb = _NativeGraph(s, self._in_graph_exchange_step)
        self.g_opt = None

    def _choose_layout(self, s, reps=8):
        """Time layout 1 (one exchange after the pass) against layout 3 (both exchanges inside the step's graph, bucket 0
        beside phase 2 of the backward pass) on the real process group and keep the faster. The caller restores the
        training state."""
        times = []
        modes = [(1, (False, "lanes"))]
        if dist.get_backend(self.pg) != "gloo":
            # (the flag-synchronised lanes only where every rank has a device of its own: ranks sharing one GPU - the rehearsal
            #  tests - also share its hardware queues, and a polling kernel may then sit in front of the signal it waits for)
            # (one-rank rehearsal with RCCL initialised: flag lanes 1.82 ms, graph 1.96-1.98 ms per step - with the side lanes at
            #  DEFAULT stream priority; at the lowest priority, beside RCCL's high-priority stream, 3.4-4.4 ms. NUNET_DP_FLAGS=0
            #  takes the candidate out.)
            if self.world <= torch.cuda.device_count() and os.environ.get("NUNET_DP_FLAGS", "1") == "1":
                modes.append((1, ("flags", "list")))
            modes.append((3, (False, "lanes")))
        def all_agree(ok):
            """A candidate is timed only if EVERY rank recorded it: the timing loop holds collectives, and a rank that skipped it
            would leave the others waiting in them."""
            f = torch.tensor([1.0 if ok else 0.0], dtype=torch.float64, device=self.eng.device)
            if dist.get_backend(self.pg) == "gloo":
                h = f.cpu(); dist.all_reduce(h, op=dist.ReduceOp.MIN, group=self.pg); f = h
            else:
                dist.all_reduce(f, op=dist.ReduceOp.MIN, group=self.pg)
            return bool(f.item() > 0.5)

        for mode, ex in modes:
            self.dp_mode = mode
            self.dp_exec = ex
            err = None
            try:
                if mode == 3:
                    self._capture_in_graph_exchange(s)
                    run = self.g_fb.replay
                else:
                    self._capture_one_pass(s)
                    run = lambda: self._exchange_after_pass_step(self.g_fb.replay, self.g_opt.replay)
            except Exception as e:       # e.g. a runtime that cannot capture the collectives, no two streams on distinct queues
                err = e
            if not all_agree(err is None):
                if (mode, ex) == modes[0]:
                    raise err if err is not None else L.NunetError("data-parallel layout 1 could not be captured on another rank")
                print("[nunet] data-parallel candidate (layout %d, %s/%s) could not be captured on every rank%s"
                      % (mode, ex[0], ex[1], ": %s" % err if err is not None else ""))
                times.append(float("inf"))
                continue
            times.append(self._time(run, 2, reps))
        t = torch.tensor(times, dtype=torch.float64, device=self.eng.device)
        t = torch.nan_to_num(t, posinf=1e30)
        if dist.get_backend(self.pg) == "gloo":
            h = t.cpu(); dist.all_reduce(h, op=dist.ReduceOp.MAX, group=self.pg); t = h
        else:
            dist.all_reduce(t, op=dist.ReduceOp.MAX, group=self.pg)     # the slowest rank decides, identically everywhere
        t = t.tolist()
        label = lambda m, ex: {1: "exchange_after_pass", 3: "exchange_inside_graph"}[m] + ("" if ex[0] is False else "/flags+list")
        self.dp_choice = {label(m, ex): v for (m, ex), v in zip(modes, t)}
        best = min(range(len(t)), key=lambda q: t[q])
        self.dp_mode, self.dp_exec = modes[best]
        self.g_fb = self.g_opt = None

    def step(self, inp=None, target=None):
        """One training iteration. `inp`/`target` are device tensors (copied into the
        static graph inputs); None re-uses what is already staged."""
        if inp is not None:
            if self.input_u8:
                raise L.NunetError("this TrainStep was built with input_u8=True: feed it with step_u8(images_u8, masks_u8, aug)")
            self.x.copy_(inp, non_blocking=True)
            self.t.copy_(target, non_blocking=True)
        self._run()

    def step_u8(self, images_u8, masks_u8, aug=None, color=None):
        """One training iteration from the decoded uint8 batch (device tensors; images [N,H,W,C], masks [N,H,W,K] with
        values {0,255}), optional augmentation codes (dataset.draw_augmentation) and, on a step built with color_aug=True,
        optional colour codes (dataset.draw_color_augmentation; None: no colour op); needs input_u8=True."""
        if not self.input_u8:
            raise L.NunetError("step_u8 needs a TrainStep built with input_u8=True")
        if self.resize:
            raise L.NunetError("this TrainStep was built with resize=True: feed it with step_u8_ragged(img_pool, img_desc, mask_pool, mask_desc, aug, color)")
        self._check_codes(aug, color, self.h, self.w)
        self.x_u8.copy_(images_u8, non_blocking=True)
        self.t_u8.copy_(masks_u8, non_blocking=True)
        self._set_codes(aug, color)
        self._run()

    def _check_codes(self, aug, color, h, w):
        """Refuse malformed augmentation / colour codes before the static buffers change (h, w: the shape an odd rot90 count must
        find square; the resizing step passes a square one, its sources need not be)."""
        if color is not None:
            if self.color is None:
                raise L.NunetError("step_u8: color codes need a TrainStep built with color_aug=True")
            if color.dtype != torch.int32 or tuple(color.shape) != tuple(self.color.shape):
                raise L.NunetError("step_u8: color must be int32 %s (dataset.draw_color_augmentation), got %s %s"
                                   % (tuple(self.color.shape), color.dtype, tuple(color.shape)))
        if aug is not None:
            _check_aug(aug, self.n, h, w)

    def _set_codes(self, aug, color):
        if aug is None:
            self.aug.zero_()
        else:
            self.aug.copy_(aug, non_blocking=True)
        if self.color is not None:
            if color is None:
                self.color.zero_()
            else:
                self.color.copy_(color, non_blocking=True)

    def _load_ragged(self, img_pool, img_desc, mask_pool, mask_desc):
        """Validate a ragged batch on the host (descriptors against their pool, pools against the capacity) and copy it into the
        static buffers the captured launches read. Nothing is written when anything is refused."""
        from .dataset import check_descriptors
        for what, pool, desc, ch in (("image", img_pool, img_desc, self._cin), ("mask", mask_pool, mask_desc, self.ncls)):
            if not isinstance(pool, torch.Tensor) or pool.dtype != torch.uint8 or pool.dim() != 1:
                raise L.NunetError("step_u8_ragged: the %s pool must be a flat uint8 tensor (dataset.pack_ragged)" % what)
            if pool.numel() > self.source_capacity:
                raise L.NunetError("step_u8_ragged: the %s pool holds %d bytes, this TrainStep was built with source_capacity=%d"
                                   % (what, pool.numel(), self.source_capacity))
            check_descriptors(desc, pool.numel(), ch, self.n)
        self.img_pool[:img_pool.numel()].copy_(img_pool, non_blocking=True)
        self.mask_pool[:mask_pool.numel()].copy_(mask_pool, non_blocking=True)
        self.img_desc.copy_(torch.as_tensor(img_desc), non_blocking=True)
        self.mask_desc.copy_(torch.as_tensor(mask_desc), non_blocking=True)

    def step_u8_ragged(self, img_pool, img_desc, mask_pool, mask_desc, aug=None, color=None):
        """One training iteration from ragged decoded samples: the byte pools (flat uint8, host or device) and HOST descriptors
        (int32 [N,4]) of the images and of the masks, as dataset.pack_ragged / FolderDataset.batch return them, optional
        augmentation codes (an odd rot90 count needs no square source) and colour codes; needs resize=True. Descriptors are
        checked against their pool and the pools against source_capacity before anything is copied or launched."""
        if not self.resize:
            raise L.NunetError("step_u8_ragged needs a TrainStep built with input_u8=True, resize=True")
        self._check_codes(aug, color, 1, 1)
        self._load_ragged(img_pool, img_desc, mask_pool, mask_desc)
        self._set_codes(aug, color)
        self._run()

    def _run(self):
        if self.model._engine is not self.eng or not self.eng.intact():
            raise L.NunetError("the module's parameter arenas were re-homed (moved to another device / parameters replaced) "
                               "after this TrainStep was built: its graphs would update orphaned memory. Build a new TrainStep.")
        if self.g_fb is not None:
            if self.dp and self.dp_mode != 3:
                self._exchange_after_pass_step(self.g_fb.replay, self.g_opt.replay)
            else:
                self.g_fb.replay()
        else:
            self._eager_step()
        self.steps += 1

    def set_lr(self, lr):
        self.lr.fill_(lr)

    def _hyper(self):
        lr = float(self.lr.item())
        if self.optimizer == "Adam":
            return dict(lr=lr, betas=self.betas, eps=self.eps, weight_decay=self.wd, amsgrad=False)
        return dict(lr=lr, momentum=self.momentum, dampening=0, weight_decay=self.wd, nesterov=self.nesterov)

    def _trainable(self):
        """(offset into the flat arena, shape) of the module's trainable parameters, in filter(requires_grad, model.parameters())
        order"""
        return [(off, p.shape) for p, off in zip(self.eng.module_params, self.eng.param_off) if p.requires_grad]

    def optimizer_state_dict(self):
        """The optimiser state in the format of torch.optim.Adam / torch.optim.SGD.state_dict(), keyed by the index of a parameter
        in filter(requires_grad, model.parameters()): a stock optimiser over those parameters loads it (one host sync)."""
        torch.cuda.current_stream().synchronize()
        if self.optimizer == "Adam":
            flat = {"exp_avg": self.exp_avg, "exp_avg_sq": self.exp_avg_sq}
            step = float(self.adam_step.item())
        else:
            flat = {"momentum_buffer": self.mom}
            step = None
        return flat_to_torch_state(self._trainable(), flat, step, self._hyper())

    def load_optimizer_state_dict(self, sd):
        """Inverse of optimizer_state_dict(): the state (and lr) of a torch.optim.Adam / SGD state dict of the same kind, over the
        same parameters, becomes this step's. The next step continues it (graphs read the same buffers)."""
        names = ("exp_avg", "exp_avg_sq") if self.optimizer == "Adam" else ("momentum_buffer",)
        flat = {"exp_avg": self.exp_avg, "exp_avg_sq": self.exp_avg_sq} if self.optimizer == "Adam" else {"momentum_buffer": self.mom}
        step, lr = torch_state_to_flat(sd, self._trainable(), {k: flat[k] for k in names})
        if self.optimizer == "Adam":
            self.adam_step.fill_(0.0 if step is None else step)
        if lr is not None:
            self.set_lr(lr)

    def reset_meters(self):
        self.meters.zero_()
        if self._scaler is not None:
            self._scaler[4:5].zero_()        # skipped steps
        if self._clip is not None:
            self._clip[2:].zero_()           # last norm, peak, sum, clipped, steps (max_norm and coef stay)
        self.steps = 0

    # -- gradient clipping -----------------------------------------------------------
    def set_clip_grad_norm(self, value):
        """A new max_norm (float('inf'): measure only) for the steps that follow; a captured step reads it from the device."""
        if self._clip is None:
            raise L.NunetError("this TrainStep was built without gradient clipping (clip_grad_norm=None)")
        if not float(value) > 0.0:
            raise L.NunetError("set_clip_grad_norm: max_norm must be > 0 (got %r)" % (value,))
        self._clip[0:1].view(torch.float32).fill_(float(value))

    def grad_norm_stats(self):
        """dict(last, mean, peak, clipped, steps) of the total gradient norm over the applied steps since reset_meters() (steps
        skipped by loss scaling do not count); one host sync. None without gradient clipping."""
        if self._clip is None:
            return None
        torch.cuda.current_stream().synchronize()
        w = self._clip.cpu()
        f = w.view(torch.float32)
        steps = int(w[7])
        return dict(last=float(f[2]), mean=float(w[4:6].view(torch.float64).item()) / max(steps, 1), peak=float(f[3]),
                    clipped=int(w[6]), steps=steps)

    # -- weight EMA ------------------------------------------------------------------
    def _need_ema(self, what):
        if self._ema is None:
            raise L.NunetError("%s: this TrainStep was built without a weight EMA (ema_decay=None)" % what)

    def _write_ema(self, n_averaged):
        """Set the device EMA words: this step's decay and warmup, n_averaged as given, w and the mode cleared."""
        L.check(L.lib().nunet_ema_init(L.ptr(self._ema), self.ema_decay, 1 if self.ema_warmup else 0, int(n_averaged), L.stream()), "ema_init")

    def _read_ema(self):
        """(decay, warmup, n_averaged, w, mode) of the device words; one host sync."""
        torch.cuda.current_stream().synchronize()
        w = self._ema.cpu()
        return (float(w[0:2].view(torch.float64).item()), bool(w[2]), int(w[3]), float(w[4:5].view(torch.float32).item()), int(w[5]))

    def ema_stats(self):
        """dict(n_averaged, w): the applied updates so far and the lerp weight of the last one (1.0 after the first, which
        copies; 0.0 before any); one host sync. None without a weight EMA."""
        if self._ema is None:
            return None
        _, _, n, w, _ = self._read_ema()
        return dict(n_averaged=n, w=w)

    def ema_state_dict(self):
        """The averaged model as a state dict: model.state_dict()'s keys, shapes and dtypes, the parameters from ema_params,
        the BatchNorm running statistics from ema_bnbuf, num_batches_tracked from the live model (it is not averaged: see
        __init__). The tensors are copies. One host sync."""
        from . import ema as EMA
        self._need_ema("ema_state_dict")
        torch.cuda.current_stream().synchronize()
        return EMA.state_dict_from_flat(self.model, self.eng, self.ema_params, self.ema_bnbuf)

    def load_ema_state_dict(self, sd, n_averaged=None):
        """Inverse of ema_state_dict(): the parameters and running statistics of `sd` become the average (num_batches_tracked
        is ignored). n_averaged: the count to continue from (0: the next applied step copies); None keeps this step's. Under
        data parallel, call it on every rank (or on one, then broadcast_state())."""
        from . import ema as EMA
        self._need_ema("load_ema_state_dict")
        EMA.flat_from_state_dict(self.model, self.eng, sd, self.ema_params, self.ema_bnbuf)
        if n_averaged is not None:
            if int(n_averaged) < 0:
                raise L.NunetError("load_ema_state_dict: n_averaged must be >= 0 (got %r)" % (n_averaged,))
            self._write_ema(int(n_averaged))

    # -- loss scaling ----------------------------------------------------------------
    def _write_scaler(self, scale, tracker, skipped=None):
        """Set the device scaler words (scale, its inverse as torch forms it, growth tracker; found_inf cleared)."""
        w = self._scaler.cpu()
        w[0:2] = torch.tensor([scale, LS.inv_scale(scale)], dtype=torch.float32).view(torch.int32)
        w[2] = int(tracker)
        w[3] = 0
        if skipped is not None:
            w[4] = int(skipped)
        self._scaler.copy_(w)

    def _read_scaler(self):
        torch.cuda.current_stream().synchronize()
        w = self._scaler.cpu()
        return w[0:1].view(torch.float32).item(), int(w[2]), int(w[4])

    def scaler_stats(self):
        """(current loss scale, steps skipped for overflow since reset_meters()); one host sync. None without loss scaling."""
        if self._scaler is None:
            return None
        scale, _, skipped = self._read_scaler()
        return scale, skipped

    def scaler_state_dict(self):
        """The loss scaler's state in torch.amp.GradScaler.state_dict()'s format (one host sync); {} without loss scaling, as a
        disabled GradScaler returns."""
        if self._scaler is None:
            return {}
        scale, tracker, _ = self._read_scaler()
        return LS.to_state_dict(scale, tracker, self.scaler_cfg)

    def load_scaler_state_dict(self, sd):
        """Inverse of scaler_state_dict() (also takes a torch.amp.GradScaler's): scale and growth tracker become this step's; the
        factors and interval too, as GradScaler.load_state_dict() does - once a step is captured they are part of its graph and
        must equal this TrainStep's. Under data parallel, call it on every rank (or on one, then broadcast_state())."""
        if self._scaler is None:
            raise L.NunetError("this TrainStep was built without loss scaling (loss_scale=None)")
        scale, tracker, cfg = LS.from_state_dict(sd)
        keys = ("growth_factor", "backoff_factor", "growth_interval")
        if self.g_fb is not None and any(cfg[k] != self.scaler_cfg[k] for k in keys):
            raise L.NunetError("load_scaler_state_dict: growth_factor / backoff_factor / growth_interval %s differ from the captured step's %s"
                               % ([cfg[k] for k in keys], [self.scaler_cfg[k] for k in keys]))
        self.scaler_cfg.update({k: cfg[k] for k in keys})
        self._write_scaler(scale, tracker)

    def epoch_stats(self):
        """(mean loss, mean IoU) over the steps since reset_meters(); one host sync.
        Equal-sized batches make this the sample-weighted AverageMeter of utils.py:29-33."""
        k = max(self.steps, 1)
        m = self.meters.tolist()
        return m[0] / k, m[1] / k


LOSS_KINDS = {"BCEDiceLoss": L.LOSS_BCE_DICE, "LovaszHingeLoss": L.LOSS_LOVASZ_HINGE, "BCEWithLogitsLoss": L.LOSS_BCE_LOGITS}


TTA_SETS = {"flips": (0, 4, 8, 12), "d4": (0, 1, 2, 3, 4, 5, 6, 7)}      # geometric codes as the input pipeline's aug
TTA_MERGES = {"logit": L.TTA_LOGIT, "prob": L.TTA_PROB}


def tta_codes(tta, h, w):
    """EvalStep's tta argument -> None (off) or the tuple of geometric codes, one per view, in merge order. Host only."""
    if tta is None:
        return None
    if isinstance(tta, str):
        if tta not in TTA_SETS:
            raise L.NunetError("EvalStep: tta %r is not one of %s, None or a tuple of codes 0 .. 15" % (tta, sorted(TTA_SETS)))
        codes = TTA_SETS[tta]
    elif isinstance(tta, (tuple, list)):
        codes = tuple(tta)
    else:
        raise L.NunetError("EvalStep: tta %r is not one of %s, None or a tuple of codes 0 .. 15" % (tta, sorted(TTA_SETS)))
    if not codes:
        raise L.NunetError("EvalStep: tta is an empty tuple: at least one view (None switches test-time augmentation off)")
    for c in codes:
        if isinstance(c, bool) or not isinstance(c, int) or not 0 <= c <= 15:
            raise L.NunetError("EvalStep: tta code %r is outside 0 .. 15 (rot90 count | hflip << 2 | vflip << 3)" % (c,))
        if c & 1 and h != w:
            raise L.NunetError("EvalStep: tta code %d has an odd rot90 count, which needs H == W (got %d x %d)" % (c, h, w))
    return codes


class _EvalBatch:
    """The buffers of one validation batch size: a Plan of its own (not Engine.plans: the training step's recorded program and
    lane state live on the cached plan of the same key), static input / target / logits, the loss workspace and outputs; under
    test-time augmentation also the view of the input and the logits of one view."""

    def __init__(self, ev, n):
        from .engine import Plan
        model, eng, dev = ev.model, ev.eng, ev.eng.device
        self.n = n
        self.pl = Plan(n, ev.h, ev.w, ev.cin, ev.ncls, getattr(model, "deep_supervision", False), model.compute_dtype, model._unet, dev,
                       depth=ev.depth)
        if self.pl.nparams != eng.flat_params.numel() or self.pl.nbnbuf != eng.bnbuf.numel() or self.pl.nbn != len(eng.bns):
            raise L.NunetError("EvalStep: plan/module parameter layout mismatch: %d vs %d params" % (self.pl.nparams, eng.flat_params.numel()))
        self.heads = self.pl.heads
        self.x = torch.zeros((n, ev.cin, ev.h, ev.w), dtype=torch.float32, device=dev)
        self.t = torch.zeros((n, ev.ncls, ev.h, ev.w), dtype=torch.float32, device=dev)
        self.logits = torch.zeros((self.heads, n, ev.ncls, ev.h, ev.w), dtype=torch.float32, device=dev)
        ws_query = L.lib().nunet_eval_step_heads_ws_bytes if ev.per_head else L.lib().nunet_eval_step_ws_bytes
        nb = ws_query(n, ev.ncls, ev.h * ev.w, self.heads, ev.loss_kind)
        self.ws = torch.empty((nb + 7) // 8, dtype=torch.float64, device=dev)        # (the caching allocator hands out 512-byte aligned blocks)
        self.loss_out = torch.zeros(self.heads + 1, dtype=torch.float32, device=dev)    # per head, then their mean
        if ev.tta is not None:      # (an odd rot90 count has H == W: the view's extents are the source's, one plan serves every view)
            self.x_view = torch.zeros_like(self.x)
            self.view_logits = torch.zeros_like(self.logits)
        self.graph = None

    def repack(self, ev):
        L.check(L.lib().nunet_plan_repack(self.pl.handle, L.ptr(ev.flat_params), L.ptr(self.pl.arena), L.nbytes(self.pl.arena), L.stream()), "plan_repack")

    def issue(self, ev):
        """forward in eval mode on the packed weights of this plan's arena (training = 2), then the validation step. Under
        test-time augmentation, per view in order: the view of the input (code 0: the input itself), its forward, and the merge
        of all heads' logits ([heads][n][K][hw] is contiguous: heads * n samples) into self.logits in the source frame."""
        lib, eng, pl, st = L.lib(), ev.eng, self.pl, L.stream()

        def forward(x, logits):
            L.check(lib.nunet_plan_forward(pl.handle, L.ptr(ev.flat_params), L.ptr(ev.bnbuf), L.ptr(eng.nbt), L.ptr(x), L.ptr(pl.arena),
                                           L.nbytes(pl.arena), L.ptr(logits), 2, st), "plan_forward")

        if ev.tta is None:
            forward(self.x, self.logits)
        for i, code in enumerate(ev.tta or ()):
            x = self.x
            if code:
                L.check(lib.nunet_dihedral_nchw(L.ptr(self.x), self.n, ev.cin, ev.h, ev.w, code, L.ptr(self.x_view), st), "dihedral_nchw")
                x = self.x_view
            forward(x, self.view_logits)
            L.check(lib.nunet_tta_merge(L.ptr(self.view_logits), self.heads * self.n, ev.ncls, ev.h, ev.w, code, ev.tta_mode, i, len(ev.tta),
                                        L.ptr(self.logits), st), "tta_merge")
        if ev.per_head:
            L.check(lib.nunet_eval_step_heads(L.ptr(self.logits), L.ptr(self.t), self.n, ev.ncls, ev.h * ev.w, self.heads, ev.loss_kind,
                                              L.ptr(self.ws), L.nbytes(self.ws), L.ptr(self.loss_out), L.ptr(ev.meters), L.ptr(ev.head_meters),
                                              ev.iou_thr, st), "eval_step_heads")
        else:
            L.check(lib.nunet_eval_step(L.ptr(self.logits), L.ptr(self.t), self.n, ev.ncls, ev.h * ev.w, self.heads, ev.loss_kind, L.ptr(self.ws),
                                        L.nbytes(self.ws), L.ptr(self.loss_out), L.ptr(ev.meters), ev.iou_thr, st), "eval_step")
        pl.trained_forward = False


class EvalStep:
    """The validation loop of reference trains.py:150-188 without a host round trip per batch: the forward pass in eval mode,
    the loss of every head (the stand-alone forwards' device code: the values of the `losses` modules, bit for bit), IoU, Dice
    and accuracy of the last head and the AverageMeter sums, captured once as ONE hipGraph and replayed per batch; the meters
    stay on the device and are read once per pass.

    evaluate(x, t) over a split (device tensors [M, C, H, W] / [M, K, H, W]): one repack of the weights from the current fp32
    parameters, the meters zeroed, a copy + replay per full batch, a tail of r < N images eagerly on a second plan of N = r
    (created on first use; not padded: the K-split of grid-starved layers depends on N) - the launches the module path makes,
    so `loss` and `iou` equal the module loop's to the bit. begin() / step(xb, tb) / result() are the same pass by hand, for
    a caller that wants `.last_logits` of every batch (val.py's mask export).
    use_graph=False issues the same launches eagerly.

    depth=L (1..4, a deep-supervision NestedUNet): the step's plans - static batch and tail - are pruned to the sub-network of
    head L (nunet_plan_create_pruned): one head, so result() and last_logits are head L's. per_head=True (a deep-supervision
    NestedUNet, no depth): the step issues nunet_eval_step_heads, result()["heads"] lists loss / iou / dice / acc / counts /
    per_class of every head - entry L - 1 is what EvalStep(depth=L) reports - and every other field is unchanged.

    weights=(flat_params, bnbuf): the step reads these arenas - flat fp32 device tensors in the order and size of
    Engine.flat_params / Engine.bnbuf, e.g. (ts.ema_params, ts.ema_bnbuf) of a TrainStep with a weight EMA - instead of the
    module's own: repack and forward take the parameter and BatchNorm arenas as arguments, so another set of weights needs no
    second module. num_batches_tracked stays the engine's (eval never reads it). depth= and per_head= work as without.

    tta="flips" (codes 0, 4, 8, 12; any H, W), "d4" (codes 0 .. 7, the eight distinct maps; H == W) or a tuple of geometric
    codes 0 .. 15 (the input pipeline's aug: rot90 count | hflip << 2 | vflip << 3): test-time augmentation. Per view, in order,
    the step forms the view of the input (nunet_dihedral_nchw), runs the forward on it and merges the logits of every head back
    into the source frame (nunet_tta_merge) - all inside the one captured graph. tta_merge="logit": the fp32 sum in view order
    divided once by the number of views; "prob": the mean of the sigmoids, clamped to [2^-23, 1 - 2^-23] and taken back to a
    logit. The merged prediction stays in logit space, so logits, last_logits, last_loss, result(), depth=, per_head=, weights=
    and the tail batch mean what they mean without it. None (default): no new launch."""

    def __init__(self, model, batch_shape, loss="BCEDiceLoss", use_graph=True, depth=None, per_head=False, weights=None, tta=None,
                 tta_merge="logit"):
        # (host-only checks first: a refused tta never touches the device)
        if tta_merge not in TTA_MERGES:
            raise L.NunetError("EvalStep: tta_merge %r is not one of %s" % (tta_merge, sorted(TTA_MERGES)))
        self.tta = tta_codes(tta, batch_shape[2], batch_shape[3])
        self.tta_merge, self.tta_mode = tta_merge, TTA_MERGES[tta_merge]
        if depth is not None:
            model.check_depth(depth, need_eval=False)     # (the step always runs the eval forward, whatever mode the module is in)
        if per_head:
            if depth is not None:
                raise L.NunetError("EvalStep: per_head=True scores the four heads of the whole network; depth=%r leaves one head" % (depth,))
            if model._unet or not getattr(model, "deep_supervision", False):
                raise L.NunetError("EvalStep: per_head=True needs a NestedUNet built with deep_supervision=True (one head otherwise)")
        self.depth, self.per_head = depth, bool(per_head)
        self.model = model
        self.eng = model.engine()
        self.flat_params, self.bnbuf = self.eng.flat_params, self.eng.bnbuf
        if weights is not None:
            if not isinstance(weights, (tuple, list)) or len(weights) != 2:
                raise L.NunetError("EvalStep: weights must be a (flat_params, bnbuf) pair of device tensors")
            fp, bb = weights
            for t, like, nm in ((fp, self.eng.flat_params, "flat_params"), (bb, self.eng.bnbuf, "bnbuf")):
                if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() != 1 or not t.is_contiguous():
                    raise L.NunetError("EvalStep: weights %s must be a flat contiguous fp32 tensor" % nm)
                if t.numel() != like.numel():
                    raise L.NunetError("EvalStep: weights %s has %d values, the model's arena %d" % (nm, t.numel(), like.numel()))
                if t.device != like.device:
                    raise L.NunetError("EvalStep: weights %s lives on %s, the model on %s" % (nm, t.device, like.device))
            self.flat_params, self.bnbuf = fp, bb
        n, cin, h, w = batch_shape
        if cin != model.input_channels:
            raise L.NunetError("EvalStep: batch_shape has %d channels, the model takes %d" % (cin, model.input_channels))
        self.n, self.cin, self.h, self.w = n, cin, h, w
        self.ncls = model.num_classes
        if loss not in LOSS_KINDS:
            raise L.NunetError("EvalStep: loss %r is not one of %s" % (loss, sorted(LOSS_KINDS)))
        if loss == "LovaszHingeLoss" and self.ncls != 1:
            raise L.NunetError("LovaszHingeLoss squeezes the class dimension (reference losses.py:126-127): num_classes must be 1")
        if self.ncls > L.EVAL_MAX_CLASSES:
            raise L.NunetError("EvalStep: %d classes, the metrics take up to %d" % (self.ncls, L.EVAL_MAX_CLASSES))
        self.loss_name, self.loss_kind = loss, LOSS_KINDS[loss]
        from .metrics import iou_logit_threshold
        self.iou_thr = iou_logit_threshold()
        self.use_graph = use_graph
        # one buffer: the step's meters, then (per_head) one nunet_eval_meters per head - one fill to zero them, one copy to read them
        msz = C.sizeof(L.EvalMeters)
        self._meters_all = torch.zeros((5 if self.per_head else 1) * msz, dtype=torch.uint8, device=self.eng.device)
        self.meters = self._meters_all[:msz]
        self.head_meters = self._meters_all[msz:] if self.per_head else None
        self.main = _EvalBatch(self, n)
        self.tail = None
        self._last = self.main
        self._packed = set()
        self.heads = self.main.heads

    @property
    def logits(self):
        """[heads, N, K, H, W] of the static batch (the tail batch has its own: see last_logits)"""
        return self.main.logits

    @property
    def last_logits(self):
        """[n, K, H, W]: the last head's logits of the batch step() ran last"""
        return self._last.logits[-1]

    @property
    def last_loss(self):
        """device fp32 [heads + 1]: per head, then their mean, of the batch step() ran last"""
        return self._last.loss_out

    def _check_engine(self):
        if self.model._engine is not self.eng or not self.eng.intact():
            raise L.NunetError("the module's parameter arenas were re-homed (moved to another device / parameters replaced) "
                               "after this EvalStep was built: it would read orphaned memory. Build a new EvalStep.")

    def begin(self):
        """Start a pass: repack the weights into this step's own arena (the parameters moved since the last pass), zero the meters."""
        self._check_engine()
        self.main.repack(self)
        self._packed = {self.main.n}
        self._zero_meters()
        if self.use_graph and self.main.graph is None:
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                self.main.issue(self)          # eager once: one-time launch attributes are set outside the capture
            torch.cuda.current_stream().wait_stream(s)
            torch.cuda.synchronize()
            self.main.graph = _NativeGraph(s, lambda: self.main.issue(self))
            torch.cuda.synchronize()
            self._zero_meters()

    def _zero_meters(self):
        self._meters_all.zero_()

    def step(self, xb, tb):
        """One batch of a pass: the static batch size replays the captured step, fewer images run eagerly on a plan of that size."""
        r = xb.size(0)
        if r == self.n:
            b = self.main
        else:
            if r > self.n or r < 1:
                raise L.NunetError("EvalStep: a batch of %d images (1 .. %d)" % (r, self.n))
            if self.tail is None or self.tail.n != r:
                self.tail = _EvalBatch(self, r)
                self._packed.discard(r)
            b = self.tail
            if r not in self._packed:
                b.repack(self)
                self._packed.add(r)
        b.x.copy_(xb, non_blocking=True)
        b.t.copy_(tb, non_blocking=True)
        if b.graph is not None:
            b.graph.replay()
        else:
            b.issue(self)
        self._last = b

    def result(self):
        """The pass so far: OrderedDict(loss, iou, dice, acc: sample-weighted means of the batch values, the reference's
        AverageMeter; samples; counts: per-class tp / fp / fn / tn lists; per_class: metrics.scores_from_counts of them,
        dataset level). One host sync."""
        from collections import OrderedDict
        from .metrics import scores_from_counts
        K = self.ncls

        def fields(m, with_samples):
            k = max(m.samples, 1.0)
            d = OrderedDict([("loss", m.loss_sum / k), ("iou", m.iou_sum / k), ("dice", m.dice_sum / k), ("acc", m.acc_sum / k)])
            if with_samples:
                d["samples"] = int(m.samples)
            d["counts"] = OrderedDict((nm, [int(v) for v in getattr(m, nm)[:K]]) for nm in ("tp", "fp", "fn", "tn"))
            d["per_class"] = scores_from_counts(*d["counts"].values())
            return d

        sz = C.sizeof(L.EvalMeters)
        raw = self._meters_all.cpu().numpy().tobytes()
        out = fields(L.EvalMeters.from_buffer_copy(raw[:sz]), True)
        if self.per_head:
            out["heads"] = [fields(L.EvalMeters.from_buffer_copy(raw[(h + 1) * sz:(h + 2) * sz]), False) for h in range(self.heads)]
        return out

    def evaluate(self, x, t):
        self.begin()
        for k in range(0, x.size(0), self.n):
            self.step(x[k:k + self.n], t[k:k + self.n])
        return self.result()


class _SegProgram:
    """nunet_seg_* wrapper with the replay() surface of torch.cuda.CUDAGraph: the step body is run twice on `side_stream` - a dry
    pass that launches nothing and finds the cross-lane events, then the pass that records the flag-synchronised lanes."""

    def __init__(self, side_stream, body):
        import ctypes as C
        lib = L.lib()
        self.stream = side_stream            # the program replays on this stream: keep it alive
        self.handle = None
        with torch.cuda.stream(side_stream):
            for mode in (1, 2):                      # NUNET_SEG_DRY, then NUNET_SEG_FLAGS
                L.check(lib.nunet_seg_begin(L.stream(), mode), "seg_begin")
                try:
                    body()
                finally:
                    h = C.c_void_p()
                    rc = lib.nunet_seg_end(L.stream(), C.byref(h))
                L.check(rc, "seg_end")
        self.handle = h

    def info(self):
        import ctypes as C
        v = [C.c_int32() for _ in range(4)]
        L.check(L.lib().nunet_seg_info(self.handle, *[C.byref(x) for x in v]), "seg_info")
        return dict(zip(("graph_launches", "event_records", "event_waits", "kernel_nodes"), (x.value for x in v)))

    def replay(self):
        L.check(L.lib().nunet_seg_launch(self.handle, L.stream()), "seg_launch")

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                L.lib().nunet_seg_destroy(self.handle)
                self.handle = None
        except Exception:
            pass


class _NativeGraph:
    """nunet_graph_* wrapper with the replay() surface of torch.cuda.CUDAGraph."""

    def __init__(self, side_stream, body):
        import ctypes as C
        lib = L.lib()
        with torch.cuda.stream(side_stream):
            L.check(lib.nunet_graph_begin(L.stream()), "graph_begin")
            try:
                body()
            finally:
                h = C.c_void_p()
                rc = lib.nunet_graph_end(L.stream(), C.byref(h))
            L.check(rc, "graph_end")
        self.handle = h

    def info(self):
        import ctypes as C
        v = [C.c_int32() for _ in range(3)]
        L.check(L.lib().nunet_graph_info(self.handle, *[C.byref(x) for x in v]), "graph_info")
        return dict(zip(("nodes", "edges", "lanes"), (x.value for x in v)))

    def replay(self):
        L.check(L.lib().nunet_graph_launch(self.handle, L.stream()), "graph_launch")

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                L.lib().nunet_graph_destroy(self.handle)
                self.handle = None
        except Exception:
            pass


def cosine_lr(base_lr, min_lr, epoch, t_max):
    """CosineAnnealingLR closed form as configured at reference trains.py:237-239."""
    return min_lr + 0.5 * (base_lr - min_lr) * (1.0 + math.cos(math.pi * epoch / t_max))
