#!/usr/bin/env python3
"""Training driver for the MI355X UNet++ path — the counterpart of reference trains.py
(flags :31-103, loop :106-188, main :191-356) on the seeded synthetic blob dataset
(pytorch_nested-unet_amd/synth.py; DSB2018 is not available offline), or - --dataset NAME - on a folder in the reference's layout,
inputs/NAME/images/*<img_ext> and inputs/NAME/masks/<class>/*<mask_ext> (dataset.FolderDataset): images of any size, decoded on the
host, resized on the device inside the captured step (TrainStep(resize=True)). --source_size LO,HI runs that path on the blobs.

Same artefacts as the reference: models/<name>/config.yml (trains.py:206-207),
models/<name>/log.csv with columns epoch, lr, loss, iou, val_loss, val_iou (:304-311,331-339),
models/<name>/model.pth = state_dict at the best val IoU (:344-349), early stopping (:351-354).
The `lr` column logs the scheduler's current lr (the reference logs the constant initial lr, :332).
Beside the fused step, validation (trains.py:150-188) runs as the captured EvalStep (--eval_step false: the module loop; the
same val_loss and val_iou to the bit); --val_metrics true appends val_dice, val_acc to the epoch line and to log.csv;
--val_tta flips|d4 validates under test-time augmentation (EvalStep(tta=...)).

Data parallel (new capability; the reference is single-device, trains.py:223): launch one process per GPU,
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port 29500 \
           train.py --gpus N [flags]
--batch_size stays the PER-GPU batch (weak scaling: the global batch is N x batch_size, every replica normalises its
BatchNorm over its own batch_size images like the single-GPU step), rank r consumes slice r of every global batch,
gradients are averaged over RCCL, rank 0's BatchNorm buffers are broadcast before validation and rank 0 writes the
artefacts.
"""
import argparse
import os
import time
from collections import OrderedDict

os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # dmabuf IPC: RCCL between processes needs it on this image

import torch  # noqa: E402
import yaml  # noqa: E402

import torch.distributed as dist

import nunet_amd
from nunet_amd import archs, losses, parallel
from nunet_amd import _lib as L
from nunet_amd.metrics import iou_counts, iou_from_counts, seg_sums
from nunet_amd.trainer import EvalStep, TrainStep, cosine_lr
from nunet_amd.utils import AverageMeter, str2bool

ARCH_NAMES = archs.__all__
LOSS_NAMES = losses.__all__ + ['BCEWithLogitsLoss']      # trains.py:27-28 (a new list: the module's stays the reference's)


def parse_args():
    p = argparse.ArgumentParser()
    p.add_argument('--name', default=None, help='model name: (default: arch+timestamp)')
    p.add_argument('--epochs', default=100, type=int)
    p.add_argument('-b', '--batch_size', default=16, type=int)
    p.add_argument('--arch', '-a', default='NestedUNet', choices=ARCH_NAMES)
    p.add_argument('--deep_supervision', default=False, type=str2bool)
    p.add_argument('--input_channels', default=3, type=int)
    p.add_argument('--num_classes', default=1, type=int)
    p.add_argument('--input_w', default=96, type=int)
    p.add_argument('--input_h', default=96, type=int)
    p.add_argument('--loss', default='BCEDiceLoss', choices=LOSS_NAMES)   # every loss runs inside the fused step (TrainStep)
    p.add_argument('--dataset', default='synthetic_blobs')
    p.add_argument('--optimizer', default='SGD', choices=['Adam', 'SGD'])
    p.add_argument('--lr', '--learning_rate', default=1e-3, type=float)
    p.add_argument('--momentum', default=0.9, type=float)
    p.add_argument('--weight_decay', default=1e-4, type=float)
    p.add_argument('--nesterov', default=False, type=str2bool)
    p.add_argument('--scheduler', default='CosineAnnealingLR',
                   choices=['CosineAnnealingLR', 'ReduceLROnPlateau', 'MultiStepLR', 'ConstantLR'])    # reference trains.py:87-88
    p.add_argument('--min_lr', default=1e-5, type=float)
    p.add_argument('--factor', default=0.1, type=float)
    p.add_argument('--patience', default=2, type=int)
    p.add_argument('--milestones', default='1,2', type=str)
    p.add_argument('--gamma', default=2 / 3, type=float)
    p.add_argument('--early_stopping', default=-1, type=int)
    p.add_argument('--num_workers', default=0, type=int, help='accepted for compatibility; data is generated in-process')
    # additions
    p.add_argument('--dtype', default='bf16', choices=['fp32', 'bf16', 'fp16'])
    p.add_argument('--loss_scale', default='none', choices=['none', 'dynamic'],
                   help='dynamic loss scaling (torch.amp.GradScaler semantics; inside the fused step on the device)')
    p.add_argument('--init_scale', default=65536.0, type=float, help='initial loss scale (--loss_scale dynamic)')
    p.add_argument('--growth_interval', default=2000, type=int, help='clean steps between scale growths (--loss_scale dynamic)')
    p.add_argument('--clip_grad_norm', default=0.0, type=float,
                   help='max_norm of torch.nn.utils.clip_grad_norm_ over all parameters, inside the fused step (0: off)')
    p.add_argument('--ema_decay', default=0.0, type=float,
                   help='decay of an exponential moving average of the weights and BatchNorm statistics, kept inside the fused step '
                        '(torch.optim.swa_utils.AveragedModel + get_ema_multi_avg_fn; 0: off). The averaged model is validated every '
                        'epoch (ema_val_loss, ema_val_iou) and saved as model_ema.pth at its best val IoU')
    p.add_argument('--ema_warmup', default=False, type=str2bool,
                   help='with --ema_decay: the decay of update t is min(ema_decay, (1 + t) / (10 + t))')
    p.add_argument('--train_size', default=512, type=int)
    p.add_argument('--val_size', default=128, type=int)
    p.add_argument('--seed', default=41, type=int)
    p.add_argument('--gpus', default=0, type=int, help='number of ranks this job was launched with (checked against WORLD_SIZE; 0: do not check)')
    p.add_argument('--device_pipeline', default=True, type=str2bool,
                   help='feed the fused step with the decoded uint8 batch and run Normalize, /255, rot90 / flips and the layout change on '
                        'the device (reference dataset.py:66-74, trains.py:258-266); False: float tensors prepared on the host')
    p.add_argument('--eval_step', default=True, type=str2bool,
                   help='with the fused step: validate through the captured EvalStep (forward, losses, IoU / Dice / accuracy and the '
                        'meters on the device, one read per pass; same val_loss and val_iou to the bit); False: the module loop')
    p.add_argument('--val_metrics', default=False, type=str2bool,
                   help='also log val_dice (reference metrics.py dice_coef) and val_acc (pixel accuracy) per epoch, after images_per_sec')
    p.add_argument('--val_tta', default='none', choices=('none', 'flips', 'd4'),
                   help='validate under test-time augmentation inside the EvalStep: the 4 flips, or the 8 rotations and flips of a square '
                        'input, merged in logit space on the device (needs --eval_step true)')
    p.add_argument('--augment', default=False, type=str2bool, help='RandomRotate90 + Flip per sample (trains.py:258-259), device pipeline only')
    p.add_argument('--color_augment', default=False, type=str2bool,
                   help='OneOf([HueSaturationValue, RandomBrightness, RandomContrast], p=1) per sample (trains.py:260-264; modelled on '
                        'albumentations, see DESIGN.md), device pipeline only; drawn from the same generator stream as --augment')
    p.add_argument('--img_ext', default='.png', help='image file extension of a folder dataset (trains.py:67)')
    p.add_argument('--mask_ext', default='.png', help='mask file extension of a folder dataset (trains.py:69)')
    p.add_argument('--source_size', default=None, type=str,
                   help='LO,HI: draw the synthetic blobs at per-sample heights and widths from LO..HI and let the device resize them to '
                        'input_h x input_w (the path a folder dataset takes, without files)')
    return p.parse_args()


def ragged_sets(config):
    """(train samples, val samples) as lists of (image uint8 [H,W,3], mask uint8 [H,W,K]) at their own sizes: a folder in the
    reference's layout (inputs/<dataset>/images, masks/<class>; split as trains.py:255), or the synthetic blobs at sizes drawn
    from --source_size."""
    import numpy as np
    if config['dataset'] != 'synthetic_blobs':
        sets = [nunet_amd.dataset.FolderDataset(config['dataset'], config['img_ext'], config['mask_ext'], config['num_classes'], split=s)
                for s in ('train', 'val')]
        return tuple([ds[i] for i in range(len(ds))] for ds in sets)
    lo, hi = (int(v) for v in config['source_size'].split(','))
    if not 1 <= lo <= hi <= L.RESIZE_MAX_EXTENT:
        raise SystemExit('--source_size %s: LO,HI with 1 <= LO <= HI <= %d' % (config['source_size'], L.RESIZE_MAX_EXTENT))
    out = []
    for count, seed in ((config['train_size'], 1000), (config['val_size'], 2000)):
        g = np.random.default_rng(seed)
        sizes = g.integers(lo, hi + 1, (count, 2))
        pairs = [nunet_amd.synth.synth_blob_pairs_u8(1, int(h), int(w), seed=seed + 1 + i) for i, (h, w) in enumerate(sizes)]
        out.append([(img[0], msk[0]) for img, msk in pairs])
    return tuple(out)


def ragged_to_floats(samples, h, w, bs):
    """the val transform (Resize, Normalize; trains.py:269-272) of ragged samples on the device -> float32 (images, masks)"""
    D = nunet_amd.dataset
    xs, ts = [], []
    for k in range(0, len(samples), bs):
        part = samples[k:k + bs]
        xs.append(D.resize_images(*D.pack_ragged([p[0] for p in part]), (h, w)))
        ts.append(D.resize_masks(*D.pack_ragged([p[1] for p in part]), (h, w), channels=part[0][1].shape[2]))
    return torch.cat(xs), torch.cat(ts)


def make_split(n, h, w, cin, ncls, seed):
    img, msk = nunet_amd.synth.synth_split(n, h, w, cin, ncls, seed)
    return torch.from_numpy(img), torch.from_numpy(msk)


class PlateauLR:
    """lr_scheduler.ReduceLROnPlateau(optimizer, factor, patience, min_lr) as configured at reference trains.py:240-243
    (mode 'min', rel threshold 1e-4, no cooldown), stepped with the validation loss (trains.py:325-326)."""

    def __init__(self, lr, factor, patience, min_lr):
        self.lr, self.factor, self.patience, self.min_lr = lr, factor, patience, min_lr
        self.best, self.bad = float('inf'), 0

    def step(self, metric):
        if metric < self.best * (1.0 - 1e-4):
            self.best, self.bad = metric, 0
        else:
            self.bad += 1
        if self.bad > self.patience:
            new = max(self.lr * self.factor, self.min_lr)
            if self.lr - new > 1e-8:
                self.lr = new
            self.bad = 0
        return self.lr


def multistep_lr(base_lr, milestones, gamma, epoch):
    """lr_scheduler.MultiStepLR closed form (trains.py:244-245). The reference builds it but never steps it
    (trains.py:323-326 step only the cosine and plateau schedulers); this driver does step it."""
    return base_lr * gamma ** sum(1 for m in milestones if epoch >= m)


def validate(config, data, model, criterion, ev=None):
    """reference trains.py:150-188. ev (an EvalStep): the same pass as captured replays, the meters read once; the module
    loop below otherwise (two host round trips per batch; a third for Dice and accuracy under --val_metrics)."""
    x, t = data
    if ev is not None:
        r = ev.evaluate(x, t)
        return OrderedDict((k, r[k]) for k in ('loss', 'iou', 'dice', 'acc'))
    extra = config.get('val_metrics', False)
    avg = {'loss': AverageMeter(), 'iou': AverageMeter(), 'dice': AverageMeter(), 'acc': AverageMeter()}
    model.eval()
    bs = config['batch_size']
    with torch.no_grad():
        for k in range(0, x.size(0), bs):
            xb, tb = x[k:k + bs].contiguous(), t[k:k + bs].contiguous()
            out = model(xb)
            if config['deep_supervision']:
                loss = sum(criterion(o, tb) for o in out) / len(out)
                last = out[-1]
            else:
                loss = criterion(out, tb)
                last = out
            avg['loss'].update(loss.item(), xb.size(0))
            avg['iou'].update(iou_from_counts(iou_counts(last.contiguous(), tb)), xb.size(0))
            if extra:
                s = L.read_struct(seg_sums(last.contiguous(), tb), L.SegSums)
                avg['dice'].update((2.0 * sum(s.soft_i) + 1e-5) / (sum(s.soft_p) + sum(s.soft_t) + 1e-5), xb.size(0))
                avg['acc'].update((sum(s.tp) + sum(s.tn)) / float(last.numel()), xb.size(0))
    return OrderedDict((k, avg[k].avg) for k in (('loss', 'iou', 'dice', 'acc') if extra else ('loss', 'iou')))


def main():
    config = vars(parse_args())
    local_rank = int(os.environ.get('LOCAL_RANK', '0'))
    torch.cuda.set_device(local_rank)
    rank, world = parallel.init_from_env('nccl')
    if config['gpus'] and config['gpus'] != world:
        raise SystemExit('--gpus %d but WORLD_SIZE is %d: launch with torch.distributed.run --nproc-per-node %d' % (config['gpus'], world, config['gpus']))
    if config['name'] is None:
        config['name'] = '%s_%s_%s' % (config['dataset'], config['arch'], 'wDS' if config['deep_supervision'] else 'woDS')
    if rank == 0:
        os.makedirs('models/%s' % config['name'], exist_ok=True)
        print('-' * 20)
        for k, v in config.items():
            print('%s: %s' % (k, v))
        print('-' * 20)
        with open('models/%s/config.yml' % config['name'], 'w') as f:
            yaml.dump(config, f)

    criterion = getattr(losses, config['loss'])().cuda()
    torch.manual_seed(config['seed'])
    model = archs.__dict__[config['arch']](config['num_classes'], config['input_channels'], config['deep_supervision'],
                                           dtype=config['dtype'])
    model = model.cuda()
    h, w, bs = config['input_h'], config['input_w'], config['batch_size']
    fused = not (config['loss'] == 'LovaszHingeLoss' and config['num_classes'] != 1)   # TrainStep: SGD or Adam, any loss
    if world > 1 and not fused:
        raise SystemExit('data parallel runs the fused step: multi-class LovaszHingeLoss is not fused')
    val_tta = None if config['val_tta'] == 'none' else config['val_tta']
    if val_tta is not None and not (fused and config['eval_step']):
        raise SystemExit('--val_tta %s merges the views inside the captured EvalStep: it needs the fused step and --eval_step true' % val_tta)
    if val_tta == 'd4' and h != w:
        raise SystemExit('--val_tta d4 rotates by 90 degrees: input_h %d must equal input_w %d (use --val_tta flips)' % (h, w))
    # ragged sources (a folder dataset, or --source_size): decoded samples at their own sizes, resized on the device
    ragged = config['dataset'] != 'synthetic_blobs' or config['source_size'] is not None
    if ragged:
        if not (fused and config['device_pipeline'] and config['input_channels'] == 3):
            raise SystemExit('a folder dataset / --source_size runs in the device pipeline (fused step, --device_pipeline, 3 input channels)')
        train_rag, val_rag = ragged_sets(config)
        config['train_size'], config['val_size'] = len(train_rag), len(val_rag)
        train = None
        val = ragged_to_floats(val_rag, h, w, bs)
    else:
        # the synthetic splits live in HBM (a few MB); batches are gathered on the device
        train = tuple(v.cuda() for v in make_split(config['train_size'], h, w, config['input_channels'], config['num_classes'], 1000))
        val = tuple(v.cuda() for v in make_split(config['val_size'], h, w, config['input_channels'], config['num_classes'], 2000))
    steps = config['train_size'] // (bs * world)          # drop_last=True (trains.py:296); global batch = world x bs

    u8 = ragged or (fused and config['device_pipeline'] and config['input_channels'] == 3 and config['num_classes'] == 1)
    color = bool(config['color_augment'] and u8)
    if config['color_augment'] and not u8:
        raise SystemExit('--color_augment runs in the device pipeline (fused step, --device_pipeline, 3 input channels, 1 class)')
    scaling = None if config['loss_scale'] == 'none' else dict(init_scale=config['init_scale'], growth_interval=config['growth_interval'])
    clip = config['clip_grad_norm'] if config['clip_grad_norm'] > 0 else None
    ema = config['ema_decay'] if config['ema_decay'] > 0 else None
    if ema is not None and not fused:
        raise SystemExit('--ema_decay averages inside the fused step: multi-class LovaszHingeLoss is not fused')
    if fused:
        model.train()
        # the largest batch of sources either pool can be handed: the bs largest samples
        rag = dict(resize=True, source_capacity=max(sum(sorted((p[k].size for p in train_rag), reverse=True)[:bs]) for k in (0, 1))) if ragged else {}
        if config['optimizer'] == 'Adam':      # torch.optim.Adam(params, lr, weight_decay) with its default betas / eps (trains.py:225-227)
            ts = TrainStep(model, (bs, config['input_channels'], h, w), lr=config['lr'], weight_decay=config['weight_decay'],
                           loss=config['loss'], input_u8=u8, optimizer='Adam', loss_scale=scaling,
                           clip_grad_norm=clip, ema_decay=ema, ema_warmup=config['ema_warmup'], color_aug=color, **rag)
        else:
            ts = TrainStep(model, (bs, config['input_channels'], h, w), lr=config['lr'], momentum=config['momentum'],
                           weight_decay=config['weight_decay'], nesterov=config['nesterov'], loss=config['loss'], input_u8=u8,
                           loss_scale=scaling, clip_grad_norm=clip, ema_decay=ema, ema_warmup=config['ema_warmup'], color_aug=color, **rag)
        if ragged:
            pack = nunet_amd.dataset.pack_ragged
            ts.capture(pack([p[0] for p in train_rag[:bs]]), pack([p[1] for p in train_rag[:bs]]))
            aug_gen = torch.Generator().manual_seed(config['seed'] + 1)
        elif u8:
            # the decoded set (what the reference's Dataset holds after cv2.imread, dataset.py:56-64) lives in HBM as uint8
            raw, m8 = nunet_amd.synth.synth_blob_pairs_u8(config['train_size'], h, w, seed=1000)
            train_u8 = (torch.from_numpy(raw).cuda(), torch.from_numpy(m8).cuda())
            ts.capture(train_u8[0][:bs], train_u8[1][:bs])
            aug_gen = torch.Generator().manual_seed(config['seed'] + 1)
        else:
            ts.capture(train[0][:bs], train[1][:bs])
        if rank == 0:
            print('=> fused training step (TrainStep): %s, %s%s%s%s' % (config['optimizer'], config['loss'],
                                                                        ', dynamic loss scaling' if scaling else '',
                                                                        ', grad norm clipped at %g' % clip if clip else '',
                                                                        ', weight EMA %g%s' % (ema, ' with warm-up' if config['ema_warmup'] else '')
                                                                        if ema else ''))
    else:
        params = filter(lambda p: p.requires_grad, model.parameters())
        if config['optimizer'] == 'Adam':
            optimizer = torch.optim.Adam(params, lr=config['lr'], weight_decay=config['weight_decay'])
        else:
            optimizer = torch.optim.SGD(params, lr=config['lr'], momentum=config['momentum'], nesterov=config['nesterov'],
                                        weight_decay=config['weight_decay'])
        scaler = torch.amp.GradScaler('cuda', **scaling) if scaling else None
        clip_params = [p for p in model.parameters() if p.requires_grad]

    # validation: the captured EvalStep beside the fused step (its own plan and arena; built behind ts.capture)
    ev = EvalStep(model, (bs, config['input_channels'], h, w), loss=config['loss'], tta=val_tta) if fused and config['eval_step'] else None
    if ev is not None and rank == 0:
        print('=> captured validation step (EvalStep)' + (', test-time augmentation %s (%d views)' % (val_tta, len(ev.tta)) if val_tta else ''))
    # the averaged weights through a second EvalStep that reads the TrainStep's averaged arenas (no second module)
    ev_ema = (EvalStep(model, (bs, config['input_channels'], h, w), loss=config['loss'], weights=(ts.ema_params, ts.ema_bnbuf), tta=val_tta)
              if ema is not None else None)
    log_keys = (('epoch', 'lr', 'loss', 'iou', 'val_loss', 'val_iou', 'images_per_sec') + (('val_dice', 'val_acc') if config['val_metrics'] else ())
                + (('ema_val_loss', 'ema_val_iou') if ema is not None else ()))
    best_ema_iou = 0
    log = OrderedDict([(k, []) for k in log_keys])
    best_iou, trigger = 0, 0
    plateau = PlateauLR(config['lr'], config['factor'], config['patience'], config['min_lr'])
    g = torch.Generator().manual_seed(config['seed'])   # host-side permutation: identical for any device
    for epoch in range(config['epochs']):
        if config['scheduler'] == 'CosineAnnealingLR':
            lr = cosine_lr(config['lr'], config['min_lr'], epoch, config['epochs'])
        elif config['scheduler'] == 'MultiStepLR':
            lr = multistep_lr(config['lr'], [int(e) for e in config['milestones'].split(',')], config['gamma'], epoch)
        elif config['scheduler'] == 'ReduceLROnPlateau':
            lr = plateau.lr
        else:
            lr = config['lr']
        perm = torch.randperm(config['train_size'], generator=g).cuda()
        model.train()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if fused:
            ts.set_lr(lr)
            ts.reset_meters()
            for k in range(steps):
                lo = (k * world + rank) * bs                             # slice `rank` of global batch k
                idx = perm[lo:lo + bs]
                if u8:
                    aug = nunet_amd.dataset.draw_augmentation(bs, aug_gen, 'cuda') if config['augment'] else None
                    col = nunet_amd.dataset.draw_color_augmentation(bs, aug_gen, 'cuda') if color else None
                    if ragged:
                        part = [train_rag[i] for i in idx.tolist()]
                        ts.step_u8_ragged(*(pack([p[0] for p in part]) + pack([p[1] for p in part])), aug=aug, color=col)
                    else:
                        ts.step_u8(train_u8[0][idx], train_u8[1][idx], aug, col)
                else:
                    ts.step(train[0][idx], train[1][idx])
            tl, ti = ts.epoch_stats()
            scale_info = ts.scaler_stats()
            norm_info = ts.grad_norm_stats()
            if world > 1:                                                # epoch means over all ranks' (equal-sized) batches
                m = torch.tensor([tl, ti], dtype=torch.float64, device='cuda')
                dist.all_reduce(m)
                tl, ti = (m / world).tolist()
                ts.sync_bn_buffers()                                     # rank 0's running statistics are the model's
        else:
            for gpar in optimizer.param_groups:
                gpar['lr'] = lr
            ml, mi = AverageMeter(), AverageMeter()
            skipped = 0
            norms = []
            for k in range(steps):                                       # reference trains.py:113-135
                idx = perm[k * bs:(k + 1) * bs]
                xb, tb = train[0][idx], train[1][idx]
                out = model(xb)
                if config['deep_supervision']:
                    loss = sum(criterion(o, tb) for o in out) / len(out)
                    last = out[-1]
                else:
                    loss = criterion(out, tb)
                    last = out
                optimizer.zero_grad()
                if scaler is not None:
                    scaler.scale(loss).backward()
                    if clip:
                        scaler.unscale_(optimizer)
                        norms.append(torch.nn.utils.clip_grad_norm_(clip_params, clip))
                    scaler.step(optimizer)
                    s0 = scaler.get_scale()
                    scaler.update()
                    skipped += int(scaler.get_scale() < s0)       # (a backoff: this step found an inf / NaN and was skipped)
                else:
                    loss.backward()
                    if clip:
                        norms.append(torch.nn.utils.clip_grad_norm_(clip_params, clip))
                    optimizer.step()
                ml.update(loss.item(), bs)
                mi.update(iou_from_counts(iou_counts(last.detach().contiguous(), tb)), bs)
            tl, ti = ml.avg, mi.avg
            scale_info = (scaler.get_scale(), skipped) if scaler is not None else None
            norm_info = None
            if clip:
                nv = torch.stack(norms)
                nv = nv[torch.isfinite(nv)]                       # (steps skipped by the scaler do not count)
                norm_info = dict(mean=float(nv.mean()) if nv.numel() else 0.0, peak=float(nv.max()) if nv.numel() else 0.0,
                                 clipped=int((nv > clip).sum()))
        torch.cuda.synchronize()
        ips = steps * bs * world / (time.perf_counter() - t0)
        val_log = validate(config, val, model, criterion, ev)             # every rank: identical replicas, identical numbers
        ema_log = validate(config, val, model, criterion, ev_ema) if ev_ema is not None else None
        if config['scheduler'] == 'ReduceLROnPlateau':
            plateau.step(val_log['loss'])                                # trains.py:325-326
        trigger += 1
        improved = val_log['iou'] > best_iou
        if rank == 0:
            print('Epoch [%d/%d] loss %.4f - iou %.4f - val_loss %.4f - val_iou %.4f - %.0f img/s'
                  % (epoch, config['epochs'], tl, ti, val_log['loss'], val_log['iou'], ips)
                  + (' - val_dice %.4f - val_acc %.4f' % (val_log['dice'], val_log['acc']) if config['val_metrics'] else '')
                  + (' - loss scale %g, %d steps skipped' % scale_info if scale_info is not None else '')
                  + (' - grad norm %.4g/%.4g, %d steps clipped' % (norm_info['mean'], norm_info['peak'], norm_info['clipped'])
                     if norm_info is not None else '')
                  + (' - ema_val_loss %.4f - ema_val_iou %.4f' % (ema_log['loss'], ema_log['iou']) if ema_log is not None else ''))
            for k, v in zip(log, (epoch, lr, tl, ti, val_log['loss'], val_log['iou'], ips) + ((val_log['dice'], val_log['acc']) if config['val_metrics'] else ())
                            + ((ema_log['loss'], ema_log['iou']) if ema_log is not None else ())):
                log[k].append(v)
            with open('models/%s/log.csv' % config['name'], 'w') as f:
                f.write(','.join(log.keys()) + '\n')
                for r in range(len(log['epoch'])):
                    f.write(','.join(str(log[k][r]) for k in log) + '\n')
            if improved:
                torch.save(model.state_dict(), 'models/%s/model.pth' % config['name'])
                print("=> saved best model")
            if ema_log is not None and ema_log['iou'] > best_ema_iou:
                torch.save(ts.ema_state_dict(), 'models/%s/model_ema.pth' % config['name'])
                print("=> saved best EMA model")
        if ema_log is not None and ema_log['iou'] > best_ema_iou:
            best_ema_iou = ema_log['iou']
        if improved:
            best_iou = val_log['iou']
            trigger = 0
        if 0 <= config['early_stopping'] <= trigger:
            if rank == 0:
                print("=> early stopping")
            break
    if dist.is_initialized():
        dist.destroy_process_group()


if __name__ == '__main__':
    main()
