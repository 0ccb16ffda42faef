#!/usr/bin/env python3
"""Evaluation driver — counterpart of reference val.py:31-109: rebuild the model from
models/<name>/config.yml, load model.pth, run the validation split, print the mean IoU and write
sigmoid(output)*255 masks per class to outputs/<name>/<class>/<id>.jpg (val.py:100-105; PIL here,
cv2 is not in the image).

A checkpoint trained with --deep_supervision true can be cut back at inference time: --depth L (1..4) evaluates and exports
masks from the network pruned to the blocks that feed head L; --per_head true adds one IoU / Dice / Acc / loss line per head
of the whole network, so one validation pass shows which depth would do.

--ema true evaluates models/<name>/model_ema.pth, the averaged weights train.py --ema_decay saved at their best val IoU.

--full_res true (a folder dataset or a --source_size run) leaves the reference's Resize out: every validation image is predicted
at its own size from overlapping input_h x input_w tiles (nunet_amd.tiled.TiledPredictor, --tile_overlap O), the masks have the
sources' sizes and IoU / Dice / Acc are means over images at that resolution. Composes with --depth and --ema.

--tta flips|d4 evaluates under test-time augmentation (EvalStep(tta=...)): the four flips, or the eight rotations and flips of a
square input, merged on the device in logit space (--tta_merge logit) or as probabilities (--tta_merge prob); the metrics, the
per-head table and the exported masks come from the merged logits. Composes with --depth, --per_head and --ema, not with
--full_res."""
import argparse
import os
import sys

import numpy as np
import torch
import yaml

import nunet_amd
from nunet_amd import archs
from nunet_amd.metrics import sigmoid_masks_u8
from nunet_amd.trainer import EvalStep
from nunet_amd.utils import str2bool


FULL_RES_GROUP_BYTES = 32 << 20      # sources of one TiledPredictor.predict call (one more image always fits)


def full_res(args, config, model, samples):
    """--full_res true: every validation image at its own size through TiledPredictor (tile = input_h x input_w, N = batch_size,
    one captured graph), masks of the sources' sizes under the names the resized path uses, IoU / Dice / Acc as the mean over
    images and the dataset-level per-class table."""
    from nunet_amd.dataset import pack_ragged
    from nunet_amd.metrics import scores_from_counts
    from nunet_amd.tiled import TiledPredictor
    K = config['num_classes']
    for c in range(K):
        os.makedirs(os.path.join('outputs', config['name'], str(c)), exist_ok=True)
    groups, size = [[]], 0
    for i, (img, _) in enumerate(samples):
        if groups[-1] and size + img.size > FULL_RES_GROUP_BYTES:
            groups.append([])
            size = 0
        groups[-1].append(i)
        size += img.size
    cap = max(sum(samples[i][0].size for i in g) for g in groups)
    tp = TiledPredictor(model, (config['batch_size'], config['input_channels'], config['input_h'], config['input_w']),
                        overlap=args.tile_overlap, source_capacity=cap, depth=args.depth)
    iou, dice, acc, tiles = [], [], [], 0
    counts = {nm: [0] * K for nm in ('tp', 'fp', 'fn', 'tn')}
    with torch.no_grad():
        for g in groups:
            r = tp.predict(*(pack_ragged([samples[i][0] for i in g]) + pack_ragged([samples[i][1] for i in g])))
            iou, dice, acc, tiles = iou + r['iou'], dice + r['dice'], acc + r['acc'], tiles + sum(r['tiles'])
            for nm in counts:
                counts[nm] = [a + b for a, b in zip(counts[nm], r['counts'][nm])]
            if not args.no_images:
                from PIL import Image
                for i, m in zip(g, r['masks']):
                    m = m.cpu().numpy()
                    for c in range(K):
                        Image.fromarray(m[c]).save(os.path.join('outputs', config['name'], str(c), 'val_%04d.jpg' % i))
    if args.depth is not None:
        print('depth: %d' % args.depth)
    if args.ema:
        print('weights: EMA (model_ema.pth)')
    print('full resolution: %d images, %d tiles of %d x %d, overlap %d' % (len(samples), tiles, tp.th, tp.tw, tp.overlap))
    print('IoU: %.4f' % np.mean(iou))
    print('Dice: %.4f' % np.mean(dice))
    print('Acc: %.4f' % np.mean(acc))
    per = scores_from_counts(*(counts[nm] for nm in ('tp', 'fp', 'fn', 'tn')))
    names = list(per)
    print('class ' + ' '.join('%11s' % nm for nm in names))
    for c in range(K):
        print('%5d ' % c + ' '.join('%11.4f' % per[nm][0][c] for nm in names))
    print('micro ' + ' '.join('%11.4f' % per[nm][1] for nm in names))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--name', default=None, help='model name')
    ap.add_argument('--no_images', action='store_true')
    ap.add_argument('--depth', default=None, type=int, choices=(1, 2, 3, 4),
                    help='evaluate the network pruned to head L (needs a checkpoint trained with --deep_supervision true)')
    ap.add_argument('--per_head', default=False, type=str2bool,
                    help='also print IoU / Dice / Acc / loss of every head (needs --deep_supervision true)')
    ap.add_argument('--ema', default=False, type=str2bool,
                    help='evaluate model_ema.pth, the weight EMA of a run trained with --ema_decay, instead of model.pth')
    ap.add_argument('--img_ext', default=None, help='image file extension of a folder dataset (default: the training run\'s)')
    ap.add_argument('--mask_ext', default=None, help='mask file extension of a folder dataset (default: the training run\'s)')
    ap.add_argument('--full_res', default=False, type=str2bool,
                    help='predict every validation image at its own size from overlapping input_h x input_w tiles (a folder dataset or a '
                         '--source_size run): masks and metrics at the sources\' resolution')
    ap.add_argument('--tile_overlap', default=None, type=int,
                    help='overlap of neighbouring tiles under --full_res, 0 .. min(input_h, input_w) / 2 (default: a quarter of the smaller side)')
    ap.add_argument('--tta', default='none', choices=('none', 'flips', 'd4'),
                    help='test-time augmentation: merge the predictions of the 4 flips / the 8 rotations and flips (d4: input_h == input_w)')
    ap.add_argument('--tta_merge', default='logit', choices=('logit', 'prob'),
                    help='merge the views as the mean logit, or as the mean probability taken back to a logit')
    args = ap.parse_args()
    if args.full_res and args.tta != 'none':
        print('error: --full_res true does not combine with --tta %s: test-time augmentation of tiled inference is not implemented' % args.tta)
        sys.exit(2)
    with open('models/%s/config.yml' % args.name) as f:
        config = yaml.load(f, Loader=yaml.FullLoader)
    print('-' * 20)
    for k in config:
        print('%s: %s' % (k, str(config[k])))
    print('-' * 20)
    if (args.depth is not None or args.per_head) and not (config['deep_supervision'] and config['arch'] == 'NestedUNet'):
        print('error: --depth / --per_head need a NestedUNet checkpoint trained with --deep_supervision true '
              '(models/%s: arch %s, deep_supervision %s)' % (args.name, config['arch'], config['deep_supervision']))
        sys.exit(2)
    model = archs.__dict__[config['arch']](config['num_classes'], config['input_channels'], config['deep_supervision'],
                                           dtype=config.get('dtype', 'fp32'))
    ckpt = 'models/%s/%s' % (config['name'], 'model_ema.pth' if args.ema else 'model.pth')
    if args.ema and not os.path.exists(ckpt):
        print('error: --ema true needs %s: train with --ema_decay D (this run: ema_decay %s)' % (ckpt, config.get('ema_decay', 0.0)))
        sys.exit(2)
    model.load_state_dict(torch.load(ckpt, map_location='cpu'))
    model = model.cuda()
    model.eval()
    for k in ('img_ext', 'mask_ext'):
        if getattr(args, k) is not None:
            config[k] = getattr(args, k)
    ragged = config.get('dataset', 'synthetic_blobs') != 'synthetic_blobs' or config.get('source_size') is not None
    if args.full_res:
        if not ragged or args.per_head:
            print('error: --full_res true needs sources at their own sizes (a folder dataset, or a run trained with --source_size LO,HI) '
                  'and does not combine with --per_head')
            sys.exit(2)
        from train import ragged_sets
        config.setdefault('img_ext', '.png')
        config.setdefault('mask_ext', '.png')
        return full_res(args, config, model, ragged_sets(config)[1])
    if ragged:
        # samples at their own sizes (the folder's validation split of val.py:53-56, or the synthetic blobs of --source_size):
        # Resize + Normalize on the device, floats into the EvalStep
        from train import ragged_sets, ragged_to_floats
        config.setdefault('img_ext', '.png')
        config.setdefault('mask_ext', '.png')
        x, t = ragged_to_floats(ragged_sets(config)[1], config['input_h'], config['input_w'], config['batch_size'])
    else:
        img, msk = nunet_amd.synth.synth_split(config['val_size'], config['input_h'], config['input_w'],
                                               config['input_channels'], config['num_classes'], seed=2000)
        x, t = torch.from_numpy(img), torch.from_numpy(msk)
    for c in range(config['num_classes']):
        os.makedirs(os.path.join('outputs', config['name'], str(c)), exist_ok=True)
    bs = config['batch_size']
    loss = config.get('loss', 'BCEDiceLoss')
    if loss == 'LovaszHingeLoss' and config['num_classes'] != 1:
        loss = 'BCEDiceLoss'                                             # (the metrics do not depend on it)
    # the validation step of train.py: forward, IoU / Dice / accuracy of the last head (val.py:92-93) and the meters on the device
    shape = (min(bs, x.size(0)), config['input_channels'], config['input_h'], config['input_w'])
    tta = None if args.tta == 'none' else args.tta
    if tta == 'd4' and config['input_h'] != config['input_w']:
        print('error: --tta d4 rotates by 90 degrees: input_h %d must equal input_w %d (use --tta flips)' % (config['input_h'], config['input_w']))
        sys.exit(2)
    ev = EvalStep(model, shape, loss=loss, depth=args.depth, tta=tta, tta_merge=args.tta_merge)
    # (the per-head table comes from the whole network: a pass of its own beside the pruned one)
    ev_heads = EvalStep(model, shape, loss=loss, per_head=True, tta=tta, tta_merge=args.tta_merge) if args.per_head else None
    bs = ev.n
    with torch.no_grad():
        ev.begin()
        for k in range(0, x.size(0), bs):
            ev.step(x[k:k + bs].cuda(), t[k:k + bs].cuda())
            out = ev.last_logits
            if not args.no_images:
                from PIL import Image
                masks = sigmoid_masks_u8(out).cpu().numpy()              # uint8 on the device: 4x fewer D2H bytes
                for i in range(masks.shape[0]):
                    for c in range(config['num_classes']):
                        Image.fromarray(masks[i, c]).save(
                            os.path.join('outputs', config['name'], str(c), 'val_%04d.jpg' % (k + i)))
    r = ev.result()
    if args.depth is not None:
        print('depth: %d' % args.depth)
    if args.ema:
        print('weights: EMA (model_ema.pth)')
    if tta is not None:
        print('tta: %s (%d views, merged as %s)' % (tta, len(ev.tta), args.tta_merge))
    print('IoU: %.4f' % r['iou'])
    print('Dice: %.4f' % r['dice'])
    print('Acc: %.4f' % r['acc'])
    if config['num_classes'] > 1:
        names = list(r['per_class'])
        print('class ' + ' '.join('%11s' % nm for nm in names))
        for c in range(config['num_classes']):
            print('%5d ' % c + ' '.join('%11.4f' % r['per_class'][nm][0][c] for nm in names))
        print('micro ' + ' '.join('%11.4f' % r['per_class'][nm][1] for nm in names))
    if ev_heads is not None:
        with torch.no_grad():
            rh = ev_heads.evaluate(x.cuda(), t.cuda())
        print('head %9s %9s %9s %9s' % ('IoU', 'Dice', 'Acc', 'loss'))
        for k, h in enumerate(rh['heads']):
            print('%4d %9.4f %9.4f %9.4f %9.4f' % (k + 1, h['iou'], h['dice'], h['acc'], h['loss']))


if __name__ == '__main__':
    main()
