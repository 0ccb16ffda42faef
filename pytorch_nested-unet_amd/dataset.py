"""Device-side counterpart of the reference sample pipeline (dataset.py:66-74: Normalize -> /255 ->
HWC->CHW; trains.py:258-264: RandomRotate90, Flip, OneOf([HueSaturationValue, RandomBrightness, RandomContrast]))
for uint8 batches already decoded on the host. Only uint8 crosses PCIe (4x fewer bytes than the reference's float
tensors). The colour ops are modelled on albumentations / OpenCV (input pipeline), not bit-identical to them.
Resize(input_h, input_w) (trains.py:265, 269) runs on the device too: samples of differing sizes travel as one byte pool with a
descriptor per sample (pack_ragged; FolderDataset reads the reference's folder layout into that form)."""
import numpy as np
import torch

from . import _lib as L

MEAN = (0.485, 0.456, 0.406)      # albumentations Normalize() defaults (trains.py:266)
STD = (0.229, 0.224, 0.225)


def _check_color(color, n, c):
    L.require_gpu_tensor(color, torch.int32, "color")
    if tuple(color.shape) != (n, L.COLOR_WORDS):
        raise L.NunetError("color must be int32 [%d,%d] (draw_color_augmentation), got %s" % (n, L.COLOR_WORDS, tuple(color.shape)))
    if c != 3:
        raise L.NunetError("the colour ops are defined on RGB images: C=%d must be 3" % c)


def _check_aug(aug, n, h, w):
    """The kernels read aug[i] for every sample i < n and, for an odd rot90 count, source row = destination column: refuse
    anything but int32 [n] on the device, and an odd count on non-square images, before a launch."""
    L.require_gpu_tensor(aug, torch.int32, "aug")
    if tuple(aug.shape) != (n,):
        raise L.NunetError("aug must be int32 [%d], one code per sample (draw_augmentation), got %s" % (n, tuple(aug.shape)))
    if h != w and bool((aug & 1).any()):
        raise L.NunetError("rot90 by an odd count needs square images")


def preprocess_images(u8_nhwc, aug=None, mean=MEAN, std=STD, color=None):
    """uint8 [N,H,W,C] (device) -> float32 [N,C,H,W]: ((u/255 - mean)/std)/255, optional per-sample
    geometric augmentation codes (int32 [N]: rot90 count | hflip<<2 | vflip<<3) and colour codes (int32 [N,4],
    draw_color_augmentation; C == 3), applied to the source pixel in the same launch."""
    L.require_gpu_tensor(u8_nhwc, torch.uint8, "images")
    n, h, w, c = u8_nhwc.shape
    dev = u8_nhwc.device
    m = torch.tensor(np.resize(np.asarray(mean, np.float32), c), device=dev)
    s = torch.tensor(np.resize(np.asarray(std, np.float32), c), device=dev)
    out = torch.empty((n, c, h, w), dtype=torch.float32, device=dev)
    if aug is not None:
        _check_aug(aug, n, h, w)
    if color is not None:
        _check_color(color, n, c)
        L.check(L.lib().nunet_preprocess_u8_color(L.ptr(u8_nhwc), n, h, w, c, L.ptr(m), L.ptr(s), L.ptr(aug), L.ptr(color), 1.0 / 255.0,
                                                  L.ptr(out), L.stream()), "nunet_preprocess_u8_color")
        return out
    L.check(L.lib().nunet_preprocess_u8(L.ptr(u8_nhwc), n, h, w, c, L.ptr(m), L.ptr(s), L.ptr(aug), 1.0 / 255.0,
                                        L.ptr(out), L.stream()), "nunet_preprocess_u8")
    return out


def color_augment(u8_nhwc, color):
    """uint8 RGB [N,H,W,3] (device) -> uint8 [N,H,W,3]: sample n through the colour op color[n] (int32 [N,4],
    draw_color_augmentation)."""
    L.require_gpu_tensor(u8_nhwc, torch.uint8, "images")
    n, h, w, c = u8_nhwc.shape
    _check_color(color, n, c)
    out = torch.empty_like(u8_nhwc)
    L.check(L.lib().nunet_color_aug_u8(L.ptr(u8_nhwc), n, h, w, c, L.ptr(color), L.ptr(out), L.stream()), "nunet_color_aug_u8")
    return out


def preprocess_masks(u8_nhwc, aug=None):
    """uint8 {0,255} [N,H,W,K] -> float32 [N,K,H,W] in {0,1} (dataset.py:73), same augmentation codes."""
    L.require_gpu_tensor(u8_nhwc, torch.uint8, "masks")
    n, h, w, c = u8_nhwc.shape
    if aug is not None:
        _check_aug(aug, n, h, w)
    out = torch.empty((n, c, h, w), dtype=torch.float32, device=u8_nhwc.device)
    L.check(L.lib().nunet_preprocess_u8(L.ptr(u8_nhwc), n, h, w, c, None, None, L.ptr(aug), 1.0, L.ptr(out), L.stream()),
            "nunet_preprocess_u8")
    return out


def draw_augmentation(n, generator=None, device="cuda"):
    """Per-sample codes for RandomRotate90() + Flip() (trains.py:258-259), drawn on the host."""
    k = torch.randint(0, 4, (n,), generator=generator)
    f = torch.randint(0, 4, (n,), generator=generator)       # bit0 hflip, bit1 vflip
    return (k | (f << 2)).to(torch.int32).to(device)


HSV_SHIFT_LIMITS = (20.0, 30.0, 20.0)      # albumentations HueSaturationValue() defaults: hue, saturation, value
BRIGHTNESS_LIMIT = CONTRAST_LIMIT = 0.2    # RandomBrightness() / RandomContrast() defaults


def color_codes(ops, params):
    """int32 [n,4] colour codes (nunet_color_aug: op, then three fp32 parameters bit-cast) from n ops and an [n,3] array."""
    ops = np.asarray(ops, np.int32).reshape(-1)
    words = np.zeros((ops.shape[0], L.COLOR_WORDS), np.int32)
    words[:, 0] = ops
    words[:, 1:] = np.ascontiguousarray(np.asarray(params, np.float32).reshape(-1, 3)).view(np.int32)
    return torch.from_numpy(words)


def draw_color_augmentation(n, generator=None, device="cuda"):
    """Per-sample codes for OneOf([HueSaturationValue(), RandomBrightness(), RandomContrast()], p=1) (trains.py:260-264),
    drawn on the host: the op uniform over the three (OneOf with equal p picks one member and forces it), HSV shifts
    U(-20,20), U(-30,30), U(-20,20), brightness p0 = float(beta * 255) with beta U(-0.2,0.2), contrast p0 = alpha =
    1 + U(-0.2,0.2). int32 [n,4]: the op, then the three fp32 parameters bit-cast (unused ones 0)."""
    op = torch.randint(1, 4, (n,), generator=generator).numpy()
    u = torch.rand((n, 3), generator=generator, dtype=torch.float64).numpy() * 2.0 - 1.0     # U(-1,1), in double
    par = np.zeros((n, 3), np.float64)
    hsv, bri, con = op == L.COLOR_HSV, op == L.COLOR_BRIGHTNESS, op == L.COLOR_CONTRAST
    par[hsv] = u[hsv] * np.asarray(HSV_SHIFT_LIMITS)
    par[bri, 0] = (u[bri, 0] * BRIGHTNESS_LIMIT) * 255.0
    par[con, 0] = 1.0 + u[con, 0] * CONTRAST_LIMIT
    return color_codes(op, par.astype(np.float32)).to(device)


# -- Resize on ragged sources --------------------------------------------------------------------------------------------------
def sample_descriptors(offsets, heights, widths):
    """int32 [n,4] descriptors (nunet_u8_sample: the int64 byte offset as two little-endian words, then H and W)."""
    d = np.zeros((len(offsets), L.SAMPLE_WORDS), np.int32)
    if len(offsets):
        d.view(np.int64)[:, 0] = np.asarray(offsets, np.int64)
        d[:, 2] = np.asarray(heights, np.int32)
        d[:, 3] = np.asarray(widths, np.int32)
    return torch.from_numpy(d)


def check_descriptors(desc, pool_bytes, channels, n=None):
    """The kernels trust nothing in a descriptor (a bad one yields zeros), but a bad one is a bug of the caller: refuse on the
    host, before any launch, an array that is not int32 [n,4], an extent outside 1 .. 16384 and a sample outside the pool."""
    if isinstance(desc, torch.Tensor):
        if desc.is_cuda:
            raise L.NunetError("descriptors are validated on the host: pass the host tensor pack_ragged returned")
        desc = desc.numpy()
    desc = np.asarray(desc)
    if desc.dtype != np.int32 or desc.ndim != 2 or desc.shape[1] != L.SAMPLE_WORDS or (n is not None and desc.shape[0] != n):
        raise L.NunetError("descriptors must be int32 [%s,%d] (pack_ragged), got %s %s"
                           % ("n" if n is None else n, L.SAMPLE_WORDS, desc.dtype, tuple(desc.shape)))
    off = np.ascontiguousarray(desc).view(np.int64)[:, 0]
    h, w = desc[:, 2].astype(np.int64), desc[:, 3].astype(np.int64)
    for i in range(desc.shape[0]):
        if not (1 <= h[i] <= L.RESIZE_MAX_EXTENT and 1 <= w[i] <= L.RESIZE_MAX_EXTENT):
            raise L.NunetError("sample %d: %d x %d: extents are 1 .. %d" % (i, h[i], w[i], L.RESIZE_MAX_EXTENT))
        if off[i] < 0 or off[i] + h[i] * w[i] * channels > pool_bytes:
            raise L.NunetError("sample %d: bytes %d .. %d lie outside the pool of %d bytes"
                               % (i, off[i], off[i] + h[i] * w[i] * channels, pool_bytes))


def pack_ragged(samples):
    """A list of decoded samples, each uint8 [H,W,C] (numpy or host tensor) at its own size and all with the same C, ->
    (pool, descriptors) on the host: the tight concatenation of their bytes as a uint8 tensor and one nunet_u8_sample per
    sample as int32 [n,4]. Raises NunetError for an empty list, a wrong dtype or rank, differing channel counts, an extent
    over 16384 - before anything reaches the device."""
    if len(samples) == 0:
        raise L.NunetError("pack_ragged: no samples")
    arrs = []
    for i, s in enumerate(samples):
        a = s.numpy() if isinstance(s, torch.Tensor) else np.asarray(s)
        if a.dtype != np.uint8 or a.ndim != 3:
            raise L.NunetError("pack_ragged: sample %d must be uint8 [H,W,C], got %s %s" % (i, a.dtype, tuple(a.shape)))
        if a.size == 0:
            raise L.NunetError("pack_ragged: sample %d is empty: %s" % (i, tuple(a.shape)))
        if arrs and a.shape[2] != arrs[0].shape[2]:
            raise L.NunetError("pack_ragged: sample %d has %d channels, the first has %d" % (i, a.shape[2], arrs[0].shape[2]))
        arrs.append(np.ascontiguousarray(a))
    sizes = np.asarray([a.size for a in arrs], np.int64)
    desc = sample_descriptors(np.concatenate([[0], np.cumsum(sizes)[:-1]]), [a.shape[0] for a in arrs], [a.shape[1] for a in arrs])
    pool = torch.from_numpy(np.concatenate([a.reshape(-1) for a in arrs]))
    check_descriptors(desc, pool.numel(), arrs[0].shape[2])
    return pool, desc


def _ragged_to_device(pool, desc, channels, device):
    """validated host pool + descriptors -> device tensors (a device pool is taken as it is; the descriptors stay host-checked)"""
    if pool.dtype != torch.uint8 or pool.dim() != 1:
        raise L.NunetError("pool must be a flat uint8 tensor (pack_ragged), got %s %s" % (pool.dtype, tuple(pool.shape)))
    check_descriptors(desc, pool.numel(), channels)
    return pool.to(device), desc.to(device)


def resize_u8(pool, desc, channels, size, mode=L.RESIZE_LINEAR, aug=None, color=None, device="cuda"):
    """nunet_resize_u8: ragged uint8 sources (pack_ragged's host tensors) -> uint8 [N,Hd,Wd,C] on the device, LINEAR or NEAREST,
    behind the per-sample augmentation and (LINEAR, C == 3) colour codes. An odd rot90 count needs no square source."""
    p, d = _ragged_to_device(pool, desc, channels, device)
    n, (hd, wd) = d.shape[0], size
    if aug is not None:
        _check_aug(aug, n, 1, 1)
    if color is not None:
        _check_color(color, n, channels)
    out = torch.empty((n, hd, wd, channels), dtype=torch.uint8, device=p.device)
    L.check(L.lib().nunet_resize_u8(L.ptr(p), p.numel(), L.ptr(d), n, channels, hd, wd, mode, L.ptr(aug), L.ptr(color), L.ptr(out), L.stream()),
            "nunet_resize_u8")
    return out


def resize_images(pool, desc, size, aug=None, mean=MEAN, std=STD, color=None, channels=3, device="cuda"):
    """Resize(input_h, input_w) + Normalize + /255 + HWC->CHW of ragged uint8 images (the reference's val transform,
    trains.py:269-272, dataset.py:66-74) -> float32 [N,C,Hd,Wd]: nunet_resize_u8 (bilinear), then preprocess_images."""
    return preprocess_images(resize_u8(pool, desc, channels, size, L.RESIZE_LINEAR, aug, color, device), None, mean, std)


def resize_masks(pool, desc, size, aug=None, channels=1, device="cuda"):
    """Ragged uint8 {0,255} masks -> float32 [N,K,Hd,Wd] in {0,1}: nearest-neighbour resize and the mask scaling in one launch
    (nunet_preprocess_u8_resize)."""
    p, d = _ragged_to_device(pool, desc, channels, device)
    n, (hd, wd) = d.shape[0], size
    if aug is not None:
        _check_aug(aug, n, 1, 1)
    out = torch.empty((n, channels, hd, wd), dtype=torch.float32, device=p.device)
    L.check(L.lib().nunet_preprocess_u8_resize(L.ptr(p), p.numel(), L.ptr(d), n, channels, hd, wd, None, None, L.ptr(aug), 1.0, L.ptr(out),
                                               L.stream()), "nunet_preprocess_u8_resize")
    return out


def train_val_split(ids, test_size=0.2, seed=41):
    """sklearn.model_selection.train_test_split(ids, test_size=0.2, random_state=41) of the reference (trains.py:255, val.py:56)
    without the dependency: ShuffleSplit's rule - one permutation of a RandomState(seed), the first ceil(test_size * n) indices
    are the validation set, the rest the training set."""
    n = len(ids)
    n_test = int(np.ceil(test_size * n))
    if n_test < 1 or n - n_test < 1:
        raise L.NunetError("a split of %d samples with test_size %g leaves an empty side" % (n, test_size))
    perm = np.random.RandomState(seed).permutation(n)
    return [ids[i] for i in perm[n_test:]], [ids[i] for i in perm[:n_test]]


class FolderDataset:
    """The reference's on-disk layout (dataset.py:20-42, 55-64), read with PIL: inputs/<name>/images/<id><img_ext> and
    inputs/<name>/masks/<class>/<id><mask_ext>, one grey-scale mask per class. A sample is (image uint8 [H,W,3], mask uint8
    [H,W,num_classes]) at the file's own size; the device resizes (TrainStep(resize=True), resize_images / resize_masks).
    Channel order: the reference reads with cv2.imread and never converts, so its network sees BGR; this class reverses PIL's
    RGB to keep that order (a checkpoint of the reference then sees what it was trained on). The ids are sorted (glob order is
    the file system's) and split as the reference splits them: train_test_split(test_size=0.2, random_state=41)."""

    def __init__(self, name, img_ext=".png", mask_ext=".png", num_classes=1, root="inputs", split=None):
        import glob
        import os
        self.img_dir = os.path.join(root, name, "images")
        self.mask_dir = os.path.join(root, name, "masks")
        self.img_ext, self.mask_ext, self.num_classes = img_ext, mask_ext, num_classes
        ids = sorted(os.path.splitext(os.path.basename(p))[0] for p in glob.glob(os.path.join(self.img_dir, "*" + img_ext)))
        if not ids:
            raise L.NunetError("FolderDataset: no %s files in %s" % (img_ext, self.img_dir))
        if split not in (None, "train", "val"):
            raise L.NunetError("FolderDataset: split %r is not None, 'train' or 'val'" % (split,))
        if split is not None:
            tr, va = train_val_split(ids)
            ids = tr if split == "train" else va
        self.ids = ids

    def __len__(self):
        return len(self.ids)

    def __getitem__(self, idx):
        import os
        from PIL import Image
        i = self.ids[idx]
        img = np.asarray(Image.open(os.path.join(self.img_dir, i + self.img_ext)).convert("RGB"))[:, :, ::-1]
        mask = [np.asarray(Image.open(os.path.join(self.mask_dir, str(c), i + self.mask_ext)).convert("L"))
                for c in range(self.num_classes)]
        return np.ascontiguousarray(img), np.ascontiguousarray(np.stack(mask, axis=-1))

    def batch(self, indices):
        """(image pool, image descriptors, mask pool, mask descriptors) of the samples `indices`, on the host (pack_ragged)."""
        pairs = [self[i] for i in indices]
        return pack_ragged([p[0] for p in pairs]) + pack_ragged([p[1] for p in pairs])
