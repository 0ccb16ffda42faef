"""Device-side counterpart of the reference sample pipeline (dataset.py:66-74: Normalize -> /255 ->
HWC->CHW; trains.py:258-264: RandomRotate90, Flip, OneOf([HueSaturationValue, RandomBrightness, RandomContrast]))
for uint8 batches already decoded on the host. Only uint8 crosses PCIe (4x fewer bytes than the reference's float
tensors). The colour ops are modelled on albumentations / OpenCV (input pipeline), not bit-identical to them."""
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
