"""Oracle and case tables of the device-side input pipeline (nunet_preprocess_u8, nunet_preprocess_u8_color,
nunet_color_aug_u8, nunet_plan_stage_u8(_color); include/nunet.h), numpy only. tests/test_input_pipeline_cpu.py proves the
tables can tell a broken index map from the right one; tests/test_input_pipeline_gpu.py holds the kernels against the oracle.

Geometry. aug[n] = rot90 count (bits 0-1, counter-clockwise like np.rot90) | hflip (bit 2) | vflip (bit 3). ref_geometry
states it FORWARD with library calls. The kernels compute the inverse (destination pixel -> source pixel); restate() is a
numpy copy of that inverse map, kept apart and used only to show that the listed mutations of it are detected.

Tagged images. Every byte says where it came from, so a wrong pixel can be decoded into the (n, y, x) it was fetched from.
The kernels compute ((u/255 - mean)/std) * post_scale; with mean = std = NULL and post_scale = 1 (the mask configuration)
that is fp32(u/255), rounded to nearest-even into the storage type by the staging kernel: not the integer u, but 256
DISTINCT values in fp32, fp16 and - narrowly, 2^-8 against 1/255 - bf16 (quotient_table, checked in the CPU test). So the
exact comparison is made on bytes: decode_bytes maps every output value back to the byte whose quotient it is bit for bit
(-1: no byte's), and the decoded image must equal the forward oracle of the source bytes.

Values. ref_values evaluates the expression in fp64 on the fp32 mean / std / post_scale the kernel receives and returns the
per-element bound
    B = 2^-24 * (|u/255| / std * post_scale + 3 * |ref|):
the rounding of u/255 carried through the subtraction and the division, then one rounding each of the subtraction, the
division and the multiplication (each at most 2^-24 relative to its own result, which is |ref| up to factors 1 + O(2^-24);
the subtraction's result, |u/255 - mean|, divided by std and scaled is |ref| again). f32_values is the same expression with
one np.float32 ufunc per operation: what a kernel that rounds every operation to fp32 must produce bit for bit, and what
the 16-bit staging rounds to nearest-even into its storage type."""
import numpy as np

MEAN = (0.485, 0.456, 0.406)      # albumentations Normalize() defaults, as dataset.MEAN / STD
STD = (0.229, 0.224, 0.225)

ALL_CODES = list(range(16))
EVEN_CODES = [c for c in range(16) if not c & 1]

# (H, W): nunet_preprocess_u8 takes any shape, a plan multiples of 16
U8_SHAPES = [(1, 1), (1, 6), (6, 1), (3, 7), (7, 3), (5, 5), (16, 16), (33, 31)]
PLAN_SHAPES = [(16, 16), (32, 32), (16, 48), (48, 16)]
CHANNELS = [1, 2, 3, 4, 8]
PLAN_CHANNELS = [1, 3, 4, 32]
# The one-pixel-per-thread kernels launch at most 4096 blocks x 256 threads; a batch past that makes their threads loop.
GRID_CAP_PIXELS = 4096 * 256
# (N, H, W) just over the cap: "plan" for the staging entries (multiples of 16: the pixel count is a multiple of 256), "free"
# for the entries that take any shape (5 * 460 * 457 = 1,051,100 = 4105 * 256 + 220: the second trip ends inside a block)
LARGE_SHAPES = {"plan": (5, 464, 464), "free": (5, 460, 457)}
LARGE_CODES = [2 | 4, 0, 8, 2, 2 | 4 | 8]      # per sample; even rot90 counts serve both shapes


def codes_for(h, w):
    """one batch per shape: square - N = 16, sample n gets code n; non-square - the 8 codes with an even rot90 count"""
    return list(ALL_CODES) if h == w else list(EVEN_CODES)


# -- geometry ------------------------------------------------------------------------------------------------------------------
def ref_geometry(src_hwc, code):
    out = np.rot90(src_hwc, k=code & 3, axes=(0, 1))
    if code & 4:
        out = out[:, ::-1]
    if code & 8:
        out = out[::-1]
    return np.ascontiguousarray(out)


def ref_batch(u, codes):
    """[N,H,W,C] -> [N,H',W',C], every sample through its own code (None: no augmentation)"""
    if codes is None:
        return u.copy()
    return np.stack([ref_geometry(u[n], int(codes[n])) for n in range(u.shape[0])])


MUTATIONS = ("swap_flips", "clockwise", "flips_after", "w_for_h", "aug0", "code_shr1")


def restate_batch(u, codes, mutate=None):
    """The kernels' inverse index map on a whole batch, with their flat source address ((n*H + ry)*W + rx): a mutated map
    may leave the sample or the batch, as the kernel's read would; such an address is wrapped into the batch here (any
    value would do: the pixel is wrong)."""
    assert mutate is None or mutate in MUTATIONS, mutate
    N, H, W, C = u.shape
    flat = u.reshape(N * H * W, C)
    out = np.empty_like(u)
    y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    for n in range(N):
        a = int(codes[0] if mutate == "aug0" else codes[n])
        if mutate == "code_shr1":
            a >>= 1
        vbit, hbit = (4, 8) if mutate == "swap_flips" else (8, 4)
        k = a & 3
        if mutate == "clockwise":
            k = (4 - k) & 3
        HH = W if mutate == "w_for_h" else H

        def flips(sy, sx):
            if a & vbit:
                sy = H - 1 - sy
            if a & hbit:
                sx = W - 1 - sx
            return sy, sx

        def rot(sy, sx):
            if k == 1:
                return sx, W - 1 - sy
            if k == 2:
                return HH - 1 - sy, W - 1 - sx
            if k == 3:
                return HH - 1 - sx, sy
            return sy, sx

        if mutate == "flips_after":
            ry, rx = flips(*rot(y, x))
        else:
            ry, rx = rot(*flips(y, x))
        idx = (n * H + ry) * W + rx
        out[n] = flat[np.mod(idx, N * H * W)]
    return out


def restate(src_hwc, code, mutate=None):
    """one sample through one code (a batch of one: 'aug0' cannot show here)"""
    return restate_batch(src_hwc[None], [code], mutate)[0]


# -- tagged images -------------------------------------------------------------------------------------------------------------
def tagged(n, h, w, c, codes):
    """uint8 [n,h,w,c], h, w <= 256: channel 0 = y, channel 1 = x, channel 2 = 16 * (sample % 16) + code, then (y + x + c) & 255"""
    assert h <= 256 and w <= 256 and len(codes) == n
    u = np.zeros((n, h, w, c), np.uint8)
    y, x = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    for i in range(n):
        for ch in range(c):
            u[i, :, :, ch] = (y, x, 16 * (i % 16) + (int(codes[i]) & 15))[ch] if ch < 3 else (y + x + ch) & 255
    return u


def tagged_large(n, h, w, c=3):
    """uint8 [n,h,w,c], n <= 8 and h, w <= 512, for the capped-grid cases: channel 0 = y & 255, channel 1 = x & 255, channel 2
    = sample | (y >> 8) << 3 | (x >> 8) << 4 - the high bits ride with the sample number, so the first three channels are
    injective over the WHOLE batch and a pixel fetched through a wrapped or truncated index decodes to where it came from."""
    assert n <= 8 and h <= 512 and w <= 512 and c >= 3
    u = np.zeros((n, h, w, c), np.uint8)
    y, x = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    for i in range(n):
        u[i, :, :, 0] = y & 255
        u[i, :, :, 1] = x & 255
        u[i, :, :, 2] = i | (y >> 8) << 3 | (x >> 8) << 4
        for ch in range(3, c):
            u[i, :, :, ch] = (y + x + ch) & 255
    return u


def decode_large(px):
    """(n, y, x) a tagged_large pixel (its first three channels, as integers) came from"""
    y0, x0, t = int(px[0]), int(px[1]), int(px[2])
    return t & 7, y0 | ((t >> 3) & 1) << 8, x0 | ((t >> 4) & 1) << 8


def triples_injective(u):
    """no two pixels of the batch carry the same (channel 0, 1, 2) triple"""
    assert u.shape[-1] >= 3
    key = u[..., 0].astype(np.int64) << 16 | u[..., 1].astype(np.int64) << 8 | u[..., 2].astype(np.int64)
    return np.unique(key).size == key.size


def first_mismatch(got, exp, decode=None):
    """'' when equal; else a message that decodes the first wrong pixel of two [N,H,W,C] integer-valued arrays"""
    if np.array_equal(got, exp):
        return ""
    bad = np.argwhere((got != exp).any(axis=-1))
    n, y, x = (int(v) for v in bad[0])
    g, e = got[n, y, x], exp[n, y, x]

    def where(px):
        if px.shape[0] < 3 or np.any(px[:3] < 0):
            return "undecodable %s" % (px[:3],)
        if decode is not None:
            return "source (n, y, x) = %s" % (decode(px),)
        return "source y = %d, x = %d, sample %% 16 = %d, code %d" % (px[0], px[1], int(px[2]) >> 4, int(px[2]) & 15)
    return ("%d of %d pixels wrong; first at destination (n, y, x) = (%d, %d, %d): found %s [%s], expected %s [%s]"
            % (len(bad), got.shape[0] * got.shape[1] * got.shape[2], n, y, x, g, where(g), e, where(e)))


# -- values --------------------------------------------------------------------------------------------------------------------
def _f32(a, c):
    return None if a is None else np.resize(np.asarray(a, np.float32), c)


def ref_values(u, mean, std, post_scale):
    """fp64 of ((u/255 - mean)/std) * post_scale on the fp32 parameters, channel-last u; returns (ref, B)"""
    c = u.shape[-1]
    m = np.zeros(c) if mean is None else _f32(mean, c).astype(np.float64)
    s = np.ones(c) if std is None else _f32(std, c).astype(np.float64)
    ps = np.float64(np.float32(post_scale))
    q = u.astype(np.float64) / 255.0
    ref = ((q - m) / s) * ps
    B = 2.0 ** -24 * (np.abs(q) / s * ps + 3.0 * np.abs(ref))
    return ref, B


def f32_values(u, mean, std, post_scale):
    """the same expression, one np.float32 ufunc per operation (no fused multiply-add, no reciprocal)"""
    c = u.shape[-1]
    m = np.zeros(c, np.float32) if mean is None else _f32(mean, c)
    s = np.ones(c, np.float32) if std is None else _f32(std, c)
    q = np.divide(u.astype(np.float32), np.float32(255))
    out = np.multiply(np.divide(np.subtract(q, m), s), np.float32(post_scale))
    assert out.dtype == np.float32
    return out


def round_bf16_bits(f):
    """fp32 -> the uint16 bit patterns of bf16, round to nearest even (finite inputs)"""
    b = np.ascontiguousarray(f, np.float32).view(np.uint32).astype(np.uint64)
    return ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint16)


def round_fp16_bits(f):
    return np.ascontiguousarray(f, np.float32).astype(np.float16).view(np.uint16)      # numpy converts to nearest even


def bf16_bits_to_f32(bits):
    return (bits.astype(np.uint32) << 16).view(np.float32)


def quotient_table(kind):
    """fp32 values of the 256 outputs of the NULL mean / std, post_scale = 1 configuration in storage type `kind`, ascending"""
    q = f32_values(np.arange(256, dtype=np.uint8).reshape(256, 1), None, None, 1.0).ravel()
    if kind == "bf16":
        q = bf16_bits_to_f32(round_bf16_bits(q))
    elif kind == "fp16":
        q = round_fp16_bits(q).view(np.float16).astype(np.float32)
    else:
        assert kind == "fp32", kind
    return q


def decode_bytes(v, kind):
    """float32 array of outputs -> int16 array of the bytes they are the exact quotients of; -1 where a value is none of the 256"""
    t = quotient_table(kind)
    v = np.asarray(v, np.float32)
    i = np.clip(np.searchsorted(t, v), 0, 255)
    return np.where(t[i] == v, i, -1).astype(np.int16)


def all_bytes_image(c, h=16, w=16):
    """[1,h,w,c] holding every byte 0..255 in every channel (channel ch is the ramp rotated by 37 * ch)"""
    assert h * w >= 256
    ramp = np.arange(h * w, dtype=np.int64)
    return np.stack([((ramp + 37 * ch) & 255).astype(np.uint8).reshape(h, w) for ch in range(c)], axis=-1)[None]
