"""The numpy oracle of the device-side Resize (tests/resize_cases.py) held to the properties its definition promises, the
destination-driven restatement held to the forward oracle, named mutations shown to be detected by the case tables, and the
host side of the feature: pack_ragged's refusals and FolderDataset. No GPU."""
import os

import numpy as np
import pytest

import nunet_amd  # noqa: F401
from nunet_amd import _lib as L
from nunet_amd import dataset as D
import color_cases as CC
import pipeline_cases as PC
import resize_cases as RC

PAIRS = [(s, d) for s in RC.SRC_SHAPES for d in RC.DST_SHAPES] + [RC.UPSCALE]


def _src(shape, c=3, seed=0):
    return RC.sources([shape], c, seed + shape[0] * 1000 + shape[1])[0]


# -- 1. properties of the definition -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", RC.SRC_SHAPES + RC.DST_SHAPES + [(464, 464)])
def test_equal_extents_reproduce_the_source(shape):
    src = _src(shape)
    assert np.array_equal(RC.bilinear(src, *shape), src)
    assert np.array_equal(RC.nearest(src, *shape), src)
    s0, s1, a0, a1 = RC.taps(shape[0], shape[0])
    assert np.array_equal(s0, np.arange(shape[0])) and not a1.any() and (a0 == 2048).all()


@pytest.mark.parametrize("src_shape,dst_shape", PAIRS)
def test_constant_image_stays_constant(src_shape, dst_shape):
    for v in (0, 1, 127, 128, 254, 255):
        out = RC.bilinear(np.full(src_shape + (3,), v, np.uint8), *dst_shape)
        assert (out == v).all(), (v, np.unique(out))


@pytest.mark.parametrize("dst_shape", RC.DST_SHAPES)
def test_exact_halving_is_the_rounded_2x2_mean(dst_shape):
    h, w = dst_shape
    src = _src((2 * h, 2 * w))
    s = src.astype(np.int64)
    mean = (s[0::2, 0::2] + s[0::2, 1::2] + s[1::2, 0::2] + s[1::2, 1::2] + 2) >> 2
    assert np.array_equal(RC.bilinear(src, h, w), mean.astype(np.uint8))


@pytest.mark.parametrize("src_shape,dst_shape", PAIRS)
def test_less_than_one_byte_from_fp64_bilinear(src_shape, dst_shape):
    src = _src(src_shape)
    d = np.abs(RC.bilinear(src, *dst_shape).astype(np.float64) - RC.bilinear_f64(src, *dst_shape))
    print("%s -> %s: max distance from the fp64 bilinear %.4f byte" % (src_shape, dst_shape, d.max()))
    assert d.max() < 1.0


@pytest.mark.parametrize("src_shape,dst_shape", PAIRS)
def test_taps_stay_inside_and_weights_sum(src_shape, dst_shape):
    for S, Dn in zip(src_shape, dst_shape):
        s0, s1, a0, a1 = RC.taps(S, Dn)
        assert s0.min() >= 0 and s1.max() <= S - 1 and (s1 >= s0).all() and (s1 - s0 <= 1).all()
        assert ((a0 + a1) == 2048).all() and a1.min() >= 0 and a1.max() <= 2048
        i = RC.nearest_index(S, Dn)
        assert i.min() >= 0 and i.max() <= S - 1 and (np.diff(i) >= 0).all()


def test_taps_at_the_extent_limit_need_no_more_than_64_bits():
    for S, Dn in ((RC.MAX_EXTENT, 1), (1, RC.MAX_EXTENT), (RC.MAX_EXTENT, RC.MAX_EXTENT), (RC.MAX_EXTENT, RC.MAX_EXTENT - 1)):
        s0, s1, a0, a1 = RC.taps(S, Dn)
        assert s0.min() >= 0 and s1.max() <= S - 1 and a1.min() >= 0 and a1.max() <= 2048
        # python integers (unbounded) agree with the int64 arrays at the far end
        d = Dn - 1
        num, den = (2 * d + 1) * S - Dn, 2 * Dn
        s = min(num // den, S - 1)
        assert int(s0[-1]) == s and int(a1[-1]) == (0 if s >= S - 1 else ((num % den) * 4096 + den) // (2 * den))


@pytest.mark.parametrize("src_shape,dst_shape", PAIRS)
def test_nearest_keeps_binary_masks_binary(src_shape, dst_shape):
    m = RC.binary_sources([src_shape], 2)[0]
    out = RC.nearest(m, *dst_shape)
    assert set(np.unique(out)) <= {0, 255}
    # every destination pixel is a source pixel of its own row / column band
    assert np.array_equal(out[0, 0], m[0, 0]) and np.array_equal(out[-1, -1], m[min((dst_shape[0] - 1) * src_shape[0] // dst_shape[0], src_shape[0] - 1),
                                                                                min((dst_shape[1] - 1) * src_shape[1] // dst_shape[1], src_shape[1] - 1)])


# -- 2. the destination-driven restatement equals the forward oracle -------------------------------------------------------------
def _batches():
    """(name, samples, codes, colours, destination) of every batch the GPU test runs at small sizes"""
    out = []
    for dst in RC.DST_SHAPES:
        out.append(("batch16", RC.sources(RC.BATCH_SHAPES, 3), RC.BATCH_CODES, RC.COLOR_CODES, dst))
        out.append(("mixed", RC.sources(RC.MIXED_SHAPES, 3, seed=8), RC.MIXED_CODES, RC.COLOR_CODES[3:3 + len(RC.MIXED_SHAPES)], dst))
    return out


def test_tables_hold_what_the_issue_lists():
    assert RC.DST_SHAPES == [(16, 16), (32, 32), (16, 48), (48, 16)]
    assert set(RC.SRC_SHAPES) == {(1, 1), (1, 9), (9, 1), (7, 5), (16, 16), (32, 32), (37, 53), (100, 75), (255, 3)}
    assert RC.UPSCALE == ((8, 8), (32, 32)) and RC.UPSCALE[0] in RC.MIXED_SHAPES and set(RC.SRC_SHAPES) <= set(RC.MIXED_SHAPES)
    assert sorted(RC.BATCH_CODES) == list(range(16)) and all(h != w for h, w in RC.BATCH_SHAPES)
    assert len(RC.MIXED_CODES) == len(RC.MIXED_SHAPES) and len(RC.LARGE_CODES) == len(RC.LARGE_SRC) == RC.LARGE_DST[0]
    n, h, w = RC.LARGE_DST
    assert n * h * w > PC.GRID_CAP_PIXELS and h % 16 == 0 and w % 16 == 0
    assert {c[0] for c in RC.COLOR_CODES} == {CC.NONE, CC.HSV, CC.BRIGHTNESS, CC.CONTRAST}


@pytest.mark.parametrize("mode", [RC.LINEAR, RC.NEAREST])
def test_restatement_equals_the_forward_oracle(mode):
    for name, samples, codes, colors, dst in _batches():
        for i, s in enumerate(samples):
            for col in (None, colors[i]) if mode == RC.LINEAR else (None,):
                exp = RC.reference(s, dst[0], dst[1], mode, codes[i], col)
                got = RC.restate(s, dst[0], dst[1], mode, codes[i], col)
                assert exp.shape == dst + (3,)
                assert np.array_equal(got, exp), (name, i, s.shape, codes[i], col, dst)


# -- 3. mutations are detected ---------------------------------------------------------------------------------------------------
def _detected(fn):
    """number of (batch, sample) cases on which fn(sample, code, dst) differs from the oracle"""
    hits = 0
    for name, samples, codes, colors, dst in _batches():
        for i, s in enumerate(samples):
            hits += int(not np.array_equal(fn(s, codes[i], dst), RC.reference(s, dst[0], dst[1], RC.LINEAR, codes[i])))
    return hits


@pytest.mark.parametrize("mutation", RC.TAP_MUTATIONS)
def test_tap_mutations_are_detected(mutation):
    hits = _detected(lambda s, code, dst: RC.reference(s, dst[0], dst[1], RC.LINEAR, code, mutate=mutation))
    print(mutation, "detected on", hits, "cases")
    assert hits >= 8


def test_resize_before_augmentation_is_detected_on_non_square_sources():
    hits = 0
    for name, samples, codes, colors, dst in _batches():
        for i, s in enumerate(samples):
            if s.shape[0] == s.shape[1] or not codes[i] & 1:
                continue
            wrong = RC.reference(s, dst[0], dst[1], RC.LINEAR, codes[i], mutate="resize_first")
            assert wrong.shape == dst + (3,)
            hits += int(not np.array_equal(wrong, RC.reference(s, dst[0], dst[1], RC.LINEAR, codes[i])))
    print("resize_first detected on", hits, "cases")
    assert hits >= 8


def test_source_height_for_width_after_an_odd_rot90_is_detected():
    hits = total = 0
    for name, samples, codes, colors, dst in _batches():
        for i, s in enumerate(samples):
            wrong = RC.restate(s, dst[0], dst[1], RC.LINEAR, codes[i], mutate="hs_for_ws")
            same = np.array_equal(wrong, RC.reference(s, dst[0], dst[1], RC.LINEAR, codes[i]))
            if codes[i] & 1 and s.shape[0] != s.shape[1]:
                total += 1
                hits += int(not same)
            else:
                assert same          # the mutation touches odd counts on non-square sources only
    print("hs_for_ws detected on %d of %d odd-count non-square cases" % (hits, total))
    assert total >= 16 and hits == total


# -- 4. pack_ragged ------------------------------------------------------------------------------------------------------------
def test_pack_ragged_layout_matches_the_oracle_packing():
    samples = RC.sources(RC.MIXED_SHAPES, 3)
    pool, desc = D.pack_ragged(samples)
    p2, d2 = RC.pack(samples)
    assert np.array_equal(pool.numpy(), p2) and np.array_equal(desc.numpy(), d2)
    assert desc.dtype.is_floating_point is False and tuple(desc.shape) == (len(samples), L.SAMPLE_WORDS)
    off = desc.numpy().view(np.int64)[:, 0]
    for i, s in enumerate(samples):
        assert np.array_equal(pool.numpy()[off[i]:off[i] + s.size].reshape(s.shape), s)
    D.check_descriptors(desc, pool.numel(), 3, len(samples))


def test_pack_ragged_refusals():
    ok = np.zeros((4, 5, 3), np.uint8)
    for bad in ([], [ok.astype(np.float32)], [ok[..., 0]], [ok, np.zeros((4, 5, 1), np.uint8)], [np.zeros((0, 5, 3), np.uint8)]):
        with pytest.raises(L.NunetError):
            D.pack_ragged(bad)
    with pytest.raises(L.NunetError, match="extents"):
        D.pack_ragged([np.zeros((1, L.RESIZE_MAX_EXTENT + 1, 1), np.uint8)])
    D.pack_ragged([np.zeros((1, L.RESIZE_MAX_EXTENT, 1), np.uint8)])


def test_descriptor_refusals():
    pool, desc = D.pack_ragged([np.zeros((4, 5, 3), np.uint8), np.zeros((2, 2, 3), np.uint8)])
    nb = pool.numel()
    D.check_descriptors(desc, nb, 3, 2)

    def edited(row, col, value):
        d = desc.numpy().copy()
        if col == 0:
            d.view(np.int64)[row, 0] = value
        else:
            d[row, col] = value
        return d

    with pytest.raises(L.NunetError, match="outside the pool"):
        D.check_descriptors(desc, nb - 1, 3, 2)                     # the last sample ends past the pool
    with pytest.raises(L.NunetError, match="outside the pool"):
        D.check_descriptors(edited(1, 0, nb - 11), nb, 3, 2)       # offset moved by one byte
    with pytest.raises(L.NunetError, match="outside the pool"):
        D.check_descriptors(edited(0, 0, -1), nb, 3, 2)
    with pytest.raises(L.NunetError, match="outside the pool"):
        D.check_descriptors(desc, nb, 4, 2)                         # more channels than were packed
    for col, v in ((2, 0), (3, 0), (2, -3), (3, L.RESIZE_MAX_EXTENT + 1)):
        with pytest.raises(L.NunetError, match="extents"):
            D.check_descriptors(edited(0, col, v), nb, 3, 2)
    with pytest.raises(L.NunetError, match="int32"):
        D.check_descriptors(desc.numpy().astype(np.int64), nb, 3, 2)
    with pytest.raises(L.NunetError, match="int32"):
        D.check_descriptors(desc, nb, 3, 3)                         # one descriptor short of the batch
    with pytest.raises(L.NunetError, match="int32"):
        D.check_descriptors(desc.numpy()[:, :3], nb, 3, 2)


# -- 5. FolderDataset ------------------------------------------------------------------------------------------------------------
@pytest.fixture
def folder(tmp_path):
    from PIL import Image
    shapes = [(7, 5), (16, 16), (37, 53), (9, 1), (12, 20), (5, 5), (8, 3), (3, 8), (10, 10), (6, 4)]
    g = np.random.default_rng(2)
    root = tmp_path / "inputs"
    (root / "set" / "images").mkdir(parents=True)
    truth = {}
    for c in range(2):
        (root / "set" / "masks" / str(c)).mkdir(parents=True)
    for i, (h, w) in enumerate(shapes):
        rgb = g.integers(0, 256, (h, w, 3), dtype=np.uint8)
        masks = (g.integers(0, 2, (h, w, 2), dtype=np.uint8) * 255).astype(np.uint8)
        name = "img%02d" % i
        Image.fromarray(rgb).save(str(root / "set" / "images" / (name + ".png")))
        for c in range(2):
            Image.fromarray(masks[..., c]).save(str(root / "set" / "masks" / str(c) / (name + ".png")))
        truth[name] = (rgb, masks)
    (root / "set" / "images" / "notes.txt").write_text("not an image")
    return str(root), truth


def test_folder_dataset_layout_order_and_split(folder):
    root, truth = folder
    ds = D.FolderDataset("set", ".png", ".png", num_classes=2, root=root)
    assert ds.ids == sorted(truth) and len(ds) == 10
    for k, name in enumerate(ds.ids):
        img, mask = ds[k]
        rgb, masks = truth[name]
        assert img.dtype == np.uint8 and img.flags["C_CONTIGUOUS"] and mask.flags["C_CONTIGUOUS"]
        assert np.array_equal(img, rgb[:, :, ::-1]), "BGR, as cv2.imread leaves it"
        assert np.array_equal(mask, masks) and mask.shape == rgb.shape[:2] + (2,)
    tr = D.FolderDataset("set", num_classes=2, root=root, split="train")
    va = D.FolderDataset("set", num_classes=2, root=root, split="val")
    assert len(tr) == 8 and len(va) == 2 and sorted(tr.ids + va.ids) == ds.ids
    perm = np.random.RandomState(41).permutation(10)
    assert va.ids == [ds.ids[i] for i in perm[:2]] and tr.ids == [ds.ids[i] for i in perm[2:]]
    ip, idesc, mp, mdesc = tr.batch([0, 3, 5])
    assert ip.numel() == sum(truth[tr.ids[i]][0].size for i in (0, 3, 5))
    assert mp.numel() == sum(truth[tr.ids[i]][1].size for i in (0, 3, 5))
    assert np.array_equal(idesc.numpy()[:, 2:], mdesc.numpy()[:, 2:])
    with pytest.raises(L.NunetError):
        D.FolderDataset("absent", root=root)
    with pytest.raises(L.NunetError):
        D.FolderDataset("set", root=root, split="test")
