"""The device-side Resize on ragged uint8 sources (nunet_resize_u8, nunet_preprocess_u8_resize, nunet_plan_stage_u8_resize,
TrainStep(resize=True).step_u8_ragged) against the numpy oracle of tests/resize_cases.py.

Criteria. The definition is integer arithmetic, so nunet_resize_u8's bytes must EQUAL the oracle's: both modes, with and
without augmentation and colour codes, every source shape of the table, every one of the 16 codes on a non-square source. The
staged image is decoded back to bytes (pipeline_cases.decode_bytes: the NULL mean / std, post_scale = 1 configuration) for every
storage type and compared with the same oracle. The fused entries are compared bit for bit with their two-launch
compositions, equal-size sources with the non-resizing entries, and a captured resizing step with a captured step_u8 fed the
same bytes. One destination is past the 4096 x 256-thread grid cap."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import nunet_amd  # noqa: E402
from nunet_amd import _lib as L  # noqa: E402
from nunet_amd import dataset as D  # noqa: E402
from nunet_amd.engine import Plan  # noqa: E402
import color_cases as CC  # noqa: E402
import pipeline_cases as PC  # noqa: E402
import resize_cases as RC  # noqa: E402

DEV = "cuda:0"
KINDS = {"fp32": L.F32, "bf16": L.BF16, "fp16": L.F16}
FILL = 0xA5
ZERO3, ONE3 = np.zeros(3, np.float32), np.ones(3, np.float32)
MEAN3, STD3 = np.asarray(D.MEAN, np.float32), np.asarray(D.STD, np.float32)
# the node count of the captured step (segmented=False, schedule='lanes': one hipGraph, one node per launch) of
# NestedUNet(1, 3, False), batch 4 x 3 x 32 x 32, SGD, input_u8=True, as counted on the commit before the resize entries existed
PARENT_STEP_NODES = 157


@pytest.fixture(autouse=True)
def _canaries(guard_bands):
    """every device buffer these tests allocate sits between guard bands that are checked after the test (conftest.py)"""
    yield


def dev(a):
    if a is None:
        return None
    a = torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a
    t = torch.empty(a.shape, dtype=a.dtype, device=DEV)
    t.copy_(a)
    return t


def aug_dev(codes):
    return None if codes is None else dev(np.asarray(codes, np.int32))


def color_dev(codes):
    return None if codes is None else dev(D.color_codes([c[0] for c in codes], [c[1:] for c in codes]))


class Ragged:
    """a packed batch on the device: the pool sits in a guarded buffer of exactly its size, so a read past a sample's end
    that leaves the pool would also leave the allocation's payload"""

    def __init__(self, samples):
        pool, desc = RC.pack(samples)
        self.pool_host, self.n, self.c = pool, len(samples), samples[0].shape[2]
        self.pool, self.desc, self.bytes = dev(pool), dev(desc), int(pool.size)


def resize_u8(r, hd, wd, mode, codes=None, colors=None):
    out = torch.full((r.n, hd, wd, r.c), 7, dtype=torch.uint8, device=DEV)
    L.check(L.lib().nunet_resize_u8(L.ptr(r.pool), r.bytes, L.ptr(r.desc), r.n, r.c, hd, wd, mode, L.ptr(aug_dev(codes)), L.ptr(color_dev(colors)),
                                    L.ptr(out), L.stream()), "nunet_resize_u8")
    torch.cuda.synchronize()
    assert np.array_equal(r.pool.cpu().numpy(), r.pool_host), "the pool was written"
    return out


def preprocess_u8_resize(r, hd, wd, codes, mean, std, post_scale):
    out = torch.full((r.n, r.c, hd, wd), 7.0, dtype=torch.float32, device=DEV)
    m = dev(None if mean is None else np.resize(np.asarray(mean, np.float32), r.c))
    s = dev(None if std is None else np.resize(np.asarray(std, np.float32), r.c))
    L.check(L.lib().nunet_preprocess_u8_resize(L.ptr(r.pool), r.bytes, L.ptr(r.desc), r.n, r.c, hd, wd, L.ptr(m), L.ptr(s), L.ptr(aug_dev(codes)),
                                               post_scale, L.ptr(out), L.stream()), "nunet_preprocess_u8_resize")
    torch.cuda.synchronize()
    return out


def make_plan(n, h, w, cin, kind):
    """a plan pruned to depth 1: the staging launch and the image buffer of the full plan, a small arena"""
    return Plan(n, h, w, cin, 1, True, KINDS[kind], False, DEV, depth=1)


def _image_bits(pl):
    torch.cuda.synchronize()
    img = pl.image()
    assert tuple(img.shape) == (pl.n, pl.h, pl.w, 32)
    host = img.cpu().contiguous()
    return host.float().numpy(), host.view(torch.int32 if pl.dtype == L.F32 else torch.int16).numpy()


def _image_region_only(pl):
    off = L.lib().nunet_plan_image(pl.handle, None, None)
    size = pl.n * pl.h * pl.w * 32 * (4 if pl.dtype == L.F32 else 2)
    assert off >= 0 and off + size <= pl.arena_bytes
    assert bool((pl.arena[:off] == FILL).all()) and bool((pl.arena[off + size:] == FILL).all()), "the staging launch wrote outside the image"


def stage_resize(pl, r, codes, colors, mean, std, post_scale, check_rest=True):
    pl.arena.fill_(FILL)
    m = dev(None if mean is None else np.resize(np.asarray(mean, np.float32), r.c))
    s = dev(None if std is None else np.resize(np.asarray(std, np.float32), r.c))
    L.check(L.lib().nunet_plan_stage_u8_resize(pl.handle, L.ptr(r.pool), r.bytes, L.ptr(r.desc), L.ptr(m), L.ptr(s), L.ptr(aug_dev(codes)),
                                               L.ptr(color_dev(colors)), post_scale, L.ptr(pl.arena), L.nbytes(pl.arena), L.stream()),
            "nunet_plan_stage_u8_resize")
    out = _image_bits(pl)
    if check_rest:
        _image_region_only(pl)
    return out


def stage_dense(pl, u8_dev, codes, colors, mean, std, post_scale):
    """nunet_plan_stage_u8(_color) on a dense device batch"""
    pl.arena.fill_(FILL)
    c = u8_dev.shape[-1]
    m = dev(None if mean is None else np.resize(np.asarray(mean, np.float32), c))
    s = dev(None if std is None else np.resize(np.asarray(std, np.float32), c))
    if colors is None:
        L.check(L.lib().nunet_plan_stage_u8(pl.handle, L.ptr(u8_dev), L.ptr(m), L.ptr(s), L.ptr(aug_dev(codes)), post_scale, L.ptr(pl.arena),
                                            L.nbytes(pl.arena), L.stream()), "nunet_plan_stage_u8")
    else:
        L.check(L.lib().nunet_plan_stage_u8_color(pl.handle, L.ptr(u8_dev), L.ptr(m), L.ptr(s), L.ptr(aug_dev(codes)), L.ptr(color_dev(colors)),
                                                  post_scale, L.ptr(pl.arena), L.nbytes(pl.arena), L.stream()), "nunet_plan_stage_u8_color")
    return _image_bits(pl)


def assert_batch_equal(got, exp, what):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    for i in range(exp.shape[0]):
        bad = got[i] != exp[i]
        if bad.any():
            y, x, c = (int(v) for v in np.argwhere(bad)[0])
            raise AssertionError("%s: sample %d: %d of %d bytes differ; first at (y, x, c) = (%d, %d, %d): found %d, expected %d"
                                 % (what, i, int(bad.sum()), bad.size, y, x, c, int(got[i, y, x, c]), int(exp[i, y, x, c])))


BATCHES = {"batch16": (RC.BATCH_SHAPES, RC.BATCH_CODES, RC.COLOR_CODES, 5),
           "mixed": (RC.MIXED_SHAPES, RC.MIXED_CODES, RC.COLOR_CODES[3:3 + len(RC.MIXED_SHAPES)], 8)}
VARIANTS = [("linear", RC.LINEAR, False, False), ("linear+aug", RC.LINEAR, True, False), ("linear+colour", RC.LINEAR, False, True),
            ("linear+aug+colour", RC.LINEAR, True, True), ("nearest", RC.NEAREST, False, False), ("nearest+aug", RC.NEAREST, True, False)]


# -- 1. nunet_resize_u8 against the oracle, byte for byte ---------------------------------------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS, ids=[v[0] for v in VARIANTS])
@pytest.mark.parametrize("dst", RC.DST_SHAPES)
@pytest.mark.parametrize("batch", sorted(BATCHES))
def test_resize_u8_equals_the_oracle(batch, dst, variant):
    shapes, codes, colors, seed = BATCHES[batch]
    name, mode, with_aug, with_color = variant
    for c in ((3,) if with_color else (3, 1, 4)):
        samples = RC.binary_sources(shapes, c, seed) if mode == RC.NEAREST else RC.sources(shapes, c, seed)
        r = Ragged(samples)
        got = resize_u8(r, dst[0], dst[1], mode, codes if with_aug else None, colors if with_color else None)
        exp = RC.reference_batch(samples, dst[0], dst[1], mode, codes if with_aug else None, colors if with_color else None)
        assert_batch_equal(got, exp, "%s %s -> %s C=%d" % (batch, name, dst, c))
        if mode == RC.NEAREST:
            assert set(np.unique(got.cpu().numpy())) <= {0, 255}


# -- 2. the staged image, every storage type ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dst", RC.DST_SHAPES)
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_stage_u8_resize_decodes_to_the_oracle_bytes(kind, dst):
    shapes, codes, colors, seed = BATCHES["batch16"]
    samples = RC.sources(shapes, 3, seed)
    r = Ragged(samples)
    pl = make_plan(len(samples), dst[0], dst[1], 3, kind)
    for what, cd, col, mean, std in (("plain", None, None, None, None), ("aug", codes, None, None, None), ("aug+colour", codes, colors, ZERO3, ONE3)):
        img, bits = stage_resize(pl, r, cd, col, mean, std, 1.0)
        exp = RC.reference_batch(samples, dst[0], dst[1], RC.LINEAR, cd, col)
        got = PC.decode_bytes(img[..., :3], kind)
        assert_batch_equal(got, exp.astype(np.int16), "stage_u8_resize %s %s %s" % (kind, dst, what))
        assert not bits[..., 3:].any(), "padding channels are zero bits"


@pytest.mark.parametrize("cin", [1, 4, 32])
def test_stage_u8_resize_other_channel_counts(cin):
    shapes, codes, _, seed = BATCHES["mixed"]
    samples = RC.sources(shapes, cin, seed)
    r = Ragged(samples)
    pl = Plan(len(samples), 16, 48, cin, 1, False, L.F32, False, DEV)
    img, bits = stage_resize(pl, r, codes, None, None, None, 1.0)
    exp = RC.reference_batch(samples, 16, 48, RC.LINEAR, codes)
    assert_batch_equal(PC.decode_bytes(img[..., :cin], "fp32"), exp.astype(np.int16), "stage_u8_resize C=%d" % cin)
    assert not bits[..., cin:].any()


# -- 3. fused entries = their two-launch compositions, bit for bit ----------------------------------------------------------------
@pytest.mark.parametrize("batch", sorted(BATCHES))
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_stage_u8_resize_equals_resize_then_stage(kind, batch):
    shapes, codes, colors, seed = BATCHES[batch]
    samples = RC.sources(shapes, 3, seed)
    r = Ragged(samples)
    for dst in ((32, 32), (16, 48)):
        pl = make_plan(len(samples), dst[0], dst[1], 3, kind)
        for cd, col in ((None, None), (codes, None), (codes, colors)):
            fused = stage_resize(pl, r, cd, col, MEAN3, STD3, 1.0 / 255.0)[1]
            two = stage_dense(pl, resize_u8(r, dst[0], dst[1], RC.LINEAR, cd, col), None, None, MEAN3, STD3, 1.0 / 255.0)[1]
            assert np.array_equal(fused, two), (kind, batch, dst, cd is not None, col is not None)
            # and against the oracle: the numpy resize followed by the existing staging entry
            exp = RC.reference_batch(samples, dst[0], dst[1], RC.LINEAR, cd, col)
            assert np.array_equal(fused, stage_dense(pl, dev(exp), None, None, MEAN3, STD3, 1.0 / 255.0)[1])


@pytest.mark.parametrize("batch", sorted(BATCHES))
def test_preprocess_u8_resize_equals_resize_then_preprocess(batch):
    shapes, codes, _, seed = BATCHES[batch]
    for c, mean, std, ps in ((1, None, None, 1.0), (2, None, None, 1.0), (3, MEAN3, STD3, 1.0 / 255.0)):
        samples = RC.binary_sources(shapes, c, seed) if mean is None else RC.sources(shapes, c, seed)
        r = Ragged(samples)
        for dst in RC.DST_SHAPES:
            for cd in (None, codes):
                fused = preprocess_u8_resize(r, dst[0], dst[1], cd, mean, std, ps)
                u8 = resize_u8(r, dst[0], dst[1], RC.NEAREST, cd)
                two = torch.full(fused.shape, 7.0, dtype=torch.float32, device=DEV)
                m, s = dev(mean), dev(std)
                L.check(L.lib().nunet_preprocess_u8(L.ptr(u8), r.n, dst[0], dst[1], c, L.ptr(m), L.ptr(s), None, ps, L.ptr(two), L.stream()), "nunet_preprocess_u8")
                assert torch.equal(fused, two), (batch, c, dst, cd is not None)
                exp = RC.reference_batch(samples, dst[0], dst[1], RC.NEAREST, cd)
                if mean is None:
                    assert np.array_equal(fused.cpu().numpy().transpose(0, 2, 3, 1), (exp // 255).astype(np.float32)), "masks are exactly 0 and 1"


def test_dataset_wrappers_feed_floats():
    """resize_images / resize_masks: what validation hands to EvalStep (float32 NCHW), from the host tensors pack_ragged returns"""
    shapes, codes, _, seed = BATCHES["mixed"]
    imgs, masks = RC.sources(shapes, 3, seed), RC.binary_sources(shapes, 1, seed)
    ip, idesc = D.pack_ragged(imgs)
    mp, mdesc = D.pack_ragged(masks)
    x = D.resize_images(ip, idesc, (32, 32))
    t = D.resize_masks(mp, mdesc, (32, 32))
    assert tuple(x.shape) == (len(shapes), 3, 32, 32) and tuple(t.shape) == (len(shapes), 1, 32, 32) and x.dtype == t.dtype == torch.float32
    assert torch.equal(x, D.preprocess_images(dev(RC.reference_batch(imgs, 32, 32, RC.LINEAR))))
    assert torch.equal(t, D.preprocess_masks(dev(RC.reference_batch(masks, 32, 32, RC.NEAREST))))
    a = aug_dev(codes)
    assert torch.equal(D.resize_masks(mp, mdesc, (16, 48), aug=a), D.preprocess_masks(dev(RC.reference_batch(masks, 16, 48, RC.NEAREST, codes))))


# -- 4. equal-size sources give the bits of the non-resizing entries -----------------------------------------------------------------
@pytest.mark.parametrize("kind", sorted(KINDS))
@pytest.mark.parametrize("hw,codes", [((32, 32), PC.ALL_CODES), ((16, 48), PC.EVEN_CODES)])
def test_equal_size_sources_give_the_dense_entries_bits(kind, hw, codes):
    h, w = hw
    n = len(codes)
    u = np.random.default_rng(h + n).integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    m8 = (np.random.default_rng(w).integers(0, 2, (n, h, w, 1), dtype=np.uint8) * 255).astype(np.uint8)
    colors = RC.COLOR_CODES[:n]
    r, rm = Ragged(list(u)), Ragged(list(m8))
    pl = make_plan(n, h, w, 3, kind)
    for cd, col in ((None, None), (codes, None), (codes, colors)):
        fused = stage_resize(pl, r, cd, col, MEAN3, STD3, 1.0 / 255.0)[1]
        dense = stage_dense(pl, dev(u), cd, col, MEAN3, STD3, 1.0 / 255.0)[1]
        assert np.array_equal(fused, dense), (kind, hw, cd is not None, col is not None)
    if kind == "fp32":
        for cd in (None, codes):
            fused = preprocess_u8_resize(rm, h, w, cd, None, None, 1.0)
            dense = torch.full(fused.shape, 7.0, dtype=torch.float32, device=DEV)
            L.check(L.lib().nunet_preprocess_u8(L.ptr(dev(m8)), n, h, w, 1, None, None, L.ptr(aug_dev(cd)), 1.0, L.ptr(dense), L.stream()), "nunet_preprocess_u8")
            assert torch.equal(fused, dense)
        assert_batch_equal(resize_u8(r, h, w, RC.LINEAR), u, "identity, bilinear")
        assert_batch_equal(resize_u8(rm, h, w, RC.NEAREST), m8, "identity, nearest")


# -- 5. past the grid cap --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def large():
    n, h, w = RC.LARGE_DST
    assert n * h * w > PC.GRID_CAP_PIXELS
    samples = RC.sources(RC.LARGE_SRC, 3, seed=12)
    colors = [CC.BYTE_CODES[3], CC.BYTE_CODES[6], CC.BYTE_CODES[4], CC.BYTE_CODES[6], CC.BYTE_CODES[5]]
    return samples, colors, RC.reference_batch(samples, h, w, RC.LINEAR, RC.LARGE_CODES, colors)


def test_capped_grid_resize_u8(large):
    samples, colors, exp = large
    n, h, w = RC.LARGE_DST
    r = Ragged(samples)
    assert_batch_equal(resize_u8(r, h, w, RC.LINEAR, RC.LARGE_CODES, colors), exp, "resize_u8 5x464x464 bilinear")
    masks = RC.binary_sources(RC.LARGE_SRC, 1, seed=13)
    rm = Ragged(masks)
    expm = RC.reference_batch(masks, h, w, RC.NEAREST, RC.LARGE_CODES)
    assert_batch_equal(resize_u8(rm, h, w, RC.NEAREST, RC.LARGE_CODES), expm, "resize_u8 5x464x464 nearest")
    got = preprocess_u8_resize(rm, h, w, RC.LARGE_CODES, None, None, 1.0).cpu().numpy().transpose(0, 2, 3, 1)
    assert np.array_equal(got, (expm // 255).astype(np.float32))


def test_capped_grid_preprocess_u8_resize_partial_last_block():
    """5 x 460 x 457 = 1,051,100 one-channel destination pixels against the 1,048,576 the grid holds: the last 2,524 are a thread's
    second trip, and that trip ends inside a block (the cases above are multiples of 256). Five small ragged masks, one of
    them a single pixel, a different rot90 / flip code each; NEAREST, then the mask preprocessing (NULL mean / std, post_scale 1)."""
    n, h, w = PC.LARGE_SHAPES["free"]
    assert n * h * w > PC.GRID_CAP_PIXELS and (n * h * w) % 256
    masks = RC.binary_sources([(5, 7), (40, 33), (1, 1), (17, 29), (33, 12)], 1, seed=14)
    codes = [1 | 4, 0, 3 | 8, 2, 1 | 4 | 8]
    exp = RC.reference_batch(masks, h, w, RC.NEAREST, codes)
    got = preprocess_u8_resize(Ragged(masks), h, w, codes, None, None, 1.0).cpu().numpy().transpose(0, 2, 3, 1)
    assert_batch_equal(PC.decode_bytes(got, "fp32"), exp.astype(np.int16), "preprocess_u8_resize 5x460x457")
    assert np.array_equal(got, PC.f32_values(exp, None, None, 1.0)) and set(np.unique(got)) <= {0.0, 1.0}


def test_capped_grid_stage_u8_resize(large):
    samples, colors, exp = large
    n, h, w = RC.LARGE_DST
    pl = make_plan(n, h, w, 3, "bf16")
    img, bits = stage_resize(pl, Ragged(samples), RC.LARGE_CODES, colors, ZERO3, ONE3, 1.0, check_rest=False)
    assert_batch_equal(PC.decode_bytes(img[..., :3], "bf16"), exp.astype(np.int16), "stage_u8_resize 5x464x464")
    assert not bits[..., 3:].any()


# -- 6. the captured step ----------------------------------------------------------------------------------------------------------
GRAPH = dict(segmented=False, schedule="lanes")      # the one-hipGraph executor: its node count is the step's launch count


def storage_bits(f32, kind):
    if kind == "bf16":
        return PC.round_bf16_bits(f32).view(np.int16)
    if kind == "fp16":
        return PC.round_fp16_bits(f32).view(np.int16)
    return np.ascontiguousarray(f32, np.float32).view(np.int32)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_captured_resizing_step(dtype, synth):
    """Two captured step_u8_ragged calls on sources of the plan's size equal two captured step_u8 calls on the same bytes: loss,
    parameters, momentum, BatchNorm buffers bit for bit, with the same number of graph nodes. The same captured step is then
    replayed with sources of other sizes: its staged image and target are the oracle's."""
    from nunet_amd.trainer import TrainStep
    n, hw = 4, 32
    torch.manual_seed(9)
    sd = {k: v.clone() for k, v in nunet_amd.archs.NestedUNet(1, 3, False).state_dict().items()}
    raw, m8 = synth.synth_blob_pairs_u8(3 * n, hw, hw, seed=77)
    augs = [[1, 2 | 4, 3 | 8, 12], [0, 3, 1 | 4, 2 | 8]]
    cols = [RC.COLOR_CODES[:4], RC.COLOR_CODES[3:7]]
    rag_shapes, rag_codes, rag_cols = [(37, 53), (100, 75), (7, 5), (255, 3)], [1, 3 | 4, 2 | 8, 1 | 12], RC.COLOR_CODES[1:5]
    rag_img, rag_msk = RC.sources(rag_shapes, 3, 21), RC.binary_sources(rag_shapes, 1, 22)
    cap = max(n * hw * hw * 3, sum(s.size for s in rag_img))

    def run(mode):
        m = nunet_amd.archs.NestedUNet(1, 3, False, dtype=dtype)
        m.load_state_dict(sd)
        m = m.to(DEV).train()
        ts = TrainStep(m, (n, 3, hw, hw), lr=1e-2, input_u8=True, color_aug=True, resize=mode == "resize",
                       source_capacity=cap if mode == "resize" else None, **GRAPH)
        if mode == "resize":
            ts.capture(D.pack_ragged(list(raw[:n])), D.pack_ragged(list(m8[:n])))
        else:
            ts.capture(dev(raw[:n]), dev(m8[:n]))
        assert ts.g_fb is not None
        losses = []
        for k in range(2):
            xb, tb = raw[(k + 1) * n:(k + 2) * n], m8[(k + 1) * n:(k + 2) * n]
            ts.reset_meters()
            if mode == "resize":
                ts.step_u8_ragged(*(D.pack_ragged(list(xb)) + D.pack_ragged(list(tb))), aug=aug_dev(augs[k]), color=color_dev(cols[k]))
            else:
                ts.step_u8(dev(xb), dev(tb), aug_dev(augs[k]), color_dev(cols[k]))
            losses.append(ts.epoch_stats())
        torch.cuda.synchronize()
        return losses, ts.eng.flat_params.clone(), ts.eng.bnbuf.clone(), ts.mom.clone(), ts.g_fb.info()["nodes"], ts

    rs, pl = run("resize"), run("plain")
    print("losses", rs[0], "graph nodes resize / plain: %d / %d" % (rs[4], pl[4]))
    assert rs[0] == pl[0], (rs[0], pl[0])
    assert torch.equal(rs[1], pl[1]) and torch.equal(rs[2], pl[2]) and torch.equal(rs[3], pl[3])
    assert rs[4] == pl[4], "the resizing step issues as many launches"
    # the same captured graph, sources of other sizes
    ts = rs[5]
    ts.step_u8_ragged(*(D.pack_ragged(rag_img) + D.pack_ragged(rag_msk)), aug=aug_dev(rag_codes), color=color_dev(rag_cols))
    torch.cuda.synchronize()
    exp = RC.reference_batch(rag_img, hw, hw, RC.LINEAR, rag_codes, rag_cols)
    want = storage_bits(PC.f32_values(exp, D.MEAN, D.STD, 1.0 / 255.0), dtype)
    host = ts.pl.image().cpu().contiguous()
    bits = host.view(torch.int32 if dtype == "fp32" else torch.int16).numpy()
    assert np.array_equal(bits[..., :3], want), "the staged image of the replay with new sizes"
    assert not bits[..., 3:].any()
    expm = RC.reference_batch(rag_msk, hw, hw, RC.NEAREST, rag_codes)
    assert np.array_equal(ts.t.cpu().numpy().transpose(0, 2, 3, 1), (expm // 255).astype(np.float32))
    # misuse is refused on the host, and nothing runs
    steps = ts.steps
    with pytest.raises(L.NunetError, match="source_capacity"):
        ts.step_u8_ragged(torch.zeros(cap + 1, dtype=torch.uint8), D.pack_ragged(rag_img)[1], *D.pack_ragged(rag_msk))
    with pytest.raises(L.NunetError, match="outside the pool"):
        ts.step_u8_ragged(D.pack_ragged(rag_img)[0][:-1], D.pack_ragged(rag_img)[1], *D.pack_ragged(rag_msk))
    with pytest.raises(L.NunetError, match="int32"):
        ts.step_u8_ragged(*(D.pack_ragged(rag_img[:3]) + D.pack_ragged(rag_msk[:3])))
    with pytest.raises(L.NunetError, match="step_u8_ragged"):
        ts.step_u8(dev(raw[:n]), dev(m8[:n]))
    with pytest.raises(L.NunetError, match="resize=True"):
        pl[5].step_u8_ragged(*(D.pack_ragged(rag_img) + D.pack_ragged(rag_msk)))
    assert ts.steps == steps


def test_step_without_resize_keeps_its_node_count():
    """resize=False changes nothing: the captured step of the configuration named at PARENT_STEP_NODES has the node count it
    had before the resize entries existed."""
    from nunet_amd.trainer import TrainStep
    n, hw = 4, 32
    torch.manual_seed(9)
    raw = np.random.default_rng(1).integers(0, 256, (n, hw, hw, 3), dtype=np.uint8)
    m8 = (np.random.default_rng(2).integers(0, 2, (n, hw, hw, 1), dtype=np.uint8) * 255).astype(np.uint8)
    m = nunet_amd.archs.NestedUNet(1, 3, False).to(DEV).train()
    ts = TrainStep(m, (n, 3, hw, hw), lr=1e-2, input_u8=True, resize=False, **GRAPH)
    ts.capture(dev(raw), dev(m8))
    nodes = ts.g_fb.info()["nodes"]
    print("graph nodes of the input_u8 step:", nodes)
    assert not hasattr(ts, "img_pool")
    assert nodes == PARENT_STEP_NODES


def test_python_misuse_raises():
    from nunet_amd.trainer import TrainStep
    m = nunet_amd.archs.NestedUNet(1, 3, False).to(DEV).train()
    with pytest.raises(L.NunetError, match="input_u8"):
        TrainStep(m, (2, 3, 32, 32), resize=True, source_capacity=1024)
    with pytest.raises(L.NunetError, match="source_capacity"):
        TrainStep(m, (2, 3, 32, 32), input_u8=True, resize=True)
    pool, desc = D.pack_ragged([np.zeros((4, 5, 3), np.uint8)])
    with pytest.raises(L.NunetError):
        D.resize_u8(pool, desc, 3, (8, 8), L.RESIZE_NEAREST, color=torch.zeros((1, 4), dtype=torch.int32, device=DEV))      # colour under NEAREST
    with pytest.raises(L.NunetError, match="outside the pool"):
        D.resize_u8(pool[:-1], desc, 3, (8, 8))
    with pytest.raises(L.NunetError, match="extents"):
        D.resize_u8(pool, desc, 3, (8, L.RESIZE_MAX_EXTENT + 1))
