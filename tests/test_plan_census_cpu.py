"""Host-only: the geometries of tests/block_cases.py reach the launch regimes the per-block backward parity test
(test_backward_blocks_gpu.py) is there to put under a per-element fp64 check. The layer descriptors are rebuilt from the
architecture (block_cases.descriptors) and classified by the launch's own host queries; a case list that stops reaching a
required regime - because a case or the policy changed - fails here instead of passing vacuously on the GPU.

Not required, on purpose: the forward multi-item loop (items > grid), which needs more than 131 072 pixels under today's
policy and stays with test_conv_tiles_gpu.py and the bs16 96x96 tests; and tile 4 (256 x 64), which the policy never
chooses."""
import itertools

import pytest

import block_cases as B
from nunet_amd import _lib as L

TILINGS = ("regular", "multi-image", "stacked-rows")
SPLITS = ("S=1", "S>1")


@pytest.fixture(scope="module")
def fp32_union():
    out = set()
    for case in B.CASES:
        out |= B.model_regimes(case, L.F32)
    return out


def some(union, kind, tile=None, tiling=None, split=None, regime=None):
    want = (kind, tile, tiling, split, regime)
    return [r for r in union if all(w is None or w == v for w, v in zip(want, r))]


def test_cases_stay_small():
    for case, (unet, n, h, w, ncls, cin, ds) in B.CASES.items():
        assert n * h * w <= 30000 and h % 16 == 0 and w % 16 == 0, case


def test_forward_convs_reach_every_tiling_with_and_without_a_k_split(fp32_union):
    for tiling, split in itertools.product(TILINGS, SPLITS):
        assert some(fp32_union, "fwd", tiling=tiling, split=split), (tiling, split)
    assert not some(fp32_union, "fwd", regime="multi-item")      # stated in the module docstring: not these cases' job
    assert not some(fp32_union, "fwd", tile=4) and not some(fp32_union, "dgrad", tile=4)


def test_input_gradient_convs_reach_every_tile_item_regime_tiling_and_split(fp32_union):
    for tile in (1, 2, 3):
        assert some(fp32_union, "dgrad", tile=tile), tile
    for tile, regime in itertools.product((2, 3), ("one-item", "multi-item")):
        assert some(fp32_union, "dgrad", tile=tile, regime=regime), (tile, regime)
    for tiling, split in itertools.product(TILINGS, SPLITS):
        assert some(fp32_union, "dgrad", tiling=tiling, split=split), (tiling, split)


def test_case_a_alone_reaches_the_large_tiles_in_both_item_regimes():
    a = B.model_regimes("A", L.F32)
    for tile, regime in itertools.product((2, 3), ("one-item", "multi-item")):
        assert some(a, "dgrad", tile=tile, regime=regime), (tile, regime)


def test_weight_gradients_reach_both_slice_regimes(fp32_union):
    assert some(fp32_union, "wgrad", split="1<k<nMT")      # slices that walk more than one pixel tile
    assert some(fp32_union, "wgrad", split="k=nMT")        # one pixel tile per slice
    assert {r[1] for r in some(fp32_union, "wgrad")} == {11}      # the plan requests the default 32 x 32 items only


@pytest.mark.parametrize("dt", [L.F32, L.BF16, L.F16])
@pytest.mark.parametrize("case", list(B.CASES))
def test_every_modelled_descriptor_is_one_the_launch_accepts(case, dt):
    fwd, bwd, wg = B.descriptors(case, dt)
    unet = B.CASES[case][0]
    nblocks = len(B.nodes(unet))
    assert len(fwd) == 2 * nblocks and len(bwd) == 2 * nblocks - 1 and len(wg) == nblocks
    for _, d in fwd + bwd:
        o = B.conv_info(d)
        assert o.items == o.nCoT * o.tilesX * o.tilesY * o.tilesG * o.S and 1 <= o.grid <= o.items
        assert o.S == 1 or d.splitk_ws_floats >= o.S * d.N * d.H * d.W * (d.D0 + d.D1)
    for _, a, b in wg:
        for d in (a, b):
            o = B.wgrad_info(d)
            assert 1 <= o.ksplit <= d.max_slabs and o.grid == o.nCoT * o.nCiT * o.ksplit


def test_16_bit_legs_keep_the_large_tiles_and_the_multi_item_loop():
    """the bf16 / fp16 legs of the GPU test (cases A and B) run the same tiles and item regimes as the fp32 leg"""
    for dt in (L.BF16, L.F16):
        u = B.model_regimes("A", dt) | B.model_regimes("B", dt)
        for tile, regime in itertools.product((2, 3), ("one-item", "multi-item")):
            assert some(u, "dgrad", tile=tile, regime=regime), (dt, tile, regime)


@pytest.mark.parametrize("case", ["B", "C"])
def test_one_hop_sums_reproduce_the_end_to_end_gradient_in_fp64(case):
    """The scheme of test_backward_blocks_gpu.py on the oracle's own tensors: with every block fed the exact block outputs
    and the exact dL/dx_{i,j}, the sum of the one-hop contributions IS the end-to-end gradient of every slot and every
    parameter (fp64 summation order aside) - deep supervision with 4 classes (B) and the U-Net wiring (C) included."""
    import torch
    feats, logits, net = B.end_to_end(case, torch.float64, True)
    slot, pgrads = B.one_hop(case, {k: v.detach() for k, v in feats.items()}, {k: v.grad for k, v in feats.items()},
                             [x.grad for x in logits], torch.float64)
    assert sorted(slot) == sorted(feats)
    for k, f in feats.items():
        assert B.rel_err(slot[k], f.grad)[0] < 1e-13, k
    for nm, p in net.params.items():
        assert B.rel_err(pgrads[nm], p.grad)[0] < 1e-13 or float(p.grad.abs().max()) < 1e-18, nm
