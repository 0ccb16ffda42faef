"""The input-pipeline oracle and its case tables (tests/pipeline_cases.py) checked against themselves, without a GPU: the
numpy restatement of the kernels' inverse index map equals the forward library-call oracle on every case; every plausible
mutation of that map is caught by each table on its own; the value bound B is pinned to an fp32 numpy evaluation (not to a
kernel); the tag schemes are injective; the byte decoding the geometry tests rely on is exact in every storage type."""
import numpy as np
import pytest

import pipeline_cases as PC

TABLES = {"preprocess_u8": PC.U8_SHAPES, "plan": PC.PLAN_SHAPES}


def _batch(h, w, c=3):
    codes = PC.codes_for(h, w)
    return PC.tagged(len(codes), h, w, c, codes), codes


def test_case_tables_are_what_the_kernels_accept():
    for h, w in PC.U8_SHAPES + PC.PLAN_SHAPES:
        codes = PC.codes_for(h, w)
        assert len(codes) == (16 if h == w else 8)
        assert h == w or not any(c & 1 for c in codes)
        assert sorted(set(codes)) == codes
    assert all(h % 16 == 0 and w % 16 == 0 for h, w in PC.PLAN_SHAPES)
    assert any(h > w for h, w in PC.PLAN_SHAPES) and any(h < w for h, w in PC.PLAN_SHAPES) and any(h == w for h, w in PC.PLAN_SHAPES)
    assert all(1 <= c <= 32 for c in PC.PLAN_CHANNELS)


@pytest.mark.parametrize("h,w", PC.U8_SHAPES + PC.PLAN_SHAPES)
def test_restatement_equals_the_forward_oracle(h, w):
    for c in (1, 3, 4):
        u, codes = _batch(h, w, c)
        exp = PC.ref_batch(u, codes)
        assert exp.shape == u.shape
        msg = PC.first_mismatch(PC.restate_batch(u, codes), exp)
        assert not msg, msg
        for n in (0, len(codes) - 1):
            assert np.array_equal(PC.restate(u[n], codes[n]), PC.ref_geometry(u[n], codes[n]))
    assert np.array_equal(PC.ref_batch(u, None), u)
    assert np.array_equal(PC.ref_batch(u, [0] * len(codes)), u)


def test_forward_oracle_on_a_hand_written_case():
    """the oracle itself, against pixels written out by hand: [[a b c], [d e f]] (2 x 3)"""
    s = np.array([[1, 2, 3], [4, 5, 6]], np.uint8)[:, :, None]
    assert PC.ref_geometry(s, 0)[..., 0].tolist() == [[1, 2, 3], [4, 5, 6]]
    assert PC.ref_geometry(s, 1)[..., 0].tolist() == [[3, 6], [2, 5], [1, 4]]          # counter-clockwise
    assert PC.ref_geometry(s, 2)[..., 0].tolist() == [[6, 5, 4], [3, 2, 1]]
    assert PC.ref_geometry(s, 3)[..., 0].tolist() == [[4, 1], [5, 2], [6, 3]]
    assert PC.ref_geometry(s, 4)[..., 0].tolist() == [[3, 2, 1], [6, 5, 4]]            # hflip: columns mirrored
    assert PC.ref_geometry(s, 8)[..., 0].tolist() == [[4, 5, 6], [1, 2, 3]]            # vflip: rows mirrored
    assert PC.ref_geometry(s, 1 | 4)[..., 0].tolist() == [[6, 3], [5, 2], [4, 1]]      # rotate first, then mirror


@pytest.mark.parametrize("table", sorted(TABLES))
@pytest.mark.parametrize("mutate", PC.MUTATIONS)
def test_every_mutation_is_detected_by_each_table(table, mutate):
    caught = []
    for h, w in TABLES[table]:
        u, codes = _batch(h, w)
        if not np.array_equal(PC.restate_batch(u, codes, mutate), PC.ref_batch(u, codes)):
            caught.append((h, w))
    print("%s / %s: caught by %s" % (table, mutate, caught))
    assert caught, "mutation %r survives every case of the %s table" % (mutate, table)


def test_mismatch_message_decodes_the_pixel():
    u, codes = _batch(16, 16)
    bad = PC.decode_bytes(PC.quotient_table("bf16")[PC.restate_batch(u, codes, "clockwise")], "bf16")
    msg = PC.first_mismatch(bad, PC.ref_batch(u, codes))
    assert "destination (n, y, x) = (1, 0, 0)" in msg and "source y = 15, x = 0" in msg and "source y = 0, x = 15" in msg, msg


def test_tag_schemes_are_injective():
    for h, w in PC.U8_SHAPES + PC.PLAN_SHAPES:
        u, codes = _batch(h, w)
        assert PC.triples_injective(u), (h, w)
        u8 = PC.tagged(len(codes), h, w, 8, codes)
        assert np.array_equal(u8[..., :3], u)
    for n, h, w in PC.LARGE_SHAPES.values():
        u = PC.tagged_large(n, h, w)
        assert n * h * w > PC.GRID_CAP_PIXELS
        assert PC.triples_injective(u), (n, h, w)
        for px in ((0, 0, 0), (n - 1, h - 1, w - 1), (n // 2, 255, 256), (1, 256, 255)):
            assert PC.decode_large(u[px]) == px
    assert not PC.triples_injective(np.zeros((1, 2, 2, 3), np.uint8))


def test_bound_holds_for_the_fp32_numpy_evaluation():
    """all 256 bytes x the three ImageNet channels at post_scale = 1/255, and the 4-channel np.resize'd parameters"""
    worst = 0.0
    for c in (3, 4):
        u = PC.all_bytes_image(c)
        assert all(np.unique(u[..., ch]).size == 256 for ch in range(c))
        ref, B = PC.ref_values(u, PC.MEAN, PC.STD, 1.0 / 255.0)
        err = np.abs(PC.f32_values(u, PC.MEAN, PC.STD, 1.0 / 255.0).astype(np.float64) - ref)
        ratio = float((err / B).max())
        print("C=%d: max err %.3e, min B %.3e, max |ref| %.4f, max err/B %.3f" % (c, err.max(), B.min(), np.abs(ref).max(), ratio))
        assert np.all(err <= B)
        assert B.min() > 4e-10 and np.abs(ref).max() < 0.0104
        worst = max(worst, ratio)
    assert 0.5 < worst <= 1.0, "the bound is neither slack nor violated by a faithful fp32 evaluation: %.3f" % worst
    # the mask configuration: {0, 255} -> {0, 1} exactly, and every byte's fp32 quotient is its own
    m = np.array([0, 255], np.uint8).reshape(1, 1, 2, 1)
    assert PC.f32_values(m, None, None, 1.0).ravel().tolist() == [0.0, 1.0]
    q = PC.f32_values(np.arange(256, dtype=np.uint8).reshape(1, 1, 256, 1), None, None, 1.0).ravel()
    assert np.unique(q).size == 256 and np.array_equal(np.rint(q.astype(np.float64) * 255), np.arange(256))


def test_quotients_are_injective_in_every_storage_type():
    """what lets the geometry tests compare bytes: the 256 outputs of the mask configuration stay distinct and ordered in
    fp32, fp16 and bf16, and decode_bytes inverts them (and flags everything else)"""
    for kind in ("fp32", "bf16", "fp16"):
        t = PC.quotient_table(kind)
        assert t.dtype == np.float32 and np.all(np.diff(t) > 0), kind
        assert t[0] == 0.0 and t[255] == 1.0
        assert np.array_equal(PC.decode_bytes(t[::-1].reshape(16, 16), kind), np.arange(255, -1, -1).reshape(16, 16))
        off = np.array([-1.0, 0.5 * (t[3] + t[4]), 2.0, np.nan, np.nextafter(t[200], np.float32(2))], np.float32)
        assert PC.decode_bytes(off, kind).tolist() == [-1] * 5
    assert np.array_equal(PC.bf16_bits_to_f32(PC.round_bf16_bits(PC.quotient_table("fp32"))), PC.quotient_table("bf16"))


def test_bf16_rounding_is_to_nearest_even():
    f = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20, -(1.0 + 3 * 2.0 ** -8), 0.0], np.float32)
    got = PC.bf16_bits_to_f32(PC.round_bf16_bits(f))
    assert got.tolist() == [1.0, 1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7, -(1.0 + 2.0 ** -6), 0.0]
    try:
        import torch
    except ImportError:
        return
    r = np.random.default_rng(5).standard_normal(4096).astype(np.float32) * 0.01
    assert np.array_equal(PC.round_bf16_bits(r).view(np.int16), torch.from_numpy(r).to(torch.bfloat16).view(torch.int16).numpy())
