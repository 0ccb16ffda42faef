"""Backward pass of the whole-network plan, one block at a time, against fp64 ("one hop at a time").

What is under test is the COMPOSITION in csrc/plan.hip: which launch regime every layer gets (tests/block_cases.py), the
accumulate masks and `written` bookkeeping of the dense skip connections, the split of conv1's input gradient into
level-buffer slots and the up-sample scratch, the pool / up-sample backward and their accumulate flags, the per-block
scratch offsets and the weight-gradient slab counts - at geometries whose layers run the 128 x 64 and 256 x 32
input-gradient tiles, the persistent multi-item loop, stacked rows and K-splits.

An end-to-end per-element bound cannot see a kernel bug here: the gradient through 30 stacked BatchNorm layers is
ill-conditioned, and the reference arithmetic itself (the oracle in fp32) sits percents away from fp64 per element
(re-measured and printed by test_fp32_backward_one_hop for case A). So every block is checked on its own, from the HIP
path's own tensors: block (i, j) is fed, in fp64, the HIP path's stored inputs and the HIP path's dL/dx_{i,j}
(Plan.feature / Plan.feature_grad), one VGGBlock backward (plus its pool / up-sample / concat) is evaluated, and what it
hands to its input slots and its parameter gradients is compared. In fp64 the sum of these one-hop contributions
reproduces the end-to-end gradient of every slot to ~1e-15.

Bounds. fp32: per tensor max(4 x e_ref, 1e-4), in max-norm relative to the expected tensor's largest magnitude and in
relative L2; e_ref is the same one-hop evaluation by the oracle in fp32 (the reference's arithmetic) against fp64 on the
same inputs; factor and floor are those of test_net_gpu.py. Both evaluations take the ReLU decisions of the pass inside the
band where fp32 cannot make them, and only there (block_cases.AMBIGUOUS). 16-bit: the project's storage-emulation yardstick, per hop:
relative L2 <= 1.5 x e_emu + 0.02 per tensor and median <= 1.2 x median(e_emu) + 0.01, e_emu the one-hop oracle with
storage= that type against the unrounded fp64 hop."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import nunet_amd  # noqa: E402
from nunet_amd import _lib as L  # noqa: E402
from oracle import nunet_oracle as O  # noqa: E402
import block_cases as B  # noqa: E402
from test_net_gpu import DEV, run_step  # noqa: E402

STORAGE = {"bf16": torch.bfloat16, "fp16": torch.float16}


@pytest.fixture(autouse=True)
def _canaries(guard_bands):
    """the arenas and every other device buffer of the step sit between guard bands that are checked after the test"""
    yield


def pre_bn_bias(nm):
    return nm.endswith("conv1.bias") or nm.endswith("conv2.bias")


@functools.lru_cache(maxsize=None)
def oracle64(case):
    """the fp64 oracle end to end: (block outputs, BN buffers after the step); case A with its backward pass, for the figures
    test_fp32_backward_one_hop prints (the outputs then carry .grad)"""
    feats, logits, net = B.end_to_end(case, torch.float64, case == "A")
    return feats, net.buffers


@functools.lru_cache(maxsize=None)
def hip_step(case, dtype):
    """one train() step of the eager module path; everything the assertions need, read back to the host"""
    unet, n, h, w, ncls, cin, ds = B.CASES[case]
    st, img, msk = B.inputs(case)
    cls = nunet_amd.archs.UNet if unet else nunet_amd.archs.NestedUNet
    m = cls(ncls, cin, ds, dtype=dtype)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in st.items()})
    m = m.to(DEV).train()
    out, loss, iou = run_step(m, img, msk, ds and not unet)
    torch.cuda.synchronize()
    pl = m.plan_for(img.to(DEV))
    r = {"feats": {}, "grads": {}, "masks": {}}
    for node in B.nodes(unet):
        k = node[:2]
        r["feats"][k] = pl.feature(*k).permute(0, 3, 1, 2).cpu().double().contiguous()
        r["grads"][k] = pl.feature_grad(*k).permute(0, 3, 1, 2).cpu().double().contiguous()
        if dtype == "fp32":   # the ReLU decisions the pass took: a1 > 0 and x_{i,j} > 0 (block_cases.AMBIGUOUS)
            r["masks"][("conv%d_%d." % k, 1)] = pl.block_act1(*k).permute(0, 3, 1, 2).cpu() > 0
            r["masks"][("conv%d_%d." % k, 2)] = r["feats"][k] > 0
    r["logits"] = [o.detach().cpu() for o in (out if isinstance(out, (list, tuple)) else [out])]
    r["pgrads"] = {nm: p.grad.detach().cpu().double() for nm, p in m.named_parameters()}
    r["state"] = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    r["census"] = (pl.census(False), pl.census(True))
    # dL/dlogits in fp64 from the HIP logits, through the reference's loss (the mean over the heads under deep supervision)
    lg = [o.double().clone().requires_grad_(True) for o in r["logits"]]
    O.criterion_ds(lg if len(lg) > 1 else lg[0], msk.double())[0].backward()
    r["dlogits"] = [x.grad for x in lg]
    return r


@functools.lru_cache(maxsize=None)
def hops(case, dtype):
    """the one-hop evaluations on the HIP path's tensors: exact (fp64), and the yardstick's (fp32 arithmetic for the fp32
    leg, fp64 with 16-bit storage points for the 16-bit legs; its slot sums rounded once to the slot's storage type)"""
    r = hip_step(case, dtype)
    masks, counts = (r["masks"], {}) if dtype == "fp32" else (None, None)
    exact = B.one_hop(case, r["feats"], r["grads"], r["dlogits"], torch.float64, masks=masks, counts=counts)
    if dtype == "fp32":
        print("case %s fp32: %d ReLU decisions inside the ambiguous band taken from the pass" % (case, counts["deferred"]))
        ref = B.one_hop(case, r["feats"], r["grads"], r["dlogits"], torch.float32, masks=masks)
    else:
        sl, pg = B.one_hop(case, r["feats"], r["grads"], r["dlogits"], torch.float64, storage=STORAGE[dtype])
        ref = ({k: v.to(STORAGE[dtype]).double() for k, v in sl.items()}, pg)
    return exact, ref


def tensors(case, dtype):
    """[(name, HIP tensor, exact one-hop tensor, yardstick one-hop tensor)]: every gradient slot, every parameter gradient
    but the conv biases in front of a BatchNorm"""
    r = hip_step(case, dtype)
    (slot64, pg64), (slot_ref, pg_ref) = hops(case, dtype)
    blocks = [node[:2] for node in B.nodes(B.CASES[case][0])]
    assert sorted(slot64) == sorted(blocks), "a block output without a consumer (or a consumer of no block)"
    out = [("dL/dx%d_%d" % k, r["grads"][k], slot64[k], slot_ref[k]) for k in blocks]
    assert list(r["pgrads"]) == list(pg64)
    out += [(nm, g, pg64[nm], pg_ref[nm]) for nm, g in r["pgrads"].items() if not pre_bn_bias(nm)]
    return out


def print_census(case, dtype, census):
    for name, entries in zip(("forward", "backward"), census):
        for e in entries:
            if e.kind == L.CENSUS_CONV:
                o = e.conv
                print("census %s %s %-8s %-12s tile %d %-12s S %2d items %4d grid %4d acc0 %x" % (
                    case, dtype, name, e.label.decode(), o.tile, B.tiling_of(o), o.S, o.items, o.grid, e.acc0_mask))
            else:
                print("census %s %s %-8s %-12s %s" % (case, dtype, name, e.label.decode(), " | ".join(
                    "%dx%d %-12s nMT %3d ksplit %3d grid %3d" % (32 * o.A, 32 * o.B, B.tiling_of(o), o.nMT, o.ksplit, o.grid) for o in e.wgrad)))


def check_census(case, dtype):
    """the plan's own census against the descriptor model of block_cases.py: label by label, and as regime sets"""
    dt = L.DTYPES[dtype]
    cf, cb = hip_step(case, dtype)["census"]
    fwd, bwd, wg = B.descriptors(case, dt)
    model = {lab: B.info_fields(B.conv_info(d)) for lab, d in fwd + bwd}
    model.update({lab: B.info_fields(B.wgrad_info(a)) + B.info_fields(B.wgrad_info(b)) for lab, a, b in wg})
    mine = {}
    for e in cf + cb:
        lab = e.label.decode()
        assert lab not in mine, lab
        mine[lab] = B.info_fields(e.conv) if e.kind == L.CENSUS_CONV else B.info_fields(e.wgrad[0]) + B.info_fields(e.wgrad[1])
    assert sorted(mine) == sorted(model)
    for lab in model:
        assert mine[lab] == model[lab], (lab, mine[lab], model[lab])
    assert B.census_regimes(cf, cb) == B.model_regimes(case, dt)


@pytest.mark.parametrize("case", list(B.CASES))
def test_fp32_census_matches_the_model(case):
    print_census(case, "fp32", hip_step(case, "fp32")["census"])
    check_census(case, "fp32")
    if case == "A":      # what no fp32 per-element check reached before
        regimes = B.census_regimes(*hip_step(case, "fp32")["census"])
        for tile in (2, 3):
            assert ("dgrad", tile, "regular", "S=1", "multi-item") in regimes


@pytest.mark.parametrize("case", list(B.CASES))
def test_fp32_forward_matches_the_fp64_oracle(case):
    r = hip_step(case, "fp32")
    feats, buffers = oracle64(case)
    worst = (0.0, None)
    for k, f in feats.items():
        f = f.detach()
        err = float((r["feats"][k] - f).abs().max() / f.abs().max())
        worst = max(worst, (err, k))
        assert err < 2e-4, (k, err)
    print("case %s fp32 forward: worst feature error %.2e of the tensor's max at x%d_%d" % ((case, worst[0]) + worst[1]))
    for nm, b in buffers.items():
        if nm.endswith("num_batches_tracked"):
            assert int(r["state"][nm]) == int(b), nm
        else:
            np.testing.assert_allclose(r["state"][nm].double().numpy(), b.numpy(), rtol=2e-4, atol=2e-6, err_msg=nm)


@pytest.mark.parametrize("case", list(B.CASES))
def test_fp32_backward_one_hop(case):
    """The hop takes the ReLU decisions of the pass (a1 > 0, x_{i,j} > 0) where, and only where, fp32 cannot make them
    (block_cases.AMBIGUOUS). Without that, cases A and B missed the bound by two orders of magnitude on the handful of tensors
    downstream of such an element (A: conv1_1.conv1.weight 1.86e-2 in max-norm against a reference fp32 error of 1.92e-6,
    conv1_1.bn1.bias 1.08e-2; B: conv2_2.conv2.weight 1.58e-2) with every other tensor at 1e-6: one pixel of dz moved by its
    whole value is 1 / sqrt(pixels) of a weight-gradient row. Two fp32 evaluations of the oracle that differ only in the order
    the input channels are summed miss each other in the same way on the CPU (worst 43 x the bound), and agree at 0.05 x the
    bound once 7 decisions inside the band are shared. Measured on the MI355X: 4 (A), 3 (B), 0 (C) decisions taken from the
    pass, worst error / bound 0.026, 0.023, 0.020."""
    r = hip_step(case, "fp32")
    if case == "A":
        # why not end to end: the reference's own arithmetic against fp64, per element, on dL/dx_{i,j}
        f64, f32 = oracle64(case)[0], B.end_to_end(case, torch.float32, True)[0]
        e2e = [B.rel_err(f32[k].grad, f64[k].grad)[0] for k in f64]
        print("case A end-to-end dL/dx_{i,j}, fp32 oracle vs fp64, max-norm: median %.2e max %.2e" % (float(np.median(e2e)), max(e2e)))
    for nm, g in r["pgrads"].items():
        if pre_bn_bias(nm):
            assert float(g.abs().max()) < 1e-4, nm
    bad, worst = [], (0.0, None, 0.0, 0.0)
    for nm, mine, want, ref in tensors(case, "fp32"):
        e_hip, e_ref = B.rel_err(mine, want), B.rel_err(ref, want)
        for kind, eh, er in zip(("max", "L2"), e_hip, e_ref):
            bound = max(4 * er, 1e-4)
            worst = max(worst, (eh / bound, nm + " " + kind, eh, er))
            if not eh <= bound:
                bad.append((nm, kind, eh, er))
    print("case %s fp32 one-hop: worst error / bound %.3f at %s (error %.2e, reference fp32 error %.2e)" % ((case,) + worst))
    for nm, kind, eh, er in bad:
        print("case %s fp32 one-hop OVER ITS BOUND: %-28s %-3s error %.2e, reference fp32 error %.2e" % (case, nm, kind, eh, er))
    assert not bad, "%d tensor figures over max(4 x e_ref, 1e-4), first: %s" % (len(bad), bad[0])


@pytest.mark.parametrize("case,dtype", [("A", "bf16"), ("B", "bf16"), ("A", "fp16")])
def test_16bit_backward_one_hop(case, dtype):
    r = hip_step(case, dtype)
    print_census(case, dtype, r["census"])
    check_census(case, dtype)
    for nm, g in r["pgrads"].items():
        if pre_bn_bias(nm):
            assert float(g.abs().max()) == 0.0, nm
    e_hip, e_emu = {}, {}
    for nm, mine, want, emu in tensors(case, dtype):
        e_hip[nm], e_emu[nm] = B.rel_err(mine, want)[1], B.rel_err(emu, want)[1]
    med = lambda d: float(np.median(list(d.values())))
    worst = max(e_hip, key=lambda k: e_hip[k] / (1.5 * e_emu[k] + 0.02))
    print("case %s %s one-hop rel-L2: HIP max %.2e median %.2e, %s-storage oracle max %.2e median %.2e; worst error / bound %.3f at %s "
          "(%.2e vs %.2e)" % (case, dtype, max(e_hip.values()), med(e_hip), dtype, max(e_emu.values()), med(e_emu),
                              e_hip[worst] / (1.5 * e_emu[worst] + 0.02), worst, e_hip[worst], e_emu[worst]))
    bad = [(nm, e_hip[nm], e_emu[nm]) for nm in e_hip if not e_hip[nm] <= 1.5 * e_emu[nm] + 0.02]
    assert not bad, bad
    assert med(e_hip) <= 1.2 * med(e_emu) + 0.01
