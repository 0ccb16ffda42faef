"""The geometries of the per-block backward parity tests (test_backward_blocks_gpu.py) and a host-side model of the
descriptors csrc/plan.hip builds for them, shared with test_plan_census_cpu.py.

The cases are the smallest geometries whose layers reach the launch regimes the golden cases (32x32 ... 64x64) never
reach on the backward side: the 128 x 64 and 256 x 32 tiles with the BatchNorm-backward loader, the persistent
multi-item loop (items > grid) and stacked-rows tiling without a K-split. `descriptors()` restates the ARCHITECTURE only
(32/64/128/256/512 filters, in_prefix * f + NBF[i+1] inputs, which conv carries which input transform / fused reduce,
the destination split of conv1's input gradient, the per-block K-split workspace); the launch POLICY is never
restated: every regime below comes out of nunet_conv3x3_launch_info / nunet_conv3x3_wgrad_launch_info, and the GPU test
holds this model against the census the plan itself records.

Not covered here, on purpose: the FORWARD multi-item loop, which needs more than 131 072 pixels under today's policy
and stays with test_conv_tiles_gpu.py and the bs16 96x96 tests; and tile 4 (256 x 64), which the policy never chooses."""
import ctypes as C
import functools

import torch
import torch.nn.functional as F

from nunet_amd import _lib as L
from nunet_amd import synth
from oracle import nunet_oracle as O

SEED = 1234

NBF = (32, 64, 128, 256, 512)
SK_MINLEV = 3          # csrc/plan.hip: blocks of levels >= 3 own a K-split workspace of 8 slabs of their widest tensor

# name: (unet, N, H, W, classes, input channels, deep supervision); every case <= ~30 000 level-0 pixels.
# A alone reaches the 128 x 64 and the 256 x 32 input-gradient tiles in both item regimes; B adds stacked rows without a
# K-split, weight-gradient slices of exactly one pixel tile and the four deep-supervision heads; C is the plain U-Net wiring.
# With the plan's REAL K-split workspace (levels 3 and 4 only, 8 slabs) no Nested U-Net level of A or B pairs regular tiling
# with a K-split: that needs a level-3 image too large to pack (more than 64 pixels) under 60 work items. C's 64 x 96 images
# (8 x 12 at level 3, two of them) supply it, forward and backward; 4 x 64 x 64 would not.
CASES = {
    "A": (False, 3, 80, 112, 1, 3, False),
    "B": (False, 7, 48, 48, 4, 1, True),
    "C": (True, 2, 64, 96, 2, 3, False),
}

_token = (C.c_float * 4)()          # the queries compare splitk_ws / bn_y with NULL and never dereference them
_ADDR = C.addressof(_token)


def nodes(unet):
    """(i, j, in_prefix, up_slot, up_j) of every block in the plan's execution order; up_j: the column of the block whose
    output the block up-samples."""
    if not unet:
        return [(s - j, j, j, j - 1 if j else -1, j - 1) for s in range(5) for j in range(s + 1)]
    return [(i, 0, 0, -1, -1) for i in range(5)] + [(i, 4 - i, 1, 0 if i == 3 else 1, 0 if i == 3 else 3 - i) for i in (3, 2, 1, 0)]


def block_cin(i, in_prefix, cin_img):
    if in_prefix == 0:
        return cin_img if i == 0 else NBF[i - 1]
    return in_prefix * NBF[i] + NBF[i + 1]


def descriptors(case, dt):
    """([(label, ConvDesc)] forward, [(label, ConvDesc)] backward, [(label, WgradDesc, WgradDesc)]) as the plan builds them."""
    unet, n, h, w, ncls, cin_img, ds = CASES[case]
    lib = L.lib()
    fwd, bwd, wg = [], [], []

    def conv(i, c0, c1, d0, d1, in_tf, bn_y, sk):
        d = L.ConvDesc()
        d.dtype = dt; d.N = n; d.H = h >> i; d.W = w >> i
        d.C0 = c0; d.P0 = c0; d.C1 = c1; d.P1 = c1
        d.D0 = d0; d.Q0 = d0; d.D1 = d1; d.Q1 = d1
        d.in_tf = in_tf
        if bn_y:
            d.bn_y = _ADDR; d.bn_py = d0
        if sk:
            d.splitk_ws = _ADDR; d.splitk_ws_floats = sk
        return d

    def wgrad(i, c0, c1, cout, other_cinpad):
        cinpad = max(c0 + c1, 32)
        target = 96 if cinpad < other_cinpad else 192
        q = L.WgradDesc()                    # the slab count is fixed at plan creation, from the padded width alone
        q.N = n; q.H = h >> i; q.W = w >> i; q.C0 = cinpad; q.Cout = cout; q.target_wgs = target
        ks = lib.nunet_conv3x3_wgrad_slabs(C.byref(q))
        d = L.WgradDesc()
        d.dtype = dt; d.N = n; d.H = h >> i; d.W = w >> i
        d.C0 = c0; d.P0 = c0; d.C1 = c1; d.P1 = c1; d.Cout = cout; d.PY = cout
        d.slab_stride = 9 * cout * cinpad; d.max_slabs = ks; d.target_wgs = target; d.dw_floats = ks * d.slab_stride
        return d

    for (i, j, pre, up_slot, up_j) in nodes(unet):
        f = NBF[i]
        cin = block_cin(i, pre, cin_img)
        cinpad = max(cin, 32)
        px = n * (h >> i) * (w >> i)
        sk = 8 * px * max(cinpad, f) if i >= SK_MINLEV else 0
        c0, c1 = (cinpad, 0) if pre == 0 else (pre * f, NBF[i + 1])
        lab = "B%d%d." % (i, j)
        fwd.append((lab + "conv1", conv(i, c0, c1, f, 0, L.TF_NONE, False, sk)))
        fwd.append((lab + "conv2", conv(i, f, 0, f, 0, L.TF_BN_RELU, False, sk)))
        d = conv(i, f, 0, f, 0, L.TF_BN_RELU_BWD, True, sk)
        d.P0 = (2 if unet and i < 4 else 1 if unet else 5 - i) * f          # read from the level buffer's slot
        bwd.append((lab + "dgrad2", d))
        if not (i == 0 and pre == 0):
            if pre == 0:
                d = conv(i, f, 0, NBF[i - 1], 0, L.TF_BN_RELU_BWD, False, sk)
            else:
                d = conv(i, f, 0, pre * f, NBF[i + 1], L.TF_BN_RELU_BWD, False, sk)
                d.acc_slot_w = f
            bwd.append((lab + "dgrad1", d))
        wg.append((lab + "wgrad", wgrad(i, c0, c1, f, f), wgrad(i, f, 0, f, cinpad)))
    return fwd, bwd, wg


def conv_info(d):
    o = L.ConvLaunchInfo()
    L.check(L.lib().nunet_conv3x3_launch_info(C.byref(d), C.byref(o)), "nunet_conv3x3_launch_info")
    return o


def wgrad_info(d):
    o = L.WgradLaunchInfo()
    L.check(L.lib().nunet_conv3x3_wgrad_launch_info(C.byref(d), C.byref(o)), "nunet_conv3x3_wgrad_launch_info")
    return o


def tiling_of(o):
    return "stacked-rows" if o.SH else "multi-image" if o.NI > 1 else "regular"


def conv_regime(kind, o):
    """(kind, tile, tiling, split, item regime) of a convolution's launch info; multi-item means items > grid"""
    return (kind, o.tile, tiling_of(o), "S>1" if o.S > 1 else "S=1", "multi-item" if o.items > o.grid else "one-item")


def wgrad_regime(o):
    split = "k=1" if o.ksplit == 1 else "k=nMT" if o.ksplit == o.nMT else "1<k<nMT"
    return ("wgrad", 10 * o.A + o.B, tiling_of(o), split, "-")


def info_fields(o):
    return tuple(getattr(o, k) for k, _ in o._fields_)


def model_regimes(case, dt):
    """the regime set of a case from the descriptor model: {(kind, tile, tiling, split, item regime)}"""
    fwd, bwd, wg = descriptors(case, dt)
    out = {conv_regime("fwd", conv_info(d)) for _, d in fwd}
    out |= {conv_regime("dgrad", conv_info(d)) for _, d in bwd}
    for _, a, b in wg:
        out |= {wgrad_regime(wgrad_info(a)), wgrad_regime(wgrad_info(b))}
    return out


def census_regimes(fwd_entries, bwd_entries):
    """the same set from the plan's own census (Plan.census(False), Plan.census(True))"""
    out = set()
    for kind, entries in (("fwd", fwd_entries), ("dgrad", bwd_entries)):
        for e in entries:
            if e.kind == L.CENSUS_CONV:
                out.add(conv_regime(kind, e.conv))
            else:
                out |= {wgrad_regime(e.wgrad[0]), wgrad_regime(e.wgrad[1])}
    return out


# ---------------------------------------------------------------------------------------------------------------------
# The one-hop scheme: every block's backward evaluated on its own by the oracle, from GIVEN block outputs
# and GIVEN output gradients. Host only; the GPU test feeds it the HIP path's tensors, test_plan_census_cpu.py the
# oracle's own (where the sums must reproduce the end-to-end gradient).
# ---------------------------------------------------------------------------------------------------------------------

def heads_of(case):
    """[(parameter prefix, column of the level-0 block the 1x1 head reads)]"""
    unet, n, h, w, ncls, cin, ds = CASES[case]
    return [("final%d" % k, k) for k in (1, 2, 3, 4)] if ds and not unet else [("final", 4)]


@functools.lru_cache(maxsize=None)
def inputs(case):
    unet, n, h, w, ncls, cin, ds = CASES[case]
    st = synth.closed_form_state_unet(ncls, cin) if unet else synth.closed_form_state(ncls, cin, ds, True)
    img, msk = synth.synth_batch(n, h, w, cin, ncls, seed=SEED)
    return st, torch.from_numpy(img), torch.from_numpy(msk)


def block_input(net, case, feats, img, node):
    """input of block (i, j) from the block outputs in `feats`: image, max-pool or cat(x_{i,0..}, up-sample), with the
    storage roundings of OracleNet.__call__"""
    i, j, pre, up_slot, up_j = node
    if pre == 0:
        if i == 0:
            return img if net.storage is None else img.to(net.storage).to(net.dtype)
        return net._r(F.max_pool2d(feats[(i - 1, 0)], 2, 2))
    up = net._r(F.interpolate(feats[(i + 1, up_j)], scale_factor=2, mode="bilinear", align_corners=True))
    return torch.cat([feats[(i, k)] for k in range(pre)] + [up], 1)


def consumed(node):
    """the blocks whose outputs block `node` reads"""
    i, j, pre, up_slot, up_j = node
    if pre == 0:
        return [(i - 1, 0)] if i else []
    return [(i, k) for k in range(pre)] + [(i + 1, up_j)]


def head_logits(net, case, feats):
    return [F.conv2d(feats[(0, col)], net.params[p + ".weight"], net.params[p + ".bias"]) for p, col in heads_of(case)]


def end_to_end(case, dtype, backward):
    """the oracle on the case's wiring: block outputs (with .grad when `backward`), logits, the net (its BN buffers updated)"""
    unet, n, h, w, ncls, cin, ds = CASES[case]
    st, img, msk = inputs(case)
    net = O.OracleNet(st, ncls, cin, ds and not unet, dtype=dtype)
    feats = {}
    with torch.set_grad_enabled(backward):
        for node in nodes(unet):
            feats[node[:2]] = net._block(block_input(net, case, feats, img.to(dtype), node), node[0], node[1])
            if backward:
                feats[node[:2]].retain_grad()
        logits = head_logits(net, case, feats)
        if backward:
            for x in logits:
                x.retain_grad()
            O.criterion_ds(logits if len(logits) > 1 else logits[0], msk.to(dtype))[0].backward()
    return feats, logits, net


# A ReLU decision the working precision cannot make. The hop recomputes z = bn(conv(x)) from the block's inputs, and the path
# under test took its decisions z > 0 on ITS fp32 evaluation of the same z: an fp32 dot product of K <= 9 * 1024 terms carries
# a rounding error of the order sqrt(K) * 2^-24 = 6e-6 of the largest |z|, so for |z| below AMBIGUOUS = 1e-5 of the tensor's
# largest |z| either decision is a correct fp32 result - and taking the other one moves that pixel's gradient by its whole
# value (1 / sqrt(pixels) of a weight-gradient row: 1e-2 at 7 000 pixels), far above any per-tensor bound. Inside that band,
# and only there, the hop takes the decision the path under test stored (`masks`); everywhere else the oracle's own stands,
# so a wrong decision outside the band still shows.
AMBIGUOUS = 1e-5


class _HopNet(O.OracleNet):
    """OracleNet whose ReLUs defer to given decisions inside the AMBIGUOUS band. masks: {(prefix, k): bool tensor} or None;
    deferred counts the elements where that changed the decision."""
    masks = None
    deferred = 0

    def _conv_bn_relu(self, x, prefix, k):
        given = None if self.masks is None else self.masks.get((prefix, k))
        if given is None:
            return super()._conv_bn_relu(x, prefix, k)
        assert self.storage is None
        y = F.conv2d(x, self.params["%sconv%d.weight" % (prefix, k)], self.params["%sconv%d.bias" % (prefix, k)], padding=1)
        z = F.batch_norm(y, self.buffers["%sbn%d.running_mean" % (prefix, k)], self.buffers["%sbn%d.running_var" % (prefix, k)],
                         self.params["%sbn%d.weight" % (prefix, k)], self.params["%sbn%d.bias" % (prefix, k)], True, O.BN_MOMENTUM, O.BN_EPS)
        zd = z.detach()
        own = zd > 0
        band = zd.abs() < AMBIGUOUS * zd.abs().max()
        take = torch.where(band, given, own)
        self.deferred += int((take != own).sum())
        return z * take.to(z.dtype)


def one_hop(case, feats, grads, dlogits, dtype, storage=None, masks=None, counts=None):
    """Every block's backward on its own: inputs `feats` (block outputs) and output gradients `grads`, both given; the
    heads from `dlogits`. Returns ({slot: sum of its consumers' contributions}, {parameter name: gradient}).
    masks: {("conv<i>_<j>.", k): stored ReLU decisions}, honoured inside the AMBIGUOUS band only (counts["deferred"]: how often)."""
    unet, n, h, w, ncls, cin, ds = CASES[case]
    st, img, msk = inputs(case)
    net = _HopNet(st, ncls, cin, ds and not unet, dtype=dtype, storage=storage)
    net.masks = masks
    slot = {}

    def hand_back(leaves):
        for k, leaf in leaves.items():
            slot[k] = leaf.grad if k not in slot else slot[k] + leaf.grad

    for node in nodes(unet):
        leaves = {k: feats[k].to(dtype).clone().requires_grad_(True) for k in consumed(node)}
        out = net._block(block_input(net, case, leaves, img.to(dtype), node), node[0], node[1])
        out.backward(grads[node[:2]].to(dtype))
        hand_back(leaves)
    for (p, col), dl in zip(heads_of(case), dlogits):
        leaves = {(0, col): feats[(0, col)].to(dtype).clone().requires_grad_(True)}
        F.conv2d(leaves[(0, col)], net.params[p + ".weight"], net.params[p + ".bias"]).backward(dl.to(dtype))
        hand_back(leaves)
    if counts is not None:
        counts["deferred"] = net.deferred
    return slot, {nm: p.grad for nm, p in net.params.items()}


def rel_err(got, want):
    """(max-norm error relative to the expected tensor's largest magnitude, relative L2 error)"""
    d = got.double() - want.double()
    return (float(d.abs().max()) / (float(want.abs().max()) + 1e-300), float(d.norm()) / (float(want.norm()) + 1e-300))
