"""Full-resolution tiled inference: masks and metrics at the images' own sizes.

The reference's val.py squeezes every image to input_h x input_w. The network is fully convolutional, so an image of any size
can instead be cut into overlapping input_h x input_w windows, each window run through the fixed-shape captured forward, and
the windows' logits blended back into a mask of the source's size. The geometry is defined here, once, and restated by the
kernels (include/nunet.h: nunet_crop_tiles_u8, nunet_plan_stage_u8_tiles, nunet_stitch_tiles); tests/tile_cases.py is its oracle.

Along one axis, source extent S, tile extent T, overlap O with 0 <= O <= T/2:
  origins     S <= T: one tile at 0. Otherwise stride = T - O, n = ceil((S - T) / stride) + 1, origin(j) = min(j * stride, S - T):
              the last tile is flush with the edge, nothing is padded when S >= T, no coordinate lies in more than 3 tiles.
  reflection  (a source smaller than the tile: rows / columns at or past S) BORDER_REFLECT_101, repeated: S == 1 gives 0;
              otherwise p = 2(S - 1), m = i mod p, the index is m if m < S else p - m. Equals np.pad(mode='reflect').
  window      separable, 'tent' w[i] = min(i + 1, T - i) or 'uniform' w[i] = 1; a pixel's weight in a tile is the integer
              product wy * wx as fp32, its blended logit sum(w_t * l_t) / sum(w_t) in ascending tile index. A pixel one tile
              covers takes that tile's logit unchanged."""
import ctypes as C
from collections import OrderedDict

import numpy as np
import torch

from . import _lib as L
from .dataset import MEAN, STD, check_descriptors

WINDOWS = {"tent": L.WINDOW_TENT, "uniform": L.WINDOW_UNIFORM}


# -- geometry ------------------------------------------------------------------------------------------------------------------
def check_overlap(tile_hw, overlap):
    """the overlap both axes share: an integer in 0 .. min(Th, Tw) / 2 (beyond it a coordinate could lie in more than 3 tiles)"""
    th, tw = tile_hw
    if isinstance(overlap, bool) or not isinstance(overlap, (int, np.integer)):
        raise L.NunetError("tile overlap must be an integer, got %r" % (overlap,))
    if not 0 <= 2 * int(overlap) <= min(th, tw):
        raise L.NunetError("tile overlap %d: 0 .. %d (half the tile's smaller side, %d x %d)" % (overlap, min(th, tw) // 2, th, tw))
    return int(overlap)


def axis_grid(S, T, O):
    """(number of tiles, stride) along one axis"""
    stride = T - O
    return (1 if S <= T else -(-(S - T) // stride) + 1), stride


def tile_origins(S, T, O):
    n, stride = axis_grid(S, T, O)
    return [min(j * stride, max(S - T, 0)) for j in range(n)]


def reflect_index(i, S):
    if S == 1:
        return 0
    p = 2 * (S - 1)
    m = i % p
    return m if m < S else p - m


def blend_window(T, window="tent"):
    if window not in WINDOWS:
        raise L.NunetError("window %r is not one of %s" % (window, sorted(WINDOWS)))
    i = np.arange(T, dtype=np.int64)
    return np.minimum(i + 1, T - i) if window == "tent" else np.ones(T, np.int64)


# -- host tables ---------------------------------------------------------------------------------------------------------------
def build_tables(shapes, tile_hw, overlap, num_classes):
    """(tiles int32 [n_tiles,4], grids int32 [n,8], out_elems) for sources of `shapes` [(H, W)]: nunet_tile per tile (sample, y0,
    x0), sample after sample, row-major within a sample; nunet_tile_grid per sample, its [K][H][W] block behind the previous
    sample's in the outputs, every block starting at a multiple of 4 elements (16-byte aligned logits, 4-byte aligned bytes:
    what nunet_sigmoid_u8 and vector loads ask of a view)."""
    th, tw = tile_hw
    overlap = check_overlap(tile_hw, overlap)
    tiles, grids = [], np.zeros((len(shapes), L.GRID_WORDS), np.int32)
    off = 0
    for n, (h, w) in enumerate(shapes):
        oy, ox = tile_origins(int(h), th, overlap), tile_origins(int(w), tw, overlap)
        grids[n:n + 1].view(np.int64)[0, 0] = off
        grids[n, 2:7] = (len(tiles), len(oy), len(ox), th - overlap, tw - overlap)
        tiles += [(n, y0, x0, 0) for y0 in oy for x0 in ox]
        off += (num_classes * int(h) * int(w) + 3) // 4 * 4
    return np.asarray(tiles, np.int32).reshape(-1, L.TILE_WORDS), grids, off


def _host_table(a, words, what):
    if isinstance(a, torch.Tensor):
        if a.is_cuda:
            raise L.NunetError("%s are validated on the host: pass a host array" % what)
        a = a.numpy()
    a = np.asarray(a)
    if a.dtype != np.int32 or a.ndim != 2 or a.shape[1] != words:
        raise L.NunetError("%s must be int32 [n,%d], got %s %s" % (what, words, a.dtype, tuple(a.shape)))
    return np.ascontiguousarray(a)


def check_tiles(tiles, shapes):
    """Refuse, before any launch, a tile table that is not int32 [n,4], names a sample outside `shapes` [(H, W)] (a null tile,
    sample < 0, is fine) or starts outside its source."""
    tiles = _host_table(tiles, L.TILE_WORDS, "tile tables")
    for t, (s, y0, x0, _) in enumerate(tiles):
        if s < 0:
            continue
        if s >= len(shapes):
            raise L.NunetError("tile %d: sample %d of %d" % (t, s, len(shapes)))
        h, w = shapes[s]
        if not (0 <= y0 < h and 0 <= x0 < w):
            raise L.NunetError("tile %d: origin (%d, %d) lies outside its %d x %d source" % (t, y0, x0, h, w))
    return tiles


def check_grids(grids, shapes, n_tiles, tile_hw, num_classes, out_elems, tiles=None):
    """Refuse, before any launch, grids that are not int32 [n,8] with one entry per source, have ny / nx / a stride < 1, tiles
    outside the store of n_tiles, a stride that leaves gaps or more than 3 tiles on a coordinate, a last tile short of the
    source's edge, an output block outside 0 .. out_elems or over another sample's - and, given the tile table, tiles that are
    not where the grid says."""
    th, tw = tile_hw
    grids = _host_table(grids, L.GRID_WORDS, "tile grids")
    if grids.shape[0] != len(shapes):
        raise L.NunetError("tile grids: %d entries for %d sources" % (grids.shape[0], len(shapes)))
    offs = grids.view(np.int64)[:, 0]
    blocks = []
    for n, (h, w) in enumerate(shapes):
        first, ny, nx, sy, sx = (int(v) for v in grids[n, 2:7])
        if ny < 1 or nx < 1 or sy < 1 or sx < 1:
            raise L.NunetError("grid %d: ny=%d nx=%d stride_y=%d stride_x=%d must be positive" % (n, ny, nx, sy, sx))
        if first < 0 or first + ny * nx > n_tiles:
            raise L.NunetError("grid %d: tiles %d .. %d lie outside the store of %d tiles" % (n, first, first + ny * nx, n_tiles))
        for nm, S, T, cnt, st in (("y", int(h), th, ny, sy), ("x", int(w), tw, nx, sx)):
            if st > T or 2 * st < T:
                raise L.NunetError("grid %d: stride_%s=%d of a tile extent %d: %d .. %d" % (n, nm, st, T, (T + 1) // 2, T))
            if (cnt - 1) * st < max(S - T, 0) or (cnt > 1 and (cnt - 2) * st >= S - T):
                raise L.NunetError("grid %d: %d tiles of stride %d along %s do not end flush with a source extent of %d (tile %d)"
                                   % (n, cnt, st, nm, S, T))
        size = num_classes * int(h) * int(w)
        if offs[n] < 0 or offs[n] + size > out_elems:
            raise L.NunetError("grid %d: output elements %d .. %d lie outside 0 .. %d" % (n, offs[n], offs[n] + size, out_elems))
        blocks.append((int(offs[n]), int(offs[n]) + size, n))
        if tiles is not None:
            want = [(n, min(j * sy, max(int(h) - th, 0)), min(i * sx, max(int(w) - tw, 0))) for j in range(ny) for i in range(nx)]
            got = [tuple(int(v) for v in r[:3]) for r in tiles[first:first + ny * nx]]
            if got != want:
                raise L.NunetError("grid %d: the tile table's entries %d .. %d are not the grid's tiles" % (n, first, first + ny * nx))
    blocks.sort()
    for a, b in zip(blocks, blocks[1:]):
        if b[0] < a[1]:
            raise L.NunetError("grids %d and %d: their output blocks overlap" % (a[2], b[2]))
    return grids


def check_source_group(pool, desc, channels, capacity=None, n=None, what="image"):
    """One group of ragged sources as predict() takes it: a flat uint8 pool of at most `capacity` bytes (None: no bound) and host
    descriptors that dataset.check_descriptors accepts for `channels` channels."""
    if not isinstance(pool, torch.Tensor) or pool.dtype != torch.uint8 or pool.dim() != 1:
        raise L.NunetError("predict: the %s pool must be a flat uint8 tensor (dataset.pack_ragged)" % what)
    if capacity is not None and pool.numel() > capacity:
        raise L.NunetError("predict: the %s pool holds %d bytes, this TiledPredictor was built with source_capacity=%d"
                           % (what, pool.numel(), capacity))
    check_descriptors(desc, pool.numel(), channels, n)


def _shapes_of(desc):
    d = desc.numpy() if isinstance(desc, torch.Tensor) else np.asarray(desc)
    return [(int(h), int(w)) for h, w in d[:, 2:4]]


def batch_tables(tiles, n):
    """The per-replay tables of a tile table run n tiles at a time: (tile tables int32 [B,n,4], sample maps int64 [B,n]). Batch
    b's tiles name their samples by position in its own sample table, whose row r is sample maps[b, r] of the call (-1: unused,
    an all-zero descriptor); the last batch is filled with null tiles (sample -1)."""
    nt = tiles.shape[0]
    nb = -(-nt // n)
    bt = np.zeros((nb, n, L.TILE_WORDS), np.int32)
    bt[:, :, 0] = -1
    smap = np.full((nb, n), -1, np.int64)
    for b in range(nb):
        part = tiles[b * n:(b + 1) * n]
        local = {}
        for r, (s, y0, x0, _) in enumerate(part):
            if s >= 0:
                bt[b, r] = (local.setdefault(int(s), len(local)), y0, x0, 0)
        for s, r in local.items():
            smap[b, r] = s
    return bt, smap


# -- kernels -------------------------------------------------------------------------------------------------------------------
def crop_tiles_u8(pool, desc, tiles, channels, tile_hw):
    """nunet_crop_tiles_u8: device pool (flat uint8), device descriptors int32 [n,4], device tile table int32 [N,4] -> uint8
    [N,Th,Tw,C]. The tables are the caller's to validate (check_descriptors, check_tiles); the kernel trusts none."""
    for t, dt, nm in ((pool, torch.uint8, "pool"), (desc, torch.int32, "descriptors"), (tiles, torch.int32, "tile table")):
        L.require_gpu_tensor(t, dt, nm)
    th, tw = tile_hw
    out = torch.empty((tiles.shape[0], th, tw, channels), dtype=torch.uint8, device=pool.device)
    L.check(L.lib().nunet_crop_tiles_u8(L.ptr(pool), pool.numel(), L.ptr(desc), desc.shape[0], L.ptr(tiles), tiles.shape[0], channels, th, tw,
                                        L.ptr(out), L.stream()), "nunet_crop_tiles_u8")
    return out


def stitch_tiles(tile_logits, desc, grids, out_elems, window="tent", want_logits=True, want_u8=True):
    """nunet_stitch_tiles: device fp32 [n_tiles,K,Th,Tw], device descriptors [n,4] and grids [n,8] -> (flat fp32 [out_elems] or
    None, flat uint8 [out_elems] or None)."""
    from .metrics import sigmoid_u8_thresholds
    L.require_gpu_tensor(tile_logits, torch.float32, "tile logits")
    L.require_gpu_tensor(desc, torch.int32, "descriptors")
    L.require_gpu_tensor(grids, torch.int32, "tile grids")
    if window not in WINDOWS:
        raise L.NunetError("window %r is not one of %s" % (window, sorted(WINDOWS)))
    if tile_logits.dim() != 4 or tuple(grids.shape) != (desc.shape[0], L.GRID_WORDS) or desc.shape[1] != L.SAMPLE_WORDS:
        raise L.NunetError("stitch_tiles: tile logits [n_tiles,K,Th,Tw], descriptors [n,4] and grids [n,8] expected")
    nt, k, th, tw = tile_logits.shape
    dev = tile_logits.device
    lo = torch.empty(out_elems, dtype=torch.float32, device=dev) if want_logits else None
    u8 = torch.empty(out_elems, dtype=torch.uint8, device=dev) if want_u8 else None
    thr = sigmoid_u8_thresholds(dev) if want_u8 else None
    L.check(L.lib().nunet_stitch_tiles(L.ptr(tile_logits), nt, k, th, tw, L.ptr(desc), L.ptr(grids), desc.shape[0], WINDOWS[window], L.ptr(thr),
                                       L.ptr(lo), L.ptr(u8), out_elems, L.stream()), "nunet_stitch_tiles")
    return lo, u8


# -- the driver ----------------------------------------------------------------------------------------------------------------
class TiledPredictor:
    """Masks at the sources' own sizes from one captured graph of the tile's shape.

    tile_shape = (N, Cin, Th, Tw): the predictor owns a Plan of N x Th x Tw (as EvalStep's batches do) and captures ONE graph:
    nunet_plan_stage_u8_tiles (N windows cut out of a static pool buffer of source_capacity bytes, through a static sample table
    and a static tile table, normalised as the val transform normalises) followed by the eval forward on the weights one
    nunet_plan_repack per predict() left in the plan's arena. use_graph=False issues the same launches eagerly.

    overlap (default min(Th, Tw) // 4) and window ('tent' / 'uniform'): the geometry of this module. depth= and weights= mean
    what they mean for EvalStep and get the same checks; under deep supervision the LAST head is the one stitched (reference
    val.py:92-93).

    predict(pool, desc, mask_pool=None, mask_desc=None) takes one group of ragged sources (dataset.pack_ragged: flat uint8 pool,
    host descriptors) of at most source_capacity bytes. It builds the tile tables on the host and checks them, runs the tiles N at
    a time - EVERY replay is a full batch of N, the last one filled with null tiles, not a smaller plan: the K-split of
    grid-starved layers depends on N, so a full batch keeps a tile's logits independent of how many tiles its image has - copies
    each batch's last-head logits into a tile store sized for the call, and stitches once. It returns an OrderedDict: `logits`
    (per image fp32 [K,H,W] views of one flat device buffer), `masks` (per image uint8 [K,H,W] views, the bytes of
    metrics.sigmoid_masks_u8 of the logits), `tiles` (tiles per image). With masks (uint8 [H,W,K] per image, packed alike;
    target = byte > 127, prediction rule metrics.iou_logit_threshold()) also `iou`, `dice`, `acc` (per image, the reference's
    formulas on that image alone), `counts` (dataset-level tp / fp / fn / tn per class) and `per_class`
    (metrics.scores_from_counts of them).

    NunetError before any launch: a group over source_capacity, a channel count other than the model's, host-visible bad
    descriptors."""

    def __init__(self, model, tile_shape, overlap=None, window="tent", use_graph=True, source_capacity=None, depth=None, weights=None):
        from .engine import Plan
        from .metrics import iou_logit_threshold
        if depth is not None:
            model.check_depth(depth, need_eval=False)
        self.model, self.depth = model, depth
        self.eng = model.engine()
        self.flat_params, self.bnbuf = self.eng.flat_params, self.eng.bnbuf
        if weights is not None:
            if not isinstance(weights, (tuple, list)) or len(weights) != 2:
                raise L.NunetError("TiledPredictor: weights must be a (flat_params, bnbuf) pair of device tensors")
            fp, bb = weights
            for t, like, nm in ((fp, self.eng.flat_params, "flat_params"), (bb, self.eng.bnbuf, "bnbuf")):
                if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() != 1 or not t.is_contiguous():
                    raise L.NunetError("TiledPredictor: weights %s must be a flat contiguous fp32 tensor" % nm)
                if t.numel() != like.numel():
                    raise L.NunetError("TiledPredictor: weights %s has %d values, the model's arena %d" % (nm, t.numel(), like.numel()))
                if t.device != like.device:
                    raise L.NunetError("TiledPredictor: weights %s lives on %s, the model on %s" % (nm, t.device, like.device))
            self.flat_params, self.bnbuf = fp, bb
        n, cin, th, tw = tile_shape
        if cin != model.input_channels:
            raise L.NunetError("TiledPredictor: tile_shape has %d channels, the model takes %d" % (cin, model.input_channels))
        self.n, self.cin, self.th, self.tw = n, cin, th, tw
        self.ncls = model.num_classes
        if self.ncls > L.EVAL_MAX_CLASSES:
            raise L.NunetError("TiledPredictor: %d classes, the metrics take up to %d" % (self.ncls, L.EVAL_MAX_CLASSES))
        self.overlap = check_overlap((th, tw), min(th, tw) // 4 if overlap is None else overlap)
        if window not in WINDOWS:
            raise L.NunetError("TiledPredictor: window %r is not one of %s" % (window, sorted(WINDOWS)))
        self.window = window
        if source_capacity is None or int(source_capacity) < 1:
            raise L.NunetError("TiledPredictor: needs source_capacity, the bytes of the largest group of sources one predict() takes: "
                               "the captured graph reads a static pool of that size")
        self.source_capacity = int(source_capacity)
        self.use_graph = use_graph
        self.iou_thr = iou_logit_threshold()
        dev = self.eng.device
        self.pl = Plan(n, th, tw, cin, self.ncls, getattr(model, "deep_supervision", False), model.compute_dtype, model._unet, dev, depth=depth)
        if self.pl.nparams != self.eng.flat_params.numel() or self.pl.nbnbuf != self.eng.bnbuf.numel() or self.pl.nbn != len(self.eng.bns):
            raise L.NunetError("TiledPredictor: plan/module parameter layout mismatch: %d vs %d params" % (self.pl.nparams, self.eng.flat_params.numel()))
        self.heads = self.pl.heads
        self.pool = torch.zeros(self.source_capacity, dtype=torch.uint8, device=dev)
        self.samples = torch.zeros((n, L.SAMPLE_WORDS), dtype=torch.int32, device=dev)      # nunet_u8_sample of the replay's sources
        self.tiles = torch.zeros((n, L.TILE_WORDS), dtype=torch.int32, device=dev)          # nunet_tile per tile of the replay
        self.tiles[:, 0] = -1
        self.logits = torch.zeros((self.heads, n, self.ncls, th, tw), dtype=torch.float32, device=dev)
        self._mean = torch.tensor(np.resize(np.asarray(MEAN, np.float32), cin), device=dev)
        self._std = torch.tensor(np.resize(np.asarray(STD, np.float32), cin), device=dev)
        self.graph = None

    def _check_engine(self):
        if self.model._engine is not self.eng or not self.eng.intact():
            raise L.NunetError("the module's parameter arenas were re-homed (moved to another device / parameters replaced) "
                               "after this TiledPredictor was built: it would read orphaned memory. Build a new TiledPredictor.")

    def _issue(self):
        """crop + normalise the replay's N tiles into the plan's image, then the eval forward on the packed weights (2 | 4)"""
        lib, pl, st = L.lib(), self.pl, L.stream()
        L.check(lib.nunet_plan_stage_u8_tiles(pl.handle, L.ptr(self.pool), self.source_capacity, L.ptr(self.samples), self.n, L.ptr(self.tiles),
                                              L.ptr(self._mean), L.ptr(self._std), 1.0 / 255.0, L.ptr(pl.arena), L.nbytes(pl.arena), st),
                "plan_stage_u8_tiles")
        L.check(lib.nunet_plan_forward(pl.handle, L.ptr(self.flat_params), L.ptr(self.bnbuf), L.ptr(self.eng.nbt), None, L.ptr(pl.arena),
                                       L.nbytes(pl.arena), L.ptr(self.logits), 2 | 4, st), "plan_forward")
        pl.trained_forward = False

    def tables(self, desc):
        """(tiles [n_tiles,4], grids [n,8], out_elems) of a group's host descriptors, checked"""
        shapes = _shapes_of(desc)
        tiles, grids, out_elems = build_tables(shapes, (self.th, self.tw), self.overlap, self.ncls)
        check_tiles(tiles, shapes)
        check_grids(grids, shapes, tiles.shape[0], (self.th, self.tw), self.ncls, out_elems, tiles)
        return tiles, grids, out_elems

    def predict(self, pool, desc, mask_pool=None, mask_desc=None):
        from .trainer import _NativeGraph
        from .metrics import scores_from_counts, sigmoid_u8_thresholds
        self._check_engine()
        check_source_group(pool, desc, self.cin, self.source_capacity)
        desc_t = torch.as_tensor(desc)
        shapes = _shapes_of(desc_t)
        ns = len(shapes)
        if ns < 1:
            raise L.NunetError("predict: no sources")
        with_masks = mask_pool is not None or mask_desc is not None
        if with_masks:
            if mask_pool is None or mask_desc is None:
                raise L.NunetError("predict: masks come as a pool and its descriptors (dataset.pack_ragged), both or neither")
            check_source_group(mask_pool, mask_desc, self.ncls, None, ns, "mask")
            if _shapes_of(torch.as_tensor(mask_desc)) != shapes:
                raise L.NunetError("predict: the masks' sizes differ from their images'")
        tiles, grids, out_elems = self.tables(desc_t)
        nt = tiles.shape[0]
        bt, smap = batch_tables(tiles, self.n)
        nb = bt.shape[0]
        dnp = np.ascontiguousarray(desc_t.numpy())
        bs = np.zeros((nb, self.n, L.SAMPLE_WORDS), np.int32)
        bs[smap >= 0] = dnp[smap[smap >= 0]]
        dev = self.eng.device
        lib = L.lib()
        # -- everything below launches ---
        self.pool[:pool.numel()].copy_(pool, non_blocking=True)
        d_desc, d_grids = desc_t.to(dev), torch.from_numpy(grids).to(dev)
        d_bt, d_bs = torch.from_numpy(bt).to(dev), torch.from_numpy(bs).to(dev)
        L.check(lib.nunet_plan_repack(self.pl.handle, L.ptr(self.flat_params), L.ptr(self.pl.arena), L.nbytes(self.pl.arena), L.stream()), "plan_repack")
        if self.use_graph and self.graph is None:
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                self._issue()                  # eager once: one-time launch attributes are set outside the capture
            torch.cuda.current_stream().wait_stream(s)
            torch.cuda.synchronize()
            self.graph = _NativeGraph(s, self._issue)
            torch.cuda.synchronize()
        store = torch.empty((nb * self.n, self.ncls, self.th, self.tw), dtype=torch.float32, device=dev)
        for b in range(nb):
            self.samples.copy_(d_bs[b], non_blocking=True)
            self.tiles.copy_(d_bt[b], non_blocking=True)
            if self.graph is not None:
                self.graph.replay()
            else:
                self._issue()
            store[b * self.n:(b + 1) * self.n].copy_(self.logits[-1], non_blocking=True)
        flat = torch.empty(out_elems, dtype=torch.float32, device=dev)
        flat_u8 = torch.empty(out_elems, dtype=torch.uint8, device=dev)
        L.check(lib.nunet_stitch_tiles(L.ptr(store), nb * self.n, self.ncls, self.th, self.tw, L.ptr(d_desc), L.ptr(d_grids), ns, WINDOWS[self.window],
                                       L.ptr(sigmoid_u8_thresholds(dev)), L.ptr(flat), L.ptr(flat_u8), out_elems, L.stream()), "stitch_tiles")
        offs = grids.view(np.int64)[:, 0]
        K = self.ncls
        out = OrderedDict()
        out["logits"] = [flat[int(offs[i]):int(offs[i]) + K * h * w].view(K, h, w) for i, (h, w) in enumerate(shapes)]
        out["masks"] = [flat_u8[int(offs[i]):int(offs[i]) + K * h * w].view(K, h, w) for i, (h, w) in enumerate(shapes)]
        out["tiles"] = [int(g[3]) * int(g[4]) for g in grids]
        if with_masks:
            out.update(self._score(out["logits"], mask_pool, torch.as_tensor(mask_desc), shapes))
            out["per_class"] = scores_from_counts(*out["counts"].values())
        return out

    def _score(self, logits, mask_pool, mask_desc, shapes):
        """nunet_seg_metrics per image on the blended logits (not the hot path): one nunet_seg_sums per image, read together"""
        lib, dev, K = L.lib(), self.eng.device, self.ncls
        mp = mask_pool.to(dev)
        moff = mask_desc.numpy().view(np.int64)[:, 0]
        sz = C.sizeof(L.SegSums)
        sums = torch.zeros(len(shapes) * sz, dtype=torch.uint8, device=dev)
        for i, (h, w) in enumerate(shapes):
            t = (mp[int(moff[i]):int(moff[i]) + h * w * K].view(h, w, K).permute(2, 0, 1) > 127).to(torch.float32).contiguous()
            ws = torch.empty((lib.nunet_seg_metrics_ws_bytes(1, K, h * w) + 7) // 8, dtype=torch.float64, device=dev)
            L.check(lib.nunet_seg_metrics(L.ptr(logits[i]), L.ptr(t), 1, K, h * w, self.iou_thr, L.ptr(ws), L.nbytes(ws), L.ptr(sums, i * sz), 0,
                                          L.stream()), "nunet_seg_metrics")
        raw = sums.cpu().numpy().tobytes()
        smooth = 1e-5
        iou, dice, acc = [], [], []
        counts = OrderedDict((nm, [0] * K) for nm in ("tp", "fp", "fn", "tn"))
        for i in range(len(shapes)):
            s = L.SegSums.from_buffer_copy(raw[i * sz:(i + 1) * sz])
            tp, fp, fn, tn = (sum(getattr(s, nm)[:K]) for nm in ("tp", "fp", "fn", "tn"))
            iou.append((tp + smooth) / (tp + fp + fn + smooth))
            dice.append((2.0 * sum(s.soft_i[:K]) + smooth) / (sum(s.soft_p[:K]) + sum(s.soft_t[:K]) + smooth))
            acc.append((tp + tn) / float(tp + fp + fn + tn))
            for nm in counts:
                for k in range(K):
                    counts[nm][k] += int(getattr(s, nm)[k])
        return OrderedDict([("iou", iou), ("dice", dice), ("acc", acc), ("counts", counts)])
