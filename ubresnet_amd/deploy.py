"""Forward-only inference helpers: checkpoint loading and whole-view tiled segmentation.

Mirrors the inference side of the reference:
  * ``load_cosmic_retrain_model`` (deploy/ubresnet_funcs.py:41-68): build ``UResNet(inplanes=16,
    input_channels=1, num_classes=4)``, ``torch.load`` the checkpoint with a ``map_location``,
    strip the ``module.`` prefix a DataParallel checkpoint carries, ``load_state_dict``.
  * the pre-cropped loop (deploy/run_ubresnet_precropped.py:115-182): ``model.eval()`` forward per
    batch -> ``segment_crops``.
  * the whole-view loop (deploy/run_ubresnet_wholeview.py:191-277, a larflow script in the
    reference; only its shape is reusable): slice (bs,1,512,832) crops out of [3,1,rows,cols]
    plane images, run the model, stitch -> ``WholeViewSegmenter``.  The reference obtains crop boxes
    from larcv's UBSplitDetector (absent C++); here the tiling is regular with overlap
    (rows {0,496}, cols {0,656,1312,1968,2624} for a 1008 x 3456 view).
    Crop and stitch are HIP kernels; the per-batch forward is captured once in a hipGraph and
    replayed (fixed shapes), tiles are independent so multi-GPU inference is replicas only.
  * event products (``output="products"``): what the downstream chain keeps of the dense scores -- a class per pixel, its
    probability and per-plane class counts, only where the wire signal is above threshold (tf/compare_caffe_to_tf.py:17,81-89,
    ADC_THRESHOLD = 10.0) -- written by one fused kernel in place of the stitch (include/ubresnet_post.h).
  * flip test-time augmentation (``tta=("rows", "cols", "both")``): training flips every axis with probability 1/2 (``Augment``),
    so the network is evaluated on the flipped views of every batch as well and the class probabilities are averaged
    (include/ubresnet_tta.h) before the unchanged stitch or event products.
  * overlap-tile inference (``margin=``, ``blend="linear"`` / ``"hann"``): a denser tiling that keeps every kept pixel at least
    `margin` pixels away from a tile edge the network padded with zeros, and, with `blend`, overlapping tiles that vote: the
    stitch becomes the log of a weighted mean of the covering tiles' probabilities (include/ubresnet_blend.h).
"""
from __future__ import annotations

import ctypes as C
from typing import List, NamedTuple, Optional, Sequence, Tuple

import torch

from . import _lib as L
from . import _post as PL
from . import _blend as VL
from . import _tta as TL
from . import calibration as CB
from . import sparse as SP


class Products(NamedTuple):
    """event products (ubp_stitch_products): `label` uint8 (fill_label where the pixel is not lit), `confidence` float16
    (exp of the winning log-probability, +0 where not lit), `counts` int64 pixels per class among the lit ones"""
    label: torch.Tensor
    confidence: torch.Tensor
    counts: torch.Tensor


def _check_output(output, pixels=False):
    """`pixels`: the caller also has the lit-pixel list (WholeViewSegmenter; segment_crops has not)"""
    if output not in (("scores", "products", "pixels") if pixels else ("scores", "products")):
        raise ValueError("output must be 'scores'%s or 'products' (got %r)" % (", 'pixels'" if pixels else "", output))


def _check_cover(tiles, P, rows, cols):
    """the products path allocates label / confidence uninitialised: every pixel must lie in exactly one keep window"""
    cover = torch.zeros((P, rows, cols), dtype=torch.uint8)
    for (p, r0, c0, kr0, kr1, kc0, kc1) in tiles:
        cover[p, r0 + kr0:min(r0 + kr1, rows), c0 + kc0:min(c0 + kc1, cols)] += 1
    if int(cover.min()) != 1 or int(cover.max()) != 1:
        raise ValueError("the keep windows of the tiling do not partition the %d x %d x %d view" % (P, rows, cols))


def _desc7(tiles):
    flat = [v for t in tiles for v in t]
    return (C.c_int32 * len(flat))(*flat)


def _stitch_products(logp, nclass, th, tw, tiles, adc, vplanes, adc_threshold, fill_label, prod: Products, P, rows, cols):
    """one ubp_stitch_products launch on the current stream; `adc` is the float32 view the lit test reads (None: all lit)"""
    use_adc = adc is not None and adc_threshold is not None
    PL.check(PL.lib().ubp_stitch_products(logp.data_ptr(), nclass, th, tw, _desc7(tiles), len(tiles),
                                          adc.data_ptr() if use_adc else None, vplanes, float(adc_threshold) if use_adc else 0.0,
                                          prod.label.data_ptr(), prod.confidence.data_ptr(), prod.counts.data_ptr(),
                                          fill_label, P, rows, cols, L.stream_ptr()), "stitch_products")


def _new_products(P, nclass, rows, cols, device, kept=None):
    """the Products of a [P,rows,cols] image: label / confidence uninitialised (every pixel lies in one keep window: _check_cover;
    `kept`: a (label, confidence) pair that is reused instead), counts zero"""
    label, confidence = kept or (torch.empty((P, rows, cols), dtype=torch.uint8, device=device),
                                 torch.empty((P, rows, cols), dtype=torch.float16, device=device))
    return Products(label, confidence, torch.zeros((P, nclass), dtype=torch.int64, device=device))


def _image_products(logp, first, adc, vplanes, adc_threshold, fill_label, prod: Products):
    """images as whole-image tiles: `logp` [m,classes,H,W] are the images `first` .. `first` + m - 1 of `prod`, PL.MAX_TILES of
    them per ubp_stitch_products launch"""
    m, nclass, H, W = logp.shape
    for j in range(0, m, PL.MAX_TILES):
        tiles = [(first + q, 0, 0, 0, H, 0, W) for q in range(j, min(j + PL.MAX_TILES, m))]
        _stitch_products(logp[j:j + len(tiles)], nclass, H, W, tiles, adc, vplanes, adc_threshold, fill_label, prod,
                         prod.label.shape[0], H, W)


def load_model(checkpointfile: Optional[str], device, num_classes: int = 4, inplanes: int = 16, input_channels: int = 1,
               map_location=None, state_dict=None, arch: str = "uresnet", ema: bool = False):
    """UResNet (arch="uresnet") or ASPP_ResNet (arch="aspp") for deployment (deploy/ubresnet_funcs.py:41-68).
    `checkpointfile` is the reference's ``{iter, epoch, state_dict, best_prec1, optimizer}`` tar; tensors only are
    read (weights_only).  `ema=True`: the checkpoint dict carries ``"ema": ParamEMA.state_dict()`` and the averaged tensors
    in it override those of ``state_dict``; a checkpoint without that entry is a KeyError."""
    if arch == "uresnet":
        from .models.ub_uresnet import UResNet
        model = UResNet(inplanes=inplanes, input_channels=input_channels, num_classes=num_classes, showsizes=False)
    elif arch == "aspp":
        from .models.ASPP_ResNet import ASPP_ResNet
        model = ASPP_ResNet(num_classes, in_channels=input_channels, inplanes=inplanes, showsizes=False)
    else:
        raise ValueError("load_model: arch must be 'uresnet' or 'aspp' (got %r)" % (arch,))
    if state_dict is None and checkpointfile is not None:
        ckpt = torch.load(checkpointfile, map_location=map_location or "cpu", weights_only=True)
        state_dict = ckpt["state_dict"] if isinstance(ckpt, dict) and "state_dict" in ckpt else ckpt
        if ema:
            if not (isinstance(ckpt, dict) and isinstance(ckpt.get("ema"), dict)):
                raise KeyError("load_model(ema=True): the checkpoint %s has no \"ema\" entry (add \"ema\": ema.state_dict() to "
                               "the dict given to save_checkpoint)" % checkpointfile)
            state_dict = dict(state_dict)
            state_dict.update(ckpt["ema"]["shadow"])
            state_dict.update(ckpt["ema"].get("stats", {}))
    elif ema:
        raise KeyError("load_model(ema=True) needs a checkpoint file whose dict has an \"ema\" entry")
    if state_dict is not None:
        clean = {}
        for k, v in state_dict.items():
            clean[k[len("module."):] if k.startswith("module.") else k] = v
        model.load_state_dict(clean)
    model = model.to(device=torch.device(device))
    model.eval()
    return model


def save_checkpoint(state: dict, is_best: bool, p: int, filename: str = "checkpoint.pth.tar"):
    """save_checkpoint (training/train_ubresnet2018_wlarcv2.py:474-479): same files, same dict layout"""
    import shutil
    if p > 0:
        filename = "checkpoint.%dth.tar" % p
    torch.save(state, filename)
    if is_best:
        shutil.copyfile(filename, "model_best.tar")
    return filename


def _tempered(logp, scale):
    """`logp` rescaled in place by `scale` (one ubf_apply launch; every image group 0 unless there is a temperature per image);
    a model output that is a view of other storage is copied first"""
    if scale is None:
        return logp
    if logp.dtype != torch.float32:
        raise RuntimeError("segment_crops: temperature needs float32 log-probabilities (got %s)" % logp.dtype)
    logp = logp.contiguous()
    return scale.apply_(logp, [0] * logp.shape[0])


def _merged_views(model, x, flips, xin, merged, scale=None):
    """the flip views of one batch: `x` [m,C,H,W] is written flipped into `xin` (the identity view is read where it lies), the
    model runs on it and its float32 log-probabilities (rescaled by `scale`, if any) are merged, un-flipped, into `merged`
    [m,classes,H,W]"""
    m, cin, H, W = x.shape
    K = len(flips)
    for k, flip in enumerate(flips):
        if flip:
            TL.flip_planes(x.data_ptr(), xin.data_ptr(), m * cin, H, W, flip, L.stream_ptr())
        logp = model(xin[:m] if flip else x).contiguous()
        if logp.dtype != torch.float32 or tuple(logp.shape) != tuple(merged.shape):
            raise RuntimeError("segment_crops: the model must return float32 log-probabilities %s (got %s %s)"
                               % (tuple(merged.shape), logp.dtype, tuple(logp.shape)))
        logp = _tempered(logp, scale)
        TL.merge_view(logp.data_ptr(), merged.data_ptr(), merged.shape[0] * merged.shape[1], H, W, flip, k, K, L.stream_ptr())


def _batch_logp(model, x, flips, xin, merged, scale, for_products):
    """the log-probabilities of one batch `x` [m,C,H,W], rescaled by `scale`, if any: with `flips`, those of the views merged into
    `merged`; else what the model returns -- contiguous float32 `for_products`, which the products kernel reads"""
    if flips:
        _merged_views(model, x, flips, xin, merged, scale)
        return merged
    logp = model(x)
    if for_products:
        logp = logp.contiguous()
        if logp.dtype != torch.float32:
            raise RuntimeError("segment_crops: the model must return float32 log-probabilities (got %s)" % logp.dtype)
    return _tempered(logp, scale)


@torch.no_grad()
def segment_crops(model, adc: torch.Tensor, batch: int = 4, output: str = "scores", adc_threshold: Optional[float] = 10.0,
                  fill_label: int = 255, tta=None, temperature=None):
    """eval forward over pre-cropped images [n,C,H,W] in batches (deploy/run_ubresnet_precropped.py:115-182).
    output="products": Products of [n,H,W] / [n,H,W] / [n,classes] instead of the scores; every image is one whole-image tile
    of ubp_stitch_products and is lit where any of its channels is above `adc_threshold` (None: everywhere).
    tta: None / () or a tuple drawn from "rows", "cols", "both": every batch also runs flipped that way and the scores are the log
    of the mean probability over the views, the identity first (needs a CUDA float32 input; the lit test reads the unflipped
    `adc`).
    temperature: None, or a float, calibration.TemperatureScale or calibration.Calibration: the scores of every forward (every
    flip view) become log_softmax(scores / T) by one ubf_apply launch before anything else reads them.  The crops carry no
    plane, so a single temperature is needed (a per-plane scale is a ValueError)."""
    _check_output(output)
    flips = TL.parse_views(tta)
    scale = CB.as_scale(temperature)
    if scale is not None and len(scale) != 1:
        raise ValueError("segment_crops: pre-cropped images carry no plane: temperature must be a single value (got %d)" % len(scale))
    model.eval()
    products = output == "products"
    cin = xin = scores = prod = None
    if flips or products:                       # the plain scores path takes whatever the model takes
        L.require_cuda(adc, "adc")
        if adc.dtype != torch.float32 or adc.dim() != 4:
            raise RuntimeError("segment_crops: expected float32 [n,C,H,W], got %s %s" % (adc.dtype, tuple(adc.shape)))
        adc = adc.contiguous()
        n, cin, H, W = adc.shape
        nclass = model.conv11.out_channels
        if flips:                               # the views merge into the scores themselves, or into one batch of them
            xin = torch.empty((min(batch, n), cin, H, W), dtype=torch.float32, device=adc.device)
            scores = torch.empty((min(batch, n) if products else n, nclass, H, W), dtype=torch.float32, device=adc.device)
        if products:
            prod = _new_products(n, nclass, H, W, adc.device)
    n, outs = adc.shape[0], []
    for i in range(0, n, batch):
        x = adc[i:i + batch]
        merged = None if not flips else scores[:x.shape[0]] if products else scores[i:i + batch]
        logp = _batch_logp(model, x, flips, xin, merged, scale, products)
        if products:
            _image_products(logp, i, adc, cin, adc_threshold, fill_label, prod)
        else:
            outs.append(logp)
    return prod if products else scores if flips else torch.cat(outs, 0)


def regular_tiling(rows: int, cols: int, th: int = 512, tw: int = 832) -> Tuple[List[int], List[int]]:
    """row/col origins of the fewest tiles covering rows x cols with the overlap spread evenly: margin_tiling without a margin
    (for n > t, ceil((n - t) / t) + 1 = ceil(n / t) tiles)"""
    return margin_tiling(rows, cols, th, tw, margin=0)


def margin_tiling(rows: int, cols: int, th: int = 512, tw: int = 832, margin: int = 0) -> Tuple[List[int], List[int]]:
    """row/col origins of the fewest evenly spread tiles whose neighbours overlap by at least 2 * margin: per axis of length n
    and tile t, [0] if n <= t, else k = ceil((n - t) / (t - 2 * margin)) + 1 tiles at round(i * (n - t) / (k - 1)).  The integer
    steps are the floor or the ceiling of a real step <= t - 2 * margin, so every overlap is at least 2 * margin and the
    mid-overlap keep windows (_keep_windows) leave at least `margin` pixels between a kept pixel and any tile edge that is not
    the view's own.  margin = 0 is regular_tiling.  0 <= 4 * margin <= min(th, tw), else ValueError."""
    if isinstance(margin, bool) or not isinstance(margin, int) or margin < 0 or 4 * margin > min(th, tw):
        raise ValueError("margin must be an int with 0 <= 4 * margin <= min(tile) = %d (got %r)" % (min(th, tw), margin))

    def origins(n, t):
        if n <= t:
            return [0]
        k = -(-(n - t) // (t - 2 * margin)) + 1
        step = (n - t) / float(k - 1)
        return sorted(set(int(round(i * step)) for i in range(k)))
    return origins(rows, th), origins(cols, tw)


def view_tiles(rows: int, cols: int, planes: int, th: int, tw: int, stacked: bool, margin: int = 0):
    """tile descriptors {plane, row0, col0, keep_r0, keep_r1, keep_c0, keep_c1} (ubr_crop_tiles / ubr_stitch_tiles) of
    margin_tiling (margin 0: the regular tiling).  Per plane: one descriptor per (plane, row origin, column origin).
    Stacked (a model that takes the planes as channels): one descriptor per (row origin, column origin) with plane 0 --
    stacked_crop_desc() expands it for the crop, the stitch takes it as it is with P = 1."""
    ro, co = margin_tiling(rows, cols, th, tw, margin)
    rk, ck = _keep_windows(ro, th, rows), _keep_windows(co, tw, cols)
    tiles = []
    for p in range(1 if stacked else planes):
        for (r0, (rl, rh)) in zip(ro, rk):
            for (c0, (cl, ch)) in zip(co, ck):
                tiles.append((p, r0, c0, rl - r0, rh - r0, cl - c0, ch - c0))
    return tiles


def stacked_crop_desc(tiles, planes: int):
    """a stacked tile is `planes` consecutive single-plane crops at the same origin: the crop kernel then writes
    [len(tiles), planes, th, tw]"""
    return [(p,) + tuple(t[1:]) for t in tiles for p in range(planes)]


def _keep_windows(origins: Sequence[int], t: int, n: int):
    """split the overlaps in the middle: tile i keeps [lo_i, hi_i) in view coordinates"""
    out = []
    for i, o in enumerate(origins):
        lo = 0 if i == 0 else (origins[i - 1] + t + o) // 2
        hi = min(n, o + t) if i == len(origins) - 1 else (o + t + origins[i + 1]) // 2
        out.append((lo, hi))
    return out


class WholeViewSegmenter:
    """Tiled whole-view inference: crop -> model (hipGraph replay) -> stitch.

        seg = WholeViewSegmenter(model, rows=1008, cols=3456, planes=3, tile=(512, 832), batch=10,
                                 dtype=torch.float16)
        scores = seg(view)          # view [planes,1,rows,cols] float32 on the GPU -> [planes,C,rows,cols]

    A model whose first conv takes one channel (UResNet, deploy/run_ubresnet_wholeview.py) sees every plane's tiles on their
    own.  A model that takes `planes` channels (ASPP_ResNet, the three planes stacked as channels) sees one stacked tile per
    position, and the result is one map per event: scores [C,rows,cols], products [rows,cols] and [C], a pixel lit if any plane
    is.  Everything runs on the current stream and nothing is read back.  A call is five stages, each keyword acting in one:

    1. Input (_input).  A float32 [planes,1,rows,cols] view on the device, or a sparse.SparseEvent (ubresnet_amd/sparse.py): the
       list is copied to the device if it is on the host and scattered (ubz_scatter_view) into a view buffer kept between calls;
       `seg.status` is the device word that counts the entries the scatter refused.  The forward of one batch of tiles is
       captured into a hipGraph on the first call (use_graph=False: run eagerly) and again if the model's storage was replaced.

    2. Output buffers (_begin).  output="scores": a fresh [planes,C,rows,cols] float32.  output="products": fresh Products --
       label and confidence [planes,rows,cols], counts [planes,C] -- and no dense score buffer.  output="pixels": the same
       products path into dense label / confidence buffers kept between calls.  blend: the dense float32 scores the tiles vote
       into, set to -inf (ubv_blend_begin); fresh for "scores", kept between calls for "products" and "pixels", which then do
       need the dense buffer that plain products avoid.

    3. Chunks of `batch` tiles (_chunk_scores).  The tiling is fixed at construction.  margin=m (0 <= 4 m <= the smaller tile
       side) makes it that of margin_tiling, whose overlaps are at least 2 m wide, so that no kept pixel lies within m pixels of a
       tile edge inside the view (the networks zero-pad every conv there): more tiles per event, the same kernels.  A chunk is
       cropped once (ubr_crop_tiles) and runs through the forward once per view.  tta=("rows", "cols", "both") or any part of it:
       the views are the identity, then the named flips in the order given; the chunk is flipped on its way into the forward's
       input (ubt_flip_planes) and the views' log-probabilities are merged, un-flipped, into the log of their mean probability
       (ubt_merge_view, include/ubresnet_tta.h).  temperature=T (a float, a sequence with one value per plane, a
       calibration.TemperatureScale or a calibration.Calibration): the scores of every forward -- every chunk, every view --
       become log_softmax(scores / T) by one in-place ubf_apply launch (include/ubresnet_calib.h) before anything else reads
       them, so the merge and the blend average calibrated probabilities.  The inverse temperature of a tile is that of its plane
       (stacked tiles: group 0).  T is that of the single-view network: fit it with tta, blend and temperature off.

    4. Sink (_emit), one launch per chunk.  blend="linear" or "hann": ubv_blend_tiles (include/ubresnet_blend.h) -- overlapping
       tiles vote instead of being cut in the middle.  Along each axis a tile's weight is zero within `margin` of a tile edge
       inside the view, rises over the next ceil(t / 2) - m pixels (linearly, or as sin^2) to one, and the weights of the tiles
       covering a pixel are normalised to sum to one; a tile's weight at a pixel is its row weight times its column weight, and
       the scores are the log of that weighted mean of probabilities.  The log-weights are two tables built at construction.
       Else "products" / "pixels": ubp_stitch_products writes class, confidence and counts of the chunk's keep windows, with the
       input view as the ADC of the lit test (`adc_threshold`, None = every pixel lit; unlit pixels get `fill_label`).  Else:
       ubr_stitch_tiles copies the keep windows into the scores.

    5. Finish (_finish).  Products with blend: ubp_stitch_products over the finished dense buffer, every plane one whole-view
       tile.  "pixels": the dense products are compacted (ubz_compact, include/ubresnet_sparse.h) into a sparse.PixelList of the
       lit pixels in ascending pixel-index order (`capacity` entries; None: as many as there are pixels); the list's buffers are
       kept between calls, so a call overwrites the list of the call before it, and PixelList.read() is the host
       synchronisation.  Stacked results lose their leading axis of one.
    """

    def __init__(self, model, rows: int, cols: int, planes: int = 3, tile=(512, 832), batch: int = 10,
                 dtype: torch.dtype = torch.float16, use_graph: bool = True, output: str = "scores",
                 adc_threshold: Optional[float] = 10.0, fill_label: int = 255, tta=None, margin: int = 0, blend=None,
                 temperature=None, capacity: Optional[int] = None):
        _check_output(output, pixels=True)
        self.scale = CB.as_scale(temperature)
        if capacity is not None and (isinstance(capacity, bool) or not isinstance(capacity, int) or capacity < 1):
            raise ValueError("capacity must be None or an int >= 1 (got %r)" % (capacity,))
        if capacity is not None and output != "pixels":
            raise ValueError("capacity is the length of the pixel list: it needs output='pixels'")
        self.capacity = capacity
        self._flips = TL.parse_views(tta)                   # () or (0, flip mask of every named view)
        self.blend = VL.check_kind(blend)
        self.output, self.adc_threshold, self.fill_label = output, adc_threshold, fill_label
        self._products = output in ("products", "pixels")
        self.model, self.rows, self.cols, self.planes = model, rows, cols, planes
        self.th, self.tw = tile
        if self.th % 32 or self.tw % 32:
            raise ValueError("tile size must be a multiple of 32")
        self.batch, self.dtype, self.use_graph = batch, dtype, use_graph
        cin = model.conv1.in_channels
        if cin != 1 and cin != planes:
            raise ValueError("WholeViewSegmenter: the model takes %d channels; 1 (per-plane tiles) or planes = %d (stacked tiles) "
                             "are supported" % (cin, planes))
        self.stacked = cin > 1
        self.cin = cin
        self._oplanes = 1 if self.stacked else planes       # planes of the result
        self._vplanes = planes if self.stacked else 1       # view planes the lit test reads per plane of the result
        self.margin = margin
        self._origins = margin_tiling(rows, cols, self.th, self.tw, margin)             # refuses a bad margin
        self.tiles = view_tiles(rows, cols, planes, self.th, self.tw, self.stacked, margin)     # (plane, r0, c0, kr0, kr1, kc0, kc1)
        if batch * cin > L.MAX_TILES:
            raise ValueError("batch * planes must be <= %d tile descriptors (UBR_MAX_TILES)" % L.MAX_TILES)
        self.nclass = model.conv11.out_channels
        self._tile_groups = None                            # temperature: the group of every tile, in the order of self.tiles
        self._chunk_betas = {}                              # and per chunk start the device array of 1 / T, built on first use
        if self.scale is not None:
            if len(self.scale) not in (1, self._oplanes):
                raise ValueError("WholeViewSegmenter: temperature must be one value or one per plane (%d), got %d; stacked tiles "
                                 "are group 0" % (self._oplanes, len(self.scale)))
            self._tile_groups = [t[0] if len(self.scale) > 1 else 0 for t in self.tiles]
        if self._products:
            _check_cover(self.tiles, self._oplanes, rows, cols)
        if self.blend is not None:
            if batch > VL.MAX_TILES:
                raise ValueError("batch must be <= %d tile descriptors (UBV_MAX_TILES) with blend" % VL.MAX_TILES)
            ro, co = self._origins
            lr = VL.axis_log_weights(ro, self.th, rows, margin, self.blend)
            lc = VL.axis_log_weights(co, self.tw, cols, margin, self.blend)
            # in the order of self.tiles: planes x row origins x column origins; float64, rounded once when they go to the device
            self._blend_host = (torch.tensor([r for _ in range(self._oplanes) for r in lr for _ in co], dtype=torch.float64),
                                torch.tensor([c for _ in range(self._oplanes) for _ in ro for c in lc], dtype=torch.float64))
        # Device state, built when its feature first runs and None until then.
        # The forward of one batch of tiles (_ensure_graph); dropped together when the model's storage is replaced:
        self._graph = self._static_in = self._static_out = self._captured_sig = None
        self._tta_side = self._tta_merged = None            # tta: the cropped chunk, unflipped; the running merge of the views
        # Kept between calls:
        self._blend_lw = None                               # blend: (lw_rows [ntiles][th], lw_cols [ntiles][tw])
        self._blend_out = None                              # blend with products: the dense scores
        self._view_buf = self.status = None                 # sparse input: the dense view; the refused entries (int64 [1])
        self._pix_dense = self._compactor = None            # "pixels": dense (label, confidence); the list's buffers and scratch

    @property
    def tiles_per_event(self):
        return len(self.tiles)

    def _forward_batch(self, x):
        old = getattr(self.model, "compute_dtype", None)
        self.model.compute_dtype = self.dtype
        try:
            return self.model(x)
        finally:
            self.model.compute_dtype = old

    def _signature(self):
        return tuple(t.data_ptr() for t in self.model.parameters()) + tuple(t.data_ptr() for t in self.model.buffers())

    def _ensure_graph(self, device):
        # the captured graph bakes in the device addresses of parameters, buffers and packed weight images: when the model's
        # storage was replaced since the capture (model.to(), a flat optimizer adopting the parameters,
        # load_state_dict(assign=True)) the replay would read freed memory -- capture again
        sig = self._signature()
        if self._static_in is not None and sig != self._captured_sig:
            self._graph = self._static_in = self._static_out = self._tta_side = self._tta_merged = None
        if self._static_in is not None:
            return
        self._captured_sig = sig
        self._static_in = torch.zeros((self.batch, self.cin, self.th, self.tw), dtype=torch.float32, device=device)
        if self._flips:
            self._tta_side = torch.zeros_like(self._static_in)
            self._tta_merged = torch.empty((self.batch, self.nclass, self.th, self.tw), dtype=torch.float32, device=device)
        self.model.eval()
        with torch.no_grad():
            self._forward_batch(self._static_in)            # warm-up: packs weights, raises LDS limits, fills allocator
            torch.cuda.synchronize()
            if self.use_graph:
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    self._static_out = self._forward_batch(self._static_in)
                self._graph = g

    def _temper(self, scores, i, n):
        """ubf_apply in place on the first n tiles of `scores`, the chunk that starts at tile i"""
        if scores.dtype != torch.float32 or not scores.is_contiguous():
            raise RuntimeError("WholeViewSegmenter: temperature needs contiguous float32 scores (got %s)" % scores.dtype)
        if i not in self._chunk_betas or self._chunk_betas[i].device != scores.device:
            self._chunk_betas[i] = self.scale.device_betas(self._tile_groups[i:i + n], scores.device)
        CB._calib.apply(scores.data_ptr(), scores.data_ptr(), self._chunk_betas[i].data_ptr(), n, self.nclass, self.th, self.tw,
                        L.stream_ptr())
        return scores

    def _scatter(self, event):
        """a SparseEvent -> the dense view in the buffer kept between calls, on the model's device (or the list's own)"""
        if (event.planes, event.rows, event.cols) != (self.planes, self.rows, self.cols):
            raise RuntimeError("WholeViewSegmenter: expected a SparseEvent of %d x %d x %d, got %d x %d x %d"
                               % (self.planes, self.rows, self.cols, event.planes, event.rows, event.cols))
        device = event.index.device if event.index.is_cuda else next(self.model.parameters()).device
        if self._view_buf is None or self._view_buf.device != device:
            self._view_buf = torch.empty((self.planes, 1, self.rows, self.cols), dtype=torch.float32, device=device)
            self.status = torch.zeros(1, dtype=torch.int64, device=device)
        return event.to_view(device, out=self._view_buf, status=self.status)

    def _input(self, view):
        """the contiguous float32 view on the device, the forward captured for that device"""
        if isinstance(view, SP.SparseEvent):
            view = self._scatter(view)
        L.require_cuda(view, "view")
        if view.dtype != torch.float32 or tuple(view.shape) != (self.planes, 1, self.rows, self.cols):
            raise RuntimeError("WholeViewSegmenter: expected float32 [%d,1,%d,%d], got %s %s"
                               % (self.planes, self.rows, self.cols, view.dtype, tuple(view.shape)))
        view = view.contiguous()
        self._ensure_graph(view.device)
        return view

    def _begin(self, device):
        """-> (out, blended): what the call fills, and the dense scores the tiles vote into (None without blend)"""
        shape = (self._oplanes, self.nclass, self.rows, self.cols)
        blended = None
        if self.blend is not None:
            if self._blend_lw is None or self._blend_lw[0].device != device:
                self._blend_lw = tuple(t.to(torch.float32).to(device) for t in self._blend_host)
            if not self._products:
                blended = torch.empty(shape, dtype=torch.float32, device=device)
            else:
                if self._blend_out is None or self._blend_out.device != device:
                    self._blend_out = torch.empty(shape, dtype=torch.float32, device=device)
                blended = self._blend_out
            VL.blend_begin(blended.data_ptr(), blended.numel(), L.stream_ptr())
        if self.output == "pixels" and (self._pix_dense is None or self._pix_dense[0].device != device):
            self._pix_dense = tuple(_new_products(self._oplanes, self.nclass, self.rows, self.cols, device)[:2])
            self._compactor = SP.Compactor(self._oplanes, self.rows, self.cols, self.capacity, device)
        if self._products:
            return _new_products(self._oplanes, self.nclass, self.rows, self.cols, device, kept=self._pix_dense), blended
        return (torch.empty(shape, dtype=torch.float32, device=device) if blended is None else blended), blended

    def _chunk_scores(self, view, i, chunk):
        """the log-probabilities of the tiles `chunk`, which start at tile i: crop, then per view flip -> forward -> temper ->
        merge.  -> the buffer the sink reads (its first len(chunk) tiles)"""
        n, st = len(chunk), L.stream_ptr()
        cropped = self._tta_side if self._flips else self._static_in
        L.check(L.lib().ubr_crop_tiles(view.data_ptr(), self.planes, self.rows, self.cols,
                                       _desc7(stacked_crop_desc(chunk, self.planes) if self.stacked else chunk), n * self.cin,
                                       self.th, self.tw, cropped.data_ptr(), st), "crop_tiles")
        for k, flip in enumerate(self._flips or (None,)):
            if flip is not None:                            # the identity view is a copy: flip 0
                TL.flip_planes(cropped.data_ptr(), self._static_in.data_ptr(), n * self.cin, self.th, self.tw, flip, st)
            if self._graph is not None:
                self._graph.replay()
                scores = self._static_out
            else:
                scores = self._forward_batch(self._static_in)
            if self.scale is not None:                      # in place on the scores of this forward, before anything reads them
                scores = self._temper(scores, i, n)
            if flip is not None:
                TL.merge_view(scores.data_ptr(), self._tta_merged.data_ptr(), n * self.nclass, self.th, self.tw, flip, k,
                              len(self._flips), st)
        return self._tta_merged if self._flips else scores

    def _emit(self, scores, i, chunk, view, out, blended):
        """the one launch that takes the chunk's scores into the result: blend, event products or stitch"""
        dims = (self._oplanes, self.rows, self.cols)
        if blended is not None:
            VL.blend_tiles(scores.data_ptr(), self.nclass, self.th, self.tw, VL.desc3(chunk), len(chunk),
                           self._blend_lw[0][i:].data_ptr(), self._blend_lw[1][i:].data_ptr(), blended.data_ptr(), *dims,
                           L.stream_ptr())
        elif self._products:
            _stitch_products(scores, self.nclass, self.th, self.tw, chunk, view, self._vplanes, self.adc_threshold, self.fill_label,
                             out, *dims)
        else:
            L.check(L.lib().ubr_stitch_tiles(scores.data_ptr(), self.nclass, self.th, self.tw, _desc7(chunk), len(chunk),
                                             out.data_ptr(), *dims, L.stream_ptr()), "stitch_tiles")

    def _finish(self, view, out, blended):
        """what the call returns: the products of the blended scores, the pixel list of the products, stacked results unwrapped"""
        if self._products and blended is not None:
            _image_products(blended, 0, view, self._vplanes, self.adc_threshold, self.fill_label, out)
        if self.output == "pixels":
            return self._compactor(out.label, out.confidence, out.counts[0] if self.stacked else out.counts, view, self._vplanes,
                                   self.adc_threshold, self.fill_label)
        if self._products:
            return Products(*(t[0] for t in out)) if self.stacked else out
        return out[0] if self.stacked else out

    @torch.no_grad()
    def __call__(self, view):
        view = self._input(view)
        out, blended = self._begin(view.device)
        for i in range(0, len(self.tiles), self.batch):
            chunk = self.tiles[i:i + self.batch]
            self._emit(self._chunk_scores(view, i, chunk), i, chunk, view, out, blended)
        return self._finish(view, out, blended)

