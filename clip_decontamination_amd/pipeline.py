"""Sliding-window segmentation pipeline on top of the HIP library (host logic only).

Mirrors reference segmentor.py: ``forward_feature`` (:286-392), ``forward_slide`` (:394-451),
``postprocess_result`` (:475-499) -- but tiles are cropped / padded / embedded on the device in batches,
stitched write-once, and (opt-in: ``tile_group``) partitioned over the ranks of a torch.distributed group with ONE
all-gather of the per-tile patch-grid logit maps; per-pixel logit maps (JBU upsampler) travel point to
point instead, only the tiles that straddle a canvas-band edge.  Every rank stitches and labels its own canvas band.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Callable, List, Optional, Sequence, Tuple, Union

import torch

from . import ops
from .engine import HipCLIP, compute_padsize


def tile_windows(H: int, W: int, stride: Tuple[int, int], crop: Tuple[int, int]) -> List[Tuple[int, int, int, int]]:
    """Raster-order windows (y1, y2, x1, x2); the last window of each axis is shifted back inside the
    image (reference segmentor.py:411-423)."""
    hs, ws = stride
    hc, wc = crop
    hg = max(H - hc + hs - 1, 0) // hs + 1
    wg = max(W - wc + ws - 1, 0) // ws + 1
    out = []
    for hi in range(hg):
        for wi in range(wg):
            y2 = min(hi * hs + hc, H)
            x2 = min(wi * ws + wc, W)
            out.append((max(y2 - hc, 0), y2, max(x2 - wc, 0), x2))
    return out


def partition(n_items: int, world: int, rank: int) -> Tuple[int, int]:
    """Contiguous block partition of the raster tile list: [lo, hi) for ``rank`` (sizes differ by <= 1)."""
    base, rem = divmod(n_items, world)
    lo = rank * base + min(rank, rem)
    return lo, lo + base + (1 if rank < rem else 0)


def _is_nccl(group) -> bool:
    return torch.distributed.get_backend(group) == "nccl"


def resolve_tile_group(group):
    """Tile sharding is OPT-IN: ``None`` = this process handles the whole scene (the reference's own multi-GPU launch shards IMAGES
    over ranks, dist_test.sh -> mmengine DefaultSampler, so an initialised default process group must NOT trigger tile sharding);
    ``"world"`` = the default group; otherwise a torch.distributed ProcessGroup."""
    if group is None:
        return None
    if isinstance(group, str):
        if group != "world":
            raise ValueError(f"tile_group must be None, 'world' or a ProcessGroup, got {group!r}")
        if not (torch.distributed.is_available() and torch.distributed.is_initialized()):
            raise RuntimeError("tile_group='world' needs an initialised torch.distributed process group")
        return torch.distributed.group.WORLD
    return group


def check_same_scene(desc: Sequence[int], device, group) -> None:
    """Every rank of a tile group must hold the SAME scene geometry (H, W, tile count, crop, stride ...): ranks that hold
    different images would silently mix tiles of different scenes in the gather.  One tiny all-gather per scene."""
    world = torch.distributed.get_world_size(group)
    dev = device if _is_nccl(group) else torch.device("cpu")
    mine = torch.tensor(list(desc), dtype=torch.int64, device=dev)
    allv = torch.empty(world * mine.numel(), dtype=torch.int64, device=dev)
    torch.distributed.all_gather_into_tensor(allv, mine, group=group)
    allv = allv.reshape(world, -1).cpu()
    if not bool((allv == allv[0]).all()):
        raise RuntimeError("tile sharding: the ranks of the tile group hold different scenes "
                           f"(per-rank [H, W, tiles, crop_h, crop_w, stride_h, stride_w, Q]: {allv.tolist()}); "
                           "every rank must be given the same image")


def gather_blocks(local: torch.Tensor, n_items: int, world: int, rank: int, group=None) -> torch.Tensor:
    """All-gather of per-rank blocks of the raster tile list (``partition``): ``local`` holds this rank's items (possibly followed
    by padding); returns the full [n_items, ...] list on every rank.  Blocks are padded to ceil(n_items / world) so the
    collective is fixed-size: ONE all_gather_into_tensor (RCCL over xGMI on GPUs) into a preallocated buffer, which IS the result
    when the tile count divides evenly."""
    lo, hi = partition(n_items, world, rank)
    t_pad = (n_items + world - 1) // world
    tail = tuple(local.shape[1:])
    buf = local.new_empty((world * t_pad,) + tail)
    block = local.new_zeros((t_pad,) + tail)
    block[:hi - lo] = local[:hi - lo]
    torch.distributed.all_gather_into_tensor(buf, block, group=group)
    if n_items == world * t_pad:
        return buf
    parts = []
    for r in range(world):
        a, b = partition(n_items, world, r)
        parts.append(buf[r * t_pad:r * t_pad + (b - a)])
    return torch.cat(parts, 0)


def band_plan(wins: Sequence[Tuple[int, int, int, int]], H: int, world: int):
    """Canvas bands for a band-local stitch: rank r owns canvas rows [yb[r], yb[r+1]) where yb[r] is the first row of its first
    tile (raster order, ``partition``); need[r] = (a, b) is the contiguous range of tile ids that overlap the band.  Because y1 is
    non-decreasing in raster order, need[r] = [a_r, hi_r) with a_r <= lo_r: a rank only ever needs tiles of LOWER ranks (the
    halo), never of higher ones."""
    T = len(wins)
    yb = []
    for r in range(world):
        lo, hi = partition(T, world, r)
        yb.append(0 if r == 0 else (wins[lo][0] if hi > lo else H))
    yb.append(H)
    for r in range(world - 1, 0, -1):                      # empty blocks sit at the end; keep yb monotone
        yb[r] = min(yb[r], yb[r + 1])
    need = []
    for r in range(world):
        lo, hi = partition(T, world, r)
        if yb[r + 1] <= yb[r]:
            need.append((lo, lo))
            continue
        a = lo
        while a > 0 and wins[a - 1][1] > yb[r]:
            a -= 1
        need.append((a, hi))
    return yb, need


def exchange_halo_tiles(local: torch.Tensor, wins, world: int, rank: int, group=None, plan=None) -> Tuple[torch.Tensor, int]:
    """Band-local stitch, step 1: every rank receives the tile logits of LOWER ranks that overlap its canvas band, point to
    point (xGMI is point-to-point: only the tiles that straddle a band edge travel, instead of all-gathering [T,Q,S,S] per-pixel
    logits to everyone).  Returns (tile logits of tiles [a, hi) in raster order, a)."""
    T = len(wins)
    yb, need = plan if plan is not None else band_plan(wins, wins[-1][1], world)
    lo, hi = partition(T, world, rank)
    owner = [r for r in range(world) for _ in range(partition(T, world, r)[1] - partition(T, world, r)[0])]
    dist = torch.distributed
    peer = (lambda r: r) if group is None or group is dist.group.WORLD else (lambda r: dist.get_global_rank(group, r))
    staged = (not _is_nccl(group)) and local.is_cuda      # gloo moves host memory only
    a, b = need[rank]
    halo = local.new_empty((lo - a,) + tuple(local.shape[1:]), device="cpu" if staged else local.device)
    ops_, keep = [], []
    src = local.cpu() if staged else local
    for r in range(rank + 1, world):                      # my tiles that a higher rank's band needs
        ra, _ = need[r]
        s0, s1 = max(ra, lo), hi
        if partition(T, world, r)[1] > partition(T, world, r)[0] and s1 > s0 and ra < hi:
            t = src[s0 - lo:s1 - lo].contiguous()
            keep.append(t)
            ops_.append(dist.P2POp(dist.isend, t, peer(r), group))
    t0 = a
    while t0 < lo:                                        # tiles [a, lo) come from their owners, one message per owner
        o = owner[t0]
        t1 = min(partition(T, world, o)[1], lo)
        ops_.append(dist.P2POp(dist.irecv, halo[t0 - a:t1 - a], peer(o), group))
        t0 = t1
    if ops_:
        for w in dist.batch_isend_irecv(ops_):
            w.wait()
    halo = halo.to(local.device) if staged else halo
    return (torch.cat([halo, local[:hi - lo]], 0) if lo > a else local[:hi - lo]), a


def sharded_cross_tile_fusion(tokens: torch.Tensor, steps, n_tiles: int, world: int, rank: int, group=None) -> torch.Tensor:
    """Cross-tile boundary fusion when the raster tile list is partitioned over ranks.  ``tokens`` [n_local, n, C]
    are this rank's PRE-fusion patch tokens; a tile needs the right columns of its left neighbour and the final bottom rows of
    its upper neighbour, which may live on another rank: two all-gathers of packed strips (a few hundred kB per tile edge)
    replace the reference's per-process boundary cache.  ``steps`` = ops.CrossTileSteps (or a stand-in with pack/fuse/apply)."""
    lo, hi = partition(n_tiles, world, rank)
    assert tokens.shape[0] == hi - lo
    if hi == lo:                                   # more ranks than tiles: still take part in the collectives
        dummy = tokens.new_zeros((0, steps.strip_len(0), tokens.shape[-1]))
        gather_blocks(dummy, n_tiles, world, rank, group)
        gather_blocks(tokens.new_zeros((0, steps.strip_len(1), tokens.shape[-1])), n_tiles, world, rank, group)
        return tokens
    right_all = gather_blocks(steps.pack(tokens, lo, 0), n_tiles, world, rank, group)
    left_res = steps.fuse(tokens, lo, right_all, 0)
    bottom_all = gather_blocks(steps.pack(tokens, lo, 1, left_res), n_tiles, world, rank, group)
    top_res = steps.fuse(tokens, lo, bottom_all, 1)
    return steps.apply(tokens, lo, left_res, top_res)


def launch_chunks(n_tiles: int, limit: int) -> List[Tuple[int, int]]:
    """[start, stop) ranges of the tile list, one per launch of the tower: as few launches as `limit` tiles per launch allows, of EQUAL size
    (33 tiles at a limit of 32 run as 17 + 16, not 32 + 1 -- a one- or two-tile launch leaves most of the chip idle)."""
    if n_tiles <= 0:
        return []
    limit = max(1, int(limit))
    n = -(-n_tiles // limit)
    base, extra = divmod(n_tiles, n)
    out, a = [], 0
    for i in range(n):
        b = a + base + (1 if i < extra else 0)
        out.append((a, b))
        a = b
    return out


@dataclass
class FlushGroup:
    """A run of whole images of one tile-size group, images [img_lo, img_hi) and tiles [tile_lo, tile_hi) of the group, whose tile
    logits and canvases are computed, stitched and handed on together; ``chunks`` = the tower launches over its tiles."""
    img_lo: int
    img_hi: int
    tile_lo: int
    tile_hi: int
    chunks: List[Tuple[int, int]]


@dataclass
class TileSizeGroup:
    """The images of a packed batch that share a window size (every window of one image has the same size, ``tile_windows``).
    Tiles are image-major, raster order within an image; ``tile_image`` holds indices into the planner's ``shapes``."""
    tile_hw: Tuple[int, int]
    images: List[int]
    shapes: List[Tuple[int, int]]
    grids: List[Tuple[int, int]]
    windows: List[Tuple[int, int, int, int]]
    tile_image: List[int]
    first_tile: List[int]
    n_tiles: List[int]
    chunks: List[Tuple[int, int]]
    canvas_offsets: List[int]            # pixel offset of each image's canvas: prefix sum of H*W over ``images`` (len + 1 entries)
    flush: List[FlushGroup] = field(default_factory=list)


def plan_images(shapes: Sequence[Tuple[int, int]], stride, crop, patch: int, tiles_per_launch: int,
                tile_bytes: Union[int, Callable[[Tuple[int, int]], int]] = 0, pixel_bytes: Union[int, Callable[[int], int]] = 0,
                flush_bytes: Optional[int] = None) -> List[TileSizeGroup]:
    """Packs the sliding windows of images of any sizes into equal tower launches (pure host logic, no device).

    Images are grouped by window size (a launch shares one tile shape; images smaller than the crop form their own groups), groups
    in order of first appearance.  Within a group the windows of all its images are concatenated and cut by ``launch_chunks``,
    freely across image boundaries.  The group is further cut into flush groups: runs of whole images whose tile logits
    (``tile_bytes`` per tile, or a function of the tile size) plus canvases (``pixel_bytes`` per pixel, or a function of the image's index
    that returns the bytes of that image's outputs: they may have another size than the image) stay within ``flush_bytes``;
    an image that alone exceeds the bound is a flush group of its own.  ``patch`` is checked, the windows do not depend on it."""
    stride = (stride, stride) if isinstance(stride, int) else tuple(stride)
    crop = (crop, crop) if isinstance(crop, int) else tuple(crop)
    if int(patch) <= 0:
        raise ValueError(f"patch must be positive, got {patch}")
    groups: dict = {}
    for i, (H, W) in enumerate(shapes):
        H, W = int(H), int(W)
        if H <= 0 or W <= 0:
            raise ValueError(f"image {i} has an empty shape {(H, W)}")
        wins = tile_windows(H, W, stride, crop)
        th, tw = wins[0][1] - wins[0][0], wins[0][3] - wins[0][2]
        g = groups.get((th, tw))
        if g is None:
            g = groups[(th, tw)] = TileSizeGroup((th, tw), [], [], [], [], [], [], [], [], [0])
        g.first_tile.append(len(g.windows))
        g.n_tiles.append(len(wins))
        g.images.append(i)
        g.shapes.append((H, W))
        g.grids.append((max(H - crop[0] + stride[0] - 1, 0) // stride[0] + 1, max(W - crop[1] + stride[1] - 1, 0) // stride[1] + 1))
        g.windows.extend(wins)
        g.tile_image.extend([i] * len(wins))
        g.canvas_offsets.append(g.canvas_offsets[-1] + H * W)
    out = list(groups.values())
    for g in out:
        g.chunks = launch_chunks(len(g.windows), tiles_per_launch)
        tb = int(tile_bytes(g.tile_hw)) if callable(tile_bytes) else int(tile_bytes)
        a, used = 0, 0
        for k in range(len(g.images)):
            H, W = g.shapes[k]
            need = tb * g.n_tiles[k] + (int(pixel_bytes(g.images[k])) if callable(pixel_bytes) else int(pixel_bytes) * H * W)
            if k > a and flush_bytes is not None and used + need > flush_bytes:
                g.flush.append(_flush_group(g, a, k, tiles_per_launch))
                a, used = k, 0
            used += need
        g.flush.append(_flush_group(g, a, len(g.images), tiles_per_launch))
    return out


def _flush_group(g: TileSizeGroup, a: int, b: int, tiles_per_launch: int) -> FlushGroup:
    t0 = g.first_tile[a]
    t1 = g.first_tile[b - 1] + g.n_tiles[b - 1]
    return FlushGroup(a, b, t0, t1, [(t0 + i, t0 + j) for i, j in launch_chunks(t1 - t0, tiles_per_launch)])


def pack_scenes(scenes, device, fill=None) -> Tuple[torch.Tensor, List[Tuple[int, int]]]:
    """Images for a packed launch -> (one batch buffer, [(H, W)] per image).  A batch tensor ([B,3,H,W] f32 / [B,H,W,3] u8) is used in
    place; a list of u8 [H,W,3] or f32 [3,H,W] images of any sizes is copied once into a buffer padded to the largest size (tiles
    address it through ``scene_stride``).  The padding is never read -- windows stay inside each image -- and is left uninitialised
    unless ``fill`` is given."""
    if torch.is_tensor(scenes) and scenes.dim() == 4:
        u8 = scenes.dtype == torch.uint8
        buf = scenes if u8 else scenes.float()
        buf = buf.to(device).contiguous()
        H, W = (buf.shape[1], buf.shape[2]) if u8 else (buf.shape[2], buf.shape[3])
        return buf, [(int(H), int(W))] * buf.shape[0]
    scenes = [scenes] if torch.is_tensor(scenes) else list(scenes)
    if not scenes:
        raise ValueError("no images to segment")
    u8 = scenes[0].dtype == torch.uint8
    if any((s.dtype == torch.uint8) != u8 for s in scenes):
        raise ValueError("packed images must all be u8 [H,W,3] or all f32 [3,H,W]")
    if any(s.dim() != 3 or (s.shape[-1] if u8 else s.shape[0]) != 3 for s in scenes):
        raise ValueError("packed images are u8 [H,W,3] or f32 [3,H,W]")
    shapes = [(int(s.shape[0]), int(s.shape[1])) if u8 else (int(s.shape[1]), int(s.shape[2])) for s in scenes]
    Hm, Wm = max(h for h, _ in shapes), max(w for _, w in shapes)
    B = len(scenes)
    shape = (B, Hm, Wm, 3) if u8 else (B, 3, Hm, Wm)
    buf = torch.empty(shape, dtype=torch.uint8 if u8 else torch.float32, device=device)
    if fill is not None:
        buf.fill_(fill)
    for b, (s, (h, w)) in enumerate(zip(scenes, shapes)):
        if u8:
            buf[b, :h, :w] = s
        else:
            buf[b, :, :h, :w] = s
    return buf, shapes


def _scene_hw(s: torch.Tensor) -> Tuple[int, int]:
    """(H, W) of one packed image: u8 [H,W,3] or f32 [3,H,W] (``pack_scenes``)."""
    return (int(s.shape[0]), int(s.shape[1])) if s.dtype == torch.uint8 else (int(s.shape[-2]), int(s.shape[-1]))


def _images(scenes):
    """What ``pack_scenes`` takes, as a sequence of images: a single [3,H,W] / [H,W,3] tensor is one image."""
    return [scenes] if torch.is_tensor(scenes) and scenes.dim() == 3 else scenes


def _out_pixels(ori_shapes, i: int, scenes) -> int:
    """Pixels of image i's outputs: its ori_shape, or its own size."""
    o = ori_shapes[i] if ori_shapes is not None else None
    h, w = (int(o[0]), int(o[1])) if o is not None else _scene_hw(_images(scenes)[i])
    return h * w


def _ori_differs(ori_shapes, scenes) -> bool:
    """Whether some image's ``ori_shape`` is another size than the image."""
    return ori_shapes is not None and any(o is not None and tuple(o) != _scene_hw(s) for o, s in zip(ori_shapes, _images(scenes)))


def _out_sizes(ori_shapes, idx, shapes) -> List[Tuple[int, int]]:
    """The output size of every image of a flush group (images ``idx``, sizes ``shapes``): its ori_shape, or its own size."""
    return [tuple(shapes[n]) if ori_shapes is None or ori_shapes[i] is None else tuple(int(v) for v in ori_shapes[i])
            for n, i in enumerate(idx)]


@dataclass(frozen=True)
class TileGeometry:
    """What the patch grid makes of a tile of ``tile_hw``: the pad to whole patches, the patch grid, the padded size that a tile's
    logits are upsampled to, and the padded tile's offset of the window's top-left corner."""
    pad: Tuple[int, int, int, int]       # (l, r, t, b), engine.compute_padsize
    grid: Tuple[int, int]                # (gh, gw)
    up_hw: Tuple[int, int]
    pad_tl: Tuple[int, int]              # (t, l)


def tile_geometry(tile_hw: Tuple[int, int], patch: int) -> TileGeometry:
    th, tw = tile_hw
    l, r, t, b = compute_padsize(th, tw, patch)
    up_hw = (th + t + b, tw + l + r)
    return TileGeometry((l, r, t, b), (up_hw[0] // patch, up_hw[1] // patch), up_hw, (t, l))


# The routes of a tail (DESIGN.md section 5 'Route table'): a head on the tile logits (no canvas), a resized head on the tile logits (no
# canvas, another ori_shape), or the stitched canvas with one multi-image post-process per flush group / image by image.
HEAD, RESIZED_HEAD, CANVAS_MULTI, CANVAS_EACH = "head", "resized_head", "canvas_multi", "canvas_each"
# Test-time augmentation on (tta_scales / tta_flip): the views' class probabilities merged at the output size, by sg_tta_head on the
# views' tile logits (no canvas, no per-view planes) or view by view through the canvas and sg_tta_accumulate / sg_tta_finish.
TTA_HEAD, TTA_CANVAS = "tta_head", "tta_canvas"


@dataclass(frozen=True)
class TailRoute:
    route: str
    pixel_bytes: int                     # what the planner counts per image pixel; per OUTPUT pixel on RESIZED_HEAD


LABEL_HEADS = ("auto", "fused", "canvas")
PROB_HEADS = LABEL_HEADS
# How labels and the k best classes reach another ``ori_shape`` than the image's: "canvas" = stitch, resize the [Q,h,w] canvas to
# [Q,H,W], post-process; "fused" = sg_label_head_resized / sg_topk_head_resized, the resize inside the head and neither canvas.  The
# default stays "canvas" until the fused route has been measured to beat it by more than the run-to-run spread on the dataset shape
# (DESIGN.md section 5 'Heads at another ori_shape').
RESIZE_HEADS = ("canvas", "fused")
# What prob_head="auto" does beyond ops.POSTPROCESS_MAX_Q queries (up to there it is the canvas route): the fused head only where it was
# measured no slower than the canvas route at both Q = 130 and Q = 256.  It was slower at both (13.9 against 10.5 ms and 28.8 against
# 20.3 ms, profiles/r08_bench_prob_head.jsonl, DESIGN.md section 5 'Probability head'), so "auto" is the canvas route everywhere.
PROB_HEAD_AUTO_FUSED_BEYOND_MAX_Q = False


TTA_HEADS = ("auto", "fused", "canvas")
# What tta_head="auto" takes where the fused head can run: the fused head unless tools/bench_tta.py showed it slower than the canvas
# route.  It did, on every case of profiles/bench_tta.jsonl (2048 x 4608, scales 0.75 / 1.0 / 1.25): 4.65 against 4.29 ms at Q = 16 and
# 29.9 against 27.9 ms at Q = 64 with three views, 9.12 against 8.32 and 63.8 against 54.9 ms with six -- so "auto" is the canvas route,
# and "fused" is the choice for memory: 0.1 to 0.3 GB beyond the tile logits for labels where the canvas route takes 2.2 GB (Q = 16) or
# 8.6 GB (Q = 64) (DESIGN.md section 5 'Test-time augmentation').
TTA_AUTO_FUSED = False


TTA_TILE_GROUP = ("test-time augmentation under tile_group sharding is not built: every view has its own canvas bands, so a rank's band "
                  "of the output would need all views' tiles that map into it; run the views on whole images per rank")


TTA_PAMR = ("test-time augmentation together with PAMR is not built: the guide image would have to follow each view (resized and "
            "mirrored) and every view's canvas be refined before its probabilities are merged; use one or the other")


TTA_AREA = ("test-time augmentation together with area_thd is not built: the class areas would have to be counted on the merged "
            "arg-max and the mean probabilities filtered afterwards; use one or the other")


TTA_TOPK = ("top-k together with test-time augmentation is not built: the k best classes would have to be ranked on the merged mean "
            "probabilities, which the top-k head never sees; run predict_topk / topk= on an instance without tta_scales / tta_flip")


def tta_view_scene(scene: torch.Tensor, hw, flipped: bool) -> torch.Tensor:
    """One view of test-time augmentation: ``scene`` (u8 [H,W,3] or f32 [3,H,W]) resized to ``hw`` -- torch plumbing on the scene's
    device: f32, F.interpolate(bilinear, align_corners=False, antialias=False), a u8 scene rounded to nearest and clamped back to
    u8 -- and then mirrored along the width when ``flipped``.  At the scene's own size without flip: the scene object itself."""
    u8 = scene.dtype == torch.uint8
    v = scene
    if tuple(int(x) for x in hw) != _scene_hw(scene):
        x = (scene.permute(2, 0, 1) if u8 else scene).float().unsqueeze(0)
        x = torch.nn.functional.interpolate(x, size=tuple(int(v_) for v_ in hw), mode="bilinear", align_corners=False, antialias=False)[0]
        v = x.round().clamp_(0, 255).to(torch.uint8).permute(1, 2, 0) if u8 else x
    if flipped:
        v = torch.flip(v, dims=[1 if u8 else 2])
    return v if v is scene else v.contiguous()


PAMR_TILE_GROUP = ("PAMR under tile_group sharding is not built: a rank's canvas band would need a halo of pamr_steps * max(pamr_stride) "
                   "rows of its neighbours' logits; run PAMR on whole images per rank")


TOPK_TILE_GROUP = ("top-k under tile_group sharding is not built: each rank would run the head on its own canvas band and the [k,rows,W] "
                   "planes would be gathered (gather_bands); run top-k on whole images per rank")


AREA_TILE_GROUP = ("area_thd under tile_group sharding is not built: the class areas are a statistic of the whole image, so the counts of "
                   "the ranks' canvas bands would need an all-reduce before any band can be relabelled; run area_thd on whole images per rank")


AREA_TOPK = ("top-k together with area_thd is not built: the k best classes would have to skip the classes that area_thd drops, which the "
             "top-k head decides before the areas are known; run predict_topk / topk= on an instance without area_thd")


SIEVE_TILE_GROUP = ("min_region under tile_group sharding is not built: a region crosses the ranks' canvas bands, so each band would need a "
                    "halo and the roots on the band borders a union across the ranks; sieve whole images per rank")


SIEVE_TOPK = ("top-k together with min_region is not built: sieving plane 0 would leave the other planes describing pixels whose label has "
              "changed; run predict_topk / topk= on an instance without min_region")


REGIONS_TILE_GROUP = ("the region table under tile_group sharding is not built: a region crosses the ranks' canvas bands, so the roots on "
                      "the band borders would need a union across the ranks and the rows a merge; list the regions of whole images per rank")


class SegPipeline:
    # Every constructor option has its default here too, so an instance built without the constructor (the CPU tests' stubs) reads them.
    pamr_steps, pamr_stride = 0, (8, 16)      # PAMR off unless the constructor says otherwise
    area_thd = None                           # area_thd off likewise
    min_region, region_connectivity, region_fill = None, 4, "neighbour"      # the sieve off likewise
    label_head, prob_head, resize_head = "auto", "auto", "canvas"
    blend, blend_ramp = "uniform", None       # weighted window blending off likewise
    tta_scales, tta_flip, tta_head = None, False, "auto"      # test-time augmentation off likewise
    apply_ctd, apply_layer_fusion, layer_fusion_lambda = False, False, 0.5
    cross_tile_fusion = tile_group = upsampler = None

    def __init__(self, net: HipCLIP, text: torch.Tensor, query_idx: torch.Tensor, model_type: str = "SegEarth",
                 ignore_residual: bool = True, cls_token_lambda: float = 0.0, global_debias_factor: float = 0.0,
                 logit_scale: float = 50.0, prob_thd: float = 0.0, bg_idx: int = 0, apply_similarity_enhancement: bool = False,
                 upsampler=None, tiles_per_launch: int = 32, cross_tile_fusion: Optional[dict] = None, apply_ctd: bool = False,
                 tile_group=None, apply_layer_fusion: bool = False, layer_fusion_lambda: float = 0.5, label_head: str = "auto",
                 prob_head: str = "auto", pamr_steps: int = 0, pamr_stride=(8, 16), resize_head: str = "canvas", area_thd=None,
                 min_region=None, region_connectivity: int = 4, region_fill: str = "neighbour", blend: str = "uniform", blend_ramp=None,
                 tta_scales=None, tta_flip: bool = False, tta_head: str = "auto"):
        # Test-time augmentation (tta_scales=None and tta_flip=False = off, and then no call changes route, launches or bytes): every
        # image is run as the views ops.tta_views lists -- resized by each scale, and mirrored too with tta_flip; tta_flip alone means
        # scales (1.0,) -- each slid with this instance's stride / crop and tower options, and the views' class probabilities are averaged
        # at the output size before the arg-max and prob_thd (the definition: include/segearth_hip.h).  tta_head: "fused" = sg_tta_head
        # on the views' tile logits, "canvas" = view by view through the canvas and sg_tta_accumulate / sg_tta_finish, "auto" = what
        # was measured faster, the canvas route (TTA_AUTO_FUSED).  "fused" where the fused head cannot run is refused
        # (``tta_fused_reason``).  The views are refused with tile_group, PAMR, area_thd and top-k.
        if tta_head not in TTA_HEADS:
            raise ValueError(f"tta_head must be one of {TTA_HEADS}, got {tta_head!r}")
        self.tta_scales = None if tta_scales is None else tuple(
            float(s) for s in ([tta_scales] if isinstance(tta_scales, (int, float)) else tta_scales))
        self.tta_flip, self.tta_head = bool(tta_flip), tta_head
        if self.tta_on():
            ops.tta_views((64, 64), self.tta_scales, self.tta_flip)         # the scales and the number of views, before anything else
            if pamr_steps:
                raise ValueError(TTA_PAMR)
            if area_thd is not None:
                raise ValueError(TTA_AREA)
        # blend ("uniform" = off, and then no call changes route, launches or bytes): overlapping windows are combined by a weighted mean,
        # each tile weighted by a ramp ("linear" or "hann", ops.blend_ramp) of the pixel's distance to the tile's own window edges
        # (sg_stitch_blend; the definition: include/segearth_hip.h), which takes the step out of the stitched logits where a window starts
        # or ends.  ``blend_ramp``: the ramp's length R in pixels, None = the full window, max(1, min(tile_h, tile_w) // 2), resolved per
        # tile size (``_ramp``).  Labels only take sg_label_head_blend where the unweighted call takes sg_label_head (not with area_thd,
        # whose second pass gathers unweighted); everything else takes the canvas route with sg_stitch_blend in place of sg_stitch.
        self.blend, self.blend_ramp = ops.blend_args(blend, blend_ramp)
        # min_region (None = off, and then no call changes route, launches or bytes): the connected regions of the FINAL labels -- after
        # prob_thd and area_thd, at ori_shape, whatever route the tail took -- that have fewer than min_region pixels are sieved out
        # (sg_sieve; the definition: include/segearth_hip.h): region_fill "neighbour" gives them the label of their largest adjacent kept
        # region, "bg" turns the non-background ones into bg_idx; region_connectivity 4 or 8.  One sg_sieve call per image or per flush
        # group.  Probabilities that are returned beside the labels are left as they are.
        _, self.region_connectivity, self.region_fill = ops.sieve_args(1 if min_region is None else min_region, region_connectivity, region_fill)
        self.min_region = min_region
        if resize_head not in RESIZE_HEADS:
            raise ValueError(f"resize_head must be one of {RESIZE_HEADS}, got {resize_head!r}")
        # labels / top-k at another ori_shape than the image's (RESIZE_HEADS); PAMR and whole-image inference keep the canvas route
        self.resize_head = resize_head
        if label_head not in LABEL_HEADS:
            raise ValueError(f"label_head must be one of {LABEL_HEADS}, got {label_head!r}")
        if prob_head not in PROB_HEADS:
            raise ValueError(f"prob_head must be one of {PROB_HEADS}, got {prob_head!r}")
        # PAMR (pixel-adaptive mask refinement, sg_pamr): ``pamr_steps`` refinement steps over the dilations ``pamr_stride`` on the stitched
        # logits, after the resize to ori_shape and before the post-process; 0 = off (the upstream option names).  With PAMR on, every
        # tail that returns labels or probabilities takes the canvas route whatever label_head / prob_head say: stitch, the resize if any,
        # PAMR, post-process.  ``forward_slide`` / ``forward_slide_many`` / ``forward_feature`` return the unrefined logits.
        self.pamr_steps = int(pamr_steps)
        self.pamr_stride = ops.pamr_dilations(pamr_stride)[0]
        if not 0 <= self.pamr_steps <= ops.PAMR_MAX_STEPS:
            raise ValueError(f"pamr_steps must lie in [0, {ops.PAMR_MAX_STEPS}], got {pamr_steps!r}")
        self._check_sharding(tile_group is not None)            # PAMR is refused before anything of the net is touched; area_thd below
        # the tail that returns class probabilities too (``probs_from_tiles``): "canvas" = stitch + postprocess, "fused" = sg_prob_head
        # (no canvas, any Q, the same bytes), "auto" = see ``fused_prob_head``
        self.prob_head = prob_head
        # the labels-only tail (``labels_from_tiles``): "canvas" = stitch + postprocess through the [Q,H,W] canvas, "fused" = sg_label_head
        # (no canvas, any Q), "auto" = the canvas wherever it works (Q <= 64) and the fused head beyond
        self.label_head = label_head
        self.apply_layer_fusion, self.layer_fusion_lambda = bool(apply_layer_fusion), float(layer_fusion_lambda)
        self.net = net
        self.visual = net.visual
        self.device = self.visual.device
        self.text = text.to(device=self.device, dtype=torch.float32).contiguous()
        self.query_idx = query_idx.to(device=self.device, dtype=torch.int32).contiguous()
        self.num_queries = int(self.text.shape[0])
        self.num_classes = int(query_idx.max()) + 1
        self.model_type = model_type
        self.ignore_residual = ignore_residual
        self.cls_token_lambda = float(cls_token_lambda)
        self.global_debias_factor = float(global_debias_factor)
        self.logit_scale, self.prob_thd, self.bg_idx = float(logit_scale), float(prob_thd), int(bg_idx)
        self.apply_similarity_enhancement = apply_similarity_enhancement
        self.upsampler = upsampler
        self.tiles_per_launch = int(tiles_per_launch)
        # opt-in: the reference ships CrossTileFusion but never calls it; kwargs of its constructor
        self.cross_tile_fusion = cross_tile_fusion
        self.apply_ctd = bool(apply_ctd)                 # Cluster-Then-Debias (segmentor.py:339-365), SegmentorEx only
        # Tile sharding over ranks is opt-in (None = off, "world" = the default process group, or a ProcessGroup whose ranks
        # all hold the SAME scene).  It is never inferred from torch.distributed being initialised: under the reference's own
        # multi-GPU launch every rank holds a different image.
        self.tile_group = tile_group
        # area_thd (the upstream option name; None = off, and then no call changes route, launches or bytes): per image, a class whose
        # arg-max area is at most area_thd times the non-background area is removed and its pixels go to the best remaining class (the
        # definition: include/segearth_hip.h).  Every tail that returns labels or probabilities then decides twice: the first pass is
        # the route's own kernel with prob_thd = 0 (its labels are the plain arg-max), then sg_class_area -> sg_area_keep on the device,
        # then sg_area_filter_probs on the probabilities (a scratch [K,H,W] where only labels are wanted) or, on the fused label head,
        # sg_area_relabel: no canvas, no probability planes, 12 bytes per pixel instead of 8 (DESIGN.md section 5 'Route table').
        self.area_thd = None if area_thd is None else float(area_thd)
        if self.area_thd is not None:
            ops.area_args("area_thd", self.num_classes, self.bg_idx, self.area_thd)
        self._check_sharding(tile_group is not None)
        if self.tta_on() and self.tta_head == "fused" and self.tta_fused_reason() is not None:
            raise ValueError(f"tta_head='fused' cannot serve this instance: {self.tta_fused_reason()}; use tta_head='canvas' or 'auto'")

    def _stitch(self, tile_logits, windows, up_hw, pad_tl, canvas_hw, ramp=None):
        if ramp is not None:
            return ops.stitch_blend(tile_logits, windows, up_hw, pad_tl, canvas_hw, ramp)
        return ops.stitch(tile_logits, windows, up_hw, pad_tl, canvas_hw)

    def _stitched(self, tile_hw, *args):
        """``_stitch`` of windows of ``tile_hw``, blended when ``blend`` is on (the weights depend on the position inside a tile's own
        window, so a band's shifted windows give the whole canvas's rows)."""
        ramp = self._ramp(tile_hw)
        return self._stitch(*args) if ramp is None else self._stitch(*args, ramp)

    def _ramp(self, tile_hw):
        """The device ramp table of ``blend`` for windows of ``tile_hw`` (R = ``blend_ramp``, or half the window's smaller side); None
        with blend = "uniform": every caller then makes the unweighted call.  A caller that only has the tile logits and windows on the
        device passes None for ``tile_hw`` and must have set ``blend_ramp``."""
        if self.blend == "uniform":
            return None
        if self.blend_ramp is None and tile_hw is None:
            raise ValueError("blend: the window size is not known here, so blend_ramp=None cannot be resolved; pass tile_hw= or set blend_ramp")
        R = self.blend_ramp if self.blend_ramp is not None else max(1, min(int(tile_hw[0]), int(tile_hw[1])) // 2)
        return ops.blend_table(self.blend, R, self.device)

    # -- which tail runs: one decision (DESIGN.md section 5 'Route table') ----------------------------------------------
    def fused_label_head(self) -> bool:
        """Whether the labels-only tail runs the fused head (sg_label_head) instead of the canvas path: "auto" = the canvas wherever it
        works (Q <= 64) and the fused head beyond.  PAMR refines the canvas, so there has to be one."""
        return self.pamr_steps == 0 and (self.label_head == "fused" or (
            self.label_head == "auto" and self.num_queries > ops.POSTPROCESS_MAX_Q))

    def fused_prob_head(self) -> bool:
        """Whether the tail that returns probabilities and labels runs the fused head (sg_prob_head) instead of the canvas path.  "auto"
        is the canvas up to 64 queries and follows the measurement beyond (PROB_HEAD_AUTO_FUSED_BEYOND_MAX_Q)."""
        return self.pamr_steps == 0 and (self.prob_head == "fused" or (
            self.prob_head == "auto" and PROB_HEAD_AUTO_FUSED_BEYOND_MAX_Q and self.num_queries > ops.POSTPROCESS_MAX_Q))

    def fused_resize_head(self) -> bool:
        """Whether labels / top-k at another ``ori_shape`` run the resized heads (no canvas) instead of stitch + resize + post-process."""
        return self.resize_head == "fused" and self.pamr_steps == 0 and self.area_thd is None

    def tta_on(self) -> bool:
        return self.tta_scales is not None or bool(self.tta_flip)

    def tta_fused_reason(self):
        """Why sg_tta_head cannot serve this instance, or None: it stitches unweighted patch-grid tile logits of at most 64 queries."""
        if self.num_queries > ops.TTA_MAX_Q:
            return f"{self.num_queries} queries exceed the fused head's {ops.TTA_MAX_Q}"
        if self.blend != "uniform":
            return f"blend={self.blend!r} needs the weighted stitch, which only the canvas route has"
        if self.upsampler is not None:
            return "the JBU upsampler's per-pixel tile logits take the canvas route"
        return None

    def tta_fused(self) -> bool:
        """Whether the merge of the views runs sg_tta_head (sliding-window inference; whole-image inference has no tiles)."""
        return self.tta_head != "canvas" and self.tta_fused_reason() is None and (self.tta_head == "fused" or TTA_AUTO_FUSED)

    def topk_k(self, topk) -> int:
        """``topk`` checked against what sg_topk_head takes: 1 .. min(ops.TOPK_MAX, the number of classes)."""
        if self.area_thd is not None:
            raise ValueError(AREA_TOPK)
        if self.min_region is not None:
            raise ValueError(SIEVE_TOPK)
        if self.tta_on():
            raise ValueError(TTA_TOPK)
        k = int(topk)
        if not 1 <= k <= min(ops.TOPK_MAX, self.num_classes):
            raise ValueError(f"topk must lie in [1, min({ops.TOPK_MAX}, {self.num_classes} classes)], got {topk!r}")
        return k

    def _wanted(self, where: str, want_probs: bool, topk: int, sharded: bool) -> Tuple[str, int]:
        """What a tail is asked for: ("labels" | "probs" | "topk", k)."""
        if not topk:
            return ("probs" if want_probs else "labels"), 0
        if want_probs:
            raise ValueError(f"{where}: topk and want_probs exclude each other (topk returns the k best class probabilities)")
        if sharded:
            raise ValueError(TOPK_TILE_GROUP)
        return "topk", self.topk_k(topk)

    def _check_sharding(self, sharded: bool) -> None:
        if sharded and self.pamr_steps > 0:
            raise ValueError(PAMR_TILE_GROUP)
        if sharded and self.area_thd is not None:
            raise ValueError(AREA_TILE_GROUP)
        if sharded and self.min_region is not None:
            raise ValueError(SIEVE_TILE_GROUP)
        if sharded and self.tta_on():
            raise ValueError(TTA_TILE_GROUP)

    def _canvas_bytes(self) -> int:
        """Per pixel of a canvas route: the [Q,H,W] canvas, and with area_thd the probability planes and labels, which then always exist."""
        return 4 * self.num_queries + (0 if self.area_thd is None else 4 * self.num_classes + 8)

    def tail_route(self, want: str, k: int = 0, given: bool = False, differs: bool = False) -> TailRoute:
        """THE route decision.  ``want``: "labels", "probs" or "topk" (then ``k``); ``differs``: some ``ori_shape`` is another size than
        its image; ``given``: some ``ori_shape`` is given at all -- the packed labels-only tail takes the fused head only when none is,
        an ``ori_shape`` equal to the image's size keeps the canvas there."""
        if self.tta_on():                      # per OUTPUT pixel: labels and conf, the mean planes; the canvas route also one view's
            K = self.num_classes               # planes and its resized canvas.  The views' tile logits come on top of either.
            if self.tta_fused():
                return TailRoute(TTA_HEAD, 8 + (4 * K if want == "probs" else 0))
            return TailRoute(TTA_CANVAS, 8 + 8 * K + 4 * self.num_queries)
        blended = self.blend != "uniform"      # only the label head has a blended form, and sg_area_relabel gathers unweighted
        if self.pamr_steps == 0:
            if want == "topk" and not differs and not blended:
                return TailRoute(HEAD, 8 * k)
            if want == "probs" and not differs and not blended and self.fused_prob_head():
                return TailRoute(HEAD, 4 * self.num_classes + 8)
            if want == "labels" and not given and not differs and self.fused_label_head() and not (blended and self.area_thd is not None):
                return TailRoute(HEAD, 8 if self.area_thd is None else 12)
            if want != "probs" and differs and not blended and self.fused_resize_head():
                return TailRoute(RESIZED_HEAD, 8 * k if want == "topk" else 8)
        return TailRoute(CANVAS_MULTI if self.num_queries <= ops.POSTPROCESS_MAX_Q else CANVAS_EACH, self._canvas_bytes())

    # -- the tails ------------------------------------------------------------------------------------------------------
    def refine(self, canvas: torch.Tensor, guide: torch.Tensor) -> torch.Tensor:
        """PAMR on one image's logits [Q,H,W], in place where they are a contiguous f32 tensor.  ``guide``: the image (u8 [H,W,3] or
        normalised f32 [3,H,W]); at another size than the logits (an ``ori_shape`` resize) its planes are resized by the same
        ``resize_bilinear``.  Returns the refined logits; with ``pamr_steps = 0`` the logits as they came."""
        if self.pamr_steps <= 0:
            return canvas
        g = ops.scene_planes(guide)
        if tuple(g.shape[1:]) != tuple(canvas.shape[1:]):
            g = ops.resize_bilinear(g, tuple(canvas.shape[1:]))
        inplace = canvas.dtype == torch.float32 and canvas.is_contiguous()
        return ops.pamr(canvas, g, self.pamr_steps, self.pamr_stride, inplace=inplace)

    def _area_keep(self, labels, image_pixels=None):
        """area_thd, between the passes: the class areas of the first pass's labels (one image, or the flat labels of a flush group with
        ``image_pixels``) -> keep; two launches, nothing comes to the host."""
        counts = ops.class_area(labels, self.num_classes) if image_pixels is None else ops.class_area_multi(labels, image_pixels, self.num_classes)
        return ops.area_keep(counts, self.bg_idx, self.area_thd)

    def area_filter_first_pass(self, probs, labels):
        """The second decision of area_thd for one image whose first pass (``prob_thd = 0``) left probs f32 [K,H,W] and labels int64
        [1,H,W]: count, keep, filter -- both tensors IN PLACE."""
        ops.area_filter_probs(probs, labels, self._area_keep(labels), self.prob_thd, self.bg_idx)
        return probs, labels

    def area_filter_first_pass_multi(self, probs, flat, out_hw):
        """``area_filter_first_pass`` for a flush group: the flat outputs of sg_postprocess_multi / sg_prob_head_multi, one launch each."""
        keep = self._area_keep(flat, [h * w for h, w in out_hw])
        ops.area_filter_probs_multi(probs, flat, keep, out_hw, self.prob_thd, self.bg_idx)

    def sieve(self, labels: torch.Tensor, image_hw=None) -> torch.Tensor:
        """min_region, the last step on final labels, IN PLACE: one label map int64 [1,H,W] / [H,W], or with ``image_hw`` the flat buffer
        of a flush group's maps (one sg_sieve call for the group).  With ``min_region = None`` the labels as they came."""
        if self.min_region is not None:
            hw = [tuple(labels.shape[-2:])] if image_hw is None else image_hw
            ops.sieve_flat(labels.view(-1), hw, self.min_region, self.region_connectivity, self.region_fill, self.bg_idx)
        return labels

    def regions(self, labels, image_hw=None, conf=None, min_area: int = 1, include_bg: bool = False, connectivity=None, skip_label=None,
                max_regions=None, want_map: bool = False) -> dict:
        """The region table of final labels (sg_regions; ``ops.regions`` describes the result): one label map int64 [1,H,W] / [H,W], a
        list of maps, or with ``image_hw`` the flat buffer of a flush group's maps -- one sg_regions call each.  ``conf``: None or f32
        of the same layout.  ``connectivity`` defaults to ``region_connectivity``, ``skip_label`` to ``bg_idx`` unless ``include_bg``.
        The labels are only read.  ``tile_group`` sharding is refused."""
        if self.tile_group is not None:
            raise ValueError(REGIONS_TILE_GROUP)
        connectivity = self.region_connectivity if connectivity is None else connectivity
        if skip_label is None and not include_bg:
            skip_label = int(self.bg_idx)
        if image_hw is not None:
            return ops.regions_flat(labels.view(-1), image_hw, None if conf is None else conf.view(-1), connectivity, min_area, skip_label,
                                    max_regions, want_map)
        return ops.regions(labels, conf, connectivity, min_area, skip_label, max_regions, want_map)

    def _image_tail(self, route: str, want: str, k: int, tile_logits, windows, up_hw, pad_tl, canvas_hw, out_hw, guide, ramp=None):
        """``_image_tail_unsieved`` and then, with min_region set, the sieve on its labels (top-k is refused with min_region)."""
        out = self._image_tail_unsieved(route, want, k, tile_logits, windows, up_hw, pad_tl, canvas_hw, out_hw, guide, ramp)
        if self.min_region is not None and want != "topk":
            self.sieve(out[1] if want == "probs" else out)
        return out

    def _image_tail_unsieved(self, route: str, want: str, k: int, tile_logits, windows, up_hw, pad_tl, canvas_hw, out_hw, guide, ramp=None):
        """One image's (or one canvas band's) tile logits [T,Q,gh,gw] + windows [T,4] -> labels int64 [1,H,W], (probs f32 [K,H,W],
        labels) or (classes int32 [k,H,W], probs f32 [k,H,W]) on ``route``, (H, W) = ``out_hw``.  ``ramp``: the table of ``_ramp`` for
        these tiles (None: the unweighted stitch); ``tail_route`` sends a blended tail to HEAD for plain labels only."""
        args = (tile_logits, windows, up_hw, pad_tl, canvas_hw)
        if ramp is not None and (route == RESIZED_HEAD or (route == HEAD and (want != "labels" or self.area_thd is not None))):
            raise ValueError("blend: only the plain label head has a blended form; everything else takes the canvas route")
        if route == RESIZED_HEAD:
            post = (out_hw, self.query_idx, self.num_classes, self.logit_scale)
            return ops.topk_head_resized(*args, *post, k) if want == "topk" else ops.label_head_resized(*args, *post, self.prob_thd, self.bg_idx)
        if route == HEAD:
            post = (self.query_idx, self.num_classes, self.logit_scale)
            if ramp is not None:
                return ops.label_head_blend(*args, *post, self.prob_thd, self.bg_idx, ramp)
            if want == "topk":
                return ops.topk_head(*args, *post, k)
            area = self.area_thd is not None
            thd = 0.0 if area else self.prob_thd                  # area_thd: the first pass is the plain arg-max
            if want == "probs":
                probs, labels = ops.prob_head(*args, *post, thd, self.bg_idx)
                return self.area_filter_first_pass(probs, labels) if area else (probs, labels)
            if not area:
                return ops.label_head(*args, *post, thd, self.bg_idx)
            labels, conf = ops.label_head(*args, *post, thd, self.bg_idx, want_conf=True)
            return ops.area_relabel(*args, *post, self.prob_thd, self.bg_idx, self._area_keep(labels), conf, labels)
        canvas = self._stitch(*args) if ramp is None else self._stitch(*args, ramp)      # stitch -> resize -> PAMR -> post-process
        if tuple(out_hw) != tuple(canvas_hw):
            canvas = ops.resize_bilinear(canvas, out_hw)
        if self.pamr_steps > 0:
            if guide is None:
                raise ValueError("PAMR needs the image of the canvas as guidance: pass guide= (a canvas band has none: " + PAMR_TILE_GROUP + ")")
            canvas = self.refine(canvas, guide)
        probs, labels = self.postprocess(canvas, want_probs=want != "labels")
        if want == "topk":
            return ops.topk_from_probs(probs, self.query_idx, k)
        return (probs, labels) if want == "probs" else labels

    def labels_from_tiles(self, tile_logits, windows, up_hw, pad_tl, canvas_hw, guide=None, tile_hw=None):
        """The labels-only tail of one image or canvas band (a canvas with shifted windows) -> labels int64 [1,H,W].  ``tile_hw``: the
        window size, which ``blend`` resolves its ramp from (``_ramp``); the same in the two tails below."""
        return self._image_tail(self.tail_route("labels").route, "labels", 0, tile_logits, windows, up_hw, pad_tl, canvas_hw, canvas_hw, guide,
                                self._ramp(tile_hw))

    def probs_from_tiles(self, tile_logits, windows, up_hw, pad_tl, canvas_hw, guide=None, tile_hw=None):
        """-> (probs f32 [K,H,W], labels int64 [1,H,W]) at the scene's own size; every route returns the same bytes."""
        return self._image_tail(self.tail_route("probs").route, "probs", 0, tile_logits, windows, up_hw, pad_tl, canvas_hw, canvas_hw, guide,
                                self._ramp(tile_hw))

    def topk_from_tiles(self, tile_logits, windows, up_hw, pad_tl, canvas_hw, k: int, guide=None, tile_hw=None):
        """-> (classes int32 [k,H,W], probs f32 [k,H,W]): the k best classes of every pixel in descending probability."""
        k = self.topk_k(k)
        return self._image_tail(self.tail_route("topk", k).route, "topk", k, tile_logits, windows, up_hw, pad_tl, canvas_hw, canvas_hw, guide,
                                self._ramp(tile_hw))

    def topk_from_logits(self, seg_logits, k: int, guide=None):
        """The canvas route to the k best classes, for logits [Q,H,W] that already exist (whole-image inference): PAMR when on,
        post-process, ``ops.topk_from_probs``."""
        k = self.topk_k(k)
        if self.pamr_steps > 0:
            seg_logits = self.refine(seg_logits.float().contiguous(), guide)
        return ops.topk_from_probs(self.postprocess(seg_logits, want_probs=True)[0], self.query_idx, k)

    def _postprocess_multi(self, canvases, chw, ohw, want_probs):
        """ops.postprocess_multi for a flush group -> (probs or Nones, labels, flat labels); with area_thd the first pass writes the
        probabilities whether wanted or not (a scratch then), and the group is counted, decided and filtered with one launch each."""
        if self.area_thd is None:
            return ops.postprocess_multi(canvases, chw, self.query_idx, self.num_classes, self.logit_scale, self.prob_thd, self.bg_idx, ohw,
                                         want_probs, flat_labels=True)
        prb, lab, flat, probs = ops.postprocess_multi(canvases, chw, self.query_idx, self.num_classes, self.logit_scale, 0.0, self.bg_idx, ohw,
                                                      True, flat_labels=True, flat_probs=True)
        self.area_filter_first_pass_multi(probs, flat, ohw)
        return (prb if want_probs else [None] * len(lab)), lab, flat

    def _postprocess_each(self, views, ohw, imgs, want_probs):
        """The canvases of a flush group image by image -- resize, PAMR when on, ``postprocess`` -> (probs or Nones, labels, flat labels):
        the label maps are copied into one flat buffer and returned as views of it."""
        prb, lab = [], []
        for c, hw, im in zip(views, ohw, imgs):
            if hw != tuple(c.shape[1:]):
                c = ops.resize_bilinear(c, hw)
            if self.pamr_steps > 0:
                c = self.refine(c, im.to(self.device))
            p_, l_ = self.postprocess(c, want_probs=want_probs)
            prb.append(p_); lab.append(l_.reshape(-1))
        flat = torch.cat(lab)
        return prb, ops.flat_views(flat, 1, ohw), flat

    def _group_ramp(self, group):
        """``_ramp`` for a flush group of ``_packed_tiles``: its windows (host tuples) all have the group's one tile size."""
        y1, y2, x1, x2 = group[2][0]
        return self._ramp((y2 - y1, x2 - x1))

    def _group_tail(self, route: str, want: str, k: int, group, ohw, imgs):
        """``_group_tail_unsieved`` and then, with min_region set, ONE sg_sieve call over the group's flat labels (the label maps are
        views of that buffer)."""
        prb, lab, flat = self._group_tail_unsieved(route, want, k, group, ohw, imgs)
        if self.min_region is not None and want != "topk":
            self.sieve(flat, ohw)
        return prb, lab, flat

    def _group_tail_unsieved(self, route: str, want: str, k: int, group, ohw, imgs):
        """One flush group of ``_packed_tiles`` on ``route`` -> (list of probs or Nones, list of labels, flat labels), or for top-k
        (list of probs [k,H,W], list of classes [k,H,W], None).  ``ohw``: the output size per image; ``imgs``: the images (PAMR's guides)."""
        idx, shapes = group[0], group[6]
        args, post = group[1:], (self.query_idx, self.num_classes, self.logit_scale)
        ramp = self._group_ramp(group)                            # None unless blend is on; tail_route then gives HEAD to plain labels only
        if route == RESIZED_HEAD and ohw == shapes:               # no image of this group differs: what runs without the option
            route = self.tail_route(want, k).route
        if route == RESIZED_HEAD:
            if want == "topk":
                cls, prb = ops.topk_head_resized_multi(*args, ohw, *post, k)
                return prb, cls, None
            lab, flat = ops.label_head_resized_multi(*args, ohw, *post, self.prob_thd, self.bg_idx)
            return [None] * len(idx), lab, flat
        if route == HEAD:
            if want == "topk":
                cls, prb = ops.topk_head_multi(*args, *post, k)
                return prb, cls, None
            area = self.area_thd is not None
            thd = 0.0 if area else self.prob_thd                  # area_thd: the first pass is the plain arg-max
            if want == "probs":
                prb, lab, flat, *probs = ops.prob_head_multi(*args, *post, thd, self.bg_idx, flat_probs=area)
                if area:
                    self.area_filter_first_pass_multi(probs[0], flat, shapes)
                return prb, lab, flat
            if ramp is not None:
                lab, flat = ops.label_head_blend_multi(*args, *post, thd, self.bg_idx, ramp)
                return [None] * len(idx), lab, flat
            lab, flat, *conf = ops.label_head_multi(*args, *post, thd, self.bg_idx, want_conf=area, flat_conf=area)
            if area:                                              # 12 bytes per pixel: labels and conf, no canvas, no probability planes
                ops.area_relabel_multi(*args, *post, self.prob_thd, self.bg_idx, self._area_keep(flat, [h * w for h, w in shapes]), conf[0], flat)
            return [None] * len(idx), lab, flat
        canvases, views = ops.stitch_multi(*args) if ramp is None else ops.stitch_blend_multi(*args, ramp)
        if route == CANVAS_MULTI and (self.pamr_steps == 0 or ohw == shapes):
            if self.pamr_steps > 0:                               # PAMR comes after the resize: a group that holds one goes image by image
                for c, im in zip(views, imgs):
                    self.refine(c, im.to(self.device))
            prb, lab, flat = self._postprocess_multi(canvases, shapes, ohw, want != "labels")
        else:
            prb, lab, flat = self._postprocess_each(views, ohw, imgs, want != "labels")
        if want == "topk":
            pairs = [ops.topk_from_probs(p, self.query_idx, k) for p in prb]
            return [p for _, p in pairs], [c for c, _ in pairs], None
        return prb, lab, flat

    def _pre_head(self, tok, cls):
        """Global debias (+ CTD) when they cannot stay fused in the logits kernel: returns (tokens, remaining debias factor)."""
        f = self.global_debias_factor if cls is not None else 0.0
        if not self.apply_ctd or cls is None:
            return tok, f
        if f != 0:                                            # reference order: global debias, then cluster on the debiased features
            tok = ops.global_debias(tok, cls, f)
        tok, _ = ops.ctd_debias(tok, cls, eps=1.1, min_samples=11, factor=-1.5, want_labels=False, normalize_cls=True)
        return tok, 0.0

    # -- per-tile logits -----------------------------------------------------------------------------------
    def _tile_geometry(self, tile_hw) -> TileGeometry:
        return tile_geometry(tile_hw, self.visual.cfg.patch)

    def _forward_opts(self):
        return self.visual.forward_opts(self.model_type, self.ignore_residual, self.apply_similarity_enhancement, self.apply_layer_fusion,
                                        self.layer_fusion_lambda)

    def _fusion_args(self) -> Tuple[int, str, float]:
        """(boundary width, mode, strength) of cross-tile fusion: the constructor kwargs of the reference's CrossTileFusion."""
        cf = self.cross_tile_fusion
        return cf.get("cache_boundary_width", 2), cf.get("fusion_mode", "weighted"), cf.get("fusion_strength", 0.3)

    def _tower(self, scene, win, tile_hw, chunks, scene_index=None):
        """The tower over the launch ``chunks`` [a, z) of the windows ``win`` -> (cls or None, tok) of all of them, concatenated."""
        opts = self._forward_opts()
        cls_all, tok_all = [], []
        for a, z in chunks:
            c_, t_ = self.visual.forward_tiles(scene, win[a:z], tile_hw, opts, None if scene_index is None else scene_index[a:z])
            cls_all.append(c_); tok_all.append(t_)
        return (None if cls_all[0] is None else torch.cat(cls_all, 0)), torch.cat(tok_all, 0)

    def _head_logits(self, tok, cls, scene, win, tile_hw, scene_index=None):
        """Tokens -> logits [T,Q,gh,gw] (per-pixel [T,Q,H',W'] with an upsampler): global debias and CTD, then the upsampler's logits tail
        (segmentor.py:368-372: tokens -> fusion -> JBU -> logits) or the cosine logits on the patch grid."""
        geo = self._tile_geometry(tile_hw)
        tok, f = self._pre_head(tok, cls)
        if self.upsampler is not None:
            return self.upsampler.logits(tok, cls, scene, win, tile_hw, (geo.pad[0], geo.pad[2]), geo.grid, self.text, f, self.cls_token_lambda,
                                         scene_index, padded_hw=geo.up_hw)
        lg = ops.cosine_logits(tok, cls, self.text, f, self.cls_token_lambda if cls is not None else 0.0)
        return lg.reshape(win.shape[0], self.num_queries, *geo.grid)

    def _logits_by_chunk(self, scene, win, tile_hw, chunks, scene_index=None):
        """Tower and head launch chunk by launch chunk: the tiles are independent (no cross-tile fusion)."""
        opts = self._forward_opts()
        outs = []
        for a, z in chunks:
            si = None if scene_index is None else scene_index[a:z]
            cls, tok = self.visual.forward_tiles(scene, win[a:z], tile_hw, opts, si)
            outs.append(self._head_logits(tok, cls, scene, win[a:z], tile_hw, si))
        return torch.cat(outs, 0) if len(outs) > 1 else outs[0]

    def tile_logits(self, scene: torch.Tensor, windows: Sequence[Tuple[int, int, int, int]], tile_hw: Tuple[int, int],
                    scene_index: Optional[torch.Tensor] = None, grid_of_tiles: Optional[Tuple[int, int]] = None) -> torch.Tensor:
        """-> [T, Q, gh, gw] patch-grid logits (or [T, Q, H', W'] per-pixel logits with the JBU upsampler)."""
        win = torch.tensor(list(windows), dtype=torch.int32, device=self.device).reshape(-1, 4)
        chunks = launch_chunks(win.shape[0], self.tiles_per_launch)
        if self.cross_tile_fusion is None or grid_of_tiles is None or grid_of_tiles[0] * grid_of_tiles[1] <= 1:
            return self._logits_by_chunk(scene, win, tile_hw, chunks, scene_index)
        # boundary fusion couples neighbouring tiles: run the tower over the whole scene first, fuse, then the head
        cls, tok = self._tower(scene, win, tile_hw, chunks, scene_index)
        tok = ops.cross_tile_fusion(tok, grid_of_tiles[0], grid_of_tiles[1], *self._tile_geometry(tile_hw).grid, *self._fusion_args())
        return self._head_logits(tok, cls, scene, win, tile_hw, scene_index)

    # -- reference forward_slide -----------------------------------------------------------------------------
    def _geometry(self, scene, stride, crop):
        H, W = _scene_hw(scene)
        stride = (stride, stride) if isinstance(stride, int) else tuple(stride)
        crop = (crop, crop) if isinstance(crop, int) else tuple(crop)
        wins = tile_windows(H, W, stride, crop)
        tile_hw = (wins[0][1] - wins[0][0], wins[0][3] - wins[0][2])
        geo = self._tile_geometry(tile_hw)
        hg = max(H - crop[0] + stride[0] - 1, 0) // stride[0] + 1
        wg = max(W - crop[1] + stride[1] - 1, 0) // stride[1] + 1
        return H, W, stride, crop, wins, tile_hw, geo.pad_tl, geo.up_hw, (hg, wg)

    def forward_slide(self, scene: torch.Tensor, stride, crop, ori_shape=None, group=None) -> torch.Tensor:
        """scene: f32 [3,H,W] normalised planes or u8 [H,W,3].  Returns logits [1,Q,H_ori,W_ori] (on every rank of the tile
        group when sharding is on: ``group`` overrides ``self.tile_group``; None = this process does the whole scene)."""
        H, W, stride, crop, wins, tile_hw, pad_tl, up_hw, grid = self._geometry(scene, stride, crop)
        group = resolve_tile_group(group if group is not None else self.tile_group)
        if group is None:
            tl = self.tile_logits(scene, wins, tile_hw, grid_of_tiles=grid)
            win_dev = torch.tensor(wins, dtype=torch.int32, device=self.device)
            canvas = self._stitched(tile_hw, tl, win_dev, up_hw, pad_tl, (H, W))
        else:
            band, y0, yb = self.sharded_canvas_band(scene, stride, crop, group)
            canvas = self.gather_bands(band, yb, H, group)
        if ori_shape is not None and tuple(ori_shape) != (H, W):
            canvas = ops.resize_bilinear(canvas, tuple(ori_shape))
        return canvas.unsqueeze(0)

    def sharded_canvas_band(self, scene, stride, crop, group):
        """``sharded_band_tiles`` stitched -> (this rank's band of the canvas, its first row, the boundaries of every rank's band)."""
        tiles, w_band, up_hw, pad_tl, hw, y0, yb = self.sharded_band_tiles(scene, stride, crop, group)
        if hw[0] <= 0:
            return tiles.new_zeros((self.num_queries, 0, hw[1])), y0, yb
        return self._stitched(self._band_tile_hw(scene, stride, crop), tiles, w_band, up_hw, pad_tl, hw), y0, yb

    def _band_tile_hw(self, scene, stride, crop):
        """The window size of a scene whose band tiles are at hand (``sharded_band_tiles`` does not return it); only ``blend`` asks."""
        return None if self.blend == "uniform" else self._geometry(scene, stride, crop)[5]

    def sharded_band_tiles(self, scene, stride, crop, group):
        """Tiles partitioned over the ranks of ``group`` -> this rank's band of the canvas, as what the stitch takes: (tile logits of the tiles
        that overlap the band, their windows in band coordinates, up_hw, pad_tl, (rows, W), first row, band boundaries of all ranks);
        rows = 0 for a rank without a band.  Patch-grid logits (44 kB per tile) are rebuilt everywhere with ONE all-gather (RCCL over xGMI);
        per-pixel logits (upsampler: 16-32 MB per tile) travel point to point, only the tiles that straddle a band edge.  Either way each
        rank stitches ONLY its own band, so the tail scales with the ranks too.  The stitch itself is identical given identical tile
        logits (write-once: the covering tiles are averaged in raster order, and all of them are present); the tile logits of a rank
        equal the single process's bit for bit in parity mode (f32: tests/test_gpu_distributed.py), while the 2-byte modes may take a
        different kernel path for a different launch size (few tiles per launch: 128 x 128 GEMM tiles and a separate LayerNorm pass,
        DESIGN.md section 4), i.e. differ by 2-byte rounding (bounded in the same test file)."""
        H, W, stride, crop, wins, tile_hw, pad_tl, up_hw, grid = self._geometry(scene, stride, crop)
        world, rank = torch.distributed.get_world_size(group), torch.distributed.get_rank(group)
        check_same_scene([H, W, len(wins), crop[0], crop[1], stride[0], stride[1], self.num_queries], self.device, group)
        T = len(wins)
        lo, hi = partition(T, world, rank)
        plan = band_plan(wins, H, world)
        yb, need = plan
        if self.upsampler is None:
            tl = self.gather_tile_logits(scene, wins, tile_hw, world, rank, group, grid_of_tiles=grid)
            a, b = need[rank]
            tiles, first = tl[a:b], a
        else:
            mine = list(wins[lo:hi])
            if self.cross_tile_fusion is not None and T > 1:      # strips are exchanged first (two small all-gathers), then JBU on the fused tokens
                local = self._fused_tile_logits(scene, mine if mine else [wins[0]], tile_hw, grid, T, world, rank, group, n_real=hi - lo)
            else:
                local = self.tile_logits(scene, mine if mine else [wins[0]], tile_hw)[:hi - lo]
            tiles, first = exchange_halo_tiles(local, wins, world, rank, group, plan)
        y0, y1 = yb[rank], yb[rank + 1]
        if y1 <= y0:
            return tiles, None, up_hw, pad_tl, (0, W), y0, yb
        w_band = torch.tensor(wins[first:first + tiles.shape[0]], dtype=torch.int32, device=self.device)
        w_band[:, 0:2] -= y0
        return tiles, w_band, up_hw, pad_tl, (y1 - y0, W), y0, yb

    def gather_bands(self, band: torch.Tensor, yb, H: int, group) -> torch.Tensor:
        """[C, rows_r, W] bands of every rank -> the full [C, H, W] on every rank (one all_gather_into_tensor of bands padded to
        the tallest one).  Used for the drop-in's full-canvas return value and for the label map."""
        world = torch.distributed.get_world_size(group)
        hmax = max(yb[r + 1] - yb[r] for r in range(world))
        C_, W = band.shape[0], band.shape[-1]
        block = band.new_zeros((C_, hmax, W))
        block[:, :band.shape[1]] = band
        buf = band.new_empty((world, C_, hmax, W))
        torch.distributed.all_gather_into_tensor(buf.view(world * C_, hmax, W), block, group=group)   # output = concat along dim 0
        if world == 1:
            return buf[0, :, :H]
        return torch.cat([buf[r, :, :yb[r + 1] - yb[r]] for r in range(world)], 1)

    def segment_scene(self, scene: torch.Tensor, stride, crop, group=None, gather_labels: bool = True, want_probs: bool = False,
                      topk: int = 0, ori_shape=None):
        """The whole path for one scene -> labels int64 [1,H,W]; with ``want_probs`` (probs f32 [K,H,W], labels); with ``topk`` > 0
        (classes int32 [topk,H,W], probs f32 [topk,H,W]) instead.  ``ori_shape`` of another size than the scene: labels or the top-k
        planes at that size.  Which kernels run is ``tail_route`` for this one image (DESIGN.md section 5 'Route table').
        Sharded (``group``, or ``tile_group``): every rank computes its tiles, stitches + labels ITS band, and only the int64 label band
        (8 B per pixel instead of 4Q) is gathered; (band labels, first row) when ``gather_labels`` is False.  Labels only: sharding
        refuses probabilities, top-k, another ``ori_shape``, PAMR and area_thd; probabilities at another ``ori_shape`` and top-k
        together with ``want_probs`` or area_thd are refused everywhere."""
        sharded = group is not None or self.tile_group is not None
        self._check_sharding(sharded)
        want, k = self._wanted("segment_scene", want_probs, topk, sharded)
        if self.tta_on():                                       # sharding and top-k were refused above
            return self.tta_image(scene, stride, crop, ori_shape, want_probs)
        resize = ori_shape is not None and tuple(ori_shape) != _scene_hw(scene)
        if resize and want_probs:
            raise ValueError("segment_scene: class probabilities at another ori_shape are not built here; use segment_scenes")
        if resize and sharded:
            raise ValueError("segment_scene: another ori_shape under tile_group sharding is not built (a canvas band does not map to "
                             "whole output rows); use forward_slide + postprocess")
        group = resolve_tile_group(group if group is not None else self.tile_group)
        if want_probs and group is not None:
            raise ValueError("segment_scene: class probabilities under tile_group sharding are not built; use forward_slide + postprocess")
        if group is None:
            H, W, stride, crop, wins, tile_hw, pad_tl, up_hw, grid = self._geometry(scene, stride, crop)
            tl = self.tile_logits(scene, wins, tile_hw, grid_of_tiles=grid)
            win_dev = torch.tensor(wins, dtype=torch.int32, device=self.device)
            out_hw = tuple(int(v) for v in ori_shape) if resize else (H, W)
            return self._image_tail(self.tail_route(want, k, differs=resize).route, want, k, tl, win_dev, up_hw, pad_tl, (H, W), out_hw, scene,
                                    self._ramp(tile_hw))
        tiles, w_band, up_hw, pad_tl, hw, y0, yb = self.sharded_band_tiles(scene, stride, crop, group)
        if hw[0] > 0:
            lab = self.labels_from_tiles(tiles, w_band, up_hw, pad_tl, hw, tile_hw=self._band_tile_hw(scene, stride, crop))
        else:
            lab = torch.empty((1, 0, hw[1]), dtype=torch.int64, device=tiles.device)
        if not gather_labels:
            return lab, y0
        return self.gather_bands(lab, yb, yb[-1], group)

    def tta_image(self, scene: torch.Tensor, stride, crop, ori_shape=None, want_probs: bool = False):
        """Test-time augmentation for one image -> labels int64 [1,H,W], or (mean probs f32 [K,H,W], labels) with ``want_probs``;
        (H, W) = ``ori_shape`` or the image's size.  Every view of ``ops.tta_views`` is made by ``tta_view_scene`` and slid like any
        image (``tile_logits``, so ``tiles_per_launch`` holds).  TTA_HEAD: the views' tile logits are kept and sg_tta_head merges them
        in one launch.  TTA_CANVAS: view by view stitch -> resize to (H, W) -> the probability tail -> sg_tta_accumulate, one view's
        planes and the accumulator alive at a time, then sg_tta_finish.  ``crop`` <= 0 (or None): whole-image inference per view
        (``forward_feature`` at (H, W)), always view by view.  ``min_region`` follows on the final labels."""
        scene = scene.to(self.device)
        H, W = _scene_hw(scene)
        out_hw = (H, W) if ori_shape is None else tuple(int(v) for v in ori_shape)
        whole = crop is None or (isinstance(crop, int) and crop <= 0)
        fused = not whole and self.tail_route("probs" if want_probs else "labels").route == TTA_HEAD
        views, acc = [], None
        post = (self.query_idx, self.num_classes, self.logit_scale)
        listed = ops.tta_views((H, W), self.tta_scales, self.tta_flip)
        for _, flipped, hw in listed:
            view = tta_view_scene(scene, hw, flipped)
            if whole:
                planes = ops.scene_planes(view) if view.dtype == torch.uint8 else view
                canvas = self.forward_feature(planes.float().unsqueeze(0), out_hw)[0]
            else:
                h, w, _, _, wins, tile_hw, pad_tl, up_hw, grid = self._geometry(view, stride, crop)
                tl = self.tile_logits(view, wins, tile_hw, grid_of_tiles=grid)
                win_dev = torch.tensor(wins, dtype=torch.int32, device=self.device)
                if fused:
                    views.append((tl, win_dev, up_hw, pad_tl, (h, w), flipped))
                    continue
                canvas = self._stitched(tile_hw, tl, win_dev, up_hw, pad_tl, (h, w))
                if (h, w) != out_hw:
                    canvas = ops.resize_bilinear(canvas, out_hw)
            probs, _ = ops.postprocess(canvas, *post, 0.0, self.bg_idx, True)
            acc = ops.tta_accumulate(probs, flipped, acc)
        if fused:
            out = ops.tta_head(views, out_hw, *post, self.prob_thd, self.bg_idx, want_probs=want_probs)
        else:
            out = ops.tta_finish(acc, len(listed), self.prob_thd, self.bg_idx, want_probs=want_probs)
        labels = self.sieve(out[0] if want_probs else out)
        return (out[1], labels) if want_probs else labels

    def gather_tile_logits(self, scene, wins, tile_hw, world, rank, group=None, grid_of_tiles=None) -> torch.Tensor:
        """Rank r computes a contiguous block of the raster tile list; one all-gather (RCCL over xGMI on GPUs)
        of equal-sized [T_pad, Q, gh, gw] blocks rebuilds the full list on every rank.  With cross-tile fusion the
        boundary strips are exchanged first (``sharded_cross_tile_fusion``)."""
        T = len(wins)
        lo, hi = partition(T, world, rank)
        mine = list(wins[lo:hi])
        fuse = self.cross_tile_fusion is not None and grid_of_tiles is not None and T > 1
        if fuse:
            local = self._fused_tile_logits(scene, mine if mine else [wins[0]], tile_hw, grid_of_tiles, T, world, rank, group,
                                            n_real=hi - lo)
        else:
            local = self.tile_logits(scene, mine if mine else [wins[0]], tile_hw)   # more ranks than tiles: a dummy so shapes agree
        return gather_blocks(local, T, world, rank, group)

    def _fused_tile_logits(self, scene, mine, tile_hw, grid_of_tiles, T, world, rank, group, n_real):
        """The logits of this rank's tiles ``mine`` (``n_real`` of them; a dummy tile keeps a rank without tiles in the collectives) with
        cross-tile fusion across the ranks: tower, ``sharded_cross_tile_fusion``, head."""
        geo = self._tile_geometry(tile_hw)
        win = torch.tensor(list(mine), dtype=torch.int32, device=self.device).reshape(-1, 4)
        cls, tok = self._tower(scene, win, tile_hw, launch_chunks(win.shape[0], self.tiles_per_launch))
        tok = tok[:n_real].contiguous()
        cls = None if cls is None else cls[:n_real].contiguous()
        steps = ops.CrossTileSteps(*geo.grid, tok.shape[-1], *self._fusion_args(), grid_of_tiles[1])
        tok = sharded_cross_tile_fusion(tok, steps, T, world, rank, group)
        if n_real == 0:
            return tok.new_zeros((0, self.num_queries) + (self.upsampler.output_hw(geo.grid, geo.up_hw) if self.upsampler is not None else geo.grid))
        return self._head_logits(tok, cls, scene, win[:n_real], tile_hw)

    # -- packed slide inference: the windows of many images in shared launches ----------------------------------------
    flush_bytes = 4 << 30       # bound on the tile logits + canvases of one flush group (plan_images)
    pack_fill = None            # value written into a ragged pack buffer's padding (None: left uninitialised -- it is never read)

    def _packed_canvases(self, scenes, stride, crop):
        """Yields (image indices, flat canvas buffer, its [Q,H,W] views) per flush group: ``_packed_tiles`` and one sg_stitch_multi
        launch."""
        for group in self._packed_tiles(scenes, stride, crop, self._canvas_bytes()):
            ramp = self._group_ramp(group)
            canvases, views = ops.stitch_multi(*group[1:]) if ramp is None else ops.stitch_blend_multi(*group[1:], ramp)
            yield group[0], canvases, views

    def _packed_tiles(self, scenes, stride, crop, pixel_bytes):
        """Yields, per flush group, what a multi-image stitch takes: (image indices, tile logits, windows, image of each tile, up_hw,
        pad_tl, [(H, W)] per image, [(first tile, count)] per image) -- the packed tower over the group's chunks, cross-tile fusion per
        image and the head.  ``pixel_bytes``: what the caller will allocate per image pixel, or for image i as a function of i (the
        planner's flush bound counts it)."""
        if self.tile_group is not None:
            raise ValueError("packed inference shards images over ranks, not tiles: with tile_group set use forward_slide / "
                             "segment_scene per image")
        buf, shapes = pack_scenes(scenes, self.device, self.pack_fill)

        def tile_bytes(thw):
            geo = self._tile_geometry(thw)
            oh, ow = self.upsampler.output_hw(geo.grid, geo.up_hw) if self.upsampler is not None else geo.grid
            tok = geo.grid[0] * geo.grid[1] * self.visual.cfg.embed_dim * 4 if self.cross_tile_fusion is not None else 0
            return 4 * self.num_queries * oh * ow + tok

        groups = plan_images(shapes, stride, crop, self.visual.cfg.patch, self.tiles_per_launch, tile_bytes, pixel_bytes, self.flush_bytes)
        for g in groups:
            geo = self._tile_geometry(g.tile_hw)
            for f in g.flush:
                tl = self._packed_tile_logits(buf, g, f)
                imgs = range(f.img_lo, f.img_hi)
                local = [k - f.img_lo for k in imgs for _ in range(g.n_tiles[k])]
                yield ([g.images[k] for k in imgs], tl, g.windows[f.tile_lo:f.tile_hi], local, geo.up_hw, geo.pad_tl,
                       [g.shapes[k] for k in imgs], [(g.first_tile[k] - f.tile_lo, g.n_tiles[k]) for k in imgs])

    def _packed_tile_logits(self, buf, g: TileSizeGroup, f: FlushGroup) -> torch.Tensor:
        win = torch.tensor(g.windows[f.tile_lo:f.tile_hi], dtype=torch.int32, device=self.device).reshape(-1, 4)
        sidx = torch.tensor(g.tile_image[f.tile_lo:f.tile_hi], dtype=torch.int32, device=self.device)
        chunks = [(i - f.tile_lo, j - f.tile_lo) for i, j in f.chunks]
        fused = [k for k in range(f.img_lo, f.img_hi) if g.grids[k][0] * g.grids[k][1] > 1]
        if self.cross_tile_fusion is None or not fused:
            return self._logits_by_chunk(buf, win, g.tile_hw, chunks, sidx)
        # boundary fusion couples the tiles of one image's grid: the packed tower first, then the fusion on each image's contiguous
        # token slice, then the head over the whole flush group
        cls, tok = self._tower(buf, win, g.tile_hw, chunks, sidx)
        gh, gw = self._tile_geometry(g.tile_hw).grid
        for k in fused:
            a, n = g.first_tile[k] - f.tile_lo, g.n_tiles[k]
            tok[a:a + n] = ops.cross_tile_fusion(tok[a:a + n], g.grids[k][0], g.grids[k][1], gh, gw, *self._fusion_args())
        return self._head_logits(tok, cls, buf, win, g.tile_hw, sidx)

    def forward_slide_many(self, scenes, stride, crop, ori_shapes=None) -> List[torch.Tensor]:
        """``forward_slide`` for many images with their windows packed into shared tower launches (``plan_images``).  scenes: a list
        of u8 [H,W,3] / f32 [3,H,W] images of any sizes, or one batch tensor.  Returns logits [1,Q,h,w] per image, (h, w) =
        ori_shapes[i] or the image size.  In f32 these equal ``forward_slide`` per image bit for bit; in the 2-byte modes a different
        launch size may take a different GEMM path, i.e. differ by 2-byte rounding."""
        out: List[Optional[torch.Tensor]] = []
        for idx, _, views in self._packed_canvases(scenes, stride, crop):
            out.extend([None] * (max(idx) + 1 - len(out)))
            for k, c in zip(idx, views):
                ori = None if ori_shapes is None or ori_shapes[k] is None else tuple(ori_shapes[k])
                out[k] = (ops.resize_bilinear(c, ori) if ori is not None and ori != tuple(c.shape[1:]) else c).unsqueeze(0)
        return out

    def label_groups(self, scenes, stride, crop, want_probs: bool = False, ori_shapes=None, topk: int = 0):
        """The whole packed path, flush group by flush group.  Yields (image indices, list of probs f32 [K,H,W] or None, list of labels
        int64 [1,H,W], the flat int64 buffer those label maps are views of, in that order of images); (H, W) = ``ori_shapes[i]`` or the
        image's size.  ``topk`` > 0 (not with ``want_probs``, not with area_thd): yields (image indices, list of probs f32 [topk,H,W],
        list of classes int32 [topk,H,W], None) -- the k best classes of every pixel.
        Which kernels run is decided once for the call by ``tail_route`` and applied per flush group by ``_group_tail``; every route
        returns the same bytes (DESIGN.md section 5 'Route table')."""
        want, k = self._wanted("label_groups", want_probs, topk, self.tile_group is not None)
        if self.tta_on():                                       # image by image through the single-image merge: one group per image
            self._check_sharding(self.tile_group is not None)
            for i, im in enumerate(_images(scenes)):
                out = self.tta_image(im, stride, crop, None if ori_shapes is None else ori_shapes[i], want_probs)
                lab = out[1] if want_probs else out
                yield [i], [out[0] if want_probs else None], [lab], lab.view(-1)
            return
        given = ori_shapes is not None and any(o is not None for o in ori_shapes)
        route = self.tail_route(want, k, given, _ori_differs(ori_shapes, scenes))
        pixel_bytes = route.pixel_bytes
        if route.route == RESIZED_HEAD:
            pixel_bytes = lambda i: route.pixel_bytes * _out_pixels(ori_shapes, i, scenes)
        for group in self._packed_tiles(scenes, stride, crop, pixel_bytes):
            idx = group[0]
            imgs = [_images(scenes)[i] for i in idx] if self.pamr_steps > 0 else [None] * len(idx)
            yield (idx,) + self._group_tail(route.route, want, k, group, _out_sizes(ori_shapes, idx, group[6]), imgs)

    def segment_scenes(self, scenes, stride, crop, want_probs: bool = False, ori_shapes=None, topk: int = 0):
        """``label_groups`` collected per image -> list of labels [1,H,W], or (list of probs [K,H,W], list of labels) with
        ``want_probs``.  With PAMR on every image's canvas is refined before its post-process (``label_groups``).
        ``topk`` > 0: a list of (classes int32 [topk,H,W], probs f32 [topk,H,W]) per image."""
        probs: List[Optional[torch.Tensor]] = []
        labels: List[Optional[torch.Tensor]] = []
        if topk:
            for idx, prb, cls, _ in self.label_groups(scenes, stride, crop, want_probs, ori_shapes, topk=topk):
                probs.extend([None] * (max(idx) + 1 - len(probs)))
                for n, i in enumerate(idx):
                    probs[i] = (cls[n], prb[n])
            return probs
        for idx, prb, lab, _ in self.label_groups(scenes, stride, crop, want_probs, ori_shapes):
            for lst, vals in ((probs, prb), (labels, lab)):
                lst.extend([None] * (max(idx) + 1 - len(lst)))
                for k, x in zip(idx, vals):
                    lst[k] = x
        return (probs, labels) if want_probs else labels

    # -- reference forward_feature (whole image / explicit logit size) ------------------------------------------
    def forward_feature(self, img: torch.Tensor, logit_size=None) -> torch.Tensor:
        """img [B,3,H,W] (H, W already patch multiples or not -- no padding is applied here, as in the
        reference) -> [B,Q,h,w] bilinearly resized to ``logit_size`` (default: the image size)."""
        B, _, H, W = img.shape
        P = self.visual.cfg.patch
        Hc, Wc = (H // P) * P, (W // P) * P           # conv1 (stride P) ignores a ragged remainder
        wins = [(0, Hc, 0, Wc)] * B
        idx = torch.arange(B, dtype=torch.int32, device=self.device)
        tl = self.tile_logits(img, wins, (Hc, Wc), idx)
        size = (H, W) if logit_size is None else tuple(logit_size)
        return torch.stack([ops.resize_bilinear(tl[i], size) for i in range(B)], 0)

    # -- reference postprocess_result --------------------------------------------------------------------------
    def postprocess(self, seg_logits: torch.Tensor, want_probs: bool = True):
        """seg_logits [Q,H,W] -> (probs [K,H,W], labels int64 [1,H,W]).  With ``area_thd`` the first pass runs with ``prob_thd = 0`` and
        always writes the probabilities (a scratch [K,H,W] when they are not wanted), then ``area_filter_first_pass``.  ``min_region``
        is not applied here (the tails call this and sieve their whole group): a caller who post-processes logits itself follows with
        ``sieve(labels)``, as the drop-in classes do."""
        if self.area_thd is not None:
            probs, labels = self.area_filter_first_pass(*ops.postprocess(seg_logits, self.query_idx, self.num_classes, self.logit_scale, 0.0,
                                                                         self.bg_idx, True))
            return (probs if want_probs else None), labels
        return ops.postprocess(seg_logits, self.query_idx, self.num_classes, self.logit_scale, self.prob_thd, self.bg_idx, want_probs)
