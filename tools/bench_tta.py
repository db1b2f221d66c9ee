"""Test-time augmentation: the fused merge head against the canvas route, from resident tile logits.  One JSON line per case.

    python tools/bench_tta.py [--queries 16,64] [--out profiles/bench_tta.jsonl]

Shape: one scene of 2048 x 4608, views at scales (0.75, 1.0, 1.25), with and without the flip (3 or 6 views), each view's windows of
512 at stride 256 on its own size (65, 119 and 198 tiles; grids 37 x 37, tiles padded to 518), merged at 2048 x 4608.  Q = K.
Routes, labels only and with the mean probability planes
  fused   ops.tta_head: sg_tta_head on the views' tile logits, one launch (the copy of the views' logits into one buffer is inside)
  canvas  per view ops.stitch -> ops.resize_bilinear -> ops.postprocess (probabilities) -> ops.tta_accumulate, then ops.tta_finish:
          what SegPipeline does with tta_head="canvas"
Both routes of one case are timed in the same process in alternating rounds: `repeats` windows of `steps` calls each, device events
around a window; median and (min, max) over the windows.  `peak_extra_mb`: the peak of device memory allocated during one call beyond
what was resident before it (the tile logits).  `agree`: the share of pixels on which the route names the fused route's class.
Tile logits are i.i.d. N(0, 0.3^2).  The towers are not part of it: they cost the same on either route."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from clip_decontamination_amd import ops  # noqa: E402
from clip_decontamination_amd.pipeline import tile_windows  # noqa: E402

SCALE, THD, BG = 50.0, 0.0, 0
HW, CROP, STRIDE, GRID, UP, PAD = (2048, 4608), 512, 256, 37, 518, 3
SCALES = (0.75, 1.0, 1.25)


def spread(xs):
    return dict(median=round(statistics.median(xs), 4), min=round(min(xs), 4), max=round(max(xs), 4))


def window_ms(fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / steps


def peak_extra_mb(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    del out
    return round((peak - base) / 1e6, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=1)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--queries", default="16,64")
    ap.add_argument("--out", default=None, help="appended to, one line per case")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_tta needs a GPU: nothing is measured without one")

    def emit(**kw):
        kw.update(steps=a.steps, warmup=a.warmup, repeats=a.repeats, device=torch.cuda.get_device_name(0))
        line = json.dumps(kw)
        print(line, flush=True)
        if a.out:                                                          # appended line by line: a cut-off run keeps what it measured
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")

    for Q in [int(q) for q in a.queries.split(",")]:
        qi = torch.arange(Q, dtype=torch.int32, device="cuda")
        gen = torch.Generator(device="cuda").manual_seed(Q)
        per_scale = {}
        for s, _, hw in ops.tta_views(HW, SCALES, False):
            wins = tile_windows(hw[0], hw[1], (STRIDE, STRIDE), (CROP, CROP))
            per_scale[s] = (0.3 * torch.randn(len(wins), Q, GRID, GRID, device="cuda", generator=gen),
                            torch.tensor(wins, dtype=torch.int32, device="cuda"), hw)
        for flip in (False, True):
            views = [(per_scale[s][0], per_scale[s][1], (UP, UP), (PAD, PAD), hw, f) for s, f, hw in ops.tta_views(HW, SCALES, flip)]
            tiles = [int(v[0].shape[0]) for v in views]
            geometry = (f"{len(views)} views of {HW[0]}x{HW[1]} at scales {SCALES}{' x flip' if flip else ''}, {tiles} tiles of {CROP} at "
                        f"stride {STRIDE}, grids {GRID}x{GRID}, merged at {HW[0]}x{HW[1]}")
            for want_probs in (False, True):
                def fused():
                    return ops.tta_head(views, HW, qi, Q, SCALE, THD, BG, want_probs=want_probs)

                def canvas():
                    acc = None
                    for tl, win, up, pad, hw, f in views:
                        c = ops.stitch(tl, win, up, pad, hw)
                        if tuple(hw) != HW:
                            c = ops.resize_bilinear(c, HW)
                        acc = ops.tta_accumulate(ops.postprocess(c, qi, Q, SCALE, 0.0, BG, True)[0], f, acc)
                        del c
                    return ops.tta_finish(acc, len(views), THD, BG, want_probs=want_probs)

                routes = {"fused": fused, "canvas": canvas}
                times = {name: [] for name in routes}
                for fn in routes.values():
                    for _ in range(a.warmup):
                        fn()
                for _ in range(a.repeats):
                    for name, fn in routes.items():                        # alternating within a round
                        times[name].append(window_ms(fn, a.steps))
                first = lambda out: (out[0] if isinstance(out, tuple) else out).reshape(-1)   # noqa: E731
                ref = first(fused())
                for name, fn in routes.items():
                    got = first(fn())
                    emit(case=name, Q=Q, K=Q, views=len(views), flip=flip, outputs="labels+probs" if want_probs else "labels", geometry=geometry,
                         ms=spread(times[name]), mpix_per_s=round(HW[0] * HW[1] / 1e3 / statistics.median(times[name]), 1),
                         peak_extra_mb=peak_extra_mb(fn), tile_logits_mb=round(sum(per_scale[s][0].numel() for s in per_scale) * 4 / 1e6, 1),
                         agree=round(float((got == ref).float().mean()), 6))
                    del got
                del ref
        del per_scale


if __name__ == "__main__":
    main()
