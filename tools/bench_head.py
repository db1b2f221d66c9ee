"""The labels-only tail, measured from resident tile logits at the bench geometry: 119 tiles of 512 at stride 256 on a 2048 x 4608 band,
ViT-L/14 grids of 37 x 37 (tiles padded to 518).  One JSON line per case.

    python tools/bench_head.py --steps 10 --warmup 2 --repeats 5 [--out profiles/rNN_bench_head.jsonl]

Routes
  canvas  sg_stitch + sg_postprocess (labels only): writes the f32 [Q,H,W] canvas and reads it back.  Q = 8, 16, 64.
  fused   sg_label_head: no canvas.  The same Q, plus 130 and 256.
For a Q both routes take they are timed in the same rounds, alternating (canvas, fused, canvas, ...), `repeats` windows of `steps` calls
each, device events around a window; median and (min, max) over the windows.  `peak_extra_mb`: the peak of device memory allocated
during one call beyond what was resident before it (tile logits, windows, query indices), i.e. canvas + labels or labels alone.
Tile logits are i.i.d. N(0, 0.3^2); the labels of the two routes are compared off ties once per Q (`label_mismatch`).
"""
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

H, W, CROP, STRIDE, GRID, UP, PAD = 2048, 4608, 512, 256, 37, 518, 3
SCALE, THD, BG = 50.0, 0.0, 0


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
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--queries", default="8,16,64,130,256")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_head needs a GPU: nothing is measured without one")
    wins = tile_windows(H, W, (STRIDE, STRIDE), (CROP, CROP))
    win = torch.tensor(wins, dtype=torch.int32, device="cuda")
    lines = []

    def emit(**kw):
        kw.update(geometry=f"{len(wins)} tiles of {CROP} at stride {STRIDE} on {H}x{W}, grids {GRID}x{GRID}", steps=a.steps, warmup=a.warmup,
                  repeats=a.repeats, device=torch.cuda.get_device_name(0))
        line = json.dumps(kw)
        print(line, flush=True)
        lines.append(line)

    for Q in [int(q) for q in a.queries.split(",")]:
        gen = torch.Generator(device="cuda").manual_seed(Q)
        tl = 0.3 * torch.randn(len(wins), Q, GRID, GRID, device="cuda", generator=gen)
        qi = torch.arange(Q, dtype=torch.int32, device="cuda")

        def canvas():
            c = ops.stitch(tl, win, (UP, UP), (PAD, PAD), (H, W))
            return ops.postprocess(c, qi, Q, SCALE, THD, BG, want_probs=False)[1]

        def fused():
            return ops.label_head(tl, win, (UP, UP), (PAD, PAD), (H, W), qi, Q, SCALE, THD, BG)

        routes = {"fused": fused}
        if Q <= ops.POSTPROCESS_MAX_Q:
            routes = {"canvas": canvas, "fused": fused}
        times = {k: [] for k in routes}
        for k, fn in routes.items():
            for _ in range(a.warmup):
                fn()
        for _ in range(a.repeats):
            for k, fn in routes.items():                                   # alternating within a round
                times[k].append(window_ms(fn, a.steps))
        mism = None
        if "canvas" in routes:
            lc, (lf, cf) = canvas(), ops.label_head(tl, win, (UP, UP), (PAD, PAD), (H, W), qi, Q, SCALE, THD, BG, want_conf=True)
            mism = int((lc[0] != lf[0]).sum())                                # ties included: an upper bound on disagreements off ties
            del lc, lf, cf
        for k, fn in routes.items():
            emit(case=k, Q=Q, ms=spread(times[k]), mpix_per_s=round(H * W / 1e3 / statistics.median(times[k]), 1),
                 peak_extra_mb=peak_extra_mb(fn), tile_logits_mb=round(tl.numel() * 4 / 1e6, 1), label_mismatch_pixels=mism)
        del tl
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
