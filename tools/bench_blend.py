"""Weighted window blending, measured from resident tile logits at the bench geometry of tools/bench_head.py: 119 tiles of 512 at stride
256 on a 2048 x 4608 band, ViT-L/14 grids of 37 x 37 (tiles padded to 518), Q = K = 16 and 64.  One JSON line per case.

    python tools/bench_blend.py [--steps 5 --warmup 2 --repeats 20 --out profiles/bench_blend.jsonl]

Cases (the blended kernel next to the unweighted one of the same run; rounds alternate between the two)
  stitch       sg_stitch against sg_stitch_blend
  label_head   sg_label_head against sg_label_head_blend
each with "hann" over the full window (R = 256, a table of 257 entries) and `ratio` = blended median / unweighted median; `spread` is
the unweighted kernel's (max - min) / median over its windows of this run, the yardstick a ratio has to beat to mean anything.
`repeats` windows of `steps` calls, device events around a window; median and (min, max) over the windows.  Tile logits are i.i.d.
N(0, 0.3^2).
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
SCALE, THD, BG = 50.0, 0.3, 0


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


def timed(routes, a):
    """{name: fn} -> {name: [ms per window]}, the routes alternating within a round."""
    times = {k: [] for k in routes}
    for fn in routes.values():
        for _ in range(a.warmup):
            fn()
    for _ in range(a.repeats):
        for k, fn in routes.items():
            times[k].append(window_ms(fn, a.steps))
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--queries", default="16,64")
    ap.add_argument("--kind", default="hann", choices=("linear", "hann"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_blend.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_blend needs a GPU: nothing is measured without one")
    wins = tile_windows(H, W, (STRIDE, STRIDE), (CROP, CROP))
    win = torch.tensor(wins, dtype=torch.int32, device="cuda")
    geo = ((UP, UP), (PAD, PAD), (H, W))
    R = CROP // 2
    ramp = ops.blend_table(a.kind, R, "cuda")
    lines = []

    def emit(**kw):
        kw.update(geometry=f"{len(wins)} tiles of {CROP} at stride {STRIDE} on {H}x{W}, grids {GRID}x{GRID}", blend=a.kind, R=R, steps=a.steps,
                  warmup=a.warmup, repeats=a.repeats, device=torch.cuda.get_device_name(0))
        line = json.dumps(kw)
        print(line, flush=True)
        lines.append(line)

    for Q in [int(q) for q in a.queries.split(",")]:
        gen = torch.Generator(device="cuda").manual_seed(Q)
        tl = 0.3 * torch.randn(len(wins), Q, GRID, GRID, device="cuda", generator=gen)
        qi = torch.arange(Q, dtype=torch.int32, device="cuda")
        cases = {
            "stitch": {"plain": lambda: ops.stitch(tl, win, *geo), "blend": lambda: ops.stitch_blend(tl, win, *geo, ramp)},
            "label_head": {"plain": lambda: ops.label_head(tl, win, *geo, qi, Q, SCALE, THD, BG),
                           "blend": lambda: ops.label_head_blend(tl, win, *geo, qi, Q, SCALE, THD, BG, ramp)},
        }
        for case, routes in cases.items():
            t = timed(routes, a)
            pm, bm = statistics.median(t["plain"]), statistics.median(t["blend"])
            emit(case=case, Q=Q, plain_ms=spread(t["plain"]), blend_ms=spread(t["blend"]), ratio=round(bm / pm, 3),
                 spread=round((max(t["plain"]) - min(t["plain"])) / pm, 3))
        del tl
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
