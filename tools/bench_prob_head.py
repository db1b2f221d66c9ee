"""The tail that returns class probabilities and labels, measured from resident tile logits at the bench geometry: 119 tiles of 512 at
stride 256 on a 2048 x 4608 band, ViT-L/14 grids of 37 x 37 (tiles padded to 518).  One JSON line per case.

    python tools/bench_prob_head.py --steps 3 --warmup 3 --repeats 20 [--out profiles/rNN_bench_prob_head.jsonl]

Routes, Q = K in {16, 64, 130, 256}
  canvas  ops.stitch + ops.postprocess with probabilities: writes the f32 [Q,H,W] canvas and reads it back (three times beyond 64
          queries, sg_postprocess_wide).
  fused   ops.prob_head (sg_prob_head): no canvas.
Both are timed in the same process in alternating rounds (canvas, fused, canvas, ...): `repeats` windows of `steps` calls each, device
events around a window; median and (min, max) over the windows.  `peak_extra_mb`: the peak of device memory allocated during one call
beyond what was resident before it (tile logits, windows, query indices), i.e. canvas + probs + labels or probs + labels.
Tile logits are i.i.d. N(0, 0.3^2).  `equal`: whether the two routes returned the same bytes (they must).  The last line applies the
rule behind prob_head="auto": the fused head beyond 64 queries only if its median is not above the canvas route's at both 130 and 256.
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


def auto_rule(medians):
    """medians: {Q: {"canvas": ms, "fused": ms}} -> whether prob_head="auto" takes the fused head beyond 64 queries."""
    return all(q in medians and medians[q]["fused"] <= medians[q]["canvas"] for q in (130, 256))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--queries", default="16,64,130,256")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_prob_head needs a GPU: nothing is measured without one")
    wins = tile_windows(H, W, (STRIDE, STRIDE), (CROP, CROP))
    win = torch.tensor(wins, dtype=torch.int32, device="cuda")
    lines, medians = [], {}

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
            return ops.postprocess(c, qi, Q, SCALE, THD, BG, want_probs=True)

        def fused():
            return ops.prob_head(tl, win, (UP, UP), (PAD, PAD), (H, W), qi, Q, SCALE, THD, BG)

        routes = {"canvas": canvas, "fused": fused}
        times = {k: [] for k in routes}
        for fn in routes.values():
            for _ in range(a.warmup):
                fn()
        for _ in range(a.repeats):
            for k, fn in routes.items():                                   # alternating within a round
                times[k].append(window_ms(fn, a.steps))
        (pc, lc), (pf, lf) = canvas(), fused()
        equal = bool(torch.equal(pc, pf)) and bool(torch.equal(lc, lf))
        del pc, lc, pf, lf
        medians[Q] = {k: statistics.median(times[k]) for k in routes}
        for k, fn in routes.items():
            emit(case=k, Q=Q, K=Q, ms=spread(times[k]), mpix_per_s=round(H * W / 1e3 / statistics.median(times[k]), 1),
                 peak_extra_mb=peak_extra_mb(fn), tile_logits_mb=round(tl.numel() * 4 / 1e6, 1), equal=equal)
        del tl
    if all(q in medians for q in (130, 256)):
        emit(case="auto_rule", fused_beyond_64=auto_rule(medians),
             medians_ms={str(q): {k: round(v, 4) for k, v in medians[q].items()} for q in (130, 256)})
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
