"""The k best classes per pixel with their probabilities, measured from resident tile logits at the bench geometry: 119 tiles of 512 at
stride 256 on a 2048 x 4608 band, ViT-L/14 grids of 37 x 37 (tiles padded to 518).  One JSON line per case.

    python tools/bench_topk_head.py --steps 2 --warmup 2 --repeats 20 [--out profiles/rNN_bench_topk_head.jsonl]

Routes, Q = K in {16, 64, 130, 256}, k in {1, 5, 8}
  topk    (a) ops.topk_head (sg_topk_head): no canvas, no [K,H,W] planes; writes 8k bytes per pixel.
  canvas  (b) ops.stitch + ops.postprocess with probabilities (sg_postprocess_wide beyond 64 queries) + ops.topk_from_probs (a stable
          torch sort over the K planes): what a caller had to do before.
  label   (c) ops.label_head with want_conf: one label and its probability, the floor for k = 1.  Does not depend on k: one line per Q.
  prob    (d) ops.prob_head: all K probabilities without the canvas.  Does not depend on k: one line per Q.
All routes of one (Q, k) are timed in the same process in alternating rounds: `repeats` windows of `steps` calls each, device events
around a window; median and (min, max) over the windows.  `peak_extra_mb`: the peak of device memory allocated during one call beyond
what was resident before it (tile logits, windows, query indices).  `agree` (on the topk and canvas lines): the share of (pixel, slot)
pairs on which (a) and (b) name the same class.  Tile logits are i.i.d. N(0, 0.3^2).
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


def alternate(routes, steps, warmup, repeats):
    times = {name: [] for name in routes}
    for fn in routes.values():
        for _ in range(warmup):
            fn()
    for _ in range(repeats):
        for name, fn in routes.items():                                    # alternating within a round
            times[name].append(window_ms(fn, steps))
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--queries", default="16,64,130,256")
    ap.add_argument("--ks", default="1,5,8")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_topk_head needs a GPU: nothing is measured without one")
    wins = tile_windows(H, W, (STRIDE, STRIDE), (CROP, CROP))
    win = torch.tensor(wins, dtype=torch.int32, device="cuda")
    lines = []

    def emit(**kw):
        kw.update(geometry=f"{len(wins)} tiles of {CROP} at stride {STRIDE} on {H}x{W}, grids {GRID}x{GRID}", steps=a.steps, warmup=a.warmup,
                  repeats=a.repeats, device=torch.cuda.get_device_name(0))
        line = json.dumps(kw)
        print(line, flush=True)
        lines.append(line)
        if a.out:                                                          # rewritten after every line: a cut-off run keeps what it measured
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    for Q in [int(q) for q in a.queries.split(",")]:
        gen = torch.Generator(device="cuda").manual_seed(Q)
        tl = 0.3 * torch.randn(len(wins), Q, GRID, GRID, device="cuda", generator=gen)
        qi = torch.arange(Q, dtype=torch.int32, device="cuda")
        mb = round(tl.numel() * 4 / 1e6, 1)

        def label():
            return ops.label_head(tl, win, (UP, UP), (PAD, PAD), (H, W), qi, Q, SCALE, THD, BG, want_conf=True)

        def prob():
            return ops.prob_head(tl, win, (UP, UP), (PAD, PAD), (H, W), qi, Q, SCALE, THD, BG)

        for k in [int(x) for x in a.ks.split(",") if int(x) <= Q]:
            def topk():
                return ops.topk_head(tl, win, (UP, UP), (PAD, PAD), (H, W), qi, Q, SCALE, k)

            def canvas():
                c = ops.stitch(tl, win, (UP, UP), (PAD, PAD), (H, W))
                p, _ = ops.postprocess(c, qi, Q, SCALE, THD, BG, want_probs=True)
                del c
                return ops.topk_from_probs(p, qi, k)

            routes = {"topk": topk, "canvas": canvas, "label": label}
            times = alternate(routes, a.steps, a.warmup, a.repeats)
            (ca, _), (cb, _) = topk(), canvas()
            agree = round(float((ca == cb).float().mean()), 6)
            del ca, cb
            for name in ("topk", "canvas"):
                emit(case=name, Q=Q, K=Q, k=k, ms=spread(times[name]), mpix_per_s=round(H * W / 1e3 / statistics.median(times[name]), 1),
                     peak_extra_mb=peak_extra_mb(routes[name]), tile_logits_mb=mb, agree=agree,
                     label_ms_same_rounds=round(statistics.median(times["label"]), 4))
        times = alternate({"label": label, "prob": prob}, a.steps, a.warmup, a.repeats)
        for name, fn in (("label", label), ("prob", prob)):
            emit(case=name, Q=Q, K=Q, k=None, ms=spread(times[name]), mpix_per_s=round(H * W / 1e3 / statistics.median(times[name]), 1),
                 peak_extra_mb=peak_extra_mb(fn), tile_logits_mb=mb)
        del tl


if __name__ == "__main__":
    main()
