"""min_region (sg_sieve), measured on resident label maps of the bench scene, 2048 x 4608.  One JSON line per case.

    python tools/bench_sieve.py [--steps 5 --warmup 2 --repeats 20 --out profiles/bench_sieve.jsonl]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_sieve.py --kernels      (the share of time per kernel)

Label maps
  blocky     i.i.d. classes on a 37 x 37 pixel grid (what patch-grid logits leave): K = 16
  speckled   the blocky map with 5 % of the pixels replaced by i.i.d. classes: isolated specks inside large regions
  flat       one class everywhere: one region of 9.4 Mpix, every union and every area add meets the same root
Cases
  sieve      ops.sieve_flat in place on a fresh copy of the map, for both fills, both connectivities, min_region 16 and 256; the copy
             is timed next to it and subtracted (`sieve_ms` = window - copy).  `changed` = the share of pixels the sieve rewrites.
             Reference lines from the same run: `copy_ms` (a device copy of the same int64 buffer) and `class_area_ms` (sg_class_area).
  tail       the labels-only fused tail from resident tile logits (119 tiles of 512 at stride 256, Q = K = 16, as tools/bench_area.py):
             sg_label_head alone against sg_label_head + sg_sieve
  scene      SegPipeline.segment_scene of a synthetic tiny-8 tower on the scene (crop 224, stride 112) with and without min_region
`repeats` windows of `steps` calls, device events around a window; median and (min, max) over the windows.  --kernels runs every
sieve case a few times and measures nothing itself: the kernel statistics of a profiler run over it give the share per kernel.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from clip_decontamination_amd import ops  # noqa: E402
from clip_decontamination_amd.pipeline import tile_windows  # noqa: E402

H, W, CROP, STRIDE, GRID, UP, PAD = 2048, 4608, 512, 256, 37, 518, 3
K, BG = 16, 0


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


def label_maps():
    gen = torch.Generator(device="cuda").manual_seed(3)
    cells = torch.randint(0, K, (H // GRID + 1, W // GRID + 1), device="cuda", generator=gen)
    blocky = cells.repeat_interleave(GRID, 0).repeat_interleave(GRID, 1)[:H, :W].contiguous()
    noise = torch.randint(0, K, (H, W), device="cuda", generator=gen)
    speck = torch.rand(H, W, device="cuda", generator=gen) < 0.05
    return {"blocky": blocky, "speckled": torch.where(speck, noise, blocky).contiguous(), "flat": torch.full((H, W), 4, dtype=torch.int64, device="cuda")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--kernels", action="store_true", help="run every sieve case three times and measure nothing (for a profiler run)")
    ap.add_argument("--no-scene", action="store_true", help="skip the segment_scene case")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_sieve.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sieve needs a GPU: nothing is measured without one")
    mpix = H * W / 1e6
    lines = []

    def emit(**kw):
        kw.update(scene=f"{H}x{W}", steps=a.steps, warmup=a.warmup, repeats=a.repeats, device=torch.cuda.get_device_name(0))
        line = json.dumps(kw)
        print(line, flush=True)
        lines.append(line)

    maps = label_maps()
    settings = [(fill, conn, mr) for fill in ("neighbour", "bg") for conn in (4, 8) for mr in (16, 256)]
    work = torch.empty(H * W, dtype=torch.int64, device="cuda")
    if a.kernels:
        for name, m in maps.items():
            for fill, conn, mr in settings:
                for _ in range(3):
                    ops.sieve_flat(work.copy_(m.view(-1)), [(H, W)], mr, conn, fill, BG)
        torch.cuda.synchronize()
        return

    for name, m in maps.items():
        flat = m.view(-1)
        ref = timed({"copy": lambda: work.copy_(flat), "class_area": lambda: ops.class_area(flat, K)}, a)
        cm = statistics.median(ref["copy"])
        for fill, conn, mr in settings:
            def run():
                ops.sieve_flat(work.copy_(flat), [(H, W)], mr, conn, fill, BG)

            t = timed({"sieve": run, "copy": lambda: work.copy_(flat)}, a)
            sm = statistics.median(t["sieve"]) - statistics.median(t["copy"])
            run()
            emit(case="sieve", map=name, fill=fill, connectivity=conn, min_region=mr, changed=round(float((work != flat).float().mean()), 5),
                 window_ms=spread(t["sieve"]), sieve_ms=round(sm, 4), us_per_mpix=round(1e3 * sm / mpix, 2), copy_ms=spread(ref["copy"]),
                 class_area_ms=spread(ref["class_area"]), ratio_to_copy=round(sm / cm, 2),
                 ratio_to_class_area=round(sm / statistics.median(ref["class_area"]), 2))

    # -- the labels-only fused tail from resident tile logits, with and without the sieve
    wins = tile_windows(H, W, (STRIDE, STRIDE), (CROP, CROP))
    win = torch.tensor(wins, dtype=torch.int32, device="cuda")
    geo = ((UP, UP), (PAD, PAD), (H, W))
    gen = torch.Generator(device="cuda").manual_seed(K)
    tl = 0.3 * torch.randn(len(wins), K, GRID, GRID, device="cuda", generator=gen)
    qi = torch.arange(K, dtype=torch.int32, device="cuda")

    def head():
        return ops.label_head(tl, win, *geo, qi, K, 50.0, 0.3, BG)

    for fill, conn, mr in (("neighbour", 4, 16), ("neighbour", 8, 256), ("bg", 4, 256)):
        def head_sieve():
            lab = ops.label_head(tl, win, *geo, qi, K, 50.0, 0.3, BG)
            return ops.sieve_flat(lab.view(-1), [(H, W)], mr, conn, fill, BG)

        t = timed({"head": head, "seq": head_sieve}, a)
        emit(case="tail", fill=fill, connectivity=conn, min_region=mr, label_head_ms=spread(t["head"]), sequence_ms=spread(t["seq"]),
             ratio=round(statistics.median(t["seq"]) / statistics.median(t["head"]), 3))
    del tl

    # -- segment_scene of a synthetic tiny-8 tower on the whole scene
    if not a.no_scene:
        import warnings
        import segmentor
        with tempfile.TemporaryDirectory() as d:
            path = os.path.join(d, "classes.txt")
            with open(path, "w") as f:
                f.write("\n".join(f"thing{i}" for i in range(8)) + "\n")
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                seg = segmentor.SegmentorEx(clip_type="CLIP", vit_type="tiny-8", model_type="SegEarth", name_path=path, device=torch.device("cuda"),
                                            precision="f32", synthetic_ok=True, prob_thd=0.05, bg_idx=BG, apply_sim_feat_up=False, slide_crop=224,
                                            slide_stride=112)
        scene = torch.randn(3, H, W, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
        b = argparse.Namespace(steps=1, warmup=1, repeats=max(3, a.repeats // 4))

        def scene_with(mr):
            seg.min_region = mr                                               # the pipeline is rebuilt per call
            return seg._pipeline().segment_scene(scene, 112, 224)

        t = timed({"plain": lambda: scene_with(None), "sieved": lambda: scene_with(64)}, b)
        changed = float((scene_with(None) != scene_with(64)).float().mean())
        emit(case="scene", tower="tiny-8 synthetic f32, crop 224, stride 112", min_region=64, fill="neighbour", connectivity=4, changed=round(changed, 5),
             plain_ms=spread(t["plain"]), sieved_ms=spread(t["sieved"]),
             added_ms=round(statistics.median(t["sieved"]) - statistics.median(t["plain"]), 3))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
