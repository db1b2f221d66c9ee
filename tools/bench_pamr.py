"""PAMR (sg_pamr_affinity / sg_pamr_step), measured at the bench geometry, and segment_scene with and without it.  One JSON line per case.

    python tools/bench_pamr.py --steps 10 --warmup 2 --repeats 5 [--cases kernel,path] [--out profiles/rNN_bench_pamr.jsonl]

Cases
  copy    a 1 GiB device-to-device copy, bytes read plus bytes written over time: the yardstick of the same run (tools/bench_metric.py)
  kernel  2048 x 4608, Q = 16 and 64, dilations (8, 16) and (1, 2, 4, 8, 12, 24): device-event time of the affinity pass and of one step
          (`repeats` windows of `steps` launches each, ping-pong between two canvases; median and spread), and the achieved fraction of
          the step's algorithmic bytes (2Q + 8D) * 4 * H * W at the copy rate of this run.  Guidance: a smooth synthetic u8 scene,
          normalised; logits 0.2 + 0.1 randn.
  path    SegPipeline.segment_scene on a resident 2048 x 4608 u8 scene, 119 tiles of 512 at stride 256 in one launch (ViT-L/14, bf16,
          synthetic weights, 16 queries), with pamr_steps = 0 and 10 over (8, 16): host clock to a device synchronise, the two routes
          alternating within a round.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from clip_decontamination_amd import ops, weights as Wt  # noqa: E402

H, W = 2048, 4608
DILATIONS = {"8,16": (8, 16), "1,2,4,8,12,24": (1, 2, 4, 8, 12, 24)}


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


def scene_u8():
    """[2048, 4608, 3] u8 on the device: the smooth synthetic tiles of the bench, repeated."""
    t = torch.from_numpy(Wt.make_tiles_u8(1, 1024, seed=1234, smooth=True)[0]).cuda()
    return t[torch.arange(H, device="cuda") % 1024][:, torch.arange(W, device="cuda") % 1024].contiguous()


def copy_rate(a, emit):
    src = torch.empty(1 << 28, dtype=torch.float32, device="cuda").normal_()
    dst = torch.empty_like(src)
    for _ in range(a.warmup):
        dst.copy_(src)
    rates = [2 * src.numel() * 4 / (window_ms(lambda: dst.copy_(src), a.steps) * 1e-3) / 1e12 for _ in range(a.repeats)]
    emit(case="copy", bytes_each_way=src.numel() * 4, tb_per_s=spread(rates))
    return statistics.median(rates) * 1e12


def kernel_cases(a, emit):
    hbm = copy_rate(a, emit)
    guide = ops.scene_planes(scene_u8())
    for name, dil in DILATIONS.items():
        D = len(dil)
        for _ in range(a.warmup):
            w = ops.pamr_weights(guide, dil)
        aff = [window_ms(lambda: ops.pamr_weights(guide, dil), a.steps) for _ in range(a.repeats)]
        arr = ops.pamr_dilations(dil)[1]
        lib = ops._lib.load()
        for Q in (16, 64):
            gen = torch.Generator(device="cuda").manual_seed(Q)
            bufs = [0.2 + 0.1 * torch.randn(Q, H, W, device="cuda", generator=gen), torch.empty(Q, H, W, device="cuda")]
            turn = [0]

            def step():                                             # the raw entry: no allocation inside the timed window
                i = turn[0]
                ops.check(lib.sg_pamr_step(ops.ptr(w), ops.ptr(bufs[i]), ops.ptr(bufs[1 - i]), Q, H, W, arr, D, ops.stream_ptr()), "sg_pamr_step")
                turn[0] = 1 - i

            for _ in range(2 * a.warmup):
                step()
            ms = [window_ms(step, a.steps) for _ in range(a.repeats)]
            nbytes = (2 * Q + 8 * D) * 4 * H * W
            med = statistics.median(ms)
            emit(case="kernel", hw=[H, W], Q=Q, dilations=name, affinity_ms=spread(aff), step_ms=spread(ms), pamr_steps=10,
                 ten_steps_plus_affinity_ms=round(10 * med + statistics.median(aff), 3), step_algorithmic_mb=round(nbytes / 1e6, 1),
                 step_tb_per_s=round(nbytes / (med * 1e-3) / 1e12, 3), fraction_of_copy_rate=round(nbytes / (med * 1e-3) / hbm, 3),
                 floor_ms_at_copy_rate=round(nbytes / hbm * 1e3, 4))
            del bufs
        del w


def path_case(a, emit):
    from clip_decontamination_amd.engine import HipCLIP, HipVisionTower
    from clip_decontamination_amd.pipeline import SegPipeline
    cfg = Wt.vit_config("ViT-L-14")
    net = HipCLIP(HipVisionTower(cfg, Wt.make_vit_weights(cfg, seed=0), precision="bf16", device="cuda:0"))
    Q = 16
    text = torch.from_numpy(Wt.make_text_features(Q, cfg.embed_dim))
    kw = dict(model_type="SegEarth", global_debias_factor=0.0, prob_thd=0.0, bg_idx=0, tiles_per_launch=119)
    routes = {"plain": SegPipeline(net, text, torch.arange(Q), **kw),
              "pamr": SegPipeline(net, text, torch.arange(Q), pamr_steps=10, pamr_stride=(8, 16), **kw)}
    scene = scene_u8()
    times = {k: [] for k in routes}
    for k, p in routes.items():
        for _ in range(a.warmup):
            p.segment_scene(scene, 256, 512)
    labels = {}
    for _ in range(a.repeats):
        for k, p in routes.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            labels[k] = p.segment_scene(scene, 256, 512)
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) * 1e3)
    med = {k: statistics.median(v) for k, v in times.items()}
    emit(case="path", vit="ViT-L/14", precision="bf16", hw=[H, W], tiles=119, Q=Q, dilations="8,16", pamr_steps=10,
         ms={k: spread(v) for k, v in times.items()}, mpix_per_s={k: round(H * W / 1e3 / med[k], 1) for k in med},
         pamr_minus_plain_ms=round(med["pamr"] - med["plain"], 3), labels_changed_share=round(float((labels["pamr"] != labels["plain"]).float().mean()), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10, help="launches per timed window (kernel case)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--cases", default="kernel,path")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.steps < 1 or a.warmup < 0 or a.repeats < 1:
        ap.error("--steps and --repeats must be >= 1 and --warmup >= 0")
    if not torch.cuda.is_available():
        raise SystemExit("bench_pamr measures on the GPU; none is visible")
    lines = []

    def emit(**kw):
        kw.update(steps=a.steps, warmup=a.warmup, repeats=a.repeats, device=torch.cuda.get_device_name(0))
        lines.append(json.dumps(kw))
        print(lines[-1], flush=True)

    for name in a.cases.split(","):
        {"kernel": kernel_cases, "path": path_case}[name](a, emit)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
