"""Packed multi-image inference against the per-image loop, same process, synthetic weights: one JSON line per case.

    python tools/bench_batch.py --steps 3 --warmup 1 [--cases a_bf16,a_f16x2,b]

Cases
  a_bf16 / a_f16x2  119 images of 512^2, ViT-L/14, crop = stride = 512 (one window per image): the per-image loop makes 119 one-tile
                    tower launches, the packed path one launch of 119 tiles (bench.py builds that slab itself)
  b                 the shipped default config: ViT-B/16 + jbu_one, 512^2 images, crop 224 / stride 112 (16 windows per image), f16x2
Both paths run the whole way to labels: SegPipeline.segment_scene per image vs SegPipeline.segment_scenes on the batch (u8 NHWC
input on the device; time from the first launch to a device synchronise).  The packed labels are checked against the loop's.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from clip_decontamination_amd import weights as Wt  # noqa: E402
from clip_decontamination_amd.engine import HipCLIP, HipVisionTower  # noqa: E402
from clip_decontamination_amd.pipeline import SegPipeline  # noqa: E402

QIDX = [0, 0, 1, 2, 3, 4, 5, 5]                     # Potsdam: 8 queries, 6 classes
CASES = {
    "a_bf16": dict(vit="ViT-L/14", precision="bf16", images=119, crop=512, stride=512, jbu=False, tiles_per_launch=119),
    "a_f16x2": dict(vit="ViT-L/14", precision="f16x2", images=119, crop=512, stride=512, jbu=False, tiles_per_launch=119),
    "b": dict(vit="ViT-B/16", precision="f16x2", images=32, crop=224, stride=112, jbu=True, tiles_per_launch=128),
}


def build(c):
    dev = torch.device("cuda:0")
    cfg = Wt.vit_config(c["vit"])
    tower = HipVisionTower(cfg, Wt.make_vit_weights(cfg, seed=0), precision=c["precision"], device=dev)
    up = None
    if c["jbu"]:
        from clip_decontamination_amd.upsampler import HipJBU
        up = HipJBU("jbu_one", cfg.embed_dim, dev, c["precision"])
        up.load_state_dict(Wt.make_jbu_weights("jbu_one", cfg.embed_dim, seed=3))
    text = torch.from_numpy(Wt.make_text_features(len(QIDX), cfg.embed_dim))
    return SegPipeline(HipCLIP(tower), text, torch.tensor(QIDX), model_type="Experimental" if not c["jbu"] else "SegEarth",
                       global_debias_factor=0.2, prob_thd=0.1, bg_idx=5, upsampler=up, tiles_per_launch=c["tiles_per_launch"])


def timed(fn, steps, warmup):
    for _ in range(warmup):
        out = fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--images", type=int, default=0, help="override the image count of every case")
    a = ap.parse_args()
    if a.steps < 1 or a.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    if not torch.cuda.is_available():
        sys.exit("bench_batch.py measures on the GPU; none is visible")
    for name in a.cases.split(","):
        c = dict(CASES[name])
        if a.images:
            c["images"] = a.images
        pipe = build(c)
        n, S = c["images"], 512
        batch = torch.from_numpy(Wt.make_tiles_u8(n, S, seed=7, smooth=True)).cuda()      # [n,512,512,3] u8
        t_loop, lab_loop = timed(lambda: [pipe.segment_scene(batch[i], c["stride"], c["crop"]) for i in range(n)], a.steps, a.warmup)
        t_pack, lab_pack = timed(lambda: pipe.segment_scenes(batch, c["stride"], c["crop"]), a.steps, a.warmup)
        agree = sum(int((x == y).sum()) for x, y in zip(lab_loop, lab_pack)) / (n * S * S)
        mpix = n * S * S / 1e6
        print(json.dumps(dict(case=name, vit=c["vit"], precision=c["precision"], upsampler="jbu_one" if c["jbu"] else None, images=n,
                              image_hw=[S, S], crop=c["crop"], stride=c["stride"], tiles_per_launch=c["tiles_per_launch"],
                              loop_images_per_s=round(n / t_loop, 2), loop_mpix_per_s=round(mpix / t_loop, 2),
                              packed_images_per_s=round(n / t_pack, 2), packed_mpix_per_s=round(mpix / t_pack, 2),
                              speedup=round(t_loop / t_pack, 3), label_agreement=round(agree, 6), steps=a.steps, warmup=a.warmup,
                              device=torch.cuda.get_device_name(0))), flush=True)
        del pipe, batch
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
