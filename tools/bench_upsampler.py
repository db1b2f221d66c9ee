"""Throughput of the upsampler head alone: patch tokens -> per-pixel logits of a batch of 512-pixel tiles (ViT-L/14 geometry: 37 x 37
tokens of 768 channels, guidance 518 x 518, 16 iSAID queries), per upsampler and precision.  Prints Mpix/s of tile area (512^2 per tile)
and ms per tile, timed with device events after a warm-up.

    python tools/bench_upsampler.py [--tiles 8] [--iters 5] [--kinds jbu_one,bilinear,resize_conv] [--precisions f32,f16x2,bf16]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from clip_decontamination_amd import weights as Wt
from clip_decontamination_amd.upsampler import HipJBU


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiles", type=int, default=8)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--kinds", default="jbu_one,bilinear,resize_conv")
    ap.add_argument("--precisions", default="f32,f16x2,bf16")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    C, g, crop, Q = 768, 37, 512, 16
    pad = (g * 14 - crop) // 2                                         # 518 = 512 + 3 + 3
    T = a.tiles
    rng = np.random.default_rng(0)
    tok = torch.from_numpy(rng.standard_normal((T, g * g, C), dtype=np.float32)).to(dev)
    cls = torch.from_numpy(rng.standard_normal((T, C), dtype=np.float32)).to(dev)
    text = torch.from_numpy(Wt.make_text_features(Q, C)).to(dev)
    scene = torch.from_numpy(Wt.make_tiles_u8(1, crop, seed=1, smooth=True)[0]).to(dev)
    windows = torch.tensor([[0, crop, 0, crop]] * T, dtype=torch.int32, device=dev)
    for kind in a.kinds.split(","):
        for prec in a.precisions.split(","):
            up = HipJBU(kind, C, dev, prec)
            if kind == "resize_conv":
                up.load_state_dict(Wt.make_resize_conv_weights(C, seed=3))
            elif kind != "bilinear":
                up.load_state_dict(Wt.make_jbu_weights(kind, C, seed=3))
            run = lambda: up.logits(tok, cls, scene, windows, (crop, crop), (pad, pad), (g, g), text, 0.0, -0.3,
                                    padded_hw=(crop + 2 * pad, crop + 2 * pad))
            out = run()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                run()
            e1.record()
            torch.cuda.synchronize()
            ms = e0.elapsed_time(e1) / a.iters
            print(f"{kind:10s} {prec:6s} ViT-L/14 {T} tiles of {crop}: out {tuple(out.shape[-2:])}  {ms / T:8.3f} ms/tile  "
                  f"{T * crop * crop / (ms * 1e-3) / 1e6:9.1f} Mpix/s", flush=True)
            del up


if __name__ == "__main__":
    main()
