#!/usr/bin/env python3
"""Mints tests/golden/upsampler_alt.npz from the REFERENCE's own upsampler modules (simfeatup_dev/upsamplers.py, imported read-only
through oracle/refimport.py; runs only where the reference tree exists, on the CPU).

For 'bilinear' (get_upsampler('bilinear', C) -> Bilinear, upsamplers.py:343-350): the module is built by the reference factory, receives the
build's (empty) state dict with strict=True exactly as segmentor.py:280-283 loads it, and runs on C = 64 features over non-square patch
grids with guidance at 16 g (patch 16) and at 14 g (patch 14).  The fixture stores the inputs, the outputs and the reference's state-dict
key list (the outputs on a fixed subset of rows and columns, stored with the fixture).  For 'resize_conv' (LayeredResizeConv(C, 1),
upsamplers.py:178-200) the same, on the build's synthetic weights (weights.make_resize_conv_weights, seed 3) loaded with strict=True.

    python tools/mint_upsampler_golden.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import refimport as R          # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "upsampler_alt.npz")
C = 64
GRIDS = [(3, 4), (2, 5)]                   # non-square patch grids
PATCHES = [16, 14]


def sample_idx(n):
    return np.array(sorted(set(range(0, n, 3)) | {n - 2, n - 1}), np.int64)


def main():
    U = R.ref("simfeatup_dev.upsamplers")
    rng = np.random.default_rng(2024)
    out = {}
    up = U.get_upsampler("bilinear", C)
    out["bilinear.keys"] = np.array(sorted(up.state_dict().keys()), dtype="U64")
    up.load_state_dict({}, strict=True)    # what segmentor.py:283 does with the (empty) checkpoint of this module
    for gh, gw in GRIDS:
        src = rng.standard_normal((1, C, gh, gw)).astype(np.float32)
        for P in PATCHES:
            img = rng.standard_normal((1, 3, P * gh, P * gw)).astype(np.float32)
            with torch.no_grad():
                y = up(torch.from_numpy(src), torch.from_numpy(img)).numpy()
            key = f"bilinear.g{gh}x{gw}.p{P}"
            out[key + ".source"] = src
            out[key + ".guidance_shape"] = np.array(img.shape, np.int64)   # Bilinear reads only the guidance's size
            # every third row and column plus the last two of each (the clamped edge): keeps the fixture far below 1 MiB
            rows, cols = sample_idx(y.shape[-2]), sample_idx(y.shape[-1])
            out[key + ".rows"], out[key + ".cols"] = rows, cols
            out[key + ".out"] = y[:, :, rows][:, :, :, cols].astype(np.float32)
    # resize_conv: LayeredResizeConv(C, 1) from the reference factory, the build's synthetic weights loaded with strict=True
    from clip_decontamination_amd import weights as Wt
    rc = U.get_upsampler("resize_conv", C)
    out["resize_conv.keys"] = np.array(sorted(rc.state_dict().keys()), dtype="U64")
    w = Wt.make_resize_conv_weights(C, seed=3)
    rc.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()}, strict=True)
    gh, gw = GRIDS[0]
    src = rng.standard_normal((1, C, gh, gw)).astype(np.float32)
    out["resize_conv.source"] = src
    for P in PATCHES:
        img = rng.standard_normal((1, 3, P * gh, P * gw)).astype(np.float32)
        with torch.no_grad():
            y = rc(torch.from_numpy(src), torch.from_numpy(img)).numpy()
        key = f"resize_conv.g{gh}x{gw}.p{P}"
        out[key + ".guidance"] = img
        rows, cols = sample_idx(y.shape[-2]), sample_idx(y.shape[-1])
        out[key + ".rows"], out[key + ".cols"] = rows, cols
        out[key + ".out"] = y[:, :, rows][:, :, :, cols].astype(np.float32)
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes, {len(out)} arrays)")


if __name__ == "__main__":
    main()
