"""The upsampler head beyond 32 queries: HipJBU.logits of jbu_one, C = 768, bf16, on tools/bench_upsampler.py's shape (8 tiles of 512 pixels,
ViT-L/14 geometry: 37 x 37 tokens, guidance 518 x 518), per query count with the fused tail (sg_jbu_logits_wide) and with
fused_tail=False (sg_jbu_upsample + cosine logits: what more than 32 queries ran before the wide tail); Q = 32 is the narrow kernel and
gives the same-run baseline.  Then the bilinear kind at Q = 130 in one call and as the former host loop over 32-query chunks (a
temporary and a strided copy per chunk).  Device events after a warm-up, as tools/bench_upsampler.py; one JSON line per case.

    python tools/bench_jbu_wide.py [--tiles 8] [--iters 5] [--queries 32,48,64,130,256] [--out profiles/r08_bench_jbu_wide.jsonl]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from clip_decontamination_amd import weights as Wt
from clip_decontamination_amd._lib import check
from clip_decontamination_amd.ops import ptr, stream_ptr
from clip_decontamination_amd.upsampler import HipJBU


def timed(run, iters):
    """(ms per call, peak allocated bytes of one call on top of what is live before it, the last result's shape)"""
    out = run()                                                           # warm-up: workspace, dynamic-LDS opt-ins
    shape = tuple(out.shape)
    del out
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    live = torch.cuda.memory_allocated()
    run()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - live
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        run()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters, peak, shape


def bilinear_chunk_loop(up, tok, cls, guid, gh, gw, text, lam):
    """The host loop HipJBU.logits ran for the bilinear kind beyond 32 queries before sg_jbu_logits_wide, restated on one launch's tiles."""
    c, Q = tok.shape[0], text.shape[0]
    ph, pw = guid.shape[-2:]
    lg = torch.empty(c, Q, ph * pw, dtype=torch.float32, device=tok.device)
    need = up.lib.sg_jbu_workspace_bytes(up._ctx, c, gh, gw)
    wp, wn = up._workspace(need)
    for q0 in range(0, Q, 32):
        qn = min(32, Q - q0)
        part = torch.empty(c, qn, ph * pw, dtype=torch.float32, device=tok.device)
        tq = text[q0:q0 + qn].contiguous()
        check(up.lib.sg_jbu_logits(up._ctx, ptr(tok), ptr(guid), c, gh, gw, ph, pw, up.precision, ptr(tq), qn, ptr(cls), lam, ptr(part), wp, wn,
                                   stream_ptr(up.device)), "sg_jbu_logits")
        lg[:, q0:q0 + qn] = part
    return lg


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiles", type=int, default=8)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--queries", default="32,48,64,130,256")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    C, g, crop = 768, 37, 512
    pad = (g * 14 - crop) // 2                                            # 518 = 512 + 3 + 3
    T = a.tiles
    rng = np.random.default_rng(0)
    tok = torch.from_numpy(rng.standard_normal((T, g * g, C), dtype=np.float32)).to(dev)
    cls = torch.from_numpy(rng.standard_normal((T, C), dtype=np.float32)).to(dev)
    scene = torch.from_numpy(Wt.make_tiles_u8(1, crop, seed=1, smooth=True)[0]).to(dev)
    windows = torch.tensor([[0, crop, 0, crop]] * T, dtype=torch.int32, device=dev)
    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    up = HipJBU("jbu_one", C, dev, "bf16")
    up.load_state_dict(Wt.make_jbu_weights("jbu_one", C, seed=3))
    for Q in (int(q) for q in a.queries.split(",")):
        text = torch.from_numpy(Wt.make_text_features(Q, C)).to(dev)
        run = lambda: up.logits(tok, cls, scene, windows, (crop, crop), (pad, pad), (g, g), text, 0.0, -0.3, padded_hw=(crop + 2 * pad, crop + 2 * pad))
        rec = {"kind": "jbu_one", "precision": "bf16", "C": C, "tiles": T, "tile": crop, "Q": Q}
        for name, fused in (("fused", True), ("fallback", False)):
            up.fused_tail = up.wide_tail = fused
            ms, peak, shape = timed(run, a.iters)
            rec[f"{name}_ms"] = round(ms, 3)
            rec[f"{name}_ms_per_tile"] = round(ms / T, 4)
            rec[f"{name}_peak_bytes"] = int(peak)
            if fused:
                rec["tail"] = up.lib.sg_jbu_last_kernels().decode().split("tail=")[-1]
                rec["out"] = list(shape)
        up.fused_tail = True
        emit(rec)
    del up
    torch.cuda.empty_cache()

    Q = 130
    text = torch.from_numpy(Wt.make_text_features(Q, C)).to(dev)
    up = HipJBU("bilinear", C, dev, "bf16")
    ph = crop + 2 * pad
    one = lambda: up.logits(tok, cls, scene, windows, (crop, crop), (pad, pad), (g, g), text, 0.0, -0.3, padded_hw=(ph, ph))
    guid = torch.zeros(T, 3, ph, ph, device=dev)                          # the bilinear kind never reads the guidance
    loop = lambda: bilinear_chunk_loop(up, tok, cls, guid, g, g, text, -0.3)
    rec = {"kind": "bilinear", "precision": "bf16", "C": C, "tiles": T, "tile": crop, "Q": Q}
    for name, run in (("one_call", one), ("chunk_loop", loop)):
        ms, peak, _ = timed(run, a.iters)
        rec[f"{name}_ms"] = round(ms, 3)
        rec[f"{name}_ms_per_tile"] = round(ms / T, 4)
        rec[f"{name}_peak_bytes"] = int(peak)
    emit(rec)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
