"""The device-side IoU metric, measured: sg_confusion_accumulate alone, and evaluate() against the routes around it.  One JSON line
per case.

    python tools/bench_metric.py --steps 20 --warmup 3 --repeats 5 [--cases kernel,path] [--images 119]

Cases
  kernel  one 4096 x 4096 map (16.8 Mpix) per launch: random / blocky (constant 64 x 64 squares) / uniform contents, K = 6 and 16, u8
          and int64 truth.  Device-event time per launch, `repeats` windows of `steps` launches each (median and spread), next to the
          HBM floor of 9 B (16 B) per pixel at the rate a 1 GiB device-to-device copy reaches in the same run (its own JSON line,
          case "copy": bytes read plus bytes written over time) and at the 8 TB/s on the data sheet.
  path    the Potsdam-like set of tools/bench_batch.py (case a_bf16: 119 images of 512^2, ViT-L/14, crop = stride = 512), three routes
          from images to an mIoU, interleaved in `repeats` rounds, host clock to a device synchronise:
            evaluate     SegmentorEx.evaluate(): packed labels, truth to the device once, one count launch per flush group, the table back
                         (its host side alone -- concatenating the truth maps and copying them to the device -- is timed as truth_upload_ms)
            labels_only  predict_many() alone: the packed labels-only path, no score
            host_route   what there was before: predict_many(), every label map copied to the host and scored there by the integer
                         restatement of mmseg's formula (tests/iou_reference.py)
          The tables of evaluate and host_route are checked equal.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from clip_decontamination_amd import ops, weights as Wt  # noqa: E402

HBM_SPEC = 8.0e12                                      # bytes / s, data sheet


def copy_rate(a):
    """Bytes per second (read + written) of a 1 GiB device-to-device copy on this box, this run: the yardstick of the HBM floors."""
    src = torch.empty(1 << 28, dtype=torch.float32, device="cuda").normal_()
    dst = torch.empty_like(src)
    for _ in range(a.warmup):
        dst.copy_(src)
    rates = []
    for _ in range(a.repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.steps):
            dst.copy_(src)
        e1.record()
        e1.synchronize()
        rates.append(2 * src.numel() * 4 * a.steps / (e0.elapsed_time(e1) * 1e-3) / 1e12)
    print(json.dumps(dict(case="copy", bytes_each_way=src.numel() * 4, tb_per_s=spread(rates), steps=a.steps, warmup=a.warmup,
                          repeats=a.repeats, device=torch.cuda.get_device_name(0))), flush=True)
    return statistics.median(rates) * 1e12


def maps(kind, n, K, seed=0):
    rng = np.random.default_rng(seed)
    if kind == "random":
        return rng.integers(0, K, (n, n)), rng.integers(0, K, (n, n))
    if kind == "blocky":
        g = rng.integers(0, K, (n // 64, n // 64))
        p = np.where(rng.random(g.shape) < 0.25, rng.integers(0, K, g.shape), g)
        up = lambda a: np.kron(a, np.ones((64, 64), dtype=np.int64))
        return up(p), up(g)
    return np.full((n, n), 2 % K), np.full((n, n), 2 % K)


def spread(xs):
    return dict(median=round(statistics.median(xs), 4), min=round(min(xs), 4), max=round(max(xs), 4))


def kernel_cases(a):
    hbm = copy_rate(a)
    n = 4096
    mpix = n * n / 1e6
    for fmt, nbytes in (("u8", 9), ("i64", 16)):
        for K in (6, 16):
            for kind in ("random", "blocky", "uniform"):
                p, g = maps(kind, n, K)
                lab = torch.from_numpy(p.astype(np.int64)).cuda()
                gt = torch.from_numpy(g.astype(np.uint8 if fmt == "u8" else np.int64)).cuda()
                t = torch.zeros(K + 1, K + 1, dtype=torch.int64, device="cuda")
                for _ in range(a.warmup):
                    ops.confusion_accumulate(lab, gt, t, K)
                us = []
                for _ in range(a.repeats):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(a.steps):
                        ops.confusion_accumulate(lab, gt, t, K)
                    e1.record()
                    e1.synchronize()
                    us.append(e0.elapsed_time(e1) * 1e3 / a.steps / mpix)
                assert int(t.sum()) == (a.warmup + a.repeats * a.steps) * n * n
                med = statistics.median(us)
                print(json.dumps(dict(case="kernel", contents=kind, K=K, truth=fmt, pixels=n * n, bytes_per_pixel=nbytes,
                                      us_per_mpix=spread(us), tb_per_s=round(nbytes * 1e6 / (med * 1e-6) / 1e12, 3),
                                      floor_us_per_mpix_at_copy_rate=round(nbytes * 1e6 / hbm * 1e6, 4),
                                      floor_us_per_mpix_spec_hbm=round(nbytes * 1e6 / HBM_SPEC * 1e6, 4),
                                      steps=a.steps, warmup=a.warmup, repeats=a.repeats, device=torch.cuda.get_device_name(0))), flush=True)


def path_case(a):
    hbm = copy_rate(a)
    import iou_reference as R
    import segmentor
    n, S = a.images, 512
    cfg = Wt.vit_config("ViT-L/14")
    seg = segmentor.SegmentorEx(clip_type="CLIP", vit_type="ViT-L/14", model_type="Experimental", name_path=os.path.join(ROOT, "configs", "cls_potsdam.txt"),
                                device=torch.device("cuda:0"), precision="bf16", synthetic_ok=True, global_debias_factor=0.2, prob_thd=0.1,
                                bg_idx=5, apply_sim_feat_up=False, slide_crop=512, slide_stride=512, tiles_per_launch=min(n, 119),
                                text_features=torch.from_numpy(Wt.make_text_features(8, cfg.embed_dim)))
    K = seg.num_classes
    u8 = torch.from_numpy(Wt.make_tiles_u8(n, S, seed=7, smooth=True)).cuda()
    mean = torch.tensor(Wt.PIXEL_MEAN, device="cuda").view(1, 3, 1, 1)
    std = torch.tensor(Wt.PIXEL_STD, device="cuda").view(1, 3, 1, 1)
    imgs = (u8.permute(0, 3, 1, 2).float() - mean) / std                                   # [n,3,512,512] f32, what predict() receives
    del u8
    gts = [maps("blocky", S, K, seed=100 + i)[1].astype(np.uint8) for i in range(n)]

    def host_route():
        labels = seg.predict_many(imgs)
        tot = [np.zeros(K, dtype=np.int64) for _ in range(4)]
        for lab, g in zip(labels, gts):
            for t_, x in zip(tot, R.intersect_and_union(lab.cpu().numpy(), g, K)):
                t_ += x
        return R.total_area_to_metrics(*tot), tot

    def upload():                                         # the host side of evaluate() alone: one concatenation, one copy to the device
        return torch.cat([torch.as_tensor(g).reshape(-1) for g in gts]).to("cuda")

    up_ms = []
    for _ in range(a.warmup + a.repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        upload()
        torch.cuda.synchronize()
        up_ms.append((time.perf_counter() - t0) * 1e3)
    up_ms = up_ms[a.warmup:]
    routes = {"evaluate": lambda: seg.evaluate(imgs, gts), "labels_only": lambda: seg.predict_many(imgs), "host_route": host_route}
    outs = {}
    for _ in range(a.warmup):
        outs = {k: f() for k, f in routes.items()}
    torch.cuda.synchronize()
    times = {k: [] for k in routes}
    for _ in range(a.repeats):
        for k, f in routes.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            outs[k] = f()
            torch.cuda.synchronize()
            times[k].append(time.perf_counter() - t0)
    from clip_decontamination_amd.metrics import areas_from_confusion
    same = all(np.array_equal(x, y) for x, y in zip(areas_from_confusion(outs["evaluate"][1].confusion), (outs["host_route"][1][i] for i in (0, 1, 2, 3))))
    mpix = n * S * S / 1e6
    med = {k: statistics.median(v) for k, v in times.items()}
    print(json.dumps(dict(case="path", vit="ViT-L/14", precision="bf16", images=n, image_hw=[S, S], crop=512, stride=512,
                          seconds={k: spread(v) for k, v in times.items()}, mpix_per_s={k: round(mpix / med[k], 2) for k in med},
                          evaluate_minus_labels_only_ms=round((med["evaluate"] - med["labels_only"]) * 1e3, 3),
                          count_pass_floor_ms=round(9 * n * S * S / hbm * 1e3, 4), truth_upload_mb=round(n * S * S / 1e6, 1), truth_upload_ms=spread(up_ms),
                          host_route_over_evaluate=round(med["host_route"] / med["evaluate"], 3), areas_equal=bool(same),
                          mIoU=outs["evaluate"][0]["summary"]["mIoU"], warmup=a.warmup, repeats=a.repeats,
                          device=torch.cuda.get_device_name(0))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20, help="launches per timed window (kernel case)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5, help="timed windows (kernel case) / interleaved rounds (path case)")
    ap.add_argument("--cases", default="kernel,path")
    ap.add_argument("--images", type=int, default=119)
    a = ap.parse_args()
    if a.steps < 1 or a.warmup < 0 or a.repeats < 1 or a.images < 1:
        ap.error("--steps, --repeats and --images must be >= 1 and --warmup >= 0")
    if not torch.cuda.is_available():
        sys.exit("bench_metric.py measures on the GPU; none is visible")
    for name in a.cases.split(","):
        {"kernel": kernel_cases, "path": path_case}[name](a)


if __name__ == "__main__":
    main()
