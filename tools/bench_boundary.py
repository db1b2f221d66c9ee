"""Boundary IoU (sg_boundary_band / sg_boundary_accumulate), measured on resident label maps of the bench scene, 2048 x 4608, K = 16.
One JSON line per case.

    python tools/bench_boundary.py [--steps 5 --warmup 2 --repeats 20 --out profiles/bench_boundary.jsonl]

Label maps: the blocky, speckled and flat maps of tools/bench_sieve.py; the truth is the same map moved by (3, 5) pixels, as uint8.
Cases
  accumulate  ops.boundary_accumulate (both bands + the counts) for d in {1, 10, 101}, next to `confusion_ms` (sg_confusion_accumulate on
              the same buffers) and `copy_ms` (a device copy of the int64 label buffer), all from the same run; `bytes_per_pixel_at_copy_rate`
              = the time expressed in bytes per pixel at the copy's rate (the copy moves 16 B per pixel).
  band        ops.boundary_band_flat alone on the int64 map, same widths.
  width       per map: time at d = 101 over time at d = 1, for both entries -- the check that the work per pixel does not grow with d
              (what remains is the column pass's halo of 2d rows per row band).
  host        once per width, on the blocky map: the label maps copied to the host, then Boundary IoU there by per-class erosion (cv2,
              else scipy.ndimage, else the numpy reference of tests/); `host_ms` is one run and includes the copy.
`repeats` windows of `steps` calls, device events around a window; median and (min, max) over the windows.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from clip_decontamination_amd import ops  # noqa: E402
from bench_sieve import H, W, K, label_maps, spread, timed  # noqa: E402

WIDTHS = (1, 10, 101)
SHIFT = (3, 5)


def host_route(pred, gt, d):
    """Boundary IoU counts on the host as one would write them today: copy, then per class mask - erode^d(pad0(mask)) for prediction and
    truth.  -> (areas int64 [3,K], seconds, the library used)."""
    t0 = time.perf_counter()
    p, g = pred.cpu().numpy(), gt.cpu().numpy()
    try:
        import cv2
        lib = "cv2"
        kernel = np.ones((3, 3), dtype=np.uint8)

        def band(mask):
            padded = cv2.copyMakeBorder(mask, 1, 1, 1, 1, cv2.BORDER_CONSTANT, value=0)
            return mask - cv2.erode(padded, kernel, iterations=d)[1:-1, 1:-1]
    except ImportError:
        try:
            from scipy import ndimage
            lib = "scipy.ndimage"
            st = np.ones((3, 3), dtype=bool)

            def band(mask):
                return mask & ~ndimage.binary_erosion(mask.astype(bool), structure=st, iterations=d, border_value=0)
        except ImportError:
            sys.path.insert(0, os.path.join(ROOT, "tests"))
            import boundary_reference
            lib = "numpy reference"

            def band(mask):
                return mask & boundary_reference.band(mask, d)
    areas = np.zeros((3, K), dtype=np.int64)
    for k in range(K):
        bp, bg = band((p == k).astype(np.uint8)).astype(bool), band((g == k).astype(np.uint8)).astype(bool)
        areas[:, k] = np.count_nonzero(bp & bg), np.count_nonzero(bp), np.count_nonzero(bg)
    return areas, time.perf_counter() - t0, lib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--no-host", action="store_true", help="skip the host route")
    ap.add_argument("--host-widths", type=int, nargs="*", default=list(WIDTHS))
    ap.add_argument("--host-map", default="blocky", help="the map the host route runs on")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_boundary.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_boundary needs a GPU: nothing is measured without one")
    mpix = H * W / 1e6
    lines = []

    def emit(**kw):
        kw.update(scene=f"{H}x{W}", K=K, steps=a.steps, warmup=a.warmup, repeats=a.repeats, device=torch.cuda.get_device_name(0))
        line = json.dumps(kw)
        print(line, flush=True)
        lines.append(line)

    work = torch.empty(H * W, dtype=torch.int64, device="cuda")
    for name, m in label_maps().items():
        flat = m.view(-1)
        gt = torch.roll(m, SHIFT, (0, 1)).to(torch.uint8).contiguous().view(-1)
        table = torch.zeros(K + 1, K + 1, dtype=torch.int64, device="cuda")
        areas = torch.zeros(3, K, dtype=torch.int64, device="cuda")
        routes = {"copy": lambda: work.copy_(flat), "confusion": lambda: ops.confusion_accumulate(flat, gt, table, K)}
        for d in WIDTHS:
            routes[f"accumulate_{d}"] = lambda d=d: ops.boundary_accumulate(flat, gt, [(H, W)], d, areas, K)
            routes[f"band_{d}"] = lambda d=d: ops.boundary_band_flat(flat, [(H, W)], d)
        t = timed(routes, a)
        med = {k: statistics.median(v) for k, v in t.items()}
        per_byte = med["copy"] / 16.0                                     # the copy reads and writes 8 B per pixel
        for d in WIDTHS:
            one = torch.zeros(3, K, dtype=torch.int64, device="cuda")
            ops.boundary_accumulate(flat, gt, [(H, W)], d, one, K)
            band = ops.boundary_band_flat(flat, [(H, W)], d)
            one = one.cpu().numpy().astype(np.float64)
            with np.errstate(divide="ignore", invalid="ignore"):
                mbiou = float(np.nanmean(one[0] / (one[1] + one[2] - one[0])))
            emit(case="accumulate", map=name, d=d, band_share=round(float(band.float().mean()), 5), mBIoU=round(mbiou, 5),
                 accumulate_ms=spread(t[f"accumulate_{d}"]), us_per_mpix=round(1e3 * med[f"accumulate_{d}"] / mpix, 2),
                 confusion_ms=spread(t["confusion"]), copy_ms=spread(t["copy"]), ratio_to_copy=round(med[f"accumulate_{d}"] / med["copy"], 2),
                 ratio_to_confusion=round(med[f"accumulate_{d}"] / med["confusion"], 2),
                 bytes_per_pixel_at_copy_rate=round(med[f"accumulate_{d}"] / per_byte, 1))
            emit(case="band", map=name, d=d, band_ms=spread(t[f"band_{d}"]), us_per_mpix=round(1e3 * med[f"band_{d}"] / mpix, 2),
                 copy_ms=spread(t["copy"]), ratio_to_copy=round(med[f"band_{d}"] / med["copy"], 2),
                 bytes_per_pixel_at_copy_rate=round(med[f"band_{d}"] / per_byte, 1))
        emit(case="width", map=name, accumulate_d101_over_d1=round(med["accumulate_101"] / med["accumulate_1"], 3),
             band_d101_over_d1=round(med["band_101"] / med["band_1"], 3))
        if not a.no_host and name == a.host_map:
            for d in a.host_widths:
                got = torch.zeros(3, K, dtype=torch.int64, device="cuda")
                ops.boundary_accumulate(flat, gt, [(H, W)], d, got, K)
                want, sec, lib = host_route(m, gt.view(H, W), d)
                emit(case="host", map=name, d=d, library=lib, host_ms=round(1e3 * sec, 1), equal_to_device=bool(np.array_equal(got.cpu().numpy(), want)),
                     device_ms=round(med[f"accumulate_{d}"], 4), ratio=round(1e3 * sec / med[f"accumulate_{d}"], 1))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
