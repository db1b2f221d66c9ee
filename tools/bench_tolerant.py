"""Relaxed precision / recall and the boundary F-score (sg_tolerant_accumulate), measured on resident label maps of the bench scene,
2048 x 4608.  One JSON line per case.

    python tools/bench_tolerant.py [--steps 5 --warmup 2 --repeats 20 --out profiles/bench_tolerant.jsonl]

Label maps: the blocky, speckled and flat maps of tools/bench_sieve.py (K = 16) and a binary map of two-pixel-wide lines, "road" (K = 2);
the truth is the same map moved by (3, 5) pixels, as uint8.
Cases
  accumulate  ops.tolerant_accumulate in both modes at 3 px (tol_sq = 9) and at the ratio rule's 38 px (tol_sq = 1444), next to
              `boundary_ms` (sg_boundary_accumulate at d = 10), `confusion_ms` (sg_confusion_accumulate) and `copy_ms` (a device copy of
              the int64 label buffer) on the same buffers, all from the same run, with the ratios to each.
  radius      per map and mode: the time at 38 px over the time at 3 px -- what the linear walk costs.
  host        once per mode on one map (default: road): the label maps copied to the host, then scipy.ndimage.distance_transform_edt per
              class and direction; `host_ms` is one run and includes the copy; `equal_to_device` at both tolerances.
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

SHIFT = (3, 5)
MODES = ("region", "contour")
BOUNDARY_D = 10


def road_map():
    yy, xx = torch.meshgrid(torch.arange(H, device="cuda"), torch.arange(W, device="cuda"), indexing="ij")
    return (((yy % 97) < 2) | (((xx + yy // 3) % 131) < 2)).to(torch.int64).contiguous()


def contour(lab):
    out = np.zeros(lab.shape, dtype=bool)
    out[1:, :] |= lab[1:, :] != lab[:-1, :]
    out[:-1, :] |= lab[:-1, :] != lab[1:, :]
    out[:, 1:] |= lab[:, 1:] != lab[:, :-1]
    out[:, :-1] |= lab[:, :-1] != lab[:, 1:]
    return out


def host_route(pred, gt, k, mode, tols):
    """The counts on the host as one would write them today: copy, then an exact Euclidean distance transform per class and direction.
    -> ({tol_sq: counts int64 [4,k]}, seconds)."""
    from scipy import ndimage
    t0 = time.perf_counter()
    p, g = pred.cpu().numpy(), gt.cpu().numpy().astype(np.int64)
    mp, mg = (contour(p), contour(g)) if mode == "contour" else (np.ones(p.shape, bool), np.ones(p.shape, bool))
    counted = g != 255
    out = {t: np.zeros((4, k), dtype=np.int64) for t in tols}
    for c in range(k):
        sp, sg = mp & (p == c), mg & (g == c)
        dg = np.rint(ndimage.distance_transform_edt(~sg) ** 2) if sg.any() else np.full(p.shape, np.inf)
        dp = np.rint(ndimage.distance_transform_edt(~sp) ** 2) if sp.any() else np.full(p.shape, np.inf)
        for t in tols:
            out[t][:, c] = (np.count_nonzero(sp & counted), np.count_nonzero(sp & counted & (dg <= t)),
                            np.count_nonzero(sg & counted), np.count_nonzero(sg & counted & (dp <= t)))
    return out, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--no-host", action="store_true", help="skip the host route")
    ap.add_argument("--host-map", default="road", help="the map the host route runs on")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_tolerant.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_tolerant needs a GPU: nothing is measured without one")
    mpix = H * W / 1e6
    tols = (9, ops.tolerance_sq((H, W)))                                   # 3 px and the ratio rule: 38 px
    lines = []

    def emit(**kw):
        kw.update(scene=f"{H}x{W}", steps=a.steps, warmup=a.warmup, repeats=a.repeats, device=torch.cuda.get_device_name(0))
        line = json.dumps(kw)
        print(line, flush=True)
        lines.append(line)

    work = torch.empty(H * W, dtype=torch.int64, device="cuda")
    maps = {n: (m, K) for n, m in label_maps().items()}
    maps["road"] = (road_map(), 2)
    for name, (m, k) in maps.items():
        flat = m.view(-1)
        gt = torch.roll(m, SHIFT, (0, 1)).to(torch.uint8).contiguous().view(-1)
        table = torch.zeros(k + 1, k + 1, dtype=torch.int64, device="cuda")
        areas = torch.zeros(3, k, dtype=torch.int64, device="cuda")
        counts = torch.zeros(4, k, dtype=torch.int64, device="cuda")
        routes = {"copy": lambda: work.copy_(flat), "confusion": lambda: ops.confusion_accumulate(flat, gt, table, k),
                  "boundary": lambda: ops.boundary_accumulate(flat, gt, [(H, W)], BOUNDARY_D, areas, k)}
        for mode in MODES:
            for t in tols:
                routes[f"{mode}_{t}"] = lambda mode=mode, t=t: ops.tolerant_accumulate(flat, gt, [(H, W)], t, counts, k, mode=mode)
        ts = timed(routes, a)
        med = {n: statistics.median(v) for n, v in ts.items()}
        for mode in MODES:
            for t in tols:
                one = torch.zeros(4, k, dtype=torch.int64, device="cuda")
                ops.tolerant_accumulate(flat, gt, [(H, W)], t, one, k, mode=mode)
                c = one.cpu().numpy().astype(np.float64)
                with np.errstate(divide="ignore", invalid="ignore"):
                    pr, rc = c[1] / c[0], c[3] / c[2]
                    f = float(np.nanmean(2 * pr * rc / (pr + rc))) if np.isfinite(2 * pr * rc / (pr + rc)).any() else float("nan")
                key = f"{mode}_{t}"
                emit(case="accumulate", map=name, K=k, mode=mode, tol_sq=t, mean_F=round(f, 5), sources=int(c[0].sum() + c[2].sum()),
                     accumulate_ms=spread(ts[key]), us_per_mpix=round(1e3 * med[key] / mpix, 2), boundary_ms=spread(ts["boundary"]),
                     confusion_ms=spread(ts["confusion"]), copy_ms=spread(ts["copy"]), ratio_to_boundary=round(med[key] / med["boundary"], 2),
                     ratio_to_confusion=round(med[key] / med["confusion"], 2), ratio_to_copy=round(med[key] / med["copy"], 2))
            emit(case="radius", map=name, K=k, mode=mode, r38_over_r3=round(med[f"{mode}_{tols[1]}"] / med[f"{mode}_{tols[0]}"], 3))
        if not a.no_host and name == a.host_map:
            for mode in MODES:
                want, sec = host_route(m, gt.view(H, W), k, mode, tols)
                equal = True
                for t in tols:
                    got = torch.zeros(4, k, dtype=torch.int64, device="cuda")
                    ops.tolerant_accumulate(flat, gt, [(H, W)], t, got, k, mode=mode)
                    equal = equal and bool(np.array_equal(got.cpu().numpy(), want[t]))
                emit(case="host", map=name, K=k, mode=mode, library="scipy.ndimage", host_ms=round(1e3 * sec, 1), equal_to_device=equal,
                     device_ms={str(t): round(med[f"{mode}_{t}"], 4) for t in tols})
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
