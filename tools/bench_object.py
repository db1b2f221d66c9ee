"""Object-level matching (sg_object_match), measured on resident label maps of the bench scene, 2048 x 4608.  One JSON line per case.

    python tools/bench_object.py [--steps 5 --warmup 2 --repeats 20 --out profiles/bench_object.jsonl]

Label maps: the blocky, speckled and flat maps of tools/bench_sieve.py (K = 16) and "buildings" (K = 2): a few thousand rectangles of 10 to
60 px on background; the truth is the same map moved by (3, 5) pixels, as uint8.
Cases
  match   ops.object_match at the thresholds 1/2 and 3/4, with and without match_map, next to `regions2_ms` (two sg_regions calls, one on
          each of the two maps: the labelling is done twice there too) and `copy_ms` (a device copy of the int64 label buffer) on the same
          buffers, all from the same run, with the ratios to each.
  host    once on one map (default: buildings): both maps copied to the host, scipy.ndimage.label per class and map, the table of the
          intersections of all pairs, the integer rule; `host_ms` is one run and includes the copy; `equal_to_device` at both thresholds.
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
from bench_sieve import H, W, K, BG, label_maps, spread, timed  # noqa: E402

SHIFT = (3, 5)
IOUS = ((1, 2), (3, 4))
N_BUILDINGS = 4000


def buildings_map():
    """Rectangles of 10 to 60 px of class 1 on background 0, drawn on the host once (a fixed seed); overlapping ones merge."""
    rng = np.random.default_rng(5)
    m = np.zeros((H, W), dtype=np.int64)
    for _ in range(N_BUILDINGS):
        h, w = (int(v) for v in rng.integers(10, 61, 2))
        y, x = int(rng.integers(0, H - h)), int(rng.integers(0, W - w))
        m[y:y + h, x:x + w] = 1
    return torch.from_numpy(m).cuda()


def host_route(pred, gt, k, skip, ious):
    """The counts on the host as one would write them today -> ({iou: counts int64 [4,k]}, seconds)."""
    from scipy import ndimage
    t0 = time.perf_counter()
    p, g = pred.cpu().numpy(), gt.cpu().numpy().astype(np.int64)
    out = {iou: np.zeros((4, k), dtype=np.int64) for iou in ious}
    for c in range(k):
        if c == skip:
            continue
        lp, n_p = ndimage.label(p == c)
        lg, n_g = ndimage.label(g == c)
        for iou in ious:
            out[iou][1, c], out[iou][2, c] = n_p, n_g
        if n_p == 0 or n_g == 0:
            continue
        ap, ag = np.bincount(lp.reshape(-1), minlength=n_p + 1), np.bincount(lg.reshape(-1), minlength=n_g + 1)
        both = (lp > 0) & (lg > 0)
        code, inter = np.unique(lp[both].astype(np.int64) * (n_g + 1) + lg[both], return_counts=True)
        a, b = code // (n_g + 1), code % (n_g + 1)
        union = ap[a] + ag[b] - inter
        for num, den in ious:
            ok = inter * den > num * union
            out[(num, den)][0, c] = int(ok.sum())
            out[(num, den)][3, c] = int(((inter[ok] << 24) // union[ok]).sum())
    return out, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--no-host", action="store_true", help="skip the host route")
    ap.add_argument("--host-map", default="buildings", help="the map the host route runs on")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_object.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_object needs a GPU: nothing is measured without one")
    mpix = H * W / 1e6
    lines = []

    def emit(**kw):
        kw.update(scene=f"{H}x{W}", steps=a.steps, warmup=a.warmup, repeats=a.repeats, device=torch.cuda.get_device_name(0))
        line = json.dumps(kw)
        print(line, flush=True)
        lines.append(line)

    work = torch.empty(H * W, dtype=torch.int64, device="cuda")
    mm = torch.empty(H * W, dtype=torch.uint8, device="cuda")
    maps = {n: (m, K) for n, m in label_maps().items()}
    maps["buildings"] = (buildings_map(), 2)
    rows = 1 << 18
    table = torch.empty(rows, ops.REGION_FIELDS, dtype=torch.int64, device="cuda")
    for name, (m, k) in maps.items():
        flat = m.contiguous().view(-1)
        gt = torch.roll(m, SHIFT, (0, 1)).to(torch.uint8).contiguous().view(-1)
        gt64 = gt.to(torch.int64)
        counts = torch.zeros(4, k, dtype=torch.int64, device="cuda")

        def regions2():
            ops.regions_table(flat, [(H, W)], None, 4, 1, BG, rows, table)
            ops.regions_table(gt64, [(H, W)], None, 4, 1, BG, rows, table)

        routes = {"copy": lambda: work.copy_(flat), "regions2": regions2}
        for iou in IOUS:
            routes[f"match_{iou[0]}_{iou[1]}"] = lambda iou=iou: ops.object_match(flat, gt, [(H, W)], counts, k, iou, skip_label=BG)
            routes[f"match_{iou[0]}_{iou[1]}_map"] = lambda iou=iou: ops.object_match(flat, gt, [(H, W)], counts, k, iou, skip_label=BG, match_map=mm)
        ts = timed(routes, a)
        med = {n: statistics.median(v) for n, v in ts.items()}
        for iou in IOUS:
            one = torch.zeros(4, k, dtype=torch.int64, device="cuda")
            ops.object_match(flat, gt, [(H, W)], one, k, iou, skip_label=BG)
            c = one.cpu().numpy()
            for with_map in (False, True):
                key = f"match_{iou[0]}_{iou[1]}" + ("_map" if with_map else "")
                emit(case="match", map=name, K=k, iou=f"{iou[0]}/{iou[1]}", match_map=with_map, matched=int(c[0].sum()), predicted=int(c[1].sum()),
                     true=int(c[2].sum()), match_ms=spread(ts[key]), us_per_mpix=round(1e3 * med[key] / mpix, 2), regions2_ms=spread(ts["regions2"]),
                     copy_ms=spread(ts["copy"]), ratio_to_regions2=round(med[key] / med["regions2"], 2), ratio_to_copy=round(med[key] / med["copy"], 2))
        if not a.no_host and name == a.host_map:
            want, sec = host_route(m, gt.view(H, W), k, BG, IOUS)
            equal = True
            for iou in IOUS:
                got = torch.zeros(4, k, dtype=torch.int64, device="cuda")
                ops.object_match(flat, gt, [(H, W)], got, k, iou, skip_label=BG)
                equal = equal and bool(np.array_equal(got.cpu().numpy(), want[iou]))
            emit(case="host", map=name, K=k, library="scipy.ndimage", host_ms=round(1e3 * sec, 1), equal_to_device=equal,
                 device_ms={f"{n}/{d}": round(med[f"match_{n}_{d}"], 4) for n, d in IOUS})
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
