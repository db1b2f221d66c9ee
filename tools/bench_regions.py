"""The region table (sg_regions), measured on resident label maps of the bench scene, 2048 x 4608.  One JSON line per case.

    python tools/bench_regions.py [--steps 5 --warmup 2 --repeats 20 --out profiles/bench_regions.jsonl]
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/bench_regions.py --kernels
    python tools/bench_regions.py --kernel-trace DIR [--kernels-out profiles/bench_regions_kernels.jsonl]

Label maps: those of tools/bench_sieve.py (blocky, speckled 5 %, flat: one region of 9.4 Mpix, every contribution meets the same row).
Cases, per map, connectivity 4, min_area 1, nothing skipped, a table of 2^18 rows (the speckled map lists more regions than that: its
table is capped, its counts are not)
  bare       sg_regions: the table alone
  conf       with a per-pixel f32 confidence (SCORE_Q)
  map        with region_of
  sieve_bg   sg_sieve(fill="bg", min_region 16) in place on a fresh copy, the copy timed next to it and subtracted, as bench_sieve does
  copy       a device copy of the int64 map
  host       the route this replaces, if scipy is importable: the map to the host, ndimage.label per class, find_objects (once per
             map, wall clock)
All device routes alternate inside one round; `repeats` windows of `steps` calls, device events around a window; median and (min, max)
over the windows.  `ratio_to_sieve` = sg_regions / sg_sieve(bg).  --kernels runs the three sg_regions cases three times per map and
measures nothing itself; --kernel-trace reads the kernel trace of such a run and writes the time per kernel."""
import argparse
import csv
import glob
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

H, W, BG, ROWS = 2048, 4608, 0, 1 << 18
CASES = ("bare", "conf", "map")
MAPS = ("blocky", "speckled", "flat")
KERNELS = ("sieve_local", "sieve_merge", "sieve_flatten", "regions_count", "regions_scan", "regions_scatter", "regions_reduce")
REPS = 3                                                                      # calls per case of a --kernels run


def kernel_lines(trace_dir):
    """The kernel trace of a --kernels run -> one line per (map, case): the median time of each of the seven kernels over the calls."""
    rows = []
    for path in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        with open(path) as f:
            for r in csv.DictReader(f):
                name = next((k for k in KERNELS if k + "_kernel" in r["Kernel_Name"]), None)
                if name:
                    rows.append((int(r["Start_Timestamp"]), name, (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3))
    rows.sort()
    want = len(MAPS) * len(CASES) * REPS * len(KERNELS)
    if len(rows) != want:
        raise SystemExit(f"{len(rows)} kernels of sg_regions in the trace, {want} expected from one --kernels run")
    lines, k = [], 0
    for m in MAPS:
        for case in CASES:
            calls = []
            for _ in range(REPS):
                call = rows[k:k + len(KERNELS)]
                k += len(KERNELS)
                if tuple(n for _, n, _ in call) != KERNELS:
                    raise SystemExit(f"unexpected kernel order in the trace: {[n for _, n, _ in call]}")
                calls.append([us for _, _, us in call])
            us = {n: round(statistics.median(c[i] for c in calls), 1) for i, n in enumerate(KERNELS)}
            lines.append(json.dumps(dict(case="regions_kernels", scene=f"{H}x{W}", map=m, variant=case, connectivity=4, kernel_us=us,
                                         total_us=round(sum(us.values()), 1), largest=max(us, key=us.get),
                                         source=f"kernel trace of tools/bench_regions.py --kernels, median of {REPS} calls")))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--kernels", action="store_true", help="run every sg_regions case three times and measure nothing (for a profiler run)")
    ap.add_argument("--kernel-trace", default=None, help="the output directory of a profiler run over --kernels: write the time per kernel")
    ap.add_argument("--kernels-out", default=os.path.join(ROOT, "profiles", "bench_regions_kernels.jsonl"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_regions.jsonl"))
    a = ap.parse_args()
    if a.kernel_trace:
        lines = kernel_lines(a.kernel_trace)
        print("\n".join(lines))
        with open(a.kernels_out, "w") as f:
            f.write("\n".join(lines) + "\n")
        return
    import torch
    from bench_sieve import label_maps, spread, timed
    from clip_decontamination_amd import ops
    if not torch.cuda.is_available():
        raise SystemExit("bench_regions needs a GPU: nothing is measured without one")
    maps = label_maps()
    assert tuple(maps) == MAPS
    hw = [(H, W)]
    table = torch.empty(ROWS, ops.REGION_FIELDS, dtype=torch.int64, device="cuda")
    region_of = torch.empty(H * W, dtype=torch.int32, device="cuda")
    conf = torch.rand(H * W, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
    work = torch.empty(H * W, dtype=torch.int64, device="cuda")

    def routes(flat):
        return {"bare": lambda: ops.regions_table(flat, hw, None, 4, 1, None, ROWS, table),
                "conf": lambda: ops.regions_table(flat, hw, conf, 4, 1, None, ROWS, table),
                "map": lambda: ops.regions_table(flat, hw, None, 4, 1, None, ROWS, table, region_of)}

    if a.kernels:
        for m in maps.values():
            for fn in routes(m.view(-1)).values():
                for _ in range(REPS):
                    fn()
        torch.cuda.synchronize()
        return

    lines = []

    def emit(**kw):
        kw.update(scene=f"{H}x{W}", steps=a.steps, warmup=a.warmup, repeats=a.repeats, device=torch.cuda.get_device_name(0))
        line = json.dumps(kw)
        print(line, flush=True)
        lines.append(line)

    try:
        from scipy import ndimage
    except ImportError:
        ndimage = None
    mpix = H * W / 1e6
    for name, m in maps.items():
        flat = m.view(-1)
        r = routes(flat)
        r["sieve_copy"] = lambda: ops.sieve_flat(work.copy_(flat), hw, 16, 4, "bg", BG)
        r["copy"] = lambda: work.copy_(flat)
        t = timed(r, a)
        med = {k: statistics.median(v) for k, v in t.items()}
        sieve_ms = med["sieve_copy"] - med["copy"]
        total = int(r["bare"]()[-1])
        for case in CASES:
            emit(case="regions", variant=case, map=name, connectivity=4, min_area=1, regions=total, rows_written=min(total, ROWS),
                 regions_ms=spread(t[case]), us_per_mpix=round(1e3 * med[case] / mpix, 2), sieve_bg_ms=round(sieve_ms, 4),
                 sieve_window_ms=spread(t["sieve_copy"]), copy_ms=spread(t["copy"]), ratio_to_sieve=round(med[case] / sieve_ms, 2),
                 ratio_to_copy=round(med[case] / med["copy"], 2))
        if ndimage is None:
            emit(case="host", map=name, measured=False, why="scipy is not importable on this machine")
            continue
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host = m.cpu().numpy()
        t1 = time.perf_counter()
        found = 0
        for v in range(int(host.max()) + 1):
            lab, n = ndimage.label(host == v)
            ndimage.find_objects(lab)
            found += n
        t2 = time.perf_counter()
        emit(case="host", map=name, measured=True, regions=found, copy_to_host_ms=round(1e3 * (t1 - t0), 2),
             label_find_objects_ms=round(1e3 * (t2 - t1), 2), total_ms=round(1e3 * (t2 - t0), 2), calls=1,
             ratio_to_regions=round(1e3 * (t2 - t0) / med["bare"], 1))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
