#!/usr/bin/env python3
"""Per-kernel table of one bench.py step from three rocprofv3 runs of the SAME command (rocpd sqlite databases):

    rocprofv3 --kernel-trace --stats -d T -- python3 bench.py ...      durations
    rocprofv3 --pmc FETCH_SIZE      -d F -- python3 bench.py ...      HBM-side read traffic   (own pass: TCC slots)
    rocprofv3 --pmc WRITE_SIZE      -d W -- python3 bench.py ...      HBM-side write traffic  (own pass)

    python tools/pmc_table.py T/*/*.db F/*/*.db W/*/*.db STEPS [TILES_PER_LAYER [PEELED_TILES]] > profiles/rNN_pmc.csv

STEPS = steps the command ran (warm-up + timed), to turn call counts into launches per step.  Kernels are keyed by
(name, grid size) so that the shapes of one template show up separately.  traffic_bytes applies the corrections of
MI355X_MICROARCH.md (HBM section): FETCH_SIZE is reported in KiB and, on gfx950, at half the bytes of wide streaming
reads -> x 2 x 1024; WRITE_SIZE KiB -> x 1024.  bench.py reads this file for `roofline.traffic`.
A grouped or window weight-gradient launch (gemm2_kernel_grouped: one workgroup of 512 per 256 x 256 tile, so its grid size / 512 is its tile
count - 216 for two bert-base layers, 256 for a full window) is listed PER LAYER'S WORTH of tiles it covers (TILES_PER_LAYER, default 108:
bert-base) - launches x tiles / TILES_PER_LAYER, duration and bytes / (tiles / TILES_PER_LAYER) - because that is the unit bench.py's
`roofline` object counts in (one event pair and one layer's algorithmic bytes per "launch").  Next to window launches the split-K
weight-gradient launch that is left (gemm2_kernel<..., 6>) is the peeled QKV + attention-out pair, PEELED_TILES (default 36) tiles:
listed in the same unit, so that the launches of a step add up to its layers.  Windows are recognised by a grouped launch of more than
two layers' tiles, and then EVERY gemm2_kernel<..., 6> row is taken for the peeled pair: right for a step whose layers all train (the
benchmark), wrong for a run that mixes windows with other split-K weight gradients (frozen or skipped matrices, a second model shape) -
pass PEELED_TILES = TILES_PER_LAYER there to list those rows as they are.
"""
import csv
import re
import sqlite3
import sys


def short(name):
    name = re.sub(r"\(anonymous namespace\)::", "", name)
    name = re.sub(r"^void ", "", name)
    name = re.sub(r"\(.*\)$", "", name)          # drop the argument list
    return name


def durations(path):
    c = sqlite3.connect(path)
    out = {}
    for name, grid, n, avg in c.execute("select name, grid_x * grid_y * grid_z, count(*), avg(end - start) from kernels group by 1, 2"):
        out[(short(name), int(grid))] = (n, avg / 1e3)
    return out


def counter(path, which):
    c = sqlite3.connect(path)
    out = {}
    for name, grid, n, avg in c.execute("select kernel_name, grid_size, count(*), avg(value) from counters_collection "
                                        "where counter_name = ? group by kernel_name, grid_size", (which,)):
        out[(short(name), int(grid))] = (n, avg)
    return out


def main():
    trace, fetch, write, steps = sys.argv[1], sys.argv[2], sys.argv[3], float(sys.argv[4])
    per_layer = float(sys.argv[5]) if len(sys.argv) > 5 else 108.0
    peeled = float(sys.argv[6]) if len(sys.argv) > 6 else 36.0
    d, f, w = durations(trace), counter(fetch, "FETCH_SIZE"), counter(write, "WRITE_SIZE")
    windows = any("gemm2_kernel_grouped" in k[0] and k[1] / 512 > 2 * per_layer for k in d)
    rows = []
    for key, (n, us) in d.items():
        if n < steps * 0.5:          # set-up kernels (initialisation, casts before the loop)
            continue
        fk, wk = f.get(key, (0, float("nan")))[1], w.get(key, (0, float("nan")))[1]
        group = 1.0
        if "gemm2_kernel_grouped" in key[0]:
            group = key[1] / 512 / per_layer
        elif windows and key[0].startswith("gemm2_kernel<") and key[0].rstrip(">").endswith(", 6"):
            group = peeled / per_layer
        n, us, fk, wk = n * group, us / group, fk / group, wk / group
        rows.append((n / steps * us, key[0], key[1], n / steps, us, fk, wk, (2.0 * fk + wk) * 1024.0))
    rows.sort(reverse=True)
    out = csv.writer(sys.stdout)
    out.writerow(["kernel", "grid_size", "launches_per_step", "avg_us", "ms_per_step", "FETCH_SIZE_KiB_avg", "WRITE_SIZE_KiB_avg",
                  "traffic_bytes_per_launch"])
    for ms, name, grid, per, us, fk, wk, tb in rows:
        out.writerow([name, grid, "%.2f" % per, "%.2f" % us, "%.4f" % (ms / 1e3), "%.1f" % fk, "%.1f" % wk, "%.0f" % tb])


if __name__ == "__main__":
    main()
