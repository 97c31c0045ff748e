#!/usr/bin/env python3
"""Summarize a rocprofv3 results.db: top kernels by total time.

    python scripts/prof_summary.py 'GLOB/of/results.db' [--by-grid]

--by-grid gives every (kernel, grid) its own line, so a kernel that runs in
both prefill and decode (silu_mul, the hipBLASLt GEMMs) shows the two apart
instead of one mean over both. The grid is printed in workgroups.
"""
import glob
import sqlite3
import sys

args = [a for a in sys.argv[1:] if not a.startswith("--")]
by_grid = "--by-grid" in sys.argv[1:]
db_path = sorted(glob.glob(args[0]))[-1]
db = sqlite3.connect(db_path)
cur = db.cursor()
if by_grid:
    # the `kernels` view has one row per dispatch: duration in ns, the grid
    # in work-items
    rows = list(cur.execute(
        "SELECT name, grid_x / workgroup_x, grid_y / workgroup_y, "
        "grid_z / workgroup_z, COUNT(*), SUM(duration) / 1000.0 AS tot "
        "FROM kernels GROUP BY 1, 2, 3, 4 ORDER BY tot DESC LIMIT 40"))
    total = cur.execute("SELECT SUM(duration) / 1000.0 FROM kernels").fetchone()[0]
    for name, gx, gy, gz, calls, tot in rows:
        short = name.split("(")[0][:80]
        grid = f"({gx},{gy},{gz})"
        print(f"{100 * tot / total:5.1f}%  n={calls:6d}  avg={tot / calls:9.1f}us  "
              f"tot={tot/1e3:9.1f}ms  grid={grid:14s} {short}")
else:
    rows = list(cur.execute(
        "SELECT name, total_calls, total_duration, average, percentage "
        "FROM top_kernels LIMIT 25"))
    for name, calls, tot, avg, pct in rows:
        short = name.split("(")[0][:90]
        print(f"{pct:5.1f}%  n={calls:6d}  avg={avg:9.1f}us  tot={tot/1e3:9.1f}ms  {short}")
