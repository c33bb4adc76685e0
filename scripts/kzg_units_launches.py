#!/usr/bin/env python3
"""The kernel launches of a `rocprofv3 --kernel-trace --output-format csv -d DIR` run, one per line
in the order of dispatch: name without its argument list, grid (in work-items) and block. Start
times are no order to compare by: the MSM forks onto side streams.
Usage: kzg_units_launches.py DIR"""
import csv
import glob
import os
import re
import sys

rows = []
for f in glob.glob(os.path.join(sys.argv[1], "**", "*kernel_trace.csv"), recursive=True):
    with open(f) as fh:
        rows += list(csv.DictReader(fh))
rows.sort(key=lambda r: int(r["Dispatch_Id"]))
for r in rows:
    name = re.sub(r"\((?!anonymous namespace\)).*", "", r["Kernel_Name"])
    print(name, "grid", r["Grid_Size_X"], r["Grid_Size_Y"], r["Grid_Size_Z"], "block", r["Workgroup_Size_X"],
          r["Workgroup_Size_Y"], r["Workgroup_Size_Z"])
