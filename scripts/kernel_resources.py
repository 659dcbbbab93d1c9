#!/usr/bin/env python3
"""The compiler's resource-usage report of the front end's kernels as a table: registers, scratch, LDS and occupancy of every kernel of
csrc/gf_tracker.hip, gf_cvt.hip and gf_clahe.hip, compiled for gfx950 with the flags of build.py.  Needs no GPU.

    python scripts/kernel_resources.py [--root TREE] [--out FILE.csv]

--root: another checkout of this repository (the parent commit, to compare with).  The table is sorted by kernel name, so two of them diff line by line."""
import argparse
import csv
import os
import re
import subprocess
import sys

UNITS = ("gf_tracker.hip", "gf_cvt.hip", "gf_clahe.hip")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c", "-o", os.devnull]
FIELDS = (("VGPRs", "vgprs"), ("AGPRs", "agprs"), ("SGPRs", "sgprs"), ("ScratchSize [bytes/lane]", "scratch_bytes"), ("Occupancy [waves/SIMD]", "waves_per_simd"),
          ("LDS Size [bytes/block]", "lds_bytes"))


def report(root):
    rows = {}
    for unit in UNITS:
        src = os.path.join(root, "ground-fusion_amd", "csrc", unit)
        err = subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + FLAGS + [src], stderr=subprocess.PIPE, text=True, check=True).stderr
        cur = None
        for line in err.splitlines():
            m = re.search(r"remark: .*?Function Name: (\S+)", line)
            if m:
                name = subprocess.check_output(["c++filt", m.group(1)], text=True).strip()
                cur = rows.setdefault(re.sub(r"\(.*", "", name).replace("void ", ""), {"unit": unit})
                continue
            for label, key in FIELDS:
                m = re.search(r"remark: .*?%s: (\d+)" % re.escape(label), line)
                if m and cur is not None:
                    cur[key] = int(m.group(1))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--out", default="-")
    a = ap.parse_args()
    rows = report(a.root)
    out = sys.stdout if a.out == "-" else open(a.out, "w", newline="")
    w = csv.writer(out, lineterminator="\n")
    w.writerow(["kernel", "unit"] + [k for _, k in FIELDS])
    for name in sorted(rows):
        w.writerow([name, rows[name]["unit"]] + [rows[name].get(k, "") for _, k in FIELDS])


if __name__ == "__main__":
    main()
