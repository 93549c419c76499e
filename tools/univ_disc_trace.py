#!/usr/bin/env python3
"""Per-launch times of the spectral kernels (spec_kernel, conv2d_*) of the last pass in a rocprofv3 kernel-trace CSV.

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o univ -- python tools/univ_disc_bench.py --hip-only --iters 3
    python tools/univ_disc_trace.py DIR/.../univ_kernel_trace.csv [--passes 5]

``--passes`` is the number of discriminator passes the traced process made (univ_disc_bench.py: --iters + 2 warm-up rounds);
the spectral launches are split evenly among them and the last pass is printed in launch order with its microseconds (per
resolution: spectrogram, then one launch per conv layer).  Divide the layer FLOPs univ_disc_bench.py prints (times 2 * batch
rows) by them for TFLOP/s.
"""
import argparse
import csv


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("trace")
    ap.add_argument("--passes", type=int, default=5)
    a = ap.parse_args()
    rows = []
    with open(a.trace) as f:
        for r in csv.DictReader(f):
            name = r.get("Kernel_Name", "")
            if "spec_kernel" in name or "conv2d_" in name:
                rows.append((int(r["Start_Timestamp"]), (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3, name))
    rows.sort()
    if not rows or len(rows) % a.passes:
        raise SystemExit(f"{len(rows)} spectral launches do not divide into {a.passes} passes: give --passes")
    for _, us, name in rows[-(len(rows) // a.passes):]:
        print(f"{us:10.1f} us  {name[:110]}")


if __name__ == "__main__":
    main()
