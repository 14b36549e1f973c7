#!/usr/bin/env python3
"""k_ingest_rgb<BGRA8> beside k_ingest<NV12> in one kernel trace: a 3840x2160 BGRA8
picture and a 3840x2160 NV12 picture, both resident on the device, are ingested alternately through
the unit seam (jmh_ingest_picture), a few dozen of each.  The seam copies the packed picture back, so
the script's own wall clock says nothing about the kernels: run it under the profiler and read the
kernel statistics with --report.

  rocprofv3 --kernel-trace --stats -d <dir> -o rgb --output-format csv -- python tools/ingest_rgb_rate.py
  python tools/ingest_rgb_rate.py --report <dir>/.../rgb_kernel_stats.csv

NV12 is the yardstick: it moves 12.4 MB in and 12.4 MB out per picture, BGRA8 33.2 MB in and 12.4 MB out."""
import argparse
import csv
import importlib.util
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 3840, 2160
YUV_BYTES = W * H * 3 // 2
MOVED = {"k_ingest_rgb<16>": ("k_ingest_rgb<BGRA8>", 4 * W * H, YUV_BYTES), "k_ingest<1>": ("k_ingest<NV12>", YUV_BYTES, YUV_BYTES)}


def report(path):
    rows = {}
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            for key in MOVED:
                if key in r["Name"]:
                    rows[key] = r
    print(f"{'kernel':22s} {'calls':>5s} {'us/picture':>10s} {'min':>7s} {'max':>7s} {'MB in':>7s} {'MB out':>7s} {'GB/s in+out':>11s}")
    for key, (name, rd, wr) in MOVED.items():
        if key not in rows:
            print(f"{name:22s} not in {path}")
            continue
        r = rows[key]
        avg = float(r["AverageNs"])
        print(f"{name:22s} {int(r['Calls']):5d} {avg / 1e3:10.1f} {int(r['MinNs']) / 1e3:7.1f} {int(r['MaxNs']) / 1e3:7.1f} {rd / 1e6:7.1f} {wr / 1e6:7.1f} "
              f"{(rd + wr) / avg:11.1f}")
    if len(rows) == 2:
        a, b = (sum(MOVED[k][1:]) / float(rows[k]["AverageNs"]) for k in MOVED)
        print(f"k_ingest_rgb<BGRA8> moves {a / b:.2f} of k_ingest<NV12>'s bytes per second")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--pictures", type=int, default=30, help="ingests of each format")
    ap.add_argument("--report", default=None, help="a kernel statistics CSV of the profiler: print the two kernels' rows as a table")
    a = ap.parse_args()
    if a.report:
        return report(a.report)
    import numpy as np
    spec = importlib.util.spec_from_file_location("jmhip", os.path.join(ROOT, "h264-jm-commentary_amd", "jmhip.py"))
    jm = importlib.util.module_from_spec(spec)
    sys.modules["jmhip"] = jm
    spec.loader.exec_module(jm)
    rng = np.random.default_rng(1)
    enc = jm.Encoder(W, H, search_range=8, pipeline_depth=2)
    words = rng.integers(0, 1 << 32, (H, W), dtype=np.uint64).astype(np.uint32)
    yuv = (rng.integers(0, 256, (H, W), dtype=np.uint8), rng.integers(0, 256, (H // 2, W // 2), dtype=np.uint8),
           rng.integers(0, 256, (H // 2, W // 2), dtype=np.uint8))
    rgb = enc.device_picture(jm.to_device_rgb(words, jm.JMH_PIX_BGRA8))
    nv12 = enc.device_picture(jm.to_device(yuv, jm.JMH_PIX_NV12))
    try:
        for i in range(a.pictures):
            y, u, v = enc.ingest(rgb)
            y2, u2, v2 = enc.ingest(nv12)
            if i == 0:      # the pictures arrived: NV12 is a copy, BGRA8 grey-ish noise inside the limited range
                assert np.array_equal(y2, yuv[0]) and np.array_equal(u2, yuv[1]) and np.array_equal(v2, yuv[2])
                assert 16 <= int(y.min()) and int(y.max()) <= 235 and 16 <= int(u.min()) and int(v.max()) <= 240
        print(f"{a.pictures} ingests each of a {W}x{H} BGRA8 and NV12 picture")
    finally:
        enc.device_free(rgb.base)
        enc.device_free(nv12.base)
        enc.close()


if __name__ == "__main__":
    main()
