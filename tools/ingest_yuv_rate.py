#!/usr/bin/env python3
"""k_ingest_yuv beside k_ingest<I420> and k_ingest_rgb<BGRA8> in one kernel trace:
1920x1080 pictures (coded 1920x1088), all resident on the device, are ingested in turn through the
unit seam (jmh_ingest_picture), a few dozen of each: UYVY, I444, VUYA8, I420 and BGRA8 in an 8-bit
context, Y410 in a 10-bit one.  The seam copies the packed picture back, so the script's own wall
clock says nothing about the kernels: run it under the profiler and read the kernel statistics with
--report.

  rocprofv3 --kernel-trace --stats -d <dir> -o yuv --output-format csv -- python tools/ingest_yuv_rate.py
  python tools/ingest_yuv_rate.py --report <dir>/.../yuv_kernel_stats.csv

I420 is the yardstick: it moves 3.1 MB in and 3.1 MB out per picture."""
import argparse
import csv
import importlib.util
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, CH = 1920, 1080, 1088
OUT8 = W * CH * 3 // 2
# substring of the kernel's name -> (label, bytes read, bytes written)
MOVED = {"k_ingest<0>": ("k_ingest<I420>", W * H * 3 // 2, OUT8),
         "k_ingest_rgb<16>": ("k_ingest_rgb<BGRA8>", 4 * W * H, OUT8),
         "k_ingest_yuv<35,": ("k_ingest_yuv<UYVY>", 2 * W * H, OUT8),
         "k_ingest_yuv<36,": ("k_ingest_yuv<I444>", 3 * W * H, OUT8),
         "k_ingest_yuv<37,": ("k_ingest_yuv<VUYA8>", 4 * W * H, OUT8),
         "k_ingest_yuv<44,": ("k_ingest_yuv<Y410>", 4 * W * H, 2 * OUT8)}


def report(path):
    rows = {}
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            for key in MOVED:
                if key in r["Name"].replace(" ", "").replace("(int)", "") + ",":
                    rows[key] = r
    base = float(rows["k_ingest<0>"]["AverageNs"]) if "k_ingest<0>" in rows else None
    print(f"{'kernel':22s} {'calls':>5s} {'us/picture':>10s} {'min':>7s} {'max':>7s} {'MB in':>7s} {'MB out':>7s} {'GB/s in+out':>11s} {'time / I420':>11s} {'bytes in / I420':>15s}")
    for key, (name, rd, wr) in MOVED.items():
        if key not in rows:
            print(f"{name:22s} not in {path}")
            continue
        r = rows[key]
        avg = float(r["AverageNs"])
        rel = f"{avg / base:11.2f}" if base else f"{'-':>11s}"
        print(f"{name:22s} {int(r['Calls']):5d} {avg / 1e3:10.1f} {int(r['MinNs']) / 1e3:7.1f} {int(r['MaxNs']) / 1e3:7.1f} {rd / 1e6:7.2f} {wr / 1e6:7.2f} "
              f"{(rd + wr) / avg:11.1f} {rel} {rd / MOVED['k_ingest<0>'][1]:15.2f}")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--pictures", type=int, default=30, help="ingests of each format")
    ap.add_argument("--report", default=None, help="a kernel statistics CSV of the profiler: print the kernels' rows as a table")
    a = ap.parse_args()
    if a.report:
        return report(a.report)
    import numpy as np
    spec = importlib.util.spec_from_file_location("jmhip", os.path.join(ROOT, "h264-jm-commentary_amd", "jmhip.py"))
    jm = importlib.util.module_from_spec(spec)
    sys.modules["jmhip"] = jm
    spec.loader.exec_module(jm)
    rng = np.random.default_rng(1)
    plane = lambda w, h, bd=8: rng.integers(0, 1 << bd, (h, w), dtype=np.int64).astype(np.uint16 if bd > 8 else np.uint8)
    enc, enc10 = jm.Encoder(W, CH, search_range=8, pipeline_depth=2), jm.Encoder(W, CH, search_range=8, pipeline_depth=2, bit_depth=10)
    p420 = (plane(W, H), plane(W // 2, H // 2), plane(W // 2, H // 2))
    p422 = (plane(W, H), plane(W // 2, H), plane(W // 2, H))
    p444 = (plane(W, H), plane(W, H), plane(W, H))
    p444w = (plane(W, H, 10), plane(W, H, 10), plane(W, H, 10))
    words = rng.integers(0, 1 << 32, (H, W), dtype=np.uint64).astype(np.uint32)
    pics = [(enc, enc.device_picture(jm.to_device(p420, jm.JMH_PIX_I420)), p420, jm.JMH_PIX_I420, 8),
            (enc, enc.device_picture(jm.to_device_rgb(words, jm.JMH_PIX_BGRA8)), None, None, 8),
            (enc, enc.device_picture(jm.to_device_yuv(p422, jm.JMH_PIX_UYVY)), p422, jm.JMH_PIX_UYVY, 8),
            (enc, enc.device_picture(jm.to_device_yuv(p444, jm.JMH_PIX_I444)), p444, jm.JMH_PIX_I444, 8),
            (enc, enc.device_picture(jm.to_device_yuv(p444, jm.JMH_PIX_VUYA8)), p444, jm.JMH_PIX_VUYA8, 8),
            (enc10, enc10.device_picture(jm.to_device_yuv(p444w, jm.JMH_PIX_Y410)), p444w, jm.JMH_PIX_Y410, 10)]
    try:
        for i in range(a.pictures):
            for e, pic, src, fmt, bd in pics:
                got = e.ingest(pic)
                if i == 0 and src is not None:      # the pictures arrived
                    want = jm.pad_to_coded(src if fmt == jm.JMH_PIX_I420 else jm.yuv_reduce(*src, fmt, bd), W, CH)
                    assert all(np.array_equal(g, w) for g, w in zip(got, want)), fmt
        print(f"{a.pictures} ingests each of {len(pics)} {W}x{H} pictures")
    finally:
        for e, pic, *_ in pics:
            e.device_free(pic.base)
        enc.close()
        enc10.close()


if __name__ == "__main__":
    main()
