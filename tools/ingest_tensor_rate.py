#!/usr/bin/env python3
"""k_ingest_tensor beside k_ingest_rgb<BGRA8> in one kernel trace: one 3840x2160
picture each of F16 CHW, U8 HWC3 and F32 CHW, and a BGRA8 picture of the same size, all resident on the
device, are ingested alternately through the unit seams (jmh_ingest_tensor, jmh_ingest_picture), 30
times each.  The seams copy the packed picture back, so the script's own wall clock says nothing about
the kernels: run it under the profiler and read the kernel statistics with --report.

  rocprofv3 --kernel-trace --stats -d <dir> -o tensor --output-format csv -- python tools/ingest_tensor_rate.py
  python tools/ingest_tensor_rate.py --report <dir>/.../tensor_kernel_stats.csv

BGRA8 is the yardstick: 33.2 MB in and 12.4 MB out per picture.  F16 CHW reads 49.8 MB, U8 HWC3 24.9 MB,
F32 CHW 99.5 MB; all write 12.4 MB.  Every source is 4 to 25 times smaller than the 256 MiB last-level
cache and is read again every fourth ingest: the sources are cache-warm, for all four kernels alike."""
import argparse
import csv
import importlib.util
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 3840, 2160
YUV_BYTES = W * H * 3 // 2
# the kernel's name in the trace -> (what to call it, bytes read, bytes written)
MOVED = {"k_ingest_rgb<16>": ("k_ingest_rgb<BGRA8>", 4 * W * H, YUV_BYTES),
         "k_ingest_tensor<2, true>": ("k_ingest_tensor<F16, PLANAR>", 6 * W * H, YUV_BYTES),
         "k_ingest_tensor<0, false>": ("k_ingest_tensor<U8, general> HWC3", 3 * W * H, YUV_BYTES),
         "k_ingest_tensor<4, true>": ("k_ingest_tensor<F32, PLANAR>", 12 * W * H, YUV_BYTES)}
YARDSTICK = "k_ingest_rgb<16>"


def report(path):
    rows = {}
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            for key in MOVED:
                if key.replace(" ", "") in r["Name"].replace(" ", ""):
                    rows[key] = r
    print(f"{'kernel':36s} {'calls':>5s} {'us/picture':>10s} {'min':>7s} {'max':>7s} {'MB in':>7s} {'MB out':>7s} {'GB/s in+out':>11s} {'of BGRA8':>8s}")
    rate = {k: sum(MOVED[k][1:]) / float(r["AverageNs"]) for k, r in rows.items()}
    for key, (name, rd, wr) in MOVED.items():
        if key not in rows:
            print(f"{name:36s} not in {path}")
            continue
        r = rows[key]
        avg = float(r["AverageNs"])
        rel = f"{rate[key] / rate[YARDSTICK]:8.2f}" if YARDSTICK in rate else f"{'-':>8s}"
        print(f"{name:36s} {int(r['Calls']):5d} {avg / 1e3:10.1f} {int(r['MinNs']) / 1e3:7.1f} {int(r['MaxNs']) / 1e3:7.1f} {rd / 1e6:7.1f} {wr / 1e6:7.1f} "
              f"{rate[key]:11.1f} {rel}")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--pictures", type=int, default=30, help="ingests of each source")
    ap.add_argument("--report", default=None, help="a kernel statistics CSV of the profiler: print the four kernels' rows as a table")
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
    q = rng.integers(0, 256, (3, H, W), dtype=np.uint8)                       # one picture, four ways
    words = q[2].astype(np.uint32) | q[1].astype(np.uint32) << 8 | q[0].astype(np.uint32) << 16 | 0xFF000000
    f32 = q.astype(np.float32) / np.float32(255)
    src = [enc.device_picture(jm.to_device_rgb(words, jm.JMH_PIX_BGRA8)),
           enc.device_tensor(jm.to_device_tensor(f32.astype(np.float16), "chw")),
           enc.device_tensor(jm.to_device_tensor(np.ascontiguousarray(q.transpose(1, 2, 0)), "hwc")),
           enc.device_tensor(jm.to_device_tensor(f32, "chw"))]
    try:
        for i in range(a.pictures):
            out = [enc.ingest(src[0])] + [enc.ingest_tensor(t) for t in src[1:]]
            if i == 0:      # the pictures arrived: U8 and F32 carry the bytes BGRA8 carries, so the three pictures are one
                for got in (out[2], out[3]):
                    assert all(np.array_equal(x, y) for x, y in zip(got, out[0]))
                assert abs(out[1][0].astype(np.int32) - out[0][0]).max() <= 1   # float16 rounds the components
        print(f"{a.pictures} ingests each of a {W}x{H} BGRA8 picture and F16 CHW, U8 HWC3 and F32 CHW tensors")
    finally:
        for s in src:
            enc.device_free(s.base)
        enc.close()


if __name__ == "__main__":
    main()
