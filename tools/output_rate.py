#!/usr/bin/env python3
"""The time of a pull: one picture is coded and popped at 1920x1080 and at 3840x2160,
then pulled again and again, deblocked, at the display size, each case back to back on a stream of the
caller's, the window ending in output_wait.  Cases: NV12, BGRA8, CHW U8 / F16 / F32, HWC3 F16.
Beside each stands a device-to-device copy of the same total bytes (the source samples read plus the
destination bytes written), timed by device events around the same number of copies (torch's copy_ of
a contiguous uint8 tensor on one device is a hipMemcpyAsync).  The kernels' own durations come from a
kernel-trace run of this script:

  python tools/output_rate.py                                                   # one JSON line per case
  rocprofv3 --kernel-trace --stats -d <dir> -o pull --output-format csv -- python tools/output_rate.py --no-copy
  python tools/output_rate.py --report <dir>/.../pull_kernel_stats.csv          # the k_pull_* lines of the trace

torch is imported first, so that the library binds to the HIP runtime torch brought."""
import argparse
import csv
import importlib.util
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = ((1920, 1080), (3840, 2160))
CASES = ("NV12", "BGRA8", "U8:chw", "F16:chw", "F32:chw", "F16:hwc3")


def load():
    spec = importlib.util.spec_from_file_location("jmhip", os.path.join(ROOT, "h264-jm-commentary_amd", "jmhip.py"))
    jm = importlib.util.module_from_spec(spec)
    sys.modules["jmhip"] = jm
    spec.loader.exec_module(jm)
    return jm


def layout_of(jm, case, w, h):
    """(layout, bytes written) of a case"""
    if case in ("NV12", "BGRA8"):
        L = jm.out_layout(jm.JMH_PIX_NV12 if case == "NV12" else jm.JMH_PIX_BGRA8, w, h)
        return L, w * h * 3 // 2 if case == "NV12" else 4 * w * h
    dt, lay = case.split(":")
    dtype = {"U8": jm.JMH_T_U8, "F16": jm.JMH_T_F16, "F32": jm.JMH_T_F32}[dt]
    L = jm.out_tensor_layout(dtype, w, h, "chw" if lay == "chw" else "hwc")
    return L, 3 * w * h * jm.TENSOR_ELEM_BYTES[dtype]


def report(path):
    with open(path) as f:
        rows = [r for r in csv.DictReader(f) if "k_pull" in r.get("Name", "")]
    for r in rows:
        print(f'{r["Name"]}: calls {r["Calls"]}, average {float(r["AverageNs"]) / 1e3:.1f} us, min {float(r["MinNs"]) / 1e3:.1f}, max {float(r["MaxNs"]) / 1e3:.1f}')


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--no-copy", action="store_true", help="leave the copies out (a kernel-trace run)")
    ap.add_argument("--report", default=None, help="print the k_pull_* lines of a kernel-stats CSV and exit")
    a = ap.parse_args()
    if a.report:
        return report(a.report)
    import torch
    if not torch.cuda.is_available():
        sys.exit("output_rate: no device")
    jm = load()
    for w, h in SIZES:
        W, H = (w + 15) // 16 * 16, (h + 15) // 16 * 16
        enc = jm.Encoder(W, H, search_range=16, search_mode=3)
        enc.push(*jm.synth_frame(w, h, 9, 0), jm.JMH_I_SLICE, 28, deblock=(0, 0, 0))
        enc.pop()
        stream = enc.device_stream()
        for case in CASES:
            L, written = layout_of(jm, case, w, h)
            total = w * h * 3 // 2 + written
            base = enc.device_alloc(L.nbytes)
            dst = L.at(base, stream)
            pull = enc.pull if case in ("NV12", "BGRA8") else enc.pull_tensor
            for _ in range(10):
                pull(dst)
            enc.output_wait()
            t0 = time.perf_counter()
            for _ in range(a.reps):
                pull(dst)
            enc.output_wait()
            us = 1e6 * (time.perf_counter() - t0) / a.reps
            enc.device_free(base)
            line = dict(case=case, size=f"{w}x{h}", bytes_read=w * h * 3 // 2, bytes_written=written, pull_us=round(us, 1),
                        pull_GBps=round(total / us / 1e3, 1))
            if not a.no_copy:
                src, out = torch.empty(total // 2, dtype=torch.uint8, device="cuda"), torch.empty(total // 2, dtype=torch.uint8, device="cuda")
                for _ in range(10):
                    out.copy_(src)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.reps):
                    out.copy_(src)
                e1.record()
                e1.synchronize()
                cus = 1e3 * e0.elapsed_time(e1) / a.reps
                line.update(copy_us=round(cus, 1), copy_GBps=round(total / cus / 1e3, 1), pull_over_copy=round(us / cus, 2))
                del src, out
            print(json.dumps(line), flush=True)
        enc.device_stream_destroy(stream)
        enc.close()


if __name__ == "__main__":
    main()
