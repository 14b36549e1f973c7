#!/usr/bin/env python3
"""The rate of coded pictures once the pipeline is kept full (DESIGN.md §5.4 "What these runs cannot
show", §5.6): a handful of source pictures resident on the device are pushed round-robin through
push_coded_device / pop_coded, so no picture waits for a source.  Reports ms per picture (wall
clock over the timed pictures, ending in the last pop) and the host time spent inside the push and
pop calls.  --source host pushes the same pictures from host memory (push_coded): the comparison
for the push's host time; JMH_LIB_PATH selects another build of the library for it.  --nal arms every
picture with one head per slice (jmh_coded_nal_heads): its pop returns the finished access unit.
--pull <dtype>:<layout> pulls every popped picture, deblocked, at the display size into one device
tensor on a stream of the caller's (jmh_pull_tensor; dtype u8, u16, f16, bf16 or f32,
layout chw, hwc3 or hwc4) and reports the host time inside the pull; the window ends with output_wait.

  python tools/coded_rate.py --config 5 --split 1024     # 2160p High 10 EPZS, RDO, CABAC, 240-MB slices
  python tools/coded_rate.py --config 2                  # 1080p Baseline FFS, CAVLC
  python tools/coded_rate.py --config 5 --split 1024 --nal   # the same, NAL units finished on the device
  python tools/coded_rate.py --config 2 --pull f16:chw   # 1080p, every picture pulled as a float16 CHW tensor
One JSON line on stdout."""
import argparse
import importlib.util
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("jmhip", os.path.join(ROOT, "h264-jm-commentary_amd", "jmhip.py"))
jm = importlib.util.module_from_spec(spec)
sys.modules["jmhip"] = jm
spec.loader.exec_module(jm)

CONFIGS = {   # bench.py's shapes; the coder is the one a lencod run of the config uses
    2: dict(disp=(1920, 1080), kw=dict(search_range=32, search_mode=0)),
    5: dict(disp=(3840, 2160), kw=dict(search_range=32, search_mode=3, bit_depth=10, rdo=1, slice_mbs=240)),
}
QP = 28


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", type=int, choices=sorted(CONFIGS), default=2)
    ap.add_argument("--size", default=None, help="WxH display size instead of the config's")
    ap.add_argument("--split", type=int, default=0, help="CABAC configs: DeviceCABACSplit chunk bins (0: one wave per slice)")
    ap.add_argument("--pictures", type=int, default=4, help="resident source pictures")
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=12)
    ap.add_argument("--source", choices=("device", "host"), default="device")
    ap.add_argument("--format", choices=("planar", "semi"), default="planar", help="device source: I420 / I010, or NV12 / P010 (10 bits only)")
    ap.add_argument("--nal", action="store_true", help="arm every picture with its slices' heads: the pop returns the access unit")
    ap.add_argument("--pull", default=None, metavar="DTYPE:LAYOUT", help="pull every popped picture as an RGB tensor, e.g. f16:chw")
    a = ap.parse_args()
    c = CONFIGS[a.config]
    dw, dh = (int(v) for v in a.size.split("x")) if a.size else c["disp"]
    W, H = (dw + 15) // 16 * 16, (dh + 15) // 16 * 16
    kw = c["kw"]
    bd = kw.get("bit_depth", 8)
    if a.source == "host" and os.environ.get("JMH_LIB_PATH"):
        jm._SIGS_INPUT.clear()                   # an older build of the library has no device-picture entry points to bind
    if not a.nal and os.environ.get("JMH_LIB_PATH"):
        jm._SIGS_NAL.clear()                     # nor the NAL ones
    enc = jm.Encoder(W, H, **kw)
    if a.split:
        enc.cabac_split(a.split)
    frames = [jm.synth_frame(dw, dh, 9, i, bit_depth=bd) for i in range(a.pictures)]          # coded size, padded on the host
    fmt = {(8, "planar"): jm.JMH_PIX_I420, (8, "semi"): jm.JMH_PIX_NV12, (10, "planar"): jm.JMH_PIX_I010, (10, "semi"): jm.JMH_PIX_P010}[(bd, a.format)]
    dev = []
    if a.source == "device":
        dev = [enc.device_picture(jm.to_device(tuple(p[:h, :w] for p, (w, h) in zip(f, ((dw, dh), (dw // 2, dh // 2), (dw // 2, dh // 2)))), fmt))
               for f in frames]
    nmb = enc.mbw * enc.mbh
    descs = {st: jm.coded_slice_descs(nmb, st, QP, kw.get("slice_mbs", 0)) for st in (jm.JMH_I_SLICE, jm.JMH_P_SLICE)}
    # a slice header's worth of head per slice: 6 bytes, the last ones zero so that runs cross the junction
    heads = {st: jm.nal_heads([(2 if st == jm.JMH_P_SLICE else 3, 1 if st == jm.JMH_P_SLICE else 5, bytes([0x88, 0x84, k & 0xFF, 0x21, 0, 0]))
                               for k in range(len(descs[st]))]) if a.nal else None for st in descs}
    pull = None
    if a.pull:
        dt, lay = a.pull.split(":")
        dtype = {"u8": jm.JMH_T_U8, "u16": jm.JMH_T_U16, "f16": jm.JMH_T_F16, "bf16": jm.JMH_T_BF16, "f32": jm.JMH_T_F32}[dt]
        L = jm.out_tensor_layout(dtype, dw, dh, "chw" if lay == "chw" else "hwc", channels=4 if lay == "hwc4" else 3)
        stream = enc.device_stream()
        pull = L.at(enc.device_alloc(L.nbytes), stream)
    pending = n = nbytes = fallbacks = 0
    push_s = pop_s = pull_s = 0.0

    def pulled():
        if not pull:
            return 0.0
        t = time.perf_counter()
        enc.pull_tensor(pull)
        return time.perf_counter() - t
    t0 = None
    total = a.warmup + a.steps
    for i in range(total):
        if i == a.warmup:
            while pending:                       # the timed window starts with an empty pipeline and ends with one
                enc.pop_coded()
                pending -= 1
            push_s = pop_s = pull_s = 0.0
            n = nbytes = fallbacks = 0
            t0 = time.perf_counter()
        if i:
            enc.set_reference_slot(-2)
        if pending == enc.depth:
            t = time.perf_counter()
            data, _, stats = enc.pop_coded()
            pop_s += time.perf_counter() - t
            pull_s += pulled()
            pending -= 1
            n += 1
            nbytes += sum(len(d) for d in data)
            fallbacks += stats["fallback"]
        st = jm.JMH_I_SLICE if i == 0 else jm.JMH_P_SLICE
        t = time.perf_counter()
        if dev:
            enc.push_coded_device(dev[i % len(dev)], st, QP, descs[st], crop=(dw, dh), deblock=(0, 0, 0), heads=heads[st])
        else:
            enc.push_coded(*frames[i % len(frames)], st, QP, descs[st], crop=(dw, dh), deblock=(0, 0, 0), heads=heads[st])
        push_s += time.perf_counter() - t
        pending += 1
    while pending:
        t = time.perf_counter()
        data, _, stats = enc.pop_coded()
        pop_s += time.perf_counter() - t
        pull_s += pulled()
        pending -= 1
        n += 1
        nbytes += sum(len(d) for d in data)
        fallbacks += stats["fallback"]
    if pull:
        enc.output_wait()
    dt = time.perf_counter() - t0
    for d in dev:
        enc.device_free(d.base)
    if pull:
        enc.device_stream_destroy(pull.stream)
        enc.device_free(pull.chans[0] - L.offsets[0])
    depth = enc.depth
    enc.close()
    print(json.dumps(dict(config=a.config, size=f"{dw}x{dh}", coded=f"{W}x{H}", source=a.source, format=jm_name(fmt) if dev else "host planes",
                          coder="CABAC" if kw.get("rdo") else "CAVLC", cabac_split=a.split, nal=int(a.nal), depth=depth, pictures=n,
                          ms_per_picture=round(1e3 * dt / n, 4), push_host_ms=round(1e3 * push_s / a.steps, 4),
                          pop_host_ms=round(1e3 * pop_s / n, 4), pull=a.pull or "", pull_host_ms=round(1e3 * pull_s / n, 4), bytes_per_picture=nbytes // n, fallbacks=fallbacks,
                          lib=os.path.basename(os.path.dirname(jm.LIB_PATH)) + "/" + os.path.basename(jm.LIB_PATH))))


def jm_name(fmt):
    return {jm.JMH_PIX_I420: "I420", jm.JMH_PIX_NV12: "NV12", jm.JMH_PIX_I010: "I010", jm.JMH_PIX_P010: "P010"}[fmt]


if __name__ == "__main__":
    main()
