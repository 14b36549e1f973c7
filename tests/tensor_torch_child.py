"""The child process of tests/test_tensor_gpu.py::test_torch_tensor_through_from_torch (TEST
INFRASTRUCTURE, not collected).  torch is imported first, so that libjmhip.so, loaded afterwards, binds
to the HIP runtime torch brought: one runtime, whose stream handles both sides understand
(jmhip.Encoder.from_torch refuses to go on otherwise).

A float16 (3, H, W) tensor is made by torch ops on a non-default torch stream and pushed, with no
synchronisation in between, as it is and as its .permute(1, 2, 0) view.  The seam and the pipeline
results must equal the reference computed from t.cpu().  Prints "SKIP: ..." and exits 0 where torch
sees no device."""
import os
import sys

import torch

if not torch.cuda.is_available():
    print("SKIP: torch sees no device")
    sys.exit(0)

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tensor_ref as tr
from jmpaths import ensure_built, load_jmhip

ensure_built()
jm = load_jmhip()
W, H, w, h, QP = 64, 48, 50, 34, 28
dev = torch.device("cuda", 0)
enc, ref = jm.Encoder(W, H, search_range=8), jm.Encoder(W, H, search_range=8)
side = torch.cuda.Stream(device=dev)
assert side.cuda_stream != 0
with torch.cuda.stream(side):
    yy, xx = torch.meshgrid(torch.arange(h, device=dev, dtype=torch.float32), torch.arange(w, device=dev, dtype=torch.float32), indexing="ij")
    planes = [0.5 + 0.6 * torch.sin(xx / a) * torch.cos(yy / b) for a, b in ((5.0, 7.0), (6.0, 4.0), (9.0, 5.0))]
    t = torch.stack(planes).to(torch.float16)
    t[0, 0, 0], t[1, 0, 0], t[2, 0, 1] = float("nan"), 0.5, float("inf")
    views = [t, t.permute(1, 2, 0)]
    assert tuple(views[1].shape) == (h, w, 3) and not views[1].is_contiguous()
    descs = [enc.from_torch(v) for v in views]                     # layout inferred, the stream torch is queueing on
    assert all(d.stream == side.cuda_stream for d in descs)
    assert (descs[0].stride_x, descs[0].stride_y) == (2, 2 * w) and descs[0].chans == [t.data_ptr() + i * 2 * w * h for i in range(3)]
    assert (descs[1].stride_x, descs[1].stride_y) == (2, 2 * w) and descs[1].chans == descs[0].chans      # a view: the same elements
    seams = [enc.ingest_tensor(d) for d in descs]
    for i, d in enumerate(descs):
        enc.push_tensor(d, jm.JMH_I_SLICE, QP)
got = [enc.pop() for _ in descs]
host = t.cpu().numpy()
assert tr.holds_condition(list(host), tr.F16)
want = tr.convert(list(host), tr.F16, 0, 8, W, H)
for s in seams:
    assert all(np.array_equal(a, b) for a, b in zip(s, want)), "seam"
ref.push(*want, jm.JMH_I_SLICE, QP)
rres, rrec = ref.pop()
for res, rec in got:
    assert res.tobytes() == rres.tobytes() and all(np.array_equal(a, b) for a, b in zip(rec, rrec)), "pipeline"
# a BGR HWC uint8 tensor with 4 channels, cropped: strides from stride(), addresses permuted
u = (torch.rand((h + 4, w + 6, 4), device=dev) * 255).to(torch.uint8)
crop = u[2:2 + h, 4:4 + w]
d = enc.from_torch(crop, order="bgr", flags=jm.JMH_PIX_FULL_RANGE)
assert d.stream is None and (d.stride_x, d.stride_y) == (4, 4 * (w + 6))
hc = crop.cpu().numpy()
want = tr.convert([hc[:, :, 2], hc[:, :, 1], hc[:, :, 0]], tr.U8, tr.FULL_RANGE, 8, W, H)
assert all(np.array_equal(a, b) for a, b in zip(enc.ingest_tensor(d), want)), "cropped BGR view"
enc.close()
ref.close()
print("torch tensor: OK")
