"""The child process of tests/test_output_gpu.py::test_torch_tensors_through_to_torch_and_into_torch
(TEST INFRASTRUCTURE, not collected).  torch is imported first, so that libjmhip.so, loaded afterwards,
binds to the HIP runtime torch brought: one runtime, whose stream handles both sides understand.

An I picture is pushed and popped.  enc.to_torch(torch.float16, "chw") on a non-default torch stream,
consumed by torch on that stream with no synchronisation in between, and enc.into_torch of a strided
(h, w, 3) view of an (h + 4, w + 6, 4) uint8 tensor equal tests/output_ref.py applied to
enc.deblocked(); the rest of that tensor keeps its canary.  The float16 tensor pushed again through
enc.from_torch gives, through ingest_tensor, the planes tensor_ref.convert gives for the reference
tensor.  Prints "SKIP: ..." and exits 0 where torch sees no device."""
import os
import sys

import torch

if not torch.cuda.is_available():
    print("SKIP: torch sees no device")
    sys.exit(0)

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import output_ref as oref
import tensor_ref as tr
from jmpaths import ensure_built, load_jmhip
from test_ingest_gpu import seq

ensure_built()
jm = load_jmhip()
W, H, w, h, QP = 64, 48, 50, 34, 28
dev = torch.device("cuda", 0)
enc = jm.Encoder(W, H, search_range=8)
enc.push(*seq(W, H, 1, 41)[0], jm.JMH_I_SLICE, QP, deblock=(0, 0, 0))
enc.pop()
dbk, rec = enc.deblocked(), enc.recon()
side = torch.cuda.Stream(device=dev)
assert side.cuda_stream != 0
with torch.cuda.stream(side):
    t = enc.to_torch(torch.float16, "chw", flags=jm.JMH_PIX_BT709, size=(w, h))
    doubled = t.float() * 2                                        # torch work behind the pull, on the same stream
    full = enc.to_torch(torch.float32, "hwc", which=jm.JMH_OUT_RECON)
assert tuple(t.shape) == (3, h, w) and t.dtype == torch.float16 and tuple(full.shape) == (H, W, 3)
want = oref.tensor(dbk, w, h, oref.F16, oref.BT709, 8)
host = t.cpu().numpy()
assert host.dtype == np.float16 and all(np.array_equal(host[c].view(np.uint16), want[c].view(np.uint16)) for c in range(3)), "to_torch"
assert np.array_equal(doubled.cpu().numpy(), np.stack(want).astype(np.float32) * 2), "torch work queued behind the pull"
wf = oref.tensor(rec, W, H, oref.F32, 0, 8)
assert np.array_equal(full.cpu().numpy(), np.stack(wf, axis=-1)), "to_torch hwc float32 of the reconstruction"
# a strided BGR view of a larger uint8 tensor with four channels, on the null stream
u = torch.full((h + 4, w + 6, 4), 0xA5, dtype=torch.uint8, device=dev)
view = u[2:2 + h, 4:4 + w, :3]
assert not view.is_contiguous()
assert enc.into_torch(view, order="bgr", flags=jm.JMH_PIX_FULL_RANGE) is view
hu = u.cpu().numpy()
r, g, b = oref.tensor(dbk, w, h, oref.U8, oref.FULL_RANGE, 8)
assert np.array_equal(hu[2:2 + h, 4:4 + w, :3], np.stack([b, g, r], axis=-1)), "into_torch of a strided view"
mask = np.ones(hu.shape, bool)
mask[2:2 + h, 4:4 + w, :3] = False
assert (hu[mask] == 0xA5).all(), "into_torch wrote outside its view"
# and round: the pulled tensor pushed again
with torch.cuda.stream(side):
    planes = enc.ingest_tensor(enc.from_torch(t, flags=jm.JMH_PIX_BT709))
assert all(np.array_equal(a, b) for a, b in zip(planes, tr.convert(want, tr.F16, tr.BT709, 8, W, H))), "the pulled tensor through ingest_tensor"
enc.close()
print("torch output: OK")
