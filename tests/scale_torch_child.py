"""The child process of tests/test_scale_gpu.py::test_torch_tensor_larger_than_the_coded_size (TEST
INFRASTRUCTURE, not collected).  torch is imported first, so that libjmhip.so, loaded afterwards, binds
to the HIP runtime torch brought (see tests/tensor_torch_child.py).

A float16 (3, 288, 352) tensor is made by torch ops on a non-default torch stream and, with no
synchronisation in between, taken through the seam and pushed as a coded picture into a 176x144 context
with a scale set.  Both must equal the reference computed from t.cpu(): tensor_ref at the source's size,
then scale_ref; the coded push against a coded push of that picture with the setting off.  Prints
"SKIP: ..." and exits 0 where torch sees no device."""
import os
import sys

import torch

if not torch.cuda.is_available():
    print("SKIP: torch sees no device")
    sys.exit(0)

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scale_ref as sr
import tensor_ref as tr
from jmpaths import ensure_built, load_jmhip

ensure_built()
jm = load_jmhip()
W, H, w, h, QP = 176, 144, 352, 288, 28
dev = torch.device("cuda", 0)
kw = dict(search_range=8, slice_mbs=33)
enc, ref = jm.Encoder(W, H, **kw), jm.Encoder(W, H, **kw)
enc.input_scale(W, H, jm.JMH_SCALE_BICUBIC)
side = torch.cuda.Stream(device=dev)
descs = jm.coded_slice_descs(enc.mbw * enc.mbh, jm.JMH_I_SLICE, QP, 33, lead=[(3, 0b101), (0, 0)])
with torch.cuda.stream(side):
    yy, xx = torch.meshgrid(torch.arange(h, device=dev, dtype=torch.float32), torch.arange(w, device=dev, dtype=torch.float32), indexing="ij")
    planes = [0.5 + 0.45 * torch.sin(xx / a) * torch.cos(yy / b) for a, b in ((5.0, 7.0), (6.0, 4.0), (9.0, 5.0))]
    t = torch.stack(planes).to(torch.float16)
    d = enc.from_torch(t)
    assert d.stream == side.cuda_stream and (d.width, d.height) == (w, h)
    seam = enc.ingest_tensor(d)
    enc.push_coded_tensor(d, jm.JMH_I_SLICE, QP, descs, deblock=(0, 0, 0))
got = enc.pop_coded()
host = t.cpu().numpy()
src = tr.convert_source_size(list(host), tr.F16, 0, 8)
want, peak = sr.scale_picture(src, W, H, W, H, sr.BICUBIC, False, 8, lambda *a: jm.scale_taps(*a))
assert all(np.array_equal(a, b) for a, b in zip(seam, want)), "seam"
ref.push_coded(*want, jm.JMH_I_SLICE, QP, descs, deblock=(0, 0, 0))
rgot = ref.pop_coded()
assert got[0] == rgot[0] and got[1] == rgot[1] and got[2] == rgot[2], "coded push"
enc.close()
ref.close()
print("scaled torch tensor: OK")
