"""bench.py's plain run and --dump-outputs on the device: a plain run (no --full) reports the
headline fields and leaves the --full legs out; the dumped arrays are those of the chain's next
picture, encoded against the last timed step's deblocked picture, and must equal the same chain
encoded one picture at a time (pipeline depth 1) in this process, value for value.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from jmpaths import ROOT, ensure_built, load_jmhip

jmhip = load_jmhip()
W, H, SR, QP = 352, 288, 32, 28


@pytest.mark.gpu
def test_plain_run_dumps_the_chain_outputs(tmp_path):
    ensure_built()
    nframes, steps = 3, 4
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "2",
           "--frames", str(nframes), "--size", f"{W}x{H}", "--dump-outputs", str(tmp_path / "out")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["full"] is False and line["cpu_baseline"] is None and line["verified"] is None and line["host_path"] is None
    assert line["steps"] == steps and line["timed_region"]["pictures_completed"] == [steps] and line["complete"]
    assert line["value"] > 0 and line["unit"] == "MP/s" and line["higher_is_better"] is True and line["dtype"] == "u8"
    assert abs(line["ms_per_step"] - W * H / 1e3 / line["value"]) <= 0.002 + 1e-3 * line["ms_per_step"]   # both rounded to 3 places

    frames = [jmhip.synth_frame(W, H, 0, i) for i in range(nframes + 1)]
    g = jmhip.Encoder(W, H, search_range=SR, pipeline_depth=1)
    dbk = (0, 0, 0)
    g.encode(*frames[0], jmhip.JMH_I_SLICE, QP, deblock=dbk)
    for i in range(line["timed_region"]["warmup_steps_run"] + steps + 1):   # the chain, then the dumped picture
        g.set_reference_slot(-2)
        res, rec = g.encode(*frames[1 + i % nframes], jmhip.JMH_P_SLICE, QP, deblock=dbk)
    want = dict(zip(("rec_y", "rec_u", "rec_v", "dbk_y", "dbk_u", "dbk_v"), rec + g.deblocked()))
    g.close()
    for name in res.dtype.names:
        if name not in ("pad0", "reserved"):
            want["res_" + name] = res[name].reshape(len(res), -1)
    got = {f[:-4]: np.load(tmp_path / "out" / f) for f in os.listdir(tmp_path / "out")}
    assert set(got) == set(want)
    assert (want["res_mb_type"] != 0).any() and want["res_luma"].any()
    for name, a in got.items():
        assert a.dtype in (np.float32, np.float64) and a.shape == want[name].shape, name
        assert np.array_equal(a, want[name]), name
