"""bench.py as a program (gpu): a plain run measures the headline alone and
--dump-outputs writes what the timed path computed in its last step."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_plain_run_dumps_the_timed_result(gpu, orc, tmp_path):
    """One plain N = 1 run on 40 MiB buckets (10 Mi lanes: above DUMP_MAX_ELEMS
    and no multiple of it, so out.npy is the seeded lane sample): the line has
    the headline keys, `steps` timed steps and none of the --full keys, and
    out.npy is, bit for bit, the oracle's result on the bench's inputs (torch's
    generator on the device, seed 1000, as bench.py draws them) at dump_lanes."""
    import torch
    sys.path.insert(0, ROOT)
    import bench
    mib, R, k = 40, 2, 25
    out_dir = tmp_path / "dump"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--bucket-mib", str(mib), "--settle-seconds", "0", "--dump-outputs", str(out_dir)],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = p.stdout.strip().splitlines()
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["metric"] == bench.METRIC and line["unit"] == "GB/s" and line["higher_is_better"] is True
    assert line["dtype"] == "int32" and line["steps"] == 3 and line["full"] is False and "error" not in line
    n = mib * (1 << 20) // 4
    assert line["ms_per_step"] > 0
    # both figures are rounded in the line: ms_per_step to 1e-4 ms of some 0.03 ms
    assert line["value"] == pytest.approx(R * n * 4 / (line["ms_per_step"] * 1e-3) / 1e9, rel=1e-2)
    for key in ("roofline", "roofline_cold", "cpu_baseline", "parity_vs_oracle", "sizes", "host_e2e", "bf16"):
        assert key not in line
    assert sorted(os.listdir(out_dir)) == ["out.npy"]
    got = np.load(out_dir / "out.npy")
    lanes = bench.dump_lanes(n)
    assert got.dtype == np.float32 and got.shape == (bench.DUMP_MAX_ELEMS,) and got.nbytes <= 64_000_000
    gen = torch.Generator(device=gpu)
    gen.manual_seed(1000)
    xs = [torch.randn(n, generator=gen, device=gpu, dtype=torch.float32).cpu().numpy() for _ in range(R)]
    want = orc.reduce_f32(xs, k)[lanes]
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
