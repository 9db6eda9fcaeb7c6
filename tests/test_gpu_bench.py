"""GPU: bench.py's plain run end to end at a small size -- the result line's
contract keys, --steps as the number of timed steps, and --dump-outputs against
the same step run in this process (the assembly is bitwise reproducible)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

pytestmark = pytest.mark.gpu


def test_plain_run_line_and_dump(ctx, tmp_path):
    import arcanefem_amd as af

    n, out = 12, tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--n", str(n), "--settle-ms", "0", "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["metric"] == bench.METRIC and line["unit"] == "MDoF/s" and line["dtype"] == "f64"
    assert line["higher_is_better"] is True and line["full"] is False
    assert (line["steps"], line["warmup"], line["n_gpus"]) == (3, 1, 1)
    n_dof = (n + 1) ** 3
    assert line["config"]["dof_total"] == n_dof
    assert line["ms_per_step"] > 0
    # value = DoF per second of the same steps; ms_per_step is printed to 1e-4 ms
    assert line["value"] == pytest.approx(n_dof / (line["ms_per_step"] * 1e-3) / 1e6,
                                          rel=1e-3 + 1e-4 / line["ms_per_step"])
    assert "cg_iter_per_s" not in line and "legs" not in line and "cpu_baseline" not in line

    mesh, bsr, ls, bottom, dbottom, _ = bench.poisson_setup(ctx, af, n, n, 1, 0)
    bench.make_step(ctx, bsr, ls, bottom, dbottom)()
    ctx.synchronize()
    vals, rhs = bsr.download()[2], ls.rhs_host()
    ctx.free(dbottom)
    ls.reset()
    bsr.close()
    mesh.close()
    assert sorted(os.listdir(out)) == ["csr_values.npy", "rhs.npy"]
    dv, dr = np.load(out / "csr_values.npy"), np.load(out / "rhs.npy")
    assert dv.dtype == np.float64 and dr.dtype == np.float64
    assert np.array_equal(dv, vals) and np.array_equal(dr, rhs)
    assert np.abs(dv).max() == 1.0e30 and dr.size == n_dof  # the penalty rows are in
