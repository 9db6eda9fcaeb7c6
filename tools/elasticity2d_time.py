"""Kernel time of the block-2 triangle elasticity assembly on a 2D box of
(n + 1)^2 nodes: the plain entry (afem_bsr_assemble_elasticity_p1) and the
fused form with mass and body force (afem_bsr_assemble_elasticity_p1_ex),
each the median of --reps HIP-event-timed launches after the bench's settle,
with the algorithmic bytes of DESIGN.md section 3.1b-2.  One JSON line.
usage: python tools/elasticity2d_time.py [--n 2048] [--reps 10] [--settle 150] [--plain-only]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import arcanefem_amd as af  # noqa: E402
import bench  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=2048)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--settle", type=float, default=150.0)
ap.add_argument("--plain-only", action="store_true", help="only the plain entry (a tree without the fused form)")
a = ap.parse_args()
E, nu = 21.0e5, 0.28
lam, mu2 = E * nu / ((1 + nu) * (1 - 2 * nu)), E / (1 + nu)
ctx = af.Context(0)
mesh = af.Mesh.structured(ctx, 2, a.n, jitter=0.2, seed=20250220)
bsr = af.BSRFormat(mesh, 2).initialize(True)
bsr.computeSparsity()
rhs = ctx.malloc(8 * 2 * mesh.n_own_nodes)
legs = {"plain": lambda: bsr.assembleElasticityP1(lam, mu2)}
if not a.plain_only:
    legs["fused"] = lambda: bsr.assembleElasticityP1Ex(lam, mu2, 3.7e6, (0.5, -1.0), rhs, rhs_mode="set")
st = bsr.stats()
v = bsr.view()
nodes, blocks = mesh.n_own_nodes, v.nnz_blocks
# coordinates 24 B per node, row offsets 8 B per row, block columns 4 B and
# values 32 B per block, the incidence table 4 B per entry (padding included)
base = 24 * mesh.n_nodes + 8 * nodes + 36 * blocks + 4 * st["inc_table_entries"]
out = {"n": a.n, "nodes": nodes, "blocks": blocks, "inc_table_entries": st["inc_table_entries"], "reps": a.reps}
for name, fn in legs.items():
    ms, _ = bench.time_launches(ctx, fn, a.reps, 2, a.settle)
    nbytes = base + (16 * nodes if name == "fused" else 0)  # RHS 16 B per owned node
    med = float(np.median(ms))
    out[name] = {"median_ms": round(med, 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
                 "last_kernel": bsr.stats()["last_kernel"], "bytes": nbytes, "GBps": round(nbytes / med * 1e-6, 1)}
ctx.free(rhs)
print(json.dumps(out), flush=True)
