"""Kernel time of the block-2 triangle elasticity assembly on a 2D box of
(n + 1)^2 nodes: the plain entry (afem_bsr_assemble_elasticity_p1) and the
fused form with mass and body force (afem_bsr_assemble_elasticity_p1_ex),
each the median of --reps HIP-event-timed launches after the bench's settle,
with the algorithmic bytes of DESIGN.md section 3.1b-2.  With --dyn also the
fused elastodynamics step (afem_bsr_assemble_elastodynamics_p1, undamped and
damped constants; + 48 B per node for U, V, A and 2 B per node of flags) and
the 2D time loop's own step_timing() (assemble_ms + rhs_ms, median over
--steps steps with a traction on the right edge; the PCG cut at 4 iterations,
its time is not what is measured).  One JSON line.
usage: python tools/elasticity2d_time.py [--n 2048] [--reps 10] [--settle 150] [--plain-only] [--dyn] [--steps 12]"""
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
ap.add_argument("--dyn", action="store_true", help="also the fused elastodynamics step and the 2D loop's step timing")
ap.add_argument("--steps", type=int, default=12)
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
dyn_legs = {}
if a.dyn:
    from oracle import oracle as O  # noqa: E402

    n2 = 2 * mesh.n_nodes
    rng = np.random.default_rng(1)
    state = [ctx.malloc(8 * n2) for _ in range(3)]
    for p in state:
        ctx.to_device(p, rng.standard_normal(n2))
    flags = ctx.malloc(n2)
    ctx.to_device(flags, (rng.random(n2) < 0.01).astype(np.uint8))
    for name, (etam, etak) in {"dyn_undamped": (0.0, 0.0), "dyn_damped": (0.01, 0.01)}.items():
        c = O.elastodynamics_constants(lam, mu2 / 2, 1.0, 0.08, etam, etak)[2]
        dyn_legs[name] = c
        legs[name] = lambda c=c: bsr.assembleElastodynamicsP1(c, (0.5, -1.0), *state, flags, rhs, rhs_mode="set")
st = bsr.stats()
v = bsr.view()
nodes, blocks = mesh.n_own_nodes, v.nnz_blocks
# coordinates 24 B per node, row offsets 8 B per row, block columns 4 B and
# values 32 B per block, the incidence table 4 B per entry (padding included)
base = 24 * mesh.n_nodes + 8 * nodes + 36 * blocks + 4 * st["inc_table_entries"]
out = {"n": a.n, "nodes": nodes, "blocks": blocks, "inc_table_entries": st["inc_table_entries"], "reps": a.reps}
for name, fn in legs.items():
    ms, _ = bench.time_launches(ctx, fn, a.reps, 2, a.settle)
    nbytes = base + (16 * nodes if name != "plain" else 0)  # RHS 16 B per owned node
    if name in dyn_legs:
        nbytes += 48 * mesh.n_nodes + 2 * nodes  # U, V, A once per node; the flags
    med = float(np.median(ms))
    out[name] = {"median_ms": round(med, 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
                 "last_kernel": bsr.stats()["last_kernel"], "bytes": nbytes, "GBps": round(nbytes / med * 1e-6, 1)}
if a.dyn:
    _, coords, _ = mesh.download()
    right = np.flatnonzero(coords[:, 0] > 1.0 - 0.25 / a.n)
    right = right[np.argsort(coords[right, 1])].astype(np.int32)
    for name, etak in (("loop_undamped", 0.0), ("loop_damped", 0.01)):
        sim = af.Elastodynamics2D(ctx, mesh, 1.0, 0.08, E=E, nu=nu, body_force=(0.5, -1.0), etam=etak, etak=etak,
                                  rtol=1e-8, max_iter=4)
        sim.setDirichlet(np.flatnonzero(coords[:, 0] < 0.25 / a.n), (0.0, 0.0))
        sim.setTraction(np.stack([right[:-1], right[1:]], 1), (None, 0.01))
        sim.profile(True)
        t = []
        for _ in range(a.steps):
            sim.step()
            t.append(sim.step_timing())
        t = t[2:]  # the first steps build the solver's work arrays
        both = [x["assemble_ms"] + x["rhs_ms"] for x in t]
        out[name] = {"assemble_plus_rhs_ms": round(float(np.median(both)), 4), "min_ms": round(min(both), 4),
                     "max_ms": round(max(both), 4),
                     "assemble_ms": round(float(np.median([x["assemble_ms"] for x in t])), 4),
                     "rhs_ms": round(float(np.median([x["rhs_ms"] for x in t])), 4), "steps": len(t),
                     "traction_nodes": int(right.size)}
        sim.close()
ctx.free(rhs)
print(json.dumps(out), flush=True)
