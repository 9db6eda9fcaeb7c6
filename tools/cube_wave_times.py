"""Per-workgroup timeline of the cube kernel (k_assemble_cubes), diagnostic.

Needs the diagnostic build:
  make -C arcanefem_amd/csrc EXTRA=-DAFEM_WAVE_TIMES OBJDIR=build_wt OUT=../libafem_wt.so
usage: AFEM_LIB=arcanefem_amd/libafem_wt.so [AFEM_CUBES_SCHED=0] python tools/cube_wave_times.py [n] [launches]

Every workgroup (= one unit of the structure's unit table) stamps its start and
end (s_memrealtime, 100 MHz) and its block index.  For the last of `launches`
assemblies (default 50: settled clocks) this prints
  * the kernel span (first start to last end) and the unit table's plan;
  * per XCD (block index & 7): units, the time its last unit starts, the time
    its first slot goes idle for good (the first unit end after that start), the
    time its last unit ends, the largest number of units in flight, its idle share;
  * the idle share 1 - sum(unit durations) / (slots x span), slots = 8 XCDs x
    256 (8 waves per CU by LDS x 32 CUs): what no ordering of the same units
    can recover more than;
  * the median unit duration by class (face or interior column; bottom, inner,
    top or short segment), and the least-squares fit
    duration = start + below [the cube layer under the segment] + full x complete
    layers + general x general layers + top [the box's top node layer],
    whose ratios to `full` are cubes.hip's kCost* constants.
Grids of more than 32 768 blocks (C4) record their first and last 16 384."""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import arcanefem_amd as af  # noqa: E402
from arcanefem_amd import _capi as C  # noqa: E402

KRUN = 7
SLOTS_PER_XCD = 256

n = int(sys.argv[1]) if len(sys.argv) > 1 else 215
launches = int(sys.argv[2]) if len(sys.argv) > 2 else 50
ctx = af.Context(0)
mesh = af.Mesh.structured(ctx, 3, n, jitter=0.2, seed=20250220)
bsr = af.BSRFormat(mesh, 1).initialize(True)
bsr.computeSparsity()
ls = af.DoFLinearSystem().initialize(ctx, mesh.n_own_nodes)
for _ in range(launches):
    bsr.assemblePoissonP1(1.0, 5.5, ls.rhsVariable(), rhs_mode="set")
ctx.synchronize()
st = bsr.stats()
table = bsr.cube_unit_table(ctx)
N = 32768
buf = (ctypes.c_ulonglong * (3 * N))()
rc = C.load().afem_debug_cube_wave_times(buf, N)
assert rc == 0, rc
a = np.frombuffer(buf, dtype=np.uint64).reshape(N, 3).astype(np.int64)
a = a[(a[:, 0] > 0) & (a[:, 1] > 0)]
bid = a[:, 2]
assert np.unique(bid).size == bid.size and bid.max() < len(table)
t0 = a[:, 0].min()
start = (a[:, 0] - t0) / 100.0  # us
end = (a[:, 1] - t0) / 100.0
dur = end - start
span = end.max()
rec = table[bid]
xcd = bid & 7
print(f"n {n}  launches {launches}  plan: sched {st['cube_sched']}  units {st['cube_units']}  "
      f"records {st['cube_unit_records']}  modelled XCD cost spread {st['cube_xcd_cost_spread']:.4f}")
print(f"recorded workgroups {bid.size}  span {span:.1f} us  sum of unit durations {dur.sum() / 1e3:.2f} ms")
whole = bid.size == st["cube_units"]
if not whole:
    print("(not every unit recorded: the shares below cover the recorded ones only)")

# the walk of each unit (cubes.hip cube_unit_work): a generator box, k0 = 0, k1 = nzc + 1
npx = npy = n + 1
nzc, k0, k1 = n, 0, n + 1
cx0, cy0, z0, z1 = KRUN * rec[:, 0], KRUN * rec[:, 1], rec[:, 2], rec[:, 3]
zhi = np.minimum(z1 - 1, nzc - 1) + 1
interior = (cx0 >= 1) & (cx0 + KRUN <= npx - 1) & (cy0 >= 1) & (cy0 + KRUN <= npy - 1)
full_on = interior & (os.environ.get("AFEM_CUBES_FULL") != "0")
zf0 = np.where(full_on, np.minimum(np.maximum(z0, k0 + 1), zhi), zhi)
zf1 = np.where(full_on, np.maximum(np.minimum(zhi, nzc), zf0), zhi)
below = (np.maximum(z0 - 1, 0) < z0).astype(float)
full = (zf1 - zf0).astype(float)
general = np.maximum(zhi - z0, 0) - full
top = ((zhi >= z0) & (zhi < z1)).astype(float)
zs = int((z1 - z0).max())

print("xcd  units  last start  first slot idle  last end  in flight  idle share   (us)")
for x in range(8):
    m = xcd == x
    if not m.any():
        print(f"{x:3d}  {0:5d}")
        continue
    last_start = start[m].max()
    idle_from = end[m][end[m] >= last_start].min()
    ev = np.concatenate([np.stack([start[m], np.ones(m.sum())], 1), np.stack([end[m], -np.ones(m.sum())], 1)])
    ev = ev[np.lexsort((ev[:, 1], ev[:, 0]))]
    flight = int(np.cumsum(ev[:, 1]).max())
    print(f"{x:3d}  {m.sum():5d}  {last_start:10.1f}  {idle_from:15.1f}  {end[m].max():8.1f}  {flight:9d}  "
          f"{1.0 - dur[m].sum() / (SLOTS_PER_XCD * span):10.4f}")
print(f"idle share overall: {1.0 - dur.sum() / (8 * SLOTS_PER_XCD * span):.4f}  "
      f"(ends: p50 {np.median(end):.1f}  p90 {np.percentile(end, 90):.1f}  max {end.max():.1f} us)")

print("median unit duration by class (us; count)")
seg_kind = np.where(z1 - z0 < zs, "short", np.where(z0 == k0, "bottom", np.where(z1 == k1, "top", "inner")))
for col, cm in (("face", ~interior), ("interior", interior)):
    for kind in ("bottom", "inner", "top", "short"):
        m = cm & (seg_kind == kind)
        if m.any():
            print(f"  {col:8s} {kind:6s} {np.median(dur[m]):8.2f}  ({m.sum()})  layers: full {np.median(full[m]):.0f} "
                  f"general {np.median(general[m]):.0f} below {np.median(below[m]):.0f} top {np.median(top[m]):.0f}")
A = np.stack([np.ones_like(full), below, full, general, top], 1)
coef, *_ = np.linalg.lstsq(A, dur, rcond=None)
res = dur - A @ coef
names = ("start", "below", "full", "general", "top")
print("fit (us): " + "  ".join(f"{k} {v:.3f}" for k, v in zip(names, coef)) + f"  rms residual {np.sqrt((res ** 2).mean()):.2f}")
print("fit / full: " + "  ".join(f"{k} {v / coef[2]:.3f}" for k, v in zip(names, coef)))
