// Scalar P1 (Poisson) assembly on the generator's Kuhn boxes, cell first:
// k_assemble_cubes.
//
// The strip / stencil kernels (assembly.hip) are row first: each of a tet's 4
// rows walks its cells and recomputes the tet's geometry (two cross products,
// |det|, the reciprocal: ~50 FP64 operations per row-step, 24 steps per row).
// Here each cube of the lattice is evaluated ONCE per unit: its 6 Kuhn tets
// (mesh.hip c_kuhn: for each axis permutation (a0,a1,a2) the tet
// (v0, v0+e_a0, v0+e_a0+e_a1, v0+(1,1,1))) give the cofactors, |det| and the 6
// off-diagonal entries K_ab = coef c_a.c_b / (6|det|) once; the contributions
// of the 6 tets to each of the cube's 19 Kuhn edges are summed in registers
// and added to the two rows of the edge with ds_add_f64 (LDS, wave-local, in
// program order: deterministic), the |det| sums of each corner likewise (the
// RHS source f |det| / 24, fused).  ~600 VALU operations per cube against
// ~1500 per row for the strip kernels.
//
// Unit = one wavefront: a column of 7 x 7 rows (node lines) over zs owned node
// layers.  Lane (i, j) owns the cube with lower corner (cx0 - 1 + i,
// cy0 - 1 + j): the 8 x 8 cubes touching the column's 7 x 7 rows, one per lane
// (the halo cubes are evaluated by both neighbouring columns: 64/49 = 1.31
// evaluations per cube, plus 1/zs for the cube layer below a segment).  The
// unit walks the cube layers upwards: node layer z's rows take the cube layers
// z-1 and z, so two row-layer accumulator buffers (by parity) live in LDS,
// [15][STRIDE] doubles each (15 column offsets in sorted order; the diagonal's
// plane, never added to, holds the |det| sum),
// and the node coordinates of the two layers of the current cube layer
// (9 x 9 nodes each, staged from registers loaded one layer ahead).  When a
// node layer is complete its 49 rows are written once: the values compacted
// by each row's present neighbours into a flat LDS image, then each x-run of
// 7 rows (contiguous in the matrix) with consecutive lanes.
//
// Single writer (the default instances: z carry, x and y exchange, dummy
// rows; V bit 2048): after the carry and the two exchanges a cube keeps 7 of
// its 19 edges and corner 3's |det| sum, each already the full sum over the
// cubes that share it, and each (row, offset) slot of a node layer takes
// exactly one of them per layer cycle.  So the 15 adds are plain LDS stores,
// nothing is zero-filled, the buffers are row-major ([64 rows][15 offsets]:
// the unit's 49 rows are the flat image already) and a complete layer's flush
// writes back the 49 diagonals only.  The instances without an exchange, with
// 49-row planes or without the dummy rows keep the adds into zeroed
// [15][STRIDE] planes described above.  Same bits either way.
//
// Which block runs which unit comes from a table (Structure::cube_units,
// build_cube_units, built once per structure and plan): block bid, on XCD
// bid & 7, loads record bid -- one 8-byte scalar load instead of the div / mod
// of the block index.  Each XCD takes a contiguous run of the units in lattice
// order (x fastest, then y, then z segment: neighbouring units share their halo
// coordinates in one L2) cut by modelled cost, not by count, and runs it most
// expensive unit first (columns on an x / y face, whose every layer takes the
// general flush, cost 1.6 x an interior column; the box's short last segment
// 0.65 x), so an XCD's slots go idle behind its cheapest units and all XCDs
// finish together: measured with the AFEM_WAVE_TIMES build
// (tools/cube_wave_times.py).  AFEM_CUBES_SCHED=0 builds
// the table in lattice order with equal counts per XCD, the mapping computed in
// the kernel up to r09a.  Same units, same arithmetic: same bits.
//
// Applies to meshes from afem_mesh_create_structured (3D, NB_DOF 1, any
// z-slab: the columns follow the local numbering -- owned layers, then the
// ghost layer below, then above -- so the sorted column order of a row next to
// the ghost layer below is recovered from the layers' local indices), and to
// lattices of Kuhn cubes handed over as arrays in any numbering (CANON: the
// structure's canonical maps, sparsity.hip canonical_lattice).  Values
// equal the oracle's to rounding (1e-12 per entry); not bitwise the strip
// kernels' (another summation order).  The default on generator boxes (C2:
// 0.58-0.59 ms against the stencil kernel's 0.64);
// AFEM_ASSEMBLY_CUBES=0 takes the strip / stencil path.
#include "afem_internal.hpp"

#include <algorithm>
#include <cstring>
#include <limits>
#include <vector>

// the 64-row instances cannot reach the 3-waves register target (their LDS
// allows 2 per SIMD): the compiler says so for each; expected
#pragma clang diagnostic ignored "-Wpass-failed"

namespace afem {

namespace {

inline unsigned grid_for(int64_t n, int threads) { return (unsigned)((n + threads - 1) / threads); }

struct P3 {
  double x, y, z;
};
__device__ __forceinline__ P3 psub(P3 a, P3 b) { return P3{ a.x - b.x, a.y - b.y, a.z - b.z }; }
__device__ __forceinline__ P3 pcross(P3 a, P3 b)
{
  return P3{ fma(a.y, b.z, -(a.z * b.y)), fma(a.z, b.x, -(a.x * b.z)), fma(a.x, b.y, -(a.y * b.x)) };
}
__device__ __forceinline__ double pdot(P3 a, P3 b) { return fma(a.z, b.z, fma(a.y, b.y, a.x * b.x)); }
__device__ __forceinline__ double precip(double a)
{
  const double r = __builtin_amdgcn_rcp(a);
  const double e = fma(-a, r, 1.0);
  return fma(r, e, r);
}

// one unit of the kernel's grid (build_cube_units): the column (cx, cy) of
// 7 x 7 rows over the owned node layers [z0, z1); z0 == z1: a padding record,
// its block ends at once.  In Structure::cube_units a record is 8 bytes,
// cx | cy << 16 and z0 | (z1 - z0) << 24 (16 bytes, one int each, compiled to 56
// spilled scalar registers in the headline instance against 49 with these 8 or
// with the arithmetic the table replaces: the kernel sits at the 106-SGPR cap)
struct CubeUnit {
  int32_t cx, cy, z0, z1;
};
constexpr int kUnitMaxColumns = 1 << 16, kUnitMaxLayer = 1 << 24, kUnitMaxLayers = 255;

#ifdef AFEM_WAVE_TIMES
// diagnostic build only (make EXTRA=-DAFEM_WAVE_TIMES OBJDIR=build_wt
// OUT=../libafem_wt.so; tools/cube_wave_times.py): start / end realtime stamps
// and the block index of every workgroup of the cube kernel, the first and the
// last 16 384 blocks of the grid (a grid of up to 32 768 blocks: all of them)
constexpr unsigned kCubeWtHalf = 16384;
__device__ unsigned long long afem_cube_wave_t[3 * 2 * kCubeWtHalf];
extern "C" int afem_debug_cube_wave_times(unsigned long long* out, int n)
{
  return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(afem_cube_wave_t), sizeof(unsigned long long) * (size_t)(3 * n));
}
#define AFEM_CWT(i, v)                                                                               \
  do {                                                                                               \
    const unsigned b_ = blockIdx.x, back_ = gridDim.x - b_;                                          \
    if (threadIdx.x == 0 && (b_ < kCubeWtHalf || back_ <= kCubeWtHalf)) {                            \
      const unsigned s_ = b_ < kCubeWtHalf ? b_ : 2 * kCubeWtHalf - back_;                           \
      afem_cube_wave_t[3 * s_ + (i)] = (v);                                                          \
      afem_cube_wave_t[3 * s_ + 2] = b_;                                                             \
    }                                                                                                \
  } while (0)
#else
#define AFEM_CWT(i, v) (void)0
#endif

struct CubeGeom {
  const uint2* units;  // the grid's unit records, one per block
  int npx, npy;      // nodes per x line, per y line
  int nzc;           // cells of the global box in z (node layers 0..nzc)
  int k0, k1;        // owned node layers [k0, k1)
  int ghost_lo, ghost_hi;
  int n_own_layers;
  int64_t L;         // nodes per layer
  int tx, ty, zs, ns;
  double s_coef;     // coef / 6
  double f_meas;     // f / 24
  int full_flush;    // flush_full for layers whose rows are all complete (AFEM_CUBES_FULL=0: not)
  double acc_init;   // single-writer instances (V bit 2048): no first fill of the accumulators (0.0),
                     // or, AFEM_CUBES_ACC_INIT=nan, a quiet NaN, to show that no flush reads a slot
                     // its layer did not write; the adding instances fill with 0.0 whatever this is
  int64_t row_stride;  // Structure::cube_row_stride: a row's offset on local layer l + 1 minus the one on
                       // layer l, for every layer a complete range can hold (0: not one constant)
};

// is global node layer k one of the slab's local layers (owned or ghost)?
__device__ __forceinline__ bool is_local(const CubeGeom& g, int k)
{
  return (k >= g.k0 && k < g.k1) || (k >= 0 && (k == g.ghost_lo || k == g.ghost_hi));
}
// local layer index of global node layer k (mesh.hip Layers::local_layer)
__device__ __forceinline__ int local_layer(const CubeGeom& g, int k)
{
  if (k >= g.k0 && k < g.k1) return k - g.k0;
  if (k == g.ghost_lo) return g.n_own_layers;
  return g.n_own_layers + (g.ghost_lo >= 0 ? 1 : 0);
}

// the 15 column offsets of a Kuhn row sorted by node id (x + npx (y + npy z)):
// by dz, then dy, then dx
__host__ __device__ constexpr int o_of(int dx, int dy, int dz)
{
  return dz < 0 ? (dy < 0 ? (dx < 0 ? 0 : 1) : (dx < 0 ? 2 : 3))
                : dz == 0 ? (dy < 0 ? (dx < 0 ? 4 : 5) : dy == 0 ? (dx < 0 ? 6 : (dx == 0 ? 7 : 8)) : (dx == 0 ? 9 : 10))
                          : (dy == 0 ? (dx == 0 ? 11 : 12) : (dx == 0 ? 13 : 14));
}
constexpr int kOffX[15] = { -1, 0, -1, 0, -1, 0, -1, 0, 1, 0, 1, 0, 1, 0, 1 };
constexpr int kOffY[15] = { -1, -1, 0, 0, -1, -1, 0, 0, 0, 1, 1, 0, 0, 1, 1 };
constexpr int kOffZ[15] = { -1, -1, -1, -1, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1 };

// corners c = ci + 2 cj + 4 ck; tet t = (0, 1 << a0, (1 << a0) | (1 << a1), 7)
constexpr int kPerm[6][2] = { { 0, 1 }, { 0, 2 }, { 1, 0 }, { 1, 2 }, { 2, 0 }, { 2, 1 } };
__host__ __device__ constexpr int tet_v(int t, int k)
{
  return k == 0 ? 0 : k == 1 ? (1 << kPerm[t][0]) : k == 2 ? ((1 << kPerm[t][0]) | (1 << kPerm[t][1])) : 7;
}
__host__ __device__ constexpr int cbit(int c, int a) { return (c >> a) & 1; }
// the row offset index of corner b seen from corner a
__host__ __device__ constexpr int edge_o(int a, int b)
{
  return o_of(cbit(b, 0) - cbit(a, 0), cbit(b, 1) - cbit(a, 1), cbit(b, 2) - cbit(a, 2));
}
// is (a, b), a < b, an edge of one of the 6 tets?
__host__ __device__ constexpr bool is_edge(int a, int b)
{
  bool e = false;
  for (int t = 0; t < 6; ++t)
    for (int p = 0; p < 4; ++p)
      for (int q = 0; q < 4; ++q)
        if (tet_v(t, p) == a && tet_v(t, q) == b) e = true;
  return e;
}

// lane L's value, wave-uniform (v_readlane into a scalar register: no LDS
// permute, and the address arithmetic on it stays scalar)
__device__ __forceinline__ int lane_i32(int v, int L) { return __builtin_amdgcn_readlane(v, L); }
__device__ __forceinline__ int64_t lane_i64(int64_t v, int L)
{
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, L);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)((uint64_t)v >> 32), L);
  return (int64_t)(((uint64_t)hi << 32) | lo);
}
__device__ __forceinline__ double lane_f64(double v, int L) { return __longlong_as_double(lane_i64(__double_as_longlong(v), L)); }

constexpr int kRun = 7;    // rows per x-run of a column
constexpr int kRows = 49;  // rows per column layer
constexpr int kCol = 9;    // staged nodes per x / y line (the column's rows + 1 halo line below)
constexpr int kAcc = 15;   // accumulators per row: 15 offsets, the diagonal's (7, never added to:
                           // v_7 = -sum of the others) holds the row's |det| sum

// One wave per block: LDS operations of a wave execute in issue order, so
// ordering its phases (staging -> cube adds -> flush reads -> image -> stores)
// needs only the compiler to keep the order, not an lgkmcnt(0) drain as
// __syncthreads emits (AFEM_CUBES_WAVESYNC=0 restores those)
#ifndef AFEM_CUBES_WAVESYNC
#define AFEM_CUBES_WAVESYNC 1
#endif
__device__ __forceinline__ void wave_lds_order()
{
#if AFEM_CUBES_WAVESYNC
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
#else
  __syncthreads();
#endif
}

// a value store, non-temporal when NT (cubes: V bits 32 / 128)
template <bool NT>
__device__ __forceinline__ void put(double* p, double v)
{
  if constexpr (NT)
    __builtin_nontemporal_store(v, p);
  else
    *p = v;
}
// two doubles as one 16-B access, at an 8-B aligned address (rows of 15 values) or a 16-B aligned one
typedef double d2u8 __attribute__((ext_vector_type(2), aligned(8)));
typedef double d2u16 __attribute__((ext_vector_type(2), aligned(16)));
template <bool NT>
__device__ __forceinline__ void put2(double* p, double a, double b)
{
  if constexpr (NT)
    __builtin_nontemporal_store(d2u8{ a, b }, reinterpret_cast<d2u8*>(p));
  else
    *reinterpret_cast<d2u8*>(p) = d2u8{ a, b };
}

// which of the 15 Kuhn neighbours (bit o: offset o) of node (x, y, z) a lattice
// of npx x npy nodes per layer, node layers 0..nzc, holds: branch-free (bitwise
// ands of the comparisons), so a flush that uses it stays straight-line code
__host__ __device__ __forceinline__ uint32_t presence_mask(int x, int y, int z, int npx, int npy, int nzc)
{
  uint32_t mask = 0;
#pragma unroll
  for (int o = 0; o < 15; ++o) {
    const int xx = x + kOffX[o], yy = y + kOffY[o], zz = z + kOffZ[o];
    const uint32_t in = (uint32_t)(xx >= 0) & (uint32_t)(yy >= 0) & (uint32_t)(xx < npx) & (uint32_t)(yy < npy) &
                        (uint32_t)(zz >= 0) & (uint32_t)(zz <= nzc);
    mask |= in << o;
  }
  return mask;
}
constexpr uint32_t kAllPresent = 0x7fffu;

// HAS_RHS / RHS_ADD at compile time: each flush's global stores are then a
// fixed, branch-free sequence.  That alone does not keep them in flight: the
// wait for the next layer's coordinates counts past them (vmcnt(N)) only if
// the loop body holds one flush and no branch around it (the z walk at the
// end of the kernel; tools/loop_waits.py shows the compiled loops)
// (registers, LDS and occupancy: cube_waves below)
// CANON: a lattice mesh in the caller's numbering (sparsity.hip canonical_lattice,
// Structure::cube_*): the unit walks lattice indices; a node's coordinates
// come through its caller id, a row's values go to the caller's row (first
// value cc.rb, canonical slot t at position cc.slot >> 4t) through a per-row
// image (row L at [15 L, 15 L + 15), stored row by row)
struct CubeCanon {
  const int32_t* phys;
  const int64_t* rb;
  const uint64_t* slot;
  double* stage;  // STAGE: one 128-B line per lattice row
};

// V: variant bits (AFEM_CUBES_V; the default kCubesV is what every result
// uses).  Values right: 16 the next layer's coordinates loaded before the
// cubes (their latency hides behind them), 32 non-temporal value stores in
// the complete-layer flush (the values are not re-read by this launch; the
// L2 keeps the coordinates the neighbouring units re-read), 64 one 16-B
// store per lane and x-run there (7 stores per layer instead of 14), 128
// non-temporal value and RHS stores in the other flushes, 256 dummy rows for
// the corners outside the unit (no zero selects; 64-row planes), 512 16-B
// row stores in the canonical flush, 1024 the canonical path STAGED (its rows
// written in lattice order as one 128-B line each -- the 15 values by Kuhn
// offset, the |det| sum at 15 -- and moved into the caller's rows by
// k_cube_unstage, caller row by caller row: whole-line stores), 2048 single
// writer (SW in the kernel: with the carry, both exchanges and the dummy rows
// every accumulator slot takes one sum per layer cycle, so the sums are stored
// into a buffer laid out as the image, flush_full writes back the diagonal
// alone and nothing is zero-filled; without 2048 the sums are added into
// zeroed offset planes, the same bits).  Diagnostic
// ablations (values wrong): 1 no value stores in the complete-layer flush, 2
// one LDS add per cube (the sum of its sums) instead of its 15, 4 no cube
// arithmetic, 8 no complete-layer flush.  Measured (r05d/e, C2 / C4, one
// process, settled): 0.520 / 4.53 ms with none, 0.465 / 4.20 with 16 | 32 | 64;
// adding 128 costs 5.6 % on the box and 11 % on the random arrays (r05h:
// scattered 8-B RHS stores and 120-B rows are worse non-temporal); 256 on top
// of 16 | 32 | 64: C2 0.4632 -> 0.4608 ms, C4 4.194 -> 4.097 ms (r05i); 512:
// random-numbered arrays (canonical path) 1.581 -> 1.538 ms (r05k); 1024 there:
// 1.539 -> 1.103 ms (r05as: 0.587 ms cube pass + 0.532 ms k_cube_unstage).
// 4096 (box and natural-lattice instances; the canonical ones never carry it):
// scalar row bases in the complete-layer loop -- where the structure's row
// offsets advance by one constant per layer (CubeGeom::row_stride != 0) that
// loop loads no row offsets (RS in the kernel); measured in DESIGN.md §3.1e (r09a).
// The bits by name (the numbers are what AFEM_CUBES_V, the tests, tools/ab_knobs.py
// and profiles/ say; the kernel derives its switches from them in one block):
constexpr int kVNoFullStores = 1;     // ablation: no value stores in the complete-layer flush
constexpr int kVOneAdd = 2;           // ablation: one LDS add per cube
constexpr int kVNoCubes = 4;          // ablation: no cube arithmetic
constexpr int kVNoFullFlush = 8;      // ablation: no complete-layer flush
constexpr int kVLoadAhead = 16;       // the next layer's coordinates loaded before the cubes
constexpr int kVFullNT = 32;          // non-temporal value stores in the complete-layer flush
constexpr int kVFull16B = 64;         // 16-B value stores there
constexpr int kVOtherNT = 128;        // non-temporal value and RHS stores in the other flushes
constexpr int kVDummyRows = 256;      // dummy rows for the corners outside the unit
constexpr int kVCanon16B = 512;       // 16-B row stores in the canonical flush
constexpr int kVStaged = 1024;        // the canonical path staged
constexpr int kVSingleWriter = 2048;  // single writer
constexpr int kVRowStride = 4096;     // scalar row bases in the complete-layer loop
constexpr int kCubesBase = kVLoadAhead | kVFullNT | kVFull16B | kVDummyRows | kVCanon16B | kVStaged |
                           kVSingleWriter;  // the default up to r08a
constexpr int kCubesV = kCubesBase | kVRowStride;

// register budget (the compiler's figures, profiles/r11a_cubes_loop_waits.txt):
// 64-row planes + one coordinate layer (carry) = 17 304 B of LDS, + two (no
// carry) 19 248 B: 2 waves per SIMD whatever the registers (256 VGPRs, no
// scratch); 49-row planes = 13 704 B with the carry, 15 648 B without: 3 per
// SIMD at <= 168 VGPRs, which those instances reach with 136-576 B of scratch
template <int STRIDE>
constexpr int cube_waves() { return STRIDE == 64 ? 2 : 3; }
template <int STRIDE, bool CARRY, bool XEX, bool YEX, bool CANON, bool HAS_RHS, bool RHS_ADD, int DIAG = kCubesV>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(cube_waves<STRIDE>(), cube_waves<STRIDE>()))) void k_assemble_cubes(
    CubeGeom g, const int64_t* __restrict__ rows, const double* __restrict__ coords, double* __restrict__ vals,
    double* __restrict__ rhs, CubeCanon cc)
{
  // STRIDE >= 49 rows per offset plane; the single-writer instances (SW below)
  // use each buffer's 15 x 64 doubles row-major instead, slot o of row r at 15 r + o
  __shared__ __align__(16) double acc[2][kAcc][STRIDE];
  // SoA coordinates of the node layers being read: with the carry the bottom
  // corners come from registers (Xc), so one layer -- the cube layer's top --
  // is read, and the next one is staged over it after the cubes
  constexpr int NCZ = CARRY ? 1 : 2;
  __shared__ double cz[NCZ][3][kCol * kCol];
  const int lane = threadIdx.x;
  // the unit of this block: one scalar load of its record from the structure's
  // unit table (build_cube_units below: blocks go round-robin over the 8 XCDs,
  // so record bid is XCD bid & 7's (bid >> 3)-th); a padding record is empty
  const uint2 rec = g.units[blockIdx.x];
  const int z0 = (int)(rec.y & 0xffffffu), z1 = z0 + (int)(rec.y >> 24);
  if (z0 >= z1) return;
  AFEM_CWT(0, __builtin_amdgcn_s_memrealtime());
  const int cx0 = kRun * (int)(rec.x & 0xffffu), cy0 = kRun * (int)(rec.x >> 16);
  const int zc_first = max(z0 - 1, 0);
  const int zc_last = min(z1 - 1, g.nzc - 1);  // cube layer zc: node layers zc, zc + 1

  // this lane's cube (i, j) and its staging share (nodes q = lane, lane + 64 of 81)
  const int ci = lane & 7, cj = lane >> 3;
  const int gx = cx0 - 1 + ci, gy = cy0 - 1 + cj;  // lower corner
  const bool cube_in = gx >= 0 && gy >= 0 && gx + 1 < g.npx && gy + 1 < g.npy;
  auto node_xy = [&](int q, int& nx, int& ny) {
    nx = cx0 - 1 + q % kCol;
    ny = cy0 - 1 + q / kCol;
  };
  // staging loads without branches (addresses clamped into the local mesh,
  // out-of-range positions hold a duplicate that no cube reads): straight-line
  // code, so the waits on them count past the later memory operations instead
  // of draining everything (vmcnt(0)) at a branch join
  double pre[2][3];
  int32_t pid[2] = { 0, 0 };  // CANON: the caller's ids of the next staged layer's nodes
  // a node's id = its layer's first id (wave-uniform: kept in scalar registers,
  // readfirstlane, so the address arithmetic of every layer's loads is a scalar
  // base plus a per-lane constant) + its place in the layer (computed once)
  auto layer_base = [&](int k) { return (int64_t)__builtin_amdgcn_readfirstlane(local_layer(g, k)) * g.L; };
  int64_t xy_id[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int q = min(lane + 64 * h, kCol * kCol - 1);
    int nx, ny;
    node_xy(q, nx, ny);
    nx = min(max(nx, 0), g.npx - 1);
    ny = min(max(ny, 0), g.npy - 1);
    xy_id[h] = nx + (int64_t)g.npx * ny;
  }
  auto clamp_layer = [&](int k) { return is_local(g, k) ? k : g.k0; };
  // CANON: the ids first (prefetch_ids, one step ahead), the coordinates through them
  auto prefetch_ids = [&](int k) {
    if constexpr (CANON) {
      const int32_t* const lp = cc.phys + layer_base(clamp_layer(k));
#pragma unroll
      for (int h = 0; h < 2; ++h) pid[h] = lp[xy_id[h]];
    }
  };
  auto load_layer_to = [&](int k, double (&dst)[2][3]) {
    const double* const lc = CANON ? coords : coords + 3 * layer_base(clamp_layer(k));
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int64_t n = CANON ? (int64_t)pid[h] : xy_id[h];
      dst[h][0] = lc[3 * n];
      dst[h][1] = lc[3 * n + 1];
      dst[h][2] = lc[3 * n + 2];
    }
  };
  auto load_layer = [&](int k) { load_layer_to(k, pre); };
  auto store_layer = [&](int buf) {
    buf = NCZ == 1 ? 0 : buf;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int q = min(lane + 64 * h, kCol * kCol - 1);  // lanes past the 81 nodes repeat node 80's store
      cz[buf][0][q] = pre[h][0];
      cz[buf][1][q] = pre[h][1];
      cz[buf][2][q] = pre[h][2];
    }
  };
  // DROWS (V bit 256, 64-row planes): dummy rows for the corners outside the
  // unit (slot_d below).  SW (V bit 2048, with the carry, both exchanges and
  // the dummy rows): SINGLE WRITER.  Every slot (row, offset) of a node layer
  // then takes exactly one sum per layer cycle -- after the carry and the
  // exchanges a cube keeps the 7 edges 0-3, 0-7, 1-7, 2-7, 3-7, 1-3, 2-3 and
  // corner 3's |det| sum, each geometric edge is exactly one cube's kept edge,
  // and that cube's lane is in the wave for every row of the unit -- so the
  // sums are STORED, not added: no zero fill anywhere, and the buffer is laid
  // out as the image (slot o of row r at 15 r + o, the dummy rows 49..63
  // behind: 960 doubles as before), so flush_full writes back the diagonal
  // alone.  Node layer z's slots 0..3 come from cube layer z - 1, 4..14 from
  // cube layer z; a slot of an absent neighbour (and a dummy row) holds stale
  // data, read only behind the presence mask.  Bitwise the adding instances:
  // 0.0 + x = x, and no summation order changes.
  // The switches of this instance, all derived here from its V bits (kV* above):
  constexpr bool NO_FULL_STORES = (DIAG & kVNoFullStores) != 0, ONE_ADD = (DIAG & kVOneAdd) != 0,
                 NO_CUBES = (DIAG & kVNoCubes) != 0, NO_FULL_FLUSH = (DIAG & kVNoFullFlush) != 0;
  constexpr bool LOAD_AHEAD = (DIAG & kVLoadAhead) != 0, FULL_NT = (DIAG & kVFullNT) != 0,
                 FULL_16B = (DIAG & kVFull16B) != 0, OTHER_NT = (DIAG & kVOtherNT) != 0,
                 CANON_16B = (DIAG & kVCanon16B) != 0;
  constexpr bool DROWS = (DIAG & kVDummyRows) != 0 && STRIDE == 64;
  constexpr bool SW = DROWS && CARRY && XEX && YEX && (DIAG & kVSingleWriter) != 0 && !ONE_ADD;
  constexpr bool STAGE = CANON && (DIAG & kVStaged) != 0;
  constexpr bool RS = !CANON && (DIAG & kVRowStride) != 0;  // (with g.row_stride != 0: load_run_bases below)
  // slot o of row r of buffer b
  auto slot = [&](int b, int r, int o) -> double* {
    return SW ? &acc[b][0][0] + kAcc * r + o : &acc[b][o][r];
  };
  // one accumulator buffer (kAcc * STRIDE doubles) filled: 16-B stores (64-row
  // planes: the buffers are 16-B aligned), 8-B ones for the 49-row planes
  auto clear_buffer = [&](double* buf, double fill) {
    if constexpr ((kAcc * STRIDE) % 2 == 0) {
      double2* const b2 = reinterpret_cast<double2*>(buf);
#pragma unroll
      for (int i = 0; i < (kAcc * STRIDE / 2 + 63) / 64; ++i)
        b2[min(64 * i + lane, kAcc * STRIDE / 2 - 1)] = make_double2(fill, fill);
    }
    else {
#pragma unroll
      for (int i = 0; i < (kAcc * STRIDE + 63) / 64; ++i) buf[min(64 * i + lane, kAcc * STRIDE - 1)] = fill;
    }
  };
  // SW: no slot is read before its layer cycle stored to it, so there is no
  // first fill either, unless the knob asks for the NaN that shows it
  // (both buffers in one rolled loop, not clear_buffer: the 49-row instances
  // gain scratch with the unrolled stores here)
  if (!SW || g.acc_init != g.acc_init) {
    const double fill = SW ? g.acc_init : 0.0;
    for (int i = lane; i < 2 * kAcc * STRIDE; i += 64) (&acc[0][0][0])[i] = fill;
  }

  // ---- node layer z complete: write its 49 rows (values compacted by the present neighbours) + RHS.
  // The rows' offsets are loaded before the layer's cubes (prefetch_rows), so
  // their latency hides behind the cube arithmetic instead of stalling here.
  const int rx = lane % kRun, ry = lane / kRun;
  const int nx = cx0 + rx, ny = cy0 + ry;
  const bool full_flush_on = g.full_flush != 0;
  int64_t pf_rb = 0, pf_re = 0, pf_r = 0;
  uint64_t pf_slot = 0;
  double pf_rhs = 0.0;
  const int64_t row_xy = min(nx, g.npx - 1) + (int64_t)g.npx * min(ny, g.npy - 1);  // the lane's row within its layer
  auto prefetch_rows = [&](int z) {  // clamped like load_layer: no branch
    const int zz = (z >= z0 && z < z1) ? z : z0;
    const int64_t lb = layer_base(zz);
    const int64_t li = lb + row_xy;
    if constexpr (STAGE) {
      (void)li;  // the rows' maps are k_cube_unstage's
    }
    else if constexpr (CANON) {
      pf_r = cc.phys[li];
      pf_rb = cc.rb[li];
      pf_slot = cc.slot[li];
    }
    else {
      pf_r = li;
      pf_rb = (rows + lb)[row_xy];
      pf_re = (rows + lb)[row_xy + 1];
      if constexpr (RHS_ADD) pf_rhs = rhs[pf_r];
    }
  };
  // a node layer whose 49 rows all have their 15 neighbours, in the sorted
  // order of the offsets (the unit away from the x / y faces of the box, z
  // off its bottom and top layers, the local layers in id order: not next to
  // a slab's ghost layer below): the row's values go to the image at 15 L + o,
  // and each x-run is 105 consecutive image values -- no masks, no
  // compaction, constant LDS offsets (flush_full)
  const bool xy_full = cx0 >= 1 && cx0 + kRun <= g.npx - 1 && cy0 >= 1 && cy0 + kRun <= g.npy - 1;
  // Such layers of a unit are one contiguous range [zf0, zf1) (wave-uniform,
  // computed once): an owned layer z has local index z - k0, below every later
  // owned layer's and below both ghost layers', so layers z and z + 1 are
  // always in id order, and z - 1 and z are unless z = k0 (the ghost layer
  // below, or no layer at all, under it).  With z + 1 <= nzc that leaves
  // k0 + 1 <= z <= nzc - 1.  The z walk runs the range in a loop of its own
  // whose body holds flush_full and no branch.
  auto full_range = [&](int zlo, int zhi, int& zf0, int& zf1) {  // of the node layers [zlo, zhi)
    const bool on = !CANON && xy_full && full_flush_on;
    zf0 = on ? min(max(zlo, g.k0 + 1), zhi) : zhi;
    zf1 = on ? max(min(zhi, g.nzc), zf0) : zhi;
  };
  // RS (V bit 4096, with g.row_stride != 0): the range's layers are consecutive
  // local layers and a row's offset grows by one constant from each to the
  // next (checked once per structure, cube_row_stride below), so its loop
  // loads no offsets: the 7 x-runs' first values of the range's first layer
  // are loaded once, with the unit's first coordinates, kept as 7 wave-uniform
  // pointers into the values and advanced by the constant per layer.  The loop's only
  // loads are then the coordinates of two layers ahead, and flush_full's first
  // store waits for nothing the previous layer's stores are queued behind
  // (loads and stores retire in order: the wait for offsets asked for after
  // layer z - 1's stores drained those stores, a quarter of a layer later).
  int64_t rs_rb = 0;
  auto load_run_bases = [&](int z) {  // clamped like prefetch_rows: no branch
    const int zz = (z >= z0 && z < z1) ? z : z0;
    rs_rb = (rows + layer_base(zz))[row_xy];
  };
  // ---- what the flushes share.  The lane's row of buffer b: its 15 slots into
  // v, the diagonal v[7] = -(the sum of the present neighbours' values, added
  // in the order o = 0..14), and meas, the |det| sum the diagonal's slot held
  auto read_row = [&](int b, uint32_t mask, double (&v)[15], double& meas) {
    const int lr = min(lane, STRIDE - 1);  // lanes past the 49 rows read a row they do not use
    double sum = 0.0;
#pragma unroll
    for (int o = 0; o < 15; ++o) {
      v[o] = *slot(b, lr, o);
      if (o != 7 && ((mask >> o) & 1u)) sum += v[o];
    }
    meas = v[7];
    v[7] = -sum;
  };
  // the row's RHS entry from its |det| sum (RHS_ADD: onto pf_rhs); lanes
  // without a row repeat lane 0's store (always a row)
  auto store_rhs = [&](bool valid, double meas) {
    if constexpr (HAS_RHS) {
      const double rv = RHS_ADD ? pf_rhs + g.f_meas * meas : g.f_meas * meas;
      const int64_t r0 = lane_i64(pf_r, 0);
      const double rv0 = lane_f64(rv, 0);
      put<OTHER_NT>(&rhs[valid ? pf_r : r0], valid ? rv : rv0);
    }
  };
  // (sb: where the 7 x-runs' first values go, wave-uniform, V bit 4096; null: by the lanes' prefetched offsets)
  auto flush_full = [&](int z, double* const* sb) {
    const int b = z & 1;
    const int lr = min(lane, STRIDE - 1);
    double v[15], meas;
    read_row(b, kAllPresent, v, meas);
    store_rhs(lane < kRows, meas);
    const int64_t rb = pf_rb;
    double* img = &acc[b][0][0];
    // (each lane storing its own row from registers instead -- 7 16-B stores at a
    // 120-B lane stride -- measured 3.19 against 0.456 ms, r05aw: the image stays)
    if constexpr (SW) {
      // the buffer is the image already: the diagonal goes where the |det| sum
      // was (the lane's own row: no other lane reads that slot before this
      // store), one LDS store instead of 15; the lanes past the 49 rows do the
      // same to their dummy rows
      img[kAcc * lane + 7] = v[7];
    }
    else {
      wave_lds_order();  // every lane's accumulator reads before the image overwrites them
      // row L at [15 L, 15 L + 15): lanes past the 49 rows write into
      // [735, 960) of the buffer, which no store reads (64-row planes), or --
      // 49-row planes, whose buffer ends at 735 -- repeat row 48's writes with
      // row 48's values (they read row 48: same addresses, same values)
#pragma unroll
      for (int o = 0; o < 15; ++o) img[15 * (STRIDE == 64 ? lane : lr) + o] = v[o];
    }
    wave_lds_order();
    // x-run q = rows 7q .. 7q + 6: 105 values contiguous in vals from row 7q's
    // first one; the second store's lanes past 105 repeat value 104 (same
    // address, same value)
    const int t1 = min(lane + 64, 15 * kRun - 1);
    // DIAG 64: one 16-B store per lane and run (values 2l, 2l + 1; lane 52
    // stores 103, 104 -- value 103 twice with the same data -- and the lanes
    // past it repeat lane 52's): 7 stores per layer instead of 14
    const int t2 = min(2 * lane, 15 * kRun - 2);
    // the 7 runs' image reads all issued before the first store (28 registers,
    // free here: the cube's sums are dead): one LDS round trip before the
    // stores instead of one per run
    double ra[kRun][2];
    if constexpr (!NO_FULL_STORES && FULL_16B) {
#pragma unroll
      for (int q = 0; q < kRun; ++q) {
        ra[q][0] = img[15 * kRun * q + t2];
        ra[q][1] = img[15 * kRun * q + t2 + 1];
      }
    }
#pragma unroll
    for (int q = 0; q < kRun; ++q) {
      double* const dst = sb ? sb[q] : vals + lane_i64(rb, kRun * q);
      if constexpr (NO_FULL_STORES) {
        (void)dst;  // diagnostic: no value stores
      }
      else if constexpr (FULL_16B) {
        put2<FULL_NT>(&dst[t2], ra[q][0], ra[q][1]);
      }
      else {
        put<FULL_NT>(&dst[lane], img[15 * kRun * q + lane]);
        put<FULL_NT>(&dst[t1], img[15 * kRun * q + t1]);
      }
    }
    wave_lds_order();
    if constexpr (!SW) {
      clear_buffer(img, 0.0);
      wave_lds_order();
    }
  };
  // STAGE: node layer z's rows into their lattice-order lines, line L = the
  // row's 15 values by Kuhn offset o and its |det| sum at 15 (an absent
  // neighbour's value is 0.0 -- the zero its slot holds, or selected here when
  // the slots are stored to (SW) -- and is never moved); x-run q
  // = 7 lines = 112 consecutive doubles, one 16-B non-temporal store per lane
  auto flush_stage = [&](int z) {
    const int b = z & 1;
    const bool valid = lane < kRows && nx < g.npx && ny < g.npy;
    // (presence_mask written out: through the function this instance's loop
    // compiles to one more vector instruction)
    uint32_t mask = 0;
#pragma unroll
    for (int o = 0; o < 15; ++o) {
      const int xx = nx + kOffX[o], yy = ny + kOffY[o], zz = z + kOffZ[o];
      const uint32_t in = (uint32_t)(xx >= 0) & (uint32_t)(yy >= 0) & (uint32_t)(xx < g.npx) & (uint32_t)(yy < g.npy) &
                          (uint32_t)(zz >= 0) & (uint32_t)(zz <= g.nzc);
      mask |= in << o;
    }
    if (!valid) mask = 0;
    double v[15], meas;
    read_row(b, mask, v, meas);
    wave_lds_order();  // every lane's accumulator reads before the image overwrites them
    double* img = &acc[b][0][0];
    if (lane < kRows) {  // 49 lines of 16 = 784 of the buffer's 960 doubles
      // SW: an absent neighbour's slot holds stale data, the line takes 0.0 for it
#pragma unroll
      for (int o = 0; o < 15; ++o) img[16 * lane + o] = (!SW || o == 7 || ((mask >> o) & 1u)) ? v[o] : 0.0;
      img[16 * lane + 15] = meas;
    }
    wave_lds_order();
    const int64_t lz = (int64_t)local_layer(g, z) * g.L + cx0;
    const bool xok = lane < 2 * 8 * kRun / 2 && cx0 + (lane >> 3) < g.npx;  // pair `lane` is line lane / 8's
    // a run past the box repeats run 0's store (always in the box), lanes
    // without a line lane 0's pair: same address, same values -- 7 stores
    // whatever the unit, so the waits after them count past them.  The image
    // reads of all runs first (as in flush_full).
    const int t = xok ? 2 * lane : 0;
    d2u16 w[kRun];
#pragma unroll
    for (int q = 0; q < kRun; ++q) {
      const int qs = cy0 + q < g.npy ? q : 0;  // uniform
      w[q] = d2u16{ img[2 * 8 * kRun * qs + t], img[2 * 8 * kRun * qs + t + 1] };
    }
#pragma unroll
    for (int q = 0; q < kRun; ++q) {
      const int qs = cy0 + q < g.npy ? q : 0;
      __builtin_nontemporal_store(w[q], reinterpret_cast<d2u16*>(&cc.stage[16 * (lz + (int64_t)g.npx * (cy0 + qs)) + t]));
    }
    wave_lds_order();
    if constexpr (!SW) {
      clear_buffer(img, 0.0);
      wave_lds_order();
    }
  };
  // the flush of any other layer (the z walk below picks flush_full for the
  // complete ones): no branch on the layer here, so its 1 + 14 stores (1 + 7
  // canonical, 7 staged) are a fixed sequence after the loop's loads
  auto flush = [&](int z) {
    if constexpr (STAGE) {
      flush_stage(z);
      return;
    }
    const int b = z & 1;
    const bool valid = lane < kRows && nx < g.npx && ny < g.npy;
    // present neighbours and the order of their local ids: the dz groups by local layer index
    uint32_t mask = presence_mask(nx, ny, z, g.npx, g.npy, g.nzc);
    if (!valid) mask = 0;
    const uint32_t gm0 = mask & 0x000Fu, gm1 = mask & 0x07F0u, gm2 = mask & 0x7800u;
    const int lm = local_layer(g, z - 1), l0 = local_layer(g, z), lp = local_layer(g, z + 1);
    const int n0 = __popc(gm0), n1 = __popc(gm1), n2 = __popc(gm2);
    const int s0 = (l0 < lm ? n1 : 0) + (lp < lm ? n2 : 0);
    const int s1 = (lm < l0 ? n0 : 0) + (lp < l0 ? n2 : 0);
    const int s2 = (lm < lp ? n0 : 0) + (l0 < lp ? n1 : 0);
    double v[15], meas;
    read_row(b, mask, v, meas);
    // the prefetched offsets are consumed without a branch (selects), so the
    // compiler keeps their load where prefetch_rows issued it
    const int64_t rb = valid ? pf_rb : 0;
    // (a 64-bit min: with only the low halves used the compiler reuses the
    // loaded high half's register at once, a write-after-write wait on the load)
    const int len = CANON ? (valid ? __popc(mask) : 0) : (valid ? (int)min(pf_re - pf_rb, (int64_t)15) : 0);
    if constexpr (CANON && RHS_ADD) pf_rhs = rhs[pf_r];
    store_rhs(valid, meas);
    // prefix of the row lengths within the x-run (7 lanes), the runs' offsets in the image
    int p = 0;
#pragma unroll
    for (int d = 1; d < kRun; ++d) {
      const int t = __shfl(len, lane - d);
      if (rx - d >= 0) p += t;
    }
    int img0 = 0;  // image offset of this lane's run
#pragma unroll
    for (int q = 0; q < kRun; ++q) {
      const int rl = lane_i32(p + len, kRun * q + kRun - 1);
      if (q < ry) img0 += rl;
    }
    wave_lds_order();  // every lane's accumulator reads before the image overwrites them
    double* img = &acc[b][0][0];
    if constexpr (CANON) {
      // row L's values at [15 L, 15 L + 15) in the caller's column order; its
      // first value and length in the free coordinate buffer of layer z & 1
      int64_t* const rbs = reinterpret_cast<int64_t*>(&cz[NCZ == 1 ? 0 : (z & 1)][0][0]);
      int* const lens = reinterpret_cast<int*>(rbs + 64);
      rbs[lane] = rb;
      lens[lane] = len;
      if (valid) {
#pragma unroll
        for (int o = 0; o < 15; ++o)
          if ((mask >> o) & 1u) {
            const int t = __popc(mask & ((1u << o) - 1u));  // canonical slot (sorted lattice indices)
            img[15 * lane + (int)((pf_slot >> (4 * t)) & 15u)] = v[o];
          }
      }
      wave_lds_order();
      // row by row, consecutive lanes over a row's values; positions past a
      // row's length repeat row 0's first value (always a row), so the store
      // count is fixed
      const int64_t rb0 = rbs[0];
      if constexpr (CANON_16B) {
        // 16 B per lane: pair k of row L = values j, j + 1 with j = min(2k, len - 2)
        // (the last pair overlaps the one before: same values), 8 pairs per row,
        // 7 stores per layer instead of 12; rows without values repeat row 0's
        // first pair
#pragma unroll
        for (int i = 0; i < (8 * kRows + 63) / 64; ++i) {
          const int Q = min(64 * i + lane, 8 * kRows - 1);
          const int L = Q >> 3, k = Q & 7;
          const int len = lens[L];
          const bool ok = len >= 2;
          const int j = ok ? min(2 * k, len - 2) : 0;
          const int src = ok ? 15 * L + j : 0;
          *reinterpret_cast<d2u8*>(&vals[ok ? rbs[L] + j : rb0]) = d2u8{ img[src], img[src + 1] };
        }
      }
      else {
#pragma unroll
        for (int i = 0; i < (15 * kRows + 63) / 64; ++i) {
          const int P = min(64 * i + lane, 15 * kRows - 1);
          const int L = P / 15, j = P - 15 * L;
          const bool ok = j < lens[L];
          put<OTHER_NT>(&vals[ok ? rbs[L] + j : rb0], img[ok ? P : 0]);
        }
      }
    }
    else {
    if (valid) {
#pragma unroll
      for (int o = 0; o < 15; ++o)
        if ((mask >> o) & 1u) {
          const int grp = o < 4 ? 0 : (o < 11 ? 1 : 2);
          const uint32_t gmask = grp == 0 ? gm0 : (grp == 1 ? gm1 : gm2);
          const int start = grp == 0 ? s0 : (grp == 1 ? s1 : s2);
          img[img0 + p + start + __popc(gmask & ((1u << o) - 1u))] = v[o];
        }
    }
    wave_lds_order();
    // x-run q: run_len(q) values from image offset img(q) to vals + rb(first row of run q).
    // A fixed count of unpredicated stores: lanes past a run repeat the first
    // value of run 0 (row 0 of the column is always a row: same address, same
    // value), so the next layer's waits on its coordinate loads count past them
    const int64_t dst0 = lane_i64(rb, 0);
    int off = 0;
#pragma unroll
    for (int q = 0; q < kRun; ++q) {
      const int rl = lane_i32(p + len, kRun * q + kRun - 1);
      const int64_t dst = lane_i64(rb, kRun * q);
#pragma unroll
      for (int h = 0; h < 2; ++h) {  // rl <= 7 rows x 15 = 105
        const int t = lane + 64 * h;
        const bool ok = t < rl;
        put<OTHER_NT>(&vals[ok ? dst + t : dst0], img[ok ? off + t : 0]);
      }
      off += rl;
    }
    }
    wave_lds_order();
    if constexpr (!SW) {
      clear_buffer(img, 0.0);
      wave_lds_order();
    }
  };

  // ---- cube layer zc: the lane's cube, its 6 tets, 19 edge sums and 8 corner |det| sums
  // CARRY: the top face of the lane's cube (5 edges, 4 corner |det| sums) is
  // the bottom face of its next cube layer, evaluated by the same lane: its
  // sums stay in registers and go into LDS once, with the next cube's
  double ce[5] = { 0.0, 0.0, 0.0, 0.0, 0.0 }, cm[4] = { 0.0, 0.0, 0.0, 0.0 };
  // the corners' accumulator rows for cube layer zc
  auto corner_frame = [&](int zc, uint32_t& inm, int& bb, int& bt) {
    bb = zc & 1;
    bt = (zc + 1) & 1;
    const int rx0 = ci - 1, ry0 = cj - 1;
    const bool zlo = zc >= z0, zhi = zc + 1 < z1;
    const bool xin0 = rx0 >= 0 && cx0 + rx0 < g.npx, xin1 = rx0 + 1 < kRun && cx0 + rx0 + 1 < g.npx;
    const bool yin0 = ry0 >= 0 && cy0 + ry0 < g.npy, yin1 = ry0 + 1 < kRun && cy0 + ry0 + 1 < g.npy;
    inm = 0;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      // (not the lane's cube_in: with the x exchange a corner row takes the
      // neighbour's sums even when this lane's cube is outside the box)
      const bool in = (cbit(c, 0) ? xin1 : xin0) && (cbit(c, 1) ? yin1 : yin0) && (cbit(c, 2) ? zhi : zlo);
      inm |= (uint32_t)in << c;
    }
  };
  // a corner outside the unit adds its zero into the OTHER node layer's
  // buffer at row lane (mod STRIDE): no address shared with the lanes adding
  // real values in the same instruction, none shared among the outside lanes
  // (a clamped row inside the column serialised the same-address adds of
  // neighbouring lanes: 0.73 -> 0.82 ms)
  const int r00 = (ci - 1) + kRun * (cj - 1), rs = lane % STRIDE;
  auto base_at = [&](uint32_t inm, int bb, int bt, int c) {
    const bool in = (inm >> c) & 1u;
    const int buf = (cbit(c, 2) ? bt : bb) ^ (in ? 0 : 1);
    return &acc[buf][0][0] + (in ? r00 + cbit(c, 0) + kRun * cbit(c, 1) : rs);
  };
  // DROWS (V bit 256, 64-row planes): a corner outside the unit (its row
  // index rx or ry outside [0, 6]) adds its REAL sum into a dummy row of its
  // own layer's buffer, rows 49..63, which no store reads: the x-outside
  // lanes (one x edge of the 8 x 8 lanes) at 49 + cj, the other y-outside ones
  // at 57 + rx -- 15 distinct rows for the 15 outside lanes of each corner, so
  // no two lanes of one ds_add_f64 share an address.  No zero selects on the
  // sums, no buffer swap; the rows of node layer z0 - 1 (below the segment,
  // not this unit's) get real sums too, so that buffer is zeroed after the
  // layer below (its next use is node layer z0 + 1).  Rows inside the unit but
  // outside the box take their sums in their own slots and are never stored.
  // SW: the same rows, the sums stored (a dummy row's slot then takes the
  // stores of several corners: nothing reads it), and no buffer is cleared.
  int row4[4];  // the corner's row (SW: its first slot, 15 x row)
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int rx = ci - 1 + (k & 1), ry = cj - 1 + (k >> 1);
    const bool inx = rx >= 0 && rx < kRun, iny = ry >= 0 && ry < kRun;
    row4[k] = (SW ? kAcc : 1) * ((inx && iny) ? rx + kRun * ry : (!inx ? kRows + cj : kRows + 8 + rx));
  }
  // corner c's slot o
  auto slot_d = [&](int bb, int bt, int c, int o) {
    return &acc[cbit(c, 2) ? bt : bb][0][0] + row4[c & 3] + (SW ? 1 : STRIDE) * o;
  };
  // a corner's sum into its slot: stored (SW) or added
  auto sum_d = [&](double* p, double x) {
    if constexpr (SW)
      *p = x;
    else
      atomicAdd(p, x);
  };
  // the top face's carried sums into LDS (the box's top node layer: no cube above)
  auto add_top = [&](int zc) {
    uint32_t inm;
    int bb, bt;
    corner_frame(zc, inm, bb, bt);
    auto kept = [&](int c, double x) { return ((inm >> c) & 1u) ? x : 0.0; };
    constexpr int ta[5] = { 4, 4, 4, 5, 6 }, tb[5] = { 5, 6, 7, 7, 7 };
    if constexpr (SW) {
      // the carried top-face sums are not exchanged, so several lanes still ADD
      // into one slot here: the dz = 0 slots (4..10) of the layer's rows are
      // cleared first (they hold the flush's leavings of two layers ago), then
      // the adds as in the adding instances -- the same bits.  Once per unit
      // at the box's top.
#pragma unroll
      for (int o = 4; o <= 10; ++o) (&acc[bt][0][0])[kAcc * lane + o] = 0.0;
      wave_lds_order();
    }
#pragma unroll
    for (int i = 0; i < 5; ++i) {
      if constexpr (DROWS) {
        atomicAdd(slot_d(bb, bt, ta[i], edge_o(ta[i], tb[i])), ce[i]);
        atomicAdd(slot_d(bb, bt, tb[i], edge_o(tb[i], ta[i])), ce[i]);
      }
      else {
        atomicAdd(base_at(inm, bb, bt, ta[i]) + STRIDE * edge_o(ta[i], tb[i]), kept(ta[i], ce[i]));
        atomicAdd(base_at(inm, bb, bt, tb[i]) + STRIDE * edge_o(tb[i], ta[i]), kept(tb[i], ce[i]));
      }
    }
#pragma unroll
    for (int c = 4; c < 8; ++c) {
      if constexpr (DROWS)
        atomicAdd(slot_d(bb, bt, c, 7), cm[c - 4]);
      else
        atomicAdd(base_at(inm, bb, bt, c) + STRIDE * 7, kept(c, cm[c - 4]));
    }
  };
  P3 Xc[4];  // the lane's cube's top corners, the next cube layer's bottom ones
  auto prime_corners = [&](int zc) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int q = (ci + cbit(c, 0)) + kCol * (cj + cbit(c, 1));
      const int bz = NCZ == 1 ? 0 : (zc & 1);
      Xc[c] = P3{ cz[bz][0][q], cz[bz][1][q], cz[bz][2][q] };
    }
  };
  auto cubes = [&](int zc) {
    // no branch around the cube: a lane whose cube is outside the box works on
    // its clamped (duplicated) coordinates and adds zeros -- a divergent region
    // here made the compiler drain the next layer's loads (vmcnt(0)) before the
    // arithmetic
    const int bb = zc & 1, bt = (zc + 1) & 1;
    // with CARRY the bottom corners are the previous cube layer's top corners
    // (registers: 12 LDS reads less per layer), the top ones from the staged layer
    P3 X[8];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int q = (ci + cbit(c, 0)) + kCol * (cj + cbit(c, 1));
      const int zb = NCZ == 1 ? 0 : bb, zt = NCZ == 1 ? 0 : bt;
      X[c] = CARRY ? Xc[c] : P3{ cz[zb][0][q], cz[zb][1][q], cz[zb][2][q] };
      X[c + 4] = P3{ cz[zt][0][q], cz[zt][1][q], cz[zt][2][q] };
      if constexpr (CARRY) Xc[c] = X[c + 4];
    }
    double ev[8][8];
    double mv[8];
#pragma unroll
    for (int a = 0; a < 8; ++a) {
      mv[a] = 0.0;
#pragma unroll
      for (int b = 0; b < 8; ++b) ev[a][b] = 0.0;
    }
#pragma unroll
    for (int t = 0; t < (NO_CUBES ? 0 : 6); ++t) {
      const int v1 = tet_v(t, 1), v2 = tet_v(t, 2);
      const P3 e1 = psub(X[v1], X[0]), e2 = psub(X[v2], X[0]), e3 = psub(X[7], X[0]);
      P3 k[4];
      k[1] = pcross(e2, e3);
      k[2] = pcross(e3, e1);
      k[3] = pcross(e1, e2);
      k[0] = P3{ -(k[1].x + k[2].x + k[3].x), -(k[1].y + k[2].y + k[3].y), -(k[1].z + k[2].z + k[3].z) };
      // a cube outside the box (clamped, duplicated coordinates) contributes
      // exact zeros: its corners' rows may still take the x-neighbour's sums
      const double meas = cube_in ? fabs(pdot(e1, k[1])) : 0.0;
      const double s = cube_in ? g.s_coef * precip(fmax(meas, 1e-300)) : 0.0;
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        mv[tet_v(t, p)] += meas;
#pragma unroll
        for (int q = p + 1; q < 4; ++q) {
          const int a = tet_v(t, p) < tet_v(t, q) ? tet_v(t, p) : tet_v(t, q);
          const int b = tet_v(t, p) < tet_v(t, q) ? tet_v(t, q) : tet_v(t, p);
          ev[a][b] += s * pdot(k[p], k[q]);
        }
      }
    }
    if constexpr (CARRY) {
      // bottom face = the previous cube layer's top face: its carried sums
      ev[0][1] += ce[0];
      ev[0][2] += ce[1];
      ev[0][3] += ce[2];
      ev[1][3] += ce[3];
      ev[2][3] += ce[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) mv[c] += cm[c];
      ce[0] = ev[4][5];
      ce[1] = ev[4][6];
      ce[2] = ev[4][7];
      ce[3] = ev[5][7];
      ce[4] = ev[6][7];
#pragma unroll
      for (int c = 0; c < 4; ++c) cm[c] = mv[c + 4];
    }
    if constexpr (YEX) {
      // the y = 1 face is the y = 0 face of lane + 8's cube: its bottom-layer
      // sums come over first (ds_bpermute; lanes with cj = 7 get their own,
      // their y = 1 corners are outside the unit), so the x exchange below
      // then passes on sums that already hold the diagonal neighbour's
      ev[2][3] += __shfl_down(ev[0][1], 8);
      ev[2][6] += __shfl_down(ev[0][4], 8);
      ev[2][7] += __shfl_down(ev[0][5], 8);
      ev[3][7] += __shfl_down(ev[1][5], 8);
      mv[2] += __shfl_down(mv[0], 8);
      mv[3] += __shfl_down(mv[1], 8);
    }
    if constexpr (XEX) {
      // the x = 1 face of this lane's cube is the x = 0 face of lane + 1's
      // (same 16-lane DPP row; a lane with ci = 7 gets a wrong neighbour but its
      // x = 1 corners are outside the unit): that lane's face sums come over
      // (row_shl:1; zeros from a cube outside the box) and this lane adds
      // both -- 4 edges and 2 corners of the bottom layer (the top face's are
      // carried, and exchanged as the next layer's bottom)
      auto from_next = [&](double x) {
        const long long v = __double_as_longlong(x);
        const int lo = __builtin_amdgcn_mov_dpp((int)(uint32_t)v, 0x101, 0xf, 0xf, true);
        const int hi = __builtin_amdgcn_mov_dpp((int)(uint32_t)((unsigned long long)v >> 32), 0x101, 0xf, 0xf, true);
        return __longlong_as_double((long long)(((unsigned long long)(uint32_t)hi << 32) | (uint32_t)lo));
      };
      ev[1][3] += from_next(ev[0][2]);
      ev[1][5] += from_next(ev[0][4]);
      ev[1][7] += from_next(ev[0][6]);
      ev[3][7] += from_next(ev[2][6]);
      mv[1] += from_next(mv[0]);
      mv[3] += from_next(mv[2]);
    }
    // each corner's accumulator row: its own when it is a row of this unit,
    // else a zero into the other buffer (base_at); every add runs unpredicated
    uint32_t inm;
    int bb_, bt_;
    corner_frame(zc, inm, bb_, bt_);
    auto kept = [&](int c, double x) { return ((inm >> c) & 1u) ? x : 0.0; };
    double dsum = 0.0;  // DIAG 2
#pragma unroll
    for (int a = 0; a < 8; ++a)
#pragma unroll
      for (int b = a + 1; b < 8; ++b)
        if (is_edge(a, b) && !(CARRY && cbit(a, 2) && cbit(b, 2)) &&
            !(XEX && !cbit(a, 0) && !cbit(b, 0) && !(cbit(a, 2) && cbit(b, 2))) &&
            !(YEX && !cbit(a, 1) && !cbit(b, 1) && !(cbit(a, 2) && cbit(b, 2)))) {
          if constexpr (ONE_ADD) {
            dsum += ev[a][b];
          }
          else if constexpr (DROWS) {
            sum_d(slot_d(bb_, bt_, a, edge_o(a, b)), ev[a][b]);
            sum_d(slot_d(bb_, bt_, b, edge_o(b, a)), ev[a][b]);
          }
          else {
            atomicAdd(base_at(inm, bb_, bt_, a) + STRIDE * edge_o(a, b), kept(a, ev[a][b]));
            atomicAdd(base_at(inm, bb_, bt_, b) + STRIDE * edge_o(b, a), kept(b, ev[a][b]));
          }
        }
#pragma unroll
    for (int c = 0; c < 8; ++c)
      if (!(CARRY && cbit(c, 2)) && !(XEX && !cbit(c, 0) && !cbit(c, 2)) && !(YEX && !cbit(c, 1) && !cbit(c, 2))) {
        if constexpr (ONE_ADD)
          dsum += mv[c];
        else if constexpr (DROWS)
          sum_d(slot_d(bb_, bt_, c, 7), mv[c]);  // |det| sums
        else
          atomicAdd(base_at(inm, bb_, bt_, c) + STRIDE * 7, kept(c, mv[c]));  // |det| sums
      }
    if constexpr (ONE_ADD) atomicAdd(&acc[bb_][0][rs], dsum);
  };

  // ---- walk the cube layers upwards (coordinates staged one layer ahead)
  // the node layers of cube layer zc sit in buffers zc & 1 and (zc + 1) & 1;
  // layer zc + 2's coordinates are loaded at the top of iteration zc and
  // staged at its end (into buffer zc & 1, read for the last time by the
  // cubes).  Loads and stores share vmcnt and retire in order, and the loads
  // are older than the flush's stores: the staging wait at the loop tail
  // leaves the layer's stores in flight only when the compiler can count them,
  // that is when every path from the loads to the tail issues the same
  // stores.  So each loop below has ONE flush and no branch around it (a
  // choice of flush inside the body made the tail wait vmcnt(0), draining the
  // stores before the next layer's arithmetic could start); tools/loop_waits.py
  // prints the loops' loads, stores and waits from the compiled code.
  // CANON: the coordinates go through the caller's ids, themselves loaded one
  // step before (next_layer: layer k's coordinates from the ids in pid, then
  // layer k + 1's ids into pid), so no trip waits for ids it has just asked for
  auto next_layer = [&](int k) {
    load_layer(k);
    prefetch_ids(k + 1);
  };
  // before a loop is entered the ids on their way are waited for (an empty
  // statement that reads them): a loop's first instruction is reached from its
  // entry and from its back edge, and a wait there takes the stricter of the
  // two counts -- with the ids just asked for on entry that is vmcnt(1),
  // which on the back edge drains the layer's stores.  The wait sits behind the
  // staging of coordinates loaded before those ids, so it costs no latency.
  auto settle_ids = [&]() {
    if constexpr (CANON) asm volatile("" : "+v"(pid[0]), "+v"(pid[1]));
  };
  // the complete range of the unit's node layers (the walk reaches z0 first)
  int zf0, zf1;
  full_range(z0, zc_last + 1, zf0, zf1);
  prefetch_ids(zc_first);
  load_layer(zc_first);
  // RS: the range's first offsets ride behind the first coordinates and are
  // settled below, behind the second layer's (in-order returns: no wait of
  // their own), so no loop head inherits a wait for them
  if constexpr (RS) load_run_bases(zf0);
  // the unit's first two layers in one batch (a second register set, free
  // here: one round trip instead of load, stage, load); CANON: the second
  // layer's ids are still on their way, its coordinates follow the staging
  double pre1[2][3];
  if constexpr (!CANON) load_layer_to(zc_first + 1, pre1);
  store_layer(zc_first & 1);
  if constexpr (CANON) {
    prefetch_ids(zc_first + 1);
    load_layer(zc_first + 1);
    prefetch_ids(zc_first + 2);
  }
  else {
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int d = 0; d < 3; ++d) pre[h][d] = pre1[h][d];
  }
  if constexpr (NCZ == 1) {  // the bottom layer into the corner registers before the top overwrites it
    wave_lds_order();
    prime_corners(zc_first);
    wave_lds_order();
  }
  store_layer((zc_first + 1) & 1);
  wave_lds_order();
  if constexpr (CARRY && NCZ == 2) prime_corners(zc_first);
  settle_ids();
  double* run_base[kRun] = {};  // RS: where x-run q's first value goes on the range's next layer
  if constexpr (RS) {
    asm volatile("" : "+v"(rs_rb));
#pragma unroll
    for (int q = 0; q < kRun; ++q) run_base[q] = vals + lane_i64(rs_rb, kRun * q);
  }
  int zc = zc_first;
  if (zc < z0) {  // the cube layer below the segment: its top corners only, no flush
    next_layer(zc + 2);
    wave_lds_order();
    cubes(zc);
    wave_lds_order();
    // node layer z0 - 1's buffer took real sums: clear it for node layer z0 + 1
    // (SW: not needed, node layer z0 + 1's cycle stores to every slot it reads)
    if constexpr (DROWS && !SW) {
      clear_buffer(&acc[zc & 1][0][0], 0.0);
      wave_lds_order();
    }
    store_layer(zc & 1);
    settle_ids();
    ++zc;
  }
  // every layer from here completes a node layer of the segment (z0 <= zc <=
  // zc_last < z1).  One trip: the offsets of the rows it completes, then the
  // coordinates of layer zc + 2 (V bit 16: before the cubes, their latency
  // hides behind them; else after, their 12 registers not live across them),
  // the cubes, the flush, the staging.
  auto layer_step = [&](int zc, auto&& fl) {
    prefetch_rows(zc);
    if constexpr (LOAD_AHEAD) next_layer(zc + 2);
    wave_lds_order();
    cubes(zc);
    if constexpr (!LOAD_AHEAD) next_layer(zc + 2);
    wave_lds_order();
    fl(zc);
    store_layer(zc & 1);
  };
  // the layers below the complete range, the range, the layers above it: the
  // general loop is compiled once and entered twice (ph), the complete-layer
  // loop between its two passes
#pragma nounroll
  for (int ph = 0; ph < 2; ++ph) {
    const int zend = ph == 0 ? zf0 : zc_last + 1;
#pragma nounroll
    for (; zc < zend; ++zc) layer_step(zc, flush);
    if constexpr (!CANON) {
      if (ph == 0) {
        if constexpr (RS) {
          // the complete range without offset loads (a loop of its own, so the
          // one below is the parent's when the structure has no constant stride)
          if (g.row_stride != 0) {
#pragma nounroll
            for (; zc < zf1; ++zc) {
              pf_r = layer_base(zc) + row_xy;  // zf0 <= zc < zf1: inside the segment
              if constexpr (RHS_ADD) pf_rhs = rhs[pf_r];
              if constexpr (LOAD_AHEAD) next_layer(zc + 2);
              wave_lds_order();
              cubes(zc);
              if constexpr (!LOAD_AHEAD) next_layer(zc + 2);
              wave_lds_order();
              if constexpr (!NO_FULL_FLUSH) flush_full(zc, run_base);
              store_layer(zc & 1);
#pragma unroll
              for (int q = 0; q < kRun; ++q) run_base[q] += g.row_stride;
            }
          }
        }
#pragma nounroll
        for (; zc < zf1; ++zc)
          layer_step(zc, [&](int z) {
            if constexpr (!NO_FULL_FLUSH) flush_full(z, nullptr);
          });
      }
    }
  }
  if (zc_last + 1 >= z0 && zc_last + 1 < z1) {  // the box's top layer (no cube above)
    prefetch_rows(zc_last + 1);
    if constexpr (CARRY) {
      add_top(zc_last);
      wave_lds_order();
    }
    flush(zc_last + 1);
  }
  AFEM_CWT(1, __builtin_amdgcn_s_memrealtime());
}

// the staged canonical path's maps, per lattice node i (caller row phys[i]):
// lat[row] = i, and for each position p of the row's columns the Kuhn offset o
// whose value goes there (canonical slot t = the rank of o among the present
// offsets, position = slot[i] >> 4t)
__global__ void k_cube_stage_maps(int64_t n, int npx, int npy, int nzc, const int32_t* __restrict__ phys,
                                  const uint64_t* __restrict__ slot, int32_t* __restrict__ lat,
                                  uint64_t* __restrict__ pinv)
{
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t L = (int64_t)npx * npy;
  const int z = (int)(i / L);
  const int64_t rem = i - (int64_t)z * L;
  const int y = (int)(rem / npx), x = (int)(rem - (int64_t)y * npx);
  const uint32_t mask = presence_mask(x, y, z, npx, npy, nzc);
  const uint64_t sl = slot[i];
  uint64_t w = 0;
  for (int o = 0; o < 15; ++o)
    if ((mask >> o) & 1u) {
      const int t = __popc(mask & ((1u << o) - 1u));
      const int pos = (int)((sl >> (4 * t)) & 15u);
      w |= (uint64_t)o << (4 * pos);
    }
  const int32_t r = phys[i];
  lat[r] = (int32_t)i;
  pinv[r] = w;
}

// the staged canonical path, second pass: caller rows r = 64 w + lane of
// wave w.  Each lane loads its row's lattice line (one aligned 128-B line:
// 8 16-B loads), puts it in LDS, picks its values into the wave's image in
// column order (row r at [rb_r - rb_0, +len)), and the wave stores the image
// -- the 64 rows' values, contiguous in the caller's matrix -- with
// consecutive lanes and 16-B stores: whole lines, where the single-pass
// canonical flush wrote each 120-B row into lines that other units complete
// at other times (WRITE_SIZE 1.77 GB for 1.28 GB)
constexpr int kUnLine = 18;  // LDS doubles per line (16 + 2: 16-B aligned, lanes l and l + 16 share banks only)
// UV: 1 non-temporal line loads, 2 non-temporal value stores -- both by default
// (the lines are read once, the values not by this launch): c2_arrays 1.102 ->
// 1.066 ms (r05bl; 1.094 / 1.075 with one of them); AFEM_UNSTAGE_V=0 / 1 / 2 for A/B
template <bool HAS_RHS, bool RHS_ADD, int UV = 3>
__global__ __launch_bounds__(64) void k_cube_unstage(int64_t n, const int64_t* __restrict__ rp,
                                                      const int32_t* __restrict__ lat,
                                                      const uint64_t* __restrict__ pinv,
                                                      const double* __restrict__ stage, double f_meas,
                                                      double* __restrict__ vals, double* __restrict__ rhs)
{
  __shared__ __align__(16) double line[64 * kUnLine];
  __shared__ __align__(16) double out[64 * 15 + 2];
  const int lane = threadIdx.x;
  const int64_t r0 = (int64_t)blockIdx.x * 64;
  const int64_t r = r0 + lane;
  const bool valid = r < n;
  const int64_t rc = valid ? r : n - 1;
  const int64_t rb = rp[rc], re = rp[rc + 1];
  const int64_t li = lat[rc];
  const uint64_t m = pinv[rc];
  typedef double d2a __attribute__((ext_vector_type(2), aligned(16)));
  // load k: lanes 8 j .. 8 j + 7 read row 8 k + j's line, 16 B each (8 whole
  // lines per instruction, not 64 pieces of 64 lines)
  const int part = lane & 7;
  d2a w[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int64_t lk = __shfl((int)li, 8 * k + (lane >> 3));
    if constexpr ((UV & 1) != 0)
      w[k] = __builtin_nontemporal_load(reinterpret_cast<const d2a*>(stage + 16 * lk) + part);
    else
      w[k] = reinterpret_cast<const d2a*>(stage + 16 * lk)[part];
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) reinterpret_cast<d2a*>(line + kUnLine * (8 * k + (lane >> 3)))[part] = w[k];
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
  if constexpr (HAS_RHS) {
    const double meas = line[kUnLine * lane + 15];
    if (valid) rhs[r] = RHS_ADD ? rhs[r] + f_meas * meas : f_meas * meas;
  }
  const int nv = (int)min((int64_t)64, n - r0);  // rows of this wave
  const int64_t rb0 = rp[r0], re1 = rp[r0 + nv];
  const int a = (int)(rb0 & 1);  // image offset: pairs 16-B aligned in the matrix
  const int len = valid ? (int)(re - rb) : 0;
  const int base = a + (int)(rb - rb0);
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int p = 0; p < 15; ++p)
    if (p < len) out[base + p] = line[kUnLine * lane + (int)((m >> (4 * p)) & 15u)];
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
  const int total = a + (int)(re1 - rb0);
#pragma unroll
  for (int k = 0; k < (64 * 15 + 2) / 128 + 1; ++k) {
    const int j = 2 * (64 * k + lane);
    if (j < total) {
      double* const g = vals + (rb0 - a + j);
      const bool lo = j >= a, hi = j + 1 < total;
      if (lo && hi) {
        if constexpr ((UV & 2) != 0)
          __builtin_nontemporal_store(d2a{ out[j], out[j + 1] }, reinterpret_cast<d2a*>(g));
        else
          *reinterpret_cast<d2a*>(g) = d2a{ out[j], out[j + 1] };
      }
      else if (lo)
        g[0] = out[j];
      else if (hi)
        g[1] = out[j + 1];
    }
  }
}

// cube_row_stride's check: rows l in [l0, l1) of nodes-per-layer L, every node
// xy: is the row's offset on layer l + 1 the one on layer l plus C?
__global__ void k_row_stride_check(const int64_t* __restrict__ rows, int64_t L, int64_t l0, int64_t l1, int64_t C,
                                   int32_t* __restrict__ bad)
{
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (l1 - l0) * L) return;
  const int64_t r = l0 * L + i;
  if (rows[r + L] - rows[r] != C) *bad = 1;
}

// the lattice the cube kernel walks on mesh m with structure S (the fields that
// do not depend on the launch); false: not a mesh for it
bool cube_lattice_geom(const Mesh& m, const Structure& S, int nb_dof, CubeGeom& g, bool& canon)
{
  const StructuredInfo& st = m.st;
  if (m.nv != 4 || nb_dof != 1) return false;
  // a generator box (or z-slab of one), a lattice of Kuhn cubes in a natural
  // numbering (lexicographic in some axis order: the plain instance, with the
  // lattice axes in that order -- the kernel's geometry reads the real
  // coordinates, and the cube's 6 tets do not depend on the axis order), or
  // one in any other numbering (the caller's maps)
  const bool natural = S.cube_natural;
  canon = !natural && S.canon && S.cube_ok;
  if (!canon && !natural && (!st.valid || st.dim != 3 || S.canon || st.lx > 0 || st.ly > 0 || st.n < 1)) return false;
  if (canon || natural) {
    const int64_t* Lc = natural ? S.nat_L : S.cube_L;
    g.npx = (int)Lc[0];
    g.npy = (int)Lc[1];
    g.nzc = (int)Lc[2] - 1;
    g.k0 = 0;
    g.k1 = (int)Lc[2];
    g.ghost_lo = g.ghost_hi = -1;
    g.L = Lc[0] * Lc[1];
  }
  else {
    g.npx = g.npy = st.n + 1;
    g.nzc = st.nz;
    g.k0 = st.k0;
    g.k1 = st.k1;
    g.ghost_lo = st.ghost_lo;
    g.ghost_hi = st.ghost_hi;
    g.L = st.L;
    if (g.L != (int64_t)g.npx * g.npy) return false;
  }
  g.n_own_layers = g.k1 - g.k0;
  if (g.n_own_layers <= 0 || g.nzc < 1 || g.npx < 2 || g.npy < 2) return false;
  g.tx = (g.npx + kRun - 1) / kRun;
  g.ty = (g.npy + kRun - 1) / kRun;
  return true;
}

// ---- the unit table.  The hardware hands out blocks in index order, block bid
// to XCD bid & 7, and a CU takes the next block when a slot frees, so the order
// of the records is a list schedule.  A unit's cost is modelled from what its
// walk runs (unit start, the cube layer below its segment, complete layers,
// general layers, the box's top layer), in units of one complete layer: the
// constants are the least-squares fit of the unit durations measured with the
// lattice-order table at C2 (profiles/r10a_cube_wave_times_parent.txt).
// (fit at C2, us: start 1.86, below 2.43, complete 2.99, general 4.99, top 2.69)
constexpr double kCostStart = 0.62;
constexpr double kCostBelow = 0.81;
constexpr double kCostFull = 1.0;
constexpr double kCostGeneral = 1.67;
constexpr double kCostTop = 0.90;
constexpr int kXcds = 8;

// One unit's walk, for the unit with first row (cx0, cy0) over the owned node
// layers [z0, z1): cube layers zc_first..zc_last, the complete node layers
// [zf0, zf1) (flush_full; none: zf0 = zf1 = zc_last + 1), below: it starts with
// the cube layer under the segment, top: it ends with the box's top node layer.
// The kernel does NOT call this: it keeps the same arithmetic in place (its
// zc_first, zc_last, xy_full, full_range, and the conditions of the layer below
// and of the top layer), because taking the walk from here, as a struct or as
// scalars, at the kernel's top or where the z walk starts, spilled 6 to 16 more
// scalar registers in 28 or more of the instances.  A
// change to either side has to be made on the other.
struct CubeWalk {
  int zc_first, zc_last, zf0, zf1;
  bool below, top;
};
__host__ __device__ __forceinline__ CubeWalk cube_walk(const CubeGeom& g, bool canon, int cx0, int cy0, int z0, int z1)
{
  CubeWalk w;
  w.zc_first = std::max(z0 - 1, 0);
  w.zc_last = std::min(z1 - 1, g.nzc - 1);
  const int zhi = w.zc_last + 1;
  const bool xy_full = cx0 >= 1 && cx0 + kRun <= g.npx - 1 && cy0 >= 1 && cy0 + kRun <= g.npy - 1;
  const bool on = !canon && xy_full && g.full_flush != 0;
  w.zf0 = on ? std::min(std::max(z0, g.k0 + 1), zhi) : zhi;
  w.zf1 = on ? std::max(std::min(zhi, g.nzc), w.zf0) : zhi;
  w.below = w.zc_first < z0;
  w.top = zhi >= z0 && zhi < z1;
  return w;
}
// what the walk runs on the unit: counted from cube_walk and nothing else
struct CubeUnitWork {
  int below, full, general, top;
};
CubeUnitWork cube_unit_work(const CubeGeom& g, bool canon, const CubeUnit& u)
{
  const CubeWalk k = cube_walk(g, canon, kRun * u.cx, kRun * u.cy, u.z0, u.z1);
  CubeUnitWork w;
  w.below = k.below ? 1 : 0;
  w.full = k.zf1 - k.zf0;
  // every cube layer after the one below flushes one node layer: the range's complete, the rest general
  w.general = std::max(k.zc_last + 1 - (k.zc_first + w.below), 0) - w.full;
  w.top = k.top ? 1 : 0;
  return w;
}
double cube_unit_cost(const CubeGeom& g, bool canon, const CubeUnit& u)
{
  const CubeUnitWork w = cube_unit_work(g, canon, u);
  return kCostStart + kCostBelow * w.below + kCostFull * w.full + kCostGeneral * w.general + kCostTop * w.top;
}

// Structure::cube_units for the plan (g, canon, sched, band_rows, pat), kept
// until the plan changes.  The units in lattice order are u = x + tx (y + ty
// segment); the segments' lengths are pat's, repeated from k0 up to k1 (one
// length: uniform segments, the default).
// sched 0: XCD x takes the x-th contiguous eighth of them by count, in that
// order; the grid is the units (the mapping the kernel computed up to r09a).
// sched 1: XCD x takes the x-th contiguous run by modelled cost (a unit goes to
// the eighth its cost's midpoint falls in: neighbouring units still share their
// halo coordinates in one L2), and runs it most expensive unit first, ties in
// lattice order, so what is left when an XCD's slots start to go idle is its
// cheapest units.  The runs differ in count: the grid is 8 x the longest, the
// shorter lists end in padding records.  band_rows > 0 (AFEM_CUBES_BAND, a
// measurement knob) sorts within bands of that many y-rows of units only: the
// whole-run sort reads 5 % more coordinates from HBM at C2 (FETCH_SIZE; 1 % of
// the launch's bytes) and is the faster one all the same.
void build_cube_units(const Mesh& m, Structure& S, const CubeGeom& g, bool canon, int sched, int band_rows,
                      const std::vector<int>& pat)
{
  int64_t pat_key = 0;
  for (int p : pat) pat_key = pat_key * 256 + p;
  const int64_t key[12] = { g.npx, g.npy, g.nzc, g.k0, g.k1, pat_key, (int64_t)pat.size(),
                            band_rows, g.n_own_layers, canon ? 1 : 0, g.full_flush, sched };
  if (S.cube_units.p && std::equal(key, key + 12, S.cube_units_key)) return;
  std::vector<int> cuts{ g.k0 };  // the segments' first layers, and k1
  for (size_t i = 0; cuts.back() < g.k1; ++i) cuts.push_back(std::min(cuts.back() + pat[i % pat.size()], g.k1));
  const int64_t n_col = (int64_t)g.tx * g.ty, n_units = n_col * (int64_t)(cuts.size() - 1);
  AFEM_REQUIRE(n_units < (int64_t(1) << 31), AFEM_ERR_LIMIT, "cube kernel: too many units");
  std::vector<CubeUnit> units((size_t)n_units);
  std::vector<double> cost((size_t)n_units);
  double total = 0.0;
  for (int64_t u = 0; u < n_units; ++u) {
    const int seg = (int)(u / n_col);
    units[u] = CubeUnit{ (int32_t)(u % g.tx), (int32_t)((u / g.tx) % g.ty), cuts[seg], cuts[seg + 1] };
    cost[u] = cube_unit_cost(g, canon, units[u]);
    total += cost[u];
  }
  std::vector<int64_t> list[kXcds];
  if (sched) {
    double cum = 0.0;
    for (int64_t u = 0; u < n_units; ++u) {
      const int x = std::min(kXcds - 1, (int)(kXcds * (cum + 0.5 * cost[u]) / total));
      list[x].push_back(u);
      cum += cost[u];
    }
    const int64_t band = band_rows > 0 ? (int64_t)band_rows * g.tx : n_units;
    for (auto& l : list)
      std::stable_sort(l.begin(), l.end(), [&](int64_t a, int64_t b) {
        return a / band != b / band ? a / band < b / band : cost[a] > cost[b];
      });
  }
  else {
    const int64_t qq = n_units / kXcds, rem = n_units % kXcds;
    for (int x = 0; x < kXcds; ++x) {
      const int64_t first = x * qq + std::min<int64_t>(x, rem), count = qq + (x < rem ? 1 : 0);
      for (int64_t j = 0; j < count; ++j) list[x].push_back(first + j);
    }
  }
  size_t longest = 0;
  double cmax = 0.0, cmin = std::numeric_limits<double>::max();
  for (const auto& l : list) {
    longest = std::max(longest, l.size());
    if (l.empty()) continue;  // fewer units than XCDs: the spread is over the XCDs that have some
    double c = 0.0;
    for (int64_t u : l) c += cost[u];
    cmax = std::max(cmax, c);
    cmin = std::min(cmin, c);
  }
  const int64_t n_rec = sched ? (int64_t)kXcds * (int64_t)longest : n_units;
  AFEM_REQUIRE(n_rec < (int64_t(1) << 31), AFEM_ERR_LIMIT, "cube kernel: too many units");
  AFEM_REQUIRE(g.tx <= kUnitMaxColumns && g.ty <= kUnitMaxColumns && g.k1 < kUnitMaxLayer,
               AFEM_ERR_LIMIT, "cube kernel: a unit does not fit its record");
  auto packed = [](const CubeUnit& u) {
    return uint2{ (uint32_t)u.cx | (uint32_t)u.cy << 16, (uint32_t)u.z0 | (uint32_t)(u.z1 - u.z0) << 24 };
  };
  std::vector<uint2> table((size_t)n_rec, packed(CubeUnit{ 0, 0, g.k0, g.k0 }));
  for (int x = 0; x < kXcds; ++x)
    for (size_t j = 0; j < list[x].size(); ++j) table[kXcds * j + x] = packed(units[list[x][j]]);
  Ctx& ctx = *m.ctx;
  S.cube_units.alloc(2 * (size_t)n_rec);
  AFEM_HIP(hipMemcpyAsync(S.cube_units.p, table.data(), sizeof(uint2) * (size_t)n_rec, hipMemcpyHostToDevice,
                          ctx.stream));
  ctx.sync();
  S.cube_units_n = n_rec;
  S.cube_units_real = n_units;
  S.cube_units_sched = sched;
  S.cube_xcd_spread = cmax / cmin;
  std::copy(key, key + 12, S.cube_units_key);
}

// ---- the compiled instances: {stride, carry, xex, yex, canon, V} and the
// kernel of each RHS mode it is compiled in (null: not compiled in that one)
enum { kRhsNone = 0, kRhsSet = 1, kRhsAdd = 2 };
constexpr int kInNone = 1 << kRhsNone, kInSet = 1 << kRhsSet, kInAll = kInNone | kInSet | 1 << kRhsAdd;
using CubeKernel = decltype(&k_assemble_cubes<64, true, true, true, false, true, false>);
struct CubeInstance {
  int stride;
  bool carry, xex, yex, canon;
  int v;
  CubeKernel k[3];
};
template <int STRIDE, bool CARRY, bool XEX, bool YEX, bool CANON, int V, int MODES>
CubeInstance cube_instance()
{
  CubeInstance i{ STRIDE, CARRY, XEX, YEX, CANON, V, { nullptr, nullptr, nullptr } };
  if constexpr ((MODES & kInNone) != 0) i.k[kRhsNone] = &k_assemble_cubes<STRIDE, CARRY, XEX, YEX, CANON, false, false, V>;
  if constexpr ((MODES & kInSet) != 0) i.k[kRhsSet] = &k_assemble_cubes<STRIDE, CARRY, XEX, YEX, CANON, true, false, V>;
  if constexpr ((MODES & 1 << kRhsAdd) != 0) i.k[kRhsAdd] = &k_assemble_cubes<STRIDE, CARRY, XEX, YEX, CANON, true, true, V>;
  return i;
}
// the other values AFEM_CUBES_V can take, RHS set only: the headline instance (box
// and natural lattices: 64 rows, carry, both exchanges) with V, and the canonical
// single-pass one with its counterpart, which never carries bits 1024 and 4096
template <int... V>
void add_variants(std::vector<CubeInstance>& t)
{
  (t.push_back(cube_instance<64, true, true, true, false, V, kInSet>()), ...);
  (t.push_back(cube_instance<64, true, true, true, true, V & ~(kVStaged | kVRowStride), kInSet>()), ...);
}
constexpr int kCanonV = kCubesBase & ~kVStaged;
std::vector<CubeInstance> cube_instances()
{
  constexpr int kB = kCubesBase;
  std::vector<CubeInstance> t{
    // what AFEM_CUBES_STRIDE / _CARRY / _XEX / _YEX and bit 4096 of AFEM_CUBES_V select, in every RHS mode
    cube_instance<64, true, true, true, false, kCubesV, kInAll>(),
    cube_instance<64, true, true, true, false, kB, kInAll>(),
    cube_instance<64, true, true, true, true, kCanonV, kInAll>(),
    cube_instance<49, true, true, true, false, kB, kInAll>(),
    cube_instance<64, true, true, false, false, kB, kInAll>(),
    cube_instance<64, true, false, false, false, kB, kInAll>(),
    cube_instance<49, false, false, false, false, kB, kInAll>(),
    cube_instance<64, false, false, false, false, kB, kInAll>(),
    // the staged canonical instances (V with bit 1024): no RHS, k_cube_unstage writes it
    cube_instance<64, true, true, true, true, kB, kInNone>(),
    cube_instance<64, true, true, true, true, kB | kVNoFullStores, kInNone>(),
    cube_instance<64, true, true, true, true, kB | kVNoCubes, kInNone>(),
    cube_instance<64, true, true, true, true, kB & ~kVSingleWriter, kInNone>(),
  };
  add_variants<0, kVLoadAhead | kVFullNT | kVFull16B, kB | kVNoFullStores, kB | kVOneAdd, kB | kVNoCubes,
               kB | kVNoFullFlush, kB & ~kVFullNT, kB & ~kVCanon16B, kB & ~kVStaged, kB & ~kVSingleWriter,
               kB & ~(kVStaged | kVSingleWriter), kCubesV | kVNoFullStores, kCubesV | kVNoCubes,
               kCubesV | kVNoFullFlush>(t);
  return t;
}
const std::vector<CubeInstance> kCubeInstances = cube_instances();
// the instance's kernel for the RHS mode; null: not compiled
CubeKernel find_cube_kernel(int stride, bool carry, bool xex, bool yex, bool canon, int v, int mode)
{
  for (const CubeInstance& i : kCubeInstances)
    if (i.stride == stride && i.carry == carry && i.xex == xex && i.yex == yex && i.canon == canon && i.v == v && i.k[mode])
      return i.k[mode];
  return nullptr;
}
// k_cube_unstage by AFEM_UNSTAGE_V, RHS set only (the other RHS modes: UV 3, the default)
using UnstageKernel = decltype(&k_cube_unstage<true, false>);
const UnstageKernel kUnstageSet[4] = { &k_cube_unstage<true, false, 0>, &k_cube_unstage<true, false, 1>,
                                       &k_cube_unstage<true, false, 2>, &k_cube_unstage<true, false, 3> };

// a knob that holds an integer (not set: dflt), and "the knob is set to 0"
int knob_int(const char* name, int dflt)
{
  const char* e = variant(name);
  return e ? atoi(e) : dflt;
}
bool knob_off(const char* name) { return knob_int(name, 1) == 0; }

}  // namespace

// Structure::cube_row_stride, once per structure (build_structure).  The node
// layers a unit's complete range can hold are z in [k0 + 1, min(k1, nzc)):
// owned, so local layers l = z - k0 in [1, lmax), consecutive.  The stride is
// the constant C with rows[(l + 1) L + xy] = rows[l L + xy] + C for every such
// pair of layers and every xy of the layer (C = rows[2 L] - rows[L]; with one
// such layer there is no pair, and C is never added to an offset that is
// used); 0 when there is no such layer, the lattice is a canonical one, or the
// device finds a pair that differs.
void cube_row_stride(const Mesh& m, Structure& S, int nb_dof)
{
  S.cube_row_stride = 0;
  CubeGeom g{};
  bool canon = false;
  if (!cube_lattice_geom(m, S, nb_dof, g, canon) || canon) return;
  const int64_t lmax = std::min(g.k1, g.nzc) - g.k0;
  if (lmax < 2 || lmax * g.L > S.n_rows) return;  // (every such layer's rows, and the one behind them, exist)
  Ctx& ctx = *m.ctx;
  int64_t h[2] = { 0, 0 };
  AFEM_HIP(hipMemcpyAsync(&h[0], S.row_ptr.p + g.L, sizeof(int64_t), hipMemcpyDeviceToHost, ctx.stream));
  AFEM_HIP(hipMemcpyAsync(&h[1], S.row_ptr.p + 2 * g.L, sizeof(int64_t), hipMemcpyDeviceToHost, ctx.stream));
  ctx.sync();
  const int64_t C = h[1] - h[0];
  if (C <= 0) return;
  int32_t bad = 0;
  const int64_t n_pairs = (lmax - 2) * g.L;  // layers l, l + 1 with 1 <= l, l + 1 < lmax
  if (n_pairs > 0) {
    DevBuf<int32_t> flag;
    flag.alloc(1);
    AFEM_HIP(hipMemsetAsync(flag.p, 0, flag.bytes(), ctx.stream));
    hipLaunchKernelGGL(k_row_stride_check, dim3(grid_for(n_pairs, 256)), dim3(256), 0, ctx.stream, S.row_ptr.p, g.L,
                       (int64_t)1, lmax - 1, C, flag.p);
    AFEM_LAUNCHED();
    AFEM_HIP(hipMemcpyAsync(&bad, flag.p, sizeof(bad), hipMemcpyDeviceToHost, ctx.stream));
    ctx.sync();
  }
  S.cube_row_stride = bad ? 0 : C;
}

bool assemble_cubes(Bsr& b, double coef, double f, double* rhs, int rhs_add)
{
  const Mesh& m = *b.mesh;
  Structure& S = b.s;
  if (knob_off("AFEM_ASSEMBLY_CUBES")) return false;  // the strip / stencil kernels
  CubeGeom g{};
  bool canon = false;
  if (!cube_lattice_geom(m, S, b.nb_dof, g, canon)) return false;
  Ctx& ctx = *m.ctx;
  g.row_stride = S.cube_row_stride;
  const char* ze = variant("AFEM_CUBES_ZS");
  // z segment: ~n/16 layers (C2 n = 215: 13, C4 n = 463: 29; r04x: zs 12 0.645 ms
  // vs zs 8 0.649 at C2, zs 32 6.38 vs zs 24 6.81 ms at C4)
  // AFEM_CUBES_ZS: one length, or a list "20/7" repeated up the box (graded segments: swept in
  // r10a, C2 within 1.4 % of the uniform default, not adopted)
  std::vector<int> pat;
  for (const char* p = ze; p && *p && pat.size() < 7; p = strchr(p, '/') ? strchr(p, '/') + 1 : "")
    pat.push_back(std::min(kUnitMaxLayers, std::max(1, atoi(p))));
  if (pat.empty()) pat.push_back(std::min(48, std::max(8, std::max(g.npx, g.npy) / 16)));
  g.zs = *std::max_element(pat.begin(), pat.end());
  g.ns = 0;
  g.s_coef = coef / 6.0;
  g.f_meas = f / 24.0;
  g.full_flush = knob_off("AFEM_CUBES_FULL") ? 0 : 1;
  // the single-writer instances' first accumulator fill (a test's knob: with a NaN
  // there the outputs stay finite only if no flush reads a slot its layer did not write)
  const char* ie = variant("AFEM_CUBES_ACC_INIT");
  g.acc_init = (ie && (ie[0] == 'n' || ie[0] == 'N')) ? std::numeric_limits<double>::quiet_NaN() : 0.0;
  // the unit table (built once per structure and plan): AFEM_CUBES_SCHED=0 keeps the
  // lattice order and the equal-count eighths, for the A/B of the order alone
  build_cube_units(m, S, g, canon, knob_off("AFEM_CUBES_SCHED") ? 0 : 1, std::max(0, knob_int("AFEM_CUBES_BAND", 0)),
                   pat);
  g.units = reinterpret_cast<const uint2*>(S.cube_units.p);
  // ---- the instance wanted, then looked up in kCubeInstances.
  // Accumulator planes of 64 rows, or of 49 (AFEM_CUBES_STRIDE=49; LDS and
  // occupancy: cube_waves -- with the carry it spills: r04y)
  const bool s49 = knob_int("AFEM_CUBES_STRIDE", 64) == 49;
  // the top face's sums carried in registers to the next cube layer (AFEM_CUBES_CARRY=0: not;
  // r04y C2: 0.605 ms with the carry at 64-row planes, 0.660 without at 49); the x = 1 face's
  // shared with lane + 1 over DPP (AFEM_CUBES_XEX=0: not; needs the carry); and the y = 1
  // face's with lane + 8 (AFEM_CUBES_YEX=0: not; needs the x exchange).  Canonical
  // structures: always all three.
  const bool carry = canon || !knob_off("AFEM_CUBES_CARRY");
  const bool xex = canon || (carry && !knob_off("AFEM_CUBES_XEX"));
  const bool yex = canon || (xex && !knob_off("AFEM_CUBES_YEX"));
  const bool all3 = carry && xex && yex;
  const int diag = knob_int("AFEM_CUBES_V", kCubesV);
  int mode = rhs ? (rhs_add ? kRhsAdd : kRhsSet) : kRhsNone;
  // 49-row planes exist with all three or with none of them.  The headline instance
  // (box, 64 rows, all three) takes bit 4096 as AFEM_CUBES_V says, in every RHS mode;
  // every other instance stays at the V it was built with: the canonical single-pass
  // one at the base without 1024, the rest at the base
  int stride = !canon && s49 && (all3 || !carry) ? 49 : 64;
  int v = canon ? kCanonV : (all3 && !s49 && (diag & kVRowStride) != 0) ? kCubesV : kCubesBase;
  // AFEM_CUBES_V: another variant of the headline instance (generator boxes and
  // natural lattices) or of the canonical one, RHS set only; a value that is not
  // in the list leaves the default
  if (diag != kCubesV && diag != kCubesBase && all3 && mode == kRhsSet &&
      find_cube_kernel(64, true, true, true, false, diag, kRhsSet)) {
    stride = 64;
    v = canon ? diag & ~(kVStaged | kVRowStride) : diag;
  }
  CubeCanon cc{ canon ? S.cube_phys.p : nullptr, canon ? S.cube_rb.p : nullptr, canon ? S.cube_slot.p : nullptr,
                nullptr };
  // the canonical path staged (V bit 1024): the cube kernel writes lattice-order
  // lines (no row maps, no RHS), k_cube_unstage moves them into the caller's rows
  // (every lattice node one of this structure's rows, as canonical_lattice builds it)
  const int64_t n_lat = g.L * (int64_t)(g.nzc + 1);
  const bool staged = canon && (diag & kVStaged) != 0 && n_lat == S.n_rows;
  if (staged) {
    if (S.cube_lat.n != (size_t)n_lat) {
      S.cube_lat.alloc(n_lat);
      S.cube_pinv.alloc(n_lat);
      hipLaunchKernelGGL(k_cube_stage_maps, dim3(grid_for(n_lat, 256)), dim3(256), 0, ctx.stream, n_lat, g.npx, g.npy,
                         g.nzc, S.cube_phys.p, S.cube_slot.p, S.cube_lat.p, S.cube_pinv.p);
      AFEM_LAUNCHED();
    }
    if (b.cube_stage.n != (size_t)(16 * n_lat)) b.cube_stage.alloc(16 * n_lat);
    cc.stage = b.cube_stage.p;
    // the staged instance exists without RHS only, in the default V or the listed ones
    mode = kRhsNone;
    v = find_cube_kernel(64, true, true, true, true, diag, kRhsNone) ? diag : kCubesBase;
  }
  const CubeKernel kern = find_cube_kernel(stride, carry, xex, yex, canon, v, mode);
  AFEM_REQUIRE(kern != nullptr, AFEM_ERR_NOT_IMPL, "cube kernel: no such instance");
  hipLaunchKernelGGL(kern, dim3((unsigned)S.cube_units_n), dim3(64), 0, ctx.stream, g, S.row_ptr.p, m.coords.p,
                     b.values.p, rhs, cc);
  AFEM_LAUNCHED();
  if (staged) {
    const int64_t n = S.n_rows;
    const int uv = knob_int("AFEM_UNSTAGE_V", 3);
    UnstageKernel un = rhs ? (rhs_add ? &k_cube_unstage<true, true> : kUnstageSet[3]) : &k_cube_unstage<false, false>;
    if (rhs && !rhs_add && uv >= 0 && uv < 3) un = kUnstageSet[uv];
    hipLaunchKernelGGL(un, dim3((unsigned)grid_for(n, 64)), dim3(64), 0, ctx.stream, n, S.row_ptr.p, S.cube_lat.p,
                       S.cube_pinv.p, b.cube_stage.p, g.f_meas, b.values.p, rhs);
    AFEM_LAUNCHED();
  }
  b.last_kernel = AFEM_KERNEL_CUBES;
  return true;
}

}  // namespace afem
