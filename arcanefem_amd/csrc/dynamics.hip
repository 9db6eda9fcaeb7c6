// Device vector kernels of the time-stepping callers of the path
// (modules/elastodynamics/FemModule.cc; modules/passmo/ElastodynamicModule.cc
// reassembles on a fixed structure every step, :469-536).  The per-step
// matrix is re-assembled by afem_bsr_assemble_elasticity_p1_ex (c0 M + K);
// these kernels form the Newmark right-hand side operand and update the
// state.  HBM-bound streaming kernels: 16-B per lane loads, grid-stride.
#include "afem_internal.hpp"

namespace afem {
namespace {

inline unsigned grid_for(int64_t n, int threads)
{
  const int64_t b = (n + threads - 1) / threads;
  return (unsigned)(b < 65535 * 16 ? b : 65535 * 16);
}

// out = a x + b y + c z  (z may be null)
__global__ void k_lincomb(int64_t n, double a, const double* __restrict__ x, double b, const double* __restrict__ y,
                          double c, const double* __restrict__ z, double* __restrict__ out)
{
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    double v = a * x[i] + b * y[i];
    if (z) v += c * z[i];
    out[i] = v;
  }
}

// modules/elastodynamics/FemModule.cc:429-455 (_updateVariables):
//   a' = (u_new - u - dt v) / (beta dt^2) - (1 - 2 beta) / (2 beta) a
//   v' = v + dt ((1 - gamma) a + gamma a');  a = a';  u = u_new
__global__ void k_newmark(int64_t n, double dt, double beta, double gamma, const double* __restrict__ un,
                          double* __restrict__ u, double* __restrict__ v, double* __restrict__ a)
{
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const double ui = u[i], vi = v[i], ai = a[i], uni = un[i];
    const double an = (uni - ui - dt * vi) / beta / (dt * dt) - (1. - 2. * beta) / 2. / beta * ai;
    v[i] = vi + dt * ((1. - gamma) * ai + gamma * an);
    a[i] = an;
    u[i] = uni;
  }
}

__global__ void k_scatter_vals(int64_t n, const int32_t* __restrict__ ids, const double* __restrict__ vals,
                               double* __restrict__ x)
{
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    x[ids[i]] = vals[i];
}

// Traction of the 2D elastodynamics loop (modules/elastodynamics/FemModule.cc:
// 880-967): node nodes[i] carries w[i] = sum of |e| / 2 over the group's edges
// at it; rhs[2 node + c] += t_c w[i] for the components of `mask`, unless the
// DoF is flagged.  Every node is listed once: one writer per DoF.
__global__ void k_traction2(int64_t n, const int32_t* __restrict__ nodes, const double* __restrict__ w, double t0,
                            double t1, unsigned mask, const uint8_t* __restrict__ fixed, double* __restrict__ rhs)
{
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t d = 2 * (int64_t)nodes[i];
  if ((mask & 1u) && !fixed[d]) rhs[d] += t0 * w[i];
  if ((mask & 2u) && !fixed[d + 1]) rhs[d + 1] += t1 * w[i];
}

__global__ void k_scatter_scaled(int64_t n, const int32_t* __restrict__ ids, const double* __restrict__ vals,
                                 double scale, double* __restrict__ x)
{
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    x[ids[i]] = scale * vals[i];
}

// Paraxial (absorbing) boundary of modules/soildynamics/FemModule.cc on block-2
// triangles, one lane per owned boundary node of the plan (ParaxialPlan).
// Per edge (node, other) of length L and unit normal n, with p7 = rho gamma /
// (beta dt), p8 = rho (1 - gamma / beta), p9 = rho dt (1 - gamma / (2 beta))
// (the module's c7 .. c9, :297-299):
//   LHS, the EDGE2 element matrix (:1376-1486): k11 = p7 (nx^2 cp + ny^2 cs),
//     k22 = p7 (ny^2 cp + nx^2 cs), k12 = p7 nx ny (cp - cs); the node's diagonal
//     block gets (k11, k22) L/3 and k12 L/6 on both cross entries, the (node,
//     other) block (k11, k22) L/6 and k12 L/6 -- the cross terms carry L/6 on
//     the diagonal block too (:1445-1483);
//   RHS (:875-935), S(W) = (W_node + W_other) + W_node per component:
//     rhs[2 node]     += (p7 f1(U) - p8 f1(V) - p9 f1(A)) L/6,
//       f1(W) = cp (nx^2 S1 + nx ny S2) + cs (ny^2 S1 - nx ny S2),
//     rhs[2 node + 1] likewise with
//       f2(W) = cp (nx ny S1 + ny^2 S2) + cs (-nx ny S1 + nx^2 S2),
//     unless the DoF is flagged in `fixed`.
// Reads: the plan, U / V / A of the node and of its edges' other ends (ghosts
// included).  Writes: the node's diagonal block (accumulated over its edges,
// added once), each (node, other) block and the node's two RHS entries --
// all of them in the node's own row, and every node is listed once, so every
// value has one writer: no atomics, the same bits every run.  The value
// positions come from the plan; no column search.
__global__ void k_paraxial2(int64_t n, const int32_t* __restrict__ nodes, const int32_t* __restrict__ eptr,
                            const int32_t* __restrict__ other, const double* __restrict__ geo,
                            const int64_t* __restrict__ dbase, const int64_t* __restrict__ obase,
                            const int32_t* __restrict__ stride, double cp, double cs, double p7, double p8, double p9,
                            const double* __restrict__ u, const double* __restrict__ v, const double* __restrict__ a,
                            const uint8_t* __restrict__ fixed, double* __restrict__ values, double* __restrict__ rhs)
{
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t nd = 2 * (int64_t)nodes[i];
  const int64_t st = stride[i];
  const double u0 = u[nd], u1 = u[nd + 1], v0 = v[nd], v1 = v[nd + 1], a0 = a[nd], a1 = a[nd + 1];
  double d00 = 0.0, d01 = 0.0, d11 = 0.0, r0 = 0.0, r1 = 0.0;
  for (int32_t e = eptr[i]; e < eptr[i + 1]; ++e) {
    const int64_t od = 2 * (int64_t)other[e];
    const double L = geo[4 * (int64_t)e], nx2 = geo[4 * (int64_t)e + 1], ny2 = geo[4 * (int64_t)e + 2],
                 nxy = geo[4 * (int64_t)e + 3];
    const double l6 = L / 6., l3 = L / 3.;
    const double k11 = p7 * (nx2 * cp + ny2 * cs), k22 = p7 * (ny2 * cp + nx2 * cs), k12 = p7 * (nxy * (cp - cs));
    d00 += k11 * l3;
    d11 += k22 * l3;
    d01 += k12 * l6;
    double* ob = values + obase[e];
    ob[0] += k11 * l6;
    ob[1] += k12 * l6;
    ob[st] += k12 * l6;
    ob[st + 1] += k22 * l6;
    const double su0 = (u0 + u[od]) + u0, su1 = (u1 + u[od + 1]) + u1;
    const double sv0 = (v0 + v[od]) + v0, sv1 = (v1 + v[od + 1]) + v1;
    const double sa0 = (a0 + a[od]) + a0, sa1 = (a1 + a[od + 1]) + a1;
    auto f1 = [&](double s1, double s2) { return cp * (nx2 * s1 + nxy * s2) + cs * (ny2 * s1 - nxy * s2); };
    auto f2 = [&](double s1, double s2) { return cp * (nxy * s1 + ny2 * s2) + cs * (-nxy * s1 + nx2 * s2); };
    r0 += (p7 * f1(su0, su1) - p8 * f1(sv0, sv1) - p9 * f1(sa0, sa1)) * l6;
    r1 += (p7 * f2(su0, su1) - p8 * f2(sv0, sv1) - p9 * f2(sa0, sa1)) * l6;
  }
  double* db = values + dbase[i];
  db[0] += d00;
  db[1] += d01;
  db[st] += d01;
  db[st + 1] += d11;
  if (!fixed || !fixed[nd]) rhs[nd] += r0;
  if (!fixed || !fixed[nd + 1]) rhs[nd + 1] += r1;
}

}  // namespace

void paraxial_add(Ctx& ctx, const ParaxialPlan& plan, double cp, double cs, const double p[3], const double* u,
                  const double* v, const double* a, const uint8_t* fixed, double* values, double* rhs)
{
  if (plan.n <= 0) return;
  hipLaunchKernelGGL(k_paraxial2, dim3(grid_for(plan.n, 64)), dim3(64), 0, ctx.stream, plan.n, plan.nodes.p,
                     plan.eptr.p, plan.other.p, plan.geo.p, plan.dbase.p, plan.obase.p, plan.stride.p, cp, cs, p[0],
                     p[1], p[2], u, v, a, fixed, values, rhs);
  AFEM_LAUNCHED();
}

void vec_scatter_scaled(Ctx& ctx, int64_t n, const int32_t* ids, const double* vals, double scale, double* x)
{
  if (n <= 0) return;
  hipLaunchKernelGGL(k_scatter_scaled, dim3(grid_for(n, 256)), dim3(256), 0, ctx.stream, n, ids, vals, scale, x);
  AFEM_LAUNCHED();
}

void traction2_add(Ctx& ctx, int64_t n, const int32_t* nodes, const double* w, const double t[2], unsigned mask,
                   const uint8_t* fixed, double* rhs)
{
  if (n <= 0 || !(mask & 3u)) return;
  hipLaunchKernelGGL(k_traction2, dim3(grid_for(n, 256)), dim3(256), 0, ctx.stream, n, nodes, w, t[0], t[1], mask,
                     fixed, rhs);
  AFEM_LAUNCHED();
}

void vec_scatter(Ctx& ctx, int64_t n, const int32_t* ids, const double* vals, double* x)
{
  if (n <= 0) return;
  hipLaunchKernelGGL(k_scatter_vals, dim3(grid_for(n, 256)), dim3(256), 0, ctx.stream, n, ids, vals, x);
  AFEM_LAUNCHED();
}

void vec_lincomb(Ctx& ctx, int64_t n, double a, const double* x, double b, const double* y, double c, const double* z,
                 double* out)
{
  if (n <= 0) return;
  hipLaunchKernelGGL(k_lincomb, dim3(grid_for(n, 256)), dim3(256), 0, ctx.stream, n, a, x, b, y, c, z, out);
  AFEM_LAUNCHED();
}

void newmark_update(Ctx& ctx, int64_t n, double dt, double beta, double gamma, const double* un, double* u, double* v,
                    double* a)
{
  if (n <= 0) return;
  hipLaunchKernelGGL(k_newmark, dim3(grid_for(n, 256)), dim3(256), 0, ctx.stream, n, dt, beta, gamma, un, u, v, a);
  AFEM_LAUNCHED();
}

}  // namespace afem
