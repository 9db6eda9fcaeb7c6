// 3D elastodynamics time stepping on the assembly + CG path (BASELINE config
// C5), native behind the C ABI.  Mirrors the reference's time-stepping callers:
//   modules/elastodynamics/FemModule.cc  Newmark-beta constants (:255-270),
//     RHS M (c0 U + c3 V + c4 A) + body force (:842-862), state update
//     _updateVariables (:429-455), the matrix re-assembled every step (:149-153);
//   modules/passmo/ElastodynamicModule.cc  3D, re-assembly every step on a
//     fixed structure (:469-536).
// Per step: the fused block-3 kernel re-assembles c0 M + K and the body-force
// RHS (rhs_mode SET), the device lincomb + mass SpMV (the mass values share
// the stiffness structure, assembled once) add M (c0 U + c3 V + c4 A), the
// clamped DoFs are imposed by penalty, the Jacobi-PCG solves (halo exchange
// and dot-product sums over ranks when a communicator is attached; warm
// started from the Newmark predictor) and the Newmark update runs on the
// device.  Rayleigh damping (etam, etak) and the generalized-alpha scheme
// (alpm, alpf) follow the module's constants c0 .. c10 (:255-290): the LHS is
// c0 M + K(c1, c2) and the RHS adds K(lambda = 1) (-c5 U + c7 V + c8 A) +
// K(2 mu = 1) (-c6 U + c9 V + c10 A) (:842-862) -- two more operators on the
// same structure, assembled once.
//
// The module's own case, 2D TRIA3 with block 2, runs through the same handle
// and the same dyn_create / dyn_step (nb = 2; the phases that differ are the
// *_tet / *_tri functions): one fused kernel per step writes
// the LHS and the complete RHS from U, V, A (assemble_elastodynamics_tri), so
// that path keeps no M / K_lambda / K_mu and runs no SpMV or lincomb for the
// RHS; tractions (:880-967, constant or a CaseTable), the vectorial Dirichlet
// blocks (Penalty, RowElimination, RowColumnElimination; NULL components), the
// re-imposition of the constrained values after the solve (:1416-1417) and
// the Newmark update follow.  One subdomain.
//
// modules/soildynamics/FemModule.cc runs on that 2D step too: paraxial
// (absorbing) boundaries -- the EDGE2 matrix on the LHS (:1376-1486) and the
// edge loop over U, V, A on the RHS (:870-936), all blocks of a handle in one
// launch from a plan built at registration (paraxial_plan_build, k_paraxial2)
// -- right after the fused kernel, and the force-based double couple
// (:946-987), an assignment of +-F to four node groups' RHS entries right
// before the solve.  Newmark-beta without damping only (:321).
#include <algorithm>
#include <cmath>
#include <map>
#include <vector>

#include "elastodynamics.hpp"

namespace afem {

namespace {

// A profiled step makes the PCG time its preconditioner applications
// (opts.profile_comm = 1) and puts the caller's value back after the solve --
// also when the solve throws, so that an error leaves the options as they were.
struct ProfileCommGuard {
  afem_solver_opts& o;
  int32_t saved;
  ProfileCommGuard(afem_solver_opts& opts, bool on) : o(opts), saved(opts.profile_comm)
  {
    if (on) o.profile_comm = 1;
  }
  void restore() { o.profile_comm = saved; }
  ~ProfileCommGuard() { restore(); }
  ProfileCommGuard(const ProfileCommGuard&) = delete;
  ProfileCommGuard& operator=(const ProfileCommGuard&) = delete;
};

template <class T>
std::vector<T> to_host(Ctx& ctx, const T* p, int64_t n, int mem)
{
  std::vector<T> h(n);
  if (n) {
    AFEM_HIP(hipMemcpyAsync(h.data(), p, n * sizeof(T), mem == AFEM_MEM_HOST ? hipMemcpyHostToHost : hipMemcpyDeviceToHost,
                            ctx.stream));
    ctx.sync();
  }
  return h;
}

template <class T>
void upload(Ctx& ctx, DevBuf<T>& b, const std::vector<T>& h)
{
  b.alloc(h.size());
  if (!h.empty()) AFEM_HIP(hipMemcpyAsync(b.p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice, ctx.stream));
  ctx.sync();
}

// CaseTable::CurveLinear with `width` values per time: piecewise linear, constant outside
void table_interp(const std::vector<double>& times, const std::vector<double>& values, int width, double t, double* out)
{
  const size_t n = times.size();
  const bool before = t <= times.front() || n == 1;
  if (before || t >= times.back()) {
    for (int i = 0; i < width; ++i) out[i] = values[width * (before ? 0 : n - 1) + i];
    return;
  }
  const size_t k = std::upper_bound(times.begin(), times.end(), t) - times.begin();  // times[k-1] <= t < times[k]
  const double w = (t - times[k - 1]) / (times[k] - times[k - 1]);
  for (int i = 0; i < width; ++i)
    out[i] = values[width * (k - 1) + i] + w * (values[width * k + i] - values[width * (k - 1) + i]);
}

void halo_for(LinearSystem& ls, const Elastodynamics* d)
{
  Comm* comm = d->comm;
  Mesh& m = *d->mesh;
  if (!comm || comm_nranks(comm) == 1) return;
  std::vector<int> nb;
  std::vector<int64_t> sc, rc;
  std::vector<int32_t> si, ri;
  if (m.part.valid) {  // partitioned general mesh (afem_mesh_create_subdomain)
    nb = m.part.nbr;
    sc = m.part.send_cnt;
    rc = m.part.recv_cnt;
    si = m.part.send_ids;
    ri = m.part.recv_ids;
  }
  else {
    AFEM_REQUIRE(m.st.valid, AFEM_ERR_NOT_IMPL,
                 "distributed elastodynamics: the mesh carries no halo plan (structured slab or "
                 "afem_mesh_create_subdomain)");
    structured_halo_lists(m.st.dim, m.st.n, m.st.nz, m.st.nranks, m.st.rank, nb, sc, rc, si, ri);
  }
  expand_dof_lists(d->nb, sc, rc, si, ri);
  std::vector<int32_t> nb32(nb.begin(), nb.end());
  ls.halo.reset(new Halo());
  halo_setup(*ls.halo, *ls.ctx, comm, (int)nb.size(), nb32.data(), sc.data(), si.data(), rc.data(), ri.data());
}

void init_ls(LinearSystem& ls, Ctx* ctx, int64_t n, int64_t n_cols)
{
  ls.ctx = ctx;
  ls.n_rows = n;
  ls.n_cols = n_cols;
  ls.opts.method = AFEM_SOLVER_PCG;
  ls.opts.max_iter = 20000;
  ls.opts.rtol = 1e-8;
  ls.opts.atol = 0.0;
  ls.opts.check_every = 8;
  ls.opts.fixed_iterations = 0;
  ls.opts.initial_guess = 0;
  ls.opts.precond_block = 0;
  ls.rhs.alloc(n);
  ls.sol.alloc(n_cols);
  ls.forced_info.alloc(n);
  ls.elim_info.alloc(n);
  ls.forced_value.alloc(n);
  ls.elim_value.alloc(n);
  for (auto* b : { (void*)ls.rhs.p, (void*)ls.forced_value.p, (void*)ls.elim_value.p })
    AFEM_HIP(hipMemsetAsync(b, 0, n * sizeof(double), ctx->stream));
  AFEM_HIP(hipMemsetAsync(ls.sol.p, 0, n_cols * sizeof(double), ctx->stream));
  AFEM_HIP(hipMemsetAsync(ls.forced_info.p, 0, n, ctx->stream));
  AFEM_HIP(hipMemsetAsync(ls.elim_info.p, 0, n, ctx->stream));
}

// the scalar CSR of K's structure (bsr_expand_scalar) with `values` on it as l's matrix
void attach_csr(LinearSystem& l, const Bsr& K, double* values)
{
  const int k = K.nb_dof;
  l.has_csr = true;
  l.csr_n = l.n_rows;
  l.csr_nnz = K.s.nnz * k * k;
  l.csr_rows = K.csr_rows.p;
  l.csr_diag = nullptr;
  l.csr_cols = K.csr_cols.p;
  l.csr_vals = values;
  l.blk_k = k;
  l.blk_n = K.s.n_rows;
  l.blk_rows = K.s.row_ptr.p;
  l.blk_cols = K.s.cols.p;
}

void require_2d(const Elastodynamics* d, const char* what)
{
  AFEM_REQUIRE(d->nb == 2, AFEM_ERR_NOT_IMPL, (std::string(what) + ": the 2D loop's entry").c_str());
}
}  // namespace

// modules/elastodynamics/FemModule.cc:255-290: the Newmark-beta and
// generalized-alpha constants with Rayleigh damping (etam, etak)
void dyn_coefficients(Elastodynamics* d)
{
  const afem_newmark_params& p = d->p;
  const double lambda = d->lambda, mu = 0.5 * d->mu2, rho = p.rho, dt = p.dt, etam = p.etam, etak = p.etak;
  double* c = d->c;
  if (p.scheme == 1) {
    const double alpm = p.alpm, alpf = p.alpf;
    const double gamma = 0.5 + alpf - alpm, beta = 0.25 * (gamma + 0.5) * (gamma + 0.5);
    d->gamma = gamma;
    d->beta = beta;
    c[0] = rho * (1. - alpm) / (beta * dt * dt) + etam * rho * gamma * (1 - alpf) / beta / dt;
    c[1] = lambda * (1. - alpf) + lambda * etak * gamma * (1. - alpf) / beta / dt;
    c[2] = 2. * mu * (1. - alpf) + 2. * mu * etak * gamma * (1. - alpf) / beta / dt;
    c[3] = rho * (1. - alpm) / beta / dt - etam * rho * (1 - gamma * (1 - alpf) / beta);
    c[4] = rho * ((1. - alpm) * (1. - 2. * beta) / 2. / beta - alpm - etam * dt * (1. - alpf) * (1. - gamma / 2 / beta));
    c[5] = lambda * alpf - lambda * etak * gamma * (1. - alpf) / beta / dt;
    c[6] = 2 * mu * alpf - 2. * mu * etak * gamma * (1. - alpf) / beta / dt;
    c[7] = etak * lambda * (gamma * (1. - alpf) / beta - 1);
    c[8] = etak * lambda * dt * (1. - alpf) * ((1. - 2 * beta) / 2. / beta - (1. - gamma));
    c[9] = etak * 2 * mu * (gamma * (1. - alpf) / beta - 1);
    c[10] = etak * 2 * mu * dt * (1. - alpf) * ((1. - 2 * beta) / 2. / beta - (1. - gamma));
  }
  else {
    const double gamma = p.gamma > 0 ? p.gamma : 0.5;
    const double beta = p.beta > 0 ? p.beta : 0.25 * (gamma + 0.5) * (gamma + 0.5);
    d->gamma = gamma;
    d->beta = beta;
    c[0] = rho / (beta * dt * dt) + etam * rho * gamma / beta / dt;
    c[1] = lambda + lambda * etak * gamma / beta / dt;
    c[2] = 2. * mu + 2. * mu * etak * gamma / beta / dt;
    c[3] = rho / beta / dt - etam * rho * (1 - gamma / beta);
    c[4] = rho * ((1. - 2. * beta) / 2. / beta - etam * dt * (1. - gamma / 2 / beta));
    c[5] = -lambda * etak * gamma / beta / dt;
    c[6] = -2. * mu * etak * gamma / beta / dt;
    c[7] = etak * lambda * (gamma / beta - 1);
    c[8] = etak * lambda * dt * ((1. - 2 * beta) / 2. / beta - (1. - gamma));
    c[9] = etak * 2 * mu * (gamma / beta - 1);
    c[10] = etak * 2 * mu * dt * ((1. - 2 * beta) / 2. / beta - (1. - gamma));
  }
}

void dyn_set_lame(Elastodynamics* d, double lambda, double mu)
{
  require_2d(d, "afem_elastodynamics_set_lame");
  AFEM_REQUIRE(mu > 0 && lambda + mu > 0, AFEM_ERR_ARG, "afem_elastodynamics_set_lame: bad Lame parameters");
  d->lambda = lambda;
  d->mu2 = 2 * mu;
  d->tri.cp = d->tri.cs = 0.0;  // the paraxial wave speeds follow the Lame parameters again (FemModule.cc:268-273)
  dyn_coefficients(d);
}

void dyn_set_dirichlet_vectorial(Elastodynamics* d, const int32_t* nodes, int64_t n, const double values[2],
                                 unsigned mask, int method, int mem)
{
  require_2d(d, "afem_elastodynamics_set_dirichlet_vectorial");
  AFEM_REQUIRE(n >= 0 && (n == 0 || nodes) && values, AFEM_ERR_ARG,
               "afem_elastodynamics_set_dirichlet_vectorial: bad node list or values");
  AFEM_REQUIRE(method == AFEM_DIRICHLET_PENALTY || method == AFEM_DIRICHLET_ROW_ELIMINATION ||
                   method == AFEM_DIRICHLET_ROW_COLUMN_ELIMINATION,
               AFEM_ERR_NOT_IMPL,
               "enforce-Dirichlet-method: Penalty, RowElimination or RowColumnElimination (WeakPenalty is not "
               "implemented)");
  AFEM_REQUIRE(d->tri.dir_method < 0 || d->tri.dir_method == method, AFEM_ERR_ARG,
               "one enforce-Dirichlet-method for all conditions of a run");
  mask &= 3u;
  if (n == 0 || !mask) return;
  Ctx& ctx = *d->ctx;
  ctx.set_device();
  const std::vector<int32_t> hn = to_host(ctx, nodes, n, mem);
  std::vector<int32_t> own;
  for (int32_t v : hn) {
    AFEM_REQUIRE(v >= 0 && v < d->mesh->n_nodes, AFEM_ERR_ARG, "Dirichlet node id out of range");
    if (v < d->mesh->n_own) own.push_back(v);
  }
  d->tri.dir_method = method;
  Elastodynamics::Tri::Dirichlet2 dc;
  upload(ctx, dc.nodes, own);
  dc.mask = mask;
  for (int i = 0; i < 2; ++i) dc.v[i] = (mask >> i) & 1u ? values[i] : 0.0;
  for (int32_t v : own)
    for (int i = 0; i < 2; ++i)
      if ((mask >> i) & 1u) d->tri.dir_dofs[2 * v + i] = values[i];
  d->tri.dir2.push_back(std::move(dc));
  // the flags of the kernel's and the tractions' guards, and the list re-imposed after the solve
  std::vector<uint8_t> flags(d->n, 0);
  std::vector<int32_t> ids;
  std::vector<double> vals;
  for (const auto& kv : d->tri.dir_dofs) {
    flags[kv.first] = 1;
    ids.push_back(kv.first);
    vals.push_back(kv.second);
  }
  upload(ctx, d->tri.fixed2, flags);
  upload(ctx, d->imp_ids, ids);
  upload(ctx, d->imp_vals, vals);
}

void dyn_set_traction(Elastodynamics* d, const int32_t* face_nodes, int64_t n_faces, const double t[2], unsigned mask,
                      int mem)
{
  require_2d(d, "afem_elastodynamics_set_traction");
  AFEM_REQUIRE(n_faces >= 0 && (n_faces == 0 || face_nodes) && t, AFEM_ERR_ARG,
               "afem_elastodynamics_set_traction: bad face list or traction");
  Ctx& ctx = *d->ctx;
  ctx.set_device();
  const std::vector<int32_t> fn = to_host(ctx, face_nodes, 2 * n_faces, mem);
  const std::vector<double> xyz = to_host(ctx, d->mesh->coords.p, 3 * d->mesh->n_nodes, AFEM_MEM_DEVICE);
  std::map<int32_t, double> w;  // node -> sum of |e| / 2, faces in their order
  for (int64_t f = 0; f < n_faces; ++f) {
    const int32_t a = fn[2 * f], b = fn[2 * f + 1];
    AFEM_REQUIRE(a >= 0 && a < d->mesh->n_nodes && b >= 0 && b < d->mesh->n_nodes, AFEM_ERR_ARG,
                 "traction face node id out of range");
    const double len = std::hypot(xyz[3 * a] - xyz[3 * b], xyz[3 * a + 1] - xyz[3 * b + 1]);
    for (int32_t v : { a, b })
      if (v < d->mesh->n_own) w[v] += len / 2.;
  }
  std::vector<int32_t> nodes;
  std::vector<double> ws;
  for (const auto& kv : w) {
    nodes.push_back(kv.first);
    ws.push_back(kv.second);
  }
  Elastodynamics::Tri::Traction2 tr;
  upload(ctx, tr.nodes, nodes);
  upload(ctx, tr.w, ws);
  tr.mask = mask & 3u;
  for (int i = 0; i < 2; ++i) tr.t[i] = (tr.mask >> i) & 1u ? t[i] : 0.0;
  d->tri.trac2.push_back(std::move(tr));
}

void dyn_set_traction_table(Elastodynamics* d, int index, const double* times, const double* values, int64_t n)
{
  require_2d(d, "afem_elastodynamics_set_traction_table");
  AFEM_REQUIRE(index >= 0 && index < (int)d->tri.trac2.size(), AFEM_ERR_ARG,
               "afem_elastodynamics_set_traction_table: no such traction");
  AFEM_REQUIRE(n >= 1 && times && values, AFEM_ERR_ARG, "afem_elastodynamics_set_traction_table: empty table");
  for (int64_t i = 1; i < n; ++i)
    AFEM_REQUIRE(times[i] > times[i - 1], AFEM_ERR_ARG, "afem_elastodynamics_set_traction_table: times must increase");
  auto& tr = d->tri.trac2[index];
  tr.times.assign(times, times + n);
  tr.values.assign(values, values + 2 * n);
}

// ---------------------------------------------------------------- modules/soildynamics on the 2D loop
void paraxial_plan_build(Bsr& b, const std::vector<int32_t>& faces, ParaxialPlan& plan)
{
  Ctx& ctx = *b.mesh->ctx;
  const Mesh& m = *b.mesh;
  const int64_t n_faces = (int64_t)faces.size() / 2, n_own = b.s.n_rows;
  const std::vector<double> xyz = to_host(ctx, m.coords.p, 3 * m.n_nodes, AFEM_MEM_DEVICE);
  const std::vector<int64_t> rp = to_host(ctx, b.s.row_ptr.p, n_own + 1, AFEM_MEM_DEVICE);
  const std::vector<int32_t> cols = to_host(ctx, b.s.cols.p, b.s.nnz, AFEM_MEM_DEVICE);
  struct Entry {
    int32_t other;
    double g[4];
  };
  std::map<int32_t, std::vector<Entry>> by_node;  // owned node -> its edges in registration order
  for (int64_t f = 0; f < n_faces; ++f) {
    const int32_t ends[2] = { faces[2 * f], faces[2 * f + 1] };
    AFEM_REQUIRE(ends[0] >= 0 && ends[0] < m.n_nodes && ends[1] >= 0 && ends[1] < m.n_nodes, AFEM_ERR_ARG,
                 "paraxial face node id out of range");
    AFEM_REQUIRE(ends[0] != ends[1], AFEM_ERR_ARG, "paraxial face with twice the same node");
    // length and unit normal (_computeEdgeLength2 / _computeEdgeNormal2); only nx^2, ny^2 and nx ny enter
    const double dx = xyz[3 * ends[1]] - xyz[3 * ends[0]], dy = xyz[3 * ends[1] + 1] - xyz[3 * ends[0] + 1];
    const double len = std::sqrt(dx * dx + dy * dy);
    AFEM_REQUIRE(len > 0, AFEM_ERR_ARG, "paraxial face of zero length");
    const double nx = dy / len, ny = -dx / len;
    for (int k = 0; k < 2; ++k)  // an end that is a ghost has no row here (the module's isOwn() guards)
      if (ends[k] < n_own) by_node[ends[k]].push_back({ ends[1 - k], { len, nx * nx, ny * ny, nx * ny } });
  }
  std::vector<int32_t> nodes, eptr{ 0 }, other, stride;
  std::vector<double> geo;
  std::vector<int64_t> dbase, obase;
  auto block_at = [&](int32_t row, int32_t col, int64_t* base, int32_t* st) {
    const auto rb = cols.begin() + rp[row], re = cols.begin() + rp[row + 1];
    const auto it = std::lower_bound(rb, re, col);
    AFEM_REQUIRE(it != re && *it == col, AFEM_ERR_ARG, "paraxial face is not an edge of the mesh");
    const int64_t k = it - cols.begin(), len = rp[row + 1] - rp[row];
    *base = b.order_per_block ? 4 * k : 4 * rp[row] + 2 * (k - rp[row]);
    *st = b.order_per_block ? 2 : (int32_t)(2 * len);
  };
  for (const auto& kv : by_node) {
    int64_t base;
    int32_t st;
    block_at(kv.first, kv.first, &base, &st);
    nodes.push_back(kv.first);
    dbase.push_back(base);
    stride.push_back(st);
    for (const Entry& e : kv.second) {
      block_at(kv.first, e.other, &base, &st);
      other.push_back(e.other);
      obase.push_back(base);
      geo.insert(geo.end(), e.g, e.g + 4);
    }
    AFEM_REQUIRE(other.size() < ((size_t)1 << 31), AFEM_ERR_LIMIT, "too many paraxial faces");
    eptr.push_back((int32_t)other.size());
  }
  upload(ctx, plan.nodes, nodes);
  upload(ctx, plan.eptr, eptr);
  upload(ctx, plan.other, other);
  upload(ctx, plan.stride, stride);
  upload(ctx, plan.geo, geo);
  upload(ctx, plan.dbase, dbase);
  upload(ctx, plan.obase, obase);
  plan.n = (int64_t)nodes.size();
  plan.key = faces;
}

namespace {
// the module's own FATAL (:321) and what the paraxial constants are derived for
void require_soil(const Elastodynamics* d, const char* what)
{
  require_2d(d, what);
  AFEM_REQUIRE(d->p.scheme == 0 && d->p.etam == 0.0 && d->p.etak == 0.0, AFEM_ERR_NOT_IMPL,
               (std::string(what) + ": Only Newmark-beta works for time-discretization (no damping, no generalized-alpha)")
                   .c_str());
}
}  // namespace

void dyn_set_wave_speeds(Elastodynamics* d, double cp, double cs)
{
  require_2d(d, "afem_elastodynamics_set_wave_speeds");
  AFEM_REQUIRE(d->p.rho > 0, AFEM_ERR_ARG, "afem_elastodynamics_set_wave_speeds: rho must be > 0");
  const double mu = cs * cs * d->p.rho, lambda = cp * cp * d->p.rho - 2 * mu;  // FemModule.cc:275-278
  AFEM_REQUIRE(cp > 0 && cs > 0 && lambda + mu > 0, AFEM_ERR_ARG, "afem_elastodynamics_set_wave_speeds: bad wave speeds");
  d->lambda = lambda;
  d->mu2 = 2 * mu;
  d->tri.cp = cp;
  d->tri.cs = cs;
  dyn_coefficients(d);
}

void dyn_set_paraxial(Elastodynamics* d, const int32_t* face_nodes, int64_t n_faces, int mem)
{
  require_soil(d, "afem_elastodynamics_set_paraxial");
  AFEM_REQUIRE(n_faces >= 0 && (n_faces == 0 || face_nodes), AFEM_ERR_ARG, "afem_elastodynamics_set_paraxial: bad face list");
  AFEM_REQUIRE(d->p.rho > 0, AFEM_ERR_ARG, "afem_elastodynamics_set_paraxial: rho must be > 0");
  if (n_faces == 0) return;
  Ctx& ctx = *d->ctx;
  ctx.set_device();
  const std::vector<int32_t> fn = to_host(ctx, face_nodes, 2 * n_faces, mem);
  std::vector<int32_t> all = d->tri.par_faces;
  all.insert(all.end(), fn.begin(), fn.end());
  ParaxialPlan plan;
  paraxial_plan_build(d->K, all, plan);  // throws before the handle changes
  d->tri.par = std::move(plan);
  d->tri.par_faces = std::move(all);
}

void dyn_set_double_couple(Elastodynamics* d, const int32_t* const nodes[4], const int64_t n_nodes[4], const double* times,
                           const double* values, int64_t n, int mem)
{
  require_soil(d, "afem_elastodynamics_set_double_couple");
  AFEM_REQUIRE(n >= 1 && times && values, AFEM_ERR_ARG, "afem_elastodynamics_set_double_couple: empty table");
  for (int64_t i = 1; i < n; ++i)
    AFEM_REQUIRE(times[i] > times[i - 1], AFEM_ERR_ARG, "afem_elastodynamics_set_double_couple: times must increase");
  Ctx& ctx = *d->ctx;
  ctx.set_device();
  // north: rhs[2 v] = F, south: rhs[2 v] = -F, east: rhs[2 v + 1] = -F, west: rhs[2 v + 1] = F (:966-985); a DoF
  // named twice keeps the last assignment, as the module's successive loops
  static const int comp[4] = { 0, 0, 1, 1 };
  static const double sgn[4] = { 1.0, -1.0, -1.0, 1.0 };
  std::map<int32_t, double> m;
  for (int g = 0; g < 4; ++g) {
    AFEM_REQUIRE(n_nodes[g] >= 0 && (n_nodes[g] == 0 || nodes[g]), AFEM_ERR_ARG,
                 "afem_elastodynamics_set_double_couple: bad node list");
    for (int32_t v : to_host(ctx, nodes[g], n_nodes[g], mem)) {
      AFEM_REQUIRE(v >= 0 && v < d->mesh->n_nodes, AFEM_ERR_ARG, "double-couple node id out of range");
      if (v < d->mesh->n_own) m[2 * v + comp[g]] = sgn[g];
    }
  }
  Elastodynamics::Tri::DoubleCouple2 dc;
  std::vector<double> s;
  for (const auto& kv : m) {
    dc.hdofs.push_back(kv.first);
    s.push_back(kv.second);
  }
  upload(ctx, dc.dofs, dc.hdofs);
  upload(ctx, dc.sign, s);
  dc.times.assign(times, times + n);
  dc.values.assign(values, values + n);
  d->tri.dc2.push_back(std::move(dc));
}

// ---------------------------------------------------------------- create
namespace {
// the mass and damping operators on K's structure, the multigrid hints, the halos and the clamped DoFs
void create_tet(Elastodynamics* d, const int32_t* fixed_nodes, int64_t n_fixed, int mem)
{
  Ctx& ctx = *d->ctx;
  Mesh* mesh = d->mesh;
  Elastodynamics::Tet& s = d->tet;
  // an operator of the RHS: its values assembled once through K, its SpMV's system on K's scalar CSR
  auto op = [&](LinearSystem& l, DevBuf<double>& vals, double lambda, double mu2, double c0) {
    vals.alloc((size_t)d->K.s.nnz * 9);
    std::swap(d->K.values, vals);
    assemble_elasticity_tet(d->K, lambda, mu2, c0, nullptr, nullptr, 0);
    std::swap(d->K.values, vals);
    init_ls(l, &ctx, d->n, d->n_cols);
    attach_csr(l, d->K, vals.p);
    halo_for(l, d);
  };
  op(s.lsm, s.mvals, 0.0, 0.0, 1.0);  // M (c0 = 1)
  if (d->damped) {                    // the RHS's stiffness operators K(lambda = 1) and K(2 mu = 1)
    op(s.lsl, s.klvals, 1.0, 0.0, 0.0);
    op(s.lsu, s.kmvals, 0.0, 1.0, 0.0);
  }
  halo_for(d->ls, d);
  // structured box (or z-slab: block-Jacobi V-cycles over the ranks): the multigrid preconditioner
  const StructuredInfo& st = mesh->st;
  if (st.valid && st.dim == 3 && !mesh->part.valid) {
    d->ls.mg_k = 3;
    d->ls.mg_nx = st.n;
    d->ls.mg_nz = (st.k1 - st.k0) - 1;
    d->ls.mg_multi = st.nranks > 1;
    d->ls.mg_nzg = st.nz;
    d->ls.mg_k0 = st.k0;
    d->ls.mg_glo = st.ghost_lo >= 0;
  }
  s.MW.alloc(d->n);
  AFEM_HIP(hipMemsetAsync(s.MW.p, 0, s.MW.bytes(), ctx.stream));
  s.W.alloc(d->n_cols);  // ghost part filled by the mass SpMV's halo exchange
  AFEM_HIP(hipMemsetAsync(s.W.p, 0, s.W.bytes(), ctx.stream));
  std::vector<int32_t> dofs;
  for (int32_t nd : to_host(ctx, fixed_nodes, n_fixed, mem)) {
    AFEM_REQUIRE(nd >= 0 && nd < mesh->n_nodes, AFEM_ERR_ARG, "fixed node id out of range");
    if (nd < mesh->n_own)
      for (int i = 0; i < 3; ++i) dofs.push_back(3 * nd + i);
  }
  upload(ctx, s.fixed, dofs);
}

void create_tri(Elastodynamics* d, const int32_t* fixed_nodes, int64_t n_fixed, int mem)
{
  Ctx& ctx = *d->ctx;
  AFEM_HIP(hipMemsetAsync(d->K.values.p, 0, d->K.values.bytes(), ctx.stream));
  d->tri.t = d->p.dt;
  d->tri.fixed2.alloc(d->n);
  AFEM_HIP(hipMemsetAsync(d->tri.fixed2.p, 0, d->tri.fixed2.bytes(), ctx.stream));
  ctx.sync();
  if (n_fixed) {  // the clamped nodes of the 3D entry: both components 0, by penalty
    const double zero[2] = { 0.0, 0.0 };
    dyn_set_dirichlet_vectorial(d, fixed_nodes, n_fixed, zero, 3u, AFEM_DIRICHLET_PENALTY, mem);
  }
}
}  // namespace

Elastodynamics* dyn_create(Mesh* mesh, Comm* comm, const afem_newmark_params* prm, const int32_t* fixed_nodes,
                           int64_t n_fixed, int mem)
{
  const bool tri = mesh->nv == 3 && mesh->dim == 2;
  AFEM_REQUIRE(tri || (mesh->nv == 4 && mesh->dim == 3), AFEM_ERR_NOT_IMPL,
               "elastodynamics needs a tetrahedral (3D) or a triangle (2D) mesh");
  AFEM_REQUIRE(prm->dt > 0 && prm->E > 0 && prm->nu > -1.0 && prm->nu < 0.5 && prm->rho >= 0, AFEM_ERR_ARG,
               "elastodynamics: bad material or time step");
  AFEM_REQUIRE(n_fixed == 0 || fixed_nodes, AFEM_ERR_ARG, "fixed_nodes is NULL");
  AFEM_REQUIRE(prm->scheme == 0 || prm->scheme == 1, AFEM_ERR_ARG,
               "elastodynamics: scheme 0 (Newmark-beta) or 1 (generalized-alpha)");
  // each loop's own requirements on the communicator: here, before anything is allocated
  if (tri) {
    AFEM_REQUIRE(!comm || comm_nranks(comm) == 1, AFEM_ERR_NOT_IMPL,
                 "2D elastodynamics runs on one subdomain (a communicator of more than one rank)");
    AFEM_REQUIRE(mesh->n_own == mesh->n_nodes, AFEM_ERR_NOT_IMPL,
                 "2D elastodynamics runs on one subdomain (the mesh has ghost nodes)");
  }
  else if (comm)
    AFEM_REQUIRE(comm_nranks(comm) == 1 ||
                     (mesh->st.valid && mesh->st.nranks == comm_nranks(comm) && mesh->st.rank == comm_rank(comm)) ||
                     (mesh->part.valid && mesh->part.nranks == comm_nranks(comm) && mesh->part.rank == comm_rank(comm)),
                 AFEM_ERR_ARG, "the mesh's slab / subdomain rank and nranks differ from the communicator");
  mesh->ctx->set_device();
  auto* d = new Elastodynamics();
  try {
    Ctx& ctx = *mesh->ctx;
    d->mesh = mesh;
    d->ctx = &ctx;
    d->comm = comm;
    d->p = *prm;
    d->nb = tri ? 2 : 3;
    if (!(d->p.penalty > 0)) d->p.penalty = 1.0e30;  // modules/elasticity/Fem.axl:37-41
    // modules/elastodynamics/FemModule.cc:130-134, :239-240 (Lame; afem_elastodynamics_set_lame: :242-246)
    // and :255-290 (time scheme)
    d->mu2 = (prm->E / (2 * (1 + prm->nu))) * 2;
    d->lambda = prm->E * prm->nu / ((1 + prm->nu) * (1 - 2 * prm->nu));
    dyn_coefficients(d);
    d->damped = prm->etak != 0.0 || (prm->scheme == 1 && prm->alpf != 0.0);
    d->n = d->nb * mesh->n_own;
    d->n_cols = d->nb * mesh->n_nodes;
    // structure once; in 3D stiffness, mass and the damping operators share it
    d->K.mesh = mesh;
    d->K.nb_dof = d->nb;
    d->K.order_per_block = false;  // CSR row order: the values are the linear system's matrix
    build_structure(*mesh, d->K.s, tri ? 2 : 0);
    d->K.values.alloc((size_t)d->K.s.nnz * d->nb * d->nb);
    d->K.has_sparsity = true;
    bsr_expand_scalar(d->K, nullptr);  // scalar rows / columns of the block CSR (shared by every operator)
    init_ls(d->ls, &ctx, d->n, d->n_cols);
    attach_csr(d->ls, d->K, d->K.values.p);
    for (auto* b : { &d->U, &d->V, &d->A }) {
      b->alloc(tri ? d->n_cols : d->n);
      AFEM_HIP(hipMemsetAsync(b->p, 0, b->bytes(), ctx.stream));
    }
    if (tri)
      create_tri(d, fixed_nodes, n_fixed, mem);
    else
      create_tet(d, fixed_nodes, n_fixed, mem);
  }
  catch (...) {
    delete d;
    throw;
  }
  return d;
}

// ---------------------------------------------------------------- step
namespace {
void mark(const Elastodynamics* d, hipEvent_t e)
{
  if (d->profile) AFEM_HIP(hipEventRecord(e, d->ctx->stream));
}

// a double-couple DoF that a Dirichlet block constrains: the assignment would undo the condition's RHS
void check_sources_tri(const Elastodynamics* d)
{
  for (const auto& dc : d->tri.dc2)
    for (int32_t dof : dc.hdofs)
      AFEM_REQUIRE(!d->tri.dir_dofs.count(dof), AFEM_ERR_ARG,
                   "elastodynamics step: a double-couple DoF is constrained by a Dirichlet condition");
}

// LHS c0 M + K(c1, c2) and the body force (rhs = f |K|/4), re-assembled on the fixed structure
void lhs_tet(Elastodynamics* d)
{
  const double f[3] = { d->p.body_force[0], d->p.body_force[1], d->p.body_force[2] };
  assemble_elasticity_tet(d->K, d->c[1], d->c[2], d->c[0], f, d->ls.rhs.p, 0);
}

// LHS c0 M + K(c1, c2) and the whole RHS of :645-867 in one pass (set mode)
void lhs_tri(Elastodynamics* d)
{
  const double f[2] = { d->p.body_force[0], d->p.body_force[1] };
  assemble_elastodynamics_tri(d->K, d->c, f, d->U.p, d->V.p, d->A.p, d->tri.fixed2.p, d->ls.rhs.p, 0);
}

// rhs += op (a U + b V + c A)
void rhs_add_tet(Elastodynamics* d, LinearSystem& op, double a, double b, double c)
{
  Ctx& ctx = *d->ctx;
  vec_lincomb(ctx, d->n, a, d->U.p, b, d->V.p, c, d->A.p, d->tet.W.p);
  ls_spmv(op, d->tet.W.p, d->tet.MW.p);
  vec_lincomb(ctx, d->n, 1.0, d->ls.rhs.p, 1.0, d->tet.MW.p, 0.0, nullptr, d->ls.rhs.p);
}

void rhs_tet(Elastodynamics* d)
{
  const double* c = d->c;
  rhs_add_tet(d, d->tet.lsm, c[0], c[3], c[4]);  // M (c0 U + c3 V + c4 A)
  if (d->damped) {  // K(lambda = 1) (-c5 U + c7 V + c8 A) + K(2 mu = 1) (-c6 U + c9 V + c10 A)
    rhs_add_tet(d, d->tet.lsl, -c[5], c[7], c[8]);
    rhs_add_tet(d, d->tet.lsu, -c[6], c[9], c[10]);
  }
}

void rhs_tri(Elastodynamics* d)
{
  Ctx& ctx = *d->ctx;
  const Elastodynamics::Tri& s = d->tri;
  // paraxial boundaries (modules/soildynamics/FemModule.cc): the EDGE2 matrix added to the LHS
  // (:1376-1486) and the edge loop over U, V, A to the RHS (:870-936), all blocks in one launch
  if (s.par.n) {
    const double rho = d->p.rho, dt = d->p.dt, gamma = d->gamma, beta = d->beta;
    // the module's c7 .. c9 (:297-299) -- not the fused kernel's damping terms c[7 .. 10], zero here
    const double p[3] = { rho * gamma / beta / dt, rho * (1. - gamma / beta), rho * dt * (1. - gamma / (2. * beta)) };
    const double mu = 0.5 * d->mu2;  // wave speeds of E, nu or lambda, mu (:261-273) unless given (:275-278)
    const double cs = s.cs > 0 ? s.cs : std::sqrt(mu / rho);
    const double cp = s.cp > 0 ? s.cp : std::sqrt((d->lambda + 2. * mu) / rho);
    paraxial_add(ctx, s.par, cp, cs, p, d->U.p, d->V.p, d->A.p, s.fixed2.p, d->K.values.p, d->ls.rhs.p);
  }
  // tractions t_i |e| / 2 per face node on the unfixed DoFs (:880-967), at the step's time for a table
  for (const auto& tr : s.trac2) {
    double t[2] = { tr.t[0], tr.t[1] };
    if (!tr.times.empty()) table_interp(tr.times, tr.values, 2, s.t, t);
    traction2_add(ctx, (int64_t)tr.nodes.n, tr.nodes.p, tr.w.p, t, tr.mask, s.fixed2.p, d->ls.rhs.p);
  }
}

void constrain_tet(Elastodynamics* d)
{
  // clamped DoFs by penalty (the reference's default Dirichlet treatment)
  if (d->tet.fixed.n)
    ls_set_list(d->ls, d->tet.fixed.p, (int64_t)d->tet.fixed.n, AFEM_MEM_DEVICE, 0, 0.0, d->p.penalty);
  // imposed displacements: diagonal = penalty, rhs = u penalty
  // (modules/passmo/ElastodynamicModule.cc:1923-1939)
  if (d->imp_ids.n)
    ls_set_list(d->ls, d->imp_ids.p, (int64_t)d->imp_ids.n, AFEM_MEM_DEVICE, 0, 0.0, d->p.penalty, d->imp_vals.p);
}

// the deck's Dirichlet blocks in their order: later ones override earlier ones per DoF
void constrain_tri(Elastodynamics* d)
{
  for (const auto& dc : d->tri.dir2)
    ls_set_vectorial(d->ls, 2, dc.nodes.p, (int64_t)dc.nodes.n, AFEM_MEM_DEVICE, d->tri.dir_method, dc.v, dc.mask,
                     d->p.penalty);
}

// double couple (modules/soildynamics/FemModule.cc:946-987): after everything else the listed DoFs'
// RHS entries are ASSIGNED +-F, F = the source's table at the step's time
void double_couple_tri(Elastodynamics* d)
{
  if (d->tri.dc2.empty()) return;
  mark(d, d->tri.ev_dc[0]);  // timed apart: it belongs to rhs_ms, not to bc_ms
  for (const auto& dc : d->tri.dc2) {
    double F;
    table_interp(dc.times, dc.values, 1, d->tri.t, &F);
    vec_scatter_scaled(*d->ctx, (int64_t)dc.dofs.n, dc.dofs.p, dc.sign.p, F, d->ls.rhs.p);
  }
  mark(d, d->tri.ev_dc[1]);
}

void read_timing(Elastodynamics* d)
{
  float ms[5] = {};
  for (int i = 0; i < 5; ++i) AFEM_HIP(hipEventElapsedTime(&ms[i], d->ev[i], d->ev[i + 1]));
  float tot = 0.f, dc_ms = 0.f;
  AFEM_HIP(hipEventElapsedTime(&tot, d->ev[0], d->ev[5]));
  if (!d->tri.dc2.empty()) AFEM_HIP(hipEventElapsedTime(&dc_ms, d->tri.ev_dc[0], d->tri.ev_dc[1]));
  afem_step_timing& t = d->timing;
  t.assemble_ms = ms[0];
  t.rhs_ms = ms[1] + dc_ms;  // 2D: the paraxial launch, the tractions and the double-couple assignment
  t.bc_ms = ms[2] - dc_ms;
  t.solve_ms = ms[3];
  t.precond_ms = d->last.precond_ms;
  t.update_ms = ms[4];
  t.total_ms = tot;
  t.iterations = d->last.iterations;
}
}  // namespace

void dyn_step(Elastodynamics* d, afem_solve_stats* st)
{
  Ctx& ctx = *d->ctx;
  ctx.set_device();
  const bool tri = d->nb == 2;
  if (tri) check_sources_tri(d);
  ProfileCommGuard prof_guard(d->ls.opts, d->profile);  // the PCG times its preconditioner applications
  mark(d, d->ev[0]);
  if (tri)
    lhs_tri(d);
  else
    lhs_tet(d);
  mark(d, d->ev[1]);
  if (tri)
    rhs_tri(d);
  else
    rhs_tet(d);
  mark(d, d->ev[2]);
  if (tri)
    constrain_tri(d);
  else
    constrain_tet(d);
  // warm start from the Newmark predictor U + dt V + dt^2 (1/2 - beta) A
  // (the PCG's stopping target is unchanged: the zero guess's residual)
  vec_lincomb(ctx, d->n, 1.0, d->U.p, d->p.dt, d->V.p, d->p.dt * d->p.dt * (0.5 - d->beta), d->A.p, d->ls.sol.p);
  d->ls.opts.initial_guess = 1;
  if (tri) double_couple_tri(d);
  mark(d, d->ev[3]);
  ls_solve(d->ls, &d->last);
  prof_guard.restore();
  mark(d, d->ev[4]);
  // the constrained / imposed values re-applied to the solution (2D: _solve, :1416-1417; passmo: _doSolve, :2369-2371)
  if (d->imp_ids.n) vec_scatter(ctx, (int64_t)d->imp_ids.n, d->imp_ids.p, d->imp_vals.p, d->ls.sol.p);
  newmark_update(ctx, d->n, d->p.dt, d->beta, d->gamma, d->ls.sol.p, d->U.p, d->V.p, d->A.p);
  mark(d, d->ev[5]);
  ctx.sync();
  if (tri) d->tri.t += d->p.dt;  // _updateTime, :189
  if (d->profile) read_timing(d);
  if (st) *st = d->last;
}

void dyn_set_dirichlet(Elastodynamics* d, const int32_t* dofs, const double* values, int64_t n, int mem)
{
  AFEM_REQUIRE(n == 0 || (dofs && values), AFEM_ERR_ARG, "afem_elastodynamics_set_dirichlet: dofs / values is NULL");
  AFEM_REQUIRE(n >= 0, AFEM_ERR_ARG, "afem_elastodynamics_set_dirichlet: negative count");
  AFEM_REQUIRE(d->nb == 3, AFEM_ERR_NOT_IMPL,
               "afem_elastodynamics_set_dirichlet is the 3D loop's entry (2D: afem_elastodynamics_set_dirichlet_vectorial)");
  Ctx& ctx = *d->ctx;
  ctx.set_device();
  const std::vector<int32_t> hd = to_host(ctx, dofs, n, mem);
  const std::vector<double> hv = to_host(ctx, values, n, mem);
  // owned DoFs only (the reference loops over ownNodes(), :1923); the last
  // value of a DoF listed twice wins, as the module's successive conditions
  std::map<int32_t, double> m;
  for (int64_t i = 0; i < n; ++i) {
    AFEM_REQUIRE(hd[i] >= 0 && hd[i] < d->n_cols, AFEM_ERR_ARG, "imposed DoF id out of range");
    if (hd[i] < d->n) m[hd[i]] = hv[i];
  }
  std::vector<int32_t> ids;
  std::vector<double> vals;
  for (const auto& kv : m) {
    ids.push_back(kv.first);
    vals.push_back(kv.second);
  }
  upload(ctx, d->imp_ids, ids);
  upload(ctx, d->imp_vals, vals);
}

void dyn_set_time_step(Elastodynamics* d, double dt)
{
  AFEM_REQUIRE(dt > 0, AFEM_ERR_ARG, "afem_elastodynamics_set_time_step: dt must be > 0");
  if (dt == d->p.dt) return;
  d->p.dt = dt;
  dyn_coefficients(d);
  // the operator c0 M + K(c1, c2) depends on dt: a reused multigrid hierarchy
  // is rebuilt at the next solve
  d->ls.mg.reset();
  d->ls.amg.reset();
}

void dyn_profile(Elastodynamics* d, bool on)
{
  d->ctx->set_device();
  if (on && !d->ev[0]) {
    for (auto& e : d->ev) AFEM_HIP(hipEventCreate(&e));
    if (d->nb == 2)
      for (auto& e : d->tri.ev_dc) AFEM_HIP(hipEventCreate(&e));
  }
  d->profile = on;
  afem_step_timing& t = d->timing;
  t.nnz_blocks = d->K.s.nnz;
  t.n_incidences = d->K.s.n_incidences;
  t.n_nodes = d->mesh->n_nodes;
  t.n_own_nodes = d->mesh->n_own;
}

void dyn_destroy(Elastodynamics* d)
{
  if (!d) return;
  d->ctx->set_device();
  (void)hipStreamSynchronize(d->ctx->stream);
  for (auto& e : d->ev)
    if (e) (void)hipEventDestroy(e);
  if (d->ls.pinned) (void)hipHostFree(d->ls.pinned);
  if (d->nb == 2) {
    for (auto& e : d->tri.ev_dc)
      if (e) (void)hipEventDestroy(e);
  }
  else {
    for (LinearSystem* l : { &d->tet.lsm, &d->tet.lsl, &d->tet.lsu })
      if (l->pinned) (void)hipHostFree(l->pinned);
  }
  delete d;
}

}  // namespace afem
