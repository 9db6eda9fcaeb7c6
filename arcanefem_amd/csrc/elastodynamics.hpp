// The elastodynamics time loop's handle and its entry points (elastodynamics.cpp; capi.cpp wraps them).
#pragma once

#include "afem_internal.hpp"

namespace afem {

struct Elastodynamics {
  Mesh* mesh = nullptr;
  Ctx* ctx = nullptr;
  Comm* comm = nullptr;
  afem_newmark_params p{};
  double lambda = 0, mu2 = 0, gamma = 0.5, beta = 0.25;
  double c[11] = {};      // modules/elastodynamics/FemModule.cc:255-290 c0 .. c10
  bool damped = false;    // a stiffness term on the RHS (etak != 0 or alpf != 0)
  int nb = 3;             // 3: the loop on tetrahedra (tet), 2: the one on triangles (tri)
  Bsr K;                  // block-nb, per-row (CSR) layout: values = c0 M + K(c1, c2)
  LinearSystem ls;        // the solve
  DevBuf<double> U, V, A;
  DevBuf<int32_t> imp_ids;  // imposed displacements re-applied after the solve: owned DoFs
  DevBuf<double> imp_vals;  //   and their values
  int64_t n = 0, n_cols = 0;
  afem_solve_stats last{};
  // afem_elastodynamics_profile: per-phase events of every step
  bool profile = false;
  hipEvent_t ev[6] = {};
  afem_step_timing timing{};

  // nb = 3: M, K_lambda and K_mu are stored on K's structure and the RHS is built by SpMVs.
  struct Tet {
    DevBuf<double> mvals;           // consistent mass on K's structure (CSR order)
    DevBuf<double> klvals, kmvals;  // damped: K(lambda = 1, 2 mu = 0) and K(0, 1) on K's structure
    LinearSystem lsm;               // the mass operator's SpMV
    LinearSystem lsl, lsu;          // damped: the SpMVs of klvals / kmvals
    DevBuf<double> W, MW;
    DevBuf<int32_t> fixed;  // clamped DoFs
  } tet;

  // nb = 2: the 2D loop on triangles (modules/elastodynamics itself).  K is block-2; one fused
  // kernel per step writes the LHS and the complete RHS from U, V, A (assemble_elastodynamics_tri):
  // no stored M / K_lambda / K_mu, no SpMV.  The Dirichlet conditions are kept as the
  // deck's blocks (replayed in order through ls_set_vectorial every step), as flags for the
  // kernel's and the tractions' guards (fixed2) and as imp_ids / imp_vals for the re-imposition.
  struct Tri {
    double t = 0.0;  // time of the next step (FemModule.cc:175, :189)
    struct Dirichlet2 {
      DevBuf<int32_t> nodes;
      double v[2] = { 0, 0 };
      unsigned mask = 0;
    };
    std::vector<Dirichlet2> dir2;
    int dir_method = -1;  // AFEM_DIRICHLET_* of the registered conditions (-1: none yet)
    std::map<int32_t, double> dir_dofs;  // DoF -> value over all blocks, later ones overriding
    DevBuf<uint8_t> fixed2;              // [2 n_own]
    struct Traction2 {
      DevBuf<int32_t> nodes;  // the group's owned nodes, each once
      DevBuf<double> w;       // sum of |e| / 2 over the group's edges at the node
      double t[2] = { 0, 0 };
      unsigned mask = 0;
      std::vector<double> times, values;  // CaseTable (values: 2 per time); empty: constant
    };
    std::vector<Traction2> trac2;
    // modules/soildynamics on the 2D loop: the wave speeds (:261-280; 0 until a paraxial block needs
    // them), the paraxial edges of all blocks in registration order and their plan (one launch per
    // step), and the double-couple sources (:946-987): DoFs and signs uploaded once, the step
    // scales them by the table's force
    double cp = 0.0, cs = 0.0;
    std::vector<int32_t> par_faces;
    ParaxialPlan par;
    struct DoubleCouple2 {
      DevBuf<int32_t> dofs;
      DevBuf<double> sign;
      std::vector<int32_t> hdofs;
      std::vector<double> times, values;
    };
    std::vector<DoubleCouple2> dc2;
    hipEvent_t ev_dc[2] = {};  // around the double-couple assignment (counted in rhs_ms)
  } tri;
};

Elastodynamics* dyn_create(Mesh* mesh, Comm* comm, const afem_newmark_params* prm, const int32_t* fixed_nodes,
                           int64_t n_fixed, int mem);
void dyn_step(Elastodynamics* d, afem_solve_stats* st);
void dyn_set_time_step(Elastodynamics* d, double dt);
void dyn_profile(Elastodynamics* d, bool on);
void dyn_destroy(Elastodynamics* d);
// the 3D loop's registration (AFEM_ERR_NOT_IMPL on a 2D handle)
void dyn_set_dirichlet(Elastodynamics* d, const int32_t* dofs, const double* values, int64_t n, int mem);
// the 2D loop's registrations (AFEM_ERR_NOT_IMPL on a 3D handle)
void dyn_set_lame(Elastodynamics* d, double lambda, double mu);
void dyn_set_dirichlet_vectorial(Elastodynamics* d, const int32_t* nodes, int64_t n, const double values[2],
                                 unsigned mask, int method, int mem);
void dyn_set_traction(Elastodynamics* d, const int32_t* face_nodes, int64_t n_faces, const double t[2], unsigned mask,
                      int mem);
void dyn_set_traction_table(Elastodynamics* d, int index, const double* times, const double* values, int64_t n);
// modules/soildynamics on the 2D loop (AFEM_ERR_NOT_IMPL on a 3D handle, with damping or generalized-alpha)
void dyn_set_wave_speeds(Elastodynamics* d, double cp, double cs);
void dyn_set_paraxial(Elastodynamics* d, const int32_t* face_nodes, int64_t n_faces, int mem);
void dyn_set_double_couple(Elastodynamics* d, const int32_t* const nodes[4], const int64_t n_nodes[4], const double* times,
                           const double* values, int64_t n, int mem);

}  // namespace afem

struct afem_elastodynamics {
  afem::Elastodynamics* d = nullptr;
};
