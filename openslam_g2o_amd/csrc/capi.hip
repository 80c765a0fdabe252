// extern "C" surface of libg2ohip (include/g2ohip.h).  Exceptions never cross the boundary: every entry point that can
// reach a throwing call runs under guarded(), which maps failures to the reference's convention -- a return code plus
// text (the reference path itself uses `false` + cerr).  An entry that takes a handle is one
// entry(handle, body) statement: handle check, then the body under guarded().
#include "../../include/g2ohip.h"

#include <cstdlib>
#include <cstring>
#include <string>
#include <type_traits>

#include "block_solver.h"

namespace g2ohip {
std::string& last_error_ref() {
  static thread_local std::string e;
  return e;
}
}  // namespace g2ohip

using namespace g2ohip;

struct g2ohip_solver {
  std::unique_ptr<BlockSolver> impl;
};

// Narrow seam: LinearSolver<MatrixType> over the same multifrontal engine.
struct g2ohip_linear_solver {
  int bs = 0, device = 0;
  hipStream_t st = nullptr;
  std::unique_ptr<SparseCholesky> chol;
  CholOptions opt;
  std::vector<int> colptr, rowidx;  // pattern the symbolic factorisation was built for
  // a second analysis for solvePattern() on a DIFFERENT pattern between two init() calls: g2o's BlockSolver factorises
  // Hschur in solve() and hands Hpp (a sub-pattern) to solvePattern() of the same LinearSolver (block_solver.hpp:489-499)
  std::unique_ptr<SparseCholesky> chol2;
  std::vector<int> colptr2, rowidx2;
  DevBuf<double> dA, db, dx;
  EventTimer tn, tl;
  double t_numeric = 0, t_solve = 0;
};

namespace {
template <class F>
int guarded(F&& f) {
  try {
    return f();
  } catch (const ArgFailure& e) {
    set_error(e.what());
    return G2OHIP_ERR_ARG;
  } catch (const StateFailure& e) {
    set_error(e.what());
    return G2OHIP_ERR_STATE;
  } catch (const HipFailure& e) {
    set_error(e.what());
    return G2OHIP_ERR_HIP;
  } catch (const std::exception& e) {
    set_error(e.what());
    return G2OHIP_ERR_HIP;
  }
}
// an argument check of an entry body: G2OHIP_ERR_ARG with a text that names the entry
void require(bool ok, const char* what) {
  if (!ok) throw ArgFailure(what);
}
// body(target) under guarded(): a body that returns nothing yields G2OHIP_OK, one that returns int yields that value
template <class T, class F>
int run_body(T& target, F&& body) {
  return guarded([&]() -> int {
    if constexpr (std::is_void_v<decltype(body(target))>) {
      body(target);
      return G2OHIP_OK;
    } else {
      return body(target);
    }
  });
}
template <class F>
int entry(g2ohip_solver* s, F&& body) {   // body(BlockSolver&)
  if (!s || !s->impl) {
    set_error("null solver handle");
    return G2OHIP_ERR_ARG;
  }
  return run_body(*s->impl, body);
}
template <class F>
int entry(g2ohip_linear_solver* ls, F&& body) {   // body(g2ohip_linear_solver&)
  if (!ls) {
    set_error("null linear solver handle");
    return G2OHIP_ERR_ARG;
  }
  return run_body(*ls, body);
}

// the options of the factorisation (CholOptions) that both handles accept; false: not one of them
bool set_chol_option(CholOptions& o, const char* name, double value) {
  static const struct { const char* name; int CholOptions::*field; } kFields[] = {
      {"nd_leaf", &CholOptions::nd_leaf},
      {"max_sn_scalars", &CholOptions::max_sn_scalars},
      {"max_sn_scalars_lds", &CholOptions::max_sn_scalars_lds},
      {"dep_levels", &CholOptions::dep_levels},
      {"band_kernel", &CholOptions::band_kernel},
      {"tree_backward", &CholOptions::tree_backward},
      {"big_group", &CholOptions::big_group},
      {"big_group_min_rows", &CholOptions::big_group_min_rows},
      {"dep_backward", &CholOptions::dep_backward},
      {"big_front_passes", &CholOptions::big_front_passes},
      {"dep_spin_limit", &CholOptions::dep_spin_limit}};
  for (const auto& f : kFields)
    if (!std::strcmp(name, f.name)) {
      o.*f.field = (int)value;
      return true;
    }
  return false;
}
// the block solver's own options; false: not one of them
bool set_solver_option(BlockSolver& solver, const char* name, double value) {
  static const struct { const char* name; void (*set)(BlockSolver&, double); } kOptions[] = {
      {"schur_tile_bytes", [](BlockSolver& b, double v) { b.schur_tile_bytes = (size_t)v; }},
      {"comm_emulate", [](BlockSolver& b, double v) { b.comm_emulate = (int)v; }},
      {"mask_solution", [](BlockSolver& b, double v) { b.mask_solution = v != 0; }},
      {"linear_solver", [](BlockSolver& b, double v) { b.linear_solver = (int)v; }},   // 0 Cholesky, 1 PCG
      {"pcg_tolerance", [](BlockSolver& b, double v) { b.pcg_opt.tolerance = v; }},
      {"pcg_max_iterations", [](BlockSolver& b, double v) { b.pcg_opt.max_iter = (int)v; }},
      {"pcg_absolute_tolerance", [](BlockSolver& b, double v) { b.pcg_opt.absolute_tolerance = v != 0; }},
      {"pcg_check_every", [](BlockSolver& b, double v) { b.pcg_opt.check_every = std::max(1, (int)v); }},
      {"fuse_schur_reduce", [](BlockSolver& b, double v) { b.fuse_schur_reduce = v != 0; }},
      {"marginals_reduced", [](BlockSolver& b, double v) { b.marginals_reduced = v != 0; }},
      // (the next pg_linearize evaluates again, in the chosen form)
      {"pg_landmark_staged", [](BlockSolver& b, double v) { b.pg_landmark_staged = v != 0; }},
      {"ba_stereo_staged", [](BlockSolver& b, double v) { b.ba_stereo_staged = v != 0; }},   // (likewise the next ba_linearize)
      {"marginals_recursion", [](BlockSolver& b, double v) { b.marginals_recursion = v != 0; }},
      {"use_graph", [](BlockSolver& b, double v) { b.use_graph = v != 0; }},
      {"sharded_graph", [](BlockSolver& b, double v) { b.sharded_graph = (int)v; }},
      {"sharded_merge", [](BlockSolver& b, double v) { b.sharded_merge = (int)v; }},
      {"sharded_selftest", [](BlockSolver& b, double v) { b.sharded_selftest = (int)v; }},
      {"setup_overlap", [](BlockSolver& b, double v) { b.setup_overlap = v != 0; }},
      // (tests only: corrupt the first variant solve)
      {"sharded_selftest_break", [](BlockSolver& b, double v) { b.selftest_break = (int)v; }},
      {"ba_fused", [](BlockSolver& b, double v) { b.ba_fused = v != 0; }},
      {"ba_fuse_landmarks", [](BlockSolver& b, double v) { b.ba_fuse_landmarks = v != 0; }}};
  for (const auto& o : kOptions)
    if (!std::strcmp(name, o.name)) {
      o.set(solver, value);
      return true;
    }
  return false;
}

void fill_chol_stats(const CholStats* cs, g2ohip_stats* out) {
  if (!cs) return;
  out->timeSymbolicDecomposition = cs->t_symbolic;
  out->choleskyNNZ = cs->nnzL;
  out->numFronts = cs->n_fronts;
  out->numLevels = cs->n_levels;
  out->maxFrontDim = cs->max_front_dim;
  out->bandChains = cs->n_band;
  out->bandCholeskyNNZ = cs->nnzL_band;
  out->bandPivots = cs->piv_band;
  out->treeBackwardGroups = cs->n_tree_groups;
  out->choleskyFlops = cs->flops;
}

// ---- narrow seam: pattern bookkeeping
bool same_pattern(const std::vector<int>& cp, const std::vector<int>& ri, int n_blocks, const int32_t* colptr, const int32_t* rowidx) {
  return (int)cp.size() == n_blocks + 1 && std::memcmp(cp.data(), colptr, sizeof(int) * (n_blocks + 1)) == 0 && (int)ri.size() == colptr[n_blocks] &&
         std::memcmp(ri.data(), rowidx, sizeof(int) * ri.size()) == 0;
}
void analyze_into(g2ohip_linear_solver& ls, std::unique_ptr<SparseCholesky>& chol, std::vector<int>& cp, std::vector<int>& ri, int n_blocks,
                  const int32_t* colptr, const int32_t* rowidx) {
  chol = std::make_unique<SparseCholesky>(ls.bs);
  cp.assign(colptr, colptr + n_blocks + 1);
  ri.assign(rowidx, rowidx + colptr[n_blocks]);
  chol->analyze(n_blocks, colptr, rowidx, ls.opt, ls.st);
}
}  // namespace

// G2OHIP_OPTIONS="name=value,..." in the environment: options for every solver handle of the process, applied at creation
// (an explicit g2ohip_set_option afterwards still wins).  Parsed HERE so that C / C++ consumers -- the g2o plugin -- see it
// too.  A malformed entry fails the creation with G2OHIP_ERR_ARG and a message; `unknown_ok` lets the narrow-seam handle
// skip names that only the block solver knows.
template <class Setter>
static int apply_env_options(Setter&& set, bool unknown_ok) {
  const char* env = std::getenv("G2OHIP_OPTIONS");
  if (!env || !*env) return G2OHIP_OK;
  std::string all(env);
  size_t pos = 0;
  while (pos <= all.size()) {
    size_t end = all.find(',', pos);
    if (end == std::string::npos) end = all.size();
    std::string kv = all.substr(pos, end - pos);
    pos = end + 1;
    const size_t a = kv.find_first_not_of(" \t"), b = kv.find_last_not_of(" \t");
    if (a == std::string::npos) continue;
    kv = kv.substr(a, b - a + 1);
    const size_t eq = kv.find('=');
    char* stop = nullptr;
    const double v = eq == std::string::npos ? 0.0 : std::strtod(kv.c_str() + eq + 1, &stop);
    if (eq == std::string::npos || eq == 0 || stop == kv.c_str() + eq + 1 || (stop && *stop && *stop != ' ')) {
      set_error("G2OHIP_OPTIONS: malformed entry '" + kv + "' (want name=value)");
      return G2OHIP_ERR_ARG;
    }
    std::string name = kv.substr(0, eq);
    name.erase(name.find_last_not_of(" \t") + 1);
    const int rc = set(name.c_str(), v);
    if (rc != G2OHIP_OK && !unknown_ok) {
      set_error("G2OHIP_OPTIONS: unknown option '" + name + "'");
      return rc;
    }
  }
  return G2OHIP_OK;
}

extern "C" {

const char* g2ohip_last_error(void) { return last_error_ref().c_str(); }

int g2ohip_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int g2ohip_create(g2ohip_solver** out, int pose_dim, int landmark_dim, int device) {
  return guarded([&] {
    require(out, "g2ohip_create: null output");
    *out = nullptr;
    auto h = std::make_unique<g2ohip_solver>();
    h->impl = std::make_unique<BlockSolver>(pose_dim, landmark_dim, device);
    g2ohip_solver* raw = h.get();
    const int rc = apply_env_options([&](const char* n, double v) { return g2ohip_set_option(raw, n, v); }, false);
    if (rc != G2OHIP_OK) return rc;
    *out = h.release();
    return G2OHIP_OK;
  });
}

void g2ohip_destroy(g2ohip_solver* s) { delete s; }

int g2ohip_set_stream(g2ohip_solver* s, void* hip_stream) {
  return entry(s, [&](BlockSolver& b) { b.set_stream((hipStream_t)hip_stream); });
}
int g2ohip_init(g2ohip_solver* s) {
  return entry(s, [&](BlockSolver& b) { b.init(); });
}
int g2ohip_add_edge_set(g2ohip_solver* s, int error_dim, int n_edges, const int32_t* v0, const int32_t* v1) {
  return entry(s, [&](BlockSolver& b) { return b.add_edge_set(error_dim, n_edges, v0, v1); });
}
int g2ohip_set_edge_set_parts(g2ohip_solver* s, int set, int parts) {
  return entry(s, [&](BlockSolver& b) { b.set_edge_set_parts(set, parts); });
}
int g2ohip_build_structure(g2ohip_solver* s, int num_poses, int num_landmarks, int do_schur) {
  return entry(s, [&](BlockSolver& b) { b.build_structure(num_poses, num_landmarks, do_schur != 0); });
}
int g2ohip_set_edge_data(g2ohip_solver* s, int set, const double* J0, const double* J1, const double* omega, const double* err,
                         int on_device) {
  return entry(s, [&](BlockSolver& b) { b.set_edge_data(set, J0, J1, omega, err, on_device != 0); });
}
int g2ohip_set_edge_errors(g2ohip_solver* s, int set, const double* err) {
  return entry(s, [&](BlockSolver& b) { b.set_edge_errors(set, err); });
}
int g2ohip_set_robust_kernel(g2ohip_solver* s, int set, int kind, double delta) {
  return entry(s, [&](BlockSolver& b) { b.set_robust_kernel(set, kind, delta); });
}
int g2ohip_set_robust_kernel_per_edge(g2ohip_solver* s, int set, const int32_t* kind, const double* delta) {
  return entry(s, [&](BlockSolver& b) { b.set_robust_kernel_per_edge(set, kind, delta); });
}
int g2ohip_build_system(g2ohip_solver* s) {
  return entry(s, [&](BlockSolver& b) { b.build_system(); });
}
int g2ohip_chi2(g2ohip_solver* s, double* chi2) {
  return entry(s, [&](BlockSolver& b) {
    require(chi2, "g2ohip_chi2: null output");
    *chi2 = b.chi2();
  });
}
int g2ohip_set_lambda(g2ohip_solver* s, double lambda, int backup) {
  return entry(s, [&](BlockSolver& b) { b.set_lambda(lambda, backup != 0); });
}
int g2ohip_set_lambda_split(g2ohip_solver* s, double lambda_pose, double lambda_landmark, int backup) {
  return entry(s, [&](BlockSolver& b) { b.set_lambda_split(lambda_pose, lambda_landmark, backup != 0); });
}
int g2ohip_add_schur_pattern(g2ohip_solver* s, int n_blocks, const int32_t* rows, const int32_t* cols) {
  return entry(s, [&](BlockSolver& b) { b.add_schur_pattern(n_blocks, rows, cols); });
}
int g2ohip_clear_edge_sets(g2ohip_solver* s) {
  return entry(s, [&](BlockSolver& b) { b.clear_edge_sets(); });
}
int g2ohip_update_structure(g2ohip_solver* s, int num_new_poses, int set, int n_new_edges, const int32_t* v0, const int32_t* v1) {
  return entry(s, [&](BlockSolver& b) {
    if (b.update_structure(num_new_poses, set, n_new_edges, v0, v1)) return G2OHIP_OK;
    set_error("updateStructure(): Schur not supported");   // (the reference's message, block_solver.hpp:314)
    return G2OHIP_ERR_UNSUPPORTED;
  });
}
int g2ohip_restore_diagonal(g2ohip_solver* s) {
  return entry(s, [&](BlockSolver& b) { b.restore_diagonal(); });
}
int g2ohip_max_diagonal(g2ohip_solver* s, double* out) {
  return entry(s, [&](BlockSolver& b) {
    require(out, "g2ohip_max_diagonal: null output");
    *out = b.max_diagonal();
  });
}
int g2ohip_compute_scale(g2ohip_solver* s, double lambda, double* out) {
  return entry(s, [&](BlockSolver& b) {
    require(out, "g2ohip_compute_scale: null output");
    *out = b.compute_scale(lambda);
  });
}

int g2ohip_solve(g2ohip_solver* s) {
  return entry(s, [&](BlockSolver& b) { return b.solve() ? G2OHIP_NOT_PD : G2OHIP_OK; });
}
int g2ohip_solve_schur(g2ohip_solver* s) {
  return entry(s, [&](BlockSolver& b) { b.solve_schur(); });
}
int g2ohip_solve_reduced(g2ohip_solver* s) {
  return entry(s, [&](BlockSolver& b) { return b.solve_reduced() ? G2OHIP_NOT_PD : G2OHIP_OK; });
}
int g2ohip_set_partition(g2ohip_solver* s, int rank, int world) {
  return entry(s, [&](BlockSolver& b) { b.set_partition(rank, world); });
}
int g2ohip_solve_reduced_local(g2ohip_solver* s) {
  return entry(s, [&](BlockSolver& b) { b.solve_reduced_local(); });
}
int g2ohip_solve_reduced_shared(g2ohip_solver* s) {
  return entry(s, [&](BlockSolver& b) { b.solve_reduced_shared(); });
}
int g2ohip_solve_reduced_finish(g2ohip_solver* s) {
  return entry(s, [&](BlockSolver& b) { return b.solve_reduced_finish() ? G2OHIP_NOT_PD : G2OHIP_OK; });
}
int g2ohip_schur_operator_prepare(g2ohip_solver* s) {
  return entry(s, [&](BlockSolver& b) { b.schur_operator_prepare(); });
}
int g2ohip_schur_operator_apply(g2ohip_solver* s, const double* in_device, double* out_device) {
  return entry(s, [&](BlockSolver& b) {
    require(in_device && out_device, "g2ohip_schur_operator_apply: null vector");
    b.schur_operator_apply(in_device, out_device);
  });
}
int g2ohip_solve_async(g2ohip_solver* s) {
  return entry(s, [&](BlockSolver& b) { b.solve_async(); });
}
int g2ohip_trial_stats_begin(g2ohip_solver* s, double lambda) {
  return entry(s, [&](BlockSolver& b) { b.trial_stats_begin(lambda); });
}
int g2ohip_trial_stats(g2ohip_solver* s, double lambda, int* solve_ok, double* chi2, double* scale) {
  return entry(s, [&](BlockSolver& b) {
    require(solve_ok && chi2 && scale, "g2ohip_trial_stats: null output");
    b.trial_stats(lambda, solve_ok, chi2, scale);
  });
}
int g2ohip_solve_reduced_finish_async(g2ohip_solver* s) {
  return entry(s, [&](BlockSolver& b) { b.solve_reduced_finish_async(); });
}
int g2ohip_exchange_setup(g2ohip_solver* s, int n_blocks, const int32_t* block_idx, const double* block_keep, int n_poses,
                          const int32_t* pose_idx, const double* pose_keep, int n_halo, const int32_t* halo_idx, const double* halo_mine) {
  return entry(s, [&](BlockSolver& b) {
    require(!((n_blocks > 0 && (!block_idx || !block_keep)) || (n_poses > 0 && (!pose_idx || !pose_keep)) ||
              (n_halo > 0 && (!halo_idx || !halo_mine))),
            "g2ohip_exchange_setup: null array");
    b.exchange_setup(n_blocks, block_idx, block_keep, n_poses, pose_idx, pose_keep, n_halo, halo_idx, halo_mine);
  });
}
int g2ohip_exchange_pack(g2ohip_solver* s, int which) {
  return entry(s, [&](BlockSolver& b) { b.exchange_pack(which); });
}
int g2ohip_exchange_unpack(g2ohip_solver* s, int which) {
  return entry(s, [&](BlockSolver& b) { b.exchange_unpack(which); });
}
int g2ohip_exchange_status(g2ohip_solver* s) {
  return entry(s, [&](BlockSolver& b) {
    const int rc = b.exchange_status();
    return rc == 0 ? G2OHIP_OK : (rc == 2 ? G2OHIP_REPEAT : G2OHIP_NOT_PD);
  });
}
int g2ohip_get_partition(g2ohip_solver* s, int32_t* pose_owner, int32_t* block_consumer) {
  return entry(s, [&](BlockSolver& b) { b.partition_info(pose_owner, block_consumer); });
}
// Host-only: partition of the reduced system's block columns over `world` ranks (no device needed).
int g2ohip_partition_poses(const g2ohip_solver* options_from, int block_dim, int n_blocks, const int32_t* colptr, const int32_t* rowidx,
                           int world, int32_t* pose_owner, int32_t* block_consumer) {
  return guarded([&] {
    require(colptr && rowidx && pose_owner && n_blocks > 0 && world >= 1, "g2ohip_partition_poses: null array, no blocks or no ranks");
    CholOptions opt = options_from ? options_from->impl->chol_opt : CholOptions();
    opt.rank = 0;
    opt.world = world;
    const CholPlan plan = plan_cholesky(block_dim, n_blocks, colptr, rowidx, opt);
    const CholSymbolic& S = plan.sym;
    std::copy(S.pose_owner.begin(), S.pose_owner.end(), pose_owner);
    if (block_consumer) std::copy(S.block_consumer.begin(), S.block_consumer.end(), block_consumer);
    return G2OHIP_OK;
  });
}
int g2ohip_solve_back_substitute(g2ohip_solver* s) {
  return entry(s, [&](BlockSolver& b) { b.solve_back_substitute(); });
}

size_t g2ohip_vector_size(g2ohip_solver* s) { return (s && s->impl) ? s->impl->vector_size() : 0; }

int g2ohip_copy_x(g2ohip_solver* s, double* x_host) {
  return entry(s, [&](BlockSolver& b) {
    require(x_host, "g2ohip_copy_x: null output");
    b.copy_x(x_host);
  });
}
int g2ohip_copy_b(g2ohip_solver* s, double* b_host) {
  return entry(s, [&](BlockSolver& b) {
    require(b_host, "g2ohip_copy_b: null output");
    b.copy_b(b_host);
  });
}
const double* g2ohip_x_device(g2ohip_solver* s) { return (s && s->impl) ? s->impl->x_device() : nullptr; }
const double* g2ohip_b_device(g2ohip_solver* s) {   // (brings the landmark part of b up to date: kernels)
  const double* p = nullptr;
  entry(s, [&](BlockSolver& b) { p = b.b_device(); });
  return p;
}

int g2ohip_multiply_hessian(g2ohip_solver* s, double* dest_host, const double* src_host) {
  return entry(s, [&](BlockSolver& b) {
    require(dest_host && src_host, "g2ohip_multiply_hessian: null vector");
    b.multiply_hessian(dest_host, src_host);
  });
}
int g2ohip_sync(g2ohip_solver* s) {
  return entry(s, [&](BlockSolver& b) { b.sync(); });
}

int g2ohip_set_profiling(g2ohip_solver* s, int enabled) {
  return entry(s, [&](BlockSolver& b) {
    // 0: off; 1: every kernel slot + the stage timers of g2ohip_get_stats; 2 + k: kernel slot k only
    b.profiling = enabled == 1;
    b.prof.enabled = enabled != 0;
    b.prof.only = enabled >= 2 ? enabled - 2 : -1;
  });
}
int g2ohip_kernel_time(g2ohip_solver* s, int slot, double* total_seconds, long* launches, int reset) {
  return entry(s, [&](BlockSolver& b) {
    require(slot >= 0 && slot < KernelProf::kNumSlots && total_seconds && launches, "g2ohip_kernel_time: bad slot or null output");
    b.prof.collect();
    *total_seconds = b.prof.total[slot];
    *launches = b.prof.launches[slot];
    if (reset) {
      b.prof.total[slot] = 0;
      b.prof.launches[slot] = 0;
    }
  });
}
const char* g2ohip_kernel_name(int slot) { return KernelProf::name(slot); }
int g2ohip_kernel_slots(void) { return KernelProf::kNumSlots; }

int g2ohip_get_stats(g2ohip_solver* s, g2ohip_stats* out) {
  return entry(s, [&](BlockSolver& b) {
    require(out, "g2ohip_get_stats: null output");
    std::memset(out, 0, sizeof(*out));
    out->timeQuadraticForm = b.times.quadratic;
    out->timeSchurComplement = b.times.schur;
    out->timeNumericDecomposition = b.times.numeric;
    out->timeLinearSolution = b.times.linsolve;
    out->timeLinearSolver = b.times.numeric + b.times.linsolve;
    out->timeBackSubstitution = b.times.backsub;
    out->hessianPoseDimension = (size_t)b.nP() * b.p();
    out->hessianLandmarkDimension = (size_t)b.nL() * b.l();
    out->hessianDimension = out->hessianPoseDimension + out->hessianLandmarkDimension;
    fill_chol_stats(b.chol_stats(), out);
    out->iterationsLinearSolver = (size_t)b.pcg_iterations;
    out->timeResiduals = b.times.residuals;
    out->timeLinearize = b.times.linearize;
    out->timeUpdate = b.times.update;
    out->dependencyFallbacks = b.dependency_fallbacks;
    out->shardedCollectives = b.sharded_collectives;
  });
}

int g2ohip_set_option(g2ohip_solver* s, const char* name, double value) {
  return entry(s, [&](BlockSolver& b) {
    require(name, "g2ohip_set_option: null name");
    if (!set_chol_option(b.chol_opt, name, value) && !set_solver_option(b, name, value)) throw ArgFailure(std::string("unknown option ") + name);
    b.invalidate_graphs();   // options change kernel arguments / launch shapes
  });
}

int g2ohip_get_nnzb(g2ohip_solver* s, int which, int* nnzb) {
  return entry(s, [&](BlockSolver& b) {
    require(nnzb, "g2ohip_get_nnzb: null output");
    *nnzb = b.nnzb(which);
  });
}
int g2ohip_get_pattern(g2ohip_solver* s, int which, int32_t* colptr, int32_t* rowidx) {
  return entry(s, [&](BlockSolver& b) {
    require(colptr && rowidx, "g2ohip_get_pattern: null output");
    b.get_pattern(which, colptr, rowidx);
  });
}
int g2ohip_copy_values(g2ohip_solver* s, int which, double* values_host) {
  return entry(s, [&](BlockSolver& b) {
    require(values_host, "g2ohip_copy_values: null output");
    b.copy_values(which, values_host);
  });
}
int g2ohip_device_array(g2ohip_solver* s, int which, double** ptr, size_t* count) {
  return entry(s, [&](BlockSolver& b) {
    require(ptr && count, "g2ohip_device_array: null output");
    b.device_array(which, ptr, count);
  });
}

// ---- page-locked host buffers -------------------------------------------------------------
int g2ohip_host_register(g2ohip_solver* s, void* ptr, size_t bytes) {
  return entry(s, [&](BlockSolver&) {
    require(ptr && bytes, "g2ohip_host_register: null or empty buffer");
    G2OHIP_HIP_CHECK(hipHostRegister(ptr, bytes, hipHostRegisterDefault));
  });
}
int g2ohip_host_unregister(g2ohip_solver* s, void* ptr) {
  return entry(s, [&](BlockSolver&) {
    require(ptr, "g2ohip_host_unregister: null buffer");
    G2OHIP_HIP_CHECK(hipHostUnregister(ptr));
  });
}

// ---- device-resident bundle-adjustment front end ---------------------------------------
int g2ohip_ba_set_edges(g2ohip_solver* s, int set, const int32_t* cam_vertex, const int32_t* point_vertex, const double* meas,
                        const double* info, double f, double cx, double cy) {
  return entry(s, [&](BlockSolver& b) { b.ba_set_edges(set, cam_vertex, point_vertex, meas, info, f, cx, cy); });
}
int g2ohip_ba_set_edges_classes(g2ohip_solver* s, int set, const int32_t* cam_vertex, const int32_t* point_vertex, const double* meas,
                                const double* info, int n_classes, const double* class_params, const int32_t* edge_class) {
  return entry(s, [&](BlockSolver& b) {
    require(n_classes >= 1 && class_params, "ba_set_edges_classes: at least one class with its parameters");
    b.ba_set_edges_classes(set, cam_vertex, point_vertex, meas, info, class_params[0], class_params[1], class_params[2], n_classes, class_params,
                           edge_class);
    if (n_classes == 1) b.set_robust_kernel(set, (int)class_params[3], class_params[4]);
  });
}
int g2ohip_ba_set_stereo_edges(g2ohip_solver* s, int set, const int32_t* cam_vertex, const int32_t* point_vertex, const double* meas,
                               const double* info, double focal_length, double cx, double cy, double baseline) {
  return entry(s, [&](BlockSolver& b) { b.ba_set_stereo_edges(set, cam_vertex, point_vertex, meas, info, focal_length, cx, cy, baseline); });
}
int g2ohip_ba_set_pose_edges(g2ohip_solver* s, int set, const int32_t* vi, const int32_t* vj, const double* meas, const double* info) {
  return entry(s, [&](BlockSolver& b) { b.ba_set_pose_edges(set, vi, vj, meas, info); });
}
int g2ohip_ba_set_inverse_depth_edges(g2ohip_solver* s, int set_point_pose, int set_point_anchor, int set_pose_anchor,
                                      const int32_t* cam_vertex, const int32_t* anchor_vertex, const int32_t* point_vertex,
                                      const double* meas, const double* info, double focal_length, double cx, double cy) {
  return entry(s, [&](BlockSolver& b) {
    b.ba_set_inverse_depth_edges(set_point_pose, set_point_anchor, set_pose_anchor, cam_vertex, anchor_vertex, point_vertex, meas, info,
                                 focal_length, cx, cy);
  });
}
int g2ohip_ba_set_estimates(g2ohip_solver* s, int n_cams, const double* cams, const int32_t* cam_hidx, int n_points,
                            const double* points, const int32_t* point_hidx) {
  return entry(s, [&](BlockSolver& b) { b.ba_set_estimates(n_cams, cams, cam_hidx, n_points, points, point_hidx); });
}
int g2ohip_ba_get_estimates(g2ohip_solver* s, double* cams, double* points) {
  return entry(s, [&](BlockSolver& b) { b.ba_get_estimates(cams, points); });
}
int g2ohip_ba_get_estimates_of(g2ohip_solver* s, int n_cams, const int32_t* cam_index, double* cams, int n_points, const int32_t* point_index,
                               double* points) {
  return entry(s, [&](BlockSolver& b) { b.ba_get_estimates_of(n_cams, cam_index, cams, n_points, point_index, points); });
}
int g2ohip_ba_fetch_estimates_begin(g2ohip_solver* s, double* cams, double* points, int point_pieces) {
  return entry(s, [&](BlockSolver& b) { b.ba_fetch_begin(cams, points, point_pieces); });
}
int g2ohip_ba_fetch_estimates_wait(g2ohip_solver* s, int piece) {
  return entry(s, [&](BlockSolver& b) { b.ba_fetch_wait(piece); });
}
int g2ohip_ba_linearize(g2ohip_solver* s, int jacobians) {
  return entry(s, [&](BlockSolver& b) { b.ba_linearize(jacobians != 0); });
}
int g2ohip_ba_update(g2ohip_solver* s) {
  return entry(s, [&](BlockSolver& b) { b.ba_update(); });
}
int g2ohip_ba_structure_only(g2ohip_solver* s, int num_iters, int num_max_trials, int32_t* point_trace, double* point_chi2) {
  return entry(s, [&](BlockSolver& b) { b.ba_structure_only(num_iters, num_max_trials, point_trace, point_chi2); });
}
int g2ohip_ba_push(g2ohip_solver* s) {
  return entry(s, [&](BlockSolver& b) { b.ba_push(); });
}
int g2ohip_ba_pop(g2ohip_solver* s) {
  return entry(s, [&](BlockSolver& b) { b.ba_pop(); });
}
int g2ohip_ba_discard_top(g2ohip_solver* s) {
  return entry(s, [&](BlockSolver& b) { b.ba_discard_top(); });
}

// ---- collectives inside the library, the sharded solve ------------------------------------
int g2ohip_comm_unique_id(char* id128) {
  return guarded([&] {
    require(id128, "g2ohip_comm_unique_id: null output");
    Comm::unique_id(id128);
    return G2OHIP_OK;
  });
}
int g2ohip_comm_init_rccl(g2ohip_solver* s, int rank, int world, const char* id128) {
  return entry(s, [&](BlockSolver& b) {
    require(id128 && world >= 1 && rank >= 0 && rank < world, "g2ohip_comm_init_rccl: null id or rank outside [0, world)");
    b.comm_init_rccl(rank, world, id128);
  });
}
int g2ohip_comm_init_host(g2ohip_solver* s, int rank, int world, g2ohip_host_allreduce_fn fn, void* ctx) {
  return entry(s, [&](BlockSolver& b) {
    require(fn && world >= 1 && rank >= 0 && rank < world, "g2ohip_comm_init_host: null callback or rank outside [0, world)");
    b.comm.init_host(rank, world, fn, ctx);
  });
}
int g2ohip_comm_init_peer(g2ohip_solver* s, int rank, int world, g2ohip_host_allreduce_fn fn, void* ctx, size_t slot_doubles) {
  return entry(s, [&](BlockSolver& b) {
    require(fn && world >= 1 && rank >= 0 && rank < world, "g2ohip_comm_init_peer: null callback or rank outside [0, world)");
    b.comm_init_peer(rank, world, fn, ctx, slot_doubles);
  });
}
int g2ohip_comm_destroy(g2ohip_solver* s) {
  return entry(s, [&](BlockSolver& b) { b.comm.destroy(); });
}
int g2ohip_comm_all_reduce(g2ohip_solver* s, double* device_buffer, size_t count, int op) {
  return entry(s, [&](BlockSolver& b) {
    require(!count || device_buffer, "g2ohip_comm_all_reduce: null buffer");
    b.comm_all_reduce(device_buffer, count, op);
  });
}
int g2ohip_solve_sharded(g2ohip_solver* s) {
  return entry(s, [&](BlockSolver& b) { return b.solve_sharded() ? G2OHIP_NOT_PD : G2OHIP_OK; });
}
int g2ohip_chi2_sharded(g2ohip_solver* s, double* chi2) {
  return entry(s, [&](BlockSolver& b) {
    require(chi2, "g2ohip_chi2_sharded: null output");
    *chi2 = b.chi2_sharded();
  });
}
int g2ohip_max_diagonal_sharded(g2ohip_solver* s, double* out) {
  return entry(s, [&](BlockSolver& b) {
    require(out, "g2ohip_max_diagonal_sharded: null output");
    *out = b.max_diagonal_sharded();
  });
}
int g2ohip_compute_scale_sharded(g2ohip_solver* s, double lambda, double* out) {
  return entry(s, [&](BlockSolver& b) {
    require(out, "g2ohip_compute_scale_sharded: null output");
    *out = b.compute_scale_sharded(lambda);
  });
}
int g2ohip_copy_diagonal(g2ohip_solver* s, double* diag_host) {
  return entry(s, [&](BlockSolver& b) { b.copy_diagonal(diag_host); });
}
int g2ohip_compute_marginals(g2ohip_solver* s, int n_blocks, const int32_t* rows, const int32_t* cols, double* out) {
  return entry(s, [&](BlockSolver& b) { return b.compute_marginals(n_blocks, rows, cols, out) ? G2OHIP_NOT_PD : G2OHIP_OK; });
}
int g2ohip_set_x(g2ohip_solver* s, const double* x_host) {
  return entry(s, [&](BlockSolver& b) { b.set_x(x_host); });
}
int g2ohip_copy_edge_data(g2ohip_solver* s, int set, double* J0, double* J1, double* err) {
  return entry(s, [&](BlockSolver& b) { b.copy_edge_data(set, J0, J1, err); });
}

// ---- device-resident pose-graph front end, its landmark half ------------------------------
int g2ohip_pg_set_edges(g2ohip_solver* s, int set, int type, const int32_t* vi, const int32_t* vj, const double* meas,
                        const double* info) {
  return entry(s, [&](BlockSolver& b) { b.pg_set_edges(set, type, vi, vj, meas, info); });
}
int g2ohip_pg_set_sim3_fix_scale(g2ohip_solver* s, int fix_scale) {
  return entry(s, [&](BlockSolver& b) { b.pg_set_sim3_fix_scale(fix_scale != 0); });
}
int g2ohip_pg_set_estimates(g2ohip_solver* s, int n_vertices, const double* poses, const int32_t* hidx) {
  return entry(s, [&](BlockSolver& b) { b.pg_set_estimates(n_vertices, poses, hidx); });
}
int g2ohip_pg_get_estimates(g2ohip_solver* s, double* poses) {
  return entry(s, [&](BlockSolver& b) {
    require(poses, "g2ohip_pg_get_estimates: null output");
    b.pg_get_estimates(poses);
  });
}
int g2ohip_pg_linearize(g2ohip_solver* s, int jacobians) {
  return entry(s, [&](BlockSolver& b) { b.pg_linearize(jacobians != 0); });
}
int g2ohip_pg_update(g2ohip_solver* s) {
  return entry(s, [&](BlockSolver& b) { b.pg_update(); });
}
int g2ohip_pg_push(g2ohip_solver* s) {
  return entry(s, [&](BlockSolver& b) { b.pg_push(); });
}
int g2ohip_pg_pop(g2ohip_solver* s) {
  return entry(s, [&](BlockSolver& b) { b.pg_pop(); });
}
int g2ohip_pg_discard_top(g2ohip_solver* s) {
  return entry(s, [&](BlockSolver& b) { b.pg_discard_top(); });
}
int g2ohip_pg_set_landmark_edges(g2ohip_solver* s, int set, int type, const int32_t* pose_vertex, const int32_t* point_vertex,
                                 const double* meas, const double* info, const double* offset) {
  return entry(s, [&](BlockSolver& b) { b.pg_set_landmark_edges(set, type, pose_vertex, point_vertex, meas, info, offset); });
}
int g2ohip_pg_set_landmark_camera_edges(g2ohip_solver* s, int set, int type, const int32_t* pose_vertex, const int32_t* point_vertex,
                                        const double* meas, const double* info, const double* offset, const double* kcam) {
  return entry(s, [&](BlockSolver& b) { b.pg_set_landmark_camera_edges(set, type, pose_vertex, point_vertex, meas, info, offset, kcam); });
}
int g2ohip_pg_set_sim3_project_edges(g2ohip_solver* s, int set, const int32_t* pose_vertex, const int32_t* point_vertex, const double* meas,
                                     const double* info, int n_cams, const double* intrinsics) {
  return entry(s, [&](BlockSolver& b) { b.pg_set_sim3_project_edges(set, pose_vertex, point_vertex, meas, info, n_cams, intrinsics); });
}
int g2ohip_pg_set_cam_project_edges(g2ohip_solver* s, int set, int type, const int32_t* pose_vertex, const int32_t* point_vertex,
                                    const double* meas, const double* info, int n_cams, const double* intrinsics) {
  return entry(s, [&](BlockSolver& b) { b.pg_set_cam_project_edges(set, type, pose_vertex, point_vertex, meas, info, n_cams, intrinsics); });
}
int g2ohip_pg_set_prior_edges(g2ohip_solver* s, int set, int type, const int32_t* pose_vertex, const double* meas, const double* info,
                              const double* offset) {
  return entry(s, [&](BlockSolver& b) { b.pg_set_prior_edges(set, type, pose_vertex, meas, info, offset); });
}
int g2ohip_pg_set_gicp_edges(g2ohip_solver* s, int set, const int32_t* vi, const int32_t* vj, const double* meas, const double* info,
                             const double* cov) {
  return entry(s, [&](BlockSolver& b) { b.pg_set_gicp_edges(set, vi, vj, meas, info, cov); });
}
int g2ohip_pg_set_offset_edges(g2ohip_solver* s, int set, int type, const int32_t* vi, const int32_t* vj, const int32_t* param_from,
                               const int32_t* param_to, const double* meas, const double* info, int n_params, const double* offsets) {
  return entry(s, [&](BlockSolver& b) { b.pg_set_offset_edges(set, type, vi, vj, param_from, param_to, meas, info, n_params, offsets); });
}
int g2ohip_pg_set_scam_edges(g2ohip_solver* s, int set, const int32_t* pose_vertex, const int32_t* point_vertex, const double* meas,
                             const double* info, const double* kcam) {
  return entry(s, [&](BlockSolver& b) { b.pg_set_scam_edges(set, pose_vertex, point_vertex, meas, info, kcam); });
}
int g2ohip_pg_set_bearing_edges(g2ohip_solver* s, int set, const int32_t* pose_vertex, const int32_t* point_vertex, const double* meas,
                                const double* info) {
  return entry(s, [&](BlockSolver& b) { b.pg_set_bearing_edges(set, pose_vertex, point_vertex, meas, info); });
}
int g2ohip_pg_set_sensor_calib_edges(g2ohip_solver* s, int set_ij, int set_il, int set_jl, const int32_t* vi, const int32_t* vj,
                                     const int32_t* vl, const double* meas, const double* info) {
  return entry(s, [&](BlockSolver& b) { b.pg_set_sensor_calib_edges(set_ij, set_il, set_jl, vi, vj, vl, meas, info); });
}
int g2ohip_pg_set_pointxy_calib_edges(g2ohip_solver* s, int set_pl, int set_pc, int set_lc, const int32_t* pose_vertex,
                                      const int32_t* point_vertex, const int32_t* calib_vertex, const double* meas, const double* info) {
  return entry(s, [&](BlockSolver& b) { b.pg_set_pointxy_calib_edges(set_pl, set_pc, set_lc, pose_vertex, point_vertex, calib_vertex, meas, info); });
}
int g2ohip_pg_set_odom_calib_edges(g2ohip_solver* s, int set_ij, int set_ip, int set_jp, const int32_t* vi, const int32_t* vj,
                                   const int32_t* vp, const double* meas, const double* info) {
  return entry(s, [&](BlockSolver& b) { b.pg_set_odom_calib_edges(set_ij, set_ip, set_jp, vi, vj, vp, meas, info); });
}
int g2ohip_pg_set_cam_edges(g2ohip_solver* s, int set, int type, const int32_t* vi, const int32_t* vj, const double* meas,
                            const double* info) {
  return entry(s, [&](BlockSolver& b) { b.pg_set_cam_edges(set, type, vi, vj, meas, info); });
}
int g2ohip_pg_set_landmark_estimates(g2ohip_solver* s, int n_points, const double* points, const int32_t* hidx) {
  return entry(s, [&](BlockSolver& b) { b.pg_set_landmark_estimates(n_points, points, hidx); });
}
int g2ohip_pg_get_landmark_estimates(g2ohip_solver* s, double* points) {
  return entry(s, [&](BlockSolver& b) {
    require(points, "g2ohip_pg_get_landmark_estimates: null output");
    b.pg_get_landmark_estimates(points);
  });
}

// ---- narrow seam ---------------------------------------------------------------------
int g2ohip_ls_create(g2ohip_linear_solver** out, int block_dim, int device) {
  return guarded([&] {
    require(out, "g2ohip_ls_create: null output");
    *out = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) throw HipFailure("no HIP device available: libg2ohip has no CPU fallback");
    if (device < 0 || device >= count) throw ArgFailure("bad device ordinal");
    if (!(block_dim == 3 || block_dim == 6 || block_dim == 7)) throw ArgFailure("block_dim must be 3, 6 or 7");
    auto h = std::make_unique<g2ohip_linear_solver>();
    h->bs = block_dim;
    h->device = device;
    G2OHIP_HIP_CHECK(hipSetDevice(device));
    G2OHIP_HIP_CHECK(hipStreamCreate(&h->st));
    g2ohip_linear_solver* raw = h.get();
    const int rc = apply_env_options([&](const char* n, double v) { return g2ohip_ls_set_option(raw, n, v); }, true);
    if (rc != G2OHIP_OK) {
      (void)hipStreamDestroy(h->st);
      return rc;
    }
    *out = h.release();
    return G2OHIP_OK;
  });
}
void g2ohip_ls_destroy(g2ohip_linear_solver* ls) {
  if (!ls) return;
  if (ls->st) (void)hipStreamDestroy(ls->st);
  delete ls;
}
int g2ohip_ls_init(g2ohip_linear_solver* ls) {
  return entry(ls, [&](g2ohip_linear_solver& l) {
    l.chol.reset();
    l.colptr.clear();
    l.rowidx.clear();
    l.chol2.reset();
    l.colptr2.clear();
    l.rowidx2.clear();
  });
}
int g2ohip_ls_solve(g2ohip_linear_solver* ls, int n_blocks, const int32_t* colptr, const int32_t* rowidx, const double* values,
                    double* x, const double* b) {
  return entry(ls, [&](g2ohip_linear_solver& l) {
    require(colptr && rowidx && values && x && b && n_blocks > 0, "g2ohip_ls_solve: null array or no blocks");
    G2OHIP_HIP_CHECK(hipSetDevice(l.device));
    const int nnzb = colptr[n_blocks];
    const int bs = l.bs;
    // first call after init(): symbolic factorisation (linear_solver_csparse.h:110-112).  The pattern has to stay the same
    // until the next init() (linear_solver.h:86-105); a different one is analysed anew instead of being factorised with a
    // stale structure
    if (!l.chol || !same_pattern(l.colptr, l.rowidx, n_blocks, colptr, rowidx)) analyze_into(l, l.chol, l.colptr, l.rowidx, n_blocks, colptr, rowidx);
    const size_t n = (size_t)n_blocks * bs;
    l.dA.upload(values, (size_t)nnzb * bs * bs, l.st);
    l.db.upload(b, n, l.st);
    l.dx.alloc(n);
    // the status is read behind the solve: one synchronisation (a repeat runs both again; the timers keep the first run)
    const bool ok = l.chol->factor_checked([&](bool again) {
      if (!again) l.tn.start(l.st);
      l.chol->factor(l.dA.p, l.st);
      if (!again) {
        l.tn.stop(l.st);
        l.tl.start(l.st);
      }
      l.chol->solve(l.db.p, l.dx.p, l.st);
      if (!again) l.tl.stop(l.st);
    }, l.st);
    l.t_numeric = l.tn.seconds();
    l.t_solve = l.tl.seconds();
    if (!ok) return G2OHIP_NOT_PD;
    l.dx.download(x, n, l.st);
    return G2OHIP_OK;
  });
}
int g2ohip_ls_solve_pattern(g2ohip_linear_solver* ls, int n_blocks, const int32_t* colptr, const int32_t* rowidx, const double* values,
                            int n_req, const int32_t* rows, const int32_t* cols, double* out) {
  return entry(ls, [&](g2ohip_linear_solver& l) {
    require(colptr && rowidx && values && n_blocks > 0 && n_req >= 0 && (n_req == 0 || (rows && cols && out)),
            "g2ohip_ls_solve_pattern: null array, no blocks or a negative count");
    for (int i = 0; i < n_req; ++i)
      require(rows[i] >= 0 && rows[i] < n_blocks && cols[i] >= 0 && cols[i] < n_blocks, "g2ohip_ls_solve_pattern: block index out of range");
    G2OHIP_HIP_CHECK(hipSetDevice(l.device));
    const int nnzb = colptr[n_blocks];
    const int bs = l.bs;
    // the pattern of solve() -> its analysis; another pattern (BlockSolver::computeMarginals hands Hpp to the LinearSolver
    // that factorised Hschur, without init(): block_solver.hpp:489-499) -> a second analysis kept next to it
    SparseCholesky* ch = nullptr;
    if (!l.chol) analyze_into(l, l.chol, l.colptr, l.rowidx, n_blocks, colptr, rowidx);
    if (same_pattern(l.colptr, l.rowidx, n_blocks, colptr, rowidx)) {
      ch = l.chol.get();
    } else {
      if (!l.chol2 || !same_pattern(l.colptr2, l.rowidx2, n_blocks, colptr, rowidx)) analyze_into(l, l.chol2, l.colptr2, l.rowidx2, n_blocks, colptr, rowidx);
      ch = l.chol2.get();
    }
    l.dA.upload(values, (size_t)nnzb * bs * bs, l.st);
    if (!ch->factor_checked([&](bool) { ch->factor(l.dA.p, l.st); }, l.st)) return G2OHIP_NOT_PD;
    ch->inverse_blocks(n_req, rows, cols, out, true, l.st);
    return G2OHIP_OK;
  });
}
int g2ohip_ls_get_stats(g2ohip_linear_solver* ls, g2ohip_stats* out) {
  return entry(ls, [&](g2ohip_linear_solver& l) {
    require(out, "g2ohip_ls_get_stats: null output");
    std::memset(out, 0, sizeof(*out));
    if (l.chol) fill_chol_stats(&l.chol->stats(), out);
    out->timeNumericDecomposition = l.t_numeric;
    out->timeLinearSolution = l.t_solve;
    out->timeLinearSolver = l.t_numeric + l.t_solve;
  });
}
int g2ohip_ls_set_option(g2ohip_linear_solver* ls, const char* name, double value) {
  return entry(ls, [&](g2ohip_linear_solver& l) {
    require(name, "g2ohip_ls_set_option: null name");
    if (!set_chol_option(l.opt, name, value)) throw ArgFailure(std::string("unknown option ") + name);
  });
}

}  // extern "C"
