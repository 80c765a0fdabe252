/* g2ohip.h -- C ABI of the MI355X-native sparse block solver for g2o's GN/LM inner loop.
 *
 * Drop-in boundary for g2o's BlockSolver<p,l> path.  Two seams:
 *
 *   wide seam   g2o::Solver            /root/reference/g2o/core/solver.h:44-149
 *               g2o::BlockSolver<T>    /root/reference/g2o/core/block_solver.h:98-178
 *   narrow seam g2o::LinearSolver<M>   /root/reference/g2o/core/linear_solver.h:40-81
 *
 * Every entry point below names the reference member it replaces.  Plain C, plain
 * pointers and sizes, no C++/Eigen/torch types.  All matrices are fp64, all indices int32
 * (the reference's hessianIndex / csi=int, EXTERNAL/csparse/cs.h:26).  Dense blocks are
 * column-major like Eigen's default (config.h.in:16-20).
 *
 * Threading: a handle is not thread-safe; all calls for one handle must come from one
 * thread (the thread that calls SparseOptimizer::optimize()).  Errors are
 * reported by return code (the reference path uses no exceptions); g2ohip_last_error()
 * gives the text.  The library never falls back to a CPU path: without a usable HIP
 * device every compute call returns G2OHIP_ERR_HIP.
 */
#ifndef G2OHIP_H
#define G2OHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define G2OHIP_OK 0
#define G2OHIP_NOT_PD 1            /* Cholesky hit a pivot <= 0: solve() == false (csparse_helper.cpp:136) */
#define G2OHIP_REPEAT 2            /* phased sharded solve only (g2ohip_exchange_status): a rank's dependency-driven launch gave
                                      up waiting; run the phases of this solve again on EVERY rank (g2ohip_solve_sharded does) */
#define G2OHIP_ERR_ARG (-1)
#define G2OHIP_ERR_HIP (-2)
#define G2OHIP_ERR_STATE (-3)
#define G2OHIP_ERR_UNSUPPORTED (-4)

#define G2OHIP_KERNEL_NONE 0
#define G2OHIP_KERNEL_HUBER 1      /* RobustKernelHuber, g2o/core/robust_kernel_impl.cpp:65-78 */
#define G2OHIP_KERNEL_PSEUDOHUBER 2 /* RobustKernelPseudoHuber :80-89 */
#define G2OHIP_KERNEL_CAUCHY 3     /* RobustKernelCauchy :91-99 */
#define G2OHIP_KERNEL_SATURATED 4  /* RobustKernelSaturated :101-113 */
#define G2OHIP_KERNEL_DCS 5        /* RobustKernelDCS :116-126 (delta = phi) */

/* which-matrix selectors for the inspection calls */
#define G2OHIP_HPP 0
#define G2OHIP_HPL 1
#define G2OHIP_HLL 2
#define G2OHIP_HSCHUR 3
#define G2OHIP_DINV 4

typedef struct g2ohip_solver g2ohip_solver;
typedef struct g2ohip_linear_solver g2ohip_linear_solver;

/* Per-call timing/size record; same fields as G2OBatchStatistics (g2o/core/batch_stats.h:40-77)
 * so `g2o -stats` columns line up.  Times in seconds, measured with HIP events on the
 * solver's stream (only filled while profiling is enabled, see g2ohip_set_profiling). */
typedef struct g2ohip_stats {
  double timeQuadraticForm;          /* buildSystem                          */
  double timeSchurComplement;        /* K5-K8                                */
  double timeSymbolicDecomposition;  /* host ordering + symbolic, last build */
  double timeNumericDecomposition;   /* multifrontal factorisation           */
  double timeLinearSolution;         /* triangular solves                    */
  double timeLinearSolver;           /* numeric + solves                     */
  double timeBackSubstitution;       /* landmark back-substitution           */
  size_t hessianDimension, hessianPoseDimension, hessianLandmarkDimension;
  size_t choleskyNNZ;                /* scalar nnz(L)                        */
  size_t numFronts, numLevels, maxFrontDim;
  size_t iterationsLinearSolver;     /* PCG iterations of the last solve (G2OBatchStatistics::iterationsLinearSolver) */
  double timeResiduals;              /* device front end: last error-only evaluation (computeActiveErrors)   */
  double timeLinearize;              /* device front end: last error + Jacobian evaluation                   */
  double timeUpdate;                 /* device front end: last oplus over all vertices (SparseOptimizer::update) */
  size_t dependencyFallbacks;        /* dependency-driven launches that gave up waiting and were repeated level by level (0 expected) */
  size_t bandChains;                 /* leaf chains of the elimination tree factorised by the sliding-window band kernel */
  size_t bandCholeskyNNZ, bandPivots; /* ... their share of choleskyNNZ and of the pivot columns (scalars) */
  size_t shardedCollectives;         /* all-reduces of the last g2ohip_solve_sharded (2 with option sharded_merge where the partition allows, else 3) */
  size_t treeBackwardGroups;         /* groups of fronts (one workgroup each) that sweep the tree levels backward (option tree_backward; 0: task by task) */
  double choleskyFlops;              /* floating-point operations of one numeric factorisation (dense-front count of the symbolic analysis: sum over the fronts of npiv m^2 - npiv^2 m + npiv^3 / 3) */
} g2ohip_stats;
/* (G2OBatchStatistics::timeIteration / levenbergIterations / chi2 belong to the caller's optimisation loop:
 *  openslam_g2o_amd/lm.py fills them and prints the `g2o -stats` line, batch_stats.cpp:49-82.) */

const char* g2ohip_last_error(void);
int g2ohip_device_count(void);

/* ---- wide seam: g2o::BlockSolver<BlockSolverTraits<pose_dim, landmark_dim>> ------------- */

/* BlockSolver(LinearSolverType*) ctor, block_solver.h:116-120.  device = HIP ordinal. */
int g2ohip_create(g2ohip_solver** out, int pose_dim, int landmark_dim, int device);
/* ~BlockSolver, block_solver.hpp:135-140 */
void g2ohip_destroy(g2ohip_solver* s);
/* Optional: run on a caller-owned hipStream_t (e.g. torch's current stream).  NULL = own stream. */
int g2ohip_set_stream(g2ohip_solver* s, void* hip_stream);

/* Solver::init(optimizer, online), block_solver.hpp:606-620: forget numeric + symbolic state. */
int g2ohip_init(g2ohip_solver* s);

/* Graph topology, replacing the walk over activeEdges() in buildStructure
 * (block_solver.hpp:206-254).  One call per homogeneous edge type ("edge set"): all edges
 * of a set share error_dim and the vertex classes of their two sides.
 *   v0, v1: hessianIndex of vertex 0 / vertex 1 in indexMapping order
 *           (sparse_optimizer.cpp:166-190): poses are [0, num_poses), landmarks
 *           [num_poses, num_poses+num_landmarks), -1 = fixed vertex.
 *   v1 == NULL: unary edges (BaseUnaryEdge, base_unary_edge.hpp:42-72).
 * Returns the set id (>= 0) or an error code (< 0).  Must precede g2ohip_build_structure. */
int g2ohip_add_edge_set(g2ohip_solver* s, int error_dim, int n_edges, const int32_t* v0, const int32_t* v1);
/* n-ary edges (BaseMultiEdge::constructQuadraticForm, base_multi_edge.hpp:170-222: H_ii and b_i once per vertex, H_ij once per
 * pair i < j, the robust weight of the edge on all of them): ONE binary edge set per vertex pair (i, j) of the edges, each handed
 * the pair's two Jacobians and the edges' information / error / robust kernel, with the parts another pair already contributes
 * switched off -- G2OHIP_PART_NO_VERTEX0 / _NO_VERTEX1: no diagonal block and no right-hand side for that side of the set,
 * G2OHIP_PART_NO_CHI2: the set's edges are not counted in g2ohip_chi2 / g2ohip_trial_stats.  E.g. three vertices: pair (0, 1)
 * whole, pair (0, 2) with NO_VERTEX0 | NO_VERTEX1 | NO_CHI2, pair (1, 2) with NO_VERTEX0 | NO_CHI2 (vertex 2's own terms).  Generic path on one GPU;
 * before g2ohip_build_structure. */
#define G2OHIP_PART_NO_VERTEX0 1
#define G2OHIP_PART_NO_VERTEX1 2
#define G2OHIP_PART_NO_CHI2 4
int g2ohip_set_edge_set_parts(g2ohip_solver* s, int set, int parts);

/* Solver::buildStructure(), block_solver.hpp:142-295.  do_schur mirrors setSchur()
 * (OptimizationAlgorithmWithHessian::init, optimization_algorithm_with_hessian.cpp:55-69). */
int g2ohip_build_structure(g2ohip_solver* s, int num_poses, int num_landmarks, int do_schur);

/* Per-iteration edge data = what linearizeOplus()/computeError() leave in each edge
 * (jacobianOplusXi/Xj, information, error; base_binary_edge.hpp:54-63), flat in edge order:
 *   J0 [n][error_dim x dim(v0)] column-major, J1 likewise (NULL for unary sets),
 *   omega [n][error_dim x error_dim], err [n][error_dim].
 * on_device != 0: the pointers are device pointers that stay valid until the next
 * g2ohip_build_system returns (zero-copy); otherwise host arrays, copied to the device. */
int g2ohip_set_edge_data(g2ohip_solver* s, int set, const double* J0, const double* J1, const double* omega,
                         const double* err, int on_device);
/* The errors of a set alone ([n][error_dim], host array) after g2ohip_set_edge_data with host arrays: what computeActiveErrors
 * (sparse_optimizer.cpp:61-74) leaves in the edges at TRIAL estimates -- chi2 of a Levenberg-Marquardt trial reads nothing else;
 * the Jacobians and information matrices stay what the system was built from. */
int g2ohip_set_edge_errors(g2ohip_solver* s, int set, const double* err);
/* OptimizableGraph::Edge::setRobustKernel (g2o.cpp:322-336); delta as RobustKernel::setDelta. */
int g2ohip_set_robust_kernel(g2ohip_solver* s, int set, int kind, double delta);
/* The same per EDGE: in g2o the robust kernel is a member of the edge (optimizable_graph.h:436-443, asked per edge by
 * base_binary_edge.hpp:92-112), so a pose graph with kernels on its loop closures only is still ONE set of EdgeSE2 / EdgeSE3.
 * kind [n], delta [n] (kind 0 = none for that edge); kind == NULL returns to the set-level kernel.  Not for a set bound to the
 * BA front end by g2ohip_ba_set_edges* (g2ohip_ba_set_edges_classes carries the kernels there: G2OHIP_ERR_STATE; a set bound by
 * g2ohip_ba_set_stereo_edges takes them).  Edges appended later by
 * g2ohip_update_structure start with no kernel until this is called again for the grown set. */
int g2ohip_set_robust_kernel_per_edge(g2ohip_solver* s, int set, const int32_t* kind, const double* delta);

/* Solver::buildSystem(), block_solver.hpp:501-560 (clear + per-edge constructQuadraticForm +
 * gather b).  Returns G2OHIP_OK on success (the reference returns 0 and nobody checks). */
int g2ohip_build_system(g2ohip_solver* s);
/* SparseOptimizer::activeRobustChi2(), sparse_optimizer.cpp:100-114, from the current edge data. */
int g2ohip_chi2(g2ohip_solver* s, double* chi2);

/* Solver::setLambda(lambda, backup) / restoreDiagonal(), block_solver.hpp:563-604.
 * With the Schur complement enabled the damping is virtual: lambda is held in device scalars and applied where
 * the diagonal is consumed (Hll + lambda I before the landmark inversion, Hpp + lambda I when Hschur is
 * formed), so Hpp / Hll in HBM are not modified and restoreDiagonal is exact by construction.  Everything read
 * through this ABI (g2ohip_copy_values, g2ohip_multiply_hessian, g2ohip_max_diagonal, Hschur, Dinv, x) shows the
 * damped system exactly as after the reference's setLambda; only raw g2ohip_device_array views of Hpp / Hll are
 * undamped.  Without Schur the diagonal is modified and restored in place as in the reference. */
int g2ohip_set_lambda(g2ohip_solver* s, double lambda, int backup);
int g2ohip_restore_diagonal(g2ohip_solver* s);
/* max_j |H_jj| over all free vertices: the quantity computeLambdaInit reads through
 * v->hessian(j,j) (optimization_algorithm_levenberg.cpp:149-163). */
int g2ohip_max_diagonal(g2ohip_solver* s, double* out);
/* sum_j x_j (lambda x_j + b_j): OptimizationAlgorithmLevenberg::computeScale (:165-172). */
int g2ohip_compute_scale(g2ohip_solver* s, double lambda, double* out);
/* The scalar diagonal of H (poses then landmarks, hessian-index order; vector_size() doubles) with the current damping:
 * what OptimizationAlgorithmLevenberg::computeLambdaInit reads through v->hessian(j, j) in the vertices' mapped memory
 * (optimization_algorithm_levenberg.cpp:149-163, base_vertex.h:62-110) -- the g2o adapter mirrors it on the host. */
int g2ohip_copy_diagonal(g2ohip_solver* s, double* diag_host);

/* Solver::solve(), block_solver.hpp:353-486: Schur complement, sparse block Cholesky of the
 * reduced pose system, landmark back-substitution.  G2OHIP_OK | G2OHIP_NOT_PD | error.
 * b is left untouched (block_solver.hpp:435-436). */
int g2ohip_solve(g2ohip_solver* s);

/* Solver::vectorSize(), x(), b() (solver.h:80-86).  x/b layout: poses then landmarks
 * (block_solver.hpp:551-557).  copy_* synchronise and copy to host; *_device return the
 * resident vectors (valid until destroy / build_structure). */
size_t g2ohip_vector_size(g2ohip_solver* s);
int g2ohip_copy_x(g2ohip_solver* s, double* x_host);
/* Overwrite the resident increment x (what g2ohip_ba_update / g2ohip_pg_update apply): SparseOptimizer::update
 * takes an arbitrary vector, e.g. Dogleg's h_dl (optimization_algorithm_dogleg.cpp:179). */
int g2ohip_set_x(g2ohip_solver* s, const double* x_host);
int g2ohip_copy_b(g2ohip_solver* s, double* b_host);
const double* g2ohip_x_device(g2ohip_solver* s);
const double* g2ohip_b_device(g2ohip_solver* s);

/* dest += H * src over the full [Hpp Hpl; Hpl' Hll] system (host vectors of vectorSize()).
 * Superset of BlockSolverBase::multiplyHessian (block_solver.h:83-91,142), used by Dogleg and
 * by residual checks. */
int g2ohip_multiply_hessian(g2ohip_solver* s, double* dest_host, const double* src_host);

int g2ohip_sync(g2ohip_solver* s);
/* HIP-event timing on the solver's stream.  0: off; 1: every kernel slot (g2ohip_kernel_time) and the stage
 * timers of g2ohip_get_stats; 2 + k: kernel slot k only (two event records per iteration -- the records are
 * not free next to sub-millisecond iterations). */
int g2ohip_set_profiling(g2ohip_solver* s, int enabled);
int g2ohip_get_stats(g2ohip_solver* s, g2ohip_stats* out);
/* Per-kernel HIP-event timing on the solver's stream (while profiling is enabled): slot in
 * [0, g2ohip_kernel_slots()), accumulated seconds and launch count since the last reset. */
int g2ohip_kernel_slots(void);
const char* g2ohip_kernel_name(int slot);
int g2ohip_kernel_time(g2ohip_solver* s, int slot, double* total_seconds, long* launches, int reset);
/* One Levenberg-Marquardt trial with a single host synchronisation (optimization_algorithm_levenberg.cpp:96-128 asks for
 * the solve status, the new chi2 and computeScale one after the other): g2ohip_solve_async queues g2ohip_solve and
 * leaves its status on the device; after the caller has updated the estimates and re-evaluated the errors,
 * g2ohip_trial_stats returns that status (solve_ok 1/0), activeRobustChi2 and computeScale(lambda) = x'(lambda x + b)
 * together.  Without a pending g2ohip_solve_async it just evaluates the two sums.  *solve_ok: 1 solved, 0 not positive
 * definite, 2 the solve has to be REPEATED (a dependency-driven launch gave up waiting -- never observed, the safety net of
 * DESIGN.md section 2; g2ohip_solve repeats by itself, the asynchronous pair leaves it to the caller: pop the estimates,
 * run the trial again).
 * g2ohip_trial_stats_begin queues the sums and their read-back WITHOUT waiting; the next g2ohip_trial_stats then only waits and
 * returns them (its lambda is ignored).  For a caller with host work to overlap: the adapter's LM driver queues the first trial of
 * the NEXT iteration this way and writes the accepted estimates into g2o's vertices (SparseOptimizer::update's effect,
 * sparse_optimizer.cpp:421-437) while the device works. */
/* The reduced (Schur) system as an operator, never formed (what "linear_solver" 2 iterates on; callers that run their own
 * Krylov loop, e.g. sharded over GPUs with one all-reduce of the product per iteration, use these directly):
 * prepare: Dinv = (Hll + lambda_l I)^-1, bschur = b_p - Hpl Dinv b_l (g2ohip_device_array 100) and the diagonal blocks
 * Hpp_ii + lambda_p I - sum B Dinv B' (g2ohip_device_array 107, [nP][p*p]); apply: out = (Hpp + lambda_p I - Hpl Dinv Hpl') in
 * on device vectors of nP*p doubles (in and out must not be the same vector: that is refused as a bad argument).  With
 * landmarks sharded over ranks both are this rank's summands. */
int g2ohip_schur_operator_prepare(g2ohip_solver* s);
int g2ohip_schur_operator_apply(g2ohip_solver* s, const double* in_device, double* out_device);
int g2ohip_solve_async(g2ohip_solver* s);
int g2ohip_trial_stats_begin(g2ohip_solver* s, double lambda);
int g2ohip_trial_stats(g2ohip_solver* s, double lambda, int* solve_ok, double* chi2, double* scale);
/* Options (name, value).  Linear solver of the reduced system: "linear_solver" 0 = multifrontal block Cholesky
 * (replaces LinearSolverCSparse / LinearSolverCholmod), 1 = block-Jacobi preconditioned CG (replaces
 * LinearSolverPCG, g2o/solvers/pcg/linear_solver_pcg.hpp:79-196; 2 = the same iteration matrix-free: with the Schur
 * complement on, Hschur is never formed -- Hschur v = Hpp v + lambda v - Hpl Dinv Hpl' v, exact block-Jacobi preconditioner)
 * with "pcg_tolerance" (1e-6),
 * "pcg_absolute_tolerance" (1), "pcg_max_iterations" (-1 = dimension), like LinearSolverPCG's setters
 * (linear_solver_pcg.h:74-85); iterations of the last solve in g2ohip_stats.iterationsLinearSolver.
 * Factorisation (also g2ohip_ls_set_option; the ordering / symbolic ones before g2ohip_build_structure): "nd_leaf"
 * (nested-dissection leaf size in blocks; 0 = auto: 32 and more for band-shaped graphs, 4 for the others), "max_sn_scalars"
 * (48: supernode width cap in scalars, at most 64 takes effect), "max_sn_scalars_lds" (0 = auto: 24 for band-shaped graphs,
 * 48 otherwise; the fronts that fit LDS), "dep_levels" (64: task levels that may share one dependency-driven launch, 0/1 =
 * one launch per level), "dep_backward" (1: the backward sweep in the same dependency-driven groups), "dep_spin_limit"
 * (1 << 21: polls before a waiting workgroup gives up), "band_kernel" (1: leaf chains of a band in the one-wave
 * sliding-window kernel), "tree_backward" (1: backward sweep of small fronts by groups in one workgroup), "big_front_passes"
 * (1: large fronts as whole-GPU passes with an MFMA update), "big_group" (8: panels of a long in-place chain updated as a
 * group; 1 = off) / "big_group_min_rows" (1024: for chains of at least that many rows).
 * Block solver: "schur_tile_bytes" (39936: LDS budget of one Schur tile), "fuse_schur_reduce" (1: g2ohip_solve on
 * one GPU folds the Schur reduction into the factorisation; Hschur is then written only when it is asked for),
 * "ba_fused" (1: the BA edge set's errors and Jacobians evaluated inside the assembly kernels), "ba_fuse_landmarks" (1: the
 * landmark side of the fused BA path assembled by the Schur tiles of the solve), "pg_landmark_staged" (1: the landmark linearize
 * kernels of the pose-graph front end store through LDS; 0: one lane per edge, for the comparison), "ba_stereo_staged" (1: the
 * same choice for the linearize kernel of g2ohip_ba_set_stereo_edges), "use_graph" (0), "mask_solution" (1),
 * "marginals_reduced" (0) / "marginals_recursion" (1) (see g2ohip_compute_marginals), "setup_overlap" (1: the symbolic
 * analysis next to the Schur tiles' set-up), "pcg_check_every" (16: PCG iterations between looks at the convergence flag),
 * "sharded_graph" (1: g2ohip_solve_sharded as one hipGraph where nothing crosses the host; 2: with RCCL too),
 * "sharded_merge" (1: the boundary blocks / b_p of a sharded solve travel in the all-reduce of the subtree roots -- two collectives per
 * solve instead of three -- whenever only the shared top of the tree consumes them; 0: always three), "sharded_selftest" (1: the
 * first sharded solve of a structure is checked against the reference schedule), "sharded_selftest_break" (tests only),
 * "comm_emulate" (timing only).  G2OHIP_OPTIONS="name=value,..." in the environment sets options for every solver of a process: g2ohip_create and
 * g2ohip_ls_create apply it (so the g2o plugin sees it too); a malformed or, for g2ohip_create, unknown entry fails the
 * creation with G2OHIP_ERR_ARG; an explicit g2ohip_set_option afterwards wins. */
int g2ohip_set_option(g2ohip_solver* s, const char* name, double value);

/* Inspection for parity tests (saveHessian-like, block_solver.hpp:628-632): block patterns
 * (column pointers + row block indices, ascending rows per column) and raw block values. */
int g2ohip_get_nnzb(g2ohip_solver* s, int which, int* nnzb);
int g2ohip_get_pattern(g2ohip_solver* s, int which, int32_t* colptr, int32_t* rowidx);
int g2ohip_copy_values(g2ohip_solver* s, int which, double* values_host);
/* Device pointers + element counts of resident arrays (for multi-GPU exchange through RCCL):
 * which = G2OHIP_HSCHUR (values), or 100 = bschur.  For tests only, no part of the supported interface: 108 = the information
 * matrices [n][3x3] of the bound GICP set as the last g2ohip_pg_linearize left them (G2OHIP_ERR_STATE without one; the pointer
 * holds until the set is bound again) -- g2ohip_copy_edge_data returns no information matrices; 109 = the inverse measurements
 * [n][7] of the bound EdgeSBACam set as g2ohip_pg_set_cam_edges stored them (G2OHIP_ERR_STATE without one). */
int g2ohip_device_array(g2ohip_solver* s, int which, double** ptr, size_t* count);
/* BlockSolver::computeMarginals / LinearSolver::solvePattern (block_solver.hpp:489-498, linear_solver.h:63-69,
 * marginal_covariance_cholesky.cpp:71-220): blocks (rows[i], cols[i]) (pose block indices) of the inverse of Hpp
 * with the current damping -- what the reference hands to solvePattern (`*_Hpp`, block_solver.hpp:492), also when
 * the Schur complement is on.  Option "marginals_reduced" = 1 (g2ohip_set_option) inverts the reduced pose system
 * instead: the pose marginals with the landmarks integrated out (a deviation from the reference, off by default).
 * Blocks inside the pattern of the factor come from ONE sparse-inverse pass over the frontal matrices (all of them at
 * once: what MarginalCovarianceCholesky's recursion computes entry by entry), the others from a pair of triangular
 * sweeps per column; option "marginals_recursion" = 0 forces the column path.
 * out [n][p*p], column-major blocks.  After g2ohip_build_system.  G2OHIP_OK | G2OHIP_NOT_PD. */
int g2ohip_compute_marginals(g2ohip_solver* s, int n_blocks, const int32_t* rows, const int32_t* cols, double* out);
/* The per-edge data the next g2ohip_build_system will consume, copied to the host (inspection / tests of the
 * device-side producers): J0 [n][d*dim0], J1 [n][d*dim1], err [n][d]; any pointer may be NULL. */
int g2ohip_copy_edge_data(g2ohip_solver* s, int set, double* J0, double* J1, double* err);

/* Drops every edge set (and the device front-end bindings) of the handle: the next g2ohip_add_edge_set starts a new
 * graph.  What BlockSolver::buildStructure does implicitly when it is called again (block_solver.hpp:142-204 deallocates
 * and rebuilds Hpp / Hll / Hpl): a second optimize() on the same solver, or a rebuild after online growth. */
int g2ohip_clear_edge_sets(g2ohip_solver* s);

/* Solver::updateStructure(vset, edges), block_solver.hpp:297-351: online growth WITHOUT Schur complement.  The new pose
 * vertices take the hessian indices [num_poses, num_poses + num_new_poses) (SparseOptimizer::updateInitialization appends them
 * to the index mapping, sparse_optimizer.cpp:269-352); the new edges are appended to an existing edge set (same error
 * dimension and vertex classes; for another edge type call g2ohip_add_edge_set first and pass n_new_edges = 0 here).  The
 * structure is rebuilt from the enlarged topology: g2ohip_vector_size grows, per-edge data of the touched set has to be
 * handed over again for ALL its edges (old ones first); a device front end bound to the touched set (g2ohip_pg_set_edges)
 * is unbound -- call g2ohip_pg_set_edges + g2ohip_pg_set_estimates again after growth (g2ohip_pg_linearize returns
 * G2OHIP_ERR_STATE until then).  G2OHIP_ERR_UNSUPPORTED where the reference aborts (a system with
 * marginalised vertices, :313-316). */
int g2ohip_update_structure(g2ohip_solver* s, int num_new_poses, int set, int n_new_edges, const int32_t* v0, const int32_t* v1);

/* Multi-GPU sharding support (openslam_g2o_amd/distributed.py).  Each rank holds a landmark
 * shard; to give every rank the SAME Hschur block layout (so the partial Schur complements
 * can be summed element-wise by one RCCL all-reduce) the union pattern is declared up front:
 * extra structural blocks (row <= col, pose block indices) of the reduced system.  Must
 * precede g2ohip_build_structure. */
int g2ohip_add_schur_pattern(g2ohip_solver* s, int n_blocks, const int32_t* rows, const int32_t* cols);
/* setLambda with separate damping of the pose and landmark diagonals: every rank damps its own
 * landmarks, only one rank adds lambda to the (summed) pose diagonal. */
int g2ohip_set_lambda_split(g2ohip_solver* s, double lambda_pose, double lambda_landmark, int backup);

/* Subtree-distributed factorisation of the reduced system: the top of the
 * elimination-task tree is split into >= world subtrees; rank r factorises its own subtrees, every rank
 * factorises the few shared tasks above them redundantly.  g2ohip_set_partition precedes
 * g2ohip_build_structure (all ranks must pass the same union Schur pattern and options: the symbolic
 * analysis is deterministic, so every rank derives the same partition).  Per solve:
 *   g2ohip_solve_reduced_local   own subtrees: factor + forward sweep, pack the subtree roots' update
 *                                matrices/vectors into the exchange buffer (g2ohip_device_array 103)
 *   [caller: all-reduce(SUM) of buffer 103 over the ranks]
 *   g2ohip_solve_reduced_shared  shared top: factor + forward/backward, backward sweep of the own
 *                                subtrees, mask x_p entries owned elsewhere (g2ohip_device_array 104)
 *   [caller: all-reduce(SUM) of buffer 104]
 *   g2ohip_solve_reduced_finish  un-permute x_p; G2OHIP_NOT_PD if a local pivot was <= 0
 * With option "mask_solution" = 0 the masking is skipped: every rank then holds valid x_p for its own and
 * the shared poses, and the caller exchanges only the few foreign poses its landmarks observe (after
 * g2ohip_solve_reduced_finish, on g2ohip_device_array 101).
 * g2ohip_get_partition: owner rank (-1 = shared) of every pose block and of every Hschur block (the rank
 * that consumes its value) -- what the caller needs to exchange only the boundary blocks.
 * g2ohip_partition_poses: the same partition (block_consumer may be NULL) from a bare block pattern, host only (no device), so
 * landmarks can be dealt to ranks before build_structure; options_from (may be NULL) supplies the ordering
 * options (g2ohip_set_option) so that the result matches what that solver will compute.  In partitioned
 * mode g2ohip_set_lambda[_split] damps a pose block only on the rank that consumes its diagonal block. */
int g2ohip_set_partition(g2ohip_solver* s, int rank, int world);
int g2ohip_solve_reduced_local(g2ohip_solver* s);
int g2ohip_solve_reduced_shared(g2ohip_solver* s);
int g2ohip_solve_reduced_finish(g2ohip_solver* s);
/* The same exchange without host round trips (what openslam_g2o_amd/distributed.py does per solve): the caller
 * registers once the reduced-system blocks / poses on partition boundaries (with 0/1 keep flags: a rank keeps the
 * summed value only of what it consumes) and the foreign "halo" poses its landmarks observe (flag 1 where this rank
 * owns the value); then per solve
 *   g2ohip_solve_schur, g2ohip_exchange_pack(1), [all-reduce g2ohip_device_array 105], g2ohip_exchange_unpack(1),
 *   g2ohip_solve_reduced_local, [all-reduce 103], g2ohip_solve_reduced_shared, g2ohip_solve_reduced_finish_async,
 *   g2ohip_exchange_pack(3), [all-reduce 106: halo x_p + failure flags], g2ohip_exchange_unpack(3),
 *   g2ohip_solve_back_substitute, g2ohip_exchange_status  (the only synchronisation; G2OHIP_NOT_PD if any rank failed,
 *   G2OHIP_REPEAT -- on every rank alike -- if the phases are to be run again: see the define). */
int g2ohip_exchange_setup(g2ohip_solver* s, int n_blocks, const int32_t* block_idx, const double* block_keep, int n_poses,
                          const int32_t* pose_idx, const double* pose_keep, int n_halo, const int32_t* halo_idx, const double* halo_mine);
int g2ohip_exchange_pack(g2ohip_solver* s, int which);
int g2ohip_exchange_unpack(g2ohip_solver* s, int which);
int g2ohip_exchange_status(g2ohip_solver* s);
int g2ohip_solve_reduced_finish_async(g2ohip_solver* s);
int g2ohip_get_partition(g2ohip_solver* s, int32_t* pose_owner, int32_t* block_consumer);

/* ---- collectives inside the library: the N > 1 path for C / C++ consumers -------------------------------------------
 * One process per GPU; every rank creates its solver, registers ITS shard of the edges, calls g2ohip_set_partition +
 * g2ohip_build_structure + g2ohip_exchange_setup (the index lists come from g2ohip_partition_poses, see
 * openslam_g2o_amd/distributed.py for the host-side recipe) and attaches a communicator:
 *   RCCL over xGMI: rank 0 calls g2ohip_comm_unique_id, hands the 128 bytes to the other ranks by any means (MPI, a file,
 *   a socket), every rank calls g2ohip_comm_init_rccl -- ncclCommInitRank; librccl is bound at run time, libg2ohip.so
 *   itself has no link dependency on it;
 *   host callback: g2ohip_comm_init_host with an in-place all-reduce over host memory (op 0 = sum, 1 = max; MPI_Allreduce
 *   fits directly): device buffers are staged through pinned memory.  For ranks sharing one GPU (tests) and boxes
 *   without peer access; not a performance path;
 *   peer mailboxes (opt-in): g2ohip_comm_init_peer -- every rank exports a device mailbox (hipIpcGetMemHandle; the handles
 *   travel through the host all-reduce once), an all-reduce is one kernel that stores the payload into the rank's slot of
 *   every peer's mailbox over xGMI and one that waits for all slots and adds them in rank order: two launches for the
 *   latency-sized payloads of the sharded solve instead of a ring.  slot_doubles = capacity of a slot (larger payloads go
 *   in pieces).  A peer that does not deliver within the wait limit (5 s) fails the call that next synchronises
 *   (G2OHIP_ERR_STATE) instead of hanging the device.  Verified with several processes on one GPU only; RCCL is the default.
 * g2ohip_solve_sharded then runs the whole linear solve (BlockSolver::solve, block_solver.hpp:353-486, on the sharded
 * system): local Schur pass | all-reduce of the boundary blocks of the reduced system and boundary b_p | own subtrees of
 * the elimination tree | all-reduce of the subtree roots' update matrices | shared top + backward sweep | all-reduce of
 * the halo x_p and the failure flags | back-substitution of the own landmarks.  G2OHIP_OK | G2OHIP_NOT_PD (on every rank
 * alike).  x_p is valid for own, shared and halo poses, x_l for the own landmarks.
 * The *_sharded scalars are the Levenberg-Marquardt quantities over all ranks (activeRobustChi2, computeLambdaInit's
 * maximum, computeScale: optimization_algorithm_levenberg.cpp:149-172). */
typedef int (*g2ohip_host_allreduce_fn)(void* ctx, double* host_buffer, size_t count, int op);
int g2ohip_comm_unique_id(char* id128);
int g2ohip_comm_init_rccl(g2ohip_solver* s, int rank, int world, const char* id128);
int g2ohip_comm_init_host(g2ohip_solver* s, int rank, int world, g2ohip_host_allreduce_fn fn, void* ctx);
int g2ohip_comm_init_peer(g2ohip_solver* s, int rank, int world, g2ohip_host_allreduce_fn fn, void* ctx, size_t slot_doubles);
int g2ohip_comm_destroy(g2ohip_solver* s);
int g2ohip_comm_all_reduce(g2ohip_solver* s, double* device_buffer, size_t count, int op);   /* in place, on the solver's stream */
int g2ohip_solve_sharded(g2ohip_solver* s);
int g2ohip_chi2_sharded(g2ohip_solver* s, double* chi2);
int g2ohip_max_diagonal_sharded(g2ohip_solver* s, double* out);
int g2ohip_compute_scale_sharded(g2ohip_solver* s, double lambda, double* out);
int g2ohip_partition_poses(const g2ohip_solver* options_from, int block_dim, int n_blocks, const int32_t* colptr,
                           const int32_t* rowidx, int world, int32_t* pose_owner, int32_t* block_consumer);

/* Split solve for the multi-GPU path: g2ohip_solve == schur + reduced + back_substitute. */
int g2ohip_solve_schur(g2ohip_solver* s);            /* K5-K8: Hschur, bschur, Dinv          */
int g2ohip_solve_reduced(g2ohip_solver* s);          /* K9-K12: x_p = Hschur \ bschur        */
int g2ohip_solve_back_substitute(g2ohip_solver* s);  /* K13: x_l = Dinv (b_l - Hpl' x_p)     */

/* ---- page-locked host buffers ---------------------------------------------------------------
 * The boundary takes plain host pointers (Solver::_x / _b are `new double[]` of g2o's own Solver::resizeVector,
 * g2o/core/solver.cpp:46-70).  Pageable memory crosses PCIe through the driver's staging copy (~6-10 GB/s); a caller that
 * keeps handing over the SAME buffers every iteration -- the adapter: estimates up, b / x / diagonal down -- registers them
 * once (hipHostRegister) and the copies run at the link rate.  Unregister before the buffer is freed or reallocated. */
int g2ohip_host_register(g2ohip_solver* s, void* ptr, size_t bytes);
int g2ohip_host_unregister(g2ohip_solver* s, void* ptr);

/* ---- device-resident bundle-adjustment front end (a "next" row) -----
 * For graphs of EdgeProjectXYZ2UV (g2o/types/sba/types_six_dof_expmap.h:127-150) the library can
 * produce errors and Jacobians itself and keep the vertex estimates on the device, so a whole
 * Levenberg-Marquardt trial loop (optimization_algorithm_levenberg.cpp:57-146) runs without moving
 * Jacobians or estimates over PCIe.  Estimates: cams [n][12] = R (column-major) | t, world -> camera
 * (what VertexSE3Expmap holds, types_six_dof_expmap.cpp:88-103); points [n][3]. */
/* edge set `set` (added with error_dim 2, vertex 0 = point, vertex 1 = pose): per-edge indices into
 * the estimate arrays (all vertices, fixed ones included), measurements [n][2], information [n][2x2]
 * (NULL = identity), CameraParameters (focal_length, principle_point). After g2ohip_build_structure. */
int g2ohip_ba_set_edges(g2ohip_solver* s, int set, const int32_t* cam_vertex, const int32_t* point_vertex, const double* meas,
                        const double* info, double focal_length, double cx, double cy);
/* The same with EDGE CLASSES: the edges of one set may differ in their CameraParameters (every EdgeProjectXYZ2UV carries
 * its own _cam, types_six_dof_expmap.h:133-153) and in their robust kernel (OptimizableGraph::Edge::setRobustKernel,
 * optimizable_graph.h:436-443; base_binary_edge.hpp:92-112 asks each edge for its own).  class_params [n_classes][5] =
 * (focal_length, principle_point x, y, robust kernel kind as in g2ohip_set_robust_kernel, delta), edge_class [n] the class of
 * every edge (NULL with one class).  1 <= n_classes <= 128; with more than one class the set must be on the fused path
 * (one observation per (pose, landmark) pair, no fixed landmark) -- G2OHIP_ERR_ARG otherwise, and
 * g2ohip_set_robust_kernel on the set is refused (G2OHIP_ERR_STATE) while the classes are bound. */
int g2ohip_ba_set_edges_classes(g2ohip_solver* s, int set, const int32_t* cam_vertex, const int32_t* point_vertex, const double* meas,
                                const double* info, int n_classes, const double* class_params, const int32_t* edge_class);
/* The same slot bound to STEREO observations: EdgeProjectXYZ2UVU (g2o/types/sba/types_six_dof_expmap.h:181-200; error
 * (u_left, v_left, u_right) = obs - CameraParameters::stereocam_uvu_map(T.map(X)), types_six_dof_expmap.cpp:40, 77-82, with the fourth
 * field of CameraParameters, `baseline`, types_six_dof_expmap.h:53-80: u_right = f (x - baseline) / z + cx).  Edge set `set` was added
 * with error_dim 3, vertex 0 = 3-dof point, vertex 1 = 6-dof pose, on a (6, 3) solver (anything else: G2OHIP_ERR_ARG);
 * measurements [n][3], information [n][3x3] column-major (NULL = identity).  After g2ohip_build_structure.  The front end has ONE
 * slot: a later g2ohip_ba_set_edges* or g2ohip_ba_set_stereo_edges replaces the binding; one that is rejected (null array,
 * non-finite parameter or focal_length == 0, index outside the estimate tables, hessian indices that differ from the set's:
 * G2OHIP_ERR_ARG; a set that carries per-edge robust kernels: G2OHIP_ERR_STATE) leaves the previous binding usable.
 * The reference leaves linearizeOplus of this edge commented out (types_six_dof_expmap.h:199) and differentiates numerically;
 * the device writes the exact derivative.  A stereo set always takes the generic assembly (option "ba_fused" is ignored for
 * it, edge classes are not offered): fixed cameras and points, several observations of one (pose, landmark) pair,
 * g2ohip_set_robust_kernel and -- on the bound set -- g2ohip_set_robust_kernel_per_edge, do_schur 0 / 1, every linear_solver
 * and use_graph work as for any generic set.  Everything below (set_estimates ... discard_top) acts on it unchanged. */
int g2ohip_ba_set_stereo_edges(g2ohip_solver* s, int set, const int32_t* cam_vertex, const int32_t* point_vertex, const double* meas,
                               const double* info, double focal_length, double cx, double cy, double baseline);
/* A SECOND slot beside the projection slot: ONE set of pose-pose constraints between cameras, EdgeSE3Expmap (tag EDGE_SE3:EXPMAP,
 * g2o/types/sba/types_six_dof_expmap.h:111-130: odometry, loop closures, the terms that tie a local window to the rest of the map).
 * Vertex 0 of an edge is Ti = cams[vi[k]], vertex 1 is Tj = cams[vj[k]] (indices into the camera table of g2ohip_ba_set_estimates,
 * fixed cameras included); meas [n][12] = the measurement C as an isometry, R column-major | t, like a camera; information
 * [n][6x6] column-major (NULL = identity, written on the device).  Error e = log(Tj^-1 C Ti) in the order (omega, upsilon), log as
 * SE3Quat::log is written (g2o/types/slam3d/se3quat.h:178-215, its branch at d > 0.99999 included; like the reference no guard near
 * a relative rotation of pi or for a trace outside [-1, 3]).  Jacobians as EdgeSE3Expmap::linearizeOplus
 * (types_six_dof_expmap.cpp:271-286): J0 = adj(Tj^-1 C), J1 = -adj(Ti^-1 C^-1), adj as se3quat.h:259-268 -- the reference's ADJOINT
 * FORM, which is the derivative of the error at e = 0 only, not the derivative of the logarithm.
 * Edge set `set` was added as a binary set with error_dim 6 and both vertex dimensions 6 on a (6, 3) solver, and is not the set of
 * the projection slot.  After g2ohip_build_structure AND after g2ohip_ba_set_edges* / g2ohip_ba_set_stereo_edges (otherwise
 * G2OHIP_ERR_STATE; so is a set that carries per-edge robust kernels at the binding -- set them on the bound set).  Null vi / vj /
 * meas, non-finite values, indices outside the camera table, cam_hidx[vi[k]] / cam_hidx[vj[k]] that differ from the set's vertex
 * 0 / 1 (-1 = fixed), a set of another shape or the projection set itself: G2OHIP_ERR_ARG.  A rejected call leaves the previous
 * binding usable.  Many edges on one pair and a pair in both orders are legal, and so are zero edges.  A later call replaces the
 * binding (a call that binds another set leaves the set that was bound without edge data: g2ohip_build_system returns
 * G2OHIP_ERR_STATE until g2ohip_set_edge_data feeds it, unless it is empty), a later g2ohip_ba_set_edges* / g2ohip_ba_set_stereo_edges keeps it, g2ohip_ba_set_estimates with changed tables validates
 * it again, g2ohip_clear_edge_sets drops it; after g2ohip_update_structure has grown the set g2ohip_ba_linearize returns
 * G2OHIP_ERR_STATE until it is bound again (a guard: today g2ohip_update_structure refuses every structure that can hold a
 * projection binding -- it needs a landmark in the structure).  g2ohip_ba_linearize writes the set's errors (and, with jacobians = 1, its Jacobians,
 * on the fused path of the projection set too); chi2 and robust weights go the generic way (g2ohip_set_robust_kernel(_per_edge) on
 * the set); the fused assembly and back-substitution of the projection set stay in place, since the set touches no landmark.
 * NOT covered: the g2o plugin adapter (EdgeSE3Expmap stays on its host path there), a pose set without a projection set (a pure
 * VertexSE3Expmap pose graph), more than one pose set per handle, sharded solves, fused kernels for the set. */
int g2ohip_ba_set_pose_edges(g2ohip_solver* s, int set, const int32_t* vi, const int32_t* vj, const double* meas, const double* info);
/* The projection slot bound to ANCHORED INVERSE-DEPTH observations: EdgeProjectPSI2UV (g2o/types/sba/types_six_dof_expmap.h:158-178,
 * types_six_dof_expmap.cpp:173-233; what g2o/examples/ba_anchored_inverse_depth runs), a THREE-vertex edge: vertex 0 the point
 * psi = (x / z, y / z, 1 / z) in the frame of its anchor keyframe (an entry of `points`), vertex 1 the observing pose T =
 * cams[cam_vertex[k]], vertex 2 the anchor pose A = cams[anchor_vertex[k]].  With x_a = (psi0, psi1, 1) / psi2 and y = T A^-1 x_a:
 * e = meas - (f y0 / y2 + cx, f y1 / y2 + cy); the Jacobians are the reference's analytic ones (J_point = -Jcam [r1, r2, -R_ca x_a] /
 * psi2, J_pose = -Jcam [-skew(y) | I], J_anchor = Jcam R_ca [-skew(x_a) | I]).  Like the reference there is no guard for psi2 == 0 or
 * y2 <= 0.  The edge is bound as the three binary sets g2ohip_set_edge_set_parts documents for three vertices, all with error_dim 2 and
 * the same number of edges, on a (6, 3) solver:
 *   set_point_pose    (v0 = point, v1 = pose)    parts 0
 *   set_point_anchor  (v0 = point, v1 = anchor)  parts G2OHIP_PART_NO_VERTEX0 | G2OHIP_PART_NO_VERTEX1 | G2OHIP_PART_NO_CHI2
 *   set_pose_anchor   (v0 = pose,  v1 = anchor)  parts G2OHIP_PART_NO_VERTEX0 | G2OHIP_PART_NO_CHI2
 * meas [n][2], information [n][2x2] (NULL = identity, written on the device).  The three sets are bound and released as ONE group and
 * share their Jacobians, information and errors on the device (g2ohip_copy_edge_data of each returns its pair's two Jacobians).  They
 * occupy the projection slot: a later g2ohip_ba_set_edges* / g2ohip_ba_set_stereo_edges replaces the binding (the three sets are
 * then without edge data until g2ohip_set_edge_data feeds them), and this call replaces theirs; the EdgeSE3Expmap slot beside it
 * keeps working.  Always the generic assembly (option "ba_fused" is ignored), do_schur 0 / 1, every linear_solver and use_graph.
 * After g2ohip_build_structure (G2OHIP_ERR_STATE otherwise; so is a set that carries per-edge robust kernels at the binding).
 * G2OHIP_ERR_ARG: a bad set id or the same id twice, wrong dimensions, parts or unequal edge counts, a null index or meas array, a
 * non-finite value or focal_length == 0, an index outside the estimate tables, a hessian index that differs from the sets'
 * (cam_hidx, num_poses + point_hidx, -1 = fixed), one of the sets being the bound pose-edge set.  A rejected call leaves the previous
 * binding usable; g2ohip_ba_set_estimates with changed tables validates the binding again, anchors included;
 * g2ohip_clear_edge_sets drops it.
 * THE ANCHOR'S OWN OBSERVATION (cam_vertex[k] == anchor_vertex[k], which the reference example creates): the error depends on psi
 * alone and the two camera Jacobians cancel exactly.  The reference maps both sides onto one diagonal block and adds the unsymmetric
 * term A1' Omega A2 there (base_multi_edge.hpp:190-208); HERE such an edge must carry -1 on every camera side of all three sets
 * (G2OHIP_ERR_ARG otherwise) and contributes to its point alone -- a deliberate deviation from the reference.
 * Robust kernels: the generic assembly weighs each set by its own kernel, so the caller sets the SAME kernel -- set-level, or per
 * edge after the binding -- on all three sets.
 * NOT covered: the g2o plugin adapter, XYZ and inverse-depth points in one graph, edge classes, sharded solves. */
int g2ohip_ba_set_inverse_depth_edges(g2ohip_solver* s, int set_point_pose, int set_point_anchor, int set_pose_anchor,
                                      const int32_t* cam_vertex, const int32_t* anchor_vertex, const int32_t* point_vertex,
                                      const double* meas, const double* info, double focal_length, double cx, double cy);
/* setEstimate for every vertex + the index mapping: cam_hidx[v] = hessianIndex (-1 fixed),
 * point_hidx[v] = landmark index (0-based, i.e. hessianIndex - num_poses) or -1. */
int g2ohip_ba_set_estimates(g2ohip_solver* s, int n_cams, const double* cams, const int32_t* cam_hidx, int n_points,
                            const double* points, const int32_t* point_hidx);
int g2ohip_ba_get_estimates(g2ohip_solver* s, double* cams, double* points);
/* The estimates of SELECTED vertices (indices into the arrays of g2ohip_ba_set_estimates): cams [n_cams][12], points [n_points][3].
 * What a caller with a few host-side edges reads of an LM trial -- BaseUnaryEdge / BaseMultiEdge::computeError
 * (base_unary_edge.hpp:42-72) need the estimates of the vertices THEY touch, not all 1.1 M -- next to the full read-back. */
int g2ohip_ba_get_estimates_of(g2ohip_solver* s, int n_cams, const int32_t* cam_index, double* cams, int n_points, const int32_t* point_index,
                               double* points);
/* The same read-back (what SparseOptimizer::update leaves in the vertices, sparse_optimizer.cpp:422-432, fetched for the caller's
 * setEstimate loop) started ASYNCHRONOUSLY behind everything queued so far -- typically right after g2ohip_ba_update of an LM
 * trial -- on a copy stream of the library, in pieces: piece 0 = the cameras, pieces 1 .. point_pieces (<= 16) = the points in
 * equal ranges.  g2ohip_ba_fetch_estimates_wait(piece) returns once that piece is in the caller's buffer (page-locked buffers,
 * g2ohip_host_register, make the copy truly asynchronous): the caller writes piece k into its vertices while piece k + 1 is
 * still in flight and the device evaluates the trial's errors.  The buffers must stay untouched until the last piece has been
 * waited for or the next g2ohip_ba_set_estimates; device-side writers of the estimates (update, pop) wait for the copy themselves. */
int g2ohip_ba_fetch_estimates_begin(g2ohip_solver* s, double* cams, double* points, int point_pieces);
int g2ohip_ba_fetch_estimates_wait(g2ohip_solver* s, int piece);
/* computeActiveErrors() (+ linearizeOplus() when jacobians != 0) into the set's edge data
 * (sparse_optimizer.cpp:61-76, types_six_dof_expmap.cpp:288-326). */
int g2ohip_ba_linearize(g2ohip_solver* s, int jacobians);
/* SparseOptimizer::update(x): oplus of every free vertex with the current solution (sparse_optimizer.cpp:421-434). */
int g2ohip_ba_update(g2ohip_solver* s);
/* SparseOptimizer::push / pop / discardTop on all vertices (one level, what LM needs; sparse_optimizer.cpp:599-650). */
int g2ohip_ba_push(g2ohip_solver* s);
int g2ohip_ba_pop(g2ohip_solver* s);
int g2ohip_ba_discard_top(g2ohip_solver* s);
/* StructureOnlySolver<3>::calc(points, num_iters, num_max_trials) on the bound projection set
 * (g2o/solvers/structure_only/structure_only_solver.h:72-194; what ba_demo.cpp:261-269 and sba_demo.cpp:351-359 run before the
 * joint optimisation, g2o_cli's structure_only_3): a Levenberg-Marquardt per landmark with every pose frozen, for every free
 * point (point_hidx >= 0) in ONE kernel launch -- all outer iterations and damping trials on the device.  mu = 0.01, nu = 2
 * (:86-87, hard-coded there too); chi2 = sum e' Omega e over the point's track, observations from fixed cameras included
 * (:89-93); per outer iteration H = sum w J' Omega J, b = -sum w J' Omega e with the robust weight of the set's kernel
 * (:106-135), stop when |b| < 0.001 (:139-142); trials: H + mu I factorised, the candidate accepted iff chi2 - new_chi2 > 0
 * and new_chi2 is finite (:145-170; the RAW chi2, as e->chi2() there), then mu *= 1/3, nu = 2, else mu *= nu, nu *= 2 and the
 * point stops after num_max_trials rejections in one outer iteration (:173-186).  Deviation: an unpivoted 3 x 3 LDL' with the
 * test "every pivot > 0" in place of Eigen's pivoted LDLT::isPositive() (:148-150); with mu > 0 they differ on non-finite
 * input only.  Bound to EdgeProjectXYZ2UV (g2ohip_ba_set_edges*, edge classes included) or EdgeProjectXYZ2UVU
 * (g2ohip_ba_set_stereo_edges); an EdgeProjectPSI2UV binding is refused with G2OHIP_ERR_STATE.
 * point_trace: NULL or [n_points][4] = (outer iterations started, accepted steps, rejected trials, stop reason: 0 ran
 * num_iters, 1 |b| < 1e-3, 2 num_max_trials reached, 3 not optimised -- the point is fixed or its track is empty);
 * point_chi2: NULL or [n_points][2] = (chi2 before, chi2 after), (0, 0) for stop reason 3; both indexed like `points` of
 * g2ohip_ba_set_estimates.  G2OHIP_ERR_STATE before g2ohip_ba_set_edges* / g2ohip_ba_set_stereo_edges and
 * g2ohip_ba_set_estimates, G2OHIP_ERR_ARG for num_iters < 0 or num_max_trials < 1; num_iters == 0 is legal (chi2 only, the
 * points stay untouched).  The call is a writer of the estimates like g2ohip_ba_update: errors, Jacobians and chi2 of the set
 * are stale afterwards and the next g2ohip_build_system assembles anew.  Between g2ohip_ba_push and g2ohip_ba_pop it is legal,
 * and pop restores the points. */
int g2ohip_ba_structure_only(g2ohip_solver* s, int num_iters, int num_max_trials, int32_t* point_trace, double* point_chi2);

/* ---- device-resident pose-graph front end ----------------------------
 * Error + Jacobian producers and vertex updates for pose graphs, so a Gauss-Newton / LM iteration needs no
 * host round trip: type 1 = EdgeSE2 / VertexSE2 (g2o/types/slam2d/edge_se2.h:51-57, edge_se2.cpp:76-99,
 * vertex_se2.h:55-59), estimates and measurements (x, y, theta), information [n][3x3];
 * type 2 = EdgeSE3 / VertexSE3 (g2o/types/slam3d/edge_se3.cpp:48-75, isometry3d_gradients.h:39-126,
 * vertex_se3.h:107-116), estimates and measurements as isometries [12] = R (column-major) | t,
 * information [n][6x6];
 * type 10 = EdgeSim3 / VertexSim3Expmap, the 7-dof pose graph of monocular SLAM (g2o/types/sim3/types_seven_dof_expmap.h:44-65
 * oplusImpl, :94-102 computeError e = log(C Si Sj^-1); g2o/types/sim3/sim3.h:70-142 exp, :148-230 log, :233-236 inverse,
 * :266-272 operator*): estimates and measurements are the members of the reference's Sim3, 8 doubles (qx, qy, qz, qw, tx, ty,
 * tz, s), information [n][7x7], on a handle of pose dimension 7 and a set of error_dim 7.  The reference defines no Jacobian
 * for this edge; the device evaluates what g2o then uses, the central differences of BaseBinaryEdge::linearizeOplus
 * (g2o/core/base_binary_edge.hpp:132-201, delta = 1e-9) through oplusImpl, and writes zeros for the block of a fixed vertex.
 * G2OHIP_ERR_ARG for a quaternion of norm 0, a scale <= 0 or a non-finite value in the measurements or estimates, for another
 * pose or error dimension, and for any prior set or landmark set of types 3-6 beside a type-10 set (either order); the one
 * landmark set that stands beside it is EdgeSim3ProjectXYZ (g2ohip_pg_set_sim3_project_edges below), and for a map of keyframes
 * and points without Sim3 constraints the type-10 set may hold zero edges (its arrays may then be NULL).  Not covered: priors
 * beside a Sim3 set, more than one landmark set per handle, sharded solves, the g2o plugin adapter (it keeps these edges on
 * its host path).
 * Edge set `set` was added with error_dim 3 / 6 / 7 and hessian indices of its two
 * vertices; vi/vj index the estimate array (all vertices, fixed ones included), hidx[v] = hessianIndex or -1.
 * The calls mirror the g2ohip_ba_* ones (set_edges after g2ohip_build_structure).
 * The set_edges / set_estimates entries of both front ends (g2ohip_ba_*, g2ohip_pg_*, the landmark half below) validate what
 * they are handed against what is already bound BEFORE they commit any of it: a call rejected with G2OHIP_ERR_ARG leaves the
 * previous edges and estimate tables bound and usable as they were (after a rejected FIRST g2ohip_*_set_estimates there is no
 * table, and linearize / update / push / get_estimates return G2OHIP_ERR_STATE until a valid one arrives). */
int g2ohip_pg_set_edges(g2ohip_solver* s, int set, int type, const int32_t* vi, const int32_t* vj, const double* meas,
                        const double* info);
int g2ohip_pg_set_estimates(g2ohip_solver* s, int n_vertices, const double* poses, const int32_t* hidx);
/* VertexSim3Expmap::_fix_scale (types_seven_dof_expmap.h:60-61, 78) for every vertex of a type-10 binding: the sigma entry of a
 * step is taken as zero in g2ohip_pg_update and in the perturbations of the numeric Jacobian, whose column 6 is then exactly
 * zero.  Default 0; kept when g2ohip_update_structure drops the binding, back to 0 after g2ohip_clear_edge_sets. */
int g2ohip_pg_set_sim3_fix_scale(g2ohip_solver* s, int fix_scale);
int g2ohip_pg_get_estimates(g2ohip_solver* s, double* poses);
int g2ohip_pg_linearize(g2ohip_solver* s, int jacobians);
int g2ohip_pg_update(g2ohip_solver* s);
int g2ohip_pg_push(g2ohip_solver* s);
int g2ohip_pg_pop(g2ohip_solver* s);
int g2ohip_pg_discard_top(g2ohip_solver* s);

/* ---- ... its landmark half: odometry between poses PLUS point landmarks observed from them ---------------------
 * One pose-landmark observation set of the same handle beside the pose-pose set of g2ohip_pg_set_edges, the landmark
 * estimates resident on the device:
 *   type 3 = EdgeSE2PointXY over VertexSE2 / VertexPointXY (g2o/types/slam2d/edge_se2_pointxy.h:44-49 computeError,
 *            edge_se2_pointxy.cpp:66-90 linearizeOplus, vertex_point_xy.h:77-81 oplusImpl): e = R(theta)' (l - t) - z,
 *            measurements [n][2], information [n][2x2], landmarks (x, y); beside a type-1 pose set only;
 *   type 4 = EdgeSE3PointXYZ over VertexSE3 / VertexPointXYZ (g2o/types/slam3d/edge_se3_pointxyz.cpp:95-131 computeError /
 *            linearizeOplus, parameter_se3_offset.cpp:44-50 CacheSE3Offset::updateImpl, vertex_pointxyz.h:48-51 oplusImpl)
 *            with ONE ParameterSE3Offset for the whole set: e = (X offset)^-1 l - z, measurements [n][3], information
 *            [n][3x3], landmarks (x, y, z), offset an isometry [12] = R (column-major) | t or NULL for the identity (type 4
 *            only); beside a type-2 pose set only.
 * Edge set `set` was added with error_dim 2 / 3, vertex 0 = the pose's hessian index, vertex 1 = the landmark's
 * (num_poses + landmark number), -1 for a fixed vertex on either side.  pose_vertex[k] indexes the pose table of
 * g2ohip_pg_set_estimates, point_vertex[k] the landmark table of g2ohip_pg_set_landmark_estimates, whose hidx[v] is the
 * landmark's hessian index in the whole system (>= num_poses) or -1; its update is the plain addition of
 * x[num_poses * pose_dim + (hidx - num_poses) * landmark_dim ..].
 * Call after g2ohip_build_structure and after g2ohip_pg_set_edges (G2OHIP_ERR_STATE otherwise); a wrong pairing of types,
 * wrong dimensions of the set, indices out of range or hessian indices that differ from the edge set's give G2OHIP_ERR_ARG.
 * g2ohip_pg_linearize / update / push / pop / discard_top then act on both halves; g2ohip_pg_linearize with landmark edges
 * bound but no landmark estimates returns G2OHIP_ERR_STATE.  The binding goes wherever the pose binding goes
 * (g2ohip_clear_edge_sets, growth of a bound set).  Robust kernels of the set: g2ohip_set_robust_kernel(_per_edge) as for
 * any set.  do_schur = 1 (landmarks marginalised) is the intended configuration; with do_schur = 0 g2ohip_solve solves the
 * pose block alone (x_p = Hpp^-1 b_p, the landmark part of x stays zero), as for every system with landmarks. */
int g2ohip_pg_set_landmark_edges(g2ohip_solver* s, int set, int type, const int32_t* pose_vertex, const int32_t* point_vertex,
                                 const double* meas, const double* info, const double* offset);
/* The projective pose -> point edges of an RGB-D / stereo front end, bound to the SAME single landmark slot of the handle (a
 * later call of either entry replaces the binding), beside a type-2 (EdgeSE3) pose set only, landmarks (x, y, z):
 *   type 5 = EdgeSE3PointXYZDepth (g2o/types/slam3d/edge_se3_pointxyz_depth.cpp:91-138 computeError / linearizeOplus):
 *            e = (p0 / p2, p1 / p2, p2) - z, measurement (u, v, depth);
 *   type 6 = EdgeSE3PointXYZDisparity (edge_se3_pointxyz_disparity.cpp:96-168, analytic Jacobian as enabled by
 *            edge_se3_pointxyz_disparity.h:36): e = (p0 / p2, p1 / p2, 1 / p2) - z, measurement (u, v, 1 / depth);
 * with p = Kcam (X offset)^-1 l and ONE ParameterCamera / CacheCamera for the whole set (parameter_camera.cpp:45-59, 93-96):
 * offset an isometry [12] = R (column-major) | t or NULL for the identity, kcam[4] = fx, fy, cx, cy (required, finite, fx and
 * fy not zero).  meas [n][3], info [n][3x3].  Like the reference there is no guard for a point on or behind the image plane
 * (p2 <= 0).  Preconditions, validation and error codes are those of g2ohip_pg_set_landmark_edges (which keeps rejecting
 * types other than 3 and 4); everything after the binding -- g2ohip_pg_set_landmark_estimates, g2ohip_pg_linearize / update /
 * push / pop / discard_top, robust kernels, g2ohip_clear_edge_sets -- acts on it unchanged. */
int g2ohip_pg_set_landmark_camera_edges(g2ohip_solver* s, int set, int type, const int32_t* pose_vertex, const int32_t* point_vertex,
                                        const double* meas, const double* info, const double* offset, const double* kcam);
/* Sim3 bundle adjustment, the other half of the reference's sim3 type group: type 11 = EdgeSim3ProjectXYZ
 * (g2o/types/sim3/types_seven_dof_expmap.h:118-137, tag EDGE_PROJECT_SIM3_XYZ:EXPMAP; computeError :126-133), the reprojection of
 * a VertexSBAPointXYZ through the similarity camera of a VertexSim3Expmap, bound to the SAME single landmark slot beside a
 * type-10 (EdgeSim3) pose set only, on a handle of (pose, landmark) dimensions (7, 3) and a set of error_dim 2:
 *   e = z - cam_map(project(S.map(X))), Sim3::map(X) = s (r X) + t (sim3.h:144-146), project = (x / z, y / z)
 *   (slam3d/se3_ops.hpp:49-55), cam_map(v)[i] = v[i] focal_length[i] + principle_point[i] (:70-76) with the intrinsics of the
 *   OBSERVING vertex: intrinsics [n_cams][4] = (fx, fy, cx, cy), one row per entry of the pose table of g2ohip_pg_set_estimates
 *   (finite, fx and fy not zero; n_cams must equal that table's size whenever one is bound, checked here and again when
 *   g2ohip_pg_set_estimates changes the table).  meas [n][2], info [n][2x2], landmarks (x, y, z).
 * As in the whole landmark slot vertex 0 of the set is the POSE and vertex 1 the landmark -- the reference's edge has the point
 * as vertex 0 and the pose as vertex 1: J0 is [n][2x7] (the reference's _jacobianOplusXj), J1 [n][2x3] (_jacobianOplusXi).
 * The reference defines no Jacobian for this edge (linearizeOplus is commented out, :135); the device evaluates what g2o then
 * uses, the central differences of BaseBinaryEdge::linearizeOplus (g2o/core/base_binary_edge.hpp:132-201, delta = 1e-9): the
 * pose through oplusImpl (g2ohip_pg_set_sim3_fix_scale makes column 6 exactly zero), the point by plain addition
 * (g2o/types/sba/types_sba.h:151-155); the block of a fixed vertex is written as zeros.  Like the reference there is no guard
 * for a point on or behind the image plane.  Preconditions, validation (validate-then-commit) and error codes are those of
 * g2ohip_pg_set_landmark_edges; that entry and g2ohip_pg_set_landmark_camera_edges keep rejecting type 11 and any set beside a
 * type-10 pose set, and g2ohip_pg_set_edges rejects types 1 and 2 while a type-11 set is bound.  Everything after the binding
 * -- g2ohip_pg_set_landmark_estimates, g2ohip_pg_linearize / update / push / pop / discard_top, robust kernels,
 * g2ohip_clear_edge_sets -- acts on it unchanged; its kernels are timed in the pg_landmark_linearize slot. */
int g2ohip_pg_set_sim3_project_edges(g2ohip_solver* s, int set, const int32_t* pose_vertex, const int32_t* point_vertex,
                                     const double* meas, const double* info, int n_cams, const double* intrinsics);
/* SBA-format bundle adjustment, the reference's own format in g2o/types/sba/types_sba.{h,cpp} (tags VERTEX_CAM, VERTEX_XYZ,
 * EDGE_PROJECT_P2MC, EDGE_PROJECT_P2SC): pose type 12 of g2ohip_pg_set_edges = the VertexCam table, on a handle of (pose,
 * landmark) dimensions (6, 3).  A row of g2ohip_pg_set_estimates is then 7 doubles (tx, ty, tz, qx, qy, qz, qw), camera-to-world,
 * the order of SE3Quat::toVector (g2o/types/slam3d/se3quat.h:138-148) and of VertexCam::write (types_sba.cpp:114-131); a
 * non-finite value or a quaternion of norm 0 is G2OHIP_ERR_ARG, otherwise the row is stored as given.  The type-12 pose-pose set
 * is the anchor the landmark slot needs and holds ZERO edges (added with error_dim 6 and n = 0; its arrays may be NULL): n > 0
 * is G2OHIP_ERR_ARG -- EdgeSBACam and EdgeSBAScale are bound with g2ohip_pg_set_cam_edges, each as a set of its own beside it.
 * g2ohip_pg_update applies SBACam::update (g2o/types/sba/sbacam.h:101-117): t += x[0:3], qr = (x[3:6], sqrt(1 - |x[3:6]|^2)),
 * q <- q qr, then q / |q|; no sign flip.  A step with |x[3:6]| > 1 gives NaN, as in the reference.
 * Beside it, in the single landmark slot, type 13 = EdgeProjectP2MC (types_sba.h:161-196; error_dim 2, meas [n][2], info
 * [n][2x2]) or type 14 = EdgeProjectP2SC (types_sba.h:200-252; error_dim 3, meas [n][3] = (u, v, u_right), info [n][3x3]) over
 * landmarks (x, y, z).  With R = toRotationMatrix(q), w2n = [R' | -R' t] (sbacam.h:120-130), pc = w2n (X, 1) = (px, py, pz):
 *   mono   (types_sba.h:170-192)  e = ((fx px + cx pz) / pz, (fy py + cy pz) / pz) - z
 *   stereo (types_sba.h:209-247)  the same two rows and (fx (px - baseline) + cx pz) / pz - z[2]
 * intrinsics [n_cams][5] = (fx, fy, cx, cy, baseline), one row per entry of the pose table (finite, fx and fy not zero; n_cams
 * must equal that table's size whenever one is bound, checked here and again when g2ohip_pg_set_estimates changes the table).
 * The Jacobians are the reference's analytic ones (types_sba.cpp:249-328 stereo, :334-403 mono; dRdx/y/z of sbacam.h:162-181).
 * As in the whole landmark slot vertex 0 of the set is the CAMERA and vertex 1 the point -- the reference's edges have the point
 * as vertex 0 and the camera as vertex 1: J0 is [n][d x 6] (the reference's _jacobianOplusXj; columns t, then the quaternion's
 * x, y, z), J1 [n][d x 3] (_jacobianOplusXi), column-major; blocks of fixed vertices are written like the others.  There is no
 * guard for a point on or behind the image plane (pz <= 0): the reference aborts on the NaN there (types_sba.cpp:270-273,
 * :355-358), the device returns the NaN or infinity.  In the .g2o format these edges carry no information matrix: the reference
 * sets the identity (types_sba.cpp:204-244); here `info` is whatever the caller passes.
 * Preconditions, validation (validate-then-commit) and error codes are those of g2ohip_pg_set_landmark_edges.  Refused with
 * G2OHIP_ERR_ARG, in either order: landmark types 3-6 and 11 and any prior set beside a type-12 set; types 13 / 14 beside pose
 * types 1, 2 and 10.  Everything after the binding -- g2ohip_pg_set_landmark_estimates, g2ohip_pg_linearize / update / push /
 * pop / discard_top, robust kernels, do_schur 0 / 1, every linear_solver, g2ohip_clear_edge_sets -- acts on it unchanged; the
 * kernel is timed in the pg_landmark_linearize slot and has the staged and direct store forms of option pg_landmark_staged.
 * Not covered: VertexIntrinsics / EdgeProjectP2MC_Intrinsics (a three-vertex edge), priors beside a
 * type-12 set, more than one landmark set per handle (mono and stereo at once), sharded solves, the g2o plugin adapter (it keeps
 * these edges on its host path). */
int g2ohip_pg_set_cam_project_edges(g2ohip_solver* s, int set, int type, const int32_t* pose_vertex, const int32_t* point_vertex,
                                    const double* meas, const double* info, int n_cams, const double* intrinsics);
/* Stereo bundle adjustment over VertexSE3, the second half of the reference's icp type group: type 23 = Edge_XYZ_VSC
 * (g2o/types/icp/types_icp.h:376-413 computeError) over a VertexSBAPointXYZ and a VertexSCam (types_icp.h:253-366; mapPoint
 * :346-361), the edge of g2o/examples/sba/sba_demo.cpp and, beside Edge_V_V_GICP, of g2o/examples/icp/gicp_sba_demo.cpp.  A
 * VertexSCam IS a VertexSE3: the cameras are rows of the type-2 pose table (isometries [12], camera-to-world) and move by
 * VertexSE3::oplusImpl; the points are rows of the landmark table.  Bound to the SAME single landmark slot beside a type-2
 * (EdgeSE3) pose set only, which may hold zero edges (sba_demo has no pose-pose edge: its gauge is two fixed cameras; the set's
 * array pointers are non-null all the same), on a handle of (pose, landmark) dimensions (6, 3) and a set of error_dim 3.  With
 * X = (R, t) and the point l:
 *   q = R' (l - t),   e = ( fx q0 / q2 + cx,  fy q1 / q2 + cy,  fx (q0 - b) / q2 + cx ) - z,   z = (u_left, v_left, u_right)
 * kcam[5] = fx, fy, cx, cy, baseline b (required, finite, fx and fy not zero): ONE for the whole set -- VertexSCam::Kcam and
 * VertexSCam::baseline are static members in the reference.  meas [n][3], info [n][3x3].
 * As in the whole landmark slot vertex 0 of the set is the POSE (the camera) and vertex 1 the landmark -- the reference's edge has
 * the point as vertex 0 and the camera as vertex 1: J0 is [n][3 x 6] (the reference's _jacobianOplusXj), J1 [n][3 x 3]
 * (_jacobianOplusXi), column-major; blocks of fixed vertices are written like the others.
 * DELIBERATE DEVIATION: the reference differentiates this edge numerically (SCAM_ANALYTIC_JACOBIANS is commented out,
 * types_icp.h:31; base_binary_edge.hpp:132-201, central difference, delta = 1e-9), and the analytic code under that macro
 * (types_icp.cpp:242-321) belongs to an older parametrisation with world-frame translation -- it is not the derivative through
 * VertexSE3::oplusImpl (X <- X * fromVectorMQT(u), translation in the camera frame) and is not used.  The device writes the exact
 * derivative through that oplus, as types 18, 20, 21 and 22 do: with h a column of [-I | 2 [q]x | R'] (3 x 9: pose columns, then
 * point columns) the output column is
 *   ( fx (h0 q2 - q0 h2) / q2^2,  fy (h1 q2 - q1 h2) / q2^2,  fx (h0 q2 - (q0 - b) h2) / q2^2 ).
 * Second deviation: VertexSCam refreshes its cached w2n / w2i in oplusImpl only, so after a pop() the reference's cache lags the
 * restored estimate; the device always evaluates at the current estimate.  Like the reference there is no guard for a point on
 * or behind the image plane (q2 <= 0): infinities / NaNs.  The reference registers no .g2o tag for either type and its read /
 * write return false (types_icp.cpp:323-333): no file format is concerned.
 * Call after g2ohip_build_structure and g2ohip_pg_set_edges (G2OHIP_ERR_STATE otherwise).  G2OHIP_ERR_ARG: a pose set of a type
 * other than 2, a set of other dimensions than (3, 6, 3) or a unary one, a set bound in another slot, a null array, a negative
 * index or one outside the pose or landmark table, a hessian index that differs from the set's, a non-finite measurement,
 * information or intrinsic, fx == 0 or fy == 0 -- validated before anything is committed: a rejected call leaves the previous
 * binding usable.  A later call of this or of another landmark entry replaces the binding; g2ohip_clear_edge_sets drops it; a set
 * grown by g2ohip_update_structure makes g2ohip_pg_linearize return G2OHIP_ERR_STATE until it is bound again.  Everything after
 * the binding -- g2ohip_pg_set_landmark_estimates, g2ohip_pg_linearize / update / push / pop / discard_top,
 * g2ohip_pg_get_landmark_estimates, chi2 and robust kernels (set-level and per-edge), do_schur 0 / 1, use_graph -- acts on it
 * unchanged.  The GICP slot (type 15), the prior slot (type 9) and the offset slot (type 19) are independent of it: any of them
 * may be bound beside it on one handle.  The kernel (csrc/pg_scam.inc) is timed in the pg_landmark_linearize slot and has the
 * staged and direct store forms of option pg_landmark_staged.
 * Not covered: the g2o plugin adapter (it keeps these edges on its host path), sharded solves, per-camera intrinsics (the
 * reference has none: Kcam and baseline are static), more than one landmark set per handle. */
int g2ohip_pg_set_scam_edges(g2ohip_solver* s, int set, const int32_t* pose_vertex, const int32_t* point_vertex, const double* meas,
                             const double* info, const double* kcam);
/* ---- ... the SBA group's pose-pose constraints: odometry and loop closures between cameras, a known baseline -----------------
 * type 16 = EdgeSBACam (types_sba.h:287-334; tag EDGE_CAM): meas [n][7] = (tx, ty, tz, qx, qy, qz, qw), info [n][6x6], a binary
 *           set of error_dim 6.  e = (delta.t, delta.q.xyz), delta = Zinv * (Ci^-1 * Cj) with SE3Quat::inverse and operator*
 *           (se3quat.h:104-128), the normalizeRotation the product ends with included (sign flip when w < 0, then q / |q|).  The
 *           measurement is normalised as SE3Quat(Vector7d) does and inverted ONCE, at binding (setMeasurement).
 * type 17 = EdgeSBAScale (types_sba.h:340-359; tag EDGE_SCALE): meas [n][1], info [n][1], a binary set of error_dim 1.
 *           e = z - |t_j - t_i|.
 * Each type binds to ONE slot of its own beside a type-12 pose set of g2ohip_pg_set_edges (which stays an empty anchor): either
 * slot or both, with or without a type-13 / 14 projection set -- a pure VertexCam pose graph on a (6, 3) handle with no landmark
 * included.  Both vertices of a set are 6-dof cameras (added over the cameras' hessian indices, -1 = fixed); vi / vj index the
 * table of g2ohip_pg_set_estimates.  Many edges on one pair, and a pair in both orders, are legal; n = 0 is legal (arrays may
 * then be NULL).  The reference defines no Jacobian for these edges: J is BaseBinaryEdge's numeric one (base_binary_edge.hpp:
 * 132-201), column c of side v = (e(C_v (+) delta u_c) - e(C_v (+) -delta u_c)) / (2 delta), delta = 1e-9, (+) = SBACam::update;
 * the device evaluates exactly that, without fused multiply-adds.  J0, J1 are [n][d x 6] column-major; the block of a fixed
 * vertex is zeros; the rotation columns of an EdgeSBAScale block are exactly zero (the step does not reach t).
 * Call after g2ohip_build_structure and g2ohip_pg_set_edges (G2OHIP_ERR_STATE otherwise).  G2OHIP_ERR_ARG: a type other than 16 /
 * 17, a pose set of type 1, 2 or 10, a set of other dimensions or a unary one, a set bound in another slot, a null array with
 * n > 0, an index outside the pose table, a hessian index that differs from the set's, a non-finite value, a measurement
 * quaternion of norm 0 -- validated before anything is committed.  A later call replaces the slot's set and clears the data of
 * the set that leaves it.  While either slot is bound g2ohip_pg_set_edges refuses types 1, 2 and 10, and the other
 * g2ohip_pg_set_* entries refuse the slots' set ids.  g2ohip_pg_set_estimates with changed tables validates the sets again;
 * update / push / pop / discard_top, chi2 and robust kernels act as for any set; g2ohip_clear_edge_sets drops the bindings; a
 * set grown by g2ohip_update_structure makes g2ohip_pg_linearize return G2OHIP_ERR_STATE until it is bound again.  The kernels
 * are timed under the "pg_landmark_linearize" slot.  For tests only: g2ohip_device_array(109) = the stored inverse measurements
 * [n][7] of the EdgeSBACam slot.  Not covered: sharded solves, the g2o plugin adapter. */
int g2ohip_pg_set_cam_edges(g2ohip_solver* s, int set, int type, const int32_t* vi, const int32_t* vj, const double* meas,
                            const double* info);
/* ---- ... its unary pose priors: GPS fixes, an anchor on the first pose, surveyed checkpoints ------------------------
 * One UNARY edge set of the same handle beside the pose-pose set of g2ohip_pg_set_edges, in a slot of its own (independent of
 * the landmark slot: with or without a landmark set, do_schur 0 or 1; a later call replaces the binding):
 *   type 7 = EdgeSE2Prior over VertexSE2 (g2o/types/slam2d/edge_se2_prior.h:45-50 computeError): e = (Z^-1 X).toVector() =
 *            (Rz' (t - tz), normalize(theta - theta_z)), measurements [n][3] = (x, y, theta), information [n][3x3].  The
 *            reference compiles its analytic linearizeOplus out (edge_se2_prior.h:52-58) and differentiates numerically; the
 *            device writes the exact derivative with respect to VertexSE2::oplusImpl (vertex_se2.h:51-58), J = [Rz' 0; 0 1],
 *            which is what the disabled reference code states;
 *   type 8 = EdgeSE2XYPrior over VertexSE2 (edge_se2_xyprior.h:66-70 computeError, edge_se2_xyprior.cpp:60-63
 *            linearizeOplus): e = t - z, J = [1 0 0; 0 1 0], measurements [n][2], information [n][2x2];
 *            types 7 and 8 beside a type-1 pose set only;
 *   type 9 = EdgeSE3Prior over VertexSE3 (g2o/types/slam3d/edge_se3_prior.cpp:94-107 computeError / linearizeOplus,
 *            isometry3d_gradients.h:269-330 computeEdgeSE3PriorGradient, parameter_se3_offset.cpp:44-50) with ONE
 *            ParameterSE3Offset P for the whole set: E = Z^-1 X P, e = toVectorMQT(E) in the convention of type 2,
 *            measurements isometries [n][12] = R (column-major) | t, information [n][6x6], offset an isometry [12] or NULL
 *            for the identity (type 9 only, finite); beside a type-2 pose set only.
 * Edge set `set` was added as a unary set (v1 == NULL) with error_dim 3 / 2 / 6 over the poses' hessian indices (-1: a prior
 * on a fixed pose, legal as in g2o: it contributes to chi2 and nothing else); pose_vertex[k] indexes the pose table of
 * g2ohip_pg_set_estimates.  Call after g2ohip_build_structure and after g2ohip_pg_set_edges (G2OHIP_ERR_STATE otherwise).
 * G2OHIP_ERR_ARG: a wrong pairing of types, a set that is not unary or has other dimensions, the set already bound as the
 * pose-pose or landmark set, an offset with type 7 or 8, a non-finite offset, a null array, a pose_vertex out of range, a
 * hessian index that differs from the set's vertex 0 -- validated before anything is committed, as for the entries above;
 * g2ohip_pg_set_estimates with changed tables validates the prior set again.  g2ohip_pg_linearize then fills the set's
 * Jacobians and errors after the other two; update / push / pop / discard_top are not concerned (priors own no vertices).
 * Robust kernels of the set: g2ohip_set_robust_kernel(_per_edge) as for any set.  g2ohip_clear_edge_sets drops the binding;
 * a prior set grown by g2ohip_update_structure makes g2ohip_pg_linearize return G2OHIP_ERR_STATE until it is bound again.
 * The kernel is timed under the "pg_landmark_linearize" slot. */
int g2ohip_pg_set_prior_edges(g2ohip_solver* s, int set, int type, const int32_t* pose_vertex, const double* meas, const double* info,
                              const double* offset);
/* ---- ... its GICP correspondences: scan-to-scan and multi-scan registration --------------------------------------------
 * Type 15 = Edge_V_V_GICP over two VertexSE3 (g2o/types/icp/types_icp.h:167-244 computeError and the plane-to-plane
 * information, types_icp.cpp:41-55 dRidx / dRidy / dRidz, types_icp.cpp:124-202 read and the analytic linearizeOplus that
 * GICP_ANALYTIC_JACOBIANS selects).  ONE second pose-pose set of the same handle beside a type-2 set of g2ohip_pg_set_edges, in a
 * slot of its own: independent of the landmark slot (types 4-6, do_schur 0 or 1) and of the prior slot; a later call replaces
 * the binding.  The type-2 set may hold zero edges (a pure registration); its array pointers are non-null all the same.
 *   e = X0^-1 (X1 pos1) - pos0, J0 = [-I | dRidx p1t, dRidy p1t, dRidz p1t], J1 = [R | R dRid{x,y,z}' pos1], R = R0' R1,
 *   with respect to VertexSE3::oplusImpl; vertex 0 (vi) is the frame of pos0, vertex 1 (vj) the frame of pos1.
 * Edge set `set` was added as a binary set with error_dim 3 and both vertex dimensions 6 over the poses' hessian indices (-1 =
 * fixed); vi / vj index the pose table of g2ohip_pg_set_estimates.  Many edges on one vertex pair are the normal case, and a pair
 * may appear in both orders.  meas [n][6] = (pos0, pos1); info [n][3x3] column-major is the point-to-plane information; cov ==
 * NULL selects point-to-plane.  cov != NULL selects plane-to-plane (pl_pl = true): cov [n][18] = (cov0, cov1), 3x3 each, read by
 * their upper triangles, and every g2ohip_pg_linearize -- the error-only one included -- rewrites the set's information to
 * (cov0 + R cov1 R')^-1, so that g2ohip_chi2 and the robust weights see it as after the reference's computeError; info is then
 * only the value the set holds before the first evaluation.  The normals are not passed: they serve to build info / cov
 * (EdgeGICP::prec0 / cov0 / cov1, types_icp.h:90-158), which is host work (openslam_g2o_amd/gicp.py).
 * Call after g2ohip_build_structure and g2ohip_pg_set_edges (G2OHIP_ERR_STATE otherwise).  G2OHIP_ERR_ARG: a pose set of type 1,
 * 10 or 12, a set of other dimensions or a unary one, a set already bound in the pose-pose, landmark or prior slot, a null vi /
 * vj / meas / info, an index outside the pose table, a hessian index that differs from the set's, a non-finite value, a cov0 or
 * cov1 that is not symmetric positive definite (3x3 Cholesky on the host: cov0 + R cov1 R' is then invertible for every R) --
 * validated before anything is committed.  While a GICP set is bound g2ohip_pg_set_edges refuses types 1, 10 and 12, and the
 * landmark and prior entries refuse its set id.  (Of these, only type 12 on a zero-edge set is refused by the GICP rule alone:
 * types 1 and 10 never fit a handle of pose dimension 6, and a set bound in one slot never has the dimensions of another --
 * (6, 6, 6), (3, 6, 3), unary 6 and (3, 6, 6) -- so the set-id refusals name the cause and the dimension checks would refuse
 * the same calls.)  g2ohip_pg_set_estimates with changed tables validates the set again; update /
 * push / pop / discard_top are not concerned (the set owns no vertices); robust kernels as for any set; g2ohip_clear_edge_sets
 * drops the binding; a GICP set grown by g2ohip_update_structure makes g2ohip_pg_linearize return G2OHIP_ERR_STATE until it is
 * bound again.  The assembly walks the edge list of one Hessian block with a fixed small group of lanes (one lane for an
 * off-diagonal block), in edge order and without a cap on the list's length.
 * The kernel is timed under the "pg_landmark_linearize" slot.  The other half of the icp group, Edge_XYZ_VSC over VertexSCam,
 * binds beside it through g2ohip_pg_set_scam_edges (the joint graph of g2o/examples/icp/gicp_sba_demo.cpp).  Not covered: more
 * than one GICP set per handle, sharded solves, the g2o plugin adapter. */
int g2ohip_pg_set_gicp_edges(g2ohip_solver* s, int set, const int32_t* vi, const int32_t* vj, const double* meas, const double* info,
                             const double* cov);
/* ---- ... the pose-pose edges of a multi-sensor rig: relative poses measured between sensor frames mounted off the body -----
 * ONE second pose-pose set of the same handle beside the set of g2ohip_pg_set_edges, in an "offset slot" of its own: independent
 * of the landmark slot, the prior slot and the GICP slot; a later call replaces the binding.
 *   type 18 = EdgeSE2Offset over two VertexSE2 (g2o/types/slam2d/edge_se2_offset.cpp:96-100 computeError,
 *             parameter_se2_offset.cpp:76-86), beside a type-1 pose set only: e = (D.t, D.angle), D = Z^-1 (Xi Pi)^-1 (Xj Pj) with
 *             SE2's products and normalize_theta as se2.h; meas [n][3] = (x, y, theta), info [n][3x3], offsets [n_params][3] =
 *             (x, y, theta).  DELIBERATE DEVIATION: the reference defines no Jacobian for this edge and differentiates
 *             numerically (base_binary_edge.hpp:132-201, delta = 1e-9); the device writes the exact derivative with respect to
 *             VertexSE2::oplusImpl, as for type 7: with si = ti + R(thi) pi, sj = tj + R(thj) pj, M = R(thz + thi + ai)',
 *             J = [0 -1; 1 0]: d e_t/d ti = -M, d e_t/d tj = M, d e_t/d thi = -J M (sj - si) - M J R(thi) pi, d e_t/d thj =
 *             M J R(thj) pj, d e_th/d thi = -1, d e_th/d thj = 1;
 *   type 19 = EdgeSE3Offset over two VertexSE3 (g2o/types/slam3d/edge_se3_offset.cpp:100-130, parameter_se3_offset.cpp:44-50),
 *             beside a type-2 pose set only: e = toVectorMQT(Z^-1 (Xi Pi)^-1 (Xj Pj)) in the convention of type 2, Jacobians
 *             the full computeEdgeSE3Gradient (isometry3d_gradients.h:86-192, its non-__clang__ branch) with A = Z^-1 Pi^-1,
 *             B = Xi^-1 Xj, C = Pj; meas isometries [n][12] = R (column-major) | t, info [n][6x6], offsets [n_params][12].
 * Edge set `set` was added as a binary set with error_dim 3 / 6 and both vertex dimensions 3 / 6 over the poses' hessian indices
 * (-1 = fixed); vi / vj index the pose table of g2ohip_pg_set_estimates; param_from[k] / param_to[k] name the rows of `offsets`
 * that are the sensor frame on vertex 0 / vertex 1 of edge k.  n = 0 is legal (the edge arrays may then be NULL); many edges on
 * one vertex pair are legal, and so is a pair in both orders.
 * Call after g2ohip_build_structure and g2ohip_pg_set_edges (G2OHIP_ERR_STATE otherwise).  G2OHIP_ERR_ARG: a wrong pairing of
 * type and pose set, a set of other dimensions or a unary one, a set already bound in another slot, a null array with n > 0,
 * n_params < 1 or a null offsets table, a parameter index outside [0, n_params), a vertex index outside the pose table, a
 * hessian index that differs from the set's, a non-finite value (for type 19 that covers the columns of every rotation part)
 * -- validated before anything is committed: a rejected call leaves the previous binding usable.  While a set is bound the
 * other g2ohip_pg_set_* entries refuse its set id and g2ohip_pg_set_edges refuses pose types that do not fit.
 * g2ohip_pg_set_estimates with changed tables validates the set again; update / push / pop / discard_top are not concerned (the
 * set owns no vertices); robust kernels and chi2 as for any set; g2ohip_clear_edge_sets drops the binding; a set grown by
 * g2ohip_update_structure makes g2ohip_pg_linearize return G2OHIP_ERR_STATE until it is bound again.
 * The kernels are timed under the "pg_landmark_linearize" slot.  Not covered: more than one offset set per handle, sharded
 * solves, the g2o plugin adapter, EdgeSE2PointXYOffset. */
int g2ohip_pg_set_offset_edges(g2ohip_solver* s, int set, int type, const int32_t* vi, const int32_t* vj, const int32_t* param_from,
                               const int32_t* param_to, const double* meas, const double* info, int n_params, const double* offsets);
/* ---- ... bearing-only observations of 2-D point landmarks: what g2o_simulator2d's bearing sensor writes ---------------------
 * ONE set of EdgeSE2PointXYBearing (type 20; tag EDGE_BEARING_SE2_XY, g2o/types/slam2d/edge_se2_pointxy_bearing.h:43-50
 * computeError, edge_se2_pointxy_bearing.cpp:56-66 read / write) over a VertexSE2 and a VertexPointXY, beside a type-1 pose set
 * only, in a "bearing slot" of its own: independent of the prior and offset slots, and WITH OR WITHOUT an EdgeSE2PointXY set
 * (type 3) in the landmark slot -- both sets index the one landmark table of g2ohip_pg_set_landmark_estimates.  A later call
 * replaces the binding.  With pose (x, y, th), landmark (lx, ly), c = cos th, s = sin th, dx = lx - x, dy = ly - y:
 *   deltax = c dx + s dy,  deltay = -s dx + c dy,  e = normalize_theta(z - atan2(deltay, deltax))     (error dimension 1)
 * DELIBERATE DEVIATION: the reference defines no linearizeOplus for this edge and differentiates numerically
 * (base_binary_edge.hpp:132-201, central difference, delta = 1e-9), which across the +-pi wrap of the error is wrong by
 * 2 pi / (2 delta); the device writes the exact derivative with respect to VertexSE2::oplusImpl (t += u[0:2], th += u[2]) and
 * VertexPointXY::oplusImpl, as for types 7 and 18: with r2 = dx dx + dy dy
 *   J0 = (-dy / r2, dx / r2, 1)  [1 x 3],   J1 = (dy / r2, -dx / r2)  [1 x 2].
 * Like the reference there is no guard for a landmark on top of the pose (r2 == 0): infinities / NaNs.
 * Edge set `set` was added as a binary set with error_dim 1 over the poses' and the landmarks' hessian indices (-1 = fixed) on a
 * handle of (pose, landmark) dimensions (3, 2); pose_vertex indexes the table of g2ohip_pg_set_estimates, point_vertex the table
 * of g2ohip_pg_set_landmark_estimates; meas [n][1] the measured angles, info [n][1].  n = 0 is legal (the arrays may then be
 * NULL) and replaces the binding.
 * Call after g2ohip_build_structure and g2ohip_pg_set_edges (G2OHIP_ERR_STATE otherwise).  G2OHIP_ERR_ARG: a pose set of a type
 * other than 1, a set of other dimensions or a unary one, a set already bound in another slot, a null array with n > 0, an index
 * outside the pose or landmark table, a hessian index that differs from the set's, a non-finite value -- validated before
 * anything is committed: a rejected call leaves the previous binding usable.  While a set is bound the other g2ohip_pg_set_*
 * entries refuse its set id and g2ohip_pg_set_edges refuses pose types other than 1.  g2ohip_pg_set_estimates and
 * g2ohip_pg_set_landmark_estimates with changed tables validate the set again; g2ohip_pg_linearize without a landmark table
 * returns G2OHIP_ERR_STATE; update / push / pop / discard_top move the landmark table as for a type-3 set; robust kernels, chi2,
 * do_schur 0 / 1 as for any set; g2ohip_clear_edge_sets drops the binding; a set grown by g2ohip_update_structure makes
 * g2ohip_pg_linearize return G2OHIP_ERR_STATE until it is bound again.
 * The kernel is timed under the "pg_landmark_linearize" slot.  Not covered: EdgeSE2PointXYOffset (in the reference its
 * computeError reads the cache's w2lMatrix, the inverse of the vertex estimate WITHOUT the offset, while its linearizeOplus mixes
 * the offset's rotation into one column, parameter_se2_offset.cpp:87-96: which of the two is meant has to be decided first),
 * more than one bearing set per handle, sharded solves, the g2o plugin adapter, a 3-D counterpart (the reference has none).
 * EdgeSE2PointXYCalib: g2ohip_pg_set_pointxy_calib_edges below. */
int g2ohip_pg_set_bearing_edges(g2ohip_solver* s, int set, const int32_t* pose_vertex, const int32_t* point_vertex,
                                const double* meas, const double* info);
/* ---- ... laser self-calibration (sclam2d): scan-match constraints that also estimate the sensor's mounting offset -----------
 * ONE group of EdgeSE2SensorCalib (type 21; tag EDGE_SE2_CALIB, g2o/types/sclam2d/edge_se2_sensor_calib.h:45-59 computeError /
 * setMeasurement, edge_se2_sensor_calib.cpp read / write), the edge of g2o/examples/calibration_odom_laser: a THREE-vertex edge
 * over two VertexSE2 poses x1, x2 and the laser offset L, an ordinary VertexSE2 -- all three are rows of the one pose table of
 * g2ohip_pg_set_estimates, so g2ohip_pg_update / push / pop / discard_top / get_estimates carry L like any pose.  Beside a type-1
 * pose set only, in a "calibration slot" of its own: independent of the landmark, prior, offset and bearing slots; a later call
 * replaces the binding.
 *   e = toVector(Z^-1 * ((x1 * L)^-1 * x2 * L))          (error dimension 3, SE2's products and normalize_theta as se2.h)
 * Z^-1 is computed per evaluation from the measurement, as _inverseMeasurement = m.inverse() would give it.
 * DELIBERATE DEVIATION: the reference defines no linearizeOplus for this edge and differentiates numerically
 * (base_multi_edge.hpp:63-116, central difference, delta = 1e-9); the device writes the exact derivative with respect to
 * VertexSE2::oplusImpl (t += u[0:2], th += u[2]), as for types 7, 18 and 20: with Q = R(-(thz + th1 + thl)), J = [0 -1; 1 0],
 * tA = t1 + R(th1) tl, tB = t2 + R(th2) tl
 *   d e_t / d t1 = -Q                     d e_t / d th1 = -J Q (tB - tA) - Q J R(th1) tl     d e_th / d th1 = -1
 *   d e_t / d t2 =  Q                     d e_t / d th2 =  Q J R(th2) tl                     d e_th / d th2 =  1
 *   d e_t / d tl =  Q (R(th2) - R(th1))   d e_t / d thl = -J Q (tB - tA)                     d e_th / d thl =  0
 * The Jacobian block of a fixed vertex (hessian index -1) is written as zeros.
 * The edge is the three binary sets g2ohip_set_edge_set_parts documents for three vertices, added by the caller with error_dim 3
 * over the vertices' hessian indices (-1 = fixed), all of the same edge count, on a handle of pose dimension 3:
 *   set_ij  (i, j)  parts 0
 *   set_il  (i, l)  parts G2OHIP_PART_NO_VERTEX0 | G2OHIP_PART_NO_VERTEX1 | G2OHIP_PART_NO_CHI2
 *   set_jl  (j, l)  parts G2OHIP_PART_NO_VERTEX0 | G2OHIP_PART_NO_CHI2
 * They are bound and released as one group and share Jacobians, information and errors on the device (as the sets of
 * g2ohip_ba_set_inverse_depth_edges do).  vi / vj / vl index the pose table; meas [n][3] = (x, y, theta); info [n][3x3], NULL =
 * identity.  Robust kernels: set the same kernel on all three sets.  L is a neighbour of every edge: the Hessian gets a dense
 * block row, and one diagonal block receives a term from every edge.
 * G2OHIP_ERR_STATE: a call before g2ohip_build_structure or before g2ohip_pg_set_edges, a set that carries per-edge robust
 * kernels.  G2OHIP_ERR_ARG: a bad or repeated set id, a pose set of a type other than 1, wrong dimensions, parts or edge
 * counts, a unary set, a set already bound in another slot, null vi / vj / vl / meas, a non-finite value, an index outside the
 * pose table, a hessian index that differs from the sets' own, vl[k] == vi[k], vl[k] == vj[k] or vi[k] == vj[k] -- validated
 * before anything is committed: a rejected call leaves the previous binding usable.  While the group is bound the other
 * g2ohip_pg_set_* entries refuse its set ids and g2ohip_pg_set_edges refuses pose types other than 1.
 * g2ohip_pg_set_estimates with changed tables validates the group again; g2ohip_clear_edge_sets drops the binding, and so does a
 * g2ohip_update_structure that grows one of the three sets or the pose set (bind again after growth).
 * The kernel is timed under the "pg_landmark_linearize" slot.  EdgeSE2OdomDifferentialCalib and VertexOdomDifferentialParams, the
 * other half of that example's graph: g2ohip_pg_set_odom_calib_edges below, in a slot of its own beside this one.  Not covered:
 * more than one calibration group of the same kind per handle, sharded solves, the g2o plugin adapter. */
int g2ohip_pg_set_sensor_calib_edges(g2ohip_solver* s, int set_ij, int set_il, int set_jl, const int32_t* vi, const int32_t* vj,
                                     const int32_t* vl, const double* meas, const double* info);
/* ---- ... odometry self-calibration (sclam2d): wheel-velocity constraints that also estimate the differential drive --------------
 * ONE group of EdgeSE2OdomDifferentialCalib (type 22; tag EDGE_SE2_ODOM_DIFFERENTIAL_CALIB,
 * g2o/types/sclam2d/edge_se2_odom_differential_calib.h:45-63 computeError, edge_se2_odom_differential_calib.cpp:39-61 read /
 * write, OdomConvert::convertToMotion g2o/types/sclam2d/odometry_measurement.cpp:95-117): a THREE-vertex edge over two VertexSE2
 * poses x1, x2 and a VertexOdomDifferentialParams p = (k_l, k_r, b) -- all three are rows of the one pose table of
 * g2ohip_pg_set_estimates.  Beside a type-1 pose set only (which may hold ZERO edges: the graph of
 * g2o/examples/calibration_odom_laser has no EdgeSE2), in the "odometry-calibration slot": independent of the landmark, prior,
 * offset, bearing and type-21 calibration slots -- both calibration groups may be bound at once -- a later call replaces the binding.
 *   vl' = vl p[0]   vr' = vr p[1]   D = vr' - vl'   S = vl' + vr'   b = p[2]
 *   |D| > 1e-7:  Rc = b 0.5 (S / D)   th = (D / b) dt   K = SE2(Rc sin th, Rc - Rc cos th, th)
 *   otherwise:   K = SE2(0.5 S dt, 0, 0)
 *   e = toVector(K^-1 * x1^-1 * x2)                        (error dimension 3; b = 0 gives non-finite values, as in the reference)
 * ADDITIVE ROWS.  VertexOdomDifferentialParams::oplusImpl is estimate += v with no angle wrap
 * (vertex_odom_differential_params.h:43-46).  While the group is bound every row named by vp is an additive row of the table:
 * g2ohip_pg_update adds all three components of its step; every other row moves as VertexSE2::oplusImpl.  The binding is the
 * declaration.  A row is read one way only: the call refuses (G2OHIP_ERR_ARG) a vp row that is also a vi / vj of this group or a
 * vertex of any set bound on the handle (pose set, prior, offset, bearing / landmark pose side, all three columns of the type-21
 * group), and while the group is bound the other g2ohip_pg_set_* entries refuse an index that names an additive row.  Once the
 * group is released the rows are ordinary VertexSE2 rows again.  push / pop / discard_top / get_estimates copy rows.
 * DELIBERATE DEVIATION: the reference defines no linearizeOplus for this edge and differentiates numerically
 * (base_multi_edge.hpp:63-116, central difference, delta = 1e-9); the device writes the exact derivative OF THE BRANCH TAKEN, as
 * for types 7, 18, 20 and 21: with Q = R(-(th + th1)), J = [0 -1; 1 0], e_t the translational error
 *   d e_t / d t1 = -Q     d e_t / d th1 = -J Q (t2 - t1)     d e_th / d th1 = -1
 *   d e_t / d t2 =  Q     d e_t / d th2 = 0                  d e_th / d th2 =  1
 *   d e_t / d q  = -R(-th) (dx/dq, dy/dq) - J e_t dth/dq     d e_th / d q   = -dth/dq            for q of (k_l, k_r, b)
 *   turning:   dRc/dk_l = b vl vr' / D^2   dRc/dk_r = -b vr vl' / D^2   dRc/db = Rc / b
 *              dth/dk_l = -vl dt / b       dth/dk_r = vr dt / b         dth/db = -th / b
 *              dx/dq = sin th dRc/dq + Rc cos th dth/dq     dy/dq = (1 - cos th) dRc/dq + Rc sin th dth/dq
 *   straight:  dx/dk_l = 0.5 vl dt   dx/dk_r = 0.5 vr dt   every other entry 0 (the column of b is zero, as the reference's
 *              difference gives it while both probes stay inside the branch)
 * Within 1e-9 max(|vl|, |vr|) of |D| = 1e-7 the reference's probes fall on different branches and its Jacobian is meaningless; the
 * device's is that of the branch the estimate is on.  The Jacobian block of a fixed vertex (hessian index < 0) is zeros.
 * The edge is the three binary sets of g2ohip_set_edge_set_parts, error_dim 3, equal edge counts, pose dimension 3:
 *   set_ij  (i, j)  parts 0
 *   set_ip  (i, p)  parts G2OHIP_PART_NO_VERTEX0 | G2OHIP_PART_NO_VERTEX1 | G2OHIP_PART_NO_CHI2
 *   set_jp  (j, p)  parts G2OHIP_PART_NO_VERTEX0 | G2OHIP_PART_NO_CHI2
 * bound and released as one group, sharing Jacobians, information and errors on the device.  vi / vj / vp index the pose table
 * (vp is per edge: several parameter vertices, one per robot, need nothing more); meas [n][3] = (vl, vr, dt); info [n][3x3], NULL =
 * identity.  Robust kernels: the same kernel on all three sets.  Each parameter vertex is a neighbour of every one of its edges: a
 * dense block row, as the laser offset's.
 * G2OHIP_ERR_STATE: a call before g2ohip_build_structure or before g2ohip_pg_set_edges, a set that carries per-edge robust
 * kernels.  G2OHIP_ERR_ARG: a bad or repeated set id, a pose set of a type other than 1, wrong dimensions, parts or edge counts, a
 * unary set, a set bound in another slot (the type-21 group's included; that group's entry refuses this one's), null vi / vj / vp /
 * meas, a non-finite value, an index outside the pose table, a hessian index that differs from the sets' own, a vertex named twice
 * in an edge, a row read both ways (above) -- validated before anything is committed: a rejected call leaves the previous binding
 * usable.  g2ohip_pg_set_estimates with changed tables validates the group again; g2ohip_clear_edge_sets drops the binding, and so
 * does a g2ohip_update_structure that grows one of the three sets or the pose set.  Captured launch sequences (use_graph) are
 * dropped at binding and at release.  The kernel is timed under the "pg_landmark_linearize" slot.  Not covered: sharded solves,
 * the g2o plugin adapter. */
int g2ohip_pg_set_odom_calib_edges(g2ohip_solver* s, int set_ij, int set_ip, int set_jp, const int32_t* vi, const int32_t* vj,
                                   const int32_t* vp, const double* meas /* [n][3] = vl, vr, dt */,
                                   const double* info /* [n][3x3], NULL = identity */);
/* ---- ... landmark self-calibration (slam2d): point observations that also estimate the sensor's mounting offset ---------------
 * ONE group of EdgeSE2PointXYCalib (type 24; tag EDGE_SE2_XY_CALIB, g2o/types/slam2d/edge_se2_pointxy_calib.h:46-52 computeError,
 * edge_se2_pointxy_calib.cpp read / write): a THREE-vertex edge over a VertexSE2 pose x1 = (t1, th1), a VertexPointXY landmark l
 * and the calibration c = (tc, thc), an ordinary VertexSE2.  The pose and the calibration vertex are rows of the pose table of
 * g2ohip_pg_set_estimates -- so g2ohip_pg_update / push / pop / discard_top / get_estimates carry c like any pose --, the landmark
 * is a row of the landmark table of g2ohip_pg_set_landmark_estimates: the one group that spans both tables.  Beside a type-1 pose
 * set only (which may hold ZERO edges), in a slot of its own: independent of the landmark (type 3), prior, offset, bearing, type-21
 * and type-22 slots, all of which read the one landmark table and the one pose table; a later call replaces the binding.
 *   a = x1 * c,  w = a^-1,  e = R(w.th) l + w.t - z        (error dimension 2; SE2's product and inverse with normalize_theta, se2.h)
 * DELIBERATE DEVIATION: the reference defines no linearizeOplus for this edge and differentiates numerically
 * (base_multi_edge.hpp:63-116, central difference, delta = 1e-9); the device writes the exact derivative with respect to
 * VertexSE2::oplusImpl (t += u[0:2], th += u[2]) and VertexPointXY::oplusImpl, as for types 7, 18, 20, 21 and 22: with
 * Q = R(-(th1 + thc)), J = [0 -1; 1 0], d = l - t1 - R(th1) tc
 *   d e / d t1 = -Q          d e / d th1 = -J Q d - Q J R(th1) tc        (J_pose  2 x 3)
 *   d e / d l  =  Q                                                      (J_point 2 x 2)
 *   d e / d tc = -R(-thc)    d e / d thc = -J Q d                        (J_calib 2 x 3)
 * The Jacobian block of a fixed vertex (hessian index -1) is written as zeros.  No guard beyond the reference's.
 * The edge is the three binary sets of g2ohip_set_edge_set_parts, added by the caller with error_dim 2 over the vertices' hessian
 * indices (-1 = fixed), all of the same edge count, on a handle of (pose, landmark) dimensions (3, 2):
 *   set_pl  (v0 = pose,     v1 = landmark)  parts 0                                                         dims (3, 2)
 *   set_pc  (v0 = pose,     v1 = calib)     parts G2OHIP_PART_NO_VERTEX0 | G2OHIP_PART_NO_VERTEX1 | G2OHIP_PART_NO_CHI2  dims (3, 3)
 *   set_lc  (v0 = landmark, v1 = calib)     parts G2OHIP_PART_NO_VERTEX0 | G2OHIP_PART_NO_CHI2              dims (2, 3)
 * (the generic assembly takes the landmark on either side of a set; a set all of whose landmarks are fixed has no landmark
 * dimension and is refused).  They are bound and released as one group and share their buffers on the device: set_pl owns J_pose,
 * J_point, the information and the errors, set_lc owns J_calib, every other pointer aliases one of those (18 + 2 doubles per edge
 * leave the producer).  pose_vertex / calib_vertex index the pose table, point_vertex the landmark table; meas [n][2]; info
 * [n][2x2], NULL = identity.  Robust kernels: set the same kernel on all three sets.  The calibration vertex is a neighbour of
 * every edge: the pose Hessian gets a dense block row, and Hpl a dense row of (calib, landmark) blocks, each with as many terms as
 * the landmark has observations (the generic (3, 2) Schur path has no cap on the edges of a vertex pair).
 * G2OHIP_ERR_STATE: a call before g2ohip_build_structure or before g2ohip_pg_set_edges, a set that carries per-edge robust
 * kernels.  G2OHIP_ERR_ARG: a bad or repeated set id, a set bound in another slot, a pose set of a type other than 1, wrong
 * dimensions, parts or edge counts, a unary set, null pose_vertex / point_vertex / calib_vertex / meas, a non-finite value, an
 * index outside its table, a hessian index that differs from the sets' own (pose and calibration vertex against the pose table's,
 * the landmark against the landmark table's), pose_vertex[k] == calib_vertex[k], a pose or calibration row that is an additive
 * row of a bound type-22 group (and that group's entry refuses a parameter row this group reads) -- validated before anything is
 * committed: a rejected call leaves the previous binding usable.  While the group is bound the other g2ohip_pg_set_* entries
 * refuse its set ids and g2ohip_pg_set_edges refuses pose types other than 1.  g2ohip_pg_linearize without a landmark table
 * returns G2OHIP_ERR_STATE.  g2ohip_pg_set_estimates / g2ohip_pg_set_landmark_estimates with changed tables validate the group
 * again; g2ohip_clear_edge_sets drops the binding.  g2ohip_update_structure refuses structures with landmarks, so the group
 * cannot grow.  Captured launch sequences (use_graph) are dropped at binding and at release.  With do_schur = 0 the solver
 * factorises Hpp alone, as for every landmark set.  The kernel is timed under the "pg_landmark_linearize" slot.
 * Not covered: EdgeSE2PointXYOffset (see g2ohip_pg_set_bearing_edges), more than one such group per handle, sharded solves, the
 * g2o plugin adapter. */
int g2ohip_pg_set_pointxy_calib_edges(g2ohip_solver* s, int set_pl, int set_pc, int set_lc, const int32_t* pose_vertex,
                                      const int32_t* point_vertex, const int32_t* calib_vertex, const double* meas /* [n][2] */,
                                      const double* info /* [n][2x2], NULL = identity */);
int g2ohip_pg_set_landmark_estimates(g2ohip_solver* s, int n_points, const double* points, const int32_t* hidx);
int g2ohip_pg_get_landmark_estimates(g2ohip_solver* s, double* points);

/* ---- narrow seam: g2o::LinearSolver<MatrixType> ------------------------------------------- */

/* LinearSolver ctor for MatrixType = block_dim x block_dim. */
int g2ohip_ls_create(g2ohip_linear_solver** out, int block_dim, int device);
void g2ohip_ls_destroy(g2ohip_linear_solver* ls);
/* LinearSolver::init(), linear_solver_csparse.h:97-104: drop the symbolic factorisation. */
int g2ohip_ls_init(g2ohip_linear_solver* ls);
/* LinearSolver::solve(A, x, b), linear_solver_csparse.h:106-142.  A: symmetric, upper blocks
 * only (rowidx[q] <= column), ascending rows per column, values [nnzb][bd x bd] column-major,
 * diagonal blocks fully stored.  Same pattern between init() calls (linear_solver.h:86-105).
 * x, b: host vectors of n_blocks*block_dim.  G2OHIP_OK | G2OHIP_NOT_PD | error. */
int g2ohip_ls_solve(g2ohip_linear_solver* ls, int n_blocks, const int32_t* colptr, const int32_t* rowidx,
                    const double* values, double* x, const double* b);
/* LinearSolver::solvePattern(spinv, blockIndices, A), linear_solver.h:71 / linear_solver_csparse.h:190-221 (factorise,
 * then MarginalCovarianceCholesky::computeCovariance): blocks (rows[i], cols[i]) of A^-1, out [n_req][bd x bd]
 * column-major.  Blocks inside the pattern of the factor come from one sparse-inverse pass over the frontal matrices,
 * the others from unit right-hand sides.  G2OHIP_OK | G2OHIP_NOT_PD | error. */
int g2ohip_ls_solve_pattern(g2ohip_linear_solver* ls, int n_blocks, const int32_t* colptr, const int32_t* rowidx,
                            const double* values, int n_req, const int32_t* rows, const int32_t* cols, double* out);
int g2ohip_ls_get_stats(g2ohip_linear_solver* ls, g2ohip_stats* out);
int g2ohip_ls_set_option(g2ohip_linear_solver* ls, const char* name, double value);

#ifdef __cplusplus
}
#endif
#endif /* G2OHIP_H */
