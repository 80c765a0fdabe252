// Device-resident replacement of g2o::BlockSolver<BlockSolverTraits<p,l>>
//   /root/reference/g2o/core/block_solver.h:98-178, block_solver.hpp (all)
// over flat index/Jacobian arrays instead of the pointer-chasing SparseBlockMatrix
// (sparse_block_matrix.h:61-220: vector<map<int,Block*>>, one heap block per tile).
//
// Data layout in HBM (all fp64 column-major blocks, int32 indices):
//   Hpp, Hschur : block-CCS upper triangle, ascending rows per column, values [nnzb][p*p]
//   Hpl         : block-CCS by landmark column (== _HplCCS, block_solver.h:157), rows = pose
//                 index ascending, values [nnzb][p*l]
//   Hll, Dinv   : dense [nL][l*l];  b, x : [nP*p | nL*l]  (block_solver.hpp:551-557)
// Scatter reductions (many edges -> one vertex block, many landmarks -> one Hschur block)
// are done destination-major from precomputed contributor lists: deterministic, no fp64
// atomics, same summation order as the reference's serial loops.
#pragma once
#include <cstring>
#include <initializer_list>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "common.h"
#include "comm.h"
#include "block_pcg.h"
#include "sparse_cholesky.h"

namespace g2ohip {

struct EdgeSet {
  int d = 0, n = 0, dim0 = 0, dim1 = 0;
  bool unary = false;
  int parts = 0;           // G2OHIP_PART_* bits: what of its quadratic form the set does NOT contribute (set_edge_set_parts)
  std::vector<int> v0, v1;
  int kernel_kind = 0;
  double delta = 1.0;
  DevBuf<double> rk;       // per-edge robust kernels [n][2] = (kind, delta), or empty: the set-level pair above (set_robust_kernel_per_edge)
  // per-iteration data (device); either own buffers or caller-owned device pointers
  const double *J0 = nullptr, *J1 = nullptr, *omega = nullptr, *err = nullptr;
  DevBuf<double> own_J0, own_J1, own_omega, own_err;
  bool has_data = false;   // Jacobians + information + errors available for build_system
  bool external = false;   // the arrays belong to the caller (set_edge_data on_device): they may change behind the solver's back
  bool has_err = false;    // errors + information available (enough for chi2)
  // destination-major contributor lists
  DevBuf<int> vp_ptr, vp_ent, vl_ptr, vl_ent;  // per pose / per landmark: (edge << 1 | side)
  DevBuf<int> vp_act;                          // poses with at least one entry (when that is not all of them)
  int n_vp_act = 0;
  std::vector<int> h_vp_ent, h_vl_ent;         // host copies (pose- / landmark-major copies of per-edge inputs)
  std::vector<int> h_vl_ptr;                   // ... and the landmark list bounds (lane slots of the fused Schur tiles)
  DevBuf<int> op_dst, op_ptr, op_ent;          // Hpp off-diagonal blocks: dest block id, (edge << 1 | transposed)
  DevBuf<int> ol_dst, ol_ptr, ol_ent;          // Hpl blocks
  int n_op = 0, n_ol = 0;
  long n_vp_ent = 0, n_vl_ent = 0;
  bool touches_pose = false, touches_lm = false, first_pose = false, first_lm = false, first_op = false, first_ol = false;
};

struct SolverTimes {
  double quadratic = 0, schur = 0, numeric = 0, linsolve = 0, backsub = 0, residuals = 0, linearize = 0, update = 0;
};

class BlockSolver {
 public:
  BlockSolver(int p, int l, int device);
  ~BlockSolver();

  void init();
  void clear_edge_sets();
  int add_edge_set(int d, int n, const int* v0, const int* v1);
  void set_edge_set_parts(int set, int parts);
  void add_schur_pattern(int n, const int* rows, const int* cols);
  void build_structure(int nP, int nL, bool do_schur);
  bool update_structure(int new_poses, int set, int n, const int* v0, const int* v1);
  void set_edge_data(int set, const double* J0, const double* J1, const double* omega, const double* err, bool on_device);
  void set_edge_errors(int set, const double* err);
  void set_robust_kernel(int set, int kind, double delta);
  void set_robust_kernel_per_edge(int set, const int* kind, const double* delta);
  void build_system();
  double chi2();
  void set_lambda(double lambda, bool backup);
  void set_lambda_split(double lambda_pose, double lambda_landmark, bool backup);
  void restore_diagonal();
  double max_diagonal();
  double compute_scale(double lambda);
  int solve();                 // 0 ok, 1 not PD
  void solve_schur();
  int solve_reduced();
  // multi-GPU split of solve_reduced (openslam_g2o_amd/distributed.py): own subtrees -> exchange of the
  // subtree-root update matrices/vectors -> shared top of the tree + back down -> exchange of x_p
  void set_partition(int rank, int world);
  void solve_reduced_local();
  void solve_reduced_shared();
  int solve_reduced_finish();
  void partition_info(int* pose_owner, int* block_consumer);
  int compute_marginals(int n, const int* rows, const int* cols, double* out);
  void copy_diagonal(double* host);
  void copy_edge_data(int set, double* J0, double* J1, double* err);
  void pg_set_edges(int set, int type, const int* vi, const int* vj, const double* meas, const double* info);
  void pg_set_sim3_fix_scale(bool fix_scale);
  void pg_set_estimates(int nv, const double* poses, const int* hidx);
  void pg_get_estimates(double* poses);
  void pg_set_landmark_edges(int set, int type, const int* pose_vertex, const int* point_vertex, const double* meas, const double* info,
                             const double* offset);
  void pg_set_landmark_camera_edges(int set, int type, const int* pose_vertex, const int* point_vertex, const double* meas,
                                    const double* info, const double* offset, const double* kcam);
  void pg_set_sim3_project_edges(int set, const int* pose_vertex, const int* point_vertex, const double* meas, const double* info,
                                 int n_cams, const double* intrinsics);
  void pg_set_cam_project_edges(int set, int type, const int* pose_vertex, const int* point_vertex, const double* meas,
                                const double* info, int n_cams, const double* intrinsics);
  void pg_set_scam_edges(int set, const int* pose_vertex, const int* point_vertex, const double* meas, const double* info,
                         const double* kcam);
  void pg_set_prior_edges(int set, int type, const int* pose_vertex, const double* meas, const double* info, const double* offset);
  void pg_set_gicp_edges(int set, const int* vi, const int* vj, const double* meas, const double* info, const double* cov);
  void pg_set_offset_edges(int set, int type, const int* vi, const int* vj, const int* param_from, const int* param_to, const double* meas,
                           const double* info, int n_params, const double* offsets);
  void pg_set_bearing_edges(int set, const int* pose_vertex, const int* point_vertex, const double* meas, const double* info);
  void pg_set_sensor_calib_edges(int set_ij, int set_il, int set_jl, const int* vi, const int* vj, const int* vl, const double* meas,
                                 const double* info);
  void pg_set_odom_calib_edges(int set_ij, int set_ip, int set_jp, const int* vi, const int* vj, const int* vp, const double* meas,
                               const double* info);
  void pg_set_pointxy_calib_edges(int set_pl, int set_pc, int set_lc, const int* pose_vertex, const int* point_vertex,
                                  const int* calib_vertex, const double* meas, const double* info);
  void pg_set_cam_edges(int set, int type, const int* vi, const int* vj, const double* meas, const double* info);
  void pg_set_landmark_estimates(int n_points, const double* points, const int* hidx);
  void pg_get_landmark_estimates(double* points);
  void pg_linearize(bool jacobians);
  void pg_update();
  void pg_push();
  void pg_pop();
  void pg_discard_top();
  void solve_back_substitute();
  void multiply_hessian(double* dest_host, const double* src_host);

  size_t vector_size() const { return (size_t)nP_ * p_ + (size_t)nL_ * l_; }
  void set_x(const double* h);
  void copy_x(double* h);
  void copy_b(double* h);
  const double* x_device() const { return d_x.p; }
  const double* b_device() {
    ensure_bl();
    return d_b.p;
  }
  void sync();
  void set_stream(hipStream_t st);
  hipStream_t stream() const { return st_; }

  int nnzb(int which) const;
  void get_pattern(int which, int* colptr, int* rowidx) const;
  void copy_values(int which, double* h);
  void device_array(int which, double** ptr, size_t* count);

  // ---- device-resident bundle-adjustment front end: error / Jacobian
  // producers, oplus and the estimate stack for EdgeProjectXYZ2UV graphs, so that a whole LM trial
  // loop needs no host round trip of Jacobians or estimates
  void ba_set_edges(int set, const int* cam_vertex, const int* point_vertex, const double* meas, const double* info, double f,
                    double cx, double cy);
  void ba_set_edges_classes(int set, const int* cam_vertex, const int* point_vertex, const double* meas, const double* info, double f,
                            double cx, double cy, int n_classes, const double* class_params, const int* edge_class);
  // the same slot bound to a set of stereo observations (EdgeProjectXYZ2UVU, error (u_left, v_left, u_right)): ba_stereo.inc
  void ba_set_stereo_edges(int set, const int* cam_vertex, const int* point_vertex, const double* meas, const double* info, double f,
                           double cx, double cy, double baseline);
  // a second slot beside it: one set of EdgeSE3Expmap constraints between two cameras (ba_pose_edge.inc); info == nullptr: identity
  void ba_set_pose_edges(int set, const int* vi, const int* vj, const double* meas, const double* info);
  // the projection slot bound to THREE-vertex observations (EdgeProjectPSI2UV: point, observing pose, anchor pose) as three binary
  // sets of the same edge count: ba_psi.inc; info == nullptr: identity
  void ba_set_inverse_depth_edges(int set_point_pose, int set_point_anchor, int set_pose_anchor, const int* cam_vertex,
                                  const int* anchor_vertex, const int* point_vertex, const double* meas, const double* info, double f,
                                  double cx, double cy);
  void ba_set_estimates(int n_cams, const double* cams, const int* cam_hidx, int n_points, const double* points, const int* point_hidx);
  void ba_get_estimates(double* cams, double* points);
  void ba_get_estimates_of(int n_cams, const int* cam_idx, double* cams, int n_points, const int* point_idx, double* points);   // selected vertices
  void ba_fetch_begin(double* cams, double* points, int point_pieces);   // the same, asynchronous and in pieces (see the definition)
  void ba_fetch_wait(int piece);
  static constexpr int kFetchMaxPieces = 17;
  void ba_linearize(bool jacobians);
  void ba_update();
  void ba_structure_only(int num_iters, int num_max_trials, int* point_trace, double* point_chi2);
  void ba_push();
  void ba_pop();
  void ba_discard_top();

  bool profiling = false;
  KernelProf prof;
  SolverTimes times;
  CholOptions chol_opt;
  size_t schur_tile_bytes = 39 * 1024;     // LDS budget of one Schur tile
  int comm_emulate = 0;                    // TIMING ONLY: solve_sharded of one rank of an N-rank job run alone, the all-reduces skipped
                                           // (results are wrong; bench.py --emulate r/N: the per-rank time an N-GPU run is bounded by)
  bool rhs_prefilled_ = false;             // solve(): schur_rhs_kernel has also written the permuted right-hand side and cleared the factorisation's
                                           // status word for the next solve_reduced_device
  bool ba_fused = true;                    // evaluate BA errors/Jacobians inside the assembly kernels (no J arrays)
  // hipGraph replay of the launch-bound kernel sequences (one launch per tree level: factorisation with the
  // fused forward sweep, backward sweep): ~30 launches per iteration, which is what limits a rank once the
  // per-rank work shrinks (multi-GPU).  Needs a non-default stream.  Timing events sit between the graphs.
  bool use_graph = false;
  int sharded_merge = 1;                   // sharded solve: TWO all-reduces instead of three -- the boundary blocks and b_p travel with the
                                           // subtree roots (after the own subtrees) whenever only the shared top of the tree consumes them
  size_t sharded_collectives = 0;          // all-reduces issued by the last solve_sharded_once (stats)
  bool setup_overlap = true;               // build_structure: the symbolic analysis of the reduced system on a thread of its own next to the Schur tiles' set-up
  int sharded_selftest = 1;                // the first solve_sharded of a structure runs twice (as configured / reference schedule) and falls back to the
                                           // reference schedule when the two disagree (see solve_sharded)
  bool selftest_fallback() const { return selftest_fallback_; }
  int selftest_break = 0;                  // (tests only) rank 0 corrupts its copy of the configured variant's solution: the self-test must fall back on EVERY rank
  int sharded_graph = 1;                   // solve_sharded as ONE hipGraph (the collectives inside it): 1 = when nothing has to cross the
                                           // host (comm_emulate, the peer mailboxes: their two kernels per all-reduce), 2 = with RCCL as well (ncclAllReduce captured into the graph; not
                                           // exercised on hardware here -- opt-in); 0 = one graph per phase, plain launches in between
  void invalidate_graphs();
  int linear_solver = 0;                   // 0: multifrontal block Cholesky, 1: block-Jacobi PCG (LinearSolverPCG) on Hschur,
                                           // 2: the same PCG matrix-free (Schur complement never formed; Schur mode only)
  PcgOptions pcg_opt;
  int pcg_iterations = 0;
  int num_cus_ = 256;
  bool fuse_schur_reduce = true;           // solve(): the factorisation assembles its fronts from Hpp and the tiles' partial
                                           // blocks directly; Hschur is only written out when somebody asks for it
  bool tiles_cover_all_ = false;
  bool mask_solution = true;               // solve_reduced_shared zeroes the x_p entries other ranks own (all-reduce of x_p)
  const CholStats* chol_stats() const { return chol_ ? &chol_->stats() : nullptr; }
  int p() const { return p_; }
  int l() const { return l_; }
  int nP() const { return nP_; }
  int nL() const { return nL_; }
  bool schur() const { return schur_; }

 private:
  int p_, l_, device_;
  int nP_ = 0, nL_ = 0;
  bool schur_ = false, structured_ = false, system_built_ = false;
  hipStream_t st_ = nullptr;
  bool own_stream_ = false;
  std::vector<std::unique_ptr<EdgeSet>> sets_;
  std::vector<std::pair<int, int>> extra_hs_;  // extra structural blocks (row, col) of the reduced system
  // host patterns
  std::vector<int> pp_colptr, pp_row, pp_diag, pl_colptr, pl_row, hs_colptr, hs_row;
  // device matrices
  enum Seg { kSegFactor = 0, kSegBackward, kSegLocal, kSegShared, kSegSharedBack, kSegFactorBand, kSegFactorRest, kSegShardedAll, kSegFactorPre, kNumSeg };
  bool in_outer_seg_ = false;   // an enclosing segment is being captured / run: inner run_seg calls are transparent
  struct GraphSeg {
    hipGraph_t g = nullptr;
    hipGraphExec_t e = nullptr;
    int state = 0;   // 0: run plainly once (first-use initialisation), 1: capture, 2: replay
  };
  GraphSeg segs_[kNumSeg];
  template <class F>
  void run_seg(int id, F&& body);
  void build_system_impl();
  void solve_schur_impl(bool want_matrix = true);
  template <int P, int L>
  void launch_schur_tiles(int G, bool fuse_inv);
  void launch_schur_reduce(bool matrix);
  void launch_reduce_kernel(int n_red, bool split, double* Hs, const unsigned char* lam_mask, const int* list);
  void launch_chi2(const EdgeSet& es, int nblocks, double* red);
  void ensure_hschur();
  bool virtual_reduced_ok();
  void solve_reduced_device();
  int solve_reduced_impl();
 public:
  // Multi-GPU halo exchange without host round trips (openslam_g2o_amd/distributed.py): index lists and keep-masks
  // live on the device, pack / unpack are single kernels, the status travels inside the last buffer.
  // LM trial without intermediate host round trips: solve_async() queues the whole solve and leaves the status on the
  // device; trial_stats() (after the caller's update / error evaluation) returns that status together with chi2 and
  // computeScale(lambda) = x'(lambda x + b) behind ONE synchronisation
  // the reduced system as an operator (matrix-free PCG, here and sharded in distributed.py)
  void schur_operator_prepare();
  void schur_operator_apply(const double* din, double* dout);
  void solve_async();
  void trial_stats(double lambda, int* ok, double* chi2, double* scale);
  void trial_stats_begin(double lambda);   // the queued half of trial_stats (kernels + read-back, no synchronisation)
  void exchange_setup(int nbb, const int* bblock, const double* hkeep, int nbp, const int* bpose, const double* bkeep, int nh,
                      const int* halo, const double* hmine);
  void exchange_pack(int which);     // 1: boundary Hschur blocks + boundary bschur -> buffer 105; 3: halo x (masked) + status -> 106
  void exchange_unpack(int which);   // 1: buffer 105 (x keep) -> Hschur / bschur; 3: buffer 106 -> x
  void solve_reduced_finish_async(); // un-permute x_p, no status read
  int exchange_status();             // after exchange_unpack(3): 0 ok, 1 some rank's factorisation failed (synchronises)
  // Collectives inside the library (comm.h): the whole sharded solve and the LM scalars without a Python / torch layer.
  Comm comm;
  void comm_init_rccl(int rank, int world, const char* id128);
  void comm_init_peer(int rank, int world, HostAllReduceFn fn, void* ctx, size_t slot_doubles);
  void comm_all_reduce(double* dev, size_t n, int op);
  int solve_sharded();
  int solve_sharded_once();                       // Schur pass, three all-reduces, subtree-distributed factorisation, back-substitution
  double chi2_sharded();                     // activeRobustChi2 over all ranks
  double max_diagonal_sharded();             // computeLambdaInit's maximum over the SUMMED pose diagonal and all landmarks
  double compute_scale_sharded(double lambda);
 private:
  struct Exchange {
    int nbb = 0, nbp = 0, nh = 0;
    DevBuf<int> bblock, bpose, halo;
    DevBuf<double> hkeep, bkeep, hmine, buf1, buf3;
    bool valid = false;       // exchange_setup has been called for the current structure (build_structure resets the whole record)
    bool merged = false;      // the boundary blocks / b_p ride in the all-reduce of the subtree roots (sharded_merge)
    double* tail = nullptr;   // ... their place behind the Cholesky's exchange buffer
  } ex_;
  bool selftest_done_ = false, selftest_fallback_ = false;
  int solve_sharded_repeat();
  void solve_back_substitute_impl();
  void launch_boundary_reduce();
  void drop_graph_segments();
  bool sv_ready_ = false, sv_now_ = false;
  size_t hpp_blocks_ = 0;
  std::vector<int> sv_base_, sv_diag_, sv_ptr_, sv_slot_;
  DevBuf<int> d_sv_slot;
  void solve_reduced_local_impl();
  void solve_reduced_shared_impl();
  DevBuf<unsigned char> d_lam_mask;
  DevBuf<double> d_lam;                    // {lambda_pose, lambda_landmark}: virtual damping (Schur mode)
  double lam_pose_ = 0.0, lam_lm_ = 0.0;
  std::vector<unsigned char> lam_mask_h_;
  DevBuf<int> d_active;                    // multi-GPU: reduced-system blocks this rank forms (schur_reduce)
  int n_active_ = -1;                      // -1: all
  std::vector<int> rd_cnt_h_, rd_ptr_h_, rd_slot_h_, hs_src_h_, hs_diag_h_;
  DevBuf<int> d_pose_diag;                 // pose -> its diagonal block of the reduced system
  bool hschur_valid_ = true, virt_now_ = false;
 public:
  size_t dependency_fallbacks = 0;   // dependency-driven launches that gave up and were repeated level by level
  bool ba_fuse_landmarks = true;      // fused BA path (Hpl not written while nobody reads it, ensure_hpl): the landmark side (Hll, b_l, errors) is
                                      // assembled by the Schur tiles of the solve, which write only b_l and Dinv, what the solve reads
  bool marginals_recursion = true;  // compute_marginals: all entries on the pattern of L in one top-down pass (sparse inverse) instead of one pair of sweeps per column
  bool pg_landmark_staged = true;   // landmark linearize kernels: results leave through LDS, contiguous per wave (pg_landmark.inc)
  bool ba_stereo_staged = true;     // the stereo BA linearize kernel likewise (ba_stereo.inc)
  bool marginals_reduced = false;   // compute_marginals: invert the reduced pose system instead of Hpp alone (the reference inverts Hpp)
 private:
  hipStream_t fetch_st_ = nullptr;                         // ba_fetch_begin: the copy stream of the asynchronous estimate read-back
  hipEvent_t fetch_fork_ = nullptr, fetch_ev_[kFetchMaxPieces] = {};
  int fetch_pieces_ = 0;
  void ba_fetch_fence();
  DevBuf<double> d_red_multi;              // trial_stats: partial sums of every reduction of the call
  double* h_trial_ = nullptr;              // ... their pinned host copy (+ the factorisation status word): ONE synchronisation per trial
  size_t h_trial_n_ = 0;
  int sync_status_ = -1;                   // status of a solve_async() that had to run synchronously (-1: none)
  struct TrialPending {                    // trial_stats_begin() -> trial_stats()
    bool begun = false, bad = false, need_chi = false;
    int mode = 0;                          // 1: the status word of an asynchronous solve is part of the read-back
    size_t hn = 0;
    std::vector<int> nblk;
  } trial_;
  hipEvent_t trial_ev_ = nullptr;
  bool deferred_status_ = false;           // a solve_async() whose status has not been read yet
  bool chi2_valid_ = false;                // chi2_value_ matches the errors / kernels of every edge set
  double chi2_value_ = 0.0;
  DevBuf<double> d_Hpp, d_Hpl, d_Hll, d_Hschur, d_Dinv, d_db, d_b, d_x, d_bschur, d_bkP, d_bkL, d_red;
  DevBuf<int> d_pp_diag, d_pl_colptr, d_pl_row, d_pl_lm;
  DevBuf<int> d_hs_src;                    // Hschur block -> Hpp block id or -1
  DevBuf<int> d_hs_diag;                   // Hschur block -> pose index when diagonal, else -1
  // Schur tiles: landmark ranges, their destination blocks and LDS-local contributor entries
  DevBuf<int> d_tile_lm0, d_tile_td0, d_td_diag, d_td_ptr, d_te_pack, d_rd_ptr, d_rd_slot;
  DevBuf<int2> d_tile_q2;         // per tile: second Hpl block range (first block, count) -- tiles of a split landmark
  int n_split_tiles_ = 0;
  std::vector<int> tile_lm0_h_;   // first landmark of every tile (+ one past the last)
  DevBuf<unsigned short> d_te_lm, d_slot_lm;
  DevBuf<double> d_Pd, d_Pr;               // per (tile, destination) partial blocks / rhs
  int n_tiles_ = 0;
  long n_td_ = 0;
  size_t schur_lds_bytes_ = 0;
  // multiply_hessian pattern
  DevBuf<int> d_pp_colptr, d_pp_row;
  long n_sc_ = 0;
  std::unique_ptr<SparseCholesky> chol_;
  std::unique_ptr<BlockPCG> pcg_;
  // linear_solver 2: PCG on the reduced system WITHOUT forming it (Hschur v = Hpp v + lambda v - Hpl Dinv Hpl' v)
  std::unique_ptr<BlockPCG> pcg_mf_, pcg_hpp_;
  DevBuf<int> d_pm_ptr, d_pm_q, d_pm_lm;     // pose-major lists of the Hpl blocks (block id, landmark)
  DevBuf<int> d_mh_ptr, d_mh_q, d_mh_lm;     // ... the same for multiply_hessian (any mode)
  std::unique_ptr<BlockPCG> mh_hpp_;         // gather-form symmetric product with Hpp (multiply_hessian)
  DevBuf<double> d_mf_l, d_mf_diag, d_mf_zero;
  bool mf_ready_ = false;
  int solve_matrix_free();
  void mf_prepare_lists();
  void ba_validate_edges(const struct EdgeSet& es, const int* cam_v, const int* pt_v, size_t n, const int* cam_hidx, int nc,
                         const int* pt_hidx, int np) const;
  void ba_validate_psi_edges(const EdgeSet& a, const EdgeSet& b, const EdgeSet& c, const int* cam_v, const int* anchor_v, const int* pt_v,
                             size_t n, const int* cam_hidx, int nc, const int* pt_hidx, int np) const;
  // Three binary sets that stand for ONE three-vertex edge (g2ohip_set_edge_set_parts): ids = (a-b, a-c, b-c).  The first owns the
  // Jacobians of a and b (own_J0, own_J1), the information and the errors, the third the Jacobian of c (own_J1); every other J0 /
  // J1 / omega / err pointer of the three aliases one of those.  alias_triple points them there; a pointer that had to be repaired
  // (set_edge_data on one of the sets repoints it to that set's own copy) drops the captured launch sequences.  release_triple:
  // the sets keep no device-written data and no pointer into each other's buffers (set_edge_data is their next source;
  // build_system refuses them until then, unless they are empty).  Used by the inverse-depth group of the BA front end and by the
  // three calibration groups of the pose-graph front end; what else a group owns is released by its caller.
  void alias_triple(const int ids[3]);
  void release_triple(const int ids[3]);
  void ba_psi_release();   // (release_triple of it, and its anchors)
  bool ba_recompute_ok() const;
  bool ba_skip_hpl_ok() const;
  bool ba_fuse_ll_ok() const;
  int ba_lm_group() const;
  void ensure_hpl();
  void launch_ba_poses();
  void ensure_ll();
  void ensure_bl();
  void launch_ba_landmarks(bool write_hpl);
  bool hpl_valid_ = true;
  bool ll_valid_ = true;   // Hll, b_l and the errors of the fused BA path match the last build_system
  bool ll_hbm_partial_ = false;   // ... but the Schur tiles that assembled them wrote b_l only (Hll and the errors stayed on chip)
  void pg_validate(const EdgeSet& es, const int* vi, const int* vj, size_t n, const int* hidx, int nv) const;
  // (landmark_first: the set's vertex 0 is the landmark and its vertex 1 the pose -- the (landmark, calibration) set of type 24)
  void pg_validate_landmarks(const EdgeSet& es, const int* vp, const int* vl, size_t n, const int* hidx, int nv, const int* pt_hidx,
                             int np, bool landmark_first = false) const;
  void pg_validate_priors(const EdgeSet& es, const int* vq, size_t n, const int* hidx, int nv) const;
  // a row of the SE2 pose table is read either as a VertexSE2 or as an additive row (VertexOdomDifferentialParams), never both:
  // throws ArgFailure where one of `lists` (index arrays read as VertexSE2) names a row of `additive` (sorted)
  static void pg_refuse_additive(const std::string& who, const std::vector<int>& additive,
                                 const std::vector<std::pair<const int*, size_t>>& lists);
  void pg_bind_landmark_edges(const char* who, int set, int type, const int* pose_vertex, const int* point_vertex, const double* meas,
                              const double* info, const double* offset, const double* kcam, int n_cams = 0);
  // ---- the table of slots (PgSlotId, PgSlot below) and the helpers that loop over it, each written once ----
  enum PgSlotId : int;
  int pg_slot_of(int set) const;   // the slot that holds the set id, -1: none
  // What every bind entry starts with, in this order: invalidate_graphs, require_structure, "call pg_set_edges first"
  // (StateFailure; not for the pose slot itself), the range of the ids, and ownership -- a set may be bound again in its own slot,
  // an id another slot holds is an ArgFailure.  `who` starts every message (the landmark slot has four entries).
  void pg_begin_bind(const char* who, PgSlotId slot, std::initializer_list<int> sets);
  // What every bind entry ends with, after its LAST check: the set that leaves the slot gives up the data the device wrote for it (a
  // group: pg_release_group), the slot takes the ids, the type, the index arrays (host copy and device) and the measurements
  // [n][meas_stride]; the first set gets the information [n][d x d] and buffers for J0 [n][d x d0], J1 [n][d x d1] (d1 = 0: a
  // unary set), errors [n][d] -- a group: the third set its J1 [n][d x d2] (the third vertex; d2 < 0: as wide as d1), then
  // alias_triple; the pointers of the sets are their own (external = false), no data and no errors until the first pg_linearize,
  // the cached evaluation and chi2 are dropped; the stream is synchronised (every array handed in has been read).
  void pg_commit(PgSlotId slot, std::initializer_list<int> sets, int type, std::initializer_list<const int*> idx, size_t n,
                 const double* meas, size_t meas_stride, int d, int d0, int d1, const double* info, int d2 = -1);
  // a bound slot against candidate estimate tables (the descriptor says which validator: pose pairs, pose-landmark pairs, priors,
  // or the three pairs of a group)
  void pg_validate_slot(PgSlotId slot, const int* hidx, int nv, const int* pt_hidx, int np) const;
  // one binary set of a group, over the vertices (a, b) of its edges, against candidate tables: the descriptor's points[] flags say
  // which of the two index arrays names landmarks (pg_validate / pg_validate_landmarks, in either vertex order)
  void pg_validate_pair(const EdgeSet& es, const int* va, bool a_point, const int* vb, bool b_point, size_t n, const int* hidx, int nv,
                        const int* pt_hidx, int np) const;
  // What the entries of the three-vertex groups check alike, up to and including the index validation against the committed
  // tables.  The group's shape: error dimension d (measurements [n][meas], information [n][d x d]) and, per vertex (a, b, x), its
  // dimension; which vertices are landmarks is the slot's kPgSlotDesc[].points.  The sets are (a, b), (a, x), (b, x) with the
  // dimensions and parts that follow from that; two vertices of one edge that are rows of the same table must differ.
  struct PgGroupShape {
    int d, meas;
    int dim[3];
    const char* words;   // the dimensions in the message
  };
  void pg_check_group(const std::string& who, PgSlotId slot, const PgGroupShape& shape, const int ids[3], const int* vi, const int* vj,
                      const int* vx, const double* meas, const double* info) const;
  void pg_release_group(PgSlotId slot);   // a group leaves its slot: release_triple, the host index copies, the cached evaluation
  void pg_od_release();                   // ... the odometry group: its additive rows are VertexSE2 rows again, the captured launches go
  void pg_od_build_mask();
  // One table of vertex estimates on the device, as both front ends keep them (ba_.cams / ba_.pts, pg_.poses / pg_.points): the
  // values, their backup (an estimate stack of depth one) and every vertex's index in the system (-1: fixed).
  // Validate, then commit: every committed (edge binding, table) pair has been validated against each other when the later of
  // the two was committed.  A set_* entry hands its CANDIDATE to ba_validate_edges / pg_validate / pg_validate_landmarks before
  // it writes any member, so a rejected call leaves the previous binding and tables as they were, and nothing is rolled back.
  struct EstimateTable {
    DevBuf<double> val, bak;
    DevBuf<int> hidx;
    std::vector<int> h_hidx;   // host copy: index validation and same()
    int n = 0, stride = 0;     // vertices, doubles per vertex
    size_t scalars() const { return (size_t)n * stride; }
    bool same(int count, int str, const int* h) const {   // the committed tables with (possibly) new values?
      return count == n && str == stride && val.p && std::memcmp(h_hidx.data(), h, sizeof(int) * (size_t)n) == 0;
    }
    void set_values(const double* v, hipStream_t st) { val.upload(v, scalars(), st); }   // (after same(): no reallocation)
    void commit(int count, int str, const double* v, const int* h, hipStream_t st) {
      n = count;
      stride = str;
      h_hidx.assign(h, h + count);
      val.upload(v, scalars(), st);
      hidx.upload(h, (size_t)count, st);
      bak.alloc(scalars());
    }
    void push(hipStream_t st) { copy(bak.p, val.p, st); }
    void pop(hipStream_t st) { copy(val.p, bak.p, st); }
    void download(double* h, hipStream_t st) const { val.download(h, scalars(), st); }
    void copy(double* dst, const double* src, hipStream_t st) const {
      if (n > 0) G2OHIP_HIP_CHECK(hipMemcpyAsync(dst, src, scalars() * sizeof(double), hipMemcpyDeviceToDevice, st));
    }
  };
  struct BaFrontEnd {
    int set = -1, n_edges = 0;
    EstimateTable cams, pts;    // T[12] per camera, (x, y, z) per point
    double f = 0, cx = 0, cy = 0;
    bool stereo = false;        // the set holds EdgeProjectXYZ2UVU observations (ba_set_stereo_edges): meas [n][3], always the generic
    double baseline = 0;        // assembly (fused_ok = false, none of the fused tables below), per-edge robust kernels allowed
    int n_classes = 1;          // edge classes (ba_set_edges_classes): > 1 = the class of an observation rides in the top byte of its
    DevBuf<double> ctab;        // camera index, ctab[5 c] = (f, cx, cy, robust kernel kind, delta)
    std::vector<double> h_ctab;
    DevBuf<int> cam_v, pt_v, edge_hpl;
    std::vector<int> h_cam_v, h_pt_v;   // host copies: index validation (ba_validate_edges)
    // which estimates the assembled system was built from (back-substitution re-evaluates the Jacobians from them)
    long est_version = 0, bak_version = 0, sys_version = -1;
    int sys_kind = 0;
    double sys_delta = 0.0;
    bool omega_identity = false;   // information = identity for the whole set (info == NULL): not read per edge
    bool err_valid = false, jac_valid = false;   // errors / Jacobians of the set match the current estimates
    DevBuf<double> chi_part;                     // per workgroup of ba_linearize_kernel: partial chi2 (folded into d_red_multi)
    bool fused_ok = false;   // every Hpl block has exactly one observation: fused on-the-fly assembly allowed
    DevBuf<double> meas;
    DevBuf<double> meas_pm, omega_pm;   // pose-major copies (observation-list order of the pose side)
    DevBuf<int> pt_pm, cam_pm;
    DevBuf<double> meas_lm, omega_lm;   // landmark-major copies
    DevBuf<int> cam_q, pt_q;            // per Hpl block (block order): camera / point of its observation
    DevBuf<double> meas_q, omega_q;
    DevBuf<int> cam_lm, pt_lm, hpl_lm, row_lm;   // (row_lm: pose block row of the observation's Hpl block, -1 = fixed pose)
    // Schur tiles that assemble their landmarks (ba_schur_tile_kernel<G, true>): lane slots of every tile -- observation
    // (12 bits, relative to the tile's first one; 0xfff: none) | list length (8 bits) | landmark inside the tile at the
    // first lane of its list, position in the list elsewhere (11 bits) | bit 31: not a first lane; a landmark never
    // straddles a wavefront -- and per tile (first slot, slots, first observation, longest list)
    DevBuf<int4> ll_rec;      // per lane slot: (slot word, camera, point, Hpl block or -1)
    DevBuf<int> ll_edge;      // ... edge id (error store)
    DevBuf<int> ll_row;       // ... pose block row of the observation's Hpl block (-1: fixed pose)
    DevBuf<double> ll_meas, ll_omega;   // ... measurement, information
    DevBuf<int4> tile_ll;
    DevBuf<int> sel_idx;      // ba_get_estimates_of: the selected cameras | points
    DevBuf<double> sel_out;
    bool ll_slots_ok = false;
    bool has_backup = false;
    DevBuf<int> so_trace;     // ba_structure_only: per point (iterations, accepted, rejected, stop reason)
    DevBuf<double> so_chi;    // ... (chi2 before, chi2 after)
    // ONE binary set of EdgeSE3Expmap constraints `pose_set` between two cameras beside the projection slot (ba_set_pose_edges,
    // ba_pose_edge.inc): pvi / pvj index `cams` (vertex 0 / vertex 1), pose_meas [n][12] = the measurement as an isometry.  The
    // set owns no vertices: ba_linearize fills its own_J0 / own_J1 / own_err, nothing else knows of it.  Its Jacobians are
    // needed whenever Jacobians are asked for, on the fused path too (jac_valid speaks of the projection set alone).
    int pose_set = -1;
    DevBuf<int> pvi, pvj;
    std::vector<int> h_pvi, h_pvj;   // host copies: index validation (pg_validate)
    DevBuf<double> pose_meas;
    bool pose_jac_valid = false;
    // The projection slot bound to EdgeProjectPSI2UV (ba_set_inverse_depth_edges, ba_psi.inc): `set` is the (point, pose) set,
    // psi_pa the (point, anchor) set, psi_ca the (pose, anchor) set -- one group, bound and released together.  anchor_v indexes
    // `cams` like cam_v.  `set` owns J_point (own_J0), J_pose (own_J1), information and errors, psi_ca owns J_anchor (own_J1); every
    // other J0 / J1 / omega / err pointer of the three aliases one of those (alias_triple).  Always the generic path.
    bool psi = false;
    int psi_pa = -1, psi_ca = -1;
    DevBuf<int> anchor_v;
    std::vector<int> h_anchor_v;   // host copy: index validation (ba_validate_psi_edges)
  } ba_;
  // Pose-graph front end: ONE table of slots beside the two estimate tables `poses` and `points`.  Every slot holds one edge set
  // (or one group of three) bound by its entry; pg_linearize fills the own_* arrays of every bound set, pg_update moves both
  // estimate tables, push / pop / discard_top treat them as one level.  The sets other than the pose-pose and the landmark set own
  // no vertices: nothing but pg_linearize knows of them.  Validate, then commit: a later call of an entry replaces what its slot
  // held; n = 0 is legal where the entry says so.
  // Schur on (landmarks marginalised) is the configuration the front end is meant for.  With do_schur = 0 and landmarks in the
  // structure the solver does what it does for any such system: H and b are assembled in full (Hpp, Hpl, Hll, b_p, b_l), solve()
  // factorises Hpp ALONE and writes x_p = Hpp^-1 b_p (what BlockSolver hands its linear solver without Schur, and what
  // OracleSolver(schur=False) computes); the landmark part of x keeps the zeros of build_structure, so pg_update leaves the
  // landmarks where they are.  The front end adds nothing of its own to that path.
  enum PgSlotId : int {
    // The pose-pose set every other slot stands beside (pg_set_edges): type 1 = EdgeSE2 over (x, y, theta), 2 = EdgeSE3 over
    // isometries T[12], 10 = EdgeSim3 over VertexSim3Expmap (qx, qy, qz, qw, tx, ty, tz, s) -- no prior set and no landmark set
    // other than type 11 beside it --, 12 = the VertexCam table (tx, ty, tz, qx, qy, qz, qw), whose set holds zero edges -- no
    // prior set and no landmark set other than 13 / 14 beside it.  v[0] / v[1] index `poses`, meas [n][stride of the type].
    kPose,
    // ONE set of pose-landmark observations: type 3 = EdgeSE2PointXY (beside type 1, landmarks (x, y)), 4 = EdgeSE3PointXYZ with
    // one ParameterSE3Offset (beside type 2, landmarks (x, y, z)), 5 = EdgeSE3PointXYZDepth, 6 = EdgeSE3PointXYZDisparity with one
    // ParameterCamera (offset + Kcam; beside type 2, pg_set_landmark_camera_edges), 11 = EdgeSim3ProjectXYZ (beside type 10, one
    // (fx, fy, cx, cy) per entry of the pose table; pg_set_sim3_project_edges), 13 = EdgeProjectP2MC, 14 = EdgeProjectP2SC
    // (beside type 12, one (fx, fy, cx, cy, baseline) per entry of the pose table; pg_set_cam_project_edges), 23 = Edge_XYZ_VSC
    // over VertexSCam (beside type 2, ONE (fx, fy, cx, cy, baseline) for the set; pg_set_scam_edges, pg_scam.inc).  Vertex 0 of an
    // observation is the pose (v[0] into `poses`), vertex 1 the landmark (v[1] into `points`); points.hidx[v] is the landmark's
    // index in the whole system (num_poses + its landmark number) or -1 when it is fixed.
    kLandmark,
    // ONE unary set of pose priors, independent of the landmark slot: type 7 = EdgeSE2Prior (measurement (x, y, theta)), 8 =
    // EdgeSE2XYPrior ((x, y)) beside type 1, 9 = EdgeSE3Prior (isometry [12], one ParameterSE3Offset pr_offset) beside type 2.
    // v[0] indexes `poses`; pg_linearize fills the set's own_J0 / own_err.
    kPrior,
    // ONE second pose-pose set of Edge_V_V_GICP (type 15) beside a type-2 set: v[0] / v[1] index `poses`, meas [n][6] = (pos0,
    // pos1), gicp_cov [n][18] = (cov0, cov1) with gicp_plpl (plane-to-plane: pg_linearize rewrites the set's own_omega on every
    // evaluation) (pg_gicp.inc).
    kGicp,
    // Beside a type-12 pose set, each in a slot of its own and independent of the projection set: EdgeSBACam (type 16, error 6;
    // meas [n][7] = the INVERSE measurements, computed once at binding) and EdgeSBAScale (type 17, error 1; meas [n]).  v[0] /
    // v[1] index `poses` (pg_sbacam_edge.inc).
    kCam,
    kScale,
    // ONE second pose-pose set of sensor-offset edges: type 18 = EdgeSE2Offset beside type 1 (measurements and offsets (x, y,
    // theta)), 19 = EdgeSE3Offset beside type 2 (isometries [12]).  v[0] / v[1] index `poses`, opf / opt the rows of off_table
    // [off_params][3 | 12] (the sensor frame on vertex 0 / vertex 1) (pg_offset.inc).
    kOffset,
    // ONE set of bearing-only observations EdgeSE2PointXYBearing (type 20, error 1) beside type 1, with or without a type-3 set in
    // the landmark slot: v[0] indexes `poses`, v[1] the SAME landmark table `points`, meas [n] the measured angles
    // (pg_bearing.inc).  The estimates, the update and push / pop are those of the landmark slot.
    kBearing,
    // ONE group of EdgeSE2SensorCalib (type 21, error 3, THREE vertices: pose, pose, laser offset -- all rows of `poses`) beside
    // type 1: the three binary sets (i, j), (i, l), (j, l) of g2ohip_set_edge_set_parts are bound and released together and share
    // Jacobians, information and errors (alias_triple).  v[0] / v[1] / v[2] index `poses`, meas [n][3] = (x, y, theta)
    // (pg_calib.inc).
    kCalib,
    // ONE group of EdgeSE2OdomDifferentialCalib (type 22, error 3, THREE vertices: pose, pose, VertexOdomDifferentialParams -- all
    // rows of `poses`) beside type 1, independent of the type-21 slot: the binary sets (i, j), (i, p), (j, p) share buffers as
    // the type-21 group's do.  meas [n][3] = (vl, vr, dt) (pg_odom_calib.inc).  While the group is bound the rows named by v[2]
    // are ADDITIVE rows: od_rows lists them (sorted, unique), od_mask [poses.n] marks them on the device for
    // pg_se2_update_additive_kernel.
    kOdom,
    // ONE group of EdgeSE2PointXYCalib (type 24, error 2, THREE vertices: pose, landmark, sensor offset) beside type 1, with or
    // without a type-3 or a bearing set over the same landmark table, independent of every other slot: the first group that spans
    // BOTH tables.  v[0] (pose) and v[2] (the calibration vertex, an ordinary VertexSE2) index `poses`, v[1] indexes `points`; the
    // binary sets (pose, landmark), (pose, calib), (landmark, calib) of dimensions (3, 2), (3, 3), (2, 3) share buffers as the
    // type-21 group's do: the first owns J_pose [n][2 x 3], J_point [n][2 x 2], information and errors, the third J_calib
    // [n][2 x 3].  meas [n][2] (pg_pointxy_calib.inc).
    kPointCalib,
    kPgSlots
  };
  struct PgSlot {
    int set[3] = {-1, -1, -1};   // single-set slots use set[0]; groups use (ij, il | ip, jl | jp), type 24 (pl, pc, lc)
    int type = 0;                // the edge type bound (PgSlotId above)
    std::vector<int> h_v[3];     // host copies of the index arrays: validation against the estimate tables
    DevBuf<int> v[3];
    DevBuf<double> meas;
    bool bound() const { return set[0] >= 0; }
    bool holds(int id) const { return id >= 0 && (id == set[0] || id == set[1] || id == set[2]); }
    size_t n() const { return h_v[0].size(); }   // edges at binding
  };
  // what the loops over the table need to know of a slot
  struct PgSlotDesc {
    const char* words;    // the slot in messages
    const char* entry;    // the entry that binds it ("... has grown since <entry>: call <entry> again")
    int sets, arrays;     // sets (1, or the 3 of a group) and index arrays
    bool points[3];       // per index array: a row of `points` (else of `poses`)
    bool clears_leaving;  // a set another call replaces in the slot gives up the data the device wrote for it (the entries of the
                          // four oldest slots never did, and their replaced sets keep theirs)
  };
  static constexpr PgSlotDesc kPgSlotDesc[kPgSlots] = {
      {"the pose-pose set", "pg_set_edges", 1, 2, {false, false, false}, false},
      {"the landmark set", "pg_set_landmark_edges", 1, 2, {false, true, false}, false},
      {"the prior set", "pg_set_prior_edges", 1, 1, {false, false, false}, false},
      {"the GICP set", "pg_set_gicp_edges", 1, 2, {false, false, false}, false},
      {"the EdgeSBACam set", "pg_set_cam_edges", 1, 2, {false, false, false}, true},
      {"the EdgeSBAScale set", "pg_set_cam_edges", 1, 2, {false, false, false}, true},
      {"the sensor-offset set", "pg_set_offset_edges", 1, 2, {false, false, false}, true},
      {"the bearing set", "pg_set_bearing_edges", 1, 2, {false, true, false}, true},
      {"the EdgeSE2SensorCalib group", "pg_set_sensor_calib_edges", 3, 3, {false, false, false}, true},
      {"the EdgeSE2OdomDifferentialCalib group", "pg_set_odom_calib_edges", 3, 3, {false, false, false}, true},
      {"the EdgeSE2PointXYCalib group", "pg_set_pointxy_calib_edges", 3, 3, {false, true, false}, true},
  };
  struct PgFrontEnd {
    PgSlot slot[kPgSlots];
    int pose_type() const { return slot[kPose].type; }   // 0: no pose-pose set bound
    EstimateTable poses;           // one row per pose of the bound pose type (PgSlotId::kPose)
    EstimateTable points;          // (x, y) or (x, y, z) per landmark
    bool fix_scale = false;        // VertexSim3Expmap::_fix_scale of the whole table (pg_set_sim3_fix_scale)
    bool has_backup = false;
    bool err_valid = false, jac_valid = false;
    // the landmark slot
    double offset[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};   // ParameterSE3Offset of the set (type 4), the offset of its ParameterCamera (5, 6)
    double kcam[4] = {1, 1, 0, 0};                              // ... and that camera's fx, fy, cx, cy; type 23: VertexSCam::Kcam
    double baseline = 0.0;                                      // type 23: VertexSCam::baseline
    DevBuf<double> cam_k;          // type 11: (fx, fy, cx, cy) of every entry of `poses` (VertexSim3Expmap::_focal_length,
    int n_cams = 0;                // _principle_point), n_cams entries: == poses.n whenever both are bound; types 13 / 14: (fx,
                                   // fy, cx, cy, baseline) (SBACam::Kcam, baseline)
    double pr_offset[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};   // the prior slot: ParameterSE3Offset of a type-9 set
    DevBuf<double> gicp_cov;       // the GICP slot
    bool gicp_plpl = false;
    DevBuf<int> opf, opt;          // the sensor-offset slot
    DevBuf<double> off_table;
    int off_params = 0;
    std::vector<int> od_rows;      // the odometry-calibration slot
    DevBuf<int> od_mask;
  } pg_;
  EventTimer tq_, ts_, tn_, tl_, tb_, tfe_;
  void require_structure() const;
  double reduce_sum_finish(int nblocks);
};

}  // namespace g2ohip
