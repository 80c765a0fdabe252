// Host-side C++ mirror of g2o::Solver / g2o::BlockSolver<Traits> over the libg2ohip C ABI.
//
// Same member names, argument meaning and error behaviour as the reference
//   /root/reference/g2o/core/solver.h:44-149         (init, buildStructure, buildSystem, solve,
//                                                     setLambda, restoreDiagonal, x, b, vectorSize)
//   /root/reference/g2o/core/block_solver.h:98-178   (BlockSolver<Traits>)
// but over flat index / Jacobian arrays, so it compiles without g2o or Eigen.  The adapter that
// derives from g2o::BlockSolverBase and fills these arrays from a SparseOptimizer is shown in
// INTEGRATION.md (it needs the consumer's g2o + Eigen headers).  Failure is `false` + text on
// stderr, like the reference path; no exceptions.
#pragma once
#include <cstdio>
#include <vector>

#include "g2ohip.h"

namespace g2o_hip {

template <int PoseDim, int LandmarkDim>
class HipBlockSolver {
 public:
  explicit HipBlockSolver(int device = 0) {
    if (g2ohip_create(&h_, PoseDim, LandmarkDim, device) != G2OHIP_OK) report("g2ohip_create");
  }
  ~HipBlockSolver() { g2ohip_destroy(h_); }
  HipBlockSolver(const HipBlockSolver&) = delete;
  HipBlockSolver& operator=(const HipBlockSolver&) = delete;
  bool valid() const { return h_ != nullptr; }

  // Solver::init(optimizer, online)
  bool init() { return ok(g2ohip_init(h_), "init"); }
  // graph topology: one edge set per edge type; indices are hessianIndex values (-1 fixed)
  int addEdgeSet(int errorDim, int n, const int32_t* v0, const int32_t* v1) {
    int rc = g2ohip_add_edge_set(h_, errorDim, n, v0, v1);
    if (rc < 0) report("addEdgeSet");
    return rc;
  }
  // Solver::buildStructure(zeroBlocks)
  bool buildStructure(int numPoses, int numLandmarks, bool schur) {
    bool r = ok(g2ohip_build_structure(h_, numPoses, numLandmarks, schur ? 1 : 0), "buildStructure");
    if (r) {
      x_.assign(g2ohip_vector_size(h_), 0.0);
      b_.assign(g2ohip_vector_size(h_), 0.0);
    }
    return r;
  }
  bool setEdgeData(int set, const double* J0, const double* J1, const double* omega, const double* err, bool onDevice = false) {
    return ok(g2ohip_set_edge_data(h_, set, J0, J1, omega, err, onDevice ? 1 : 0), "setEdgeData");
  }
  bool setRobustKernelHuber(int set, double delta) { return ok(g2ohip_set_robust_kernel(h_, set, G2OHIP_KERNEL_HUBER, delta), "setRobustKernel"); }
  // any kernel of robust_kernel_impl.cpp: G2OHIP_KERNEL_{HUBER, PSEUDOHUBER, CAUCHY, SATURATED, DCS}
  bool setRobustKernel(int set, int kind, double delta) { return ok(g2ohip_set_robust_kernel(h_, set, kind, delta), "setRobustKernel"); }
  // Solver::buildSystem(): afterwards b() holds -J' Omega e (block_solver.hpp:551-557)
  bool buildSystem() {
    if (!ok(g2ohip_build_system(h_), "buildSystem")) return false;
    return ok(g2ohip_copy_b(h_, b_.data()), "b");
  }
  // Solver::solve(): false iff not positive definite; x() valid afterwards, b() untouched
  bool solve() {
    int rc = g2ohip_solve(h_);
    if (rc == G2OHIP_NOT_PD) return false;
    if (!ok(rc, "solve")) return false;
    return ok(g2ohip_copy_x(h_, x_.data()), "x");
  }
  bool setLambda(double lambda, bool backup = false) { return ok(g2ohip_set_lambda(h_, lambda, backup ? 1 : 0), "setLambda"); }
  void restoreDiagonal() { (void)ok(g2ohip_restore_diagonal(h_), "restoreDiagonal"); }
  double chi2() {
    double c = 0;
    (void)ok(g2ohip_chi2(h_, &c), "chi2");
    return c;
  }
  double maxDiagonal() {
    double m = 0;
    (void)ok(g2ohip_max_diagonal(h_, &m), "maxDiagonal");
    return m;
  }
  // BlockSolverBase::multiplyHessian(dest, src)
  void multiplyHessian(double* dest, const double* src) { (void)ok(g2ohip_multiply_hessian(h_, dest, src), "multiplyHessian"); }
  // Solver::computeMarginals (block_solver.hpp:489-498): out[i] = column-major PoseDim x PoseDim block (rows[i], cols[i])
  bool computeMarginals(int n, const int32_t* rows, const int32_t* cols, double* out) {
    return g2ohip_compute_marginals(h_, n, rows, cols, out) == G2OHIP_OK;
  }
  // LinearSolverPCG instead of the direct solver (linear_solver_pcg.h:53-85)
  bool usePCG(bool on, double tolerance = 1e-6) {
    return ok(g2ohip_set_option(h_, "linear_solver", on ? 1.0 : 0.0), "set_option") &&
           ok(g2ohip_set_option(h_, "pcg_tolerance", tolerance), "set_option");
  }
  // EdgeProjectXYZ2UVU observations (stereo bundle adjustment) in the slot of the device-resident BA front end
  // (g2ohip_ba_set_stereo_edges; the estimates and the trial loop through handle()): `set` was added with errorDim 3, vertex 0 =
  // point, vertex 1 = pose; meas [n][3] = (u_left, v_left, u_right), info [n][3x3] or nullptr (identity)
  bool baSetStereoEdges(int set, const int32_t* camVertex, const int32_t* pointVertex, const double* meas, const double* info,
                        double focalLength, double cx, double cy, double baseline) {
    return ok(g2ohip_ba_set_stereo_edges(h_, set, camVertex, pointVertex, meas, info, focalLength, cx, cy, baseline), "baSetStereoEdges");
  }
  // StructureOnlySolver<3>::calc(points, numIters, numMaxTrials) on the bound projection set, every free point in one kernel launch
  // (g2ohip_ba_structure_only): pointTrace nullptr or [nPoints][4] = (outer iterations, accepted, rejected, stop reason), pointChi2
  // nullptr or [nPoints][2] = (chi2 before, after), indexed like the points of g2ohip_ba_set_estimates
  bool baStructureOnly(int numIters = 10, int numMaxTrials = 10, int32_t* pointTrace = nullptr, double* pointChi2 = nullptr) {
    return ok(g2ohip_ba_structure_only(h_, numIters, numMaxTrials, pointTrace, pointChi2), "baStructureOnly");
  }
  // EdgeSE3Expmap constraints between two cameras in the second slot of the device-resident BA front end (g2ohip_ba_set_pose_edges,
  // after baSetStereoEdges / g2ohip_ba_set_edges): `set` was added as a binary set with errorDim 6 over two 6-dof poses; vi / vj index
  // the camera table (vertex 0 / vertex 1), meas [n][12] = the measurement as an isometry, info [n][6x6] or nullptr (identity)
  bool baSetPoseEdges(int set, const int32_t* vi, const int32_t* vj, const double* meas, const double* info) {
    return ok(g2ohip_ba_set_pose_edges(h_, set, vi, vj, meas, info), "baSetPoseEdges");
  }
  // EdgeProjectPSI2UV observations (point psi, observing pose, anchor pose) in the projection slot (g2ohip_ba_set_inverse_depth_edges):
  // the three binary sets of the edge's vertex pairs -- (point, pose), (point, anchor), (pose, anchor), errorDim 2, parts as the
  // header lists them -- bound as one group; camVertex / anchorVertex index the camera table; info == nullptr: identity.  A robust
  // kernel goes on all three sets.
  bool baSetInverseDepthEdges(int setPointPose, int setPointAnchor, int setPoseAnchor, const int32_t* camVertex, const int32_t* anchorVertex,
                              const int32_t* pointVertex, const double* meas, const double* info, double focalLength, double cx, double cy) {
    return ok(g2ohip_ba_set_inverse_depth_edges(h_, setPointPose, setPointAnchor, setPoseAnchor, camVertex, anchorVertex, pointVertex, meas,
                                                info, focalLength, cx, cy),
              "baSetInverseDepthEdges");
  }
  // EdgeSE3PointXYZDepth (type 5) / EdgeSE3PointXYZDisparity (type 6) observations with one ParameterCamera, kept on the device
  // beside an EdgeSE3 pose set of g2ohip_pg_set_edges (handle()): offset isometry [12] or nullptr, kcam = fx, fy, cx, cy
  bool pgSetLandmarkCameraEdges(int set, int type, const int32_t* poseVertex, const int32_t* pointVertex, const double* meas,
                                const double* info, const double* offset, const double* kcam) {
    return ok(g2ohip_pg_set_landmark_camera_edges(h_, set, type, poseVertex, pointVertex, meas, info, offset, kcam), "pgSetLandmarkCameraEdges");
  }
  // Edge_XYZ_VSC stereo observations (type 23) of VertexSBAPointXYZ points from VertexSCam cameras, kept on the device beside an
  // EdgeSE3 pose set (type 2, possibly with zero edges) of g2ohip_pg_set_edges (handle()): vertex 0 of the set is the camera,
  // vertex 1 the point; meas [n][3] = u_left, v_left, u_right; kcam = fx, fy, cx, cy, baseline, one for the whole set
  bool pgSetScamEdges(int set, const int32_t* poseVertex, const int32_t* pointVertex, const double* meas, const double* info,
                      const double* kcam) {
    return ok(g2ohip_pg_set_scam_edges(h_, set, poseVertex, pointVertex, meas, info, kcam), "pgSetScamEdges");
  }
  // EdgeSim3ProjectXYZ observations (type 11) beside an EdgeSim3 pose set (type 10) of g2ohip_pg_set_edges (handle()): vertex 0 of
  // the set is the pose, vertex 1 the point; intrinsics [nCams][4] = fx, fy, cx, cy per entry of the pose table
  bool pgSetSim3ProjectEdges(int set, const int32_t* poseVertex, const int32_t* pointVertex, const double* meas, const double* info,
                             int nCams, const double* intrinsics) {
    return ok(g2ohip_pg_set_sim3_project_edges(h_, set, poseVertex, pointVertex, meas, info, nCams, intrinsics), "pgSetSim3ProjectEdges");
  }
  // SBA-format observations beside a VertexCam set (type 12, zero edges) of g2ohip_pg_set_edges (handle()): type 13 =
  // EdgeProjectP2MC, 14 = EdgeProjectP2SC; vertex 0 of the set is the camera, vertex 1 the point; intrinsics [nCams][5] = fx, fy,
  // cx, cy, baseline per entry of the pose table
  bool pgSetCamProjectEdges(int set, int type, const int32_t* poseVertex, const int32_t* pointVertex, const double* meas,
                            const double* info, int nCams, const double* intrinsics) {
    return ok(g2ohip_pg_set_cam_project_edges(h_, set, type, poseVertex, pointVertex, meas, info, nCams, intrinsics), "pgSetCamProjectEdges");
  }
  // unary pose priors (g2ohip_pg_set_prior_edges): type 7 = EdgeSE2Prior, 8 = EdgeSE2XYPrior beside an EdgeSE2 pose set, 9 =
  // EdgeSE3Prior beside an EdgeSE3 one; `set` is a unary set (addEdgeSet with v1 == nullptr), offset isometry [12] or nullptr (type 9)
  bool pgSetPriorEdges(int set, int type, const int32_t* poseVertex, const double* meas, const double* info, const double* offset) {
    return ok(g2ohip_pg_set_prior_edges(h_, set, type, poseVertex, meas, info, offset), "pgSetPriorEdges");
  }
  // EdgeSim3 over VertexSim3Expmap (g2ohip_pg_set_edges type 10): estimates / measurements (qx, qy, qz, qw, tx, ty, tz, s),
  // information [n][49], on a solver of pose dimension 7; fixScale = VertexSim3Expmap::_fix_scale of every vertex
  bool pgSetEdges(int set, int type, const int32_t* vi, const int32_t* vj, const double* meas, const double* info) {
    return ok(g2ohip_pg_set_edges(h_, set, type, vi, vj, meas, info), "pgSetEdges");
  }
  bool pgSetSim3FixScale(bool fixScale) { return ok(g2ohip_pg_set_sim3_fix_scale(h_, fixScale ? 1 : 0), "pgSetSim3FixScale"); }
  // GICP correspondences (g2ohip_pg_set_gicp_edges): type 15 = Edge_V_V_GICP, a second pose-pose set (error_dim 3) beside an
  // EdgeSE3 one; meas [n][6] = (pos0, pos1), info [n][3x3]; cov nullptr = point-to-plane, [n][18] = (cov0, cov1) = plane-to-plane
  bool pgSetGicpEdges(int set, const int32_t* vi, const int32_t* vj, const double* meas, const double* info, const double* cov) {
    return ok(g2ohip_pg_set_gicp_edges(h_, set, vi, vj, meas, info, cov), "pgSetGicpEdges");
  }
  // SBA pose-pose constraints (g2ohip_pg_set_cam_edges) beside a VertexCam set: type 16 = EdgeSBACam (error_dim 6, meas [n][7] =
  // (t, qx, qy, qz, qw), info [n][6x6]), 17 = EdgeSBAScale (error_dim 1, meas [n], info [n]); one slot per type
  bool pgSetCamEdges(int set, int type, const int32_t* vi, const int32_t* vj, const double* meas, const double* info) {
    return ok(g2ohip_pg_set_cam_edges(h_, set, type, vi, vj, meas, info), "pgSetCamEdges");
  }
  // Sensor-offset pose-pose edges (g2ohip_pg_set_offset_edges), a second pose-pose set in a slot of its own: type 18 =
  // EdgeSE2Offset beside an EdgeSE2 set (meas [n][3], info [n][3x3], offsets [nParams][3]), 19 = EdgeSE3Offset beside an EdgeSE3
  // set (meas [n][12], info [n][6x6], offsets [nParams][12]); paramFrom / paramTo name the rows of the offsets table
  bool pgSetOffsetEdges(int set, int type, const int32_t* vi, const int32_t* vj, const int32_t* paramFrom, const int32_t* paramTo,
                        const double* meas, const double* info, int nParams, const double* offsets) {
    return ok(g2ohip_pg_set_offset_edges(h_, set, type, vi, vj, paramFrom, paramTo, meas, info, nParams, offsets), "pgSetOffsetEdges");
  }
  // Bearing-only observations of 2-D point landmarks (g2ohip_pg_set_bearing_edges): EdgeSE2PointXYBearing beside an EdgeSE2 set, in
  // a slot of its own with or without an EdgeSE2PointXY set; poseVertex / pointVertex index the pose and landmark tables, meas [n]
  // the measured angles, info [n]
  bool pgSetBearingEdges(int set, const int32_t* poseVertex, const int32_t* pointVertex, const double* meas, const double* info) {
    return ok(g2ohip_pg_set_bearing_edges(h_, set, poseVertex, pointVertex, meas, info), "pgSetBearingEdges");
  }
  // Laser self-calibration (g2ohip_pg_set_sensor_calib_edges): three-vertex EdgeSE2SensorCalib edges beside an EdgeSE2 set, as the
  // three binary sets (i, j), (i, l), (j, l) with their parts; vi / vj / vl index the pose table (vl = the laser offset), meas
  // [n][3], info [n][3x3] or null (identity)
  bool pgSetSensorCalibEdges(int setIJ, int setIL, int setJL, const int32_t* vi, const int32_t* vj, const int32_t* vl, const double* meas,
                             const double* info) {
    return ok(g2ohip_pg_set_sensor_calib_edges(h_, setIJ, setIL, setJL, vi, vj, vl, meas, info), "pgSetSensorCalibEdges");
  }
  // Landmark self-calibration (g2ohip_pg_set_pointxy_calib_edges): three-vertex EdgeSE2PointXYCalib edges beside an EdgeSE2 set, as
  // the binary sets (pose, landmark), (pose, calib), (landmark, calib) of setEdgeSetParts; poseVertex / calibVertex index the pose
  // table, pointVertex the landmark table; meas [n][2], info [n][2x2] or null (identity)
  bool pgSetPointXYCalibEdges(int setPL, int setPC, int setLC, const int32_t* poseVertex, const int32_t* pointVertex,
                              const int32_t* calibVertex, const double* meas, const double* info) {
    return ok(g2ohip_pg_set_pointxy_calib_edges(h_, setPL, setPC, setLC, poseVertex, pointVertex, calibVertex, meas, info), "pgSetPointXYCalibEdges");
  }
  // Odometry self-calibration (g2ohip_pg_set_odom_calib_edges): three-vertex EdgeSE2OdomDifferentialCalib edges beside an EdgeSE2
  // set, as the three binary sets (i, j), (i, p), (j, p) with their parts; vi / vj / vp index the pose table (vp = the
  // VertexOdomDifferentialParams row, additive while bound), meas [n][3] = (vl, vr, dt), info [n][3x3] or null (identity)
  bool pgSetOdomCalibEdges(int setIJ, int setIP, int setJP, const int32_t* vi, const int32_t* vj, const int32_t* vp, const double* meas,
                           const double* info) {
    return ok(g2ohip_pg_set_odom_calib_edges(h_, setIJ, setIP, setJP, vi, vj, vp, meas, info), "pgSetOdomCalibEdges");
  }
  double* x() { return x_.data(); }
  const double* b() const { return b_.data(); }
  size_t vectorSize() const { return x_.size(); }
  bool supportsSchur() const { return true; }
  g2ohip_solver* handle() { return h_; }

 private:
  bool ok(int rc, const char* what) {
    if (rc >= 0) return true;
    report(what);
    return false;
  }
  void report(const char* what) { std::fprintf(stderr, "g2o_hip::HipBlockSolver::%s: %s\n", what, g2ohip_last_error()); }
  g2ohip_solver* h_ = nullptr;
  std::vector<double> x_, b_;
};

typedef HipBlockSolver<6, 3> HipBlockSolver_6_3;  // block_solver.h:180-186
typedef HipBlockSolver<3, 2> HipBlockSolver_3_2;
typedef HipBlockSolver<7, 3> HipBlockSolver_7_3;

}  // namespace g2o_hip
