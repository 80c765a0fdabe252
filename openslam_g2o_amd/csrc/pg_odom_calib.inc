// ---- odometry self-calibration: wheel-velocity constraints that also estimate the differential drive's parameters (included by
// block_solver.hip behind pg_calib.inc, inside namespace g2ohip; type 22 of the pose-graph front end, a THREE-vertex edge over rows
// of the one pose table, beside a type-1 pose set, in the odometry-calibration slot) --
//   EdgeSE2OdomDifferentialCalib::computeError   g2o/types/sclam2d/edge_se2_odom_differential_calib.h:45-63
//   OdomConvert::convertToMotion                 g2o/types/sclam2d/odometry_measurement.cpp:95-117
//   EdgeSE2OdomDifferentialCalib::read / write   g2o/types/sclam2d/edge_se2_odom_differential_calib.cpp:39-61
//   VertexOdomDifferentialParams::oplusImpl      g2o/types/sclam2d/vertex_odom_differential_params.h:43-46 (estimate += v, NO wrap)
//   SE2::operator*, SE2::inverse, toVector       g2o/types/slam2d/se2.h; normalize_theta g2o/stuff/misc.h
//   BaseMultiEdge::linearizeOplus (numeric)      g2o/core/base_multi_edge.hpp:63-116 (central difference, delta = 1e-9)
// Vertex 0 of an edge is the pose x1 (row vi[k] of the pose table), vertex 1 the pose x2 (row vj[k]), vertex 2 the parameter vertex
// p = (k_l, k_r, b) (row vp[k]): NOT an SE2, its row is an additive row of the table (pg_se2_update_additive_kernel).  The
// measurement is (vl, vr, dt).  Output in the layout of g2ohip_set_edge_data: Ji, Jj, Jp [n][3 x 3] column-major, err [n][3]; the
// three binary sets that stand for the edge share these four arrays (pg_set_odom_calib_edges).  The Jacobian block of a FIXED
// vertex (hidx < 0) is written as zeros.  jac = 0 writes the errors only and leaves the Jacobians in place.  One lane per edge;
// lanes past the end evaluate the last edge and store nothing (every lane reaches the barriers of the staged form).
//
// Error, operation for operation as openslam_g2o_amd/odom_calib.py states it:
//   vl' = vl * p[0]   vr' = vr * p[1]   D = vr' - vl'   S = vl' + vr'   b = p[2]
//   |D| > 1e-7:  Rc = (b * 0.5) * (S / D)   w = D / b   th = w * dt   x = sin(th) * Rc   y = -(cos(th) * Rc) + Rc
//                (what rot(th) * (-0, -Rc) + (0, Rc) evaluates to: the products with zero vanish)
//   otherwise:   x = (0.5 * S) * dt   y = 0   th = 0
//   K = (x, y, th)   ki = K.inverse()   w1 = x1.inverse()   t = ki * w1   d = t * x2   e = (d.t, d.angle)
// with pg_offset_se2_mul / pg_offset_se2_inverse / pg_offset_normalize_theta of pg_offset.inc, compiled without contraction to
// fused multiply-adds, so that the fp64 evaluation there and the one here round alike up to sin / cos.  The branch is taken by
// selects: sin / cos run once per lane on th (0 on the straight branch, where they return 0 and 1 exactly), so a wave whose edges
// are of both kinds does not run the expansions twice.  b = 0 yields non-finite values, as in the reference; it is not guarded.
//
// DELIBERATE DEVIATION.  The reference defines no linearizeOplus for this edge and differentiates numerically
// (base_multi_edge.hpp:63-116, delta = 1e-9).  The kernel writes the exact derivative OF THE BRANCH TAKEN, with respect to
// VertexSE2::oplusImpl for the poses and plain addition for p, as types 7, 18, 20 and 21 do.  With Q = R(-(th + th1)) (its angle is
// ki.angle + w1.angle), J = [0 -1; 1 0], e_t the translational error:
//   d e_t / d t1 = -Q     d e_t / d th1 = -J Q (t2 - t1)     d e_th / d th1 = -1
//   d e_t / d t2 =  Q     d e_t / d th2 = 0                  d e_th / d th2 =  1
//   d e_t / d q  = -R(-th) (dx/dq, dy/dq) - J e_t dth/dq     d e_th / d q   = -dth/dq          for q of (k_l, k_r, b)
//   turning:   dRc/dk_l = b vl vr' / D^2     dRc/dk_r = -b vr vl' / D^2     dRc/db = Rc / b
//              dth/dk_l = -vl dt / b         dth/dk_r = vr dt / b           dth/db = -th / b
//              dx/dq = sin th dRc/dq + Rc cos th dth/dq      dy/dq = (1 - cos th) dRc/dq + Rc sin th dth/dq
//   straight:  dx/dk_l = 0.5 vl dt    dx/dk_r = 0.5 vr dt    every other entry 0 (the column of b is zero: the branch as written
//              does not read b, and the reference's central difference gives the same while both probes stay inside the branch)
// so it agrees with the reference's numeric Jacobian up to that one's truncation and rounding error, away from |D| = 1e-7.
//
// Store forms of pg_landmark.inc (option pg_landmark_staged); both write the same bits.  Staged, the four arrays pass through one
// LDS buffer of kThreads x 9 doubles (rows of 3 and 9 doubles: odd, no bank conflicts).
//
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage):
//   pg_se2_odom_calib_linearize_kernel<true>    112 VGPRs, 0 AGPRs, 45 SGPRs, scratch 0 bytes / lane, no spills, LDS 18 432 bytes /
//                                               block, occupancy 4 waves / SIMD
//   pg_se2_odom_calib_linearize_kernel<false>   112 VGPRs, 0 AGPRs, 42 SGPRs, scratch 0 bytes / lane, no spills, LDS 0,
//                                               occupancy 4 waves / SIMD
// (the registers are the double-precision sin / cos expansions': six pairs per edge for the error, one more for the Jacobians)
//   pg_se2_update_additive_kernel (block_solver.hip)   18 VGPRs, 18 SGPRs, scratch 0, LDS 0, occupancy 8 waves / SIMD
template <bool STAGED>
__global__ void __launch_bounds__(kThreads) pg_se2_odom_calib_linearize_kernel(int n, const double* __restrict__ poses, const int* __restrict__ hidx,
                                                                             const int* __restrict__ vi, const int* __restrict__ vj,
                                                                             const int* __restrict__ vp, const double* __restrict__ meas,
                                                                             double* __restrict__ Ji, double* __restrict__ Jj,
                                                                             double* __restrict__ Jp, double* __restrict__ err, int jac) {
#pragma clang fp contract(off)
  __shared__ double lds[STAGED ? kThreads * 9 : 1];
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  const int kk = min(k, n - 1);   // (lanes past the end evaluate the last edge and store nothing)
  const int ri = vi[kk], rj = vj[kk], rp = vp[kk];
  double x1[3], x2[3], p[3], m[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    x1[i] = poses[3 * (size_t)ri + i];
    x2[i] = poses[3 * (size_t)rj + i];
    p[i] = poses[3 * (size_t)rp + i];
    m[i] = meas[3 * (size_t)kk + i];
  }
  const double vl = m[0], vr = m[1], dt = m[2], b = p[2];
  const double vlc = vl * p[0], vrc = vr * p[1];
  const double D = vrc - vlc, S = vlc + vrc;
  const bool turning = fabs(D) > 1e-7;
  const double Rc = turning ? (b * 0.5) * (S / D) : 0.0;
  const double th = turning ? (D / b) * dt : 0.0;
  const double ct = cos(th), st = sin(th);   // (1 and 0 exactly on the straight branch)
  double K[3];
  K[0] = turning ? st * Rc : (0.5 * S) * dt;
  K[1] = turning ? -(ct * Rc) + Rc : 0.0;
  K[2] = th;
  double ki[3], w1[3], t[3], d[3];
  pg_offset_se2_inverse(K, ki);
  pg_offset_se2_inverse(x1, w1);
  pg_offset_se2_mul(ki, w1, t);
  pg_offset_se2_mul(t, x2, d);
  const double e[3] = {d[0], d[1], d[2]};
  pg_store<STAGED, 3>(lds, e, err, k, n);
  if (!jac) return;   // (uniform over the grid)
  const double thq = ki[2] + w1[2];
  const double cq = cos(thq), sq = sin(thq);
  const double dx = x2[0] - x1[0], dy = x2[1] - x1[1];                     // t2 - t1
  const double jqd0 = -(sq * dx) - cq * dy, jqd1 = cq * dx - sq * dy;      // J Q (t2 - t1)
  double ji[9] = {-cq, -sq, 0, sq, -cq, 0, -jqd0, -jqd1, -1};              // column-major 3x3
  double jj[9] = {cq, sq, 0, -sq, cq, 0, 0, 0, 1};
  // per parameter q: (dRc/dq, dth/dq) on the turning branch, dx/dq on the straight one
  const double D2 = D * D, hdt = 0.5 * dt;
  const double dR[3] = {b * vl * vrc / D2, -(b * vr * vlc) / D2, Rc / b};
  const double dT[3] = {-(vl * dt) / b, vr * dt / b, -th / b};
  const double dS[3] = {vl * hdt, vr * hdt, 0.0};
  double jp[9];
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    const double dth = turning ? dT[q] : 0.0;
    const double dxq = turning ? st * dR[q] + Rc * ct * dth : dS[q];
    const double dyq = turning ? (1.0 - ct) * dR[q] + Rc * st * dth : 0.0;
    jp[3 * q + 0] = -(ct * dxq + st * dyq) + e[1] * dth;
    jp[3 * q + 1] = -(ct * dyq - st * dxq) - e[0] * dth;
    jp[3 * q + 2] = -dth;
  }
  const bool fixed_i = hidx[ri] < 0, fixed_j = hidx[rj] < 0, fixed_p = hidx[rp] < 0;
#pragma unroll
  for (int i = 0; i < 9; ++i) {
    if (fixed_i) ji[i] = 0;
    if (fixed_j) jj[i] = 0;
    if (fixed_p) jp[i] = 0;
  }
  pg_store<STAGED, 9>(lds, ji, Ji, k, n);
  pg_store<STAGED, 9>(lds, jj, Jj, k, n);
  pg_store<STAGED, 9>(lds, jp, Jp, k, n);
}
