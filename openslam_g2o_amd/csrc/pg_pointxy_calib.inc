// ---- landmark self-calibration: point-landmark observations that also estimate the sensor's mounting offset (included by
// block_solver.hip behind pg_odom_calib.inc, inside namespace g2ohip; type 24 of the pose-graph front end, a THREE-vertex edge over
// BOTH estimate tables -- pose and calibration vertex rows of the pose table, the landmark a row of the landmark table -- beside a
// type-1 pose set, in a slot of its own) --
//   EdgeSE2PointXYCalib::computeError       g2o/types/slam2d/edge_se2_pointxy_calib.h:46-52
//   EdgeSE2PointXYCalib::read / write       g2o/types/slam2d/edge_se2_pointxy_calib.cpp (tag EDGE_SE2_XY_CALIB)
//   SE2::operator*, SE2::inverse            g2o/types/slam2d/se2.h; normalize_theta g2o/stuff/misc.h
//   BaseMultiEdge::linearizeOplus (numeric) g2o/core/base_multi_edge.hpp:63-116 (central difference, delta = 1e-9)
//   VertexSE2::oplusImpl                    t += u[0:2], theta = normalize_theta(theta + u[2]) (pg_se2_update_kernel)
//   VertexPointXY::oplusImpl                plain addition (pg_points_update_kernel)
// Vertex 0 of an edge is the pose x1 (row vp[k] of the pose table), vertex 1 the landmark l (row vl[k] of the landmark table),
// vertex 2 the calibration c (row vc[k] of the POSE table): an ordinary VertexSE2.  Output in the layout of g2ohip_set_edge_data:
// Jp [n][2 x 3], Jl [n][2 x 2], Jc [n][2 x 3] column-major, err [n][2]; the three binary sets that stand for the edge share these
// four arrays (pg_set_pointxy_calib_edges).  The Jacobian block of a FIXED vertex (hidx == -1; the landmark's in hidx_l) is
// written as zeros.  jac = 0 writes the errors only and leaves the Jacobians in place.  One lane per edge; lanes past the end
// evaluate the last edge and store nothing (every lane reaches the barriers of the staged form).
//
// Error, in the association of computeError and operation for operation as openslam_g2o_amd/pointxy_calib.py states it:
//   a = x1 * c    w = a.inverse()    e = R(w.th) l + w.t - z
// with pg_offset_se2_mul / pg_offset_se2_inverse / pg_offset_normalize_theta of pg_offset.inc (normalize_theta after the product
// and in the inverse, as se2.h), compiled without contraction to fused multiply-adds, so that the fp64 evaluation there and the one
// here round alike up to sin / cos.
//
// DELIBERATE DEVIATION.  The reference defines no linearizeOplus for this edge and differentiates numerically
// (base_multi_edge.hpp:63-116, delta = 1e-9).  The kernel writes the exact derivative with respect to VertexSE2::oplusImpl /
// VertexPointXY::oplusImpl, as types 7, 18, 20, 21 and 22 do.  With Q = R(-(th1 + thc)) (its angle taken as w.th), J = [0 -1; 1 0],
// d = l - t1 - R(th1) tc:
//   d e / d t1 = -Q          d e / d th1 = -J Q d - Q J R(th1) tc
//   d e / d l  =  Q
//   d e / d tc = -R(-thc)    d e / d thc = -J Q d
// so it agrees with the reference's numeric Jacobian up to that one's truncation and rounding error.
//
// Store forms of pg_landmark.inc (option pg_landmark_staged); both write the same bits.  Staged, the four arrays pass through one
// LDS buffer of kThreads x 7 doubles (rows of 2, 6 and 4 doubles padded to 3, 7 and 5: odd, so that the 64 lanes of a wavefront
// writing their rows fall on different banks).
//
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage):
//   pg_se2_pointxy_calib_linearize_kernel<true>    84 VGPRs, 0 AGPRs, 49 SGPRs, scratch 0 bytes / lane, no spills, LDS 14 336 bytes /
//                                                  block, occupancy 5 waves / SIMD
//   pg_se2_pointxy_calib_linearize_kernel<false>   82 VGPRs, 0 AGPRs, 44 SGPRs, scratch 0 bytes / lane, no spills, LDS 0,
//                                                  occupancy 5 waves / SIMD
// (the registers are the double-precision sin / cos expansions': two pairs per edge for the error, one more for the Jacobians)
template <bool STAGED>
__global__ void __launch_bounds__(kThreads) pg_se2_pointxy_calib_linearize_kernel(
    int n, const double* __restrict__ poses, const double* __restrict__ points, const int* __restrict__ hidx,
    const int* __restrict__ hidx_l, const int* __restrict__ vp, const int* __restrict__ vl, const int* __restrict__ vc,
    const double* __restrict__ meas, double* __restrict__ Jp, double* __restrict__ Jl, double* __restrict__ Jc, double* __restrict__ err,
    int jac) {
#pragma clang fp contract(off)
  __shared__ double lds[STAGED ? kThreads * 7 : 1];
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  const int kk = min(k, n - 1);   // (lanes past the end evaluate the last edge and store nothing)
  const int rp = vp[kk], rl = vl[kk], rc = vc[kk];
  double x1[3], c[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    x1[i] = poses[3 * (size_t)rp + i];
    c[i] = poses[3 * (size_t)rc + i];
  }
  const double l0 = points[2 * (size_t)rl], l1 = points[2 * (size_t)rl + 1];
  const double z0 = meas[2 * (size_t)kk], z1 = meas[2 * (size_t)kk + 1];
  double a[3], w[3];
  pg_offset_se2_mul(x1, c, a);
  pg_offset_se2_inverse(a, w);
  const double cq = cos(w[2]), sq = sin(w[2]);
  const double e[2] = {(cq * l0 - sq * l1) + w[0] - z0, (sq * l0 + cq * l1) + w[1] - z1};
  pg_store<STAGED, 2>(lds, e, err, k, n);
  if (!jac) return;   // (uniform over the grid)
  const double c1 = cos(x1[2]), s1 = sin(x1[2]), cc = cos(c[2]), sc = sin(c[2]);
  const double r10 = c1 * c[0] - s1 * c[1], r11 = s1 * c[0] + c1 * c[1];   // R(th1) tc
  const double dx = (l0 - x1[0]) - r10, dy = (l1 - x1[1]) - r11;           // d
  const double jqd0 = -(sq * dx) - cq * dy, jqd1 = cq * dx - sq * dy;      // J Q d
  const double a0 = -r11, a1 = r10;                                        // J R(th1) tc
  const double qa0 = cq * a0 - sq * a1, qa1 = sq * a0 + cq * a1;
  double jp[6] = {-cq, -sq, sq, -cq, -jqd0 - qa0, -jqd1 - qa1};   // column-major 2x3
  double jl[4] = {cq, sq, -sq, cq};                               // column-major 2x2
  double jc[6] = {-cc, sc, -sc, -cc, -jqd0, -jqd1};
  const bool fixed_p = hidx[rp] < 0, fixed_l = hidx_l[rl] < 0, fixed_c = hidx[rc] < 0;
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    if (fixed_p) jp[i] = 0;
    if (fixed_c) jc[i] = 0;
  }
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (fixed_l) jl[i] = 0;
  pg_store<STAGED, 6>(lds, jp, Jp, k, n);
  pg_store<STAGED, 4>(lds, jl, Jl, k, n);
  pg_store<STAGED, 6>(lds, jc, Jc, k, n);
}
