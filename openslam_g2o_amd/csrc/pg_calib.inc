// ---- laser self-calibration: scan-match constraints that also estimate the sensor's mounting offset (included by block_solver.hip
// behind pg_offset.inc and pg_bearing.inc, inside namespace g2ohip; type 21 of the pose-graph front end, a THREE-vertex edge over
// rows of the one pose table, beside a type-1 pose set, in a slot of its own) --
//   EdgeSE2SensorCalib::computeError        g2o/types/sclam2d/edge_se2_sensor_calib.h:45-54
//   EdgeSE2SensorCalib::setMeasurement      g2o/types/sclam2d/edge_se2_sensor_calib.h:56-59 (_inverseMeasurement = m.inverse())
//   EdgeSE2SensorCalib::read / write        g2o/types/sclam2d/edge_se2_sensor_calib.cpp (tag EDGE_SE2_CALIB)
//   SE2::operator*, SE2::inverse, toVector  g2o/types/slam2d/se2.h; normalize_theta g2o/stuff/misc.h
//   BaseMultiEdge::linearizeOplus (numeric) g2o/core/base_multi_edge.hpp:63-116 (central difference, delta = 1e-9)
//   VertexSE2::oplusImpl                    t += u[0:2], theta = normalize_theta(theta + u[2]) (pg_se2_update_kernel)
// Vertex 0 of an edge is the pose x1 (row vi[k] of the pose table), vertex 1 the pose x2 (row vj[k]), vertex 2 the laser offset L
// (row vl[k]): an ordinary VertexSE2.  Output in the layout of g2ohip_set_edge_data: Ji, Jj, Jl [n][3 x 3] column-major, err
// [n][3]; the three binary sets that stand for the edge share these four arrays (pg_set_sensor_calib_edges).  The Jacobian block
// of a FIXED vertex (hidx == -1) is written as zeros.  jac = 0 writes the errors only and leaves the Jacobians in place.  One lane
// per edge; lanes past the end evaluate the last edge and store nothing (every lane reaches the barriers of the staged form).
//
// Error, in the association of computeError and operation for operation as openslam_g2o_amd/sensor_calib.py states it:
//   invm = Z.inverse()    a = x1 * L    w = a.inverse()    b = w * x2    c = b * L    d = invm * c    e = (d.t, d.angle)
// with pg_offset_se2_mul / pg_offset_se2_inverse / pg_offset_normalize_theta of pg_offset.inc (normalize_theta after every product
// and in the inverse, as se2.h), compiled without contraction to fused multiply-adds, so that the fp64 evaluation there and the one
// here round alike up to sin / cos.  Z^-1 is computed PER EVALUATION from the measurement (four multiplications, one sin / cos
// pair), not once at binding: the kernel reads the 24 bytes of Z either way.
//
// DELIBERATE DEVIATION.  The reference defines no linearizeOplus for this edge and differentiates numerically
// (base_multi_edge.hpp:63-116, delta = 1e-9).  The kernel writes the exact derivative with respect to VertexSE2::oplusImpl, as
// types 7, 18 and 20 do.  With Q = R(-(thz + th1 + thl)) (its angle is invm.angle + w.angle), J = [0 -1; 1 0],
// tA = t1 + R(th1) tl, tB = t2 + R(th2) tl:
//   d e_t / d t1 = -Q                    d e_t / d th1 = -J Q (tB - tA) - Q J R(th1) tl      d e_th / d th1 = -1
//   d e_t / d t2 =  Q                    d e_t / d th2 =  Q J R(th2) tl                      d e_th / d th2 =  1
//   d e_t / d tl =  Q (R(th2) - R(th1))  d e_t / d thl = -J Q (tB - tA)                      d e_th / d thl =  0
// so it agrees with the reference's numeric Jacobian up to that one's truncation and rounding error.  Where th1 == th2 the block
// d e_t / d tl is exactly zero.
//
// Store forms of pg_landmark.inc (option pg_landmark_staged); both write the same bits.  Staged, the four arrays pass through one
// LDS buffer of kThreads x 9 doubles (rows of 3 and 9 doubles: odd, no bank conflicts).
//
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage):
//   pg_se2_calib_linearize_kernel<true>    118 VGPRs, 0 AGPRs, 44 SGPRs, scratch 0 bytes / lane, no spills, LDS 18 432 bytes / block,
//                                          occupancy 4 waves / SIMD
//   pg_se2_calib_linearize_kernel<false>   118 VGPRs, 0 AGPRs, 46 SGPRs, scratch 0 bytes / lane, no spills, LDS 0,
//                                          occupancy 4 waves / SIMD
// (the registers are the double-precision sin / cos expansions': six pairs per edge for the error, up to three more for the Jacobians)
template <bool STAGED>
__global__ void __launch_bounds__(kThreads) pg_se2_calib_linearize_kernel(int n, const double* __restrict__ poses, const int* __restrict__ hidx,
                                                                        const int* __restrict__ vi, const int* __restrict__ vj,
                                                                        const int* __restrict__ vl, const double* __restrict__ meas,
                                                                        double* __restrict__ Ji, double* __restrict__ Jj,
                                                                        double* __restrict__ Jl, double* __restrict__ err, int jac) {
#pragma clang fp contract(off)
  __shared__ double lds[STAGED ? kThreads * 9 : 1];
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  const int kk = min(k, n - 1);   // (lanes past the end evaluate the last edge and store nothing)
  const int ri = vi[kk], rj = vj[kk], rl = vl[kk];
  double x1[3], x2[3], L[3], z[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    x1[i] = poses[3 * (size_t)ri + i];
    x2[i] = poses[3 * (size_t)rj + i];
    L[i] = poses[3 * (size_t)rl + i];
    z[i] = meas[3 * (size_t)kk + i];
  }
  double invm[3], a[3], w[3], b[3], c[3], d[3];
  pg_offset_se2_inverse(z, invm);
  pg_offset_se2_mul(x1, L, a);
  pg_offset_se2_inverse(a, w);
  pg_offset_se2_mul(w, x2, b);
  pg_offset_se2_mul(b, L, c);
  pg_offset_se2_mul(invm, c, d);
  const double e[3] = {d[0], d[1], d[2]};
  pg_store<STAGED, 3>(lds, e, err, k, n);
  if (!jac) return;   // (uniform over the grid)
  const double thq = invm[2] + w[2];
  const double cq = cos(thq), sq = sin(thq);
  const double c1 = cos(x1[2]), s1 = sin(x1[2]), c2 = cos(x2[2]), s2 = sin(x2[2]);
  const double r10 = c1 * L[0] - s1 * L[1], r11 = s1 * L[0] + c1 * L[1];   // R(th1) tl
  const double r20 = c2 * L[0] - s2 * L[1], r21 = s2 * L[0] + c2 * L[1];   // R(th2) tl
  const double dx = (x2[0] + r20) - (x1[0] + r10), dy = (x2[1] + r21) - (x1[1] + r11);   // tB - tA
  const double jqd0 = -(sq * dx) - cq * dy, jqd1 = cq * dx - sq * dy;      // J Q (tB - tA)
  const double a0 = -r11, a1 = r10, b0 = -r21, b1 = r20;                   // J R(th1) tl, J R(th2) tl
  const double qa0 = cq * a0 - sq * a1, qa1 = sq * a0 + cq * a1;
  const double qb0 = cq * b0 - sq * b1, qb1 = sq * b0 + cq * b1;
  const double dc = c2 - c1, ds = s2 - s1;                                 // R(th2) - R(th1) = [dc -ds; ds dc]
  const double m0 = cq * dc - sq * ds, m1 = sq * dc + cq * ds;             // Q (R(th2) - R(th1)) = [m0 -m1; m1 m0]
  double ji[9] = {-cq, -sq, 0, sq, -cq, 0, -jqd0 - qa0, -jqd1 - qa1, -1};   // column-major 3x3
  double jj[9] = {cq, sq, 0, -sq, cq, 0, qb0, qb1, 1};
  double jl[9] = {m0, m1, 0, -m1, m0, 0, -jqd0, -jqd1, 0};
  const bool fixed_i = hidx[ri] < 0, fixed_j = hidx[rj] < 0, fixed_l = hidx[rl] < 0;
#pragma unroll
  for (int i = 0; i < 9; ++i) {
    if (fixed_i) ji[i] = 0;
    if (fixed_j) jj[i] = 0;
    if (fixed_l) jl[i] = 0;
  }
  pg_store<STAGED, 9>(lds, ji, Ji, k, n);
  pg_store<STAGED, 9>(lds, jj, Jj, k, n);
  pg_store<STAGED, 9>(lds, jl, Jl, k, n);
}
