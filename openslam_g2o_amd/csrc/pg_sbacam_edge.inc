// ---- EdgeSBACam / EdgeSBAScale: pose-pose constraints between SBA cameras (included by block_solver.hip behind
// pg_cam_project.inc, inside namespace g2ohip; types 16 / 17 of the pose-graph front end, each a set of its own beside a type-12
// pose set) ------------------------------------------------------------------------------------------------------------------
//   SE3Quat(Vector7d) / operator* / inverse / normalizeRotation   g2o/types/slam3d/se3quat.h:86-93, 104-110, 123-128, 280-285
//   SBACam::update                                                g2o/types/sba/sbacam.h:101-114 (t += x[0:3], q <- normalised q * qr)
//   EdgeSBACam::computeError / setMeasurement                     g2o/types/sba/types_sba.h:294-310 (e = (t, q.xyz) of Zinv (Ci^-1 Cj))
//   EdgeSBAScale::computeError                                    g2o/types/sba/types_sba.h:347-353 (e = z - |tj - ti|)
//   BaseBinaryEdge::linearizeOplus, numeric branch                g2o/core/base_binary_edge.hpp:132-201 (central, delta = 1e-9)
// A camera, a measurement and an inverse measurement are 7 doubles (tx, ty, tz, qx, qy, qz, qw).  The reference defines NO
// Jacobian for either edge: g2o differentiates the error numerically with a step of 1e-9 through VertexCam::oplusImpl, and
// 1 / (2 delta) = 5e8 carries every rounding of the error into the Jacobian -- so, as in pg_sim3.inc and for its reason, the
// chain is restated operation for operation (the pieces of Eigen included: quaternion product, quaternion * vector, coeffs /
// norm with the squared norm summed x, y, z, w) and compiled without contraction to fused multiply-adds.
// openslam_g2o_amd/sbacam.py states the same operations in fp64 and, in the tests, at 60 digits.
// The update of pg_cam_update_kernel has the reference's operation order but lives inside that kernel; pg_sbacam_oplus below is
// the same sequence as a function, and the existing kernel is left alone.

// SE3Quat::normalizeRotation: the sign flip when w < 0, then coeffs / norm
__device__ __forceinline__ void pg_sbacam_normalize_rotation(double* q) {
#pragma clang fp contract(off)
  if (q[3] < 0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) q[i] = q[i] * -1;
  }
  const double norm = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
#pragma unroll
  for (int i = 0; i < 4; ++i) q[i] = q[i] / norm;
}
// SE3Quat::operator*: t = a.t + a.q * b.t, q = a.q b.q, normalizeRotation
__device__ __forceinline__ void pg_sbacam_mul(const double* a, const double* b, double* r) {
#pragma clang fp contract(off)
  double rt[3];
  pg_sim3_qrot(a + 3, b, rt);
#pragma unroll
  for (int i = 0; i < 3; ++i) r[i] = a[i] + rt[i];
  pg_sim3_qmul(a + 3, b + 3, r + 3);
  pg_sbacam_normalize_rotation(r + 3);
}
// SE3Quat::inverse: q = conjugate, t = q * (t * -1); nothing is normalised
__device__ __forceinline__ void pg_sbacam_inverse(const double* a, double* r) {
#pragma clang fp contract(off)
  r[3] = -a[3]; r[4] = -a[4]; r[5] = -a[5]; r[6] = a[6];
  const double mt[3] = {a[0] * -1., a[1] * -1., a[2] * -1.};
  pg_sim3_qrot(r + 3, mt, r);
}
// SBACam::update: t += u[0:3]; qr = (u[3:6], sqrt(1 - |u[3:6]|^2)); q <- q qr, then coeffs / norm (no sign flip)
__device__ __forceinline__ void pg_sbacam_oplus(const double* c, const double* u, double* r) {
#pragma clang fp contract(off)
  const double qr[4] = {u[3], u[4], u[5], sqrt(1.0 - (u[3] * u[3] + u[4] * u[4] + u[5] * u[5]))};
  double p[4];
  pg_sim3_qmul(c + 3, qr, p);
  const double norm = sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2] + p[3] * p[3]);
#pragma unroll
  for (int i = 0; i < 3; ++i) r[i] = c[i] + u[i];
#pragma unroll
  for (int i = 0; i < 4; ++i) r[3 + i] = p[i] / norm;
}
// EdgeSBACam::computeError: delta = Zinv * (Ci^-1 * Cj), e = (delta.t, delta.q.xyz)
__device__ __forceinline__ void pg_sbacam_error(const double* Ci, const double* Cj, const double* Zi, double* e) {
  double A[7], B[7], D[7];
  pg_sbacam_inverse(Ci, A);
  pg_sbacam_mul(A, Cj, B);
  pg_sbacam_mul(Zi, B, D);
#pragma unroll
  for (int i = 0; i < 6; ++i) e[i] = D[i];
}
__device__ __forceinline__ void pg_sbacam_load(const double* __restrict__ p, double* C) {
#pragma unroll
  for (int i = 0; i < 7; ++i) C[i] = p[i];
}

// EdgeSBACam::setMeasurement on SE3Quat(Vector7d): normalizeRotation, then the inverse, once per binding; one lane per edge,
// in place (meas [n][7] becomes the inverse measurements)
__global__ void __launch_bounds__(kThreads) pg_sbacam_invert_meas_kernel(int n, double* __restrict__ meas) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  double Z[7], Zi[7];
  pg_sbacam_load(meas + 7 * (size_t)k, Z);
  pg_sbacam_normalize_rotation(Z + 3);
  pg_sbacam_inverse(Z, Zi);
#pragma unroll
  for (int i = 0; i < 7; ++i) meas[7 * (size_t)k + i] = Zi[i];
}

// err [n][6]: one lane per edge
__global__ void __launch_bounds__(kThreads) pg_sbacam_error_kernel(int n, const double* __restrict__ est, const int* __restrict__ vi,
                                                                 const int* __restrict__ vj, const double* __restrict__ zinv,
                                                                 double* __restrict__ err) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  double Ci[7], Cj[7], Zi[7], e[6];
  pg_sbacam_load(est + 7 * (size_t)vi[k], Ci);
  pg_sbacam_load(est + 7 * (size_t)vj[k], Cj);
  pg_sbacam_load(zinv + 7 * (size_t)k, Zi);
  pg_sbacam_error(Ci, Cj, Zi, e);
#pragma unroll
  for (int i = 0; i < 6; ++i) err[6 * (size_t)k + i] = e[i];
}

// J0, J1 [n][6x6] column-major: one lane per (edge, side, column), 12 lanes per edge, as pg_sim3_jacobian_kernel has 14 -- a
// lane's state is one column, and the 12 lanes of an edge store 2 x 36 contiguous doubles, so the stores are dense without an
// LDS stage.  Column c of side v: (e(C_v (+) +delta u_c) - e(C_v (+) -delta u_c)) / (2 delta), (+) = SBACam::update.  The block
// of a fixed vertex (hidx < 0) is written as zeros; the reference leaves it unset and the assembly does not read it.  The two
// signs run through ONE loop body (not unrolled).
__global__ void __launch_bounds__(kThreads) pg_sbacam_jacobian_kernel(int n, const double* __restrict__ est, const int* __restrict__ hidx,
                                                                    const int* __restrict__ vi, const int* __restrict__ vj,
                                                                    const double* __restrict__ zinv, double* __restrict__ J0,
                                                                    double* __restrict__ J1) {
#pragma clang fp contract(off)
  const size_t g = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (g >= 12 * (size_t)n) return;
  const size_t k = g / 12;
  const int r = (int)(g % 12), side = r / 6, c = r % 6;
  const int a = vi[k], b = vj[k];
  double* out = (side ? J1 : J0) + 36 * k + 6 * c;
  if (hidx[side ? b : a] < 0) {
#pragma unroll
    for (int i = 0; i < 6; ++i) out[i] = 0.0;
    return;
  }
  const double delta = 1e-9;
  const double scalar = 1.0 / (2 * delta);
  double Ci[7], Cj[7], Zi[7];
  pg_sbacam_load(est + 7 * (size_t)a, Ci);
  pg_sbacam_load(est + 7 * (size_t)b, Cj);
  pg_sbacam_load(zinv + 7 * k, Zi);
  double col[6];
#pragma unroll 1
  for (int pass = 0; pass < 2; ++pass) {
    double add[6], Cv[7], P[7], Pi[7], Pj[7], e[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) add[i] = (i == c) ? (pass ? -delta : delta) : 0.0;
#pragma unroll
    for (int i = 0; i < 7; ++i) Cv[i] = side ? Cj[i] : Ci[i];   // (a select per member: no pointer into the lane's arrays)
    pg_sbacam_oplus(Cv, add, P);
#pragma unroll
    for (int i = 0; i < 7; ++i) {
      Pi[i] = side ? Ci[i] : P[i];
      Pj[i] = side ? P[i] : Cj[i];
    }
    pg_sbacam_error(Pi, Pj, Zi, e);
#pragma unroll
    for (int i = 0; i < 6; ++i) col[i] = pass ? col[i] - e[i] : e[i];
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) out[i] = scalar * col[i];
}

// EdgeSBAScale: err [n][1], J0, J1 [n][1x6]; one lane per edge.  e = z - |tj - ti| (the squared norm summed x, y, z).  Column c < 3
// of side v is the central difference through SBACam::update, which adds the step to t_v.  A rotation step does not touch t_v:
// both evaluations of such a column read identical operands, their difference is exactly zero, so columns 3-5 are written as
// zeros without being evaluated.  The block of a fixed vertex is written as zeros.  Two cameras at one position give
// |dt| = delta in both evaluations of every column: a finite error and a zero Jacobian.
__device__ __forceinline__ double pg_sbascale_error(const double* ti, const double* tj, double z) {
#pragma clang fp contract(off)
  const double d[3] = {tj[0] - ti[0], tj[1] - ti[1], tj[2] - ti[2]};
  return z - sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
}
__global__ void __launch_bounds__(kThreads) pg_sbascale_linearize_kernel(int n, const double* __restrict__ est, const int* __restrict__ hidx,
                                                                       const int* __restrict__ vi, const int* __restrict__ vj,
                                                                       const double* __restrict__ meas, double* __restrict__ J0,
                                                                       double* __restrict__ J1, double* __restrict__ err, int jac) {
#pragma clang fp contract(off)
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const int a = vi[k], b = vj[k];
  const double* pi = est + 7 * (size_t)a;
  const double* pj = est + 7 * (size_t)b;
  const double ti[3] = {pi[0], pi[1], pi[2]}, tj[3] = {pj[0], pj[1], pj[2]};
  const double z = meas[k];
  err[k] = pg_sbascale_error(ti, tj, z);
  if (!jac) return;
  const double delta = 1e-9;
  const double scalar = 1.0 / (2 * delta);
  const bool free_i = hidx[a] >= 0, free_j = hidx[b] >= 0;
  double* o0 = J0 + 6 * (size_t)k;
  double* o1 = J1 + 6 * (size_t)k;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    double p[3], m[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      p[i] = ti[i] + (i == c ? delta : 0.0);
      m[i] = ti[i] + (i == c ? -delta : 0.0);
    }
    o0[c] = free_i ? scalar * (pg_sbascale_error(p, tj, z) - pg_sbascale_error(m, tj, z)) : 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      p[i] = tj[i] + (i == c ? delta : 0.0);
      m[i] = tj[i] + (i == c ? -delta : 0.0);
    }
    o1[c] = free_j ? scalar * (pg_sbascale_error(ti, p, z) - pg_sbascale_error(ti, m, z)) : 0.0;
  }
#pragma unroll
  for (int c = 3; c < 6; ++c) o0[c] = o1[c] = 0.0;
}
