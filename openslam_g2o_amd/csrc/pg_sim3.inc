// ---- Sim3 pose-pose edges of the pose-graph front end (included by block_solver.hip behind pg_prior.inc, inside namespace
// g2ohip) --------------------------------------------------------------------------------------------------------------------
//   Sim3(const Vector7d&) / log / inverse / operator*    g2o/types/sim3/sim3.h:70-142, 148-230, 233-236, 266-272
//   VertexSim3Expmap::oplusImpl                          g2o/types/sim3/types_seven_dof_expmap.h:56-65 (S <- exp(x) S, _fix_scale)
//   EdgeSim3::computeError                               g2o/types/sim3/types_seven_dof_expmap.h:94-102 (e = log(C Si Sj^-1))
//   BaseBinaryEdge::linearizeOplus, numeric branch       g2o/core/base_binary_edge.hpp:132-201 (central, delta = 1e-9)
// A Sim3 is 8 doubles (qx, qy, qz, qw, tx, ty, tz, s), the members of the reference's struct; a minimal vector is (omega,
// upsilon, sigma).  The helpers restate the reference operation for operation, the pieces of Eigen it goes through included
// (Quaternion(Matrix3), toRotationMatrix, quaternion product, quaternion * vector, partial-pivot LU), and in its order of
// floating-point operations: the reference defines NO Jacobian for this edge, g2o differentiates the error numerically with a
// step of 1e-9, and 1 / (2 delta) = 5e8 carries every rounding of the error into the Jacobian -- so the functions below are
// compiled without contraction to fused multiply-adds (the tree's default is -ffp-contract=on), as the reference's host build
// is, and tests/sim3_helpers.py states the same operations in fp64 and at 60 digits.

__device__ __forceinline__ void pg_sim3_qmul(const double* a, const double* b, double* r) {
#pragma clang fp contract(off)
  r[0] = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1];
  r[1] = a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2];
  r[2] = a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0];
  r[3] = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2];
}
// quaternion * vector: uv = 2 (q.vec x v), v + w uv + q.vec x uv
__device__ __forceinline__ void pg_sim3_qrot(const double* q, const double* v, double* r) {
#pragma clang fp contract(off)
  double ux = q[1] * v[2] - q[2] * v[1], uy = q[2] * v[0] - q[0] * v[2], uz = q[0] * v[1] - q[1] * v[0];
  ux += ux; uy += uy; uz += uz;
  r[0] = v[0] + q[3] * ux + (q[1] * uz - q[2] * uy);
  r[1] = v[1] + q[3] * uy + (q[2] * ux - q[0] * uz);
  r[2] = v[2] + q[3] * uz + (q[0] * uy - q[1] * ux);
}
// toRotationMatrix, R row-major [3 i + j]
__device__ __forceinline__ void pg_sim3_q_to_R(const double* q, double* R) {
#pragma clang fp contract(off)
  const double x = q[0], y = q[1], z = q[2], w = q[3];
  const double tx = x + x, ty = y + y, tz = z + z;
  const double twx = tx * w, twy = ty * w, twz = tz * w, txx = tx * x, txy = ty * x, txz = tz * x, tyy = ty * y, tyz = tz * y,
               tzz = tz * z;
  R[0] = 1 - (tyy + tzz); R[1] = txy - twz; R[2] = txz + twy;
  R[3] = txy + twz; R[4] = 1 - (txx + tzz); R[5] = tyz - twx;
  R[6] = txz - twy; R[7] = tyz + twx; R[8] = 1 - (txx + tyy);
}
// Quaternion(Matrix3): trace > 0, else by the largest diagonal entry (register-resident: no run-time indexed array)
__device__ __forceinline__ void pg_sim3_R_to_q(const double* R, double* q) {
#pragma clang fp contract(off)
  double t = R[0] + R[4] + R[8];
  if (t > 0) {
    t = sqrt(t + 1.0);
    q[3] = 0.5 * t;
    t = 0.5 / t;
    q[0] = (R[7] - R[5]) * t;
    q[1] = (R[2] - R[6]) * t;
    q[2] = (R[3] - R[1]) * t;
    return;
  }
  int i = 0;
  if (R[4] > R[0]) i = 1;
  if (R[8] > (i ? R[4] : R[0])) i = 2;
  if (i == 0) {          // j = 1, k = 2
    t = sqrt(R[0] - R[4] - R[8] + 1.0);
    q[0] = 0.5 * t;
    t = 0.5 / t;
    q[3] = (R[7] - R[5]) * t;
    q[1] = (R[3] + R[1]) * t;
    q[2] = (R[6] + R[2]) * t;
  } else if (i == 1) {   // j = 2, k = 0
    t = sqrt(R[4] - R[8] - R[0] + 1.0);
    q[1] = 0.5 * t;
    t = 0.5 / t;
    q[3] = (R[2] - R[6]) * t;
    q[2] = (R[7] + R[5]) * t;
    q[0] = (R[1] + R[3]) * t;
  } else {               // j = 0, k = 1
    t = sqrt(R[8] - R[0] - R[4] + 1.0);
    q[2] = 0.5 * t;
    t = 0.5 / t;
    q[3] = (R[3] - R[1]) * t;
    q[0] = (R[2] + R[6]) * t;
    q[1] = (R[5] + R[7]) * t;
  }
}
// the coefficients of W = A Omega + B Omega^2 + C I that exp and log share (theta: the rotation angle, unused when small)
__device__ __forceinline__ void pg_sim3_abc(double sigma, double s, double theta, bool small_sigma, bool small_theta, double& A,
                                            double& B, double& C) {
#pragma clang fp contract(off)
  if (small_sigma) {
    C = 1;
    if (small_theta) {
      A = 1. / 2.;
      B = 1. / 6.;
    } else {
      const double theta2 = theta * theta;
      A = (1 - cos(theta)) / theta2;
      B = (theta - sin(theta)) / (theta2 * theta);
    }
  } else {
    C = (s - 1) / sigma;
    if (small_theta) {
      const double sigma2 = sigma * sigma;
      A = ((sigma - 1) * s + 1) / sigma2;
      B = ((0.5 * sigma2 - sigma + 1) * s) / (sigma2 * sigma);
    } else {
      const double a = s * sin(theta), b = s * cos(theta);
      const double theta2 = theta * theta, sigma2 = sigma * sigma;
      const double c = theta2 + sigma2;
      A = (a * sigma + (1 - b) * theta) / (theta * c);
      B = (C - ((b - 1) * sigma + a * theta) / c) * 1. / theta2;
    }
  }
}
// skew(o) and its square, row-major
__device__ __forceinline__ void pg_sim3_skew(const double* o, double* Om) {
  Om[0] = 0; Om[1] = -o[2]; Om[2] = o[1];
  Om[3] = o[2]; Om[4] = 0; Om[5] = -o[0];
  Om[6] = -o[1]; Om[7] = o[0]; Om[8] = 0;
}
__device__ __forceinline__ void pg_sim3_mat3_mul(const double* A, const double* B, double* C) {
#pragma clang fp contract(off)
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) C[3 * i + j] = A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j] + A[3 * i + 2] * B[6 + j];
}

// Sim3(const Vector7d& update)
__device__ __forceinline__ void pg_sim3_exp(const double* u, double* S) {
#pragma clang fp contract(off)
  const double eps = 0.00001;
  const double sigma = u[6];
  const double theta = sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
  double Om[9], Om2[9], R[9];
  pg_sim3_skew(u, Om);
  const double s = exp(sigma);
  pg_sim3_mat3_mul(Om, Om, Om2);
  const bool small_sigma = fabs(sigma) < eps, small_theta = theta < eps;
  double A, B, C;
  pg_sim3_abc(sigma, s, theta, small_sigma, small_theta, A, B, C);
  if (small_theta) {
#pragma unroll
    for (int i = 0; i < 9; ++i) R[i] = (i % 4 == 0 ? 1.0 : 0.0) + Om[i] + Om2[i];
  } else {
    const double k1 = sin(theta) / theta, k2 = (1 - cos(theta)) / (theta * theta);
#pragma unroll
    for (int i = 0; i < 9; ++i) R[i] = (i % 4 == 0 ? 1.0 : 0.0) + k1 * Om[i] + k2 * Om2[i];
  }
  pg_sim3_R_to_q(R, S);
  double W[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) W[i] = A * Om[i] + B * Om2[i] + C * (i % 4 == 0 ? 1.0 : 0.0);
#pragma unroll
  for (int i = 0; i < 3; ++i) S[4 + i] = W[3 * i] * u[3] + W[3 * i + 1] * u[4] + W[3 * i + 2] * u[5];
  S[7] = s;
}

// 3x3 solve by LU with partial pivoting (largest |entry| of the column, the first on ties); rows held in registers, the
// exchanges are selects
__device__ __forceinline__ void pg_sim3_lu_solve(const double* W, const double* b, double* x) {
#pragma clang fp contract(off)
  double a0[4] = {W[0], W[1], W[2], b[0]}, a1[4] = {W[3], W[4], W[5], b[1]}, a2[4] = {W[6], W[7], W[8], b[2]};
  auto swap_rows = [](double* p, double* q, bool doit) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const double pv = p[k], qv = q[k];
      p[k] = doit ? qv : pv;
      q[k] = doit ? pv : qv;
    }
  };
  {  // column 0
    int p = 0;
    if (fabs(a1[0]) > fabs(a0[0])) p = 1;
    if (fabs(a2[0]) > fabs(p ? a1[0] : a0[0])) p = 2;
    swap_rows(a0, a1, p == 1);
    swap_rows(a0, a2, p == 2);
    const double f1 = a1[0] / a0[0], f2 = a2[0] / a0[0];
#pragma unroll
    for (int k = 1; k < 4; ++k) {
      a1[k] = a1[k] - f1 * a0[k];
      a2[k] = a2[k] - f2 * a0[k];
    }
  }
  {  // column 1
    swap_rows(a1, a2, fabs(a2[1]) > fabs(a1[1]));
    const double f = a2[1] / a1[1];
    a2[2] = a2[2] - f * a1[2];
    a2[3] = a2[3] - f * a1[3];
  }
  x[2] = a2[3] / a2[2];
  x[1] = (a1[3] - a1[2] * x[2]) / a1[1];
  x[0] = (a0[3] - a0[1] * x[1] - a0[2] * x[2]) / a0[0];
}

// Sim3::log
__device__ __forceinline__ void pg_sim3_log(const double* S, double* e) {
#pragma clang fp contract(off)
  const double eps = 0.00001;
  const double s = S[7];
  const double sigma = log(s);
  double R[9];
  pg_sim3_q_to_R(S, R);
  const double d = 0.5 * (R[0] + R[4] + R[8] - 1);
  const double dR[3] = {R[7] - R[5], R[2] - R[6], R[3] - R[1]};
  const bool small_sigma = fabs(sigma) < eps, small_theta = d > 1 - eps;
  double theta = 0, om[3];
  if (small_theta) {
#pragma unroll
    for (int i = 0; i < 3; ++i) om[i] = 0.5 * dR[i];
  } else {
    theta = acos(d);
    const double k = theta / (2 * sqrt(1 - d * d));
#pragma unroll
    for (int i = 0; i < 3; ++i) om[i] = k * dR[i];
  }
  double A, B, C;
  pg_sim3_abc(sigma, s, theta, small_sigma, small_theta, A, B, C);
  double Om[9], BOm[9], BOm2[9], W[9];
  pg_sim3_skew(om, Om);
#pragma unroll
  for (int i = 0; i < 9; ++i) BOm[i] = B * Om[i];
  pg_sim3_mat3_mul(BOm, Om, BOm2);   // (B * Omega) * Omega, as the expression associates
#pragma unroll
  for (int i = 0; i < 9; ++i) W[i] = A * Om[i] + BOm2[i] + C * (i % 4 == 0 ? 1.0 : 0.0);
  pg_sim3_lu_solve(W, S + 4, e + 3);
  e[0] = om[0]; e[1] = om[1]; e[2] = om[2];
  e[6] = sigma;
}

__device__ __forceinline__ void pg_sim3_inverse(const double* S, double* r) {
#pragma clang fp contract(off)
  r[0] = -S[0]; r[1] = -S[1]; r[2] = -S[2]; r[3] = S[3];
  const double k = -1. / S[7];
  const double t[3] = {k * S[4], k * S[5], k * S[6]};
  pg_sim3_qrot(r, t, r + 4);
  r[7] = 1. / S[7];
}
__device__ __forceinline__ void pg_sim3_mul(const double* a, const double* b, double* r) {
#pragma clang fp contract(off)
  double rt[3];
  pg_sim3_qmul(a, b, r);
  pg_sim3_qrot(a, b + 4, rt);
#pragma unroll
  for (int i = 0; i < 3; ++i) r[4 + i] = a[7] * rt[i] + a[4 + i];
  r[7] = a[7] * b[7];
}
__device__ __forceinline__ void pg_sim3_load(const double* __restrict__ p, double* S) {
#pragma unroll
  for (int i = 0; i < 8; ++i) S[i] = p[i];
}

// err [n][7]: one lane per edge
__global__ void __launch_bounds__(kThreads) pg_sim3_error_kernel(int n, const double* __restrict__ est, const int* __restrict__ vi,
                                                               const int* __restrict__ vj, const double* __restrict__ meas,
                                                               double* __restrict__ err) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  double Si[8], Sj[8], Cm[8], A[8], Bi[8], E[8], e[7];
  pg_sim3_load(est + 8 * (size_t)vi[k], Si);
  pg_sim3_load(est + 8 * (size_t)vj[k], Sj);
  pg_sim3_load(meas + 8 * (size_t)k, Cm);
  pg_sim3_mul(Cm, Si, A);
  pg_sim3_inverse(Sj, Bi);
  pg_sim3_mul(A, Bi, E);
  pg_sim3_log(E, e);
#pragma unroll
  for (int i = 0; i < 7; ++i) err[7 * (size_t)k + i] = e[i];
}

// J0, J1 [n][7x7] column-major: one lane per (edge, side, column), 14 lanes per edge -- 28 evaluations of exp . mul . mul . log
// per edge spread over 14 lanes, a lane's state is one column (no 49-entry block in registers), and the 14 lanes of an edge
// store 2 x 49 contiguous doubles, so the stores are dense without an LDS stage.  Column c of side v:
//   (e(exp(+delta u_c) S_v) - e(exp(-delta u_c) S_v)) / (2 delta),
// the perturbation through oplusImpl (with fix_scale the sigma entry of the step is zeroed: both evaluations coincide and column
// 6 is exactly zero).  The block of a fixed vertex (hidx < 0) is written as zeros; the reference leaves it unset and the assembly
// does not read it.  The two signs run through ONE loop body (not unrolled): the body holds every transcendental of the kernel.
__global__ void __launch_bounds__(kThreads) pg_sim3_jacobian_kernel(int n, const double* __restrict__ est, const int* __restrict__ hidx,
                                                                  const int* __restrict__ vi, const int* __restrict__ vj,
                                                                  const double* __restrict__ meas, int fix_scale,
                                                                  double* __restrict__ J0, double* __restrict__ J1) {
#pragma clang fp contract(off)
  const size_t g = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (g >= 14 * (size_t)n) return;
  const size_t k = g / 14;
  const int r = (int)(g % 14), side = r / 7, c = r % 7;
  const int a = vi[k], b = vj[k];
  double* out = (side ? J1 : J0) + 49 * k + 7 * c;
  if (hidx[side ? b : a] < 0) {
#pragma unroll
    for (int i = 0; i < 7; ++i) out[i] = 0.0;
    return;
  }
  const double delta = 1e-9;
  const double scalar = 1.0 / (2 * delta);
  double Si[8], Sj[8], Cm[8], A[8], Bi[8];
  pg_sim3_load(est + 8 * (size_t)a, Si);
  pg_sim3_load(est + 8 * (size_t)b, Sj);
  pg_sim3_load(meas + 8 * k, Cm);
  pg_sim3_mul(Cm, Si, A);      // side 1 perturbs Sj: C Si stands
  pg_sim3_inverse(Sj, Bi);     // side 0 perturbs Si: Sj^-1 stands
  double col[7];
#pragma unroll 1
  for (int pass = 0; pass < 2; ++pass) {
    double add[7], X[8], Sv[8], P[8], T[8], E[8], e[7];
#pragma unroll
    for (int i = 0; i < 7; ++i) add[i] = (i == c) ? (pass ? -delta : delta) : 0.0;
    if (fix_scale) add[6] = 0.0;
    pg_sim3_exp(add, X);
#pragma unroll
    for (int i = 0; i < 8; ++i) Sv[i] = side ? Sj[i] : Si[i];   // (a select per member: no pointer into the lane's arrays)
    pg_sim3_mul(X, Sv, P);
    if (side == 0) {
      pg_sim3_mul(Cm, P, T);
      pg_sim3_mul(T, Bi, E);
    } else {
      pg_sim3_inverse(P, T);
      pg_sim3_mul(A, T, E);
    }
    pg_sim3_log(E, e);
#pragma unroll
    for (int i = 0; i < 7; ++i) col[i] = pass ? col[i] - e[i] : e[i];
  }
#pragma unroll
  for (int i = 0; i < 7; ++i) out[i] = scalar * col[i];
}

// S_v <- exp(x_v) S_v for every free vertex (x_v[6] taken as 0 with fix_scale); nothing is renormalised
__global__ void __launch_bounds__(kThreads) pg_sim3_update_kernel(int nv, double* __restrict__ est, const int* __restrict__ hidx,
                                                                const double* __restrict__ x, int fix_scale) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= nv || hidx[v] < 0) return;
  const double* u = x + 7 * (size_t)hidx[v];
  double add[7], X[8], S[8], P[8];
#pragma unroll
  for (int i = 0; i < 7; ++i) add[i] = u[i];
  if (fix_scale) add[6] = 0.0;
  pg_sim3_load(est + 8 * (size_t)v, S);
  pg_sim3_exp(add, X);
  pg_sim3_mul(X, S, P);
#pragma unroll
  for (int i = 0; i < 8; ++i) est[8 * (size_t)v + i] = P[i];
}
