// ---- sensor-offset pose-pose edges of a multi-sensor rig (included by block_solver.hip behind pg_gicp.inc, inside namespace
// g2ohip; types 18 and 19 of the pose-graph front end, a second pose-pose set beside a type-1 / type-2 one, in a slot of its own) --
//   EdgeSE3Offset::computeError / linearizeOplus   g2o/types/slam3d/edge_se3_offset.cpp:100-130
//   computeEdgeSE3Gradient (Pi, Pj given)          g2o/types/slam3d/isometry3d_gradients.h:86-192
//   compute_dq_dR                                  g2o/types/slam3d/dquat2mat.cpp (pg_dq_dR of block_solver.hip)
//   CacheSE3Offset::updateImpl                     g2o/types/slam3d/parameter_se3_offset.cpp:44-50 (n2w = X P, w2n = n2w^-1)
//   EdgeSE2Offset::computeError                    g2o/types/slam2d/edge_se2_offset.cpp:96-100
//   CacheSE2Offset::updateImpl                     g2o/types/slam2d/parameter_se2_offset.cpp:76-86
//   VertexSE2::oplusImpl / VertexSE3::oplusImpl    the updates of pg_se2_update_kernel / pg_se3_update_kernel
// Every edge names two rows of the offsets table: pf[k] is the sensor frame Pi on vertex 0, pt[k] the sensor frame Pj on vertex 1.
// Output in the layout of g2ohip_set_edge_data: J0, J1 [n][d x d] column-major, err [n][d], d = 3 (SE2) or 6 (SE3).  Blocks of
// fixed vertices are written like the others (the assembly does not read them); jac = 0 writes the errors only and leaves the
// Jacobians in place.  One lane per edge; lanes past the end evaluate the last edge and store nothing (every lane reaches the
// barriers of the staged form).  The arithmetic follows openslam_g2o_amd/offset_edges.py operation for operation and is compiled
// without contraction to fused multiply-adds, so that the fp64 evaluation there and the one here round alike up to sin / cos.
// That is why the isometry, quaternion and SE2 helpers are restated below (pg_offset_iso_mul / _iso_inv / _R_to_quat / _se2_mul /
// _se2_inverse / _normalize_theta): they are pg_iso_mul / pg_iso_inv / pg_R_to_quat / pg_se2_mul / pg_se2_inverse /
// pg_normalize_theta of block_solver.hip, the same operations in the same order, but those are compiled with the library's
// -ffp-contract=on, and a pragma at the call site does not reach into them.
//
// Type 19.  D = (Z^-1 (Xi Pi)^-1) (Xj Pj) in the association of computeError, e = toVectorMQT(D) (w >= 0).  The
// Jacobians are the full computeEdgeSE3Gradient with A = Z^-1 Pi^-1, B = Xi^-1 Xj, C = Pj:
//   Ji = [-Ra | Ra skewT(tbc); 0 | dq_dR [Ra Sxt(Rbc); Ra Syt(Rbc); Ra Szt(Rbc)]]
//   Jj = [Rab | Rab skew(tc);  0 | dq_dR [Rab Sx(Rc); Rab Sy(Rc); Rab Sz(Rc)]]
// (pg_se3_linearize_kernel hard-codes the two right-hand blocks of Jj for C = I).  This is the non-__clang__ branch of that
// function (Mx = Ra Sxt); its __clang__ branch multiplies the first block by Rab, an inconsistency of the reference and not the
// derivative.  dq_dR is taken at the rotation of D, the matrix the error's quaternion came from (the reference forms E = (A B) C a
// second time).  pg_offset_dq_dR below is pg_dq_dR -- the same operations in the same order -- with every index a compile-time
// constant: the 27 doubles stay in registers (pg_dq_dR's run-time indices put them into 224 bytes of scratch in
// pg_se3_linearize_kernel and pg_se3_prior_linearize_kernel).
//
// Type 18.  D = (Z^-1 (Xi Pi)^-1) (Xj Pj) with SE2's product and inverse (normalize_theta after every product, as se2.h),
// e = (D.t, D.angle).  DELIBERATE DEVIATION: the reference defines no Jacobian for this edge and differentiates numerically
// (base_binary_edge.hpp:132-201, delta = 1e-9).  The kernel writes the exact derivative with respect to VertexSE2::oplusImpl, as
// types 7 and the stereo edge do: with si = ti + R(thi) pi, sj = tj + R(thj) pj, M = R(thz + thi + ai)' (the rotation of
// Z^-1 (Xi Pi)^-1) and J = [0 -1; 1 0]
//   d e_t / d ti = -M     d e_t / d thi = -J M (sj - si) - M J R(thi) pi     d e_th / d thi = -1
//   d e_t / d tj =  M     d e_t / d thj =  M J R(thj) pj                     d e_th / d thj =  1
// so it agrees with the reference's numeric Jacobian up to that one's truncation and rounding error.
//
// Store forms of pg_landmark.inc (option pg_landmark_staged); both write the same bits.  A lane of the SE3 kernel holds 6 + 36 +
// 36 results: staged, a J array leaves in two halves of 128 edges through LDS rows of 37 doubles (ba_pose_store_halves of
// ba_pose_edge.inc: 128 x 37 x 8 = 37 888 bytes, what the other staged producers take), the errors through pg_store<true, 6> in the
// same buffer.
template <int N>
__device__ __forceinline__ void ba_pose_store_halves(double* lds, const double (&v)[N], double* __restrict__ out, int n);   // ba_pose_edge.inc

// ---- the shared helpers, restated without contraction (see above) ----
__device__ __forceinline__ void pg_offset_iso_mul(const double* A, const double* B, double* C) {
#pragma clang fp contract(off)
  double R[9], t[3];
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      double s = 0;
#pragma unroll
      for (int m = 0; m < 3; ++m) s += PG_R(A, r, m) * PG_R(B, m, c);
      R[r + 3 * c] = s;
    }
#pragma unroll
  for (int r = 0; r < 3; ++r) t[r] = PG_R(A, r, 0) * B[9] + PG_R(A, r, 1) * B[10] + PG_R(A, r, 2) * B[11] + A[9 + r];
#pragma unroll
  for (int i = 0; i < 9; ++i) C[i] = R[i];
  C[9] = t[0];
  C[10] = t[1];
  C[11] = t[2];
}
__device__ __forceinline__ void pg_offset_iso_inv(const double* A, double* C) {
#pragma clang fp contract(off)
  double R[9], t[3];
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int r = 0; r < 3; ++r) R[r + 3 * c] = PG_R(A, c, r);
#pragma unroll
  for (int r = 0; r < 3; ++r) t[r] = -(R[r] * A[9] + R[r + 3] * A[10] + R[r + 6] * A[11]);
#pragma unroll
  for (int i = 0; i < 9; ++i) C[i] = R[i];
  C[9] = t[0];
  C[10] = t[1];
  C[11] = t[2];
}
// the largest-diagonal case I of Quaterniond(R): q = (x, y, z, w), not yet normalised
template <int I>
__device__ __forceinline__ void pg_offset_quat_case(const double* R, double* q) {
#pragma clang fp contract(off)
  constexpr int J = (I + 1) % 3, K = (I + 2) % 3;
  double t = sqrt(PG_R(R, I, I) - PG_R(R, J, J) - PG_R(R, K, K) + 1.0);
  q[I] = 0.5 * t;
  t = 0.5 / t;
  q[3] = (PG_R(R, K, J) - PG_R(R, J, K)) * t;
  q[J] = (PG_R(R, J, I) + PG_R(R, I, J)) * t;
  q[K] = (PG_R(R, K, I) + PG_R(R, I, K)) * t;
}
// Quaterniond(R) (four cases), normalised, w >= 0 (isometry3d_mappings.cpp:38-44); q = (x, y, z, w)
__device__ __forceinline__ void pg_offset_R_to_quat(const double* R, double* q) {
#pragma clang fp contract(off)
  const double tr = PG_R(R, 0, 0) + PG_R(R, 1, 1) + PG_R(R, 2, 2);
  if (tr > 0) {
    double t = sqrt(tr + 1.0);
    q[3] = 0.5 * t;
    t = 0.5 / t;
    q[0] = (PG_R(R, 2, 1) - PG_R(R, 1, 2)) * t;
    q[1] = (PG_R(R, 0, 2) - PG_R(R, 2, 0)) * t;
    q[2] = (PG_R(R, 1, 0) - PG_R(R, 0, 1)) * t;
  } else {
    int i = 0;
    if (PG_R(R, 1, 1) > PG_R(R, 0, 0)) i = 1;
    if (PG_R(R, 2, 2) > (i == 1 ? PG_R(R, 1, 1) : PG_R(R, 0, 0))) i = 2;
    if (i == 0) pg_offset_quat_case<0>(R, q);
    else if (i == 1) pg_offset_quat_case<1>(R, q);
    else pg_offset_quat_case<2>(R, q);
  }
  const double nrm = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
#pragma unroll
  for (int i = 0; i < 4; ++i) q[i] /= nrm;
  if (q[3] < 0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) q[i] = -q[i];
  }
}
__device__ __forceinline__ double pg_offset_normalize_theta(double theta) {
#pragma clang fp contract(off)
  if (theta >= -M_PI && theta < M_PI) return theta;
  const double multiplier = floor(theta / (2 * M_PI));
  theta = theta - multiplier * 2 * M_PI;
  if (theta >= M_PI) theta -= 2 * M_PI;
  if (theta < -M_PI) theta += 2 * M_PI;
  return theta;
}
__device__ __forceinline__ void pg_offset_se2_inverse(const double* a, double* r) {
#pragma clang fp contract(off)
  const double th = pg_offset_normalize_theta(-a[2]), c = cos(th), s = sin(th);
  r[0] = c * (-a[0]) - s * (-a[1]);
  r[1] = s * (-a[0]) + c * (-a[1]);
  r[2] = th;
}
__device__ __forceinline__ void pg_offset_se2_mul(const double* a, const double* b, double* r) {
#pragma clang fp contract(off)
  const double c = cos(a[2]), s = sin(a[2]);
  const double x = a[0] + c * b[0] - s * b[1], y = a[1] + s * b[0] + c * b[1];
  r[0] = x;
  r[1] = y;
  r[2] = pg_offset_normalize_theta(a[2] + b[2]);
}

template <bool STAGED>
__device__ __forceinline__ void pg_offset_store36(double* lds, const double (&v)[36], double* __restrict__ out, int k, int n) {
  if constexpr (STAGED) {
    ba_pose_store_halves<36>(lds, v, out, n);
  } else {
    if (k < n) pg_store_direct<36>(v, out, (size_t)k);
  }
}

// rows C of the largest-diagonal case I of pg_dq_dR (C != I): 0.25 / s on (C, I) and (I, C), -dd, dd, dd on the diagonal
template <int I, int C>
__device__ __forceinline__ void pg_offset_dq_row(const double* R, double s, double (&D)[27]) {
#pragma clang fp contract(off)
  constexpr int J = (I + 1) % 3, K = (I + 2) % 3;
  const double num = PG_R(R, C, I) + PG_R(R, I, C);
  D[C * 9 + (C + 3 * I)] = 0.25 / s;
  D[C * 9 + (I + 3 * C)] = 0.25 / s;
  const double dd = num / (32.0 * s * s * s);
  D[C * 9 + (I + 3 * I)] = -dd;
  D[C * 9 + (J + 3 * J)] = dd;
  D[C * 9 + (K + 3 * K)] = dd;
}
template <int I>
__device__ __forceinline__ double pg_offset_dq_case(const double* R, double (&D)[27]) {
#pragma clang fp contract(off)
  constexpr int J = (I + 1) % 3, K = (I + 2) % 3;
  const double s = 0.5 * sqrt(1.0 + PG_R(R, I, I) - PG_R(R, J, J) - PG_R(R, K, K));
  const double qw = (PG_R(R, K, J) - PG_R(R, J, K)) / (4.0 * s);
  D[I * 9 + (I + 3 * I)] = 1.0 / (8.0 * s);
  D[I * 9 + (J + 3 * J)] = -1.0 / (8.0 * s);
  D[I * 9 + (K + 3 * K)] = -1.0 / (8.0 * s);
  pg_offset_dq_row<I, J>(R, s, D);
  pg_offset_dq_row<I, K>(R, s, D);
  return qw;
}
// d(qx,qy,qz)/d vec(R) (3 x 9, vec column-major; D row-major): pg_dq_dR with constant indices
__device__ __forceinline__ void pg_offset_dq_dR(const double* R, double (&D)[27]) {
#pragma clang fp contract(off)
#pragma unroll
  for (int i = 0; i < 27; ++i) D[i] = 0;
  const double r00 = PG_R(R, 0, 0), r11 = PG_R(R, 1, 1), r22 = PG_R(R, 2, 2);
  const double tr = r00 + r11 + r22;
  double qw;
  if (tr > 0) {
    const double w = 0.5 * sqrt(tr + 1.0);
    qw = w;
    const double d0 = -(PG_R(R, 2, 1) - PG_R(R, 1, 2)) / (32.0 * w * w * w);
    const double d1 = -(PG_R(R, 0, 2) - PG_R(R, 2, 0)) / (32.0 * w * w * w);
    const double d2 = -(PG_R(R, 1, 0) - PG_R(R, 0, 1)) / (32.0 * w * w * w);
    const double p = 0.25 / w, m = -0.25 / w;
    D[0] = d0; D[4] = d0; D[8] = d0; D[2 + 3 * 1] = p; D[1 + 3 * 2] = m;                       // row 0: (2, 1), (1, 2)
    D[9] = d1; D[9 + 4] = d1; D[9 + 8] = d1; D[9 + 0 + 3 * 2] = p; D[9 + 2 + 3 * 0] = m;       // row 1: (0, 2), (2, 0)
    D[18] = d2; D[18 + 4] = d2; D[18 + 8] = d2; D[18 + 1 + 3 * 0] = p; D[18 + 0 + 3 * 1] = m;  // row 2: (1, 0), (0, 1)
  } else if ((r00 > r11) & (r00 > r22)) {
    qw = pg_offset_dq_case<0>(R, D);
  } else if (r11 > r22) {
    qw = pg_offset_dq_case<1>(R, D);
  } else {
    qw = pg_offset_dq_case<2>(R, D);
  }
  if (qw <= 0) {
#pragma unroll
    for (int i = 0; i < 27; ++i) D[i] = -D[i];
  }
}

// the lower-right block of a Jacobian: column a = D vec(L S_a), S_a the a-th doubled generator applied to R2 = 2 R; SIGN = +1:
// skew(Sx, Sy, Sz, R) of isometry3d_gradients.h:58-70, SIGN = -1: skewT (:72-84)
template <int SIGN>
__device__ __forceinline__ void pg_offset_rot_block(const double* L, const double* R, const double (&D)[27], double (&J)[36]) {
#pragma clang fp contract(off)
  double r2[9];   // SIGN * 2 R, column-major
#pragma unroll
  for (int i = 0; i < 9; ++i) r2[i] = SIGN * (2 * R[i]);
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    // rows of S_a: row a is zero, row (a + 1) % 3 is -r2[(a + 2) % 3][:], row (a + 2) % 3 is r2[(a + 1) % 3][:]
    constexpr int kNext[3] = {1, 2, 0}, kPrev[3] = {2, 0, 1};
    const int b = kNext[a], c = kPrev[a];
    double M[9];
#pragma unroll
    for (int col = 0; col < 3; ++col)
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        double s = 0;
#pragma unroll
        for (int m = 0; m < 3; ++m) {
          const double sm = m == a ? 0.0 : m == b ? -PG_R(r2, c, col) : PG_R(r2, b, col);
          s += PG_R(L, r, m) * sm;
        }
        M[r + 3 * col] = s;
      }
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      double s = 0;
#pragma unroll
      for (int m = 0; m < 9; ++m) s += D[r * 9 + m] * M[m];
      J[(3 + r) + 6 * (3 + a)] = s;
    }
  }
}

// the upper blocks of a Jacobian: [SIGN L | L S], S = skew(t) (SIGN = +1, isometry3d_gradients.h:42-48) or skewT(t) (SIGN = -1,
// :50-56) of the doubled t; the lower-left block is zero
template <int SIGN>
__device__ __forceinline__ void pg_offset_upper_blocks(const double* L, const double* t, double (&J)[36]) {
#pragma clang fp contract(off)
#pragma unroll
  for (int i = 0; i < 36; ++i) J[i] = 0;
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int r = 0; r < 3; ++r) J[r + 6 * c] = SIGN > 0 ? PG_R(L, r, c) : -PG_R(L, r, c);
  const double x = SIGN * (2 * t[0]), y = SIGN * (2 * t[1]), z = SIGN * (2 * t[2]);
  double S[9];
  PG_R(S, 0, 0) = 0; PG_R(S, 0, 1) = z; PG_R(S, 0, 2) = -y;
  PG_R(S, 1, 0) = -z; PG_R(S, 1, 1) = 0; PG_R(S, 1, 2) = x;
  PG_R(S, 2, 0) = y; PG_R(S, 2, 1) = -x; PG_R(S, 2, 2) = 0;
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      double s = 0;
#pragma unroll
      for (int m = 0; m < 3; ++m) s += PG_R(L, r, m) * PG_R(S, m, c);
      J[r + 6 * (3 + c)] = s;
    }
}

template <bool STAGED>
__global__ void __launch_bounds__(kThreads) pg_se3_offset_linearize_kernel(int n, const double* __restrict__ poses, const int* __restrict__ vi,
                                                                         const int* __restrict__ vj, const int* __restrict__ pf,
                                                                         const int* __restrict__ pt, const double* __restrict__ meas,
                                                                         const double* __restrict__ offsets, double* __restrict__ J0,
                                                                         double* __restrict__ J1, double* __restrict__ err, int jac) {
#pragma clang fp contract(off)
  __shared__ double lds[STAGED ? (kThreads / 2) * 37 : 1];   // (>= kThreads * 7: the errors pass through it in one piece)
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  const int kk = min(k, n - 1);   // (lanes past the end evaluate the last edge and store nothing)
  double Xi[12], Xj[12], Pi[12], Pj[12], Zi[12], T[12], U[12], E[12], q[4];
  {
    const double* xi = poses + 12 * (size_t)vi[kk];
    const double* xj = poses + 12 * (size_t)vj[kk];
    const double* pi = offsets + 12 * (size_t)pf[kk];
    const double* pj = offsets + 12 * (size_t)pt[kk];
#pragma unroll
    for (int i = 0; i < 12; ++i) {
      Xi[i] = xi[i];
      Xj[i] = xj[i];
      Pi[i] = pi[i];
      Pj[i] = pj[i];
    }
  }
  pg_offset_iso_inv(meas + 12 * (size_t)kk, Zi);
  pg_offset_iso_mul(Xi, Pi, T);    // n2w of vertex 0
  pg_offset_iso_inv(T, U);         // w2n of vertex 0
  pg_offset_iso_mul(Zi, U, T);     // Z^-1 (Xi Pi)^-1
  pg_offset_iso_mul(Xj, Pj, U);    // n2w of vertex 1
  pg_offset_iso_mul(T, U, E);
  pg_offset_R_to_quat(E, q);
  const double e[6] = {E[9], E[10], E[11], q[0], q[1], q[2]};
  pg_store<STAGED, 6>(lds, e, err, k, n);
  if (!jac) return;
  double A[12], B[12], D[27], J[36];
  pg_offset_iso_inv(Pi, U);
  pg_offset_iso_mul(Zi, U, A);     // A = Z^-1 Pi^-1
  pg_offset_iso_inv(Xi, U);
  pg_offset_iso_mul(U, Xj, B);     // B = Xi^-1 Xj
  pg_offset_iso_mul(B, Pj, T);     // BC
  pg_offset_dq_dR(E, D);
  pg_offset_upper_blocks<-1>(A, T + 9, J);   // -Ra | Ra skewT(tbc)
  pg_offset_rot_block<-1>(A, T, D, J);       // dq_dR [Ra Sxt(Rbc); ...]
  pg_offset_store36<STAGED>(lds, J, J0, k, n);
  pg_offset_iso_mul(A, B, U);      // AB
  pg_offset_upper_blocks<1>(U, Pj + 9, J);   // Rab | Rab skew(tc)
  pg_offset_rot_block<1>(U, Pj, D, J);       // dq_dR [Rab Sx(Rc); ...]
  pg_offset_store36<STAGED>(lds, J, J1, k, n);
}

template <bool STAGED>
__global__ void __launch_bounds__(kThreads) pg_se2_offset_linearize_kernel(int n, const double* __restrict__ poses, const int* __restrict__ vi,
                                                                         const int* __restrict__ vj, const int* __restrict__ pf,
                                                                         const int* __restrict__ pt, const double* __restrict__ meas,
                                                                         const double* __restrict__ offsets, double* __restrict__ J0,
                                                                         double* __restrict__ J1, double* __restrict__ err, int jac) {
#pragma clang fp contract(off)
  __shared__ double lds[STAGED ? kThreads * 9 : 1];
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  const int kk = min(k, n - 1);   // (lanes past the end evaluate the last edge and store nothing)
  double xi[3], xj[3], pi[3], pj[3], z[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    xi[i] = poses[3 * (size_t)vi[kk] + i];
    xj[i] = poses[3 * (size_t)vj[kk] + i];
    pi[i] = offsets[3 * (size_t)pf[kk] + i];
    pj[i] = offsets[3 * (size_t)pt[kk] + i];
    z[i] = meas[3 * (size_t)kk + i];
  }
  double invm[3], a[3], w2n[3], n2w[3], T[3], delta[3];
  pg_offset_se2_inverse(z, invm);
  pg_offset_se2_mul(xi, pi, a);      // n2w of vertex 0
  pg_offset_se2_inverse(a, w2n);
  pg_offset_se2_mul(xj, pj, n2w);
  pg_offset_se2_mul(invm, w2n, T);   // Z^-1 (Xi Pi)^-1
  pg_offset_se2_mul(T, n2w, delta);
  const double e[3] = {delta[0], delta[1], delta[2]};
  pg_store<STAGED, 3>(lds, e, err, k, n);
  if (!jac) return;
  const double cm = cos(T[2]), sm = sin(T[2]);
  const double ci = cos(xi[2]), si = sin(xi[2]), cj = cos(xj[2]), sj = sin(xj[2]);
  const double rpi0 = ci * pi[0] - si * pi[1], rpi1 = si * pi[0] + ci * pi[1];   // R(thi) pi
  const double rpj0 = cj * pj[0] - sj * pj[1], rpj1 = sj * pj[0] + cj * pj[1];   // R(thj) pj
  const double dx = (xj[0] + rpj0) - (xi[0] + rpi0), dy = (xj[1] + rpj1) - (xi[1] + rpi1);   // sj - si
  const double a0 = -rpi1, a1 = rpi0, b0 = -rpj1, b1 = rpj0;                     // J R(thi) pi, J R(thj) pj
  const double jmd0 = -(sm * dx) - cm * dy, jmd1 = cm * dx - sm * dy;            // J M (sj - si)
  const double ma0 = cm * a0 - sm * a1, ma1 = sm * a0 + cm * a1;
  const double mb0 = cm * b0 - sm * b1, mb1 = sm * b0 + cm * b1;
  const double ja[9] = {-cm, -sm, 0, sm, -cm, 0, -jmd0 - ma0, -jmd1 - ma1, -1};   // column-major 3x3
  const double jb[9] = {cm, sm, 0, -sm, cm, 0, mb0, mb1, 1};
  pg_store<STAGED, 9>(lds, ja, J0, k, n);
  pg_store<STAGED, 9>(lds, jb, J1, k, n);
}
