// ---- unary pose priors of the pose-graph front end (included by block_solver.hip behind pg_landmark.inc, inside namespace
// g2ohip) --------------------------------------------------------------------------------------------------------------------
//   EdgeSE2Prior::computeError                       g2o/types/slam2d/edge_se2_prior.h:45-50
//   EdgeSE2XYPrior::computeError / linearizeOplus    g2o/types/slam2d/edge_se2_xyprior.h:66-70, edge_se2_xyprior.cpp:60-63
//   EdgeSE3Prior::computeError / linearizeOplus      g2o/types/slam3d/edge_se3_prior.cpp:94-107, computeEdgeSE3PriorGradient of
//                                                    isometry3d_gradients.h:269-330
//   CacheSE3Offset::updateImpl                       g2o/types/slam3d/parameter_se3_offset.cpp:44-50 (n2w = X offset)
//   VertexSE2::oplusImpl                             g2o/types/slam2d/vertex_se2.h:51-58 (additive, angle normalised)
// The only vertex of an edge is a pose (index vq into the pose table).  Output in the layout of g2ohip_set_edge_data for a UNARY
// set: J0 [n][d x dim] column-major, err [n][d]; there is no J1.  One lane per edge, store forms of pg_landmark.inc.
//
// EdgeSE2Prior: the reference compiles its analytic linearizeOplus out (edge_se2_prior.h:52-58, "#if 0 // this is untested") and
// differentiates the error numerically.  This kernel writes the exact derivative of e = (Z^-1 X).toVector() = (Rz' (t - tz),
// normalize(theta - theta_z)) with respect to the additive VertexSE2::oplusImpl, J = [Rz' 0; 0 1] -- which is also what the
// disabled reference code states -- so it agrees with the reference's numeric Jacobian up to that one's truncation error.
template <int TYPE, bool STAGED>
__global__ void __launch_bounds__(kThreads) pg_se2_prior_linearize_kernel(int n, const double* __restrict__ poses,
                                                                        const int* __restrict__ vq, const double* __restrict__ meas,
                                                                        double* __restrict__ J0, double* __restrict__ err, int jac) {
  static_assert(TYPE == 7 || TYPE == 8, "EdgeSE2Prior, EdgeSE2XYPrior");
  __shared__ double lds[STAGED ? kThreads * (TYPE == 7 ? 9 : 7) : 1];
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  const int kk = min(k, n - 1);   // (lanes past the end evaluate the last edge and store nothing)
  const double* x = poses + 3 * (size_t)vq[kk];
  if constexpr (TYPE == 7) {
    double invm[3], delta[3];
    pg_se2_inverse(meas + 3 * (size_t)kk, invm);
    pg_se2_mul(invm, x, delta);
    const double e[3] = {delta[0], delta[1], delta[2]};
    pg_store<STAGED, 3>(lds, e, err, k, n);
    if (!jac) return;
    const double cz = cos(invm[2]), sz = sin(invm[2]);   // R(Z^-1) = Rz'
    const double a[9] = {cz, sz, 0, -sz, cz, 0, 0, 0, 1};   // column-major 3x3
    pg_store<STAGED, 9>(lds, a, J0, k, n);
  } else {
    // e = t - z, J = [1 0 0; 0 1 0]
    const double e[2] = {x[0] - meas[2 * (size_t)kk], x[1] - meas[2 * (size_t)kk + 1]};
    pg_store<STAGED, 2>(lds, e, err, k, n);
    if (!jac) return;
    const double a[6] = {1, 0, 0, 1, 0, 0};   // column-major 2x3
    pg_store<STAGED, 6>(lds, a, J0, k, n);
  }
}

// EdgeSE3Prior with ONE ParameterSE3Offset P for the set: A = Z^-1 X, E = A P, e = toVectorMQT(E) -- translation, then the
// vector part of the unit quaternion with w >= 0, the convention (sign included) of pg_se3_linearize_kernel.  Jacobian with
// respect to VertexSE3::oplusImpl (X <- X fromVectorMQT(u)), computeEdgeSE3PriorGradient:
//   J[0:3,0:3] = Ra, J[0:3,3:6] = Ra skew(tP), J[3:6,3:6] = dq_dR(Re) [Ra Sx(RP); Ra Sy(RP); Ra Sz(RP)], the rest zero,
// skew(t) = -2 [t]x and Sx, Sy, Sz the doubled generators applied to RP (isometry3d_gradients.h:42-70).
// The staged store form passes the 36 doubles of J through LDS in one piece: 256 x 37 doubles = 74 KiB of the 160 KiB of a
// gfx950 compute unit.
template <bool STAGED>
__global__ void __launch_bounds__(kThreads) pg_se3_prior_linearize_kernel(int n, const double* __restrict__ poses,
                                                                        const int* __restrict__ vq, const double* __restrict__ meas,
                                                                        PgIso offset, double* __restrict__ J0, double* __restrict__ err,
                                                                        int jac) {
  __shared__ double lds[STAGED ? kThreads * 37 : 1];
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  const int kk = min(k, n - 1);   // (lanes past the end evaluate the last edge and store nothing)
  const double* Xp = poses + 12 * (size_t)vq[kk];
  const double* Zp = meas + 12 * (size_t)kk;
  double X[12], Z[12], Zi[12], A[12], E[12], q[4];
#pragma unroll
  for (int i = 0; i < 12; ++i) {
    X[i] = Xp[i];
    Z[i] = Zp[i];
  }
  pg_iso_inv(Z, Zi);
  pg_iso_mul(Zi, X, A);
  pg_iso_mul(A, offset.v, E);
  pg_R_to_quat(E, q);
  const double e[6] = {E[9], E[10], E[11], q[0], q[1], q[2]};
  pg_store<STAGED, 6>(lds, e, err, k, n);
  if (!jac) return;
  double J[36];   // column-major 6x6
#pragma unroll
  for (int i = 0; i < 36; ++i) J[i] = 0;
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int r = 0; r < 3; ++r) J[r + 6 * c] = PG_R(A, r, c);
  {  // dte/dq = Ra skew(tP) (doubled components)
    const double x = 2 * offset.v[9], y = 2 * offset.v[10], z = 2 * offset.v[11];
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
        for (int m = 0; m < 3; ++m) s += PG_R(A, r, m) * PG_R(S, m, c);
        J[r + 6 * (3 + c)] = s;
      }
  }
  double D[27];
  pg_dq_dR(E, D);
  {  // dre/dq
    const double* Rp = offset.v;
    const double r11 = 2 * PG_R(Rp, 0, 0), r12 = 2 * PG_R(Rp, 0, 1), r13 = 2 * PG_R(Rp, 0, 2), r21 = 2 * PG_R(Rp, 1, 0),
                 r22 = 2 * PG_R(Rp, 1, 1), r23 = 2 * PG_R(Rp, 1, 2), r31 = 2 * PG_R(Rp, 2, 0), r32 = 2 * PG_R(Rp, 2, 1),
                 r33 = 2 * PG_R(Rp, 2, 2);
    const double S[3][9] = {{0, 0, 0, -r31, -r32, -r33, r21, r22, r23}, {r31, r32, r33, 0, 0, 0, -r11, -r12, -r13},
                            {-r21, -r22, -r23, r11, r12, r13, 0, 0, 0}};   // row-wise
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      double M[9];
#pragma unroll
      for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int r = 0; r < 3; ++r) {
          double s = 0;
#pragma unroll
          for (int m = 0; m < 3; ++m) s += PG_R(A, r, m) * S[a][m * 3 + c];
          M[r + 3 * c] = s;
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
  pg_store<STAGED, 36>(lds, J, J0, k, n);
}
