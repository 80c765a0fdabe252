// ---- stereo observations of the bundle-adjustment front end (included by block_solver.hip, inside namespace g2ohip) ------
//   EdgeProjectXYZ2UVU::computeError          g2o/types/sba/types_six_dof_expmap.h:181-200 (obs - stereocam_uvu_map(T.map(X)))
//   CameraParameters::stereocam_uvu_map       g2o/types/sba/types_six_dof_expmap.cpp:40, 77-82; baseline: types_six_dof_expmap.h:53-80
// Vertex 0 of an edge is the point, vertex 1 the pose (as EdgeProjectXYZ2UV).  cams [n][12] = R column-major | t, world -> camera,
// pts [n][3], meas [n][3] = (u_left, v_left, u_right).  With (x, y, z) = R X + t:
//   e  = meas - (f x / z + cx, f y / z + cy, f (x - b) / z + cx)
//   J0 (point, 3 x 3)  rows 0-1 as EdgeProjectXYZ2UV::linearizeOplus (types_six_dof_expmap.cpp:288-326),
//                      row 2 = -(1 / z) [f, 0, -f (x - b) / z] R
//   J1 (pose, 3 x 6, update (omega, upsilon) of VertexSE3Expmap::oplusImpl)  rows 0-1 as there,
//                      row 2 = f [(x - b) y / z^2, -(1 + x (x - b) / z^2), y / z, -1 / z, 0, (x - b) / z^2]
// The reference leaves linearizeOplus of this edge commented out (types_six_dof_expmap.h:199) and differentiates numerically
// (BaseBinaryEdge::linearizeOplus, central differences with step 1e-9): the device writes the exact derivative instead, as
// decided for EdgeSE2Prior.  Like the reference and ba_linearize_kernel there is no guard for z <= 0.
// Output in the layout of g2ohip_set_edge_data (J0 [n][3 x 3], J1 [n][3 x 6] column-major, err [n][3]), through either store
// form of pg_landmark.inc.  The robustified chi2 of the edges rides along as in ba_linearize_kernel: e' Omega e formed as
// chi2_kernel<3> forms it, one partial sum per workgroup (the reduction borrows the first kThreads doubles of the staging
// buffer BEFORE the first array passes through it: pg_store_rows opens with a barrier).  rk != nullptr: per-edge robust kernels
// (kind, delta) as chi2_kernel reads them.
template <bool STAGED>
__global__ void __launch_bounds__(kThreads) ba_stereo_linearize_kernel(int n, const double* __restrict__ cams, const double* __restrict__ pts,
                                                                     const int* __restrict__ cam_v, const int* __restrict__ pt_v,
                                                                     const double* __restrict__ meas, double f, double cx, double cy,
                                                                     double bl, double* __restrict__ J0, double* __restrict__ J1,
                                                                     double* __restrict__ err, int jac, const double* __restrict__ omega,
                                                                     int ident, int kind, double delta, const double* __restrict__ rk,
                                                                     double* __restrict__ chi_part) {
  __shared__ double lds[STAGED ? kThreads * 19 : kThreads];
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  const int kk = min(k, n - 1);   // (lanes past the end evaluate the last edge, store nothing and add nothing: every lane reaches the barriers)
  double T[12];
  load_vec<12>(cams + 12 * (size_t)cam_v[kk], T);
  const double* Xp = pts + 3 * (size_t)pt_v[kk];
  const double X[3] = {Xp[0], Xp[1], Xp[2]};
  const double* zm = meas + 3 * (size_t)kk;
  const double x = T[0] * X[0] + T[3] * X[1] + T[6] * X[2] + T[9];
  const double y = T[1] * X[0] + T[4] * X[1] + T[7] * X[2] + T[10];
  const double z = T[2] * X[0] + T[5] * X[1] + T[8] * X[2] + T[11];
  const double xr = x - bl;
  const double e[3] = {zm[0] - (x / z * f + cx), zm[1] - (y / z * f + cy), zm[2] - (xr / z * f + cx)};
  if (chi_part) {
    double rho = 0.0;
    if (k < n) {
      double e2 = 0.0;
      if (ident) {
        e2 = e[0] * e[0] + e[1] * e[1] + e[2] * e[2];
      } else {
        const double* O = omega + 9 * (size_t)kk;
#pragma unroll
        for (int i = 0; i < 3; ++i) e2 += e[i] * (O[i] * e[0] + O[i + 3] * e[1] + O[i + 6] * e[2]);
      }
      rho = rk ? robust_rho((int)rk[2 * (size_t)kk], rk[2 * (size_t)kk + 1], e2) : robust_rho(kind, delta, e2);
    }
    lds[threadIdx.x] = rho;
    __syncthreads();
    for (int o = kThreads / 2; o > 0; o >>= 1) {
      if ((int)threadIdx.x < o) lds[threadIdx.x] += lds[threadIdx.x + o];
      __syncthreads();
    }
    if (threadIdx.x == 0) chi_part[blockIdx.x] = lds[0];
  }
  pg_store<STAGED, 3>(lds, e, err, k, n);
  if (!jac) return;
  const double iz = 1.0 / z, z_2 = z * z;
  const double tmp[9] = {f, 0.0, -x / z * f, 0.0, f, -y / z * f, f, 0.0, -xr / z * f};   // row-major 3 x 3
  double A[9], B[18];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      double t = 0.0;
#pragma unroll
      for (int m = 0; m < 3; ++m) t += tmp[r * 3 + m] * T[m + 3 * c];
      A[r + 3 * c] = -iz * t;
    }
  B[0 + 3 * 0] = x * y / z_2 * f;          B[0 + 3 * 1] = -(1.0 + (x * x / z_2)) * f;  B[0 + 3 * 2] = y / z * f;
  B[0 + 3 * 3] = -1.0 / z * f;             B[0 + 3 * 4] = 0.0;                         B[0 + 3 * 5] = x / z_2 * f;
  B[1 + 3 * 0] = (1.0 + y * y / z_2) * f;  B[1 + 3 * 1] = -x * y / z_2 * f;            B[1 + 3 * 2] = -x / z * f;
  B[1 + 3 * 3] = 0.0;                      B[1 + 3 * 4] = -1.0 / z * f;                B[1 + 3 * 5] = y / z_2 * f;
  B[2 + 3 * 0] = xr * y / z_2 * f;         B[2 + 3 * 1] = -(1.0 + (x * xr / z_2)) * f; B[2 + 3 * 2] = y / z * f;
  B[2 + 3 * 3] = -1.0 / z * f;             B[2 + 3 * 4] = 0.0;                         B[2 + 3 * 5] = xr / z_2 * f;
  pg_store<STAGED, 9>(lds, A, J0, k, n);
  pg_store<STAGED, 18>(lds, B, J1, k, n);
}

// [n] 3 x 3 identity matrices (a stereo set whose information matrices were declared the identity: the generic assembly reads them)
__global__ void __launch_bounds__(kThreads) identity3_kernel(size_t n, double* __restrict__ om) {
  const size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (t < n * 9) om[t] = (t % 9) % 4 == 0 ? 1.0 : 0.0;
}
