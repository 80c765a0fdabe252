// ---- landmark half of the pose-graph front end (included by block_solver.hip, inside namespace g2ohip) ------------------
//   EdgeSE2PointXY::computeError / linearizeOplus    g2o/types/slam2d/edge_se2_pointxy.h:44-49, edge_se2_pointxy.cpp:66-90
//   EdgeSE3PointXYZ::computeError / linearizeOplus   g2o/types/slam3d/edge_se3_pointxyz.cpp:95-131
//   CacheSE3Offset::updateImpl                       g2o/types/slam3d/parameter_se3_offset.cpp:44-50 (w2n, w2l)
//   EdgeSE3PointXYZDepth / EdgeSE3PointXYZDisparity  g2o/types/slam3d/edge_se3_pointxyz_{depth,disparity}.cpp (see the SE3 kernel)
//   VertexPointXY / VertexPointXYZ::oplusImpl        g2o/types/slam2d/vertex_point_xy.h:77-81, slam3d/vertex_pointxyz.h:48-51
// Vertex 0 of an edge is the pose, vertex 1 the landmark.  Output in the layout of g2ohip_set_edge_data: J0 [n][d x dim0],
// J1 [n][d x dim1] column-major, err [n][d].
//
// Store form.  A lane owns one edge and holds its 6 + 4 + 2 (SE2) or 18 + 9 + 3 (SE3) results in registers.  Written straight
// from there (STAGED = false) every store instruction of the wave touches 64 places 16 ... 144 bytes apart; STAGED = true
// passes each array through LDS (row per lane, padded to an odd number of doubles so that neither side has bank conflicts)
// and writes it out with consecutive lanes on consecutive doubles: one store instruction = 512 contiguous bytes.
template <int N>
__device__ __forceinline__ void pg_store_rows(double* lds, const double (&v)[N], double* __restrict__ out, size_t first_edge,
                                              int edges_here) {
  constexpr int NP = N | 1;
  const int tid = threadIdx.x;
  __syncthreads();   // (the previous array has left the buffer)
#pragma unroll
  for (int i = 0; i < N; ++i) lds[tid * NP + i] = v[i];
  __syncthreads();
  double* dst = out + first_edge * N;
  const int total = edges_here * N;
#pragma unroll
  for (int m = 0; m < N; ++m) {
    const int j = tid + m * kThreads;
    if (j < total) {
      const int e = j / N, c = j - e * N;
      dst[j] = lds[e * NP + c];
    }
  }
}
template <int N>
__device__ __forceinline__ void pg_store_direct(const double (&v)[N], double* __restrict__ out, size_t edge) {
  if constexpr (N % 2 == 0) {   // (rows of an even number of doubles are 16-byte aligned: hipMalloc'ed base)
    double2* dst = reinterpret_cast<double2*>(out + edge * N);
#pragma unroll
    for (int i = 0; i < N / 2; ++i) dst[i] = make_double2(v[2 * i], v[2 * i + 1]);
  } else {
    double* dst = out + edge * N;
#pragma unroll
    for (int i = 0; i < N; ++i) dst[i] = v[i];
  }
}
template <bool STAGED, int N>
__device__ __forceinline__ void pg_store(double* lds, const double (&v)[N], double* __restrict__ out, int k, int n) {
  if constexpr (STAGED) {
    const size_t first = (size_t)blockIdx.x * kThreads;
    pg_store_rows<N>(lds, v, out, first, min(kThreads, n - (int)first));
  } else {
    if (k < n) pg_store_direct<N>(v, out, (size_t)k);
  }
}

// e = R(theta)' (l - t) - z; the Jacobians are the analytic entries of EdgeSE2PointXY::linearizeOplus
template <bool STAGED>
__global__ void __launch_bounds__(kThreads) pg_se2_pointxy_linearize_kernel(int n, const double* __restrict__ poses,
                                                                          const double* __restrict__ points, const int* __restrict__ vp,
                                                                          const int* __restrict__ vl, const double* __restrict__ meas,
                                                                          double* __restrict__ J0, double* __restrict__ J1,
                                                                          double* __restrict__ err, int jac) {
  __shared__ double lds[STAGED ? kThreads * 7 : 1];
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  const int kk = min(k, n - 1);   // (lanes past the end evaluate the last edge and store nothing)
  const double* x = poses + 3 * (size_t)vp[kk];
  const double* l = points + 2 * (size_t)vl[kk];
  const double x1 = x[0], y1 = x[1], th1 = x[2], x2 = l[0], y2 = l[1];
  const double c = cos(th1), s = sin(th1);
  const double dx = x2 - x1, dy = y2 - y1;
  const double e[2] = {c * dx + s * dy - meas[2 * (size_t)kk], -s * dx + c * dy - meas[2 * (size_t)kk + 1]};
  pg_store<STAGED, 2>(lds, e, err, k, n);
  if (!jac) return;
  // column-major 2x3 and 2x2
  const double a[6] = {-c, s, -s, -c, c * y2 - c * y1 - s * x2 + s * x1, -s * y2 + s * y1 - c * x2 + c * x1};
  const double b[4] = {c, -s, s, c};
  pg_store<STAGED, 6>(lds, a, J0, k, n);
  pg_store<STAGED, 4>(lds, b, J1, k, n);
}

struct PgIso {
  double v[12];
};

struct PgKcam {
  double fx, fy, cx, cy;
};

// The three SE3 pose -> point edges, OBS = the edge type of the C ABI:
//   4  EdgeSE3PointXYZ over ParameterSE3Offset            g2o/types/slam3d/edge_se3_pointxyz.cpp:95-131
//   5  EdgeSE3PointXYZDepth, 6 EdgeSE3PointXYZDisparity over ParameterCamera / CacheCamera (one sensor offset + Kcam = (fx, fy,
//      cx, cy))   g2o/types/slam3d/edge_se3_pointxyz_depth.cpp:91-138, edge_se3_pointxyz_disparity.cpp:96-168,
//      parameter_camera.cpp:45-59, 93-96 (setKcam / setOffset, CacheCamera::updateImpl)
// Shared: w2n = (X offset)^-1, w2l = X^-1, q = w2n l the point in the sensor frame, J = [-I | 2 [w2l l]x | R(w2l)] (3 x 9) and
// the columns h of Roff' J.  What differs is the error taken from q and the output column made of h, split 6 | 3:
//   4     e = q - z, the column is h itself (kc is not read);
//   5, 6  p = K q with K = [fx 0 cx; 0 fy cy; 0 0 1], so p2 is the depth in the sensor frame; e = (p0 / p2, p1 / p2, p2) - z
//         (depth) or (p0 / p2, p1 / p2, 1 / p2) - z (disparity); with J' = K h, rows 0-1 of the column are
//         (J'[0:2] p2 - p[0:2] J'[2]) / p2^2, row 2 J'[2] (depth) or -J'[2] / p2^2 (disparity).
// The reference has no guard for a point on or behind the image plane (p2 <= 0), and neither has this kernel: such an edge
// gives the same infinities / NaNs here as there.
template <int OBS, bool STAGED>
__global__ void __launch_bounds__(kThreads) pg_se3_point_linearize_kernel(int n, const double* __restrict__ poses,
                                                                        const double* __restrict__ points, const int* __restrict__ vp,
                                                                        const int* __restrict__ vl, const double* __restrict__ meas,
                                                                        PgIso offset, PgKcam kc, double* __restrict__ J0,
                                                                        double* __restrict__ J1, double* __restrict__ err, int jac) {
  static_assert(OBS == 4 || OBS == 5 || OBS == 6, "EdgeSE3PointXYZ, ...Depth, ...Disparity");
  constexpr bool DISPARITY = OBS == 6;
  __shared__ double lds[STAGED ? kThreads * 19 : 1];
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  const int kk = min(k, n - 1);   // (lanes past the end evaluate the last edge and store nothing)
  const double* Xp = poses + 12 * (size_t)vp[kk];
  const double* lp = points + 3 * (size_t)vl[kk];
  double X[12], n2w[12], w2n[12], w2l[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) X[i] = Xp[i];
  const double l[3] = {lp[0], lp[1], lp[2]};
  pg_iso_mul(X, offset.v, n2w);
  pg_iso_inv(n2w, w2n);
  double e[3], p[3];   // (p: the camera edges only)
  if constexpr (OBS == 4) {
#pragma unroll
    for (int r = 0; r < 3; ++r)
      e[r] = PG_R(w2n, r, 0) * l[0] + PG_R(w2n, r, 1) * l[1] + PG_R(w2n, r, 2) * l[2] + w2n[9 + r] - meas[3 * (size_t)kk + r];
  } else {
    double q[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) q[r] = PG_R(w2n, r, 0) * l[0] + PG_R(w2n, r, 1) * l[1] + PG_R(w2n, r, 2) * l[2] + w2n[9 + r];
    p[0] = kc.fx * q[0] + kc.cx * q[2];
    p[1] = kc.fy * q[1] + kc.cy * q[2];
    p[2] = q[2];
    e[0] = p[0] / p[2] - meas[3 * (size_t)kk];
    e[1] = p[1] / p[2] - meas[3 * (size_t)kk + 1];
    e[2] = (DISPARITY ? 1.0 / p[2] : p[2]) - meas[3 * (size_t)kk + 2];
  }
  pg_store<STAGED, 3>(lds, e, err, k, n);
  if (!jac) return;
  pg_iso_inv(X, w2l);
  double Z[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) Z[r] = PG_R(w2l, r, 0) * l[0] + PG_R(w2l, r, 1) * l[1] + PG_R(w2l, r, 2) * l[2] + w2l[9 + r];
  // J (3 x 9, column-major) as EdgeSE3PointXYZ::linearizeOplus fills it
  const double J[27] = {-1, 0, 0, 0, -1, 0, 0, 0, -1,
                        0, 2 * Z[2], -2 * Z[1], -2 * Z[2], 0, 2 * Z[0], 2 * Z[1], -2 * Z[0], 0,
                        w2l[0], w2l[1], w2l[2], w2l[3], w2l[4], w2l[5], w2l[6], w2l[7], w2l[8]};
  double iz2 = 0.0;
  if constexpr (OBS != 4) iz2 = 1.0 / (p[2] * p[2]);
  double a[18], b[9];
#pragma unroll
  for (int cidx = 0; cidx < 9; ++cidx) {
    double h[3], g[3];   // column cidx of Roff' J (row r of inverseOffset().rotation() = column r of R(offset)), ... of the output
#pragma unroll
    for (int r = 0; r < 3; ++r)
      h[r] = PG_R(offset.v, 0, r) * J[3 * cidx] + PG_R(offset.v, 1, r) * J[3 * cidx + 1] + PG_R(offset.v, 2, r) * J[3 * cidx + 2];
    if constexpr (OBS == 4) {
#pragma unroll
      for (int r = 0; r < 3; ++r) g[r] = h[r];
    } else {
      const double jp[3] = {kc.fx * h[0] + kc.cx * h[2], kc.fy * h[1] + kc.cy * h[2], h[2]};   // ... of J' = K Roff' J
      g[0] = iz2 * (jp[0] * p[2] - p[0] * jp[2]);
      g[1] = iz2 * (jp[1] * p[2] - p[1] * jp[2]);
      g[2] = DISPARITY ? -iz2 * jp[2] : jp[2];
    }
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      if (cidx < 6) a[r + 3 * cidx] = g[r];
      else b[r + 3 * (cidx - 6)] = g[r];
    }
  }
  pg_store<STAGED, 18>(lds, a, J0, k, n);
  pg_store<STAGED, 9>(lds, b, J1, k, n);
}

// landmark estimate += its slice of x (one thread per scalar); hidx is the landmark's index in the whole system
// (>= num_poses) or -1 for a fixed landmark
__global__ void __launch_bounds__(kThreads) pg_points_update_kernel(size_t n_scalars, int l, double* __restrict__ points,
                                                                  const int* __restrict__ hidx, const double* __restrict__ x,
                                                                  size_t pose_scalars, int num_poses) {
  const size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (t >= n_scalars) return;
  const size_t v = t / l;
  const int c = (int)(t - v * l), h = hidx[v];
  if (h < 0) return;
  points[t] += x[pose_scalars + (size_t)(h - num_poses) * l + c];
}
