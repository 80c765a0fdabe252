// ---- pose-pose constraints of the bundle-adjustment front end (included by block_solver.hip behind ba_stereo.inc, inside
// namespace g2ohip): EdgeSE3Expmap between two VertexSE3Expmap, the second slot of BaFrontEnd (ba_set_pose_edges) --------------
//   EdgeSE3Expmap::computeError     g2o/types/sba/types_six_dof_expmap.h:111-130 (e = log(Tj^-1 C Ti), Ti = vertex 0, Tj = vertex 1)
//   EdgeSE3Expmap::linearizeOplus   g2o/types/sba/types_six_dof_expmap.cpp:271-286 (J0 = adj(Tj^-1 C), J1 = -adj(Ti^-1 C^-1))
//   SE3Quat::log                    g2o/types/slam3d/se3quat.h:178-215
//   SE3Quat::adj                    g2o/types/slam3d/se3quat.h:259-268 ([R 0; skew(t) R  R])
// cams [n][12] = R column-major | t, world -> camera: the camera table of ba_set_estimates.  meas [n][12] = the measurement C as
// an isometry in the same layout.  The estimates are rotation matrices already: the reference's quaternion -> matrix step has no
// counterpart here.  With E = Tj^-1 C Ti = (R, t), d = (tr R - 1) / 2 and deltaR = (R21 - R12, R02 - R20, R10 - R01):
//   d > 0.99999:  omega = deltaR / 2,                                   V^-1 = I - Omega / 2 + Omega^2 / 12
//   otherwise:    theta = acos(d), omega = theta / (2 sqrt(1 - d^2)) deltaR, V^-1 = I - Omega / 2 + (1 - theta / (2 tan(theta / 2))) / theta^2 Omega^2
//   e = (omega, V^-1 t)
// These are the reference's formulas, branch point included, and not a better-conditioned logarithm.  Like the reference there is
// NO guard near theta = pi (sqrt(1 - d^2) -> 0) and none for d outside [-1, 1] (acos of a rounded trace gives NaN): the caller
// keeps relative rotations away from pi, as the reference's users do.
// The Jacobians are the reference's adjoint form, exact at e = 0 only, and not the derivative of the logarithm.  Blocks of fixed
// vertices are written like the others (the reference writes them too; the assembly does not read them).  jac = 0 writes the
// errors only and leaves the Jacobians in place.
// Output in the layout of g2ohip_set_edge_data: J0, J1 [n][6 x 6] column-major (columns (omega, upsilon) of
// VertexSE3Expmap::oplusImpl), err [n][6] = (omega, upsilon).
// The arithmetic follows openslam_g2o_amd/se3expmap.py operation for operation and is compiled without contraction to fused
// multiply-adds, so that the fp64 evaluation there and the one here round alike up to acos / tan / sqrt.
// One lane per edge; lanes past the end evaluate the last edge and store nothing (every lane reaches the barriers).
//
// Store form.  A lane holds 6 + 36 + 36 results; its rows of the two J arrays lie 288 bytes apart, so stores straight from the
// registers would touch 64 separate places per instruction.  The errors leave through pg_store<true, 6> (pg_landmark.inc).  A J
// array leaves in two halves of 128 edges through LDS rows of 37 doubles (36 padded to odd): 128 x 37 x 8 = 37 888 bytes of LDS,
// what the other staged producers take (a whole block of both arrays would be 147 KB), and every store instruction of a wave
// writes 512 contiguous bytes.
//
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage):
//   ba_pose_edge_linearize_kernel   124 VGPRs, 0 AGPRs, 92 SGPRs, scratch 0 bytes / lane, no spills, LDS 37 888 bytes / block,
//                                   occupancy 4 waves / SIMD
//   identity6_kernel                9 VGPRs, scratch 0
template <int N>
__device__ __forceinline__ void ba_pose_store_halves(double* lds, const double (&v)[N], double* __restrict__ out, int n) {
  constexpr int H = kThreads / 2, NP = N | 1;
  const int tid = threadIdx.x;
  const int first = blockIdx.x * kThreads;   // (< n: fits an int)
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    __syncthreads();   // (the previous pass has left the buffer)
    if (tid / H == h) {
#pragma unroll
      for (int i = 0; i < N; ++i) lds[(tid - h * H) * NP + i] = v[i];
    }
    __syncthreads();
    const int total = min(H, n - first - h * H) * N;   // (<= 0: this half lies past the last edge)
    double* dst = out + ((size_t)first + h * H) * N;
#pragma unroll
    for (int m = 0; m < N / 2; ++m) {   // H * N = (kThreads / 2) * N values, kThreads per round
      const int j = tid + m * kThreads;
      if (j < total) {
        const int e = j / N, c = j - e * N;
        dst[j] = lds[e * NP + c];
      }
    }
  }
}

// adj of the isometry (R, t), times sign: [R 0; skew(t) R  R], column-major 6 x 6
__device__ __forceinline__ void ba_pose_adj(const double* R, const double* t, double sign, double (&J)[36]) {
#pragma clang fp contract(off)
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const double r0 = PG_R(R, 0, c), r1 = PG_R(R, 1, c), r2 = PG_R(R, 2, c);
    const double s0 = t[1] * r2 - t[2] * r1, s1 = t[2] * r0 - t[0] * r2, s2 = t[0] * r1 - t[1] * r0;   // t x R(:, c)
    J[0 + 6 * c] = sign * r0; J[1 + 6 * c] = sign * r1; J[2 + 6 * c] = sign * r2;
    J[3 + 6 * c] = sign * s0; J[4 + 6 * c] = sign * s1; J[5 + 6 * c] = sign * s2;
    J[0 + 6 * (3 + c)] = 0.0; J[1 + 6 * (3 + c)] = 0.0; J[2 + 6 * (3 + c)] = 0.0;
    J[3 + 6 * (3 + c)] = sign * r0; J[4 + 6 * (3 + c)] = sign * r1; J[5 + 6 * (3 + c)] = sign * r2;
  }
}

// C = A' B (3 x 3, column-major) and C = A B
__device__ __forceinline__ void ba_pose_atb(const double* A, const double* B, double* C) {
#pragma clang fp contract(off)
#pragma unroll
  for (int j = 0; j < 3; ++j)
#pragma unroll
    for (int i = 0; i < 3; ++i) PG_R(C, i, j) = (PG_R(A, 0, i) * PG_R(B, 0, j) + PG_R(A, 1, i) * PG_R(B, 1, j)) + PG_R(A, 2, i) * PG_R(B, 2, j);
}
__device__ __forceinline__ void ba_pose_ab(const double* A, const double* B, double* C) {
#pragma clang fp contract(off)
#pragma unroll
  for (int j = 0; j < 3; ++j)
#pragma unroll
    for (int i = 0; i < 3; ++i) PG_R(C, i, j) = (PG_R(A, i, 0) * PG_R(B, 0, j) + PG_R(A, i, 1) * PG_R(B, 1, j)) + PG_R(A, i, 2) * PG_R(B, 2, j);
}
// y = A' x and y = A x
__device__ __forceinline__ void ba_pose_atx(const double* A, const double* x, double* y) {
#pragma clang fp contract(off)
#pragma unroll
  for (int i = 0; i < 3; ++i) y[i] = (PG_R(A, 0, i) * x[0] + PG_R(A, 1, i) * x[1]) + PG_R(A, 2, i) * x[2];
}
__device__ __forceinline__ void ba_pose_ax(const double* A, const double* x, double* y) {
#pragma clang fp contract(off)
#pragma unroll
  for (int i = 0; i < 3; ++i) y[i] = (PG_R(A, i, 0) * x[0] + PG_R(A, i, 1) * x[1]) + PG_R(A, i, 2) * x[2];
}

__global__ void __launch_bounds__(kThreads) ba_pose_edge_linearize_kernel(int n, const double* __restrict__ cams, const int* __restrict__ vi,
                                                                        const int* __restrict__ vj, const double* __restrict__ meas,
                                                                        double* __restrict__ J0, double* __restrict__ J1,
                                                                        double* __restrict__ err, int jac) {
#pragma clang fp contract(off)
  __shared__ double lds[(kThreads / 2) * 37];
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  const int kk = min(k, n - 1);   // (lanes past the end evaluate the last edge and store nothing)
  double Ti[12], Tj[12], C[12];
  load_vec<12>(cams + 12 * (size_t)vi[kk], Ti);
  load_vec<12>(cams + 12 * (size_t)vj[kk], Tj);
  load_vec<12>(meas + 12 * (size_t)kk, C);
  // A = Tj^-1 C, E = A Ti
  double RA[9], tA[3], RE[9], tE[3], w[3];
  ba_pose_atb(Tj, C, RA);
  ba_pose_atx(Tj, Tj + 9, w);
  ba_pose_atx(Tj, C + 9, tA);
#pragma unroll
  for (int i = 0; i < 3; ++i) tA[i] = tA[i] + (-w[i]);
  ba_pose_ab(RA, Ti, RE);
  ba_pose_ax(RA, Ti + 9, tE);
#pragma unroll
  for (int i = 0; i < 3; ++i) tE[i] = tE[i] + tA[i];
  // SE3Quat::log
  const double d = 0.5 * (((PG_R(RE, 0, 0) + PG_R(RE, 1, 1)) + PG_R(RE, 2, 2)) - 1.0);
  const double dR[3] = {PG_R(RE, 2, 1) - PG_R(RE, 1, 2), PG_R(RE, 0, 2) - PG_R(RE, 2, 0), PG_R(RE, 1, 0) - PG_R(RE, 0, 1)};
  double sc, cf;
  if (d > 0.99999) {
    sc = 0.5;
    cf = 1.0 / 12.0;
  } else {
    const double theta = acos(d);
    sc = theta / (2.0 * sqrt(1.0 - d * d));
    cf = (1.0 - theta / (2.0 * tan(theta / 2.0))) / (theta * theta);
  }
  const double ox = sc * dR[0], oy = sc * dR[1], oz = sc * dR[2];
  const double xx = ox * ox, yy = oy * oy, zz = oz * oz, xy = ox * oy, xz = ox * oz, yz = oy * oz;
  // V^-1 = I - Omega / 2 + cf Omega^2, Omega = skew(omega), Omega^2 = omega omega' - |omega|^2 I
  const double V00 = 1.0 + cf * (-(yy + zz)), V01 = 0.5 * oz + cf * xy, V02 = -0.5 * oy + cf * xz;
  const double V10 = -0.5 * oz + cf * xy, V11 = 1.0 + cf * (-(xx + zz)), V12 = 0.5 * ox + cf * yz;
  const double V20 = 0.5 * oy + cf * xz, V21 = -0.5 * ox + cf * yz, V22 = 1.0 + cf * (-(xx + yy));
  const double e[6] = {ox, oy, oz, (V00 * tE[0] + V01 * tE[1]) + V02 * tE[2], (V10 * tE[0] + V11 * tE[1]) + V12 * tE[2],
                       (V20 * tE[0] + V21 * tE[1]) + V22 * tE[2]};
  pg_store<true, 6>(lds, e, err, k, n);
  if (!jac) return;   // (uniform over the grid)
  double J[36];
  ba_pose_adj(RA, tA, 1.0, J);
  ba_pose_store_halves<36>(lds, J, J0, n);
  // B = Ti^-1 C^-1: RB = Ri' Rc', tB = Ri' (-(Rc' tc)) + (-(Ri' ti))
  double Rct[9], RB[9], tc[3], tB[3];
#pragma unroll
  for (int j = 0; j < 3; ++j)
#pragma unroll
    for (int i = 0; i < 3; ++i) PG_R(Rct, i, j) = PG_R(C, j, i);
  ba_pose_atb(Ti, Rct, RB);
  ba_pose_atx(C, C + 9, tc);
#pragma unroll
  for (int i = 0; i < 3; ++i) tc[i] = -tc[i];
  ba_pose_atx(Ti, tc, tB);
  ba_pose_atx(Ti, Ti + 9, w);
#pragma unroll
  for (int i = 0; i < 3; ++i) tB[i] = tB[i] + (-w[i]);
  ba_pose_adj(RB, tB, -1.0, J);
  ba_pose_store_halves<36>(lds, J, J1, n);
}

// [n] 6 x 6 identity matrices (a pose set whose information matrices were declared the identity: the generic assembly reads them)
__global__ void __launch_bounds__(kThreads) identity6_kernel(size_t n, double* __restrict__ om) {
  const size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (t < n * 36) om[t] = (t % 36) % 7 == 0 ? 1.0 : 0.0;
}
