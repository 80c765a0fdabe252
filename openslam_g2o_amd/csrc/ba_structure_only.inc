// ---- structure-only bundle adjustment of the BA front end (included by block_solver.hip, inside namespace g2ohip) ----------
//   StructureOnlySolver<3>::calc(points, num_iters, num_max_trials)   g2o/solvers/structure_only/structure_only_solver.h:72-194
// A Levenberg-Marquardt per landmark with every pose frozen.  With the poses frozen the points are independent: ONE launch runs
// all outer iterations and all damping trials of every free point of the bound projection set, with no host round trip, no
// global synchronisation and no linear solver.  Per point (control flow of :84-190):
//   mu = 0.01, nu = 2, chi2 = sum e' Omega e over the point's track (observations from fixed cameras included)
//   up to num_iters times:
//     H = sum w J' Omega J, b = -sum w J' Omega e  (J the point-side Jacobian, w = rho' of the set's robust kernel as the generic
//     assembly applies it: constructQuadraticForm, first order only)
//     stop (reason 1) when |b| < 0.001
//     trial = 0; repeat: factorise H + mu I; when positive, candidate X + delta, new_chi2 on the candidate;
//       accept iff chi2 - new_chi2 > 0 and new_chi2 is finite: chi2 = new_chi2, mu *= 1/3, nu = 2, next outer iteration
//       else mu *= nu, nu *= 2, ++trial; stop (reason 2) when trial >= num_max_trials
// mu and nu persist across the outer iterations of a point.  The acceptance test uses the RAW chi2 (e->chi2(), :92 and :158), not
// the robustified one.
// Deliberate deviation: an unpivoted 3 x 3 LDL' with the test "every pivot > 0" stands in for Eigen's pivoted
// LDLT::isPositive().  With mu > 0 the two differ only on non-finite input (a NaN pivot fails "> 0" and rejects the trial).
// Mapping: G consecutive lanes share one point of the estimate table (a point never straddles a wave: G divides 64) and walk the
// observation list of its landmark, G entries per pass (a list longer than one pass takes several).  Sums over the group go
// through the xor butterfly of group_sum, so every lane of a group holds bit-identical chi2, H, b and takes the same branch.
// Points of a wave finish at different times: the outer and the trial loop run while ANY lane of the wave needs them, and a
// lane that does not is predicated (its list range is empty); nobody leaves before the last cross-lane operation.
// MODE 0: EdgeProjectXYZ2UV through the landmark-major copies (cam_t = cam_lm, meas_t = meas_lm, omega_t = omega_lm, indexed by
//         list position) and ba_edge_linearize -- the errors of ba_linearize_kernel; 1: the same with edge classes;
//      2: EdgeProjectXYZ2UVU with the formulas of ba_stereo.inc through the edge id of the list entry (cam_t = cam_v, meas_t =
//         meas, omega_t = the set's information, indexed by edge; rk: per-edge robust kernels or null).
// The candidate lives in registers: the estimate stack of the front end (bak, has_backup) is not touched, and a point is
// written back once, at the end, when at least one step was accepted.
// trace[v] = (outer iterations started, accepted steps, rejected trials, stop reason: 0 ran num_iters, 1 |b| < 1e-3, 2
// num_max_trials reached, 3 not optimised -- fixed or empty track), chi[v] = (chi2 before, chi2 after).
template <int G, int MODE, bool LIN>
__device__ __forceinline__ void ba_so_track(int k0, int k1, int g, const double (&X)[3], const int* __restrict__ vent,
                                            const double* __restrict__ cams, const int* __restrict__ cam_t,
                                            const double* __restrict__ meas_t, const double* __restrict__ omega_t, int ident, double f,
                                            double cx, double cy, double bl, int kind, double delta, const double* __restrict__ rk,
                                            const double* __restrict__ ctab, double& chi, double (&H)[9], double (&b)[3]) {
  chi = 0.0;
  if (LIN) {
#pragma unroll
    for (int i = 0; i < 9; ++i) H[i] = 0.0;
    b[0] = b[1] = b[2] = 0.0;
  }
  for (int k = k0 + g; k < k1; k += G) {
    double T[12];
    if constexpr (MODE < 2) {
      load_vec<12>(cams + (size_t)ba_edge_class<MODE == 1>(cam_t[k], ctab, f, cx, cy, kind, delta) * 12, T);
      double z2[2], Op[4];
      load_vec<2>(meas_t + (size_t)k * 2, z2);
      if (ident) {
        Op[0] = Op[3] = 1.0;
        Op[1] = Op[2] = 0.0;
      } else {
        load_vec<4>(omega_t + (size_t)k * 4, Op);
      }
      BaEdgeLin L;
      ba_edge_linearize(T, X, z2, Op, f, cx, cy, kind, delta, LIN, L);
      chi += L.r[0] * (L.O[0] * L.r[0] + L.O[2] * L.r[1]) + L.r[1] * (L.O[1] * L.r[0] + L.O[3] * L.r[1]);
      if (LIN) {
        double OA[6];
        ba_lm_accumulate(L, H, b, OA);
      }
    } else {
      const size_t e = (size_t)(vent[k] >> 1);
      load_vec<12>(cams + (size_t)cam_t[e] * 12, T);
      const double* zm = meas_t + 3 * e;
      const double x = T[0] * X[0] + T[3] * X[1] + T[6] * X[2] + T[9];
      const double y = T[1] * X[0] + T[4] * X[1] + T[7] * X[2] + T[10];
      const double z = T[2] * X[0] + T[5] * X[1] + T[8] * X[2] + T[11];
      const double xr = x - bl;
      const double r[3] = {zm[0] - (x / z * f + cx), zm[1] - (y / z * f + cy), zm[2] - (xr / z * f + cx)};
      double O[9];
      if (ident) {
#pragma unroll
        for (int i = 0; i < 9; ++i) O[i] = (i % 4 == 0) ? 1.0 : 0.0;
      } else {
        load_vec<9>(omega_t + 9 * e, O);
      }
      double Or[3], e2 = 0.0;
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        Or[i] = O[i] * r[0] + O[i + 3] * r[1] + O[i + 6] * r[2];
        e2 += r[i] * Or[i];
      }
      chi += e2;
      if (LIN) {
        const double w = rk ? robust_weight((int)rk[2 * e], rk[2 * e + 1], e2) : robust_weight(kind, delta, e2);
        const double iz = 1.0 / z;
        const double tmp[9] = {f, 0.0, -x / z * f, 0.0, f, -y / z * f, f, 0.0, -xr / z * f};   // row-major 3 x 3
        double A[9];
#pragma unroll
        for (int rr = 0; rr < 3; ++rr)
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            double t = 0.0;
#pragma unroll
            for (int m = 0; m < 3; ++m) t += tmp[rr * 3 + m] * T[m + 3 * c];
            A[rr + 3 * c] = -iz * t;
          }
        // b -= A' (w O r), H += A' (w O) A, column by column (the order of assemble_vertex_kernel)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          b[c] -= w * (A[0 + 3 * c] * Or[0] + A[1 + 3 * c] * Or[1] + A[2 + 3 * c] * Or[2]);
          double OJ[3];
#pragma unroll
          for (int i = 0; i < 3; ++i) OJ[i] = w * (O[i] * A[0 + 3 * c] + O[i + 3] * A[1 + 3 * c] + O[i + 6] * A[2 + 3 * c]);
#pragma unroll
          for (int a = 0; a < 3; ++a) H[a + 3 * c] += A[0 + 3 * a] * OJ[0] + A[1 + 3 * a] * OJ[1] + A[2 + 3 * a] * OJ[2];
        }
      }
    }
  }
  if (G > 1) {
    chi = group_sum<G>(chi);
    if (LIN) {
#pragma unroll
      for (int i = 0; i < 9; ++i) H[i] = group_sum<G>(H[i]);
#pragma unroll
      for (int i = 0; i < 3; ++i) b[i] = group_sum<G>(b[i]);
    }
  }
}

template <int G, int MODE>
__global__ void __launch_bounds__(kThreads) ba_structure_only_kernel(
    int np, const int* __restrict__ hidx, const int* __restrict__ vptr, const int* __restrict__ vent, const double* __restrict__ cams,
    double* __restrict__ pts, const int* __restrict__ cam_t, const double* __restrict__ meas_t, const double* __restrict__ omega_t,
    int ident, double f, double cx, double cy, double bl, int kind, double delta, const double* __restrict__ rk,
    const double* __restrict__ ctab, int num_iters, int max_trials, int* __restrict__ trace, double* __restrict__ chi_out) {
  static_assert(G == 1 || G == 4 || G == 8, "lane groups of 1, 4 or 8");
  const int gt = blockIdx.x * blockDim.x + threadIdx.x;
  const int v = gt / G, g = gt % G;
  const bool in_table = v < np;
  const int h = in_table ? hidx[v] : -1;
  const int k0 = h >= 0 ? vptr[h] : 0, k1 = h >= 0 ? vptr[h + 1] : 0;
  double X[3] = {0.0, 0.0, 0.0};
  if (in_table) {
    X[0] = pts[(size_t)v * 3];
    X[1] = pts[(size_t)v * 3 + 1];
    X[2] = pts[(size_t)v * 3 + 2];
  }
  double H[9], b[3], chi2, mu = 0.01, nu = 2.0;
  ba_so_track<G, MODE, false>(k0, k1, g, X, vent, cams, cam_t, meas_t, omega_t, ident, f, cx, cy, bl, kind, delta, rk, ctab, chi2, H, b);
  const double chi2_before = chi2;
  int iters = 0, accepted = 0, rejected = 0, reason = k1 > k0 ? 0 : 3;
  bool done = k1 <= k0;   // fixed, empty track, or past the table (group-uniform, as everything below)
  for (int it = 0; it < num_iters; ++it) {
    if (!__any(!done)) break;   // (wave-uniform)
    double dummy;
    ba_so_track<G, MODE, true>(k0, done ? k0 : k1, g, X, vent, cams, cam_t, meas_t, omega_t, ident, f, cx, cy, bl, kind, delta, rk, ctab,
                            dummy, H, b);
    bool in_trial = !done;
    if (in_trial) {
      ++iters;
      if (sqrt(b[0] * b[0] + b[1] * b[1] + b[2] * b[2]) < 0.001) {
        done = true;
        reason = 1;
        in_trial = false;
      }
    }
    int trial = 0;
    while (__any(in_trial)) {   // (wave-uniform)
      // unpivoted LDL' of H + mu I (lower triangle), then the solve
      const double a00 = H[0] + mu, a10 = H[1], a20 = H[2], a11 = H[4] + mu, a21 = H[5], a22 = H[8] + mu;
      const double d0 = a00, l10 = a10 / d0, l20 = a20 / d0;
      const double d1 = a11 - l10 * a10, t21 = a21 - l20 * a10, l21 = t21 / d1;
      const double d2 = a22 - l20 * a20 - l21 * t21;
      const bool positive = d0 > 0.0 && d1 > 0.0 && d2 > 0.0;
      const double y0 = b[0], y1 = b[1] - l10 * y0, y2 = b[2] - l20 * y0 - l21 * y1;
      const double x2 = y2 / d2, x1 = y1 / d1 - l21 * x2, x0 = y0 / d0 - l10 * x1 - l20 * x2;
      const bool cand = in_trial && positive;
      const double Xn[3] = {cand ? X[0] + x0 : X[0], cand ? X[1] + x1 : X[1], cand ? X[2] + x2 : X[2]};
      double new_chi2, Hn[9], bn[3];
      ba_so_track<G, MODE, false>(k0, cand ? k1 : k0, g, Xn, vent, cams, cam_t, meas_t, omega_t, ident, f, cx, cy, bl, kind, delta, rk, ctab,
                               new_chi2, Hn, bn);
      if (in_trial) {
        if (positive && chi2 - new_chi2 > 0.0 && isfinite(new_chi2)) {
          X[0] = Xn[0]; X[1] = Xn[1]; X[2] = Xn[2];
          chi2 = new_chi2;
          mu *= 1.0 / 3.0;
          nu = 2.0;
          ++accepted;
          in_trial = false;
        } else {
          mu *= nu;
          nu *= 2.0;
          ++rejected;
          if (++trial >= max_trials) {
            done = true;
            reason = 2;
            in_trial = false;
          }
        }
      }
    }
  }
  if (!in_table || g != 0) return;
  if (accepted > 0) {
    const double Xo[3] = {X[0], X[1], X[2]};
    store_vec<3>(pts + (size_t)v * 3, Xo);
  }
  // (vector stores; v * 4 ints and v * 2 doubles are 16-byte aligned)
  *reinterpret_cast<int4*>(trace + (size_t)v * 4) = make_int4(iters, accepted, rejected, reason);
  const double co[2] = {chi2_before, chi2};
  store_vec<2>(chi_out + (size_t)v * 2, co);
}
