// Factorisation of SMALL frontal matrices on the matrix cores: one four-wave workgroup per task (chain of fronts).
// Included by sparse_cholesky.hip inside its anonymous namespace.
//
// Replaces, for the fronts of the reduced bundle-adjustment system (<= 24 pivot columns, <= 48 boundary rows), the
// LDS-resident front_factor_kernel: there every operand of the trailing update travels LDS -> register once per
// pivot step (a 3 x 3 register tile costs as many LDS operations as FMAs; six fronts per CU saturate the CU's
// single LDS pipe).  Here the front is in LDS only while it is ASSEMBLED (scatter target of the original blocks
// and of the children's update matrices); the numeric work runs on a front held in registers:
//   * the symmetric front F (plus the right-hand side of the fused forward sweep as one more row / column, index m)
//     is kept as UPPER 16 x 16 tiles in the accumulator layout of v_mfma_f64_16x16x4_f64: register v of lane l of tile
//     (ti, tj) holds F(16 ti + l / 16 + 4 v, 16 tj + l % 16); the 15 tiles are dealt to the four waves, wave w holding
//     the two tiles of the pivot rows of column tile w + 1;
//   * ROW 4 kb + l / 16 of a pivot-row tile (0 / 1, t) -- one register -- is, by symmetry, the panel
//     F(16 t + l % 16, 4 kb + l / 16) in the OPERAND layout of the instruction;
//   * phase 1 (rounds 1-5: six right-looking steps of four columns with two barriers each, the 4 x 4 pivot block
//     factorised redundantly by every lane; round 6): the pivot block F11 = L11 L11' (csparse_helper.cpp:109-140
//     restricted to the block) by COLUMN BLOCKS dealt to the waves, lane = row, the columns in registers, the pivot
//     column over v_readlane, the rows of W = L11^-1 in lanes 32-55 through the same instructions; a wave factorises
//     its block, publishes it in LDS, a barrier, the waves behind apply it (multipliers as LDS broadcast reads);
//   * phase 2: L' = W [F11 F12 b] -- per wave one column tile, up to ten instructions back to back with the tile
//     registers as the B operand and W (from LDS) as the A operand; the result is again in operand layout;
//   * phase 3: F22 -= L21 L21' -- up to six instructions per tile with those registers as the A (sign flipped) and B
//     operands; five barriers per front in all.
// The right-hand side column comes out as y = L11^-1 b1 (cs_lsolve restricted to the front) in the pivot rows and
// as w = b2 - L21 y in the boundary rows.  The L panel, the reciprocal diagonal and y are written to HBM from LDS
// BEHIND the hand-off to the parent: nothing in the launch reads them.
// A wavefront issues one instruction per ~4 cycles whatever its kind (tools/probe/issue_latency.hip), so the assembly
// is written to keep the instruction count low: the 36 elements of a block are handled by 36 fixed lanes, so that
// everything that depends on the block only is wave-uniform; LDS offsets of front elements are the sum of a row part
// and a column part read from two small tables; the blocks of a front are dealt to the four waves.
// Results (L panel, update matrix, update vector) leave in the formats of front_factor_kernel, so the triangular
// sweeps, the multi-GPU exchange and parents handled by the other kernel variants are unchanged.
//
// MFMA layout (probed on gfx950, tools/probe/mfma_f64_layout.hip): D[i][j] = sum_k A[i][k] B[j][k] with A[i][k] in
// lane i + 16 k, B[j][k] in lane j + 16 k, D[lane / 16 + 4 v][lane % 16] in register v.
//
// LDS per workgroup: TB (the upper tiles, tile (ti, tj) at (tj (tj + 1) / 2 + ti) * 256, row-major inside: the element
// of accumulator register v sits at lane + 64 v; once every wave has its tiles in registers the same memory holds the
// published pivot block -- per column 24 rows of L and the row of W -- and L' by column tile) | sink (64 slots for lanes
// without an element) | Rb, Lb (unused since round 6) | ET (records of the original blocks) | RP, CP (row / column part
// of an element's offset in TB) | RPR, CPR (child boundary row -> row / column part of its destination).

__device__ __forceinline__ double wv_neg(double v) { return __hiloint2double(__double2hiint(v) ^ (int)0x80000000u, __double2loint(v)); }
__device__ __forceinline__ void wv_lds_add(double* p, double v) {   // ds_add_f64, no return
  (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
// the lane id behind an opaque copy: what is derived from it is recomputed where it is used instead of being
// hoisted out of the per-front loop (lane-only addresses and predicates would otherwise stay live across the kernel)
__device__ __forceinline__ int wv_opaque(int x) {
  asm volatile("" : "+v"(x));
  return x;
}

typedef double wv_d4 __attribute__((ext_vector_type(4)));

// what the kernel needs of CholPlanDev (the full plan is ~45 pointers: kept whole in SGPRs it forces spills into the hot loops)
struct WvPlan {
  const int2* slots;
  const FrontRec* rec;
  const ChildDesc* cdesc;
  const int *crel, *cmap, *asm_q, *asm_pos, *asm_r8, *vslots;
  const double *vbase, *vparts, *vlam;
  double *L, *U, *w;
  int *status, *ready;
  long long *dbg, *tl;
  int vsplit, dep_spin_limit;
};
inline WvPlan wv_plan(const CholPlanDev& P) {
  WvPlan q;
  q.slots = P.slots; q.rec = P.rec; q.cdesc = P.cdesc; q.crel = P.crel; q.cmap = P.cmap; q.asm_q = P.asm_q; q.asm_pos = P.asm_pos;
  q.asm_r8 = P.asm_r8; q.vslots = P.vslots; q.vbase = P.vbase; q.vparts = P.vparts; q.vlam = P.vlam; q.L = P.L; q.U = P.U; q.w = P.w;
  q.status = P.status; q.ready = P.ready; q.dbg = P.dbg; q.tl = P.tl; q.vsplit = P.vsplit; q.dep_spin_limit = P.dep_spin_limit;
  return q;
}

#ifndef G2OHIP_WV_UC
#define G2OHIP_WV_UC 4
#endif
constexpr int kWvWaves = 4;
constexpr int kWvOwn = (kWvTiles + kWvWaves - 1) / kWvWaves;   // tiles per wave

template <int BS, bool VIRT>
__global__ void __launch_bounds__(64 * kWvWaves, 4) wave_front_kernel(WvPlan P, int slot0, const double* __restrict__ A,
                                                                      const double* __restrict__ bperm, double* __restrict__ yout,
                                                                      int dep) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  constexpr int BB = BS * BS;
  constexpr int T = kWvT, NT = kWvTiles, MX = 16 * T, NW = kWvWaves, OWN = kWvOwn;
  const int tid = threadIdx.x;
  const int lane0 = tid & 63;
  // the ROLE of a wave (which tiles, which pivot columns) is rotated by the workgroup: the four workgroups of a CU then run the same
  // phase of the pivot block on four different SIMDs instead of one (tree levels 0.180 -> 0.177 ms)
  const int w = __builtin_amdgcn_readfirstlane(((tid >> 6) + (int)blockIdx.x) & (kWvWaves - 1));
  double* TB = smem;
  double* Rb = TB + NT * 256 + 64;
  double* Lb = Rb + T * 64;
  int4* ET = reinterpret_cast<int4*>(Lb + T * 64);   // records of the front's original blocks (two int4 per entry, <= 64 entries)
  int* RP = reinterpret_cast<int*>(ET + 2 * 64);
  int* CP = RP + MX;
  int* RPR = CP + MX;   // child boundary row -> row / column part of its destination in this front
  int* CPR = RPR + 64;
  const bool fwd = bperm != nullptr;
  const int2 slot = P.slots[slot0 + blockIdx.x];
  const int f_first = __builtin_amdgcn_readfirstlane(slot.x), t1 = __builtin_amdgcn_readfirstlane(slot.y);
#ifdef G2OHIP_CHOL_STAMPS
  int nstamp = 0;
#ifndef WSTAMP_BLOCK
#define WSTAMP_BLOCK 0
#endif
#define WSTAMP() do { if (P.dbg && blockIdx.x == WSTAMP_BLOCK && tid == 0 && nstamp < 58) P.dbg[4 + nstamp++] = wall_clock64(); } while (0)
  if (P.tl && tid == 0) P.tl[6 * (slot0 + blockIdx.x)] = wall_clock64();
#else
#define WSTAMP() do {} while (0)
#endif
  WSTAMP();
  // offset of front element (a, b), a <= b, in TB = RP[a] + CP[b]
  for (int i = tid; i < MX; i += 64 * NW) {
    const int t = i >> 4;
    RP[i] = (t << 8) + ((i & 15) << 4);
    CP[i] = ((t * (t + 1)) << 7) + (i & 15);
  }
  // this wave's tiles (oti[k], otj[k]); (T, T): none.  Wave w holds the two tiles of column tile w + 1 that contain pivot rows
  // (k = 0, 1: the B operands of its share of phase 2) and up to two of the remaining tiles.
  static_assert(T == 5 && NW == 4 && OWN == 4, "tile ownership table below");
  int oti[OWN], otj[OWN];
  oti[0] = 0;
  otj[0] = w + 1;
  oti[1] = 1;
  otj[1] = w + 1;
  oti[2] = w == 0 ? 0 : (w == 1 ? 3 : 2);
  otj[2] = w == 0 ? 0 : (w == 3 ? 2 : 4);
  oti[3] = w == 0 ? 4 : (w == 1 ? T : (w == 2 ? 3 : 2));
  otj[3] = w == 0 ? 4 : (w == 1 ? T : 3);
  wv_d4 S[OWN];             // this wave's tiles of the front; after the factorisation: update matrix and update vector
  int prev_npiv = 0, prev_m = 0;   // prev_m > 0: S holds the results of the previous chain front
#pragma unroll
  for (int k = 0; k < OWN; ++k) S[k] = wv_d4{0.0, 0.0, 0.0, 0.0};

  for (int ti_ = 0; ti_ < t1; ++ti_) {
    const int f = f_first + ti_;
    int lane = wv_opaque(lane0);
    const FrontRec rec = load_front_rec(P.rec + f);
    const int ns = rec.ns, nbd = rec.nb;
    const int npiv = ns * BS, nbr = nbd * BS, m = npiv + nbr;
    const int mext = m + 1;               // rows incl. the right-hand side row
    const int na = rec.asm_cnt;
    const int nch = rec.child_cnt;
    const bool carried = prev_m > 0;
    // lanes 0 .. BB-1 <-> element (bi, bj) of a block (extend-add of the children)
    const bool inblk = lane < BB;
    const int bj = lane / BS, bi = lane - bj * BS;
    // table of the original blocks: thread e fetches the record of entry e -> ET (LDS), read back per ELEMENT below
    int4 t_a = make_int4(-1, 0, 0, 0), t_b = make_int4(0, 0, 0, 0);
    if (tid < na) {
      const int e = rec.asm_off + tid;
      if constexpr (VIRT) {
        t_a = reinterpret_cast<const int4*>(P.asm_r8)[2 * (size_t)e];       // base, pos, count, slot 0
        t_b = reinterpret_cast<const int4*>(P.asm_r8)[2 * (size_t)e + 1];   // slot 1, slot 2, first list index, -
      } else {
        t_a.x = P.asm_q[e];
        t_a.y = P.asm_pos[e];
      }
    }
    if (carried && tid < 64) {   // (all 64 entries defined: the lookups below are clamped instead of predicated)
      const int i = min(tid, prev_m - prev_npiv - 1);
      const int pr = P.crel[rec.crel_off + rec.ch[0].crel_start + i / BS] * BS + i % BS, t = pr >> 4;
      RPR[tid] = (t << 8) + ((pr & 15) << 4);
      CPR[tid] = ((t * (t + 1)) << 7) + (pr & 15);
    }
    // ---- zero the assembly buffer
    for (int i = tid; i < NT * 256; i += 64 * NW) TB[i] = 0.0;
    if (tid < na) {
      ET[2 * tid] = t_a;
      if constexpr (VIRT) ET[2 * tid + 1] = t_b;
    }
    __syncthreads();
    WSTAMP();   // rec + zero
    // ---- original entries (lower blocks of pivot columns): element (r, c), r >= c, is stored as (c, r).
    // The na * BB elements of the front's blocks are dealt to the 256 threads and every load of a thread is requested
    // before the first one is used: ONE memory round trip for the usual front (a block per pass and wave took three to
    // five: the time of this kernel is its dependent memory round trips, not its instruction count).
    {
      constexpr int UE = VIRT ? 4 : 6;   // (six with the partial blocks spill)
      const int nel = na * BB;
      constexpr int HB = BS / 2;
      const bool vsplit = VIRT && P.vsplit != 0;
      auto pe_of = [&](int rr, int cc) {   // partial layout [row part][column][row in part]
        const int rp = (vsplit && rr >= HB) ? 1 : 0, nrp = vsplit ? HB : BS;
        return rp * (nrp * BS) + (rr - rp * nrp) + nrp * cc;
      };
      double lam0 = 0.0;
      if constexpr (VIRT) lam0 = P.vlam[0];
      for (int base = 0; base < nel; base += 64 * NW * UE) {
        double a[UE], p0[UE], p1[UE], p2[UE];
        int ee[UE];
#pragma unroll
        for (int u = 0; u < UE; ++u) {
          const int idx = min(base + u * 64 * NW + tid, nel - 1);
          const int e = idx / BB, el = idx - e * BB;
          const int ej = el / BS, ei = el - ej * BS;
          ee[u] = e | (el << 8);
          const int4 ra = ET[2 * e];
          const int q = ra.x;
          const bool tr = (ra.y >> 30) & 1;
          const int off = tr ? ej + BS * ei : ei + BS * ej;
          if constexpr (VIRT) {
            // block = base (+ lambda on the diagonal of diagonal blocks) minus its partial blocks in list order: the
            // Schur complement's reduction folded into this load (same operations, same order as schur_reduce_kernel);
            // absent partials point at an all-zero block
            const int4 rb = ET[2 * e + 1];
            const int pe = tr ? pe_of(ej, ei) : pe_of(ei, ej);
            a[u] = 0.0;
            if (q >= 0) a[u] = P.vbase[(size_t)q * BB + off];
            p0[u] = P.vparts[(size_t)ra.w * BB + pe];
            p1[u] = P.vparts[(size_t)rb.x * BB + pe];
            p2[u] = P.vparts[(size_t)rb.y * BB + pe];
          } else {
            a[u] = A[(size_t)q * BB + off];
          }
        }
#pragma unroll
        for (int u = 0; u < UE; ++u) {
          if (base + u * 64 * NW + tid < nel) {
            const int e = ee[u] & 0xff, el = ee[u] >> 8;
            const int ej = el / BS, ei = el - ej * BS;
            const int4 ra = ET[2 * e];
            const int pos = ra.y;
            const int lr = pos & 0x7fff, lc = (pos >> 15) & 0x7fff;
            double v = a[u];
            if constexpr (VIRT) {
              if (pos < 0 && ei == ej) v += lam0;   // (bit 31: diagonal block)
              v -= p0[u];
              v -= p1[u];
              const int nn = ra.z;
              if (nn > 2) {
                v -= p2[u];
                if (nn > 3) {
                  const bool tr = (pos >> 30) & 1;
                  const int pe = tr ? pe_of(ej, ei) : pe_of(ei, ej);
                  const int k0 = ET[2 * e + 1].z;
                  for (int k = k0 + 3; k < k0 + nn; ++k) v -= P.vparts[(size_t)P.vslots[k] * BB + pe];
                }
              }
            }
            if (lr != lc || ei >= ej) TB[RP[lc * BS + ej] + CP[lr * BS + ei]] = v;
          }
        }
      }
    }
    // right-hand side: column m of the front (pivot part from the permuted right-hand side, boundary part from the children)
    if (fwd && tid < npiv) TB[RP[tid] + CP[m]] = bperm[(size_t)rec.c0 * BS + tid];
    WSTAMP();   // originals + rhs
    // ---- dependency-driven launch: the children of this front run in THIS launch; everything above did not depend
    // on them
    const int dep_wait = dep ? ((rec.pad[1] >> 24) & 0x7f) : 0;
    if (dep_wait > 0 && tid == 0) {
      int spins = 0;
      while (dep_poll(P.ready + f) < dep_wait) {
        __builtin_amdgcn_s_sleep(2);
        if (++spins > P.dep_spin_limit || ((spins & 255) == 0 && __hip_atomic_load(P.status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 2)) {
          __hip_atomic_store(P.status, 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          break;
        }
      }
      __hip_atomic_store(P.ready + f, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // ready for the next factorisation
    }
    __syncthreads();   // (originals of all waves are in TB; the children have signalled)
    WSTAMP();   // dep wait
#ifdef G2OHIP_CHOL_STAMPS
    if (P.tl && tid == 0) {   // timeline record: when the children were there, this front, its parent (tools/tree_handoff.py)
      P.tl[6 * (slot0 + blockIdx.x) + 2] = wall_clock64();
      P.tl[6 * (slot0 + blockIdx.x) + 3] = f;
      P.tl[6 * (slot0 + blockIdx.x) + 4] = rec.pad[1] & 0x00ffffff;
    }
#endif
    // ---- extend-add of the children: update matrices and update vectors
    lane = wv_opaque(lane0);
    if (carried) {
      // the only child arrived in the tile registers: boundary rows of the previous front -> rows of this front (RPR /
      // CPR: row / column part of the destination).  The destinations of one child are distinct and they hold the
      // original entry or zero: ds_add_f64 gives original + child whatever the waves' relative timing.
      const int cpm = CP[m];
#pragma unroll
      for (int k = 0; k < OWN; ++k) {
        const int c = 16 * otj[k] + (lane & 15);
        const bool cin = c >= prev_npiv && c < prev_m, cw = fwd && c == prev_m;
        const int co = cin ? CPR[min(max(c - prev_npiv, 0), 63)] : cpm;
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const int r = 16 * oti[k] + (lane >> 4) + 4 * v;
          const bool rin = r >= prev_npiv && r < prev_m;
          const int ro = RPR[min(max(r - prev_npiv, 0), 63)];
          if (rin && (cin || cw) && r <= c) wv_lds_add(TB + ro + co, S[k][v]);
        }
      }
    }
    if (carried && nch > 1) __syncthreads();   // (a chain front has one child; kept safe: the adds below are atomic, the ones above are not)
    // children from HBM: the blocks of an update matrix are dealt to the waves; every block of up to two children is
    // requested before the first wait (one memory round trip; at the top of the tree this load is the critical path).
    for (int ch = carried ? 1 : 0; ch < nch; ch += 2) {
      ChildDesc cd[2];
      int nblk[2], nblk_w[2], e_map[2];
      const bool two = ch + 1 < nch;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int c = min(ch + h, nch - 1);
        if (c == 0) cd[h] = rec.ch[0]; else if (c == 1) cd[h] = rec.ch[1]; else cd[h] = load_child_desc(P.cdesc + rec.child_off + c);
        nblk[h] = cd[h].nbc * (cd[h].nbc + 1) / 2;
        nblk_w[h] = (h == 0 || two) ? (nblk[h] - w + NW - 1) / NW : 0;   // blocks of this wave: b = w + NW k
        e_map[h] = 0;
        if (lane < nblk_w[h]) e_map[h] = P.cmap[rec.cmap_off + cd[h].cmap_start + w + NW * lane];
      }
      // update vectors: child ch by wave 0, child ch + 1 by wave 1 -- requested with the first batch of blocks (one round trip)
      const bool vec_wave = fwd && (w == 0 || (w == 1 && two));
      const ChildDesc cv = w == 0 ? cd[0] : cd[1];
      const bool vec_lane = vec_wave && lane < cv.nbc * BS;
      double wvv = 0.0;
      int wrow = 0;
#ifdef G2OHIP_WV_NOHOIST
      if (false) {
#else
      if (vec_lane) {
#endif
        wvv = ld_coh(P.w + cv.w_off + lane);
        wrow = P.crel[rec.crel_off + cv.crel_start + lane / BS] * BS + lane % BS;
      }
      constexpr int UC = G2OHIP_WV_UC;   // blocks in flight per child and wave (round 5, -DG2OHIP_WV_UC: five = two batches instead of three is equal within noise, 0.202-0.216 vs 0.207-0.211 ms; nine = one batch spills 96 B/lane at the 128-register limit, 0.305 ms)
      const int nb_wg = max((nblk[0] + NW - 1) / NW, two ? (nblk[1] + NW - 1) / NW : 0);   // (loop bounds are per workgroup: barriers inside)
      for (int b0 = 0; b0 < nb_wg; b0 += UC) {
        double u[2][UC];
        if (inblk) {
#pragma unroll
          for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int k = 0; k < UC; ++k) u[h][k] = ld_coh(P.U + cd[h].U_off + (size_t)min(w + NW * (b0 + k), nblk[h] - 1) * BB + lane);
        }
        // one child at a time (barrier in between): every element then receives its contributions in child order,
        // whatever the waves' relative timing -- the factorisation stays bit-repeatable
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          if (h == 1 || b0 > 0) __syncthreads();
#ifdef G2OHIP_WV_NOHOIST
          if (b0 == 0 && vec_lane && w == h) {
            wvv = ld_coh(P.w + cv.w_off + lane);
            wrow = P.crel[rec.crel_off + cv.crel_start + lane / BS] * BS + lane % BS;
          }
#endif
          if (b0 == 0 && vec_lane && w == h) wv_lds_add(TB + RP[wrow] + CP[m], wvv);
          if (inblk) {
#pragma unroll
            for (int k = 0; k < UC; ++k) {
              if (b0 + k < nblk_w[h]) {   // (wave-uniform)
                const int d = __builtin_amdgcn_readlane(e_map[h], b0 + k);
                const int pi = d & 0xffff, pj = d >> 16;
                if (pi != pj || bi >= bj) wv_lds_add(TB + RP[pj * BS + bj] + CP[pi * BS + bi], u[h][k]);
              }
            }
          }
        }
      }
      if (ch + 2 < nch) __syncthreads();
    }
    __syncthreads();
    // ---- factorisation in three phases (round 6; replaces six 4-column right-looking steps with two barriers each)
    //   1. the pivot block F11 = L11 L11' (<= 24 columns) by COLUMN BLOCKS dealt to the waves (six columns each; seven for 7 x 7
    //      blocks): lane i = row i, a wave's columns in registers, the pivot column through v_readlane;
    //      lanes 32 + c carry column c of the rows of W = L11^-1 through the SAME instructions (row j of W is scaled like column j
    //      of L, row c of W receives -L(c, j) x row j like column c of F11).  A wave factorises its block, publishes it in LDS,
    //      a barrier, the waves behind apply it to their columns (the multipliers L(c, j) as LDS broadcast reads): the critical
    //      path is one block's columns + one application per block instead of 24 columns + 276 applications on one wave;
    //   2. every wave: L' = W [F11 F12 b] for its 16-column tile of the pivot rows (operand B = the tile's accumulator
    //      registers as they are, operand A = W from LDS): up to ten matrix instructions back to back; the result is in
    //      operand layout for phase 3 and for the L panel in HBM;
    //   3. every wave: F22 -= L21 L21' on its tiles, up to six instructions per tile back to back.
    WSTAMP();   // children added
    constexpr int NSMAX = kWvNPV / BS, NP = NSMAX * BS;
    constexpr int CW = BS == 7 ? 7 : 6, NCW = NP / CW;   // pivot columns per wave, waves that hold columns
    static_assert(NCW * CW == NP && NCW <= NW, "pivot columns dealt to the waves");
    constexpr int PS = 48;                 // a published column: rows 0 .. 23 of L | entries 0 .. 23 of the row of W
    double* pub = TB;                      // (after barrier 0: every wave has its tiles and columns in registers)
    double* LTl = TB + 1280;               // L' by column tile and 4-column block: [(t * 6 + kb) * 64 + lane]
    static_assert(24 * PS <= 1280 && 1280 + T * 6 * 64 <= NT * 256, "LDS reuse of the tile buffer");
    lane = wv_opaque(lane0);
    const int lr = lane & 15, lk = lane >> 4;
    const int tcr = m >> 4, mcr = m & 15;   // tile / position of the right-hand side column
    const int nkb = (npiv + 3) >> 2;
    double* Lg = P.L + rec.L_off;
    bool bad = false;
    if (w == 0) {
      // the two diagonal tiles that hold pivot rows are read as FULL tiles by phase 2: mirror their upper part
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        double* tile = TB + (t * (t + 1) / 2 + t) * 256;
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const int i = (lane >> 4) + 4 * v, j = lane & 15;
          const double x = tile[lane + 64 * v];
          if (i < j) tile[j * 16 + i] = x;
        }
      }
    }
    // this wave's pivot columns -> registers: lanes >= c hold column c of F11 (element (c, i) of the upper storage), lane 32 + c a one
    double R[CW];
    {
      const int xi = lane - 32;
      const int cpi = CP[min(lane, 31)];
#pragma unroll
      for (int cc = 0; cc < CW; ++cc) {   // (every lane loads a valid address and selects: no exec-mask branches)
        const int c = min(CW * w + cc, NP - 1);
        const double t = TB[((c >> 4) << 8) + ((c & 15) << 4) + cpi];
        double v = (w < NCW && lane >= c && lane < npiv) ? t : 0.0;
        v = (w < NCW && xi == c && c < npiv) ? 1.0 : v;
        R[cc] = v;
      }
    }
    // ---- front -> registers (every wave its own tiles; wave 0 after its mirror)
#pragma unroll
    for (int k = 0; k < OWN; ++k) {
      const int q = min(otj[k] * (otj[k] + 1) / 2 + oti[k], NT - 1);
#pragma unroll
      for (int v = 0; v < 4; ++v) S[k][v] = TB[q * 256 + lane + 64 * v];
    }
    __syncthreads();   // barrier 0: nobody reads the tile buffer any more
    {
      const bool plane_ok = lane < 24 || (lane >= 32 && lane < 56);
      const int plane = lane < 24 ? lane : lane - 8;
      // (a pivot that is not positive is recorded in a VECTOR register and is not replaced: what follows it is not a number, the
      // status word says so; the diagonal of L is stored as d * d^-1/2, the sweeps read the reciprocal diagonal)
      int badv = 0;
      auto pivot = [&](double col, int j) {
        const double d = readlane_f64(col, j);
        badv = d > 0.0 ? badv : 1;
        double sq, rs;
        sqrt_and_rsqrt(d, sq, rs);
        (void)sq;
        return col * rs;
      };
      if (NP < 24 && w == NW - 1 && lane >= 32 && lane < 56) {   // rows of W the blocks do not cover (7 x 7 blocks: 21 columns)
#pragma unroll
        for (int r = NP; r < 24; ++r) pub[r * PS + lane - 8] = 0.0;
      }
#pragma unroll
      for (int k = 0; k < NCW; ++k) {
        if (w == k) {
          if (CW * k < npiv) {   // (wave-uniform) right-looking inside the block, software-pipelined by one column as before
            double l = pivot(R[0], CW * k);
            R[0] = l;
#pragma unroll
            for (int jj = 0; jj + 1 < CW; ++jj) {
              if (CW != BS && CW * k + jj + 1 >= npiv) break;   // (3 x 3 blocks: a wave's six columns are two blocks, the second may be absent)
              R[jj + 1] = fma(-l, readlane_f64(l, CW * k + jj + 1), R[jj + 1]);
              const double ln = pivot(R[jj + 1], CW * k + jj + 1);
#pragma unroll
              for (int cc = jj + 2; cc < CW; ++cc) R[cc] = fma(-l, readlane_f64(l, CW * k + cc), R[cc]);
              R[jj + 1] = ln;
              l = ln;
              __builtin_amdgcn_sched_barrier(0);
            }
          }
          // publish (columns beyond npiv are zero: pivot(0) was not run for them -- R holds the zeros it was loaded with)
          if (plane_ok) {
#pragma unroll
            for (int jj = 0; jj < CW; ++jj) pub[(CW * k + jj) * PS + plane] = R[jj];
          }
        }
        __syncthreads();   // block k is in LDS (the last one: barrier 1 -- W is complete)
        if (k + 1 < NCW && w > k && w < NCW && CW * k < npiv && CW * w < npiv) {
          // apply block k to this wave's columns: R(c) -= l_j x L(c, j), l_j per lane, L(c, j) = entry c of the published column
          double lj[CW];
#pragma unroll
          for (int jj = 0; jj < CW; ++jj) lj[jj] = plane_ok ? pub[(CW * k + jj) * PS + plane] : 0.0;
          const double* mult = pub + CW * w;
#pragma unroll
          for (int jj = 0; jj < CW; ++jj)
#pragma unroll
            for (int cc = 0; cc < CW; ++cc) R[cc] = fma(-lj[jj], mult[(CW * k + jj) * PS + cc], R[cc]);
        }
      }
      bad = bad || badv != 0;
    }
    WSTAMP();   // pivot block
    // ---- phase 2: L' for this wave's column tile(s)
    {
      double a0[4], a1[6];
#pragma unroll
      for (int kb = 0; kb < 4; ++kb) a0[kb] = pub[lr * PS + 24 + 4 * kb + lk];
#pragma unroll
      for (int kb = 0; kb < 6; ++kb) {
        const double v = pub[(16 + (lr & 7)) * PS + 24 + 4 * kb + lk];
        a1[kb] = lr < 8 ? v : 0.0;
      }
      auto panel_out = [&](int t, int kb, double lp) { LTl[(t * 6 + kb) * 64 + lane] = lp; };   // (to HBM at the end of the front: l_panel_out)
      const int t = w + 1;
      if (16 * t < mext) {   // (wave-uniform)
        wv_d4 o0 = wv_d4{0.0, 0.0, 0.0, 0.0}, o1 = wv_d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int kb = 0; kb < 6; ++kb) {
          if (kb < nkb) {
            const double bop = kb < 4 ? S[0][kb & 3] : S[1][kb & 3];
            if (kb < 4) o0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a0[kb & 3], bop, o0, 0, 0, 0);
            if (npiv > 16) o1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1[kb], bop, o1, 0, 0, 0);
          }
        }
#pragma unroll
        for (int kb = 0; kb < 6; ++kb)
          if (kb < nkb) panel_out(t, kb, kb < 4 ? o0[kb & 3] : o1[kb & 3]);
      }
      if (w == 0 && npiv < 16) {   // boundary rows inside the first tile: its own panel (the tile is symmetric: mirrored above)
        wv_d4 o0 = wv_d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int kb = 0; kb < 4; ++kb)
          if (kb < nkb) o0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a0[kb], S[2][kb], o0, 0, 0, 0);
#pragma unroll
        for (int kb = 0; kb < 4; ++kb)
          if (kb < nkb) panel_out(0, kb, o0[kb]);
      }
    }
    WSTAMP();   // panel
    __syncthreads();   // barrier 2: L' of every column tile is in LDS
    // ---- phase 3: rank-npiv update of this wave's tiles that hold boundary rows
#pragma unroll
    for (int k = 0; k < OWN; ++k) {
      if (otj[k] < T && 16 * (oti[k] + 1) > npiv && 16 * oti[k] < m && 16 * otj[k] < mext) {   // (wave-uniform)
        double la[6], lb_[6];
#pragma unroll
        for (int kb = 0; kb < 6; ++kb) {
          la[kb] = LTl[(oti[k] * 6 + kb) * 64 + lane];
          lb_[kb] = LTl[(otj[k] * 6 + kb) * 64 + lane];
        }
#pragma unroll
        for (int kb = 0; kb < 6; ++kb)
          if (kb < nkb) S[k] = __builtin_amdgcn_mfma_f64_16x16x4f64(wv_neg(la[kb]), lb_[kb], S[k], 0, 0, 0);
      }
    }
    if (bad && lane == 0) atomicMax(P.status, 1);   // (2 = a dependency wait gave up: must survive)
    WSTAMP();   // factorisation
    // ---- update vector / update matrix: stay in the tile registers for the next chain front, or go to HBM
    lane = wv_opaque(lane0);
    const bool last = ti_ + 1 == t1;
    if (!last) {
      prev_npiv = npiv;
      prev_m = m;
    } else {
      prev_npiv = 0;
      prev_m = 0;
      double* Ug = P.U + rec.U_off;
      // tile element (r, c), r <= c, is element (c - npiv, r - npiv) of the packed lower-triangular blocks: offset = part
      // of c + part of r
#pragma unroll
      for (int k = 0; k < OWN; ++k) {
        if (otj[k] < T && 16 * (otj[k] + 1) > npiv && 16 * otj[k] <= m && 16 * (oti[k] + 1) > npiv) {   // (wave-uniform)
          const int c = 16 * otj[k] + (lane & 15);
          const int cc = c - npiv;
          const int ib = cc / BS;
          const int ucol = (ib * (ib + 1) / 2) * BB + (cc - ib * BS);
#pragma unroll
          for (int v = 0; v < 4; ++v) {
            const int r = 16 * oti[k] + (lane >> 4) + 4 * v;
            const int rr = r - npiv;
            const int jb = rr / BS;
            const double x = S[k][v];
            if (r >= npiv && r <= c && c < m) {
              st_coh(Ug + ucol + jb * BB + BS * (rr - jb * BS), x);
              if (ib == jb && r != c)   // (above the diagonal of a diagonal block: unused)
                st_coh(Ug + (size_t)(ib * (ib + 1) / 2 + ib) * BB + (rr - jb * BS) + BS * (cc - ib * BS), 0.0);
            }
            if (fwd && r >= npiv && r < m && c == m) st_coh(P.w + rec.w_off + rr, x);
          }
        }
      }
      const bool dep_signal = dep && rec.pad[1] < 0;   // (bit 31) the parent front waits in this launch
      if (dep_signal) {
        __builtin_amdgcn_s_waitcnt(0);   // every wave: its (coherent) U / w stores have been acknowledged
        __syncthreads();
        if (tid == 0) dep_add(P.ready + (rec.pad[1] & 0x00ffffff), 1);
      }
    }
    // ---- the L panel, the reciprocal diagonal and y to HBM -- BEHIND the hand-off: nothing in this launch reads them (the
    // sweeps are later launches), so their address arithmetic and their acknowledgement are off the tree's critical path.
    // Sources: the published pivot block (pub: L11 by column, W's diagonal) and L' by column tile (LTl), both still in LDS.
    lane = wv_opaque(lane0);
    {
      for (int idx = tid; idx < NP * 24; idx += 64 * NW) {
        const int c = idx / 24, i = idx - c * 24;
        if (c < npiv && i < npiv) Lg[i + (size_t)m * c] = pub[c * PS + i];     // (zero above the diagonal; the diagonal as d * d^-1/2)
      }
      if (tid < npiv) Lg[(size_t)m * npiv + tid] = pub[tid * PS + 24 + tid];   // reciprocal diagonal = diagonal of W
      const int lr2 = lane & 15, lk2 = lane >> 4;
      auto l_panel_out = [&](int t) {
#pragma unroll
        for (int kb = 0; kb < 6; ++kb)
          if (kb < nkb) {
            const double lp = LTl[(t * 6 + kb) * 64 + lane];
            const int col = 4 * kb + lk2, row = 16 * t + lr2;
            if (col < npiv && row >= npiv && row < m) Lg[row + (size_t)m * col] = lp;
            if (fwd && t == tcr && lr2 == mcr && col < npiv) yout[(size_t)rec.c0 * BS + col] = lp;
          }
      };
      if (16 * (w + 1) < mext) l_panel_out(w + 1);
      if (w == 0 && npiv < 16) l_panel_out(0);
    }
    __syncthreads();   // TB / the tables are reused by the next front of the chain
    WSTAMP();   // U / w out
#ifdef G2OHIP_CHOL_STAMPS
    if (P.dbg && blockIdx.x == WSTAMP_BLOCK && tid == 0 && nstamp < 58) P.dbg[4 + nstamp++] = -(long long)(ns * 1000 + m);
#endif
  }
#ifdef G2OHIP_CHOL_STAMPS
  if (P.dbg && blockIdx.x == WSTAMP_BLOCK && tid == 0) P.dbg[0] = nstamp;
  if (P.tl && tid == 0) P.tl[6 * (slot0 + blockIdx.x) + 1] = wall_clock64();
#endif
}
