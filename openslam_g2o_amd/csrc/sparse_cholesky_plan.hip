// Multifrontal sparse block Cholesky: the host symbolic analysis (plan_cholesky).  Ordering, elimination tree,
// supernodes and fronts, tasks, multi-GPU partition, launch lists and every table the kernels read; no device
// work (SparseCholesky::analyze uploads the result).
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <numeric>

#include "sparse_cholesky.h"

namespace g2ohip {

// supernode amalgamation, LDS fronts, launch shapes
constexpr double kRelaxZeros = 0.25;              // relaxed amalgamation: tolerated share of explicit zero blocks in a panel
constexpr size_t kRelaxFrontBytes = 42 * 1024;    // ... relaxed merges only while the front stays this small (3 workgroups per CU)
constexpr size_t kLdsFrontBytes = 256 * 1024;     // fronts up to this DENSE size (m*m*8) are candidates for LDS (stored packed: half) ...
constexpr size_t kLdsBudgetBytes = 150 * 1024;    // ... if blocks + vectors + index tables fit this per-workgroup LDS budget
constexpr int kWaveFrontTasks = 1024;             // launches at least this wide use two waves (128 threads) per front
constexpr int kBigFrontMinDim = 180;              // scratch-slab fronts as whole-GPU passes (big_front_passes) on launches whose largest front has this many rows
constexpr int kGatherChildren = 4;   // scratch-slab fronts: children whose update matrices the merged level launch gathers at load time
constexpr int kFillChunk = 4096;         // doubles zeroed by one workgroup of big_fill_kernel

// =====================================================================================
// Host: nested dissection on the block graph (George-Liu automatic nested dissection:
// BFS level structure from a pseudo-peripheral node, separator = the part of the middle
// level that touches the next level).
// =====================================================================================
namespace {

struct NdWork {
  const std::vector<int>& xadj;
  const std::vector<int>& adj;
  std::vector<int> region, level, queue;
  NdWork(int n, const std::vector<int>& xa, const std::vector<int>& a) : xadj(xa), adj(a), region(n, 0), level(n, -1), queue() {
    queue.reserve(n);
  }
  // BFS inside region rid from s; fills queue (visit order) and level[]; returns #levels
  int bfs(int s, int rid) {
    queue.clear();
    queue.push_back(s);
    level[s] = 0;
    size_t head = 0;
    int maxl = 0;
    while (head < queue.size()) {
      int v = queue[head++];
      for (int q = xadj[v]; q < xadj[v + 1]; ++q) {
        int u = adj[q];
        if (region[u] != rid || level[u] >= 0) continue;
        level[u] = level[v] + 1;
        maxl = level[u];
        queue.push_back(u);
      }
    }
    return maxl + 1;
  }
  void clear_levels() {
    for (int v : queue) level[v] = -1;
  }
};

}  // namespace

void nested_dissection(int n, const std::vector<int>& xadj, const std::vector<int>& adj, int leaf, std::vector<int>& perm) {
  perm.assign(n, -1);
  if (n == 0) return;
  NdWork W(n, xadj, adj);
  struct Item {
    std::vector<int> nodes;
    int base, rid;
  };
  std::vector<Item> stack;
  {
    Item it;
    it.nodes.resize(n);
    std::iota(it.nodes.begin(), it.nodes.end(), 0);
    it.base = 0;
    it.rid = 0;
    stack.push_back(std::move(it));
  }
  int next_rid = 1;
  if (leaf < 1) leaf = 1;
  while (!stack.empty()) {
    Item it = std::move(stack.back());
    stack.pop_back();
    const int sz = (int)it.nodes.size();
    if (sz == 0) continue;
    // connected component of the first node
    int nlev = W.bfs(it.nodes[0], it.rid);
    if ((int)W.queue.size() < sz) {
      // split off this component; the rest is handled as another item (independent subtrees)
      Item comp, rest;
      comp.rid = next_rid++;
      rest.rid = next_rid++;
      comp.base = it.base;
      comp.nodes = W.queue;
      for (int v : comp.nodes) W.region[v] = comp.rid;
      W.clear_levels();
      rest.base = it.base + (int)comp.nodes.size();
      rest.nodes.reserve(sz - comp.nodes.size());
      for (int v : it.nodes)
        if (W.region[v] == it.rid) {
          W.region[v] = rest.rid;
          rest.nodes.push_back(v);
        }
      stack.push_back(std::move(rest));
      stack.push_back(std::move(comp));
      continue;
    }
    // connected: pseudo-peripheral start (two more sweeps)
    for (int sweep = 0; sweep < 2; ++sweep) {
      int far = W.queue.back();
      W.clear_levels();
      int nl2 = W.bfs(far, it.rid);
      if (nl2 <= nlev && sweep > 0) {
        nlev = nl2;
        break;
      }
      nlev = nl2;
    }
    if (sz <= leaf || nlev < 3) {
      // leaf: Cuthill-McKee order.  Start = the node of minimum degree (inside the region) in the last level of the
      // level structure (George & Liu's choice of a pseudo-peripheral node); the unnumbered neighbours of a node
      // are numbered by increasing degree.  On a band (a stretch of a camera trajectory) this is the natural order
      // from one end, in either direction: every column then reaches at most `half-width` blocks down, which is
      // what the sliding-window kernel (band_chain.inc) relies on; the plain queue order above numbers the
      // neighbours of the start node farthest first.
      auto deg = [&](int v) {
        int d = 0;
        for (int q = xadj[v]; q < xadj[v + 1]; ++q)
          if (W.region[adj[q]] == it.rid) ++d;
        return d;
      };
      int start = W.queue.back();
      {
        const int last_level = W.level[start];
        int best = deg(start);
        for (int k = sz - 1; k >= 0 && W.level[W.queue[k]] == last_level; --k) {
          const int d = deg(W.queue[k]);
          if (d < best || (d == best && W.queue[k] < start)) {
            best = d;
            start = W.queue[k];
          }
        }
      }
      W.clear_levels();
      std::vector<int> order;
      order.reserve(sz);
      order.push_back(start);
      W.level[start] = 0;
      std::vector<std::pair<int, int>> nbr;
      for (size_t head = 0; head < order.size(); ++head) {
        const int v = order[head];
        nbr.clear();
        for (int q = xadj[v]; q < xadj[v + 1]; ++q) {
          const int u = adj[q];
          if (W.region[u] == it.rid && W.level[u] < 0) {
            W.level[u] = W.level[v] + 1;
            nbr.emplace_back(deg(u), u);
          }
        }
        std::sort(nbr.begin(), nbr.end());
        for (const auto& pr : nbr) order.push_back(pr.second);
      }
      for (int k = 0; k < sz; ++k) perm[it.base + k] = order[k];
      for (int v : order) W.level[v] = -1;
      continue;
    }
    // level sizes
    std::vector<int> lsize(nlev, 0);
    for (int v : W.queue) lsize[W.level[v]]++;
    int best = -1;
    long best_cost = -1;
    int before = 0;
    int fallback = 1;
    long fallback_bal = -1;
    for (int m = 0; m < nlev; ++m) {
      if (m >= 1 && m <= nlev - 2) {
        int after = sz - before - lsize[m];
        int bal = std::min(before, after);
        if (bal > fallback_bal) {
          fallback_bal = bal;
          fallback = m;
        }
        if (bal * 4 >= sz) {  // each side at least 25 %
          long cost = (long)lsize[m] * 1000000L - bal;  // smallest separator, then best balance
          if (best < 0 || cost < best_cost) {
            best = m;
            best_cost = cost;
          }
        }
      }
      before += lsize[m];
    }
    const int m = best >= 0 ? best : fallback;
    Item A, B;
    A.rid = next_rid++;
    B.rid = next_rid++;
    std::vector<int> sep;
    for (int v : W.queue) {
      int lv = W.level[v];
      if (lv < m)
        A.nodes.push_back(v);
      else if (lv > m)
        B.nodes.push_back(v);
      else {
        bool touches = false;
        for (int q = xadj[v]; q < xadj[v + 1] && !touches; ++q) {
          int u = adj[q];
          if (W.region[u] == it.rid && W.level[u] == m + 1) touches = true;
        }
        if (touches)
          sep.push_back(v);
        else
          A.nodes.push_back(v);
      }
    }
    W.clear_levels();
    for (int v : A.nodes) W.region[v] = A.rid;
    for (int v : B.nodes) W.region[v] = B.rid;
    for (int v : sep) W.region[v] = -1;  // ordered
    A.base = it.base;
    B.base = it.base + (int)A.nodes.size();
    int sbase = B.base + (int)B.nodes.size();
    for (size_t k = 0; k < sep.size(); ++k) perm[sbase + k] = sep[k];
    stack.push_back(std::move(A));
    stack.push_back(std::move(B));
  }
}

// =====================================================================================
// Host: symbolic analysis
// =====================================================================================
namespace {

// lower pattern (CSC: for column j rows i>j) and its transpose (for row i the columns j<i)
// of the permuted matrix
void permuted_lower(int nb, const int* colptr, const int* rowidx, const std::vector<int>& iperm, std::vector<int>& cp,
                    std::vector<int>& ci, std::vector<int>& rp, std::vector<int>& ri) {
  cp.assign(nb + 1, 0);
  rp.assign(nb + 1, 0);
  for (int c = 0; c < nb; ++c)
    for (int q = colptr[c]; q < colptr[c + 1]; ++q) {
      int r = rowidx[q];
      if (r == c) continue;
      int a = iperm[r], b = iperm[c];
      int i = std::max(a, b), j = std::min(a, b);
      cp[j + 1]++;
      rp[i + 1]++;
    }
  for (int k = 0; k < nb; ++k) {
    cp[k + 1] += cp[k];
    rp[k + 1] += rp[k];
  }
  ci.assign(cp[nb], 0);
  ri.assign(rp[nb], 0);
  std::vector<int> wc(cp.begin(), cp.end() - 1), wr(rp.begin(), rp.end() - 1);
  for (int c = 0; c < nb; ++c)
    for (int q = colptr[c]; q < colptr[c + 1]; ++q) {
      int r = rowidx[q];
      if (r == c) continue;
      int a = iperm[r], b = iperm[c];
      int i = std::max(a, b), j = std::min(a, b);
      ci[wc[j]++] = i;
      ri[wr[i]++] = j;
    }
  for (int j = 0; j < nb; ++j) std::sort(ci.begin() + cp[j], ci.begin() + cp[j + 1]);
}

void etree(int nb, const std::vector<int>& rp, const std::vector<int>& ri, std::vector<int>& parent) {
  parent.assign(nb, -1);
  std::vector<int> anc(nb, -1);
  for (int k = 0; k < nb; ++k)
    for (int q = rp[k]; q < rp[k + 1]; ++q) {
      int i = ri[q];
      while (i != -1 && i < k) {
        int nx = anc[i];
        anc[i] = k;
        if (nx == -1) parent[i] = k;
        i = nx;
      }
    }
}

void postorder(int nb, const std::vector<int>& parent, std::vector<int>& post) {
  std::vector<int> head(nb, -1), next(nb, -1);
  for (int j = nb - 1; j >= 0; --j)
    if (parent[j] >= 0) {
      next[j] = head[parent[j]];
      head[parent[j]] = j;
    }
  post.clear();
  post.reserve(nb);
  std::vector<int> stk;
  for (int r = 0; r < nb; ++r) {
    if (parent[r] >= 0) continue;
    stk.push_back(r);
    while (!stk.empty()) {
      int v = stk.back();
      int c = head[v];
      if (c == -1) {
        post.push_back(v);
        stk.pop_back();
      } else {
        head[v] = next[c];
        stk.push_back(c);
      }
    }
  }
}


// The stages of plan_cholesky, in order; the members are what one stage hands on to the next.
struct Planner {
  CholPlan& P;
  CholSymbolic& S;
  const CholOptions& opt;
  const int bs, nb;
  const int *colptr, *rowidx;
  Planner(CholPlan& plan, int bs_, int nb_, const int* colptr_, const int* rowidx_)
      : P(plan), S(plan.sym), opt(plan.opt), bs(bs_), nb(nb_), colptr(colptr_), rowidx(rowidx_) {}

  std::vector<int> perm0;                  // nested-dissection order (before the postorder)
  bool band_like = true;                   // the block graph is a band (a camera trajectory)
  std::vector<std::vector<int>> st_;       // column structures struct(j) = rows > j of L(:,j)
  int nf = 0, nnzb = 0, nlev = 0, ntask = 0;
  std::vector<int> sn_of;                  // block column -> front
  std::vector<int> ent_front;              // original block -> front
  std::vector<int> task_of, task_level;
  std::vector<int> inpl_prev, inpl_next;   // scratch-slab fronts continued in place
  std::vector<int> grp_prev, grp_rem;      // grouped in-place chains
  std::vector<int> factor_order;           // launch slot -> task for the FACTOR launches (solve sweeps keep level order)
  int sw_max = 0;                          // row chunks of the widest multi-workgroup sweep launch
  int why_cnt[32] = {0};                   // band chains rejected, by rule

  void order();
  void etree_and_columns();
  void supernodes();
  void assembly_and_storage();
  void tasks();
  void partition();
  void launch_lists();
  void scratch_slab();
  void front_records();
  void grouped_chains();
  void big_tiles();
  void backward_runs();
  void hoisted_chunks();
  void two_streams();
  void factor_groups();
  void band_chains();
  void tree_backward();
  void exchange();
  void slot_orders();

  int local_pos(int f, int i) const;
  size_t front_dim(int f) const { return (size_t)(S.f_ns[f] + S.f_nb[f]) * bs; }
  long long lds_need(int f, long long& lds_ints) const;
  bool is_lds(int f) const;
  struct BandInfo {
    BandChainRec rec;
    std::vector<int> tab, ent_asm;
    std::vector<int4> ent;
  };
  bool try_band(int t, BandInfo& out);
  bool why(int c) { ++why_cnt[c & 31]; return false; }
  std::vector<int2> slots_of(const std::vector<int>& order) const;
};

// --- block graph, leaf size, nested dissection
void Planner::order() {
  std::vector<int> xadj(nb + 1, 0), adj;
  for (int c = 0; c < nb; ++c)
    for (int q = colptr[c]; q < colptr[c + 1]; ++q) {
      int r = rowidx[q];
      if (r > c) throw ArgFailure("analyze: pattern must be upper triangular (row block <= column block)");
      if (r != c) {
        xadj[r + 1]++;
        xadj[c + 1]++;
      }
    }
  for (int k = 0; k < nb; ++k) xadj[k + 1] += xadj[k];
  adj.resize(xadj[nb]);
  {
    std::vector<int> w(xadj.begin(), xadj.end() - 1);
    for (int c = 0; c < nb; ++c)
      for (int q = colptr[c]; q < colptr[c + 1]; ++q) {
        int r = rowidx[q];
        if (r != c) {
          adj[w[r]++] = c;
          adj[w[c]++] = r;
        }
      }
    // duplicates cannot occur: the pattern has unique (r,c)
  }
  // leaf size: large systems get about as many leaves as the band kernel has chain slots (256 CUs x 8 one-wave chains, one
  // round instead of two and one tree level less: 0.53 -> 0.48 ms at the metric configuration), within what a chain may hold
  // (round 6) nd_leaf = 0 (default): by the shape of the graph.  A camera trajectory's reduced system is a BAND -- the level structure
  // from a pseudo-peripheral node has a handful of blocks per level --: its leaves are the band kernel's chains, long ones (32 blocks
  // and more).  Anything wider (pose graphs, loop closures) gets leaves of 4 blocks: the separators then do the ordering and the tree
  // is a third shallower (sphere 2 200: 57 -> 37 levels, 2.07 -> 1.44 ms per solve; manhattan: fill 2.45 -> 1.89 x the reference's
  // block-AMD; profiles/r6_nd_leaf.txt).
  int nd_leaf = opt.nd_leaf;
  band_like = true;   // (an explicit leaf size keeps the band kernel's supernode width)
  if (nd_leaf <= 0) {
    band_like = false;
    if (nb > 0) {
      NdWork W(nb, xadj, adj);
      int nlev = W.bfs(0, 0);
      for (int sweep = 0; sweep < 2; ++sweep) {
        const int far = W.queue.back();
        W.clear_levels();
        nlev = W.bfs(far, 0);
      }
      std::vector<int> lsize(nlev, 0);
      for (int v : W.queue) lsize[W.level[v]]++;
      const int widest = *std::max_element(lsize.begin(), lsize.end());
      band_like = widest <= 12 && (long long)W.queue.size() <= 6LL * nlev;   // (the component of block 0 stands for the graph)
    }
    nd_leaf = band_like ? 32 : 4;
  }
  if (opt.band_kernel && bs == 6 && nd_leaf >= 32) nd_leaf = std::min(std::max(nd_leaf, (nb / std::max(opt.world, 1) + 2047) / 2048), 128);   // (per rank: its share of the chains)
  nested_dissection(nb, xadj, adj, nd_leaf, perm0);
}

void Planner::etree_and_columns() {
  // --- etree + postorder, compose
  std::vector<int> iperm(nb), cp, ci, rp, ri, parent, post;
  for (int k = 0; k < nb; ++k) iperm[perm0[k]] = k;
  permuted_lower(nb, colptr, rowidx, iperm, cp, ci, rp, ri);
  etree(nb, rp, ri, parent);
  postorder(nb, parent, post);
  S.perm.resize(nb);
  S.iperm.resize(nb);
  for (int k = 0; k < nb; ++k) S.perm[k] = perm0[post[k]];
  for (int k = 0; k < nb; ++k) S.iperm[S.perm[k]] = k;
  permuted_lower(nb, colptr, rowidx, S.iperm, cp, ci, rp, ri);
  etree(nb, rp, ri, S.parent);
  // --- column structures struct(j) = rows > j of L(:,j)
  st_.resize(nb);
  {
    std::vector<int> mark(nb, -1);
    std::vector<std::vector<int>> kids(nb);
    for (int j = 0; j < nb; ++j)
      if (S.parent[j] >= 0) kids[S.parent[j]].push_back(j);
    for (int j = 0; j < nb; ++j) {
      std::vector<int>& s = st_[j];
      mark[j] = j;
      for (int q = cp[j]; q < cp[j + 1]; ++q) {
        int i = ci[q];
        if (mark[i] != j) {
          mark[i] = j;
          s.push_back(i);
        }
      }
      for (int c : kids[j])
        for (int i : st_[c])
          if (i != j && mark[i] != j) {
            mark[i] = j;
            s.push_back(i);
          }
      std::sort(s.begin(), s.end());
    }
  }
}

void Planner::supernodes() {
  // --- supernodes (maximal chains with nested structure), capped in width
  // (a pivot panel wider than 64 scalars has no whole-GPU pass: its level would fall back to one workgroup per front -- 430 ms instead of
  // 18 on the 10 000-camera grid graph, profiles/r6_grid_sweep.txt -- so the cap is itself capped)
  const int max_sn_blocks = std::max(1, std::min(opt.max_sn_scalars, 64) / bs);
  // supernodes of the LDS-resident fronts: 24 scalars = the register fronts of the band graphs (wave_front_kernel); graphs that are not a
  // band have few such fronts and gain from twice the width (manhattan 0.845 -> 0.831, sphere 1.442 -> 1.414 ms: fewer levels)
  const int sn_lds = (opt.max_sn_scalars_lds <= 0) ? (band_like ? 24 : 48) : opt.max_sn_scalars_lds;
  // scratch-slab fronts of a thousand rows and more: panels of the full 64 scalars (every panel is a level of whole-GPU passes: fewer of them)
  // (10 000-camera grid graph: 169 -> 143 levels, 21.6 -> 20.6 ms; 49 729 cameras 100.7 -> 97.6; narrower thresholds cost the pose graphs
  // levels of their own: profiles/r6_grid_sweep.txt)
  constexpr int wide_rows = 1024;
  const int wide_blocks = opt.max_sn_scalars >= 48 ? std::max(max_sn_blocks, 64 / bs) : max_sn_blocks;
  S.sn_start.clear();
  {
    // Exact merges (identical structure) always; relaxed merges along a parent chain while the
    // explicit zero blocks stay below kRelaxZeros of the dense panel and the front still fits LDS.
    long true_blocks = 0;  // structural blocks of the current supernode's columns
    for (int j = 0; j < nb; ++j) {
      bool merge = false;
      if (j > 0 && S.parent[j - 1] == j) {
        const int c0 = S.sn_start.back();
        const long w = j - c0 + 1, nbn = (long)st_[j].size();
        const long total = w * (w + 1) / 2 + w * nbn;
        const long tb = true_blocks + 1 + nbn;
        const bool exact = st_[j - 1].size() == st_[j].size() + 1 && total == tb;
        const size_t m = (size_t)(w + nbn) * bs;
        const bool fits = m * m * 8 <= std::min(kLdsFrontBytes, kRelaxFrontBytes);
        // narrower panels for the fronts that live in LDS (shorter pivot loops per front, smaller solve panels), wide
        // ones for the scratch-slab fronts (each panel is a whole-GPU pass there)
        const bool lds_class = m * m * 8 <= kLdsFrontBytes;
        const long cap = lds_class ? std::max(1, std::min(opt.max_sn_scalars, sn_lds) / bs) : (m >= (size_t)wide_rows ? wide_blocks : max_sn_blocks);
        if (w <= cap && (exact || (fits && (double)(total - tb) <= kRelaxZeros * (double)total))) merge = true;
      }
      if (!merge) {
        S.sn_start.push_back(j);
        true_blocks = 0;
      }
      true_blocks += 1 + (long)st_[j].size();
    }
  }
  nf = (int)S.sn_start.size();
  S.sn_start.push_back(nb);
  sn_of.resize(nb);
  for (int f = 0; f < nf; ++f)
    for (int j = S.sn_start[f]; j < S.sn_start[f + 1]; ++j) sn_of[j] = f;
  S.f_ns.resize(nf);
  S.f_nb.resize(nf);
  S.f_parent.assign(nf, -1);
  S.f_level.assign(nf, 0);
  S.rows_off.assign(nf + 1, 0);
  for (int f = 0; f < nf; ++f) {
    int last = S.sn_start[f + 1] - 1;
    S.f_ns[f] = S.sn_start[f + 1] - S.sn_start[f];
    S.f_nb[f] = (int)st_[last].size();
    S.rows_off[f + 1] = S.rows_off[f] + S.f_nb[f];
    if (!st_[last].empty()) S.f_parent[f] = sn_of[st_[last][0]];
  }
  S.rows.resize(S.rows_off[nf]);
  for (int f = 0; f < nf; ++f) {
    int last = S.sn_start[f + 1] - 1;
    std::copy(st_[last].begin(), st_[last].end(), S.rows.begin() + S.rows_off[f]);
  }
  // --- child -> parent relative indices, children lists, levels
  S.rel_off = S.rows_off;
  S.rel.assign(S.rows.size(), -1);
  S.child_off.assign(nf + 1, 0);
  for (int f = 0; f < nf; ++f)
    if (S.f_parent[f] >= 0) S.child_off[S.f_parent[f] + 1]++;
  for (int f = 0; f < nf; ++f) S.child_off[f + 1] += S.child_off[f];
  S.children.resize(S.child_off[nf]);
  {
    std::vector<int> w(S.child_off.begin(), S.child_off.end() - 1);
    for (int f = 0; f < nf; ++f) {
      int p = S.f_parent[f];
      if (p < 0) continue;
      S.children[w[p]++] = f;
      for (int k = 0; k < S.f_nb[f]; ++k) {
        int lp = local_pos(p, S.rows[S.rows_off[f] + k]);
        if (lp < 0) throw StateFailure("symbolic: child row missing in parent front");
        S.rel[S.rel_off[f] + k] = lp;
      }
      S.f_level[p] = std::max(S.f_level[p], S.f_level[f] + 1);  // fronts are postordered: children first
    }
  }
}

// local position of a permuted block row i in front f (pivots first, then boundary rows)
int Planner::local_pos(int f, int i) const {
  int c0 = S.sn_start[f], c1 = S.sn_start[f + 1];
  if (i >= c0 && i < c1) return i - c0;
  const int* b = S.rows.data() + S.rows_off[f];
  const int* e = b + S.f_nb[f];
  const int* it = std::lower_bound(b, e, i);
  if (it == e || *it != i) return -1;
  return S.f_ns[f] + (int)(it - b);
}

void Planner::assembly_and_storage() {
  // --- assembly lists of original blocks
  S.asm_off.assign(nf + 1, 0);
  nnzb = colptr[nb];
  ent_front.resize(nnzb);
  std::vector<int> ent_pos(nnzb);
  for (int c = 0; c < nb; ++c)
    for (int q = colptr[c]; q < colptr[c + 1]; ++q) {
      int r = rowidx[q];
      int a = S.iperm[r], b = S.iperm[c];
      int i = std::max(a, b), j = std::min(a, b);
      int tr = (a < b) ? 1 : 0;  // stored block is A(r,c); front holds F(i,j) = A(perm i, perm j)
      if (r == c) tr = 0;
      int f = sn_of[j];
      int lr = local_pos(f, i), lc = j - S.sn_start[f];
      if (lr < 0 || lr >= (1 << 15)) throw StateFailure("symbolic: assembly position out of range");
      ent_front[q] = f;
      ent_pos[q] = lr | (lc << 15) | (tr << 30);
      S.asm_off[f + 1]++;
    }
  for (int f = 0; f < nf; ++f) S.asm_off[f + 1] += S.asm_off[f];
  S.asm_q.resize(nnzb);
  S.asm_pos.resize(nnzb);
  {
    std::vector<int> w(S.asm_off.begin(), S.asm_off.end() - 1);
    for (int q = 0; q < nnzb; ++q) {
      int d = w[ent_front[q]]++;
      S.asm_q[d] = q;
      S.asm_pos[d] = ent_pos[q];
    }
  }
  // --- storage
  S.L_off.resize(nf);
  S.U_off.resize(nf);
  S.w_off.resize(nf);
  S.L_total = S.U_total = S.w_total = 0;
  for (int f = 0; f < nf; ++f) {
    long long m = (long long)(S.f_ns[f] + S.f_nb[f]) * bs, np = (long long)S.f_ns[f] * bs, nbs = (long long)S.f_nb[f] * bs;
    S.L_off[f] = S.L_total;
    S.L_total += m * np + np;   // panel + reciprocals of its diagonal (used by the triangular sweeps)
    S.U_off[f] = S.U_total;
    S.U_total += (long long)S.f_nb[f] * (S.f_nb[f] + 1) / 2 * bs * bs;   // lower-triangular blocks, packed by block column
    S.w_off[f] = S.w_total;
    S.w_total += nbs;
    P.stats.nnzL += (size_t)(np * m - np * (np - 1) / 2);
    P.stats.max_front_dim = std::max(P.stats.max_front_dim, (size_t)m);
    for (long long k = 0; k < np; ++k) P.stats.flops += (double)(m - k) * (double)(m - k);
  }
  P.stats.n_fronts = nf;
  P.stats.bytes_L = (size_t)S.L_total * 8;
}

// LDS-resident iff the dense size is within the class limit AND everything the factor kernel keeps in LDS for this
// front (packed blocks, rhs vectors, mailboxes, index tables) fits the per-workgroup budget; lds_ints: the index part
long long Planner::lds_need(int f, long long& lds_ints) const {
  const long long nbt = S.f_ns[f] + S.f_nb[f], mm = nbt * bs;
  const long long T_ = (bs % 3 == 0) ? 3 : bs;
  const long long nt0 = (nbt - 1) * bs / T_;
  long long ints = (2 + kVirtInts) * (long long)(S.asm_off[f + 1] - S.asm_off[f]) + std::max(nt0 * (nt0 + 1) / 2, (long long)S.f_nb[f] * (S.f_nb[f] + 1) / 2) + 4;
  for (int ch = S.child_off[f]; ch < S.child_off[f + 1]; ++ch) {
    const long long nbc = S.f_nb[S.children[ch]];
    ints += nbc * (nbc + 1) / 2 + nbc;
  }
  lds_ints = 4 * ints;
  return 8 * (nbt * (nbt + 1) / 2 * bs * bs + 2 * mm + 2 * (bs * bs + bs)) + 4 * ints;
}

// A launch sizes its LDS by the largest block part and the largest index part among ITS fronts separately (the kernel
// places the index tables behind a launch-uniform block region), so the two parts are capped separately: their sum of
// maxima then fits whatever fronts share a launch.  (A front with few rows but a child with hundreds of boundary
// blocks -- a landmark seen by hundreds of poses -- used to push a launch beyond 160 KB.)
bool Planner::is_lds(int f) const {
  if (front_dim(f) * front_dim(f) * 8 > kLdsFrontBytes) return false;
  long long lds_ints = 0;
  const long long total = lds_need(f, lds_ints);
  const long long cap = (long long)kLdsBudgetBytes;
  return total <= cap && lds_ints <= 24 * 1024 && total - lds_ints <= 134 * 1024;   // (158 KB of the CU's 160 KB)
}

void Planner::tasks() {
  // --- tasks: a front whose parent has no other child is fused with it (chain); the workgroup that
  // factorises the child carries the update matrix to the parent in registers.  Both fronts must be
  // LDS-resident and the carried matrix must fit kChainU doubles per thread.
  std::vector<int> chain_next(nf, -1), has_prev(nf, 0);
  for (int f = 0; f < nf; ++f) {
    const int p = S.f_parent[f];
    if (p < 0 || S.child_off[p + 1] - S.child_off[p] != 1 || !is_lds(f) || !is_lds(p)) continue;
    if ((size_t)S.f_nb[f] * (S.f_nb[f] + 1) / 2 * bs * bs > (size_t)kChainU * kFactorThreads) continue;
    if (S.f_nb[f] * bs > 256) continue;   // solve kernels carry the boundary vector in one round
    chain_next[f] = p;
    has_prev[p] = 1;
  }
  S.task_ptr.assign(1, 0);
  S.task_fronts.clear();
  task_of.assign(nf, -1);
  for (int f = 0; f < nf; ++f) {
    if (has_prev[f]) continue;
    const int t = (int)S.task_ptr.size() - 1;
    int lvl = 0;
    for (int ch = S.child_off[f]; ch < S.child_off[f + 1]; ++ch) lvl = std::max(lvl, task_level[task_of[S.children[ch]]] + 1);
    for (int g = f; g >= 0; g = chain_next[g]) {
      S.task_fronts.push_back(g);
      task_of[g] = t;
    }
    S.task_ptr.push_back((int)S.task_fronts.size());
    task_level.push_back(lvl);
  }
  ntask = (int)task_level.size();
  nlev = 0;
  for (int t = 0; t < ntask; ++t) nlev = std::max(nlev, task_level[t] + 1);
  P.stats.n_levels = nlev;
  P.stats.n_tasks = ntask;
}

void Planner::partition() {
  // --- multi-GPU partition of the task tree: the top of the tree is split until there are >= world
  // subtrees and the longest-processing-time deal of them to the ranks is balanced within 10%; every task
  // above them is "shared" and executed redundantly by all ranks
  S.task_owner.assign(ntask, opt.world > 1 ? -2 : opt.rank);
  S.xroots.clear();
  if (opt.world > 1) {
    std::vector<std::vector<int>> tkids(ntask);
    std::vector<int> tparent(ntask, -1);
    for (int t = 0; t < ntask; ++t) {
      const int last = S.task_fronts[S.task_ptr[t + 1] - 1];
      const int pf = S.f_parent[last];
      if (pf >= 0) {
        tparent[t] = task_of[pf];
        tkids[task_of[pf]].push_back(t);
      }
    }
    std::vector<double> work(ntask, 0.0);
    for (int t = 0; t < ntask; ++t) {   // tasks are created in postorder of their head fronts: children first
      for (int k = S.task_ptr[t]; k < S.task_ptr[t + 1]; ++k) {
        const double m = (double)front_dim(S.task_fronts[k]), np = (double)S.f_ns[S.task_fronts[k]] * bs;
        work[t] += np * m * m;
      }
      for (int c : tkids[t]) work[t] += work[c];
    }
    std::vector<int> cut;
    for (int t = 0; t < ntask; ++t)
      if (tparent[t] < 0) cut.push_back(t);
    // longest-processing-time deal of the current cut; returns max load / mean load
    std::vector<int> cut_rank;
    auto deal = [&]() {
      std::vector<int> order(cut.size());
      for (size_t k = 0; k < cut.size(); ++k) order[k] = (int)k;
      std::sort(order.begin(), order.end(), [&](int x, int y) { return work[cut[x]] != work[cut[y]] ? work[cut[x]] > work[cut[y]] : cut[x] < cut[y]; });
      std::vector<double> load(opt.world, 0.0);
      cut_rank.assign(cut.size(), 0);
      double total = 0.0;
      for (int k : order) {
        int r = 0;
        for (int q = 1; q < opt.world; ++q)
          if (load[q] < load[r]) r = q;
        load[r] += work[cut[k]];
        cut_rank[k] = r;
        total += work[cut[k]];
      }
      return *std::max_element(load.begin(), load.end()) / std::max(total / opt.world, 1e-300);
    };
    for (;;) {
      const bool enough = (int)cut.size() >= opt.world;
      if (enough && ((int)cut.size() >= 8 * opt.world || deal() <= 1.10)) break;
      int best = -1;
      for (size_t k = 0; k < cut.size(); ++k)
        if (!tkids[cut[k]].empty() && (best < 0 || work[cut[k]] > work[cut[best]])) best = (int)k;
      if (best < 0) break;
      const int t = cut[best];
      S.task_owner[t] = -1;   // shared
      cut.erase(cut.begin() + best);
      for (int c : tkids[t]) cut.push_back(c);
    }
    deal();
    for (size_t k = 0; k < cut.size(); ++k) {
      const int t = cut[k];
      std::vector<int> stk(1, t);
      while (!stk.empty()) {
        int u = stk.back();
        stk.pop_back();
        S.task_owner[u] = cut_rank[k];
        for (int c : tkids[u]) stk.push_back(c);
      }
      if (tparent[t] >= 0) S.xroots.push_back(t);   // its update matrix / vector feeds a shared task
    }
    std::sort(S.xroots.begin(), S.xroots.end());
    for (int t = 0; t < ntask; ++t)
      if (S.task_owner[t] == -2) throw StateFailure("partition: unassigned task");
  }
  S.pose_owner.assign(nb, opt.rank);
  for (int t = 0; t < ntask; ++t)
    for (int k = S.task_ptr[t]; k < S.task_ptr[t + 1]; ++k) {
      const int f = S.task_fronts[k];
      for (int j = S.sn_start[f]; j < S.sn_start[f + 1]; ++j) S.pose_owner[S.perm[j]] = S.task_owner[t];
    }
  S.block_consumer.resize(nnzb);
  for (int q = 0; q < nnzb; ++q) S.block_consumer[q] = S.task_owner[task_of[ent_front[q]]];
}

void Planner::launch_lists() {
  // --- launch lists (task ids) per phase: [0] this rank's tasks, [1] shared tasks; inside a level the
  // LDS-class tasks come first, then the scratch-slab (single large front) tasks
  S.level_fronts.clear();
  for (int ph = 0; ph < 2; ++ph) {
    P.launches[ph].assign(nlev, LevelLaunch());
    std::vector<std::vector<int>> lds(nlev), glb(nlev);
    for (int t = 0; t < ntask; ++t) {
      const bool in_phase = ph == 0 ? (S.task_owner[t] == opt.rank) : (S.task_owner[t] == -1);
      if (!in_phase) continue;
      (is_lds(S.task_fronts[S.task_ptr[t]]) ? lds : glb)[task_level[t]].push_back(t);
    }
    for (int l = 0; l < nlev; ++l) {
      LevelLaunch& LL = P.launches[ph][l];
      LL.lds_begin = (int)S.level_fronts.size();
      LL.lds_count = (int)lds[l].size();
      // levels whose fronts all fit the register-resident wave kernel (wave_front.inc): <= kWvNPV pivot columns,
      // <= 16 kWvNTL boundary rows, <= kFwdChildren children
      LL.wv = glb[l].empty() && !lds[l].empty();
      for (int t : lds[l]) {
        if (!LL.wv) break;
        for (int k = S.task_ptr[t]; k < S.task_ptr[t + 1] && LL.wv; ++k) {
          const int f = S.task_fronts[k];
          const int npv = S.f_ns[f] * bs, nbr = S.f_nb[f] * bs;
          if (npv > kWvNPV || nbr > 16 * kWvNTL || S.child_off[f + 1] - S.child_off[f] > kFwdChildren) LL.wv = false;
          if (S.asm_off[f + 1] - S.asm_off[f] > 64) LL.wv = false;   // (one table entry per lane)
          for (int ch = S.child_off[f]; ch < S.child_off[f + 1]; ++ch) {
            const int nbc = S.f_nb[S.children[ch]];
            if (nbc * (nbc + 1) / 2 > 64) LL.wv = false;
          }
        }
      }
      // wide launches run two waves per front (see front_factor_kernel); *_max_m = packed doubles of the largest front
      if (!LL.wv && LL.lds_count >= kWaveFrontTasks) LL.sm_count = LL.lds_count;
      for (int i = 0; i < (int)lds[l].size(); ++i) {
        const int t = lds[l][i];
        S.level_fronts.push_back(t);
        P.scratch_off.push_back(0);
        int& mx = i < LL.sm_count ? LL.sm_max_m : LL.lds_max_m;
        for (int k = S.task_ptr[t]; k < S.task_ptr[t + 1]; ++k) {
          const int nbt = S.f_ns[S.task_fronts[k]] + S.f_nb[S.task_fronts[k]];
          mx = std::max(mx, nbt * (nbt + 1) / 2 * bs * bs);
        }
      }
      LL.glb_begin = (int)S.level_fronts.size();
      LL.glb_count = (int)glb[l].size();
      long long so = 0;
      for (int t : glb[l]) {
        P.scratch_off.push_back(so);
        const long long m = (long long)front_dim(S.task_fronts[S.task_ptr[t]]);
        so += m * m;
        S.level_fronts.push_back(t);
        LL.glb_max_m = std::max(LL.glb_max_m, (int)m);
      }
      P.scratch_max = std::max(P.scratch_max, so);
      LL.glb_scratch = so;
      for (int q = LL.lds_begin; q < LL.glb_begin + LL.glb_count; ++q) {
        const int t = S.level_fronts[q];
        for (int k = S.task_ptr[t]; k < S.task_ptr[t + 1]; ++k) {
          const int f = S.task_fronts[k];
          const int m = (int)front_dim(f);
          LL.max_m = std::max(LL.max_m, m);
          LL.max_panel = std::max(LL.max_panel, m * S.f_ns[f] * bs + S.f_ns[f] * bs);
        }
      }
    }
  }
  if (getenv("G2OHIP_PLAN_DUMP")) {   // per level: tasks, fronts per task, histogram of the largest front (blocks) per task
    for (int l = 0; l < nlev; ++l) {
      const LevelLaunch& LL = P.launches[0][l];
      std::vector<int> hist(32, 0);
      long long nfr = 0, npiv = 0, sumtri = 0;
      for (int q = LL.lds_begin; q < LL.lds_begin + LL.lds_count; ++q) {
        const int t = S.level_fronts[q];
        int mx = 0;
        for (int k = S.task_ptr[t]; k < S.task_ptr[t + 1]; ++k) {
          const int f = S.task_fronts[k], nbt = S.f_ns[f] + S.f_nb[f];
          mx = std::max(mx, nbt);
          ++nfr;
          npiv += S.f_ns[f];
          sumtri += nbt * (nbt + 1) / 2;
        }
        ++hist[std::min(mx, 31)];
      }
      fprintf(stderr, "level %d: tasks %d fronts %lld pivots %lld blocks %lld | max-front hist:", l, LL.lds_count, nfr, npiv, sumtri);
      for (int i = 0; i < 32; ++i)
        if (hist[i]) fprintf(stderr, " %d:%d", i, hist[i]);
      fprintf(stderr, "\n");
    }
  }
}

void Planner::scratch_slab() {
  // --- scratch-slab fronts: where each one lives, and CHAINS factorised in place.
  // A large supernode is cut into panels of <= max_sn_scalars pivot columns: a chain of fronts, each the only child of
  // the next, the parent's rows being exactly the child's boundary rows.  Such a parent is factorised IN PLACE in the
  // trailing part of its child's frontal matrix: the child's rank-npiv update writes there instead of a packed update
  // matrix, the parent adds its original blocks, and neither the zero fill, nor the extend-add, nor the O(m^2) update
  // matrix per panel exist (a dense m-row supernode used to cost m^3 / (6 * 48) doubles of update matrices).
  // Every front that is not such a parent owns a region of the slab for good (no reuse across levels: a chain keeps
  // its region over several levels).
  P.scratch_ld.assign(P.scratch_off.size(), 0);
  inpl_prev.assign(nf, -1);
  inpl_next.assign(nf, -1);
  {
    std::vector<int> slot_of(nf, -1), lvl_of(nf, -1), ph_of(nf, -1);
    // whole-GPU passes for the level's scratch-slab fronts (LevelLaunch::big_passes)
    auto level_big = [&](const LevelLaunch& LL) {
      if (LL.glb_count <= 0 || !opt.big_front_passes || LL.glb_max_m < kBigFrontMinDim) return false;
      for (int q = LL.glb_begin; q < LL.glb_begin + LL.glb_count; ++q) {
        const int f = S.task_fronts[S.task_ptr[S.level_fronts[q]]];
        if (S.f_ns[f] * bs > 64 || S.child_off[f + 1] - S.child_off[f] > 16) return false;
      }
      return true;
    };
    for (int ph = 0; ph < 2; ++ph)
      for (int l = 0; l < nlev; ++l) {
        LevelLaunch& LL = P.launches[ph][l];
        LL.big_passes = level_big(LL);
        for (int q = LL.glb_begin; q < LL.glb_begin + LL.glb_count; ++q) {
          const int f = S.task_fronts[S.task_ptr[S.level_fronts[q]]];
          slot_of[f] = q;
          lvl_of[f] = l;
          ph_of[f] = ph;
        }
      }
    if (opt.world == 1)
      for (int f = 0; f < nf; ++f) {
        if (slot_of[f] < 0 || S.child_off[f + 1] - S.child_off[f] != 1) continue;
        const int c = S.children[S.child_off[f]];
        if (slot_of[c] < 0 || ph_of[c] != ph_of[f] || lvl_of[c] + 1 != lvl_of[f]) continue;
        if (!P.launches[ph_of[f]][lvl_of[f]].big_passes || !P.launches[ph_of[c]][lvl_of[c]].big_passes) continue;
        if (S.f_ns[f] + S.f_nb[f] != S.f_nb[c]) continue;
        bool ident = true;
        for (int k = 0; k < S.f_nb[c] && ident; ++k) ident = S.rel[S.rel_off[c] + k] == k;
        if (!ident) continue;
        inpl_prev[f] = c;
        inpl_next[c] = f;
      }
    long long total = 0;
    for (int ph = 0; ph < 2; ++ph)
      for (int l = 0; l < nlev; ++l) {   // (levels ascending: a child's region is placed before its in-place parent)
        LevelLaunch& LL = P.launches[ph][l];
        for (int q = LL.glb_begin; q < LL.glb_begin + LL.glb_count; ++q) {
          const int f = S.task_fronts[S.task_ptr[S.level_fronts[q]]];
          const long long m = (long long)front_dim(f);
          if (inpl_prev[f] >= 0) {
            const int c = inpl_prev[f], qc = slot_of[c];
            P.scratch_ld[q] = P.scratch_ld[qc];
            P.scratch_off[q] = P.scratch_off[qc] + (long long)S.f_ns[c] * bs * (P.scratch_ld[qc] + 1);
          } else {
            P.scratch_ld[q] = (int)m;
            P.scratch_off[q] = total;
            total += m * m;
          }
        }
      }
    P.scratch_max = std::max<long long>(total, 1);
    if (getenv("G2OHIP_PLAN_DUMP")) {
      int nglb = 0, nmem = 0, single = 0, rows_ne = 0, not_ident = 0;
      for (int f = 0; f < nf; ++f) {
        if (slot_of[f] < 0) continue;
        ++nglb;
        if (inpl_prev[f] >= 0) { ++nmem; continue; }
        if (S.child_off[f + 1] - S.child_off[f] != 1) continue;
        ++single;
        const int c = S.children[S.child_off[f]];
        if (S.f_ns[f] + S.f_nb[f] != S.f_nb[c]) ++rows_ne; else ++not_ident;
      }
      fprintf(stderr, "scratch-slab fronts %d, continued in place %d; single-child but not in place %d (rows differ %d, other %d); slab %.1f MB\n", nglb, nmem,
              single, rows_ne, not_ident, total * 8e-6);
    }
    // update matrices: none for a front whose parent continues in place
    bool any = false;
    for (int f = 0; f < nf; ++f) any = any || inpl_next[f] >= 0;
    if (any) {
      S.U_total = 0;
      for (int f = 0; f < nf; ++f) {
        S.U_off[f] = S.U_total;
        if (inpl_next[f] < 0) S.U_total += (long long)S.f_nb[f] * (S.f_nb[f] + 1) / 2 * bs * bs;
      }
    }
    P.stats.bytes_U = (size_t)S.U_total * 8;
  }
  if (S.level_fronts.empty()) {
    S.level_fronts.push_back(0);
    P.scratch_off.push_back(0);
    P.scratch_ld.push_back(0);
  }
}

void Planner::front_records() {
  // --- packed per-front records and per-parent extend-add descriptors
  P.recs.resize(nf);
  P.cdesc.resize(S.children.size());
  P.crel.reserve(S.rel.size());
  const int T_ = (bs % 3 == 0) ? 3 : bs;
  int tri_max = 1;
  for (int f = 0; f < nf; ++f) {
    FrontRec& R = P.recs[f];
    std::memset(&R, 0, sizeof(R));
    R.ns = S.f_ns[f];
    R.nb = S.f_nb[f];
    R.c0 = S.sn_start[f];
    R.asm_off = S.asm_off[f];
    R.asm_cnt = S.asm_off[f + 1] - S.asm_off[f];
    R.child_off = S.child_off[f];
    R.child_cnt = S.child_off[f + 1] - S.child_off[f];
    R.crel_off = (int)P.crel.size();
    R.cmap_off = (int)P.cmap.size();
    R.L_off = S.L_off[f];
    R.pad[0] = 0;   // (set below once the children are known) third child fits the three-children fast path
    R.rows_off = S.rows_off[f];
    if (S.w_off[f] > 0x7fffffffLL) throw StateFailure("symbolic: solve workspace exceeds 2^31 doubles");
    R.w_off = (int)S.w_off[f];
    R.U_off = S.U_off[f];
    for (int ch = S.child_off[f]; ch < S.child_off[f + 1]; ++ch) {
      int c = S.children[ch];
      P.cdesc[ch].U_off = S.U_off[c];
      P.cdesc[ch].nbc = S.f_nb[c];
      P.cdesc[ch].crel_start = (int)P.crel.size() - R.crel_off;
      P.cdesc[ch].cmap_start = (int)P.cmap.size() - R.cmap_off;
      P.cdesc[ch].w_off = (int)S.w_off[c];
      const int* rl = S.rel.data() + S.rel_off[c];
      P.crel.insert(P.crel.end(), rl, rl + S.f_nb[c]);
      for (int ib = 0; ib < S.f_nb[c]; ++ib)
        for (int jb = 0; jb <= ib; ++jb) {
          if (rl[ib] >= (1 << 16) || rl[jb] >= (1 << 15)) throw StateFailure("symbolic: front too large for the packed child map");
          P.cmap.push_back(rl[ib] | (rl[jb] << 16));   // packed block (ib,jb), row-major lower order
        }
      if (ch - S.child_off[f] < 2) R.ch[ch - S.child_off[f]] = P.cdesc[ch];
    }
    if (R.child_cnt == 3) {   // third child within the three-children fast path of the factor kernel (8 doubles x 256 threads)?
      const int nbc2 = P.cdesc[R.child_off + 2].nbc;
      R.pad[0] = (nbc2 * (nbc2 + 1) / 2 * bs * bs <= 8 * kFactorThreads) ? 1 : 0;
    }
    R.crel_cnt = (int)P.crel.size() - R.crel_off;
    R.cmap_cnt = (int)P.cmap.size() - R.cmap_off;
    const int nt0 = (R.nb + R.ns - 1) * bs / T_;          // trailing tiles per side after the first pivot block
    R.tri_cnt = std::max(nt0 * (nt0 + 1) / 2, R.nb * (R.nb + 1) / 2);
    tri_max = std::max(tri_max, R.tri_cnt);
  }
  P.tri.resize(tri_max);
  {
    int k = 0;
    for (int i = 0; k < tri_max; ++i)
      for (int j = 0; j <= i && k < tri_max; ++j) P.tri[k++] = i | (j << 16);
  }
  for (int ph = 0; ph < 2; ++ph)
  for (LevelLaunch& LL : P.launches[ph]) {
    LL.lds_idx_ints = LL.glb_idx_ints = LL.sm_idx_ints = 0;
    LL.lds_vec_m = 0;
    LL.lds_max_panel = 0;
    for (int q = LL.lds_begin; q < LL.glb_begin + LL.glb_count; ++q) {
      const int t = S.level_fronts[q];
      for (int k = S.task_ptr[t]; k < S.task_ptr[t + 1]; ++k) {
        const FrontRec& R = P.recs[S.task_fronts[k]];
        if (q < LL.glb_begin) LL.lds_vec_m = std::max(LL.lds_vec_m, (R.ns + R.nb) * bs);
        if (q < LL.glb_begin) LL.lds_max_panel = std::max(LL.lds_max_panel, (R.ns + R.nb) * bs * R.ns * bs + R.ns * bs);
        if (q < LL.glb_begin) {   // may the factor kernel carry the forward sweep of this launch?
          const int nthr = LL.sm_count > 0 ? 128 : kFactorThreads;
          // (any number of children, any boundary size: the fifth and later children and those with more boundary rows
          // than threads are added by a loop; one right-hand side value per thread in the pivot part)
          if (R.ns * bs > nthr) LL.fuse_fwd = false;
        }
        if (q < LL.glb_begin) LL.wv_idx_ints = std::max(LL.wv_idx_ints, (2 + kVirtInts) * R.asm_cnt + R.cmap_cnt + R.crel_cnt);
        if (q < LL.lds_begin + LL.sm_count) LL.sm_idx_ints = std::max(LL.sm_idx_ints, (2 + kVirtInts) * R.asm_cnt + R.cmap_cnt + R.tri_cnt + R.crel_cnt);
        else if (q < LL.glb_begin) LL.lds_idx_ints = std::max(LL.lds_idx_ints, (2 + kVirtInts) * R.asm_cnt + R.cmap_cnt + R.tri_cnt + R.crel_cnt);
        else LL.glb_idx_ints = std::max(LL.glb_idx_ints, (2 + kVirtInts) * R.asm_cnt);
      }
    }
  }
}

void Planner::grouped_chains() {
  // --- grouped in-place chains.  The panels of one large supernode (a chain continued in place) each made a pass over the
  // whole trailing matrix: (m - k)^2 / 2 doubles read and written per 48 columns -- 460 GB for a 20 000-row front, which is
  // what its 250 ms were.  Panels are grouped by big_group: a panel inside a group updates only the columns of the group's
  // remaining panels (what their pivot blocks and panel rows need), the group's LAST panel updates everything behind the group
  // with all the group's pivot columns at once (they are adjacent columns of the same frontal matrix).
  grp_prev.assign(nf, 0);
  grp_rem.assign(nf, 0);
  P.gtab_off.assign(nf, -1);
  if (opt.big_group > 1)
    for (int f0 = 0; f0 < nf; ++f0) {
      if (inpl_prev[f0] >= 0 || inpl_next[f0] < 0) continue;   // (chain heads only)
      if (front_dim(f0) < opt.big_group_min_rows) continue;
      std::vector<int> chain;
      for (int f = f0; f >= 0; f = inpl_next[f]) chain.push_back(f);
      for (size_t g0 = 0; g0 < chain.size(); g0 += (size_t)opt.big_group) {
        const size_t g1 = std::min(chain.size(), g0 + (size_t)opt.big_group);
        int total = 0;
        for (size_t i = g0; i < g1; ++i) total += S.f_ns[chain[i]] * bs;
        if (total >= (1 << 15)) continue;
        int before = 0;
        for (size_t i = g0; i < g1; ++i) {
          const int f = chain[i], np_ = S.f_ns[f] * bs;
          if (i + 1 == g1) grp_prev[f] = before;                 // the group's last panel: all of the group's columns
          else grp_rem[f] = total - before - np_;                // inside the group: up to the group's end
          before += np_;
        }
        // the group's last panel reads the earlier panels' solved rows from THEIR L panels (not from the frontal matrix: the fused
        // solve + update kernel leaves the raw rows there): per earlier panel (L offset low / high, rows of its front, pivot columns,
        // row of its trailing part that is row 0 of the last panel's trailing part)
        if (g1 - g0 > 1) {
          const int fl = chain[g1 - 1];
          P.gtab_off[fl] = (int)P.gtab.size();
          P.gtab.push_back((int)(g1 - g0 - 1));
          for (size_t i = g0; i + 1 < g1; ++i) {
            const int f = chain[i];
            int rowoff = 0;
            for (size_t k = i + 1; k < g1; ++k) rowoff += S.f_ns[chain[k]] * bs;
            P.gtab.push_back((int)(unsigned int)(S.L_off[f] & 0xffffffffLL));
            P.gtab.push_back((int)(S.L_off[f] >> 32));
            P.gtab.push_back((int)front_dim(f));
            P.gtab.push_back(S.f_ns[f] * bs);
            P.gtab.push_back(rowoff);
          }
        }
      }
    }
  if (P.gtab.empty()) P.gtab.push_back(0);
}

void Planner::big_tiles() {
  // --- trailing-update tiles of the scratch-slab fronts (big_front_update_kernel), per level launch
  P.cinv_slot.assign(S.level_fronts.size(), make_int2(-1, 0));   // per launch slot: (offset into cinv, ints) of the front's gather table
  for (int ph = 0; ph < 2; ++ph)
    for (LevelLaunch& LL : P.launches[ph]) {
      LL.bt_begin = (int)P.big_tiles.size();
      for (int q = LL.glb_begin; q < LL.glb_begin + LL.glb_count; ++q) {
        const int f = S.task_fronts[S.task_ptr[S.level_fronts[q]]];
        const int nt64 = (S.f_nb[f] * bs + 63) / 64;
        // w: bit 0 = update in place (the parent continues in this frontal matrix); grouped chains (grp_prev / grp_rem, below):
        // bits 1..15 = pivot columns of the group's earlier panels that ride along (the group's last panel), bits 16..31 = the
        // update stops at this column of the trailing matrix (a panel inside a group: the columns of the group's remaining panels)
        const int w = (inpl_next[f] >= 0 ? 1 : 0) | (grp_prev[f] << 1) | (grp_rem[f] << 16);
        if (grp_prev[f] > 0) LL.grouped = true;
        if (grp_rem[f] > 0) LL.group_in = true;
        const int ntc = grp_rem[f] > 0 ? std::min(nt64, (grp_rem[f] + 63) / 64) : nt64;
        for (int ti = 0; ti < nt64; ++ti)
          for (int tj = 0; tj <= std::min(ti, ntc - 1); ++tj) P.big_tiles.push_back(make_int4(q, ti, tj, w));
      }
      LL.bt_count = (int)P.big_tiles.size() - LL.bt_begin;
    }
  // --- fronts whose region is WRITTEN by the extend-add (big_extend_gather_kernel<.., true>: the children's entries or zero for every
  // lower block) instead of zero-filled, read and written: the heads of levels that run the one-launch extend-add as a whole-GPU
  // pass of its own.  Their original blocks -- and those of the fronts that continue in place behind them -- are added behind that
  // launch (LevelLaunch::la_*) instead of with everybody else's at the start of the phase.
  std::vector<char> write_head(nf, 0), late(nf, 0);
  std::vector<int> slot_of_f(nf, -1);
  for (int ph = 0; ph < 2; ++ph)
    for (LevelLaunch& LL : P.launches[ph]) {
      int max_children = 0;
      bool ok = LL.big_passes && opt.world == 1;
      for (int q = LL.glb_begin; q < LL.glb_begin + LL.glb_count; ++q) {
        const int f = S.task_fronts[S.task_ptr[S.level_fronts[q]]];
        slot_of_f[f] = q;
        max_children = std::max(max_children, S.child_off[f + 1] - S.child_off[f]);
      }
      LL.eg_write = ok && max_children >= 1 && max_children <= 7 && LL.bt_count > merge_tiles_of(LL);
      if (!LL.eg_write) continue;
      int heads = 0;
      for (int q = LL.glb_begin; q < LL.glb_begin + LL.glb_count; ++q) {
        const int f = S.task_fronts[S.task_ptr[S.level_fronts[q]]];
        if (S.child_off[f + 1] == S.child_off[f] || inpl_prev[f] >= 0) continue;
        write_head[f] = 1;
        ++heads;
        for (int g = f; g >= 0; g = inpl_next[g]) late[g] = 1;
      }
      if (heads == 0) LL.eg_write = false;   // (a level of fronts continued in place: nothing to extend-add)
    }
  for (int ph = 0; ph < 2; ++ph)
    for (LevelLaunch& LL : P.launches[ph]) {
      // zero-fill chunks of the fronts that start a region at this level
      LL.fz_begin = (int)P.big_tiles.size();
      for (int q = LL.glb_begin; q < LL.glb_begin + LL.glb_count; ++q) {
        const int f = S.task_fronts[S.task_ptr[S.level_fronts[q]]];
        if (inpl_prev[f] >= 0 || write_head[f]) continue;
        // (the lower block triangle only -- nothing uses what lies above a diagonal block: a chunk = a few columns from the first row of
        // their diagonal block down, ~kFillChunk doubles; the full squares were 5.4 GB = 1 ms per iteration of the 10 000-camera grid graph)
        const int m = (int)front_dim(f);
        for (int c0 = 0; c0 < m;) {
          const int row0 = (c0 / bs) * bs, h = m - row0;
          const int nc = std::max(1, std::min(m - c0, kFillChunk / h));
          P.big_tiles.push_back(make_int4(q, c0, nc, row0));
          c0 += nc;
        }
      }
      LL.fz_count = (int)P.big_tiles.size() - LL.fz_begin;
      // assembly chunks (32 original blocks each)
      LL.ba_begin = (int)P.big_tiles.size();
      LL.big_ok = LL.glb_count > 0;
      int max_children = 0;
      for (int q = LL.glb_begin; q < LL.glb_begin + LL.glb_count; ++q) {
        const int f = S.task_fronts[S.task_ptr[S.level_fronts[q]]];
        if (S.f_ns[f] * bs > 64) LL.big_ok = false;
        const int na = S.asm_off[f + 1] - S.asm_off[f];
        for (int e = 0; e < na && !late[f]; e += 32) P.big_tiles.push_back(make_int4(q, e, std::min(32, na - e), inpl_prev[f] >= 0 ? 1 : 0));   // w: add to what is there
        max_children = std::max(max_children, S.child_off[f + 1] - S.child_off[f]);
      }
      LL.ba_count = (int)P.big_tiles.size() - LL.ba_begin;
      if (max_children > 16) LL.big_ok = false;   // (one launch per child ordinal)
      // inverse block maps for the gather at load time (big_level_kernel): front block -> child's boundary block
      LL.gather = LL.big_ok && max_children <= kGatherChildren;
      // ... and for the extend-add of a level in ONE launch (big_extend_gather_kernel: a workgroup owns blocks of the parent and adds
      // its children's entries in child order -- one read-modify-write of the frontal matrix instead of one per child ordinal); the
      // header has room for seven children
      LL.eg_ok = LL.big_ok && (max_children >= 2 || LL.eg_write) && max_children <= 7;   // (one child per front: a pass per ordinal is one launch too -- unless it writes)
      LL.eg_begin = (int)P.big_tiles.size();
      for (int q = LL.glb_begin; q < LL.glb_begin + LL.glb_count && (LL.gather || LL.eg_ok); ++q) {
        const int f = S.task_fronts[S.task_ptr[S.level_fronts[q]]];
        const int nch = S.child_off[f + 1] - S.child_off[f], mb = S.f_ns[f] + S.f_nb[f];
        if (nch == 0 || inpl_prev[f] >= 0) continue;
        if (kGatherHeader + nch * mb > kGatherInts) LL.gather = false;   // (the merged level launch stages the table of a front in LDS)
        if (!LL.gather && !LL.eg_ok) break;
        // table: [0] children, [1 + 2 c], [2 + 2 c] offset of child c's update matrix (low, high word), [kGatherHeader + c mb + b] the maps
        const size_t t0 = P.cinv.size();
        P.cinv.resize(t0 + kGatherHeader + (size_t)nch * mb, -1);
        P.cinv[t0] = nch;
        for (int ch = S.child_off[f]; ch < S.child_off[f + 1]; ++ch) {
          const int c = S.children[ch], k0 = ch - S.child_off[f];
          P.cinv[t0 + 1 + 2 * k0] = (int)(unsigned int)(S.U_off[c] & 0xffffffffLL);
          P.cinv[t0 + 2 + 2 * k0] = (int)(S.U_off[c] >> 32);
          const int* rl = S.rel.data() + S.rel_off[c];
          for (int k = 0; k < S.f_nb[c]; ++k) P.cinv[t0 + kGatherHeader + (size_t)k0 * mb + rl[k]] = k;
        }
        P.cinv_slot[q] = make_int2((int)t0, kGatherHeader + nch * mb);
        if (LL.eg_ok) {   // chunks of lower blocks of ONE block column of the parent (consecutive rows: the stores of a chunk are contiguous per column),
                          // 256 scalar rows each: one row per thread (more per workgroup was measured slower: what the kernel lives on is requests in flight)
          const int cb = std::max(1, std::min(64, kEgThreads / bs));
          for (int jb = 0; jb < mb; ++jb)
            for (int ib = jb; ib < mb; ib += cb) P.big_tiles.push_back(make_int4(q, jb, ib, std::min(cb, mb - ib)));
        }
      }
      LL.eg_count = LL.eg_ok ? (int)P.big_tiles.size() - LL.eg_begin : 0;
      LL.eg_maxc = max_children;
      // original blocks added behind the writing extend-add: the heads of this level and the fronts continued in place behind them
      LL.la_begin = (int)P.big_tiles.size();
      for (int q = LL.glb_begin; q < LL.glb_begin + LL.glb_count && LL.eg_write; ++q) {
        const int f = S.task_fronts[S.task_ptr[S.level_fronts[q]]];
        if (!write_head[f]) continue;
        for (int g = f; g >= 0; g = inpl_next[g]) {
          const int na = S.asm_off[g + 1] - S.asm_off[g];
          for (int e = 0; e < na; e += 32) P.big_tiles.push_back(make_int4(slot_of_f[g], e, std::min(32, na - e), 1));
        }
      }
      LL.la_count = (int)P.big_tiles.size() - LL.la_begin;
      if (LL.eg_write && (!LL.eg_ok || LL.eg_count == 0)) throw StateFailure("symbolic: a level marked for the writing extend-add has no gather tables");
      // extend-add passes: pass c handles child c of every front (the children of one front may hit the same blocks)
      LL.be_pass.clear();
      for (int c = 0; c < max_children && LL.big_ok; ++c) {
        const int b0 = (int)P.big_tiles.size();
        for (int q = LL.glb_begin; q < LL.glb_begin + LL.glb_count; ++q) {
          const int f = S.task_fronts[S.task_ptr[S.level_fronts[q]]];
          if (S.child_off[f] + c >= S.child_off[f + 1] || inpl_prev[f] >= 0) continue;   // (in place: the child's update is there)
          const int nbc = S.f_nb[S.children[S.child_off[f] + c]];
          const int nblk = nbc * (nbc + 1) / 2;
          for (int b = 0; b < nblk; b += 64) P.big_tiles.push_back(make_int4(q, c, b, std::min(64, nblk - b)));
        }
        LL.be_pass.emplace_back(b0, (int)P.big_tiles.size() - b0);
      }
      // panel row chunks (256 rows below the pivot block each)
      LL.tr_begin = (int)P.big_tiles.size();
      for (int q = LL.glb_begin; q < LL.glb_begin + LL.glb_count; ++q) {
        const int f = S.task_fronts[S.task_ptr[S.level_fronts[q]]];
        const int rows = S.f_nb[f] * bs;
        for (int r = 0; r < rows; r += 256) P.big_tiles.push_back(make_int4(q, r, 0, 0));
      }
      LL.tr_count = (int)P.big_tiles.size() - LL.tr_begin;
      LL.tr_all = LL.glb_count > 0;   // every front has panel rows (big_panel_solve_kernel: a front without would have no workgroup)
      for (int q = LL.glb_begin; q < LL.glb_begin + LL.glb_count; ++q)
        if (S.f_nb[S.task_fronts[S.task_ptr[S.level_fronts[q]]]] == 0) LL.tr_all = false;
      // row chunks for the multi-workgroup sweeps (big_forward_kernel / big_backward_kernel): the chunks of a front are
      // contiguous, w = ordinal | count << 16
      LL.sw_begin = (int)P.big_tiles.size();
      bool sw_ok = LL.glb_count > 0;
      for (int q = LL.glb_begin; q < LL.glb_begin + LL.glb_count && sw_ok; ++q) {
        const int t = S.level_fronts[q];
        if (S.task_ptr[t + 1] - S.task_ptr[t] != 1 || S.f_ns[S.task_fronts[S.task_ptr[t]]] * bs > 64) sw_ok = false;
      }
      for (int q = LL.glb_begin; q < LL.glb_begin + LL.glb_count && sw_ok; ++q) {
        const int f = S.task_fronts[S.task_ptr[S.level_fronts[q]]];
        const int rows = S.f_nb[f] * bs, G = std::max(1, (rows + 255) / 256);
        for (int g = 0; g < G; ++g) P.big_tiles.push_back(make_int4(f, g * 256, std::max(0, std::min(256, rows - g * 256)), g | (G << 16)));
      }
      LL.sw_count = (int)P.big_tiles.size() - LL.sw_begin;
      sw_max = std::max(sw_max, LL.sw_count);
    }
  if (P.cinv.empty()) P.cinv.push_back(-1);
}

// merged backward launches: maximal runs of consecutive levels with scratch-slab fronts (their LDS-class fronts, chains
// included, ride along front by front: the kernel works per front, from the L panel in memory), top level first, a
// front's chunks behind those of its parent.  A waiting workgroup never blocks the one it waits for: workgroups are
// dispatched in order and the parent's come first.  Chunk word
// w = ordinal | count << 8 | (wait for the parent's flag) << 16 | (raise the own flag) << 17.
void Planner::backward_runs() {
  constexpr int kMaxMerged = 1024;
  std::vector<int> fpar(nf, -1), fgroup(nf, -1);
  for (int f = 0; f < nf; ++f)
    for (int ch = S.child_off[f]; ch < S.child_off[f + 1]; ++ch) fpar[S.children[ch]] = f;
  int merged_max = 0;
  for (int ph = 0; ph < 2; ++ph) {
    P.bw_groups[ph].clear();
    P.bw_of_level[ph].assign(nlev, -1);
    int cur = -1;
    for (int l = nlev - 1; l >= 0; --l) {
      const LevelLaunch& LL = P.launches[ph][l];
      std::vector<int4> lev;
      bool ok = LL.glb_count > 0 && opt.big_front_passes != 0;   // (levels of LDS fronts only: the dependency-driven launches)
      for (int q = LL.lds_begin; q < LL.glb_begin + LL.glb_count && ok; ++q) {
        const int t = S.level_fronts[q];
        for (int k = S.task_ptr[t + 1] - 1; k >= S.task_ptr[t] && ok; --k) {   // chain top first
          const int f = S.task_fronts[k];
          const int rows = S.f_nb[f] * bs, Gc = std::max(1, (rows + 255) / 256);
          if (S.f_ns[f] * bs > 64 || Gc > 255) ok = false;
          for (int g = 0; g < Gc && ok; ++g) lev.push_back(make_int4(f, g * 256, std::max(0, std::min(256, rows - g * 256)), g | (Gc << 8)));
        }
      }
      if (!ok || (int)lev.size() > kMaxMerged) { cur = -1; continue; }
      if (cur < 0 || P.bw_groups[ph][cur].count + (int)lev.size() > kMaxMerged || P.bw_groups[ph][cur].bottom_level != l + 1) {
        P.bw_groups[ph].push_back(BwGroup{l, l, (int)P.big_tiles.size(), 0});
        cur = (int)P.bw_groups[ph].size() - 1;
      }
      BwGroup& G = P.bw_groups[ph][cur];
      G.bottom_level = l;
      P.bw_of_level[ph][l] = cur;
      for (int4 c : lev) {
        const int f = c.x;
        fgroup[f] = ph * 65536 + cur;
        const int par = fpar[f];
        const bool wait = par >= 0 && fgroup[par] == ph * 65536 + cur;
        c.w |= (wait ? 1 << 16 : 0) | (1 << 17);
        P.big_tiles.push_back(c);
      }
      G.count = (int)P.big_tiles.size() - G.begin;
      merged_max = std::max(merged_max, G.count);
    }
    // (a group of one level gains nothing: leave it to the per-level launch)
    for (size_t gi = 0; gi < P.bw_groups[ph].size(); ++gi)
      if (P.bw_groups[ph][gi].top_level == P.bw_groups[ph][gi].bottom_level) P.bw_of_level[ph][P.bw_groups[ph][gi].top_level] = -1;
  }
  sw_max = std::max(sw_max, merged_max);
  P.n_sw_flag = ((size_t)nf + 256) & ~(size_t)255;   // (a multiple of 1 KB: one fill kernel per zeroing)
}

// phase-wide copies of the fill and assembly chunks: the regions of the slab are never reused and the original
// blocks do not depend on any child, so both passes can run once per phase instead of once per level
void Planner::hoisted_chunks() {
  for (int ph = 0; ph < 2; ++ph) {
    P.hz_begin[ph] = (int)P.big_tiles.size();
    for (LevelLaunch& LL : P.launches[ph])
      if (LL.big_passes)
        for (int i = 0; i < LL.fz_count; ++i) { const int4 c = P.big_tiles[LL.fz_begin + i]; P.big_tiles.push_back(c); }
    P.hz_count[ph] = (int)P.big_tiles.size() - P.hz_begin[ph];
    P.ha_begin[ph] = (int)P.big_tiles.size();
    for (LevelLaunch& LL : P.launches[ph]) {
      LL.hoisted = LL.big_passes;
      if (LL.hoisted)
        for (int i = 0; i < LL.ba_count; ++i) { const int4 c = P.big_tiles[LL.ba_begin + i]; P.big_tiles.push_back(c); }
    }
    P.ha_count[ph] = (int)P.big_tiles.size() - P.ha_begin[ph];
  }
  if (P.big_tiles.empty()) P.big_tiles.push_back(make_int4(0, 0, 0, 0));
  P.n_sw_part = (size_t)std::max(sw_max, 1) * 64;
  P.n_sw_cnt = (size_t)nf + 1;
}

void Planner::two_streams() {
  // --- levels split over two streams: where the streams have to wait for each other (LevelLaunch::fork / join).  The side stream
  // runs the LDS fronts of the split levels in level order, the main stream everything else: a wait is needed only where a front
  // has a child on the OTHER stream that the last wait does not cover yet (a cross-stream wait costs ~10 us on the chain of
  // whole-GPU passes even when its event fired long ago: the queue drains at the barrier packet).
  for (int ph = 0; ph < 2; ++ph) {
    auto in_phase = [&](int t) { return ph == 0 ? (S.task_owner[t] == opt.rank) : (S.task_owner[t] == -1); };
    std::vector<char> on_side(ntask, 0);
    int fork_cover = -1, join_cover = 0, nsplit = 0, nfork = 0, njoin = 0;
    for (int l = 0; l < nlev; ++l) {
      LevelLaunch& LL = P.launches[ph][l];
      LL.split_ok = LL.lds_count > 0 && LL.big_passes;
      auto child_on = [&](int q0, int q1, bool side, int since) {
        for (int q = q0; q < q1; ++q) {
          const int t = S.level_fronts[q];
          for (int k = S.task_ptr[t]; k < S.task_ptr[t + 1]; ++k) {
            const int f = S.task_fronts[k];
            for (int ch = S.child_off[f]; ch < S.child_off[f + 1]; ++ch) {
              const int ct = task_of[S.children[ch]];
              if (ct != t && in_phase(ct) && (on_side[ct] != 0) == side && task_level[ct] >= since) return true;
            }
          }
        }
        return false;
      };
      LL.join = child_on(LL.split_ok ? LL.glb_begin : LL.lds_begin, LL.glb_begin + LL.glb_count, true, join_cover);
      if (LL.join) join_cover = l;
      LL.fork = false;
      if (LL.split_ok) {
        LL.fork = fork_cover < 0 || child_on(LL.lds_begin, LL.lds_begin + LL.lds_count, false, fork_cover);
        if (LL.fork) fork_cover = l;
        for (int q = LL.lds_begin; q < LL.lds_begin + LL.lds_count; ++q) on_side[S.level_fronts[q]] = 1;
        ++nsplit;
      }
      nfork += LL.fork;
      njoin += LL.join;
    }
    if (getenv("G2OHIP_PLAN_DUMP") && nsplit > 0) fprintf(stderr, "phase %d: %d split levels, %d forks, %d joins\n", ph, nsplit, nfork, njoin);
  }
}

void Planner::factor_groups() {
  // --- factorisation launch groups.  Consecutive levels with the same kernel variant (and nothing the fused
  // kernel cannot carry) may share one launch: workgroups are dispatched in blockIdx order and the slots are in
  // level order, so every child of a waiting parent is already running or done (no deadlock); the parent
  // prefetches its tables, then spins on a device-scope counter its children bump after a release fence.
  for (int f = 0; f < nf; ++f) P.recs[f].pad[1] = 0x00ffffff;
  for (int f = 0; f < nf; ++f)
    for (int ch = S.child_off[f]; ch < S.child_off[f + 1]; ++ch) P.recs[S.children[ch]].pad[1] = f & 0x00ffffff;
  factor_order = S.level_fronts;
  for (int ph = 0; ph < 2; ++ph) {
    P.groups[ph].clear();
    auto in_phase = [&](int t) { return ph == 0 ? (S.task_owner[t] == opt.rank) : (S.task_owner[t] == -1); };
    for (int l = 0; l < nlev;) {
      FactorGroup G{P.launches[ph][l], l, l, false};
      int l1 = l + 1;
      const bool sm = G.LL.sm_count > 0, wv = G.LL.wv;
      auto plain = [](const LevelLaunch& X) { return X.glb_count == 0 && X.lds_count > 0 && X.fuse_fwd; };
      if (opt.dep_levels > 1 && nf < (1 << 24) && plain(G.LL)) {
        int end = G.LL.lds_begin + G.LL.lds_count;
        while (l1 < nlev && l1 - l < opt.dep_levels) {
          const LevelLaunch& N = P.launches[ph][l1];
          if (!plain(N) || (N.sm_count > 0) != sm || N.wv != wv || N.lds_begin != end) break;
          end += N.lds_count;
          ++l1;
        }
        // children each task of the levels (l, l1) has to wait for (those inside the group)
        std::vector<std::pair<int, int>> waits;   // (front, count)
        std::vector<int> signals;
        bool ok = l1 - l > 1;
        for (int lev = l + 1; lev < l1 && ok; ++lev) {
          const LevelLaunch& N = P.launches[ph][lev];
          for (int q = N.lds_begin; q < N.lds_begin + N.lds_count && ok; ++q) {
            const int t = S.level_fronts[q], f = S.task_fronts[S.task_ptr[t]];
            int cnt = 0;
            for (int ch = S.child_off[f]; ch < S.child_off[f + 1]; ++ch) {
              const int c = S.children[ch], ct = task_of[c];
              if (ct != t && in_phase(ct) && task_level[ct] >= l && task_level[ct] < l1) {
                ++cnt;
                signals.push_back(c);
              }
            }
            if (cnt > 127) ok = false;
            if (cnt > 0) waits.emplace_back(f, cnt);
          }
        }
        if (ok) {
          for (int lev = l + 1; lev < l1; ++lev) {
            const LevelLaunch& N = P.launches[ph][lev];
            G.LL.lds_count += N.lds_count;
            if (sm) {
              G.LL.sm_count += N.sm_count;
              G.LL.sm_max_m = std::max(G.LL.sm_max_m, N.sm_max_m);
              G.LL.sm_idx_ints = std::max(G.LL.sm_idx_ints, N.sm_idx_ints);
            } else {
              G.LL.lds_max_m = std::max(G.LL.lds_max_m, N.lds_max_m);
              G.LL.lds_idx_ints = std::max(G.LL.lds_idx_ints, N.lds_idx_ints);
            }
            G.LL.max_m = std::max(G.LL.max_m, N.max_m);
            G.LL.join = G.LL.join || N.join;
            G.LL.lds_vec_m = std::max(G.LL.lds_vec_m, N.lds_vec_m);
            G.LL.max_panel = std::max(G.LL.max_panel, N.max_panel);
            G.LL.wv_pn = std::max(G.LL.wv_pn, N.wv_pn);
            G.LL.wv_idx_ints = std::max(G.LL.wv_idx_ints, N.wv_idx_ints);
          }
          G.LL.glb_begin = G.LL.lds_begin + G.LL.lds_count;
          for (auto& w : waits) P.recs[w.first].pad[1] |= w.second << 24;
          for (int c : signals) P.recs[c].pad[1] |= (int)0x80000000u;
          // the backward sweep runs the same groups top-down: the child task (its top front c) waits for the parent front
          for (auto& w : waits) P.recs[w.first].pad[0] |= w.second << 8;
          for (int c : signals) P.recs[c].pad[0] |= 2;
          G.last_level = l1 - 1;
          G.dep = true;
        } else {
          l1 = l + 1;
        }
      }
      if (getenv("G2OHIP_PLAN_DUMP"))
        fprintf(stderr, "phase %d group: levels %d..%d tasks %d dep %d sm %d wv %d (pn %d idx %d)\n", ph, G.first_level, G.last_level, G.LL.lds_count + G.LL.glb_count,
                (int)G.dep, G.LL.sm_count, (int)G.LL.wv, G.LL.wv_pn, G.LL.wv_idx_ints);
      P.groups[ph].push_back(G);
      l = l1;
    }
  }
  P.n_ready = (size_t)std::max(nf, 1);   // dependency counters of the dependency-driven launches, per front
}

// --- band chains (band_chain.inc): leaf tasks whose rows are a band of half-width <= 4 blocks plus one border of <= 4
// blocks.  They go to the head of level 0 of their launch group and are factorised by the sliding-window kernel in a
// launch of their own in front of the group's (the parents' dependency counters are bumped the same way).
void Planner::band_chains() {
  int n_band = 0, n_leaf = 0;
  for (int ph = 0; ph < 2; ++ph)
    for (FactorGroup& G : P.groups[ph]) {
      if (G.first_level != 0 || !G.LL.wv) continue;
      const LevelLaunch& L0 = P.launches[ph][0];
      const int b0 = L0.lds_begin, cnt = L0.lds_count;
      std::vector<int> head, tail;
      std::vector<BandInfo> infos;
      for (int i = 0; i < cnt; ++i) {
        const int t = factor_order[b0 + i];
        BandInfo bi;
        ++n_leaf;
        if (try_band(t, bi)) {
          head.push_back(t);
          infos.push_back(std::move(bi));
        } else {
          tail.push_back(t);
        }
      }
      if (head.empty()) continue;
      std::copy(head.begin(), head.end(), factor_order.begin() + b0);
      std::copy(tail.begin(), tail.end(), factor_order.begin() + b0 + head.size());
      G.band_count = (int)head.size();
      G.band_rec0 = (int)P.band_rec.size();
      for (BandInfo& bi : infos) {
        bi.rec.tab_off = (int)P.band_tab.size();
        bi.rec.ent0 = (int)P.band_ent_asm.size();
        P.band_tab.insert(P.band_tab.end(), bi.tab.begin(), bi.tab.end());
        P.band_ent.insert(P.band_ent.end(), bi.ent.begin(), bi.ent.end());
        P.band_ent_asm.insert(P.band_ent_asm.end(), bi.ent_asm.begin(), bi.ent_asm.end());
        G.band_ent_cap = std::max(G.band_ent_cap, bi.rec.nent);
        G.band_tab_cap = std::max(G.band_tab_cap, bi.rec.tab_n);
        P.band_rec.push_back(bi.rec);
      }
      n_band += G.band_count;
    }
  P.stats.n_band = (size_t)n_band;
  P.stats.nnzL_band = P.stats.piv_band = 0;
  for (const BandChainRec& r : P.band_rec)
    for (int f = r.f_first; f < r.f_first + r.nfronts; ++f) {
      const size_t m = (size_t)(S.f_ns[f] + S.f_nb[f]) * bs, np = (size_t)S.f_ns[f] * bs;
      P.stats.nnzL_band += np * m - np * (np - 1) / 2;
      P.stats.piv_band += np;
    }
  if (getenv("G2OHIP_PLAN_DUMP")) {
    fprintf(stderr, "band chains rejected by rule:");
    for (int c = 0; c < 32; ++c)
      if (why_cnt[c]) fprintf(stderr, " %d:%d", c, why_cnt[c]);
    fprintf(stderr, "\n");
  }
  if (getenv("G2OHIP_PLAN_DUMP")) fprintf(stderr, "band chains: %d of %d leaf tasks (entries %zu, table ints %zu)\n", n_band, n_leaf, P.band_ent_asm.size(), P.band_tab.size());
  if (P.band_rec.empty()) {
    BandChainRec z;
    std::memset(&z, 0, sizeof(z));
    P.band_rec.push_back(z);
  }
  if (P.band_tab.empty()) P.band_tab.push_back(0);
  if (P.band_ent.empty()) P.band_ent.push_back(make_int4(0, 0, 0, 0));
}

bool Planner::try_band(int t, BandInfo& out) {
  constexpr int kMaxFr = 48, kMaxBlk = 160, kMaxEnt = 4096;
  if (bs != 6 || !opt.band_kernel) return why(1);
  const int k0 = S.task_ptr[t], k1 = S.task_ptr[t + 1];
  const int nfr = k1 - k0;
  if (nfr < 1 || nfr > kMaxFr) return why(2);
  const int f0 = S.task_fronts[k0], fl = S.task_fronts[k1 - 1];
  if (S.child_off[f0 + 1] != S.child_off[f0]) return why(3);   // a leaf of the tree
  for (int k = k0 + 1; k < k1; ++k)
    if (S.task_fronts[k] != S.task_fronts[k - 1] + 1) return why(4);
  const int base = S.sn_start[f0], nblk = S.sn_start[fl + 1] - base;
  if (nblk < 1 || nblk > kMaxBlk) return why(5);
  // boundary rows of the last front: border = those the first front has already, the rest continues the band
  const int* Bl = S.rows.data() + S.rows_off[fl];
  const int nbl = S.f_nb[fl];
  const int* B0 = S.rows.data() + S.rows_off[f0];
  const int nb0 = S.f_nb[f0];
  std::vector<int> Sset, Rset;
  for (int k = 0; k < nbl; ++k) (std::binary_search(B0, B0 + nb0, Bl[k]) && nfr > 1 ? Sset : Rset).push_back(Bl[k]);
  if (nfr == 1) {   // one front: every boundary row may be band or border; the nearest four continue the band
    Sset.clear();
    Rset.assign(Bl, Bl + nbl);
  }
  // the staying band rows in the order they are met (first column that couples to them)
  {
    std::vector<std::pair<int, int>> key;
    for (int r : Rset) {
      int first = nblk;
      for (int j = base; j < base + nblk && first == nblk; ++j)
        if (std::binary_search(st_[j].begin(), st_[j].end(), r)) first = j - base;
      key.emplace_back(first, r);
    }
    std::sort(key.begin(), key.end());
    for (size_t k = 0; k < key.size(); ++k) Rset[k] = key[k].second;
    if (nfr == 1 && Rset.size() > 4) {   // the ones met first stay band rows, the others are the border
      Sset.assign(Rset.begin() + 4, Rset.end());
      Rset.resize(4);
      std::sort(Sset.begin(), Sset.end());
    }
  }
  if (Sset.size() > 4 || Rset.size() > 4) return why(6);
  auto cls = [&](int r, int& bandblk, int& borderk) -> bool {
    bandblk = borderk = -1;
    if (r >= base && r < base + nblk) {
      bandblk = r - base;
      return true;
    }
    for (size_t k = 0; k < Rset.size(); ++k)
      if (Rset[k] == r) {
        bandblk = nblk + (int)k;
        return true;
      }
    for (size_t k = 0; k < Sset.size(); ++k)
      if (Sset[k] == r) {
        borderk = (int)k;
        return true;
      }
    return false;
  };
  for (int j = base; j < base + nblk; ++j)
    for (int i : st_[j]) {
      int bb, bk;
      if (!cls(i, bb, bk)) return why(8);
      if (bb >= 0 && bb - (j - base) > 4) {
        static int shown = 0;
        if (getenv("G2OHIP_BAND_DEBUG") && shown++ < 3) {
          fprintf(stderr, "band reject: chain of %d blocks, col %d row class %d; pivots (original ids):", nblk, j - base, bb);
          for (int q = 0; q < nblk; ++q) fprintf(stderr, " %d", S.perm[base + q]);
          fprintf(stderr, " | R:");
          for (int r : Rset) fprintf(stderr, " %d", S.perm[r]);
          fprintf(stderr, " | S:");
          for (int r : Sset) fprintf(stderr, " %d", S.perm[r]);
          fprintf(stderr, "\n");
        }
        return why(9);   // beyond the window of its column
      }
    }
  BandChainRec& R = out.rec;
  std::memset(&R, 0, sizeof(R));
  R.f_first = f0;
  R.nfronts = nfr;
  R.nblk = nblk;
  R.nS = (int)Sset.size();
  R.nR = (int)Rset.size();
  R.c0 = base;
  out.tab.clear();
  out.ent.clear();
  out.ent_asm.clear();
  std::vector<int> colfront(nblk, 0);
  for (int fi = 0; fi < nfr; ++fi) {
    const int f = f0 + fi, pb = S.sn_start[f] - base, ns = S.f_ns[f];
    const long long Loff = S.L_off[f];
    int fr[kBandFrontInts];
    fr[0] = pb;
    fr[1] = ns * bs;
    fr[2] = (int)(unsigned int)(Loff & 0xffffffffLL);
    fr[3] = (int)(Loff >> 32);
    fr[4] = (ns + S.f_nb[f]) * bs;
    for (int d = 0; d < 8; ++d) {
      const int bb = pb + d;
      int prow = -1;
      if (bb < nblk) prow = base + bb;
      else if (bb - nblk < (int)Rset.size()) prow = Rset[bb - nblk];
      fr[5 + d] = prow >= 0 ? local_pos(f, prow) : -1;
      // the kernel addresses a row that is a pivot of the chain as (band position - first pivot of the front): the band rows
      // of a front have to be contiguous (no holes in the band)
      if (bb < nblk && fr[5 + d] >= 0 && fr[5 + d] != d) return why(17);
    }
    for (int k = 0; k < 4; ++k) {
      fr[13 + k] = k < (int)Sset.size() ? local_pos(f, Sset[k]) : -1;
      if (k < (int)Sset.size() && fr[13 + k] < 0) return why(10);   // (the border is carried by every front)
    }
    out.tab.insert(out.tab.end(), fr, fr + kBandFrontInts);
    for (int c = 0; c < ns; ++c) colfront[pb + c] = fi;
    for (int e = S.asm_off[f]; e < S.asm_off[f + 1]; ++e) {
      const int pos = S.asm_pos[e], lr = pos & 0x7fff, lc = (pos >> 15) & 0x7fff;
      int bb = -1, bk = -1;
      if (lr < ns) bb = pb + lr;
      else if (!cls(S.rows[S.rows_off[f] + lr - ns], bb, bk)) return why(11);
      const int C0 = (pb + lc) * bs;
      const int R0 = bb >= 0 ? bb * bs : (0x10000 | (bk * bs));
      if (bb >= 0 && (bb < pb + lc || bb - (pb + lc) > 4)) return why(12);
      out.ent.push_back(make_int4(S.asm_q[e], pos, 0, 0));
      out.ent.push_back(make_int4(0, 0, 0, R0));
      out.ent.push_back(make_int4(C0, 0, 0, 0));
      out.ent_asm.push_back(e);
    }
  }
  const int nent = (int)out.ent_asm.size();
  if (nent > kMaxEnt) return why(13);
  R.ntiles = ((nblk + (int)Rset.size()) * bs + 15) / 16;
  // table: front records | (16-byte aligned) one record per pivot block | tile -> first record
  while (out.tab.size() % 4) out.tab.push_back(0);
  R.pad[1] = (int)out.tab.size();
  for (int cb = 0; cb < nblk; ++cb) {
    const int fi = colfront[cb];
    int fr[5];
    for (int q = 0; q < 5; ++q) fr[q] = out.tab[(size_t)kBandFrontInts * fi + q];   // (copied: the vector grows below)
    // band rows of the front that are pivots of the chain: its own pivots and the contiguous run behind them
    int nbp = 0;
    while (nbp < 8 && fr[0] + nbp < nblk && out.tab[(size_t)kBandFrontInts * fi + 5 + nbp] == nbp) ++nbp;
    out.tab.push_back(fr[2]);
    out.tab.push_back(fr[3]);
    out.tab.push_back(fr[4]);
    out.tab.push_back(fr[0] | ((fr[1]) << 8) | (fi << 16) | (nbp << 24));
  }
  // per band tile the records of the blocks with rows (border blocks: columns) in it: (source offset, -, -, -), (flags, -,
  // first row relative to the tile | border row, first column relative to the window | to the tile)
  std::vector<std::vector<int>> lists(R.ntiles);
  for (int i = 0; i < nent; ++i) {
    const int R0 = out.ent[3 * i + 1].w, C0 = out.ent[3 * i + 2].x;
    const int a = (R0 & 0x10000) ? C0 : R0;   // border entries enter with their columns, band entries with their rows
    for (int j = a / 16; j <= (a + bs - 1) / 16; ++j) {
      if (j >= R.ntiles) return why(14);
      lists[j].push_back(i);
    }
  }
  R.pad[0] = (int)out.tab.size();
  int run = 0;
  std::vector<int4> recs2;
  std::vector<int> recs_asm;
  for (int j = 0; j < R.ntiles; ++j) {
    out.tab.push_back(run);
    if ((int)lists[j].size() > 32) return why(15);   // (kBandListCap)
    run += (int)lists[j].size();
    const int lo = 16 * j;
    for (int i : lists[j]) {
      const int4 e0 = out.ent[3 * i];
      const int R0 = out.ent[3 * i + 1].w, C0 = out.ent[3 * i + 2].x;
      const bool border = (R0 & 0x10000) != 0;
      const int flags = ((e0.y >> 30) & 1) | (border ? 4 : 0) | ((!border && R0 == C0) ? 8 : 0);
      if ((long long)e0.x * bs * bs > 0x7fffff00LL) return why(16);
      recs2.push_back(make_int4(e0.x * bs * bs, 0, 0, 0));
      recs2.push_back(make_int4(flags, 0, border ? (R0 & 0xffff) : R0 - lo, border ? C0 - lo : C0 - (lo - 32)));
      recs_asm.push_back(out.ent_asm[i]);
    }
  }
  out.tab.push_back(run);
  out.ent.swap(recs2);
  out.ent_asm.swap(recs_asm);
  R.nent = run;
  R.tab_n = (int)out.tab.size();
  const int nsl = S.f_ns[fl];
  for (size_t k = 0; k < Rset.size(); ++k) R.ublk |= (local_pos(fl, Rset[k]) - nsl) << (4 * (int)k);
  for (size_t k = 0; k < Sset.size(); ++k) R.ublk |= (local_pos(fl, Sset[k]) - nsl) << (4 * (4 + (int)k));
  return true;
}

// --- backward sweep of the tree levels by groups of fronts (tree_backward_kernel).  In a dependency-driven group the levels
// above the leaf level whose fronts are all small (kTreePiv pivot columns, kTreeBnd boundary rows) are cut into groups top
// down: a root and whole levels of descendants while they fit sixteen waves (the first group of a tree is made shallower so
// that the groups below it are full: four levels of a binary tree); the fronts of the next level start groups of their own.
// Groups are listed parents first (the launch order the no-deadlock argument needs).
void Planner::tree_backward() {
  P.tb_rows = S.rows;
  if (P.tb_rows.empty()) P.tb_rows.push_back(0);
  for (int ph = 0; ph < 2; ++ph)
    for (FactorGroup& G : P.groups[ph]) {
      G.tb_grp0 = (int)P.tb_grec.size();
      G.tb_ngrp = G.tb_low = 0;
      if (!opt.tree_backward || !G.dep || !opt.dep_backward || G.LL.glb_count > 0) continue;
      auto small = [&](int f) { return S.f_ns[f] * bs <= kTreePiv && S.f_nb[f] * bs <= kTreeBnd && S.f_ns[f] > 0; };
      int lc = G.last_level + 1;
      for (int l = G.last_level; l > G.first_level; --l) {
        const LevelLaunch& N = P.launches[ph][l];
        bool ok = true;
        for (int q = N.lds_begin; q < N.lds_begin + N.lds_count && ok; ++q) {
          const int t = S.level_fronts[q];
          for (int k = S.task_ptr[t]; k < S.task_ptr[t + 1]; ++k) ok = ok && small(S.task_fronts[k]);
        }
        if (!ok) break;
        lc = l;
      }
      if (G.last_level + 1 - lc < 2) continue;
      std::vector<int> in_tree(nf, 0);
      for (int l = lc; l <= G.last_level; ++l) {
        const LevelLaunch& N = P.launches[ph][l];
        for (int q = N.lds_begin; q < N.lds_begin + N.lds_count; ++q) {
          const int t = S.level_fronts[q];
          for (int k = S.task_ptr[t]; k < S.task_ptr[t + 1]; ++k) in_tree[S.task_fronts[k]] = 1;
        }
      }
      std::vector<std::vector<int>> kids(nf);
      std::vector<int> height(nf, 0), roots;
      for (int f2 = 0; f2 < nf; ++f2) {   // (fronts are numbered children first)
        if (!in_tree[f2]) continue;
        height[f2] = std::max(height[f2], 1);
        const int pf = S.f_parent[f2];
        if (pf >= 0 && in_tree[pf]) {
          kids[pf].push_back(f2);
          height[pf] = std::max(height[pf], height[f2] + 1);
        } else {
          roots.push_back(f2);
        }
      }
      // depth of the deepest full group: the largest d with 2^d - 1 <= sixteen fronts
      constexpr int kDepth = 4;
      std::vector<int> grp_of(nf, -1), pos_of(nf, 0);
      std::vector<int> queue(roots);
      for (size_t qi = 0; qi < queue.size(); ++qi) {
        const int r = queue[qi];
        const int gid = (int)P.tb_grec.size();
        const int depth_cap = (height[r] - 1) % kDepth + 1;
        std::vector<int> level(1, r), next;
        const int first = (int)P.tb_front.size();
        int cnt = 0, nl = 0;
        while (!level.empty()) {
          for (int f2 : level) {
            grp_of[f2] = gid;
            pos_of[f2] = cnt++;
            P.tb_front.push_back(make_int2(f2, nl));
          }
          ++nl;
          next.clear();
          for (int f2 : level)
            for (int c : kids[f2]) next.push_back(c);
          if (next.empty()) break;
          if (nl >= depth_cap || cnt + (int)next.size() > kTreeWaves) {
            for (int c : next) queue.push_back(c);   // groups of their own
            break;
          }
          level.swap(next);
        }
        const int pf = S.f_parent[r];
        P.tb_grec.push_back(make_int4(first, cnt, nl, (pf >= 0 && in_tree[pf]) ? pf : -1));
      }
      G.tb_ngrp = (int)P.tb_grec.size() - G.tb_grp0;
      for (int l = G.first_level; l < lc; ++l) G.tb_low += P.launches[ph][l].lds_count;
      // what a front releases: the groups rooted below it and the tasks of the per-task launch that wait for it; where the
      // boundary values of a front come from
      std::vector<int> rel(nf, 0);
      for (int f2 = 0; f2 < nf; ++f2) {
        const int pf = S.f_parent[f2];
        if (pf < 0 || !in_tree[pf]) continue;
        if (in_tree[f2]) {
          if (grp_of[f2] != grp_of[pf]) ++rel[pf];
        } else {
          const int t = task_of[f2];
          const bool top = S.task_fronts[S.task_ptr[t + 1] - 1] == f2;
          if (top && task_level[t] >= G.first_level && task_level[t] < lc && (P.recs[f2].pad[0] & 2)) ++rel[pf];
        }
      }
      for (int e = P.tb_grec[G.tb_grp0].x; e < (int)P.tb_front.size(); ++e) {
        const int f2 = P.tb_front[e].x;
        if (rel[f2] > 0x7fffff) throw StateFailure("tree_backward: release count out of range");
        P.tb_front[e].y |= rel[f2] << 8;
        for (int j = 0; j < S.f_nb[f2]; ++j) {
          const int r = S.rows[S.rows_off[f2] + j], o = sn_of[r];
          if (grp_of[o] == grp_of[f2]) P.tb_rows[S.rows_off[f2] + j] = -1 - (pos_of[o] * kTreePiv + (r - S.sn_start[o]) * bs);
        }
      }
      if (getenv("G2OHIP_PLAN_DUMP")) {
        fprintf(stderr, "phase %d tree backward: levels %d..%d in %d groups (%d fronts), %d slots left to the per-task kernel\n", ph, lc, G.last_level,
                G.tb_ngrp, (int)P.tb_front.size() - P.tb_grec[G.tb_grp0].x, G.tb_low);
        int mx = 0;
        long long tot = 0, cnt = 0;
        std::vector<int> hist(8, 0);
        for (int l = G.first_level; l < lc; ++l)
          for (int q = P.launches[ph][l].lds_begin; q < P.launches[ph][l].lds_begin + P.launches[ph][l].lds_count; ++q) {
            const int t = S.level_fronts[q], n = S.task_ptr[t + 1] - S.task_ptr[t];
            mx = std::max(mx, n);
            tot += n;
            ++cnt;
            ++hist[std::min(7, n / 8)];
          }
        fprintf(stderr, "  tasks below: %lld, fronts per task avg %.1f max %d; by length /8:", cnt, cnt ? (double)tot / cnt : 0.0, mx);
        for (int v : hist) fprintf(stderr, " %d", v);
        fprintf(stderr, "\n");
      }
    }
  P.stats.n_tree_groups = P.tb_grec.size();
  if (P.tb_grec.empty()) P.tb_grec.push_back(make_int4(0, 0, 0, -1));
  if (P.tb_front.empty()) P.tb_front.push_back(make_int2(0, 0));
}

void Planner::exchange() {
  // --- multi-GPU exchange plan: update matrices / vectors of the subtree roots, solution mask
  long long xoff = 0;
  for (int pass = 0; pass < 2; ++pass)
    for (int t : S.xroots) {
      const int f = S.task_fronts[S.task_ptr[t + 1] - 1];
      SegCopy sc;
      sc.flags = (S.task_owner[t] == opt.rank ? 1 : 0) | (pass ? 2 : 0);
      sc.a = pass ? S.w_off[f] : S.U_off[f];
      sc.n = pass ? S.f_nb[f] * bs : S.f_nb[f] * (S.f_nb[f] + 1) / 2 * bs * bs;
      sc.b = xoff;
      xoff += sc.n;
      P.xseg.push_back(sc);
    }
  P.n_xbuf = (size_t)xoff;
  P.xmask.assign((size_t)nb * bs, 1.0);
  if (opt.world > 1)
    for (int j = 0; j < nb; ++j) {
      const int o = S.task_owner[task_of[sn_of[j]]];
      const double v = (o == opt.rank || (o == -1 && opt.rank == 0)) ? 1.0 : 0.0;
      for (int r = 0; r < bs; ++r) P.xmask[(size_t)j * bs + r] = v;
    }
}

// launch slot -> (first front, chain length) of the tasks in `order`
std::vector<int2> Planner::slots_of(const std::vector<int>& order) const {
  std::vector<int2> slots(order.size());
  for (size_t q = 0; q < slots.size(); ++q) {
    const int t = order[q];
    const int a = S.task_ptr[t], b = S.task_ptr[t + 1];
    for (int k = a + 1; k < b; ++k)
      if (S.task_fronts[k] != S.task_fronts[k - 1] + 1) throw StateFailure("symbolic: chain fronts are not consecutive");
    slots[q] = make_int2(a < b ? S.task_fronts[a] : 0, b - a);
  }
  return slots;
}

void Planner::slot_orders() {
  P.slots = slots_of(S.level_fronts);
  P.fslots = slots_of(factor_order);
  // backward sweep of a dependency-driven group: the same slots in reverse (parents before children)
  P.bslots = slots_of(std::vector<int>(S.level_fronts.rbegin(), S.level_fronts.rend()));
}

}  // namespace

CholPlan plan_cholesky(int bs, int nb, const int* colptr, const int* rowidx, const CholOptions& opt) {
  CholPlan P;
  P.opt = opt;
  P.sym.nb = nb;
  P.sym.bs = bs;
  Planner W(P, bs, nb, colptr, rowidx);
  W.order();
  W.etree_and_columns();
  W.supernodes();
  W.assembly_and_storage();
  W.tasks();
  W.partition();
  W.launch_lists();
  W.scratch_slab();
  W.front_records();
  W.grouped_chains();
  W.big_tiles();
  W.backward_runs();
  W.hoisted_chunks();
  W.two_streams();
  W.factor_groups();
  W.band_chains();
  W.tree_backward();
  W.exchange();
  W.slot_orders();
  return P;
}

}  // namespace g2ohip
