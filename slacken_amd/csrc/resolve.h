// resolve.h -- LowestCommonAncestor.resolveTree (S/slacken/LowestCommonAncestor.scala:91-146) and .apply (:49-78), written once for
// every serial caller: the staged classify kernel (kernels.hip), the lane kernel (lane.hip) and the Bracken window (bracken.hip); the
// wave-per-fragment form (fused.hip: resolve_intervals) keeps loops of its own and shares the tie and the lift step.
//   step 1 (:101-123)  the LCA of the map taxa with the maximal root-path score: the k-mer count of the map taxa on a taxon's root path
//   step 2 (:125-144)  from that candidate towards the root until the candidate's clade holds `required` k-mers of the map
//                      (the caller's ceil(confidence * totalKmers), :94); NONE when the root's does not
// Two forms: on the Euler-tour intervals of the taxonomy (build_tour below), with no walk of a root path except towards a tie's LCA
// and past a side branch; and by the reference's walks of parent pointers, for a taxonomy without a tour.
// Nothing here lays out memory or writes a result.  The callers hand in views:
//   map   n(), taxon(j), count(j), tin(j), tout(j), live(j): entry j of an insertion-ordered taxon -> count map (Int2IntArrayMap).
//         live(j) is false for the NONE entry a map may keep (TaxonCounts.toMap :70-81 does): NONE is on no root path and in no clade.
//   tour  node(t) -> TourNode {parent, tin, tout}            (Tour below, over the array build_tour makes)
//   walk  parent(t)                                          (Parents below)
// No HIP header: tests/test_resolve_cpu.py compiles this file alone and runs it on the host.
#pragma once
#include "layouts.h"   // SLK_HD: host and device and forced inline under hipcc, plain inline for the host compiler alone

#include <utility>
#include <vector>

#ifdef __HIPCC__
#define SLK_HD_CALL __host__ __device__ inline   // the same, left to the inliner
#else
#define SLK_HD_CALL inline
#endif

namespace slk {

// ---- the taxonomy as the resolvers read it ---------------------------------------------------------------------------------------
struct alignas(16) TourNode { uint32_t parent, tin, tout, pad; };   // one 16-byte load per taxon

// An id outside the taxonomy is a tree of its own: no parent, an interval that holds nothing else (a tour's tins are under 2^26).
SLK_HD TourNode outside_node(int32_t t) { return TourNode{0u, 0x40000000u + (uint32_t)t, 0x40000000u + (uint32_t)t, 0u}; }

struct Tour {
  const TourNode *nodes;
  int32_t ntax;
  SLK_HD TourNode node(int32_t t) const { return ((uint32_t)t < (uint32_t)ntax) ? nodes[t] : outside_node(t); }
};

SLK_HD int32_t tax_parent(const int32_t *parents, int32_t ntax, int32_t t) { return ((uint32_t)t < (uint32_t)ntax) ? parents[t] : 0; }

struct Parents {
  const int32_t *parents;
  int32_t ntax;
  SLK_HD int32_t parent(int32_t t) const { return tax_parent(parents, ntax, t); }
};

// LowestCommonAncestor.apply (:49-78) by parent walks: the first node of b's path to the root that lies on a's path; ROOT when the
// paths never meet; NONE is the identity.  Computed by levelling the depths (O(depth) loads), which finds the same node on a forest.
// (No lane reads another's: wave-uniform arguments make the loads scalar and the control flow uniform, divergent ones walk alone.)
template <class Par>
SLK_HD_CALL int32_t tax_lca(const Par &P, int32_t a, int32_t b) {
  if (a == 0 || b == 0) return b == 0 ? a : b;
  if (a == b) return a;
  int da = 0, db = 0;
  for (int32_t x = a; x != 0; x = P.parent(x)) da++;
  for (int32_t y = b; y != 0; y = P.parent(y)) db++;
  for (; da > db; da--) a = P.parent(a);
  for (; db > da; db--) b = P.parent(b);
  while (a != b && a != 0) { a = P.parent(a); b = P.parent(b); }
  return a != 0 ? a : 1;
}
SLK_HD_CALL int32_t tax_lca(const int32_t *parents, int32_t ntax, int32_t a, int32_t b) { return tax_lca(Parents{parents, ntax}, a, b); }

// ---- resolveTree on intervals ----------------------------------------------------------------------------------------------------
struct Best { int32_t taxon; uint32_t tin, tout; int32_t sum_all; };   // step 1's candidate with its interval; the map's k-mers

// LowestCommonAncestor.apply (:49-78) of the candidate b (not NONE: a caller takes the first taxon of a new maximum itself) and a
// taxon t tied with it, by intervals: b holds t -- it stays; t holds b -- t; else the first node above b whose interval holds t,
// ROOT when there is none.
template <class TourT>
SLK_HD void tie_lca(const TourT &T, Best &b, int32_t t, uint32_t tin, uint32_t tout) {
  if (b.tin <= tin && tin <= b.tout) return;
  if (tin <= b.tin && b.tin <= tout) { b.taxon = t; b.tin = tin; b.tout = tout; return; }
  int32_t x = (int32_t)T.node(b.taxon).parent;
  TourNode nx = {0u, 0u, 0u, 0u};
  while (x != 0) { nx = T.node(x); if (nx.tin <= tin && tin <= nx.tout) break; x = (int32_t)nx.parent; }
  if (x == 0) { x = 1; nx = T.node(1); }   // no common node: ROOT (:77)
  b.taxon = x; b.tin = nx.tin; b.tout = nx.tout;
}

// Step 2 past a side branch: the candidate mt becomes its parent (Taxonomy.parents), [cin, cout] that node's interval.  cur caches
// the candidate's record from one such step to the next (have_cur; a jump to a map taxon drops it).
template <class TourT>
SLK_HD void lift_parent(const TourT &T, int32_t &mt, uint32_t &cin, uint32_t &cout, TourNode &cur, bool &have_cur) {
  if (!have_cur) cur = T.node(mt);
  mt = (int32_t)cur.parent;
  if (mt != 0) { cur = T.node(mt); have_cur = true; cin = cur.tin; cout = cur.tout; }
}

// Step 1 (:101-123): a taxon's score is the count of the entries whose interval holds its tin.
template <class Map, class TourT>
SLK_HD Best resolve_best(const Map &M, const TourT &T) {
  Best b = {0, 0u, 0u, 0};
  int32_t best = 0;
  const int n = M.n();
  for (int a = 0; a < n; a++) {
    if (!M.live(a)) continue;
    const uint32_t ain = M.tin(a), aout = M.tout(a);
    int32_t score = 0;
    for (int j = 0; j < n; j++) score += (M.live(j) && M.tin(j) <= ain && ain <= M.tout(j)) ? M.count(j) : 0;
    b.sum_all += M.count(a);
    if (score > best) { b.taxon = M.taxon(a); best = score; b.tin = ain; b.tout = aout; }
    else if (score == best) tie_lca(T, b, M.taxon(a), ain, aout);
  }
  return b;
}

// Step 2 (:125-144): the taxon the candidate is lifted to, NONE when no clade holds `required`.  The clade sum only changes where
// the candidate's interval comes to hold another map taxon, and once it holds them all no ancestor can do better: the walk ends
// there (the reference goes on to the root and finds nothing).
template <class Map, class TourT>
SLK_HD int32_t resolve_lift(const Map &M, const TourT &T, const Best &b, double required) {
  int32_t mt = b.taxon;
  uint32_t cin = b.tin, cout = b.tout;
  TourNode cur = {0u, 0u, 0u, 0u};
  bool have_cur = false;
  const int n = M.n();
  while (mt != 0) {
    int32_t ms = 0;
    bool side = false;          // a map taxon outside the clade that is NOT an ancestor of the candidate
    int up = -1;                // the nearest map taxon above the candidate
    uint32_t up_in = 0;
    for (int j = 0; j < n; j++) {
      if (!M.live(j)) continue;
      const uint32_t jin = M.tin(j), jout = M.tout(j);
      const bool inside = cin <= jin && jin <= cout;
      ms += inside ? M.count(j) : 0;
      const bool above = !inside && jin <= cin && cin <= jout;
      side = side || (!inside && !above);
      if (above && (up < 0 || jin > up_in)) { up = j; up_in = jin; }   // (deeper on one root path = later in the tour)
    }
    if ((double)ms >= required) break;
    if (ms == b.sum_all) { mt = 0; break; }
    if (!side) {
      // everything left lies above the candidate, on its root path: the next clade that differs is the nearest of them
      mt = M.taxon(up); cin = up_in; cout = M.tout(up);
      have_cur = false;
    } else lift_parent(T, mt, cin, cout, cur, have_cur);
  }
  return mt;
}

// ---- resolveTree by the reference's walks (a taxonomy without a tour) ------------------------------------------------------------
// Here a map needs n(), taxon(j) and count(j) only, and a NONE entry is an entry like any other: its root path is empty.
template <class Map>
SLK_HD int32_t map_count_of(const Map &M, int32_t t) {   // Int2IntMap.get, default value 0
  const int n = M.n();
  for (int i = 0; i < n; i++) if (M.taxon(i) == t) return M.count(i);
  return 0;
}

// Step 1 (:101-123)
template <class Map, class Par>
SLK_HD int32_t resolve_walk_best(const Map &M, const Par &P) {
  int32_t maxTaxon = 0, maxScore = 0;
  const int n = M.n();
  for (int it = 0; it < n; it++) {
    const int32_t taxon = M.taxon(it);
    int32_t score = 0;
    for (int32_t node = taxon; node != 0; node = P.parent(node)) score += map_count_of(M, node);
    if (score > maxScore) { maxTaxon = taxon; maxScore = score; }
    else if (score == maxScore) maxTaxon = tax_lca(P, maxTaxon, taxon);
  }
  return maxTaxon;
}

// Step 2 (:125-144)
template <class Map, class Par>
SLK_HD int32_t resolve_walk_lift(const Map &M, const Par &P, int32_t maxTaxon, double required) {
  int32_t mt = maxTaxon;
  int32_t ms = map_count_of(M, mt);                        // :125
  const int n = M.n();
  while (mt != 0 && (double)ms < required) {               // :126-144
    ms = 0;
    for (int it = 0; it < n; it++) {
      bool in_clade = false;                               // Taxonomy.hasAncestor(taxon, mt), Taxonomy.scala:236-244
      for (int32_t x = M.taxon(it); x != 0; x = P.parent(x)) if (x == mt) { in_clade = true; break; }
      if (in_clade) ms += M.count(it);
    }
    if ((double)ms >= required) break;
    mt = P.parent(mt);
  }
  return mt;
}

// ---- the tour, built on the host -------------------------------------------------------------------------------------------------
// Per id {parent, tin, tout, 0}, tin / tout from a depth-first tour of the forest (every id whose parent is NONE is a root: ROOT,
// unused ids, the top of a detached subtree), so that "a is an ancestor-or-self of b" is tin[a] <= tin[b] <= tout[a] -- two compares
// on values that are loaded once per taxon of a read's map -- instead of a walk of b's root path: NCBI lineages are 25-40 nodes deep,
// and resolveTree asks it for every pair of map taxa and again at every step of the confidence walk.  (parents: a forest, n >= 2.)
inline std::vector<TourNode> build_tour(const int32_t *parents, int32_t n) {
  std::vector<uint32_t> first((size_t)n + 1, 0), kids;   // children of p: kids[first[p] .. first[p + 1]), in increasing id order
  for (int32_t t = 1; t < n; t++) if (parents[t] != 0) first[(size_t)parents[t] + 1]++;
  for (int32_t p = 0; p < n; p++) first[(size_t)p + 1] += first[p];
  kids.resize(first[n]);
  {
    std::vector<uint32_t> at(first.begin(), first.end() - 1);
    for (int32_t t = 1; t < n; t++) if (parents[t] != 0) kids[at[parents[t]]++] = (uint32_t)t;
  }
  std::vector<TourNode> nodes((size_t)n, TourNode{0u, 0u, 0u, 0u});
  std::vector<std::pair<uint32_t, uint32_t>> stack;   // (node, next child)
  uint32_t clock = 0;
  for (int32_t r = 1; r < n; r++) {
    if (parents[r] != 0) continue;
    stack.emplace_back((uint32_t)r, first[r]);
    nodes[r].tin = ++clock;
    while (!stack.empty()) {
      auto &top = stack.back();
      if (top.second < first[(size_t)top.first + 1]) {
        const uint32_t c = kids[top.second++];
        nodes[c].parent = top.first;
        nodes[c].tin = ++clock;
        stack.emplace_back(c, first[c]);
      } else {
        nodes[top.first].tout = clock;   // the largest tin of the subtree
        stack.pop_back();
      }
    }
  }
  return nodes;
}

}  // namespace slk
