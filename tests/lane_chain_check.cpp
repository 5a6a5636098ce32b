// Stand-alone check of the cross-lane sweep of include/nbp_lanes.h on stage lists with promoted chains (host only: no HIP, no
// device).  Usage: lane_chain_check <count> <seed>
// Each list is the down pass of a random tree, compiled the way nbp_tree_schedule compiles it: a clique starts when its parent
// has finished and runs one to three rounds; time step tt holds a points-only copy stage (the cliques that start: the parent's
// slot -> the clique's separator slot), a proposal stage (every running clique: its separator and frontal slots -> its
// scratch slot) and a product stage (scratch -> frontal).  In front of the pass one lane-0 part writes every slot (the up
// pass), behind it a barrier part joins the lanes.  A deep leaf and its ancestors up to some depth are on lane 1: the
// promoted chain.  Parts as nbp_api.hip cuts them: per stage the lane-0 descriptors, then the lane-1 descriptors.
//   * pure lists: nothing else is on lane 1 and nobody reads across cliques but the copies.  The chain then touches only what
//     the chain wrote since it started, so after its first part no lane-1 part may wait for a lane-0 part.
//   * mixed lists: random further hints and random further reads, wrong ones included.
// In both: every pair of parts on different lanes that conflict on a slot is ordered by a happens-before path (nbp_lane_reach),
// no wait points forward, at the own lane or at a part that does not signal, and the join covers every lane-1 part.
// Prints one summary line; exit status 1 and a message on the first violation.
#include "../include/nbp_lanes.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <unordered_set>

struct clique { int parent = -1, depth = 0, start = 0, rounds = 1; bool side = false; };

static int ordered(const std::vector<nbp_lane_part> &parts, int t, long *edges, long *conflicts) {
  const int n = (int)parts.size();
  for (int k = 0; k < n; k++)
    for (int w : parts[(size_t)k].waits) {
      ++*edges;
      if (w < 0 || w >= k || (parts[(size_t)w].lane != 0) == (parts[(size_t)k].lane != 0) || !parts[(size_t)w].signals) {
        fprintf(stderr, "list %d: part %d waits for part %d: forward, own lane or no signal\n", t, k, w);
        return 1;
      }
    }
  const std::vector<int> reach = nbp_lane_reach(parts);
  std::vector<std::unordered_set<int32_t>> R((size_t)n), W((size_t)n);
  for (int k = 0; k < n; k++) {
    R[(size_t)k].insert(parts[(size_t)k].reads.begin(), parts[(size_t)k].reads.end());
    W[(size_t)k].insert(parts[(size_t)k].writes.begin(), parts[(size_t)k].writes.end());
  }
  auto meets = [](const std::unordered_set<int32_t> &a, const std::unordered_set<int32_t> &b) {
    for (int32_t x : a)
      if (b.count(x)) return true;
    return false;
  };
  int last1 = -1;
  for (int b = 0; b < n; b++) {
    const int lb = parts[(size_t)b].lane ? 1 : 0;
    if (lb && b < n - 1) last1 = b;
    for (int a = 0; a < b; a++) {
      const int la = parts[(size_t)a].lane ? 1 : 0;
      if (la == lb || !(meets(W[(size_t)a], R[(size_t)b]) || meets(R[(size_t)a], W[(size_t)b]) || meets(W[(size_t)a], W[(size_t)b]))) continue;
      ++*conflicts;
      if (reach[(size_t)b * 2 + la] < a) {
        fprintf(stderr, "list %d: parts %d (stage %d, lane %d) and %d (stage %d, lane %d) conflict on a slot and nothing orders them\n", t, a,
                parts[(size_t)a].stage, la, b, parts[(size_t)b].stage, lb);
        return 1;
      }
    }
  }
  if (reach[(size_t)(n - 1) * 2 + 1] < last1) { fprintf(stderr, "list %d: the join does not cover lane-1 part %d\n", t, last1); return 1; }
  return 0;
}

int main(int argc, char **argv) {
  if (argc < 3) { fprintf(stderr, "usage: lane_chain_check <count> <seed>\n"); return 2; }
  const int count = atoi(argv[1]);
  std::mt19937 rng((unsigned)atoi(argv[2]));
  long edges = 0, conflicts = 0, nparts = 0, side_parts = 0, lane0_waits = 0, promoted = 0;
  for (int t = 0; t < count; t++) {
    const bool pure = t % 2 == 0;
    // a random tree, parents in front of children; slots of clique c: 3c (separator), 3c + 1 (frontal), 3c + 2 (scratch)
    const int nc = 8 + (int)(rng() % 40);
    std::vector<clique> cl((size_t)nc);
    int T = 0, deepest = 0;
    for (int c = 0; c < nc; c++) {
      cl[(size_t)c].rounds = 1 + (int)(rng() % 3);
      if (c > 0) {
        // (now and then a child of the clique in front: deep chains are what the check is about)
        cl[(size_t)c].parent = rng() % 3 ? c - 1 - (int)(rng() % (unsigned)std::min(c, 2)) : (int)(rng() % (unsigned)c);
        const clique &p = cl[(size_t)cl[(size_t)c].parent];
        cl[(size_t)c].depth = p.depth + 1;
        cl[(size_t)c].start = p.start + p.rounds;
      }
      T = std::max(T, cl[(size_t)c].start + cl[(size_t)c].rounds);
      if (cl[(size_t)c].depth > cl[(size_t)deepest].depth) deepest = c;
    }
    // the chain: the deepest clique and its ancestors of depth >= top (top >= 1: the root stays on lane 0)
    const int top = 1 + (int)(rng() % (unsigned)std::max(1, cl[(size_t)deepest].depth));
    for (int a = deepest; a >= 0 && cl[(size_t)a].depth >= top; a = cl[(size_t)a].parent) { cl[(size_t)a].side = true; promoted++; }
    if (!pure)
      for (int c = 1; c < nc; c++)
        if (rng() % 5 == 0) cl[(size_t)c].side = !cl[(size_t)c].side;  // wrong hints: they know nothing of the slots
    std::vector<nbp_lane_part> parts;
    {
      nbp_lane_part up;  // the up pass wrote everything
      up.stage = 0;
      for (int s = 0; s < 3 * nc; s++) up.writes.push_back(s);
      parts.push_back(up);
    }
    int stage = 1;
    for (int tt = 0; tt < T; tt++)
      for (int kind = 0; kind < 3; kind++, stage++) {  // copies, proposals, products
        nbp_lane_part p[2];
        bool used[2] = {false, false};
        for (int c = 0; c < nc; c++) {
          const clique &q = cl[(size_t)c];
          const int l = q.side ? 1 : 0;
          if (kind == 0) {
            if (q.start != tt || q.parent < 0) continue;
            p[l].reads.push_back(3 * q.parent + 1);
            p[l].writes.push_back(3 * c);
          } else {
            if (!(q.start <= tt && tt < q.start + q.rounds)) continue;
            if (kind == 1) {
              p[l].reads.push_back(3 * c);
              p[l].reads.push_back(3 * c + 1);
              p[l].writes.push_back(3 * c + 2);
              if (!pure && rng() % 4 == 0) p[l].reads.push_back((int32_t)(rng() % (unsigned)(3 * nc)));
            } else {
              p[l].reads.push_back(3 * c + 2);
              p[l].writes.push_back(3 * c + 1);
            }
          }
          used[l] = true;
        }
        for (int l = 0; l < 2; l++)
          if (used[l]) { p[l].stage = stage; p[l].lane = l; parts.push_back(p[l]); }
      }
    nbp_lane_part join;
    join.stage = stage;
    join.barrier = true;
    parts.push_back(join);
    nbp_lane_sweep(parts);
    if (ordered(parts, t, &edges, &conflicts)) return 1;
    bool first = true;
    for (size_t k = 0; k < parts.size(); k++) {
      if (!parts[k].lane) continue;
      side_parts++;
      if (pure && !first && !parts[k].waits.empty()) {
        fprintf(stderr, "list %d: lane-1 part %zu (stage %d) of a chain that reads only what the chain wrote waits for lane-0 part %d\n", t, k,
                parts[k].stage, parts[k].waits[0]);
        return 1;
      }
      if (pure && first && parts[k].waits.empty()) { fprintf(stderr, "list %d: the chain's first part does not wait for its parent\n", t); return 1; }
      lane0_waits += (long)parts[k].waits.size();
      first = false;
    }
    nparts += (long)parts.size();
  }
  printf("ok lists %d parts %ld lane1 %ld promoted %ld waits %ld lane1_waits %ld conflicts %ld\n", count, nparts, side_parts, promoted, edges, lane0_waits, conflicts);
  return 0;
}
