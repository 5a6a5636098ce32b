// Stand-alone check of the cross-lane sweep of include/nbp_lanes.h (host only: no HIP, no device).
//   lane_plan_check file <path>      parts from a text file, one per line: stage lane barrier nreads r.. nwrites w..
//   lane_plan_check random <count> <seed>   that many random stage lists with random hints, wrong ones included
// For each list: sweep, then
//   * every pair of parts on different lanes that conflict on a slot (read/write, write/read, write/write) is ordered by a
//     happens-before path through same-lane order and wait edges;
//   * no wait points forward in list order, or at a part of the same lane, or at a part that does not signal;
//   * the join (the trailing barrier part) covers every lane-1 part.
// Prints one summary line per list ("file") or one for all ("random"); exit status 1 and a message on the first violation.
#include "../include/nbp_lanes.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <unordered_set>

static int check(std::vector<nbp_lane_part> &parts, const char *what, long *edges_out, long *conflicts_out) {
  nbp_lane_sweep(parts);
  const int n = (int)parts.size();
  long edges = 0, conflicts = 0;
  for (int k = 0; k < n; k++)
    for (int w : parts[(size_t)k].waits) {
      edges++;
      if (w < 0 || w >= k) { fprintf(stderr, "%s: part %d waits for part %d, which is not in front of it\n", what, k, w); return 1; }
      if ((parts[(size_t)w].lane != 0) == (parts[(size_t)k].lane != 0)) { fprintf(stderr, "%s: part %d waits for part %d of its own lane\n", what, k, w); return 1; }
      if (!parts[(size_t)w].signals) { fprintf(stderr, "%s: part %d waits for part %d, which records nothing\n", what, k, w); return 1; }
    }
  const std::vector<int> reach = nbp_lane_reach(parts);
  std::vector<std::unordered_set<int32_t>> R((size_t)n), W((size_t)n);
  for (int k = 0; k < n; k++) {
    R[(size_t)k].insert(parts[(size_t)k].reads.begin(), parts[(size_t)k].reads.end());
    W[(size_t)k].insert(parts[(size_t)k].writes.begin(), parts[(size_t)k].writes.end());
  }
  auto meets = [](const std::unordered_set<int32_t> &a, const std::unordered_set<int32_t> &b) {
    const auto &s = a.size() < b.size() ? a : b, &l = a.size() < b.size() ? b : a;
    for (int32_t x : s)
      if (l.count(x)) return true;
    return false;
  };
  for (int b = 0; b < n; b++)
    for (int a = 0; a < b; a++) {
      const int la = parts[(size_t)a].lane ? 1 : 0, lb = parts[(size_t)b].lane ? 1 : 0;
      if (la == lb) continue;
      if (!(meets(W[(size_t)a], R[(size_t)b]) || meets(R[(size_t)a], W[(size_t)b]) || meets(W[(size_t)a], W[(size_t)b]))) continue;
      conflicts++;
      if (reach[(size_t)b * 2 + la] < a) {
        fprintf(stderr, "%s: parts %d (stage %d, lane %d) and %d (stage %d, lane %d) touch a slot, one of them writing, and nothing orders them\n", what, a,
                parts[(size_t)a].stage, la, b, parts[(size_t)b].stage, lb);
        return 1;
      }
    }
  if (n > 0 && parts[(size_t)n - 1].barrier) {
    int last1 = -1;
    for (int k = 0; k < n - 1; k++)
      if (parts[(size_t)k].lane) last1 = k;
    const int lj = parts[(size_t)n - 1].lane ? 1 : 0;
    if (lj == 0 && reach[(size_t)(n - 1) * 2 + 1] < last1) { fprintf(stderr, "%s: the join does not cover lane-1 part %d\n", what, last1); return 1; }
  }
  *edges_out += edges;
  *conflicts_out += conflicts;
  return 0;
}

int main(int argc, char **argv) {
  if (argc >= 3 && !strcmp(argv[1], "file")) {
    FILE *f = fopen(argv[2], "r");
    if (!f) { perror(argv[2]); return 2; }
    std::vector<nbp_lane_part> parts;
    int stage, lane, barrier, nr;
    while (fscanf(f, "%d %d %d %d", &stage, &lane, &barrier, &nr) == 4) {
      nbp_lane_part p;
      p.stage = stage; p.lane = lane; p.barrier = barrier != 0;
      for (int i = 0, x; i < nr && fscanf(f, "%d", &x) == 1; i++) p.reads.push_back(x);
      int nw = 0;
      if (fscanf(f, "%d", &nw) != 1) { fprintf(stderr, "%s: truncated\n", argv[2]); return 2; }
      for (int i = 0, x; i < nw && fscanf(f, "%d", &x) == 1; i++) p.writes.push_back(x);
      parts.push_back(std::move(p));
    }
    fclose(f);
    long edges = 0, conflicts = 0;
    if (check(parts, argv[2], &edges, &conflicts)) return 1;
    int n1 = 0;
    for (const nbp_lane_part &p : parts) n1 += p.lane != 0;
    printf("ok parts %zu lane1 %d waits %ld conflicts %ld\n", parts.size(), n1, edges, conflicts);
    for (size_t k = 0; k < parts.size(); k++)
      for (int w : parts[k].waits) printf("wait %zu %d\n", k, w);
    return 0;
  }
  if (argc >= 4 && !strcmp(argv[1], "random")) {
    const int count = atoi(argv[2]);
    std::mt19937 rng((unsigned)atoi(argv[3]));
    long edges = 0, conflicts = 0, nparts = 0;
    for (int t = 0; t < count; t++) {
      // a stage list over a small pool of slots, so that conflicts are common; each descriptor reads up to three slots and
      // writes one; the hint is random per descriptor (wrong on purpose: it knows nothing of the slots), in some lists
      // everything is on lane 1, in some a stage is an empty barrier
      const int nslots = 4 + (int)(rng() % 40), nstages = 1 + (int)(rng() % 30);
      const int mode = (int)(rng() % 5);  // 0: no lane 1 at all, 1: all lane 1, else mixed with probability mode / 6
      std::vector<nbp_lane_part> parts;
      for (int s = 0; s < nstages; s++) {
        if (rng() % 11 == 0) {
          nbp_lane_part b;
          b.stage = s; b.barrier = true;
          parts.push_back(b);
          continue;
        }
        nbp_lane_part p[2];
        const int nd = 1 + (int)(rng() % 12);
        for (int d = 0; d < nd; d++) {
          const int l = mode == 0 ? 0 : (mode == 1 ? 1 : ((int)(rng() % 6) < mode ? 1 : 0));
          for (int r = (int)(rng() % 4); r > 0; r--) p[l].reads.push_back((int32_t)(rng() % nslots));
          p[l].writes.push_back((int32_t)(rng() % nslots));
          p[l].stage = -2;  // (marks the lane as used)
        }
        for (int l = 0; l < 2; l++)
          if (p[l].stage == -2) { p[l].stage = s; p[l].lane = l; parts.push_back(p[l]); }
      }
      nbp_lane_part join;
      join.stage = nstages; join.barrier = true;
      parts.push_back(join);
      char what[64];
      snprintf(what, sizeof what, "random list %d", t);
      if (check(parts, what, &edges, &conflicts)) return 1;
      nparts += (long)parts.size();
    }
    printf("ok lists %d parts %ld waits %ld conflicts %ld\n", count, nparts, edges, conflicts);
    return 0;
  }
  fprintf(stderr, "usage: lane_plan_check file <path> | random <count> <seed>\n");
  return 2;
}
