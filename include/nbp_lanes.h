// Program lanes: the cross-lane ordering of the parts of a program (nbp_api.hip: plan_lanes / run_lanes; DESIGN.md 3, "Lanes").
// Host only, plain arrays, no HIP: tests/lane_plan_check.cpp compiles this header alone.
//
// A program with lanes is a list of PARTS in list order: the lane-0 descriptors of a stage, then its lane-1 descriptors,
// then the next stage.  Lane 0 runs its parts in list order on the library stream, lane 1 its own on the second stream.
// What one lane must wait for on the other is derived here from the slots the parts touch -- never from the hint that put
// a descriptor on a lane: a wrong hint costs time, not correctness.
#ifndef NBP_LANES_H
#define NBP_LANES_H
#include <cstddef>
#include <cstdint>
#include <unordered_map>
#include <vector>

struct nbp_lane_part {
  // in
  int stage = 0, lane = 0;
  std::vector<int32_t> reads, writes;  // slots (arena slots; pseudo slots < 0 for what lies outside the arena); a fit the part
                                       // runs is in both lists
  bool barrier = false;                // everything before it, on either lane, has happened when it starts
  // out
  std::vector<int> waits;  // parts of the OTHER lane that must have finished before this one starts: indices below its own
  bool signals = false;    // a part of the other lane waits for this one
};

// One sweep in list order.  Per slot and lane: the last part that wrote it and the last part that read it.  A part waits for
// the other lane's last writer of what it reads (read after write), and for the other lane's last writer and last reader of
// what it writes (write after write, write after read).  A lane runs its parts in order, so one wait per part is enough --
// the latest of those -- and none at all where an earlier part of the same lane already waited for that part or a later one.
static inline void nbp_lane_sweep(std::vector<nbp_lane_part> &parts) {
  struct touch { int writer[2] = {-1, -1}, reader[2] = {-1, -1}; };
  std::unordered_map<int32_t, touch> slots;
  int waited[2] = {-1, -1};  // the latest part of the other lane that lane l has waited for
  int last[2] = {-1, -1};    // the latest part of lane l
  for (int k = 0; k < (int)parts.size(); k++) {
    nbp_lane_part &p = parts[(size_t)k];
    p.waits.clear();
    const int l = p.lane ? 1 : 0, o = 1 - l;
    int need = p.barrier ? last[o] : -1;
    for (int32_t s : p.reads) {
      auto it = slots.find(s);
      if (it != slots.end() && it->second.writer[o] > need) need = it->second.writer[o];
    }
    for (int32_t s : p.writes) {
      auto it = slots.find(s);
      if (it == slots.end()) continue;
      if (it->second.writer[o] > need) need = it->second.writer[o];
      if (it->second.reader[o] > need) need = it->second.reader[o];
    }
    if (need > waited[l]) {
      p.waits.push_back(need);
      parts[(size_t)need].signals = true;
      waited[l] = need;
    }
    for (int32_t s : p.reads) slots[s].reader[l] = k;
    for (int32_t s : p.writes) slots[s].writer[l] = k;
    last[l] = k;
  }
}

// Does a happens-before path lead from part a to part b (a < b)?  Same-lane order and wait edges only: what the streams and
// events give.  reach[k] = for part k, the latest part of each lane known to have finished when k starts.
static inline std::vector<int> nbp_lane_reach(const std::vector<nbp_lane_part> &parts) {
  std::vector<int> reach(parts.size() * 2, -1);
  int last[2] = {-1, -1};
  for (int k = 0; k < (int)parts.size(); k++) {
    const int l = parts[(size_t)k].lane ? 1 : 0;
    int r[2] = {-1, -1};
    auto take = [&](int j) {  // j finished: so has everything j knew of
      if (j < 0) return;
      const int lj = parts[(size_t)j].lane ? 1 : 0;
      if (j > r[lj]) r[lj] = j;
      for (int q = 0; q < 2; q++)
        if (reach[(size_t)j * 2 + q] > r[q]) r[q] = reach[(size_t)j * 2 + q];
    };
    take(last[l]);
    for (int w : parts[(size_t)k].waits) take(w);
    reach[(size_t)k * 2] = r[0];
    reach[(size_t)k * 2 + 1] = r[1];
    last[l] = k;
  }
  return reach;
}
#endif
