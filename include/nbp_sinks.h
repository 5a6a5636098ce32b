// Program sinks: products that only a later pass reads leave the chain of their own pass (nbp_api.hip: plan_sinks /
// gather_sinks; DESIGN.md 3, "Sinks").
// Host only, plain arrays, no HIP: tests/sink_plan_check.cpp compiles this header alone.
//
// A pass of a tree program is a run of stages, PROPOSALS and PRODUCTS in turn.  An UPDATE is a product descriptor with the
// proposals of the stage in front that write its inputs.  The stage list puts every update of a clique's round into the
// stage of that round, also the updates whose result nothing in the pass reads: the chain up the tree then waits, level
// by level, for work that is not on its path.  The planner names the stage each update runs in: its own, or a later SINK
// stage of the pass, where the updates that left their stages run as one launch that fills the chip.
//   * deferrable: a lane-0 product of two or more densities whose inputs that are written in the stage in front each come
//     from one lane-0 proposal which feeds it alone, and -- from that proposal stage to the end of the pass -- no other
//     descriptor reads or writes what the update writes (its output, the scratch slots of its proposals), and none writes
//     what it reads.  Such an update computes the same thing in any later stage of the pass.
//   * it leaves its stage only when the other lane-0 products of the stage are all pass-throughs (one density) and a later
//     stage of the pass reads the output of at least one of them: the chain runs through the stage, and nothing else would
//     need the launches the update rides in.
//   * sinks, two per pass: an update that waits for nothing lane 1 writes, directly or through what it reads, goes to the
//     last step in front of the first lane-0 descriptor that does (where lane 0 would idle until lane 1 is done);
//     every other update, and every update behind that step, to the last step of the pass.  No lane-1 work: the last step.
// Slots are whatever the caller numbers: nbp_api.hip keeps the points and the bandwidth of an arena slot apart (2 * slot,
// 2 * slot + 1), as it does for nbp_lane_sweep.  Passes < 0 are left alone.
#ifndef NBP_SINKS_H
#define NBP_SINKS_H
#include <cstddef>
#include <cstdint>
#include <unordered_map>
#include <unordered_set>
#include <vector>

enum { NBP_SINK_OTHER = 0, NBP_SINK_PROPOSALS = 1, NBP_SINK_PRODUCTS = 2 };
enum { NBP_SINK_TWO = 0, NBP_SINK_LAST = 1 };  // placement: two sinks per pass (above), or everything at the last step

struct nbp_sink_desc {
  // in
  int lane = 0;      // the hint: 0 or 1
  int nfactors = 0;  // products: the densities multiplied
  std::vector<int32_t> reads, writes;
  // out
  int to = -1;              // the stage it runs in: its own unless it left
  bool deferrable = false;  // products
  bool waits_lane1 = false; // reads what lane 1 wrote, directly or through the chain
  std::vector<int> props;   // a deferrable product: its proposals in the stage in front
};
struct nbp_sink_stage {
  // in
  int kind = NBP_SINK_OTHER, pass = -1;
  std::vector<nbp_sink_desc> d;
  // out
  int gained = 0;  // descriptors that came from other stages
};

static inline void nbp_sink_plan(std::vector<nbp_sink_stage> &st, int placement = NBP_SINK_TWO) {
  const int ns = (int)st.size();
  for (int s = 0; s < ns; s++) {
    st[(size_t)s].gained = 0;
    for (nbp_sink_desc &d : st[(size_t)s].d) { d.to = s; d.deferrable = d.waits_lane1 = false; d.props.clear(); }
  }
  for (int a = 0; a < ns;) {
    int b = a;
    while (b + 1 < ns && st[(size_t)b + 1].pass == st[(size_t)a].pass) b++;
    const int first = a, last = b;
    a = b + 1;
    if (st[(size_t)first].pass < 0) continue;
    auto is_step = [&](int s) { return s > first && s <= last && st[(size_t)s].kind == NBP_SINK_PRODUCTS && st[(size_t)s - 1].kind == NBP_SINK_PROPOSALS; };
    // ---- deferrable, and which stages let their deferrable updates go: one walk from the end of the pass, holding per
    // slot how many reads and writes lie in the stages not yet passed
    std::unordered_map<int32_t, int> nr, nw;
    auto count = [&](const nbp_sink_stage &g) {
      for (const nbp_sink_desc &d : g.d) {
        for (int32_t x : d.reads) nr[x]++;
        for (int32_t x : d.writes) nw[x]++;
      }
    };
    auto at = [](const std::unordered_map<int32_t, int> &m, int32_t x) { auto it = m.find(x); return it == m.end() ? 0 : it->second; };
    std::vector<char> lets_go((size_t)ns, 0);
    for (int s = last; s >= first;) {
      if (!is_step(s)) { count(st[(size_t)s--]); continue; }
      nbp_sink_stage &P = st[(size_t)s - 1], &Q = st[(size_t)s];
      // (what lies behind the step: is a pass-through's output read there?)
      std::vector<char> read_later(Q.d.size(), 0);
      for (size_t i = 0; i < Q.d.size(); i++)
        for (int32_t x : Q.d[i].writes) read_later[i] |= at(nr, x) > 0;
      count(Q);
      count(P);
      std::unordered_map<int32_t, int> writer, feeds;  // slot -> the proposal writing it (-2: several); proposal -> the product it feeds (-2: several)
      for (int k = 0; k < (int)P.d.size(); k++)
        for (int32_t x : P.d[(size_t)k].writes) { auto r = writer.emplace(x, k); if (!r.second && r.first->second != k) r.first->second = -2; }
      for (int i = 0; i < (int)Q.d.size(); i++)
        for (int32_t x : Q.d[(size_t)i].reads) {
          auto w = writer.find(x);
          if (w == writer.end() || w->second < 0) continue;
          auto r = feeds.emplace(w->second, i);
          if (!r.second && r.first->second != i) r.first->second = -2;
        }
      for (int i = 0; i < (int)Q.d.size(); i++) {
        nbp_sink_desc &q = Q.d[(size_t)i];
        if (q.lane != 0 || q.nfactors < 2) continue;
        bool ok = true;
        std::vector<int> props;
        for (int32_t x : q.reads) {
          auto w = writer.find(x);
          if (w == writer.end()) continue;  // (an input from further back: a message slot)
          if (w->second < 0 || feeds[w->second] != i || P.d[(size_t)w->second].lane != 0) { ok = false; break; }
          bool seen = false;
          for (int k : props) seen |= k == w->second;
          if (!seen) props.push_back(w->second);
        }
        if (!ok) continue;
        std::unordered_map<int32_t, int> own_r, own_w;
        auto own = [&](const nbp_sink_desc &d) {
          for (int32_t x : d.reads) own_r[x]++;
          for (int32_t x : d.writes) own_w[x]++;
        };
        own(q);
        for (int k : props) own(P.d[(size_t)k]);
        for (auto &kv : own_w) ok = ok && at(nw, kv.first) == kv.second && at(nr, kv.first) == at(own_r, kv.first);
        for (auto &kv : own_r) ok = ok && (own_w.count(kv.first) || at(nw, kv.first) == 0);
        if (!ok) continue;
        q.deferrable = true;
        q.props = props;
      }
      bool others = false, plain = true, chain = false;
      for (size_t i = 0; i < Q.d.size(); i++) {
        const nbp_sink_desc &q = Q.d[i];
        if (q.lane != 0 || q.deferrable) continue;
        others = true;
        plain = plain && q.nfactors == 1;
        chain = chain || read_later[i];
      }
      lets_go[(size_t)s] = others && plain && chain;
      s -= 2;
    }
    // ---- what waits for lane 1: one walk from the start of the pass over the slots lane 1 wrote, or that were written
    // from such a slot
    std::unordered_set<int32_t> hot;
    int first_wait = -1;  // the first stage with a lane-0 descriptor that waits for lane 1 and stays where it is
    for (int s = first; s <= last; s++) {
      nbp_sink_stage &g = st[(size_t)s];
      for (nbp_sink_desc &d : g.d) {
        d.waits_lane1 = d.lane != 0;
        for (int32_t x : d.reads) d.waits_lane1 = d.waits_lane1 || hot.count(x) > 0;
      }
      for (const nbp_sink_desc &d : g.d)
        for (int32_t x : d.writes) { if (d.waits_lane1) hot.insert(x); else hot.erase(x); }
    }
    for (int s = first; s <= last && first_wait < 0; s++) {
      const nbp_sink_stage &g = st[(size_t)s];
      for (size_t i = 0; i < g.d.size(); i++) {
        const nbp_sink_desc &d = g.d[i];
        if (d.lane != 0 || !d.waits_lane1) continue;
        bool leaves = false;  // (an update that may leave is not what lane 0 waits with)
        if (g.kind == NBP_SINK_PRODUCTS) leaves = is_step(s) && lets_go[(size_t)s] && d.deferrable;
        if (g.kind == NBP_SINK_PROPOSALS && is_step(s + 1) && lets_go[(size_t)s + 1])
          for (const nbp_sink_desc &q : st[(size_t)s + 1].d)
            if (q.deferrable)
              for (int k : q.props) leaves = leaves || k == (int)i;
        if (!leaves) { first_wait = s; break; }
      }
    }
    int sink_last = -1, sink_early = -1;
    for (int s = last; s >= first && sink_last < 0; s--)
      if (is_step(s)) sink_last = s;
    if (sink_last < 0) continue;
    if (placement == NBP_SINK_TWO && first_wait >= 0) {
      const int step_start = is_step(first_wait) ? first_wait - 1 : first_wait;
      for (int s = step_start - 1; s >= first && sink_early < 0; s--)
        if (is_step(s)) sink_early = s;
    }
    // ---- where each update runs
    for (int s = first; s <= last; s++) {
      if (!is_step(s) || !lets_go[(size_t)s]) continue;
      auto target = [&](const nbp_sink_desc &q) {
        bool waits = q.waits_lane1;
        for (int k : q.props) waits = waits || st[(size_t)s - 1].d[(size_t)k].waits_lane1;
        return (sink_early >= s && !waits) ? sink_early : sink_last;
      };
      bool keeps = false;  // a sink keeps what it holds itself, and then all of it: no update leaves beside one that stays
      for (const nbp_sink_desc &q : st[(size_t)s].d) keeps = keeps || (q.deferrable && target(q) == s);
      if (keeps) continue;
      for (nbp_sink_desc &q : st[(size_t)s].d) {
        if (!q.deferrable) continue;
        const int to = target(q);
        q.to = to;
        st[(size_t)to].gained++;
        for (int k : q.props) { st[(size_t)s - 1].d[(size_t)k].to = to - 1; st[(size_t)to - 1].gained++; }
      }
    }
  }
}
#endif
