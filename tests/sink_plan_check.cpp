// Stand-alone check of the sink planner of include/nbp_sinks.h (host only: no HIP, no device).
//   sink_plan_check file <path> [placement]   a stage list from a text file: per stage a line "S kind pass ndesc", then per
//                                             descriptor a line "lane nfactors nreads r.. nwrites w.."
//   sink_plan_check random <count> <seed>     that many random stage lists: levels of cliques with pass-through chains, products
//                                             nothing reads, lane-1 cliques, scratch slots used twice, stray copies
// For each list: plan, then
//   * the original order and the planned order are interpreted symbolically (a slot holds the descriptor that last wrote it;
//     the descriptors of a stage read what lay there when the stage began): every read of every descriptor must see the same
//     writer in both, and every slot must end with the same writer;
//   * a descriptor that moved lands behind its own stage, inside its pass, proposals one stage in front of their product,
//     and in front of the first reader of what it writes;
//   * no update leaves a stage that keeps a lane-0 product of two or more densities; only lane-0 updates move; passes < 0
//     are untouched.
// "file" prints the plan ("def S i", "to S i T", "gained S n"); exit status 1 and a message on the first violation.
#include "../include/nbp_sinks.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <random>

typedef std::vector<nbp_sink_stage> stage_list;

// -> per descriptor (in list order) the writers it saw, and the final writer of every slot
static void interpret(const stage_list &st, bool planned, std::vector<std::vector<long>> &saw, std::map<int32_t, long> &end) {
  std::vector<size_t> base(st.size() + 1, 0);
  for (size_t s = 0; s < st.size(); s++) base[s + 1] = base[s] + st[s].d.size();
  saw.assign(base[st.size()], {});
  std::vector<std::vector<std::pair<int, int>>> runs(st.size());  // stage -> (stage, descriptor) it runs
  for (size_t s = 0; s < st.size(); s++)
    for (size_t i = 0; i < st[s].d.size(); i++) runs[(size_t)(planned ? st[s].d[i].to : (int)s)].push_back({(int)s, (int)i});
  end.clear();
  for (size_t s = 0; s < st.size(); s++) {
    for (auto &si : runs[s]) {
      const nbp_sink_desc &d = st[(size_t)si.first].d[(size_t)si.second];
      std::vector<long> &v = saw[base[(size_t)si.first] + (size_t)si.second];
      for (int32_t x : d.reads) { auto it = end.find(x); v.push_back(it == end.end() ? -1 : it->second); }
    }
    // (the reads above all saw the state at the start of the stage: `end` is written only now)
    for (auto &si : runs[s])
      for (int32_t x : st[(size_t)si.first].d[(size_t)si.second].writes) end[x] = (long)(base[(size_t)si.first] + (size_t)si.second);
  }
}

static int check(stage_list &st, int placement, const char *what, long *moved_out, long *early_out, long *deferrable_out) {
  nbp_sink_plan(st, placement);
  const int ns = (int)st.size();
  std::vector<std::vector<long>> saw0, saw1;
  std::map<int32_t, long> end0, end1;
  interpret(st, false, saw0, end0);
  for (int s = 0; s < ns; s++)
    for (size_t i = 0; i < st[(size_t)s].d.size(); i++) {
      const int to = st[(size_t)s].d[i].to;
      if (to < s || to >= ns || st[(size_t)to].pass != st[(size_t)s].pass || st[(size_t)to].kind != st[(size_t)s].kind) {
        fprintf(stderr, "%s: descriptor %zu of stage %d goes to stage %d\n", what, i, s, to);
        return 1;
      }
      for (int t = s; t <= to; t++)
        if (st[(size_t)t].pass != st[(size_t)s].pass) { fprintf(stderr, "%s: descriptor %zu of stage %d leaves its pass\n", what, i, s); return 1; }
    }
  interpret(st, true, saw1, end1);
  if (saw0 != saw1) {
    for (size_t k = 0; k < saw0.size(); k++)
      if (saw0[k] != saw1[k]) { fprintf(stderr, "%s: descriptor %zu (in list order) reads another writer's value in the planned order\n", what, k); break; }
    return 1;
  }
  if (end0 != end1) { fprintf(stderr, "%s: a slot ends with another writer in the planned order\n", what); return 1; }
  long moved = 0, early = 0, deferrable = 0;
  int last_sink = -1;
  for (int s = 0; s < ns; s++) {
    nbp_sink_stage &g = st[(size_t)s];
    int gained = 0;
    for (int t = 0; t < s; t++)
      for (const nbp_sink_desc &d : st[(size_t)t].d) gained += d.to == s;
    if (gained != g.gained) { fprintf(stderr, "%s: stage %d says it gained %d descriptors, %d came\n", what, s, g.gained, gained); return 1; }
    if (g.kind != NBP_SINK_PRODUCTS) {
      if (g.kind != NBP_SINK_PROPOSALS || s + 1 >= ns || st[(size_t)s + 1].kind != NBP_SINK_PRODUCTS)
        for (const nbp_sink_desc &d : g.d)
          if (d.to != s) { fprintf(stderr, "%s: a descriptor of stage %d, neither proposal nor product, moved\n", what, s); return 1; }
      continue;
    }
    bool left = false, keeps = false;
    for (size_t i = 0; i < g.d.size(); i++) {
      const nbp_sink_desc &q = g.d[i];
      deferrable += q.deferrable;
      if (q.to == s) { keeps = keeps || (q.lane == 0 && q.nfactors >= 2); continue; }
      left = true;
      moved++;
      if (q.to > last_sink) last_sink = q.to;
      if (g.pass < 0 || q.lane != 0 || q.nfactors < 2 || !q.deferrable) { fprintf(stderr, "%s: product %zu of stage %d moved, which may not\n", what, i, s); return 1; }
      for (int k : q.props) {
        const nbp_sink_desc &pr = st[(size_t)s - 1].d[(size_t)k];
        if (pr.to != q.to - 1 || pr.lane != 0) { fprintf(stderr, "%s: proposal %d of stage %d does not run in front of its product\n", what, k, s - 1); return 1; }
      }
      // the first reader of what it writes, its own product's reads of its proposals apart: behind the stage it runs in
      for (int t = s + 1; t < ns; t++)
        for (const nbp_sink_desc &d : st[(size_t)t].d) {
          if (d.to != t) continue;  // (a moved descriptor reads nothing a moved descriptor writes: the interpretation above holds that)
          for (int32_t x : d.reads)
            for (int32_t w : q.writes)
              if (x == w && t <= q.to) { fprintf(stderr, "%s: product %zu of stage %d lands in stage %d, at or behind its reader in stage %d\n", what, i, s, q.to, t); return 1; }
        }
    }
    if (left && keeps) { fprintf(stderr, "%s: an update left stage %d, which keeps a lane-0 product of two or more densities\n", what, s); return 1; }
    // a proposal moves only with its product
    for (size_t k = 0; s > 0 && st[(size_t)s - 1].kind == NBP_SINK_PROPOSALS && k < st[(size_t)s - 1].d.size(); k++) {
      const nbp_sink_desc &pr = st[(size_t)s - 1].d[k];
      if (pr.to == s - 1) continue;
      bool owned = false;
      for (const nbp_sink_desc &q : g.d)
        for (int j : q.props) owned = owned || (j == (int)k && q.to == pr.to + 1);
      if (!owned) { fprintf(stderr, "%s: proposal %zu of stage %d moved without a product\n", what, k, s - 1); return 1; }
    }
  }
  for (int s = 0; s < ns; s++)
    if (st[(size_t)s].kind == NBP_SINK_PRODUCTS)
      for (const nbp_sink_desc &q : st[(size_t)s].d) early += q.to != s && q.to < last_sink && st[(size_t)q.to].pass == st[(size_t)last_sink].pass;
  *moved_out += moved;
  *early_out += early;
  *deferrable_out += deferrable;
  return 0;
}

int main(int argc, char **argv) {
  if (argc >= 3 && !strcmp(argv[1], "file")) {
    FILE *f = fopen(argv[2], "r");
    if (!f) { perror(argv[2]); return 2; }
    const int placement = argc >= 4 ? atoi(argv[3]) : NBP_SINK_TWO;
    stage_list st;
    char tag[8];
    int kind, pass, nd;
    while (fscanf(f, "%7s %d %d %d", tag, &kind, &pass, &nd) == 4) {
      if (strcmp(tag, "S")) { fprintf(stderr, "%s: expected a stage line\n", argv[2]); return 2; }
      nbp_sink_stage g;
      g.kind = kind; g.pass = pass;
      for (int i = 0; i < nd; i++) {
        nbp_sink_desc d;
        int nr = 0, nw = 0;
        if (fscanf(f, "%d %d %d", &d.lane, &d.nfactors, &nr) != 3) { fprintf(stderr, "%s: truncated\n", argv[2]); return 2; }
        for (int k = 0, x; k < nr && fscanf(f, "%d", &x) == 1; k++) d.reads.push_back(x);
        if (fscanf(f, "%d", &nw) != 1) { fprintf(stderr, "%s: truncated\n", argv[2]); return 2; }
        for (int k = 0, x; k < nw && fscanf(f, "%d", &x) == 1; k++) d.writes.push_back(x);
        g.d.push_back(std::move(d));
      }
      st.push_back(std::move(g));
    }
    fclose(f);
    long moved = 0, early = 0, deferrable = 0;
    if (check(st, placement, argv[2], &moved, &early, &deferrable)) return 1;
    printf("ok stages %zu deferrable %ld moved %ld early %ld\n", st.size(), deferrable, moved, early);
    for (size_t s = 0; s < st.size(); s++) {
      if (st[s].gained) printf("gained %zu %d\n", s, st[s].gained);
      for (size_t i = 0; i < st[s].d.size(); i++) {
        if (st[s].d[i].deferrable) printf("def %zu %zu\n", s, i);
        if (st[s].d[i].to != (int)s) printf("to %zu %zu %d\n", s, i, st[s].d[i].to);
      }
    }
    return 0;
  }
  if (argc >= 4 && !strcmp(argv[1], "random")) {
    const int count = atoi(argv[2]);
    std::mt19937 rng((unsigned)atoi(argv[3]));
    long moved = 0, early = 0, deferrable = 0, nstages = 0;
    auto coin = [&](int one_in) { return rng() % (unsigned)one_in == 0; };
    for (int t = 0; t < count; t++) {
      stage_list st;
      int32_t fresh = 0;
      std::vector<int32_t> all;  // every slot named so far
      auto slot = [&]() { all.push_back(fresh); return fresh++; };
      auto any = [&]() { return all.empty() ? slot() : all[rng() % all.size()]; };
      const int npasses = 1 + (int)(rng() % 3);
      const bool lanes = !coin(4);
      for (int ps = 0; ps < npasses; ps++) {
        const int pass = coin(5) ? -1 : ps;
        std::vector<int32_t> msgs;
        const int nsteps = 2 + (int)(rng() % 9);
        for (int step = 0; step < nsteps; step++) {
          nbp_sink_stage P, Q;
          P.kind = NBP_SINK_PROPOSALS; Q.kind = NBP_SINK_PRODUCTS;
          P.pass = Q.pass = pass;
          std::vector<int32_t> next;
          auto msg = [&]() { return msgs.empty() || coin(8) ? any() : msgs[rng() % msgs.size()]; };
          const int ncl = 1 + (int)(rng() % 6);
          for (int c = 0; c < ncl; c++) {
            const int lane = lanes && coin(5) ? 1 : 0;
            auto update = [&](int F, int32_t out) {
              nbp_sink_desc q;
              q.lane = lane; q.nfactors = F;
              for (int j = 0; j < F; j++) {
                if (F > 1 && coin(6)) { q.reads.push_back(msg()); continue; }  // an input from further back
                nbp_sink_desc pr;
                pr.lane = coin(40) ? 1 - lane : lane;
                pr.reads.push_back(msg());
                if (coin(3)) pr.reads.push_back(msg());
                const int32_t scratch = coin(12) ? any() : slot();  // (sometimes a slot that is in use: the planner must see it)
                pr.writes.push_back(scratch);
                q.reads.push_back(scratch);
                P.d.push_back(std::move(pr));
              }
              q.writes.push_back(out);
              Q.d.push_back(std::move(q));
            };
            for (int k = (int)(rng() % 3); k > 0; k--) {  // pass-throughs: the chain
              const int32_t out = slot();
              update(1, out);
              next.push_back(out);
            }
            if (!coin(3)) {  // the frontal: mostly read by nothing in this pass
              const int32_t out = coin(10) ? any() : slot();
              update(2 + (int)(rng() % 2), out);
              if (coin(4)) next.push_back(out);
            }
          }
          st.push_back(std::move(P));
          st.push_back(std::move(Q));
          if (coin(9)) {  // a stray stage of copies
            nbp_sink_stage X;
            X.pass = pass;
            for (int k = 1 + (int)(rng() % 3); k > 0; k--) {
              nbp_sink_desc d;
              d.reads.push_back(any());
              d.writes.push_back(coin(2) ? any() : slot());
              X.d.push_back(std::move(d));
            }
            st.push_back(std::move(X));
          }
          for (int32_t m : msgs)
            if (coin(3)) next.push_back(m);
          msgs = next;
        }
        nbp_sink_stage turn;  // between two passes: everything is read (whole-slot copies)
        turn.pass = -1;
        for (int k = 0; k < 4 && !all.empty(); k++) {
          nbp_sink_desc d;
          d.reads.push_back(any());
          d.writes.push_back(slot());
          turn.d.push_back(std::move(d));
        }
        st.push_back(std::move(turn));
      }
      char what[64];
      snprintf(what, sizeof what, "random list %d", t);
      if (check(st, t % 4 == 3 ? NBP_SINK_LAST : NBP_SINK_TWO, what, &moved, &early, &deferrable)) return 1;
      nstages += (long)st.size();
    }
    printf("ok lists %d stages %ld deferrable %ld moved %ld early %ld\n", count, nstages, deferrable, moved, early);
    return 0;
  }
  fprintf(stderr, "usage: sink_plan_check file <path> [placement] | random <count> <seed>\n");
  return 2;
}
