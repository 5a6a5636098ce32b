/*
 * solve_incremental.c -- the "add a pose, solve, repeat" loop through the C ABI alone (include/nbp.h + include/nbp_host.h):
 * a ContinuousEuclid(2) odometry chain is solved, grown by a few poses, its oldest poses are frozen (setfreeze!), and it
 * is solved again against the tree of the first solve (solveTree!(fg, oldtree)): cliques the old tree has already solved
 * are not up-solved again (UPRECYCLED), cliques whose variables are all frozen are left alone (MARGINALIZED).
 *
 *   gcc -O2 -Iinclude examples/solve_incremental.c -o /tmp/solve_incremental \
 *       -Lincrementalinference.jl_amd/csrc -lnbp -Wl,-rpath,$PWD/incrementalinference.jl_amd/csrc -lm
 *   /tmp/solve_incremental [nvars=24] [grow=4] [N=100]
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "nbp_host.h"

#define CHK(call)                                                                  \
  do {                                                                             \
    int rc_ = (call);                                                              \
    if (rc_ < 0) {                                                                 \
      fprintf(stderr, "%s -> %d: %s\n", #call, rc_, nbp_last_error());             \
      return 1;                                                                    \
    }                                                                              \
  } while (0)

static void gaussian_factor(nbp_factor_spec *f, int kind, int nvars, int a, int b, double mx, double my, double sigma) {
  memset(f, 0, sizeof(*f));
  f->factor_kind = kind;
  f->nvars = nvars;
  f->vars[0] = a;
  f->vars[1] = b;
  f->ncomp = 1;
  f->comp[0][0] = 1.0;
  f->comp[0][1] = mx; f->comp[0][2] = my;
  f->comp[0][4] = sigma;
  f->comp[0][4 + 3 * 1 + 1] = sigma;
}

/* poses [from, to): the odometry factor to the previous pose, and a prior every 8 poses */
static int add_poses(nbp_graph *g, int from, int to) {
  nbp_factor_spec f;
  for (int i = from; i < to; i++) {
    CHK(nbp_graph_add_variable(g, NBP_EUCLID2));
    if (i > 0) { gaussian_factor(&f, NBP_F_LINREL, 2, i - 1, i, 1.0, 1.0, 0.1); CHK(nbp_graph_add_factor(g, &f)); }
    if (i % 8 == 0) { gaussian_factor(&f, NBP_F_PRIOR, 1, i, 0, i, i, 0.1); CHK(nbp_graph_add_factor(g, &f)); }
  }
  return 0;
}

int main(int argc, char **argv) {
  const int n0 = argc > 1 ? atoi(argv[1]) : 24, grow = argc > 2 ? atoi(argv[2]) : 4, N = argc > 3 ? atoi(argv[3]) : 100;
  const int n1 = n0 + grow, nfrozen = n0 / 3;
  if (n0 < 4 || grow < 1) { fprintf(stderr, "usage: solve_incremental [nvars >= 4] [grow >= 1] [N]\n"); return 1; }
  nbp_solver_params sp;
  memset(&sp, 0, sizeof(sp));
  sp.N = N; sp.gibbs_iters = 3; sp.inflate_cycles = 3; sp.product_niter = 1; sp.upsolve = sp.downsolve = 1;
  sp.limitfixeddown = 1; /* defaultFixedLagOnTree!: the down solve does not reach the frozen variables either */
  sp.spread_nh = 3.0; sp.inflation = 5.0; sp.null_surplus_add = 0.3;
  nbp_graph *g = NULL;
  CHK(nbp_graph_create(&sp, &g));
  double *pts = calloc(2 * (size_t)N, sizeof(double)), *frozen = calloc((size_t)nfrozen * 2 * N, sizeof(double)), bw[2] = {1.0, 1.0};
  double *bel = calloc((size_t)n1 * 2 * N, sizeof(double)), *belbw = calloc((size_t)n1 * 2, sizeof(double));
  int32_t *order = malloc(sizeof(int32_t) * n1), *mainslot = malloc(sizeof(int32_t) * n1);
  nbp_tree *tree[2] = {NULL, NULL};
  int64_t updates_up[2] = {0, 0};
  int32_t rec[4] = {0, 0, 0, 0};
  double worst = 0;
  for (int pass = 0; pass < 2; pass++) {
    const int nv = pass ? n1 : n0, nold = pass ? n0 : 0;
    if (add_poses(g, nold, nv)) return 1;
    if (pass)  /* setfreeze!: the oldest third stays as the first solve left it */
      for (int v = 0; v < nfrozen; v++) CHK(nbp_graph_set_variable_flags(g, v, 1, 1));
    /* the natural order keeps the old end of the chain at the leaves: appending poses leaves those cliques as they were */
    for (int i = 0; i < nv; i++) order[i] = i;
    CHK(nbp_tree_build(g, order, nv, &tree[pass]));
    CHK(nbp_tree_recycle(tree[pass], tree[0] == tree[pass] ? NULL : tree[0], 1)); /* solveTree!(fg, oldtree) */
    const int n_slots = nbp_tree_plan_slots(tree[pass], 0);
    CHK(n_slots);
    CHK(nbp_tree_main_slots(tree[pass], mainslot, NULL));
    const int init_slots = nbp_graph_init_plan(g, 7 + pass); /* initAll!: the new poses only */
    CHK(init_slots);
    nbp_ctx *ctx = NULL; /* every solve makes its own context and uploads the beliefs it starts from */
    CHK(nbp_ctx_create(0, N, n_slots > init_slots ? n_slots : init_slots, NULL, 0, 0, &ctx));
    for (int v = 0; v < nv; v++) {
      if (v < nold) CHK(nbp_slot_write(ctx, mainslot[v], NBP_EUCLID2, bel + (size_t)v * 2 * N, belbw + 2 * v));
      else CHK(nbp_slot_write(ctx, mainslot[v], NBP_EUCLID2, pts, bw));
    }
    nbp_program *init = NULL, *prog = NULL;
    CHK(nbp_graph_init_compile(g, ctx, &init));
    CHK(nbp_program_run(init, 0, -1));
    CHK(nbp_program_destroy(init));
    CHK(nbp_tree_compile(tree[pass], ctx, 2024 + pass, &prog));
    CHK(nbp_program_run(prog, 0, -1));
    CHK(nbp_synchronize(ctx));
    nbp_tree_stats st;
    CHK(nbp_tree_get_stats(tree[pass], &st));
    updates_up[pass] = st.updates_up;
    CHK(nbp_tree_cliques_recycled(tree[pass], rec));
    for (int v = 0; v < nv; v++) {
      double *p = bel + (size_t)v * 2 * N;
      if (pass && v < nfrozen) memcpy(frozen + (size_t)v * 2 * N, p, sizeof(double) * 2 * N); /* as written */
      CHK(nbp_slot_read(ctx, mainslot[v], NBP_EUCLID2, p, belbw + 2 * v));
      if (pass && v < nfrozen && memcmp(frozen + (size_t)v * 2 * N, p, sizeof(double) * 2 * N)) {
        fprintf(stderr, "frozen x%d changed\n", v);
        return 2;
      }
      double mx = 0, my = 0;
      for (int n = 0; n < N; n++) { mx += p[2 * n]; my += p[2 * n + 1]; }
      const double e = fmax(fabs(mx / N - v), fabs(my / N - v));
      if (e > worst) worst = e;
    }
    nbp_program_destroy(prog);
    nbp_ctx_destroy(ctx);
  }
  printf("solve_incremental: %d + %d poses; second solve: %d cliques, %d marginalized, %d reused; up updates %lld -> %lld; "
         "worst posterior mean error %.3f\n", n0, grow, rec[0], rec[1], rec[2], (long long)updates_up[0], (long long)updates_up[1], worst);
  nbp_tree_destroy(tree[0]);
  nbp_tree_destroy(tree[1]);
  nbp_graph_destroy(g);
  free(order); free(mainslot); free(pts); free(frozen); free(bel); free(belbw);
  if (rec[1] + rec[2] == 0 || updates_up[1] >= updates_up[0]) { fprintf(stderr, "nothing was recycled\n"); return 4; }
  return worst < 1.5 ? 0 : 3;
}
