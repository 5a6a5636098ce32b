// The pair schedule of the single-precision likelihood evaluation (neg_loo_ll_f32, nbp_device.h) in one-row workgroups: every
// unordered pair of points in FULL chunks of 64 is visited once, by one lane, which adds the pair's term to its own point's
// sum and to a partner sum that travels round the wave with the partner's coordinate (DPP wave_ror:1) -- no partner atomics.
// Plain functions for host and device: tests/test_lcv_pair_schedule.py enumerates the schedule on the host.
//
// The N points split into W = N >> 6 full chunks, chunk c = the points of wave c, and at most one partial chunk.  Wave w < W
// runs nbp_lcv_blocks(W) blocks; in block b it meets chunk `chunk` at the lane offsets t = t0 .. t0 + n - 1: at offset t,
// lane l holds the partner of lane (l - t) & 63 of that chunk.
//   b = 0                 the diagonal block (w, w): t = 1 .. 32.  The first 31 offsets add to both ends; at t = 32 the pair
//                         (l, l - 32) is also the pair that lane l - 32 holds, so each of the two adds to its OWN sum only.
//   b = 1 .. KF           whole blocks (w, w + b mod W), KF = (W - 1) / 2: t = 0 .. 63
//   b = KF + 1 (even W)   the block opposite, (w, w + W / 2 mod W), shared by its two waves: the lower one runs
//                         t = 0 .. 31, the upper one t = 1 .. 32 of the mirrored block -- offsets r and 64 - r of one pair
// After the last both-ends offset `tl` the partner sum in lane l belongs to lane (l - tl) & 63 of `chunk`: it is written to
// entry nbp_lcv_slot() of LDS row b -- every (row, chunk) has exactly one writing wave -- and point i adds the rows at
// nbp_lcv_read() in the order b = 0, 1, ..
// The partial chunk stays on ordered pairs: the full waves take its points as broadcast partners (the groups of four
// from nbp_lcv_tail_group(W) on), its own wave sums over all partners.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define NBP_LCV_HD __host__ __device__ inline
#else
#define NBP_LCV_HD inline
#endif

struct nbp_lcv_block {
  int chunk;  // the chunk met
  int t0, n;  // lane offsets t0 .. t0 + n - 1
  int nboth;  // the first nboth of them add to both ends, the rest to the own sum only
};

// one row of Npad lanes, as many waves as chunks, at most four of them (rows of five waves fold their last wave; a belief of
// fewer points than its slot leaves waves without a point: both keep the ordered loop), at least one full chunk
NBP_LCV_HD bool nbp_lcv_pairs_once(int N, int Npad, int P) { return P == 1 && N >= 64 && Npad <= 256 && Npad == ((N + 63) & ~63); }
NBP_LCV_HD int nbp_lcv_full(int N) { return N >> 6; }
NBP_LCV_HD int nbp_lcv_blocks(int W) { return 1 + (W - 1) / 2 + ((W & 1) ? 0 : 1); }  // = LDS rows of 64 W partner sums
NBP_LCV_HD nbp_lcv_block nbp_lcv_block_of(int W, int w, int b) {
  nbp_lcv_block k;
  const int KF = (W - 1) / 2;
  if (b == 0) { k.chunk = w; k.t0 = 1; k.n = 32; k.nboth = 31; }
  else if (b <= KF) { k.chunk = (w + b) % W; k.t0 = 0; k.n = 64; k.nboth = 64; }
  else { const bool up = w >= W / 2; k.chunk = up ? w - W / 2 : w + W / 2; k.t0 = up ? 1 : 0; k.n = 32; k.nboth = 32; }
  return k;
}
NBP_LCV_HD int nbp_lcv_partner(int l, int t) { return (l - t) & 63; }  // the lane of `chunk` that lane l meets at offset t
// where lane l writes its travelling sum after block b (row b, the partner's own entry) and where point i reads row b
NBP_LCV_HD int nbp_lcv_slot(int W, int b, const nbp_lcv_block &k, int l) { return (b * W + k.chunk) * 64 + nbp_lcv_partner(l, k.t0 + k.nboth - 1); }
NBP_LCV_HD int nbp_lcv_read(int W, int b, int i) { return b * W * 64 + i; }
NBP_LCV_HD int nbp_lcv_tail_group(int W) { return 16 * W; }  // the first group of four of the partial chunk
// the longest chain of additions behind a point's sum: a term that enters a travelling sum at the first offset of a whole
// block, the 63 additions that follow it round the wave, and the rows added from its own on (at most nbp_lcv_blocks).  The
// own sums are four chains, the longest of (nboth - 1) / 4 + 3 additions per block and one per partial group (<= 16): at
// most 44, + 2 to join the four, + the rows -- shorter.  W <= 4: at most 66.
NBP_LCV_HD int nbp_lcv_chain(int W) { return 63 + nbp_lcv_blocks(W); }
