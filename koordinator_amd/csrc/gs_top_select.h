// gs_top_select.h — the selection of the top-N score table (gs_schedule_top_scores; kernels: gs_top_scores.hip): which
// entries of a pod's score row make the table, and where each one goes. Compiles for the device and for the host
// (gsx_top_select, the CPU test's driver), so the threshold and take logic the kernel runs is the logic the test holds
// to numpy.
//
// The table is the first topn candidates by (score descending, node ascending). A candidate is a node with a score
// >= 0 that is not excluded (the batch's landed nodes). From the histogram of the candidates' scores, top_cut finds
// the threshold t with count(> t) < topn <= count(>= t): every candidate above t is taken, and of those at t the
// first topn - count(> t) in node order. With fewer than topn candidates every one is taken (t = -1). top_slot gives
// a candidate's place in the node-ordered compaction from the counts of candidates before it; top_rank its final
// place among the taken entries.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define GS_TOP_HD __host__ __device__ __forceinline__
#else
#define GS_TOP_HD inline
#endif

namespace gs {

constexpr int TOP_BINS = 2048;   // scores 0..MAX_SCORE_LIMIT
constexpr int TOP_MAX = 64;      // GS_MAX_TOP_SCORES

struct TopCut {
  int32_t t;         // threshold score (-1: fewer than topn candidates, every one is taken)
  uint32_t above;    // candidates with a score > t (all taken)
  uint32_t take_at;  // candidates taken at t, the first ones in node order
};

// hist[s] = candidates with score s, s in [0, nbins)
GS_TOP_HD TopCut top_cut(const uint32_t* hist, int nbins, uint32_t topn) {
  uint32_t acc = 0;
  for (int s = nbins - 1; s >= 0; --s) {
    const uint32_t h = hist[s];
    if (acc + h >= topn) return TopCut{s, acc, topn - acc};
    acc += h;
  }
  return TopCut{-1, acc, 0u};
}

// The slot of a candidate with `score` in the node-ordered list of taken entries, or -1 when it is not taken.
// above_before / at_before: candidates before it in node order with a score > t / == t.
GS_TOP_HD int32_t top_slot(int32_t score, const TopCut& c, uint32_t above_before, uint32_t at_before) {
  const uint32_t at_taken = at_before < c.take_at ? at_before : c.take_at;
  if (score > c.t) return (int32_t)(above_before + at_taken);
  if (score == c.t && at_before < c.take_at) return (int32_t)(above_before + at_before);
  return -1;
}

// whether entry (sa, na) comes before entry (sb, nb) in the table: total descending, node ascending
GS_TOP_HD bool top_before(int32_t sa, uint32_t na, int32_t sb, uint32_t nb) { return sa > sb || (sa == sb && na < nb); }

// final place of entry i among n taken entries (distinct nodes)
GS_TOP_HD int32_t top_rank(const int16_t* score, const uint32_t* node, int n, int i) {
  int32_t r = 0;
  for (int j = 0; j < n; ++j) r += top_before(score[j], node[j], score[i], node[i]) ? 1 : 0;
  return r;
}

// whether sorted[0..n) (ascending, distinct) holds v
GS_TOP_HD bool top_excluded(const int32_t* sorted, int n, int32_t v) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (sorted[mid] < v) lo = mid + 1;
    else hi = mid;
  }
  return lo < n && sorted[lo] == v;
}

}  // namespace gs
