// gs_debug_scores.cpp — koord-scheduler's --debug-scores table on the host:
//   gs_debug_scores_string  frameworkext/debug.go:61-109 debugScores with go-pretty's RenderMarkdown (pinned by
//                           debug_test.go TestDebugScores), as a pure function of its inputs
//   gsx_top_select          the selection of gs_top_select.h run serially over one score row, the way
//                           top_scores_kernel (gs_top_scores.hip) runs it: the CPU test's driver
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <numeric>
#include <string>
#include <vector>

#include "../../include/gpuscore.h"
#include "gs_top_select.h"

extern "C" int gs_debug_scores_string(int topn, const char* pod_ref, const char* const* node_names, uint32_t n_nodes,
                                      const char* const* plugin_names, uint32_t n_plugins, const int64_t* scores,
                                      char* buf, size_t len) {
  if (topn < 0 || !pod_ref || (n_nodes && !node_names) || (n_plugins && !plugin_names) ||
      (n_nodes && n_plugins && !scores))
    return GS_EINVAL;
  std::vector<int64_t> total(n_nodes, 0);
  for (uint32_t p = 0; p < n_plugins; ++p)
    for (uint32_t n = 0; n < n_nodes; ++n) total[n] += scores[(size_t)p * n_nodes + n];
  // sort.Slice by score descending; the fixed order: nodes of equal total keep their input order
  std::vector<uint32_t> order(n_nodes);
  std::iota(order.begin(), order.end(), 0u);
  std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return total[a] > total[b]; });
  // sort.Strings(pluginNames): bytewise
  std::vector<uint32_t> cols(n_plugins);
  std::iota(cols.begin(), cols.end(), 0u);
  std::stable_sort(cols.begin(), cols.end(), [&](uint32_t a, uint32_t b) {
    return std::string(plugin_names[a]) < std::string(plugin_names[b]);
  });
  std::string msg = "| # | Pod | Node | Score |";
  for (uint32_t c : cols) msg += std::string(" ") + plugin_names[c] + " |";
  msg += "\n| --- | --- | --- | ---:|";
  for (uint32_t c = 0; c < n_plugins; ++c) msg += " ---:|";
  const uint32_t rows = std::min<uint32_t>(n_nodes, (uint32_t)topn);
  for (uint32_t i = 0; i < rows; ++i) {
    const uint32_t n = order[i];
    msg += "\n| " + std::to_string(i) + " | " + pod_ref + " | " + node_names[n] + " | " + std::to_string(total[n]) + " |";
    for (uint32_t c : cols) msg += " " + std::to_string(scores[(size_t)c * n_nodes + n]) + " |";
  }
  if (buf && len) {
    const size_t k = msg.size() < len - 1 ? msg.size() : len - 1;
    memcpy(buf, msg.data(), k);
    buf[k] = '\0';
  }
  return (int)msg.size();
}

// One score row through the kernel's selection: the histogram of the candidates (entries >= 0 whose index is not in
// excl[0..nexcl), any order, duplicates allowed), top_cut, the node-ordered compaction by top_slot from running
// counts, top_rank. nodes / totals [topn] receive the table; returns its length, -1 for bad arguments.
extern "C" int gsx_top_select(const int16_t* row, uint32_t len, const uint32_t* excl, uint32_t nexcl, uint32_t topn,
                              uint32_t* nodes, int16_t* totals) {
  using namespace gs;
  if (!row || !nodes || !totals || topn < 1 || topn > (uint32_t)TOP_MAX || (nexcl && !excl)) return -1;
  std::vector<int32_t> land(excl, excl + nexcl);
  std::sort(land.begin(), land.end());
  land.erase(std::unique(land.begin(), land.end()), land.end());
  const int nL = (int)land.size();
  std::vector<uint32_t> hist(TOP_BINS, 0u);
  for (uint32_t i = 0; i < len; ++i)
    if (row[i] >= 0 && row[i] < TOP_BINS) ++hist[row[i]];
  for (int32_t n : land)
    if ((uint32_t)n < len && row[n] >= 0 && row[n] < TOP_BINS) --hist[row[n]];
  const TopCut cut = top_cut(hist.data(), TOP_BINS, topn);
  const int want = (int)(cut.above + cut.take_at);
  uint32_t s_node[TOP_MAX];
  int16_t s_tot[TOP_MAX];
  uint32_t above = 0, at = 0;
  for (uint32_t i = 0; i < len && want; ++i) {
    int32_t s = row[i];
    if (s >= cut.t && s >= 0 && top_excluded(land.data(), nL, (int32_t)i)) s = -1;
    if (s < 0 || s < cut.t) continue;
    const int32_t slot = top_slot(s, cut, above, at);
    if (slot >= TOP_MAX) return -1;
    if (slot >= 0) {
      s_node[slot] = i;
      s_tot[slot] = (int16_t)s;
    }
    if (s > cut.t) ++above;
    else ++at;
    if (above >= cut.above && at >= cut.take_at) break;
  }
  for (int i = 0; i < want; ++i) {
    const int32_t r = top_rank(s_tot, s_node, want, i);
    nodes[r] = s_node[i];
    totals[r] = s_tot[i];
  }
  return want;
}
