// gs_top_scores.hip — the top-N score table of every scored pod (gs_schedule_top_scores; koord-scheduler's
// --debug-scores N, frameworkext/debug.go debugScores): the N best feasible nodes of a pod at the pod's turn, by
// (total descending, node ascending), each with its three plugin scores.
//
// For pod p of batch b every node the batch did not land on has, in the slot's score row S[p][*], its exact total at
// p's turn (the row holds the batch-start score, and such a node did not change during the batch), and in the mirror
// after b's commit its exact state at p's turn (DESIGN 6g's argument). Only b's landed nodes (<= 128) differ:
//   top_scores_kernel         behind the batch's commit on its stream, one workgroup per committed pod: the batch's
//                             distinct landed nodes sorted in LDS; pass 1 over S[p][0..N) with 16-byte loads into an LDS
//                             histogram of the scores, the landed nodes taken out of it; the threshold (top_cut); pass 2,
//                             an order-preserving compaction of the nodes above the threshold and the first ones at it
//                             (a prefix sum of per-thread counts within a wave, the waves' sums through LDS); wave 0
//                             rank-sorts the <= 64 entries, and its lanes evaluate eval_pair on their node's mirror row
//                             for the plugin scores (policy nodes through the NUMA path)
//   top_scores_landed_kernel  the batch's landed nodes, from host-derived versions of their rows as they were at each
//                             scored pod's turn (the diagnosis' slab: the kernel reads nothing else); the host merges
//                             these <= 128 entries into the pod's list and cuts at N
// The threshold and take logic is gs_top_select.h, which the CPU test drives through gsx_top_select.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gs_eval_dev.h"
#include "gs_top_select.h"

namespace gs {

static_assert(TOP_MAX == GS_MAX_TOP_SCORES && TOP_MAX == 64, "one wave's lanes");
static_assert(TOP_BINS == MAX_SCORE_LIMIT + 1, "one bin per score");
static_assert(sizeof(gs_top_score) == 12, "gs_top_score layout");
constexpr int TOP_THREADS = 256, TOP_WAVES = TOP_THREADS / 64;

__global__ void __launch_bounds__(TOP_THREADS) top_scores_kernel(TopArgs a) {
  __shared__ uint32_t s_hist[TOP_BINS];
  __shared__ int32_t s_land[MAX_BATCH];            // the batch's distinct landed nodes, ascending
  __shared__ int32_t s_raw[MAX_BATCH];
  __shared__ uint32_t s_wcnt[2][TOP_WAVES];        // per iteration parity and wave: candidates above | at the threshold << 16
  __shared__ uint32_t s_node[TOP_MAX];
  __shared__ int16_t s_tot[TOP_MAX];
  __shared__ TopCut s_cut;
  __shared__ int s_nl;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int p = blockIdx.x;
  const int nc = min(a.committed[0], a.npods);
  if (p >= nc) return;   // a voided pass, or a pod the pass did not commit
  uint32_t* const cnt_out = reinterpret_cast<uint32_t*>(a.top);
  gs_top_score* const rows_out = reinterpret_cast<gs_top_score*>(a.top + TOP_COUNT_BYTES) + (size_t)p * TOP_MAX;
  if (a.out[p].node < 0) {   // no feasible node: no table
    if (tid == 0) cnt_out[p] = 0;
    return;
  }
  // the batch's landed nodes, distinct and sorted: a node's first landing keeps it, its rank is its place
  for (int t = tid; t < TOP_BINS; t += TOP_THREADS) s_hist[t] = 0;
  if (tid < MAX_BATCH) s_raw[tid] = tid < nc ? a.out[tid].node : -1;
  if (tid == 0) s_nl = 0;
  __syncthreads();
  const int32_t mine = tid < MAX_BATCH ? s_raw[tid] : -1;
  bool first = mine >= 0;
  for (int k = 0; k < tid && k < nc; ++k) first = first && s_raw[k] != mine;
  __syncthreads();
  if (tid < MAX_BATCH && !first) s_raw[tid] = -1;
  __syncthreads();
  if (first) {
    int rank = 0;
    for (int k = 0; k < nc; ++k) {
      const int32_t v = s_raw[k];
      rank += (v >= 0 && v < mine) ? 1 : 0;
    }
    s_land[rank] = mine;   // ok: rank < distinct landed nodes <= nc <= MAX_BATCH
    atomicAdd(&s_nl, 1);
  }
  __syncthreads();
  const int nL = s_nl;
  const int16_t* __restrict__ row = a.S + (size_t)p * a.ld;
  // pass 1: the histogram of the row's scores. 8 entries per load; the row's stride ld is a multiple of 8 and >= N, so
  // a load that starts below N stays inside the row, and entries at or past N (the -1 padding) are never counted
  for (uint32_t base = (uint32_t)tid * 8u; base < a.N; base += TOP_THREADS * 8u) {
    const uint4 v = *reinterpret_cast<const uint4*>(row + base);
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int32_t s = (int16_t)(w[e >> 1] >> ((e & 1) * 16));
      if (base + e < a.N && s >= 0 && s < a.nbins) atomicAdd(&s_hist[s], 1u);
    }
  }
  __syncthreads();
  if (tid < nL) {   // the landed nodes leave it: their rows changed within the batch (the landed pass)
    const int32_t s = row[s_land[tid]];   // ok: a landed node is < N
    if (s >= 0 && s < a.nbins) atomicSub(&s_hist[s], 1u);
  }
  __syncthreads();
  if (tid == 0) s_cut = top_cut(s_hist, a.nbins, a.topn);   // (no score lies above the profile's maximum)
  __syncthreads();
  const TopCut cut = s_cut;
  const uint32_t want = cut.above + cut.take_at;   // <= topn <= TOP_MAX
  // pass 2: the taken entries in node order. Each iteration covers 2,048 consecutive nodes: a thread 8 of them (one
  // 16-byte load), a wave 512; a thread's counts of entries above / at the threshold (packed: 16 bits each, <= 512 per
  // wave) are prefix-summed over the wave's lanes, and the waves' sums go through LDS
  uint32_t run_above = 0, run_at = 0;
  int it = 0;
  for (uint32_t base = 0; base < a.N && want; base += TOP_THREADS * 8u, ++it) {
    const uint32_t i0 = base + (uint32_t)tid * 8u;
    uint32_t w[4] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
    if (i0 < a.N) {   // (inside the row, as in pass 1)
      const uint4 v = *reinterpret_cast<const uint4*>(row + i0);
      w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
    }
    int32_t sv[8];
    uint32_t mine = 0;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      int32_t s = (int16_t)(w[e >> 1] >> ((e & 1) * 16));
      if (i0 + e >= a.N) s = -1;
      if (s >= cut.t && s >= 0 && top_excluded(s_land, nL, (int32_t)(i0 + e))) s = -1;
      sv[e] = s;
      if (s >= 0 && s > cut.t) mine += 1u;
      else if (s >= 0 && s == cut.t) mine += 1u << 16;
    }
    const uint32_t incl = (uint32_t)wave_incl_scan((int)mine);   // (all 64 lanes are active here)
    if (lane == 63) s_wcnt[it & 1][wave] = incl;
    __syncthreads();
    uint32_t before = incl - mine, all = 0;
#pragma unroll
    for (int w2 = 0; w2 < TOP_WAVES; ++w2) {
      const uint32_t c2 = s_wcnt[it & 1][w2];
      if (w2 < wave) before += c2;
      all += c2;
    }
    uint32_t before_above = run_above + (before & 0xFFFFu), before_at = run_at + (before >> 16);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int32_t s = sv[e];
      if (s < 0 || s < cut.t) continue;
      const int32_t slot = top_slot(s, cut, before_above, before_at);
      if (slot >= 0 && slot < TOP_MAX) {
        s_node[slot] = i0 + e;
        s_tot[slot] = (int16_t)s;
      }
      if (s > cut.t) ++before_above;
      else ++before_at;
    }
    run_above += all & 0xFFFFu;
    run_at += all >> 16;
    if (run_above >= cut.above && run_at >= cut.take_at) break;   // (block-uniform: every thread holds the same sums)
  }
  __syncthreads();
  if (wave != 0) return;
  // wave 0: the entries' final order, and each lane's node evaluated on its mirror row for the plugin scores
  const int n = (int)want;
  const bool ok = lane < n;
  const uint32_t node = ok ? s_node[lane] : (n ? s_node[0] : 0u);   // ok: a taken node is < N; N >= 1
  const int16_t tot = ok ? s_tot[lane] : (int16_t)0;
  const int32_t rank = ok ? top_rank(s_tot, s_node, n, lane) : 0;
  Row r;
  load_row(a.m, node, true, (a.pf.enabled & 0x30u) != 0, r);
  const PairOut o = eval_pair<false, false, true>(r, a.pods[p], a.pf, a.m);
  if (ok) {
    gs_top_score t;
    t.node = node;
    t.total = tot;
    t.plugin[GS_PLUGIN_FIT] = (int16_t)o.fit;
    t.plugin[GS_PLUGIN_LOADAWARE] = (int16_t)o.la;
    t.plugin[GS_PLUGIN_NUMA] = (int16_t)o.numa;
    rows_out[rank] = t;   // ok: rank < n <= TOP_MAX
  }
  if (lane == 0) cnt_out[p] = (uint32_t)n;
}

__global__ void __launch_bounds__(MAX_BATCH) top_scores_landed_kernel(MirrorView slab, const PodVec* __restrict__ pods,
                                                                      Profile pf, const uint16_t* __restrict__ vidx,
                                                                      int nL, TopLanded* __restrict__ out) {
  const int f = blockIdx.x, tid = threadIdx.x;
  const bool ok = tid < nL;
  const uint32_t ver = ok ? vidx[(size_t)f * nL + tid] : vidx[(size_t)f * nL];
  Row row;
  load_row(slab, ver, true, (pf.enabled & 0x30u) != 0, row);   // row.node = ver: the scalar slots come from the slab too
  const PairOut o = eval_pair<false, false, true>(row, pods[f], pf, slab);
  if (ok) {
    TopLanded t;
    t.total = (int16_t)total_score(o, pf);
    t.plugin[GS_PLUGIN_FIT] = (int16_t)o.fit;
    t.plugin[GS_PLUGIN_LOADAWARE] = (int16_t)o.la;
    t.plugin[GS_PLUGIN_NUMA] = (int16_t)o.numa;
    out[(size_t)f * nL + tid] = t;   // ok: tid < nL
  }
}

hipError_t launch_top_scores(const TopArgs& a, hipStream_t st) {
  if (a.npods < 1 || a.npods > MAX_BATCH || !a.N || a.ld < a.N || (a.ld & 7u) || a.topn < 1 || a.topn > TOP_MAX || !a.top ||
      !a.S || a.nbins < 1 || a.nbins > TOP_BINS)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(top_scores_kernel, dim3(a.npods), dim3(TOP_THREADS), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_top_scores_landed(const MirrorView& slab, const PodVec* pods, const Profile& pf, const uint16_t* vidx,
                                    int nF, int nL, TopLanded* out, hipStream_t st) {
  if (nF < 1 || nF > MAX_BATCH || nL < 1 || nL > MAX_BATCH || !out) return hipErrorInvalidValue;
  hipLaunchKernelGGL(top_scores_landed_kernel, dim3(nF), dim3(MAX_BATCH), 0, st, slab, pods, pf, vidx, nL, out);
  return hipGetLastError();
}

hipError_t preload_top_scores() {
  hipFuncAttributes at;
  const void* const fn[] = {(const void*)top_scores_kernel, (const void*)top_scores_landed_kernel};
  for (const void* f : fn)
    if (hipError_t e = hipFuncGetAttributes(&at, f)) return e;
  return hipSuccess;
}

}  // namespace gs
