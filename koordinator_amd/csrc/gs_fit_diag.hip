// gs_fit_diag.hip — the FitError diagnosis of gs_schedule_diag: for a pod no node can hold, the histogram over all
// nodes of the status the Filter chain gives each node at the pod's turn ([upstream] schedule_one.go
// findNodesThatFitPod's Diagnosis.NodeToStatusMap, summed per reason as framework/types.go FitError.Error() does).
//
// A pod that finds no node assumes nothing, so for pod p of batch b every node the batch did not land on has, in the
// mirror after the batch's commit, exactly its state at p's turn:
//   fit_diag_kernel         behind the batch's commit on its stream: those nodes, from the mirror. <NUMA, false>: every
//                           node without a NUMA topology policy (row in registers, the pods wave-uniform, as
//                           eval_kernel); <true, true>: the policy nodes through the shard's index list (as
//                           eval_numa_kernel)
//   fit_diag_landed_kernel  the batch's landed nodes (<= 128), from host-derived versions of their rows as they were
//                           at each such pod's turn (a slab of its own: the kernel reads nothing else)
// Lanes classify a pair's failure code into gs_fit_reason counters (RunFilterPlugins stops at the first failing
// plugin: Fit's reasons each, else LoadAware's one, else NodeNUMAResource's), the workgroup sums them in LDS, and one
// 32-bit atomic add per (workgroup, pod, non-zero counter) reaches the pod's counters: integer adds, so the result does
// not depend on the order.
//
// The status map (gs_schedule_diag_nodes; the MAP instantiations): the same passes also store each counted pair's
// status word, the wide pass at words[row][node] (row: the pod's rank among the pass's pods with no node, in queue
// order — lanes of one wave hold consecutive nodes, so a wave stores 128 consecutive bytes per pod), the landed pass
// at words[pod][version lane]. The counters-only instantiations hold none of this.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "gs_eval_dev.h"

namespace gs {

// the counters (bits: gs_fit_reason, DIAG_FAILED) one pair's failure code adds to; scalar_fail: bit s = the pod's
// request of scalar slot s (3..6) exceeds the node's free amount
__device__ __forceinline__ uint32_t fit_reason_bits(uint32_t code, uint32_t scalar_fail) {
  if (!code) return 0u;
  uint32_t b = 1u << DIAG_FAILED;
  if (code & 0x1Fu) b |= (code & 0xFu) | ((scalar_fail >> 3) & 0xFu) << GS_FR_FIT_SCALAR0;
  else if (code & GS_FAIL_LOADAWARE) b |= 1u << (GS_FR_LA_CPU + ((code >> 10) & 3u));
  else b |= 1u << (GS_FR_NUMA0 + ((code & GS_FAIL_NUMA_MASK) >> GS_FAIL_NUMA_SHIFT));
  return b;
}

// the status word of one pair (gs_status_map): the bits of the first failing plugin, as fit_reason_bits chooses it, and
// with GS_FAIL_FIT_SCALAR the short slots 3..6 in bits 12..15
__device__ __forceinline__ uint32_t status_word(uint32_t code, uint32_t scalar_fail) {
  if (code & 0x1Fu) return (code & 0x1Fu) | ((scalar_fail >> 3) & 0xFu) << 12;
  if (code & GS_FAIL_LOADAWARE) return code & (GS_FAIL_LOADAWARE | GS_FAIL_LA_MEMORY | GS_FAIL_LA_AGGREGATED);
  return code & GS_FAIL_NUMA_MASK;
}

// which requested scalar slots of pod p the row `node` of m is short of (eval_pair's GS_FAIL_FIT_SCALAR, per slot)
__device__ __forceinline__ uint32_t scalar_fail_bits(const MirrorView& m, uint32_t node, const PodVec& p) {
  uint32_t f = 0;
  for (int s = 3; s < 7; ++s)
    if ((p.scalar_mask >> s & 1u) && p.req[s] > m.c64(C_FREE_CPU + s)[node]) f |= 1u << s;
  return f;
}

// bits of every lane of the wave summed into cnt[DIAG_WORDS] (LDS): one ballot and one LDS add per counter any lane
// holds. All 64 lanes must be active.
__device__ __forceinline__ void diag_count(uint32_t bits, uint32_t* cnt, int lane) {
  uint32_t any = (uint32_t)wave_or((int)bits);
  while (any) {
    const int b = __ffs((int)any) - 1;
    any &= any - 1;
    const unsigned long long bal = __ballot((bits >> b) & 1u);
    if (lane == 0) atomicAdd(&cnt[b], (uint32_t)__popcll(bal));
  }
}

template <bool NUMA, bool POLICY, bool MAP = false>
__global__ void __launch_bounds__(256) fit_diag_kernel(std::conditional_t<MAP, DiagMapArgs, DiagArgs> a) {
  __shared__ int s_land[MAX_BATCH], s_fpod[MAX_BATCH], s_n[2];
  __shared__ uint32_t s_cnt[MAX_BATCH * DIAG_WORDS];
  const int tid = threadIdx.x;
  const int nc = a.force0 ? 1 : min(a.committed[0], a.npods);
  if (nc <= 0) return;   // a voided pass, or nothing committed
  if (tid < 2) s_n[tid] = 0;
  __syncthreads();
  if (MAP) {
    // s_fpod in queue order (f is the pod's row): the pods sit on the lanes of waves 0 and 1; a pod's rank is the
    // count of such pods below its lane, plus wave 0's count for wave 1
    static_assert(MAX_BATCH == 128, "two waves of placement lanes");
    const int node = (tid < nc && !a.force0) ? a.out[tid].node : -1;
    const unsigned long long bal = __ballot(tid < nc && node < 0);
    if (tid == 0) s_n[0] = __popcll(bal);
    __syncthreads();
    if (tid < nc) {
      if (node < 0) s_fpod[__popcll(bal & ((1ull << (tid & 63)) - 1ull)) + (tid >= 64 ? s_n[0] : 0)] = tid;
      else s_land[atomicAdd(&s_n[1], 1)] = node;
    }
    __syncthreads();
    if (tid == 64) s_n[0] += __popcll(bal);
  } else if (tid < nc) {
    const int node = a.force0 ? -1 : a.out[tid].node;
    if (node < 0) s_fpod[atomicAdd(&s_n[0], 1)] = tid;
    else s_land[atomicAdd(&s_n[1], 1)] = node;
  }
  __syncthreads();
  const int nF = s_n[0], nL = s_n[1];
  if (!nF) return;
  for (int t = tid; t < nF * DIAG_WORDS; t += 256) s_cnt[t] = 0;
  uint32_t i = blockIdx.x * 256 + tid;
  bool ok;
  if (POLICY) {
    ok = i < a.numa_n;
    i = a.numa_idx[ok ? i : 0];
  } else {
    ok = i < a.N;
    if (!ok) i = 0;
  }
  Row row;
  load_row(a.m, i, false, NUMA, row);
  // (nodes with a NUMA topology policy: the <true, true> launch)
  if (NUMA && !POLICY && ((row.nr.nflags >> NF_POLICY_SHIFT) & 3u)) ok = false;
  for (int j = 0; j < nL; ++j)
    if (s_land[j] == (int)i) ok = false;   // its row changed within the batch: the landed pass
  Profile pf = a.pf;
  if (!NUMA) pf.enabled &= ~0x30u;
  __syncthreads();
  for (int f = 0; f < nF; ++f) {
    const int k = __builtin_amdgcn_readfirstlane(s_fpod[f]);
    const PodVec& p = a.pods[k];
    const PairOut o = eval_pair<false, false, POLICY>(row, p, pf, a.m);
    uint32_t bits = 0;
    if (ok) {
      const uint32_t sf = (o.code & GS_FAIL_FIT_SCALAR) ? scalar_fail_bits(a.m, i, p) : 0u;
      bits = fit_reason_bits(o.code, sf);
      if constexpr (MAP) a.words[(size_t)f * a.npad + i] = (uint16_t)status_word(o.code, sf);   // ok: i < N <= npad
    }
    diag_count(bits, s_cnt + f * DIAG_WORDS, tid & 63);
  }
  __syncthreads();
  for (int t = tid; t < nF * DIAG_WORDS; t += 256) {
    const uint32_t v = s_cnt[t];
    if (v) atomicAdd(&a.diag[(size_t)s_fpod[t / DIAG_WORDS] * DIAG_WORDS + t % DIAG_WORDS], v);
  }
}

template <bool MAP>
__device__ __forceinline__ void fit_diag_landed(const MirrorView& slab, const PodVec* __restrict__ pods, const Profile& pf,
                                                const uint16_t* __restrict__ vidx, int nL, uint32_t* __restrict__ out,
                                                uint16_t* __restrict__ words) {
  __shared__ uint32_t s_cnt[DIAG_WORDS];
  const int f = blockIdx.x, tid = threadIdx.x;
  if (tid < DIAG_WORDS) s_cnt[tid] = 0;
  __syncthreads();
  const bool ok = tid < nL;
  const uint32_t ver = ok ? vidx[(size_t)f * nL + tid] : vidx[(size_t)f * nL];
  Row row;
  load_row(slab, ver, false, (pf.enabled & 0x30u) != 0, row);   // row.node = ver: the scalar slots come from the slab too
  const PodVec& p = pods[f];
  const PairOut o = eval_pair<false, false, true>(row, p, pf, slab);
  uint32_t bits = 0;
  if (ok) {
    const uint32_t sf = (o.code & GS_FAIL_FIT_SCALAR) ? scalar_fail_bits(slab, ver, p) : 0u;
    bits = fit_reason_bits(o.code, sf);
    if constexpr (MAP) words[(size_t)f * nL + tid] = (uint16_t)status_word(o.code, sf);   // ok: tid < nL
  }
  diag_count(bits, s_cnt, tid & 63);
  __syncthreads();
  if (tid < DIAG_WORDS) out[(size_t)f * DIAG_WORDS + tid] = s_cnt[tid];
}

__global__ void __launch_bounds__(MAX_BATCH) fit_diag_landed_kernel(MirrorView slab, const PodVec* __restrict__ pods,
                                                                    Profile pf, const uint16_t* __restrict__ vidx, int nL,
                                                                    uint32_t* __restrict__ out) {
  fit_diag_landed<false>(slab, pods, pf, vidx, nL, out, nullptr);
}

__global__ void __launch_bounds__(MAX_BATCH) fit_diag_landed_map_kernel(MirrorView slab, const PodVec* __restrict__ pods,
                                                                        Profile pf, const uint16_t* __restrict__ vidx,
                                                                        int nL, uint32_t* __restrict__ out,
                                                                        uint16_t* __restrict__ words) {
  fit_diag_landed<true>(slab, pods, pf, vidx, nL, out, words);
}

template <bool MAP, class Args>
static hipError_t launch_wide(const Args& a, hipStream_t st) {
  if (a.npods < 1 || a.npods > MAX_BATCH || !a.N) return hipErrorInvalidValue;
  const uint32_t grid = (a.N + 255) / 256;
  if (a.pf.enabled & 0x30u) {
    hipLaunchKernelGGL((fit_diag_kernel<true, false, MAP>), dim3(grid), dim3(256), 0, st, a);
    if (a.numa_n)
      hipLaunchKernelGGL((fit_diag_kernel<true, true, MAP>), dim3((a.numa_n + 255) / 256), dim3(256), 0, st, a);
  } else {
    hipLaunchKernelGGL((fit_diag_kernel<false, false, MAP>), dim3(grid), dim3(256), 0, st, a);
  }
  return hipGetLastError();
}

hipError_t launch_fit_diag(const DiagArgs& a, hipStream_t st) { return launch_wide<false>(a, st); }

hipError_t launch_fit_diag_map(const DiagMapArgs& a, hipStream_t st) {
  if (!a.words || a.npad < a.N) return hipErrorInvalidValue;
  return launch_wide<true>(a, st);
}

hipError_t launch_fit_diag_landed(const MirrorView& slab, const PodVec* pods, const Profile& pf, const uint16_t* vidx,
                                  int nF, int nL, uint32_t* out, hipStream_t st) {
  if (nF < 1 || nF > MAX_BATCH || nL < 1 || nL > MAX_BATCH) return hipErrorInvalidValue;
  hipLaunchKernelGGL(fit_diag_landed_kernel, dim3(nF), dim3(MAX_BATCH), 0, st, slab, pods, pf, vidx, nL, out);
  return hipGetLastError();
}

hipError_t preload_fit_diag_map() {
  hipFuncAttributes at;
  const void* const fn[] = {(const void*)fit_diag_kernel<true, false, true>, (const void*)fit_diag_kernel<true, true, true>,
                            (const void*)fit_diag_kernel<false, false, true>, (const void*)fit_diag_landed_map_kernel};
  for (const void* f : fn)
    if (hipError_t e = hipFuncGetAttributes(&at, f)) return e;
  return hipSuccess;
}

hipError_t launch_fit_diag_landed_map(const MirrorView& slab, const PodVec* pods, const Profile& pf, const uint16_t* vidx,
                                      int nF, int nL, uint32_t* out, uint16_t* words, hipStream_t st) {
  if (nF < 1 || nF > MAX_BATCH || nL < 1 || nL > MAX_BATCH || !words) return hipErrorInvalidValue;
  hipLaunchKernelGGL(fit_diag_landed_map_kernel, dim3(nF), dim3(MAX_BATCH), 0, st, slab, pods, pf, vidx, nL, out, words);
  return hipGetLastError();
}

}  // namespace gs
