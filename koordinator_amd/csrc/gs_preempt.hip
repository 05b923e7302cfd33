// gs_preempt.hip — the ElasticQuota PostFilter dry run of gs_preempt_dry_run: [upstream] DryRunPreemption over every
// potential node (elasticquota/preempt.go:43-45 GetOffsetAndNumCandidates returns all of them) with the plugin's
// SelectVictimsOnNode (preempt.go:111-215) per node, and pickOneNodeForPreemption over the candidates.
//
//   preempt_nodes_kernel  grid (ceil(N / 256), preemptors). A lane owns one node: its mirror row in registers, the
//                         four scalar free columns in Row::free[3..6] (eval_pair's LDS_SCALARS form reads the row
//                         alone); the preemptor's vectors are wave-uniform. <NUMA, false>: every node without a NUMA
//                         topology policy; <true, true>: the policy nodes through the ascending index list, as
//                         fit_diag_kernel. Per lane: the potential-node test on the row word, pass 1 over the node's
//                         records (the 128-bit potential mask, Requested and `used` with the potential victims gone),
//                         the Filter, then the reprieve pass in the records' order (MoreImportantPod: the table keeps
//                         it) with free[], free_pods and `used` updated in registers. Every Filter evaluation is the
//                         whole non-FULL eval_pair on the updated row: nothing is assumed invariant between steps.
//                         Out: status byte, two victim words; per workgroup the lexicographic minimum of the
//                         candidates' pick keys (wave reduction, then one key per workgroup) and three counts.
//   preempt_pick_kernel   one workgroup per preemptor behind it on the stream: the minimum of the workgroups' keys
//                         and the sums of their counts.
// The key (first priority, priority sum, victims, earliest start descending, node) is compared field by field, never
// packed: pre_key_before is the order gs_preempt_pick_node applies on the host.
//
// Memory: the lanes of a wave walk 64 different lists, so one step's load of a record field touches up to 64
// different 128-B lines (a 160-B record lies in at most two); a lane reads each record of its node once in pass 1
// and once more if it is a potential victim. Nothing is indexed at run time per lane: no scratch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gs_eval_dev.h"
#include "gs_preempt.h"

namespace gs {

__device__ __forceinline__ int64_t shfl_xor_i64(int64_t v, int m) {
  const int lo = __shfl_xor((int)(uint32_t)(uint64_t)v, m), hi = __shfl_xor((int)(uint32_t)((uint64_t)v >> 32), m);
  return (int64_t)(((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo);
}

__device__ __forceinline__ uint64_t shfl_u64(uint64_t v, int src) {
  const int lo = __shfl((int)(uint32_t)v, src), hi = __shfl((int)(uint32_t)(v >> 32), src);
  return ((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo;
}

// the wave's first key in pick order, in every lane (all 64 lanes active)
__device__ __forceinline__ PreKey wave_min_key(PreKey k) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) {
    PreKey o;
    o.sum = shfl_xor_i64(k.sum, m);
    o.earliest = shfl_xor_i64(k.earliest, m);
    o.first = __shfl_xor(k.first, m);
    o.nvict = (uint32_t)__shfl_xor((int)k.nvict, m);
    o.node = __shfl_xor(k.node, m);
    o.valid = __shfl_xor(k.valid, m);
    if (pre_key_before(o, k)) k = o;
  }
  return k;
}

template <bool NUMA, bool POLICY>
__global__ void __launch_bounds__(256) preempt_nodes_kernel(PreemptArgs a) {
  __shared__ PrePart s_part[4];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int k = blockIdx.y;
  const PrePod& P = a.pods[k];   // wave-uniform
  uint32_t i = blockIdx.x * 256 + tid;
  bool own;
  if (POLICY) {
    own = i < a.numa_n;
    i = a.numa_idx[own ? i : 0];
  } else {
    own = i < a.N;
    if (!own) i = 0;
  }
  Row row;
  load_row(a.m, i, false, NUMA, row);
#pragma unroll
  for (int s = 3; s < 7; ++s) row.free[s] = a.m.c64(C_FREE_CPU + s)[i];
  // (nodes with a NUMA topology policy: the <true, true> launch)
  if (NUMA && !POLICY && ((row.nr.nflags >> NF_POLICY_SHIFT) & 3u)) own = false;
  Profile pf = a.pf;
  pf.enabled &= NUMA ? 0x15u : 0x05u;   // the three Filters; no Score

  uint32_t status = GS_PNODE_NOT_POTENTIAL;
  uint64_t v0 = 0, v1 = 0;   // victim bits
  PreKey key{0, 0, 0, 0u, (int32_t)i, 0};
  const bool potential = own && P.active && (P.row < 0 || pre_potential(a.rows[(size_t)P.row * a.N + i]));
  if (potential) {
    const PreSeg sg = a.segs[i];
    const PreRec* __restrict__ recs = a.recs + sg.off;
    const int cnt = (int)min(sg.cnt, (uint32_t)GS_MAX_NODE_PODS);
    const bool skip = P.skip;
    int64_t used[8];
#pragma unroll
    for (int d = 0; d < 8; ++d) used[d] = P.used[d];
    // NodeInfo.RemovePod / AddPodInfo of one record on the row, and the plugin's RemovePod / AddPod on `used`
    auto remove_pod = [&](const PreRec& r) {
#pragma unroll
      for (int s = 0; s < 7; ++s) row.free[s] += r.req[s];
      row.free_pods += 1;
      if (!skip && (r.flags & GS_RESIDENT_QUOTA_TRACKED)) {
#pragma unroll
        for (int d = 0; d < 8; ++d) {
          const int64_t u = used[d] - r.qreq[d];
          used[d] = u < 0 ? 0 : u;
        }
      }
    };
    auto add_pod = [&](const PreRec& r) {
#pragma unroll
      for (int s = 0; s < 7; ++s) row.free[s] -= r.req[s];
      row.free_pods -= 1;
      if (!skip && (r.flags & GS_RESIDENT_QUOTA_TRACKED)) {
#pragma unroll
        for (int d = 0; d < 8; ++d) used[d] += r.qreq[d];
      }
    };
    // pass 1: the potential victims leave
    uint64_t p0 = 0, p1 = 0;
    for (int j = 0; j < cnt; ++j) {
      const PreRec& r = recs[j];
      if ((r.flags & GS_RESIDENT_NON_PREEMPTIBLE) || r.priority >= P.priority || r.quota != P.quota) continue;
      if (j < 64) p0 |= 1ull << j;
      else p1 |= 1ull << (j - 64);
      remove_pod(r);
    }
    if (!(p0 | p1)) {
      status = GS_PNODE_NO_VICTIMS;
    } else {
      // j = -1: the Filter with every potential victim gone; j >= 0: the reprieve of potential victim j
      status = GS_PNODE_FITS;
      for (int j = -1; j < cnt; ++j) {
        if (j >= 0 && !((j < 64 ? p0 >> j : p1 >> (j - 64)) & 1ull)) continue;
        const PreRec& r = recs[j < 0 ? 0 : j];
        if (j >= 0) add_pod(r);
        const uint32_t code = eval_pair<false, true, POLICY>(row, P.v, pf, a.m).code;
        if (j < 0) {
          if (code) {
            status = GS_PNODE_UNFIT;
            break;
          }
          continue;
        }
        bool victim = false;
        if (code) {
          remove_pod(r);
          victim = true;
        }
        bool exceed = false;
#pragma unroll
        for (int d = 0; d < 8; ++d)
          if ((P.check >> d & 1u) && used[d] + P.qreq[d] > P.limit[d]) exceed = true;
        if (exceed) {
          if (victim) {   // removed already: the second nodeInfo.RemovePod fails
            status = GS_PNODE_ERROR;
            break;
          }
          remove_pod(r);
          victim = true;
        }
        if (victim) {
          if (j < 64) v0 |= 1ull << j;
          else v1 |= 1ull << (j - 64);
          if (!key.nvict) {   // the first victim: the highest priority among the victims
            key.first = r.priority;
            key.earliest = r.start;
          } else if (r.priority == key.first && r.start < key.earliest) {
            key.earliest = r.start;
          }
          key.nvict += 1;
          key.sum += (int64_t)r.priority + 2147483648LL;
          status = GS_PNODE_CANDIDATE;
        }
      }
      if (status != GS_PNODE_CANDIDATE) v0 = v1 = 0;
    }
  }
  key.valid = status == GS_PNODE_CANDIDATE;
  if (own) {   // i < N
    a.status[(size_t)k * a.N + i] = (uint8_t)status;
    a.bits[((size_t)k * a.N + i) * 2] = v0;
    a.bits[((size_t)k * a.N + i) * 2 + 1] = v1;
  }
  // the workgroup's part: every lane is active from here on
  const PreKey w = wave_min_key(key);
  const unsigned long long src = __ballot(key.valid && key.node == w.node);
  const int sl = src ? __ffsll(src) - 1 : 0;
  const uint64_t b0 = shfl_u64(v0, sl), b1 = shfl_u64(v1, sl);
  const uint32_t npot = (uint32_t)__popcll(__ballot(potential));
  const uint32_t ncand = (uint32_t)__popcll(__ballot(status == GS_PNODE_CANDIDATE));
  const uint32_t nerr = (uint32_t)__popcll(__ballot(status == GS_PNODE_ERROR));
  if (lane == 0) s_part[wv] = PrePart{w, {w.valid ? b0 : 0, w.valid ? b1 : 0}, npot, ncand, nerr, 0u};
  __syncthreads();
  if (tid == 0) {
    PrePart o = s_part[0];
    for (int q = 1; q < 4; ++q) {
      const PrePart& t = s_part[q];
      if (pre_key_before(t.key, o.key)) {
        o.key = t.key;
        o.bits[0] = t.bits[0];
        o.bits[1] = t.bits[1];
      }
      o.npot += t.npot;
      o.ncand += t.ncand;
      o.nerr += t.nerr;
    }
    const uint32_t part = POLICY ? (a.N + 255) / 256 + blockIdx.x : blockIdx.x;   // < nparts (launch_preempt)
    a.parts[(size_t)k * a.nparts + part] = o;
  }
}

// one workgroup per preemptor: the first of the parts' keys and the sums of their counts
__global__ void __launch_bounds__(256) preempt_pick_kernel(const PrePart* __restrict__ parts, uint32_t nparts,
                                                           PrePart* __restrict__ result) {
  __shared__ PrePart s_part[4];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, k = blockIdx.x;
  PreKey key{0, 0, 0, 0u, 0, 0};
  uint32_t best = 0, npot = 0, ncand = 0, nerr = 0;
  for (uint32_t q = tid; q < nparts; q += 256) {
    const PrePart& t = parts[(size_t)k * nparts + q];
    if (pre_key_before(t.key, key)) {
      key = t.key;
      best = q;
    }
    npot += t.npot;
    ncand += t.ncand;
    nerr += t.nerr;
  }
  const PreKey w = wave_min_key(key);
  const unsigned long long src = __ballot(key.valid && key.node == w.node);
  const int sl = src ? __ffsll(src) - 1 : 0;
  const uint32_t bq = (uint32_t)__shfl((int)best, sl);
  npot = (uint32_t)wave_sum((int)npot);
  ncand = (uint32_t)wave_sum((int)ncand);
  nerr = (uint32_t)wave_sum((int)nerr);
  if (lane == 0) {
    PrePart o{w, {0, 0}, npot, ncand, nerr, 0u};
    if (w.valid) {
      o.bits[0] = parts[(size_t)k * nparts + bq].bits[0];
      o.bits[1] = parts[(size_t)k * nparts + bq].bits[1];
    }
    s_part[wv] = o;
  }
  __syncthreads();
  if (tid == 0) {
    PrePart o = s_part[0];
    for (int q = 1; q < 4; ++q) {
      const PrePart& t = s_part[q];
      if (pre_key_before(t.key, o.key)) {
        o.key = t.key;
        o.bits[0] = t.bits[0];
        o.bits[1] = t.bits[1];
      }
      o.npot += t.npot;
      o.ncand += t.ncand;
      o.nerr += t.nerr;
    }
    result[k] = o;
  }
}

uint32_t preempt_parts(const Profile& pf, uint32_t N, uint32_t numa_n) {
  return (N + 255) / 256 + ((pf.enabled & 0x30u) ? (numa_n + 255) / 256 : 0u);
}

hipError_t launch_preempt(const PreemptArgs& a, hipStream_t st) {
  if (a.npre < 1 || a.npre > MAX_BATCH || !a.N || a.nparts != preempt_parts(a.pf, a.N, a.numa_n)) return hipErrorInvalidValue;
  const dim3 grid((a.N + 255) / 256, a.npre);
  if (a.pf.enabled & 0x30u) {
    hipLaunchKernelGGL((preempt_nodes_kernel<true, false>), grid, dim3(256), 0, st, a);
    if (a.numa_n)
      hipLaunchKernelGGL((preempt_nodes_kernel<true, true>), dim3((a.numa_n + 255) / 256, a.npre), dim3(256), 0, st, a);
  } else {
    hipLaunchKernelGGL((preempt_nodes_kernel<false, false>), grid, dim3(256), 0, st, a);
  }
  hipLaunchKernelGGL(preempt_pick_kernel, dim3(a.npre), dim3(256), 0, st, a.parts, a.nparts, a.result);
  return hipGetLastError();
}

}  // namespace gs
