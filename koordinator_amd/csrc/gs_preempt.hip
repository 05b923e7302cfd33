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
// gs_preempt_dry_run_pdb (PodDisruptionBudgets) runs the same body with PDB = true behind one more kernel:
//   preempt_partition_kernel  grid (ceil(N / 256), preemptors), a lane per node: filterPodsWithPDBViolation. The
//                         potential mask as pass 1 builds it, then per potential victim j with a non-empty list the
//                         count, per listed PDB, of potential victims at positions <= j that list it (a re-scan of the
//                         records' 8-byte lists: four counters, statically indexed); j is violating iff a count
//                         exceeds that PDB's budget in the device table. Out: two violating words per (preemptor, node).
//   preempt_nodes_pdb_kernel  the node kernel with those words loaded: the reprieve loop takes one step per potential
//                         victim, the violating ones first, then the others (eval_pair still inlined once); the
//                         key carries the violation count (violating pods whose Filter failed), `first` is the first
//                         victim in that order and `earliest` follows GetEarliestPodStartTime over all victims.
//   preempt_pick_pdb_kernel   the pick over PrePartPdb.
// The partition is a kernel of its own so that the policy instantiation, which already parks well over a hundred
// scalar registers in VGPR lanes, gains two loads and no loop.
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

__device__ __forceinline__ PreKeyPdb wave_min_key(PreKeyPdb k) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) {
    PreKeyPdb o;
    o.sum = shfl_xor_i64(k.sum, m);
    o.earliest = shfl_xor_i64(k.earliest, m);
    o.first = __shfl_xor(k.first, m);
    o.nvict = (uint32_t)__shfl_xor((int)k.nvict, m);
    o.node = __shfl_xor(k.node, m);
    o.valid = __shfl_xor(k.valid, m);
    o.nviol = (uint32_t)__shfl_xor((int)k.nviol, m);
    o.pad = 0u;
    if (pre_key_before(o, k)) k = o;
  }
  return k;
}

// the key, part and buffers of the two forms of the node kernel
template <bool PDB>
struct PreTypes {
  using Key = PreKey;
  using Part = PrePart;
  static __device__ __forceinline__ Part* parts(const PreemptArgs& a) { return a.parts; }
};
template <>
struct PreTypes<true> {
  using Key = PreKeyPdb;
  using Part = PrePartPdb;
  static __device__ __forceinline__ Part* parts(const PreemptArgs& a) { return a.parts_pdb; }
};
__device__ __forceinline__ void set_viol(PreKey&, uint32_t) {}
__device__ __forceinline__ void set_viol(PreKeyPdb& k, uint32_t n) { k.nviol = n; }
__device__ __forceinline__ void set_viol_bits(PrePart&, uint64_t, uint64_t) {}
__device__ __forceinline__ void set_viol_bits(PrePartPdb& p, uint64_t w0, uint64_t w1) {
  p.viol[0] = w0;
  p.viol[1] = w1;
}

__device__ __forceinline__ void copy_viol_bits(PrePart&, const PrePart&) {}
__device__ __forceinline__ void copy_viol_bits(PrePartPdb& o, const PrePartPdb& t) {
  o.viol[0] = t.viol[0];
  o.viol[1] = t.viol[1];
}

template <bool NUMA, bool POLICY, bool PDB>
__device__ __forceinline__ void preempt_nodes_body(const PreemptArgs& a, typename PreTypes<PDB>::Part* s_part /* LDS, [4] */) {
  using Key = typename PreTypes<PDB>::Key;
  using Part = typename PreTypes<PDB>::Part;
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
  uint64_t w0 = 0, w1 = 0;   // PDB: the violating group of the potential victims
  uint32_t nviol = 0;        // PDB: numViolatingVictim
  int32_t top = 0;           // PDB: the highest priority among the victims so far
  Key key{};
  key.node = (int32_t)i;
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
      if (PDB) {   // filterPodsWithPDBViolation: preempt_partition_kernel's words
        w0 = a.viol[((size_t)k * a.N + i) * 2];
        w1 = a.viol[((size_t)k * a.N + i) * 2 + 1];
      }
      // j = -1: the Filter with every potential victim gone; j >= 0: the reprieve of potential victim j. PDB: one
      // step per potential victim, the lowest remaining violating one while there is one, then the lowest remaining
      // other one (the two sweeps, without the steps that would skip)
      status = GS_PNODE_FITS;
      const int steps = PDB ? __popcll(p0) + __popcll(p1) : cnt;
      uint64_t r0 = p0, r1 = p1;   // PDB: the potential victims not reprieved yet
      for (int t = -1; t < steps; ++t) {
        int j = t;
        bool violating = false;
        if (PDB && t >= 0) {
          uint64_t a0 = r0 & w0, a1 = r1 & w1;
          violating = (a0 | a1) != 0;
          if (!violating) {
            a0 = r0;
            a1 = r1;
          }
          j = a0 ? __ffsll((unsigned long long)a0) - 1 : 63 + __ffsll((unsigned long long)a1);   // (a0 | a1) != 0: t < steps
          if (j < 64) r0 &= ~(1ull << j);
          else r1 &= ~(1ull << (j - 64));
        }
        if (!PDB && j >= 0 && !((j < 64 ? p0 >> j : p1 >> (j - 64)) & 1ull)) continue;
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
          if (PDB) {   // the first victim in slice order; GetEarliestPodStartTime over all victims
            if (code && violating) nviol += 1;
            if (!key.nvict) key.first = r.priority;
            if (!key.nvict || r.priority > top) {
              top = r.priority;
              key.earliest = r.start;
            } else if (r.priority == top && r.start < key.earliest) {
              key.earliest = r.start;
            }
          } else if (!key.nvict) {   // the first victim: the highest priority among the victims
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
  if (PDB && !key.valid) {
    w0 = w1 = 0;
    nviol = 0;
  }
  set_viol(key, nviol);
  if (own) {   // i < N
    a.status[(size_t)k * a.N + i] = (uint8_t)status;
    a.bits[((size_t)k * a.N + i) * 2] = v0;
    a.bits[((size_t)k * a.N + i) * 2 + 1] = v1;
    if (PDB) {
      a.viol[((size_t)k * a.N + i) * 2] = w0;
      a.viol[((size_t)k * a.N + i) * 2 + 1] = w1;
      a.nviol[(size_t)k * a.N + i] = (uint8_t)nviol;
    }
  }
  // the workgroup's part: every lane is active from here on
  const Key w = wave_min_key(key);
  const unsigned long long src = __ballot(key.valid && key.node == w.node);
  const int sl = src ? __ffsll(src) - 1 : 0;
  const uint64_t b0 = shfl_u64(v0, sl), b1 = shfl_u64(v1, sl);
  uint64_t c0 = 0, c1 = 0;
  if (PDB) {
    c0 = shfl_u64(w0, sl);
    c1 = shfl_u64(w1, sl);
  }
  const uint32_t npot = (uint32_t)__popcll(__ballot(potential));
  const uint32_t ncand = (uint32_t)__popcll(__ballot(status == GS_PNODE_CANDIDATE));
  const uint32_t nerr = (uint32_t)__popcll(__ballot(status == GS_PNODE_ERROR));
  if (lane == 0) {
    Part& o = s_part[wv];
    o.key = w;
    o.bits[0] = w.valid ? b0 : 0;
    o.bits[1] = w.valid ? b1 : 0;
    set_viol_bits(o, w.valid ? c0 : 0, w.valid ? c1 : 0);
    o.npot = npot;
    o.ncand = ncand;
    o.nerr = nerr;
    o.pad = 0u;
  }
  __syncthreads();
  if (tid == 0) {
    Part o = s_part[0];
    for (int q = 1; q < 4; ++q) {
      const Part& t = s_part[q];
      if (pre_key_before(t.key, o.key)) {
        o.key = t.key;
        o.bits[0] = t.bits[0];
        o.bits[1] = t.bits[1];
        copy_viol_bits(o, t);
      }
      o.npot += t.npot;
      o.ncand += t.ncand;
      o.nerr += t.nerr;
    }
    const uint32_t part = POLICY ? (a.N + 255) / 256 + blockIdx.x : blockIdx.x;   // < nparts (launch_preempt)
    PreTypes<PDB>::parts(a)[(size_t)k * a.nparts + part] = o;
  }
}

template <bool NUMA, bool POLICY>
__global__ void __launch_bounds__(256) preempt_nodes_kernel(PreemptArgs a) {
  __shared__ PrePart s_part[4];
  preempt_nodes_body<NUMA, POLICY, false>(a, s_part);
}

template <bool NUMA, bool POLICY>
__global__ void __launch_bounds__(256) preempt_nodes_pdb_kernel(PreemptArgs a) {
  __shared__ PrePartPdb s_part[4];
  preempt_nodes_body<NUMA, POLICY, true>(a, s_part);
}

// filterPodsWithPDBViolation (preempt.go:222-267) per (preemptor, node): the violating group of the potential victims.
// Potential victim j is violating iff, for a PDB p of its list, the potential victims at positions <= j that list p
// outnumber budgets[p]: what the reference's running counters say, without a counter per PDB.
__global__ void __launch_bounds__(256) preempt_partition_kernel(PreemptArgs a) {
  const int k = blockIdx.y;
  const PrePod& P = a.pods[k];   // wave-uniform
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= a.N) return;
  uint64_t w0 = 0, w1 = 0;
  if (P.active && (P.row < 0 || pre_potential(a.rows[(size_t)P.row * a.N + i]))) {
    const PreSeg sg = a.segs[i];
    const PreRec* __restrict__ recs = a.recs + sg.off;
    const int cnt = (int)min(sg.cnt, (uint32_t)GS_MAX_NODE_PODS);
    auto potential = [&](const PreRec& r) {
      return !((r.flags & GS_RESIDENT_NON_PREEMPTIBLE) || r.priority >= P.priority || r.quota != P.quota);
    };
    for (int j = 0; j < cnt; ++j) {
      const PreRec& r = recs[j];
      if (r.pdb[0] == GS_PDB_NONE || !potential(r)) continue;   // (the ids stand first in the list)
      const uint32_t id0 = r.pdb[0], id1 = r.pdb[1], id2 = r.pdb[2], id3 = r.pdb[3];
      int32_t n0 = 0, n1 = 0, n2 = 0, n3 = 0;   // potential victims at positions <= j that list id0..3
      for (int q = 0; q <= j; ++q) {
        const PreRec& e = recs[q];
        if (e.pdb[0] == GS_PDB_NONE || !potential(e)) continue;
#pragma unroll
        for (int u = 0; u < GS_MAX_POD_PDBS; ++u) {
          const uint32_t id = e.pdb[u];
          if (id == GS_PDB_NONE) continue;
          n0 += id == id0;
          n1 += id == id1;
          n2 += id == id2;
          n3 += id == id3;
        }
      }
      bool violating = n0 > a.budgets[id0];
      if (id1 != GS_PDB_NONE) violating |= n1 > a.budgets[id1];
      if (id2 != GS_PDB_NONE) violating |= n2 > a.budgets[id2];
      if (id3 != GS_PDB_NONE) violating |= n3 > a.budgets[id3];
      if (violating) {
        if (j < 64) w0 |= 1ull << j;
        else w1 |= 1ull << (j - 64);
      }
    }
  }
  a.viol[((size_t)k * a.N + i) * 2] = w0;
  a.viol[((size_t)k * a.N + i) * 2 + 1] = w1;
}

// one workgroup per preemptor: the first of the parts' keys and the sums of their counts (Part: PrePart or PrePartPdb;
// fields are copied one by one, a whole-struct copy would become a stack object)
template <class Part>
__device__ __forceinline__ void preempt_pick_body(const Part* __restrict__ parts, uint32_t nparts, Part* __restrict__ result,
                                                  Part* s_part /* LDS, [4] */) {
  using Key = decltype(Part::key);
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, k = blockIdx.x;
  Key key{};
  uint32_t best = 0, npot = 0, ncand = 0, nerr = 0;
  for (uint32_t q = tid; q < nparts; q += 256) {
    const Part& t = parts[(size_t)k * nparts + q];
    if (pre_key_before(t.key, key)) {
      key = t.key;
      best = q;
    }
    npot += t.npot;
    ncand += t.ncand;
    nerr += t.nerr;
  }
  const Key w = wave_min_key(key);
  const unsigned long long src = __ballot(key.valid && key.node == w.node);
  const int sl = src ? __ffsll(src) - 1 : 0;
  const uint32_t bq = (uint32_t)__shfl((int)best, sl);
  npot = (uint32_t)wave_sum((int)npot);
  ncand = (uint32_t)wave_sum((int)ncand);
  nerr = (uint32_t)wave_sum((int)nerr);
  if (lane == 0) {
    Part& o = s_part[wv];
    o.key = w;
    o.bits[0] = o.bits[1] = 0;
    set_viol_bits(o, 0, 0);
    o.npot = npot;
    o.ncand = ncand;
    o.nerr = nerr;
    o.pad = 0u;
    if (w.valid) {
      const Part& t = parts[(size_t)k * nparts + bq];
      o.bits[0] = t.bits[0];
      o.bits[1] = t.bits[1];
      copy_viol_bits(o, t);
    }
  }
  __syncthreads();
  if (tid == 0) {
    Part o = s_part[0];
    for (int q = 1; q < 4; ++q) {
      const Part& t = s_part[q];
      if (pre_key_before(t.key, o.key)) {
        o.key = t.key;
        o.bits[0] = t.bits[0];
        o.bits[1] = t.bits[1];
        copy_viol_bits(o, t);
      }
      o.npot += t.npot;
      o.ncand += t.ncand;
      o.nerr += t.nerr;
    }
    result[k] = o;
  }
}

__global__ void __launch_bounds__(256) preempt_pick_kernel(const PrePart* __restrict__ parts, uint32_t nparts,
                                                           PrePart* __restrict__ result) {
  __shared__ PrePart s_part[4];
  preempt_pick_body(parts, nparts, result, s_part);
}

__global__ void __launch_bounds__(256) preempt_pick_pdb_kernel(const PrePartPdb* __restrict__ parts, uint32_t nparts,
                                                               PrePartPdb* __restrict__ result) {
  __shared__ PrePartPdb s_part[4];
  preempt_pick_body(parts, nparts, result, s_part);
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

hipError_t launch_preempt_pdb(const PreemptArgs& a, hipStream_t st) {
  if (a.npre < 1 || a.npre > MAX_BATCH || !a.N || a.nparts != preempt_parts(a.pf, a.N, a.numa_n)) return hipErrorInvalidValue;
  if (!a.budgets || !a.viol || !a.nviol || !a.parts_pdb || !a.result_pdb) return hipErrorInvalidValue;
  const dim3 grid((a.N + 255) / 256, a.npre);
  hipLaunchKernelGGL(preempt_partition_kernel, grid, dim3(256), 0, st, a);
  if (a.pf.enabled & 0x30u) {
    hipLaunchKernelGGL((preempt_nodes_pdb_kernel<true, false>), grid, dim3(256), 0, st, a);
    if (a.numa_n)
      hipLaunchKernelGGL((preempt_nodes_pdb_kernel<true, true>), dim3((a.numa_n + 255) / 256, a.npre), dim3(256), 0, st, a);
  } else {
    hipLaunchKernelGGL((preempt_nodes_pdb_kernel<false, false>), grid, dim3(256), 0, st, a);
  }
  hipLaunchKernelGGL(preempt_pick_pdb_kernel, dim3(a.npre), dim3(256), 0, st, a.parts_pdb, a.nparts, a.result_pdb);
  return hipGetLastError();
}

}  // namespace gs
