// gs_preempt.h — the ElasticQuota PostFilter dry run (gs_preempt_dry_run): the resident-pod table's device image, the
// per-preemptor vectors and the launch interface of gs_preempt.hip (host <-> device contract).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "../../include/gpuscore.h"
#include "gs_kernels.h"
#include "gs_owned.h"

namespace gs {

// One resident pod, as the table holds it on the host and on the device (the host pool IS the image): 160 B, so a
// record starts 32-B aligned and never straddles more than two 128-B lines.
struct PreRec {
  int64_t req[7];        // gs_resident_pod.requests, slots 0..6 (NodeInfo.RemovePod / AddPod)
  int64_t start;         // start_time_ns
  int64_t qreq[8];       // quota_request, 0 outside its mask
  uint64_t uid;
  int32_t priority;
  int32_t quota;
  uint32_t flags;        // GS_RESIDENT_*
  uint32_t qmask;
  uint16_t pdb[GS_MAX_POD_PDBS];   // gs_node_pods_set_pdbs: the PDBs decremented for this pod, GS_PDB_NONE = no entry
};
static_assert(sizeof(PreRec) == 160, "PreRec layout");

// A node's segment of the pool: records [off, off + cnt), in MoreImportantPod order
struct PreSeg {
  uint32_t off, cnt;
};

// One preemptor (wave-uniform in the kernel: read with scalar loads)
struct PrePod {
  PodVec v;
  int64_t qreq[8];       // quota_request (0 outside check)
  int64_t used[8];       // postFilterState.used
  int64_t limit[8];      // postFilterState.usedLimit
  uint32_t check;        // quota_request keys ∧ usedLimit keys (0 with skip: the check always passes)
  uint32_t skip;         // postFilterState.skip: AddPod / RemovePod leave `used` alone
  int32_t priority;
  int32_t quota;
  int32_t row;           // row of the status words, -1: every node is potential
  int32_t active;        // 0: not eligible (every node's status is 0)
  int32_t pad[2];
};
static_assert(sizeof(PrePod) == sizeof(PodVec) + 3 * 64 + 32, "PrePod layout");

// The pick key of one candidate node: gs_preempt_candidate, valid = 0 for "none"
struct PreKey {
  int64_t sum;
  int64_t earliest;
  int32_t first;
  uint32_t nvict;
  int32_t node;
  int32_t valid;
};

// What one workgroup leaves per preemptor, and what the final pass leaves per preemptor
struct PrePart {
  PreKey key;
  uint64_t bits[2];      // the key's victim bits
  uint32_t npot, ncand, nerr, pad;
};
static_assert(sizeof(PrePart) == 64, "PrePart layout");

// The same three for gs_preempt_dry_run_pdb: the key begins with the violation count
struct PreKeyPdb {
  int64_t sum;
  int64_t earliest;      // GetEarliestPodStartTime: the earliest start among the victims of the highest priority
  int32_t first;         // the first victim in slice order (violating group first): not always the highest priority
  uint32_t nvict;
  int32_t node;
  int32_t valid;
  uint32_t nviol;        // numViolatingVictim
  uint32_t pad;
};
struct PrePartPdb {
  PreKeyPdb key;
  uint64_t bits[2];      // the key's victim bits
  uint64_t viol[2];      // ... and its violating group
  uint32_t npot, ncand, nerr, pad;
};
static_assert(sizeof(PreKeyPdb) == 40 && sizeof(PrePartPdb) == 88, "PrePartPdb layout");

// the potential-node test on a status word: framework.Code != UnschedulableAndUnresolvable, as
// gs_status_framework_code reads the word (Fit and LoadAware statuses are Unschedulable; NodeNUMAResource's reasons
// 1, 2, 3, 5, 6, 7, 9 are UnschedulableAndUnresolvable: gs_reasons.cpp kNuma)
constexpr uint32_t PRE_UNRESOLVABLE_NUMA = 0x2EEu;
#ifdef __HIPCC__
__host__ __device__
#endif
inline bool pre_potential(uint32_t word) {
  const uint32_t code = word & 0x0FFFu;
  if (code & 0x3Fu) return true;
  if (code & (GS_FAIL_LA_MEMORY | GS_FAIL_LA_AGGREGATED)) return true;   // malformed (no code 2 to report)
  return !(PRE_UNRESOLVABLE_NUMA >> ((code & GS_FAIL_NUMA_MASK) >> GS_FAIL_NUMA_SHIFT) & 1u);
}

struct PreemptArgs {
  MirrorView m;
  Profile pf;
  uint32_t N;
  int npre;                  // preemptors (grid.y)
  const PrePod* pods;
  const uint16_t* rows;      // [num_rows][N] status words
  const PreRec* recs;        // the pool
  const PreSeg* segs;        // [N]
  const uint32_t* numa_idx;  // the nodes with a NUMA topology policy (ascending), numa_n of them
  uint32_t numa_n;
  uint8_t* status;           // [npre][N]
  uint64_t* bits;            // [npre][N][2]
  PrePart* parts;            // [npre][nparts]: one per workgroup of either instantiation
  uint32_t nparts;
  PrePart* result;           // [npre]
  // gs_preempt_dry_run_pdb only (launch_preempt_pdb; parts and result above are unused there)
  const int32_t* budgets;    // [GS_MAX_PDBS] DisruptionsAllowed, GS_PDB_UNLIMITED where never set
  uint64_t* viol;            // [npre][N][2]: preempt_partition_kernel writes the violating group of the potential
                             // victims, the node kernel reads it and zeroes it unless the node is a candidate
  uint8_t* nviol;            // [npre][N] numViolatingVictim
  PrePartPdb* parts_pdb;     // [npre][nparts]
  PrePartPdb* result_pdb;    // [npre]
};
// workgroups of the two node passes for N nodes of which numa_n carry a NUMA topology policy
uint32_t preempt_parts(const Profile& pf, uint32_t N, uint32_t numa_n);
// preempt_nodes_kernel over every node (policy nodes through numa_idx in a second instantiation) and the
// one-workgroup-per-preemptor pick pass behind it
hipError_t launch_preempt(const PreemptArgs& a, hipStream_t st);
// the same with PodDisruptionBudgets: preempt_partition_kernel, preempt_nodes_pdb_kernel, preempt_pick_pdb_kernel
hipError_t launch_preempt_pdb(const PreemptArgs& a, hipStream_t st);

// the pick of step 4 as a strict order: a is picked before b
#ifdef __HIPCC__
__host__ __device__
#endif
inline bool pre_key_before(const PreKey& a, const PreKey& b) {
  if (a.valid != b.valid) return a.valid > b.valid;
  if (a.first != b.first) return a.first < b.first;
  if (a.sum != b.sum) return a.sum < b.sum;
  if (a.nvict != b.nvict) return a.nvict < b.nvict;
  if (a.earliest != b.earliest) return a.earliest > b.earliest;
  return a.node < b.node;
}

// pickOneNodeForPreemption in full: fewest PDB violations first, then the order above
#ifdef __HIPCC__
__host__ __device__
#endif
inline bool pre_key_before(const PreKeyPdb& a, const PreKeyPdb& b) {
  if (a.valid != b.valid) return a.valid > b.valid;
  if (a.nviol != b.nviol) return a.nviol < b.nviol;
  if (a.first != b.first) return a.first < b.first;
  if (a.sum != b.sum) return a.sum < b.sum;
  if (a.nvict != b.nvict) return a.nvict < b.nvict;
  if (a.earliest != b.earliest) return a.earliest > b.earliest;
  return a.node < b.node;
}

// ---- the resident-pod table (host side, gs_preempt.cpp) ----
// Per node a segment of a pool of PreRec, kept in MoreImportantPod order (priority desc, start asc, uid asc: the
// order does not depend on the preemptor, so the kernel never sorts). Segments have capacities 8, 16, .., 128 and are
// recycled per capacity; the device image is the pool plus the per-node (offset, count) column, and a change to k
// nodes uploads those nodes' segments and column entries.
class PreemptTable {
 public:
  explicit PreemptTable(uint32_t num_nodes) : segs_(num_nodes, PreSeg{0, 0}), cap_(num_nodes, 0), dirty_(num_nodes, 0) {}
  // 0, GS_EINVAL (duplicate uid, bad request), GS_EUNSUPPORTED (129th pod)
  int check_add(uint32_t node, const gs_resident_pod& p, const char** why) const;
  void add(uint32_t node, const gs_resident_pod& p);
  void remove(uint32_t node, uint64_t uid);
  // the record of uid on node, nullptr if the node does not hold it; set_pdbs replaces its PDB list
  const PreRec* find(uint32_t node, uint64_t uid) const;
  void set_pdbs(uint32_t node, uint64_t uid, const uint16_t* ids);
  uint32_t count(uint32_t node) const { return segs_[node].cnt; }
  const PreRec* records(uint32_t node) const { return pool_.data() + segs_[node].off; }
  // brings the device image up to date on st (the caller has made sure no kernel reads it); rebuild: all of it
  hipError_t sync(hipStream_t st, bool rebuild);
  const PreRec* d_recs() const { return d_pool_.get(); }
  const PreSeg* d_segs() const { return d_segs_.get(); }

 private:
  void mark(uint32_t node);
  std::vector<PreRec> pool_;
  std::vector<PreSeg> segs_;
  std::vector<uint32_t> cap_;             // the node's segment capacity (0: none)
  std::vector<uint32_t> free_[5];         // free segment offsets per capacity class 8 << k
  std::vector<uint8_t> dirty_;
  std::vector<uint32_t> dirty_list_;
  DevBuf<PreRec> d_pool_;
  DevBuf<PreSeg> d_segs_;
  size_t d_pool_cap_ = 0;                 // records the device pool holds
};

// ---- the PodDisruptionBudget table (gs_pdbs_upsert): DisruptionsAllowed by PDB id, and its device image ----
class PdbTable {
 public:
  PdbTable() : allowed_(GS_MAX_PDBS, GS_PDB_UNLIMITED), dirty_(GS_MAX_PDBS, 0) {}
  void set(uint32_t id, int32_t allowed);
  int32_t get(uint32_t id) const { return allowed_[id]; }
  // as PreemptTable::sync: the changed entries one by one, or the whole table once more than a few dozen changed
  hipError_t sync(hipStream_t st, bool rebuild);
  const int32_t* d_allowed() const { return d_allowed_.get(); }

 private:
  std::vector<int32_t> allowed_;
  std::vector<uint8_t> dirty_;
  std::vector<uint32_t> dirty_list_;
  DevBuf<int32_t> d_allowed_;
};

}  // namespace gs
