// gs_preempt.cpp — host side of the ElasticQuota PostFilter dry run that needs no context: the resident-pod table
// (per-node segments in MoreImportantPod order, and their device image) and the pick of
// [upstream] pickOneNodeForPreemption over candidate keys. gs_engine.cpp holds the entry points that need a gs_ctx.
#include "gs_preempt.h"

#include <algorithm>
#include <cstring>

namespace gs {
namespace {

// [upstream] util.MoreImportantPod: higher priority first, then the earlier start time; the reference sorts with the
// unstable sort.Slice, so a remaining tie has no defined order there: ascending uid here
bool more_important(const PreRec& a, const PreRec& b) {
  if (a.priority != b.priority) return a.priority > b.priority;
  if (a.start != b.start) return a.start < b.start;
  return a.uid < b.uid;
}

int cap_class(uint32_t cap) {   // 8 << k
  int k = 0;
  while ((8u << k) < cap) ++k;
  return k;
}

}  // namespace

int PreemptTable::check_add(uint32_t node, const gs_resident_pod& p, const char** why) const {
  const PreSeg& sg = segs_[node];
  for (int s = 0; s < GS_NUM_RES; ++s)
    if (p.requests[s] < 0 || p.requests[s] >= (1LL << 53)) {
      *why = "a resident pod's request is negative or beyond 2^53";
      return GS_EINVAL;
    }
  for (int d = 0; d < GS_QUOTA_DIMS; ++d)
    if ((p.quota_request_mask >> d & 1u) && (p.quota_request[d] < 0 || p.quota_request[d] >= (1LL << 53))) {
      *why = "a resident pod's quota request is negative or beyond 2^53";
      return GS_EINVAL;
    }
  for (uint32_t j = 0; j < sg.cnt; ++j)
    if (pool_[sg.off + j].uid == p.uid) {
      *why = "the node already holds a resident pod with this uid";
      return GS_EINVAL;
    }
  if (sg.cnt >= GS_MAX_NODE_PODS) {
    *why = "a node holds at most GS_MAX_NODE_PODS resident pods";
    return GS_EUNSUPPORTED;
  }
  return GS_OK;
}

void PreemptTable::mark(uint32_t node) {
  if (!dirty_[node]) {
    dirty_[node] = 1;
    dirty_list_.push_back(node);
  }
}

void PreemptTable::add(uint32_t node, const gs_resident_pod& p) {
  PreSeg& sg = segs_[node];
  if (sg.cnt == cap_[node]) {   // the next capacity class: a recycled segment, else the pool grows
    const uint32_t ncap = cap_[node] ? cap_[node] * 2 : 8;
    std::vector<uint32_t>& fl = free_[cap_class(ncap)];
    uint32_t off;
    if (!fl.empty()) {
      off = fl.back();
      fl.pop_back();
    } else {
      off = (uint32_t)pool_.size();
      pool_.resize(pool_.size() + ncap);
    }
    if (sg.cnt) std::memcpy(&pool_[off], &pool_[sg.off], sizeof(PreRec) * sg.cnt);
    if (cap_[node]) free_[cap_class(cap_[node])].push_back(sg.off);
    sg.off = off;
    cap_[node] = ncap;
  }
  PreRec r{};
  for (int s = 0; s < 7; ++s) r.req[s] = p.requests[s];
  r.start = p.start_time_ns;
  for (int d = 0; d < GS_QUOTA_DIMS; ++d) r.qreq[d] = (p.quota_request_mask >> d & 1u) ? p.quota_request[d] : 0;
  r.uid = p.uid;
  r.priority = p.priority;
  r.quota = p.quota;
  r.flags = p.flags;
  r.qmask = p.quota_request_mask;
  for (int q = 0; q < GS_MAX_POD_PDBS; ++q) r.pdb[q] = GS_PDB_NONE;
  PreRec* b = &pool_[sg.off];
  PreRec* pos = std::upper_bound(b, b + sg.cnt, r, more_important);
  std::memmove(pos + 1, pos, sizeof(PreRec) * (size_t)(b + sg.cnt - pos));
  *pos = r;
  sg.cnt += 1;
  mark(node);
}

void PreemptTable::remove(uint32_t node, uint64_t uid) {
  PreSeg& sg = segs_[node];
  PreRec* b = sg.cnt ? &pool_[sg.off] : nullptr;
  for (uint32_t j = 0; j < sg.cnt; ++j) {
    if (b[j].uid != uid) continue;
    std::memmove(b + j, b + j + 1, sizeof(PreRec) * (sg.cnt - j - 1));
    sg.cnt -= 1;
    mark(node);
    return;
  }
}

const PreRec* PreemptTable::find(uint32_t node, uint64_t uid) const {
  const PreSeg& sg = segs_[node];
  for (uint32_t j = 0; j < sg.cnt; ++j)
    if (pool_[sg.off + j].uid == uid) return &pool_[sg.off + j];
  return nullptr;
}

void PreemptTable::set_pdbs(uint32_t node, uint64_t uid, const uint16_t* ids) {
  PreRec* r = const_cast<PreRec*>(find(node, uid));
  if (!r) return;
  int k = 0;   // the ids first, GS_PDB_NONE behind them
  for (int q = 0; q < GS_MAX_POD_PDBS; ++q)
    if (ids[q] != GS_PDB_NONE) r->pdb[k++] = ids[q];
  for (; k < GS_MAX_POD_PDBS; ++k) r->pdb[k] = GS_PDB_NONE;
  mark(node);
}

hipError_t PreemptTable::sync(hipStream_t st, bool rebuild) {
  hipError_t e;
  if (!d_segs_) {
    if ((e = d_segs_.alloc(sizeof(PreSeg) * std::max<size_t>(segs_.size(), 1)))) return e;
    rebuild = true;
  }
  if (pool_.size() > d_pool_cap_ || !d_pool_) {   // (no kernel reads the image: the caller waited)
    d_pool_cap_ = std::max<size_t>(pool_.size() + pool_.size() / 2, 1024);
    if ((e = d_pool_.alloc(sizeof(PreRec) * d_pool_cap_))) return e;
    rebuild = true;
  }
  if (rebuild || dirty_list_.size() > segs_.size() / 8) {
    if (!pool_.empty()) {
      if ((e = hipMemcpyAsync(d_pool_.get(), pool_.data(), sizeof(PreRec) * pool_.size(), hipMemcpyHostToDevice, st))) return e;
    }
    if (!segs_.empty()) {
      if ((e = hipMemcpyAsync(d_segs_.get(), segs_.data(), sizeof(PreSeg) * segs_.size(), hipMemcpyHostToDevice, st))) return e;
    }
  } else {
    for (uint32_t node : dirty_list_) {   // the changed nodes' records and column entries
      const PreSeg& sg = segs_[node];
      if (sg.cnt &&
          (e = hipMemcpyAsync(d_pool_.get() + sg.off, &pool_[sg.off], sizeof(PreRec) * sg.cnt, hipMemcpyHostToDevice, st)))
        return e;
      if ((e = hipMemcpyAsync(d_segs_.get() + node, &segs_[node], sizeof(PreSeg), hipMemcpyHostToDevice, st))) return e;
    }
  }
  for (uint32_t node : dirty_list_) dirty_[node] = 0;
  dirty_list_.clear();
  return hipStreamSynchronize(st);   // the copies read pool_ / segs_, which the next table call may move
}

void PdbTable::set(uint32_t id, int32_t allowed) {
  if (allowed_[id] == allowed) return;
  allowed_[id] = allowed;
  if (!dirty_[id]) {
    dirty_[id] = 1;
    dirty_list_.push_back(id);
  }
}

// Changed entries beyond which the whole 256-KB table goes in one copy. An estimate, not a measurement: a 4-byte copy
// from pageable memory costs a few microseconds of launch overhead whatever its size, the whole table some tens of
// microseconds at PCIe rates, so a few dozen entry copies already cost as much (the segments' eighth would be 8,191).
constexpr size_t kPdbWholeAbove = 32;

hipError_t PdbTable::sync(hipStream_t st, bool rebuild) {
  hipError_t e;
  if (!d_allowed_) {
    if ((e = d_allowed_.alloc(sizeof(int32_t) * allowed_.size()))) return e;
    rebuild = true;
  }
  if (rebuild || dirty_list_.size() > kPdbWholeAbove) {
    if ((e = hipMemcpyAsync(d_allowed_.get(), allowed_.data(), sizeof(int32_t) * allowed_.size(), hipMemcpyHostToDevice, st)))
      return e;
  } else {
    for (uint32_t id : dirty_list_)
      if ((e = hipMemcpyAsync(d_allowed_.get() + id, &allowed_[id], sizeof(int32_t), hipMemcpyHostToDevice, st))) return e;
  }
  for (uint32_t id : dirty_list_) dirty_[id] = 0;
  dirty_list_.clear();
  return hipStreamSynchronize(st);
}

}  // namespace gs

extern "C" int gs_preempt_pick_node_pdb(const gs_preempt_candidate_pdb* c, uint32_t n) {
  if (!c || !n) return -1;
  auto key = [&](uint32_t i) {
    return gs::PreKeyPdb{c[i].sum_priorities, c[i].earliest_start_ns, c[i].first_priority, c[i].num_victims, c[i].node, 1,
                         c[i].num_pdb_violations, 0u};
  };
  uint32_t best = 0;
  for (uint32_t i = 1; i < n; ++i)
    if (gs::pre_key_before(key(i), key(best))) best = i;
  return (int)best;
}

extern "C" int gs_preempt_pick_node(const gs_preempt_candidate* c, uint32_t n) {
  if (!c || !n) return -1;
  auto key = [&](uint32_t i) {
    return gs::PreKey{c[i].sum_priorities, c[i].earliest_start_ns, c[i].first_priority, c[i].num_victims, c[i].node, 1};
  };
  uint32_t best = 0;
  for (uint32_t i = 1; i < n; ++i)
    if (gs::pre_key_before(key(i), key(best))) best = i;
  return (int)best;
}
