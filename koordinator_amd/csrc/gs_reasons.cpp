// gs_reasons.cpp — the reference's Filter status (framework.Code + message) for a gs_evaluate failure code, so a
// cgo wrapper can return the same *framework.Status the plugins return.
//
//   NodeResourcesFit  [upstream] noderesources/fit.go fitsRequest: "Too many pods", "Insufficient cpu",
//                     "Insufficient memory", "Insufficient ephemeral-storage", "Insufficient <scalar>", joined by ", "
//                     (framework.Status.Message), Unschedulable
//   LoadAware         load_aware.go:45-46 ErrReasonUsageExceedThreshold / ErrReasonAggregatedUsageExceedThreshold
//                     with the resource (GS_FAIL_LA_MEMORY / GS_FAIL_LA_AGGREGATED), Unschedulable (:218-221, :250)
//   NodeNUMAResource  plugin.go:48-55 (Err* constants), util.go:117, topology_hint.go:36, topologymanager/manager.go:70,
//                     resource_manager.go:292,396 (the allocator's errors)
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <string>
#include <vector>

#include "../../include/gpuscore.h"
#include "gs_reasons.h"

namespace {

constexpr int kSuccess = 0, kUnschedulable = 1, kUnresolvable = 2;

struct NumaReason {
  int code;
  const char* msg;
};
// indexed by gs_numa_reason
const NumaReason kNuma[] = {
    {kSuccess, ""},
    {kUnresolvable, "the requested CPUs must be integer"},                               // ErrInvalidRequestedCPUs
    {kUnresolvable, "node(s) invalid CPU amplification ratio"},                          // ErrInvalidCPUAmplificationRatio
    {kUnresolvable, "node(s) invalid CPU Topology"},                                     // GetAvailableCPUs error (:396)
    {kUnschedulable, "Insufficient amplified cpu"},                                      // ErrInsufficientAmplifiedCPU
    {kUnresolvable, "node(s) invalid CPU Topology"},                                     // ErrInvalidCPUTopology
    {kUnresolvable, "node(s) cpu bind policy conflicts with pod's required cpu bind policy"},   // ErrCPUBindPolicyConflict
    {kUnresolvable, "node(s) requested cpus not multiple cpus per core"},                // ErrSMTAlignmentError
    {kUnschedulable, "not enough cpus available to satisfy request"},                    // allocateCPUSet (:292)
    {kUnresolvable, "node(s) missing NUMA resources"},                                   // topology_hint.go:36
    {kUnschedulable, "node(s) NUMA Topology affinity error"},                            // manager.go:70
    {kUnschedulable, "not enough cpus available to satisfy request"},                    // Allocate after Admit (see gpuscore.h)
};

const char* const kScalarDefault[4] = {"kubernetes.io/batch-cpu", "kubernetes.io/batch-memory", "kubernetes.io/mid-cpu",
                                       "kubernetes.io/mid-memory"};

// the reason text counter fr (gs_fit_reason) stands for: the one table gs_reason_string and gs_fit_error_string render
std::string reason_text(int fr, const char* const* scalar_names) {
  switch (fr) {
    case GS_FR_FIT_PODS: return "Too many pods";
    case GS_FR_FIT_CPU: return "Insufficient cpu";
    case GS_FR_FIT_MEMORY: return "Insufficient memory";
    case GS_FR_FIT_EPHEMERAL: return "Insufficient ephemeral-storage";
    default: break;
  }
  if (fr >= GS_FR_FIT_SCALAR0 && fr < GS_FR_FIT_SCALAR0 + 4) {
    const int s = fr - GS_FR_FIT_SCALAR0;
    return std::string("Insufficient ") + (scalar_names && scalar_names[s] ? scalar_names[s] : kScalarDefault[s]);
  }
  if (fr >= GS_FR_LA_CPU && fr <= GS_FR_LA_MEMORY_AGG) {
    const int d = fr - GS_FR_LA_CPU;   // bit 0: memory, bit 1: the aggregated form
    return std::string("node(s) ") + ((d & 1) ? "memory" : "cpu") +
           ((d & 2) ? " aggregated usage exceed threshold" : " usage exceed threshold");
  }
  if (fr > GS_FR_NUMA0 && fr < GS_NUM_FIT_REASONS) return kNuma[fr - GS_FR_NUMA0].msg;
  return "";
}

}  // namespace

namespace gs {
int fit_reason_status(int fr) {
  if (fr < 0 || fr >= GS_NUM_FIT_REASONS) return kSuccess;
  return fr > GS_FR_NUMA0 ? kNuma[fr - GS_FR_NUMA0].code : kUnschedulable;
}
}  // namespace gs

extern "C" int gs_reason_string(uint32_t code, uint32_t scalar_mask, const char* const* scalar_names, char* buf,
                                size_t len) {
  const uint32_t known = GS_FAIL_FIT_PODS | GS_FAIL_FIT_CPU | GS_FAIL_FIT_MEMORY | GS_FAIL_FIT_EPHEMERAL |
                         GS_FAIL_FIT_SCALAR | GS_FAIL_LOADAWARE | GS_FAIL_NUMA_MASK | GS_FAIL_LA_MEMORY |
                         GS_FAIL_LA_AGGREGATED;
  const uint32_t numa = (code & GS_FAIL_NUMA_MASK) >> GS_FAIL_NUMA_SHIFT;
  if ((code & ~known) || numa >= sizeof(kNuma) / sizeof(kNuma[0])) return GS_EINVAL;
  if ((code & (GS_FAIL_LA_MEMORY | GS_FAIL_LA_AGGREGATED)) && !(code & GS_FAIL_LOADAWARE)) return GS_EINVAL;
  std::string msg;
  int status = kSuccess;
  const uint32_t fit = code & (GS_FAIL_FIT_PODS | GS_FAIL_FIT_CPU | GS_FAIL_FIT_MEMORY | GS_FAIL_FIT_EPHEMERAL |
                               GS_FAIL_FIT_SCALAR);
  if (fit) {   // the first plugin of the Filter order fails: its reasons, in fitsRequest order
    status = kUnschedulable;
    auto add = [&](const std::string& r) { msg += (msg.empty() ? "" : ", ") + r; };
    for (int b = 0; b < 4; ++b)   // GS_FAIL_FIT_PODS .. _EPHEMERAL are bits GS_FR_FIT_PODS .. _EPHEMERAL
      if (code >> b & 1u) add(reason_text(b, scalar_names));
    if (code & GS_FAIL_FIT_SCALAR)
      for (int s = 3; s < 7; ++s)
        if (scalar_mask >> s & 1u) add(reason_text(GS_FR_FIT_SCALAR0 + s - 3, scalar_names));
  } else if (code & GS_FAIL_LOADAWARE) {
    status = kUnschedulable;
    msg = reason_text(GS_FR_LA_CPU + ((code & GS_FAIL_LA_MEMORY) ? 1 : 0) + ((code & GS_FAIL_LA_AGGREGATED) ? 2 : 0),
                      scalar_names);
  } else if (numa) {
    status = kNuma[numa].code;
    msg = reason_text(GS_FR_NUMA0 + (int)numa, scalar_names);
  }
  if (buf && len) {
    const size_t n = msg.size() < len - 1 ? msg.size() : len - 1;
    memcpy(buf, msg.data(), n);
    buf[n] = '\0';
  }
  return status;
}

// [upstream] framework/types.go FitError.Error(): "0/<NumAllNodes> nodes are available: " + the histogram of the
// NodeToStatusMap's reasons as "<count> <reason>" strings, sorted (sort.Strings: bytewise), joined by ", ", + ".".
extern "C" int gs_fit_error_string(const gs_fit_diagnosis* d, const char* const* scalar_names, char* buf, size_t len) {
  if (!d) return GS_EINVAL;
  std::string msg;
  if (d->valid) {
    std::map<std::string, uint64_t> hist;   // counts of reasons that share a text are merged
    for (int fr = 0; fr < GS_NUM_FIT_REASONS; ++fr) {
      if (!d->reasons[fr]) continue;
      const std::string t = reason_text(fr, scalar_names);
      if (!t.empty()) hist[t] += d->reasons[fr];
    }
    std::vector<std::string> entries;
    for (const auto& e : hist) entries.push_back(std::to_string(e.second) + " " + e.first);
    std::sort(entries.begin(), entries.end());
    msg = "0/" + std::to_string(d->num_all_nodes) + " nodes are available: ";
    for (size_t i = 0; i < entries.size(); ++i) msg += (i ? ", " : "") + entries[i];
    msg += ".";
  }
  if (buf && len) {
    const size_t n = msg.size() < len - 1 ? msg.size() : len - 1;
    memcpy(buf, msg.data(), n);
    buf[n] = '\0';
  }
  return (int)msg.size();
}
