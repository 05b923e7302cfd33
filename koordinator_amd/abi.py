"""ctypes mirror of include/gpuscore.h (the drop-in C-ABI of libgpuscore).

Struct layouts here must match the header byte for byte; tests/test_abi.py checks the sizes
against the compiled library (gs_abi_sizes) and that every declared symbol is exported.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

GS_ABI_VERSION = 6
GS_NUM_RES = 8
GS_RES_CPU, GS_RES_MEMORY, GS_RES_EPHEMERAL = 0, 1, 2
GS_RES_BATCH_CPU, GS_RES_BATCH_MEMORY, GS_RES_MID_CPU, GS_RES_MID_MEMORY = 3, 4, 5, 6
GS_SCALAR_RES_MASK = 0x78

GS_PRIO_NONE, GS_PRIO_PROD, GS_PRIO_MID, GS_PRIO_BATCH, GS_PRIO_FREE = 0, 1, 2, 3, 4
GS_AGG_NONE, GS_AGG_AVG, GS_AGG_P50, GS_AGG_P90, GS_AGG_P95, GS_AGG_P99 = -1, 0, 1, 2, 3, 4
GS_NUM_AGG_TYPES = 5
GS_MAX_AGG_USAGES = 4
GS_USAGE_CPU, GS_USAGE_MEMORY, GS_USAGE_OTHER = 0x1, 0x2, 0x80
GS_POD_DAEMONSET, GS_POD_TERMINATED = 0x1, 0x2
GS_NODE_CUSTOM_THRESHOLDS, GS_NODE_CUSTOM_AGGREGATED = 0x1, 0x2

GS_PLUGIN_FIT, GS_PLUGIN_LOADAWARE, GS_PLUGIN_NUMA, GS_NUM_PLUGINS = 0, 1, 2, 3
GS_ENABLE_FIT_FILTER, GS_ENABLE_FIT_SCORE = 0x1, 0x2
GS_ENABLE_LA_FILTER, GS_ENABLE_LA_SCORE = 0x4, 0x8
GS_ENABLE_NUMA_FILTER, GS_ENABLE_NUMA_SCORE = 0x10, 0x20
GS_ENABLE_LA_FIT = 0xF
GS_ENABLE_ALL = 0x3F

# NodeNUMAResource vocabulary
GS_MAX_NUMA, GS_MAX_CPUS, GS_CPU_WORDS = 4, 256, 4
GS_QOS_NONE, GS_QOS_LSE, GS_QOS_LSR, GS_QOS_LS, GS_QOS_BE, GS_QOS_SYSTEM = 0, 1, 2, 3, 4, 5
CPU_BIND = {"": 0, "Default": 1, "FullPCPUs": 2, "SpreadByPCPUs": 3, "ConstrainedBurst": 4}
CPU_EXCLUSIVE = {"": 0, "None": 0, "PCPULevel": 1, "NUMANodeLevel": 2}
NODE_CPU_BIND = {"": 0, "None": 0, "FullPCPUsOnly": 1, "SpreadByPCPUs": 2}
NUMA_POLICY = {"": 0, "BestEffort": 1, "Restricted": 2, "SingleNUMANode": 3}
GS_NUMA_POLICY_NONE, GS_NUMA_POLICY_BEST_EFFORT, GS_NUMA_POLICY_RESTRICTED, GS_NUMA_POLICY_SINGLE_NUMA_NODE = 0, 1, 2, 3
NUMA_ALLOC = {"": 0, "MostAllocated": 1, "LeastAllocated": 2, "DistributeEvenly": 3}
GS_SCORING_LEAST_ALLOCATED, GS_SCORING_MOST_ALLOCATED = 0, 1
GS_FAIL_NUMA_SHIFT, GS_FAIL_NUMA_MASK = 6, 0x3C0
GS_FAIL_LA_MEMORY, GS_FAIL_LA_AGGREGATED = 0x400, 0x800
# gs_numa_reason (the NodeNUMAResource reason in bits GS_FAIL_NUMA_MASK)
(GS_NUMA_OK, GS_NUMA_INVALID_REQUESTED_CPUS, GS_NUMA_INVALID_AMP_RATIO, GS_NUMA_AVAILABLE_CPUS_ERROR,
 GS_NUMA_INSUFFICIENT_AMP_CPU, GS_NUMA_INVALID_TOPOLOGY, GS_NUMA_BIND_POLICY_CONFLICT, GS_NUMA_SMT_ALIGNMENT,
 GS_NUMA_ALLOCATE_FAILED, GS_NUMA_MISSING_NUMA_RESOURCES, GS_NUMA_AFFINITY_ERROR, GS_NUMA_ADMIT_ALLOCATE_FAILED) = range(12)


def reason_string(code: int, scalar_mask: int = 0) -> tuple[int, str]:
    """(framework.Code, message) of the reference's Filter status for a gs_evaluate failure code (gs_reason_string)."""
    buf = C.create_string_buffer(512)
    st = load().gs_reason_string(int(code), int(scalar_mask), None, buf, len(buf))
    return st, buf.value.decode()
NUMA_REASONS = ["OK", "InvalidRequestedCPUs", "InvalidAmplificationRatio", "AvailableCPUsError",
                "InsufficientAmplifiedCPU", "InvalidCPUTopology", "CPUBindPolicyConflict", "SMTAlignment",
                "AllocateFailed", "MissingNUMAResources", "NUMATopologyAffinity", "AdmitAllocateFailed"]
GS_PLACED_NUMA, GS_PLACED_CPUSET, GS_PLACED_AFFINITY_SHIFT = 0x2, 0x4, 8
# gs_fit_reason: the counters of a gs_fit_diagnosis (NodeNUMAResource reason r at GS_FR_NUMA0 + r)
GS_FR_FIT_PODS, GS_FR_FIT_CPU, GS_FR_FIT_MEMORY, GS_FR_FIT_EPHEMERAL, GS_FR_FIT_SCALAR0 = 0, 1, 2, 3, 4
GS_FR_LA_CPU, GS_FR_LA_MEMORY, GS_FR_LA_CPU_AGG, GS_FR_LA_MEMORY_AGG, GS_FR_NUMA0 = 8, 9, 10, 11, 11
GS_NUM_FIT_REASONS = 23


def fit_error_message(diag, scalar_names=None) -> str:
    """[upstream] FitError.Error() of one gs_fit_diagnosis (a FIT_DIAGNOSIS_DTYPE record or a GsFitDiagnosis):
    gs_fit_error_string. scalar_names: the names of resource slots 3..6 (None: the defaults). '' when not valid."""
    d = diag if isinstance(diag, GsFitDiagnosis) else GsFitDiagnosis.from_buffer_copy(
        np.ascontiguousarray(np.atleast_1d(diag), FIT_DIAGNOSIS_DTYPE)[:1].tobytes())
    names = None
    if scalar_names is not None:
        names = (C.c_char_p * 4)(*[n.encode() for n in scalar_names])
    n = load().gs_fit_error_string(C.byref(d), names, None, 0)
    if n < 0:
        raise ValueError(f"gs_fit_error_string: {n}")
    buf = C.create_string_buffer(n + 1)
    load().gs_fit_error_string(C.byref(d), names, buf, len(buf))
    return buf.value.decode()


def status_code(word: int) -> int:
    """GS_STATUS_CODE: the GS_FAIL_* bits of a status word (what reason_string takes)."""
    return int(word) & 0x0FFF


def status_scalar_mask(word: int) -> int:
    """GS_STATUS_SCALAR_MASK: the scalar_mask of a status word, exactly the resource slots 3..6 that were short."""
    return ((int(word) >> 12) & 0xF) << 3


def status_framework_code(word: int) -> int:
    """gs_status_framework_code: 0 Success, 1 Unschedulable, 2 UnschedulableAndUnresolvable."""
    return load().gs_status_framework_code(int(word))


def preemption_candidates(row, cap: int | None = None) -> tuple[int, np.ndarray]:
    """gs_preemption_candidates over one status row: (count, the first min(count, cap) nodes, ascending)."""
    row = np.ascontiguousarray(row, dtype=np.uint16)
    cap = len(row) if cap is None else int(cap)
    nodes = np.zeros(max(cap, 1), np.uint32)
    n = load().gs_preemption_candidates(ptr(row), len(row), ptr(nodes), cap)
    if n < 0:
        raise ValueError(f"gs_preemption_candidates: {n}")
    return n, nodes[:min(n, cap)]


GS_FAIL_FIT_PODS, GS_FAIL_FIT_CPU, GS_FAIL_FIT_MEMORY = 0x01, 0x02, 0x04
GS_FAIL_FIT_EPHEMERAL, GS_FAIL_FIT_SCALAR, GS_FAIL_LOADAWARE = 0x08, 0x10, 0x20
GS_PLACED_SLOWPATH = 0x1

GS_OK, GS_EINVAL, GS_EDEVICE, GS_ENOMEM, GS_EUNSUPPORTED, GS_ECOMM, GS_ESTATE = 0, -1, -2, -3, -4, -5, -6

i64, u64, i32, u32 = C.c_int64, C.c_uint64, C.c_int32, C.c_uint32


class GsPod(C.Structure):
    _fields_ = [
        ("uid", u64), ("name_key", u64),
        ("requests", i64 * GS_NUM_RES), ("limits", i64 * GS_NUM_RES),
        ("nonzero_requests", i64 * 2),
        ("request_mask", u32), ("priority_class", i32), ("flags", u32),
        ("qos_class", i32), ("required_cpu_bind_policy", i32), ("preferred_cpu_bind_policy", i32),
        ("preferred_cpu_exclusive_policy", i32), ("pad0", i32),
    ]


class GsNode(C.Structure):
    _fields_ = [
        ("allocatable", i64 * GS_NUM_RES), ("requested", i64 * GS_NUM_RES),
        ("nonzero_requested", i64 * 2),
        ("allowed_pod_number", i64), ("pod_count", i64),
        ("raw_allocatable", i64 * 2),
        ("raw_allocatable_mask", u32), ("custom_flags", u32),
        ("custom_usage_thresholds", i64 * 2), ("custom_prod_usage_thresholds", i64 * 2),
        ("custom_agg_usage_thresholds", i64 * 2),
        ("custom_usage_mask", u32), ("custom_prod_usage_mask", u32), ("custom_agg_usage_mask", u32),
        ("custom_agg_type", i32), ("custom_agg_duration_ns", i64),
    ]


class GsCpuTopology(C.Structure):
    _fields_ = [("num_cpus", i32), ("pad0", i32), ("core_id", i32 * GS_MAX_CPUS),
                ("socket_id", C.c_uint8 * GS_MAX_CPUS), ("node_id", C.c_uint8 * GS_MAX_CPUS)]


class GsNumaZone(C.Structure):
    _fields_ = [("node_id", i32), ("mask", u32), ("cpu_milli", i64), ("memory", i64)]


class GsNodeNuma(C.Structure):
    _fields_ = [
        ("has_options", i32), ("topology", i32), ("max_ref_count", i32), ("node_cpu_bind_policy", i32),
        ("numa_topology_policy", i32), ("numa_allocate_strategy", i32),
        ("cpu_amplification_ratio", C.c_double), ("node_cpu_amplification_ratio", C.c_double),
        ("node_amplification_invalid", i32), ("num_zones", i32), ("zones", GsNumaZone * GS_MAX_NUMA),
        ("reserved_cpus", u64 * GS_CPU_WORDS),
    ]


class GsPodAllocation(C.Structure):
    _fields_ = [("uid", u64), ("cpuset", u64 * GS_CPU_WORDS), ("cpu_exclusive_policy", i32), ("num_numa", i32),
                ("numa", GsNumaZone * GS_MAX_NUMA)]


class GsNumaArgs(C.Structure):
    _fields_ = [("default_cpu_bind_policy", i32), ("scoring_type", i32), ("numa_scoring_type", i32), ("pad0", i32),
                ("resource_weights", i64 * GS_NUM_RES)]


class GsUsage(C.Structure):
    _fields_ = [("cpu_milli", i64), ("memory", i64), ("mask", u32), ("pad0", u32)]


class GsAggUsage(C.Structure):
    _fields_ = [("duration_ns", i64), ("type_mask", u32), ("pad0", u32), ("usage", GsUsage * GS_NUM_AGG_TYPES)]


class GsNodeMetric(C.Structure):
    _fields_ = [
        ("exists", i32), ("has_update_time", i32), ("update_time_ns", i64),
        ("has_report_interval", i32), ("has_node_metric", i32), ("report_interval_s", i64),
        ("node_usage", GsUsage), ("n_aggregated", i32), ("pad0", u32),
        ("aggregated", GsAggUsage * GS_MAX_AGG_USAGES),
    ]


class GsPodMetric(C.Structure):
    _fields_ = [("name_key", u64), ("in_lister", i32), ("priority_class", i32), ("usage", GsUsage)]


class GsLoadAwareArgs(C.Structure):
    _fields_ = [
        ("filter_expired_node_metrics", i32), ("has_node_metric_expiration", i32),
        ("node_metric_expiration_seconds", i64),
        ("resource_weights", i64 * 2), ("usage_thresholds", i64 * 2),
        ("prod_usage_thresholds", i64 * 2), ("estimated_scaling_factors", i64 * 2),
        ("resource_weights_mask", u32), ("usage_thresholds_mask", u32),
        ("prod_usage_thresholds_mask", u32), ("estimated_scaling_factors_mask", u32),
        ("score_according_prod_usage", i32), ("has_aggregated", i32),
        ("agg_usage_thresholds", i64 * 2), ("agg_usage_thresholds_mask", u32),
        ("agg_usage_type", i32), ("agg_usage_duration_ns", i64),
        ("agg_score_type", i32), ("pad0", i32), ("agg_score_duration_ns", i64),
    ]


class GsFitArgs(C.Structure):
    _fields_ = [("resource_weights", i64 * GS_NUM_RES)]


class GsConfig(C.Structure):
    _fields_ = [
        ("abi_version", u32), ("device", i32), ("num_nodes", u32), ("enabled", u32),
        ("plugin_weights", i64 * GS_NUM_PLUGINS),
        ("loadaware", GsLoadAwareArgs), ("fit", GsFitArgs), ("numa", GsNumaArgs),
        ("seed", u64), ("batch_size", u32), ("cand_cap", u32),
        ("sample_nodes", i32), ("percentage_of_nodes_to_score", i32),
    ]


class GsPlacement(C.Structure):
    _fields_ = [("node", i32), ("feasible", u32), ("score", i64), ("ties", u32), ("flags", u32)]


class GsFitDiagnosis(C.Structure):
    _fields_ = [("valid", u32), ("num_all_nodes", u32), ("failed_nodes", u32), ("unresolvable_nodes", u32),
                ("reasons", u32 * 24)]


class GsStatusMap(C.Structure):
    """gs_status_map: the per-node status rows of a call's FitError pods (gs_schedule_diag_nodes)."""
    _fields_ = [("words", C.c_void_p), ("cap_rows", u32), ("row_of", C.c_void_p), ("rows_used", u32),
                ("rows_dropped", u32)]


class GsStats(C.Structure):
    _fields_ = [
        ("batches", u64), ("pods", u64), ("cuts", u64), ("slowpath_pods", u64),
        ("eval_launches", u64), ("eval_pairs", u64),
        ("eval_ms", C.c_double), ("cand_ms", C.c_double), ("commit_ms", C.c_double), ("exchange_ms", C.c_double),
        ("node_row_bytes", u64), ("shard_begin", u32), ("shard_end", u32),
        ("next_start_node_index", u32), ("pad0", u32), ("delta_rows", u64), ("delta_bytes", u64),
    ]


class GsKv(C.Structure):
    _fields_ = [("key", C.c_char_p), ("value", C.c_char_p)]


GS_QUOTA_DIMS = 8
GS_QUOTA_RUNTIME, GS_QUOTA_CHECK_PARENT, GS_QUOTA_NON_PREEMPTIBLE = 1, 2, 4
GS_QUOTA_ADMIT, GS_QUOTA_INSUFFICIENT, GS_QUOTA_INSUFFICIENT_NON_PREEMPTIBLE = 0, 1, 2


class GsQuotaGroup(C.Structure):
    _fields_ = [("parent", i32), ("allow_lent", u32), ("max_mask", u32), ("min_mask", u32),
                ("max", i64 * GS_QUOTA_DIMS), ("min", i64 * GS_QUOTA_DIMS), ("guaranteed", i64 * GS_QUOTA_DIMS),
                ("shared_weight", i64 * GS_QUOTA_DIMS), ("request", i64 * GS_QUOTA_DIMS),
                ("used", i64 * GS_QUOTA_DIMS), ("non_preemptible_used", i64 * GS_QUOTA_DIMS)]


class GsQuotaStatus(C.Structure):
    _fields_ = [("code", i32), ("group", i32), ("exceed_mask", u32), ("depth", u32),
                ("used", i64 * GS_QUOTA_DIMS)]


# ---- ElasticQuota PostFilter: the resident-pod table and the preemption dry run ----
GS_MAX_NODE_PODS = 128
GS_RESIDENT_NON_PREEMPTIBLE, GS_RESIDENT_QUOTA_TRACKED, GS_RESIDENT_TERMINATING = 0x1, 0x2, 0x4
GS_PREEMPT_NEVER = 0x1
(GS_PREEMPT_NOMINATED, GS_PREEMPT_NOT_ELIGIBLE, GS_PREEMPT_NO_POTENTIAL_NODES, GS_PREEMPT_NO_CANDIDATES,
 GS_PREEMPT_ERROR) = range(5)
(GS_PNODE_NOT_POTENTIAL, GS_PNODE_CANDIDATE, GS_PNODE_NO_VICTIMS, GS_PNODE_UNFIT, GS_PNODE_FITS,
 GS_PNODE_ERROR) = range(6)


class GsResidentPod(C.Structure):
    _fields_ = [("uid", u64), ("start_time_ns", i64), ("requests", i64 * GS_NUM_RES),
                ("quota_request", i64 * GS_QUOTA_DIMS), ("quota_request_mask", u32), ("priority", i32),
                ("quota", i32), ("flags", u32)]


class GsPreemptor(C.Structure):
    _fields_ = [("pod", GsPod), ("priority", i32), ("quota", i32), ("quota_request", i64 * GS_QUOTA_DIMS),
                ("quota_request_mask", u32), ("limit_mask", u32), ("used", i64 * GS_QUOTA_DIMS),
                ("used_limit", i64 * GS_QUOTA_DIMS), ("flags", u32), ("nominated_node", i32), ("row", i32),
                ("pad0", i32)]


class GsPreemptResult(C.Structure):
    _fields_ = [("status", i32), ("node", i32), ("num_victims", u32), ("num_potential", u32),
                ("num_candidates", u32), ("num_errors", u32), ("victims", u64 * GS_MAX_NODE_PODS)]


class GsPreemptDetail(C.Structure):
    _fields_ = [("node_status", C.c_void_p), ("victim_bits", C.c_void_p)]


class GsPreemptCandidate(C.Structure):
    _fields_ = [("node", i32), ("first_priority", i32), ("sum_priorities", i64), ("num_victims", u32), ("pad0", u32),
                ("earliest_start_ns", i64)]


# PodDisruptionBudgets in the dry run (gs_preempt_dry_run_pdb)
GS_MAX_PDBS, GS_MAX_POD_PDBS, GS_PDB_NONE, GS_PDB_UNLIMITED = 65535, 4, 0xFFFF, 2**31 - 1


class GsPreemptResultPdb(C.Structure):
    _fields_ = [("status", i32), ("node", i32), ("num_victims", u32), ("num_potential", u32),
                ("num_candidates", u32), ("num_errors", u32), ("num_pdb_violations", u32), ("pad0", u32),
                ("victims", u64 * GS_MAX_NODE_PODS)]


class GsPreemptDetailPdb(C.Structure):
    _fields_ = [("node_status", C.c_void_p), ("victim_bits", C.c_void_p), ("violating_bits", C.c_void_p),
                ("pdb_violations", C.c_void_p)]


class GsPreemptCandidatePdb(C.Structure):
    _fields_ = [("node", i32), ("first_priority", i32), ("sum_priorities", i64), ("num_victims", u32),
                ("num_pdb_violations", u32), ("earliest_start_ns", i64)]


def preempt_pick_node_pdb(cands) -> int:
    """gs_preempt_pick_node_pdb over PREEMPT_CANDIDATE_PDB_DTYPE records: the index of the pick, -1 for none."""
    cands = np.ascontiguousarray(cands, dtype=PREEMPT_CANDIDATE_PDB_DTYPE)
    return load().gs_preempt_pick_node_pdb(ptr(cands), len(cands))


def preempt_pick_node(cands) -> int:
    """gs_preempt_pick_node over PREEMPT_CANDIDATE_DTYPE records: the index of the pick, -1 for none."""
    cands = np.ascontiguousarray(cands, dtype=PREEMPT_CANDIDATE_DTYPE)
    return load().gs_preempt_pick_node(ptr(cands), len(cands))


# ---- Reservation + DeviceShare ----
GS_NUM_GPU_RES = 3
GS_GPU_CORE, GS_GPU_MEMORY_RATIO, GS_GPU_MEMORY = 0, 1, 2
GS_NUM_GPU_NAMES = 5
GPU_NAMES = {"nvidia.com/gpu": 0, "koordinator.sh/gpu": 1, "koordinator.sh/gpu-core": 2,
             "koordinator.sh/gpu-memory": 3, "koordinator.sh/gpu-memory-ratio": 4}
GS_MAX_GPUS = 8
GS_MAX_XRES = 8   # registered extended resources (any vendor name outside the fixed slots / GPU names)
RSV_POLICY = {"": 0, "Default": 0, "Aligned": 1, "Restricted": 2}
GS_EXT_DEVICESHARE, GS_EXT_RESERVATION = 0x1, 0x2
GS_POD_EVENT_ADD, GS_POD_EVENT_UPDATE, GS_POD_EVENT_DELETE = 0, 1, 2
GS_EXT_FAIL_DEVICE, GS_EXT_FAIL_RESERVATION, GS_EXT_FAIL_POD = 0x1000, 0x2000, 0x4000


# gs_commit_counters (gs_debug_commit_counters): uint64 words in this order
COMMIT_COUNTER_KEYS = ("decisions", "rollbacks", "rollback_depth", "restored_rows", "full_row", "old_path",
                       "general_path", "list_beyond_32", "list_beyond_64", "pending_ge", "pending_ge_rollbacks",
                       "pending_gt", "pending_gt_rollbacks", "split_late_landings", "split_rerecords",
                       "split_excluded_ties", "split_settled_early", "prep_records", "prep_old_path",
                       "prep_general_path", "prep_list_beyond_32", "prep_list_beyond_64", "est_decisions", "est_prev_gt",
                       "est_prev_eq", "est_position_moved", "split_batches", "single_batches")

EXT_ROW_KEYS = ("feasible", "base", "ds_raw", "rs_raw", "total")          # GS_EXT_ROW_*
EXT_ROWS_RESULT_KEYS = ("node", "score", "ties", "feasible_count", "pref_node", "ds_norm", "rs_norm",
                        "fail_code")                                       # GS_EXT_ROWS_*


def ext_rows_dict(rows, nom, res) -> dict:
    """The (rows[5][N], nominated_uid[N], result[8]) triple of gs_debug_ext_rows as a dict of arrays and ints."""
    out = {k: rows[i] for i, k in enumerate(EXT_ROW_KEYS)}
    out["nominated_uid"] = nom
    out.update({k: int(res[i]) for i, k in enumerate(EXT_ROWS_RESULT_KEYS)})
    return out


class GsGpuDevice(C.Structure):
    _fields_ = [("minor", i32), ("has_info", i32), ("numa_node", i32), ("pad", i32), ("total", i64 * GS_NUM_GPU_RES),
                ("used", i64 * GS_NUM_GPU_RES)]


class GsNodeDevices(C.Structure):
    _fields_ = [("has_device", i32), ("num_gpus", i32), ("gpus", GsGpuDevice * GS_MAX_GPUS),
                ("allocatable", i64 * GS_NUM_GPU_NAMES), ("requested", i64 * GS_NUM_GPU_NAMES),
                ("xres_allocatable", i64 * GS_MAX_XRES), ("xres_requested", i64 * GS_MAX_XRES)]


class GsReservation(C.Structure):
    _fields_ = [("uid", u64), ("owner_key", u64), ("node", u32), ("allocate_policy", i32), ("order", i64),
                ("available", i32), ("unschedulable", i32), ("allocate_once", i32), ("assigned_pods", i32),
                ("allocatable", i64 * GS_NUM_RES), ("allocated", i64 * GS_NUM_RES), ("allocatable_mask", u32),
                ("allocated_mask", u32), ("resource_names_mask", u32), ("pad0", u32)]


class GsPodExt(C.Structure):
    _fields_ = [("reservation_owner", u64), ("reservation_required", i32), ("gpu_request_mask", u32),
                ("gpu_requests", i64 * GS_NUM_GPU_NAMES), ("xres_request_mask", u32), ("pad0", u32),
                ("xres_requests", i64 * GS_MAX_XRES)]


class GsExtArgs(C.Structure):
    _fields_ = [("enabled", u32), ("device_scoring_type", i32), ("device_weights", i64 * GS_NUM_GPU_RES),
                ("weight_deviceshare", i64), ("weight_reservation", i64), ("fit_ignored_gpu_names", u32),
                ("fit_ignored_xres", u32)]


class GsExtPlacement(C.Structure):
    _fields_ = [("reservation_uid", u64), ("gpu_minor_mask", u32), ("gpu_count", i32),
                ("gpu_per_instance", i64 * GS_NUM_GPU_RES), ("deviceshare_score", i32), ("reservation_score", i32),
                ("fail_code", u32), ("pad0", u32)]


# ---- DeviceShare device types beyond GPU: RDMA and FPGA (gs_schedule_ext_aux) ----
GS_AUX_RDMA, GS_AUX_FPGA, GS_NUM_AUX_TYPES = 0, 1, 2
GS_MAX_AUX_DEVICES = 8
GS_AUX_STRATEGY_NONE, GS_AUX_APPLY_FOR_ALL, GS_AUX_REQUESTS_AS_COUNT = 0, 1, 2
AUX_NAMES = {"koordinator.sh/rdma": GS_AUX_RDMA, "koordinator.sh/fpga": GS_AUX_FPGA}
AUX_STRATEGY = {"": 0, "ApplyForAll": 1, "RequestsAsCount": 2}


class GsAuxDevice(C.Structure):
    _fields_ = [("minor", i32), ("has_info", i32), ("numa_node", i32), ("pad", i32), ("total", i64), ("used", i64)]


class GsNodeAuxDevices(C.Structure):
    _fields_ = [("num", i32 * GS_NUM_AUX_TYPES), ("dev", (GsAuxDevice * GS_MAX_AUX_DEVICES) * GS_NUM_AUX_TYPES)]


class GsPodAux(C.Structure):
    _fields_ = [("request", i64 * GS_NUM_AUX_TYPES), ("strategy", i32 * GS_NUM_AUX_TYPES),
                ("device_exclusive", i32 * GS_NUM_AUX_TYPES)]


class GsAuxPlacement(C.Structure):
    _fields_ = [("minor_mask", u32 * GS_NUM_AUX_TYPES), ("count", i32 * GS_NUM_AUX_TYPES),
                ("per_instance", i64 * GS_NUM_AUX_TYPES)]


ALLGATHER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t)

# numpy dtypes with the exact C layout (for bulk construction of node/pod arrays)
class GsMergeCase(C.Structure):
    _fields_ = [("lc", u32), ("totc", u32), ("lm", u32), ("totm", u32), ("nz", i32), ("policy", i32),
                ("nil_hints", i32), ("has_cpu", i32), ("has_mem", i32), ("tot_c_any", i32), ("tot_m_any", i32),
                ("score", i32 * 15), ("gpu_hints", u32), ("pad", i32)]


class GsMergeResult(C.Structure):
    _fields_ = [("admit", i32), ("aff_has", i32), ("aff", u32), ("pad", i32)]


class GsGangArgs(C.Structure):
    _fields_ = [("default_timeout_ns", i64), ("skip_check_schedule_cycle", i32), ("pad", i32)]


class GsGangSpec(C.Structure):
    _fields_ = [("gang_id", u64), ("min_member", i32), ("total_children", i32), ("mode", i32), ("match_policy", i32),
                ("wait_time_ns", i64), ("create_time_ns", i64), ("group_n", u32), ("pad", u32), ("group", u64 * 8)]


class GsGangInfo(C.Structure):
    _fields_ = [(n, i32) for n in ("has_init", "min_member", "total_children", "mode", "match_policy", "schedule_cycle",
                                   "schedule_cycle_valid", "once_resource_satisfied", "children", "waiting", "bound",
                                   "pad")] + [("wait_time_ns", i64)]


class GsTopScore(C.Structure):
    _fields_ = [("node", u32), ("total", C.c_int16), ("plugin", C.c_int16 * GS_NUM_PLUGINS)]


class GsTopScores(C.Structure):
    _fields_ = [("rows", C.c_void_p), ("count", C.c_void_p), ("topn", u32)]


GS_MAX_TOP_SCORES = 64
# the score plugins of a gs_top_score row: (index in plugin[] and gs_config.plugin_weights, gs_config.enabled bit, name)
SCORE_PLUGINS = ((GS_PLUGIN_FIT, GS_ENABLE_FIT_SCORE, "NodeResourcesFit"),
                 (GS_PLUGIN_LOADAWARE, GS_ENABLE_LA_SCORE, "LoadAwareScheduling"),
                 (GS_PLUGIN_NUMA, GS_ENABLE_NUMA_SCORE, "NodeNUMAResource"))


def debug_scores_string(topn: int, pod_ref: str, node_names, plugin_names, scores) -> str:
    """gs_debug_scores_string: frameworkext/debug.go debugScores' markdown table. scores[plugin][node]: weighted."""
    sc = np.ascontiguousarray(scores, dtype=np.int64).reshape(len(plugin_names), len(node_names))
    nn = (C.c_char_p * max(1, len(node_names)))(*[n.encode() for n in node_names])
    pn = (C.c_char_p * max(1, len(plugin_names)))(*[n.encode() for n in plugin_names])
    args = (int(topn), pod_ref.encode(), nn, len(node_names), pn, len(plugin_names), ptr(sc))
    n = load().gs_debug_scores_string(*args, None, 0)
    if n < 0:
        raise ValueError(f"gs_debug_scores_string: {n}")
    buf = C.create_string_buffer(n + 1)
    load().gs_debug_scores_string(*args, buf, len(buf))
    return buf.value.decode()


def debug_scores_table(rows, cfg, pod_ref: str, node_names) -> str:
    """The --debug-scores table of one pod from its gs_top_score rows (TOP_SCORE_DTYPE, already sorted and cut):
    a column per enabled score plugin of cfg (a GsConfig) holding plugin x weight, as RunScorePlugins leaves them.
    node_names: the name of every node of the cluster, by node index."""
    cols = [(k, name) for k, bit, name in SCORE_PLUGINS if cfg.enabled & bit]
    names = [node_names[int(n)] for n in rows["node"]]
    sc = np.zeros((len(cols), len(rows)), np.int64)
    for j, (k, _) in enumerate(cols):
        sc[j] = rows["plugin"][:, k].astype(np.int64) * int(cfg.plugin_weights[k])
    return debug_scores_string(len(rows), pod_ref, names, [name for _, name in cols], sc)


MERGE_CASE_DTYPE = np.dtype(GsMergeCase)
MERGE_RESULT_DTYPE = np.dtype(GsMergeResult)
POD_DTYPE = np.dtype(GsPod)
NODE_DTYPE = np.dtype(GsNode)
METRIC_DTYPE = np.dtype(GsNodeMetric)
POD_METRIC_DTYPE = np.dtype(GsPodMetric)
PLACEMENT_DTYPE = np.dtype(GsPlacement)
FIT_DIAGNOSIS_DTYPE = np.dtype(GsFitDiagnosis)
TOP_SCORE_DTYPE = np.dtype(GsTopScore)
TOPOLOGY_DTYPE = np.dtype(GsCpuTopology)
NODE_NUMA_DTYPE = np.dtype(GsNodeNuma)
POD_ALLOCATION_DTYPE = np.dtype(GsPodAllocation)
NODE_DEVICES_DTYPE = np.dtype(GsNodeDevices)
RESERVATION_DTYPE = np.dtype(GsReservation)
POD_EXT_DTYPE = np.dtype(GsPodExt)
EXT_PLACEMENT_DTYPE = np.dtype(GsExtPlacement)
NODE_AUX_DEVICES_DTYPE = np.dtype(GsNodeAuxDevices)
POD_AUX_DTYPE = np.dtype(GsPodAux)
AUX_PLACEMENT_DTYPE = np.dtype(GsAuxPlacement)
RESIDENT_POD_DTYPE = np.dtype(GsResidentPod)
PREEMPTOR_DTYPE = np.dtype(GsPreemptor)
PREEMPT_RESULT_DTYPE = np.dtype(GsPreemptResult)
PREEMPT_CANDIDATE_DTYPE = np.dtype(GsPreemptCandidate)
PREEMPT_RESULT_PDB_DTYPE = np.dtype(GsPreemptResultPdb)
PREEMPT_CANDIDATE_PDB_DTYPE = np.dtype(GsPreemptCandidatePdb)

STRUCT_SIZES = {
    "gs_pod": C.sizeof(GsPod), "gs_node": C.sizeof(GsNode), "gs_node_metric": C.sizeof(GsNodeMetric),
    "gs_pod_metric": C.sizeof(GsPodMetric), "gs_config": C.sizeof(GsConfig),
    "gs_placement": C.sizeof(GsPlacement), "gs_stats": C.sizeof(GsStats),
    "gs_loadaware_args": C.sizeof(GsLoadAwareArgs), "gs_cpu_topology": C.sizeof(GsCpuTopology),
    "gs_node_numa": C.sizeof(GsNodeNuma), "gs_pod_allocation": C.sizeof(GsPodAllocation),
    "gs_numa_args": C.sizeof(GsNumaArgs), "gs_quota_group": C.sizeof(GsQuotaGroup),
    "gs_quota_status": C.sizeof(GsQuotaStatus), "gs_node_devices": C.sizeof(GsNodeDevices),
    "gs_reservation": C.sizeof(GsReservation), "gs_pod_ext": C.sizeof(GsPodExt), "gs_ext_args": C.sizeof(GsExtArgs),
    "gs_ext_placement": C.sizeof(GsExtPlacement), "gs_status_map": C.sizeof(GsStatusMap),
    "gs_resident_pod": C.sizeof(GsResidentPod), "gs_preemptor": C.sizeof(GsPreemptor),
    "gs_preempt_result": C.sizeof(GsPreemptResult), "gs_preempt_detail": C.sizeof(GsPreemptDetail),
    "gs_preempt_candidate": C.sizeof(GsPreemptCandidate),
    "gs_preempt_result_pdb": C.sizeof(GsPreemptResultPdb), "gs_preempt_detail_pdb": C.sizeof(GsPreemptDetailPdb),
    "gs_preempt_candidate_pdb": C.sizeof(GsPreemptCandidatePdb),
    "gs_top_score": C.sizeof(GsTopScore), "gs_top_scores": C.sizeof(GsTopScores),
}
# gs_abi_sizes goes on after STRUCT_SIZES with the RDMA / FPGA structs (a table of their own: STRUCT_SIZES keeps its
# length and last entries)
AUX_STRUCT_SIZES = {
    "gs_aux_device": C.sizeof(GsAuxDevice), "gs_node_aux_devices": C.sizeof(GsNodeAuxDevices),
    "gs_pod_aux": C.sizeof(GsPodAux), "gs_aux_placement": C.sizeof(GsAuxPlacement),
}

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(PKG_DIR, "libgpuscore.so")

# every symbol include/gpuscore.h declares: name -> (restype, argtypes)
P = C.c_void_p
SIGNATURES = {
    "gs_loadaware_args_default": (None, [C.POINTER(GsLoadAwareArgs)]),
    "gs_fit_args_default": (None, [C.POINTER(GsFitArgs)]),
    "gs_loadaware_args_validate": (C.c_int, [C.POINTER(GsLoadAwareArgs), C.c_char_p, C.c_size_t]),
    "gs_create": (C.c_int, [C.POINTER(GsConfig), C.POINTER(P)]),
    "gs_destroy": (C.c_int, [P]),
    "gs_last_error": (C.c_char_p, [P]),
    "gs_version": (C.c_char_p, []),
    "gs_set_now": (C.c_int, [P, i64]),
    "gs_nodes_upsert": (C.c_int, [P, P, P, u32]),
    "gs_node_metrics_upsert": (C.c_int, [P, P, P, u32, P, P]),
    "gs_pods_assign": (C.c_int, [P, P, P, P, u32]),
    "gs_pods_unassign": (C.c_int, [P, P, P, u32]),
    "gs_pods_forget": (C.c_int, [P, P, P, u32]),
    "gs_evaluate": (C.c_int, [P, P, u32, P, P, P]),
    "gs_schedule": (C.c_int, [P, P, u32, P, P]),
    "gs_schedule_submit": (C.c_int, [P, P, u32, P, P, C.POINTER(u64)]),
    "gs_schedule_wait": (C.c_int, [P, u64]),
    "gs_schedule_diag": (C.c_int, [P, P, u32, P, P, P]),
    "gs_schedule_submit_diag": (C.c_int, [P, P, u32, P, P, P, C.POINTER(u64)]),
    "gs_fit_error_string": (C.c_int, [P, P, C.c_char_p, C.c_size_t]),
    "gs_schedule_diag_nodes": (C.c_int, [P, P, u32, P, P, P, C.POINTER(GsStatusMap)]),
    "gs_schedule_submit_diag_nodes": (C.c_int, [P, P, u32, P, P, P, C.POINTER(GsStatusMap), C.POINTER(u64)]),
    "gs_schedule_top_scores": (C.c_int, [P, P, u32, P, P, C.POINTER(GsTopScores)]),
    "gs_schedule_submit_top_scores": (C.c_int, [P, P, u32, P, P, C.POINTER(GsTopScores), C.POINTER(u64)]),
    "gs_debug_scores_string": (C.c_int, [C.c_int, C.c_char_p, P, u32, P, u32, P, C.c_char_p, C.c_size_t]),
    "gs_status_framework_code": (C.c_int, [C.c_uint16]),
    "gs_preemption_candidates": (C.c_int, [P, u32, P, u32]),
    "gs_comm_unique_id": (C.c_int, [P]),
    "gs_comm_init_rccl": (C.c_int, [P, P, C.c_int, C.c_int]),
    "gs_comm_init_callback": (C.c_int, [P, C.c_int, C.c_int, ALLGATHER_FN, P]),
    "gs_local_group_create": (C.c_int, [C.c_int, C.POINTER(P)]),
    "gs_local_group_destroy": (C.c_int, [P]),
    "gs_comm_init_local": (C.c_int, [P, P, C.c_int]),
    "gs_get_stats": (C.c_int, [P, C.POINTER(GsStats)]),
    "gs_reset_stats": (C.c_int, [P]),
    "gs_synchronize": (C.c_int, [P]),
    "gs_debug_mirror_check": (C.c_int, [P]),
    "gs_debug_verify_cpuset": (C.c_int, [P, C.c_int]),
    "gs_debug_commit_counters": (C.c_int, [P, P]),
    "gs_debug_pair_probe": (C.c_int, [P, P, C.c_uint32, P, P, C.c_uint32, C.c_int, P, P]),
    "gs_debug_numa_merge": (C.c_int, [P, P, u32, P]),
    "gs_debug_ext_rows": (C.c_int, [P, P, P, u64, P, P, P]),
    "gs_gang_args_default": (None, [C.POINTER(GsGangArgs)]),
    "gs_gang_mgr_create": (C.c_int, [C.POINTER(GsGangArgs), C.POINTER(P)]),
    "gs_gang_mgr_destroy": (C.c_int, [P]),
    "gs_gang_mgr_clone": (C.c_int, [P, C.POINTER(P)]),
    "gs_gang_mgr_assign": (C.c_int, [P, P]),
    "gs_gang_podgroup_upsert": (C.c_int, [P, C.POINTER(GsGangSpec)]),
    "gs_gang_podgroup_delete": (C.c_int, [P, u64]),
    "gs_gang_pod_add": (C.c_int, [P, u64, u64, C.c_int, C.POINTER(GsGangSpec)]),
    "gs_gang_pod_delete": (C.c_int, [P, u64, u64]),
    "gs_gang_prefilter": (C.c_int, [P, u64, u64, C.c_int]),
    "gs_gang_permit": (C.c_int, [P, u64, u64, i64, C.POINTER(i64), P, u32, C.POINTER(u32)]),
    "gs_gang_post_bind": (C.c_int, [P, u64, u64]),
    "gs_gang_post_filter": (C.c_int, [P, u64, u64, P, u32, C.POINTER(u32)]),
    "gs_gang_unreserve": (C.c_int, [P, u64, u64, P, u32, C.POINTER(u32)]),
    "gs_gang_expire": (C.c_int, [P, i64, P, u32, C.POINTER(u32)]),
    "gs_gang_get": (C.c_int, [P, u64, C.POINTER(GsGangInfo)]),
    "gs_gang_child_cycle": (C.c_int, [P, u64, u64]),
    "gs_gang_waiting_pods": (C.c_int, [P, P, u32, C.POINTER(u32)]),
    "gs_gang_debug_set": (C.c_int, [P, u64, u64, C.c_int, C.c_int]),
    "gs_gang_pass_create": (C.c_int, [P, u32, P, P, P, i64, P, P, P, P, C.POINTER(P)]),
    "gs_gang_pass_destroy": (C.c_int, [P]),
    "gs_gang_walk": (C.c_int, [P, u32, u32, P, C.POINTER(u32), C.POINTER(u32)]),
    "gs_gang_replay": (C.c_int, [P, u32, u32, P, u32, P, C.POINTER(u32), C.POINTER(u32), C.POINTER(i32)]),
    "gs_gang_pass_after_single": (C.c_int, [P, u32, i32]),
    "gs_gang_pass_forgets": (C.c_int, [P, P, u32, C.POINTER(u32)]),
    "gs_gang_pass_carried": (C.c_int, [P, P, P, u32, C.POINTER(u32)]),
    "gs_reason_string": (C.c_int, [C.c_uint32, C.c_uint32, P, C.c_char_p, C.c_size_t]),
    "gs_reset": (C.c_int, [P]),
    "gs_abi_sizes": (None, [C.POINTER(u64), u32]),
    "gs_topology_register": (C.c_int, [P, C.POINTER(GsCpuTopology), C.POINTER(i32)]),
    "gs_nodes_numa_upsert": (C.c_int, [P, P, P, u32]),
    "gs_numa_allocations_update": (C.c_int, [P, P, P, u32]),
    "gs_numa_allocations_release": (C.c_int, [P, P, P, u32]),
    "gs_numa_allocation_get": (C.c_int, [P, u32, u64, C.POINTER(GsPodAllocation)]),
    "gs_numa_args_default": (None, [C.POINTER(GsNumaArgs)]),
    "gs_num_feasible_nodes_to_find": (u32, [u32, i32]),
    "gs_decode_quantity": (C.c_int, [C.c_char_p, C.POINTER(i64), C.POINTER(i64)]),
    "gs_decode_cpuset": (C.c_int, [C.c_char_p, C.POINTER(u64)]),
    "gs_decode_node_annotations": (C.c_int, [C.POINTER(GsKv), u32, C.POINTER(GsNode), C.POINTER(GsNodeNuma)]),
    "gs_node_reservation_trim": (C.c_int, [C.POINTER(GsKv), u32, C.POINTER(GsNode)]),
    "gs_node_reserved_cpus": (C.c_int, [C.POINTER(GsKv), u32, C.POINTER(u64), C.POINTER(C.c_int32)]),
    "gs_decode_nrt_reserved_cpus": (C.c_int, [C.POINTER(GsKv), u32, C.POINTER(u64)]),
    "gs_decode_node_labels": (C.c_int, [C.POINTER(GsKv), u32, C.c_char_p, C.c_char_p, C.POINTER(GsNodeNuma)]),
    "gs_decode_resource_spec": (C.c_int, [C.c_char_p, C.POINTER(GsPod)]),
    "gs_decode_cpu_topology": (C.c_int, [C.c_char_p, C.POINTER(GsCpuTopology)]),
    "gs_quota_redistribute": (C.c_int, [P, P, P, P, P, u32, i64, P]),
    "gs_quota_refresh_runtime": (C.c_int, [P, u32, P, P, P, P]),
    "gs_quota_prefilter": (C.c_int, [P, u32, P, P, i32, P, u32, u32, C.POINTER(GsQuotaStatus)]),
    "gs_quota_reserve": (C.c_int, [P, u32, i32, P, u32, i32]),
    "gs_quota_admit_batch": (C.c_int, [P, u32, P, P, P, P, P, P, u32, P, C.POINTER(u32)]),
    "gs_quota_settle_batch": (C.c_int, [P, u32, P, P, P, P, P, P, u32, P, P]),
    "gs_pods_on_event": (C.c_int, [P, C.c_int, P, P, u32]),
    "gs_assign_cache_get": (C.c_int, [P, u32, P, P, u32]),
    "gs_ext_args_default": (None, [C.POINTER(GsExtArgs)]),
    "gs_ext_configure": (C.c_int, [P, C.POINTER(GsExtArgs)]),
    "gs_node_devices_upsert": (C.c_int, [P, P, P, u32]),
    "gs_node_devices_get": (C.c_int, [P, u32, C.POINTER(GsNodeDevices)]),
    "gs_reservations_upsert": (C.c_int, [P, P, u32]),
    "gs_reservations_remove": (C.c_int, [P, P, u32]),
    "gs_reservation_get": (C.c_int, [P, u64, C.POINTER(GsReservation)]),
    "gs_schedule_ext": (C.c_int, [P, P, P, u32, P, P, P]),
    "gs_ext_reserved_get": (C.c_int, [P, u64, P, P]),
    "gs_ext_configure_aux": (C.c_int, [P, P]),
    "gs_node_aux_devices_upsert": (C.c_int, [P, P, P, u32]),
    "gs_node_aux_devices_get": (C.c_int, [P, u32, P]),
    "gs_schedule_ext_aux": (C.c_int, [P, P, P, P, u32, P, P, P, P]),
    "gs_ext_aux_reserved_get": (C.c_int, [P, u64, P, P]),
    "gs_debug_ext_rows_aux": (C.c_int, [P, P, P, P, u64, P, P, P]),
    "gs_node_pods_add": (C.c_int, [P, P, P, u32]),
    "gs_node_pods_remove": (C.c_int, [P, P, P, u32]),
    "gs_node_pods_get": (C.c_int, [P, u32, P, u32]),
    "gs_preempt_dry_run": (C.c_int, [P, P, u32, P, u32, P, C.POINTER(GsPreemptDetail)]),
    "gs_preempt_pick_node": (C.c_int, [P, u32]),
    "gs_pdbs_upsert": (C.c_int, [P, P, P, u32]),
    "gs_node_pods_set_pdbs": (C.c_int, [P, P, P, P, u32]),
    "gs_node_pods_get_pdbs": (C.c_int, [P, u32, P, u32]),
    "gs_preempt_dry_run_pdb": (C.c_int, [P, P, u32, P, u32, P, C.POINTER(GsPreemptDetailPdb)]),
    "gs_preempt_pick_node_pdb": (C.c_int, [P, u32]),
}


def header_symbols(header_path: str | None = None) -> list[str]:
    """Function names declared in include/gpuscore.h (parsed, not hard-coded)."""
    import re
    if header_path is None:
        header_path = os.path.join(os.path.dirname(PKG_DIR), "include", "gpuscore.h")
    text = open(header_path).read()
    return sorted(set(re.findall(r"^\s*(?:[A-Za-z_][\w\s\*]*?)\b(gs_\w+)\s*\(", text, re.M)))


_LOADED: dict = {}


def load(path: str = LIB_PATH) -> C.CDLL:
    """Load libgpuscore and declare signatures (once per path). Raises if the HIP extension is missing."""
    lib = _LOADED.get(path)
    if lib is not None:
        return lib
    if not os.path.exists(path):
        raise RuntimeError(f"libgpuscore not built: {path} missing (run __graft_entry__.build())")
    lib = C.CDLL(path)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _LOADED[path] = lib
    return lib


def ptr(a) -> int | None:
    """Address of a numpy array's data (None for None)."""
    if a is None:
        return None
    return a.ctypes.data
