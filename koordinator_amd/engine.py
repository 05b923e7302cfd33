"""Python host mirror of the plugin interface over libgpuscore's C-ABI.

`Engine` is one scheduler profile (NodeResourcesFit + LoadAwareScheduling) on one GPU. Its methods map
1:1 onto the C-ABI, which in turn replaces the reference plugin entry points:

  Engine(cfg)            loadaware.New / noderesources.NewFit        (load_aware.go:76-110)
  set_now                time.Now injection                           (helper.go:36-41, pod_assign_cache.go:30)
  upsert_nodes           scheduler cache snapshot (NodeInfo)          ([upstream] Cache.UpdateSnapshot)
  upsert_metrics         NodeMetric informer                          (load_aware.go:95,133,278)
  assign / unassign      podAssignCache.assign / unAssign             (pod_assign_cache.go:53-80)
  evaluate               RunFilterPlugins + RunScorePlugins per node  (load_aware.go:123-171,269-335)
  schedule               scheduleOne loop incl. selectHost + Reserve  ([upstream] schedule_one.go)
  schedule_diag          ... with the FitError diagnosis of each pod   ([upstream] framework/types.go FitError)
  schedule_top_scores    ... with each scored pod's --debug-scores table (frameworkext/debug.go:61-109)

The product path has no CPU fallback: if libgpuscore or a GPU is missing, construction fails.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import abi

_lib = None


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        _lib = abi.load()
    return _lib


class GpuScoreError(RuntimeError):
    pass


class LocalGroup:
    """The in-process device transport's group (gs_local_group): the ranks are threads of this process, each with its
    own Engine; the per-batch all-gathers (score rows, or candidate levels under GS_XCHG=levels) run stream-ordered on
    the device as ncclAllGather does."""

    def __init__(self, nranks: int):
        self._h = C.c_void_p()
        rc = lib().gs_local_group_create(nranks, C.byref(self._h))
        if rc != 0:
            raise GpuScoreError(f"gs_local_group_create: {rc}")

    def __del__(self):
        if getattr(self, "_h", None):
            lib().gs_local_group_destroy(self._h)
            self._h = None


class Engine:
    def __init__(self, cfg: abi.GsConfig):
        self.cfg = cfg
        self.n = cfg.num_nodes
        h = C.c_void_p()
        rc = lib().gs_create(C.byref(cfg), C.byref(h))
        if rc != 0:
            raise GpuScoreError(f"gs_create failed: {rc}")
        self._h = h
        self._cb = None

    def close(self):
        if getattr(self, "_h", None):
            lib().gs_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc: int, what: str):
        if rc != 0:
            msg = lib().gs_last_error(self._h)
            raise GpuScoreError(f"{what}: rc={rc}: {msg.decode() if msg else ''}")

    def set_now(self, now_ns: int):
        self._chk(lib().gs_set_now(self._h, int(now_ns)), "gs_set_now")

    def upsert_nodes(self, nodes, idx=None):
        nodes = np.ascontiguousarray(nodes, dtype=abi.NODE_DTYPE)
        if idx is not None:
            idx = np.ascontiguousarray(idx, dtype=np.uint32)
        self._chk(lib().gs_nodes_upsert(self._h, abi.ptr(idx), abi.ptr(nodes), len(nodes)), "gs_nodes_upsert")

    def upsert_metrics(self, metrics, pod_metrics=None, offsets=None, idx=None):
        metrics = np.ascontiguousarray(metrics, dtype=abi.METRIC_DTYPE)
        if idx is not None:
            idx = np.ascontiguousarray(idx, dtype=np.uint32)
        if pod_metrics is not None:
            pod_metrics = np.ascontiguousarray(pod_metrics, dtype=abi.POD_METRIC_DTYPE)
            offsets = np.ascontiguousarray(offsets, dtype=np.uint32)
        self._chk(lib().gs_node_metrics_upsert(self._h, abi.ptr(idx), abi.ptr(metrics), len(metrics),
                                               abi.ptr(pod_metrics), abi.ptr(offsets)), "gs_node_metrics_upsert")

    def assign(self, node_idx, pods, ts):
        node_idx = np.ascontiguousarray(node_idx, dtype=np.uint32)
        pods = np.ascontiguousarray(pods, dtype=abi.POD_DTYPE)
        ts = np.ascontiguousarray(ts, dtype=np.int64)
        self._chk(lib().gs_pods_assign(self._h, abi.ptr(node_idx), abi.ptr(pods), abi.ptr(ts), len(pods)),
                  "gs_pods_assign")

    def unassign(self, node_idx, pods):
        node_idx = np.ascontiguousarray(node_idx, dtype=np.uint32)
        pods = np.ascontiguousarray(pods, dtype=abi.POD_DTYPE)
        self._chk(lib().gs_pods_unassign(self._h, abi.ptr(node_idx), abi.ptr(pods), len(pods)), "gs_pods_unassign")

    def forget(self, node_idx, pods):
        """gs_pods_forget: ForgetPod of assumed pods after Unreserve (NodeInfo, podAssignCache, NUMA allocation), with
        the DeviceShare / Reservation Unreserve of a pod schedule_ext placed (ext_reserved)."""
        node_idx = np.ascontiguousarray(node_idx, dtype=np.uint32)
        pods = np.ascontiguousarray(pods, dtype=abi.POD_DTYPE)
        self._chk(lib().gs_pods_forget(self._h, abi.ptr(node_idx), abi.ptr(pods), len(pods)), "gs_pods_forget")

    def evaluate(self, pods):
        pods = np.ascontiguousarray(pods, dtype=abi.POD_DTYPE)
        P, N = len(pods), self.n
        scores = np.empty((P, N), np.int16)
        codes = np.empty((P, N), np.uint16)
        plugin = np.empty((P, N, abi.GS_NUM_PLUGINS), np.int16)
        self._chk(lib().gs_evaluate(self._h, abi.ptr(pods), P, abi.ptr(scores), abi.ptr(codes), abi.ptr(plugin)),
                  "gs_evaluate")
        return scores, codes, plugin

    def schedule(self, pods, seq=None):
        pods = np.ascontiguousarray(pods, dtype=abi.POD_DTYPE)
        if seq is None:
            seq = np.arange(len(pods), dtype=np.uint64)
        seq = np.ascontiguousarray(seq, dtype=np.uint64)
        out = np.zeros(len(pods), abi.PLACEMENT_DTYPE)
        self._chk(lib().gs_schedule(self._h, abi.ptr(pods), len(pods), abi.ptr(seq), abi.ptr(out)), "gs_schedule")
        return out

    def schedule_submit(self, pods, seq=None):
        """gs_schedule_submit: returns a handle for schedule_wait (the placements array, filled once it completes)."""
        pods = np.ascontiguousarray(pods, dtype=abi.POD_DTYPE)
        if seq is None:
            seq = np.arange(len(pods), dtype=np.uint64)
        seq = np.ascontiguousarray(seq, dtype=np.uint64)
        out = np.zeros(len(pods), abi.PLACEMENT_DTYPE)
        t = C.c_uint64(0)
        self._chk(lib().gs_schedule_submit(self._h, abi.ptr(pods), len(pods), abi.ptr(seq), abi.ptr(out), C.byref(t)),
                  "gs_schedule_submit")
        return (t.value, out)

    def schedule_wait(self, handle):
        """The placements of a schedule_submit handle; (placements, diag) of a schedule_submit_diag handle;
        (placements, diag, words, row_of) of a schedule_submit_diag_nodes handle; (placements, rows, count) of a
        schedule_submit_top_scores handle."""
        t, *res = handle
        self._chk(lib().gs_schedule_wait(self._h, t), "gs_schedule_wait")
        if res and isinstance(res[-1], abi.GsTopScores):   # (the handle kept the struct alive)
            res.pop()
        if res and isinstance(res[-1], abi.GsStatusMap):   # words: the rows handed out
            m = res.pop()
            res[2] = res[2][:m.rows_used]
        return res[0] if len(res) == 1 else tuple(res)

    def _status_map(self, pods, cap_rows):
        """The caller-owned buffers of a gs_status_map; cap_rows None: a row for every pod."""
        cap = len(pods) if cap_rows is None else int(cap_rows)
        words = np.zeros((cap, self.cfg.num_nodes), np.uint16)
        row_of = np.full(len(pods), -1, np.int32)
        m = abi.GsStatusMap(words=abi.ptr(words) if cap else None, cap_rows=cap, row_of=abi.ptr(row_of))
        return words, row_of, m

    def schedule_diag_nodes(self, pods, seq=None, cap_rows=None):
        """gs_schedule_diag_nodes: (placements, diag, words, row_of). words[row_of[i]] (uint16[num_nodes]) is the
        Filter status of every node at the turn of pod i, a pod with node -1 (abi.status_code / status_scalar_mask /
        status_framework_code / preemption_candidates read it); row_of[i] is -1 for a placed pod and for a FitError
        pod beyond the first cap_rows of them (None: a row for every pod). words holds the rows handed out."""
        pods = np.ascontiguousarray(pods, dtype=abi.POD_DTYPE)
        if seq is None:
            seq = np.arange(len(pods), dtype=np.uint64)
        seq = np.ascontiguousarray(seq, dtype=np.uint64)
        out = np.zeros(len(pods), abi.PLACEMENT_DTYPE)
        diag = np.zeros(len(pods), abi.FIT_DIAGNOSIS_DTYPE)
        words, row_of, m = self._status_map(pods, cap_rows)
        self._chk(lib().gs_schedule_diag_nodes(self._h, abi.ptr(pods), len(pods), abi.ptr(seq), abi.ptr(out),
                                               abi.ptr(diag), C.byref(m)), "gs_schedule_diag_nodes")
        return out, diag, words[:m.rows_used], row_of

    def schedule_submit_diag_nodes(self, pods, seq=None, cap_rows=None):
        """gs_schedule_submit_diag_nodes: a handle for schedule_wait, which then returns what schedule_diag_nodes does."""
        pods = np.ascontiguousarray(pods, dtype=abi.POD_DTYPE)
        if seq is None:
            seq = np.arange(len(pods), dtype=np.uint64)
        seq = np.ascontiguousarray(seq, dtype=np.uint64)
        out = np.zeros(len(pods), abi.PLACEMENT_DTYPE)
        diag = np.zeros(len(pods), abi.FIT_DIAGNOSIS_DTYPE)
        words, row_of, m = self._status_map(pods, cap_rows)
        t = C.c_uint64(0)
        self._chk(lib().gs_schedule_submit_diag_nodes(self._h, abi.ptr(pods), len(pods), abi.ptr(seq), abi.ptr(out),
                                                      abi.ptr(diag), C.byref(m), C.byref(t)),
                  "gs_schedule_submit_diag_nodes")
        return (t.value, out, diag, words, row_of, m)

    def _top_scores(self, pods, topn):
        """The caller-owned buffers of a gs_top_scores."""
        rows = np.zeros((len(pods), max(1, min(int(topn), abi.GS_MAX_TOP_SCORES))), abi.TOP_SCORE_DTYPE)
        count = np.zeros(len(pods), np.uint32)
        return rows, count, abi.GsTopScores(rows=abi.ptr(rows), count=abi.ptr(count), topn=int(topn))

    def schedule_top_scores(self, pods, seq=None, topn=8):
        """gs_schedule_top_scores: (placements, rows, count). rows[i, :count[i]] (abi.TOP_SCORE_DTYPE) is the
        --debug-scores table of pod i at its turn: its topn best feasible nodes by (total descending, node ascending)
        with the unweighted plugin scores; count[i] is 0 for a pod with fewer than two feasible nodes.
        abi.debug_scores_table renders one. One rank, no node sampling."""
        pods = np.ascontiguousarray(pods, dtype=abi.POD_DTYPE)
        if seq is None:
            seq = np.arange(len(pods), dtype=np.uint64)
        seq = np.ascontiguousarray(seq, dtype=np.uint64)
        out = np.zeros(len(pods), abi.PLACEMENT_DTYPE)
        rows, count, t = self._top_scores(pods, topn)
        self._chk(lib().gs_schedule_top_scores(self._h, abi.ptr(pods), len(pods), abi.ptr(seq), abi.ptr(out),
                                               C.byref(t)), "gs_schedule_top_scores")
        return out, rows, count

    def schedule_submit_top_scores(self, pods, seq=None, topn=8):
        """gs_schedule_submit_top_scores: a handle for schedule_wait, which then returns what schedule_top_scores does."""
        pods = np.ascontiguousarray(pods, dtype=abi.POD_DTYPE)
        if seq is None:
            seq = np.arange(len(pods), dtype=np.uint64)
        seq = np.ascontiguousarray(seq, dtype=np.uint64)
        out = np.zeros(len(pods), abi.PLACEMENT_DTYPE)
        rows, count, ts = self._top_scores(pods, topn)
        t = C.c_uint64(0)
        self._chk(lib().gs_schedule_submit_top_scores(self._h, abi.ptr(pods), len(pods), abi.ptr(seq), abi.ptr(out),
                                                      C.byref(ts), C.byref(t)), "gs_schedule_submit_top_scores")
        return (t.value, out, rows, count, ts)

    def schedule_diag(self, pods, seq=None):
        """gs_schedule_diag: (placements, diag); diag[i] (abi.FIT_DIAGNOSIS_DTYPE) is the FitError diagnosis of a pod
        with node -1 (valid = 1), zero otherwise. One rank, no node sampling."""
        pods = np.ascontiguousarray(pods, dtype=abi.POD_DTYPE)
        if seq is None:
            seq = np.arange(len(pods), dtype=np.uint64)
        seq = np.ascontiguousarray(seq, dtype=np.uint64)
        out = np.zeros(len(pods), abi.PLACEMENT_DTYPE)
        diag = np.zeros(len(pods), abi.FIT_DIAGNOSIS_DTYPE)
        self._chk(lib().gs_schedule_diag(self._h, abi.ptr(pods), len(pods), abi.ptr(seq), abi.ptr(out), abi.ptr(diag)),
                  "gs_schedule_diag")
        return out, diag

    def schedule_submit_diag(self, pods, seq=None):
        """gs_schedule_submit_diag: a handle for schedule_wait, which then returns (placements, diag)."""
        pods = np.ascontiguousarray(pods, dtype=abi.POD_DTYPE)
        if seq is None:
            seq = np.arange(len(pods), dtype=np.uint64)
        seq = np.ascontiguousarray(seq, dtype=np.uint64)
        out = np.zeros(len(pods), abi.PLACEMENT_DTYPE)
        diag = np.zeros(len(pods), abi.FIT_DIAGNOSIS_DTYPE)
        t = C.c_uint64(0)
        self._chk(lib().gs_schedule_submit_diag(self._h, abi.ptr(pods), len(pods), abi.ptr(seq), abi.ptr(out),
                                                abi.ptr(diag), C.byref(t)), "gs_schedule_submit_diag")
        return (t.value, out, diag)

    def pod_event(self, event: int, node_idx, pods):
        """podAssignCache OnAdd / OnUpdate / OnDelete (node_idx -1 = pod.Spec.NodeName == "")."""
        pods = np.ascontiguousarray(pods, dtype=abi.POD_DTYPE)
        idx = np.ascontiguousarray(node_idx, dtype=np.int32)
        self._chk(lib().gs_pods_on_event(self._h, event, abi.ptr(idx), abi.ptr(pods), len(pods)), "gs_pods_on_event")

    def assign_cache(self, node: int) -> list[tuple[int, int]]:
        u = np.zeros(256, np.uint64)
        t = np.zeros(256, np.int64)
        n = lib().gs_assign_cache_get(self._h, node, abi.ptr(u), abi.ptr(t), 256)
        self._chk(min(n, 0), "gs_assign_cache_get")
        return list(zip(u[:n].tolist(), t[:n].tolist()))

    # ---- ElasticQuota PostFilter: the resident-pod table and the preemption dry run
    def node_pods_add(self, node_idx, pods):
        """gs_node_pods_add: RESIDENT_POD_DTYPE records join the resident-pod table of their nodes."""
        node_idx = np.ascontiguousarray(node_idx, dtype=np.uint32)
        pods = np.ascontiguousarray(pods, dtype=abi.RESIDENT_POD_DTYPE)
        assert len(node_idx) == len(pods)
        self._chk(lib().gs_node_pods_add(self._h, abi.ptr(node_idx), abi.ptr(pods), len(pods)), "gs_node_pods_add")

    def node_pods_remove(self, node_idx, uids):
        node_idx = np.ascontiguousarray(node_idx, dtype=np.uint32)
        uids = np.ascontiguousarray(uids, dtype=np.uint64)
        assert len(node_idx) == len(uids)
        self._chk(lib().gs_node_pods_remove(self._h, abi.ptr(node_idx), abi.ptr(uids), len(uids)),
                  "gs_node_pods_remove")

    def node_pods(self, node: int):
        """gs_node_pods_get: the node's resident pods in MoreImportantPod order (the order of the victim bits)."""
        out = np.zeros(abi.GS_MAX_NODE_PODS, abi.RESIDENT_POD_DTYPE)
        n = lib().gs_node_pods_get(self._h, int(node), abi.ptr(out), len(out))
        self._chk(min(n, 0), "gs_node_pods_get")
        return out[:n]

    def preempt_dry_run(self, preemptors, rows=None, detail: bool = True):
        """gs_preempt_dry_run: (results, node_status, victim_bits) for PREEMPTOR_DTYPE records; rows: the status
        words [num_rows][num_nodes] their `row` fields index (gs_schedule_diag_nodes' words). node_status is
        uint8[n][num_nodes], victim_bits uint64[n][num_nodes][2] (both None without detail)."""
        pre = np.ascontiguousarray(preemptors, dtype=abi.PREEMPTOR_DTYPE)
        n, N = len(pre), self.cfg.num_nodes
        if rows is not None:
            rows = np.ascontiguousarray(rows, dtype=np.uint16).reshape(-1, N)
        out = np.zeros(n, abi.PREEMPT_RESULT_DTYPE)
        status = bits = None
        d = None
        if detail:
            status = np.zeros((n, N), np.uint8)
            bits = np.zeros((n, N, 2), np.uint64)
            d = C.byref(abi.GsPreemptDetail(node_status=abi.ptr(status), victim_bits=abi.ptr(bits)))
        self._chk(lib().gs_preempt_dry_run(self._h, abi.ptr(pre), n, abi.ptr(rows), 0 if rows is None else len(rows),
                                           abi.ptr(out), d), "gs_preempt_dry_run")
        return out, status, bits

    # ---- PodDisruptionBudgets in the dry run
    def pdbs_upsert(self, ids, disruptions_allowed):
        """gs_pdbs_upsert: the budget (DisruptionsAllowed) of each PDB id; abi.GS_PDB_UNLIMITED deletes a PDB."""
        ids = np.ascontiguousarray(ids, dtype=np.uint32)
        allowed = np.ascontiguousarray(disruptions_allowed, dtype=np.int32)
        assert len(ids) == len(allowed)
        self._chk(lib().gs_pdbs_upsert(self._h, abi.ptr(ids), abi.ptr(allowed), len(ids)), "gs_pdbs_upsert")

    def node_pods_set_pdbs(self, node_idx, uids, pdb_ids):
        """gs_node_pods_set_pdbs: pdb_ids uint16[n][4] (abi.GS_PDB_NONE = no entry) replaces the PDB list of resident
        pod uids[i] on node node_idx[i]."""
        node_idx = np.ascontiguousarray(node_idx, dtype=np.uint32)
        uids = np.ascontiguousarray(uids, dtype=np.uint64)
        pdb_ids = np.ascontiguousarray(pdb_ids, dtype=np.uint16).reshape(-1, abi.GS_MAX_POD_PDBS)
        assert len(node_idx) == len(uids) == len(pdb_ids)
        self._chk(lib().gs_node_pods_set_pdbs(self._h, abi.ptr(node_idx), abi.ptr(uids), abi.ptr(pdb_ids), len(uids)),
                  "gs_node_pods_set_pdbs")

    def node_pods_pdbs(self, node: int):
        """gs_node_pods_get_pdbs: uint16[count][4], the PDB lists of the node's pods in the order of node_pods."""
        out = np.full((abi.GS_MAX_NODE_PODS, abi.GS_MAX_POD_PDBS), abi.GS_PDB_NONE, np.uint16)
        n = lib().gs_node_pods_get_pdbs(self._h, int(node), abi.ptr(out), len(out))
        self._chk(min(n, 0), "gs_node_pods_get_pdbs")
        return out[:n]

    def preempt_dry_run_pdb(self, preemptors, rows=None, detail: bool = True):
        """gs_preempt_dry_run_pdb: (results, node_status, victim_bits, violating_bits, pdb_violations) for
        PREEMPTOR_DTYPE records, as preempt_dry_run; violating_bits is uint64[n][num_nodes][2], pdb_violations
        uint8[n][num_nodes] (the four arrays are None without detail)."""
        pre = np.ascontiguousarray(preemptors, dtype=abi.PREEMPTOR_DTYPE)
        n, N = len(pre), self.cfg.num_nodes
        if rows is not None:
            rows = np.ascontiguousarray(rows, dtype=np.uint16).reshape(-1, N)
        out = np.zeros(n, abi.PREEMPT_RESULT_PDB_DTYPE)
        status = bits = viol = nviol = None
        d = None
        if detail:
            status = np.zeros((n, N), np.uint8)
            bits = np.zeros((n, N, 2), np.uint64)
            viol = np.zeros((n, N, 2), np.uint64)
            nviol = np.zeros((n, N), np.uint8)
            d = C.byref(abi.GsPreemptDetailPdb(node_status=abi.ptr(status), victim_bits=abi.ptr(bits),
                                               violating_bits=abi.ptr(viol), pdb_violations=abi.ptr(nviol)))
        self._chk(lib().gs_preempt_dry_run_pdb(self._h, abi.ptr(pre), n, abi.ptr(rows),
                                               0 if rows is None else len(rows), abi.ptr(out), d),
                  "gs_preempt_dry_run_pdb")
        return out, status, bits, viol, nviol

    # ---- Reservation + DeviceShare
    def ext_configure(self, args: abi.GsExtArgs):
        self._chk(lib().gs_ext_configure(self._h, C.byref(args)), "gs_ext_configure")

    def upsert_devices(self, devs, idx=None):
        devs = np.ascontiguousarray(devs, dtype=abi.NODE_DEVICES_DTYPE)
        if idx is not None:
            idx = np.ascontiguousarray(idx, dtype=np.uint32)
        self._chk(lib().gs_node_devices_upsert(self._h, abi.ptr(idx), abi.ptr(devs), len(devs)), "gs_node_devices_upsert")

    def devices(self, node: int):
        out = abi.GsNodeDevices()
        self._chk(lib().gs_node_devices_get(self._h, node, C.byref(out)), "gs_node_devices_get")
        return np.frombuffer(bytes(out), dtype=abi.NODE_DEVICES_DTYPE)[0]

    def upsert_reservations(self, rsv):
        rsv = np.ascontiguousarray(rsv, dtype=abi.RESERVATION_DTYPE)
        self._chk(lib().gs_reservations_upsert(self._h, abi.ptr(rsv), len(rsv)), "gs_reservations_upsert")

    def remove_reservations(self, uids):
        uids = np.ascontiguousarray(uids, dtype=np.uint64)
        self._chk(lib().gs_reservations_remove(self._h, abi.ptr(uids), len(uids)), "gs_reservations_remove")

    def reservation(self, uid: int):
        out = abi.GsReservation()
        rc = lib().gs_reservation_get(self._h, uid, C.byref(out))
        self._chk(min(rc, 0), "gs_reservation_get")
        return np.frombuffer(bytes(out), dtype=abi.RESERVATION_DTYPE)[0] if rc == 1 else None

    def schedule_ext(self, pods, ext, seq=None):
        pods = np.ascontiguousarray(pods, dtype=abi.POD_DTYPE)
        ext = np.ascontiguousarray(ext, dtype=abi.POD_EXT_DTYPE)
        assert len(ext) == len(pods)
        if seq is None:
            seq = np.arange(len(pods), dtype=np.uint64)
        seq = np.ascontiguousarray(seq, dtype=np.uint64)
        out = np.zeros(len(pods), abi.PLACEMENT_DTYPE)
        eo = np.zeros(len(pods), abi.EXT_PLACEMENT_DTYPE)
        self._chk(lib().gs_schedule_ext(self._h, abi.ptr(pods), abi.ptr(ext), len(pods), abi.ptr(seq), abi.ptr(out),
                                        abi.ptr(eo)), "gs_schedule_ext")
        return out, eo

    def ext_reserved(self, uid: int):
        """gs_ext_reserved_get: (node, EXT_PLACEMENT_DTYPE record) of the extension-path Reserve recorded for an
        assumed pod, None when there is none (never placed by schedule_ext, or forgotten / unassigned since)."""
        node = C.c_uint32(0)
        out = np.zeros(1, abi.EXT_PLACEMENT_DTYPE)
        rc = lib().gs_ext_reserved_get(self._h, int(uid), C.byref(node), abi.ptr(out))
        self._chk(min(rc, 0), "gs_ext_reserved_get")
        return (int(node.value), out[0]) if rc == 1 else None

    # ---- DeviceShare device types beyond GPU: RDMA and FPGA
    def ext_configure_aux(self, weights):
        """ScoringStrategy.Resources weights of koordinator.sh/rdma and koordinator.sh/fpga (default 0, 0)"""
        w = np.ascontiguousarray(weights, dtype=np.int64)
        assert len(w) == abi.GS_NUM_AUX_TYPES
        self._chk(lib().gs_ext_configure_aux(self._h, abi.ptr(w)), "gs_ext_configure_aux")

    def upsert_aux_devices(self, devs, idx=None):
        devs = np.ascontiguousarray(devs, dtype=abi.NODE_AUX_DEVICES_DTYPE)
        if idx is not None:
            idx = np.ascontiguousarray(idx, dtype=np.uint32)
        self._chk(lib().gs_node_aux_devices_upsert(self._h, abi.ptr(idx), abi.ptr(devs), len(devs)),
                  "gs_node_aux_devices_upsert")

    def aux_devices(self, node: int):
        out = np.zeros(1, abi.NODE_AUX_DEVICES_DTYPE)
        self._chk(lib().gs_node_aux_devices_get(self._h, node, abi.ptr(out)), "gs_node_aux_devices_get")
        return out[0]

    def schedule_ext_aux(self, pods, ext, aux=None, seq=None):
        """gs_schedule_ext_aux: (placements, EXT_PLACEMENT_DTYPE, AUX_PLACEMENT_DTYPE records); aux None = schedule_ext"""
        pods = np.ascontiguousarray(pods, dtype=abi.POD_DTYPE)
        ext = np.ascontiguousarray(ext, dtype=abi.POD_EXT_DTYPE)
        assert len(ext) == len(pods)
        if aux is not None:
            aux = np.ascontiguousarray(aux, dtype=abi.POD_AUX_DTYPE)
            assert len(aux) == len(pods)
        if seq is None:
            seq = np.arange(len(pods), dtype=np.uint64)
        seq = np.ascontiguousarray(seq, dtype=np.uint64)
        out = np.zeros(len(pods), abi.PLACEMENT_DTYPE)
        eo = np.zeros(len(pods), abi.EXT_PLACEMENT_DTYPE)
        ao = np.zeros(len(pods), abi.AUX_PLACEMENT_DTYPE)
        self._chk(lib().gs_schedule_ext_aux(self._h, abi.ptr(pods), abi.ptr(ext), abi.ptr(aux), len(pods), abi.ptr(seq),
                                            abi.ptr(out), abi.ptr(eo), abi.ptr(ao)), "gs_schedule_ext_aux")
        return out, eo, ao

    def ext_aux_reserved(self, uid: int):
        """gs_ext_aux_reserved_get: (node, AUX_PLACEMENT_DTYPE record) of an assumed pod's recorded Reserve, or None"""
        node = C.c_uint32(0)
        out = np.zeros(1, abi.AUX_PLACEMENT_DTYPE)
        rc = lib().gs_ext_aux_reserved_get(self._h, int(uid), C.byref(node), abi.ptr(out))
        self._chk(min(rc, 0), "gs_ext_aux_reserved_get")
        return (int(node.value), out[0]) if rc == 1 else None

    def ext_rows_aux(self, pod, ext, aux, seq: int = 0) -> dict:
        """ext_rows of a pod with RDMA / FPGA requests (gs_debug_ext_rows_aux): the same keys"""
        pod = np.ascontiguousarray(np.atleast_1d(pod), dtype=abi.POD_DTYPE)
        ext = np.ascontiguousarray(np.atleast_1d(ext), dtype=abi.POD_EXT_DTYPE)
        if aux is not None:
            aux = np.ascontiguousarray(np.atleast_1d(aux), dtype=abi.POD_AUX_DTYPE)
        n = self.cfg.num_nodes
        rows = np.zeros((len(abi.EXT_ROW_KEYS), n), np.int32)
        nom = np.zeros(n, np.uint64)
        res = np.zeros(len(abi.EXT_ROWS_RESULT_KEYS), np.int64)
        self._chk(lib().gs_debug_ext_rows_aux(self._h, abi.ptr(pod), abi.ptr(ext), abi.ptr(aux), int(seq), abi.ptr(rows),
                                              abi.ptr(nom), abi.ptr(res)), "gs_debug_ext_rows_aux")
        return abi.ext_rows_dict(rows, nom, res)

    # ---- NodeNUMAResource state
    def register_topology(self, topo) -> int:
        t = abi.GsCpuTopology.from_buffer_copy(np.ascontiguousarray(np.atleast_1d(topo), abi.TOPOLOGY_DTYPE).tobytes())
        out = C.c_int32()
        self._chk(lib().gs_topology_register(self._h, C.byref(t), C.byref(out)), "gs_topology_register")
        return out.value

    def upsert_numa(self, numa, idx=None):
        numa = np.ascontiguousarray(numa, dtype=abi.NODE_NUMA_DTYPE)
        if idx is not None:
            idx = np.ascontiguousarray(idx, dtype=np.uint32)
        self._chk(lib().gs_nodes_numa_upsert(self._h, abi.ptr(idx), abi.ptr(numa), len(numa)), "gs_nodes_numa_upsert")

    def update_allocations(self, node_idx, allocs):
        node_idx = np.ascontiguousarray(node_idx, dtype=np.uint32)
        allocs = np.ascontiguousarray(allocs, dtype=abi.POD_ALLOCATION_DTYPE)
        self._chk(lib().gs_numa_allocations_update(self._h, abi.ptr(node_idx), abi.ptr(allocs), len(allocs)),
                  "gs_numa_allocations_update")

    def release_allocations(self, node_idx, uids):
        node_idx = np.ascontiguousarray(node_idx, dtype=np.uint32)
        uids = np.ascontiguousarray(uids, dtype=np.uint64)
        self._chk(lib().gs_numa_allocations_release(self._h, abi.ptr(node_idx), abi.ptr(uids), len(uids)),
                  "gs_numa_allocations_release")

    def allocation(self, node: int, uid: int):
        out = abi.GsPodAllocation()
        rc = lib().gs_numa_allocation_get(self._h, node, uid, C.byref(out))
        if rc < 0:
            self._chk(rc, "gs_numa_allocation_get")
        return np.frombuffer(bytes(out), abi.POD_ALLOCATION_DTYPE)[0] if rc == 1 else None

    # ---- multi-GPU
    def comm_init_rccl(self, uid: bytes, nranks: int, rank: int):
        buf = (C.c_uint8 * 128).from_buffer_copy(uid)
        self._chk(lib().gs_comm_init_rccl(self._h, buf, nranks, rank), "gs_comm_init_rccl")

    def comm_init_callback(self, nranks: int, rank: int, allgather):
        """allgather(send: bytes) -> list[bytes] of every rank's payload (rank order)."""
        def _cb(user, send, recv, nbytes):
            try:
                data = C.string_at(send, nbytes)
                parts = allgather(data)
                blob = b"".join(parts)
                C.memmove(recv, blob, len(blob))
                return 0
            except Exception:
                return -1
        self._cb = abi.ALLGATHER_FN(_cb)
        self._chk(lib().gs_comm_init_callback(self._h, nranks, rank, self._cb, None), "gs_comm_init_callback")

    def comm_init_local(self, group: "LocalGroup", rank: int):
        """In-process device transport: this context is rank `rank` of `group` (ranks as threads of this process)."""
        self._group = group   # the group outlives its contexts
        self._chk(lib().gs_comm_init_local(self._h, group._h, rank), "gs_comm_init_local")

    def stats(self) -> dict:
        s = abi.GsStats()
        self._chk(lib().gs_get_stats(self._h, C.byref(s)), "gs_get_stats")
        return {k: getattr(s, k) for k, _ in abi.GsStats._fields_}

    def reset_stats(self):
        self._chk(lib().gs_reset_stats(self._h), "gs_reset_stats")

    def reset(self):
        """Rebuild the HBM mirror from the host state after a failed call (gs_reset)."""
        self._chk(lib().gs_reset(self._h), "gs_reset")

    def synchronize(self):
        self._chk(lib().gs_synchronize(self._h), "gs_synchronize")

    def mirror_check(self) -> int:
        rc = lib().gs_debug_mirror_check(self._h)
        if rc < 0:
            self._chk(rc, "gs_debug_mirror_check")
        return rc

    def commit_counters(self) -> dict:
        """Diagnostics: the speculative commit's event counters over the engine's life (gs_debug_commit_counters;
        abi.COMMIT_COUNTER_KEYS). Needs GS_COMMIT_STAMPS=1 in the environment when the engine is created."""
        out = np.zeros(len(abi.COMMIT_COUNTER_KEYS), np.uint64)
        self._chk(lib().gs_debug_commit_counters(self._h, abi.ptr(out)), "gs_debug_commit_counters")
        return {k: int(v) for k, v in zip(abi.COMMIT_COUNTER_KEYS, out)}

    def numa_merge(self, cases):
        """Diagnostics: the device's topology-manager Merge on gs_merge_case records (gs_debug_numa_merge)."""
        cases = np.ascontiguousarray(cases, dtype=abi.MERGE_CASE_DTYPE)
        out = np.zeros(len(cases), abi.MERGE_RESULT_DTYPE)
        self._chk(lib().gs_debug_numa_merge(self._h, abi.ptr(cases), len(cases), abi.ptr(out)), "gs_debug_numa_merge")
        return out

    def pair_probe(self, pods, nodes, pod_of, mode: int):
        """Diagnostics: (scores, cycles) of the commit kernel's pair evaluation on mirror rows (gs_debug_pair_probe)."""
        pods = np.ascontiguousarray(pods, dtype=abi.POD_DTYPE)
        nodes = np.ascontiguousarray(nodes, dtype=np.uint32)
        pod_of = np.ascontiguousarray(pod_of, dtype=np.int32)
        n = len(nodes)
        scores = np.zeros(n * (64 if mode == 1 else 1), np.int32)
        cycles = np.zeros(10 * n, np.uint64)
        self._chk(lib().gs_debug_pair_probe(self._h, abi.ptr(pods), len(pods), abi.ptr(nodes), abi.ptr(pod_of), n, mode,
                                            abi.ptr(scores), abi.ptr(cycles)), "gs_debug_pair_probe")
        self.last_probe_stamps = cycles[2 * n:].reshape(n, 8).astype(np.int64)
        return (scores.reshape(n, 64) if mode == 1 else scores), cycles[:n], cycles[n:2 * n]

    def ext_rows(self, pod, ext, seq: int = 0) -> dict:
        """Diagnostics: the per-node view of one extension pod and its select result (gs_debug_ext_rows); nothing is
        reserved or assumed. Keys: abi.EXT_ROW_KEYS (arrays over the nodes), nominated_uid, abi.EXT_ROWS_RESULT_KEYS."""
        pod = np.ascontiguousarray(np.atleast_1d(pod), dtype=abi.POD_DTYPE)
        ext = np.ascontiguousarray(np.atleast_1d(ext), dtype=abi.POD_EXT_DTYPE)
        n = self.cfg.num_nodes
        rows = np.zeros((len(abi.EXT_ROW_KEYS), n), np.int32)
        nom = np.zeros(n, np.uint64)
        res = np.zeros(len(abi.EXT_ROWS_RESULT_KEYS), np.int64)
        self._chk(lib().gs_debug_ext_rows(self._h, abi.ptr(pod), abi.ptr(ext), int(seq), abi.ptr(rows), abi.ptr(nom),
                                          abi.ptr(res)), "gs_debug_ext_rows")
        return abi.ext_rows_dict(rows, nom, res)

    def verify_cpusets(self, on: bool = True):
        """Re-run the host takeCPUs for every cpuset the commit kernel selects (schedule fails on a difference)."""
        self._chk(lib().gs_debug_verify_cpuset(self._h, int(on)), "gs_debug_verify_cpuset")


def unique_id() -> bytes:
    buf = (C.c_uint8 * 128)()
    rc = lib().gs_comm_unique_id(buf)
    if rc != 0:
        raise GpuScoreError(f"gs_comm_unique_id failed: {rc}")
    return bytes(buf)
