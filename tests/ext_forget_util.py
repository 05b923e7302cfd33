"""The reference side of forgetting a pod the extension path placed. The oracle's ForgetPod (or_pods_forget) knows
NodeInfo, the podAssignCache and the NUMA allocations only, so the two plugin Unreserves and the scalar part of
NodeInfo.RemovePod are restated here through the oracle's public calls:

  DeviceShare Unreserve   deviceshare/plugin.go:432-451 -> updateCacheUsed(..., false), device_cache.go:124-201:
                          used[minor] = SubtractWithNonNegativeResult(used[minor], allocation.Resources) on the minors
                          the Device object still has; nothing on a node without one
  Reservation Unreserve   reservation/plugin.go:572-594 -> cache.go:175-177 -> RemoveAssignedPod
                          (frameworkext/reservation_info.go:390-401): Allocated = SubtractWithNonNegativeResult(Allocated,
                          Mask(requests, ResourceNames)) (keys kept, a missing key comes back as 0), the pod leaves
                          AssignedPods; nothing when the reservation is gone
  NodeInfo.RemovePod      [upstream] the GPU-name and extended-resource scalars leave Requested

`OracleExt` wraps an Oracle as the engine of oracle/coscheduling.py schedule_sequential (schedule / forget) and of
koordinator_amd/gang.py schedule_with_gangs(ext=...) (schedule_ext / forget), remembering each placed pod's plugin
inputs and gs_ext_placement so that its forget can run the helper."""
import numpy as np

from koordinator_amd import abi

DS, RS = abi.GS_EXT_DEVICESHARE, abi.GS_EXT_RESERVATION


def oracle_forget_ext(o, node, pod, ext, xout, enabled=DS | RS):
    """Unreserve + ForgetPod of `pod` (POD_DTYPE record) assumed on `node` by o.schedule_ext with the inputs `ext`
    (POD_EXT_DTYPE record, None for a plain pod) and the result `xout` (EXT_PLACEMENT_DTYPE record, or None)."""
    node = int(node)
    pod = np.ascontiguousarray(np.atleast_1d(pod), abi.POD_DTYPE)
    if ext is not None and xout is not None:
        dev = np.zeros(1, abi.NODE_DEVICES_DTYPE)
        dev[0] = o.devices(node)
        before = dev.tobytes()
        mask = int(xout["gpu_minor_mask"])
        if dev["has_device"][0] and mask:
            inst = np.asarray(xout["gpu_per_instance"], np.int64)
            for g in range(int(dev["num_gpus"][0])):
                if mask >> int(dev["gpus"]["minor"][0, g]) & 1:
                    dev["gpus"]["used"][0, g] = np.maximum(0, dev["gpus"]["used"][0, g] - inst)
        uid = int(xout["reservation_uid"])
        r = o.reservation(uid) if uid else None
        if r is not None:
            rsv = np.zeros(1, abi.RESERVATION_DTYPE)
            rsv[0] = r
            slots = int(r["resource_names_mask"]) & int(pod["request_mask"][0]) & 0x7F
            amask = int(r["allocated_mask"])
            for s in range(7):
                if slots >> s & 1:
                    have = int(r["allocated"][s]) if amask >> s & 1 else 0
                    rsv["allocated"][0, s] = max(0, have - int(pod["requests"][0, s]))
            rsv["allocated_mask"] = amask | slots
            rsv["assigned_pods"] = max(0, int(r["assigned_pods"]) - 1)
            o.upsert_reservations(rsv)
        gm = int(ext["gpu_request_mask"]) & 0x1F
        if (enabled & DS) and gm:
            for n in range(abi.GS_NUM_GPU_NAMES):
                if gm >> n & 1:
                    dev["requested"][0, n] -= int(ext["gpu_requests"][n])
        xm = int(ext["xres_request_mask"]) & ((1 << abi.GS_MAX_XRES) - 1)
        for x in range(abi.GS_MAX_XRES):
            if xm >> x & 1:
                dev["xres_requested"][0, x] -= int(ext["xres_requests"][x])
        if dev.tobytes() != before:
            o.upsert_devices(dev, idx=[node])
    o.forget(np.array([node], np.uint32), pod)


class OracleExt:
    """An Oracle with the Reservation / DeviceShare state loaded, as a gang driver's engine."""

    def __init__(self, o, pods, ext, enabled=DS | RS):
        self.o, self.enabled = o, enabled
        self.ext_of = {int(u): ext[k].copy() for k, u in enumerate(pods["uid"])}
        self.placed = {}         # uid -> (gs_pod_ext, gs_ext_placement) of an assumed pod
        self.forgot_gpu = []     # uids of forgotten pods that held GPU minors / a reservation
        self.forgot_rsv = []
        self.freed_minors = {}   # node -> minors a forget freed; reservation uids a forget freed
        self.freed_rsv = set()
        self.reused_gpu = self.reused_rsv = 0   # later pods taking a freed minor / assumed into a freed reservation

    def __getattr__(self, name):
        return getattr(self.o, name)

    def schedule_ext(self, pods, ext, seq=None):
        pods = np.ascontiguousarray(pods, abi.POD_DTYPE)
        ext = np.ascontiguousarray(ext, abi.POD_EXT_DTYPE)
        out, xo = self.o.schedule_ext(pods, ext, seq)
        for k in np.flatnonzero(out["node"] >= 0):
            self.placed[int(pods["uid"][k])] = (ext[k].copy(), xo[k].copy())
            node, mask, ruid = int(out["node"][k]), int(xo["gpu_minor_mask"][k]), int(xo["reservation_uid"][k])
            if mask & self.freed_minors.get(node, 0):
                self.reused_gpu += 1
                self.freed_minors[node] &= ~mask
            if ruid in self.freed_rsv:
                self.reused_rsv += 1
        return out, xo

    def schedule(self, pods, seq=None):
        pods = np.ascontiguousarray(pods, abi.POD_DTYPE)
        ext = np.array([self.ext_of[int(u)] for u in pods["uid"]], abi.POD_EXT_DTYPE)
        return self.schedule_ext(pods, ext, seq)[0]

    def forget(self, nodes, pods):
        pods = np.ascontiguousarray(pods, abi.POD_DTYPE)
        for k in range(len(pods)):
            uid = int(pods["uid"][k])
            e, x = self.placed.pop(uid, (None, None))
            if x is not None and int(x["gpu_minor_mask"]):
                self.forgot_gpu.append(uid)
                self.freed_minors[int(nodes[k])] = self.freed_minors.get(int(nodes[k]), 0) | int(x["gpu_minor_mask"])
            if x is not None and int(x["reservation_uid"]):
                self.forgot_rsv.append(uid)
                self.freed_rsv.add(int(x["reservation_uid"]))
            oracle_forget_ext(self.o, nodes[k], pods[k:k + 1], e, x, self.enabled)


def same_ext_state(c, a, b, superset=False):
    """Every reservation (allocated_mask included) and every node's Device row and scalars of two engines / oracles.
    superset: a's allocated_mask may hold keys b's lacks, with the value 0. That is the state a batched gang driver
    leaves against the one-pod-at-a-time order: a run's withdrawn placement was assumed into a reservation and
    forgotten, and the reference's subtraction keeps the zero-valued keys; the sequential order never assumed it."""
    for r in c.ext["reservations"]:
        x, y = a.reservation(int(r["uid"])), b.reservation(int(r["uid"]))
        assert (x is None) == (y is None), int(r["uid"])
        if x is None:
            continue
        for f in ("assigned_pods", "node", "owner_key"):
            assert x[f] == y[f], (int(r["uid"]), f, x[f], y[f])
        mx, my = int(x["allocated_mask"]), int(y["allocated_mask"])
        assert (mx & my) == my if superset else mx == my, (int(r["uid"]), mx, my)
        for s in range(abi.GS_NUM_RES):
            vx = int(x["allocated"][s]) if mx >> s & 1 else 0
            vy = int(y["allocated"][s]) if my >> s & 1 else 0
            assert vx == vy, (int(r["uid"]), s, vx, vy)
    for i in range(c.num_nodes):
        x, y = a.devices(i), b.devices(i)
        for f in ("requested", "xres_requested"):
            assert np.array_equal(x[f], y[f]), (i, f)
        assert np.array_equal(x["gpus"]["used"], y["gpus"]["used"]), i
