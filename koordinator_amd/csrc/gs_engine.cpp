// gs_engine.cpp — libgpuscore host side: the C-ABI of include/gpuscore.h over the HIP kernels.
//
// Owns the host mirror of the scheduler state the hot path reads (NodeInfo rows, NodeMetrics, the
// LoadAware podAssignCache) and its HBM structure-of-arrays image. Per-node derived columns (LoadAware
// usage verdicts, estimated usage, free capacities) are recomputed on the host only for rows an event
// touched and scattered to HBM; pod placements made by gs_schedule are applied on the device by the
// commit kernel and replayed on the host mirror, so no row crosses PCIe for them.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <vector>
#include <condition_variable>
#include <deque>
#include <memory>
#include <mutex>
#include <thread>
#include <atomic>

#include "../../include/gpuscore.h"
#include "gs_ext.h"
#include "gs_kernels.h"
#include "gs_numa_host.h"
#include "gs_owned.h"
#include "gs_preempt.h"
#include "gs_reasons.h"

using namespace gs;

namespace {

constexpr int64_t kDefaultMilliCPURequest = 250;              // loadaware/estimator/default_estimator.go:36
constexpr int64_t kDefaultMemoryRequest = 200LL * 1024 * 1024; // loadaware/estimator/default_estimator.go:38
constexpr int64_t kDefaultReportIntervalNs = 60LL * 1000000000LL;
constexpr int64_t kZeroTime = INT64_MIN;
constexpr int64_t kMaxExact = 1LL << 53;                      // value bound for the exact int64 score paths

struct Assigned {
  int64_t ts;
  gs_pod pod;
};

struct HostNode {
  gs_node node{};
  bool valid = false;
  gs_node_metric metric{};
  std::vector<gs_pod_metric> pms;
  std::unordered_map<uint64_t, Assigned> assigned;   // podAssignCache.podInfoItems[node]
};

struct Vec2 {
  int64_t v[2] = {0, 0};
  uint32_t mask = 0;
  bool has(int r) const { return mask & (1u << r); }
  int64_t get(int r) const { return has(r) ? v[r] : 0; }
  void add(int r, int64_t x) { v[r] = get(r) + x; mask |= 1u << r; }
};

Vec2 usage_of(const gs_usage& u) {
  Vec2 o;
  if (u.mask & GS_USAGE_CPU) { o.v[0] = u.cpu_milli; o.mask |= 1; }
  if (u.mask & GS_USAGE_MEMORY) { o.v[1] = u.memory; o.mask |= 2; }
  if (u.mask & GS_USAGE_OTHER) o.mask |= GS_USAGE_OTHER;
  return o;
}

// The reports a batch's device pass computes behind its commit: the FitError diagnosis' wide pass (rows: with the
// status rows), or the top-N score tables' pass (topn > 0). A run asks for one kind at most.
struct ReportMode {
  bool diag = false, rows = false;
  uint32_t topn = 0;
  bool any() const { return diag || topn; }
};
// Where a run's reports go (all null: a plain run computes none).
struct Reports {
  gs_fit_diagnosis* diag = nullptr;   // gs_schedule_diag: the FitError diagnosis of each pod
  gs_status_map* map = nullptr;       // gs_schedule_diag_nodes: the per-node status rows of those pods (with diag)
  gs_top_scores* top = nullptr;       // gs_schedule_top_scores: the top-N score table of each scored pod
  uint32_t topn() const { return top ? top->topn : 0u; }
  // whether the run's batches run the wide pass with the status rows (a map without rows keeps the counters-only kernels)
  bool wants_rows() const { return diag && map && map->cap_rows; }
  ReportMode mode() const { return ReportMode{diag != nullptr, wants_rows(), topn()}; }
};

// One of the two per-batch buffer sets: everything a batch in flight reads or writes on its own. While one slot's batch
// commits, the next batch is staged and enqueued speculatively on the other slot (schedule_stream).
struct Slot {
  Event ev_go, ev_evdone;
  Event ev[6];                      // timing marks: eval start [0] / end [1], forced commit [3], commit end [4]; [5] readback
  bool untimed = false;             // the batch recorded no timing events (a short direct batch)
  DevBuf<int16_t> d_S;              // score rows of the slot's batch
  DevBuf<uint8_t> d_aff;            // [pod][ld] Filter-time NUMA affinity of policy nodes (eval -> commit Reserve)
  // pods | seq and committed | out share one allocation each (device and pinned host): one copy per batch each way
  DevBuf<PodVec> d_pods;
  PinnedBuf<PodVec> h_pods;
  DevBuf<int32_t> d_committed;
  PinnedBuf<int32_t> h_committed;
  DevBuf<uint8_t> d_lst;            // overlapped cand (one shard): the slot's lists + headers, and its histograms
  DevBuf<uint32_t> d_hist;
  DevBuf<uint8_t> d_landed;         // the landed slab the slot's commit leaves for the next batch's fix-up (cand_overlap)
  // Views, not owners: seq behind the slot's pods and out behind its committed words; the slot's part of gs_ctx's
  // tb_all (gs_create) and of its sx_send_all, sx_recv_all and d_xerr (alloc_exchange)
  uint64_t *d_seq = nullptr, *h_seq = nullptr;
  PlacementDev *d_out = nullptr, *h_out = nullptr;
  int32_t* d_tb = nullptr;          // the slot's tie-break records: cand_kernel writes the next batch's beside this commit
  uint8_t* d_sx_send = nullptr;     // score-row exchange: [B x pld int16 | B x pld u8 | ... | XTag]
  uint8_t* d_sx_recv = nullptr;     // R blocks
  // the verdict on the batch's exchange tags (score rows: the slot's own, written by unpack_scores_kernel; levels:
  // merge_levels_kernel's, one block for both slots; one rank: none)
  int32_t* d_xerr = nullptr;
  ReportMode rep;                   // the reports the slot's batch runs behind its commit (launch_batch)
  // FitError diagnosis (gs_schedule_diag; allocated by the context's first such run, alloc_diag)
  Event ev_dg;                      // the wide pass's end (a readback on st_rb waits for it)
  DevBuf<uint32_t> d_diag;          // [MAX_BATCH][DIAG_WORDS]: the wide pass's counters, read back with the placements
  PinnedBuf<uint32_t> h_diag;
  // the landed pass of the slot's batch (landed_pass): one staged block (row versions | their slab indices | pod
  // vectors | version indices), the slab the versions are scattered into, and the pass's counters
  PinnedBuf<uint8_t> h_dgl;
  DevBuf<uint8_t> d_dgl;
  DevBuf<int64_t> dgl_i64;
  DevBuf<int32_t> dgl_i32;
  DevBuf<uint32_t> d_ldiag;
  PinnedBuf<uint32_t> h_ldiag;
  // the diagnosis' status map (gs_schedule_diag_nodes; allocated by the context's first such run, alloc_map)
  DevBuf<uint16_t> d_words;         // [MAX_BATCH][npad]: row f = the batch's f-th pod with no node, in queue order
  PinnedBuf<uint16_t> h_words;      // the rows the host asked for (fetch_rows), same stride
  int rows_fetched = 0;             // rows of the slot's batch on their way to h_words (fetch_rows -> apply_batch)
  Event ev_rows;                    // ... the copy's end: the slot's next wide pass with rows waits for it
  bool rows_in_flight = false;      // ev_rows is recorded and no later pass has waited for it yet
  DevBuf<uint16_t> d_lwords;        // [pod of the landed pass][landed node]: the landed pass's words
  PinnedBuf<uint16_t> h_lwords;
  // the top-N score tables (gs_schedule_top_scores; allocated by the context's first such run, alloc_top)
  DevBuf<uint8_t> d_top;            // the pass's counts and rows (TOP_BYTES), read back with the placements
  PinnedBuf<uint8_t> h_top;
  DevBuf<TopLanded> d_ltop;         // [pod of the landed pass][landed node]: the landed pass's totals and plugin scores
  PinnedBuf<TopLanded> h_ltop;
};

// The ElasticQuota PostFilter dry run (gs_preempt_dry_run): the resident-pod table with its device image and the dry
// run's buffers. Created by the context's first gs_node_pods_* or dry-run call: a context that makes neither holds none.
struct PreemptState {
  explicit PreemptState(uint32_t n) : table(n) {}
  PreemptTable table;
  bool rebuild = false;             // gs_reset: the next dry run uploads the whole image
  std::vector<uint32_t> numa_idx;   // the nodes with a NUMA topology policy, as d_numa_idx holds them
  DevBuf<uint32_t> d_numa_idx;
  DevBuf<PrePod> d_pods;            // MAX_BATCH preemptors
  DevBuf<PrePart> d_result;
  DevBuf<uint16_t> d_rows;          // the status rows the call's preemptors name
  DevBuf<uint8_t> d_status;
  DevBuf<uint64_t> d_bits;
  DevBuf<PrePart> d_parts;
  size_t rows_cap = 0, out_cap = 0, parts_cap = 0;   // rows of d_rows, preemptors of d_status / d_bits, parts
  // PodDisruptionBudgets (gs_preempt_dry_run_pdb): none until the first gs_pdbs_upsert, gs_node_pods_set_pdbs or
  // gs_preempt_dry_run_pdb
  struct Pdb {
    PdbTable table;
    bool rebuild = false;           // gs_reset: the next dry run uploads the whole budget table
    DevBuf<uint64_t> d_viol;        // [preemptors][N][2]
    DevBuf<uint8_t> d_nviol;        // [preemptors][N]
    DevBuf<PrePartPdb> d_parts, d_result;
    size_t out_cap = 0, parts_cap = 0;
  };
  std::unique_ptr<Pdb> pdb;
};

}  // namespace

// ---- asynchronous submissions (gs_schedule_submit / gs_schedule_wait): a worker thread runs schedule_stream over
// the submitted runs in order, taking the next run while the current one's last batch is in flight
struct AsyncRun {
  std::vector<gs_pod> pods;
  std::vector<uint64_t> seq;
  gs_placement* out = nullptr;
  Reports rep;                        // gs_schedule_submit_diag / _diag_nodes / _top_scores
  uint64_t ticket = 0;
  int rc = 1;   // 1: not complete
  std::string err;
};
struct AsyncQueue {
  std::thread th;
  std::mutex mu;
  std::condition_variable cv_work, cv_done;
  std::deque<std::shared_ptr<AsyncRun>> pending;                  // submitted, not yet taken by the worker
  std::unordered_map<uint64_t, std::shared_ptr<AsyncRun>> runs;   // submitted, not yet waited for
  uint64_t next_ticket = 1;
  bool busy = false, stop = false;
};


// In-process device transport (gs_comm_init_local): the ranks are threads of one process. Per exchange each rank
// publishes its send block and the event recorded after its tag, the threads meet (host barrier, no GPU wait), every
// rank enqueues on its stream a wait on each rank's event and the device-to-device copy of its block, publishes the
// event after its copies, and after a second meeting waits on every rank's copies event on its stream: the collective
// is complete on a rank's stream only once every rank has read its block, as with ncclAllGather, and the host never
// waits for the GPU. A rank that does not arrive within GS_LOCAL_WAIT_S (60 s) fails the call with GS_ECOMM.
struct gs_local_group {
  int n = 0;
  std::mutex mu;
  std::condition_variable cv;
  int arrived = 0;
  uint64_t gen = 0;
  bool broken = false;
  std::vector<const uint8_t*> send;
  std::vector<size_t> bytes;
  std::vector<hipEvent_t> ready, done;
  // true: every rank arrived; false: the wait expired or the group is broken (a rank failed)
  bool meet(double limit_s) {
    std::unique_lock<std::mutex> lk(mu);
    if (broken) return false;
    const uint64_t g = gen;
    if (++arrived == n) {
      arrived = 0;
      ++gen;
      cv.notify_all();
      return true;
    }
    const bool ok = cv.wait_for(lk, std::chrono::duration<double>(limit_s), [&] { return gen != g || broken; });
    if (!ok || broken) {
      broken = true;
      cv.notify_all();
      return false;
    }
    return true;
  }
};

// What the extension path's Reserve (ext_schedule_one) applied for one assumed pod: gs_pods_forget takes exactly this
// back (DeviceShare Unreserve, Reservation Unreserve, NodeInfo.RemovePod of the scalars), gs_ext_reserved_get reports it.
struct ExtReserved {
  uint32_t node = 0;
  uint32_t gpu_minor_mask = 0;                  // gs_ext_placement.gpu_minor_mask
  int32_t gpu_count = 0;
  uint32_t gpu_keys = 0;                        // the keys of each minor's DeviceAllocation.Resources (bit = gs_gpu_res)
  int64_t gpu_per_instance[GS_NUM_GPU_RES] = {};
  uint64_t reservation_uid = 0;                 // 0: assumed into none
  uint32_t rsv_slots = 0;                       // slots of the reservation's Allocated the pod's requests were added to
  int64_t rsv_added[GS_NUM_RES] = {};
  uint32_t gpu_names = 0, xres = 0;             // NodeInfo.AddPod: GPU names / registered extended resources added
  int64_t gpu_name_req[GS_NUM_GPU_NAMES] = {};
  int64_t xres_req[GS_MAX_XRES] = {};
  gs_aux_placement aux = {};                    // RDMA / FPGA minors and per-instance amounts (ext_aux_reserve)
};

// Members are destroyed in reverse order: the buffers go first, then the events, then the streams (gs_destroy).
struct gs_ctx {
  Stream st;
  Stream st2;                               // side stream: eval_kernel beside eval_numa_kernel
  Stream st_ev;                             // eval passes: a batch's eval runs beside the previous batch's commit
  Stream st_rb;                             // a batch's placement readback, off the stream the next batch runs on
  Stream st_dg;                             // FitError diagnosis: the landed pass, off the commit stream (alloc_diag)
  Event ev_fork, ev_join;
  std::vector<Event> x_ev;                  // RCCL all-gather start / end events not yet accounted (exchange_ms)
  int x_pending = 0;
  Event lg_ready, lg_done;                  // in-process device transport: this rank's events of an exchange
  // double-buffered per-batch state: the next batch is enqueued speculatively before the current one is read back
  // (gs_schedule). cur_slot: the slot whose batch is current; between runs its buffers serve as scratch (current_slot)
  Slot slot[2];
  int cur_slot = 0;
  std::unordered_map<uint64_t, ExtReserved> ext_reserved;   // assumed pods' extension-path Reserves (gs_schedule_ext)
  gs_config cfg{};
  std::string err;
  std::unique_ptr<AsyncQueue> aq;   // gs_schedule_submit's worker (created by the first submission)
  uint32_t N = 0, npad = 0;
  uint32_t window_k = 0;                    // node sampling: numFeasibleNodesToFind(N) (0 = every node)
  uint32_t next_start = 0;                  // [upstream] Scheduler.nextStartNodeIndex
  // device mirror (mv: views of the two)
  DevBuf<int64_t> mirror_i64;
  DevBuf<int32_t> mirror_i32;
  MirrorView mv{};
  // batch buffers
  int B = MAX_BATCH;
  uint32_t ld = 0;
  DevBuf<uint8_t> d_xchg_send;      // local lists + headers (contiguous, all-gathered)
  DevBuf<uint8_t> d_xchg_recv;      // R blocks
  DevBuf<uint8_t> d_xmerged;        // several ranks, speculative commit: the R blocks' levels merged into one block
  size_t xchg_bytes = 0;
  int lstride = LCAP;               // listed nodes per pod in the local / exchanged blocks (XCAP: several ranks, spec)
  DevBuf<int32_t> tb_all;           // speculative commit: tie-break records of the batches' pods, both slots' (Slot::d_tb)
  DevBuf<RowStat> d_rowstat;
  DevBuf<int32_t> d_sel;
  DevBuf<int64_t> d_stage_rows;     // flush_rows staging (device / pinned): rows, then their node indices
  PinnedBuf<int64_t> h_stage_rows;
  uint32_t stage_cap = 0;
  PinnedBuf<uint8_t> h_xchg_send, h_xchg_recv;   // host-callback transport
  bool cand_overlap = false;        // GS_CAND_OVERLAP (default on): cand beside the previous commit, fix_levels after it
  DevBuf<uint32_t> d_cscratch;      // launch_cand's short-batch split (slice histograms, slice offsets)
  // host mirror
  std::vector<HostNode> nodes;
  std::vector<uint8_t> row_dirty;
  std::vector<uint32_t> dirty_list;
  std::unordered_map<uint64_t, uint32_t> uid_node;
  std::unordered_map<uint64_t, int> metric_names;
  int64_t now = 0;
  bool prep_stale = true;
  Profile pf{};
  int max_score = 0;
  // sharding
  int nranks = 1, rank = 0;
  uint32_t n0 = 0, n1 = 0;          // the node range the levels, fixes and commit see (all nodes: one rank, scores)
  // Several ranks exchange either their score rows (sgather, the default: every rank evaluates its shard [e0, e1), the
  // all-gather makes the full rows, and the one-shard pipeline runs on every rank) or their candidate levels
  // (GS_XCHG=levels: n0/n1 = the shard, merged level lists, the multi-shard commit)
  bool sgather = false;
  uint32_t e0 = 0, e1 = 0;          // the node range this rank evaluates
  uint32_t sx_per = 0, sx_pld = 0;  // nodes per shard, the block's row stride
  size_t sx_bytes = 0;              // one rank's score block (tag included)
  DevBuf<uint8_t> sx_send_all, sx_recv_all;   // both slots' send blocks (Slot::d_sx_send), R-block sets (d_sx_recv)
  PinnedBuf<uint8_t> h_sx_send, h_sx_recv;    // host-callback transport
  uint32_t n_valid = 0;   // nodes upserted at least once (ready())
  ncclComm_t comm = nullptr;
  gs_allgather_fn cb = nullptr;
  void* cb_user = nullptr;
  gs_local_group* lg = nullptr;     // in-process device transport (tests: ranks as threads)
  // exchange sequence (XTag): every exchange's block carries (site, seq, batch, rank); all ranks check all tags
  std::atomic<uint64_t> xseq{0};    // exchanges so far
  std::atomic<uint64_t> xbatch{0};  // batch passes launched so far (launch_batch)
  DevBuf<int32_t> d_xerr;           // the tag verdicts of unpack_scores_kernel / merge_levels_kernel (Slot::d_xerr)
  DevBuf<uint8_t> d_xsmall;         // small exchanges (row stats, selection): [own block | R blocks] of XSMALL bytes
  PinnedBuf<uint8_t> h_xsmall;      // their R blocks read back
  int64_t dbg_xskew_rank = -1;      // GS_DEBUG_XCHG_SKEW=rank:batch (tests): that rank skips one sequence number there
  uint64_t dbg_xskew_batch = 0;
  // GS_WATCHDOG_S=<seconds> (diagnostics): a thread reports on stderr any host wait of the scheduling path that lasts
  // longer, naming the wait (Where markers), the batch pass and the exchange count
  std::atomic<const char*> where{nullptr};
  std::atomic<int64_t> where_t{0};
  std::thread watchdog;
  std::atomic<bool> wd_stop{false};
  gs_stats stats{};
  DevBuf<uint64_t> d_stamps;      // GS_COMMIT_STAMPS=1: commit-kernel phase cycle sums
  uint64_t stats_all_pods = 0;     // pods placed by gs_schedule over the context's life (stamp averages)
  uint64_t spec_split_launches = 0, spec_single_launches = 0;   // commit_spec_kernel launches by pipeline (launch_commit_spec's rule)
  // GS_HOST_TIMING=1: host time per batch of schedule_stream, by phase (printed by gs_destroy)
  bool host_timing = false;
  double ht_wait = 0, ht_apply = 0, ht_stage = 0, ht_launch = 0, ht_max_busy = 0;
  uint64_t ht_batches = 0, ht_busy_hist[8] = {};
  // ... and of the batch reports, per kind ([0] FitError diagnosis, [1] top-N score tables): deriving the landed-row
  // versions, the landed pass (upload to results, waited for), merging into the caller's buffers
  struct ReportTiming {
    double derive = 0, landed = 0, merge = 0;
    uint64_t batches = 0, versions = 0, pods = 0;
  } hr[2];
  uint64_t hd_map_rows = 0, hd_map_bytes = 0;   // status map: rows read back, and their bytes with the landed words'
  // ... and of gs_schedule_ext: per extension pod (records, flushes, the device chain up to the host's wake-up, the
  // Reserves) and per plain run (the whole gs_schedule call)
  double hx_prep = 0, hx_flush = 0, hx_gpu = 0, hx_reserve = 0, hx_plain = 0;
  uint64_t hx_pods = 0, hx_runs = 0;
  // NodeNUMAResource: per-node TopologyOptions + NodeAllocation mirror, registered CPU topologies
  std::vector<NumaNode> numa;
  std::vector<std::shared_ptr<TopoClass>> topos;
  std::shared_ptr<TopoClass> empty_topo = std::make_shared<TopoClass>();
  std::unordered_map<uint64_t, uint32_t> numa_uid_node;   // pods holding a NodeAllocation record
  bool numa_on = false;
  // the shard's nodes with a NUMA topology policy (eval_numa_kernel's work list), rebuilt when policies change
  DevBuf<uint32_t> d_numa_idx;
  uint32_t numa_n = 0;
  DevBuf<int64_t> slab_i64;                  // the eval pass's dense copy of the NUMA-policy rows (gather_numa_kernel)
  DevBuf<int32_t> slab_i32;
  MirrorView slab_mv{nullptr, nullptr, 0};   // (views of the two)
  uint32_t slab_cap = 0;
  bool numa_idx_stale = true;
  // the extension path's list over [n0, n1) (all nodes under the score-row exchange, where the batch path's list covers
  // the rank's shard only): its own buffer, so pods alternating between the two paths rebuild neither
  DevBuf<uint32_t> d_xnuma_idx;
  uint32_t xnuma_n = 0;
  bool xnuma_stale = true;
  uint32_t numa_idx_lo = 0, numa_idx_hi = 0;   // the node range d_numa_idx lists (the batch path's shard [e0, e1))
  int64_t prep_now = INT64_MIN;             // `now` of the last full node_prep pass
  // registered topologies in bit-plane form (the commit kernel's cpuset Reserve), and the host re-check of
  // every device-chosen cpuset (GS_VERIFY_CPUSET=1)
  DevBuf<TopoDev> d_topos;
  bool verify_cpuset = false;
  // Reservation + DeviceShare (gs_ext.hip): host mirror of the nodes' GPU devices and of the reservation cache
  gs_ext_args ext{};
  std::vector<gs_node_devices> devs;             // per node (has_device = 0: no Device object)
  std::vector<uint8_t> dev_dirty;
  std::vector<uint32_t> dev_dirty_list;
  std::map<uint64_t, gs_reservation> rsv;        // reservationCache by uid (uid order = the harness's iteration order)
  std::vector<std::vector<uint64_t>> rsv_node;   // uids per node, ascending
  std::unordered_map<uint64_t, std::vector<uint64_t>> rsv_owner;   // owner key -> uids
  // RDMA / FPGA devices (gs_node_aux_devices_upsert): empty until the first upsert; the HBM image exists from the first
  // pod requesting one of the types on (ext_aux_alloc), and only then are rows marked dirty
  std::vector<gs_node_aux_devices> aux;
  std::vector<uint8_t> aux_dirty;
  std::vector<uint32_t> aux_dirty_list;
  int64_t aux_weights[GS_NUM_AUX_TYPES] = {0, 0};
  DevBuf<DevAuxNode> d_aux;
  PinnedBuf<DevAuxNode> h_aux_stage;
  DevBuf<DevAuxNode> d_aux_stage;
  DevBuf<DevNode> d_dev;
  PinnedBuf<DevNode> h_dev_stage;   // ext_flush_devices staging (pinned / device): images, then node indices
  DevBuf<DevNode> d_dev_stage;
  DevBuf<int32_t> d_xtot;
  DevBuf<int16_t> d_xds, d_xrs;
  DevBuf<int32_t> d_xnom;
  DevBuf<int32_t> d_xT;
  DevBuf<ExtOut> d_xout;
  PinnedBuf<unsigned char> h_xin;    // one extension pod's inputs, staged for ONE copy: ExtPod | PodVec | ExtRec[] |
  DevBuf<unsigned char> d_xin;       // ExtRes[] (pinned host / device, ext_stage_layout)
  // views into h_xin / d_xin (ext_stage_reserve): the sections of the staged block
  ExtPod* h_xpod = nullptr;
  ExtPod* d_xpod = nullptr;
  PodVec* d_xpv = nullptr;
  ExtRec* d_xrec = nullptr;
  ExtRes* d_xres = nullptr;
  size_t xin_off_rec = 0, xin_off_res = 0, xin_bytes = 0;
  PinnedBuf<ExtOut> h_xout;
  PinnedBuf<int32_t> h_xnom;
  std::vector<ExtRec> xrec;
  std::vector<ExtRes> xres;
  std::vector<uint64_t> xres_uid;
  uint32_t xrec_cap = 0, xres_cap = 0;
  bool ext_configured = false;       // gs_ext_configure was called (gs_preempt_dry_run refuses such a context)
  std::unique_ptr<PreemptState> pre; // gs_node_pods_* / gs_preempt_dry_run (none until the first such call)
};

int quiesce(gs_ctx* c);   // the async submissions' worker is idle (gs_schedule_submit)

namespace {
// The slot whose batch is current. Between runs no batch is in flight: gs_evaluate and the extension path borrow its
// buffers and events as scratch, whichever of the two slots the last run ended on.
Slot& current_slot(gs_ctx* c) { return c->slot[c->cur_slot]; }

int64_t mono_ns() {
  return std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
// marks a host wait of the scheduling path (the watchdog names it when it lasts)
struct Where {
  gs_ctx* c;
  const char* prev;
  int64_t prev_t;
  Where(gs_ctx* cc, const char* site) : c(cc), prev(cc->where.load()), prev_t(cc->where_t.load()) {
    c->where_t.store(mono_ns());
    c->where.store(site);
  }
  ~Where() {
    c->where.store(prev);
    c->where_t.store(prev_t);
  }
};
// Host waits of the scheduling path: poll the event / stream (spin, then yield, then short sleeps) instead of HIP's
// blocking synchronisation. Several processes sharing one GPU (the C4 rehearsal) showed a rank parked for 10-100 s
// inside hipStreamSynchronize / hipEventSynchronize while every stream and event of that rank had long completed (the
// watchdog's queries), i.e. a lost wake-up of the blocking wait. A poll sees the completion at once;
// bounded: past GS_WAIT_LIMIT_S (default 600 s) the call fails with GS_EDEVICE naming the wait.
template <class Query>
hipError_t poll_until(Query&& query, double limit_s) {
  const auto t0 = std::chrono::steady_clock::now();
  for (uint64_t it = 0;; ++it) {
    const hipError_t e = query();
    if (e != hipErrorNotReady) return e;
    if (it < 2000) {
      __builtin_ia32_pause();
    } else if (it < 20000) {
      std::this_thread::yield();
    } else {
      std::this_thread::sleep_for(std::chrono::microseconds(20));
      if ((it & 1023) == 0 &&
          std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > limit_s)
        return hipErrorLaunchTimeOut;   // (the wait exceeded its bound: reported as GS_EDEVICE)
    }
  }
}
double wait_limit_s() {
  static const double lim = env_num("GS_WAIT_LIMIT_S", 600.0);
  return lim > 0 ? lim : 600.0;
}
hipError_t host_wait_event(hipEvent_t ev) {
  return poll_until([&] { return hipEventQuery(ev); }, wait_limit_s());
}
hipError_t host_wait_stream(hipStream_t st) {
  return poll_until([&] { return hipStreamQuery(st); }, wait_limit_s());
}

void watchdog_loop(gs_ctx* c, double limit_s) {
  (void)hipSetDevice(c->cfg.device);
  const char* reported = nullptr;
  int64_t reported_t = 0;
  while (!c->wd_stop.load()) {
    std::this_thread::sleep_for(std::chrono::milliseconds(250));
    const char* w = c->where.load();
    const int64_t t = c->where_t.load();
    if (!w || (w == reported && t == reported_t)) continue;
    const double s = (mono_ns() - t) * 1e-9;
    if (s < limit_s) continue;
    // which device work is still pending: the streams, and per batch slot its eval-pass end (evdone), commit end
    // (ev[4]) and readback end (ev[5]) (0 = complete, 1 = pending)
    auto q = [](hipError_t e) { return e == hipSuccess ? 0 : e == hipErrorNotReady ? 1 : 9; };
    auto qe = [&](const Event& ev) { return q(hipEventQuery(ev.get())); };
    const Slot &s0 = c->slot[0], &s1 = c->slot[1];
    fprintf(stderr, "gpuscore watchdog: rank %d of %d blocked %.1f s in %s (batch pass %llu, exchange %llu); pending: "
            "st %d st_ev %d st2 %d st_rb %d | slot 0 evdone %d ev4 %d ev5 %d | slot 1 evdone %d ev4 %d ev5 %d (bound %d)\n",
            c->rank, c->nranks, s, w, (unsigned long long)c->xbatch, (unsigned long long)c->xseq, q(hipStreamQuery(c->st.get())),
            q(hipStreamQuery(c->st_ev.get())), q(hipStreamQuery(c->st2.get())), q(hipStreamQuery(c->st_rb.get())), qe(s0.ev_evdone),
            qe(s0.ev[4]), qe(s0.ev[5]), qe(s1.ev_evdone), qe(s1.ev[4]), qe(s1.ev[5]), c->cur_slot);
    fflush(stderr);
    reported = w;
    reported_t = t;
  }
}
}  // namespace
void async_stop(gs_ctx* c);

namespace {

int fail(gs_ctx* c, int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  if (c) c->err = buf;
  return code;
}

#define HIP_TRY(c, expr)                                                                    \
  do {                                                                                      \
    hipError_t _e = (expr);                                                                 \
    if (_e != hipSuccess) return fail((c), GS_EDEVICE, "%s: %s", #expr, hipGetErrorString(_e)); \
  } while (0)

// diagnostics (gs_debug_commit_counters): which pipeline of commit_spec_kernel a launch takes (launch_commit_spec)
inline void count_spec_launch(gs_ctx* c, const CommitArgs& a) {
  if (a.window_k) return;
  if (a.nranks <= 1 && a.npods >= 32) ++c->spec_split_launches;
  else ++c->spec_single_launches;
}

// ---- DefaultEstimator (loadaware/estimator/default_estimator.go:57-108) ------------------------
int translate(int32_t prio, int r) {   // extension.TranslateResourceNameByPriorityClass
  if (prio == GS_PRIO_PROD || prio == GS_PRIO_NONE) return r;
  if (prio == GS_PRIO_BATCH) return r == 0 ? GS_RES_BATCH_CPU : GS_RES_BATCH_MEMORY;
  if (prio == GS_PRIO_MID) return r == 0 ? GS_RES_MID_CPU : GS_RES_MID_MEMORY;
  return -1;
}

int64_t estimate_resource(const gs_pod& p, int real, int64_t sf) {
  int64_t lim = real >= 0 ? p.limits[real] : 0, req = real >= 0 ? p.requests[real] : 0;
  int64_t q = req;
  if (lim > req) { sf = 100; q = lim; }
  if (q == 0) {
    if (real == GS_RES_CPU || real == GS_RES_BATCH_CPU) return kDefaultMilliCPURequest;
    if (real == GS_RES_MEMORY || real == GS_RES_BATCH_MEMORY) return kDefaultMemoryRequest;
    return 0;
  }
  int64_t e = (int64_t)std::round((double)q * (double)sf / 100);
  if (lim > 0 && e > lim) e = lim;
  return e;
}

Vec2 estimate_pod(const gs_loadaware_args& a, const gs_pod& p) {
  Vec2 o;
  for (int r = 0; r < 2; ++r) {
    if (!(a.resource_weights_mask & (1u << r))) continue;
    int64_t sf = (a.estimated_scaling_factors_mask & (1u << r)) ? a.estimated_scaling_factors[r] : 0;
    o.add(r, estimate_resource(p, translate(p.priority_class, r), sf));
  }
  return o;
}

int64_t estimate_node(const gs_node& n, int r) {   // EstimateNode (default_estimator.go:110-129)
  return (n.raw_allocatable_mask & (1u << r)) ? n.raw_allocatable[r] : n.allocatable[r];
}

// ---- LoadAware node-side derivations (loadaware/load_aware.go, helper.go) -----------------------
bool target_agg(const gs_node_metric& m, int64_t dur, int32_t type, Vec2* out) {   // helper.go:58-90
  if (!m.has_node_metric || m.n_aggregated <= 0 || type < 0 || type >= GS_NUM_AGG_TYPES) return false;
  int n = std::min(m.n_aggregated, GS_MAX_AGG_USAGES);
  if (dur == 0) {
    int64_t maxd = 0;
    int mi = 0;
    for (int i = 0; i < n; ++i)
      if (m.aggregated[i].duration_ns > maxd) { maxd = m.aggregated[i].duration_ns; mi = i; }
    if (m.aggregated[mi].type_mask & (1u << type)) {
      Vec2 u = usage_of(m.aggregated[mi].usage[type]);
      if (u.mask) { *out = u; return true; }
    }
    return false;
  }
  for (int i = 0; i < n; ++i) {
    if (m.aggregated[i].duration_ns != dur || !(m.aggregated[i].type_mask & (1u << type))) continue;
    Vec2 u = usage_of(m.aggregated[i].usage[type]);
    if (u.mask) { *out = u; return true; }
  }
  return false;
}

struct Thr {
  int64_t v[2] = {0, 0};
  uint32_t mask = 0;
};

// 0: within the thresholds; else 1 + the first exceeding resource in the order cpu, memory
int usage_exceeds(const Thr& th, const Vec2& used, const gs_node& n) {
  for (int r = 0; r < 2; ++r) {
    if (!(th.mask & (1u << r)) || th.v[r] == 0) continue;
    int64_t total = estimate_node(n, r);
    if (total == 0) continue;
    int64_t u = used.get(r);
    double mu = (double)(r == 0 ? u : u * 1000), mt = (double)(r == 0 ? total : total * 1000);
    int64_t pct = (int64_t)std::round(mu / mt * 100);   // load_aware.go:214,248
    if (pct >= th.v[r]) return 1 + r;
  }
  return 0;
}

struct LaDerived {
  uint32_t sflags = 0;
  int64_t used_np[2] = {0, 0};
  int64_t used_p[2] = {0, 0};
};

LaDerived derive_loadaware(const gs_loadaware_args& a, const HostNode& hn) {
  LaDerived d;
  const gs_node& n = hn.node;
  const gs_node_metric& m = hn.metric;
  // Score-side usage is derived even without a NodeMetric (Score then returns 0 anyway): the value is
  // what the row must hold once a metric appears, and what device-side Reserve deltas accumulate into.
  if (m.exists) d.sflags |= SF_METRIC;
  if (m.exists && m.has_update_time) d.sflags |= SF_UPDATE_TIME;
  // ---- Filter profile (helper.go:102-140)
  Thr usage{{a.usage_thresholds[0], a.usage_thresholds[1]}, a.usage_thresholds_mask};
  Thr prod{{a.prod_usage_thresholds[0], a.prod_usage_thresholds[1]}, a.prod_usage_thresholds_mask};
  bool has_agg = false;
  Thr agg;
  int32_t agg_type = GS_AGG_NONE;
  int64_t agg_dur = 0;
  if (n.custom_flags & GS_NODE_CUSTOM_THRESHOLDS) {
    if (n.custom_usage_mask) usage = Thr{{n.custom_usage_thresholds[0], n.custom_usage_thresholds[1]}, n.custom_usage_mask};
    if (n.custom_prod_usage_mask)
      prod = Thr{{n.custom_prod_usage_thresholds[0], n.custom_prod_usage_thresholds[1]}, n.custom_prod_usage_mask};
    if ((n.custom_flags & GS_NODE_CUSTOM_AGGREGATED) && n.custom_agg_usage_mask && n.custom_agg_type != GS_AGG_NONE) {
      has_agg = true;
      agg = Thr{{n.custom_agg_usage_thresholds[0], n.custom_agg_usage_thresholds[1]}, n.custom_agg_usage_mask};
      agg_type = n.custom_agg_type;
      agg_dur = n.custom_agg_duration_ns;
    }
  }
  if (!has_agg && a.has_aggregated && a.agg_usage_thresholds_mask && a.agg_usage_type != GS_AGG_NONE) {
    has_agg = true;
    agg = Thr{{a.agg_usage_thresholds[0], a.agg_usage_thresholds[1]}, a.agg_usage_thresholds_mask};
    agg_type = a.agg_usage_type;
    agg_dur = a.agg_usage_duration_ns;
  }
  // non-prod verdict: filterNodeUsage (load_aware.go:173-224)
  const Thr& th = has_agg ? agg : usage;
  if (m.exists && th.mask && m.has_node_metric) {
    Vec2 u;
    bool have = has_agg ? target_agg(m, agg_dur, agg_type, &u) : (u = usage_of(m.node_usage), true);
    const int ex = have ? usage_exceeds(th, u, n) : 0;
    if (ex) d.sflags |= SF_FAIL_NP | (ex == 2 ? SF_NP_MEM : 0u) | (has_agg ? SF_NP_AGG : 0u);
  }
  // prod verdict: filterProdUsage (load_aware.go:226-254)
  if (prod.mask) {
    d.sflags |= SF_PROD_THR;
    if (m.exists && !hn.pms.empty()) {
      std::unordered_map<uint64_t, Vec2> pm;
      for (const auto& e : hn.pms)
        if (e.in_lister && e.priority_class == GS_PRIO_PROD) pm[e.name_key] = usage_of(e.usage);
      Vec2 sum;
      for (const auto& kv : pm)
        for (int r = 0; r < 2; ++r)
          if (kv.second.has(r)) sum.add(r, kv.second.v[r]);
      const int ex = usage_exceeds(prod, sum, n);
      if (ex) d.sflags |= SF_FAIL_P | (ex == 2 ? SF_P_MEM : 0u);
    }
  }
  // ---- Score-side usage (load_aware.go:291-327, 337-376), for both prodPod modes
  int64_t update = m.has_update_time ? m.update_time_ns : kZeroTime;
  int64_t interval = m.has_report_interval ? m.report_interval_s * 1000000000LL : kDefaultReportIntervalNs;
  bool score_agg = a.has_aggregated && a.agg_score_type != GS_AGG_NONE;
  Vec2 score_usage;
  bool have_score_usage = false;
  if (score_agg) have_score_usage = target_agg(m, a.agg_score_duration_ns, a.agg_score_type, &score_usage);
  bool agg_missing = score_agg && !have_score_usage;
  for (int mode = 0; mode < 2; ++mode) {
    bool prod_mode = mode == 1;
    std::unordered_map<uint64_t, Vec2> pm;
    for (const auto& e : hn.pms) {
      if (!e.in_lister) continue;
      if (prod_mode && e.priority_class != GS_PRIO_PROD) continue;
      pm[e.name_key] = usage_of(e.usage);
    }
    Vec2 used;
    std::unordered_map<uint64_t, bool> estimated;
    for (const auto& kv : hn.assigned) {
      const Assigned& as = kv.second;
      if (prod_mode && as.pod.priority_class != GS_PRIO_PROD) continue;
      auto it = pm.find(as.pod.name_key);
      Vec2 pu;
      if (it != pm.end()) pu = it->second;
      bool est_it = pu.mask == 0 || as.ts > update || (as.ts < update && update - as.ts < interval) || agg_missing;
      if (!est_it) continue;
      Vec2 e = estimate_pod(a, as.pod);
      for (int r = 0; r < 2; ++r) {
        if (!e.has(r)) continue;
        int64_t v = e.v[r];
        if (pu.has(r) && pu.v[r] > v) v = pu.v[r];
        used.add(r, v);
      }
      estimated[as.pod.name_key] = true;
    }
    Vec2 actual, est_actual;
    for (const auto& kv : pm) {
      Vec2& dst = estimated.count(kv.first) ? est_actual : actual;
      for (int r = 0; r < 2; ++r)
        if (kv.second.has(r)) dst.add(r, kv.second.v[r]);
    }
    if (prod_mode) {
      for (int r = 0; r < 2; ++r) used.add(r, actual.get(r));
    } else if (m.has_node_metric) {
      Vec2 nu;
      bool have = score_agg ? have_score_usage : true;
      if (score_agg) nu = score_usage;
      else nu = usage_of(m.node_usage);
      if (have) {
        for (int r = 0; r < 2; ++r) {
          if (!nu.has(r)) continue;
          int64_t q = nu.v[r], e = est_actual.get(r);
          if (e != 0 && q >= e) q -= e;
          used.add(r, q);
        }
      }
    }
    int64_t* dst = prod_mode ? d.used_p : d.used_np;
    dst[0] = used.get(0);
    dst[1] = used.get(1);
  }
  return d;
}

gs_node reservation_view(const gs_ctx* c, uint32_t i, uint64_t owner);

void derive_row(const gs_ctx* c, uint32_t i, int64_t* row) {
  const HostNode& hn = c->nodes[i];
  // NodeInfo as a pod that matches none of the node's reservations sees it (reservation/transformer.go:266-292)
  const gs_node n = reservation_view(c, i, 0);
  for (int s = 0; s < 7; ++s) {
    row[C_FREE_CPU + s] = n.allocatable[s] - n.requested[s];
    row[C_ALLOC_CPU + s] = n.allocatable[s];
  }
  row[C_NZFREE_CPU] = n.allocatable[0] - n.nonzero_requested[0];
  row[C_NZFREE_MEM] = n.allocatable[1] - n.nonzero_requested[1];
  LaDerived d = derive_loadaware(c->cfg.loadaware, hn);
  for (int r = 0; r < 2; ++r) {
    int64_t cap = estimate_node(n, r);
    row[C_LA_CAP_CPU + r] = cap;
    row[C_LA_FREE_CPU + r] = cap - d.used_np[r];
    row[C_LA_PFREE_CPU + r] = cap - d.used_p[r];
  }
  row[C_UPDATE_TIME] = hn.metric.has_update_time ? hn.metric.update_time_ns : 0;
  int64_t fp = n.allowed_pod_number - n.pod_count;
  fp = std::max<int64_t>(INT32_MIN, std::min<int64_t>(INT32_MAX, fp));
  row[NUM_I64_COLS + C_FREE_PODS] = fp;
  row[NUM_I64_COLS + C_SFLAGS] = (int64_t)(d.sflags | (hn.valid ? SF_VALID : 0));
  row[NUM_I64_COLS + C_DFLAGS] = 0;
}

// ---- Reservation restore (reservation/transformer.go:50-292) on the host mirror ----------------------------------
// A reservation enters a pod's NodeInfo in BeforePreFilter: available ones (IsAvailable, no parse error, not an
// allocate-once reservation already used) that the pod matches are removed with their reserve pod (RemovePod); the
// others with assigned pods are "unmatched" and trimmed to their remaining resources (updateNodeInfoRequested).
bool rsv_usable(const gs_reservation& r) { return r.available && !(r.allocate_once && r.assigned_pods > 0); }
bool rsv_matches(const gs_reservation& r, uint64_t owner) {
  return owner != 0 && !r.unschedulable && r.owner_key == owner && rsv_usable(r);
}

// one-container pod requests -> (Requested delta per slot, NonZeroRequested delta): [upstream] calculateResource with
// schedutil.GetNonzeroRequests (100m / 200Mi for an absent cpu / memory key)
void rsv_request_delta(const int64_t* v, uint32_t mask, int64_t sign, int64_t* req, int64_t* nz) {
  for (int s = 0; s < GS_NUM_RES; ++s)
    if (mask >> s & 1u) req[s] += sign * v[s];
  nz[0] += sign * ((mask & 1u) ? v[0] : 100);
  nz[1] += sign * ((mask & 2u) ? v[1] : 200LL * 1024 * 1024);
}
// SubtractWithNonNegativeResult(Allocatable, Allocated): values and keys
uint32_t rsv_remained(const gs_reservation& r, int64_t* rem) {
  const uint32_t keys = r.allocatable_mask | r.allocated_mask;
  for (int s = 0; s < GS_NUM_RES; ++s) {
    const int64_t a = (r.allocatable_mask >> s & 1u) ? r.allocatable[s] : 0;
    const int64_t u = (r.allocated_mask >> s & 1u) ? r.allocated[s] : 0;
    rem[s] = (keys >> s & 1u) ? std::max<int64_t>(0, a - u) : 0;
  }
  return keys;
}
bool all_zero(const int64_t* v) {
  for (int s = 0; s < GS_NUM_RES; ++s)
    if (v[s]) return false;
  return true;
}
// restoreUnmatchedReservations on a NodeInfo copy
void rsv_trim_unmatched(const gs_reservation& r, gs_node& n) {
  rsv_request_delta(r.allocatable, r.allocatable_mask, -1, n.requested, n.nonzero_requested);
  int64_t rem[GS_NUM_RES];
  const uint32_t keys = rsv_remained(r, rem);
  if (!all_zero(rem)) rsv_request_delta(rem, keys, +1, n.requested, n.nonzero_requested);
}

// NodeInfo of node i as a pod with owner key `owner` sees it after the unmatched trim (podRequested; the matched
// reservations are not removed here)
gs_node reservation_view(const gs_ctx* c, uint32_t i, uint64_t owner) {
  gs_node n = c->nodes[i].node;
  if (c->rsv_node.empty() || !(c->ext.enabled & GS_EXT_RESERVATION)) return n;
  for (uint64_t uid : c->rsv_node[i]) {
    const gs_reservation& r = c->rsv.at(uid);
    if (!rsv_usable(r) || rsv_matches(r, owner) || r.assigned_pods <= 0) continue;
    rsv_trim_unmatched(r, n);
  }
  return n;
}

void derive_row_numa(const gs_ctx* c, uint32_t i, int64_t* row) {
  numa_derive(c->numa[i], c->cfg.numa.numa_scoring_type == GS_SCORING_MOST_ALLOCATED, row, row + NUM_I64_COLS);
}

bool in_range(int64_t v) { return v > -kMaxExact && v < kMaxExact; }

int validate_node(gs_ctx* c, const gs_node& n) {
  for (int s = 0; s < GS_NUM_RES; ++s)
    if (!in_range(n.allocatable[s]) || !in_range(n.requested[s]) || n.allocatable[s] < 0)
      return fail(c, GS_EUNSUPPORTED, "node resource slot %d outside the exact range [0, 2^53)", s);
  if (!in_range(n.nonzero_requested[0]) || !in_range(n.nonzero_requested[1]) || !in_range(n.raw_allocatable[0]) ||
      !in_range(n.raw_allocatable[1]) || n.raw_allocatable[0] < 0 || n.raw_allocatable[1] < 0)
    return fail(c, GS_EUNSUPPORTED, "node quantity outside the exact range [0, 2^53)");
  // NodeInfo.Requested / NonZeroRequested are sums of pod requests: never negative. A negative one would put the
  // scored quantity above the capacity, outside the per-pair division's range (pct_floor: 0 <= x <= cap)
  for (int s = 0; s < GS_NUM_RES; ++s)
    if (n.requested[s] < 0) return fail(c, GS_EINVAL, "node requested of resource slot %d is negative", s);
  if (n.nonzero_requested[0] < 0 || n.nonzero_requested[1] < 0)
    return fail(c, GS_EINVAL, "node nonzero_requested is negative");
  if (n.allocatable[GS_RES_RESERVED] || n.requested[GS_RES_RESERVED])
    return fail(c, GS_EINVAL, "resource slot 7 is reserved");
  return GS_OK;
}

PodVec prep_pod(const gs_ctx* c, const gs_pod& p) {
  PodVec v{};
  for (int s = 0; s < 7; ++s) v.req[s] = p.requests[s];
  v.nz[0] = p.nonzero_requests[0];
  v.nz[1] = p.nonzero_requests[1];
  Vec2 e = estimate_pod(c->cfg.loadaware, p);
  v.est[0] = e.get(0);
  v.est[1] = e.get(1);
  uint32_t f = 0;
  if (p.flags & GS_POD_DAEMONSET) f |= PF_DAEMONSET;
  if (p.priority_class == GS_PRIO_PROD) {
    f |= PF_PROD;
    if (c->cfg.loadaware.score_according_prod_usage) f |= PF_PROD_SCORE;
  }
  uint32_t scalar = p.request_mask & GS_SCALAR_RES_MASK;
  if (p.requests[0] == 0 && p.requests[1] == 0 && p.requests[2] == 0 && scalar == 0) f |= PF_ALL_ZERO;
  v.flags = f;
  v.scalar_mask = scalar;
  // NodeNUMAResource PreFilter (nodenumaresource/plugin.go:219-269)
  uint32_t keys = p.request_mask & 0x7Fu;
  v.req_keys = keys;
  bool zero = true;
  for (int s = 0; s < 7; ++s)
    if ((keys >> s & 1) && p.requests[s] != 0) zero = false;
  uint32_t pn = 0;
  int64_t cpu = (keys & 1u) ? p.requests[GS_RES_CPU] : 0;
  v.num_cpus = (int32_t)(cpu / 1000);
  if (zero) {
    pn |= PN_SKIP;
  } else if ((p.qos_class == GS_QOS_LSE || p.qos_class == GS_QOS_LSR) && p.priority_class == GS_PRIO_PROD) {
    const int def = c->cfg.numa.default_cpu_bind_policy;
    int bind = p.preferred_cpu_bind_policy;
    if (bind == GS_CPU_BIND_UNSET || bind == GS_CPU_BIND_DEFAULT) bind = def;
    int required = p.required_cpu_bind_policy;
    if (required == GS_CPU_BIND_DEFAULT) required = def;
    if (required != GS_CPU_BIND_UNSET) bind = required;
    if (bind == GS_CPU_BIND_FULL_PCPUS || bind == GS_CPU_BIND_SPREAD_BY_PCPUS) {
      if (cpu % 1000 != 0) pn |= PN_PREFAIL;
      else if (cpu > 0)
        pn |= PN_BIND | ((uint32_t)required << PN_REQ_SHIFT) | ((uint32_t)bind << PN_PREF_SHIFT) |
              ((uint32_t)p.preferred_cpu_exclusive_policy << PN_EXCL_SHIFT);
    }
  }
  v.numa = pn;
  return v;
}

// a pod the device path takes (msg: why not); no context state written (gs_schedule_submit runs it beside the worker)
int validate_pod_msg(bool numa_on, const gs_pod& p, char* msg, size_t len) {
  for (int s = 0; s < GS_NUM_RES; ++s)
    if (!in_range(p.requests[s]) || p.requests[s] < 0 || !in_range(p.limits[s]) || p.limits[s] < 0) {
      snprintf(msg, len, "pod resource slot %d outside the exact range [0, 2^53)", s);
      return GS_EUNSUPPORTED;
    }
  for (int r = 0; r < 2; ++r)   // (the quantity Fit's score subtracts from the node's free non-zero request)
    if (!in_range(p.nonzero_requests[r]) || p.nonzero_requests[r] < 0) {
      snprintf(msg, len, "pod nonzero_requests[%d] outside the exact range [0, 2^53)", r);
      return GS_EUNSUPPORTED;
    }
  if (p.requests[GS_RES_RESERVED] || (p.request_mask & 0x80u)) {
    snprintf(msg, len, "resource slot 7 is reserved");
    return GS_EINVAL;
  }
  if (numa_on) {
    for (int s = 2; s < 7; ++s)
      if ((p.request_mask >> s & 1) && p.requests[s] == 0) {
        snprintf(msg, len, "NodeNUMAResource: a zero-valued request key other than cpu/memory (slot %d) is not "
                 "supported on the device path", s);
        return GS_EUNSUPPORTED;
      }
    if (p.required_cpu_bind_policy < 0 || p.required_cpu_bind_policy > 4 || p.preferred_cpu_bind_policy < 0 ||
        p.preferred_cpu_bind_policy > 4 || p.preferred_cpu_exclusive_policy < 0 || p.preferred_cpu_exclusive_policy > 2) {
      snprintf(msg, len, "pod cpu bind / exclusive policy out of range");
      return GS_EINVAL;
    }
  }
  return GS_OK;
}

int validate_pod(gs_ctx* c, const gs_pod& p) {
  char msg[256];
  const int rc = validate_pod_msg(c->numa_on, p, msg, sizeof msg);
  return rc ? fail(c, rc, "%s", msg) : GS_OK;
}

void mark_dirty(gs_ctx* c, uint32_t i) {
  if (!c->row_dirty[i]) {
    c->row_dirty[i] = 1;
    c->dirty_list.push_back(i);
  }
}

int flush_rows(gs_ctx* c) {
  if (c->dirty_list.empty()) return GS_OK;
  size_t done = 0;
  while (done < c->dirty_list.size()) {
    uint32_t n = (uint32_t)std::min<size_t>(c->stage_cap, c->dirty_list.size() - done);
    // staging buffers are reused: the previous scatter must have consumed them
    Where w_(c, "flush_rows: previous scatter");
    HIP_TRY(c, host_wait_stream(c->st.get()));
    // one staged block, one copy: the n rows, then their node indices
    uint32_t* h_idx = reinterpret_cast<uint32_t*>(c->h_stage_rows.get() + (size_t)n * ROW_WORDS);
    for (uint32_t j = 0; j < n; ++j) {
      uint32_t i = c->dirty_list[done + j];
      h_idx[j] = i;
      derive_row(c, i, c->h_stage_rows.get() + (size_t)j * ROW_WORDS);
      derive_row_numa(c, i, c->h_stage_rows.get() + (size_t)j * ROW_WORDS);
      c->row_dirty[i] = 0;
    }
    HIP_TRY(c, hipMemcpyAsync(c->d_stage_rows.get(), c->h_stage_rows.get(), (size_t)n * (ROW_WORDS * 8 + 4), hipMemcpyHostToDevice,
                              c->st.get()));
    const uint32_t* d_idx = reinterpret_cast<const uint32_t*>(c->d_stage_rows.get() + (size_t)n * ROW_WORDS);
    // with the rows' LoadAware verdicts at `now` (node_prep, fused into the scatter), unless a full pass is due anyway
    if (!c->prep_stale && c->prep_now == c->now) {
      const gs_loadaware_args& la = c->cfg.loadaware;
      const ScatterPrep sp{c->now, la.filter_expired_node_metrics, la.has_node_metric_expiration,
                           la.has_node_metric_expiration ? la.node_metric_expiration_seconds * 1000000000LL : 0};
      HIP_TRY(c, launch_scatter_rows(c->mv, d_idx, c->d_stage_rows.get(), n, c->st.get(), &sp));
    } else {
      HIP_TRY(c, launch_scatter_rows(c->mv, d_idx, c->d_stage_rows.get(), n, c->st.get()));
    }

    c->stats.delta_rows += n;
    c->stats.delta_bytes += (uint64_t)n * (4 + ROW_WORDS * 8);
    done += n;
  }
  c->dirty_list.clear();
  if (c->prep_now != c->now) c->prep_stale = true;
  return GS_OK;
}

int node_prep(gs_ctx* c) {
  const gs_loadaware_args& a = c->cfg.loadaware;
  int64_t exp_ns = a.has_node_metric_expiration ? a.node_metric_expiration_seconds * 1000000000LL : 0;
  HIP_TRY(c, launch_node_prep(c->mv, 0, c->N, c->now, a.filter_expired_node_metrics, a.has_node_metric_expiration,
                              exp_ns, c->st.get()));
  c->prep_stale = false;
  c->prep_now = c->now;
  return GS_OK;
}

// every node upserted at least once (nodes never become invalid again: a count, not a scan of the N host rows — at
// 100k nodes the scan cost ~0.1 ms per gs_schedule call, i.e. per short plain run on the C5 extension path)
int ready(gs_ctx* c) {
  if (c->n_valid == c->N) return GS_OK;
  for (uint32_t i = 0; i < c->N; ++i)
    if (!c->nodes[i].valid) return fail(c, GS_ESTATE, "node %u was never upserted", i);
  return GS_OK;
}

double ev_ms(hipEvent_t a, hipEvent_t b) {
  float ms = 0;
  if (hipEventElapsedTime(&ms, a, b) != hipSuccess) {
    (void)hipGetLastError();   // (an event without timing: not sticky for the next launch's check)
    return 0;
  }
  return ms;
}

// exchange_ms of RCCL all-gathers: completion time from events around each collective on the stream, added up once
// a collective's end event has completed (finish_batch); the pairs of a speculative batch still in flight stay pending
void flush_exchange_times(gs_ctx* c) {
  int keep = 0;
  for (int i = 0; i < c->x_pending; ++i) {
    hipEvent_t a = c->x_ev[2 * i].get(), b = c->x_ev[2 * i + 1].get();
    if (hipEventQuery(b) == hipSuccess) {
      c->stats.exchange_ms += ev_ms(a, b);
    } else {   // still in flight: keep the pair (moved to the front)
      std::swap(c->x_ev[2 * keep], c->x_ev[2 * i]);
      std::swap(c->x_ev[2 * keep + 1], c->x_ev[2 * i + 1]);
      ++keep;
    }
  }
  c->x_pending = keep;
}

constexpr size_t XSMALL = 64;   // small exchange block: payload <= 32 B, XTag at 32

const char* xsite_name(uint32_t s) {
  return s == XSITE_LEVELS ? "levels" : s == XSITE_ROWSTAT ? "row stats" : s == XSITE_SELECT ? "selection"
       : s == XSITE_SCORES ? "score rows" : s == XSITE_RUNS ? "run boundary" : "?";
}

// The R received blocks' tags against the tag this rank sent: every rank checks all of them, so a divergence fails
// on every rank at the same exchange.
int check_tags(gs_ctx* c, const uint8_t* blocks, size_t bytes, const XTag& mine) {
  for (int r = 0; r < c->nranks; ++r) {
    XTag t;
    std::memcpy(&t, blocks + (size_t)r * bytes + bytes - sizeof(XTag), sizeof t);
    if (t.magic != XTAG_MAGIC || t.site != mine.site || t.seq != mine.seq || t.batch != mine.batch || t.rank != r ||
        t.bytes != mine.bytes)
      return fail(c, GS_ECOMM,
                  "exchange sequence diverged: rank %d is at exchange %llu (%s, batch %llu), rank %d sent exchange %llu "
                  "(%s, batch %llu, %u bytes, magic %#x)",
                  c->rank, (unsigned long long)mine.seq, xsite_name(mine.site), (unsigned long long)mine.batch, r,
                  (unsigned long long)t.seq, xsite_name(t.site), (unsigned long long)t.batch, t.bytes, t.magic);
  }
  return GS_OK;
}

// the start / end event pair of the next device-side exchange (x_ev[2 * x_pending], + 1), created on first use
int reserve_exchange_events(gs_ctx* c) {
  while (c->x_pending * 2 + 2 > (int)c->x_ev.size()) {
    Event ev;
    HIP_TRY(c, ev.create());
    c->x_ev.push_back(std::move(ev));
  }
  return GS_OK;
}

// One all-gather of `bytes`-byte blocks (each ending in an XTag, filled here) from d_send into R blocks at d_recv.
// RCCL: stream-ordered, the tag written on the stream before the collective; the receiver checks the tags (the level
// blocks on the device in merge_levels_kernel, the small ones on the host). Callback: host-synchronous, checked here.
int exchange(gs_ctx* c, uint32_t site, uint8_t* d_send, uint8_t* d_recv, size_t bytes, XTag* sent = nullptr,
             hipStream_t xs = nullptr) {
  auto t0 = std::chrono::steady_clock::now();
  if (!xs) xs = c->st.get();
  // the host-callback transport's staging: the score blocks have their own buffers
  uint8_t* h_send = site == XSITE_SCORES ? c->h_sx_send.get() : c->h_xchg_send.get();
  uint8_t* h_recv = site == XSITE_SCORES ? c->h_sx_recv.get() : c->h_xchg_recv.get();
  const size_t h_cap = site == XSITE_SCORES ? c->sx_bytes : c->xchg_bytes;
  if (bytes < sizeof(XTag) || bytes % 8) return fail(c, GS_EINVAL, "exchange block of %zu bytes", bytes);
  XTag tag{XTAG_MAGIC, site, ++c->xseq, c->xbatch, c->rank, (uint32_t)bytes};
  if (c->rank == c->dbg_xskew_rank && c->xbatch == c->dbg_xskew_batch && (site == XSITE_LEVELS || site == XSITE_SCORES))
    tag.seq = ++c->xseq;
  if (sent) *sent = tag;
  if (c->comm) {
    HIP_TRY(c, launch_write_tag(d_send + bytes - sizeof(XTag), tag, xs));
    if (int rc = reserve_exchange_events(c)) return rc;
    HIP_TRY(c, hipEventRecord(c->x_ev[2 * c->x_pending].get(), xs));
    ncclResult_t r = ncclAllGather(d_send, d_recv, bytes, ncclUint8, c->comm, xs);
    if (r != ncclSuccess) return fail(c, GS_ECOMM, "ncclAllGather: %s", ncclGetErrorString(r));
    HIP_TRY(c, hipEventRecord(c->x_ev[2 * c->x_pending + 1].get(), xs));
    ++c->x_pending;
    return GS_OK;
  } else if (c->lg) {
    gs_local_group& g = *c->lg;
    static const double limit = env_num("GS_LOCAL_WAIT_S", 60.0);
    HIP_TRY(c, launch_write_tag(d_send + bytes - sizeof(XTag), tag, xs));
    if (int rc = reserve_exchange_events(c)) return rc;
    HIP_TRY(c, hipEventRecord(c->x_ev[2 * c->x_pending].get(), xs));
    HIP_TRY(c, hipEventRecord(c->lg_ready.get(), xs));
    {
      std::lock_guard<std::mutex> lk(g.mu);
      g.send[c->rank] = d_send;
      g.bytes[c->rank] = bytes;
      g.ready[c->rank] = c->lg_ready.get();
    }
    bool met;
    {
      Where w_(c, "exchange (local transport): the ranks' send blocks");
      met = g.meet(limit);
    }
    if (!met)
      return fail(c, GS_ECOMM, "local transport: a rank did not reach exchange %llu (%s, batch %llu) within %.0f s",
                  (unsigned long long)tag.seq, xsite_name(site), (unsigned long long)tag.batch, limit);
    bool same = true;
    for (int s = 0; s < c->nranks; ++s) same = same && g.bytes[s] == bytes;
    if (same)
      for (int s = 0; s < c->nranks; ++s) {
        HIP_TRY(c, hipStreamWaitEvent(xs, g.ready[s], 0));
        HIP_TRY(c, hipMemcpyAsync(d_recv + (size_t)s * bytes, g.send[s], bytes, hipMemcpyDeviceToDevice, xs));
      }
    HIP_TRY(c, hipEventRecord(c->lg_done.get(), xs));
    {
      std::lock_guard<std::mutex> lk(g.mu);
      g.done[c->rank] = c->lg_done.get();
    }
    {
      Where w_(c, "exchange (local transport): the ranks' copies");
      met = g.meet(limit);
    }
    if (!met)
      return fail(c, GS_ECOMM, "local transport: a rank did not finish exchange %llu (%s, batch %llu) within %.0f s",
                  (unsigned long long)tag.seq, xsite_name(site), (unsigned long long)tag.batch, limit);
    if (!same) return fail(c, GS_ECOMM, "local transport: the ranks' blocks of exchange %llu differ in size",
                           (unsigned long long)tag.seq);
    for (int s = 0; s < c->nranks; ++s)
      if (s != c->rank) HIP_TRY(c, hipStreamWaitEvent(xs, g.done[s], 0));
    HIP_TRY(c, hipEventRecord(c->x_ev[2 * c->x_pending + 1].get(), xs));
    ++c->x_pending;
    return GS_OK;
  } else if (c->cb) {
    if (bytes > h_cap || !h_send) return fail(c, GS_EINVAL, "exchange payload too large");
    Where w_(c, site == XSITE_LEVELS   ? "exchange (levels): stream before the callback"
                : site == XSITE_SCORES ? "exchange (score rows): stream before the callback"
                                       : "exchange (small): stream before the callback");
    HIP_TRY(c, hipMemcpyAsync(h_send, d_send, bytes - sizeof(XTag), hipMemcpyDeviceToHost, xs));
    HIP_TRY(c, host_wait_stream(xs));
    c->where.store("exchange: allgather callback");
    std::memcpy(h_send + bytes - sizeof(XTag), &tag, sizeof tag);
    if (c->cb(c->cb_user, h_send, h_recv, bytes) != 0) return fail(c, GS_ECOMM, "allgather callback failed");
    if (int rc = check_tags(c, h_recv, bytes, tag)) return rc;
    HIP_TRY(c, hipMemcpyAsync(d_recv, h_recv, bytes * c->nranks, hipMemcpyHostToDevice, xs));
  } else {
    return fail(c, GS_ESTATE, "multi-rank context without a communicator");
  }
  c->stats.exchange_ms +=
      std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return GS_OK;
}

// A small exchange (payload <= 32 B at d_payload, device) and its R payloads read back to host_out (R x payload bytes).
// xs: the stream (default st); a host payload (d_payload == nullptr) is taken from host_in.
int exchange_small(gs_ctx* c, uint32_t site, const void* d_payload, size_t payload, void* host_out,
                   hipStream_t xs = nullptr, const void* host_in = nullptr) {
  static_assert(XSMALL >= 32 + sizeof(XTag), "small exchange block");
  if (payload > XSMALL - sizeof(XTag)) return fail(c, GS_EINVAL, "small exchange payload too large");
  if (!xs) xs = c->st.get();
  if (d_payload) {
    HIP_TRY(c, hipMemcpyAsync(c->d_xsmall.get(), d_payload, payload, hipMemcpyDeviceToDevice, xs));
  } else {   // (h_xsmall is free between small exchanges: staged through it, in stream order)
    std::memcpy(c->h_xsmall.get(), host_in, payload);
    HIP_TRY(c, hipMemcpyAsync(c->d_xsmall.get(), c->h_xsmall.get(), payload, hipMemcpyHostToDevice, xs));
  }
  XTag tag{};
  if (int rc = exchange(c, site, c->d_xsmall.get(), c->d_xsmall.get() + XSMALL, XSMALL, &tag, xs)) return rc;
  HIP_TRY(c, hipMemcpyAsync(c->h_xsmall.get(), c->d_xsmall.get() + XSMALL, XSMALL * c->nranks, hipMemcpyDeviceToHost, xs));
  Where w_(c, "exchange_small: read back");
  HIP_TRY(c, host_wait_stream(xs));
  if (int rc = check_tags(c, c->h_xsmall.get(), XSMALL, tag)) return rc;
  for (int r = 0; r < c->nranks; ++r)
    std::memcpy(static_cast<uint8_t*>(host_out) + (size_t)r * payload, c->h_xsmall.get() + (size_t)r * XSMALL, payload);
  return GS_OK;
}

bool special_pod(const gs_ctx* c, const gs_pod& p) {
  // Placements whose LoadAware effect is not "+EstimatePod" on the chosen row: the pod UID already sits
  // in an assign cache, a PodMetric with the pod's name exists, or the pod is terminated (assign skips it).
  if (p.flags & GS_POD_TERMINATED) return true;
  if (c->uid_node.count(p.uid)) return true;
  if (c->metric_names.count(p.name_key)) return true;
  if (c->numa_on && c->numa_uid_node.count(p.uid)) return true;   // Update() would release its old allocation
  return false;
}

// NodeNUMAResource Reserve (nodenumaresource/plugin.go:375-422) replayed on the host mirror: NUMA resources
// along the device-chosen affinity (already applied to HBM by the commit kernel), and for cpuset pods the
// cpuset selection itself (resourceManager.Allocate -> allocateCPUSet -> takeCPUs).
int numa_reserve(gs_ctx* c, const gs_pod& p, const PodVec& v, const PlacementDev& pd) {
  if (!c->numa_on || pd.node < 0) return GS_OK;
  if (v.numa & (PN_SKIP | PN_PREFAIL)) return GS_OK;
  NumaNode& nn = c->numa[pd.node];
  const bool rb = pd.flags & GS_PLACED_CPUSET;
  if (!rb && nn.cfg.numa_topology_policy == GS_NUMA_POLICY_NONE) return GS_OK;
  PodAllocRec rec;
  rec.uid = p.uid;
  rec.excl = (v.numa & PN_BIND) ? p.preferred_cpu_exclusive_policy : GS_CPU_EXCLUSIVE_NONE;
  for (int z = 0; z < GS_MAX_NUMA; ++z) {
    if (!(pd.zkeys >> z & 1) && !(pd.zkeys >> (4 + z) & 1)) continue;
    gs_numa_zone a{};
    a.node_id = nn.cfg.zones[z].node_id;
    if (pd.zkeys >> z & 1) { a.mask |= GS_USAGE_CPU; a.cpu_milli = pd.zcpu[z]; }
    if (pd.zkeys >> (4 + z) & 1) { a.mask |= GS_USAGE_MEMORY; a.memory = pd.zmem[z]; }
    rec.numa.push_back(a);
  }
  if (pd.flags & PL_RESERVE_FAILED)
    return fail(c, GS_ESTATE, "NodeNUMAResource Reserve failed on the device for node %d after a feasible Filter",
                pd.node);
  const bool on_device = pd.flags & PL_DEVICE_CPUSET;   // the commit kernel chose the cpuset and updated the row
  if (rb && (!on_device || c->verify_cpuset)) {
    // getCPUBindPolicy (util.go:85-103) and GetNUMAAllocateStrategy (util.go:35-41)
    int req = (v.numa >> PN_REQ_SHIFT) & 7, pref = (v.numa >> PN_PREF_SHIFT) & 7;
    int bind = pref;
    bool required = false;
    if (req != GS_CPU_BIND_UNSET) { bind = req; required = true; }
    else if (nn.cfg.node_cpu_bind_policy == GS_NODE_CPU_BIND_SPREAD_BY_PCPUS) { bind = GS_CPU_BIND_SPREAD_BY_PCPUS; required = true; }
    else if (nn.cfg.node_cpu_bind_policy == GS_NODE_CPU_BIND_FULL_PCPUS_ONLY) { bind = GS_CPU_BIND_FULL_PCPUS; required = true; }
    int strategy = nn.cfg.numa_allocate_strategy;
    if (strategy == GS_NUMA_ALLOC_UNSET)
      strategy = c->cfg.numa.numa_scoring_type == GS_SCORING_MOST_ALLOCATED ? GS_NUMA_ALLOC_MOST_ALLOCATED
                                                                          : GS_NUMA_ALLOC_LEAST_ALLOCATED;
    if (!numa_allocate_cpuset(nn, v.num_cpus, bind, required, rec.excl, strategy, rec.numa, &rec.cpus))
      return fail(c, GS_ESTATE, "NodeNUMAResource Reserve: cpuset allocation failed on node %d after a feasible Filter",
                  pd.node);
    if (on_device && std::memcmp(rec.cpus.w, pd.cpuset, sizeof(pd.cpuset)) != 0)
      return fail(c, GS_ESTATE, "NodeNUMAResource Reserve: device cpuset differs from the host takeCPUs on node %d",
                  pd.node);
  }
  if (on_device)
    for (int w = 0; w < GS_CPU_WORDS; ++w) rec.cpus.w[w] = pd.cpuset[w];
  if (!nn.topo_valid()) return GS_OK;   // resourceManager.Update skips nodes without a valid CPU topology
  numa_release(nn, rec.uid);
  numa_add(nn, rec);
  c->numa_uid_node[rec.uid] = (uint32_t)pd.node;
  if (rb && !on_device) mark_dirty(c, (uint32_t)pd.node);
  return GS_OK;
}

void apply_placement(gs_ctx* c, const gs_pod& p, int32_t node, bool special) {
  if (node < 0) return;
  HostNode& hn = c->nodes[node];
  for (int s = 0; s < GS_NUM_RES; ++s) hn.node.requested[s] += p.requests[s];
  hn.node.nonzero_requested[0] += p.nonzero_requests[0];
  hn.node.nonzero_requested[1] += p.nonzero_requests[1];
  hn.node.pod_count += 1;
  if (!(p.flags & GS_POD_TERMINATED)) {
    hn.assigned[p.uid] = Assigned{c->now, p};
    c->uid_node[p.uid] = (uint32_t)node;
  }
  if (special) mark_dirty(c, (uint32_t)node);
}

void index_metric_names(gs_ctx* c, const HostNode& hn, int delta) {
  for (const auto& e : hn.pms) {
    auto it = c->metric_names.find(e.name_key);
    if (delta > 0) {
      c->metric_names[e.name_key] += 1;
    } else if (it != c->metric_names.end()) {
      if (--it->second <= 0) c->metric_names.erase(it);
    }
  }
}

int compute_profile(gs_ctx* c) {
  const gs_config& cfg = c->cfg;
  Profile& pf = c->pf;
  pf = Profile{};
  pf.enabled = cfg.enabled & 0x3Fu;
  c->numa_on = (pf.enabled & (GS_ENABLE_NUMA_FILTER | GS_ENABLE_NUMA_SCORE)) != 0;
  pf.w_numa = (int32_t)cfg.plugin_weights[GS_PLUGIN_NUMA];
  for (int s = 0; s < 7; ++s) {
    int64_t w = cfg.numa.resource_weights[s];
    if (w < 0 || w > 100) return fail(c, GS_EINVAL, "NodeNUMAResource weight of slot %d not in [0, 100]", s);
    pf.numa_w[s] = (int32_t)w;
  }
  pf.numa_most = cfg.numa.scoring_type == GS_SCORING_MOST_ALLOCATED;
  pf.numa_hint_most = cfg.numa.numa_scoring_type == GS_SCORING_MOST_ALLOCATED;
  {
    int d = cfg.numa.default_cpu_bind_policy;   // validation.ValidateNodeNUMAResourceArgs (validation_pluginargs.go:156-172)
    if (d != GS_CPU_BIND_UNSET && d != GS_CPU_BIND_FULL_PCPUS && d != GS_CPU_BIND_SPREAD_BY_PCPUS)
      return fail(c, GS_EINVAL, "defaultCPUBindPolicy must specified CPU bind policy FullPCPUs or SpreadByPCPUs");
  }
  pf.w_fit = (int32_t)cfg.plugin_weights[GS_PLUGIN_FIT];
  pf.w_la = (int32_t)cfg.plugin_weights[GS_PLUGIN_LOADAWARE];
  for (int r = 0; r < 2; ++r) {
    if (cfg.loadaware.resource_weights_mask & (1u << r)) {
      // validateResourceWeights (validation_pluginargs.go:61-70): a present key is in (0, 100]; the weighted mean's
      // division (small_div) is exact for sums below 2^24 only
      const int64_t w = cfg.loadaware.resource_weights[r];
      if (w <= 0 || w > 100) return fail(c, GS_EINVAL, "LoadAwareScheduling resource weight %d not in (0, 100]", r);
      pf.la_w[r] = (int32_t)w;
    }
    pf.la_wsum += pf.la_w[r];
  }
  for (int s = 0; s < 7; ++s) {
    int64_t w = cfg.fit.resource_weights[s];
    if (w < 0 || w > 100) return fail(c, GS_EINVAL, "NodeResourcesFit weight of slot %d not in (0, 100]", s);
    pf.fit_w[s] = (int32_t)w;
    if (s >= 2 && w) pf.fit_scalar_w_mask |= 1u << s;
  }
  if (cfg.fit.resource_weights[7]) return fail(c, GS_EINVAL, "resource slot 7 is reserved");
  if ((pf.enabled & GS_ENABLE_LA_SCORE) && pf.la_wsum == 0)
    return fail(c, GS_EINVAL, "LoadAwareScheduling scoring needs at least one resource weight");
  int64_t ms = 0;
  if (pf.enabled & GS_ENABLE_FIT_SCORE) ms += 100 * cfg.plugin_weights[GS_PLUGIN_FIT];
  if (pf.enabled & GS_ENABLE_LA_SCORE) ms += 100 * cfg.plugin_weights[GS_PLUGIN_LOADAWARE];
  if (pf.enabled & GS_ENABLE_NUMA_SCORE) ms += 100 * cfg.plugin_weights[GS_PLUGIN_NUMA];
  if (cfg.plugin_weights[0] < 0 || cfg.plugin_weights[1] < 0 || cfg.plugin_weights[2] < 0 || ms > MAX_SCORE_LIMIT)
    return fail(c, GS_EUNSUPPORTED, "profile score weights must keep the max total score <= %d (got %lld)",
                MAX_SCORE_LIMIT, (long long)ms);
  c->max_score = (int)ms;
  return GS_OK;
}

// GS_XCHG=levels (read at every comm init): the per-shard candidate levels instead of the score rows
bool xchg_levels() { const char* x = env_str("GS_XCHG"); return x && std::strcmp(x, "levels") == 0; }

void set_shard(gs_ctx* c) {
  uint32_t per = (c->N + c->nranks - 1) / c->nranks;
  c->e0 = std::min(c->N, per * (uint32_t)c->rank);
  c->e1 = std::min(c->N, c->e0 + per);
  c->sgather = c->nranks > 1 && !xchg_levels();
  c->n0 = c->sgather ? 0 : c->e0;
  c->n1 = c->sgather ? c->N : c->e1;
  c->sx_per = per;
  c->sx_pld = (per + 1023) / 1024 * 1024;
  c->stats.shard_begin = c->e0;
  c->stats.shard_end = c->e1;
}

// set_shard of a context that may have scheduled already (comm init, after quiesce). The score rows get their -1 padding
// once, in gs_create; the eval pass rewrites [0, round_up(len, 256)) of a row and the level kernels read
// [0, round_up(len, 512)), so a row that becomes shorter would keep scores of the longer rows' batches between the two
// (counted as feasible nodes, listed with node ids of another shard or past N): every slot's rows are filled again.
int reshard(gs_ctx* c) {
  const uint32_t n0 = c->n0, n1 = c->n1;
  set_shard(c);
  if (c->n0 == n0 && c->n1 == n1) return GS_OK;
  HIP_TRY(c, hipSetDevice(c->cfg.device));
  HIP_TRY(c, hipStreamSynchronize(c->st_ev.get()));
  for (Slot& sl : c->slot)
    if (sl.d_S) HIP_TRY(c, hipMemsetAsync(sl.d_S.get(), 0xff, (size_t)c->B * c->ld * 2, c->st.get()));
  HIP_TRY(c, hipStreamSynchronize(c->st.get()));
  return GS_OK;
}

// ranks whose candidate levels the commit merges: 1 unless the ranks exchange level lists (GS_XCHG=levels)
int lvl_ranks(const gs_ctx* c) { return c->sgather ? 1 : c->nranks; }

// one rank's exchange block: [B x lstride listed node ids | B LevelHdr | B LevelExt | ... | XTag], padded to 256 B (the
// tag in the block's last 32 bytes)
size_t lists_bytes(int B, int lstride) { return (size_t)B * lstride * 4; }
size_t xchg_block_bytes(int B, int lstride) {
  size_t raw = lists_bytes(B, lstride) + (size_t)B * (sizeof(LevelHdr) + sizeof(LevelExt)) + sizeof(XTag);
  return (raw + 255) / 256 * 256;
}

int alloc_exchange(gs_ctx* c) {
  // the speculative commit merges the shards' lists: XCAP listed nodes per (pod, shard) are enough for a pod at batch
  // position k (k + 1 per shard), and the all-gathered block is 8x smaller; the other kernels read LCAP-wide blocks
  // (score rows: every rank runs the one-shard pipeline over all nodes, LCAP-wide local lists)
  c->lstride = !c->sgather && commit_spec_selected(c->window_k) ? XCAP : LCAP;
  c->xchg_bytes = xchg_block_bytes(c->B, c->lstride);
  // (alloc() frees the old block first, here and below: comm init runs after quiesce, with no batch in flight)
  HIP_TRY(c, c->d_xchg_recv.alloc(c->xchg_bytes * c->nranks + 64));
  HIP_TRY(c, c->h_xchg_recv.alloc(c->xchg_bytes * c->nranks + 64));
  HIP_TRY(c, c->d_xmerged.alloc(xchg_block_bytes(c->B, LCAP) + 64));
  if (!c->d_xerr) HIP_TRY(c, c->d_xerr.alloc(2 * XERR_BYTES));   // one per batch slot (score rows)
  HIP_TRY(c, hipMemset(c->d_xerr.get(), 0, 2 * XERR_BYTES));
  c->sx_send_all.reset();
  c->sx_recv_all.reset();
  c->h_sx_send.reset();
  c->h_sx_recv.reset();
  for (Slot& sl : c->slot) sl.d_sx_send = sl.d_sx_recv = nullptr;
  c->sx_bytes = 0;
  if (c->sgather) {
    c->sx_bytes = ((size_t)c->B * c->sx_pld * 3 + sizeof(XTag) + 255) / 256 * 256;
    HIP_TRY(c, c->sx_send_all.alloc(c->sx_bytes * 2));               // one per batch slot
    HIP_TRY(c, c->sx_recv_all.alloc(c->sx_bytes * c->nranks * 2));
    if (c->cb) {
      HIP_TRY(c, c->h_sx_send.alloc(c->sx_bytes));
      HIP_TRY(c, c->h_sx_recv.alloc(c->sx_bytes * c->nranks));
    }
    for (int k = 0; k < 2; ++k) {
      c->slot[k].d_sx_send = c->sx_send_all.get() + c->sx_bytes * k;
      c->slot[k].d_sx_recv = c->sx_recv_all.get() + c->sx_bytes * c->nranks * k;
    }
  }
  for (int k = 0; k < 2; ++k)
    c->slot[k].d_xerr = c->sgather ? c->d_xerr.get() + (XERR_BYTES / 4) * k : c->nranks > 1 ? c->d_xerr.get() : nullptr;
  if (!c->d_xsmall) HIP_TRY(c, c->d_xsmall.alloc(XSMALL * (1 + MAX_RANKS)));
  if (!c->h_xsmall) HIP_TRY(c, c->h_xsmall.alloc(XSMALL * MAX_RANKS));
  if (const char* sk = env_str("GS_DEBUG_XCHG_SKEW")) {   // "rank:batch" (tests of the sequence check)
    long r = -1;
    unsigned long long b = 0;
    if (sscanf(sk, "%ld:%llu", &r, &b) == 2) { c->dbg_xskew_rank = r; c->dbg_xskew_batch = b; }
  }
  return GS_OK;
}

constexpr int GS_REDO = 1;   // internal: re-run the batch (its score rows were overwritten by a speculative pass)
constexpr size_t COMMITTED_BYTES = 32;   // committed[0..7] (the commit kernels write [0..4]); the placements follow

// The candidate levels of a one-shard pass without node sampling are built on st_ev right after the eval pass (beside
// the previous batch's commit, on the stale rows it lands on), then fixed up on st once that commit is done
// A batch with no speculative pass before it, of at most SHORT_BATCH pods, on one shard: its
// upload, eval pass and levels go on st in order instead of through st_ev. st_ev then waits for that eval pass and its
// levels (launch_batch): a speculative pass enqueued after it on st_ev shares the NUMA slab, st2 and the fork / join
// events with it, so it starts only once they are done. Short runs (the plain pods between C5's extension pods) lose
// two queue hops per batch.
// SHORT_BATCH: a batch of fewer pods is short (the host waits on each one): it is read back in order on st and, when
// direct, untimed; a batch of up to SHORT_BATCH pods may run direct.
constexpr int SHORT_BATCH = 32;
bool direct_batch(const gs_ctx* c, int b, bool speculative) {
  return !speculative && b <= SHORT_BATCH && lvl_ranks(c) == 1;
}

bool cand_overlapped(const gs_ctx* c, const Slot& s) {
  return c->cand_overlap && lvl_ranks(c) == 1 && !c->window_k && s.d_lst;
}

CommitArgs commit_args(gs_ctx* c, const Slot& s, int b) {
  CommitArgs a{};
  a.m = c->mv;
  a.pods = s.d_pods.get();
  a.seq = s.d_seq;
  a.npods = b;
  a.nranks = lvl_ranks(c);
  // several level shards: the speculative commit reads their merged levels
  a.xbase = a.nranks == 1 ? (cand_overlapped(c, s) ? s.d_lst.get() : c->d_xchg_send.get()) : c->d_xmerged.get();
  a.bmax = c->B;
  a.pf = c->pf;
  a.seed = c->cfg.seed;
  a.forced_node = -1;
  a.out = s.d_out;
  a.committed = s.d_committed.get();
  a.stamps = c->d_stamps.get();
  a.topos = c->d_topos.get();
  a.aff = s.d_aff.get();
  a.ld = c->ld;
  a.own0 = c->n0;
  a.own1 = c->n1;
  a.S = a.nranks == 1 ? s.d_S.get() : nullptr;
  a.S_own = s.d_S.get();
  a.window_k = c->window_k;
  a.start = c->next_start;
  a.nnodes = c->N;
  a.tb = s.d_tb;
  a.landed = s.d_landed.get();
  a.xerr = s.d_xerr;
  return a;
}

// ---- FitError diagnosis (gs_schedule_diag; kernels: gs_fit_diag.hip) ----
constexpr size_t DIAG_BYTES = sizeof(uint32_t) * MAX_BATCH * DIAG_WORDS;
// the landed pass's staged block at its largest: DIAG_VERSIONS rows and indices, MAX_BATCH pod vectors, the index table
constexpr size_t DGL_BYTES = (size_t)DIAG_VERSIONS * (ROW_WORDS * 8 + 4) + 8 + sizeof(PodVec) * MAX_BATCH +
                             2 * (size_t)MAX_BATCH * MAX_BATCH;

// the buffers and the stream of the diagnosis, on the context's first run that asks for one
int alloc_diag(gs_ctx* c) {
  if (c->st_dg) return GS_OK;
  HIP_TRY(c, hipSetDevice(c->cfg.device));
  for (Slot& s : c->slot) {
    HIP_TRY(c, s.ev_dg.create(hipEventDisableTiming));
    HIP_TRY(c, s.d_diag.alloc(DIAG_BYTES));
    HIP_TRY(c, s.h_diag.alloc(DIAG_BYTES));
    HIP_TRY(c, s.h_dgl.alloc(DGL_BYTES));
    HIP_TRY(c, s.d_dgl.alloc(DGL_BYTES));
    HIP_TRY(c, s.dgl_i64.alloc((size_t)NUM_I64_COLS * DIAG_VERSIONS * 8));
    HIP_TRY(c, s.dgl_i32.alloc((size_t)NUM_I32_COLS * DIAG_VERSIONS * 4));
    HIP_TRY(c, s.d_ldiag.alloc(DIAG_BYTES));
    HIP_TRY(c, s.h_ldiag.alloc(DIAG_BYTES));
  }
  HIP_TRY(c, c->st_dg.create(hipStreamNonBlocking));
  return GS_OK;
}

// the buffers of the status map, on the context's first run that asks for one (after alloc_diag)
int alloc_map(gs_ctx* c) {
  if (c->slot[0].d_words) return GS_OK;
  HIP_TRY(c, hipSetDevice(c->cfg.device));
  const size_t rows = sizeof(uint16_t) * MAX_BATCH * (size_t)c->npad, lw = sizeof(uint16_t) * MAX_BATCH * MAX_BATCH;
  for (Slot& s : c->slot) {
    HIP_TRY(c, s.ev_rows.create(hipEventDisableTiming));
    HIP_TRY(c, s.h_words.alloc(rows));
    HIP_TRY(c, s.d_lwords.alloc(lw));
    HIP_TRY(c, s.h_lwords.alloc(lw));
    HIP_TRY(c, s.d_words.alloc(rows));
    // the rows start out zeroed, and the read-back path (fetch_rows: copy, event) has run once before a batch is in
    // flight: its first use costs the host milliseconds, which between two batches would delay the next launch
    HIP_TRY(c, hipMemsetAsync(s.d_words.get(), 0, rows, c->st_dg.get()));
    HIP_TRY(c, hipMemcpyAsync(s.h_words.get(), s.d_words.get(), rows, hipMemcpyDeviceToHost, c->st_dg.get()));
    HIP_TRY(c, hipEventRecord(s.ev_rows.get(), c->st_dg.get()));
  }
  HIP_TRY(c, host_wait_stream(c->st_dg.get()));
  HIP_TRY(c, preload_fit_diag_map());
  return GS_OK;
}

// the buffers of the top-N score tables, on the context's first run that asks for them (after alloc_diag: the landed
// pass shares the diagnosis' staged block, slab and stream)
int alloc_top(gs_ctx* c) {
  if (c->slot[0].d_top) return GS_OK;
  HIP_TRY(c, hipSetDevice(c->cfg.device));
  const size_t lt = sizeof(TopLanded) * MAX_BATCH * MAX_BATCH;
  for (Slot& s : c->slot) {
    HIP_TRY(c, s.h_top.alloc(TOP_BYTES));
    HIP_TRY(c, s.d_ltop.alloc(lt));
    HIP_TRY(c, s.h_ltop.alloc(lt));
    HIP_TRY(c, s.d_top.alloc(TOP_BYTES));
    // the read-back path has run once before a batch is in flight (its first use costs the host milliseconds)
    HIP_TRY(c, hipMemsetAsync(s.d_top.get(), 0, TOP_BYTES, c->st_dg.get()));
    HIP_TRY(c, hipMemcpyAsync(s.h_top.get(), s.d_top.get(), TOP_BYTES, hipMemcpyDeviceToHost, c->st_dg.get()));
  }
  HIP_TRY(c, host_wait_stream(c->st_dg.get()));
  HIP_TRY(c, preload_top_scores());
  return GS_OK;
}

TopArgs top_args(const gs_ctx* c, const Slot& s, int b) {
  TopArgs a{};
  a.m = c->mv;
  a.pods = s.d_pods.get();
  a.pf = c->pf;
  a.N = c->N;
  a.npods = b;
  a.committed = s.d_committed.get();
  a.out = s.d_out;
  a.S = s.d_S.get();
  a.ld = c->ld;
  a.topn = s.rep.topn;
  a.nbins = c->max_score + 1;
  a.top = s.d_top.get();
  return a;
}

DiagMapArgs diag_args(const gs_ctx* c, const Slot& s, int b) {
  DiagMapArgs a{};
  a.m = c->mv;
  a.pods = s.d_pods.get();
  a.pf = c->pf;
  a.N = c->N;
  a.npods = b;
  a.committed = s.d_committed.get();
  a.out = s.d_out;
  a.diag = s.d_diag.get();
  a.numa_idx = c->d_numa_idx.get();   // (one rank: the list covers every node)
  a.numa_n = c->numa_on ? c->numa_n : 0;
  a.words = s.d_words.get();
  a.npad = c->npad;
  return a;
}

// The reports of slot s's batch of b pods (s.rep) behind its commit on st: the wide pass over counters zeroed first
// (clear; force0: for pod 0 alone, which the host found unschedulable, on every node of the mirror), or the top-N
// score tables' pass. rb: the stream of the batch's read-back, which waits for the pass.
int launch_reports(gs_ctx* c, Slot& s, int b, hipStream_t st, hipStream_t rb, bool clear, bool force0 = false) {
  if (s.rep.diag) {
    if (clear) HIP_TRY(c, hipMemsetAsync(s.d_diag.get(), 0, DIAG_BYTES, st));
    DiagMapArgs a = diag_args(c, s, b);
    a.force0 = force0 ? 1 : 0;
    HIP_TRY(c, s.rep.rows ? launch_fit_diag_map(a, st) : launch_fit_diag(a, st));
  } else {
    HIP_TRY(c, launch_top_scores(top_args(c, s, b), st));
  }
  if (rb != st) {
    HIP_TRY(c, hipEventRecord(s.ev_dg.get(), st));
    HIP_TRY(c, hipStreamWaitEvent(rb, s.ev_dg.get(), 0));
  }
  return GS_OK;
}

// ... and their read-back for the batch's first n pods, beside the placements': the wide pass's counters, or the counts
// and rows of the tables
int read_reports(gs_ctx* c, Slot& s, int n, hipStream_t rb) {
  if (s.rep.diag)
    HIP_TRY(c, hipMemcpyAsync(s.h_diag.get(), s.d_diag.get(), sizeof(uint32_t) * DIAG_WORDS * n, hipMemcpyDeviceToHost, rb));
  else
    HIP_TRY(c, hipMemcpyAsync(s.h_top.get(), s.d_top.get(), TOP_COUNT_BYTES + TOP_POD_BYTES * n, hipMemcpyDeviceToHost, rb));
  return GS_OK;
}

// What the landed pass evaluates: the diagnosis' counters, those with the status words, or the top-N totals.
enum class Landed { DIAG, DIAG_MAP, TOP };

// The landed pass of a batch (blocking; off the commit stream): nv row versions staged at the head of s.h_dgl are
// scattered into the slot's slab with their LoadAware verdicts at `now`, and pod f (fpods[f]) is evaluated on versions
// vidx[f * nL ..]. DIAG: the nF pods' counters arrive in s.h_ldiag; DIAG_MAP: their status words [f][nL] in s.h_lwords
// too; TOP: the nF x nL totals and plugin scores in s.h_ltop.
int landed_pass(gs_ctx* c, Slot& s, Landed kind, int nv, const std::vector<PodVec>& fpods, const std::vector<uint16_t>& vidx,
                int nL) {
  const int nF = (int)fpods.size();
  const size_t off_idx = (size_t)nv * ROW_WORDS * 8;
  const size_t off_pods = (off_idx + (size_t)nv * 4 + 7) & ~(size_t)7;
  const size_t off_vidx = off_pods + sizeof(PodVec) * nF;
  const size_t total = off_vidx + 2 * (size_t)nF * nL;
  if (nv > DIAG_VERSIONS || total > DGL_BYTES)
    return fail(c, GS_ESTATE, "%s: landed-row versions overflow", kind == Landed::TOP ? "top scores" : "FitError diagnosis");
  uint8_t* h = s.h_dgl.get();
  uint32_t* h_idx = reinterpret_cast<uint32_t*>(h + off_idx);
  for (int v = 0; v < nv; ++v) h_idx[v] = (uint32_t)v;
  std::memcpy(h + off_pods, fpods.data(), sizeof(PodVec) * nF);
  std::memcpy(h + off_vidx, vidx.data(), 2 * (size_t)nF * nL);
  const hipStream_t st = c->st_dg.get();
  uint8_t* d = s.d_dgl.get();
  const MirrorView slab{s.dgl_i64.get(), s.dgl_i32.get(), (uint32_t)DIAG_VERSIONS};
  const gs_loadaware_args& la = c->cfg.loadaware;
  const ScatterPrep sp{c->now, la.filter_expired_node_metrics, la.has_node_metric_expiration,
                       la.has_node_metric_expiration ? la.node_metric_expiration_seconds * 1000000000LL : 0};
  HIP_TRY(c, hipMemcpyAsync(d, h, total, hipMemcpyHostToDevice, st));
  HIP_TRY(c, launch_scatter_rows(slab, reinterpret_cast<const uint32_t*>(d + off_idx), reinterpret_cast<const int64_t*>(d),
                                 (uint32_t)nv, st, &sp));
  const PodVec* d_pods = reinterpret_cast<const PodVec*>(d + off_pods);
  const uint16_t* d_vidx = reinterpret_cast<const uint16_t*>(d + off_vidx);
  if (kind == Landed::TOP) {
    HIP_TRY(c, launch_top_scores_landed(slab, d_pods, c->pf, d_vidx, nF, nL, s.d_ltop.get(), st));
    HIP_TRY(c, hipMemcpyAsync(s.h_ltop.get(), s.d_ltop.get(), sizeof(TopLanded) * nF * nL, hipMemcpyDeviceToHost, st));
  } else {
    if (kind == Landed::DIAG_MAP) {
      HIP_TRY(c, launch_fit_diag_landed_map(slab, d_pods, c->pf, d_vidx, nF, nL, s.d_ldiag.get(), s.d_lwords.get(), st));
      HIP_TRY(c, hipMemcpyAsync(s.h_lwords.get(), s.d_lwords.get(), sizeof(uint16_t) * nF * nL, hipMemcpyDeviceToHost, st));
    } else {
      HIP_TRY(c, launch_fit_diag_landed(slab, d_pods, c->pf, d_vidx, nF, nL, s.d_ldiag.get(), st));
    }
    HIP_TRY(c, hipMemcpyAsync(s.h_ldiag.get(), s.d_ldiag.get(), sizeof(uint32_t) * DIAG_WORDS * nF, hipMemcpyDeviceToHost, st));
  }
  Where w_(c, "landed_pass: the landed pass");
  HIP_TRY(c, host_wait_stream(st));
  return GS_OK;
}

// Enqueue one device pass over pods [0, b) of slot s's staged batch, and its read-back; no host wait.
// The eval pass runs on st_ev, the rest on st. before != nullptr: a speculative pass behind slot `before`'s batch of
// prev_b pods (prev: its committed words, prev_out: its placements): its eval pass runs beside that batch's commit, on
// the mirror as it was before it, and the rows that batch landed on are re-evaluated on st once it committed (patch_kernel);
// its commit kernel does nothing unless that batch committed every pod and needs no host-side Reserve (prev[1] == 1).
// rep.diag: the FitError diagnosis' wide pass behind the commit, its counters read back with the placements; rep.rows:
// the pass also leaves the status rows in the slot's d_words (fetch_rows reads back the ones the caller has room for).
// rep.topn > 0: the top-N score tables' pass behind the commit instead, its counts and rows read back with the placements.
int launch_batch(gs_ctx* c, Slot& s, int b, ReportMode rep, const Slot* before = nullptr, int prev_b = 0) {
  const int32_t* prev = before ? before->d_committed.get() : nullptr;
  const PlacementDev* prev_out = before ? before->d_out : nullptr;
  const hipStream_t st = c->st.get(), st_ev = c->st_ev.get();
  PodVec *const d_pods = s.d_pods.get(), *const h_pods = s.h_pods.get();
  int16_t* const d_S = s.d_S.get();
  uint8_t* const d_aff = s.d_aff.get();
  const bool ovl = cand_overlapped(c, s);
  uint8_t* lblk = ovl ? s.d_lst.get() : c->d_xchg_send.get();
  uint32_t* d_lists = reinterpret_cast<uint32_t*>(lblk);
  LevelHdr* d_hdrs = reinterpret_cast<LevelHdr*>(lblk + lists_bytes(c->B, c->lstride));
  LevelExt* d_ext = reinterpret_cast<LevelExt*>(lblk + lists_bytes(c->B, c->lstride) + (size_t)c->B * sizeof(LevelHdr));
  int prod_cols = 0;
  for (int i = 0; i < b; ++i) prod_cols |= (h_pods[i].flags & PF_PROD_SCORE) ? 1 : 0;
  uint32_t len = c->n1 - c->n0;
  if (c->numa_on && (c->numa_idx_stale || c->numa_idx_lo != c->e0 || c->numa_idx_hi != c->e1)) {
    std::vector<uint32_t> idx;   // the policy nodes this rank evaluates
    for (uint32_t n = c->e0; n < c->e1; ++n)
      if (c->numa[n].cfg.numa_topology_policy != GS_NUMA_POLICY_NONE) idx.push_back(n);
    if (c->d_numa_idx) {
      HIP_TRY(c, host_wait_stream(st));
      HIP_TRY(c, host_wait_stream(st_ev));
      c->d_numa_idx.reset();
    }
    c->numa_n = (uint32_t)idx.size();
    if (c->numa_n) {
      HIP_TRY(c, c->d_numa_idx.alloc(4 * idx.size()));
      HIP_TRY(c, hipMemcpy(c->d_numa_idx.get(), idx.data(), 4 * idx.size(), hipMemcpyHostToDevice));
    }
    if (c->numa_n > c->slab_cap) {   // columns of numa_n entries (rounded), the mirror's numbering
      HIP_TRY(c, host_wait_stream(st_ev));
      c->slab_mv = MirrorView{nullptr, nullptr, 0};
      c->slab_i64.reset();
      c->slab_i32.reset();
      c->slab_cap = (c->numa_n + 1023) & ~1023u;
      HIP_TRY(c, c->slab_i64.alloc((size_t)NUM_I64_COLS * c->slab_cap * 8));
      HIP_TRY(c, c->slab_i32.alloc((size_t)NUM_I32_COLS * c->slab_cap * 4));
      c->slab_mv = MirrorView{c->slab_i64.get(), c->slab_i32.get(), c->slab_cap};
    }
    c->numa_idx_stale = false;
    c->numa_idx_lo = c->e0;
    c->numa_idx_hi = c->e1;
  }
  // a short batch with no pass beside it: upload, eval and levels in order on st (no queue hops)
  const bool direct = direct_batch(c, b, prev != nullptr);
  hipStream_t se = direct ? st : st_ev;
  // full batches: readback on its own stream, so that the speculative next batch's patch / cand start right after the
  // commit (the slot's buffers are rewritten only after finish_batch has waited for ev[5]). Short batches (the host
  // waits on each one) keep it in order on st: the extra queue hop costs more than it hides there.
  hipStream_t rb = b >= SHORT_BATCH ? c->st_rb.get() : st;
  // A direct batch read back on st records no timing events: three HIP calls less per short plain run (C5 at 100k nodes,
  // medians of 7 alternations: 23.6k against 21.8k pods/s); its eval and levels intervals are not counted in the stats,
  // the commit's comes from the kernel. (st_rb waits on ev[4]: a batch read back there is always timed.)
  const bool untimed = direct && rb == st;
  s.untimed = untimed;
  if (!untimed) HIP_TRY(c, hipEventRecord(s.ev[0].get(), se));
  if (c->sgather) {
    // several ranks, score rows: this rank's shard into its block of the all-gather (rows of sx_pld entries), then the
    // R blocks into the full-width rows S / aff: every rank continues with the one-shard pipeline over all nodes
    const uint32_t pld = c->sx_pld;
    uint8_t *blk = s.d_sx_send, *rcv = s.d_sx_recv;
    HIP_TRY(c, launch_eval(c->mv, d_pods, b, c->pf, c->e0, c->e1, reinterpret_cast<int16_t*>(blk), pld, prod_cols,
                           c->d_numa_idx.get(), c->numa_n, blk + (size_t)b * pld * 2, se, c->st2.get(),
                           c->ev_fork.get(), c->ev_join.get(), c->slab_mv.i64 ? &c->slab_mv : nullptr));
    if (!untimed) HIP_TRY(c, hipEventRecord(s.ev[1].get(), se));
    const size_t bytes = ((size_t)b * pld * 3 + sizeof(XTag) + 255) / 256 * 256;
    if (int rc = exchange(c, XSITE_SCORES, blk, rcv, bytes, nullptr, se)) return rc;
    HIP_TRY(c, launch_unpack_scores(rcv, bytes, c->nranks, b, c->sx_per, pld, c->N, d_S, d_aff, c->ld, s.d_xerr, se));
  } else {
    HIP_TRY(c, launch_eval(c->mv, d_pods, b, c->pf, c->n0, c->n1, d_S, c->ld, prod_cols, c->d_numa_idx.get(), c->numa_n,
                           d_aff, se, c->st2.get(), c->ev_fork.get(), c->ev_join.get(),
                           c->slab_mv.i64 ? &c->slab_mv : nullptr));
    if (!untimed) HIP_TRY(c, hipEventRecord(s.ev[1].get(), se));
  }
  const bool fix = ovl && prev && prev_b > 0;
  int32_t tb_ready = 0;
  if (ovl) {
    // levels on st_ev beside the previous batch's commit: the rows it lands on are stale here (listed with a margin of
    // prev_b nodes, histogram kept), fixed up on st below once it committed
    CandPatch cp{};
    cp.extra = fix ? prev_b : 0;
    cp.hist = fix ? s.d_hist.get() : nullptr;
    // the batch's tie-break records too (off the commit's prologue); a short batch split over cs_* kernels leaves them
    // to the commit
    cp.tb = s.d_tb;
    cp.seq = s.d_seq;
    cp.seed = c->cfg.seed;
    HIP_TRY(c, launch_cand(d_S, c->ld, len, c->n0, b, c->max_score, c->lstride, d_lists, d_hdrs, d_ext, se, &cp,
                           c->d_cscratch.get(), &tb_ready));
  }
  if (!direct) {
    HIP_TRY(c, hipEventRecord(s.ev_evdone.get(), st_ev));
    HIP_TRY(c, hipStreamWaitEvent(st, s.ev_evdone.get(), 0));
  } else {   // the next speculative pass on st_ev (gather into the shared slab, eval) after this one
    HIP_TRY(c, hipEventRecord(s.ev_evdone.get(), st));
    HIP_TRY(c, hipStreamWaitEvent(st_ev, s.ev_evdone.get(), 0));
  }
  if (fix) {
    CandPatch cp{c->mv, d_pods, c->pf, c->n0, c->n1, prod_cols, 0, d_aff, prev_out, prev};
    cp.extra = prev_b;
    cp.hist = s.d_hist.get();
    cp.landed = before->d_landed.get();   // (the slab the previous batch's commit leaves)
    HIP_TRY(c, launch_fix_levels(d_S, c->ld, b, c->max_score, c->lstride, d_lists, d_hdrs, d_ext, cp, st));
  }
  // the rows the previous batch landed on, re-evaluated on their committed state: inside cand_kernel (block k patches
  // pod k's row before its histogram; one launch less on the commit chain), or by patch_kernel under node sampling
  // (no candidate levels)
  const bool fused = prev && prev_b > 0 && !c->window_k;
  if (!ovl && prev && !fused)
    HIP_TRY(c, launch_patch(c->mv, d_pods, b, c->pf, c->n0, c->n1, d_S, c->ld, prod_cols, d_aff, prev_out, prev, prev_b,
                            st));
  if (!c->window_k && !ovl) {   // node sampling selects over the rotation window, not the candidate levels
    CandPatch cp{c->mv, d_pods, c->pf, c->n0, c->n1, prod_cols, 1, d_aff, prev_out, prev};
    HIP_TRY(c, launch_cand(d_S, c->ld, len, c->n0, b, c->max_score, c->lstride, d_lists, d_hdrs, d_ext, st,
                           fused ? &cp : nullptr, c->d_cscratch.get()));
  }
  // no timing markers between the levels and the commit kernel (each one held the commit's dispatch ~13 us): the
  // commit's duration comes from the kernel itself (committed[4]), the levels' interval is the rest up to ev[4]
  if (lvl_ranks(c) > 1) {
    int rc = exchange(c, XSITE_LEVELS, c->d_xchg_send.get(), c->d_xchg_recv.get(), c->xchg_bytes);
    if (rc) return rc;
    HIP_TRY(c, launch_merge_levels(c->d_xchg_recv.get(), c->xchg_bytes, c->nranks, b, c->B, c->lstride,
                                   c->d_xmerged.get(), s.d_xerr, st));
  }
  CommitArgs a = commit_args(c, s, b);
  a.prev = prev;
  a.tb_ready = tb_ready;
  ++c->xbatch;
  count_spec_launch(c, a);
  HIP_TRY(c, launch_commit(a, st));
  if (!untimed) HIP_TRY(c, hipEventRecord(s.ev[4].get(), st));
  if (rb != st) HIP_TRY(c, hipStreamWaitEvent(rb, s.ev[4].get(), 0));
  s.rep = rep;
  if (rep.rows && s.rows_in_flight) {   // the rows of the slot's last batch are still being read back (fetch_rows)
    HIP_TRY(c, hipStreamWaitEvent(st, s.ev_rows.get(), 0));
    s.rows_in_flight = false;
  }
  // behind the commit's write-back, before the next batch's fix-up and commit (stream order): the mirror holds the
  // commit's write-back, the slot's score rows are still the batch's
  if (rep.any())
    if (int rc = launch_reports(c, s, b, st, rb, true)) return rc;
  // Two copies, not one over the adjacent committed words and placements: with one merged copy, 4 processes sharing the
  // GPU (the C4 rehearsal) stalled for 10-100 s at a time, every rank's commit and next eval pass pending;
  // for a direct batch the merged form measured within noise
  HIP_TRY(c, hipMemcpyAsync(s.h_committed.get(), s.d_committed.get(), COMMITTED_BYTES, hipMemcpyDeviceToHost, rb));
  HIP_TRY(c, hipMemcpyAsync(s.h_out, s.d_out, sizeof(PlacementDev) * b, hipMemcpyDeviceToHost, rb));
  if (rep.any())
    if (int rc = read_reports(c, s, b, rb)) return rc;
  HIP_TRY(c, hipEventRecord(s.ev[5].get(), rb));
  return GS_OK;
}

// Wait for slot s's batch; when it committed nothing, resolve its pod 0 by the exact full-row path
// (several shards). clobbered: a speculative pass has overwritten the score rows and lists since -> GS_REDO.
int finish_batch(gs_ctx* c, Slot& s, int b, bool clobbered, int* committed_out) {
  uint32_t len = c->n1 - c->n0;
  const hipStream_t st = c->st.get();
  int32_t* const h_committed = s.h_committed.get();
  {
    Where w_(c, "finish_batch: the batch's readback event");
    HIP_TRY(c, host_wait_event(s.ev[5].get()));
  }
  flush_exchange_times(c);
  if (!s.untimed) c->stats.eval_ms += ev_ms(s.ev[0].get(), s.ev[1].get());
  {   // commit kernel: its own duration (s_memrealtime, 100 MHz) in committed[4]; levels: the rest from the eval's end
    const double cm = (double)(uint32_t)h_committed[4] * 1e-5;
    c->stats.commit_ms += cm;
    if (!s.untimed) c->stats.cand_ms += std::max(0.0, ev_ms(s.ev[1].get(), s.ev[4].get()) - cm);
  }
  c->stats.eval_launches += 1;
  c->stats.eval_pairs += (uint64_t)b * (c->e1 - c->e0);
  c->stats.batches += 1;
  int committed = h_committed[0];
  if (committed < 0) return fail(c, GS_ESTATE, "commit pass of a batch was voided unexpectedly");
  if (h_committed[3] == COMMIT_ERR_XTAG) {   // the level exchange paired different exchanges of the ranks
    // the first mismatching exchange's tags, as merge_levels_kernel kept them
    std::vector<uint8_t> xe(XERR_BYTES);
    HIP_TRY(c, host_wait_stream(st));
    HIP_TRY(c, hipMemcpy(xe.data(), s.d_xerr, xe.size(), hipMemcpyDeviceToHost));
    const uint8_t* tags = xe.data() + 4 * XERR_TAGS;
    XTag mine;
    std::memcpy(&mine, tags + (size_t)c->rank * sizeof(XTag), sizeof mine);
    if (int rc = check_tags(c, tags, sizeof(XTag), mine)) return rc;
    return fail(c, GS_ECOMM, "exchange sequence diverged at a %s exchange (device check)",
                c->sgather ? "score-row" : "level");
  }
  if (h_committed[3])
    return fail(c, GS_EDEVICE, "commit kernel: a pipeline wait expired (internal error, site %d)", h_committed[3]);
  if (c->window_k) {
    if (committed == 0) return fail(c, GS_ESTATE, "node-sampling commit made no progress");
    c->next_start = (uint32_t)h_committed[2];
    c->stats.next_start_node_index = c->next_start;
  }
  if (committed == 0 && clobbered) return GS_REDO;
  if (committed == 0) {
    CommitArgs a = commit_args(c, s, b);
    // exact full-row path for pod 0: (max, ties, feasible) of every shard's row, global selection
    HIP_TRY(c, launch_row_stats(s.d_S.get(), len, c->d_rowstat.get(), st));
    const int lr = lvl_ranks(c);
    std::vector<RowStat> rs(lr);
    if (lr > 1) {
      int rc = exchange_small(c, XSITE_ROWSTAT, c->d_rowstat.get(), sizeof(RowStat), rs.data());
      if (rc) return rc;
    } else {
      HIP_TRY(c, hipMemcpyAsync(rs.data(), c->d_rowstat.get(), sizeof(RowStat), hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(c, host_wait_stream(st));
    int M = -1;
    int64_t T = 0, F = 0;
    for (const auto& r : rs) {
      F += r.feasible;
      if (r.max_score > M) { M = r.max_score; T = r.ties; }
      else if (r.max_score == M && M >= 0) T += r.ties;
    }
    if (M < 0) {
      s.h_out[0] = PlacementDev{-1, (uint32_t)F, 0, 0, GS_PLACED_SLOWPATH, 0, 0, {0, 0, 0, 0}, {0, 0, 0, 0}};
      if (s.rep.diag) {   // a FitError the host found: nothing landed in the pass, every node from the mirror
        if (int rc = launch_reports(c, s, b, st, st, false, true)) return rc;
        if (int rc = read_reports(c, s, 1, st)) return rc;
        HIP_TRY(c, host_wait_stream(st));
      }
      *committed_out = 1;
      return GS_OK;
    }
    int64_t jstar = host_tiebreak_position(c->cfg.seed, s.h_seq[0], T);
    int owner = -1;
    int64_t before = 0;
    for (int r = 0; r < lr; ++r) {
      if (rs[r].max_score != M) continue;
      if (jstar <= before + rs[r].ties) { owner = r; break; }
      before += rs[r].ties;
    }
    int32_t winner = -1;
    if (owner == (lr > 1 ? c->rank : 0)) {
      HIP_TRY(c, launch_row_select(s.d_S.get(), len, M, jstar - before, c->n0, c->d_sel.get(), st));
    } else {
      HIP_TRY(c, hipMemsetAsync(c->d_sel.get(), 0xff, 4, st));
    }
    if (lr > 1) {
      std::vector<int32_t> w(lr);
      int rc = exchange_small(c, XSITE_SELECT, c->d_sel.get(), 4, w.data());
      if (rc) return rc;
      winner = w[owner];
    } else {
      HIP_TRY(c, hipMemcpyAsync(&winner, c->d_sel.get(), 4, hipMemcpyDeviceToHost, st));
      HIP_TRY(c, host_wait_stream(st));
    }
    if (winner < 0) return fail(c, GS_ESTATE, "exact path could not locate tie %lld", (long long)jstar);
    a.forced_node = winner;
    a.forced_score = M;
    a.forced_ties = T;
    a.forced_feasible = (int32_t)F;
    HIP_TRY(c, hipEventRecord(s.ev[3].get(), st));
    count_spec_launch(c, a);
    HIP_TRY(c, launch_commit(a, st));
    HIP_TRY(c, hipEventRecord(s.ev[4].get(), st));
    if (s.rep.any())   // (the first pass committed nothing: the counters are 0, and it wrote no table)
      if (int rc = launch_reports(c, s, b, st, st, false)) return rc;
    HIP_TRY(c, hipMemcpyAsync(h_committed, s.d_committed.get(), COMMITTED_BYTES, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, host_wait_stream(st));
    c->stats.commit_ms += ev_ms(s.ev[3].get(), s.ev[4].get());
    committed = h_committed[0];
    if (committed < 1) return fail(c, GS_ESTATE, "forced commit made no progress");
    HIP_TRY(c, hipMemcpyAsync(s.h_out, s.d_out, sizeof(PlacementDev) * committed, hipMemcpyDeviceToHost, st));
    if (s.rep.any())
      if (int rc = read_reports(c, s, committed, st)) return rc;
    HIP_TRY(c, host_wait_stream(st));
  }
  flush_exchange_times(c);
  if (committed < b) {
    c->stats.cuts += 1;
    static const bool dbg = env_on("GS_DEBUG_CUTS");
    if (dbg) {
      const PlacementDev& x = s.h_out[committed];
      fprintf(stderr, "gpuscore: batch of %d ended after %d pods (code %#x) [%d run %u M %lld Mc %lld Md %lld T %u Tc %d new %u old %u jp %lld nd %lld pend %lld]\n",
              b, committed, h_committed[2], x.node, x.feasible, (long long)(x.score & 0xfffff),
              (long long)((x.score >> 20) & 0xfffff), (long long)(x.score >> 40), x.ties, (int)x.flags, x.zkeys, x.pad,
              (long long)x.zcpu[0], (long long)x.zcpu[1], (long long)x.zcpu[2]);
      fprintf(stderr, "   old slot %lld node %llu hash %lld S %d dso %d\n", (long long)x.cpuset[0],
              (unsigned long long)x.cpuset[1], (long long)x.cpuset[2], (int)(x.cpuset[3] >> 32), (int)(int32_t)x.cpuset[3]);
    }
  }
  *committed_out = committed;
  return GS_OK;
}

// ---- Reservation + DeviceShare: one extension pod (gs_ext.hip) ------------------------------------------------

// GetPodDeviceRequests for the GPU type (deviceshare/utils.go:147-252): ValidateDeviceRequest + ConvertDeviceRequest.
// 0: ok (mask 0 = no GPU request), -1: invalid (PreFilter UnschedulableAndUnresolvable)
int gpu_request_of(const gs_pod_ext& e, int64_t req[3], uint32_t* mask) {
  req[0] = req[1] = req[2] = 0;
  *mask = 0;
  const uint32_t m = e.gpu_request_mask & 0x1Fu;
  if (!m) return 0;
  for (int n : {GS_GPU_NAME_KOORD_GPU, GS_GPU_NAME_CORE, GS_GPU_NAME_MEMORY_RATIO})   // ValidatePercentageResource
    if ((m >> n & 1u) && e.gpu_requests[n] > 100 && e.gpu_requests[n] % 100 != 0) return -1;
  const int64_t* q = e.gpu_requests;
  switch (m) {   // ValidDeviceResourceCombinations -> ResourceCombinationsMapper
    case 1u << GS_GPU_NAME_NVIDIA: req[0] = req[1] = q[GS_GPU_NAME_NVIDIA] * 100; *mask = 3; return 0;
    case 1u << GS_GPU_NAME_KOORD_GPU: req[0] = req[1] = q[GS_GPU_NAME_KOORD_GPU]; *mask = 3; return 0;
    case 1u << GS_GPU_NAME_MEMORY: req[2] = q[GS_GPU_NAME_MEMORY]; *mask = 4; return 0;
    case 1u << GS_GPU_NAME_MEMORY_RATIO: req[1] = q[GS_GPU_NAME_MEMORY_RATIO]; *mask = 2; return 0;
    case (1u << GS_GPU_NAME_CORE) | (1u << GS_GPU_NAME_MEMORY):
      req[0] = q[GS_GPU_NAME_CORE]; req[2] = q[GS_GPU_NAME_MEMORY]; *mask = 5; return 0;
    case (1u << GS_GPU_NAME_CORE) | (1u << GS_GPU_NAME_MEMORY_RATIO):
      req[0] = q[GS_GPU_NAME_CORE]; req[1] = q[GS_GPU_NAME_MEMORY_RATIO]; *mask = 3; return 0;
    default: return -1;
  }
}

// The HBM image of node i's Device object; a GPU's Topology.NodeID becomes a slot of the node's NUMA zones (the zone
// masks the topology manager merges), GZ_FOREIGN when it is none of them.
DevNode dev_image(const gs_ctx* c, uint32_t i) {
  const gs_node_devices& d = c->devs[i];
  const gs_node_numa* nn = c->numa_on ? &c->numa[i].cfg : nullptr;
  DevNode o{};
  o.has_device = d.has_device;
  o.num_gpus = d.has_device ? d.num_gpus : 0;
  for (int n = 0; n < GS_NUM_GPU_NAMES; ++n) o.fit_free[n] = d.allocatable[n] - d.requested[n];
  for (int x = 0; x < GS_MAX_XRES; ++x) o.fit_free[GS_NUM_GPU_NAMES + x] = d.xres_allocatable[x] - d.xres_requested[x];
  for (int g = 0; g < o.num_gpus; ++g) {
    o.g[g].minor = d.gpus[g].minor;
    o.g[g].has_info = d.gpus[g].has_info ? 1 : 0;
    o.g[g].zone = GZ_NONE;
    if (d.gpus[g].numa_node >= 0) {
      o.g[g].zone = GZ_FOREIGN;
      for (int z = 0; nn && z < nn->num_zones; ++z)
        if (nn->zones[z].node_id == d.gpus[g].numa_node) o.g[g].zone = (int16_t)z;
    }
    for (int r = 0; r < 3; ++r) {
      o.g[g].total[r] = d.gpus[g].total[r];
      o.g[g].free[r] = std::max<int64_t>(0, d.gpus[g].total[r] - d.gpus[g].used[r]);
    }
  }
  return o;
}

int ext_alloc(gs_ctx* c) {
  if (c->d_dev) return GS_OK;
  HIP_TRY(c, c->d_dev.alloc(sizeof(DevNode) * std::max<uint32_t>(1, c->N)));
  std::vector<DevNode> img(c->N);
  for (uint32_t i = 0; i < c->N; ++i) img[i] = dev_image(c, i);
  HIP_TRY(c, hipMemcpy(c->d_dev.get(), img.data(), sizeof(DevNode) * c->N, hipMemcpyHostToDevice));
  c->dev_dirty_list.clear();
  std::fill(c->dev_dirty.begin(), c->dev_dirty.end(), 0);
  HIP_TRY(c, c->d_xtot.alloc(4 * (size_t)c->ld));
  HIP_TRY(c, c->d_xT.alloc(4 * ext_select_scratch_words(c->ld)));
  HIP_TRY(c, c->d_xds.alloc(2 * (size_t)c->ld));
  HIP_TRY(c, c->d_xrs.alloc(2 * (size_t)c->ld));
  HIP_TRY(c, c->d_xout.alloc(sizeof(ExtOut)));
  HIP_TRY(c, c->h_xout.alloc(sizeof(ExtOut)));   // written by ext_finish_kernel
  return GS_OK;
}

// The extension pod's input block (pinned host + device, one H2D copy per pod) and the nomination arrays, for at
// least nrec matched records and nres matched reservations.
int ext_stage_reserve(gs_ctx* c, uint32_t nrec, uint32_t nres) {
  if (c->h_xin && nrec <= c->xrec_cap && nres <= c->xres_cap) return GS_OK;
  c->xrec_cap = std::max<uint32_t>({64, c->xrec_cap, nrec * 2});
  c->xres_cap = std::max<uint32_t>({64, c->xres_cap, nres * 2});
  auto al = [](size_t x) { return (x + 15) & ~(size_t)15; };
  const size_t off_pv = al(sizeof(ExtPod));
  c->xin_off_rec = off_pv + al(sizeof(PodVec));
  c->xin_off_res = c->xin_off_rec + al(sizeof(ExtRec) * c->xrec_cap);
  c->xin_bytes = c->xin_off_res + sizeof(ExtRes) * c->xres_cap;
  HIP_TRY(c, host_wait_stream(c->st.get()));
  HIP_TRY(c, c->h_xin.alloc(c->xin_bytes));   // (alloc() frees the old block: the wait above covers the four)
  HIP_TRY(c, c->d_xin.alloc(c->xin_bytes));
  HIP_TRY(c, c->d_xnom.alloc(4 * c->xrec_cap));
  HIP_TRY(c, c->h_xnom.alloc(4 * c->xrec_cap));   // written by ext_finish_kernel
  c->h_xpod = reinterpret_cast<ExtPod*>(c->h_xin.get());
  c->d_xpod = reinterpret_cast<ExtPod*>(c->d_xin.get());
  c->d_xpv = reinterpret_cast<PodVec*>(c->d_xin.get() + off_pv);
  c->d_xrec = reinterpret_cast<ExtRec*>(c->d_xin.get() + c->xin_off_rec);
  c->d_xres = reinterpret_cast<ExtRes*>(c->d_xin.get() + c->xin_off_res);
  return GS_OK;
}

// the dirty nodes' Device images: staged in pinned memory, one copy and one scatter per EXT_DEV_STAGE nodes
int ext_flush_devices(gs_ctx* c) {
  if (c->dev_dirty_list.empty()) return GS_OK;
  if (!c->d_dev) return ext_alloc(c);
  if (!c->h_dev_stage) {   // n images, then their node indices: one copy
    HIP_TRY(c, c->h_dev_stage.alloc((sizeof(DevNode) + 4) * EXT_DEV_STAGE));
    HIP_TRY(c, c->d_dev_stage.alloc((sizeof(DevNode) + 4) * EXT_DEV_STAGE));
  }
  DevNode *const h_stage = c->h_dev_stage.get(), *const d_stage = c->d_dev_stage.get();
  for (size_t done = 0; done < c->dev_dirty_list.size();) {
    const uint32_t n = (uint32_t)std::min<size_t>(EXT_DEV_STAGE, c->dev_dirty_list.size() - done);
    HIP_TRY(c, host_wait_stream(c->st.get()));   // the previous scatter has consumed the staging buffers
    uint32_t* h_idx = reinterpret_cast<uint32_t*>(h_stage + n);
    for (uint32_t j = 0; j < n; ++j) {
      const uint32_t i = c->dev_dirty_list[done + j];
      h_stage[j] = dev_image(c, i);
      h_idx[j] = i;
      c->dev_dirty[i] = 0;
    }
    HIP_TRY(c, hipMemcpyAsync(d_stage, h_stage, (sizeof(DevNode) + 4) * n, hipMemcpyHostToDevice, c->st.get()));
    HIP_TRY(c, launch_scatter_devnodes(c->d_dev.get(), reinterpret_cast<const uint32_t*>(d_stage + n), d_stage, n,
                                       c->st.get()));
    done += n;
  }
  c->dev_dirty_list.clear();
  return GS_OK;
}

void dev_mark(gs_ctx* c, uint32_t i) {
  if (!c->dev_dirty[i]) { c->dev_dirty[i] = 1; c->dev_dirty_list.push_back(i); }
}

// ---- RDMA / FPGA devices: the table beside c->devs, its HBM image beside d_dev
DevAuxNode aux_image(const gs_ctx* c, uint32_t i) {
  DevAuxNode o{};
  if (c->aux.empty()) return o;
  const gs_node_aux_devices& a = c->aux[i];
  for (int T = 0; T < GS_NUM_AUX_TYPES; ++T) {
    o.num[T] = std::min<int32_t>(a.num[T], GS_MAX_AUX_DEVICES);
    for (int k = 0; k < o.num[T]; ++k) {
      o.d[T][k].total = a.dev[T][k].total;
      o.d[T][k].free = std::max<int64_t>(0, a.dev[T][k].total - a.dev[T][k].used);
      o.d[T][k].minor = a.dev[T][k].minor;
      o.d[T][k].has_info = a.dev[T][k].has_info ? 1 : 0;
    }
  }
  return o;
}

void aux_mark(gs_ctx* c, uint32_t i) {
  if (!c->d_aux) return;   // (ext_aux_alloc uploads every row)
  if (c->aux_dirty.empty()) c->aux_dirty.assign(c->N, 0);
  if (!c->aux_dirty[i]) { c->aux_dirty[i] = 1; c->aux_dirty_list.push_back(i); }
}

int ext_aux_alloc(gs_ctx* c) {
  if (c->d_aux) return GS_OK;
  HIP_TRY(c, c->d_aux.alloc(sizeof(DevAuxNode) * std::max<uint32_t>(1, c->N)));
  std::vector<DevAuxNode> img(c->N);
  for (uint32_t i = 0; i < c->N; ++i) img[i] = aux_image(c, i);
  HIP_TRY(c, hipMemcpy(c->d_aux.get(), img.data(), sizeof(DevAuxNode) * c->N, hipMemcpyHostToDevice));
  c->aux_dirty_list.clear();
  std::fill(c->aux_dirty.begin(), c->aux_dirty.end(), 0);
  return GS_OK;
}

// the dirty nodes' aux images, staged like the Device images (ext_flush_devices)
int ext_flush_aux(gs_ctx* c) {
  if (c->aux_dirty_list.empty() || !c->d_aux) return GS_OK;
  if (!c->h_aux_stage) {
    HIP_TRY(c, c->h_aux_stage.alloc((sizeof(DevAuxNode) + 4) * EXT_DEV_STAGE));
    HIP_TRY(c, c->d_aux_stage.alloc((sizeof(DevAuxNode) + 4) * EXT_DEV_STAGE));
  }
  DevAuxNode *const h_stage = c->h_aux_stage.get(), *const d_stage = c->d_aux_stage.get();
  for (size_t done = 0; done < c->aux_dirty_list.size();) {
    const uint32_t n = (uint32_t)std::min<size_t>(EXT_DEV_STAGE, c->aux_dirty_list.size() - done);
    HIP_TRY(c, host_wait_stream(c->st.get()));   // the previous scatter has consumed the staging buffers
    uint32_t* h_idx = reinterpret_cast<uint32_t*>(h_stage + n);
    for (uint32_t j = 0; j < n; ++j) {
      const uint32_t i = c->aux_dirty_list[done + j];
      h_stage[j] = aux_image(c, i);
      h_idx[j] = i;
      c->aux_dirty[i] = 0;
    }
    HIP_TRY(c, hipMemcpyAsync(d_stage, h_stage, (sizeof(DevAuxNode) + 4) * n, hipMemcpyHostToDevice, c->st.get()));
    HIP_TRY(c, launch_scatter_auxnodes(c->d_aux.get(), reinterpret_cast<const uint32_t*>(d_stage + n), d_stage, n,
                                       c->st.get()));
    done += n;
  }
  c->aux_dirty_list.clear();
  return GS_OK;
}

// DefaultDeviceHandler.CalcDesiredRequestsAndCount (devicehandler_default.go:44-93) for q > 0 on a node listing n
// devices of the type
void aux_desired(int64_t q, int32_t strategy, int32_t exclusive, int n, int64_t* inst, int64_t* count) {
  *inst = q;
  *count = 1;
  if (q > 100 && q % 100 == 0) { *count = q / 100; *inst = 100; }
  else if (strategy == GS_AUX_APPLY_FOR_ALL) *count = n;
  else if (strategy == GS_AUX_REQUESTS_AS_COUNT) { *count = q; *inst = exclusive ? 100 : 1; }
}

// DeviceShare Reserve of one RDMA / FPGA type on one node's row (plugin.go:377-430 -> defaultAllocateDevices,
// device_allocator.go:397-467): the minors by scoreDevice (scoring.go:186-211) descending, then minor ascending
// (device_resources.go:171-208); exactly count of them get used += inst. false: fewer than count usable devices
bool aux_reserve_row(gs_node_aux_devices* a, int T, int64_t q, int32_t strategy, int32_t exclusive, int64_t weight,
                     bool most, gs_aux_placement* ao) {
  const int n = a->num[T];
  if (n <= 0) return false;
  int64_t inst, count;
  aux_desired(q, strategy, exclusive, n, &inst, &count);
  struct Cand { int k; int64_t score; };
  std::vector<Cand> cs;
  bool all_zero = true;
  for (int k = 0; k < n; ++k) all_zero &= a->dev[T][k].total <= a->dev[T][k].used;
  if (all_zero) return false;
  for (int k = 0; k < n; ++k) {
    const gs_aux_device& x = a->dev[T][k];
    if (!x.has_info) continue;
    const int64_t t = x.total, f = std::max<int64_t>(0, x.total - x.used);
    int64_t sc = 0;
    if (weight && t != 0) {
      int64_t rq = t;
      if (t >= f) rq = t - f + inst;
      sc = most ? (std::min(rq, t) * 100) / t : (rq > t ? 0 : ((t - rq) * 100) / t);
    }
    cs.push_back({k, sc});
  }
  std::stable_sort(cs.begin(), cs.end(), [&](const Cand& x, const Cand& y) {
    if (x.score != y.score) return x.score > y.score;
    return a->dev[T][x.k].minor < a->dev[T][y.k].minor;
  });
  std::vector<int> take;
  for (const Cand& x : cs) {
    const gs_aux_device& dv = a->dev[T][x.k];
    const int64_t f = std::max<int64_t>(0, dv.total - dv.used);
    if (f == 0 || inst > f) continue;
    take.push_back(x.k);
    if ((int64_t)take.size() == count) break;
  }
  if ((int64_t)take.size() < count) return false;
  for (int k : take) {
    a->dev[T][k].used += inst;
    ao->minor_mask[T] |= 1u << (a->dev[T][k].minor & 31);
  }
  ao->count[T] = (int32_t)count;
  ao->per_instance[T] = inst;
  return true;
}

// DeviceShare Unreserve of the recorded RDMA / FPGA minors (updateCacheUsed(..., false), device_cache.go:124-201):
// SubtractWithNonNegativeResult on the minors the row still has
void aux_unreserve_row(gs_node_aux_devices* a, const gs_aux_placement& x) {
  for (int T = 0; T < GS_NUM_AUX_TYPES; ++T) {
    if (!x.minor_mask[T]) continue;
    for (int k = 0; k < a->num[T] && k < GS_MAX_AUX_DEVICES; ++k) {
      gs_aux_device& dv = a->dev[T][k];
      if (dv.minor < 0 || dv.minor > 31 || !(x.minor_mask[T] >> dv.minor & 1u)) continue;
      dv.used = std::max<int64_t>(0, dv.used - x.per_instance[T]);
    }
  }
}

// DeviceShare Unreserve of recorded GPU minors: SubtractWithNonNegativeResult on the minors the Device row still has
void gpu_unreserve_row(gs_node_devices* d, uint32_t minor_mask, uint32_t keys, const int64_t inst[GS_NUM_GPU_RES]) {
  for (int g = 0; g < d->num_gpus; ++g) {
    if (d->gpus[g].minor < 0 || d->gpus[g].minor > 31 || !(minor_mask >> d->gpus[g].minor & 1u)) continue;
    for (int r = 0; r < GS_NUM_GPU_RES; ++r)
      if (keys >> r & 1u) d->gpus[g].used[r] = std::max<int64_t>(0, d->gpus[g].used[r] - inst[r]);
  }
}

// the pod's matched reservations grouped by node (node order, uid order within a node)
void matched_of(const gs_ctx* c, uint64_t owner, std::vector<std::pair<uint32_t, uint64_t>>* out) {
  out->clear();
  if (!owner || !(c->ext.enabled & GS_EXT_RESERVATION)) return;
  auto it = c->rsv_owner.find(owner);
  if (it == c->rsv_owner.end()) return;
  for (uint64_t uid : it->second) {
    const gs_reservation& r = c->rsv.at(uid);
    if (rsv_matches(r, owner)) out->push_back({r.node, uid});
  }
  std::sort(out->begin(), out->end());
}

bool is_ext_pod(const gs_ctx* c, const gs_pod_ext& e, const gs_pod_aux* ax = nullptr) {
  if (ax && (c->ext.enabled & GS_EXT_DEVICESHARE))   // an RDMA / FPGA request
    for (int T = 0; T < GS_NUM_AUX_TYPES; ++T)
      if (ax->request[T]) return true;
  if (e.xres_request_mask & ((1u << GS_MAX_XRES) - 1u)) return true;   // Fit over a registered extended resource
  if ((c->ext.enabled & GS_EXT_DEVICESHARE) && (e.gpu_request_mask & 0x1Fu)) return true;
  if (!(c->ext.enabled & GS_EXT_RESERVATION)) return false;
  if (e.reservation_required) return true;
  std::vector<std::pair<uint32_t, uint64_t>> m;
  matched_of(c, e.reservation_owner, &m);
  return !m.empty();
}

// DeviceShare Reserve (deviceshare/plugin.go:377-430) on the host mirror: defaultAllocateDevices with the scorer
// (device_allocator.go:397-467; minors by device score descending, then minor), within the node's NUMA affinity
// (aff: 0x10 | zone-slot mask, 0 = none; device_allocator.go:148-152)
int ext_device_reserve(gs_ctx* c, uint32_t node, const int64_t preq[3], uint32_t pmask, gs_ext_placement* eo,
                       uint32_t aff, uint32_t* keys) {
  gs_node_devices& d = c->devs[node];
  *keys = 0;
  if (!d.has_device) return GS_OK;
  const DevNode img = dev_image(c, node);
  int64_t total_mem = -1;
  for (int g = 0; g < img.num_gpus; ++g)
    if (img.g[g].total[0] | img.g[g].total[1] | img.g[g].total[2]) { total_mem = img.g[g].total[2]; break; }
  if (img.num_gpus <= 0 || total_mem < 0) return fail(c, GS_ESTATE, "DeviceShare Reserve: no GPU on node %u", node);
  int64_t core = preq[0], ratio = preq[1], mem = preq[2];
  if (pmask & 4u) ratio = (int64_t)((double)mem / (double)total_mem * 100.0);
  else mem = ratio * total_mem / 100;
  uint32_t m = pmask | 6u;
  int64_t count = 1;
  if (ratio > 100 && ratio % 100 == 0) { count = ratio / 100; core /= count; mem /= count; ratio /= count; m = 7u; }
  const int64_t inst[3] = {core, ratio, mem};
  struct Cand { int g; int64_t score; };
  std::vector<Cand> cs;
  for (int g = 0; g < img.num_gpus; ++g) {
    if (!img.g[g].has_info) continue;
    if ((aff & 0x10u) && (img.g[g].zone < 0 || !(aff >> img.g[g].zone & 1u))) continue;
    int64_t ns = 0, ws = 0;   // scoreDevice (deviceshare/scoring.go:186-211)
    for (int r = 0; r < 3; ++r) {
      const int64_t w = c->ext.device_weights[r], t = img.g[g].total[r], f = img.g[g].free[r];
      if (!w || t == 0) continue;
      int64_t rq = t;
      if (t >= f) rq = t - f + ((m >> r & 1u) ? inst[r] : 0);
      int64_t sc;
      if (c->ext.device_scoring_type == GS_SCORING_MOST_ALLOCATED) sc = (std::min(rq, t) * 100) / t;
      else sc = rq > t ? 0 : ((t - rq) * 100) / t;
      ns += sc * w;
      ws += w;
    }
    cs.push_back({g, ws ? ns / ws : 0});
  }
  std::stable_sort(cs.begin(), cs.end(), [&](const Cand& a, const Cand& b) {
    if (a.score != b.score) return a.score > b.score;
    return img.g[a.g].minor < img.g[b.g].minor;
  });
  std::vector<int> take;
  for (const Cand& x : cs) {
    const DevGpu& g = img.g[x.g];
    if (!(g.free[0] | g.free[1] | g.free[2])) continue;
    bool ok = true;
    for (int r = 0; r < 3; ++r) ok &= !(m >> r & 1u) || inst[r] <= g.free[r];
    if (!ok) continue;
    take.push_back(x.g);
    if ((int64_t)take.size() == count) break;
  }
  if ((int64_t)take.size() < count)
    return fail(c, GS_ESTATE, "DeviceShare Reserve: allocation failed on node %u after a feasible Filter", node);
  for (int g : take) {
    for (int r = 0; r < 3; ++r)
      if (m >> r & 1u) d.gpus[g].used[r] += inst[r];
    eo->gpu_minor_mask |= 1u << (d.gpus[g].minor & 31);
  }
  eo->gpu_count = (int32_t)count;
  for (int r = 0; r < 3; ++r) eo->gpu_per_instance[r] = (m >> r & 1u) ? inst[r] : 0;
  *keys = m & 7u;
  dev_mark(c, node);
  return GS_OK;
}

// What the device chain of one extension pod (ext_chain) leaves behind: for the pod's Reserve (ext_schedule_one) and
// for its per-node view (gs_debug_ext_rows). The result itself is in c->h_xout / c->h_xnom, the matched records in
// c->xrec / c->xres_uid.
struct ExtChain {
  bool early = false;       // PreFilter ended the pod before any launch (fail_code: DeviceShare's, 0: Reservation's)
  uint32_t fail_code = 0;
  bool rs_on = false;
  int64_t greq[3] = {0, 0, 0};
  uint32_t gmask = 0, gpu_names_all = 0, xres_all = 0;
  uint32_t amask = 0;       // RDMA / FPGA types the pod requests
  PodVec v{};
  int nrec = 0;
  Slot* sl = nullptr;
  bool ext_ev = false;
  std::chrono::steady_clock::time_point t0, t_done;
};

// scheduleOne of one extension pod up to selectHost: eval pass (B = 1) -> ext_nodes -> ext_numa -> ext_matched ->
// ext_select -> ext_finish, and the wait for the stream. No host or device state of the cluster changes here.
int ext_chain(gs_ctx* c, const gs_pod& pod, const gs_pod_ext& e, const gs_pod_aux* ax, uint64_t seq, ExtChain* ch) {
  // several ranks: with the score-row exchange every rank holds every node's state and runs the one-GPU pipeline, so an
  // extension pod runs whole on every rank (no exchange: the same inputs give the same placement everywhere); the
  // level exchange's ranks hold their shard's rows only
  if ((c->nranks > 1 && !c->sgather) || c->window_k)
    return fail(c, GS_EUNSUPPORTED, "Reservation / DeviceShare pods need one rank (or the score-row exchange) and no "
                "node sampling");
  const bool ds_on = c->ext.enabled & GS_EXT_DEVICESHARE, rs_on = c->ext.enabled & GS_EXT_RESERVATION;
  int64_t* const greq = ch->greq;
  uint32_t& gmask = ch->gmask;
  ch->rs_on = rs_on;
  // RDMA / FPGA requests (GetPodDeviceRequests, utils.go:232-252): what is not restated is refused first
  uint32_t& amask = ch->amask;
  amask = 0;
  for (int T = 0; ax && ds_on && T < GS_NUM_AUX_TYPES; ++T) {
    if (!ax->request[T]) continue;
    if (ax->request[T] < 0 || ax->request[T] >= (1LL << 53))
      return fail(c, GS_EUNSUPPORTED, "RDMA / FPGA request outside [0, 2^53)");
    if (ax->strategy[T] < GS_AUX_STRATEGY_NONE || ax->strategy[T] > GS_AUX_REQUESTS_AS_COUNT)
      return fail(c, GS_EINVAL, "unknown device allocate strategy %d", ax->strategy[T]);
    amask |= 1u << T;
  }
  if (amask && (e.reservation_owner || e.reservation_required))
    return fail(c, GS_EUNSUPPORTED, "a pod requesting RDMA / FPGA devices with a reservation owner or a required "
                "reservation is not supported");
  if (amask && c->numa_on)
    for (uint32_t n = 0; n < c->N; ++n)
      if (c->numa[n].cfg.numa_topology_policy != GS_NUMA_POLICY_NONE)
        return fail(c, GS_EUNSUPPORTED, "a pod requesting RDMA / FPGA devices while node %u has a NUMA topology policy "
                    "is not supported (DeviceShare hints for several device types)", n);
  for (int T = 0; T < GS_NUM_AUX_TYPES; ++T)   // ValidatePercentageResource (utils.go:84-90), whatever the strategy
    if ((amask >> T & 1u) && ax->request[T] > 100 && ax->request[T] % 100 != 0) {
      ch->early = true;
      ch->fail_code = GS_EXT_FAIL_POD;
      return GS_OK;
    }
  if (ds_on && gpu_request_of(e, greq, &gmask) < 0) {   // DeviceShare PreFilter: UnschedulableAndUnresolvable
    ch->early = true;
    ch->fail_code = GS_EXT_FAIL_POD;
    return GS_OK;
  }
  if (!ds_on) { greq[0] = greq[1] = greq[2] = 0; gmask = 0; }
  std::vector<std::pair<uint32_t, uint64_t>> matched;
  if (rs_on) matched_of(c, e.reservation_owner, &matched);
  for (int x = 0; x < GS_MAX_XRES; ++x)
    if (e.xres_requests[x] < 0 || !in_range(e.xres_requests[x]))
      return fail(c, GS_EUNSUPPORTED, "extended resource request outside [0, 2^53)");
  PodVec& v = ch->v;
  v = prep_pod(c, pod);
  if (rs_on && e.reservation_required && matched.empty()) {   // PreFilter: ErrReasonReservationAffinity
    ch->early = true;
    return GS_OK;
  }
  int rc;
  using hx_clk = std::chrono::steady_clock;
  const auto hx0 = hx_clk::now();
  if ((rc = ext_alloc(c))) return rc;
  if ((rc = ext_flush_devices(c))) return rc;
  if (amask && ((rc = ext_aux_alloc(c)) || (rc = ext_flush_aux(c)))) return rc;
  if ((rc = flush_rows(c))) return rc;
  if (c->prep_stale && (rc = node_prep(c))) return rc;
  const auto hx1 = hx_clk::now();
  // ---- BeforePreFilter: per-node restore records (reservation/transformer.go:50-235)
  c->xrec.clear();
  c->xres.clear();
  c->xres_uid.clear();
  for (size_t a = 0; a < matched.size();) {
    const uint32_t node = matched[a].first;
    size_t b = a;
    while (b < matched.size() && matched[b].first == node) ++b;
    if (b - a > (size_t)EXT_MAX_RES_PER_NODE)
      return fail(c, GS_EUNSUPPORTED, "more than %d matched reservations on node %u", EXT_MAX_RES_PER_NODE, node);
    ExtRec rec{};
    rec.node = node;
    rec.nres = (int32_t)(b - a);
    rec.first = (int32_t)c->xres.size();
    rec.dpods = rec.nres;
    rec.order_min = INT64_MAX;
    const gs_node mirror = reservation_view(c, node, 0);
    const gs_node podreq = reservation_view(c, node, e.reservation_owner);
    for (int s = 0; s < 7; ++s) {
      rec.pod_requested[s] = podreq.requested[s];
      rec.allocatable[s] = podreq.allocatable[s];
    }
    gs_node restored = podreq;
    for (size_t k = a; k < b; ++k) {
      const gs_reservation& r = c->rsv.at(matched[k].second);
      if (c->numa_on && (v.numa & PN_BIND)) {
        // NodeNUMAResource's reservation restore (nodenumaresource/reservation.go:76-113, plugin.go:488-549) hands a
        // cpuset pod the reservation's remaining CPUs (preferredCPUs, reusableResources): not restated. It applies only
        // when the reservation itself holds a cpuset allocation; without one the restore is empty
        auto it = c->numa[node].pods.find(r.uid);
        if (it != c->numa[node].pods.end() && !it->second.cpus.empty())
          return fail(c, GS_EUNSUPPORTED, "a cpuset pod matching reservation %llu, which holds a cpuset on node %u, is "
                      "not on the device path", (unsigned long long)r.uid, node);
      }
      rsv_request_delta(r.allocatable, r.allocatable_mask, -1, restored.requested, restored.nonzero_requested);
      ExtRes x{};
      int64_t rem[GS_NUM_RES];
      (void)rsv_remained(r, rem);
      for (int s = 0; s < 7; ++s) {
        x.alloc[s] = (r.allocatable_mask >> s & 1u) ? r.allocatable[s] : 0;
        x.allocated[s] = (r.allocated_mask >> s & 1u) ? r.allocated[s] : 0;
        rec.r_allocated[s] += x.allocated[s];
        // SubtractWithNonNegativeResult(Allocatable, Mask(Allocated, ResourceNames)) (Restricted policy)
        const int64_t am = (r.resource_names_mask >> s & 1u) ? x.allocated[s] : 0;
        x.remained_nn[s] = std::max<int64_t>(0, x.alloc[s] - am);
      }
      x.order = r.order;
      x.alloc_mask = r.allocatable_mask;
      x.allocated_mask = r.allocated_mask;
      x.names = r.resource_names_mask;
      x.policy = r.allocate_policy;
      x.skip = (r.allocate_once && r.assigned_pods > 0) ? 1 : 0;
      if (r.order != 0 && rec.order_min > r.order) rec.order_min = r.order;
      c->xres.push_back(x);
      c->xres_uid.push_back(r.uid);
    }
    for (int s = 0; s < 7; ++s) rec.dfree[s] = mirror.requested[s] - restored.requested[s];
    rec.dnz[0] = mirror.nonzero_requested[0] - restored.nonzero_requested[0];
    rec.dnz[1] = mirror.nonzero_requested[1] - restored.nonzero_requested[1];
    rec.restored_pods = podreq.pod_count - rec.nres;
    rec.allowed_pods = podreq.allowed_pod_number;
    c->xrec.push_back(rec);
    a = b;
  }
  const int nrec = ch->nrec = (int)c->xrec.size();
  if ((rc = ext_stage_reserve(c, (uint32_t)nrec, (uint32_t)c->xres.size()))) return rc;
  ExtPod& xp = *c->h_xpod;
  xp = ExtPod{};
  for (int r = 0; r < 3; ++r) { xp.gpu_req[r] = greq[r]; xp.dev_w[r] = c->ext.device_weights[r]; }
  xp.gpu_mask = gmask;
  // NodeInfo.AddPod adds them all
  const uint32_t gpu_names_all = ch->gpu_names_all = gmask ? (e.gpu_request_mask & 0x1Fu) : 0u;
  // Fit checks the non-ignored ones ([upstream] fit.go fitsRequest), and only as NodeResourcesFit's Filter: none
  // with that Filter off
  const bool fit_filter = c->cfg.enabled & GS_ENABLE_FIT_FILTER;
  xp.gpu_names = fit_filter ? gpu_names_all & ~c->ext.fit_ignored_gpu_names : 0u;
  for (int n = 0; n < GS_NUM_GPU_NAMES; ++n) xp.gpu_name_req[n] = (xp.gpu_names >> n & 1u) ? e.gpu_requests[n] : 0;
  const uint32_t xres_all = ch->xres_all = e.xres_request_mask & ((1u << GS_MAX_XRES) - 1u);
  const uint32_t xres_fit = fit_filter ? xres_all & ~c->ext.fit_ignored_xres : 0u;
  xp.gpu_names |= xres_fit << GS_NUM_GPU_NAMES;
  for (int x = 0; x < GS_MAX_XRES; ++x)
    xp.gpu_name_req[GS_NUM_GPU_NAMES + x] = (xres_fit >> x & 1u) ? e.xres_requests[x] : 0;
  xp.w_ds = c->ext.weight_deviceshare;
  xp.w_rs = c->ext.weight_reservation;
  for (int s = 0; s < 7; ++s) xp.pod_req[s] = pod.requests[s];
  xp.pod_mask = pod.request_mask & 0x7Fu;
  xp.required = rs_on && e.reservation_required;
  xp.nrec = nrec;
  xp.ds_on = ds_on;
  xp.rs_on = rs_on;
  xp.dev_most = c->ext.device_scoring_type == GS_SCORING_MOST_ALLOCATED;
  xp.seq = seq;
  xp.aux_mask = amask;
  for (int T = 0; T < GS_NUM_AUX_TYPES; ++T)
    if (amask >> T & 1u) {
      xp.aux_req[T] = ax->request[T];
      xp.aux_strategy[T] = ax->strategy[T];
      xp.aux_excl[T] = ax->device_exclusive[T] ? 1 : 0;
      xp.aux_w[T] = c->aux_weights[T];
    }
  // GPU names are scalar requests: the Fit filter's all-zero short cut no longer applies
  if (gpu_names_all || xres_all) v.flags &= ~PF_ALL_ZERO;
  *reinterpret_cast<PodVec*>(c->h_xin.get() + ((sizeof(ExtPod) + 15) & ~(size_t)15)) = v;
  // the NUMA-policy work list over [n0, n1) for the eval pass and ext_numa_kernel (launch_batch's list is the shard's)
  if (c->numa_on && c->xnuma_stale) {
    std::vector<uint32_t> idx;
    for (uint32_t n = c->n0; n < c->n1; ++n)
      if (c->numa[n].cfg.numa_topology_policy != GS_NUMA_POLICY_NONE) idx.push_back(n);
    HIP_TRY(c, host_wait_stream(c->st.get()));
    c->d_xnuma_idx.reset();
    c->xnuma_n = (uint32_t)idx.size();
    if (c->xnuma_n) {
      HIP_TRY(c, c->d_xnuma_idx.alloc(4 * idx.size()));
      HIP_TRY(c, hipMemcpy(c->d_xnuma_idx.get(), idx.data(), 4 * idx.size(), hipMemcpyHostToDevice));
    }
    c->xnuma_stale = false;
  }
  const int prod_cols = (v.flags & PF_PROD_SCORE) ? 1 : 0;
  // no batch is in flight: the current slot's score rows, affinities and timing events serve this pod
  Slot& sl = current_slot(c);
  int16_t* const d_S = sl.d_S.get();
  uint8_t* const d_aff = sl.d_aff.get();
  const hipStream_t st = c->st.get();
  DevNode* const d_dev = c->d_dev.get();
  int32_t *const d_xtot = c->d_xtot.get(), *const d_xT = c->d_xT.get(), *const d_xnom = c->d_xnom.get();
  int16_t *const d_xds = c->d_xds.get(), *const d_xrs = c->d_xrs.get();
  // inputs: one copy of the staged block (ExtPod, PodVec, the matched records and reservations)
  if (nrec) {
    std::memcpy(c->h_xin.get() + c->xin_off_rec, c->xrec.data(), sizeof(ExtRec) * nrec);
    std::memcpy(c->h_xin.get() + c->xin_off_res, c->xres.data(), sizeof(ExtRes) * c->xres.size());
  }
  const size_t in_bytes = nrec ? c->xin_off_res + sizeof(ExtRes) * c->xres.size() : c->xin_off_rec;
  // no event markers inside the chain (each one holds the next dispatch for microseconds): the pass is timed on the
  // host, from the input copy's enqueue to the end of the stream synchronisation (GS_EXT_EVENTS=1: per-kernel events)
  static const bool ext_ev = env_on("GS_EXT_EVENTS");
  const auto ext_t0 = std::chrono::steady_clock::now();
  HIP_TRY(c, hipMemcpyAsync(c->d_xin.get(), c->h_xin.get(), in_bytes, hipMemcpyHostToDevice, st));
  if (ext_ev) HIP_TRY(c, hipEventRecord(sl.ev[0].get(), st));
  HIP_TRY(c, launch_eval(c->mv, c->d_xpv, 1, c->pf, c->n0, c->n1, d_S, c->ld, prod_cols, c->d_xnuma_idx.get(),
                         c->xnuma_n, d_aff, st));
  if (ext_ev) HIP_TRY(c, hipEventRecord(sl.ev[1].get(), st));
  // (ext_nodes_kernel also resets the select accumulators; ext_matched runs for pods with matched reservations only)
  // (the refusals above keep an RDMA / FPGA pod away from ext_numa_kernel and ext_matched_kernel, which do not read the
  // aux image)
  if (amask && (nrec || (c->numa_on && c->xnuma_n)))
    return fail(c, GS_ESTATE, "an RDMA / FPGA pod reached the matched-reservation or NUMA-policy kernels");
  HIP_TRY(c, launch_ext_nodes(d_dev, amask ? c->d_aux.get() : nullptr, d_S, c->n0, c->n1, c->d_xpod, d_xtot, d_xds, d_xrs,
                              d_xT, st));
  // GPU pods on NUMA-policy nodes: DeviceShare is the topology manager's second hint provider
  if (gmask && c->numa_on && c->xnuma_n)
    HIP_TRY(c, launch_ext_numa(c->mv, c->d_xpv, c->pf, prod_cols, d_dev, c->d_xpod, c->d_xnuma_idx.get(), c->xnuma_n,
                               c->n0, d_xtot, d_xds, d_aff, d_xT, c->n1 - c->n0, st));
  // the matched nodes last: their restored rows over the whole Filter chain (incl. the policy nodes' affinity)
  if (nrec)
    HIP_TRY(c, launch_ext_matched(c->mv, c->d_xpv, c->pf, prod_cols, d_dev, c->d_xpod, c->d_xrec, c->d_xres, nrec,
                                  d_xtot, d_xds, d_xrs, d_xnom, d_aff, c->n0, d_xT, c->n1 - c->n0, st));
  HIP_TRY(c, launch_ext_select(d_xtot, d_xds, d_xrs, c->d_xrec, c->n0, c->n1, c->d_xpod, c->cfg.seed, d_xT,
                               c->d_xout.get(), st));
  // outputs: the NodeNUMAResource Reserve of the selected node along its affinity, and the result and nominations
  // written straight into pinned host memory (no copy)
  HIP_TRY(c, launch_ext_finish(c->mv, c->d_xpv, c->pf, prod_cols, d_aff, c->n0, c->numa_on ? 1 : 0, c->d_xout.get(),
                               d_xnom, nrec, c->h_xout.get(), c->h_xnom.get(), st));
  if (ext_ev) HIP_TRY(c, hipEventRecord(sl.ev[4].get(), st));
  HIP_TRY(c, host_wait_stream(st));
  const auto hx3 = hx_clk::now();
  if (c->host_timing) {
    const auto us = [](hx_clk::duration d) { return std::chrono::duration<double, std::micro>(d).count(); };
    c->hx_flush += us(hx1 - hx0);
    c->hx_prep += us(ext_t0 - hx1);
    c->hx_gpu += us(hx3 - ext_t0);
    c->hx_pods += 1;
  }
  ch->sl = &sl;
  ch->ext_ev = ext_ev;
  ch->t0 = ext_t0;
  ch->t_done = hx3;
  return GS_OK;
}

// scheduleOne of one extension pod: the device chain (ext_chain), then the Reserve of NodeNUMAResource (no-op on the
// supported nodes), DeviceShare and Reservation, and assume.
int ext_schedule_one(gs_ctx* c, const gs_pod& pod, const gs_pod_ext& e, const gs_pod_aux* ax, uint64_t seq,
                     gs_placement* out, gs_ext_placement* eo, gs_aux_placement* ao) {
  *out = gs_placement{-1, 0, 0, 0, 0};
  *eo = gs_ext_placement{};
  *ao = gs_aux_placement{};
  ExtChain ch;
  int rc;
  if ((rc = ext_chain(c, pod, e, ax, seq, &ch))) return rc;
  if (ch.early) {
    eo->fail_code = ch.fail_code;
    c->stats.pods += 1;
    return GS_OK;
  }
  using hx_clk = std::chrono::steady_clock;
  const bool rs_on = ch.rs_on;
  const int64_t* const greq = ch.greq;
  const uint32_t gmask = ch.gmask, gpu_names_all = ch.gpu_names_all, xres_all = ch.xres_all;
  const PodVec& v = ch.v;
  const auto hx3 = ch.t_done;
  if (ch.ext_ev) {
    Slot& sl = *ch.sl;
    c->stats.eval_ms += ev_ms(sl.ev[0].get(), sl.ev[1].get());
    c->stats.commit_ms += ev_ms(sl.ev[1].get(), sl.ev[4].get());
  } else {
    c->stats.commit_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - ch.t0).count();
  }
  c->stats.eval_launches += 1;
  c->stats.eval_pairs += c->n1 - c->n0;
  c->stats.batches += 1;
  c->stats.pods += 1;
  const ExtOut xo = *c->h_xout.get();
  const int32_t* h_xnom = c->h_xnom.get();   // (the nominations ext_finish_kernel wrote)
  if (xo.err & 1u)
    return fail(c, GS_EUNSUPPORTED, "a GPU's NUMA node is not one of its node's NUMA zones (DeviceShare hints)");
  if (xo.err & 2u)
    return fail(c, GS_EUNSUPPORTED, "the topology-manager merge of a GPU pod exceeds its permutation bound");
  out->feasible = xo.feasible;
  if (xo.node < 0) return GS_OK;
  out->node = xo.node;
  out->score = xo.score;
  out->ties = xo.ties;
  eo->deviceshare_score = xo.ds_norm;
  eo->reservation_score = xo.rs_norm;
  const uint32_t node = (uint32_t)xo.node;
  // ---- Reserve: NodeNUMAResource (the zones the device allocated along the affinity), DeviceShare, Reservation
  if (c->numa_on) {
    PlacementDev pd{};
    pd.node = xo.node;
    pd.flags = xo.nflags;
    pd.zkeys = xo.zkeys;
    for (int z = 0; z < 4; ++z) { pd.zcpu[z] = xo.zcpu[z]; pd.zmem[z] = xo.zmem[z]; }
    if ((rc = numa_reserve(c, pod, v, pd))) return rc;
    out->flags = xo.nflags & ~PL_INTERNAL_FLAGS;
  }
  ExtReserved done{};   // what the Reserves below apply
  done.node = node;
  // the reference runs every plugin's Unreserve on a Reserve failure: NodeNUMAResource's allocation goes again
  const auto undo_numa = [&]() {
    if (c->numa_on && c->numa_uid_node.count(pod.uid)) {
      numa_release(c->numa[node], pod.uid);
      c->numa_uid_node.erase(pod.uid);
      mark_dirty(c, node);
    }
  };
  if (gmask && (rc = ext_device_reserve(c, node, greq, gmask, eo, xo.aff, &done.gpu_keys))) {
    undo_numa();
    return rc;
  }
  // the RDMA / FPGA types after the GPU type (a node without a Device object allocates nothing, as for GPUs)
  if (ch.amask && c->devs[node].has_device) {
    gs_node_aux_devices row = c->aux.empty() ? gs_node_aux_devices{} : c->aux[node];   // (applied only when every type fits)
    bool ok = true;
    for (int T = 0; ok && T < GS_NUM_AUX_TYPES; ++T)
      if (ch.amask >> T & 1u)
        ok = aux_reserve_row(&row, T, ax->request[T], ax->strategy[T], ax->device_exclusive[T] ? 1 : 0, c->aux_weights[T],
                             c->ext.device_scoring_type == GS_SCORING_MOST_ALLOCATED, ao);
    if (!ok) {   // ... and the GPU minors just reserved
      gpu_unreserve_row(&c->devs[node], eo->gpu_minor_mask, done.gpu_keys, eo->gpu_per_instance);
      dev_mark(c, node);
      undo_numa();
      return fail(c, GS_ESTATE, "DeviceShare Reserve: RDMA / FPGA allocation failed on node %u after a feasible Filter",
                  node);
    }
    c->aux[node] = row;
    aux_mark(c, node);
    done.aux = *ao;
  }
  int rec_i = -1;   // the chosen node's matched record (records are in node order)
  {
    auto it = std::lower_bound(c->xrec.begin(), c->xrec.end(), node,
                               [](const ExtRec& r, uint32_t n) { return r.node < n; });
    if (it != c->xrec.end() && it->node == node) rec_i = (int)(it - c->xrec.begin());
  }
  if (rs_on && rec_i >= 0) {   // Reservation.Reserve -> reservationCache.assumePod (AddAssignedPod, reservation_info.go:379-388)
    const int nom = h_xnom[rec_i];
    if (nom >= 0) {
      gs_reservation& r = c->rsv.at(c->xres_uid[c->xrec[rec_i].first + nom]);
      for (int s = 0; s < 7; ++s)
        if ((r.resource_names_mask >> s & 1u) && (pod.request_mask >> s & 1u)) {
          r.allocated[s] = ((r.allocated_mask >> s & 1u) ? r.allocated[s] : 0) + pod.requests[s];
          r.allocated_mask |= 1u << s;
          done.rsv_slots |= 1u << s;
          done.rsv_added[s] = pod.requests[s];
        }
      r.assigned_pods += 1;
      eo->reservation_uid = r.uid;
    }
  }
  for (int n = 0; n < GS_NUM_GPU_NAMES; ++n)   // NodeInfo.AddPod of the GPU-name scalars
    if (gpu_names_all >> n & 1u) {
      c->devs[node].requested[n] += e.gpu_requests[n];
      done.gpu_name_req[n] = e.gpu_requests[n];
      dev_mark(c, node);
    }
  for (int x = 0; x < GS_MAX_XRES; ++x)         // ... and of the registered extended resources
    if (xres_all >> x & 1u) {
      c->devs[node].xres_requested[x] += e.xres_requests[x];
      done.xres_req[x] = e.xres_requests[x];
      dev_mark(c, node);
    }
  if (gmask || (rs_on && rec_i >= 0 && h_xnom[rec_i] >= 0) || gpu_names_all || xres_all || ch.amask) {
    done.gpu_minor_mask = eo->gpu_minor_mask;
    done.gpu_count = eo->gpu_count;
    for (int r = 0; r < GS_NUM_GPU_RES; ++r) done.gpu_per_instance[r] = eo->gpu_per_instance[r];
    done.reservation_uid = eo->reservation_uid;
    done.gpu_names = gpu_names_all;
    done.xres = xres_all;
    c->ext_reserved[pod.uid] = done;   // gs_pods_forget undoes exactly this
  }
  apply_placement(c, pod, xo.node, true);
  if (c->host_timing)
    c->hx_reserve += std::chrono::duration<double, std::micro>(hx_clk::now() - hx3).count();
  return GS_OK;
}

}  // namespace

// ================================================================================================
extern "C" {

uint32_t gs_num_feasible_nodes_to_find(uint32_t num_all_nodes, int32_t pct) {
  // [upstream] schedule_one.go numFeasibleNodesToFind: minFeasibleNodesToFind = 100,
  // minFeasibleNodesPercentageToFind = 5, adaptive 50 - N/125 % (int32 arithmetic)
  const int32_t n = (int32_t)num_all_nodes;
  if (n < 100 || pct >= 100) return num_all_nodes;
  int32_t p = pct > 0 ? pct : std::max<int32_t>(5, 50 - n / 125);
  const int32_t k = n * p / 100;
  return k < 100 ? 100u : (uint32_t)k;
}

const char* gs_version(void) { return "libgpuscore 0.1 (gfx950, ABI 1)"; }

void gs_abi_sizes(uint64_t* out, uint32_t n) {
  const uint64_t s[] = {sizeof(gs_pod), sizeof(gs_node), sizeof(gs_node_metric), sizeof(gs_pod_metric),
                        sizeof(gs_config), sizeof(gs_placement), sizeof(gs_stats), sizeof(gs_loadaware_args),
                        sizeof(gs_cpu_topology), sizeof(gs_node_numa), sizeof(gs_pod_allocation), sizeof(gs_numa_args),
                        sizeof(gs_quota_group), sizeof(gs_quota_status), sizeof(gs_node_devices),
                        sizeof(gs_reservation), sizeof(gs_pod_ext), sizeof(gs_ext_args), sizeof(gs_ext_placement),
                        sizeof(gs_status_map), sizeof(gs_resident_pod), sizeof(gs_preemptor),
                        sizeof(gs_preempt_result), sizeof(gs_preempt_detail), sizeof(gs_preempt_candidate),
                        sizeof(gs_preempt_result_pdb), sizeof(gs_preempt_detail_pdb), sizeof(gs_preempt_candidate_pdb),
                        sizeof(gs_top_score), sizeof(gs_top_scores), sizeof(gs_aux_device),
                        sizeof(gs_node_aux_devices), sizeof(gs_pod_aux), sizeof(gs_aux_placement)};
  for (uint32_t i = 0; i < n && i < sizeof(s) / sizeof(s[0]); ++i) out[i] = s[i];
}

void gs_loadaware_args_default(gs_loadaware_args* a) {
  if (!a) return;
  std::memset(a, 0, sizeof(*a));
  a->filter_expired_node_metrics = 1;
  a->has_node_metric_expiration = 1;
  a->node_metric_expiration_seconds = 180;
  a->resource_weights[0] = a->resource_weights[1] = 1;
  a->resource_weights_mask = GS_USAGE_CPU | GS_USAGE_MEMORY;
  a->usage_thresholds[0] = 65;
  a->usage_thresholds[1] = 95;
  a->usage_thresholds_mask = GS_USAGE_CPU | GS_USAGE_MEMORY;
  a->estimated_scaling_factors[0] = 85;
  a->estimated_scaling_factors[1] = 70;
  a->estimated_scaling_factors_mask = GS_USAGE_CPU | GS_USAGE_MEMORY;
  a->agg_usage_type = GS_AGG_NONE;
  a->agg_score_type = GS_AGG_NONE;
}

void gs_fit_args_default(gs_fit_args* a) {
  if (!a) return;
  std::memset(a, 0, sizeof(*a));
  a->resource_weights[GS_RES_CPU] = 1;
  a->resource_weights[GS_RES_MEMORY] = 1;
}

int gs_loadaware_args_validate(const gs_loadaware_args* a, char* msg, size_t len) {
  auto bad = [&](const char* s) {
    if (msg && len) snprintf(msg, len, "%s", s);
    return GS_EINVAL;
  };
  if (!a) return bad("nil args");
  if (a->has_node_metric_expiration && a->node_metric_expiration_seconds <= 0)
    return bad("nodeMetricExpiredSeconds should be a positive value");
  for (int r = 0; r < 2; ++r) {
    if (a->resource_weights_mask & (1u << r)) {
      if (a->resource_weights[r] <= 0) return bad("resource Weight should be a positive value");
      if (a->resource_weights[r] > 100) return bad("resource Weight should be less than 100");
    }
    if (a->usage_thresholds_mask & (1u << r)) {
      if (a->usage_thresholds[r] < 0) return bad("resource Threshold should be a positive value");
      if (a->usage_thresholds[r] > 100) return bad("resource Threshold should be less than 100");
    }
    if (a->estimated_scaling_factors_mask & (1u << r)) {
      if (a->estimated_scaling_factors[r] <= 0) return bad("estimated resource Threshold should be a positive value");
      if (a->estimated_scaling_factors[r] > 100) return bad("estimated  resource Threshold should be less than 100");
    }
    if ((a->resource_weights_mask & (1u << r)) && !(a->estimated_scaling_factors_mask & (1u << r)))
      return bad("estimatedScalingFactors: Not found");
  }
  if ((a->resource_weights_mask | a->usage_thresholds_mask | a->prod_usage_thresholds_mask |
       a->estimated_scaling_factors_mask | a->agg_usage_thresholds_mask) & GS_USAGE_OTHER)
    return bad("resources other than cpu/memory are not supported on this path");
  if (msg && len) msg[0] = 0;
  return GS_OK;
}

int gs_create(const gs_config* cfg, gs_ctx** out) {
  if (!cfg || !out) return GS_EINVAL;
  *out = nullptr;
  if (cfg->abi_version != GS_ABI_VERSION) return GS_EINVAL;
  gs_ctx* c = new gs_ctx();
  c->cfg = *cfg;
  char msg[256];
  if (gs_loadaware_args_validate(&cfg->loadaware, msg, sizeof msg) != GS_OK) {
    fprintf(stderr, "gpuscore: invalid LoadAwareSchedulingArgs: %s\n", msg);
    delete c;
    return GS_EINVAL;
  }
  if (cfg->num_nodes == 0) { delete c; return GS_EINVAL; }
  if (compute_profile(c) != GS_OK) {
    fprintf(stderr, "gpuscore: %s\n", c->err.c_str());
    delete c;
    return GS_EINVAL;
  }
  if (cfg->sample_nodes != 0 && cfg->sample_nodes != 1) { delete c; return GS_EINVAL; }
  c->window_k = cfg->sample_nodes ? gs_num_feasible_nodes_to_find(cfg->num_nodes, cfg->percentage_of_nodes_to_score) : 0;
  c->B = cfg->batch_size ? (int)cfg->batch_size : MAX_BATCH;
  if (c->B < 1 || c->B > MAX_BATCH || (cfg->cand_cap && cfg->cand_cap != (uint32_t)LCAP)) {
    fprintf(stderr, "gpuscore: batch_size must be in [1,%d] and cand_cap %d\n", MAX_BATCH, LCAP);
    delete c;
    return GS_EUNSUPPORTED;
  }
  c->N = cfg->num_nodes;
  c->npad = (c->N + 1023) & ~1023u;
  c->nodes.resize(c->N);
  c->numa.resize(c->N);
  // pod uid -> node maps grow by one entry per placement: buckets for a few pods per node up front, so the scheduling
  // loop does not stop for a rehash of tens of thousands of entries (a multi-ms stall of the batch pipeline)
  c->uid_node.reserve(std::max<size_t>(size_t(1) << 17, 4 * (size_t)c->N));
  c->numa_uid_node.reserve(std::max<size_t>(size_t(1) << 16, (size_t)c->N));
  c->row_dirty.assign(c->N, 0);
  c->devs.assign(c->N, gs_node_devices{});
  c->dev_dirty.assign(c->N, 0);
  c->rsv_node.assign(c->N, {});
  gs_ext_args_default(&c->ext);
  c->ext.enabled = 0;   // the extension plugins are off until gs_ext_configure
  set_shard(c);
  auto bail = [&](const char* what, hipError_t e) {
    fprintf(stderr, "gpuscore: %s: %s\n", what, hipGetErrorString(e));
    gs_destroy(c);
    return GS_EDEVICE;
  };
  hipError_t e;
  if ((e = hipSetDevice(cfg->device)) != hipSuccess) return bail("hipSetDevice", e);
  if ((e = set_kernel_attributes()) != hipSuccess) return bail("hipFuncSetAttribute", e);
  // priorities: the commit chain (patch, cand, commit on st) before the next batch's eval pass (st_ev, st2), which
  // otherwise fills every CU while patch / cand wait for slots
  int prio_lo = 0, prio_hi = 0;
  if ((e = hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi)) != hipSuccess) return bail("hipDeviceGetStreamPriorityRange", e);
  // (Round 3 tried a CU partition here: the commit chain on CU-masked streams, the eval pass on the other CUs, with the
  // host applying a batch's placements one batch late. CU-masked streams are blocking streams — they synchronise with
  // the null stream, which hipMemset / hipMemcpy / hipFree use — and a one-pod-batch test hung in gs_destroy's hipFree
  // with it; the commit measured no faster on a CU of its own. Removed)
  if ((e = c->st.create(hipStreamNonBlocking, prio_hi)) != hipSuccess) return bail("hipStreamCreate", e);
  if ((e = c->st2.create(hipStreamNonBlocking, prio_lo)) != hipSuccess) return bail("hipStreamCreate", e);
  if ((e = c->st_ev.create(hipStreamNonBlocking, prio_lo)) != hipSuccess) return bail("hipStreamCreate", e);
  if ((e = c->st_rb.create(hipStreamNonBlocking)) != hipSuccess) return bail("hipStreamCreate", e);
  if ((e = c->ev_fork.create(hipEventDisableTiming)) != hipSuccess) return bail("hipEventCreate", e);
  if ((e = c->ev_join.create(hipEventDisableTiming)) != hipSuccess) return bail("hipEventCreate", e);
  size_t np = c->npad;
  if ((e = c->mirror_i64.alloc(np * NUM_I64_COLS * 8)) != hipSuccess) return bail("hipMalloc mirror", e);
  if ((e = c->mirror_i32.alloc(np * NUM_I32_COLS * 4)) != hipSuccess) return bail("hipMalloc mirror", e);
  c->mv = MirrorView{c->mirror_i64.get(), c->mirror_i32.get(), (uint32_t)np};
  (void)hipMemset(c->mv.i64, 0, np * NUM_I64_COLS * 8);
  (void)hipMemset(c->mv.i32, 0, np * NUM_I32_COLS * 4);
  c->ld = c->npad;
  size_t xb = xchg_block_bytes(c->B, LCAP);
  if ((e = c->d_xchg_send.alloc(xb)) != hipSuccess) return bail("hipMalloc", e);
  c->xchg_bytes = xb;
  if ((e = c->tb_all.alloc(sizeof(int32_t) * TB_N * c->B * 2)) != hipSuccess) return bail("hipMalloc", e);   // both slots'
  if ((e = c->d_rowstat.alloc(sizeof(RowStat) * (1 + MAX_RANKS))) != hipSuccess) return bail("hipMalloc", e);
  if ((e = c->d_sel.alloc(4 * (1 + MAX_RANKS))) != hipSuccess) return bail("hipMalloc", e);
  c->stage_cap = std::min<uint32_t>(c->N, 65536);
  // staged rows then their node indices (flush_rows)
  if ((e = c->d_stage_rows.alloc((size_t)(8 * ROW_WORDS + 4) * c->stage_cap)) != hipSuccess) return bail("hipMalloc", e);
  if ((e = c->h_stage_rows.alloc((size_t)(8 * ROW_WORDS + 4) * c->stage_cap)) != hipSuccess) return bail("hipHostMalloc", e);
  if ((e = c->h_xchg_send.alloc(xb)) != hipSuccess) return bail("hipHostMalloc", e);
  c->cand_overlap = !env_off("GS_CAND_OVERLAP");
  // pods | seq and committed | out share one allocation each: one copy per batch each way
  static_assert(sizeof(PodVec) % 8 == 0 && sizeof(PlacementDev) % 8 == 0, "staging layout");
  const size_t pods_bytes = (sizeof(PodVec) + 8) * c->B, out_bytes = COMMITTED_BYTES + sizeof(PlacementDev) * c->B;
  for (int k = 0; k < 2; ++k) {
    Slot& sl = c->slot[k];
    if ((e = sl.ev_go.create(hipEventDisableTiming)) != hipSuccess) return bail("hipEventCreate", e);
    if ((e = sl.ev_evdone.create(hipEventDisableTiming)) != hipSuccess) return bail("hipEventCreate", e);
    for (Event& ev : sl.ev)
      if ((e = ev.create()) != hipSuccess) return bail("hipEventCreate", e);
    if ((e = sl.d_S.alloc((size_t)c->B * c->ld * 2)) != hipSuccess) return bail("hipMalloc S", e);
    if ((e = sl.d_aff.alloc((size_t)c->B * c->ld)) != hipSuccess) return bail("hipMalloc aff", e);
    (void)hipMemset(sl.d_S.get(), 0xff, (size_t)c->B * c->ld * 2);
    if ((e = sl.d_pods.alloc(pods_bytes)) != hipSuccess) return bail("hipMalloc", e);
    if ((e = sl.h_pods.alloc(pods_bytes)) != hipSuccess) return bail("hipHostMalloc", e);
    sl.d_seq = reinterpret_cast<uint64_t*>(sl.d_pods.get() + c->B);
    sl.h_seq = reinterpret_cast<uint64_t*>(sl.h_pods.get() + c->B);
    if ((e = sl.d_committed.alloc(out_bytes)) != hipSuccess) return bail("hipMalloc", e);
    if ((e = sl.h_committed.alloc(out_bytes)) != hipSuccess) return bail("hipHostMalloc", e);
    sl.d_out = reinterpret_cast<PlacementDev*>(sl.d_committed.get() + COMMITTED_BYTES / 4);
    sl.h_out = reinterpret_cast<PlacementDev*>(sl.h_committed.get() + COMMITTED_BYTES / 4);
    sl.d_tb = c->tb_all.get() + (size_t)TB_N * c->B * k;
    if (!c->cand_overlap) continue;
    if ((e = sl.d_lst.alloc(xb)) != hipSuccess) return bail("hipMalloc", e);
    if ((e = sl.d_hist.alloc((size_t)4 * c->B * (MAX_SCORE_LIMIT + 1))) != hipSuccess) return bail("hipMalloc", e);
    if ((e = sl.d_landed.alloc(landed_slab_bytes())) != hipSuccess) return bail("hipMalloc", e);
    (void)hipMemset(sl.d_landed.get(), 0, landed_slab_bytes());
  }
  if ((e = c->d_cscratch.alloc(cand_split_scratch_bytes())) != hipSuccess) return bail("hipMalloc", e);
  c->host_timing = env_on("GS_HOST_TIMING");
  if (env_on("GS_COMMIT_STAMPS")) {
    // 8 waves x 64 entries (commit_spec_kernel: one region per wave; the other commit kernels: region 0), then the
    // cand kernel's 8 at entry 512
    if ((e = c->d_stamps.alloc(8 * 524)) != hipSuccess) return bail("hipMalloc", e);
    (void)hipMemset(c->d_stamps.get(), 0, 8 * 524);
    set_cand_stamps(c->d_stamps.get() + 512);
  }
  if ((e = hipDeviceSynchronize()) != hipSuccess) return bail("hipDeviceSynchronize", e);
  // 96 B (LoadAware + Fit row), + 192 B NodeNUMAResource columns when enabled
  c->stats.node_row_bytes = 3 * 8 + 4 + 2 * 8 + 2 * 8 + 2 * 8 + 2 * 8 + 4 + (c->numa_on ? 18 * 8 + 12 * 4 : 0);
  if (const double lim = env_num("GS_WATCHDOG_S", 0.0); lim > 0) c->watchdog = std::thread(watchdog_loop, c, lim);
  *out = c;
  return GS_OK;
}

namespace {
// GS_HOST_TIMING=1: the host's time per batch of schedule_stream and per extension pod, on stderr
void report_host_timing(const gs_ctx* c) {
  if (c->host_timing && c->ht_batches) {
    const double n = (double)c->ht_batches;
    fprintf(stderr, "gpuscore host per batch (us, %llu batches): waiting for the batch %.0f | applying placements %.0f | "
            "staging the next %.0f | enqueueing it %.0f | busy max %.0f; busy histogram (100-us bins):",
            (unsigned long long)c->ht_batches, c->ht_wait / n, c->ht_apply / n, c->ht_stage / n, c->ht_launch / n,
            c->ht_max_busy);
    for (int k = 0; k < 8; ++k) fprintf(stderr, " %llu", (unsigned long long)c->ht_busy_hist[k]);
    fprintf(stderr, "\n");
  }
  if (c->host_timing && c->hx_pods) {
    const double n = (double)c->hx_pods;
    fprintf(stderr, "gpuscore extension path (us): per extension pod (%llu): records %.1f | flushes %.1f | device chain "
            "to wake-up %.1f | Reserves %.1f; per plain run (%llu): gs_schedule %.1f\n", (unsigned long long)c->hx_pods,
            c->hx_prep / n, c->hx_flush / n, c->hx_gpu / n, c->hx_reserve / n, (unsigned long long)c->hx_runs,
            c->hx_runs ? c->hx_plain / (double)c->hx_runs : 0.0);
  }
  const gs_ctx::ReportTiming &hd = c->hr[0], &tp = c->hr[1];
  if (c->host_timing && hd.batches) {
    const double n = (double)hd.batches;
    fprintf(stderr, "gpuscore FitError diagnosis, host per batch with such a pod (us, %llu batches, %llu pods, %llu "
            "landed-row versions): deriving the versions %.1f | landed pass, upload to counters %.1f\n",
            (unsigned long long)hd.batches, (unsigned long long)hd.pods, (unsigned long long)hd.versions,
            hd.derive / n, (hd.landed + hd.merge) / n);
    if (c->hd_map_rows)
      fprintf(stderr, "gpuscore status map: %llu rows read back, %.0f bytes device-to-host per such batch\n",
              (unsigned long long)c->hd_map_rows, (double)c->hd_map_bytes / n);
  }
  if (c->host_timing && tp.batches) {
    const double n = (double)tp.batches;
    fprintf(stderr, "gpuscore top scores, host per batch with a scored pod (us, %llu batches, %llu pods, %llu landed-row "
            "versions): deriving the versions %.1f | landed pass, upload to rows %.1f | merge %.1f\n",
            (unsigned long long)tp.batches, (unsigned long long)tp.pods, (unsigned long long)tp.versions,
            tp.derive / n, tp.landed / n, tp.merge / n);
  }
}

// GS_COMMIT_STAMPS=1: the commit kernel's phase cycle sums, on stderr
void report_commit_stamps(const gs_ctx* c) {
  if (!c->d_stamps) return;
  if (!c->window_k) {   // speculative commit kernel: one stamp region per wave
    std::vector<uint64_t> sa(524);
    if (hipMemcpy(sa.data(), c->d_stamps.get(), 8 * 524, hipMemcpyDeviceToHost) != hipSuccess) return;
    const double np = c->stats_all_pods ? (double)c->stats_all_pods : 1.0;
    auto W = [&](int w, int i) { return (double)sa[w * 64 + i] / np; };
    fprintf(stderr, "gpuscore spec commit, cycles per committed pod (%llu pods, %llu decisions, %llu rollbacks, %.0f "
            "rollback cycles, full-row %llu):\n", (unsigned long long)c->stats_all_pods, (unsigned long long)sa[9],
            (unsigned long long)sa[3], W(0, 4) + W(0, 37) + W(0, 38) + W(0, 39),
            (unsigned long long)sa[10]);
    fprintf(stderr, "  wave 0 total %.0f: checks %.0f | dirty state %.0f | hdr+fresh store+dirty loads %.0f | level scan "
            "%.0f | winner %.0f | fresh slot %.0f | record %.0f | waiting %.0f (at batch end %.0f) | full-row %.0f\n",
            W(0, 12), W(0, 27), W(0, 28), W(0, 29), W(0, 18), W(0, 19), W(0, 20), W(0, 0), W(0, 2), W(0, 23), W(0, 11));
    if (sa[64 + 9] > 0)   // the split selector: wave 0 finishes the prep wave's decisions and verifies
      fprintf(stderr, "  wave 0 (split): verification loop %.0f | fresh slot's scores + snapshot %.0f | record read + late "
              "decisions %.0f | exclusions %.0f | rows settled early %.0f | window %.0f | record %.0f (fresh slot %.0f) | "
              "waiting %.0f (the loop's passes while waiting count in the first two)\n", W(0, 55), W(0, 27), W(0, 52),
              W(0, 53), W(0, 54), W(0, 19), W(0, 0), W(0, 20), W(0, 2));
    if (sa[64 + 9] > 0)
      fprintf(stderr, "  wave 0 (split) waiting passes per pod: batch end %.2f | speculation depth %.2f | host cut %.2f | "
              "exact record asked %.2f | prep record not ready %.2f\n", W(0, 56), W(0, 57), W(0, 58), W(0, 59), W(0, 60));
    fprintf(stderr, "  winner split: ties + tie-break position %.0f | old-nodes path: level segment + list window %.0f\n",
            W(0, 30), W(0, 46));
    if (sa[64 + 9] == 0)   // (single selector wave; the split selector reuses these entries, printed below)
      fprintf(stderr, "  late-landing estimate: %llu decisions, previous pod's row as it stood > M %llu, == M %llu (tie-break "
            "position moves %llu)\n", (unsigned long long)sa[47], (unsigned long long)sa[48], (unsigned long long)sa[49],
            (unsigned long long)sa[50]);
    fprintf(stderr, "  wave 0 raw (cycles per pod by stamp index):");
    for (int i = 0; i < 60; ++i)
      if (sa[i] && (i < 47 || i > 50)) fprintf(stderr, " %d=%.0f", i, W(0, i));
    fprintf(stderr, "\n  wave 1 raw (the split selector's prep wave):");
    for (int i = 0; i < 52; ++i)
      if (sa[64 + i]) fprintf(stderr, " %d=%.0f", i, W(1, i));
    fprintf(stderr, "\n  split: late landings %llu, full decisions %llu, excluded ties %llu, rows settled early %llu\n",
            (unsigned long long)sa[47], (unsigned long long)sa[48], (unsigned long long)sa[49], (unsigned long long)sa[50]);
    const double ng = sa[31] ? (double)sa[31] : 1.0;
    fprintf(stderr, "  winner: old-nodes-only path %llu decisions (%.1f%%), general path %llu (%.1f%%): avg old %.1f new "
            "%.1f window %.1f; avg dirty slots %.1f; list window beyond 32: %llu, beyond 64: %llu\n",
            (unsigned long long)sa[36], 100.0 * sa[36] / np, (unsigned long long)sa[31], 100.0 * sa[31] / np,
            sa[32] / (ng + sa[36]), sa[33] / ng, sa[34] / ng, sa[35] / np, (unsigned long long)sa[24],
            (unsigned long long)sa[25]);
    const double nr = sa[3] ? (double)sa[3] : 1.0;
    auto R = [&](int i) { return (double)sa[i] / nr; };
    fprintf(stderr, "  rollback (cycles per rollback): parking %.0f | undo+hash %.0f | restored-row re-scoring %.0f | "
            "rest %.0f; restored rows %.2f, depth %.2f decisions\n", R(37), R(38), R(39), R(4), R(40), R(41));
    fprintf(stderr, "  pending row's pre-landing score >= M: %llu decisions, %llu of the rollbacks; > M: %llu decisions, %llu "
            "of the rollbacks\n", (unsigned long long)sa[42], (unsigned long long)sa[43], (unsigned long long)sa[44],
            (unsigned long long)sa[45]);
    const bool split = sa[64 + 9] > 0;   // the prep wave counted its records: the split selector ran
    if (split)
      fprintf(stderr, "  wave 1 (prep): busy %.0f (dirty state %.0f, loads %.0f, level scan %.0f, winner %.0f, record "
              "%.0f) waiting %.0f\n", W(1, 28) + W(1, 29) + W(1, 18) + W(1, 30) + W(1, 46) + W(1, 19) + W(1, 0),
              W(1, 28), W(1, 29), W(1, 18), W(1, 30) + W(1, 46) + W(1, 19), W(1, 0), W(1, 2));
    else
      fprintf(stderr, "  wave 4 (verify): busy %.0f waiting %.0f\n", W(4, 1), W(4, 2));
    for (int w = 2; w < 4; ++w)
      fprintf(stderr, "  wave %d (Reserve): fetch+undo %.0f numa_eval %.0f lane0 %.0f rest %.0f (fresh fetch %.0f, landed-"
              "again wait %.0f) waiting %.0f (first decision %.0f)\n", w, W(w, 15), W(w, 16), W(w, 17), W(w, 5), W(w, 21),
              W(w, 22), W(w, 6), W(w, 26));
    for (int w : {split ? 4 : 1, 5, 6, 7})
      fprintf(stderr, "  wave %d (re-scoring): busy %.0f (row copy + hint table %.0f, scores %.0f) waiting %.0f, jobs %.2f "
              "per pod\n", w, W(w, 7) + W(w, 9), W(w, 9), W(w, 7), W(w, 8), W(w, 10));
    for (int base : {30, 40}) {   // re-scoring jobs by what their lanes needed (gs_commit_spec.hip, ST)
      uint64_t v[8] = {};
      for (int w : {split ? 4 : 1, 5, 6, 7})
        for (int i = 0; i < 8; ++i) v[i] += sa[w * 64 + base + i];
      fprintf(stderr, "  re-scoring jobs on %s rows: %llu jobs, %llu lanes: infeasible at batch start %llu, below the "
              "lowest listed level %llu, needed %llu, lists too short %llu; jobs with every lane infeasible %llu, with "
              "no lane needed %llu\n", base == 30 ? "no-policy" : "NUMA-policy", (unsigned long long)v[0],
              (unsigned long long)v[1], (unsigned long long)v[2], (unsigned long long)v[3], (unsigned long long)v[4],
              (unsigned long long)v[5], (unsigned long long)v[6], (unsigned long long)v[7]);
    }
    const double nb = c->stats.batches ? (double)c->stats.batches * c->B : 1.0;
    fprintf(stderr, "gpuscore cand_kernel, wave-0 cycles per pod row: pass 1 %.0f, level sums %.0f, level pick %.0f, "
            "offsets %.0f, pass 2 %.0f\n", sa[512] / nb, sa[513] / nb, sa[514] / nb, sa[515] / nb, sa[516] / nb);
    fprintf(stderr, "gpuscore fix_levels_kernel, thread-0 cycles per pod row: loads+dedupe %.0f, landed rows + level pick "
            "%.0f, lists %.0f; the block's slowest landed-row lane: row loads %.0f, loads + evaluation %.0f; thread 0: "
            "start -> its evaluation %.0f, start -> every lane evaluated %.0f\n",
            sa[517] / nb, sa[518] / nb, sa[519] / nb, sa[520] / nb, sa[521] / nb, sa[522] / nb, sa[523] / nb);
  } else {   // commit_window_kernel (node sampling): thread 0's stamps 7..11, thread 128's 12 and 13
    // a stamp takes the time since the thread's previous one: a pod's window selection and winner fetch count in
    // the first stamp after them (the Reserve's pair evaluation where the pod has one, else the assume)
    uint64_t st[14] = {};
    if (hipMemcpy(st, c->d_stamps.get(), sizeof st, hipMemcpyDeviceToHost) != hipSuccess) return;
    const double np = c->stats_all_pods ? (double)c->stats_all_pods : 1.0;
    uint64_t tot = 0;
    for (int i = 7; i < 12; ++i) tot += st[i];
    auto P = [&](int i) { return tot ? 100.0 * (double)st[i] / (double)tot : 0.0; };
    fprintf(stderr, "gpuscore window commit, thread 0 (s_memtime ticks, %% of %llu; %llu pods, %.0f ticks per pod): "
            "selection + Reserve pair evaluation %.1f%% | device cpuset Reserve %.1f%% | selection (pods without the "
            "pair evaluation) + assume %.1f%% | re-scoring of a NUMA-policy row %.1f%% | of another row %.1f%%\n",
            (unsigned long long)tot, (unsigned long long)c->stats_all_pods, (double)tot / np, P(10), P(11), P(7), P(8),
            P(9));
    fprintf(stderr, "  policy-row re-scoring: %llu pods, %.0f ticks per pair (thread 128)\n", (unsigned long long)st[12],
            st[12] ? (double)st[13] / (double)st[12] : 0.0);
  }
}
}  // namespace

// Stop what still uses the context (worker, watchdog), report, then wait for every stream before the members go
// (gs_ctx: buffers, then events, then streams). Also the way out of a half-built context (gs_create's bail).
int gs_destroy(gs_ctx* c) {
  if (!c) return GS_EINVAL;
  async_stop(c);
  if (c->watchdog.joinable()) {
    c->wd_stop.store(true);
    c->watchdog.join();
  }
  report_host_timing(c);
  report_commit_stamps(c);
  if (c->comm) ncclCommDestroy(c->comm);
  // readbacks into the pinned buffers and the side stream's eval pass may still be in flight
  for (const Stream* s : {&c->st, &c->st_ev, &c->st_rb, &c->st2, &c->st_dg})
    if (*s) (void)host_wait_stream(s->get());
  // the candidate kernels' stamp pointer is the process's: a later context must not write into this one's buffer
  if (c->d_stamps) clear_cand_stamps(c->d_stamps.get() + 512);
  delete c;
  return GS_OK;
}

const char* gs_last_error(gs_ctx* c) {
  if (!c) return "nil context";
  quiesce(c);
  return c->err.c_str();
}

int gs_set_now(gs_ctx* c, int64_t now) {
  if (!c) return GS_EINVAL;
  quiesce(c);
  if (now != c->now) c->prep_stale = true;
  c->now = now;
  return GS_OK;
}

int gs_nodes_upsert(gs_ctx* c, const uint32_t* idx, const gs_node* nodes, uint32_t n) {
  if (!c || (!nodes && n)) return GS_EINVAL;
  quiesce(c);
  for (uint32_t j = 0; j < n; ++j) {
    uint32_t i = idx ? idx[j] : j;
    if (i >= c->N) return fail(c, GS_EINVAL, "node index %u >= %u", i, c->N);
    int rc = validate_node(c, nodes[j]);
    if (rc) return rc;
    c->nodes[i].node = nodes[j];
    if (!c->nodes[i].valid) ++c->n_valid;
    c->nodes[i].valid = true;
    mark_dirty(c, i);
  }
  return flush_rows(c);
}

int gs_node_metrics_upsert(gs_ctx* c, const uint32_t* idx, const gs_node_metric* m, uint32_t n,
                           const gs_pod_metric* pm, const uint32_t* off) {
  if (!c || (!m && n)) return GS_EINVAL;
  quiesce(c);
  for (uint32_t j = 0; j < n; ++j) {
    uint32_t i = idx ? idx[j] : j;
    if (i >= c->N) return fail(c, GS_EINVAL, "node index %u >= %u", i, c->N);
    if (m[j].n_aggregated < 0 || m[j].n_aggregated > GS_MAX_AGG_USAGES)
      return fail(c, GS_EINVAL, "n_aggregated %d outside [0,%d]", m[j].n_aggregated, GS_MAX_AGG_USAGES);
    HostNode& hn = c->nodes[i];
    index_metric_names(c, hn, -1);
    hn.metric = m[j];
    hn.pms.clear();
    if (pm && off) hn.pms.assign(pm + off[j], pm + off[j + 1]);
    index_metric_names(c, hn, +1);
    mark_dirty(c, i);
  }
  return flush_rows(c);
}

int gs_pods_assign(gs_ctx* c, const uint32_t* node_idx, const gs_pod* pods, const int64_t* ts, uint32_t n) {
  if (!c || (n && (!node_idx || !pods))) return GS_EINVAL;
  quiesce(c);
  for (uint32_t j = 0; j < n; ++j) {
    uint32_t i = node_idx[j];
    if (i >= c->N) return fail(c, GS_EINVAL, "node index %u >= %u", i, c->N);
    if (pods[j].flags & GS_POD_TERMINATED) continue;       // pod_assign_cache.go:54
    c->nodes[i].assigned[pods[j].uid] = Assigned{ts ? ts[j] : c->now, pods[j]};
    c->uid_node[pods[j].uid] = i;
    mark_dirty(c, i);
  }
  return flush_rows(c);
}

int gs_pods_unassign(gs_ctx* c, const uint32_t* node_idx, const gs_pod* pods, uint32_t n) {
  if (!c || (n && (!node_idx || !pods))) return GS_EINVAL;
  quiesce(c);
  for (uint32_t j = 0; j < n; ++j) {
    uint32_t i = node_idx[j];
    if (i >= c->N) return fail(c, GS_EINVAL, "node index %u >= %u", i, c->N);
    c->nodes[i].assigned.erase(pods[j].uid);
    auto it = c->uid_node.find(pods[j].uid);
    if (it != c->uid_node.end() && it->second == i) c->uid_node.erase(it);
    c->ext_reserved.erase(pods[j].uid);   // the pod left: its extension-path Reserve record goes with it
    mark_dirty(c, i);
  }
  return flush_rows(c);
}

// The scheduler cache's ForgetPod of an assumed pod after the Unreserve plugins ([upstream] scheduleOne's binding-cycle
// failure path). A pod the extension path placed first gets the Unreserves of its recorded Reserve, in the reference's
// order: DeviceShare (deviceshare/plugin.go:432-451 -> updateCacheUsed(..., false), device_cache.go:124-201), Reservation
// (reservation/plugin.go:572-594 -> cache.go:175-177 -> RemoveAssignedPod, frameworkext/reservation_info.go:390-401) and
// NodeInfo.RemovePod of the GPU-name / extended-resource scalars. Then for every pod: NodeInfo.RemovePod, LoadAware
// Unreserve (podAssignCache.unAssign, load_aware.go:265-267) and NodeNUMAResource Unreserve (resourceManager.Release,
// plugin.go:467-476).
int gs_pods_forget(gs_ctx* c, const uint32_t* node_idx, const gs_pod* pods, uint32_t n) {
  if (!c || (n && (!node_idx || !pods))) return GS_EINVAL;
  quiesce(c);
  for (uint32_t j = 0; j < n; ++j) {   // the whole call is validated before anything changes
    if (node_idx[j] >= c->N) return fail(c, GS_EINVAL, "node index %u >= %u", node_idx[j], c->N);
    if (c->ext_reserved.empty()) continue;
    auto xt = c->ext_reserved.find(pods[j].uid);
    if (xt != c->ext_reserved.end() && xt->second.node != node_idx[j])
      return fail(c, GS_EINVAL, "gs_pods_forget: pod %llu was assumed on node %u, not %u",
                  (unsigned long long)pods[j].uid, xt->second.node, node_idx[j]);
  }
  for (uint32_t j = 0; j < n; ++j) {
    const uint32_t i = node_idx[j];
    const gs_pod& p = pods[j];
    auto xt = c->ext_reserved.empty() ? c->ext_reserved.end() : c->ext_reserved.find(p.uid);
    if (xt != c->ext_reserved.end()) {
      const ExtReserved& x = xt->second;
      gs_node_devices& d = c->devs[i];
      // DeviceShare Unreserve: SubtractWithNonNegativeResult on the minors the Device row still has (a node without a
      // Device object now: getNodeDevice == nil, nothing to do)
      if (d.has_device && x.gpu_minor_mask) gpu_unreserve_row(&d, x.gpu_minor_mask, x.gpu_keys, x.gpu_per_instance);
      // ... and on the RDMA / FPGA minors the aux row still has
      if (d.has_device && !c->aux.empty() && (x.aux.minor_mask[0] | x.aux.minor_mask[1])) {
        aux_unreserve_row(&c->aux[i], x.aux);
        aux_mark(c, i);
      }
      // Reservation Unreserve: the subtraction keeps a zero-valued key, so allocated_mask stays; a reservation deleted
      // since is skipped (forgetPod finds no rInfo)
      if (x.reservation_uid) {
        auto rt = c->rsv.find(x.reservation_uid);
        if (rt != c->rsv.end()) {
          gs_reservation& r = rt->second;
          for (int s = 0; s < GS_NUM_RES; ++s)
            if (x.rsv_slots >> s & 1u) {   // (a key an upsert dropped since comes back with the value 0, as in the reference)
              r.allocated[s] = (r.allocated_mask >> s & 1u) ? std::max<int64_t>(0, r.allocated[s] - x.rsv_added[s]) : 0;
              r.allocated_mask |= 1u << s;
            }
          r.assigned_pods = std::max<int32_t>(0, r.assigned_pods - 1);
          mark_dirty(c, r.node);   // its row carries the unmatched restore (reservation_view)
        }
      }
      for (int g = 0; g < GS_NUM_GPU_NAMES; ++g)   // NodeInfo.RemovePod of the scalars
        if (x.gpu_names >> g & 1u) d.requested[g] -= x.gpu_name_req[g];
      for (int k = 0; k < GS_MAX_XRES; ++k)
        if (x.xres >> k & 1u) d.xres_requested[k] -= x.xres_req[k];
      dev_mark(c, i);
      c->ext_reserved.erase(xt);
    }
    HostNode& hn = c->nodes[i];
    for (int s = 0; s < GS_NUM_RES; ++s) hn.node.requested[s] -= p.requests[s];
    hn.node.nonzero_requested[0] -= p.nonzero_requests[0];
    hn.node.nonzero_requested[1] -= p.nonzero_requests[1];
    hn.node.pod_count -= 1;
    hn.assigned.erase(p.uid);
    auto it = c->uid_node.find(p.uid);
    if (it != c->uid_node.end() && it->second == i) c->uid_node.erase(it);
    if (c->numa_on) {
      numa_release(c->numa[i], p.uid);
      auto nt = c->numa_uid_node.find(p.uid);
      if (nt != c->numa_uid_node.end() && nt->second == i) c->numa_uid_node.erase(nt);
    }
    mark_dirty(c, i);
  }
  return flush_rows(c);
}

int gs_pods_on_event(gs_ctx* c, int event, const int32_t* node_idx, const gs_pod* pods, uint32_t n) {
  if (!c || (n && (!node_idx || !pods))) return GS_EINVAL;
  quiesce(c);
  if (event < GS_POD_EVENT_ADD || event > GS_POD_EVENT_DELETE) return fail(c, GS_EINVAL, "unknown pod event %d", event);
  for (uint32_t j = 0; j < n; ++j) {
    const int32_t i = node_idx[j];
    if (i >= (int32_t)c->N) return fail(c, GS_EINVAL, "node index %d >= %u", i, c->N);
    if (i < 0) continue;                                      // nodeName == "": assign / unAssign return early
    const bool terminated = pods[j].flags & GS_POD_TERMINATED;
    const bool assign = event == GS_POD_EVENT_ADD || (event == GS_POD_EVENT_UPDATE && !terminated);
    int rc = assign ? gs_pods_assign(c, (const uint32_t*)&node_idx[j], &pods[j], nullptr, 1)
                    : gs_pods_unassign(c, (const uint32_t*)&node_idx[j], &pods[j], 1);
    if (rc) return rc;
  }
  return GS_OK;
}

int gs_assign_cache_get(gs_ctx* c, uint32_t node, uint64_t* uids, int64_t* ts, uint32_t cap) {
  if (!c || node >= c->N) return GS_EINVAL;
  quiesce(c);
  std::vector<std::pair<uint64_t, int64_t>> v;
  for (const auto& kv : c->nodes[node].assigned) v.push_back({kv.first, kv.second.ts});
  std::sort(v.begin(), v.end());
  for (uint32_t k = 0; k < v.size() && k < cap; ++k) {
    if (uids) uids[k] = v[k].first;
    if (ts) ts[k] = v[k].second;
  }
  return (int)v.size();
}

int gs_evaluate(gs_ctx* c, const gs_pod* pods, uint32_t npods, int16_t* scores, uint16_t* codes,
                int16_t* plugin_scores) {
  if (!c || (npods && !pods)) return GS_EINVAL;
  quiesce(c);
  int rc = ready(c);
  if (rc) return rc;
  if ((rc = flush_rows(c))) return rc;
  if ((rc = node_prep(c))) return rc;
  const uint32_t N = c->N;
  const int chunk = c->B;
  DevBuf<int16_t> d_sc, d_pl;   // (released on every way out)
  DevBuf<uint16_t> d_cd;
  HIP_TRY(c, d_sc.alloc((size_t)chunk * N * 2));
  HIP_TRY(c, d_cd.alloc((size_t)chunk * N * 2));
  HIP_TRY(c, d_pl.alloc((size_t)chunk * N * 2 * GS_NUM_PLUGINS));
  const Slot& s = current_slot(c);   // no batch is in flight: its pod staging buffers serve the chunks
  PodVec *const h_pods = s.h_pods.get(), *const d_pods = s.d_pods.get();
  const hipStream_t st = c->st.get();
  for (uint32_t p0 = 0; p0 < npods; p0 += chunk) {
    int b = (int)std::min<uint32_t>(chunk, npods - p0);
    int prod_cols = 0;
    for (int i = 0; i < b; ++i) {
      if ((rc = validate_pod(c, pods[p0 + i]))) break;
      h_pods[i] = prep_pod(c, pods[p0 + i]);
      prod_cols |= (h_pods[i].flags & PF_PROD_SCORE) ? 1 : 0;
    }
    if (rc) break;
    HIP_TRY(c, hipMemcpyAsync(d_pods, h_pods, sizeof(PodVec) * b, hipMemcpyHostToDevice, st));
    HIP_TRY(c, launch_eval_full(c->mv, d_pods, b, c->pf, N, d_sc.get(), d_cd.get(), d_pl.get(), prod_cols, st));
    if (scores)
      HIP_TRY(c, hipMemcpyAsync(scores + (size_t)p0 * N, d_sc.get(), (size_t)b * N * 2, hipMemcpyDeviceToHost, st));
    if (codes) HIP_TRY(c, hipMemcpyAsync(codes + (size_t)p0 * N, d_cd.get(), (size_t)b * N * 2, hipMemcpyDeviceToHost, st));
    if (plugin_scores)
      HIP_TRY(c, hipMemcpyAsync(plugin_scores + (size_t)p0 * N * GS_NUM_PLUGINS, d_pl.get(),
                                (size_t)b * N * 2 * GS_NUM_PLUGINS, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, host_wait_stream(st));
  }
  return rc;
}

namespace {
// batch [i, i+b): a special pod always runs alone (its row is re-derived on the host afterwards)
int batch_len(const gs_ctx* c, const gs_pod* pods, uint32_t i, uint32_t npods, bool* special_first) {
  int b = (int)std::min<uint32_t>(c->B, npods - i);
  *special_first = special_pod(c, pods[i]);
  if (*special_first) return 1;
  for (int j = 1; j < b; ++j)
    if (special_pod(c, pods[i + j])) return j;
  return b;
}

// PreFilter of pods [i, i+b) into slot s, and their upload
// (uploads on st_ev, where the batch's eval pass runs; a non-speculative batch's eval first waits for everything
// enqueued on st — row deltas, node prep, the previous commit — a speculative one only for the eval pass before it)
int stage_batch(gs_ctx* c, Slot& s, const gs_pod* pods, const uint64_t* seq, uint32_t i, int b, bool speculative) {
  PodVec *const h_pods = s.h_pods.get(), *const d_pods = s.d_pods.get();
  for (int j = 0; j < b; ++j) {
    h_pods[j] = prep_pod(c, pods[i + j]);
    s.h_seq[j] = seq ? seq[i + j] : (uint64_t)(i + j);
  }
  if (!speculative) {
    HIP_TRY(c, hipEventRecord(s.ev_go.get(), c->st.get()));
    HIP_TRY(c, hipStreamWaitEvent(c->st_ev.get(), s.ev_go.get(), 0));
  }
  // one copy: the B pod vectors' block (b of them staged) and the b sequence numbers after it
  hipStream_t up = direct_batch(c, b, speculative) ? c->st.get() : c->st_ev.get();
  // (the merged copy spans all B pod vectors, d_seq following the block: a short batch copies its b vectors and seq)
  if (4 * b >= c->B) {
    HIP_TRY(c, hipMemcpyAsync(d_pods, h_pods, sizeof(PodVec) * c->B + 8 * b, hipMemcpyHostToDevice, up));
  } else {
    HIP_TRY(c, hipMemcpyAsync(d_pods, h_pods, sizeof(PodVec) * b, hipMemcpyHostToDevice, up));
    HIP_TRY(c, hipMemcpyAsync(s.d_seq, s.h_seq, 8 * b, hipMemcpyHostToDevice, up));
  }
  return GS_OK;
}

bool uid_overlap(const gs_pod* a, int na, const gs_pod* b, int nb) {
  std::unordered_set<uint64_t> u;
  u.reserve(2 * na);
  for (int i = 0; i < na; ++i) u.insert(a[i].uid);
  for (int i = 0; i < nb; ++i)
    if (u.count(b[i].uid)) return true;
  return false;
}
}  // namespace

extern "C++" {
namespace {
// A contiguous run of the pod stream: one gs_schedule call or one gs_schedule_submit.
struct PodRun {
  const gs_pod* pods = nullptr;
  const uint64_t* seq = nullptr;
  gs_placement* out = nullptr;
  uint32_t n = 0;
  void* tag = nullptr;
  Reports rep;
};

// Several ranks: whether the next run is already known (gs_schedule_submit) is a matter of each rank's timing. The
// ranks agree on it at every batch that ends a run (all of them must hold it), so that they speculate across the run
// boundary together and their exchanges pair up; a rank that holds the next run when the others do not starts it
// after the current one without speculation, as they do. Behind the current batch's all-gather on its stream, so that
// every collective of the context is ordered by its streams (an RCCL communicator's collectives must run in issue
// order): score rows on st_ev (the commit in flight on st keeps running while the host waits), levels on st.
int agree_next_run(gs_ctx* c, bool* use) {
  const uint32_t mine = *use ? 1u : 0u;
  std::vector<uint32_t> all(c->nranks);
  if (int rc = exchange_small(c, XSITE_RUNS, nullptr, 4, all.data(), c->sgather ? c->st_ev.get() : c->st.get(), &mine)) return rc;
  for (uint32_t v : all) *use = *use && v;
  return GS_OK;
}

// A batch's results as the host applies them: the slot's pinned buffers, or the copy a deferred batch keeps of them
// (schedule_stream). wide: the wide pass's counters ([pod][DIAG_WORDS]: every node the batch did not land on); top: the
// device pass's block (per pod the first topn of the nodes the batch did not land on, sorted).
struct BatchResults {
  const PlacementDev* out;
  const PodVec* pods;
  const uint32_t* wide;
  const uint8_t* top;
};

// apply_batch's tables of a reported batch, kept across the batches of a schedule_stream call: the landed nodes, per
// node its current row version and whether a landing has made it stale, and per pod that wants versions its vector,
// its index in the batch and its version per landed node; the top scores' merge list.
struct ReportScratch {
  std::vector<uint32_t> nodes;
  std::vector<uint16_t> cur, vidx;
  std::vector<uint8_t> stale;
  std::vector<PodVec> pods;
  std::vector<int> k;
  std::vector<gs_top_score> rows;
};

// The status rows of slot sl's batch, just waited for (n committed pods, placements hout), into sl->h_words: the
// batch's share of the map's rows is chosen here (every batch before it is applied: rows_used is current), and
// those rows alone are copied, as one block (rows are in queue order), on the landed pass's stream. The batch may be
// applied deferred, after the batch two ahead is launched into this slot: that batch's wide pass waits for the copy
// on the device (launch_batch), so the launch is not held back and the rows are not overwritten under the copy.
int fetch_rows(gs_ctx* c, Slot& sl, const PlacementDev* hout, int n, gs_status_map* mp) {
  sl.rows_fetched = 0;
  if (!mp || mp->rows_used >= mp->cap_rows) return GS_OK;
  uint32_t nfit = 0;
  for (int k = 0; k < n; ++k) nfit += hout[k].node < 0;
  const uint32_t nrow = std::min<uint32_t>(nfit, mp->cap_rows - mp->rows_used);
  if (!nrow) return GS_OK;
  if (!sl.rep.rows) return fail(c, GS_ESTATE, "status map: the batch ran without its rows");
  HIP_TRY(c, hipMemcpyAsync(sl.h_words.get(), sl.d_words.get(), sizeof(uint16_t) * (size_t)nrow * c->npad,
                            hipMemcpyDeviceToHost, c->st_dg.get()));
  HIP_TRY(c, hipEventRecord(sl.ev_rows.get(), c->st_dg.get()));
  sl.rows_in_flight = true;
  sl.rows_fetched = (int)nrow;
  return GS_OK;
}

// The diagnoses of the batch's pods with no node (w.k) into dg[0..n): the wide pass's counters plus the landed pass's.
// mp != nullptr: the first nrow of those pods (queue order) take the map's next rows; their device rows (the wide pass
// wrote row f for the batch's f-th such pod) are in sl.h_words (fetch_rows), the landed pass's words are patched in at
// the landed nodes, and each row goes to the caller's words at its stride of num_nodes.
void merge_diag(gs_ctx* c, const ReportScratch& w, gs_fit_diagnosis* dg, gs_status_map* mp, uint32_t base, int nrow,
                const Slot& sl, const uint32_t* wide) {
  const int nL = (int)w.nodes.size();
  for (int f = 0; f < nrow; ++f) {
    const uint32_t row = mp->rows_used + (uint32_t)f;
    uint16_t* dst = mp->words + (size_t)row * c->N;
    std::memcpy(dst, sl.h_words.get() + (size_t)f * c->npad, sizeof(uint16_t) * c->N);
    for (int j = 0; j < nL; ++j) dst[w.nodes[j]] = sl.h_lwords.get()[(size_t)f * nL + j];
    mp->row_of[base + w.k[f]] = (int32_t)row;
  }
  if (mp) mp->rows_used += (uint32_t)nrow;
  const uint32_t* landed = sl.h_ldiag.get();
  for (size_t f = 0; f < w.k.size(); ++f) {
    const int k = w.k[f];
    gs_fit_diagnosis& d = dg[k];
    d.valid = 1;
    d.num_all_nodes = c->N;
    for (int r = 0; r < GS_NUM_FIT_REASONS; ++r) {
      d.reasons[r] = wide[(size_t)k * DIAG_WORDS + r] + (nL ? landed[f * DIAG_WORDS + r] : 0u);
      if (fit_reason_status(r) == 2) d.unresolvable_nodes += d.reasons[r];
    }
    d.failed_nodes = wide[(size_t)k * DIAG_WORDS + DIAG_FAILED] + (nL ? landed[f * DIAG_WORDS + DIAG_FAILED] : 0u);
  }
  if (c->host_timing) {
    c->hd_map_rows += (uint64_t)nrow;
    if (nrow) c->hd_map_bytes += sizeof(uint16_t) * ((size_t)nrow * c->npad + w.k.size() * nL);
  }
}

// The tables of the batch's scored pods (w.k) into tp's rows and counts from base on: a feasible landed node joins the
// device's list of the other nodes, which is sorted by (total descending, node ascending) and cut at topn. The top-N of
// the union lies within the device's top-N of the other nodes and the landed ones.
int merge_top(gs_ctx* c, ReportScratch& w, gs_top_scores* tp, uint32_t base, const Slot& sl, const uint8_t* topblk) {
  const int nL = (int)w.nodes.size();
  const uint32_t* dcnt = reinterpret_cast<const uint32_t*>(topblk);
  const gs_top_score* drows = reinterpret_cast<const gs_top_score*>(topblk + TOP_COUNT_BYTES);
  const TopLanded* landed = sl.h_ltop.get();
  for (size_t f = 0; f < w.k.size(); ++f) {
    const int k = w.k[f];
    const uint32_t dn = dcnt[k];
    if (dn > tp->topn) return fail(c, GS_ESTATE, "top scores: the device pass wrote no table for a scored pod");
    w.rows.assign(drows + (size_t)k * GS_MAX_TOP_SCORES, drows + (size_t)k * GS_MAX_TOP_SCORES + dn);
    // (the device's list is full and sorted: a landed node behind its last row cannot make the cut)
    const bool full = dn == tp->topn;
    const gs_top_score last = full ? w.rows.back() : gs_top_score{};
    for (int j = 0; j < nL; ++j) {
      const TopLanded& l = landed[f * nL + j];
      if (l.total < 0) continue;
      if (full && (l.total < last.total || (l.total == last.total && w.nodes[j] > last.node))) continue;
      gs_top_score r;
      r.node = w.nodes[j];
      r.total = l.total;
      for (int q = 0; q < GS_NUM_PLUGINS; ++q) r.plugin[q] = l.plugin[q];
      w.rows.push_back(r);
    }
    std::sort(w.rows.begin(), w.rows.end(), [](const gs_top_score& a, const gs_top_score& b) {
      return a.total > b.total || (a.total == b.total && a.node < b.node);
    });
    const uint32_t cnt = std::min<uint32_t>((uint32_t)w.rows.size(), tp->topn);
    std::memcpy(tp->rows + (size_t)(base + k) * tp->topn, w.rows.data(), sizeof(gs_top_score) * cnt);
    tp->count[base + k] = cnt;
  }
  return GS_OK;
}

// The placements of pods [base, base + n) of `run`, as slot sl's batch committed them (r), to the caller's out[] and
// the host state, and the run's reports of the batch to their destinations. The device passes behind the commit saw
// every node the batch did not land on; the landed nodes are added here: walking the placements in queue order, the
// host state of every node at a pod's turn is its state before that pod's own landing, so at every pod that wants them
// (the diagnosis: no node; the top scores: placed with more than one node feasible, [upstream] schedulePod skips
// prioritizeNodes otherwise) the device-format rows of the batch's landed nodes are derived there (derive_row /
// derive_row_numa, the two gs_debug_mirror_check holds to the device's rows). A row changes only at a landing, so each
// version is derived once and the pod gets an index per landed node; the landed pass evaluates them on sl's buffers.
int apply_batch(gs_ctx* c, ReportScratch& w, const PodRun& run, uint32_t base, int n, bool special, Slot& sl,
                const BatchResults& r) {
  const gs_pod* pods = run.pods + base;
  gs_placement* outp = run.out + base;
  const Reports& rep = run.rep;
  enum { NONE, NO_NODE, SCORED } want = NONE;   // the pods that want the landed nodes' versions
  int nrow = 0, nv = 0;
  if (rep.top) {
    std::fill_n(rep.top->count + base, n, 0u);
    want = SCORED;
  } else if (rep.diag) {
    std::memset(rep.diag + base, 0, sizeof(gs_fit_diagnosis) * n);
    if (rep.map) std::fill_n(rep.map->row_of + base, n, -1);
    int nfit = 0;
    for (int k = 0; k < n; ++k) nfit += r.out[k].node < 0;
    if (nfit) want = NO_NODE;
    if (nfit && rep.map) {
      nrow = (int)std::min<uint32_t>((uint32_t)nfit, rep.map->cap_rows - rep.map->rows_used);
      rep.map->rows_dropped += (uint32_t)(nfit - nrow);
      if (nrow != sl.rows_fetched) return fail(c, GS_ESTATE, "status map: the batch's rows were not read back");
    }
  }
  if (want) {
    w.nodes.clear();
    for (int k = 0; k < n; ++k)
      if (r.out[k].node >= 0 && std::find(w.nodes.begin(), w.nodes.end(), (uint32_t)r.out[k].node) == w.nodes.end())
        w.nodes.push_back((uint32_t)r.out[k].node);
    w.cur.assign(w.nodes.size(), 0);
    w.stale.assign(w.nodes.size(), 1);
    w.vidx.clear();
    w.pods.clear();
    w.k.clear();
  }
  const int nL = want ? (int)w.nodes.size() : 0;
  double t_derive = 0;
  for (int k = 0; k < n; ++k) {
    const PlacementDev& pd = r.out[k];
    gs_placement& o = outp[k];
    o.node = pd.node;
    o.feasible = pd.feasible;
    o.score = pd.node >= 0 ? pd.score : 0;
    o.ties = pd.node >= 0 ? pd.ties : 0;
    o.flags = pd.flags & ~PL_INTERNAL_FLAGS;
    if (pd.flags & GS_PLACED_SLOWPATH) c->stats.slowpath_pods += 1;   // resolved from its whole score row
    if (want && (want == NO_NODE ? pd.node < 0 : pd.node >= 0 && pd.feasible >= 2)) {
      const int64_t t0 = c->host_timing ? mono_ns() : 0;
      for (int j = 0; j < nL; ++j) {
        if (w.stale[j]) {
          if (nv >= DIAG_VERSIONS)
            return fail(c, GS_ESTATE, "%s: landed-row versions overflow", rep.top ? "top scores" : "FitError diagnosis");
          int64_t* row = reinterpret_cast<int64_t*>(sl.h_dgl.get()) + (size_t)nv * ROW_WORDS;
          derive_row(c, w.nodes[j], row);
          derive_row_numa(c, w.nodes[j], row);
          w.cur[j] = (uint16_t)nv++;
          w.stale[j] = 0;
        }
        w.vidx.push_back(w.cur[j]);
      }
      w.pods.push_back(r.pods[k]);
      w.k.push_back(k);
      if (c->host_timing) t_derive += (double)(mono_ns() - t0) * 1e-3;
    }
    if (int rc = numa_reserve(c, pods[k], r.pods[k], pd)) return rc;
    apply_placement(c, pods[k], pd.node, special);
    if (want && pd.node >= 0) w.stale[std::find(w.nodes.begin(), w.nodes.end(), (uint32_t)pd.node) - w.nodes.begin()] = 1;
  }
  if (!want || w.k.empty()) return GS_OK;
  const int64_t t1 = c->host_timing ? mono_ns() : 0;
  if (nL) {   // (a scored pod landed: the top scores always have one)
    const Landed kind = rep.top ? Landed::TOP : nrow ? Landed::DIAG_MAP : Landed::DIAG;
    if (int rc = landed_pass(c, sl, kind, nv, w.pods, w.vidx, nL)) return rc;
  } else if (nrow) {
    Where w_(c, "apply_batch: the status rows");
    HIP_TRY(c, host_wait_stream(c->st_dg.get()));
  }
  const int64_t t2 = c->host_timing ? mono_ns() : 0;
  if (rep.top) {
    if (int rc = merge_top(c, w, rep.top, base, sl, r.top)) return rc;
  } else {
    merge_diag(c, w, rep.diag + base, rep.map, base, nrow, sl, r.wide);
  }
  if (c->host_timing) {
    gs_ctx::ReportTiming& t = c->hr[rep.top ? 1 : 0];
    t.derive += t_derive;
    t.landed += (double)(t2 - t1) * 1e-3;
    t.merge += (double)(mono_ns() - t2) * 1e-3;
    t.batches += 1;
    t.versions += nv;
    t.pods += w.k.size();
  }
  return GS_OK;
}

// The scheduleOne loop over the pod stream, batch by batch. Pipelining: while batch [i, i+b) runs, the next batch is
// staged and enqueued behind it on the stream (other slot). Its commit kernel checks on the device that the batch
// before committed all its pods with no host-side Reserve pending, else it is a no-op; the host only keeps it when the
// same holds on its side. The next batch may be the first of the next run (next_run: the run after the current one
// if it is already known), so the pipeline continues across runs. Every rank takes the same decisions (replicated
// host state), so speculative exchanges pair up; with the host-callback transport the speculative pass's exchange
// waits for the current batch (no overlap, same result). run_done(run, rc): the run's placements are all written
// (rc 0), or it failed; on an error the current run gets the error and a run already taken from next_run GS_ESTATE.
template <class Next, class Done>
int schedule_stream(gs_ctx* c, PodRun run, Next&& next_run, Done&& run_done) {
  static const bool can_spec = !env_on("GS_NO_PIPELINE");
  PodRun nxt{};
  bool have_nxt = false;
  auto drain = [&]() {
    Where w_(c, "schedule_stream: drain");
    (void)host_wait_stream(c->st.get());
    (void)host_wait_stream(c->st_ev.get());
    (void)host_wait_stream(c->st_rb.get());   // a voided or in-flight batch's readback into the pinned buffers
  };
  // Deferred application: a batch that committed every pod with no host work and no special pod changes no row on
  // the host side (apply_placement / numa_reserve only mirror what the commit wrote to HBM), so its placements are
  // applied to the host state after the batch two ahead is launched — the eval pass then starts right as the previous
  // commit ends instead of after the host's ~0.2 ms of bookkeeping, and runs beside the next commit.
  struct Pend {
    PodRun run;             // the batch's run: its pods [base, base + n)
    uint32_t base = 0;
    int n = 0;
    bool active = false;
    Slot* slot = nullptr;   // the slot the batch ran on (its landed-pass buffers)
  } pend;
  ReportScratch scratch;
  std::vector<uint8_t> pend_top;
  std::vector<PlacementDev> pend_out;
  std::vector<PodVec> pend_pods;
  std::vector<uint32_t> pend_wide;
  auto apply_pending = [&]() -> int {
    if (!pend.active) return GS_OK;
    pend.active = false;
    return apply_batch(c, scratch, pend.run, pend.base, pend.n, false, *pend.slot,
                       BatchResults{pend_out.data(), pend_pods.data(), pend_wide.data(), pend_top.data()});
  };
  auto body = [&]() -> int {
    int rc = GS_OK;
    uint32_t i = 0;
    bool inflight = false, cur_special = false, spec_ok = true;
    int cur_b = 0;
    for (;;) {
      if (i == run.n) {   // the run is complete; the next one (its first batch may be in flight already)
        if ((rc = apply_pending())) { drain(); return rc; }
        run_done(run, GS_OK);
        if (!have_nxt) have_nxt = next_run(&nxt);
        if (!have_nxt) break;
        run = nxt;
        have_nxt = false;
        i = 0;
        continue;
      }
      const gs_pod* pods = run.pods;
      // the current batch's slot, and the other one for the batch after it (keeping that batch flips cur_slot below)
      Slot& cur = c->slot[c->cur_slot];
      Slot& ahead = c->slot[1 - c->cur_slot];
      if (!inflight) {
        if ((rc = apply_pending())) { drain(); return rc; }
        if ((rc = flush_rows(c))) return rc;
        if (c->prep_stale && (rc = node_prep(c))) return rc;
        cur_b = batch_len(c, pods, i, run.n, &cur_special);
        // (a cpuset pod whose node is outside the device cpuset scope ends the batch inside the commit kernel)
        if ((rc = stage_batch(c, cur, pods, run.seq, i, cur_b, false))) return rc;
        if ((rc = launch_batch(c, cur, cur_b, run.rep.mode()))) return rc;
      }
      // the batch after this one: in this run, or the first of the next run
      const gs_pod* np = nullptr;
      const uint64_t* ns = nullptr;
      uint32_t nj = 0, nn = 0;
      const uint32_t j = i + cur_b;
      ReportMode nrep = run.rep.mode();   // the reports of the batch after this one (its own run's choice)
      if (j < run.n) {
        np = pods; ns = run.seq; nj = j; nn = run.n;
      } else {
        if (!have_nxt) have_nxt = next_run(&nxt);
        bool use = have_nxt && nxt.n;
        if (c->nranks > 1 && (rc = agree_next_run(c, &use))) { drain(); return rc; }
        if (use) { np = nxt.pods; ns = nxt.seq; nn = nxt.n; nrep = nxt.rep.mode(); }
      }
      bool spec = false;
      int nb = 0;
      using hclk = std::chrono::steady_clock;
      const auto t_a = hclk::now();
      double busy = 0;
      if (pend.active && np) {   // the next batch shares a pod uid with the deferred one: its host state first
        const int nb0 = std::min<int>(c->B, (int)(nn - nj));
        if (uid_overlap(pend.run.pods + pend.base, pend.n, np + nj, nb0) && (rc = apply_pending())) { drain(); return rc; }
      }
      if (can_spec && spec_ok && !cur_special && np && c->dirty_list.empty() && !c->prep_stale) {
        bool sf = false;
        nb = batch_len(c, np, nj, nn, &sf);
        if (!sf && !uid_overlap(pods + i, cur_b, np + nj, nb)) {
          rc = stage_batch(c, ahead, np, ns, nj, nb, true);
          const auto t_b = hclk::now();
          if (!rc) rc = launch_batch(c, ahead, nb, nrep, &cur, cur_b);
          if (c->host_timing) {
            const double st = std::chrono::duration<double, std::micro>(t_b - t_a).count();
            const double la = std::chrono::duration<double, std::micro>(hclk::now() - t_b).count();
            c->ht_stage += st;
            c->ht_launch += la;
            busy += st + la;
          }
          if (rc) { drain(); return rc; }
          spec = true;
        }
      }
      // the previous batch's deferred placements, while this batch and the one after it run
      if ((rc = apply_pending())) { drain(); return rc; }
      spec_ok = true;
      int committed = 0;
      const auto t_w = hclk::now();
      rc = finish_batch(c, cur, cur_b, spec, &committed);
      const auto t_f = hclk::now();
      if (rc == GS_REDO) {   // pod 0 needs the full-row path, the speculative pass (void) overwrote its lists: re-run
        drain();
        if ((rc = apply_pending())) return rc;
        if ((rc = stage_batch(c, cur, pods, run.seq, i, cur_b, false))) return rc;
        if ((rc = launch_batch(c, cur, cur_b, run.rep.mode()))) return rc;
        inflight = true;
        spec_ok = false;
        continue;
      }
      if (rc) { if (spec) drain(); return rc; }
      const PodVec* h_pods = cur.h_pods.get();
      // the device-side continuation flag the speculative pass read
      const bool host_work = cur.h_committed.get()[1] != 1;
      if ((rc = fetch_rows(c, cur, cur.h_out, committed, run.rep.map))) {
        if (spec) drain();
        return rc;
      }
      if (spec && !host_work && !cur_special && committed == cur_b) {
        // no host row changes: keep the results (this slot's buffers are reused by the batch two ahead) and apply them
        // after that batch is launched
        pend_out.assign(cur.h_out, cur.h_out + committed);
        pend_pods.assign(h_pods, h_pods + committed);
        pend.run = run;
        pend.base = i;
        pend.n = committed;
        pend.active = true;
        pend.slot = &cur;
        if (run.rep.diag) pend_wide.assign(cur.h_diag.get(), cur.h_diag.get() + (size_t)DIAG_WORDS * committed);
        if (run.rep.top) pend_top.assign(cur.h_top.get(), cur.h_top.get() + TOP_COUNT_BYTES + TOP_POD_BYTES * committed);
      } else if ((rc = apply_batch(c, scratch, run, i, committed, cur_special, cur,
                                   BatchResults{cur.h_out, h_pods, cur.h_diag.get(), cur.h_top.get()}))) {
        if (spec) drain();
        return rc;
      }
      if (c->host_timing) {
        const double wt = std::chrono::duration<double, std::micro>(t_f - t_w).count();
        const double ap = std::chrono::duration<double, std::micro>(hclk::now() - t_f).count();
        c->ht_wait += wt;
        c->ht_apply += ap;
        busy += ap;
        c->ht_batches += 1;
        c->ht_max_busy = std::max(c->ht_max_busy, busy);
        c->ht_busy_hist[std::min(7, (int)(busy / 100.0))] += 1;   // 100-us bins
      }
      c->stats.pods += committed;
      c->stats_all_pods += committed;
      i += committed;
      inflight = false;
      if (spec) {
        if (!host_work && committed == cur_b) {
          if (!c->dirty_list.empty() || c->prep_stale) {
            drain();
            return fail(c, GS_ESTATE, "speculative batch ran while host rows were pending");
          }
          c->cur_slot = 1 - c->cur_slot;   // the speculative batch is now the current one
          cur_b = nb;
          cur_special = false;
          inflight = true;   // (when it is the next run's first batch, i == run.n: the top of the loop moves there)
        } else {
          drain();   // its commit kernel was a no-op
        }
      }
    }
    if ((rc = apply_pending())) return rc;
    return flush_rows(c);
  };
  int rc = body();
  if (rc && pend.active) {   // a batch the device committed: its placements reach the outputs and the host state
    drain();
    (void)apply_pending();
  }
  if (rc) {
    run_done(run, rc);
    if (have_nxt) run_done(nxt, GS_ESTATE);
  }
  return rc;
}

}  // namespace

namespace {
void async_worker(gs_ctx* c) {
  AsyncQueue& q = *c->aq;
  (void)hipSetDevice(c->cfg.device);
  std::unique_lock<std::mutex> lk(q.mu);
  for (;;) {
    q.cv_work.wait(lk, [&] { return q.stop || !q.pending.empty(); });
    if (q.pending.empty()) return;   // stop
    std::shared_ptr<AsyncRun> first = q.pending.front();
    q.pending.pop_front();
    q.busy = true;
    lk.unlock();
    std::vector<std::shared_ptr<AsyncRun>> taken{first};   // keeps the runs alive while the loop reads them
    auto as_run = [](const std::shared_ptr<AsyncRun>& r) {
      PodRun p;
      p.pods = r->pods.data();
      p.seq = r->seq.data();
      p.out = r->out;
      p.rep = r->rep;
      p.n = (uint32_t)r->pods.size();
      p.tag = r.get();
      return p;
    };
    auto next = [&](PodRun* out) -> bool {
      std::lock_guard<std::mutex> g(q.mu);
      if (q.pending.empty()) return false;
      taken.push_back(q.pending.front());
      q.pending.pop_front();
      *out = as_run(taken.back());
      return true;
    };
    auto done = [&](const PodRun& r, int rc) {
      AsyncRun* a = static_cast<AsyncRun*>(r.tag);
      std::lock_guard<std::mutex> g(q.mu);
      a->rc = rc;
      if (rc) a->err = c->err;
      q.cv_done.notify_all();
    };
    const int rc = schedule_stream(c, as_run(first), next, done);
    lk.lock();
    if (rc) {   // an error fails every later submission (the stream's order is broken)
      for (auto& r : q.pending) {
        r->rc = GS_ESTATE;
        r->err = "an earlier gs_schedule_submit failed: " + c->err;
      }
      q.pending.clear();
    }
    q.busy = false;
    q.cv_done.notify_all();
  }
}
}  // namespace

// Every other call on the context waits until the submitted runs are complete (the worker is idle).
int quiesce(gs_ctx* c) {
  if (!c || !c->aq) return GS_OK;
  AsyncQueue& q = *c->aq;
  std::unique_lock<std::mutex> lk(q.mu);
  q.cv_done.wait(lk, [&] { return q.pending.empty() && !q.busy; });
  return GS_OK;
}

void async_stop(gs_ctx* c) {
  if (!c->aq) return;
  quiesce(c);
  {
    std::lock_guard<std::mutex> g(c->aq->mu);
    c->aq->stop = true;
  }
  c->aq->cv_work.notify_all();
  if (c->aq->th.joinable()) c->aq->th.join();
  c->aq.reset();
}

}  // extern "C++"

namespace {
int schedule_run(gs_ctx* c, const gs_pod* pods, uint32_t npods, const uint64_t* seq, gs_placement* out, Reports rep) {
  int rc = ready(c);
  if (rc) return rc;
  for (uint32_t i = 0; i < npods; ++i)
    if ((rc = validate_pod(c, pods[i]))) return rc;
  PodRun run;
  run.pods = pods;
  run.seq = seq;
  run.out = out;
  run.n = npods;
  run.rep = rep;
  return schedule_stream(c, run, [](PodRun*) { return false; }, [](const PodRun&, int) {});
}

// gs_schedule_submit: the run copied and queued for the worker
int submit_run(gs_ctx* c, const gs_pod* pods, uint32_t npods, const uint64_t* seq, gs_placement* out, Reports rep,
               uint64_t* ticket) {
  auto r = std::make_shared<AsyncRun>();
  // checks that write nothing (the worker may be running): on an error, wait for it, then report
  if (c->n_valid != c->N) {
    quiesce(c);
    if (int rc = ready(c)) return rc;
  }
  char msg[256];
  for (uint32_t i = 0; i < npods; ++i) {
    const int rc = validate_pod_msg(c->numa_on, pods[i], msg, sizeof msg);
    if (rc) {
      quiesce(c);
      return fail(c, rc, "%s", msg);
    }
  }
  r->pods.assign(pods, pods + npods);
  r->seq.resize(npods);
  for (uint32_t i = 0; i < npods; ++i) r->seq[i] = seq ? seq[i] : (uint64_t)i;
  r->out = out;
  r->rep = rep;
  if (!c->aq) {
    c->aq = std::make_unique<AsyncQueue>();
    c->aq->th = std::thread(async_worker, c);
  }
  {
    std::lock_guard<std::mutex> g(c->aq->mu);
    r->ticket = c->aq->next_ticket++;
    c->aq->runs[r->ticket] = r;
    c->aq->pending.push_back(r);
  }
  c->aq->cv_work.notify_all();
  *ticket = r->ticket;
  return GS_OK;
}
}  // namespace

int gs_schedule(gs_ctx* c, const gs_pod* pods, uint32_t npods, const uint64_t* seq, gs_placement* out) {
  if (!c || (npods && (!pods || !out))) return GS_EINVAL;
  quiesce(c);
  return schedule_run(c, pods, npods, seq, out, Reports{});
}

int gs_schedule_submit(gs_ctx* c, const gs_pod* pods, uint32_t npods, const uint64_t* seq, gs_placement* out,
                       uint64_t* ticket) {
  if (!c || !ticket || (npods && (!pods || !out))) return GS_EINVAL;
  return submit_run(c, pods, npods, seq, out, Reports{}, ticket);
}

namespace {
// the caller's status map before a run: no rows handed out (row_of is written per batch, as out is)
bool map_begin(gs_status_map* m, uint32_t npods) {
  if (!m || (npods && !m->row_of) || (m->cap_rows && !m->words)) return false;
  m->rows_used = m->rows_dropped = 0;
  return true;
}
bool top_valid(const gs_top_scores* t) {
  return t && t->rows && t->count && t->topn >= 1 && t->topn <= GS_MAX_TOP_SCORES;
}

enum class ReportKind { DIAG, DIAG_NODES, TOP };

// A run with reports of one kind, blocking (ticket == nullptr) or submitted. The scope of the FitError diagnosis is one
// rank with every node checked (the wide pass reads the whole mirror of one rank's commit; under node sampling the
// reference's map holds only the nodes of the rotation window), and the top-N score tables share it (the reference then
// scores only the rotation window). The buffers come with the context's first run of the kind; the status map's and
// the tables' presuppose the diagnosis' (the landed pass's staged block, slab and stream). A submission runs beside
// the worker (the rank count and the sampling window are fixed before any submission) and waits for it only for the
// buffers' first allocation or the refusal's message.
int report_run(gs_ctx* c, const gs_pod* pods, uint32_t npods, const uint64_t* seq, gs_placement* out, ReportKind kind,
               Reports rep, bool submit, uint64_t* ticket) {
  const bool map = kind == ReportKind::DIAG_NODES, top = kind == ReportKind::TOP;
  if (!c || (submit && !ticket) || (npods && (!pods || !out || (!top && !rep.diag)))) return GS_EINVAL;
  if ((map && !map_begin(rep.map, npods)) || (top && !top_valid(rep.top))) return GS_EINVAL;
  const bool allocated = c->st_dg && (!map || c->slot[0].d_words) && (!top || c->slot[0].d_top);
  if (!submit || c->nranks > 1 || c->window_k || !allocated) {
    quiesce(c);
    const char* what = top ? "top scores" : "FitError diagnosis";
    if (c->nranks > 1) return fail(c, GS_EUNSUPPORTED, "%s: several ranks are not supported", what);
    if (c->window_k) return fail(c, GS_EUNSUPPORTED, "%s: node sampling is not supported", what);
    if (int rc = alloc_diag(c)) return rc;
    if (map)
      if (int rc = alloc_map(c)) return rc;
    if (top)
      if (int rc = alloc_top(c)) return rc;
  }
  if (!npods) rep = Reports{};
  return submit ? submit_run(c, pods, npods, seq, out, rep, ticket) : schedule_run(c, pods, npods, seq, out, rep);
}
}  // namespace

int gs_schedule_diag(gs_ctx* c, const gs_pod* pods, uint32_t npods, const uint64_t* seq, gs_placement* out,
                     gs_fit_diagnosis* diag) {
  return report_run(c, pods, npods, seq, out, ReportKind::DIAG, Reports{diag, nullptr, nullptr}, false, nullptr);
}

int gs_schedule_submit_diag(gs_ctx* c, const gs_pod* pods, uint32_t npods, const uint64_t* seq, gs_placement* out,
                            gs_fit_diagnosis* diag, uint64_t* ticket) {
  return report_run(c, pods, npods, seq, out, ReportKind::DIAG, Reports{diag, nullptr, nullptr}, true, ticket);
}

int gs_schedule_diag_nodes(gs_ctx* c, const gs_pod* pods, uint32_t npods, const uint64_t* seq, gs_placement* out,
                           gs_fit_diagnosis* diag, gs_status_map* map) {
  return report_run(c, pods, npods, seq, out, ReportKind::DIAG_NODES, Reports{diag, map, nullptr}, false, nullptr);
}

int gs_schedule_submit_diag_nodes(gs_ctx* c, const gs_pod* pods, uint32_t npods, const uint64_t* seq, gs_placement* out,
                                  gs_fit_diagnosis* diag, gs_status_map* map, uint64_t* ticket) {
  return report_run(c, pods, npods, seq, out, ReportKind::DIAG_NODES, Reports{diag, map, nullptr}, true, ticket);
}

int gs_schedule_top_scores(gs_ctx* c, const gs_pod* pods, uint32_t npods, const uint64_t* seq, gs_placement* out,
                           gs_top_scores* top) {
  return report_run(c, pods, npods, seq, out, ReportKind::TOP, Reports{nullptr, nullptr, top}, false, nullptr);
}

int gs_schedule_submit_top_scores(gs_ctx* c, const gs_pod* pods, uint32_t npods, const uint64_t* seq, gs_placement* out,
                                  gs_top_scores* top, uint64_t* ticket) {
  return report_run(c, pods, npods, seq, out, ReportKind::TOP, Reports{nullptr, nullptr, top}, true, ticket);
}

int gs_status_framework_code(uint16_t word) { return gs_reason_string(GS_STATUS_CODE(word), 0, nullptr, nullptr, 0); }

int gs_preemption_candidates(const uint16_t* row, uint32_t num_nodes, uint32_t* nodes, uint32_t cap) {
  if (!row || (cap && !nodes)) return GS_EINVAL;
  uint32_t n = 0;
  uint16_t last = 0;   // (a row holds few distinct words, mostly in runs: the last word's code is kept)
  int last_code = 0;
  for (uint32_t i = 0; i < num_nodes; ++i) {
    if (row[i] != last) {
      last = row[i];
      last_code = gs_status_framework_code(last);
    }
    if (last_code == 2) continue;
    if (n < cap) nodes[n] = i;
    ++n;
  }
  return (int)n;
}

// ---- the resident-pod table and the ElasticQuota PostFilter dry run (gs_preempt.hip, gs_preempt.cpp) ----
namespace {
PreemptState* preempt_state(gs_ctx* c) {
  if (!c->pre) c->pre = std::make_unique<PreemptState>(c->N);
  return c->pre.get();
}

PreemptState::Pdb* pdb_state(gs_ctx* c) {
  PreemptState* ps = preempt_state(c);
  if (!ps->pdb) ps->pdb = std::make_unique<PreemptState::Pdb>();
  return ps->pdb.get();
}

// pre_potential (the kernel's potential-node test) against gs_status_framework_code, over every status word, once
bool potential_test_agrees() {
  static const bool ok = [] {
    for (uint32_t w = 0; w < 0x10000u; ++w)
      if (pre_potential(w) != (gs_status_framework_code((uint16_t)w) != 2)) return false;
    return true;
  }();
  return ok;
}
}  // namespace

int gs_node_pods_add(gs_ctx* c, const uint32_t* node_idx, const gs_resident_pod* pods, uint32_t n) {
  if (!c || (n && (!node_idx || !pods))) return GS_EINVAL;
  quiesce(c);
  PreemptState* ps = preempt_state(c);
  // the whole call is checked first: pods the call itself adds count towards the node's limit and its uids
  std::unordered_map<uint32_t, std::vector<uint64_t>> added;
  for (uint32_t i = 0; i < n; ++i) {
    if (node_idx[i] >= c->N) return fail(c, GS_EINVAL, "resident pod %u: node %u out of range", i, node_idx[i]);
    const char* why = "";
    if (int rc = ps->table.check_add(node_idx[i], pods[i], &why)) return fail(c, rc, "resident pod %u: %s", i, why);
    std::vector<uint64_t>& a = added[node_idx[i]];
    if (std::find(a.begin(), a.end(), pods[i].uid) != a.end())
      return fail(c, GS_EINVAL, "resident pod %u: the node already holds a resident pod with this uid", i);
    if (ps->table.count(node_idx[i]) + a.size() >= GS_MAX_NODE_PODS)
      return fail(c, GS_EUNSUPPORTED, "resident pod %u: a node holds at most GS_MAX_NODE_PODS resident pods", i);
    a.push_back(pods[i].uid);
  }
  for (uint32_t i = 0; i < n; ++i) ps->table.add(node_idx[i], pods[i]);
  return GS_OK;
}

int gs_node_pods_remove(gs_ctx* c, const uint32_t* node_idx, const uint64_t* uids, uint32_t n) {
  if (!c || (n && (!node_idx || !uids))) return GS_EINVAL;
  quiesce(c);
  PreemptState* ps = preempt_state(c);
  for (uint32_t i = 0; i < n; ++i)
    if (node_idx[i] >= c->N) return fail(c, GS_EINVAL, "resident pod %u: node %u out of range", i, node_idx[i]);
  for (uint32_t i = 0; i < n; ++i) ps->table.remove(node_idx[i], uids[i]);
  return GS_OK;
}

int gs_node_pods_get(gs_ctx* c, uint32_t node, gs_resident_pod* out, uint32_t cap) {
  if (!c || node >= c->N || (cap && !out)) return GS_EINVAL;
  quiesce(c);
  if (!c->pre) return 0;
  const uint32_t cnt = c->pre->table.count(node);
  const PreRec* r = c->pre->table.records(node);
  for (uint32_t j = 0; j < cnt && j < cap; ++j) {
    gs_resident_pod& o = out[j];
    std::memset(&o, 0, sizeof(o));
    o.uid = r[j].uid;
    o.start_time_ns = r[j].start;
    for (int s = 0; s < 7; ++s) o.requests[s] = r[j].req[s];
    for (int d = 0; d < GS_QUOTA_DIMS; ++d) o.quota_request[d] = r[j].qreq[d];
    o.quota_request_mask = r[j].qmask;
    o.priority = r[j].priority;
    o.quota = r[j].quota;
    o.flags = r[j].flags;
  }
  return (int)cnt;
}

int gs_pdbs_upsert(gs_ctx* c, const uint32_t* ids, const int32_t* disruptions_allowed, uint32_t n) {
  if (!c || (n && (!ids || !disruptions_allowed))) return GS_EINVAL;
  quiesce(c);
  for (uint32_t i = 0; i < n; ++i)
    if (ids[i] >= GS_MAX_PDBS) return fail(c, GS_EINVAL, "PDB %u: id %u is not below GS_MAX_PDBS", i, ids[i]);
  PreemptState::Pdb* pd = pdb_state(c);
  for (uint32_t i = 0; i < n; ++i) pd->table.set(ids[i], disruptions_allowed[i]);
  return GS_OK;
}

int gs_node_pods_set_pdbs(gs_ctx* c, const uint32_t* node_idx, const uint64_t* uids, const uint16_t* pdb_ids, uint32_t n) {
  if (!c || (n && (!node_idx || !uids || !pdb_ids))) return GS_EINVAL;
  quiesce(c);
  // the whole call is checked first, before any state is created (a uint16_t entry is an id below GS_MAX_PDBS or
  // GS_PDB_NONE: there is no third kind to refuse)
  for (uint32_t i = 0; i < n; ++i) {
    if (node_idx[i] >= c->N) return fail(c, GS_EINVAL, "PDB list %u: node %u out of range", i, node_idx[i]);
    if (!c->pre || !c->pre->table.find(node_idx[i], uids[i]))
      return fail(c, GS_EINVAL, "PDB list %u: the node holds no resident pod with this uid", i);
    const uint16_t* l = pdb_ids + (size_t)i * GS_MAX_POD_PDBS;
    for (int q = 0; q < GS_MAX_POD_PDBS; ++q)
      for (int r = 0; r < q && l[q] != GS_PDB_NONE; ++r)
        if (l[r] == l[q]) return fail(c, GS_EINVAL, "PDB list %u: id %u is repeated", i, (unsigned)l[q]);
  }
  pdb_state(c);
  PreemptTable& tb = c->pre->table;
  for (uint32_t i = 0; i < n; ++i) tb.set_pdbs(node_idx[i], uids[i], pdb_ids + (size_t)i * GS_MAX_POD_PDBS);
  return GS_OK;
}

int gs_node_pods_get_pdbs(gs_ctx* c, uint32_t node, uint16_t* out, uint32_t cap) {
  if (!c || node >= c->N || (cap && !out)) return GS_EINVAL;
  quiesce(c);
  if (!c->pre) return 0;
  const uint32_t cnt = c->pre->table.count(node);
  const PreRec* r = c->pre->table.records(node);
  for (uint32_t j = 0; j < cnt && j < cap; ++j)
    for (int q = 0; q < GS_MAX_POD_PDBS; ++q) out[(size_t)j * GS_MAX_POD_PDBS + q] = r[j].pdb[q];
  return (int)cnt;
}

namespace {
// gs_preempt_dry_run (out) and gs_preempt_dry_run_pdb (out_pdb): one of the two results, and the detail's arrays
struct DryRunOut {
  gs_preempt_result* out = nullptr;
  gs_preempt_result_pdb* out_pdb = nullptr;
  bool detail = false;
  uint8_t* node_status = nullptr;
  uint64_t* victim_bits = nullptr;
  uint64_t* violating_bits = nullptr;
  uint8_t* pdb_violations = nullptr;
};
int preempt_dry_run(gs_ctx* c, const gs_preemptor* p, uint32_t n, const uint16_t* rows, uint32_t num_rows, const DryRunOut& dst);
}  // namespace

int gs_preempt_dry_run(gs_ctx* c, const gs_preemptor* p, uint32_t n, const uint16_t* rows, uint32_t num_rows,
                       gs_preempt_result* out, gs_preempt_detail* detail) {
  if (!c || (n && (!p || !out))) return GS_EINVAL;
  DryRunOut dst;
  dst.out = out;
  if (detail) {
    dst.detail = true;
    dst.node_status = detail->node_status;
    dst.victim_bits = detail->victim_bits;
  }
  return preempt_dry_run(c, p, n, rows, num_rows, dst);
}

int gs_preempt_dry_run_pdb(gs_ctx* c, const gs_preemptor* p, uint32_t n, const uint16_t* rows, uint32_t num_rows,
                           gs_preempt_result_pdb* out, gs_preempt_detail_pdb* detail) {
  if (!c || (n && (!p || !out))) return GS_EINVAL;
  DryRunOut dst;
  dst.out_pdb = out;
  if (detail) {
    dst.detail = true;
    dst.node_status = detail->node_status;
    dst.victim_bits = detail->victim_bits;
    dst.violating_bits = detail->violating_bits;
    dst.pdb_violations = detail->pdb_violations;
  }
  return preempt_dry_run(c, p, n, rows, num_rows, dst);
}

namespace {
int preempt_dry_run(gs_ctx* c, const gs_preemptor* p, uint32_t n, const uint16_t* rows, uint32_t num_rows, const DryRunOut& dst) {
  const bool pdb = dst.out_pdb != nullptr;
  quiesce(c);
  // refusals, before any work: the dry run reads one rank's whole mirror, and the extension plugins' AddPod /
  // RemovePod (DeviceShare, Reservation) are not restated
  if (c->nranks > 1) return fail(c, GS_EUNSUPPORTED, "preemption dry run: several ranks are not supported");
  if (c->ext_configured) return fail(c, GS_EUNSUPPORTED, "preemption dry run: a context with gs_ext_configure is not supported");
  if (n > (uint32_t)MAX_BATCH) return fail(c, GS_EINVAL, "preemption dry run: at most %d preemptors per call", MAX_BATCH);
  if (dst.detail && n && (!dst.node_status || !dst.victim_bits || (pdb && (!dst.violating_bits || !dst.pdb_violations))))
    return fail(c, GS_EINVAL, "preemption dry run: a detail without its arrays");
  if (!n) return GS_OK;
  int rc = ready(c);
  if (rc) return rc;
  const uint32_t N = c->N;
  for (uint32_t k = 0; k < n; ++k) {
    if ((rc = validate_pod(c, p[k].pod))) return rc;
    if (p[k].row >= 0 && (!rows || (uint32_t)p[k].row >= num_rows))
      return fail(c, GS_EINVAL, "preemptor %u: row %d outside the %u status rows", k, p[k].row, num_rows);
    if (p[k].row < -1 || p[k].nominated_node < -1 || (p[k].nominated_node >= 0 && (uint32_t)p[k].nominated_node >= N))
      return fail(c, GS_EINVAL, "preemptor %u: row or nominated node out of range", k);
    for (int d = 0; d < GS_QUOTA_DIMS; ++d)
      if (std::llabs(p[k].used[d]) >= kMaxExact || std::llabs(p[k].used_limit[d]) >= kMaxExact ||
          std::llabs(p[k].quota_request[d]) >= kMaxExact)
        return fail(c, GS_EUNSUPPORTED, "preemptor %u: a quota quantity beyond 2^53", k);
  }
  if (!potential_test_agrees()) return fail(c, GS_ESTATE, "preemption dry run: the potential-node test disagrees with gs_status_framework_code");
  PreemptState* ps = preempt_state(c);
  PreemptState::Pdb* pd = pdb ? pdb_state(c) : nullptr;
  const PreemptTable& tb = ps->table;
  if ((rc = flush_rows(c))) return rc;
  if ((rc = node_prep(c))) return rc;
  const hipStream_t st = c->st.get();
  // nothing of an earlier run or dry run is in flight when the image and the buffers change
  for (const Stream* s : {&c->st_ev, &c->st_rb})
    if (*s) HIP_TRY(c, host_wait_stream(s->get()));
  HIP_TRY(c, host_wait_stream(st));

  // step 1, PodEligibleToPreemptOthers (preempt.go:61-94), and the preemptors' device vectors; the status rows the
  // call names, compacted
  std::vector<PrePod> hp(n);
  std::vector<int32_t> row_map(num_rows, -1);
  std::vector<uint32_t> used_rows;
  for (uint32_t k = 0; k < n; ++k) {
    const gs_preemptor& q = p[k];
    PrePod& d = hp[k];
    std::memset(&d, 0, sizeof(d));
    d.v = prep_pod(c, q.pod);
    d.skip = q.quota < 0;
    d.check = d.skip ? 0u : (q.quota_request_mask & q.limit_mask & 0xFFu);
    for (int j = 0; j < GS_QUOTA_DIMS; ++j) {
      d.qreq[j] = (d.check >> j & 1u) ? q.quota_request[j] : 0;
      d.used[j] = q.used[j];
      d.limit[j] = q.used_limit[j];
    }
    d.priority = q.priority;
    d.quota = q.quota;
    bool eligible = !(q.flags & GS_PREEMPT_NEVER);
    if (eligible && q.nominated_node >= 0) {
      const uint32_t nom = (uint32_t)q.nominated_node;
      const bool unresolvable = q.row >= 0 && !pre_potential(rows[(size_t)q.row * N + nom]);
      if (!unresolvable) {
        const PreRec* r = tb.records(nom);
        for (uint32_t j = 0; j < tb.count(nom); ++j)
          if ((r[j].flags & GS_RESIDENT_TERMINATING) && r[j].quota == q.quota && r[j].priority < q.priority) eligible = false;
      }
    }
    d.active = eligible;
    d.row = -1;
    if (q.row >= 0) {
      if (row_map[q.row] < 0) {
        row_map[q.row] = (int32_t)used_rows.size();
        used_rows.push_back((uint32_t)q.row);
      }
      d.row = row_map[q.row];
    }
  }

  // the image, the policy-node list and the buffers
  HIP_TRY(c, ps->table.sync(st, ps->rebuild));
  ps->rebuild = false;
  if (pdb) {
    HIP_TRY(c, pd->table.sync(st, pd->rebuild));
    pd->rebuild = false;
  }
  if (c->numa_on) {
    std::vector<uint32_t> idx;
    for (uint32_t i = 0; i < N; ++i)
      if (c->numa[i].cfg.numa_topology_policy != GS_NUMA_POLICY_NONE) idx.push_back(i);
    if (idx != ps->numa_idx || (!idx.empty() && !ps->d_numa_idx)) {
      if (!idx.empty()) {
        HIP_TRY(c, ps->d_numa_idx.alloc(4 * idx.size()));
        HIP_TRY(c, hipMemcpy(ps->d_numa_idx.get(), idx.data(), 4 * idx.size(), hipMemcpyHostToDevice));
      }
      ps->numa_idx.swap(idx);
    }
  } else {
    ps->numa_idx.clear();
  }
  const uint32_t numa_n = (uint32_t)ps->numa_idx.size();
  const uint32_t nparts = preempt_parts(c->pf, N, numa_n);
  if (!ps->d_pods) {
    HIP_TRY(c, ps->d_pods.alloc(sizeof(PrePod) * MAX_BATCH));
    HIP_TRY(c, ps->d_result.alloc(sizeof(PrePart) * MAX_BATCH));
  }
  if (used_rows.size() > ps->rows_cap) {
    HIP_TRY(c, ps->d_rows.alloc(used_rows.size() * (size_t)N * 2));
    ps->rows_cap = used_rows.size();
  }
  if (n > ps->out_cap) {
    HIP_TRY(c, ps->d_status.alloc((size_t)n * N));
    HIP_TRY(c, ps->d_bits.alloc((size_t)n * N * 16));
    ps->out_cap = n;
  }
  if (!pdb && (size_t)n * nparts > ps->parts_cap) {
    HIP_TRY(c, ps->d_parts.alloc((size_t)n * nparts * sizeof(PrePart)));
    ps->parts_cap = (size_t)n * nparts;
  }
  if (pdb) {
    if (!pd->d_result) HIP_TRY(c, pd->d_result.alloc(sizeof(PrePartPdb) * MAX_BATCH));
    if (n > pd->out_cap) {
      HIP_TRY(c, pd->d_viol.alloc((size_t)n * N * 16));
      HIP_TRY(c, pd->d_nviol.alloc((size_t)n * N));
      pd->out_cap = n;
    }
    if ((size_t)n * nparts > pd->parts_cap) {
      HIP_TRY(c, pd->d_parts.alloc((size_t)n * nparts * sizeof(PrePartPdb)));
      pd->parts_cap = (size_t)n * nparts;
    }
  }
  HIP_TRY(c, hipMemcpyAsync(ps->d_pods.get(), hp.data(), sizeof(PrePod) * n, hipMemcpyHostToDevice, st));
  for (size_t r = 0; r < used_rows.size(); ++r)
    HIP_TRY(c, hipMemcpyAsync(ps->d_rows.get() + r * N, rows + (size_t)used_rows[r] * N, (size_t)N * 2, hipMemcpyHostToDevice, st));

  PreemptArgs a{};
  a.m = c->mv;
  a.pf = c->pf;
  a.N = N;
  a.npre = (int)n;
  a.pods = ps->d_pods.get();
  a.rows = ps->d_rows.get();
  a.recs = tb.d_recs();
  a.segs = tb.d_segs();
  a.numa_idx = ps->d_numa_idx.get();
  a.numa_n = numa_n;
  a.status = ps->d_status.get();
  a.bits = ps->d_bits.get();
  a.parts = ps->d_parts.get();
  a.nparts = nparts;
  a.result = ps->d_result.get();
  std::vector<PrePart> res(pdb ? 0 : n);
  std::vector<PrePartPdb> res_pdb(pdb ? n : 0);
  if (pdb) {
    a.budgets = pd->table.d_allowed();
    a.viol = pd->d_viol.get();
    a.nviol = pd->d_nviol.get();
    a.parts_pdb = pd->d_parts.get();
    a.result_pdb = pd->d_result.get();
    HIP_TRY(c, launch_preempt_pdb(a, st));
    HIP_TRY(c, hipMemcpyAsync(res_pdb.data(), pd->d_result.get(), sizeof(PrePartPdb) * n, hipMemcpyDeviceToHost, st));
  } else {
    HIP_TRY(c, launch_preempt(a, st));
    HIP_TRY(c, hipMemcpyAsync(res.data(), ps->d_result.get(), sizeof(PrePart) * n, hipMemcpyDeviceToHost, st));
  }
  if (dst.detail) {
    HIP_TRY(c, hipMemcpyAsync(dst.node_status, ps->d_status.get(), (size_t)n * N, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipMemcpyAsync(dst.victim_bits, ps->d_bits.get(), (size_t)n * N * 16, hipMemcpyDeviceToHost, st));
    if (pdb) {
      HIP_TRY(c, hipMemcpyAsync(dst.violating_bits, pd->d_viol.get(), (size_t)n * N * 16, hipMemcpyDeviceToHost, st));
      HIP_TRY(c, hipMemcpyAsync(dst.pdb_violations, pd->d_nviol.get(), (size_t)n * N, hipMemcpyDeviceToHost, st));
    }
  }
  HIP_TRY(c, host_wait_stream(st));

  // the results; the chosen node's victim bits expanded into uids from the host table
  for (uint32_t k = 0; pdb && k < n; ++k) {
    gs_preempt_result_pdb& o = dst.out_pdb[k];
    std::memset(&o, 0, sizeof(o));
    o.node = -1;
    const PrePartPdb& r = res_pdb[k];
    if (!hp[k].active) {
      o.status = GS_PREEMPT_NOT_ELIGIBLE;
      continue;
    }
    o.num_potential = r.npot;
    o.num_candidates = r.ncand;
    o.num_errors = r.nerr;
    if (!r.npot) o.status = GS_PREEMPT_NO_POTENTIAL_NODES;
    else if (r.key.valid) {
      o.status = GS_PREEMPT_NOMINATED;
      o.node = r.key.node;
      o.num_pdb_violations = r.key.nviol;
      const PreRec* recs = tb.records((uint32_t)r.key.node);
      const uint32_t cnt = tb.count((uint32_t)r.key.node);
      // the reference's slice order: the violating group's victims, then the non-violating group's
      for (uint64_t group : {~0ull, 0ull})
        for (uint32_t j = 0; j < cnt && j < GS_MAX_NODE_PODS; ++j) {
          const uint64_t bit = 1ull << (j & 63);
          if ((r.bits[j >> 6] & bit) && (r.viol[j >> 6] & bit) == (group & bit)) o.victims[o.num_victims++] = recs[j].uid;
        }
      if (o.num_victims != r.key.nvict) return fail(c, GS_ESTATE, "preemption dry run: victim bits and count disagree");
    } else {
      o.status = r.nerr ? GS_PREEMPT_ERROR : GS_PREEMPT_NO_CANDIDATES;
    }
  }
  for (uint32_t k = 0; !pdb && k < n; ++k) {
    gs_preempt_result& o = dst.out[k];
    std::memset(&o, 0, sizeof(o));
    o.node = -1;
    const PrePart& r = res[k];
    if (!hp[k].active) {
      o.status = GS_PREEMPT_NOT_ELIGIBLE;
      continue;
    }
    o.num_potential = r.npot;
    o.num_candidates = r.ncand;
    o.num_errors = r.nerr;
    if (!r.npot) o.status = GS_PREEMPT_NO_POTENTIAL_NODES;
    else if (r.key.valid) {
      o.status = GS_PREEMPT_NOMINATED;
      o.node = r.key.node;
      const PreRec* recs = tb.records((uint32_t)r.key.node);
      const uint32_t cnt = tb.count((uint32_t)r.key.node);
      for (uint32_t j = 0; j < cnt && j < GS_MAX_NODE_PODS; ++j)
        if (r.bits[j >> 6] >> (j & 63) & 1ull) o.victims[o.num_victims++] = recs[j].uid;
      if (o.num_victims != r.key.nvict) return fail(c, GS_ESTATE, "preemption dry run: victim bits and count disagree");
    } else {
      o.status = r.nerr ? GS_PREEMPT_ERROR : GS_PREEMPT_NO_CANDIDATES;
    }
  }
  return GS_OK;
}
}  // namespace

int gs_schedule_wait(gs_ctx* c, uint64_t ticket) {
  if (!c || !c->aq) return GS_EINVAL;
  AsyncQueue& q = *c->aq;
  std::unique_lock<std::mutex> lk(q.mu);
  auto it = q.runs.find(ticket);
  if (it == q.runs.end()) return GS_EINVAL;
  std::shared_ptr<AsyncRun> r = it->second;
  q.cv_done.wait(lk, [&] { return r->rc != 1; });
  q.runs.erase(it);
  if (r->rc) {
    q.cv_done.wait(lk, [&] { return q.pending.empty() && !q.busy; });   // the worker has stopped writing c->err
    c->err = r->err;
  }
  return r->rc;
}

void gs_numa_args_default(gs_numa_args* a) {
  if (!a) return;
  std::memset(a, 0, sizeof(*a));
  a->default_cpu_bind_policy = GS_CPU_BIND_FULL_PCPUS;   // defaults.go:50,103-106
  a->scoring_type = GS_SCORING_LEAST_ALLOCATED;
  a->numa_scoring_type = GS_SCORING_LEAST_ALLOCATED;
  a->resource_weights[GS_RES_CPU] = 1;
  a->resource_weights[GS_RES_MEMORY] = 1;
}

int gs_topology_register(gs_ctx* c, const gs_cpu_topology* t, int32_t* id) {
  if (!c || !t || !id) return GS_EINVAL;
  quiesce(c);
  const char* err = nullptr;
  auto topo = make_topo(*t, &err);
  if (!topo) return fail(c, GS_EUNSUPPORTED, "gs_topology_register: %s", err ? err : "invalid topology");
  c->topos.push_back(topo);
  *id = (int32_t)c->topos.size() - 1;
  // device copy of every registered topology's TopoDev (index = topology id)
  std::vector<TopoDev> all(c->topos.size());
  for (size_t i = 0; i < all.size(); ++i) all[i] = c->topos[i]->dev;
  HIP_TRY(c, host_wait_stream(c->st.get()));
  HIP_TRY(c, c->d_topos.alloc(sizeof(TopoDev) * all.size()));   // (frees the old copy: the wait above covers it)
  HIP_TRY(c, hipMemcpy(c->d_topos.get(), all.data(), sizeof(TopoDev) * all.size(), hipMemcpyHostToDevice));
  return GS_OK;
}

int gs_nodes_numa_upsert(gs_ctx* c, const uint32_t* idx, const gs_node_numa* nn, uint32_t n) {
  if (!c || (!nn && n)) return GS_EINVAL;
  quiesce(c);
  for (uint32_t j = 0; j < n; ++j) {
    uint32_t i = idx ? idx[j] : j;
    if (i >= c->N) return fail(c, GS_EINVAL, "node index %u >= %u", i, c->N);
    const gs_node_numa& x = nn[j];
    if (x.num_zones < 0 || x.num_zones > GS_MAX_NUMA)
      return fail(c, GS_EUNSUPPORTED, "node %u: %d NUMA zones (device path supports <= %d)", i, x.num_zones, GS_MAX_NUMA);
    for (int z = 0; z < x.num_zones; ++z) {
      if (x.zones[z].node_id < 0 || x.zones[z].node_id >= 64 || (z && x.zones[z].node_id <= x.zones[z - 1].node_id))
        return fail(c, GS_EINVAL, "node %u: NUMA zones must be sorted by distinct node id in [0,64)", i);
      if (x.zones[z].cpu_milli < 0 || x.zones[z].memory < 0 || x.zones[z].cpu_milli >= kMaxExact || x.zones[z].memory >= kMaxExact)
        return fail(c, GS_EUNSUPPORTED, "node %u: NUMA zone quantity outside [0, 2^53)", i);
    }
    if (x.numa_topology_policy < 0 || x.numa_topology_policy > 3 || x.node_cpu_bind_policy < 0 ||
        x.node_cpu_bind_policy > 2 || x.numa_allocate_strategy < 0 || x.numa_allocate_strategy > 3)
      return fail(c, GS_EINVAL, "node %u: policy enum out of range", i);
    if (x.has_options && x.topology >= (int32_t)c->topos.size())
      return fail(c, GS_EINVAL, "node %u: topology id %d not registered", i, x.topology);
    NumaNode& st = c->numa[i];
    if (st.cfg.numa_topology_policy != x.numa_topology_policy) c->numa_idx_stale = c->xnuma_stale = true;
    st.cfg = x;
    if (c->devs[i].has_device) dev_mark(c, i);   // its GPUs' zone slots (dev_image)
    st.topo = !x.has_options ? nullptr : (x.topology >= 0 ? c->topos[x.topology] : c->empty_topo);
    mark_dirty(c, i);
  }
  return flush_rows(c);
}

int gs_numa_allocations_update(gs_ctx* c, const uint32_t* node_idx, const gs_pod_allocation* a, uint32_t n) {
  if (!c || (n && (!node_idx || !a))) return GS_EINVAL;
  quiesce(c);
  for (uint32_t j = 0; j < n; ++j) {
    uint32_t i = node_idx[j];
    if (i >= c->N) return fail(c, GS_EINVAL, "node index %u >= %u", i, c->N);
    NumaNode& st = c->numa[i];
    if (!st.topo_valid()) continue;   // resourceManager.Update (resource_manager.go:362-373)
    PodAllocRec rec;
    rec.uid = a[j].uid;
    for (int w = 0; w < GS_CPU_WORDS; ++w) rec.cpus.w[w] = a[j].cpuset[w];
    rec.excl = a[j].cpu_exclusive_policy;
    if (a[j].num_numa < 0 || a[j].num_numa > GS_MAX_NUMA) return fail(c, GS_EINVAL, "num_numa out of range");
    for (int z = 0; z < a[j].num_numa; ++z) rec.numa.push_back(a[j].numa[z]);
    numa_release(st, rec.uid);
    numa_add(st, rec);
    c->numa_uid_node[rec.uid] = i;
    mark_dirty(c, i);
  }
  return flush_rows(c);
}

int gs_numa_allocations_release(gs_ctx* c, const uint32_t* node_idx, const uint64_t* uids, uint32_t n) {
  if (!c || (n && (!node_idx || !uids))) return GS_EINVAL;
  quiesce(c);
  for (uint32_t j = 0; j < n; ++j) {
    uint32_t i = node_idx[j];
    if (i >= c->N) return fail(c, GS_EINVAL, "node index %u >= %u", i, c->N);
    numa_release(c->numa[i], uids[j]);
    auto it = c->numa_uid_node.find(uids[j]);
    if (it != c->numa_uid_node.end() && it->second == i) c->numa_uid_node.erase(it);
    mark_dirty(c, i);
  }
  return flush_rows(c);
}

int gs_numa_allocation_get(gs_ctx* c, uint32_t node, uint64_t uid, gs_pod_allocation* out) {
  if (!c || !out || node >= c->N) return GS_EINVAL;
  quiesce(c);
  const NumaNode& st = c->numa[node];
  auto it = st.pods.find(uid);
  if (it == st.pods.end()) return 0;
  std::memset(out, 0, sizeof(*out));
  out->uid = uid;
  for (int w = 0; w < GS_CPU_WORDS; ++w) out->cpuset[w] = it->second.cpus.w[w];
  out->cpu_exclusive_policy = it->second.excl;
  out->num_numa = (int32_t)std::min<size_t>(it->second.numa.size(), GS_MAX_NUMA);
  for (int z = 0; z < out->num_numa; ++z) out->numa[z] = it->second.numa[z];
  return 1;
}

int gs_comm_unique_id(uint8_t out[128]) {
  if (!out) return GS_EINVAL;
  ncclUniqueId id;
  if (ncclGetUniqueId(&id) != ncclSuccess) return GS_ECOMM;
  static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId size");
  std::memcpy(out, &id, 128);
  return GS_OK;
}

int gs_comm_init_rccl(gs_ctx* c, const uint8_t id[128], int nranks, int rank) {
  if (!c || !id || nranks < 1 || nranks > MAX_RANKS || rank < 0 || rank >= nranks) return GS_EINVAL;
  quiesce(c);
  // node sampling's rotation window needs every node's Filter verdict on every rank: the score rows carry them
  if (c->window_k && nranks > 1 && xchg_levels())
    return fail(c, GS_EUNSUPPORTED, "node sampling on several ranks needs the score-row exchange");
  if (nranks > 1) {
    ncclUniqueId uid;
    std::memcpy(&uid, id, 128);
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    ncclResult_t r = ncclCommInitRank(&c->comm, nranks, uid, rank);
    if (r != ncclSuccess) return fail(c, GS_ECOMM, "ncclCommInitRank: %s", ncclGetErrorString(r));
  }
  c->nranks = nranks;
  c->rank = rank;
  if (int rc = reshard(c)) return rc;
  c->numa_idx_stale = c->xnuma_stale = true;
  return alloc_exchange(c);
}

int gs_comm_init_callback(gs_ctx* c, int nranks, int rank, gs_allgather_fn fn, void* user) {
  if (!c || !fn || nranks < 1 || nranks > MAX_RANKS || rank < 0 || rank >= nranks) return GS_EINVAL;
  quiesce(c);
  // node sampling's rotation window needs every node's Filter verdict on every rank: the score rows carry them
  if (c->window_k && nranks > 1 && xchg_levels())
    return fail(c, GS_EUNSUPPORTED, "node sampling on several ranks needs the score-row exchange");
  c->cb = fn;
  c->cb_user = user;
  c->nranks = nranks;
  c->rank = rank;
  if (int rc = reshard(c)) return rc;
  c->numa_idx_stale = c->xnuma_stale = true;
  return alloc_exchange(c);
}

int gs_local_group_create(int nranks, gs_local_group** out) {
  if (!out || nranks < 1 || nranks > MAX_RANKS) return GS_EINVAL;
  gs_local_group* g = new gs_local_group;
  g->n = nranks;
  g->send.assign(nranks, nullptr);
  g->bytes.assign(nranks, 0);
  g->ready.assign(nranks, nullptr);
  g->done.assign(nranks, nullptr);
  *out = g;
  return GS_OK;
}

int gs_local_group_destroy(gs_local_group* g) {
  delete g;
  return GS_OK;
}

int gs_comm_init_local(gs_ctx* c, gs_local_group* g, int rank) {
  if (!c || !g || rank < 0 || rank >= g->n) return GS_EINVAL;
  quiesce(c);
  if (c->window_k && g->n > 1 && xchg_levels())
    return fail(c, GS_EUNSUPPORTED, "node sampling on several ranks needs the score-row exchange");
  HIP_TRY(c, hipSetDevice(c->cfg.device));
  if (!c->lg_ready) HIP_TRY(c, c->lg_ready.create(hipEventDisableTiming));
  if (!c->lg_done) HIP_TRY(c, c->lg_done.create(hipEventDisableTiming));
  c->lg = g;
  c->nranks = g->n;
  c->rank = rank;
  if (int rc = reshard(c)) return rc;
  c->numa_idx_stale = c->xnuma_stale = true;
  return alloc_exchange(c);
}

int gs_get_stats(gs_ctx* c, gs_stats* out) {
  if (!c || !out) return GS_EINVAL;
  quiesce(c);
  *out = c->stats;
  out->next_start_node_index = c->next_start;
  return GS_OK;
}

int gs_reset_stats(gs_ctx* c) {
  if (!c) return GS_EINVAL;
  quiesce(c);
  uint64_t rb = c->stats.node_row_bytes;   // keep
  c->stats = gs_stats{};
  c->stats.node_row_bytes = rb;
  c->stats.shard_begin = c->n0;
  c->stats.shard_end = c->n1;
  return GS_OK;
}

int gs_synchronize(gs_ctx* c) {
  if (!c) return GS_EINVAL;
  quiesce(c);
  HIP_TRY(c, host_wait_stream(c->st_ev.get()));
  HIP_TRY(c, host_wait_stream(c->st.get()));
  HIP_TRY(c, host_wait_stream(c->st_rb.get()));
  return GS_OK;
}

// Device-error recovery (a GPU error becomes framework.Error, then the mirror is rebuilt from the
// host snapshot): drain the streams, re-derive every node row from the host state into HBM, re-run node prep.
int gs_reset(gs_ctx* c) {
  if (!c) return GS_EINVAL;
  quiesce(c);
  (void)host_wait_stream(c->st.get());
  (void)host_wait_stream(c->st_ev.get());
  (void)host_wait_stream(c->st2.get());
  (void)host_wait_stream(c->st_rb.get());
  (void)hipGetLastError();
  for (uint32_t i = 0; i < c->N; ++i)
    if (c->nodes[i].valid) mark_dirty(c, i);
  c->numa_idx_stale = c->xnuma_stale = true;
  if (c->d_dev)
    for (uint32_t i = 0; i < c->N; ++i) dev_mark(c, i);
  if (c->d_aux)
    for (uint32_t i = 0; i < c->N; ++i) aux_mark(c, i);
  int rc = flush_rows(c);
  if (!rc) rc = ext_flush_devices(c);
  if (!rc) rc = ext_flush_aux(c);
  if (rc) return rc;
  if ((rc = node_prep(c))) return rc;
  if (c->pre) c->pre->rebuild = true;   // the resident-pod image: rebuilt from the host table by the next dry run
  if (c->pre && c->pre->pdb) c->pre->pdb->rebuild = true;   // ... and the budget table
  hipError_t e = host_wait_stream(c->st.get());
  if (e != hipSuccess) return fail(c, GS_EDEVICE, "reset: the device is unusable (%s): destroy and recreate the context",
                                   hipGetErrorString(e));
  c->err.clear();
  return GS_OK;
}

int gs_debug_verify_cpuset(gs_ctx* c, int on) {
  if (!c) return GS_EINVAL;
  quiesce(c);
  c->verify_cpuset = on != 0;
  return GS_OK;
}

// Cycle cost of the commit kernel's pair evaluations on mirror rows (gs_probe.hip): n probes, probe i on node
// nodes[i] with pod pod_of[i] (modes 0, 2) or with pods 0..min(npods,64)-1 one per lane (mode 1).
int gs_debug_pair_probe(gs_ctx* c, const gs_pod* pods, uint32_t npods, const uint32_t* nodes, const int32_t* pod_of,
                        uint32_t n, int mode, int32_t* scores, uint64_t* cycles) {
  if (!c || !pods || !nodes || !pod_of || !scores || !cycles || npods == 0 || npods > 64 || mode < 0 || mode > 2)
    return GS_EINVAL;
  quiesce(c);
  int rc = ready(c);
  if (rc) return rc;
  if ((rc = flush_rows(c))) return rc;
  if (c->prep_stale && (rc = node_prep(c))) return rc;
  for (uint32_t i = 0; i < n; ++i)
    if (nodes[i] >= c->N || pod_of[i] < 0 || (uint32_t)pod_of[i] >= npods) return GS_EINVAL;
  std::vector<PodVec> pv(npods);
  int prod_cols = 0;
  for (uint32_t i = 0; i < npods; ++i) {
    if ((rc = validate_pod(c, pods[i]))) return rc;
    pv[i] = prep_pod(c, pods[i]);
    prod_cols |= (pv[i].flags & PF_PROD_SCORE) ? 1 : 0;
  }
  DevBuf<PodVec> d_p;
  DevBuf<uint32_t> d_n;
  DevBuf<int32_t> d_o, d_s;
  DevBuf<uint64_t> d_c;
  const size_t ns = (size_t)n * (mode == 1 ? 64 : 1);
  hipError_t e = d_p.alloc(sizeof(PodVec) * npods);
  if (e == hipSuccess) e = d_n.alloc(4 * n);
  if (e == hipSuccess) e = d_o.alloc(4 * n);
  if (e == hipSuccess) e = d_s.alloc(4 * ns);
  if (e == hipSuccess) e = d_c.alloc(80 * n);
  if (e == hipSuccess) e = hipMemset(d_c.get(), 0, 80 * n);
  if (e == hipSuccess) e = hipMemcpy(d_p.get(), pv.data(), sizeof(PodVec) * npods, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d_n.get(), nodes, 4 * n, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d_o.get(), pod_of, 4 * n, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = host_wait_stream(c->st.get());
  if (e == hipSuccess)
    e = launch_probe(mode, c->mv, c->pf, d_p.get(), (int)npods, d_n.get(), d_o.get(), n, prod_cols, d_s.get(), d_c.get(),
                     c->st.get());
  if (e == hipSuccess) e = host_wait_stream(c->st.get());
  if (e == hipSuccess) e = hipMemcpy(scores, d_s.get(), 4 * ns, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(cycles, d_c.get(), 80 * n, hipMemcpyDeviceToHost);
  if (e != hipSuccess) return fail(c, GS_EDEVICE, "probe: %s", hipGetErrorString(e));
  return GS_OK;
}

// The device merge on given hint lists (gs_probe.hip merge_probe_kernel).
int gs_debug_numa_merge(gs_ctx* c, const gs_merge_case* cases, uint32_t n, gs_merge_result* out) {
  if (!c || (n && (!cases || !out))) return GS_EINVAL;
  quiesce(c);
  for (uint32_t i = 0; i < n; ++i)
    if (cases[i].nz < 1 || cases[i].nz > 4 || cases[i].policy < GS_NUMA_POLICY_NONE ||
        cases[i].policy > GS_NUMA_POLICY_SINGLE_NUMA_NODE)
      return GS_EINVAL;
  if (!n) return GS_OK;   // (no mirror state involved: the merge's inputs are the cases)
  DevBuf<gs_merge_case> d_c;
  DevBuf<gs_merge_result> d_o;
  hipError_t e = d_c.alloc(sizeof(gs_merge_case) * n);
  if (e == hipSuccess) e = d_o.alloc(sizeof(gs_merge_result) * n);
  if (e == hipSuccess) e = hipMemcpy(d_c.get(), cases, sizeof(gs_merge_case) * n, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = host_wait_stream(c->st.get());
  if (e == hipSuccess) e = launch_merge_probe(d_c.get(), (int)n, d_o.get(), c->st.get());
  if (e == hipSuccess) e = host_wait_stream(c->st.get());
  if (e == hipSuccess) e = hipMemcpy(out, d_o.get(), sizeof(gs_merge_result) * n, hipMemcpyDeviceToHost);
  if (e != hipSuccess) return fail(c, GS_EDEVICE, "merge probe: %s", hipGetErrorString(e));
  return GS_OK;
}

// The speculative commit's event counters (the entries of a.stamps that count events, not cycles: the numbers
// report_commit_stamps prints): wave 0's region, and the prep wave's (region 1) for the split selector's first decisions.
int gs_debug_commit_counters(gs_ctx* c, gs_commit_counters* out) {
  if (!c || !out) return GS_EINVAL;
  quiesce(c);
  if (!c->d_stamps || c->window_k) return fail(c, GS_EINVAL, "commit counters: the context was created without GS_COMMIT_STAMPS=1, or with node sampling");
  std::vector<uint64_t> sa(524);
  HIP_TRY(c, host_wait_stream(c->st.get()));
  HIP_TRY(c, hipMemcpy(sa.data(), c->d_stamps.get(), 8 * 524, hipMemcpyDeviceToHost));
  // entries 47..50 are the split selector's exclusion counts or the single selector's late-landing estimate, and the
  // prep wave's region is a re-scoring wave's under the single selector: which of them ran is the host's knowledge
  const bool split = c->spec_split_launches > 0, single = c->spec_single_launches > 0;
  const uint64_t* w1 = sa.data() + 64;
  auto sp = [&](uint64_t v) { return split ? v : 0; };
  auto es = [&](uint64_t v) { return single && !split ? v : 0; };
  *out = gs_commit_counters{sa[9],      sa[3],      sa[41],     sa[40],     sa[10],     sa[36],     sa[31],
                            sa[24],     sa[25],     sa[42],     sa[43],     sa[44],     sa[45],     sp(sa[47]),
                            sp(sa[48]), sp(sa[49]), sp(sa[50]), sp(w1[9]),  sp(w1[36]), sp(w1[31]), sp(w1[24]),
                            sp(w1[25]), es(sa[47]), es(sa[48]), es(sa[49]), es(sa[50]), c->spec_split_launches,
                            c->spec_single_launches};
  return GS_OK;
}

// Compares every HBM mirror row against a fresh host derivation; returns the number of mismatching rows.
int gs_debug_mirror_check(gs_ctx* c) {
  if (!c) return GS_EINVAL;
  quiesce(c);
  int rc = flush_rows(c);
  if (rc) return rc;
  std::vector<int64_t> d64((size_t)c->npad * NUM_I64_COLS);
  std::vector<int32_t> d32((size_t)c->npad * NUM_I32_COLS);
  HIP_TRY(c, host_wait_stream(c->st.get()));
  HIP_TRY(c, hipMemcpy(d64.data(), c->mv.i64, d64.size() * 8, hipMemcpyDeviceToHost));
  HIP_TRY(c, hipMemcpy(d32.data(), c->mv.i32, d32.size() * 4, hipMemcpyDeviceToHost));
  int bad = 0;
  std::vector<int64_t> row(ROW_WORDS);
  for (uint32_t i = 0; i < c->N; ++i) {
    derive_row(c, i, row.data());
    bool ok = true;
    derive_row_numa(c, i, row.data());
    for (int k = 0; k < NUM_I64_COLS; ++k) ok &= d64[(size_t)k * c->npad + i] == row[k];
    for (int k = 0; k < NUM_I32_COLS; ++k)
      if (k != C_DFLAGS) ok &= d32[(size_t)k * c->npad + i] == (int32_t)row[NUM_I64_COLS + k];
    if (!ok) {
      if (bad < 4) fprintf(stderr, "gpuscore: mirror row %u differs from its host derivation\n", i);
      ++bad;
    }
  }
  return bad;
}

}  // extern "C"

// ---- Reservation + DeviceShare ----------------------------------------------------------------
extern "C" {

void gs_ext_args_default(gs_ext_args* a) {
  if (!a) return;
  std::memset(a, 0, sizeof(*a));
  a->enabled = GS_EXT_DEVICESHARE | GS_EXT_RESERVATION;
  a->device_scoring_type = GS_SCORING_LEAST_ALLOCATED;   // v1beta2 SetDefaults_DeviceShareArgs (defaults.go:187-203)
  a->device_weights[GS_GPU_MEMORY_RATIO] = 1;            // (its rdma weight has no GPU counterpart)
  a->weight_deviceshare = 1;                              // config/manager/scheduler-config.yaml:80-89
  a->weight_reservation = 5000;
}

int gs_ext_configure(gs_ctx* c, const gs_ext_args* a) {
  if (!c || !a) return GS_EINVAL;
  quiesce(c);
  if (a->enabled & ~(GS_EXT_DEVICESHARE | GS_EXT_RESERVATION)) return fail(c, GS_EINVAL, "unknown extension plugin bits");
  if (a->fit_ignored_gpu_names & ~0x1Fu) return fail(c, GS_EINVAL, "fit_ignored_gpu_names outside the GPU names");
  if (a->fit_ignored_xres & ~((1u << GS_MAX_XRES) - 1u))
    return fail(c, GS_EINVAL, "fit_ignored_xres outside the registered extended resources");
  if (a->device_scoring_type != GS_SCORING_LEAST_ALLOCATED && a->device_scoring_type != GS_SCORING_MOST_ALLOCATED)
    return fail(c, GS_EINVAL, "DeviceShare scoring strategy not supported");
  for (int r = 0; r < GS_NUM_GPU_RES; ++r)
    if (a->device_weights[r] < 0 || a->device_weights[r] > 100) return fail(c, GS_EINVAL, "DeviceShare weight out of range");
  if (a->weight_deviceshare < 0 || a->weight_reservation < 0 || a->weight_deviceshare > 100000 ||
      a->weight_reservation > 100000)
    return fail(c, GS_EINVAL, "extension plugin weights out of range");
  const bool rs_changed = (c->ext.enabled ^ a->enabled) & GS_EXT_RESERVATION;
  c->ext = *a;
  c->ext_configured = true;
  if (rs_changed)   // the mirror rows carry the unmatched restore only with the Reservation plugin on
    for (uint32_t i = 0; i < c->N; ++i)
      if (c->nodes[i].valid) mark_dirty(c, i);
  return GS_OK;
}

int gs_node_devices_upsert(gs_ctx* c, const uint32_t* idx, const gs_node_devices* d, uint32_t n) {
  if (!c || (n && !d)) return GS_EINVAL;
  quiesce(c);
  for (uint32_t k = 0; k < n; ++k) {
    const uint32_t i = idx ? idx[k] : k;
    if (i >= c->N) return fail(c, GS_EINVAL, "node index %u out of range", i);
    if (d[k].num_gpus < 0 || d[k].num_gpus > GS_MAX_GPUS) return fail(c, GS_EINVAL, "num_gpus out of range");
    for (int g = 0; g < d[k].num_gpus; ++g) {
      for (int h = 0; h < g; ++h)
        if (d[k].gpus[h].minor == d[k].gpus[g].minor) return fail(c, GS_EINVAL, "duplicate GPU minor on node %u", i);
      if (d[k].gpus[g].minor < 0 || d[k].gpus[g].minor > 31) return fail(c, GS_EUNSUPPORTED, "GPU minor outside 0..31");
      for (int r = 0; r < GS_NUM_GPU_RES; ++r)
        if (d[k].gpus[g].total[r] < 0 || d[k].gpus[g].used[r] < 0 || d[k].gpus[g].total[r] >= (1LL << 53))
          return fail(c, GS_EUNSUPPORTED, "GPU quantity outside [0, 2^53)");
    }
    for (int x = 0; x < GS_MAX_XRES; ++x)
      if (!in_range(d[k].xres_allocatable[x]) || !in_range(d[k].xres_requested[x]))
        return fail(c, GS_EUNSUPPORTED, "extended resource quantity outside the exact range (-2^53, 2^53)");
    c->devs[i] = d[k];
    dev_mark(c, i);
  }
  return GS_OK;
}

int gs_node_devices_get(gs_ctx* c, uint32_t node, gs_node_devices* out) {
  if (!c || !out || node >= c->N) return GS_EINVAL;
  quiesce(c);
  *out = c->devs[node];
  return GS_OK;
}

namespace {
void rsv_unindex(gs_ctx* c, const gs_reservation& r) {
  auto& v = c->rsv_node[r.node];
  v.erase(std::remove(v.begin(), v.end(), r.uid), v.end());
  auto it = c->rsv_owner.find(r.owner_key);
  if (it != c->rsv_owner.end()) {
    auto& o = it->second;
    o.erase(std::remove(o.begin(), o.end(), r.uid), o.end());
    if (o.empty()) c->rsv_owner.erase(it);
  }
  mark_dirty(c, r.node);
}
}  // namespace

int gs_reservations_upsert(gs_ctx* c, const gs_reservation* r, uint32_t n) {
  if (!c || (n && !r)) return GS_EINVAL;
  quiesce(c);
  for (uint32_t k = 0; k < n; ++k) {
    const gs_reservation& x = r[k];
    if (x.node >= c->N) return fail(c, GS_EINVAL, "reservation node %u out of range", x.node);
    if (x.allocate_policy < GS_RSV_POLICY_DEFAULT || x.allocate_policy > GS_RSV_POLICY_RESTRICTED)
      return fail(c, GS_EINVAL, "reservation allocate policy out of range");
    if ((x.allocatable_mask | x.allocated_mask | x.resource_names_mask) & ~0x7Fu)
      return fail(c, GS_EINVAL, "reservation resource keys outside slots 0..6");
    for (int s = 0; s < GS_NUM_RES; ++s)
      if (x.allocatable[s] < 0 || x.allocated[s] < 0 || x.allocatable[s] >= (1LL << 50) || x.allocated[s] >= (1LL << 50))
        return fail(c, GS_EUNSUPPORTED, "reservation quantity outside [0, 2^50)");
    auto it = c->rsv.find(x.uid);
    if (it != c->rsv.end()) rsv_unindex(c, it->second);
    c->rsv[x.uid] = x;
    auto& v = c->rsv_node[x.node];
    v.insert(std::lower_bound(v.begin(), v.end(), x.uid), x.uid);
    if (x.owner_key) {
      auto& o = c->rsv_owner[x.owner_key];
      o.insert(std::lower_bound(o.begin(), o.end(), x.uid), x.uid);
    }
    mark_dirty(c, x.node);
  }
  return GS_OK;
}

int gs_reservations_remove(gs_ctx* c, const uint64_t* uids, uint32_t n) {
  if (!c || (n && !uids)) return GS_EINVAL;
  quiesce(c);
  for (uint32_t k = 0; k < n; ++k) {
    auto it = c->rsv.find(uids[k]);
    if (it == c->rsv.end()) continue;
    rsv_unindex(c, it->second);
    c->rsv.erase(it);
  }
  return GS_OK;
}

int gs_reservation_get(gs_ctx* c, uint64_t uid, gs_reservation* out) {
  if (!c || !out) return GS_EINVAL;
  quiesce(c);
  auto it = c->rsv.find(uid);
  if (it == c->rsv.end()) return 0;
  *out = it->second;
  return 1;
}

int gs_ext_reserved_get(gs_ctx* c, uint64_t uid, uint32_t* node, gs_ext_placement* out) {
  if (!c || !node || !out) return GS_EINVAL;
  quiesce(c);
  auto it = c->ext_reserved.find(uid);
  if (it == c->ext_reserved.end()) return 0;
  const ExtReserved& x = it->second;
  *node = x.node;
  *out = gs_ext_placement{};
  out->reservation_uid = x.reservation_uid;
  out->gpu_minor_mask = x.gpu_minor_mask;
  out->gpu_count = x.gpu_count;
  for (int r = 0; r < GS_NUM_GPU_RES; ++r) out->gpu_per_instance[r] = x.gpu_per_instance[r];
  return 1;
}

int gs_schedule_ext_aux(gs_ctx* c, const gs_pod* pods, const gs_pod_ext* ext, const gs_pod_aux* aux, uint32_t npods,
                        const uint64_t* seq, gs_placement* out, gs_ext_placement* ext_out, gs_aux_placement* aux_out) {
  if (!c || (npods && (!pods || !out)) || (aux && !ext)) return GS_EINVAL;
  quiesce(c);
  int rc = ready(c);
  if (rc) return rc;
  for (uint32_t i = 0; i < npods; ++i)
    if ((rc = validate_pod(c, pods[i]))) return rc;
  uint32_t i = 0;
  while (i < npods) {
    // a run of plain pods goes through the batched path (both plugins score 0 for them; the mirror rows carry the
    // unmatched restore), an extension pod through the normalizing path
    uint32_t j = i;
    while (j < npods && !(ext && (c->ext.enabled || ext[j].xres_request_mask) &&
                          is_ext_pod(c, ext[j], aux ? &aux[j] : nullptr)))
      ++j;
    if (j > i) {
      std::vector<uint64_t> sq;
      if (!seq) { sq.resize(j - i); for (uint32_t k = i; k < j; ++k) sq[k - i] = k; }
      const auto hp0 = std::chrono::steady_clock::now();
      if ((rc = gs_schedule(c, pods + i, j - i, seq ? seq + i : sq.data(), out + i))) return rc;
      if (c->host_timing) {
        c->hx_plain += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - hp0).count();
        c->hx_runs += 1;
      }
      if (ext_out) std::memset(ext_out + i, 0, sizeof(gs_ext_placement) * (j - i));
      if (aux_out) std::memset(aux_out + i, 0, sizeof(gs_aux_placement) * (j - i));
      i = j;
      continue;
    }
    gs_ext_placement eo{};
    gs_aux_placement ao{};
    if ((rc = ext_schedule_one(c, pods[i], ext[i], aux ? &aux[i] : nullptr, seq ? seq[i] : i, &out[i], &eo, &ao)))
      return rc;
    if (ext_out) ext_out[i] = eo;
    if (aux_out) aux_out[i] = ao;
    ++i;
  }
  rc = flush_rows(c);
  if (!rc) rc = ext_flush_devices(c);
  if (!rc) rc = ext_flush_aux(c);
  return rc;
}

int gs_schedule_ext(gs_ctx* c, const gs_pod* pods, const gs_pod_ext* ext, uint32_t npods, const uint64_t* seq,
                    gs_placement* out, gs_ext_placement* ext_out) {
  return gs_schedule_ext_aux(c, pods, ext, nullptr, npods, seq, out, ext_out, nullptr);
}

int gs_ext_configure_aux(gs_ctx* c, const int64_t weights[GS_NUM_AUX_TYPES]) {
  if (!c || !weights) return GS_EINVAL;
  quiesce(c);
  for (int T = 0; T < GS_NUM_AUX_TYPES; ++T)
    if (weights[T] < 0 || weights[T] > 100) return fail(c, GS_EINVAL, "DeviceShare weight out of range");
  for (int T = 0; T < GS_NUM_AUX_TYPES; ++T) c->aux_weights[T] = weights[T];
  return GS_OK;
}

int gs_node_aux_devices_upsert(gs_ctx* c, const uint32_t* idx, const gs_node_aux_devices* d, uint32_t n) {
  if (!c || (n && !d)) return GS_EINVAL;
  quiesce(c);
  for (uint32_t k = 0; k < n; ++k) {   // (validated like gs_node_devices_upsert's GPUs)
    const uint32_t i = idx ? idx[k] : k;
    if (i >= c->N) return fail(c, GS_EINVAL, "node index %u out of range", i);
    for (int T = 0; T < GS_NUM_AUX_TYPES; ++T) {
      if (d[k].num[T] < 0 || d[k].num[T] > GS_MAX_AUX_DEVICES) return fail(c, GS_EINVAL, "RDMA / FPGA device count out of range");
      for (int g = 0; g < d[k].num[T]; ++g) {
        const gs_aux_device& x = d[k].dev[T][g];
        for (int h = 0; h < g; ++h)
          if (d[k].dev[T][h].minor == x.minor) return fail(c, GS_EINVAL, "duplicate RDMA / FPGA minor on node %u", i);
        if (x.minor < 0 || x.minor > 31) return fail(c, GS_EUNSUPPORTED, "RDMA / FPGA minor outside 0..31");
        if (x.numa_node < -1) return fail(c, GS_EINVAL, "RDMA / FPGA numa_node below -1");
        if (x.total < 0 || x.used < 0 || x.total >= (1LL << 53) || x.used >= (1LL << 53))
          return fail(c, GS_EUNSUPPORTED, "RDMA / FPGA quantity outside [0, 2^53)");
      }
    }
    if (c->aux.empty()) c->aux.assign(c->N, gs_node_aux_devices{});
    c->aux[i] = d[k];
    aux_mark(c, i);
  }
  return GS_OK;
}

int gs_node_aux_devices_get(gs_ctx* c, uint32_t node, gs_node_aux_devices* out) {
  if (!c || !out || node >= c->N) return GS_EINVAL;
  quiesce(c);
  *out = c->aux.empty() ? gs_node_aux_devices{} : c->aux[node];
  return GS_OK;
}

int gs_ext_aux_reserved_get(gs_ctx* c, uint64_t uid, uint32_t* node, gs_aux_placement* out) {
  if (!c || !node || !out) return GS_EINVAL;
  quiesce(c);
  auto it = c->ext_reserved.find(uid);
  if (it == c->ext_reserved.end()) return 0;
  *node = it->second.node;
  *out = it->second.aux;
  return 1;
}

// The per-node view of one extension pod: ext_schedule_one's device chain, then the rows it left in HBM. Nothing is
// reserved or assumed.
int gs_debug_ext_rows_aux(gs_ctx* c, const gs_pod* pod, const gs_pod_ext* ext, const gs_pod_aux* aux, uint64_t seq,
                          int32_t* rows, uint64_t* nominated_uid, int64_t* result) {
  if (!c || !pod || !ext || !rows || !nominated_uid || !result) return GS_EINVAL;
  quiesce(c);
  int rc = ready(c);
  if (rc) return rc;
  if ((rc = validate_pod(c, *pod))) return rc;
  const uint32_t N = c->N;
  for (uint32_t i = 0; i < N; ++i) {
    rows[i] = 0;
    rows[N + i] = -1;
    rows[2 * N + i] = rows[3 * N + i] = 0;
    rows[4 * N + i] = -1;
    nominated_uid[i] = 0;
  }
  for (int k = 0; k < GS_EXT_ROWS_RESULT_WORDS; ++k) result[k] = 0;
  result[GS_EXT_ROWS_NODE] = result[GS_EXT_ROWS_PREF_NODE] = -1;
  ExtChain ch;
  if ((rc = ext_chain(c, *pod, *ext, aux, seq, &ch))) return rc;
  if (ch.early) {
    result[GS_EXT_ROWS_FAIL_CODE] = ch.fail_code;
    return GS_OK;
  }
  const ExtOut xo = *c->h_xout.get();
  if (xo.err & 1u)
    return fail(c, GS_EUNSUPPORTED, "a GPU's NUMA node is not one of its node's NUMA zones (DeviceShare hints)");
  if (xo.err & 2u)
    return fail(c, GS_EUNSUPPORTED, "the topology-manager merge of a GPU pod exceeds its permutation bound");
  const uint32_t len = c->n1 - c->n0;
  std::vector<int32_t> tot(len), T(len);
  std::vector<int16_t> ds(len), rs(len);
  HIP_TRY(c, hipMemcpy(tot.data(), c->d_xtot.get(), 4 * (size_t)len, hipMemcpyDeviceToHost));
  HIP_TRY(c, hipMemcpy(T.data(), c->d_xT.get(), 4 * (size_t)len, hipMemcpyDeviceToHost));
  HIP_TRY(c, hipMemcpy(ds.data(), c->d_xds.get(), 2 * (size_t)len, hipMemcpyDeviceToHost));
  HIP_TRY(c, hipMemcpy(rs.data(), c->d_xrs.get(), 2 * (size_t)len, hipMemcpyDeviceToHost));
  for (uint32_t j = 0; j < len; ++j) {
    const uint32_t i = c->n0 + j;
    rows[i] = tot[j] >= 0 ? 1 : 0;
    rows[N + i] = tot[j] >= 0 ? tot[j] : -1;
    rows[2 * N + i] = ds[j];
    rows[3 * N + i] = rs[j];
    rows[4 * N + i] = T[j];
  }
  const int32_t* h_xnom = c->h_xnom.get();
  for (int k = 0; k < ch.nrec; ++k)
    if (ch.rs_on && h_xnom[k] >= 0) nominated_uid[c->xrec[k].node] = c->xres_uid[c->xrec[k].first + h_xnom[k]];
  result[GS_EXT_ROWS_NODE] = xo.node;
  result[GS_EXT_ROWS_SCORE] = xo.node >= 0 ? xo.score : 0;
  result[GS_EXT_ROWS_TIES] = xo.node >= 0 ? xo.ties : 0;
  result[GS_EXT_ROWS_FEASIBLE] = xo.feasible;
  result[GS_EXT_ROWS_PREF_NODE] = xo.pref_node;
  result[GS_EXT_ROWS_DS_NORM] = xo.node >= 0 ? xo.ds_norm : 0;
  result[GS_EXT_ROWS_RS_NORM] = xo.node >= 0 ? xo.rs_norm : 0;
  return GS_OK;
}

int gs_debug_ext_rows(gs_ctx* c, const gs_pod* pod, const gs_pod_ext* ext, uint64_t seq, int32_t* rows,
                      uint64_t* nominated_uid, int64_t* result) {
  return gs_debug_ext_rows_aux(c, pod, ext, nullptr, seq, rows, nominated_uid, result);
}

}  // extern "C"
