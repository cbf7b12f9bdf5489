/* ksg.h — C ABI of the MI355X scheduling-cycle engine (drop-in boundary).
 *
 * This is the surface a cgo package behind the simulator's debuggable scheduler
 * binds.  It replaces, for the hot-path plugins
 * (NodeResourcesFit, NodeResourcesBalancedAllocation, TaintToleration,
 * NodeAffinity, PodTopologySpread, InterPodAffinity), the per-(pod, node)
 * plugin calls the framework makes through the simulator's wrapper:
 *
 *   PreFilter        simulator/scheduler/plugin/wrappedplugin.go:504
 *   Filter           wrappedplugin.go:535   (interface pinned: plugin/mock/framework.go:114)
 *   PreScore         wrappedplugin.go:472   (mock :233)
 *   Score            wrappedplugin.go:433   (mock :285)
 *   NormalizeScore   wrappedplugin.go:400   (mock :338, ScoreExtensions :300)
 *   Reserve          wrappedplugin.go:631   (mock :597)  -> assume delta on the device
 *   selectHost       upstream schedule_one.go (seeded deterministic tie-break)
 * and renders the result store's annotations (resultstore/store.go:133-198) for
 * the evaluated pod, so filter-result / score-result / finalscore-result /
 * selected-node are byte-identical to what the wrapper records.
 *
 * Objects cross the boundary as Kubernetes JSON (what json.Marshal of a *v1.Pod /
 * *v1.Node produces); the library interns them into the device SoA snapshot.
 * Conventions: every function returns 0 on success and a negative KSG_E* code on
 * failure (message in ksg_last_error: the calling thread's last failure on that
 * context); no exceptions or aborts cross the ABI; output buffers are
 * caller-owned; one context per scheduler profile and GPU.
 * Threads: every call that takes a context holds that context's lock for its
 * duration, so calls from several threads (goroutines) are safe and serialised;
 * the per-node lookups of the framework's parallel workers should read a
 * ksg_cycle_view (no call at all) instead of ksg_filter_status & co. per node.
 * ksg_destroy must not race with other calls on the same context.
 */
#ifndef KSG_H_
#define KSG_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ABI history.  1: round-1..2 surface.  2: ksg_load_cluster orders the queue by
 * PrioritySort and holds back pods with schedulingGates (queue index q is no
 * longer document order: ksg_queue_pod names it); ksg_queue_pod, ksg_gated_pods,
 * ksg_cycle_view_acquire / _release added; a context whose persistent launch
 * stalled refuses calls (KSG_E_STATE) until ksg_load_cluster.  Bindings check
 * ksg_abi_version() >= the version they were written against.  3: ksg_cycle_view
 * holds the Filter outcome once per node (fail_pos / fail_code / fail_msg) and
 * 32-bit scores per position, built on the device.  4: its score rows are as
 * narrow as their values allow (score_bytes / normalized_bytes; ksg_view_score).
 * Added within 4 (no existing entry point or struct changed): ksg_ranked_nodes,
 * ksg_ranked_node, KSG_RANK_MAX; ksg_filter_histogram, ksg_fit_error,
 * ksg_filter_bucket, KSG_DIAG_MAX; ksg_headroom (the call and the struct),
 * ksg_headroom_nodes, ksg_resource_name, KSG_HEADROOM_BOUNDS; ksg_bound_count,
 * ksg_bound_pod, ksg_bound_fit (the call and the struct), ksg_bound_fit_nodes,
 * ksg_node_evictability, ksg_node_evict; ksg_drain (the call and the struct),
 * ksg_drain_plan, ksg_drain_move, KSG_DRAIN_MAX; ksg_scale_up (the call and the
 * struct), ksg_scale_up_plan, KSG_SCALE_MAX; ksg_drain_sets, ksg_drain_prefixes,
 * ksg_drain_set_plan, ksg_drain_set (the struct), KSG_DRAIN_SET_NODES. */
#define KSG_ABI_VERSION 4

#define KSG_OK 0
#define KSG_E_INVALID (-1)   /* bad argument / JSON */
#define KSG_E_DEVICE (-2)    /* HIP error */
#define KSG_E_STATE (-3)     /* call out of order */
#define KSG_E_RANGE (-4)     /* index out of range */
#define KSG_E_NOBUF (-5)     /* output buffer too small (*len holds the size) */

/* plugin ids (profile positions are reported in this order of the profile) */
#define KSG_PLUGIN_NODE_RESOURCES_FIT 0
#define KSG_PLUGIN_NODE_RESOURCES_BALANCED_ALLOCATION 1
#define KSG_PLUGIN_TAINT_TOLERATION 2
#define KSG_PLUGIN_NODE_AFFINITY 3
#define KSG_PLUGIN_POD_TOPOLOGY_SPREAD 4
#define KSG_PLUGIN_INTER_POD_AFFINITY 5

/* ksg_pod_result.status */
#define KSG_SCHEDULED 0
#define KSG_UNSCHEDULABLE 1
#define KSG_ERROR 2

/* filter code per (pod, node): see ksg_filter_codes */
#define KSG_FILTER_PASSED 0xFFFFFFFFu
#define KSG_FILTER_NOT_EVALUATED 0xFFFFFFFEu

typedef struct ksg_ctx ksg_ctx;

typedef struct ksg_opts {
  int32_t device;        /* HIP device ordinal */
  void* stream;          /* hipStream_t to run on; NULL = library-owned stream */
  uint32_t shard_rank;   /* node sharding across GPUs: this context owns nodes   */
  uint32_t shard_count;  /* [rank*N/count, (rank+1)*N/count) of the cluster      */
  uint32_t flags;        /* reserved, 0 */
} ksg_opts;

typedef struct ksg_pod_result {
  int32_t selected;      /* global node index, -1 when none */
  int32_t feasible;      /* nodes that passed every filter plugin */
  int32_t status;        /* KSG_SCHEDULED / KSG_UNSCHEDULABLE / KSG_ERROR */
  uint32_t skip_filter;  /* bit i: plugin id i returned Skip from PreFilter */
  uint32_t skip_score;   /* bit i: plugin id i returned Skip from PreScore */
  int32_t total;         /* weighted score of the selected node */
} ksg_pod_result;

/* Profile JSON: {"plugins": [names in MultiPoint order], "weights": {name: w},
 * "storeWeights": {name: w}, "pluginConfig": {name: args}, "seed": n}
 * (the shape of KubeSchedulerConfiguration.profiles[0] restricted to the hot path;
 * storeWeights is the result store's map, plugins.go:289-304). */
int ksg_create(const char* profile_json, size_t len, const ksg_opts* opts, ksg_ctx** out);
void ksg_destroy(ksg_ctx* ctx);
const char* ksg_last_error(const ksg_ctx* ctx);
int ksg_abi_version(void);

/* Snapshot: {"nodes": [v1.Node], "pods": [bound v1.Pod], "queue": [v1.Pod],
 * "pvs": [v1.PersistentVolume], "pvcs": [v1.PersistentVolumeClaim],
 * "storageClasses": [storagev1.StorageClass]} (ResourcesForSnap field names; the
 * storage objects feed the volume plugins).
 * Replaces the device snapshot (UpdateSnapshot) and the queue.
 * With DefaultPreemption in the profile and >= 2,048 bound pods, the call starts a
 * thread of the context that compiles the bound pods' programs and uploads the
 * victim store DefaultPreemption's search reads (slices under the context's lock;
 * KSG_VICTIM_WARM=0: off); it is joined by the next ksg_load_cluster and by
 * ksg_destroy.  No entry point waits for it. */
int ksg_load_cluster(ksg_ctx* ctx, const char* json, size_t len);
int ksg_num_nodes(const ksg_ctx* ctx);     /* global node count */
int ksg_queue_len(const ksg_ctx* ctx);
/* The queue a document loads is the scheduling queue's pop order (upstream
 * v1.30.4 internal/queue/scheduling_queue.go): with SchedulingGates in the
 * profile (its PreEnqueue; default MultiPoint, scheduler_test.go:536) pods
 * carrying spec.schedulingGates never enter it — no cycle, no annotations —
 * and the rest are ordered as PrioritySort's Less (queuesort/priority_sort.go):
 * higher spec.priority first, then document order.  Queue index q is that
 * position; ksg_queue_pod names it ("namespace/name"), ksg_gated_pods lists the
 * held-back pods ("namespace/name\n" lines).  ksg_cycle pods are appended in
 * the order the framework runs them. */
int ksg_queue_pod(const ksg_ctx* ctx, uint32_t q, char* buf, size_t cap, size_t* len);
int ksg_gated_pods(const ksg_ctx* ctx, char* buf, size_t cap, size_t* len);

/* Queue mode: schedule queue pods [first, first+count) back to back on the
 * device; every selection is assumed on the device before the next pod
 * (no host round trip per pod).  Runs of consecutive PodTopologySpread /
 * InterPodAffinity table-chain pods execute as one persistent launch each
 * (env KSG_RUN=0: one launch pair per pod).  A persistent launch starts with a
 * handshake: when its blocks are not all resident within a few ms (e.g. another
 * context's persistent launch holds part of the CUs) every block leaves before
 * touching any state and the segment's pods run on the two-launch chain; the
 * call blocks until each segment's handshake has decided.  A launch that stalls
 * after its handshake (a poll bound of seconds) fails the call (KSG_E_DEVICE
 * from this call or ksg_wait) instead of hanging, and the context then refuses
 * every call (KSG_E_STATE) until ksg_load_cluster.  Asynchronous: ksg_wait()
 * completes it.
 * Every queue pod gets exactly one scheduling cycle, in queue order: a pod that
 * is unschedulable stays so (upstream parks it in unschedulablePods and retries
 * it after cluster events such as AssignedPodAdd; here the caller re-submits it,
 * e.g. through ksg_cycle, as the framework does in plugin mode).  The oracle
 * follows the same rule, so long queues on a tight cluster can diverge from a
 * live scheduler's retry order, not from the per-cycle results. */
int ksg_schedule_queue(ksg_ctx* ctx, uint32_t first, uint32_t count);
int ksg_wait(ksg_ctx* ctx, float* device_ms);
/* What-if step (BASELINE cfg5): queue pods [first, first+count) are each
 * scheduled against the SAME snapshot (no assume between them: the question
 * "where would each of these pods go now?"), then all their placements are
 * bound together, in queue order.  Any profile: NodeResourcesFit /
 * BalancedAllocation / TaintToleration / NodeAffinity profiles run as two
 * pod-tile x node-tile passes, the first leaving a 4- or 8-byte record per
 * (pod, node) for the second (count x nodes x 4 B: 16 GB at 4,096 pods x 1M
 * nodes; env KSG_WHATIF_REC_MB caps it, default 40960, larger steps run in pod
 * chunks, 0 recomputes every pair in the second pass instead; the record
 * buffer stays allocated across steps until the next ksg_load_cluster or
 * ksg_compact); a what-if step runs no PostFilter (no nomination is reported for its pods); others (PodTopologySpread / InterPodAffinity on
 * frozen class tables, the default profile) run every pod's cycle without
 * assume.  Sharded contexts reduce the per-pod feasible counts, normaliser
 * max/min and argmax keys across ranks.
 * Asynchronous like ksg_schedule_queue; results via ksg_pod_results. */
int ksg_whatif(ksg_ctx* ctx, uint32_t first, uint32_t count);
int ksg_pod_results(ksg_ctx* ctx, uint32_t first, uint32_t count, ksg_pod_result* out);

/* Restore node rows and the existing-pod table to the loaded snapshot
 * (benchmark steps replay the same queue). */
int ksg_reset(ksg_ctx* ctx);
/* Time the dominant Filter/Score kernel with HIP events on the context stream
 * for every `every`-th pod of the following ksg_schedule_queue (0 = off). */
int ksg_sample_kernel(ksg_ctx* ctx, uint32_t every);
int ksg_kernel_time(ksg_ctx* ctx, float* avg_ms, uint32_t* samples);
/* Execution path: profiles made only of NodeResourcesFit / BalancedAllocation
 * run as exact speculative 32-pod windows (k_window: evaluation of window j+1
 * beside the exact replay of window j); every other profile runs the per-pod
 * kernel chain.  per_pod != 0 forces the chain. */
int ksg_set_path(ksg_ctx* ctx, int per_pod);
int ksg_batch_path(const ksg_ctx* ctx);  /* 1 when the batch path is active */

/* Node sharding across GPUs (ksg_opts.shard_rank / shard_count; existing pods
 * live with their node).  Fit/BalancedAllocation profiles: per window of 32
 * pods every rank all-gathers its per-pod top-64 candidates (with their node
 * rows) and local feasible counts, merges them, and runs the same deterministic
 * replay, applying only its own nodes' assume deltas.  Other profiles: the
 * table chain on every rank's nodes against global class tables (each rank sums
 * its pair-level counts with the others' when a class is built and applies every
 * assume's pair-level delta), two exchanges per cycle (counts and normalisers;
 * argmax key), three with several PodTopologySpread score constraints; pods
 * whose spread constraints the tables cannot answer run the scanning chain
 * (four exchanges).  Needs ksg_set_exchange before the first run.  What-if
 * steps: per-pod summaries merged after each pass.
 *   mode 1: RCCL all-gather on the context stream; nccl_id = 128 bytes from
 *           ksg_nccl_unique_id() on one rank, broadcast by the caller.
 *   mode 2: host callback fn(user, send, recv, bytes_per_rank) that all-gathers
 *           host buffers (recv = ranks x bytes, rank order); returns 0.        */
typedef int (*ksg_exchange_fn)(void* user, const void* send, void* recv, size_t bytes_per_rank);
int ksg_nccl_unique_id(uint8_t* out128);
int ksg_set_exchange(ksg_ctx* ctx, int mode, const uint8_t* nccl_id, ksg_exchange_fn fn, void* user);

/* Keep per-(pod, node) outputs for queue pods [first, first+count) (tests,
 * annotation rendering).  Must precede ksg_schedule_queue. */
int ksg_keep_outputs(ksg_ctx* ctx, uint32_t first, uint32_t count);
/* Filter code per local node: KSG_FILTER_PASSED, KSG_FILTER_NOT_EVALUATED or
 * (profile position << 24) | detail (volume plugins: KSG_VOL_* reason bits of
 * ksg_types.h in the low 16 bits). */
int ksg_filter_codes(ksg_ctx* ctx, uint32_t q, uint32_t* out, uint32_t n);
/* Raw Score of profile position pos per local node (valid where the filter passed). */
int ksg_scores(ksg_ctx* ctx, uint32_t q, uint32_t pos, int32_t* out, uint32_t n);
/* Store.GetStoredResult for queue pod q as a JSON object {annotation key: value}. */
int ksg_annotations(ksg_ctx* ctx, uint32_t q, char* buf, size_t cap, size_t* len);

/* Drop-in cycle (one pod, the framework's scheduleOne): PreFilter..Score..
 * NormalizeScore for a new pod (v1.Pod JSON, appended to the queue: its index
 * is ksg_queue_len() - 1), its per-node outputs kept for ksg_filter_codes /
 * ksg_scores / ksg_annotations.  commit != 0 also assumes it on the engine's
 * selectHost choice (harness mode); commit == 0 leaves the assume to
 * ksg_reserve with the framework's own choice (plugin mode).  New label keys,
 * label values and namespaces are interned in place; a pod bringing a topology
 * key, a scalar resource or a host port the snapshot has not seen triggers a
 * re-encode of the snapshot (placements kept). */
int ksg_cycle(ksg_ctx* ctx, const char* pod_json, size_t len, int commit, ksg_pod_result* out);
/* ReservePlugin.Reserve (wrappedplugin.go:631 -> scheduler cache assume):
 * assume queue pod q (run with commit == 0) on global node `node`.  The device
 * delta is queued without a wait: a device failure of it is reported late, by the
 * next call that synchronises (a cycle, a view, Unreserve ...), which then returns
 * KSG_E_DEVICE and leaves the context refusing calls (KSG_E_STATE) until
 * ksg_load_cluster, since the host already counts the pod as placed. */
int ksg_reserve(ksg_ctx* ctx, uint32_t q, int32_t node);
/* ReservePlugin.Unreserve (mock framework.go:611): undo the assume of queue
 * pod q (cycle or queue mode): node rows, and its existing-pod table entry. */
int ksg_unreserve(ksg_ctx* ctx, uint32_t q);
/* Bounded memory in plugin mode: queue pods [0, keep_from) leave the queue —
 * the placed ones become bound pods of the snapshot, the rest are forgotten
 * (their documents released) — and pod keep_from + i becomes queue pod i, its
 * results and placement kept.  One snapshot re-encode; call between cycles with
 * keep_from = the oldest pod whose Reserve / Unreserve / lookups may still come
 * (ksg_queue_len() when none). */
int ksg_compact(ksg_ctx* ctx, uint32_t keep_from);

/* ---- what each wrapped plugin's extension point returns (the Go plugin's calls,
 * INTEGRATION.md), for queue pod q whose per-node outputs are kept (the pod of the
 * last ksg_cycle, or a range given to ksg_keep_outputs).  `pos` is the profile
 * position (ksg_plugin_position); `node` a global node index (ksg_node_index).
 * Status codes are framework.Code values (v1.30 framework/interface.go):
 * 0 Success, 1 Error, 2 Unschedulable, 3 UnschedulableAndUnresolvable, 5 Skip;
 * -1 means the framework does not call this plugin there (an earlier filter
 * failed on the node, PreFilter Skip, outside the PreFilterResult, no scoring).
 * Messages are Status.Message() (what the wrapper records, wrappedplugin.go:542). */
int ksg_plugin_position(const ksg_ctx* ctx, const char* name, size_t len);  /* or KSG_E_RANGE; "…Wrapped" accepted */
/* The weights the profile resolved for position `pos`: *weight is the framework's
 * (upstream framework.go getScoreWeights: an explicit Score weight wins over
 * MultiPoint's; it scales the total selectHost uses), *store_weight the result
 * store's (plugins.go:289-304 getScorePluginWeight: MultiPoint overwrites; it
 * scales finalscore-result, store.go:504-507).  They differ only in the quirk of
 * scheduler_test.go:344-407.  ksg_create takes the flat profile
 * {plugins, weights, storeWeights, pluginConfig} or a KubeSchedulerConfiguration /
 * KubeSchedulerProfile (plugins.multiPoint / plugins.score, pluginConfig list). */
int ksg_plugin_weights(const ksg_ctx* ctx, uint32_t pos, int64_t* weight, int64_t* store_weight);
int ksg_node_index(const ksg_ctx* ctx, const char* name, size_t len);       /* or KSG_E_RANGE */
/* PreFilter (wrappedplugin.go:504, mock framework.go:61): status; and the
 * PreFilterResult node set as a JSON array of node names, "null" for all nodes. */
int ksg_prefilter_status(ksg_ctx* ctx, uint32_t q, uint32_t pos, int32_t* code, char* msg, size_t cap, size_t* len);
int ksg_prefilter_result(ksg_ctx* ctx, uint32_t q, char* buf, size_t cap, size_t* len);
/* The PreFilterResult of the plugin at profile position pos (NodeAffinity's, or
 * VolumeBinding's GetEligibleNodes for claims bound to local PVs): JSON array of
 * node names, "null" when the plugin returns none.  The framework intersects them;
 * an empty intersection rejects the pod after the later plugin's PreFilter, whose
 * own status stays Success (ksg_prefilter_status). */
int ksg_prefilter_result_pos(ksg_ctx* ctx, uint32_t q, uint32_t pos, char* buf, size_t cap, size_t* len);
/* Filter (wrappedplugin.go:535, mock framework.go:114) on one node. */
int ksg_filter_status(ksg_ctx* ctx, uint32_t q, uint32_t pos, uint32_t node, int32_t* code, char* msg, size_t cap,
                      size_t* len);
/* PreScore (wrappedplugin.go:472, mock framework.go:233): status and message. */
int ksg_prescore_status(ksg_ctx* ctx, uint32_t q, uint32_t pos, int32_t* code, char* msg, size_t cap, size_t* len);
/* NormalizeScore (wrappedplugin.go:400, mock framework.go:338): the plugin's
 * normalized score per local node (raw score for plugins without
 * ScoreExtensions), computed on the device by the NormalizeScore the selection
 * used; valid where the node passed every filter. */
int ksg_normalized_scores(ksg_ctx* ctx, uint32_t q, uint32_t pos, int64_t* out, uint32_t n);
/* Ranked candidates: the min(k, feasible) best feasible nodes of queue pod q's
 * cycle, best first, selected on the device from the pod's kept outputs (the
 * pod of a ksg_cycle with either commit value, or a ksg_keep_outputs range; the
 * lifetime of ksg_normalized_scores).  The order is the engine's own selection
 * order: descending selection key (weighted total, then the seeded tie-break
 * hash, then the node index) with the seed and queue index the pod's selection
 * used, so out[0] is (result.selected, result.total) of a scheduled pod and the
 * order is total, ties included (upstream selectHost reports its highest-scored
 * nodes beside the winner).  `total` is the sum over the scoring positions of
 * normalized score x framework weight (ksg_plugin_weights' *weight).  *n_out
 * receives the count: 0 for an unschedulable pod or a cycle that ended in
 * KSG_ERROR; 1, the selected node with the result's total, for a pod with one
 * feasible node (upstream runs no scoring then).  k outside [1, KSG_RANK_MAX],
 * out or n_out NULL, q outside the queue: KSG_E_RANGE; outputs not kept for q:
 * KSG_E_STATE (as ksg_normalized_scores); a sharded context: KSG_E_INVALID.
 * Changes no scheduling state; two calls on one pod return the same bytes.
 * Env KSG_RANK_TILE (read at ksg_create): nodes per block of the select, a power
 * of two in [128, 2048] (tests reach the multi-level merge with few nodes). */
#define KSG_RANK_MAX 64
typedef struct ksg_ranked_node {
  int32_t node;   /* global node index */
  int32_t total;  /* its weighted score */
} ksg_ranked_node;
int ksg_ranked_nodes(ksg_ctx* ctx, uint32_t q, uint32_t k, ksg_ranked_node* out, uint32_t* n_out);
/* Unschedulable diagnosis: why queue pod q's cycle found the nodes it found,
 * counted on the device from the pod's kept outputs (valid for the pods
 * ksg_ranked_nodes accepts).
 * ksg_filter_histogram: the distinct (code, status) pairs over every local node,
 * passed and not-evaluated nodes included, so the counts sum to the node count;
 * ascending by (code, status), so two calls return the same bytes.  *n_out
 * receives the number of buckets; cap too small: KSG_E_NOBUF with the needed
 * count in *n_out.  A cycle can hold more than KSG_DIAG_MAX distinct pairs (every
 * node its own taint): the call then counts the kept filter row on the host,
 * with the same answer.  out or n_out NULL, q outside the queue: KSG_E_RANGE;
 * outputs not kept for q: KSG_E_STATE (as ksg_normalized_scores); a sharded
 * context: KSG_E_INVALID.  Changes no scheduling state.
 * Env KSG_DIAG_SLOTS (read at ksg_create): slots of the device table, a power of
 * two in [4, KSG_DIAG_MAX] (tests reach the host count with a handful of reasons).
 * ksg_fit_error: the text of upstream v1.30.4 framework.FitError.Error() for an
 * unschedulable pod (the PodScheduled condition's message),
 *   "0/5000 nodes are available: 12 node(s) had untolerated taint {dedicated: gpu}, 4988 Insufficient cpu."
 * up to but not including the PostFilter clause ("preemption: 0/N nodes are
 * available: ..."), which needs per-node preemption statuses the dry run does not
 * keep.  "0/<nodes of the snapshot> nodes are available:", then either the
 * rejecting PreFilter's message (for an empty PreFilterResult intersection the
 * framework's "node(s) didn't satisfy plugin(s) [A B] simultaneously" / "node(s)
 * didn't satisfy plugin A") or, per distinct Filter reason (a NodeResourcesFit or
 * VolumeBinding status splits into its reasons, each counted once per node),
 * "<count> <reason>", the entries sorted as byte strings (sort.Strings: "10 x"
 * before "2 x") and joined with ", "; a full stop closes a non-empty list.  Nodes
 * outside the PreFilterResult are not counted.  A scheduled pod, or a cycle that
 * ended in KSG_ERROR, gives *len = 0.  Buffer convention and codes of
 * ksg_annotations (cap 0: the size in *len, KSG_E_NOBUF); otherwise the codes of
 * ksg_filter_histogram. */
#define KSG_DIAG_MAX 1024
typedef struct ksg_filter_bucket {
  uint32_t code;    /* device filter code, as ksg_filter_codes: KSG_FILTER_PASSED,
                       KSG_FILTER_NOT_EVALUATED or (position << 24) | detail */
  int32_t pos;      /* failing profile position; n_positions: passed; -1: not evaluated */
  int32_t status;   /* framework.Code of that Filter failure (2 or 3), 0 passed, -1 not evaluated:
                       what ksg_filter_status / the cycle view's fail_code give for these nodes */
  uint32_t count;   /* local nodes with this (code, status) */
} ksg_filter_bucket;
int ksg_filter_histogram(ksg_ctx* ctx, uint32_t q, ksg_filter_bucket* out, uint32_t cap, uint32_t* n_out);
int ksg_fit_error(ksg_ctx* ctx, uint32_t q, char* buf, size_t cap, size_t* len);
/* Headroom: how many more copies of queue pod q fit, on which nodes, and which
 * constraint runs out first -- the cluster-capacity question, counted on the device
 * in one pass over the node columns per pod.
 * The per-node count of pod q on local node n, against the device snapshot as it
 * stands when the call runs (every assume, Reserve and event applied so far; the
 * call is ordered on the context stream after any pending delta):
 *   0 when the pod's PreFilter rejected it or ended in an error, when n is outside
 *   its PreFilterResult, or when one of the profile's TaintToleration, NodeAffinity,
 *   NodeUnschedulable or NodeName Filters fails on n (the node is not "open");
 *   otherwise min(room, min over the resource columns r with request[r] > 0 of
 *   fit_r), where room = max(0, allowed pods - pod count), free_r = allocatable_r -
 *   requested_r and fit_r = free_r < 0 ? 0 : floor(free_r / request[r]).  A pod whose
 *   requests are all zero is bounded by the room alone, as fitsRequest returns early.
 * This is the number of further copies of q upstream's fitsRequest admits one after
 * another on n: k copies add k x request to requested and k to the pod count.  It is
 * at most room, so it fits int32.  Integer arithmetic throughout; exact.
 * ksg_headroom fills out[i] for queue pods [first, first + count) in one launch:
 *   replicas    the sum of the per-node counts over the local nodes
 *   nodes       nodes whose count is >= 1
 *   open_nodes  nodes that pass every Filter plugin other than NodeResourcesFit
 *   max_node    the largest per-node count (0 when replicas == 0)
 *   best_node   the lowest global node index holding max_node (-1 when replicas == 0)
 *   bound[]     over the open nodes, count 0 included (what the cluster is short of):
 *               which constraint is the minimum -- index 0 the pod room, index 1 + r
 *               resource column r (the bit order of the Fit filter's detail;
 *               ksg_resource_name names r); a tie counts for the lowest index;
 *               sum(bound) == open_nodes.
 * ksg_headroom_nodes writes the per-node counts of one pod: n must be the local node
 * count (the convention of ksg_filter_codes).
 * ksg_resource_name: the name of resource column r ("cpu", "memory",
 * "ephemeral-storage", then the scalar resources in vocabulary order): the rows of
 * ksg_node_requested and bound[1 + r].  Buffer convention of ksg_annotations;
 * KSG_E_RANGE past the last column.
 * Profiles: NodeResourcesFit must be there, and every plugin with a Filter must be
 * one of NodeResourcesFit, TaintToleration, NodeAffinity, NodeUnschedulable,
 * NodeName (plugins that only score or only run PostFilter do not matter).  With
 * PodTopologySpread, InterPodAffinity, NodePorts or a volume plugin replicas of a
 * pod interact through that plugin's Filter and no closed form exists:
 * KSG_E_INVALID, the message naming the plugin.  A sharded context: KSG_E_INVALID.
 * out NULL, the range outside the queue, n different from the local node count:
 * KSG_E_RANGE.  count == 0: KSG_OK, nothing written.  The calls need no kept
 * outputs and no earlier cycle of the pod, change no scheduling state, and two
 * calls return the same bytes.
 * (C: the struct is named by its tag, `struct ksg_headroom`, beside the call of the
 * same name -- as stat(2).) */
#define KSG_HEADROOM_BOUNDS 9            /* 1 + KSG_MAX_RES */
struct ksg_headroom {
  int64_t  replicas;    /* sum over local nodes of the per-node count */
  int32_t  nodes;       /* nodes whose count is >= 1 */
  int32_t  open_nodes;  /* nodes that pass every Filter plugin other than NodeResourcesFit */
  int32_t  max_node;    /* the largest per-node count (0 when replicas == 0) */
  int32_t  best_node;   /* lowest global node index holding max_node; -1 when replicas == 0 */
  uint32_t bound[KSG_HEADROOM_BOUNDS]; /* over the open nodes: which constraint is the minimum */
};
int ksg_headroom(ksg_ctx* ctx, uint32_t first, uint32_t count, struct ksg_headroom* out);
int ksg_headroom_nodes(ksg_ctx* ctx, uint32_t q, int32_t* out, uint32_t n);
int ksg_resource_name(const ksg_ctx* ctx, uint32_t r, char* buf, size_t cap, size_t* len);

/* Eviction fit (the descheduler's nodeFit and its taint / affinity / overcommit
 * violation checks): which pods that are already running would their node no
 * longer admit, and which of them has another node to go to -- every (bound pod,
 * node) pair judged on the device (csrc/bound_fit.hip).
 * Subjects.  b is the host's bound index: the document's pods with spec.nodeName,
 * then the pods of addPod events, then the placed queue pods ksg_compact turned into
 * bound pods.  ksg_bound_count counts them, ksg_bound_pod names one
 * ("namespace/name", buffer convention of ksg_annotations; *node = its global node
 * index, -1 when its node is not in the cluster).  An index is valid until the next
 * ksg_load_cluster, ksg_apply_events or ksg_compact.  Queue pods placed since the
 * last encode count as load on their nodes (the device rows hold them) but are
 * not subjects: a caller who wants them calls ksg_compact(ksg_queue_len()) first.
 * code(b, n), for bound pod b on node o, against the device snapshot as it stands
 * when the call runs (every assume, Reserve and event applied so far; the call is
 * ordered on the context stream after any pending delta): the Filter code
 * ksg_filter_codes would report for node n after b was removed from the snapshot
 * and run through ksg_cycle(commit = 0) with spec.nodeName cleared -- a bound pod's
 * spec.nodeName is its placement, not a constraint, and its replacement comes from a
 * controller without one, so NodeName's Filter is not applied.  In closed form:
 *   n != o  the first failing Filter in profile order against n's current rows;
 *   n == o  the same, NodeResourcesFit reading requested_r - request_r(b) for every
 *           resource column and pod count - 1;
 *   KSG_FILTER_NOT_EVALUATED when b's PreFilter rejects it or ends in an error, or n
 *           is outside its PreFilterResult, as a cycle reports;
 *   a pod whose requests are all zero is checked against the pod room alone, as
 *           fitsRequest returns early;  KSG_FILTER_PASSED when every Filter passes.
 * Codes are (position << 24) | detail, the detail of NodeResourcesFit its reason
 * bits, as ksg_filter_codes.  Integer arithmetic throughout; exact.
 * ksg_bound_fit fills out[i] for bound pods [first, first + count);
 * ksg_bound_fit_nodes writes code(b, n) for every local node n: n must be the local
 * node count (the convention of ksg_filter_codes).  ksg_node_evictability judges
 * every bound pod and counts per local node (n: the local node count).  stuck is a
 * necessary condition for a drain, not a sufficient one: each pod is judged alone,
 * against the snapshot with only itself removed, so two pods counted as movable may
 * compete for the same room.
 * Profiles: those of ksg_headroom (NodeResourcesFit there; every plugin with a
 * Filter one of NodeResourcesFit, TaintToleration, NodeAffinity, NodeUnschedulable,
 * NodeName) -- under them removing b changes node o's rows only.  Any other:
 * KSG_E_INVALID, the message naming the plugin.  A sharded context: KSG_E_INVALID.
 * out NULL, the range outside [0, ksg_bound_count), n different from the local node
 * count: KSG_E_RANGE.  count == 0: KSG_OK, nothing written.  The calls change no
 * scheduling state and two calls return the same bytes.  The first call of a
 * snapshot generation (after a load, an event batch, a compact) compiles every
 * bound pod's program and uploads them, the store DefaultPreemption's victim
 * search keeps; later calls find it resident.
 * (C: `struct ksg_bound_fit` is named by its tag beside the call, as ksg_headroom.) */
int ksg_bound_count(const ksg_ctx* ctx);
int ksg_bound_pod(ksg_ctx* ctx, uint32_t b, char* buf, size_t cap, size_t* len, int32_t* node);
struct ksg_bound_fit {          /* 16 bytes */
  int32_t  node;         /* the node the pod is bound to (global index) */
  uint32_t own_code;     /* code(b, own node): KSG_FILTER_PASSED when its node would admit it again */
  int32_t  other_nodes;  /* nodes other than its own with code == KSG_FILTER_PASSED */
  int32_t  first_other;  /* the lowest global index among them; -1 when other_nodes == 0 */
};
int ksg_bound_fit(ksg_ctx* ctx, uint32_t first, uint32_t count, struct ksg_bound_fit* out);
int ksg_bound_fit_nodes(ksg_ctx* ctx, uint32_t b, uint32_t* codes, uint32_t n);
struct ksg_node_evict {         /* 16 bytes, per local node */
  int32_t pods;      /* bound pods on the node */
  int32_t stuck;     /* of them, other_nodes == 0: nowhere else to go */
  int32_t drifted;   /* of them, own_code != KSG_FILTER_PASSED: the node would not admit them today */
  int32_t reserved;  /* 0 */
};
int ksg_node_evictability(ksg_ctx* ctx, struct ksg_node_evict* out, uint32_t n);

/* Drain simulation (the cluster-autoscaler's scale-down simulation, the planning
 * of a `kubectl drain`): can local node x be emptied -- its pods re-placed one
 * after another, each counted on its new node before the next is judged.  Where
 * ksg_node_evictability gives the necessary condition, this is the sufficient
 * one for the order it simulates.  One block per candidate on the device
 * (csrc/drain.hip), every candidate of a call in one launch.
 * Subjects.  The bound pods on x (the bound list of the eviction fit above) in
 * ascending bound index, except the pods a drain leaves in place: pods whose
 * controller owner reference has kind DaemonSet, and mirror pods (annotation
 * kubernetes.io/config.mirror), as `kubectl drain --ignore-daemonsets` and the
 * autoscaler leave them.  They are counted in `daemon` and stay on x.  Queue
 * pods placed since the last encode are load, not subjects, as above.
 * The simulation runs against the device snapshot as it stands when the call
 * runs (every assume, Reserve and event applied so far).  For subject b, in
 * order, dest(b) is the lowest global node index n != x whose code is
 * KSG_FILTER_PASSED, the code being that of ksg_bound_fit_nodes (NodeName's
 * Filter is not applied) with this drain's earlier placements counted:
 * NodeResourcesFit reads requested_r(n) plus the sum of request_r(b') over the
 * earlier subjects b' with dest(b') == n, and pod count(n) plus the number of
 * those subjects.  x itself is never a destination.  A subject with no such node
 * is unplaced, and the simulation goes on with the next subject.  Every
 * candidate's drain is independent of every other candidate's; nothing is moved
 * and no scheduling state changes.
 * First fit in node order is deliberate: it is deterministic, needs no Score, and
 * is what a scale-down simulation does.  It is not the scheduler's choice: a real
 * cycle scores the feasible nodes and selectHost picks among the best, so the
 * pods of a real drain may land elsewhere.  The answer says that a placement
 * exists for this order, not which one the scheduler will make.
 * At most KSG_DRAIN_MAX subjects are simulated per candidate; further subjects are
 * counted in `skipped` (dest -2 in the plan) and the drain is then not complete.
 * A node is drainable when unplaced == 0 && skipped == 0.  (Environment
 * KSG_DRAIN_MAX, read at ksg_create: a power of two in [2, 512] that lowers the
 * cap; tests reach it with a handful of pods.)
 * ksg_drain fills out[i] for local nodes [first_node, first_node + count).
 * ksg_drain_plan returns the subjects of one local node in simulation order with
 * their destinations; buffer convention of ksg_filter_histogram: *n_out receives
 * the number of subjects, cap too small: KSG_E_NOBUF with the needed count.
 * Profiles, refusals and errors are those of ksg_bound_fit: a profile outside
 * headroom's closed form or a sharded context: KSG_E_INVALID; out (or n_out) NULL,
 * the range outside the local nodes: KSG_E_RANGE; count == 0: KSG_OK, nothing
 * written.  Two calls return the same bytes.  Indices in the answer are host bound
 * indices and global node indices. */
#define KSG_DRAIN_MAX 512
struct ksg_drain {            /* 32 bytes, per candidate node */
  int32_t pods;            /* bound pods on the node */
  int32_t daemon;          /* of them, DaemonSet-owned or mirror pods: left in place */
  int32_t placed;          /* subjects that found a destination */
  int32_t unplaced;        /* subjects that found none */
  int32_t skipped;         /* subjects beyond KSG_DRAIN_MAX: not simulated */
  int32_t first_unplaced;  /* bound index of the first unplaced subject, -1 when none */
  int32_t dest_nodes;      /* distinct destination nodes */
  int32_t reserved;        /* 0 */
};                          /* drainable: unplaced == 0 && skipped == 0 */
struct ksg_drain_move { int32_t bound; int32_t dest; };  /* dest: global node, -1 unplaced, -2 skipped */
int ksg_drain(ksg_ctx* ctx, uint32_t first_node, uint32_t count, struct ksg_drain* out);
int ksg_drain_plan(ksg_ctx* ctx, uint32_t node, struct ksg_drain_move* out, uint32_t cap, uint32_t* n_out);

/* Set drain (the cluster-autoscaler's cumulative scale-down simulation, Karpenter's
 * multi-node consolidation): can these nodes be removed together.  ksg_drain
 * judges every candidate alone: two nodes that are each drainable may send their
 * pods to the same room, or one to the other.  Here the nodes of a set leave
 * together, in one simulation.  One block per set on the device
 * (csrc/drain_set.hip), every set of a call in one launch.
 * Sets.  Set i is the local nodes nodes[set_start[i] .. set_start[i + 1]), in the
 * caller's order; set_start has n_sets + 1 entries and does not descend.  The
 * order matters and the call does not sort: the same nodes in another order may
 * give another plan and another answer.  A set holds at most
 * KSG_DRAIN_SET_NODES nodes, each once.
 * Subjects.  The set's nodes in list order, and within a node its drain subjects
 * exactly as ksg_drain defines them: ascending bound index, DaemonSet-owned and
 * mirror pods left out.  Those go with their node and are counted in `daemon`.
 * Destinations.  For subject b, in order, dest(b) is the lowest global node index
 * not in the set whose code is KSG_FILTER_PASSED.  The code is that of
 * ksg_bound_fit_nodes (NodeName's Filter is not applied) with every earlier
 * placement of this set's simulation counted on its destination (requests and pod
 * count), from whichever member it came.  A member is never a destination,
 * neither an earlier one of the list nor a later one.  A subject with no such
 * node is unplaced; it changes nothing and the simulation goes on with the next.
 * At most KSG_DRAIN_MAX subjects are simulated per set (the engine's effective
 * cap: the environment override of ksg_drain holds here too); the rest are counted
 * in `skipped` and get dest -2 in the plan.  A set is removable when
 * unplaced == 0 && skipped == 0.  first_blocked is the position in the set's list
 * of the first node one of whose subjects is unplaced or skipped: the prefix
 * before it went through.
 * First fit in node order, as in ksg_drain: deterministic and what a scale-down
 * simulation does, and not the scheduler's choice.  A real cycle scores the
 * feasible nodes, so the pods of a real removal may land elsewhere: the answer
 * says that a placement exists for this order, not which one will be made.  A set
 * of one node x equals ksg_drain of x, field by field (first_blocked is then 0 or
 * -1), and its plan equals ksg_drain_plan(x).
 * ksg_drain_sets fills out[i] for set i.  ksg_drain_prefixes fills out[k] with the
 * answer for the set nodes[0 .. k] inclusive, for every k < n, in one launch: a
 * longer prefix excludes more destinations, so it is no continuation of a shorter
 * one, and every prefix is simulated from the start.  ksg_drain_set_plan returns
 * one set's subjects in simulation order with their destinations, buffer
 * convention of ksg_drain_plan: *n_out receives the number of subjects, cap too
 * small: KSG_E_NOBUF with the needed count.
 * Profiles, refusals and errors are those of ksg_drain: a NULL context, a profile
 * outside headroom's closed form or a sharded context: KSG_E_INVALID.  A required
 * pointer that is NULL with a non-zero count (nodes, set_start, out, n_out), a
 * descending set_start, a node outside the local nodes, a set (or n) of more than
 * KSG_DRAIN_SET_NODES nodes: KSG_E_RANGE.  A node listed twice in one set (for
 * ksg_drain_prefixes and ksg_drain_set_plan: in the list): KSG_E_INVALID, the
 * message names the node.  n_sets == 0 or n == 0: KSG_OK, nothing written.  An
 * empty set: all counts 0, first_unplaced and first_blocked -1.  Nothing is moved
 * and no scheduling state changes; sets are independent of each other; two calls
 * return the same bytes.  Indices in the answer are host bound indices and global
 * node indices. */
#define KSG_DRAIN_SET_NODES 128          /* nodes per set */
struct ksg_drain_set {        /* 32 bytes, per set */
  int32_t pods;            /* bound pods on the set's nodes */
  int32_t daemon;          /* of them DaemonSet-owned or mirror pods: they go with their node */
  int32_t placed;          /* subjects that found a destination */
  int32_t unplaced;        /* subjects that found none */
  int32_t skipped;         /* subjects beyond the cap: not simulated */
  int32_t first_unplaced;  /* bound index of the first unplaced subject, -1 when none */
  int32_t first_blocked;   /* position in the set's list of the first node with an unplaced or skipped subject, -1 */
  int32_t dest_nodes;      /* distinct destination nodes */
};                          /* removable: unplaced == 0 && skipped == 0 */
int ksg_drain_sets(ksg_ctx* ctx, const uint32_t* nodes, const uint32_t* set_start, uint32_t n_sets,
                   struct ksg_drain_set* out);
int ksg_drain_prefixes(ksg_ctx* ctx, const uint32_t* nodes, uint32_t n, struct ksg_drain_set* out);
int ksg_drain_set_plan(ksg_ctx* ctx, const uint32_t* nodes, uint32_t n, struct ksg_drain_move* out, uint32_t cap,
                       uint32_t* n_out);

/* Scale-up simulation (the cluster-autoscaler's scale-up estimate, its binpacking
 * estimator; Karpenter's provisioning loop): for pods that do not fit, which node
 * group to grow, by how many nodes, and which pods still stay pending.  Per
 * template the listed pods are packed onto fresh nodes of the template's shape,
 * first fit in bin order, the same rule as the drain above.  One block per
 * template on the device (csrc/scale_up.hip), every template of a call in one
 * launch; the static verdicts of all (pod, template) pairs in one launch before.
 * Pods.  pods[] lists queue indices in packing order.  The order is the caller's
 * choice (the autoscaler sorts by decreasing size); the call does not sort.  An
 * index listed twice is packed twice, as two replicas.  A pod's own scheduling
 * state (pending, scheduled, unschedulable) does not matter to the call.
 * Templates.  templates[] lists local node indices.  A fresh node of template t
 * has t's allocatable columns, allowed pod count, labels, taints and
 * spec.unschedulable flag, exactly as the device snapshot holds them when the
 * call runs (every event applied so far; the call is ordered on the context
 * stream after any pending delta).
 * Base load.  A fresh node starts with the requests and the count of t's bound
 * pods that a drain leaves in place: pods owned by a DaemonSet controller and
 * mirror pods (ksg_drain above), as the autoscaler's template keeps them.  They
 * are counted in base_pods.  t's other bound pods do not count, queue pods placed
 * on t do not count, requested(t) does not count.
 * open(p, t).  Pod p is open for template t when all of these hold, and closed
 * for t otherwise: p's PreFilter neither rejected it nor ended in an error; p has
 * no PreFilterResult node set (such a set names existing nodes); with NodeName in
 * the profile p sets no spec.nodeName (a fresh node carries a new name); the
 * profile's TaintToleration, NodeAffinity and NodeUnschedulable Filters pass on
 * node t.  Limitation: the labels are t's verbatim, kubernetes.io/hostname
 * included, so a selector on the template's own host name matches the fresh
 * nodes too; the autoscaler's templates have the same limitation.
 * Packing.  For each pod in list order: a closed pod is counted in `closed` and
 * the simulation goes on.  Otherwise the pod goes to the lowest opened bin whose
 * remaining room admits it, the test being NodeResourcesFit's against
 * allocatable_r(t) - base_r - the sum of the requests packed into the bin, and
 * allowed(t) - base_pods - the pods packed into the bin (a zero-request pod is
 * bounded by the pod room alone).  If no opened bin admits it, an empty fresh
 * node is tested: if that does not admit it, it is counted in `too_big`;
 * otherwise, if nodes == max_nodes, in `over_cap`; otherwise bin `nodes` is
 * opened and the pod placed there.  The simulation always goes on with the next
 * pod.  Arithmetic is integer and exact.  Templates are independent of each
 * other; no scheduling state changes, and two calls return the same bytes.
 * First fit in bin order is what a scale-up estimate does; it is not the
 * scheduler's choice among the opened nodes, and the answer is an estimate of
 * the nodes needed, not a placement the scheduler will make.
 * max_nodes lies in [1, KSG_SCALE_MAX].  (Environment KSG_SCALE_MAX, read at
 * ksg_create: a power of two in [2, 1024] that lowers the upper bound; tests reach
 * it with a handful of pods.)
 * ksg_scale_up fills out[i] for templates[i].  ksg_scale_up_plan returns for one
 * template the bin of every listed pod: bin_out[i] >= 0 the bin, -1 closed, -2 too
 * big, -3 over the cap.
 * Profiles, refusals and errors are those of ksg_drain: a sharded context or a
 * profile outside headroom's closed form: KSG_E_INVALID; out, bin_out, pods or
 * templates NULL with a non-zero count, a queue index outside the queue, a
 * template outside the local nodes, max_nodes outside its range: KSG_E_RANGE;
 * n_templates == 0: KSG_OK, nothing written; n_pods == 0: structs with every count
 * 0, first_unpacked -1 and base_pods set (the plan writes nothing). */
#define KSG_SCALE_MAX 1024
struct ksg_scale_up {          /* 32 bytes, per template */
  int32_t nodes;           /* fresh nodes opened */
  int32_t packed;          /* pods of the list placed on one of them */
  int32_t closed;          /* pods a node of this shape never admits (see above) */
  int32_t too_big;         /* open pods that an empty fresh node does not admit */
  int32_t over_cap;        /* open pods that fit an empty node, met when `nodes` == max_nodes and no opened node had room */
  int32_t first_unpacked;  /* position in the pod list of the first pod not packed, -1 when none */
  int32_t base_pods;       /* pods every fresh node starts with (the template's DaemonSet / mirror pods) */
  int32_t reserved;        /* 0 */
};                          /* satisfied: packed == n_pods */
int ksg_scale_up(ksg_ctx* ctx, const uint32_t* pods, uint32_t n_pods, const uint32_t* templates,
                 uint32_t n_templates, uint32_t max_nodes, struct ksg_scale_up* out);
int ksg_scale_up_plan(ksg_ctx* ctx, const uint32_t* pods, uint32_t n_pods, uint32_t template_node,
                      uint32_t max_nodes, int32_t* bin_out /* n_pods entries */);

/* PostFilter (wrappedplugin.go:550-577 -> store.go:442 AddPostFilterResult):
 * DefaultPreemption's dry run for an unschedulable pod q (PodEligibleToPreemptOthers,
 * nodesWherePreemptionMightHelp, SelectVictimsOnNode, pickOneNodeForPreemption of
 * upstream v1.30.4 default_preemption.go / preemption.go; nothing is evicted).
 * *nominated = the nominated global node index, -1 none; buf receives the
 * victims as "namespace/name\n" lines (most important first).  Unsharded
 * contexts with DefaultPreemption in the profile; queue runs stop after each
 * pod that may preempt (ksg_schedule_queue then returns with them done). */
int ksg_postfilter_result(ksg_ctx* ctx, uint32_t q, int32_t* nominated, char* buf, size_t cap, size_t* len);

/* ---- per-node results of one cycle for concurrent readers.  The framework
 * calls Filter (wrappedplugin.go:523-548) and Score (:420-445) from its 16
 * parallelize.Until workers and NormalizeScore (:388-415) per plugin; a Go
 * plugin acquires the cycle's view once (the cycle's first PreFilter, after
 * ksg_cycle; kept in CycleState) and its per-node calls index these immutable
 * arrays — no library call, no lock.  Local node i is global node
 * node_offset + i.  The device builds the view (one kernel, one copy into a
 * pinned host block): the per-node Filter outcome is stored once per node, not
 * per position.  Filter of profile position pos on node i returns
 *   -1 (not called)               if !filter_called[pos] or fail_pos[i] < 0 or pos > fail_pos[i]
 *   Success (0)                    if pos < fail_pos[i]  (fail_pos[i] == n_positions: passed every filter)
 *   fail_code[i], messages[fail_msg[i]]   if pos == fail_pos[i]
 * Codes are framework.Code values (as ksg_filter_status).  score[pos] /
 * normalized[pos] point at n_nodes signed little-endian integers of
 * score_bytes[pos] / normalized_bytes[pos] bytes each (1, 2 or 4: the narrowest
 * width the cycle's values need, so fewer bytes cross the host link; read them
 * with ksg_view_score), NULL when there is no device Score at pos; valid where
 * the node passed every filter; normalized[pos] == score[pos] for plugins
 * without ScoreExtensions.  A view stays valid, unchanged, until
 * ksg_cycle_view_release, whatever the context does meanwhile (later cycles,
 * Reserve, events, ksg_destroy); release needs no context and may run on any
 * thread. */
typedef struct ksg_cycle_view {
  uint32_t q;                          /* queue pod */
  uint32_t n_positions;                /* profile positions */
  uint32_t node_offset;                /* global index of local node 0 */
  uint32_t n_nodes;                    /* local nodes */
  ksg_pod_result result;               /* the cycle's outcome (engine selectHost) */
  const uint8_t* filter_called;        /* [pos] 1: the framework calls this position's Filter */
  const int8_t* fail_pos;              /* [node] first failing position; n_positions: passed; -1: not evaluated */
  const int8_t* fail_code;             /* [node] framework code of that failure */
  const uint16_t* fail_msg;            /* [node] its Status.Message(): index into messages */
  const void* const* score;            /* [pos] -> [node] raw Score (score_bytes[pos] each), or NULL */
  const void* const* normalized;       /* [pos] -> [node] NormalizeScore output, or NULL */
  const uint8_t* score_bytes;          /* [pos] width of score[pos]'s values: 1, 2 or 4 */
  const uint8_t* normalized_bytes;     /* [pos] width of normalized[pos]'s values */
  const int8_t* prefilter_code;        /* [pos] PreFilter code (ksg_prefilter_status) */
  const uint16_t* prefilter_msg;       /* [pos] its message index */
  const int8_t* prescore_code;         /* [pos] PreScore code (ksg_prescore_status) */
  const uint16_t* prescore_msg;        /* [pos] its message index */
  const char* const* messages;         /* message table; messages[0] == "" */
  uint32_t n_messages;
  const void* owner;                   /* library-private */
} ksg_cycle_view;
/* The raw (normalized == 0) or normalized score of position pos on local node i. */
static inline int64_t ksg_view_score(const ksg_cycle_view* v, uint32_t pos, uint32_t i, int normalized) {
  const void* row = normalized ? v->normalized[pos] : v->score[pos];
  const uint8_t w = normalized ? v->normalized_bytes[pos] : v->score_bytes[pos];
  if (!row) return 0;
  if (w == 1) return ((const int8_t*)row)[i];
  if (w == 2) return ((const int16_t*)row)[i];
  return ((const int32_t*)row)[i];
}
/* Snapshot the kept outputs of queue pod q (the pod of the last ksg_cycle, or a
 * ksg_keep_outputs range) into a view.  For the pod of the last ksg_cycle with
 * commit = 0, acquired before any other state-changing call, the view was filled
 * behind that cycle's own kernels and is returned without a device launch. */
int ksg_cycle_view_acquire(ksg_ctx* ctx, uint32_t q, const ksg_cycle_view** out);
void ksg_cycle_view_release(const ksg_cycle_view* view);

/* Scheduler-cache events between cycles (replaces the informer -> Cache path:
 * Cache.AddNode/UpdateNode/RemoveNode/AddPod/UpdatePod/RemovePod of upstream
 * v1.30.4 pkg/scheduler/internal/cache/cache.go, driven by eventhandlers.go;
 * the simulator raises them from its apiserver).  JSON:
 *   {"events": [{"op": "addNode"|"updateNode", "node": {v1.Node}},
 *               {"op": "removeNode", "name": "node-x"},
 *               {"op": "addPod"|"updatePod", "pod": {v1.Pod with spec.nodeName}},
 *               {"op": "removePod", "name": "p", "namespace": "ns"}, ...]}
 * applied in order; the batch is all-or-nothing.  removePod also takes a queue
 * pod that was scheduled (its placement is released, its result kept);
 * removeNode requires that no pod is bound or assumed on the node (upstream
 * deletes the node's pods first).  Batches of bound-pod add/remove events,
 * deletions of queue pods scheduled since the last encode, and node updates of
 * allocatable, spec.unschedulable, labels (keys and values some node already
 * carried, no topology key changing value) and taints (taints some node already
 * carried) with the same images, all bringing no new vocabulary, are applied in
 * place on the device; any other batch re-encodes the snapshot (after an in-place
 * batch ksg_reset is refused: reload).  Placements of scheduled queue pods are kept;
 * node indices after a removed node shift down by one.  Per-node outputs kept for
 * pods scheduled before the batch are not re-indexed. */
int ksg_apply_events(ksg_ctx* ctx, const char* events_json, size_t len);

/* Device node rows (assume parity): requested [n_res][n], pod count [n]. */
int ksg_node_requested(ksg_ctx* ctx, int64_t* requested, int32_t* pod_count, uint32_t n_res, uint32_t n);
/* NonZeroRequested rows (Fit scoring input): cpu in nonzero[0..n), memory in nonzero[n..2n). */
int ksg_node_nonzero(ksg_ctx* ctx, int64_t* nonzero, uint32_t n);

/* Harness mode (benchmarks, full-size tests; no context): the synthetic cluster
 * document of BASELINE.json config 2..5 — the document
 * ksg/generator.py builds, from the same seeded draws.  Sizes < 0: the config's
 * default; seed 0: the config's seed.  *out is malloc'd: release with ksg_free. */
int ksg_synth_cluster(int config, int64_t n_nodes, int64_t n_pods, int64_t n_existing, int64_t n_zones, uint64_t seed,
                      char** out, size_t* len);
void ksg_free(void* p);

#ifdef __cplusplus
}
#endif
#endif /* KSG_H_ */
