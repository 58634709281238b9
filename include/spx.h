/*
 * spx.h — C ABI of the MI355X batched Filter/Score engine (libspx.so).
 *
 * This is the drop-in boundary for the one hot path of kubernetes-sigs/scheduler-plugins:
 * the per-pod x per-node Filter()/Score()/NormalizeScore() loops.  A Go plugin keeps its
 * framework.FilterPlugin / framework.ScorePlugin method signatures and binds these entry
 * points through cgo (INTEGRATION.md shows the stub).  Reference interfaces replaced:
 *
 *   Allocatable.Score / NormalizeScore   pkg/noderesources/allocatable.go:63,143
 *   TargetLoadPacking.Score              pkg/trimaran/targetloadpacking/targetloadpacking.go:107
 *   LoadVariationRiskBalancing.Score     pkg/trimaran/loadvariationriskbalancing/loadvariationriskbalancing.go:84
 *   TopologyMatch.Filter / Score         pkg/noderesourcetopology/filter.go:179, score.go:62
 *   NetworkOverhead.PreFilter/Filter/Score/NormalizeScore
 *                                        pkg/networkaware/networkoverhead/networkoverhead.go:174,326,362,389
 *   TopologicalSort.Less                 pkg/networkaware/topologicalsort/topologicalsort.go:102
 *   CapacityScheduling.PreFilter         pkg/capacityscheduling/capacity_scheduling.go:208
 *   NodeMetadata.Score / NormalizeScore  pkg/nodemetadata/node_metadata.go:57,150
 *   PodState.Score / NormalizeScore      pkg/podstate/pod_state.go:42,66
 *   QOSSort.Less                         pkg/qos/queue_sort.go:46
 *
 * Rules of the boundary (cgo-safe):
 *   - every function returns int: 0 = ok, <0 = error (spx_last_error() gives the text);
 *   - all tables are flat arrays of fixed-width ints/doubles, caller-owned and only
 *     borrowed for the duration of the call (no pointer is retained, no pointer-to-pointer);
 *   - results live in device memory owned by the engine; rows are fetched into
 *     caller-provided buffers; fetches after spx_sync() are read-only and lock-free, so
 *     16 concurrent reader goroutines (upstream Parallelizer) may call spx_fetch_* at once;
 *   - no global state (unlike targetloadpacking.go:49-53): one engine per scheduler profile.
 *
 * Two table levels exist:
 *   "object tables"  (spx_*_objects): a lossless columnar/CSR image of the API objects the
 *                    reference reads (pods, nodes, watcher metrics, NRT zones, AppGroups ...);
 *                    this is what the Go shim marshals.
 *   "SoA tables"     (spx_*_soa): dense per-node / per-pod columns the kernels read from HBM.
 *   spx_flatten_*() (host C++, part of this library) turns the former into the latter.
 *
 * The header is kept in a regular "one field per line" form because the Python ctypes
 * binding (scheduler-plugins_amd/_abi.py) parses it — it is the single source of truth.
 */
#ifndef SPX_H
#define SPX_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------ constants */

#define SPX_OK 0
#define SPX_ERR_ARG (-1)
#define SPX_ERR_HIP (-2)
#define SPX_ERR_STATE (-3)
#define SPX_ERR_NOGPU (-4)

/* plugin ids (bit i of a plugin mask = plugin i) */
#define SPX_PLUGIN_ALLOCATABLE 0
#define SPX_PLUGIN_TLP 1
#define SPX_PLUGIN_LVRB 2
#define SPX_PLUGIN_NRT 3
#define SPX_PLUGIN_NETOVERHEAD 4
#define SPX_PLUGIN_CAPACITY 5
#define SPX_PLUGIN_TOPOSORT 6
#define SPX_PLUGIN_LROC 7  /* trimaran LowRiskOverCommitment */
#define SPX_PLUGIN_PEAKS 8 /* trimaran Peaks */
#define SPX_PLUGIN_SYSCHED 9 /* SySched (pkg/sysched) */
/* Coscheduling (pkg/coscheduling): a PreFilter gate per pending pod.  The id lies inside the per-plugin arrays SPX_NUM_PLUGINS sizes
 * (on the host and in the argmax kernels) but owns no score table and no status table there, and its entry of the weight vector is
 * ignored; bit 10 of a plugin mask is accepted by spx_eval, spx_eval_best, spx_decide and spx_fetch_prefilter, and the table calls
 * (spx_fetch_scores, spx_score_table, spx_bind_score_table ...) refuse the id. */
#define SPX_PLUGIN_COSCHED 10
#define SPX_PLUGIN_NODEMETA 11 /* NodeMetadata (pkg/nodemetadata) */
#define SPX_PLUGIN_PODSTATE 12 /* PodState (pkg/podstate) */
#define SPX_NUM_PLUGINS 13
#define SPX_NUM_PLUGIN_IDS 13

/* fwk.Status codes (k8s.io/kube-scheduler/framework) */
#define SPX_STATUS_SUCCESS 0
#define SPX_STATUS_ERROR 1
#define SPX_STATUS_UNSCHEDULABLE 2

/* Coscheduling PreFilter status per pending pod (0 = Success), in the order PodGroupManager.PreFilter returns them
 * (pkg/coscheduling/core/core.go:243-305) */
#define SPX_COSCHED_ST_BACKED_OFF 1   /* the group is in backedOffPG                              :251-253 */
#define SPX_COSCHED_ST_FEW_SIBLINGS 2 /* MinMember - listed pods > 0                              :262-266 */
#define SPX_COSCHED_ST_GATED 3        /* MinMember - listed + gated > 0                           :270-277 */
#define SPX_COSCHED_ST_RESOURCE_GAP 4 /* CheckClusterResource failed on MinResources + pods       :295-302 */
#define SPX_COSCHED_MAX_SLOTS 16

/* canonical resource ids; quantities are int64 in canonical units:
 * cpu = millicores (Quantity.MilliValue()), everything else = Quantity.Value() */
#define SPX_RES_CPU 0
#define SPX_RES_MEMORY 1
#define SPX_RES_EPHEMERAL 2
#define SPX_RES_PODS 3
#define SPX_RES_STORAGE 4
#define SPX_RES_FIRST_DYNAMIC 8

/* resource class flags (spx_resource_classes.flags[id]) */
#define SPX_RC_HUGEPAGE 1   /* v1helper.IsHugePageResourceName  */
#define SPX_RC_NATIVE 2     /* v1helper.IsNativeResource        */
#define SPX_RC_SCALAR 4     /* schedutil.IsScalarResourceName   */

/* container kinds */
#define SPX_CTR_APP 0
#define SPX_CTR_INIT 1
#define SPX_CTR_SIDECAR 2 /* init container with restartPolicy Always (pkg/util/sidecar.go) */

/* watcher metric types / operators (paypal/load-watcher v0.2.4 constants, resolved by the shim) */
#define SPX_MT_CPU 0
#define SPX_MT_MEMORY 1
#define SPX_MT_OTHER 2
#define SPX_MO_AVG 0
#define SPX_MO_STD 1
#define SPX_MO_LATEST 2
#define SPX_MO_EMPTY 3 /* Operator == "" */
#define SPX_MO_OTHER 4

/* Allocatable modes (apis/config/types.go ModeType) */
#define SPX_MODE_LEAST 0
#define SPX_MODE_MOST 1

/* ------------------------------------------------------------------ object tables */

/* class flags per resource id (ids are interned by the caller once per snapshot) */
typedef struct spx_resource_classes {
  int32_t n_res;
  const uint8_t* flags;
} spx_resource_classes;

/* v1.Pod image.  Containers of pod i are ctr_ptr[i]..ctr_ptr[i+1]-1, init containers first
 * (spec order) then app containers (spec order) — the order
 * append(pod.Spec.InitContainers, pod.Spec.Containers...) the reference walks.
 * Resource lists are CSR: container c requests = req_res/req_qty[req_ptr[c]..req_ptr[c+1]). */
typedef struct spx_pod_objects {
  int64_t n_pods;
  const int32_t* ctr_ptr;
  const uint8_t* ctr_kind;
  const int32_t* req_ptr;
  const int32_t* req_res;
  const int64_t* req_qty;
  const int32_t* lim_ptr;
  const int32_t* lim_res;
  const int64_t* lim_qty;
  const int32_t* ovh_ptr;
  const int32_t* ovh_res;
  const int64_t* ovh_qty;
  const int32_t* priority;
  const int64_t* queue_ts;
  const int32_t* appgroup;
  const int32_t* selector;
  const int32_t* ns;
} spx_pod_objects;

/* framework.NodeInfo / v1.Node image */
typedef struct spx_node_objects {
  int64_t n_nodes;
  const int64_t* alloc_cpu_milli;
  const int64_t* alloc_mem;
  const int64_t* alloc_eph;
  const int64_t* alloc_pods;
  const int32_t* scalar_ptr;
  const int32_t* scalar_res;
  const int64_t* scalar_qty;
  const int64_t* cap_cpu_milli;
  const int32_t* region;
  const int32_t* zone;
} spx_node_objects;

/* watcher.WatcherMetrics image (pkg/trimaran/collector.go:110-123) */
typedef struct spx_metrics_objects {
  int32_t map_is_nil;
  int64_t window_end;
  const uint8_t* node_present;
  const uint8_t* node_metrics_nil;
  const int32_t* m_ptr;
  const uint8_t* m_type;
  const uint8_t* m_op;
  const double* m_value;
} spx_metrics_objects;

/* PodAssignEventHandler.ScheduledPodsCache image (pkg/trimaran/handler.go:47-58):
 * entries of node n are e_ptr[n]..e_ptr[n+1]-1; e_pod indexes `pods` */
typedef struct spx_assigned_objects {
  const int32_t* e_ptr;
  const int64_t* e_ts_unix;
  const int32_t* e_pod;
  const spx_pod_objects* pods;
} spx_assigned_objects;

/* framework.NodeInfo.GetPods() image (what trimaran.GetNodeRequestsAndLimits walks, pkg/trimaran/resourcestats.go:163-206):
 * the pods already on node n are p_pod[p_ptr[n]..p_ptr[n+1]), indexes into `pods` */
typedef struct spx_node_pods_objects {
  const int32_t* p_ptr;
  const int32_t* p_pod;
  const spx_pod_objects* pods;
} spx_node_pods_objects;

/* PeaksArgs.NodePowerModel image (apis/config/types.go:309-324): the power model of node n as getPowerModel resolves it by
 * node name (peaks.go:190-196); all three are 0 for a node without an entry */
typedef struct spx_power_model_objects {
  const double* k0;
  const double* k1;
  const double* k2;
} spx_power_model_objects;

/* SySched (pkg/sysched/sysched.go): everything Score reads, with syscall names interned to ids 0..n_names-1 (at most
 * SPX_SYSCHED_MAX_NAMES).  The distinct syscall sets getSyscalls resolves (:124-210) are a CSR: set s holds the name ids
 * set_name[set_ptr[s] .. set_ptr[s+1]) (any order, repeats allowed; an empty set is legal: Score answers math.MaxInt64 for such
 * a pod, :249-251).  pod_set[p] is pending pod p's set.  Per node: host_present = HostSyscalls has an entry (:253-259), the
 * cached set itself as the CSR host_ptr / host_name, and the resident pods HostToPods lists (:267) as set ids res_set[res_ptr[n]
 * .. res_ptr[n+1]) — Score recomputes getSyscalls for each of them, so a resident's set may hold names the cached host set lacks
 * (a SeccompProfile that changed after addPod). */
#define SPX_SYSCHED_MAX_NAMES 1024
#define SPX_SYSCHED_MAX_WORDS 16 /* 64-bit words of a bitset over the names */
typedef struct spx_sysched_objects {
  int32_t n_names;
  int32_t n_sets;
  const int32_t* set_ptr;
  const int32_t* set_name;
  int64_t n_pods;
  const int32_t* pod_set;
  int64_t n_nodes;
  const uint8_t* host_present;
  const int32_t* host_ptr;
  const int32_t* host_name;
  const int32_t* res_ptr;
  const int32_t* res_set;
} spx_sysched_objects;

/* Coscheduling (pkg/coscheduling/core/core.go): what PodGroupManager.PreFilter and Coscheduling.Less read.
 * Groups: one entry per PodGroup full name ("namespace/label value") that a pod of the snapshot carries or a PodGroup object has.
 * g_ns / g_name are the caller's interned ids of the two halves (kept for the caller; the flatteners identify a group by its
 * index).  g_exists = the PodGroup object exists (GetPodGroup's pg != nil, :392-402); the columns after it up to g_permitted
 * are read only for such a group.  MinResources is the CSR g_res_ptr / g_res_id / g_res_qty in canonical units (cpu in milli,
 * rounded up: spx_ingest_quantity(text, 1, ..)); an entry for SPX_RES_PODS is ignored, PreFilter overwrites it with MinMember
 * (:296-297).  g_backed_off / g_permitted: the group is in backedOffPG / permittedPG now (TTL caches the control plane owns; the
 * engine does not age them).  g_created_ns = PodGroup.CreationTimestamp, g_has_last_failed / g_last_failed_ns =
 * lastFailedSchedulePG (:368-384; it is looked up by full name, so it may be set for a group that does not exist).
 * g_listed = pods of the namespace that carry the label, pending and assigned (podLister, :255-257); g_gated = those of them with
 * SchedulingGates.  pod_group[p] = pending pod p's group or -1 (no label).
 * Assigned pods: node n hosts the entries a_ptr[n] .. a_ptr[n+1]; a_group = the entry's group or -1; its effective request
 * (what NodeInfo.AddPod charged: max(sum of containers, init containers) + overhead) is the CSR a_req_ptr / a_req_res / a_req_qty.
 * Every pod on the node must be listed: the node's Requested and its pod count are their sums.  node_present = Node() != nil. */
typedef struct spx_cosched_objects {
  int32_t n_groups;
  const int32_t* g_ns;
  const int32_t* g_name;
  const uint8_t* g_exists;
  const int32_t* g_min_member;
  const uint8_t* g_has_min_resources;
  const int32_t* g_res_ptr;
  const int32_t* g_res_id;
  const int64_t* g_res_qty;
  const uint8_t* g_backed_off;
  const uint8_t* g_permitted;
  const int64_t* g_created_ns;
  const uint8_t* g_has_last_failed;
  const int64_t* g_last_failed_ns;
  const int32_t* g_listed;
  const int32_t* g_gated;
  int64_t n_pods;
  const int32_t* pod_group;
  int64_t n_nodes;
  const uint8_t* node_present;
  const int32_t* a_ptr;
  const int32_t* a_group;
  const int32_t* a_req_ptr;
  const int32_t* a_req_res;
  const int64_t* a_req_qty;
} spx_cosched_objects;

/* NodeResourceTopology CR image per node plus the NRT cache's verdict for it
 * (pkg/noderesourcetopology/cache: GetCachedNRTCopy -> (nrt, CachedNRTInfo{Fresh})).
 * legacy_policy encodes TopologyPolicies[0] (nodeconfig/topologymanager.go:131-162) as
 * (policy << 1) | scope, -1 when absent/unknown; attr_* are the Attributes overrides (:98-115),
 * -1 when absent or invalid.  policy: 0 none, 1 best-effort, 2 restricted, 3 single-numa-node;
 * scope: 0 container, 1 pod.  zone_numa_id / zcost_numa_id = numanode.NameToID(name), -1 on error.
 * assumed_* is the OverReserve store (cache/store.go:315-356): one resource list per assumed pod. */
typedef struct spx_nrt_objects {
  int64_t n_nodes;
  const uint8_t* has_nrt;
  const uint8_t* fresh;
  const int8_t* legacy_policy;
  const int8_t* attr_scope;
  const int8_t* attr_policy;
  const int32_t* attr_max_numa;
  const int32_t* zone_ptr;
  const uint8_t* zone_is_node;
  const int32_t* zone_numa_id;
  const int32_t* zres_ptr;
  const int32_t* zres_res;
  const int64_t* zres_avail;
  const int32_t* zcost_ptr;
  const int32_t* zcost_numa_id;
  const int64_t* zcost_value;
  const int32_t* assumed_ptr;
  const int32_t* arl_ptr;
  const int32_t* arl_res;
  const int64_t* arl_qty;
  const int64_t* zres_allocatable; /* optional (may be NULL), same layout as zres_avail: ResourceInfo.Allocatable; only the eviction simulation reads it */
} spx_nrt_objects;

/* diktyo AppGroup CRs (appgroup.diktyo.x-k8s.io v1alpha1) as the network-aware plugins read them.
 * Group g: Spec.Workloads = wl_ptr[g]..wl_ptr[g+1]-1 with their Dependencies (dep_*), Status.TopologyOrder
 * (topo_*), and the scheduled list util.GetScheduledList builds from the pod lister (placed_*: pods labelled
 * with the group that already have a node name; placed_node = index of that node in the snapshot).
 * Selector ids MUST preserve the lexicographic order of the selector strings: util.FindPodOrder
 * (pkg/networkaware/util/util.go:138-153) binary-searches TopologyOrder with string comparisons. */
typedef struct spx_appgroup_objects {
  int32_t n_groups;
  const int32_t* wl_ptr;
  const int32_t* wl_selector;
  const int32_t* dep_ptr;
  const int32_t* dep_selector;
  const int64_t* dep_max_cost;
  const int32_t* topo_ptr;
  const int32_t* topo_selector;
  const int32_t* topo_index;
  const int32_t* placed_ptr;
  const int32_t* placed_selector;
  const int32_t* placed_node;
} spx_appgroup_objects;

/* NetworkTopology CR (networktopology.diktyo.x-k8s.io v1alpha1), the weights set the plugin was configured
 * with (no.weightsName), keyed by interned label values: region ids and zone ids are the same id spaces as
 * spx_node_objects.region / .zone.  Origin o's CostList is the slice [ptr[o], ptr[o+1]) of the dest and cost arrays; later entries
 * for the same destination override earlier ones (map assignment, networkoverhead.go:467-472). */
typedef struct spx_nettopo_objects {
  int32_t n_regions;
  int32_t n_zones;
  const int32_t* rc_ptr;
  const int32_t* rc_dest;
  const int64_t* rc_cost;
  const int32_t* zc_ptr;
  const int32_t* zc_dest;
  const int64_t* zc_cost;
} spx_nettopo_objects;

/* CapacityScheduling: ElasticQuotaInfos + nominated pods (pkg/capacityscheduling/elasticquota.go:62-68,
 * capacity_scheduling.go:231-253).  A framework.Resource is a vector of SPX_QUOTA_SLOTS int64:
 * [0] MilliCPU [1] Memory [2] EphemeralStorage [3] AllowedPodNumber [4..7] ScalarResources by slot
 * (quota_scalar_res gives the canonical resource id of each scalar slot); *_present bit s (4..7) = the
 * scalar key exists in that Resource's map.  Quotas are indexed by namespace id (spx_pod_objects.ns). */
#define SPX_QUOTA_SLOTS 8
#define SPX_QUOTA_ST_OVER_MAX 1 /* "...is rejected in PreFilter because ElasticQuota %v is more than Max"      capacity_scheduling.go:276 */
#define SPX_QUOTA_ST_OVER_MIN 2 /* "...is rejected in PreFilter because total ElasticQuota used is more than min" :280 */
typedef struct spx_quota_objects {
  int32_t n_namespaces;
  int32_t n_scalar_slots;
  const int32_t* scalar_res;
  const uint8_t* has_quota;
  const int64_t* min;
  const uint8_t* min_present;
  const int64_t* max;
  const uint8_t* max_present;
  const int64_t* used;
  const uint8_t* used_present;
  int64_t n_nominated;
  const int32_t* nom_ns;
  const int32_t* nom_priority;
  const int64_t* nom_pending_index;
  const spx_pod_objects* nom_pods;
} spx_quota_objects;

/* ------------------------------------------------------------------ plugin params */

typedef struct spx_allocatable_params {
  int32_t mode;
  int32_t n_res;
  const int32_t* res;
  const int64_t* weight;
} spx_allocatable_params;

typedef struct spx_tlp_params {
  int64_t target_utilization;
  int64_t default_requests_milli;
  double requests_multiplier;
} spx_tlp_params;

typedef struct spx_lvrb_params {
  double safe_variance_margin;
  double safe_variance_sensitivity;
} spx_lvrb_params;

/* LowRiskOverCommitmentArgs after defaulting (apis/config/v1/defaults.go:172-188): SmoothingWindowSize > 0,
 * RiskLimitWeights["cpu"/"memory"] (lowriskovercommitment.go:76-81) */
typedef struct spx_lroc_params {
  int64_t smoothing_window_size;
  double risk_limit_weight_cpu;
  double risk_limit_weight_mem;
} spx_lroc_params;

/* NodeResourceTopologyMatch scoring strategy (apis/config/types.go ScoringStrategyType) */
#define SPX_NRT_MOST_ALLOCATED 0
#define SPX_NRT_BALANCED_ALLOCATION 1
#define SPX_NRT_LEAST_ALLOCATED 2
#define SPX_NRT_LEAST_NUMA_NODES 3

typedef struct spx_nrt_params {
  int32_t strategy;
  int32_t n_weights;
  const int32_t* weight_res;
  const int64_t* weight;
} spx_nrt_params;

/* ------------------------------------------------------------------ SoA tables (what the kernels read) */

/* Allocatable: alloc is [n_res][n_nodes] resource-major, rows in spx_allocatable_params.res order */
typedef struct spx_alloc_nodes_soa {
  int64_t n_nodes;
  int32_t n_res;
  const int64_t* alloc;
} spx_alloc_nodes_soa;

/* trimaran node columns (TLP reads Capacity, LVRB reads Allocatable — SURVEY appendix B.6) */
typedef struct spx_trimaran_nodes_soa {
  int64_t n_nodes;
  const int64_t* cap_cpu_milli;
  const double* tlp_cpu_util;
  const int64_t* tlp_missing_milli;
  const uint8_t* tlp_valid;
  const int64_t* lv_alloc_cpu_milli;
  const int64_t* lv_alloc_mem;
  const double* lv_cpu_avg;
  const double* lv_cpu_std;
  const double* lv_mem_avg;
  const double* lv_mem_std;
  const uint8_t* lv_flags;
} spx_trimaran_nodes_soa;

#define SPX_LV_HAS_METRICS 1
#define SPX_LV_CPU_VALID 2
#define SPX_LV_MEM_VALID 4

typedef struct spx_trimaran_pods_soa {
  int64_t n_pods;
  const int64_t* tlp_pod_milli;
  const int64_t* lv_req_cpu_milli;
  const int64_t* lv_req_mem;
} spx_trimaran_pods_soa;

/* LowRiskOverCommitment.  Reads the LVRB columns of spx_trimaran_nodes_soa (allocatable, avg/std, flags:
 * the same CreateResourceStats / GetResourceData inputs) plus, per node, the sums GetNodeRequestsAndLimits accumulates over the
 * pods already on it (requests, and limits raised to the requests; resourcestats.go:184-206, before the capacity caps) */
typedef struct spx_lroc_nodes_soa {
  int64_t n_nodes;
  const int64_t* req_cpu_milli;
  const int64_t* req_mem;
  const int64_t* lim_cpu_milli;
  const int64_t* lim_mem;
} spx_lroc_nodes_soa;

/* PodResourcesStateData (lowriskovercommitment.go:259-275): requests, and limits raised to the requests */
typedef struct spx_lroc_pods_soa {
  int64_t n_pods;
  const int64_t* req_cpu_milli;
  const int64_t* req_mem;
  const int64_t* lim_cpu_milli;
  const int64_t* lim_mem;
} spx_lroc_pods_soa;

/* Peaks.  cpu_util is the FIRST cpu metric whose operator is AVG or Latest (peaks.go:117-126; TLP takes
 * the last one, LVRB prefers AVG — three different selections); valid = the node has metrics and such a
 * metric exists; cap_cpu_milli is node.Status.Capacity (:131) */
typedef struct spx_peaks_nodes_soa {
  int64_t n_nodes;
  const int64_t* cap_cpu_milli;
  const double* cpu_util;
  const uint8_t* valid;
  const double* k1;
  const double* k2;
} spx_peaks_nodes_soa;

/* resource.GetResourceRequestQuantity(pod, cpu).MilliValue() (peaks.go:114-115) */
typedef struct spx_peaks_pods_soa {
  int64_t n_pods;
  const int64_t* cpu_milli;
} spx_peaks_pods_soa;

/* SySched.  With H the node's cached host set, Q_q its resident pods' sets, k = n_resident and P the pending pod's set,
 * Score (sysched.go:261-278) is |H \ P| + sum_q |(H u P) \ Q_q| = popc(H & ~P) + a + k popc(P & ~H) - sum over b in P \ H of c[b],
 * a = resident_missing = sum_q |H \ Q_q| and c[b] = the residents whose set holds b.  The last term exists only on nodes with a
 * resident set that is not inside H; those carry the (b, c[b]) pairs with b outside H and c[b] > 0 in the CSR stale_ptr [N+1] /
 * stale_bit / stale_count.  host_bits is word-major [n_words][n_nodes] (bit b of the set = bit b % 64 of word b / 64), zero for
 * a node that is not present; n_words = ceil(n_names / 64) <= SPX_SYSCHED_MAX_WORDS.  Every score must stay below
 * SPX_SYSCHED_MAX_SCORE (100 x score is formed in 32 bits): a + (k + 1) n_names of every node is checked at the upload. */
#define SPX_SYSCHED_MAX_SCORE 21474836
typedef struct spx_sysched_nodes_soa {
  int64_t n_nodes;
  int32_t n_words;
  const uint64_t* host_bits;
  const uint8_t* present;
  const int32_t* n_resident;
  const int32_t* resident_missing;
  const int32_t* stale_ptr;
  const int32_t* stale_bit;
  const int32_t* stale_count;
} spx_sysched_nodes_soa;

/* the distinct sets as bitsets, set_bits [n_sets][n_words], and each pending pod's set */
typedef struct spx_sysched_pods_soa {
  int64_t n_pods;
  int32_t n_words;
  int32_t n_sets;
  const uint64_t* set_bits;
  const int32_t* pod_set;
} spx_sysched_pods_soa;

/* Coscheduling.  CheckClusterResource (core.go:406-426) subtracts, node by node in list order, what getNodeResource (:433-467)
 * leaves on the node once the group's own pods are removed, and deletes a resource for good the first time it is <= 0.  So with
 * left_g[i][r] = left_base[r][i] + (what g's pods on node i requested, +1 pod each) and S_g,r[i] its prefix sum over the present
 * nodes up to i, the check succeeds iff every named resource has a present node i with S_g,r[i] >= req_r.
 * Slots: the resources any group's MinResources names plus SPX_RES_PODS, ascending id, at most SPX_COSCHED_MAX_SLOTS.
 * left_base is slot-major [n_slots][n_nodes], 0 on a node that is not present or does not list the resource.  req [n_groups]
 * [n_slots] with req_mask (bit s = slot s named; 0 for a group without MinResources or without a PodGroup object).  The steps of
 * group g are step_ptr[g] .. step_ptr[g+1]: step_node strictly ascending present nodes, step_add [n_steps][n_slots] >= 0.
 * Limits: for every slot, sum_i |left_base| + sum over all steps of step_add < 2^62, and |req| < 2^62 (spx_cosched_check). */
typedef struct spx_cosched_soa {
  int64_t n_nodes;
  int32_t n_slots;
  const int32_t* slot_res;
  const int64_t* left_base;
  const uint8_t* node_present;
  int32_t n_groups;
  const uint8_t* g_exists;
  const int32_t* min_member;
  const uint8_t* has_min_resources;
  const uint8_t* backed_off;
  const uint8_t* permitted;
  const int32_t* listed;
  const int32_t* gated;
  const int64_t* req;
  const uint32_t* req_mask;
  const int32_t* step_ptr;
  const int32_t* step_node;
  const int64_t* step_add;
  int64_t n_pods;
  const int32_t* pod_group;
} spx_cosched_soa;

/* NodeResourceTopologyMatch.  Resources are renumbered into dense "slots" 0..n_res-1 (the union of
 * what pods request and zones report; slot_res gives the canonical id).  Limits of this build:
 * NUMA zones per node <= SPX_NRT_TALL_MAX_ZONES = 64 with ids 0..63 (flatten fails beyond them).  The dense
 * node table holds up to SPX_NRT_MAX_ZONES = 8 zones per node; a node with 9 to 64 zones is a "tall node" —
 * n_zones = SPX_NRT_ZONES_TALL, zone quantities zero, flags those of a node without an NRT object — whose
 * zones travel in spx_nrt_tall_nodes and are evaluated by kernels_nrt_tall.hip after the dense sweep.  With
 * LeastNUMANodes a tall node may list up to SPX_NRT_TALL_MAX_ZONES_LEAST_NUMA = 16 zones (65 535 subsets).
 * Tall nodes are declined, by an error that says so, in spx_commit_sequential with NodeResourceTopologyMatch,
 * in spx_update_nrt_nodes and in a wide snapshot.  The dense tables below (spx_nrt_nodes_soa,
 * spx_nrt_pods_soa) hold n_res <= SPX_NRT_MAX_RES = 8 slots, and spx_flatten_nrt_slots fails beyond 8.
 * A snapshot with up to SPX_NRT_MAX_RES_WIDE = 32 slots travels in the wide tables (spx_nrt_nodes_wide,
 * spx_nrt_pods_wide; spx_flatten_nrt_slots_wide), which spx_load_nrt takes by itself above 8 slots; a wide
 * snapshot's pods may hold up to SPX_NRT_WIDE_MAX_CTRS containers each.  In the dense tables containers
 * per pod are unbounded: a pod with up to SPX_NRT_MAX_CTRS containers keeps them in the dense pod table; a
 * pod with more is a "long row" — n_ctr = SPX_NRT_CTRS_LONG, per-container columns zero, pod-level columns
 * (qos, non_native, pod_present, pod_req) filled as for any row — whose containers travel in
 * spx_nrt_long_pods. */
#define SPX_NRT_MAX_RES 8
#define SPX_NRT_MAX_RES_WIDE 32
#define SPX_NRT_WIDE_MAX_CTRS 64
#define SPX_NRT_MAX_ZONES 8
#define SPX_NRT_ZONES_TALL 255
#define SPX_NRT_TALL_MAX_ZONES 64
#define SPX_NRT_TALL_MAX_ZONES_LEAST_NUMA 16
#define SPX_NRT_MAX_CTRS 8
#define SPX_NRT_CTRS_LONG 255
#define SPX_NRT_F_HAS_NRT 1
#define SPX_NRT_F_FRESH 2
#define SPX_NRT_F_SINGLE_NUMA 4
#define SPX_NRT_F_POD_SCOPE 8
#define SPX_NRT_SLOT_AFFINE 1     /* isNUMAAffineResource  numaresources.go:120-135 */
#define SPX_NRT_SLOT_HOST_LEVEL 2 /* isHostLevelResource   numaresources.go:105-118 */
#define SPX_NRT_SLOT_CPU 4        /* quantity is millicores: Value() = ceil(milli/1000) */
#define SPX_QOS_GUARANTEED 0
#define SPX_QOS_BURSTABLE 1
#define SPX_QOS_BESTEFFORT 2

/* filter status reason codes of the NRT status table (0 = pass) and their reference messages */
#define SPX_NRT_ST_INVALID_TOPOLOGY 1 /* "invalid node topology data"      filter.go:199 */
#define SPX_NRT_ST_INIT_CONTAINER 2   /* "cannot align init container"     filter.go:55  */
#define SPX_NRT_ST_SIDECAR_CONTAINER 3/* "cannot align sidecar container"  filter.go:55  */
#define SPX_NRT_ST_CONTAINER 4        /* "cannot align container"          filter.go:67  */
#define SPX_NRT_ST_POD 5              /* "cannot align pod"                filter.go:172 */
/* fwk.Error, not Unschedulable: "inconsistent resource accounting" filter.go:73-77 — a container fits one of several zones that share
 * a NUMA id, is charged to every one of them, and a smaller one goes below zero (numaresources.go:145-182).  Infeasible like 1..5 */
#define SPX_NRT_ST_ERROR 255

typedef struct spx_nrt_slots {
  int32_t n_res;
  const int32_t* slot_res;
  const uint8_t* slot_flags;
  const int64_t* slot_weight;
} spx_nrt_slots;

typedef struct spx_nrt_nodes_soa {
  int64_t n_nodes;
  int32_t n_res;
  const uint8_t* flags;
  const int32_t* max_numa;
  const uint8_t* n_zones;
  const uint8_t* zone_id;
  const uint8_t* zone_present;
  const int64_t* zone_avail;
  const int32_t* zone_cost;
  const float* min_avg_dist;
  const uint8_t* node_present;
} spx_nrt_nodes_soa;

typedef struct spx_nrt_pods_soa {
  int64_t n_pods;
  int32_t n_res;
  const uint8_t* qos;
  const uint8_t* non_native;
  const uint8_t* n_ctr;
  const uint8_t* ctr_kind;
  const uint8_t* ctr_present;
  const int64_t* ctr_req;
  const uint8_t* pod_present;
  const int64_t* pod_req;
} spx_nrt_pods_soa;

/* The containers of the long rows of an spx_nrt_pods_soa batch, CSR: long row k is batch row pod_row[k] (ascending), its containers
 * ctr_ptr[k] .. ctr_ptr[k+1]-1 in document order (init and sidecar containers first, then app containers, as in spx_pod_objects);
 * ctr_kind / ctr_present / ctr_req [n_ctr][n_res] as the dense table's per-container columns. */
typedef struct spx_nrt_long_pods {
  int64_t n_long;
  int32_t n_res;
  const int32_t* pod_row;
  const int32_t* ctr_ptr;
  const uint8_t* ctr_kind;
  const uint8_t* ctr_present;
  const int64_t* ctr_req;
} spx_nrt_long_pods;

/* The tall nodes of an spx_nrt_nodes_soa table (n_zones = SPX_NRT_ZONES_TALL), host row-major: tall node k is node node_idx[k]
 * (ascending); zone_stride = the most zones any of them lists, shorter nodes padded (zone_id / zone_present / zone_avail 0, zone_cost
 * 255, min_avg_dist 255).  flags / max_numa / node_present / n_zones [n_tall] are the node's own (flags with SPX_NRT_F_HAS_NRT as the
 * snapshot has it); zone_id / zone_present / min_avg_dist [n_tall*zone_stride], zone_avail [n_tall*zone_stride*n_res], zone_cost
 * [n_tall*zone_stride*zone_stride] by list position (255 where Costs has no entry).  min_avg_dist[k*zone_stride + s-1] is
 * minAvgDistanceInCombinations for subsets of size s, filled for nodes of at most SPX_NRT_TALL_MAX_ZONES_LEAST_NUMA zones (255 above). */
typedef struct spx_nrt_tall_nodes {
  int64_t n_tall;
  int32_t n_res;
  int32_t zone_stride;
  const int32_t* node_idx;
  const uint8_t* flags;
  const int32_t* max_numa;
  const uint8_t* node_present;
  const uint8_t* n_zones;
  const uint8_t* zone_id;
  const uint8_t* zone_present;
  const int64_t* zone_avail;
  const int32_t* zone_cost;
  const float* min_avg_dist;
} spx_nrt_tall_nodes;

/* The wide NRT node table (up to SPX_NRT_MAX_RES_WIDE slots): the columns of spx_nrt_nodes_soa, host row-major, with uint32 presence
 * masks (bit s = slot s).  zone_id / zone_present / min_avg_dist [N*8], zone_avail [N*8*n_res], zone_cost [N*64], node_present [N]. */
typedef struct spx_nrt_nodes_wide {
  int64_t n_nodes;
  int32_t n_res;
  const uint8_t* flags;
  const int32_t* max_numa;
  const uint8_t* n_zones;
  const uint8_t* zone_id;
  const uint32_t* zone_present;
  const int64_t* zone_avail;
  const int32_t* zone_cost;
  const float* min_avg_dist;
  const uint32_t* node_present;
} spx_nrt_nodes_wide;

/* The wide NRT pod table, CSR throughout.  Pod p's effective request (GetPodEffectiveRequest with key presence) is the list
 * req_ptr[p] .. req_ptr[p+1]-1 of (req_slot, req_qty); its containers are ctr_ptr[p] .. ctr_ptr[p+1]-1 (document order: init and
 * sidecar containers first, then app containers), container c with kind ctr_kind[c] and request list ent_ptr[c] .. ent_ptr[c+1]-1
 * of (ent_slot, ent_qty).  Every list is in ascending slot order (= ascending resource id) and keeps zero quantities. */
typedef struct spx_nrt_pods_wide {
  int64_t n_pods;
  int32_t n_res;
  const uint8_t* qos;
  const uint8_t* non_native;
  const int32_t* req_ptr;
  const uint8_t* req_slot;
  const int64_t* req_qty;
  const int32_t* ctr_ptr;
  const uint8_t* ctr_kind;
  const int32_t* ent_ptr;
  const uint8_t* ent_slot;
  const int64_t* ent_qty;
} spx_nrt_pods_wide;

/* NetworkOverhead.  A pod's PreFilter state depends only on its (AppGroup, workload selector) "workload
 * key"; the matched (placed pod, dependency) pairs are flattened once per key. */
#define SPX_NET_ST_UNSCHEDULABLE 1 /* "Node %v does not meet several network requirements ..." networkoverhead.go:355-357 */
#define SPX_NET_RAW_COST 0
#define SPX_NET_RAW_SATISFIED 1
#define SPX_NET_RAW_VIOLATED 2
#define SPX_NET_SAME_ZONE 1   /* networkoverhead.go:60  */
#define SPX_NET_MAX_COST 100  /* networkoverhead.go:63  */

typedef struct spx_net_nodes_soa {
  int64_t n_nodes;
  const int32_t* region;
  const int32_t* zone;
} spx_net_nodes_soa;

/* region_cost [n_regions * n_regions], zone_cost [n_zones * n_zones], row = origin, -1 = no entry.  The 32-bit tables select the
 * 32-bit sweep as long as (largest entry) x (most pairs of any workload key) stays below 2^31; beyond that the engine widens them
 * and runs the 64-bit sweep (spx_kernel_path reports 2). */
typedef struct spx_net_topo_soa {
  int32_t n_regions;
  int32_t n_zones;
  const int32_t* region_cost;
  const int32_t* zone_cost;
} spx_net_topo_soa;

/* The same columns with the CRD's own int64 entries (NetworkTopology costs and MaxNetworkCost are int64): entries of any size >= -1.
 * An engine that holds these runs the 64-bit sweep: int64 accumulation and the reference's float64 NormalizeScore
 * (networkoverhead.go:389-418, :576-638).  The engine holds one width at a time: an upload of either replaces the other.  A snapshot
 * whose (largest entry) x (most pairs of any workload key) reaches 2^63 is refused by spx_eval with SPX_ERR_ARG: the reference's own
 * sum could wrap there. */
typedef struct spx_net_topo_wide {
  int32_t n_regions;
  int32_t n_zones;
  const int64_t* region_cost;
  const int64_t* zone_cost;
} spx_net_topo_wide;

typedef struct spx_net_pods_soa {
  int64_t n_pods;
  int32_t n_keys;
  const int32_t* pod_key;
  const uint8_t* key_score_equally;
  const int32_t* pair_ptr;
  const int32_t* pair_node;
  const int64_t* pair_max_cost;
  const int32_t* topo_order;
} spx_net_pods_soa;

/* TopologicalSort: the four per-pod values TopologicalSort.Less reads (topologicalsort.go:102-132): pod.Spec.Priority and
 * QueuedPodInfo.Timestamp (upstream PrioritySort, :109-113), the AppGroup id (-1 = no label) and the pod's index in its
 * group's Status.TopologyOrder as util.FindPodOrder returns it (-1 = selector not listed) — the `topo_order` column
 * spx_flatten_net_keys produces. */
typedef struct spx_sort_keys_soa {
  int64_t n_pods;
  const int32_t* priority;
  const int64_t* queue_ts;
  const int32_t* appgroup;
  const int32_t* topo_order;
} spx_sort_keys_soa;

/* NodeMetadata / PodState: one raw int64 Score per node, the same for every pod (node_metadata.go:57-73, pod_state.go:54-66).
 * NodeMetadata: raw[i] == INT64_MIN is the reference's own invalidScore (node_metadata.go:48: missing key, unparsable value) and is
 * carried as such.  PodState: terminating pods minus nominated pods of the node, |raw[i]| < 2^31. */
typedef struct spx_node_column_soa {
  int64_t n_nodes;
  const int64_t* raw;
} spx_node_column_soa;

/* NodeMetadata's MetadataType / ScoringStrategy (apis/config/types.go), for spx_flatten_nodemeta */
#define SPX_NODEMETA_NUMBER 0
#define SPX_NODEMETA_TIMESTAMP 1
#define SPX_NODEMETA_HIGHEST 0
#define SPX_NODEMETA_LOWEST 1
#define SPX_NODEMETA_NEWEST 2
#define SPX_NODEMETA_OLDEST 3

/* QOSSort: the three per-pod values Sort.Less reads (pkg/qos/queue_sort.go:46-58): pod priority, the QoS class in qosOrder's numbering
 * (:69-73: 1 BestEffort, 2 Burstable, 3 Guaranteed — spx_flatten_pod_qos) and QueuedPodInfo.Timestamp. */
#define SPX_QOSSORT_BEST_EFFORT 1
#define SPX_QOSSORT_BURSTABLE 2
#define SPX_QOSSORT_GUARANTEED 3
typedef struct spx_qos_sort_keys_soa {
  int64_t n_pods;
  const int32_t* priority;
  const uint8_t* qos;
  const int64_t* queue_ts;
} spx_qos_sort_keys_soa;

/* CapacityScheduling.PreFilter: per-pod request vectors and per-namespace nominated lists (CSR, any order) */
typedef struct spx_quota_soa {
  int64_t n_pods;
  int32_t n_namespaces;
  const int32_t* pod_ns;
  const int32_t* pod_priority;
  const int64_t* pod_req;
  const uint8_t* pod_req_present;
  const uint8_t* has_quota;
  const int64_t* used;
  const uint8_t* used_present;
  const int64_t* max;
  const uint8_t* max_present;
  const int64_t* agg_used;
  const uint8_t* agg_used_present;
  const int64_t* agg_min;
  const uint8_t* agg_min_present;
  const int64_t* other_nominated;
  const uint8_t* other_nominated_present;
  const int32_t* nom_ptr;
  const int32_t* nom_priority;
  const int64_t* nom_pending_index;
  const int64_t* nom_req;
  const uint8_t* nom_req_present;
  const int64_t* min;          /* optional (may be NULL), [NS][8] + min_present [NS]: ElasticQuotaInfo.Min per namespace.  Only the */
  const uint8_t* min_present;  /* sequential commit loop reads them (a bound pod can push its quota over min, elasticquota.go:166-191) */
} spx_quota_soa;

/* CapacityScheduling.PostFilter's preemption dry run (capacity_scheduling.go:331-348 -> preemption.Evaluator.DryRunPreemption ->
 * SelectVictimsOnNode :486-677), for many preemptors x all nodes in one launch (kernels_preempt.hip).
 * Vectors have SPX_QUOTA_SLOTS int64 slots in spx_quota_objects' layout.  The node's assigned pods are a CSR IN WALK ORDER (least
 * important first, :537-539: MoreImportantPod = priority higher, else start time earlier); pod_hi_order lists, per node, the positions
 * of that list most important first.  The reference's sort.Slice is unstable: ties in (priority, start time) are broken here by the
 * order of the table in both directions, by the flattener and by the test oracle alike.
 *   allocatable / requested [N][8]: NodeInfo.Allocatable / Requested; slot 3 = AllowedPodNumber / len(Pods).  A scalar the node does
 *     not list is 0 on both sides, which is all NodeResourcesFit reads, so the tables carry no presence mask for them.
 *   pod_fit_req [..][8]: what NodeInfo.AddPod / RemovePod charges (slot 3 = 1); pod_quota_req + pod_quota_req_present:
 *     computePodResourceRequest (:865-882), what the quota's Used moves by.
 *   pod_flags: SPX_PREEMPT_POD_IN_QUOTA_SET = the pod is in its ElasticQuotaInfo's `pods` set (deletePodIfPresent only then shrinks
 *     Used, elasticquota.go:172-187), SPX_PREEMPT_POD_TERMINATING = DeletionTimestamp set (spx_preempt_eligible reads it).
 *   pod_pdb_mask: bit k = node-local PDB k matches the pod (label selector, namespace, not in DisruptedPods: host work, :899-917);
 *     node-local PDBs keep the order of the PDB list; pdb_allowed [pdb_ptr[n] .. pdb_ptr[n+1]) their Status.DisruptionsAllowed.
 *   nom_*: pods nominated to the node (PodNominator): priority, what NodeInfo.AddPod charges, the pending row or -1.
 * NodeResourcesFit (default args), the rule that a node without victims is no candidate and pickOneNodeForPreemption restate upstream
 * kube-scheduler code that is not part of the reference tree. */
#define SPX_PREEMPT_MAX_NODE_PODS 256
#define SPX_PREEMPT_MAX_NODE_PDBS 32
#define SPX_PREEMPT_POD_IN_QUOTA_SET 1
#define SPX_PREEMPT_POD_TERMINATING 2
#define SPX_PREEMPT_ST_CANDIDATE 0     /* victims found: the cell takes part in the pick */
#define SPX_PREEMPT_ST_NO_VICTIMS 1    /* "No victims found on node ..." (UnschedulableAndUnresolvable)         :596-599 */
#define SPX_PREEMPT_ST_NOT_FIT 2       /* the Filter fails with every potential victim removed                  :607-609 */
#define SPX_PREEMPT_ST_QUOTA 3         /* "global quota max exceeded"                                           :614-619 */
#define SPX_PREEMPT_ST_ALL_REPRIEVED 4 /* success without a victim: upstream drops the node                              */
#define SPX_PREEMPT_ST_REMOVE_TWICE 5  /* nodeInfo.RemovePod of a pod already removed: the node returns an error :639, :647 */
#define SPX_PREEMPT_ST_SKIPPED 6       /* excluded by node_mask, or the node is absent                                   */
typedef struct spx_preempt_nodes_soa {
  int64_t n_nodes;
  const uint8_t* present;
  const int64_t* allocatable;
  const int64_t* requested;
  const int32_t* pod_ptr;
  const int32_t* pod_priority;
  const int64_t* pod_start;
  const int32_t* pod_ns;
  const int64_t* pod_fit_req;
  const int64_t* pod_quota_req;
  const uint8_t* pod_quota_req_present;
  const uint8_t* pod_flags;
  const uint32_t* pod_pdb_mask;
  const int32_t* pod_hi_order;
  const int32_t* nom_ptr;
  const int32_t* nom_priority;
  const int64_t* nom_fit_req;
  const int64_t* nom_pending_row;
  const int32_t* pdb_ptr;
  const int32_t* pdb_allowed;
} spx_preempt_nodes_soa;

/* per pending pod row: what NodeResourcesFit reads of the preemptor (computePodResourceRequest-style vector, slot 3 unused: a pod
 * counts once).  A scalar request of 0 and an absent one behave alike in fitsRequest, so there is no presence mask. */
typedef struct spx_preempt_pods_soa {
  int64_t n_pods;
  const int64_t* fit_req;
} spx_preempt_pods_soa;

/* what spx_flatten_preempt_nodes reads besides the node objects: the assigned pods (any order; `assigned` supplies namespace, priority
 * and containers), where and since when they run, set membership, PDB matches as indices into pdb_allowed (ascending per pod), and the
 * nominated pods.  start_ns: Status.StartTime, or the caller's "now" where it is nil (GetPodStartTime).  node_present NULL = all. */
typedef struct spx_preempt_objects {
  int64_t n_assigned;
  const spx_pod_objects* assigned;
  const int64_t* assigned_node;
  const int64_t* assigned_start_ns;
  const uint8_t* assigned_in_quota_set;
  const uint8_t* assigned_terminating;
  const int32_t* assigned_pdb_ptr;
  const int32_t* assigned_pdb;
  int32_t n_pdbs;
  const int32_t* pdb_allowed;
  int64_t n_nominated;
  const spx_pod_objects* nominated;
  const int64_t* nominated_node;
  const int64_t* nominated_pending_row;
  const uint8_t* node_present;
} spx_preempt_objects;

/* NetworkOverhead bookkeeping of the sequential commit loop: what binding pending pod p adds to the AppGroup scheduled lists the
 * later pods see.  Entries of pod p: eff_key / eff_max_cost [eff_ptr[p], eff_ptr[p+1]); eff_max_cost >= 0: workload key eff_key gains
 * the pair (p's node, that MaxNetworkCost); -1: the key merely stops scoring equally.  Built by spx_flatten_net_commit. */
typedef struct spx_net_commit_soa {
  int64_t n_pods;
  const int32_t* eff_ptr;
  const int32_t* eff_key;
  const int64_t* eff_max_cost;
} spx_net_commit_soa;

/* ------------------------------------------------------------------ engine */

/* What each entry point stands in for in the reference (sigs.k8s.io/scheduler-plugins; the Go method keeps its
 * signature and becomes an index into a fetched row — INTEGRATION.md shows the cgo side):
 *
 *   spx_eval + spx_fetch_scores(ALLOCATABLE)   Allocatable.Score + NormalizeScore      pkg/noderesources/allocatable.go:63-71, :143-168
 *   spx_fetch_raw(ALLOCATABLE)                 Allocatable.Score (raw int64)           pkg/noderesources/allocatable.go:117-140
 *   spx_eval + spx_fetch_scores(TLP)           TargetLoadPacking.Score                 pkg/trimaran/targetloadpacking/targetloadpacking.go:107-187
 *   spx_eval + spx_fetch_scores(LVRB)          LoadVariationRiskBalancing.Score        pkg/trimaran/loadvariationriskbalancing/loadvariationriskbalancing.go:84-122
 *   spx_eval + spx_fetch_scores(LROC)          LowRiskOverCommitment.PreScore + Score  pkg/trimaran/lowriskovercommitment/lowriskovercommitment.go:96-141, :158-255, beta.go:85-191
 *   spx_eval + spx_fetch_scores(PEAKS)         Peaks.Score + NormalizeScore            pkg/trimaran/peaks/peaks.go:103-144, :150-166, :186-188
 *   spx_fetch_raw(PEAKS)                       Peaks.Score (raw int64: power jump x 1e15)
 *   spx_eval + spx_fetch_scores(SYSCHED)       SySched.Score + NormalizeScore          pkg/sysched/sysched.go:234-279, :281-288
 *   spx_fetch_raw(SYSCHED)                     SySched.Score (raw int64; math.MaxInt64 for a pod with the empty set, :249-251)
 *   spx_eval + spx_fetch_scores(NODEMETA)      NodeMetadata.Score + NormalizeScore     pkg/nodemetadata/node_metadata.go:57-73, :150-210
 *   spx_fetch_raw(NODEMETA)                    NodeMetadata.Score (raw int64; math.MinInt64 = invalidScore, :48)   node_metadata.go:80-145
 *   spx_eval + spx_fetch_scores(PODSTATE)      PodState.Score + NormalizeScore         pkg/podstate/pod_state.go:42-64, :66-91
 *   spx_fetch_raw(PODSTATE)                    PodState.score (terminating - nominated pods of the node)           pod_state.go:52-64
 *   spx_eval + spx_fetch_status(NRT)           TopologyMatch.Filter                    pkg/noderesourcetopology/filter.go:179-245
 *   spx_eval + spx_fetch_scores(NRT)           TopologyMatch.Score                     pkg/noderesourcetopology/score.go:62-102
 *   spx_eval + spx_fetch_status(NETOVERHEAD)   NetworkOverhead.PreFilter + Filter      pkg/networkaware/networkoverhead/networkoverhead.go:174-298, :326-359
 *   spx_fetch_raw(NETOVERHEAD, cost/sat/vio)   NetworkOverhead.Score, PreFilterState   networkoverhead.go:362-386, :85-115
 *   spx_eval + spx_fetch_scores(NETOVERHEAD)   NetworkOverhead.NormalizeScore          networkoverhead.go:389-418
 *   spx_eval + spx_fetch_prefilter(CAPACITY)   CapacityScheduling.PreFilter            pkg/capacityscheduling/capacity_scheduling.go:208-283
 *   spx_eval + spx_fetch_prefilter(COSCHED)    PodGroupManager.PreFilter               pkg/coscheduling/core/core.go:243-305
 *   spx_fetch_cosched_gap                      CheckClusterResource, getNodeResource   core.go:406-426, :433-467 (the "resource gap" of the error text)
 *   spx_cosched_less                           Coscheduling.Less, GetCreationTimestamp pkg/coscheduling/coscheduling.go:133-145, core.go:368-384
 *   spx_flatten_net_keys + spx_toposort_less   TopologicalSort.Less, FindPodOrder      pkg/networkaware/topologicalsort/topologicalsort.go:102-132, util/util.go:138-153
 *   spx_upload_sort_keys + spx_sort_keys       the activeQ ordering TopologicalSort.Less induces, as one device sort
 *   spx_flatten_pod_qos + spx_qos_less         QOSSort.Less, compQOS                   pkg/qos/queue_sort.go:46-58, :65-82
 *   spx_upload_qos_sort_keys + spx_qos_sort    the activeQ ordering QOSSort.Less induces, as one device sort
 *   spx_flatten_nodemeta / _nodemeta_unix      calculateScore, parseNumericValue, parseTimestampValue              node_metadata.go:80-145
 *   spx_flatten_podstate                       PodState.score's two counts per node    pod_state.go:52-64
 *   spx_flatten_trimaran_*                     GetNodeMetrics / ScheduledPodsCache / PredictUtilisation / GetResourceRequested
 *                                              pkg/trimaran/collector.go:110-123, handler.go:47-58, targetloadpacking.go:198-205, resourcestats.go:45-146
 *   spx_flatten_nrt_*                          createNUMANodeList / TopologyManagerFromNodeResourceTopology / GetPodEffectiveRequest / OverReserve
 *                                              pkg/noderesourcetopology/pluginhelpers.go:105-173, nodeconfig/topologymanager.go:78-162, pkg/util/resource.go:51-85, cache/store.go:315-356
 *   spx_flatten_net_topo                       populateCostMap                         networkoverhead.go:448-497
 *   spx_flatten_quota                          ElasticQuotaInfos (used / min / max, nominated pods)   pkg/capacityscheduling/elasticquota.go:48-123
 *   spx_preempt_dry_run + spx_fetch_preempt_*  CapacityScheduling.PostFilter: SelectVictimsOnNode per (pod, node), pickOneNodeForPreemption
 *                                              capacity_scheduling.go:331-348, :486-677, :889-934
 *   spx_preempt_eligible                       preemptor.PodEligibleToPreemptOthers    capacity_scheduling.go:409-484
 *   spx_preempt_sequential                     CapacityScheduling.PostFilter repeated over a batch, each pod against what the earlier ones
 *                                              evicted, nominated and took out of their quotas' Used (deletePodIfPresent :778-792)
 *   spx_eval_best + spx_fetch_best             upstream prioritizeNodes + selectHost input (sum of weight x score over feasible nodes)
 *   spx_decide + spx_fetch_best                the same decision input without materialising the per-plugin tables
 *   spx_commit_sequential                      upstream scheduleOne repeated over the queue, with trimaran's bind-time bookkeeping
 *                                              pkg/trimaran/handler.go:131-139, targetloadpacking.go:151-168
 */

typedef struct spx_engine spx_engine;

/* create an engine on HIP device `device_id`; fails with SPX_ERR_NOGPU when no device exists
 * (there is no CPU fallback by design) */
int spx_create(int device_id, spx_engine** out);
int spx_destroy(spx_engine* e);
/* last error text: of engine `e`, or of the failed spx_create when e == NULL (thread-local) */
const char* spx_last_error(const spx_engine* e);
/* number of entry points this build exports, and the ABI version */
int spx_abi_version(void);
/* run on an externally owned hipStream_t (e.g. torch's current stream); NULL = engine's own */
int spx_set_stream(spx_engine* e, void* hip_stream);
/* the stream kernels are launched on (for HIP-event timing by the caller) */
int spx_get_stream(spx_engine* e, void** hip_stream);

int spx_set_allocatable_params(spx_engine* e, const spx_allocatable_params* p);
int spx_set_tlp_params(spx_engine* e, const spx_tlp_params* p);
int spx_set_lvrb_params(spx_engine* e, const spx_lvrb_params* p);

int spx_set_nrt_params(spx_engine* e, const spx_nrt_params* p);
int spx_set_lroc_params(spx_engine* e, const spx_lroc_params* p);

int spx_upload_alloc_nodes(spx_engine* e, const spx_alloc_nodes_soa* t);
int spx_upload_trimaran_nodes(spx_engine* e, const spx_trimaran_nodes_soa* t);
int spx_upload_trimaran_pods(spx_engine* e, const spx_trimaran_pods_soa* t);
/* LowRiskOverCommitment tables; the node table needs spx_upload_trimaran_nodes first (same node count) */
int spx_upload_lroc_nodes(spx_engine* e, const spx_lroc_nodes_soa* t);
int spx_upload_lroc_pods(spx_engine* e, const spx_lroc_pods_soa* t);
int spx_upload_peaks_nodes(spx_engine* e, const spx_peaks_nodes_soa* t);
int spx_upload_peaks_pods(spx_engine* e, const spx_peaks_pods_soa* t);
/* SySched tables (spx_flatten_sysched_*).  SPX_ERR_ARG: n_words outside [1, SPX_SYSCHED_MAX_WORDS], a set id out of range, a node
 * whose largest possible score reaches SPX_SYSCHED_MAX_SCORE, a stale bit outside the names */
int spx_upload_sysched_nodes(spx_engine* e, const spx_sysched_nodes_soa* t);
int spx_upload_sysched_pods(spx_engine* e, const spx_sysched_pods_soa* t);
/* NodeMetadata's and PodState's node columns (spx_flatten_nodemeta, spx_flatten_podstate).  n_nodes must equal the engine's node count
 * once that is known, as for every node table.  There is no row delta: a column is n_nodes x 8 bytes, upload it again.  An upload
 * clears the plugin's "evaluated" state.  now_unused is reserved (the flattener takes "now"; the column holds finished scores) and
 * must be 0.  spx_upload_podstate_nodes: SPX_ERR_ARG for a value with |raw| >= 2^31 (these are pod counts; the refusal keeps
 * `highest = -math.MaxInt64`, pod_state.go:68, out of play).  Neither plugin is carried by spx_commit_sequential or the spx_multi
 * loaders. */
int spx_upload_nodemeta_nodes(spx_engine* e, const spx_node_column_soa* t, int64_t now_unused);
int spx_upload_podstate_nodes(spx_engine* e, const spx_node_column_soa* t);
/* Coscheduling tables (spx_flatten_cosched_*).  SPX_ERR_ARG: more than SPX_COSCHED_MAX_SLOTS slots, a group / node index out of range,
 * steps that are not strictly ascending present nodes, a negative add-back, or a table spx_cosched_check refuses (the text names the
 * slot).  Every upload marks the gate stale: the next spx_eval with the COSCHED bit scans and gates again. */
int spx_upload_cosched(spx_engine* e, const spx_cosched_soa* t);
/* the limits of the device's int64 sums (the reference falls into inf.Dec there): SPX_ERR_ARG and *bad_slot = the first slot whose
 * sum_i |left_base| + (all add-backs) reaches 2^62, or that holds a request with |req| >= 2^62; SPX_OK and -1 otherwise.  Host only. */
int spx_cosched_check(const spx_cosched_soa* t, int32_t* bad_slot);
/* Snapshot deltas (SURVEY 8d "upload deltas"): `t` holds t->n_nodes ROWS in the layout of the full upload; row i replaces node
 * idx[i] of the table already on the device (spx_upload_* must have run once: it fixes the shape).  The changed rows travel as one
 * staged blob and are scattered into the device columns; for NRT the float64 formulation's derived columns are recomputed on the
 * device for those nodes (bit-identical to a full re-upload).  Every table evaluated from the old rows becomes stale.
 *   trimaran: collector refresh of a node's metrics (collector.go:139-150), the bind-time cache (handler.go:131-139)
 *   NRT: a republished NodeResourceTopology (pluginhelpers.go:105-161), an assumed pod charged to a node (overreserve.go:170-203) */
int spx_update_trimaran_nodes(spx_engine* e, const int64_t* idx, const spx_trimaran_nodes_soa* t);
int spx_update_nrt_nodes(spx_engine* e, const int64_t* idx, const spx_nrt_nodes_soa* t);
/* SySched: a bind or a delete changes one node's cached host set, resident count, a and stale list (sysched.go:310-366 addPod /
 * removePod); `t` holds t->n_nodes rows in the layout of the full upload (host_bits [n_words][t->n_nodes], stale_ptr over the rows) */
int spx_update_sysched_nodes(spx_engine* e, const int64_t* idx, const spx_sysched_nodes_soa* t);
/* NetworkOverhead: pairs appended to the workload keys' lists (AppGroup scheduled lists grow between cycles, networkoverhead.go:654-694).
 * Entry i: key[i] gains (node[i], max_cost[i]); max_cost[i] == -1: the key merely stops scoring equally.  Built by spx_flatten_net_placed.
 * Equal to re-uploading spx_flatten_net_keys' tables of the grown AppGroups (tests/test_gpu_delta.py). */
int spx_update_net_placed(spx_engine* e, int64_t n, const int32_t* key, const int32_t* node, const int64_t* max_cost);
/* CapacityScheduling: rows of ElasticQuotaInfo.Used replaced (AddPod / DeletePod events, capacity_scheduling.go:679-803): namespace ns[i]
 * takes used[i][SPX_QUOTA_SLOTS] / used_present[i]; agg_used[SPX_QUOTA_SLOTS] / *agg_used_present: the new aggregate over all quotas. */
int spx_update_quota_used(spx_engine* e, int64_t n_rows, const int32_t* ns, const int64_t* used, const uint8_t* used_present, const int64_t* agg_used, const uint8_t* agg_used_present);
int spx_upload_nrt_slots(spx_engine* e, const spx_nrt_slots* t);
int spx_upload_nrt_nodes(spx_engine* e, const spx_nrt_nodes_soa* t);
int spx_upload_nrt_pods(spx_engine* e, const spx_nrt_pods_soa* t);
/* the containers of the batch's long rows (after spx_upload_nrt_pods; t->pod_row must list exactly the rows whose n_ctr is
 * SPX_NRT_CTRS_LONG, else SPX_ERR_ARG).  An NRT spx_eval / spx_decide / spx_commit_sequential of a batch with long rows and no table
 * fails with SPX_ERR_STATE; a table with n_long = 0 for a batch without long rows is accepted (and clears the table). */
int spx_upload_nrt_long_pods(spx_engine* e, const spx_nrt_long_pods* t);
/* *n_out = long rows the last NodeResourceTopologyMatch sweep of spx_eval evaluated (those inside its row range; 0 = none / no sweep yet) */
int spx_nrt_long_rows(const spx_engine* e, int64_t* n_out);
/* the zones of the node table's tall nodes (after spx_upload_nrt_nodes; t->node_idx must list exactly the rows whose n_zones is
 * SPX_NRT_ZONES_TALL, else SPX_ERR_ARG; a table with n_tall = 0 for a node table without tall nodes is accepted).  Until it arrives an
 * NRT spx_eval / spx_decide / spx_fetch_raw fails with SPX_ERR_STATE.  A later spx_upload_nrt_nodes or slot upload drops it.  With
 * tall nodes in place spx_commit_sequential with NodeResourceTopologyMatch and spx_update_nrt_nodes fail with SPX_ERR_STATE, and an
 * evaluation with LeastNUMANodes fails with SPX_ERR_STATE when a tall node lists more than SPX_NRT_TALL_MAX_ZONES_LEAST_NUMA zones. */
int spx_upload_nrt_tall_nodes(spx_engine* e, const spx_nrt_tall_nodes* t);
/* *n_out = tall nodes the last NodeResourceTopologyMatch sweep of spx_eval evaluated (0 = none / no sweep yet / an empty row range) */
int spx_nrt_tall_count(const spx_engine* e, int64_t* n_out);
/* The wide NRT tables (up to SPX_NRT_MAX_RES_WIDE slots), evaluated by kernels_nrt_wide.hip; order: slots, nodes, pods.  The wide
 * slot table replaces the dense NRT tables (and a later spx_upload_nrt_slots the wide ones): an engine holds one form at a time.
 * On a wide engine spx_commit_sequential with NodeResourceTopologyMatch and spx_update_nrt_nodes fail with SPX_ERR_STATE. */
int spx_upload_nrt_slots_wide(spx_engine* e, const spx_nrt_slots* t);
int spx_upload_nrt_nodes_wide(spx_engine* e, const spx_nrt_nodes_wide* t);
int spx_upload_nrt_pods_wide(spx_engine* e, const spx_nrt_pods_wide* t);
/* 1 = the NRT tables in place are the wide form, 0 = dense (or none) */
int spx_nrt_wide(const spx_engine* e);
int spx_upload_net_nodes(spx_engine* e, const spx_net_nodes_soa* t);
int spx_upload_net_topo(spx_engine* e, const spx_net_topo_soa* t);
/* the int64 cost matrices (spx_flatten_net_topo_wide); replaces the 32-bit ones, as a later spx_upload_net_topo replaces these */
int spx_upload_net_topo_wide(spx_engine* e, const spx_net_topo_wide* t);
int spx_upload_net_pods(spx_engine* e, const spx_net_pods_soa* t);
int spx_upload_quota(spx_engine* e, const spx_quota_soa* t);
/* after spx_upload_net_pods; only spx_commit_sequential with NETOVERHEAD in its mask needs it */
int spx_upload_net_commit(spx_engine* e, const spx_net_commit_soa* t);
/* TopologicalSort as one batched sort of the pending queue (replaces the activeQ heap's pairwise Less calls).  Less is not a
 * strict weak order (same AppGroup: `orderP1 <= orderP2`; otherwise PrioritySort), but it is complete, so an order exists in
 * which EVERY ADJACENT PAIR (x, y) satisfies Less(x, y) — or ties under PrioritySort (equal priority and timestamp).
 * spx_sort_keys returns such an order: perm_out[i] = pod row at queue position i.  Construction (kernels_sort.hip): stable
 * radix sort by (priority descending, timestamp ascending), then every maximal run of consecutive pods of one AppGroup is
 * reordered by topology index.  The table is independent of the other pod tables (its n_pods is the queue length).
 * Synchronous; spx_last_eval_ms reports the device time. */
int spx_upload_sort_keys(spx_engine* e, const spx_sort_keys_soa* t);
int spx_sort_keys(spx_engine* e, int32_t* perm_out);
/* QOSSort as one batched sort of the pending queue.  Sort.Less (queue_sort.go:46-58) is a strict weak order: priority descending, QoS
 * class descending (Guaranteed, Burstable, BestEffort), timestamp ascending.  spx_qos_sort returns perm_out[i] = pod row at queue
 * position i; rows equal in all three keys keep ascending row order.  Construction: kernels_sort.hip's stable radix passes, twice
 * (class and timestamp, then priority and the first order's rank), around the key-building kernels of kernels_node_columns.hip.
 * Independent of spx_upload_sort_keys / spx_sort_keys (whose keys it leaves alone) and of the other pod tables.  SPX_ERR_ARG: n_pods
 * outside [1, 2^31), a class outside 1..3.  Synchronous; spx_last_eval_ms reports the device time. */
int spx_upload_qos_sort_keys(spx_engine* e, const spx_qos_sort_keys_soa* t);
int spx_qos_sort(spx_engine* e, int32_t* perm_out);
/* CapacityScheduling.PreFilter status per pod (n_pods bytes: 0 Success, SPX_QUOTA_ST_*); valid after spx_eval with the CAPACITY bit */
int spx_fetch_prefilter(spx_engine* e, int plugin, int64_t row_begin, int64_t row_end, uint8_t* out);
/* with plugin == SPX_PLUGIN_COSCHED the same call returns PodGroupManager.PreFilter's status per pod (0 Success, SPX_COSCHED_ST_*),
 * valid after spx_eval with the COSCHED bit.  With that bit in the mask of spx_eval_best or spx_decide, a pod whose gate failed
 * reads back through spx_fetch_best as node -1 / score 0 / 0 ties / 0 feasible, as a pod failing CapacityScheduling's does.
 * spx_fetch_cosched_gap: CheckClusterResource per group [group_begin, group_end) of the last evaluation, whatever permittedPG says:
 * pass_mask bit s = named slot s closed, open_mask bit s = named slot s still open after the last node, gap [groups][n_slots] =
 * req - S_g[last present node] for an open slot (what the reference's "resource gap" lists), 0 otherwise. */
int spx_fetch_cosched_gap(spx_engine* e, int32_t group_begin, int32_t group_end, uint32_t* pass_mask, uint32_t* open_mask, int64_t* gap);

/* The preemption dry run.  Tables: spx_upload_quota WITH min (namespace, priority, quota request and the nominated sums of a
 * preemptor are formed exactly as CapacityScheduling.PreFilter's: a snapshot without quotas is a table whose has_quota is all 0),
 * spx_upload_preempt_nodes, spx_upload_preempt_pods.  Every one of these uploads (and spx_update_quota_used) marks earlier results stale.
 * SPX_ERR_ARG, the text naming the node: more than SPX_PREEMPT_MAX_NODE_PODS pods or SPX_PREEMPT_MAX_NODE_PDBS PDBs on a node, a
 * negative request or allocatable, a slot whose absolute values sum to 2^62 or more (device sums are int64), a list that is not in walk
 * order, a pod_hi_order that is no permutation, a PDB bit outside the node's PDBs.
 * spx_preempt_dry_run: rows[n_rows] are pod rows of the uploaded batch (any order, gaps allowed, no duplicates needed); node_mask
 * [n_rows][n_nodes], NULL = all, 0 = the Filter status of that node was UnschedulableAndUnresolvable (upstream's
 * nodesWherePreemptionMightHelp).  All preemptors see the same frozen snapshot and every (preemptor, node) cell starts from a fresh copy
 * of the node and of the ElasticQuotaInfos, as the reference's per-node clone does.  Asynchronous on the engine stream;
 * spx_last_eval_ms reports its device time.  The call holds 32 bytes per cell (n_rows rounded up to 64, times n_nodes) plus 320 bytes
 * per row; a row list whose records do not fit the device's free memory is refused with SPX_ERR_ARG before anything is allocated.
 * SPX_ERR_STATE without the quota tables (with min) or the preempt tables.
 * spx_fetch_preempt_cells / _pick address the rows by their index i in the row list of the last dry run: status u8, n_victims and
 * n_violations int32 [i_end - i_begin][n_nodes] (each may be NULL); pick: node (-1 = no candidate), the picked cell's n_victims and
 * n_violations, the number of CANDIDATE cells, and the size of the final tie set (upstream takes "the first" of an unordered map; the
 * lowest node index of the set is returned).  Order of pickOneNodeForPreemption: fewest violations, lowest highest-victim priority,
 * smallest sum of (priority + 2^31), fewest victims, latest earliest-start-time among the highest-priority victims.
 * spx_fetch_preempt_victims recomputes one cell and returns the victims as positions in the node's list, most important first
 * (:672-675); *n_out is written even when it exceeds cap (SPX_ERR_ARG then).  *status_out (may be NULL) = the cell's status. */
int spx_upload_preempt_nodes(spx_engine* e, const spx_preempt_nodes_soa* t);
int spx_upload_preempt_pods(spx_engine* e, const spx_preempt_pods_soa* t);
int spx_preempt_dry_run(spx_engine* e, const int64_t* rows, int64_t n_rows, const uint8_t* node_mask);
int spx_fetch_preempt_cells(spx_engine* e, int64_t i_begin, int64_t i_end, uint8_t* status, int32_t* n_victims, int32_t* n_violations);
/* the keys pickOneNodeForPreemption compares, per cell [i_end - i_begin][n_nodes] (each may be NULL; 0 where the cell is no CANDIDATE): the
 * highest victim priority, the sum of (priority + 2^31) over the victims, the earliest start time among the victims of that priority */
int spx_fetch_preempt_keys(spx_engine* e, int64_t i_begin, int64_t i_end, int32_t* hi_priority, int64_t* priority_sum, int64_t* start);
int spx_fetch_preempt_pick(spx_engine* e, int64_t i_begin, int64_t i_end, int32_t* node, int32_t* n_victims, int32_t* n_violations, int32_t* n_candidates, int32_t* n_ties);
int spx_fetch_preempt_victims(spx_engine* e, int64_t i, int64_t node, int32_t* pod_pos_out, int32_t cap, int32_t* n_out, int32_t* status_out);

/* PreemptionToleration.PostFilter's dry run (pkg/preemptiontoleration/preemption_toleration.go:188-299; kernels_ptol.hip, DESIGN.md
 * 3.9d): DefaultPreemption's SelectVictimsOnNode with one more predicate per (preemptor, lower-priority pod) pair,
 * ExemptedFromPreemption (:129-181), decided by the annotations of the pod's PriorityClass (preemption_toleration_policy.go).  There
 * are no quotas: the call needs the node and pod tables of spx_upload_preempt_nodes / _pods and the side table below, nothing else.
 * spx_preempt_toleration_soa: one entry per assigned pod in the order of spx_preempt_nodes_soa's pod CSR (n_pods == pod_ptr[N]):
 *   flags            SPX_PTOL_POD_HAS_CLASS = PriorityClassName is set and the class exists; SPX_PTOL_POD_CLASS_MISSING = it is set and
 *                    the lister does not have it (:139-142, an error: the node ends with it); neither = the name is empty (:136)
 *   min_preemptable  Policy.MinimumPreemptablePriority; INT32_MIN for a policy that does not parse (:153-162: no toleration at all,
 *                    but a PreemptNever preemptor was answered before the parse, :148-150, which HAS_CLASS still carries)
 *   exempt_until_ns  the pod is exempted from a preemptor of priority < min_preemptable while exempt_until_ns > now (strict, :180):
 *                    INT64_MAX for TolerationSeconds < 0 (:168) or a pod without a PodScheduled=True condition (:173-176), else
 *                    scheduledAt + time.Duration(TolerationSeconds) * time.Second with the product wrapped to int64 as Go wraps it
 *                    and the sum clamped to int64 (Time.Add does not wrap).  spx_flatten_preempt_toleration forms all three.
 * A pod of priority < the preemptor's is a potential victim unless it is exempted; if any such pod's class is missing the cell's status
 * is SPX_PREEMPT_ST_CLASS_ERROR, whatever else holds.  NO_VICTIMS, NOT_FIT, ALL_REPRIEVED, CANDIDATE, SKIPPED, the five keys and the
 * pick are spx_preempt_dry_run's; QUOTA and REMOVE_TWICE cannot occur.
 * spx_upload_preempt_toleration: SPX_ERR_STATE before spx_upload_preempt_nodes; SPX_ERR_ARG when n_pods differs from the node table's
 * pod count or an entry has both flags.  It marks earlier results stale; a later spx_upload_preempt_nodes drops the table.
 * spx_preempt_toleration_dry_run: rows / node_mask as in spx_preempt_dry_run; priority / preempt_never [n_rows] are the preemptors'
 * PodPriority and PreemptionPolicy == Never, per entry of rows; now_ns = the plugin's curTime, INT64_MAX is refused (SPX_ERR_ARG: an
 * exempt_until_ns of INT64_MAX means "for ever").  No quota upload is needed.  Memory: 32 bytes per cell plus 80 bytes per row, checked
 * against the device's free memory first; at most 2^24 rows; spx_last_eval_ms reports its device time.
 * spx_fetch_preempt_cells / _keys / _pick / _victims answer for whichever of the two dry runs ran last. */
#define SPX_PREEMPT_ST_CLASS_ERROR 7   /* a lower-priority pod names a PriorityClass that does not exist           ptol :139-142, :225-228 */
#define SPX_PTOL_POD_HAS_CLASS 1
#define SPX_PTOL_POD_CLASS_MISSING 2
typedef struct spx_preempt_toleration_soa {
  int64_t n_pods;
  const int32_t* min_preemptable;
  const int64_t* exempt_until_ns;
  const uint8_t* flags;
} spx_preempt_toleration_soa;
int spx_upload_preempt_toleration(spx_engine* e, const spx_preempt_toleration_soa* t);
int spx_preempt_toleration_dry_run(spx_engine* e, const int64_t* rows, int64_t n_rows, const int32_t* priority, const uint8_t* preempt_never, int64_t now_ns, const uint8_t* node_mask);

/* PreemptionToleration's sequential preemption loop (kernels_ptol_seq.hip).  Tables, argument checks, limits, the memory
 * pre-check and staleness are spx_preempt_toleration_dry_run's; in addition a pod row listed twice is SPX_ERR_ARG.  With an all-zero
 * flags column in spx_preempt_toleration_soa this is upstream's DefaultPreemption.
 * The rows are attempted once each, in list order.  Step i evaluates rows[i] on every unmasked node (the dry run's SelectVictimsOnNode
 * and pick) against the state that steps 0..i-1 left, then moves the state to the scheduler's cache as it is once the events of the
 * step have been observed (restated from upstream kube-scheduler, unpinned by a reference test):
 *   T1  the victims of the picked cell leave the picked node n: Requested and the pod count shrink, nobody walks them again (NodeInfo.RemovePod)
 *   T2  rows[i] becomes a pod nominated to n, with its priority and its fit_req; later preemptors charge it by the existing rule
 *       (nominated priority >= the preemptor's)
 *   T3  nominated pods of n with a priority BELOW rows[i]'s lose their nomination, uploaded ones and rows nominated earlier in the loop
 *       alike (prepareCandidate / getLowerPriorityNominatedPods)
 *   T4  every uploaded nomination of rows[i] itself (nom_pending_row == rows[i], on any node) is dropped: the nominator moves it when a
 *       node was picked; without a candidate upstream returns an empty nominated node, which clears it
 * Two kinds of row change nothing.  preempt_never[i]: upstream never lets such a pod into PostFilter's preemption; its cells, pick and
 * victims are what spx_preempt_toleration_dry_run gives for it, on the uploaded state, whatever the rows before it did.  eligible[i] == 0
 * (NULL = all eligible): the row is evaluated at its own step like any other, its pick is reported and not applied.
 * PDB DisruptionsAllowed stays as uploaded at every step: it is the disruption controller's status, not the scheduler's.  A row whose
 * nomination T3 cleared is not attempted again.  The uploaded tables are left unchanged: a spx_preempt_toleration_dry_run or
 * spx_preempt_dry_run after the loop gives what it gave before it.
 * Asynchronous on the engine stream and without a host round trip between steps; spx_last_eval_ms reports the device time of the whole
 * loop.  Memory beyond the dry run's: 100 bytes per node, 37 bytes per row, one byte per nominated record and 4 bytes per row and
 * dirty slot (1 + the most uploaded nominations any one listed row has).
 * The fetches answer for the loop until the next dry run of either kind: spx_fetch_preempt_pick gives row i's pick at its own step;
 * spx_fetch_preempt_cells / _keys give row i's cells as it saw them at its own step (a step re-evaluates only the rows after it, so
 * row i's cells are never rewritten after step i); spx_fetch_preempt_victims(i, node) answers for node == row i's picked node from the
 * victim set stored at the step, as positions in the UPLOADED list of the node, most important first, and is SPX_ERR_ARG for any other
 * node (the state that cell saw is gone). */
int spx_preempt_toleration_sequential(spx_engine* e, const int64_t* rows, int64_t n_rows, const int32_t* priority, const uint8_t* preempt_never, const uint8_t* eligible, int64_t now_ns, const uint8_t* node_mask);

/* PreemptionToleration's dry run with NodeResourceTopologyMatch's single-NUMA Filter in the refit (kernels_ptol_nrt.hip, DESIGN.md
 * 3.9g).  SelectVictimsOnNode runs every Filter through RunFilterPluginsWithNominatedPods; NRT's sees the pods removed so far as its
 * preemption stack (prefilter.go:66-102), simulates their eviction on the node's zone table (filter.go:205-220, preemption.go:39-157)
 * and runs the single-NUMA handler on the result.  The refit of the walk becomes NodeResourcesFit-with-nominated && F; everything else is
 * spx_preempt_toleration_dry_run's, and a failing F is SPX_PREEMPT_ST_NOT_FIT.  F(p, n, stack), in this order: p BestEffort without a
 * non-native request: pass; the node's NRT not fresh: fail; no NRT: pass; with preemption_mode, a non-empty stack and placement info
 * that holds containers the simulation runs: no contributing pod on the stack: fail, a zone's available + releases above its
 * allocatable: fail; then a policy other than single-numa-node: pass; else the pod-scope or container-scope handler on available +
 * releases.  preemption_mode == 0 (prefilter.go:52): the stack is never kept and F is the ordinary Filter on the live table.  NRT
 * ignores nominated pods.  The NodeMaybeOverReserved mark of a failing Filter outside the preemption flow is control-plane state and is
 * not modelled.
 * spx_preempt_nrt_soa is a side table of the preemption tables, indexed by their node index, their assigned-pod CSR order and their
 * pod rows; it does not read spx_upload_nrt_*'s tables.  Host row-major:
 *   slots            the NRT slot table, n_res <= SPX_NRT_MAX_RES
 *   node_flags [N]   SPX_NRT_F_* | SPX_PNRT_F_PLACEMENT (placement info present and Containers() != 0)
 *   n_zones [N], zone_id [N][8], zone_present [N][8] (bit = slot), node_present [N]: as spx_nrt_nodes_soa's columns
 *   zone_avail / zone_headroom [N][8][n_res]: available, and allocatable - available (>= 0)
 *   pod_contributes [n_assigned]: the pod, once on the stack, gives the simulation something to add (whether or not the node has the
 *                    zone or the resource); rel_ptr [n_assigned + 1], rel_zone / rel_slot / rel_qty: its releases mapped to the node's
 *                    zone list (position, slot, quantity > 0; zero quantities are dropped: with available <= allocatable they cannot fail)
 *   pods             the preemptors' NRT records, one per pod row of spx_upload_preempt_pods (n_pods equal, n_res the slots')
 * spx_upload_preempt_nrt: SPX_ERR_STATE before spx_upload_preempt_nodes / spx_upload_preempt_pods; SPX_ERR_ARG, naming the node or pod,
 * for a size that differs from theirs, more than 8 slots, zones or containers of a preemptor (wide tables and long rows are declined),
 * negative headroom (a zone with available > allocatable: malformed, a documented limit), a release that is negative, outside the
 * node's zones or slots, or a node whose releases sum to 2^62 or more in a slot.  It marks earlier results stale; a later
 * spx_upload_preempt_nodes or spx_upload_preempt_pods drops the table.
 * spx_preempt_toleration_nrt_dry_run: the arguments of spx_preempt_toleration_dry_run and preemption_mode; SPX_ERR_STATE without the
 * toleration table or this side table.  The spx_fetch_preempt_* calls answer for it while it is the last run; the victims fetch
 * recomputes the cell with the same kernel. */
#define SPX_PNRT_F_PLACEMENT 16
typedef struct spx_preempt_nrt_soa {
  int64_t n_nodes;
  const spx_nrt_slots* slots;
  const uint8_t* node_flags;
  const uint8_t* n_zones;
  const uint8_t* zone_id;
  const uint8_t* zone_present;
  const uint8_t* node_present;
  const int64_t* zone_avail;
  const int64_t* zone_headroom;
  int64_t n_assigned;
  const uint8_t* pod_contributes;
  const int32_t* rel_ptr;
  const uint8_t* rel_zone;
  const uint8_t* rel_slot;
  const int64_t* rel_qty;
  const spx_nrt_pods_soa* pods;
} spx_preempt_nrt_soa;
int spx_upload_preempt_nrt(spx_engine* e, const spx_preempt_nrt_soa* t);
int spx_preempt_toleration_nrt_dry_run(spx_engine* e, const int64_t* rows, int64_t n_rows, const int32_t* priority, const uint8_t* preempt_never, int64_t now_ns, const uint8_t* node_mask, int32_t preemption_mode);

/* CapacityScheduling's dry run with the same Filter in the refit (kernels_preempt_nrt.hip).  Its SelectVictimsOnNode
 * makes the same calls: removePod (capacity_scheduling.go:513) and addPod (:523) run the PreFilter extensions that push and pop NRT's
 * preemption stack, and both Filter runs (:607 after the potential victims are gone, :636 inside reprievePod) run NRT's Filter on it.
 * The refit of the walk becomes NodeResourcesFit-with-nominated && F, with F exactly as stated above for
 * spx_preempt_toleration_nrt_dry_run (the same six steps in the same order; NRT ignores nominated pods); everything else is
 * spx_preempt_dry_run's.  A failing F is SPX_PREEMPT_ST_NOT_FIT; no new status.  The order of :596-619 is kept: SPX_PREEMPT_ST_NO_VICTIMS,
 * then the refit (SPX_PREEMPT_ST_NOT_FIT), then the quota test (SPX_PREEMPT_ST_QUOTA): a cell the reference ends at :607 is never reported
 * as QUOTA.  A pod that fits but is removed again for the quota (:646-649) goes back onto NRT's stack, and every later reprieve's F
 * sees it there.  The borrowed marks (:572) depend on no Filter.
 * Arguments, argument checks, limits, the memory pre-check and staleness are spx_preempt_dry_run's, plus preemption_mode as in
 * spx_preempt_toleration_nrt_dry_run and at most 65 535 x 64 rows per call (SPX_ERR_ARG beyond).  SPX_ERR_STATE without the quota tables
 * (with min), without spx_upload_preempt_nodes / spx_upload_preempt_pods, or without the side table of spx_upload_preempt_nrt (which a
 * later spx_upload_preempt_nodes or spx_upload_preempt_pods drops); the toleration table is not needed.  Every upload of a preemption
 * table marks the results stale.  The spx_fetch_preempt_* calls answer for it while it is the last run; the victims fetch recomputes
 * the cell with the same kernel. */
int spx_preempt_nrt_dry_run(spx_engine* e, const int64_t* rows, int64_t n_rows, const uint8_t* node_mask, int32_t preemption_mode);

/* PreemptionToleration's sequential preemption loop with the same Filter in the refit (kernels_ptol_nrt_seq.hip).  The
 * contract is spx_preempt_toleration_sequential's in full (T1-T4, preempt_never, eligible, rows listed once, PDB budgets as uploaded,
 * results through the same fetches, spx_fetch_preempt_victims(i, node) for the picked node only) with the refit of
 * spx_preempt_toleration_nrt_dry_run: NodeResourcesFit-with-nominated && F.  One more rule:
 *   T5  the zone table, the placement info and the per-pod releases of spx_preempt_nrt_soa stay as uploaded at every step.  A pod that
 *       left at an earlier step contributes no release and is not counted in the stack size or the contributing count: it is gone from
 *       NodeInfo, nobody calls RemovePod for it again, so it is never on NRT's preemption stack again.  NRT ignores nominated pods, so T2
 *       and T3 do not touch F.  Unlike T1-T4 this is pinned by reference source: NRT's caches have no pod-delete path
 *       (pkg/noderesourcetopology/cache/passthrough.go, discardreserved.go, overreserve.go change on an NRT update, a Reserve / Unreserve
 *       or a resync only), so between two PostFilter calls of one batch the zone table is what the node agent last reported.
 * A preempt_never row is answered on the uploaded state with F: what spx_preempt_toleration_nrt_dry_run writes for it, bit for bit.
 * With preemption_mode == 0, F is the ordinary Filter on the live table at every step.
 * Argument checks, limits, the memory pre-check (which counts the NRT row record of 75 int64 per row as well) and staleness are the
 * union of the two: SPX_ERR_STATE without spx_upload_preempt_nodes / _pods, the toleration table or the side table of
 * spx_upload_preempt_nrt (which a later spx_upload_preempt_nodes or spx_upload_preempt_pods drops); SPX_ERR_ARG for an empty list, a row
 * outside the batch or listed twice, now_ns == INT64_MAX, or more than 65 535 x 64 rows.  The uploaded tables are never written: either
 * dry run and spx_preempt_toleration_sequential give after this loop what they gave before it. */
int spx_preempt_toleration_nrt_sequential(spx_engine* e, const int64_t* rows, int64_t n_rows, const int32_t* priority, const uint8_t* preempt_never, const uint8_t* eligible, int64_t now_ns, const uint8_t* node_mask, int32_t preemption_mode);

/* CapacityScheduling's sequential preemption loop (kernels_preempt_seq.hip).  Tables, argument checks, limits, the
 * memory pre-check and staleness are spx_preempt_dry_run's, plus the side table below; a pod row listed twice is SPX_ERR_ARG.
 * spx_preempt_nominated_quota_soa: one entry per nominated record of the uploaded node table, in nom_ptr CSR order (n_nominated ==
 * nom_ptr[N]): the pod's namespace and its computePodResourceRequest with the scalar-key mask (spx_flatten_preempt_nominated_quota
 * forms all three).  spx_upload_preempt_nominated_quota: SPX_ERR_STATE before spx_upload_preempt_nodes; SPX_ERR_ARG when n_nominated
 * differs from the node table's nominated count; it marks earlier results stale, and a later spx_upload_preempt_nodes drops the table.
 * The loop needs it (SPX_ERR_STATE without) unless the node table has no nominated records.  Inside the loop PreFilter's two nominated
 * sums (capacity_scheduling.go:226-265) are formed from THIS list and the loop's own nominations, not from spx_quota_soa's nom_* list:
 * the device then has one list of nominated pods that it can clear and extend.  Precondition: both lists describe the same nominated
 * pods (those on present nodes); then a one-row loop is spx_preempt_dry_run of that row, bit for bit.
 * The rows are attempted once each, in list order.  Step i evaluates rows[i] on every unmasked present node (the dry run's
 * SelectVictimsOnNode and pick) against the state that steps 0..i-1 left, then applies (T1-T3 only when a node n was picked; restated
 * from upstream kube-scheduler — the nominator, prepareCandidate, the pod delete event reaching deletePod —, unpinned by a reference test):
 *   T4  every uploaded nomination of rows[i] itself, on any node, is dropped, also when there is no candidate
 *   T1  the victims of cell (i, n) leave n: Requested and the pod count shrink, nobody walks them again; for a victim of a quota'd
 *       namespace deletePodIfPresent (capacity_scheduling.go:778-792, elasticquota.go:172-187): that quota's Used and the aggregate Used
 *       shrink by the pod's quota request iff its SPX_PREEMPT_POD_IN_QUOTA_SET bit is set, scalar key presence OR-ed in (SetScalar)
 *   T3  nominated pods of n with a priority BELOW rows[i]'s lose their nomination, uploaded ones and earlier rows of the loop alike:
 *       they stop counting in the Filter's charge and in both PreFilter sums
 *   T2  rows[i] becomes a pod nominated to n, with its namespace, priority, fit_req and quota request.  It does not enter Used
 *       (Reserve's job)
 * At its own step a row sees: nominatedPodsReqInEQWithPodReq = its request + the live nominated entries of its namespace with priority
 * >= its own, other than itself; nominatedPodsReqWithPodReq = that + the live entries of other quota'd namespaces whose quota is not
 * usedOverMin() on the CURRENT Used; usedOverMinWith(inEQ) on the current Used; the borrowed marks formed from the current Used,
 * skipping the pods that left; the node's working Requested; the charge of the live nominated entries.  The sums are wrapping int64 adds.
 * eligible[i] == 0 (NULL = all eligible): the row is evaluated at its own step, its pick is reported and nothing is applied (T4
 * included).  There is no preempt_never column, as the capacity dry run has none: such rows arrive with eligible == 0.
 * PDB DisruptionsAllowed stays as uploaded.  A row whose nomination T3 cleared is not attempted again; eligibility is not recomputed.
 * The uploaded tables and marks are never written: a dry run of either kind after the loop gives what it gave before it, and a second
 * loop starts from the uploaded state.
 * Asynchronous on the engine stream, no host round trip between steps; spx_last_eval_ms reports the device time of the whole loop.
 * Memory beyond the dry run's: 100 bytes per node, 37 bytes per row, 65 bytes per namespace, one byte per assigned pod and per
 * nominated record (plus 69 per record for the side table).
 * The fetches answer for the loop until the next dry run of either kind: spx_fetch_preempt_pick / _cells / _keys give row i's pick
 * and cells as it saw them at its own step (column i of the cell buffer is written at step i and never again);
 * spx_fetch_preempt_victims(i, node) answers for node == row i's picked node from the victim set stored at the step, as positions
 * in the UPLOADED list of the node, most important first, and is SPX_ERR_ARG for any other node. */
typedef struct spx_preempt_nominated_quota_soa {
  int64_t n_nominated;
  const int32_t* ns;
  const int64_t* quota_req;          /* [n_nominated][8] */
  const uint8_t* quota_req_present;
} spx_preempt_nominated_quota_soa;
int spx_upload_preempt_nominated_quota(spx_engine* e, const spx_preempt_nominated_quota_soa* t);
int spx_preempt_sequential(spx_engine* e, const int64_t* rows, int64_t n_rows, const uint8_t* eligible, const uint8_t* node_mask);

/* CapacityScheduling's sequential preemption loop with NodeResourceTopologyMatch's Filter in the refit (kernels_preempt_nrt_seq.hip,
 * DESIGN.md 3.9j).  The contract is spx_preempt_sequential's in full (T1-T4, eligible, rows listed once, PDB budgets as uploaded,
 * PreFilter's sums from the nominated side table and the loop's own nominations, results through the same fetches,
 * spx_fetch_preempt_victims(i, node) for the picked node only) with the refit of spx_preempt_nrt_dry_run: NodeResourcesFit-with-nominated
 * && F at :607 and :636, the status order SPX_PREEMPT_ST_NO_VICTIMS, then the refit (SPX_PREEMPT_ST_NOT_FIT), then the quota test
 * (SPX_PREEMPT_ST_QUOTA), and a pod removed again for the quota (:646-649) on F's stack from then on.  One more rule, taken over from
 * spx_preempt_toleration_nrt_sequential:
 *   T5  the zone table, the placement info and the per-pod releases of spx_preempt_nrt_soa stay as uploaded at every step.  A pod that
 *       left at an earlier step contributes no release and is not counted in the stack size or the contributing count: it is gone from
 *       NodeInfo, nobody calls RemovePod for it again, so it is never on NRT's preemption stack again.  NRT ignores nominated pods, so T2
 *       and T3 do not touch F.  Unlike T1-T4 this is pinned by reference source: NRT's caches have no pod-delete path
 *       (pkg/noderesourcetopology/cache/passthrough.go, discardreserved.go, overreserve.go change on an NRT update, a Reserve / Unreserve
 *       or a resync only), so between two PostFilter calls of one batch the zone table is what the node agent last reported.
 *       A victim that F alone kept (NodeResourcesFit would have reprieved it) leaves its quota through T1 like any other victim: its
 *       quota's Used and the aggregate move, and with them the borrowed marks and over-min branches of later rows on every node.
 * With preemption_mode == 0, F is the ordinary Filter on the uploaded zone table at every step.
 * Argument checks, limits, the memory pre-check (which counts the NRT row record of 75 int64 per row, rounded up to 64 rows, as well)
 * and staleness are the union of the two: SPX_ERR_STATE without the quota tables (with min), without spx_upload_preempt_nodes / _pods,
 * without spx_upload_preempt_nominated_quota when the node table has nominated records, or without the side table of
 * spx_upload_preempt_nrt (which a later spx_upload_preempt_nodes or spx_upload_preempt_pods drops); SPX_ERR_ARG for an empty list or a
 * row outside the batch or listed twice.  The column of a step is launched by nodes, one wave each, so spx_preempt_nrt_dry_run's
 * limit of 65 535 x 64 rows does not apply here.  The uploaded tables and marks are never written: every dry run and every other loop
 * gives after this loop what it gave before it, and a second run of this loop starts from the uploaded state. */
int spx_preempt_nrt_sequential(spx_engine* e, const int64_t* rows, int64_t n_rows, const uint8_t* eligible, const uint8_t* node_mask, int32_t preemption_mode);

/* optional per-(pod,node) feasibility mask for normalizing score plugins: uint8 [n_pods][n_nodes],
 * non-zero = node passed Filter for that pod (upstream scores feasible nodes only).  NULL clears it. */
int spx_upload_feasible_mask(spx_engine* e, const uint8_t* mask, int64_t n_pods, int64_t n_nodes);

/* evaluate plugins in `plugin_mask` for pod rows [row_begin,row_end) against all nodes;
 * asynchronous on the engine stream; result tables stay in HBM */
int spx_eval(spx_engine* e, uint32_t plugin_mask, int64_t row_begin, int64_t row_end);
int spx_sync(spx_engine* e);

/* normalized score row of one pod (n_nodes bytes, 0..100) */
int spx_fetch_scores(spx_engine* e, int plugin, int64_t pod_row, uint8_t* out);
/* filter status row of one pod (n_nodes bytes; 0 = pass, else plugin-specific reason code) */
int spx_fetch_status(spx_engine* e, int plugin, int64_t pod_row, uint8_t* out);
/* rows [row_begin,row_end) of a score / status table in one strided copy: row r lands at out + (r - row_begin) * out_stride
 * (out_stride >= n_nodes bytes) — what a caller that drains a whole batch (or a parity harness) uses instead of row-by-row fetches */
int spx_fetch_score_rows(spx_engine* e, int plugin, int64_t row_begin, int64_t row_end, uint8_t* out, int64_t out_stride);
int spx_fetch_status_rows(spx_engine* e, int plugin, int64_t row_begin, int64_t row_end, uint8_t* out, int64_t out_stride);
/* exactness bookkeeping of the fast formulations: how many cells the float32 sweeps of TLP, LVRB and
 * LowRiskOverCommitment could not prove to round like the reference and re-evaluated with the reference's float64 sequence,
 * accumulated per plugin id since the last reset (SPX_NUM_PLUGINS entries; plugins without a fallback report 0).  The count is of
 * EVALUATIONS: a TargetLoadPacking sweep in the class form (SPX_OPT_TLP_POD_CLASSES) evaluates a run of rows with equal pod values
 * once and counts its re-evaluated cells once, not once per row of the table that holds them.  Synchronises the engine stream. */
int spx_fetch_stats(spx_engine* e, int64_t* reevaluated_cells, int reset);
/* raw int64 Score() row (before NormalizeScore) recomputed for one pod — the parity harness
 * and direct-call tests observe raw values (e.g. networkoverhead_test.go:803) */
int spx_fetch_raw(spx_engine* e, int plugin, int which, int64_t pod_row, int64_t* out);

/* device pointer + row stride (bytes) of a plugin's uint8 score table, for RCCL all-gather
 * by the caller (torch.distributed) or for zero-copy consumers */
int spx_score_table(spx_engine* e, int plugin, void** dptr, int64_t* row_stride, int64_t* n_rows);
/* make the engine write a plugin's score table into caller-owned device memory */
int spx_bind_score_table(spx_engine* e, int plugin, void* dptr, int64_t row_stride, int64_t n_rows);

/* per-pod weighted argmax over the evaluated plugins: best[k] node indices and their
 * sum_i weight[i]*score_i (upstream selectHost input); infeasible nodes are skipped.
 * `weights` holds SPX_NUM_PLUGINS entries indexed by plugin id (the entry of SPX_PLUGIN_COSCHED is ignored: the gate scores nothing).  Any int64 is a weight, negative ones included (the general
 * int64 argmax serves what the 32-bit one does not: a negative weight, a weight >= 2^23, sum of weight * 255 >= 2^31), as long
 * as no total can leave int64: with sum of |weight| * 255 over the plugins that own a score table above INT64_MAX the call
 * is refused with SPX_ERR_ARG and the weights in place stay (the largest single weight is 36170086419038336) */
int spx_set_plugin_weights(spx_engine* e, const int64_t* weights);
int spx_eval_best(spx_engine* e, uint32_t plugin_mask, int64_t row_begin, int64_t row_end);
/* per pod in [row_begin,row_end): best node (lowest index among ties, -1 when no node is feasible or the pod
 * failed CapacityScheduling.PreFilter), its weighted score, how many nodes tie for it, how many were feasible;
 * n_ties / n_feasible may be NULL */
int spx_fetch_best(spx_engine* e, int64_t row_begin, int64_t row_end, int32_t* node_idx, int64_t* weighted_score, int32_t* n_ties, int32_t* n_feasible);

/* Decisions without tables: what spx_eval + spx_eval_best would leave for spx_fetch_best, computed in one sweep that never
 * writes a score table (the per-row argmax is folded into the sweep: no 1 B/cell/plugin to HBM and back).  Fused for the
 * Filter-less profiles made of TLP, optionally ALLOCATABLE, and any of the Score-only plugins LVRB / LROC / PEAKS, with
 * non-negative plugin weights and no caller feasibility mask.  ALLOCATABLE's and TLP's tables are never written; the
 * (a mask that holds SYSCHED is served by the unfused route: spx_eval + spx_eval_best; NODEMETA and PODSTATE are summed from their
 * tables by either route)
 * Score-only plugins' tables ARE evaluated (spx_eval on those plugins, so they can be fetched afterwards) and read once by
 * the fused sweep in place of spx_eval_best's pass over every table.  Any other request is served by running spx_eval and
 * spx_eval_best.  Asynchronous on the engine stream like spx_eval. */
int spx_decide(spx_engine* e, uint32_t plugin_mask, int64_t row_begin, int64_t row_end);

/* Sequential scheduling of pod rows [row_begin,row_end), in row (= queue) order.  Unlike spx_eval's frozen
 * snapshot, every pod sees the commits of the pods before it:
 *   trimaran           a bound pod adds its predicted CPU utilisation to its node's missing utilisation
 *                      (pkg/trimaran/handler.go:131-139 feeding targetloadpacking.go:151-168);
 *   NRT                TopologyMatch.Reserve: the pod's effective request is subtracted from every zone of its node that reports the
 *                      resource (reserve.go:28-46, cache/overreserve.go:170-186, cache/store.go:315-356);
 *   CAPACITY           Reserve: the namespace's Used grows by the pod's request, a nominated pod that gets bound stops counting as
 *                      nominated (capacity_scheduling.go:350-364, elasticquota.go:89-98) — needs spx_quota_soa.min;
 *   NETOVERHEAD        the pod joins its AppGroup's scheduled list (networkoverhead.go:205-224) — needs spx_upload_net_commit.
 *   LROC               the scheduler cache has assumed the bound pod, so it is in nodeInfo.GetPods() of the next cycle: its requests and
 *                      its limits raised to the requests (the four numbers of spx_lroc_pods_soa) join the node's four sums of
 *                      spx_lroc_nodes_soa (GetNodeRequestsAndLimits, resourcestats.go:163-225, read by computeRank,
 *                      lowriskovercommitment.go:158-171).  Both risk terms of that node move: riskLimit through the sums, riskLoad
 *                      through NodeRequestMinusPod (:210-246) — the node's Beta fit is redone on the device;
 *   PEAKS              no commit state (load-watcher metric and node capacity only, peaks.go:103-144), but NormalizeScore is a
 *                      min-max over the pod's feasible nodes (:150-166): with NRT or NETOVERHEAD in the mask each pod's row is
 *                      normalised against that pod's own status rows; without one the rows are fixed and swept once up front.
 * plugin_mask is a subset of {ALLOCATABLE, TLP, LVRB, NRT, NETOVERHEAD, CAPACITY, LROC, PEAKS}; LROC and PEAKS need their node and
 * pod tables uploaded.  SYSCHED is still rejected (SySched's bind-time bookkeeping — addPod's union into the host set,
 * sysched.go:310-333 — is not carried by the loop).  NODEMETA and PODSTATE are rejected with the same SPX_ERR_ARG: PodState's nominated
 * count changes when a nominated pod binds, which is commit state the loop does not carry, and NodeMetadata stays out with it.
 * Route: a mask of ALLOCATABLE / TLP / LVRB alone runs the whole chain in one workgroup (about 3 us per pod).  Any other mask runs
 * per pod: one single-row spx_eval + spx_eval_best + the bookkeeping launches on the engine stream (tens of us per pod), the first
 * pod as plain launches, the rest replayed from one captured graph (a linear chain on the engine stream) whose kernels read the
 * row from a device counter — or, for a mask with a Filter plugin and without LROC / PEAKS, as ONE cooperative persistent launch
 * (SPX_OPT_COMMIT_COOP; it declines a mask with either scorer).  LowRiskOverCommitment's form (float32 / float64 / int64) is chosen
 * once for the batch from bounds that hold after every possible commit — per column, (largest node sum) + (sum of the batch's pod
 * column): below 2^47 with no limit below its request float32, below 2^52 float64, else int64; spx_kernel_path reports it.
 * On the per-pod route the score / status tables end up holding each row as its pod saw it (except Allocatable's when Filter
 * plugins are in the mask: its feasibility-aware normalisation then happens inside the argmax kernel, as in spx_decide).  A pod that fails PreFilter or has no
 * feasible node gets node -1 and reserves nothing.  Per pod: the node with the highest
 * sum of plugin_weight x score (lowest index among ties; upstream's selectHost draws among them), that sum, and the size
 * of the tie set (NULL = not wanted).  tlp_missing_out (NULL = not wanted) receives the per-node missing utilisation after
 * the last commit.  The engine's uploaded tables are left untouched (every table the loop mutates — LROC's four node sums and its
 * per-node table among them — is saved before and restored after); with LVRB in the mask its score table is (re)evaluated
 * for the row range first (LVRB carries no commit state, so the loop reads those rows).  Synchronous. */
int spx_commit_sequential(spx_engine* e, uint32_t plugin_mask, int64_t row_begin, int64_t row_end, int32_t* node_idx, int64_t* weighted_score, int32_t* n_ties, int64_t* tlp_missing_out);

/* duration in ms of the last spx_eval's kernels measured with HIP events on the engine stream.  It waits for those kernels but is not a
 * synchronisation point for their tables (the events carry no system-scope fence): spx_sync and the fetches are. */
int spx_last_eval_ms(spx_engine* e, float* ms);

/* Per-engine options (no process-wide state: two profiles in one scheduler process may differ).  Unknown option or value
 * out of range -> SPX_ERR_ARG.  Options take effect at the next launch, except SPX_OPT_ROW_ALIGN (before the first upload).
 *   SPX_OPT_ROW_ALIGN          row padding of the result tables in bytes (multiple of 16; default 128)
 *   SPX_OPT_REFERENCE_KERNELS  bit mask of plugin ids whose sweep runs the reference-arithmetic ("generic") kernel instead of
 *                              the fast formulation: TLP and LVRB (one switch for both), NRT, NETOVERHEAD, LROC (int64 form)
 *   SPX_OPT_LROC_FLOAT64       1 = LowRiskOverCommitment in the float64 form (no float32 quotient; that form also runs, whatever the
 *                              option says, when a column holds a value from 2^47 or a limit below its request)
 *   SPX_OPT_DECIDE_UNFUSED     1 = spx_decide always runs spx_eval + spx_eval_best
 *   SPX_OPT_NRT_SINGLE_LAUNCH  1 = NRT Filter and Score in one launch (default: two for Least/MostAllocated)
 *   SPX_OPT_COMMIT_FROM_MEMORY 1 = spx_commit_sequential keeps node state in memory (any node count) instead of registers
 *   SPX_OPT_PEAKS_TILE         nodes per lane of Peaks' float64 (min/max pass, write pass) — SPX_OPT_PEAKS_ESTIMATE 0: 44 (default), 84, 48, 88
 *   SPX_OPT_NRT_POD_CLASSES    1 (default) = a whole-batch NRT sweep evaluates one representative row per class of pods whose
 *                              records agree in everything the sweep reads and copies it to the rest of the class; 0 = every row
 *   SPX_OPT_NRT_LN_LIST_PERMILLE  LeastNUMANodes, batch Score launch: room, in thousandths of the node count, of each per-(row, scope)
 *                              list of cells left to the complete subset search (default 375; 4 bytes per entry).  A list that
 *                              overflows sends the launch back to the complete sweep: same table, slower
 *   SPX_OPT_PEAKS_POD_CLASSES  1 (default) = a whole-batch Peaks sweep with no Filter table in play evaluates one row per distinct
 *                              pod cpu request (all Peaks.Score reads of the pod, peaks.go:134-138) and copies it; 0 = every row
 *   SPX_OPT_COMMIT_COOP        1 (default) = spx_commit_sequential with Filter plugins in the mask runs as ONE cooperative persistent launch
 *                              (node state in registers, two granule exchanges per pod) when the profile fits it; 0 = always the per-pod
 *                              single-row launches replayed from a graph
 *   SPX_OPT_NRT_RANK_FILTER    1 (default) = a whole-batch NRT sweep over pod classes runs its Filter launch in rank space (requests and
 *                              zone quantities as positions in the chunk's sorted request list: integer subtracts instead of float64
 *                              compares, no zone-table mutation); 0 = the float64 Filter launch.  Same status table either way
 *   SPX_OPT_ROW_WORKGROUP      1 = the per-row kernels of a profile with Filter plugins (Allocatable's feasibility-aware NormalizeScore,
 *                              spx_decide's argmax) give every row a whole workgroup in batch launches too; 0 (default) = four rows per
 *                              workgroup, and the whole-workgroup mapping only when four rows' feasibility bytes would not fit the LDS
 *                              (rows of more than about 65k nodes).  Same tables either way
 *   SPX_OPT_TLP_AMB_TABLE      1 (default) = a multi-row TargetLoadPacking sweep (tables or spx_decide; LoadVariationRiskBalancing's sweep likewise, per cpu / memory request) first lists, per pod value and node tile,
 *                              where a cell of the float32 formulation can be within its error bound of a rounding tie or of the branch point
 *                              (a property of the node alone: the score is piecewise linear in the pod's integer millicores), and only the rows
 *                              named there carry the per-cell exactness bookkeeping; 0 = every cell carries it.  Same tables either way
 *   SPX_OPT_NRT_PACKED_SCORE   1 (default) = NodeResourceTopologyMatch LeastAllocated's Score launch of a row range keeps the zone totals of two
 *                              zones per register and scores in packed float32 (4 instructions per zone pair and resource instead of 6) when
 *                              every weighted slot qualifies: capacities / 2^s <= 32768 with 2^s the power of two common to the slot's
 *                              capacities and requests (cpu in whole cores, devices, hugepages in pages), or — one slot, memory in bytes —
 *                              through a per-launch table of the requests for which the float32 form differs from the division (those pods
 *                              are recomputed in float64 for the node window concerned); spx_nrt_packed_score_slots reports which;
 *                              0 = float64 throughout.  Same tables either way
 *   SPX_OPT_NET_ALLOC_FUSED    1 (default) = when NetworkOverhead and NodeResourcesAllocatable are evaluated together over a row range with
 *                              Filter plugins in play, the NetworkOverhead table sweep also writes Allocatable's table (NormalizeScore over
 *                              each pod's feasible nodes — the set that sweep already walks) instead of a separate launch that reads every
 *                              status table again; 0 = separate launches.  Same tables either way
 *   SPX_OPT_NRT_RANK_NARROW    1 (default) = chunks of the rank-space Filter's stream (SPX_OPT_NRT_RANK_FILTER) whose lists all have at most 127
 *                              distinct quantities keep four zones' counts per register instead of two (half the subtract / and instructions
 *                              per comparison); 0 = two per register everywhere.  Read when pod rows are uploaded.  Same tables either way
 *   SPX_OPT_PEAKS_ESTIMATE     1 (default) = both passes of Peaks (row min / max, then NormalizeScore) first bound every cell's raw score by a
 *                              float32 interval proven to contain the float64 value (13 float32 instructions + one v_exp_f32) and run the
 *                              float64 sequence (division, exp) only for the cells the interval cannot decide — the candidates for a row's
 *                              extremes, the cells next to a step of floor(100 (raw - min) / span), nodes outside the interval's
 *                              preconditions — listed by the sweep and evaluated by a second launch with every lane busy; rows in which
 *                              the interval decides little (a pod that requests no cpu) take the float64 sequence for the whole tile;
 *                              8 = the same with 8 instead of 16 nodes per lane; 0 = the float64 sequence for every cell.  Same tables either way.
 *                              (The interval's bounds assume cpu requests >= 0: a batch that holds a negative one runs the float64 passes)
 *                              Scratch, allocated by the first Peaks evaluation with the option on and kept: the undecided cells' lists, 24 bytes
 *                              per (swept pod row, tile of 1024 nodes — 512 with the value 8) whatever the chunking — 24 MB for 100 000 rows x
 *                              10 000 nodes, 240 MB for 500 000 x 20 000 — plus 96 bytes per node; a list that fills up falls back to one
 *                              "whole tile" entry, so the size bounds memory, not correctness
 *   SPX_OPT_NRT_FUSED          1 (default) = a whole-batch NodeResourceTopologyMatch sweep runs Filter and Score in ONE launch
 *                              (kernels_nrt_fused.hip: rank-space Filter, float32 Score, pod records staged once) for the Least- and
 *                              MostAllocated strategies with unit weights under the preconditions of SPX_OPT_NRT_RANK_FILTER and
 *                              SPX_OPT_NRT_PACKED_SCORE, and for BalancedAllocation with up to four resource slots (its undecided cells are
 *                              recomputed in float64 by a second launch); 0 = the Filter launch and the Score launch.  Same tables either way
 *   SPX_OPT_NRT_WIDE           1 = spx_load_nrt / spx_load_profile take the wide NRT tables (kernels_nrt_wide.hip) for a snapshot of 8 or
 *                              fewer resource slots too; 0 (default) = only above 8 slots.  Read at the load, not at the launch
 *   SPX_OPT_ALLOC_TABLE_KEEP   1 (default) = an spx_eval with no Filter plugin and no feasibility mask in play does not write rows of
 *                              NodeResourcesAllocatable's engine-owned score table that already hold what it would write: without a Filter the
 *                              table is one normalised row repeated for every pod (allocatable.go:118-126 never reads the pod), so it changes
 *                              only when the node allocatable columns or spx_set_allocatable_params change that row — not with a new pod
 *                              batch, a load-watcher delta, or a node re-list that leaves the row as it was.  The engine records which rows
 *                              hold the row in place; the masked normalisations, spx_bind_score_table and a reallocation reset the record, and
 *                              a bound (caller-owned) table is always written.  A caller that writes into the engine-owned table through the
 *                              pointer of spx_score_table sets the option to 0.  The record is made when the writing launch is issued and
 *                              assumes that issued launches execute: a caller that captures spx_eval into a graph of its own and does not
 *                              replay it sets the option to 0 as well.  0 = every spx_eval writes the rows.  Same tables either
 *                              way; spx_alloc_table_path reports what the last spx_eval did
 *   SPX_OPT_TLP_POD_CLASSES    1 (default) = a whole-batch spx_eval of TargetLoadPacking (rows [0, n_pods), at least 256 of them, under the
 *                              conditions of SPX_OPT_TLP_AMB_TABLE, which must be on) sweeps the rows in the order of their pod value —
 *                              the pod enters a TargetLoadPacking row through the one number spx_flatten_trimaran_pods computes for it
 *                              (targetloadpacking.go:137-160), so rows with equal values are equal byte for byte — and evaluates a run of
 *                              equal values once per 64 positions of that order, storing the result to every row of the run.  The order
 *                              is built on the device whenever the pod column is uploaded (spx_upload_trimaran_pods, spx_load_trimaran,
 *                              spx_load_trimaran_pods); a batch takes this form only when enough of its rows are such copies
 *                              (spx_tlp_pod_classes reports the count).  2 = whenever at least one row is a copy (measurements);
 *                              0 = every row is evaluated, in row order.  Same tables either way; spx_tlp_form reports what ran.
 *                              spx_decide's sweep and partial row ranges always evaluate every row
 *   SPX_OPT_TLP_CHUNK_SCHED    1 (default) = the order of SPX_OPT_TLP_POD_CLASSES is launched heaviest chunk first: its chunks of 64 positions
 *                              are sorted (stable) by descending number of positions the sweep evaluates in them, so that the launch ends
 *                              in waves that only store instead of in the waves that compute most; the last, partial chunk stays last.
 *                              0 = the chunks in value order.  Read when the order is built, i.e. it takes effect at the next upload of
 *                              the pod column.  Same tables and the same spx_tlp_pod_classes either way
 */
#define SPX_OPT_ROW_ALIGN 0
#define SPX_OPT_REFERENCE_KERNELS 1
#define SPX_OPT_LROC_FLOAT64 2
#define SPX_OPT_DECIDE_UNFUSED 3
#define SPX_OPT_NRT_SINGLE_LAUNCH 4
#define SPX_OPT_COMMIT_FROM_MEMORY 5
#define SPX_OPT_PEAKS_TILE 6
#define SPX_OPT_NRT_POD_CLASSES 7
#define SPX_OPT_PEAKS_POD_CLASSES 8
#define SPX_OPT_NRT_LN_LIST_PERMILLE 9
#define SPX_OPT_COMMIT_COOP 10
#define SPX_OPT_NRT_RANK_FILTER 11
#define SPX_OPT_ROW_WORKGROUP 12
#define SPX_OPT_TLP_AMB_TABLE 13
#define SPX_OPT_NRT_PACKED_SCORE 14
#define SPX_OPT_NET_ALLOC_FUSED 15
#define SPX_OPT_NRT_RANK_NARROW 16
#define SPX_OPT_PEAKS_ESTIMATE 17
#define SPX_OPT_NRT_FUSED 18
#define SPX_OPT_NRT_WIDE 19
#define SPX_OPT_ALLOC_TABLE_KEEP 20
#define SPX_OPT_TLP_POD_CLASSES 21
#define SPX_OPT_TLP_CHUNK_SCHED 22
#define SPX_NUM_OPTIONS 23
int spx_set_option(spx_engine* e, int option, int64_t value);
int spx_get_option(const spx_engine* e, int option, int64_t* value);

/* Pod equivalence classes of the uploaded NRT pod batch (spx_upload_nrt_pods): n_unique = rows that represent a class (or only
 * themselves), n_copies = rows that repeat an earlier row's NRT record in everything the sweep reads — Deployment replicas, and
 * pods whose verdict does not depend on quantities (not filtered: filter.go:186-190; non-Guaranteed: score.go:72-76,
 * numaresources.go:137-142).  n_unique + n_copies = n_pods.  A whole-batch spx_eval of NRT evaluates the unique rows and copies. */
int spx_nrt_pod_classes(const spx_engine* e, int64_t* n_unique, int64_t* n_copies);
/* The same for the uploaded Peaks pod batch (spx_upload_peaks_pods): Peaks.Score reads one number of the pod — the cpu request of
 * peaks.go:134 (GetResourceRequestQuantity) — so pods that request the same amount get the same raw row, and, when no Filter plugin
 * or feasibility mask narrows a pod's node list, the same NormalizeScore (peaks.go:150-166). */
int spx_peaks_pod_classes(const spx_engine* e, int64_t* n_unique, int64_t* n_copies);

/* The same for TargetLoadPacking and the uploaded trimaran pod batch, in the terms of the class form's sweep (SPX_OPT_TLP_POD_CLASSES):
 * rows_evaluated = positions of the value-sorted row order that start a chunk of 64 or hold another value than the position before,
 * rows_copied = n_pods - rows_evaluated, the rows that are stores of a result the wave already holds.  SPX_ERR_STATE without a batch. */
int spx_tlp_pod_classes(const spx_engine* e, int64_t* rows_evaluated, int64_t* rows_copied);
/* Which form the last spx_eval with TargetLoadPacking in the mask launched for it: 1 = every row evaluated in row order, 2 = the class
 * form; 0 = none yet, or the reference-arithmetic kernel ran (SPX_OPT_REFERENCE_KERNELS, a target outside [1, 99]) */
int spx_tlp_form(const spx_engine* e);
/* The order the class form sweeps the uploaded batch in, copied to the host (tests, measurements): rows[pos] = the pod row at position
 * pos, n_pods entries.  Positions [64 c, 64 c + 64) are one wave's chunk; SPX_OPT_TLP_CHUNK_SCHED decides the order of the chunks.
 * SPX_ERR_STATE without an order. */
int spx_tlp_fetch_order(spx_engine* e, int32_t* rows);

/* The same for the uploaded SySched pod batch (spx_upload_sysched_pods): a pod enters SySched.Score through its syscall set alone, so
 * n_unique = pods that are the first of the batch with their set, n_copies = the rest. */
int spx_sysched_pod_classes(const spx_engine* e, int64_t* n_unique, int64_t* n_copies);

/* Object tables -> SoA columns -> device in one call per plugin family: the host flatteners (spx_flatten_*, below) run with the
 * engine's current plugin parameters and their result is uploaded.  For callers that hold object tables — marshalled by the shim or
 * decoded by spx_ingest_* — and would rather not size and own the intermediate arrays (the cgo shim: shim/go/pkg/spx/snapshot.go).
 * spx_load_trimaran serves Allocatable + TargetLoadPacking + LoadVariationRiskBalancing (rc / assigned may be NULL);
 * spx_load_network also uploads the commit effects spx_commit_sequential needs; it flattens the cost matrices in int64 and uploads the
 * 32-bit tables when every entry fits them, the wide ones otherwise (spx_upload_net_topo_wide): the caller sees no difference. */
int spx_load_trimaran(spx_engine* e, const spx_node_objects* nodes, const spx_resource_classes* rc, const spx_pod_objects* pods, const spx_metrics_objects* metrics, const spx_assigned_objects* assigned);
/* a new pending batch only (node tables stay): the trimaran / Allocatable pod columns flattened straight into pinned staging, one pass */
int spx_load_trimaran_pods(spx_engine* e, const spx_pod_objects* pods);
int spx_load_nrt(spx_engine* e, const spx_node_objects* nodes, const spx_nrt_objects* nrt, const spx_resource_classes* rc, const spx_pod_objects* pods, const spx_nrt_params* params);
/* wall time in ms of the six stages of the last spx_load_nrt on this engine: [0] spx_flatten_nrt_slots, [1] spx_flatten_nrt_nodes,
 * [2] spx_flatten_nrt_pods, [3] parameters + slot table, [4] spx_upload_nrt_nodes, [5] spx_upload_nrt_pods (bench.py reports them) */
int spx_last_load_nrt_ms(const spx_engine* e, double* ms6);
int spx_load_network(spx_engine* e, const spx_node_objects* nodes, const spx_pod_objects* pods, const spx_appgroup_objects* appgroups, const spx_nettopo_objects* nettopo);
int spx_load_quota(spx_engine* e, const spx_pod_objects* pods, const spx_resource_classes* rc, const spx_quota_objects* quota);
/* SySched: flatten + upload of both tables (spx_flatten_sysched_nodes / _pods) */
int spx_load_sysched(spx_engine* e, const spx_sysched_objects* o);
/* The whole profile in one call: the loaders above run side by side on host threads of the library (they fill disjoint tables and share
 * the engine's stream; spx_load_nrt itself runs its node half and its pod half on two threads).  nodes and pods are required; a loader
 * whose members are NULL is skipped: metrics (+ rc, assigned) = spx_load_trimaran, nrt + nrt_params = spx_load_nrt, appgroups + nettopo =
 * spx_load_network, quota = spx_load_quota; nrt without nrt_params is SPX_ERR_ARG.  Returns the first failing loader's code, and
 * spx_last_error on the calling thread names that loader's failure.  No other call on the engine may run meanwhile. */
typedef struct spx_profile_objects {
  const spx_node_objects* nodes;
  const spx_resource_classes* rc;
  const spx_pod_objects* pods;
  const spx_metrics_objects* metrics;
  const spx_assigned_objects* assigned;
  const spx_nrt_objects* nrt;
  const spx_nrt_params* nrt_params;
  const spx_appgroup_objects* appgroups;
  const spx_nettopo_objects* nettopo;
  const spx_quota_objects* quota;
} spx_profile_objects;
int spx_load_profile(spx_engine* e, const spx_profile_objects* o);

/* Which form the last spx_commit_sequential ran: 1 = the one-workgroup chain of a mask of ALLOCATABLE / TLP / LVRB, 2 = per-pod single-row
 * launches (replayed from a graph; always with LROC or PEAKS in the mask), 3 = the cooperative persistent kernel; 0 = none yet */
int spx_commit_path(const spx_engine* e);
/* Which Filter launch the last NodeResourceTopologyMatch sweep ran: 1 = float64 compares (k_nrt_fast / the reference-arithmetic
 * kernel), 2 = rank space (SPX_OPT_NRT_RANK_FILTER: whole-batch sweeps), 3 = rank space inside the fused Filter + Score launch
 * (SPX_OPT_NRT_FUSED), 4 = the wide tables' sweep (kernels_nrt_wide.hip); 0 = none yet */
int spx_nrt_filter_path(const spx_engine* e);
/* What the last spx_eval on this engine (those spx_decide and spx_commit_sequential issue included) did with NodeResourcesAllocatable's
 * score table: 1 = wrote the rows (the broadcast row, or the feasibility-aware normalisation with Filter plugins in play), 2 = kept
 * them (SPX_OPT_ALLOC_TABLE_KEEP: they already held the row in place, no Allocatable store was issued); 0 = Allocatable was not in
 * the mask, its normalisation was folded into spx_decide's argmax, or no spx_eval has run */
int spx_alloc_table_path(const spx_engine* e);
/* SPX_OPT_NRT_PACKED_SCORE with the uploaded tables and parameters: 0 = the LeastAllocated Score launch keeps float64 (other strategy,
 * large weights, a slot that qualifies neither way, option off); else bit 24 set, bits 0..15 = the weighted slots (positions of the
 * uploaded slot table) that are packed unconditionally, bits 16..23 = 1 + the slot that goes through the per-launch table, 0 = none */
int spx_nrt_packed_score_slots(const spx_engine* e);

/* which formulation of a plugin's sweep the uploaded tables select: 0 = generic (reference arithmetic, operation for
 * operation), 1 = fast formulation (same results; see DESIGN.md for each kernel's preconditions); <0 on error.
 * Tests use it to make sure both formulations are exercised.
 * SPX_PLUGIN_LROC: 1 = the float32 sweep; after a spx_commit_sequential with LROC in its mask, and until the next spx_eval of the
 * plugin or upload of its tables, the form that loop chose for its batch (1 = float32, 0 = float64 or int64).
 * SPX_PLUGIN_NETOVERHEAD also reports 2 = the 64-bit sweep (kernels_network_wide.hip): the engine holds int64 cost matrices, or
 * (largest cost entry) x (most pairs of any workload key) reaches 2^31.  SPX_OPT_REFERENCE_KERNELS selects the per-node form of the
 * same 64-bit arithmetic there, and the value stays 2.
 * SPX_PLUGIN_SYSCHED has one formulation; for it the call reports how many chunks of distinct sets the last SySched sweep of
 * spx_eval built its raw table in (the table is scratch bounded at 256 MiB, kernels_sysched.hip), 0 before the first sweep. */
/* SPX_PLUGIN_COSCHED: how many groups of the last evaluation of the gate took the walk (the groups with assigned pods: a workgroup
 * each over the nodes, kernels_cosched.hip); the others read their slots' overall maxima. */
int spx_kernel_path(const spx_engine* e, int plugin);

/* make the engine write a Filter plugin's status table (NRT, NETOVERHEAD) into caller-owned device memory; row_stride must be
 * the engine's (spx_score_table reports it), n_rows >= n_pods; dptr NULL unbinds */
int spx_bind_status_table(spx_engine* e, int plugin, void* dptr, int64_t row_stride, int64_t n_rows);

/* ------------------------------------------------------------------ several devices, one host process
 *
 * north_star: "the pods x nodes matrix shards by pod rows across the 8 GPUs of one node with a single RCCL all-gather over
 * xGMI to reassemble the global score/feasibility table", driven by ONE Go scheduler process.  spx_multi owns one engine per
 * device and one host thread per device (launches of a step are issued concurrently).  Pod rows shard in equal contiguous
 * ranges (spx_multi_shard); node tables are replicated: the caller uploads the node tables to every rank's engine and each
 * rank's slice of the pod columns to that rank's engine (spx_multi_engine + the spx_upload_* calls — slicing SoA pod columns is
 * pointer arithmetic).  The evaluation itself has no collective.  Afterwards:
 *   spx_multi_gather_best        all-gathers the per-pod decisions (20 B per pod) so that every device holds the global vector and
 *                                hands it to the host in batch order;
 *   spx_multi_bind_global_table  gives every device a [n_pods_total][row_stride] uint8 table (which: 0 score, 1 Filter status)
 *                                into whose own slice the rank's engine writes directly (no staging copy), and
 *   spx_multi_allgather_table    reassembles it on every device in place.
 * transport: SPX_MULTI_TRANSPORT_RCCL = ncclAllGather on each engine's stream (librccl.so.1 is dlopen'ed here, so a
 * single-GPU scheduler never maps it; needs distinct devices); SPX_MULTI_TRANSPORT_PEER_COPY = the same bytes with
 * hipMemcpyPeerAsync (also works with several ranks on one device: how the sharding logic is tested on a one-GPU box).
 * Calls on one spx_multi must come from one thread at a time.  The layer's loaders carry no LROC, Peaks or SySched tables: those
 * plugins are uploaded per rank through spx_multi_engine. */
#define SPX_MULTI_TRANSPORT_RCCL 0
#define SPX_MULTI_TRANSPORT_PEER_COPY 1
typedef struct spx_multi spx_multi;
int spx_multi_create(const int* device_ids, int n_devices, int transport, spx_multi** out);
int spx_multi_destroy(spx_multi* m);
/* of `m`, or of the failed spx_multi_create when m == NULL (thread-local) */
const char* spx_multi_last_error(const spx_multi* m);
int spx_multi_size(const spx_multi* m);
int spx_multi_engine(spx_multi* m, int rank, spx_engine** out);
/* ranks of the RCCL communicator the exchange runs on, as RCCL reports it (ncclCommCount of rank 0's communicator after
 * ncclCommInitAll); 0 with the peer-copy transport.  bench.py prints it so that a scaling record shows how many ranks RCCL saw */
int spx_multi_rccl_ranks(const spx_multi* m);
/* rank's rows of a batch of n_pods_total pending pods: [rank * per, (rank + 1) * per) clipped to the batch, per = ceil(n / size) */
int spx_multi_shard(const spx_multi* m, int64_t n_pods_total, int rank, int64_t* row_begin, int64_t* row_end);
/* every rank: spx_eval / spx_eval_best / spx_decide over all of its local rows, issued concurrently, asynchronous */
int spx_multi_eval(spx_multi* m, uint32_t plugin_mask);
int spx_multi_eval_best(spx_multi* m, uint32_t plugin_mask);
int spx_multi_decide(spx_multi* m, uint32_t plugin_mask);
int spx_multi_sync(spx_multi* m);
/* outputs are indexed by batch row, n_pods_total entries each; n_ties / n_feasible may be NULL.  Synchronous. */
int spx_multi_gather_best(spx_multi* m, int64_t n_pods_total, int32_t* node_idx, int64_t* weighted_score, int32_t* n_ties, int32_t* n_feasible);
int spx_multi_bind_global_table(spx_multi* m, int plugin, int which, int64_t n_pods_total);
int spx_multi_allgather_table(spx_multi* m, int plugin, int which);
/* rank's copy of the global table (device pointer on that rank's device) */
int spx_multi_global_table(spx_multi* m, int plugin, int which, int rank, void** dptr, int64_t* row_stride, int64_t* n_rows);
/* batch rows [row_begin,row_end) of rank's copy of a gathered global table (any rank holds all rows) */
int spx_multi_fetch_global_rows(spx_multi* m, int plugin, int which, int rank, int64_t row_begin, int64_t row_end, uint8_t* out, int64_t out_stride);
/* region timing with HIP events on every rank's stream: spx_multi_mark(m, 0) ... work ... spx_multi_mark(m, 1), then the
 * elapsed time between the marks per rank (ms_per_rank: size entries, may be NULL) and its maximum */
int spx_multi_mark(spx_multi* m, int which);
int spx_multi_marked_ms(spx_multi* m, float* ms_max, float* ms_per_rank);
/* HIP-event durations, max over ranks: of the last spx_multi_eval / _decide, and of the last gather (either may be NULL) */
int spx_multi_last_ms(spx_multi* m, float* eval_ms, float* gather_ms);

/* ------------------------------------------------------------------ host flatteners (object -> SoA) */

/* output buffers are caller-allocated with the sizes noted */
int spx_flatten_alloc_nodes(const spx_node_objects* nodes, const spx_resource_classes* rc, const spx_allocatable_params* p, int64_t* alloc_out);
int spx_flatten_trimaran_nodes(const spx_node_objects* nodes, const spx_metrics_objects* metrics, const spx_assigned_objects* assigned, const spx_tlp_params* tlp, int64_t* cap_cpu_milli, double* tlp_cpu_util, int64_t* tlp_missing_milli, uint8_t* tlp_valid, int64_t* lv_alloc_cpu_milli, int64_t* lv_alloc_mem, double* lv_cpu_avg, double* lv_cpu_std, double* lv_mem_avg, double* lv_mem_std, uint8_t* lv_flags);
int spx_flatten_trimaran_pods(const spx_pod_objects* pods, const spx_tlp_params* tlp, int64_t* tlp_pod_milli, int64_t* lv_req_cpu_milli, int64_t* lv_req_mem);
/* the same columns for the listed nodes only (n_rows rows; row j = node idx[j]): the input of spx_update_trimaran_nodes */
int spx_flatten_trimaran_node_rows(const spx_node_objects* nodes, const spx_metrics_objects* metrics, const spx_assigned_objects* assigned, const spx_tlp_params* tlp, const int64_t* idx, int64_t n_rows, int64_t* cap_cpu_milli, double* tlp_cpu_util, int64_t* tlp_missing_milli, uint8_t* tlp_valid, int64_t* lv_alloc_cpu_milli, int64_t* lv_alloc_mem, double* lv_cpu_avg, double* lv_cpu_std, double* lv_mem_avg, double* lv_mem_std, uint8_t* lv_flags);
/* LowRiskOverCommitment: every output array has one entry per node / per pod */
int spx_flatten_lroc_nodes(const spx_node_objects* nodes, const spx_node_pods_objects* node_pods, int64_t* req_cpu_milli, int64_t* req_mem, int64_t* lim_cpu_milli, int64_t* lim_mem);
int spx_flatten_lroc_pods(const spx_pod_objects* pods, int64_t* req_cpu_milli, int64_t* req_mem, int64_t* lim_cpu_milli, int64_t* lim_mem);
/* Peaks: node arrays sized [N], pod array [P] */
int spx_flatten_peaks_nodes(const spx_node_objects* nodes, const spx_metrics_objects* metrics, const spx_power_model_objects* models, int64_t* cap_cpu_milli, double* cpu_util, uint8_t* valid, double* k1, double* k2);
int spx_flatten_peaks_pods(const spx_pod_objects* pods, int64_t* cpu_milli);

/* SySched.  spx_flatten_sysched_nodes: *n_words_out and *n_stale_out (entries of the stale CSR) are written first; with every
 * output array NULL the call only counts.  Otherwise host_bits [n_words][N], present / n_resident / resident_missing [N],
 * stale_ptr [N+1], stale_bit / stale_count [stale_cap] (stale entries of a node in ascending bit order); more entries than
 * stale_cap, more than SPX_SYSCHED_MAX_NAMES names, or a name / set id out of range are SPX_ERR_ARG.  A node that is not
 * present gets zero bits, k = a = 0 and no stale entries (Score returns 0 there whatever HostToPods holds, sysched.go:253-259).
 * spx_flatten_sysched_pods: set_bits [n_sets][n_words], pod_set [P]. */
int spx_flatten_sysched_nodes(const spx_sysched_objects* o, int64_t stale_cap, int32_t* n_words_out, int64_t* n_stale_out, uint64_t* host_bits, uint8_t* present, int32_t* n_resident, int32_t* resident_missing, int32_t* stale_ptr, int32_t* stale_bit, int32_t* stale_count);
int spx_flatten_sysched_pods(const spx_sysched_objects* o, uint64_t* set_bits, int32_t* pod_set);

/* NRT: builds the dense slot numbering from every resource id pods request or zones report
 * (slot_res/slot_flags/slot_weight sized SPX_NRT_MAX_RES; *n_res_out receives the count) */
int spx_flatten_nrt_slots(const spx_pod_objects* pods, const spx_nrt_objects* nrt, const spx_resource_classes* rc, const spx_nrt_params* p, int32_t* n_res_out, int32_t* slot_res, uint8_t* slot_flags, int64_t* slot_weight);
/* node arrays sized: flags[N], max_numa[N], n_zones[N], zone_id[N*8], zone_present[N*8], zone_avail[N*8*n_res], zone_cost[N*8*8], min_avg_dist[N*8], node_present[N] */
int spx_flatten_nrt_nodes(const spx_node_objects* nodes, const spx_nrt_objects* nrt, const spx_nrt_slots* slots, uint8_t* flags, int32_t* max_numa, uint8_t* n_zones, uint8_t* zone_id, uint8_t* zone_present, int64_t* zone_avail, int32_t* zone_cost, float* min_avg_dist, uint8_t* node_present);
/* the same columns for the listed nodes only (n_rows rows; row j = node idx[j]): the input of spx_update_nrt_nodes */
int spx_flatten_nrt_node_rows(const spx_node_objects* nodes, const spx_nrt_objects* nrt, const spx_nrt_slots* slots, const int64_t* idx, int64_t n_rows, uint8_t* flags, int32_t* max_numa, uint8_t* n_zones, uint8_t* zone_id, uint8_t* zone_present, int64_t* zone_avail, int32_t* zone_cost, float* min_avg_dist, uint8_t* node_present);
/* pod arrays sized: qos[P], non_native[P], n_ctr[P], ctr_kind[P*8], ctr_present[P*8], ctr_req[P*8*n_res], pod_present[P], pod_req[P*n_res] */
int spx_flatten_nrt_pods(const spx_pod_objects* pods, const spx_resource_classes* rc, const spx_nrt_slots* slots, uint8_t* qos, uint8_t* non_native, uint8_t* n_ctr, uint8_t* ctr_kind, uint8_t* ctr_present, int64_t* ctr_req, uint8_t* pod_present, int64_t* pod_req);
/* the containers of the pods with more than SPX_NRT_MAX_CTRS containers (the long rows spx_flatten_nrt_pods marks), CSR as
 * spx_nrt_long_pods.  *n_long_out / *n_ctr_out receive the counts; with every output array NULL the call only counts.  Otherwise
 * pod_row / ctr_ptr must hold long_cap / long_cap + 1 entries and ctr_kind / ctr_present / ctr_req ctr_cap / ctr_cap / ctr_cap x n_res,
 * and a table larger than that is SPX_ERR_ARG (the counts are written first, so the caller can resize and call again). */
int spx_flatten_nrt_long_pods(const spx_pod_objects* pods, const spx_resource_classes* rc, const spx_nrt_slots* slots, int64_t long_cap, int64_t ctr_cap, int64_t* n_long_out, int64_t* n_ctr_out, int32_t* pod_row, int32_t* ctr_ptr, uint8_t* ctr_kind, uint8_t* ctr_present, int64_t* ctr_req);
/* the zones of the nodes with 9 to SPX_NRT_TALL_MAX_ZONES zones (the tall nodes spx_flatten_nrt_nodes marks), as spx_nrt_tall_nodes.
 * *n_tall_out / *zone_stride_out receive the counts; with every output array NULL the call only counts.  Otherwise tall_cap nodes and
 * stride_cap zones per node must hold them (SPX_ERR_ARG if not); the arrays are laid out by the counts themselves (zone_stride =
 * *zone_stride_out, the most zones any tall node lists), not by the caps.  Assumed pods are subtracted and duplicate ids' costs
 * resolved as in spx_flatten_nrt_nodes.  SPX_ERR_ARG for a node with a 65th zone or with id 64 on a counted zone, and for a slot table
 * of more than SPX_NRT_MAX_RES slots (tall nodes in a wide snapshot stay refused). */
int spx_flatten_nrt_tall_nodes(const spx_node_objects* nodes, const spx_nrt_objects* nrt, const spx_nrt_slots* slots, int64_t tall_cap, int32_t stride_cap, int64_t* n_tall_out, int32_t* zone_stride_out, int32_t* node_idx, uint8_t* flags, int32_t* max_numa, uint8_t* node_present, uint8_t* n_zones, uint8_t* zone_id, uint8_t* zone_present, int64_t* zone_avail, int32_t* zone_cost, float* min_avg_dist);
/* SPX_OK and the first node (or -1) with more than SPX_NRT_MAX_ZONES zones of type Node with ids 0..64, and its zone count; SPX_ERR_ARG
 * and the first node beyond this build's limits (a 65th zone, or id 64 on a tall node) when there is one: what a loader names when
 * it refuses a snapshot.  Host only. */
int spx_nrt_first_tall_node(const spx_nrt_objects* nrt, int64_t* node_out, int32_t* n_zones_out);
/* The wide forms (up to SPX_NRT_MAX_RES_WIDE slots).  spx_flatten_nrt_slots_wide: the numbering of spx_flatten_nrt_slots (ascending
 * resource id) for up to cap <= SPX_NRT_MAX_RES_WIDE slots; *n_res_out receives the count even when it exceeds cap (SPX_ERR_ARG). */
int spx_flatten_nrt_slots_wide(const spx_pod_objects* pods, const spx_nrt_objects* nrt, const spx_resource_classes* rc, const spx_nrt_params* p, int32_t cap, int32_t* n_res_out, int32_t* slot_res, uint8_t* slot_flags, int64_t* slot_weight);
/* node arrays sized as spx_flatten_nrt_nodes', zone_present [N*8] and node_present [N] as uint32 masks */
int spx_flatten_nrt_nodes_wide(const spx_node_objects* nodes, const spx_nrt_objects* nrt, const spx_nrt_slots* slots, uint8_t* flags, int32_t* max_numa, uint8_t* n_zones, uint8_t* zone_id, uint32_t* zone_present, int64_t* zone_avail, int32_t* zone_cost, float* min_avg_dist, uint32_t* node_present);
/* the pod table of spx_nrt_pods_wide.  *n_req_out / *n_ent_out receive the entry counts of the pod-level and container lists; with
 * every output array NULL the call only counts.  Otherwise qos / non_native [P], req_ptr / ctr_ptr [P+1], ctr_kind [C], ent_ptr [C+1]
 * (C = pods->ctr_ptr[P] - pods->ctr_ptr[0]: the outputs start at 0), req_slot / req_qty [req_cap], ent_slot / ent_qty [ent_cap]; larger
 * lists than that are SPX_ERR_ARG. */
int spx_flatten_nrt_pods_wide(const spx_pod_objects* pods, const spx_resource_classes* rc, const spx_nrt_slots* slots, int64_t req_cap, int64_t ent_cap, int64_t* n_req_out, int64_t* n_ent_out, uint8_t* qos, uint8_t* non_native, int32_t* req_ptr, uint8_t* req_slot, int64_t* req_qty, int32_t* ctr_ptr, uint8_t* ctr_kind, int32_t* ent_ptr, uint8_t* ent_slot, int64_t* ent_qty);

/* NetworkOverhead / TopologicalSort.  region_cost[n_regions*n_regions] and zone_cost[n_zones*n_zones]: -1 = no entry.
 * spx_flatten_net_keys sizes: *n_keys_out and *n_pairs_out first (pass NULL arrays), then fill
 * pod_key[P], topo_order[P], key_score_equally[n_keys], pair_ptr[n_keys+1], pair_node/pair_max_cost[n_pairs]. */
int spx_flatten_net_topo(const spx_nettopo_objects* nt, int32_t* region_cost, int32_t* zone_cost);
/* the same with int64 outputs (spx_net_topo_wide): entries of any size, only negative ones are SPX_ERR_ARG; spx_flatten_net_topo
 * refuses entries above INT32_MAX */
int spx_flatten_net_topo_wide(const spx_nettopo_objects* nt, int64_t* region_cost, int64_t* zone_cost);
int spx_flatten_net_keys(const spx_pod_objects* pods, const spx_appgroup_objects* ag, int32_t* n_keys_out, int64_t* n_pairs_out, int32_t* pod_key, int32_t* topo_order, uint8_t* key_score_equally, int32_t* pair_ptr, int32_t* pair_node, int64_t* pair_max_cost);
/* TopologicalSort.Less (topologicalsort.go:102-132) for n pairs of pod indices, from the flattened keys */
/* Coscheduling.Less over pairs (coscheduling.go:133-145): priority descending, then GetCreationTimestamp (the group's last failure
 * time if recorded, else the PodGroup's creation time if the object exists, else the pod's initial-attempt timestamp; a pod without
 * a label: that timestamp), then the pods' "namespace/name" as strings: key i is the bytes key_bytes[key_ptr[i] .. key_ptr[i+1]).
 * pod_group comes from `o` (o->n_pods entries); a[i], b[i] index pods; less_out[i] = Less(a[i], b[i]).  Host only. */
int spx_cosched_less(const spx_cosched_objects* o, const int32_t* priority, const int64_t* initial_attempt_ns, const int64_t* key_ptr, const uint8_t* key_bytes, int64_t n_pairs, const int64_t* a, const int64_t* b, uint8_t* less_out);
/* Coscheduling flatteners.  _slots: slot_res [SPX_COSCHED_MAX_SLOTS], *n_slots_out is written even when it exceeds the cap (SPX_ERR_ARG).
 * _nodes: left_base [n_slots][N], node_present [N] (nodes->n_nodes must equal o->n_nodes).  _groups: *n_steps_out is written first;
 * with step_node and step_add NULL the call only counts; otherwise req [G][n_slots], req_mask [G], step_ptr [G+1], step_node
 * [step_cap], step_add [step_cap][n_slots].  An add-back on a node that does not list the resource is 0, as getNodeResource's
 * left-over is (:457-464); assigned pods on a node that is not present are skipped with the node (:408-410). */
int spx_flatten_cosched_slots(const spx_cosched_objects* o, int32_t* n_slots_out, int32_t* slot_res);
int spx_flatten_cosched_nodes(const spx_node_objects* nodes, const spx_cosched_objects* o, int32_t n_slots, const int32_t* slot_res, int64_t* left_base, uint8_t* node_present);
int spx_flatten_cosched_groups(const spx_node_objects* nodes, const spx_cosched_objects* o, int32_t n_slots, const int32_t* slot_res, int64_t step_cap, int64_t* n_steps_out, int64_t* req, uint32_t* req_mask, int32_t* step_ptr, int32_t* step_node, int64_t* step_add);
int spx_toposort_less(const spx_pod_objects* pods, const int32_t* topo_order, int64_t n_pairs, const int64_t* a, const int64_t* b, uint8_t* less_out);
/* NodeMetadata.calculateScore per node (node_metadata.go:80-145) -> spx_node_column_soa.raw.  Node i's label or annotation value
 * (which of the two is the caller's choice, MetadataSource) is the bytes values[value_ptr[i] .. value_ptr[i+1]); found[i] = the key
 * exists.  raw_out[i] = INT64_MIN (invalidScore) for !found or a value that does not parse.
 *   SPX_NODEMETA_NUMBER: strconv.ParseFloat(s, 64)'s grammar exactly — decimal and 0x...p... hexadecimal forms, "inf" / "infinity" /
 *     "nan" in any case with an optional sign, underscores only after a base prefix, no blanks, a hexadecimal mantissa needs its p
 *     exponent, a value out of float64's range is an error.  Then int64(v), negated for SPX_NODEMETA_LOWEST (:115-119); NaN, +-Inf
 *     and |v| >= 2^63 convert to INT64_MIN as on amd64, hence invalid under either strategy.
 *   SPX_NODEMETA_TIMESTAMP: RFC 3339 as time.Parse(time.RFC3339, s) takes it (the default TimestampFormat, :221-223); age =
 *     float64(now_unix_nanos - t) / 1e9; -int64(age) for SPX_NODEMETA_NEWEST, int64(age) for SPX_NODEMETA_OLDEST (:134-144).  time.Since
 *     becomes the explicit now_unix_nanos.  A timestamp outside the years time.Duration can hold saturates as Go's Sub does.
 * SPX_ERR_ARG: a strategy that does not belong to the type, a value_ptr that is not ascending.
 * spx_flatten_nodemeta_unix: the same scores from timestamps the caller parsed (any other TimestampFormat is parsed on the Go side):
 * unix_nanos[i] and valid[i] in place of the strings. */
int spx_flatten_nodemeta(const char* values, const int64_t* value_ptr, const uint8_t* found, int64_t n_nodes, int type, int strategy, int64_t now_unix_nanos, int64_t* raw_out);
int spx_flatten_nodemeta_unix(const int64_t* unix_nanos, const uint8_t* valid, int64_t n_nodes, int strategy, int64_t now_unix_nanos, int64_t* raw_out);
/* PodState.score per node (pod_state.go:52-64): raw_out[n] = assigned pods of node n with a DeletionTimestamp minus pods nominated to
 * node n — the columns the preemption object tables carry (spx_preempt_objects: assigned pods' node and terminating flag, the
 * nominated pods' node).  SPX_ERR_ARG: a node index outside [0, n_nodes). */
int spx_flatten_podstate(int64_t n_nodes, int64_t n_assigned, const int64_t* assigned_node, const uint8_t* assigned_terminating, int64_t n_nominated, const int64_t* nominated_node, int64_t* raw_out);
/* v1qos.GetPodQOS per pod in QOSSort's numbering (SPX_QOSSORT_*), from the restatement the NRT pod flattener uses */
int spx_flatten_pod_qos(const spx_pod_objects* pods, uint8_t* qos_out);
/* QOSSort's Sort.Less (queue_sort.go:46-58) for one pair; 1 = Less(pod 1, pod 2).  Host only. */
int spx_qos_less(int32_t priority1, int qos1, int64_t ts1, int32_t priority2, int qos2, int64_t ts2);
/* spx_net_commit_soa columns: *n_entries_out first (NULL arrays), then eff_ptr[P+1], eff_key / eff_max_cost[n_entries] */
int spx_flatten_net_commit(const spx_pod_objects* pods, const spx_appgroup_objects* ag, int64_t* n_entries_out, int32_t* eff_ptr, int32_t* eff_key, int64_t* eff_max_cost);
/* pods that joined AppGroup scheduled lists since the flatten: the entries spx_update_net_placed appends (sizes first: NULL arrays) */
int spx_flatten_net_placed(const spx_pod_objects* pods, const spx_appgroup_objects* ag, int64_t n_placed, const int32_t* group, const int32_t* selector, const int32_t* node, int64_t* n_entries_out, int32_t* key_out, int32_t* node_out, int64_t* cost_out);

/* NRT preemption flow: preemption.GetNRTPostPodsEviction (pkg/noderesourcetopology/preemption/preemption.go:39-157)
 * for node `node`.  The Filter of a preemption dry-run (filter.go:205-220) is the ordinary Filter on the zone table this call
 * produces, so a batch of candidate nodes is evaluated by uploading their post-eviction availabilities (spx_upload_nrt_nodes).
 * `victims` are the victim pods; victim_qos[v] = v1qos.GetPodQOS; ctr_numa has one entry per container row of `victims`
 * (CSR order): numaplacement.EncodedInfo.NUMAAffinity -> NUMA id >= 0, -1 = no affinity, SPX_EVICT_CTR_UNKNOWN = lookup error.
 * placement_present = 0 stands for a nil EncodedInfo; placement_containers = EncodedInfo.Containers().
 * zres_avail_out receives the node's zone-resource availabilities (its slice of nrt->zres_avail, same order) after the
 * simulation, or unchanged when *code_out != SPX_EVICT_OK — the reference hands the original NRT back on every error. */
#define SPX_EVICT_OK 0
#define SPX_EVICT_NO_NRT 1                /* "NRT not found, cannot process eviction simulation"                    :41 */
#define SPX_EVICT_NO_VICTIMS 2            /* "no victims found, cannot process eviction simulation"                  :45 */
#define SPX_EVICT_NO_PLACEMENT 3          /* "numa placement info not found, cannot process eviction simulation"    :49 */
#define SPX_EVICT_NO_CONTAINERS 4         /* "no containers found in numa placement info, cannot process ..."       :53 */
#define SPX_EVICT_NOTHING_TO_ADD 5        /* "no resources to add, cannot process eviction simulation"               :62 */
#define SPX_EVICT_EXCEEDS_ALLOCATABLE 6   /* "resource release request exceeds NUMA allocatable"                     :147 */
#define SPX_EVICT_CTR_UNKNOWN (-2)
int spx_nrt_post_eviction(const spx_nrt_objects* nrt, const spx_resource_classes* rc, int64_t node, const spx_pod_objects* victims, const uint8_t* victim_qos, const int32_t* ctr_numa, int32_t placement_present, int32_t placement_containers, int64_t* zres_avail_out, int32_t* code_out);

/* CapacityScheduling: sizes are pod_req[P*8], pod_req_present[P]; the per-namespace arrays [NS*8] / [NS];
 * agg_*[8] / [1]; other_nominated[NS*8]: nominated requests of OTHER namespaces whose quota is not over min
 * (capacity_scheduling.go:248-250), i.e. total minus the namespace's own share; nom_* are the nominated pods
 * grouped by namespace (nom_ptr[NS+1]); n_nominated entries. */
int spx_flatten_quota(const spx_pod_objects* pods, const spx_resource_classes* rc, const spx_quota_objects* q, int32_t* pod_ns, int32_t* pod_priority, int64_t* pod_req, uint8_t* pod_req_present, int64_t* agg_used, uint8_t* agg_used_present, int64_t* agg_min, uint8_t* agg_min_present, int64_t* other_nominated, uint8_t* other_nominated_present, int32_t* nom_ptr, int32_t* nom_priority, int64_t* nom_pending_index, int64_t* nom_req, uint8_t* nom_req_present);

/* Preemption dry run, host side.  spx_flatten_preempt_nodes: node objects + spx_preempt_objects -> the columns of
 * spx_preempt_nodes_soa.  Requests are formed as spx_flatten_quota forms them (q supplies the scalar slots); pod_fit_req is the same
 * vector with slot 3 = 1.  *n_pods_out / *n_nom_out / *n_pdb_out are written first; called with every output column NULL the call
 * only counts (and still checks).  Columns: present [N], allocatable / requested [N][8], pod_ptr / nom_ptr / pdb_ptr [N+1], the pod
 * columns [*n_pods_out] (pod_src: index of the table's pod in `o->assigned`), the nominated columns [*n_nom_out], pdb_allowed
 * [*n_pdb_out].  Pods on an absent node, or with node -1, are left out.  SPX_ERR_ARG with *bad_out = the node (or -1 - the assigned
 * pod's index for a request it cannot hold): more than SPX_PREEMPT_MAX_NODE_PODS pods or SPX_PREEMPT_MAX_NODE_PDBS distinct PDBs on
 * a node, a request in a scalar outside the quota's slots, a negative request, a slot whose absolute values sum to 2^62 or more. */
int spx_flatten_preempt_nodes(const spx_node_objects* nodes, const spx_resource_classes* rc, const spx_quota_objects* q, const spx_preempt_objects* o, int64_t* n_pods_out, int64_t* n_nom_out, int64_t* n_pdb_out, int64_t* bad_out, uint8_t* present, int64_t* allocatable, int64_t* requested, int32_t* pod_ptr, int32_t* pod_src, int32_t* pod_priority, int64_t* pod_start, int32_t* pod_ns, int64_t* pod_fit_req, int64_t* pod_quota_req, uint8_t* pod_quota_req_present, uint8_t* pod_flags, uint32_t* pod_pdb_mask, int32_t* pod_hi_order, int32_t* nom_ptr, int32_t* nom_priority, int64_t* nom_fit_req, int64_t* nom_pending_row, int32_t* pdb_ptr, int32_t* pdb_allowed);
/* the checks spx_upload_preempt_nodes applies, host only: SPX_OK, or SPX_ERR_ARG with *bad_node_out = the first offending node */
int spx_preempt_check(const spx_preempt_nodes_soa* t, int64_t* bad_node_out);
/* The side table of CapacityScheduling's sequential loop: spx_preempt_nominated_quota_soa's columns for the nominated pods of
 * `o`, in the record order of spx_flatten_preempt_nodes' table (node by node, the objects' order within a node; pods nominated to an
 * absent node, or to node -1, are left out).  n_nom: that table's nominated count (*n_nom_out); SPX_ERR_ARG when it differs.  nom_src
 * (may be NULL) [n_nom]: index of each record's pod in o->nominated.  ns: the object's namespace, whether it has a quota or not;
 * quota_req / quota_req_present: computePodResourceRequest (:865-882) as spx_flatten_quota forms it.  Host only. */
int spx_flatten_preempt_nominated_quota(const spx_node_objects* nodes, const spx_resource_classes* rc, const spx_quota_objects* q, const spx_preempt_objects* o, int64_t n_nom, int32_t* nom_src, int32_t* ns, int64_t* quota_req, uint8_t* quota_req_present);
/* preemptor.PodEligibleToPreemptOthers (:409-484) for n pods: ns / priority / preempt_never of the pod, nominated_node (-1 = none, an
 * absent node answers eligible as a nil NodeInfo does), nominated_unresolvable = the nominated node's Filter status code was
 * UnschedulableAndUnresolvable, more_than_min = usedOverMinWith(nominatedPodsReqInEQWithPodReq) of the pod (read only when its
 * namespace has a quota), over_min [n_namespaces] = usedOverMin() of each quota.  Host only. */
int spx_preempt_eligible(const spx_preempt_nodes_soa* t, const spx_quota_objects* q, const uint8_t* over_min, int64_t n, const int32_t* ns, const int32_t* priority, const uint8_t* preempt_never, const int64_t* nominated_node, const uint8_t* nominated_unresolvable, const uint8_t* more_than_min, uint8_t* eligible_out);

/* PreemptionToleration, host side.  The PriorityClasses the assigned pods name: present = the lister has the class, value = its
 * Value, and the texts of the annotations preemption-toleration.scheduling.x-k8s.io/minimum-preemptable-priority and
 * .../toleration-seconds (NULL = the annotation is absent; NULL columns = no class has it). */
typedef struct spx_priority_classes {
  int32_t n_classes;
  const uint8_t* present;
  const int32_t* value;
  const char* const* minimum_preemptable_priority;
  const char* const* toleration_seconds;
} spx_priority_classes;
/* parsePreemptionTolerationPolicy (preemption_toleration_policy.go:55-83) and the part of ExemptedFromPreemption that does not depend
 * on the preemptor, per assigned pod IN OBJECT ORDER (the `assigned` pods of spx_preempt_objects): pod_class = index into the class
 * table, -1 = empty PriorityClassName; pod_scheduled = a PodScheduled condition with status True exists, pod_scheduled_at_ns its
 * LastTransitionTime.  pod_src [n_pods] = spx_flatten_preempt_nodes' column: the outputs (the columns of spx_preempt_toleration_soa,
 * [n_pods] each) are in the node table's CSR order.  strconv.ParseInt(s, 10, bits) is restated here: one optional sign, then digits only,
 * within the range of the bit size.  An absent minimum-preemptable-priority is Value + 1 in int32 arithmetic (2^31-1 gives -2^31).
 * SPX_ERR_ARG: a class index outside [-1, n_classes), a pod_src outside [0, n_assigned). */
int spx_flatten_preempt_toleration(const spx_priority_classes* classes, int64_t n_assigned, const int32_t* pod_class, const uint8_t* pod_scheduled, const int64_t* pod_scheduled_at_ns, int64_t n_pods, const int32_t* pod_src, int32_t* min_preemptable, int64_t* exempt_until_ns, uint8_t* flags);
/* PreemptionToleration.PodEligibleToPreemptOthers (preemption_toleration.go:339-364) for n pods: false for PreemptNever; true when the
 * nominated node (-1 = none) was UnschedulableAndUnresolvable or is absent; false when a terminating pod of lower priority sits on it;
 * else true.  Reads pod_ptr, pod_priority, pod_flags & SPX_PREEMPT_POD_TERMINATING and present.  Host only. */
int spx_preempt_toleration_eligible(const spx_preempt_nodes_soa* t, int64_t n, const int32_t* priority, const uint8_t* preempt_never, const int64_t* nominated_node, const uint8_t* nominated_unresolvable, uint8_t* eligible_out);
/* The side table of spx_upload_preempt_nrt from the objects (host/flatten_preempt_nrt.cc).  nodes / nrt / slots as
 * spx_flatten_nrt_nodes takes them (nrt->zres_allocatable is required); o->assigned are the pods of the preemption tables (their QoS
 * class is computed here) and ctr_numa holds one entry per container of o->assigned in CSR order, in the encoding of
 * spx_nrt_post_eviction (NUMA id, -1 = no affinity, SPX_EVICT_CTR_UNKNOWN); placement_present / placement_containers [N] per node.
 * pod_src [n_pods] = spx_flatten_preempt_nodes' column: the per-pod outputs are in the node table's CSR order.  The per-pod release rule
 * is spx_nrt_post_eviction's (one copy, host/nrt_release.hpp): for any set of victims of one node, available + the sum of their releases
 * and the three verdicts (nothing to add / exceeds allocatable / ok) are what that function gives.  rel_cap: the capacity of the rel_*
 * arrays; *n_rel_out receives the count.  SPX_ERR_ARG with *bad_out = the node (>= 0) or -1 - the assigned pod: more than 8 slots or
 * zones, a zone whose name parses to a NUMA id but that the Filter does not list (not of type Node, or an id above 63), a resource
 * listed twice in a zone, available > allocatable, a negative release, a node's releases summing to 2^62 or more in a slot, rel_cap too
 * small; *bad_out = INT64_MIN for a NULL or inconsistent argument.  The preemptors' records are spx_flatten_nrt_pods' on the same slots.
 * spx_flatten_preempt_nrt_check: the limits that can be read off the flattened table (what spx_upload_preempt_nrt runs first, before
 * it adds up a node's releases against the node table's CSR): *kind_out = 0 and SPX_OK, or SPX_ERR_ARG with 1 = node *bad_out, 2 =
 * assigned pod *bad_out (CSR order), 3 = pod row *bad_out, 4 = a NULL column or sizes that contradict each other. */
int spx_flatten_preempt_nrt(const spx_node_objects* nodes, const spx_nrt_objects* nrt, const spx_resource_classes* rc, const spx_nrt_slots* slots, const spx_preempt_objects* o, const int32_t* ctr_numa, const uint8_t* placement_present, const int32_t* placement_containers, int64_t n_pods, const int32_t* pod_src, int64_t rel_cap, int64_t* n_rel_out, int64_t* bad_out, uint8_t* node_flags, uint8_t* n_zones, uint8_t* zone_id, uint8_t* zone_present, uint8_t* node_present, int64_t* zone_avail, int64_t* zone_headroom, uint8_t* pod_contributes, int32_t* rel_ptr, uint8_t* rel_zone, uint8_t* rel_slot, int64_t* rel_qty);
int spx_flatten_preempt_nrt_check(const spx_preempt_nrt_soa* t, int32_t* kind_out, int64_t* bad_out);

/* ------------------------------------------------------------------ wire format -> object tables (first slice)
 *
 * NodeResourceTopology objects as the API server serves them (JSON of topology.node.k8s.io/v1alpha2; schema = the reference's
 * manifests/crds/topology.node.k8s.io_noderesourcetopologies.yaml) decoded into the spx_nrt_objects columns, replacing the
 * informer-cache walk of pluginhelpers.go:105-161 / nodeconfig/topologymanager.go:78-162 on the Go side.  The handle owns the
 * tables; pointers returned by the accessors stay valid until the next spx_ingest_nrt_json / spx_ingest_destroy.  node_names fixes
 * the node order of the snapshot (objects of other names are counted and skipped); resource_names pre-seeds the resource
 * interner (ids >= SPX_RES_FIRST_DYNAMIC in that order) so that pod tables built elsewhere share the id space.  `fresh` is 1 for
 * every node and the assumed-pod lists are empty: both are the NRT cache's verdict, which stays with the caller. */
typedef struct spx_ingest spx_ingest;
int spx_ingest_create(const char* const* node_names, int64_t n_nodes, const char* const* resource_names, int32_t n_resource_names, spx_ingest** out);
int spx_ingest_destroy(spx_ingest* h);
const char* spx_ingest_error(const spx_ingest* h);
/* json: one object, a List ("items") or an array; may be called repeatedly — a later object replaces an earlier one of the same name */
int spx_ingest_nrt_json(spx_ingest* h, const char* json, int64_t len, int64_t* n_objects_out, int64_t* n_unknown_out);
const spx_nrt_objects* spx_ingest_nrt_objects(const spx_ingest* h);
const spx_resource_classes* spx_ingest_resource_classes(const spx_ingest* h);
int32_t spx_ingest_resource_id(const spx_ingest* h, const char* name);
/* v1.Node objects -> spx_node_objects in the handle's node order (by metadata.name): status.allocatable / capacity in canonical
 * units, the scalar resources framework.Resource.Add keeps, topology.kubernetes.io/region and /zone label values interned
 * (-1 when absent or empty).  v1.Pod objects -> spx_pod_objects, appended in document order until spx_ingest_pods_reset: init
 * containers first (restartPolicy Always = SPX_CTR_SIDECAR) then app containers, requests / limits / overhead lists in document
 * order, spec.priority, metadata.creationTimestamp as queue timestamp (microseconds), namespace and the two AppGroup labels
 * (appgroup.diktyo.x-k8s.io, appgroup.diktyo.x-k8s.io.workload) interned, -1 when absent.  Name id spaces (kind: 0 region, 1 zone,
 * 2 namespace, 3 AppGroup, 4 workload selector) grow in first-seen order; spx_ingest_seed_names fixes them beforehand (workload
 * selectors are the exception: see spx_ingest_appgroups_json). */
int spx_ingest_nodes_json(spx_ingest* h, const char* json, int64_t len, int64_t* n_objects_out, int64_t* n_unknown_out);
int spx_ingest_pods_json(spx_ingest* h, const char* json, int64_t len, int64_t* n_objects_out);
int spx_ingest_pods_reset(spx_ingest* h);
const spx_node_objects* spx_ingest_node_objects(const spx_ingest* h);
const spx_pod_objects* spx_ingest_pod_objects(const spx_ingest* h);
int spx_ingest_seed_names(spx_ingest* h, int32_t kind, const char* const* names, int32_t n);
int32_t spx_ingest_name_id(const spx_ingest* h, int32_t kind, const char* name);
/* AppGroup CRs (appgroup.diktyo.x-k8s.io/v1alpha1) -> spx_appgroup_objects, row g = the group whose name id (kind 3) is g — the id
 * the pod table's appgroup column carries, whatever order CRs and pods arrive in; a later CR of the same name replaces the earlier one: spec.workloads[].workload.selector, their dependencies[].{workload.selector, maxNetworkCost}, status.topologyOrder[] as
 * written.  Workload selector ids always preserve the lexicographic order of the selector strings: whenever a call (AppGroups or pods)
 * leaves the table out of order it is re-sorted and the pod table's selector column renumbered — query ids (spx_ingest_name_id)
 * after the last ingestion call, not before.  The scheduled-pods list is not part of the CR and stays empty.
 * One NetworkTopology CR (networktopology.diktyo.x-k8s.io/v1alpha1) -> spx_nettopo_objects for the weights set weights_name
 * (populateCostMap, networkoverhead.go:448-497); region / zone names share the id spaces of the node table (kinds 0 and 1). */
int spx_ingest_appgroups_json(spx_ingest* h, const char* json, int64_t len, int64_t* n_objects_out);
const spx_appgroup_objects* spx_ingest_appgroup_objects(const spx_ingest* h);
int spx_ingest_nettopo_json(spx_ingest* h, const char* json, int64_t len, const char* weights_name);
const spx_nettopo_objects* spx_ingest_nettopo_objects(const spx_ingest* h);
/* ElasticQuota CRs (scheduling.x-k8s.io/v1alpha1) -> spx_quota_objects indexed by the given namespace list (which also seeds the
 * namespace ids of the pod table): spec.min / spec.max with newElasticQuotaInfo's replacements for nil lists (elasticquota.go:70-76),
 * `used` from status.used; quotas of other namespaces are counted and skipped.  The nominated-pod list (capacity_scheduling.go:231-253 walks
 * PodNominator.NominatedPodsForNode over the snapshot's nodes) is rebuilt from the handle's pod table on every pod / quota call: the
 * pods whose status.nominatedNodeName names a node of the snapshot, nom_pending_index = the pod's own row (the reference skips the pod
 * under evaluation by UID).
 * NULL from the accessor until the first successful call. */
int spx_ingest_quota_json(spx_ingest* h, const char* json, int64_t len, const char* const* namespaces, int32_t n_namespaces, int64_t* n_objects_out, int64_t* n_unknown_out);
const spx_quota_objects* spx_ingest_quota_objects(const spx_ingest* h);
/* The load-watcher response trimaran's Collector polls (collector.go:139-150) -> spx_metrics_objects in the handle's node order.
 * The struct it decodes into (watcher.WatcherMetrics, github.com/paypal/load-watcher v0.2.4) is not vendored in the reference and
 * the reference holds no golden document: field names are the struct's published json tags, decoding rules are encoding/json's
 * (case-insensitive member names, unknown members ignored) — PARITY UNPINNED.  A successful call replaces the whole
 * metrics snapshot; a failed one keeps the previous one, like the Collector.  n_nodes_out counts the entries of
 * data.NodeMetricsMap, n_unknown_out those whose name is not in the handle's node list.  NULL from the accessor until the first
 * successful call. */
int spx_ingest_metrics_json(spx_ingest* h, const char* json, int64_t len, int64_t* n_nodes_out, int64_t* n_unknown_out);
const spx_metrics_objects* spx_ingest_metrics_objects(const spx_ingest* h);
/* resource.Quantity text -> canonical int64: MilliValue() when milli != 0 (cpu), Value() otherwise; both round up */
int spx_ingest_quantity(const char* text, int32_t milli, int64_t* out);

#ifdef __cplusplus
}
#endif
#endif /* SPX_H */
