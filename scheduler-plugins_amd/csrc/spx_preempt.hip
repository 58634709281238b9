// spx_preempt.hip — the preemption dry runs' entry points (include/spx.h: spx_upload_preempt_*, spx_preempt_dry_run,
// spx_preempt_sequential, spx_preempt_toleration_dry_run, spx_preempt_toleration_sequential, spx_upload_preempt_nrt,
// spx_preempt_toleration_nrt_dry_run, spx_preempt_nrt_dry_run, spx_preempt_toleration_nrt_sequential, spx_preempt_nrt_sequential,
// spx_fetch_preempt_*): table checks and uploads, the launches of kernels_preempt.hip, kernels_preempt_seq.hip, kernels_ptol.hip,
// kernels_ptol_seq.hip, kernels_ptol_nrt.hip, kernels_preempt_nrt.hip, kernels_ptol_nrt_seq.hip and kernels_preempt_nrt_seq.hip, and the
// fetches, which serve whichever of the eight ran last.
// State: spx_engine.h; of the shared helpers it takes fail, ensure, upload, set_nodes and set_pods (spx_state.hip).
#include "spx_engine.h"

#include <algorithm>
#include <cstring>
#include <type_traits>
#include <unordered_map>

namespace {

constexpr int S = SPX_QUOTA_SLOTS;
constexpr int64_t kSumLimit = int64_t{1} << 62;

// The first node the device cannot take, or -1: the limits of include/spx.h, and everything the kernels index with.
int64_t preempt_bad_node(const spx_preempt_nodes_soa* t, std::string* why) {
  auto bad = [&](int64_t n, const char* text) {
    if (why) *why = text;
    return n;
  };
  const int64_t N = t->n_nodes;
  if (t->pod_ptr[0] != 0 || t->nom_ptr[0] != 0 || t->pdb_ptr[0] != 0) return bad(0, "a CSR does not start at 0");
  // per slot: sum of |values| over everything a cell can add up (one node's side at a time is what a lane sums, but the bound is
  // kept global: it is the one spx_cosched_check states)
  uint64_t total[S] = {0};
  auto account = [&](const int64_t* v) {
    for (int s = 0; s < S; ++s) {
      if (v[s] < 0) return false;
      total[s] += static_cast<uint64_t>(v[s]);
      if (total[s] >= static_cast<uint64_t>(kSumLimit)) return false;
    }
    return true;
  };
  std::vector<uint8_t> seen(SPX_PREEMPT_MAX_NODE_PODS);
  for (int64_t n = 0; n < N; ++n) {
    const int64_t p0 = t->pod_ptr[n], p1 = t->pod_ptr[n + 1], L = p1 - p0;
    if (L < 0 || t->nom_ptr[n + 1] < t->nom_ptr[n] || t->pdb_ptr[n + 1] < t->pdb_ptr[n]) return bad(n, "a CSR pointer decreases");
    if (L > SPX_PREEMPT_MAX_NODE_PODS) return bad(n, "more than SPX_PREEMPT_MAX_NODE_PODS pods on the node");
    const int n_pdb = t->pdb_ptr[n + 1] - t->pdb_ptr[n];
    if (n_pdb > SPX_PREEMPT_MAX_NODE_PDBS) return bad(n, "more than SPX_PREEMPT_MAX_NODE_PDBS PDBs among the node's pods");
    if (!account(t->allocatable + n * S) || !account(t->requested + n * S)) return bad(n, "a negative quantity, or a slot whose values sum to 2^62 or more");
    std::fill(seen.begin(), seen.begin() + L, 0);
    for (int64_t j = p0; j < p1; ++j) {
      if (!account(t->pod_fit_req + j * S) || !account(t->pod_quota_req + j * S)) return bad(n, "a negative request, or a slot whose values sum to 2^62 or more");
      if (n_pdb < 32 && (t->pod_pdb_mask[j] >> n_pdb)) return bad(n, "a PDB bit outside the node's PDBs");
      if (j > p0 && (t->pod_priority[j] < t->pod_priority[j - 1] || (t->pod_priority[j] == t->pod_priority[j - 1] && t->pod_start[j] > t->pod_start[j - 1])))
        return bad(n, "the node's pods are not in walk order (least important first)");
      const int32_t h = t->pod_hi_order[j];
      if (h < 0 || h >= L || seen[h]) return bad(n, "pod_hi_order is no permutation of the node's positions");
      seen[h] = 1;
    }
    for (int64_t k = 1; k < L; ++k) {  // most important first, ties by position
      const int64_t x = p0 + t->pod_hi_order[p0 + k - 1], y = p0 + t->pod_hi_order[p0 + k];
      const bool ordered = t->pod_priority[x] > t->pod_priority[y] ||
                           (t->pod_priority[x] == t->pod_priority[y] && (t->pod_start[x] < t->pod_start[y] || (t->pod_start[x] == t->pod_start[y] && x < y)));
      if (!ordered) return bad(n, "pod_hi_order is not most important first with ties by position");
    }
    for (int64_t j = t->nom_ptr[n]; j < t->nom_ptr[n + 1]; ++j)
      if (!account(t->nom_fit_req + j * S)) return bad(n, "a negative request, or a slot whose values sum to 2^62 or more");
  }
  return -1;
}

bool preempt_columns_present(const spx_preempt_nodes_soa* t) {
  if (!t || t->n_nodes <= 0 || !t->present || !t->allocatable || !t->requested || !t->pod_ptr || !t->nom_ptr || !t->pdb_ptr) return false;
  const int64_t A = t->pod_ptr[t->n_nodes], M = t->nom_ptr[t->n_nodes], B = t->pdb_ptr[t->n_nodes];
  if (A < 0 || M < 0 || B < 0) return false;
  if (A > 0 && (!t->pod_priority || !t->pod_start || !t->pod_ns || !t->pod_fit_req || !t->pod_quota_req || !t->pod_quota_req_present || !t->pod_flags ||
                !t->pod_pdb_mask || !t->pod_hi_order))
    return false;
  if (M > 0 && (!t->nom_priority || !t->nom_fit_req || !t->nom_pending_row)) return false;
  return B == 0 || t->pdb_allowed;
}

spx::PreemptArgs preempt_args(spx_engine* e) {
  spx::PreemptArgs a{};
  a.n_nodes = e->n_nodes;
  a.n_rows = e->pre_n_rows;
  a.row_stride = e->pre_row_stride;
  a.rows = static_cast<const int64_t*>(e->d_pre_rows.p);
  a.node_mask = e->pre_has_mask ? static_cast<const uint8_t*>(e->d_pre_mask.p) : nullptr;
  a.n_namespaces = e->q_n_namespaces;
  a.pod_ns = static_cast<const int32_t*>(e->d_q_pod_ns.p);
  a.pod_priority = static_cast<const int32_t*>(e->d_q_pod_prio.p);
  a.pod_req = static_cast<const int64_t*>(e->d_q_pod_req.p);
  a.pod_req_present = static_cast<const uint8_t*>(e->d_q_pod_reqp.p);
  a.has_quota = static_cast<const uint8_t*>(e->d_q_has.p);
  a.used = static_cast<const int64_t*>(e->d_q_used.p);
  a.used_present = static_cast<const uint8_t*>(e->d_q_usedp.p);
  a.min = static_cast<const int64_t*>(e->d_q_min.p);
  a.min_present = static_cast<const uint8_t*>(e->d_q_minp.p);
  a.max = static_cast<const int64_t*>(e->d_q_max.p);
  a.max_present = static_cast<const uint8_t*>(e->d_q_maxp.p);
  std::memcpy(a.agg_used, e->q_agg_used, sizeof a.agg_used);
  std::memcpy(a.agg_min, e->q_agg_min, sizeof a.agg_min);
  a.agg_used_present = e->q_agg_used_present;
  a.agg_min_present = e->q_agg_min_present;
  a.other_nominated = static_cast<const int64_t*>(e->d_q_other.p);
  a.other_nominated_present = static_cast<const uint8_t*>(e->d_q_otherp.p);
  a.q_nom_ptr = static_cast<const int32_t*>(e->d_q_nom_ptr.p);
  a.q_nom_priority = static_cast<const int32_t*>(e->d_q_nom_prio.p);
  a.q_nom_pending_index = static_cast<const int64_t*>(e->d_q_nom_idx.p);
  a.q_nom_req = static_cast<const int64_t*>(e->d_q_nom_req.p);
  a.q_nom_req_present = static_cast<const uint8_t*>(e->d_q_nom_reqp.p);
  a.pre_fit = static_cast<const int64_t*>(e->d_pre_pod_fit.p);
  a.nodes = static_cast<const spx::PreemptNode*>(e->d_pre_nodes.p);
  a.pods = static_cast<spx::PreemptPod*>(e->d_pre_podrec.p);
  a.noms = static_cast<const spx::PreemptNom*>(e->d_pre_noms.p);
  a.pdb_allowed = static_cast<const int32_t*>(e->d_pre_pdb_allowed.p);
  a.row_rec = static_cast<int64_t*>(e->d_pre_rec.p);
  a.cells = static_cast<spx::PreemptCell*>(e->d_pre_cells.p);
  a.pick = static_cast<const int32_t*>(e->d_pre_pick.p);
  return a;
}

spx::PtolArgs ptol_args(spx_engine* e) {
  spx::PtolArgs a{};
  a.n_nodes = e->n_nodes;
  a.n_rows = e->pre_n_rows;
  a.row_stride = e->pre_row_stride;
  a.now = e->ptol_now;
  a.rows = static_cast<const int64_t*>(e->d_pre_rows.p);
  a.row_meta = static_cast<const int64_t*>(e->d_ptol_meta.p);
  a.node_mask = e->pre_has_mask ? static_cast<const uint8_t*>(e->d_pre_mask.p) : nullptr;
  a.pre_fit = static_cast<const int64_t*>(e->d_pre_pod_fit.p);
  a.nodes = static_cast<const spx::PreemptNode*>(e->d_pre_nodes.p);
  a.pods = static_cast<const spx::PreemptPod*>(e->d_pre_podrec.p);
  a.tol = static_cast<const spx::PtolPod*>(e->d_ptol_pods.p);
  a.noms = static_cast<const spx::PreemptNom*>(e->d_pre_noms.p);
  a.pdb_allowed = static_cast<const int32_t*>(e->d_pre_pdb_allowed.p);
  a.row_rec = static_cast<int64_t*>(e->d_ptol_rec.p);
  a.cells = static_cast<spx::PreemptCell*>(e->d_pre_cells.p);
  return a;
}

// The NRT side table and the preemptors' columns, for either plugin's walk.
spx::NrtRefitArgs nrt_refit_args(spx_engine* e) {
  spx::NrtRefitArgs a{};
  a.n_res = e->pnrt_n_res, a.mode = e->pnrt_mode, a.max_zones = e->pnrt_max_zones, a.slot_flags = e->pnrt_slot_flags;
  a.nodes = static_cast<const spx::PnrtNode*>(e->d_pnrt_nodes.p);
  a.contributes = static_cast<const uint8_t*>(e->d_pnrt_contrib.p);
  a.rel_ptr = static_cast<const int32_t*>(e->d_pnrt_rel_ptr.p);
  a.rel = static_cast<const spx::PnrtRel*>(e->d_pnrt_rel.p);
  const char* const pods = static_cast<const char*>(e->d_pnrt_pods.p);
  auto col = [&](int k) { return reinterpret_cast<const uint8_t*>(pods + e->pnrt_pod_off[k]); };
  a.qos = col(0), a.non_native = col(1), a.n_ctr = col(2), a.ctr_kind = col(3), a.ctr_present = col(4), a.pod_present = col(5);
  a.ctr_req = reinterpret_cast<const int64_t*>(col(6)), a.pod_req = reinterpret_cast<const int64_t*>(col(7));
  a.nrt_rec = static_cast<int64_t*>(e->d_pnrt_rec.p);
  return a;
}

spx::PnrtArgs pnrt_args(spx_engine* e) { return {ptol_args(e), nrt_refit_args(e)}; }
spx::CnrtArgs cnrt_args(spx_engine* e) { return {preempt_args(e), nrt_refit_args(e)}; }

// What either pick kernel reads, whichever plugin wrote the cells.
spx::PickArgs pick_args(spx_engine* e) {
  return {e->n_nodes, e->pre_n_rows, e->pre_row_stride, 0, static_cast<const spx::PreemptCell*>(e->d_pre_cells.p), static_cast<int32_t*>(e->d_pre_pick.p)};
}

int preempt_results(spx_engine* e, int64_t i_begin, int64_t i_end) {
  if (!e->pre_valid) return fail(e, SPX_ERR_STATE, "no preemption dry run since the last upload of its tables");
  if (i_begin < 0 || i_end > e->pre_n_rows || i_begin > i_end) return fail(e, SPX_ERR_ARG, "preemption rows: index range outside the row list of the dry run");
  return SPX_OK;
}

// Every entry of a dry run's row list is a row of the batch.
int rows_in_batch(spx_engine* e, const std::string& who, const int64_t* rows, int64_t n_rows) {
  for (int64_t i = 0; i < n_rows; ++i)
    if (rows[i] < 0 || rows[i] >= e->n_pods) return fail(e, SPX_ERR_ARG, who + ": rows[" + std::to_string(i) + "] is no row of the batch");
  return SPX_OK;
}

// What the two toleration entry points check before anything moves: state first, then the arguments.
int ptol_check(spx_engine* e, const std::string& who, const int64_t* rows, int64_t n_rows, const int32_t* priority, const uint8_t* preempt_never, int64_t now_ns) {
  if (!e->pre_nodes || !e->pre_pods) return fail(e, SPX_ERR_STATE, who + ": spx_upload_preempt_nodes / spx_upload_preempt_pods not called");
  if (!e->ptol_table) return fail(e, SPX_ERR_STATE, who + ": no spx_upload_preempt_toleration since the last spx_upload_preempt_nodes");
  if (!rows || n_rows <= 0 || !priority || !preempt_never) return fail(e, SPX_ERR_ARG, who + ": empty row list");
  if (now_ns == INT64_MAX) return fail(e, SPX_ERR_ARG, who + ": now_ns == INT64_MAX (an exempt_until_ns of INT64_MAX means for ever)");
  return rows_in_batch(e, who, rows, n_rows);
}

struct Staged {  // a device buffer a run needs at `bytes`; filled from src when that is set
  DevBuf* buf;
  size_t bytes;
  const void* src;
};

// What every dry run stages once its arguments are checked: the limits, the memory pre-check, then the row list and the node mask on the
// device, the row record (`fields` int64 columns), the cells, the pick and `more` sized or uploaded; then the engine's view of the run.
int preempt_stage(spx_engine* e, const std::string& who, const int64_t* rows, int64_t n_rows, const uint8_t* node_mask, DevBuf& rec, int fields, const std::vector<Staged>& more) {
  SPX_HIP(e, hipSetDevice(e->device));
  const size_t N = static_cast<size_t>(e->n_nodes), R = static_cast<size_t>(spx::round_up(n_rows, 64));
  if (R > (size_t{1} << 24) || N > (size_t{1} << 31)) return fail(e, SPX_ERR_ARG, who + ": more than 2^24 rows");
  std::vector<Staged> want = {{&e->d_pre_rows, static_cast<size_t>(n_rows) * 8, rows},
                              {&rec, R * static_cast<size_t>(fields) * 8, nullptr},
                              {&e->d_pre_cells, N * R * sizeof(spx::PreemptCell), nullptr},
                              {&e->d_pre_pick, R * 5 * 4, nullptr}};
  want.insert(want.end(), more.begin(), more.end());
  if (node_mask) want.push_back({&e->d_pre_mask, static_cast<size_t>(n_rows) * N, node_mask});
  {  // refuse what cannot fit instead of failing in hipMalloc: what has to grow against what is free
    size_t free_b = 0, total_b = 0, grow = 0;
    SPX_HIP(e, hipMemGetInfo(&free_b, &total_b));
    for (const Staged& w : want)
      if (w.bytes > w.buf->bytes) grow += w.bytes, free_b += w.buf->bytes;  // ensure() frees the old allocation first
    if (grow > free_b)
      return fail(e, SPX_ERR_ARG, who + ": " + std::to_string(n_rows) + " rows x " + std::to_string(N) + " nodes need " + std::to_string(grow) +
                                      " bytes of cell records, the device has " + std::to_string(free_b) + " free: split the row list");
  }
  e->pre_valid = e->pre_nrt = false;
  for (const Staged& w : want)
    if (int rc = w.src ? upload(e, *w.buf, w.src, w.bytes) : ensure(e, *w.buf, w.bytes)) return rc;
  SPX_HIP(e, hipStreamSynchronize(e->stream));  // what was uploaded is only borrowed for the call
  e->pre_has_mask = node_mask != nullptr;
  e->pre_n_rows = n_rows;
  e->pre_row_stride = static_cast<int64_t>(R);
  return SPX_OK;
}

// The toleration runs' staging: preempt_stage with the meta column of the row list (priority, PreemptNever, and "not eligible" where
// `eligible` is given and 0) among the uploads.
int ptol_stage(spx_engine* e, const std::string& who, const int64_t* rows, int64_t n_rows, const int32_t* priority, const uint8_t* preempt_never, const uint8_t* eligible,
               int64_t now_ns, const uint8_t* node_mask, std::vector<Staged> more) {
  std::vector<int64_t> meta(static_cast<size_t>(n_rows));
  for (int64_t i = 0; i < n_rows; ++i)
    meta[i] = static_cast<int64_t>(static_cast<uint32_t>(priority[i])) | (preempt_never[i] ? int64_t{1} << 32 : 0) | (eligible && !eligible[i] ? int64_t{1} << 33 : 0);
  more.push_back({&e->d_ptol_meta, meta.size() * 8, meta.data()});
  if (int rc = preempt_stage(e, who, rows, n_rows, node_mask, e->d_ptol_rec, spx::kPtolRowFields, more)) return rc;
  e->pre_toleration = true;
  e->ptol_now = now_ns;
  return SPX_OK;
}

struct SeqStaged {
  spx::SeqOverlay o;
  std::vector<char*> extra;     // the caller's regions of the carve, in the order it asked for them
  int32_t n_dirty;              // 1 + the most uploaded nominations any one row of the list has
  const int32_t* row_nom_node;  // parallel to o.row_nom: the node each record sits on
};

// What the two sequential loops stage once their state and arguments are checked.  A row is attempted once; the uploaded nominations
// each row came with (T4) become a CSR over the row list, [ptr | record | node of the record]; the overlay, the stored victim sets and
// the regions of extra_bytes(n_dirty) are carved from one allocation; stage(more) is the caller's staging with these two buffers
// among `more`; then the overlay is addressed and its zero and -1 parts are set.
template <class ExtraBytes, class Stage>
int seq_stage(spx_engine* e, const std::string& who, const int64_t* rows, int64_t n_rows, ExtraBytes extra_bytes, Stage stage, SeqStaged* out) {
  std::unordered_map<int64_t, int64_t> at;  // pod row -> its index in the list
  for (int64_t i = 0; i < n_rows; ++i)
    if (!at.emplace(rows[i], i).second) return fail(e, SPX_ERR_ARG, who + ": rows[" + std::to_string(i) + "] is listed twice");
  const int64_t N = e->n_nodes, M = e->h_pre_nom_ptr.back();
  std::vector<int32_t> csr(static_cast<size_t>(n_rows) + 1, 0);
  for (int64_t j = 0; j < M; ++j) {
    const auto it = at.find(e->h_pre_nom_row[j]);
    if (it != at.end()) ++csr[it->second + 1];
  }
  out->n_dirty = 1;
  for (int64_t i = 0; i < n_rows; ++i) out->n_dirty = std::max(out->n_dirty, 1 + csr[i + 1]), csr[i + 1] += csr[i];
  const size_t own = static_cast<size_t>(csr[n_rows]);
  std::vector<int32_t> fill(csr.begin(), csr.end() - 1);
  csr.resize(static_cast<size_t>(n_rows) + 1 + 2 * own);
  for (int64_t n = 0; n < N; ++n)  // node by node: the records of a row in ascending record index
    for (int32_t j = e->h_pre_nom_ptr[n]; j < e->h_pre_nom_ptr[n + 1]; ++j) {
      const auto it = at.find(e->h_pre_nom_row[j]);
      if (it == at.end()) continue;
      const size_t k = static_cast<size_t>(fill[it->second]++);
      csr[n_rows + 1 + k] = j, csr[n_rows + 1 + own + k] = static_cast<int32_t>(n);
    }
  const size_t R = static_cast<size_t>(spx::round_up(n_rows, 64));
  constexpr size_t kSetBytes = SPX_PREEMPT_MAX_NODE_PODS / 8;
  size_t total = 0;
  auto carve = [&](size_t bytes) {
    const size_t o = total;
    total += static_cast<size_t>(spx::round_up(static_cast<int64_t>(bytes), 256));
    return o;
  };
  const size_t o_gone = carve(static_cast<size_t>(N) * kSetBytes), o_clear = carve(static_cast<size_t>(M)), o_rowclear = carve(R), zeroed = total;
  const size_t o_head = carve(static_cast<size_t>(N) * 4), minus_one = total - o_head;
  const size_t o_req = carve(static_cast<size_t>(N) * S * 8), o_next = carve(R * 4), o_vict = carve(R * kSetBytes);
  std::vector<size_t> o_extra;
  for (size_t bytes : extra_bytes(out->n_dirty)) o_extra.push_back(carve(bytes));
  if (int rc = stage(std::vector<Staged>{{&e->d_pseq, total, nullptr}, {&e->d_pseq_nom, csr.size() * 4, csr.data()}})) return rc;
  char* const base = static_cast<char*>(e->d_pseq.p);
  spx::SeqOverlay& o = out->o;
  auto addr = [&](size_t off, auto*& p) { p = reinterpret_cast<std::remove_reference_t<decltype(p)>>(base + off); };
  o.step = 0, addr(o_gone, o.gone), addr(o_clear, o.nom_cleared), addr(o_rowclear, o.row_cleared), addr(o_head, o.head), addr(o_req, o.requested);
  addr(o_next, o.row_next), addr(o_vict, o.victims);
  o.row_nom_ptr = static_cast<const int32_t*>(e->d_pseq_nom.p);
  o.row_nom = o.row_nom_ptr + n_rows + 1;
  out->row_nom_node = o.row_nom + own;
  for (size_t x : o_extra) out->extra.push_back(base + x);
  SPX_HIP(e, hipMemsetAsync(base, 0, zeroed, e->stream));
  SPX_HIP(e, hipMemsetAsync(base + o_head, 0xFF, minus_one, e->stream));
  e->pre_sequential = true, e->pseq_victims = o.victims;
  return SPX_OK;
}

// What CapacityScheduling's two loops check before anything moves: state first, then the arguments.
// nrt: the loop reads spx_upload_preempt_nrt's side table too.
int cap_seq_check(spx_engine* e, const std::string& who, const int64_t* rows, int64_t n_rows, bool nrt) {
  if (!e->quota || !e->q_has_min) return fail(e, SPX_ERR_STATE, who + ": the quota tables (spx_upload_quota with min) are not uploaded");
  if (!e->pre_nodes || !e->pre_pods) return fail(e, SPX_ERR_STATE, who + ": spx_upload_preempt_nodes / spx_upload_preempt_pods not called");
  if (e->h_pre_nom_ptr.back() > 0 && !e->pre_nomq) return fail(e, SPX_ERR_STATE, who + ": no spx_upload_preempt_nominated_quota since the last spx_upload_preempt_nodes");
  if (nrt && !e->pnrt_table) return fail(e, SPX_ERR_STATE, who + ": no spx_upload_preempt_nrt since the last spx_upload_preempt_nodes / spx_upload_preempt_pods");
  if (!rows || n_rows <= 0) return fail(e, SPX_ERR_ARG, who + ": empty row list");
  return rows_in_batch(e, who, rows, n_rows);
}

// Their staging: seq_stage around preempt_stage with the working marks, Used and aggregate among the carve-outs (SeqStaged::extra, in
// that order), `eligible` and the caller's `more` among the staged buffers.  The run is a CapacityScheduling loop from here on.
int cap_seq_stage(spx_engine* e, const std::string& who, const int64_t* rows, int64_t n_rows, const uint8_t* eligible, const uint8_t* node_mask, std::vector<Staged> mine,
                  SeqStaged* st) {
  const int64_t A = e->h_pre_pod_ptr.back(), NS = e->q_n_namespaces;
  auto extra = [&](int32_t) { return std::vector<size_t>{static_cast<size_t>(A), static_cast<size_t>(NS) * S * 8, static_cast<size_t>(NS), S * 8, 4}; };
  auto stage = [&](std::vector<Staged> more) {
    more.insert(more.end(), mine.begin(), mine.end());
    if (eligible) more.push_back({&e->d_pre_elig, static_cast<size_t>(n_rows), eligible});
    return preempt_stage(e, who, rows, n_rows, node_mask, e->d_pre_rec, spx::kPreemptRowFields, more);
  };
  if (int rc = seq_stage(e, who, rows, n_rows, extra, stage, st)) return rc;
  e->pre_toleration = false;
  return SPX_OK;
}

// Their arguments at step 0, once cap_seq_stage has carved the overlay.
spx::CapSeqArgs cap_seq_args(spx_engine* e, const SeqStaged& st, const uint8_t* eligible) {
  const size_t M = static_cast<size_t>(e->h_pre_nom_ptr.back());
  spx::CapSeqArgs q{};
  q.t = preempt_args(e);
  q.overlay(st.o);
  q.eligible = eligible ? static_cast<const uint8_t*>(e->d_pre_elig.p) : nullptr;
  const char* const side = static_cast<const char*>(e->d_pre_nomq.p);  // (never read when M == 0)
  q.nom_qreq = reinterpret_cast<const int64_t*>(side);
  q.nom_ns = reinterpret_cast<const int32_t*>(side + M * S * 8);
  q.nom_qreq_present = reinterpret_cast<const uint8_t*>(side + M * (S * 8 + 4));
  q.marks = reinterpret_cast<uint8_t*>(st.extra[0]);
  q.used = reinterpret_cast<int64_t*>(st.extra[1]);
  q.used_present = reinterpret_cast<uint8_t*>(st.extra[2]);
  q.agg_used = reinterpret_cast<int64_t*>(st.extra[3]);
  q.agg_used_present = reinterpret_cast<uint32_t*>(st.extra[4]);
  return q;
}

// The end of every entry point: what `launches` enqueues between the two events, and the run as the one the fetches answer for.
// Everything is enqueued here; each launch reads what the one before it left on the device, and nothing is read back in between.
template <class Launches>
int preempt_launch(spx_engine* e, Launches launches) {
  SPX_HIP(e, hipEventRecord(e->ev0, e->stream));
  launches();
  SPX_HIP(e, hipGetLastError());
  SPX_HIP(e, hipEventRecord(e->ev1, e->stream));
  e->timed = e->pre_valid = true;
  return SPX_OK;
}

}  // namespace

extern "C" {

int spx_preempt_check(const spx_preempt_nodes_soa* t, int64_t* bad_node_out) {
  if (!preempt_columns_present(t) || !bad_node_out) return SPX_ERR_ARG;
  *bad_node_out = preempt_bad_node(t, nullptr);
  return *bad_node_out < 0 ? SPX_OK : SPX_ERR_ARG;
}

int spx_upload_preempt_nodes(spx_engine* e, const spx_preempt_nodes_soa* t) {
  if (!e || !t) return SPX_ERR_ARG;
  if (!preempt_columns_present(t)) return fail(e, SPX_ERR_ARG, "preempt nodes: NULL column in a non-empty table");
  std::string why;
  const int64_t badn = preempt_bad_node(t, &why);
  if (badn >= 0) return fail(e, SPX_ERR_ARG, "preempt nodes: node " + std::to_string(badn) + ": " + why);
  SPX_HIP(e, hipSetDevice(e->device));
  int rc = set_nodes(e, t->n_nodes);
  if (rc) return rc;
  e->pre_nodes = e->pre_marks_valid = e->pre_valid = e->ptol_table = e->pre_nomq = e->pnrt_table = false;
  const size_t N = static_cast<size_t>(t->n_nodes), A = static_cast<size_t>(t->pod_ptr[N]), M = static_cast<size_t>(t->nom_ptr[N]), B = static_cast<size_t>(t->pdb_ptr[N]);
  // the columns as records: a wave reads a node and each of its pods through one base pointer
  std::vector<spx::PreemptNode> nodes(N);
  std::vector<spx::PreemptPod> pods(A);
  std::vector<spx::PreemptNom> noms(M);
  for (size_t n = 0; n < N; ++n) {
    spx::PreemptNode& r = nodes[n];
    std::memcpy(r.alloc, t->allocatable + n * S, sizeof r.alloc);
    std::memcpy(r.requested, t->requested + n * S, sizeof r.requested);
    r.pod_begin = t->pod_ptr[n], r.pod_end = t->pod_ptr[n + 1], r.nom_begin = t->nom_ptr[n], r.nom_end = t->nom_ptr[n + 1];
    r.pdb_begin = t->pdb_ptr[n], r.pdb_end = t->pdb_ptr[n + 1], r.present = t->present[n] != 0, r.pad = 0;
  }
  for (size_t j = 0; j < A; ++j) {
    spx::PreemptPod& r = pods[j];
    std::memcpy(r.fit, t->pod_fit_req + j * S, sizeof r.fit);
    std::memcpy(r.qreq, t->pod_quota_req + j * S, sizeof r.qreq);
    r.start = t->pod_start[j], r.prio = t->pod_priority[j], r.ns = t->pod_ns[j], r.pdb_mask = t->pod_pdb_mask[j], r.hi_order = t->pod_hi_order[j];
    r.qreq_present = t->pod_quota_req_present[j], r.marks = (t->pod_flags[j] & SPX_PREEMPT_POD_IN_QUOTA_SET) ? 1 : 0;
    std::memset(r.pad, 0, sizeof r.pad);
  }
  for (size_t j = 0; j < M; ++j) {
    spx::PreemptNom& r = noms[j];
    std::memcpy(r.fit, t->nom_fit_req + j * S, sizeof r.fit);
    r.row = t->nom_pending_row[j], r.prio = t->nom_priority[j], r.pad = 0;
  }
  struct Drain {  // the staged records live until the copies have landed
    spx_engine* e;
    ~Drain() { (void)hipStreamSynchronize(e->stream); }
  } drain{e};
  if ((rc = upload(e, e->d_pre_nodes, nodes.data(), N * sizeof(spx::PreemptNode))) || (rc = upload(e, e->d_pre_podrec, pods.data(), A * sizeof(spx::PreemptPod))) ||
      (rc = upload(e, e->d_pre_noms, noms.data(), M * sizeof(spx::PreemptNom))) || (rc = upload(e, e->d_pre_pdb_allowed, t->pdb_allowed, B * 4)))
    return rc;
  e->h_pre_pod_ptr.assign(t->pod_ptr, t->pod_ptr + N + 1);
  e->h_pre_hi.assign(t->pod_hi_order, t->pod_hi_order + A);  // (an empty column may be NULL: A == 0 then)
  e->h_pre_nom_ptr.assign(t->nom_ptr, t->nom_ptr + N + 1);
  e->h_pre_nom_row.assign(t->nom_pending_row, t->nom_pending_row + M);
  SPX_HIP(e, hipStreamSynchronize(e->stream));
  e->pre_nodes = true;
  return SPX_OK;
}

int spx_upload_preempt_pods(spx_engine* e, const spx_preempt_pods_soa* t) {
  if (!e || !t) return SPX_ERR_ARG;
  if (t->n_pods <= 0 || !t->fit_req) return fail(e, SPX_ERR_ARG, "preempt pods: empty table");
  uint64_t total[S] = {0};
  for (int64_t p = 0; p < t->n_pods; ++p)
    for (int s = 0; s < S; ++s) {
      const int64_t v = t->fit_req[p * S + s];
      if (v < 0) return fail(e, SPX_ERR_ARG, "preempt pods: row " + std::to_string(p) + ": a negative request");
      if ((total[s] += static_cast<uint64_t>(v)) >= static_cast<uint64_t>(kSumLimit))
        return fail(e, SPX_ERR_ARG, "preempt pods: row " + std::to_string(p) + ": slot " + std::to_string(s) + " sums to 2^62 or more");
    }
  SPX_HIP(e, hipSetDevice(e->device));
  int rc = set_pods(e, t->n_pods);
  if (rc) return rc;
  e->pre_pods = e->pre_valid = e->pnrt_table = false;
  if ((rc = upload(e, e->d_pre_pod_fit, t->fit_req, static_cast<size_t>(t->n_pods) * S * 8))) return rc;
  SPX_HIP(e, hipStreamSynchronize(e->stream));
  e->pre_pods = true;
  return SPX_OK;
}

int spx_preempt_dry_run(spx_engine* e, const int64_t* rows, int64_t n_rows, const uint8_t* node_mask) {
  if (!e) return SPX_ERR_ARG;
  if (!e->quota || !e->q_has_min) return fail(e, SPX_ERR_STATE, "preemption dry run: the quota tables (spx_upload_quota with min) are not uploaded");
  if (!e->pre_nodes || !e->pre_pods) return fail(e, SPX_ERR_STATE, "preemption dry run: spx_upload_preempt_nodes / spx_upload_preempt_pods not called");
  const std::string who = "preemption dry run";
  if (!rows || n_rows <= 0) return fail(e, SPX_ERR_ARG, who + ": empty row list");
  int rc;
  if ((rc = rows_in_batch(e, who, rows, n_rows)) || (rc = preempt_stage(e, who, rows, n_rows, node_mask, e->d_pre_rec, spx::kPreemptRowFields, {}))) return rc;
  e->pre_toleration = e->pre_sequential = false;
  const spx::PreemptArgs a = preempt_args(e);
  return preempt_launch(e, [&] {
    if (!e->pre_marks_valid) {
      spx::launch_preempt_marks(a, e->stream);
      e->pre_marks_valid = true;
    }
    spx::launch_preempt_rows(a, e->stream);
    spx::launch_preempt_cells(a, static_cast<unsigned>(e->n_nodes), e->stream);
    spx::launch_preempt_pick(pick_args(e), e->stream);
  });
}

int spx_upload_preempt_nominated_quota(spx_engine* e, const spx_preempt_nominated_quota_soa* t) {
  if (!e || !t) return SPX_ERR_ARG;
  if (!e->pre_nodes) return fail(e, SPX_ERR_STATE, "preempt nominated quota: spx_upload_preempt_nodes not called");
  const int64_t M = e->h_pre_nom_ptr.back();
  if (t->n_nominated != M)
    return fail(e, SPX_ERR_ARG, "preempt nominated quota: " + std::to_string(t->n_nominated) + " entries for the node table's " + std::to_string(M) + " nominated records");
  if (M > 0 && (!t->ns || !t->quota_req || !t->quota_req_present)) return fail(e, SPX_ERR_ARG, "preempt nominated quota: NULL column in a non-empty table");
  for (int64_t j = 0; j < M * S; ++j)
    if (t->quota_req[j] < 0 || t->quota_req[j] >= kSumLimit) return fail(e, SPX_ERR_ARG, "preempt nominated quota: record " + std::to_string(j / S) + ": a request that is negative or 2^62 or more");
  // one allocation: [quota_req | ns | present], the widest first so that each part is aligned
  const size_t m = static_cast<size_t>(M);
  std::vector<char> packed(m * (S * 8 + 4 + 1));
  if (m) {
    std::memcpy(packed.data(), t->quota_req, m * S * 8);
    std::memcpy(packed.data() + m * S * 8, t->ns, m * 4);
    std::memcpy(packed.data() + m * (S * 8 + 4), t->quota_req_present, m);
  }
  SPX_HIP(e, hipSetDevice(e->device));
  e->pre_nomq = e->pre_valid = false;
  if (int rc = upload(e, e->d_pre_nomq, packed.data(), packed.size())) return rc;
  SPX_HIP(e, hipStreamSynchronize(e->stream));  // the staged records live until the copy has landed
  e->pre_nomq = true;
  return SPX_OK;
}

int spx_preempt_sequential(spx_engine* e, const int64_t* rows, int64_t n_rows, const uint8_t* eligible, const uint8_t* node_mask) {
  if (!e) return SPX_ERR_ARG;
  const std::string who = "sequential capacity preemption";
  if (int rc = cap_seq_check(e, who, rows, n_rows, false)) return rc;
  SeqStaged st;
  if (int rc = cap_seq_stage(e, who, rows, n_rows, eligible, node_mask, {}, &st)) return rc;
  spx::PickArgs pick = pick_args(e);
  spx::CapSeqArgs q = cap_seq_args(e, st, eligible);
  return preempt_launch(e, [&] {
    spx::launch_cap_seq_init(q, e->stream);
    for (; q.step < n_rows; ++q.step) {
      pick.step = q.step;
      spx::launch_cap_seq_step(q, e->stream);
      spx::launch_ptol_seq_pick(pick, e->stream);
      spx::launch_cap_seq_apply(q, e->stream);
    }
  });
}

int spx_preempt_nrt_sequential(spx_engine* e, const int64_t* rows, int64_t n_rows, const uint8_t* eligible, const uint8_t* node_mask, int32_t preemption_mode) {
  if (!e) return SPX_ERR_ARG;
  const std::string who = "sequential capacity preemption with NRT";
  if (int rc = cap_seq_check(e, who, rows, n_rows, true)) return rc;
  const size_t rec = static_cast<size_t>(spx::round_up(n_rows, 64)) * spx::kPnrtRowFields * 8;
  SeqStaged st;
  if (int rc = cap_seq_stage(e, who, rows, n_rows, eligible, node_mask, {{&e->d_pnrt_rec, rec, nullptr}}, &st)) return rc;  // the memory pre-check counts the NRT row record too
  e->pre_nrt = true, e->pnrt_mode = preemption_mode != 0;
  spx::PickArgs pick = pick_args(e);
  spx::CnrtSeqArgs p{cap_seq_args(e, st, eligible), nrt_refit_args(e)};
  return preempt_launch(e, [&] {
    spx::launch_cap_seq_init(p.q, e->stream);
    spx::launch_cnrt_rows(spx::CnrtArgs{p.q.t, p.n}, e->stream);  // a function of the preemptors' uploaded columns alone: once, for every row
    for (; p.q.step < n_rows; ++p.q.step) {
      pick.step = p.q.step;
      spx::launch_cap_seq_row(p.q, e->stream);
      spx::launch_cnrt_seq_cells(p, e->stream);
      spx::launch_ptol_seq_pick(pick, e->stream);
      spx::launch_cnrt_seq_apply(p, e->stream);
    }
  });
}

int spx_upload_preempt_toleration(spx_engine* e, const spx_preempt_toleration_soa* t) {
  if (!e || !t) return SPX_ERR_ARG;
  if (!e->pre_nodes) return fail(e, SPX_ERR_STATE, "preempt toleration: spx_upload_preempt_nodes not called");
  const int64_t A = e->h_pre_pod_ptr.back();
  if (t->n_pods != A) return fail(e, SPX_ERR_ARG, "preempt toleration: " + std::to_string(t->n_pods) + " entries for the node table's " + std::to_string(A) + " pods");
  if (A > 0 && (!t->min_preemptable || !t->exempt_until_ns || !t->flags)) return fail(e, SPX_ERR_ARG, "preempt toleration: NULL column in a non-empty table");
  std::vector<spx::PtolPod> rec(static_cast<size_t>(A));
  for (int64_t j = 0; j < A; ++j) {
    const uint8_t f = t->flags[j];
    if ((f & SPX_PTOL_POD_HAS_CLASS) && (f & SPX_PTOL_POD_CLASS_MISSING))
      return fail(e, SPX_ERR_ARG, "preempt toleration: pod " + std::to_string(j) + " has its class and misses it");
    rec[j] = spx::PtolPod{t->exempt_until_ns[j], t->min_preemptable[j], static_cast<uint32_t>(f & (SPX_PTOL_POD_HAS_CLASS | SPX_PTOL_POD_CLASS_MISSING))};
  }
  SPX_HIP(e, hipSetDevice(e->device));
  e->ptol_table = e->pre_valid = false;
  if (int rc = upload(e, e->d_ptol_pods, rec.data(), rec.size() * sizeof(spx::PtolPod))) return rc;
  SPX_HIP(e, hipStreamSynchronize(e->stream));  // the staged records live until the copy has landed
  e->ptol_table = true;
  return SPX_OK;
}

int spx_preempt_toleration_dry_run(spx_engine* e, const int64_t* rows, int64_t n_rows, const int32_t* priority, const uint8_t* preempt_never, int64_t now_ns,
                                   const uint8_t* node_mask) {
  if (!e) return SPX_ERR_ARG;
  const std::string who = "preemption toleration dry run";
  int rc;
  if ((rc = ptol_check(e, who, rows, n_rows, priority, preempt_never, now_ns)) || (rc = ptol_stage(e, who, rows, n_rows, priority, preempt_never, nullptr, now_ns, node_mask, {})))
    return rc;
  e->pre_sequential = false;
  const spx::PtolArgs a = ptol_args(e);
  return preempt_launch(e, [&] {
    spx::launch_ptol_rows(a, e->stream);
    spx::launch_ptol_cells(a, static_cast<unsigned>(e->n_nodes), e->stream);
    spx::launch_preempt_pick(pick_args(e), e->stream);
  });
}

int spx_upload_preempt_nrt(spx_engine* e, const spx_preempt_nrt_soa* t) {
  if (!e || !t) return SPX_ERR_ARG;
  const std::string who = "preempt nrt";
  if (!e->pre_nodes || !e->pre_pods) return fail(e, SPX_ERR_STATE, who + ": spx_upload_preempt_nodes / spx_upload_preempt_pods not called");
  int32_t kind = 0;
  int64_t bad = -1;
  if (spx_flatten_preempt_nrt_check(t, &kind, &bad) != SPX_OK) {
    static const char* const what[] = {"", "node ", "assigned pod ", "pod row ", ""};
    const char* const why[] = {"", "more than 8 zones, a NUMA id above 63, a slot outside the slot table, or available > allocatable",
                               "a release that is negative, 2^62 or more, or outside the zone and slot tables", "more than SPX_NRT_MAX_CTRS containers (a long row)",
                               "a NULL column, more than SPX_NRT_MAX_RES slots, or sizes that contradict each other"};
    return fail(e, SPX_ERR_ARG, who + ": " + what[kind] + (kind < 4 ? std::to_string(bad) + ": " : std::string()) + why[kind]);
  }
  const int64_t N = e->n_nodes, A = e->h_pre_pod_ptr.back(), P = e->n_pods;
  const int R = t->slots->n_res;
  if (t->n_nodes != N) return fail(e, SPX_ERR_ARG, who + ": " + std::to_string(t->n_nodes) + " nodes for the node table's " + std::to_string(N));
  if (t->n_assigned != A) return fail(e, SPX_ERR_ARG, who + ": " + std::to_string(t->n_assigned) + " entries for the node table's " + std::to_string(A) + " pods");
  if (t->pods->n_pods != P) return fail(e, SPX_ERR_ARG, who + ": " + std::to_string(t->pods->n_pods) + " pod rows for the pod table's " + std::to_string(P));
  constexpr int Z = SPX_NRT_MAX_ZONES, RM = SPX_NRT_MAX_RES, CM = SPX_NRT_MAX_CTRS;
  std::vector<spx::PnrtNode> nodes(static_cast<size_t>(N));
  std::vector<spx::PnrtRel> rel(static_cast<size_t>(t->rel_ptr[A]));
  for (int64_t n = 0; n < N; ++n) {
    spx::PnrtNode& r = nodes[n];
    std::memset(&r, 0, sizeof r);
    r.flags = t->node_flags[n], r.n_zones = t->n_zones[n], r.node_present = t->node_present[n];
    for (int z = 0; z < r.n_zones; ++z) {
      r.zone_id[z] = t->zone_id[n * Z + z], r.zone_present[z] = t->zone_present[n * Z + z];
      for (int s = 0; s < R; ++s) r.avail[z][s] = t->zone_avail[(n * Z + z) * R + s], r.headroom[z][s] = t->zone_headroom[(n * Z + z) * R + s];
    }
    // what a lane can add up: every release of the node's pods, per slot
    uint64_t total[RM] = {0};
    for (int64_t j = e->h_pre_pod_ptr[n]; j < e->h_pre_pod_ptr[n + 1]; ++j)
      for (int32_t k = t->rel_ptr[j]; k < t->rel_ptr[j + 1]; ++k) {
        const int z = t->rel_zone[k], s = t->rel_slot[k];
        if (z >= r.n_zones || !((r.zone_present[z] >> s) & 1u))
          return fail(e, SPX_ERR_ARG, who + ": assigned pod " + std::to_string(j) + ": a release outside the zones and resources of node " + std::to_string(n));
        if ((total[s] += static_cast<uint64_t>(t->rel_qty[k])) >= static_cast<uint64_t>(kSumLimit))
          return fail(e, SPX_ERR_ARG, who + ": node " + std::to_string(n) + ": the releases of slot " + std::to_string(s) + " sum to 2^62 or more");
        rel[k] = spx::PnrtRel{t->rel_qty[k], z * RM + s, 0};
      }
  }
  // the preemptors' columns, the 8-byte ones last so that each part is aligned
  const spx_nrt_pods_soa* p = t->pods;
  const size_t np = static_cast<size_t>(P);
  const size_t bytes[8] = {np, np, np, np * CM, np * CM, np, np * CM * R * 8, np * R * 8};
  const void* const src[8] = {p->qos, p->non_native, p->n_ctr, p->ctr_kind, p->ctr_present, p->pod_present, p->ctr_req, p->pod_req};
  size_t off = 0;
  for (int k = 0; k < 8; ++k) {
    if (k == 6) off = static_cast<size_t>(spx::round_up(static_cast<int64_t>(off), 8));
    e->pnrt_pod_off[k] = off, off += bytes[k];
  }
  std::vector<char> packed(off);
  for (int k = 0; k < 8; ++k)
    if (bytes[k]) std::memcpy(packed.data() + e->pnrt_pod_off[k], src[k], bytes[k]);
  SPX_HIP(e, hipSetDevice(e->device));
  e->pnrt_table = e->pre_valid = false;
  struct Drain {  // the staged records live until the copies have landed
    spx_engine* e;
    ~Drain() { (void)hipStreamSynchronize(e->stream); }
  } drain{e};
  int rc;
  if ((rc = upload(e, e->d_pnrt_nodes, nodes.data(), nodes.size() * sizeof(spx::PnrtNode))) || (rc = upload(e, e->d_pnrt_contrib, t->pod_contributes, static_cast<size_t>(A))) ||
      (rc = upload(e, e->d_pnrt_rel_ptr, t->rel_ptr, static_cast<size_t>(A + 1) * 4)) || (rc = upload(e, e->d_pnrt_rel, rel.data(), rel.size() * sizeof(spx::PnrtRel))) ||
      (rc = upload(e, e->d_pnrt_pods, packed.data(), packed.size())))
    return rc;
  SPX_HIP(e, hipStreamSynchronize(e->stream));
  e->pnrt_n_res = R;
  e->pnrt_max_zones = 0;
  for (int64_t n = 0; n < N; ++n) e->pnrt_max_zones = std::max<int32_t>(e->pnrt_max_zones, t->n_zones[n]);
  e->pnrt_slot_flags = 0;
  for (int s = 0; s < R; ++s) e->pnrt_slot_flags |= static_cast<uint64_t>(t->slots->slot_flags[s]) << (8 * s);
  e->pnrt_table = true;
  return SPX_OK;
}

int spx_preempt_toleration_nrt_dry_run(spx_engine* e, const int64_t* rows, int64_t n_rows, const int32_t* priority, const uint8_t* preempt_never, int64_t now_ns,
                                       const uint8_t* node_mask, int32_t preemption_mode) {
  if (!e) return SPX_ERR_ARG;
  const std::string who = "preemption toleration dry run with NRT";
  if (int rc = ptol_check(e, who, rows, n_rows, priority, preempt_never, now_ns)) return rc;
  if (!e->pnrt_table) return fail(e, SPX_ERR_STATE, who + ": no spx_upload_preempt_nrt since the last spx_upload_preempt_nodes / spx_upload_preempt_pods");
  if (n_rows > int64_t{65535} * 64) return fail(e, SPX_ERR_ARG, who + ": more than 65535 x 64 rows (a workgroup is one wave here): split the row list");
  const size_t rec = static_cast<size_t>(spx::round_up(n_rows, 64)) * spx::kPnrtRowFields * 8;
  if (int rc = ptol_stage(e, who, rows, n_rows, priority, preempt_never, nullptr, now_ns, node_mask, {{&e->d_pnrt_rec, rec, nullptr}})) return rc;
  e->pre_sequential = false;
  e->pre_nrt = true, e->pnrt_mode = preemption_mode != 0;
  const spx::PnrtArgs a = pnrt_args(e);
  return preempt_launch(e, [&] {
    spx::launch_ptol_rows(a.t, e->stream);
    spx::launch_pnrt_rows(a, e->stream);
    spx::launch_pnrt_cells(a, static_cast<unsigned>(e->n_nodes), e->stream);
    spx::launch_preempt_pick(pick_args(e), e->stream);
  });
}

int spx_preempt_nrt_dry_run(spx_engine* e, const int64_t* rows, int64_t n_rows, const uint8_t* node_mask, int32_t preemption_mode) {
  if (!e) return SPX_ERR_ARG;
  const std::string who = "preemption dry run with NRT";
  if (!e->quota || !e->q_has_min) return fail(e, SPX_ERR_STATE, who + ": the quota tables (spx_upload_quota with min) are not uploaded");
  if (!e->pre_nodes || !e->pre_pods) return fail(e, SPX_ERR_STATE, who + ": spx_upload_preempt_nodes / spx_upload_preempt_pods not called");
  if (!e->pnrt_table) return fail(e, SPX_ERR_STATE, who + ": no spx_upload_preempt_nrt since the last spx_upload_preempt_nodes / spx_upload_preempt_pods");
  if (!rows || n_rows <= 0) return fail(e, SPX_ERR_ARG, who + ": empty row list");
  if (int rc = rows_in_batch(e, who, rows, n_rows)) return rc;
  if (n_rows > int64_t{65535} * 64) return fail(e, SPX_ERR_ARG, who + ": more than 65535 x 64 rows (a workgroup is one wave here): split the row list");
  const size_t rec = static_cast<size_t>(spx::round_up(n_rows, 64)) * spx::kPnrtRowFields * 8;
  if (int rc = preempt_stage(e, who, rows, n_rows, node_mask, e->d_pre_rec, spx::kPreemptRowFields, {{&e->d_pnrt_rec, rec, nullptr}})) return rc;
  e->pre_toleration = e->pre_sequential = false;
  e->pre_nrt = true, e->pnrt_mode = preemption_mode != 0;
  const spx::CnrtArgs a = cnrt_args(e);
  return preempt_launch(e, [&] {
    if (!e->pre_marks_valid) {
      spx::launch_preempt_marks(a.t, e->stream);
      e->pre_marks_valid = true;
    }
    spx::launch_preempt_rows(a.t, e->stream);
    spx::launch_cnrt_rows(a, e->stream);
    spx::launch_cnrt_cells(a, static_cast<unsigned>(e->n_nodes), e->stream);
    spx::launch_preempt_pick(pick_args(e), e->stream);
  });
}

int spx_preempt_toleration_sequential(spx_engine* e, const int64_t* rows, int64_t n_rows, const int32_t* priority, const uint8_t* preempt_never, const uint8_t* eligible,
                                      int64_t now_ns, const uint8_t* node_mask) {
  if (!e) return SPX_ERR_ARG;
  const std::string who = "sequential preemption";
  if (int rc = ptol_check(e, who, rows, n_rows, priority, preempt_never, now_ns)) return rc;
  SeqStaged st;
  auto extra = [&](int32_t n_dirty) { return std::vector<size_t>{static_cast<size_t>(n_rows) * static_cast<size_t>(n_dirty) * 4}; };
  auto stage = [&](std::vector<Staged> more) { return ptol_stage(e, who, rows, n_rows, priority, preempt_never, eligible, now_ns, node_mask, more); };
  if (int rc = seq_stage(e, who, rows, n_rows, extra, stage, &st)) return rc;
  spx::PickArgs pick = pick_args(e);
  spx::PtolSeqArgs q{};
  q.t = ptol_args(e);
  q.o = st.o;
  q.n_dirty = st.n_dirty;
  q.pick = pick.pick;
  q.row_nom_node = st.row_nom_node;
  q.dirty = reinterpret_cast<int32_t*>(st.extra[0]);
  return preempt_launch(e, [&] {
    spx::launch_ptol_seq_init(q, e->stream);
    spx::launch_ptol_rows(q.t, e->stream);
    spx::launch_ptol_cells(q.t, static_cast<unsigned>(e->n_nodes), e->stream);  // the untouched state: no row of the list has moved anything yet
    for (; q.o.step < n_rows; ++q.o.step) {
      pick.step = q.o.step;
      spx::launch_ptol_seq_pick(pick, e->stream);
      spx::launch_ptol_seq_step(q, e->stream);
    }
  });
}

int spx_preempt_toleration_nrt_sequential(spx_engine* e, const int64_t* rows, int64_t n_rows, const int32_t* priority, const uint8_t* preempt_never, const uint8_t* eligible,
                                          int64_t now_ns, const uint8_t* node_mask, int32_t preemption_mode) {
  if (!e) return SPX_ERR_ARG;
  const std::string who = "sequential preemption with NRT";
  if (int rc = ptol_check(e, who, rows, n_rows, priority, preempt_never, now_ns)) return rc;
  if (!e->pnrt_table) return fail(e, SPX_ERR_STATE, who + ": no spx_upload_preempt_nrt since the last spx_upload_preempt_nodes / spx_upload_preempt_pods");
  if (n_rows > int64_t{65535} * 64) return fail(e, SPX_ERR_ARG, who + ": more than 65535 x 64 rows (a workgroup is one wave here): split the row list");
  const size_t rec = static_cast<size_t>(spx::round_up(n_rows, 64)) * spx::kPnrtRowFields * 8;
  SeqStaged st;
  auto extra = [&](int32_t n_dirty) { return std::vector<size_t>{static_cast<size_t>(n_rows) * static_cast<size_t>(n_dirty) * 4}; };
  auto stage = [&](std::vector<Staged> more) {
    more.push_back({&e->d_pnrt_rec, rec, nullptr});  // the memory pre-check counts the NRT row record too
    return ptol_stage(e, who, rows, n_rows, priority, preempt_never, eligible, now_ns, node_mask, more);
  };
  if (int rc = seq_stage(e, who, rows, n_rows, extra, stage, &st)) return rc;
  e->pre_nrt = true, e->pnrt_mode = preemption_mode != 0;
  spx::PickArgs pick = pick_args(e);
  spx::PnrtSeqArgs p{};
  p.q.t = ptol_args(e);
  p.q.o = st.o;
  p.q.n_dirty = st.n_dirty;
  p.q.pick = pick.pick;
  p.q.row_nom_node = st.row_nom_node;
  p.q.dirty = reinterpret_cast<int32_t*>(st.extra[0]);
  p.n = nrt_refit_args(e);
  const spx::PnrtArgs sweep{p.q.t, p.n};
  return preempt_launch(e, [&] {
    spx::launch_ptol_seq_init(p.q, e->stream);
    spx::launch_ptol_rows(p.q.t, e->stream);
    spx::launch_pnrt_rows(sweep, e->stream);
    spx::launch_pnrt_cells(sweep, static_cast<unsigned>(e->n_nodes), e->stream);  // the untouched state with F: no row of the list has moved anything yet
    for (; p.q.o.step < n_rows; ++p.q.o.step) {
      pick.step = p.q.o.step;
      spx::launch_ptol_seq_pick(pick, e->stream);
      spx::launch_pnrt_seq_step(p, e->stream);
    }
  });
}

}  // extern "C"

namespace {

// rows [i_begin, i_end) of the cell records, [node][i] on the host
int fetch_cells(spx_engine* e, int64_t i_begin, int64_t i_end, std::vector<spx::PreemptCell>& h) {
  if (int rc = preempt_results(e, i_begin, i_end)) return rc;
  const size_t n = static_cast<size_t>(i_end - i_begin), N = static_cast<size_t>(e->n_nodes), R = static_cast<size_t>(e->pre_row_stride);
  h.resize(n * N);
  if (n == 0) return SPX_OK;
  SPX_HIP(e, hipSetDevice(e->device));
  SPX_HIP(e, hipStreamSynchronize(e->stream));
  SPX_HIP(e, hipMemcpy2D(h.data(), n * sizeof(spx::PreemptCell), static_cast<const spx::PreemptCell*>(e->d_pre_cells.p) + i_begin, R * sizeof(spx::PreemptCell),
                         n * sizeof(spx::PreemptCell), N, hipMemcpyDeviceToHost));
  return SPX_OK;
}

// put(i * n_nodes + node, cell) for every fetched cell
template <class Put>
int each_cell(spx_engine* e, int64_t i_begin, int64_t i_end, Put put) {
  if (!e) return SPX_ERR_ARG;
  std::vector<spx::PreemptCell> h;
  if (int rc = fetch_cells(e, i_begin, i_end, h)) return rc;
  const size_t n = static_cast<size_t>(i_end - i_begin), N = static_cast<size_t>(e->n_nodes);
  for (size_t i = 0; i < n; ++i)
    for (size_t node = 0; node < N; ++node) put(i * N + node, h[node * n + i]);
  return SPX_OK;
}

// a victim set of `node` (bit = position in its uploaded list) as positions, most important first
int victims_in_order(spx_engine* e, int64_t node, const uint32_t* mask, int32_t* pod_pos_out, int32_t cap, int32_t* n_out) {
  const int32_t p0 = e->h_pre_pod_ptr[node], L = e->h_pre_pod_ptr[node + 1] - p0;
  int32_t n = 0;
  for (int32_t k = 0; k < L; ++k) {
    const int32_t pos = e->h_pre_hi[p0 + k];
    if (!((mask[pos >> 5] >> (pos & 31)) & 1u)) continue;
    if (n < cap) pod_pos_out[n] = pos;
    ++n;
  }
  *n_out = n;
  if (n > cap) return fail(e, SPX_ERR_ARG, "preemption victims: " + std::to_string(n) + " victims do not fit cap");
  return SPX_OK;
}

}  // namespace

extern "C" {

int spx_fetch_preempt_cells(spx_engine* e, int64_t i_begin, int64_t i_end, uint8_t* status, int32_t* n_victims, int32_t* n_violations) {
  return each_cell(e, i_begin, i_end, [&](size_t at, const spx::PreemptCell& c) {
    if (status) status[at] = static_cast<uint8_t>(c.status);
    if (n_victims) n_victims[at] = c.n_victims;
    if (n_violations) n_violations[at] = c.n_violations;
  });
}

int spx_fetch_preempt_keys(spx_engine* e, int64_t i_begin, int64_t i_end, int32_t* hi_priority, int64_t* priority_sum, int64_t* start) {
  return each_cell(e, i_begin, i_end, [&](size_t at, const spx::PreemptCell& c) {
    if (hi_priority) hi_priority[at] = c.hi_prio;
    if (priority_sum) priority_sum[at] = c.prio_sum;
    if (start) start[at] = c.start;
  });
}

int spx_fetch_preempt_pick(spx_engine* e, int64_t i_begin, int64_t i_end, int32_t* node, int32_t* n_victims, int32_t* n_violations, int32_t* n_candidates,
                           int32_t* n_ties) {
  if (!e) return SPX_ERR_ARG;
  if (int rc = preempt_results(e, i_begin, i_end)) return rc;
  const size_t n = static_cast<size_t>(i_end - i_begin), R = static_cast<size_t>(e->pre_row_stride);
  SPX_HIP(e, hipSetDevice(e->device));
  SPX_HIP(e, hipStreamSynchronize(e->stream));
  int32_t* const out[5] = {node, n_victims, n_violations, n_candidates, n_ties};
  for (int k = 0; k < 5; ++k)
    if (out[k] && n) SPX_HIP(e, hipMemcpy(out[k], static_cast<const int32_t*>(e->d_pre_pick.p) + k * R + i_begin, n * 4, hipMemcpyDeviceToHost));
  return SPX_OK;
}

int spx_fetch_preempt_victims(spx_engine* e, int64_t i, int64_t node, int32_t* pod_pos_out, int32_t cap, int32_t* n_out, int32_t* status_out) {
  if (!e || !n_out || cap < 0 || (cap > 0 && !pod_pos_out)) return SPX_ERR_ARG;
  if (int rc = preempt_results(e, i, i + 1)) return rc;
  if (node < 0 || node >= e->n_nodes) return fail(e, SPX_ERR_ARG, "preemption victims: node out of range");
  SPX_HIP(e, hipSetDevice(e->device));
  constexpr size_t kMaskBytes = SPX_PREEMPT_MAX_NODE_PODS / 8;
  if (e->pre_sequential) {
    // the loop stored the victim set of the row's picked cell at its step; the state any other cell of the row saw is gone
    int32_t picked = -1;
    uint32_t mask[kMaskBytes / 4];
    SPX_HIP(e, hipStreamSynchronize(e->stream));
    SPX_HIP(e, hipMemcpy(&picked, static_cast<const int32_t*>(e->d_pre_pick.p) + i, 4, hipMemcpyDeviceToHost));
    if (picked != node) return fail(e, SPX_ERR_ARG, "preemption victims: after the sequential loop only the row's picked node is answered for");
    SPX_HIP(e, hipMemcpy(mask, e->pseq_victims + i * (kMaskBytes / 4), kMaskBytes, hipMemcpyDeviceToHost));
    if (status_out) *status_out = SPX_PREEMPT_ST_CANDIDATE;
    return victims_in_order(e, node, mask, pod_pos_out, cap, n_out);
  }
  std::lock_guard<std::mutex> g(e->raw_mu);  // one scratch cell: concurrent callers take turns, as in spx_fetch_raw
  if (int rc = ensure(e, e->d_pre_one, sizeof(spx::PreemptCell) + kMaskBytes)) return rc;
  // the one cell again, as row 0 of a list of one, by the kernel of the dry run that ran last: the row's record and mask row are
  // addressed through offset pointers
  spx::PreemptCell* const d_cell = static_cast<spx::PreemptCell*>(e->d_pre_one.p);
  uint32_t* const d_mask = reinterpret_cast<uint32_t*>(static_cast<char*>(e->d_pre_one.p) + sizeof(spx::PreemptCell));
  auto one_cell = [&](auto a) {
    a.n_rows = 1;
    a.row_rec += i;
    if (a.node_mask) a.node_mask += i * e->n_nodes;
    a.node_begin = node;
    a.cells = d_cell;
    a.victims_out = d_mask;
    return a;
  };
  if (e->pre_toleration && e->pre_nrt) {
    spx::PnrtArgs a = pnrt_args(e);
    a.t = one_cell(a.t);
    a.n.nrt_rec += i;
    spx::launch_pnrt_cells(a, 1, e->stream);
  } else if (e->pre_nrt) {
    spx::CnrtArgs a = cnrt_args(e);
    a.t = one_cell(a.t);
    a.n.nrt_rec += i;
    spx::launch_cnrt_cells(a, 1, e->stream);
  } else if (e->pre_toleration) spx::launch_ptol_cells(one_cell(ptol_args(e)), 1, e->stream);
  else spx::launch_preempt_cells(one_cell(preempt_args(e)), 1, e->stream);
  SPX_HIP(e, hipGetLastError());
  struct {
    spx::PreemptCell cell;
    uint32_t mask[kMaskBytes / 4];
  } h;
  SPX_HIP(e, hipMemcpyAsync(&h.cell, d_cell, sizeof h.cell, hipMemcpyDeviceToHost, e->stream));
  SPX_HIP(e, hipMemcpyAsync(h.mask, d_mask, kMaskBytes, hipMemcpyDeviceToHost, e->stream));
  SPX_HIP(e, hipStreamSynchronize(e->stream));
  if (status_out) *status_out = h.cell.status;
  return victims_in_order(e, node, h.mask, pod_pos_out, cap, n_out);
}

}  // extern "C"
