// spx_state.hip — the helpers every engine unit builds on, defined once: the error slots' writer (fail), device and pinned buffers
// (ensure, upload, ensure_pinned), the snapshot's shape (set_nodes, set_pods), TargetLoadPacking's row order, and the score and
// argmax tables that both the evaluation and the commit loops size.  Declared in spx_engine.h; no kernel and no entry point lives here.
#include "spx_engine.h"

#include <limits>

namespace spx_eng {

int fail(const spx_engine* e, int code, const std::string& msg) {
  if (e) {
    {
      std::lock_guard<std::mutex> g(e->err_mu);
      e->err = msg;
    }
    tl_err = msg;
    tl_err_engine = e;
  } else {
    g_create_error = msg;
  }
  return code;
}

int ensure(spx_engine* e, DevBuf& b, size_t bytes) {
  if (b.external) return fail(e, SPX_ERR_STATE, "internal: resize of an externally bound buffer");
  if (bytes == 0) bytes = 16;
  if (b.bytes >= bytes) return SPX_OK;
  if (b.p) SPX_HIP(e, hipFree(b.p));
  b.p = nullptr;
  b.bytes = 0;
  SPX_HIP(e, hipMalloc(&b.p, bytes));
  b.bytes = bytes;
  return SPX_OK;
}

int upload(spx_engine* e, DevBuf& b, const void* src, size_t bytes) {
  if (!src && bytes) return fail(e, SPX_ERR_ARG, "NULL column in table");  // an empty column (e.g. no resource slots) may be NULL
  int rc = ensure(e, b, bytes);
  if (rc) return rc;
  if (bytes) SPX_HIP(e, hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, e->stream));
  return SPX_OK;
}

// a pinned host buffer of at least `want` bytes; a buffer that has to grow is allocated with `slack` bytes to spare
int ensure_pinned(spx_engine* e, void*& p, size_t& bytes, size_t want, size_t slack) {
  if (bytes >= want) return SPX_OK;
  if (p) SPX_HIP(e, hipHostFree(p));
  p = nullptr, bytes = 0;
  SPX_HIP(e, hipHostMalloc(&p, want + slack, hipHostMallocDefault));
  bytes = want + slack;
  return SPX_OK;
}

int set_nodes(spx_engine* e, int64_t n) {
  if (n <= 0) return fail(e, SPX_ERR_ARG, "n_nodes must be positive");
  if (e->n_nodes != -1 && e->n_nodes != n)
    return fail(e, SPX_ERR_STATE, "n_nodes differs from tables already uploaded (one snapshot per engine; destroy and re-create to change shape)");
  e->n_nodes = n;
  e->row_stride = spx::round_up(n, e->option[SPX_OPT_ROW_ALIGN]);
  return SPX_OK;
}

int set_pods(spx_engine* e, int64_t p) {
  if (p <= 0) return fail(e, SPX_ERR_ARG, "n_pods must be positive");
  if (e->n_pods != -1 && e->n_pods != p)
    return fail(e, SPX_ERR_STATE, "n_pods differs from tables already uploaded");
  e->n_pods = p;
  return SPX_OK;
}

// The order of TargetLoadPacking's class form for the pod column in place (n_pods rows of d_tlp_pod, queued on the stream before
// this call): built on the stream, the count of evaluated rows read back.  The caller has cleared tlp_order_valid before it wrote the
// column and synchronises the stream afterwards anyway; this synchronises for the one number.
int tlp_build_order(spx_engine* e) {
  e->tlp_order_valid = false;
  if (e->n_pods <= 0 || e->n_pods > std::numeric_limits<int32_t>::max()) return SPX_OK;  // (rows are int32 in the order: such a batch sweeps plain)
  int rc;
  const size_t words = spx::tlp_order_scratch_words(spx::kTlpAmbSize, e->n_pods);
  if ((rc = ensure(e, e->d_tlp_order, static_cast<size_t>(e->n_pods) * sizeof(int32_t))) || (rc = ensure(e, e->d_tlp_order_scratch, words * sizeof(uint32_t))))
    return rc;
  uint32_t* scratch = static_cast<uint32_t*>(e->d_tlp_order_scratch.p);
  // (SPX_OPT_TLP_CHUNK_SCHED is read here: the order in place keeps the schedule it was built with)
  spx::launch_tlp_order(static_cast<const int64_t*>(e->d_tlp_pod.p), e->n_pods, spx::kTlpAmbSize, e->option[SPX_OPT_TLP_CHUNK_SCHED] != 0,
                        static_cast<int32_t*>(e->d_tlp_order.p), scratch, e->stream);
  SPX_HIP(e, hipGetLastError());
  uint32_t evaluated = 0;
  SPX_HIP(e, hipMemcpyAsync(&evaluated, scratch + spx::tlp_order_evaluated_word(spx::kTlpAmbSize), sizeof evaluated, hipMemcpyDeviceToHost, e->stream));
  SPX_HIP(e, hipStreamSynchronize(e->stream));
  e->tlp_rows_evaluated = evaluated;
  e->tlp_order_valid = true;
  return SPX_OK;
}

// A check of a plugin's score table that writes nothing (spx_eval makes it, with its siblings in spx_engine.hip, before its first
// allocation): a table the caller bound must hold n_pods x row_stride
int score_table_fits(const spx_engine* e, int plugin) {
  if (e->score[plugin].external && (e->score_rows[plugin] < e->n_pods || e->score_stride[plugin] < e->row_stride))
    return fail(e, SPX_ERR_STATE, "bound score table is smaller than n_pods x row_stride");
  return SPX_OK;
}

int ensure_score_table(spx_engine* e, int plugin) {
  DevBuf& b = e->score[plugin];
  if (b.external) return score_table_fits(e, plugin);
  const size_t had = b.p ? b.bytes : 0;
  int rc = ensure(e, b, static_cast<size_t>(e->n_pods) * static_cast<size_t>(e->row_stride));
  if (plugin == SPX_PLUGIN_ALLOCATABLE && (rc || b.bytes != had)) alloc_table_dirty(e);  // (a new allocation may come back at the old address)
  if (rc) return rc;
  e->score_rows[plugin] = e->n_pods;
  e->score_stride[plugin] = e->row_stride;
  return SPX_OK;
}

BestRows best_rows(const spx_engine* e) {
  int64_t* score = static_cast<int64_t*>(e->d_best.p);
  int32_t* node = reinterpret_cast<int32_t*>(score + e->n_pods);
  return BestRows{score, node, node + e->n_pods, node + 2 * e->n_pods};
}
int ensure_best(spx_engine* e, BestRows* out) {
  int rc = ensure(e, e->d_best, static_cast<size_t>(e->n_pods) * 20);
  if (rc == SPX_OK) *out = best_rows(e);
  return rc;
}

// rows [b, e) of `plugin` hold results of an spx_eval
int rows_evaluated(const spx_engine* e, int plugin, int64_t b, int64_t en) {
  const spx_engine::EvalInfo& i = e->eval_info[plugin];
  if (!(e->evaluated & (1u << plugin)) || b < i.begin || en > i.end)
    return fail(e, SPX_ERR_STATE, "rows requested have not been evaluated for this plugin (spx_eval covers [" + std::to_string(i.begin) + ", " +
                                      std::to_string(i.end) + "))");
  return SPX_OK;
}

}  // namespace spx_eng
