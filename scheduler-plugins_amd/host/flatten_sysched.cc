// flatten_sysched.cc — object tables -> SoA columns for SySched (pkg/sysched/sysched.go).  Host-side product code (once per snapshot).
//
// What is hoisted out of the per-(pod,node) path, and where the reference does it per call:
//   node : the cached HostSyscalls[node] (getHostSyscalls, sysched.go:295-303)                       -> a bitset, word-major
//          the loop over HostToPods[node] with getSyscalls per resident pod (sysched.go:267-271)    -> k, a = sum_q |H \ Q_q|, and,
//          where a resident's set holds names the cached host set lacks, the (name, residents holding it) pairs
//   pod  : getSyscalls(pod) (sysched.go:244), resolved to a set id by the caller                    -> the distinct sets as bitsets
// With those, Score (sysched.go:261-278) is popc(H & ~P) + a + k popc(P & ~H) - sum over b in P \ H of c[b] (include/spx.h).
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/spx.h"
#include "parallel.hpp"

namespace {

// the CSR of sets is sane: monotone offsets, name ids inside [0, n_names)
bool sets_ok(const spx_sysched_objects* o) {
  if (o->n_names < 0 || o->n_names > SPX_SYSCHED_MAX_NAMES || o->n_sets < 0) return false;
  if (o->n_sets && !o->set_ptr) return false;
  for (int32_t s = 0; s < o->n_sets; ++s)
    if (o->set_ptr[s] < 0 || o->set_ptr[s + 1] < o->set_ptr[s]) return false;
  const int32_t total = o->n_sets ? o->set_ptr[o->n_sets] : 0;
  if (total && !o->set_name) return false;
  for (int32_t i = 0; i < total; ++i)
    if (o->set_name[i] < 0 || o->set_name[i] >= o->n_names) return false;
  return true;
}

inline int32_t words_of(int32_t n_names) { return n_names > 0 ? (n_names + 63) / 64 : 1; }

void set_to_bits(const spx_sysched_objects* o, int32_t s, uint64_t* w, int32_t W) {
  std::memset(w, 0, sizeof(uint64_t) * static_cast<size_t>(W));
  for (int32_t i = o->set_ptr[s]; i < o->set_ptr[s + 1]; ++i) w[o->set_name[i] >> 6] |= uint64_t{1} << (o->set_name[i] & 63);
}

// one node: host bits, k, a and the stale pairs (appended to `stale`, ascending bit); false = an id out of range
bool flatten_node(const spx_sysched_objects* o, const uint64_t* set_bits, int32_t W, int64_t n, uint64_t* h, int32_t* k_out, int32_t* a_out,
                  std::vector<std::pair<int32_t, int32_t>>& stale) {
  std::memset(h, 0, sizeof(uint64_t) * static_cast<size_t>(W));
  *k_out = *a_out = 0;
  if (!o->host_present[n]) return true;
  for (int32_t i = o->host_ptr[n]; i < o->host_ptr[n + 1]; ++i) {
    const int32_t b = o->host_name[i];
    if (b < 0 || b >= o->n_names) return false;
    h[b >> 6] |= uint64_t{1} << (b & 63);
  }
  int64_t a = 0;
  int32_t count[SPX_SYSCHED_MAX_NAMES];
  bool any_stale = false;
  for (int32_t i = o->res_ptr[n]; i < o->res_ptr[n + 1]; ++i) {
    const int32_t s = o->res_set[i];
    if (s < 0 || s >= o->n_sets) return false;
    const uint64_t* q = set_bits + static_cast<size_t>(s) * W;
    for (int32_t w = 0; w < W; ++w) {
      a += __builtin_popcountll(h[w] & ~q[w]);
      uint64_t out = q[w] & ~h[w];  // names of the resident's set the cached host set lacks
      if (out && !any_stale) std::memset(count, 0, sizeof(int32_t) * static_cast<size_t>(W) * 64), any_stale = true;
      for (; out; out &= out - 1) ++count[w * 64 + __builtin_ctzll(out)];
    }
  }
  *k_out = o->res_ptr[n + 1] - o->res_ptr[n];
  if (a > INT32_MAX) return false;
  *a_out = static_cast<int32_t>(a);
  if (any_stale)
    for (int32_t b = 0; b < W * 64; ++b)
      if (count[b]) stale.emplace_back(b, count[b]);
  return true;
}

}  // namespace

extern "C" int spx_flatten_sysched_pods(const spx_sysched_objects* o, uint64_t* set_bits, int32_t* pod_set) {
  if (!o || !set_bits || !pod_set || !sets_ok(o) || o->n_pods < 0 || (o->n_pods && !o->pod_set)) return SPX_ERR_ARG;
  const int32_t W = words_of(o->n_names);
  for (int32_t s = 0; s < o->n_sets; ++s) set_to_bits(o, s, set_bits + static_cast<size_t>(s) * W, W);
  for (int64_t p = 0; p < o->n_pods; ++p) {
    if (o->pod_set[p] < 0 || o->pod_set[p] >= o->n_sets) return SPX_ERR_ARG;
    pod_set[p] = o->pod_set[p];
  }
  return SPX_OK;
}

extern "C" int spx_flatten_sysched_nodes(const spx_sysched_objects* o, int64_t stale_cap, int32_t* n_words_out, int64_t* n_stale_out, uint64_t* host_bits,
                                         uint8_t* present, int32_t* n_resident, int32_t* resident_missing, int32_t* stale_ptr, int32_t* stale_bit,
                                         int32_t* stale_count) {
  if (!o || !n_words_out || !n_stale_out || !sets_ok(o) || o->n_nodes < 0) return SPX_ERR_ARG;
  if (o->n_nodes && (!o->host_present || !o->host_ptr || !o->res_ptr)) return SPX_ERR_ARG;
  const bool count_only = !host_bits && !present && !n_resident && !resident_missing && !stale_ptr && !stale_bit && !stale_count;
  if (!count_only && (!host_bits || !present || !n_resident || !resident_missing || !stale_ptr || (stale_cap > 0 && (!stale_bit || !stale_count)))) return SPX_ERR_ARG;
  const int32_t W = words_of(o->n_names);
  const int64_t N = o->n_nodes;
  for (int64_t n = 0; n < N; ++n) {
    if (o->host_ptr[n] < 0 || o->host_ptr[n + 1] < o->host_ptr[n] || o->res_ptr[n] < 0 || o->res_ptr[n + 1] < o->res_ptr[n]) return SPX_ERR_ARG;
    if (o->host_ptr[n + 1] > o->host_ptr[n] && !o->host_name) return SPX_ERR_ARG;
    if (o->res_ptr[n + 1] > o->res_ptr[n] && !o->res_set) return SPX_ERR_ARG;
  }
  std::vector<uint64_t> set_bits(static_cast<size_t>(o->n_sets) * W + 1);
  for (int32_t s = 0; s < o->n_sets; ++s) set_to_bits(o, s, set_bits.data() + static_cast<size_t>(s) * W, W);
  // per node on all host threads; the stale pairs are gathered per node and laid out afterwards (they are rare)
  std::vector<std::vector<std::pair<int32_t, int32_t>>> stale(static_cast<size_t>(N));
  std::vector<int32_t> k(static_cast<size_t>(N)), a(static_cast<size_t>(N));
  std::vector<uint8_t> bad(static_cast<size_t>(N), 0);
  spx_host::parallel_rows(N, [&](int64_t row0, int64_t row1) {
    uint64_t h[SPX_SYSCHED_MAX_WORDS];
    for (int64_t n = row0; n < row1; ++n) {
      if (!flatten_node(o, set_bits.data(), W, n, h, &k[static_cast<size_t>(n)], &a[static_cast<size_t>(n)], stale[static_cast<size_t>(n)])) {
        bad[static_cast<size_t>(n)] = 1;
        continue;
      }
      if (count_only) continue;
      for (int32_t w = 0; w < W; ++w) host_bits[static_cast<size_t>(w) * N + n] = h[w];
      present[n] = o->host_present[n] ? 1 : 0;
      n_resident[n] = k[static_cast<size_t>(n)];
      resident_missing[n] = a[static_cast<size_t>(n)];
    }
  }, 256);
  int64_t total = 0;
  for (int64_t n = 0; n < N; ++n) {
    if (bad[static_cast<size_t>(n)]) return SPX_ERR_ARG;
    total += static_cast<int64_t>(stale[static_cast<size_t>(n)].size());
  }
  *n_words_out = W;
  *n_stale_out = total;
  if (count_only) return SPX_OK;
  if (total > stale_cap || total > INT32_MAX) return SPX_ERR_ARG;
  int32_t at = 0;
  for (int64_t n = 0; n < N; ++n) {
    stale_ptr[n] = at;
    for (const auto& e : stale[static_cast<size_t>(n)]) stale_bit[at] = e.first, stale_count[at] = e.second, ++at;
  }
  stale_ptr[N] = at;
  return SPX_OK;
}
