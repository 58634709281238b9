// store-pattern microbenchmark, sibling of wperm.hip: what keeps the class form of the TLP sweep (k_tlp_fast2<..., CLS>) above its own
// store pattern?  wperm's kernel shape — a wave owns (tile, chunk of 64 positions), 16 B per lane and row, 10 tiles, 4 waves per
// block, 100 000 x 10 112 B — with the sweep's row order and "copy" flags (tools/wcls_inputs.py dumps them from the engine's flattened
// pod column), and one thing added at a time:
//   (a) stores only (= wperm's whole-batch shuffle);
//   (b) an evaluated position first runs K independent packed FMAs on 16 registers; K is calibrated once so that an all-evaluated
//       batch takes what the plain form of the sweep takes on this box (--plain-ms);
//   (c) the wave start: sixteen float4 loads of node constants and the chain order -> pod value -> ambiguity word (three dependent
//       loads), or with the values kept next to the order (two);
//   (d) the chunk order: ascending value, heaviest (most evaluated positions) first, heavy / light interleaved;
//   (e) the same held to 4 waves per SIMD by LDS size, against 8;
//   (f) two or four chunks of one tile per wave, a heavy one paired with a light one (k_cls_multi).
// Prints mean and best of 5 x 20 launches per variant.  Plain stores; no inline assembly.
// usage: wcls INPUT [--plain-ms 0.24] [--stride 10112]
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <string>
#include <vector>

#define CHECK(x)                                                                              \
  do {                                                                                        \
    hipError_t e_ = (x);                                                                      \
    if (e_ != hipSuccess) {                                                                   \
      std::fprintf(stderr, "%s: %s (line %d)\n", #x, hipGetErrorString(e_), __LINE__);        \
      std::exit(1);                                                                           \
    }                                                                                         \
  } while (0)

typedef float F32x2 __attribute__((ext_vector_type(2)));
constexpr int kAmb = 1 << 16;

struct Args {
  uint8_t* out;
  const int32_t* perm;      // [rows] row at each position
  const uint8_t* copy;      // [rows] 1 = the position stores what the wave already holds
  const int64_t* val_row;   // [rows] pod value by row (the three-load chain)
  const int64_t* val_pos;   // [rows] pod value by position (the two-load chain)
  const uint32_t* amb;      // [kAmb]
  const float4* consts;     // [n_tiles * 16 * 64]
  int64_t stride, rows;
  int n_tiles, k;           // k: packed FMAs per evaluated position (a multiple of 8)
};

// START: 0 = no loads but the order, 1 = constants + three-load chain, 2 = constants + two-load chain
template <bool EVAL, int START>
__global__ __launch_bounds__(256) void k_cls(Args a) {
  extern __shared__ uint32_t lds[];  // only its size matters: it bounds the blocks per CU
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t unit = static_cast<int64_t>(blockIdx.x) * (blockDim.x >> 6) + wave;
  const int tile = static_cast<int>(unit % a.n_tiles);
  const int64_t pos0 = (unit / a.n_tiles) * 64;
  if (pos0 >= a.rows) return;  // wave-uniform
  const int n_rows = static_cast<int>(pos0 + 64 < a.rows ? 64 : a.rows - pos0);
  const bool live = lane < n_rows;
  const int my_row = live ? min(static_cast<uint32_t>(a.perm[pos0 + lane]), static_cast<uint32_t>(a.rows - 1)) : 0;  // (clamped: no store leaves the table)
  uint64_t copies = 0;
  if (EVAL) copies = __ballot(live && lane > 0 && a.copy[pos0 + lane] != 0);
  F32x2 acc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = F32x2{1.0f + lane, 2.0f + j};
  unsigned extra = 0;
  if (START != 0) {
    const float4* tab = a.consts + static_cast<int64_t>(tile) * 16 * 64 + lane;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const float4 c = tab[j * 64];
      acc[j >> 1] += F32x2{c.x + c.z, c.y + c.w};
    }
    const int64_t v = live ? (START == 1 ? a.val_row[my_row] : a.val_pos[pos0 + lane]) : 0;
    const uint32_t word = a.amb[static_cast<uint32_t>(v) & (kAmb - 1)];
    extra = __ballot(((word >> (tile & 31)) & 1u) != 0) != 0 ? 1u : 0u;  // (as the sweep's slow_rows: wave-uniform, needed before the first row)
  }
  const int64_t col = (static_cast<int64_t>(tile) * 64 + lane) * 16;
  const bool active = col < a.stride;
  if (a.stride < 0) lds[threadIdx.x] = 1;  // never: keeps the dynamic LDS referenced
  uint4 v{1u, 2u, 3u, static_cast<unsigned>(tile) + extra};
  const F32x2 m{1.0001f, 0.9999f}, d{0.5f, 0.25f};
  for (int r = 0; r < n_rows; ++r) {
    const int64_t row = __builtin_amdgcn_readlane(my_row, r);
    if (EVAL && ((copies >> r) & 1ull) == 0) {
      for (int k = 0; k < a.k; k += 8) {
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] = __builtin_elementwise_fma(acc[j], m, d);
      }
      v.x = __float_as_uint(acc[0].x + acc[1].y + acc[2].x + acc[3].y);
      v.y = __float_as_uint(acc[4].x + acc[5].y + acc[6].x + acc[7].y);
    }
    if (active) *reinterpret_cast<uint4*>(a.out + row * a.stride + col) = v;
  }
}

// (f) NCH chunks of one tile per wave, one after the other: pair index f = u * NCH / 2 + t / 2 takes chunk f from the front of the launch
// order (even t) and chunk n_chunks - 1 - f from its back (odd t), so with the heaviest chunks first every wave carries about the same
// number of evaluated positions.  The constants are loaded once; the order -> value -> ambiguity chains of all NCH chunks are issued
// together, before the first row loop; the chunk loop stays rolled (its records rotate through registers).  A chunk that the front and
// the back would both take (an odd count's middle one) runs once: the later trip has no rows.
template <int NCH>
__global__ __launch_bounds__(256) void k_cls_multi(Args a) {
  extern __shared__ uint32_t lds[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t unit = static_cast<int64_t>(blockIdx.x) * (blockDim.x >> 6) + wave;
  const int tile = static_cast<int>(unit % a.n_tiles);
  const int64_t u = unit / a.n_tiles;
  const int64_t n_chunks = (a.rows + 63) / 64;
  if (u * NCH >= n_chunks) return;  // wave-uniform
  auto chunk_rows = [&](int t, int64_t* pos0) -> int {  // rows of trip t (0: none), scalar
    const int64_t f = u * (NCH / 2) + t / 2, b = n_chunks - 1 - f;
    const bool valid = (t & 1) ? b > f : f <= b;
    const int64_t c = (t & 1) ? b : f;
    *pos0 = valid ? c * 64 : 0;
    return valid ? static_cast<int>(c * 64 + 64 < a.rows ? 64 : a.rows - c * 64) : 0;
  };
  F32x2 acc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = F32x2{1.0f + lane, 2.0f + j};
  {
    const float4* tab = a.consts + static_cast<int64_t>(tile) * 16 * 64 + lane;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const float4 c = tab[j * 64];
      acc[j >> 1] += F32x2{c.x + c.z, c.y + c.w};
    }
  }
  int rec_row[NCH];
  uint32_t rec_copy[NCH], rec_word[NCH];
#pragma unroll
  for (int t = 0; t < NCH; ++t) {
    int64_t pos0;
    const bool live = lane < chunk_rows(t, &pos0);
    rec_row[t] = live ? min(static_cast<uint32_t>(a.perm[pos0 + lane]), static_cast<uint32_t>(a.rows - 1)) : 0;  // (clamped: no store leaves the table)
    rec_copy[t] = live && lane > 0 ? a.copy[pos0 + lane] : 0u;
  }
#pragma unroll
  for (int t = 0; t < NCH; ++t) {
    const int64_t v = a.val_row[rec_row[t]];
    rec_word[t] = a.amb[static_cast<uint32_t>(v) & (kAmb - 1)];
  }
  const int64_t col = (static_cast<int64_t>(tile) * 64 + lane) * 16;
  const bool active = col < a.stride;
  if (a.stride < 0) lds[threadIdx.x] = 1;  // never: keeps the dynamic LDS referenced
  const F32x2 m{1.0001f, 0.9999f}, d{0.5f, 0.25f};
  uint4 v{1u, 2u, 3u, static_cast<unsigned>(tile)};
#pragma unroll 1
  for (int t = 0; t < NCH; ++t) {
    int64_t pos0;
    const int n_rows = chunk_rows(t, &pos0);
    const int my_row = rec_row[0];
    const uint64_t copies = __ballot(rec_copy[0] != 0);
    v.w = static_cast<unsigned>(tile) + (__ballot(lane < n_rows && ((rec_word[0] >> (tile & 31)) & 1u) != 0) != 0 ? 1u : 0u);
#pragma unroll
    for (int k = 0; k + 1 < NCH; ++k) rec_row[k] = rec_row[k + 1], rec_copy[k] = rec_copy[k + 1], rec_word[k] = rec_word[k + 1];
    for (int r = 0; r < n_rows; ++r) {
      const int64_t row = __builtin_amdgcn_readlane(my_row, r);
      if (((copies >> r) & 1ull) == 0) {
        for (int k = 0; k < a.k; k += 8) {
#pragma unroll
          for (int j = 0; j < 8; ++j) acc[j] = __builtin_elementwise_fma(acc[j], m, d);
        }
        v.x = __float_as_uint(acc[0].x + acc[1].y + acc[2].x + acc[3].y);
        v.y = __float_as_uint(acc[4].x + acc[5].y + acc[6].x + acc[7].y);
      }
      if (active) *reinterpret_cast<uint4*>(a.out + row * a.stride + col) = v;
    }
  }
}

struct Timing { float mean, best; };
template <typename Launch>
static Timing run_launch(Launch launch) {
  float best = 1e30f, sum = 0.0f;
  const int reps = 5, per = 20;
  for (int i = 0; i < 3; ++i) launch();
  CHECK(hipDeviceSynchronize());
  hipEvent_t e0, e1;
  CHECK(hipEventCreate(&e0));
  CHECK(hipEventCreate(&e1));
  for (int rep = 0; rep < reps; ++rep) {
    CHECK(hipEventRecord(e0));
    for (int i = 0; i < per; ++i) launch();
    CHECK(hipEventRecord(e1));
    CHECK(hipEventSynchronize(e1));
    float ms;
    CHECK(hipEventElapsedTime(&ms, e0, e1));
    ms /= per;
    best = std::min(best, ms), sum += ms;
  }
  CHECK(hipGetLastError());
  CHECK(hipEventDestroy(e0));
  CHECK(hipEventDestroy(e1));
  return {sum / reps, best};
}
template <int NCH>
static Timing run_multi(const Args& a, size_t lds_bytes) {
  const int64_t n_chunks = (a.rows + 63) / 64, units = (n_chunks + NCH - 1) / NCH;
  const unsigned blocks = static_cast<unsigned>((units * a.n_tiles + 3) / 4);
  return run_launch([&] { hipLaunchKernelGGL((k_cls_multi<NCH>), dim3(blocks), dim3(256), lds_bytes, 0, a); });
}
template <bool EVAL, int START>
static Timing run(const Args& a, unsigned blocks, size_t lds_bytes) {
  return run_launch([&] { hipLaunchKernelGGL((k_cls<EVAL, START>), dim3(blocks), dim3(256), lds_bytes, 0, a); });
}

int main(int argc, char** argv) {
  if (argc < 2) {
    std::fprintf(stderr, "usage: wcls INPUT [--plain-ms MS] [--stride BYTES]\n");
    return 2;
  }
  double plain_ms = 0.24;
  int64_t stride = 10112;
  for (int i = 2; i + 1 < argc; i += 2) {
    if (!std::strcmp(argv[i], "--plain-ms")) plain_ms = std::atof(argv[i + 1]);
    else if (!std::strcmp(argv[i], "--stride")) stride = std::atoll(argv[i + 1]);
  }
  // INPUT (tools/wcls_inputs.py): int64 rows | int32 order[rows] | int64 value[rows] (by position) — the value-sorted order
  FILE* f = std::fopen(argv[1], "rb");
  int64_t rows = 0;
  if (!f || std::fread(&rows, sizeof rows, 1, f) != 1 || rows <= 0 || rows > (1 << 22) || stride <= 0 || stride % 16 != 0 || stride > 16384) {
    std::fprintf(stderr, "cannot read %s (rows in 1..2^22, stride a multiple of 16 up to 16384)\n", argv[1]);
    return 2;
  }
  std::vector<int32_t> order(rows);
  std::vector<int64_t> val(rows);
  if (std::fread(order.data(), sizeof(int32_t), rows, f) != static_cast<size_t>(rows) || std::fread(val.data(), sizeof(int64_t), rows, f) != static_cast<size_t>(rows)) {
    std::fprintf(stderr, "short input\n");
    return 2;
  }
  std::fclose(f);
  for (int64_t p = 0; p < rows; ++p)
    if (order[p] < 0 || order[p] >= rows) {
      std::fprintf(stderr, "order[%lld] out of range\n", static_cast<long long>(p));
      return 2;
    }
  const int n_tiles = static_cast<int>((stride + 1023) / 1024);
  const int64_t chunks = (rows + 63) / 64, whole = rows / 64;
  const unsigned blocks = static_cast<unsigned>((chunks * n_tiles + 3) / 4);

  // the three chunk orders: positions of the sorted order, whole chunks permuted (the last, partial one stays last)
  std::vector<int> key(whole);
  for (int64_t c = 0; c < whole; ++c) {
    int e = 1;
    for (int i = 1; i < 64; ++i) e += val[c * 64 + i] != val[c * 64 + i - 1];
    key[c] = e;
  }
  std::vector<int64_t> asc(whole), heavy(whole), inter(whole);
  std::iota(asc.begin(), asc.end(), 0);
  heavy = asc;
  std::stable_sort(heavy.begin(), heavy.end(), [&](int64_t x, int64_t y) { return key[x] > key[y]; });
  for (int64_t i = 0, lo = 0, hi = whole - 1; i < whole; ++i) inter[i] = (i & 1) ? heavy[hi--] : heavy[lo++];  // heavy, light, heavy, ...
  int64_t evaluated = rows - whole * 64 > 0 ? 1 : 0;
  for (int64_t p = whole * 64 + 1; p < rows; ++p) evaluated += val[p] != val[p - 1];
  for (int64_t c = 0; c < whole; ++c) evaluated += key[c];
  std::printf("rows %lld, chunks %lld, evaluated %lld, stride %lld, plain form %.4f ms\n", static_cast<long long>(rows), static_cast<long long>(chunks),
              static_cast<long long>(evaluated), static_cast<long long>(stride), plain_ms);

  Args a{};
  a.stride = stride, a.rows = rows, a.n_tiles = n_tiles;
  int32_t* d_perm;
  uint8_t* d_copy;
  int64_t *d_vr, *d_vp;
  uint32_t* d_amb;
  float4* d_consts;
  CHECK(hipMalloc(&a.out, rows * stride));
  CHECK(hipMalloc(&d_perm, rows * sizeof(int32_t)));
  CHECK(hipMalloc(&d_copy, rows));
  CHECK(hipMalloc(&d_vr, rows * sizeof(int64_t)));
  CHECK(hipMalloc(&d_vp, rows * sizeof(int64_t)));
  CHECK(hipMalloc(&d_amb, kAmb * sizeof(uint32_t)));
  CHECK(hipMalloc(&d_consts, static_cast<size_t>(n_tiles) * 16 * 64 * sizeof(float4)));
  CHECK(hipMemset(d_amb, 0, kAmb * sizeof(uint32_t)));
  CHECK(hipMemset(d_consts, 0, static_cast<size_t>(n_tiles) * 16 * 64 * sizeof(float4)));
  a.perm = d_perm, a.copy = d_copy, a.val_row = d_vr, a.val_pos = d_vp, a.amb = d_amb, a.consts = d_consts;
  {
    std::vector<int64_t> by_row(rows);
    for (int64_t p = 0; p < rows; ++p) by_row[order[p]] = val[p];
    CHECK(hipMemcpy(d_vr, by_row.data(), rows * sizeof(int64_t), hipMemcpyHostToDevice));
  }
  auto upload = [&](const std::vector<int64_t>& chunk_order, bool all_evaluated) {
    std::vector<int32_t> perm(rows);
    std::vector<int64_t> vp(rows);
    std::vector<uint8_t> copy(rows);
    for (int64_t p = 0; p < rows; ++p) {
      const int64_t c = p / 64, src = (c < whole ? chunk_order[c] : c) * 64 + p % 64;
      perm[p] = order[src], vp[p] = val[src];
      copy[p] = !all_evaluated && p % 64 != 0 && val[src] == val[src - 1];
    }
    CHECK(hipMemcpy(d_perm, perm.data(), rows * sizeof(int32_t), hipMemcpyHostToDevice));
    CHECK(hipMemcpy(d_vp, vp.data(), rows * sizeof(int64_t), hipMemcpyHostToDevice));
    CHECK(hipMemcpy(d_copy, copy.data(), rows, hipMemcpyHostToDevice));
  };
  const double bytes = static_cast<double>(rows) * stride;
  auto report = [&](const std::string& name, Timing t) {
    std::printf("%-64s mean %.4f ms = %.2f TB/s, best %.4f ms = %.2f TB/s\n", name.c_str(), t.mean, bytes / t.mean / 1e9, t.best, bytes / t.best / 1e9);
    std::fflush(stdout);
  };
  constexpr size_t kLds4 = 36 * 1024;  // 160 KiB of LDS per CU: four blocks (= 4 waves per SIMD) fit, a fifth does not

  // (b) calibration: every position evaluated, value order
  upload(asc, true);
  int k_cal = 8;
  for (int k = 8; k <= 256; k += 8) {
    a.k = k;
    const Timing t = run<true, 0>(a, blocks, 0);
    std::printf("calibration K = %3d: all rows evaluated, mean %.4f ms best %.4f ms\n", k, t.mean, t.best);
    k_cal = k;
    if (t.mean >= plain_ms) break;
  }
  a.k = k_cal;
  std::printf("K = %d\n", k_cal);

  upload(asc, false);
  report("(a) stores only, value order", run<false, 0>(a, blocks, 0));
  report("(a,e) stores only, 4 waves per SIMD", run<false, 0>(a, blocks, kLds4));
  report("(b) + K FMAs per evaluated position", run<true, 0>(a, blocks, 0));
  report("(b,e) ... 4 waves per SIMD", run<true, 0>(a, blocks, kLds4));
  report("(c3) + 16 constant loads, three-load chain", run<true, 1>(a, blocks, 0));
  report("(c3,e) ... 4 waves per SIMD", run<true, 1>(a, blocks, kLds4));
  report("(c2) + 16 constant loads, two-load chain", run<true, 2>(a, blocks, 0));
  report("(c2,e) ... 4 waves per SIMD", run<true, 2>(a, blocks, kLds4));
  const std::pair<const char*, const std::vector<int64_t>*> orders[] = {{"value order", &asc}, {"heaviest first", &heavy}, {"heavy / light interleaved", &inter}};
  for (const auto& o : orders) {
    upload(*o.second, false);
    report(std::string("(d) ") + o.first + ", three-load chain, 4 waves per SIMD", run<true, 1>(a, blocks, kLds4));
    report(std::string("(d) ") + o.first + ", two-load chain, 4 waves per SIMD", run<true, 2>(a, blocks, kLds4));
    report(std::string("(d) ") + o.first + ", no wave start, 4 waves per SIMD", run<true, 0>(a, blocks, kLds4));
  }
  // (f) several chunks per wave, heaviest-first order, beside the one-chunk form measured again next to them
  upload(heavy, false);
  report("(f) heaviest first, one chunk per wave (= (d)), 4 waves per SIMD", run<true, 1>(a, blocks, kLds4));
  report("(f) heaviest first, two chunks per wave (q, n-1-q), 4 waves per SIMD", run_multi<2>(a, kLds4));
  report("(f) heaviest first, four chunks per wave (q, n-1-q, q+1, n-2-q), 4 waves per SIMD", run_multi<4>(a, kLds4));
  report("(f) heaviest first, one chunk per wave, again", run<true, 1>(a, blocks, kLds4));
  CHECK(hipFree(a.out));
  return 0;
}
