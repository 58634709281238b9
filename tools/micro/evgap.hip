// what a timing packet between two sweeps costs: 200 back-to-back launches of wcls.hip's store kernel (a wave owns (tile, chunk of 64
// rows), 16 B per lane and row, 10 tiles, 4 waves per block, 100 000 x 10 112 B, rows in place) on one stream inside one outer event
// pair, with one of these between consecutive launches:
//   (a) nothing;
//   (b) two hipEventRecords on default-flag events — what spx_eval does (ev1 after its launches, ev0 before the next call's);
//   (c) the same on events created with hipEventDisableSystemFence;
//   (d) hipEventRecord for the start, the stop event handed to hipExtLaunchKernelGGL;
//   (e) both events handed to hipExtLaunchKernelGGL;
//   (f), (g) as (d) and (e) with events created with hipEventDisableSystemFence.
// Per variant: the outer time per launch (mean and best of 5 series), and "inner against outer" — the variant's own event pair round
// ONE launch beside an outer default-flag pair recorded round that launch alone, five times.  A variant whose inner figure is not the
// launch's duration cannot serve spx_last_eval_ms, whatever it saves.
// usage: evgap [--rows 100000] [--stride 10112] [--launches 200]
#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#define CHECK(x)                                                                              \
  do {                                                                                        \
    hipError_t e_ = (x);                                                                      \
    if (e_ != hipSuccess) {                                                                   \
      std::fprintf(stderr, "%s: %s (line %d)\n", #x, hipGetErrorString(e_), __LINE__);        \
      std::exit(1);                                                                           \
    }                                                                                         \
  } while (0)

struct Args {
  uint8_t* out;
  int64_t stride, rows;
  int n_tiles;
};

__global__ __launch_bounds__(256) void k_store(Args a) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t unit = static_cast<int64_t>(blockIdx.x) * (blockDim.x >> 6) + wave;
  const int tile = static_cast<int>(unit % a.n_tiles);
  const int64_t row0 = (unit / a.n_tiles) * 64;
  if (row0 >= a.rows) return;  // wave-uniform
  const int n_rows = static_cast<int>(row0 + 64 < a.rows ? 64 : a.rows - row0);
  const int64_t col = (static_cast<int64_t>(tile) * 64 + lane) * 16;
  if (col >= a.stride) return;  // (stride is a multiple of 16: the 16 bytes stay inside the row)
  const uint4 v{1u, 2u, 3u, static_cast<unsigned>(tile)};
  for (int r = 0; r < n_rows; ++r) *reinterpret_cast<uint4*>(a.out + (row0 + r) * a.stride + col) = v;
}

enum Variant { kNone, kRecord, kRecordNoFence, kExtStop, kExtBoth, kExtStopNoFence, kExtBothNoFence };
static const char* const kNames[] = {"(a) nothing between launches", "(b) two hipEventRecords, default flags", "(c) two hipEventRecords, hipEventDisableSystemFence",
                                     "(d) hipEventRecord start, stop event on the dispatch (hipExtLaunchKernelGGL)", "(e) both events on the dispatch (hipExtLaunchKernelGGL)",
                                     "(f) as (d), hipEventDisableSystemFence", "(g) as (e), hipEventDisableSystemFence"};

struct Ctx {
  Args a;
  unsigned blocks;
  hipStream_t s;
  hipEvent_t i0, i1;  // the variant's pair
};

// one step as the variant times it
static void step(const Ctx& c, Variant v) {
  switch (v) {
    case kNone:
      hipLaunchKernelGGL(k_store, dim3(c.blocks), dim3(256), 0, c.s, c.a);
      break;
    case kRecord:
    case kRecordNoFence:
      CHECK(hipEventRecord(c.i0, c.s));
      hipLaunchKernelGGL(k_store, dim3(c.blocks), dim3(256), 0, c.s, c.a);
      CHECK(hipEventRecord(c.i1, c.s));
      break;
    case kExtStop:
    case kExtStopNoFence:
      CHECK(hipEventRecord(c.i0, c.s));
      hipExtLaunchKernelGGL(k_store, dim3(c.blocks), dim3(256), 0, c.s, nullptr, c.i1, 0, c.a);
      break;
    case kExtBoth:
    case kExtBothNoFence:
      hipExtLaunchKernelGGL(k_store, dim3(c.blocks), dim3(256), 0, c.s, c.i0, c.i1, 0, c.a);
      break;
  }
}

int main(int argc, char** argv) {
  int64_t rows = 100000, stride = 10112;
  int launches = 200;
  for (int i = 1; i + 1 < argc; i += 2) {
    if (!std::strcmp(argv[i], "--rows")) rows = std::atoll(argv[i + 1]);
    else if (!std::strcmp(argv[i], "--stride")) stride = std::atoll(argv[i + 1]);
    else if (!std::strcmp(argv[i], "--launches")) launches = std::atoi(argv[i + 1]);
  }
  if (rows <= 0 || rows > (1 << 22) || stride <= 0 || stride % 16 != 0 || stride > 16384 || launches < 1 || launches > 10000) {
    std::fprintf(stderr, "rows in 1..2^22, stride a multiple of 16 up to 16384, launches in 1..10000\n");
    return 2;
  }
  Ctx c{};
  c.a.stride = stride, c.a.rows = rows, c.a.n_tiles = static_cast<int>((stride + 1023) / 1024);
  c.blocks = static_cast<unsigned>(((rows + 63) / 64 * c.a.n_tiles + 3) / 4);
  CHECK(hipMalloc(&c.a.out, static_cast<size_t>(rows) * stride));
  CHECK(hipStreamCreate(&c.s));
  hipEvent_t o0, o1;
  CHECK(hipEventCreate(&o0));
  CHECK(hipEventCreate(&o1));
  std::printf("rows %lld, stride %lld, %d launches per series\n", static_cast<long long>(rows), static_cast<long long>(stride), launches);
  for (int vi = kNone; vi <= kExtBothNoFence; ++vi) {
    const Variant v = static_cast<Variant>(vi);
    const unsigned flags = (v == kRecordNoFence || v == kExtStopNoFence || v == kExtBothNoFence) ? hipEventDisableSystemFence : hipEventDefault;
    CHECK(hipEventCreateWithFlags(&c.i0, flags));
    CHECK(hipEventCreateWithFlags(&c.i1, flags));
    for (int i = 0; i < 5; ++i) step(c, v);
    CHECK(hipStreamSynchronize(c.s));
    float best = 1e30f, sum = 0.0f;
    for (int rep = 0; rep < 5; ++rep) {
      CHECK(hipEventRecord(o0, c.s));
      for (int i = 0; i < launches; ++i) step(c, v);
      CHECK(hipEventRecord(o1, c.s));
      CHECK(hipEventSynchronize(o1));
      float ms;
      CHECK(hipEventElapsedTime(&ms, o0, o1));
      ms /= launches;
      best = std::min(best, ms), sum += ms;
    }
    std::printf("%-84s outer per launch: mean %.4f ms, best %.4f ms\n", kNames[vi], sum / 5, best);
    if (v != kNone) {
      std::printf("    inner / outer of one launch (ms):");
      for (int rep = 0; rep < 5; ++rep) {
        CHECK(hipStreamSynchronize(c.s));
        CHECK(hipEventRecord(o0, c.s));
        step(c, v);
        CHECK(hipEventRecord(o1, c.s));
        CHECK(hipEventSynchronize(o1));
        float outer, inner = -1.0f;
        CHECK(hipEventElapsedTime(&outer, o0, o1));
        const hipError_t st = hipEventSynchronize(c.i1) != hipSuccess ? hipErrorUnknown : hipEventElapsedTime(&inner, c.i0, c.i1);
        if (st != hipSuccess) {
          (void)hipGetLastError();
          std::printf("  (%s) / %.4f", hipGetErrorName(st), outer);
        } else {
          std::printf("  %.4f / %.4f", inner, outer);
        }
      }
      std::printf("\n");
    }
    std::fflush(stdout);
    CHECK(hipStreamSynchronize(c.s));
    CHECK(hipEventDestroy(c.i0));
    CHECK(hipEventDestroy(c.i1));
  }
  CHECK(hipGetLastError());
  CHECK(hipFree(c.a.out));
  return 0;
}
