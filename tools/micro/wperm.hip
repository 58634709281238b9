// write-pattern microbenchmark, sibling of wpattern.hip: does it matter WHICH rows a wave's 64 x 1 KiB stores go to?  The table of
// config #2 (100 000 rows x 10 112 B) is written exactly as k_tlp_fast2 writes it — a wave owns (tile, chunk of 64 positions), 16 B
// per lane and row, 10 tiles, 4 waves per block — but position p of the sweep writes row perm[p]: the identity (today's sweep), a
// shuffle of the whole batch (rows sorted by pod value land anywhere in the 1 GB), and shuffles inside windows of 4 096 and 16 384
// consecutive rows.  No compute; stores only.  usage: wperm [rows] [row_stride]
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <random>
#include <vector>

#define CHECK(x)                                                                              \
  do {                                                                                        \
    hipError_t e_ = (x);                                                                      \
    if (e_ != hipSuccess) {                                                                   \
      std::fprintf(stderr, "%s: %s (line %d)\n", #x, hipGetErrorString(e_), __LINE__);        \
      std::exit(1);                                                                           \
    }                                                                                         \
  } while (0)

__global__ __launch_bounds__(256) void k_perm(uint8_t* out, const int32_t* perm, int64_t stride, int n_tiles, int64_t rows) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t unit = static_cast<int64_t>(blockIdx.x) * (blockDim.x >> 6) + wave;
  const int tile = static_cast<int>(unit % n_tiles);
  const int64_t pos0 = (unit / n_tiles) * 64;
  if (pos0 >= rows) return;  // wave-uniform
  const int n_rows = static_cast<int>(pos0 + 64 < rows ? 64 : rows - pos0);
  const int my_row = lane < n_rows ? perm[pos0 + lane] : 0;  // every lane writes it: v_readlane's source is whole
  const int64_t col = (static_cast<int64_t>(tile) * 64 + lane) * 16;
  const bool active = col < stride;
  const uint4 v{1u, 2u, 3u, static_cast<unsigned>(tile)};
  for (int r = 0; r < n_rows; ++r) {
    const int64_t row = __builtin_amdgcn_readlane(my_row, r);
    if (active) *reinterpret_cast<uint4*>(out + row * stride + col) = v;
  }
}

int main(int argc, char** argv) {
  const int64_t rows = argc > 1 ? std::atoll(argv[1]) : 100000;
  const int64_t stride = argc > 2 ? std::atoll(argv[2]) : 10112;
  if (rows <= 0 || rows > (1 << 22) || stride <= 0 || stride % 16 != 0 || stride > 16384) {
    std::fprintf(stderr, "rows in 1..2^22, row_stride a multiple of 16 up to 16384\n");
    return 2;
  }
  const int n_tiles = static_cast<int>((stride + 1023) / 1024);
  uint8_t* buf;
  int32_t* d_perm;
  CHECK(hipMalloc(&buf, rows * stride));
  CHECK(hipMalloc(&d_perm, rows * sizeof(int32_t)));
  hipEvent_t e0, e1;
  CHECK(hipEventCreate(&e0));
  CHECK(hipEventCreate(&e1));
  const int64_t chunks = (rows + 63) / 64;
  const unsigned blocks = static_cast<unsigned>((chunks * n_tiles + 3) / 4);
  std::mt19937_64 rng(20240611);
  const int64_t windows[] = {0, rows, 4096, 16384};  // 0 = identity
  const char* names[] = {"identity", "whole-batch shuffle", "shuffle in windows of 4096", "shuffle in windows of 16384"};
  for (int k = 0; k < 4; ++k) {
    std::vector<int32_t> perm(rows);
    std::iota(perm.begin(), perm.end(), 0);
    if (windows[k] > 0)
      for (int64_t w0 = 0; w0 < rows; w0 += windows[k]) std::shuffle(perm.begin() + w0, perm.begin() + std::min(rows, w0 + windows[k]), rng);
    CHECK(hipMemcpy(d_perm, perm.data(), rows * sizeof(int32_t), hipMemcpyHostToDevice));
    float best = 1e30f, sum = 0.0f;
    const int reps = 5, per = 20;
    for (int i = 0; i < 3; ++i) hipLaunchKernelGGL(k_perm, dim3(blocks), dim3(256), 0, 0, buf, d_perm, stride, n_tiles, rows);
    for (int rep = 0; rep < reps; ++rep) {
      CHECK(hipEventRecord(e0));
      for (int i = 0; i < per; ++i) hipLaunchKernelGGL(k_perm, dim3(blocks), dim3(256), 0, 0, buf, d_perm, stride, n_tiles, rows);
      CHECK(hipEventRecord(e1));
      CHECK(hipEventSynchronize(e1));
      float ms;
      CHECK(hipEventElapsedTime(&ms, e0, e1));
      ms /= per;
      best = std::min(best, ms), sum += ms;
    }
    CHECK(hipGetLastError());
    const double bytes = static_cast<double>(rows) * stride;
    std::printf("%-28s mean %.4f ms = %.2f TB/s, best %.4f ms = %.2f TB/s\n", names[k], sum / reps, bytes / (sum / reps) / 1e9, best, bytes / best / 1e9);
  }
  CHECK(hipFree(buf));
  CHECK(hipFree(d_perm));
  return 0;
}
