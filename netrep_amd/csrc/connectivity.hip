// Module connectivity (include/netrep_gpu.h, nr_module_connectivity): for
// every node i of the resident network its connectivity to every module,
// kMod[i, m] = sum over j != i with slot[j] == m of |net[j, i]|, and to
// everything, kTotal[i] = sum over j != i of |net[j, i]|, in one pass over the
// network per module tile.
//
// connectivity_kernel: one wave (a workgroup of 64 threads) owns column i
// (grid-stride). Lane l walks rows l, l + 64, ... in increasing order; the
// element (j, i) is pairs[(i n + j) es].y in either pair layout, so a wave
// instruction reads 1 KiB (es = 1) or 2 KiB (es = 2) of contiguous memory.
// kTotal is one register accumulator per lane; the module cells are bins
// bin[m][lane] in LDS at (m 64 + lane) 8 bytes: a lane touches its own bins
// only, so there are no atomics and program order within the lane is the
// contract's order; the bank of a bin depends on the lane alone, so the
// 8-byte accesses of a wave never conflict. The column ends with the fixed
// reduction p[l] += p[l + off], off = 32 .. 1, of kTotal and of every bin, and
// lane 0 stores the cells. A wave needs no other wave: there is no barrier,
// and a workgroup of one wave lets the LDS limit occupancy in steps of one
// wave (tile 512 bytes each) instead of four.
//
// More modules than the tile run further launches over the network, kTotal in
// the first only. The bits of a cell depend on (net, slot) alone: not on the
// tile, the number of modules, the pair layout or the grid.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "kernels.h"

// Only additions occur; contraction is off all the same (and in the Makefile
// rule), as for hclust.hip.
#pragma clang fp contract(off)

namespace nr {

int connectivity_tile(int M) {
  const int passes = (M + kConnectivityTileMax - 1) / kConnectivityTileMax;
  return (M + passes - 1) / passes;
}

namespace {

constexpr int kConnUnroll = 8;  // rows a lane has in flight

__device__ __forceinline__ double conn_reduce(double v) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;  // lane 0: p[0] of the contract
}

__global__ __launch_bounds__(64) void connectivity_kernel(const double2* __restrict__ pairs, int es, int64_t n,
                                                          const int32_t* __restrict__ slot, int m_lo, int m_cnt,
                                                          double* __restrict__ k_total, double* __restrict__ k_mod) {
  extern __shared__ double bins[];  // [m_cnt][64]
  const int lane = threadIdx.x;
  for (int m = 0; m < m_cnt; ++m) bins[m * 64 + lane] = 0.0;
  // one row of this lane: the diagonal and the rows of other tiles add +0.0 or nothing (net >= 0: the same)
  auto take = [&](int64_t j, int64_t i, double y, int s, double& tot) {
    const double w = j == i ? 0.0 : fabs(y);
    tot += w;
    const unsigned b = (unsigned)(s - m_lo);  // slot -1 and the slots below m_lo wrap above m_cnt
    if (b < (unsigned)m_cnt) bins[b * 64 + lane] += w;
  };
  for (int64_t i = blockIdx.x; i < n; i += gridDim.x) {
    const double2* const col = pairs + i * n * es;
    double tot = 0.0;
    int64_t j = lane;
    for (; j + 64 * (kConnUnroll - 1) < n; j += 64 * kConnUnroll) {
      double y[kConnUnroll];
      int s[kConnUnroll];
#pragma unroll
      for (int u = 0; u < kConnUnroll; ++u) {
        y[u] = col[(j + 64 * u) * es].y;
        s[u] = slot[j + 64 * u];
      }
#pragma unroll
      for (int u = 0; u < kConnUnroll; ++u) take(j + 64 * u, i, y[u], s[u], tot);
    }
    for (; j < n; j += 64) take(j, i, col[j * es].y, slot[j], tot);
    if (k_total) {
      tot = conn_reduce(tot);
      if (lane == 0) k_total[i] = tot;
    }
    for (int m = 0; m < m_cnt; ++m) {
      double v = bins[m * 64 + lane];
      bins[m * 64 + lane] = 0.0;  // the next column's bins
      v = conn_reduce(v);
      if (lane == 0) k_mod[(int64_t)(m_lo + m) * n + i] = v;
    }
  }
}

}  // namespace

hipError_t launch_connectivity(const double2* pairs, int es, int64_t n, const int32_t* slot, int M, int tile,
                               double* k_total, double* k_mod, hipStream_t st) {
  if (M <= 0 || n <= 0) return hipSuccess;
  if (tile <= 0) tile = connectivity_tile(M);
  tile = std::min(tile, std::min(M, kConnectivityTileMax));
  const unsigned grid = (unsigned)std::min<int64_t>(n, (int64_t)1 << 16);
  for (int m_lo = 0; m_lo < M; m_lo += tile) {
    const int cnt = std::min(tile, M - m_lo);
    hipLaunchKernelGGL(connectivity_kernel, dim3(grid), dim3(64), (size_t)cnt * 64 * sizeof(double), st, pairs, es, n,
                       slot, m_lo, cnt, m_lo == 0 ? k_total : nullptr, k_mod);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace nr
