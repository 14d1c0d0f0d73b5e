// Module membership (include/netrep_gpu.h, nr_module_membership): the
// correlation of every node of the resident data block with every module
// eigengene, kME[i, m] = sum_s (x_si - mu_i) e^_sm / sqrt(sum_s (x_si - mu_i)^2).
//
// eigengene_unit_kernel writes E^ (S x M, column-major), the centred,
// unit-norm copy of the eigengenes, one workgroup per column.
//
// membership_kernel: one workgroup of 256 threads per kMembershipNodes = 16
// consecutive nodes (contiguous in the node-major data block). The 16 columns
// are staged in LDS once (their means and sums of squares are taken there),
// centred in place, and stay there while E^ passes by in tiles of
// 16 RM eigengenes (membership_tile picks RM and the sample chunk from S
// alone). Thread (node = tid & 15, group = tid >> 4) owns RM cells of the
// tile and sums each over s = 0 .. S - 1 in increasing order, one fused
// multiply-add per sample: the bits of a cell depend on S, the column and the
// eigengene only, not on M, on the eigengene's place in the call, or on the
// other nodes of the launch. No atomics; every cell is stored once.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "kernels.h"

namespace nr {

MembershipTile membership_tile(int64_t S) {
  MembershipTile t{};
  const int64_t pad = S | 1;  // odd row stride: the 16 nodes of a wave fall on distinct banks
  for (int rm : {4, 2, 1}) {
    const size_t bytes = (size_t)(kMembershipNodes + 16 * rm) * (size_t)pad * sizeof(double);
    if (bytes <= kMembershipLds) {
      t.rm = rm;
      t.chunk = (int)S;
      t.pad = (int)pad;
      t.lds = bytes;
      return t;
    }
  }
  // S beyond what one column set and one eigengene per thread hold: both are
  // walked in chunks of kMembershipChunk samples (the columns come from L2
  // again for every eigengene tile)
  t.rm = 1;
  t.chunk = kMembershipChunk;
  t.pad = kMembershipChunk | 1;
  t.lds = (size_t)(kMembershipNodes + 16) * (size_t)t.pad * sizeof(double);
  return t;
}

namespace {

__device__ __forceinline__ double wave_total(double v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// Sum of f(s) over s < S by one workgroup of 256 threads: each thread adds
// its s = tid, tid + 256, ... in increasing order, a butterfly adds the
// lanes, and the four wave totals are added in wave order. A function of S.
template <typename F>
__device__ double block_total(int64_t S, double* part, F f) {
  double a = 0.0;
  for (int64_t s = threadIdx.x; s < S; s += 256) a += f(s);
  a = wave_total(a);
  __syncthreads();  // part is free again
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = a;
  __syncthreads();
  return ((part[0] + part[1]) + part[2]) + part[3];
}

__global__ __launch_bounds__(256) void eigengene_unit_kernel(const double* __restrict__ eig, int64_t S,
                                                             double* __restrict__ ehat) {
  __shared__ double part[4];
  const double* e = eig + (int64_t)blockIdx.x * S;
  double* out = ehat + (int64_t)blockIdx.x * S;
  const double mean = block_total(S, part, [&](int64_t s) { return e[s]; }) / (double)S;
  const double ss = block_total(S, part, [&](int64_t s) {
    const double d = e[s] - mean;
    return d * d;
  });
  const double norm = sqrt(ss);
  for (int64_t s = threadIdx.x; s < S; s += 256) out[s] = (e[s] - mean) / norm;
}

template <int RM>
__global__ __launch_bounds__(256) void membership_kernel(const double* __restrict__ data, int64_t S, int64_t n,
                                                         const double* __restrict__ ehat, int M,
                                                         double* __restrict__ kme, int chunk, int pad) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __shared__ double s_mu[kMembershipNodes], s_ss[kMembershipNodes];
  double* xs = reinterpret_cast<double*>(smem);    // [16][pad] centred columns
  double* es = xs + kMembershipNodes * pad;        // [16 RM][pad] eigengene tile
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t i0 = (int64_t)blockIdx.x * kMembershipNodes;
  const int nb = (int)min((int64_t)kMembershipNodes, n - i0);  // >= 1 by the grid
  const bool resident = chunk >= S;
  // Resident columns are staged raw first, so that their statistics read LDS and not global memory.
  if (resident) {
#pragma unroll 4
    for (int j = 0; j < kMembershipNodes; ++j)
      for (int s = tid; s < (int)S; s += 256) xs[j * pad + s] = j < nb ? data[(i0 + j) * S + s] : 0.0;
    __syncthreads();
  }
  // mean and centred sum of squares of each column: wave w takes columns w, w + 4, ...; a lane adds its
  // samples lane, lane + 64, ... in increasing order and a butterfly adds the lanes (either source, same order)
  for (int j = wave; j < kMembershipNodes; j += 4) {
    double mu = 0.0, ss = 0.0;
    if (j < nb) {
      const double* x = resident ? xs + j * pad : data + (i0 + j) * S;
      double a = 0.0;
      for (int64_t s = lane; s < S; s += 64) a += x[s];
      mu = wave_total(a) / (double)S;
      double b = 0.0;
      for (int64_t s = lane; s < S; s += 64) {
        const double d = x[s] - mu;
        b += d * d;
      }
      ss = wave_total(b);
    }
    if (lane == 0) {
      s_mu[j] = mu;
      s_ss[j] = ss;
    }
  }
  __syncthreads();
  if (resident) {  // centre in place; the tile loop's first barrier orders it
#pragma unroll 4
    for (int j = 0; j < kMembershipNodes; ++j)
      for (int s = tid; s < (int)S; s += 256) xs[j * pad + s] -= s_mu[j];
  }
  // beyond the resident sizes: the columns' samples [s0, s0 + len), centred into xs (zeros past the last node)
  auto fill_columns = [&](int64_t s0, int len) {
#pragma unroll 4
    for (int j = 0; j < kMembershipNodes; ++j)
      for (int s = tid; s < len; s += 256) xs[j * pad + s] = j < nb ? data[(i0 + j) * S + s0 + s] - s_mu[j] : 0.0;
  };
  const int node = tid & (kMembershipNodes - 1), group = tid >> 4;
  const double* xr = xs + node * pad;
  const double* er = es + group * RM * pad;
  for (int m0 = 0; m0 < M; m0 += 16 * RM) {
    double acc[RM];
#pragma unroll
    for (int r = 0; r < RM; ++r) acc[r] = 0.0;
    for (int64_t s0 = 0; s0 < S; s0 += chunk) {
      const int len = (int)min((int64_t)chunk, S - s0);
      __syncthreads();  // the previous tile has been read
      if (!resident) fill_columns(s0, len);
#pragma unroll 4
      for (int c = 0; c < 16 * RM; ++c)
        for (int s = tid; s < len; s += 256) es[c * pad + s] = m0 + c < M ? ehat[(int64_t)(m0 + c) * S + s0 + s] : 0.0;
      __syncthreads();
      // unrolled so that the LDS reads of eight samples are in flight together; the sums stay in sample order
#pragma unroll 8
      for (int s = 0; s < len; ++s) {
        const double x = xr[s];
#pragma unroll
        for (int r = 0; r < RM; ++r) acc[r] = fma(x, er[r * pad + s], acc[r]);
      }
    }
    const double norm = sqrt(s_ss[node]);
#pragma unroll
    for (int r = 0; r < RM; ++r) {
      const int m = m0 + group * RM + r;
      if (node < nb && m < M) kme[(int64_t)m * n + i0 + node] = acc[r] / norm;
    }
  }
}

}  // namespace

hipError_t launch_eigengene_unit(const double* eig, int64_t S, int M, double* ehat, hipStream_t st) {
  if (M <= 0) return hipSuccess;
  hipLaunchKernelGGL(eigengene_unit_kernel, dim3((unsigned)M), dim3(256), 0, st, eig, S, ehat);
  return hipGetLastError();
}

hipError_t launch_membership(const double* data, int64_t S, int64_t n, const double* ehat, int M, double* kme,
                             hipStream_t st) {
  if (M <= 0 || n <= 0) return hipSuccess;
  const MembershipTile t = membership_tile(S);
  const dim3 grid((unsigned)((n + kMembershipNodes - 1) / kMembershipNodes));
  switch (t.rm) {
    case 4:
      hipLaunchKernelGGL(membership_kernel<4>, grid, dim3(256), t.lds, st, data, S, n, ehat, M, kme, t.chunk, t.pad);
      break;
    case 2:
      hipLaunchKernelGGL(membership_kernel<2>, grid, dim3(256), t.lds, st, data, S, n, ehat, M, kme, t.chunk, t.pad);
      break;
    default:
      hipLaunchKernelGGL(membership_kernel<1>, grid, dim3(256), t.lds, st, data, S, n, ehat, M, kme, t.chunk, t.pad);
      break;
  }
  return hipGetLastError();
}

}  // namespace nr
