// The correlation types of the from-data path other than Pearson
// (NR_COR_SPEARMAN, NR_COR_BICOR): a transient S x (n + 2) matrix Z made from
// the resident scaled block X, column by column, on which netbuild_kernel then
// runs instead of X: corr(i, j) = clamp(z_i . z_j / (S - 1), -1, 1). X itself
// stays the dataset's data block.
//
//   Spearman: z = Scale(r), r_i = L_i + (E_i + 1) / 2 with L_i the number of
//     entries of the column less than x_i and E_i the number equal to it
//     (itself included): R's rank(ties.method = "average"). Every rank is a
//     multiple of 1/2: exact. The ranks go to a plain S x n buffer and through
//     the existing scale_kernel (launch_scale), not fused, so that Z is bit
//     for bit the scaled block of a dataset whose data are those ranks.
//     +-Inf are ranked like any value; a column holding a NaN becomes NaN.
//   Bicor: WGCNA's bicor with maxPOutliers = 1, pearsonFallback "individual":
//     med = median (0.5 (lo + hi) of the order statistics at 0-based positions
//     (S - 1) / 2 and S / 2), d_i = |x_i - med|, mad = median of d (no 1.4826),
//     u_i = (x_i - med) / (9 mad), w_i = (1 - u_i^2)^2 where |u_i| < 1, else 0,
//     a_i = (x_i - med) w_i; mad == 0: a_i = x_i - mean(x) (the Pearson
//     fallback for that column alone); z_i = a_i sqrt(S - 1) / sqrt(sum a^2).
//     A column with any non-finite entry becomes NaN; an all-zero a (a
//     constant column) gives 0 / 0 = NaN.
//
// Both transforms read the *scaled* block. Both are invariant under a
// column's positive affine map, so the scaling changes nothing -- except where
// its rounding merges two distinct raw values into one (a new tie).
//
// One counting primitive serves both (cor_count): for each entry of a column,
// how many entries are less than it and how many equal it. Ranks are
// L + (E + 1) / 2; the k-th order statistic is the entry with L <= k < L + E
// (every entry tied at that position holds the same value; it is stored as
// value + 0.0, so that -0.0 and +0.0, which compare equal, store the same
// bits). Bicor's two medians, of x and then of d, are that primitive twice.
// Counting is exact, needs no atomics and does not depend on scheduling.
//
// Shape: 256-thread workgroups. Each thread owns the rows t, t + G, ... of
// its column (G threads per column) and, kCorRows owned rows at a time in
// registers, sweeps the whole column: every lane reads the same address (an
// LDS broadcast, no bank conflicts) and does 2 kCorRows compares per read.
// Columns per workgroup by S:
//   S <= kCorWaveRows : one wave per column, four columns per workgroup (at
//                       S = 500 a lane owns 8 rows: two sweeps); no workgroup
//                       barrier anywhere, the waves run independently;
//   S <= kCorLdsRows  : one workgroup per column;
//   beyond            : one workgroup per column that sweeps the column in
//                       global memory (x in X; bicor's d in the column's own
//                       slot of Z, which its z overwrites at the end).
// Sums (sum a^2, the fallback's mean) run in a fixed order: each thread over
// its rows in sequence, then wave_sum and a fixed sum over the waves in LDS
// (block_sums). Plain vector stores only.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <math.h>
#include <stdint.h>

#include "../../include/netrep_gpu.h"
#include "device_common.h"
#include "kernels.h"

namespace nr {

namespace {

constexpr int kCorRows = 4;  // owned rows a thread counts per sweep of the column

// For each v[r]: how many of col[0 .. S) are less than it, how many equal it.
// col is wave-uniform. A NaN v[r] (a row past S) counts nothing.
__device__ __forceinline__ void cor_count(const double* col, int64_t S, const double (&v)[kCorRows],
                                          int (&less)[kCorRows], int (&equal)[kCorRows]) {
#pragma unroll
  for (int r = 0; r < kCorRows; ++r) less[r] = equal[r] = 0;
#pragma unroll 4
  for (int64_t j = 0; j < S; ++j) {
    const double c = col[j];
#pragma unroll
    for (int r = 0; r < kCorRows; ++r) {
      less[r] += c < v[r] ? 1 : 0;
      equal[r] += c == v[r] ? 1 : 0;
    }
  }
}

// Barrier of the G = 64 NW threads that share a column, with a vote.
template <int NW>
__device__ __forceinline__ bool cor_any(bool p) {
  if constexpr (NW == 1) {
    nr_sync<1>();
    return __any(p) != 0;
  } else {
    return __syncthreads_or(p) != 0;
  }
}

// sel[0], sel[1] = the order statistics of col[0 .. S) at positions k_lo and
// k_hi; thread t of the column's G owns rows t, t + G, ... No barrier inside:
// the caller synchronises before it reads sel.
template <int G>
__device__ __forceinline__ void cor_order_stats(const double* col, int64_t S, int t, int64_t k_lo, int64_t k_hi,
                                                double* sel) {
  for (int64_t base = t; base < S; base += (int64_t)G * kCorRows) {
    double v[kCorRows];
    int less[kCorRows], equal[kCorRows];
#pragma unroll
    for (int r = 0; r < kCorRows; ++r) {
      const int64_t row = base + (int64_t)G * r;
      v[r] = row < S ? col[row] : nr_nan();
    }
    cor_count(col, S, v, less, equal);
#pragma unroll
    for (int r = 0; r < kCorRows; ++r) {
      if (less[r] <= k_lo && k_lo < (int64_t)less[r] + equal[r]) sel[0] = v[r] + 0.0;
      if (less[r] <= k_hi && k_hi < (int64_t)less[r] + equal[r]) sel[1] = v[r] + 0.0;
    }
  }
}

// a_i of bicor: (x - center) w with w = (1 - u^2)^2 where |u| < 1, else 0,
// u = (x - center) / (9 mad); mad == 0: x - center (center is the mean then).
// No contraction: the arithmetic is the definition's, operation by operation.
__device__ __forceinline__ double bicor_a(double x, double center, double mad) {
#pragma clang fp contract(off)
  const double dx = x - center;
  if (mad == 0.0) return dx;
  const double u = dx / (9.0 * mad);
  const double h = 1.0 - u * u;
  const double w = fabs(u) < 1.0 ? h * h : 0.0;
  return dx * w;
}

// TYPE: NR_COR_SPEARMAN (out: the plain S x n rank buffer) or NR_COR_BICOR
// (out: Z's first n columns). NW waves per column, 4 / NW columns per
// workgroup. LDS: the column (and bicor's d) staged in LDS, S <= kCorWaveRows
// (NW == 1) or kCorLdsRows (NW == 4); otherwise swept in global memory.
template <int TYPE, int NW, bool LDS>
__global__ void __launch_bounds__(256)
cor_transform_kernel(const double* __restrict__ X, int64_t S, int64_t n, double* out) {
  constexpr bool kBicor = TYPE == NR_COR_BICOR;
  constexpr int G = 64 * NW;      // threads per column
  constexpr int CPW = 4 / NW;     // columns per workgroup
  constexpr int kSlotRows = NW == 1 ? kCorWaveRows : kCorLdsRows;  // LDS rows per column
  constexpr int kColDoubles = LDS ? (kBicor ? 2 : 1) * kCorLdsRows : 0;
  static_assert(CPW * kSlotRows == kCorLdsRows, "the columns of a workgroup fill the LDS row budget");
  __shared__ double lds[kColDoubles + 32];
  const int slot = NW == 1 ? (int)(threadIdx.x >> 6) : 0;
  const int t = NW == 1 ? (int)(threadIdx.x & 63) : (int)threadIdx.x;
  double* const xs = lds + slot * ((kBicor ? 2 : 1) * kSlotRows);  // [kSlotRows] the column
  double* const ds = xs + kSlotRows;                               // [kSlotRows] bicor's d
  double* const sel = lds + kColDoubles + 4 * slot;                // [4] order statistics: x lo, hi; d lo, hi
  double* const red = lds + kColDoubles + 16;                      // [NW] block_sums
  const int64_t k_lo = (S - 1) / 2, k_hi = S / 2;

  for (int64_t g = blockIdx.x; g * CPW < n; g += gridDim.x) {
    const int64_t c = g * CPW + slot;
    if (c >= n) continue;  // NW == 1 only: wave-uniform, and that shape has no workgroup barrier
    const double* const x_glob = X + c * S;
    double* const o = out + c * S;
    bool bad = false;
    for (int64_t i = t; i < S; i += G) {
      const double x = x_glob[i];
      if (LDS) xs[i] = x;
      bad |= kBicor ? !isfinite(x) : x != x;
    }
    bad = cor_any<NW>(bad);  // and the staged column is visible
    const double* const xc = LDS ? xs : x_glob;
    if (bad) {
      for (int64_t i = t; i < S; i += G) o[i] = nr_nan();
    } else if (!kBicor) {
      for (int64_t base = t; base < S; base += (int64_t)G * kCorRows) {
        double v[kCorRows];
        int less[kCorRows], equal[kCorRows];
#pragma unroll
        for (int r = 0; r < kCorRows; ++r) {
          const int64_t row = base + (int64_t)G * r;
          v[r] = row < S ? xc[row] : nr_nan();
        }
        cor_count(xc, S, v, less, equal);
#pragma unroll
        for (int r = 0; r < kCorRows; ++r) {
          const int64_t row = base + (int64_t)G * r;
          if (row < S) o[row] = (double)less[r] + 0.5 * (double)(equal[r] + 1);
        }
      }
    } else {
      cor_order_stats<G>(xc, S, t, k_lo, k_hi, sel);
      nr_sync<NW>();
      const double med = 0.5 * (sel[0] + sel[1]);
      // d: in LDS, or in the column's slot of Z (read back through `o`, which
      // the compiler cannot take for read-only memory)
      double* const dc = LDS ? ds : o;
      for (int64_t i = t; i < S; i += G) dc[i] = fabs(xc[i] - med);
      nr_sync<NW>();
      cor_order_stats<G>(dc, S, t, k_lo, k_hi, sel + 2);
      nr_sync<NW>();
      const double mad = 0.5 * (sel[2] + sel[3]);
      double center = med;
      if (mad == 0.0) {  // the Pearson fallback: centre on the mean
        double s[1] = {0.0};
        for (int64_t i = t; i < S; i += G) s[0] += xc[i];
        block_sums<1, NW>(s, red);
        center = s[0] / (double)S;
      }
      double ss[1] = {0.0};
      for (int64_t i = t; i < S; i += G) {
        const double a = bicor_a(xc[i], center, mad);
        ss[0] += a * a;
      }
      block_sums<1, NW>(ss, red);  // every sweep of d has finished: `o` may take z
      const double num = sqrt((double)(S - 1)), den = sqrt(ss[0]);
      for (int64_t i = t; i < S; i += G) o[i] = bicor_a(xc[i], center, mad) * num / den;
    }
    nr_sync<NW>();  // the LDS column is free for the next one
  }
}

template <int TYPE>
hipError_t launch_cor_kernel(const double* X, int64_t S, int64_t n, double* out, hipStream_t st) {
  const int cpw = cor_cols_per_workgroup(S);
  const unsigned g = (unsigned)std::min<int64_t>((n + cpw - 1) / cpw, (int64_t)1 << 20);
  if (S <= kCorWaveRows)
    hipLaunchKernelGGL((cor_transform_kernel<TYPE, 1, true>), dim3(g), dim3(256), 0, st, X, S, n, out);
  else if (S <= kCorLdsRows)
    hipLaunchKernelGGL((cor_transform_kernel<TYPE, 4, true>), dim3(g), dim3(256), 0, st, X, S, n, out);
  else
    hipLaunchKernelGGL((cor_transform_kernel<TYPE, 4, false>), dim3(g), dim3(256), 0, st, X, S, n, out);
  return hipGetLastError();
}

}  // namespace

int cor_cols_per_workgroup(int64_t S) { return S <= kCorWaveRows ? 4 : 1; }

size_t cor_scratch_bytes(int64_t n, int64_t S, int cor_type) {
  if (cor_type != NR_COR_SPEARMAN && cor_type != NR_COR_BICOR) return 0;
  const size_t z = (size_t)S * (size_t)(n + 2);
  const size_t ranks = cor_type == NR_COR_SPEARMAN ? (size_t)S * (size_t)n : 0;
  return (z + ranks) * sizeof(double);
}

hipError_t launch_cor_transform(const double* X, int64_t S, int64_t n, int cor_type, double* scratch,
                                hipStream_t st) {
  double* const Z = scratch;
  double* const ranks = scratch + S * (n + 2);
  // the two padding columns: n + 1 is what netbuild_kernel reads for panel
  // columns past n; n is never read and is zeroed too
  hipError_t e = hipMemsetAsync(Z + n * S, 0, 2 * (size_t)S * sizeof(double), st);
  if (e != hipSuccess) return e;
  if (cor_type == NR_COR_SPEARMAN) {
    e = launch_cor_kernel<NR_COR_SPEARMAN>(X, S, n, ranks, st);
    if (e == hipSuccess) e = launch_scale(ranks, Z, S, n, st);
    return e;
  }
  return launch_cor_kernel<NR_COR_BICOR>(X, S, n, Z, st);
}

}  // namespace nr
