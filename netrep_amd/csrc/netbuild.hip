// The from-data path (nr_set_dataset_from_data): the resident {corr, net} pair
// array computed on the device from the scaled data block, as the reference's
// example data derives it on the host (R/example-data.R:111-116: cor(data),
// abs(correlation)^5), and the export of a resident pair array back to two
// plain matrices (nr_get_dataset_matrices).
//
// netbuild_kernel: a lower-triangle SYRK on v_mfma_f64_16x16x4_f64. One
// 256-thread workgroup owns one kNetbuildTile x kNetbuildTile (64 x 64) tile
// (I, J), I >= J, of g = X^T X; its four waves own one 32 x 32 quadrant each
// (2 x 2 MFMA tiles). The two 64-column panels go through LDS in chunks of
// kNbChunk samples: every operand element is fetched from global memory once
// per workgroup tile, and the next chunk's loads are in flight while the
// current one is multiplied. The epilogue turns g into {c, w} per element and
// stores the tile twice, at (i, j) and -- the same bits -- at (j, i). Both
// stores go through an LDS image of half the tile so that each wave
// instruction writes 16 bytes per lane along contiguous rows of the
// column-major array: neither store is strided by n.
//
// tom_kernel (NR_NET_TOM) and soft_connectivity_kernel (nr_soft_connectivity:
// the soft-threshold connectivities, no n x n array stored) run the same main
// loop, nb_syrk_tile, with epilogues of their own; see there.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <math.h>
#include <stdint.h>

#include "../../include/netrep_gpu.h"
#include "kernels.h"

namespace nr {

namespace {

typedef double nb_f64x4 __attribute__((ext_vector_type(4)));

constexpr int kNbTile = kNetbuildTile;  // 64: output tile side per workgroup
constexpr int kNbChunk = 32;            // samples per LDS chunk (8 MFMA K-steps)
// Doubles per panel column in LDS: kNbChunk + 2. A lane reads 16 bytes at
// column * 272 + const, so 8 consecutive lanes (the group one ds_read_b128
// cycle serves) fall on banks 0, 4, ..., 28 (+ const): conflict-free.
constexpr int kNbLd = kNbChunk + 2;
// The epilogue's LDS images of half a tile (32 columns j x 64 rows i): g as
// doubles, then {c, w} as double2, both with 65 elements per column (130 / 260
// dwords = 2 / 4 mod 64): conflict-free for the 8-byte writes of the MFMA
// layout and for the 16-byte accesses along either direction.
constexpr int kNbOutLd = kNbTile + 1;
constexpr int kNbPanelDoubles = 2 * kNbTile * kNbLd;       // 4,352 doubles = 34,816 bytes
constexpr int kNbHalfG = (kNbTile / 2) * kNbOutLd;         // 2,080 doubles
constexpr int kNbStageDoubles = kNbHalfG + 2 * kNbHalfG;   // 6,240 doubles = 49,920 bytes
constexpr int kNbLdsDoubles = kNbPanelDoubles > kNbStageDoubles ? kNbPanelDoubles : kNbStageDoubles;

// The lower-triangle tile (I, J), I >= J, of linear index t = I (I + 1) / 2 + J.
__device__ __forceinline__ void tile_of(int64_t t, int64_t& I, int64_t& J) {
  int64_t i = (int64_t)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
  while (i * (i + 1) / 2 > t) --i;
  while ((i + 1) * (i + 2) / 2 <= t) ++i;
  I = i;
  J = t - i * (i + 1) / 2;
}

// c -> w of the three network types through one pow; NaN in, NaN out (the
// hybrid's test is written so that it is false for NaN).
__device__ __forceinline__ double net_weight(double c, int net_type, double beta) {
  const double base = net_type == NR_NET_UNSIGNED ? fabs(c) : (net_type == NR_NET_SIGNED ? (1.0 + c) * 0.5 : c);
  const double w = pow(base, beta);
  return net_type == NR_NET_SIGNED_HYBRID && c <= 0.0 ? 0.0 : w;
}

// One chunk of a thread's share of both panels: 4 + 4 double2, rows
// [s0 + 2 (t & 15), + 2) of columns (t >> 4) + 16 p of panel A (tile I) and B
// (tile J). Columns past n read the block's zero column. Branch-free, so that
// the eight loads are in flight together: a whole chunk (FULL) loads 16 bytes
// per column; the last, partial chunk loads each row from an address clamped
// into the column and zeroes the rows past S afterwards.
struct NbFetch {
  double2 a[4], b[4];
};

template <bool FULL>
__device__ __forceinline__ void nb_fetch(const double* __restrict__ X, int64_t S, const int64_t (&col_a)[4],
                                         const int64_t (&col_b)[4], int64_t s0, NbFetch& f) {
  const int64_t r = s0 + 2 * (threadIdx.x & 15);
  if (FULL) {
#pragma unroll
    for (int p = 0; p < 4; ++p) {  // columns start at any multiple of 8 bytes (S odd): memcpy, not a double2 load
      __builtin_memcpy(&f.a[p], X + col_a[p] + r, sizeof(double2));
      __builtin_memcpy(&f.b[p], X + col_b[p] + r, sizeof(double2));
    }
  } else {
    const int64_t r0 = r < S ? r : S - 1, r1 = r + 1 < S ? r + 1 : S - 1;
    const double m0 = r < S ? 1.0 : 0.0, m1 = r + 1 < S ? 1.0 : 0.0;
    double t[4][4];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      t[p][0] = X[col_a[p] + r0];
      t[p][1] = X[col_a[p] + r1];
      t[p][2] = X[col_b[p] + r0];
      t[p][3] = X[col_b[p] + r1];
    }
#pragma unroll
    for (int p = 0; p < 4; ++p) {  // selects, not products: a NaN or Inf above the clamp must not leak
      f.a[p] = make_double2(m0 != 0.0 ? t[p][0] : 0.0, m1 != 0.0 ? t[p][1] : 0.0);
      f.b[p] = make_double2(m0 != 0.0 ? t[p][2] : 0.0, m1 != 0.0 ? t[p][3] : 0.0);
    }
  }
}

// This thread's share of a chunk into the panels.
__device__ __forceinline__ void nb_to_lds(double* pA, double* pB, const NbFetch& f) {
  const int kp = 2 * (threadIdx.x & 15), c0 = threadIdx.x >> 4;
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    *reinterpret_cast<double2*>(pA + (c0 + 16 * p) * kNbLd + kp) = f.a[p];
    *reinterpret_cast<double2*>(pB + (c0 + 16 * p) * kNbLd + kp) = f.b[p];
  }
}

// The wave's 2 x 2 MFMA tiles over one chunk in LDS: lane (i16, kk) feeds rows
// 8 kk .. 8 kk + 7 of the chunk, one per MFMA (the same rows on both operands;
// which row goes with which K-step only permutes the sum).
__device__ __forceinline__ void nb_multiply(const double* pA, const double* pB, int wr, int wc, int i16, int kk,
                                            nb_f64x4 (&acc)[2][2]) {
  double va[2][8], vb[2][8];
#pragma unroll
  for (int a = 0; a < 2; ++a) {
    const double* ra = pA + (32 * wr + 16 * a + i16) * kNbLd + 8 * kk;
    const double* rb = pB + (32 * wc + 16 * a + i16) * kNbLd + 8 * kk;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const double2 x = *reinterpret_cast<const double2*>(ra + 2 * q);
      const double2 y = *reinterpret_cast<const double2*>(rb + 2 * q);
      va[a][2 * q] = x.x;
      va[a][2 * q + 1] = x.y;
      vb[a][2 * q] = y.x;
      vb[a][2 * q + 1] = y.y;
    }
  }
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(va[0][q], vb[0][q], acc[0][0], 0, 0, 0);
    acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(va[0][q], vb[1][q], acc[0][1], 0, 0, 0);
    acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(va[1][q], vb[0][q], acc[1][0], 0, 0, 0);
    acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(va[1][q], vb[1][q], acc[1][1], 0, 0, 0);
  }
}

// acc = this wave's quadrant of tile (I, J) of X^T X, X an S x (n + 2)
// column-major block whose column n + 1, at offset zero_col, is zero (columns
// past n read it): whole chunks, the next chunk's loads in flight while this
// one is multiplied; the last, partial chunk (its own code, so that its waits
// never sit in the whole chunks' path) after them. The panels are free on
// return. Shared by netbuild_kernel (X the data block) and tom_kernel (X the
// adjacency scratch, S = n).
__device__ __forceinline__ void nb_syrk_tile(const double* __restrict__ X, int64_t S, int64_t n, int64_t zero_col,
                                             int64_t I, int64_t J, double* pA, double* pB, int wr, int wc, int i16,
                                             int kk, nb_f64x4 (&acc)[2][2]) {
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) acc[a][b] = nb_f64x4{0.0, 0.0, 0.0, 0.0};

  int64_t col_a[4], col_b[4];  // offsets of this thread's panel columns in X
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const int64_t ca = I * kNbTile + (threadIdx.x >> 4) + 16 * p, cb = J * kNbTile + (threadIdx.x >> 4) + 16 * p;
    col_a[p] = ca < n ? ca * S : zero_col;
    col_b[p] = cb < n ? cb * S : zero_col;
  }
  const int64_t s_full = S / kNbChunk * kNbChunk;
  NbFetch f;
  if (s_full > 0) nb_fetch<true>(X, S, col_a, col_b, 0, f);
  for (int64_t s0 = 0; s0 < s_full; s0 += kNbChunk) {
    nb_to_lds(pA, pB, f);
    __syncthreads();
    if (s0 + kNbChunk < s_full) nb_fetch<true>(X, S, col_a, col_b, s0 + kNbChunk, f);
    nb_multiply(pA, pB, wr, wc, i16, kk, acc);
    __syncthreads();  // the panels are free (for the next chunk, or the output image)
  }
  if (s_full < S) {
    nb_fetch<false>(X, S, col_a, col_b, s_full, f);
    nb_to_lds(pA, pB, f);
    __syncthreads();
    nb_multiply(pA, pB, wr, wc, i16, kk, acc);
    __syncthreads();
  }
}

__global__ void __launch_bounds__(256, 2)
netbuild_kernel(const double* __restrict__ X, int64_t S, int64_t n, double2* __restrict__ pairs, int net_type,
                double beta, int* __restrict__ flags) {
  __shared__ __attribute__((aligned(16))) double lds[kNbLdsDoubles];
  double* const pA = lds;                       // [64 columns][kNbLd]
  double* const pB = lds + kNbTile * kNbLd;
  double* const stage_g = lds;                                          // [32 columns j][kNbOutLd rows i]
  double2* const stage = reinterpret_cast<double2*>(lds + kNbHalfG);    // the same shape, {c, w}

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i16 = lane & 15, kk = lane >> 4;
  const int wr = wave & 1, wc = wave >> 1;  // the wave's quadrant: rows 32 wr.., columns 32 wc..
  const int64_t nT = (n + kNbTile - 1) / kNbTile;
  const int64_t n_tiles = nT * (nT + 1) / 2;
  const int64_t zero_col = (n + 1) * S;
  const double denom = (double)(S - 1);
  int bad = 0;

  for (int64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    int64_t I, J;
    tile_of(t, I, J);
    const bool diag = I == J;

    nb_f64x4 acc[2][2];
    nb_syrk_tile(X, S, n, zero_col, I, J, pA, pB, wr, wc, i16, kk, acc);

    // Epilogue, one half of the tile's columns (held by the waves wc == h) at
    // a time: g into stage_g[j][i]; every thread turns 8 elements into {c, w}
    // in stage[j][i]; then out along i (the (i, j) store) and along j (the
    // mirror at (j, i)).
    for (int h = 0; h < 2; ++h) {
      if (wc == h) {
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
          for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 4; ++r)
              // D[row = (lane >> 4) + 4 r][col = lane & 15] (f64 MFMA C/D map)
              stage_g[(16 * b + i16) * kNbOutLd + 32 * wr + 16 * a + kk + 4 * r] = acc[a][b][r];
      }
      __syncthreads();
#pragma unroll 1
      for (int q = 0; q < 8; ++q) {
        const int il = lane, jl = wave + 4 * q;
        const int64_t gi = I * kNbTile + il, gj = J * kNbTile + 32 * h + jl;
        double c = stage_g[jl * kNbOutLd + il] / denom;
        c = c > 1.0 ? 1.0 : (c < -1.0 ? -1.0 : c);  // R's cor clamps; NaN stays NaN
        const double w = net_weight(c, net_type, beta);
        if (gi < n && gj < n && (!diag || gi >= gj)) bad |= (isfinite(c) ? 0 : 2) | (isfinite(w) ? 0 : 4);
        stage[jl * kNbOutLd + il] = make_double2(c, w);
      }
      __syncthreads();
      // (i, j): one column of 64 rows per wave instruction (1 KiB contiguous)
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int jl = 8 * wave + q;
        const int64_t gi = I * kNbTile + lane, gj = J * kNbTile + 32 * h + jl;
        if (gi < n && gj < n && (!diag || gi >= gj)) pairs[gi + gj * n] = stage[jl * kNbOutLd + lane];
      }
      // (j, i): two rows i of 32 columns j per wave instruction (2 x 512 contiguous bytes)
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int il = 16 * wave + 2 * q + (lane >> 5), jl = lane & 31;
        const int64_t gi = I * kNbTile + il, gj = J * kNbTile + 32 * h + jl;
        if (gi < n && gj < n && (!diag || gi >= gj)) pairs[gj + gi * n] = stage[jl * kNbOutLd + il];
      }
      __syncthreads();
    }
  }
  // one reduction per wave, one atomic per wave that saw a non-finite value
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) bad |= __shfl_xor(bad, o, 64);
  if (bad && lane == 0) atomicOr(flags, bad);
}

// ---- topological overlap (NR_NET_TOM) ---------------------------------------
//
// The TOM scratch matrix A: the adjacency (the pairs' .y) with a zero
// diagonal, column-major, n rows and n + 2 columns, so that tom_kernel can
// hand it to the SYRK main loop as "X with S = n". Padding rule (the data
// block's, restated): columns 0 .. n - 1 hold values; column n + 1 is all
// zeros and is what every panel column past n reads; column n (the data
// block's ones column) is never read by the main loop and is zeroed too, so
// that no byte of the scratch is left undefined.
//
// tom_extract_kernel: one workgroup per column j (grid-stride): A(:, j) from
// the pairs, and the degree k_j = sum_i A(i, j) in one fixed order: thread t
// adds rows t, t + 256, ... in sequence, then a fixed LDS tree over the 256
// partial sums. No atomics: k does not depend on scheduling.
__global__ void __launch_bounds__(256)
tom_extract_kernel(const double2* __restrict__ pairs, int64_t n, double* __restrict__ A, double* __restrict__ k) {
  __shared__ double part[256];
  for (int64_t j = blockIdx.x; j < n + 2; j += gridDim.x) {
    double* const col = A + j * n;
    if (j >= n) {  // the two padding columns
      for (int64_t i = threadIdx.x; i < n; i += 256) col[i] = 0.0;
      continue;
    }
    double sum = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += 256) {
      const double a = i == j ? 0.0 : pairs[i + j * n].y;
      col[i] = a;
      sum += a;
    }
    part[threadIdx.x] = sum;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
      if ((int)threadIdx.x < o) part[threadIdx.x] += part[threadIdx.x + o];
      __syncthreads();
    }
    if (threadIdx.x == 0) k[j] = part[0];
    __syncthreads();  // part is free for the next column
  }
}

// t_ij of WGCNA's unsigned TOM (TOMDenom = "min") from L_ij = sum_u a_iu a_uj,
// a_ij and the two degrees. The minimum is two selects that keep a NaN of
// either degree (fmin would drop it); the denominator is >= 1.
__device__ __forceinline__ double tom_value(double L, double a, double ki, double kj) {
  double m = ki < kj ? ki : kj;  // kj where kj is NaN
  m = ki == ki ? m : ki;         // ki where ki is NaN
  return (L + a) / (m + 1.0 - a);
}

// tom_kernel: the same lower-triangle SYRK as netbuild_kernel, over A with
// K = n (main loop: nb_syrk_tile, which reads A only, never the pairs), and
// its own epilogue: t_ij from L, a_ij (read from A), k_i and k_j, 1 on the
// diagonal; stored into the .y of pair (i, j) and -- the same bits -- of
// (j, i) as 8-byte stores, so the .x (corr) keeps its bits. A tile reads and
// writes only its own (i, j) and (j, i), so the update is in place. flags
// |= 4 for a non-finite t.
__global__ void __launch_bounds__(256, 2)
tom_kernel(const double* __restrict__ A, const double* __restrict__ k, int64_t n, double2* __restrict__ pairs,
           int* __restrict__ flags) {
  __shared__ __attribute__((aligned(16))) double lds[kNbPanelDoubles];
  double* const pA = lds;
  double* const pB = lds + kNbTile * kNbLd;
  double* const stage_t = lds;  // [32 columns j][kNbOutLd rows i]: L, then t in place
  double* const net = reinterpret_cast<double*>(pairs) + 1;  // net[2 e]: the .y of pair e

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i16 = lane & 15, kk = lane >> 4;
  const int wr = wave & 1, wc = wave >> 1;
  const int64_t nT = (n + kNbTile - 1) / kNbTile;
  const int64_t n_tiles = nT * (nT + 1) / 2;
  const int64_t zero_col = (n + 1) * n;  // A's second padding column
  int bad = 0;

  for (int64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    int64_t I, J;
    tile_of(t, I, J);
    const bool diag = I == J;

    nb_f64x4 acc[2][2];
    nb_syrk_tile(A, n, n, zero_col, I, J, pA, pB, wr, wc, i16, kk, acc);

    for (int h = 0; h < 2; ++h) {
      if (wc == h) {
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
          for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 4; ++r)
              stage_t[(16 * b + i16) * kNbOutLd + 32 * wr + 16 * a + kk + 4 * r] = acc[a][b][r];
      }
      __syncthreads();
      // every thread turns its own 8 elements of L into t in place
      const int64_t gi = I * kNbTile + lane;
      const double ki = gi < n ? k[gi] : 0.0;
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int jl = wave + 4 * q;
        const int64_t gj = J * kNbTile + 32 * h + jl;
        const bool in = gi < n && gj < n;
        const double a = in ? A[gi + gj * n] : 0.0;
        const double kj = gj < n ? k[gj] : 0.0;
        double tv = tom_value(stage_t[jl * kNbOutLd + lane], a, ki, kj);
        tv = gi == gj ? 1.0 : tv;
        if (in && (!diag || gi >= gj)) bad |= isfinite(tv) ? 0 : 4;
        stage_t[jl * kNbOutLd + lane] = tv;
      }
      __syncthreads();
      // (i, j): one column of 64 rows per wave instruction
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int jl = 8 * wave + q;
        const int64_t gj = J * kNbTile + 32 * h + jl;
        if (gi < n && gj < n && (!diag || gi >= gj)) net[2 * (gi + gj * n)] = stage_t[jl * kNbOutLd + lane];
      }
      // (j, i): two rows i of 32 columns j per wave instruction
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int il = 16 * wave + 2 * q + (lane >> 5), jl = lane & 31;
        const int64_t mi = I * kNbTile + il, mj = J * kNbTile + 32 * h + jl;
        if (mi < n && mj < n && (!diag || mi >= mj)) net[2 * (mj + mi * n)] = stage_t[jl * kNbOutLd + il];
      }
      __syncthreads();
    }
  }
  // one reduction per wave, one atomic per wave that saw a non-finite value
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) bad |= __shfl_xor(bad, o, 64);
  if (bad && lane == 0) atomicOr(flags, bad);
}

// ---- soft-threshold connectivities (nr_soft_connectivity) -------------------
//
// The distinct powers of a call in ascending order are its "slots";
// slot_of[m] is the slot of the caller's m-th power (duplicates share one). A
// launch of soft_connectivity_kernel takes up to kSftChainSlots (chain path)
// or kSftPowSlots (pow path: that many inlined pows fit the register budget
// of two workgroups per CU without a spill) of them, slots slot0 .. slot0 +
// n_slots - 1 of n_slots_total, one running sum in registers each: for the
// chain path step[s] is the number of multiplications by b that lead from the
// launch's slot s - 1 (from b itself for s = 0) to slot s; for the pow path
// p[s] is the power.
constexpr int kSftChainSlots = 16;
constexpr int kSftPowSlots = 8;
constexpr int kSftLaunchSlots = kSftChainSlots > kSftPowSlots ? kSftChainSlots : kSftPowSlots;
struct SftPowers {
  int n_slots, slot0, n_slots_total;
  int step[kSftLaunchSlots];
  double p[kSftLaunchSlots];
};
struct SftSlots {
  int slot_of[kSftMaxPowers];
};

// c of the SYRK's g as netbuild_kernel's epilogue computes it, and the base b
// the powers are taken of: NaN in, NaN out (the hybrid's test is false for NaN).
__device__ __forceinline__ double sft_base(double g, double denom, int net_type) {
  double c = g / denom;
  c = c > 1.0 ? 1.0 : (c < -1.0 ? -1.0 : c);  // R's cor clamps; NaN stays NaN
  return net_type == NR_NET_UNSIGNED ? fabs(c) : (net_type == NR_NET_SIGNED ? (1.0 + c) * 0.5 : (c <= 0.0 ? 0.0 : c));
}

constexpr int kSftRows = kNbTile / 4;   // rows of a tile per thread: wave w owns rows 16 w .. 16 w + 15
constexpr int kSftBatch = 8;            // of which the chain path holds this many in registers at a time
static_assert(kNbTile * kNbOutLd <= kNbPanelDoubles, "the whole tile's g is staged in the panels' LDS");
static_assert(4 * kSftLaunchSlots * kNbTile <= kNbPanelDoubles, "so are the four partial sums per slot and column");
static_assert(kSftChainSlots % 4 == 0 && kSftPowSlots % 4 == 0,
              "the strip-end combine gives every thread slots / 4 sums to finish");

// soft_connectivity_kernel: workgroup (J, r) = blockIdx.(x, y) owns columns
// 64 J .. 64 J + 63 and the row tiles [r tiles_per_group, (r + 1)
// tiles_per_group) of the FULL matrix (not the lower triangle: twice the SYRK
// flops, for no n^2 scratch and no dependency between tiles). Per tile: the
// SYRK main loop, g staged whole in LDS as stage[j][i] (kNbOutLd per column),
// then thread (wave w, lane l) reads rows 16 w .. 16 w + 15 of column l --
// the column index is in the lane, so the odd stride is conflict-free -- and
// adds b^p to its n_slots running sums, in increasing row order. Rows and
// columns past n and the diagonal enter as b = 0 (a select: a NaN there must
// not leak), which adds +0 for every power > 0. At the strip's end the four
// threads of a column add up in wave order and part[(r n_slots_total + slot0
// + s) n + j] is written with plain stores, 64 consecutive j per wave
// instruction. A group without row tiles writes zeros.
template <bool CHAIN>
__global__ void __launch_bounds__(256, 2)
soft_connectivity_kernel(const double* __restrict__ X, int64_t S, int64_t n, int net_type, SftPowers pw,
                         int64_t tiles_per_group, double* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) double lds[kNbPanelDoubles];
  double* const pA = lds;
  double* const pB = lds + kNbTile * kNbLd;
  double* const stage = lds;  // [64 columns j][kNbOutLd rows i]
  // the slots' steps / powers, read where they are used (by value they would
  // sit in scalar registers for the whole kernel)
  __shared__ double slot_p[kSftLaunchSlots];
  __shared__ int slot_step[kSftLaunchSlots];
  if (threadIdx.x < kSftLaunchSlots) {
    slot_p[threadIdx.x] = pw.p[threadIdx.x];
    slot_step[threadIdx.x] = pw.step[threadIdx.x];
  }
  __syncthreads();
  const int n_slots = pw.n_slots;
  constexpr int NS = CHAIN ? kSftChainSlots : kSftPowSlots;

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i16 = lane & 15, kk = lane >> 4;
  const int wr = wave & 1, wc = wave >> 1;
  const int64_t nT = (n + kNbTile - 1) / kNbTile;
  const int64_t zero_col = (n + 1) * S;
  const double denom = (double)(S - 1);
  const int64_t J = blockIdx.x, r = blockIdx.y;
  const int64_t gj = J * kNbTile + lane;
  const int64_t I0 = r * tiles_per_group;
  const int64_t I1 = I0 + tiles_per_group < nT ? I0 + tiles_per_group : nT;

  double sum[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) sum[s] = 0.0;

  for (int64_t I = I0; I < I1; ++I) {
    nb_f64x4 acc[2][2];
    nb_syrk_tile(X, S, n, zero_col, I, J, pA, pB, wr, wc, i16, kk, acc);
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int q = 0; q < 4; ++q)
          // D[row = (lane >> 4) + 4 q][col = lane & 15] (f64 MFMA C/D map)
          stage[(32 * wc + 16 * b + i16) * kNbOutLd + 32 * wr + 16 * a + kk + 4 * q] = acc[a][b][q];
    __syncthreads();
    const double* const col = stage + lane * kNbOutLd + kSftRows * wave;
    const int64_t gi0 = I * kNbTile + kSftRows * wave;
    if (CHAIN) {
#pragma unroll 1
      for (int h = 0; h < kSftRows / kSftBatch; ++h) {
        double b[kSftBatch], v[kSftBatch];
#pragma unroll
        for (int q = 0; q < kSftBatch; ++q) {
          const int64_t gi = gi0 + kSftBatch * h + q;
          const double x = sft_base(col[kSftBatch * h + q], denom, net_type);
          b[q] = gi < n && gj < n && gi != gj ? x : 0.0;
          v[q] = b[q];
        }
#pragma unroll
        for (int s = 0; s < NS; ++s) {
          if (s < n_slots) {
            const int steps = __builtin_amdgcn_readfirstlane(slot_step[s]);
            for (int t = 0; t < steps; ++t) {
#pragma unroll
              for (int q = 0; q < kSftBatch; ++q) v[q] *= b[q];
            }
#pragma unroll
            for (int q = 0; q < kSftBatch; ++q) sum[s] += v[q];
          }
        }
      }
    } else {
#pragma unroll 1
      for (int q = 0; q < kSftRows; ++q) {
        const int64_t gi = gi0 + q;
        const double x = sft_base(col[q], denom, net_type);
        const double b = gi < n && gj < n && gi != gj ? x : 0.0;
#pragma unroll
        for (int s = 0; s < NS; ++s)
          if (s < n_slots) sum[s] += pow(b, slot_p[s]);
      }
    }
    __syncthreads();  // the stage is free for the next tile's panels
  }

  // the four threads of a column, in wave order: lds[wave][slot][column]
#pragma unroll
  for (int s = 0; s < NS; ++s) lds[(wave * NS + s) * kNbTile + lane] = sum[s];
  __syncthreads();
#pragma unroll
  for (int t = 0; t < NS / 4; ++t) {
    const int s = wave + 4 * t;
    const double* const q = lds + s * kNbTile + lane;
    constexpr int kWave = NS * kNbTile;
    const double total = ((q[0] + q[kWave]) + q[2 * kWave]) + q[3 * kWave];
    if (s < n_slots && gj < n) part[((int64_t)r * pw.n_slots_total + pw.slot0 + s) * n + gj] = total;
  }
}

// k[j + m n] = the sum over the row groups, in increasing r, of the partials
// of power m's slot; blockIdx.y = m. flags |= 4 for a non-finite k.
__global__ void __launch_bounds__(256)
soft_connectivity_reduce_kernel(const double* __restrict__ part, int64_t n, int row_groups, int n_slots, SftSlots sl,
                                double* __restrict__ k, int* __restrict__ flags) {
  const int m = blockIdx.y;
  const double* const src = part + (int64_t)sl.slot_of[m] * n;
  int bad = 0;
  for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < n; j += (int64_t)gridDim.x * blockDim.x) {
    double t = 0.0;
    for (int r = 0; r < row_groups; ++r) t += src[(int64_t)r * n_slots * n + j];
    k[j + (int64_t)m * n] = t;
    bad |= isfinite(t) ? 0 : 4;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) bad |= __shfl_xor(bad, o, 64);
  if (bad && (threadIdx.x & 63) == 0) atomicOr(flags, bad);
}

// corr[e] / net[e] of elements [first, first + len) of a pair array with
// element stride es (1: {corr, net}; 2: the Gram-table layout).
__global__ void deinterleave_kernel(const double2* __restrict__ pairs, int es, int64_t first, int64_t len,
                                    double* __restrict__ corr, double* __restrict__ net) {
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < len; e += (int64_t)gridDim.x * blockDim.x) {
    const double2 p = pairs[(first + e) * es];
    if (corr) corr[e] = p.x;
    if (net) net[e] = p.y;
  }
}

}  // namespace

hipError_t launch_netbuild(const double* X, int64_t S, int64_t n, double2* pairs, int net_type, double beta,
                           int* flags, hipStream_t st) {
  const int64_t nT = (n + kNbTile - 1) / kNbTile;
  const int64_t n_tiles = nT * (nT + 1) / 2;
  const unsigned g = (unsigned)std::min<int64_t>(n_tiles, (int64_t)1 << 20);
  hipLaunchKernelGGL(netbuild_kernel, dim3(g), dim3(256), 0, st, X, S, n, pairs, net_type, beta, flags);
  return hipGetLastError();
}

size_t tom_scratch_bytes(int64_t n) {
  return ((size_t)n * (size_t)(n + 2) + (size_t)n) * sizeof(double);
}

hipError_t launch_tom(int64_t n, double2* pairs, double* scratch, int* flags, hipStream_t st) {
  double* const A = scratch;
  double* const k = scratch + n * (n + 2);
  const unsigned ge = (unsigned)std::min<int64_t>(n + 2, (int64_t)1 << 20);
  hipLaunchKernelGGL(tom_extract_kernel, dim3(ge), dim3(256), 0, st, pairs, n, A, k);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const int64_t nT = (n + kNbTile - 1) / kNbTile;
  const int64_t n_tiles = nT * (nT + 1) / 2;
  const unsigned g = (unsigned)std::min<int64_t>(n_tiles, (int64_t)1 << 20);
  hipLaunchKernelGGL(tom_kernel, dim3(g), dim3(256), 0, st, A, k, n, pairs, flags);
  return hipGetLastError();
}

// A pure function of n and compile-time constants (never of the device): k
// is the same bits wherever it is computed.
int sft_row_groups(int64_t n) {
  const int64_t nT = (n + kNbTile - 1) / kNbTile;
  return (int)std::min<int64_t>((nT + kSftTilesPerGroup - 1) / kSftTilesPerGroup, kSftMaxRowGroups);
}

size_t sft_result_offset(int64_t n, int n_powers, int row_groups) {
  return (size_t)row_groups * (size_t)n_powers * (size_t)n;
}

size_t sft_scratch_bytes(int64_t n, int n_powers, int row_groups) {
  return (sft_result_offset(n, n_powers, row_groups) + (size_t)n_powers * (size_t)n) * sizeof(double);
}

hipError_t launch_soft_connectivity(const double* X, int64_t S, int64_t n, int net_type, const double* powers,
                                    int n_powers, int row_groups, double* scratch, int* flags, hipStream_t st) {
  if (n_powers < 1 || n_powers > kSftMaxPowers || row_groups < 0 || row_groups > kSftRowGroupsLimit)
    return hipErrorInvalidValue;
  const int R = row_groups ? row_groups : sft_row_groups(n);
  bool chain = true;
  for (int m = 0; m < n_powers; ++m)
    chain = chain && powers[m] >= 1.0 && powers[m] <= (double)kSftMaxChain && powers[m] == floor(powers[m]);
  // the distinct powers, ascending
  double distinct[kSftMaxPowers];
  std::copy(powers, powers + n_powers, distinct);
  std::sort(distinct, distinct + n_powers);
  const int n_slots = (int)(std::unique(distinct, distinct + n_powers) - distinct);
  SftSlots sl = {};
  for (int m = 0; m < n_powers; ++m)
    sl.slot_of[m] = (int)(std::lower_bound(distinct, distinct + n_slots, powers[m]) - distinct);

  const int64_t nT = (n + kNbTile - 1) / kNbTile;
  const int64_t tiles_per_group = (nT + R - 1) / R;
  double* const part = scratch;
  double* const k = scratch + sft_result_offset(n, n_powers, R);
  const dim3 grid((unsigned)nT, (unsigned)R);
  const int per_launch = chain ? kSftChainSlots : kSftPowSlots;
  for (int s0 = 0; s0 < n_slots; s0 += per_launch) {  // more distinct powers than a launch takes: another sweep
    SftPowers pw = {};
    pw.n_slots = std::min(per_launch, n_slots - s0);
    pw.slot0 = s0;
    pw.n_slots_total = n_slots;
    for (int s = 0; s < pw.n_slots; ++s) {
      pw.p[s] = distinct[s0 + s];
      pw.step[s] = chain ? (int)distinct[s0 + s] - (s ? (int)distinct[s0 + s - 1] : 1) : 0;
    }
    if (chain)
      hipLaunchKernelGGL(soft_connectivity_kernel<true>, grid, dim3(256), 0, st, X, S, n, net_type, pw,
                         tiles_per_group, part);
    else
      hipLaunchKernelGGL(soft_connectivity_kernel<false>, grid, dim3(256), 0, st, X, S, n, net_type, pw,
                         tiles_per_group, part);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  const dim3 rgrid((unsigned)std::min<int64_t>((n + 255) / 256, 4096), (unsigned)n_powers);
  hipLaunchKernelGGL(soft_connectivity_reduce_kernel, rgrid, dim3(256), 0, st, part, n, R, n_slots, sl, k, flags);
  return hipGetLastError();
}

hipError_t launch_deinterleave(const double2* pairs, int es, int64_t first, int64_t len, double* corr, double* net,
                               hipStream_t st) {
  if (len <= 0) return hipSuccess;
  const unsigned g = (unsigned)std::min<int64_t>((len + 255) / 256, 8192);
  hipLaunchKernelGGL(deinterleave_kernel, dim3(g), dim3(256), 0, st, pairs, es, first, len, corr, net);
  return hipGetLastError();
}

}  // namespace nr
