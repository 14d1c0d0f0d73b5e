// Average-linkage dendrogram of the resident network (nr_hclust_average,
// include/netrep_gpu.h): the working matrix D = 1 - net in device scratch and
// the nearest-neighbour chain on it, run by one persistent workgroup in
// bounded launches. The chain is a serial sequence of column scans and
// row / column updates of a matrix that stays in HBM; there is no grid-wide
// wait anywhere: one workgroup owns all of it, and its __syncthreads order
// its own global stores and loads (one CU, one vector L1).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>

#include "hclust_host.h"
#include "kernels.h"

// The Lance-Williams update must round each of its operations on its own, so
// that a restatement in any language gives the same bits. The __d*_rn
// intrinsics are plain operators to the compiler, which fuses a * b + c by
// default: contraction is off for this file (and in its Makefile rule).
#pragma clang fp contract(off)

namespace nr {

namespace {

constexpr int kHcThreads = 1024;           // the largest workgroup: 16 waves scan one column
constexpr int kHcWaves = kHcThreads / 64;

// hclust_extract_kernel: one workgroup per column j (grid-stride):
// D(i, j) = 1 - net(i, j), +inf on the diagonal and in the padding rows
// n .. ld - 1, read through the {pairs, es} convention (es = 1: the pair
// array, 2: the Gram table). Also the chain's initial state: every slot a live
// singleton, the state words zero.
__global__ void __launch_bounds__(256)
hclust_extract_kernel(const double2* __restrict__ pairs, int es, int64_t n, int64_t ld, double* __restrict__ D,
                      double* __restrict__ size, int32_t* __restrict__ id, long long* __restrict__ st) {
  const double inf = __builtin_huge_val();
  for (int64_t j = blockIdx.x; j < n; j += gridDim.x) {
    double* const col = D + j * ld;
    for (int64_t i = threadIdx.x; i < ld; i += blockDim.x)
      col[i] = (i >= n || i == j) ? inf : 1.0 - pairs[(i + j * n) * es].y;
  }
  const int64_t g = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  for (int64_t i = g; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    size[i] = 1.0;
    id[i] = (int32_t)i;
  }
  if (g < kHclustStateWords) st[g] = 0;
}

// The smaller of two (value, index) candidates, the lower index on ties.
__device__ __forceinline__ void hc_take(double& bv, int& bi, double ov, int oi) {
  if (ov < bv || (ov == bv && oi < bi)) {
    bv = ov;
    bi = oi;
  }
}

// hclust_chain_kernel: ONE workgroup of 1,024 threads runs the chain for at
// most max_merges merges and returns; everything it needs to resume is in
// global memory (st: chain length, merges done, searches, error word, the
// lowest-live cursor; chain, size, id; the emitted merges).
//
// Every trip of the loop makes exactly one nearest-neighbour search and counts
// it before the scan; the loop ends when the merges of this launch or of the
// tree are done, or with an error word when the call's searches reach
// search_cap, when a search finds nothing finite, or when the chain would
// outgrow its array. There is no other exit, and no trip skips the counter, so
// a launch makes at most search_cap trips whatever D holds. The only other
// data-dependent loop is thread 0's lowest-live cursor, which only advances
// and stops at n.
//
// A search: min / argmin over the contiguous column a of D (retired slots and
// the diagonal hold +inf, so no mask): 16-byte loads, a running (value, index)
// per thread in increasing row order, a shuffle reduction per wave, one LDS
// step across the 16 waves. Thread 0 then applies the tie rule (the chain's
// previous element wins if it attains the minimum) and decides: push, or merge.
//
// A merge of slots lo < hi: read columns lo and hi, write the Lance-Williams
// column hi contiguously and row hi at stride ld, +inf into column and row lo.
// The update is two multiplications, one addition and one division, each
// rounded on its own.
__global__ void __launch_bounds__(kHcThreads)
hclust_chain_kernel(HclustParams P) {
  __shared__ double w_val[kHcWaves];
  __shared__ int w_idx[kHcWaves];
  __shared__ long long s_i[6];   // go, a, prev | action, lo, hi
  __shared__ double s_d[3];      // s_lo, s_hi, s_lo + s_hi
  const double inf = __builtin_huge_val();
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t n = P.n, ld = P.ld;
  const int half = (int)(ld >> 1);
  // thread 0 alone keeps the chain's state
  long long chain_len = 0, n_merged = 0, searches = 0, err = 0, first = 0, done = 0;
  if (tid == 0) {
    chain_len = P.st[kHclustStChainLen];
    n_merged = P.st[kHclustStMerged];
    searches = P.st[kHclustStSearches];
    err = P.st[kHclustStError];
    first = P.st[kHclustStFirstLive];
  }
  for (;;) {
    if (tid == 0) {
      long long go = 0, a = 0, prev = -1;
      if (err == 0 && n_merged < n - 1 && done < P.max_merges) {
        if (searches >= P.search_cap) {
          err = kHclustErrSearchCap;
        } else {
          if (chain_len == 0) {  // the lowest-index live slot; slots only ever retire, so the cursor only advances
            while (first < n && P.size[first] == 0.0) ++first;
            if (first < n) {
              P.chain[0] = (int32_t)first;
              chain_len = 1;
            }
          }
          if (chain_len == 0) {
            err = kHclustErrChain;
          } else {
            a = P.chain[chain_len - 1];
            prev = chain_len >= 2 ? P.chain[chain_len - 2] : -1;
            ++searches;
            go = 1;
          }
        }
      }
      s_i[0] = go;
      s_i[1] = a;
      s_i[2] = prev;
    }
    __syncthreads();  // also: the last merge's stores are visible to every wave
    if (s_i[0] == 0) break;
    const int64_t a = s_i[1];
    const int64_t prev = s_i[2];

    // ---- the search: min / argmin of column a
    double bv = inf;
    int bi = INT_MAX;
    {
      const double2* const col = reinterpret_cast<const double2*>(P.D + a * ld);
#pragma unroll 2
      for (int p = tid; p < half; p += kHcThreads) {
        const double2 v = col[p];
        if (v.x < bv) {
          bv = v.x;
          bi = 2 * p;
        }
        if (v.y < bv) {
          bv = v.y;
          bi = 2 * p + 1;
        }
      }
    }
    for (int off = 32; off > 0; off >>= 1) hc_take(bv, bi, __shfl_down(bv, off), __shfl_down(bi, off));
    if (lane == 0) {
      w_val[wave] = bv;
      w_idx[wave] = bi;
    }
    __syncthreads();
    if (wave == 0) {
      bv = lane < kHcWaves ? w_val[lane] : inf;
      bi = lane < kHcWaves ? w_idx[lane] : INT_MAX;
      for (int off = kHcWaves / 2; off > 0; off >>= 1) hc_take(bv, bi, __shfl_down(bv, off), __shfl_down(bi, off));
      if (tid == 0) {
        long long action = 0, lo = 0, hi = 0;  // 0: pushed (or stopped with err), 1: merge
        if (!(bv < inf)) {
          err = kHclustErrNoNeighbour;  // n_merged < n - 1: more than one slot is live
        } else {
          if (prev >= 0 && P.D[a * ld + prev] == bv) bi = (int)prev;
          if (prev >= 0 && bi == (int)prev) {
            action = 1;
            lo = a < prev ? a : prev;
            hi = a < prev ? prev : a;
            const double s_lo = P.size[lo], s_hi = P.size[hi];
            const double tot = __dadd_rn(s_lo, s_hi);
            s_d[0] = s_lo;
            s_d[1] = s_hi;
            s_d[2] = tot;
            P.m_lo[n_merged] = P.id[lo];
            P.m_hi[n_merged] = P.id[hi];
            P.m_height[n_merged] = bv;
            P.m_size[n_merged] = tot;
            P.id[hi] = (int32_t)(n + n_merged);
            P.size[hi] = tot;
            P.size[lo] = 0.0;
            chain_len -= 2;
            ++n_merged;
            ++done;
          } else if (chain_len >= n) {
            err = kHclustErrChain;
          } else {
            P.chain[chain_len++] = bi;
          }
        }
        s_i[3] = action;
        s_i[4] = lo;
        s_i[5] = hi;
      }
    }
    __syncthreads();
    if (s_i[3] == 0) continue;

    // ---- the merge: column / row hi updated, column / row lo retired
    {
      const int64_t lo = s_i[4], hi = s_i[5];
      const double s_lo = s_d[0], s_hi = s_d[1], tot = s_d[2];
      double2* const col_lo = reinterpret_cast<double2*>(P.D + lo * ld);
      double2* const col_hi = reinterpret_cast<double2*>(P.D + hi * ld);
      const double2 inf2 = make_double2(inf, inf);
      for (int p = tid; p < half; p += kHcThreads) {
        const double2 l = col_lo[p], h = col_hi[p];
        const int64_t k0 = 2 * (int64_t)p, k1 = k0 + 1;
        double2 r;
        r.x = (k0 == lo || k0 == hi || k0 >= n) ? inf : __ddiv_rn(__dadd_rn(__dmul_rn(s_lo, l.x), __dmul_rn(s_hi, h.x)), tot);
        r.y = (k1 == lo || k1 == hi || k1 >= n) ? inf : __ddiv_rn(__dadd_rn(__dmul_rn(s_lo, l.y), __dmul_rn(s_hi, h.y)), tot);
        col_hi[p] = r;
        col_lo[p] = inf2;
        if (k0 < n) {
          P.D[k0 * ld + hi] = r.x;
          P.D[k0 * ld + lo] = inf;
        }
        if (k1 < n) {
          P.D[k1 * ld + hi] = r.y;
          P.D[k1 * ld + lo] = inf;
        }
      }
    }
    // the next trip's first __syncthreads orders these stores before its scan
  }
  if (tid == 0) {
    P.st[kHclustStChainLen] = chain_len;
    P.st[kHclustStMerged] = n_merged;
    P.st[kHclustStSearches] = searches;
    P.st[kHclustStError] = err;
    P.st[kHclustStFirstLive] = first;
  }
}

}  // namespace

size_t hclust_state_bytes(int64_t n) {
  // st | size, m_height, m_size (doubles) | chain, id, m_lo, m_hi (int32)
  return sizeof(long long) * kHclustStateWords + (size_t)n * (3 * sizeof(double) + 4 * sizeof(int32_t));
}

HclustParams hclust_params(int64_t n, double* D, void* state) {
  HclustParams P = {};
  P.D = D;
  P.n = n;
  P.ld = hclust_ld(n);
  P.st = static_cast<long long*>(state);
  P.size = reinterpret_cast<double*>(P.st + kHclustStateWords);
  P.m_height = P.size + n;
  P.m_size = P.m_height + n;
  P.chain = reinterpret_cast<int32_t*>(P.m_size + n);
  P.id = P.chain + n;
  P.m_lo = P.id + n;
  P.m_hi = P.m_lo + n;
  P.max_merges = kHclustMergesPerLaunch;
  P.search_cap = hclust_search_cap(n);
  return P;
}

hipError_t launch_hclust_extract(const double2* pairs, int es, const HclustParams& P, hipStream_t st) {
  const unsigned g = (unsigned)std::min<int64_t>(P.n, 4096);
  hipLaunchKernelGGL(hclust_extract_kernel, dim3(g), dim3(256), 0, st, pairs, es, P.n, P.ld, P.D, P.size, P.id, P.st);
  return hipGetLastError();
}

hipError_t launch_hclust_chain(const HclustParams& P, hipStream_t st) {
  hipLaunchKernelGGL(hclust_chain_kernel, dim3(1), dim3(kHcThreads), 0, st, P);
  return hipGetLastError();
}

}  // namespace nr
