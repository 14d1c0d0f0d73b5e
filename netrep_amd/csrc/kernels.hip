// Device kernels of the MI355X NetRep permutation engine (gfx950 / CDNA4).
//
// One work item = (permutation p, module m). Two kernels cover the seven
// statistics of calculateNulls (src/permutations.cpp:71-101):
//   module_net_kernel      avg.weight, cor.cor, cor.degree, avg.cor
//                          (CorrVector + WeightedDegree gathers; HBM-bound)
//   module_profile_kernel  coherence, cor.contrib, avg.contrib
//                          (SummaryProfile + NodeContribution: fp64-MFMA Gram
//                           of the S x k data block + Lanczos top eigenpair)
// The network-only path (src/permutationsNoData.cpp:66-85) is the first kernel
// alone. Both also run in "vector" mode to produce the per-module vectors of
// IntermediateProperties (src/discProps.cpp:100-121) and NetProps
// (src/properties.cpp:155-184).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <type_traits>
#include <stdint.h>
#include <math.h>

#include "prp.h"
#include "kernels.h"
#include "device_common.h"

// the Gram-table items' gathers: pairs per chunk, and whether the next
// chunk's gathers are issued before the current chunk is processed. Measured
// (C3 shape, profiles/r03/table_gathers/): 7 pairs 15.86 ms per 256
// permutations, 5: 15.07, 4: 14.73, 3: 14.41-14.56, 2: 14.27, 1: 14.87; the
// next chunk in flight adds at most 0.4% (2 pairs: 14.21) for more spill.
#define NR_TABLE_U 2
#define NR_TABLE_PIPE false
// the network kernel's gathers: pairs per chunk (3/4/7 measured, profiles/r03/net_chunk/)
#define NR_NET_U 7
// units in flight per wave in the packed matvec's fp64 passes (2 measured
// slower, profiles/r03/matvec_uf/)
#define NR_MV_UF64 1
// Lanczos stop rule: top Ritz residual <= NR_LZ_TOL * theta (DESIGN.md section 5;
// 5e-14 measured 2.9% faster at twice the worst statistic difference)
#define NR_LZ_TOL 5e-15

namespace nr {


// ---------------------------------------------------------------------------
// Weighted degree as the reference computes it (src/netStats.cpp:124-144):
// the column sums of |net(srt, srt)| over the module's SORTED nodes with the
// diagonal included, minus |diag|. arma::sum over a column is Armadillo's
// arrayops::accumulate: two accumulators over the even and odd row
// positions, returned as acc1 + acc2 (RcppArmadillo, unvendored; the same
// loop is restated in oracle/netrep_ref.cpp). When |diag| dwarfs the
// off-diagonal weights -- a correlation network's diagonal is 1 -- every
// addition after the diagonal rounds to the accumulator's ulp, and those
// roundings move cor.degree by up to ~1e-9 (measured on the
// C5 shape). The kernel therefore reproduces them instead of summing exactly:
//  * per node c (sorted position p, d = |diag|): the same-parity terms before
//    p (Pb), the first same-parity term after p (F, from the node at position
//    p + 2), the remaining same-parity terms (each rounded to the grid unit g
//    of the accumulator once it holds the diagonal: added in units of g), and
//    the other parity's sum (O);
//  * Pb and O are accumulated in 64-bit fixed point (2^-16 g), the unit counts
//    as integers, so the sums are exact and order independent (bitwise
//    reproducible whatever the thread schedule);
//  * WD = fl(fl(x + g * units + O) - d) with x = fl(fl(Pb + d) + F), valid
//    while the accumulator stays in g's binade; otherwise (or d = 0) the plain
//    sum of the off-diagonal terms, per-wave copies added in wave order.
// Bitwise equal to the two-accumulator loop in the cancellation regime
// (tools check: oracle/netrep_ref.cpp vs the kernel, tests/test_gpu_configs.py).
// ---------------------------------------------------------------------------
// (WD_FX_BITS, WD_NO_GRID, wd_grid_exp, wd_fx: device_common.h)

struct NetLds {
  double* red;                       // 8 * NW
  uint32_t* idx;                     // [k] test column of each node
  int* rk;                           // [k] sorted position (SortNodes rank)
  int* ge;                           // [k] grid exponent (WD_NO_GRID: none)
  double* dg;                        // [k] |diag|
  double* plain;                     // [NW][k] plain off-diagonal sums, per wave
  unsigned long long *pb, *on, *tn;  // [k] fixed-point Pb, O; unit count of the rest
  double* ff;                        // [k] the first same-parity term after the diagonal
  int k_stride;
  // Node i's slot in the per-node arrays: one pad slot per 32 nodes, so the
  // row targets of one wave instruction (nodes U apart in a column) spread
  // over all LDS banks (U = 2: a 4-way conflict without it).
  __device__ __forceinline__ static int at(int i) { return i + (i >> 5); }
};

// net_kpad(kmax) slots per per-node array (NetLds::at), net_lds_bytes in all:
// device_common.h.
template <int NW>
__device__ __forceinline__ NetLds carve_net_lds(unsigned char* smem, int kmax) {
  NetLds L;
  const int kp = net_kpad(kmax);
  L.red = reinterpret_cast<double*>(smem);
  L.plain = L.red + 8 * NW;
  L.dg = L.plain + (size_t)NW * kp;
  L.ff = L.dg + kp;
  L.pb = reinterpret_cast<unsigned long long*>(L.ff + kp);
  L.on = L.pb + kp;
  L.tn = L.on + kp;
  L.idx = reinterpret_cast<uint32_t*>(L.tn + kp);
  L.rk = reinterpret_cast<int*>(L.idx + kmax);
  L.ge = L.rk + kp;
  L.k_stride = kp;
  return L;
}

// The same layout in a workgroup's global scratch slot (modules too large for
// LDS); only the reduction scratch stays in LDS.
template <int NW>
__device__ __forceinline__ NetLds carve_net_mem(unsigned char* smem, double* slot, int kmax) {
  NetLds L = carve_net_lds<NW>(reinterpret_cast<unsigned char*>(slot) - sizeof(double) * 8 * NW, kmax);
  L.red = reinterpret_cast<double*>(smem);
  return L;
}

// The same layout over a region the caller lends (the summary-profile
// kernel's Lanczos vectors, idle before its Gram), sharing its index set.
template <int NW>
__device__ __forceinline__ NetLds carve_net_over(double* region, double* red, uint32_t* idx, int kmax) {
  NetLds L = carve_net_lds<NW>(reinterpret_cast<unsigned char*>(region - 8 * NW), kmax);
  L.red = red;
  L.idx = idx;
  return L;
}

// One weighted-degree contribution a = |net(source, target)| (a >= 0).
__device__ __forceinline__ void wd_add(const NetLds& L, double* plain_w, int t0, int pt, int ps, double a) {
  const int t = NetLds::at(t0);
  atomicAdd(&plain_w[t], a);
  const int ge = L.ge[t];
  if (ge == WD_NO_GRID || !isfinite(a)) return;
  if (((pt ^ ps) & 1) == 0) {
    if (ps < pt) atomicAdd(&L.pb[t], wd_fx(a, ge, WD_FX_BITS));
    else if (ps == pt + 2) atomicAdd(&L.ff[t], a);
    else atomicAdd(&L.tn[t], wd_fx(a, ge, 0));
  } else {
    atomicAdd(&L.on[t], wd_fx(a, ge, WD_FX_BITS));
  }
}

// The column target's parts at a chunk's end. The lanes of a wave hold
// consecutive chunks of the column-major pair order, so most of them end in
// the same column: adding every lane's parts to LDS directly was up to a
// 64-way same-address LDS atomic per wave instruction (VERDICT r3, weak 4:
// 1.0e10 bank-conflict cycles per C3 launch). A segmented inclusive scan over
// the lanes, keyed by the column (non-decreasing with the lane), sums them in
// registers, and only each segment's last lane adds to LDS. Lanes that have
// left the chunk loop are a suffix of the wave, so every shuffle reads an
// active lower lane. The fixed-point parts are integers (exact in any order);
// the plain sums stay per wave in a fixed order (deterministic); the first
// same-parity term after the diagonal is one term per node.
// One step of the segmented scan: the values of the lane DPP control CTRL
// names (row_shr:s within 16-lane rows, row_bcast:15 / :31 across rows; rows
// outside ROWMASK and lanes without a source keep the identity) are added
// where that lane's column equals this one's. DPP moves are VALU operations:
// no LDS instruction and no LDS round trip on the flush's dependency chain
// (the __shfl_up form issued 66 ds_bpermute per flush).
template <int CTRL, int ROWMASK>
__device__ __forceinline__ int wd_dpp_i32(int old, int v) {
  return __builtin_amdgcn_update_dpp(old, v, CTRL, ROWMASK, 0xF, false);
}
template <int CTRL, int ROWMASK>
__device__ __forceinline__ unsigned long long wd_dpp_u64(unsigned long long v) {
  const int lo = wd_dpp_i32<CTRL, ROWMASK>(0, (int)(unsigned)v);
  const int hi = wd_dpp_i32<CTRL, ROWMASK>(0, (int)(unsigned)(v >> 32));
  return ((unsigned long long)(unsigned)hi << 32) | (unsigned)lo;
}
template <int CTRL, int ROWMASK>
__device__ __forceinline__ void wd_scan_step(int jc, double& cpl, double& cff, unsigned long long& cpb,
                                             unsigned long long& con, unsigned long long& ctn) {
  const int ko = wd_dpp_i32<CTRL, ROWMASK>(-1, jc);
  const double a0 = __builtin_bit_cast(double, wd_dpp_u64<CTRL, ROWMASK>(__builtin_bit_cast(unsigned long long, cpl)));
  const double a1 = __builtin_bit_cast(double, wd_dpp_u64<CTRL, ROWMASK>(__builtin_bit_cast(unsigned long long, cff)));
  const unsigned long long b0 = wd_dpp_u64<CTRL, ROWMASK>(cpb), b1 = wd_dpp_u64<CTRL, ROWMASK>(con),
                           b2 = wd_dpp_u64<CTRL, ROWMASK>(ctn);
  if (ko == jc) {
    cpl += a0;
    cff += a1;
    cpb += b0;
    con += b1;
    ctn += b2;
  }
}

__device__ __forceinline__ void wd_flush_column(const NetLds& L, double* plain_w, int jc, int gj, double cpl,
                                                double cff, unsigned long long cpb, unsigned long long con,
                                                unsigned long long ctn) {
  const int lane = threadIdx.x & 63;
  // Hillis-Steele within rows (the columns are non-decreasing with the lane,
  // so a matching key at distance s means the whole span matches), then the
  // rows' last lanes across rows
  wd_scan_step<0x111, 0xF>(jc, cpl, cff, cpb, con, ctn);  // row_shr:1
  wd_scan_step<0x112, 0xF>(jc, cpl, cff, cpb, con, ctn);  // row_shr:2
  wd_scan_step<0x114, 0xF>(jc, cpl, cff, cpb, con, ctn);  // row_shr:4
  wd_scan_step<0x118, 0xF>(jc, cpl, cff, cpb, con, ctn);  // row_shr:8
  wd_scan_step<0x142, 0xA>(jc, cpl, cff, cpb, con, ctn);  // row_bcast:15 into rows 1, 3
  wd_scan_step<0x143, 0xC>(jc, cpl, cff, cpb, con, ctn);  // row_bcast:31 into rows 2, 3
  const unsigned long long act = __ballot(1);
  const int kn = __shfl_down(jc, 1, 64);
  const bool last = lane == 63 || !((act >> (lane + 1)) & 1ull) || kn != jc;
  if (last) {
    const int t = NetLds::at(jc);
    atomicAdd(&plain_w[t], cpl);
    if (gj != WD_NO_GRID) {
      atomicAdd(&L.pb[t], cpb);
      atomicAdd(&L.on[t], con);
      atomicAdd(&L.tn[t], ctn);
      atomicAdd(&L.ff[t], cff);
    }
  }
}

// The reference's weighted degree of node c from its accumulated parts.
__device__ __forceinline__ double wd_final(const NetLds& L, int NWn, int c0, int k) {
  const int c = NetLds::at(c0);
  double plain = 0.0;
  for (int w = 0; w < NWn; ++w) plain += L.plain[w * L.k_stride + c];
  const double d = L.dg[c];
  if (!isfinite(d)) return nr_nan();      // colsum carries the NaN/Inf diagonal, minus itself
  if (!isfinite(plain)) return plain;
  const int ge = L.ge[c];
  if (ge == WD_NO_GRID) return plain;
  // fixed point valid (no 2^61 clamp reached) and the sums small against d
  if (ldexp(plain, WD_FX_BITS - ge) >= 1.1529215046068470e18) return plain;  // 2^60
  const double s = ldexp(1.0, ge - WD_FX_BITS);
  const double g = ldexp(1.0, ge);
  const double pb = (double)L.pb[c] * s;
  const double o = (double)L.on[c] * s;
  double x = pb + d;
  if (L.rk[c] + 2 < k) x = x + L.ff[c];
  if (!(x > 0.0) || ilogb(x) - 52 != ge) return plain;   // the predicted grid was not x's
  const double chain = x + (double)L.tn[c] * g;
  if (ilogb(chain) - 52 != ge) return plain;              // the accumulator left g's binade
  return (chain + o) - d;
}

// ---------------------------------------------------------------------------
// Module network statistics of one item (p, m): avg.weight, cor.cor,
// cor.degree, avg.cor (CorrVector + WeightedDegree gathers, src/netStats.cpp:
// 124-204; src/permutations.cpp:75-97). One NW-wave workgroup per item. The
// k(k-1)/2 pairs (column-major lower triangle of the unsorted module order,
// CorrVector's order) are cut into chunks of U consecutive pairs dealt
// round-robin to the threads; a thread gathers a chunk's U random 16-byte
// pairs at once (net_issue), keeps the column's (target jj) weighted-degree
// parts in registers and flushes them at a column change, and adds the row
// node's (target ii) parts in LDS, where the targets of one wave instruction
// are distinct (no same-address atomics) (net_process). L.idx holds the
// item's test columns.
//
// PIPE (the two-wave workgroups of modules too large for four waves' LDS
// copies, one workgroup per CU): the next chunk's gathers are issued before
// the current chunk is processed, so every lane keeps U gathers in flight
// through its LDS work -- with two waves per CU nothing else hides it.
// ---------------------------------------------------------------------------
// Element (r, c) of the resident {corr, net} pairs: column-major n x n with
// element stride es (1 = pairs, 2 = the Gram table). (A packed lower triangle
// of symmetric matrices measured equal or slower, profiles/r04/ab8/.)
__device__ __forceinline__ int64_t pair_at(int64_t r, int64_t c, int64_t n, int64_t es) {
  return (r + c * n) * es;
}

// a global (not constant) cell, so the discovery-load pointer stays a global pointer
__device__ double kNetNanCell = __builtin_nan("");

// The packed symmetric Gram's addressing (layout described at pk_store_tile
// below; pk_groups, pk_base: device_common.h).
__device__ __forceinline__ int64_t pk_at(int r, int c, int kc) {  // r >= 16 (c / 16)
  const int g = c >> 4;
  const int rr = r - 16 * g;
  const int j = rr >> 6;
  const int h = min(64, kc - 16 * g - 64 * j);
  return pk_base(g, kc) + 1024 * (int64_t)j + (int64_t)(c & 15) * h + (rr & 63);
}
__device__ __forceinline__ int64_t pk_col(int c, int kc) { return pk_at(c, c, kc); }  // the diagonal (HD: G_cc / 2)

// Where a Gram-table item puts its Gram: the slot's packed Gram (and its fp32
// copy) of side kc = k + 1, the ones column's entries from colsum, and S.
struct GramOut {
  double* G;
  float* G32;
  int kc;
  double S;
  __device__ __forceinline__ void put(int64_t a, double v) const {
    G[a] = v;
    if (G32) G32[a] = (float)v;
  }
};

template <int U>
struct NetChunk {
  double2 e[U];   // {corr, net}(idx[ii], idx[jj])
  double e2[U];   // net(idx[jj], idx[ii])
  double g[U];    // gram(idx[ii], idx[jj]) (Gram table)
  double x[U];    // the discovery correlation of the pair
  int iis[U];     // row node (-1: past the end)
  int jjs[U];     // column node
  int64_t v0;     // the chunk's first pair
  int j0;         // its column
};

// Every lane issues all U (2U when the network is not symmetric or the Gram
// table is read) gathers and U discovery loads whatever its chunk holds --
// entries past the item's end read the item's first diagonal pair and first
// discovery value -- so the number of loads in flight is the same on every
// path and the compiler's wait counts can leave the next chunk's gathers
// outstanding (PIPE). Table layout (es = 2): the pair's second 16 bytes,
// {gram, net^T}, sit in the same 32-byte sector as {corr, net}.
// ESC >= 0: the pairs' layout (P.es) fixed at compile time (no per-gather
// select between the packed and the strided addressing).
template <int U, bool SYM, bool GRAM, int ESC = -1>
__device__ __forceinline__ void net_issue(const NetParams& P, const NetLds& L, int64_t k, int64_t cvo,
                                          int64_t npairs, int64_t ch, NetChunk<U>& c) {
  const double2* __restrict__ pairs = P.pairs;
  const int64_t n = P.n_nodes;
  const int64_t es = ESC >= 0 ? ESC : P.es;
  const int64_t v0 = ch * U;
  const int64_t v1 = v0 + U < npairs ? v0 + U : npairs;
  // no discovery vector (observed / vector runs): every x reads the NaN cell
  const double* __restrict__ xp = P.disc_cv ? P.disc_cv + cvo : &kNetNanCell;
  const int64_t xstep = P.disc_cv ? 1 : 0;
  int64_t jj64, ii64;
  decode_pair(v0, k, jj64, ii64);
  int jj = (int)jj64, ii = (int)ii64;
  c.v0 = v0;
  c.j0 = jj;
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int64_t v = v0 + u;
    const bool ok = v < v1;
    c.iis[u] = ok ? ii : -1;
    c.jjs[u] = jj;
    const int64_t r = L.idx[ok ? ii : 0], cc = L.idx[ok ? jj : 0];
    const int64_t a = pair_at(r, cc, n, es);
    c.e[u] = pairs[a];                          // corr(idx[ii], idx[jj]), net(idx[ii], idx[jj])
    if (GRAM) {  // (symmetry a run-time select: the load is there either way)
      const double2 f = pairs[a + 1];           // gram(idx[ii], idx[jj]), net(idx[jj], idx[ii])
      c.g[u] = f.x;
      c.e2[u] = P.symmetric ? c.e[u].y : f.y;
    } else if (SYM) {
      c.e2[u] = c.e[u].y;
    } else {                                    // net(idx[jj], idx[ii])
      c.e2[u] = es == 2 ? pairs[a + 1].y : pairs[cc + r * n].y;
    }
    c.x[u] = xp[(ok ? v : v0) * xstep];
    if (ok && ++ii == k) {
      ++jj;
      ii = jj + 1;
    }
  }
}

// SEG: the column flush by segmented lane scan (wd_flush_column); the
// two-wave pipelined items (PIPE) flush directly (their lanes mostly share
// one column, and the scan's dependent shuffles sit on the pipeline's
// critical path: C5 network launch 38.1 vs 35.2 G reads/s, profiles/r04/ab7).
template <int U, bool STORE, bool GRAM, bool SEG = true>
__device__ __forceinline__ void net_process(const NetParams& P, const NetLds& L, double* plain_w, int64_t cvo,
                                            double xs, double ys, const NetChunk<U>& c, double* acc,
                                            const GramOut& go, double& g1) {
  // the column's parts, in registers until the column changes
  int jc = c.j0;
  int pj = L.rk[NetLds::at(jc)];
  int gj = L.ge[NetLds::at(jc)];
  double cpl = 0.0, cff = 0.0;
  unsigned long long cpb = 0, con = 0, ctn = 0;
#pragma unroll
  for (int u = 0; u < U; ++u) {
    if (c.iis[u] >= 0) {
      const int i = c.iis[u], j = c.jjs[u];
      if (j != jc) {  // the chunk crossed into column j: flush the previous column
        const int t = NetLds::at(jc);
        atomicAdd(&plain_w[t], cpl);
        if (gj != WD_NO_GRID) {
          atomicAdd(&L.pb[t], cpb);
          atomicAdd(&L.on[t], con);
          atomicAdd(&L.tn[t], ctn);
          atomicAdd(&L.ff[t], cff);
        }
        cpl = cff = 0.0;
        cpb = con = ctn = 0;
        jc = j;
        pj = L.rk[NetLds::at(j)];
        gj = L.ge[NetLds::at(j)];
      }
      const double y = c.e[u].x;
      if (STORE) P.cv_out[cvo + c.v0 + u] = y;
      if (GRAM) {  // G_ij (i > j: the packed lower triangle), twice in 1'G1
        const double gv = c.g[u];
        go.put(pk_at(i, j, go.kc), gv);
        g1 += 2.0 * gv;
      }
      const int pi = L.rk[NetLds::at(i)];
      // target jj (column idx[jj]) gains row idx[ii]: registers
      const double a = fabs(c.e[u].y);
      cpl += a;
      if (gj != WD_NO_GRID && isfinite(a)) {
        if (((pj ^ pi) & 1) == 0) {
          if (pi < pj) cpb += wd_fx(a, gj, WD_FX_BITS);
          else if (pi == pj + 2) cff += a;
          else ctn += wd_fx(a, gj, 0);
        } else {
          con += wd_fx(a, gj, WD_FX_BITS);
        }
      }
      // target ii (column idx[ii]) gains row idx[jj]: LDS
      wd_add(L, plain_w, i, pi, pj, fabs(c.e2[u]));
      const double xv = c.x[u];
      if (isfinite(xv) && isfinite(y)) {        // CompleteCases src/netStats.cpp:43-61
        const double dx = xv - xs, dy = y - ys;
        acc[0] += 1.0;
        acc[1] += dx;
        acc[2] += dy;
        acc[3] += dx * dx;
        acc[4] += dy * dy;
        acc[5] += dx * dy;
        acc[6] += (xv > 0.0 ? y : (xv < 0.0 ? -y : 0.0));
      }
    }
  }
  // flush the last column of the chunk
  if (SEG) {
    wd_flush_column(L, plain_w, jc, gj, cpl, cff, cpb, con, ctn);
  } else {
    const int t = NetLds::at(jc);
    atomicAdd(&plain_w[t], cpl);
    if (gj != WD_NO_GRID) {
      atomicAdd(&L.pb[t], cpb);
      atomicAdd(&L.on[t], con);
      atomicAdd(&L.tn[t], ctn);
      atomicAdd(&L.ff[t], cff);
    }
  }
}

// GRAM (the Gram-table kernel's items): the item's packed Gram is filled from
// the same gathers -- G_ij for every pair, the diagonal and the ones column
// here -- into a region the caller zeroed; g1 / bad return this thread's part
// of 1'G1 over the data block and a non-finite-diagonal flag.
template <int NW, bool PIPE, bool SYM, bool GRAM = false, int U = 7, int ESC = -1>
__device__ __forceinline__ void net_item(const NetParams& P, int m, int64_t p_local, int64_t off, int64_t k,
                                         const NetLds& L, const GramOut& go = GramOut{}, double* g1_out = nullptr,
                                         int* bad_out = nullptr) {
  constexpr int BS = NW * 64;
  const int tid = threadIdx.x;
  const int wave = tid >> 6;
  const double2* __restrict__ pairs = P.pairs;
  const int64_t n = P.n_nodes;
  const int64_t es = ESC >= 0 ? ESC : P.es;
  double g1 = 0.0;
  int bad = 0;
  // per node: sorted position (SortNodes, src/netStats.cpp:23-32), |diag|,
  // grid exponent, zeroed accumulators
  for (int64_t c = tid; c < k; c += BS) {
    const uint32_t ic = L.idx[c];
    int r = 0;
    for (int64_t c2 = 0; c2 < k; ++c2) r += L.idx[c2] < ic;
    const int t = NetLds::at((int)c);
    L.rk[t] = r;
    const int64_t ad = pair_at(ic, ic, n, es);
    const double d = fabs(pairs[ad].y);
    if (GRAM) {  // G_cc and the ones column's G_kc = sum of column c
      const double gcc = pairs[ad + 1].x;
      const double cs = P.colsum[ic];
      const int64_t a1 = pk_at((int)c, (int)c, go.kc), a2 = pk_at((int)k, (int)c, go.kc);
      go.put(a1, 0.5 * gcc);  // GRAM implies the halved packed diagonal (HD, packed_gram_doubles)
      go.put(a2, cs);
      g1 += gcc;
      bad |= (int)!isfinite(gcc);
    }
    L.dg[t] = d;
    L.ge[t] = wd_grid_exp(d);
#pragma unroll
    for (int w = 0; w < NW; ++w) L.plain[w * L.k_stride + t] = 0.0;
    L.pb[t] = 0;
    L.on[t] = 0;
    L.tn[t] = 0;
    L.ff[t] = 0.0;
  }
  __syncthreads();

  const int64_t npairs = k * (k - 1) / 2;
  const int64_t cvo = P.cv_off[m];
  double* plain_w = L.plain + wave * L.k_stride;
  // Shifts keep the one-pass sums well conditioned and make a constant
  // vector give exactly zero variance, as the reference's two-pass stddev does.
  // The test-side shift is the item's first pair; a non-finite first pair
  // (dropped by CompleteCases, src/netStats.cpp:43-61) falls back to 0 so it
  // cannot poison the other pairs' sums.
  const double xs = P.cv_shift ? P.cv_shift[m] : 0.0;
  const double y0 = npairs > 0 ? pairs[pair_at(L.idx[1], L.idx[0], n, es)].x : 0.0;
  if (GRAM && tid == 0) go.put(pk_at((int)k, (int)k, go.kc), go.S);  // 1'1 = S
  const double ys = isfinite(y0) ? y0 : 0.0;

  double acc[7] = {0, 0, 0, 0, 0, 0, 0};  // n, sx, sy, sxx, syy, sxy, s(sign(x) y)
  const int64_t nchunks = (npairs + U - 1) / U;
  if (!GRAM && P.cv_out) {  // vector runs (one item per module): CorrVector out, no pipeline
    for (int64_t ch = tid; ch < nchunks; ch += BS) {
      NetChunk<U> c;
      net_issue<U, SYM, false, ESC>(P, L, k, cvo, npairs, ch, c);
      net_process<U, true, false>(P, L, plain_w, cvo, xs, ys, c, acc, go, g1);
    }
  } else if (!PIPE) {
    for (int64_t ch = tid; ch < nchunks; ch += BS) {
      NetChunk<U> c;
      net_issue<U, SYM, GRAM, ESC>(P, L, k, cvo, npairs, ch, c);
      net_process<U, false, GRAM, !PIPE>(P, L, plain_w, cvo, xs, ys, c, acc, go, g1);
    }
  } else if (tid < nchunks) {
    // (no global stores in this loop: pending stores next to the gathers
    // would make every wait a full drain)
    // two chunks in registers, roles alternating (no register copies, which
    // would wait for the younger gathers); the issue past the last chunk
    // re-reads the last chunk and is never processed
    NetChunk<U> a, b;
    const int64_t last = nchunks - 1;
    int64_t ch = tid;
    net_issue<U, SYM, GRAM, ESC>(P, L, k, cvo, npairs, ch, a);
    for (;;) {
      net_issue<U, SYM, GRAM, ESC>(P, L, k, cvo, npairs, ch + BS < last ? ch + BS : last, b);
      net_process<U, false, GRAM, !PIPE>(P, L, plain_w, cvo, xs, ys, a, acc, go, g1);
      ch += BS;
      if (ch >= nchunks) break;
      net_issue<U, SYM, GRAM, ESC>(P, L, k, cvo, npairs, ch + BS < last ? ch + BS : last, a);
      net_process<U, false, GRAM, !PIPE>(P, L, plain_w, cvo, xs, ys, b, acc, go, g1);
      ch += BS;
      if (ch >= nchunks) break;
    }
  }
  block_sums<7, NW>(acc, L.red);   // its barriers also complete the weighted-degree parts

  // Weighted degrees (the reference's rounding, wd_final), into plain[0]:
  // node c's parts are read and overwritten by its owner thread only
  double* wd = L.plain;
  for (int64_t c = tid; c < k; c += BS) wd[NetLds::at((int)c)] = wd_final(L, NW, (int)c, (int)k);
  __syncthreads();

  // Weighted degree statistics: two-pass over the k values held in LDS.
  const int64_t woff = off;
  double a1[4] = {0, 0, 0, 0};  // sum(all wd), n, sx, sy
  for (int64_t c = tid; c < k; c += BS) {
    const double y = wd[NetLds::at((int)c)];
    const double xv = P.disc_wd ? P.disc_wd[woff + c] : nr_nan();
    a1[0] += y;
    if (isfinite(xv) && isfinite(y)) {
      a1[1] += 1.0;
      a1[2] += xv;
      a1[3] += y;
    }
  }
  block_sums<4, NW>(a1, L.red);
  const double mx = a1[2] / a1[1], my = a1[3] / a1[1];
  double a2[3] = {0, 0, 0};
  for (int64_t c = tid; c < k; c += BS) {
    const double y = wd[NetLds::at((int)c)];
    const double xv = P.disc_wd ? P.disc_wd[woff + c] : nr_nan();
    if (isfinite(xv) && isfinite(y)) {
      const double dx = xv - mx, dy = y - my;
      a2[0] += dx * dx;
      a2[1] += dy * dy;
      a2[2] += dx * dy;
    }
    if (P.wd_out) P.wd_out[woff + c] = y;
  }
  block_sums<3, NW>(a2, L.red);

  // AverageEdgeWeight src/netStats.cpp:154-162: unsigned int pair count.
  const uint32_t ku = (uint32_t)k;
  const double avg_weight = a1[0] / (double)(uint32_t)(ku * ku - ku);
  if (tid == 0 && P.avgw_out) P.avgw_out[m] = avg_weight;
  if (tid == 0 && P.out) {
    const double cor_degree = a1[1] >= 1.0 ? a2[2] / (sqrt(a2[0]) * sqrt(a2[1])) : nr_nan();
    const double cor_cor = pearson_sums(acc[0], acc[1], acc[2], acc[3], acc[4], acc[5]);
    const double avg_cor = acc[0] >= 1.0 ? acc[6] / acc[0] : nr_nan();
    double* o = P.out + (int64_t)P.row_of[m] + (int64_t)P.n_rows * (int64_t)P.n_stat * p_local;
    o[(int64_t)P.n_rows * P.slot_avg_weight] = na_fill(avg_weight);
    o[(int64_t)P.n_rows * P.slot_cor_cor] = na_fill(cor_cor);
    o[(int64_t)P.n_rows * P.slot_cor_degree] = na_fill(cor_degree);
    o[(int64_t)P.n_rows * P.slot_avg_cor] = na_fill(avg_cor);
  }
  if (GRAM) {
    *g1_out = g1;
    *bad_out = bad;
  }
  __syncthreads();  // LDS free again
}

// Kernel 1: module network statistics. One workgroup of NW waves per item
// (NW = 2 for modules too large for four waves' LDS copies). BIG: modules too
// large for LDS at all -- a persistent grid whose workgroups keep the per-node
// arrays in their global scratch slot (L2-resident; the atomics go to L2) and
// loop over the items.
template <int NW, bool BIG, bool SYM, int ESC = -1>
__global__ void __launch_bounds__(NW * 64)
module_net_kernel(NetParams P) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const NetLds L = BIG ? carve_net_mem<NW>(smem, P.big_scratch + (int64_t)blockIdx.x * P.big_stride, P.k_max)
                       : carve_net_lds<NW>(smem, P.k_max);
  const int64_t step = BIG ? (int64_t)gridDim.x : P.n_items;
  for (int64_t item = blockIdx.x; item < P.n_items; item += step) {
    const int64_t mslot = item / P.n_perm;
    const int64_t p_local = item - mslot * P.n_perm;
    const int m = P.mod_order[mslot];
    const int64_t off = P.node_off[m];
    const int64_t k = P.node_off[m + 1] - off;
    nr_prp_key key;
    if (P.src.mode == NR_IDX_PRP) key = nr_prp_make_key(P.src.seed, (uint64_t)(P.src.perm_base + p_local), P.src.n_null);
    for (int64_t c = threadIdx.x; c < k; c += NW * 64) L.idx[c] = node_index(P.src, key, p_local, off + c);
    __syncthreads();
    net_item<NW, NW == 2 || BIG, SYM, false, NR_NET_U, ESC>(P, m, p_local, off, k, L);
  }
}


// w = G x over the leading k x k block of G (column-major, leading dimension
// ld, symmetric, both triangles stored). Waves take contiguous column ranges,
// lanes own rows (RB per 64*RB-row block), U columns are loaded ahead per
// lane; no cross-lane reduction. part[wave][r] is written (not accumulated).
template <int RB, int U>
__device__ __forceinline__ void matvec_part(const double* __restrict__ G, int ld, int k,
                                            const double* x, double* part, int kstride,
                                            int wave, int lane) {
  const int cpw = (k + NR_WAVES - 1) / NR_WAVES;
  const int c0 = wave * cpw;
  const int c1 = min(k, c0 + cpw);
  for (int rb = 0; rb < k; rb += 64 * RB) {
    double acc[RB];
#pragma unroll
    for (int i = 0; i < RB; ++i) acc[i] = 0.0;
    int c = c0;
    for (; c + U <= c1; c += U) {
      double g[U][RB];
#pragma unroll
      for (int u = 0; u < U; ++u)
#pragma unroll
        for (int i = 0; i < RB; ++i) {
          const int r = rb + lane + 64 * i;
          g[u][i] = r < k ? G[r + (int64_t)(c + u) * ld] : 0.0;
        }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const double xc = x[c + u];
#pragma unroll
        for (int i = 0; i < RB; ++i) acc[i] += g[u][i] * xc;
      }
    }
    for (; c < c1; ++c) {
      const double xc = x[c];
#pragma unroll
      for (int i = 0; i < RB; ++i) {
        const int r = rb + lane + 64 * i;
        if (r < k) acc[i] += G[r + (int64_t)c * ld] * xc;
      }
    }
#pragma unroll
    for (int i = 0; i < RB; ++i) {
      const int r = rb + lane + 64 * i;
      if (r < k) part[wave * kstride + r] = c1 > c0 ? acc[i] : 0.0;
    }
  }
}

// out = G x; returns (block-wide) sum_r y[r] * out[r] when y != NULL.
__device__ __forceinline__ double matvec(const double* __restrict__ G, int ld, int k, const double* x,
                                         double* out, double* part, int kstride, const double* y,
                                         double* red) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  matvec_part<2, 4>(G, ld, k, x, part, kstride, wave, lane);
  __syncthreads();
  double d[1] = {0.0};
  for (int r = threadIdx.x; r < k; r += NR_BS) {
    double s = part[r];
#pragma unroll
    for (int w = 1; w < NR_WAVES; ++w) s += part[w * kstride + r];
    out[r] = s;
    if (y) d[0] += y[r] * s;
  }
  block_sums<1>(d, red);
  return d[0];
}

// Lanczos 3-term step w <- w - a q - b qprev; returns |w|^2. No trailing
// barrier: `red` must not be written again before the next barrier.
template <int NW = NR_WAVES>
__device__ __forceinline__ double three_term(int k, double* w, const double* q, const double* qprev,
                                             double a, double b, double* red) {
  double nrm[1] = {0.0};
  for (int c = threadIdx.x; c < k; c += NW * 64) {
    const double z = w[c] - a * q[c] - b * qprev[c];
    w[c] = z;
    nrm[0] += z * z;
  }
  block_sums<1, NW, false>(nrm, red);
  return nrm[0];
}

// Classical Gram-Schmidt of w against the stored basis Q (column-major k x n):
// h = Q^T w (four dots in flight per wave), w <- w - Q h. Returns |w|^2.
template <int NW = NR_WAVES>
__device__ __forceinline__ double reorthogonalise_cgs(const double* __restrict__ Q, int k, int n, double* w,
                                                  double* h, double* red) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int i0 = 4 * wave; i0 < n; i0 += 4 * NW) {
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (int c = lane; c < k; c += 64) {
      const double z = w[c];
#pragma unroll
      for (int t = 0; t < 4; ++t)
        if (i0 + t < n) s[t] += Q[(int64_t)(i0 + t) * k + c] * z;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
#pragma unroll
      for (int t = 0; t < 4; ++t) s[t] += __shfl_xor(s[t], o, 64);
    if (lane < 4 && i0 + lane < n) h[i0 + lane] = lane == 0 ? s[0] : lane == 1 ? s[1] : lane == 2 ? s[2] : s[3];
  }
  nr_sync<NW>();
  double nrm[1] = {0.0};
  for (int c = threadIdx.x; c < k; c += NW * 64) {
    double acc = 0.0;
    int i = 0;
    for (; i + 4 <= n; i += 4) {
      const double q0 = Q[(int64_t)i * k + c], q1 = Q[(int64_t)(i + 1) * k + c];
      const double q2 = Q[(int64_t)(i + 2) * k + c], q3 = Q[(int64_t)(i + 3) * k + c];
      acc += h[i] * q0 + h[i + 1] * q1 + h[i + 2] * q2 + h[i + 3] * q3;
    }
    for (; i < n; ++i) acc += h[i] * Q[(int64_t)i * k + c];
    const double z = w[c] - acc;
    w[c] = z;
    nrm[0] += z * z;
  }
  block_sums<1, NW>(nrm, red);
  return nrm[0];
}


// Packed symmetric storage of the lower triangle over kc = k + 1 columns (the
// last is the virtual all-ones column), in chunked column groups: column group
// g (columns 16 g .. 16 g + 15, pk_groups(kc) of them) holds rows 16 g .. kc - 1
// (entries above the diagonal stored as zero, columns >= kc of the last group
// as the zero padding the Gram produces there), cut into row chunks of 64 (the
// last one h = kc - 16 g - 64 j rows); chunk j stores its 16 columns one after
// the other, h rows each. A matvec unit (group, chunk) is then one contiguous
// run of 16 h doubles; every group, and every full chunk's column piece,
// starts on a 128-byte line (packed_matvec). Group g starts at pk_base(g, kc).
// (Round 4: rows are no longer padded to a multiple of 16 -- 17% fewer bytes
// per pass at C2's Lanczos dimension 100.)
// HD (the Gram-table kernel; profile_body): the diagonal entries of the node
// columns (c < k) hold G_cc / 2, exactly (fp64 and the fp32 copy alike). With
// the zeros above the diagonal, the matvec's lower part (w_r += G_rc x_c) and
// its mirrored part (w_c += G_rc x_r) then both run over every stored element
// without a test for the diagonal, each adding half of G_cc x_c. The table
// fill halves at its store of the diagonal (net_item); whoever reads G_cc
// itself doubles what is stored (start_column, profile_body's contributions).
// The ones row (k, c) and the corner (k, k) are stored as they are.
// HD is a compile-time flag of the kernel (profile_body: the Gram source is
// the table) that its fill, its matvec and its readers of G_cc all take. Every
// other packed kernel fills its Gram on the matrix cores (pk_store_tile,
// pk_store_tile16) and keeps the plain diagonal, the matvec's test for it and
// with them its outputs bit for bit: one null of
// tests/test_gpu_small.py::test_small_class_primal_only_vs_cpp_oracle (a
// near-degenerate top eigenpair) sits at 9.8e-11 of the oracle against the
// 1e-10 bar, and the halved diagonal's rounding moved it to 1.1e-10.
// A packed Gram never leaves the kernel that filled it.

// Stores one 16 x 16 MFMA accumulator tile of the Gram's super-tile (I2, J2)
// into the packed layout: lane (i16, kk) holds rows gj = 32 J2 + 16 b + i16 of
// columns gi = 32 I2 + 16 a + kk + 4 r (f64 MFMA C/D map). The tile lies in
// one column group (g = 2 I2 + a) and one row chunk, so the chunk, its height
// and the diagonal test are uniform over it.
__device__ __forceinline__ void pk_store_tile(double* G, float* G32, int kc, int I2, int J2, int a, int b,
                                              const nr_f64x4& v, int lane) {
  const int g = 2 * I2 + a;
  const int rb = 32 * (J2 - I2) + 16 * (b - a);  // first row of the tile, relative to the group's
  const int i16 = lane & 15, kk = lane >> 4;
  const int j = rb >> 6;
  const int h = min(64, kc - 16 * g - 64 * j);
  if (rb >= 0 && (rb & 63) + i16 < h) {  // not above the group, nor past row kc - 1
    const int base = (int)pk_base(g, kc) + 1024 * j + (rb & 63) + i16;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int t = kk + 4 * r;
      const double x = (rb == 0 && i16 < t) ? 0.0 : v[r];  // zero above the diagonal
      G[base + t * h] = x;
      if (G32) G32[base + t * h] = (float)x;  // the relaxed-phase copy (packed_matvec<NW, true>)
    }
  }
}

// G = [X 1]^T [X 1] over the k module columns of X (S x N, column-major) plus a
// virtual all-ones column at index k, so row k of G holds the column sums;
// both triangles stored, leading dimension ld >= round32(k + 1), or the packed
// lower triangle. 32 x 32 super-tiles (2 x 2 MFMA tiles of
// v_mfma_f64_16x16x4_f64) per wave; each lane feeds 4 consecutive rows of every
// operand column per 16-row step (the K order of the dot products is permuted,
// identically for both operands): two 16-byte loads per operand column, the
// next step's in flight during this step's 16 MFMAs. The ones column and the
// zero padding columns are real columns of the resident data block (N and
// N + 1, written at upload), so every lane loads unconditionally; only the
// last step (S not a multiple of 16) guards its rows. Non-finite data shows
// on G's diagonal (G_cc = sum of squares of column c), checked in the
// epilogue. Returns the per-lane part of 1^T G 1 over the X block and a
// non-finite flag.
template <int NW = NR_WAVES, bool PACKED = false>
__device__ void gram_mfma(const double* __restrict__ X, int S, const uint32_t* idx, int k, int64_t ones_off,
                          double* __restrict__ G, float* __restrict__ G32, int ld, double& g1sum, int& bad) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i16 = lane & 15, kk = lane >> 4;
  const int kc = k + 1;
  const int T2 = (kc + 31) / 32;
  const int nsup = T2 * (T2 + 1) / 2;
  const int full = S / 16 * 16;  // steps whose 16 rows are all in range
  // Whole rounds of super-tiles (one per wave); the last nsup % NW are cut into
  // their 16 x 16 tiles below, dealt over every wave (load balance).
  const int nfull = nsup - nsup % NW;
  for (int t = wave; t < nfull; t += NW) {
    int I2 = 0, rem = t;
    while (rem >= T2 - I2) { rem -= T2 - I2; ++I2; }
    const int J2 = I2 + rem;
    const double* col[4];
#pragma unroll
    for (int o = 0; o < 4; ++o) {
      const int c = (o < 2 ? I2 : J2) * 32 + (o & 1) * 16 + i16;
      const int64_t off = c < k ? (int64_t)idx[c] * S : (c == k ? ones_off : ones_off + S);
      col[o] = X + off + 4 * kk;
    }
    nr_f64x4 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b) acc[a][b] = nr_f64x4{0.0, 0.0, 0.0, 0.0};
    auto ld16 = [&](int s0, double (&v)[4][4]) {
#pragma unroll
      for (int o = 0; o < 4; ++o) {
        double2 p0, p1;
        __builtin_memcpy(&p0, col[o] + s0, sizeof(double2));
        __builtin_memcpy(&p1, col[o] + s0 + 2, sizeof(double2));
        v[o][0] = p0.x;
        v[o][1] = p0.y;
        v[o][2] = p1.x;
        v[o][3] = p1.y;
      }
    };
    auto mfma16 = [&](const double (&v)[4][4]) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(v[0][q], v[2][q], acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(v[0][q], v[3][q], acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(v[1][q], v[2][q], acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(v[1][q], v[3][q], acc[1][1], 0, 0, 0);
      }
    };
    double cur[4][4];
    // one 16-row step in flight (a second one spilled in the 3-workgroup
    // kernel and ran slower: profiles/r02/profile_variants.txt)
    double nxt[4][4];
    if (full > 0) ld16(0, cur);
    for (int s0 = 0; s0 < full; s0 += 16) {
      if (s0 + 16 < full) ld16(s0 + 16, nxt);
      mfma16(cur);
#pragma unroll
      for (int o = 0; o < 4; ++o)
#pragma unroll
        for (int q = 0; q < 4; ++q) cur[o][q] = nxt[o][q];
    }
    if (full < S) {  // the last, partial step
#pragma unroll
      for (int o = 0; o < 4; ++o)
#pragma unroll
        for (int q = 0; q < 4; ++q) cur[o][q] = full + 4 * kk + q < S ? col[o][full + q] : 0.0;
      mfma16(cur);
    }
    const double wgt = (I2 == J2) ? 1.0 : 2.0;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        if (PACKED) pk_store_tile(G, G32, kc, I2, J2, a, b, acc[a][b], lane);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          // D[row = (lane>>4) + 4r][col = lane & 15] (f64 MFMA C/D map)
          const int gi = I2 * 32 + 16 * a + kk + 4 * r;
          const int gj = J2 * 32 + 16 * b + i16;
          const double val = acc[a][b][r];
          if (!PACKED) {
            G[gi + (int64_t)gj * ld] = val;
            G[gj + (int64_t)gi * ld] = val;
          }
          if (gi < k && gj < k) g1sum += wgt * val;
          if (gi == gj && gi < k) bad |= (int)!isfinite(val);
        }
      }
  }
  // The remainder round: 4 (nsup % NW) single tiles over the NW waves, each
  // with one accumulator fed by its two 16-column operand blocks (same K
  // order as the super-tile path, so every G entry is bitwise the same).
  const int nsub = 4 * (nsup - nfull);
  for (int u = wave; u < nsub; u += NW) {
    const int t = nfull + (u >> 2), a = (u >> 1) & 1, b = u & 1;
    int I2 = 0, rem = t;
    while (rem >= T2 - I2) { rem -= T2 - I2; ++I2; }
    const int J2 = I2 + rem;
    const double* cp[2];
#pragma unroll
    for (int o = 0; o < 2; ++o) {
      const int c = (o == 0 ? I2 * 32 + 16 * a : J2 * 32 + 16 * b) + i16;
      const int64_t off = c < k ? (int64_t)idx[c] * S : (c == k ? ones_off : ones_off + S);
      cp[o] = X + off + 4 * kk;
    }
    nr_f64x4 acc1 = nr_f64x4{0.0, 0.0, 0.0, 0.0};
    auto ld4 = [&](int s0, double (&v)[2][4]) {
#pragma unroll
      for (int o = 0; o < 2; ++o) {
        double2 p0, p1;
        __builtin_memcpy(&p0, cp[o] + s0, sizeof(double2));
        __builtin_memcpy(&p1, cp[o] + s0 + 2, sizeof(double2));
        v[o][0] = p0.x;
        v[o][1] = p0.y;
        v[o][2] = p1.x;
        v[o][3] = p1.y;
      }
    };
    double c1[2][4], n1[2][4];
    if (full > 0) ld4(0, c1);
    for (int s0 = 0; s0 < full; s0 += 16) {
      if (s0 + 16 < full) ld4(s0 + 16, n1);
#pragma unroll
      for (int q = 0; q < 4; ++q) acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(c1[0][q], c1[1][q], acc1, 0, 0, 0);
#pragma unroll
      for (int o = 0; o < 2; ++o)
#pragma unroll
        for (int q = 0; q < 4; ++q) c1[o][q] = n1[o][q];
    }
    if (full < S) {  // the last, partial step
#pragma unroll
      for (int o = 0; o < 2; ++o)
#pragma unroll
        for (int q = 0; q < 4; ++q) c1[o][q] = full + 4 * kk + q < S ? cp[o][full + q] : 0.0;
#pragma unroll
      for (int q = 0; q < 4; ++q) acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(c1[0][q], c1[1][q], acc1, 0, 0, 0);
    }
    const double wgt = (I2 == J2) ? 1.0 : 2.0;
    if (PACKED) pk_store_tile(G, G32, kc, I2, J2, a, b, acc1, lane);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int gi = I2 * 32 + 16 * a + kk + 4 * r;
      const int gj = J2 * 32 + 16 * b + i16;
      const double val = acc1[r];
      if (!PACKED) {
        G[gi + (int64_t)gj * ld] = val;
        G[gj + (int64_t)gi * ld] = val;
      }
      if (gi < k && gj < k) g1sum += wgt * val;
      if (gi == gj && gi < k) bad |= (int)!isfinite(val);
    }
  }
}


// One 16 x 16 accumulator tile of column block gc (16 gc .. 16 gc + 15) and
// row block gr >= gc into the packed layout (pk_store_tile with block indices).
__device__ __forceinline__ void pk_store_tile16(double* G, float* G32, int kc, int gc, int gr, const nr_f64x4& v,
                                                int lane) {
  const int rb = 16 * (gr - gc);
  const int i16 = lane & 15, kk = lane >> 4;
  const int j = rb >> 6;
  const int h = min(64, kc - 16 * gc - 64 * j);
  if (rb >= 0 && (rb & 63) + i16 < h) {  // not above the group, nor past row kc - 1
    const int base = (int)pk_base(gc, kc) + 1024 * j + (rb & 63) + i16;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int t = kk + 4 * r;
      const double x = (rb == 0 && i16 < t) ? 0.0 : v[r];  // zero above the diagonal
      G[base + t * h] = x;
      if (G32) G32[base + t * h] = (float)x;
    }
  }
}

// The large modules' Gram (primal [X 1]^T[X 1], or the dual H of k > S) in
// 64 x 64 super-tiles per wave (4 x 4 MFMA tiles; the diagonal super-tiles
// skip their upper tiles): four times the MFMAs per operand load of the
// 32 x 32 scheme of gram_mfma / gram_mfma_dual, whose operand streams made the
// large items' Gram memory-bound (83% of a C5 item, profiles/r03/packed_big).
// Same operand layout, K order and epilogue as those two; needs the register
// budget of one wave per SIMD (the large-module kernel runs one workgroup
// per CU). Packed storage only.
template <int NW, bool DUAL>
__device__ void gram_mfma64(const double* __restrict__ X, int S, const uint32_t* idx, int k, int64_t ones_off,
                            double* __restrict__ G, float* __restrict__ G32, double& g1sum, int& bad) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i16 = lane & 15, kk = lane >> 4;
  const int kc = DUAL ? S + 1 : k + 1;
  const int T4 = (kc + 63) / 64;
  const int nsup = T4 * (T4 + 1) / 2;
  const int full = S / 16 * 16;  // primal: steps whose 16 rows are all in range
  // (Four waves on a 2 x 2 block of super-tiles instead of a row of four
  // read 4 operand panels per round instead of 5, but idle a wave in every
  // diagonal block: C5 profile kernel 56.6 vs 53.6 ms, profiles/r05/g64ab/.)
  for (int t = wave; t < nsup; t += NW) {
    int I4 = 0, rem = t;
    while (rem >= T4 - I4) { rem -= T4 - I4; ++I4; }
    const int J4 = I4 + rem;
    const bool diag = I4 == J4;
    // operand blocks: o < 4 the column side (16 (4 I4 + o) + i16), o >= 4 the row side
    const double* col[8];
    int cs[8];
#pragma unroll
    for (int o = 0; o < 8; ++o) {
      const int c = (o < 4 ? 4 * I4 + o : 4 * J4 + o - 4) * 16 + i16;
      cs[o] = c;
      if (!DUAL) {
        const int64_t off = c < k ? (int64_t)idx[c] * S : (c == k ? ones_off : ones_off + S);
        col[o] = X + off + 4 * kk;
      }
    }
    nr_f64x4 acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b) acc[a][b] = nr_f64x4{0.0, 0.0, 0.0, 0.0};
    auto mfma64 = [&](const double (&v)[8][4]) {
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
          for (int b = 0; b < 4; ++b)
            if (!diag || b >= a) acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(v[a][q], v[4 + b][q], acc[a][b], 0, 0, 0);
    };
    double cur[8][4], nxt[8][4];
    if (!DUAL) {
      auto ld16 = [&](int s0, double (&v)[8][4]) {
#pragma unroll
        for (int o = 0; o < 8; ++o) {
          double2 p0, p1;
          __builtin_memcpy(&p0, col[o] + s0, sizeof(double2));
          __builtin_memcpy(&p1, col[o] + s0 + 2, sizeof(double2));
          v[o][0] = p0.x;
          v[o][1] = p0.y;
          v[o][2] = p1.x;
          v[o][3] = p1.y;
        }
      };
      if (full > 0) ld16(0, cur);
      // the prefetched step copied into the current set (two register sets
      // used in turn spilled more: profiles/r03/big_gram64/)
      for (int s0 = 0; s0 < full; s0 += 16) {
        if (s0 + 16 < full) ld16(s0 + 16, nxt);
        mfma64(cur);
#pragma unroll
        for (int o = 0; o < 8; ++o)
#pragma unroll
          for (int q = 0; q < 4; ++q) cur[o][q] = nxt[o][q];
      }
      if (full < S) {  // the last, partial step
#pragma unroll
        for (int o = 0; o < 8; ++o)
#pragma unroll
          for (int q = 0; q < 4; ++q) cur[o][q] = full + 4 * kk + q < S ? col[o][full + q] : 0.0;
        mfma64(cur);
      }
    } else {
      // operand columns are samples (S: the row sums' all-ones node value,
      // beyond: zero), the contraction runs over the k nodes, 16 per step.
      // Super-tiles inside the first S samples (every one but the last row of
      // them) load unconditionally from the node's column at immediate
      // offsets; nodes past k load node k-1's values and select zero.
      const bool interior = 64 * J4 + 64 <= S;
      auto load = [&](int c0, double (&v)[8][4]) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int c = c0 + q;
          const bool valid = c < k;
          const double* colp = X + (int64_t)idx[valid ? c : k - 1] * S;
          if (interior) {
            const double* pi = colp + 64 * I4 + i16;
            const double* pj = colp + 64 * J4 + i16;
#pragma unroll
            for (int o = 0; o < 4; ++o) {
              const double xi = pi[16 * o], xj = pj[16 * o];
              v[o][q] = valid ? xi : 0.0;
              v[4 + o][q] = valid ? xj : 0.0;
            }
          } else {
#pragma unroll
            for (int o = 0; o < 8; ++o) {
              const double x = cs[o] < S ? colp[cs[o]] : (cs[o] == S ? 1.0 : 0.0);
              v[o][q] = valid ? x : 0.0;
            }
          }
        }
      };
      load(4 * kk, cur);
      for (int c0 = 0; c0 < k; c0 += 16) {
        if (c0 + 16 < k) load(c0 + 16 + 4 * kk, nxt);
        mfma64(cur);
#pragma unroll
        for (int o = 0; o < 8; ++o)
#pragma unroll
          for (int q = 0; q < 4; ++q) cur[o][q] = nxt[o][q];
      }
    }
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        if (diag && b < a) continue;
        pk_store_tile16(G, G32, kc, 4 * I4 + a, 4 * J4 + b, acc[a][b], lane);
        const double wgt = (diag && a == b) ? 1.0 : 2.0;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          // D[row = (lane>>4) + 4r][col = lane & 15] (f64 MFMA C/D map)
          const int gi = (4 * I4 + a) * 16 + kk + 4 * r;
          const int gj = (4 * J4 + b) * 16 + i16;
          const double val = acc[a][b][r];
          if (DUAL) {
            if (gj == S && gi < S) g1sum += val * val;  // |X 1|^2 from the row sums
            if (gi == gj && gi < S) bad |= (int)!isfinite(val);
          } else {
            if (gi < k && gj < k) g1sum += wgt * val;
            if (gi == gj && gi < k) bad |= (int)!isfinite(val);
          }
        }
      }
  }
}

// The large modules' dual Gram in 64 x 16 RW super-tiles per wave (round 6):
// a 64-wide column panel (4 blocks of 16) against a 16 RW-wide row panel (RW
// blocks), 4 x RW MFMA tiles in the wave's accumulator registers, with one
// register set of operands refilled column by column. 4 + RW operand blocks
// per 16-deep step feed 4 RW tiles (gram_mfma64: 8 feed 16), fewer operand
// reads per MFMA from L2 / the Infinity Cache, where the 64 x 64 scheme's
// Gram phase waits (38% MFMA-busy, profiles/r05/c5gram/). Every tile is
// computed, those above the diagonal (row block < column block) are not
// stored; the same operand layout, K order (bitwise the same Gram), packed
// stores and epilogue as gram_mfma64 otherwise. Measured on C5 (10,000
// permutations per dataset, profiles/r06/ab_gram/): RW = 4 (the rolling
// buffer alone) 984 perms/s, 6: 1,007, 7: 1,031, against 967 for
// gram_mfma64; RW = 8 (all 256 accumulator registers) spills ~1.1 KB per
// lane. The primal Gram (k <= S) keeps gram_mfma64: its 64 x 80 version was
// slower (997) and its 64 x 64 rolling version equal (1,007).
constexpr int kGramDualRows = 7;
template <int NW, bool DUAL, int RW>
__device__ void gram_mfma128(const double* __restrict__ X, int S, const uint32_t* idx, int k, int64_t ones_off,
                             double* __restrict__ G, float* __restrict__ G32, double& g1sum, int& bad) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i16 = lane & 15, kk = lane >> 4;
  const int kc = DUAL ? S + 1 : k + 1;
  const int RB = (kc + 15) / 16;  // 16-blocks of the side
  const int T4 = (RB + 3) / 4, T8 = (RB + RW - 1) / RW;
  int nsup = 0;
  for (int I4 = 0; I4 < T4; ++I4) nsup += T8 - 4 * I4 / RW;
  const int full = S / 16 * 16;
  for (int t = wave; t < nsup; t += NW) {
    int I4 = 0, rem = t;
    while (rem >= T8 - 4 * I4 / RW) {
      rem -= T8 - 4 * I4 / RW;
      ++I4;
    }
    const int R8 = 4 * I4 / RW + rem;
    // row block 8 R8 + b >= column block 4 I4 + a, i.e. b >= a + d (uniform per super-tile)
    const int d = 4 * I4 - RW * R8;  // -4 * (odd/even offset) .. 4
    // operand blocks: o < 4 the column side (16 (4 I4 + o) + i16), o >= 4 the row side (16 (8 R8 + o - 4) + i16)
    const double* col[4 + RW];
    int cs[4 + RW];
#pragma unroll
    for (int o = 0; o < 4 + RW; ++o) {
      const int c = (o < 4 ? 4 * I4 + o : RW * R8 + o - 4) * 16 + i16;
      cs[o] = c;
      if (!DUAL) {
        const int64_t off = c < k ? (int64_t)idx[c] * S : (c == k ? ones_off : ones_off + S);
        col[o] = X + off + 4 * kk;
      }
    }
    nr_f64x4 acc[4][RW];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < RW; ++b) acc[a][b] = nr_f64x4{0.0, 0.0, 0.0, 0.0};
    // one register set of operands, refilled column q by column q: once a
    // step's MFMAs have read v[.][q], the next step's v[.][q] is loaded into
    // the same registers while the MFMAs of q + 1.. run (96 VGPRs of operands
    // instead of two 96-register sets; the loads are unconditional -- the
    // last step re-reads its own operands -- so the waits count them exactly)
    double v[4 + RW][4];
    // every tile of the super-tile, the ones above the diagonal too (not
    // stored): a branch per tile split the loop and spilled; the extra MFMAs
    // (~10% over the triangle) are free in this operand-bound phase
    auto mfma_q = [&](int q) {
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < RW; ++b)
          acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(v[a][q], v[4 + b][q], acc[a][b], 0, 0, 0);
    };
    if (!DUAL) {
      auto ldp = [&](int s0, int qp) {  // samples s0 + 4 kk + 2 qp, + 1 of every operand column
#pragma unroll
        for (int o = 0; o < 4 + RW; ++o) {
          double2 p;
          __builtin_memcpy(&p, col[o] + s0 + 2 * qp, sizeof(double2));
          v[o][2 * qp] = p.x;
          v[o][2 * qp + 1] = p.y;
        }
      };
      if (full > 0) {
        ldp(0, 0);
        ldp(0, 1);
      }
      for (int s0 = 0; s0 < full; s0 += 16) {
        const int sn = s0 + 16 < full ? s0 + 16 : s0;
        mfma_q(0);
        mfma_q(1);
        ldp(sn, 0);
        mfma_q(2);
        mfma_q(3);
        ldp(sn, 1);
      }
      if (full < S) {  // the last, partial step
#pragma unroll
        for (int o = 0; o < 4 + RW; ++o)
#pragma unroll
          for (int q = 0; q < 4; ++q) v[o][q] = full + 4 * kk + q < S ? col[o][full + q] : 0.0;
#pragma unroll
        for (int q = 0; q < 4; ++q) mfma_q(q);
      }
    } else {
      // operand columns are samples (S: the ones row, beyond: zero), the
      // contraction over the k nodes, 16 per step (node c0 + 4 kk + q in
      // column q); super-tiles whose row panel lies inside the first S
      // samples load at immediate offsets
      const bool interior = 16 * RW * R8 + 16 * RW <= S;
      auto ldq = [&](int c, int q) {
        const bool valid = c < k;
        const double* colp = X + (int64_t)idx[valid ? c : k - 1] * S;
        if (interior) {
          const double* pi = colp + 64 * I4 + i16;
          const double* pj = colp + 16 * RW * R8 + i16;
#pragma unroll
          for (int o = 0; o < 4; ++o) {
            const double xi = pi[16 * o];
            v[o][q] = valid ? xi : 0.0;
          }
#pragma unroll
          for (int o = 0; o < RW; ++o) {
            const double xj = pj[16 * o];
            v[4 + o][q] = valid ? xj : 0.0;
          }
        } else {
#pragma unroll
          for (int o = 0; o < 4 + RW; ++o) {
            const double x = cs[o] < S ? colp[cs[o]] : (cs[o] == S ? 1.0 : 0.0);
            v[o][q] = valid ? x : 0.0;
          }
        }
      };
#pragma unroll
      for (int q = 0; q < 4; ++q) ldq(4 * kk + q, q);
      for (int c0 = 0; c0 < k; c0 += 16) {
        const int cn = c0 + 16 < k ? c0 + 16 : c0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          mfma_q(q);
          ldq(cn + 4 * kk + q, q);
        }
      }
    }
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < RW; ++b) {
        if (b < a + d) continue;
        const int gc = 4 * I4 + a, gr = RW * R8 + b;
        pk_store_tile16(G, G32, kc, gc, gr, acc[a][b], lane);
        const double wgt = gc == gr ? 1.0 : 2.0;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int gi = gc * 16 + kk + 4 * r;
          const int gj = gr * 16 + i16;
          const double val = acc[a][b][r];
          if (DUAL) {
            if (gj == S && gi < S) g1sum += val * val;
            if (gi == gj && gi < S) bad |= (int)!isfinite(val);
          } else {
            if (gi < k && gj < k) g1sum += wgt * val;
            if (gi == gj && gi < k) bad |= (int)!isfinite(val);
          }
        }
      }
  }
}

// Dual Gram for modules with more nodes than samples (k > S): H = [X' 1]' [X' 1]
// over the k module nodes, i.e. X X' (S x S) bordered by the row sums X 1 and
// k. Its top eigenvector is the summary profile u itself (the left singular
// vector svd_econ returns, src/netStats.cpp:229-236), so Lanczos runs in
// dimension S instead of k and the Gram costs 2 k S^2 flops instead of
// 2 S k^2. Same super-tile / storage scheme as gram_mfma with the roles of
// samples and nodes exchanged: operand columns are samples (16 consecutive
// samples of one node per lane group: one 128-byte read), the contraction
// runs over the nodes. Returns the per-lane part of |X 1|^2 (= 1'G1 of the
// primal Gram; here the squared norm of H's ones column) and a non-finite flag
// (from H's diagonal).
template <int NW = NR_WAVES, bool PACKED = false>
__device__ void gram_mfma_dual(const double* __restrict__ X, int S, const uint32_t* idx, int k,
                               double* __restrict__ G, float* __restrict__ G32, int ld, double& g1sum, int& bad) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i16 = lane & 15, kk = lane >> 4;
  const int kc = S + 1;
  const int T2 = (kc + 31) / 32;
  const int nsup = T2 * (T2 + 1) / 2;
  for (int t = wave; t < nsup; t += NW) {
    int I2 = 0, rem = t;
    while (rem >= T2 - I2) { rem -= T2 - I2; ++I2; }
    const int J2 = I2 + rem;
    const int cols[4] = {I2 * 32 + i16, I2 * 32 + 16 + i16, J2 * 32 + i16, J2 * 32 + 16 + i16};
    nr_f64x4 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b) acc[a][b] = nr_f64x4{0.0, 0.0, 0.0, 0.0};
    auto load = [&](int c0, double (&v)[4][4]) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int c = c0 + q;
        const double* col = c < k ? X + (int64_t)idx[c] * S : nullptr;
#pragma unroll
        for (int o = 0; o < 4; ++o)
          v[o][q] = col ? (cols[o] < S ? col[cols[o]] : (cols[o] == S ? 1.0 : 0.0)) : 0.0;
      }
    };
    double cur[4][4], nxt[4][4];
    load(4 * kk, cur);
    for (int c0 = 0; c0 < k; c0 += 16) {
      if (c0 + 16 < k) load(c0 + 16 + 4 * kk, nxt);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(cur[0][q], cur[2][q], acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(cur[0][q], cur[3][q], acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(cur[1][q], cur[2][q], acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(cur[1][q], cur[3][q], acc[1][1], 0, 0, 0);
      }
#pragma unroll
      for (int o = 0; o < 4; ++o)
#pragma unroll
        for (int q = 0; q < 4; ++q) cur[o][q] = nxt[o][q];
    }
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        if (PACKED) pk_store_tile(G, G32, kc, I2, J2, a, b, acc[a][b], lane);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int gi = I2 * 32 + 16 * a + kk + 4 * r;
          const int gj = J2 * 32 + 16 * b + i16;
          const double val = acc[a][b][r];
          if (!PACKED) {
            G[gi + (int64_t)gj * ld] = val;
            G[gj + (int64_t)gi * ld] = val;
          }
          if (gj == S && gi < S) g1sum += val * val;  // |X 1|^2 from the row sums (X 1)_gi
          if (gi == gj && gi < S) bad |= (int)!isfinite(val);  // H_ss: squares of sample s's values
        }
      }
  }
}

// w = G x over the leading k x k block of the PACKED symmetric G (pk_at), NW
// waves. Work units are (column group, row chunk) pairs, numbered group-major
// and cut into NW contiguous ranges, one per wave; a unit is one contiguous
// run of 16 column pieces (16 back-to-back raw buffer loads, lanes own rows,
// no lane mask except past a short last chunk). Its lower part
// (w_r += G_rc x_c) is lane-local and added to the wave's row partials; the
// mirrored upper part (w_c += sum_{r>c} G_rc x_r) accumulates lane-locally
// over the wave's units of one group and is reduced over the lanes by the
// register butterfly once per (wave, group). HD (the diagonal stored halved,
// the Gram-table kernel): both parts take every stored element -- the entries
// above the diagonal are zero, and the diagonal term is the sum of the two
// parts' halves; otherwise the mirrored part tests for the diagonal block.
// Rows >= k and columns >= k carry x = 0.
// Both parts go to the wave's one partial array (the wave's own
// LDS operations are ordered), and per-wave arrays keep the sums
// deterministic; they are zero on entry (zeroed once per kernel and again by
// the combine that reads them). Returns sum_r y_r out_r if y. (tools/probes/matvec_probe.hip: 17-23%
// faster per pass than row-block units over the plain packed triangle.)
//
// F32: the same matvec over the fp32 copy of G (G32, same packed indexing),
// the Lanczos steps after the residual has dropped below 1e-7 theta
// (lanczos_ritz): half the bytes per pass, fp64 arithmetic.
//
// SQ: out_r = sum_c G_rc^2 over c < k instead (squared row norms of the
// leading k x k block, for start_column; x and y unused). HD: the two parts
// each add (G_cc / 2)^2; the combine adds the remaining G_cc^2 / 2.
template <int NW, bool F32 = false, bool SQ = false, bool HD = false>
__device__ __forceinline__ double packed_matvec(const void* __restrict__ G, int kc, int k, const double* x,
                                                 double* out, double* part, int ks,
                                                 const double* y, double* red) {
  constexpr int EB = F32 ? 4 : 8;  // element bytes
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int P = kc;  // rows of the packed layout
  const auto rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)G, (short)0, (int)(pk_base(pk_groups(kc), P) * EB),
                                                      0x00020000);
  const int ncg = (k + 15) / 16;
  int n_units = 0;
  for (int g = 0; g < ncg; ++g) n_units += (P - 16 * g + 63) >> 6;
  const int u0 = n_units * wave / NW, u1 = n_units * (wave + 1) / NW;
  int cg = 0, first = 0;
  while (first + ((P - 16 * cg + 63) >> 6) <= u0) {
    first += (P - 16 * cg + 63) >> 6;
    ++cg;
  }
  int j = u0 - first;
  int nj = (P - 16 * cg + 63) >> 6;
  double up[16];
#pragma unroll
  for (int t = 0; t < 16; ++t) up[t] = 0.0;
  // Units in flight per wave: the fp32 pieces of two units occupy the
  // registers of one fp64 unit, so the relaxed (F32) passes issue two units'
  // loads (32 per lane) before the first wait; the matvec is latency-bound at
  // three workgroups per CU, not byte-bound (profiles/r02/profile_variants.txt).
  // A unit beyond the wave's range loads nothing (range-checked offsets).
  constexpr int UF = F32 ? 2 : NR_MV_UF64;
  using LT = typename std::conditional<F32, float, double>::type;
  for (int u = u0; u < u1; u += UF) {
    LT gb[UF][16];
    {
      int lcg = cg, lj = j;
#pragma unroll
      for (int i = 0; i < UF; ++i) {
        const bool valid = u + i < u1;
        const int h = min(64, P - 16 * lcg - 64 * lj);
        const int64_t base = pk_base(lcg, P) + 1024 * (int64_t)lj;
        const int vo = valid && lane < h ? lane * EB : (int)0x80000000;
        int so = valid ? (int)base * EB : 0;
#pragma unroll
        for (int t = 0; t < 16; ++t) {
          if (F32)
            gb[i][t] = (LT)__builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrc, vo, so, 0));
          else
            gb[i][t] = __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(rsrc, vo, so, 0));
          so += h * EB;
        }
        if (++lj == ((P - 16 * lcg + 63) >> 6)) {
          ++lcg;
          lj = 0;
        }
      }
    }
#pragma unroll
    for (int i = 0; i < UF; ++i) {
      if (u + i >= u1) break;
      const int c0 = cg * 16;
      const int r = c0 + 64 * j + lane;
      const double xr = SQ ? (r < k ? 1.0 : 0.0) : (r < k ? x[r] : 0.0);  // SQ: row mask
      // one pass over the unit's 16 pieces, each converted where it is used
      // (no 16-double copy next to the next unit's pieces in flight)
      // HD: the diagonal entry is stored halved and the entries above it as
      // zero (packed_gram_doubles), so the lower and the mirrored part each
      // take every element of the unit: the two halves of G_cc x_c add up to
      // the diagonal term, with no test for the diagonal block.
      const bool diag = j == 0;  // the chunk holding the group's diagonal block (!HD)
      double acc = 0.0;
      if (SQ) {
#pragma unroll
        for (int t = 0; t < 16; ++t) {
          const double gt = (double)gb[i][t];
          const double g2 = gt * gt;  // the mirrored part sums squares too
          // (the column mask stays per element: a second copy of the loop for
          // the last group behind a wave-uniform branch took the table kernel
          // from 72 to 228 bytes of scratch per lane, and this pass runs once
          // per item)
          acc += c0 + t < k ? g2 : 0.0;
          if (HD)
            up[t] = fma(g2, xr, up[t]);
          else
            up[t] += (!diag || r > c0 + t) ? g2 * xr : 0.0;
        }
      } else {
        const double xl = c0 + (lane & 15) < k ? x[c0 + (lane & 15)] : 0.0;  // the unit's 16 x_c, one per lane
#pragma unroll
        for (int t = 0; t < 16; ++t) {
          const double gt = (double)gb[i][t];
          acc += gt * nr_readlane_f64(xl, t);  // (saves 30 VGPRs over 16 LDS reads)
          if (HD)
            up[t] = fma(gt, xr, up[t]);
          else
            up[t] += (!diag || r > c0 + t) ? gt * xr : 0.0;
        }
      }
      if (r < k) part[wave * ks + r] += acc;
      ++j;
      if (j == nj || u + i + 1 == u1) {
        const double v = nr_transpose_reduce16(up, lane);
        if ((lane & 3) == 0) {
          const int c = c0 + ((lane >> 5) & 1) * 8 + ((lane >> 4) & 1) * 4 + ((lane >> 3) & 1) * 2 + ((lane >> 2) & 1);
          if (c < k) part[wave * ks + c] += v;
        }
#pragma unroll
        for (int t = 0; t < 16; ++t) up[t] = 0.0;
        ++cg;
        j = 0;
        nj = (P - 16 * cg + 63) >> 6;
      }
    }
  }
  __syncthreads();
  double d[1] = {0.0};
  for (int rr = threadIdx.x; rr < k; rr += NW * 64) {
    double sum = 0.0;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
      sum += part[w * ks + rr];
      part[w * ks + rr] = 0.0;  // zero again for the next matvec (block_sums' barriers order it)
    }
    if (SQ && HD) {  // the two parts each added (G_cc / 2)^2: the other half of G_cc^2
      const double hd = (double)static_cast<const LT*>(G)[pk_col(rr, kc)];
      sum += 2.0 * hd * hd;
    }
    out[rr] = sum;
    if (y) d[0] += y[rr] * sum;
  }
  // y . out, without the trailing barrier (the caller's next writer of `red`
  // is behind a barrier); no y: each thread reads back only its own out[]
  // entries before the caller's next barrier
  if (y) block_sums<1, NW, false>(d, red);
  return d[0];
}

// Lanczos start vector: column c* of the packed symmetric G (leading n x n
// block) with the largest norm, i.e. G e_c* for the node whose row of G is
// largest. That node carries a large share of the top eigenvector, and G e_c*
// is e_c* one Krylov step on for free (the column is already stored): offline
// on C3 null items 33.3 vs 35.8 Lanczos steps for the near-constant start
// (200 items, paired difference -2.5 +- 0.1). Norms from one squared pass over
// the fp32 copy when present (only their order matters; deterministic: fixed
// summation order, ties to the smaller index). q <- G e_c* (fp64); cn: n
// doubles of LDS work space. Returns false (q untouched) if every column is
// zero. Ends with a barrier.
template <int NW, bool HD>
__device__ __forceinline__ bool start_column(const double* __restrict__ G, const float* __restrict__ G32, int kc,
                                             int n, double* q, double* cn, double* part, int ks, double* red) {
  constexpr int BS = NW * 64;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (G32)
    packed_matvec<NW, true, true, HD>(G32, kc, n, nullptr, cn, part, ks, nullptr, red);
  else
    packed_matvec<NW, false, true, HD>(G, kc, n, nullptr, cn, part, ks, nullptr, red);
  __syncthreads();
  double best = -1.0;
  int bi = 0x7fffffff;
  for (int r = tid; r < n; r += BS) {
    const double v = cn[r];
    if (v > best) {  // increasing r per thread: the first maximum is kept
      best = v;
      bi = r;
    }
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const double ov = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (ov > best || (ov == best && oi < bi)) {
      best = ov;
      bi = oi;
    }
  }
  if (lane == 0) {
    red[wave] = best;
    red[NW + wave] = (double)bi;
  }
  __syncthreads();
  best = red[0];
  bi = (int)red[NW];
#pragma unroll
  for (int w = 1; w < NW; ++w) {
    const double ov = red[w];
    const int oi = (int)red[NW + w];
    if (ov > best || (ov == best && oi < bi)) {
      best = ov;
      bi = oi;
    }
  }
  const bool ok = best > 0.0 && bi < n;  // uniform over the workgroup
  if (ok)
    for (int r = tid; r < n; r += BS) {
      const int64_t a = pk_at(r > bi ? r : bi, r > bi ? bi : r, kc);
      q[r] = HD && r == bi ? 2.0 * G[a] : G[a];  // HD: the diagonal is stored halved
    }
  __syncthreads();  // q published; red free again
  return ok;
}

// Classical Gram-Schmidt of w against the stored basis Q (column-major k x n),
// register-butterfly form used by the packed kernels: h = Q^T w over units of
// (16 basis vectors x 64-row block), each a 16-load burst of raw buffer loads
// (out-of-range lanes zeroed by the range check) reduced over the rows by
// nr_transpose_reduce16. Row blocks are split into ns slices (ns * n <= hp_cap;
// ns = ceil(k/64) for modules of <= 320 nodes) whose partials hp[sl * n + i]
// are summed in a fixed order. Then w <- w - Q h with eight basis vectors per
// load burst. Returns |w|^2.
template <int NW>
__device__ __forceinline__ double reorthogonalise_bf(const double* __restrict__ Q, int k, int n, double* w,
                                                     double* h, double* hp, int hp_cap, double* red) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int nrb = (k + 63) / 64, ng = (n + 15) / 16;
  const int ns = max(1, min(nrb, hp_cap / n));
  const auto rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)Q, (short)0, n * k * 8, 0x00020000);
  for (int u = wave; u < ns * ng; u += NW) {
    const int sl = u / ng, g = u - sl * ng;
    double acc16[16];
#pragma unroll
    for (int t = 0; t < 16; ++t) acc16[t] = 0.0;
    for (int rb = sl; rb < nrb; rb += ns) {
      const int r = rb * 64 + lane;
      const double wr = w[min(r, k - 1)];  // rows >= k load 0
      double s16[16];
#pragma unroll
      for (int t = 0; t < 16; ++t) {
        const int i = g * 16 + t;
        const bool ok = r < k && i < n;
        s16[t] = __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(
                                                rsrc, ok ? r * 8 : (int)0x80000000, i * k * 8, 0));
      }
#pragma unroll
      for (int t = 0; t < 16; ++t) acc16[t] = fma(s16[t], wr, acc16[t]);
    }
    const double v = nr_transpose_reduce16(acc16, lane);
    if ((lane & 3) == 0) {
      const int i = g * 16 + ((lane >> 5) & 1) * 8 + ((lane >> 4) & 1) * 4 + ((lane >> 3) & 1) * 2 +
                    ((lane >> 2) & 1);
      if (i < n) hp[sl * n + i] = v;
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < n; i += NW * 64) {
    double a = 0.0;
    for (int sl = 0; sl < ns; ++sl) a += hp[sl * n + i];
    h[i] = a;
  }
  __syncthreads();
  double nrm[1] = {0.0};
  for (int c = threadIdx.x; c < k; c += NW * 64) {
    double acc = 0.0;
    int i = 0;
    for (; i + 8 <= n; i += 8) {
      double q8[8];
#pragma unroll
      for (int t = 0; t < 8; ++t) q8[t] = Q[(int64_t)(i + t) * k + c];
#pragma unroll
      for (int t = 0; t < 8; ++t) acc += h[i + t] * q8[t];
    }
    for (; i < n; ++i) acc += h[i] * Q[(int64_t)i * k + c];
    const double z = w[c] - acc;
    w[c] = z;
    nrm[0] += z * z;
  }
  block_sums<1, NW>(nrm, red);
  return nrm[0];
}

// ---------------------------------------------------------------------------
// Summary-profile item pipeline, shared by every Gram storage scheme:
//   index set -> Gram (scheme) -> Lanczos top eigenpair (lanczos_ritz) ->
//   node contributions (profile_contrib) -> statistics (profile_stats).
// ---------------------------------------------------------------------------




// One-wave Lanczos helpers (the wave class): the basis Q (column-major
// k x n, k <= 128) lives in the slot's global scratch, and a single wave has
// no other waves to hide a load's latency behind, so each pass keeps 16 basis
// vectors' loads (both rows of a lane: c = lane, lane + 64) in flight.
//
// Classical Gram-Schmidt of w against q_0..q_{n-1} in ONE pass over the
// basis: h_i = q_i . w for a burst of 16 vectors (transpose-reduce over the
// lanes, published through h in LDS), and their share of Q h subtracted from
// the same registers (CGS: every h_i comes from the original w). Returns |w|^2.
__device__ __forceinline__ double reorthogonalise_wave(const double* __restrict__ Q, int k, int n, double* w,
                                                       double* h) {
  const int lane = threadIdx.x & 63;
  const bool r0 = lane < k, r1 = lane + 64 < k;
  const double w0 = r0 ? w[lane] : 0.0, w1 = r1 ? w[lane + 64] : 0.0;
  double d0 = 0.0, d1 = 0.0;
  for (int i0 = 0; i0 < n; i0 += 16) {
    double a[16], b[16], p[16];
#pragma unroll
    for (int t = 0; t < 16; ++t) {
      const int i = i0 + t;
      a[t] = i < n && r0 ? Q[(int64_t)i * k + lane] : 0.0;
      b[t] = i < n && r1 ? Q[(int64_t)i * k + lane + 64] : 0.0;
    }
#pragma unroll
    for (int t = 0; t < 16; ++t) p[t] = fma(b[t], w1, a[t] * w0);
    const double v = nr_transpose_reduce16(p, lane);
    if ((lane & 3) == 0) {
      const int t = ((lane >> 5) & 1) * 8 + ((lane >> 4) & 1) * 4 + ((lane >> 3) & 1) * 2 + ((lane >> 2) & 1);
      if (i0 + t < n) h[i0 + t] = v;
    }
    nr_sync<1>();
#pragma unroll
    for (int t = 0; t < 16; ++t) {
      const double ht = i0 + t < n ? h[i0 + t] : 0.0;
      d0 = fma(ht, a[t], d0);
      d1 = fma(ht, b[t], d1);
    }
  }
  const double z0 = w0 - d0, z1 = w1 - d1;
  if (r0) w[lane] = z0;
  if (r1) w[lane + 64] = z1;
  return nr_wave_sum(z0 * z0 + z1 * z1);
}

// v = Q y over the first n basis vectors (rows c = lane, lane + 64 < k), the
// terms in basis order as the general loop.
__device__ __forceinline__ void ritz_vector_wave(const double* __restrict__ Q, int k, int n, const double* y,
                                                 double* v) {
  const int lane = threadIdx.x & 63;
  const bool r0 = lane < k, r1 = lane + 64 < k;
  double s0 = 0.0, s1 = 0.0;
  for (int i0 = 0; i0 < n; i0 += 16) {
    double a[16], b[16];
#pragma unroll
    for (int t = 0; t < 16; ++t) {
      const int i = i0 + t;
      a[t] = i < n && r0 ? Q[(int64_t)i * k + lane] : 0.0;
      b[t] = i < n && r1 ? Q[(int64_t)i * k + lane + 64] : 0.0;
    }
#pragma unroll
    for (int t = 0; t < 16; ++t) {
      const double yt = i0 + t < n ? y[i0 + t] : 0.0;
      s0 = fma(yt, a[t], s0);
      s1 = fma(yt, b[t], s1);
    }
  }
  if (r0) v[lane] = s0;
  if (r1) v[lane + 64] = s1;
  nr_sync<1>();
}

// Lanczos for the top eigenpair of the k x k operator mv (mv(x, out, y)
// writes out = G x for rows < k and returns y . out; x is zero beyond k):
// three-term update, partial reorthogonalisation by the omega recurrence
// (one CGS pass against the basis Q, k x mcap in global scratch), top Ritz
// pair of the tridiagonal by Sturm multisection + inverse iteration at
// predicted convergence checks. Leaves the normalised Ritz vector in L.vv.
// relax (optional): set from the first check whose residual is below
// 1e-7 theta on; the caller's mv then reads the fp32 copy of G. Matvec errors
// that late no longer move the converged Ritz vector (relaxed Krylov
// accuracy: the later a step, the smaller its weight in the Ritz vector;
// offline study on C3 null items, tools/sim_lanczos_relax.py: same steps, same
// 2e-14 worst eigenvector error as fp64 throughout, 19% fewer Gram bytes).
// q_given: start from the vector the caller left in L.q (start_column's
// G e_c*) instead of the near-constant one. gv_out: also leave G v in L.gv,
// from the Lanczos relation (see the end of the function).
// BIG: the large-module kernel, whose register allocation is the tightest:
// it keeps the previous loops of the tridiagonal eigenvector (the grouped
// ones put spill code into its Gram loop).
template <int NW, bool BF, class MV, bool BIG = false>
__device__ __forceinline__ void lanczos_ritz(const ProfileParams& P, int k, const LzLds& L, int* flags,
                                             double* Q, MV& mv, uint64_t& t_mark, bool* relax = nullptr,
                                             bool q_given = false, bool gv_out = false) {
  constexpr int BS = NW * 64;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int mmax = L.mmax;
  double* q = L.q;
  double* qprev = L.qprev;
  double* w = L.w;
  double* red = L.red;
  double* alpha = L.alpha;
  double* beta = L.beta;
  double* h = L.h;
  double* ty = L.ty;
  double* twork = L.twork;
  double* omg = L.omg;
  int& s_done = flags[2];
  int& s_reorth = flags[3];
  int& s_next_check = flags[4];

  const int mcap = k < mmax ? k : mmax;
  double nq[1] = {0.0};
  for (int c = tid; c < k; c += BS) {
    const uint32_t hsh = nr_lowbias32((uint32_t)c * 0x9E3779B9u + 0x1234567u);
    const double v = q_given ? q[c] : 1.0 + 0.01 * ((double)(hsh & 0xFFFF) / 65536.0 - 0.5);
    q[c] = v;
    qprev[c] = 0.0;
    nq[0] += v * v;
  }
  block_sums<1, NW>(nq, red);
  {
    const double inv = 1.0 / sqrt(nq[0]);
    for (int c = tid; c < k; c += BS) q[c] *= inv;
  }
  if (tid == 0) s_done = 0;
  nr_sync<NW>();
  int nsteps = 0;
  double beta_prev = 0.0;
  // First convergence check at step 16; later checks where the residual's
  // geometric decay since the previous check predicts convergence (at most 8
  // steps on). Offline study on C3 null items (tools/sim_lanczos.py): 36.0
  // steps/item vs 37.9 for a fixed 8-step cadence, same number of checks.
  // (the wave class checks first at step 18: its lone wave pays for every
  // check's Sturm passes in full; round 5 measured 20 against 16 on the C2
  // shape, 1.908 -> 1.841 ms per 256 permutations; on round 6's cheaper
  // checks, C2's profile kernel at 16 / 18 / 20 / 22 / 24: 24.69 / 24.24 /
  // 24.87 / 25.41 / 25.61 ms per 5,120, profiles/r06/ab_firstcheck/. The
  // 4-wave kernels keep 16: at C3, 20 and 24 measured -0.2% and +0.9%,
  // profiles/r05/firstcheck/; on the cheaper checks 18 and 20 +0.03% and
  // +0.8%, profiles/r06/ab_firstcheck_c3/)
  constexpr int first_check = NW == 1 ? 18 : 16;
  int next_check = mcap < first_check ? mcap : first_check;
  int prev_j = 0;  // lane 0 of wave 0 only
  double prev_r = 0.0;
  double hint_theta = 0.0, hint_r = 0.0;  // previous check, every lane of wave 0 (warm start)
  const double sqrt_eps = 1.4901161193847656e-08;
  // The omega recurrence reorthogonalises at an estimated loss of orthogonality
  // of sqrt(eps) (Simon), which keeps the Ritz VALUES at eps. The Ritz vector
  // Q y inherits the loss itself, weighted by y: nothing on runs that converge
  // in a few dozen steps (y is small where the loss sits), but on a top that
  // is one end of a dense ramp of eigenvalues (flat(0.3),
  // tests/test_gpu_spectra.py) runs of 60-130 steps left 1e-9 in the summary
  // profile, and a long fp32 phase on top of that loss ended on a wrong
  // vector. A numpy restatement of these rules puts the damage between steps 8
  // and 16 (a tighter bound from step 16 or 48 on changes nothing) and gives
  // 1e-9 .. 4e-9 at sqrt(eps), 2e-12 at a bound of 1e-11. The tight bound on
  // every item measured 2.4% slower on the C3 benchmark, and the residual at
  // the first check does not tell the slow runs apart (C3 null items reach
  // 2e-3 theta there, flat(0.3) starts at 2e-3). So: a run that took more
  // than 64 steps (C3 null items: 35 on average, 51 at most of 60 emulated)
  // is run again from the same q_0 with the bound at 1e-11, and dimensions up
  // to 64, where a reorthogonalisation costs next to nothing and a run cannot
  // get that long, use it from the start. Every other run is bit for bit what
  // it was.
  constexpr int kLongRun = 64;
  int tight = k <= kLongRun;  // (uniform: a scalar register)
  bool force_next = false;
  double anorm = 0.0;
  if (tid == 0) {
    omg[0] = 1.0;  // omega_{0,0}
    s_reorth = 0;
    flags[5] = 0;  // relaxed (fp32) matvecs
    // the next check is predicted to end the run: its eigenvalue to full
    // precision in one go. Not the first check (the wave class's, at step
    // 20, was one stage: measured faster there, profiles/r06/ab_checks/; at
    // step 18 the coarse stage first is 0.4% faster, profiles/r06/ab_coarse/)
    flags[6] = 0;
  }
  for (int c = tid; c < k; c += BS) Q[c] = q[c];  // q_0 (later q_j are stored by the update below)
  bool again;
  do {
  again = false;
  for (int j = 0; j < mcap; ++j) {
    NR_STAMP(2);  // Lanczos: vector updates / tridiagonal checks
    // Barriers per step: the matvec's combine and its sum, the 3-term norm,
    // the omega decision, and one after the q update (+ one per check). The
    // two block sums write alternate halves of `red` and skip their trailing
    // barrier: the next writer of each half is behind the omega barrier.
    const double alpha0 = mv(q, w, q);
    NR_STAMP(3);  // Lanczos: matvec
    double nb = three_term<NW>(k, w, q, qprev, alpha0, beta_prev, red + NW);
    double alpha_j = alpha0;
    double* om_cur = omg + (j % 3) * (mmax + 1);
    double* om_prev = omg + ((j + 2) % 3) * (mmax + 1);
    double* om_next = omg + ((j + 1) % 3) * (mmax + 1);
    // one wave: |w| and the q update's scale 1/|w| before the omega phase, off
    // the chain after its fence (recomputed when the step reorthogonalises).
    // C2's wave class -1.7%; the 4-wave table kernel measured +0.2% and keeps
    // the previous order (profiles/r06/ab_inv/)
    constexpr bool EARLY = NW == 1 && !BIG;
    const double beta0 = sqrt(nb);
    const double inv0 = EARLY ? 1.0 / beta0 : 0.0;
    anorm = fmax(anorm, fabs(alpha0) + beta0 + beta_prev);
    bool reorth = false;  // one wave: decided in registers (omega_update's max is wave-uniform), no LDS round trip
    if (wave == 0) {  // alpha[j] passed in registers: no barrier before the recurrence
      const double mx = omega_update(alpha, beta, j, alpha0, beta0, om_cur, om_prev, om_next, anorm, k, lane);
      if constexpr (NW == 1)
        reorth = __builtin_amdgcn_readfirstlane((int)(force_next || mx > (tight ? 1e-11 : sqrt_eps))) != 0;  // a scalar branch
      else if (lane == 0)
        s_reorth = force_next || mx > (tight ? 1e-11 : sqrt_eps);
    }
    nr_sync<NW>();
    NR_STAMP(4);  // Lanczos: three-term step + omega recurrence
    const bool reorthed = NW == 1 ? reorth : s_reorth != 0;
    if (reorthed) {  // reorthogonalise q_{j+1} against q_0..q_j, and the next one too
      if constexpr (NW == 1)
        nb = reorthogonalise_wave(Q, k, j + 1, w, h);
      else
        nb = BF ? reorthogonalise_bf<NW>(Q, k, j + 1, w, h, twork, 5 * mmax, red)  // twork idle until the next check
                : reorthogonalise_cgs<NW>(Q, k, j + 1, w, h, red);
      if (BF) {  // twork is the packed matvec's partial array: zero again
        for (int i = tid; i < 5 * mmax; i += BS) twork[i] = 0.0;
        nr_sync<NW>();
      }
      alpha_j += h[j];
      if (wave == 0) {
        const double eps = 2.220446049250313e-16;
        for (int i = lane; i <= j; i += 64) om_next[i] = eps;
      }
      force_next = !force_next;
      if (P.diag && tid == 0) atomicAdd(P.diag + 3, 1);
    }
    NR_STAMP(9);  // Lanczos: reorthogonalisation
    const double beta_j = !EARLY || reorthed ? sqrt(nb) : beta0;
    if (tid == 0) {
      alpha[j] = alpha_j;
      beta[j] = beta_j;
    }
    nsteps = j + 1;
    {  // next Lanczos vector (unused if this step's check ends the run), into the basis too
      const double inv = !EARLY || reorthed ? 1.0 / beta_j : inv0;
      double* qn = j + 1 < mcap ? Q + (int64_t)(j + 1) * k : nullptr;
      for (int c = tid; c < k; c += BS) {
        qprev[c] = q[c];
        const double v = w[c] * inv;
        q[c] = v;
        if (qn) qn[c] = v;
      }
    }
    beta_prev = beta_j;
    nr_sync<NW>();
    NR_STAMP(6);  // Lanczos: q update + barrier
    const bool last = (j + 1 == mcap);
    // Breakdown: beta_j at rounding level of the operator's norm, i.e. the
    // Krylov space is invariant to working precision (a Gram of low rank: the
    // start vector spans it after rank steps). The run ends here, its top Ritz
    // pair is an eigenpair (residual <= beta_j <= NR_LZ_TOL anorm). Going on
    // would divide rounding noise by beta_j: the next vectors carry O(1)
    // components of the converged ones, and once the omega recurrence skips a
    // reorthogonalisation they enter the tridiagonal as a second, unconverged
    // copy of the top pair (tests/test_gpu_spectra.py, the rank-3 blocks:
    // errors up to 0.2 in the summary profile before this rule).
    const bool broke = !(beta_j > NR_LZ_TOL * anorm);  // (also beta_j == 0 or NaN; uniform over the workgroup)
    if (j + 1 == next_check || last || broke) {
      if (wave == 0) {
        // the top eigenvalue to 1e-9 of the scale, enough for the residual
        // estimate, unless this check was predicted to end the run; to 2e-16
        // where the run may stop here (its Ritz pair is then the result)
        const bool full = flags[6] != 0;
        SturmBracket sb = sturm_init(alpha, beta, j + 1, lane, hint_theta, hint_r, h, ty);  // h, ty idle here
        sturm_passes(sb, j + 1, lane, h, ty, (full ? 2e-16 : 1e-9) * sb.scale);
        double theta = 0.5 * (sb.lo + sb.hi);
        NR_STAMP(13);  // Ritz check: the top eigenvalue (Sturm multisection)
        double resid = tri_top_resid(alpha, beta, j + 1, theta, beta_j, ty, lane);
        if (!full && (resid <= 1e3 * NR_LZ_TOL * fabs(theta) || last || broke) &&
            sb.hi - sb.lo > 2e-16 * sb.scale) {
          sturm_coeffs(alpha, beta, j + 1, lane, sb.inv, h, ty);  // ty held the residual's reciprocals
          sturm_passes(sb, j + 1, lane, h, ty, 2e-16 * sb.scale);
          theta = 0.5 * (sb.lo + sb.hi);
          resid = tri_top_resid(alpha, beta, j + 1, theta, beta_j, ty, lane);
        }
        NR_STAMP(14);  // Ritz check: the residual (backward recurrence)
        hint_theta = sb.lo;  // a lower bound of the top eigenvalue (the next check's warm start)
        hint_r = resid;
        if (lane == 0) {
          const double tol = NR_LZ_TOL * fabs(theta);
          const bool conv = resid <= tol;
          s_done = conv || last || broke;
          if (relax && resid <= 1e-7 * fabs(theta)) flags[5] = 1;
          // the Ritz vector's coefficients: inverse iteration (LU), once
          if (s_done) {
            NR_STAMP(7);
            // the Ritz coefficients by inverse iteration (the residual check's
            // backward recurrence is 2-4% faster but moved statistics by up to
            // 1.5e-10: profiles/r03/ritz_coefficients/)
            tri_eigenvector<BIG ? 1 : 8>(alpha, beta, j + 1, theta, ty, twork);
            NR_STAMP(12);  // Ritz coefficients (inverse iteration)
            L.h[0] = theta;  // for gv_out (h is idle once the run ends)
          }
          if (last && !conv && P.diag && tight) atomicAdd(P.diag, 1);  // step cap hit (a run at sqrt(eps) that gets here is run again)
          int step = 8;
          bool pred = false;
          if (prev_j > 0 && resid < prev_r && resid > 0.0) {
            const double lr = nr_log2_fast(resid);
            const double rate = (lr - nr_log2_fast(prev_r)) / (double)(j + 1 - prev_j);  // < 0
            const double need = ceil((nr_log2_fast(tol) - lr) / rate);
            step = need < 1.0 ? 1 : (need > 8.0 ? 8 : (int)need);
            pred = need <= 8.0;
          }
          // Still on fp64 matvecs: also check where the decay predicts the
          // residual's crossing of the fp32 threshold (the decay since the
          // previous check, or since step 0 at residual theta for the first),
          // so the relaxed phase starts near the crossing instead of at the
          // next convergence check (offline, tools/sim_lanczos_tiers.py: Gram
          // bytes per entry 226.8 -> 216.6, +0.25 checks). Neutral at round
          // 5's check cost (profiles/r06/ab_tiers/), C3 -1.0% with the
          // cheaper checks (profiles/r06/ab_cross/).
          if (relax && flags[5] == 0 && resid > 1e-7 * fabs(theta) && resid < fabs(theta)) {
            const double lr = nr_log2_fast(resid);
            const double rate = prev_j > 0 && resid < prev_r && resid > 0.0
                                    ? (lr - nr_log2_fast(prev_r)) / (double)(j + 1 - prev_j)
                                    : (lr - nr_log2_fast(fabs(theta))) / (double)(j + 1);
            const double cross = ceil((nr_log2_fast(1e-7 * fabs(theta)) - lr) / rate);
            if (cross >= 1.0 && cross < (double)step) {
              step = (int)cross;
              pred = false;  // not the predicted convergence: the coarse stage suffices
            }
          }
          flags[6] = pred;
          prev_j = j + 1;
          prev_r = resid;
          s_next_check = min(j + 1 + step, mcap);
        }
      }
      nr_sync<NW>();
      if (s_done) break;
      next_check = s_next_check;
      if (relax) *relax = flags[5] != 0;
      NR_STAMP(7);  // Lanczos: Ritz checks
    }
  }
  again = !tight && nsteps > kLongRun;
  if (again) {  // the long run starts again from q_0 (the basis' first column), with the tight bound
    tight = 1;
    nr_sync<NW>();  // (every thread has read s_done)
    if (tid == 0) {
      s_done = 0;
      s_reorth = 0;
      flags[5] = 0;
      flags[6] = 0;
    }
    if (relax) *relax = false;
    if (BF)  // twork (the packed matvec's partials) held the tridiagonal LU: zero again
      for (int i = tid; i < 5 * mmax; i += BS) twork[i] = 0.0;
    for (int c = tid; c < k; c += BS) {
      q[c] = Q[c];
      qprev[c] = 0.0;
    }
    if (tid == 0) omg[0] = 1.0;
    beta_prev = 0.0;
    anorm = 0.0;
    force_next = false;
    next_check = first_check;
    prev_j = 0;
    prev_r = hint_theta = hint_r = 0.0;
    nr_sync<NW>();
  }
  } while (again);
  NR_STAMP(7);
  if (tid == 0 && P.diag) {
    atomicAdd(P.diag + 1, 1);
    atomicAdd(P.diag + 2, nsteps);
  }
  // Ritz vector v = Q y, normalised. gv_out: also G v into L.gv from the
  // Lanczos relation G Q y = Q T y + w y_m = theta Q y + y_m w (w = beta_m
  // q_{m+1}, still in L.w), instead of one more fp64 pass over G. Rounding,
  // the relaxed fp32 steps and the projections a reorthogonalisation drops
  // perturb it by sum_j |y_j| |E_j|: the same terms the relaxed Krylov
  // argument already bounds for the Ritz vector, on coefficients y_j that are
  // at the residual's level once those steps start.
  double nv[1] = {0.0};
  const double theta_f = gv_out ? L.h[0] : 0.0;
  const double ym = gv_out ? ty[nsteps - 1] : 0.0;
  if constexpr (NW == 1) {  // one wave: 16 basis vectors' loads in flight per burst (ritz_vector_wave)
    ritz_vector_wave(Q, k, nsteps, ty, L.vv);
    for (int c = tid; c < k; c += BS) {
      const double s = L.vv[c];
      if (gv_out) L.gv[c] = theta_f * s + ym * w[c];
      nv[0] += s * s;
    }
  } else {
    for (int c = tid; c < k; c += BS) {
      // eight basis entries' loads in flight at a time (the same sum, in the
      // same order: one dependent global load per step otherwise)
      double s = 0.0;
      int i = 0;
      for (; i + 8 <= nsteps; i += 8) {
        double q8[8];
#pragma unroll
        for (int t = 0; t < 8; ++t) q8[t] = Q[(int64_t)(i + t) * k + c];
#pragma unroll
        for (int t = 0; t < 8; ++t) s += ty[i + t] * q8[t];
      }
      for (; i < nsteps; ++i) s += ty[i] * Q[(int64_t)i * k + c];
      L.vv[c] = s;
      if (gv_out) L.gv[c] = theta_f * s + ym * w[c];
      nv[0] += s * s;
    }
  }
  if (BF)  // twork (the packed matvec's partials) held the tridiagonal LU: zero again
    for (int i = tid; i < 5 * mmax; i += BS) twork[i] = 0.0;
  block_sums<1, NW>(nv, red);
  {
    const double inv = 1.0 / sqrt(nv[0]);
    for (int c = tid; c < k; c += BS) {
      L.vv[c] *= inv;
      if (gv_out) L.gv[c] *= inv;
    }
  }
  nr_sync<NW>();
  NR_STAMP(10);  // Ritz vector
}

// ---------------------------------------------------------------------------
// Scheme 1 (global scratch): G in the workgroup's scratch slot, full (both
// triangles) or packed symmetric; the Lanczos matvecs stream it from L2 /
// Infinity Cache. Any module size that fits the LDS vectors.
// The kernel's shape is profile_traits(K) (profile_plan.h), which the planner
// sizes the launch from. kb > 0 fixes the LDS layout at compile time for
// modules of at most kb nodes (every carve-out an immediate offset; frees the
// SGPRs runtime offsets cost). Only the Gram source it names is compiled in:
// no matrix-core or dual Gram in the table kernel, no table fill in the
// others, which keeps the register demand down (spills at the 168-VGPR budget).
// ---------------------------------------------------------------------------
template <ProfileKernel K>
__device__ __forceinline__ void profile_body(const ProfileParams& P) {
  constexpr ProfileTraits T = profile_traits(K);
  constexpr int NW = T.waves, BS = NW * 64, KB = T.kb, MB = T.mb;
  constexpr bool PACKED = T.storage == GramStorage::Packed;
  constexpr bool TABLE = T.source == GramSource::Table, G64 = T.source == GramSource::SuperTile64;
  constexpr bool HD = TABLE;  // the packed diagonal stored halved (the notes above pk_store_tile)
  NR_STAMP_INIT();
  uint64_t t_mark = P.stamps && threadIdx.x == 0 ? nr_clock() : 0;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __shared__ int s_flags[8];
  const int kmax = KB > 0 ? KB : (P.kvec > 0 ? P.kvec : P.k_max);  // LDS vector length
  const int mmax = KB > 0 ? MB : P.m_max;
  const int S = (int)P.n_samples;
  // The per-wave matvec partials. Packed: in LDS, one array per wave, which
  // also serves as the Ritz checks' work area (twork, 5 mmax doubles) between
  // matvecs. Full Gram: in the slot's scratch behind the basis; the
  // workgroup's barriers order them (one CU, one vector L1).
  const int64_t n_part = PACKED ? packed_part_doubles(NW, kmax, mmax) : (int64_t)NW * kmax;
  double* G = P.scratch + (int64_t)blockIdx.x * P.scratch_stride;  // Gram
  const int ld = P.ld;
  double* Q = G + P.gram_doubles;                                  // Lanczos basis
  // FullVectorsInScratch: every vector in the slot's scratch behind the partials
  const bool vglob = !PACKED && P.vec_global;
  double* part = nullptr;
  const LzLds L = vglob ? carve_split<NW>(smem, Q + P.basis_doubles + (int64_t)NW * kmax, kmax, mmax)
                        : carve_lds<NW>(smem, kmax, mmax, PACKED ? n_part : 0, &part, PACKED);
  const int tid = threadIdx.x;
  // fp32 copy of the packed Gram for the relaxed Lanczos steps (0: off)
  float* G32 = PACKED && P.g32_off > 0 ? reinterpret_cast<float*>(G + P.g32_off) : nullptr;
  if (!PACKED) part = Q + P.basis_doubles;
  // modules of more than kmax nodes (dual by construction, plan_profile):
  // x_c.u, column means, sums of squares, contributions and the index set in
  // the slot's scratch
  double* gnode = Q + P.basis_doubles + (PACKED ? 0 : n_part);
  const double* __restrict__ X = P.data;
  const double Sd = (double)S;

  if (PACKED) {  // the matvec's partial arrays start zero (packed_matvec keeps them so)
    for (int i = tid; i < n_part; i += BS) part[i] = 0.0;
    __syncthreads();
  }
  int m, k;
  int64_t p_local, off;
  uint32_t* idx_p = L.idx;
  while (next_item<NW>(P, L, s_flags, m, p_local, off, k, kmax,
                       reinterpret_cast<uint32_t*>(gnode + 4 * (int64_t)P.k_max), &idx_p)) {
    NR_STAMP(0);  // queue + index derivation
    LzLds Li = L;  // this item's view: per-node arrays in scratch when k > kmax
    Li.idx = idx_p;
    if (k > kmax) {
      Li.gv = gnode;
      Li.colm = gnode + P.k_max;
      Li.q = gnode + 2 * (int64_t)P.k_max;
      Li.w = gnode + 3 * (int64_t)P.k_max;
    }
    const bool dual = !TABLE && k > S;
    const int n = dual ? S : k;  // Lanczos dimension
    const int kc = n + 1;
    double g1[1] = {0.0};
    int bad = 0;
    if constexpr (TABLE) {
      // Gram table: the item's network statistics from one 32-byte gather per
      // pair, which also carries G_ij -- the packed Gram is filled here (into
      // a zeroed region: padding and the diagonal blocks' upper parts stay 0)
      // and the matrix-core Gram is skipped. The per-node arrays live in the
      // Lanczos vectors' LDS, idle until the Lanczos phase.
      const GramOut go{G, G32, kc, Sd};
      // The fill below writes every lower-triangle entry over kc = k + 1
      // (pairs, diagonal, ones column); zero only what it never writes: the
      // diagonal blocks' upper parts, which include the last group's columns
      // >= kc (its rows all lie in its diagonal block). (Round 3: zeroing the
      // whole packed region first doubled the item's Gram stores.)
      const int ngr = pk_groups(kc);
      for (int i = tid; i < ngr * 256; i += BS) {
        const int g = i >> 8, r = 16 * g + ((i >> 4) & 15), c = 16 * g + (i & 15);
        if (r < c && r < kc) go.put(pk_at(r, c, kc), 0.0);
      }
      __syncthreads();
      const NetLds NL = carve_net_over<NW>(L.q, L.red, L.idx, kmax);
      net_item<NW, NR_TABLE_PIPE, true, true, NR_TABLE_U, 2>(P.net, m, p_local, off, k, NL, go, g1, &bad);
      for (int64_t i = tid; i < n_part; i += BS) part[i] = 0.0;  // the per-node arrays overlapped them
    } else if constexpr (G64) {
      // ---- Gram [X 1]^T [X 1] on the matrix cores (S x S dual when k > S) ----
      if (dual)
        gram_mfma128<NW, true, kGramDualRows>(X, S, Li.idx, k, P.ones_off, G, G32, g1[0], bad);
      else
        gram_mfma64<NW, false>(X, S, L.idx, k, P.ones_off, G, G32, g1[0], bad);
    } else {
      if (dual)
        gram_mfma_dual<NW, PACKED>(X, S, Li.idx, k, G, G32, ld, g1[0], bad);
      else
        gram_mfma<NW, PACKED>(X, S, L.idx, k, P.ones_off, G, G32, ld, g1[0], bad);
    }
    if (bad) atomicOr(&s_flags[1], 1);
#ifdef NR_GRAM_ONLY
    // diagnostic build only (make EXTRA=-DNR_GRAM_ONLY=1 OUT=...): the Gram
    // phase alone, for its counters; every item then takes the non-finite
    // path (NA statistics), so nothing after the Gram runs
    if (tid == 0) atomicOr(&s_flags[1], 1);
#endif
    block_sums<1, NW>(g1, L.red);  // barriers also publish G to the whole workgroup
    NR_STAMP(1);  // Gram
    if (s_flags[1] == 0) {
      if (!dual)
        for (int c = tid; c < k; c += BS)
          L.colm[c] = (PACKED ? G[pk_at(k, c, kc)] : G[k + (int64_t)c * ld]) / Sd;
      bool relax = false;
      auto mv = [&](const double* x, double* out, const double* y) -> double {
        if (!PACKED) return matvec(G, ld, n, x, out, part, kmax, y, L.red);
        return relax ? packed_matvec<NW, true, false, HD>(G32, kc, n, x, out, part, kmax, y, L.red)
                     : packed_matvec<NW, false, false, HD>(G, kc, n, x, out, part, kmax, y, L.red);
      };
      const bool q_given = PACKED && start_column<NW, HD>(G, G32, kc, n, L.q, L.w, part, kmax, L.red);
      NR_STAMP(8);  // start column
      const bool gv_rel = !dual;
      lanczos_ritz<NW, PACKED, decltype(mv), G64>(P, n, L, s_flags, Q, mv, t_mark, G32 ? &relax : nullptr,
                                                         q_given, gv_rel);
      relax = false;  // node contributions: the fp64 Gram
      if (!TABLE && dual) {
        profile_contrib_dual<NW>(P, k, m, Li, X, S, g1[0]);
      } else {
        profile_contrib<NW>(P, k, m, L, X, S, g1[0], mv, [&](int c) {
          return PACKED ? (HD ? 2.0 : 1.0) * G[pk_col(c, kc)] : G[c + (int64_t)c * ld];  // (HD: stored halved)
        }, gv_rel);
      }
      NR_STAMP(11);  // node contributions
    } else {
      profile_nonfinite<NW>(P, k, m, S, Li);
    }
    profile_stats<NW>(P, k, m, off, p_local, Li);
    NR_STAMP(5);  // Ritz vector, contributions, statistics
  }
  NR_STAMP_FLUSH();
}

// A kernel's workgroup size and waves per SIMD, from its description.
#define NR_PROFILE_BOUNDS(K) __launch_bounds__(64 * profile_traits(K).waves, profile_traits(K).launch_occ)
static_assert(profile_traits(ProfileKernel::FullGram).waves == NR_WAVES, "matvec (the full Gram) runs on NR_WAVES waves");

__global__ void NR_PROFILE_BOUNDS(ProfileKernel::FullGram)
module_profile_kernel(ProfileParams P) {
  profile_body<ProfileKernel::FullGram>(P);
}

// Packed Gram in the lean 4-wave structure, compile-time LDS layout (KB > 0)
// or runtime. (KB and OCC restate the description: the symbols profiles name.)
template <int KB, int OCC>
__global__ void __launch_bounds__(NR_BS, OCC)
module_profile_packed4_kernel(ProfileParams P) {
  constexpr ProfileKernel K = KB > 0 ? ProfileKernel::PackedFixed : ProfileKernel::PackedRuntime;
  static_assert(profile_traits(K).kb == KB && profile_traits(K).launch_occ == OCC, "not profile_traits(K)");
  profile_body<K>(P);
}

// Packed modules beyond the compile-time layout (runtime LDS layout, one
// workgroup per CU): the 64 x 64 super-tile Gram at one wave per SIMD. (The
// 128 x 128 LDS-staged workgroup tile measured 8% slower on C5 and was
// removed, profiles/r04/ab7/.)
__global__ void NR_PROFILE_BOUNDS(ProfileKernel::PackedBig)
module_profile_big_kernel(ProfileParams P) {
  profile_body<ProfileKernel::PackedBig>(P);
}

// The Gram-table launches of the packed class (every item from the table, k <= S).
// (An LDS prefix of the item's Gram and a CU-resident one-workgroup-per-CU
// version measured equal and 1.8x slower: profiles/r04/ab4/, r04/resident/.)
__global__ void NR_PROFILE_BOUNDS(ProfileKernel::Table)
module_profile_table_kernel(ProfileParams P) {
  profile_body<ProfileKernel::Table>(P);
}

// The small class: Lanczos dimension <= kSmallDim (MB = KB = kSmallDim), NW
// waves per item; three waves per SIMD (HIP's second launch bound is waves per
// execution unit: the 168-VGPR budget of the packed kernel), as many items
// per CU as the LDS holds. (Computing the items' network statistics in the
// same workgroups measured 1.6x slower on C2, profiles/r04/ab2/.)
template <int NW>
__global__ void NR_PROFILE_BOUNDS(ProfileKernel::Small)
module_profile_small_kernel(ProfileParams P) {
  static_assert(NW == profile_traits(ProfileKernel::Small).waves, "not the kernel profile_traits describes");
  profile_body<ProfileKernel::Small>(P);
}

// ---------------------------------------------------------------------------
// The wave class (round 5): Lanczos dimension n = min(k, S) <= kWaveDim, one
// wave per item, and the item's whole Gram [X 1]^T [X 1] (side n + 1 <= 112,
// seven 16-row blocks) kept in the wave's registers as its 28 lower 16 x 16
// MFMA accumulator tiles (tile (I, J), I >= J, at I (I + 1) / 2 + J; a
// diagonal tile holds both of its triangles). The Gram is never written to
// memory, and every Lanczos matvec reads it from registers: the small class
// streamed a ~41 KB packed Gram per matvec from the cache hierarchy, about 40
// times per item, latency-bound (57% of a C2 item, profiles/r04/stamps/
// stamps_C2.txt). Lane (i16, kk) = (lane & 15, lane >> 4) holds
// G[16 I + kk + 4 r][16 J + i16], r = 0..3 (f64 MFMA C/D map). 224 registers
// of Gram put one wave on each SIMD: four items per CU, each on its own
// matrix core.
// ---------------------------------------------------------------------------
constexpr int kWaveTiles = kWaveBlocks * (kWaveBlocks + 1) / 2;
static_assert(kWaveDim + 1 <= kWaveVec, "the wave class's Gram side must fit its tiles");

__device__ __forceinline__ constexpr int wave_tile(int I, int J) { return I * (I + 1) / 2 + J; }

// A Gram value for the VALU. (Reading the tiles through an inline-asm AGPR
// operand kept them out of VGPRs too, but hides the MFMA -> read hazard from
// the compiler; with one MFMA site the allocator keeps them in AGPRs itself,
// 64 B/lane of spill outside the matvec.)
__device__ __forceinline__ double tile_val(const nr_f64x4& t, int r) { return t[r]; }

// The Gram on the matrix cores, straight into the tiles. Primal (k <= S): the
// vectors are the module's columns (block position c < k: column idx[c];
// c == k: the data block's ones column; beyond: its zero column), contracted
// over the S samples, each lane feeding 4 consecutive samples of its column
// per 16-sample step (two 16-byte loads), as gram_mfma. Dual (k > S): the
// vectors are the samples (position s < S: row s of X; s == S: the ones row;
// beyond: zero), contracted over the k module nodes, each lane feeding nodes
// c0 + 4 kk + q of a 16-node step (16 lanes read 16 consecutive samples of a
// column), as gram_mfma_dual. One operand register per block serves as A for
// the block's tile row and as B for its tile column; the next step's operands
// are in flight during this step's MFMAs. One MFMA site for both shapes (two
// sites put the tiles in VGPRs and spilled). nb: blocks of the side n + 1.
__device__ __forceinline__ void gram_wave(const double* __restrict__ X, int S, const uint32_t* idx, int k,
                                          int64_t ones_off, int nb, bool dual, nr_f64x4 (&T)[kWaveTiles]) {
  const int lane = threadIdx.x & 63;
  const int i16 = lane & 15, kk = lane >> 4;
#pragma unroll
  for (int t = 0; t < kWaveTiles; ++t) T[t] = nr_f64x4{0.0, 0.0, 0.0, 0.0};
  // Every operand is a range-checked buffer load (an out-of-range offset
  // reads 0, no branch), so the compiler counts the loads in flight exactly
  // and waits for this step's operands only, not the next step's too.
  const auto rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)X, (short)0, (int)((ones_off + 2 * (int64_t)S) * 8),
                                                      0x00020000);
  constexpr int OOR = (int)0x80000000;
  int col[kWaveBlocks];  // primal: the lane's column of each block (element offset)
#pragma unroll
  for (int I = 0; I < kWaveBlocks; ++I) {
    const int c = 16 * I + i16;
    col[I] = c < k ? (int)idx[c] * S : (int)(c == k ? ones_off : ones_off + S);
  }
  auto ld = [&](int st, double (&v)[kWaveBlocks][4]) {
    if (!dual) {
      const int s0 = 16 * st + 4 * kk;
#pragma unroll
      for (int I = 0; I < kWaveBlocks; ++I)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int vo = I < nb && s0 + q < S ? (col[I] + s0 + q) * 8 : OOR;
          v[I][q] = __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(rsrc, vo, 0, 0));
        }
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int c = 16 * st + 4 * kk + q;
        const int base = c < k ? (int)idx[c] * S : 0;
#pragma unroll
        for (int I = 0; I < kWaveBlocks; ++I) {
          const int s = 16 * I + i16;
          const int vo = I < nb && c < k && s < S ? (base + s) * 8 : OOR;
          const double x = __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(rsrc, vo, 0, 0));
          v[I][q] = s == S && c < k ? 1.0 : x;  // the ones row
        }
      }
    }
  };
  const int nsteps = dual ? (k + 15) / 16 : (S + 15) / 16;
  double cur[kWaveBlocks][4], nxt[kWaveBlocks][4];
  ld(0, cur);
  for (int st = 0; st < nsteps; ++st) {
    if (st + 1 < nsteps) ld(st + 1, nxt);
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int I = 0; I < kWaveBlocks; ++I) {
        if (I >= nb) break;
#pragma unroll
        for (int J = 0; J <= I; ++J)
          T[wave_tile(I, J)] =
              __builtin_amdgcn_mfma_f64_16x16x4f64(cur[I][q], cur[J][q], T[wave_tile(I, J)], 0, 0, 0);
      }
#pragma unroll
    for (int I = 0; I < kWaveBlocks; ++I)
#pragma unroll
      for (int q = 0; q < 4; ++q) cur[I][q] = nxt[I][q];
  }
}

__device__ __forceinline__ double sel4(const nr_f64x4& t, int r) {
  const double a = tile_val(t, 0), b = tile_val(t, 1), c = tile_val(t, 2), d = tile_val(t, 3);
  return r == 0 ? a : (r == 1 ? b : (r == 2 ? c : d));
}

// What the rest of the item needs from the tiles: the diagonal G_cc (c < n,
// into dg), the non-finite flag (a non-finite diagonal entry, as the other
// Gram schemes), the column means (primal: row k of G is the column sums),
// and the per-lane part of 1'G1 over the X block (primal: the sum of G over
// c, c' < k; dual: |X 1|^2 from the ones row).
__device__ __forceinline__ void gram_wave_epilogue(const nr_f64x4 (&T)[kWaveTiles], int nb, int n, int k, int S,
                                                   bool dual, double* dg, double* colm, double& g1, int& bad) {
  const int lane = threadIdx.x & 63;
  const int i16 = lane & 15, kk = lane >> 4;
  // the lane's entry of a diagonal tile's diagonal: row kk + 4 r == column i16
  const bool has_diag = i16 >= kk && ((i16 - kk) & 3) == 0;
  const int rd = (i16 - kk) >> 2;
  // the ones row (index n: k primal, S dual): tile row n >> 4, the lanes whose
  // row kk + 4 r is n & 15
  const int In = n >> 4, rn = (n & 15) - kk;
  const bool has_ones = rn >= 0 && (rn & 3) == 0;
#pragma unroll
  for (int I = 0; I < kWaveBlocks; ++I) {
    if (I >= nb) break;
    if (has_diag && 16 * I + i16 < n) {
      const double val = sel4(T[wave_tile(I, I)], rd);
      dg[16 * I + i16] = val;
      bad |= (int)!isfinite(val);
    }
    if (I == In && has_ones) {
#pragma unroll
      for (int J = 0; J <= I; ++J) {
        const int gj = 16 * J + i16;
        const double val = sel4(T[wave_tile(I, J)], rn >> 2);
        if (gj < n) {
          if (dual)
            g1 += val * val;
          else
            colm[gj] = val / (double)S;
        }
      }
    }
    if (!dual) {  // 1'G1 over the k x k block: tiles below the diagonal count twice
#pragma unroll
      for (int J = 0; J <= I; ++J) {
        const double wgt = I == J ? 1.0 : 2.0;
        const int gj = 16 * J + i16;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int gi = 16 * I + kk + 4 * r;
          g1 += (gi < k && gj < k) ? wgt * tile_val(T[wave_tile(I, J)], r) : 0.0;
        }
      }
    }
  }
}

// out = G x over the leading n x n block (x zero at n and beyond; rows >= n
// not written), from the registers. Lower tiles (I >= J, diagonal tiles
// whole): lane-local sums over the tile's columns, then over the 16 column
// lanes (rg_row_reduce) into ylo; mirrored part of the tiles below the
// diagonal (I > J): lane-local sums over the tile rows, then over the four
// row groups (two permlane swaps) into yup; out = ylo + yup. A fixed order
// throughout: bitwise reproducible. Returns sum_r y_r out_r if y (every lane).
// SQ: out_r = sum_c G_rc^2 over c < n instead (start column norms; x unused).
constexpr int kRowGroup = 3;  // tile rows per branch of wave_matvec
template <bool SQ>
__device__ __forceinline__ double wave_matvec(const nr_f64x4 (&T)[kWaveTiles], int nb, int n, const double* x,
                                              double* out, const double* y, double* ylo, double* yup) {
  const int lane = threadIdx.x & 63;
  const int i16 = lane & 15, kk = lane >> 4;
  double xc[kWaveBlocks], au[kWaveBlocks];
#pragma unroll
  for (int I = 0; I < kWaveBlocks; ++I) {
    au[I] = 0.0;
    xc[I] = 0.0;
    if (I < nb + kRowGroup - 1) xc[I] = SQ ? (16 * I + i16 < n ? 1.0 : 0.0) : x[16 * I + i16];
  }
  const int rg = 4 * (((lane >> 3) & 1) * 2 + ((lane >> 2) & 1));  // row offset of rg_row_reduce's group
  // one pass over the tiles, each value read once: tile row I's lower sums
  // (reduced and stored when the row is done) and, below the diagonal, the
  // mirrored sums of the tile columns J < I
  // tile rows in groups of three, one branch on nb per group: the rows'
  // reductions interleave (their DPP wait states filled by each other). A row
  // of a group past nb has zero tiles and x, and writes ylo rows >= n only.
  // (C2 shape per 256 permutations: one row per branch 1.860 ms, groups of 2
  // 1.822, 3 1.797, 4 1.842; no branch at all spilled inside the Lanczos
  // loop. profiles/r05/rowg/)
#pragma unroll
  for (int I0 = 0; I0 < kWaveBlocks; I0 += kRowGroup) {
    if (I0 >= nb) break;
#pragma unroll
    for (int I = I0; I < I0 + kRowGroup && I < kWaveBlocks; ++I) {
      double xri[4], a[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int r = 0; r < 4; ++r) xri[r] = SQ ? (16 * I + kk + 4 * r < n ? 1.0 : 0.0) : x[16 * I + kk + 4 * r];
#pragma unroll
      for (int J = 0; J <= I; ++J)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const double g = tile_val(T[wave_tile(I, J)], r);
          const double gg = SQ ? g * g : g;
          a[r] = fma(gg, xc[J], a[r]);
          if (J < I) au[J] = fma(gg, xri[r], au[J]);
        }
      const double v = rg_row_reduce(a, lane);
      if ((lane & 3) == 0) ylo[16 * I + kk + rg] = v;
    }
  }
  // (no branch: a column past nb sums zeros into yup rows >= n; the seven
  // swap chains interleave)
#pragma unroll
  for (int J = 0; J < kWaveBlocks; ++J) {
    double a = nr_swap16_sum(au[J], au[J]);
    a = nr_swap32_sum(a, a);
    if (kk == 0) yup[16 * J + i16] = a;
  }
  nr_sync<1>();  // one wave: orders the LDS writes above before the reads below
  double d = 0.0;
  for (int c = lane; c < n; c += 64) {
    const double s = ylo[c] + yup[c];
    out[c] = s;
    if (y) d += y[c] * s;
  }
  return y ? nr_wave_sum(d) : 0.0;
}

// Lanczos start vector q = G e_c* for the column c* of largest norm (ties to
// the smaller index), as start_column; norms from the fp64 tiles. Returns
// false (q untouched) if every column is zero. e: kWaveVec doubles of LDS.
__device__ __forceinline__ bool wave_start_column(const nr_f64x4 (&T)[kWaveTiles], int nb, int n, double* q,
                                                  double* cn, double* e, double* ylo, double* yup) {
  const int lane = threadIdx.x & 63;
  wave_matvec<true>(T, nb, n, nullptr, cn, nullptr, ylo, yup);
  nr_sync<1>();
  double best = -1.0;
  int bi = 0x7fffffff;
  for (int r = lane; r < n; r += 64) {
    const double v = cn[r];
    if (v > best) {
      best = v;
      bi = r;
    }
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const double ov = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (ov > best || (ov == best && oi < bi)) {
      best = ov;
      bi = oi;
    }
  }
  const bool ok = best > 0.0 && bi < n;
  if (ok) {
    for (int c = lane; c < kWaveVec; c += 64) e[c] = c == bi ? 1.0 : 0.0;
    nr_sync<1>();
    wave_matvec<false>(T, nb, n, e, q, nullptr, ylo, yup);  // exact: one nonzero per row sum
  }
  nr_sync<1>();
  return ok;
}

__global__ void NR_PROFILE_BOUNDS(ProfileKernel::Wave)
module_profile_wave_kernel(ProfileParams P) {
  constexpr int KB = kWaveVec, MB = kWaveVec;
  NR_STAMP_INIT();
  uint64_t t_mark = P.stamps && threadIdx.x == 0 ? nr_clock() : 0;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __shared__ int s_flags[8];
  const int lane = threadIdx.x;
  const int S = (int)P.n_samples;
  // the slot's scratch: the Lanczos basis (no Gram in memory), then the
  // per-node arrays and index set of modules longer than the LDS vectors
  double* Q = P.scratch + (int64_t)blockIdx.x * P.scratch_stride;
  double* ext;
  const LzLds L = carve_lds<1>(smem, KB, MB, 3 * KB, &ext);
  double* ylo = ext;
  double* yup = ext + KB;
  double* dg = ext + 2 * KB;
  double* gnode = Q + P.basis_doubles;
  const double* __restrict__ X = P.data;
  int m, k;
  int64_t p_local, off;
  uint32_t* idx_p = L.idx;
  while (next_item<1>(P, L, s_flags, m, p_local, off, k, KB,
                      reinterpret_cast<uint32_t*>(gnode + 4 * (int64_t)P.k_max), &idx_p)) {
    NR_STAMP(0);
    LzLds Li = L;
    Li.idx = idx_p;
    if (k > KB) {
      Li.gv = gnode;
      Li.colm = gnode + P.k_max;
      Li.q = gnode + 2 * (int64_t)P.k_max;
      Li.w = gnode + 3 * (int64_t)P.k_max;
    }
    const bool dual = k > S;
    const int n = dual ? S : k;  // Lanczos dimension
    const int nb = (n + 16) / 16;  // blocks of the Gram's side n + 1
    // the matvec operands read x up to the last block: zero beyond n (the
    // previous item's per-node arrays may have left values there)
    for (int c = n + lane; c < KB; c += 64) {
      L.q[c] = 0.0;
      L.vv[c] = 0.0;
    }
    nr_f64x4 T[kWaveTiles];
    gram_wave(X, S, Li.idx, k, P.ones_off, nb, dual, T);
    double g1 = 0.0;
    int bad = 0;
    gram_wave_epilogue(T, nb, n, k, S, dual, dg, L.colm, g1, bad);
    g1 = nr_wave_sum(g1);
    bool nonfinite = __ballot(bad != 0) != 0;
#ifdef NR_GRAM_ONLY
    nonfinite = true;  // diagnostic build only: the Gram phase alone (see profile_body)
#endif
    nr_sync<1>();  // dg, colm published; the zeroed vector tails too
    NR_STAMP(1);
    if (!nonfinite) {
      auto mv = [&](const double* x, double* out, const double* y) -> double {
        return wave_matvec<false>(T, nb, n, x, out, y, ylo, yup);
      };
      const bool q_given = wave_start_column(T, nb, n, L.q, L.w, L.vv, ylo, yup);
      NR_STAMP(8);
      lanczos_ritz<1, false>(P, n, L, s_flags, Q, mv, t_mark, nullptr, q_given, !dual);
      if (dual) {
        profile_contrib_dual<1>(P, k, m, Li, X, S, g1);
      } else {
        profile_contrib<1>(P, k, m, L, X, S, g1, mv, [&](int c) { return dg[c]; }, true);
      }
      NR_STAMP(11);
    } else {
      profile_nonfinite<1>(P, k, m, S, Li);
    }
    profile_stats<1>(P, k, m, off, p_local, Li);
    NR_STAMP(5);
  }
  NR_STAMP_FLUSH();
}

// ---------------------------------------------------------------------------
// Support kernels
// ---------------------------------------------------------------------------

// {corr, net} interleave (one 16-byte element per (i, j)).
// Big-endian (XDR) doubles of an R serialisation stream into native ones:
// into one half of the {corr, net} pairs (half 0 / 1) or a plain array.
__global__ void xdr_pairs_kernel(const unsigned long long* __restrict__ raw, double2* __restrict__ pairs,
                                 int64_t n, int half) {
  double* dst = reinterpret_cast<double*>(pairs) + half;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    dst[2 * i] = __longlong_as_double((long long)__builtin_bswap64(raw[i]));
}

__global__ void xdr_plain_kernel(const unsigned long long* __restrict__ raw, double* __restrict__ out, int64_t n) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    out[i] = __longlong_as_double((long long)__builtin_bswap64(raw[i]));
}

__global__ void interleave_kernel(const double* __restrict__ corr, const double* __restrict__ net,
                                  double2* __restrict__ out, int64_t n_elem) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n_elem;
       i += (int64_t)gridDim.x * blockDim.x)
    out[i] = make_double2(corr[i], net[i]);
}

// Gram table of the resident data block: gram[i + j n] = x_i . x_j (fp64
// matrix cores, the super-tile scheme of gram_mfma over the whole matrix, one
// 32 x 32 super-tile per wave; columns past n read the zero column n + 1).
// Computed once per dataset (2 S n^2 flops) for the Gram-table items.
__global__ void __launch_bounds__(256)
gram_full_kernel(const double* __restrict__ X, int S, int64_t n, double* __restrict__ gram) {
  const int lane = threadIdx.x & 63;
  const int i16 = lane & 15, kk = lane >> 4;
  const int64_t T = (n + 31) / 32;
  const int full = S / 16 * 16;
  const int64_t zero_col = (n + 1) * (int64_t)S;
  for (int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); t < T * T; t += (int64_t)gridDim.x * 4) {
    const int64_t I = t % T, J = t / T;
    const double* col[4];
#pragma unroll
    for (int o = 0; o < 4; ++o) {
      const int64_t c = (o < 2 ? I : J) * 32 + (o & 1) * 16 + i16;
      col[o] = X + (c < n ? c * S : zero_col) + 4 * kk;
    }
    nr_f64x4 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b) acc[a][b] = nr_f64x4{0.0, 0.0, 0.0, 0.0};
    double v[4][4];
    for (int s0 = 0; s0 < S; s0 += 16) {
#pragma unroll
      for (int o = 0; o < 4; ++o) {
        if (s0 < full) {
          double2 p0, p1;
          __builtin_memcpy(&p0, col[o] + s0, sizeof(double2));
          __builtin_memcpy(&p1, col[o] + s0 + 2, sizeof(double2));
          v[o][0] = p0.x;
          v[o][1] = p0.y;
          v[o][2] = p1.x;
          v[o][3] = p1.y;
        } else {  // the last, partial step
#pragma unroll
          for (int q = 0; q < 4; ++q) v[o][q] = s0 + 4 * kk + q < S ? col[o][s0 + q] : 0.0;
        }
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(v[0][q], v[2][q], acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(v[0][q], v[3][q], acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(v[1][q], v[2][q], acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(v[1][q], v[3][q], acc[1][1], 0, 0, 0);
      }
    }
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          // D[row = (lane>>4) + 4r][col = lane & 15] (f64 MFMA C/D map), as gram_mfma
          const int64_t gi = I * 32 + 16 * a + kk + 4 * r;
          const int64_t gj = J * 32 + 16 * b + i16;
          if (gi < n && gj < n) gram[gi + gj * n] = acc[a][b][r];
        }
  }
}

// colsum[j] = sum over the S rows of column j (one wave per column).
__global__ void colsum_kernel(const double* __restrict__ X, int S, int64_t n, double* __restrict__ colsum) {
  const int lane = threadIdx.x & 63;
  for (int64_t c = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); c < n;
       c += (int64_t)gridDim.x * (blockDim.x >> 6)) {
    double a = 0.0;
    for (int s = lane; s < S; s += 64) a += X[c * S + s];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
    if (lane == 0) colsum[c] = a;
  }
}

// {corr, net} + gram -> the table layout {corr, net}, {gram, net^T} per
// element, 32 x 32 tiles (net^T staged in LDS so both reads are coalesced).
__global__ void __launch_bounds__(256)
widen_pairs_kernel(const double2* __restrict__ in, const double* __restrict__ gram, double2* __restrict__ out,
                   int64_t n, int symmetric) {
  __shared__ double t[32][33];
  const int64_t r0 = (int64_t)blockIdx.x * 32, c0 = (int64_t)blockIdx.y * 32;
  const int i = threadIdx.x & 31;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int j = (threadIdx.x >> 5) + 8 * q;
    // t[j][i] = net(c0 + j, r0 + i)... staged as t[jj][ii] = in[(c0 + ii) + (r0 + jj) n].y
    if (!symmetric && c0 + i < n && r0 + j < n) t[j][i] = in[(c0 + i) + (r0 + j) * n].y;
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int j = (threadIdx.x >> 5) + 8 * q;
    const int64_t r = r0 + i, c = c0 + j;
    if (r < n && c < n) {
      const int64_t e = r + c * n;
      const double2 p = in[e];
      out[2 * e] = p;
      out[2 * e + 1] = make_double2(gram[e], symmetric ? p.y : t[i][j]);   // net(c, r)
    }
  }
}

// Exact symmetry check of the interleaved matrix via 32x32 LDS tiles: block
// (I, J), J >= I, stages A(J, I) in LDS and compares it with A(I, J); both
// reads are coalesced along rows. The same pass is CheckFinite
// (src/checkFinite.cpp:21-28) for both matrices of the upload, so the
// reference's separate full scans (R/check-user-input.R:796-799) cost no extra
// HBM traffic: every element is read here exactly once (diagonal tiles twice).
// flags: bit 0 asymmetric, bit 1 corr non-finite, bit 2 net non-finite.
__global__ void symmetry_kernel(const double2* __restrict__ a, int64_t n, int* flags) {
  __shared__ double2 tile[32][33];
  const int64_t bi = (int64_t)blockIdx.y * 32, bj = (int64_t)blockIdx.x * 32;
  if (bj < bi) return;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 256 threads: 32 x 8
  int bad = 0;
  for (int r = ty; r < 32; r += 8) {
    const int64_t row = bj + tx, col = bi + r;               // tile[r][c] = A(bj + c, bi + r)
    const double2 v = (row < n && col < n) ? a[row + col * n] : make_double2(0.0, 0.0);
    bad |= (isfinite(v.x) ? 0 : 2) | (isfinite(v.y) ? 0 : 4);
    tile[r][tx] = v;
  }
  __syncthreads();
  for (int r = ty; r < 32; r += 8) {
    const int64_t row = bi + tx, col = bj + r;               // A(bi + c, bj + r) vs tile[c][r]
    if (row < n && col < n) {
      const double2 x = a[row + col * n];
      const double2 t = tile[tx][r];
      bad |= (x.x != t.x) | (x.y != t.y);
      bad |= (isfinite(x.x) ? 0 : 2) | (isfinite(x.y) ? 0 : 4);
    }
  }
  if (bad) atomicOr(flags, bad);
}

// Scale (src/scale.cpp:14-25): one wave per column; arma mean + corrected
// two-pass variance with n-1 normalisation.
__global__ void scale_kernel(const double* __restrict__ in, double* __restrict__ out, int64_t S,
                             int64_t N) {
  const int lane = threadIdx.x & 63;
  const int64_t col = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (col >= N) return;
  const double* x = in + col * S;
  double s = 0.0;
  for (int64_t r = lane; r < S; r += 64) s += x[r];
  s = wave_sum(s);
  const double mean = s / (double)S;
  double a2 = 0.0, a3 = 0.0;
  for (int64_t r = lane; r < S; r += 64) {
    const double t = mean - x[r];
    a2 += t * t;
    a3 += t;
  }
  a2 = wave_sum(a2);
  a3 = wave_sum(a3);
  const double var = (a2 - a3 * a3 / (double)S) / (double)(S - 1);
  const double sd = sqrt(var);
  double* o = out + col * S;
  for (int64_t r = lane; r < S; r += 64) o[r] = (x[r] - mean) / sd;
}

__global__ void finite_kernel(const double* __restrict__ a, int64_t n, int* nonfinite) {
  int bad = 0;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x)
    bad |= !isfinite(a[i]);
  if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(nonfinite, 1);
}

// Exported index sets of permutations (nr_export_indices).
__global__ void export_indices_kernel(IndexSource src, int64_t n_nodes_total, int32_t* out,
                                      int64_t n_perm) {
  const int64_t p = blockIdx.y;
  if (p >= n_perm) return;
  nr_prp_key key;
  if (src.mode == NR_IDX_PRP) key = nr_prp_make_key(src.seed, (uint64_t)(src.perm_base + p), src.n_null);
  for (int64_t c = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; c < n_nodes_total;
       c += (int64_t)gridDim.x * blockDim.x)
    out[p * n_nodes_total + c] = (int32_t)node_index(src, key, p, c);
}

// ---------------------------------------------------------------------------
// Launchers
// ---------------------------------------------------------------------------
// Four waves per item unless their per-wave weighted-degree copies would not
// fit the LDS (modules of more than ~1,900 nodes): then two.
int net_kernel_waves(int k_max) { return net_lds_bytes(4, k_max) <= kLdsBudget ? 4 : 2; }

bool net_kernel_big(int k_max) { return net_lds_bytes(2, k_max) > kLdsBudget; }

size_t net_kernel_lds(int k_max) {
  return net_kernel_big(k_max) ? sizeof(double) * 8 * 4 : net_lds_bytes(net_kernel_waves(k_max), k_max);
}

size_t net_big_slot_bytes(int k_max) { return (net_lds_bytes(4, k_max) + 255) / 256 * 256; }

hipError_t launch_net(const NetParams& P0, int64_t n_items, hipStream_t st) {
  NetParams P = P0;
  P.n_items = n_items;
  if (n_items <= 0) return hipSuccess;
  const size_t lds = net_kernel_lds(P.k_max);
  // the pairs' layout as a template argument where it is the plain one; the
  // Gram table's stride at run time
#define NR_NET_LAUNCH(NW_, BIG_, GRID, BLOCK)                                                                \
  do {                                                                                                      \
    if (P.symmetric && P.es == 1)                                                                           \
      hipLaunchKernelGGL((module_net_kernel<NW_, BIG_, true, 1>), GRID, BLOCK, lds, st, P);                 \
    else if (P.symmetric)                                                                                   \
      hipLaunchKernelGGL((module_net_kernel<NW_, BIG_, true, -1>), GRID, BLOCK, lds, st, P);                \
    else if (P.es == 1)                                                                                     \
      hipLaunchKernelGGL((module_net_kernel<NW_, BIG_, false, 1>), GRID, BLOCK, lds, st, P);                \
    else                                                                                                    \
      hipLaunchKernelGGL((module_net_kernel<NW_, BIG_, false, -1>), GRID, BLOCK, lds, st, P);               \
  } while (0)
  if (net_kernel_big(P.k_max)) {
    if (!P.big_scratch || P.big_slots <= 0) return hipErrorInvalidValue;
    const unsigned g = (unsigned)(n_items < P.big_slots ? n_items : P.big_slots);
    NR_NET_LAUNCH(4, true, dim3(g), dim3(256));
  } else if (net_kernel_waves(P.k_max) == 4) {
    NR_NET_LAUNCH(4, false, dim3((unsigned)n_items), dim3(256));
  } else {
    NR_NET_LAUNCH(2, false, dim3((unsigned)n_items), dim3(128));
  }
#undef NR_NET_LAUNCH
  return hipGetLastError();
}

hipError_t launch_profile(const ProfileParams& P, const ProfilePlan& plan, hipStream_t st) {
  const dim3 g((unsigned)plan.slots), b((unsigned)plan.block);
#define NR_PROFILE_LAUNCH(K, ...) \
  case ProfileKernel::K: hipLaunchKernelGGL((__VA_ARGS__), g, b, plan.lds, st, P); break
  switch (plan.kernel) {
    NR_PROFILE_LAUNCH(FullGram, module_profile_kernel);
    NR_PROFILE_LAUNCH(PackedFixed, module_profile_packed4_kernel<kPackedLayoutK, 3>);
    NR_PROFILE_LAUNCH(PackedRuntime, module_profile_packed4_kernel<0, 2>);
    NR_PROFILE_LAUNCH(PackedBig, module_profile_big_kernel);
    NR_PROFILE_LAUNCH(Table, module_profile_table_kernel);
    NR_PROFILE_LAUNCH(Small, module_profile_small_kernel<kSmallWaves>);
    NR_PROFILE_LAUNCH(Wave, module_profile_wave_kernel);
  }
#undef NR_PROFILE_LAUNCH
  return hipGetLastError();
}

hipError_t launch_interleave(const double* corr, const double* net, double2* out, int64_t n_elem,
                             hipStream_t st) {
  hipLaunchKernelGGL(interleave_kernel, dim3(4096), dim3(256), 0, st, corr, net, out, n_elem);
  return hipGetLastError();
}

hipError_t launch_gram_full(const double* X, int64_t S, int64_t n, double* gram, double* colsum, hipStream_t st) {
  const int64_t T = (n + 31) / 32;
  const unsigned g = (unsigned)std::min<int64_t>((T * T + 3) / 4, 8192);
  hipLaunchKernelGGL(gram_full_kernel, dim3(g), dim3(256), 0, st, X, (int)S, n, gram);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(colsum_kernel, dim3((unsigned)std::min<int64_t>((n + 3) / 4, 4096)), dim3(256), 0, st, X,
                     (int)S, n, colsum);
  return hipGetLastError();
}

hipError_t launch_widen_pairs(const double2* in, const double* gram, double2* out, int64_t n, int symmetric,
                              hipStream_t st) {
  const unsigned nb = (unsigned)((n + 31) / 32);
  hipLaunchKernelGGL(widen_pairs_kernel, dim3(nb, nb), dim3(256), 0, st, in, gram, out, n, symmetric);
  return hipGetLastError();
}

hipError_t launch_symmetry(const double2* a, int64_t n, int* asym, hipStream_t st) {
  const unsigned nb = (unsigned)((n + 31) / 32);
  hipLaunchKernelGGL(symmetry_kernel, dim3(nb, nb), dim3(256), 0, st, a, n, asym);
  return hipGetLastError();
}

hipError_t launch_xdr(const void* raw, double2* pairs, int half, double* plain, int64_t n, hipStream_t st) {
  const unsigned g = (unsigned)std::min<int64_t>((n + 255) / 256, 8192);
  if (pairs)
    hipLaunchKernelGGL(xdr_pairs_kernel, dim3(g), dim3(256), 0, st, (const unsigned long long*)raw, pairs, n, half);
  else
    hipLaunchKernelGGL(xdr_plain_kernel, dim3(g), dim3(256), 0, st, (const unsigned long long*)raw, plain, n);
  return hipGetLastError();
}

hipError_t launch_scale(const double* in, double* out, int64_t S, int64_t N, hipStream_t st) {
  const unsigned nb = (unsigned)((N + 3) / 4);
  hipLaunchKernelGGL(scale_kernel, dim3(nb), dim3(256), 0, st, in, out, S, N);
  return hipGetLastError();
}

hipError_t launch_finite(const double* a, int64_t n, int* nonfinite, hipStream_t st) {
  hipLaunchKernelGGL(finite_kernel, dim3(2048), dim3(256), 0, st, a, n, nonfinite);
  return hipGetLastError();
}

hipError_t launch_export(const IndexSource& src, int64_t n_nodes_total, int32_t* out,
                         int64_t n_perm, hipStream_t st) {
  const unsigned gx = (unsigned)((n_nodes_total + 255) / 256 < 64 ? (n_nodes_total + 255) / 256 : 64);
  hipLaunchKernelGGL(export_indices_kernel, dim3(gx > 0 ? gx : 1, (unsigned)n_perm), dim3(256), 0, st,
                     src, n_nodes_total, out, n_perm);
  return hipGetLastError();
}

}  // namespace nr
