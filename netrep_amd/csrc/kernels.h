// Launch parameter blocks shared by kernels.hip and engine.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "profile_plan.h"

namespace nr {

enum { NR_IDX_PRP = 0, NR_IDX_TABLE = 1, NR_IDX_DIRECT = 2 };

// phase-stamp slots of the summary-profile kernel (nr_set_stamps)
constexpr int NR_N_STAMPS = 16;

// Where the test column of module node c comes from.
struct IndexSource {
  int mode;                    // NR_IDX_*
  uint64_t seed;               // PRP key
  int64_t perm_base;           // global index of local permutation 0
  uint32_t n_null;             // null-pool size
  const int32_t* null_idx;     // [n_null] test columns of the null pool
  const int32_t* null_pos;     // [nodes] null-pool position of each module node
  const uint32_t* pi;          // [n_perm x n_null] explicit shuffles (TABLE)
  const int32_t* direct_idx;   // [nodes] test column of each node (DIRECT)
};

struct NetParams {
  const double2* pairs;        // interleaved {corr, net}, column-major n x n (es = 1), or the
                               // Gram table: {corr, net}, {gram, net^T} per (i, j) (es = 2)
  int32_t es;                  // element stride of pairs in double2 units (1 or 2)
  const double* colsum;        // [n_nodes] column sums of the data (Gram table only)
  int64_t n_nodes;
  int symmetric;               // both matrices exactly symmetric
  IndexSource src;
  const int64_t* node_off;     // [n_mod + 1]
  const int64_t* cv_off;       // [n_mod + 1] CorrVector offsets (k(k-1)/2)
  const double* disc_cv;       // discovery CorrVector (NULL: no statistics)
  const double* disc_wd;       // discovery weighted degree
  const double* cv_shift;      // [n_mod] one-pass shift for the discovery corr values
  const int32_t* mod_order;    // [n_present] module processing order (large first)
  int32_t n_perm;              // permutations in this launch
  int32_t k_max;
  const int32_t* row_of;       // [n_mod] output row
  int32_t n_rows, n_stat;
  int32_t slot_avg_weight, slot_cor_cor, slot_cor_degree, slot_avg_cor;
  double* out;                 // cube slice (NULL in vector mode)
  double* cv_out;              // vector outputs (NULL unless vector mode)
  double* wd_out;
  double* avgw_out;            // [n_mod] average edge weight (vector mode)
  int64_t n_items;             // items of this launch (set by launch_net)
  // Modules too large for the per-node arrays in LDS: a persistent grid of
  // big_slots workgroups, each with big_stride doubles of global scratch
  double* big_scratch;
  int64_t big_stride;
  int32_t big_slots;
};

struct ProfileParams {
  const double* data;          // n_samples x (n_nodes + 2), column-major, scaled; column n_nodes
                               // all ones, n_nodes + 1 zeros (the Gram's virtual columns)
  int64_t n_samples;
  int64_t ones_off;            // n_nodes * n_samples: offset of the ones column
  IndexSource src;
  const int64_t* node_off;
  const double* disc_nc;       // discovery contribution (NULL: vector mode)
  const int32_t* mod_order;
  int32_t n_perm;
  int32_t n_items;
  int32_t k_max, m_max;
  int32_t ld;                  // leading dimension of the per-slot Gram (full storage)
  int64_t gram_doubles;        // doubles reserved for the Gram per slot
  const int32_t* row_of;
  int32_t n_rows, n_stat;
  int32_t slot_coherence, slot_cor_contrib, slot_avg_contrib;
  double* out;
  double* sp_out;              // [n_mod x n_samples] summary profiles (vector mode)
  double* nc_out;              // [nodes] node contributions (vector mode)
  double* coh_out;             // [n_mod] coherence (vector mode)
  double* scratch;             // per-slot Gram (ld x ld) + Lanczos basis (k_max x m_max)
  int64_t scratch_stride;
  int* queue;                  // work-queue head, zeroed before launch
  int* diag;                   // [0] Lanczos step-cap hits, [1] items, [2] Lanczos steps, [3] reorthogonalisations
  unsigned long long* stamps;  // [8] per-phase shader cycles (diagnostics; NULL = off)
  int32_t kvec;                // LDS vector length (0: k_max); larger (dual) modules keep their
                               // per-node arrays in the slot's scratch
  int64_t basis_doubles;       // Lanczos basis doubles per slot (behind the Gram)
  int64_t g32_off;             // doubles from the slot start to the fp32 copy of the packed Gram
                               // (relaxed Lanczos steps; 0: no copy, fp64 matvecs throughout)
  int32_t vec_global;          // 1: the Lanczos vectors, per-node arrays and index set in the slot's
                               // scratch too (ProfileClass::FullVectorsInScratch)
  int32_t order_tail;          // queue order: 0 = module-major (large modules first); T > 0 =
                               // permutation-major over all modules (a size mix in flight) for the
                               // first n_perm - T permutations, the last T module-major
  // The Gram-table kernel only: each item's network statistics, from the one
  // gather per pair of the table that also fills the item's packed Gram
  NetParams net;
};

// The column sweep (sweep.hip): network statistics of a batch organised by
// test column (each column chunk streamed into LDS once, every occurrence of
// the column reads its rows there) instead of one random gather per pair.
constexpr int kSweepWaves = 16;                   // waves per (column, chunk) workgroup: one per CU
// Lanes per occurrence: 8 (16: 2-5% slower at C4 / C2, r05/l8b), except where a
// module exceeds kSweepWideK nodes (C5): 16 lanes halve each
// occurrence's serial run over its entries, and at C5's 64-permutation
// launches (~64 occurrences per column) eight-lane batches fill only half of
// a workgroup's 16 waves (C5 sweep 12.8 ms per 64 permutations at 16 lanes,
// 16.3 at 8: profiles/r05/final3/C5.json, profiles/r05/sweep16/)
constexpr int kSweepWideK = 1024;
constexpr int kSweepMaxChunks = 16;               // chunks per column (n <= 65,535)
constexpr int kSweepMaxK = 4096;                  // module nodes (LDS of the per-item kernels)
constexpr int64_t kSweepChunkBytes = 160000;      // LDS per (column, chunk) workgroup
constexpr int kSweepRec = 12;                     // doubles per (occurrence, chunk) record
struct SweepParams {
  const double2* pairs;        // {corr, net} (es = 1) or the Gram table (es = 2), column-major n x n
  int64_t n_nodes;
  int32_t es;
  IndexSource src;
  int64_t n_node_total;        // module nodes of the present modules (CSR)
  int32_t n_present;
  const int64_t* node_off;     // [n_present + 1]
  const int32_t* mod_order;    // [n_present] modules by size, descending
  const int64_t* cv_off;       // [n_present + 1] CorrVector offsets
  const double* disc_cv;       // discovery CorrVector (NULL: no CorrVector statistics)
  int64_t n_cv;                // its length
  int32_t finite;              // 1: the test correlations and disc_cv are all finite (no complete-case tests)
  const double* disc_wd;       // discovery weighted degree
  const double* cv_shift;      // [n_present] one-pass shift of the discovery values
  int32_t n_perm;              // permutations of this batch
  int32_t k_max;
  int64_t n_occ;               // n_perm x n_node_total occurrences
  int64_t chunk_rows;          // rows per column chunk
  int32_t n_chunks;
  // per batch work buffers
  int32_t* col;                // [n_occ] test column of each (permutation, node)
  uint32_t* sorted;            // [n_occ] per item: (column << 16 | position), sorted by column
  int32_t* rank;               // [n_occ] sorted rank of each position
  int32_t* count;              // [n_nodes] occurrences per column
  int32_t* col_off;            // [n_nodes + 1]
  const double* zero;          // >= 32 zero bytes: the address of a lane with nothing to load
  double* sink;                // [256] the address of a lane with nothing to store
  double* dabs;                // [n_nodes] |diagonal| of each column with occurrences (written by the sweep)
  int32_t* lrank;              // [n_occ] slot of each occurrence within its column
  uint4* meta;                 // [n_occ x 2] by column slot: item base, jj | rank << 16, CorrVector base,
                               //   b1 | k << 16; CorrVector shifts {module, item}
  uint32_t* bndh;              // [n_chunks x n_occ] by slot (more than two chunks): e0 | e1 << 16 of the chunk
  double* rec;                 // [n_occ x n_chunks x kSweepRec] one record per (occurrence, chunk)
  const int32_t* row_of;
  int32_t n_rows, n_stat;
  int32_t slot_avg_weight, slot_cor_cor, slot_cor_degree, slot_avg_cor;
  double* out;
};
// rows per chunk for LDS elements of elem_bytes (16: {corr, net}; 8: net only)
int64_t sweep_chunk_rows(int64_t n_nodes, int elem_bytes, int64_t cap_rows = 0);
bool sweep_supported(int64_t n_nodes, int k_max);
hipError_t launch_sweep(const SweepParams& P, hipStream_t st);

size_t net_kernel_lds(int k_max);
bool net_kernel_big(int k_max);        // per-node arrays in global scratch
size_t net_big_slot_bytes(int k_max);  // global scratch per workgroup in that mode
hipError_t launch_net(const NetParams& P, int64_t n_items, hipStream_t st);
// The Gram table of a dataset with data: gram[i + j n] = x_i . x_j over the
// n_samples rows of X (n_samples x (n + 2), the virtual columns behind), and
// colsum[j] = sum of column j.
hipError_t launch_gram_full(const double* X, int64_t S, int64_t n, double* gram, double* colsum, hipStream_t st);
// {corr, net} pairs (es = 1) + gram -> the table layout (es = 2):
// out[2e] = in[e], out[2e + 1] = {gram[e], net(j, i)} for e = i + j n.
hipError_t launch_widen_pairs(const double2* in, const double* gram, double2* out, int64_t n, int symmetric,
                              hipStream_t st);
// One summary-profile launch as planned (profile_plan.h): plan.kernel on
// plan.slots workgroups of plan.block threads and plan.lds bytes of LDS.
hipError_t launch_profile(const ProfileParams& P, const ProfilePlan& plan, hipStream_t st);
hipError_t launch_interleave(const double* corr, const double* net, double2* out, int64_t n_elem,
                             hipStream_t st);
hipError_t launch_symmetry(const double2* a, int64_t n, int* asym, hipStream_t st);
// The from-data path (netbuild.hip): {corr, net} pairs (es = 1) of the scaled
// block X (S x (n + 2), the virtual columns behind): corr = clamp(x_i . x_j /
// (S - 1), -1, 1), net by net_type (NR_NET_*) and beta, one workgroup per
// kNetbuildTile-square tile of the lower triangle, each tile stored at (i, j)
// and mirrored at (j, i). flags (symmetry_kernel's layout): |= 2 for a
// non-finite corr, |= 4 for a non-finite net.
constexpr int kNetbuildTile = 64;
hipError_t launch_netbuild(const double* X, int64_t S, int64_t n, double2* pairs, int net_type, double beta,
                           int* flags, hipStream_t st);
// The topological overlap of a from-data network (NR_NET_TOM), in place: the
// .y of every pair becomes t_ij = (sum_u a_iu a_uj + a_ij) / (min(k_i, k_j) +
// 1 - a_ij), a the .y with a zero diagonal, k its column sums, t_ii = 1; the
// .x keeps its bits. scratch: tom_scratch_bytes(n) bytes, the plain matrix A
// (n rows, n + 2 columns, column-major: a with a zero diagonal in columns
// 0 .. n - 1, columns n and n + 1 zero -- the SYRK main loop reads column
// n + 1 for every panel column past n) and, behind it, k[n]. Two launches:
// extract + degrees, then the same tile SYRK as launch_netbuild with K = n.
// flags |= 4 for a non-finite t.
size_t tom_scratch_bytes(int64_t n);
hipError_t launch_tom(int64_t n, double2* pairs, double* scratch, int* flags, hipStream_t st);
// The correlation types other than Pearson (cortransform.hip; NR_COR_SPEARMAN,
// NR_COR_BICOR): Z, S x (n + 2) with both padding columns zero, from the scaled
// block X, for launch_netbuild to run on instead of X. scratch:
// cor_scratch_bytes(n, S, cor_type) bytes (0 for Pearson): Z and, for
// Spearman, the plain S x n rank buffer behind it that launch_scale turns into
// Z. A column is staged in LDS up to kCorLdsRows rows (beyond: swept in global
// memory); up to kCorWaveRows rows a wave owns a column and a workgroup holds
// four (cor_cols_per_workgroup), above that a workgroup owns one.
constexpr int kCorLdsRows = 2048;
constexpr int kCorWaveRows = kCorLdsRows / 4;
int cor_cols_per_workgroup(int64_t S);
size_t cor_scratch_bytes(int64_t n, int64_t S, int cor_type);
hipError_t launch_cor_transform(const double* X, int64_t S, int64_t n, int cor_type, double* scratch,
                                hipStream_t st);
// The soft-threshold connectivities (netbuild.hip, nr_soft_connectivity):
// k[j + m n] = sum over i != j of b_ij^powers[m], b the base of net_type
// (|c|, (1 + c) / 2, or c where c > 0 else 0) of c = clamp(x_i . x_j / (S - 1),
// -1, 1), from the block X that launch_netbuild takes; no n x n array exists.
// soft_connectivity_kernel: one workgroup per (column tile, row group) walks
// its row tiles through the SYRK main loop and keeps one running sum per
// distinct power and column in registers; it writes part[r][slot][j]. A second
// kernel adds the row groups in increasing r. No floating-point atomics: k
// depends on n and the row-group count alone, never on the grid's schedule.
// All powers integers <= kSftMaxChain: one multiplication chain b, b^2, ...
// per element; otherwise one pow per element and distinct power. A launch
// holds 16 distinct powers on the chain path, 8 on the pow path; more run
// another sweep of the matrix into the same partials. row_groups
// 0: sft_row_groups(n). scratch: sft_scratch_bytes(n, P, R) bytes, the
// partials (8 R P n) and k (8 P n) behind them; the result is at
// scratch + sft_result_offset(n, P, R) doubles. flags |= 4 for a non-finite k.
constexpr int kSftMaxPowers = 32;
constexpr int kSftMaxChain = 64;
constexpr int kSftTilesPerGroup = 16;   // row tiles a workgroup walks by default
constexpr int kSftMaxRowGroups = 32;    // default row groups at most (bounds the partials)
constexpr int kSftRowGroupsLimit = 1024;  // largest row-group count the test override takes
int sft_row_groups(int64_t n);
size_t sft_result_offset(int64_t n, int n_powers, int row_groups);
size_t sft_scratch_bytes(int64_t n, int n_powers, int row_groups);
hipError_t launch_soft_connectivity(const double* X, int64_t S, int64_t n, int net_type, const double* powers,
                                    int n_powers, int row_groups, double* scratch, int* flags, hipStream_t st);
// The average-linkage dendrogram of the resident network (hclust.hip,
// nr_hclust_average). hclust_extract_kernel writes the working matrix D
// (column-major, n columns of ld = hclust_ld(n) doubles: 1 - net, +inf on the
// diagonal and in the padding row) from the pairs in either layout, and the
// chain's initial state; hclust_chain_kernel, one workgroup of 1,024 threads,
// runs the nearest-neighbour chain for at most max_merges merges per launch
// and resumes from the state block. state: hclust_state_bytes(n) bytes, laid
// out by hclust_params.
enum { kHclustStChainLen = 0, kHclustStMerged, kHclustStSearches, kHclustStError, kHclustStFirstLive,
       kHclustStateWords = 8 };
struct HclustParams {
  double* D;                   // n x ld working matrix
  int64_t n, ld;
  long long* st;               // [kHclustStateWords] state words
  double* size;                // [n] cluster size of each slot (0: retired)
  int32_t* chain;              // [n] the chain's stack of slots
  int32_t* id;                 // [n] cluster id of each slot
  int32_t *m_lo, *m_hi;        // [n - 1] emitted merges, discovery order
  double *m_height, *m_size;
  int64_t max_merges;          // merges per launch
  int64_t search_cap;          // nearest-neighbour searches per call (hclust_search_cap)
};
size_t hclust_state_bytes(int64_t n);
HclustParams hclust_params(int64_t n, double* D, void* state);
hipError_t launch_hclust_extract(const double2* pairs, int es, const HclustParams& P, hipStream_t st);
hipError_t launch_hclust_chain(const HclustParams& P, hipStream_t st);
// Module membership (membership.hip, nr_module_membership): ehat = the centred,
// unit-norm columns of eig (S x M, column-major); kme [n x M, column-major] =
// the correlation of every column of the node-major data block with every
// column of ehat. A workgroup holds kMembershipNodes centred columns in LDS
// while ehat passes by in tiles of 16 rm eigengenes; membership_tile, a pure
// function of S, gives rm (eigengenes per thread), the sample chunk, the LDS
// row stride and the bytes: the largest rm of 4, 2, 1 whose
// (16 + 16 rm) (S | 1) doubles fit kMembershipLds with the whole column
// resident (S <= 229, 383, 575); beyond that rm = 1 and columns and tile are
// both walked in chunks of kMembershipChunk samples.
constexpr int kMembershipNodes = 16;
constexpr size_t kMembershipLds = 144 * 1024;
constexpr int kMembershipChunk = 512;
struct MembershipTile {
  int rm, chunk, pad;
  size_t lds;
};
MembershipTile membership_tile(int64_t S);
hipError_t launch_eigengene_unit(const double* eig, int64_t S, int M, double* ehat, hipStream_t st);
hipError_t launch_membership(const double* data, int64_t S, int64_t n, const double* ehat, int M, double* kme,
                             hipStream_t st);
// Module connectivity (connectivity.hip, nr_module_connectivity): k_mod
// [n x M, column-major] and k_total [n] (may be NULL) from the pairs in either
// layout and slot [n] (-1 .. M - 1), all device arrays. One wave per column
// keeps a tile of module bins in LDS, 512 bytes per module; M modules run
// ceil(M / tile) launches over the network. connectivity_tile, a pure function
// of M: the passes are the fewest that kConnectivityTileMax modules each
// allow, ceil(M / 64), and the tile splits M evenly among them, ceil(M /
// passes), so a wave holds at most 32 KiB and a CU at least five waves.
// tile 0: that default; else 1 .. kConnectivityTileMax (a test's choice).
constexpr int kConnectivityTileMax = 64;
int connectivity_tile(int M);
hipError_t launch_connectivity(const double2* pairs, int es, int64_t n, const int32_t* slot, int M, int tile,
                               double* k_total, double* k_mod, hipStream_t st);
// corr[e], net[e] (either may be NULL) = elements [first, first + len) of a
// pair array in layout es (1, or 2: the Gram table).
hipError_t launch_deinterleave(const double2* pairs, int es, int64_t first, int64_t len, double* corr, double* net,
                               hipStream_t st);
hipError_t launch_scale(const double* in, double* out, int64_t S, int64_t N, hipStream_t st);
// XDR (big-endian) doubles -> native: into pairs[i].x (half 0) / .y (half 1), or `plain`
hipError_t launch_xdr(const void* raw, double2* pairs, int half, double* plain, int64_t n, hipStream_t st);
hipError_t launch_finite(const double* a, int64_t n, int* nonfinite, hipStream_t st);
hipError_t launch_export(const IndexSource& src, int64_t n_nodes_total, int32_t* out,
                         int64_t n_perm, hipStream_t st);

}  // namespace nr
