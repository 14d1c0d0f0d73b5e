/* netrep_gpu.h -- C ABI of the MI355X NetRep permutation engine.
 *
 * Plain pointers and sizes only; no C++ exceptions cross this boundary. All
 * matrices are R column-major fp64: A(i,j) at i + j*nrow. Every function
 * returns NR_OK (0) or an NR_ERR_* code; nr_last_error() has the message.
 *
 * Two layers:
 *  1. Engine layer (nr_*): one context per GPU holding ONE dataset resident
 *     in HBM, as the reference holds one dataset in RAM at a time
 *     (R/modulePreservation.R:553-620). It replaces the std::thread pool of
 *     calculateNulls (src/permutations.cpp:39-105, :335-380;
 *     src/permutationsNoData.cpp:35-89, :305-339) with batched device
 *     launches, and the Armadillo/LAPACK statistics of src/netStats.cpp with
 *     HIP kernels.
 *  2. Reference-interface layer (netrep_*): the eight Rcpp entry points of
 *     src/RcppExports.cpp:131-146 with the same argument meaning, taking
 *     names as C strings. An Rcpp glue unpacks SEXPs and
 *     calls these one-for-one.
 */
#ifndef NETREP_GPU_H
#define NETREP_GPU_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NR_OK 0
#define NR_ERR_HIP 1          /* HIP runtime / launch failure */
#define NR_ERR_INVALID 2      /* bad argument, shape or missing prerequisite */
#define NR_ERR_OOM 3          /* device allocation failed */
#define NR_ERR_UNSUPPORTED 4  /* size beyond an engine limit (n_nodes >= 2^31); modules of any
                                 size and any sample count are accepted, as svd_econ accepts any
                                 S x k block (src/netStats.cpp:217-280): Lanczos dimensions beyond
                                 the LDS vectors keep their vectors in device scratch */
#define NR_ERR_CANCELLED 5    /* nr_cancel() was called during a run */
#define NR_ERR_NONFINITE 6    /* CheckFinite failure (src/checkFinite.cpp:25-27) */
#define NR_ERR_INTERNAL 7     /* a kernel's termination guard stopped it (nr_hclust_average) */

#define NR_HOST 0
#define NR_DEVICE 1

/* Statistic slots in the nulls cube (src/permutations.cpp:95-101, :174-177). */
#define NR_NSTAT_DATA 7
#define NR_NSTAT_NODATA 4

typedef struct nr_ctx nr_ctx;

/* ---- engine layer ------------------------------------------------------ */

int nr_device_count(int* count);
int nr_ctx_create(int device, nr_ctx** out);
void nr_ctx_destroy(nr_ctx* ctx);
/* Message of the last failing call on ctx (ctx == NULL: last nr_ctx_create failure). */
const char* nr_last_error(const nr_ctx* ctx);

/* Make one dataset resident: corr, net (n_nodes x n_nodes) and optional data
 * (n_samples x n_nodes, scaled as by Scale, src/scale.cpp:14-25; NULL for the
 * network-only path). `where` = NR_HOST or NR_DEVICE (device pointers, e.g.
 * after an RCCL broadcast). Replaces the previous dataset. The matrices are
 * stored interleaved as {corr(i,j), net(i,j)} pairs so one 16-byte read serves
 * CorrVector (src/netStats.cpp:196-201) and WeightedDegree (:135). */
int nr_set_dataset(nr_ctx* ctx, const double* corr, const double* net,
                   const double* data, int64_t n_nodes, int64_t n_samples, int where);
/* The same with flags: NR_SCALE_DATA = `data` is unscaled and is scaled on
 * the device (Scale, src/scale.cpp:14-25) on its way into HBM (NetProps,
 * src/properties.cpp:49). corr == net (same pointer): the matrix crosses
 * PCIe once and fills both halves of the pairs. */
#define NR_SCALE_DATA 1
int nr_set_dataset_ex(nr_ctx* ctx, const double* corr, const double* net,
                      const double* data, int64_t n_nodes, int64_t n_samples, int where, int flags);
/* The from-data path: the resident dataset made from the data matrix alone,
 * as NetRep users derive the other two from it (R/example-data.R:111-116:
 * cor(data), abs(correlation)^5). Only `data` (n_samples x n_nodes) is
 * uploaded (flags: NR_SCALE_DATA = unscaled, scaled on the device; 0 = already
 * scaled as by Scale); a lower-triangle SYRK on the fp64 matrix cores then
 * writes the {corr, net} pairs in place:
 *   corr(i,j) = clamp(x_i . x_j / (n_samples - 1), -1, 1)   (R's cor clamps)
 *   net(i,j)  = |corr|^beta                  NR_NET_UNSIGNED
 *               ((1 + corr) / 2)^beta        NR_NET_SIGNED
 *               corr > 0 ? corr^beta : 0     NR_NET_SIGNED_HYBRID
 * with NaN propagating through all three. Every tile is stored at (i, j) and,
 * the same bits, at (j, i): the matrices are exactly symmetric by
 * construction (no symmetry pass), and nr_dataset_finite reports what the
 * kernel's epilogue saw (a constant column gives NaN, as R's cor gives NA).
 * Everything downstream (modules, observed, run, Gram table, broadcast) runs
 * on the dataset unchanged. NR_ERR_INVALID before anything touches the GPU:
 * data == NULL, n_samples < 2, n_nodes < 1, an unknown net_type or flag, beta
 * not finite or <= 0. `where` as nr_set_dataset. */
#define NR_NET_UNSIGNED 0
#define NR_NET_SIGNED 1
#define NR_NET_SIGNED_HYBRID 2
/* OR-ed onto one of the three: the resident net becomes the topological
 * overlap matrix of that adjacency (WGCNA's unsigned TOM, TOMDenom = "min").
 * With a = net as above but a zero diagonal:
 *   k_i  = sum_u a_ui
 *   L_ij = sum_u a_iu a_uj
 *   t_ij = (L_ij + a_ij) / (min(k_i, k_j) + 1 - a_ij)   for i != j,  t_ii = 1
 * NaN propagates (a constant column makes every off-diagonal t NaN; the
 * diagonal stays 1); the denominator is >= 1. corr is what it is without the
 * flag, bit for bit, and t is stored at (i, j) and (j, i) from the same bits.
 * The order of work on the context's stream: the build as above, one pass
 * that extracts a and sums its columns in a fixed order (no atomics), then a
 * second lower-triangle SYRK with K = n_nodes on the fp64 matrix cores. It
 * needs 8 n (n + 2) + 8 n bytes of device scratch for the call (n = n_nodes),
 * freed before the call returns; when that allocation fails the call returns
 * NR_ERR_OOM and leaves no dataset resident. Any other net_type value stays
 * NR_ERR_INVALID. */
#define NR_NET_TOM 0x10
/* The correlation type, OR-ed onto net_type as NR_NET_TOM is (neither bit:
 * Pearson, exactly as above). net_type is (0|1|2) | (0|0x10) | (0|0x100|0x200);
 * both correlation bits together return NR_ERR_INVALID "unknown correlation
 * type", every other value NR_ERR_INVALID "unknown network type", before
 * anything touches the GPU. With X the resident data block (S x n, scaled as
 * by Scale whether or not NR_SCALE_DATA was given), a correlation type makes
 * a second, transient S x n matrix Z from X, column by column, and
 *   corr(i,j) = clamp(z_i . z_j / (S - 1), -1, 1)
 * by the same kernel, run on Z instead of X; the clamp, the network types,
 * NR_NET_TOM, the mirrored stores and the finite flags are as above. X stays
 * the dataset's data block: the Gram table and all seven statistics run on it
 * unchanged.
 *   NR_COR_SPEARMAN: z = Scale(r) with r_i = L_i + (E_i + 1) / 2, L_i the
 *     number of entries of the column less than x_i, E_i the number equal to
 *     it (itself included): R's rank(ties.method = "average"), exact. +-Inf
 *     are ranked like any value, as R does; a column holding a NaN becomes
 *     all NaN; a constant column has sd 0 and becomes NaN, as for Pearson.
 *   NR_COR_BICOR: WGCNA's bicor with its defaults (maxPOutliers = 1,
 *     pearsonFallback = "individual"). med = median of the column, always
 *     0.5 (lo + hi) of the order statistics at 0-based positions (S - 1) / 2
 *     and S / 2; d_i = |x_i - med|; mad = median of d (no 1.4826 factor);
 *     u_i = (x_i - med) / (9 mad); w_i = (1 - u_i^2)^2 where |u_i| < 1, else
 *     0; a_i = (x_i - med) w_i; if mad == 0, a_i = x_i - mean(x) (the Pearson
 *     fallback for that column alone); z_i = a_i sqrt(S - 1) / sqrt(sum a^2).
 *     A column with any non-finite entry becomes all NaN; an all-zero a (a
 *     constant column) gives 0 / 0 = NaN.
 * Both read the *scaled* block. Both are invariant under a column's positive
 * affine map, so scaling changes nothing except where its rounding merges two
 * distinct raw values into a tie. Ranks and order statistics come from exact
 * counting (no atomics, independent of scheduling); the sums run in a fixed
 * order. Device scratch for the call: 8 S (n + 2) bytes for Z and, for
 * Spearman, 8 S n for the ranks; freed before the call returns; when the
 * allocation fails the call returns NR_ERR_OOM and leaves no dataset
 * resident. Order of work on the context's stream: transform (+ scale), the
 * build on Z, the optional TOM. */
#define NR_COR_SPEARMAN 0x100
#define NR_COR_BICOR 0x200
int nr_set_dataset_from_data(nr_ctx* ctx, const double* data, int64_t n_nodes, int64_t n_samples,
                             int where, int flags, int net_type, double beta);
/* Device time in ms (HIP events on the context's stream) of the kernel that
 * built the resident dataset's matrices from its data; 0 for a dataset made
 * any other way. A copy (nr_copy_dataset, nr_broadcast_dataset) reports the
 * figure of the dataset it was copied from. */
int nr_netbuild_ms(nr_ctx* ctx, double* ms);
/* Device time in ms of the NR_NET_TOM step behind that kernel (extract,
 * degrees and the TOM kernel together; nr_netbuild_ms does not include it);
 * 0 for a dataset built without NR_NET_TOM or made any other way. A copy
 * reports its source's figure. */
int nr_tom_ms(nr_ctx* ctx, double* ms);
/* Device time in ms of the correlation-type transform ahead of that kernel
 * (NR_COR_SPEARMAN: ranks and their scaling; NR_COR_BICOR: the bicor
 * columns; neither nr_netbuild_ms nor nr_tom_ms includes it); 0 for Pearson
 * or a dataset made any other way. A copy reports its source's figure. */
int nr_cor_ms(nr_ctx* ctx, double* ms);

/* The soft-threshold connectivities of WGCNA's pickSoftThreshold, from the
 * data matrix alone: for each of the n_powers candidate powers,
 *   k_out[i + m n_nodes] = sum over u != i of b_iu ^ powers[m]
 * with c = clamp(x_i . x_u / (n_samples - 1), -1, 1) of the scaled data (or,
 * with NR_COR_SPEARMAN / NR_COR_BICOR in net_type, of its transform Z as
 * nr_set_dataset_from_data makes it), written as that call's kernel writes
 * it so that NaN stays NaN, and the base b of net_type:
 *   |c|                  NR_NET_UNSIGNED
 *   (1 + c) / 2          NR_NET_SIGNED
 *   c > 0 ? c : 0        NR_NET_SIGNED_HYBRID (NaN propagates)
 * The diagonal is left out (WGCNA sums it and subtracts 1); n_nodes = 1
 * gives k = 0; a column that is NaN (a constant column) makes every k NaN.
 * powers: finite and > 0, their order and duplicates kept (duplicates come
 * out bitwise equal), n_powers <= 32. If every power is an integer <= 64,
 * b^p comes from one multiplication chain b, b b, (b b) b, ... per element;
 * otherwise every power takes one pow(b, p). `data` is host memory,
 * n_samples x n_nodes, raw (scale != 0: scaled on the device) or scaled as by
 * Scale (scale == 0). NR_ERR_INVALID before anything touches the GPU: a NULL
 * pointer, n_samples < 2, n_nodes < 1, n_powers outside 1 .. 32, a power not
 * finite or <= 0, NR_NET_TOM in net_type ("NR_NET_TOM has no soft-threshold
 * connectivity"), any other unknown type.
 * No n x n array exists at any time. Only `data` is uploaded, into a
 * transient block; one workgroup per (64-column tile, row group) runs the
 * from-data kernel's SYRK main loop over its row tiles of the full matrix
 * and keeps one running sum per distinct power and column in registers; a
 * second kernel adds the R row groups in increasing order. No floating-point
 * atomics: the result is bitwise repeatable and a function of the inputs and
 * R alone; R is a function of n_nodes alone (ceil(ceil(n / 64) / 16), at most
 * 32), never of the device. Device memory for the call, all freed before it
 * returns on every path: the block, 8 S (n + 2) bytes (8 S n more while it is
 * scaled), the correlation-type scratch, and 8 R P n + 8 P n bytes of partial
 * sums and result; a failed allocation returns NR_ERR_OOM naming the bytes.
 * The context's resident dataset, modules, null pool and per-batch buffers
 * are not touched. */
int nr_soft_connectivity(nr_ctx* ctx, const double* data, int64_t n_nodes, int64_t n_samples, int scale,
                         int net_type, const double* powers, int n_powers, double* k_out);
/* Device time in ms (HIP events) of the two kernels of the context's last
 * nr_soft_connectivity call (not the upload, scaling or transform); 0 before
 * the first. */
int nr_sft_ms(nr_ctx* ctx, double* ms);
/* 1 if every connectivity of that call was finite (the reduction kernel's
 * flag word, as nr_dataset_finite reports the build's), else 0. */
int nr_sft_finite(nr_ctx* ctx, int* finite);
/* Test knob: the number of row groups R of later nr_soft_connectivity calls
 * on this context (1 .. 1024; more groups than row tiles leaves the surplus
 * empty); 0 restores the default. It regroups the sums, so k moves at
 * rounding level. */
int nr_set_sft_row_groups(nr_ctx* ctx, int row_groups);

/* The average-linkage (UPGMA) dendrogram of the resident dataset's nodes, on
 * the GPU: what R's hclust(as.dist(1 - net), "average") computes, with every
 * tie broken by rule so that the output is a function of the resident net
 * alone.
 * Dissimilarity: d_ij = 1 - net_ij for i != j (net: the adjacency, or the TOM
 * of a dataset built with NR_NET_TOM), +inf on the diagonal. net must be
 * symmetric and finite, as every from-data dataset is by construction.
 * Linkage, by the Lance-Williams update with cluster sizes s as doubles:
 *   d(k, a u b) = (s_a d(k, a) + s_b d(k, b)) / (s_a + s_b)
 * as two multiplications, one addition, one division and the size sum, each
 * rounded to fp64 on its own (never fused).
 * Algorithm: the nearest-neighbour chain over n slots, one per node at first.
 *   - The merged cluster lives in the slot of the higher index hi = max(a, b);
 *     slot lo is retired.
 *   - An empty chain starts at the lowest-index live slot.
 *   - The nearest neighbour of the chain's top a is the live slot k != a with
 *     the smallest d(a, k); ties go to the lowest index, except that the
 *     chain's previous element is chosen whenever it attains the minimum.
 *   - When the nearest neighbour is the previous element the two are merged
 *     at height d(a, b); both are popped and the rest of the chain is kept.
 *   - Merges are emitted in discovery order: step t = 0 .. n - 2 gives
 *     id_lo[t], id_hi[t] (the ids of the clusters in slots lo and hi: 0 ..
 *     n - 1 are nodes, n + u is the cluster of step u), height[t] and size[t]
 *     (the merged cluster's node count). Heights need not be sorted.
 * n = 1 writes nothing; n = 2 gives one merge.
 * Device scratch for the call: the working matrix, 8 n ld bytes (ld = n
 * rounded up to even; 3.2 GB at n = 20,000), and 64 + 40 n bytes of chain
 * state; freed before the call returns on every path; a failed allocation
 * returns NR_ERR_OOM naming the bytes. The resident dataset is read once (in
 * either pair layout) to fill the working matrix and never written; modules,
 * null pool and per-batch buffers are not touched.
 * One workgroup runs the chain in launches of at most M merges each
 * (nr_set_hclust_merges_per_launch); nr_cancel, from any thread before or
 * during the call, is honoured between launches and consumed
 * (NR_ERR_CANCELLED, nothing written). The result does not depend on M.
 * Termination guard: the kernel counts its nearest-neighbour searches; it
 * stops, and is not launched again, when the call's total would exceed
 * 4 n + 16 (the rules need fewer than 3 n) or when a search finds no finite
 * neighbour while more than one slot is live: NR_ERR_INTERNAL with the reason.
 * NR_ERR_INVALID: no dataset, or an output missing with n > 1.
 * NR_ERR_UNSUPPORTED: n > 2^30. */
int nr_hclust_average(nr_ctx* ctx, int32_t* id_lo, int32_t* id_hi, double* height, double* size);
/* Device time in ms (HIP events) of the extract and all chain launches of the
 * context's last nr_hclust_average call; 0 before the first. */
int nr_hclust_ms(nr_ctx* ctx, double* ms);
/* Of that call (any output may be NULL): nearest-neighbour searches made,
 * chain launches, and device scratch bytes it allocated. */
int nr_hclust_info(nr_ctx* ctx, int64_t* searches, int64_t* launches, int64_t* scratch_bytes);
/* Test knob: merges per chain launch M of later nr_hclust_average calls on
 * this context; 0 restores the default (512). A call of n nodes takes
 * ceil((n - 1) / M) launches. It changes no result. */
int nr_set_hclust_merges_per_launch(nr_ctx* ctx, int64_t merges);
/* The guard's host-side arithmetic, pure host functions (no context, no GPU):
 * the search cap 4 n + 16 of a call of n_nodes, and the message of a kernel
 * error word (1: search cap exceeded, 2: no finite neighbour, 3: the chain
 * outgrew the live slots) into buf (NUL-terminated); NR_ERR_INVALID for an
 * unknown word or a buffer too small. */
int nr_hclust_search_cap(int64_t n_nodes, int64_t* cap);
int nr_hclust_error_message(int32_t word, char* buf, int64_t cap);
/* Module eigengenes on explicit index sets (CSR, as nr_module_vectors takes
 * them): the summary-profile half of nr_module_vectors and nothing else --
 * the same kernels, module order and size classes, so eigengenes,
 * var_explained and contribution carry the bits of its summary, coherence and
 * contribution -- with no network statistics and none of their allocations.
 * The eigengene of a module is NetRep's summary profile (src/netStats.cpp:
 * 217-250): the first left singular vector of the module's columns of the
 * resident data, unit length, its sign chosen so that it correlates
 * positively with the mean of the columns: WGCNA's moduleEigengenes for a
 * scaled data block. var_explained is the module's coherence (the mean
 * squared contribution), contribution each node's correlation with its own
 * module's eigengene, the in-module kME, in CSR order; it may be NULL.
 * eigengenes [n_samples x n_mod, column-major], var_explained [n_mod].
 * The eigengenes also stay in a device buffer of the context until the next
 * call, a dataset change or nr_release_scratch; the buffer counts in
 * nr_scratch_bytes. Nothing resident is written.
 * NR_ERR_INVALID: n_mod < 1, a missing array, no dataset or one without data,
 * an empty module, an index outside the dataset. */
int nr_module_eigengenes(nr_ctx* ctx, int32_t n_mod, const int64_t* node_off, const int32_t* idx,
                         double* eigengenes, double* var_explained, double* contribution);
/* Module membership of every node of the resident dataset:
 *   kME[i, m] = sum_s (x_si - mu_i) e^_sm / sqrt(sum_s (x_si - mu_i)^2),
 * x_i column i of the resident data exactly as stored (scaled or not), mu_i
 * its mean, e^_m eigengene m centred and scaled to unit length: the Pearson
 * correlation of node i with eigengene m. kme [n_nodes x n_mod, column-major].
 * eigengenes NULL: the n_mod eigengenes the context keeps from its last
 * nr_module_eigengenes call on this dataset (no upload); else n_mod host
 * columns [n_samples x n_mod], uploaded (counted in nr_h2d_bytes).
 * Every sum runs over s in increasing order per thread or lane set fixed by
 * n_samples alone and there are no atomics: a cell's bits do not depend on
 * n_mod, on the eigengene's place in the call, or on the other nodes.
 * Device scratch for the call: 8 n_samples n_mod (twice with an upload) and
 * 8 n_nodes n_mod bytes, freed before it returns. Nothing resident is written.
 * NR_ERR_INVALID: n_mod < 1, kme missing, no dataset or one without data,
 * n_samples < 3, or eigengenes NULL with no matching kept eigengenes. */
int nr_module_membership(nr_ctx* ctx, int32_t n_mod, const double* eigengenes, double* kme);
/* Device time in ms (HIP events) of the two kernels of the context's last
 * nr_module_membership call; 0 before the first. */
int nr_membership_ms(nr_ctx* ctx, double* ms);
/* Module connectivity of every node of the resident network: the network-side
 * counterpart of nr_module_membership. slot [n_nodes]: node j's module index
 * 0 .. n_mod - 1, or -1 for an unassigned node. With net the resident network
 * (adjacency or TOM),
 *   k_mod[i, m] = sum over j != i with slot[j] == m of |net[j, i]|,
 *   k_total[i]  = sum over all j != i of |net[j, i]|, unassigned nodes included.
 * k_mod [n_nodes x n_mod, column-major]; k_total [n_nodes], may be NULL.
 * The absolute value is what NetRep's weighted degree takes
 * (src/netStats.cpp:135); a from-data network is non-negative already, so
 * there it changes no bit, and a dataset set from host matrices with negative
 * weights is summed by magnitude, as nr_module_vectors' degree is.
 * The summation order is part of the contract:
 *   - each sum is split into 64 partials; partial l adds the participating
 *     rows j = l (mod 64) in increasing j, starting from +0.0;
 *   - the partials are combined by p[l] += p[l + off] for l < off, with
 *     off = 32, 16, 8, 4, 2, 1; the result is p[0];
 *   - a row that does not take part (the diagonal, another module's row) adds
 *     nothing, which for |net| >= 0 is the same as adding +0.0;
 *   - only additions occur, none fused, and there are no atomics.
 * So a cell's bits depend on (net, slot) alone: not on n_mod, on the module
 * tile, on the pair layout or on the device. k_total is not derived from the
 * module cells.
 * The network is read in either pair layout, once per module tile: n_mod
 * modules take ceil(n_mod / 64) passes, the tile being n_mod split evenly
 * among them. Device scratch for the call: 4 n + 8 n (n_mod + 1) bytes (slots,
 * table, k_total), freed before the call returns on every path; a failed
 * allocation returns NR_ERR_OOM naming the bytes. Nothing resident is
 * written and nr_scratch_bytes is unchanged. Any n_nodes >= 1 and n_mod >= 1.
 * NR_ERR_INVALID: n_mod < 1, slot or k_mod missing, no dataset, a slot
 * outside -1 .. n_mod - 1. */
int nr_module_connectivity(nr_ctx* ctx, int32_t n_mod, const int32_t* slot, double* k_total, double* k_mod);
/* Device time in ms (HIP events) of the kernels of the context's last
 * nr_module_connectivity call; 0 before the first. */
int nr_connectivity_ms(nr_ctx* ctx, double* ms);
/* Test knob: modules per pass of later nr_module_connectivity calls on this
 * context, 1 .. 64; 0 restores the default. It changes no result. */
int nr_set_connectivity_module_tile(nr_ctx* ctx, int32_t tile);
/* The resident corr and net (n_nodes x n_nodes each, column-major) to host
 * arrays; either may be NULL. Works for a dataset made by any of the
 * set-dataset calls, before or after the Gram table is built: the pairs are
 * split on the device into a bounded staging buffer and copied out in chunks. */
int nr_get_dataset_matrices(nr_ctx* ctx, double* corr_out, double* net_out);

/* Drop the resident dataset (and modules / null pool bound to it); the
 * context keeps its streams and scratch for the next dataset. */
int nr_clear_dataset(nr_ctx* ctx);

/* disk.matrix files straight to HBM (R/disk-matrix-class.R:175-182 reads them
 * back with readRDS): numeric matrices serialised by saveRDS (gzip or
 * uncompressed, XDR format 2/3) or objects of a save() archive (`*_object`,
 * NULL: the first numeric matrix). The payload is read straight into pinned
 * buffers and converted from big-endian on the device; `data` (samples x
 * nodes, NULL for the network-only path) is scaled there as Scale does
 * (src/scale.cpp:14-25) when scale_data != 0. The network file's column names
 * become the dataset's node names (nr_dataset_colnames). */
int nr_set_dataset_files(nr_ctx* ctx, const char* corr_path, const char* net_path, const char* data_path,
                         const char* corr_object, const char* net_object, const char* data_object,
                         int scale_data);
int nr_dataset_shape(const nr_ctx* ctx, int64_t* n_nodes, int64_t* n_samples);
/* NUL-separated node names of a dataset loaded from files; *needed = bytes
 * (written only when cap >= *needed). */
int nr_dataset_colnames(const nr_ctx* ctx, char* buf, int64_t cap, int64_t* needed);

/* Make src's resident dataset resident in dst too, device to device (over
 * xGMI when the contexts are on different GPUs): the host matrices cross PCIe
 * once, to the first GPU, and fan out from there. */
int nr_copy_dataset(nr_ctx* dst, const nr_ctx* src);
/* ctxs[0]'s resident dataset to ctxs[1..n): the broadcast of SURVEY.md 8e as
 * a scatter + all-gather of peer copies over the full xGMI mesh (each
 * destination receives one piece from the source and the other n - 2 pieces
 * from the destinations that received them; every link carries 1/(n-1) of
 * the bytes per phase). Contexts must be distinct; several may share a GPU.
 * Peer access is enabled per GPU pair; a pair without it is copied through
 * host memory by the runtime (slower, still correct) and counted by
 * nr_peer_staged_pairs. The calling thread's current device is restored. */
int nr_broadcast_dataset(nr_ctx* const* ctxs, int n);
/* Ordered GPU pairs found without peer access so far in this process. */
int nr_peer_staged_pairs(int* n);

/* 1 if corr and net of the resident dataset are exactly symmetric. */
int nr_dataset_symmetric(nr_ctx* ctx, int* symmetric);

/* 1 when the resident dataset carries the Gram table (the data block's
 * X^T X interleaved with the matrices, built by the first run or observed
 * call), else 0. Whether it is built depends on the shapes only (never on
 * free device memory): the packed-class modules (<= 320 nodes) must form one
 * packed-kernel launch (min(k, S) > 112, no module with more nodes than
 * samples), carry at least half the Gram work, and n_nodes <= 50,000; an
 * allocation failure then returns NR_ERR_OOM from the run / observed call
 * (DESIGN.md section 5.2). */
int nr_gram_table(nr_ctx* ctx, int* on);
/* Wall time in ms of the resident Gram table's build (X^T X on the matrix
 * cores + the widened layout, synchronised), 0 without a table. */
int nr_gram_table_ms(nr_ctx* ctx, double* ms);

/* CheckFinite (src/checkFinite.cpp:21-28) of the resident corr and net,
 * computed by nr_set_dataset's symmetry pass over the uploaded matrices (no
 * extra scan): 1 = every element finite. The caller raises the reference's
 * error ("matrices must not contain NaN/Inf", R/check-user-input.R:796-799). */
int nr_dataset_finite(nr_ctx* ctx, int* corr_finite, int* net_finite);

/* Module index sets (a4 of SURVEY.md 8) and discovery vectors (a15).
 *   n_rows      rows of the output cube = length of `modules`
 *   n_present   modules with >= 1 node in the test dataset (modsPresent,
 *               src/permutations.cpp:196-201), in `modules` order
 *   row_of      [n_present] output row of each present module
 *   node_off    [n_present+1] CSR offsets of module nodes
 *   test_idx    [node_off[n_present]] column of each node in the resident
 *               dataset (GetNodeIdx, src/utils.cpp:147-162); used for the
 *               observed statistics
 *   null_pos    [same] position of each node in the null pool (MakeNullMap
 *               nullMap, src/utils.cpp:108-136); may be NULL if no
 *               permutations will be run
 *   disc_corr   concatenated discovery CorrVector per module, k(k-1)/2 each
 *   disc_degree [nodes] discovery weighted degree (node order)
 *   disc_contrib[nodes] discovery node contribution, NULL for network-only */
int nr_set_modules(nr_ctx* ctx, int32_t n_rows, int32_t n_present,
                   const int32_t* row_of, const int64_t* node_off,
                   const int32_t* test_idx, const int32_t* null_pos,
                   const double* disc_corr, const double* disc_degree,
                   const double* disc_contrib);

/* The null pool nullIdx (MakeNullMap, src/utils.cpp:108-136): test columns. */
int nr_set_null_pool(nr_ctx* ctx, const int32_t* null_idx, int64_t n_null);

/* Observed statistics (src/permutations.cpp:246-285) into observed
 * [n_rows x n_stat], column-major (R matrix), NA_REAL for absent modules and
 * non-finite values (src/permutations.cpp:383-384). n_stat = 7 with data,
 * 4 without. */
int nr_observed(nr_ctx* ctx, double* observed);

/* The same, split so that it runs beside the permutations: nr_observed_async
 * enqueues the observed launch on the context's second stream (its own
 * scratch and work queue) and returns; nr_run / nr_run_device may follow at
 * once, and their first batch shares the GPU with it. nr_observed_wait
 * copies the statistics out (blocking). Any change of dataset, modules or
 * null pool in between waits for the launch and discards it (nr_observed_wait
 * then returns NR_ERR_INVALID). */
int nr_observed_async(nr_ctx* ctx);
int nr_observed_wait(nr_ctx* ctx, double* observed);

/* Null distributions for global permutations [perm_begin, perm_end).
 * pi == NULL: permutation p draws pi_p = keyed PRP(seed, p) (prp.h).
 * pi != NULL: explicit host table [(perm_end-perm_begin) x n_null] of
 *   null-pool permutations, pi[p][q] = source position (the exported
 *   shuffles of the reference, src/permutations.cpp:63). The table must hold
 *   exactly that many entries, each < n_null; an entry >= n_null is rejected
 *   with NR_ERR_INVALID before anything runs (device tables are checked by a
 *   device scan). Module nodes' null_pos (nr_set_modules) must be < n_null
 *   (NR_ERR_INVALID otherwise).
 * Cancellation: nr_cancel (any thread) stops the run in progress -- or the
 *   next one started on ctx -- between launches; it returns NR_ERR_CANCELLED
 *   with every slice not computed set to NA_real_ (the reference's
 *   interrupted workers leave their part of the NA-filled cube,
 *   src/permutations.cpp:375-384).
 * nulls receives (perm_end-perm_begin) slices of n_rows x n_stat, i.e. the
 * cube layout m + n_rows*s + n_rows*n_stat*p of src/permutations.cpp:55
 * starting at permutation perm_begin. Host pointer for nr_run, device pointer
 * for nr_run_device. */
int nr_run(nr_ctx* ctx, int64_t perm_begin, int64_t perm_end, uint64_t seed,
           const uint32_t* pi, double* nulls);
int nr_run_device(nr_ctx* ctx, int64_t perm_begin, int64_t perm_end,
                  uint64_t seed, const uint32_t* pi_device, double* nulls_device);

/* Host evaluation of the keyed null-pool permutation: out[p - perm_begin][q]
 * = pi_p(q) for q < n_null (no GPU needed). */
int nr_prp_table(uint64_t seed, int64_t perm_begin, int64_t perm_end,
                 int64_t n_null, uint32_t* out);

/* Export the index sets a run would use: test column of every module node of
 * permutations [perm_begin, perm_end), layout [perm][node] (CSR node order). */
int nr_export_indices(nr_ctx* ctx, int64_t perm_begin, int64_t perm_end,
                      uint64_t seed, int32_t* indices);

/* Per-module vectors for explicit index sets on the resident dataset
 * (IntermediateProperties src/discProps.cpp:92-122, NetProps
 * src/properties.cpp:152-185): corr_vec (k(k-1)/2 per module), degree (k),
 * avg_weight (one per module, AverageEdgeWeight src/netStats.cpp:154-162),
 * contribution (k), summary (n_samples per module) and coherence (one per
 * module, ModuleCoherence src/netStats.cpp:293-305). Any output may be NULL;
 * the last three need data. Node order = CSR order of idx. */
int nr_module_vectors(nr_ctx* ctx, int32_t n_mod, const int64_t* node_off,
                      const int32_t* idx, double* corr_vec, double* degree,
                      double* avg_weight, double* contribution, double* summary,
                      double* coherence);

/* Column scaling (Scale, src/scale.cpp:14-25) on the device. */
int nr_scale(nr_ctx* ctx, const double* data, int64_t n_samples,
             int64_t n_nodes, double* scaled);

/* CheckFinite (src/checkFinite.cpp:21-28): *all_finite = 1 or 0. */
int nr_check_finite(nr_ctx* ctx, const double* mat, int64_t n_elem, int* all_finite);

/* Progress (replaces MonitorProgress, src/thread-utils.cpp:49-82) and
 * cancellation (replaces the `interrupted` flag, src/permutations.cpp:362);
 * both are safe to call from another host thread during nr_run. */
int nr_progress(nr_ctx* ctx, int64_t* done, int64_t* total);
int nr_cancel(nr_ctx* ctx);

/* Tuning and measurement. */
int nr_set_batch(nr_ctx* ctx, int64_t perms_per_launch);
/* Host threads of the staging copies: the process-wide default for contexts
 * created afterwards (n <= 0: 8; capped at 16), and one context's own count.
 * The reference-interface calls set their contexts' count from n_cores and
 * never change the process default. */
int nr_set_host_threads(int n);
/* The process-wide default set by nr_set_host_threads (pooled contexts are
 * reset to it when a reference-interface call returns them). */
int nr_get_host_threads(void);
int nr_ctx_set_host_threads(nr_ctx* ctx, int n);
/* Host -> device bytes the library has copied since it was loaded (every
 * upload path counts): a caller can verify that resident data is not
 * uploaded again. */
int nr_h2d_bytes(int64_t* bytes);
int nr_set_timing(nr_ctx* ctx, int enable);
/* Accumulated device time (HIP events on the launch stream) per kernel:
 * kernel 0 = module network statistics, 1 = summary-profile statistics. */
int nr_get_timing(nr_ctx* ctx, int kernel, double* total_ms, int64_t* launches,
                  int64_t* items);
int nr_reset_timing(nr_ctx* ctx);
/* Summary-profile eigen-solver counters since the last nr_reset_timing:
 * items solved, Lanczos steps taken, items that reached the step cap, and
 * partial-reorthogonalisation passes performed. */
int nr_get_diagnostics(nr_ctx* ctx, int64_t* eig_items, int64_t* eig_steps,
                       int64_t* eig_cap_hits, int64_t* eig_reorths);
int nr_synchronize(nr_ctx* ctx);
/* Diagnostics: per-phase shader-cycle stamps of the summary-profile kernel,
 * summed over workgroups, 16 slots (0 index, 1 Gram, 2 Lanczos set-up,
 * 3 matvec, 4 three-term step + omega, 5 statistics, 6 q update, 7 Ritz
 * checks, 8 start column, 9 reorthogonalisation, 10 Ritz vector,
 * 11 node contributions, 12 Ritz coefficients, 13 a Ritz check's top
 * eigenvalue, 14 its residual (and the full-precision refinement where the
 * check may end the run; 7 keeps the rest of the check); 15 spare). Off by
 * default; a diagnostic build (make EXTRA=-DNR_STAMPS=1) records them; a run with stamps on
 * is a measurement run, not a timed one. */
int nr_set_stamps(nr_ctx* ctx, int enable);
int nr_get_stamps(nr_ctx* ctx, uint64_t* cycles);

/* Per-batch work buffers (column-sweep sets, profile-slot scratch, device
 * output and shuffle-table buffers): nr_release_scratch frees them (the next
 * run reallocates), nr_scratch_bytes reports what a context holds. The
 * reference-interface layer releases them whenever it pools a context. */
int nr_release_scratch(nr_ctx* ctx);
int nr_scratch_bytes(const nr_ctx* ctx, int64_t* bytes);
/* A context's own host-thread count (nr_ctx_set_host_threads). */
int nr_ctx_get_host_threads(const nr_ctx* ctx, int* n);

/* Test knobs, process-wide. The first two change no result.
 * NR_DEBUG_SWEEP_MAX_OCC: the column sweep's sub-batch bound in occurrences
 * (value <= 0 restores the default, 64M). NR_DEBUG_FAIL_SWEEP_ALLOC: the
 * value-th column-sweep buffer allocation from now fails with NR_ERR_OOM (0:
 * off). NR_DEBUG_SWEEP_CHUNK_ROWS: a positive multiple of 64 caps the rows per
 * column chunk of the sweep in place of the LDS budget's cap (9,984 rows of
 * {corr, net}); the chunks stay balanced and rounded to 64 rows, a value above
 * the budget's cap has no effect, value <= 0 restores the default, any other
 * value returns NR_ERR_INVALID. It regroups the CorrVector partial sums, so
 * cor.cor and avg.cor move at rounding level; avg.weight and cor.degree (exact
 * fixed-point parts, or plain sums cut at other places) move at rounding
 * level at most. Whether the sweep runs at all is decided from the production
 * height; a cap that gives more than 16 chunks makes the run fail with
 * NR_ERR_INVALID instead of taking another kernel. */
#define NR_DEBUG_SWEEP_MAX_OCC 1
#define NR_DEBUG_FAIL_SWEEP_ALLOC 2
#define NR_DEBUG_SWEEP_CHUNK_ROWS 3
int nr_debug_set(int what, int64_t value);

/* ---- reference-interface layer ----------------------------------------- */
/* Names are arrays of NUL-terminated strings. moduleAssignments is the named
 * character vector as (node names, labels). Per-module discovery vectors are
 * given in `modules` order ([n_modules] pointers + lengths; NULL/0 for
 * modules absent from the test dataset). */

typedef struct netrep_disc_props {
  const double* const* degree;        /* [n_modules] */
  const int64_t* degree_len;
  const double* const* corr;
  const int64_t* corr_len;
  const double* const* contribution;  /* NULL for the network-only path */
  const int64_t* contribution_len;
} netrep_disc_props;

/* Interrupt hook: the replacement of checkInterrupt (src/interrupt.cpp:9-11)
 * as polled by MonitorProgress (src/thread-utils.cpp:49-82). While
 * netrep_PermutationProcedure runs, its calling thread polls fn(user) every
 * 100 ms (the engine works on other host threads); a non-zero return cancels
 * every GPU's run. The R glue installs a function that wraps
 * R_ToplevelExec(R_CheckUserInterrupt). NULL removes it.
 * Process-wide; set it before the call. */
typedef int (*netrep_interrupt_fn)(void* user);
void netrep_set_interrupt_hook(netrep_interrupt_fn fn, void* user);

/* Progress hook: the replacement of MonitorProgress's console output
 * (src/thread-utils.cpp:54-81: Rcpp::Rcout << endl, then "\r%5d% completed."
 * about once a second, then endl endl). While netrep_PermutationProcedure or
 * netrep_PermutationProcedureFiles runs with verbose != 0, the CALLING
 * thread -- the thread R called from, so the hook may write to
 * Rcpp::Rcout -- calls fn(event, done, total, user): NETREP_PROGRESS_BEGIN
 * once before the first permutation, NETREP_PROGRESS_UPDATE about once a
 * second and once more when the last permutation completes (done == total),
 * NETREP_PROGRESS_END once after the run (also after an interrupt).
 * netrep_format_progress renders an UPDATE exactly as the reference does.
 * The library itself never writes to stdout or stderr (R CMD check): with no
 * hook installed, verbose output is dropped. NULL removes the hook.
 * Process-wide; set it before the call. */
#define NETREP_PROGRESS_BEGIN 0
#define NETREP_PROGRESS_UPDATE 1
#define NETREP_PROGRESS_END 2
typedef void (*netrep_progress_fn)(int32_t event, int64_t done, int64_t total, void* user);
void netrep_set_progress_hook(netrep_progress_fn fn, void* user);
/* "\r%5d% completed." with the reference's rounding
 * ((unsigned)round((float)done / (float)total * 100), src/thread-utils.cpp:
 * 66-68) into buf (NUL-terminated, at most cap bytes); returns the length
 * written, or -1 if cap is too small. */
int netrep_format_progress(int64_t done, int64_t total, char* buf, int64_t cap);

/* PermutationProcedure (src/permutations.cpp:160-166) and
 * PermutationProcedureNoData (src/permutationsNoData.cpp:140-146, t_data =
 * NULL). nulls_out [n_modules x n_stat x n_perm], observed_out
 * [n_modules x n_stat], both column-major, NA-filled. `seed` keys the PRP;
 * `pi` (optional, [n_perm x n_null]) supplies explicit shuffles. n_cores
 * (nThreads of the reference, which sizes its worker pool) bounds the host
 * threads the call uses for its own work -- the pinned staging copies of the
 * test matrices (at most min(n_cores, 16) threads; n_cores <= 0: 8); the
 * permutations themselves run on the GPUs. NETREP_NUM_GPUS selects the GPU count
 * (NETREP_SHARE_DEVICE=1 lets several contexts share the visible GPUs, a test
 * mode for the sharded path on a one-GPU machine). The test matrices are
 * uploaded once, to the first GPU, and copied device to device to the others.
 * Interrupted (netrep_set_interrupt_hook): returns NR_ERR_CANCELLED with
 * observed_out complete and nulls_out holding every completed permutation,
 * NA_real_ elsewhere -- the partial cube the reference returns
 * (src/permutations.cpp:375-408). */
int netrep_PermutationProcedure(
    const netrep_disc_props* disc_props, const double* t_data,
    const double* t_corr, const double* t_net, int64_t n_samples,
    int64_t n_nodes, const char* const* t_names, const char* const* ma_names,
    const char* const* ma_labels, int64_t n_assign,
    const char* const* modules, int64_t n_modules, int64_t n_perm,
    int32_t n_cores, const char* null_hypothesis, int32_t verbose,
    uint64_t seed, const uint32_t* pi, double* nulls_out, double* observed_out);

/* Pipelining modulePreservation's loop over test datasets
 * (R/modulePreservation.R:553-620, one PermutationProcedure call per test
 * dataset): starts uploading the NEXT test dataset's matrices to GPU 0 in the
 * background (pinned, double-buffered chunks on the copy engine) and returns
 * at once: prefetch dataset t+1, then call netrep_PermutationProcedure on
 * dataset t, and the host->HBM copy of t+1 overlaps t's permutations. The
 * netrep_PermutationProcedure call naming the same three pointers and sizes
 * adopts the uploaded dataset instead of copying it again. At most two
 * prefetches are pending (the oldest is dropped beyond that); the arrays must
 * stay alive and unchanged until adopted or discarded. No reference
 * counterpart (the reference loads one test dataset at a time into RAM). */
int netrep_PrefetchTestDataset(const double* t_data, const double* t_corr, const double* t_net,
                               int64_t n_samples, int64_t n_nodes);
void netrep_DiscardPrefetch(void);

/* PermutationProcedure with the test dataset given as disk.matrix files
 * (R/disk-matrix-class.R; the R code would otherwise loadIntoRAM() them,
 * R/modulePreservation.R:553-620): the files go straight to GPU 0's HBM,
 * tData is scaled there, and the node names are the network file's column
 * names. The three files must agree on the node order: the correlation,
 * network and data files' column names (and the square matrices' row names)
 * must be identical where present, as R/check-user-input.R:757-771 requires
 * ("mismatch in node order between data, correlation, and network"). pi_len
 * is the number of entries in pi (n_perm x n_null, checked once the node
 * names -- hence n_null -- are known; -1: unchecked). Other arguments and
 * outputs as netrep_PermutationProcedure. */
int netrep_PermutationProcedureFiles(const netrep_disc_props* disc_props, const char* t_data_file,
                                     const char* t_corr_file, const char* t_net_file,
                                     const char* const* ma_names, const char* const* ma_labels,
                                     int64_t n_assign, const char* const* modules, int64_t n_modules,
                                     int64_t n_perm, int32_t n_cores, const char* null_hypothesis,
                                     int32_t verbose, uint64_t seed, const uint32_t* pi, int64_t pi_len,
                                     double* nulls_out, double* observed_out);

/* PermutationProcedure with the test dataset given as its data matrix alone
 * (nr_set_dataset_from_data on GPU 0: t_data is uploaded, scaled there when
 * scale_data != 0, and the correlation and network are built in HBM from it
 * by net_type (NR_NET_*, with NR_NET_TOM OR-ed on: the network is the
 * topological overlap of that adjacency; with NR_COR_SPEARMAN or NR_COR_BICOR
 * OR-ed on: the correlation is of that type) and beta; no n x n host matrix exists or crosses
 * PCIe). Built matrices that are not all finite -- a constant column, for
 * which R's cor gives NA -- return NR_ERR_NONFINITE with CheckFinite's
 * message before any permutation runs (the reference stops such input in
 * R/check-user-input.R:796-799). Other arguments, outputs, multi-GPU
 * broadcast, progress, interrupt and the NR_ERR_OOM retry as
 * netrep_PermutationProcedure. */
int netrep_PermutationProcedureFromData(
    const netrep_disc_props* disc_props, const double* t_data, int32_t scale_data, int32_t net_type,
    double beta, int64_t n_samples, int64_t n_nodes, const char* const* t_names,
    const char* const* ma_names, const char* const* ma_labels, int64_t n_assign,
    const char* const* modules, int64_t n_modules, int64_t n_perm, int32_t n_cores,
    const char* null_hypothesis, int32_t verbose, uint64_t seed, const uint32_t* pi,
    double* nulls_out, double* observed_out);

/* The same build, copied back: corr_out and net_out (n_nodes x n_nodes each,
 * either may be NULL) for callers who still need host matrices, e.g. for the
 * discovery-side calls. With NR_NET_TOM in net_type, net_out is the
 * topological overlap matrix. Non-finite results are returned as they are. */
int netrep_BuildNetwork(const double* data, int32_t scale_data, int32_t net_type, double beta,
                        int64_t n_samples, int64_t n_nodes, double* corr_out, double* net_out);

/* WGCNA's scaleFreeFitIndex of one connectivity vector k[n], with R's
 * current cut() binning; a pure host function (no context, no GPU).
 * B = n_breaks >= 3 bins over [min k, max k]: dx = max k - min k, edges
 * e_m = min k + m (dx / B), m = 0 .. B; node i is in bin 1 + #{m in
 * 1 .. B - 1 : k_i > e_m} (right-closed bins; the minimum is in bin 1, the
 * maximum in bin B). Per bin: p_m = count_m / n; d_m = the mean of k in the
 * bin, or (e_{m-1} + e_m) / 2 if the bin is empty or that mean is 0;
 * x_m = log10(d_m), y_m = log10(p_m + 1e-9). remove_first drops bin 1; N
 * bins remain. out3[0] = R^2 = 1 - SSR / SST of the least-squares line
 * y ~ x (SFT.R.sq), out3[1] = its slope, out3[2] = the adjusted R^2
 * 1 - (1 - R^2) (N - 1) / (N - 3) of the least-squares fit y ~ x + d
 * (truncated.R.sq; NaN for N <= 3). dx == 0 or a non-finite k: three NaNs.
 * NR_ERR_INVALID: a NULL pointer, n < 1, n_breaks < 3. */
int netrep_ScaleFreeFit(const double* k, int64_t n, int32_t n_breaks, int32_t remove_first, double* out3);
/* The bin (1 .. n_breaks) of every node under that binning into
 * bins_out[n]; all 0 where netrep_ScaleFreeFit gives NaNs. */
int netrep_ScaleFreeBins(const double* k, int64_t n, int32_t n_breaks, int32_t* bins_out);
/* powerEstimate of a pickSoftThreshold table (n_powers x 7, column-major:
 * Power, SFT.R.sq, slope, ...): the first power, in the table's order, with
 * -sign(slope) SFT.R.sq > rsquared_cut; NaN if none passes (a NaN row does
 * not). A pure host function. */
int netrep_SftPowerEstimate(const double* table, int32_t n_powers, double rsquared_cut, double* power_estimate_out);
/* WGCNA's pickSoftThreshold from the data matrix alone: the connectivities
 * of nr_soft_connectivity on GPU 0 (data raw when scale_data != 0, else
 * scaled already; net_type as there), then per power the fit above and
 * the table row Power, SFT.R.sq, slope, truncated.R.sq, mean.k., median.k.
 * (R's: the mean of the two middle values for even n), max.k. into
 * table_out (n_powers x 7, column-major); *power_estimate_out as
 * netrep_SftPowerEstimate; connectivity_out (optional, n_nodes x n_powers,
 * column-major) receives the connectivities. Connectivities that are not all
 * finite -- a constant column -- return NR_ERR_NONFINITE as the other
 * from-data entries do. Every argument check (those of nr_soft_connectivity,
 * n_breaks >= 3, rsquared_cut not NaN) runs before a context is opened. */
int netrep_PickSoftThreshold(const double* data, int32_t scale_data, int32_t net_type, int64_t n_samples,
                             int64_t n_nodes, const double* powers, int32_t n_powers, double rsquared_cut,
                             int32_t n_breaks, int32_t remove_first, double* table_out,
                             double* power_estimate_out, double* connectivity_out);

/* Host read of one numeric matrix from an RDS file or save() archive (the
 * same reader): dims always; values (column-major, native) into `out` when
 * non-NULL; NUL-separated column names into `colnames` when cap suffices
 * (*colnames_needed = bytes). No GPU involved. */
int netrep_ReadRDSMatrix(const char* path, const char* object, int64_t* nrow, int64_t* ncol, double* out,
                         char* colnames, int64_t colnames_cap, int64_t* colnames_needed);

/* IntermediateProperties[NoData] (src/discProps.cpp:44-48, :171-175).
 * Outputs per module in `modules` order, concatenated; lengths written to
 * *_len (0 for modules absent from the test node list). Buffers must hold
 * sum(k), sum(k(k-1)/2) and sum(k) doubles (k = module size in discovery). */
int netrep_IntermediateProperties(
    const double* d_data, const double* d_corr, const double* d_net,
    int64_t n_samples, int64_t n_nodes, const char* const* d_names,
    const char* const* t_node_names, int64_t n_t_nodes,
    const char* const* ma_names, const char* const* ma_labels,
    int64_t n_assign, const char* const* modules, int64_t n_modules,
    double* degree_out, int64_t* degree_len, double* corr_out,
    int64_t* corr_len, double* contribution_out, int64_t* contribution_len);

/* NetProps[NoData] (src/properties.cpp:41-44, :190-193). data is unscaled
 * (NetProps scales internally, :49). Per module (in `modules` order) with
 * k_all = all module nodes in moduleAssignments order: degree[k_all],
 * contribution[k_all], summary[n_samples], coherence, avg_weight; NA for
 * absent nodes (:133-139). *_len receive k_all per module. */
int netrep_NetProps(const double* data, const double* net, int64_t n_samples,
                    int64_t n_nodes, const char* const* node_names,
                    const char* const* ma_names, const char* const* ma_labels,
                    int64_t n_assign, const char* const* modules,
                    int64_t n_modules, double* degree_out,
                    double* contribution_out, double* summary_out,
                    double* coherence_out, double* avg_weight_out,
                    int64_t* k_all_out);

/* Scale (src/scale.cpp:38-45): the host matrix through the context's pinned
 * staging in ~16 MiB column chunks, scaled on the device, copied back. */
int netrep_Scale(const double* data, int64_t n_samples, int64_t n_nodes,
                 double* scaled_out);

/* CheckFinite (src/checkFinite.cpp:21-28): NR_ERR_NONFINITE with the
 * reference's message if any element is NA/NaN/Inf. */
int netrep_CheckFinite(const double* mat, int64_t nrow, int64_t ncol);

/* Residency across calls of the reference-interface layer (modulePreservation
 * calls IntermediateProperties and PermutationProcedure once per (discovery,
 * test) pair, R/modulePreservation.R:553-635; networkProperties calls NetProps
 * once per pair, R/networkProperties.R:295-302): the discovery dataset of
 * netrep_IntermediateProperties and the dataset of netrep_NetProps stay
 * resident in HBM while later calls name the same host arrays (same
 * pointers and shape, and the same fingerprint of every element, hashed on
 * the process-wide host threads of nr_set_host_threads -- a full pass over
 * the host arrays at memory bandwidth, the price of reuse; a sampled check
 * of 4,096 elements per array runs first, so a changed array skips the full
 * pass); contexts (streams) are pooled across calls, and a pooled context is
 * reset to the defaults (no dataset, no per-batch work buffers, no cancel
 * request, the process-wide host-thread count). A changed array
 * is uploaded again. netrep_ReleaseResident frees all of it (the R glue calls
 * it when modulePreservation / networkProperties return); a
 * netrep_PermutationProcedure call that runs out of device memory releases
 * the resident datasets and retries once before returning NR_ERR_OOM. */
void netrep_ReleaseResident(void);
/* The pooled contexts (idle between calls): how many, the device bytes of
 * per-batch work buffers they hold (0: released), and the range of their
 * host-thread counts (each equals nr_get_host_threads after a call). With
 * no pooled context the thread range is 0, 0. */
int netrep_PoolInfo(int64_t* n_pooled, int64_t* scratch_bytes, int32_t* host_threads_min,
                    int32_t* host_threads_max);

/* A from-data dataset kept resident and used in every role: discovery
 * properties, network properties and the permutation test, with one upload
 * and one build. The handle owns a context on GPU 0 that holds the scaled
 * data and the {correlation, network} built from them
 * (nr_set_dataset_from_data; 16 n^2 + 8 S (n + 2) bytes of HBM, 40 n^2 while a
 * permutation run's Gram table stands in for the pair array), and a copy of
 * the node names. A handle is used by one thread at a time: concurrent calls
 * on one handle are serialised by a mutex in the handle. netrep_ReleaseResident
 * does NOT free live handles (their contexts are not pooled); only
 * netrep_DatasetRelease does. */
typedef struct netrep_dataset netrep_dataset;

/* Build the handle. The argument checks of the other from-data entries run
 * before any context is opened (same messages). net_type takes NR_NET_TOM and
 * the NR_COR_* bits as everywhere else. A correlation or network that is not
 * all finite (a constant column) returns NR_ERR_NONFINITE with CheckFinite's
 * message: no handle is returned and the context goes back to the pool. On
 * NR_ERR_OOM what is held between calls is released (netrep_ReleaseResident)
 * and the build tried once more. n_cores: the host threads of the upload (0:
 * the process-wide count). */
int netrep_DatasetFromData(const double* data, int32_t scale_data, int32_t net_type, double beta,
                           int64_t n_samples, int64_t n_nodes, const char* const* node_names,
                           int32_t n_cores, netrep_dataset** out);
/* Free the dataset; its context goes back to the pool. NULL is a no-op. */
void netrep_DatasetRelease(netrep_dataset* d);
/* Either output may be NULL. */
int netrep_DatasetShape(netrep_dataset* d, int64_t* n_nodes, int64_t* n_samples);
/* The resident matrices copied back (nr_get_dataset_matrices; n_nodes x
 * n_nodes each, either may be NULL), whichever pair layout is resident. */
int netrep_DatasetMatrices(netrep_dataset* d, double* corr_out, double* net_out);
/* netrep_IntermediateProperties with the handle as the discovery dataset: its
 * node names are the discovery names, nothing is uploaded but the module index
 * sets, and contribution is always produced (the handle always has data). */
int netrep_DatasetIntermediateProperties(
    netrep_dataset* d, const char* const* t_node_names, int64_t n_t_nodes,
    const char* const* ma_names, const char* const* ma_labels, int64_t n_assign,
    const char* const* modules, int64_t n_modules, double* degree_out, int64_t* degree_len,
    double* corr_out, int64_t* corr_len, double* contribution_out, int64_t* contribution_len);
/* netrep_NetProps on the handle's network and data (the data as the handle
 * holds them: scaled on the device if it was built with scale_data). */
int netrep_DatasetNetProps(netrep_dataset* d, const char* const* ma_names, const char* const* ma_labels,
                           int64_t n_assign, const char* const* modules, int64_t n_modules,
                           double* degree_out, double* contribution_out, double* summary_out,
                           double* coherence_out, double* avg_weight_out, int64_t* k_all_out);
/* netrep_PermutationProcedureFromData without the build: the handle is the
 * test dataset. The handle's dataset is resident and unchanged afterwards
 * (whichever pair layout the run chose, after a multi-GPU broadcast, an
 * interrupt or an error); the run's per-batch work buffers are freed. */
int netrep_DatasetPermutationProcedure(
    const netrep_disc_props* disc_props, netrep_dataset* d, const char* const* ma_names,
    const char* const* ma_labels, int64_t n_assign, const char* const* modules, int64_t n_modules,
    int64_t n_perm, int32_t n_cores, const char* null_hypothesis, int32_t verbose, uint64_t seed,
    const uint32_t* pi, double* nulls_out, double* observed_out);

/* The gene dendrogram of the handle's network as R's hclust object:
 * nr_hclust_average on the handle's context (the definition is there), then
 * netrep_HclustFinish. merge [(n - 1) x 2, column-major], height [n - 1],
 * order [n]; n_repairs may be NULL. While it runs the calling thread polls
 * the interrupt hook every 100 ms (NR_ERR_CANCELLED, between launches); the
 * handle's dataset is unchanged and no per-batch buffer remains. */
int netrep_DatasetHclust(netrep_dataset* d, int32_t* merge, double* height, int32_t* order, int32_t* n_repairs);
/* Discovery order (nr_hclust_average's id_lo, id_hi, height) to R's hclust
 * components; a pure host function (no context, no GPU).
 *   - Monotone repair, in discovery order: h_t = max(h_t, h of each child
 *     cluster). A no-op unless heights tie to rounding level; *n_repairs
 *     (optional) counts the steps it raised.
 *   - Stable sort by height: ties keep discovery order, so children always
 *     precede parents.
 *   - merge: singleton i becomes -(i + 1), the cluster of sorted step s
 *     becomes s + 1; within a row two singletons stand in increasing node
 *     index, a singleton before a cluster, two clusters in increasing step.
 *   - order (1-based): the last merge expanded recursively, the first
 *     column's leaves before the second's, as R derives it.
 *   - height: the sorted heights.
 * n = 1: merge and height are empty, order = {1}. NR_ERR_INVALID: a NULL
 * pointer (id_lo, id_hi, height, merge may be NULL when n = 1), n < 1 or
 * > 2^30, a NaN height, ids that are not a binary tree in construction
 * order (each id below n + t at step t, each a child exactly once). */
int netrep_HclustFinish(int64_t n, const int32_t* id_lo, const int32_t* id_hi, const double* height_in,
                        int32_t* merge, double* height, int32_t* order, int32_t* n_repairs);
/* A static cut of such a tree into module labels, after WGCNA's
 * cutreeStatic(dendro, cutHeight, minSize); a pure host function. WGCNA is
 * not consulted: these rules are the contract.
 *   - Every merge with height <= cut_height is applied.
 *   - The resulting clusters are numbered by first appearance in node order
 *     (R's cutree).
 *   - Clusters with fewer than min_size nodes get label 0.
 *   - The rest are renumbered 1, 2, ... by decreasing size; ties go to the
 *     lower cutree number.
 * labels [n]. NR_ERR_INVALID: a NULL pointer, n < 1, a NaN, or a merge
 * matrix whose rows refer to anything but nodes and earlier rows, once each. */
int netrep_CutreeStatic(int64_t n, const int32_t* merge, const double* height, double cut_height,
                        int64_t min_size, int32_t* labels);

/* What follows a cut: eigengenes, module membership, the merging of close
 * modules and the kME trimming. Neither R nor WGCNA is consulted: these rules
 * are the contract. Labels are int32 [n_nodes] in the dataset's node order, 0
 * unassigned, positive values modules (what netrep_CutreeStatic writes);
 * "modules" are the distinct positive labels in increasing order, M of them.
 *
 * The eigengene tree (netrep_EigengeneGroups; a pure host function). eig
 * [S x M, column-major].
 *   - c = cor(E), Pearson over samples: each column's mean (its sum in sample
 *     order over S), the centred values z, their sum of squares ss, and
 *     c_ab = sum_s z_sa z_sb / sqrt(ss_a ss_b) clamped to [-1, 1]; d = 1 - c.
 *     Every product, sum, division and root is rounded to fp64 on its own.
 *   - Average linkage by the Lance-Williams update of nr_hclust_average,
 *     d(k, a u b) = (s_a d(k, a) + s_b d(k, b)) / (s_a + s_b), never fused.
 *   - Each step merges the globally closest pair of clusters; a cluster is
 *     indexed by its lowest column, and ties go to the lowest (lower index,
 *     higher index) pair. height_out [M - 1]: the heights in merge order.
 *   - Groups: the clusters left after every merge with height <= cut_height.
 *     group_out [M]: the 0-based index of the first column of each column's
 *     group.
 * M = 1: one group, no height. NR_ERR_INVALID: a NULL pointer, S < 2, M < 1,
 * cut_height outside [0, 2] or NaN, a non-finite or constant column. */
int netrep_EigengeneGroups(const double* eig, int64_t n_samples, int64_t n_mod, double cut_height,
                           int32_t* group_out, double* height_out);
/* One merge step (a pure host function): every node of module
 * module_labels[m] gets the label module_labels[group[m]], the label of the
 * first module of its group (under netrep_CutreeStatic's numbering the lowest
 * label and hence the largest module); 0 never changes. relabel != 0: the
 * surviving modules are then renumbered 1, 2, ... by decreasing size, ties to
 * the lower old label. labels_out may be labels_in. NR_ERR_INVALID: a NULL
 * pointer, a negative label, a positive label missing from module_labels, a
 * module label that is not positive or given twice, group[m] outside 0 .. m. */
int netrep_MergeLabels(int64_t n, const int32_t* labels_in, int64_t n_mod, const int32_t* module_labels,
                       const int32_t* group, int32_t relabel, int32_t* labels_out);
/* The kME trimming of WGCNA's blockwiseModules, in-module kME only, one pass,
 * no relabelling (a pure host function). kme_own [n]: each node's correlation
 * with its own module's eigengene (ignored for label 0). Per module:
 *   - fewer than min_core_kme_size nodes with kme_own > min_core_kme: the
 *     whole module goes to 0 (min_core_kme_size < 0: the default, min_size / 3,
 *     as a count: rounded up);
 *   - otherwise its nodes with kme_own < min_kme_to_stay go to 0;
 *   - a module then left with fewer than min_size nodes goes to 0.
 * WGCNA's defaults are 0.3, 0.5 and min_size / 3. Its reassignment by kME
 * p-value (reassignThreshold) is not offered. NR_ERR_INVALID: a NULL pointer,
 * n < 1, a negative label, a NaN threshold. */
int netrep_TrimModulesKME(int64_t n, const int32_t* labels_in, const double* kme_own, double min_kme_to_stay,
                          double min_core_kme, int64_t min_core_kme_size, int64_t min_size, int32_t* labels_out);
/* On the handle. Common to the netrep_Dataset* entries below, down to
 * netrep_DatasetTrimModules: labels [n_nodes] as above;
 * NR_ERR_INVALID with a text naming it for a NULL argument, a negative
 * label, or a label vector with no positive label; the interrupt hook is
 * polled before every device call (NR_ERR_CANCELLED); the handle's dataset
 * is unchanged and no per-batch buffer remains.
 * The eigengenes are those of the data as the handle holds them: WGCNA's
 * moduleEigengenes for a handle built with scale_data, the unscaled data's
 * otherwise.
 * netrep_DatasetModuleEigengenes: nr_module_eigengenes of the label vector's
 * modules. n_mod_out and module_labels_out [M] (optional), eigengenes
 * [S x M, column-major], var_explained [M], kme_own [n_nodes] in node order
 * (optional; NA for label 0). The caller sizes the outputs by its own count
 * of distinct positive labels. */
int netrep_DatasetModuleEigengenes(netrep_dataset* d, const int32_t* labels, int32_t* n_mod_out,
                                   int32_t* module_labels_out, double* eigengenes, double* var_explained,
                                   double* kme_own);
/* The module-membership table: the eigengenes as above, then
 * nr_module_membership on the context's copy of them. kme [n_nodes x M,
 * column-major]. */
int netrep_DatasetModuleMembership(netrep_dataset* d, const int32_t* labels, double* kme);
/* The eigengene tree itself (a pure host function): the tree that
 * netrep_EigengeneGroups cuts -- the same cor(E), the same "globally closest
 * pair, ties to the lowest (lower, higher) pair" rule, clusters indexed by
 * their lowest column -- with the linkage chosen: NR_LINKAGE_AVERAGE (the
 * bits of netrep_EigengeneGroups' heights) or NR_LINKAGE_COMPLETE,
 * d(k, a u b) = max(d(k, a), d(k, b)), R's hclust default. It emits the
 * merges as nr_hclust_average does, in discovery order, for
 * netrep_HclustFinish: step t = 0 .. M - 2 gives id_lo[t], id_hi[t] (the ids
 * of the clusters with the lower and the higher lowest column: 0 .. M - 1
 * are columns, M + u is the cluster of step u) and height[t]. M = 1 writes
 * nothing. NR_ERR_INVALID: a NULL pointer (the outputs may be NULL when
 * M = 1), S < 2, M < 1, an unknown linkage, a non-finite or constant column. */
#define NR_LINKAGE_AVERAGE 0
#define NR_LINKAGE_COMPLETE 1
int netrep_EigengeneTree(const double* eig, int64_t n_samples, int64_t n_mod, int32_t linkage, int32_t* id_lo,
                         int32_t* id_hi, double* height);
/* Connectivity by module, the network-side counterpart of the kME table.
 * slot[j] is node j's module index 0 .. M - 1 among the distinct positive
 * labels in increasing order, or -1 for label 0; the table and the summation
 * order are nr_module_connectivity's (the definition is there).
 * netrep_DatasetModuleConnectivity: k_total [n_nodes] (optional) and k_mod
 * [n_nodes x M, column-major] of the handle's network; conventions as the
 * other label entries on the handle. */
int netrep_DatasetModuleConnectivity(netrep_dataset* d, const int32_t* labels, double* k_total, double* k_mod);
/* WGCNA's intramodularConnectivity from that table (a pure host function;
 * k_total [n], k_mod [n x M, column-major] as above):
 *   k_within[i] = k_mod[i, slot[i]], k_out = k_total - k_within,
 *   k_diff = k_within - k_out, each one rounding; NaN all three for label 0.
 * NR_ERR_INVALID: a NULL pointer, n < 1, a negative label, no positive label. */
int netrep_IntramodularConnectivity(int64_t n, const int32_t* labels, const double* k_total, const double* k_mod,
                                    double* k_within, double* k_out, double* k_diff);
/* Both on the handle: the four vectors [n_nodes] of its network. */
int netrep_DatasetIntramodularConnectivity(netrep_dataset* d, const int32_t* labels, double* k_total,
                                           double* k_within, double* k_out, double* k_diff);
/* WGCNA's mergeCloseModules with iterate = TRUE. A round computes the
 * eigengenes of the current labels, builds their tree, cuts it at cut_height
 * (netrep_EigengeneGroups) and merges (netrep_MergeLabels, no relabelling);
 * rounds repeat until one merges nothing or one module is left: at most
 * M - 1 rounds merge. *n_rounds_out: the rounds that merged something.
 * relabel != 0: the final labels go through the renumbering by size.
 * The last round (the one that merged nothing, on the final modules) is
 * reported through the optional outputs: *n_mod_last_out the final module
 * count M', eigengenes_last_out [S x M', at most S x M], its columns in the
 * order of the returned labels' modules, heights_last_out [M' - 1, at most
 * M - 1] its tree's heights (all above cut_height).
 * NR_ERR_INVALID also for cut_height outside [0, 2] or NaN. */
int netrep_DatasetMergeCloseModules(netrep_dataset* d, const int32_t* labels_in, double cut_height, int32_t relabel,
                                    int32_t* labels_out, int32_t* n_rounds_out, int32_t* n_mod_last_out,
                                    double* eigengenes_last_out, double* heights_last_out);
/* netrep_TrimModulesKME with kme_own from the handle (netrep_DatasetModuleEigengenes). */
int netrep_DatasetTrimModules(netrep_dataset* d, const int32_t* labels_in, double min_kme_to_stay,
                              double min_core_kme, int64_t min_core_kme_size, int64_t min_size, int32_t* labels_out);

/* One-shots for glue whose call sites are separate: build the handle, make
 * the one call, release it. */
int netrep_IntermediatePropertiesFromData(
    const double* d_data, int32_t scale_data, int32_t net_type, double beta, int64_t n_samples,
    int64_t n_nodes, const char* const* d_names, const char* const* t_node_names, int64_t n_t_nodes,
    const char* const* ma_names, const char* const* ma_labels, int64_t n_assign,
    const char* const* modules, int64_t n_modules, double* degree_out, int64_t* degree_len,
    double* corr_out, int64_t* corr_len, double* contribution_out, int64_t* contribution_len);
int netrep_NetPropsFromData(const double* data, int32_t scale_data, int32_t net_type, double beta,
                            int64_t n_samples, int64_t n_nodes, const char* const* node_names,
                            const char* const* ma_names, const char* const* ma_labels, int64_t n_assign,
                            const char* const* modules, int64_t n_modules, double* degree_out,
                            double* contribution_out, double* summary_out, double* coherence_out,
                            double* avg_weight_out, int64_t* k_all_out);

/* Last error of the reference-interface layer (thread-local). */
const char* netrep_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* NETREP_GPU_H */
