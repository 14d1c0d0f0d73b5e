// Shared by engine.hip (planning, launches, modules, null pool, scratch,
// timing) and dataset.hip (everything that makes a dataset resident): the
// context, its resident Dataset, and the error / allocation / upload helpers.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/netrep_gpu.h"

struct DeviceTimer {
  double ms = 0.0;
  int64_t launches = 0;
  int64_t items = 0;
};

// The resident dataset of a context. Every field is reset by assigning a
// default-constructed Dataset (reset_dataset) and carried to a copy by
// copy_dataset_fields, so a field added here needs no other bookkeeping.
struct Dataset {
  double2* d_pairs = nullptr;
  double* d_colsum = nullptr;    // [n_nodes] column sums of the data (Gram table)
  double* d_data = nullptr;
  int32_t pairs_es = 1;          // d_pairs element stride in double2: 2 = the Gram table layout
  int64_t n_nodes = 0, n_samples = 0;
  std::vector<std::string> node_names;  // column names of a dataset loaded from files
  int symmetric = 0;
  int corr_finite = 0, net_finite = 0;  // CheckFinite of the resident matrices
  double table_ms = 0.0;         // wall time of the last Gram-table build
  double netbuild_ms = 0.0;      // device time of the from-data build of the matrices (0: not built from data)
  double tom_ms = 0.0;           // device time of the TOM step behind it (0: built without NR_NET_TOM)
  double cor_ms = 0.0;           // device time of the correlation-type transform ahead of it (0: Pearson)
};

struct nr_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  std::string err;
  std::mutex mu;
  int host_threads = 8;  // host threads of this context's staging copies (nr_ctx_set_host_threads)

  Dataset ds;
  // nr_soft_connectivity (it touches nothing of the resident dataset)
  double sft_ms = 0.0;           // device time of the last call's kernels (0: none yet)
  int sft_finite = 1;            // the last call's connectivities were all finite
  int sft_row_groups = 0;        // nr_set_sft_row_groups (0: the default, nr::sft_row_groups(n))
  // nr_hclust_average (it reads the resident net once and writes nothing resident)
  int64_t hclust_merges = 0;     // nr_set_hclust_merges_per_launch (0: the default, nr::kHclustMergesPerLaunch)
  double hclust_ms = 0.0;        // device time of the last call's extract and chain launches
  int64_t hclust_searches = 0, hclust_launches = 0, hclust_scratch = 0;  // of the last call (nr_hclust_info)
  // nr_module_eigengenes / nr_module_membership (they write nothing resident)
  double* d_eig = nullptr;       // [S x eig_n_mod] the last nr_module_eigengenes call's eigengenes (scratch)
  size_t eig_cap = 0;
  int32_t eig_n_mod = 0;         // 0: none
  int64_t eig_gen = -1;          // data_gen they were computed for
  double membership_ms = 0.0;    // device time of the last nr_module_membership call's two kernels
  // nr_module_connectivity (it reads the resident net and writes nothing resident)
  double connectivity_ms = 0.0;  // device time of the last call's kernels
  int32_t connectivity_tile = 0; // nr_set_connectivity_module_tile (0: the default, nr::connectivity_tile(M))
  int64_t table_checked = -1;   // modules_serial the Gram-table decision was made for
  int64_t data_gen = 0;          // bumped by every dataset change (reset_dataset)
  int64_t modules_gen = -1;      // data_gen the modules were validated against
  int64_t modules_serial = 0;    // bumped by every nr_set_modules
  int64_t null_gen = -1;         // data_gen the null pool was validated against
  int disc_cv_finite = 0;        // the present modules' discovery CorrVector is all finite

  // modules
  int32_t n_rows = 0, n_present = 0, k_max = 0;
  int64_t n_node_total = 0, n_cv_total = 0;
  int64_t null_pos_max = -1;  // largest null-pool position of any module node (-1: none)
  std::vector<int64_t> node_off_h, cv_off_h;
  int32_t* d_row_of = nullptr;
  int64_t* d_node_off = nullptr;
  int64_t* d_cv_off = nullptr;
  int32_t* d_test_idx = nullptr;
  int32_t* d_null_pos = nullptr;
  double* d_disc_cv = nullptr;
  double* d_disc_wd = nullptr;
  double* d_disc_nc = nullptr;
  double* d_cv_shift = nullptr;
  int32_t* d_mod_order = nullptr;
  std::vector<int32_t> order_k_h;  // module sizes in d_mod_order's order (descending)

  // null pool
  int32_t* d_null_idx = nullptr;
  int64_t n_null = 0;

  // run buffers
  double* d_out = nullptr;
  size_t out_cap = 0;
  double* h_stage = nullptr;
  size_t stage_cap = 0;
  uint32_t* d_pi = nullptr;
  size_t pi_cap = 0;
  double* d_scratch = nullptr;
  size_t scratch_cap = 0;
  double* d_net_scratch = nullptr;  // per-workgroup node arrays of modules too large for LDS
  size_t net_scratch_cap = 0;
  int* d_counters = nullptr;  // [0] queue head, [1..4] lanczos diagnostics, [5] flag
  int64_t batch = 0;          // 0 = automatic
  // the second output / staging buffer of run_impl's two batches in flight
  double* d_out2 = nullptr;
  size_t out2_cap = 0;
  double* h_stage2 = nullptr;
  size_t stage2_cap = 0;
  double* h_scale = nullptr;  // nr_scale's pinned staging (4 column chunks)
  size_t scale_cap = 0;
  double* d_scale = nullptr;  // and its device chunks (kept between calls, released as scratch)
  size_t d_scale_cap = 0;
  hipEvent_t ev_copy[2] = {nullptr, nullptr};

  // The observed statistics' own lane (nr_observed_async): stream, scratch and
  // work queue, so that they run beside the first permutation batch instead
  // of ahead of it (at C5 the one-item-per-module launch held the GPU ~85 ms
  // per PermutationProcedure call with 40 workgroups busy).
  hipStream_t obs_stream = nullptr;
  double* obs_scratch = nullptr;
  size_t obs_scratch_cap = 0;
  double* obs_net_scratch = nullptr;
  size_t obs_net_cap = 0;
  int* obs_counters = nullptr;
  double* d_obs = nullptr;
  size_t obs_cap = 0;
  bool obs_pending = false;  // cleared by every change of dataset, modules or null pool

  // the column sweep's per-batch work buffers (sweep.hip), one set per lane
  struct SweepBuf {
    int32_t *col = nullptr, *rank = nullptr, *lrank = nullptr, *count = nullptr, *col_off = nullptr;
    uint32_t *sorted = nullptr, *bndh = nullptr;
    uint4* meta = nullptr;
    double *rec = nullptr, *dabs = nullptr;
    double* zs = nullptr;  // [4] zeros + [256] sink (sweep.hip: lanes with nothing to load / store)
    size_t occ_cap = 0, col_cap = 0;
    int32_t chunk_cap = 0;
  } sweep[2];

  std::atomic<int64_t> done{0}, total{0};
  std::atomic<bool> cancel{false};

  bool timing = false;
  unsigned long long* d_stamps = nullptr;  // phase stamps (nr_set_stamps)
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  bool ev_pending[2] = {false, false};
  DeviceTimer timers[2];
};

static inline int fail(nr_ctx* ctx, int code, const std::string& msg) {
  if (ctx) ctx->err = msg;
  return code;
}

static inline int hip_fail(nr_ctx* ctx, hipError_t e, const char* what) {
  return fail(ctx, e == hipErrorOutOfMemory ? NR_ERR_OOM : NR_ERR_HIP,
              std::string(what) + ": " + hipGetErrorString(e));
}

#define NR_HIP(ctx, call)                              \
  do {                                                 \
    hipError_t e_ = (call);                            \
    if (e_ != hipSuccess) return hip_fail(ctx, e_, #call); \
  } while (0)

template <typename T>
static void dfree(T*& p) {
  if (p) (void)hipFree((void*)p);
  p = nullptr;
}

// Host -> device bytes moved by the library since it was loaded (nr_h2d_bytes):
// every upload path adds what it copies, so a caller can check that a
// resident dataset is not uploaded again. Defined in dataset.hip.
extern std::atomic<int64_t> g_h2d_bytes;

// Every host -> device copy of the library goes through here (counted).
static inline hipError_t h2d_async(void* dst, const void* src, size_t bytes, hipStream_t st) {
  g_h2d_bytes.fetch_add((int64_t)bytes);
  return hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st);
}

template <typename T>
static int ensure(nr_ctx* ctx, T*& buf, size_t& cap, size_t n) {
  if (n <= cap && buf) return NR_OK;
  dfree(buf);
  NR_HIP(ctx, hipMalloc((void**)&buf, n * sizeof(T)));
  cap = n;
  return NR_OK;
}

static inline int ensure_stage(nr_ctx* ctx, double*& h, size_t& cap, size_t n) {
  if (n <= cap && h) return NR_OK;
  if (h) (void)hipHostFree(h);
  h = nullptr;
  NR_HIP(ctx, hipHostMalloc((void**)&h, n * sizeof(double), hipHostMallocDefault));
  cap = n;
  return NR_OK;
}

// Wait for an observed launch still running on the second lane (before its
// inputs are replaced or freed) and drop its result: nr_observed_wait then
// refuses until nr_observed_async is called again.
static inline void sync_obs(nr_ctx* ctx) {
  if (ctx->obs_stream) (void)hipStreamSynchronize(ctx->obs_stream);
  ctx->obs_pending = false;
}

// dataset.hip. No dataset: buffers freed, shape zero. Modules validated
// against an earlier dataset (their node indices) stop being usable:
// check_ready demands a new nr_set_modules after any dataset change.
void reset_dataset(nr_ctx* ctx);

// engine.hip. Explicit module index sets (CSR) checked against the resident
// dataset and uploaded, with the modules' order by decreasing size: what
// nr_module_vectors and nr_module_eigengenes launch their kernels on. The
// device arrays live as long as the object.
struct ModuleSets {
  int64_t* d_off = nullptr;
  int32_t* d_idx = nullptr;
  int32_t* d_order = nullptr;
  std::vector<int32_t> order;     // the host copy behind d_order (alive while the upload may run)
  std::vector<int32_t> k_sorted;  // module sizes in d_order's order
  int32_t k_max = 0;
  int64_t nodes = 0;
  ModuleSets() = default;
  ModuleSets(const ModuleSets&) = delete;
  ModuleSets& operator=(const ModuleSets&) = delete;
  ~ModuleSets() {
    dfree(d_off);
    dfree(d_idx);
    dfree(d_order);
  }
};
int upload_module_sets(nr_ctx* ctx, int32_t n_mod, const int64_t* node_off, const int32_t* idx, ModuleSets& ms);
// The summary-profile launches of those sets on the context's main lane:
// d_sp [n_mod x S], d_nc [nodes], d_coh [n_mod], all device arrays.
int launch_module_profiles(nr_ctx* ctx, const ModuleSets& ms, double* d_sp, double* d_nc, double* d_coh);

// engine.hip. Copy n doubles with up to `threads` host threads (pageable ->
// pinned staging).
void parallel_copy(double* dst, const double* src, int64_t n, int threads,
                   int64_t min_part = (int64_t)1 << 20 /* 8 MiB per thread at least */);
