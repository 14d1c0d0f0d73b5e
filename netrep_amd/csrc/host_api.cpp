// Reference-interface layer of the C ABI (netrep_* in include/netrep_gpu.h).
//
// Mirrors NetRep's eight Rcpp entry points (src/RcppExports.cpp:131-146):
// name maps and index derivation are restated from src/utils.cpp, the driver
// logic from src/permutations.cpp, src/permutationsNoData.cpp,
// src/discProps.cpp, src/properties.cpp, src/scale.cpp and
// src/checkFinite.cpp. All arithmetic on matrices runs on the GPU through the
// engine layer; this file only resolves names to index sets, moves buffers and
// shards permutations over GPUs (one host thread + context per GPU, replacing
// the std::thread pool of src/permutations.cpp:334-380).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include "../../include/netrep_gpu.h"
#include "hclust_host.h"
#include "modmerge_host.h"
#include "rds_reader.h"
#include "sft_fit.h"

namespace {

thread_local std::string g_err;

int set_err(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

int ctx_err(int code, nr_ctx* ctx) {
  g_err = nr_last_error(ctx);
  return code;
}

typedef std::unordered_map<std::string, int64_t> NameMap;

// MakeIdxMap (src/utils.cpp:5-11).
NameMap make_idx_map(const char* const* names, int64_t n) {
  NameMap m;
  m.reserve((size_t)n * 2);
  for (int64_t i = 0; i < n; ++i) m[names[i]] = i;
  return m;
}

// MakeModMap (src/utils.cpp:21-65): label -> node names. Node order inside a
// module is the order of appearance in moduleAssignments (the reference's
// Boost multimap order is implementation-defined; see oracle/netrep_oracle.py).
struct ModMap {
  std::unordered_map<std::string, std::vector<std::string>> nodes;
  const std::vector<std::string>* find(const std::string& label) const {
    auto it = nodes.find(label);
    return it == nodes.end() ? nullptr : &it->second;
  }
};

ModMap make_mod_map(const char* const* ma_names, const char* const* ma_labels, int64_t n,
                    const NameMap* present_in) {
  ModMap mm;
  for (int64_t i = 0; i < n; ++i) {
    if (present_in && present_in->find(ma_names[i]) == present_in->end()) continue;
    mm.nodes[ma_labels[i]].push_back(ma_names[i]);
  }
  return mm;
}

struct CtxDeleter {
  void operator()(nr_ctx* c) const { nr_ctx_destroy(c); }
};
typedef std::unique_ptr<nr_ctx, CtxDeleter> CtxPtr;

// Contexts are pooled across calls (streams, events, slot scratch and
// staging buffers survive; the dataset does not): modulePreservation makes
// one PermutationProcedure call per (discovery, test) pair.
std::mutex g_pool_mu;
struct Pooled {
  int device;
  CtxPtr ctx;
};
// at process exit the pooled contexts are left to the driver's teardown (the
// HIP runtime may already be gone), as the prefetch contexts are
struct Pool {
  std::vector<Pooled> v;
  ~Pool() {
    for (Pooled& p : v) (void)p.ctx.release();
  }
};
Pool g_pool_;
std::vector<Pooled>& g_pool = g_pool_.v;
std::unordered_map<const nr_ctx*, int> g_ctx_device;  // device of every context this layer opened
constexpr size_t kPoolMax = 8;

int open_ctx(int device, CtxPtr& out) {
  {
    std::lock_guard<std::mutex> lk(g_pool_mu);
    for (size_t i = 0; i < g_pool.size(); ++i) {
      if (g_pool[i].device == device) {
        out = std::move(g_pool[i].ctx);
        g_pool.erase(g_pool.begin() + (long)i);
        return NR_OK;
      }
    }
  }
  nr_ctx* c = nullptr;
  const int rc = nr_ctx_create(device, &c);
  if (rc) return set_err(rc, nr_last_error(nullptr));
  out.reset(c);
  std::lock_guard<std::mutex> lk(g_pool_mu);
  g_ctx_device[c] = device;
  return NR_OK;
}

// Back to the pool without its dataset or its per-batch work buffers (HBM is
// not held between calls).
void give_ctx(CtxPtr& c) {
  if (!c) return;
  std::lock_guard<std::mutex> lk(g_pool_mu);
  auto it = g_ctx_device.find(c.get());
  // nr_clear_dataset also clears a pending cancellation (the
  // progress monitor cancels every context of a call, including ones whose
  // run had already returned); the host-thread count goes back to the
  // process default, so the next call's staging does not inherit nCores
  if (it == g_ctx_device.end() || g_pool.size() >= kPoolMax || nr_clear_dataset(c.get()) != NR_OK ||
      nr_release_scratch(c.get()) != NR_OK || nr_ctx_set_host_threads(c.get(), nr_get_host_threads()) != NR_OK) {
    if (it != g_ctx_device.end()) g_ctx_device.erase(it);
    c.reset();
    return;
  }
  g_pool.push_back({it->second, std::move(c)});
}

// Returns every context of a call to the pool when it goes out of scope;
// with `keep`, the first one (the primary, which holds a dataset handle's
// dataset) goes back to its owner as it is instead.
struct CtxLease {
  std::vector<CtxPtr>* v;
  CtxPtr* keep = nullptr;
  ~CtxLease() {
    if (keep && !v->empty() && (*v)[0]) *keep = std::move((*v)[0]);
    for (CtxPtr& c : *v) give_ctx(c);
  }
};

// A dataset kept resident between calls that name the same host arrays: the
// pointers and shape must match, and so must a fingerprint of EVERY element of
// each array (a sampled fingerprint missed in-place edits between
// the sample points, and R's temporaries reuse freed addresses). One host pass
// at memory bandwidth, split over the process's staging threads; each element
// is mixed with its position, so a changed, moved or swapped element changes
// the sum (a 64-bit sum of position-keyed multiplicative mixes).
uint64_t fp_chunk(const double* a, int64_t i0, int64_t i1) {
  uint64_t h = 0;
  for (int64_t i = i0; i < i1; ++i) {
    uint64_t b;
    std::memcpy(&b, a + i, 8);
    uint64_t x = b ^ ((uint64_t)i * 0x9E3779B97F4A7C15ull);
    x ^= x >> 31;
    x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 29;
    h += x;
  }
  return h;
}
uint64_t fingerprint(const double* a, int64_t n) {
  uint64_t h = 0x243F6A8885A308D3ull ^ (uint64_t)n;
  if (!a || n <= 0) return h;
  const int64_t per = 1 << 22;  // 32 MiB per task
  const int nt = (int)std::min<int64_t>(std::max(1, nr_get_host_threads()), (n + per - 1) / per);
  std::vector<uint64_t> part((size_t)nt, 0);
  auto body = [&](int t) {
    const int64_t i0 = n * t / nt, i1 = n * (t + 1) / nt;
    part[(size_t)t] = fp_chunk(a, i0, i1);
  };
  std::vector<std::thread> th;
  for (int t = 1; t < nt; ++t) th.emplace_back(body, t);
  body(0);
  for (auto& x : th) x.join();
  for (uint64_t v : part) h += v;
  return h;
}

// A cheap first look: 4,096 evenly spaced elements of the array (first and
// last included). A changed array usually fails here, and then the full hash
// is not computed at all; a match still needs the full hash.
uint64_t sampled_fingerprint(const double* a, int64_t n) {
  uint64_t h = 0x13198A2E03707344ull ^ (uint64_t)n;
  if (!a || n <= 0) return h;
  const int64_t m = std::min<int64_t>(n, 4096);
  for (int64_t t = 0; t < m; ++t) {
    const int64_t i = m == 1 ? 0 : (int64_t)((__int128)t * (n - 1) / (m - 1));
    h += fp_chunk(a + i, 0, 1) * (uint64_t)(2 * t + 1);
  }
  return h;
}

struct Resident {
  CtxPtr ctx;
  const double *data = nullptr, *corr = nullptr, *net = nullptr;
  int64_t n_samples = 0, n_nodes = 0;
  uint64_t fp = 0, sfp = 0;
  static uint64_t fp_of(const double* data, const double* corr, const double* net, int64_t s, int64_t n) {
    return fingerprint(corr, n * n) * 3 + fingerprint(net, n * n) * 5 + fingerprint(data, s * n) * 7;
  }
  static uint64_t sfp_of(const double* data, const double* corr, const double* net, int64_t s, int64_t n) {
    return sampled_fingerprint(corr, n * n) * 3 + sampled_fingerprint(net, n * n) * 5 +
           sampled_fingerprint(data, s * n) * 7;
  }
  bool holds(const double* d, const double* c, const double* nt, int64_t s, int64_t n) const {
    if (!(ctx && data == d && corr == c && net == nt && n_nodes == n && (d == nullptr || n_samples == s))) return false;
    const int64_t ss = d ? s : 0;
    return sfp == sfp_of(d, c, nt, ss, n) && fp == fp_of(d, c, nt, ss, n);
  }
  void keep(CtxPtr c, const double* d, const double* cr, const double* nt, int64_t s, int64_t n) {
    ctx = std::move(c);
    data = d;
    corr = cr;
    net = nt;
    n_samples = d ? s : 0;
    n_nodes = n;
    fp = fp_of(d, cr, nt, n_samples, n);
    sfp = sfp_of(d, cr, nt, n_samples, n);
  }
  void drop() {
    give_ctx(ctx);
    data = corr = net = nullptr;
    n_samples = n_nodes = 0;
  }
  ~Resident() { (void)ctx.release(); }  // process exit: as Pool
};
std::mutex g_res_mu;
Resident g_disc_res;   // netrep_IntermediateProperties' discovery dataset
Resident g_props_res;  // netrep_NetProps' dataset (net + data scaled on the device)

// Contexts requested by NETREP_NUM_GPUS, clamped to the visible GPUs unless
// NETREP_SHARE_DEVICE=1 (test mode: contexts share GPUs round-robin, so the
// sharded chunk/merge path runs on a one-GPU machine).
int gpu_count_requested(int* avail_out) {
  int avail = 0;
  nr_device_count(&avail);
  *avail_out = std::max(avail, 1);
  int want = 1;
  if (const char* e = std::getenv("NETREP_NUM_GPUS")) want = std::max(1, std::atoi(e));
  const char* share = std::getenv("NETREP_SHARE_DEVICE");
  if (share && std::atoi(share) != 0) return std::min(want, 64);
  return std::max(1, std::min(want, avail));
}

// checkInterrupt replacement (netrep_set_interrupt_hook).
std::mutex g_hook_mu;
netrep_interrupt_fn g_hook = nullptr;
void* g_hook_user = nullptr;

// MonitorProgress's console output replacement (netrep_set_progress_hook).
netrep_progress_fn g_progress = nullptr;
void* g_progress_user = nullptr;

void progress_event(int32_t ev, int64_t done, int64_t total) {
  netrep_progress_fn fn;
  void* user;
  {
    std::lock_guard<std::mutex> lk(g_hook_mu);
    fn = g_progress;
    user = g_progress_user;
  }
  if (fn) fn(ev, done, total, user);
}

bool interrupt_requested() {
  netrep_interrupt_fn fn;
  void* user;
  {
    std::lock_guard<std::mutex> lk(g_hook_mu);
    fn = g_hook;
    user = g_hook_user;
  }
  return fn != nullptr && fn(user) != 0;
}

// Test datasets uploaded ahead of their PermutationProcedure calls
// (netrep_PrefetchTestDataset): each has its own context on GPU 0, filled by
// a host thread while the previous dataset's permutations run. At most
// kMaxPrefetch are pending (the oldest is dropped beyond that).
struct Prefetch {
  std::thread th;
  CtxPtr ctx;
  const double *data = nullptr, *corr = nullptr, *net = nullptr;
  int64_t n_samples = 0, n_nodes = 0;
  std::atomic<int> rc{NR_OK};
  void join() {
    if (th.joinable()) th.join();
  }
  // at process exit: finish the upload thread, leave the context to the
  // driver's teardown (the HIP runtime may already be gone)
  ~Prefetch() {
    join();
    (void)ctx.release();
  }
};
constexpr size_t kMaxPrefetch = 2;
std::mutex g_pf_mu;
std::vector<std::unique_ptr<Prefetch>> g_pf;

void drop_prefetch(std::unique_ptr<Prefetch>& p) {
  p->join();
  give_ctx(p->ctx);  // back to the pool (its dataset freed) while the runtime is alive
  p.reset();
}

// The pending prefetch of exactly these matrices (pointers and sizes), joined
// and removed from the queue; its context when the upload succeeded.
CtxPtr take_prefetch(const double* data, const double* corr, const double* net, int64_t n_samples,
                     int64_t n_nodes) {
  std::unique_ptr<Prefetch> hit;
  {
    std::lock_guard<std::mutex> lk(g_pf_mu);
    for (size_t i = 0; i < g_pf.size(); ++i) {
      Prefetch& p = *g_pf[i];
      if (p.data == data && p.corr == corr && p.net == net && p.n_nodes == n_nodes &&
          (data == nullptr || p.n_samples == n_samples)) {
        hit = std::move(g_pf[i]);
        g_pf.erase(g_pf.begin() + (long)i);
        break;
      }
    }
  }
  CtxPtr out;
  if (!hit) return out;
  hit->join();
  if (hit->rc.load() == NR_OK) out = std::move(hit->ctx);
  drop_prefetch(hit);
  return out;
}

// Index sets of the modules present in the test dataset (a4 of SURVEY.md 8).
struct ModuleSets {
  int32_t n_rows = 0, n_present = 0;
  std::vector<int32_t> row_of;
  std::vector<int64_t> node_off{0};
  std::vector<int32_t> test_idx, null_pos;
  std::vector<int32_t> null_idx;
  std::vector<double>& disc_cv;  // the calling thread's reused buffer (cv_buffer)
  std::vector<double> disc_wd, disc_nc;
  explicit ModuleSets(std::vector<double>& cv) : disc_cv(cv) { disc_cv.clear(); }
};

// The concatenated discovery correlations of one call (C5: 10.3M doubles)
// live in a per-thread buffer that keeps its pages between calls:
// modulePreservation calls PermutationProcedure once per test dataset with
// the same discovery vectors, and a fresh 82 MB vector per call cost ~40 ms
// of page faults and copies.
std::vector<double>& cv_buffer() {
  thread_local std::vector<double> buf;
  return buf;
}

}  // namespace

extern "C" {

const char* netrep_last_error(void) { return g_err.c_str(); }

void netrep_set_interrupt_hook(netrep_interrupt_fn fn, void* user) {
  std::lock_guard<std::mutex> lk(g_hook_mu);
  g_hook = fn;
  g_hook_user = user;
}

void netrep_set_progress_hook(netrep_progress_fn fn, void* user) {
  std::lock_guard<std::mutex> lk(g_hook_mu);
  g_progress = fn;
  g_progress_user = user;
}

int netrep_format_progress(int64_t done, int64_t total, char* buf, int64_t cap) {
  if (!buf || cap <= 0) return -1;
  // src/thread-utils.cpp:66-68: round((float)nCompleted / (float)nPerm * 100)
  const unsigned pct = total > 0 ? (unsigned)std::round((float)done / (float)total * 100.0f) : 0u;
  const int n = std::snprintf(buf, (size_t)cap, "\r%5u%% completed.", pct);
  return (n < 0 || n >= cap) ? -1 : n;
}

void netrep_ReleaseResident(void) {
  netrep_DiscardPrefetch();
  {
    std::lock_guard<std::mutex> lk(g_res_mu);
    g_disc_res.drop();
    g_props_res.drop();
  }
  std::vector<Pooled> all;
  {
    std::lock_guard<std::mutex> lk(g_pool_mu);
    all.swap(g_pool);
    for (Pooled& p : all) g_ctx_device.erase(p.ctx.get());
  }
  all.clear();  // contexts destroyed while the runtime is alive
}

int netrep_PoolInfo(int64_t* n_pooled, int64_t* scratch_bytes, int32_t* host_threads_min,
                    int32_t* host_threads_max) {
  std::lock_guard<std::mutex> lk(g_pool_mu);
  int64_t bytes = 0;
  int32_t lo = 0, hi = 0;
  for (size_t i = 0; i < g_pool.size(); ++i) {
    int64_t b = 0;
    int t = 0;
    if (nr_scratch_bytes(g_pool[i].ctx.get(), &b) != NR_OK || nr_ctx_get_host_threads(g_pool[i].ctx.get(), &t) != NR_OK)
      return set_err(NR_ERR_INVALID, "pool inspection failed");
    bytes += b;
    lo = i == 0 ? t : std::min(lo, (int32_t)t);
    hi = i == 0 ? t : std::max(hi, (int32_t)t);
  }
  if (n_pooled) *n_pooled = (int64_t)g_pool.size();
  if (scratch_bytes) *scratch_bytes = bytes;
  if (host_threads_min) *host_threads_min = lo;
  if (host_threads_max) *host_threads_max = hi;
  return NR_OK;
}

void netrep_DiscardPrefetch(void) {
  std::vector<std::unique_ptr<Prefetch>> all;
  {
    std::lock_guard<std::mutex> lk(g_pf_mu);
    all.swap(g_pf);
  }
  for (auto& p : all) drop_prefetch(p);
}

int netrep_PrefetchTestDataset(const double* t_data, const double* t_corr, const double* t_net,
                               int64_t n_samples, int64_t n_nodes) try {
  if (!t_corr || !t_net || n_nodes <= 0 || (t_data && n_samples < 2))
    return set_err(NR_ERR_INVALID, "invalid arguments to PrefetchTestDataset");
  std::unique_ptr<Prefetch> p(new Prefetch());
  const int rc = open_ctx(0, p->ctx);
  if (rc) return rc;
  p->data = t_data;
  p->corr = t_corr;
  p->net = t_net;
  p->n_samples = n_samples;
  p->n_nodes = n_nodes;
  Prefetch* raw = p.get();
  raw->th = std::thread([raw]() {
    raw->rc = nr_set_dataset(raw->ctx.get(), raw->corr, raw->net, raw->data, raw->n_nodes, raw->n_samples,
                             NR_HOST);
  });
  std::unique_ptr<Prefetch> dropped;
  {
    std::lock_guard<std::mutex> lk(g_pf_mu);
    g_pf.push_back(std::move(p));
    if (g_pf.size() > kMaxPrefetch) {
      dropped = std::move(g_pf.front());
      g_pf.erase(g_pf.begin());
    }
  }
  if (dropped) drop_prefetch(dropped);
  return NR_OK;
} catch (const std::bad_alloc&) {
  return set_err(NR_ERR_OOM, "host memory allocation failed");
} catch (const std::exception& e) {
  return set_err(NR_ERR_INVALID, std::string("internal error: ") + e.what());
}

}  // extern "C"

namespace {

// PermutationProcedure with the dataset given either as host matrices or as a
// context that already holds it (`preloaded`: a prefetch, a file load or a
// dataset handle's). With `keep`, the preloaded context is handed back there
// on every return, its dataset still resident, instead of going to the pool.
int permutation_impl(const netrep_disc_props* disc, bool with_data, const double* t_data,
                     const double* t_corr, const double* t_net, int64_t n_samples, int64_t n_nodes,
                     const char* const* t_names, const char* const* ma_names, const char* const* ma_labels,
                     int64_t n_assign, const char* const* modules, int64_t n_modules, int64_t n_perm,
                     const char* null_hypothesis, int32_t verbose, uint64_t seed, const uint32_t* pi,
                     double* nulls_out, double* observed_out, CtxPtr preloaded, int32_t n_cores,
                     int64_t pi_len = -1, CtxPtr* keep = nullptr) {
  // returns before the lease below exists
  struct HandBack {
    CtxPtr* keep;
    CtxPtr* from;
    ~HandBack() {
      if (keep && *from) *keep = std::move(*from);
    }
  } hand_back{keep, &preloaded};
  if (with_data && !disc->contribution)
    return set_err(NR_ERR_INVALID, "discProps has no 'contribution' but tData was given");
  const std::string null_type = null_hypothesis ? null_hypothesis : "overlap";
  if (null_type != "overlap" && null_type != "all")
    return set_err(NR_ERR_INVALID, "nullHypothesis must be \"overlap\" or \"all\"");

  // src/permutations.cpp:184-201
  const NameMap t_idx_map = make_idx_map(t_names, n_nodes);
  const ModMap present = make_mod_map(ma_names, ma_labels, n_assign, &t_idx_map);

  // MakeNullMap (src/utils.cpp:108-136) over validNodes (src/permutations.cpp:319-323)
  ModuleSets ms(cv_buffer());
  NameMap null_map;
  {
    const char* const* valid = null_type == "overlap" ? ma_names : t_names;
    const int64_t n_valid = null_type == "overlap" ? n_assign : n_nodes;
    for (int64_t i = 0; i < n_valid; ++i) {
      auto it = t_idx_map.find(valid[i]);
      if (it == t_idx_map.end()) continue;
      null_map[valid[i]] = (int64_t)ms.null_idx.size();
      ms.null_idx.push_back((int32_t)it->second);
    }
  }

  ms.n_rows = (int32_t)n_modules;
  {  // one allocation per vector
    int64_t n_node = 0, n_pair = 0;
    for (int64_t mi = 0; mi < n_modules; ++mi) {
      const std::vector<std::string>* nodes = present.find(modules[mi]);
      const int64_t k = nodes ? (int64_t)nodes->size() : 0;
      n_node += k;
      n_pair += k * (k - 1) / 2;
    }
    ms.test_idx.reserve((size_t)n_node);
    ms.null_pos.reserve((size_t)n_node);
    ms.disc_wd.reserve((size_t)n_node);
    if (with_data) ms.disc_nc.reserve((size_t)n_node);
    ms.disc_cv.reserve((size_t)n_pair);
  }
  for (int64_t mi = 0; mi < n_modules; ++mi) {
    const std::vector<std::string>* nodes = present.find(modules[mi]);
    if (!nodes || nodes->empty()) continue;  // modsPresent (src/permutations.cpp:196-201)
    const int64_t k = (int64_t)nodes->size();
    if (disc->degree[mi] == nullptr || disc->degree_len[mi] != k || disc->corr[mi] == nullptr ||
        disc->corr_len[mi] != k * (k - 1) / 2 ||
        (with_data && (disc->contribution[mi] == nullptr || disc->contribution_len[mi] != k)))
      return set_err(NR_ERR_INVALID, std::string("discProps vectors of module '") + modules[mi] +
                                         "' do not match its nodes present in the test dataset");
    ms.row_of.push_back((int32_t)mi);
    for (const std::string& nm : *nodes) {
      ms.test_idx.push_back((int32_t)t_idx_map.at(nm));      // GetNodeIdx src/utils.cpp:147-162
      auto np = null_map.find(nm);
      if (np == null_map.end())
        return set_err(NR_ERR_INVALID, "module node '" + nm + "' is not in the null pool");
      ms.null_pos.push_back((int32_t)np->second);
    }
    ms.node_off.push_back((int64_t)ms.test_idx.size());
    ms.disc_cv.insert(ms.disc_cv.end(), disc->corr[mi], disc->corr[mi] + k * (k - 1) / 2);
    ms.disc_wd.insert(ms.disc_wd.end(), disc->degree[mi], disc->degree[mi] + k);
    if (with_data) ms.disc_nc.insert(ms.disc_nc.end(), disc->contribution[mi], disc->contribution[mi] + k);
  }
  ms.n_present = (int32_t)ms.row_of.size();
  const int n_stat = with_data ? NR_NSTAT_DATA : NR_NSTAT_NODATA;
  // an explicit shuffle table of a known length must hold n_perm x n_null
  // entries (the engine reads exactly that many)
  if (pi && pi_len >= 0 && pi_len != n_perm * (int64_t)ms.null_idx.size())
    return set_err(NR_ERR_INVALID, "pi holds " + std::to_string(pi_len) + " entries, not nPermutations x n_null = " +
                                       std::to_string(n_perm) + " x " + std::to_string(ms.null_idx.size()));

  int n_dev = 1;
  const int n_gpu = (n_perm > 0) ? (int)std::min<int64_t>(gpu_count_requested(&n_dev), std::max<int64_t>(n_perm, 1)) : 1;
  std::vector<CtxPtr> ctxs(n_gpu);
  CtxLease lease{&ctxs, keep};  // the contexts go back to the pool (without the dataset) on every return
  // a dataset already resident (prefetched or loaded from files) becomes GPU 0's
  ctxs[0] = std::move(preloaded);
  const bool prefetched = ctxs[0] != nullptr;
  for (int g = prefetched ? 1 : 0; g < n_gpu; ++g) {
    int rc = open_ctx(g % n_dev, ctxs[g]);
    if (rc) return rc;
  }
  for (CtxPtr& c : ctxs) nr_ctx_set_host_threads(c.get(), n_cores);  // nThreads: this call's host threads
  // The host matrices cross PCIe once, into the first GPU; the other GPUs
  // receive them device to device by the scatter + all-gather broadcast over
  // the xGMI mesh (nr_broadcast_dataset).
  if (!prefetched) {
    const int rc = nr_set_dataset(ctxs[0].get(), t_corr, t_net, t_data, n_nodes, n_samples, NR_HOST);
    if (rc) return ctx_err(rc, ctxs[0].get());
  }
  if (n_gpu > 1) {
    std::vector<nr_ctx*> raw(n_gpu);
    for (int g = 0; g < n_gpu; ++g) raw[g] = ctxs[g].get();
    const int rc = nr_broadcast_dataset(raw.data(), n_gpu);
    if (rc) return ctx_err(rc, ctxs[0].get());
  }
  std::vector<int> rcs(n_gpu, NR_OK);
  auto setup = [&](int g) {
    nr_ctx* c = ctxs[g].get();
    int rc = nr_set_modules(c, ms.n_rows, ms.n_present, ms.row_of.data(), ms.node_off.data(),
                            ms.test_idx.data(), ms.null_pos.data(), ms.disc_cv.data(),
                            ms.disc_wd.data(), with_data ? ms.disc_nc.data() : nullptr);
    if (!rc && !ms.null_idx.empty()) rc = nr_set_null_pool(c, ms.null_idx.data(), (int64_t)ms.null_idx.size());
    rcs[g] = rc;
  };
  {
    std::vector<std::thread> th;
    for (int g = 1; g < n_gpu; ++g) th.emplace_back(setup, g);
    setup(0);
    for (auto& t : th) t.join();
  }
  for (int g = 0; g < n_gpu; ++g)
    if (rcs[g]) return ctx_err(rcs[g], ctxs[g].get());

  // Observed statistics (src/permutations.cpp:246-285): enqueued on GPU 0's
  // second stream, where they run beside the first permutation batch, and
  // collected after the permutations.
  {
    const int rc = nr_observed_async(ctxs[0].get());
    if (rc) return ctx_err(rc, ctxs[0].get());
  }
  auto collect_observed = [&]() -> int {
    const int rc = nr_observed_wait(ctxs[0].get(), observed_out);
    return rc ? ctx_err(rc, ctxs[0].get()) : NR_OK;
  };
  if (n_perm == 0) return collect_observed();  // src/permutations.cpp:288-299

  // Contiguous permutation chunks, remainder to the first devices
  // (src/permutations.cpp:338-354).
  std::vector<int64_t> start(n_gpu + 1, 0);
  for (int g = 0; g < n_gpu; ++g)
    start[g + 1] = start[g] + n_perm / n_gpu + (g < n_perm % n_gpu ? 1 : 0);
  const int64_t slice = (int64_t)ms.n_rows * n_stat;
  const int64_t n_null = (int64_t)ms.null_idx.size();
  if (verbose) progress_event(NETREP_PROGRESS_BEGIN, 0, n_perm);
  std::atomic<int> running{n_gpu};
  std::vector<std::thread> th;
  for (int g = 0; g < n_gpu; ++g) {
    th.emplace_back([&, g]() {
      rcs[g] = nr_run(ctxs[g].get(), start[g], start[g + 1], seed,
                      pi ? pi + start[g] * n_null : nullptr, nulls_out + start[g] * slice);
      running.fetch_sub(1);
    });
  }
  // Progress monitor (MonitorProgress, src/thread-utils.cpp:49-82): the
  // calling thread polls progress and the interrupt hook every 100 ms and,
  // when verbose, reports progress through the progress hook once a second
  // (the library prints nothing itself). On an interrupt every
  // context is cancelled; the workers stop between launches and leave their
  // remaining slices NA, and the partial cube is returned
  // (src/permutations.cpp:375-408) with NR_ERR_CANCELLED.
  bool interrupted = false;
  auto last_print = std::chrono::steady_clock::now() - std::chrono::seconds(1);
  for (;;) {
    const bool done_all = running.load() == 0;
    if (verbose && (done_all || std::chrono::steady_clock::now() - last_print >= std::chrono::seconds(1))) {
      int64_t done = 0;
      for (int g = 0; g < n_gpu; ++g) {
        int64_t d = 0;
        nr_progress(ctxs[g].get(), &d, nullptr);
        done += d;
      }
      progress_event(NETREP_PROGRESS_UPDATE, done, n_perm);
      last_print = std::chrono::steady_clock::now();
    }
    if (done_all) break;
    if (!interrupted && interrupt_requested()) {
      interrupted = true;
      for (int g = 0; g < n_gpu; ++g) nr_cancel(ctxs[g].get());
    }
    std::this_thread::sleep_for(std::chrono::milliseconds(100));
  }
  if (verbose) progress_event(NETREP_PROGRESS_END, n_perm, n_perm);
  for (auto& t : th) t.join();
  if (int rc = collect_observed()) return rc;
  int cancelled_at = -1;
  for (int g = 0; g < n_gpu; ++g) {
    if (rcs[g] == NR_ERR_CANCELLED) {
      if (cancelled_at < 0) cancelled_at = g;
      continue;
    }
    if (rcs[g]) return ctx_err(rcs[g], ctxs[g].get());
  }
  if (cancelled_at >= 0) return ctx_err(NR_ERR_CANCELLED, ctxs[cancelled_at].get());
  return NR_OK;
}

}  // namespace

extern "C" {

int netrep_PermutationProcedure(const netrep_disc_props* disc, const double* t_data,
                                const double* t_corr, const double* t_net, int64_t n_samples,
                                int64_t n_nodes, const char* const* t_names,
                                const char* const* ma_names, const char* const* ma_labels,
                                int64_t n_assign, const char* const* modules, int64_t n_modules,
                                int64_t n_perm, int32_t n_cores, const char* null_hypothesis,
                                int32_t verbose, uint64_t seed, const uint32_t* pi,
                                double* nulls_out, double* observed_out) try {
  if (!disc || !t_corr || !t_net || !t_names || !ma_names || !ma_labels || !modules ||
      !observed_out || n_perm < 0 || (n_perm > 0 && !nulls_out) || n_nodes <= 0)
    return set_err(NR_ERR_INVALID, "invalid arguments to PermutationProcedure");
  // a dataset uploaded ahead (netrep_PrefetchTestDataset) is adopted
  CtxPtr pre = take_prefetch(t_data, t_corr, t_net, n_samples, n_nodes);
  int rc = permutation_impl(disc, t_data != nullptr, t_data, t_corr, t_net, n_samples, n_nodes, t_names, ma_names,
                            ma_labels, n_assign, modules, n_modules, n_perm, null_hypothesis, verbose, seed, pi,
                            nulls_out, observed_out, std::move(pre), n_cores);
  // Device memory held between calls (resident discovery / NetProps datasets,
  // pending prefetches, pooled contexts' scratch) must not turn a run that
  // fits the device into NR_ERR_OOM: release all of it and try
  // once more from the host matrices. The numerical path does not change.
  if (rc == NR_ERR_OOM) {
    netrep_ReleaseResident();
    rc = permutation_impl(disc, t_data != nullptr, t_data, t_corr, t_net, n_samples, n_nodes, t_names, ma_names,
                          ma_labels, n_assign, modules, n_modules, n_perm, null_hypothesis, verbose, seed, pi,
                          nulls_out, observed_out, CtxPtr(), n_cores);
  }
  return rc;
} catch (const std::bad_alloc&) {
  return set_err(NR_ERR_OOM, "host memory allocation failed");
} catch (const std::exception& e) {
  return set_err(NR_ERR_INVALID, std::string("internal error: ") + e.what());
}

int netrep_PermutationProcedureFiles(const netrep_disc_props* disc, const char* t_data_file,
                                     const char* t_corr_file, const char* t_net_file,
                                     const char* const* ma_names, const char* const* ma_labels,
                                     int64_t n_assign, const char* const* modules, int64_t n_modules,
                                     int64_t n_perm, int32_t n_cores, const char* null_hypothesis,
                                     int32_t verbose, uint64_t seed, const uint32_t* pi, int64_t pi_len,
                                     double* nulls_out, double* observed_out) try {
  if (!disc || !t_corr_file || !t_net_file || !ma_names || !ma_labels || !modules || !observed_out ||
      n_perm < 0 || (n_perm > 0 && !nulls_out))
    return set_err(NR_ERR_INVALID, "invalid arguments to PermutationProcedureFiles");
  CtxPtr ctx;
  int rc = open_ctx(0, ctx);
  if (rc) return rc;
  std::vector<CtxPtr> lease_v;
  CtxLease lease{&lease_v};  // back to the pool if the load fails
  // disk.matrix files straight to HBM; tData scaled on the device
  rc = nr_set_dataset_files(ctx.get(), t_corr_file, t_net_file, t_data_file, nullptr, nullptr, nullptr, 1);
  if (rc) {
    rc = ctx_err(rc, ctx.get());
    lease_v.push_back(std::move(ctx));
    return rc;
  }
  int64_t n_nodes = 0, n_samples = 0, need = 0;
  nr_dataset_shape(ctx.get(), &n_nodes, &n_samples);
  nr_dataset_colnames(ctx.get(), nullptr, 0, &need);
  std::vector<char> buf((size_t)std::max<int64_t>(need, 1));
  nr_dataset_colnames(ctx.get(), buf.data(), need, &need);
  std::vector<const char*> names;
  for (int64_t o = 0; o < need; o += (int64_t)std::strlen(buf.data() + o) + 1) names.push_back(buf.data() + o);
  if ((int64_t)names.size() != n_nodes)
    return set_err(NR_ERR_INVALID, "the network file has no column names (node names are needed)");
  return permutation_impl(disc, t_data_file != nullptr, nullptr, nullptr, nullptr, n_samples, n_nodes, names.data(),
                          ma_names, ma_labels, n_assign, modules, n_modules, n_perm, null_hypothesis, verbose,
                          seed, pi, nulls_out, observed_out, std::move(ctx), n_cores, pi_len);
} catch (const std::bad_alloc&) {
  return set_err(NR_ERR_OOM, "host memory allocation failed");
} catch (const std::exception& e) {
  return set_err(NR_ERR_INVALID, std::string("internal error: ") + e.what());
}

}  // extern "C"

namespace {

// The argument checks of the from-data entries (before any context is opened).
int check_from_data_args(const double* data, int32_t net_type, double beta, int64_t n_samples, int64_t n_nodes) {
  if (!data) return set_err(NR_ERR_INVALID, "data missing");
  if (n_samples < 2 || n_nodes < 1) return set_err(NR_ERR_INVALID, "data needs n_samples >= 2 and n_nodes >= 1");
  // NR_NET_TOM and one correlation type may ride on any of the three
  const int32_t cor_type = net_type & (NR_COR_SPEARMAN | NR_COR_BICOR);
  const int32_t base_type = net_type & ~(NR_NET_TOM | NR_COR_SPEARMAN | NR_COR_BICOR);
  if (base_type != NR_NET_UNSIGNED && base_type != NR_NET_SIGNED && base_type != NR_NET_SIGNED_HYBRID)
    return set_err(NR_ERR_INVALID, "unknown network type");
  if (cor_type == (NR_COR_SPEARMAN | NR_COR_BICOR)) return set_err(NR_ERR_INVALID, "unknown correlation type");
  if (!std::isfinite(beta) || beta <= 0.0) return set_err(NR_ERR_INVALID, "beta must be finite and > 0");
  return NR_OK;
}

// Context 0 with the dataset built from `data`; on failure the context goes
// back to the pool.
int open_from_data(const double* data, int32_t scale_data, int32_t net_type, double beta, int64_t n_samples,
                   int64_t n_nodes, int32_t n_cores, CtxPtr& ctx) {
  int rc = open_ctx(0, ctx);
  if (rc) return rc;
  if (n_cores != 0) nr_ctx_set_host_threads(ctx.get(), n_cores);
  rc = nr_set_dataset_from_data(ctx.get(), data, n_nodes, n_samples, NR_HOST, scale_data ? NR_SCALE_DATA : 0,
                                net_type, beta);
  if (rc) {
    rc = ctx_err(rc, ctx.get());
    give_ctx(ctx);
  }
  return rc;
}

int from_data_once(const netrep_disc_props* disc, const double* t_data, int32_t scale_data, int32_t net_type,
                   double beta, int64_t n_samples, int64_t n_nodes, const char* const* t_names,
                   const char* const* ma_names, const char* const* ma_labels, int64_t n_assign,
                   const char* const* modules, int64_t n_modules, int64_t n_perm, int32_t n_cores,
                   const char* null_hypothesis, int32_t verbose, uint64_t seed, const uint32_t* pi,
                   double* nulls_out, double* observed_out) {
  CtxPtr ctx;
  int rc = open_from_data(t_data, scale_data, net_type, beta, n_samples, n_nodes, n_cores, ctx);
  if (rc) return rc;
  int cf = 0, nf = 0;
  nr_dataset_finite(ctx.get(), &cf, &nf);
  if (!cf || !nf) {  // R/check-user-input.R:796-799, before any permutation runs
    give_ctx(ctx);
    return set_err(NR_ERR_NONFINITE, "matrices cannot have non-finite or missing values");
  }
  return permutation_impl(disc, true, nullptr, nullptr, nullptr, n_samples, n_nodes, t_names, ma_names, ma_labels,
                          n_assign, modules, n_modules, n_perm, null_hypothesis, verbose, seed, pi, nulls_out,
                          observed_out, std::move(ctx), n_cores);
}

// IntermediateProperties' module resolution (src/discProps.cpp:64-79): the
// modules with a node in the test node list, their nodes as discovery indices.
struct DiscSets {
  std::vector<int64_t> node_off{0};
  std::vector<int32_t> idx;
  std::vector<int64_t> which;  // row in `modules` of each set
};

int resolve_disc_sets(const NameMap& d_idx_map, const char* const* t_node_names, int64_t n_t_nodes,
                      const char* const* ma_names, const char* const* ma_labels, int64_t n_assign,
                      const char* const* modules, int64_t n_modules, int64_t* degree_len, int64_t* corr_len,
                      int64_t* contribution_len, DiscSets& ds) {
  const NameMap t_idx_map = make_idx_map(t_node_names, n_t_nodes);
  const ModMap present = make_mod_map(ma_names, ma_labels, n_assign, &t_idx_map);
  for (int64_t mi = 0; mi < n_modules; ++mi) {
    degree_len[mi] = corr_len[mi] = 0;
    if (contribution_len) contribution_len[mi] = 0;
    const std::vector<std::string>* nodes = present.find(modules[mi]);
    if (!nodes || nodes->empty()) continue;
    for (const std::string& nm : *nodes) {
      auto it = d_idx_map.find(nm);  // GetNodeIdx (src/utils.cpp:157) throws on a miss
      if (it == d_idx_map.end())
        return set_err(NR_ERR_INVALID, "node '" + nm + "' of moduleAssignments is not in the discovery dataset");
      ds.idx.push_back((int32_t)it->second);
    }
    ds.node_off.push_back((int64_t)ds.idx.size());
    ds.which.push_back(mi);
  }
  return NR_OK;
}

// The discovery vectors of the resolved modules from the context's resident
// dataset, concatenated in `modules` order (src/discProps.cpp:119-125).
int disc_vectors(nr_ctx* ctx, const DiscSets& ds, bool with_data, double* degree_out, int64_t* degree_len,
                 double* corr_out, int64_t* corr_len, double* contribution_out, int64_t* contribution_len) {
  const int32_t n_mod = (int32_t)ds.which.size();
  const std::vector<int64_t>& node_off = ds.node_off;
  const int64_t nodes = node_off.back();
  int64_t n_cv = 0;
  for (int32_t m = 0; m < n_mod; ++m) {
    const int64_t k = node_off[m + 1] - node_off[m];
    n_cv += k * (k - 1) / 2;
  }
  std::vector<double> cv((size_t)std::max<int64_t>(n_cv, 1)), wd((size_t)nodes), nc(with_data ? (size_t)nodes : 0);
  const int rc = nr_module_vectors(ctx, n_mod, node_off.data(), ds.idx.data(), cv.data(), wd.data(), nullptr,
                                   with_data ? nc.data() : nullptr, nullptr, nullptr);
  if (rc) return ctx_err(rc, ctx);
  int64_t o_cv = 0, o_n = 0;
  for (int32_t m = 0; m < n_mod; ++m) {
    const int64_t mi = ds.which[m];
    const int64_t k = node_off[m + 1] - node_off[m];
    const int64_t kc = k * (k - 1) / 2;
    std::memcpy(corr_out + o_cv, cv.data() + o_cv, (size_t)kc * sizeof(double));
    std::memcpy(degree_out + o_n, wd.data() + node_off[m], (size_t)k * sizeof(double));
    if (with_data) std::memcpy(contribution_out + o_n, nc.data() + node_off[m], (size_t)k * sizeof(double));
    corr_len[mi] = kc;
    degree_len[mi] = k;
    if (with_data) contribution_len[mi] = k;
    o_cv += kc;
    o_n += k;
  }
  return NR_OK;
}

double na_real() {
  const uint64_t b = 0x7FF00000000007A2ull;
  double d;
  std::memcpy(&d, &b, 8);
  return d;
}

// NetProps' module resolution: per module all its nodes (k_all), and the
// present ones as dataset index + slot in the module's output.
struct PropSets {
  std::vector<int64_t> node_off{0}, out_off;
  std::vector<int32_t> idx, slot;
  std::vector<int64_t> which;
};

// Resolves the modules and NA-initialises the outputs (src/properties.cpp:131-139).
void resolve_prop_sets(const NameMap& node_idx, const char* const* ma_names, const char* const* ma_labels,
                       int64_t n_assign, const char* const* modules, int64_t n_modules, bool with_data,
                       int64_t n_samples, double* degree_out, double* contribution_out, double* summary_out,
                       double* coherence_out, double* avg_weight_out, int64_t* k_all_out, PropSets& ps) {
  const double na = na_real();
  const ModMap all = make_mod_map(ma_names, ma_labels, n_assign, nullptr);  // src/properties.cpp:108
  std::vector<int64_t> k_all(n_modules, 0);
  std::vector<int64_t>& out_off = ps.out_off;
  out_off.assign(n_modules + 1, 0);
  for (int64_t mi = 0; mi < n_modules; ++mi) {
    const std::vector<std::string>* nodes = all.find(modules[mi]);
    k_all[mi] = nodes ? (int64_t)nodes->size() : 0;
    out_off[mi + 1] = out_off[mi] + k_all[mi];
    if (!nodes) continue;
    const size_t before = ps.idx.size();
    for (size_t j = 0; j < nodes->size(); ++j) {
      auto it = node_idx.find((*nodes)[j]);
      if (it == node_idx.end()) continue;
      ps.idx.push_back((int32_t)it->second);
      ps.slot.push_back((int32_t)j);
    }
    if (ps.idx.size() > before) {
      ps.node_off.push_back((int64_t)ps.idx.size());
      ps.which.push_back(mi);
    }
  }
  for (int64_t mi = 0; mi < n_modules; ++mi) {
    k_all_out[mi] = k_all[mi];
    avg_weight_out[mi] = na;
    for (int64_t j = out_off[mi]; j < out_off[mi + 1]; ++j) {
      degree_out[j] = na;
      if (with_data) contribution_out[j] = na;
    }
    if (with_data) {
      coherence_out[mi] = na;
      for (int64_t s = 0; s < n_samples; ++s) summary_out[mi * n_samples + s] = na;
    }
  }
}

// The network properties of the resolved modules from the context's resident
// dataset, filled into the outputs' slots.
int prop_vectors(nr_ctx* ctx, const PropSets& ps, bool with_data, int64_t n_samples, double* degree_out,
                 double* contribution_out, double* summary_out, double* coherence_out, double* avg_weight_out) {
  const double na = na_real();
  const int32_t n_mod = (int32_t)ps.which.size();
  const std::vector<int64_t>& node_off = ps.node_off;
  const int64_t nodes = node_off.back();
  std::vector<double> wd((size_t)nodes), aw((size_t)n_mod), nc, sp, coh;
  if (with_data) {
    nc.resize((size_t)nodes);
    sp.resize((size_t)(n_mod * n_samples));
    coh.resize((size_t)n_mod);
  }
  const int rc = nr_module_vectors(ctx, n_mod, node_off.data(), ps.idx.data(), nullptr, wd.data(), aw.data(),
                                   with_data ? nc.data() : nullptr, with_data ? sp.data() : nullptr,
                                   with_data ? coh.data() : nullptr);
  if (rc) return ctx_err(rc, ctx);
  auto na_if = [&](double x) { return std::isfinite(x) ? x : na; };
  for (int32_t m = 0; m < n_mod; ++m) {
    const int64_t mi = ps.which[m];
    avg_weight_out[mi] = aw[m];  // AverageEdgeWeight result kept as is (src/properties.cpp:160)
    for (int64_t c = node_off[m]; c < node_off[m + 1]; ++c) {
      const int64_t j = ps.out_off[mi] + ps.slot[c];  // Fill (src/utils.cpp:245-257)
      degree_out[j] = wd[c];
      if (with_data) contribution_out[j] = na_if(nc[c]);  // :176
    }
    if (with_data) {
      coherence_out[mi] = na_if(coh[m]);  // :177-179
      for (int64_t s = 0; s < n_samples; ++s)
        summary_out[mi * n_samples + s] = na_if(sp[m * n_samples + s]);  // :175
    }
  }
  return NR_OK;
}

}  // namespace

// The opaque handle of include/netrep_gpu.h: a context that holds a from-data
// dataset, and the node names it was built with.
struct netrep_dataset {
  std::mutex mu;
  CtxPtr ctx;
  std::vector<std::string> names;
  std::vector<const char*> name_ptrs;
  NameMap idx_map;
  int64_t n_nodes = 0, n_samples = 0;
  int32_t n_cores = 0;
  ~netrep_dataset() { give_ctx(ctx); }
};

namespace {

int dataset_from_data_once(const double* data, int32_t scale_data, int32_t net_type, double beta, int64_t n_samples,
                           int64_t n_nodes, int32_t n_cores, CtxPtr& ctx) {
  int rc = open_from_data(data, scale_data, net_type, beta, n_samples, n_nodes, n_cores, ctx);
  if (rc) return rc;
  int cf = 0, nf = 0;
  nr_dataset_finite(ctx.get(), &cf, &nf);
  if (!cf || !nf) {
    give_ctx(ctx);
    return set_err(NR_ERR_NONFINITE, "matrices cannot have non-finite or missing values");
  }
  return NR_OK;
}

int no_dataset(const char* entry) {
  return set_err(NR_ERR_INVALID, std::string("invalid arguments to ") + entry + " (no dataset)");
}

// With the handle's mutex held: its context is there.
int live(netrep_dataset* d) {
  if (!d->ctx) return set_err(NR_ERR_INVALID, "the dataset's context was lost to an earlier error");
  return NR_OK;
}


// The modules of a label vector as nr_module_eigengenes takes them: the
// distinct positive labels in increasing order and their nodes in CSR form.
struct LabelSets {
  std::vector<int32_t> modules;
  std::vector<int64_t> node_off;
  std::vector<int32_t> idx;
};

int resolve_labels(const char* entry, int64_t n, const int32_t* labels, LabelSets& ls) {
  if (!nr::module_labels_of(n, labels, ls.modules))
    return set_err(NR_ERR_INVALID, std::string("invalid arguments to ") + entry + " (a negative label)");
  if (ls.modules.empty())
    return set_err(NR_ERR_INVALID, std::string("invalid arguments to ") + entry + " (no positive label)");
  const size_t M = ls.modules.size();
  ls.node_off.assign(M + 1, 0);
  auto slot = [&](int32_t lab) {
    return (size_t)(std::lower_bound(ls.modules.begin(), ls.modules.end(), lab) - ls.modules.begin());
  };
  for (int64_t i = 0; i < n; ++i)
    if (labels[i] > 0) ++ls.node_off[slot(labels[i]) + 1];
  for (size_t m = 0; m < M; ++m) ls.node_off[m + 1] += ls.node_off[m];
  ls.idx.resize((size_t)ls.node_off[M]);
  std::vector<int64_t> at(ls.node_off.begin(), ls.node_off.end() - 1);
  for (int64_t i = 0; i < n; ++i)
    if (labels[i] > 0) ls.idx[(size_t)at[slot(labels[i])]++] = (int32_t)i;
  return NR_OK;
}

// With the handle's mutex held: the eigengenes of a label vector's modules on
// the handle's context (they stay on the device for nr_module_membership).
// kme_own, optional: [n] in node order, NA for label 0.
int label_eigengenes(netrep_dataset* d, const LabelSets& ls, double* eigengenes, double* var_explained,
                     double* kme_own) {
  if (interrupt_requested()) return set_err(NR_ERR_CANCELLED, "interrupted");
  nr_ctx* const c = d->ctx.get();
  std::vector<double> nc(kme_own ? ls.idx.size() : 0);
  const int rc = nr_module_eigengenes(c, (int32_t)ls.modules.size(), ls.node_off.data(), ls.idx.data(), eigengenes,
                                      var_explained, kme_own ? nc.data() : nullptr);
  if (rc) return ctx_err(rc, c);
  if (kme_own) {
    std::fill(kme_own, kme_own + d->n_nodes, na_real());
    for (size_t j = 0; j < ls.idx.size(); ++j) kme_own[ls.idx[j]] = nc[j];
  }
  return NR_OK;
}

// slot[j]: node j's module index in ls.modules, -1 for label 0.
std::vector<int32_t> slots_of(int64_t n, const int32_t* labels, const LabelSets& ls) {
  std::vector<int32_t> slot((size_t)n, -1);
  for (int64_t j = 0; j < n; ++j)
    if (labels[j] > 0)
      slot[(size_t)j] =
          (int32_t)(std::lower_bound(ls.modules.begin(), ls.modules.end(), labels[j]) - ls.modules.begin());
  return slot;
}

// With the handle's mutex held: nr_module_connectivity of a label vector's
// modules on the handle's context.
int label_connectivity(netrep_dataset* d, const int32_t* labels, const LabelSets& ls, double* k_total,
                       double* k_mod) {
  if (interrupt_requested()) return set_err(NR_ERR_CANCELLED, "interrupted");
  nr_ctx* const c = d->ctx.get();
  const std::vector<int32_t> slot = slots_of(d->n_nodes, labels, ls);
  int rc = nr_module_connectivity(c, (int32_t)ls.modules.size(), slot.data(), k_total, k_mod);
  if (rc) rc = ctx_err(rc, c);
  (void)nr_release_scratch(c);
  return rc;
}

}  // namespace

extern "C" {

int netrep_PermutationProcedureFromData(const netrep_disc_props* disc, const double* t_data, int32_t scale_data,
                                        int32_t net_type, double beta, int64_t n_samples, int64_t n_nodes,
                                        const char* const* t_names, const char* const* ma_names,
                                        const char* const* ma_labels, int64_t n_assign, const char* const* modules,
                                        int64_t n_modules, int64_t n_perm, int32_t n_cores,
                                        const char* null_hypothesis, int32_t verbose, uint64_t seed,
                                        const uint32_t* pi, double* nulls_out, double* observed_out) try {
  if (int rc = check_from_data_args(t_data, net_type, beta, n_samples, n_nodes)) return rc;
  if (!disc || !t_names || !ma_names || !ma_labels || !modules || !observed_out || n_perm < 0 ||
      (n_perm > 0 && !nulls_out))
    return set_err(NR_ERR_INVALID, "invalid arguments to PermutationProcedureFromData");
  int rc = from_data_once(disc, t_data, scale_data, net_type, beta, n_samples, n_nodes, t_names, ma_names, ma_labels,
                          n_assign, modules, n_modules, n_perm, n_cores, null_hypothesis, verbose, seed, pi,
                          nulls_out, observed_out);
  if (rc == NR_ERR_OOM) {  // as netrep_PermutationProcedure: free what is held between calls, once
    netrep_ReleaseResident();
    rc = from_data_once(disc, t_data, scale_data, net_type, beta, n_samples, n_nodes, t_names, ma_names, ma_labels,
                        n_assign, modules, n_modules, n_perm, n_cores, null_hypothesis, verbose, seed, pi,
                        nulls_out, observed_out);
  }
  return rc;
} catch (const std::bad_alloc&) {
  return set_err(NR_ERR_OOM, "host memory allocation failed");
} catch (const std::exception& e) {
  return set_err(NR_ERR_INVALID, std::string("internal error: ") + e.what());
}

int netrep_BuildNetwork(const double* data, int32_t scale_data, int32_t net_type, double beta, int64_t n_samples,
                        int64_t n_nodes, double* corr_out, double* net_out) try {
  if (int rc = check_from_data_args(data, net_type, beta, n_samples, n_nodes)) return rc;
  CtxPtr ctx;
  int rc = open_from_data(data, scale_data, net_type, beta, n_samples, n_nodes, 0, ctx);
  if (rc) return rc;
  rc = nr_get_dataset_matrices(ctx.get(), corr_out, net_out);
  if (rc) rc = ctx_err(rc, ctx.get());
  give_ctx(ctx);
  return rc;
} catch (const std::bad_alloc&) {
  return set_err(NR_ERR_OOM, "host memory allocation failed");
} catch (const std::exception& e) {
  return set_err(NR_ERR_INVALID, std::string("internal error: ") + e.what());
}

int netrep_ScaleFreeFit(const double* k, int64_t n, int32_t n_breaks, int32_t remove_first, double* out3) try {
  if (!k || !out3 || n < 1 || n_breaks < 3)
    return set_err(NR_ERR_INVALID, "invalid arguments to ScaleFreeFit (k, out3, n >= 1, n_breaks >= 3)");
  nr::scale_free_fit(k, n, n_breaks, remove_first != 0, out3);
  return NR_OK;
} catch (const std::bad_alloc&) {
  return set_err(NR_ERR_OOM, "host memory allocation failed");
}

int netrep_ScaleFreeBins(const double* k, int64_t n, int32_t n_breaks, int32_t* bins_out) {
  if (!k || !bins_out || n < 1 || n_breaks < 3)
    return set_err(NR_ERR_INVALID, "invalid arguments to ScaleFreeBins (k, bins_out, n >= 1, n_breaks >= 3)");
  (void)nr::scale_free_bins(k, n, n_breaks, bins_out, nullptr, nullptr);
  return NR_OK;
}

int netrep_SftPowerEstimate(const double* table, int32_t n_powers, double rsquared_cut, double* power_estimate_out) {
  if (!table || !power_estimate_out || n_powers < 1 || std::isnan(rsquared_cut))
    return set_err(NR_ERR_INVALID, "invalid arguments to SftPowerEstimate");
  *power_estimate_out = nr::sft_power_estimate(table, n_powers, rsquared_cut);
  return NR_OK;
}

int netrep_PickSoftThreshold(const double* data, int32_t scale_data, int32_t net_type, int64_t n_samples,
                             int64_t n_nodes, const double* powers, int32_t n_powers, double rsquared_cut,
                             int32_t n_breaks, int32_t remove_first, double* table_out,
                             double* power_estimate_out, double* connectivity_out) try {
  // every check before a context is opened (those of nr_soft_connectivity restated)
  if (!data || !powers || !table_out || !power_estimate_out)
    return set_err(NR_ERR_INVALID, "data, powers, table_out or power_estimate_out missing");
  if (n_powers < 1 || n_powers > 32) return set_err(NR_ERR_INVALID, "n_powers must be 1 .. 32");
  for (int32_t m = 0; m < n_powers; ++m)
    if (!std::isfinite(powers[m]) || powers[m] <= 0.0)
      return set_err(NR_ERR_INVALID, "powers must be finite and > 0");
  if (net_type & NR_NET_TOM) return set_err(NR_ERR_INVALID, "NR_NET_TOM has no soft-threshold connectivity");
  if (int rc = check_from_data_args(data, net_type, 1.0, n_samples, n_nodes)) return rc;
  if (n_breaks < 3) return set_err(NR_ERR_INVALID, "n_breaks must be >= 3");
  if (std::isnan(rsquared_cut)) return set_err(NR_ERR_INVALID, "rsquared_cut is NaN");
  std::vector<double> own;
  double* k = connectivity_out;
  if (!k) {
    own.resize((size_t)n_nodes * (size_t)n_powers);
    k = own.data();
  }
  CtxPtr ctx;
  int rc = open_ctx(0, ctx);
  if (rc) return rc;
  rc = nr_soft_connectivity(ctx.get(), data, n_nodes, n_samples, scale_data, net_type, powers, n_powers, k);
  int finite = 1;
  if (!rc) rc = nr_sft_finite(ctx.get(), &finite);
  if (rc) rc = ctx_err(rc, ctx.get());
  give_ctx(ctx);
  if (rc) return rc;
  if (!finite) return set_err(NR_ERR_NONFINITE, "matrices cannot have non-finite or missing values");
  for (int32_t m = 0; m < n_powers; ++m)
    nr::sft_table_row(powers[m], k + (size_t)m * (size_t)n_nodes, n_nodes, n_breaks, remove_first != 0,
                      table_out + m, n_powers);
  *power_estimate_out = nr::sft_power_estimate(table_out, n_powers, rsquared_cut);
  return NR_OK;
} catch (const std::bad_alloc&) {
  return set_err(NR_ERR_OOM, "host memory allocation failed");
} catch (const std::exception& e) {
  return set_err(NR_ERR_INVALID, std::string("internal error: ") + e.what());
}

int netrep_ReadRDSMatrix(const char* path, const char* object, int64_t* nrow, int64_t* ncol, double* out,
                         char* colnames, int64_t colnames_cap, int64_t* colnames_needed) try {
  if (!path || !nrow || !ncol) return set_err(NR_ERR_INVALID, "invalid arguments to ReadRDSMatrix");
  nr::RMatrixMeta meta;
  std::vector<double> v;
  std::string err;
  if (!nr::read_matrix_host(path, object, &meta, &v, out != nullptr, &err))
    return set_err(NR_ERR_INVALID, std::string(path) + ": " + err);
  *nrow = meta.nrow;
  *ncol = meta.ncol;
  if (out) std::memcpy(out, v.data(), v.size() * sizeof(double));
  int64_t total = 0;
  for (const std::string& s : meta.colnames) total += (int64_t)s.size() + 1;
  if (colnames_needed) *colnames_needed = total;
  if (colnames && colnames_cap >= total)
    for (const std::string& s : meta.colnames) {
      std::memcpy(colnames, s.c_str(), s.size() + 1);
      colnames += s.size() + 1;
    }
  return NR_OK;
} catch (const std::bad_alloc&) {
  return set_err(NR_ERR_OOM, "host memory allocation failed");
} catch (const std::exception& e) {
  return set_err(NR_ERR_INVALID, std::string("internal error: ") + e.what());
}

int netrep_IntermediateProperties(const double* d_data, const double* d_corr, const double* d_net,
                                  int64_t n_samples, int64_t n_nodes, const char* const* d_names,
                                  const char* const* t_node_names, int64_t n_t_nodes,
                                  const char* const* ma_names, const char* const* ma_labels,
                                  int64_t n_assign, const char* const* modules, int64_t n_modules,
                                  double* degree_out, int64_t* degree_len, double* corr_out,
                                  int64_t* corr_len, double* contribution_out,
                                  int64_t* contribution_len) try {
  if (!d_corr || !d_net || !d_names || !t_node_names || !ma_names || !ma_labels || !modules ||
      !degree_out || !degree_len || !corr_out || !corr_len || n_nodes <= 0)
    return set_err(NR_ERR_INVALID, "invalid arguments to IntermediateProperties");
  const bool with_data = d_data != nullptr;
  if (with_data && (!contribution_out || !contribution_len))
    return set_err(NR_ERR_INVALID, "contribution buffers required with data");
  DiscSets sets;
  if (int rc = resolve_disc_sets(make_idx_map(d_names, n_nodes), t_node_names, n_t_nodes, ma_names, ma_labels,
                                 n_assign, modules, n_modules, degree_len, corr_len,
                                 with_data ? contribution_len : nullptr, sets))
    return rc;
  if (sets.which.empty()) return NR_OK;
  // The discovery dataset stays resident across the calls of one discovery
  // dataset's loop over test datasets (the reference loads it once per di,
  // R/modulePreservation.R:553-590): uploaded only when these arrays are not
  // the resident ones.
  std::lock_guard<std::mutex> res_lk(g_res_mu);
  int rc = NR_OK;
  if (!g_disc_res.holds(d_data, d_corr, d_net, n_samples, n_nodes)) {
    g_disc_res.drop();
    CtxPtr ctx;
    if ((rc = open_ctx(0, ctx))) return rc;
    rc = nr_set_dataset(ctx.get(), d_corr, d_net, d_data, n_nodes, n_samples, NR_HOST);
    if (rc) return ctx_err(rc, ctx.get());
    g_disc_res.keep(std::move(ctx), d_data, d_corr, d_net, n_samples, n_nodes);
  }
  return disc_vectors(g_disc_res.ctx.get(), sets, with_data, degree_out, degree_len, corr_out, corr_len,
                      contribution_out, contribution_len);
} catch (const std::bad_alloc&) {
  return set_err(NR_ERR_OOM, "host memory allocation failed");
} catch (const std::exception& e) {
  return set_err(NR_ERR_INVALID, std::string("internal error: ") + e.what());
}

int netrep_NetProps(const double* data, const double* net, int64_t n_samples, int64_t n_nodes,
                    const char* const* node_names, const char* const* ma_names,
                    const char* const* ma_labels, int64_t n_assign, const char* const* modules,
                    int64_t n_modules, double* degree_out, double* contribution_out,
                    double* summary_out, double* coherence_out, double* avg_weight_out,
                    int64_t* k_all_out) try {
  if (!net || !node_names || !ma_names || !ma_labels || !modules || !degree_out ||
      !avg_weight_out || !k_all_out || n_nodes <= 0)
    return set_err(NR_ERR_INVALID, "invalid arguments to NetProps");
  const bool with_data = data != nullptr;
  if (with_data && (!contribution_out || !summary_out || !coherence_out))
    return set_err(NR_ERR_INVALID, "contribution/summary/coherence buffers required with data");
  PropSets sets;
  resolve_prop_sets(make_idx_map(node_names, n_nodes), ma_names, ma_labels, n_assign, modules, n_modules, with_data,
                    n_samples, degree_out, contribution_out, summary_out, coherence_out, avg_weight_out, k_all_out,
                    sets);
  if (sets.which.empty()) return NR_OK;
  // NetProps scales internally (src/properties.cpp:49): the raw data is
  // scaled on the device on its way into HBM. No correlation matrix on this
  // path: the network doubles as the (unused) correlation operand and
  // crosses PCIe once. The dataset stays resident while later calls name the
  // same arrays (networkProperties calls NetProps per (discovery, test) pair,
  // R/networkProperties.R:295-302).
  std::lock_guard<std::mutex> res_lk(g_res_mu);
  int rc = NR_OK;
  if (!g_props_res.holds(data, net, net, n_samples, n_nodes)) {
    g_props_res.drop();
    CtxPtr ctx;
    if ((rc = open_ctx(0, ctx))) return rc;
    rc = nr_set_dataset_ex(ctx.get(), net, net, data, n_nodes, n_samples, NR_HOST, with_data ? NR_SCALE_DATA : 0);
    if (rc) return ctx_err(rc, ctx.get());
    g_props_res.keep(std::move(ctx), data, net, net, n_samples, n_nodes);
  }
  return prop_vectors(g_props_res.ctx.get(), sets, with_data, n_samples, degree_out, contribution_out, summary_out,
                      coherence_out, avg_weight_out);
} catch (const std::bad_alloc&) {
  return set_err(NR_ERR_OOM, "host memory allocation failed");
} catch (const std::exception& e) {
  return set_err(NR_ERR_INVALID, std::string("internal error: ") + e.what());
}

int netrep_Scale(const double* data, int64_t n_samples, int64_t n_nodes, double* scaled_out) try {
  if (!data || !scaled_out || n_samples <= 0 || n_nodes <= 0)
    return set_err(NR_ERR_INVALID, "invalid arguments to Scale");
  std::vector<CtxPtr> v(1);
  CtxLease lease{&v};
  int rc = open_ctx(0, v[0]);
  if (rc) return rc;
  rc = nr_scale(v[0].get(), data, n_samples, n_nodes, scaled_out);
  if (rc) return ctx_err(rc, v[0].get());
  return NR_OK;
} catch (const std::bad_alloc&) {
  return set_err(NR_ERR_OOM, "host memory allocation failed");
} catch (const std::exception& e) {
  return set_err(NR_ERR_INVALID, std::string("internal error: ") + e.what());
}

int netrep_CheckFinite(const double* mat, int64_t nrow, int64_t ncol) try {
  if (!mat || nrow < 0 || ncol < 0) return set_err(NR_ERR_INVALID, "invalid arguments to CheckFinite");
  std::vector<CtxPtr> v(1);
  CtxLease lease{&v};
  int rc = open_ctx(0, v[0]);
  if (rc) return rc;
  int ok = 1;
  rc = nr_check_finite(v[0].get(), mat, nrow * ncol, &ok);
  if (rc) return ctx_err(rc, v[0].get());
  if (!ok) return set_err(NR_ERR_NONFINITE, "matrices cannot have non-finite or missing values");
  return NR_OK;
} catch (const std::bad_alloc&) {
  return set_err(NR_ERR_OOM, "host memory allocation failed");
} catch (const std::exception& e) {
  return set_err(NR_ERR_INVALID, std::string("internal error: ") + e.what());
}

int netrep_DatasetFromData(const double* data, int32_t scale_data, int32_t net_type, double beta, int64_t n_samples,
                           int64_t n_nodes, const char* const* node_names, int32_t n_cores,
                           netrep_dataset** out) try {
  if (out) *out = nullptr;
  if (int rc = check_from_data_args(data, net_type, beta, n_samples, n_nodes)) return rc;
  if (!node_names || !out) return set_err(NR_ERR_INVALID, "invalid arguments to DatasetFromData");
  std::unique_ptr<netrep_dataset> d(new netrep_dataset());
  d->names.reserve((size_t)n_nodes);
  for (int64_t i = 0; i < n_nodes; ++i) {
    if (!node_names[i]) return set_err(NR_ERR_INVALID, "invalid arguments to DatasetFromData (a NULL node name)");
    d->names.emplace_back(node_names[i]);
  }
  for (const std::string& s : d->names) d->name_ptrs.push_back(s.c_str());
  d->idx_map = make_idx_map(d->name_ptrs.data(), n_nodes);
  d->n_nodes = n_nodes;
  d->n_samples = n_samples;
  d->n_cores = n_cores;
  int rc = dataset_from_data_once(data, scale_data, net_type, beta, n_samples, n_nodes, n_cores, d->ctx);
  if (rc == NR_ERR_OOM) {  // as netrep_PermutationProcedureFromData: free what is held between calls, once
    netrep_ReleaseResident();
    rc = dataset_from_data_once(data, scale_data, net_type, beta, n_samples, n_nodes, n_cores, d->ctx);
  }
  if (rc) return rc;
  *out = d.release();
  return NR_OK;
} catch (const std::bad_alloc&) {
  return set_err(NR_ERR_OOM, "host memory allocation failed");
} catch (const std::exception& e) {
  return set_err(NR_ERR_INVALID, std::string("internal error: ") + e.what());
}

void netrep_DatasetRelease(netrep_dataset* d) {
  if (!d) return;
  { std::lock_guard<std::mutex> lk(d->mu); }  // a call in flight on another thread finishes first
  delete d;
}

int netrep_DatasetShape(netrep_dataset* d, int64_t* n_nodes, int64_t* n_samples) {
  if (!d) return set_err(NR_ERR_INVALID, "invalid arguments to DatasetShape (no dataset)");
  if (n_nodes) *n_nodes = d->n_nodes;
  if (n_samples) *n_samples = d->n_samples;
  return NR_OK;
}

int netrep_DatasetMatrices(netrep_dataset* d, double* corr_out, double* net_out) try {
  if (!d) return no_dataset("DatasetMatrices");
  std::lock_guard<std::mutex> lk(d->mu);
  if (int rc = live(d)) return rc;
  const int rc = nr_get_dataset_matrices(d->ctx.get(), corr_out, net_out);
  return rc ? ctx_err(rc, d->ctx.get()) : NR_OK;
} catch (const std::bad_alloc&) {
  return set_err(NR_ERR_OOM, "host memory allocation failed");
} catch (const std::exception& e) {
  return set_err(NR_ERR_INVALID, std::string("internal error: ") + e.what());
}

int netrep_DatasetIntermediateProperties(netrep_dataset* d, const char* const* t_node_names, int64_t n_t_nodes,
                                         const char* const* ma_names, const char* const* ma_labels,
                                         int64_t n_assign, const char* const* modules, int64_t n_modules,
                                         double* degree_out, int64_t* degree_len, double* corr_out,
                                         int64_t* corr_len, double* contribution_out,
                                         int64_t* contribution_len) try {
  if (!d) return no_dataset("DatasetIntermediateProperties");
  if (!t_node_names || !ma_names || !ma_labels || !modules || !degree_out || !degree_len || !corr_out ||
      !corr_len || !contribution_out || !contribution_len)
    return set_err(NR_ERR_INVALID, "invalid arguments to DatasetIntermediateProperties");
  std::lock_guard<std::mutex> lk(d->mu);
  if (int rc = live(d)) return rc;
  DiscSets sets;
  if (int rc = resolve_disc_sets(d->idx_map, t_node_names, n_t_nodes, ma_names, ma_labels, n_assign, modules,
                                 n_modules, degree_len, corr_len, contribution_len, sets))
    return rc;
  if (sets.which.empty()) return NR_OK;
  return disc_vectors(d->ctx.get(), sets, true, degree_out, degree_len, corr_out, corr_len, contribution_out,
                      contribution_len);
} catch (const std::bad_alloc&) {
  return set_err(NR_ERR_OOM, "host memory allocation failed");
} catch (const std::exception& e) {
  return set_err(NR_ERR_INVALID, std::string("internal error: ") + e.what());
}

int netrep_DatasetNetProps(netrep_dataset* d, const char* const* ma_names, const char* const* ma_labels,
                           int64_t n_assign, const char* const* modules, int64_t n_modules, double* degree_out,
                           double* contribution_out, double* summary_out, double* coherence_out,
                           double* avg_weight_out, int64_t* k_all_out) try {
  if (!d) return no_dataset("DatasetNetProps");
  if (!ma_names || !ma_labels || !modules || !degree_out || !contribution_out || !summary_out || !coherence_out ||
      !avg_weight_out || !k_all_out)
    return set_err(NR_ERR_INVALID, "invalid arguments to DatasetNetProps");
  std::lock_guard<std::mutex> lk(d->mu);
  if (int rc = live(d)) return rc;
  PropSets sets;
  resolve_prop_sets(d->idx_map, ma_names, ma_labels, n_assign, modules, n_modules, true, d->n_samples, degree_out,
                    contribution_out, summary_out, coherence_out, avg_weight_out, k_all_out, sets);
  if (sets.which.empty()) return NR_OK;
  return prop_vectors(d->ctx.get(), sets, true, d->n_samples, degree_out, contribution_out, summary_out,
                      coherence_out, avg_weight_out);
} catch (const std::bad_alloc&) {
  return set_err(NR_ERR_OOM, "host memory allocation failed");
} catch (const std::exception& e) {
  return set_err(NR_ERR_INVALID, std::string("internal error: ") + e.what());
}

int netrep_DatasetPermutationProcedure(const netrep_disc_props* disc, netrep_dataset* d,
                                       const char* const* ma_names, const char* const* ma_labels, int64_t n_assign,
                                       const char* const* modules, int64_t n_modules, int64_t n_perm,
                                       int32_t n_cores, const char* null_hypothesis, int32_t verbose, uint64_t seed,
                                       const uint32_t* pi, double* nulls_out, double* observed_out) try {
  if (!d) return no_dataset("DatasetPermutationProcedure");
  if (!disc || !ma_names || !ma_labels || !modules || !observed_out || n_perm < 0 || (n_perm > 0 && !nulls_out))
    return set_err(NR_ERR_INVALID, "invalid arguments to DatasetPermutationProcedure");
  std::lock_guard<std::mutex> lk(d->mu);
  if (int rc = live(d)) return rc;
  // the handle's context is the run's primary one and comes back on every return
  const int rc = permutation_impl(disc, true, nullptr, nullptr, nullptr, d->n_samples, d->n_nodes,
                                  d->name_ptrs.data(), ma_names, ma_labels, n_assign, modules, n_modules, n_perm,
                                  null_hypothesis, verbose, seed, pi, nulls_out, observed_out, std::move(d->ctx),
                                  n_cores, -1, &d->ctx);
  if (nr_ctx* c = d->ctx.get()) {
    if (rc == NR_ERR_CANCELLED) {
      // a cancellation that reached the context after its run had returned is
      // consumed by an empty run, so the next call on the handle starts clean
      double none = 0.0;
      (void)nr_run(c, 0, 0, seed, nullptr, &none);
    }
    // between calls the handle holds its dataset only, as a pooled context holds nothing
    (void)nr_release_scratch(c);
    (void)nr_ctx_set_host_threads(c, d->n_cores != 0 ? d->n_cores : nr_get_host_threads());
  }
  return rc;
} catch (const std::bad_alloc&) {
  return set_err(NR_ERR_OOM, "host memory allocation failed");
} catch (const std::exception& e) {
  return set_err(NR_ERR_INVALID, std::string("internal error: ") + e.what());
}

int netrep_HclustFinish(int64_t n, const int32_t* id_lo, const int32_t* id_hi, const double* height_in,
                        int32_t* merge, double* height, int32_t* order, int32_t* n_repairs) try {
  if (n < 1 || !order || (n > 1 && (!id_lo || !id_hi || !height_in || !merge || !height)))
    return set_err(NR_ERR_INVALID, "invalid arguments to HclustFinish");
  if (!nr::hclust_finish(n, id_lo, id_hi, height_in, merge, height, order, n_repairs))
    return set_err(NR_ERR_INVALID, "invalid arguments to HclustFinish (not a binary tree in construction order, "
                                   "a NaN height, or more than 2^30 nodes)");
  return NR_OK;
} catch (const std::bad_alloc&) {
  return set_err(NR_ERR_OOM, "host memory allocation failed");
} catch (const std::exception& e) {
  return set_err(NR_ERR_INVALID, std::string("internal error: ") + e.what());
}

int netrep_CutreeStatic(int64_t n, const int32_t* merge, const double* height, double cut_height, int64_t min_size,
                        int32_t* labels) try {
  if (n < 1 || !labels || (n > 1 && (!merge || !height)))
    return set_err(NR_ERR_INVALID, "invalid arguments to CutreeStatic");
  if (!nr::cutree_static(n, merge, height, cut_height, min_size, labels))
    return set_err(NR_ERR_INVALID, "invalid arguments to CutreeStatic (a NaN, or merge is not an hclust merge matrix)");
  return NR_OK;
} catch (const std::bad_alloc&) {
  return set_err(NR_ERR_OOM, "host memory allocation failed");
} catch (const std::exception& e) {
  return set_err(NR_ERR_INVALID, std::string("internal error: ") + e.what());
}

int netrep_DatasetHclust(netrep_dataset* d, int32_t* merge, double* height, int32_t* order,
                         int32_t* n_repairs) try {
  if (!d) return no_dataset("DatasetHclust");
  if (!order || (d->n_nodes > 1 && (!merge || !height)))
    return set_err(NR_ERR_INVALID, "invalid arguments to DatasetHclust");
  std::lock_guard<std::mutex> lk(d->mu);
  if (int rc = live(d)) return rc;
  nr_ctx* const c = d->ctx.get();
  const size_t m = (size_t)(d->n_nodes - 1);
  std::vector<int32_t> id_lo(m), id_hi(m);
  std::vector<double> h(m), size(m);
  // The chain runs on a worker thread; the calling thread polls the interrupt
  // hook every 100 ms, as the permutation path does, and returns as soon as
  // the worker is done.
  std::atomic<bool> finished{false};
  int rc = NR_OK;
  std::thread worker([&]() {
    rc = nr_hclust_average(c, id_lo.data(), id_hi.data(), h.data(), size.data());
    finished.store(true);
  });
  bool interrupted = false;
  for (int tick = 0; !finished.load(); ++tick) {
    std::this_thread::sleep_for(std::chrono::milliseconds(1));
    if (tick % 100 == 99 && !interrupted && interrupt_requested()) {
      interrupted = true;
      nr_cancel(c);
    }
  }
  worker.join();
  if (interrupted && rc == NR_OK) {
    // A cancellation that reached the context after its last launch is still
    // pending: a call that finds one consumes it and returns at once, so the
    // next call on the handle starts clean, and the interrupt is reported.
    if (nr_hclust_average(c, nullptr, nullptr, nullptr, nullptr) == NR_ERR_CANCELLED) rc = NR_ERR_CANCELLED;
  }
  if (rc) return ctx_err(rc, c);
  if (!nr::hclust_finish(d->n_nodes, id_lo.data(), id_hi.data(), h.data(), merge, height, order, n_repairs))
    return set_err(NR_ERR_INTERNAL, "hclust: the device returned merges that are not a binary tree");
  return NR_OK;
} catch (const std::bad_alloc&) {
  return set_err(NR_ERR_OOM, "host memory allocation failed");
} catch (const std::exception& e) {
  return set_err(NR_ERR_INVALID, std::string("internal error: ") + e.what());
}

int netrep_EigengeneGroups(const double* eig, int64_t n_samples, int64_t n_mod, double cut_height,
                           int32_t* group_out, double* height_out) try {
  if (!eig || !group_out || n_samples < 2 || n_mod < 1 || (n_mod > 1 && !height_out))
    return set_err(NR_ERR_INVALID, "invalid arguments to EigengeneGroups");
  if (!(cut_height >= 0.0 && cut_height <= 2.0))
    return set_err(NR_ERR_INVALID, "invalid arguments to EigengeneGroups (cut_height outside [0, 2])");
  if (!nr::eigengene_groups(eig, n_samples, n_mod, cut_height, group_out, height_out))
    return set_err(NR_ERR_INVALID, "invalid arguments to EigengeneGroups (a non-finite or constant eigengene)");
  return NR_OK;
} catch (const std::bad_alloc&) {
  return set_err(NR_ERR_OOM, "host memory allocation failed");
}

int netrep_MergeLabels(int64_t n, const int32_t* labels_in, int64_t n_mod, const int32_t* module_labels,
                       const int32_t* group, int32_t relabel, int32_t* labels_out) try {
  if (n < 1 || !labels_in || n_mod < 0 || (n_mod > 0 && (!module_labels || !group)) || !labels_out)
    return set_err(NR_ERR_INVALID, "invalid arguments to MergeLabels");
  for (int64_t i = 0; i < n; ++i)
    if (labels_in[i] < 0) return set_err(NR_ERR_INVALID, "invalid arguments to MergeLabels (a negative label)");
  if (!nr::merge_labels(n, labels_in, n_mod, module_labels, group, relabel != 0, labels_out))
    return set_err(NR_ERR_INVALID, "invalid arguments to MergeLabels (a label missing from module_labels, a module "
                                   "label not positive or given twice, or group[m] outside 0 .. m)");
  return NR_OK;
} catch (const std::bad_alloc&) {
  return set_err(NR_ERR_OOM, "host memory allocation failed");
}

int netrep_TrimModulesKME(int64_t n, const int32_t* labels_in, const double* kme_own, double min_kme_to_stay,
                          double min_core_kme, int64_t min_core_kme_size, int64_t min_size,
                          int32_t* labels_out) try {
  if (n < 1 || !labels_in || !kme_own || !labels_out || std::isnan(min_kme_to_stay) || std::isnan(min_core_kme))
    return set_err(NR_ERR_INVALID, "invalid arguments to TrimModulesKME");
  for (int64_t i = 0; i < n; ++i)
    if (labels_in[i] < 0) return set_err(NR_ERR_INVALID, "invalid arguments to TrimModulesKME (a negative label)");
  nr::trim_modules_kme(n, labels_in, kme_own, min_kme_to_stay, min_core_kme, min_core_kme_size, min_size, labels_out);
  return NR_OK;
} catch (const std::bad_alloc&) {
  return set_err(NR_ERR_OOM, "host memory allocation failed");
}

int netrep_DatasetModuleEigengenes(netrep_dataset* d, const int32_t* labels, int32_t* n_mod_out,
                                   int32_t* module_labels_out, double* eigengenes, double* var_explained,
                                   double* kme_own) try {
  if (!d) return no_dataset("DatasetModuleEigengenes");
  if (!labels || !eigengenes || !var_explained)
    return set_err(NR_ERR_INVALID, "invalid arguments to DatasetModuleEigengenes");
  std::lock_guard<std::mutex> lk(d->mu);
  if (int rc = live(d)) return rc;
  LabelSets ls;
  if (int rc = resolve_labels("DatasetModuleEigengenes", d->n_nodes, labels, ls)) return rc;
  if (n_mod_out) *n_mod_out = (int32_t)ls.modules.size();
  if (module_labels_out) std::copy(ls.modules.begin(), ls.modules.end(), module_labels_out);
  const int rc = label_eigengenes(d, ls, eigengenes, var_explained, kme_own);
  (void)nr_release_scratch(d->ctx.get());
  return rc;
} catch (const std::bad_alloc&) {
  return set_err(NR_ERR_OOM, "host memory allocation failed");
} catch (const std::exception& e) {
  return set_err(NR_ERR_INVALID, std::string("internal error: ") + e.what());
}

int netrep_DatasetModuleMembership(netrep_dataset* d, const int32_t* labels, double* kme) try {
  if (!d) return no_dataset("DatasetModuleMembership");
  if (!labels || !kme) return set_err(NR_ERR_INVALID, "invalid arguments to DatasetModuleMembership");
  std::lock_guard<std::mutex> lk(d->mu);
  if (int rc = live(d)) return rc;
  LabelSets ls;
  if (int rc = resolve_labels("DatasetModuleMembership", d->n_nodes, labels, ls)) return rc;
  nr_ctx* const c = d->ctx.get();
  const size_t M = ls.modules.size();
  std::vector<double> eig((size_t)d->n_samples * M), ve(M);
  int rc = label_eigengenes(d, ls, eig.data(), ve.data(), nullptr);
  if (!rc && interrupt_requested()) rc = set_err(NR_ERR_CANCELLED, "interrupted");
  if (!rc) {
    rc = nr_module_membership(c, (int32_t)M, nullptr, kme);
    if (rc) rc = ctx_err(rc, c);
  }
  (void)nr_release_scratch(c);
  return rc;
} catch (const std::bad_alloc&) {
  return set_err(NR_ERR_OOM, "host memory allocation failed");
} catch (const std::exception& e) {
  return set_err(NR_ERR_INVALID, std::string("internal error: ") + e.what());
}

int netrep_EigengeneTree(const double* eig, int64_t n_samples, int64_t n_mod, int32_t linkage, int32_t* id_lo,
                         int32_t* id_hi, double* height) try {
  if (!eig || n_samples < 2 || n_mod < 1 || (n_mod > 1 && (!id_lo || !id_hi || !height)))
    return set_err(NR_ERR_INVALID, "invalid arguments to EigengeneTree");
  if (linkage != NR_LINKAGE_AVERAGE && linkage != NR_LINKAGE_COMPLETE)
    return set_err(NR_ERR_INVALID, "invalid arguments to EigengeneTree (linkage is neither average nor complete)");
  if (!nr::eigengene_tree(eig, n_samples, n_mod,
                          linkage == NR_LINKAGE_COMPLETE ? nr::kLinkageComplete : nr::kLinkageAverage, id_lo, id_hi,
                          height))
    return set_err(NR_ERR_INVALID, "invalid arguments to EigengeneTree (a non-finite or constant eigengene)");
  nr::tree_slots_to_ids(n_mod, id_lo, id_hi, id_lo, id_hi);
  return NR_OK;
} catch (const std::bad_alloc&) {
  return set_err(NR_ERR_OOM, "host memory allocation failed");
}

int netrep_IntramodularConnectivity(int64_t n, const int32_t* labels, const double* k_total, const double* k_mod,
                                    double* k_within, double* k_out, double* k_diff) try {
  if (n < 1 || !labels || !k_total || !k_mod || !k_within || !k_out || !k_diff)
    return set_err(NR_ERR_INVALID, "invalid arguments to IntramodularConnectivity");
  LabelSets ls;
  if (int rc = resolve_labels("IntramodularConnectivity", n, labels, ls)) return rc;
  const std::vector<int32_t> slot = slots_of(n, labels, ls);
  nr::intramodular_connectivity(n, slot.data(), k_total, k_mod, k_within, k_out, k_diff);
  return NR_OK;
} catch (const std::bad_alloc&) {
  return set_err(NR_ERR_OOM, "host memory allocation failed");
}

int netrep_DatasetModuleConnectivity(netrep_dataset* d, const int32_t* labels, double* k_total, double* k_mod) try {
  if (!d) return no_dataset("DatasetModuleConnectivity");
  if (!labels || !k_mod) return set_err(NR_ERR_INVALID, "invalid arguments to DatasetModuleConnectivity");
  std::lock_guard<std::mutex> lk(d->mu);
  if (int rc = live(d)) return rc;
  LabelSets ls;
  if (int rc = resolve_labels("DatasetModuleConnectivity", d->n_nodes, labels, ls)) return rc;
  return label_connectivity(d, labels, ls, k_total, k_mod);
} catch (const std::bad_alloc&) {
  return set_err(NR_ERR_OOM, "host memory allocation failed");
} catch (const std::exception& e) {
  return set_err(NR_ERR_INVALID, std::string("internal error: ") + e.what());
}

int netrep_DatasetIntramodularConnectivity(netrep_dataset* d, const int32_t* labels, double* k_total,
                                           double* k_within, double* k_out, double* k_diff) try {
  if (!d) return no_dataset("DatasetIntramodularConnectivity");
  if (!labels || !k_total || !k_within || !k_out || !k_diff)
    return set_err(NR_ERR_INVALID, "invalid arguments to DatasetIntramodularConnectivity");
  std::lock_guard<std::mutex> lk(d->mu);
  if (int rc = live(d)) return rc;
  LabelSets ls;
  if (int rc = resolve_labels("DatasetIntramodularConnectivity", d->n_nodes, labels, ls)) return rc;
  std::vector<double> k_mod((size_t)d->n_nodes * ls.modules.size());
  if (int rc = label_connectivity(d, labels, ls, k_total, k_mod.data())) return rc;
  const std::vector<int32_t> slot = slots_of(d->n_nodes, labels, ls);
  nr::intramodular_connectivity(d->n_nodes, slot.data(), k_total, k_mod.data(), k_within, k_out, k_diff);
  return NR_OK;
} catch (const std::bad_alloc&) {
  return set_err(NR_ERR_OOM, "host memory allocation failed");
} catch (const std::exception& e) {
  return set_err(NR_ERR_INVALID, std::string("internal error: ") + e.what());
}

int netrep_DatasetMergeCloseModules(netrep_dataset* d, const int32_t* labels_in, double cut_height, int32_t relabel,
                                    int32_t* labels_out, int32_t* n_rounds_out, int32_t* n_mod_last_out,
                                    double* eigengenes_last_out, double* heights_last_out) try {
  if (!d) return no_dataset("DatasetMergeCloseModules");
  if (!labels_in || !labels_out) return set_err(NR_ERR_INVALID, "invalid arguments to DatasetMergeCloseModules");
  if (!(cut_height >= 0.0 && cut_height <= 2.0))
    return set_err(NR_ERR_INVALID, "invalid arguments to DatasetMergeCloseModules (cut_height outside [0, 2])");
  std::lock_guard<std::mutex> lk(d->mu);
  if (int rc = live(d)) return rc;
  const int64_t n = d->n_nodes, S = d->n_samples;
  std::vector<int32_t> labels(labels_in, labels_in + n), group;
  std::vector<double> eig, ve, height;
  LabelSets ls;
  int32_t rounds = 0;
  int rc = NR_OK;
  for (;;) {
    if ((rc = resolve_labels("DatasetMergeCloseModules", n, labels.data(), ls))) break;
    const int64_t M = (int64_t)ls.modules.size();
    eig.resize((size_t)(S * M));
    ve.resize((size_t)M);
    group.assign((size_t)M, 0);
    height.assign((size_t)std::max<int64_t>(M - 1, 0), 0.0);
    if ((rc = label_eigengenes(d, ls, eig.data(), ve.data(), nullptr))) break;
    if (M == 1) break;
    if (!nr::eigengene_groups(eig.data(), S, M, cut_height, group.data(), height.data())) {
      rc = set_err(NR_ERR_NONFINITE, "mergeCloseModules: a non-finite or constant eigengene");
      break;
    }
    bool merged = false;
    for (int64_t m = 0; m < M; ++m) merged = merged || group[(size_t)m] != (int32_t)m;
    if (!merged) break;
    nr::merge_labels(n, labels.data(), M, ls.modules.data(), group.data(), false, labels.data());
    ++rounds;
  }
  (void)nr_release_scratch(d->ctx.get());
  if (rc) return rc;
  // ls, eig and height are the last round's: the final modules in increasing label order
  const size_t M = ls.modules.size();
  std::vector<int32_t> column_of(M);  // source column of each output column
  for (size_t m = 0; m < M; ++m) column_of[m] = (int32_t)m;
  if (relabel) {
    std::vector<int32_t> old_of_new;
    nr::relabel_by_size(n, labels.data(), labels.data(), &old_of_new);
    for (size_t m = 0; m < M; ++m)
      column_of[m] =
          (int32_t)(std::lower_bound(ls.modules.begin(), ls.modules.end(), old_of_new[m]) - ls.modules.begin());
  }
  std::copy(labels.begin(), labels.end(), labels_out);
  if (n_rounds_out) *n_rounds_out = rounds;
  if (n_mod_last_out) *n_mod_last_out = (int32_t)M;
  if (eigengenes_last_out)
    for (size_t m = 0; m < M; ++m)
      std::copy(eig.begin() + (size_t)column_of[m] * (size_t)S, eig.begin() + ((size_t)column_of[m] + 1) * (size_t)S,
                eigengenes_last_out + m * (size_t)S);
  if (heights_last_out) std::copy(height.begin(), height.end(), heights_last_out);
  return NR_OK;
} catch (const std::bad_alloc&) {
  return set_err(NR_ERR_OOM, "host memory allocation failed");
} catch (const std::exception& e) {
  return set_err(NR_ERR_INVALID, std::string("internal error: ") + e.what());
}

int netrep_DatasetTrimModules(netrep_dataset* d, const int32_t* labels_in, double min_kme_to_stay,
                              double min_core_kme, int64_t min_core_kme_size, int64_t min_size,
                              int32_t* labels_out) try {
  if (!d) return no_dataset("DatasetTrimModules");
  if (!labels_in || !labels_out || std::isnan(min_kme_to_stay) || std::isnan(min_core_kme))
    return set_err(NR_ERR_INVALID, "invalid arguments to DatasetTrimModules");
  std::lock_guard<std::mutex> lk(d->mu);
  if (int rc = live(d)) return rc;
  LabelSets ls;
  if (int rc = resolve_labels("DatasetTrimModules", d->n_nodes, labels_in, ls)) return rc;
  const size_t M = ls.modules.size();
  std::vector<double> eig((size_t)d->n_samples * M), ve(M), own((size_t)d->n_nodes);
  const int rc = label_eigengenes(d, ls, eig.data(), ve.data(), own.data());
  (void)nr_release_scratch(d->ctx.get());
  if (rc) return rc;
  nr::trim_modules_kme(d->n_nodes, labels_in, own.data(), min_kme_to_stay, min_core_kme, min_core_kme_size, min_size,
                       labels_out);
  return NR_OK;
} catch (const std::bad_alloc&) {
  return set_err(NR_ERR_OOM, "host memory allocation failed");
} catch (const std::exception& e) {
  return set_err(NR_ERR_INVALID, std::string("internal error: ") + e.what());
}

int netrep_IntermediatePropertiesFromData(const double* d_data, int32_t scale_data, int32_t net_type, double beta,
                                          int64_t n_samples, int64_t n_nodes, const char* const* d_names,
                                          const char* const* t_node_names, int64_t n_t_nodes,
                                          const char* const* ma_names, const char* const* ma_labels,
                                          int64_t n_assign, const char* const* modules, int64_t n_modules,
                                          double* degree_out, int64_t* degree_len, double* corr_out,
                                          int64_t* corr_len, double* contribution_out, int64_t* contribution_len) {
  if (int rc = check_from_data_args(d_data, net_type, beta, n_samples, n_nodes)) return rc;
  if (!d_names || !t_node_names || !ma_names || !ma_labels || !modules || !degree_out || !degree_len || !corr_out ||
      !corr_len || !contribution_out || !contribution_len)
    return set_err(NR_ERR_INVALID, "invalid arguments to IntermediatePropertiesFromData");
  netrep_dataset* d = nullptr;
  int rc = netrep_DatasetFromData(d_data, scale_data, net_type, beta, n_samples, n_nodes, d_names, 0, &d);
  if (rc) return rc;
  rc = netrep_DatasetIntermediateProperties(d, t_node_names, n_t_nodes, ma_names, ma_labels, n_assign, modules,
                                            n_modules, degree_out, degree_len, corr_out, corr_len, contribution_out,
                                            contribution_len);
  netrep_DatasetRelease(d);
  return rc;
}

int netrep_NetPropsFromData(const double* data, int32_t scale_data, int32_t net_type, double beta, int64_t n_samples,
                            int64_t n_nodes, const char* const* node_names, const char* const* ma_names,
                            const char* const* ma_labels, int64_t n_assign, const char* const* modules,
                            int64_t n_modules, double* degree_out, double* contribution_out, double* summary_out,
                            double* coherence_out, double* avg_weight_out, int64_t* k_all_out) {
  if (int rc = check_from_data_args(data, net_type, beta, n_samples, n_nodes)) return rc;
  if (!node_names || !ma_names || !ma_labels || !modules || !degree_out || !contribution_out || !summary_out ||
      !coherence_out || !avg_weight_out || !k_all_out)
    return set_err(NR_ERR_INVALID, "invalid arguments to NetPropsFromData");
  netrep_dataset* d = nullptr;
  int rc = netrep_DatasetFromData(data, scale_data, net_type, beta, n_samples, n_nodes, node_names, 0, &d);
  if (rc) return rc;
  rc = netrep_DatasetNetProps(d, ma_names, ma_labels, n_assign, modules, n_modules, degree_out, contribution_out,
                              summary_out, coherence_out, avg_weight_out, k_all_out);
  netrep_DatasetRelease(d);
  return rc;
}

}  // extern "C"
