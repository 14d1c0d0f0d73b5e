// Dataset residency of the C ABI (include/netrep_gpu.h): the routes that put
// a dataset into HBM (host or device matrices, the data matrix alone, files),
// its copies between contexts, and the queries and export of what is resident.
#include <algorithm>
#include <array>
#include <cmath>
#include <cstring>
#include <exception>
#include <new>
#include <set>

#include "engine_internal.h"
#include "hclust_host.h"
#include "kernels.h"
#include "rds_reader.h"

std::atomic<int64_t> g_h2d_bytes{0};

void reset_dataset(nr_ctx* ctx) {
  sync_obs(ctx);
  dfree(ctx->ds.d_pairs);
  dfree(ctx->ds.d_data);
  dfree(ctx->ds.d_colsum);
  ctx->ds = Dataset();
  ctx->table_checked = -1;
  ++ctx->data_gen;
}

namespace {

// The device buffers of a dataset in a fixed order (pairs, data, colsum), and
// their sizes: the {corr, net} array in its layout (pairs_es), the data block
// with its two virtual columns, the column sums. 0: the dataset has none.
using Buffers = std::array<char*, 3>;
using BufferBytes = std::array<size_t, 3>;

Buffers buffers_of(const Dataset& ds) {
  return {reinterpret_cast<char*>(ds.d_pairs), reinterpret_cast<char*>(ds.d_data),
          reinterpret_cast<char*>(ds.d_colsum)};
}

BufferBytes buffer_bytes_of(const Dataset& ds) {
  const size_t n = (size_t)ds.n_nodes;
  return {n * n * sizeof(double2) * (size_t)ds.pairs_es,
          ds.d_data ? (size_t)ds.n_samples * (n + 2) * sizeof(double) : 0,
          ds.d_colsum ? n * sizeof(double) : 0};
}

hipError_t alloc_buffers(Dataset& ds, const BufferBytes& bytes) {
  hipError_t e = hipMalloc((void**)&ds.d_pairs, bytes[0]);
  if (e == hipSuccess && bytes[1]) e = hipMalloc((void**)&ds.d_data, bytes[1]);
  if (e == hipSuccess && bytes[2]) e = hipMalloc((void**)&ds.d_colsum, bytes[2]);
  return e;
}

// Everything a copy of `src` carries except the device buffers, which the
// copy routes allocate and fill themselves.
void copy_dataset_fields(Dataset& dst, const Dataset& src) {
  Dataset d = src;
  d.d_pairs = dst.d_pairs;
  d.d_data = dst.d_data;
  d.d_colsum = dst.d_colsum;
  dst = std::move(d);
}

// Replace the context's dataset by the one `body(Dataset&)` builds. The old
// dataset is dropped first; on any failure the context is left with no
// dataset at all (never a new buffer with the old shape), and modules set
// for the old dataset are invalidated either way. No exception of the host
// code in `body` crosses the C ABI.
template <typename Body>
int replace_dataset(nr_ctx* ctx, Body body) {
  NR_HIP(ctx, hipSetDevice(ctx->device));
  NR_HIP(ctx, hipStreamSynchronize(ctx->stream));
  reset_dataset(ctx);
  int rc;
  try {
    rc = body(ctx->ds);
  } catch (const std::bad_alloc&) {
    rc = fail(ctx, NR_ERR_OOM, "host memory allocation failed");
  } catch (const std::exception& ex) {
    rc = fail(ctx, NR_ERR_INVALID, std::string("internal error: ") + ex.what());
  }
  if (rc != NR_OK) {
    (void)hipStreamSynchronize(ctx->stream);
    reset_dataset(ctx);
  }
  return rc;
}

// Zero the flag counter, run `pass` (the symmetry pass or the from-data
// build, which |= 1 for an asymmetric pair, 2 for a non-finite corr, 4 for a
// non-finite net), read it back and decode it into the dataset's flags.
template <typename Pass>
int read_flags(nr_ctx* ctx, Dataset& ds, const char* what, Pass pass) {
  int bits = 0;
  hipError_t e = hipMemsetAsync(ctx->d_counters + 5, 0, sizeof(int), ctx->stream);
  if (e == hipSuccess) e = pass(ctx->d_counters + 5);
  if (e == hipSuccess)
    e = hipMemcpyAsync(&bits, ctx->d_counters + 5, sizeof(int), hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) return hip_fail(ctx, e, what);
  ds.symmetric = (bits & 1) ? 0 : 1;
  ds.corr_finite = (bits & 2) ? 0 : 1;
  ds.net_finite = (bits & 4) ? 0 : 1;
  return NR_OK;
}

// n doubles through two pinned host buffers (and two device buffers of
// d_elems doubles, 0: none) in chunks of `chunk`: fill(h, o, len) puts chunk
// [o, o + len) into pinned buffer h on the host (false: stop), while the
// stream still works on the previous chunk that send(h, d, o, len) queued.
template <typename Fill, typename Send>
hipError_t stage_chunks(int64_t n, int64_t chunk, size_t h_elems, size_t d_elems, hipStream_t st, Fill fill,
                        Send send) {
  double* h[2] = {nullptr, nullptr};
  double* d[2] = {nullptr, nullptr};
  hipEvent_t ev[2] = {nullptr, nullptr};
  hipError_t e = hipSuccess;
  for (int b = 0; b < 2 && e == hipSuccess; ++b) {
    e = hipHostMalloc((void**)&h[b], h_elems * sizeof(double), hipHostMallocDefault);
    if (e == hipSuccess && d_elems) e = hipMalloc((void**)&d[b], d_elems * sizeof(double));
    if (e == hipSuccess) e = hipEventCreateWithFlags(&ev[b], hipEventDisableTiming);
  }
  int64_t i = 0;
  for (int64_t o = 0; o < n && e == hipSuccess; o += chunk, ++i) {
    const int b = (int)(i & 1);
    const int64_t len = std::min(chunk, n - o);
    if (i >= 2) e = hipEventSynchronize(ev[b]);  // chunk i-2 has left buffer b
    if (e != hipSuccess || !fill(h[b], o, len)) break;
    e = send(h[b], d[b], o, len);
    if (e == hipSuccess) e = hipEventRecord(ev[b], st);
  }
  const hipError_t e2 = hipStreamSynchronize(st);
  if (e == hipSuccess) e = e2;
  for (int b = 0; b < 2; ++b) {
    if (h[b]) (void)hipHostFree(h[b]);
    if (d[b]) (void)hipFree(d[b]);
    if (ev[b]) (void)hipEventDestroy(ev[b]);
  }
  return e;
}

// Host matrices to HBM through pinned, double-buffered chunks: host threads
// fill a pinned buffer with chunk i+1 (from the caller's pageable arrays)
// while the copy engine moves chunk i and, for the corr/net pair, the
// interleave kernel packs it into the {corr, net} layout. `net` NULL: a plain
// copy of `corr` into `dst_plain`. net == corr (NetProps: the network doubles
// as the unused correlation operand): the matrix crosses PCIe once and fills
// both halves of the pairs.
int upload_pinned(nr_ctx* ctx, const double* corr, const double* net, int64_t n_elem, double2* dst_pairs,
                  double* dst_plain, hipStream_t st) {
  const bool same = net != nullptr && net == corr;
  const int parts = net && !same ? 2 : 1;
  const int threads = ctx->host_threads;
  const int64_t chunk = std::min<int64_t>(n_elem, (int64_t)1 << 23);  // 64 MiB per matrix per chunk
  const hipError_t e = stage_chunks(
      n_elem, chunk, (size_t)(parts * chunk), net ? (size_t)(parts * chunk) : 0, st,
      [&](double* h, int64_t o, int64_t len) {
        parallel_copy(h, corr + o, len, threads);
        if (parts == 2) parallel_copy(h + chunk, net + o, len, threads);
        return true;
      },
      [&](double* h, double* d, int64_t o, int64_t len) {
        if (!net) return h2d_async(dst_plain + o, h, (size_t)len * sizeof(double), st);
        hipError_t e = h2d_async(d, h, (size_t)len * sizeof(double), st);
        if (e == hipSuccess && parts == 2) e = h2d_async(d + chunk, h + chunk, (size_t)len * sizeof(double), st);
        if (e == hipSuccess) e = nr::launch_interleave(d, parts == 2 ? d + chunk : d, dst_pairs + o, len, st);
        return e;
      });
  if (e != hipSuccess) return hip_fail(ctx, e, "dataset upload");
  return NR_OK;
}

// File -> pinned -> HBM for one matrix payload: the host inflates / reads
// straight into a pinned buffer while the copy engine moves the previous one
// and a kernel converts it from XDR into `pairs` (half 0 / 1) or `plain`.
int upload_file_matrix(nr_ctx* ctx, nr::RMatrixReader& rd, double2* pairs, int half, double* plain,
                       hipStream_t st) {
  const int64_t n = rd.length();
  const int64_t chunk = std::min<int64_t>(std::max<int64_t>(n, 1), (int64_t)1 << 23);  // 64 MiB
  bool read_ok = true;
  const hipError_t e = stage_chunks(
      n, chunk, (size_t)chunk, (size_t)chunk, st,
      [&](double* h, int64_t, int64_t len) { return read_ok = rd.read_raw(h, len); },
      [&](double* h, double* d, int64_t o, int64_t len) {
        const hipError_t e = h2d_async(d, h, (size_t)len * sizeof(double), st);
        if (e != hipSuccess) return e;
        return nr::launch_xdr(d, pairs ? pairs + o : nullptr, half, plain ? plain + o : nullptr, len, st);
      });
  if (!read_ok) return fail(ctx, NR_ERR_INVALID, rd.error());
  if (e != hipSuccess) return hip_fail(ctx, e, "file upload");
  return NR_OK;
}

__global__ void fill_kernel(double* p, int64_t n, double v) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    p[i] = v;
}

// The resident data block: n_samples x n_nodes values and, behind them, the
// Gram's virtual columns (column N all ones, column N + 1 zeros,
// ProfileParams::ones_off). put(dst) queues the raw values into dst on the
// context's stream (pinned upload, device-to-device copy or file upload):
// straight into the block, or with `scale` into a raw buffer that is scaled
// on the device (Scale, src/scale.cpp:14-25) into the block.
template <typename Put>
int load_data_block(nr_ctx* ctx, Dataset& ds, int64_t n_nodes, int64_t n_samples, bool scale, Put put) {
  const size_t bytes = (size_t)(n_samples * n_nodes) * sizeof(double);
  NR_HIP(ctx, hipMalloc((void**)&ds.d_data, bytes + 2 * (size_t)n_samples * sizeof(double)));
  double* ones = ds.d_data + n_nodes * n_samples;
  hipLaunchKernelGGL(fill_kernel, dim3(64), dim3(256), 0, ctx->stream, ones, n_samples, 1.0);
  NR_HIP(ctx, hipGetLastError());
  NR_HIP(ctx, hipMemsetAsync(ones + n_samples, 0, (size_t)n_samples * sizeof(double), ctx->stream));
  double* raw = nullptr;
  if (scale) NR_HIP(ctx, hipMalloc((void**)&raw, bytes));
  int rc = put(raw ? raw : ds.d_data);
  if (!rc) {
    hipError_t e = raw ? nr::launch_scale(raw, ds.d_data, n_samples, n_nodes, ctx->stream) : hipSuccess;
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) rc = hip_fail(ctx, e, raw ? "scale" : "data upload");
  }
  if (raw) (void)hipFree(raw);
  return rc;
}

// The caller's data matrix (host or device memory) into `dst`.
int put_data(nr_ctx* ctx, const double* data, int64_t n_elem, int where, double* dst) {
  if (where != NR_DEVICE) return upload_pinned(ctx, data, nullptr, n_elem, nullptr, dst, ctx->stream);
  const hipError_t e =
      hipMemcpyAsync(dst, data, (size_t)n_elem * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream);
  return e == hipSuccess ? NR_OK : hip_fail(ctx, e, "data copy");
}

int set_dataset_files_impl(nr_ctx* ctx, Dataset& ds, const char* corr_path, const char* net_path,
                           const char* data_path, const char* corr_object, const char* net_object,
                           const char* data_object, int scale_data) {
  nr::RMatrixReader rc_, rn_;
  if (!rc_.open(corr_path, corr_object)) return fail(ctx, NR_ERR_INVALID, std::string(corr_path) + ": " + rc_.error());
  if (!rn_.open(net_path, net_object)) return fail(ctx, NR_ERR_INVALID, std::string(net_path) + ": " + rn_.error());
  const int64_t n_elem = rc_.length();
  int64_t n_nodes = (int64_t)std::llround(std::sqrt((double)n_elem));
  if (n_nodes <= 0 || n_nodes * n_nodes != n_elem) return fail(ctx, NR_ERR_INVALID, "correlation matrix is not square");
  if (rn_.length() != n_elem) return fail(ctx, NR_ERR_INVALID, "network and correlation matrices differ in size");
  if (n_nodes > (int64_t)INT32_MAX) return fail(ctx, NR_ERR_UNSUPPORTED, "n_nodes exceeds 2^31-1");
  NR_HIP(ctx, hipMalloc((void**)&ds.d_pairs, (size_t)n_elem * sizeof(double2)));
  int rc;
  nr::RMatrixMeta mc, mn;
  if ((rc = upload_file_matrix(ctx, rc_, ds.d_pairs, 0, nullptr, ctx->stream))) return rc;
  if (!rc_.finish(&mc)) return fail(ctx, NR_ERR_INVALID, std::string(corr_path) + ": " + rc_.error());
  if ((rc = upload_file_matrix(ctx, rn_, ds.d_pairs, 1, nullptr, ctx->stream))) return rc;
  if (!rn_.finish(&mn)) return fail(ctx, NR_ERR_INVALID, std::string(net_path) + ": " + rn_.error());
  if (mc.nrow != n_nodes || mc.ncol != n_nodes || mn.nrow != n_nodes || mn.ncol != n_nodes)
    return fail(ctx, NR_ERR_INVALID, "correlation / network matrices must be square and of one size");
  // R/check-user-input.R:750-771: row and column names of each square matrix
  // agree, and the node order is the same in correlation, network and data
  if ((!mc.rownames.empty() && !mc.colnames.empty() && mc.rownames != mc.colnames) ||
      (!mn.rownames.empty() && !mn.colnames.empty() && mn.rownames != mn.colnames))
    return fail(ctx, NR_ERR_INVALID, "mismatch between row and column names in 'correlation' / 'network'");
  if (!mc.colnames.empty() && !mn.colnames.empty() && mc.colnames != mn.colnames)
    return fail(ctx, NR_ERR_INVALID, "mismatch in node order between 'data', 'correlation', and 'network'");
  const std::vector<std::string> names = !mn.colnames.empty() ? mn.colnames : mc.colnames;
  int64_t n_samples = 0;
  if (data_path) {
    nr::RMatrixReader rd;
    if (!rd.open(data_path, data_object)) return fail(ctx, NR_ERR_INVALID, std::string(data_path) + ": " + rd.error());
    if (rd.length() % n_nodes != 0) return fail(ctx, NR_ERR_INVALID, "data matrix columns do not match the network");
    n_samples = rd.length() / n_nodes;
    if (n_samples < 2) return fail(ctx, NR_ERR_INVALID, "data needs n_samples >= 2");
    // scaled on the device, as the R code scales after loading
    rc = load_data_block(ctx, ds, n_nodes, n_samples, scale_data != 0, [&](double* dst) {
      if (int r = upload_file_matrix(ctx, rd, nullptr, 0, dst, ctx->stream)) return r;
      nr::RMatrixMeta md;
      if (!rd.finish(&md)) return fail(ctx, NR_ERR_INVALID, std::string(data_path) + ": " + rd.error());
      if (md.nrow != n_samples || md.ncol != n_nodes)
        return fail(ctx, NR_ERR_INVALID, "data matrix must be samples x nodes");
      if (!md.colnames.empty() && !names.empty() && md.colnames != names)
        return fail(ctx, NR_ERR_INVALID, "mismatch in node order between 'data', 'correlation', and 'network'");
      return (int)NR_OK;
    });
    if (rc) return rc;
  }
  rc = read_flags(ctx, ds, "symmetry check",
                  [&](int* flag) { return nr::launch_symmetry(ds.d_pairs, n_nodes, flag, ctx->stream); });
  if (rc) return rc;
  ds.node_names = names;
  ds.n_nodes = n_nodes;
  ds.n_samples = n_samples;
  return NR_OK;
}

}  // namespace

extern "C" {

int nr_h2d_bytes(int64_t* bytes) {
  if (!bytes) return NR_ERR_INVALID;
  *bytes = g_h2d_bytes.load();
  return NR_OK;
}

int nr_set_dataset(nr_ctx* ctx, const double* corr, const double* net, const double* data,
                   int64_t n_nodes, int64_t n_samples, int where) {
  return nr_set_dataset_ex(ctx, corr, net, data, n_nodes, n_samples, where, 0);
}

int nr_set_dataset_ex(nr_ctx* ctx, const double* corr, const double* net, const double* data,
                      int64_t n_nodes, int64_t n_samples, int where, int flags) {
  if (!ctx) return NR_ERR_INVALID;
  if (flags & ~NR_SCALE_DATA) return fail(ctx, NR_ERR_INVALID, "unknown nr_set_dataset_ex flags");
  if (!corr || !net || n_nodes <= 0) return fail(ctx, NR_ERR_INVALID, "corr/net missing or n_nodes <= 0");
  if (data && n_samples < 2) return fail(ctx, NR_ERR_INVALID, "data needs n_samples >= 2");
  if (n_nodes > (int64_t)INT32_MAX) return fail(ctx, NR_ERR_UNSUPPORTED, "n_nodes exceeds 2^31-1");
  return replace_dataset(ctx, [&](Dataset& ds) -> int {
    const int64_t n_elem = n_nodes * n_nodes;
    NR_HIP(ctx, hipMalloc((void**)&ds.d_pairs, (size_t)n_elem * sizeof(double2)));
    if (where == NR_DEVICE) {
      NR_HIP(ctx, nr::launch_interleave(corr, net, ds.d_pairs, n_elem, ctx->stream));
    } else if (int rc = upload_pinned(ctx, corr, net, n_elem, ds.d_pairs, nullptr, ctx->stream)) {
      return rc;
    }
    int rc = read_flags(ctx, ds, "symmetry check",
                        [&](int* flag) { return nr::launch_symmetry(ds.d_pairs, n_nodes, flag, ctx->stream); });
    if (!rc && data)
      rc = load_data_block(ctx, ds, n_nodes, n_samples, (flags & NR_SCALE_DATA) != 0,
                           [&](double* dst) { return put_data(ctx, data, n_samples * n_nodes, where, dst); });
    if (rc) return rc;
    ds.n_nodes = n_nodes;
    ds.n_samples = data ? n_samples : 0;
    return NR_OK;
  });
}

int nr_set_dataset_from_data(nr_ctx* ctx, const double* data, int64_t n_nodes, int64_t n_samples, int where,
                             int flags, int net_type, double beta) {
  if (!ctx) return NR_ERR_INVALID;
  if (flags & ~NR_SCALE_DATA) return fail(ctx, NR_ERR_INVALID, "unknown nr_set_dataset_from_data flags");
  if (!data) return fail(ctx, NR_ERR_INVALID, "data missing");
  if (n_nodes < 1 || n_samples < 2) return fail(ctx, NR_ERR_INVALID, "data needs n_nodes >= 1 and n_samples >= 2");
  if (where != NR_HOST && where != NR_DEVICE) return fail(ctx, NR_ERR_INVALID, "where must be NR_HOST or NR_DEVICE");
  const int cor_type = net_type & (NR_COR_SPEARMAN | NR_COR_BICOR);
  const int base_type = net_type & ~(NR_NET_TOM | NR_COR_SPEARMAN | NR_COR_BICOR);
  const bool tom = (net_type & NR_NET_TOM) != 0;
  if (base_type != NR_NET_UNSIGNED && base_type != NR_NET_SIGNED && base_type != NR_NET_SIGNED_HYBRID)
    return fail(ctx, NR_ERR_INVALID, "unknown network type");
  if (cor_type == (NR_COR_SPEARMAN | NR_COR_BICOR)) return fail(ctx, NR_ERR_INVALID, "unknown correlation type");
  if (!std::isfinite(beta) || beta <= 0.0) return fail(ctx, NR_ERR_INVALID, "beta must be finite and > 0");
  if (n_nodes > (int64_t)INT32_MAX) return fail(ctx, NR_ERR_UNSUPPORTED, "n_nodes exceeds 2^31-1");
  return replace_dataset(ctx, [&](Dataset& ds) -> int {
    const size_t pair_bytes = (size_t)n_nodes * (size_t)n_nodes * sizeof(double2);
    if (hipMalloc((void**)&ds.d_pairs, pair_bytes) != hipSuccess) {
      (void)hipGetLastError();
      return fail(ctx, NR_ERR_OOM,
                  "from-data dataset: allocation of the " + std::to_string(pair_bytes >> 20) +
                      " MiB {corr, net} array failed (16 bytes per matrix element)");
    }
    int rc = load_data_block(ctx, ds, n_nodes, n_samples, (flags & NR_SCALE_DATA) != 0,
                             [&](double* dst) { return put_data(ctx, data, n_samples * n_nodes, where, dst); });
    if (rc) return rc;
    // The TOM scratch (kernels.h, launch_tom): the plain adjacency A,
    // column-major, n rows x (n + 2) columns, and the n degrees behind it:
    // 8 n (n + 2) + 8 n bytes. Padding rule (the data block's): columns
    // 0 .. n - 1 hold values (zero diagonal); column n + 1 is all zeros and is
    // what the SYRK main loop reads for every panel column past n; column n is
    // never read and is zeroed too. tom_extract_kernel writes all n + 2
    // columns. The scratch lives for this call only (freed on every path).
    struct Scratch {
      double* p = nullptr;
      ~Scratch() {
        if (p) (void)hipFree(p);
      }
    } tom_scratch, cor_scratch;
    // The correlation-type scratch (kernels.h, launch_cor_transform): Z in the
    // data block's shape, S x (n + 2) with both padding columns zero, and for
    // Spearman the plain S x n rank buffer behind it; for this call only.
    if (cor_type) {
      const size_t cor_bytes = nr::cor_scratch_bytes(n_nodes, n_samples, cor_type);
      if (hipMalloc((void**)&cor_scratch.p, cor_bytes) != hipSuccess) {
        (void)hipGetLastError();
        cor_scratch.p = nullptr;
        return fail(ctx, NR_ERR_OOM,
                    "from-data dataset: allocation of the " + std::to_string(cor_bytes) + "-byte (" +
                        std::to_string(cor_bytes >> 20) + " MiB) correlation-type scratch failed (8 S (n + 2)" +
                        (cor_type == NR_COR_SPEARMAN ? " + 8 S n" : "") + " bytes)");
      }
    }
    if (tom) {
      const size_t tom_bytes = nr::tom_scratch_bytes(n_nodes);
      if (hipMalloc((void**)&tom_scratch.p, tom_bytes) != hipSuccess) {
        (void)hipGetLastError();
        tom_scratch.p = nullptr;
        return fail(ctx, NR_ERR_OOM,
                    "from-data dataset: allocation of the " + std::to_string(tom_bytes) + "-byte (" +
                        std::to_string(tom_bytes >> 20) + " MiB) TOM scratch failed (8 n (n + 2) + 8 n bytes)");
      }
    }
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    hipEvent_t ev_cor = nullptr;  // the start of the transform step, which ends at ev[0]
    hipError_t e = hipSuccess;
    for (hipEvent_t& x : ev)
      if (e == hipSuccess) e = hipEventCreate(&x);
    if (e == hipSuccess && cor_type) e = hipEventCreate(&ev_cor);
    float ms = 0.f, ms_tom = 0.f, ms_cor = 0.f;
    // what netbuild_kernel runs on: the data block, or the transform's Z
    const double* const build_from = cor_type ? cor_scratch.p : ds.d_data;
    // one flag word for both epilogues: netbuild's, then the TOM's on top
    if (e == hipSuccess)
      rc = read_flags(ctx, ds, "from-data build", [&](int* flag) {
        hipError_t p = hipSuccess;
        if (cor_type) {
          p = hipEventRecord(ev_cor, ctx->stream);
          if (p == hipSuccess)
            p = nr::launch_cor_transform(ds.d_data, n_samples, n_nodes, cor_type, cor_scratch.p, ctx->stream);
        }
        if (p == hipSuccess) p = hipEventRecord(ev[0], ctx->stream);
        if (p == hipSuccess)
          p = nr::launch_netbuild(build_from, n_samples, n_nodes, ds.d_pairs, base_type, beta, flag, ctx->stream);
        if (p == hipSuccess) p = hipEventRecord(ev[1], ctx->stream);
        if (p == hipSuccess && tom) p = nr::launch_tom(n_nodes, ds.d_pairs, tom_scratch.p, flag, ctx->stream);
        if (p == hipSuccess) p = hipEventRecord(ev[2], ctx->stream);
        return p;
      });
    if (e == hipSuccess && !rc) e = hipEventElapsedTime(&ms, ev[0], ev[1]);
    if (e == hipSuccess && !rc && tom) e = hipEventElapsedTime(&ms_tom, ev[1], ev[2]);
    if (e == hipSuccess && !rc && cor_type) e = hipEventElapsedTime(&ms_cor, ev_cor, ev[0]);
    for (hipEvent_t x : ev)
      if (x) (void)hipEventDestroy(x);
    if (ev_cor) (void)hipEventDestroy(ev_cor);
    if (rc) return rc;
    if (e != hipSuccess) return hip_fail(ctx, e, "from-data build");
    ds.netbuild_ms = (double)ms;
    ds.tom_ms = (double)ms_tom;
    ds.cor_ms = (double)ms_cor;
    ds.symmetric = 1;  // every tile is stored and mirrored from the same bits
    ds.n_nodes = n_nodes;
    ds.n_samples = n_samples;
    return NR_OK;
  });
}

int nr_soft_connectivity(nr_ctx* ctx, const double* data, int64_t n_nodes, int64_t n_samples, int scale,
                         int net_type, const double* powers, int n_powers, double* k_out) {
  if (!ctx) return NR_ERR_INVALID;
  if (!data || !powers || !k_out) return fail(ctx, NR_ERR_INVALID, "data, powers or k_out missing");
  if (n_nodes < 1 || n_samples < 2) return fail(ctx, NR_ERR_INVALID, "data needs n_nodes >= 1 and n_samples >= 2");
  if (n_powers < 1 || n_powers > nr::kSftMaxPowers)
    return fail(ctx, NR_ERR_INVALID, "n_powers must be 1 .. " + std::to_string(nr::kSftMaxPowers));
  for (int m = 0; m < n_powers; ++m)
    if (!std::isfinite(powers[m]) || powers[m] <= 0.0) return fail(ctx, NR_ERR_INVALID, "powers must be finite and > 0");
  const int cor_type = net_type & (NR_COR_SPEARMAN | NR_COR_BICOR);
  const int base_type = net_type & ~(NR_COR_SPEARMAN | NR_COR_BICOR);
  if (net_type & NR_NET_TOM) return fail(ctx, NR_ERR_INVALID, "NR_NET_TOM has no soft-threshold connectivity");
  if (base_type != NR_NET_UNSIGNED && base_type != NR_NET_SIGNED && base_type != NR_NET_SIGNED_HYBRID)
    return fail(ctx, NR_ERR_INVALID, "unknown network type");
  if (cor_type == (NR_COR_SPEARMAN | NR_COR_BICOR)) return fail(ctx, NR_ERR_INVALID, "unknown correlation type");
  if (n_nodes > (int64_t)INT32_MAX) return fail(ctx, NR_ERR_UNSUPPORTED, "n_nodes exceeds 2^31-1");
  NR_HIP(ctx, hipSetDevice(ctx->device));
  NR_HIP(ctx, hipStreamSynchronize(ctx->stream));
  // Everything on the device lives for this call only: the scaled block in a
  // Dataset of its own (never the context's), the correlation-type scratch,
  // the partial sums with the result behind them, two events.
  struct Transient {
    Dataset ds;
    double *cor = nullptr, *sft = nullptr;
    hipEvent_t ev[2] = {nullptr, nullptr};
    ~Transient() {
      dfree(ds.d_data);
      dfree(cor);
      dfree(sft);
      for (hipEvent_t x : ev)
        if (x) (void)hipEventDestroy(x);
    }
  } t;
  auto oom = [&](const char* what, size_t bytes, const char* formula) {
    (void)hipGetLastError();
    return fail(ctx, NR_ERR_OOM,
                std::string("soft connectivity: allocation of the ") + std::to_string(bytes) + "-byte (" +
                    std::to_string(bytes >> 20) + " MiB) " + what + " failed (" + formula + ")");
  };
  try {
    const size_t block_bytes = (size_t)n_samples * (size_t)(n_nodes + 2) * sizeof(double);
    int rc = load_data_block(ctx, t.ds, n_nodes, n_samples, scale != 0,
                             [&](double* dst) { return put_data(ctx, data, n_samples * n_nodes, NR_HOST, dst); });
    if (rc == NR_ERR_OOM) return oom("data block", block_bytes, "8 S (n + 2) bytes, and 8 S n more while it is scaled");
    if (rc) return rc;
    if (cor_type) {
      const size_t cor_bytes = nr::cor_scratch_bytes(n_nodes, n_samples, cor_type);
      if (hipMalloc((void**)&t.cor, cor_bytes) != hipSuccess) {
        t.cor = nullptr;
        return oom("correlation-type scratch", cor_bytes,
                   cor_type == NR_COR_SPEARMAN ? "8 S (n + 2) + 8 S n bytes" : "8 S (n + 2) bytes");
      }
    }
    const int R = ctx->sft_row_groups ? ctx->sft_row_groups : nr::sft_row_groups(n_nodes);
    const size_t sft_bytes = nr::sft_scratch_bytes(n_nodes, n_powers, R);
    if (hipMalloc((void**)&t.sft, sft_bytes) != hipSuccess) {
      t.sft = nullptr;
      return oom("partial sums and result", sft_bytes, "8 R P n + 8 P n bytes");
    }
    for (hipEvent_t& x : t.ev) NR_HIP(ctx, hipEventCreate(&x));
    const double* const from = cor_type ? t.cor : t.ds.d_data;
    rc = read_flags(ctx, t.ds, "soft connectivity", [&](int* flag) {
      hipError_t p = hipSuccess;
      if (cor_type) p = nr::launch_cor_transform(t.ds.d_data, n_samples, n_nodes, cor_type, t.cor, ctx->stream);
      if (p == hipSuccess) p = hipEventRecord(t.ev[0], ctx->stream);
      if (p == hipSuccess)
        p = nr::launch_soft_connectivity(from, n_samples, n_nodes, base_type, powers, n_powers, R, t.sft, flag,
                                         ctx->stream);
      if (p == hipSuccess) p = hipEventRecord(t.ev[1], ctx->stream);
      if (p == hipSuccess)
        p = hipMemcpyAsync(k_out, t.sft + nr::sft_result_offset(n_nodes, n_powers, R),
                           (size_t)n_nodes * (size_t)n_powers * sizeof(double), hipMemcpyDeviceToHost, ctx->stream);
      return p;
    });
    if (rc) {
      (void)hipStreamSynchronize(ctx->stream);  // nothing queued still reads what is freed on return
      return rc;
    }
    float ms = 0.f;
    NR_HIP(ctx, hipEventElapsedTime(&ms, t.ev[0], t.ev[1]));
    ctx->sft_ms = (double)ms;
    ctx->sft_finite = t.ds.net_finite;
    return NR_OK;
  } catch (const std::bad_alloc&) {
    (void)hipStreamSynchronize(ctx->stream);
    return fail(ctx, NR_ERR_OOM, "host memory allocation failed");
  } catch (const std::exception& ex) {
    (void)hipStreamSynchronize(ctx->stream);
    return fail(ctx, NR_ERR_INVALID, std::string("internal error: ") + ex.what());
  }
}

int nr_sft_ms(nr_ctx* ctx, double* ms) {
  if (!ctx || !ms) return NR_ERR_INVALID;
  *ms = ctx->sft_ms;
  return NR_OK;
}

int nr_sft_finite(nr_ctx* ctx, int* finite) {
  if (!ctx || !finite) return NR_ERR_INVALID;
  *finite = ctx->sft_finite;
  return NR_OK;
}

int nr_set_sft_row_groups(nr_ctx* ctx, int row_groups) {
  if (!ctx) return NR_ERR_INVALID;
  if (row_groups < 0 || row_groups > nr::kSftRowGroupsLimit)
    return fail(ctx, NR_ERR_INVALID, "row groups must be 0 (the default) .. " + std::to_string(nr::kSftRowGroupsLimit));
  ctx->sft_row_groups = row_groups;
  return NR_OK;
}

int nr_hclust_average(nr_ctx* ctx, int32_t* id_lo, int32_t* id_hi, double* height, double* size) {
  if (!ctx) return NR_ERR_INVALID;
  if (!ctx->ds.d_pairs) return fail(ctx, NR_ERR_INVALID, "no dataset");
  // a cancellation requested before the call is honoured and consumed, as nr_run does
  if (ctx->cancel.exchange(false)) return fail(ctx, NR_ERR_CANCELLED, "hclust cancelled");
  const int64_t n = ctx->ds.n_nodes;
  if (n > 1 && (!id_lo || !id_hi || !height || !size))
    return fail(ctx, NR_ERR_INVALID, "id_lo, id_hi, height or size missing");
  if (n > nr::kHclustMaxNodes) return fail(ctx, NR_ERR_UNSUPPORTED, "hclust: n_nodes exceeds 2^30");
  ctx->hclust_ms = 0.0;
  ctx->hclust_searches = ctx->hclust_launches = ctx->hclust_scratch = 0;
  if (n < 2) return NR_OK;  // one node: no merge
  NR_HIP(ctx, hipSetDevice(ctx->device));
  // the table build replaces d_pairs between launches only; wait for both lanes
  NR_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (ctx->obs_stream) NR_HIP(ctx, hipStreamSynchronize(ctx->obs_stream));
  // Everything on the device lives for this call only and is freed on every path.
  struct Transient {
    double* D = nullptr;
    char* state = nullptr;
    hipEvent_t ev[2] = {nullptr, nullptr};
    hipStream_t stream = nullptr;
    ~Transient() {
      (void)hipStreamSynchronize(stream);  // nothing queued still uses what is freed
      dfree(D);
      dfree(state);
      for (hipEvent_t x : ev)
        if (x) (void)hipEventDestroy(x);
    }
  } t;
  t.stream = ctx->stream;
  const int64_t ld = nr::hclust_ld(n);
  const size_t d_bytes = (size_t)n * (size_t)ld * sizeof(double);
  const size_t state_bytes = nr::hclust_state_bytes(n);
  auto oom = [&](const char* what, size_t bytes, const char* formula) {
    (void)hipGetLastError();
    return fail(ctx, NR_ERR_OOM,
                std::string("hclust: allocation of the ") + std::to_string(bytes) + "-byte (" +
                    std::to_string(bytes >> 20) + " MiB) " + what + " failed (" + formula + ")");
  };
  if (hipMalloc((void**)&t.D, d_bytes) != hipSuccess) {
    t.D = nullptr;
    return oom("working matrix", d_bytes, "8 n ld bytes, ld = n rounded up to even");
  }
  if (hipMalloc((void**)&t.state, state_bytes) != hipSuccess) {
    t.state = nullptr;
    return oom("chain state", state_bytes, "64 + 40 n bytes");
  }
  ctx->hclust_scratch = (int64_t)(d_bytes + state_bytes);
  for (hipEvent_t& x : t.ev) NR_HIP(ctx, hipEventCreate(&x));
  nr::HclustParams P = nr::hclust_params(n, t.D, t.state);
  if (ctx->hclust_merges > 0) P.max_merges = ctx->hclust_merges;
  double total_ms = 0.0;
  auto timed = [&](hipError_t launched) -> hipError_t {  // between the two event records: one launch
    hipError_t e = launched;
    if (e == hipSuccess) e = hipEventRecord(t.ev[1], ctx->stream);
    if (e == hipSuccess) e = hipEventSynchronize(t.ev[1]);
    float ms = 0.f;
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, t.ev[0], t.ev[1]);
    total_ms += (double)ms;
    return e;
  };
  NR_HIP(ctx, hipEventRecord(t.ev[0], ctx->stream));
  NR_HIP(ctx, timed(nr::launch_hclust_extract(ctx->ds.d_pairs, ctx->ds.pairs_es, P, ctx->stream)));
  // The resident dataset is not read again. Launches of at most max_merges
  // merges each; every launch but a failing one completes its share, so the
  // count is known ahead and bounds this loop.
  const int64_t expected = nr::hclust_launches(n, P.max_merges);
  long long st[nr::kHclustStateWords] = {};
  for (int64_t launch = 0; launch < expected; ++launch) {
    if (ctx->cancel.load()) {
      ctx->cancel = false;
      return fail(ctx, NR_ERR_CANCELLED, "hclust cancelled");
    }
    NR_HIP(ctx, hipEventRecord(t.ev[0], ctx->stream));
    NR_HIP(ctx, timed(nr::launch_hclust_chain(P, ctx->stream)));
    NR_HIP(ctx, hipMemcpy(st, P.st, sizeof(st), hipMemcpyDeviceToHost));
    ++ctx->hclust_launches;
    ctx->hclust_searches = (int64_t)st[nr::kHclustStSearches];
    ctx->hclust_ms = total_ms;
    if (st[nr::kHclustStError] != 0) {
      const char* text = nr::hclust_error_text((int32_t)st[nr::kHclustStError]);
      return fail(ctx, NR_ERR_INTERNAL,
                  std::string("hclust: ") + (text ? text : "unknown error word") + " (after " +
                      std::to_string(st[nr::kHclustStMerged]) + " merges and " +
                      std::to_string(st[nr::kHclustStSearches]) + " searches)");
    }
    if (st[nr::kHclustStMerged] >= n - 1) break;
  }
  if (st[nr::kHclustStMerged] != n - 1)
    return fail(ctx, NR_ERR_INTERNAL, "hclust: the launches ended with " + std::to_string(st[nr::kHclustStMerged]) +
                                          " of " + std::to_string(n - 1) + " merges");
  ctx->cancel = false;  // a cancellation that arrives after the last launch has nothing left to stop
  const size_t m = (size_t)(n - 1);
  NR_HIP(ctx, hipMemcpy(id_lo, P.m_lo, m * sizeof(int32_t), hipMemcpyDeviceToHost));
  NR_HIP(ctx, hipMemcpy(id_hi, P.m_hi, m * sizeof(int32_t), hipMemcpyDeviceToHost));
  NR_HIP(ctx, hipMemcpy(height, P.m_height, m * sizeof(double), hipMemcpyDeviceToHost));
  NR_HIP(ctx, hipMemcpy(size, P.m_size, m * sizeof(double), hipMemcpyDeviceToHost));
  return NR_OK;
}

int nr_hclust_ms(nr_ctx* ctx, double* ms) {
  if (!ctx || !ms) return NR_ERR_INVALID;
  *ms = ctx->hclust_ms;
  return NR_OK;
}

int nr_hclust_info(nr_ctx* ctx, int64_t* searches, int64_t* launches, int64_t* scratch_bytes) {
  if (!ctx) return NR_ERR_INVALID;
  if (searches) *searches = ctx->hclust_searches;
  if (launches) *launches = ctx->hclust_launches;
  if (scratch_bytes) *scratch_bytes = ctx->hclust_scratch;
  return NR_OK;
}

int nr_set_hclust_merges_per_launch(nr_ctx* ctx, int64_t merges) {
  if (!ctx) return NR_ERR_INVALID;
  if (merges < 0) return fail(ctx, NR_ERR_INVALID, "merges per launch must be 0 (the default) or more");
  ctx->hclust_merges = merges;
  return NR_OK;
}

int nr_module_eigengenes(nr_ctx* ctx, int32_t n_mod, const int64_t* node_off, const int32_t* idx, double* eigengenes,
                         double* var_explained, double* contribution) {
  if (!ctx) return NR_ERR_INVALID;
  if (n_mod < 1 || !node_off || !idx || !eigengenes || !var_explained)
    return fail(ctx, NR_ERR_INVALID, "n_mod < 1, or node_off, idx, eigengenes or var_explained missing");
  if (!ctx->ds.d_pairs) return fail(ctx, NR_ERR_INVALID, "no dataset");
  if (!ctx->ds.d_data) return fail(ctx, NR_ERR_INVALID, "eigengenes need a dataset with data");
  std::lock_guard<std::mutex> lk(ctx->mu);
  NR_HIP(ctx, hipSetDevice(ctx->device));
  ctx->eig_n_mod = 0;  // valid again only once everything below has succeeded
  const int64_t S = ctx->ds.n_samples;
  ModuleSets ms;
  double *d_nc = nullptr, *d_coh = nullptr;
  int rc = upload_module_sets(ctx, n_mod, node_off, idx, ms);
  if (!rc) rc = ensure(ctx, ctx->d_eig, ctx->eig_cap, (size_t)n_mod * (size_t)S);
  if (!rc) {
    hipError_t e = hipMalloc((void**)&d_nc, (size_t)ms.nodes * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void**)&d_coh, (size_t)n_mod * sizeof(double));
    if (e != hipSuccess) rc = hip_fail(ctx, e, "hipMalloc module eigengenes");
  }
  if (!rc) rc = launch_module_profiles(ctx, ms, ctx->d_eig, d_nc, d_coh);
  if (!rc) {
    auto d2h = [&](double* h, const double* d, int64_t n) {
      return h ? hipMemcpyAsync(h, d, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream) : hipSuccess;
    };
    hipError_t e = d2h(eigengenes, ctx->d_eig, (int64_t)n_mod * S);
    if (e == hipSuccess) e = d2h(var_explained, d_coh, n_mod);
    if (e == hipSuccess) e = d2h(contribution, d_nc, ms.nodes);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) rc = hip_fail(ctx, e, "module eigengenes");
  }
  if (rc) (void)hipStreamSynchronize(ctx->stream);  // nothing queued still uses what is freed
  dfree(d_nc);
  dfree(d_coh);
  if (rc) return rc;
  ctx->eig_n_mod = n_mod;
  ctx->eig_gen = ctx->data_gen;
  return NR_OK;
}

int nr_module_membership(nr_ctx* ctx, int32_t n_mod, const double* eigengenes, double* kme) {
  if (!ctx) return NR_ERR_INVALID;
  if (n_mod < 1 || !kme) return fail(ctx, NR_ERR_INVALID, "n_mod < 1 or kme missing");
  if (!ctx->ds.d_pairs) return fail(ctx, NR_ERR_INVALID, "no dataset");
  if (!ctx->ds.d_data) return fail(ctx, NR_ERR_INVALID, "module membership needs a dataset with data");
  const int64_t S = ctx->ds.n_samples, n = ctx->ds.n_nodes;
  if (S < 3) return fail(ctx, NR_ERR_INVALID, "module membership needs at least 3 samples");
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (!eigengenes && (!ctx->d_eig || ctx->eig_n_mod != n_mod || ctx->eig_gen != ctx->data_gen))
    return fail(ctx, NR_ERR_INVALID, "no eigengenes of n_mod modules from nr_module_eigengenes on this dataset");
  NR_HIP(ctx, hipSetDevice(ctx->device));
  ctx->membership_ms = 0.0;
  // Everything on the device lives for this call only and is freed on every path.
  struct Transient {
    double *up = nullptr, *ehat = nullptr, *kme = nullptr;
    hipEvent_t ev[2] = {nullptr, nullptr};
    hipStream_t stream = nullptr;
    ~Transient() {
      (void)hipStreamSynchronize(stream);
      dfree(up);
      dfree(ehat);
      dfree(kme);
      for (hipEvent_t x : ev)
        if (x) (void)hipEventDestroy(x);
    }
  } t;
  t.stream = ctx->stream;
  const size_t e_bytes = (size_t)S * (size_t)n_mod * sizeof(double);
  NR_HIP(ctx, hipMalloc((void**)&t.ehat, e_bytes));
  NR_HIP(ctx, hipMalloc((void**)&t.kme, (size_t)n * (size_t)n_mod * sizeof(double)));
  for (hipEvent_t& x : t.ev) NR_HIP(ctx, hipEventCreate(&x));
  const double* src = ctx->d_eig;
  if (eigengenes) {
    NR_HIP(ctx, hipMalloc((void**)&t.up, e_bytes));
    NR_HIP(ctx, h2d_async(t.up, eigengenes, e_bytes, ctx->stream));
    src = t.up;
  }
  NR_HIP(ctx, hipEventRecord(t.ev[0], ctx->stream));
  NR_HIP(ctx, nr::launch_eigengene_unit(src, S, n_mod, t.ehat, ctx->stream));
  NR_HIP(ctx, nr::launch_membership(ctx->ds.d_data, S, n, t.ehat, n_mod, t.kme, ctx->stream));
  NR_HIP(ctx, hipEventRecord(t.ev[1], ctx->stream));
  NR_HIP(ctx, hipMemcpyAsync(kme, t.kme, (size_t)n * (size_t)n_mod * sizeof(double), hipMemcpyDeviceToHost,
                             ctx->stream));
  NR_HIP(ctx, hipStreamSynchronize(ctx->stream));
  float ms = 0.f;
  NR_HIP(ctx, hipEventElapsedTime(&ms, t.ev[0], t.ev[1]));
  ctx->membership_ms = (double)ms;
  return NR_OK;
}

int nr_membership_ms(nr_ctx* ctx, double* ms) {
  if (!ctx || !ms) return NR_ERR_INVALID;
  *ms = ctx->membership_ms;
  return NR_OK;
}

int nr_module_connectivity(nr_ctx* ctx, int32_t n_mod, const int32_t* slot, double* k_total, double* k_mod) {
  if (!ctx) return NR_ERR_INVALID;
  if (n_mod < 1 || !slot || !k_mod) return fail(ctx, NR_ERR_INVALID, "n_mod < 1, or slot or k_mod missing");
  if (!ctx->ds.d_pairs) return fail(ctx, NR_ERR_INVALID, "no dataset");
  const int64_t n = ctx->ds.n_nodes;
  for (int64_t j = 0; j < n; ++j)
    if (slot[j] < -1 || slot[j] >= n_mod)
      return fail(ctx, NR_ERR_INVALID, "slot[" + std::to_string(j) + "] = " + std::to_string(slot[j]) +
                                           " is outside -1 .. n_mod - 1");
  std::lock_guard<std::mutex> lk(ctx->mu);
  NR_HIP(ctx, hipSetDevice(ctx->device));
  // the table build replaces d_pairs between launches only; wait for both lanes
  NR_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (ctx->obs_stream) NR_HIP(ctx, hipStreamSynchronize(ctx->obs_stream));
  ctx->connectivity_ms = 0.0;
  // Everything on the device lives for this call only and is freed on every path.
  struct Transient {
    char* buf = nullptr;
    hipEvent_t ev[2] = {nullptr, nullptr};
    hipStream_t stream = nullptr;
    ~Transient() {
      (void)hipStreamSynchronize(stream);  // nothing queued still uses what is freed
      dfree(buf);
      for (hipEvent_t x : ev)
        if (x) (void)hipEventDestroy(x);
    }
  } t;
  t.stream = ctx->stream;
  // k_mod [n x n_mod] | k_total [n] | slot [n]
  const size_t cells = (size_t)n * ((size_t)n_mod + 1);
  const size_t bytes = cells * sizeof(double) + (size_t)n * sizeof(int32_t);
  if (hipMalloc((void**)&t.buf, bytes) != hipSuccess) {
    t.buf = nullptr;
    (void)hipGetLastError();
    return fail(ctx, NR_ERR_OOM, "module connectivity: allocation of the " + std::to_string(bytes) + "-byte (" +
                                     std::to_string(bytes >> 20) + " MiB) scratch failed (4 n + 8 n (n_mod + 1) bytes)");
  }
  double* const d_mod = reinterpret_cast<double*>(t.buf);
  double* const d_tot = d_mod + (size_t)n * (size_t)n_mod;
  int32_t* const d_slot = reinterpret_cast<int32_t*>(d_mod + cells);
  for (hipEvent_t& x : t.ev) NR_HIP(ctx, hipEventCreate(&x));
  NR_HIP(ctx, h2d_async(d_slot, slot, (size_t)n * sizeof(int32_t), ctx->stream));
  NR_HIP(ctx, hipEventRecord(t.ev[0], ctx->stream));
  NR_HIP(ctx, nr::launch_connectivity(ctx->ds.d_pairs, ctx->ds.pairs_es, n, d_slot, n_mod, ctx->connectivity_tile,
                                      d_tot, d_mod, ctx->stream));
  NR_HIP(ctx, hipEventRecord(t.ev[1], ctx->stream));
  NR_HIP(ctx, hipMemcpyAsync(k_mod, d_mod, (size_t)n * (size_t)n_mod * sizeof(double), hipMemcpyDeviceToHost,
                             ctx->stream));
  if (k_total)
    NR_HIP(ctx, hipMemcpyAsync(k_total, d_tot, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  NR_HIP(ctx, hipStreamSynchronize(ctx->stream));
  float ms = 0.f;
  NR_HIP(ctx, hipEventElapsedTime(&ms, t.ev[0], t.ev[1]));
  ctx->connectivity_ms = (double)ms;
  return NR_OK;
}

int nr_connectivity_ms(nr_ctx* ctx, double* ms) {
  if (!ctx || !ms) return NR_ERR_INVALID;
  *ms = ctx->connectivity_ms;
  return NR_OK;
}

int nr_set_connectivity_module_tile(nr_ctx* ctx, int32_t tile) {
  if (!ctx) return NR_ERR_INVALID;
  if (tile < 0 || tile > nr::kConnectivityTileMax)
    return fail(ctx, NR_ERR_INVALID,
                "module tile must be 0 (the default) .. " + std::to_string(nr::kConnectivityTileMax));
  ctx->connectivity_tile = tile;
  return NR_OK;
}

int nr_set_dataset_files(nr_ctx* ctx, const char* corr_path, const char* net_path, const char* data_path,
                         const char* corr_object, const char* net_object, const char* data_object,
                         int scale_data) {
  if (!ctx) return NR_ERR_INVALID;
  if (!corr_path || !net_path) return fail(ctx, NR_ERR_INVALID, "corr/net file missing");
  return replace_dataset(ctx, [&](Dataset& ds) {
    return set_dataset_files_impl(ctx, ds, corr_path, net_path, data_path, corr_object, net_object, data_object,
                                  scale_data);
  });
}

int nr_clear_dataset(nr_ctx* ctx) {
  if (!ctx) return NR_ERR_INVALID;
  NR_HIP(ctx, hipSetDevice(ctx->device));
  NR_HIP(ctx, hipStreamSynchronize(ctx->stream));
  reset_dataset(ctx);
  ctx->cancel = false;  // a context cancelled after its run returned starts clean
  return NR_OK;
}

int nr_copy_dataset(nr_ctx* dst, const nr_ctx* src) {
  if (!dst || !src || dst == src) return NR_ERR_INVALID;
  if (!src->ds.d_pairs) return fail(dst, NR_ERR_INVALID, "source context has no dataset");
  NR_HIP(dst, hipSetDevice(dst->device));
  NR_HIP(dst, hipStreamSynchronize(dst->stream));
  reset_dataset(dst);  // on a failure below dst is left with no dataset
  const Buffers from = buffers_of(src->ds);
  const BufferBytes bytes = buffer_bytes_of(src->ds);
  hipError_t e = alloc_buffers(dst->ds, bytes);
  const Buffers to = buffers_of(dst->ds);
  // Device to device: over xGMI between GPUs, an on-device copy when both
  // contexts share a GPU. The source must be idle (its upload synchronised).
  for (int i = 0; i < 3; ++i)
    if (e == hipSuccess && bytes[i])
      e = hipMemcpyPeerAsync(to[i], dst->device, from[i], src->device, bytes[i], dst->stream);
  const hipError_t e2 = hipStreamSynchronize(dst->stream);
  if (e == hipSuccess) e = e2;
  if (e != hipSuccess) {
    reset_dataset(dst);
    return hip_fail(dst, e, "dataset copy");
  }
  copy_dataset_fields(dst->ds, src->ds);
  return NR_OK;
}

}  // extern "C"

// One resident dataset to n - 1 other contexts ("broadcast once
// per test dataset"), bandwidth-optimal on a full xGMI mesh: a scatter and an
// all-gather of peer copies. Each buffer is cut into n - 1 pieces. Phase 1:
// piece p goes from the source to context p + 1 (every source link busy at
// once, B / (n-1) bytes each). Phase 2: context p + 1 forwards piece p to the
// other n - 2 destinations over its own direct links, each copy behind the
// event that marks the piece's arrival. Every link carries at most
// B / (n-1) per phase: 2B / ((n-1) L) in all, against B / L for a direct
// fan-out (each destination pulls all B over its one link to the source) or
// a single pipelined ring (DESIGN.md section 7 has the arithmetic). The source
// must be idle; on failure every destination is left with no dataset.
// Peer access between every pair of distinct GPUs a broadcast uses, in both
// directions (the scatter reads GPU 0 from each destination's stream, the
// all-gather reads every destination from every other): direct copies over
// the xGMI links instead of copies staged through host memory
// (src/permutations.cpp:335-380 is the reference's one-process parallel
// section this replaces). Enabled once per ordered pair per process. A pair
// without peer access still works -- hipMemcpyPeerAsync stages it through
// host memory -- at PCIe speed; such pairs are recorded
// (nr_peer_staged_pairs) instead of failing the broadcast.
namespace {

std::mutex g_peer_mu;
std::set<std::pair<int, int>> g_peer_on, g_peer_staged;

int enable_peer_access(nr_ctx* err_ctx, const std::vector<int>& devs) {
  std::lock_guard<std::mutex> lk(g_peer_mu);
  for (int a : devs)
    for (int b : devs) {
      if (a == b || g_peer_on.count({a, b}) || g_peer_staged.count({a, b})) continue;
      int can = 0;
      NR_HIP(err_ctx, hipDeviceCanAccessPeer(&can, a, b));
      if (!can) {
        g_peer_staged.insert({a, b});
        continue;
      }
      NR_HIP(err_ctx, hipSetDevice(a));
      const hipError_t e = hipDeviceEnablePeerAccess(b, 0);
      if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) return hip_fail(err_ctx, e, "hipDeviceEnablePeerAccess");
      (void)hipGetLastError();  // clears hipErrorPeerAccessAlreadyEnabled
      g_peer_on.insert({a, b});
    }
  return NR_OK;
}

// The calling thread's current device, restored on every return path.
struct DeviceRestore {
  int dev = -1;
  DeviceRestore() {
    if (hipGetDevice(&dev) != hipSuccess) dev = -1;
  }
  ~DeviceRestore() {
    if (dev >= 0) (void)hipSetDevice(dev);
  }
};

}  // namespace

extern "C" {

int nr_peer_staged_pairs(int* n) {
  if (!n) return NR_ERR_INVALID;
  std::lock_guard<std::mutex> lk(g_peer_mu);
  *n = (int)g_peer_staged.size();
  return NR_OK;
}

int nr_broadcast_dataset(nr_ctx* const* ctxs, int n) {
  if (!ctxs || n < 1) return NR_ERR_INVALID;
  DeviceRestore restore;
  nr_ctx* src = ctxs[0];
  if (!src) return NR_ERR_INVALID;
  for (int g = 1; g < n; ++g)
    for (int h = 0; h < g; ++h)
      if (!ctxs[g] || ctxs[g] == ctxs[h]) return fail(src, NR_ERR_INVALID, "broadcast: contexts must be distinct");
  if (!src->ds.d_pairs) return fail(src, NR_ERR_INVALID, "source context has no dataset");
  if (n == 1) return NR_OK;
  {
    std::vector<int> devs;
    for (int g = 0; g < n; ++g)
      if (std::find(devs.begin(), devs.end(), ctxs[g]->device) == devs.end()) devs.push_back(ctxs[g]->device);
    if (int rc = enable_peer_access(src, devs)) return rc;
  }
  const int parts = n - 1;
  const BufferBytes bytes = buffer_bytes_of(src->ds);
  std::vector<Buffers> at(n);  // at[g]: context g's buffers
  at[0] = buffers_of(src->ds);
  auto clear_all = [&]() {
    for (int g = 1; g < n; ++g) {
      (void)hipSetDevice(ctxs[g]->device);
      (void)hipStreamSynchronize(ctxs[g]->stream);
      reset_dataset(ctxs[g]);
    }
  };
  for (int g = 1; g < n; ++g) {
    nr_ctx* d = ctxs[g];
    NR_HIP(d, hipSetDevice(d->device));
    NR_HIP(d, hipStreamSynchronize(d->stream));
    reset_dataset(d);
    const hipError_t e = alloc_buffers(d->ds, bytes);
    if (e != hipSuccess) {
      const int rc = hip_fail(d, e, "broadcast allocation");
      clear_all();
      return fail(src, rc, d->err);
    }
    at[g] = buffers_of(d->ds);
  }
  auto piece = [&](size_t total, int p, size_t* a, size_t* len) {
    const size_t per = ((total + parts - 1) / parts + 255) / 256 * 256;
    *a = std::min(total, (size_t)p * per);
    *len = std::min(total, *a + per) - *a;
  };
  // piece p of every buffer from context `from` to context `to`, on to's stream
  auto send_piece = [&](int p, int from, int to) {
    hipError_t e = hipSuccess;
    for (int i = 0; i < 3 && e == hipSuccess; ++i) {
      size_t a, len;
      piece(bytes[i], p, &a, &len);
      if (len)
        e = hipMemcpyPeerAsync(at[to][i] + a, ctxs[to]->device, at[from][i] + a, ctxs[from]->device, len,
                               ctxs[to]->stream);
    }
    return e;
  };
  NR_HIP(src, hipSetDevice(src->device));
  NR_HIP(src, hipStreamSynchronize(src->stream));
  std::vector<hipEvent_t> ev(parts, nullptr);
  hipError_t e = hipSuccess;
  // phase 1: the scatter
  for (int p = 0; p < parts && e == hipSuccess; ++p) {
    e = hipSetDevice(ctxs[p + 1]->device);
    if (e == hipSuccess) e = send_piece(p, 0, p + 1);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&ev[p], hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventRecord(ev[p], ctxs[p + 1]->stream);
  }
  // phase 2: the all-gather among the destinations
  for (int g = 1; g < n && e == hipSuccess; ++g) {
    e = hipSetDevice(ctxs[g]->device);
    for (int p = 0; p < parts && e == hipSuccess; ++p) {
      if (p == g - 1) continue;
      e = hipStreamWaitEvent(ctxs[g]->stream, ev[p], 0);
      if (e == hipSuccess) e = send_piece(p, p + 1, g);
    }
  }
  for (int g = 1; g < n; ++g) {
    const hipError_t e2 = hipSetDevice(ctxs[g]->device);
    const hipError_t e3 = hipStreamSynchronize(ctxs[g]->stream);
    if (e == hipSuccess) e = e2 != hipSuccess ? e2 : e3;
  }
  for (hipEvent_t x : ev)
    if (x) (void)hipEventDestroy(x);
  if (e != hipSuccess) {
    const int rc = hip_fail(src, e, "dataset broadcast");
    clear_all();
    return rc;
  }
  for (int g = 1; g < n; ++g) copy_dataset_fields(ctxs[g]->ds, src->ds);
  return NR_OK;
}

// ---- queries and export ---------------------------------------------------

int nr_dataset_shape(const nr_ctx* ctx, int64_t* n_nodes, int64_t* n_samples) {
  if (!ctx) return NR_ERR_INVALID;
  if (n_nodes) *n_nodes = ctx->ds.n_nodes;
  if (n_samples) *n_samples = ctx->ds.n_samples;
  return NR_OK;
}

int nr_dataset_colnames(const nr_ctx* ctx, char* buf, int64_t cap, int64_t* needed) {
  if (!ctx || !needed) return NR_ERR_INVALID;
  int64_t total = 0;
  for (const std::string& s : ctx->ds.node_names) total += (int64_t)s.size() + 1;
  *needed = total;
  if (!buf || cap < total) return NR_OK;
  for (const std::string& s : ctx->ds.node_names) {
    std::memcpy(buf, s.c_str(), s.size() + 1);
    buf += s.size() + 1;
  }
  return NR_OK;
}

int nr_dataset_symmetric(nr_ctx* ctx, int* symmetric) {
  if (!ctx || !symmetric) return NR_ERR_INVALID;
  if (!ctx->ds.d_pairs) return fail(ctx, NR_ERR_INVALID, "no dataset");
  *symmetric = ctx->ds.symmetric;
  return NR_OK;
}

int nr_dataset_finite(nr_ctx* ctx, int* corr_finite, int* net_finite) {
  if (!ctx || !corr_finite || !net_finite) return NR_ERR_INVALID;
  if (!ctx->ds.d_pairs) return fail(ctx, NR_ERR_INVALID, "no dataset");
  *corr_finite = ctx->ds.corr_finite;
  *net_finite = ctx->ds.net_finite;
  return NR_OK;
}

int nr_gram_table(nr_ctx* ctx, int* on) {
  if (!ctx || !on) return NR_ERR_INVALID;
  *on = ctx->ds.d_pairs && ctx->ds.pairs_es == 2 ? 1 : 0;
  return NR_OK;
}

int nr_gram_table_ms(nr_ctx* ctx, double* ms) {
  if (!ctx || !ms) return NR_ERR_INVALID;
  *ms = ctx->ds.d_pairs && ctx->ds.pairs_es == 2 ? ctx->ds.table_ms : 0.0;
  return NR_OK;
}

int nr_netbuild_ms(nr_ctx* ctx, double* ms) {
  if (!ctx || !ms) return NR_ERR_INVALID;
  *ms = ctx->ds.d_pairs ? ctx->ds.netbuild_ms : 0.0;
  return NR_OK;
}

int nr_tom_ms(nr_ctx* ctx, double* ms) {
  if (!ctx || !ms) return NR_ERR_INVALID;
  *ms = ctx->ds.d_pairs ? ctx->ds.tom_ms : 0.0;
  return NR_OK;
}

int nr_cor_ms(nr_ctx* ctx, double* ms) {
  if (!ctx || !ms) return NR_ERR_INVALID;
  *ms = ctx->ds.d_pairs ? ctx->ds.cor_ms : 0.0;
  return NR_OK;
}

int nr_get_dataset_matrices(nr_ctx* ctx, double* corr_out, double* net_out) {
  if (!ctx) return NR_ERR_INVALID;
  if (!ctx->ds.d_pairs) return fail(ctx, NR_ERR_INVALID, "no dataset");
  if (!corr_out && !net_out) return NR_OK;
  NR_HIP(ctx, hipSetDevice(ctx->device));
  // the table build replaces d_pairs between launches only; wait for both lanes
  NR_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (ctx->obs_stream) NR_HIP(ctx, hipStreamSynchronize(ctx->obs_stream));
  const int64_t n_elem = ctx->ds.n_nodes * ctx->ds.n_nodes;
  const int64_t chunk = std::min<int64_t>(n_elem, (int64_t)1 << 22);  // 32 MiB per matrix per chunk
  const int parts = (corr_out ? 1 : 0) + (net_out ? 1 : 0);
  double* d = nullptr;
  NR_HIP(ctx, hipMalloc((void**)&d, (size_t)(parts * chunk) * sizeof(double)));
  double* dc = corr_out ? d : nullptr;
  double* dn = net_out ? d + (corr_out ? chunk : 0) : nullptr;
  hipError_t e = hipSuccess;
  for (int64_t o = 0; o < n_elem && e == hipSuccess; o += chunk) {
    const int64_t len = std::min(chunk, n_elem - o);
    e = nr::launch_deinterleave(ctx->ds.d_pairs, ctx->ds.pairs_es, o, len, dc, dn, ctx->stream);
    if (e == hipSuccess && dc)
      e = hipMemcpyAsync(corr_out + o, dc, (size_t)len * sizeof(double), hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess && dn)
      e = hipMemcpyAsync(net_out + o, dn, (size_t)len * sizeof(double), hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);  // the staging buffer is free again
  }
  (void)hipFree(d);
  if (e != hipSuccess) return hip_fail(ctx, e, "matrix export");
  return NR_OK;
}

}  // extern "C"
