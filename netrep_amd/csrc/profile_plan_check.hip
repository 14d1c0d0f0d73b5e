// Stand-alone check of the summary-profile launch planner; no HIP call, runs
// without a GPU (tests/test_profile_plan.py).
//   profile_plan_check carve   carves a host buffer with carve_lds / carve_split
//                              for every kernel class's parameters and holds the
//                              result against the byte formulas and the planner
//   profile_plan_check plans   reads "k_max n_samples n_items [data_doubles]"
//                              lines, prints each plan (256 CUs) and holds its
//                              workgroup against the kernel's description
#include <cstdio>
#include <cstring>
#include <vector>

#include "device_common.h"
#include "kernels.h"

using namespace nr;

namespace {

// the names `plans` prints (tests/test_profile_plan.py maps the recorded classes to them)
const char* profile_class_name(ProfileClass c) {
  switch (c) {
    case ProfileClass::Wave: return "wave";
    case ProfileClass::Small: return "small";
    case ProfileClass::Packed: return "packed";
    case ProfileClass::FullPartialsInScratch: return "full_partials_in_scratch";
    case ProfileClass::FullVectorsInScratch: return "full_vectors_in_scratch";
  }
  return "?";
}

const char* profile_kernel_name(ProfileKernel k) {
  switch (k) {
    case ProfileKernel::FullGram: return "full_gram";
    case ProfileKernel::PackedFixed: return "packed_fixed";
    case ProfileKernel::PackedRuntime: return "packed_runtime";
    case ProfileKernel::PackedBig: return "packed_big";
    case ProfileKernel::Table: return "table";
    case ProfileKernel::Small: return "small";
    case ProfileKernel::Wave: return "wave";
  }
  return "?";
}

int g_failed = 0;

#define CHECK(cond, ...)                      \
  do {                                        \
    if (!(cond)) {                            \
      if (++g_failed <= 20) {                 \
        fprintf(stderr, "FAILED %s: ", #cond); \
        fprintf(stderr, __VA_ARGS__);         \
        fprintf(stderr, "\n");                \
      }                                       \
    }                                         \
  } while (0)

alignas(16) unsigned char g_lds[kLdsBudget];

// Walks the arrays of a carve-out in their documented order: each starts
// where the one before ends.
struct Walk {
  const unsigned char* at;
  const char* what;
  int kvec, mmax;
  void next(const void* p, size_t bytes, const char* name) {
    CHECK((const unsigned char*)p == at, "%s: %s at %td, expected %td (kvec %d, mmax %d)", what, name,
          (const unsigned char*)p - g_lds, at - g_lds, kvec, mmax);
    at = (const unsigned char*)p + bytes;
  }
};

// carve_lds<NW> as a kernel calls it; returns the carved bytes.
template <int NW>
size_t check_carve(const char* what, int kvec, int mmax, int64_t extra, bool twork_in_extra) {
  const size_t bytes = carve_lds_bytes(NW, kvec, mmax, extra, twork_in_extra);
  CHECK(bytes <= kLdsBudget, "%s: %zu bytes (kvec %d, mmax %d)", what, bytes, kvec, mmax);
  if (bytes > kLdsBudget) return bytes;
  double* ext = nullptr;
  const LzLds L = carve_lds<NW>(g_lds, kvec, mmax, extra, &ext, twork_in_extra);
  const size_t d = sizeof(double);
  Walk w{g_lds, what, kvec, mmax};
  w.next(L.red, 8 * NW * d, "red");
  w.next(L.q, kvec * d, "q");
  w.next(L.qprev, kvec * d, "qprev");
  w.next(L.w, kvec * d, "w");
  w.next(L.vv, kvec * d, "vv");
  w.next(L.gv, kvec * d, "gv");
  w.next(L.colm, kvec * d, "colm");
  w.next(ext, extra * d, "extra");
  w.next(L.alpha, mmax * d, "alpha");
  w.next(L.beta, mmax * d, "beta");
  w.next(L.h, mmax * d, "h");
  w.next(L.ty, mmax * d, "ty");
  if (twork_in_extra) {  // the one alias: twork inside the extra area, which must hold it
    CHECK(L.twork == ext, "%s: twork not at the extra area", what);
    CHECK(extra >= 5 * (int64_t)mmax, "%s: extra %lld < 5 mmax (kvec %d, mmax %d)", what, (long long)extra, kvec, mmax);
  } else {
    w.next(L.twork, 5 * mmax * d, "twork");
  }
  w.next(L.omg, 3 * (mmax + 1) * d, "omg");
  w.next(L.idx, kvec * sizeof(uint32_t), "idx");
  CHECK(w.at == g_lds + bytes, "%s: carved %td, carve_lds_bytes %zu (kvec %d, mmax %d)", what, w.at - g_lds, bytes,
        kvec, mmax);
  CHECK(L.mmax == mmax, "%s: mmax", what);
  return bytes;
}

constexpr int kFullWaves = profile_traits(ProfileKernel::FullGram).waves;  // and the packed 4-wave kernels'

size_t check_split(int kvec, int mmax, std::vector<double>& gbuf) {
  constexpr int NW = kFullWaves;
  const char* what = "all in scratch";
  const size_t bytes = carve_split_bytes(NW, mmax);
  CHECK(bytes <= kLdsBudget, "%s: %zu bytes (mmax %d)", what, bytes, mmax);
  if (bytes > kLdsBudget) return bytes;
  gbuf.resize((size_t)carve_split_doubles(kvec));
  const LzLds L = carve_split<NW>(g_lds, gbuf.data(), kvec, mmax);
  const size_t d = sizeof(double);
  Walk w{g_lds, what, kvec, mmax};
  w.next(L.red, 8 * NW * d, "red");
  w.next(L.alpha, mmax * d, "alpha");
  w.next(L.beta, mmax * d, "beta");
  w.next(L.h, mmax * d, "h");
  w.next(L.ty, mmax * d, "ty");
  w.next(L.twork, 5 * mmax * d, "twork");
  w.next(L.omg, 3 * (mmax + 1) * d, "omg");
  CHECK(w.at == g_lds + bytes, "%s: carved %td, carve_split_bytes %zu (mmax %d)", what, w.at - g_lds, bytes, mmax);
  // the slot's scratch: six vectors, then the index set
  const double* g = gbuf.data();
  const double* vec[6] = {L.q, L.qprev, L.w, L.vv, L.gv, L.colm};
  for (int i = 0; i < 6; ++i) CHECK(vec[i] == g + (size_t)i * kvec, "%s: vector %d (kvec %d)", what, i, kvec);
  CHECK((const void*)L.idx == (const void*)(g + 6 * (size_t)kvec), "%s: idx (kvec %d)", what, kvec);
  const size_t end = 6 * (size_t)kvec * d + (size_t)kvec * sizeof(uint32_t);
  CHECK(end <= gbuf.size() * d && end + d > gbuf.size() * d, "%s: scratch end %zu of %zu (kvec %d)", what, end,
        gbuf.size() * d, kvec);
  return bytes;
}

// The carve-out kernel K makes of a planned launch (profile_body and the wave
// kernel in kernels.hip), from the description the kernel is compiled from.
template <ProfileKernel K>
size_t carve_as(const ProfilePlan& q, std::vector<double>& gbuf) {
  constexpr ProfileTraits T = profile_traits(K);
  const char* what = profile_kernel_name(K);
  const int kvec = T.kb > 0 ? T.kb : q.kvec, m = T.kb > 0 ? T.mb : q.m;
  if (K == ProfileKernel::Wave) return check_carve<T.waves>(what, kvec, m, 3 * kvec, false);
  if (T.storage == GramStorage::Packed)
    return check_carve<T.waves>(what, kvec, m, packed_part_doubles(T.waves, kvec, m), true);
  return q.vec_global ? check_split(kvec, m, gbuf) : check_carve<T.waves>(what, kvec, m, 0, false);
}

size_t carve_planned(const ProfilePlan& q, std::vector<double>& gbuf) {
  switch (q.kernel) {
    case ProfileKernel::Wave: return carve_as<ProfileKernel::Wave>(q, gbuf);
    case ProfileKernel::Small: return carve_as<ProfileKernel::Small>(q, gbuf);
    case ProfileKernel::Table: return carve_as<ProfileKernel::Table>(q, gbuf);
    case ProfileKernel::PackedFixed: return carve_as<ProfileKernel::PackedFixed>(q, gbuf);
    case ProfileKernel::PackedRuntime: return carve_as<ProfileKernel::PackedRuntime>(q, gbuf);
    case ProfileKernel::PackedBig: return carve_as<ProfileKernel::PackedBig>(q, gbuf);
    case ProfileKernel::FullGram: return carve_as<ProfileKernel::FullGram>(q, gbuf);
  }
  return 0;
}

// A plan launches its kernel on the workgroup the kernel is compiled for, at
// no more workgroups per CU than the kernel's cap.
void check_shape(const ProfilePlan& q) {
  const ProfileTraits T = profile_traits(q.kernel);
  CHECK(q.block == 64 * T.waves, "%s: block %d, %d waves", profile_kernel_name(q.kernel), q.block, T.waves);
  CHECK(q.per_cu >= 1 && q.per_cu <= T.cu_cap, "%s: per_cu %d, cap %d", profile_kernel_name(q.kernel), q.per_cu,
        T.cu_cap);
}

void check_plan(int k_max, int n_samples) {
  ProfilePlan p;
  if (!plan_profile(1000000, k_max, n_samples, 0, 256, &p)) {
    CHECK(false, "no plan for k_max %d, n_samples %d", k_max, n_samples);
    return;
  }
  std::vector<double> gbuf;
  size_t carved = carve_planned(p, gbuf);
  CHECK(carved == p.lds, "%s: plan.lds %zu, carved %zu (k_max %d, n_samples %d)", profile_kernel_name(p.kernel), p.lds,
        carved, k_max, n_samples);
  CHECK(p.kernel != ProfileKernel::PackedFixed || k_max <= kPackedLayoutK, "compile-time layout for k_max %d", k_max);
  check_shape(p);
  if (profile_takes_table(p, k_max, n_samples)) {
    profile_use_table(&p);
    carved = carve_planned(p, gbuf);
    CHECK(carved == p.lds, "table: plan.lds %zu, carved %zu (k_max %d, n_samples %d)", p.lds, carved, k_max,
          n_samples);
    check_shape(p);
  }
}

int carve_mode() {
  // every vector length a class's layout takes, up to the largest that fits
  for (const int m : {113, 160, 320}) {
    int n = 0;
    for (int kvec = kPackedLayoutK + 1;
         carve_lds_bytes(kFullWaves, kvec, m, packed_part_doubles(kFullWaves, kvec, m), true) <= kLdsBudget; ++kvec, ++n)
      check_carve<kFullWaves>("packed, runtime layout", kvec, m, packed_part_doubles(kFullWaves, kvec, m), true);
    CHECK(n > 1000, "packed sweep too short: %d", n);
    n = 0;
    for (int kvec = 1; carve_lds_bytes(kFullWaves, kvec, m, 0, false) <= kLdsBudget; ++kvec, ++n)
      check_carve<kFullWaves>("full Gram, partials in scratch", kvec, m, 0, false);
    CHECK(n > 2000, "full-Gram sweep too short: %d", n);
    std::vector<double> gbuf;
    for (int kvec = 1; kvec <= 20000; kvec += kvec < 3000 ? 1 : 997) check_split(kvec, m, gbuf);
  }
  // every class through the planner: the boundaries of each class and kernel
  for (const int S : {30, 112, 113, 200, 400, 1000, 1728, 1729, 1744, 2544, 2545, 2600, 5000})
    for (const int k : {1, 111, 112, 113, 320, 321, 433, 434, 758, 759, 1733, 1734, 2554, 2555, 4200, 20000})
      check_plan(k, S);
  if (g_failed) fprintf(stderr, "%d checks failed\n", g_failed);
  return g_failed ? 1 : 0;
}

int plans_mode() {
  char line[256];
  while (fgets(line, sizeof line, stdin)) {
    long long k = 0, S = 0, items = 0, data = 0;
    if (sscanf(line, "%lld %lld %lld %lld", &k, &S, &items, &data) < 3) continue;
    ProfilePlan p;
    const bool ok = plan_profile(items, (int)k, (int)S, data, 256, &p);
    printf("k_max=%lld n_samples=%lld n_items=%lld data_doubles=%lld status=%d class=%s kernel=%s block=%d lds=%zu "
           "per_cu=%d slots=%d k_gram=%d ld=%d m=%d kvec=%d big=%d gram_doubles=%lld basis_doubles=%lld stride=%lld "
           "g32_off=%lld part_global=%d vec_global=%d takes_table=%d\n",
           k, S, items, data, ok ? 0 : 1, profile_class_name(p.cls), profile_kernel_name(p.kernel), p.block, p.lds,
           p.per_cu, p.slots, p.k_gram, p.ld, p.m, p.kvec, (int)p.big, (long long)p.gram_doubles,
           (long long)p.basis_doubles, (long long)p.stride, (long long)p.g32_off,
           (int)(ok && p.kernel == ProfileKernel::FullGram),  // (the full Gram's partials: always in scratch)
           (int)p.vec_global, (int)(ok && profile_takes_table(p, (int)k, S)));
    if (ok) check_shape(p);
  }
  ProfilePlan t;
  profile_use_table(&t);
  check_shape(t);
  printf("table_kernel=%s block=%d lds=%zu\n", profile_kernel_name(t.kernel), t.block, t.lds);
  if (g_failed) fprintf(stderr, "%d checks failed\n", g_failed);
  return g_failed ? 1 : 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "carve")) return carve_mode();
  if (argc == 2 && !strcmp(argv[1], "plans")) return plans_mode();
  fprintf(stderr, "usage: %s carve | plans < lines of \"k_max n_samples n_items [data_doubles]\"\n", argv[0]);
  return 2;
}
