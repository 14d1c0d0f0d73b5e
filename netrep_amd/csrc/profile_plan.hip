// The summary-profile launch planner (profile_plan.h): host code only, sized
// by the carve-outs' own byte formulas (device_common.h).
#include "profile_plan.h"

#include <algorithm>

#include "device_common.h"
#include "kernels.h"

namespace nr {

namespace {

// The packed class's LDS is sized before its kernel is chosen (from the
// workgroups per CU that LDS allows): its kernels share one workgroup shape.
constexpr int kWaves = profile_traits(ProfileKernel::FullGram).waves;
static_assert(profile_traits(ProfileKernel::PackedFixed).waves == kWaves &&
              profile_traits(ProfileKernel::PackedRuntime).waves == kWaves &&
              profile_traits(ProfileKernel::PackedBig).waves == kWaves);

// Lanczos basis columns per item: 160 covers every C2/C3 module (<= 46 steps
// measured); large modules (C5: up to 2,000 nodes, spectra with small gaps)
// get 320.
int profile_m_max(int k_max) { return k_max <= kPackedLayoutK ? std::min(k_max, 160) : 320; }
// Leading dimension of the per-slot Gram: k module columns + the ones column,
// padded to a 32-column super-tile.
int gram_ld(int k_max) { return (k_max + 1 + 31) / 32 * 32; }

int64_t round32(int64_t v) { return (v + 31) / 32 * 32; }

// LDS of the packed kernels (the matvec partials double as twork): the
// compile-time layout up to kPackedLayoutK nodes, whatever the module, else
// vectors of kvec and a basis of m.
size_t packed_lds(int nw, int kvec, int m) {
  return carve_lds_bytes(nw, kvec, m, packed_part_doubles(nw, kvec, m), true);
}
size_t packed4_lds(int kvec, int m) {
  return kvec <= kPackedLayoutK ? packed_lds(kWaves, kPackedLayoutK, kPackedLayoutM) : packed_lds(kWaves, kvec, m);
}
// LDS of the full-Gram kernel with the matvec partials in scratch.
size_t full_lds(int kvec, int m) { return carve_lds_bytes(kWaves, kvec, m, 0, false); }
// Its longest LDS vectors (a multiple of 16) beside a basis of m.
int full_kvec_max(int m) {
  const size_t fixed = full_lds(0, m), per = full_lds(1, m) - fixed;
  return (int)((kLdsBudget - fixed) / per) / 16 * 16;
}

// Workgroups per CU: what the LDS holds, at most the kernel's cap.
int per_cu(size_t lds, ProfileKernel k) {
  return std::max(1, std::min((int)(kLdsBudget / lds), profile_traits(k).cu_cap));
}

// Whether the packed kernel's LDS (vectors of kvec, basis mmax) holds the
// network item's per-node arrays: NetLds (carve_net_over, from L.q; its
// reduction scratch is L.red) against the LzLds span from q up to idx.
bool fused_net_fits(int kvec, int mmax, int nw) {
  const size_t need = net_lds_bytes(nw, kvec) - sizeof(double) * 8 * nw;
  const size_t have = packed_lds(nw, kvec, mmax) - sizeof(double) * 8 * nw - sizeof(uint32_t) * kvec;
  return need <= have;
}

}  // namespace

int64_t packed_gram_doubles(int kc) { return round32(pk_base(pk_groups(kc), kc)); }

bool plan_profile(int64_t n_items, int k_max, int n_samples, int64_t data_doubles, int dev_cus, ProfilePlan* plan) {
  ProfilePlan p;
  // the dual (S x S) Gram of modules with k > S: the Gram side is min(k, S),
  // and so is every Lanczos dimension (basis columns of that length)
  p.k_gram = std::min(k_max, n_samples);
  p.ld = gram_ld(p.k_gram);
  // (the wave kernel's buffer loads take 32-bit byte offsets into the data block)
  if (p.k_gram <= kWaveDim && data_doubles * 8 < ((int64_t)1 << 31)) {
    // the Gram in registers: the slot's scratch holds the Lanczos basis only;
    // three extra LDS vectors (ylo, yup, the Gram diagonal); one wave per SIMD
    p.cls = ProfileClass::Wave;
    p.kernel = ProfileKernel::Wave;
    p.m = p.kvec = kWaveVec;
    p.lds = carve_lds_bytes(1, kWaveVec, kWaveVec, 3 * kWaveVec, false);
    p.per_cu = per_cu(p.lds, p.kernel);
  } else if (p.k_gram <= kSmallDim) {
    p.cls = ProfileClass::Small;
    p.kernel = ProfileKernel::Small;
    p.m = p.kvec = kSmallDim;
    p.lds = packed_lds(kSmallWaves, kSmallDim, kSmallDim);
    p.per_cu = per_cu(p.lds, p.kernel);
    p.gram_doubles = packed_gram_doubles(p.k_gram + 1);
  } else {
    p.m = profile_m_max(p.k_gram);
    p.kvec = k_max;
    p.cls = ProfileClass::Packed;
    if (packed4_lds(p.kvec, p.m) > kLdsBudget) {
      // Large modules on the packed Gram too (half the Lanczos bytes of the
      // full ld x ld Gram): LDS vectors as long as fit, and the per-node arrays
      // of modules longer than them in the slot's scratch, as long as every
      // Lanczos dimension min(k, S) fits the vectors.
      int kp = (k_max + 15) / 16 * 16;
      while (kp > 16 && packed4_lds(kp, p.m) > kLdsBudget) kp -= 16;
      // Else the full Gram, its per-wave matvec partials (4 x k doubles) in
      // the slot's scratch, which leaves LDS for the six Lanczos vectors only
      // (with them in LDS it never fits here: DESIGN.md section 5.2).
      if (p.k_gram <= kp)
        p.kvec = kp;
      else
        p.cls = ProfileClass::FullPartialsInScratch;
    }
    // Modules beyond even those vectors (any k up to N, as src/netStats.cpp:
    // 217-280): Lanczos runs on the dual Gram (dimension S <= kvec) and their
    // per-node arrays live in the slot's scratch; where the Lanczos dimension
    // min(k, S) itself exceeds the LDS vectors (S > kvec), every vector and
    // the index set move to the slot's scratch too.
    if (p.cls == ProfileClass::FullPartialsInScratch && full_lds(p.kvec, p.m) > kLdsBudget) {
      p.kvec = full_kvec_max(p.m);
      if (n_samples > p.kvec) {
        p.cls = ProfileClass::FullVectorsInScratch;
        p.kvec = k_max;
      }
    }
    if (p.cls == ProfileClass::Packed) {
      p.lds = packed4_lds(p.kvec, p.m);
      p.per_cu = per_cu(p.lds, ProfileKernel::PackedFixed);  // (the class's widest cap)
      // the compile-time layout at three workgroups per CU (measured fastest:
      // profiles/r02/profile_variants.txt), else the runtime layout
      p.kernel = k_max <= kPackedLayoutK && p.per_cu >= 3 ? ProfileKernel::PackedFixed
                 : p.per_cu == 1                          ? ProfileKernel::PackedBig
                                                          : ProfileKernel::PackedRuntime;
      p.gram_doubles = packed_gram_doubles(p.k_gram + 1);
    } else {
      p.vec_global = p.cls == ProfileClass::FullVectorsInScratch;
      p.kernel = ProfileKernel::FullGram;
      p.lds = p.vec_global ? carve_split_bytes(kWaves, p.m) : full_lds(p.kvec, p.m);
      p.per_cu = per_cu(p.lds, p.kernel);
      p.gram_doubles = (int64_t)p.ld * p.ld;
    }
  }
  if (p.lds > kLdsBudget) return false;
  p.block = 64 * profile_traits(p.kernel).waves;
  p.big = k_max > p.kvec;
  p.slots = (int)std::max<int64_t>(1, std::min<int64_t>(n_items, (int64_t)dev_cus * p.per_cu));
  p.basis_doubles = (int64_t)p.k_gram * p.m;
  const bool full = p.kernel == ProfileKernel::FullGram;  // its matvec partials (4 x kvec) behind the basis
  p.stride = p.gram_doubles + p.basis_doubles + (full ? (int64_t)kWaves * p.kvec : 0) +
             (p.big ? 5 * (int64_t)k_max : 0) +  // x.u, means, squares, contributions, index set
             (p.vec_global ? carve_split_doubles(p.kvec) : 0);
  if (!full) p.stride = round32(p.stride);
  if (!full && p.gram_doubles > 0) {
    // fp32 copy of the packed Gram at the slot's end (relaxed Lanczos steps)
    p.g32_off = p.stride;
    p.stride += round32(p.gram_doubles / 2);
  }
  *plan = p;
  return true;
}

bool profile_takes_table(const ProfilePlan& plan, int k_max, int64_t n_samples) {
  return plan.cls == ProfileClass::Packed && k_max <= kPackedLayoutK && k_max <= n_samples &&
         fused_net_fits(kPackedLayoutK, kPackedLayoutM, profile_traits(ProfileKernel::Table).waves);
}

void profile_use_table(ProfilePlan* plan) {
  plan->kernel = ProfileKernel::Table;
  constexpr ProfileTraits T = profile_traits(ProfileKernel::Table);
  plan->block = 64 * T.waves;
  plan->lds = packed_lds(T.waves, T.kb, T.mb);
}

}  // namespace nr
