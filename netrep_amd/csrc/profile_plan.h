// The launch plan of one summary-profile launch (one size class of modules):
// which kernel runs, on what workgroup shape and LDS, and how a slot's scratch
// is laid out. plan_profile is the only place that decides any of it; it is
// pure (no context, no HIP call), so profile_plan_check.hip runs it, and the
// LDS carve-outs it sizes, on a machine without a GPU
// (tests/test_profile_plan.py). DESIGN.md section 5.2 tabulates the classes.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace nr {

// The LDS a workgroup may ask for (gfx950: 160 KB per CU).
constexpr size_t kLdsBudget = 160 * 1024;

// What a launch keeps where. Modules with k > S use the S x S dual Gram, so
// the Gram side and every Lanczos dimension is min(k, S). One numerical path
// per class: no run-time switch selects another.
enum class ProfileClass {
  Wave,    // min(k, S) <= kWaveDim: one wave per item, the Gram in its registers ("variant 7")
  Small,   // min(k, S) <= kSmallDim: packed Gram, kSmallWaves-wave workgroups, several per CU ("variant 5")
  Packed,  // the packed symmetric Gram in the slot's scratch, 4-wave workgroups; LDS vectors as
           // long as fit (<= 1,733), longer (dual) modules' per-node arrays in scratch ("variant 2")
  FullPartialsInScratch,  // min(k, S) beyond the packed layout's vectors: the full ld x ld Gram, the
                          // matvec partials in scratch too; LDS vectors up to 2,554 ("variant 4")
  FullVectorsInScratch,   // min(k, S) beyond those as well: every Lanczos vector and the index set
                          // in scratch, no size limit but device memory ("variant 6")
};

enum class ProfileKernel {
  FullGram,       // module_profile_kernel
  PackedFixed,    // module_profile_packed4_kernel<kPackedLayoutK, 3>: compile-time LDS layout
  PackedRuntime,  // module_profile_packed4_kernel<0, 2>: runtime LDS layout
  PackedBig,      // module_profile_big_kernel: runtime layout, one workgroup per CU
  Table,          // module_profile_table_kernel: Gram and network statistics from the Gram table
  Small,          // module_profile_small_kernel<kSmallWaves>
  Wave,           // module_profile_wave_kernel
};

constexpr int kPackedLayoutK = 320;  // modules of the packed kernel's compile-time LDS layout
constexpr int kPackedLayoutM = kPackedLayoutK < 160 ? kPackedLayoutK : 160;  // its Lanczos basis columns
// The small class: several items per CU in flight instead of three 4-wave
// items; per-node arrays of modules longer than kSmallDim in the slot's scratch.
constexpr int kSmallDim = 112;
constexpr int kSmallWaves = 2;  // (one wave per item measured slower: profiles/r03/small_class/)
// The wave class (round 5): the item's whole Gram in one wave's registers (kernels.hip).
constexpr int kWaveBlocks = 7;                // 16-row blocks of the Gram's side (<= 112)
constexpr int kWaveVec = 16 * kWaveBlocks;     // LDS vector length and Lanczos basis columns
constexpr int kWaveDim = kWaveVec - 1;         // the side is the dimension plus the ones column
constexpr int kTableWaves = 4;  // (2 waves x 5 per CU measured 13% slower, profiles/r03/table_waves/)

enum class GramStorage { Full, Packed };  // ld x ld, or the packed lower triangle (kernels.hip, pk_at)
// Who fills an item's Gram. A kernel compiles one: with two, the compiler
// merges their MFMA blocks and spills around them.
enum class GramSource {
  MatrixCore,   // gram_mfma / gram_mfma_dual: 32 x 32 super-tiles
  SuperTile64,  // gram_mfma64 / gram_mfma128: 64-row super-tiles per wave, one workgroup per CU
  Table,        // the table's gathers, with the item's network statistics: no dual items, diagonal halved
};

// What a kernel is compiled as: the planner sizes its launches from this, and
// the kernel's body and __launch_bounds__ are instantiated from it.
struct ProfileTraits {
  int waves;       // per workgroup
  int launch_occ;  // second __launch_bounds__ argument: waves per SIMD the registers must allow
  int cu_cap;      // workgroups per CU the planner asks for at most
  int kb, mb;      // compile-time LDS layout: vector length, basis columns (0: the plan's kvec, m)
  GramStorage storage;
  GramSource source;  // (the wave kernel has its own body: the Gram in registers)
};
constexpr ProfileTraits profile_traits(ProfileKernel k) {
  constexpr auto PK = GramStorage::Packed;
  constexpr auto MC = GramSource::MatrixCore;
  switch (k) {
    case ProfileKernel::FullGram: return {4, 3, 1, 0, 0, GramStorage::Full, MC};
    case ProfileKernel::PackedFixed: return {4, 3, 3, kPackedLayoutK, kPackedLayoutM, PK, MC};
    case ProfileKernel::PackedRuntime: return {4, 2, 3, 0, 0, PK, MC};
    case ProfileKernel::PackedBig: return {4, 1, 1, 0, 0, PK, GramSource::SuperTile64};
    case ProfileKernel::Table: return {kTableWaves, 3, 3, kPackedLayoutK, kPackedLayoutM, PK, GramSource::Table};
    case ProfileKernel::Small: return {kSmallWaves, 3, 12 / kSmallWaves, kSmallDim, kSmallDim, PK, MC};  // 12 waves per CU
    case ProfileKernel::Wave: break;
  }
  return {1, 1, 4, kWaveVec, kWaveVec, PK, MC};
}

struct ProfilePlan {
  ProfileClass cls = ProfileClass::Packed;
  ProfileKernel kernel = ProfileKernel::PackedFixed;
  int block = 0;       // threads per workgroup
  size_t lds = 0;      // dynamic LDS bytes per workgroup
  int per_cu = 1;      // workgroups per CU
  int slots = 0;       // workgroups of the launch, one scratch slot each
  int k_gram = 0;      // side of the largest Gram (minus the ones column): min(k_max, S)
  int ld = 0;          // leading dimension of the full Gram
  int m = 0;           // Lanczos basis columns
  int kvec = 0;        // LDS vector length
  bool big = false;    // modules beyond kvec: their per-node arrays in the slot's scratch
  // a slot's scratch, in doubles: Gram, Lanczos basis, [matvec partials],
  // [per-node arrays of big modules], [Lanczos vectors + index set], [fp32 Gram copy]
  int64_t gram_doubles = 0, basis_doubles = 0, stride = 0;
  int64_t g32_off = 0;       // fp32 copy of the packed Gram (relaxed Lanczos steps), 0: none
  bool vec_global = false;   // the Lanczos vectors and index set behind the partials
};

// Plans a launch of n_items items of modules of at most k_max nodes over
// n_samples samples, the data block being data_doubles long, on dev_cus CUs.
// false: no layout fits the LDS budget.
bool plan_profile(int64_t n_items, int k_max, int n_samples, int64_t data_doubles, int dev_cus, ProfilePlan* plan);

// Whether a planned segment of modules of at most k_max nodes takes the Gram
// table where the dataset has one: the packed class on its compile-time
// layout with no dual item (the table kernel compiles no matrix-core or dual
// Gram), its LDS vectors holding the network item's per-node arrays. This
// rule fixes the numerical path of a dataset (engine.hip, table_wanted).
bool profile_takes_table(const ProfilePlan& plan, int k_max, int64_t n_samples);
// Moves such a segment's plan to the Gram-table kernel.
void profile_use_table(ProfilePlan* plan);

// Doubles of the packed (chunked column-group) Gram of side kc, rounded to 32.
int64_t packed_gram_doubles(int kc);

}  // namespace nr
