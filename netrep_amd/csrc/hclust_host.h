// Host side of the average-linkage dendrogram (include/netrep_gpu.h,
// nr_hclust_average): the termination guard's arithmetic, and the finishing
// and static-cut steps as pure host functions -- no context, no HIP call, so
// they run, and are tested (tests/test_hclust_host.py), without a GPU.
#pragma once
#include <stdint.h>

namespace nr {

// Error words of hclust_chain_kernel (0: none).
enum {
  kHclustErrSearchCap = 1,    // the call's nearest-neighbour searches exceeded hclust_search_cap(n)
  kHclustErrNoNeighbour = 2,  // a search found no finite neighbour while more than one slot was live
  kHclustErrChain = 3,        // the chain outgrew the live slots, or no live slot was left to start from
};

// Default merges per chain launch (nr_set_hclust_merges_per_launch, 0).
constexpr int64_t kHclustMergesPerLaunch = 512;
// Largest n: ids n + t are int32, and so are the kernel's row indices.
constexpr int64_t kHclustMaxNodes = (int64_t)1 << 30;

// Nearest-neighbour searches one call may make: 4 n + 16 (the rules need
// fewer than 3 n).
int64_t hclust_search_cap(int64_t n);
// Leading dimension of the working matrix: n rounded up to even, so every
// column starts on a 16-byte boundary.
int64_t hclust_ld(int64_t n);
// Launches a call of n nodes takes at M merges per launch.
int64_t hclust_launches(int64_t n, int64_t merges_per_launch);
// Text of an error word; NULL for 0 or an unknown word.
const char* hclust_error_text(int32_t word);

// Discovery order -> R's hclust components (the header has the rules).
// merge [(n - 1) x 2, column-major], height_out [n - 1], order [n], all
// written; false (nothing defined) if (id_lo, id_hi) is not a binary tree in
// construction order or a height is NaN.
bool hclust_finish(int64_t n, const int32_t* id_lo, const int32_t* id_hi, const double* height, int32_t* merge,
                   double* height_out, int32_t* order, int32_t* n_repairs);

// cutreeStatic; false if merge is not an R merge matrix in height order.
bool cutree_static(int64_t n, const int32_t* merge, const double* height, double cut_height, int64_t min_size,
                   int32_t* labels);

}  // namespace nr
