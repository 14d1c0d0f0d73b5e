// Host rules that follow the eigengenes (include/netrep_gpu.h has them in
// full): the eigengene tree and its cut, the merging and relabelling of
// labels, and the kME trimming -- pure host functions, no context, no HIP
// call, so they run, and are tested (tests/test_modmerge_host.py), without a
// GPU. Compiled with contraction off: every product and sum is rounded on its
// own, so a restatement in plain fp64 gives the same bits.
#pragma once
#include <stdint.h>

#include <vector>

namespace nr {

// Average linkage on d = 1 - cor(E) of the M columns of eig (S x M,
// column-major), cut at cut_height. group[m]: the index (0-based, in column
// order) of the first column of m's group; height [M - 1]: the merge heights
// in merge order. false: a NaN in eig or a constant column (nothing defined).
bool eigengene_groups(const double* eig, int64_t S, int64_t M, double cut_height, int32_t* group, double* height);

// The distinct positive labels in increasing order; false for a negative one.
bool module_labels_of(int64_t n, const int32_t* labels, std::vector<int32_t>& modules);

// One merge step: a node of module module_labels[m] gets
// module_labels[group[m]]; 0 stays 0. With relabel the result goes through
// relabel_by_size. false: a label that is neither 0 nor in module_labels, or
// a group index outside 0 .. m.
bool merge_labels(int64_t n, const int32_t* labels_in, int64_t M, const int32_t* module_labels, const int32_t* group,
                  bool relabel, int32_t* labels_out);

// The positive labels renumbered 1, 2, ... by decreasing size, ties to the
// lower old label (in place allowed). old_of_new, optional: the old label of
// each new one.
void relabel_by_size(int64_t n, const int32_t* labels_in, int32_t* labels_out, std::vector<int32_t>* old_of_new);

// blockwiseModules' kME trimming in one pass (kme_own: each node's
// correlation with its own module's eigengene). min_core_kme_size < 0: the
// default, min_size / 3 rounded up.
void trim_modules_kme(int64_t n, const int32_t* labels_in, const double* kme_own, double min_kme_to_stay,
                      double min_core_kme, int64_t min_core_kme_size, int64_t min_size, int32_t* labels_out);

}  // namespace nr
