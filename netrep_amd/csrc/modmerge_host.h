// Host rules that follow the eigengenes (include/netrep_gpu.h has them in
// full): the eigengene tree and its cut, the merging and relabelling of
// labels, the kME trimming and the intramodular connectivity -- pure host
// functions, no context, no HIP call, so they run, and are tested
// (tests/test_modmerge_host.py, tests/test_connectivity_host.py), without a
// GPU. Compiled with contraction off: every product and sum is rounded on its
// own, so a restatement in plain fp64 gives the same bits.
#pragma once
#include <stdint.h>

#include <vector>

namespace nr {

// The tree of the M columns of eig (S x M, column-major) on d = 1 - cor(E):
// each step merges the globally closest pair of clusters, ties to the lowest
// (lower, higher) pair, a cluster indexed by its lowest column. linkage:
// average (the Lance-Williams update, never fused) or complete (the larger of
// the two distances). Step t = 0 .. M - 2: slot_lo[t] < slot_hi[t], the lowest
// columns of the two clusters merged, and height[t]. false: a NaN in eig or a
// constant column (nothing defined).
enum { kLinkageAverage = 0, kLinkageComplete = 1 };
bool eigengene_tree(const double* eig, int64_t S, int64_t M, int linkage, int32_t* slot_lo, int32_t* slot_hi,
                    double* height);
// Those steps as nr_hclust_average emits its own: ids 0 .. M - 1 are columns,
// M + u the cluster of step u (in place allowed).
void tree_slots_to_ids(int64_t M, const int32_t* slot_lo, const int32_t* slot_hi, int32_t* id_lo, int32_t* id_hi);

// eigengene_tree with average linkage, cut at cut_height. group[m]: the index (0-based, in column
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

// Intramodular connectivity from the module-connectivity table (k_mod
// [n x M, column-major], slot [n], -1 unassigned): k_within = the node's own
// module's cell, k_out = k_total - k_within, k_diff = k_within - k_out; NaN
// all three for slot -1.
void intramodular_connectivity(int64_t n, const int32_t* slot, const double* k_total, const double* k_mod,
                               double* k_within, double* k_out, double* k_diff);

}  // namespace nr
