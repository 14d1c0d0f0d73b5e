// Host rules that follow the eigengenes: see modmerge_host.h and the contract
// in include/netrep_gpu.h (netrep_EigengeneGroups, netrep_EigengeneTree,
// netrep_MergeLabels, netrep_TrimModulesKME, netrep_IntramodularConnectivity).
#include "modmerge_host.h"

#include <algorithm>
#include <cmath>
#include <limits>
#include <map>

namespace nr {

bool eigengene_tree(const double* eig, int64_t S, int64_t M, int linkage, int32_t* slot_lo, int32_t* slot_hi,
                    double* height) {
  if (M < 1 || S < 2) return false;
  // centred columns and their sums of squares, every sum in sample order
  std::vector<double> z((size_t)(S * M)), ss((size_t)M);
  for (int64_t m = 0; m < M; ++m) {
    double sum = 0.0;
    for (int64_t s = 0; s < S; ++s) sum += eig[m * S + s];
    const double mean = sum / (double)S;
    double q = 0.0;
    for (int64_t s = 0; s < S; ++s) {
      const double d = eig[m * S + s] - mean;
      z[(size_t)(m * S + s)] = d;
      q += d * d;
    }
    if (!(q > 0.0) || !std::isfinite(q)) return false;
    ss[(size_t)m] = q;
  }
  // d = 1 - cor, both triangles
  std::vector<double> d((size_t)(M * M), 0.0);
  for (int64_t a = 0; a < M; ++a)
    for (int64_t b = a + 1; b < M; ++b) {
      double dot = 0.0;
      for (int64_t s = 0; s < S; ++s) dot += z[(size_t)(a * S + s)] * z[(size_t)(b * S + s)];
      double c = dot / std::sqrt(ss[(size_t)a] * ss[(size_t)b]);
      c = std::min(1.0, std::max(-1.0, c));
      d[(size_t)(a * M + b)] = d[(size_t)(b * M + a)] = 1.0 - c;
    }
  // The merged cluster lives in the slot of the lower index, which is the
  // lowest column index among its members; the other slot is retired.
  std::vector<double> size((size_t)M, 1.0);
  std::vector<char> live((size_t)M, 1);
  for (int64_t step = 0; step + 1 < M; ++step) {
    int64_t bi = -1, bj = -1;
    double best = 0.0;
    for (int64_t i = 0; i < M; ++i) {
      if (!live[(size_t)i]) continue;
      for (int64_t j = i + 1; j < M; ++j) {
        if (!live[(size_t)j]) continue;
        const double v = d[(size_t)(i * M + j)];
        if (bi < 0 || v < best) {
          bi = i;
          bj = j;
          best = v;
        }
      }
    }
    height[step] = best;
    slot_lo[step] = (int32_t)bi;
    slot_hi[step] = (int32_t)bj;
    const double si = size[(size_t)bi], sj = size[(size_t)bj];
    for (int64_t k = 0; k < M; ++k) {
      if (!live[(size_t)k] || k == bi || k == bj) continue;
      const double di = d[(size_t)(k * M + bi)], dj = d[(size_t)(k * M + bj)];
      const double v = linkage == kLinkageComplete ? std::max(di, dj) : (si * di + sj * dj) / (si + sj);
      d[(size_t)(k * M + bi)] = d[(size_t)(bi * M + k)] = v;
    }
    size[(size_t)bi] = si + sj;
    live[(size_t)bj] = 0;
  }
  return true;
}

bool eigengene_groups(const double* eig, int64_t S, int64_t M, double cut_height, int32_t* group, double* height) {
  std::vector<int32_t> lo((size_t)std::max<int64_t>(M - 1, 0)), hi(lo.size());
  if (!eigengene_tree(eig, S, M, kLinkageAverage, lo.data(), hi.data(), height)) return false;
  for (int64_t m = 0; m < M; ++m) group[m] = (int32_t)m;
  for (int64_t step = 0; step + 1 < M; ++step)
    if (height[step] <= cut_height)
      for (int64_t m = 0; m < M; ++m)
        if (group[m] == hi[(size_t)step]) group[m] = lo[(size_t)step];
  return true;
}

void tree_slots_to_ids(int64_t M, const int32_t* slot_lo, const int32_t* slot_hi, int32_t* id_lo, int32_t* id_hi) {
  std::vector<int32_t> id((size_t)M);
  for (int64_t m = 0; m < M; ++m) id[(size_t)m] = (int32_t)m;
  for (int64_t t = 0; t + 1 < M; ++t) {
    const int32_t lo = slot_lo[t], hi = slot_hi[t];  // read first: the outputs may be the inputs
    id_lo[t] = id[(size_t)lo];
    id_hi[t] = id[(size_t)hi];
    id[(size_t)lo] = (int32_t)(M + t);
  }
}

void intramodular_connectivity(int64_t n, const int32_t* slot, const double* k_total, const double* k_mod,
                               double* k_within, double* k_out, double* k_diff) {
  const double na = std::numeric_limits<double>::quiet_NaN();
  for (int64_t i = 0; i < n; ++i) {
    if (slot[i] < 0) {
      k_within[i] = k_out[i] = k_diff[i] = na;
      continue;
    }
    const double w = k_mod[(int64_t)slot[i] * n + i];
    const double o = k_total[i] - w;
    k_within[i] = w;
    k_out[i] = o;
    k_diff[i] = w - o;
  }
}

bool module_labels_of(int64_t n, const int32_t* labels, std::vector<int32_t>& modules) {
  modules.clear();
  for (int64_t i = 0; i < n; ++i) {
    if (labels[i] < 0) return false;
    if (labels[i] > 0) modules.push_back(labels[i]);
  }
  std::sort(modules.begin(), modules.end());
  modules.erase(std::unique(modules.begin(), modules.end()), modules.end());
  return true;
}

void relabel_by_size(int64_t n, const int32_t* labels_in, int32_t* labels_out, std::vector<int32_t>* old_of_new) {
  std::map<int32_t, int64_t> count;
  for (int64_t i = 0; i < n; ++i)
    if (labels_in[i] > 0) ++count[labels_in[i]];
  std::vector<std::pair<int32_t, int64_t>> by(count.begin(), count.end());  // increasing old label
  std::stable_sort(by.begin(), by.end(), [](const auto& a, const auto& b) { return a.second > b.second; });
  std::map<int32_t, int32_t> new_of;
  if (old_of_new) old_of_new->clear();
  for (size_t r = 0; r < by.size(); ++r) {
    new_of[by[r].first] = (int32_t)r + 1;
    if (old_of_new) old_of_new->push_back(by[r].first);
  }
  for (int64_t i = 0; i < n; ++i) labels_out[i] = labels_in[i] > 0 ? new_of[labels_in[i]] : labels_in[i];
}

bool merge_labels(int64_t n, const int32_t* labels_in, int64_t M, const int32_t* module_labels, const int32_t* group,
                  bool relabel, int32_t* labels_out) {
  std::map<int32_t, int32_t> to;
  for (int64_t m = 0; m < M; ++m) {
    if (module_labels[m] <= 0 || group[m] < 0 || group[m] > m) return false;
    if (!to.emplace(module_labels[m], module_labels[group[m]]).second) return false;
  }
  for (int64_t i = 0; i < n; ++i) {
    if (labels_in[i] == 0) continue;
    if (!to.count(labels_in[i])) return false;
  }
  for (int64_t i = 0; i < n; ++i) labels_out[i] = labels_in[i] == 0 ? 0 : to[labels_in[i]];
  if (relabel) relabel_by_size(n, labels_out, labels_out, nullptr);
  return true;
}

void trim_modules_kme(int64_t n, const int32_t* labels_in, const double* kme_own, double min_kme_to_stay,
                      double min_core_kme, int64_t min_core_kme_size, int64_t min_size, int32_t* labels_out) {
  if (min_core_kme_size < 0) min_core_kme_size = (min_size + 2) / 3;
  std::map<int32_t, int64_t> core, kept;
  for (int64_t i = 0; i < n; ++i) {
    if (labels_in[i] <= 0) continue;
    if (kme_own[i] > min_core_kme) ++core[labels_in[i]];
    if (!(kme_own[i] < min_kme_to_stay)) ++kept[labels_in[i]];
  }
  for (int64_t i = 0; i < n; ++i) {
    const int32_t lab = labels_in[i];
    labels_out[i] = lab;
    if (lab <= 0) continue;
    if (core[lab] < min_core_kme_size || kme_own[i] < min_kme_to_stay || kept[lab] < min_size) labels_out[i] = 0;
  }
}

}  // namespace nr
