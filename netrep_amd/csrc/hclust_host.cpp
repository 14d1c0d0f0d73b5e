// Host side of the average-linkage dendrogram (hclust_host.h). Heights are
// only compared and copied here, never computed; the file is still built
// without contraction, like sft_fit.cpp, so that nothing added later can
// change a bit of them.
#include "hclust_host.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <numeric>
#include <vector>

#include "../../include/netrep_gpu.h"

#pragma STDC FP_CONTRACT OFF
#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace nr {

int64_t hclust_search_cap(int64_t n) { return 4 * n + 16; }

int64_t hclust_ld(int64_t n) { return (n + 1) & ~(int64_t)1; }

int64_t hclust_launches(int64_t n, int64_t merges_per_launch) {
  const int64_t m = merges_per_launch > 0 ? merges_per_launch : kHclustMergesPerLaunch;
  return n < 2 ? 0 : (n - 1 + m - 1) / m;
}

const char* hclust_error_text(int32_t word) {
  switch (word) {
    case kHclustErrSearchCap:
      return "the nearest-neighbour chain exceeded its search cap of 4 n + 16";
    case kHclustErrNoNeighbour:
      return "a nearest-neighbour search found no finite dissimilarity while more than one cluster was live";
    case kHclustErrChain:
      return "the nearest-neighbour chain outgrew the live clusters";
    default:
      return nullptr;
  }
}

bool hclust_finish(int64_t n, const int32_t* id_lo, const int32_t* id_hi, const double* height, int32_t* merge,
                   double* height_out, int32_t* order, int32_t* n_repairs) {
  if (n < 1 || n > kHclustMaxNodes) return false;
  const int64_t m = n - 1;
  // a binary tree in construction order: every id below n + t, each a child once
  std::vector<char> used((size_t)(n + m), 0);
  for (int64_t t = 0; t < m; ++t) {
    if (std::isnan(height[t])) return false;
    const int64_t kids[2] = {id_lo[t], id_hi[t]};
    for (int64_t c : kids) {
      if (c < 0 || c >= n + t || used[(size_t)c]) return false;
      used[(size_t)c] = 1;
    }
  }
  // monotone repair, in discovery order
  std::vector<double> h(height, height + m);
  int32_t repairs = 0;
  for (int64_t t = 0; t < m; ++t) {
    double top = h[(size_t)t];
    if (id_lo[t] >= n) top = std::max(top, h[(size_t)(id_lo[t] - n)]);
    if (id_hi[t] >= n) top = std::max(top, h[(size_t)(id_hi[t] - n)]);
    if (top > h[(size_t)t]) {
      h[(size_t)t] = top;
      ++repairs;
    }
  }
  // stable sort by height: ties keep discovery order, so children precede parents
  std::vector<int64_t> perm((size_t)m), rank((size_t)m);
  std::iota(perm.begin(), perm.end(), (int64_t)0);
  std::stable_sort(perm.begin(), perm.end(), [&](int64_t a, int64_t b) { return h[(size_t)a] < h[(size_t)b]; });
  for (int64_t s = 0; s < m; ++s) rank[(size_t)perm[(size_t)s]] = s;
  auto label = [&](int64_t c) -> int32_t { return c < n ? (int32_t)(-(c + 1)) : (int32_t)(rank[(size_t)(c - n)] + 1); };
  for (int64_t s = 0; s < m; ++s) {
    const int64_t t = perm[(size_t)s];
    const int32_t x = label(id_lo[t]), y = label(id_hi[t]);
    const bool both_single = x < 0 && y < 0;
    // two singletons by node index (-1 before -5); else the smaller first: a
    // singleton before a cluster, two clusters by step
    merge[s] = both_single ? std::max(x, y) : std::min(x, y);
    merge[s + m] = both_single ? std::min(x, y) : std::max(x, y);
    height_out[s] = h[(size_t)t];
  }
  // order: the last merge expanded, first column's leaves before the second's
  std::vector<int32_t> todo;
  todo.push_back(m ? (int32_t)m : -1);
  int64_t at = 0;
  while (!todo.empty()) {
    const int32_t c = todo.back();
    todo.pop_back();
    if (c < 0) {
      order[at++] = -c;
    } else {
      todo.push_back(merge[(c - 1) + m]);
      todo.push_back(merge[c - 1]);
    }
  }
  if (n_repairs) *n_repairs = repairs;
  return at == n;
}

bool cutree_static(int64_t n, const int32_t* merge, const double* height, double cut_height, int64_t min_size,
                   int32_t* labels) {
  if (n < 1 || n > kHclustMaxNodes || std::isnan(cut_height)) return false;
  const int64_t m = n - 1;
  // parent step of every leaf (0 .. n - 1) and step (n + s); -1: the root
  std::vector<int64_t> parent((size_t)(n + m), -1);
  for (int64_t s = 0; s < m; ++s) {
    if (std::isnan(height[s])) return false;
    for (int col = 0; col < 2; ++col) {
      const int64_t c = merge[s + col * m];
      if (c == 0 || c < -n || c > s) return false;  // a step refers to earlier steps only
      const int64_t id = c < 0 ? -c - 1 : n + c - 1;
      if (parent[(size_t)id] >= 0) return false;
      parent[(size_t)id] = s;
    }
  }
  // the outermost applied step above every step (-1: none), root first
  std::vector<int64_t> top((size_t)std::max<int64_t>(m, 1), -1);
  for (int64_t s = m - 1; s >= 0; --s) {
    const int64_t p = parent[(size_t)(n + s)];
    if (p >= 0 && top[(size_t)p] >= 0)
      top[(size_t)s] = top[(size_t)p];
    else
      top[(size_t)s] = height[s] <= cut_height ? s : -1;
  }
  // R's cutree numbering: by first appearance in node order
  std::vector<int32_t> number_of_step((size_t)std::max<int64_t>(m, 1), 0);
  std::vector<int32_t> cut((size_t)n);
  std::vector<int64_t> sizes(1, 0);
  for (int64_t i = 0; i < n; ++i) {
    const int64_t p = parent[(size_t)i];
    const int64_t s = p >= 0 ? top[(size_t)p] : -1;
    int32_t c;
    if (s < 0) {
      c = (int32_t)sizes.size();
      sizes.push_back(0);
    } else {
      if (!number_of_step[(size_t)s]) {
        number_of_step[(size_t)s] = (int32_t)sizes.size();
        sizes.push_back(0);
      }
      c = number_of_step[(size_t)s];
    }
    cut[(size_t)i] = c;
    ++sizes[(size_t)c];
  }
  // clusters of min_size or more, by decreasing size, ties to the lower cutree number
  std::vector<int32_t> keep;
  for (int32_t c = 1; c < (int32_t)sizes.size(); ++c)
    if (sizes[(size_t)c] >= min_size) keep.push_back(c);
  std::stable_sort(keep.begin(), keep.end(), [&](int32_t a, int32_t b) { return sizes[(size_t)a] > sizes[(size_t)b]; });
  std::vector<int32_t> relabel(sizes.size(), 0);
  for (size_t r = 0; r < keep.size(); ++r) relabel[(size_t)keep[r]] = (int32_t)r + 1;
  for (int64_t i = 0; i < n; ++i) labels[i] = relabel[(size_t)cut[(size_t)i]];
  return true;
}

}  // namespace nr

extern "C" {

int nr_hclust_search_cap(int64_t n_nodes, int64_t* cap) {
  if (n_nodes < 1 || !cap) return NR_ERR_INVALID;
  *cap = nr::hclust_search_cap(n_nodes);
  return NR_OK;
}

int nr_hclust_error_message(int32_t word, char* buf, int64_t cap) {
  const char* text = nr::hclust_error_text(word);
  if (!text || !buf) return NR_ERR_INVALID;
  const size_t len = std::strlen(text);
  if (cap < (int64_t)len + 1) return NR_ERR_INVALID;
  std::memcpy(buf, text, len + 1);
  return NR_OK;
}

}  // extern "C"
