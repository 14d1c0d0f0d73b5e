// The scale-free topology fit (sft_fit.h). The bin edges and memberships are
// plain fp64 expressions, written so that a restatement in any language gives
// the same bins bit for bit (no contraction into fused multiply-adds); the two
// least-squares fits run on centred sums in long double.
#include "sft_fit.h"

#include <algorithm>
#include <cmath>
#include <limits>
#include <vector>

#pragma STDC FP_CONTRACT OFF
#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace nr {

namespace {

const double kNaN = std::numeric_limits<double>::quiet_NaN();

// e_m = min + m (dx / B)
inline double edge(double mn, double dx, int n_breaks, int m) { return mn + (double)m * (dx / (double)n_breaks); }

}  // namespace

bool scale_free_bins(const double* k, int64_t n, int n_breaks, int32_t* bins, double* min_out, double* dx_out) {
  std::fill(bins, bins + n, 0);
  double mn = k[0], mx = k[0];
  for (int64_t i = 0; i < n; ++i) {
    if (!std::isfinite(k[i])) return false;
    mn = std::min(mn, k[i]);
    mx = std::max(mx, k[i]);
  }
  const double dx = mx - mn;
  if (!(dx > 0.0)) return false;
  for (int64_t i = 0; i < n; ++i) {
    int b = 1;
    for (int m = 1; m < n_breaks; ++m) b += k[i] > edge(mn, dx, n_breaks, m) ? 1 : 0;
    bins[i] = b;
  }
  if (min_out) *min_out = mn;
  if (dx_out) *dx_out = dx;
  return true;
}

void scale_free_fit(const double* k, int64_t n, int n_breaks, bool remove_first, double* out3) {
  out3[0] = out3[1] = out3[2] = kNaN;
  std::vector<int32_t> bins((size_t)n);
  double mn = 0.0, dx = 0.0;
  if (!scale_free_bins(k, n, n_breaks, bins.data(), &mn, &dx)) return;
  std::vector<double> sum((size_t)n_breaks, 0.0);
  std::vector<int64_t> count((size_t)n_breaks, 0);
  for (int64_t i = 0; i < n; ++i) {
    sum[(size_t)bins[i] - 1] += k[i];
    ++count[(size_t)bins[i] - 1];
  }
  std::vector<long double> x, y, d;
  for (int m = remove_first ? 1 : 0; m < n_breaks; ++m) {
    double dm = count[m] ? sum[m] / (double)count[m] : 0.0;
    if (count[m] == 0 || dm == 0.0) dm = (edge(mn, dx, n_breaks, m) + edge(mn, dx, n_breaks, m + 1)) / 2.0;
    const double pm = (double)count[m] / (double)n;
    d.push_back((long double)dm);
    x.push_back((long double)std::log10(dm));
    y.push_back((long double)std::log10(pm + 1e-9));
  }
  const size_t N = x.size();
  long double xm = 0, ym = 0, dmn = 0;
  for (size_t i = 0; i < N; ++i) {
    xm += x[i];
    ym += y[i];
    dmn += d[i];
  }
  xm /= N;
  ym /= N;
  dmn /= N;
  long double sxx = 0, sxy = 0, syy = 0, sxd = 0, sdd = 0, sdy = 0;
  for (size_t i = 0; i < N; ++i) {
    const long double xc = x[i] - xm, yc = y[i] - ym, dc = d[i] - dmn;
    sxx += xc * xc;
    sxy += xc * yc;
    syy += yc * yc;
    sxd += xc * dc;
    sdd += dc * dc;
    sdy += dc * yc;
  }
  const long double slope = sxy / sxx;
  long double ssr = 0;
  for (size_t i = 0; i < N; ++i) {
    const long double e = (y[i] - ym) - slope * (x[i] - xm);
    ssr += e * e;
  }
  out3[0] = (double)(1.0L - ssr / syy);
  out3[1] = (double)slope;
  if (N <= 3) return;
  const long double det = sxx * sdd - sxd * sxd;
  const long double b1 = (sxy * sdd - sdy * sxd) / det, b2 = (sdy * sxx - sxy * sxd) / det;
  long double ssr2 = 0;
  for (size_t i = 0; i < N; ++i) {
    const long double e = (y[i] - ym) - b1 * (x[i] - xm) - b2 * (d[i] - dmn);
    ssr2 += e * e;
  }
  const long double r2 = 1.0L - ssr2 / syy;
  out3[2] = (double)(1.0L - (1.0L - r2) * (long double)(N - 1) / (long double)(N - 3));
}

void sft_table_row(double power, const double* k, int64_t n, int n_breaks, bool remove_first, double* row,
                   int64_t stride) {
  double fit[3];
  scale_free_fit(k, n, n_breaks, remove_first, fit);
  double total = 0.0;
  for (int64_t i = 0; i < n; ++i) total += k[i];
  std::vector<double> v(k, k + n);
  std::sort(v.begin(), v.end());  // R's median: the mean of the two middle values for even n
  const double median = n % 2 ? v[(size_t)(n / 2)] : (v[(size_t)(n / 2 - 1)] + v[(size_t)(n / 2)]) / 2.0;
  row[kSftPower * stride] = power;
  row[kSftRsq * stride] = fit[0];
  row[kSftSlope * stride] = fit[1];
  row[kSftTruncRsq * stride] = fit[2];
  row[kSftMeanK * stride] = total / (double)n;
  row[kSftMedianK * stride] = median;
  row[kSftMaxK * stride] = v[(size_t)(n - 1)];
}

double sft_power_estimate(const double* table, int n_powers, double cut) {
  for (int m = 0; m < n_powers; ++m) {
    const double r2 = table[m + kSftRsq * n_powers], slope = table[m + kSftSlope * n_powers];
    const double sign = slope > 0.0 ? 1.0 : (slope < 0.0 ? -1.0 : 0.0);
    if (-sign * r2 > cut) return table[m + kSftPower * n_powers];  // false for NaN
  }
  return kNaN;
}

}  // namespace nr
