// The scale-free topology fit of WGCNA's pickSoftThreshold
// (scaleFreeFitIndex with R's current cut() binning) and the table built from
// it, as pure host functions: no context, no HIP call, so they run -- and are
// tested (tests/test_sft_host.py) -- on a machine without a GPU.
// include/netrep_gpu.h (netrep_ScaleFreeFit) has the definition.
#pragma once
#include <stdint.h>

namespace nr {

// Columns of a pickSoftThreshold table row.
enum { kSftPower = 0, kSftRsq, kSftSlope, kSftTruncRsq, kSftMeanK, kSftMedianK, kSftMaxK, kSftTableCols };

// bins[i] = the bin (1 .. n_breaks) of k[i]; false (bins all 0) if k holds a
// non-finite value or max k == min k. min_out / dx_out (optional): the range.
bool scale_free_bins(const double* k, int64_t n, int n_breaks, int32_t* bins, double* min_out, double* dx_out);

// out3 = {R^2 of y ~ x, its slope, adjusted R^2 of y ~ x + d}; NaNs where
// scale_free_bins is false (and out3[2] where fewer than four bins remain).
void scale_free_fit(const double* k, int64_t n, int n_breaks, bool remove_first, double* out3);

// One table row (kSftTableCols values, stride `stride`) of `power` from its
// connectivities k[n].
void sft_table_row(double power, const double* k, int64_t n, int n_breaks, bool remove_first, double* row,
                   int64_t stride);

// The first power of the table (n_powers x kSftTableCols, column-major) with
// -sign(slope) R^2 > cut; NaN if none.
double sft_power_estimate(const double* table, int n_powers, double cut);

}  // namespace nr
