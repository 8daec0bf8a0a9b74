// What feature_norm.hip offers the other files of the library (host side).
#pragma once
#include "common.h"

// mean[r] = mean of row r of t [rows][P]: the library's only per-row mean over positions (one workgroup per row, the sum in
// double, CHAIN order, rounded once).  The caller checks the launch.
void feature_rowmean_launch(const float* t, int rows, int P, float* mean, hipStream_t stream);
