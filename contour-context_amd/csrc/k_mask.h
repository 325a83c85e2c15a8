// Scan masks (cc_scan_mask_t): rows of bits, one per database scan, that restrict a query's retrieval to the scans whose bit
// is set (cc_knn_walk's MASK instances, k_knn.h).  Here: the rows of a position prior, made on the device.
#pragma once
#include "cc_dev.h"

// Bit g of row r = scan g lies within gate r's circle: with dx = x_g - x_r, dy = y_g - y_r the f32 sum dx * dx + dy * dy, as
// written (the library is built with -ffp-contract=off), is <= rad_r * rad_r, and rad_r >= 0.  A NaN anywhere fails every
// comparison and a negative radius the last one: no bit.  Bits n_scans .. 32 * row_words - 1 are written as 0.
// One wave takes 64 scans of a row, ballots, and lanes 0 and 1 store the two words.
// grid = n_rows * ceil(row_words / 2), block = 64
__global__ void __launch_bounds__(64)
cc_k_mask_gates(const float *__restrict__ xy /*[n_scans][2]*/, int n_scans, const float *__restrict__ gate /*[n_rows][3]*/,
                unsigned *__restrict__ bits /*[n_rows][row_words]*/, int row_words) {
  const int lane = threadIdx.x;
  const int per_row = (row_words + 1) >> 1;
  const int r = (int)blockIdx.x / per_row, b = (int)blockIdx.x - r * per_row;
  const float gx = gate[3 * r], gy = gate[3 * r + 1], rad = gate[3 * r + 2];
  const int g = b * 64 + lane;
  bool in = false;
  if (g < n_scans) {
    const float dx = xy[2 * (size_t)g] - gx, dy = xy[2 * (size_t)g + 1] - gy;
    in = rad >= 0.f && dx * dx + dy * dy <= rad * rad;
  }
  const unsigned long long m = __ballot(in);
  const int w = 2 * b + lane;
  if (lane < 2 && w < row_words) bits[(size_t)r * row_words + w] = lane == 0 ? (unsigned)m : (unsigned)(m >> 32);
}
