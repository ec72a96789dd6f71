// The device-wide exclusive scan of int32 (scan.hip) and the size of the scratch its callers hand it.
#pragma once

#include "common.hpp"

namespace ep {

constexpr int kScanTile = 2048;  // elements per workgroup: 256 threads x 8 items

// scratch of a scan over n elements: one int32 per tile (n = 0: none), and the same as a 256-byte aligned segment of a workspace.
// Grows with n: a scratch sized for a capacity serves every shorter scan.
constexpr int64_t scan_scratch_ints(int64_t n) { return (n + kScanTile - 1) / kScanTile; }
constexpr size_t scan_scratch_bytes(int64_t n) { return ((size_t)scan_scratch_ints(n) * sizeof(int32_t) + 255) / 256 * 256; }

// out[i] = sum of in[0 .. i); scratch holds scan_scratch_ints(n) int32; `total_dev` (optional) receives the grand total
int exclusive_scan_i32(const int32_t *in, int n, int32_t *out, int32_t *scratch, int32_t *total_dev,
                       hipStream_t st);
// the same with the live length on the device: min(n, *n_dev) (n_dev may be nullptr); launches are sized by n
int exclusive_scan_i32_dn(const int32_t *in, int n, const int32_t *n_dev, int32_t *out, int32_t *scratch, int32_t *total_dev,
                          hipStream_t st);

}  // namespace ep
