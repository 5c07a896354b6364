// apd_sort.h -- the device sort and the device scan of the library (apd_sort.hip): a stable least-significant-digit radix sort of
// 64-bit keys with an optional 32-bit payload, and the 64-bit exclusive scan it is built on.  Written for gfx950 (wave64); no
// library underneath.  Nothing here decides a position with a global atomic: two runs over the same input write the same bytes.
// Every call runs on the current device's null stream and returns after its kernels were launched (a later copy or
// hipDeviceSynchronize waits for them), except where it says that it reads a result back.
#pragma once

#include <hip/hip_runtime.h>

#include <stddef.h>
#include <stdint.h>

namespace apd_sort {

constexpr int kDigitBits = 8;                 // one pass sorts by 8 bits of the key
constexpr int kDigits = 1 << kDigitBits;
constexpr int kSortThreads = 256;             // four waves
constexpr int kSortRounds = 8;                // a block takes its tile in rounds of kSortThreads consecutive elements
constexpr int kSortTile = kSortThreads * kSortRounds;  // elements of one block of k_sort_histogram / k_sort_scatter
constexpr int kScanThreads = 256;
constexpr int kScanItems = 8;                 // consecutive entries of one lane
constexpr int kScanTile = kScanThreads * kScanItems;   // entries of one block of the scan
constexpr int kScanTopThreads = 1024;         // the one workgroup that scans the sums of the scan's blocks
constexpr int kBitsBlocks = 256;              // workgroups of the OR / AND reduction of the keys

inline size_t sort_blocks(size_t n) { return (n + kSortTile - 1) / kSortTile; }
inline size_t scan_blocks(size_t n) { return (n + kScanTile - 1) / kScanTile; }

// out[i] = in[0] + ... + in[i - 1] for i = 0 .. n, so out[n] is the total: n + 1 entries.  n = 0 writes out[0] = 0.  Allocates
// and frees one sum per block of kScanTile entries.
hipError_t exclusive_scan(const uint32_t *in, uint64_t *out, size_t n);

// Sorts keys[0 .. n) ascending, stably; vals (may be null, then vals_alt too) are carried along.  keys_alt / vals_alt: n entries
// each, the other half of the double buffer.  *in_alt = 1: the result is in keys_alt / vals_alt, 0: in keys / vals; the other
// pair holds garbage.  A pass whose digit is the same in every key is skipped (one OR / AND reduction of the keys, read back
// here, finds them); *passes (may be null): the passes that ran.  Allocates and frees the [digit][block] table of a pass.
hipError_t sort_pairs(uint64_t *keys, uint64_t *keys_alt, uint32_t *vals, uint32_t *vals_alt, size_t n, int *in_alt, int *passes);

}  // namespace apd_sort
