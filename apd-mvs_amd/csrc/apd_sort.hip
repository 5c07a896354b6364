// apd_sort.hip -- the device scan and the device radix sort of apd_sort.h.
//
// The scan (exclusive_scan): three kernels.  k_scan_sums adds up each block of kScanTile entries; k_scan_top, one workgroup, turns
// the block sums into block prefixes (every lane over a run of consecutive sums: scan_sums_in_place of apd_scan.h);
// k_scan_apply repeats a block's own scan in LDS and adds its prefix.  Sums and outputs are 64-bit.
//
// The sort (sort_pairs): least significant digit first, 8 bits a pass.  A pass is k_sort_histogram (per block of kSortTile
// elements the count of every digit, into a [digit][block] table), the scan of that table -- digit-major, so the scanned entry
// of (digit, block) is the position of the block's first element with that digit -- and k_sort_scatter, which ranks the
// elements of a block *stably*: a block walks its tile in rounds of 256 consecutive elements, a wave ranks its 64 by ballot (the
// peers of a lane are the lanes with the same digit: the AND over the digit's bits of `ballot(bit) == mine`; the rank is the
// number of peers below the lane), the four waves of a round are ordered by their per-wave counts in LDS, and the rounds by a
// running base per digit.  An element's position is therefore a function of the input alone.  The LDS atomics of the histogram
// count, they do not place.  Destinations of a wave are runs of one digit each, so the stores are scattered over up to 256
// streams per block; nothing is staged through LDS to widen them (the merge this sort serves is a small part of a fusion).
#include "apd_sort.h"

#include "../../include/apd_mi355x.h"
#include "apd_scan.h"

namespace apd_sort {

namespace {

constexpr int kWaves = kSortThreads / 64;

// k_sort_histogram and k_sort_scatter index count[t], base[t] and wave_count[w][t] by thread; the reductions and the Hillis-Steele
// scan of apd_scan.h halve or double their stride
static_assert(kSortThreads == kDigits, "one thread of a sort block per digit of the [kDigits] tables in LDS");
static_assert(kSortThreads % 64 == 0, "a sort block is whole waves: the ballots rank 64 lanes");
static_assert(kScanThreads > 0 && (kScanThreads & (kScanThreads - 1)) == 0, "k_scan_sums reduces with strides kScanThreads / 2, / 4, ... 1");
static_assert(kScanTopThreads > 0 && (kScanTopThreads & (kScanTopThreads - 1)) == 0, "kScanTopThreads is a power of two");

__global__ __launch_bounds__(kScanThreads) void k_scan_sums(const uint32_t *__restrict__ in, size_t n, uint64_t *__restrict__ sums)
{
    __shared__ uint64_t part[kScanThreads];
    const int t = threadIdx.x;
    const size_t first = (size_t)blockIdx.x * kScanTile + (size_t)t * kScanItems;
    uint64_t sum = 0;
    for (int j = 0; j < kScanItems; ++j) {
        sum += first + j < n ? in[first + j] : 0u;
    }
    part[t] = sum;
    __syncthreads();
    for (int off = kScanThreads / 2; off > 0; off >>= 1) {
        if (t < off) {
            part[t] += part[t + off];
        }
        __syncthreads();
    }
    if (t == 0) {
        sums[blockIdx.x] = part[0];
    }
}

// sums[b] becomes the sum of the blocks before b; sums[nblocks]: the total
__global__ __launch_bounds__(kScanTopThreads) void k_scan_top(uint64_t *__restrict__ sums, size_t nblocks)
{
    __shared__ uint64_t part[kScanTopThreads];
    const uint64_t total = apd_scan::scan_sums_in_place(sums, nblocks, part);
    if (threadIdx.x == kScanTopThreads - 1) {
        sums[nblocks] = total;
    }
}

__global__ __launch_bounds__(kScanThreads) void k_scan_apply(const uint32_t *__restrict__ in, size_t n, const uint64_t *__restrict__ sums,
                                                             size_t nblocks, uint64_t *__restrict__ out)
{
    __shared__ uint64_t part[kScanThreads];
    const int t = threadIdx.x;
    const size_t first = (size_t)blockIdx.x * kScanTile + (size_t)t * kScanItems;
    uint32_t item[kScanItems];
    uint64_t sum = 0;
    for (int j = 0; j < kScanItems; ++j) {
        item[j] = first + j < n ? in[first + j] : 0u;
        sum += item[j];
    }
    const uint64_t upto = apd_scan::block_inclusive_scan(part, t, sum);
    uint64_t run = sums[blockIdx.x] + upto - sum;
    for (int j = 0; j < kScanItems; ++j) {
        if (first + j < n) {
            out[first + j] = run;
        }
        run += item[j];
    }
    if (blockIdx.x == 0 && t == 0) {
        out[n] = sums[nblocks];
    }
}

// partial[b] = OR of the keys block b saw, partial[kBitsBlocks + b] = their AND (a block that saw none: 0 and all ones)
__global__ __launch_bounds__(256) void k_key_bits(const uint64_t *__restrict__ keys, size_t n, uint64_t *__restrict__ partial)
{
    __shared__ uint64_t any[256], all[256];
    const int t = threadIdx.x;
    uint64_t o = 0, a = ~0ull;
    for (size_t i = (size_t)blockIdx.x * 256 + t; i < n; i += (size_t)kBitsBlocks * 256) {
        const uint64_t k = keys[i];
        o |= k;
        a &= k;
    }
    any[t] = o;
    all[t] = a;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (t < off) {
            any[t] |= any[t + off];
            all[t] &= all[t + off];
        }
        __syncthreads();
    }
    if (t == 0) {
        partial[blockIdx.x] = any[0];
        partial[kBitsBlocks + blockIdx.x] = all[0];
    }
}

// table[digit * nblocks + block] = elements of the block's tile with that digit
__global__ __launch_bounds__(kSortThreads) void k_sort_histogram(const uint64_t *__restrict__ keys, size_t n, int shift,
                                                                 uint32_t *__restrict__ table, size_t nblocks)
{
    __shared__ uint32_t count[kDigits];
    const int t = threadIdx.x;
    count[t] = 0;
    __syncthreads();
    const size_t first = (size_t)blockIdx.x * kSortTile;
    for (int r = 0; r < kSortRounds; ++r) {
        const size_t i = first + (size_t)r * kSortThreads + t;
        if (i < n) {
            atomicAdd(&count[(keys[i] >> shift) & (kDigits - 1)], 1u);
        }
    }
    __syncthreads();
    table[(size_t)t * nblocks + blockIdx.x] = count[t];
}

// Element i of the block's tile goes to offsets[digit][block] + (elements of the tile before i with i's digit)
__global__ __launch_bounds__(kSortThreads) void k_sort_scatter(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ vals, size_t n,
                                                               int shift, const uint64_t *__restrict__ offsets, size_t nblocks,
                                                               uint64_t *__restrict__ keys_out, uint32_t *__restrict__ vals_out)
{
    __shared__ uint64_t base[kDigits];              // where the block's next element of a digit goes
    __shared__ uint32_t wave_count[kWaves][kDigits];  // this round: elements of a digit in each wave
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    base[t] = offsets[(size_t)t * nblocks + blockIdx.x];
    for (int w = 0; w < kWaves; ++w) {
        wave_count[w][t] = 0;
    }
    __syncthreads();
    const size_t first = (size_t)blockIdx.x * kSortTile;
    const uint64_t below = (1ull << lane) - 1ull;
    for (int r = 0; r < kSortRounds; ++r) {  // the same trip count in every lane: the ballots below are wave-wide
        const size_t i = first + (size_t)r * kSortThreads + t;
        const bool valid = i < n;
        const uint64_t key = valid ? keys[i] : 0;
        const uint32_t digit = (uint32_t)(key >> shift) & (kDigits - 1);
        uint64_t peers = __ballot(valid);  // lanes past the end are nobody's peers
        for (int b = 0; b < kDigitBits; ++b) {
            const bool mine = (digit >> b) & 1u;
            const uint64_t set = __ballot(mine);
            peers &= mine ? set : ~set;
        }
        const uint32_t rank = (uint32_t)__popcll(peers & below);
        if (valid && rank == 0) {
            wave_count[wave][digit] = (uint32_t)__popcll(peers);
        }
        __syncthreads();
        if (valid) {
            uint64_t at = base[digit] + rank;
            for (int w = 0; w < wave; ++w) {
                at += wave_count[w][digit];
            }
            keys_out[at] = key;
            if (vals) {
                vals_out[at] = vals[i];
            }
        }
        __syncthreads();
        uint32_t round = 0;
        for (int w = 0; w < kWaves; ++w) {
            round += wave_count[w][t];
            wave_count[w][t] = 0;
        }
        base[t] += round;
        __syncthreads();
    }
}

// hipFree on every way out
struct Buffer {
    void *p = nullptr;
    ~Buffer() { hipFree(p); }
    hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes > 0 ? bytes : 1); }
};

constexpr size_t kMaxGrid = 0x7fffffffull;

#define SORT_TRY(expr)                       \
    do {                                     \
        const hipError_t e_ = (expr);        \
        if (e_ != hipSuccess) {              \
            return e_;                       \
        }                                    \
    } while (0)

hipError_t scan_with(const uint32_t *in, uint64_t *out, size_t n, uint64_t *sums)
{
    const size_t nb = scan_blocks(n);
    hipLaunchKernelGGL(k_scan_sums, dim3((unsigned)nb), dim3(kScanThreads), 0, 0, in, n, sums);
    hipLaunchKernelGGL(k_scan_top, dim3(1), dim3(kScanTopThreads), 0, 0, sums, nb);
    hipLaunchKernelGGL(k_scan_apply, dim3((unsigned)nb), dim3(kScanThreads), 0, 0, in, n, (const uint64_t *)sums, nb, out);
    return hipGetLastError();
}

}  // namespace

hipError_t exclusive_scan(const uint32_t *in, uint64_t *out, size_t n)
{
    if (n == 0) {
        return hipMemset(out, 0, sizeof(uint64_t));
    }
    if (scan_blocks(n) > kMaxGrid) {
        return hipErrorInvalidValue;
    }
    Buffer sums;
    SORT_TRY(sums.alloc((scan_blocks(n) + 1) * sizeof(uint64_t)));
    SORT_TRY(scan_with(in, out, n, (uint64_t *)sums.p));
    return hipDeviceSynchronize();  // `sums` is freed on return
}

hipError_t sort_pairs(uint64_t *keys, uint64_t *keys_alt, uint32_t *vals, uint32_t *vals_alt, size_t n, int *in_alt, int *passes)
{
    *in_alt = 0;
    if (passes) {
        *passes = 0;
    }
    if (n < 2) {
        return hipSuccess;
    }
    const size_t nb = sort_blocks(n);
    const size_t entries = nb * (size_t)kDigits;
    if (nb > kMaxGrid || scan_blocks(entries) > kMaxGrid) {
        return hipErrorInvalidValue;
    }
    Buffer bits, table, offsets, sums;
    SORT_TRY(bits.alloc(2 * kBitsBlocks * sizeof(uint64_t)));
    SORT_TRY(table.alloc(entries * sizeof(uint32_t)));
    SORT_TRY(offsets.alloc((entries + 1) * sizeof(uint64_t)));
    SORT_TRY(sums.alloc((scan_blocks(entries) + 1) * sizeof(uint64_t)));
    // the bits that differ between keys: a digit without one is the same in every key, and its pass would move nothing
    hipLaunchKernelGGL(k_key_bits, dim3(kBitsBlocks), dim3(256), 0, 0, (const uint64_t *)keys, n, (uint64_t *)bits.p);
    SORT_TRY(hipGetLastError());
    uint64_t partial[2 * kBitsBlocks];
    SORT_TRY(hipMemcpy(partial, bits.p, sizeof(partial), hipMemcpyDeviceToHost));
    uint64_t any = 0, all = ~0ull;
    for (int b = 0; b < kBitsBlocks; ++b) {
        any |= partial[b];
        all &= partial[kBitsBlocks + b];
    }
    const uint64_t varying = any ^ all;
    uint64_t *k[2] = {keys, keys_alt};
    uint32_t *v[2] = {vals, vals_alt};
    int from = 0;
    for (int shift = 0; shift < 64; shift += kDigitBits) {
        if (((varying >> shift) & (uint64_t)(kDigits - 1)) == 0) {
            continue;
        }
        hipLaunchKernelGGL(k_sort_histogram, dim3((unsigned)nb), dim3(kSortThreads), 0, 0, (const uint64_t *)k[from], n, shift, (uint32_t *)table.p, nb);
        SORT_TRY(scan_with((const uint32_t *)table.p, (uint64_t *)offsets.p, entries, (uint64_t *)sums.p));
        hipLaunchKernelGGL(k_sort_scatter, dim3((unsigned)nb), dim3(kSortThreads), 0, 0, (const uint64_t *)k[from], (const uint32_t *)v[from], n, shift,
                           (const uint64_t *)offsets.p, nb, k[1 - from], v[1 - from]);
        SORT_TRY(hipGetLastError());
        from = 1 - from;
        if (passes) {
            ++*passes;
        }
    }
    *in_alt = from;
    return hipDeviceSynchronize();  // the buffers of the passes are freed on return
}

}  // namespace apd_sort

extern "C" void apd_sort_tile_sizes(int *sort_tile, int *scan_tile)
{
    *sort_tile = apd_sort::kSortTile;
    *scan_tile = apd_sort::kScanTile;
}
