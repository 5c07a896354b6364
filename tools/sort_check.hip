// sort_check.hip -- the device sort and the device scan of csrc/apd_sort.h, called directly and held to plain host references, at the
// sizes, keys and values the callers of the library (voxel merge, radius filter) never produce:
//   sort_check --group scan_sizes | scan_values | sort_sizes | sort_keys | sort_large     one group of cases on the current device
//   sort_check --self-test                                                                 no HIP call: the comparisons themselves
// The code under test is the shipped one: the program includes the header and links libapd_mi355x.so.  References: a uint64_t running
// sum; std::stable_sort of (key, payload) pairs comparing keys only.  Every device buffer ends in kCanary canary words after its last
// legal entry.  One line per case, CHECK_<group>_<case>=<mismatching entries> (a failure adds the first one), then
// CHECK_<group>_cases=<count>.  The self-test damages reference results the way a subtly wrong kernel would and requires that the
// comparison reports every damage.  Built by __graft_entry__.build() into tools/_build/sort_check.
#include "../apd-mvs_amd/csrc/apd_sort.h"

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <string>
#include <utility>
#include <vector>

using apd_sort::kDigitBits;
using apd_sort::kDigits;
using apd_sort::kScanItems;
using apd_sort::kSortThreads;

namespace {

constexpr size_t T = apd_sort::kSortTile;        // elements of one workgroup of a sort pass
constexpr size_t S = apd_sort::kScanTile;        // entries of one workgroup of the scan
constexpr size_t P = apd_sort::kScanTopThreads;  // lanes of the one workgroup that scans the block sums
constexpr size_t kWave = 64;
constexpr size_t kTableTile = S / kDigits;       // sort blocks whose [digit][block] table fills one scan tile
constexpr size_t kTableTop = S * P / kDigits;    // sort blocks whose table gives every lane of the top scan one block sum
constexpr size_t kCanary = 64;
constexpr int kKeyDigits = 64 / kDigitBits;

template <typename W> constexpr W canary();
template <> constexpr uint64_t canary<uint64_t>() { return 0xC0DEC0DEC0DEC0DEull; }
template <> constexpr uint32_t canary<uint32_t>() { return 0xC0DEC0DEu; }
template <typename W> constexpr W filler();   // what a buffer the call has to write holds before it
template <> constexpr uint64_t filler<uint64_t>() { return 0xABABABABABABABABull; }
template <> constexpr uint32_t filler<uint32_t>() { return 0xABABABABu; }

// ---------------------------------------------------------------------------------------------------------------------------
// inputs
// ---------------------------------------------------------------------------------------------------------------------------

struct Rng {   // splitmix64
    uint64_t state;
    explicit Rng(uint64_t seed) : state(seed) {}
    uint64_t next()
    {
        uint64_t z = (state += 0x9E3779B97F4A7C15ull);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        return z ^ (z >> 31);
    }
};

// the seed of a case: FNV-1a of its name, so a case keeps its inputs when others are added
uint64_t seed_of(const std::string &name)
{
    uint64_t h = 0xCBF29CE484222325ull;
    for (const char c : name) {
        h = (h ^ (uint8_t)c) * 0x100000001B3ull;
    }
    return h;
}

uint64_t with_digit(uint64_t key, int position, uint64_t digit)
{
    const int shift = position * kDigitBits;
    return (key & ~((uint64_t)(kDigits - 1) << shift)) | ((digit & (uint64_t)(kDigits - 1)) << shift);
}

std::vector<uint32_t> iota(size_t n)
{
    std::vector<uint32_t> v(n);
    for (size_t i = 0; i < n; ++i) {
        v[i] = (uint32_t)i;
    }
    return v;
}

// ---------------------------------------------------------------------------------------------------------------------------
// references and comparisons (host only: the self-test runs them without a device)
// ---------------------------------------------------------------------------------------------------------------------------

struct Tally {
    size_t bad = 0;
    std::string first;
    void note(const char *what, size_t index, uint64_t got, uint64_t want)
    {
        if (bad++ == 0) {
            char text[200];
            snprintf(text, sizeof text, " first=%s[%zu] got=0x%llx want=0x%llx", what, index, (unsigned long long)got, (unsigned long long)want);
            first = text;
        }
    }
};

// `data` followed by the canary words: what goes up to the device, and what has to come back where nothing may be written
template <typename W> std::vector<W> image(const std::vector<W> &data)
{
    std::vector<W> v(data);
    v.resize(data.size() + kCanary, canary<W>());
    return v;
}

template <typename W> std::vector<W> blank_image(size_t n)
{
    std::vector<W> v(n, filler<W>());
    v.resize(n + kCanary, canary<W>());
    return v;
}

template <typename W> void check_canaries(Tally &t, const char *what, const std::vector<W> &got, size_t n)
{
    if (got.size() != n + kCanary) {
        t.note(what, got.size(), got.size(), n + kCanary);
        return;
    }
    for (size_t i = n; i < n + kCanary; ++i) {
        if (got[i] != canary<W>()) {
            t.note(what, i, got[i], canary<W>());
        }
    }
}

std::vector<uint64_t> scan_reference(const std::vector<uint32_t> &in)
{
    std::vector<uint64_t> out(in.size() + 1);
    uint64_t run = 0;
    for (size_t i = 0; i < in.size(); ++i) {
        out[i] = run;
        run += in[i];
    }
    out[in.size()] = run;
    return out;
}

// got_in: the input buffer as it came back (n entries + canaries); got_out: the output buffer (n + 1 entries + canaries)
void check_scan(Tally &t, const std::vector<uint32_t> &in, const std::vector<uint64_t> &want, const std::vector<uint32_t> &got_in,
                const std::vector<uint64_t> &got_out)
{
    const size_t n = in.size();
    check_canaries(t, "in_canary", got_in, n);
    check_canaries(t, "out_canary", got_out, n + 1);
    if (t.bad) {
        return;   // a buffer of another size: nothing below can be indexed
    }
    for (size_t i = 0; i < n; ++i) {
        if (got_in[i] != in[i]) {
            t.note("in", i, got_in[i], in[i]);
        }
    }
    for (size_t i = 0; i <= n; ++i) {
        if (got_out[i] != want[i]) {
            t.note("out", i, got_out[i], want[i]);
        }
    }
}

struct SortResult {   // the four buffers as they came back, each n entries + canaries (vals: empty when the call had none)
    std::vector<uint64_t> keys[2];
    std::vector<uint32_t> vals[2];
    int in_alt = -1, passes = -1;
};

// payload: vals, or the input index when vals is null
void sort_reference(const std::vector<uint64_t> &keys, const std::vector<uint32_t> *vals, std::vector<uint64_t> &want_keys,
                    std::vector<uint32_t> &want_vals)
{
    const size_t n = keys.size();
    std::vector<std::pair<uint64_t, uint32_t>> pairs(n);
    for (size_t i = 0; i < n; ++i) {
        pairs[i] = {keys[i], vals ? (*vals)[i] : (uint32_t)i};
    }
    std::stable_sort(pairs.begin(), pairs.end(), [](const std::pair<uint64_t, uint32_t> &a, const std::pair<uint64_t, uint32_t> &b) { return a.first < b.first; });
    want_keys.resize(n);
    want_vals.resize(n);
    for (size_t i = 0; i < n; ++i) {
        want_keys[i] = pairs[i].first;
        want_vals[i] = pairs[i].second;
    }
}

// the byte positions at which the keys differ: the passes that may not be skipped, and the only ones that may run
int passes_reference(const std::vector<uint64_t> &keys)
{
    if (keys.empty()) {
        return 0;
    }
    uint64_t any = 0, all = ~0ull;
    for (const uint64_t k : keys) {
        any |= k;
        all &= k;
    }
    int passes = 0;
    for (int d = 0; d < kKeyDigits; ++d) {
        passes += (((any ^ all) >> (d * kDigitBits)) & (uint64_t)(kDigits - 1)) != 0;
    }
    return passes;
}

// want_vals: null when the call had no payload.  With no pass to run (want_passes == 0) the result is the input, in place.
void check_sort(Tally &t, const std::vector<uint64_t> &want_keys, const std::vector<uint32_t> *want_vals, int want_passes, const SortResult &r)
{
    const size_t n = want_keys.size();
    for (int side = 0; side < 2; ++side) {
        check_canaries(t, side ? "keys_alt_canary" : "keys_canary", r.keys[side], n);
        if (want_vals) {
            check_canaries(t, side ? "vals_alt_canary" : "vals_canary", r.vals[side], n);
        }
    }
    if (r.passes != want_passes) {
        t.note("passes", 0, (uint64_t)(int64_t)r.passes, (uint64_t)want_passes);
    }
    if (r.in_alt != (r.passes & 1) || r.in_alt != (want_passes & 1)) {
        t.note("in_alt", 0, (uint64_t)(int64_t)r.in_alt, (uint64_t)(want_passes & 1));
    }
    if (r.keys[0].size() != n + kCanary || r.keys[1].size() != n + kCanary || (want_vals && (r.vals[0].size() != n + kCanary || r.vals[1].size() != n + kCanary))) {
        return;
    }
    const int side = want_passes == 0 ? 0 : (r.in_alt & 1);
    for (size_t i = 0; i < n; ++i) {
        if (r.keys[side][i] != want_keys[i]) {
            t.note("key", i, r.keys[side][i], want_keys[i]);
        }
    }
    if (want_vals) {
        for (size_t i = 0; i < n; ++i) {
            if (r.vals[side][i] != (*want_vals)[i]) {
                t.note("val", i, r.vals[side][i], (*want_vals)[i]);
            }
        }
    }
}

// two runs over the same input: the same answer, byte for byte, on the side that holds it
void check_same(Tally &t, const SortResult &a, const SortResult &b)
{
    if (a.in_alt != b.in_alt || a.passes != b.passes) {
        t.note("second_run_in_alt_passes", 0, (uint64_t)(int64_t)(b.in_alt * 16 + b.passes), (uint64_t)(int64_t)(a.in_alt * 16 + a.passes));
        return;
    }
    const int side = a.in_alt & 1;
    if (a.keys[side].size() != b.keys[side].size() || a.vals[side].size() != b.vals[side].size()) {
        t.note("second_run_size", 0, b.keys[side].size(), a.keys[side].size());
        return;
    }
    for (size_t i = 0; i < a.keys[side].size(); ++i) {
        if (a.keys[side][i] != b.keys[side][i]) {
            t.note("second_run_key", i, b.keys[side][i], a.keys[side][i]);
        }
    }
    for (size_t i = 0; i < a.vals[side].size(); ++i) {
        if (a.vals[side][i] != b.vals[side][i]) {
            t.note("second_run_val", i, b.vals[side][i], a.vals[side][i]);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// the device
// ---------------------------------------------------------------------------------------------------------------------------

#define HIP_OK(expr)                                                                                        \
    do {                                                                                                    \
        const hipError_t e_ = (expr);                                                                       \
        if (e_ != hipSuccess) {                                                                             \
            printf("HIP error: %s (%s) at %s:%d\n", hipGetErrorString(e_), #expr, __FILE__, __LINE__);      \
            fflush(stdout);                                                                                 \
            exit(2); /* no further case is started */                                                       \
        }                                                                                                   \
    } while (0)

template <typename W> struct DeviceBuffer {   // holds what `host_image` holds: the entries and the canary words after them
    W *p = nullptr;
    size_t words;
    explicit DeviceBuffer(const std::vector<W> &host_image) : words(host_image.size())
    {
        HIP_OK(hipMalloc((void **)&p, words * sizeof(W)));
        HIP_OK(hipMemcpy(p, host_image.data(), words * sizeof(W), hipMemcpyHostToDevice));
    }
    DeviceBuffer(const DeviceBuffer &) = delete;
    DeviceBuffer &operator=(const DeviceBuffer &) = delete;
    ~DeviceBuffer() { HIP_OK(hipFree(p)); }
    std::vector<W> download() const
    {
        std::vector<W> v(words);
        HIP_OK(hipMemcpy(v.data(), p, words * sizeof(W), hipMemcpyDeviceToHost));
        return v;
    }
};

struct Group {
    std::string name;
    int cases = 0;
    size_t bad = 0;
};

void report(Group &g, const std::string &name, const Tally &t)
{
    printf("CHECK_%s_%s=%zu%s\n", g.name.c_str(), name.c_str(), t.bad, t.first.c_str());
    fflush(stdout);
    ++g.cases;
    g.bad += t.bad;
}

void scan_case(Group &g, const std::string &name, const std::vector<uint32_t> &in)
{
    const size_t n = in.size();
    std::vector<uint32_t> got_in;
    std::vector<uint64_t> got_out;
    {
        DeviceBuffer<uint32_t> d_in(image(in));
        DeviceBuffer<uint64_t> d_out(blank_image<uint64_t>(n + 1));
        HIP_OK(apd_sort::exclusive_scan(d_in.p, d_out.p, n));
        HIP_OK(hipDeviceSynchronize());
        got_in = d_in.download();
        got_out = d_out.download();
    }
    Tally t;
    check_scan(t, in, scan_reference(in), got_in, got_out);
    report(g, name, t);
}

SortResult run_sort(const std::vector<uint64_t> &keys, const std::vector<uint32_t> *vals)
{
    const size_t n = keys.size();
    SortResult r;
    DeviceBuffer<uint64_t> k0(image(keys)), k1(blank_image<uint64_t>(n));
    if (vals) {
        DeviceBuffer<uint32_t> v0(image(*vals)), v1(blank_image<uint32_t>(n));
        HIP_OK(apd_sort::sort_pairs(k0.p, k1.p, v0.p, v1.p, n, &r.in_alt, &r.passes));
        HIP_OK(hipDeviceSynchronize());
        r.vals[0] = v0.download();
        r.vals[1] = v1.download();
    } else {
        HIP_OK(apd_sort::sort_pairs(k0.p, k1.p, nullptr, nullptr, n, &r.in_alt, &r.passes));
        HIP_OK(hipDeviceSynchronize());
    }
    r.keys[0] = k0.download();
    r.keys[1] = k1.download();
    return r;
}

void sort_case(Group &g, const std::string &name, const std::vector<uint64_t> &keys, const std::vector<uint32_t> *vals)
{
    Tally t;
    const SortResult r = run_sort(keys, vals);
    {
        const SortResult again = run_sort(keys, vals);
        check_same(t, r, again);
    }
    std::vector<uint64_t> want_keys;
    std::vector<uint32_t> want_vals;
    sort_reference(keys, vals, want_keys, want_vals);
    check_sort(t, want_keys, vals ? &want_vals : nullptr, passes_reference(keys), r);
    report(g, name, t);
}

// ---------------------------------------------------------------------------------------------------------------------------
// the groups
// ---------------------------------------------------------------------------------------------------------------------------

std::string sized(const char *stem, size_t n)
{
    return std::string(stem) + "_n" + std::to_string(n);
}

void group_scan_sizes(Group &g)
{
    const size_t I = kScanItems;
    const size_t sizes[] = {0, 1, 2, I - 1, I, I + 1, S - 1, S, S + 1, 3 * S + 17,
                            S * P - 1, S * P, S * P + 1,   // the last: the first with two block sums in a lane of the top scan
                            S * (P + 1) + 1,               // P + 2 blocks, two to a lane: the upper half of the lanes owns none
                            2 * S * P + 1, 3 * S * P + 5 * S + 3};
    for (const size_t n : sizes) {
        const std::string name = sized("random", n);
        Rng rng(seed_of(g.name + name));
        std::vector<uint32_t> in(n);
        for (auto &x : in) {
            x = (uint32_t)(rng.next() & 3);
        }
        scan_case(g, name, in);
        scan_case(g, sized("ones", n), std::vector<uint32_t>(n, 1u));
    }
}

void group_scan_values(Group &g)
{
    const size_t n = 3 * S + 17;
    scan_case(g, sized("zeros", n), std::vector<uint32_t>(n, 0u));
    for (const size_t m : {(size_t)2, S + 1, S * P + 1}) {   // the total passes 2^32 at the second entry
        scan_case(g, sized("all_ones_bits", m), std::vector<uint32_t>(m, 0xFFFFFFFFu));
    }
    for (const size_t m : {3 * S + 17, S * P + 1}) {
        const std::string name = sized("random32", m);
        Rng rng(seed_of(g.name + name));
        std::vector<uint32_t> in(m);
        for (auto &x : in) {
            x = (uint32_t)rng.next();
        }
        scan_case(g, name, in);
    }
    for (const size_t at : {(size_t)0, S - 1, S, n - 1}) {
        std::vector<uint32_t> in(n, 0u);
        in[at] = 0x80000001u;
        scan_case(g, sized("single_at", at), in);
    }
}

std::vector<uint64_t> random_keys(const std::string &name, size_t n)
{
    Rng rng(seed_of(name));
    std::vector<uint64_t> keys(n);
    for (auto &k : keys) {
        k = rng.next();
    }
    return keys;
}

void group_sort_sizes(Group &g)
{
    const size_t sizes[] = {0, 1, 2, kWave - 1, kWave, kWave + 1, (size_t)kSortThreads - 1, (size_t)kSortThreads, (size_t)kSortThreads + 1,
                            T - 1, T, T + 1, 3 * T + 17, 5 * T + 3 * kSortThreads + 17,
                            kTableTile * T, kTableTile * T + 1,   // the table of a pass: one scan tile, and one entry more
                            100 * T + 5};
    for (const size_t n : sizes) {
        const std::string name = sized("random", n);
        const std::vector<uint32_t> vals = iota(n);
        sort_case(g, name, random_keys(g.name + name, n), &vals);
    }
}

// every case with its payload and again without one
void both(Group &g, const std::string &name, const std::vector<uint64_t> &keys, const std::vector<uint32_t> &vals)
{
    sort_case(g, name, keys, &vals);
    sort_case(g, name + "_novals", keys, nullptr);
}

void group_sort_keys(Group &g)
{
    const size_t n = 3 * T + 17;
    const std::vector<uint32_t> index = iota(n);
    const uint64_t fixed = 0xA5A5A5A5A5A5A5A5ull;   // the digits that do not vary are not zero
    auto keys_of = [&](const std::string &name, size_t count, auto &&make) {
        Rng rng(seed_of(g.name + name));
        std::vector<uint64_t> keys(count);
        for (size_t i = 0; i < count; ++i) {
            keys[i] = make(i, rng);
        }
        return keys;
    };
    both(g, "all_zero", std::vector<uint64_t>(n, 0ull), index);
    both(g, "all_ones", std::vector<uint64_t>(n, ~0ull), index);
    for (int d = 0; d < kKeyDigits; ++d) {
        const std::string name = "digit" + std::to_string(d);
        both(g, name, keys_of(name, n, [&](size_t, Rng &rng) { return with_digit(fixed, d, rng.next()); }), index);
    }
    for (const int bit : {0, kDigitBits - 1, kDigitBits, 63}) {
        const std::string name = "bit" + std::to_string(bit);
        both(g, name, keys_of(name, n, [&](size_t, Rng &rng) { return (fixed & ~(1ull << bit)) | ((rng.next() & 1ull) << bit); }), index);
    }
    both(g, "digits_1_and_5", keys_of("digits_1_and_5", n, [&](size_t, Rng &rng) { return with_digit(with_digit(fixed, 1, rng.next()), 5, rng.next()); }), index);
    {
        std::vector<uint64_t> keys = random_keys(g.name + "sorted", n);
        std::sort(keys.begin(), keys.end());
        both(g, "sorted", keys, index);
        std::reverse(keys.begin(), keys.end());
        both(g, "reversed", keys, index);
    }
    for (const size_t distinct : {(size_t)2, (size_t)4, (size_t)kDigits}) {   // long runs of equal keys: the payload shows their order
        const std::string name = "distinct" + std::to_string(distinct);
        const std::vector<uint64_t> pool = random_keys(g.name + name + "pool", distinct);
        both(g, name, keys_of(name, n, [&](size_t, Rng &rng) { return pool[rng.next() % distinct]; }), index);
    }
    // every wave on one digit (each lane's peers: the whole wave), low and top digit
    both(g, "wave_uniform", keys_of("wave_uniform", n, [&](size_t i, Rng &) {
             const uint64_t w = i / kWave;
             return with_digit(with_digit(0, 0, w), kKeyDigits - 1, ~w);
         }), index);
    // every lane of a wave on a digit of its own
    both(g, "lanes_distinct", keys_of("lanes_distinct", n, [&](size_t i, Rng &) {
             const uint64_t d = i % kWave + kWave * ((i / kWave) & 3);
             return with_digit(with_digit(0, 0, d), kKeyDigits - 1, ~d);
         }), index);
    // one digit for the whole of the second tile, that digit and others in the tiles either side
    both(g, "whole_tile", keys_of("whole_tile", n, [&](size_t i, Rng &rng) {
             const uint64_t r = rng.next();
             return i / T == 1 ? with_digit(fixed, 2, 7) : with_digit(fixed, 2, 5 + r % 5);
         }), index);
    for (const size_t m : {kWave + 1, T + 1, n}) {   // digit 0 in a last, partly filled wave: the lanes past the end read key 0
        const std::string name = sized("digits_0_to_3", m);
        both(g, name, keys_of(name, m, [&](size_t, Rng &rng) {
                 const uint64_t r = rng.next();
                 return with_digit(with_digit(0, 0, r & 3), kKeyDigits - 1, (r >> 2) & 3);
             }), iota(m));
    }
    {
        const std::vector<uint64_t> pool = random_keys(g.name + "random_payload_pool", 16);
        Rng rng(seed_of(g.name + "random_payload_vals"));
        std::vector<uint32_t> vals(n);
        for (size_t i = 0; i < n; ++i) {
            const uint64_t r = rng.next();
            vals[i] = r % 7 == 0 ? 0xFFFFFFFFu : (uint32_t)(r >> 32);
        }
        both(g, "random_payload", keys_of("random_payload", n, [&](size_t, Rng &rng2) { return pool[rng2.next() % 16]; }), vals);
    }
}

void group_sort_large(Group &g)
{
    // the [digit][block] table of kTableTop blocks gives every lane of the top scan one block sum; one block more, two.  Low digit
    // random, top digit one of four values on both halves of its range: two passes, equal keys many and far apart.
    const uint64_t top[4] = {0, kDigits / 2 - 1, kDigits / 2, kDigits - 1};
    for (const size_t n : {kTableTop * T, kTableTop * T + 1}) {
        const std::string name = sized("two_digits", n);
        Rng rng(seed_of(g.name + name));
        std::vector<uint64_t> keys(n);
        for (auto &k : keys) {
            const uint64_t r = rng.next();
            k = with_digit(with_digit(0, 0, r), kKeyDigits - 1, top[(r >> 32) & 3]);
        }
        const std::vector<uint32_t> vals = iota(n);
        sort_case(g, name, keys, &vals);
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// the self-test: no HIP call.  A reference result passes; each damage of it is reported.
// ---------------------------------------------------------------------------------------------------------------------------

struct SelfTest {
    int damages = 0, caught = 0;
    void expect_clean(const char *what, const Tally &t)
    {
        printf("SELFTEST_clean_%s=%zu%s\n", what, t.bad, t.first.c_str());
        ++damages;
        caught += t.bad == 0;
    }
    void expect_caught(const char *what, const Tally &t)
    {
        printf("SELFTEST_%s=%s%s\n", what, t.bad ? "caught" : "MISSED", t.first.c_str());
        ++damages;
        caught += t.bad != 0;
    }
};

// what a right sort_pairs leaves: the answer and canaries on the side the parity names, filler on the other
SortResult right_sort_result(const std::vector<uint64_t> &want_keys, const std::vector<uint32_t> &want_vals, int passes)
{
    SortResult r;
    r.passes = passes;
    r.in_alt = passes & 1;
    r.keys[r.in_alt] = image(want_keys);
    r.vals[r.in_alt] = image(want_vals);
    r.keys[1 - r.in_alt] = blank_image<uint64_t>(want_keys.size());
    r.vals[1 - r.in_alt] = blank_image<uint32_t>(want_vals.size());
    return r;
}

int self_test()
{
    SelfTest st;
    for (const size_t n : {(size_t)5, kWave + 1, (size_t)300}) {
        const std::string tag = "n" + std::to_string(n);
        // ---- the scan: entries near 2^32, so the total is past it
        Rng rng(seed_of("self_test_scan" + tag));
        std::vector<uint32_t> in(n);
        for (auto &x : in) {
            x = 0xFFFFFF00u + (uint32_t)(rng.next() & 0xFF);
        }
        const std::vector<uint64_t> want = scan_reference(in);
        const std::vector<uint32_t> in_image = image(in);
        const std::vector<uint64_t> out_image = image(want);
        auto scan_with = [&](auto &&damage) {
            std::vector<uint32_t> got_in = in_image;
            std::vector<uint64_t> got_out = out_image;
            damage(got_in, got_out);
            Tally t;
            check_scan(t, in, want, got_in, got_out);
            return t;
        };
        st.expect_clean(("scan_" + tag).c_str(), scan_with([](auto &, auto &) {}));
        st.expect_caught(("scan_off_by_one_from_an_index_on_" + tag).c_str(), scan_with([&](auto &, auto &out) {
            for (size_t i = n / 2; i <= n; ++i) {
                out[i] += 1;
            }
        }));
        st.expect_caught(("scan_total_truncated_to_32_bits_" + tag).c_str(), scan_with([&](auto &, auto &out) { out[n] &= 0xFFFFFFFFull; }));
        st.expect_caught(("scan_last_element_dropped_" + tag).c_str(), scan_with([&](auto &, auto &out) { out[n] = filler<uint64_t>(); }));
        st.expect_caught(("scan_last_input_dropped_" + tag).c_str(), scan_with([&](auto &, auto &out) { out[n] = out[n - 1]; }));
        st.expect_caught(("scan_canary_overwritten_" + tag).c_str(), scan_with([&](auto &, auto &out) { out[n + 1] = want[n]; }));
        st.expect_caught(("scan_input_canary_overwritten_" + tag).c_str(), scan_with([&](auto &got_in, auto &) { got_in[n] = 0; }));
        st.expect_caught(("scan_input_changed_" + tag).c_str(), scan_with([&](auto &got_in, auto &) { got_in[n / 2] ^= 1u; }));

        // ---- the sort: four distinct keys that differ in the lowest and the highest digit (two passes), and in the lowest alone (one)
        for (const int passes : {2, 1}) {
            const std::string stag = tag + "_passes" + std::to_string(passes);
            Rng krng(seed_of("self_test_sort" + stag));
            std::vector<uint64_t> keys(n);
            for (size_t i = 0; i < n; ++i) {
                const uint64_t r = i < 4 ? i : krng.next() & 3;   // each of the four at least once
                keys[i] = passes == 2 ? with_digit(with_digit(0, 0, r & 1), kKeyDigits - 1, kDigits / 2 - 1 + (r >> 1)) : r;
            }
            const std::vector<uint32_t> vals = iota(n);
            std::vector<uint64_t> want_keys;
            std::vector<uint32_t> want_vals;
            sort_reference(keys, &vals, want_keys, want_vals);
            if (passes_reference(keys) != passes) {
                printf("SELFTEST_passes_reference_%s=MISSED\n", stag.c_str());
                ++st.damages;
                continue;
            }
            const SortResult right = right_sort_result(want_keys, want_vals, passes);
            const int side = right.in_alt;
            auto sort_with = [&](bool with_vals, auto &&damage) {
                SortResult r = right;
                if (!with_vals) {
                    r.vals[0].clear();
                    r.vals[1].clear();
                }
                damage(r);
                Tally t;
                check_sort(t, want_keys, with_vals ? &want_vals : nullptr, passes, r);
                return t;
            };
            st.expect_clean(("sort_" + stag).c_str(), sort_with(true, [](SortResult &) {}));
            st.expect_clean(("sort_novals_" + stag).c_str(), sort_with(false, [](SortResult &) {}));
            size_t pair_at = n;
            for (size_t i = 0; i + 1 < n && pair_at == n; ++i) {
                if (want_keys[i] == want_keys[i + 1]) {
                    pair_at = i;
                }
            }
            st.expect_caught(("sort_equal_neighbours_swapped_" + stag).c_str(), sort_with(true, [&](SortResult &r) {
                if (pair_at < n) {
                    std::swap(r.vals[side][pair_at], r.vals[side][pair_at + 1]);
                }
            }));
            st.expect_caught(("sort_last_element_dropped_" + stag).c_str(), sort_with(true, [&](SortResult &r) {
                r.keys[side][n - 1] = filler<uint64_t>();
                r.vals[side][n - 1] = filler<uint32_t>();
            }));
            st.expect_caught(("sort_last_key_dropped_novals_" + stag).c_str(), sort_with(false, [&](SortResult &r) { r.keys[side][n - 1] = filler<uint64_t>(); }));
            st.expect_caught(("sort_last_payload_dropped_" + stag).c_str(), sort_with(true, [&](SortResult &r) { r.vals[side][n - 1] = filler<uint32_t>(); }));
            for (int s = 0; s < 2; ++s) {
                const std::string where = (s == side ? "result_side_" : "other_side_") + stag;
                st.expect_caught(("sort_key_canary_overwritten_" + where).c_str(), sort_with(true, [&](SortResult &r) { r.keys[s][n] = want_keys[n - 1]; }));
                st.expect_caught(("sort_payload_canary_overwritten_" + where).c_str(), sort_with(true, [&](SortResult &r) { r.vals[s][n + kCanary - 1] = 0; }));
            }
            // both sides hold the answer: only the parity rule can tell
            st.expect_caught(("sort_in_alt_flipped_" + stag).c_str(), sort_with(true, [&](SortResult &r) {
                r.keys[1 - side] = r.keys[side];
                r.vals[1 - side] = r.vals[side];
                r.in_alt = 1 - r.in_alt;
            }));
            st.expect_caught(("sort_passes_one_too_many_" + stag).c_str(), sort_with(true, [&](SortResult &r) {
                r.keys[1 - side] = r.keys[side];
                r.vals[1 - side] = r.vals[side];
                r.passes += 1;
                r.in_alt = r.passes & 1;
            }));
            {
                SortResult again = right;
                std::swap(again.vals[side][0], again.vals[side][n - 1]);
                Tally t;
                check_same(t, right, again);
                st.expect_caught(("sort_second_run_differs_" + stag).c_str(), t);
                Tally same;
                check_same(same, right, right);
                st.expect_clean(("sort_second_run_" + stag).c_str(), same);
            }
        }
    }
    {   // every key equal: no pass may run, and the keys and payloads stay where they were
        const size_t n = 70;
        const std::vector<uint64_t> keys(n, 0x0123456789ABCDEFull);
        const std::vector<uint32_t> vals = iota(n);
        SortResult moved = right_sort_result(keys, vals, 0);
        std::swap(moved.keys[0], moved.keys[1]);
        std::swap(moved.vals[0], moved.vals[1]);
        moved.in_alt = 1;
        Tally t;
        check_sort(t, keys, &vals, passes_reference(keys), moved);
        st.expect_caught("sort_no_pass_but_result_moved", t);
        Tally clean;
        check_sort(clean, keys, &vals, passes_reference(keys), right_sort_result(keys, vals, 0));
        st.expect_clean("sort_no_pass", clean);
    }
    printf("SELFTEST_checks=%d passed=%d\n", st.damages, st.caught);
    return st.damages == st.caught ? 0 : 1;
}

int usage()
{
    printf("usage: sort_check --group scan_sizes|scan_values|sort_sizes|sort_keys|sort_large\n       sort_check --self-test\n");
    return 2;
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc == 2 && strcmp(argv[1], "--self-test") == 0) {
        return self_test();
    }
    if (argc != 3 || strcmp(argv[1], "--group") != 0) {
        return usage();
    }
    const struct {
        const char *name;
        void (*run)(Group &);
    } groups[] = {{"scan_sizes", group_scan_sizes}, {"scan_values", group_scan_values}, {"sort_sizes", group_sort_sizes},
                  {"sort_keys", group_sort_keys}, {"sort_large", group_sort_large}};
    for (const auto &entry : groups) {
        if (strcmp(argv[2], entry.name) == 0) {
            Group g;
            g.name = entry.name;
            const auto start = std::chrono::steady_clock::now();
            entry.run(g);
            printf("CHECK_%s_cases=%d\n", g.name.c_str(), g.cases);
            printf("TIME_%s_seconds=%.2f\n", g.name.c_str(), std::chrono::duration<double>(std::chrono::steady_clock::now() - start).count());
            return g.bad == 0 ? 0 : 1;
        }
    }
    return usage();
}
