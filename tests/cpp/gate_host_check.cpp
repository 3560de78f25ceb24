// gate_host_check — icp4r_sequence_pairs' host code (csrc/icp4r_gate_pairs.hpp, the code the library
// entry wraps) against the node's literal accumulate-and-clear loop over std::vector clouds
// (src/iterative_closest_point.cpp:306-315, :505, :698-699), over every count vector of length <= 8
// with counts in {0, 3}.  Also asserts the two bounds the rule implies: a registered target holds at
// most one non-empty scan, a registered source at most two.  Built with -fsanitize=address,undefined
// and run as a program (tests/test_gate.py); prints "<cases> cases, <m> mismatches".
#include <cstdint>
#include <cstdio>
#include <vector>

#include "icp4r_gate_pairs.hpp"

namespace {

// the clouds as vectors of the scan index each point came from
std::vector<int32_t> expand(const std::vector<int32_t>& counts, int32_t first, int32_t last) {
    std::vector<int32_t> pts;
    for (int32_t s = first; s <= last; ++s)
        for (int32_t i = 0; i < counts[(size_t)s]; ++i) pts.push_back(s);
    return pts;
}

int nonempty(const std::vector<int32_t>& counts, int32_t first, int32_t last) {
    int c = 0;
    for (int32_t s = first; s <= last; ++s) c += counts[(size_t)s] > 0;
    return c;
}

int check(const std::vector<int32_t>& counts) {
    const int32_t n = (int32_t)counts.size();
    // exact-size outputs: an index past the end is a heap overflow the sanitizer reports
    std::vector<int32_t> sf((size_t)n), sl((size_t)n), tf((size_t)n), tl((size_t)n), reg((size_t)n);
    if (icp4r_gate::sequence_pairs(counts.data(), n, sf.data(), sl.data(), tf.data(), tl.data(), reg.data()) != -1) return 1;
    int bad = 0;
    std::vector<int32_t> cloud_src_in, cloud_tar_in;
    for (int32_t k = 0; k < n; ++k) {
        const int32_t last = k ? k - 1 : 0;
        for (int32_t i = 0; i < counts[(size_t)k]; ++i) cloud_src_in.push_back(k);
        for (int32_t i = 0; i < counts[(size_t)last]; ++i) cloud_tar_in.push_back(last);
        const bool registered = cloud_tar_in.size() && cloud_src_in.size();
        if (registered != (reg[(size_t)k] != 0)) ++bad;
        if (sf[(size_t)k] < 0 || sl[(size_t)k] >= n || tf[(size_t)k] < 0 || tl[(size_t)k] >= n) {
            ++bad;
            continue;
        }
        if (expand(counts, sf[(size_t)k], sl[(size_t)k]) != cloud_src_in) ++bad;
        if (expand(counts, tf[(size_t)k], tl[(size_t)k]) != cloud_tar_in) ++bad;
        if (registered) {
            if (nonempty(counts, tf[(size_t)k], tl[(size_t)k]) > 1) ++bad;
            if (nonempty(counts, sf[(size_t)k], sl[(size_t)k]) > 2) ++bad;
            cloud_src_in.clear();
            cloud_tar_in.clear();
        }
    }
    return bad;
}

}  // namespace

int main() {
    long cases = 0, mismatches = 0;
    for (int len = 0; len <= 8; ++len)
        for (int bits = 0; bits < (1 << len); ++bits) {
            std::vector<int32_t> counts((size_t)len);
            for (int k = 0; k < len; ++k) counts[(size_t)k] = (bits >> k) & 1 ? 3 : 0;
            mismatches += check(counts);
            ++cases;
        }
    // null outputs are allowed, and a negative count is refused with its index
    const int32_t neg[3] = {3, -1, 3};
    if (icp4r_gate::sequence_pairs(neg, 3, nullptr, nullptr, nullptr, nullptr, nullptr) != 1) ++mismatches;
    if (icp4r_gate::sequence_pairs(neg, 1, nullptr, nullptr, nullptr, nullptr, nullptr) != -1) ++mismatches;
    std::printf("%ld cases, %ld mismatches\n", cases, mismatches);
    return mismatches ? 1 : 0;
}
