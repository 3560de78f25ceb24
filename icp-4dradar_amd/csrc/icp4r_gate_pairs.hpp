// icp4r_gate_pairs.hpp — the node's running-cloud pairing as range arithmetic (icp4r_sequence_pairs,
// include/icp4r/icp4r_gate.h).  Plain C++ with no device or library dependency: icp4r_gate.cpp wraps it,
// and tests/cpp/gate_host_check.cpp compiles it alone under the host sanitizers.
#pragma once

#include <stdint.h>

namespace icp4r_gate {

// Frame k appends scan k to the source cloud and scan k-1 (scan 0 for k = 0) to the target cloud
// (src/iterative_closest_point.cpp:306-315); it registers iff both then hold a point (:505), and only a
// registered frame clears them (:698-699).  The clouds are therefore the inclusive scan ranges written
// here (for a skipped frame: what has accumulated).  Any output may be null.  -> the first scan with a
// negative count, or -1.
inline int32_t sequence_pairs(const int32_t* counts, int32_t nscans, int32_t* src_first, int32_t* src_last,
                              int32_t* tgt_first, int32_t* tgt_last, int32_t* registered) {
    for (int32_t k = 0; k < nscans; ++k)
        if (counts[k] < 0) return k;
    int32_t sf = 0, tf = 0;  // first scan of the running source / target cloud
    int64_t src_pts = 0, tgt_pts = 0;
    for (int32_t k = 0; k < nscans; ++k) {
        const int32_t prev = k ? k - 1 : 0;
        src_pts += counts[k];
        tgt_pts += counts[prev];
        const int reg = src_pts > 0 && tgt_pts > 0;
        if (src_first) src_first[k] = sf;
        if (src_last) src_last[k] = k;
        if (tgt_first) tgt_first[k] = tf;
        if (tgt_last) tgt_last[k] = prev;
        if (registered) registered[k] = reg;
        if (reg) {  // cleared: the next frame appends scan k + 1 and scan k
            sf = k + 1;
            tf = k;
            src_pts = tgt_pts = 0;
        }
    }
    return -1;
}

}  // namespace icp4r_gate
