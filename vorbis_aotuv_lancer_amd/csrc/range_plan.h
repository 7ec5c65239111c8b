// The host planner of vbm_synthesis_ranges (capi_decoder.cpp).  Pure host code over plain arrays, no HIP header: a
// stand-alone program can run it without a device (tests/native/range_plan_host.cpp).
#pragma once
#include <algorithm>
#include <vector>

namespace {                              // internal to the file that includes this: the library exports none of it
struct vbm_range_piece {
    int r, pre, first, count;            // output row, pre-roll packet, first packet after it, packets after it
};

struct vbm_range_plan {
    std::vector<vbm_range_piece> pieces;
    std::vector<int> call_first, call_r0;   // per sub-call: first piece (and the end of the last), first output row
};

// The packets of `got` > 0 samples from s of a stream whose packets are [a, b): k, the first with output past s; m, which
// holds sample s + got - 1; pre, the last valid packet (status 0) before k, the pre-roll.  False: there is none.
// (vbm_plan_ranges below, and the Ogg cut of ogg_cut.hip, which copies the packets pre .. m.)
inline bool vbm_range_find(long long a, long long b, const int *status, const long long *out_end, long long s,
                           long long got, int &k, int &m, int &pre)
{
    k = (int)(std::upper_bound(out_end + a, out_end + b, s) - out_end);
    m = (int)(std::upper_bound(out_end + a, out_end + b, s + got - 1) - out_end);
    pre = k - 1;
    while (pre >= a && status[pre] != 0) pre--;
    return pre >= a;
}

// The index: stream i has packets first[i] .. first[i + 1] - 1 and totals[i] samples; packet j has status[j] (0: it
// decodes) and out_end[j], its stream's samples up to and with it.  Range r: lengths[r] samples of stream stream_ids[r]
// from starts[r], all checked by the caller; got[r] becomes the samples of it that exist.  Per range the packets k (first
// with output past s) .. m (holds s + got - 1) after the pre-roll p (the last valid packet before k), cut into pieces
// of at most cap rows (cap >= 2); pieces packed into sub-calls of at most cap rows and cap output rows.
// -> nullptr, or the error of an index that no decode gives, with an empty plan
// last, lo (a live store's; live_store.h): stream i's packets end at last[i] instead of first[i + 1], and a range that
// starts before lo[i], the stream's first retained sample, gets nothing.
inline const char *vbm_plan_ranges(const long long *first, const long long *last, const long long *lo, const int *status,
                                   const long long *out_end, const long long *totals, int cap, int nranges,
                                   const int *stream_ids, const long long *starts, const int *lengths, int *got,
                                   vbm_range_plan *plan)
{
    *plan = {{}, {0}, {}};
    std::vector<vbm_range_piece> &pieces = plan->pieces;
    std::vector<int> &call_first = plan->call_first, &call_r0 = plan->call_r0;
    int rows = 0;
    for (int r = 0; r < nranges; r++) {
        const int i = stream_ids[r];
        const long long total = totals[i], s = starts[r];
        got[r] = (int)std::max(0LL, std::min(total - s, (long long)lengths[r]));
        if (lo && s < lo[i]) got[r] = 0;
        if (got[r] == 0) continue;
        int k, m, pre;
        if (!vbm_range_find(first[i], last[i], status, out_end, s, got[r], k, m, pre)) {   // lW >= 0 at k
            *plan = {};
            return "range store index: no pre-roll packet";
        }
        for (int f = pre + 1; f <= m;) {
            const int count = std::min(m - f + 1, cap - 1);
            if (rows + count + 1 > cap || (!call_r0.empty() && r - call_r0.back() >= cap)) {
                call_first.push_back((int)pieces.size());
                rows = 0;
            }
            if (call_r0.size() < call_first.size()) call_r0.push_back(r);
            pieces.push_back({r - call_r0.back(), pre, f, count});
            rows += count + 1;
            f += count;
            for (int j = f - 1; j > pre; j--)            // the next piece's pre-roll: this one's last valid packet
                if (status[j] == 0) { pre = j; break; }
        }
    }
    call_first.push_back((int)pieces.size());
    return nullptr;
}

// the plan over a plain store, whose streams lie back to back
inline const char *vbm_plan_ranges(const long long *first, const int *status, const long long *out_end,
                                   const long long *totals, int cap, int nranges, const int *stream_ids,
                                   const long long *starts, const int *lengths, int *got, vbm_range_plan *plan)
{
    return vbm_plan_ranges(first, first + 1, nullptr, status, out_end, totals, cap, nranges, stream_ids, starts, lengths,
                           got, plan);
}
}  // namespace
