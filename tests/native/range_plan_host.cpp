// The range planner of vbm_synthesis_ranges (csrc/range_plan.h) on seeded synthetic indexes, stand-alone: no device,
// no library.  Every plan is checked against a linear scan of the index (tests/test_range_plan_cpu.py builds and runs
// this, plain and under the address and undefined-behaviour sanitizers).  Exit status 0 and a count line, or 1 and what
// failed.
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "range_plan.h"

namespace {

struct Index {
    std::vector<long long> first{0}, out_end, totals;
    std::vector<int> status, stream_of;
};

struct Rng {                              // xorshift64*: the same sequence with every compiler
    uint64_t s;
    uint64_t next()
    {
        s ^= s >> 12;
        s ^= s << 25;
        s ^= s >> 27;
        return s * 0x2545F4914F6CDD1DULL;
    }
    long long below(long long n) { return (long long)((next() >> 11) % (uint64_t)n); }
};

// streams of 0 or 1 .. 200 packets; a packet fails (status != 0, no samples) or gives 0, 128 or 1024 samples, none
// before its stream's first good packet, as a decoder's first block gives none
Index make_index(Rng &g, int nstreams)
{
    Index ix;
    for (int i = 0; i < nstreams; i++) {
        const int n = g.below(5) == 0 ? 0 : 1 + (int)g.below(g.below(3) == 0 ? 200 : 12);
        const int fail_one_in = 2 + (int)g.below(8);
        long long run = 0;
        bool primed = false;
        for (int j = 0; j < n; j++) {
            const bool failed = g.below(fail_one_in) == 0;
            const long long samples[3] = {0, 128, 1024};
            if (!failed && primed) run += samples[g.below(3)];
            primed |= !failed;
            ix.status.push_back(failed ? -136 : 0);
            ix.out_end.push_back(run);
            ix.stream_of.push_back(i);
        }
        ix.first.push_back((long long)ix.status.size());
        ix.totals.push_back(run);
    }
    return ix;
}

struct Ranges {
    std::vector<int> ids, lengths;
    std::vector<long long> starts;
    void add(int i, long long s, long long n)
    {
        ids.push_back(i);
        starts.push_back(s);
        lengths.push_back((int)n);
    }
};

Ranges make_ranges(Rng &g, const Index &ix, int flavour)
{
    Ranges rs;
    const int S = (int)ix.totals.size();
    if (flavour == 0) {                                  // the edges of every stream
        for (int i = 0; i < S; i++) {
            const long long t = ix.totals[i];
            rs.add(i, 0, 0);
            rs.add(i, 0, 1);
            rs.add(i, 0, t);                             // the whole stream
            rs.add(i, 0, t + 1000);
            rs.add(i, t, 5);                             // at the total, and past it
            rs.add(i, t + 77, 5);
            if (t > 0) {
                rs.add(i, t - 1, 1);
                rs.add(i, t - 1, 100);
                rs.add(i, t / 2, 0);
                rs.add(i, t / 2, 1);                     // inside one packet
                rs.add(i, t / 2 + 3, 40);
            }
        }
    } else if (flavour == 1) {                           // many ranges of one stream: more output rows than cap
        const int i = (int)g.below(S);
        for (int r = 0; r < 150; r++) rs.add(i, g.below(ix.totals[i] + 50), g.below(3000));
    } else {                                             // random windows over all streams
        const int n = 1 + (int)g.below(40);
        for (int r = 0; r < n; r++) {
            const int i = (int)g.below(S);
            const long long t = ix.totals[i];
            rs.add(i, g.below(t + 200), g.below(4) == 0 ? g.below(t + 2000) : g.below(2500));
        }
    }
    return rs;
}

#define REQUIRE(cond, ...)                                                            \
    do {                                                                              \
        if (!(cond)) {                                                                \
            std::fprintf(stderr, "range_plan_host: %s fails: ", #cond);               \
            std::fprintf(stderr, __VA_ARGS__);                                        \
            std::fprintf(stderr, "\n");                                               \
            return false;                                                             \
        }                                                                             \
    } while (0)

// the last packet before f, in f's stream, that decodes; -1 if none
int last_good_before(const Index &ix, int f)
{
    const int i = ix.stream_of[f];
    for (int j = f - 1; j >= ix.first[i]; j--)
        if (ix.status[j] == 0) return j;
    return -1;
}

long long g_pieces = 0, g_calls = 0, g_failed_before_k = 0, g_cut = 0;

bool check_plan(const Index &ix, const Ranges &rs, int cap)
{
    const int n = (int)rs.ids.size();
    std::vector<int> got((size_t)n, -7);
    vbm_range_plan plan;
    const char *err = vbm_plan_ranges(ix.first.data(), ix.status.data(), ix.out_end.data(), ix.totals.data(), cap, n,
                                      rs.ids.data(), rs.starts.data(), rs.lengths.data(), got.data(), &plan);
    REQUIRE(err == nullptr, "%s on a consistent index (cap %d)", err, cap);
    const std::vector<vbm_range_piece> &pc = plan.pieces;
    // sub-calls partition the pieces in order
    const size_t ncalls = plan.call_first.size() - 1;
    REQUIRE(!plan.call_first.empty() && plan.call_first.front() == 0 && plan.call_first.back() == (int)pc.size(),
            "call_first does not run from 0 to %zu", pc.size());
    for (size_t c = 0; c < ncalls; c++)
        REQUIRE(plan.call_first[c] <= plan.call_first[c + 1], "call_first decreases at %zu", c);
    // per sub-call: the rows fit, and every output row is in 0 .. cap - 1; range_of[p]: the range piece p belongs to
    std::vector<int> range_of(pc.size(), -1);
    for (size_t c = 0; c < ncalls; c++) {
        const int p0 = plan.call_first[c], p1 = plan.call_first[c + 1];
        if (p0 == p1) continue;
        REQUIRE(c < plan.call_r0.size(), "sub-call %zu has pieces and no first range", c);
        int rows = 0;
        for (int p = p0; p < p1; p++) {
            REQUIRE(pc[p].count >= 1 && pc[p].count <= cap - 1, "piece %d has count %d at cap %d", p, pc[p].count, cap);
            REQUIRE(pc[p].r >= 0 && pc[p].r < cap, "piece %d writes output row %d at cap %d", p, pc[p].r, cap);
            rows += pc[p].count + 1;
            range_of[p] = plan.call_r0[c] + pc[p].r;
            REQUIRE(range_of[p] < n, "piece %d belongs to range %d of %d", p, range_of[p], n);
            REQUIRE(p == 0 || range_of[p] >= range_of[p - 1], "piece %d goes back to range %d", p, range_of[p]);
        }
        REQUIRE(rows <= cap, "sub-call %zu has %d rows at cap %d", c, rows, cap);
        g_calls++;
    }
    g_pieces += (long long)pc.size();
    size_t p = 0;
    for (int r = 0; r < n; r++) {
        const int i = rs.ids[r];
        const long long s = rs.starts[r], total = ix.totals[i];
        const long long want = std::max(0LL, std::min(total - s, (long long)rs.lengths[r]));
        REQUIRE(got[r] == want, "range %d (stream %d, start %lld, length %d, total %lld): got %d, not %lld", r, i, s,
                rs.lengths[r], total, got[r], want);
        const size_t pr0 = p;
        while (p < pc.size() && range_of[p] == r) p++;
        if (got[r] == 0) {
            REQUIRE(p == pr0, "range %d has nothing to give and %zu pieces", r, p - pr0);
            continue;
        }
        REQUIRE(p > pr0, "range %d gives %d samples and has no piece", r, got[r]);
        // k: the first packet of the stream whose output goes past s; m: the one that holds sample s + got - 1
        int k = -1, m = -1;
        for (long long j = ix.first[i]; j < ix.first[i + 1]; j++) {
            if (k < 0 && ix.out_end[j] > s) k = (int)j;
            if (m < 0 && ix.out_end[j] > s + got[r] - 1) m = (int)j;
        }
        REQUIRE(k >= 0 && m >= k, "the index of stream %d holds no k .. m for range %d", i, r);
        // the packets after the pre-rolls, concatenated: k .. m, behind the failed packets (they give no samples) that
        // lie between k's pre-roll and k
        int next = pc[pr0].first;
        REQUIRE(next == pc[pr0].pre + 1 && next <= k, "range %d starts at packet %d after pre-roll %d; k is %d", r, next,
                pc[pr0].pre, k);
        for (int j = next; j < k; j++) REQUIRE(ix.status[j] != 0, "range %d decodes good packet %d ahead of k = %d", r, j, k);
        g_failed_before_k += k - next;
        g_cut += (long long)(p - pr0 > 1);
        for (size_t q = pr0; q < p; q++) {
            REQUIRE(pc[q].first == next, "range %d: piece %zu starts at packet %d, not %d", r, q, pc[q].first, next);
            next += pc[q].count;
            const int pre = pc[q].pre;
            REQUIRE(pre >= ix.first[i] && pre < ix.first[i + 1], "range %d: pre-roll %d is outside stream %d", r, pre, i);
            REQUIRE(ix.status[pre] == 0, "range %d: pre-roll %d did not decode", r, pre);
            REQUIRE(pre == last_good_before(ix, pc[q].first), "range %d: pre-roll %d is not the last good packet before %d",
                    r, pre, pc[q].first);
        }
        REQUIRE(next == m + 1, "range %d ends before packet %d, not after m = %d", r, next, m);
    }
    REQUIRE(p == pc.size(), "%zu pieces belong to no range", pc.size() - p);
    return true;
}

// positive out_end and no packet that decodes: no decode gives this index, and the planner must say so
bool check_inconsistent()
{
    const long long first[2] = {0, 3}, out_end[3] = {0, 128, 1152}, totals[1] = {1152}, starts[2] = {0, 200};
    const int status[3] = {-136, -136, -136}, ids[2] = {0, 0}, lengths[2] = {0, 300};
    int got[2] = {-7, -7};
    vbm_range_plan plan;
    const char *err = vbm_plan_ranges(first, status, out_end, totals, 8, 2, ids, starts, lengths, got, &plan);
    REQUIRE(err != nullptr, "an index without a good packet was planned");
    REQUIRE(plan.pieces.empty(), "%zu pieces come with the error", plan.pieces.size());
    return true;
}

}  // namespace

int main()
{
    Rng g{0x9e3779b97f4a7c15ULL};
    const int caps[4] = {2, 3, 7, 64};
    long long plans = 0;
    for (int round = 0; round < 60; round++) {
        const Index ix = make_index(g, 1 + (int)g.below(6));
        for (int flavour = 0; flavour < 3; flavour++) {
            const Ranges rs = make_ranges(g, ix, flavour);
            for (int cap : caps) {
                if (!check_plan(ix, rs, cap)) return 1;
                plans++;
            }
        }
    }
    if (!check_inconsistent()) return 1;
    // the generator reached what the checks are about
    if (g_pieces < 1000 || g_calls < 1000 || g_failed_before_k < 10 || g_cut < 100) {
        std::fprintf(stderr, "range_plan_host: too little was exercised: %lld pieces, %lld sub-calls, %lld failed packets "
                             "ahead of k, %lld cut ranges\n", g_pieces, g_calls, g_failed_before_k, g_cut);
        return 1;
    }
    std::printf("range_plan_host ok: %lld plans, %lld pieces, %lld sub-calls, %lld failed packets ahead of k, %lld cut ranges\n",
                plans, g_pieces, g_calls, g_failed_before_k, g_cut);
    return 0;
}
