// The host twin's append of the live range store (csrc/live_store.h: vbml_plan_entry, vbml_drop, the moves,
// vbml_walk_entry) as a program of its own, so that it can run under the address and undefined-behaviour sanitizers.
// Every array of the store is allocated at exactly its size, so a write past a region's end is a write past an
// allocation.  Seeded streams of one-byte packet heads with seeded bytes behind them are appended in seeded runs to
// stores that trim by the packet cap and by the byte cap, at full and half rate; after every append the slot must hold
// the matching suffix of the stream's untrimmed index (one walk with vbmd_blockin), with absolute positions and the same bytes, and
// `dropped` must be what a linear restatement of the rule gives.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "live_store.h"

namespace {

uint64_t g_seed = 88172645463325252ull;
uint32_t rnd(uint32_t n)
{
    g_seed ^= g_seed << 13, g_seed ^= g_seed >> 7, g_seed ^= g_seed << 17;
    return (uint32_t)((g_seed >> 11) % n);
}

#define CHECK(x) do { if (!(x)) { printf("live_store_host: line %d: %s\n", __LINE__, #x); exit(1); } } while (0)

const int kBS[2] = {256, 2048};

struct Stream {                       // n packets: a head byte (bit 0: not audio, bit 1: W), then padding
    std::vector<uint8_t> data;
    std::vector<long long> off, gp;
    std::vector<uint8_t> eos, gap;
    std::vector<int> status, W, begin, end;      // the untrimmed index
    std::vector<long long> out_start;
    long long total = 0;
};

template <int HS> Stream make(int n, int most, int invalid_pct, bool marks)
{
    Stream s;
    s.off.push_back(0);
    for (int k = 0; k < n; k++) {
        const int size = 1 + (int)rnd((uint32_t)most);
        const bool bad = (int)rnd(100) < invalid_pct;
        s.data.push_back((uint8_t)((bad ? 1 : 0) | (rnd(2) << 1) | (rnd(4) << 2)));
        for (int i = 1; i < size; i++) s.data.push_back((uint8_t)rnd(256));
        s.off.push_back((long long)s.data.size());
        s.gp.push_back(rnd(5) == 0 ? (long long)rnd(400000) - 3 : -1);
        s.eos.push_back(rnd(10) == 0);
        s.gap.push_back(marks && rnd(12) == 0);
        s.status.push_back(bad ? -135 : 0);
        s.W.push_back(bad ? 0 : (s.data[(size_t)s.off[(size_t)k]] >> 1) & 1);
    }
    // the whole stream walked once, gap marks as k_run_plan applies them
    s.begin.resize((size_t)n), s.end.resize((size_t)n), s.out_start.resize((size_t)n);
    int lW = -1;
    long long sc = -1, gp = -1, at = 0;
    for (int k = 0; k < n; k++) {
        if (s.gap[(size_t)k]) sc = gp = -1;
        long b = 0, e = 0;
        if (s.status[(size_t)k] == 0) {
            vbmd_blockin<HS>(kBS, lW, s.W[(size_t)k], s.gp[(size_t)k], s.eos[(size_t)k], sc, gp, b, e);
            lW = s.W[(size_t)k];
        }
        s.begin[(size_t)k] = (int)b, s.end[(size_t)k] = (int)e, s.out_start[(size_t)k] = at;
        at += e - b;
    }
    s.total = at;
    return s;
}

int drop_rule(const Stream &s, int gone, int a, int np, long long nb, int MP, long long MB)
{
    if (a - gone + np <= MP && s.off[(size_t)a] - s.off[(size_t)gone] + nb <= MB) return 0;
    const int keep_p = MP / 2 < MP - np ? MP / 2 : MP - np;
    const long long keep_b = MB / 2 < MB - nb ? MB / 2 : MB - nb;
    int d = 0;
    while (a - gone - d > keep_p || s.off[(size_t)a] - s.off[(size_t)(gone + d)] > keep_b) d++;
    return d;
}

template <int HS> void run(int MP, long long MB, int most, int invalid_pct, bool marks, long long *trims)
{
    const int S = 3, sid = 1, n = 600;                    // the slot in the middle: both neighbours must stay untouched
    const Stream s = make<HS>(n, most, invalid_pct, marks);
    const long long stride = (MB + 15) & ~15LL;
    const size_t slots = (size_t)S * ((size_t)MP + 1);
    std::vector<vbml_slot> st((size_t)S, vbml_fresh(0));
    std::vector<uint8_t> data((size_t)(S * stride), 0xee);
    std::vector<long long> offsets(slots, -7), out_start(slots, -7);
    std::vector<int> status(slots, -7), begin(slots, -7), end(slots, -7);
    for (int i = 0; i < S; i++) offsets[(size_t)i * ((size_t)MP + 1)] = i * stride;
    const vbml_arrays A = {MP, MB, stride, st.data(), data.data(), offsets.data(), out_start.data(), status.data(),
                           begin.data(), end.data()};
    const long long P0 = (long long)sid * (MP + 1);
    int a = 0, gone = 0;
    while (a < n) {
        int c = (int)rnd((uint32_t)(MP < 12 ? MP : 12) + 3);        // now and then above a cap
        if (c > n - a) c = n - a;
        const long long nb = s.off[(size_t)(a + c)] - s.off[(size_t)a];
        // the run alone, at exactly its size, under offsets that do not start at 0
        std::vector<uint8_t> src(s.data.begin() + s.off[(size_t)a], s.data.begin() + s.off[(size_t)(a + c)]);
        std::vector<long long> so((size_t)c + 1);
        for (int k = 0; k <= c; k++) so[(size_t)k] = s.off[(size_t)(a + k)] - s.off[(size_t)a];
        std::vector<int> hst((size_t)c), hW((size_t)c), pks((size_t)c);
        std::vector<long long> pke((size_t)c);
        for (int k = 0; k < c; k++) hst[(size_t)k] = s.status[(size_t)(a + k)], hW[(size_t)k] = s.W[(size_t)(a + k)];
        vbml_back back;
        vbml_host_append_entry<HS>(A, kBS, sid, 0, c, src.data(), so.data(), nb, hst.data(), hW.data(),
                                   s.gp.data() + a, s.eos.data() + a, s.gap.data() + a, pks.data(), pke.data(), back);
        if (c > MP || nb > MB) {
            CHECK(back.status == VBM_LIVE_EBIG && back.dropped == 0 && back.retained == a - gone);
            CHECK(st[(size_t)sid].count == a - gone);
            continue;                                      // refused and untouched: another run goes in next
        }
        const int d = drop_rule(s, gone, a, c, nb, MP, MB);
        CHECK(back.status == 0 && back.dropped == d && back.retained == a + c - gone - d);
        trims[0] += back.by & 1, trims[1] += (back.by >> 1) & 1;
        gone += d, a += c;
        CHECK(st[(size_t)sid].count == a - gone && back.total == (a < n ? s.out_start[(size_t)a] : s.total));
        CHECK(back.bytes == s.off[(size_t)a] - s.off[(size_t)gone] && back.bytes <= MB && a - gone <= MP);
        long long lo = back.total;
        for (int k = a - 1; k >= gone; k--)
            if (s.status[(size_t)k] == 0) lo = s.out_start[(size_t)k] + s.end[(size_t)k] - s.begin[(size_t)k];
        CHECK(back.first_sample == lo);
        for (int k = gone; k < a; k++) {
            const size_t j = (size_t)(P0 + k - gone), q = (size_t)k;
            CHECK(status[j] == s.status[q] && begin[j] == s.begin[q] && end[j] == s.end[q] && out_start[j] == s.out_start[q]);
            CHECK(offsets[j + 1] - offsets[j] == s.off[q + 1] - s.off[q]);
            if (k >= a - c) CHECK(pks[(size_t)(k - (a - c))] == s.status[q] && pke[(size_t)(k - (a - c))] == s.out_start[q] + s.end[q] - s.begin[q]);
        }
        CHECK(offsets[(size_t)P0] == sid * stride);
        for (long long i = 0; i < back.bytes; i++) CHECK(data[(size_t)(sid * stride + i)] == s.data[(size_t)(s.off[(size_t)gone] + i)]);
    }
    for (int i = 0; i < S; i += 2) {                       // the neighbours: as they were made
        CHECK(st[(size_t)i].count == 0 && offsets[(size_t)i * ((size_t)MP + 1)] == i * stride);
        for (long long b = 0; b < stride; b++) CHECK(data[(size_t)(i * stride + b)] == 0xee);
        for (int k = 0; k < MP; k++) CHECK(status[(size_t)i * ((size_t)MP + 1) + (size_t)k] == -7);
    }
}

}  // namespace

int main()
{
    long long by_packets[2] = {0, 0}, by_bytes[2] = {0, 0};
    for (int marks = 0; marks < 2; marks++)
        for (int invalid = 0; invalid <= 90; invalid += 45) {
            run<0>(8, 1 << 20, 1, invalid, marks != 0, by_packets);          // one-byte packets: the packet cap alone
            run<1>(9, 1 << 20, 30, invalid, marks != 0, by_packets);
            run<0>(1000, 200, 40, invalid, marks != 0, by_bytes);            // the byte cap alone
            run<1>(1000, 333, 40, invalid, marks != 0, by_bytes);
            run<0>(16, 400, 40, invalid, marks != 0, by_bytes);              // either
        }
    CHECK(by_packets[0] > 0 && by_packets[1] == 0 && by_bytes[1] > 0);
    printf("live_store_host ok: %lld trims by the packet cap, %lld by the byte cap\n", by_packets[0] + by_bytes[0],
           by_bytes[1]);
    return 0;
}
