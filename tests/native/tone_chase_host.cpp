// Host harness of tests/test_tone_chase_cpu.py: the chase phase of k_tonemask (csrc/tone_chase.h, the text the kernel
// compiles: the closed-form step, and chase_run driven chunk by chunk the way the kernel's lanes run it) beside a serial
// restatement of seed_chase's stack walk (reference lib/psy.c:851-881), for a comparison of the surviving lines.
// Seeds are ints here: the walk only ever compares them.
//
// With -DTONE_CHASE_MAIN the file is a stand-alone program (random rows of every kind through both forms), for a
// run under the host sanitizers.
#include <stdint.h>
#include <string.h>
#include <vector>
#include "tone_chase.h"

#define LINESPER 8          /* eighth_octave_lines of every shipped setup */
#define CHUNK 64
#define MAXCHUNKS 16

// ---- serial: the source's walk with its explicit stack; alive[i] = line i is on the stack at the end
static void serial_walk(const int n, const int *seed, unsigned char *alive)
{
    std::vector<int> pos(n + 1), amp(n + 1);
    int depth = 0;
    for (int i = 0; i < n; i++) {
        while (depth >= 2) {
            if (seed[i] < amp[depth - 1]) break;                            // below the top: just push
            if (!(i < pos[depth - 1] + LINESPER)) break;                    // the top is out of reach
            if (!(amp[depth - 1] <= amp[depth - 2] && i < pos[depth - 2] + LINESPER)) break;
            depth--;                                                        // the top is overlapped completely
        }
        pos[depth] = i;
        amp[depth++] = seed[i];
    }
    memset(alive, 0, n);
    for (int k = 0; k < depth; k++) alive[pos[k]] = 1;
}

// ---- the kernel's compare phase: gl[j] = GE | LE << 8 (GE bit k-1 = !(s[j] < s[j-k]), LE bit d-1 = (s[j] <= s[j-d]))
// in a row that is 8-byte aligned and readable past its end like the kernel's LDS row
struct gl_row {
    std::vector<unsigned long long> store;
    unsigned short *gl;
    gl_row(const int n, const int *s) : store(((n + 8) & ~7) / 4 + 1, 0ull), gl((unsigned short *)store.data())
    {
        for (int j = 0; j < n; j++) {
            unsigned ge = 0, le = 0;
            for (int k = 1; k <= 7; k++) {
                if (j - k < 0) continue;
                if (!(s[j] < s[j - k])) ge |= 1u << (k - 1);
                if (k <= 6 && s[j] <= s[j - k]) le |= 1u << (k - 1);
            }
            gl[j] = (unsigned short)(ge | (le << 8));
        }
    }
};

// ---- the step alone, line after line from the empty stack.  Returns how often L was no subset of m.
static int step_walk(const int n, const unsigned short *gl, unsigned char *alive)
{
    unsigned m = 0, L = 0;
    int loose = 0;
    memset(alive, 0, n);
    for (int i = 0; i < n; i++) {
        const unsigned mp = tone_chase_step(m, L, gl[i] & 0xffu, gl[i] >> 8);
        if (i >= 7) alive[i - 7] = (mp >> 6) & 1u;
        if ((L & 0x7fu) & ~m) loose++;
    }
    for (int b = 0; b < 7; b++)
        if (n - 1 - b >= 0) alive[n - 1 - b] = (m >> b) & 1u;
    return loose;
}

// ---- the chunked walk as the kernel's chase phase runs it: every chunk at once from (0, 0) at own - runin, then
// rounds of check-against-the-left-neighbour and re-run until no chunk disagrees, then the left7 hand-over.
// stats[0] += chunks, [1] += chunks that ran again at least once, [2] += re-runs, [3] += rounds
static void chunked_walk(const int n, const unsigned short *gl, const int runin, unsigned char *alive, long long *stats)
{
    const int nch = (n + CHUNK - 1) / CHUNK;
    unsigned long long al[MAXCHUNKS];
    unsigned m_own[MAXCHUNKS], L_own[MAXCHUNKS], m_next[MAXCHUNKS], L_next[MAXCHUNKS], used[MAXCHUNKS], left7[MAXCHUNKS];
    int oend[MAXCHUNKS], again[MAXCHUNKS];
    bool last[MAXCHUNKS];
    for (int c = 0; c < nch; c++) {
        const int own = c * CHUNK;
        oend[c] = own + CHUNK - 1 < n - 1 ? own + CHUNK - 1 : n - 1;
        last[c] = own + CHUNK >= n;
        again[c] = 0;
        const int i0 = own >= runin ? own - runin : 0;
        chase_run(gl, i0, 0u, 0u, own, oend[c], last[c], al[c], left7[c], m_own[c], L_own[c], m_next[c], L_next[c]);
        used[c] = m_own[c] | ((L_own[c] & m_own[c]) << 8);
    }
    for (;;) {
        unsigned truth[MAXCHUNKS];
        bool any = false;
        for (int c = 1; c < nch; c++) {                         // (one shuffle: every lane reads before any re-runs)
            truth[c] = m_next[c - 1] | ((L_next[c - 1] & m_next[c - 1]) << 8);
            any |= truth[c] != used[c];
        }
        if (!any) break;
        stats[3]++;
        for (int c = 1; c < nch; c++) {
            if (truth[c] == used[c]) continue;
            chase_run(gl, c * CHUNK, truth[c] & 0x7fu, truth[c] >> 8, c * CHUNK, oend[c], last[c], al[c], left7[c], m_own[c],
                      L_own[c], m_next[c], L_next[c]);
            used[c] = truth[c];
            again[c]++;
        }
    }
    memset(alive, 0, n);
    for (int c = 0; c < nch; c++) {
        unsigned long long w = al[c];
        if (!last[c]) w |= (unsigned long long)left7[c + 1] << 57;
        for (int t = 0; t < CHUNK && c * CHUNK + t < n; t++) alive[c * CHUNK + t] = (w >> t) & 1ull;
        stats[0]++;
        stats[1] += again[c] > 0;
        stats[2] += again[c];
    }
}

// Rows `seeds` [nrows][pitch], row r of len[r] lines.  mode 0: the step alone, 1: the chunked walk.  Returns the first
// row whose survivors differ from the serial walk's (-1: none); stats as above, stats[4] += L bits outside m (mode 0).
extern "C" int tone_chase_rows(int nrows, int pitch, const int *len, const int *seeds, int mode, int runin, long long *stats)
{
    std::vector<unsigned char> want(pitch + 1), got(pitch + 1);
    for (int r = 0; r < nrows; r++) {
        const int n = len[r];
        const int *s = seeds + (size_t)r * pitch;
        serial_walk(n, s, want.data());
        gl_row row(n, s);
        if (mode == 0) stats[4] += step_walk(n, row.gl, got.data());
        else chunked_walk(n, row.gl, runin, got.data(), stats);
        if (memcmp(want.data(), got.data(), n)) return r;
    }
    return -1;
}

#ifdef TONE_CHASE_MAIN
#include <stdio.h>
int main()
{
    uint32_t x = 12345u;
    auto rnd = [&x]() { x = x * 1664525u + 1013904223u; return x >> 8; };
    long long stats[5] = {0, 0, 0, 0, 0};
    for (int r = 0; r < 4000; r++) {
        const int n = 2 + (int)(rnd() % 900), kind = r % 5;
        std::vector<int> s(n);
        for (int i = 0; i < n; i++)
            s[i] = kind == 0 ? 7 : kind == 1 ? (i / 3) % 2 : kind == 2 ? (int)(rnd() % 3) : kind == 3 ? i : (int)(rnd() % 100000);
        for (int mode = 0; mode < 2; mode++)
            if (tone_chase_rows(1, n, &n, s.data(), mode, 16, stats) >= 0) {
                printf("row %d (n %d, kind %d, mode %d) differs\n", r, n, kind, mode);
                return 1;
            }
    }
    printf("ok: %lld chunks, %lld ran again, %lld loose L bits\n", stats[0], stats[1], stats[4]);
    return stats[4] != 0;
}
#endif
