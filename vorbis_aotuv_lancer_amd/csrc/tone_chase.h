// seed_chase's stack walk (reference lib/psy.c:851-881) as k_tonemask (tone_kernels.hip) runs it: a two-mask machine
// with a closed-form step per seed line.  A header of its own so that the same text also compiles for the host:
// tests/test_tone_chase_cpu.py drives it against a serial restatement of the source's walk, survivor set for survivor set.
//
// The walk pushes every line and first pops while (a) the new seed is not below the top of the stack, (b) the top
// is not above the entry below it, and both lie within eighth_octave_lines (8) of the new line.  Only lines less
// than 8 back can be popped, so the state is a window of 7 lines:
//   m  bit b: line i-1-b is on the stack
//   L  bit b: that entry is <= the entry below it on the stack (its seed compared with the next older survivor's)
// (b) compares two stack entries, and the stack is LIFO: the entry below a given entry never changes while that entry
// is on the stack.  So the bit is known when the upper entry is pushed (l below: the LE bit of the new line at the
// distance of the top that stays), and a line's whole pop sequence is a prefix operation on the two masks: the entries
// the new seed may pop are P = GE & L, the first entry that stays is the youngest one outside P, or the oldest of the
// window whatever its bits say (the entry below that one is out of reach: the source's second distance test), and
// every younger entry goes.  No loop and no branch.  L is always a subset of m; of L only bits 0..6 mean anything.
#pragma once

#ifdef __HIPCC__
#define TONE_CHASE_FN __host__ __device__ __forceinline__
#else
#define TONE_CHASE_FN static inline
#endif

// the highest set bit of a 7-bit mask (0 for 0).  The count is taken of m << 1 | 1, which is never 0: for m == 0 the
// shift is by 31.  On gfx950: v_lshl_or_b32, v_ffbh_u32, v_lshrrev_b32 of a constant (a count that may meet 0 costs a
// v_min_u32 against 32 more, and the AND with m that hides the wrong bit).
TONE_CHASE_FN unsigned tone_chase_msb7(const unsigned m) { return 0x40000000u >> __builtin_clz((m << 1) | 1u); }

// One line of the walk.  ge: GE bits of the line (bit k-1 = !(s[i] < s[i-k]), k = 1..7), le: its LE bits (bit d-1 =
// (s[i] <= s[i-d]), d = 1..6; bits 6 and up are 0).  Returns the window mask before the line itself is pushed: its
// bit 6 is the final fate of line i-7.  m and L become the state at line i+1 (m within 7 bits; L may carry a stray
// bit 7, which the next step's AND with m drops).
TONE_CHASE_FN unsigned tone_chase_step(unsigned &m, unsigned &L, const unsigned ge, const unsigned le)
{
    const unsigned P = ge & L;                              // entries the new seed may pop
    const unsigned t = m & ~P;                              // the youngest of these is the first entry that stays; if there is
    const unsigned mp = (m & (t | (0u - t))) | tone_chase_msb7(m);  // none, the oldest in reach.  Every younger one is popped
                                                            // (t | -t: the bits from t's lowest up, 0 for 0; the oldest lies there too)
    const unsigned k0 = (unsigned)__builtin_ctz(mp | 0x40u);    // the new line's entry below, at distance k0 + 1
    const unsigned l = (le >> k0) & 1u;                     // (0 at distance 7 and for an empty window: le has no bit 6)
    L = ((L & mp) << 1) | l;
    m = ((mp << 1) | 1u) & 0x7fu;
    return mp;
}

// One chase lane: run-in lines [i, own), then its own lines [own, oend], starting with the state (m, L) at line i.
// gl[j] = GE | LE << 8 of line j.  i and own are multiples of 4 (four lines per 8-byte read; the row is readable up
// to the next multiple of 4 past oend).
//   m_own, L_own / m_next, L_next  the state at the start of lines own and oend + 1 (L within 7 bits)
//   alive           final fate of the own lines the walk itself sees leave the window: own .. oend - 7, and for the
//                   last chunk of a row (`last`) also the lines it ended on top of
//   left7           bit t: final fate of line own - 7 + t, the left neighbour's last seven lines.  They sit in this
//                   walk's mask at its first line and leave the window in its first seven steps, so once the state at
//                   own has been checked against the neighbour's at its oend + 1 they are the truth and the neighbour
//                   need not walk on past its chunk to learn them.
// The run-in loop only carries the state; the own loop collects bit 6 of every step into F (bit t: line own + t - 7),
// a nibble per read: alive = F >> 7, left7 = F & 0x7f.
TONE_CHASE_FN void chase_run(const unsigned short *__restrict__ gl, int i, unsigned m, unsigned L, const int own, const int oend,
                             const bool last, unsigned long long &alive, unsigned &left7, unsigned &m_own, unsigned &L_own,
                             unsigned &m_next, unsigned &L_next)
{
    for (; i < own; i += 4) {
        const unsigned long long g4 = *(const unsigned long long *)(gl + i);
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const unsigned g = (unsigned)(g4 >> (16 * u)) & 0xffffu;
            (void)tone_chase_step(m, L, g & 0xffu, g >> 8);
        }
    }
    m_own = m;
    L_own = L & 0x7fu;
    unsigned long long F = 0;
    for (; i + 3 <= oend; i += 4) {
        const unsigned long long g4 = *(const unsigned long long *)(gl + i);
        unsigned nb = 0;
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const unsigned g = (unsigned)(g4 >> (16 * u)) & 0xffffu;
            const unsigned mp = tone_chase_step(m, L, g & 0xffu, g >> 8);
            nb |= ((mp >> 6) & 1u) << u;
        }
        F |= (unsigned long long)nb << (i - own);
    }
    if (i <= oend) {                        // the last chunk's one to three lines past a multiple of four
        const unsigned long long g4 = *(const unsigned long long *)(gl + i);
        unsigned nb = 0;
#pragma unroll
        for (int u = 0; u < 3; u++) {
            if (i + u <= oend) {
                const unsigned g = (unsigned)(g4 >> (16 * u)) & 0xffffu;
                const unsigned mp = tone_chase_step(m, L, g & 0xffu, g >> 8);
                nb |= ((mp >> 6) & 1u) << u;
            }
        }
        F |= (unsigned long long)nb << (i - own);
    }
    m_next = m;
    L_next = L & 0x7fu;
    alive = F >> 7;
    left7 = (unsigned)F & 0x7fu;
    if (last) {
#pragma unroll
        for (int b = 0; b < 7; b++) {       // lines the walk ended on top of (a chunk of fewer than seven lines: the
            const int q = oend - b - own;   // left neighbour's too)
            const unsigned bit = (m >> b) & 1u;
            if (q >= 0) alive |= (unsigned long long)bit << q;
            else left7 |= bit << (q + 7);
        }
    }
}
