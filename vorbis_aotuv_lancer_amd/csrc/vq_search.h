// The residue VQ search of one vector, local_book_besterror (reference lib/res0.c:316-378), as k_res_vq
// (pack_kernels.hip) runs it per lane.  A header of its own so that the same text also compiles for the host:
// tests/test_vq_search_cpu.py drives it over every shipped residue book against the oracle, including the two
// paths that no audio input was found to reach (a lattice point without a codeword, a numerator >= 2^23).
#pragma once
#include <stdint.h>
#include <stdlib.h>
#include "setup.h"

#ifdef __HIPCC__
#define VQ_FN __device__ __forceinline__
#else
#define VQ_FN static inline
#endif

struct alignas(16) vq_u4 { uint32_t x, y, z, w; };

// two 16-bit products accumulated in 32 bits (v_dot2_i32_i16)
VQ_FN int vq_dot2(uint32_t a, uint32_t b, int acc)
{
#ifdef __HIPCC__
    typedef short short2v __attribute__((ext_vector_type(2)));
    return __builtin_amdgcn_sdot2(__builtin_bit_cast(short2v, a), __builtin_bit_cast(short2v, b), acc, false);
#else
    return acc + (int)(int16_t)(a & 0xffffu) * (int)(int16_t)(b & 0xffffu) + (int)(int16_t)(a >> 16) * (int)(int16_t)(b >> 16);
#endif
}

// the fields of a book the lattice step reads per vector, fetched once per (partition, stage): the book
// is addressed per lane, and the compiler cannot hoist its loads over the stores of the search loop.
// What only the exhaustive search needs (used, used_*) stays behind `book` and is fetched there.
struct book_regs {
    int dim, minval, delta, quantvals;
    const signed char *lengthlist;
    const uint32_t *codelist;
    const vbm_book *book;
};
VQ_FN book_regs load_book(const vbm_book *book)
{
    book_regs r;
    r.dim = book->dim; r.minval = book->minval; r.delta = book->delta; r.quantvals = book->quantvals;
    r.lengthlist = book->lengthlist; r.codelist = book->codelist;
    r.book = book;
    return r;
}

// One statement per element of a vector, element numbers as literals: the vector and its remainder live in VGPRs, and
// a register array indexed by a run-time number costs an 8-way compare-select chain per access.  dim is per lane
// (lanes are different stream-blocks with their own classes and books); the outer tests let a wavefront whose books
// are all short skip the upper elements in one branch.
#define VQ_EACH_DOWN(dim, X) do {                                                             \
        if ((dim) > 4) { if ((dim) > 7) { X(7) } if ((dim) > 6) { X(6) } if ((dim) > 5) { X(5) } X(4) }   \
        if ((dim) > 2) { if ((dim) > 3) { X(3) } X(2) }                                         \
        if ((dim) > 1) { X(1) }                                                                 \
        X(0)                                                                                    \
    } while (0)

// local_book_besterror (lib/res0.c:316-378) of the vector src[0], src[64], ... (dim <= 8 samples of this lane in
// the LDS stage) in two parts: the second one is rare and needs tables the first does not.
//
// Part 1, the lattice step (:322-340), elements dim-1 down to 0 as in the source: returns the lattice point's
// entry, leaves the vector in a[] (0 past dim) and puts the remainder after that point into the stage (it is what
// the next stage reads in the common case, so p[] of the source never exists as an array).
// num / del truncates toward zero as C does: below 2^23 the correctly rounded float quotient cannot reach the next
// integer (it is at least 1/del away, the rounding error is below |num| / del * 2^-24), so its truncation is the
// integer quotient, ~10 instructions instead of ~40.  A vector with a wider numerator is done again with the
// integer division, out of line, from the samples the stage still holds.
VQ_FN int vq_lattice(const book_regs *book, int *src, int *a)
{
    const int dim = book->dim;
    const int minval = book->minval, del = book->delta, qv = book->quantvals;
    const int ze = (qv >> 1);
    const int half = (del != 1) ? (del >> 1) : 0;
    const float fdel = (float)del;
    int index = 0;
    int rem[VBM_MAX_BOOK_DIM];
    bool wide = false;

#define VQ_LOAD(k) a[k] = src[(k) * 64];
    VQ_EACH_DOWN(dim, VQ_LOAD);
#undef VQ_LOAD
#define VQ_STEP(k) {                                                                          \
        const int num = a[k] - minval + half;                                                  \
        int v = num;                                                                           \
        if (del != 1) {                                                                        \
            v = (int)((float)num / fdel);                                                      \
            wide = wide || (abs(num) >= (1 << 23));                                            \
        }                                                                                      \
        const int m = (v < ze ? ((ze - v) << 1) - 1 : ((v - ze) << 1));                        \
        index = index * qv + (m < 0 ? 0 : (m >= qv ? qv - 1 : m));                             \
        rem[k] = a[k] - (v * del + minval);                                                    \
    }
    VQ_EACH_DOWN(dim, VQ_STEP);
#undef VQ_STEP
    if (__builtin_expect(wide, 0)) {
        index = 0;
        for (int o = dim - 1; o >= 0; o--) {
            const int x = src[o * 64];
            const int v = (x - minval + half) / del;
            const int m = (v < ze ? ((ze - v) << 1) - 1 : ((v - ze) << 1));
            index = index * qv + (m < 0 ? 0 : (m >= qv ? qv - 1 : m));
            src[o * 64] = x - (v * del + minval);
        }
    } else {
#define VQ_STORE(k) src[(k) * 64] = rem[k];
        VQ_EACH_DOWN(dim, VQ_STORE);
#undef VQ_STORE
    }
    return index;       // < quantvals^dim <= entries
}

// Part 2, only when the lattice point has no codeword: the exhaustive search over the entries that have one,
// first minimum wins (lib/res0.c:343-370).  |pt - a|^2 = |pt|^2 - 2 pt.a + |a|^2: the last term is common, so
// entries are compared by |pt|^2 - 2 pt.a (same order, same ties); pt.a as packed 16-bit dot products, one 16-byte
// load per entry.  Only the winner's index is tracked; its point is fetched afterwards and the stage gets the
// remainder after it.  Returns the winner's codeword length (0: the book has no used entry, and the source then
// keeps the lattice point's remainder and writes no bits).
VQ_FN int vq_exhaustive(const book_regs *book, int *src, const int *a, uint32_t &code)
{
    const vbm_book *bk = book->book;
    const int dim = book->dim;
    const int used = bk->used;
    if (used <= 0) return 0;
    int i, bi = 0;
    bool small = bk->used_pack != nullptr;
#pragma unroll
    for (int k = 0; k < VBM_MAX_BOOK_DIM; k++) small = small && (a[k] >= -32768 && a[k] <= 32767);
    if (small) {
        uint32_t pa[4];      // (a[k] is 0 for k >= dim, as the packed points are)
#pragma unroll
        for (int k = 0; k < 4; k++) pa[k] = ((uint32_t)a[2 * k] & 0xffffu) | ((uint32_t)a[2 * k + 1] << 16);
        const vq_u4 *pk = reinterpret_cast<const vq_u4 *>(bk->used_pack);
        const int *nrm = bk->used_norm;
        const int words = (dim + 1) >> 1;
        int best = 0;
        for (i = 0; i < used; i++) {
            const vq_u4 v = pk[i];
            int dot = vq_dot2(v.x, pa[0], 0);
            if (words > 1) dot = vq_dot2(v.y, pa[1], dot);
            if (words > 2) {
                dot = vq_dot2(v.z, pa[2], dot);
                dot = vq_dot2(v.w, pa[3], dot);
            }
            const int score = nrm[i] - 2 * dot;
            if (i == 0 || score < best) { best = score; bi = i; }
        }
    } else {
        int best = -1;
        const int *pt = bk->used_point;
        for (i = 0; i < used; i++, pt += dim) {
            int dist = 0;
#define VQ_DIST(k) { const int val = pt[k] - a[k]; dist += val * val; }
            VQ_EACH_DOWN(dim, VQ_DIST);      // (an integer sum: its order is free)
#undef VQ_DIST
            if (best == -1 || dist < best) { best = dist; bi = i; }
        }
    }
    const int *pt = bk->used_point + (size_t)bi * dim;
#define VQ_STORE(k) src[(k) * 64] = a[k] - pt[k];
    VQ_EACH_DOWN(dim, VQ_STORE);
#undef VQ_STORE
    const int index = bk->used_index[bi];
    if (index < 0 || index >= bk->entries) return 0;
    code = bk->codelist[index];
    return bk->lengthlist[index];
}

// _encodepart (lib/res0.c:384-404) of one partition with one book: spp samples of this lane in the stage
// ([sample][64 lanes]), codeword t (code | length << 32, 0: none) to sl[t * 64]; returns the bits.
// The codeword is asked for beside the length: in the common case the lattice point has one, and the two gathers
// are then in flight together instead of one after the other.
VQ_FN int vq_encode_partition(const book_regs *book, int *stage, const int spp, uint64_t *sl)
{
    const int dim = book->dim;
    const int step = spp / dim;
    int bits = 0;
    for (int t = 0; t < step; t++) {
        int a[VBM_MAX_BOOK_DIM] = {0, 0, 0, 0, 0, 0, 0, 0};
        int *src = stage + t * dim * 64;
        const int index = vq_lattice(book, src, a);
        int len = book->lengthlist[index];
        uint32_t code = book->codelist[index];
        if (__builtin_expect(len <= 0, 0)) len = vq_exhaustive(book, src, a, code);
        uint64_t cw = 0;
        if (len > 0) {
            cw = (uint64_t)code | ((uint64_t)(uint32_t)len << 32);
            bits += len;
        }
        sl[(size_t)t * 64] = cw;
    }
    return bits;
}

#undef VQ_EACH_DOWN
