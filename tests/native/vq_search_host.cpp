// Host harness of tests/test_vq_search_cpu.py: the product's residue VQ search (csrc/vq_search.h, the text the
// kernel compiles) on one partition with one book, for the comparison with the oracle's orc_book_besterror.
#include "vq_search.h"

// vec: spp samples in, the remainder out; cw: spp / dim codewords (code | length << 32) out; returns the bits
extern "C" int vq_search_host(int dim, int entries, int quantvals, int minval, int delta, const signed char *lengthlist,
                              const uint32_t *codelist, int used, const int *used_index, const int *used_point,
                              const short *used_pack, const int *used_norm, int spp, int *vec, uint64_t *cw)
{
    vbm_book b = {};
    b.dim = dim; b.entries = entries; b.quantvals = quantvals; b.minval = minval; b.delta = delta;
    b.lengthlist = lengthlist; b.codelist = codelist;
    b.used = used; b.used_index = used_index; b.used_point = used_point; b.used_pack = used_pack; b.used_norm = used_norm;
    if (spp < 1 || spp > 64 || dim < 1 || dim > VBM_MAX_BOOK_DIM) return -1;
    static int stage[64 * 64];                        // the kernel's LDS stage: [sample][64 lanes], this is lane 0
    static uint64_t slots[64 * 64];
    for (int k = 0; k < spp; k++) stage[k * 64] = vec[k];
    const book_regs r = load_book(&b);
    const int bits = vq_encode_partition(&r, stage, spp, slots);
    for (int k = 0; k < spp; k++) vec[k] = stage[k * 64];
    for (int t = 0; t < spp / dim; t++) cw[t] = slots[t * 64];
    return bits;
}
