/* Host helper of tests/test_psy_small_forms_gpu.py: what the test corpus holds for aoTuV M7, asked of
 * the oracle itself.  orc_noisemask takes the block type as an argument of its own: called for a block with its true type
 * and again as a long block (3: no M7; everything else it does for types 2 and 3 is the same), with the compander level
 * off and no post-echo in both calls, the two logmask rows differ exactly where M7 changed the block's noise row. */
#include "oracle.h"
#include <stdlib.h>

/* out: n, tonefix_end, n25p, n75p, "the mean of lb_loudnoise_fix is formed for this block type" (lib/psy.c:5157-5159) */
void psy_probe_info(const orc_setup *s, int block_mode, int *out)
{
    const orc_psy *p = &s->psy[block_mode];
    out[0] = p->n; out[1] = p->tonefix_end; out[2] = p->n25p; out[3] = p->n75p;
    out[4] = !(p->m_val < 0.5) && !(p->normal_thresh > .45);
}

int psy_probe_m7(const orc_setup *s, int block_mode, const float *logmdct, float *with, float *without)
{
    const orc_psy *p = &s->psy[block_mode];
    const int n = p->n;
    float *epeak = (float *)malloc(n * sizeof(float)), *npeak = (float *)malloc(n * sizeof(float));
    orc_noisemask(s, p, -1.f, logmdct, logmdct, epeak, npeak, with, 0.f, block_mode);
    orc_noisemask(s, p, -1.f, logmdct, logmdct, epeak, npeak, without, 0.f, 3);
    free(epeak); free(npeak);
    return n;
}
