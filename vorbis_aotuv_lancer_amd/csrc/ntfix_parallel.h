// aoTuV M7 (ntfix, reference lib/psy.c:3645-3768) cut into per-bin and per-group bodies, as k_noisemask
// (noise_kernels.hip) runs them with every thread of the workgroup.  A header of its own so that the same text also compiles for the host: tests/test_ntfix_parallel_cpu.py drives it against a
// serial restatement of the source, bit for bit.
//
// Short blocks (block_mode <= 1).  The source walks i over [4, nx), tests spectral[i] against both neighbours, and
// after a peak jumps to its upper edge pe.  The jump never skips a peak: bin i + 1 is below bin i, and pe only
// advances over bins j with spectral[j] <= spectral[j - 1], so none of i + 1 .. pe passes the strict test
// spectral[j] > spectral[j - 1].  The peaks are therefore exactly the bins that pass the test, and a peak's ps, pe and ss
// are functions of spectral, inmod and noise[i] within +-3 bins.  temp[j] is the largest ss of the peaks whose
// [ps, pe] holds j, or 0: every ss that is stamped is > 0 (it is above the tolerance, or (ss - tolerance) * .6 of
// such a one), so the source's clamp at 0 never acts and the maximum does not depend on the order of the peaks.
//   ntfix_short_peak   a thread per bin: ss and the reach of the peak at that bin (0: none)
//   ntfix_short_temp   a thread per bin: the maximum over the at most seven peaks that can reach it
//
// Transition blocks (block_mode == 2).  The 8-bin means are independent double sums in bin order; all of them are
// formed before any subtraction.  The peak test reads the means only, so the peaks are independent as well.  The
// subtractions noise[j] -= thres are NOT free in order (float): the source makes them peak after peak, and the ranges
// [8 a, 8 (i + 3)] (a = i - 3 or i - 2) of peaks up to six groups apart overlap.  Bin j therefore pulls: it walks its
// seven candidate groups j / 8 - 3 .. j / 8 + 3 in ascending order and subtracts the thres of each peak whose range
// holds it: the same float sequence per bin.
//   ntfix_group_mean, ntfix_group_peak, ntfix_trans_pull
#pragma once

#ifdef __HIPCC__
#define NTFIX_FN __host__ __device__ __forceinline__
#else
#define NTFIX_FN static inline
#endif

#define NTFIX_MIN(x, y) ((x) > (y) ? (y) : (x))
#define NTFIX_MAX(x, y) ((x) < (y) ? (y) : (x))
#define NTFIX_FREQ_UPC 3
#define NTFIX_FREQ_UNC 4

// lib/psy.c:3680-3684; bins from nxplus on keep the cleared 0
NTFIX_FN float ntfix_inmod(const float sp, const int i, const int nxplus)
{
    if (i >= nxplus) return 0.f;
    if (sp < -70) return (float)(-70 + (double)(sp + 70) * .1);
    return sp;
}

NTFIX_FN float ntfix_short_tolerance(const int n) { return n == 256 ? 15.f : 9.f; }

// bin i of [4, nx): 0 if it is no peak or its ss stays within the tolerance, else the ss the source stamps on
// [i - *down, i + *up] (lib/psy.c:3686-3716).  spectral and inmod are read at i - 3 .. i + 3.
NTFIX_FN float ntfix_short_peak(const float *spectral, const float *inmod, const float noise_i, const int i, const float tolerance,
                                int *down, int *up)
{
    *down = 0; *up = 0;
    if (!((spectral[i] > spectral[i - 1]) && (spectral[i] > spectral[i + 1]))) return 0.f;
    int ps = i - 1, pe = i + 1, j;
    const int upper = i - NTFIX_FREQ_UPC, under = i + NTFIX_FREQ_UNC;
    for (j = ps; j > upper; j--) {
        if (spectral[j + 1] < spectral[j]) break;
        ps = j;
    }
    for (j = pe; j < under; j++) {
        if (spectral[j - 1] < spectral[j]) break;
        pe = j;
    }
    float ss = inmod[i] - inmod[ps];
    ss = NTFIX_MAX(ss, inmod[i] - inmod[pe]);
    if (!(ss > tolerance)) return 0.f;
    if (spectral[i] > noise_i) {
        ss -= tolerance;
        ss *= .6f;
    }
    *down = i - ps; *up = pe - i;
    return ss;
}

// one word per bin for the pull: the reach of the bin's peak, down in bits 0-3, up in bits 4-7
NTFIX_FN int ntfix_reach_pack(const int down, const int up) { return down | (up << 4); }

// temp[j] as the source leaves it before the clamp at `test`: peak_ss / reach as ntfix_short_peak left them for the
// bins of [4, nx) (lib/psy.c:3710-3713 over all peaks)
NTFIX_FN float ntfix_short_temp(const float *peak_ss, const int *reach, const int j, const int nx)
{
    float t = 0.f;
    const int lo = NTFIX_MAX(j - 3, NTFIX_FREQ_UNC), hi = NTFIX_MIN(j + 3, nx - 1);
    for (int q = lo; q <= hi; q++) {
        const float ss = peak_ss[q];
        if (!(ss > 0.f)) continue;
        const int rc = reach[q];
        if (j >= q - (rc & 15) && j <= q + (rc >> 4)) t = NTFIX_MAX(ss, t);
    }
    return t;
}

// lib/psy.c:3719-3723, bins [3, nx)
NTFIX_FN float ntfix_short_apply(const float noise_i, float temp, const float tone_off, const float noise_off, const float limit)
{
    const float test = NTFIX_MIN(tone_off, noise_off + limit);
    if (temp > test) temp = test;
    return noise_i - temp;
}

// lib/psy.c:3726-3731: group k of eight bins (noise points at the group's first bin)
NTFIX_FN float ntfix_group_mean(const float *noise)
{
    double na = 0;
    for (int j = 0; j < 8; j++) na += noise[j];
    na /= 8;
    return (float)na;
}

// group i of [3, nx / 8): -1 if the source subtracts nothing for it, else the first group `a` of its range (which
// ends at bin 8 (i + 3), inclusive), with *thres what it subtracts.  temp: the means, 0 behind the last one.
// tone_off, noise_off: ntfix_noiseoffset[8 i], noiseoffset[1][8 i]  (lib/psy.c:3734-3756)
NTFIX_FN int ntfix_group_peak(const float *temp, const int i, const float tone_off, const float noise_off, const float limit,
                              float *thres_out)
{
    *thres_out = 0.f;
    if (!((temp[i] > temp[i - 1]) && (temp[i] > temp[i + 1]))) return -1;
    int a;
    float thres;
    if (temp[i - 1] > temp[i - 2]) {
        thres = temp[i - 2];
        a = i - 3;
    } else {
        thres = temp[i - 1];
        a = i - 2;
    }
    thres = temp[i] - thres;
    if (!((double)thres > 2.)) return -1;
    const float test = NTFIX_MIN(tone_off, noise_off + limit);
    *thres_out = NTFIX_MIN(thres - 2, test);
    return a;
}

// bin j after the subtractions of every peak whose range holds it, in ascending peak order; nx8 = nx / 8
NTFIX_FN float ntfix_trans_pull(float noise_j, const float *thres, const int *first, const int j, const int nx8)
{
    const int g = j >> 3;
    const int lo = NTFIX_MAX(g - 3, 3), hi = NTFIX_MIN(g + 3, nx8 - 1);
    for (int q = lo; q <= hi; q++) {
        const int a = first[q];
        if (a >= 0 && j >= 8 * a && j <= 8 * (q + 3)) noise_j -= thres[q];
    }
    return noise_j;
}
