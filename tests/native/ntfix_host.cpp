// Host harness of tests/test_ntfix_parallel_cpu.py: aoTuV M7 as k_noisemask runs it
// (csrc/ntfix_parallel.h, the text the kernel compiles, driven bin by bin and group by group in the kernel's phases)
// beside a serial restatement of the source (lib/psy.c:3645-3768), for a bit-for-bit comparison.
#include <math.h>
#include <string.h>
#include "ntfix_parallel.h"

#define PAD 4

// ---- serial: the source's loops, on rows of n + PAD floats (the kernel's LDS rows are padded alike)
extern "C" void ntfix_serial(int block_mode, int n, int nx, const float *tone_off, const float *noise_off, const float *spectral,
                             float *noise)
{
    int i, j, k;
    const float limit = fabsf(noise_off[0]);
    float temp[256 + 8], inmod[256 + 8];
    if (!nx) return;
    memset(temp, 0, sizeof(temp));
    memset(inmod, 0, sizeof(inmod));
    if (block_mode <= 1) {
        const int freq_upc = 3, freq_unc = 4;
        int nxplus = nx + freq_unc;
        float tolerance = 9.f;
        const float strength = .6f;
        if (n == 256) tolerance = 15.f;
        if (nxplus > n) { nx = n; nxplus = n - freq_unc; }
        for (i = 0; i < nxplus; i++) {
            if (spectral[i] < -70) inmod[i] = (float)(-70 + (double)(spectral[i] + 70) * .1);
            else inmod[i] = spectral[i];
        }
        for (i = freq_unc; i < nx; i++) {
            if ((spectral[i] > spectral[i - 1]) && (spectral[i] > spectral[i + 1])) {
                int ps = i - 1, pe = i + 1;
                const int upper = i - freq_upc, under = i + freq_unc;
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
                if (ss > tolerance) {
                    if (spectral[i] > noise[i]) {
                        ss -= tolerance;
                        ss *= strength;
                    }
                    for (j = ps; j <= pe; j++) {
                        temp[j] = NTFIX_MAX(ss, temp[j]);
                        if (temp[j] < 0) temp[j] = 0;
                    }
                }
                i = pe;
            }
        }
        for (i = freq_unc - 1; i < nx; i++) {
            const float test = NTFIX_MIN(tone_off[i], noise_off[i] + limit);
            if (temp[i] > test) temp[i] = test;
            noise[i] -= temp[i];
        }
    } else if (block_mode == 2) {
        for (i = 0, k = 0; i < nx; i += 8, k++) {
            double na = 0;
            for (j = 0; j < 8; j++) na += noise[i + j];
            na /= 8;
            temp[k] = (float)na;
        }
        nx /= 8;
        for (i = 3; i < nx; i++) {
            if ((temp[i] > temp[i - 1]) && (temp[i] > temp[i + 1])) {
                int a = 0, bb = 0;
                float thres = 0;
                if (temp[i - 1] > temp[i - 2]) {
                    thres = temp[i - 2];
                    a = i - 3;
                } else {
                    thres = temp[i - 1];
                    a = i - 2;
                }
                bb = i + 3;
                thres = temp[i] - thres;
                if ((double)thres > 2.) {
                    const int eightimes = i * 8;
                    const float test = NTFIX_MIN(tone_off[eightimes], noise_off[eightimes] + limit);
                    thres = NTFIX_MIN(thres - 2, test);
                    a *= 8;
                    bb *= 8;
                    for (j = a; j <= bb; j++) noise[j] -= thres;
                }
            }
        }
    }
}

// ---- the kernel's phases (noise_kernels.hip, "aoTuV M7"): every loop below is a set of independent threads there, and
//      a new loop starts where the kernel has a barrier.  counts (may be 0): [0] peaks stamped, [1] bins covered by two
//      peaks with different ss, [2] bins whose temp the clamp lowers; transition: [0] peaks, [1] bins two peaks reach
extern "C" void ntfix_parallel(int block_mode, int n, int nx, const float *tone_off, const float *noise_off, const float *spectral,
                               float *noise, int *counts)
{
    const int NS = n + PAD;
    const float limit = fabsf(noise_off[0]);
    static float r1[4096 + PAD], r2[4096 + PAD];
    static int r3[4096 + PAD];
    int c[3] = {0, 0, 0};
    if (!nx) return;
    (void)NS;
    if (block_mode <= 1) {
        int nxplus = nx + NTFIX_FREQ_UNC;
        if (nxplus > n) { nx = n; nxplus = n - NTFIX_FREQ_UNC; }
        const float tolerance = ntfix_short_tolerance(n);
        for (int i = 0; i < n; i++) r1[i] = ntfix_inmod(spectral[i], i, nxplus);
        for (int i = NTFIX_FREQ_UNC; i < nx; i++) {
            int down, up;
            r2[i] = ntfix_short_peak(spectral, r1, noise[i], i, tolerance, &down, &up);
            r3[i] = ntfix_reach_pack(down, up);
            c[0] += r2[i] > 0;
        }
        for (int i = NTFIX_FREQ_UNC - 1; i < nx; i++) {
            const float temp = ntfix_short_temp(r2, r3, i, nx);
            int cover = 0, differ = 0;
            for (int q = NTFIX_MAX(i - 3, NTFIX_FREQ_UNC); q <= NTFIX_MIN(i + 3, nx - 1); q++)
                if (r2[q] > 0 && i >= q - (r3[q] & 15) && i <= q + (r3[q] >> 4)) { cover++; differ |= r2[q] != temp; }
            c[1] += cover >= 2 && differ;
            c[2] += temp > NTFIX_MIN(tone_off[i], noise_off[i] + limit);
            noise[i] = ntfix_short_apply(noise[i], temp, tone_off[i], noise_off[i], limit);
        }
    } else if (block_mode == 2) {
        const int ngr = (nx + 7) >> 3, nx8 = nx >> 3;
        for (int k = 0; k <= nx8; k++) r1[k] = (k < ngr) ? ntfix_group_mean(noise + 8 * k) : 0.f;
        for (int k = 3; k < nx8; k++) {
            r3[k] = ntfix_group_peak(r1, k, tone_off[8 * k], noise_off[8 * k], limit, &r2[k]);
            c[0] += r3[k] >= 0;
        }
        for (int i = 0; i < n; i++) {
            int cover = 0;
            for (int q = NTFIX_MAX((i >> 3) - 3, 3); q <= NTFIX_MIN((i >> 3) + 3, nx8 - 1); q++)
                cover += r3[q] >= 0 && i >= 8 * r3[q] && i <= 8 * (q + 3);
            c[1] += cover >= 2;
            noise[i] = ntfix_trans_pull(noise[i], r2, r3, i, nx8);
        }
    }
    if (counts) for (int k = 0; k < 3; k++) counts[k] += c[k];
}
