// internal: launchers of the decode kernels (decode_kernels.hip), used by capi_decoder.cpp
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "decode.h"

enum { VBMD_SIZES = 5 };             // block sizes 256 .. 4096

// one header class of a mixed decoder (vbm_decoder_add_class): its setup and book blob in device memory
struct vbmd_class {
    const vbmd_setup *s;
    const uint8_t *blob;
};

// What the kernels of a mixed decoder (vbm_decoder_create_mixed) read in place of the one setup: each row's class, and
// the strides of the row buffers, which are those of the decoder's caps and not of any class.
struct vbmd_mixed {
    const vbmd_class *table;         // [max_classes], slots below the class count filled
    const int *rcls;                 // [nsb] class of each row of the call
    const int *scls;                 // [streams] class of each stream (-1: not bound)
    int CH;                          // channels of a row of every row buffer (max_channels)
    int cls_bytes;                   // partition-class scratch of a row
    long list_stride;                // entries of one block list: max_batch * CH
    const float *win[VBMD_SIZES];    // rising half-windows of 256 << z >> hs, by size index z
};

// device buffers of one decoder, as the kernels see them (rows: the current call's nsb)
struct vbmd_launch {
    const vbmd_setup *s;             // device copy of the setup, the book blob follows it (null in a mixed decoder)
    const uint8_t *blob;
    bool mx;                         // mixed decoder: M in place of s / blob / win0 / win1
    vbmd_mixed M;
    long nblocks;                    // rows x channels of this call, or a bound on them: sizes the IMDCT grids
    int nsb, ch;
    int hs;                          // 1: half-rate decoder (IMDCT, windows, overlap-add and PCM at half the sizes)
    long half, n1;                   // blocksizes[1]/2 (residue / spectrum rows), blocksizes[1] >> hs (IMDCT rows)
    long ohalf;                      // blocksizes[1]/2 >> hs (tail and PCM rows)
    int *info, *fit, *flags, *status, *lists, *counts;
    float *res, *spec, *imdct;
    uint8_t *cls;
    const float *fromdB, *win0, *win1;
    float *tail;                     // [streams][ch][ohalf]
    int *prevW;                      // [streams] -1: no block yet (pcm_returned == -1)
    long long *gp, *sc;              // [streams] granulepos, sample_count
};

int vbmd_launch_unpack(const vbmd_launch &L, const uint8_t *packets, long stride, const int *nbytes, int *status_out,
                       hipStream_t q);
int vbmd_launch_spectrum(const vbmd_launch &L, float *spec, int *findex, hipStream_t q);
// N: the transform size, blocksizes[W] >> hs (128 .. 4096), trig its table; W: the list, in a mixed decoder the size index
int vbmd_launch_imdct(const vbmd_launch &L, int W, int N, const float *trig, hipStream_t q);
int vbmd_launch_overlap(const vbmd_launch &L, const int *ids, const long long *granulepos, const uint8_t *eos,
                        float *pcm, int *samples, hipStream_t q);
// runs (vbm_synthesis_runs): CSR unpack; then plan, overlap-add into the runs' PCM and the tail commit.  runtab:
// stream ids [nruns] and run starts [nruns + 1]; plan: 6 ints per row; run_last: [nruns]; gap: null, or a mark per row
int vbmd_launch_unpack_csr(const vbmd_launch &L, const uint8_t *data, const long long *offsets, long long data_bytes,
                           int *status_out, hipStream_t q);
int vbmd_launch_runs(const vbmd_launch &L, int nruns, const int *runtab, const long long *granulepos,
                     const uint8_t *eos, const uint8_t *gap, int *plan, int *run_last, float *pcm, long pcm_stride,
                     int *run_samples, int *samples, hipStream_t q);
// ranges (vbm_synthesis_ranges): rtab is the piece table (k_range_rows in decode_kernels.hip); rows: [nsb] store
// packet of each row; pk_begin / pk_end / out_start: the store's index; runtab: one readable int per output row
// mixed: the pieces' classes [npieces] lie behind rtab, and rcls (L.M.rcls) gets the class of every row
int vbmd_launch_unpack_rows(const vbmd_launch &L, int npieces, const int *rtab, int *rows, int *rcls,
                            const uint8_t *data, const long long *offsets, long long data_bytes, hipStream_t q);
int vbmd_launch_ranges(const vbmd_launch &L, int npieces, const int *rtab, const int *rows, const int *pk_begin,
                       const int *pk_end, const long long *out_start, const int *runtab, int *plan, float *pcm,
                       long pcm_stride, hipStream_t q);
// cls / scls: null, or the new class of each stream and the stream -> class map it goes to
int vbmd_launch_restart(const int *ids, int n, int *prevW, long long *gp, long long *sc, const int *cls, int *scls,
                        hipStream_t q);
int vbmd_launch_used(const int *flags, int *out, long n, hipStream_t q);
