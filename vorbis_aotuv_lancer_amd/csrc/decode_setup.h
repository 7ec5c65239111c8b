// host-side decode setup (decode_setup.cpp) shared with the device decoder (capi_decoder.cpp)
#pragma once
#include <stdint.h>
#include <vector>
#include "decode.h"

struct vbm_decode_setup {
    vbmd_setup s;
    std::vector<uint8_t> blob;        // codebook tables (vbmd_book offsets)
    std::vector<float> fromdB;        // FLOOR1_fromdB_LOOKUP [256]
    std::vector<float> win[2];        // rising half-windows of blocksizes[0] and [1] (_vorbis_window_get)
    std::vector<float> hwin[2];       // ... of blocksizes[0] / 2 and [1] / 2, for half-rate decoders
};

// FLOOR1_fromdB_LOOKUP and the rising half-windows of n block sizes (win[i]: sizes[i] / 2 floats), from the package's
// common tables: what a setup carries for its own sizes, and a mixed decoder for every size its caps allow
int vbmd_common_tables(std::vector<float> *fromdB, int n, const int *sizes, std::vector<float> *const *win);

// The host index of one stream's n packets (CSR as vbm_synthesis_runs takes them, clamped to [0, data_bytes)), from a
// fresh stream state: per packet the status (vbmd_head) and, for valid packets, vbmd_blockin's [begin, end) (0, 0 for
// failed ones) and out_start, the exclusive prefix sum of end - begin; *total = the sum.  begin / end may be NULL.
// halfrate 1: the index of a half-rate decoder, in its output samples (vbmd_blockin<1>).
void vbmd_index_stream(const vbmd_setup &s, int halfrate, long long n, const uint8_t *data, const long long *offsets,
                       long long data_bytes, const long long *granulepos, const uint8_t *eos, int *status, int *begin,
                       int *end, long long *out_start, long long *total);

void vbmd_host_floor_index(const vbmd_setup &s, const vbmd_floor &f, const int *fit, int n, int *out);
