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
};

void vbmd_host_floor_index(const vbmd_setup &s, const vbmd_floor &f, const int *fit, int n, int *out);
