// internal: kernel launchers (device code lives in mdct_kernel.hip)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// addressing of the envelope detector's 128-sample search windows inside the per-channel PCM buffers
// (frontend.h): block blk = channel * steps + t covers samples [64*j, 64*j + 128) of its channel with
// j = first[stream] + t0 + t, and exists while j < last[stream].  first == nullptr: plain block-major rows.
struct vbm_ve_gather {
    const float *pcm;       // buffer 0 of channel 0
    const int *first, *last, *parity;   // [S]
    const int *base;                    // [S] origin of the stream's samples inside its channel buffers
    int ch, steps, t0;
    long cap, plane;        // floats per channel buffer, floats per buffer set (all channels)
};

// A second way to name a block's first sample, beside the block-major rows pcm + blk * N: the long blocks of a
// device-built round's big batch are read where they lie in the front end's channel buffers (frontend.h).  Block
// blk = sb * ch + c (stream-block sb, channel c) starts at pcm + off[sb] + c * cap.  Every such address is 16-byte
// aligned (the loads are float4, as the gather's were): origins, window starts and cap are multiples of four floats.
struct vbm_block_src {
    const long long *off;   // [stream-blocks] float offset of channel 0's first sample (k_fe_round_commit writes it)
    const float *pcm;       // vbm_fe_state::pcm
    long cap;               // floats from a channel's buffer to the next channel's
    int ch;
};

extern "C" int vbm_launch_ve_mdct(const vbm_ve_gather *g, float *d_out, const float *d_trig, const float *d_win,
                                  long nblocks, hipStream_t stream);

extern "C" int vbm_launch_window_mdct(const float *d_pcm, float *d_out, const uint8_t *d_wflags,
                                      const float *d_trig, const float *d_win_self,
                                      const float *d_win_short, int n, int short_n,
                                      int apply_window, long nblocks, int max_workgroups,
                                      const int *d_live, int live_mult,   // NULL, or device count: *d_live * live_mult blocks exist
                                      const vbm_block_src *direct,        // NULL: rows of d_pcm; else d_pcm is unused (n == 2048)
                                      hipStream_t stream);

extern "C" int vbm_launch_window_fft_log(const float *d_pcm, float *d_logfft, float *d_local_ampmax,
                                         const uint8_t *d_wflags, const float *d_wa, const float *d_win_self,
                                         const float *d_win_short, int n, int short_n, long nblocks,
                                         const int *d_live, int live_mult, const vbm_block_src *direct, hipStream_t stream);
