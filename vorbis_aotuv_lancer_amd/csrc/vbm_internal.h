// internal helpers shared by the host-side translation units
#pragma once
#include <hip/hip_runtime.h>
#include <string>

extern thread_local std::string g_vbm_err;
int vbm_set_hip_error(hipError_t e, const char *where);

// what the translation units use of each other's objects
struct vbm_setup_handle;
struct vbm_setup_host;
struct vbm_encoder;
vbm_setup_host *vbm_setup_handle_host(vbm_setup_handle *h);        // capi_setup.cpp
vbm_setup_host *vbm_encoder_setup_host(vbm_encoder *e);            // capi_encoder.cpp, for the stream front end
int vbm_encoder_streams(const vbm_encoder *e);
int vbm_encoder_workspaces(const vbm_encoder *e);
int vbm_encoder_reset_streams_dev(vbm_encoder *e, const int *d_ids, int n, hipStream_t q);
struct vbm_block_src;                                              // mdct_kernel.h
int vbm_encoder_device_round_open(vbm_encoder *e, hipStream_t fork, int *w_out, int **d_stream_id, uint8_t **d_wflags,
                                  long long **d_src, int *lanes, int **d_counts);
bool vbm_encoder_device_round_direct(const vbm_encoder *e);        // the next first round's long blocks need no gather
int vbm_encoder_device_round_run(vbm_encoder *e, int w, const int *lane0, const int *cap, const int *d_count,
                                 const float *d_blocks, const vbm_block_src *big_direct, uint8_t *d_packets,
                                 int *d_packet_bytes, bool first_round, hipStream_t fork);
struct vbm_range_store;
struct vbm_range_store_view {          // a range store's index and device arrays, for ogg_cut.hip
    int S, halfrate;
    long long packets, data_bytes;
    const long long *first, *out_end, *totals;   // host: [S + 1], [P], [S]
    const long long *last;                       // host: [S] the end of each stream's packets: first + 1, or a live
                                                 // store's, whose streams do not end where the next begins
    const long long *lo;                         // host: [S] a live store's first retained samples, else null
    int host;                                    // a host twin's store (vbm_host_live_store_create): no device array
    const int *status;                           // host: [P]
    const uint8_t *d_data;
    const long long *d_offsets, *d_out_start;    // device: [P + 1], [P]
    const int *d_begin, *d_end;                  // device: [P]
};
void vbm_range_store_get_view(const vbm_range_store *st, vbm_range_store_view *v);   // capi_decoder.cpp
extern "C" void vbm_debug_stamp(hipStream_t st, int tag);          // util_kernels.hip (timing experiments, VBM_DEBUG_STAMPS)

// test instrumentation (debug_hooks.hip): a spin kernel on `q` when `point` is in the mask of vbm_debug_set_delay
enum vbm_delay_point {
    VBM_DP_JOB_BIG = 0,        // host-built round: before the first kernel of a big batch (its own front stream)
    VBM_DP_JOB_SMALL = 1,      // ... of a small batch (stream of its block type)
    VBM_DP_JOB_STATE = 2,      // before the first kernel of a batch that touches the carried stream state
    VBM_DP_JOB_BACK = 3,       // before a batch's back half (floor fit .. packets)
    VBM_DP_JOB_OUT = 4,        // before a batch's outputs are copied to the caller's buffers
    VBM_DP_FE_FORK = 5,        // front end: between the gathers of a round and the round's fork
    VBM_DP_FE_SHIFT = 6,       // front end: before the buffer shift of a round
    VBM_DP_DEV_BIG_FRONT = 7,  // device-built round: before the big batch's psychoacoustics graph, behind its state waits
    VBM_DP_DEV_BIG_BACK = 8,   // ... back-half graph
    VBM_DP_DEV_SMALL_FRONT = 9,
    VBM_DP_DEV_SMALL_BACK = 10,
    VBM_DP_DEV_PLAN = 11,      // front end: before a device-built round is planned
    VBM_DP_BATCH_FRONT = 12,   // vbm_analysis_batch2: before the front half
    VBM_DP_BATCH_BACK = 13,    // ... the back half
    VBM_DP_FE_WRITE = 14,      // front end: before the append of a write
    VBM_DP_DEV_OUT = 15,       // device-built round: before a batch's output copy
    VBM_DP_DEV_BIG_TRANSFORMS = 16,    // device-built round: before the big batch's transforms graph (ahead of its state waits)
    VBM_DP_DEV_SMALL_TRANSFORMS = 17,  // ... a small batch's
};
void vbm_debug_delay_point(int point, hipStream_t q);
